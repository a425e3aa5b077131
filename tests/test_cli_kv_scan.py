"""./spiral nu1 nu2 K a --kv-value-bytes V --device-client [--high-rate] --kv-scan (OUTN = 2): after the keyed run's own steps the whole table is
listed with values, reconciled against the keys the run stored -- the key written by kv_put included -- and every held value is compared with the
generator.  The number of entries is computed here from the restatement (tests/test_cli_kv.py loaded).  Without the flag the run prints no Scan: line;
the flag without --kv-value-bytes is refused by name."""
import os
import re
import subprocess

import pytest

import kv_restated as K
import pack_kv_restated as PK
from test_cli_kv import BIN, loaded, run

RUNS = [  # name, arguments, the layout, key number
    ("base-32-V248", ["3", "2", "5", "a", "--seed", "41", "--kv-value-bytes", "248", "--device-client", "--kv-scan"], K.layout(256, 3, 2, 248), 5),
    ("pack-42-V3000", ["4", "2", "5", "a", "--seed", "43", "--high-rate", "--kv-value-bytes", "3000", "--device-client", "--kv-scan"], PK.layout(256, 4, 2, 2, 3000), 5),
    ("base-32-beyond", ["3", "2", "600", "a", "--seed", "44", "--kv-value-bytes", "248", "--device-client", "--kv-scan"], K.layout(256, 3, 2, 248), 600),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,args,lay,key_no", RUNS, ids=[r[0] for r in RUNS])
def test_cli_kv_scan_run(name, args, lay, key_no):
    n = loaded(lay)
    entries = n + (0 if key_no < n else 1)  # (the put of a key beyond the loaded ones adds an entry)
    r = run(args)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"Scan: {entries} entries, missing: 0, orphans: 0, values correct: 1\nIs correct?: 1\n" in r.stdout, r.stdout[-2000:]
    assert re.search(rf"Table load \(kv_stats\): {entries} of ", r.stdout), r.stdout[-2000:]
    # without the flag: the same run, no Scan: line, every other line as it is
    plain = run([a for a in args if a != "--kv-scan"])
    assert plain.returncode == 0 and "Scan:" not in plain.stdout and "Is correct?: 1\n" in plain.stdout, plain.stdout[-2000:] + plain.stderr[-2000:]
    assert len(r.stdout.splitlines()) == len(plain.stdout.splitlines()) + 1, "the flag adds the Scan: line and nothing else"


def test_cli_kv_scan_needs_a_keyed_run():
    """refused by name before anything touches a device"""
    import spiral_amd

    spiral_amd.build()
    for args in (["3", "2", "5", "a", "--kv-scan"], ["3", "2", "5", "a", "--device-client", "--kv-scan"], ["4", "2", "5", "a", "--high-rate", "--kv-scan"]):
        r = subprocess.run([BIN] + args, capture_output=True, text=True, timeout=600, env=dict(os.environ, OUTN="2"))
        assert r.returncode == 1 and "--kv-scan takes --kv-value-bytes" in r.stderr, r.stdout[-1000:] + r.stderr[-1000:]
        assert "Is correct?" not in r.stdout
