"""./spiral --batch B --query-batch: after the batch, every client's fresh query goes in through one spiral_gpu_server_set_query_batch call and
every response comes back through one spiral_gpu_server_read_response_wire_batch; each client decodes its own item.  The command line's own
client makes valid seeded encryptions (row 0 from its seed), so --seeded checks the seeded form end to end."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spiral_amd", "spiral")


@pytest.mark.gpu
@pytest.mark.parametrize("B,extra,form,who", [
    (3, ["--seeded"], "seeded", lambda b, B: b),
    (8, ["--key-store"], "wire", lambda b, B: (b + 2) % B),  # (keys bound from the store first: lane b serves the client two lanes on)
], ids=["seeded", "key-store"])
def test_cli_query_batch(B, extra, form, who):
    r = subprocess.run([BIN, "4", "3", "40", "a", "--seed", "9", "--batch", str(B), "--query-batch"] + extra, capture_output=True, text=True,
                       env=dict(os.environ, TGSW="4"), timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = re.findall(r"Query batch, client (\d) on lane (\d), Is correct\?: (\d)", r.stdout)
    assert len(got) == B and all(ok == "1" for *_, ok in got), r.stdout
    assert [(int(c), int(b)) for c, b, _ in got] == [(who(b, B), b) for b in range(B)]
    assert re.search(rf"The batch's {B} queries went in as one set_query_batch call \({form} form, \d+ bytes each\)", r.stdout), r.stdout
    m = re.search(rf"Batch of {B} queries, Is correct\?:([01 ]+)", r.stdout)
    assert m and m.group(1).split() == ["1"] * B, r.stdout


@pytest.mark.gpu
def test_cli_query_batch_refused_with_high_rate():
    r = subprocess.run([BIN, "4", "3", "40", "a", "--high-rate", "--batch", "3", "--query-batch"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--query-batch takes --batch B in 2 .. 8" in r.stderr, r.stdout + r.stderr
