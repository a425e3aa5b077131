"""./spiral nu1 nu2 K a --kv-value-bytes V --device-client [--high-rate] (OUTN = 2): a keyed table loaded by kv_load from the key set "key-%08d" and the
record runs' byte generator, key number K looked up privately (kv_queries, two answers, kv_decode), overwritten or inserted by kv_put and looked up
again, one absent key looked up, and the table's load from kv_stats.  How many keys the run loads -- half of the capacity, or the longest prefix of the
key set the placement rule accepts -- is computed here from the restatement (tests/kv_restated.py, tests/pack_kv_restated.py).  And the flags the run
does not go with, refused by name."""
import os
import re
import subprocess

import numpy as np
import pytest

import kv_restated as K
import pack_kv_restated as PK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spiral_amd", "spiral")
TK = bytes(range(16))  # the run's table key


def run(args):
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=600, env=dict(os.environ, OUTN="2"))


def loaded(lay) -> int:
    """the keys the run loads: half of the capacity, or the longest prefix of key_set that the restated rule places"""
    half = lay.capacity // 2
    _, b1, b2 = K.kv_hash_many(lay.buckets, TK, K.key_array(K.key_set(half)))
    try:
        K.place_fresh(lay.buckets, lay.slots, b1, b2)
        return half
    except K.Full as e:
        return e.position


RUNS = [  # name, arguments, the layout, key number
    ("base-32-V248", ["3", "2", "77", "a", "--seed", "41", "--kv-value-bytes", "248", "--device-client"], K.layout(256, 3, 2, 248), 77),
    ("pack-42-V248", ["4", "2", "1000", "a", "--seed", "42", "--kv-value-bytes", "248", "--device-client", "--high-rate"], PK.layout(256, 4, 2, 2, 248), 1000),
    ("pack-42-V3000", ["4", "2", "31", "a", "--seed", "43", "--kv-value-bytes", "3000", "--device-client", "--high-rate"], PK.layout(256, 4, 2, 2, 3000), 31),
    ("base-32-beyond", ["3", "2", "600", "a", "--seed", "44", "--kv-value-bytes", "248", "--device-client"], K.layout(256, 3, 2, 248), 600),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,args,lay,key_no", RUNS, ids=[r[0] for r in RUNS])
def test_cli_kv_run(name, args, lay, key_no):
    n = loaded(lay)
    assert (n == lay.capacity // 2) == (lay.slots > 2), "the 2-slot table overflows before half of its capacity; the others take it"
    present = key_no < n
    assert present == (name != "base-32-beyond")
    r = run(args)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"{lay.slots} slots per bucket of {lay.item_bytes} bytes, {lay.buckets} buckets, capacity {lay.capacity}\n" in r.stdout, r.stdout
    assert f"done loading/generating db: {n} keys (half of the capacity: {lay.capacity // 2})\n" in r.stdout, r.stdout
    key = "key-%08d" % key_no
    m = re.search(rf"Key {key} as loaded, found: (\d), correct: 1\n", r.stdout)
    assert m and (int(m.group(1)) in (1, 2)) == present, r.stdout
    assert re.search(rf"Key {key} after kv_put, found: [12], correct: 1\n", r.stdout), r.stdout
    assert "Absent key, found: 0\n" in r.stdout, r.stdout
    used = n + (0 if present else 1)
    m = re.search(r"Table load \(kv_stats\): (\d+) of (\d+) slots used, load ([0-9.e-]+), fullest bucket (\d+) of (\d+), full buckets (\d+)\n", r.stdout)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(5))) == (used, lay.capacity, lay.slots), r.stdout
    assert abs(float(m.group(3)) - used / lay.capacity) < 1e-4 and 1 <= int(m.group(4)) <= lay.slots
    assert re.search(r"\nIs correct\?: 1\n", r.stdout), r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [["--batch", "2"], ["--instances", "2"], ["--record-bytes", "256"], ["--high-rate", "--pack-record-bytes", "256"]],
                         ids=["batch", "instances", "record-bytes", "pack-record-bytes"])
def test_cli_kv_refusals(extra):
    r = run(["4", "2", "5", "a", "--kv-value-bytes", "248", "--device-client"] + extra)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]
    flag = [x for x in extra if x.startswith("--") and x != "--high-rate"][0]
    assert "--kv-value-bytes does not go with " + flag in r.stderr, r.stderr
    assert "Is correct?" not in r.stdout


@pytest.mark.gpu
def test_cli_kv_needs_the_device_client_and_a_value_size():
    r = run(["3", "2", "5", "a", "--kv-value-bytes", "248"])
    assert r.returncode == 1 and "--kv-value-bytes takes --device-client" in r.stderr, r.stdout[-1000:] + r.stderr[-1000:]
    for tail in (["--kv-value-bytes", "0"], ["--kv-value-bytes"]):
        r = run(["3", "2", "5", "a", "--device-client"] + tail)
        assert r.returncode == 1 and "--kv-value-bytes takes a value size of at least 1 byte" in r.stderr, r.stdout[-1000:] + r.stderr[-1000:]
    r = run(["3", "2", "5", "a", "--device-client", "--kv-value-bytes", "9000"])
    assert r.returncode == 1 and "slots = 0" in r.stderr, r.stdout[-1000:] + r.stderr[-1000:]
    assert "Is correct?" not in r.stdout
