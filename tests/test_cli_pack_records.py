"""./spiral nu1 nu2 R a --high-rate --pack-record-bytes S [--device-client] with OUTN = 2: SpiralPack servers filled through load_records from the
counter-based byte generator, record R fetched by one query and decoded (decode_records on a client session, or packed in trial order and cut on the
host), replaced through update_records, fetched and decoded again; both results checked against the generator."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spiral_amd", "spiral")


def run(args):
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=600, env=dict(os.environ, OUTN="2"))


@pytest.mark.gpu
@pytest.mark.parametrize("args,layout", [
    (["4", "2", "1000", "a", "--seed", "31", "--high-rate", "--pack-record-bytes", "256"], "32 per item of 8192 bytes, 1 instance"),
    (["4", "2", "50", "a", "--seed", "32", "--high-rate", "--pack-record-bytes", "20000"], "1 per item of 8192 bytes, 3 instance"),
    (["4", "2", "2047", "a", "--seed", "33", "--high-rate", "--pack-record-bytes", "256", "--device-client"], "32 per item of 8192 bytes, 1 instance"),
    (["4", "2", "63", "a", "--seed", "34", "--high-rate", "--pack-record-bytes", "20000", "--device-client"], "1 per item of 8192 bytes, 3 instance"),
], ids=["S256", "S20000", "S256-device-client", "S20000-device-client"])
def test_cli_pack_record_run(args, layout):
    r = run(args)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Using n=2" in r.stdout, r.stdout
    assert layout in r.stdout, r.stdout
    assert re.search(r"Record \d+ as loaded, correct: 1\n", r.stdout), r.stdout
    assert re.search(r"Record \d+ after update_records, correct: 1\n", r.stdout), r.stdout
    assert re.search(r"\nIs correct\?: 1\n", r.stdout), r.stdout


@pytest.mark.gpu
def test_cli_pack_record_refusals():
    r = run(["4", "2", "5", "a", "--pack-record-bytes", "256"])
    assert r.returncode == 1 and "--pack-record-bytes takes --high-rate" in r.stderr, r.stdout[-1000:] + r.stderr[-1000:]
    r = run(["4", "2", "5", "a", "--high-rate", "--pack-record-bytes", "0"])
    assert r.returncode == 1 and "--pack-record-bytes takes a record size of at least 1 byte" in r.stderr, r.stdout[-1000:] + r.stderr[-1000:]
    r = run(["4", "2", "5", "a", "--high-rate", "--pack-record-bytes", "256", "--batch", "2"])
    assert r.returncode == 1 and "--pack-record-bytes does not go with --batch" in r.stderr, r.stdout[-1000:] + r.stderr[-1000:]
    r = run(["4", "2", "2048", "a", "--high-rate", "--pack-record-bytes", "256"])
    assert r.returncode == 1 and "record 2048 out of range (2048 records of 256 bytes)" in r.stderr, r.stdout[-1000:] + r.stderr[-1000:]
    r = run(["4", "2", "5", "a", "--record-bytes", "256", "--high-rate"])  # the base records run with --high-rate stays refused by name
    assert r.returncode == 1 and "--record-bytes does not go with --high-rate" in r.stderr, r.stderr
