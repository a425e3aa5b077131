"""./spiral nu1 nu2 R a --record-bytes S [--device-client]: the database filled through load_records from the counter-based byte generator, record R
fetched by one query and decoded (decode_records on a client session, or packed and cut on the host), replaced through update_records, fetched and
decoded again; both results checked against the generator.  And the flags it does not go with, refused by name."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spiral_amd", "spiral")


def run(args):
    return subprocess.run([BIN] + args, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
@pytest.mark.parametrize("args,layout", [
    (["4", "3", "1000", "a", "--seed", "31", "--record-bytes", "256"], "32 per item of 8192 bytes, 1 instance"),
    (["4", "3", "100", "a", "--seed", "32", "--record-bytes", "20000"], "1 per item of 8192 bytes, 3 instance"),
    (["4", "3", "4095", "a", "--seed", "33", "--record-bytes", "256", "--device-client"], "32 per item of 8192 bytes, 1 instance"),
    (["4", "3", "127", "a", "--seed", "34", "--record-bytes", "20000", "--device-client"], "1 per item of 8192 bytes, 3 instance"),
], ids=["S256", "S20000", "S256-device-client", "S20000-device-client"])
def test_cli_record_run(args, layout):
    r = run(args)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert layout in r.stdout, r.stdout
    assert re.search(r"Record \d+ as loaded, correct: 1\n", r.stdout), r.stdout
    assert re.search(r"Record \d+ after update_records, correct: 1\n", r.stdout), r.stdout
    assert re.search(r"\nIs correct\?: 1\n", r.stdout), r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [["--high-rate"], ["--batch", "2"], ["--instances", "2"], ["--batch", "2", "--key-store"], ["--batch", "2", "--query-batch"]],
                         ids=["high-rate", "batch", "instances", "key-store", "query-batch"])
def test_cli_record_refusals(extra):
    r = run(["4", "3", "5", "a", "--record-bytes", "256"] + extra)
    assert r.returncode == 1, r.stdout[-2000:] + r.stderr[-2000:]
    assert "--record-bytes does not go with " + extra[-1 if extra[-1].startswith("--") else 0] in r.stderr, r.stderr
    assert "Is correct?" not in r.stdout


@pytest.mark.gpu
def test_cli_record_out_of_range():
    r = run(["4", "3", "4096", "a", "--record-bytes", "256"])
    assert r.returncode == 1 and "record 4096 out of range (4096 records of 256 bytes)" in r.stderr, r.stdout[-1000:] + r.stderr[-1000:]
    r = run(["4", "3", "0", "a", "--record-bytes", str(17 * 8192)])
    assert r.returncode == 1 and "at most 16" in r.stderr, r.stdout[-1000:] + r.stderr[-1000:]


@pytest.mark.gpu
def test_cli_record_bytes_zero_is_refused():
    for tail in (["--record-bytes", "0"], ["--record-bytes"]):
        r = run(["4", "3", "5", "a"] + tail)
        assert r.returncode == 1 and "--record-bytes takes a record size of at least 1 byte" in r.stderr, r.stdout[-1000:] + r.stderr[-1000:]
        assert "Is correct?" not in r.stdout
