"""./spiral ... --device-client --output-err FILE: the session measures the error of the run's answer against the true item (include/spiral_gpu.h
spiral_gpu_client_response_noise).  The printed variance is recomputed from the file the run appended, the budget line is checked against its
own radius, and the run's own check (`Is correct?`) stays in place."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spiral_amd", "spiral")


@pytest.fixture(scope="module")
def sa():
    import torch

    torch.cuda.is_available()
    import spiral_amd

    assert spiral_amd.lib().spiral_gpu_device_count() > 0, "GPU tests need a device"
    return spiral_amd


@pytest.mark.parametrize("args,rows", [(["4", "3", "5", "a"], 2), (["4", "3", "5", "a", "--seeded"], 2), (["6", "2", "5", "a", "--high-rate"], 2)],
                         ids=["base", "base-seeded", "high-rate"])
def test_cli_output_err(sa, tmp_path, args, rows):
    f = tmp_path / "err.txt"
    f.write_text("7 ")  # the run appends, as the reference's output_diffs does
    r = subprocess.run([BIN] + args + ["--seed", "77", "--device-client", "--output-err", str(f)], capture_output=True, text=True, timeout=600)
    out = r.stdout
    assert r.returncode == 0, out[-2000:] + r.stderr[-2000:]
    assert re.search(r"Is correct\s?\?\s?: 1\n", out), out
    m = re.search(r"^variance of diff w/o modswitching: 2\^(-?[0-9.]+)$", out, re.M)
    assert m, out
    vals = [int(x) for x in f.read_text().split()]
    assert vals[0] == 7 and len(vals) == 1 + rows * rows * 2048
    e = np.array(vals[1:], dtype=np.float64)
    scale = 268369921 * 249561089 // 256
    assert np.abs(e).max() < scale / 2, "the run decoded, so every unswitched error lies inside the radius"
    # printed to four decimals from the exact sums; np.var in double carries about 1e-13 relative
    assert abs(float(m.group(1)) - math.log2(np.var(e))) < 1e-3, (m.group(1), math.log2(np.var(e)))
    b = re.search(r"^noise budget: ([0-9.]+) of ([0-9.]+) bits$", out, re.M)
    assert b, out
    q = sa.get_pack_shape(sa.make_params(6, 2), 2).qprime if "--high-rate" in args else sa.get_shape(sa.make_params(4, 3)).qprime
    assert abs(float(b.group(2)) - math.log2(2 * q)) < 1e-3 and 0 < float(b.group(1)) <= float(b.group(2))


def test_cli_output_err_needs_a_one_query_device_client_run(sa, tmp_path):
    """without --device-client the flag names it, and the file is not written; with --device-client on a batch run the flag is refused"""
    f = tmp_path / "err.txt"
    r = subprocess.run([BIN, "4", "3", "5", "a", "--seed", "77", "--output-err", str(f)], capture_output=True, text=True, timeout=600)
    assert "--device-client" in r.stdout + r.stderr and not f.exists()
    assert "variance of diff" not in r.stdout and "noise budget" not in r.stdout
    for extra in (["--batch", "2"], ["--instances", "2"], ["--batch", "2", "--key-store"], ["--batch", "2", "--query-batch"]):
        r = subprocess.run([BIN, "4", "3", "5", "a", "--seed", "77", "--device-client", "--output-err", str(f)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "--output-err takes --device-client on a one-query run" in r.stderr, extra
        assert not f.exists()


def test_cli_output_without_the_flag_is_unchanged(sa):
    """no new line appears without the flag"""
    r = subprocess.run([BIN, "4", "3", "5", "a", "--seed", "77", "--device-client"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "variance of diff" not in r.stdout and "noise budget" not in r.stdout and "output-err" not in r.stdout
