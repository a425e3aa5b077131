"""./spiral ... --wire-input: the client sends its public parameters and queries in their 7-byte wire form (spiral_gpu_raw_to_wire of the raw form)
and the server ingests them through the wire entry points; every answer decodes, and the bytes uploaded are printed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spiral_amd", "spiral")
DIRECT = {"TEXP": "2", "TGSW": "5", "QPBITS": "19"}


def summary(out, name):
    m = re.search(name + r" \(b\): (\d+)", out)
    return int(m.group(1)) if m else None


@pytest.mark.gpu
@pytest.mark.parametrize("args,env", [
    (["4", "3", "40", "a", "--seed", "31"], {}),
    (["5", "2", "7", "a", "--direct-upload", "--seed", "32"], DIRECT),
    (["4", "3", "40", "a", "--seed", "33", "--batch", "3"], {}),
    (["4", "3", "40", "a", "--seed", "34", "--instances", "3"], {}),
    (["4", "3", "40", "a", "--seed", "35", "--batch", "3", "--instances", "3"], {}),
    (["5", "2", "7", "a", "--direct-upload", "--seed", "36", "--batch", "3", "--instances", "3"], DIRECT),
    (["6", "2", "9", "a", "--high-rate", "--seed", "37"], {}),
    (["6", "2", "9", "a", "--high-rate", "--seed", "38", "--batch", "3"], {}),
], ids=["base", "direct-upload", "batch", "instances", "batch-instances", "direct-batch-instances", "high-rate", "high-rate-batch"])
def test_cli_wire_input(args, env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([BIN] + args + ["--wire-input"], capture_output=True, text=True, env=e, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert re.search(r"Is correct\s?\?\s?: 1\n", out), out
    for m in re.finditer(r"Is correct\?:((?: [01])+)", out):
        assert set(m.group(1).split()) == {"1"}, out
    m = re.search(r"Wire input, uploaded offline / online \(b\): (\d+) / (\d+)", out)
    assert m, out
    offline, online = int(m.group(1)), int(m.group(2))
    if "--high-rate" not in args:
        # the summary's online figure counts n_query_cts ciphertexts of two polynomials at 56 bits per coefficient: exactly what went up.  Its
        # offline figure leaves out V on direct-upload geometries (client.cpp gen_pub_params), which the server still takes.
        assert online == summary(out, "Total online query size"), out
        if "--direct-upload" not in args:
            assert offline == summary(out, "Total offline query size"), out
    else:
        assert offline == summary(out, "Total offline query size"), out
