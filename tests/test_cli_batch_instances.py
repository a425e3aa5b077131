"""./spiral --batch B --instances F: B clients, each with its own keys and index, fetch an item of F plaintexts in one
spiral_gpu_server_answer_batch_instances call; every plaintext of every client is decoded from its wire form and checked."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spiral_amd", "spiral")


@pytest.mark.gpu
@pytest.mark.parametrize("args,env", [
    (["4", "3", "40", "a", "--seed", "21", "--batch", "3", "--instances", "3"], {}),
    (["5", "2", "7", "a", "--direct-upload", "--seed", "22", "--batch", "3", "--instances", "3"], {"TEXP": "2", "TGSW": "5", "QPBITS": "19"}),
])
def test_cli_batch_of_items(args, env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([BIN] + args, capture_output=True, text=True, env=e, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert re.search(r"\s+Is correct\?: 1\n", r.stdout), r.stdout
    m = re.search(r"Batch of 3 items of 3 plaintexts, Is correct\?: ([01 ]+)", r.stdout)
    assert m and m.group(1).split() == ["1", "1", "1"], r.stdout
    assert re.search(r"Batch of 3 items of 3 plaintexts \(3 clients, 3 database instances\), device \(GPU·us\): [0-9]+", r.stdout), r.stdout
