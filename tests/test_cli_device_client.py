"""./spiral ... --device-client: keys, queries and decoding through client sessions on the device (include/spiral_gpu.h spiral_gpu_client_*), one per
client of a --batch, combined with the flags that choose the messages' form and the server path.  The check is the command line's own: every decoded
plaintext is compared with the seeded database's item (`Is correct?`), so a wrong key, query or decode fails it; the summary lines stay in place."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spiral_amd", "spiral")


@pytest.fixture(scope="module")
def sa():
    # torch first: it ships its own HIP runtime and the two must not be initialised in the opposite order (this file runs first in the suite)
    import torch

    torch.cuda.is_available()
    import spiral_amd

    assert spiral_amd.lib().spiral_gpu_device_count() > 0, "GPU tests need a device"
    return spiral_amd


@pytest.mark.parametrize("args", [
    ["4", "3", "5", "a"],
    ["4", "3", "5", "a", "--batch", "3", "--query-batch", "--seeded", "--key-store", "compact"],
    ["6", "2", "5", "a", "--high-rate"],
    ["4", "3", "5", "a", "--nonoise", "--wire-input", "--instances", "2"],
    ["4", "3", "40", "a", "--batch", "2", "--key-store"],
    ["5", "2", "7", "a", "--direct-upload", "--seeded", "--batch", "2", "--instances", "2"],
    ["6", "2", "9", "a", "--high-rate", "--seeded", "--batch", "2"],
], ids=["base", "batch-query-batch-seeded-key-store", "high-rate", "nonoise-wire-instances", "batch-key-store-ntt", "direct-seeded-item-batch", "high-rate-seeded-batch"])
def test_cli_device_client(sa, args):
    e = dict(os.environ)
    if "--direct-upload" in args:
        e.update({"TEXP": "2", "TGSW": "5", "QPBITS": "19"})
    r = subprocess.run([BIN] + args + ["--seed", "77", "--device-client"], capture_output=True, text=True, env=e, timeout=600)
    out = r.stdout
    assert r.returncode == 0, out[-2000:] + r.stderr[-2000:]
    assert "Using client sessions on the device" in out
    assert re.search(r"Is correct\s?\?\s?: 1\n", out), out
    checks = 0
    for m in re.finditer(r"Is correct\?:((?: [01])+)", out):
        assert set(m.group(1).split()) == {"1"}, out
        checks += len(m.group(1).split())
    if "--batch" in args:  # every client of the batch was decoded and checked
        assert checks >= int(args[args.index("--batch") + 1]), out
    for line in ("Key generation (CPU·us):", "Query generation (CPU·us):", "Decoding (CPU·us):", "Total offline query size (b):"):
        assert line in out, line


def test_offline_size_is_the_host_clients(sa):
    """the summary's offline query size does not depend on which client made the keys"""
    size = lambda extra: int(re.search(r"Total offline query size \(b\): (\d+)", subprocess.run(  # noqa: E731
        [BIN, "4", "3", "5", "a", "--seed", "3"] + extra, capture_output=True, text=True, timeout=600, check=True).stdout).group(1))
    assert size(["--device-client"]) == size([])
