"""SpiralPack batches on trial-sharded servers, without a device: the layout helpers of spiral_amd/dist.py (pack_trial_cuts, pack_batch_block_cts,
pack_batch_position) against a numpy model, the list and null-argument checks of the C entry points (the cases tests/test_lanes_cpu.py runs on the
calls of its table), and the one collective on CPU tensors (gloo, world size 2)."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CT = 2 * 2048


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


def test_layout_helpers_match_a_numpy_model():
    """every (world <= 16, trials in {4, 9, 16, 144}, n <= 8): the cuts are consecutive, non-empty and cover the trials; a gathered buffer filled at
    pack_batch_position from the model's [rank][lane][k] blocks holds every (lane, trial) exactly once, inside its rank's block, and the rest is padding"""
    from spiral_amd import dist as D

    assert D.PACK_CT_WORDS == CT
    for trials in (4, 9, 16, 144):
        for world in range(1, 17):
            if world > trials:
                with pytest.raises(ValueError):
                    D.pack_trial_cuts(world, trials)
                continue
            cuts = D.pack_trial_cuts(world, trials)
            model = np.floor(np.arange(world + 1) * trials / world + 1e-9).astype(np.int64)  # an even split, the remainder spread out
            assert cuts == model.tolist() and cuts[0] == 0 and cuts[-1] == trials and len(cuts) == world + 1
            lens = np.diff(cuts)
            assert lens.min() >= 1 and lens.max() - lens.min() <= 1
            for n in range(1, 9):
                block = D.pack_batch_block_cts(n, cuts)
                assert block == n * lens.max()
                # the model: rank r's block as an array [n][len_r] of (lane, trial) ids, laid at r * block, the rest -1
                buf = np.full(world * block, -1, dtype=np.int64)
                for r in range(world):
                    ids = np.arange(n)[:, None] * trials + (cuts[r] + np.arange(lens[r]))[None, :]
                    buf[r * block:r * block + n * lens[r]] = ids.reshape(-1)
                got = np.full(world * block, -1, dtype=np.int64)
                for r in range(world):
                    for b in range(n):
                        for k in range(lens[r]):
                            pos = D.pack_batch_position(r, b, k, n, cuts, block)
                            assert r * block <= pos < (r + 1) * block and got[pos] == -1  # inside the block, injective
                            got[pos] = b * trials + cuts[r] + k
                assert (got == buf).all()
                assert (got >= 0).sum() == n * trials
    for bad in ((0, 0, 2), (1, 3), (0, 2, 2, 4)):
        with pytest.raises(ValueError):
            D.pack_batch_block_cts(2, bad)
    with pytest.raises(ValueError):
        D.pack_batch_block_cts(9, (0, 4))
    cuts = (0, 1, 3, 4)
    for args in ((3, 0, 0), (0, 2, 0), (1, 0, 2), (0, 0, 1), (-1, 0, 0)):
        with pytest.raises(ValueError):
            D.pack_batch_position(*args, 2, cuts, 4)
    with pytest.raises(ValueError):
        D.pack_batch_position(1, 0, 0, 2, cuts, 3)  # a block too small for two lanes of two trials


def test_bindings_exist(sa):
    from spiral_amd import dist as D
    from spiral_amd import pack as _  # noqa: F401  (spiral_amd.pack is also the name of a function: take the module itself)

    P = sys.modules["spiral_amd.pack"]
    L = sa.lib()
    for name in ("create_shard_lane", "fold_trials_batch", "pack_gathered_batch"):
        assert hasattr(L, "spiral_gpu_pack_server_" + name)
    header = open(os.path.join(ROOT, "include", "spiral_gpu.h")).read()
    for name in ("create_shard_lane", "fold_trials_batch", "pack_gathered_batch"):
        assert f"int spiral_gpu_pack_server_{name}(" in header
    assert callable(P.PackServer.create_shard_lane) and callable(P.fold_trials_batch) and callable(P.pack_gathered_batch)
    assert callable(D.pack_batch_buffers) and callable(D.all_gather_pack_batch) and callable(D.answer_pack_batch_sharded)


def test_entry_points_refuse_before_any_device_call(sa):
    """null arguments, then the shared list check (its texts as in tests/test_lanes_cpu.py): no servers, nine, a null entry -- no server exists here, so
    a call that dereferenced one or reached the device would crash or fail differently; nothing is written"""
    L = sa.lib()
    from spiral_amd._lib import U64P

    out = np.zeros(64, dtype=np.uint64)
    buf = np.zeros(64, dtype=np.uint64)
    outv, bufv = C.c_void_p(out.ctypes.data), C.c_void_p(buf.ctypes.data)
    out_list = (U64P * 9)(*([out.ctypes.data_as(U64P)] * 9))
    void_list = (C.c_void_p * 9)(*([buf.ctypes.data] * 9))
    cuts = (C.c_uint32 * 3)(0, 2, 4)
    nulls = (C.c_void_p * 9)()
    err = lambda: L.spiral_gpu_last_error().decode()

    def fold(hs, n, form=0, queries=void_list, folded=outv):
        return L.spiral_gpu_pack_server_fold_trials_batch(hs, n, form, queries, 16, folded)

    def pack(hs, n, gathered=bufv, cuts_=cuts, responses=out_list, packed=out_list, wire=outv):
        return L.spiral_gpu_pack_server_pack_gathered_batch(hs, n, gathered, cuts_, 2, 8, responses, packed, wire)

    assert fold(nulls, 1, queries=None) != 0 and err() == "fold_trials_batch: null queries or output buffer"
    assert fold(nulls, 1, folded=None) != 0 and err() == "fold_trials_batch: null queries or output buffer"
    assert fold(nulls, 1, form=3) != 0 and err() == "fold_trials_batch: unknown query form 3"
    assert pack(nulls, 1, gathered=None) != 0 and err() == "pack_gathered_batch: null gathered buffer or cuts"
    assert pack(nulls, 1, cuts_=None) != 0 and err() == "pack_gathered_batch: null gathered buffer or cuts"
    assert pack(nulls, 1, responses=None, packed=None, wire=None) != 0 and err() == "pack_gathered_batch: no output (responses, packed_cts or wire)"
    for call, what in ((fold, "fold_trials_batch"), (pack, "pack_gathered_batch")):
        for n, hs, text in ((1, None, "no servers"), (0, nulls, "no servers"), (9, nulls, "at most 8 clients per batch"), (2, nulls, "null server 0")):
            assert call(hs, n) != 0, (what, n)
            assert err() == f"{what}: {text}", (what, n)
    h = C.c_void_p()
    assert L.spiral_gpu_pack_server_create_shard_lane(None, C.byref(h)) != 0 and err() == "null argument"
    assert L.spiral_gpu_pack_server_create_shard_lane(bufv, None) != 0 and err() == "null argument"
    assert not out.any() and not h.value, "a refused call wrote to its output"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _gather_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist

    from spiral_amd import dist as D

    dist.init_process_group("gloo", rank=rank, world_size=world)
    n, trials, words = 3, 9, 8  # (a few words stand in for a ciphertext: the collective moves whole blocks)
    cuts = D.pack_trial_cuts(world, trials)  # (0, 4, 9): unequal ranges
    block = D.pack_batch_block_cts(n, cuts)
    value = lambda r, b, k: (r * 100 + b * 10 + k) * 1000
    mine = torch.full((block * words,), -1, dtype=torch.int64)
    for b in range(n):
        for k in range(cuts[rank + 1] - cuts[rank]):
            at = D.pack_batch_position(rank, b, k, n, cuts, block) - rank * block
            mine[at * words:(at + 1) * words] = value(rank, b, k) + torch.arange(words)
    gathered = torch.zeros(world * block * words, dtype=torch.int64)
    D.all_gather_pack_batch(gathered, mine)
    ok = True
    seen = torch.zeros(world * block, dtype=torch.bool)
    for r in range(world):
        for b in range(n):
            for k in range(cuts[r + 1] - cuts[r]):
                at = D.pack_batch_position(r, b, k, n, cuts, block)
                seen[at] = True
                ok &= bool((gathered[at * words:(at + 1) * words] == value(r, b, k) + torch.arange(words)).all())
    ok &= bool((gathered.view(-1, words)[~seen] == -1).all())  # the padding of the shorter rank's block travelled as it was
    try:
        D.all_gather_pack_batch(gathered[:-1], mine)
        ok = False
    except ValueError:
        pass
    q.put((rank, ok))
    dist.destroy_process_group()


def test_gloo_all_gather_lands_each_block_at_its_rank():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got == {0: True, 1: True}
