"""CPU-side checks of the batch calls of a sharded answer (run_pre_sweep_batch ... fold_root_batch): the library exports them, the Python binding
declares them, the size and layout helpers of spiral_amd/dist.py agree with the header, every argument check that runs before a device call
refuses bad input, and answer_batch_sharded on a gloo group of two ranks reaches its first library call."""
import ctypes as C
import os
import socket
import sys
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CT = 6 * 2048

NEW_SYMBOLS = [
    "spiral_gpu_server_run_pre_sweep_batch",
    "spiral_gpu_server_run_expand_pack_batch",
    "spiral_gpu_server_run_unpack_convert_sweep_batch",
    "spiral_gpu_server_fold_local_batch",
    "spiral_gpu_server_fold_root_batch",
]


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


def test_new_symbols_exported_and_declared(sa):
    from spiral_amd import _lib
    from spiral_amd import dist as sdist

    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES, name
    for fn in ("run_pre_sweep_batch", "run_expand_pack_batch", "run_unpack_convert_sweep_batch", "fold_local_batch", "fold_root_batch"):
        assert callable(getattr(sa, fn)) and callable(getattr(sa.server, fn)), fn
    for fn in ("batch_acc_words", "batch_chunk_words", "batch_ct_words", "batch_gathered_ct_words", "batch_bits_words", "batch_acc_position",
               "batch_collective_bytes", "batch_buffers", "reduce_scatter_batch", "all_gather_batch_cts", "all_gather_batch_bits", "answer_batch_sharded"):
        assert callable(getattr(sdist, fn)), fn


def test_size_helpers():
    from spiral_amd import dist as sdist

    c1, c2 = SimpleNamespace(num_per=128), SimpleNamespace(num_per=1024)  # configs[1] and configs[2]
    # the reduce-scatter input: n x num_per x 96 KiB
    assert sdist.batch_acc_words(c1, 8) * 8 == 96 << 20
    assert sdist.batch_acc_words(c2, 8) * 8 == 768 << 20
    assert sdist.batch_chunk_words(c2, 8, 8) * 8 == sdist.batch_acc_words(c2, 8)
    assert sdist.batch_chunk_words(c2, 3, 4) == 3 * 256 * CT
    assert sdist.batch_ct_words(5) == 5 * CT and sdist.batch_gathered_ct_words(5, 4) == 20 * CT
    assert sdist.batch_bits_words(100, 3) == 300
    b = sdist.batch_collective_bytes(c2, 8, 8, gsw_bits_words=1000)
    assert b == {"reduce_scatter_in_bytes": 768 << 20, "all_gather_cts_out_bytes": 64 * CT * 8, "all_gather_bits_out_bytes": 8 * 8 * 1000 * 8}
    assert sdist.batch_collective_bytes(c1, 2, 1) == {"reduce_in_bytes": 2 * 128 * CT * 8}
    for bad in (0, 9):
        with pytest.raises(ValueError):
            sdist.batch_acc_words(c1, bad)
    with pytest.raises(ValueError):
        sdist.batch_chunk_words(SimpleNamespace(num_per=6), 1, 4)


@pytest.mark.parametrize("n,G,num_per", [(1, 1, 8), (3, 1, 16), (3, 2, 16), (8, 4, 32), (5, 8, 64)])
def test_rank_major_layout(n, G, num_per):
    """every (lane, ciphertext) has its own slot, and rank g's contiguous 1/G of the buffer is [lane][k] of the ciphertexts ii = g + G k"""
    from spiral_amd import dist as sdist

    L = num_per // G
    seen = {}
    for b in range(n):
        for ii in range(num_per):
            pos = sdist.batch_acc_position(ii, b, n, G, num_per)
            assert 0 <= pos < n * num_per and pos not in seen
            seen[pos] = (b, ii)
            g, rem = divmod(pos, n * L)  # the reduce-scatter's slice and the place in it
            assert g == ii % G and rem == b * L + ii // G
    if n == 1:  # one client: the one-query grouping by ii mod G (acc_position)
        for ii in range(num_per):
            assert sdist.batch_acc_position(ii, 0, 1, G, num_per) == sdist.acc_position(ii, G, num_per)


def test_null_arguments_fail_before_any_device_call(sa):
    """null lists, null servers, too many lanes: refused with a message by the library's checks, which run before anything is launched"""
    lib = sa.lib()
    err = lambda: lib.spiral_gpu_last_error().decode()
    one = (C.c_void_p * 1)(None)
    nine = (C.c_void_p * 9)(*([None] * 9))
    buf = C.c_void_p(0x1000)
    cases = [
        ("run_pre_sweep_batch", lambda a, n: lib.spiral_gpu_server_run_pre_sweep_batch(a, n, buf)),
        ("run_expand_pack_batch", lambda a, n: lib.spiral_gpu_server_run_expand_pack_batch(a, n, buf)),
        ("run_unpack_convert_sweep_batch", lambda a, n: lib.spiral_gpu_server_run_unpack_convert_sweep_batch(a, n, buf, buf)),
        ("fold_local_batch", lambda a, n: lib.spiral_gpu_server_fold_local_batch(a, n, buf, buf)),
        ("fold_root_batch", lambda a, n: lib.spiral_gpu_server_fold_root_batch(a, n, buf, None, None)),
    ]
    for what, call in cases:
        assert call(None, 1) != 0
        assert f"{what}: no servers" in err()
        assert call(one, 0) != 0
        assert call(nine, 9) != 0
        assert "at most 8 clients" in err(), what
        assert call(one, 1) != 0
        assert f"{what}: null server 0" in err(), what


def test_python_wrappers_reach_the_library_checks(sa):
    fake = SimpleNamespace(h=None)
    with pytest.raises(RuntimeError, match="run_pre_sweep_batch: null server 0"):
        sa.run_pre_sweep_batch([fake], 0x1000)
    with pytest.raises(RuntimeError, match="fold_root_batch: no servers"):
        sa.fold_root_batch([], 0x1000)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    try:
        import torch
        import torch.distributed as dist

        from spiral_amd import dist as sdist

        dist.init_process_group("gloo", rank=rank, world_size=world)
        n, shape = 3, SimpleNamespace(num_per=16)
        bufs = {k: torch.zeros(w, dtype=torch.int64) for k, w in (("acc", sdist.batch_acc_words(shape, n)), ("cts", sdist.batch_ct_words(n)),
                                                                   ("responses", sdist.batch_ct_words(n)), ("chunk", sdist.batch_chunk_words(shape, n, world)),
                                                                   ("gathered_cts", sdist.batch_gathered_ct_words(n, world)))}
        servers = [SimpleNamespace(h=None, shape=shape) for _ in range(n)]
        try:
            sdist.answer_batch_sharded(servers, None, bufs)
            q.put((rank, "no error"))
        except RuntimeError as e:  # the first library call: the library refuses the (null) servers before any device call
            q.put((rank, str(e)))
        try:
            sdist.answer_batch_sharded(servers, None, dict(bufs, acc=bufs["acc"][1:]))
            q.put((rank, "no error"))
        except ValueError as e:  # a buffer of the wrong size never reaches the library
            q.put((rank, str(e)))
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover - reported to the parent
        q.put((rank, f"worker failed: {e!r}"))


def test_answer_batch_sharded_gloo_world_two_reaches_the_library():
    import multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in range(4)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    msgs = sorted(got)
    for rank in (0, 1):
        mine = [m for r, m in msgs if r == rank]
        assert any("run_pre_sweep_batch: null server 0" in m for m in mine), mine
        assert any("answer_batch_sharded: acc" in m for m in mine), mine
