"""Column shards without a device: the three entry points are exported, declared in the header and bound in Python; spiral_gpu_column_shard_has_limb_form
is spiral_gpu_has_limb_form of the geometry with nu2 - log2 G (the same rule, the same option "sweep_narrow") and refuses a rank count that gives no
shard; the collective of a column-sharded batch is one all-gather, sized from the shapes; creating a server fails loudly where there is no GPU."""
import ctypes as C
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = {
    "spiral_gpu_server_create_column_shard": "int spiral_gpu_server_create_column_shard(const spiral_gpu_params *p, int device, uint32_t rank, uint32_t n_ranks, spiral_gpu_server **out);",
    "spiral_gpu_column_shard_has_limb_form": "int spiral_gpu_column_shard_has_limb_form(const spiral_gpu_params *p, uint32_t n_ranks);",
    "spiral_gpu_server_run_column_batch": "int spiral_gpu_server_run_column_batch(spiral_gpu_server *const *servers, uint32_t n, void *out_cts);",
}
GEOMETRIES = [(8, 7), (9, 10), (8, 6), (5, 5)]


@pytest.fixture(scope="module")
def sa():
    # torch first, as in the GPU files: it ships its own HIP runtime, and where there is a GPU this file opens it (a server is created below)
    import torch

    torch.cuda.is_available()
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


def test_symbols_exported_declared_and_bound(sa):
    from spiral_amd import _lib, dist, ops, server

    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "spiral_gpu.h")).read()
    for name, decl in NEW_SYMBOLS.items():
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES and _lib.PROTOTYPES[name][0] is C.c_int, name
        assert decl in header, name
    assert sa.run_column_batch is server.run_column_batch and list(inspect.signature(sa.run_column_batch).parameters) == ["servers", "out_cts_ptr"]
    assert sa.column_shard_has_limb_form is ops.column_shard_has_limb_form
    sig = inspect.signature(sa.Server.__init__).parameters
    assert list(sig)[:6] == ["self", "params", "device", "j_begin", "j_end", "share_db_of"]  # the positional use is untouched
    for k in ("col_rank", "col_ranks"):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY and sig[k].default is None
    for name in ("column_batch_buffers", "column_batch_collective_bytes", "answer_batch_column_sharded"):
        assert callable(getattr(dist, name)), name
    sig = inspect.signature(dist.answer_batch_column_sharded).parameters
    assert list(sig) == ["servers", "group", "bufs", "root", "wire_ptr"] and sig["root"].kind is inspect.Parameter.KEYWORD_ONLY


def test_create_fails_loudly_without_a_device(sa):
    """like every compute entry point; where there is a GPU the same call gives a server, and a bad rank count is refused either way"""
    L = sa.lib()
    p = sa.make_params(4, 4, t_gsw=4)
    h = C.c_void_p()
    for rank, G, text in ((0, 3, "power of two"), (0, 0, "power of two"), (0, 32, "at least 1"), (2, 2, "no such rank")):
        assert L.spiral_gpu_server_create_column_shard(C.byref(p), 0, rank, G, C.byref(h)) != 0 and not h.value
        assert text in L.spiral_gpu_last_error().decode(), (rank, G)
    assert L.spiral_gpu_server_create_column_shard(None, 0, 0, 2, C.byref(h)) != 0 and L.spiral_gpu_server_create_column_shard(C.byref(p), 0, 0, 2, None) != 0
    with pytest.raises(ValueError, match="both col_rank and col_ranks"):
        sa.Server(p, col_rank=1)
    with pytest.raises(ValueError, match="no j-range"):
        sa.Server(p, 0, 0, 8, col_rank=0, col_ranks=2)
    if L.spiral_gpu_device_count() == 0:
        with pytest.raises(sa.SpiralGpuError):
            sa.Server(p, col_rank=0, col_ranks=2)
        assert L.spiral_gpu_server_create_column_shard(C.byref(p), 0, 0, 2, C.byref(h)) != 0 and not h.value
    else:
        srv = sa.Server(p, col_rank=1, col_ranks=2)
        assert (srv.col_rank, srv.col_ranks) == (1, 2)
        srv.close()


def test_list_check(sa):
    """the cases tests/test_lanes_cpu.py runs on every call of its table, on run_column_batch: a missing list, an empty one, nine entries and a null
    entry are refused with the call's name and the SAME text for the same cause, before a handle is dereferenced and without writing the output"""
    import numpy as np

    L = sa.lib()
    out = np.zeros(64, dtype=np.uint64)
    nulls = (C.c_void_p * 9)()
    for n, hs, err in ((1, None, "no servers"), (0, nulls, "no servers"), (9, nulls, "at most 8 clients per batch"), (2, nulls, "null server 0")):
        assert L.spiral_gpu_server_run_column_batch(hs, n, C.c_void_p(out.ctypes.data)) != 0, (n, err)
        assert L.spiral_gpu_last_error().decode() == f"run_column_batch: {err}", (n, err)
    assert not out.any(), "a refused call wrote to its output"


@pytest.mark.parametrize("narrow", [0, 1])
def test_limb_form_is_that_of_the_geometry_with_fewer_columns(sa, opts, narrow):
    opts(sweep_narrow=narrow)
    L = sa.lib()
    seen = set()
    for nu1, nu2 in GEOMETRIES:
        p = sa.make_params(nu1, nu2, t_gsw=4)
        for g_log, G in enumerate((1, 2, 4, 8)):
            rc = L.spiral_gpu_column_shard_has_limb_form(C.byref(p), G)
            assert rc in (0, 1) and sa.column_shard_has_limb_form(p, G) is bool(rc), (nu1, nu2, G)
            assert bool(rc) is sa.has_limb_form(sa.make_params(nu1, nu2 - g_log, t_gsw=4)), (nu1, nu2, G, narrow)
            seen.add(rc)
        assert sa.column_shard_has_limb_form(p, 1) is sa.has_limb_form(p)
    assert seen == {0, 1}  # (the comparison saw both answers)
    # the rule itself at the shapes the GPU tests use: (8, 6) over 4 ranks is 16 columns -- the narrow form, with the option only
    assert sa.column_shard_has_limb_form(sa.make_params(8, 6, t_gsw=4), 4) is bool(narrow)
    assert sa.column_shard_has_limb_form(sa.make_params(7, 7, t_gsw=4), 2) is True  # 64 columns: the wide form


def test_limb_form_refuses_rank_counts_that_give_no_shard(sa):
    L = sa.lib()
    p = sa.make_params(8, 6, t_gsw=4)
    err = lambda: L.spiral_gpu_last_error().decode()
    for G in (3, 6, 0):
        assert L.spiral_gpu_column_shard_has_limb_form(C.byref(p), G) == 0 and "power of two" in err(), G
    assert L.spiral_gpu_column_shard_has_limb_form(C.byref(p), 128) == 0  # L = 0, below the bound of one column
    assert "at least 1" in err() and "128 ranks" in err()
    assert L.spiral_gpu_column_shard_has_limb_form(C.byref(p), 64) == 0  # (L = 1 is a shard; it has no limb form)
    assert L.spiral_gpu_column_shard_has_limb_form(None, 2) == -1
    assert L.spiral_gpu_column_shard_has_limb_form(C.byref(p), 1) == 1  # (an error is not sticky)
    assert sa.column_shard_has_limb_form(p, 3) is False


def test_collective_bytes_are_one_all_gather(sa):
    from spiral_amd import dist

    kw = dict(t_gsw=10, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=22, p_db=256)  # configs[2]
    s = sa.get_shape(sa.make_params(9, 10, **kw))
    out = dist.column_batch_collective_bytes(s, 8, 8)
    assert out == {"all_gather_cts_out_bytes": 8 * 8 * 96 * 1024}
    assert not any("reduce" in k for k in out)
    # against the j-shard's step at the same point: the same all-gather, and 768 MiB of reduce-scatter that the column shard does not have
    j = dist.batch_collective_bytes(s, 8, 8)
    assert j["all_gather_cts_out_bytes"] == out["all_gather_cts_out_bytes"] and j["reduce_scatter_in_bytes"] == 768 << 20
    for n, G in ((1, 2), (3, 4)):
        assert dist.column_batch_collective_bytes(s, n, G) == {"all_gather_cts_out_bytes": n * G * 96 * 1024}
    with pytest.raises(ValueError, match="column shards"):
        dist.column_batch_collective_bytes(s, 2, 3)
    with pytest.raises(ValueError, match="1 .. 8 clients"):
        dist.column_batch_collective_bytes(s, 9, 2)


def test_buffers_have_no_accumulator_and_no_chunk(sa):
    """the buffers are torch tensors on whichever device is asked for: built here on the CPU device, which needs no GPU"""
    import torch

    from spiral_amd import dist

    class Lane:
        pass

    bufs = dist.column_batch_buffers([Lane(), Lane(), Lane()], 4, device=torch.device("cpu"))
    assert sorted(bufs) == ["cts", "gathered_cts", "responses"] and "acc" not in bufs and "chunk" not in bufs
    ct = 6 * 2048
    assert [bufs[k].numel() for k in ("cts", "gathered_cts", "responses")] == [3 * ct, 4 * 3 * ct, 3 * ct]
    assert all(t.dtype == torch.int64 and not t.any() for t in bufs.values())


def test_documents_name_the_calls():
    for path, words in (("README.md", ["run_column_batch", "column_shard.json"]), ("DESIGN.md", ["Column shards", "create_column_shard"]),
                        ("INTEGRATION.md", ["run_column_batch", "fold_root_batch"]), ("profiles/README.md", ["column_shard.json"])):
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        for w in words:
            assert w in text, (path, w)
