"""CPU-side checks of the SpiralPack record store (include/spiral_gpu.h "Records", SpiralPack): spiral_gpu_pack_record_layout_of against the numpy
restatement of the layout (tests/pack_records_restated.py), the new symbols exported and declared, and every argument check of every new call failing
cleanly without a device."""
import ctypes as C
import os

import numpy as np
import pytest

import pack_records_restated as PR
import records_restated as R

NEW_SYMBOLS = ["spiral_gpu_pack_record_layout_of", "spiral_gpu_pack_server_load_records", "spiral_gpu_pack_server_update_records",
               "spiral_gpu_pack_server_read_records", "spiral_gpu_pack_server_read_records_at"]
NU1, NU2 = 7, 4


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


def fields(lay):
    return (lay.coeff_bits, lay.item_bytes, lay.per_item, lay.instances, lay.capacity)


def test_new_symbols_exported_and_declared(sa):
    from spiral_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spiral_gpu.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES, name
        assert name + "(" in header, name
    assert sa.lib().spiral_gpu_abi_version() == 1, "additive: the ABI version is unchanged"
    for meth in ("load_records", "update_records", "read_records", "read_records_at"):
        assert callable(getattr(sa.PackServer, meth)), meth


def sizes_of(item_bytes):
    return [1, 99, 256, 2048, 3000, item_bytes, item_bytes + 1, 16 * item_bytes, 16 * item_bytes + 1]


@pytest.mark.parametrize("p_db", [256, 32, 48])
@pytest.mark.parametrize("out_n", [1, 2, 3])
def test_layout_equals_the_restatement(sa, out_n, p_db):
    pg = sa.make_params(NU1, NU2, p_db=p_db)
    w = p_db.bit_length() - 1
    item_bytes = out_n * out_n * 256 * w
    for S in sizes_of(item_bytes):
        want = PR.layout(p_db, NU1, NU2, out_n, S)
        if S == 16 * item_bytes + 1:
            assert want is None
            with pytest.raises(sa.SpiralGpuError, match="at most 16"):
                sa.record_layout(pg, S, out_n)
            continue
        got = sa.record_layout(pg, S, out_n)
        assert fields(got) == fields(want), (out_n, p_db, S)
        assert got.coeff_bits == w and got.item_bytes == item_bytes
        assert got.capacity == (1 << (NU1 + NU2)) * got.per_item
    assert PR.layout(p_db, NU1, NU2, out_n, item_bytes + 1).instances == 2
    assert PR.layout(p_db, NU1, NU2, out_n, 16 * item_bytes).instances == 16


def test_a_few_layouts_by_hand(sa):
    """out_n = 2 at 8 bits: 4 polynomials of 2048 bytes, the base server's item size; out_n = 4: 32 KiB items, 128 records of 256 bytes"""
    pg = sa.make_params(10, 8)
    two, four = sa.record_layout(pg, 256, 2), sa.record_layout(pg, 256, 4)
    assert fields(two) == (8, 8192, 32, 1, 32 << 18)
    assert fields(four) == (8, 32768, 128, 1, 128 << 18)
    assert fields(sa.record_layout(pg, 3000, 3)) == (8, 18432, 6, 1, 6 << 18)
    assert fields(sa.record_layout(pg, 20000, 2)) == (8, 8192, 1, 3, 1 << 18)
    lay = PR.layout(256, 10, 8, 2, 3000)
    assert PR.place(lay, 3000, 2) == (1, 0, 3000, 0) and PR.place(lay, 3000, 1) == (0, 3000, 3000, 0)
    assert list(PR.trials_of(lay, 3000, 3000)) == [1, 2], "record 1 of 3000 bytes straddles trials 1 and 2"


def test_out_n_0_is_the_base_layout(sa):
    pg = sa.make_params(6, 6)
    for S in (1, 99, 256, 3000, 8192, 8193):
        assert fields(sa.record_layout(pg, S, 0)) == fields(sa.record_layout(pg, S)) == fields(R.layout(256, 6, 6, S))
    L = sa.lib()
    out = sa.RecordLayout(7, 7, 7, 7, 7)
    assert L.spiral_gpu_pack_record_layout_of(C.byref(pg), 0, 256, C.byref(out)) != 0 and b"out_n" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_pack_record_layout_of(C.byref(pg), 17, 256, C.byref(out)) != 0 and b"out_n" in L.spiral_gpu_last_error()
    assert fields(out) == (7, 7, 7, 7, 7), "a refused layout writes nothing"


def test_layout_refusals(sa):
    pg = sa.make_params(6, 6)
    with pytest.raises(sa.SpiralGpuError, match="at least one byte"):
        sa.record_layout(pg, 0, 2)
    with pytest.raises(ValueError):
        sa.record_layout(pg, 256, -1)
    with pytest.raises(ValueError):
        sa.record_layout(pg, 256, 2.0)
    with pytest.raises(sa.SpiralGpuError, match="out_n"):
        sa.record_layout(pg, 256, 17)
    with pytest.raises(sa.SpiralGpuError):
        sa.record_layout(sa.make_params(6, 6, p_db=1), 256, 2)  # parameters get_shape refuses
    L = sa.lib()
    out = sa.RecordLayout(7, 7, 7, 7, 7)
    assert L.spiral_gpu_pack_record_layout_of(None, 2, 256, C.byref(out)) != 0 and b"null" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_pack_record_layout_of(C.byref(pg), 2, 256, None) != 0 and b"null" in L.spiral_gpu_last_error()
    assert fields(out) == (7, 7, 7, 7, 7)


def test_null_server_fails_with_a_message(sa):
    L = sa.lib()
    ids = (C.c_uint64 * 1)(0)
    buf = np.full(8192, 0xA5, dtype=np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    for rc in (L.spiral_gpu_pack_server_load_records(None, p, 256, 0, 0, 32), L.spiral_gpu_pack_server_update_records(None, p, 256, 0, ids, 1),
               L.spiral_gpu_pack_server_read_records(None, p, 256, 0, 0, 1), L.spiral_gpu_pack_server_read_records_at(None, p, 256, 0, ids, 1)):
        assert rc != 0 and b"null" in L.spiral_gpu_last_error()
    assert (buf == 0xA5).all(), "nothing written"


@pytest.fixture
def fake(sa):
    """a PackServer that never touched the library (a handle no wrapper may pass on): closed again whatever the test did"""
    s = sa.PackServer.__new__(sa.PackServer)
    s.h = C.c_void_p(0x1000)
    s.params, s.out_n = sa.make_params(6, 6), 2
    yield s
    s.h = None


def test_wrappers_reject_bad_argument_lists(sa, fake):
    two = np.zeros(2 * 256, dtype=np.uint8)
    with pytest.raises(ValueError, match="bytes"):
        fake.update_records(two, 256, [1])  # two records for one id
    with pytest.raises(ValueError, match="duplicate"):
        fake.update_records(two, 256, [5, 5])
    with pytest.raises(TypeError, match="integers"):
        fake.update_records(two, 256, [1.0, 2.0])
    with pytest.raises(ValueError, match="non-negative"):
        fake.update_records(two, 256, [-1, 2])
    with pytest.raises(TypeError, match="uint8"):
        fake.update_records(np.zeros(64, dtype=np.uint64), 256, [1, 2])
    with pytest.raises(sa.SpiralGpuError, match="at least one byte"):
        fake.update_records(two, 0, [1, 2])
    with pytest.raises(ValueError, match="whole"):
        fake.load_records(np.zeros(300, dtype=np.uint8), 256)
    with pytest.raises(sa.SpiralGpuError, match="at most 16"):
        fake.load_records(two, 16 * 8192 + 1)
    out = np.full(3 * 256, 0xA5, dtype=np.uint8)
    with pytest.raises(ValueError, match="out must be"):
        fake.read_records_at(256, [1, 2], out=out)  # three records' room for two ids
    with pytest.raises(ValueError, match="out must be"):
        fake.read_records(256, 0, 2, out=out)
    with pytest.raises(TypeError, match="integers"):
        fake.read_records_at(256, [0.5], out=out)
    with pytest.raises(sa.SpiralGpuError, match="at most 16"):
        fake.read_records(16 * 8192 + 1, 0, 1)
    assert (out == 0xA5).all(), "nothing written"


def test_restated_splice_and_cut_round_trip():
    """the restatement against itself: a record that straddles trials 1 and 2 and ends inside a coefficient (w = 5)"""
    rng = np.random.default_rng(3)
    w, trials = 5, 4
    item = rng.integers(0, 1 << w, size=(trials, PR.N), dtype=np.uint64)
    data = rng.integers(0, 256, size=99, dtype=np.uint8)
    off = 2 * 256 * w - 40
    new = PR.splice(item, w, off, data)
    assert (PR.cut(new, w, off, 99) == data).all()
    assert (new[0] == item[0]).all() and (new[3] == item[3]).all()
    assert (PR.cut(new, w, 0, off) == PR.cut(item, w, 0, off)).all()
    tail = off + 99
    assert (PR.cut(new, w, tail, trials * 256 * w - tail) == PR.cut(item, w, tail, trials * 256 * w - tail)).all()
    assert list(PR.trials_of(PR.Layout(w, trials * 256 * w, 1, 1, 1), off, 99)) == [1, 2]
