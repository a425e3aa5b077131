"""CPU-side checks of the record store (include/spiral_gpu.h "Records"): spiral_gpu_record_layout_of against the numpy restatement of the layout
(tests/records_restated.py), the new symbols exported and declared, and every argument check of every new call failing cleanly without a device."""
import ctypes as C

import numpy as np
import pytest

import records_restated as R

NEW_SYMBOLS = ["spiral_gpu_record_layout_of", "spiral_gpu_server_load_records", "spiral_gpu_server_update_records", "spiral_gpu_server_read_records",
               "spiral_gpu_server_read_records_at", "spiral_gpu_client_record_queries", "spiral_gpu_client_decode_records"]
CONFIG1 = dict(nu1=8, nu2=7, t_gsw=8, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=20, p_db=256)  # bench.py WORKLOADS configs[1]
CONFIG3 = dict(nu1=11, nu2=9, t_gsw=4, t_conv=56, t_exp=2, t_exp_right=56, qprime_bits=27, p_db=32768, direct_upload=1)  # configs[3]


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
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES, name
    assert sa.lib().spiral_gpu_abi_version() == 1


@pytest.mark.parametrize("S", [1, 99, 256, 3000, 8192, 8193, 16 * 8192])
def test_layout_at_8_bits(sa, S):
    pg = sa.make_params(6, 6)
    want = R.layout(256, 6, 6, S)
    assert fields(sa.record_layout(pg, S)) == fields(want)
    if S == 8193:
        assert want.instances == 2 and want.per_item == 1
    if S == 99:
        assert want.per_item == 82 and want.item_bytes - want.per_item * S == 74


@pytest.mark.parametrize("p_db,S", [(32, 99), (32, 5120), (48, 99), (2, 1), (2, 1024), (1 << 15, 15360), (1 << 40, 1)])
def test_layout_at_other_widths(sa, p_db, S):
    pg = sa.make_params(4, 3, p_db=p_db)
    assert fields(sa.record_layout(pg, S)) == fields(R.layout(p_db, 4, 3, S))
    assert sa.record_layout(pg, S).coeff_bits == p_db.bit_length() - 1


def test_layout_of_the_quoted_configurations(sa):
    one = sa.record_layout(sa.make_params(**CONFIG1), 256)
    assert fields(one) == fields(R.layout(256, 8, 7, 256))
    assert (one.coeff_bits, one.item_bytes, one.per_item, one.instances, one.capacity) == (8, 8192, 32, 1, 1 << 20)
    three = sa.record_layout(sa.make_params(**CONFIG3), 100_000)
    assert fields(three) == fields(R.layout(32768, 11, 9, 100_000))
    assert (three.coeff_bits, three.item_bytes, three.per_item, three.instances, three.capacity) == (15, 15360, 1, 7, 1 << 20)


def test_layout_refusals(sa):
    pg = sa.make_params(6, 6)
    assert R.layout(256, 6, 6, 17 * 8192) is None
    with pytest.raises(sa.SpiralGpuError, match="at most 16"):
        sa.record_layout(pg, 17 * 8192)
    with pytest.raises(sa.SpiralGpuError, match="at least one byte"):
        sa.record_layout(pg, 0)
    with pytest.raises(ValueError):
        sa.record_layout(pg, -1)
    with pytest.raises(ValueError):
        sa.record_layout(pg, 2.0)
    with pytest.raises(sa.SpiralGpuError):
        sa.record_layout(sa.make_params(6, 6, p_db=1), 256)  # parameters get_shape refuses
    L = sa.lib()
    out = sa.RecordLayout(7, 7, 7, 7, 7)
    assert L.spiral_gpu_record_layout_of(None, 256, C.byref(out)) != 0 and b"null" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_record_layout_of(C.byref(pg), 256, None) != 0 and b"null" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_record_layout_of(C.byref(pg), 17 * 8192, C.byref(out)) != 0
    assert fields(out) == (7, 7, 7, 7, 7), "a refused layout writes nothing"


def test_null_server_fails_with_a_message(sa):
    L = sa.lib()
    ids = (C.c_uint64 * 1)(0)
    buf = np.full(8192, 0xA5, dtype=np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    for rc in (L.spiral_gpu_server_load_records(None, p, 256, 0, 0, 32), L.spiral_gpu_server_update_records(None, p, 256, 0, ids, 1),
               L.spiral_gpu_server_read_records(None, p, 256, 0, 0, 1), L.spiral_gpu_server_read_records_at(None, p, 256, 0, ids, 1)):
        assert rc != 0 and b"null" in L.spiral_gpu_last_error()
    assert (buf == 0xA5).all(), "nothing written"


def test_null_client_fails_with_a_message(sa):
    L = sa.lib()
    ids = (C.c_uint64 * 1)(0)
    buf = np.full(8192, 0xA5, dtype=np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.spiral_gpu_client_record_queries(None, 256, ids, 1, 2, p, buf.size) != 0 and b"null client session" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_client_decode_records(None, p, 1, 0, 256, ids, p) != 0 and b"null client session" in L.spiral_gpu_last_error()
    assert (buf == 0xA5).all(), "nothing written"


@pytest.fixture
def fake(sa):
    """a Server that never touched the library (a handle no wrapper may pass on): closed again whatever the test did"""
    from spiral_amd import server as SV

    s = SV.Server.__new__(SV.Server)
    s.h = C.c_void_p(0x1000)
    s.params = sa.make_params(6, 6)
    yield s
    s.h = None


def test_wrappers_reject_bad_argument_lists(sa, fake):
    two = np.zeros(2 * 256, dtype=np.uint8)
    with pytest.raises(ValueError, match="bytes"):
        fake.update_records(two, 256, [1])  # two records for one id
    with pytest.raises(ValueError, match="bytes"):
        fake.update_records(two, 256, [1, 2, 3])
    with pytest.raises(ValueError, match="duplicate"):
        fake.update_records(two, 256, [5, 5])
    with pytest.raises(TypeError, match="integers"):
        fake.update_records(two, 256, [1.0, 2.0])
    with pytest.raises(TypeError, match="integers"):
        fake.update_records(two, 256, [True, False])
    with pytest.raises(ValueError, match="non-negative"):
        fake.update_records(two, 256, [-1, 2])
    with pytest.raises(ValueError, match="flat"):
        fake.update_records(two, 256, [[1, 2]])
    with pytest.raises(TypeError, match="uint8"):
        fake.update_records(np.zeros(64, dtype=np.uint64), 256, [1, 2])
    with pytest.raises(sa.SpiralGpuError, match="at least one byte"):
        fake.update_records(two, 0, [1, 2])
    with pytest.raises(ValueError, match="whole"):
        fake.load_records(np.zeros(300, dtype=np.uint8), 256)
    with pytest.raises(TypeError, match="uint8"):
        fake.load_records(np.zeros(256, dtype=np.int32), 256)
    with pytest.raises(sa.SpiralGpuError, match="at most 16"):
        fake.load_records(two, 17 * 8192)
    out = np.full(3 * 256, 0xA5, dtype=np.uint8)
    with pytest.raises(ValueError, match="out must be"):
        fake.read_records_at(256, [1, 2], out=out)  # three records' room for two ids
    with pytest.raises(ValueError, match="out must be"):
        fake.read_records(256, 0, 2, out=out)
    with pytest.raises(ValueError, match="out must be"):
        fake.read_records(256, 0, 3, out=out.astype(np.int8))
    with pytest.raises(TypeError, match="integers"):
        fake.read_records_at(256, [0.5], out=out)
    with pytest.raises(sa.SpiralGpuError, match="at most 16"):
        fake.read_records(17 * 8192, 0, 1)
    assert (out == 0xA5).all(), "nothing written"
