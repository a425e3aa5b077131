"""CPU-side checks of the narrow base forms of the batch's shared pass (8, 16 and 32 ciphertexts per slot, option "sweep_narrow"): the option is
settable, readable and bounded; spiral_gpu_has_limb_form (and spiral_amd.has_limb_form) follows it below 64 ciphertexts per slot and nowhere else;
the header and the README document both."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NU1 = range(5, 13)
NU2 = range(0, 9)


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


def has(sa, nu1, nu2, j_begin=0, j_end=0):
    """the C call and the Python call, which must agree"""
    p = sa.make_params(nu1, nu2)
    rc = sa.lib().spiral_gpu_has_limb_form(C.byref(p), j_begin, j_end)
    assert rc in (0, 1) and sa.has_limb_form(p, j_begin, j_end) is bool(rc), (nu1, nu2, j_begin, j_end)
    return rc


def test_option_is_settable_readable_and_bounded(sa, opts):
    assert sa.get_option("sweep_narrow") == 0  # the default
    for start in (0, 1):
        opts(sweep_narrow=start)
        assert sa.get_option("sweep_narrow") == start
        for bad in (2, -1):
            with pytest.raises(sa.SpiralGpuError, match="sweep_narrow"):
                sa.set_option("sweep_narrow", bad)
            assert sa.get_option("sweep_narrow") == start  # a refused value changes nothing
    sa.set_option("sweep_narrow", 0)
    assert sa.get_option("sweep_narrow") == 0


def test_symbol_is_declared_and_exported(sa):
    from spiral_amd import _lib

    assert "spiral_gpu_has_limb_form" in _lib.PROTOTYPES and hasattr(sa.lib(), "spiral_gpu_has_limb_form")
    assert "has_limb_form" in dir(sa)


def test_coverage_with_the_option_off_is_todays_rule(sa, opts):
    opts(sweep_narrow=0)
    for nu1 in NU1:
        for nu2 in NU2:
            assert has(sa, nu1, nu2) == int(6 <= nu1 <= 11 and nu2 >= 6), (nu1, nu2)


def test_coverage_with_the_option_on_adds_8_16_32_per_slot(sa, opts):
    opts(sweep_narrow=1)
    for nu1 in NU1:
        for nu2 in NU2:
            assert has(sa, nu1, nu2) == int(6 <= nu1 <= 11 and nu2 >= 3), (nu1, nu2)
    for nu2 in (0, 1, 2):  # never below 8 ciphertexts per slot
        assert has(sa, 8, nu2) == 0
    for nu2 in NU2:  # nor at a first dimension of 32 or 4096
        assert has(sa, 5, nu2) == 0 and has(sa, 12, nu2) == 0
    sa.set_option("sweep_narrow", 0)
    assert [has(sa, 8, nu2) for nu2 in (3, 4, 5, 6)] == [0, 0, 0, 1]


@pytest.mark.parametrize("narrow,nu2", [(1, 3), (1, 4), (1, 5), (0, 6), (1, 6)])
def test_shards(sa, opts, narrow, nu2):
    """at nu1 = 7 the shard [0, 64) has the form and [0, 96) (not a power of two) has not; (0, 0) is the whole first dimension"""
    opts(sweep_narrow=narrow)
    assert has(sa, 7, nu2, 0, 64) == 1 and has(sa, 7, nu2, 64, 128) == 1
    assert has(sa, 7, nu2, 0, 96) == 0
    assert has(sa, 7, nu2, 0, 0) == has(sa, 7, nu2, 0, 128) == 1
    assert has(sa, 7, nu2, 0, 32) == 0  # a shard of 32


def test_bad_arguments(sa):
    L = sa.lib()
    p = sa.make_params(7, 4)
    assert L.spiral_gpu_has_limb_form(None, 0, 0) == -1
    assert L.spiral_gpu_has_limb_form(C.byref(p), 64, 64) == -1 and b"shard" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_has_limb_form(C.byref(p), 0, 129) == -1
    with pytest.raises(sa.SpiralGpuError, match="shard"):
        sa.has_limb_form(p, 5, 3)
    assert L.spiral_gpu_has_limb_form(C.byref(p), 0, 0) == 0  # (an error is not sticky)
    # how the query arrives is not the image's business: nu1 = 11 needs a direct upload to be served, the form exists either way
    assert has(sa, 11, 6) == 1 and L.spiral_gpu_has_limb_form(C.byref(sa.make_params(11, 6, direct_upload=1)), 0, 0) == 1


def test_header_and_readme_document_option_and_call():
    for path in (os.path.join(ROOT, "include", "spiral_gpu.h"), os.path.join(ROOT, "README.md")):
        with open(path) as f:
            text = f.read()
        assert '"sweep_narrow"' in text, path
        assert "spiral_gpu_has_limb_form" in text, path
    with open(os.path.join(ROOT, "include", "spiral_gpu.h")) as f:
        assert "int spiral_gpu_has_limb_form(const spiral_gpu_params *p, uint32_t j_begin, uint32_t j_end);" in f.read()
