"""CPU-side checks of the pair form of the SpiralPack batch's shared pass (8 ciphertexts per slot, option "pack_pair_blocks"): the option is settable,
readable and bounded; spiral_gpu_pack_has_limb_form follows it at 8 ciphertexts per slot and nowhere else; the header documents it."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAIRS = [(7, 3), (9, 3), (12, 3)]                    # 8 ciphertexts per slot, first dimension 2^7 .. 2^12
NEVER = [(6, 3), (13, 3), (7, 2), (7, 1)]            # first dimension 64 or 8192; 4 and 2 ciphertexts per slot
ALWAYS = [(7, 4), (10, 8)]                           # the narrow and the wide form: not the option's business
OUT_N = [1, 2, 3, 12]


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


@pytest.fixture(scope="module")
def P(sa):
    return sys.modules["spiral_amd.pack"]


def test_option_is_settable_readable_and_bounded(sa, opts):
    assert sa.get_option("pack_pair_blocks") == 0  # the default
    opts(pack_pair_blocks=1)
    assert sa.get_option("pack_pair_blocks") == 1
    for bad in (2, -1):
        with pytest.raises(sa.SpiralGpuError, match="pack_pair_blocks"):
            sa.set_option("pack_pair_blocks", bad)
        assert sa.get_option("pack_pair_blocks") == 1  # a refused value changes nothing
    sa.set_option("pack_pair_blocks", 0)
    assert sa.get_option("pack_pair_blocks") == 0


@pytest.mark.parametrize("out_n", OUT_N)
def test_coverage_follows_the_option_at_8_columns_only(sa, P, opts, out_n):
    L = sa.lib()

    def has(nu1, nu2):
        p = sa.make_params(nu1, nu2)
        rc = L.spiral_gpu_pack_has_limb_form(C.byref(p), out_n)
        assert rc in (0, 1) and P.has_limb_form(p, out_n) is bool(rc), (nu1, nu2, out_n)
        return rc

    assert [has(*g) for g in PAIRS] == [0] * len(PAIRS)  # today's rule while the option is off
    assert [has(*g) for g in ALWAYS] == [1] * len(ALWAYS)
    opts(pack_pair_blocks=1)
    assert [has(*g) for g in PAIRS] == [1] * len(PAIRS)
    assert [has(*g) for g in NEVER] == [0] * len(NEVER)
    assert [has(*g) for g in ALWAYS] == [1] * len(ALWAYS)
    sa.set_option("pack_pair_blocks", 0)
    assert has(7, 3) == 0 and has(9, 3) == 0
    assert [has(*g) for g in NEVER] == [0] * len(NEVER)
    assert [has(*g) for g in ALWAYS] == [1] * len(ALWAYS)


def test_geometries_are_what_the_cases_say(sa):
    for nu1, nu2 in PAIRS[:2]:  # (nu1 = 12 needs a directly uploaded query: has_limb_form does not care how the query arrives)
        s = sa.get_pack_shape(sa.make_params(nu1, nu2), 2)
        assert s.num_per == 8 and s.dim0 == 1 << nu1
    assert sa.get_pack_shape(sa.make_params(7, 2), 2).num_per == 4


def test_header_documents_the_option():
    with open(os.path.join(ROOT, "include", "spiral_gpu.h")) as f:
        text = f.read()
    assert '"pack_pair_blocks"' in text
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "pack_pair_blocks" in f.read()
