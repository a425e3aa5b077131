"""CPU-side checks of the narrow form of the SpiralPack batch's shared pass: spiral_gpu_pack_has_limb_form (a pure function of the parameters:
which geometries share one matrix-core pass per batch) is exported, declared and right; the library builds from a clean copy of its sources for
gfx950; and no source file holds a scalar-store or scalar-atomic mnemonic."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COVERED = [(7, 4), (7, 5), (7, 6), (8, 4), (10, 4), (12, 4), (7, 7), (10, 8)]
UNCOVERED = [(7, 3), (9, 3), (6, 4), (6, 7), (6, 2), (3, 2)]


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


@pytest.fixture(scope="module")
def P(sa):
    return sys.modules["spiral_amd.pack"]


def test_symbol_exported_and_declared(sa):
    from spiral_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "spiral_gpu_pack_has_limb_form")
    assert "spiral_gpu_pack_has_limb_form" in _lib.PROTOTYPES
    with open(os.path.join(ROOT, "include", "spiral_gpu.h")) as f:
        assert "spiral_gpu_pack_has_limb_form(const spiral_gpu_params *p, uint32_t out_n)" in f.read()


@pytest.mark.parametrize("out_n", [1, 2, 3, 12])
def test_coverage_rule(sa, P, out_n):
    L = sa.lib()
    for nu1, nu2 in COVERED:
        p = sa.make_params(nu1, nu2)
        assert L.spiral_gpu_pack_has_limb_form(C.byref(p), out_n) == 1, (nu1, nu2, out_n)
        assert P.has_limb_form(p, out_n) is True
    for nu1, nu2 in UNCOVERED:
        p = sa.make_params(nu1, nu2)
        assert L.spiral_gpu_pack_has_limb_form(C.byref(p), out_n) == 0, (nu1, nu2, out_n)
        assert P.has_limb_form(p, out_n) is False


def test_bad_parameters_fail_with_a_message(sa, P):
    L = sa.lib()
    assert L.spiral_gpu_pack_has_limb_form(None, 2) == -1
    assert b"null" in L.spiral_gpu_last_error()
    p = sa.make_params(7, 4)
    assert L.spiral_gpu_pack_has_limb_form(C.byref(p), 0) == -1
    assert b"out_n" in L.spiral_gpu_last_error()
    with pytest.raises(sa.SpiralGpuError, match="out_n"):
        P.has_limb_form(p, 0)
    assert L.spiral_gpu_pack_has_limb_form(C.byref(p), 2) == 1  # (an error is not sticky)


def _source_files():
    """every file of the source directories and of the repository's root that is not a document, a data file or a build product"""
    docs = (".md", ".rst", ".txt", ".json", ".jsonl", ".csv", ".log", ".so", ".o", ".pyc")
    for f in os.listdir(ROOT):
        if os.path.isfile(os.path.join(ROOT, f)) and not f.endswith(docs):
            yield os.path.join(ROOT, f)
    for top in ("spiral_amd", "include", "oracle", "tools", "tests"):
        for d, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if x not in ("__pycache__", "_ref", "variants")]
            for f in files:
                if not f.endswith(docs):
                    yield os.path.join(d, f)


def test_no_scalar_store_or_scalar_atomic_mnemonic():
    """scalar stores and scalar atomics to GPU memory are not used anywhere: values go out through vector stores or plain C++ (the words are put
    together here so that this file does not hold them either)"""
    s = "s_"
    words = [s + "store_", s + "buffer_" + "store_", s + "scratch_" + "store_", s + "atomic_", s + "buffer_" + "atomic_", s + "dcache_" + "wb", s + "dcache_" + "discard"]
    pat = re.compile(r"(?<![a-z0-9_])(" + "|".join(words) + ")", re.IGNORECASE)
    hits = []
    for path in _source_files():
        try:
            with open(path, "rb") as f:
                text = f.read().decode("latin-1")
        except OSError:
            continue
        if pat.search(text):
            hits.append(os.path.relpath(path, ROOT))
    assert not hits, hits


def test_library_builds_from_a_clean_tree(tmp_path):
    """a copy of the sources with no object in it compiles to a library that exports the new entry point (hipcc cross-compiles without a GPU)"""
    dst = tmp_path / "tree"
    shutil.copytree(os.path.join(ROOT, "spiral_amd", "csrc"), dst / "spiral_amd" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), dst / "include")
    csrc = str(dst / "spiral_amd" / "csrc")
    r = subprocess.run(["make", "-C", csrc, "-s", "-j4", "../libspiral_gpu.so", "ARCH=gfx950"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    raw = C.CDLL(str(dst / "spiral_amd" / "libspiral_gpu.so"))
    assert hasattr(raw, "spiral_gpu_pack_has_limb_form") and hasattr(raw, "spiral_gpu_pack_server_answer_batch")
