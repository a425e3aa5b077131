"""CPU-side checks of the key store (include/spiral_gpu.h spiral_gpu_key_store_*, spiral_amd/keys.py): the library exports and declares every new
symbol with its signature, the slot sizes are the figures the message layouts give, bad parameters are refused without a device, and ./spiral parses
--key-store before it looks for one."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spiral_amd", "spiral")
N = 2048
POLY_BYTES = 8 * N  # one polynomial in the device layout: 16 KiB
WIRE_POLY = 7 * N
NEW_SYMBOLS = {
    "spiral_gpu_key_store_create": 6, "spiral_gpu_key_store_destroy": 1, "spiral_gpu_key_store_slot_bytes": 3, "spiral_gpu_key_store_put": 6,
    "spiral_gpu_key_store_put_wire": 4, "spiral_gpu_key_store_put_seeded": 4, "spiral_gpu_key_store_drop": 2, "spiral_gpu_key_store_has": 2,
    "spiral_gpu_server_bind_keys": 4, "spiral_gpu_pack_server_bind_keys": 4,
}
CONFIG1 = dict(nu1=8, nu2=7, t_gsw=8, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=20, p_db=256)  # bench.py's configs[1]


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


def test_new_symbols_exported_and_declared(sa):
    from spiral_amd import _lib, keys
    from spiral_amd import pack as _  # noqa: F401

    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "spiral_gpu.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs, name
        assert name + "(" in header, name
    assert _lib.PROTOTYPES["spiral_gpu_key_store_slot_bytes"][0] is C.c_size_t
    assert "SPIRAL_GPU_KEYS_FULL 0" in header and "SPIRAL_GPU_KEYS_COMPACT 1" in header and '"key_binds"' in header
    assert (keys.FULL, keys.COMPACT) == (0, 1)
    assert sa.KeyStore is keys.KeyStore and sa.bind_keys is keys.bind_keys
    assert list(inspect.signature(keys.KeyStore.__init__).parameters) == ["self", "params", "capacity", "out_n", "form", "device"]
    sig = inspect.signature(keys.KeyStore.__init__).parameters
    assert (sig["out_n"].default, sig["form"].default, sig["device"].default) == (0, "full", 0)
    for f in ("put", "put_wire", "put_seeded", "drop", "has", "slot_bytes", "close"):
        assert callable(getattr(keys.KeyStore, f)), f
    assert list(inspect.signature(sa.bind_keys).parameters) == ["servers", "store", "slots"]
    pack = sys.modules["spiral_amd.pack"]
    assert list(inspect.signature(pack.bind_keys).parameters) == ["servers", "store", "slots"]
    assert sa.get_option("key_binds") >= 0  # (read only)
    with pytest.raises(sa.SpiralGpuError):
        sa.set_option("key_binds", 1)


def test_slot_bytes(sa):
    """FULL: every polynomial of the message (the wire form's count) x 16 KiB, the words the server's arena carves for its four key buffers.
    COMPACT: the polynomials the seeded form sends x 16 KiB, plus the 32-byte seed padded to one 256-byte piece"""
    from spiral_amd import keys

    p1 = sa.make_params(**CONFIG1)
    polys, sent = sa.pub_params_wire_bytes(p1) // WIRE_POLY, (sa.pub_params_seeded_bytes(p1) - 32) // WIRE_POLY
    s = sa.get_shape(p1)
    assert polys == s.n_left * 2 * 8 + s.n_right * 2 * 56 + 2 * 3 * 2 * 4 == 976 and sent == 496
    assert keys.slot_bytes(p1, 0, "full") == polys * POLY_BYTES == 15_990_784
    assert keys.slot_bytes(p1, 0, "compact") == 256 + sent * POLY_BYTES == 8_126_720
    assert keys.slot_bytes(p1, 0, keys.COMPACT) == keys.slot_bytes(p1, form="compact")
    # SpiralPack, compressed (expansion keys, V, v_W) and streaming (v_W only)
    pk = sa.make_params(10, 8, t_gsw=8, t_conv=4, t_exp=16, t_exp_right=56, qprime_bits=20, p_db=256)
    ps = sa.get_pack_shape(pk, 4)
    polys = ps.n_left * 2 * 16 + ps.n_right * 2 * 56 + 2 * 2 * 4 + 4 * 5 * 4
    assert sa.pack_pub_params_wire_bytes(pk, 4) == polys * WIRE_POLY
    assert keys.slot_bytes(pk, 4, "full") == polys * POLY_BYTES
    assert keys.slot_bytes(pk, 4, "compact") == 256 + (sa.pack_pub_params_seeded_bytes(pk, 4) - 32) // WIRE_POLY * POLY_BYTES
    pst = sa.make_params(8, 4, t_gsw=5, t_conv=4, t_exp=2, qprime_bits=20, p_db=256, direct_upload=1)
    assert keys.slot_bytes(pst, 2, "full") == 2 * 3 * 4 * POLY_BYTES and keys.slot_bytes(pst, 2, "compact") == 256 + 2 * 2 * 4 * POLY_BYTES
    # the base path and SpiralPack hold different messages for the same parameters
    assert keys.slot_bytes(pk, 0, "full") != keys.slot_bytes(pk, 4, "full")


def test_bad_parameters_refused_without_a_device(sa):
    from spiral_amd import keys

    L = sa.lib()
    p1 = sa.make_params(**CONFIG1)
    for bad, out_n, form, msg in [(sa.make_params(8, 7, t_gsw=1), 0, 0, "gadget dimension"), (sa.make_params(8, 7, qprime_bits=3), 0, 1, "q' bit width"),
                                  (p1, 17, 0, "out_n out of range"), (p1, 0, 2, "unknown slot form 2"), (p1, 0, -1, "unknown slot form")]:
        assert L.spiral_gpu_key_store_slot_bytes(C.byref(bad), out_n, form) == 0
        assert msg in L.spiral_gpu_last_error().decode(), msg
    assert L.spiral_gpu_key_store_slot_bytes(None, 0, 0) == 0 and "null" in L.spiral_gpu_last_error().decode()
    with pytest.raises(sa.SpiralGpuError, match="gadget dimension"):
        keys.slot_bytes(sa.make_params(8, 7, t_gsw=1))
    with pytest.raises(ValueError, match="'full' or 'compact'"):
        keys.slot_bytes(p1, 0, "packed")
    # null handles are refused, not dereferenced
    h = C.c_void_p()
    assert L.spiral_gpu_key_store_create(None, 0, 0, 1, 0, C.byref(h)) != 0 and "null" in L.spiral_gpu_last_error().decode()
    assert L.spiral_gpu_key_store_create(C.byref(p1), 0, 0, 0, 0, C.byref(h)) != 0 and "capacity" in L.spiral_gpu_last_error().decode()
    assert L.spiral_gpu_key_store_put_seeded(None, 0, None, 0) != 0 and "null key store" in L.spiral_gpu_last_error().decode()
    assert L.spiral_gpu_key_store_drop(None, 0) != 0
    assert L.spiral_gpu_key_store_has(None, 0) == 0
    L.spiral_gpu_key_store_destroy(None)
    assert L.spiral_gpu_server_bind_keys(None, 1, None, None) != 0 and "no servers" in L.spiral_gpu_last_error().decode()
    assert L.spiral_gpu_pack_server_bind_keys(None, 1, None, None) != 0 and "no servers" in L.spiral_gpu_last_error().decode()


def test_cli_parses_key_store(sa):
    """--key-store [compact] is taken by the argument parser (it announces the store, then looks for a device or runs); without a valid --batch, or
    with --instances / --high-rate, it is refused before that"""
    for extra, form in ([], "full"), (["compact"], "compact"):
        r = subprocess.run([BIN, "4", "3", "40", "a", "--batch", "3", "--key-store"] + extra, capture_output=True, text=True, timeout=300)
        assert f"Binding the batch's keys from a key store ({form} slots)" in r.stdout, r.stdout + r.stderr
        assert "--key-store takes" not in r.stderr
        assert r.returncode == 0 or "no ROCm device" in r.stderr, r.stdout[-1000:] + r.stderr
    for flags in (["--key-store"], ["--batch", "9", "--key-store"], ["--batch", "3", "--instances", "2", "--key-store", "compact"],
                  ["--high-rate", "--batch", "3", "--key-store"]):
        r = subprocess.run([BIN, "4", "3", "40", "a"] + flags, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--key-store takes" in r.stderr, (flags, r.stdout + r.stderr)
