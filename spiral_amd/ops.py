"""Function-level mirror of the reference's hot-path interface (host numpy buffers in reference
layouts), each a direct call through the C ABI.  See include/spiral_gpu.h for the reference citations."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import SEED_BYTES, SEED_PACK_PUB_PARAMS, SEED_PACK_QUERY, SEED_PUB_PARAMS, SEED_QUERY, WIRE_POLY_BYTES, U64P, Params, Shape, check, lib, wire_bytes

N = 2048
P = 268369921
B = 249561089
Q = P * B

__all__ = [
    "N", "P", "B", "Q", "make_params", "get_shape", "has_limb_form", "column_shard_has_limb_form", "get_tables", "ntt_forward", "ntt_inverse", "to_ntt", "to_ntt_no_reduce", "from_ntt",
    "multiply", "add", "mul_by_const", "automorph", "invert", "gadget_invert", "getRescaled", "multiplyQueryByDatabase", "multiplyQueriesByDatabase", "split_and_crt",
    "foldOneFurtherDimension", "expandImproved", "scalToMat", "regevToGSW", "time_ntt", "time_ntt_digits", "response_wire_bytes", "response_from_wire",
    "query_wire_bytes", "pub_params_wire_bytes", "pack_query_wire_bytes", "pack_pub_params_wire_bytes", "raw_to_wire", "raw_from_wire",
    "query_seeded_bytes", "pub_params_seeded_bytes", "pack_query_seeded_bytes", "pack_pub_params_seeded_bytes", "seed_expand",
    "SEED_BYTES", "SEED_QUERY", "SEED_PUB_PARAMS", "SEED_PACK_QUERY", "SEED_PACK_PUB_PARAMS",
    "set_option", "get_option", "options",
]


def _p(a: np.ndarray):
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(U64P)


def _c(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64)


def set_option(name: str, value: int) -> None:
    """spiral_gpu_set_option: a process-wide schedule option (include/spiral_gpu.h lists them); servers take the values in force at creation"""
    check(lib().spiral_gpu_set_option(name.encode(), int(value)))


def get_option(name: str) -> int:
    v = C.c_int64()
    check(lib().spiral_gpu_get_option(name.encode(), C.byref(v)))
    return v.value


class options:
    """with sa.options(fold_pair=0, fwd2=1): ...  -- sets the options and restores the previous values on exit"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            set_option(k, v)
        return False


def make_params(nu1, nu2, t_gsw=8, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=20, p_db=256, direct_upload=0) -> Params:
    return Params(nu1, nu2, t_gsw, t_conv, t_exp, t_exp_right, qprime_bits, direct_upload, p_db)


def get_shape(p: Params) -> Shape:
    s = Shape()
    check(lib().spiral_gpu_get_shape(C.byref(p), C.byref(s)))
    return s


def has_limb_form(p: Params, j_begin: int = 0, j_end: int = 0) -> bool:
    """whether a server of these parameters on the first-dimension shard [j_begin, j_end) ((0, 0): all of it) may hold its database as limb planes, so
    that a batch (run_query_batch) shares ONE matrix-core pass over it: a shard that is a power of two in [64, 2048] and at least 64 ciphertexts per
    slot -- or 8, 16 or 32 while option "sweep_narrow" is 1 (set_option; default 0).  A function of the parameters and of that one option as it is
    now: no GPU needed."""
    rc = lib().spiral_gpu_has_limb_form(C.byref(p), j_begin, j_end)
    if rc < 0:
        check(rc)
    return bool(rc)


def column_shard_has_limb_form(p: Params, n_ranks: int) -> bool:
    """has_limb_form for the image of a column shard of n_ranks ranks (Server(..., col_rank=, col_ranks=)): num_per / n_ranks ciphertexts per slot and
    the whole first dimension, i.e. has_limb_form of the parameters with nu2 - log2 n_ranks; the same rule, the same option "sweep_narrow", no GPU
    needed.  A rank count that gives no shard (not a power of two, more ranks than columns) has no image: False, and last_error says why"""
    rc = lib().spiral_gpu_column_shard_has_limb_form(C.byref(p), n_ranks)
    if rc < 0:
        check(rc)
    return bool(rc)


def get_tables() -> np.ndarray:
    out = np.zeros((8, N), dtype=np.uint64)
    check(lib().spiral_gpu_get_tables(_p(out)))
    return out


def ntt_forward(operand) -> np.ndarray:
    """ntt_forward (src/core.cpp:247) on [..., 2, N]; returns a new array"""
    x = _c(operand).copy()
    check(lib().spiral_gpu_ntt_forward(_p(x), x.size // (2 * N)))
    return x


def ntt_inverse(operand) -> np.ndarray:
    x = _c(operand).copy()
    check(lib().spiral_gpu_ntt_inverse(_p(x), x.size // (2 * N)))
    return x


def to_ntt(raw) -> np.ndarray:
    raw = _c(raw)
    out = np.zeros(raw.shape[:-1] + (2, N), dtype=np.uint64)
    check(lib().spiral_gpu_to_ntt(_p(out), _p(raw), raw.size // N, 1))
    return out


def to_ntt_no_reduce(raw) -> np.ndarray:
    raw = _c(raw)
    out = np.zeros(raw.shape[:-1] + (2, N), dtype=np.uint64)
    check(lib().spiral_gpu_to_ntt(_p(out), _p(raw), raw.size // N, 0))
    return out


def from_ntt(a) -> np.ndarray:
    a = _c(a)
    out = np.zeros(a.shape[:-2] + (N,), dtype=np.uint64)
    check(lib().spiral_gpu_from_ntt(_p(out), _p(a), a.size // (2 * N)))
    return out


def multiply(a, b) -> np.ndarray:
    a, b = _c(a), _c(b)
    rs, ms, cs = a.shape[0], a.shape[1], b.shape[1]
    assert b.shape[0] == ms
    out = np.zeros((rs, cs, 2, N), dtype=np.uint64)
    check(lib().spiral_gpu_multiply(_p(out), _p(a), _p(b), rs, ms, cs))
    return out


def add(a, b) -> np.ndarray:
    a, b = _c(a), _c(b)
    out = np.zeros_like(a)
    check(lib().spiral_gpu_add(_p(out), _p(a), _p(b), a.size // (2 * N)))
    return out


def mul_by_const(single, a) -> np.ndarray:
    single, a = _c(single), _c(a)
    out = np.zeros_like(a)
    check(lib().spiral_gpu_mul_by_const(_p(out), _p(single), _p(a), a.size // (2 * N)))
    return out


def automorph(raw, t) -> np.ndarray:
    raw = _c(raw)
    out = np.zeros_like(raw)
    check(lib().spiral_gpu_automorph(_p(out), _p(raw), raw.size // N, int(t)))
    return out


def invert(raw) -> np.ndarray:
    raw = _c(raw)
    out = np.zeros_like(raw)
    check(lib().spiral_gpu_invert(_p(out), _p(raw), raw.size // N))
    return out


def gadget_invert(raw, mx, rdim) -> np.ndarray:
    raw = _c(raw)
    cols = raw.shape[1]
    out = np.zeros((mx, cols, N), dtype=np.uint64)
    check(lib().spiral_gpu_gadget_invert(_p(out), _p(raw), mx, rdim, cols))
    return out


def getRescaled(a, inp_mod, out_mod) -> np.ndarray:
    a = _c(a)
    out = np.zeros_like(a)
    check(lib().spiral_gpu_get_rescaled(_p(out), _p(a), a.size, int(inp_mod), int(out_mod)))
    return out


def response_wire_bytes(params, out_n: int = 2) -> int:
    """size of a response's wire form (include/spiral_gpu.h): the "Response size" of the reference's summary"""
    return int(lib().spiral_gpu_response_wire_bytes(C.byref(params), out_n))


def response_from_wire(params, wire, out_n: int = 2) -> np.ndarray:
    """client half of the wire form (load_modswitched_into_ct, src/client.cpp:90): bytes -> [(out_n+1)][out_n][N] values; host code"""
    wire = np.ascontiguousarray(wire, dtype=np.uint8)
    assert wire.size >= response_wire_bytes(params, out_n)
    out = np.zeros((out_n + 1, out_n, N), dtype=np.uint64)
    check(lib().spiral_gpu_response_from_wire(C.byref(params), out_n, wire.ctypes.data_as(C.c_void_p), _p(out)))
    return out


def query_wire_bytes(params) -> int:
    """size of a query's wire form (include/spiral_gpu.h): n_query_cts ciphertexts n0 x 1 at 7 bytes per coefficient; 0 for refused parameters"""
    return int(lib().spiral_gpu_query_wire_bytes(C.byref(params)))


def pub_params_wire_bytes(params) -> int:
    """size of the public parameters' wire form (W_exp_left, W_exp_right, W, V in one message); 0 for refused parameters"""
    return int(lib().spiral_gpu_pub_params_wire_bytes(C.byref(params)))


def pack_query_wire_bytes(params, out_n: int) -> int:
    """SpiralPack: size of a query's wire form; 0 for refused parameters"""
    return int(lib().spiral_gpu_pack_query_wire_bytes(C.byref(params), int(out_n)))


def pack_pub_params_wire_bytes(params, out_n: int) -> int:
    """SpiralPack: size of the public parameters' wire form (W_exp_left, W_exp_right, V, v_W in one message); 0 for refused parameters"""
    return int(lib().spiral_gpu_pack_pub_params_wire_bytes(C.byref(params), int(out_n)))


def raw_to_wire(raw) -> np.ndarray:
    """the client's half of the wire form: raw polynomials (values in [0, Q], 2048 per polynomial) -> 7 bytes per coefficient, uint8; host code.
    A value above Q is refused (SpiralGpuError naming it)"""
    raw = _c(raw)
    if raw.size % N:
        raise ValueError(f"raw_to_wire: {raw.size} values are not whole polynomials of {N}")
    out = np.zeros(raw.size // N * WIRE_POLY_BYTES, dtype=np.uint8)
    check(lib().spiral_gpu_raw_to_wire(_p(raw), raw.size // N, out.ctypes.data_as(C.c_void_p)))
    return out


def raw_from_wire(wire) -> np.ndarray:
    """the converse: a wire message -> [npolys][2048] raw values; host code"""
    wire = wire_bytes(wire)
    if wire.size % WIRE_POLY_BYTES:
        raise ValueError(f"raw_from_wire: {wire.size} bytes are not whole polynomials of {WIRE_POLY_BYTES}")
    out = np.zeros((wire.size // WIRE_POLY_BYTES, N), dtype=np.uint64)
    check(lib().spiral_gpu_raw_from_wire(wire.ctypes.data_as(C.c_void_p), out.shape[0], _p(out)))
    return out


def query_seeded_bytes(params) -> int:
    """size of a query's seeded form (include/spiral_gpu.h): the 32-byte seed and row 1 of each ciphertext in its wire form; 0 for refused parameters"""
    return int(lib().spiral_gpu_query_seeded_bytes(C.byref(params)))


def pub_params_seeded_bytes(params) -> int:
    """size of the public parameters' seeded form (the wire message less every matrix's row 0, after a seed); 0 for refused parameters"""
    return int(lib().spiral_gpu_pub_params_seeded_bytes(C.byref(params)))


def pack_query_seeded_bytes(params, out_n: int) -> int:
    """SpiralPack: size of a query's seeded form; 0 for refused parameters"""
    return int(lib().spiral_gpu_pack_query_seeded_bytes(C.byref(params), int(out_n)))


def pack_pub_params_seeded_bytes(params, out_n: int) -> int:
    """SpiralPack: size of the public parameters' seeded form; 0 for refused parameters"""
    return int(lib().spiral_gpu_pack_pub_params_seeded_bytes(C.byref(params), int(out_n)))


def seed_expand(seed, domain: int, first_k: int, npolys: int) -> np.ndarray:
    """the client's half of the seeded form: row-0 polynomials first_k .. first_k + npolys - 1 of `domain` (SEED_QUERY ...) under the 32-byte seed,
    [npolys][2][2048] uint64 in the reference's NTT layout (residues mod p, then mod b); host code"""
    seed = wire_bytes(seed)
    if seed.size != SEED_BYTES:
        raise ValueError(f"seed_expand: a seed is {SEED_BYTES} bytes, not {seed.size}")
    out = np.zeros((int(npolys), 2, N), dtype=np.uint64)
    check(lib().spiral_gpu_seed_expand(seed.ctypes.data_as(C.c_void_p), int(domain), int(first_k), int(npolys), _p(out)))
    return out


def multiplyQueryByDatabase(reoriented_cts, database, dim0, num_per) -> np.ndarray:
    out = np.zeros((num_per, 3, 2, 2, N), dtype=np.uint64)
    check(lib().spiral_gpu_multiply_query_by_database(_p(out), _p(_c(reoriented_cts)), _p(_c(database)), dim0, num_per))
    return out


def multiplyQueriesByDatabase(reoriented_cts_list, database, dim0, num_per) -> np.ndarray:
    """n <= 8 queries against one pass over the database (the matrix-core sweep where the geometry allows): [n][num_per][3][2][2][N]"""
    n = len(reoriented_cts_list)
    re = np.ascontiguousarray(np.stack([_c(r).reshape(-1) for r in reoriented_cts_list]))
    out = np.zeros((n, num_per, 3, 2, 2, N), dtype=np.uint64)
    check(lib().spiral_gpu_multiply_queries_by_database(_p(out), _p(re), n, _p(_c(database)), dim0, num_per))
    return out


def split_and_crt(raw_cts, t_gsw) -> np.ndarray:
    raw_cts = _c(raw_cts)
    num_per = raw_cts.shape[0]
    out = np.zeros((num_per, 3 * t_gsw, 2, 2, N), dtype=np.uint64)
    check(lib().spiral_gpu_split_and_crt(_p(out), _p(raw_cts), num_per, t_gsw))
    return out


def foldOneFurtherDimension(cts, num_per, query_ct, query_ct_neg, t_gsw) -> np.ndarray:
    """returns the num_per folded raw ciphertexts (the reference overwrites the first half in place)"""
    x = _c(cts).copy()
    check(lib().spiral_gpu_fold_one_further_dimension(_p(x), num_per, _p(_c(query_ct)), _p(_c(query_ct_neg)), t_gsw))
    return x[:num_per]


def expandImproved(cv_v, g, m_exp, W_left, W_right, m_exp_right, n_right, max_bits_to_gen_right, stopround) -> np.ndarray:
    x = _c(cv_v).copy()
    check(lib().spiral_gpu_expand_improved(_p(x), g, m_exp, _p(_c(W_left)), m_exp_right, _p(_c(W_right)), n_right, max_bits_to_gen_right, stopround))
    return x


def scalToMat(m_conv, cv, W) -> np.ndarray:
    out = np.zeros((3, 2, 2, N), dtype=np.uint64)
    check(lib().spiral_gpu_scal_to_mat(_p(out), _p(_c(cv)), _p(_c(W)), m_conv))
    return out


def regevToGSW(m_conv, t, cv_v, W, V) -> np.ndarray:
    out = np.zeros((3, 3 * t, 2, N), dtype=np.uint64)
    check(lib().spiral_gpu_regev_to_gsw(_p(out), _p(_c(cv_v)), _p(_c(W)), _p(_c(V)), m_conv, t))
    return out


def time_ntt(npolys: int, iters: int = 10):
    """average ms of one batched to_ntt / from_ntt launch over npolys polynomials resident in HBM -> (fwd_ms, inv_ms)"""
    f, i = C.c_float(), C.c_float()
    check(lib().spiral_gpu_time_ntt(npolys, iters, C.byref(f), C.byref(i)))
    return f.value, i.value


def time_ntt_digits(npolys: int, n_digits: int, iters: int = 10) -> float:
    """ms per launch of npolys * n_digits gadget-digit transforms (the launch the conversion / expansion stages are made of)"""
    ms = C.c_float()
    check(lib().spiral_gpu_time_ntt_digits(npolys, n_digits, iters, C.byref(ms)))
    return ms.value
