"""Client session: one client's secret key resident on the device, drawn from a 32-byte seed; its public parameters and batches of its queries in the
forms the server ingests (NTT, wire, seeded), and the decoding of batches of responses in one launch (include/spiral_gpu.h, spiral_gpu_client_*; the
format of the randomness: csrc/client_device.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import FORM_NTT, FORM_SEEDED, FORM_WIRE, PackShape, Params, Shape, U64P, check, kv_keys, kv_layout_for, kv_table_key, lib, read_ids, record_layout, wire_bytes

N = 2048
RESPONSE_RAW, RESPONSE_WIRE = 0, 1  # spiral_gpu_response_form
RESPONSE_FINAL = 2  # SPIRAL_GPU_RESPONSE_FINAL: response_noise alone
Q = 268369921 * 249561089
_FORMS = {"raw": RESPONSE_RAW, "wire": RESPONSE_WIRE}
_NOISE_FORMS = {"raw": RESPONSE_RAW, "wire": RESPONSE_WIRE, "final": RESPONSE_FINAL}
_MESSAGE_FORMS = {"ntt": FORM_NTT, "wire": FORM_WIRE, "seeded": FORM_SEEDED}


def _message_form(form) -> int:
    if form not in _MESSAGE_FORMS:
        raise ValueError(f"message form {form!r}: 'ntt', 'wire' or 'seeded'")
    return _MESSAGE_FORMS[form]


def client_noise_table() -> np.ndarray:
    """the 128 thresholds T[i] = floor(2^64 C_i / C_128) of the session's noise sampler (plain host code, no device)"""
    out = np.zeros(128, dtype=np.uint64)
    check(lib().spiral_gpu_client_noise_table(out.ctypes.data_as(U64P)))
    return out


class Client:
    def __init__(self, params: Params, seed, out_n: int = 0, device: int = 0, nonoise: bool = False):
        """a session for `params` (out_n = 0: base Spiral, else SpiralPack with that out_n) on `device`, its secret key drawn from the 32-byte `seed`"""
        seed = bytes(seed)
        if len(seed) != 32:
            raise ValueError(f"a client seed is 32 bytes, not {len(seed)}")
        self.params, self.out_n, self.device, self.nonoise = params, out_n, device, bool(nonoise)
        self.rows = self.cols = out_n if out_n else 2
        L = lib()
        if out_n:
            sh = PackShape()
            check(L.spiral_gpu_pack_get_shape(C.byref(params), out_n, C.byref(sh)))
            ex = 0 if params.direct_upload else 1
            # (count, rows, cols) of W_exp_left, W_exp_right, V, v_W
            self.parts = [(ex * sh.n_left, 2, params.t_exp), (ex * sh.n_right, 2, params.t_exp_right), (ex, 2, 2 * params.t_conv), (out_n, out_n + 1, params.t_conv)]
            sizes = lambda kind: getattr(L, f"spiral_gpu_pack_{kind}_bytes")(C.byref(params), out_n)  # noqa: E731
        else:
            sh = Shape()
            check(L.spiral_gpu_get_shape(C.byref(params), C.byref(sh)))
            # W_exp_left, W_exp_right, W, V
            self.parts = [(sh.n_left, 2, params.t_exp), (sh.n_right, 2, params.t_exp_right), (1, 3, 2 * params.t_conv), (1, 3, 2 * params.t_conv)]
            sizes = lambda kind: getattr(L, f"spiral_gpu_{kind}_bytes")(C.byref(params))  # noqa: E731
        self.shape = sh
        self.n_items = sh.dim0 * sh.num_per
        self._bytes = {("pub_params", FORM_WIRE): sizes("pub_params_wire"), ("pub_params", FORM_SEEDED): sizes("pub_params_seeded"),
                       ("query", FORM_WIRE): sizes("query_wire"), ("query", FORM_SEEDED): sizes("query_seeded"),
                       ("query", FORM_NTT): sh.n_query_cts * 2 * 2 * N * 8}
        h = C.c_void_p()
        check(lib().spiral_gpu_client_create(C.byref(params), out_n, device, seed, 1 if nonoise else 0, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().spiral_gpu_client_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def secret(self):
        """(sr [2048], Sp [rows][2048]) as raw values mod Q"""
        sr, sp = np.zeros(N, dtype=np.uint64), np.zeros((self.rows, N), dtype=np.uint64)
        check(lib().spiral_gpu_client_get_secret(self.h, sr.ctypes.data_as(U64P), sp.ctypes.data_as(U64P)))
        return sr, sp

    def set_secret(self, sr, sp):
        """replace the secret key: raw values mod Q, every coefficient in [-64, 64]"""
        sr, sp = np.ascontiguousarray(sr, dtype=np.uint64), np.ascontiguousarray(sp, dtype=np.uint64)
        if sr.size != N or sp.size != self.rows * N:
            raise ValueError(f"sr holds {sr.size} and Sp {sp.size} coefficients, the session's key takes {N} and {self.rows * N}")
        check(lib().spiral_gpu_client_set_secret(self.h, sr.ctypes.data_as(U64P), sp.ctypes.data_as(U64P)))

    @property
    def counter(self) -> int:
        """the message number the next query takes (the public parameters are message 0)"""
        n = C.c_uint64()
        check(lib().spiral_gpu_client_get_counter(self.h, C.byref(n)))
        return int(n.value)

    @counter.setter
    def counter(self, n: int):
        check(lib().spiral_gpu_client_set_counter(self.h, int(n)))

    def pub_params(self, form="ntt"):
        """form "ntt": the four arrays set_pub_params takes, [count][rows][cols][2][2048] each (an absent matrix: one zero word); "wire" / "seeded":
        the one message set_pub_params_wire / _seeded and the key store take, as a uint8 array.  Always message 0: every form holds the same matrices"""
        f = _message_form(form)
        if f == FORM_NTT:
            arrs = [np.zeros((n, r, c, 2, N), dtype=np.uint64) if n else np.zeros(1, dtype=np.uint64) for n, r, c in self.parts]
            check(lib().spiral_gpu_client_pub_params(self.h, *[a.ctypes.data_as(U64P) if a.size > 1 else None for a in arrs]))
            return tuple(arrs)
        msg = np.zeros(self._bytes["pub_params", f], dtype=np.uint8)
        check(lib().spiral_gpu_client_pub_params_msg(self.h, f, msg.ctypes.data_as(C.c_void_p), msg.size))
        return msg

    def queries(self, idx, form="seeded") -> np.ndarray:
        """one query per item index of idx, each under the next message number, from one launch sequence: form "ntt", an array
        [n][n_query_cts][2][1][2][2048] (a row is what set_query takes); "wire" / "seeded", a uint8 array [n][bytes] of messages"""
        f = _message_form(form)
        ids = np.ascontiguousarray(idx, dtype=np.uint64).reshape(-1)
        each = self._bytes["query", f]
        out = np.zeros((ids.size, each), dtype=np.uint8)
        check(lib().spiral_gpu_client_queries(self.h, ids.ctypes.data_as(U64P), ids.size, f, out.ctypes.data_as(C.c_void_p), each))
        return out.view(np.uint64).reshape(ids.size, self.shape.n_query_cts, 2, 1, 2, N) if f == FORM_NTT else out

    def query(self, idx: int, form="seeded") -> np.ndarray:
        return self.queries([idx], form)[0]

    def response_wire_bytes(self) -> int:
        return int(lib().spiral_gpu_response_wire_bytes(C.byref(self.params), self.cols))

    def decode(self, responses, form="raw") -> np.ndarray:
        """the plaintexts [n][rows][cols][2048] of n responses: form "raw", an array [n][(rows + 1)][cols][2048] (or one response) of switched
        responses; form "wire", n bit-packed responses back to back (bytes or a uint8 array), as read_response_wire_batch returns them"""
        if form not in _FORMS:
            raise ValueError(f"response form {form!r}: 'raw' or 'wire'")
        if form == "raw":
            buf = np.ascontiguousarray(responses, dtype=np.uint64)
            each = (self.rows + 1) * self.cols * N
        else:
            buf = wire_bytes(responses)
            each = self.response_wire_bytes()
        if buf.size == 0 or buf.size % each:
            raise ValueError(f"{buf.size} {'words' if form == 'raw' else 'bytes'} are no whole number of responses of {each}")
        n = buf.size // each
        out = np.zeros((n, self.rows, self.cols, N), dtype=np.uint64)
        check(lib().spiral_gpu_client_decode(self.h, buf.ctypes.data_as(C.c_void_p), n, _FORMS[form], out.ctypes.data_as(U64P)))
        return out

    # ---- records of any byte size (include/spiral_gpu.h "Records"; the base layout, or SpiralPack's for a session with out_n >= 1) ----
    def record_queries(self, record_ids, record_bytes: int, form="seeded") -> np.ndarray:
        """queries() for the items the records live in: one query per record (it serves every instance of a record of several)"""
        f = _message_form(form)
        ids = read_ids(record_ids)
        each = self._bytes["query", f]
        out = np.zeros((ids.size, each), dtype=np.uint8)
        check(lib().spiral_gpu_client_record_queries(self.h, record_bytes, ids.ctypes.data_as(U64P), ids.size, f, out.ctypes.data_as(C.c_void_p), each))
        return out.view(np.uint64).reshape(ids.size, self.shape.n_query_cts, 2, 1, 2, N) if f == FORM_NTT else out

    def decode_records(self, responses, record_ids, record_bytes: int, form="raw") -> np.ndarray:
        """the records record_ids[k] as a uint8 array [n][record_bytes] from n x instances responses laid out [record][instance], in decode()'s forms:
        bit for bit decode() followed by packing at w bits and cutting out each record's range, done per touched output polynomial on the device"""
        if form not in _FORMS:
            raise ValueError(f"response form {form!r}: 'raw' or 'wire'")
        lay = record_layout(self.params, record_bytes, self.out_n)
        ids = read_ids(record_ids)
        if form == "raw":
            buf = np.ascontiguousarray(responses, dtype=np.uint64)
            each = (self.rows + 1) * self.cols * N
        else:
            buf = wire_bytes(responses)
            each = self.response_wire_bytes()
        if ids.size == 0 and buf.size == 0:
            return np.zeros((0, record_bytes), dtype=np.uint8)
        if buf.size != ids.size * lay.instances * each:
            raise ValueError(f"{buf.size} {'words' if form == 'raw' else 'bytes'} are not the {ids.size} x {lay.instances} responses of {each} of {ids.size} records")
        out = np.zeros((ids.size, record_bytes), dtype=np.uint8)
        check(lib().spiral_gpu_client_decode_records(self.h, buf.ctypes.data_as(C.c_void_p), ids.size, _FORMS[form], record_bytes, ids.ctypes.data_as(U64P),
                                                     out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- keyed records (include/spiral_gpu.h "Keyed records"; a base session, or a SpiralPack session created with out_n >= 1) ----
    def kv_queries(self, table_key, keys, form="seeded") -> np.ndarray:
        """queries() for both candidate buckets of every key, laid out [key][candidate] under 2 n message numbers; both are always made"""
        f = _message_form(form)
        tk, keys = kv_table_key(table_key), kv_keys(keys)
        n, each = keys.shape[0], self._bytes["query", f]
        out = np.zeros((2 * n, each), dtype=np.uint8)
        check(lib().spiral_gpu_client_kv_queries(self.h, tk.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p) if keys.size else None, keys.shape[1], n, f,
                                                 out.ctypes.data_as(C.c_void_p), each))
        return out.view(np.uint64).reshape(2 * n, self.shape.n_query_cts, 2, 1, 2, N) if f == FORM_NTT else out

    def kv_decode(self, table_key, keys, responses, value_bytes: int, form="raw"):
        """(values uint8 [n][value_bytes], found uint8 [n]) from the 2 n responses laid out [key][candidate], in decode()'s forms: found[k] is 0
        (absent: its value bytes are zero), 1 or 2; one launch finds the tag in the headers and decodes only what the found value touches"""
        if form not in _FORMS:
            raise ValueError(f"response form {form!r}: 'raw' or 'wire'")
        kv_layout_for(self.params, value_bytes, self.out_n)
        tk, keys = kv_table_key(table_key), kv_keys(keys)
        n = keys.shape[0]
        if form == "raw":
            buf = np.ascontiguousarray(responses, dtype=np.uint64)
            each = (self.rows + 1) * self.cols * N
        else:
            buf = wire_bytes(responses)
            each = self.response_wire_bytes()
        if buf.size != 2 * n * each:
            raise ValueError(f"{buf.size} {'words' if form == 'raw' else 'bytes'} are not the 2 x {n} responses of {each} of {n} keys")
        values, found = np.zeros((n, value_bytes), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        check(lib().spiral_gpu_client_kv_decode(self.h, tk.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p) if keys.size else None, keys.shape[1],
                                                buf.ctypes.data_as(C.c_void_p), n, _FORMS[form], value_bytes, values.ctypes.data_as(C.c_void_p),
                                                found.ctypes.data_as(C.c_void_p)))
        return values, found

    def noise_step(self, form="raw") -> int:
        """the step of the error's scale (include/spiral_gpu.h, response_noise): D = 4 q' for the switched forms, scale_k = Q // p_db for "final";
        half of it is the decoding radius"""
        if form not in _NOISE_FORMS:
            raise ValueError(f"response form {form!r}: 'raw', 'wire' or 'final'")
        return Q // int(self.params.p_db) if form == "final" else 4 * int(self.shape.qprime)

    def response_noise(self, responses, form="raw", expected=None, errors=False) -> "ResponseNoise":
        """the error e of n responses, per output polynomial and (errors=True) per coefficient, from one launch: the definition is
        include/spiral_gpu.h's.  form "raw" / "wire": decode's inputs; "final": the ciphertexts before the modulus switch,
        [n][(rows + 1)][cols][2048] raw values mod Q.  expected: None (e is the distance from the nearest plaintext) or the true plaintexts
        [n][rows][cols][2048] below p_db (e is the distance from them, and n_wrong counts the coefficients that decode to something else)"""
        step = self.noise_step(form)
        if form == "wire":
            buf = wire_bytes(responses)
            each = self.response_wire_bytes()
        else:
            buf = np.ascontiguousarray(responses, dtype=np.uint64)
            each = (self.rows + 1) * self.cols * N
        if buf.size == 0 or buf.size % each:
            raise ValueError(f"{buf.size} {'bytes' if form == 'wire' else 'words'} are no whole number of responses of {each}")
        n = buf.size // each
        shape = (n, self.rows, self.cols)
        exp = None
        if expected is not None:
            exp = np.ascontiguousarray(expected, dtype=np.uint64)
            if exp.size != n * self.rows * self.cols * N:
                raise ValueError(f"expected holds {exp.size} values, {n} responses take {n * self.rows * self.cols * N}")
        stats = np.zeros(shape + (6,), dtype=np.uint64)
        err = np.zeros(shape + (N,), dtype=np.int64) if errors else None
        check(lib().spiral_gpu_client_response_noise(self.h, buf.ctypes.data_as(C.c_void_p), n, _NOISE_FORMS[form], None if exp is None else exp.ctypes.data_as(U64P),
                                                     stats.ctypes.data_as(U64P), None if err is None else err.ctypes.data_as(C.POINTER(C.c_int64))))
        return ResponseNoise(stats, step, err)


class ResponseNoise:
    """the records of Client.response_noise: max_abs and n_wrong, uint64 [n][rows][cols]; sum and sumsq, exact Python ints in object arrays of that
    shape; step (the decoding radius is step / 2); errors, int64 [n][rows][cols][2048] or None"""

    def __init__(self, stats, step: int, errors=None):
        stats = np.asarray(stats, dtype=np.uint64)
        self.stats, self.step, self.errors = stats, int(step), errors
        self.max_abs, self.n_wrong = stats[..., 0].copy(), stats[..., 1].copy()
        words = stats.astype(object)
        s = words[..., 2] + words[..., 3] * (1 << 64)
        self.sum = np.where(words[..., 3] >= (1 << 63), s - (1 << 128), s)  # 128-bit two's complement
        self.sumsq = words[..., 4] + words[..., 5] * (1 << 64)
        self.count = N  # coefficients per record

    def variance(self, pooled: bool = False):
        """E[e^2] - E[e]^2 from the exact sums: per polynomial (a float array [n][rows][cols]), or pooled=True over all of them (one float)"""
        from fractions import Fraction

        def var(s, sq, cnt):
            return float(Fraction(int(sq), cnt) - Fraction(int(s), cnt) ** 2)

        if pooled:
            return var(self.sum.sum(), self.sumsq.sum(), self.count * self.sum.size)
        out = np.zeros(self.sum.shape, dtype=np.float64)
        for i in np.ndindex(*self.sum.shape):
            out[i] = var(self.sum[i], self.sumsq[i], self.count)
        return out

    def budget_bits(self) -> float:
        """log2(step / 2) - log2(max(max_abs, 1)): the bits between the largest error seen and the decoding radius (negative: it decoded wrongly)"""
        import math

        return math.log2(self.step / 2) - math.log2(max(int(self.max_abs.max()), 1))

    def width2(self, pooled: bool = True):
        """2 pi variance / step^2: the squared Gaussian width parameter of the error in steps -- the unit of the noise model (scheme.py), whose
        sigma = 6.4 is a width parameter (csrc/client_device.h's table)"""
        import math

        return 2 * math.pi * self.variance(pooled) / float(self.step) ** 2
