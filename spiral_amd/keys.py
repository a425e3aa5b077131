"""Key store: the public parameters of a population of clients resident on the device in the device layout, and bind_keys, which makes "lane b
serves the client of slot slots[b]" one launch for all lanes of a batch (include/spiral_gpu.h, spiral_gpu_key_store_*)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import U64P, Params, check, lib, wire_bytes

FULL, COMPACT = 0, 1  # SPIRAL_GPU_KEYS_FULL / SPIRAL_GPU_KEYS_COMPACT
_FORMS = {"full": FULL, "compact": COMPACT}


def _form(form) -> int:
    if form in _FORMS:
        return _FORMS[form]
    if form in (FULL, COMPACT) and not isinstance(form, bool):
        return int(form)
    raise ValueError(f"key store form {form!r}: 'full' or 'compact'")


def slot_bytes(params: Params, out_n: int = 0, form="full") -> int:
    """device bytes of one slot: a pure function of the parameters (no GPU); raises for parameters the path refuses"""
    n = lib().spiral_gpu_key_store_slot_bytes(C.byref(params), out_n, _form(form))
    if n == 0:
        check(-1)
    return int(n)


class KeyStore:
    def __init__(self, params: Params, capacity: int, out_n: int = 0, form="full", device: int = 0):
        """capacity slots of public parameters for `params` (out_n = 0: the base path's, else SpiralPack's for that out_n) on `device`.
        form "full": every polynomial, filled from any message form; "compact": the seed and rows 1.. of every matrix, filled from the seeded form only"""
        self.params, self.capacity, self.out_n, self.form, self.device = params, capacity, out_n, _form(form), device
        h = C.c_void_p()
        check(lib().spiral_gpu_key_store_create(C.byref(params), out_n, device, capacity, self.form, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().spiral_gpu_key_store_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def slot_bytes(self) -> int:
        """device bytes of one slot"""
        return slot_bytes(self.params, self.out_n, self.form)

    def put(self, slot: int, w_left, w_right, w_or_v, v_or_vw):
        """the arguments of set_pub_params (SpiralPack: of PackServer.set_pub_params) into a slot; a full store only"""
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.uint64) for a in (w_left, w_right, w_or_v, v_or_vw)]
        check(lib().spiral_gpu_key_store_put(self.h, slot, *[None if a is None else a.ctypes.data_as(U64P) for a in arrs]))

    def put_wire(self, slot: int, wire):
        """the public parameters as one wire message; a full store only"""
        w = wire_bytes(wire)
        check(lib().spiral_gpu_key_store_put_wire(self.h, slot, w.ctypes.data_as(C.c_void_p), w.size))

    def put_seeded(self, slot: int, msg):
        """the public parameters as one seeded message; either form of store"""
        w = wire_bytes(msg)
        check(lib().spiral_gpu_key_store_put_seeded(self.h, slot, w.ctypes.data_as(C.c_void_p), w.size))

    def put_client(self, slot: int, client):
        """the public parameters of a client session (spiral_amd.Client) into a slot, as their seeded message"""
        self.put_seeded(slot, client.pub_params("seeded"))

    def drop(self, slot: int):
        check(lib().spiral_gpu_key_store_drop(self.h, slot))

    def has(self, slot: int) -> bool:
        return bool(lib().spiral_gpu_key_store_has(self.h, slot))


def _bind(entry: str, servers, store: KeyStore, slots):
    servers, slots = list(servers), [int(s) for s in slots]
    if len(slots) != len(servers):
        raise ValueError(f"bind_keys: {len(servers)} servers, {len(slots)} slots")
    hs = (C.c_void_p * len(servers))(*[s.h for s in servers])
    arr = (C.c_uint32 * len(slots))(*slots)
    check(getattr(lib(), entry)(hs, len(servers), store.h, arr))


def bind_keys(servers, store: KeyStore, slots):
    """lane b (a Server: an owner and its lanes, as run_query_batch takes them) now serves the client of slot slots[b]: one launch on servers[0]'s
    stream, not synchronised; see include/spiral_gpu.h spiral_gpu_server_bind_keys"""
    _bind("spiral_gpu_server_bind_keys", servers, store, slots)
