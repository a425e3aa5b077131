"""The list check every multi-server call shares (spiral_amd/csrc/lanes.h), without a device: each entry point of the library that takes a list of
servers refuses a missing list, an empty one, nine entries and null entries with its own name followed by the SAME text for the same cause, before
it dereferences a handle (no server can exist here) and without writing its output.  An entry point that checks its list any other way fails this."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


class Args:
    """every other argument of a call, non-null and plausible; `out` is what a call that went too far could write"""

    def __init__(self):
        from spiral_amd._lib import U64P

        self.out = np.zeros(64, dtype=np.uint64)
        self.buf = np.zeros(64, dtype=np.uint64)  # (inputs: queries, messages, device buffers no call may reach)
        self.outp = self.out.ctypes.data_as(U64P)
        self.outv = C.c_void_p(self.out.ctypes.data)
        self.bufv = C.c_void_p(self.buf.ctypes.data)
        self.u64_list = (U64P * 9)(*([self.buf.ctypes.data_as(U64P)] * 9))
        self.out_list = (U64P * 9)(*([self.outp] * 9))
        self.void_list = (C.c_void_p * 9)(*([self.buf.ctypes.data] * 9))
        self.others = (C.c_void_p * 2)()  # instances / a key store: never looked at before the list of servers
        self.slots = (C.c_uint32 * 9)()
        self.ms = C.c_float(0)
        self.us = (C.c_double * 8)()


# name of the entry point -> (the `what` its messages begin with, its arguments behind (servers, n))
BASE = {
    "first_dim_batch": ("first_dim_batch", lambda a: ()),
    "run_query_batch": ("run_query_batch", lambda a: ()),
    "run_query_batch_instances": ("run_query_batch_instances", lambda a: (a.others, 1, 1, a.outv, a.outv, a.outv)),
    "answer_batch_instances": ("run_query_batch_instances", lambda a: (a.others, 1, a.u64_list, a.outp, a.outv, a.us)),
    "run_pre_sweep_batch": ("run_pre_sweep_batch", lambda a: (a.outv,)),
    "run_expand_pack_batch": ("run_expand_pack_batch", lambda a: (a.outv,)),
    "run_unpack_convert_sweep_batch": ("run_unpack_convert_sweep_batch", lambda a: (a.bufv, a.outv)),
    "fold_local_batch": ("fold_local_batch", lambda a: (a.bufv, a.outv)),
    "fold_root_batch": ("fold_root_batch", lambda a: (a.bufv, a.outv, a.outv)),
    "bind_keys": ("bind_keys", lambda a: (C.c_void_p(a.buf.ctypes.data), a.slots)),
    "set_query_batch": ("set_query_batch", lambda a: (1, a.void_list, 16)),
    "read_response_wire_batch": ("read_response_wire_batch", lambda a: (a.outv, a.out.nbytes)),
    "time_sweep_batch": ("time_sweep_batch", lambda a: (1, C.byref(a.ms))),
}
PACK = {
    "answer_batch": ("answer_batch", lambda a: (a.u64_list, a.out_list, a.out_list, a.us)),
    "answer_batch_wire": ("answer_batch_wire", lambda a: (a.void_list, 16, a.out_list, a.out_list, a.us)),
    "answer_batch_seeded": ("answer_batch_seeded", lambda a: (a.void_list, 16, a.out_list, a.out_list, a.us)),
    "bind_keys": ("pack bind_keys", lambda a: (C.c_void_p(a.buf.ctypes.data), a.slots)),
    "time_sweep_batch": ("time_sweep_batch", lambda a: (1, C.byref(a.ms))),
}
# the item calls: their own null-argument line comes first (tests/test_pack_instances_cpu.py), the list check behind it
PACK_ITEMS = {
    "answer_batch_instances": ("answer_batch_instances", lambda a: (a.others, 1, a.u64_list, a.outp, a.outv, a.us)),
    "answer_batch_instances_wire": ("answer_batch_instances_wire", lambda a: (a.others, 1, a.void_list, 16, a.outp, a.outv, a.us)),
    "answer_batch_instances_seeded": ("answer_batch_instances_seeded", lambda a: (a.others, 1, a.void_list, 16, a.outp, a.outv, a.us)),
}
CALLS = ([("spiral_gpu_server_" + k, v, True) for k, v in BASE.items()] + [("spiral_gpu_pack_server_" + k, v, True) for k, v in PACK.items()] +
         [("spiral_gpu_pack_server_" + k, v, False) for k, v in PACK_ITEMS.items()])


def test_every_list_taking_entry_point_is_covered(sa):
    """whatever the binding declares with a list of servers first is in the table above"""
    from spiral_amd import _lib

    takes_list = {name for name, (_, args) in _lib.PROTOTYPES.items()
                  if len(args) >= 2 and args[0] == C.POINTER(C.c_void_p) and args[1] is C.c_uint32 and "_server_" in name}
    assert takes_list == {name for name, _, _ in CALLS}


@pytest.mark.parametrize("symbol,spec,null_list", CALLS, ids=[c[0].replace("spiral_gpu_", "") for c in CALLS])
def test_list_check(sa, symbol, spec, null_list):
    L = sa.lib()
    what, rest = spec
    a = Args()
    nulls = (C.c_void_p * 9)()
    cases = [(0, nulls, "no servers"), (9, nulls, "at most 8 clients per batch"), (2, nulls, "null server 0")]
    if null_list:
        cases.insert(0, (1, None, "no servers"))
    for n, hs, err in cases:
        assert getattr(L, symbol)(hs, n, *rest(a)) != 0, (n, err)
        assert L.spiral_gpu_last_error().decode() == f"{what}: {err}", (n, err)
    assert not a.out.any() and a.ms.value == 0 and not any(a.us), "a refused call wrote to its output"
