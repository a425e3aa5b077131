"""SpiralPack / SpiralStreamPack (`--high-rate`, reference src/testing.cpp): host mirror of the function seams and
the resident server handle, each a direct call through the C ABI."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import U64P, KeyedRecords, PackShape, Params, TrackedFingerprint, check, fingerprint_call, fingerprint_key, fingerprint_range, lib, read_args, read_ids, record_array, record_layout, record_out, update_args, wire_bytes

N = 2048
PACK_STAGE_NAMES = ["expansion_us", "conversion_us", "first_dim_us", "folding_us", "packing_us", "sweep_kernels_us", "total_us", "reserved"]


def _p(a: np.ndarray):
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(U64P)


def _c(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64)


def get_pack_shape(p: Params, out_n: int) -> PackShape:
    s = PackShape()
    check(lib().spiral_gpu_pack_get_shape(C.byref(p), out_n, C.byref(s)))
    return s


def has_limb_form(p: Params, out_n: int) -> bool:
    """whether a batch (answer_batch, answer_batch_instances) on this geometry shares ONE matrix-core pass over the trial images: at least 16
    ciphertexts per slot -- or exactly 8 while option "pack_pair_blocks" is 1 (set_option; default 0), the pair form -- and a first dimension that is a
    power of two in [128, 4096].  A function of the parameters and of that one option as it is now: no GPU needed."""
    rc = lib().spiral_gpu_pack_has_limb_form(C.byref(p), out_n)
    if rc < 0:
        check(rc)
    return bool(rc)


def pack(out_n, m_conv, v_ct, v_W) -> np.ndarray:
    """pack (include/testing.h:36): out_n^2 raw 2x1 cts + out_n key matrices -> (out_n+1) x out_n NTT ciphertext"""
    out = np.zeros((out_n + 1, out_n, 2, N), dtype=np.uint64)
    check(lib().spiral_gpu_pack(_p(out), out_n, m_conv, _p(_c(v_ct)), _p(_c(v_W))))
    return out


def fastMultiplyQueryByDatabaseDim1(db, v_firstdim, dim0, num_per) -> np.ndarray:
    out = np.zeros((num_per, 2, 2, N), dtype=np.uint64)
    check(lib().spiral_gpu_fast_multiply_query_by_database_dim1(_p(out), _p(_c(db)), _p(_c(v_firstdim)), dim0, num_per))
    return out


def fastMultiplyQueriesByDatabaseDim1(dbs, v_firstdims, dim0, num_per) -> np.ndarray:
    """n = len(v_firstdims) <= 8 reoriented queries against the len(dbs) trial images in ONE pass (one launch on the matrix cores where the geometry
    has a limb-plane form -- get_option("mfma_sweeps") rises by one --, else one vector-ALU sweep per query): out[b][t] is
    fastMultiplyQueryByDatabaseDim1(dbs[t], v_firstdims[b], dim0, num_per)"""
    n, trials = len(v_firstdims), len(dbs)
    db = np.stack([_c(d).reshape(-1) for d in dbs]) if trials else np.zeros(1, dtype=np.uint64)
    re = np.stack([_c(v).reshape(-1) for v in v_firstdims]) if n else np.zeros(1, dtype=np.uint64)
    out = np.zeros((max(n, 1), max(trials, 1), num_per, 2, 2, N), dtype=np.uint64)
    check(lib().spiral_gpu_fast_multiply_queries_by_database_dim1(_p(out), _p(db), _p(re), n, trials, dim0, num_per))
    return out


class PackServer(TrackedFingerprint, KeyedRecords):
    def __init__(self, params: Params, out_n: int, device: int = 0, trial0: int = 0, trial1: int = 0):
        """trial0, trial1: this server's share [trial0, trial1) of the out_n^2 trials (N GPUs); 0, 0 = all of them"""
        self.params, self.out_n = params, out_n
        self.shape = get_pack_shape(params, out_n)
        h = C.c_void_p()
        check(lib().spiral_gpu_pack_server_create_sharded(C.byref(params), out_n, device, trial0, trial1, C.byref(h)))
        self.h = h
        self.trial0, self.trial1 = (trial0, trial1) if trial1 else (0, self.shape.trials)

    def set_stream(self, hip_stream: int):
        check(lib().spiral_gpu_pack_server_set_stream(self.h, C.c_void_p(hip_stream)))

    def fold_trials(self, query, folded_ptr: int):
        """expansion + conversion + this server's sweeps and folding; the folded ciphertexts ([n_local][2][N] raw u64) are written to
        the device buffer at folded_ptr (asynchronous on the server's stream)"""
        check(lib().spiral_gpu_pack_server_fold_trials(self.h, _p(_c(query)), C.c_void_p(folded_ptr)))

    def stage_us(self) -> dict:
        """stage times of the last answer / fold_trials (synchronises the stream)"""
        us = (C.c_double * 8)()
        check(lib().spiral_gpu_pack_server_stage_us(self.h, us))
        return dict(zip(PACK_STAGE_NAMES, list(us)))

    def pack_gathered(self, gathered_ptr: int, want_packed: bool = False):
        """pack + modulus switch of all out_n^2 folded ciphertexts (device buffer in trial order): (response, packed or None)"""
        n = self.out_n
        resp = np.zeros((n + 1, n, N), dtype=np.uint64)
        packed = np.zeros((n + 1, n, 2, N), dtype=np.uint64) if want_packed else None
        check(lib().spiral_gpu_pack_server_pack_gathered(self.h, C.c_void_p(gathered_ptr), _p(resp), _p(packed) if want_packed else None))
        return resp, packed

    def close(self):
        if getattr(self, "h", None):
            lib().spiral_gpu_pack_server_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def gen_db(self, seed: int):
        check(lib().spiral_gpu_pack_server_gen_db(self.h, seed))

    def load_db(self, trial: int, db):
        check(lib().spiral_gpu_pack_server_load_db(self.h, trial, _p(_c(db))))

    def load_db_items(self, trial: int, items, coeff_bits: int, first_item: int = 0, n_items=None):
        """raw ingest of one trial: bit-packed plaintext coefficients (coeff_bits each), 2048 per item"""
        items = np.ascontiguousarray(items)
        if n_items is None:
            n_items = items.nbytes * 8 // (N * coeff_bits)
        check(lib().spiral_gpu_pack_server_load_db_items(self.h, trial, items.ctypes.data_as(C.c_void_p), coeff_bits, first_item, n_items))

    def update_db_items(self, trial: int, items, coeff_bits: int, item_ids):
        """replace the items item_ids[k] <- plaintext k of `items` (2048 coefficients each, as load_db_items) of one trial in place, in the image's
        current form, on this server's stream; see include/spiral_gpu.h spiral_gpu_pack_server_update_db_items"""
        items, ids = update_args(items, coeff_bits, item_ids, 1)
        check(lib().spiral_gpu_pack_server_update_db_items(self.h, trial, items.ctypes.data_as(C.c_void_p), coeff_bits, _p(ids), len(ids)))

    def read_db_items(self, trial: int, coeff_bits: int, first_item: int = 0, n_items=None, out=None) -> np.ndarray:
        """items first_item .. first_item + n_items - 1 (default: to the end) of one trial back as plaintexts, uint8 bytes in load_db_items' layout,
        read from the trial image in its current form; see include/spiral_gpu.h spiral_gpu_pack_server_read_db_items"""
        if n_items is None:
            n_items = self.shape.dim0 * self.shape.num_per - first_item
        out = read_args(self.params, coeff_bits, n_items, self.out_n, out)
        check(lib().spiral_gpu_pack_server_read_db_items(self.h, trial, out.ctypes.data_as(C.c_void_p), coeff_bits, first_item, n_items))
        return out

    def read_db_items_at(self, trial: int, coeff_bits: int, ids, out=None) -> np.ndarray:
        """the items ids[k] of one trial (any order, duplicates allowed) back as plaintexts, plaintext k at k * 256 * coeff_bits bytes"""
        ids = read_ids(ids)
        out = read_args(self.params, coeff_bits, len(ids), self.out_n, out)
        check(lib().spiral_gpu_pack_server_read_db_items_at(self.h, trial, out.ctypes.data_as(C.c_void_p), coeff_bits, _p(ids), len(ids)))
        return out

    # ---- content fingerprints (include/spiral_gpu.h "Fingerprints"): computed on the device from the image in its current form ----
    def fingerprint_items(self, key, first_item: int = 0, n_items=None, per_item: bool = False):
        """the combined fingerprint F of items first_item .. first_item + n_items - 1 (default: to the end) under `key`, a pair of ints in [0, 2^64);
        with per_item, (F, the item fingerprints as a uint64 array).  A shard returns its partial sums (0 for an item it does not hold): add the
        shards' values with spiral_amd.fingerprint_add"""
        k = fingerprint_key(key)
        first_item, n_items = fingerprint_range(first_item, n_items, self.shape.dim0 * self.shape.num_per)
        return fingerprint_call(lib().spiral_gpu_pack_server_fingerprint_items, (self.h, k, first_item, n_items), n_items, per_item)

    def fingerprint_items_at(self, key, ids):
        """(F, the item fingerprints as a uint64 array) of the items ids[k] (any order; a repeated id counts as often as it is listed); see
        fingerprint_items"""
        k = fingerprint_key(key)
        ids = read_ids(ids)
        return fingerprint_call(lib().spiral_gpu_pack_server_fingerprint_items_at, (self.h, k, _p(ids), len(ids)), len(ids), True)

    # ---- tracked fingerprints: fingerprint_track, _untrack, _tracked, _tracked_polys, _scrub (_lib.TrackedFingerprint) ----
    _fp_prefix = "spiral_gpu_pack_server"
    _kv_prefix = "spiral_gpu_pack_server"  # keyed records on the trial images: kv_load, kv_put, kv_delete, kv_get, kv_stats (_lib.KeyedRecords)

    def _fp_table(self):
        total = self.shape.dim0 * self.shape.num_per
        return total, self.trial1 - self.trial0, total

    # ---- records of any byte size (include/spiral_gpu.h "Records", SpiralPack): no trial argument, the layout names the trial images ----
    def load_records(self, records, record_bytes: int, first_record: int = 0, instance: int = 0):
        """records first_record .. (whole items' worth) from one contiguous byte array, through load_db_items' ingest of every trial, padding zero"""
        lay = record_layout(self.params, record_bytes, self.out_n)
        records = record_array(records, record_bytes)
        check(lib().spiral_gpu_pack_server_load_records(self.h, records.ctypes.data_as(C.c_void_p), record_bytes, instance, first_record, records.size // record_bytes))
        return lay

    def update_records(self, records, record_bytes: int, record_ids, instance: int = 0):
        """replace the records record_ids[k] <- record k of `records` in place, in every touched trial image's current form, on this server's stream;
        ids distinct; see include/spiral_gpu.h spiral_gpu_pack_server_update_records"""
        record_layout(self.params, record_bytes, self.out_n)
        ids = read_ids(record_ids)
        if np.unique(ids).size != ids.size:
            raise ValueError("record_ids holds a duplicate id")
        records = record_array(records, record_bytes, len(ids))
        check(lib().spiral_gpu_pack_server_update_records(self.h, records.ctypes.data_as(C.c_void_p), record_bytes, instance, _p(ids), len(ids)))

    def read_records(self, record_bytes: int, first_record: int = 0, n_records=None, out=None, instance: int = 0) -> np.ndarray:
        """records first_record .. first_record + n_records - 1 (default: to the end) as a uint8 array [n][record_bytes], read from the trial images
        in their current form; a trial shard or an instance server fills in what it holds (pass the same `out` to each)"""
        lay = record_layout(self.params, record_bytes, self.out_n)
        if n_records is None:
            n_records = lay.capacity - first_record
        out = record_out(record_bytes, n_records, out)
        check(lib().spiral_gpu_pack_server_read_records(self.h, out.ctypes.data_as(C.c_void_p), record_bytes, instance, first_record, n_records))
        return out

    def read_records_at(self, record_bytes: int, record_ids, out=None, instance: int = 0) -> np.ndarray:
        """the records record_ids[k] (any order, duplicates allowed) as a uint8 array [n][record_bytes]; see read_records"""
        record_layout(self.params, record_bytes, self.out_n)
        ids = read_ids(record_ids)
        out = record_out(record_bytes, len(ids), out)
        check(lib().spiral_gpu_pack_server_read_records_at(self.h, out.ctypes.data_as(C.c_void_p), record_bytes, instance, _p(ids), len(ids)))
        return out

    def read_acc(self, trial: int) -> np.ndarray:
        """first-dimension accumulators of one trial of the last answer: [num_per][2][2][N] NTT form"""
        out = np.zeros((self.shape.num_per, 2, 2, N), dtype=np.uint64)
        check(lib().spiral_gpu_pack_server_read_acc(self.h, trial, _p(out)))
        return out

    def read_response_wire(self) -> np.ndarray:
        """the last answer's response in its wire form (bit-packed on the device): bytes"""
        n = lib().spiral_gpu_response_wire_bytes(C.byref(self.params), self.out_n)
        out = np.zeros(n, dtype=np.uint8)
        check(lib().spiral_gpu_pack_server_read_response_wire(self.h, out.ctypes.data_as(C.c_void_p), n))
        return out

    def fill_db_random(self, seed: int):
        check(lib().spiral_gpu_pack_server_fill_db_random(self.h, seed))

    def set_pub_params(self, w_left, w_right, v, v_w):
        check(lib().spiral_gpu_pack_server_set_pub_params(self.h, _p(w_left), _p(w_right), _p(v), _p(v_w)))

    def set_pub_params_wire(self, wire):
        """the public parameters as one wire message (W_exp_left, W_exp_right, V -- expansion only -- and v_W); decoded on the device"""
        w = wire_bytes(wire)
        check(lib().spiral_gpu_pack_server_set_pub_params_wire(self.h, w.ctypes.data_as(C.c_void_p), w.size))

    def set_pub_params_seeded(self, msg):
        """the public parameters as one seeded message (include/spiral_gpu.h): row 0 of every matrix from the seed"""
        w = wire_bytes(msg)
        check(lib().spiral_gpu_pack_server_set_pub_params_seeded(self.h, w.ctypes.data_as(C.c_void_p), w.size))

    def _answer(self, form: str, query, want_packed: bool):
        q = _query_arrays(form, [query])[0]
        qargs = (_p(q),) if form == "ntt" else (q.ctypes.data_as(C.c_void_p), q.size)
        n = self.out_n
        resp = np.zeros((n + 1, n, N), dtype=np.uint64)
        packed = np.zeros((n + 1, n, 2, N), dtype=np.uint64) if want_packed else None
        us = (C.c_double * 8)()
        check(getattr(lib(), "spiral_gpu_pack_server_answer" + _FORMS[form])(self.h, *qargs, _p(resp), _p(packed) if want_packed else None, us))
        return resp, packed, dict(zip(PACK_STAGE_NAMES, list(us)))

    def answer(self, query, want_packed: bool = True):
        return self._answer("ntt", query, want_packed)

    def answer_wire(self, query_wire, want_packed: bool = True):
        """answer with the query in its wire form: as answer"""
        return self._answer("wire", query_wire, want_packed)

    def answer_seeded(self, query_msg, want_packed: bool = True):
        """answer with the query in its seeded form: as answer"""
        return self._answer("seeded", query_msg, want_packed)

    def sweep_bytes(self) -> int:
        return int(lib().spiral_gpu_pack_server_sweep_bytes(self.h))

    def create_lane(self) -> "PackServer":
        """a query lane: a new server with this one's parameters, out_n and device that sweeps THIS server's trial images (answer_batch);
        its own public parameters, query and intermediates; loads through it fail"""
        h = C.c_void_p()
        check(lib().spiral_gpu_pack_server_create_lane(self.h, C.byref(h)))
        lane = PackServer.__new__(PackServer)
        lane.params, lane.out_n, lane.shape, lane.h = self.params, self.out_n, self.shape, h
        lane.trial0, lane.trial1 = self.trial0, self.trial1
        return lane

    def create_shard_lane(self) -> "PackServer":
        """a lane of a server that holds a trial range only: this one's parameters, out_n, device and trial range, THIS server's trial images, its own
        public parameters, query and intermediates (fold_trials_batch on every rank, pack_gathered_batch on the root, bind_keys; loads through it
        fail).  Of a server that holds every trial it is an ordinary lane; see include/spiral_gpu.h spiral_gpu_pack_server_create_shard_lane"""
        h = C.c_void_p()
        check(lib().spiral_gpu_pack_server_create_shard_lane(self.h, C.byref(h)))
        lane = PackServer.__new__(PackServer)
        lane.params, lane.out_n, lane.shape, lane.h = self.params, self.out_n, self.shape, h
        lane.trial0, lane.trial1 = self.trial0, self.trial1
        return lane

    def set_db_format(self, fmt: int):
        """convert the trial images in place: DB_PACKED (0) or DB_LIMBS (1, the batched matrix-core sweep's form; only where that sweep applies)"""
        check(lib().spiral_gpu_pack_server_set_db_format(self.h, int(fmt)))

    def db_format(self) -> int:
        return int(lib().spiral_gpu_pack_server_db_format(self.h))

    def db_device_bytes(self) -> int:
        return int(lib().spiral_gpu_pack_server_db_device_bytes(self.h))


DB_PACKED, DB_LIMBS = 0, 1
MAX_LANES = 8
# the forms a query comes in (include/spiral_gpu.h) -> the suffix of the entry points that take it
_FORMS = {"ntt": "", "wire": "_wire", "seeded": "_seeded"}


def _query_arrays(form: str, queries) -> list:
    """queries as contiguous arrays: uint64 polynomials (NTT form) or uint8 messages"""
    return [_c(q) if form == "ntt" else wire_bytes(q) for q in queries]


def _query_list_args(form: str, qs):
    """what a multi-query entry point takes for its queries: the pointer array, and in the message forms the bytes of each"""
    if form == "ntt":
        return ((U64P * len(qs))(*[_p(q) for q in qs]),)
    return (C.c_void_p * len(qs))(*[q.ctypes.data for q in qs]), qs[0].size


def _lane_handles(servers, what: str):
    servers = list(servers)
    if not 1 <= len(servers) <= MAX_LANES:
        raise ValueError(f"{what}: {len(servers)} servers, 1 .. {MAX_LANES} per batch")
    if not all(isinstance(s, PackServer) for s in servers):
        raise TypeError(f"{what}: every server must be a PackServer")
    if len({id(s) for s in servers}) != len(servers):
        raise ValueError(f"{what}: a server appears twice")
    if any(not getattr(s, "h", None) for s in servers):
        raise ValueError(f"{what}: a server is closed")
    return servers, (C.c_void_p * len(servers))(*[s.h for s in servers])


def bind_keys(servers, store, slots):
    """lane b (an owner PackServer and its lanes, as answer_batch takes them) now serves the client of slot slots[b] of a keys.KeyStore created with
    their out_n: one launch on servers[0]'s stream, not synchronised; see include/spiral_gpu.h spiral_gpu_pack_server_bind_keys"""
    from .keys import _bind

    servers, _ = _lane_handles(servers, "bind_keys")
    _bind("spiral_gpu_pack_server_bind_keys", servers, store, slots)


def _answer_batch(form: str, servers, queries, want_packed: bool):
    what = "answer_batch" + _FORMS[form]
    servers, hs = _lane_handles(servers, what)
    qs = list(queries) if form == "ntt" else _query_arrays(form, queries)
    if len(qs) != len(servers):
        raise ValueError(f"{what}: {len(qs)} queries for {len(servers)} servers")
    if form == "ntt":
        qs = _query_arrays(form, qs)
    elif len({w.size for w in qs}) != 1:
        raise ValueError(f"{what}: the queries differ in size")
    n = servers[0].out_n
    resp = [np.zeros((n + 1, n, N), dtype=np.uint64) for _ in servers]
    packed = [np.zeros((n + 1, n, 2, N), dtype=np.uint64) if want_packed else None for _ in servers]
    arr = lambda xs: (U64P * len(xs))(*[_p(x) if x is not None else None for x in xs])
    us = (C.c_double * 8)()
    check(getattr(lib(), "spiral_gpu_pack_server_" + what)(hs, len(servers), *_query_list_args(form, qs), arr(resp), arr(packed), us))
    return list(zip(resp, packed)), dict(zip(PACK_STAGE_NAMES[:7] + ["n"], list(us)))


def answer_batch(servers, queries, want_packed: bool = False):
    """n <= 8 queries, one per server (an owner and its lanes, create_lane), answered with ONE first-dimension pass over the trial images:
    ([(response, packed or None) per server], stage times of the batch).  Each lane's results equal its own answer's.  From option
    "pack_batch_lanes" servers on (set_option; default 0 = never) the batch takes the lane form: expansion, conversion, folding, packing and switch
    are one launch sequence that carries every client, not one client after another; get_option("pack_lane_batches") counts the calls that did.  The
    servers may come in any order (servers[0]'s stream runs the batch); in lane form the stage times are whole-batch intervals."""
    return _answer_batch("ntt", servers, queries, want_packed)


def answer_batch_wire(servers, query_wires, want_packed: bool = False):
    """answer_batch with the queries in their wire form (all of one size); every query is checked and decoded before the batch runs"""
    return _answer_batch("wire", servers, query_wires, want_packed)


def answer_batch_seeded(servers, query_msgs, want_packed: bool = False):
    """answer_batch with the queries in their seeded form (all of one size); every query is checked and expanded before the batch runs"""
    return _answer_batch("seeded", servers, query_msgs, want_packed)


def fold_trials_batch(servers, queries, folded_ptr: int, form: str = "ntt"):
    """every rank's half of a trial-sharded batch: n <= 8 queries, one per server (this rank's owner and / or its shard lanes, create_shard_lane),
    through expansion, conversion, ONE pass over the rank's trial images and the folding; lane b's folded ciphertexts of the local trials
    [trial0, trial1) go to the device buffer at folded_ptr + ((b * (trial1 - trial0) + k) * 2 * 2048) words.  Asynchronous on servers[0]'s stream.
    form: "ntt" (uint64 polynomials), "wire" or "seeded" (messages of one size).  See include/spiral_gpu.h spiral_gpu_pack_server_fold_trials_batch"""
    what = "fold_trials_batch"
    if form not in _FORMS:
        raise ValueError(f"{what}: form {form!r}, one of {sorted(_FORMS)}")
    servers, hs = _lane_handles(servers, what)
    qs = _query_arrays(form, list(queries))
    if len(qs) != len(servers):
        raise ValueError(f"{what}: {len(qs)} queries for {len(servers)} servers")
    if form != "ntt" and len({w.size for w in qs}) != 1:
        raise ValueError(f"{what}: the queries differ in size")
    ptrs = (C.c_void_p * len(qs))(*[q.ctypes.data for q in qs])
    code = {"ntt": 0, "wire": 1, "seeded": 2}[form]  # (spiral_gpu_message_form; 0 = the NTT form)
    check(lib().spiral_gpu_pack_server_fold_trials_batch(hs, len(servers), code, ptrs, 0 if form == "ntt" else qs[0].size, C.c_void_p(folded_ptr)))


def pack_gathered_batch(servers, gathered_ptr: int, cuts, block_cts: int, want_packed: bool = False, wire: bool = False):
    """the root's half: the all-gathered blocks at gathered_ptr (block r = rank r's [lane][k] of the trials [cuts[r], cuts[r + 1]), at a stride of
    block_cts ciphertexts) packed and switched for all n clients in one lane-aware launch sequence.  servers: n lanes of one image on the root, lane b
    the client that was lane b on every rank.  Returns [(response, packed or None) per server], and with wire=True also their wire forms
    [n, bytes] uint8.  See include/spiral_gpu.h spiral_gpu_pack_server_pack_gathered_batch"""
    what = "pack_gathered_batch"
    servers, hs = _lane_handles(servers, what)
    cuts = [int(c) for c in cuts]
    if len(cuts) < 2 or min(cuts) < 0 or max(cuts) >= 1 << 32:
        raise ValueError(f"{what}: cuts {cuts}: at least two, each a uint32")
    s0 = servers[0]
    n = s0.out_n
    resp = [np.zeros((n + 1, n, N), dtype=np.uint64) for _ in servers]
    packed = [np.zeros((n + 1, n, 2, N), dtype=np.uint64) if want_packed else None for _ in servers]
    arr = lambda xs: (U64P * len(xs))(*[_p(x) if x is not None else None for x in xs])
    wires = np.zeros((len(servers), lib().spiral_gpu_response_wire_bytes(C.byref(s0.params), n)), dtype=np.uint8) if wire else None
    check(lib().spiral_gpu_pack_server_pack_gathered_batch(hs, len(servers), C.c_void_p(gathered_ptr), (C.c_uint32 * len(cuts))(*cuts), len(cuts) - 1,
                                                           int(block_cts), arr(resp), arr(packed) if want_packed else None,
                                                           wires.ctypes.data_as(C.c_void_p) if wire else None))
    out = list(zip(resp, packed))
    return (out, wires) if wire else out


def time_sweep_batch(servers, iters: int = 10) -> float:
    """the batched first-dimension sweep alone (with the lanes' current queries, each answered once): average ms per pass"""
    servers, hs = _lane_handles(servers, "time_sweep_batch")
    if int(iters) < 1:
        raise ValueError("time_sweep_batch: iters >= 1")
    ms = C.c_float()
    check(lib().spiral_gpu_pack_server_time_sweep_batch(hs, len(servers), int(iters), C.byref(ms)))
    return float(ms.value)


def _item_args(servers, instances, what: str):
    """the clients' and the instances' handle arrays, checked in Python first (the library checks everything again)"""
    servers, hs = _lane_handles(servers, what)
    instances = list(instances)
    if not instances:
        raise ValueError(f"{what}: no instances")
    if not all(isinstance(s, PackServer) for s in instances):
        raise TypeError(f"{what}: every instance must be a PackServer")
    if any(not getattr(s, "h", None) for s in instances):
        raise ValueError(f"{what}: an instance is closed")
    return servers, hs, instances, (C.c_void_p * len(instances))(*[s.h for s in instances])


def _item_call(servers, instances, wire: bool, stats, call):
    """the outputs of an item call, [B, F, out_n + 1, out_n, 2048] uint64 (and [B, F, wire bytes] uint8 with wire=True), filled by call(resp, wire)"""
    s0 = servers[0]
    n, B, F = s0.out_n, len(servers), len(instances)
    resp = np.zeros((B, F, n + 1, n, N), dtype=np.uint64)
    wb = lib().spiral_gpu_response_wire_bytes(C.byref(s0.params), n)
    wires = np.zeros((B, F, wb), dtype=np.uint8) if wire else None
    us = C.c_double()
    call(_p(resp), wires.ctypes.data_as(C.c_void_p) if wire else None, C.byref(us))
    if stats is not None:
        stats["total_us"] = us.value
    return (resp, wires) if wire else resp


def _answer_batch_instances(form: str, servers, instances, queries, wire: bool, stats):
    what = "answer_batch_instances" + _FORMS[form]
    servers, hs, instances, ins = _item_args(servers, instances, what)
    s0 = servers[0]
    qs = list(queries) if form == "ntt" else _query_arrays(form, queries)
    if len(qs) != len(servers):
        raise ValueError(f"{what}: {len(qs)} queries for {len(servers)} clients")
    if form == "ntt":
        words = s0.shape.n_query_cts * 2 * 2 * N  # ([ct][row] polynomials of the reference's NTT form, two words per coefficient)
        for q in qs:
            if not isinstance(q, np.ndarray) or q.dtype != np.uint64:
                raise TypeError(f"{what}: a query is a uint64 array, not {getattr(q, 'dtype', type(q).__name__)}")
            if q.size != words:
                raise ValueError(f"{what}: a query of {q.size} words, this geometry's takes {words}")
        qs = _query_arrays(form, qs)
    else:
        want = getattr(lib(), f"spiral_gpu_pack_query_{form}_bytes")(C.byref(s0.params), s0.out_n)
        if any(w.size != want for w in qs):
            raise ValueError(f"{what}: the {form} form of a query takes {want} bytes, got {[w.size for w in qs]}")
    fn, qargs = getattr(lib(), "spiral_gpu_pack_server_" + what), _query_list_args(form, qs)
    return _item_call(servers, instances, wire, stats, lambda r, w, us: check(fn(hs, len(servers), ins, len(instances), *qargs, r, w, us)))


def answer_batch_instances(servers, instances, queries, wire: bool = False, stats: dict = None):
    """B <= 8 clients (an owner and its lanes, each with its own public parameters) fetch an item of F = len(instances) plaintexts each: one query per
    client, F instances (PackServers holding all trial images of their own database).  Returns [B, F, out_n + 1, out_n, 2048] uint64 responses -- slot
    [q, k] equals client q's own answer against instance k -- and with wire=True also their wire forms [B, F, bytes] uint8.  stats (a dict, optional)
    receives total_us, the device time of the call.  See include/spiral_gpu.h spiral_gpu_pack_server_answer_batch_instances."""
    return _answer_batch_instances("ntt", servers, instances, queries, wire, stats)


def answer_batch_instances_wire(servers, instances, query_wires, wire: bool = False, stats: dict = None):
    """answer_batch_instances with the queries in their wire form (each spiral_gpu_pack_query_wire_bytes long); every query is decoded before the call runs"""
    return _answer_batch_instances("wire", servers, instances, query_wires, wire, stats)


def answer_batch_instances_seeded(servers, instances, query_msgs, wire: bool = False, stats: dict = None):
    """answer_batch_instances with the queries in their seeded form (each spiral_gpu_pack_query_seeded_bytes long); every query is expanded before
    the call runs"""
    return _answer_batch_instances("seeded", servers, instances, query_msgs, wire, stats)


def answer_instances(server, instances, query, wire: bool = False, stats: dict = None):
    """one client's item of F = len(instances) plaintexts: [F, out_n + 1, out_n, 2048] uint64 (and [F, bytes] uint8 with wire=True)"""
    out = answer_batch_instances([server], instances, [query], wire, stats)
    return (out[0][0], out[1][0]) if wire else out[0]


def answer_instances_wire(server, instances, query_wire, wire: bool = False, stats: dict = None):
    """answer_instances with the query in its wire form"""
    out = answer_batch_instances_wire([server], instances, [query_wire], wire, stats)
    return (out[0][0], out[1][0]) if wire else out[0]
