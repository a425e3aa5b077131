"""Resident server handle: the server half of do_test (src/spiral.cpp:2337-2406, 1584-1629) with the
database, public parameters and intermediates kept in HBM."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import FORM_NTT, FORM_SEEDED, FORM_WIRE, U64P, KeyedRecords, Params, Shape, TrackedFingerprint, check, fingerprint_call, fingerprint_key, fingerprint_range, lib, read_args, read_ids, record_array, record_layout, record_out, update_args, wire_bytes

N = 2048

BUF_EXPANDED, BUF_CTS, BUF_GSW, BUF_ACC, BUF_RAW, BUF_FINAL, BUF_RESPONSE, BUF_QUERY = range(8)
DB_PACKED, DB_LIMBS = 0, 1  # spiral_gpu_db_format
STAGE_NAMES = ["expansion_us", "conversion_us", "first_dim_us", "folding_us", "response_us", "sweep_kernel_us", "total_us", "scaltomat_us"]


def _p(a: np.ndarray):
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(U64P)


def first_dim_batch(servers):
    """one pass over the database for the (converted) queries of up to eight servers sharing one image; see include/spiral_gpu.h"""
    arr = (C.c_void_p * len(servers))(*[s.h for s in servers])
    check(lib().spiral_gpu_server_first_dim_batch(arr, len(servers)))


def time_sweep_batch(servers, iters: int = 20) -> float:
    """average ms of first_dim_batch's sweep launch alone (HIP events on servers[0]'s stream)"""
    arr = (C.c_void_p * len(servers))(*[s.h for s in servers])
    ms = C.c_float()
    check(lib().spiral_gpu_server_time_sweep_batch(arr, len(servers), iters, C.byref(ms)))
    return ms.value


def run_query_batch(servers):
    """the whole answer for the queries of up to eight servers sharing one image, every launch carrying all of them; see include/spiral_gpu.h"""
    arr = (C.c_void_p * len(servers))(*[s.h for s in servers])
    check(lib().spiral_gpu_server_run_query_batch(arr, len(servers)))


MESSAGE_FORMS = {"ntt": FORM_NTT, "wire": FORM_WIRE, "seeded": FORM_SEEDED}


def set_query_batch(servers, msgs, form="wire"):
    """the queries of all lanes of a batch in one call: msgs[b], a wire message (form="wire": what set_query_wire takes) or a seeded one
    (form="seeded": what set_query_seeded takes), into servers[b]'s query buffer by one lane-aware launch on servers[0]'s stream; compressed
    queries are not synchronised.  See include/spiral_gpu.h spiral_gpu_server_set_query_batch"""
    servers, msgs = list(servers), list(msgs)
    if form not in MESSAGE_FORMS:
        raise ValueError(f"set_query_batch: form {form!r}: 'wire' or 'seeded'")
    if len(msgs) != len(servers):
        raise ValueError(f"set_query_batch: {len(servers)} servers, {len(msgs)} messages")
    ws = [None if m is None else wire_bytes(m) for m in msgs]
    sizes = {w.size for w in ws if w is not None}
    if len(sizes) > 1:
        raise ValueError(f"set_query_batch: messages of different sizes {sorted(sizes)}")
    ptrs = (C.c_void_p * len(ws))(*[None if w is None else w.ctypes.data for w in ws])
    check(lib().spiral_gpu_server_set_query_batch(_lanes(servers), len(servers), MESSAGE_FORMS[form], ptrs, sizes.pop() if sizes else 0))


def read_response_wire_batch(servers) -> np.ndarray:
    """the wire forms of the last responses of all lanes of a batch in one launch, one copy and one synchronisation: [n][wire bytes] uint8, row b
    what servers[b].read_response_wire() returns"""
    servers = list(servers)
    nb = lib().spiral_gpu_response_wire_bytes(C.byref(servers[0].params), 2) if servers and servers[0] is not None else 0
    out = np.zeros((len(servers), nb), dtype=np.uint8)
    check(lib().spiral_gpu_server_read_response_wire_batch(_lanes(servers), len(servers), out.ctypes.data_as(C.c_void_p), out.nbytes))
    return out


def _lanes(servers):
    return (C.c_void_p * len(servers))(*[s.h if s is not None else None for s in servers])


def run_pre_sweep_batch(servers, acc_ptr: int):
    """one rank's expansion, conversion and sweep for up to eight clients (an owner on its j-shard and its lanes) into the rank-major accumulator
    buffer [rank][lane][num_per / G][6][2048]; see include/spiral_gpu.h"""
    check(lib().spiral_gpu_server_run_pre_sweep_batch(_lanes(servers), len(servers), C.c_void_p(acc_ptr or None)))


def run_expand_pack_batch(servers, bits_ptr: int):
    """sharded expansion of every client's query and the pack of this rank's GSW bits into [lane][gsw_bits_words]"""
    check(lib().spiral_gpu_server_run_expand_pack_batch(_lanes(servers), len(servers), C.c_void_p(bits_ptr or None)))


def run_unpack_convert_sweep_batch(servers, gathered_bits_ptr: int, acc_ptr: int):
    """unpack of the all-gathered [rank][lane][gsw_bits_words] blocks, conversion and the sweep into the rank-major accumulator buffer"""
    check(lib().spiral_gpu_server_run_unpack_convert_sweep_batch(_lanes(servers), len(servers), C.c_void_p(gathered_bits_ptr or None), C.c_void_p(acc_ptr or None)))


def fold_local_batch(servers, chunk_ptr: int, out_cts_ptr: int):
    """every lane's reduce-scattered chunk ([lane][num_per / G] ciphertexts) through the local folding rounds -> [lane][6][2048] raw ciphertexts"""
    check(lib().spiral_gpu_server_fold_local_batch(_lanes(servers), len(servers), C.c_void_p(chunk_ptr or None), C.c_void_p(out_cts_ptr or None)))


def fold_root_batch(servers, gathered_cts_ptr: int, responses_ptr: int = 0, wire_ptr: int = 0):
    """the root's last log2(G) rounds and the switch on the all-gathered [rank][lane][6][2048]; optional [lane] outputs of the responses and wire forms"""
    check(lib().spiral_gpu_server_fold_root_batch(_lanes(servers), len(servers), C.c_void_p(gathered_cts_ptr or None), C.c_void_p(responses_ptr or None),
                                                  C.c_void_p(wire_ptr or None)))


def run_column_batch(servers, out_cts_ptr: int):
    """a column shard's whole local share for up to eight clients (the shard's owner and its lanes): expansion, conversion, ONE pass over the shard's
    num_per / G columns into the lanes' own accumulators and the first nu2 - log2 G fold rounds -> [lane][6][2048] raw ciphertexts at out_cts_ptr; then
    one all-gather and fold_root_batch on the root.  See include/spiral_gpu.h spiral_gpu_server_run_column_batch"""
    check(lib().spiral_gpu_server_run_column_batch(_lanes(servers), len(servers), C.c_void_p(out_cts_ptr or None)))


def run_query_batch_instances(servers, instances, responses_ptr: int = 0, finals_ptr: int = 0, wire_ptr: int = 0, pre: bool = True):
    """item queries of up to eight clients (an owner and its lanes, each with its own query) against the same database instances: one sweep per instance
    for all of them; device outputs, client q and instance k at slot q * len(instances) + k: responses / finals 6 x 2048 words, wire
    spiral_gpu_response_wire_bytes(params, 2) bytes per slot (at least one of responses and wire); see include/spiral_gpu.h"""
    arr = (C.c_void_p * len(servers))(*[s.h for s in servers])
    inst = (C.c_void_p * len(instances))(*[s.h for s in instances])
    check(lib().spiral_gpu_server_run_query_batch_instances(arr, len(servers), inst, len(instances), 1 if pre else 0, C.c_void_p(responses_ptr or None),
                                                             C.c_void_p(finals_ptr or None), C.c_void_p(wire_ptr or None)))


def answer_batch_instances(servers, instances, queries, wire: bool = False):
    """host-buffer form of run_query_batch_instances: (responses [B][n][3][2][N], device us of the item batch), or with wire=True
    (wire forms [B][n][bytes] uint8, device us)"""
    B, n = len(servers), len(instances)
    arr = (C.c_void_p * B)(*[s.h for s in servers])
    inst = (C.c_void_p * n)(*[s.h for s in instances])
    qs = [np.ascontiguousarray(q, dtype=np.uint64) for q in queries]
    qp = (U64P * B)(*[_p(q) for q in qs])
    us = C.c_double()
    if wire:
        nb = lib().spiral_gpu_response_wire_bytes(C.byref(servers[0].params), 2)
        out = np.zeros((B, n, nb), dtype=np.uint8)
        check(lib().spiral_gpu_server_answer_batch_instances(arr, B, inst, n, qp, None, out.ctypes.data_as(C.c_void_p), C.byref(us)))
    else:
        out = np.zeros((B, n, 3, 2, N), dtype=np.uint64)
        check(lib().spiral_gpu_server_answer_batch_instances(arr, B, inst, n, qp, _p(out), None, C.byref(us)))
    return out, us.value


class Server(TrackedFingerprint, KeyedRecords):
    def __init__(self, params: Params, device: int = 0, j_begin: int = 0, j_end: int = 0, share_db_of: "Server | None" = None, *,
                 col_rank: "int | None" = None, col_ranks: "int | None" = None):
        """share_db_of: make this server a query lane of that one -- same parameters, device and shard, sweeping ITS database
        image (no second image is ever allocated).  col_rank, col_ranks (both or neither): a column shard -- the ciphertext columns
        ii = col_rank (mod col_ranks) of the whole first dimension (include/spiral_gpu.h spiral_gpu_server_create_column_shard); a lane of a column
        shard is one of the same rank"""
        self.params = params
        self.shape = Shape()
        check(lib().spiral_gpu_get_shape(C.byref(params), C.byref(self.shape)))
        if (col_rank is None) != (col_ranks is None):
            raise ValueError("a column shard takes both col_rank and col_ranks")
        h = C.c_void_p()
        if share_db_of is not None:
            if col_rank is not None and (col_rank, col_ranks) != (share_db_of.col_rank, share_db_of.col_ranks):
                raise ValueError(f"a lane of a server is a column shard of its owner's rank ({share_db_of.col_rank} of {share_db_of.col_ranks}) or none")
            col_rank, col_ranks = share_db_of.col_rank, share_db_of.col_ranks
            check(lib().spiral_gpu_server_create_lane(share_db_of.h, C.byref(h)))
            self._db_owner = share_db_of  # keeps the owner alive
        elif col_rank is not None:
            if j_begin or j_end:
                raise ValueError("a column shard holds the whole first dimension: no j-range")
            check(lib().spiral_gpu_server_create_column_shard(C.byref(params), device, col_rank, col_ranks, C.byref(h)))
        else:
            check(lib().spiral_gpu_server_create(C.byref(params), device, j_begin, j_end, C.byref(h)))
        self.h = h
        self.col_rank, self.col_ranks = col_rank, col_ranks
        self.dim0_shard = (j_end - j_begin) if (j_begin or j_end) else self.shape.dim0

    def close(self):
        if getattr(self, "h", None):
            lib().spiral_gpu_server_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- inputs ----
    def set_stream(self, stream_ptr: int):
        check(lib().spiral_gpu_server_set_stream(self.h, C.c_void_p(stream_ptr)))

    def load_db(self, database: np.ndarray):
        check(lib().spiral_gpu_server_load_db(self.h, _p(np.ascontiguousarray(database, dtype=np.uint64))))

    def gen_db(self, seed: int):
        check(lib().spiral_gpu_server_gen_db(self.h, seed))

    def load_db_items(self, items: np.ndarray, coeff_bits: int, first_item: int = 0, n_items: int | None = None):
        """raw ingest: bit-packed plaintext coefficients (uint8 stream, coeff_bits each) or raw u64 MatPoly words (coeff_bits = 64)"""
        items = np.ascontiguousarray(items)
        if n_items is None:
            n_items = items.nbytes * 8 // (4 * N * coeff_bits)
        check(lib().spiral_gpu_server_load_db_items(self.h, items.ctypes.data_as(C.c_void_p), coeff_bits, first_item, n_items))

    def update_db_items(self, items: np.ndarray, coeff_bits: int, item_ids):
        """replace the items item_ids[k] <- plaintext k of `items` (laid out as for load_db_items) in place, in the image's current form, on this
        server's stream; see include/spiral_gpu.h spiral_gpu_server_update_db_items"""
        items, ids = update_args(items, coeff_bits, item_ids, 4)
        check(lib().spiral_gpu_server_update_db_items(self.h, items.ctypes.data_as(C.c_void_p), coeff_bits, _p(ids), len(ids)))

    def read_db_items(self, coeff_bits: int, first_item: int = 0, n_items: int | None = None, out: np.ndarray | None = None) -> np.ndarray:
        """items first_item .. first_item + n_items - 1 (default: to the end) back as plaintexts, uint8 bytes in load_db_items' layout, read from the
        image in its current form; a sharded server fills in its own items only (pass the same `out` to every shard); see include/spiral_gpu.h
        spiral_gpu_server_read_db_items"""
        if n_items is None:
            n_items = self.shape.dim0 * self.shape.num_per - first_item
        out = read_args(self.params, coeff_bits, n_items, 0, out)
        check(lib().spiral_gpu_server_read_db_items(self.h, out.ctypes.data_as(C.c_void_p), coeff_bits, first_item, n_items))
        return out

    def read_db_items_at(self, coeff_bits: int, ids, out: np.ndarray | None = None) -> np.ndarray:
        """the items ids[k] (any order, duplicates allowed) back as plaintexts, plaintext k at k * 1024 * coeff_bits bytes; see read_db_items"""
        ids = read_ids(ids)
        out = read_args(self.params, coeff_bits, len(ids), 0, out)
        check(lib().spiral_gpu_server_read_db_items_at(self.h, out.ctypes.data_as(C.c_void_p), coeff_bits, _p(ids), len(ids)))
        return out

    # ---- content fingerprints (include/spiral_gpu.h "Fingerprints"): computed on the device from the image in its current form ----
    def fingerprint_items(self, key, first_item: int = 0, n_items=None, per_item: bool = False):
        """the combined fingerprint F of items first_item .. first_item + n_items - 1 (default: to the end) under `key`, a pair of ints in [0, 2^64);
        with per_item, (F, the item fingerprints as a uint64 array).  A shard returns its partial sums (0 for an item it does not hold): add the
        shards' values with spiral_amd.fingerprint_add"""
        k = fingerprint_key(key)
        first_item, n_items = fingerprint_range(first_item, n_items, self.shape.dim0 * self.shape.num_per)
        return fingerprint_call(lib().spiral_gpu_server_fingerprint_items, (self.h, k, first_item, n_items), n_items, per_item)

    def fingerprint_items_at(self, key, ids):
        """(F, the item fingerprints as a uint64 array) of the items ids[k] (any order; a repeated id counts as often as it is listed); see
        fingerprint_items"""
        k = fingerprint_key(key)
        ids = read_ids(ids)
        return fingerprint_call(lib().spiral_gpu_server_fingerprint_items_at, (self.h, k, _p(ids), len(ids)), len(ids), True)

    # ---- tracked fingerprints: fingerprint_track, _untrack, _tracked, _tracked_polys, _scrub (_lib.TrackedFingerprint) ----
    _fp_prefix = "spiral_gpu_server"

    def _fp_table(self):
        total = self.shape.dim0 * self.shape.num_per
        return self.dim0_shard * (self.shape.num_per // (self.col_ranks or 1)), 4, total

    # ---- keyed records: kv_load, kv_put, kv_delete, kv_get, kv_stats (_lib.KeyedRecords) ----
    _kv_prefix = "spiral_gpu_server"

    # ---- records of any byte size (include/spiral_gpu.h "Records"); instance: which chunk of each record this server's image holds ----
    def load_records(self, records, record_bytes: int, first_record: int = 0, instance: int = 0):
        """records first_record .. (whole items' worth) from one contiguous byte array, through load_db_items' ingest, padding zero"""
        lay = record_layout(self.params, record_bytes)
        records = record_array(records, record_bytes)
        check(lib().spiral_gpu_server_load_records(self.h, records.ctypes.data_as(C.c_void_p), record_bytes, instance, first_record, records.size // record_bytes))
        return lay

    def update_records(self, records, record_bytes: int, record_ids, instance: int = 0):
        """replace the records record_ids[k] <- record k of `records` in place, in the image's current form, on this server's stream; ids distinct;
        see include/spiral_gpu.h spiral_gpu_server_update_records"""
        record_layout(self.params, record_bytes)
        ids = read_ids(record_ids)
        if np.unique(ids).size != ids.size:
            raise ValueError("record_ids holds a duplicate id")
        records = record_array(records, record_bytes, len(ids))
        check(lib().spiral_gpu_server_update_records(self.h, records.ctypes.data_as(C.c_void_p), record_bytes, instance, _p(ids), len(ids)))

    def read_records(self, record_bytes: int, first_record: int = 0, n_records: int | None = None, out: np.ndarray | None = None, instance: int = 0) -> np.ndarray:
        """records first_record .. first_record + n_records - 1 (default: to the end) as a uint8 array [n][record_bytes], read from the image in its
        current form; a shard or an instance server fills in what it holds (pass the same `out` to each)"""
        lay = record_layout(self.params, record_bytes)
        if n_records is None:
            n_records = lay.capacity - first_record
        out = record_out(record_bytes, n_records, out)
        check(lib().spiral_gpu_server_read_records(self.h, out.ctypes.data_as(C.c_void_p), record_bytes, instance, first_record, n_records))
        return out

    def read_records_at(self, record_bytes: int, record_ids, out: np.ndarray | None = None, instance: int = 0) -> np.ndarray:
        """the records record_ids[k] (any order, duplicates allowed) as a uint8 array [n][record_bytes]; see read_records"""
        record_layout(self.params, record_bytes)
        ids = read_ids(record_ids)
        out = record_out(record_bytes, len(ids), out)
        check(lib().spiral_gpu_server_read_records_at(self.h, out.ctypes.data_as(C.c_void_p), record_bytes, instance, _p(ids), len(ids)))
        return out

    def read_db_item(self, item: int) -> np.ndarray:
        out = np.zeros((2, 2, 2, N), dtype=np.uint64)
        check(lib().spiral_gpu_server_read_db_item(self.h, item, _p(out)))
        return out

    def read_db_slots(self, z_begin: int, nz: int = 1) -> np.ndarray:
        """load_db's layout restricted to this server's j-range: [nz][num_per][n2][j][n0] packed words"""
        out = np.zeros((nz, self.shape.num_per, 2, self.dim0_shard, 2), dtype=np.uint64)
        check(lib().spiral_gpu_server_read_db_slots(self.h, z_begin, nz, _p(out)))
        return out

    def read_db_columns(self, ii_begin: int, n_ii: int = 1) -> np.ndarray:
        """all 2048 slots of the plaintext columns ii_begin .. ii_begin + n_ii - 1: [2048][n_ii][n2][j][n0] packed words"""
        out = np.zeros((N, n_ii, 2, self.dim0_shard, 2), dtype=np.uint64)
        check(lib().spiral_gpu_server_read_db_columns(self.h, ii_begin, n_ii, _p(out)))
        return out

    def fill_db_random(self, seed: int):
        check(lib().spiral_gpu_server_fill_db_random(self.h, seed))

    def run_query_instances(self, instances, responses_ptr: int, finals_ptr: int = 0, pre: bool = True):
        """this server's query against every database instance in `instances` (servers holding the images of one item's `factor` databases): expansion +
        conversion once (pre), then sweep + folding + switch per instance; responses_ptr / finals_ptr: device memory, 6 x 2048 words per instance"""
        arr = (C.c_void_p * len(instances))(*[s.h for s in instances])
        check(lib().spiral_gpu_server_run_query_instances(self.h, arr, len(instances), 1 if pre else 0, C.c_void_p(responses_ptr), C.c_void_p(finals_ptr or None)))

    def answer_instances(self, instances, query):
        """host-buffer form of run_query_instances: (responses [n][3][2][N], folded ciphertexts [n][3][2][N], device us of the item query)"""
        arr = (C.c_void_p * len(instances))(*[s.h for s in instances])
        n = len(instances)
        resp, fin, us = np.zeros((n, 3, 2, N), dtype=np.uint64), np.zeros((n, 3, 2, N), dtype=np.uint64), C.c_double()
        check(lib().spiral_gpu_server_answer_instances(self.h, arr, n, _p(np.ascontiguousarray(query, dtype=np.uint64)), _p(resp), _p(fin), C.byref(us)))
        return resp, fin, us.value

    def set_db_format(self, fmt: int):
        """convert this server's database image in place: DB_PACKED (vector-ALU sweep) <-> DB_LIMBS (matrix-core sweep); see include/spiral_gpu.h"""
        check(lib().spiral_gpu_server_set_db_format(self.h, fmt))

    def db_format(self) -> int:
        return lib().spiral_gpu_server_db_format(self.h)

    def db_device_bytes(self) -> int:
        """device bytes the holder of this server's image keeps for database images"""
        return lib().spiral_gpu_server_db_device_bytes(self.h)

    def share_db(self, owner: "Server"):
        """sweep `owner`'s database image instead of an own copy (a second query lane on one database)"""
        check(lib().spiral_gpu_server_share_db(self.h, owner.h))
        self._db_owner = owner  # keeps the owner alive

    def set_pub_params(self, w_left, w_right, w, v):
        check(lib().spiral_gpu_server_set_pub_params(self.h, _p(w_left), _p(w_right), _p(w), _p(v)))

    def set_query(self, query):
        check(lib().spiral_gpu_server_set_query(self.h, _p(np.ascontiguousarray(query, dtype=np.uint64))))

    def _set_message(self, setter: str, msg):
        """one wire or seeded message to the entry point spiral_gpu_server_<setter>"""
        w = wire_bytes(msg)
        check(getattr(lib(), "spiral_gpu_server_" + setter)(self.h, w.ctypes.data_as(C.c_void_p), w.size))

    def set_pub_params_wire(self, wire):
        """the public parameters as one wire message (ops.raw_to_wire of W_exp_left, W_exp_right, W, V); decoded on the device"""
        self._set_message("set_pub_params_wire", wire)

    def set_query_wire(self, wire):
        """the query in its wire form (ops.raw_to_wire of the raw ciphertexts); decoded on the device into set_query's buffer.  A failure
        leaves no query set"""
        self._set_message("set_query_wire", wire)

    def set_pub_params_seeded(self, msg):
        """the public parameters as one seeded message (include/spiral_gpu.h): row 0 of every matrix generated on the device from the seed, the
        other rows decoded as set_pub_params_wire does"""
        self._set_message("set_pub_params_seeded", msg)

    def set_query_seeded(self, msg):
        """the query in its seeded form: the seed, then row 1 of each ciphertext in its wire form; into set_query's buffer.  A failure leaves no
        query set"""
        self._set_message("set_query_seeded", msg)

    # ---- stages ----
    def expand(self):
        check(lib().spiral_gpu_server_expand(self.h))

    def convert(self):
        check(lib().spiral_gpu_server_convert(self.h))

    def first_dim(self):
        check(lib().spiral_gpu_server_first_dim(self.h))

    def lift(self, reduce_first: bool = False):
        check(lib().spiral_gpu_server_lift(self.h, 1 if reduce_first else 0))

    def fold(self):
        check(lib().spiral_gpu_server_fold(self.h))

    def finish(self):
        check(lib().spiral_gpu_server_finish(self.h))

    def sync(self):
        check(lib().spiral_gpu_server_sync(self.h))

    def use_graphs(self, on: bool = True):
        check(lib().spiral_gpu_server_use_graphs(self.h, 1 if on else 0))

    def set_overlap(self, on=2):
        """0: one stream; 2: the split schedule -- the whole GSW side of the query (the odd tree of the expansion + the conversion) as its own
        launch sequence on the side stream beside the even tree + ScalToMat + sweep (same results, different schedule)"""
        check(lib().spiral_gpu_server_set_overlap(self.h, int(on)))

    def run_pre(self):
        """expand + convert (one hipGraph replay when graphs are on)"""
        check(lib().spiral_gpu_server_run_pre(self.h))

    def run_query(self):
        """run_pre + first_dim + run_post as one group (one hipGraph replay when graphs are on); single GPU only"""
        check(lib().spiral_gpu_server_run_query(self.h))

    def run_pre_sweep(self):
        """run_pre + first_dim as one group: what a rank does before the collective of a sharded answer"""
        check(lib().spiral_gpu_server_run_pre_sweep(self.h))

    def run_post(self, reduce_first: bool = False):
        """lift + fold + finish"""
        check(lib().spiral_gpu_server_run_post(self.h, 1 if reduce_first else 0))

    def set_fold_ranks(self, n_ranks: int):
        check(lib().spiral_gpu_server_set_fold_ranks(self.h, n_ranks))

    def fold_local(self, acc_chunk_ptr: int, out_ct_ptr: int):
        """lift this rank's reduce-scattered chunk and run the local folding rounds -> one raw ct at out_ct_ptr"""
        check(lib().spiral_gpu_server_fold_local(self.h, C.c_void_p(acc_chunk_ptr), C.c_void_p(out_ct_ptr)))

    def fold_root(self, gathered_ptr: int):
        """last log2(G) folding rounds + response switch on the G gathered cts (rank order)"""
        check(lib().spiral_gpu_server_fold_root(self.h, C.c_void_p(gathered_ptr)))

    def set_expand_shard(self, rank: int, n_ranks: int):
        """expand only what rank `rank` of an n_ranks-GPU answer needs (own first-dimension block, every n_ranks-th GSW bit)"""
        check(lib().spiral_gpu_server_set_expand_shard(self.h, rank, n_ranks))

    def gsw_bits_words(self) -> int:
        return int(lib().spiral_gpu_server_gsw_bits_words(self.h))

    def gsw_bits_pack(self, block_ptr: int):
        check(lib().spiral_gpu_server_gsw_bits_pack(self.h, C.c_void_p(block_ptr)))

    def gsw_bits_unpack(self, gathered_ptr: int):
        check(lib().spiral_gpu_server_gsw_bits_unpack(self.h, C.c_void_p(gathered_ptr)))

    def run_expand_pack(self, block_ptr: int):
        """sharded expansion + pack of this rank's GSW bits (one hipGraph replay when graphs are on)"""
        check(lib().spiral_gpu_server_run_expand_pack(self.h, C.c_void_p(block_ptr)))

    def run_unpack_convert_sweep(self, gathered_ptr: int):
        """unpack of the all-gathered GSW bits + convert + first_dim (one hipGraph replay when graphs are on)"""
        check(lib().spiral_gpu_server_run_unpack_convert_sweep(self.h, C.c_void_p(gathered_ptr)))

    def run_scal2mat_sweep(self):
        """ScalToMat + first_dim: the database-dependent part needs no GSW bit, so it can run under their all-gather"""
        check(lib().spiral_gpu_server_run_scal2mat_sweep(self.h))

    def set_sweep_stages(self, n_stages: int):
        """pipelined sweep: accumulators laid out [stage][rank][ct], so each stage's 1/n of the buffer can be reduce-scattered while the next sweeps"""
        check(lib().spiral_gpu_server_set_sweep_stages(self.h, n_stages))

    def max_sweep_stages(self) -> int:
        return int(lib().spiral_gpu_server_max_sweep_stages(self.h))

    def first_dim_stage(self, stage: int):
        check(lib().spiral_gpu_server_first_dim_stage(self.h, stage))

    def run_scal2mat(self):
        """ScalToMat alone (the pipelined schedule issues the sweep stage by stage after it)"""
        check(lib().spiral_gpu_server_run_scal2mat(self.h))

    def run_unpack_gsw(self, gathered_ptr: int):
        """unpack of the all-gathered GSW bits + Regev->GSW conversion (fold keys)"""
        check(lib().spiral_gpu_server_run_unpack_gsw(self.h, C.c_void_p(gathered_ptr)))

    def acc(self):
        nbytes = C.c_size_t()
        ptr = lib().spiral_gpu_server_acc(self.h, C.byref(nbytes))
        return ptr, nbytes.value

    def set_acc(self, device_ptr: int):
        check(lib().spiral_gpu_server_set_acc(self.h, C.c_void_p(device_ptr)))

    def answer(self, query):
        """process_crtd_query on one query -> (final raw ct n1 x n2, response, stage times in us)"""
        fin = np.zeros((3, 2, N), dtype=np.uint64)
        resp = np.zeros((3, 2, N), dtype=np.uint64)
        us = (C.c_double * 8)()
        check(lib().spiral_gpu_server_answer(self.h, _p(np.ascontiguousarray(query, dtype=np.uint64)), _p(fin), _p(resp), us))
        return fin, resp, dict(zip(STAGE_NAMES, list(us)))

    def answer_resident(self):
        us = (C.c_double * 8)()
        check(lib().spiral_gpu_server_answer_resident(self.h, us))
        return dict(zip(STAGE_NAMES, list(us)))

    # ---- introspection ----
    def keep_cts(self, on: bool = True):
        check(lib().spiral_gpu_server_keep_cts(self.h, 1 if on else 0))

    def read_response_wire(self) -> np.ndarray:
        """the last answer's response in its wire form (bit-packed on the device): bytes"""
        n = lib().spiral_gpu_response_wire_bytes(C.byref(self.params), 2)
        out = np.zeros(n, dtype=np.uint8)
        check(lib().spiral_gpu_server_read_response_wire(self.h, out.ctypes.data_as(C.c_void_p), n))
        return out

    def read(self, which: int) -> np.ndarray:
        words = lib().spiral_gpu_server_buffer_words(self.h, which)
        out = np.zeros(words, dtype=np.uint64)
        check(lib().spiral_gpu_server_read(self.h, which, _p(out)))
        s, p = self.shape, self.params
        shapes = {
            BUF_EXPANDED: (s.n_bits, 2, 2, N),
            BUF_CTS: (-1, 3, 2, 2, N),
            BUF_GSW: (p.nu2, 3, s.m2, 2, N),
            BUF_ACC: (s.num_per, 3, 2, 2, N),
            BUF_RAW: (s.num_per, 3, 2, N),
            BUF_FINAL: (3, 2, N),
            BUF_RESPONSE: (3, 2, N),
            BUF_QUERY: (s.n_query_cts, 2, 2, N),
        }
        return out.reshape(shapes[which])

    def write_raw(self, raw_cts):
        check(lib().spiral_gpu_server_write_raw(self.h, _p(np.ascontiguousarray(raw_cts, dtype=np.uint64))))

    def write_acc(self, acc):
        """overwrite the accumulators with [num_per][3][2][2][N] NTT-form words, the layout read(BUF_ACC) returns"""
        acc = np.ascontiguousarray(acc, dtype=np.uint64)
        if acc.size != self.shape.num_per * 6 * 2 * N:
            raise ValueError(f"write_acc: {acc.size} words, the accumulators hold {self.shape.num_per * 6 * 2 * N}")
        check(lib().spiral_gpu_server_write_acc(self.h, _p(acc)))

    def time_sweep(self, iters: int = 20) -> float:
        ms = C.c_float()
        check(lib().spiral_gpu_server_time_sweep(self.h, iters, C.byref(ms)))
        return ms.value

    def sweep_bytes(self) -> int:
        return int(lib().spiral_gpu_server_sweep_bytes(self.h))

    def sweep_device_bytes(self) -> int:
        """bytes one sweep launch has to move on this device (packed database + query records + accumulators)"""
        return int(lib().spiral_gpu_server_sweep_device_bytes(self.h))
