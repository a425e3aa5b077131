// The calls of the resident server that carry the queries of several servers (lanes): an owner and its lanes (create_lane / share_db).  Each
// checks its list in one place (check_lanes over lanes.h) and runs ONE launch sequence on servers[0]'s stream, built from the one-query pieces of
// server.cpp (server_state.h) with every lane in each launch: the batch sweep, whole query batches, item queries against several database
// instances, the batches of a sharded answer, and the batch forms of key binding, query intake and response read-out.
#include "server_state.h"

namespace {

// Checks the lanes servers[0 .. n) of one call and fills their arena offsets: the list, the image, NO_CAPTURE and the layouts in lanes.h, between them
// the base server's own rules for each lane against servers[0].  Unless SWEEP_ONLY: the same parameters and shard, public parameters set, the default
// schedule.  Column shards (create_column_shard): a call takes them where its flags say so (COLUMN_SHARDS, COLUMN_ONLY, a call that only moves data or
// keys, a sweep on each server's own pointers), every lane then one of the same rank and rank count; their arenas are laid out like a base server's of
// the same parameters, so it is this check, not the layout comparison, that keeps the two kinds apart.
int check_lanes(spiral_gpu_server* const* servers, uint32_t n, const char* what, uint32_t needs, Lanes* lanes) {
    const bool whole = !(needs & SWEEP_ONLY), sharded = needs & SHARDED, moves = needs & MOVES_DATA;
    const bool column_ok = needs & (COLUMN_SHARDS | COLUMN_ONLY | MOVES_DATA | GIVES_KEYS | SWEEP_ONLY);
    return check_lane_list(servers, n, what, needs, lanes, [&](uint32_t b) {
        const spiral_gpu_server *S = servers[0], *L = servers[b];
        if (L->col.on && !column_ok) return refuse_column(L, what);
        if ((needs & COLUMN_ONLY) && !L->col.on) return fail("%s: server %u is not a column shard (create_column_shard)", what, b);
        if (!(L->col == S->col))
            return fail("%s: server %u is %s, server 0 %s: the lanes of a call are column shards of one rank and rank count, or none is", what, b,
                        L->col.on ? "a column shard of another rank or rank count" : "no column shard", S->col.on ? "is a column shard" : "is none");
        if (whole && (((needs & NEED_QUERY) && !L->have_query) || (!L->have_pp && !(needs & (GIVES_KEYS | MOVES_DATA))))) return fail("%s: server %u needs its query and public parameters set first", what, b);
        if ((needs & NEED_DB) && !L->img->loaded) return fail("%s: server %u has no database", what, b);
        if ((needs & NEED_RECORDS) && !L->have_records) return fail("%s: server %u has not converted its query (run_pre first)", what, b);
        if (L->device != S->device || L->dim0_shard != S->dim0_shard || L->s.num_per != S->s.num_per ||
            (whole && (memcmp(&L->p, &S->p, sizeof(S->p)) != 0 || L->j0 != S->j0 || L->j1 != S->j1)))
            return fail("%s: server %u differs from server 0 in parameters, device or shard", what, b);
        if ((sharded || !whole) && L->fold_g_log != S->fold_g_log)
            return fail("%s: server %u has %u fold ranks, server 0 has %u", what, b, 1u << L->fold_g_log, 1u << S->fold_g_log);
        if (sharded && (L->ex_shard.g_log != S->ex_shard.g_log || L->ex_shard.rank != S->ex_shard.rank))
            return fail("%s: server %u has another expansion shard than server 0", what, b);
        // (a column shard's fold ranks are part of what it is, not a setting: bind_keys takes it)
        if (whole && !sharded && !moves && (L->acc != L->acc_own.p || (L->fold_g_log && !L->col.on) || L->ex_shard.g_log))
            return fail("%s: server %u has an external accumulator, fold ranks or a sharded expansion set", what, b);
        if (!moves && (L->sweep_k_log || (whole && (L->keep_cts || L->overlap || L->side_pending || L->fold_pair != S->fold_pair || L->fold_chain != S->fold_chain))))
            return fail("%s: server %u has keep_cts, a split or staged schedule or other fold options set", what, b);
        return 0;
    });
}

// Each server's own query records and accumulators, as sweep_queries takes them: the one route to them.  For the lanes of a call whose layouts
// check_lanes has compared they are servers[0]'s plus the lane's arena offset, which is where the lane-aware launches around the sweep read and write
// (records: always; accumulators: check_lanes lets only a sharded batch keep a set_acc buffer, and that sweeps into the caller's, sweep_rank_major).
// first_dim_batch and time_sweep_batch (SWEEP_ONLY: no layout check, no offsets) sweep into servers[b]->acc whatever set_acc has made it.
void server_records(spiral_gpu_server* const* servers, uint32_t n, const uint32_t** qs, uint64_t** acc) {
    for (uint32_t b = 0; b < n; b++) {
        qs[b] = (const uint32_t*)servers[b]->qs.p;
        acc[b] = servers[b]->acc;
    }
}

// the batched sweep (server_state.h sweep_queries) of the image H holds, in whichever form it is in
int sweep_image(const DbImage* H, const uint64_t* limbs, const uint32_t* const* qs, uint64_t* const* acc, uint32_t n, uint32_t g_log, hipStream_t st) {
    if (!limbs && H->format == SPIRAL_GPU_DB_LIMBS) limbs = H->db.p;  // the one image is in limb-plane form: every sweep is the matrix-core one
    return sweep_queries(H->db.p, limbs, H->lay.num_per, 2 * H->lay.dim0, qs, acc, n, g_log, st);
}

// DbImage::limb_view of the image H for a batched sweep of n queries with S's threshold, on S's stream; never call this inside a capture
int limb_image(spiral_gpu_server* S, DbImage* H, uint32_t n, const uint64_t** out) { return H->limb_view(n, S->sweep_mfma_min, S->stream, out); }

// The key of a lane call's capture: the lane count, the limb-plane image its sweep reads (or null), each lane's arena (every pointer the capture holds is
// one of them plus a fixed offset) and the caller's buffers and flags `words`
using Key = std::vector<uint64_t>;
int lane_key(Key* key, spiral_gpu_server* const* servers, uint32_t n, const uint64_t* limbs, std::initializer_list<uint64_t> words) {
    *key = {n, word(limbs)};
    for (uint32_t b = 0; b < n; b++) key->push_back(word(servers[b]->w_left.p));
    for (uint64_t w : words) key->push_back(w);
    return 0;
}

// A lane call's sequence on servers[0]'s stream: the other lanes' streams joined into it, then prepare(&key) -- host work that must not run inside a
// capture (limb_image) and the key -- then body() as servers[0]'s graph `id` (run_graph), then the lanes' streams released
template <class P, class F>
int run_lanes(spiral_gpu_server* const* servers, uint32_t n, GraphId id, P prepare, F body) {
    if (lanes_join(servers, n)) return -1;
    Key key;
    if (int rc = prepare(&key)) return rc;
    if (int rc = run_graph(servers[0], id, servers[0]->stream, key, body)) return rc;
    return lanes_release(servers, n);
}

// The pieces run_query_batch, run_query_instances and run_query_batch_instances share.

// Checks the instances of an item query answered by S's query (same device, shard, database geometry and plaintext modulus, each with a database)
int check_instances(const spiral_gpu_server* S, spiral_gpu_server* const* instances, uint32_t n, const char* what) {
    for (uint32_t k = 0; k < n; k++) {
        const spiral_gpu_server* I = instances[k];
        if (!I) return fail("null instance %u", k);
        if (!I->img->loaded) return fail("%s: instance %u has no database", what, k);
        if (I->col.on) return refuse_column(I, what);
        if (I->device != S->device || I->j0 != S->j0 || I->dim0_shard != S->dim0_shard || I->p.nu1 != S->p.nu1 || I->p.nu2 != S->p.nu2 || I->p.p_db != S->p.p_db ||
            I->p.direct_upload != S->p.direct_upload)
            return fail("%s: instance %u differs from the query's server in device, shard, database geometry or plaintext modulus", what, k);
    }
    return 0;
}

// appends to a capture's key what it bakes in of each instance: its image, the limb-plane image the sweep reads (limbs[k], when given), and the form the
// image is in (the holder's epoch covers the form; update_db_items keeps it: captured graphs replay across updates)
void key_instances(Key* key, spiral_gpu_server* const* instances, uint32_t n, const uint64_t* const* limbs) {
    for (uint32_t k = 0; k < n; k++) {
        const DbImage* H = instances[k]->img;
        for (uint64_t w : {word(H->db.p), word(limbs ? limbs[k] : nullptr), H->epoch, (uint64_t)H->format}) key->push_back(w);
    }
}

// Expansion and conversion of the queries of `lanes` (lane 0 = S): one query is expand_convert, a batch carries every lane in each launch.
// Batches of four or more: the Regev->GSW conversion runs as soon as the odd (GSW-bit) tree of the expansion is complete, after round `stopround`
// (src/spiral.cpp:1700-1702: no odd ciphertext is touched later), and ScalToMat after the last round.  The same launches' work in another order -- at
// these sizes none of them is launch-bound -- but the 24 MiB of GSW matrices and keys per query are then written ~0.3 ms before the sweep instead of
// right in front of it: dirty lines draining into the database stream cost the matrix-core sweep 30-70 us (profiles/r06_sweep_in_situ_batch.txt).
int convert_lanes(spiral_gpu_server* S, const Lanes& lanes) {
    if (lanes.n == 1) return expand_convert(S);
    const bool gsw_early = lanes.n >= 4 && !S->p.direct_upload && S->s.stopround > 0 && S->s.stopround + 1 < S->s.g && S->p.nu2 > 0;
    if (gsw_early && tuning_env("SPIRAL_GSW_ORDER") && atoi(tuning_env("SPIRAL_GSW_ORDER")) == 2) {  // (tuning builds only) ScalToMat first, the GSW side last
        if (expand_lanes(S, lanes)) return -1;
        if (convert_part(S, CONV_S2M, S->stream, false, lanes)) return -1;
        if (convert_part(S, CONV_GSW, S->stream, false, lanes)) return -1;
    } else if (gsw_early) {
        if (expand_lanes(S, lanes, 0, S->s.stopround + 1)) return -1;
        if (convert_part(S, CONV_GSW, S->stream, false, lanes)) return -1;
        if (expand_lanes(S, lanes, S->s.stopround + 1)) return -1;
        if (convert_part(S, CONV_S2M, S->stream, false, lanes)) return -1;
    } else {
        if (expand_lanes(S, lanes)) return -1;
        if (convert_part(S, CONV_BOTH, S->stream, false, lanes)) return -1;
    }
    return 0;
}

// Where an item query's results go (device pointers, each optional): (client q, instance k) at slot q * n_inst + k of resp and fin (6 x 2048 words
// each) and of wire (wire_bytes(p, 2) each).  via_resp: run_query_instances' sequence -- the switch into S->resp, then copies.
struct ItemOut {
    uint64_t *resp = nullptr, *fin = nullptr, *wire = nullptr;
    bool via_resp = false;
};
// The per-instance part of an item query for the queries of `lanes` (lane 0 = S), converted already: for each instance k, the sweep of its image (one
// matrix-core pass for every lane where limbs[k] is given; sweep_queries), the folding, and the switch and wire form straight into the outputs
int item_rounds(spiral_gpu_server* const* servers, const Lanes& lanes, spiral_gpu_server* const* instances, const uint64_t* const* limbs, uint32_t n_inst, const ItemOut& o) {
    const uint32_t* qs[kMaxLanes];
    uint64_t* acc[kMaxLanes];
    spiral_gpu_server* S = servers[0];
    server_records(servers, lanes.n, qs, acc);
    const size_t rw = 6 * kN, ww = wire_bytes(&S->p, 2) / 8;  // (whole words: 2048 values per polynomial)
    for (uint32_t k = 0; k < n_inst; k++) {
        if (sweep_image(instances[k]->img, limbs ? limbs[k] : nullptr, qs, acc, lanes.n, 0, S->stream)) return -1;
        if (o.via_resp) {
            if (run_fold_rounds(S, {.np0 = S->s.num_per, .rounds = S->p.nu2, .src_pk = S->acc, .finish = true})) return -1;
            HIP_OK(hipMemcpyAsync(o.resp + k * rw, S->resp.p, 6 * kPolyBytes, hipMemcpyDeviceToDevice, S->stream));
            if (o.fin) HIP_OK(hipMemcpyAsync(o.fin + k * rw, S->raw.p, 6 * kPolyBytes, hipMemcpyDeviceToDevice, S->stream));
            continue;
        }
        if (run_fold_rounds(S, {.np0 = S->s.num_per, .rounds = S->p.nu2, .src_pk = S->acc, .lanes = lanes})) return -1;
        // row 0 -> q', rows 1.. -> 4*p_db (src/spiral.cpp:1441-1447), lane q's into its slot; without resp, into each lane's own S->resp (for the wire form)
        uint64_t* out = o.resp ? o.resp + k * rw : S->resp.p;
        const int64_t out_stride = o.resp ? (int64_t)(n_inst * rw) : 0;
        launch_rescale2(S->raw.p, out, 2 * kN, 6 * kN, kQ, S->s.qprime, 4 * S->p.p_db, S->stream, lanes, out_stride);
        for (uint32_t q = 0; o.fin && q < lanes.n; q++)
            HIP_OK(hipMemcpyAsync(o.fin + (q * n_inst + k) * rw, S->raw.p + lanes.off[q], 6 * kPolyBytes, hipMemcpyDeviceToDevice, S->stream));
        if (o.wire)
            launch_response_wire(out, o.wire + k * ww, 2 * kN, S->p.qprime_bits, 4 * kN, wire_bits_rest(&S->p), S->stream, lanes, out_stride, (int64_t)(n_inst * ww));
    }
    return 0;
}

// The host tail of the answer_* calls of item queries: device scratch for each output the caller wants (host != null), run(device pointers) between
// two events on S's stream, the outputs downloaded; total_us (optional): the device time between the events
struct HostOut {
    void* host;
    size_t bytes;
};
template <class F>
int answer_on_host(spiral_gpu_server* S, HostOut a, HostOut b, double* total_us, F run) {
    Scratch sc;
    const HostOut out[2] = {a, b};
    void* d[2] = {};
    for (int i = 0; i < 2; i++)
        if (out[i].host && !(d[i] = sc.get((out[i].bytes + 7) / 8))) return fail("device allocation failed");
    HIP_OK(hipEventRecord(S->ev[0], S->stream));
    if (run(d[0], d[1])) return -1;
    HIP_OK(hipEventRecord(S->ev[1], S->stream));
    for (int i = 0; i < 2; i++)
        if (out[i].host) HIP_OK(hipMemcpyAsync(out[i].host, d[i], out[i].bytes, hipMemcpyDeviceToHost, S->stream));
    HIP_OK(hipStreamSynchronize(S->stream));
    if (total_us) {
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, S->ev[0], S->ev[1]));
        *total_us = ms * 1e3;
    }
    return 0;
}

// every argument check of run_query_batch_instances / answer_batch_instances, before anything is uploaded or launched
int check_batch_instances(spiral_gpu_server* const* servers, uint32_t n, spiral_gpu_server* const* instances, uint32_t n_inst, int pre, bool need_query,
                          Lanes* lanes) {
    const char* what = "run_query_batch_instances";
    if (!instances || n_inst == 0) return fail("%s: no servers or no instances", what);
    if (check_lanes(servers, n, what, (need_query ? NEED_QUERY : 0) | (pre ? 0 : NEED_RECORDS) | NO_CAPTURE, lanes)) return -1;
    return check_instances(servers[0], instances, n_inst, what);
}

// ---- batches of a sharded answer (include/spiral_gpu.h: run_pre_sweep_batch ... fold_root_batch) ----------------------------------------------
// The sweep of every lane's query over this rank's shard into the caller's rank-major buffer acc = [rank g][lane b][k < L], L = num_per / G: lane b's
// ciphertext ii = g + G k at (g n + b) L + k.  One pass on the matrix cores where the image is in limb-plane form, else passes of two on the vector
// ALU; a geometry neither kernel covers sweeps each query into its own accumulators and copies its G chunks into place (one strided copy).
int sweep_rank_major(spiral_gpu_server* const* servers, const Lanes& lanes, const uint64_t* limbs, uint64_t* acc_out) {
    spiral_gpu_server* S = servers[0];
    const DbImage* H = S->img;
    const uint32_t n = lanes.n, G = 1u << S->fold_g_log, L = S->s.num_per >> S->fold_g_log, np = S->s.num_per, jm = 2 * S->dim0_shard;
    const size_t chunk = (size_t)L * 6 * kN;
    const uint32_t* qs[kMaxLanes];
    uint64_t* acc[kMaxLanes];
    uint64_t* own[kMaxLanes];
    server_records(servers, lanes.n, qs, own);
    for (uint32_t b = 0; b < n; b++) {
        acc[b] = acc_out + b * chunk;
        own[b] = S->acc_own.p + lanes.off[b];  // (scratch of the fallback: whatever set_acc says, the lane's own buffer)
    }
    if (n == 1 || G == 1)  // [lane][num_per] or one query's own layout: the grouping by ii mod G of the one-query sweep
        return sweep_image(H, limbs, qs, acc, n, S->fold_g_log, S->stream);
    return sweep_queries(H->db.p, limbs, np, jm, qs, acc, n, S->fold_g_log, S->stream, 0, (n - 1) * L, [&](uint32_t b) {
        launch_sweep(H->db.p, qs[b], own[b], np, jm, S->fold_g_log, S->stream);
        HIP_OK(hipMemcpy2DAsync(acc[b], n * chunk * sizeof(uint64_t), own[b], chunk * sizeof(uint64_t), chunk * sizeof(uint64_t), G, hipMemcpyDeviceToDevice,
                                S->stream));
        return 0;
    });
}
}  // namespace

extern "C" {

// "Lane b now serves the client of slot slots[b]" for the n lanes of a batch (an owner and its lanes, as run_query_batch takes them), in one launch on
// servers[0]'s stream (keys.hip): each lane's four key buffers then hold what its own set_pub_params* of the slot's message would have left.  Every
// check comes before the launch, so a failing call changes nothing; a lane whose memo names the slot's present content is left out of the launch.
// Arena addresses do not move, so captured graphs replay with the new keys.  Nothing is synchronised.
int spiral_gpu_server_bind_keys(spiral_gpu_server* const* servers, uint32_t n, spiral_gpu_key_store* store, const uint32_t* slots) {
    const char* what = "bind_keys";
    Lanes lanes;
    if (check_lanes(servers, n, what, NO_CAPTURE | GIVES_KEYS, &lanes)) return -1;
    spiral_gpu_server* S = servers[0];
    uint64_t* const dst[kMessageParts] = {S->w_left.p, S->w_right.p, S->w.p, S->v.p};
    const size_t dst_words[kMessageParts] = {S->w_left.words, S->w_right.words, S->w.words, S->v.words};
    return bind_keys(servers, lanes, store, slots, 0, dst, dst_words, what);
}

// The queries of the n lanes of a batch in one call: message b (wire or seeded form, pageable memory) into servers[b]'s query buffer, through ONE
// lane-aware kernel (query_ingest.hip) on servers[0]'s stream.  Everything is checked before anything is written.  Messages the host can check
// (at most kWireHostCheckPolys polynomials per lane: every compressed query) go up in one copy from a pinned slot and one launch, and the call
// returns without synchronising.  Larger ones (direct upload) go through the staging [lane][chunk] a pass at a time, one launch per pass for all
// lanes, with one synchronisation and one read of the generation-tagged error word at the end; a bad coefficient found there leaves every lane of
// the call without a query.
static_assert((int)FORM_NTT == 0 && (int)FORM_WIRE == SPIRAL_GPU_FORM_WIRE && (int)FORM_SEEDED == SPIRAL_GPU_FORM_SEEDED, "message.h Form is the public enum");
static_assert(Options{}.query_batch_chunk == kWireChunkPolys / kMaxLanes, "the default pass of set_query_batch: set_query_wire's staging shared by all lanes");
int spiral_gpu_server_set_query_batch(spiral_gpu_server* const* servers, uint32_t n, int form, const void* const* msgs, size_t bytes_each) {
    const char* what = "set_query_batch";
    Lanes lanes;
    if (check_lanes(servers, n, what, NO_CAPTURE | MOVES_DATA, &lanes)) return -1;
    spiral_gpu_server* S = servers[0];
    if (form == FORM_NTT) return fail("%s: the NTT form is not taken (one host buffer per part: use set_query); pass the wire or the seeded form", what);
    if (form != SPIRAL_GPU_FORM_WIRE && form != SPIRAL_GPU_FORM_SEEDED) return fail("%s: unknown message form %d", what, form);
    const bool seeded = form == SPIRAL_GPU_FORM_SEEDED;
    const MessageLayout m = query_layout(S->p, S->s);
    const MessagePart& part = m.part[0];
    const size_t npolys = message_polys(m, (Form)form), want = message_bytes(m, (Form)form);
    if (bytes_each != want)
        return fail("%s: %zu bytes per message, the %s form of this query takes %zu", what, bytes_each, seeded ? "seeded" : "wire", want);
    if (seeded && part.rows < 2) return fail("%s: the query is not a run of matrices with rows >= 2", what);
    if (!msgs) return fail("%s: null message list", what);
    for (uint32_t b = 0; b < n; b++)
        if (!msgs[b]) return fail("%s: null message %u", what, b);
    // the error word's index names (lane, message polynomial, coefficient)
    if ((uint64_t)n * npolys * kN >= 0xffffffffull) return fail("%s: %u messages of %zu polynomials exceed the coefficient index range", what, n, npolys);
    if (npolys == 0) return 0;
    QueryBatchIn& Q = S->query_batch_in;
    hipStream_t st = S->stream;
    const uint32_t head = seeded ? kSeedBytes : 0u;
    // a pass covers whole units: one polynomial (wire), the rows 1.. of one matrix and its destinations (seeded)
    const uint32_t unit_msg = seeded ? (part.rows - 1u) * part.cols : 1u, unit_dst = seeded ? part.rows * part.cols : 1u;
    const size_t units = npolys / unit_msg;
    QueryIngestParams qp{};
    qp.head = head;
    qp.dst = S->query.p;
    qp.rows = part.rows;
    qp.cols = part.cols;
    qp.domain = m.domain;
    qp.msg_polys = (uint32_t)npolys;
    qp.lanes = lanes;
    if (Q.last && Q.last_stream != st) HIP_OK(hipStreamWaitEvent(st, Q.last, 0));  // (the stream changed under a call in flight)

    if (npolys <= kWireHostCheckPolys) {
        const size_t stride = head + npolys * kWirePolyBytes;
        QueryBatchIn::Slot& slot = Q.ring[Q.next];
        if (slot.in_flight) HIP_OK(hipEventSynchronize(slot.ev));  // the call two back: its copy has read the slot
        slot.in_flight = false;
        if (slot.bytes < kMaxLanes * stride) {
            if (slot.p) HIP_OK(hipHostFree(slot.p));
            slot.p = nullptr;
            HIP_OK(hipHostMalloc((void**)&slot.p, kMaxLanes * stride, hipHostMallocDefault));
            slot.bytes = kMaxLanes * stride;
        }
        if (!slot.ev) HIP_OK(hipEventCreateWithFlags(&slot.ev, hipEventDisableTiming));
        for (uint32_t b = 0; b < n; b++) {  // checked while copied: a bad coefficient fails before anything goes up
            const uint8_t* msg = (const uint8_t*)msgs[b];
            const int64_t i = wire_first_above_q(msg + head, npolys * kN);
            if (i >= 0)
                return fail("%s: server %u: coefficient %u (polynomial %u, index %u) is above Q", what, b, (uint32_t)i, (uint32_t)i / kN, (uint32_t)i % kN);
            memcpy(slot.p + b * stride, msg, stride);
        }
        if (Q.reserve(kMaxLanes * stride, st)) return -1;
        HIP_OK(hipMemcpyAsync(Q.bytes(), slot.p, n * stride, hipMemcpyHostToDevice, st));
        if (lanes_join(servers, n)) return -1;
        qp.stage = Q.bytes();
        qp.lane_stride = stride;
        qp.err = reinterpret_cast<uint32_t*>(Q.stage.p);
        qp.gen = ++Q.gen;  // (never read: the host has checked)
        launch_query_ingest(S->tb, qp, seeded ? QUERY_SEEDED : QUERY_WIRE, (uint32_t)(units * unit_dst), st);
        HIP_OK(hipGetLastError());
        for (uint32_t b = 0; b < n; b++) {
            servers[b]->have_query = true;
            servers[b]->have_records = false;
        }
        if (lanes_release(servers, n)) return -1;
        HIP_OK(hipEventRecord(slot.ev, st));
        slot.in_flight = true;
        Q.last = slot.ev;
        Q.last_stream = st;
        Q.next ^= 1u;
        return 0;
    }

    const size_t chunk = std::max<size_t>(std::min<size_t>(options().query_batch_chunk, npolys), unit_msg) / unit_msg;  // units per pass
    const size_t stride = head + chunk * unit_msg * kWirePolyBytes;
    if (Q.reserve(kMaxLanes * stride, st)) return -1;
    if (!Q.host_err) HIP_OK(hipHostMalloc((void**)&Q.host_err, sizeof(uint64_t), hipHostMallocDefault));
    qp.stage = Q.bytes();
    qp.lane_stride = stride;
    qp.err = reinterpret_cast<uint32_t*>(Q.stage.p);
    qp.gen = ++Q.gen;
    for (uint32_t b = 0; b < n; b++) servers[b]->have_query = servers[b]->have_records = false;  // from the first write on nothing answers from these buffers
    if (lanes_join(servers, n)) return -1;
    for (size_t u0 = 0; u0 < units; u0 += chunk) {
        const size_t nu = std::min(chunk, units - u0);
        for (uint32_t b = 0; b < n; b++) {  // (the first pass takes the seed with it)
            const uint8_t* msg = (const uint8_t*)msgs[b];
            if (u0 == 0)
                HIP_OK(hipMemcpyAsync(Q.bytes() + b * stride, msg, head + nu * unit_msg * kWirePolyBytes, hipMemcpyHostToDevice, st));
            else
                HIP_OK(hipMemcpyAsync(Q.bytes() + b * stride + head, msg + head + u0 * unit_msg * kWirePolyBytes, nu * unit_msg * kWirePolyBytes,
                                      hipMemcpyHostToDevice, st));
        }
        qp.first_dst = (uint32_t)(u0 * unit_dst);
        qp.first_msg = (uint32_t)(u0 * unit_msg);
        launch_query_ingest(S->tb, qp, seeded ? QUERY_SEEDED : QUERY_WIRE, (uint32_t)(nu * unit_dst), st);
    }
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(Q.host_err, Q.stage.p, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (lanes_release(servers, n)) return -1;
    HIP_OK(hipStreamSynchronize(st));
    Q.last = nullptr;
    const uint64_t err = *Q.host_err;
    if ((uint32_t)(err >> 32) == (uint32_t)~qp.gen) {
        const uint32_t i = (uint32_t)err, c = i % (uint32_t)(npolys * kN);
        return fail("%s: server %u: coefficient %u (polynomial %u, index %u) is above Q", what, i / (uint32_t)(npolys * kN), c, c / kN, c % kN);
    }
    for (uint32_t b = 0; b < n; b++) servers[b]->have_query = true;
    return 0;
}

// The wire forms of the n lanes' last responses in one launch, one copy and one synchronisation: lane b's at out + b * response_wire_bytes, the
// bytes its own read_response_wire returns
int spiral_gpu_server_read_response_wire_batch(spiral_gpu_server* const* servers, uint32_t n, void* out, size_t capacity) {
    const char* what = "read_response_wire_batch";
    Lanes lanes;
    if (check_lanes(servers, n, what, NO_CAPTURE | MOVES_DATA, &lanes)) return -1;
    spiral_gpu_server* S = servers[0];
    if (!out) return fail("%s: null output buffer", what);
    const size_t nbytes = wire_bytes(&S->p, 2);
    if (capacity < n * nbytes) return fail("%s: response buffer of %zu bytes, the wire forms of %u lanes need %zu", what, capacity, n, n * nbytes);
    if (S->wire.words * 8 < n * nbytes && (S->wire.release(), S->wire.alloc(n * nbytes / 8))) return -1;
    if (lanes_join(servers, n)) return -1;
    launch_response_wire(S->resp.p, S->wire.p, 2 * kN, S->p.qprime_bits, 4 * kN, wire_bits_rest(&S->p), S->stream, lanes, 0, (int64_t)(nbytes / 8));
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(out, S->wire.p, n * nbytes, hipMemcpyDeviceToHost, S->stream));
    if (lanes_release(servers, n)) return -1;
    HIP_OK(hipStreamSynchronize(S->stream));
    return 0;
}

// One pass over the database for the queries of n servers that sweep the SAME image (an owner and its lanes, create_lane /
// share_db): server b's query records against the database into server b's accumulators.  The launch goes on servers[0]'s stream;
// every other lane's stream is made to wait for it and it for theirs (events), so each lane's run_pre / run_post on its own stream
// stay correctly ordered around it.  Geometries the batched kernel does not cover fall back to one sweep per lane.
int spiral_gpu_server_first_dim_batch(spiral_gpu_server* const* servers, uint32_t n) {
    if (servers && n == 1 && servers[0]) return spiral_gpu_server_first_dim(servers[0]);
    Lanes lanes;
    if (check_lanes(servers, n, "first_dim_batch", NEED_DB | NEED_RECORDS | SWEEP_ONLY, &lanes)) return -1;  // a failure leaves no lane swept
    spiral_gpu_server* S0 = servers[0];
    const uint32_t* qs[kMaxLanes];
    uint64_t* acc[kMaxLanes];
    server_records(servers, n, qs, acc);
    const uint64_t* limbs;
    if (limb_image(S0, S0->img, n, &limbs)) return -1;
    if (!limbs && !sweep_batch_ok(srv_np(S0), 2 * S0->dim0_shard)) {  // (a packed image: limb planes always come back as `limbs`)
        for (uint32_t b = 0; b < n; b++)
            if (spiral_gpu_server_first_dim(servers[b])) return -1;
        return 0;
    }
    if (lanes_join(servers, n)) return -1;  // the lanes' records must be complete
    if (sweep_image(S0->img, limbs, qs, acc, n, sweep_g_log(S0), S0->stream)) return -1;
    mark_raw_stale(servers, n);
    return lanes_release(servers, n);
}

// B <= kMaxLanes whole queries -- one per server: an owner and its lanes (create_lane), all with the same parameters, each with its own
// client's keys and query -- as ONE launch sequence: every launch of expansion, conversion, lift, folding and the switch carries all B queries
// (gridDim.z = B, kernels.h Lanes), and the sweep makes one pass over the database for all of them (sweep_mfma_kernel; sweep_queries).  The reference
// answers one query per process_crtd_query (src/spiral.cpp:2337-2406); this is throughput, not latency: a query's ~50 launch-bound launches
// cost the same ~5 us whether they carry one query or four.  Every lane's buffers end up exactly as after its own run_query.
// The sequence runs on servers[0]'s stream (captured once per lane set into a hipGraph when servers[0] has use_graphs on); the other
// lanes' streams are ordered before and after it with events, as in first_dim_batch.
int spiral_gpu_server_run_query_batch(spiral_gpu_server* const* servers, uint32_t n) {
    if (servers && n == 1 && servers[0]) return spiral_gpu_server_run_query(servers[0]);
    Lanes lanes;
    if (check_lanes(servers, n, "run_query_batch", NEED_QUERY | NEED_DB, &lanes)) return -1;  // every lane is validated before anything is launched
    spiral_gpu_server* S = servers[0];
    const uint64_t* limbs = nullptr;
    const int rc = run_lanes(
        servers, n, G_BATCH,
        [&](Key* key) {  // (limb_image: not inside the capture, it may build the image)
            return limb_image(S, S->img, n, &limbs) ? -1 : lane_key(key, servers, n, limbs, {});
        },
        [&]() {
            if (convert_lanes(S, lanes)) return -1;
            const uint32_t* qs[kMaxLanes];
            uint64_t* acc[kMaxLanes];
            server_records(servers, n, qs, acc);
            if (sweep_image(S->img, limbs, qs, acc, n, 0, S->stream)) return -1;  // one pass on the matrix cores where the limb-plane image exists
            return run_fold_rounds(S, {.np0 = S->s.num_per, .rounds = S->p.nu2, .src_pk = S->acc, .finish = true, .lanes = lanes});
        });
    if (!rc) mark_swept(servers, n);
    return rc;
}

// One query against n INSTANCES of the database.  An item larger than one plaintext (configs[3]: 100 KB items, 15 360-byte plaintexts) is
// factor = ceil(item / plaintext) database instances (select_params.py:297-298); the client sends ONE query, the server expands and converts it once and
// answers it against every instance: first dimension + folding + response switch per instance, `factor` responses (the reference runs one instance and
// multiplies fdim_us, fold_us and the response size by the factor, select_params.py:409-418).  S holds the query (its public parameters, query, records,
// keys, accumulators); instances[k] hold the images (servers with the same geometry on the same device, each with its own database; S may be one of them).
// pre != 0: expansion + conversion first (run_pre's work), else S must have converted its query already.  Instance k's switched response goes to
// responses + k * 6 * 2048 words and, when finals != null, its folded ciphertext to finals + k * 6 * 2048 (device pointers).  One launch sequence on S's
// stream, sweeps back to back; a hipGraph per (instance set, output buffers) when S has use_graphs on.
int spiral_gpu_server_run_query_instances(spiral_gpu_server* S, spiral_gpu_server* const* instances, uint32_t n, int pre, void* responses, void* finals) {
    if (!S || !instances || n == 0 || !responses) return fail("null argument");
    Lanes one;  // (S alone, on the default schedule)
    if (check_lanes(&S, 1, "run_query_instances", NEED_QUERY | (pre ? 0 : NEED_RECORDS), &one)) return -1;
    if (check_instances(S, instances, n, "run_query_instances")) return -1;
    std::vector<uint64_t> key{word(responses), word(finals), pre != 0};
    key_instances(&key, instances, n, nullptr);
    if (srv_join_side(S)) return -1;
    ItemOut o;
    o.resp = (uint64_t*)responses;
    o.fin = (uint64_t*)finals;
    o.via_resp = true;
    auto body = [&]() {
        if (pre && expand_convert(S)) return -1;
        return item_rounds(&S, Lanes{}, instances, nullptr, n, o);
    };
    if (int rc = run_graph(S, G_INSTANCES, S->stream, key, body)) return rc;
    if (pre)
        mark_swept(&S, 1);
    else
        mark_raw_stale(&S, 1);
    return 0;
}

// the same from host buffers, as spiral_gpu_server_answer is to the stages: upload the query, answer it against the n instances, download the n
// responses (n x 6 x 2048 words) and, when finals != null, the folded ciphertexts; total_us (optional): device time of the whole item query
int spiral_gpu_server_answer_instances(spiral_gpu_server* S, spiral_gpu_server* const* instances, uint32_t n, const uint64_t* query, uint64_t* responses,
                                       uint64_t* finals, double* total_us) {
    if (!S || !instances || n == 0 || !query || !responses) return fail("null argument");
    if (refuse_column(S, "answer_instances")) return -1;
    HIP_OK(hipSetDevice(S->device));
    if (spiral_gpu_server_set_query(S, query)) return -1;
    const size_t bytes = (size_t)n * 6 * kPolyBytes;
    return answer_on_host(S, {responses, bytes}, {finals, bytes}, total_us,
                          [&](void* d_resp, void* d_fin) { return spiral_gpu_server_run_query_instances(S, instances, n, 1, d_resp, d_fin); });
}

// B <= kMaxLanes clients' item queries against the same n_inst instances (include/spiral_gpu.h): the clients' expansion and conversion as in
// run_query_batch, then per instance one sweep for all B (sweep_queries: one matrix-core pass where the geometry has limb planes), the folding with
// every lane in each launch, and the switch and wire form written straight into the callers' [client][instance] slots.  B = 1 is run_query_instances'
// sequence (NoLanes launches) with the switch into the output and the wire form added.  One hipGraph per key on servers[0] with use_graphs on.
int spiral_gpu_server_run_query_batch_instances(spiral_gpu_server* const* servers, uint32_t n, spiral_gpu_server* const* instances, uint32_t n_inst, int pre,
                                                void* responses, void* finals, void* wire) {
    Lanes lanes;
    if (!responses && !wire) return fail("run_query_batch_instances: no output (responses or wire)");
    if (check_batch_instances(servers, n, instances, n_inst, pre, true, &lanes)) return -1;
    spiral_gpu_server* S = servers[0];
    if (srv_join_side(S)) return -1;
    std::vector<const uint64_t*> limbs(n_inst);
    ItemOut o;
    o.resp = (uint64_t*)responses;
    o.fin = (uint64_t*)finals;
    o.wire = (uint64_t*)wire;
    const int rc = run_lanes(
        servers, n, G_BATCH_INSTANCES,
        [&](Key* key) {
            // each instance image in the form the sweep of B queries reads, converted in place on first use (never inside the capture)
            for (uint32_t k = 0; k < n_inst; k++)
                if (limb_image(S, instances[k]->img, n, &limbs[k])) return -1;
            lane_key(key, servers, n, nullptr, {word(responses), word(finals), word(wire), pre != 0});
            key_instances(key, instances, n_inst, limbs.data());
            return 0;
        },
        [&]() {
            if (pre && convert_lanes(S, lanes)) return -1;
            return item_rounds(servers, lanes, instances, limbs.data(), n_inst, o);
        });
    if (rc) return rc;
    if (pre)
        mark_swept(servers, n);
    else
        mark_raw_stale(servers, n);
    return 0;
}

// the same from host buffers: upload the B queries, answer them, download the B x n_inst responses and / or wire forms; total_us: device time of the batch
int spiral_gpu_server_answer_batch_instances(spiral_gpu_server* const* servers, uint32_t n, spiral_gpu_server* const* instances, uint32_t n_inst,
                                             const uint64_t* const* queries, uint64_t* responses, void* wire, double* total_us) {
    Lanes lanes;
    if (!queries || (!responses && !wire)) return fail("answer_batch_instances: null queries or no output (responses or wire)");
    if (check_batch_instances(servers, n, instances, n_inst, 1, false, &lanes)) return -1;
    for (uint32_t b = 0; b < n; b++)
        if (!queries[b]) return fail("answer_batch_instances: null query %u", b);
    for (uint32_t b = 0; b < n; b++)
        if (spiral_gpu_server_set_query(servers[b], queries[b])) return -1;
    const size_t slots = (size_t)n * n_inst;
    return answer_on_host(servers[0], {responses, slots * 6 * kPolyBytes}, {wire, slots * wire_bytes(&servers[0]->p, 2)}, total_us, [&](void* d_resp, void* d_wire) {
        return spiral_gpu_server_run_query_batch_instances(servers, n, instances, n_inst, 1, d_resp, nullptr, d_wire);
    });
}

int spiral_gpu_server_run_pre_sweep_batch(spiral_gpu_server* const* servers, uint32_t n, void* acc) {
    const char* what = "run_pre_sweep_batch";
    Lanes lanes;
    if (check_lanes(servers, n, what, SHARD_LANES | NEED_QUERY | NEED_DB, &lanes)) return -1;
    if (!acc) return fail("%s: null accumulator buffer", what);
    spiral_gpu_server* S = servers[0];
    if (S->ex_shard.g_log) return fail("%s: the expansion is sharded: run_expand_pack_batch, the all-gather, then run_unpack_convert_sweep_batch", what);
    const uint64_t* limbs;
    if (limb_image(S, S->img, n, &limbs)) return -1;  // (not inside a capture: it may convert the image)
    const int rc = run_lanes(servers, n, G_SHARD_PRE_SWEEP, [&](Key* k) { return lane_key(k, servers, n, limbs, {word(acc)}); }, [&]() {
        if (convert_lanes(S, lanes)) return -1;
        return sweep_rank_major(servers, lanes, limbs, (uint64_t*)acc);
    });
    if (!rc) mark_swept(servers, n);
    return rc;
}

int spiral_gpu_server_run_expand_pack_batch(spiral_gpu_server* const* servers, uint32_t n, void* bits_out) {
    const char* what = "run_expand_pack_batch";
    Lanes lanes;
    if (check_lanes(servers, n, what, SHARD_LANES | NEED_QUERY, &lanes)) return -1;
    if (!bits_out) return fail("%s: null output buffer", what);
    spiral_gpu_server* S = servers[0];
    return run_lanes(servers, n, G_SHARD_EXPAND_PACK, [&](Key* k) { return lane_key(k, servers, n, nullptr, {word(bits_out)}); }, [&]() {
        if (expand_lanes(S, lanes)) return -1;
        launch_gsw_bits_pack_lanes(S->cv.p, (uint64_t*)bits_out, S->ex_shard.rank, 1u << S->ex_shard.g_log, S->s.ell * S->p.nu2, lanes, S->stream);
        return 0;
    });
}

int spiral_gpu_server_run_unpack_convert_sweep_batch(spiral_gpu_server* const* servers, uint32_t n, const void* gathered_bits, void* acc) {
    const char* what = "run_unpack_convert_sweep_batch";
    Lanes lanes;
    if (check_lanes(servers, n, what, SHARD_LANES | NEED_QUERY | NEED_DB, &lanes)) return -1;
    if (!gathered_bits || !acc) return fail("%s: null buffer", what);
    spiral_gpu_server* S = servers[0];
    const uint64_t* limbs;
    if (limb_image(S, S->img, n, &limbs)) return -1;
    const int rc = run_lanes(servers, n, G_SHARD_UNPACK_SWEEP, [&](Key* k) { return lane_key(k, servers, n, limbs, {word(gathered_bits), word(acc)}); }, [&]() {
        launch_gsw_bits_unpack_lanes(S->cv.p, (const uint64_t*)gathered_bits, 1u << S->ex_shard.g_log, S->s.ell * S->p.nu2, lanes, S->stream);
        if (convert_part(S, CONV_BOTH, S->stream, false, lanes)) return -1;
        return sweep_rank_major(servers, lanes, limbs, (uint64_t*)acc);
    });
    if (!rc) mark_swept(servers, n);
    return rc;
}

// the caller's reduce-scattered chunk [lane][k < L] into each lane's own accumulators (the fold's first round reads them with the lanes' arena
// offsets), the first nu2 - log2 G rounds for every lane in the same launches, each lane's folded ciphertext out to out_cts + b * 6 * 2048
int spiral_gpu_server_fold_local_batch(spiral_gpu_server* const* servers, uint32_t n, const void* chunk, void* out_cts) {
    const char* what = "fold_local_batch";
    Lanes lanes;
    if (check_lanes(servers, n, what, SHARD_LANES, &lanes)) return -1;
    if (!chunk || !out_cts) return fail("%s: null buffer", what);
    spiral_gpu_server* S = servers[0];
    const uint32_t L = S->s.num_per >> S->fold_g_log;
    const size_t ctw = 6 * kN, cw = (size_t)L * ctw;
    const int rc = run_lanes(servers, n, G_SHARD_FOLD_LOCAL, [&](Key* k) { return lane_key(k, servers, n, nullptr, {word(chunk), word(out_cts)}); }, [&]() {
        for (uint32_t b = 0; b < n; b++)
            HIP_OK(hipMemcpyAsync(S->acc_own.p + lanes.off[b], (const uint64_t*)chunk + b * cw, cw * sizeof(uint64_t), hipMemcpyDeviceToDevice, S->stream));
        if (run_fold_rounds(S, {.np0 = L, .rounds = S->p.nu2 - S->fold_g_log, .src_pk = S->acc_own.p, .pre_reduce = true, .lanes = lanes})) return -1;
        for (uint32_t b = 0; b < n; b++)
            HIP_OK(hipMemcpyAsync((uint64_t*)out_cts + b * ctw, S->raw.p + lanes.off[b], ctw * sizeof(uint64_t), hipMemcpyDeviceToDevice, S->stream));
        return 0;
    });
    if (!rc) mark_raw_stale(servers, n);
    return rc;
}

// the all-gathered [rank][lane][6 x 2048] into each lane's raw buffer (one strided copy per lane), the last log2 G rounds and the switch for every lane;
// optionally the responses to responses + b * 6 * 2048 and the wire forms to wire + b * wire_bytes
int spiral_gpu_server_fold_root_batch(spiral_gpu_server* const* servers, uint32_t n, const void* gathered_cts, void* responses, void* wire) {
    const char* what = "fold_root_batch";
    Lanes lanes;
    if (check_lanes(servers, n, what, SHARD_LANES | COLUMN_SHARDS, &lanes)) return -1;
    if (!gathered_cts) return fail("%s: null buffer", what);
    spiral_gpu_server* S = servers[0];
    const uint32_t G = 1u << S->fold_g_log;
    const size_t ctw = 6 * kN, ww = wire_bytes(&S->p, 2) / 8;
    const int rc = run_lanes(servers, n, G_SHARD_FOLD_ROOT, [&](Key* k) { return lane_key(k, servers, n, nullptr, {word(gathered_cts), word(responses), word(wire)}); }, [&]() {
        for (uint32_t b = 0; b < n; b++)
            HIP_OK(hipMemcpy2DAsync(S->raw.p + lanes.off[b], ctw * sizeof(uint64_t), (const uint64_t*)gathered_cts + b * ctw, n * ctw * sizeof(uint64_t),
                                    ctw * sizeof(uint64_t), G, hipMemcpyDeviceToDevice, S->stream));
        if (run_fold_rounds(S, {.np0 = G, .d0 = S->p.nu2 - S->fold_g_log, .rounds = S->fold_g_log, .finish = true, .lanes = lanes})) return -1;
        if (responses)  // (the same switch again, into the caller's [lane] slots)
            launch_rescale2(S->raw.p, (uint64_t*)responses, 2 * kN, 6 * kN, kQ, S->s.qprime, 4 * S->p.p_db, S->stream, lanes, (int64_t)ctw);
        if (wire) launch_response_wire(S->resp.p, (uint64_t*)wire, 2 * kN, S->p.qprime_bits, 4 * kN, wire_bits_rest(&S->p), S->stream, lanes, 0, (int64_t)ww);
        return 0;
    });
    if (!rc) mark_raw_stale(servers, n);
    return rc;
}

// A column shard's whole local share (include/spiral_gpu.h): every lane's expansion and conversion, ONE pass over the shard's L columns for all lanes
// straight into each lane's own accumulators -- finished sums of its own chunk ii = rank + G k, in the order k: no rank-major buffer, nothing to reduce,
// no chunk to copy in -- the first nu2 - log2 G fold rounds on them as they stand (canonical words: no pre_reduce), each lane's ciphertext out
int spiral_gpu_server_run_column_batch(spiral_gpu_server* const* servers, uint32_t n, void* out_cts) {
    const char* what = "run_column_batch";
    Lanes lanes;
    if (check_lanes(servers, n, what, SHARD_LANES | COLUMN_ONLY | NEED_QUERY | NEED_DB, &lanes)) return -1;
    if (!out_cts) return fail("%s: null output buffer", what);
    spiral_gpu_server* S = servers[0];
    const uint32_t L = srv_np(S);
    const size_t ctw = 6 * kN;
    if (S->img->lay.num_per != L || S->img->lay.dim0 != S->s.dim0) return fail("%s: the image is not this column shard's", what);  // (cannot happen: share_db compares)
    const uint64_t* limbs;
    if (limb_image(S, S->img, n, &limbs)) return -1;  // (not inside a capture: it may convert the image)
    const bool on_limbs = limbs || S->img->format == SPIRAL_GPU_DB_LIMBS;
    const uint64_t launched = g_mfma_sweeps.load(std::memory_order_relaxed);
    const int rc = run_lanes(
        servers, n, G_COLUMN_BATCH, [&](Key* k) { return lane_key(k, servers, n, limbs, {word(out_cts), (uint64_t)S->img->format}); },
        [&]() {
            if (convert_lanes(S, lanes)) return -1;
            const uint32_t* qs[kMaxLanes];
            uint64_t* acc[kMaxLanes];
            server_records(servers, n, qs, acc);
            for (uint32_t b = 0; b < n; b++) acc[b] = S->acc_own.p + lanes.off[b];  // (whatever set_acc says: where the fold below reads)
            if (sweep_image(S->img, limbs, qs, acc, n, 0, S->stream)) return -1;
            if (run_fold_rounds(S, {.np0 = L, .rounds = S->p.nu2 - S->col.g_log, .src_pk = S->acc_own.p, .lanes = lanes})) return -1;
            for (uint32_t b = 0; b < n; b++)
                HIP_OK(hipMemcpyAsync((uint64_t*)out_cts + b * ctw, S->raw.p + lanes.off[b], ctw * sizeof(uint64_t), hipMemcpyDeviceToDevice, S->stream));
            return 0;
        });
    // "mfma_sweeps" counts this call's pass whether it was launched or replayed: the launcher counts the first, a replay runs no host code
    if (!rc && on_limbs && g_mfma_sweeps.load(std::memory_order_relaxed) == launched) g_mfma_sweeps.fetch_add(1, std::memory_order_relaxed);
    if (!rc) mark_swept(servers, n);
    return rc;
}

int spiral_gpu_server_time_sweep_batch(spiral_gpu_server* const* servers, uint32_t n, int iters, float* avg_ms) {
    if (!avg_ms || iters <= 0) return fail("time_sweep_batch: bad argument");
    Lanes lanes;
    if (check_lanes(servers, n, "time_sweep_batch", NEED_DB | NEED_RECORDS | SWEEP_ONLY, &lanes)) return -1;  // (first_dim_batch's lanes)
    spiral_gpu_server* S = servers[0];
    const uint32_t* qs[kMaxLanes];
    uint64_t* acc[kMaxLanes];
    server_records(servers, n, qs, acc);
    mark_raw_stale(servers, n);
    const uint64_t* limbs;
    if (limb_image(S, S->img, n, &limbs)) return -1;
    HIP_OK(hipDeviceSynchronize());  // (the lanes' streams: their records are complete)
    HIP_OK(hipEventRecord(S->ev[0], S->stream));
    for (int i = 0; i < iters; i++)
        if (sweep_image(S->img, limbs, qs, acc, n, sweep_g_log(S), S->stream)) return -1;
    HIP_OK(hipEventRecord(S->ev[1], S->stream));
    HIP_OK(hipStreamSynchronize(S->stream));
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, S->ev[0], S->ev[1]));
    *avg_ms = ms / iters;
    return 0;
}

}  // extern "C"
