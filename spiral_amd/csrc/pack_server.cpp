// SpiralPack / SpiralStreamPack: host orchestration and C ABI (server half of testHighRate, reference
// src/testing.cpp:1009-1081).  Kernels: pack.hip, ntt.hip (LD_PDIGIT / LD_DBGEN1), poly.hip (matmul, rescale), sweep_mfma.hip (the batched
// first-dimension sweep of answer_batch: several lanes' queries in one pass over the trial images, from their limb-plane form).
#include "db_image.h"
#include "key_store.h"
#include "kv_host.h"
#include "message.h"

using namespace spiral;
using namespace spiral::host;

// The buffers the folding, packing and switch of one client write: its own (one instance), or one group of G instances of answer_batch_instances
// (instance j's part of each buffer j x its one-instance words further on: the folding and packing launches take the group as G * n^2 trials)
struct PkBufs {
    uint64_t *acc, *raw, *fold_d, *fold_c, *fold_c2, *ginv, *ct2, *res, *pk_raw, *resp, *wire;
    size_t acc_words, slot_words, wire_words;  // one instance's words of acc / of res, pk_raw and resp / of wire (whole words: 2048 values per polynomial)
};

struct spiral_gpu_pack_server : LaneHost {  // (lanes.h: device, stream, img, arena and its layout record, ev_lane)
    spiral_gpu_params p;
    spiral_gpu_pack_shape s;
    uint32_t out_n = 0;
    uint32_t t0 = 0, nt = 0;  // this server's trials [t0, t0 + nt) of the out_n^2 (all of them unless created sharded)
    bool own_stream = true;
    DeviceTables tb;
    bool have_pp = false;
    bool packed_after_front = false;  // event 6 belongs to the same answer as events 0..5
    bool events_elsewhere = false;    // the last call that answered this server's query recorded its stages on ANOTHER server's events (a lane-form
                                      // batch or item call, as lane 1 .. n - 1): events 0..6 are an older call's, or were never recorded
    uint32_t n_cv = 0;
    // every buffer below but the lazy ones (stage, wire_in, item) is a piece of `arena`, carved in one fixed order (pk_layout): servers with equal
    // parameters, out_n and trial range have equal layouts
    DevBuf w_left, w_right, v, v_w, query, cv, ex_raw, ex_g, gs_raw, gs_chat, gs_tmp, gsw, key, qs1;  // the client's own
    DevBuf gath;  // pack_gathered_batch: this client's out_n^2 folded ciphertexts in trial order, regrouped from the gathered blocks (a piece of the
                  // arena like the rest, so that the pack's readers find every lane's at the lane's offset)
    PkBufs own{};  // what one answer writes
    DevBuf stage;
    DevBuf wire_batch;  // pack_gathered_batch as servers[0]: the lanes' wire forms side by side for the one copy; grown on first use, kept
    WireIn wire_in;  // the staging of the wire and seeded forms (message.h ingest)
    KeyMemo key_memo;  // the store slot the four key buffers were last bound from (bind_keys); none once set_pub_params* has written them
    hipEvent_t ev[8] = {};  // [0..6] the stages of an answer, [7] batch sweep / item call end (its stream is ordered around another server's call by ev_lane)
    bool have_records = false;  // qs1 holds the records of a converted query (time_sweep_batch)
    // img, the trial images this server sweeps (db_image.h): its own, or its owner's, of which a query lane (create_lane) holds a reference and
    // which it never writes
    DevBuf item;            // answer_batch_instances as a client: the arena of its item groups of more than one instance, kept for the next call
    uint32_t item_cap = 0;  // instances per group the arena holds
};

namespace {

int pack_shape_of(const spiral_gpu_params* p, uint32_t out_n, spiral_gpu_pack_shape* s) {  // src/testing.cpp:777-801
    spiral_gpu_shape base;
    spiral_gpu_params q = *p;
    q.direct_upload = 1;  // validate the common fields without the base path's query-size rule
    if (shape_of(&q, &base)) return -1;
    if (out_n < 1 || out_n > 16) return fail("out_n out of range");
    if (p->nu2 < 1 || p->nu1 < 1) return fail("SpiralPack needs nu1 >= 1 and nu2 >= 1");
    s->dim0 = base.dim0;
    s->num_per = base.num_per;
    s->ell = base.ell;
    s->trials = out_n * out_n;
    s->qprime = base.qprime;
    if (p->direct_upload) {
        s->g = s->stopround = s->n_left = s->n_right = 0;
        s->n_query_cts = s->dim0 + p->nu2 * 2 * s->ell;
    } else {
        s->g = ceil_log2((uint64_t)s->ell * p->nu2 + s->dim0);
        s->stopround = ceil_log2((uint64_t)s->ell * p->nu2);
        s->n_left = s->g;
        s->n_right = s->stopround + 1;
        s->n_query_cts = 1;
        if (s->g > kLogN || s->stopround == 0 || s->stopround >= s->g) return fail("query does not fit one polynomial");
    }
    return 0;
}

// the owner of the images S sweeps, while it lives (S itself, or a lane's owner)
spiral_gpu_pack_server* pk_owner(const spiral_gpu_pack_server* S) { return (spiral_gpu_pack_server*)S->img->owner; }

// what writes the trial images goes through the server that owns them: a lane refuses (verb null: set_db_format's wording)
int pk_refuse_lane(const spiral_gpu_pack_server* S, const char* verb) {
    if (S->img->owner == S) return 0;
    return verb ? fail("this server is a lane: it sweeps its owner's database, %s it through the owner", verb)
                : fail("this server is a lane: convert the image through its owner");
}
int pk_check_trial(const spiral_gpu_pack_server* S, uint32_t trial) {
    if (trial >= S->t0 && trial < S->t0 + S->nt) return 0;
    return fail("trial %u is not one of this server's [%u, %u)", trial, S->t0, S->t0 + S->nt);
}

void pk_free(spiral_gpu_pack_server* S) {
    DbImage::drop(S->img, S);
    for (DevBuf* b : {&S->arena, &S->stage, &S->item, &S->wire_batch}) b->release();  // (what owns memory: every other buffer is a piece of the arena)
    S->item_cap = 0;
    S->wire_in.release();
    S->xwork.release();
    for (auto& e : S->ev)
        if (e) (void)hipEventDestroy(e), e = nullptr;
    if (S->ev_lane) (void)hipEventDestroy(S->ev_lane), S->ev_lane = nullptr;
    if (S->stream && S->own_stream) (void)hipStreamDestroy(S->stream);
    S->stream = nullptr;
}

// Every device buffer of a SpiralPack server but the lazy ones, stated once, in the order it is carved from one allocation.  Two parts: the client's own
// buffers (client: the members of S), then the per-answer buffers B for g instances, each g x its one-instance words -- the server's own with g = 1
// (pk_alloc), the arena of an item group with g = G and no client part (pk_item_group, pk_answer_items).
void pk_layout(spiral_gpu_pack_server* S, Arena& a, bool client, uint32_t g, PkBufs& B) {
    const spiral_gpu_params& p = S->p;
    const spiral_gpu_pack_shape& s = S->s;
    const size_t ngs = (size_t)p.nu2 * s.ell, rows = S->out_n + 1, half = s.num_per / 2;
    if (client) {
        a.carve(S->w_left, (size_t)s.n_left * 2 * p.t_exp * kN);
        a.carve(S->w_right, (size_t)s.n_right * 2 * p.t_exp_right * kN);
        a.carve(S->v, (size_t)2 * 2 * p.t_conv * kN);
        a.carve(S->v_w, (size_t)S->out_n * rows * p.t_conv * kN);
        a.carve(S->query, (size_t)s.n_query_cts * 2 * kN);
        a.carve(S->cv, (size_t)S->n_cv * 2 * kN);
        if (!p.direct_upload) {
            a.carve(S->ex_raw, (size_t)S->n_cv * 2 * kN);
            a.carve(S->ex_g, expand_g_polys(s.g, p.t_exp, p.t_exp_right) * kN);
            a.carve(S->gs_raw, ngs * 2 * kN);
            a.carve(S->gs_chat, ngs * 2 * p.t_conv * kN);
            a.carve(S->gs_tmp, ngs * 2 * kN);
        }
        a.carve(S->gsw, (size_t)p.nu2 * 2 * 2 * s.ell * kN);
        a.carve(S->key, (size_t)p.nu2 * 2 * 4 * s.ell * kN);
        a.carve(S->qs1, (size_t)kN * s.dim0 * 2);  // 4 u32 per (z, j)
        a.carve(S->gath, (size_t)s.trials * 2 * kN);
    }
    B.acc_words = (size_t)S->nt * s.num_per * 2 * kN;
    B.slot_words = rows * S->out_n * kN;
    B.wire_words = (wire_bytes(&p, S->out_n) + 7) / 8;
    B.acc = a.take(g * B.acc_words);
    B.raw = a.take(g * B.acc_words);
    B.fold_d = a.take(g * ((size_t)S->nt * half * 4 * s.ell * kN));
    B.fold_c = a.take(g * ((size_t)S->nt * half * 2 * kN));
    B.fold_c2 = a.take(g * ((size_t)S->nt * half * 2 * kN));
    B.ginv = a.take(g * ((size_t)s.trials * p.t_conv * kN));
    B.ct2 = a.take(g * ((size_t)s.trials * kN));
    B.res = a.take(g * B.slot_words);
    B.pk_raw = a.take(g * B.slot_words);
    B.resp = a.take(g * B.slot_words);
    B.wire = a.take(g * B.wire_words);
}

int pk_alloc(spiral_gpu_pack_server* S, DbImage* owners) {
    S->img = owners ? owners->share() : DbImage::create(DbLayout::packed1(S->s.num_per, S->s.dim0, S->nt), S);  // (a lane sweeps its owner's images)
    if (!S->img) return -1;
    S->n_cv = S->p.direct_upload ? S->s.n_query_cts : (1u << S->s.g);
    if (alloc_carved(S->arena, S->pieces, [&](Arena& a) { pk_layout(S, a, true, 1, S->own); })) return -1;
    HIP_OK(hipMemset(S->cv.p, 0, S->cv.words * sizeof(uint64_t)));
    return 0;
}

// The two ways client input gets into a server, in any form (message.h); both return synchronised.  A null NTT-form buffer is refused with the previous
// message untouched; from the first write on nothing answers from half-written keys: have_pp is cleared, and set again on success.
int pk_take_pub_params(spiral_gpu_pack_server* S, Form form, const MessageIn& in, const char* what) {
    if (enter(S)) return -1;
    const MessageLayout m = pack_pub_params_layout(S->p, S->s, S->out_n);
    if (form == FORM_NTT && check_ntt_parts(m, in, what)) return -1;
    uint64_t* const dst[kMessageParts] = {S->w_left.p, S->w_right.p, S->v.p, S->v_w.p};
    S->have_pp = false;
    S->key_memo = KeyMemo{};
    if (ingest(form, IngestOn{S->stage, S->wire_in, S->tb, S->stream}, m, dst, in, what)) return -1;
    S->have_pp = true;
    return 0;
}
// the query into S->query, on S's own stream, before the first launch of the call that answers it (`query`: the NTT form's polynomials or the message)
int pk_take_query(spiral_gpu_pack_server* S, Form form, const void* query, size_t bytes, const char* what) {
    HIP_OK(hipSetDevice(S->device));
    const MessageLayout m = pack_query_layout(S->p, S->s, S->out_n);
    const MessageIn in = form == FORM_NTT ? MessageIn{{(const uint64_t*)query}, nullptr, 0} : MessageIn{{}, query, bytes};
    uint64_t* const dst[kMessageParts] = {S->query.p};
    return ingest(form, IngestOn{S->stage, S->wire_in, S->tb, S->stream}, m, dst, in, what);
}
// a message's bytes in the wire / seeded form for parameters SpiralPack accepts, else 0
size_t pack_message_bytes(const spiral_gpu_params* p, uint32_t out_n, MessageLayout (*layout)(const spiral_gpu_params&, const spiral_gpu_pack_shape&, uint32_t),
                          Form form) {
    spiral_gpu_pack_shape s;
    return !p || pack_shape_of(p, out_n, &s) ? 0 : message_bytes(layout(*p, s, out_n), form);
}

// pack (src/testing.cpp:198-241) on device buffers: raw cts at trial stride `ct_stride` polynomials
// n_inst > 1: an item group, n_inst instances' trials one after another in raw_cts, ginv, ct2 and result (answer_batch_instances)
// lanes (n_inst = 1): the clients of a batch, every pointer lane 0's
void run_pack(const DeviceTables& tb, const uint64_t* raw_cts, uint32_t ct_stride_cts, const uint64_t* v_w, uint64_t* ginv, uint64_t* ct2, uint64_t* result,
              uint32_t out_n, uint32_t t_conv, hipStream_t st, uint32_t n_inst = 1, const Lanes& lanes = Lanes{}) {
    const uint32_t trials = n_inst * out_n * out_n;
    launch_job(tb, pack_digits_job(LD_PDIGIT, raw_cts, ginv, trials, t_conv, {.pmode = PM_PACK, .pk_num_per = ct_stride_cts, .lanes = lanes}), st);
    launch_job(tb, raw_job(raw_cts, ct2, trials, ST_PK, IndexMap{1, 2 * ct_stride_cts, 1}, lanes), st);  // row 1 of each trial's folded ct
    launch_pack_mac(v_w, ginv, ct2, result, out_n, t_conv, st, n_inst, lanes);
}

// the first-dimension sweep of n queries (their records qs[b]) over every trial image of H into accs[b], on `st`: one pass on the matrix cores when
// the image is in limb-plane form, else one sweep1 launch (all trials) per query
int pk_sweep_into(const DbImage* H, const uint32_t* const* qs, uint64_t* const* accs, uint32_t n, hipStream_t st) {
    const DbLayout& s = H->lay;
    const size_t acc_stride = (size_t)s.num_per * 2 * kN;
    if (H->format == SPIRAL_GPU_DB_LIMBS) {
        const hipError_t e = launch_sweep1_mfma(H->db.p, qs, accs, n, s.num_per, s.dim0, s.trials, s.trial_words, acc_stride, st);
        return e == hipSuccess ? 0 : fail("the matrix-core sweep could not be launched: %s", hipGetErrorString(e));
    }
    for (uint32_t b = 0; b < n; b++) launch_sweep1(H->db.p, qs[b], accs[b], s.num_per, s.dim0, s.trials, s.trial_words, acc_stride, st);
    return 0;
}
// lane b's records of S's query lanes (S = lane 0)
void pk_lane_records(const spiral_gpu_pack_server* S, const Lanes& lanes, const uint32_t** qs) {
    for (uint32_t b = 0; b < lanes.n; b++) qs[b] = (const uint32_t*)(S->qs1.p + lanes.off[b]);
}
// piece 2 of an answer: ... over S's images, into each lane's own accumulators
int pk_sweep(spiral_gpu_pack_server* S, const Lanes& lanes, hipStream_t st) {
    const uint32_t* qs[kMaxLanes];
    uint64_t* acc[kMaxLanes];
    pk_lane_records(S, lanes, qs);
    for (uint32_t b = 0; b < lanes.n; b++) acc[b] = S->own.acc + lanes.off[b];
    return pk_sweep_into(S->img, qs, acc, lanes.n, st);
}

}  // namespace

extern "C" {

int spiral_gpu_pack_get_shape(const spiral_gpu_params* p, uint32_t out_n, spiral_gpu_pack_shape* out) {
    if (!p || !out) return fail("null argument");
    return pack_shape_of(p, out_n, out);
}

int spiral_gpu_pack_has_limb_form(const spiral_gpu_params* p, uint32_t out_n) {
    if (!p) return fail("null argument");
    spiral_gpu_pack_shape s;
    spiral_gpu_params q = *p;
    q.direct_upload = 1;  // the image's form does not depend on how the query arrives: no query-size rule here
    if (pack_shape_of(&q, out_n, &s)) return -1;
    return DbLayout::packed1(s.num_per, s.dim0, s.trials).limbs_ok() ? 1 : 0;  // (at 8 ciphertexts per slot: option pack_pair_blocks, as read now)
}

int spiral_gpu_pack(uint64_t* result, uint32_t out_n, uint32_t m_conv, const uint64_t* v_ct, const uint64_t* v_W) {
    DeviceTables tb;
    if (current_tables(&tb)) return -1;
    if (out_n < 1 || out_n > 16 || m_conv < 1 || m_conv > 56) return fail("bad pack dimensions");
    Scratch sc;
    const uint32_t trials = out_n * out_n, rows = out_n + 1;
    uint64_t* d_ct = sc.upload(v_ct, (size_t)trials * 2 * kN);
    uint64_t* d_w = upload_pk(sc, v_W, (size_t)out_n * rows * m_conv);
    uint64_t* d_g = sc.get((size_t)trials * m_conv * kN);
    uint64_t* d_c2 = sc.get((size_t)trials * kN);
    uint64_t* d_res = sc.get((size_t)rows * out_n * kN);
    if (!d_ct || !d_w || !d_g || !d_c2 || !d_res) return fail("device allocation/upload failed");
    run_pack(tb, d_ct, 1, d_w, d_g, d_c2, d_res, out_n, m_conv, 0);
    return download_pk(sc, d_res, identity_map(), result, (size_t)rows * out_n);
}

int spiral_gpu_fast_multiply_query_by_database_dim1(uint64_t* out, const uint64_t* db, const uint64_t* v_firstdim, size_t dim0, size_t num_per) {
    if (dim0 < 2 || (dim0 & 1) || num_per == 0) return fail("unsupported geometry");
    Scratch sc;
    const size_t words = (size_t)kN * dim0 * num_per;
    uint64_t* d_ref = sc.upload(db, words);
    uint64_t* d_db = sc.get(db1_device_words((uint32_t)num_per, (uint32_t)dim0));
    uint64_t* d_re = sc.upload(v_firstdim, (size_t)kN * dim0 * 2);
    uint64_t* d_qs = sc.get((size_t)kN * dim0 * 2);
    uint64_t* d_acc = sc.get(num_per * 2 * kN);
    if (!d_ref || !d_db || !d_re || !d_qs || !d_acc) return fail("device allocation/upload failed");
    launch_db1_relayout(d_ref, d_db, (uint32_t)num_per, (uint32_t)dim0, 0);
    launch_qs1_from_reoriented(d_re, (uint32_t*)d_qs, (uint32_t)dim0, 0);
    launch_sweep1(d_db, (const uint32_t*)d_qs, d_acc, (uint32_t)num_per, (uint32_t)dim0, 1, 0, 0, 0);
    return download_pk(sc, d_acc, identity_map(), out, num_per * 2);
}

// The same for n queries against `trials` images, the way a batch sweeps them: ONE matrix-core pass where the geometry has a limb-plane form (wide,
// NARROW or, with option pack_pair_blocks, PAIR), else one vector-ALU sweep per query.  The accumulators are followed by one trial's worth of guard
// words; everything is filled with a byte pattern first, and a guard word that changed fails the call: what a ragged group's surplus waves and the
// empty half of an odd last pair-block must not store would land there (trial index `trials` of the last query).
int spiral_gpu_fast_multiply_queries_by_database_dim1(uint64_t* outs, const uint64_t* dbs, const uint64_t* v_firstdims, size_t n, size_t trials, size_t dim0,
                                                      size_t num_per) {
    if (!outs || !dbs || !v_firstdims) return fail("null argument");
    if (n == 0 || n > kMaxLanes) return fail("1 to %u queries per pass, not %zu", kMaxLanes, n);
    if (trials == 0 || trials > (1u << 16)) return fail("1 to 65536 trials, not %zu", trials);
    if (dim0 < 2 || (dim0 & 1) || dim0 > (1u << 16)) return fail("unsupported first dimension %zu (even, 2 to 65536)", dim0);
    if (num_per == 0 || num_per > (1u << 16)) return fail("unsupported number of ciphertexts per slot %zu (1 to 65536)", num_per);
    const uint32_t np = (uint32_t)num_per, d0 = (uint32_t)dim0, nt = (uint32_t)trials;
    const DbLayout lay = DbLayout::packed1(np, d0, nt);
    const bool mfma = lay.limbs_ok();  // (8 ciphertexts per slot: option pack_pair_blocks)
    const size_t ref_words = (size_t)kN * dim0 * num_per, re_words = (size_t)kN * dim0 * 2, trial_acc = num_per * 2 * kN, query_acc = trials * trial_acc;
    constexpr int kFill = 0xA5;  // no accumulator word: both halves are above the moduli
    Scratch sc;
    uint64_t* d_ref = sc.upload(dbs, trials * ref_words);
    uint64_t* d_db = sc.get(trials * lay.trial_words);
    uint64_t* d_limbs = mfma ? sc.get(trials * lay.trial_words) : nullptr;
    uint64_t* d_re = sc.upload(v_firstdims, n * re_words);
    uint64_t* d_qs = sc.get(n * re_words);
    uint64_t* d_acc = sc.get(n * query_acc + trial_acc);
    if (!d_ref || !d_db || (mfma && !d_limbs) || !d_re || !d_qs || !d_acc) return fail("device allocation/upload failed");
    HIP_OK(hipMemsetAsync(d_acc, kFill, (n * query_acc + trial_acc) * sizeof(uint64_t), 0));
    for (uint32_t t = 0; t < nt; t++) {
        launch_db1_relayout(d_ref + t * ref_words, d_db + t * lay.trial_words, np, d0, 0);
        if (mfma) launch_db1_limb_planes(d_db + t * lay.trial_words, d_limbs + t * lay.trial_words, np, d0, 0, kN);
    }
    const uint32_t* qs[kMaxLanes];
    uint64_t* acc[kMaxLanes];
    for (size_t b = 0; b < n; b++) {
        qs[b] = (const uint32_t*)(d_qs + b * re_words);
        acc[b] = d_acc + b * query_acc;
        launch_qs1_from_reoriented(d_re + b * re_words, (uint32_t*)qs[b], d0, 0);
    }
    if (mfma) {
        const hipError_t e = launch_sweep1_mfma(d_limbs, qs, acc, (uint32_t)n, np, d0, nt, lay.trial_words, trial_acc, 0);
        if (e != hipSuccess) return fail("the matrix-core sweep could not be launched: %s", hipGetErrorString(e));
    } else {
        for (size_t b = 0; b < n; b++) launch_sweep1(d_db, qs[b], acc[b], np, d0, nt, lay.trial_words, trial_acc, 0);
    }
    HIP_OK(hipGetLastError());
    std::vector<uint64_t> guard(trial_acc);
    HIP_OK(hipMemcpy(guard.data(), d_acc + n * query_acc, trial_acc * sizeof(uint64_t), hipMemcpyDeviceToHost));
    uint64_t fill = 0;
    memset(&fill, kFill, sizeof(fill));
    for (size_t k = 0; k < trial_acc; k++)
        if (guard[k] != fill) return fail("the sweep wrote past the last trial (guard word %zu)", k);
    return download_pk(sc, d_acc, identity_map(), outs, n * trials * num_per * 2);
}

int spiral_gpu_pack_server_create(const spiral_gpu_params* p, uint32_t out_n, int device, spiral_gpu_pack_server** out) {
    return spiral_gpu_pack_server_create_sharded(p, out_n, device, 0, 0, out);
}

// The out_n^2 trials are independent up to the packing step (each has its own database image, sweep and folding), so N GPUs split
// them: a server created for trials [trial0, trial1) holds only those images; fold_trials leaves their folded ciphertexts in a
// caller-provided device buffer, one all-gather of out_n^2 x 2 polynomials collects them, pack_gathered finishes on the root.
static int pk_create(const spiral_gpu_params* p, uint32_t out_n, int device, uint32_t trial0, uint32_t trial1, DbImage* owners,
                     spiral_gpu_pack_server** out) {
    if (!p || !out) return fail("null argument");
    spiral_gpu_pack_shape s;
    if (pack_shape_of(p, out_n, &s)) return -1;
    if (trial0 == 0 && trial1 == 0) trial1 = s.trials;
    if (trial0 >= trial1 || trial1 > s.trials) return fail("bad trial range [%u, %u) of %u", trial0, trial1, s.trials);
    HIP_OK(hipSetDevice(device));
    auto* S = new spiral_gpu_pack_server();
    S->p = *p;
    S->s = s;
    S->out_n = out_n;
    S->t0 = trial0;
    S->nt = trial1 - trial0;
    S->device = device;
    if (tables_get(device, &S->tb) != 0) {
        delete S;
        return fail("twiddle table setup failed on device %d", device);
    }
    bool ok = hipStreamCreate(&S->stream) == hipSuccess && hipEventCreateWithFlags(&S->ev_lane, hipEventDisableTiming) == hipSuccess;
    for (auto& e : S->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    if (!ok || pk_alloc(S, owners)) {
        if (ok == false) fail("stream/event creation failed");
        pk_free(S);
        delete S;
        return -1;
    }
    *out = S;
    return 0;
}

int spiral_gpu_pack_server_create_sharded(const spiral_gpu_params* p, uint32_t out_n, int device, uint32_t trial0, uint32_t trial1,
                                          spiral_gpu_pack_server** out) {
    return pk_create(p, out_n, device, trial0, trial1, nullptr, out);
}

// a query lane of `owner`: the owner's parameters, out_n and device, its own public parameters, query and intermediates, and the owner's trial images
int spiral_gpu_pack_server_create_lane(spiral_gpu_pack_server* owner, spiral_gpu_pack_server** out) {
    if (!owner || !out) return fail("null argument");
    if (owner->img->owner != owner) return fail("the owner does not own its database image (it is a lane)");
    if (owner->nt != owner->s.trials) return fail("the owner holds trials [%u, %u) only: trial-sharded servers have no lanes", owner->t0, owner->t0 + owner->nt);
    if (!owner->img->loaded) return fail("the owner has no database loaded");
    return pk_create(&owner->p, owner->out_n, owner->device, 0, 0, owner->img, out);
}

// a lane of a server that holds the trials [t0, t0 + nt) only: as create_lane, with the owner's trial range (fold_trials_batch on every rank,
// pack_gathered_batch on the root).  Of an owner that holds every trial it is an ordinary lane.
int spiral_gpu_pack_server_create_shard_lane(spiral_gpu_pack_server* owner, spiral_gpu_pack_server** out) {
    if (!owner || !out) return fail("null argument");
    if (owner->img->owner != owner) return fail("the owner does not own its database image (it is a lane)");
    if (!owner->img->loaded) return fail("the owner has no database loaded");
    return pk_create(&owner->p, owner->out_n, owner->device, owner->t0, owner->t0 + owner->nt, owner->img, out);
}

void spiral_gpu_pack_server_destroy(spiral_gpu_pack_server* S) {
    if (!S) return;
    (void)hipSetDevice(S->device);
    (void)hipDeviceSynchronize();
    pk_free(S);  // (images its lanes still sweep live on until the last of them goes)
    delete S;
}

int spiral_gpu_pack_server_set_db_format(spiral_gpu_pack_server* S, int format) {
    if (!S) return fail("null server");
    if (format != SPIRAL_GPU_DB_PACKED && format != SPIRAL_GPU_DB_LIMBS) return fail("unknown database image format %d", format);
    if (pk_refuse_lane(S, nullptr)) return -1;
    if (!S->img->loaded) return fail("no database loaded");
    HIP_OK(hipSetDevice(S->device));
    return S->img->set_format((uint32_t)format, S->stream);
}
int spiral_gpu_pack_server_db_format(spiral_gpu_pack_server* S) { return S ? (int)S->img->format : -1; }
uint64_t spiral_gpu_pack_server_db_device_bytes(spiral_gpu_pack_server* S) { return S ? S->img->device_bytes() : 0; }

int spiral_gpu_pack_server_gen_db(spiral_gpu_pack_server* S, uint64_t seed) {
    if (!S) return fail("null server");
    if (pk_refuse_lane(S, "load")) return -1;
    HIP_OK(hipSetDevice(S->device));
    S->img->begin_rewrite();
    const uint64_t total = (uint64_t)S->s.dim0 * S->s.num_per, chunk = 1u << 18;
    for (uint32_t t = 0; t < S->nt; t++) {
        FwdJob encode = db_encode_job(LD_DBGEN1, ST_DB1, S->img->trial(t), S->p.p_db,
                                      {.num_per = S->s.num_per, .dim0_shard = S->s.dim0, .trial = S->t0 + t, .total_n = total});
        for (uint64_t done = 0; done < total; done += chunk) {
            db_encode_seeded(encode, seed, done, (uint32_t)std::min(chunk, total - done));
            launch_job(S->tb, encode, S->stream);
        }
    }
    HIP_OK(hipStreamSynchronize(S->stream));
    S->img->finish_load();
    return 0;
}

int spiral_gpu_pack_server_load_db(spiral_gpu_pack_server* S, uint32_t trial, const uint64_t* db) {
    if (!S || !db) return fail("null argument");
    if (pk_refuse_lane(S, "load")) return -1;
    HIP_OK(hipSetDevice(S->device));
    if (pk_check_trial(S, trial)) return -1;
    // one trial is rewritten: the others keep their words, so an image in limb-plane form goes back to the packed form first
    if (S->img->begin_partial(S->stream)) return -1;
    DevBuf st;
    const size_t ref_words = (size_t)kN * S->s.dim0 * S->s.num_per;
    if (st.alloc(ref_words)) return -1;
    hipError_t e = hipMemcpy(st.p, db, ref_words * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        S->img->dirty();
        launch_db1_relayout(st.p, S->img->trial(trial - S->t0), S->s.num_per, S->s.dim0, S->stream);
        e = hipStreamSynchronize(S->stream);
    }
    st.release();
    if (e != hipSuccess) return fail("database upload failed: %s", hipGetErrorString(e));
    S->img->finish_load();
    return 0;
}

// raw ingest of one trial's 1 x 1 plaintexts (src/testing.cpp:845-869 + convertDb :316-340 on the device)
int spiral_gpu_pack_server_load_db_items(spiral_gpu_pack_server* S, uint32_t trial, const void* items, uint32_t coeff_bits, uint64_t first_item,
                                         uint64_t n_items) {
    if (!S) return fail("null server");
    if (pk_refuse_lane(S, "load")) return -1;
    HIP_OK(hipSetDevice(S->device));
    if (pk_check_trial(S, trial)) return -1;
    // a partial load scatters packed words into the image: an image in limb-plane form goes back to the packed form first
    if (S->img->begin_partial(S->stream)) return -1;
    const uint64_t total = (uint64_t)S->s.dim0 * S->s.num_per;
    if (first_item > total || n_items > total - first_item) return fail("items outside the database");
    FwdJob encode = db_encode_job(LD_DBGEN1, ST_DB1, S->img->trial(trial - S->t0), S->p.p_db,
                                  {.num_per = S->s.num_per, .dim0_shard = S->s.dim0, .trial = trial, .total_n = total});
    if (ingest_items(items, coeff_bits, first_item, first_item, first_item + n_items, 1, S->p.p_db, S->stream,
                     [&](const uint8_t* d_items, uint32_t* d_err, uint64_t first, uint64_t n) {
                         S->img->dirty();
                         db_encode_staged(encode, d_items, coeff_bits, d_err, first, (uint32_t)n);
                         launch_job(S->tb, encode, S->stream);
                     }))
        return -1;
    S->img->finish_load();
    return 0;
}

// In place, in the trial image's current form, on the holder's stream (include/spiral_gpu.h; the base path's update_db_items with 1 x 1 plaintexts)
namespace {
// what the update calls need to keep a tracked image's fingerprint current (t null: not tracked): the polynomial of local trial q0 + m of item (j, ii),
// database item j num_per + ii, is polynomial t0 + q0 + m of that item
void pk_track_ctx(const spiral_gpu_pack_server* S, uint32_t q0, FpTrackCtx& c) {
    if (!S->img->trk.on) return;
    c.t = &S->img->trk;
    c.q0 = q0;
    c.poly0 = S->t0;
    const uint64_t np = S->s.num_per;
    c.db_index = [=](uint32_t j, uint32_t ii) { return j * np + ii; };
}
}  // namespace
int spiral_gpu_pack_server_update_db_items(spiral_gpu_pack_server* S, uint32_t trial, const void* items, uint32_t coeff_bits, const uint64_t* item_ids,
                                           uint64_t n) {
    if (!S) return fail("null server");
    if (pk_refuse_lane(S, "update")) return -1;
    if (!S->img->loaded) return fail("no database loaded");
    if (pk_check_trial(S, trial)) return -1;
    HIP_OK(hipSetDevice(S->device));
    const uint64_t np = S->s.num_per;
    if (check_update_ids(items, item_ids, n, (uint64_t)S->s.dim0 * np)) return -1;
    std::vector<UpdateItem> sel(n);
    for (uint64_t k = 0; k < n; k++) sel[k] = UpdateItem{k, (uint32_t)(item_ids[k] / np), (uint32_t)(item_ids[k] % np)};
    FpTrackCtx trk;
    pk_track_ctx(S, trial - S->t0, trk);
    return update_items(S->img->upd, S->tb, S->stream, items, coeff_bits, S->p.p_db, sel, S->img->update_target(trial - S->t0), trk.t ? &trk : nullptr);
}

// One trial's items back as plaintexts, in the load_db_items layout, from the trial image in its current form (include/spiral_gpu.h): the owner or a
// lane, on its own stream
int spiral_gpu_pack_server_read_db_items(spiral_gpu_pack_server* S, uint32_t trial, void* items, uint32_t coeff_bits, uint64_t first_item, uint64_t n_items) {
    if (enter(S)) return -1;
    if (!items) return fail("null argument");
    if (!S->img->loaded) return fail("no database loaded");
    if (pk_check_trial(S, trial)) return -1;
    const uint64_t total = (uint64_t)S->s.dim0 * S->s.num_per;
    if (first_item > total || n_items > total - first_item)
        return fail("items [%llu, +%llu) outside the database of %llu", (unsigned long long)first_item, (unsigned long long)n_items, (unsigned long long)total);
    if (check_export_width(coeff_bits, S->p.p_db)) return -1;
    return export_items(S->xwork, S->tb, S->stream, items, coeff_bits, S->p.p_db, S->img->export_source(trial - S->t0), first_item, n_items, 0, nullptr,
                        [&](uint64_t pos) { return first_item + pos; });
}
int spiral_gpu_pack_server_read_db_items_at(spiral_gpu_pack_server* S, uint32_t trial, void* items, uint32_t coeff_bits, const uint64_t* item_ids, uint64_t n) {
    if (enter(S)) return -1;
    if (!items || !item_ids) return fail("null argument");
    if (!S->img->loaded) return fail("no database loaded");
    if (pk_check_trial(S, trial)) return -1;
    const uint64_t np = S->s.num_per, total = (uint64_t)S->s.dim0 * np;
    for (uint64_t k = 0; k < n; k++)
        if (item_ids[k] >= total) return fail("item id %llu outside the database of %llu items", (unsigned long long)item_ids[k], (unsigned long long)total);
    if (check_export_width(coeff_bits, S->p.p_db)) return -1;
    std::vector<ExportItem> sel(n);
    for (uint64_t k = 0; k < n; k++) sel[k] = ExportItem{k, (uint32_t)(item_ids[k] / np), (uint32_t)(item_ids[k] % np)};
    return export_items(S->xwork, S->tb, S->stream, items, coeff_bits, S->p.p_db, S->img->export_source(trial - S->t0), 0, 0, 0, &sel,
                        [&](uint64_t pos) { return item_ids[pos]; });
}

// The content fingerprint of items over this server's trial images, each in its current form (include/spiral_gpu.h "Fingerprints"): polynomial q of an
// item is its plaintext in trial q, and a trial shard sums the q of its own range [t0, t0 + nt)
namespace {
static int pk_fingerprint_enter(spiral_gpu_pack_server* S, const uint64_t* key, const uint64_t* per_item, const uint64_t* combined) {
    if (enter(S)) return -1;
    if (!key) return fail("null argument");
    if (!per_item && !combined) return fail("per_item and combined are both null: nothing to compute");
    if (!S->img->loaded) return fail("no database loaded");
    return 0;
}
}  // namespace
int spiral_gpu_pack_server_fingerprint_items(spiral_gpu_pack_server* S, const uint64_t* key, uint64_t first_item, uint64_t n_items, uint64_t* per_item,
                                             uint64_t* combined) {
    if (pk_fingerprint_enter(S, key, per_item, combined)) return -1;
    const uint64_t total = (uint64_t)S->s.dim0 * S->s.num_per;
    if (first_item > total || n_items > total - first_item)
        return fail("items [%llu, +%llu) outside the database of %llu", (unsigned long long)first_item, (unsigned long long)n_items, (unsigned long long)total);
    FingerprintSel fs;
    fs.first_l = fs.idx0 = first_item;
    fs.n = n_items;
    return fingerprint_items(S->xwork, S->tb, S->stream, key, S->p.p_db, S->img->export_source(0), S->img->lay.trial_words, S->nt, S->t0, fs, n_items, per_item,
                             combined);
}
int spiral_gpu_pack_server_fingerprint_items_at(spiral_gpu_pack_server* S, const uint64_t* key, const uint64_t* item_ids, uint64_t n, uint64_t* per_item,
                                                uint64_t* combined) {
    if (pk_fingerprint_enter(S, key, per_item, combined)) return -1;
    if (!item_ids) return fail("null argument");
    if (n > 0xFFFFFFFFull) return fail("at most 2^32 - 1 items per fingerprint call");
    const uint64_t np = S->s.num_per, total = (uint64_t)S->s.dim0 * np;
    for (uint64_t k = 0; k < n; k++)
        if (item_ids[k] >= total) return fail("item id %llu outside the database of %llu items", (unsigned long long)item_ids[k], (unsigned long long)total);
    std::vector<ExportItem> sel(n);
    for (uint64_t k = 0; k < n; k++) sel[k] = ExportItem{k, (uint32_t)(item_ids[k] / np), (uint32_t)(item_ids[k] % np)};
    FingerprintSel fs;
    fs.sel = &sel;
    fs.ids = item_ids;
    return fingerprint_items(S->xwork, S->tb, S->stream, key, S->p.p_db, S->img->export_source(0), S->img->lay.trial_words, S->nt, S->t0, fs, n, per_item, combined);
}

// ---- tracked fingerprints (include/spiral_gpu.h "Fingerprints", Tracked; host_common.h): over this server's trial images, polynomial q = trial q --
namespace {
int pk_fingerprint_check_range(const spiral_gpu_pack_server* S, uint64_t first_item, uint64_t n_items) {
    const uint64_t total = (uint64_t)S->s.dim0 * S->s.num_per;
    if (first_item > total || n_items > total - first_item)
        return fail("items [%llu, +%llu) outside the database of %llu", (unsigned long long)first_item, (unsigned long long)n_items, (unsigned long long)total);
    return 0;
}
}  // namespace
int spiral_gpu_pack_server_fingerprint_track(spiral_gpu_pack_server* S, const uint64_t* key, const uint64_t* poly_sums) {
    if (enter(S)) return -1;
    if (!key) return fail("null argument");
    if (pk_refuse_lane(S, "track")) return -1;
    if (!S->img->loaded) return fail("no database loaded");
    const FpTrackGeom geom{(uint64_t)S->s.dim0 * S->s.num_per, 0, 1, S->nt, S->t0};
    return fingerprint_track(S->img->trk, S->xwork, S->tb, S->stream, key, S->p.p_db, S->img->export_source(0), S->img->lay.trial_words, geom, poly_sums);
}
int spiral_gpu_pack_server_fingerprint_untrack(spiral_gpu_pack_server* S) {
    if (enter(S)) return -1;
    if (pk_refuse_lane(S, "untrack")) return -1;
    HIP_OK(hipStreamSynchronize(S->stream));  // (an update's apply launch may still write the table)
    S->img->trk.release();
    return 0;
}
int spiral_gpu_pack_server_fingerprint_tracked(spiral_gpu_pack_server* S, uint64_t* key_out, uint64_t* combined, uint64_t* n_updates) {
    if (enter(S)) return -1;
    return fingerprint_tracked(S->img->trk, S->stream, key_out, combined, n_updates);
}
int spiral_gpu_pack_server_fingerprint_tracked_polys(spiral_gpu_pack_server* S, uint64_t first_item, uint64_t n_items, uint64_t* poly_sums) {
    if (enter(S)) return -1;
    if (pk_fingerprint_check_range(S, first_item, n_items)) return -1;
    return fingerprint_tracked_polys(S->img->trk, S->stream, first_item, n_items, 0, 1, n_items, poly_sums);
}
int spiral_gpu_pack_server_fingerprint_scrub(spiral_gpu_pack_server* S, uint64_t first_item, uint64_t n_items, uint64_t* n_bad, uint64_t* first_bad_item,
                                             uint32_t* first_bad_poly) {
    if (enter(S)) return -1;
    if (!n_bad) return fail("null argument");
    if (!S->img->loaded) return fail("no database loaded");
    if (pk_fingerprint_check_range(S, first_item, n_items)) return -1;
    FingerprintSel fs;
    fs.first_l = fs.idx0 = first_item;
    fs.n = n_items;
    return fingerprint_scrub(S->img->trk, S->xwork, S->tb, S->stream, S->p.p_db, S->img->export_source(0), S->img->lay.trial_words, S->t0, fs, n_bad, first_bad_item,
                             first_bad_poly);
}

// ---- records (include/spiral_gpu.h "Records", SpiralPack; records_host.h, records.hip) -----------------------------------------------------------
namespace {
// the layout, this instance's chunk and the trial images of a record call
struct PkRecordCall {
    spiral_gpu_record_layout l;
    RecordChunk chunk;
    RecordTrials tr;
};
int pk_record_call(const spiral_gpu_pack_server* S, uint64_t record_bytes, uint32_t instance, PkRecordCall* rc) {
    if (record_layout(&S->p, record_bytes, &rc->l, S->out_n)) return -1;
    rc->tr = RecordTrials{S->s.trials, S->t0, S->nt, S->img->lay.trial_words};
    return record_chunk(rc->l, record_bytes, instance, &rc->chunk);
}
// record r of the call as a piece of its item's stream (every server holds every item; which polynomials it holds, the tables decide)
RecordPiece pk_record_piece(const spiral_gpu_pack_server* S, const PkRecordCall& rc, uint64_t pos, uint64_t r) {
    const uint64_t item = r / rc.l.per_item;
    return RecordPiece{pos, (uint32_t)(item / S->s.num_per), (uint32_t)(item % S->s.num_per),
                       (uint32_t)((r % rc.l.per_item) * (rc.l.instances == 1 ? rc.chunk.len : 0)), (uint32_t)rc.chunk.len};
}
}  // namespace

int spiral_gpu_pack_record_layout_of(const spiral_gpu_params* p, uint32_t out_n, uint64_t record_bytes, spiral_gpu_record_layout* out) {
    if (p && out && out_n < 1) return fail("out_n out of range");
    return record_layout(p, record_bytes, out, out_n);
}

// Through load_db_items, one call per trial this server holds: the records repacked into items on the host, padding zero (not a hot path)
int spiral_gpu_pack_server_load_records(spiral_gpu_pack_server* S, const void* records, uint64_t record_bytes, uint32_t instance, uint64_t first_record,
                                        uint64_t n_records) {
    if (!S) return fail("null server");
    PkRecordCall rc;
    if (pk_record_call(S, record_bytes, instance, &rc)) return -1;
    if (pk_refuse_lane(S, "load")) return -1;
    if (first_record > rc.l.capacity || n_records > rc.l.capacity - first_record)
        return fail("records [%llu, +%llu) outside the database of %llu", (unsigned long long)first_record, (unsigned long long)n_records, (unsigned long long)rc.l.capacity);
    if (first_record % rc.l.per_item || n_records % rc.l.per_item)
        return fail("records [%llu, +%llu) do not start and end at a multiple of the %llu records of an item", (unsigned long long)first_record,
                    (unsigned long long)n_records, (unsigned long long)rc.l.per_item);
    if (n_records && !records) return fail("null argument");
    const uint32_t w = rc.l.coeff_bits, cb = (1ull << w) < S->p.p_db ? w + 1 : w;  // (load_db_items wants a width that holds every value below p_db)
    const uint64_t first_item = first_record / rc.l.per_item, n_items = n_records / rc.l.per_item, poly_bytes = 256ull * w;
    const uint64_t used = rc.l.instances == 1 ? rc.l.per_item * record_bytes : rc.chunk.len;  // bytes of an item's stream that records fill
    const uint8_t* src = static_cast<const uint8_t*>(records);
    const uint64_t pass = std::max<uint64_t>(1, std::min<uint64_t>(options().db_stage_bytes / (256ull * cb), 1u << 14));  // polynomials repacked at a time
    std::vector<uint8_t> stream, wide;
    for (uint32_t t = S->t0; t < S->t0 + S->nt; t++)
        for (uint64_t done = 0; done < n_items; done += pass) {
            const uint64_t cnt = std::min(pass, n_items - done);
            stream.assign((size_t)(cnt * poly_bytes), 0);
            const uint64_t lo = t * poly_bytes, hi = std::min(lo + poly_bytes, used);  // the bytes of an item's stream that are trial t's record bytes
            for (uint64_t i = 0; i < cnt && lo < hi; i++) {
                const uint64_t r0 = (done + i) * rc.l.per_item;  // (relative to first_record)
                memcpy(stream.data() + i * poly_bytes, src + r0 * record_bytes + (rc.l.instances == 1 ? 0 : rc.chunk.first) + lo, (size_t)(hi - lo));
            }
            const uint8_t* items = stream.data();
            if (cb != w) {
                wide.assign((size_t)(cnt * 256ull * cb), 0);
                widen_coeffs(stream.data(), wide.data(), (size_t)(cnt * kN), w, cb);
                items = wide.data();
            }
            if (spiral_gpu_pack_server_load_db_items(S, t, items, cb, first_item + done, cnt)) return -1;
        }
    return 0;
}

// In place, in each trial image's current form, on the holder's stream: ONE upload, ONE read-modify-write launch and ONE scatter launch over every trial
// the records touch
int spiral_gpu_pack_server_update_records(spiral_gpu_pack_server* S, const void* records, uint64_t record_bytes, uint32_t instance, const uint64_t* record_ids,
                                          uint64_t n) {
    if (!S) return fail("null server");
    if (pk_refuse_lane(S, "update")) return -1;
    PkRecordCall rc;
    if (pk_record_call(S, record_bytes, instance, &rc)) return -1;
    if (!S->img->loaded) return fail("no database loaded");
    HIP_OK(hipSetDevice(S->device));
    if (n == 0) return 0;
    if (!records || !record_ids) return fail("null argument");
    if (n > (1ull << 24)) return fail("at most 2^24 records per update");
    {
        std::vector<uint64_t> sorted(record_ids, record_ids + n);
        std::sort(sorted.begin(), sorted.end());
        if (sorted.back() >= rc.l.capacity)
            return fail("record id %llu outside the database of %llu records", (unsigned long long)sorted.back(), (unsigned long long)rc.l.capacity);
        for (uint64_t k = 1; k < n; k++)
            if (sorted[k] == sorted[k - 1]) return fail("record id %llu given twice", (unsigned long long)sorted[k]);
    }
    std::vector<RecordPiece> pieces(n);
    for (uint64_t k = 0; k < n; k++) pieces[k] = pk_record_piece(S, rc, k, record_ids[k]);
    FpTrackCtx trk;
    pk_track_ctx(S, 0, trk);
    return update_record_pieces(S->img->upd, S->tb, S->stream, static_cast<const uint8_t*>(records), record_bytes, rc.chunk, rc.l.coeff_bits, S->p.p_db, pieces,
                                S->img->update_target(0), S->img->export_source(0), [&](uint64_t pos) { return record_ids[pos]; }, rc.tr, trk.t ? &trk : nullptr);
}

// The records back, from the trial images in their current form: the owner or a lane, on its own stream; a trial shard writes the bytes that lie in its
// trials' polynomials and leaves the other bytes of `records` alone
int spiral_gpu_pack_server_read_records(spiral_gpu_pack_server* S, void* records, uint64_t record_bytes, uint32_t instance, uint64_t first_record,
                                        uint64_t n_records) {
    if (enter(S)) return -1;
    PkRecordCall rc;
    if (pk_record_call(S, record_bytes, instance, &rc)) return -1;
    if (!records) return fail("null argument");
    if (!S->img->loaded) return fail("no database loaded");
    if (first_record > rc.l.capacity || n_records > rc.l.capacity - first_record)
        return fail("records [%llu, +%llu) outside the database of %llu", (unsigned long long)first_record, (unsigned long long)n_records, (unsigned long long)rc.l.capacity);
    return read_record_pieces(S->xwork, S->tb, S->stream, static_cast<uint8_t*>(records), record_bytes, rc.chunk, rc.l.coeff_bits, S->p.p_db, n_records,
                              [&](uint64_t k, RecordPiece* pc) { return *pc = pk_record_piece(S, rc, k, first_record + k), true; }, S->img->export_source(0),
                              [&](uint64_t pos) { return first_record + pos; }, rc.tr);
}
int spiral_gpu_pack_server_read_records_at(spiral_gpu_pack_server* S, void* records, uint64_t record_bytes, uint32_t instance, const uint64_t* record_ids,
                                           uint64_t n) {
    if (enter(S)) return -1;
    PkRecordCall rc;
    if (pk_record_call(S, record_bytes, instance, &rc)) return -1;
    if (n && (!records || !record_ids)) return fail("null argument");
    if (!S->img->loaded) return fail("no database loaded");
    for (uint64_t k = 0; k < n; k++)
        if (record_ids[k] >= rc.l.capacity)
            return fail("record id %llu outside the database of %llu records", (unsigned long long)record_ids[k], (unsigned long long)rc.l.capacity);
    return read_record_pieces(S->xwork, S->tb, S->stream, static_cast<uint8_t*>(records), record_bytes, rc.chunk, rc.l.coeff_bits, S->p.p_db, n,
                              [&](uint64_t k, RecordPiece* pc) { return *pc = pk_record_piece(S, rc, k, record_ids[k]), true; }, S->img->export_source(0),
                              [&](uint64_t pos) { return record_ids[pos]; }, rc.tr);
}

// ---- keyed records (include/spiral_gpu.h "Keyed records", SpiralPack; kv_host.h, kv.hip) ----------------------------------------------------------
namespace {
// how every keyed call opens: the layout, and a server that holds every trial image (a value's bytes span trials; the header is in trial 0)
int pk_kv_call(const spiral_gpu_pack_server* S, const char* what, uint64_t value_bytes, spiral_gpu_kv_layout* l) {
    if (kv_layout(&S->p, value_bytes, l, S->out_n)) return -1;
    if (S->nt != S->s.trials)
        return fail("%s: this server is a trial shard (trials [%u, %u) of %u): keyed records need every trial image in one place (a bucket's header is in "
                    "trial 0, its values span the trials)",
                    what, S->t0, S->t0 + S->nt, S->s.trials);
    return 0;
}
// the trial images as the shared keyed bodies take them (kv_host.h KvImage): src and dst name trial 0; trk: the caller's, filled by pk_track_ctx
extern "C++" KvImage pk_kv_image(spiral_gpu_pack_server* S, const FpTrackCtx& trk) {
    return KvImage{S->xwork, S->img->upd, S->tb, S->stream, S->img->export_source(0), S->img->update_target(0), RecordTrials{S->s.trials, S->t0, S->nt, S->img->lay.trial_words},
                   trk.t ? &trk : nullptr, S->s.num_per, S->p.p_db};
}
// put, and delete: the owner's checks, then kv_host.h kv_write
int pk_kv_write(spiral_gpu_pack_server* S, const char* what, bool put, const void* table_key16, const void* keys, uint64_t key_bytes, const void* values,
                uint64_t value_bytes, uint64_t n, uint64_t* n_deleted) {
    if (!S) return fail("null server");
    if (S->img->owner != S) return fail("%s: this server is a lane: it sweeps its owner's database, update it through the owner", what);
    spiral_gpu_kv_layout l;
    if (pk_kv_call(S, what, value_bytes, &l)) return -1;
    if (!S->img->loaded) return fail("no database loaded");
    HIP_OK(hipSetDevice(S->device));
    FpTrackCtx trk;
    pk_track_ctx(S, 0, trk);
    return kv_write(pk_kv_image(S, trk), what, put, l, table_key16, keys, key_bytes, values, n, n_deleted);
}
}  // namespace

int spiral_gpu_pack_kv_layout_of(const spiral_gpu_params* p, uint32_t out_n, uint64_t value_bytes, spiral_gpu_kv_layout* out) {
    if (p && out && out_n < 1) return fail("out_n out of range");
    return kv_layout(p, value_bytes, out, out_n);
}

int spiral_gpu_pack_kv_hash(const spiral_gpu_params* p, uint32_t out_n, const void* table_key16, const void* key, uint64_t key_bytes, uint64_t* tag, uint64_t* b1,
                            uint64_t* b2) {
    if (!p || !table_key16 || !tag || !b1 || !b2 || (key_bytes && !key)) return fail("kv_hash: null argument");
    if (out_n < 1) return fail("out_n out of range");
    uint64_t nb;
    if (kv_buckets(p, out_n, &nb)) return -1;
    static const uint8_t none = 0;
    const KvKey h = kv_hash(nb, static_cast<const uint8_t*>(table_key16), key_bytes ? static_cast<const uint8_t*>(key) : &none, key_bytes);
    *tag = h.tag;
    *b1 = h.b[0];
    *b2 = h.b[1];
    return 0;
}

// A fresh table: placement from empty on the host, then the item stream built a pass of buckets at a time and every trial image loaded through
// load_db_items' ingest, polynomial t of each bucket to trial t (not a hot path)
int spiral_gpu_pack_server_kv_load(spiral_gpu_pack_server* S, const void* table_key16, const void* keys, uint64_t key_bytes, const void* values, uint64_t value_bytes,
                                   uint64_t n) {
    if (!S) return fail("null server");
    if (S->img->owner != S) return fail("kv_load: this server is a lane: it sweeps its owner's database, load it through the owner");
    spiral_gpu_kv_layout l;
    if (pk_kv_call(S, "kv_load", value_bytes, &l)) return -1;
    if (n && !values) return fail("kv_load: null argument");
    std::vector<KvKey> hk;
    if (kv_hash_keys("kv_load", l.buckets, table_key16, keys, key_bytes, n, true, hk)) return -1;
    KvTable table;
    table.slots = l.slots;
    table.ids.resize((size_t)l.buckets);
    for (uint64_t b = 0; b < l.buckets; b++) table.ids[b] = b;
    table.occ.assign((size_t)l.buckets, std::array<uint64_t, 4>{});
    // placement first: a key that cannot be placed fails the call before the stream is built.  where[k] = bucket << 8 | slot
    std::vector<std::pair<uint64_t, uint64_t>> where((size_t)n);  // (bucket << 8 | slot, key), sorted by bucket below
    for (uint64_t k = 0; k < n; k++) {
        uint32_t cand, slot;
        if (!table.place(hk[k], &cand, &slot))
            return fail("kv_load: key %llu cannot be placed: its buckets %llu and %llu are both full (%u slots each); the image was not touched", (unsigned long long)k,
                        (unsigned long long)hk[k].b[0], (unsigned long long)hk[k].b[1], l.slots);
        where[k] = {(hk[k].b[cand] << 8) | slot, k};
    }
    std::sort(where.begin(), where.end());
    // the item stream a pass of buckets at a time (at most 2^14 buckets: 512 MiB at 32 KiB buckets, not the whole table), polynomial t of each to trial t
    const uint32_t w = l.coeff_bits, cb = (1ull << w) < S->p.p_db ? w + 1 : w;  // (load_db_items wants a width that holds every value below p_db)
    const uint64_t poly_bytes = 256ull * w;
    const uint64_t pass = std::max<uint64_t>(1, std::min<uint64_t>(options().db_stage_bytes / (256ull * cb), 1u << 14));  // buckets built and repacked at a time
    std::vector<uint8_t> stream, polys, wide;
    size_t next = 0;
    for (uint64_t done = 0; done < l.buckets; done += pass) {
        const uint64_t cnt = std::min(pass, l.buckets - done);
        stream.assign((size_t)(cnt * l.item_bytes), 0);
        for (; next < where.size() && (where[next].first >> 8) < done + cnt; next++) {
            const uint64_t k = where[next].second, slot = where[next].first & 0xFFu;
            uint8_t* item = stream.data() + ((where[next].first >> 8) - done) * l.item_bytes;
            for (int b = 0; b < 8; b++) item[8u * slot + b] = (uint8_t)(hk[k].tag >> (8 * b));
            memcpy(item + 8u * l.slots + slot * value_bytes, static_cast<const uint8_t*>(values) + k * value_bytes, (size_t)value_bytes);
        }
        for (uint32_t t = 0; t < S->s.trials; t++) {
            polys.resize((size_t)(cnt * poly_bytes));
            for (uint64_t i = 0; i < cnt; i++) memcpy(polys.data() + i * poly_bytes, stream.data() + i * l.item_bytes + t * poly_bytes, (size_t)poly_bytes);
            const uint8_t* items = polys.data();
            if (cb != w) {
                wide.assign((size_t)(cnt * 256ull * cb), 0);
                widen_coeffs(polys.data(), wide.data(), (size_t)(cnt * kN), w, cb);
                items = wide.data();
            }
            if (spiral_gpu_pack_server_load_db_items(S, t, items, cb, done, cnt)) return -1;
        }
    }
    return 0;
}

int spiral_gpu_pack_server_kv_put(spiral_gpu_pack_server* S, const void* table_key16, const void* keys, uint64_t key_bytes, const void* values, uint64_t value_bytes,
                                  uint64_t n) {
    if (n && !values) return fail("kv_put: null argument");
    return pk_kv_write(S, "kv_put", true, table_key16, keys, key_bytes, values, value_bytes, n, nullptr);
}

int spiral_gpu_pack_server_kv_delete(spiral_gpu_pack_server* S, const void* table_key16, const void* keys, uint64_t key_bytes, uint64_t value_bytes, uint64_t n,
                                     uint64_t* n_deleted) {
    return pk_kv_write(S, "kv_delete", false, table_key16, keys, key_bytes, nullptr, value_bytes, n, n_deleted);
}

// The probe, then the found slots' values through read_records' path; the owner or a lane, on its own stream
int spiral_gpu_pack_server_kv_get(spiral_gpu_pack_server* S, const void* table_key16, const void* keys, uint64_t key_bytes, void* values, uint64_t value_bytes, uint64_t n,
                                  uint8_t* found) {
    if (enter(S)) return -1;
    spiral_gpu_kv_layout l;
    if (pk_kv_call(S, "kv_get", value_bytes, &l)) return -1;
    if (n && (!values || !found)) return fail("kv_get: null argument");
    if (!S->img->loaded) return fail("no database loaded");
    FpTrackCtx none;
    return kv_get(pk_kv_image(S, none), l, table_key16, keys, key_bytes, values, n, found);
}

// Table occupancy: one launch over the range's buckets in trial image 0, 257 words back (kv_host.h kv_stats); the owner or a lane, on its own stream
int spiral_gpu_pack_server_kv_stats(spiral_gpu_pack_server* S, uint64_t value_bytes, uint64_t first_bucket, uint64_t n_buckets, spiral_gpu_kv_stats* out) {
    if (enter(S)) return -1;
    if (!out) return fail("kv_stats: null argument");
    spiral_gpu_kv_layout l;
    if (pk_kv_call(S, "kv_stats", value_bytes, &l)) return -1;
    if (!S->img->loaded) return fail("no database loaded");
    return kv_stats(S->xwork, S->tb, S->stream, S->img->export_source(0), l, S->p.p_db, first_bucket, n_buckets, out);
}

// Listing: the headers from trial image 0, the entries' values across the trials through read_records' path (kv_host.h kv_scan); the owner or a lane,
// on its own stream
namespace {
int pk_kv_scan_call(spiral_gpu_pack_server* S, const char* what, uint64_t value_bytes, uint64_t first_bucket, const uint64_t* buckets, uint64_t n_buckets,
                    spiral_gpu_kv_entry* entries, void* values, uint64_t max_entries, uint64_t* n_entries) {
    if (enter(S)) return -1;
    if (!n_entries) return fail("%s: null argument", what);
    spiral_gpu_kv_layout l;
    if (pk_kv_call(S, what, value_bytes, &l)) return -1;
    if (!S->img->loaded) return fail("no database loaded");
    FpTrackCtx none;
    return kv_scan(pk_kv_image(S, none), what, l, first_bucket, buckets, n_buckets, entries, values, max_entries, n_entries);
}
}  // namespace
int spiral_gpu_pack_server_kv_scan(spiral_gpu_pack_server* S, uint64_t value_bytes, uint64_t first_bucket, uint64_t n_buckets, spiral_gpu_kv_entry* entries, void* values,
                                   uint64_t max_entries, uint64_t* n_entries) {
    return pk_kv_scan_call(S, "kv_scan", value_bytes, first_bucket, nullptr, n_buckets, entries, values, max_entries, n_entries);
}
int spiral_gpu_pack_server_kv_scan_at(spiral_gpu_pack_server* S, uint64_t value_bytes, const uint64_t* buckets, uint64_t n_buckets, spiral_gpu_kv_entry* entries,
                                      void* values, uint64_t max_entries, uint64_t* n_entries) {
    static const uint64_t none = 0;  // (an empty list may be NULL)
    if (n_buckets && !buckets) return fail("kv_scan_at: null argument");
    return pk_kv_scan_call(S, "kv_scan_at", value_bytes, 0, buckets ? buckets : &none, n_buckets, entries, values, max_entries, n_entries);
}

int spiral_gpu_pack_server_fill_db_random(spiral_gpu_pack_server* S, uint64_t seed) {
    if (!S) return fail("null server");
    if (pk_refuse_lane(S, "load")) return -1;
    HIP_OK(hipSetDevice(S->device));
    S->img->begin_rewrite();
    for (uint32_t t = 0; t < S->nt; t++) launch_fill_db1_random(S->img->trial(t), S->s.num_per, S->s.dim0, seed + S->t0 + t, S->stream);
    HIP_OK(hipStreamSynchronize(S->stream));
    S->img->finish_load();
    return 0;
}

// the public parameters in their three forms (include/spiral_gpu.h): W_exp_left, W_exp_right, V (expansion only), v_W
int spiral_gpu_pack_server_set_pub_params(spiral_gpu_pack_server* S, const uint64_t* w_left, const uint64_t* w_right, const uint64_t* v,
                                          const uint64_t* v_w) {
    return pk_take_pub_params(S, FORM_NTT, MessageIn{{w_left, w_right, v, v_w}, nullptr, 0}, "set_pub_params");
}
int spiral_gpu_pack_server_set_pub_params_wire(spiral_gpu_pack_server* S, const void* wire, size_t bytes) {
    return pk_take_pub_params(S, FORM_WIRE, MessageIn{{}, wire, bytes}, "set_pub_params_wire");
}
int spiral_gpu_pack_server_set_pub_params_seeded(spiral_gpu_pack_server* S, const void* msg, size_t bytes) {
    return pk_take_pub_params(S, FORM_SEEDED, MessageIn{{}, msg, bytes}, "set_pub_params_seeded");
}

size_t spiral_gpu_pack_query_wire_bytes(const spiral_gpu_params* p, uint32_t out_n) { return pack_message_bytes(p, out_n, pack_query_layout, FORM_WIRE); }
size_t spiral_gpu_pack_query_seeded_bytes(const spiral_gpu_params* p, uint32_t out_n) { return pack_message_bytes(p, out_n, pack_query_layout, FORM_SEEDED); }
size_t spiral_gpu_pack_pub_params_wire_bytes(const spiral_gpu_params* p, uint32_t out_n) {
    return pack_message_bytes(p, out_n, pack_pub_params_layout, FORM_WIRE);
}
size_t spiral_gpu_pack_pub_params_seeded_bytes(const spiral_gpu_params* p, uint32_t out_n) {
    return pack_message_bytes(p, out_n, pack_pub_params_layout, FORM_SEEDED);
}

// The answer up to and including the folding, for this server's trials, in three pieces (pk_front; answer_batch puts one shared sweep between the
// lanes' first and last pieces): the folded ciphertexts end up at the head of each trial's num_per slots of S->raw (events 0..5 bracket the stages).
// Every piece takes the query lanes of its launches (kernels.h Lanes): S is lane 0, whose buffers the launches name and whose events bracket the stages,
// and lane b works in its own arena lanes.off[b] words further on.  Lanes{} is one client: the launches of a single answer, nothing else.
// Piece 1: expansion and conversion of the query in S->query (pk_take_query) -> the sweep's records qs1 and the folding keys, on `st`
static int pk_expand_convert(spiral_gpu_pack_server* S, const Lanes& lanes, hipStream_t st) {
    const spiral_gpu_params& p = S->p;
    const spiral_gpu_pack_shape& s = S->s;
    const uint32_t ell = s.ell, ngs = p.nu2 * ell;
    HIP_OK(hipEventRecord(S->ev[0], st));
    S->events_elsewhere = false;
    // ---- coefficientExpansion + reorientCiphertextsDim1 (src/testing.cpp:1009-1020)
    if (!p.direct_upload) {
        ExpandWork wk{S->ex_raw.p, S->ex_g.p};
        run_expand(S->tb, S->cv.p, s.g, p.t_exp, S->w_left.p, p.t_exp_right, S->w_right.p, ell * p.nu2, s.stopround, wk, st,
                   s.g ? S->query.p : nullptr, 0, 0xffffffffu, ExpandShard{}, 3, lanes);
        if (s.g == 0)
            for (uint32_t b = 0; b < lanes.n; b++)
                HIP_OK(hipMemcpyAsync(S->cv.p + lanes.off[b], S->query.p + lanes.off[b], 2 * kPolyBytes, hipMemcpyDeviceToDevice, st));
        launch_qs1_from_cv(S->cv.p, (uint32_t*)S->qs1.p, s.dim0, 2, st, lanes);
    } else {
        launch_qs1_from_cv(S->query.p, (uint32_t*)S->qs1.p, s.dim0, 1, st, lanes);
    }
    HIP_OK(hipEventRecord(S->ev[1], st));
    // ---- regevToSimpleGsw + the negated GSW ciphertexts (:1022-1033)
    if (!p.direct_upload) {
        launch_job(S->tb, lift_job(S->cv.p, S->gs_raw.p, 2 * ngs, {.src_map = IndexMap{2, 4, 2}, .lanes = lanes}), st);  // both rows of ct 2*ij + 1
        launch_job(S->tb, pack_digits_job(LD_PDIGIT, S->gs_raw.p, S->gs_chat.p, 2 * ngs, p.t_conv, {.pmode = PM_GSW, .lanes = lanes}), st);
        MatmulParams mp{{S->v.p, S->gs_chat.p, S->gs_tmp.p, 2, 2 * p.t_conv, 1, 0, 2 * p.t_conv, 2}, lanes};
        launch_matmul(mp, ngs, st);
        launch_pack_gsw_assemble(S->gs_tmp.p, S->cv.p, S->gsw.p, ell, p.nu2, st, lanes);
    } else {
        launch_pack_gsw_from_upload(S->query.p, S->gsw.p, s.dim0, ell, p.nu2, st, lanes);
    }
    launch_pack_fold_key(S->gsw.p, S->key.p, ell, p.nu2, st, lanes);
    HIP_OK(hipEventRecord(S->ev[2], st));
    S->have_records = true;
    return 0;
}

// piece 3 (piece 2 is pk_sweep: the first dimension for every trial, :1049-1051): one INTT + CRT lift (:1055-1057) and the folding, on `st`, of nt
// trials in the buffers B (pk_fold: S's own trials in its own buffers).  With lanes B must be S's own: a piece of the arena the offsets are taken from.
static int pk_fold_into(spiral_gpu_pack_server* S, const PkBufs& B, uint32_t nt, const Lanes& lanes, hipStream_t st) {
    const spiral_gpu_params& p = S->p;
    const spiral_gpu_pack_shape& s = S->s;
    const uint32_t ell = s.ell;
    HIP_OK(hipEventRecord(S->ev[3], st));
    HIP_OK(hipEventRecord(S->ev[4], st));  // (the lift is chained into the first fold round's digit transforms)
    // ---- foldCiphertextsDim1 (:596-624), all trials batched: each round = fold_chain_kernel (lift of the previous
    // product or of the accumulators + unsigned digits + forward transforms) and one product; a last lift to raw
    uint32_t np = s.num_per;
    const uint64_t* src = B.acc;
    uint32_t src_stride = s.num_per;
    // Pair form (option fold_pair = 0 keeps the reference's two products): folding_neg = gadget - F (:1027-1032), so
    // F_neg G^-1(L) + F G^-1(H) = L + F (G^-1(H) - G^-1(L)) -- the unsigned digits always recompose their value -- i.e. per round one lift
    // of the 2 np ciphertexts, ell digit-difference transforms per polynomial pair (LD_PDIFF) and a product of K = 2 ell terms + L.
    const bool pair = options().fold_pair != 0;  // (read per call: tests switch it inside one process)
    uint64_t* out = B.fold_c;
    for (uint32_t cur = 0; cur < p.nu2; cur++) {
        np /= 2;
        if (src == out) out = out == B.fold_c ? B.fold_c2 : B.fold_c;
        if (pair) {
            // B.raw: [t][2 np][2], compact
            launch_job(S->tb, lift_job(src, B.raw, nt * 4 * np, {.src_map = IndexMap{4 * np, 2 * src_stride, 0}, .lanes = lanes}), st);
            // pack_fold_mac sums 2 ell products and the addend per accumulator
            launch_job(S->tb, pack_digits_job(LD_PDIFF, B.raw, B.fold_d, nt * np * 2, ell, {.np = np, .mac_terms = 2 * ell + 1, .lanes = lanes}), st);
            launch_pack_fold_mac(S->key.p + ((size_t)cur * 2 * 4 * ell + 2 * ell) * kN, B.fold_d, out, 2 * ell, nt * np, st, 4 * ell, src, np, src_stride, lanes);
            src = out;
            src_stride = np;
            continue;
        }
        FoldChainParams cp{};
        cp.src = src;
        cp.dst = B.fold_d;
        cp.ell = ell;
        cp.bits = get_bits_per(ell);
        cp.fold_np = np;
        cp.pack = 1;
        cp.src_stride = src_stride;
        const uint32_t n_src = nt * 2 * np * 2;
        uint32_t dpb = ell;
        while (dpb > 1 && n_src * lanes.n * ((ell + dpb - 1) / dpb) < 768u) dpb = (dpb + 1) / 2;  // (the workgroups of all lanes)
        cp.dpb = dpb;
        cp.lanes = lanes;
        launch_fold_chain(S->tb, cp, n_src, st);
        launch_pack_fold_mac(S->key.p + (size_t)cur * 2 * 4 * ell * kN, B.fold_d, out, 4 * ell, nt * np, st, 0, nullptr, 1, 1, lanes);
        src = out;
        src_stride = np;
    }
    // the trial's surviving np cts to the head of its num_per slots
    launch_job(S->tb, lift_job(src, B.raw, nt * np * 2, {.src_map = p.nu2 ? identity_map() : IndexMap{2 * s.num_per, 2 * s.num_per, 0},
                                                      .dst_map = IndexMap{2 * np, 2 * s.num_per, 0}, .lanes = lanes}), st);
    HIP_OK(hipEventRecord(S->ev[5], st));
    S->packed_after_front = false;
    return 0;
}

static int pk_fold(spiral_gpu_pack_server* S, const Lanes& lanes, hipStream_t st) { return pk_fold_into(S, S->own, S->nt, lanes, st); }

static int pk_front(spiral_gpu_pack_server* S) {
    const Lanes one{};
    if (pk_expand_convert(S, one, S->stream) || pk_sweep(S, one, S->stream)) return -1;
    return pk_fold(S, one, S->stream);
}

// pack + modulus switch (:1064-1081) of out_n^2 folded ciphertexts at a stride of `ct_stride` ciphertexts; event 6 closes it.  With lanes `folded` is
// S's own raw buffer, and the switch is one launch_rescale2 for all of them (row 0 to q', the rest to 4p: the same words as the two launches of one client)
static int pk_back(spiral_gpu_pack_server* S, const uint64_t* folded, uint32_t ct_stride, const Lanes& lanes, hipStream_t st) {
    const spiral_gpu_params& p = S->p;
    const PkBufs& B = S->own;
    const uint32_t rows = S->out_n + 1;
    run_pack(S->tb, folded, ct_stride, S->v_w.p, B.ginv, B.ct2, B.res, S->out_n, p.t_conv, st, 1, lanes);
    launch_job(S->tb, lift_job(B.res, B.pk_raw, rows * S->out_n, {.lanes = lanes}), st);
    if (lanes.n > 1) {
        launch_rescale2(B.pk_raw, B.resp, S->out_n * kN, rows * S->out_n * kN, kQ, S->s.qprime, 4 * p.p_db, st, lanes);
    } else {
        launch_rescale(B.pk_raw, B.resp, S->out_n * kN, kQ, S->s.qprime, st);
        launch_rescale(B.pk_raw + (size_t)S->out_n * kN, B.resp + (size_t)S->out_n * kN, S->out_n * S->out_n * kN, kQ, 4 * p.p_db, st);
    }
    HIP_OK(hipEventRecord(S->ev[6], st));
    S->packed_after_front = folded == B.raw;  // (a gathered buffer was filled by other servers too: no common time line)
    return 0;
}

static int pk_download(spiral_gpu_pack_server* S, uint64_t* response, uint64_t* packed_ct) {
    const uint32_t rows = S->out_n + 1;
    HIP_OK(hipStreamSynchronize(S->stream));
    HIP_OK(hipGetLastError());
    if (response) HIP_OK(hipMemcpy(response, S->own.resp, (size_t)rows * S->out_n * kPolyBytes, hipMemcpyDeviceToHost));
    if (packed_ct) {
        Scratch sc;
        if (download_pk(sc, S->own.res, identity_map(), packed_ct, (size_t)rows * S->out_n)) return -1;
    }
    return 0;
}

// what an answer checks before its query is taken
static int pk_check_answer(spiral_gpu_pack_server* S) {
    HIP_OK(hipSetDevice(S->device));
    if (!S->img->loaded || !S->have_pp) return fail("database and public parameters must be set first");
    if (S->nt != S->s.trials) return fail("this server holds trials [%u, %u) only: fold_trials + pack_gathered", S->t0, S->t0 + S->nt);
    return 0;
}

// the answer to the query in S->query
static int pk_answer_taken(spiral_gpu_pack_server* S, uint64_t* response, uint64_t* packed_ct, double stage_us[8]) {
    if (pk_front(S) || pk_back(S, S->own.raw, S->s.num_per, Lanes{}, S->stream) || pk_download(S, response, packed_ct)) return -1;
    return stage_us ? spiral_gpu_pack_server_stage_us(S, stage_us) : 0;
}

static int pk_answer(spiral_gpu_pack_server* S, Form form, const void* query, size_t bytes, uint64_t* response, uint64_t* packed_ct, double stage_us[8],
                     const char* what) {
    if (!S || !query) return fail("null argument");
    if (pk_check_answer(S) || pk_take_query(S, form, query, bytes, what)) return -1;
    return pk_answer_taken(S, response, packed_ct, stage_us);
}

int spiral_gpu_pack_server_answer(spiral_gpu_pack_server* S, const uint64_t* query, uint64_t* response, uint64_t* packed_ct, double stage_us[8]) {
    return pk_answer(S, FORM_NTT, query, 0, response, packed_ct, stage_us, "answer");
}
int spiral_gpu_pack_server_answer_wire(spiral_gpu_pack_server* S, const void* query_wire, size_t bytes, uint64_t* response, uint64_t* packed_ct,
                                       double stage_us[8]) {
    return pk_answer(S, FORM_WIRE, query_wire, bytes, response, packed_ct, stage_us, "answer_wire");
}
int spiral_gpu_pack_server_answer_seeded(spiral_gpu_pack_server* S, const void* query_msg, size_t bytes, uint64_t* response, uint64_t* packed_ct,
                                         double stage_us[8]) {
    return pk_answer(S, FORM_SEEDED, query_msg, bytes, response, packed_ct, stage_us, "answer_seeded");
}

// the lanes of a batch, checked before anything is launched, and their arena offsets: the list, the image, NO_CAPTURE and the layouts in lanes.h,
// between them SpiralPack's own rules -- none trial-sharded unless the call takes TRIAL_SHARDS, the same parameters, out_n and trial range, and what
// `needs` names (NEED_DB, NEED_RECORDS; public parameters unless the call GIVES_KEYS)
static int pk_check_lanes(spiral_gpu_pack_server* const* servers, uint32_t n, const char* what, uint32_t needs, Lanes* lanes) {
    return check_lane_list(servers, n, what, needs, lanes, [&](uint32_t b) {
        const spiral_gpu_pack_server *H = servers[0], *L = servers[b];
        if (!(needs & TRIAL_SHARDS) && H->nt != H->s.trials) return fail("%s: the image holds trials [%u, %u) only: trial-sharded servers have no batch", what, H->t0, H->t0 + H->nt);
        if ((needs & NEED_DB) && !H->img->loaded) return fail("%s: no database loaded", what);
        if (memcmp(&L->p, &H->p, sizeof(L->p)) != 0 || L->out_n != H->out_n || L->device != H->device || L->nt != H->nt || L->t0 != H->t0)
            return fail("%s: server %u has other parameters than server 0", what, b);
        if (!(needs & GIVES_KEYS) && !L->have_pp) return fail("%s: server %u has no public parameters", what, b);
        if ((needs & NEED_RECORDS) && !L->have_records) return fail("%s: server %u has no converted query (answer it once first)", what, b);
        return 0;
    });
}

// The queries of a multi-lane call, one per server.  Every argument (in the message forms each query's byte count included) is checked before anything
// is uploaded; then every lane's query is taken into its own buffer, and only when all of them were does anything launch -- a bad query leaves every
// lane's previous results intact
static int pk_take_queries(spiral_gpu_pack_server* const* servers, uint32_t n, Form form, const void* const* queries, size_t bytes_each, const char* what) {
    if (!queries) return fail("%s: null queries", what);
    const spiral_gpu_pack_server* S = servers[0];
    const size_t want = message_bytes(pack_query_layout(S->p, S->s, S->out_n), form);
    if (form != FORM_NTT && bytes_each != want)
        return fail("%s: %zu bytes per query, the %s form of a query takes %zu", what, bytes_each, form == FORM_SEEDED ? "seeded" : "wire", want);
    for (uint32_t b = 0; b < n; b++)
        if (!queries[b]) return fail("%s: query %u is null", what, b);
    for (uint32_t b = 0; b < n; b++) {
        char w[64];
        snprintf(w, sizeof(w), "%s: query %u", what, b);
        if (pk_take_query(servers[b], form, queries[b], bytes_each, w)) return -1;
    }
    return 0;
}

// spiral_gpu_server_bind_keys for SpiralPack: the keys of slot slots[b] of a store created for this out_n into lane b's W_exp_left, W_exp_right, V and v_W
int spiral_gpu_pack_server_bind_keys(spiral_gpu_pack_server* const* servers, uint32_t n, spiral_gpu_key_store* store, const uint32_t* slots) {
    const char* what = "pack bind_keys";
    Lanes lanes;
    if (pk_check_lanes(servers, n, what, NO_CAPTURE | GIVES_KEYS | TRIAL_SHARDS, &lanes)) return -1;  // (every rank holds every client's keys)
    spiral_gpu_pack_server* S = servers[0];
    uint64_t* const dst[kMessageParts] = {S->w_left.p, S->w_right.p, S->v.p, S->v_w.p};
    const size_t dst_words[kMessageParts] = {S->w_left.words, S->w_right.words, S->v.words, S->v_w.words};
    return bind_keys(servers, lanes, store, slots, S->out_n, dst, dst_words, what);
}

// whether a call of n clients runs as one lane-aware launch sequence (option pack_batch_lanes, read per call; 0 = never)
static bool pk_lane_form(uint32_t n) { return n >= 2 && options().pack_batch_lanes != 0 && n >= options().pack_batch_lanes; }

// Beyond the reference (one query per call): n <= kMaxLanes queries, one per server, in one launch sequence on servers[0]'s stream, with ONE
// first-dimension pass over the trial images for all of them (matrix cores, once the image is in limb-plane form: the first batch on a covered geometry
// converts it).  From option pack_batch_lanes clients on (the lane form) every other launch carries all n clients too, in gridDim.z: one expansion and
// conversion, the pass, one folding, one packing and switch; below it those run per lane, one client after another.  Either way every lane's buffers and
// flags end up as its own answer would leave them.  Returns synchronised.
static int pk_answer_batch(spiral_gpu_pack_server* const* servers, uint32_t n, Form form, const void* const* queries, size_t bytes_each,
                           uint64_t* const* responses, uint64_t* const* packed_cts, double stage_us[8], const char* what) {
    Lanes lanes;
    if (pk_check_lanes(servers, n, what, NEED_DB, &lanes) || pk_take_queries(servers, n, form, queries, bytes_each, what)) return -1;
    if (n == 1) return pk_answer_taken(servers[0], responses ? responses[0] : nullptr, packed_cts ? packed_cts[0] : nullptr, stage_us);
    spiral_gpu_pack_server* S = servers[0];
    if (S->img->lay.limbs_ok() && S->img->set_format(SPIRAL_GPU_DB_LIMBS, S->stream)) return -1;
    hipStream_t st = S->stream;
    const bool lane_form = pk_lane_form(n);
    if (lane_form) {
        if (lanes_join(servers, n)) return -1;  // (the queries were taken on the lanes' own streams)
        if (pk_expand_convert(S, lanes, st) || pk_sweep(S, lanes, st)) return -1;
        HIP_OK(hipEventRecord(S->ev[7], st));  // (the sweep began at event 2)
        if (pk_fold(S, lanes, st) || pk_back(S, S->own.raw, S->s.num_per, lanes, st) || lanes_release(servers, n)) return -1;
        for (uint32_t b = 1; b < n; b++)  // (what the pieces set on servers[0]; the stages' events are servers[0]'s alone)
            servers[b]->have_records = true, servers[b]->packed_after_front = true, servers[b]->events_elsewhere = true;
        g_pack_lane_batches++;
    } else {
        for (uint32_t b = 0; b < n; b++)
            if (pk_expand_convert(servers[b], Lanes{}, st)) return -1;
        if (pk_sweep(S, lanes, st)) return -1;
        HIP_OK(hipEventRecord(S->ev[7], st));  // (the sweep began at servers[n - 1]'s event 2)
        for (uint32_t b = 0; b < n; b++) {
            spiral_gpu_pack_server* L = servers[b];
            if (pk_fold(L, Lanes{}, st) || pk_back(L, L->own.raw, L->s.num_per, Lanes{}, st)) return -1;
        }
    }
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    for (uint32_t b = 0; b < n; b++)
        if (pk_download(servers[b], responses ? responses[b] : nullptr, packed_cts ? packed_cts[b] : nullptr)) return -1;
    if (!stage_us) return 0;
    for (int i = 0; i < 8; i++) stage_us[i] = 0;
    float sw = 0, total = 0;
    if (lane_form) {
        // whole-batch intervals between servers[0]'s events: the lanes' stages ran together, [2] = [5] the one shared sweep
        float ms[4] = {};
        HIP_OK(hipEventElapsedTime(&ms[0], S->ev[0], S->ev[1]));
        HIP_OK(hipEventElapsedTime(&ms[1], S->ev[1], S->ev[2]));
        HIP_OK(hipEventElapsedTime(&ms[2], S->ev[4], S->ev[5]));
        HIP_OK(hipEventElapsedTime(&ms[3], S->ev[5], S->ev[6]));
        stage_us[0] = ms[0] * 1e3, stage_us[1] = ms[1] * 1e3, stage_us[3] = ms[2] * 1e3, stage_us[4] = ms[3] * 1e3;
        HIP_OK(hipEventElapsedTime(&sw, S->ev[2], S->ev[7]));
        HIP_OK(hipEventElapsedTime(&total, S->ev[0], S->ev[6]));
    } else {
        // the lanes' stages ran one after another on one stream: [0], [1], [3], [4] are the sums over the lanes, [2] = [5] the one shared sweep
        for (uint32_t b = 0; b < n; b++) {
            spiral_gpu_pack_server* L = servers[b];
            float ms[4] = {};
            HIP_OK(hipEventElapsedTime(&ms[0], L->ev[0], L->ev[1]));
            HIP_OK(hipEventElapsedTime(&ms[1], L->ev[1], L->ev[2]));
            HIP_OK(hipEventElapsedTime(&ms[2], L->ev[4], L->ev[5]));
            HIP_OK(hipEventElapsedTime(&ms[3], L->ev[5], L->ev[6]));
            stage_us[0] += ms[0] * 1e3, stage_us[1] += ms[1] * 1e3, stage_us[3] += ms[2] * 1e3, stage_us[4] += ms[3] * 1e3;
        }
        HIP_OK(hipEventElapsedTime(&sw, servers[n - 1]->ev[2], S->ev[7]));
        HIP_OK(hipEventElapsedTime(&total, S->ev[0], servers[n - 1]->ev[6]));
    }
    stage_us[2] = stage_us[5] = sw * 1e3;
    stage_us[6] = total * 1e3;
    stage_us[7] = n;
    return 0;
}

int spiral_gpu_pack_server_answer_batch(spiral_gpu_pack_server* const* servers, uint32_t n, const uint64_t* const* queries, uint64_t* const* responses,
                                        uint64_t* const* packed_cts, double stage_us[8]) {
    return pk_answer_batch(servers, n, FORM_NTT, (const void* const*)queries, 0, responses, packed_cts, stage_us, "answer_batch");
}
int spiral_gpu_pack_server_answer_batch_wire(spiral_gpu_pack_server* const* servers, uint32_t n, const void* const* query_wires, size_t bytes_each,
                                             uint64_t* const* responses, uint64_t* const* packed_cts, double stage_us[8]) {
    return pk_answer_batch(servers, n, FORM_WIRE, query_wires, bytes_each, responses, packed_cts, stage_us, "answer_batch_wire");
}
int spiral_gpu_pack_server_answer_batch_seeded(spiral_gpu_pack_server* const* servers, uint32_t n, const void* const* query_msgs, size_t bytes_each,
                                               uint64_t* const* responses, uint64_t* const* packed_cts, double stage_us[8]) {
    return pk_answer_batch(servers, n, FORM_SEEDED, query_msgs, bytes_each, responses, packed_cts, stage_us, "answer_batch_seeded");
}

// ---- items of several database instances (answer_batch_instances, include/spiral_gpu.h) ----
// every argument check, before anything is uploaded or launched; what the clients' own image holds does not matter (it is read only as an instance)
static int pk_check_items(spiral_gpu_pack_server* const* servers, uint32_t n, spiral_gpu_pack_server* const* instances, uint32_t n_inst, const void* queries,
                          const void* responses, const void* wire, const char* what, Lanes* lanes) {
    if (!servers || !instances || !queries) return fail("%s: null servers, instances or queries", what);
    if (n_inst == 0) return fail("%s: no instances", what);
    if (!responses && !wire) return fail("%s: no output (responses or wire)", what);
    if (pk_check_lanes(servers, n, what, 0, lanes)) return -1;
    const spiral_gpu_pack_server* S = servers[0];
    for (uint32_t k = 0; k < n_inst; k++) {
        const spiral_gpu_pack_server* I = instances[k];
        if (!I) return fail("%s: instance %u is null or destroyed", what, k);
        if (memcmp(&I->p, &S->p, sizeof(S->p)) != 0 || I->out_n != S->out_n || I->device != S->device)
            return fail("%s: instance %u has other parameters, out_n or device than the clients", what, k);
        if (I->nt != I->s.trials) return fail("%s: instance %u holds trials [%u, %u) only: trial-sharded servers are no instances", what, k, I->t0, I->t0 + I->nt);
        if (!I->img->loaded) return fail("%s: instance %u has no database loaded", what, k);
    }
    return 0;
}

// the group size: option pack_item_group (0 = automatic: the largest G <= n_inst whose arenas, on every client, fit a quarter of the device memory free
// now, counting what the clients' arenas already hold), never more launch rows than the folding's product takes in one grid dimension; then the
// arenas, halving G while an allocation fails.  G = 1 needs none: the clients' own buffers.
static size_t pk_group_words(spiral_gpu_pack_server* S, uint32_t G) {  // (the sizing pass of pk_answer_items' carve)
    Arena a;
    PkBufs B;
    pk_layout(S, a, false, G, B);
    return a.used;
}
static uint32_t pk_item_group(spiral_gpu_pack_server* const* servers, uint32_t n, uint32_t n_inst) {
    spiral_gpu_pack_server* S = servers[0];
    const size_t per_group = (size_t)S->nt * (S->s.num_per / 2);  // the first fold round's ciphertexts per instance: grid rows of pack_fold_mac
    uint32_t G = options().pack_item_group ? std::min(options().pack_item_group, n_inst) : n_inst;
    G = (uint32_t)std::max<size_t>(1, std::min<size_t>(G, 65535 / std::max<size_t>(1, per_group)));
    if (G > 1 && options().pack_item_group == 0) {
        size_t free_b = 0, total_b = 0, held = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
        (void)hipGetLastError();
        for (uint32_t b = 0; b < n; b++) held += servers[b]->item.p ? servers[b]->item.words * 8 : 0;
        const size_t budget = (free_b + held) / 4;
        while (G > 1 && (size_t)n * pk_group_words(S, G) * 8 > budget) G--;
    }
    for (; G > 1; G /= 2) {
        bool ok = true;
        for (uint32_t b = 0; b < n && ok; b++) {
            spiral_gpu_pack_server* L = servers[b];
            if (L->item_cap >= G) continue;
            L->item.release();
            L->item_cap = 0;
            const size_t words = pk_group_words(L, G);
            if (hipMalloc(&L->item.p, words * 8) != hipSuccess) {
                (void)hipGetLastError();  // (no sticky out-of-memory for the launches that follow)
                L->item.p = nullptr;
                ok = false;
            } else {
                L->item.words = words, L->item.carved = false, L->item_cap = G;
            }
        }
        if (ok) return G;
    }
    return 1;
}

// the packing, switch and wire form of one client's group of g instances (folded in B): one launch sequence for all g
static int pk_item_back(spiral_gpu_pack_server* L, const PkBufs& B, uint32_t g, bool want_wire, hipStream_t st) {
    const spiral_gpu_params& p = L->p;
    const uint32_t rows = L->out_n + 1;
    run_pack(L->tb, B.raw, L->s.num_per, L->v_w.p, B.ginv, B.ct2, B.res, L->out_n, p.t_conv, st, g);
    launch_job(L->tb, lift_job(B.res, B.pk_raw, g * rows * L->out_n), st);
    const Slots slots{g, (int64_t)B.slot_words};
    launch_rescale2_slots(B.pk_raw, B.resp, L->out_n * kN, (uint32_t)B.slot_words, kQ, L->s.qprime, 4 * p.p_db, slots, st);
    if (want_wire)
        launch_response_wire_slots(B.resp, B.wire, L->out_n * kN, p.qprime_bits, L->out_n * L->out_n * kN, wire_bits_rest(&p), slots, (int64_t)B.wire_words, st);
    L->packed_after_front = false;
    return 0;
}

// the item call: every argument checked, then every query taken; the launches run only when all of them were
static int pk_answer_items(spiral_gpu_pack_server* const* servers, uint32_t n, spiral_gpu_pack_server* const* instances, uint32_t n_inst, Form form,
                           const void* const* queries, size_t bytes_each, uint64_t* responses, void* wire, double* total_us, const char* what) {
    Lanes lanes;
    if (pk_check_items(servers, n, instances, n_inst, queries, responses, wire, what, &lanes) || pk_take_queries(servers, n, form, queries, bytes_each, what))
        return -1;
    spiral_gpu_pack_server* S = servers[0];
    hipStream_t st = S->stream;
    // whatever the clients' and the instances' streams hold (an update_db_items on an instance's holder) comes first
    if (lanes_join(servers, n)) return -1;
    for (uint32_t k = 0; k < n_inst; k++)
        if (stream_before(instances[k], st) || (pk_owner(instances[k]) && stream_before(pk_owner(instances[k]), st))) return -1;  // (no owner left: nothing writes the image)
    // a batch sweeps each instance image on the matrix cores where the geometry has limb planes: converted in place on first use, as answer_batch's holder
    if (n >= 2 && DbLayout::packed1(S->s.num_per, S->s.dim0, S->s.trials).limbs_ok())
        for (uint32_t k = 0; k < n_inst; k++)
            if (instances[k]->img->set_format(SPIRAL_GPU_DB_LIMBS, st)) return -1;
    const uint32_t G = pk_item_group(servers, n, n_inst);
    PkBufs bufs[kMaxLanes];  // G = 1: the clients' own; else their item arenas, carved for G instances
    for (uint32_t b = 0; b < n; b++) {
        Arena a{servers[b]->item.p};
        bufs[b] = servers[b]->own;
        if (G > 1) pk_layout(servers[b], a, false, G, bufs[b]);
    }
    const size_t slot_words = bufs[0].slot_words, wire_b = bufs[0].wire_words * 8;
    const uint32_t* qs[kMaxLanes];
    pk_lane_records(S, lanes, qs);
    // expansion and conversion, once per client whatever the number of instances: one lane-aware sequence from option pack_batch_lanes clients on.  (The
    // folding and packing below stay per client: an item group's arena is an allocation of its own, outside the arena the lane offsets are taken from.)
    if (pk_lane_form(n)) {
        if (pk_expand_convert(S, lanes, st)) return -1;
        for (uint32_t b = 1; b < n; b++) servers[b]->have_records = true, servers[b]->events_elsewhere = true;
        g_pack_lane_batches++;
    } else {
        for (uint32_t b = 0; b < n; b++)
            if (pk_expand_convert(servers[b], Lanes{}, st)) return -1;
    }
    for (uint32_t k0 = 0; k0 < n_inst; k0 += G) {
        const uint32_t g = std::min(G, n_inst - k0);
        for (uint32_t j = 0; j < g; j++) {  // one first-dimension pass per instance for all clients, into instance j's part of each group arena
            uint64_t* acc[kMaxLanes];
            for (uint32_t b = 0; b < n; b++) acc[b] = bufs[b].acc + (size_t)j * bufs[b].acc_words;
            if (pk_sweep_into(instances[k0 + j]->img, qs, acc, n, st)) return -1;
        }
        for (uint32_t b = 0; b < n; b++) {  // folding, packing, switch and wire form: one sequence per client and group
            spiral_gpu_pack_server* L = servers[b];
            if (pk_fold_into(L, bufs[b], g * L->nt, Lanes{}, st) || pk_item_back(L, bufs[b], g, wire != nullptr, st)) return -1;
            const size_t first = (size_t)b * n_inst + k0;
            if (responses) HIP_OK(hipMemcpyAsync(responses + first * slot_words, bufs[b].resp, g * slot_words * 8, hipMemcpyDeviceToHost, st));
            if (wire) HIP_OK(hipMemcpyAsync((uint8_t*)wire + first * wire_b, bufs[b].wire, g * wire_b, hipMemcpyDeviceToHost, st));
        }
    }
    HIP_OK(hipEventRecord(S->ev[7], st));
    for (uint32_t b = 1; b < n; b++)  // and what follows on the other streams comes after
        if (stream_after(servers[b], st, S->ev[7])) return -1;
    for (uint32_t k = 0; k < n_inst; k++)
        if (stream_after(instances[k], st, S->ev[7]) || (pk_owner(instances[k]) && stream_after(pk_owner(instances[k]), st, S->ev[7]))) return -1;
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    if (total_us) {
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, S->ev[0], S->ev[7]));
        *total_us = ms * 1e3;
    }
    return 0;
}

int spiral_gpu_pack_server_answer_batch_instances(spiral_gpu_pack_server* const* servers, uint32_t n_clients, spiral_gpu_pack_server* const* instances,
                                                  uint32_t n_instances, const uint64_t* const* queries, uint64_t* responses, void* wire, double* total_us) {
    return pk_answer_items(servers, n_clients, instances, n_instances, FORM_NTT, (const void* const*)queries, 0, responses, wire, total_us,
                           "answer_batch_instances");
}
int spiral_gpu_pack_server_answer_batch_instances_wire(spiral_gpu_pack_server* const* servers, uint32_t n_clients, spiral_gpu_pack_server* const* instances,
                                                       uint32_t n_instances, const void* const* query_wires, size_t bytes_each, uint64_t* responses, void* wire,
                                                       double* total_us) {
    return pk_answer_items(servers, n_clients, instances, n_instances, FORM_WIRE, query_wires, bytes_each, responses, wire, total_us,
                           "answer_batch_instances_wire");
}
int spiral_gpu_pack_server_answer_batch_instances_seeded(spiral_gpu_pack_server* const* servers, uint32_t n_clients, spiral_gpu_pack_server* const* instances,
                                                         uint32_t n_instances, const void* const* query_msgs, size_t bytes_each, uint64_t* responses,
                                                         void* wire, double* total_us) {
    return pk_answer_items(servers, n_clients, instances, n_instances, FORM_SEEDED, query_msgs, bytes_each, responses, wire, total_us,
                           "answer_batch_instances_seeded");
}

// the batched first-dimension sweep alone (answer_batch's), iters times on servers[0]'s stream with the lanes' current records, timed with device
// events; as answer_batch, a covered geometry's image is converted to limb planes first
int spiral_gpu_pack_server_time_sweep_batch(spiral_gpu_pack_server* const* servers, uint32_t n, int iters, float* avg_ms) {
    if (!avg_ms || iters <= 0) return fail("time_sweep_batch: bad argument");
    Lanes lanes;
    if (pk_check_lanes(servers, n, "time_sweep_batch", NEED_DB | NEED_RECORDS, &lanes)) return -1;
    spiral_gpu_pack_server* S = servers[0];
    if (S->img->lay.limbs_ok() && S->img->set_format(SPIRAL_GPU_DB_LIMBS, S->stream)) return -1;
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipEventRecord(S->ev[0], S->stream));
    for (int i = 0; i < iters; i++)
        if (pk_sweep(S, lanes, S->stream)) return -1;
    HIP_OK(hipEventRecord(S->ev[1], S->stream));
    HIP_OK(hipStreamSynchronize(S->stream));
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, S->ev[0], S->ev[1]));
    *avg_ms = ms / iters;
    for (uint32_t b = 0; b < n; b++) servers[b]->packed_after_front = false;
    return 0;
}

// stage times of the last answer (or fold_trials [+ pack_gathered]) from the events between its stages; synchronises the stream.
// [4] packing and [6] total are 0 when no packing followed the last fold_trials on this server.
int spiral_gpu_pack_server_stage_us(spiral_gpu_pack_server* S, double stage_us[8]) {
    if (!S || !stage_us) return fail("null argument");
    HIP_OK(hipSetDevice(S->device));
    if (S->events_elsewhere)
        return fail("this server's last answer was a lane of a lane-form batch or item call: its stages were timed on that call's servers[0] (the call's stage_us / total_us)");
    HIP_OK(hipStreamSynchronize(S->stream));
    float ms[6] = {}, total = 0;
    for (int i = 0; i < (S->packed_after_front ? 6 : 5); i++) HIP_OK(hipEventElapsedTime(&ms[i], S->ev[i], S->ev[i + 1]));
    if (S->packed_after_front) HIP_OK(hipEventElapsedTime(&total, S->ev[0], S->ev[6]));
    stage_us[0] = ms[0] * 1e3;
    stage_us[1] = ms[1] * 1e3;
    stage_us[2] = (ms[2] + ms[3]) * 1e3;
    stage_us[3] = ms[4] * 1e3;
    stage_us[4] = ms[5] * 1e3;
    stage_us[5] = ms[2] * 1e3;
    stage_us[6] = total * 1e3;
    stage_us[7] = 0;
    return 0;
}

// trial-sharded answer, part 1: expansion and conversion (replicated: they are database-independent), then the sweeps and the folding
// of this server's trials; their folded ciphertexts ([nt][2][N] raw words) are left at `folded_dev`, a device buffer of the caller
// (the send buffer of the all-gather).  Asynchronous on the server's stream.
int spiral_gpu_pack_server_fold_trials(spiral_gpu_pack_server* S, const uint64_t* query, void* folded_dev) {
    if (!S || !query || !folded_dev) return fail("null argument");
    HIP_OK(hipSetDevice(S->device));
    if (!S->img->loaded || !S->have_pp) return fail("database and public parameters must be set first");
    if (pk_take_query(S, FORM_NTT, query, 0, "fold_trials") || pk_front(S)) return -1;
    HIP_OK(hipMemcpy2DAsync(folded_dev, 2 * kPolyBytes, S->own.raw, (size_t)S->s.num_per * 2 * kPolyBytes, 2 * kPolyBytes, S->nt, hipMemcpyDeviceToDevice,
                            S->stream));
    return 0;
}

// part 2, on the root: pack + modulus switch of all out_n^2 folded ciphertexts (`gathered_dev`: [out_n^2][2][N] raw words in trial
// order, device memory -- the receive buffer of the all-gather)
int spiral_gpu_pack_server_pack_gathered(spiral_gpu_pack_server* S, const void* gathered_dev, uint64_t* response, uint64_t* packed_ct) {
    if (!S || !gathered_dev) return fail("null argument");
    HIP_OK(hipSetDevice(S->device));
    if (!S->have_pp) return fail("public parameters must be set first");
    if (pk_back(S, (const uint64_t*)gathered_dev, 1, Lanes{}, S->stream)) return -1;
    return pk_download(S, response, packed_ct);
}

// ---- batches of a trial-sharded answer (include/spiral_gpu.h): fold_trials_batch on every rank, one all-gather, pack_gathered_batch on the root ----
// the server that may write the lanes' image, when it is none of them: its stream (an update_db_items) is ordered around the call too
static spiral_gpu_pack_server* pk_outside_owner(spiral_gpu_pack_server* const* servers, uint32_t n) {
    spiral_gpu_pack_server* own = pk_owner(servers[0]);
    for (uint32_t b = 0; b < n; b++)
        if (servers[b] == own) return nullptr;
    return own;
}

// part 1 for n clients: answer_batch's front half over this rank's trials -- expansion and conversion (lane form or per lane), ONE sweep of the
// local images for all lanes, the folding -- and lane b's nt folded ciphertexts to folded_dev + (b * nt + k) x 2 x 2048 words.  Asynchronous on
// servers[0]'s stream, the other lanes' streams ordered around it.
int spiral_gpu_pack_server_fold_trials_batch(spiral_gpu_pack_server* const* servers, uint32_t n, int form, const void* const* queries, size_t bytes_each,
                                             void* folded_dev) {
    const char* what = "fold_trials_batch";
    if (!queries || !folded_dev) return fail("%s: null queries or output buffer", what);
    if (form != FORM_NTT && form != SPIRAL_GPU_FORM_WIRE && form != SPIRAL_GPU_FORM_SEEDED) return fail("%s: unknown query form %d", what, form);
    Lanes lanes;
    if (pk_check_lanes(servers, n, what, NEED_DB | NO_CAPTURE | TRIAL_SHARDS, &lanes) || pk_take_queries(servers, n, (Form)form, queries, bytes_each, what))
        return -1;
    spiral_gpu_pack_server* S = servers[0];
    hipStream_t st = S->stream;
    if (n >= 2 && S->img->lay.limbs_ok() && S->img->set_format(SPIRAL_GPU_DB_LIMBS, st)) return -1;
    spiral_gpu_pack_server* own = pk_outside_owner(servers, n);
    if (lanes_join(servers, n) || (own && stream_before(own, st))) return -1;
    if (n == 1) {
        if (pk_front(S)) return -1;
    } else if (pk_lane_form(n)) {
        if (pk_expand_convert(S, lanes, st) || pk_sweep(S, lanes, st)) return -1;
        HIP_OK(hipEventRecord(S->ev[7], st));
        if (pk_fold(S, lanes, st)) return -1;
        for (uint32_t b = 1; b < n; b++) servers[b]->have_records = true, servers[b]->packed_after_front = false, servers[b]->events_elsewhere = true;
        g_pack_lane_batches++;
    } else {
        for (uint32_t b = 0; b < n; b++)
            if (pk_expand_convert(servers[b], Lanes{}, st)) return -1;
        if (pk_sweep(S, lanes, st)) return -1;
        HIP_OK(hipEventRecord(S->ev[7], st));
        for (uint32_t b = 0; b < n; b++)
            if (pk_fold(servers[b], Lanes{}, st)) return -1;
    }
    const size_t ct_bytes = 2 * kPolyBytes;
    for (uint32_t b = 0; b < n; b++)  // one strided copy per lane: the head of each trial's num_per slots
        HIP_OK(hipMemcpy2DAsync((uint8_t*)folded_dev + (size_t)b * S->nt * ct_bytes, ct_bytes, servers[b]->own.raw, (size_t)S->s.num_per * ct_bytes, ct_bytes,
                                S->nt, hipMemcpyDeviceToDevice, st));
    if (lanes_release(servers, n)) return -1;
    if (own && own->stream != st) {
        HIP_OK(hipEventRecord(S->ev_lane, st));
        if (stream_after(own, st, S->ev_lane)) return -1;
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// part 2 for n clients, on the root: the gathered rank-major blocks (block r = [lane][k] of the trials [cuts[r], cuts[r + 1]), at a stride of
// block_cts ciphertexts) regrouped into each lane's trial order in ONE launch, then ONE lane-aware pack and switch.  Returns synchronised.
int spiral_gpu_pack_server_pack_gathered_batch(spiral_gpu_pack_server* const* servers, uint32_t n, const void* gathered_dev, const uint32_t* cuts,
                                               uint32_t n_ranks, uint64_t block_cts, uint64_t* const* responses, uint64_t* const* packed_cts, void* wire) {
    const char* what = "pack_gathered_batch";
    if (!gathered_dev || !cuts) return fail("%s: null gathered buffer or cuts", what);
    if (!responses && !packed_cts && !wire) return fail("%s: no output (responses, packed_cts or wire)", what);
    Lanes lanes;
    if (pk_check_lanes(servers, n, what, NO_CAPTURE | TRIAL_SHARDS, &lanes)) return -1;
    spiral_gpu_pack_server* S = servers[0];
    const uint32_t trials = S->s.trials;
    if ((uintptr_t)gathered_dev % 16) return fail("%s: the gathered buffer must be 16-byte aligned", what);
    if (n_ranks == 0 || n_ranks > trials) return fail("%s: %u ranks for %u trials", what, n_ranks, trials);
    if (cuts[0] != 0 || cuts[n_ranks] != trials) return fail("%s: the cuts run from %u to %u, not from 0 to %u", what, cuts[0], cuts[n_ranks], trials);
    uint32_t longest = 0;
    for (uint32_t r = 0; r < n_ranks; r++) {
        if (cuts[r + 1] <= cuts[r] || cuts[r + 1] > trials) return fail("%s: the cuts are not strictly increasing at rank %u", what, r);
        longest = std::max(longest, cuts[r + 1] - cuts[r]);
    }
    if (block_cts < (uint64_t)n * longest || block_cts > ((uint64_t)1 << 32))
        return fail("%s: blocks of %llu ciphertexts, %u lanes of up to %u trials need at least %llu", what, (unsigned long long)block_cts, n, longest,
                    (unsigned long long)n * longest);
    static_assert(kMaxPackTrials >= 16 * 16, "the cuts of every out_n fit the regroup launch's table");
    const size_t nbytes = wire_bytes(&S->p, S->out_n);
    if (wire && S->wire_batch.words * 8 < n * nbytes && (S->wire_batch.release(), S->wire_batch.alloc(n * nbytes / 8))) return -1;
    hipStream_t st = S->stream;
    if (lanes_join(servers, n)) return -1;
    PackRegroupParams rp{(const uint64_t*)gathered_dev, S->gath.p, block_cts, n_ranks, {}, lanes};
    std::copy(cuts, cuts + n_ranks + 1, rp.cuts);
    launch_pack_regroup(rp, trials, st);
    if (pk_back(S, S->gath.p, 1, lanes, st)) return -1;
    for (uint32_t b = 1; b < n; b++) servers[b]->packed_after_front = false;
    if (wire) {
        launch_response_wire(S->own.resp, S->wire_batch.p, S->out_n * kN, S->p.qprime_bits, S->out_n * S->out_n * kN, wire_bits_rest(&S->p), st, lanes, 0,
                             (int64_t)(nbytes / 8));
        HIP_OK(hipMemcpyAsync(wire, S->wire_batch.p, n * nbytes, hipMemcpyDeviceToHost, st));
    }
    if (lanes_release(servers, n)) return -1;
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    for (uint32_t b = 0; b < n; b++)
        if (pk_download(servers[b], responses ? responses[b] : nullptr, packed_cts ? packed_cts[b] : nullptr)) return -1;
    return 0;
}

int spiral_gpu_pack_server_set_stream(spiral_gpu_pack_server* S, void* stream) {
    if (enter(S)) return -1;
    HIP_OK(hipStreamSynchronize(S->stream));
    if (S->own_stream) {
        (void)hipStreamDestroy(S->stream);
        S->own_stream = false;
    }
    S->stream = (hipStream_t)stream;
    return 0;
}

int spiral_gpu_pack_server_read_response_wire(spiral_gpu_pack_server* S, void* out, size_t capacity) {
    if (!S || !out) return fail("null argument");
    HIP_OK(hipSetDevice(S->device));
    const size_t nbytes = wire_bytes(&S->p, S->out_n);
    if (capacity < nbytes) return fail("response buffer of %zu bytes, the wire form needs %zu", capacity, nbytes);
    launch_response_wire(S->own.resp, S->own.wire, S->out_n * kN, S->p.qprime_bits, S->out_n * S->out_n * kN, wire_bits_rest(&S->p), S->stream);
    HIP_OK(hipMemcpyAsync(out, S->own.wire, nbytes, hipMemcpyDeviceToHost, S->stream));
    HIP_OK(hipStreamSynchronize(S->stream));
    return 0;
}

int spiral_gpu_pack_server_read_acc(spiral_gpu_pack_server* S, uint32_t trial, uint64_t* out) {
    if (!S || !out) return fail("null argument");
    HIP_OK(hipSetDevice(S->device));
    if (pk_check_trial(S, trial)) return -1;
    HIP_OK(hipStreamSynchronize(S->stream));
    Scratch sc;
    return download_pk(sc, S->own.acc + (size_t)(trial - S->t0) * S->s.num_per * 2 * kN, identity_map(), out, (size_t)S->s.num_per * 2);
}

uint64_t spiral_gpu_pack_server_sweep_bytes(spiral_gpu_pack_server* S) {
    if (!S) return 0;
    // SURVEY.md 8d, pack form: 2^(nu1+nu2)*N*8 + 2^nu1*2*N*8 + 2^nu2*2*2*N*8 per trial
    const uint64_t n = kN;
    return (uint64_t)S->s.dim0 * S->s.num_per * n * 8 + (uint64_t)S->s.dim0 * 2 * n * 8 + (uint64_t)S->s.num_per * 4 * n * 8;
}

}  // extern "C"
