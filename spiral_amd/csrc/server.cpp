// The resident server of libspiral_gpu.so: the server object, its database calls and message intake, and the one-query answer path -- the stage
// API, the launch groups and the hipGraph cache that replays them (server halves of runConversionImproved / process_crtd_query /
// process_query_fast, reference src/spiral.cpp:2040-2406, 1584-1629).  Everything is kernel launches on one HIP stream; there is no CPU
// arithmetic path -- without a device every compute entry point fails.  The calls that carry several servers are in server_lanes.cpp, the
// stateless host-buffer seams in primitives.cpp; what the three share is declared in server_state.h and defined here.
#include "kv_host.h"
#include "records_host.h"
#include "server_state.h"

// hipGraphs the servers of this process have captured so far (get_option "graph_captures"): shows a replay is not a re-capture
std::atomic<uint64_t> spiral::host::g_captures{0};

namespace {

// digits per workgroup of a fold round with n_src source polynomials: as few workgroups as keep the chip busy (every
// workgroup repeats the inverse transform once), halved from ell until the round has about fold_blocks of them
uint32_t fold_dpb(const spiral_gpu_server* S, uint32_t n_src) {
    uint32_t dpb = S->s.ell;
    while (dpb > 1 && n_src * ((S->s.ell + dpb - 1) / dpb) < S->fold_blocks) dpb = (dpb + 1) / 2;
    return dpb;
}

int srv_alloc(spiral_gpu_server* S, DbImage* owners) {
    const spiral_gpu_params& p = S->p;
    const spiral_gpu_shape& s = S->s;
    S->img = owners ? owners->share() : DbImage::create(DbLayout::base(srv_np(S), S->dim0_shard), S);  // (a query lane: the owner's image)
    if (!S->img) return -1;
    S->n_cv = p.direct_upload ? s.n_bits : (1u << s.g);
    const size_t ngs = (size_t)p.nu2 * s.ell;
    const size_t half = s.num_per > 1 ? s.num_per / 2 : 1;
    auto layout = [&](Arena& a) {
        a.carve(S->w_left, (size_t)s.n_left * 2 * p.t_exp * kN);
        a.carve(S->w_right, (size_t)s.n_right * 2 * p.t_exp_right * kN);
        a.carve(S->w, (size_t)3 * 2 * p.t_conv * kN);
        a.carve(S->v, (size_t)3 * 2 * p.t_conv * kN);
        a.carve(S->query, (size_t)s.n_query_cts * 2 * kN);
        a.carve(S->cv, (size_t)S->n_cv * 2 * kN);
        if (!p.direct_upload) {
            a.carve(S->ex_raw, (size_t)S->n_cv * 2 * kN);
            a.carve(S->ex_g, expand_g_polys(s.g, p.t_exp, p.t_exp_right) * kN);
        }
        // conversion scratch: the ScalToMat sources/digits followed by the Regev->GSW ones, so both sets go through one lift
        // launch and one digit-transform launch
        a.carve(S->cv_raw, ((size_t)S->dim0_shard + ngs * 2) * kN);
        a.carve(S->cv_g, ((size_t)S->dim0_shard + ngs * 2) * p.t_conv * kN);
        a.carve(S->key, (size_t)p.nu2 * 3 * s.m2 * kN);
        a.carve(S->qs, (size_t)kN * S->dim0_shard * 6);  // 12 u32 per (z, j)
        a.carve(S->acc_own, (size_t)s.num_per * 6 * kN);
        a.carve(S->raw, (size_t)s.num_per * 6 * kN);
        a.carve(S->fold_d, half * 2 * s.m2 * 2 * kN);
        a.carve(S->fold_c, half * 6 * kN);
        a.carve(S->fold_c2, half * 6 * kN);
        a.carve(S->resp, (size_t)6 * kN);
    };
    if (alloc_carved(S->arena, S->pieces, layout)) return -1;
    HIP_OK(hipMemset(S->cv.p, 0, S->cv.words * sizeof(uint64_t)));
    S->gs_raw_p = S->cv_raw.p + (size_t)S->dim0_shard * kN;
    S->gs_chat_p = S->cv_g.p + (size_t)S->dim0_shard * p.t_conv * kN;
    S->acc = S->acc_own.p;
    return 0;
}

void srv_drop_graphs(spiral_gpu_server* S) {
    for (Captured& c : S->graphs) {
        if (c.exec) (void)hipGraphExecDestroy(c.exec);
        c = Captured{};
    }
}

void srv_free(spiral_gpu_server* S) {
    srv_drop_graphs(S);
    DbImage::drop(S->img, S);
    for (DevBuf* b : {&S->arena, &S->ex_raw2, &S->ex_g2, &S->cts_keep, &S->stage, &S->wire}) b->release();  // (what owns memory: the rest are pieces of the arena)
    S->wire_in.release();
    S->query_batch_in.release();
    S->xwork.release();
    for (auto& e : S->ev)
        if (e) (void)hipEventDestroy(e);
    if (S->ev_fork) (void)hipEventDestroy(S->ev_fork);
    if (S->ev_join) (void)hipEventDestroy(S->ev_join);
    if (S->ev_lane) (void)hipEventDestroy(S->ev_lane);
    if (S->side_stream) (void)hipStreamDestroy(S->side_stream);
    if (S->own_stream) (void)hipStreamDestroy(S->own_stream);
    S->side_stream = S->own_stream = nullptr;
    S->ev_fork = S->ev_join = S->ev_lane = nullptr;
    for (auto& e : S->ev) e = nullptr;
}

// The two ways client input gets into a server, in any form (message.h).  A null NTT-form buffer is refused with the previous message untouched; from
// the first write on nothing answers from a half-written buffer: the flags are cleared, and set again on success.
int take_pub_params(spiral_gpu_server* S, Form form, const MessageIn& in, const char* what) {
    if (enter(S)) return -1;
    const MessageLayout m = pub_params_layout(S->p, S->s);
    if (form == FORM_NTT && check_ntt_parts(m, in, what)) return -1;
    uint64_t* const dst[kMessageParts] = {S->w_left.p, S->w_right.p, S->w.p, S->v.p};
    S->have_pp = false;
    S->key_memo = KeyMemo{};
    if (ingest(form, IngestOn{S->stage, S->wire_in, S->tb, S->stream}, m, dst, in, what)) return -1;
    S->have_pp = true;
    return 0;
}
int take_query(spiral_gpu_server* S, Form form, const MessageIn& in, const char* what) {
    if (enter(S)) return -1;
    const MessageLayout m = query_layout(S->p, S->s);
    if (form == FORM_NTT && check_ntt_parts(m, in, what)) return -1;
    uint64_t* const dst[kMessageParts] = {S->query.p};
    S->have_query = S->have_records = false;
    if (ingest(form, IngestOn{S->stage, S->wire_in, S->tb, S->stream}, m, dst, in, what)) return -1;
    S->have_query = true;
    return 0;
}

int download_pk_as_ref(spiral_gpu_server* S, const uint64_t* pk, IndexMap map, uint64_t* host, size_t npolys) {
    if (npolys == 0) return 0;
    const size_t chunk = 4096;
    if (S->stage.words < std::min(npolys, chunk) * kRefNtt) {
        S->stage.release();
        if (S->stage.alloc(std::min(npolys, chunk) * kRefNtt)) return -1;
    }
    for (size_t done = 0; done < npolys; done += chunk) {
        const size_t n = std::min(chunk, npolys - done);
        IndexMap m = map;
        // shift the map by `done` polynomials: valid because chunk is a multiple of every inner we use
        m.off += (uint32_t)(done / map.inner) * map.outer_stride;
        launch_pk_to_ref(pk, S->stage.p, (uint32_t)n, m, S->stream);
        HIP_OK(hipMemcpyAsync(host + done * kRefNtt, S->stage.p, n * kRefNtt * sizeof(uint64_t), hipMemcpyDeviceToHost, S->stream));
        HIP_OK(hipStreamSynchronize(S->stream));
    }
    return 0;
}

int srv_create(const spiral_gpu_params* p, int device, uint32_t j_begin, uint32_t j_end, DbImage* owners, spiral_gpu_server** out, ColumnShard col = {}) {
    if (!p || !out) return fail("null argument");
    spiral_gpu_shape s;
    if (shape_of(p, &s)) return -1;
    if (j_end == 0 && j_begin == 0) j_end = s.dim0;
    if (j_begin >= j_end || j_end > s.dim0) return fail("bad first-dimension shard [%u, %u) of %u", j_begin, j_end, s.dim0);
    if (col.on && !column_shard_columns(s.num_per, col.rank, 1u << col.g_log)) return -1;
    HIP_OK(hipSetDevice(device));
    spiral_gpu_server* S = new spiral_gpu_server();
    S->p = *p;
    S->s = s;
    S->device = device;
    S->j0 = j_begin;
    S->j1 = j_end;
    S->dim0_shard = j_end - j_begin;
    S->col = col;
    if (col.on) S->fold_g_log = col.g_log;  // the last log2 G rounds are the root's (fold_root_batch): fixed for the server's life
    {  // the process-wide options as they stand now (spiral_gpu_set_option; SPIRAL_FOLD_PAIR / SPIRAL_SWEEP_MFMA give their initial values)
        const Options& o = options();
        S->fold_chain = o.fold_chain != 0;
        S->fold_pair = o.fold_pair != 0;
        S->fold_blocks = o.fold_blocks;
        S->sweep_mfma_min = o.sweep_mfma_min;
    }
    if (p->direct_upload || s.stopround == 0) {
        S->pos_stride = 1;
        S->pos_first = 0;
        S->pos_rest = s.dim0;
    } else {  // reorderFromStopround (src/spiral.cpp:2027-2036): even slots, then odd slots
        S->pos_stride = 2;
        S->pos_first = 0;
        S->pos_rest = 1;
    }
    if (tables_get(device, &S->tb) != 0) {
        delete S;
        return fail("twiddle table setup failed on device %d", device);
    }
    if (hipStreamCreate(&S->own_stream) != hipSuccess) {
        delete S;
        return fail("hipStreamCreate failed");
    }
    S->stream = S->own_stream;
    if (hipStreamCreateWithFlags(&S->side_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&S->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&S->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&S->ev_lane, hipEventDisableTiming) != hipSuccess) {
        srv_free(S);
        delete S;
        return fail("side stream setup failed");
    }
    for (auto& e : S->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            srv_free(S);
            delete S;
            return fail("hipEventCreate failed");
        }
    if (srv_alloc(S, owners)) {
        srv_free(S);
        delete S;
        return -1;
    }
    *out = S;
    return 0;
}

int read_db_region(spiral_gpu_server* S, uint32_t z_begin, uint32_t nz, uint32_t ii0, uint32_t n_ii, uint64_t* out) {
    if (!S || !out) return fail("null argument");
    if (refuse_column(S, "read_db_slots / read_db_columns (read its items with read_db_items)")) return -1;
    HIP_OK(hipSetDevice(S->device));
    if (z_begin >= kN || nz == 0 || nz > kN - z_begin) return fail("slot range out of bounds");
    if (n_ii == 0 || ii0 >= S->s.num_per || n_ii > S->s.num_per - ii0) return fail("column range out of bounds");
    const size_t per_z = (size_t)n_ii * 2 * S->dim0_shard * 2;
    const uint32_t zchunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(nz, ((size_t)256 << 20) / (per_z * sizeof(uint64_t))));
    DevBuf st;
    if (st.alloc(per_z * zchunk)) return -1;
    hipError_t e = hipSuccess;
    for (uint32_t z = 0; z < nz && e == hipSuccess; z += zchunk) {
        const uint32_t n = std::min(zchunk, nz - z);
        launch_db_read_slots(S->img->db.p, st.p, S->s.num_per, S->dim0_shard, z_begin + z, n, ii0, n_ii, S->stream, S->img->format == SPIRAL_GPU_DB_LIMBS);
        e = hipMemcpyAsync(out + (size_t)z * per_z, st.p, (size_t)n * per_z * sizeof(uint64_t), hipMemcpyDeviceToHost, S->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(S->stream);
    }
    st.release();
    if (e != hipSuccess) return fail("database read-back failed: %s", hipGetErrorString(e));
    return 0;
}
}  // namespace

// ---- what server_lanes.cpp uses too (declared in server_state.h) ----
namespace spiral {
namespace host {

// graphs hold a sweep kernel chosen for the image's form at capture time: drop them when the image has changed since
void srv_check_epoch(spiral_gpu_server* S) {
    const uint64_t e = S->img->epoch;
    if (S->epoch_seen != e) {
        srv_drop_graphs(S);
        S->epoch_seen = e;
    }
}

// the matrix-core sweep of n queries against the limb-plane image `limbs` (sweep_mfma.hip), and what a launch that could not be made reports
int sweep_mfma(const uint64_t* limbs, const uint32_t* const* qs, uint64_t* const* acc, uint32_t n, uint32_t np, uint32_t jm, uint32_t g_log, hipStream_t st,
               uint32_t k_log, uint32_t g_extra) {
    const hipError_t e = launch_sweep_mfma(limbs, qs, acc, n, np, jm, g_log, st, k_log, g_extra);
    return e == hipSuccess ? 0 : fail("the matrix-core sweep could not be launched: %s", hipGetErrorString(e));
}
// one query's sweep (all stages, or one stage of a pipelined sweep: packed image only) of S's image, in whichever form it is in, with S's query
// records into S's accumulators on S's stream: the one-query kernel forms (sweep_mfma_kernel<1>, NoLanes), never the batched helper
int sweep_one(spiral_gpu_server* S, int stage) {
    const DbImage* H = S->img;
    if (H->format == SPIRAL_GPU_DB_LIMBS) {
        if (stage >= 0 && S->sweep_k_log)
            return fail("a staged sweep needs the packed database image, and a batch has since converted it to limb planes: call set_sweep_stages again (or set option one_image = 0)");
        const uint32_t* qs[1] = {(const uint32_t*)S->qs.p};
        uint64_t* acc[1] = {S->acc};
        return sweep_mfma(H->db.p, qs, acc, 1, srv_np(S), 2 * S->dim0_shard, sweep_g_log(S), S->stream, S->sweep_k_log);
    }
    launch_sweep(H->db.p, (const uint32_t*)S->qs.p, S->acc, srv_np(S), 2 * S->dim0_shard, sweep_g_log(S), S->stream, S->sweep_k_log, stage);
    return 0;
}

// the fold needs the keys the forked conversion produces
int srv_join_side(spiral_gpu_server* S) {
    if (S->side_pending) {
        HIP_OK(hipStreamWaitEvent(S->stream, S->ev_join, 0));
        S->side_pending = false;
    }
    return 0;
}

// what a sweep or fold of servers[0 .. n) leaves: their accumulators or raw buffers overwritten (S->raw no longer the lift of S->acc)
void mark_raw_stale(spiral_gpu_server* const* servers, uint32_t n) {
    for (uint32_t b = 0; b < n; b++) servers[b]->raw_from_acc = false;
}
// ... and converting their queries before it: their records enqueued
void mark_swept(spiral_gpu_server* const* servers, uint32_t n) {
    for (uint32_t b = 0; b < n; b++) servers[b]->have_records = true;
    mark_raw_stale(servers, n);
}

// expandImproved for the query lanes `lanes` of S (lane 0 = S itself); rounds [r_begin, r_end) of it
int expand_lanes(spiral_gpu_server* S, const Lanes& lanes, uint32_t r_begin, uint32_t r_end) {
    const spiral_gpu_params& p = S->p;
    if (p.direct_upload || S->s.g == 0) {  // nothing to expand: the query ciphertexts are the expanded ones
        const size_t n = p.direct_upload ? (size_t)S->s.n_bits * 2 : 2;
        for (uint32_t q = 0; q < lanes.n && r_begin == 0; q++)
            HIP_OK(hipMemcpyAsync(S->cv.p + lanes.off[q], S->query.p + lanes.off[q], n * kPolyBytes, hipMemcpyDeviceToDevice, S->stream));
        return 0;
    }
    ExpandWork wk{S->ex_raw.p, S->ex_g.p};
    run_expand(S->tb, S->cv.p, S->s.g, p.t_exp, S->w_left.p, p.t_exp_right, S->w_right.p, S->s.ell * p.nu2, S->s.stopround, wk, S->stream, S->query.p, r_begin, r_end,
               S->ex_shard, 3, lanes);
    return 0;
}

// The conversion is: lift (INTT + CRT) of the source rows, t_conv gadget digits of each + forward transforms, then the two
// products.  WHAT selects the ScalToMat part (this shard's first-dimension ciphertexts, src/spiral.cpp:2230-2253), the
// Regev->GSW part (the nu2 further dimensions + fold keys, src/spiral.cpp:2315-2331, 2361-2386), or both with the lifts and
// the digit transforms of the two parts merged into one launch each (their scratch is contiguous).
int convert_part(spiral_gpu_server* S, uint32_t what, hipStream_t st, bool mark_split, const Lanes& lanes) {
    const spiral_gpu_params& p = S->p;
    const spiral_gpu_shape& s = S->s;
    const uint32_t ps = S->pos_stride, ngs = p.nu2 * s.ell;
    if (ngs == 0) what &= ~CONV_GSW;
    if (what & CONV_S2M) S->have_records = true;  // (eager runs; after a replayed graph the entry point that launched it sets it)
    const uint32_t n1 = (what & CONV_S2M) ? S->dim0_shard : 0, n2 = (what & CONV_GSW) ? 2 * ngs : 0;
    const IndexMap map1{1, 2 * ps, 2 * (S->j0 * ps + S->pos_first)};  // row 0 of ct pos(j0 + a)
    const IndexMap map2{2, 2 * ps, 2 * S->pos_rest};                   // rows 0, 1 of the nu2*ell GSW-bit cts
    uint64_t* raw = n1 ? S->cv_raw.p : S->gs_raw_p;
    launch_job(S->tb, lift_job(S->cv.p, raw, n1 + n2, {.src_map = n1 ? map1 : map2, .split = (n1 && n2) ? n1 : 0, .src_map2 = map2, .lanes = lanes}), st);
    // read only by the conversion products, which sum at most 2 * t_conv terms per accumulator
    launch_job(S->tb, gadget_digits_job(raw, n1 ? S->cv_g.p : S->gs_chat_p, n1 + n2, p.t_conv, 2 * p.t_conv, lanes), st);
    Scal2MatParams sp{};
    sp.w = S->w.p;
    sp.g = S->cv_g.p;
    sp.cv = S->cv.p;
    sp.cv_pos = IndexMap{1, ps, S->j0 * ps + S->pos_first};
    sp.out = S->keep_cts ? S->cts_keep.p : nullptr;
    sp.qs = (uint32_t*)S->qs.p;
    sp.t_conv = p.t_conv;
    sp.count = S->dim0_shard;
    sp.jm_total = 2 * S->dim0_shard;
    sp.j_base = 0;
    sp.lanes = lanes;
    GswParams gp{};
    gp.w = S->w.p;
    gp.v = S->v.p;
    gp.chat = S->gs_chat_p;
    gp.cv = S->cv.p;
    gp.cv_pos = IndexMap{1, ps, S->pos_rest};
    gp.gsw = S->key.p;  // the GSW matrices ARE the fold key: written once (the reference also keeps Q_neg = G2 - Q, src/spiral.cpp:2361-2379: derived here where a round needs it)
    gp.t_conv = p.t_conv;
    gp.ell = s.ell;
    gp.dims = p.nu2;
    gp.key = nullptr;
    gp.lanes = lanes;
    if (what == CONV_BOTH && !mark_split) {  // the two products are independent: one launch
        launch_convert_products(sp, gp, st);
        return 0;
    }
    if (what & CONV_S2M) launch_scal2mat(sp, st);
    if (mark_split) HIP_OK(hipEventRecord(S->ev[7], st));  // ScalToMat | RegevToGSW split of the reference summary
    if (what & CONV_GSW) launch_regev_to_gsw(gp, st);
    return 0;
}

// expand + convert as the launch groups run them.  (Tried: forking the Regev->GSW conversion onto the side stream after
// round `stopround`, where the odd-index side of the expansion is complete, to run beside the remaining even-only rounds.
// Inside a hipGraph the second branch costs far more than the 26 us it hides -- expand + convert went from 340 to 415 us --
// so the group stays one chain.)  Every caller has checked that the query and the public parameters are set.
int expand_convert(spiral_gpu_server* S) {
    if (expand_lanes(S, Lanes{})) return -1;
    return convert_part(S, CONV_BOTH, S->stream, !S->use_graphs);  // (eager: the two products apart, with the summary's event between them)
}

// the response modulus switch of the folded ciphertexts: row 0 -> q', rows 1.. -> 4*p_db (src/spiral.cpp:1441-1447)
int finish_lanes(spiral_gpu_server* S, const Lanes& lanes) {
    launch_rescale2(S->raw.p, S->resp.p, 2 * kN, 6 * kN, kQ, S->s.qprime, 4 * S->p.p_db, S->stream, lanes);
    return 0;
}
// foldOneFurtherDimension rounds [d0, d0 + rounds) on np0 ciphertexts (src/spiral.cpp:1349-1410; the arguments: server_state.h FoldJob); the
// result is left CRT-lifted at the head of S->raw
int run_fold_rounds(spiral_gpu_server* S, const FoldJob& job) {
    const spiral_gpu_shape& s = S->s;
    const Lanes& lanes = job.lanes;
    S->raw_from_acc = false;  // S->raw ends up holding the folded ciphertext
    uint32_t np = job.np0;
    const uint64_t *src_pk = job.src_pk, *raw_addend = job.raw_addend;
    bool pre_reduce = job.pre_reduce;
    auto lift = [&](uint32_t npolys) {  // src_pk -> S->raw
        launch_job(S->tb, lift_job(src_pk, S->raw.p, npolys, {.pre_reduce = pre_reduce, .lanes = lanes}), S->stream);
        src_pk = nullptr;
    };
    auto digits = [&](FwdLoad ld, uint32_t n_src, uint32_t mac_terms) {  // S->raw -> the round's operand S->fold_d
        launch_job(S->tb, fold_digits_job(ld, S->raw.p, S->fold_d.p, n_src, s.ell, np, mac_terms, lanes), S->stream);
    };
    uint64_t* out_pk = S->fold_c.p;
    for (uint32_t d = job.d0; d < job.d0 + job.rounds; d++) {
        np /= 2;
        const uint32_t n_src = 2 * np * 6;
        const uint64_t* key = S->key.p + (size_t)d * 3 * s.m2 * kN;
        if (src_pk == out_pk) out_pk = out_pk == S->fold_c.p ? S->fold_c2.p : S->fold_c.p;  // the pair form's product reads its source
        const bool from_raw = !src_pk && raw_addend && S->fold_pair && fold_pair_exact(s.ell);  // lifted already, transform-domain words at hand
        if (from_raw || (src_pk && S->fold_chain && S->fold_pair && fold_pair_exact(s.ell))) {
            // wide round: the lift of all 2 np ciphertexts as one full-occupancy launch, then one digit-difference transform per
            // workgroup (LD_SDIFF) -- no inverse transform is repeated, both kernels run 8 workgroups per CU
            const uint64_t* low = from_raw ? raw_addend : src_pk;
            if (!from_raw) lift(n_src);
            raw_addend = nullptr;
            digits(LD_SDIFF, n_src / 2, 3 * s.ell + 1);  // fold_mac sums m2 = 3 ell products and the addend per accumulator
            launch_fold_mac(key, S->fold_d.p, out_pk, s.m2, np, S->stream, s.m2, low, lanes);
        } else {
            if (src_pk && S->fold_chain) {
                FoldChainParams cp{};
                cp.src = src_pk;
                cp.dst = S->fold_d.p;
                cp.ell = s.ell;
                cp.bits = get_bits_per(s.ell);
                cp.fold_np = np;
                cp.pre_reduce = pre_reduce ? 1 : 0;
                cp.dpb = fold_dpb(S, n_src);
                cp.lazy_out = lazy_ok(6 * s.ell) ? 1 : 0;  // fold_mac sums 2 * m2 = 6 ell products per accumulator
                cp.lanes = lanes;
                launch_fold_chain(S->tb, cp, n_src, S->stream);
            } else {
                if (src_pk) lift(n_src);
                digits(LD_SDIGIT, n_src, 0);
            }
            launch_fold_mac_two(key, S->fold_d.p, out_pk, s.m2, s.ell, get_bits_per(s.ell), np, S->stream, lanes);  // the reference's two products, Q_neg derived
        }
        src_pk = out_pk;
        pre_reduce = false;
    }
    if (src_pk) lift(np * 6);
    // (the switch is its own launch: fused into the 6-workgroup lift it serialises 8 coefficients per thread and is slower)
    return job.finish ? finish_lanes(S, lanes) : 0;
}

}  // namespace host
}  // namespace spiral

extern "C" {

int spiral_gpu_server_create(const spiral_gpu_params* p, int device, uint32_t j_begin, uint32_t j_end, spiral_gpu_server** out) {
    return srv_create(p, device, j_begin, j_end, nullptr, out);
}

int spiral_gpu_server_create_column_shard(const spiral_gpu_params* p, int device, uint32_t rank, uint32_t n_ranks, spiral_gpu_server** out) {
    if (!p || !out) return fail("null argument");
    spiral_gpu_shape s;
    if (shape_of(p, &s)) return -1;
    if (!column_shard_columns(s.num_per, rank, n_ranks)) return -1;
    return srv_create(p, device, 0, 0, nullptr, out, ColumnShard{true, rank, ceil_log2(n_ranks)});
}

int spiral_gpu_server_create_lane(spiral_gpu_server* owner, spiral_gpu_server** out) {
    if (!owner || !out) return fail("null argument");
    if (owner->img->owner != owner) return fail("the owner does not own its database image");
    if (!owner->img->loaded) return fail("the owner has no database loaded");
    return srv_create(&owner->p, owner->device, owner->j0, owner->j1, owner->img, out, owner->col);  // (a column shard's lane is one of the same rank)
}

void spiral_gpu_server_destroy(spiral_gpu_server* S) {
    if (!S) return;
    (void)hipSetDevice(S->device);
    (void)hipDeviceSynchronize();
    srv_free(S);  // (an image its lanes still sweep lives on until the last of them goes)
    delete S;
}

int spiral_gpu_server_set_stream(spiral_gpu_server* S, void* hip_stream) {
    if (!S) return fail("null server");
    S->stream = hip_stream ? (hipStream_t)hip_stream : S->own_stream;
    return 0;
}

void* spiral_gpu_server_get_stream(spiral_gpu_server* S) { return S ? (void*)S->stream : nullptr; }

int spiral_gpu_server_use_graphs(spiral_gpu_server* S, int on) {
    if (!S) return fail("null server");
    S->use_graphs = on != 0;
    if (!on) srv_drop_graphs(S);
    return 0;
}

int spiral_gpu_server_load_db(spiral_gpu_server* S, const uint64_t* database) {
    if (!S || !database) return fail("null argument");
    if (S->img->owner != S) return fail("this server sweeps another server's database image (share_db): load it through the owner");
    HIP_OK(hipSetDevice(S->device));
    // stage the reference-layout database one z-slab group at a time and re-lay the shard
    const size_t per_z_ref = (size_t)S->s.num_per * 2 * S->s.dim0 * 2;
    const size_t stage_bytes = options().db_stage_bytes;  // (tests force several staging passes)
    const uint32_t zchunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(kN, stage_bytes / (per_z_ref * sizeof(uint64_t))));
    DevBuf st;
    if (st.alloc(per_z_ref * zchunk)) return -1;
    S->img->begin_rewrite();
    for (uint32_t z = 0; z < kN; z += zchunk) {
        const uint32_t nz = std::min(zchunk, kN - z);
        if (hipMemcpyAsync(st.p, database + (size_t)z * per_z_ref, (size_t)nz * per_z_ref * sizeof(uint64_t), hipMemcpyHostToDevice, S->stream) !=
            hipSuccess) {
            st.release();
            return fail("database upload failed");
        }
        // (a column shard keeps the reference's columns rank + G k: its own num_per is L, the slab's L G)
        launch_db_relayout(st.p, S->img->db.p, srv_np(S), S->s.dim0, S->j0, S->dim0_shard, z, nz, S->stream, S->col.rank, col_ranks(S));
        if (hipStreamSynchronize(S->stream) != hipSuccess) {
            st.release();
            return fail("database relayout failed");
        }
    }
    st.release();
    S->img->finish_load();
    return 0;
}

int spiral_gpu_server_gen_db(spiral_gpu_server* S, uint64_t seed) {
    if (!S) return fail("null server");
    if (S->img->owner != S) return fail("this server sweeps another server's database image (share_db): load it through the owner");
    HIP_OK(hipSetDevice(S->device));
    // (a column shard: local item l is the database's item rank + G l, in an image of L columns)
    FwdJob encode = db_encode_job(LD_DBGEN, ST_DB, S->img->db.p, S->p.p_db,
                                  {.num_per = srv_np(S), .dim0_shard = S->dim0_shard, .j0 = S->j0, .item_stride = col_ranks(S), .item_off = S->col.rank});
    const uint64_t items = (uint64_t)S->dim0_shard * srv_np(S), first = (uint64_t)S->j0 * srv_np(S);
    const uint64_t chunk = 1u << 16;  // items per launch (4 polynomials each)
    S->img->begin_rewrite();
    for (uint64_t done = 0; done < items; done += chunk) {
        db_encode_seeded(encode, seed, first + done, (uint32_t)(std::min(chunk, items - done) * 4));
        launch_job(S->tb, encode, S->stream);
    }
    HIP_OK(hipStreamSynchronize(S->stream));
    S->img->finish_load();
    return 0;
}

int spiral_gpu_server_load_db_items(spiral_gpu_server* S, const void* items, uint32_t coeff_bits, uint64_t first_item, uint64_t n_items) {
    if (!S) return fail("null server");
    if (S->img->owner != S) return fail("this server sweeps another server's database image (share_db): load it through the owner");
    HIP_OK(hipSetDevice(S->device));
    const uint64_t total = (uint64_t)S->s.dim0 * S->s.num_per;
    if (first_item > total || n_items > total - first_item) return fail("items [%llu, +%llu) outside the database of %llu", (unsigned long long)first_item,
                                                                         (unsigned long long)n_items, (unsigned long long)total);
    // item i lives at (ii = i % num_per, j = i / num_per): this shard holds the items of j in [j0, j1)
    const uint64_t lo = std::max<uint64_t>(first_item, (uint64_t)S->j0 * S->s.num_per), hi = std::min<uint64_t>(first_item + n_items, (uint64_t)S->j1 * S->s.num_per);
    const uint64_t G = col_ranks(S), g = S->col.rank;
    FwdJob encode = db_encode_job(LD_DBGEN, ST_DB, S->img->db.p, S->p.p_db,
                                  {.num_per = srv_np(S), .dim0_shard = S->dim0_shard, .j0 = S->j0, .item_stride = (uint32_t)G, .item_off = (uint32_t)g});
    // a partial load scatters packed words into the image: an image a batch has converted to limb planes goes back to the packed form first
    if (S->img->begin_partial(S->stream)) return -1;
    if (ingest_items(items, coeff_bits, first_item, lo, hi, 4, S->p.p_db, S->stream, [&](const uint8_t* d_items, uint32_t* d_err, uint64_t first, uint64_t n) {
            // a column shard keeps every G-th item of the staged run, the ids = g (mod G): local items [l0, l1), read at item stride G
            const uint64_t l0 = (first + G - 1 - g) / G, l1 = (first + n + G - 1 - g) / G;  // (g < G: no underflow; G = 1: [first, first + n))
            if (l0 >= l1) return;
            S->img->dirty();
            db_encode_staged(encode, d_items, coeff_bits, d_err, first, (uint32_t)((l1 - l0) * 4), l0);
            launch_job(S->tb, encode, S->stream);
        }))
        return -1;
    S->img->finish_load();
    return 0;
}

// In place, in the image's current form, on the holder's stream (include/spiral_gpu.h): no conversion, no new epoch -- the image keeps its address
// and its form, so captured graphs replay unchanged and read the new items.
namespace {
// what the update calls need to keep a tracked image's fingerprint current (t null: not tracked): local item (j, ii) is database item
// ((j0 + j) L + ii) G + g -- fingerprint_items' map
void track_ctx(const spiral_gpu_server* S, FpTrackCtx& c) {
    if (!S->img->trk.on) return;
    c.t = &S->img->trk;
    const uint64_t G = col_ranks(S), g = S->col.on ? S->col.rank : 0u, L = srv_np(S), j0 = S->j0;
    c.db_index = [=](uint32_t j, uint32_t ii) { return ((j0 + j) * L + ii) * G + g; };
}
}  // namespace
int spiral_gpu_server_update_db_items(spiral_gpu_server* S, const void* items, uint32_t coeff_bits, const uint64_t* item_ids, uint64_t n) {
    if (!S) return fail("null server");
    if (S->img->owner != S) return fail("this server sweeps another server's database image (share_db or a lane): update it through the owner");
    if (!S->img->loaded) return fail("no database loaded");
    HIP_OK(hipSetDevice(S->device));
    const uint64_t np = S->s.num_per;
    if (check_update_ids(items, item_ids, n, (uint64_t)S->s.dim0 * np)) return -1;
    std::vector<UpdateItem> sel;  // the ids of this shard's j-range (a column shard: of its columns, (j, ii) at (j, ii / G))
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t j = item_ids[k] / np;
        const uint32_t ii = (uint32_t)(item_ids[k] % np);
        if (j >= S->j0 && j < S->j1 && holds_column(S, ii)) sel.push_back(UpdateItem{k, (uint32_t)(j - S->j0), ii >> col_g_log(S)});
    }
    FpTrackCtx trk;
    track_ctx(S, trk);
    return update_items(S->img->upd, S->tb, S->stream, items, coeff_bits, S->p.p_db, sel, S->img->update_target(), trk.t ? &trk : nullptr);
}

// The items back as plaintexts, in the load_db_items layout, from the image in its current form (include/spiral_gpu.h): any server that references a
// loaded image, on its own stream; a shard writes the items of its j-range and leaves the other bytes of `items` alone
int spiral_gpu_server_read_db_items(spiral_gpu_server* S, void* items, uint32_t coeff_bits, uint64_t first_item, uint64_t n_items) {
    if (enter(S)) return -1;
    if (!items) return fail("null argument");
    if (!S->img->loaded) return fail("no database loaded");
    const uint64_t np = S->s.num_per, total = (uint64_t)S->s.dim0 * np;
    if (first_item > total || n_items > total - first_item)
        return fail("items [%llu, +%llu) outside the database of %llu", (unsigned long long)first_item, (unsigned long long)n_items, (unsigned long long)total);
    if (check_export_width(coeff_bits, S->p.p_db)) return -1;
    const uint64_t lo = std::max<uint64_t>(first_item, S->j0 * np), hi = std::min<uint64_t>(first_item + n_items, S->j1 * np);
    if (lo >= hi) return 0;
    if (S->col.on && S->col.g_log) {  // its items lie G apart in `items`: the table form, each to its own place, the bytes between left alone
        const uint64_t G = col_ranks(S), g = S->col.rank, L = srv_np(S);
        std::vector<ExportItem> sel;
        sel.reserve((size_t)((hi - lo) / G + 1));
        for (uint64_t i = lo + (g + G - lo % G) % G; i < hi; i += G) sel.push_back(ExportItem{i - first_item, (uint32_t)(i / np), (uint32_t)((i / G) % L)});
        return export_items(S->xwork, S->tb, S->stream, items, coeff_bits, S->p.p_db, S->img->export_source(), 0, 0, 0, &sel,
                            [&](uint64_t pos) { return first_item + pos; });
    }
    return export_items(S->xwork, S->tb, S->stream, items, coeff_bits, S->p.p_db, S->img->export_source(), lo - S->j0 * np, hi - lo, lo - first_item, nullptr,
                        [&](uint64_t pos) { return first_item + pos; });
}
int spiral_gpu_server_read_db_items_at(spiral_gpu_server* S, void* items, uint32_t coeff_bits, const uint64_t* item_ids, uint64_t n) {
    if (enter(S)) return -1;
    if (!items || !item_ids) return fail("null argument");
    if (!S->img->loaded) return fail("no database loaded");
    const uint64_t np = S->s.num_per, total = (uint64_t)S->s.dim0 * np;
    for (uint64_t k = 0; k < n; k++)
        if (item_ids[k] >= total) return fail("item id %llu outside the database of %llu items", (unsigned long long)item_ids[k], (unsigned long long)total);
    if (check_export_width(coeff_bits, S->p.p_db)) return -1;
    std::vector<ExportItem> sel;  // the ids of this shard's j-range
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t j = item_ids[k] / np;
        const uint32_t ii = (uint32_t)(item_ids[k] % np);
        if (j >= S->j0 && j < S->j1 && holds_column(S, ii)) sel.push_back(ExportItem{k, (uint32_t)(j - S->j0), ii >> col_g_log(S)});
    }
    return export_items(S->xwork, S->tb, S->stream, items, coeff_bits, S->p.p_db, S->img->export_source(), 0, 0, 0, &sel, [&](uint64_t pos) { return item_ids[pos]; });
}

// The content fingerprint of items of the image this server references, computed from the image in its current form (include/spiral_gpu.h
// "Fingerprints"): read_db_items' contract with 8 bytes per item, or 8 bytes in all, in place of the item stream.  A shard returns its partial sums.
namespace {
static int fingerprint_enter(spiral_gpu_server* S, const uint64_t* key, const uint64_t* per_item, const uint64_t* combined) {
    if (enter(S)) return -1;
    if (!key) return fail("null argument");
    if (!per_item && !combined) return fail("per_item and combined are both null: nothing to compute");
    if (!S->img->loaded) return fail("no database loaded");
    return 0;
}
}  // namespace
namespace {
// what this server holds of the database items [first_item, + n_items), as fingerprint_items' range form
void fingerprint_range_sel(const spiral_gpu_server* S, uint64_t first_item, uint64_t n_items, FingerprintSel& fs) {
    // database item i of column shard g of G is local item i / G of the shard's columns (read_db_items' map: j = i / np, column (i / G) % L, np = L G),
    // so the items this server holds of a range are a range of local items, G apart in the database
    const uint64_t np = S->s.num_per, G = col_ranks(S), g = S->col.on ? S->col.rank : 0u, L = srv_np(S);
    const uint64_t lo = std::max<uint64_t>(first_item, S->j0 * np), hi = std::min<uint64_t>(first_item + n_items, S->j1 * np);
    if (lo < hi) {
        const uint64_t u0 = (lo + G - 1 - g) / G, u1 = (hi + G - 1 - g) / G;  // i = u G + g in [lo, hi)
        if (u0 < u1) {
            fs.first_l = u0 - S->j0 * L;
            fs.n = u1 - u0;
            fs.idx0 = u0 * G + g;
            fs.stride = G;
            fs.pos0 = fs.idx0 - first_item;
        }
    }
}
int fingerprint_check_range(const spiral_gpu_server* S, uint64_t first_item, uint64_t n_items) {
    const uint64_t total = (uint64_t)S->s.dim0 * S->s.num_per;
    if (first_item > total || n_items > total - first_item)
        return fail("items [%llu, +%llu) outside the database of %llu", (unsigned long long)first_item, (unsigned long long)n_items, (unsigned long long)total);
    return 0;
}
}  // namespace
int spiral_gpu_server_fingerprint_items(spiral_gpu_server* S, const uint64_t* key, uint64_t first_item, uint64_t n_items, uint64_t* per_item, uint64_t* combined) {
    if (fingerprint_enter(S, key, per_item, combined)) return -1;
    const uint64_t np = S->s.num_per, total = (uint64_t)S->s.dim0 * np;
    if (first_item > total || n_items > total - first_item)
        return fail("items [%llu, +%llu) outside the database of %llu", (unsigned long long)first_item, (unsigned long long)n_items, (unsigned long long)total);
    FingerprintSel fs;
    fingerprint_range_sel(S, first_item, n_items, fs);
    return fingerprint_items(S->xwork, S->tb, S->stream, key, S->p.p_db, S->img->export_source(), 0, 4, 0, fs, n_items, per_item, combined);
}
int spiral_gpu_server_fingerprint_items_at(spiral_gpu_server* S, const uint64_t* key, const uint64_t* item_ids, uint64_t n, uint64_t* per_item, uint64_t* combined) {
    if (fingerprint_enter(S, key, per_item, combined)) return -1;
    if (!item_ids) return fail("null argument");
    if (n > 0xFFFFFFFFull) return fail("at most 2^32 - 1 items per fingerprint call");
    const uint64_t np = S->s.num_per, total = (uint64_t)S->s.dim0 * np;
    for (uint64_t k = 0; k < n; k++)
        if (item_ids[k] >= total) return fail("item id %llu outside the database of %llu items", (unsigned long long)item_ids[k], (unsigned long long)total);
    std::vector<ExportItem> sel;  // the ids this shard holds, as read_db_items_at
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t j = item_ids[k] / np;
        const uint32_t ii = (uint32_t)(item_ids[k] % np);
        if (j >= S->j0 && j < S->j1 && holds_column(S, ii)) sel.push_back(ExportItem{k, (uint32_t)(j - S->j0), ii >> col_g_log(S)});
    }
    FingerprintSel fs;
    fs.sel = &sel;
    fs.ids = item_ids;
    return fingerprint_items(S->xwork, S->tb, S->stream, key, S->p.p_db, S->img->export_source(), 0, 4, 0, fs, n, per_item, combined);
}

// ---- tracked fingerprints (include/spiral_gpu.h "Fingerprints", Tracked; host_common.h) -----------------------------------------------------------
int spiral_gpu_server_fingerprint_track(spiral_gpu_server* S, const uint64_t* key, const uint64_t* poly_sums) {
    if (enter(S)) return -1;
    if (!key) return fail("null argument");
    if (S->img->owner != S) return fail("this server sweeps another server's database image (share_db or a lane): track its fingerprint through the owner");
    if (!S->img->loaded) return fail("no database loaded");
    const uint64_t G = col_ranks(S), g = S->col.on ? S->col.rank : 0u, L = srv_np(S);
    const FpTrackGeom geom{(uint64_t)S->dim0_shard * L, (uint64_t)S->j0 * L * G + g, G, 4u, 0u};
    return fingerprint_track(S->img->trk, S->xwork, S->tb, S->stream, key, S->p.p_db, S->img->export_source(), 0, geom, poly_sums);
}
int spiral_gpu_server_fingerprint_untrack(spiral_gpu_server* S) {
    if (enter(S)) return -1;
    if (S->img->owner != S) return fail("this server sweeps another server's database image (share_db or a lane): untrack through the owner");
    HIP_OK(hipStreamSynchronize(S->stream));  // (an update's apply launch may still write the table)
    S->img->trk.release();
    return 0;
}
int spiral_gpu_server_fingerprint_tracked(spiral_gpu_server* S, uint64_t* key_out, uint64_t* combined, uint64_t* n_updates) {
    if (enter(S)) return -1;
    return fingerprint_tracked(S->img->trk, S->stream, key_out, combined, n_updates);
}
int spiral_gpu_server_fingerprint_tracked_polys(spiral_gpu_server* S, uint64_t first_item, uint64_t n_items, uint64_t* poly_sums) {
    if (enter(S)) return -1;
    if (fingerprint_check_range(S, first_item, n_items)) return -1;
    FingerprintSel fs;
    fingerprint_range_sel(S, first_item, n_items, fs);
    return fingerprint_tracked_polys(S->img->trk, S->stream, fs.first_l, fs.n, fs.pos0, fs.stride, n_items, poly_sums);
}
int spiral_gpu_server_fingerprint_scrub(spiral_gpu_server* S, uint64_t first_item, uint64_t n_items, uint64_t* n_bad, uint64_t* first_bad_item, uint32_t* first_bad_poly) {
    if (enter(S)) return -1;
    if (!n_bad) return fail("null argument");
    if (!S->img->loaded) return fail("no database loaded");
    if (fingerprint_check_range(S, first_item, n_items)) return -1;
    FingerprintSel fs;
    fingerprint_range_sel(S, first_item, n_items, fs);
    return fingerprint_scrub(S->img->trk, S->xwork, S->tb, S->stream, S->p.p_db, S->img->export_source(), 0, 0, fs, n_bad, first_bad_item, first_bad_poly);
}

// ---- records (include/spiral_gpu.h "Records"; records_host.h, records.hip) ---------------------------------------------------------------------
namespace {
// the layout and this instance's chunk for a record call
struct RecordCall {
    spiral_gpu_record_layout l;
    RecordChunk chunk;
};
int record_call(const spiral_gpu_server* S, uint64_t record_bytes, uint32_t instance, RecordCall* rc) {
    if (record_layout(&S->p, record_bytes, &rc->l)) return -1;
    return record_chunk(rc->l, record_bytes, instance, &rc->chunk);
}
// record r as a piece of this server's image, when the server holds its item (a j-shard: its rows; a column shard: its columns, ii at ii / G)
bool record_piece(const spiral_gpu_server* S, const RecordCall& rc, uint64_t pos, uint64_t r, RecordPiece* pc) {
    const uint64_t item = r / rc.l.per_item, j = item / S->s.num_per;
    const uint32_t ii = (uint32_t)(item % S->s.num_per);
    if (j < S->j0 || j >= S->j1 || !holds_column(S, ii)) return false;
    *pc = RecordPiece{pos, (uint32_t)(j - S->j0), ii >> col_g_log(S), (uint32_t)((r % rc.l.per_item) * (rc.l.instances == 1 ? rc.chunk.len : 0)), (uint32_t)rc.chunk.len};
    return true;
}
}  // namespace

int spiral_gpu_record_layout_of(const spiral_gpu_params* p, uint64_t record_bytes, spiral_gpu_record_layout* out) { return record_layout(p, record_bytes, out); }

// Through load_db_items: the records repacked into items on the host, padding zero (not a hot path); bytes that need no repacking go as they are
int spiral_gpu_server_load_records(spiral_gpu_server* S, const void* records, uint64_t record_bytes, uint32_t instance, uint64_t first_record, uint64_t n_records) {
    if (!S) return fail("null server");
    RecordCall rc;
    if (record_call(S, record_bytes, instance, &rc)) return -1;
    if (first_record > rc.l.capacity || n_records > rc.l.capacity - first_record)
        return fail("records [%llu, +%llu) outside the database of %llu", (unsigned long long)first_record, (unsigned long long)n_records, (unsigned long long)rc.l.capacity);
    if (first_record % rc.l.per_item || n_records % rc.l.per_item)
        return fail("records [%llu, +%llu) do not start and end at a multiple of the %llu records of an item", (unsigned long long)first_record,
                    (unsigned long long)n_records, (unsigned long long)rc.l.per_item);
    if (n_records && !records) return fail("null argument");
    const uint32_t w = rc.l.coeff_bits, cb = (1ull << w) < S->p.p_db ? w + 1 : w;  // (load_db_items wants a width that holds every value below p_db)
    const uint64_t first_item = first_record / rc.l.per_item, n_items = n_records / rc.l.per_item;
    const uint8_t* src = static_cast<const uint8_t*>(records);
    if (cb == w && rc.l.per_item * record_bytes == rc.l.item_bytes) return spiral_gpu_server_load_db_items(S, src, w, first_item, n_items);
    const uint64_t pass = std::max<uint64_t>(1, std::min<uint64_t>(options().db_stage_bytes / (1024ull * cb), 1u << 12));  // items repacked at a time
    std::vector<uint8_t> stream, wide;
    for (uint64_t done = 0; done < n_items; done += pass) {
        const uint64_t cnt = std::min(pass, n_items - done);
        stream.assign((size_t)(cnt * rc.l.item_bytes), 0);
        for (uint64_t i = 0; i < cnt; i++) {
            const uint64_t r0 = (done + i) * rc.l.per_item;  // (relative to first_record)
            if (rc.l.instances == 1)
                memcpy(stream.data() + i * rc.l.item_bytes, src + r0 * record_bytes, (size_t)(rc.l.per_item * record_bytes));
            else
                memcpy(stream.data() + i * rc.l.item_bytes, src + r0 * record_bytes + rc.chunk.first, (size_t)rc.chunk.len);
        }
        const uint8_t* items = stream.data();
        if (cb != w) {
            wide.assign((size_t)(cnt * 1024ull * cb), 0);
            widen_coeffs(stream.data(), wide.data(), (size_t)(cnt * 4 * kN), w, cb);
            items = wide.data();
        }
        if (spiral_gpu_server_load_db_items(S, items, cb, first_item + done, cnt)) return -1;
    }
    return 0;
}

// In place, in the image's current form, on the holder's stream: update_db_items' contract at a record's granularity
int spiral_gpu_server_update_records(spiral_gpu_server* S, const void* records, uint64_t record_bytes, uint32_t instance, const uint64_t* record_ids, uint64_t n) {
    if (!S) return fail("null server");
    if (S->img->owner != S) return fail("this server sweeps another server's database image (share_db or a lane): update it through the owner");
    RecordCall rc;
    if (record_call(S, record_bytes, instance, &rc)) return -1;
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
    std::vector<RecordPiece> pieces;
    RecordPiece pc;
    for (uint64_t k = 0; k < n; k++)
        if (record_piece(S, rc, k, record_ids[k], &pc)) pieces.push_back(pc);
    FpTrackCtx trk;
    track_ctx(S, trk);
    return update_record_pieces(S->img->upd, S->tb, S->stream, static_cast<const uint8_t*>(records), record_bytes, rc.chunk, rc.l.coeff_bits, S->p.p_db, pieces,
                                S->img->update_target(), S->img->export_source(), [&](uint64_t pos) { return record_ids[pos]; }, RecordTrials{},
                                trk.t ? &trk : nullptr);
}

// The records back, from the image in its current form: any server that references a loaded image, on its own stream; a shard writes the records it
// holds and leaves the other bytes of `records` alone
int spiral_gpu_server_read_records(spiral_gpu_server* S, void* records, uint64_t record_bytes, uint32_t instance, uint64_t first_record, uint64_t n_records) {
    if (enter(S)) return -1;
    RecordCall rc;
    if (record_call(S, record_bytes, instance, &rc)) return -1;
    if (!records) return fail("null argument");
    if (!S->img->loaded) return fail("no database loaded");
    if (first_record > rc.l.capacity || n_records > rc.l.capacity - first_record)
        return fail("records [%llu, +%llu) outside the database of %llu", (unsigned long long)first_record, (unsigned long long)n_records, (unsigned long long)rc.l.capacity);
    // whole items of a layout without padding, at a width the export takes: the range export as it is
    if (rc.l.per_item * record_bytes == rc.l.item_bytes && first_record % rc.l.per_item == 0 && n_records % rc.l.per_item == 0 && (1ull << rc.l.coeff_bits) == S->p.p_db)
        return spiral_gpu_server_read_db_items(S, records, rc.l.coeff_bits, first_record / rc.l.per_item, n_records / rc.l.per_item);
    return read_record_pieces(S->xwork, S->tb, S->stream, static_cast<uint8_t*>(records), record_bytes, rc.chunk, rc.l.coeff_bits, S->p.p_db, n_records,
                              [&](uint64_t k, RecordPiece* pc) { return record_piece(S, rc, k, first_record + k, pc); }, S->img->export_source(),
                              [&](uint64_t pos) { return first_record + pos; });
}
int spiral_gpu_server_read_records_at(spiral_gpu_server* S, void* records, uint64_t record_bytes, uint32_t instance, const uint64_t* record_ids, uint64_t n) {
    if (enter(S)) return -1;
    RecordCall rc;
    if (record_call(S, record_bytes, instance, &rc)) return -1;
    if (n && (!records || !record_ids)) return fail("null argument");
    if (!S->img->loaded) return fail("no database loaded");
    for (uint64_t k = 0; k < n; k++)
        if (record_ids[k] >= rc.l.capacity)
            return fail("record id %llu outside the database of %llu records", (unsigned long long)record_ids[k], (unsigned long long)rc.l.capacity);
    return read_record_pieces(S->xwork, S->tb, S->stream, static_cast<uint8_t*>(records), record_bytes, rc.chunk, rc.l.coeff_bits, S->p.p_db, n,
                              [&](uint64_t k, RecordPiece* pc) { return record_piece(S, rc, k, record_ids[k], pc); }, S->img->export_source(),
                              [&](uint64_t pos) { return record_ids[pos]; });
}

// ---- keyed records (include/spiral_gpu.h "Keyed records"; kv_host.h, kv.hip) --------------------------------------------------------------------
namespace {
// how every keyed call opens: the layout, and an unsharded image (both candidates of a key are probed in one place)
int kv_call(const spiral_gpu_server* S, const char* what, uint64_t value_bytes, spiral_gpu_kv_layout* l) {
    if (kv_layout(&S->p, value_bytes, l)) return -1;
    if (S->col.on) return fail("%s: this server is a column shard: keyed records need the whole image in one place (both candidate buckets of a key are probed together)", what);
    if (S->j0 != 0 || S->j1 != S->s.dim0) return fail("%s: this server is a j-shard (rows [%u, %u) of %u): keyed records need the whole image in one place (both candidate buckets of a key are probed together)", what, S->j0, S->j1, S->s.dim0);
    return 0;
}
// n whole items of the record layout's stream (w bits per coefficient) through load_db_items, widened by a bit where p_db is no power of two
int load_item_stream(spiral_gpu_server* S, const uint8_t* stream, uint32_t w, uint64_t item_bytes, uint64_t first_item, uint64_t n_items) {
    const uint32_t cb = (1ull << w) < S->p.p_db ? w + 1 : w;  // (load_db_items wants a width that holds every value below p_db)
    if (cb == w) return spiral_gpu_server_load_db_items(S, stream, w, first_item, n_items);
    const uint64_t pass = std::max<uint64_t>(1, std::min<uint64_t>(options().db_stage_bytes / (1024ull * cb), 1u << 12));  // items widened at a time
    std::vector<uint8_t> wide;
    for (uint64_t done = 0; done < n_items; done += pass) {
        const uint64_t cnt = std::min(pass, n_items - done);
        wide.assign((size_t)(cnt * 1024ull * cb), 0);
        widen_coeffs(stream + done * item_bytes, wide.data(), (size_t)(cnt * 4 * kN), w, cb);
        if (spiral_gpu_server_load_db_items(S, wide.data(), cb, first_item + done, cnt)) return -1;
    }
    return 0;
}
// the image as the shared keyed bodies take it (kv_host.h KvImage); trk: the caller's, filled by track_ctx
extern "C++" KvImage kv_image(spiral_gpu_server* S, const FpTrackCtx& trk) {
    return KvImage{S->xwork, S->img->upd, S->tb, S->stream, S->img->export_source(), S->img->update_target(), RecordTrials{}, trk.t ? &trk : nullptr, S->s.num_per, S->p.p_db};
}
// put, and delete: the owner's checks, then kv_host.h kv_write
int kv_write(spiral_gpu_server* S, const char* what, bool put, const void* table_key16, const void* keys, uint64_t key_bytes, const void* values, uint64_t value_bytes,
             uint64_t n, uint64_t* n_deleted) {
    if (!S) return fail("null server");
    if (S->img->owner != S) return fail("%s: this server sweeps another server's database image (share_db or a lane): update it through the owner", what);
    spiral_gpu_kv_layout l;
    if (kv_call(S, what, value_bytes, &l)) return -1;
    if (!S->img->loaded) return fail("no database loaded");
    HIP_OK(hipSetDevice(S->device));
    FpTrackCtx trk;
    track_ctx(S, trk);
    return kv_write(kv_image(S, trk), what, put, l, table_key16, keys, key_bytes, values, n, n_deleted);
}
}  // namespace

int spiral_gpu_kv_layout_of(const spiral_gpu_params* p, uint64_t value_bytes, spiral_gpu_kv_layout* out) { return kv_layout(p, value_bytes, out); }

int spiral_gpu_kv_hash(const spiral_gpu_params* p, const void* table_key16, const void* key, uint64_t key_bytes, uint64_t* tag, uint64_t* b1, uint64_t* b2) {
    if (!p || !table_key16 || !tag || !b1 || !b2 || (key_bytes && !key)) return fail("kv_hash: null argument");
    uint64_t nb;
    if (kv_buckets(p, 0, &nb)) return -1;
    static const uint8_t none = 0;
    const KvKey h = kv_hash(nb, static_cast<const uint8_t*>(table_key16), key_bytes ? static_cast<const uint8_t*>(key) : &none, key_bytes);
    *tag = h.tag;
    *b1 = h.b[0];
    *b2 = h.b[1];
    return 0;
}

// A fresh table: placement from empty and the item stream on the host, then load_db_items' ingest of the whole image (not a hot path)
int spiral_gpu_server_kv_load(spiral_gpu_server* S, const void* table_key16, const void* keys, uint64_t key_bytes, const void* values, uint64_t value_bytes, uint64_t n) {
    if (!S) return fail("null server");
    if (S->img->owner != S) return fail("kv_load: this server sweeps another server's database image (share_db): load it through the owner");
    spiral_gpu_kv_layout l;
    if (kv_call(S, "kv_load", value_bytes, &l)) return -1;
    if (n && !values) return fail("kv_load: null argument");
    std::vector<KvKey> hk;
    if (kv_hash_keys("kv_load", l.buckets, table_key16, keys, key_bytes, n, true, hk)) return -1;
    KvTable table;
    table.slots = l.slots;
    table.ids.resize((size_t)l.buckets);
    for (uint64_t b = 0; b < l.buckets; b++) table.ids[b] = b;
    table.occ.assign((size_t)l.buckets, std::array<uint64_t, 4>{});
    std::vector<uint8_t> stream((size_t)(l.buckets * l.item_bytes), 0);
    for (uint64_t k = 0; k < n; k++) {
        uint32_t cand, slot;
        if (!table.place(hk[k], &cand, &slot))
            return fail("kv_load: key %llu cannot be placed: its buckets %llu and %llu are both full (%u slots each); the image was not touched", (unsigned long long)k,
                        (unsigned long long)hk[k].b[0], (unsigned long long)hk[k].b[1], l.slots);
        uint8_t* item = stream.data() + hk[k].b[cand] * l.item_bytes;
        for (int b = 0; b < 8; b++) item[8u * slot + b] = (uint8_t)(hk[k].tag >> (8 * b));
        memcpy(item + 8u * l.slots + slot * value_bytes, static_cast<const uint8_t*>(values) + k * value_bytes, (size_t)value_bytes);
    }
    return load_item_stream(S, stream.data(), l.coeff_bits, l.item_bytes, 0, l.buckets);
}

int spiral_gpu_server_kv_put(spiral_gpu_server* S, const void* table_key16, const void* keys, uint64_t key_bytes, const void* values, uint64_t value_bytes, uint64_t n) {
    if (n && !values) return fail("kv_put: null argument");
    return kv_write(S, "kv_put", true, table_key16, keys, key_bytes, values, value_bytes, n, nullptr);
}

int spiral_gpu_server_kv_delete(spiral_gpu_server* S, const void* table_key16, const void* keys, uint64_t key_bytes, uint64_t value_bytes, uint64_t n, uint64_t* n_deleted) {
    return kv_write(S, "kv_delete", false, table_key16, keys, key_bytes, nullptr, value_bytes, n, n_deleted);
}

// The probe, then the found slots' values through read_records' path; any server that references the image, on its own stream
int spiral_gpu_server_kv_get(spiral_gpu_server* S, const void* table_key16, const void* keys, uint64_t key_bytes, void* values, uint64_t value_bytes, uint64_t n,
                             uint8_t* found) {
    if (enter(S)) return -1;
    spiral_gpu_kv_layout l;
    if (kv_call(S, "kv_get", value_bytes, &l)) return -1;
    if (n && (!values || !found)) return fail("kv_get: null argument");
    if (!S->img->loaded) return fail("no database loaded");
    FpTrackCtx none;
    return kv_get(kv_image(S, none), l, table_key16, keys, key_bytes, values, n, found);
}

// Table occupancy: one launch over the range's buckets, 257 words back (kv_host.h kv_stats); any server that references the image, on its own stream
int spiral_gpu_server_kv_stats(spiral_gpu_server* S, uint64_t value_bytes, uint64_t first_bucket, uint64_t n_buckets, spiral_gpu_kv_stats* out) {
    if (enter(S)) return -1;
    if (!out) return fail("kv_stats: null argument");
    spiral_gpu_kv_layout l;
    if (kv_call(S, "kv_stats", value_bytes, &l)) return -1;
    if (!S->img->loaded) return fail("no database loaded");
    return kv_stats(S->xwork, S->tb, S->stream, S->img->export_source(), l, S->p.p_db, first_bucket, n_buckets, out);
}

// Listing: passes of three launches over the buckets named, the live entries back, their values through read_records' path (kv_host.h kv_scan); any
// server that references the image, on its own stream
namespace {
int kv_scan_call(spiral_gpu_server* S, const char* what, uint64_t value_bytes, uint64_t first_bucket, const uint64_t* buckets, uint64_t n_buckets,
                 spiral_gpu_kv_entry* entries, void* values, uint64_t max_entries, uint64_t* n_entries) {
    if (enter(S)) return -1;
    if (!n_entries) return fail("%s: null argument", what);
    spiral_gpu_kv_layout l;
    if (kv_call(S, what, value_bytes, &l)) return -1;
    if (!S->img->loaded) return fail("no database loaded");
    FpTrackCtx none;
    return kv_scan(kv_image(S, none), what, l, first_bucket, buckets, n_buckets, entries, values, max_entries, n_entries);
}
}  // namespace
int spiral_gpu_server_kv_scan(spiral_gpu_server* S, uint64_t value_bytes, uint64_t first_bucket, uint64_t n_buckets, spiral_gpu_kv_entry* entries, void* values,
                              uint64_t max_entries, uint64_t* n_entries) {
    return kv_scan_call(S, "kv_scan", value_bytes, first_bucket, nullptr, n_buckets, entries, values, max_entries, n_entries);
}
int spiral_gpu_server_kv_scan_at(spiral_gpu_server* S, uint64_t value_bytes, const uint64_t* buckets, uint64_t n_buckets, spiral_gpu_kv_entry* entries, void* values,
                                 uint64_t max_entries, uint64_t* n_entries) {
    static const uint64_t none = 0;  // (an empty list may be NULL)
    if (n_buckets && !buckets) return fail("kv_scan_at: null argument");
    return kv_scan_call(S, "kv_scan_at", value_bytes, 0, buckets ? buckets : &none, n_buckets, entries, values, max_entries, n_entries);
}

int spiral_gpu_kv_reconcile(const spiral_gpu_params* p, const void* table_key16, const void* keys, uint64_t key_bytes, uint64_t n_keys, const spiral_gpu_kv_entry* entries,
                            uint64_t n_entries, int64_t* where, uint8_t* entry_class, spiral_gpu_kv_reconcile_counts* counts) {
    uint64_t nb;
    if (kv_buckets(p, 0, &nb)) return -1;  // (nb = 2^(nu1 + nu2), whatever out_n: one function for base and SpiralPack tables)
    return kv_reconcile(nb, table_key16, keys, key_bytes, n_keys, entries, n_entries, where, entry_class, counts);
}

int spiral_gpu_server_read_db_item(spiral_gpu_server* S, uint64_t item, uint64_t* out) {
    if (!S || !out) return fail("null argument");
    if (refuse_column(S, "read_db_item (read its items with read_db_items_at)")) return -1;
    HIP_OK(hipSetDevice(S->device));
    const uint64_t j = item / S->s.num_per;
    if (j < S->j0 || j >= S->j1) return fail("item %llu is not in this shard", (unsigned long long)item);
    Scratch sc;
    uint64_t* d = sc.get(4 * kRefNtt);
    if (!d) return fail("device allocation failed");
    HIP_OK(hipStreamSynchronize(S->stream));
    launch_db_read_item(S->img->db.p, d, S->s.num_per, S->dim0_shard, (uint32_t)(j - S->j0), (uint32_t)(item % S->s.num_per), S->stream,
                        S->img->format == SPIRAL_GPU_DB_LIMBS);
    HIP_OK(hipMemcpyAsync(out, d, 4 * kRefNtt * sizeof(uint64_t), hipMemcpyDeviceToHost, S->stream));
    HIP_OK(hipStreamSynchronize(S->stream));
    return 0;
}

int spiral_gpu_server_read_db_slots(spiral_gpu_server* S, uint32_t z_begin, uint32_t nz, uint64_t* out) {
    if (!S) return fail("null argument");
    return read_db_region(S, z_begin, nz, 0, S->s.num_per, out);
}
int spiral_gpu_server_read_db_columns(spiral_gpu_server* S, uint32_t ii_begin, uint32_t n_ii, uint64_t* out) {
    return read_db_region(S, 0, kN, ii_begin, n_ii, out);
}

int spiral_gpu_server_set_db_format(spiral_gpu_server* S, int format) {
    if (!S) return fail("null server");
    if (format != SPIRAL_GPU_DB_PACKED && format != SPIRAL_GPU_DB_LIMBS) return fail("unknown database image format %d", format);
    if (S->img->owner != S) return fail("this server sweeps another server's database image: convert it through the owner");
    if (!S->img->loaded) return fail("no database loaded");
    HIP_OK(hipSetDevice(S->device));
    return S->img->set_format((uint32_t)format, S->stream);
}
int spiral_gpu_server_db_format(spiral_gpu_server* S) { return S ? (int)S->img->format : -1; }
uint64_t spiral_gpu_server_db_device_bytes(spiral_gpu_server* S) { return S ? S->img->device_bytes() : 0; }

int spiral_gpu_server_fill_db_random(spiral_gpu_server* S, uint64_t seed) {
    if (!S) return fail("null server");
    if (S->img->owner != S) return fail("this server sweeps another server's database image (share_db): load it through the owner");
    HIP_OK(hipSetDevice(S->device));
    S->img->begin_rewrite();
    launch_fill_db_random(S->img->db.p, srv_np(S), S->dim0_shard, seed, S->stream);
    HIP_OK(hipStreamSynchronize(S->stream));
    S->img->finish_load();
    return 0;
}

// A second in-flight query on the same database: `S` gives its own image's reference back and takes one of `owner`'s (the image
// is read-only on the answer path).  Same parameters, shard and device; `owner` must not reload its database while `S`
// answers.  With one handle per query lane, each on its own stream, the latency-bound expansion / fold of one query runs
// under the HBM-bound sweep of the other.
int spiral_gpu_server_share_db(spiral_gpu_server* S, spiral_gpu_server* owner) {
    if (!S || !owner || S == owner) return fail("share_db needs two different servers");
    if (owner->img->owner != owner) return fail("the owner does not own its database image");
    if (S->device != owner->device || S->j0 != owner->j0 || S->dim0_shard != owner->dim0_shard || S->p.nu1 != owner->p.nu1 || S->p.nu2 != owner->p.nu2 ||
        S->s.num_per != owner->s.num_per || !(S->col == owner->col))
        return fail("share_db: the servers differ in device, shard (first-dimension range, or column shard and its rank) or database geometry");
    // the image encodes plaintexts mod p_db (centred lift) and the lane's response switch uses ITS p_db: they must agree
    if (S->p.p_db != owner->p.p_db || S->p.direct_upload != owner->p.direct_upload)
        return fail("share_db: the servers differ in plaintext modulus or query form");
    if (!owner->img->loaded) return fail("the owner has no database loaded");
    HIP_OK(hipSetDevice(S->device));
    HIP_OK(hipStreamSynchronize(S->stream));
    srv_drop_graphs(S);  // captured sweeps hold the old image's address
    if (S->img->owner == S && S->img->lanes() > 0) return fail("share_db: this server's own image is swept by %u lanes", S->img->lanes());
    if (S->img != owner->img) {
        DbImage::drop(S->img, S);
        S->img = owner->img->share();
    }
    return 0;
}

// The client's two messages in their three forms (include/spiral_gpu.h).  The wire and seeded forms are decoded and transformed on the device into the
// same buffers as the NTT form, so graphs captured on them replay the new query; any failure after the first write leaves no public parameters / no
// query behind
int spiral_gpu_server_set_pub_params(spiral_gpu_server* S, const uint64_t* w_left, const uint64_t* w_right, const uint64_t* w,
                                     const uint64_t* v) {
    return take_pub_params(S, FORM_NTT, MessageIn{{w_left, w_right, w, v}, nullptr, 0}, "set_pub_params");
}
int spiral_gpu_server_set_query(spiral_gpu_server* S, const uint64_t* query) { return take_query(S, FORM_NTT, MessageIn{{query}, nullptr, 0}, "set_query"); }
int spiral_gpu_server_set_pub_params_wire(spiral_gpu_server* S, const void* wire, size_t bytes) {
    return take_pub_params(S, FORM_WIRE, MessageIn{{}, wire, bytes}, "set_pub_params_wire");
}
int spiral_gpu_server_set_query_wire(spiral_gpu_server* S, const void* wire, size_t bytes) {
    return take_query(S, FORM_WIRE, MessageIn{{}, wire, bytes}, "set_query_wire");
}
int spiral_gpu_server_set_pub_params_seeded(spiral_gpu_server* S, const void* msg, size_t bytes) {
    return take_pub_params(S, FORM_SEEDED, MessageIn{{}, msg, bytes}, "set_pub_params_seeded");
}
int spiral_gpu_server_set_query_seeded(spiral_gpu_server* S, const void* msg, size_t bytes) {
    return take_query(S, FORM_SEEDED, MessageIn{{}, msg, bytes}, "set_query_seeded");
}

int spiral_gpu_server_expand(spiral_gpu_server* S) {
    if (enter(S)) return -1;
    if (!S->have_query || !S->have_pp) return fail("query and public parameters must be set before expand");
    return expand_lanes(S, Lanes{});
}

int spiral_gpu_server_convert(spiral_gpu_server* S) {
    if (enter(S)) return -1;
    return convert_part(S, CONV_BOTH, S->stream, !S->use_graphs);
}

int spiral_gpu_server_set_overlap(spiral_gpu_server* S, int on) {
    if (enter(S)) return -1;
    if (on != 0 && on != 2) return fail("overlap mode %d: only 0 (one stream) and 2 (split: the GSW side on a side stream) exist", on);
    if (srv_join_side(S)) return -1;
    if (on == 2) {  // the odd tree needs its own work buffers, and evens / odds must be first-dimension / GSW ciphertexts
        if (S->p.direct_upload || S->s.g == 0 || S->s.stopround == 0 || S->ex_shard.g_log) return fail("split overlap needs query compression with stopround > 0 on an unsharded expansion");
        if (!S->ex_raw2.p && S->ex_raw2.alloc((size_t)S->n_cv * 2 * kN)) return -1;
        if (!S->ex_g2.p && S->ex_g2.alloc(expand_g_polys(S->s.g, S->p.t_exp, S->p.t_exp_right) * kN)) return -1;
    }
    S->overlap = on;
    srv_drop_graphs(S);
    return 0;
}

int spiral_gpu_server_first_dim(spiral_gpu_server* S) {
    if (enter(S)) return -1;
    if (!S->img->loaded) return fail("no database loaded");
    S->raw_from_acc = false;
    return sweep_one(S, -1);
}

// Pipelined sweep (N > 1): the output columns are independent (src/spiral.cpp:628-999 loops over i and c outside j), so a rank may
// sweep them in K stages of num_per / K ciphertexts and hand every stage's accumulators to its own reduce-scatter while the next
// stage streams the database.  set_sweep_stages lays the accumulators out [stage][rank][ct] (every stage one contiguous block of
// 1/K of the buffer; a rank's reduce-scattered rows still come out in the order fold_local expects); first_dim_stage launches one
// stage; first_dim launches all of them at once into the same layout.
int spiral_gpu_server_set_sweep_stages(spiral_gpu_server* S, uint32_t n_stages) {
    if (enter(S)) return -1;
    if (refuse_column(S, "set_sweep_stages")) return -1;
    if (n_stages == 0 || (n_stages & (n_stages - 1))) return fail("sweep stages must be a power of two");
    const uint32_t k_log = ceil_log2(n_stages);
    if (!sweep_stages_ok(S->s.num_per, 2 * S->dim0_shard, S->fold_g_log, k_log))
        return fail("%u sweep stages: needs the packed layout, whole 64-column blocks per stage (at most %u stages here) and a ciphertext per rank and stage", n_stages,
                    S->s.num_per / 32);
    // stage-by-stage launches exist for the packed image only: an image a batch has converted to limb planes goes back (its holder's lanes re-capture)
    if (k_log && S->img->format != SPIRAL_GPU_DB_PACKED && S->img->set_format(SPIRAL_GPU_DB_PACKED, S->stream)) return -1;
    S->sweep_k_log = k_log;
    srv_drop_graphs(S);
    return 0;
}

uint32_t spiral_gpu_server_max_sweep_stages(spiral_gpu_server* S) {
    if (!S) return 0;
    if (S->col.on) return 1;
    uint32_t k = 0;
    while (k < 16 && sweep_stages_ok(S->s.num_per, 2 * S->dim0_shard, S->fold_g_log, k + 1)) k++;
    return 1u << k;
}

int spiral_gpu_server_first_dim_stage(spiral_gpu_server* S, uint32_t stage) {
    if (enter(S)) return -1;
    if (refuse_column(S, "first_dim_stage")) return -1;
    if (!S->img->loaded) return fail("no database loaded");
    if (stage >= (1u << S->sweep_k_log)) return fail("stage %u of %u", stage, 1u << S->sweep_k_log);
    if (S->sweep_k_log == 0) return spiral_gpu_server_first_dim(S);
    S->raw_from_acc = false;
    return sweep_one(S, (int)stage);
}

int spiral_gpu_server_lift(spiral_gpu_server* S, int reduce_first) {
    if (enter(S)) return -1;
    if (refuse_column(S, "lift")) return -1;
    launch_job(S->tb, lift_job(S->acc, S->raw.p, S->s.num_per * 6, {.pre_reduce = reduce_first != 0}), S->stream);
    S->raw_from_acc = true;
    return 0;
}

int spiral_gpu_server_fold(spiral_gpu_server* S) {
    if (enter(S)) return -1;
    if (refuse_column(S, "fold")) return -1;
    if (srv_join_side(S)) return -1;  // no-op inside run_post's capture: run_post joined before capturing
    return run_fold_rounds(S, {.np0 = S->s.num_per, .rounds = S->p.nu2, .raw_addend = S->raw_from_acc ? S->acc : nullptr});  // src/spiral.cpp:1622-1626
}

int spiral_gpu_server_set_fold_ranks(spiral_gpu_server* S, uint32_t n_ranks) {
    if (enter(S)) return -1;
    if (n_ranks == 0 || (n_ranks & (n_ranks - 1)) || n_ranks > S->s.num_per) return fail("fold ranks must be a power of two <= num_per");
    if (S->col.on && n_ranks != col_ranks(S))
        return fail("set_fold_ranks: this server is a column shard of %u ranks (create_column_shard): its fold-rank count is fixed to that, not %u", col_ranks(S), n_ranks);
    S->fold_g_log = ceil_log2(n_ranks);
    S->sweep_k_log = 0;  // the stage layout depends on the rank count: set_sweep_stages comes after
    srv_drop_graphs(S);
    return 0;
}

// Sharded expansion for one rank of an n_ranks-GPU answer.  After it, expand() leaves this rank with
// the first-dimension ciphertexts of its own j-range (which must be the contiguous block `rank` of n_ranks equal ones) and
// with the GSW bits i = rank mod n_ranks; gsw_bits_pack / one all-gather / gsw_bits_unpack give every rank all of them
// before convert().  Needs the reordered layout (stopround > 0, src/spiral.cpp:2027-2036) and query compression.
int spiral_gpu_server_set_expand_shard(spiral_gpu_server* S, uint32_t rank, uint32_t n_ranks) {
    if (enter(S)) return -1;
    if (refuse_column(S, "set_expand_shard")) return -1;
    srv_drop_graphs(S);
    if (n_ranks <= 1) {
        S->ex_shard = ExpandShard{};
        return 0;
    }
    if ((n_ranks & (n_ranks - 1)) || n_ranks > S->s.dim0 || rank >= n_ranks) return fail("expansion shard %u of %u: the rank count must be a power of two <= dim0", rank, n_ranks);
    if (S->p.direct_upload || S->s.stopround == 0) return fail("sharded expansion needs query compression with stopround > 0");
    if (S->overlap) return fail("sharded expansion and the split overlap schedule exclude each other");
    const uint32_t per = S->s.dim0 / n_ranks;
    if (S->j0 != rank * per || S->j1 != (rank + 1) * per) return fail("sharded expansion: this server must hold first-dimension block %u of %u, it holds [%u, %u)", rank, n_ranks, S->j0, S->j1);
    S->ex_shard = ExpandShard{rank, ceil_log2(n_ranks), S->p.nu1 - ceil_log2(n_ranks)};
    return 0;
}

size_t spiral_gpu_server_gsw_bits_words(spiral_gpu_server* S) {
    if (!S) return 0;
    const uint32_t G = 1u << S->ex_shard.g_log, n_bits = S->s.ell * S->p.nu2;
    return (size_t)((n_bits + G - 1) / G) * 2 * kN;
}

int spiral_gpu_server_gsw_bits_pack(spiral_gpu_server* S, void* block_out) {
    if (!S || !block_out) return fail("null argument");
    HIP_OK(hipSetDevice(S->device));
    launch_gsw_bits_pack(S->cv.p, (uint64_t*)block_out, S->ex_shard.rank, 1u << S->ex_shard.g_log, S->s.ell * S->p.nu2, S->stream);
    return 0;
}

int spiral_gpu_server_gsw_bits_unpack(spiral_gpu_server* S, const void* gathered) {
    if (!S || !gathered) return fail("null argument");
    HIP_OK(hipSetDevice(S->device));
    launch_gsw_bits_unpack(S->cv.p, (const uint64_t*)gathered, 1u << S->ex_shard.g_log, S->s.ell * S->p.nu2, S->stream);
    return 0;
}

int spiral_gpu_server_finish(spiral_gpu_server* S) {
    if (enter(S)) return -1;
    return finish_lanes(S, Lanes{});
}

int spiral_gpu_server_sync(spiral_gpu_server* S) {
    if (enter(S)) return -1;
    if (srv_join_side(S)) return -1;
    HIP_OK(hipStreamSynchronize(S->stream));
    HIP_OK(hipGetLastError());
    return 0;
}

void* spiral_gpu_server_acc(spiral_gpu_server* S, size_t* bytes) {
    if (!S) return nullptr;
    if (bytes) *bytes = (size_t)S->s.num_per * 6 * kPolyBytes;
    return S->acc;
}

int spiral_gpu_server_set_acc(spiral_gpu_server* S, void* device_ptr) {
    if (!S) return fail("null server");
    S->acc = device_ptr ? (uint64_t*)device_ptr : S->acc_own.p;
    S->raw_from_acc = false;
    srv_drop_graphs(S);  // the accumulator pointer is baked into the captured lift
    return 0;
}

int spiral_gpu_server_run_pre(spiral_gpu_server* S) {
    if (enter(S)) return -1;
    if (!S->have_query || !S->have_pp) return fail("query and public parameters must be set first");
    // split: [odd tree of the expansion + Regev->GSW + fold keys] on the side stream, [even tree + ScalToMat] on the main stream, forked
    // HERE (the side depends on the query only: it runs beside the even tree); the fold joins the side stream
    const spiral_gpu_params& p = S->p;
    auto half = [&](uint32_t parity, hipStream_t st, uint64_t* raw, uint64_t* g) {
        ExpandWork wk{raw, g};
        run_expand(S->tb, S->cv.p, S->s.g, p.t_exp, S->w_left.p, p.t_exp_right, S->w_right.p, S->s.ell * p.nu2, S->s.stopround, wk, st, S->query.p, 0, 0xffffffffu,
                   ExpandShard{}, parity);
    };
    if (S->overlap) {
        if (srv_join_side(S)) return -1;
        HIP_OK(hipEventRecord(S->ev_fork, S->stream));  // the previous query's fold has read its keys; the new query is uploaded
        HIP_OK(hipStreamWaitEvent(S->side_stream, S->ev_fork, 0));
        if (run_graph(S, G_PRE_SIDE, S->side_stream, {}, [&]() {
                half(2u, S->side_stream, S->ex_raw2.p, S->ex_g2.p);
                return convert_part(S, CONV_GSW, S->side_stream);
            }))
            return -1;
        HIP_OK(hipEventRecord(S->ev_join, S->side_stream));
        S->side_pending = true;
    }
    if (int rc = run_graph(S, G_PRE, S->stream, {}, [&]() {
            if (!S->overlap) return expand_convert(S);
            half(1u, S->stream, S->ex_raw.p, S->ex_g.p);
            return convert_part(S, CONV_S2M, S->stream);
        }))
        return rc;
    S->have_records = true;
    return 0;
}

int spiral_gpu_server_run_query(spiral_gpu_server* S) {
    if (enter(S)) return -1;
    if (refuse_column(S, "run_query")) return -1;
    if (!S->have_query || !S->have_pp) return fail("query and public parameters must be set first");
    if (!S->img->loaded) return fail("no database loaded");
    if (S->overlap) {  // the split schedule is three launch groups on two streams, not one graph
        if (spiral_gpu_server_run_pre(S)) return -1;
        if (spiral_gpu_server_first_dim(S)) return -1;
        return spiral_gpu_server_run_post(S, 0);
    }
    if (srv_join_side(S)) return -1;
    if (int rc = run_graph(S, G_QUERY, S->stream, {}, [&]() {
            if (expand_convert(S)) return -1;
            if (spiral_gpu_server_first_dim(S)) return -1;
            return run_fold_rounds(S, {.np0 = S->s.num_per, .rounds = S->p.nu2, .src_pk = S->acc, .finish = true});
        }))
        return rc;
    mark_swept(&S, 1);
    return 0;
}

int spiral_gpu_server_fold_local(spiral_gpu_server* S, const void* acc_chunk, void* out_ct) {
    if (!S || !acc_chunk || !out_ct) return fail("null argument");
    if (refuse_column(S, "fold_local")) return -1;
    HIP_OK(hipSetDevice(S->device));
    const uint32_t L = S->s.num_per >> S->fold_g_log;
    if (srv_join_side(S)) return -1;
    if (int rc = run_graph(S, G_FOLD_LOCAL, S->stream, {word(acc_chunk), word(out_ct)}, [&]() {
            if (run_fold_rounds(S, {.np0 = L, .rounds = S->p.nu2 - S->fold_g_log, .src_pk = (const uint64_t*)acc_chunk, .pre_reduce = true})) return -1;
            HIP_OK(hipMemcpyAsync(out_ct, S->raw.p, 6 * kPolyBytes, hipMemcpyDeviceToDevice, S->stream));
            return 0;
        }))
        return rc;
    S->raw_from_acc = false;
    return 0;
}

int spiral_gpu_server_fold_root(spiral_gpu_server* S, const void* gathered_cts) {
    if (!S || !gathered_cts) return fail("null argument");
    HIP_OK(hipSetDevice(S->device));
    const uint32_t G = 1u << S->fold_g_log;
    if (srv_join_side(S)) return -1;
    if (int rc = run_graph(S, G_FOLD_ROOT, S->stream, {word(gathered_cts)}, [&]() {
            HIP_OK(hipMemcpyAsync(S->raw.p, gathered_cts, (size_t)G * 6 * kPolyBytes, hipMemcpyDeviceToDevice, S->stream));
            return run_fold_rounds(S, {.np0 = G, .d0 = S->p.nu2 - S->fold_g_log, .rounds = S->fold_g_log, .finish = true});
        }))
        return rc;
    S->raw_from_acc = false;
    return 0;
}

// run_pre + first_dim as one group: what a rank does before the collective
int spiral_gpu_server_run_pre_sweep(spiral_gpu_server* S) {
    if (enter(S)) return -1;
    if (refuse_column(S, "run_pre_sweep")) return -1;
    if (!S->have_query || !S->have_pp) return fail("query and public parameters must be set first");
    if (!S->img->loaded) return fail("no database loaded");
    if (S->overlap) {
        if (spiral_gpu_server_run_pre(S)) return -1;
        return spiral_gpu_server_first_dim(S);
    }
    if (int rc = run_graph(S, G_PRE_SWEEP, S->stream, {}, [&]() {
            if (expand_convert(S)) return -1;
            return spiral_gpu_server_first_dim(S);
        }))
        return rc;
    mark_swept(&S, 1);
    return 0;
}

// the two halves of everything before the accumulator reduce when the expansion is sharded: run_expand_pack = expand + pack of
// this rank's GSW bits into bits_out; [all-gather]; run_unpack_convert_sweep = unpack of the gathered blocks + convert + sweep
int spiral_gpu_server_run_expand_pack(spiral_gpu_server* S, void* bits_out) {
    if (!S || !bits_out) return fail("null argument");
    if (refuse_column(S, "run_expand_pack")) return -1;
    HIP_OK(hipSetDevice(S->device));
    if (!S->have_query || !S->have_pp) return fail("query and public parameters must be set first");
    return run_graph(S, G_EXPAND_PACK, S->stream, {word(bits_out)}, [&]() {
        if (expand_lanes(S, Lanes{})) return -1;
        return spiral_gpu_server_gsw_bits_pack(S, bits_out);
    });
}

int spiral_gpu_server_run_unpack_convert_sweep(spiral_gpu_server* S, const void* gathered) {
    if (!S || !gathered) return fail("null argument");
    if (refuse_column(S, "run_unpack_convert_sweep")) return -1;
    HIP_OK(hipSetDevice(S->device));
    if (!S->img->loaded) return fail("no database loaded");
    if (int rc = run_graph(S, G_UNPACK_CONVERT_SWEEP, S->stream, {word(gathered)}, [&]() {
            if (spiral_gpu_server_gsw_bits_unpack(S, gathered)) return -1;
            if (convert_part(S, CONV_BOTH, S->stream, !S->use_graphs)) return -1;
            return spiral_gpu_server_first_dim(S);
        }))
        return rc;
    mark_swept(&S, 1);
    return 0;
}

// The same split so that the all-gather of the GSW bits can run UNDER the database-dependent work: the sweep needs only the
// ScalToMat outputs (this rank's own first-dimension ciphertexts), the GSW bits only feed the folding keys.
// run_scal2mat_sweep = ScalToMat + sweep (after run_expand_pack, while the all-gather is in flight);
// run_unpack_gsw = unpack of the gathered blocks + Regev->GSW conversion (after the all-gather, e.g. under the reduce-scatter).
int spiral_gpu_server_run_scal2mat_sweep(spiral_gpu_server* S) {
    if (enter(S)) return -1;
    if (!S->img->loaded) return fail("no database loaded");
    if (int rc = run_graph(S, G_SCAL2MAT_SWEEP, S->stream, {}, [&]() {
            if (convert_part(S, CONV_S2M, S->stream)) return -1;
            return spiral_gpu_server_first_dim(S);
        }))
        return rc;
    mark_swept(&S, 1);
    return 0;
}

// ScalToMat alone (the pipelined schedule issues the sweep stage by stage after it)
int spiral_gpu_server_run_scal2mat(spiral_gpu_server* S) {
    if (enter(S)) return -1;
    if (int rc = run_graph(S, G_SCAL2MAT, S->stream, {}, [&]() { return convert_part(S, CONV_S2M, S->stream); })) return rc;
    S->have_records = true;
    return 0;
}

int spiral_gpu_server_run_unpack_gsw(spiral_gpu_server* S, const void* gathered) {
    if (!S || !gathered) return fail("null argument");
    HIP_OK(hipSetDevice(S->device));
    return run_graph(S, G_UNPACK_GSW, S->stream, {word(gathered)}, [&]() {
        if (spiral_gpu_server_gsw_bits_unpack(S, gathered)) return -1;
        return convert_part(S, CONV_GSW, S->stream);
    });
}

int spiral_gpu_server_run_post(spiral_gpu_server* S, int reduce_first) {
    if (enter(S)) return -1;
    if (refuse_column(S, "run_post")) return -1;
    if (srv_join_side(S)) return -1;
    if (int rc = run_graph(S, reduce_first ? G_POST_REDUCE : G_POST, S->stream, {}, [&]() {
            return run_fold_rounds(S, {.np0 = S->s.num_per, .rounds = S->p.nu2, .src_pk = S->acc, .pre_reduce = reduce_first != 0, .finish = true});  // lift chained into round 0, switch into the last
        }))
        return rc;
    S->raw_from_acc = false;
    return 0;
}

int spiral_gpu_server_answer_resident(spiral_gpu_server* S, double stage_us[8]) {
    if (enter(S)) return -1;
    if (refuse_column(S, "answer_resident")) return -1;
    hipStream_t st = S->stream;
    const bool g = S->use_graphs;
    HIP_OK(hipEventRecord(S->ev[0], st));
    if (g) {
        if (spiral_gpu_server_run_pre(S)) return -1;
        HIP_OK(hipEventRecord(S->ev[1], st));
    } else {
        if (spiral_gpu_server_expand(S)) return -1;  // (the stage calls where they check or set flags: expand, first_dim, lift, fold)
        HIP_OK(hipEventRecord(S->ev[1], st));
        if (convert_part(S, CONV_BOTH, st, true)) return -1;
    }
    HIP_OK(hipEventRecord(S->ev[2], st));
    if (spiral_gpu_server_first_dim(S)) return -1;
    HIP_OK(hipEventRecord(S->ev[3], st));
    if (g) {
        if (spiral_gpu_server_run_post(S, 0)) return -1;
        HIP_OK(hipEventRecord(S->ev[4], st));
        HIP_OK(hipEventRecord(S->ev[5], st));
    } else {
        if (spiral_gpu_server_lift(S, 0)) return -1;
        HIP_OK(hipEventRecord(S->ev[4], st));
        if (spiral_gpu_server_fold(S)) return -1;
        HIP_OK(hipEventRecord(S->ev[5], st));
        if (finish_lanes(S, Lanes{})) return -1;
    }
    HIP_OK(hipEventRecord(S->ev[6], st));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());
    if (stage_us) {
        float ms[6];
        for (int i = 0; i < 6; i++) HIP_OK(hipEventElapsedTime(&ms[i], S->ev[i], S->ev[i + 1]));
        float total = 0;
        HIP_OK(hipEventElapsedTime(&total, S->ev[0], S->ev[6]));
        // with graphs on, expansion+conversion land in [0] and lift+fold+switch in [2]/[3] as one group
        stage_us[0] = ms[0] * 1e3;
        stage_us[1] = ms[1] * 1e3;
        stage_us[2] = (ms[2] + ms[3]) * 1e3;
        stage_us[3] = ms[4] * 1e3;
        stage_us[4] = ms[5] * 1e3;
        stage_us[5] = ms[2] * 1e3;
        stage_us[6] = total * 1e3;
        stage_us[7] = 0;
        if (!g) {  // ScalToMat share of the conversion bucket (src/spiral.cpp:2254-2256)
            float s2m = 0;
            HIP_OK(hipEventElapsedTime(&s2m, S->ev[1], S->ev[7]));
            stage_us[7] = s2m * 1e3;
        }
    }
    return 0;
}

int spiral_gpu_server_answer(spiral_gpu_server* S, const uint64_t* query, uint64_t* final_ct, uint64_t* response, double stage_us[8]) {
    if (enter(S)) return -1;
    if (refuse_column(S, "answer")) return -1;
    if (spiral_gpu_server_set_query(S, query)) return -1;
    if (spiral_gpu_server_answer_resident(S, stage_us)) return -1;
    if (final_ct) HIP_OK(hipMemcpy(final_ct, S->raw.p, 6 * kPolyBytes, hipMemcpyDeviceToHost));
    if (response) HIP_OK(hipMemcpy(response, S->resp.p, 6 * kPolyBytes, hipMemcpyDeviceToHost));
    return 0;
}

int spiral_gpu_server_keep_cts(spiral_gpu_server* S, int on) {
    if (enter(S)) return -1;
    if (on && !S->cts_keep.p && S->cts_keep.alloc((size_t)S->dim0_shard * 6 * kN)) return -1;
    if (S->keep_cts != (on != 0)) srv_drop_graphs(S);  // ScalToMat's output pointer is baked into the captured conversion
    S->keep_cts = on != 0;
    return 0;
}

size_t spiral_gpu_server_buffer_words(spiral_gpu_server* S, int which) {
    if (!S) return 0;
    const spiral_gpu_shape& s = S->s;
    switch (which) {
        case SPIRAL_GPU_BUF_EXPANDED: return (size_t)s.n_bits * 2 * kRefNtt;
        case SPIRAL_GPU_BUF_CTS: return (size_t)S->dim0_shard * 6 * kRefNtt;
        case SPIRAL_GPU_BUF_GSW: return (size_t)S->p.nu2 * 3 * s.m2 * kRefNtt;
        case SPIRAL_GPU_BUF_ACC: return (size_t)s.num_per * 6 * kRefNtt;
        case SPIRAL_GPU_BUF_RAW: return (size_t)s.num_per * 6 * kN;
        case SPIRAL_GPU_BUF_FINAL: return (size_t)6 * kN;
        case SPIRAL_GPU_BUF_RESPONSE: return (size_t)6 * kN;
        case SPIRAL_GPU_BUF_QUERY: return (size_t)s.n_query_cts * 2 * kRefNtt;
        default: return 0;
    }
}

int spiral_gpu_server_read(spiral_gpu_server* S, int which, uint64_t* out) {
    if (!S || !out) return fail("null argument");
    HIP_OK(hipSetDevice(S->device));
    HIP_OK(hipStreamSynchronize(S->stream));
    const spiral_gpu_shape& s = S->s;
    const uint32_t ps = S->pos_stride;
    switch (which) {
        case SPIRAL_GPU_BUF_EXPANDED: {
            // first dim0 cts, then the ell*nu2 conversion inputs, each 2 polys
            if (download_pk_as_ref(S, S->cv.p, IndexMap{2, 2 * ps, 2 * S->pos_first}, out, (size_t)s.dim0 * 2)) return -1;
            return download_pk_as_ref(S, S->cv.p, IndexMap{2, 2 * ps, 2 * S->pos_rest}, out + (size_t)s.dim0 * 2 * kRefNtt,
                                      (size_t)s.ell * S->p.nu2 * 2);
        }
        case SPIRAL_GPU_BUF_CTS:
            if (!S->keep_cts) return fail("keep_cts is off");
            return download_pk_as_ref(S, S->cts_keep.p, identity_map(), out, (size_t)S->dim0_shard * 6);
        case SPIRAL_GPU_BUF_GSW: return download_pk_as_ref(S, S->key.p, identity_map(), out, (size_t)S->p.nu2 * 3 * s.m2);
        case SPIRAL_GPU_BUF_ACC: return download_pk_as_ref(S, S->acc, identity_map(), out, (size_t)s.num_per * 6);
        case SPIRAL_GPU_BUF_RAW: HIP_OK(hipMemcpy(out, S->raw.p, (size_t)s.num_per * 6 * kPolyBytes, hipMemcpyDeviceToHost)); return 0;
        case SPIRAL_GPU_BUF_FINAL: HIP_OK(hipMemcpy(out, S->raw.p, 6 * kPolyBytes, hipMemcpyDeviceToHost)); return 0;
        case SPIRAL_GPU_BUF_RESPONSE: HIP_OK(hipMemcpy(out, S->resp.p, 6 * kPolyBytes, hipMemcpyDeviceToHost)); return 0;
        case SPIRAL_GPU_BUF_QUERY: return download_pk_as_ref(S, S->query.p, identity_map(), out, (size_t)s.n_query_cts * 2);
        default: return fail("unknown buffer %d", which);
    }
}

int spiral_gpu_server_read_response_wire(spiral_gpu_server* S, void* out, size_t capacity) {
    if (!S || !out) return fail("null argument");
    HIP_OK(hipSetDevice(S->device));
    const size_t nbytes = wire_bytes(&S->p, 2);
    if (capacity < nbytes) return fail("response buffer of %zu bytes, the wire form needs %zu", capacity, nbytes);
    if (S->wire.words * 8 < nbytes && (S->wire.release(), S->wire.alloc(nbytes / 8))) return -1;
    launch_response_wire(S->resp.p, S->wire.p, 2 * kN, S->p.qprime_bits, 4 * kN, wire_bits_rest(&S->p), S->stream);
    HIP_OK(hipMemcpyAsync(out, S->wire.p, nbytes, hipMemcpyDeviceToHost, S->stream));
    HIP_OK(hipStreamSynchronize(S->stream));
    return 0;
}

int spiral_gpu_server_write_raw(spiral_gpu_server* S, const uint64_t* raw_cts) {
    if (!S || !raw_cts) return fail("null argument");
    HIP_OK(hipSetDevice(S->device));
    HIP_OK(hipMemcpy(S->raw.p, raw_cts, (size_t)S->s.num_per * 6 * kPolyBytes, hipMemcpyHostToDevice));
    S->raw_from_acc = false;
    return 0;
}

// the counterpart for the accumulators: read(SPIRAL_GPU_BUF_ACC)'s layout and index map, in the other direction
int spiral_gpu_server_write_acc(spiral_gpu_server* S, const uint64_t* acc_ref) {
    if (!S || !acc_ref) return fail("null argument");
    HIP_OK(hipSetDevice(S->device));
    S->raw_from_acc = false;
    return upload_ref_ntt(S->stage, S->stream, acc_ref, S->acc, (size_t)S->s.num_per * 6);
}

int spiral_gpu_server_time_sweep(spiral_gpu_server* S, int iters, float* avg_ms) {
    if (!S || !avg_ms || iters <= 0) return fail("bad argument");
    HIP_OK(hipSetDevice(S->device));
    if (!S->img->loaded) return fail("no database loaded");
    HIP_OK(hipEventRecord(S->ev[0], S->stream));
    for (int i = 0; i < iters; i++)
        if (sweep_one(S, -1)) return -1;
    S->raw_from_acc = false;
    HIP_OK(hipEventRecord(S->ev[1], S->stream));
    HIP_OK(hipStreamSynchronize(S->stream));
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, S->ev[0], S->ev[1]));
    *avg_ms = ms / iters;
    return 0;
}

uint64_t spiral_gpu_server_sweep_device_bytes(spiral_gpu_server* S) {
    if (!S) return 0;
    // what one launch has to move on this device: the database in its device layout (7 bytes per word when packed),
    // the query records (48 B per (z, j)) and the accumulators
    const uint64_t n = kN;
    return (uint64_t)db_device_words(2 * srv_np(S), S->dim0_shard) * 8 + (uint64_t)S->dim0_shard * 48 * n + (uint64_t)srv_np(S) * 6 * n * 8;
}

uint64_t spiral_gpu_server_sweep_bytes(spiral_gpu_server* S) {
    if (!S) return 0;
    // SURVEY.md 8d at 8 B per packed word: database + packed query (3 rows x 2 x dim0) + output (2 limbs as u64)
    const uint64_t n = kN;
    return (uint64_t)S->dim0_shard * srv_np(S) * 4 * n * 8 + (uint64_t)S->dim0_shard * 3 * 2 * n * 8 + (uint64_t)srv_np(S) * 6 * 2 * n * 8;
}

}  // extern "C"
