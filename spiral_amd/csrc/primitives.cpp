// What libspiral_gpu.so keeps per process and what it offers without a server: the error text, the options and counters, and the stateless
// seams of include/spiral_gpu.h -- one reference function each on host buffers, on stream 0, plus the client's plain host halves of the wire and
// seeded forms.  Nothing here touches a spiral_gpu_server; server_state.h is included for the batched sweep and the capture counter.
#include "server_state.h"

thread_local std::string spiral::host::g_err;
// SpiralPack batch calls of this process that ran as one lane-aware launch sequence (get_option "pack_lane_batches"; counted by pack_server.cpp)
std::atomic<uint64_t> spiral::host::g_pack_lane_batches{0};
// matrix-core sweep launches of this process that were made (get_option "mfma_sweeps"; counted by the two launchers of sweep_mfma.hip)
std::atomic<uint64_t> spiral::g_mfma_sweeps{0};
// device nanoseconds of the export launches of this process's last read_db_items / read_db_items_at call (get_option "db_export_ns"; host_common.h export_items)
std::atomic<uint64_t> spiral::host::g_db_export_ns{0};
// the same of its last fingerprint_items / fingerprint_items_at call (get_option "db_fingerprint_ns"; host_common.h fingerprint_items)
std::atomic<uint64_t> spiral::host::g_db_fingerprint_ns{0};

// the process-wide options (kernels.h); the three documented environment variables give their initial values, once
spiral::Options& spiral::options() {
    static Options o = [] {
        Options v;
        if (const char* e = getenv("SPIRAL_FOLD_PAIR")) v.fold_pair = atoi(e) != 0;
        if (const char* e = getenv("SPIRAL_SWEEP_MFMA")) v.sweep_mfma_min = (uint32_t)strtoul(e, nullptr, 10);
        if (const char* e = getenv("SPIRAL_DB_STAGE_BYTES")) v.db_stage_bytes = (size_t)strtoull(e, nullptr, 10);
        return v;
    }();
    return o;
}

namespace {
// a message's bytes in the wire / seeded form for parameters the base path accepts, else 0
size_t base_message_bytes(const spiral_gpu_params* p, MessageLayout (*layout)(const spiral_gpu_params&, const spiral_gpu_shape&), Form form) {
    spiral_gpu_shape s;
    return shape_of(p, &s) ? 0 : message_bytes(layout(*p, s), form);
}
}  // namespace

extern "C" {

int spiral_gpu_abi_version(void) { return SPIRAL_GPU_ABI_VERSION; }

int spiral_gpu_set_option(const char* name, int64_t value) {
    if (!name) return fail("null option name");
    Options& o = options();
    const std::string n = name;
    if (n == "fold_pair") o.fold_pair = value != 0;
    else if (n == "fold_chain") o.fold_chain = value != 0;
    else if (n == "fold_blocks" && value >= 0) o.fold_blocks = (uint32_t)value;
    else if (n == "sweep_mfma_min" && value >= 0) o.sweep_mfma_min = (uint32_t)value;
    else if (n == "one_image") o.one_image = value != 0;
    else if (n == "fwd2" && value >= -1 && value <= 1) o.fwd2 = (int)value;
    else if (n == "fwd2_min" && value >= 0) o.fwd2_min = (uint32_t)value;
    else if (n == "db_stage_bytes" && value > 0) o.db_stage_bytes = (size_t)value;
    else if (n == "pack_item_group" && value >= 0 && value <= 0xFFFFFFFFll) o.pack_item_group = (uint32_t)value;
    else if (n == "pack_batch_lanes" && value >= 0 && value <= (int64_t)kMaxLanes) o.pack_batch_lanes = (uint32_t)value;
    else if (n == "pack_pair_blocks" && (value == 0 || value == 1)) o.pack_pair_blocks = (int)value;
    else if (n == "sweep_narrow" && (value == 0 || value == 1)) o.sweep_narrow = (int)value;
    else if (n == "query_batch_chunk" && value >= 1 && value <= 0xFFFFFFFFll) o.query_batch_chunk = (uint32_t)value;
    else if (n == "kv_scan_chunk" && value >= 0 && value <= (1ll << 16)) o.kv_scan_chunk = (uint32_t)value;
    else return fail("unknown option '%s' or value %lld out of range", name, (long long)value);
    return 0;
}
int spiral_gpu_get_option(const char* name, int64_t* value) {
    if (!name || !value) return fail("null argument");
    const Options& o = options();
    const std::string n = name;
    if (n == "fold_pair") *value = o.fold_pair;
    else if (n == "fold_chain") *value = o.fold_chain;
    else if (n == "fold_blocks") *value = o.fold_blocks;
    else if (n == "sweep_mfma_min") *value = o.sweep_mfma_min;
    else if (n == "one_image") *value = o.one_image;
    else if (n == "fwd2") *value = o.fwd2;
    else if (n == "fwd2_min") *value = o.fwd2_min;
    else if (n == "db_stage_bytes") *value = (int64_t)o.db_stage_bytes;
    else if (n == "pack_item_group") *value = o.pack_item_group;
    else if (n == "pack_batch_lanes") *value = o.pack_batch_lanes;
    else if (n == "pack_pair_blocks") *value = o.pack_pair_blocks;
    else if (n == "sweep_narrow") *value = o.sweep_narrow;
    else if (n == "query_batch_chunk") *value = o.query_batch_chunk;
    else if (n == "kv_scan_chunk") *value = o.kv_scan_chunk;
    else if (n == "graph_captures") *value = (int64_t)g_captures.load();  // (read only)
    else if (n == "pack_lane_batches") *value = (int64_t)g_pack_lane_batches.load();  // (read only)
    else if (n == "key_binds") *value = (int64_t)g_key_binds.load();  // (read only)
    else if (n == "db_export_ns") *value = (int64_t)g_db_export_ns.load();  // (read only)
    else if (n == "db_fingerprint_ns") *value = (int64_t)g_db_fingerprint_ns.load();  // (read only)
    else if (n == "mfma_sweeps") *value = (int64_t)g_mfma_sweeps.load(std::memory_order_relaxed);  // (read only)
    else return fail("unknown option '%s'", name);
    return 0;
}
const char* spiral_gpu_last_error(void) { return g_err.c_str(); }
int spiral_gpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
int spiral_gpu_get_shape(const spiral_gpu_params* p, spiral_gpu_shape* out) { return shape_of(p, out); }
int spiral_gpu_has_limb_form(const spiral_gpu_params* p, uint32_t j_begin, uint32_t j_end) {
    if (!p) return fail("null argument");
    spiral_gpu_shape s;
    spiral_gpu_params q = *p;
    q.direct_upload = 1;  // the image's form does not depend on how the query arrives: no query-size rule here
    if (shape_of(&q, &s)) return -1;
    if (j_end == 0 && j_begin == 0) j_end = s.dim0;
    if (j_begin >= j_end || j_end > s.dim0) return fail("bad first-dimension shard [%u, %u) of %u", j_begin, j_end, s.dim0);
    return DbLayout::base(s.num_per, j_end - j_begin).limbs_ok() ? 1 : 0;  // (below 64 ciphertexts per slot: option sweep_narrow, as read now)
}
// the twin for a column shard's image: L = num_per / n_ranks columns and the whole first dimension, the same rule read in the same place.  A rank count
// that gives no shard (not a power of two, L below the bound) has no image and so no limb form: 0, and last_error says why
int spiral_gpu_column_shard_has_limb_form(const spiral_gpu_params* p, uint32_t n_ranks) {
    if (!p) return fail("null argument");
    spiral_gpu_shape s;
    spiral_gpu_params q = *p;
    q.direct_upload = 1;  // (as above)
    if (shape_of(&q, &s)) return -1;
    const uint32_t L = column_shard_columns(s.num_per, 0, n_ranks);
    if (!L) return 0;
    return DbLayout::base(L, s.dim0).limbs_ok() ? 1 : 0;
}
int spiral_gpu_get_tables(uint64_t* out) {
    if (!out) return fail("null argument");
    tables_host_rows(out);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// host-buffer seams
// ------------------------------------------------------------------------------------------------
int spiral_gpu_ntt_forward(uint64_t* operand, size_t npolys) {
    DeviceTables tb;
    if (current_tables(&tb)) return -1;
    Scratch sc;
    uint64_t* d = sc.upload(operand, npolys * kRefNtt);
    if (!d) return fail("device allocation/upload failed");
    FwdParams fp{};
    fp.src = d;
    fp.dst = d;
    fp.src_map = fp.dst_map = identity_map();
    fp.n_digits = 1;
    launch_ntt_forward(tb, fp, LD_LIMBS, ST_REF, (uint32_t)npolys, 0);
    HIP_OK(hipMemcpy(operand, d, npolys * kRefNtt * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

int spiral_gpu_ntt_inverse(uint64_t* operand, size_t npolys) {
    DeviceTables tb;
    if (current_tables(&tb)) return -1;
    Scratch sc;
    uint64_t* d = sc.upload(operand, npolys * kRefNtt);
    if (!d) return fail("device allocation/upload failed");
    InvParams ip{};
    ip.src = d;
    ip.dst = d;
    ip.src_map = ip.dst_map = identity_map();
    ip.src_ref = 1;
    ip.pre_reduce = 1;
    launch_ntt_inverse(tb, ip, IST_LIMBS, (uint32_t)npolys, 0);
    HIP_OK(hipMemcpy(operand, d, npolys * kRefNtt * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

int spiral_gpu_to_ntt(uint64_t* out, const uint64_t* in, size_t npolys, int reduce) {
    DeviceTables tb;
    if (current_tables(&tb)) return -1;
    Scratch sc;
    uint64_t* d_in = sc.upload(in, npolys * kN);
    uint64_t* d_out = sc.get(npolys * kRefNtt);
    if (!d_in || !d_out) return fail("device allocation/upload failed");
    if (reduce) {
        launch_job(tb, raw_job(d_in, d_out, (uint32_t)npolys, ST_REF), 0);
    } else {
        uint64_t* d_pk = sc.get(npolys * kN);
        if (!d_pk) return fail("device allocation failed");
        launch_job(tb, raw32_job(d_in, d_pk, (uint32_t)npolys), 0);
        launch_pk_to_ref(d_pk, d_out, (uint32_t)npolys, identity_map(), 0);
    }
    HIP_OK(hipMemcpy(out, d_out, npolys * kRefNtt * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

int spiral_gpu_from_ntt(uint64_t* out, const uint64_t* in, size_t npolys) {
    DeviceTables tb;
    if (current_tables(&tb)) return -1;
    Scratch sc;
    uint64_t* d_in = sc.upload(in, npolys * kRefNtt);
    uint64_t* d_out = sc.get(npolys * kN);
    if (!d_in || !d_out) return fail("device allocation/upload failed");
    InvParams ip{};
    ip.src = d_in;
    ip.dst = d_out;
    ip.src_map = ip.dst_map = identity_map();
    ip.src_ref = 1;
    ip.pre_reduce = 1;
    launch_ntt_inverse(tb, ip, IST_CRT, (uint32_t)npolys, 0);
    HIP_OK(hipMemcpy(out, d_out, npolys * kN * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}


// measurement helper: average duration of one batched forward (to_ntt: raw -> packed NTT form) and one batched inverse
// (from_ntt: packed NTT form -> CRT-lifted raw) launch over npolys polynomials, HIP events on the default stream
int spiral_gpu_time_ntt(size_t npolys, int iters, float* fwd_ms, float* inv_ms) {
    if (!fwd_ms || !inv_ms || iters <= 0 || npolys == 0) return fail("bad argument");
    DeviceTables tb;
    if (current_tables(&tb)) return -1;
    Scratch sc;
    uint64_t* d_raw = sc.get(npolys * kN);
    uint64_t* d_pk = sc.get(npolys * kN);
    if (!d_raw || !d_pk) return fail("device allocation failed");
    HIP_OK(hipMemset(d_raw, 0x5a, npolys * kN * sizeof(uint64_t)));
    hipEvent_t e[3];
    for (auto& x : e) HIP_OK(hipEventCreate(&x));
    const FwdJob fwd = raw_job(d_raw, d_pk, (uint32_t)npolys);
    const InvJob inv = lift_job(d_pk, d_raw, (uint32_t)npolys);
    launch_job(tb, fwd, 0);  // warm
    launch_job(tb, inv, 0);
    HIP_OK(hipEventRecord(e[0], 0));
    for (int i = 0; i < iters; i++) launch_job(tb, fwd, 0);
    HIP_OK(hipEventRecord(e[1], 0));
    for (int i = 0; i < iters; i++) launch_job(tb, inv, 0);
    HIP_OK(hipEventRecord(e[2], 0));
    HIP_OK(hipEventSynchronize(e[2]));
    HIP_OK(hipEventElapsedTime(fwd_ms, e[0], e[1]));
    HIP_OK(hipEventElapsedTime(inv_ms, e[1], e[2]));
    *fwd_ms /= iters;
    *inv_ms /= iters;
    for (auto& x : e) (void)hipEventDestroy(x);
    return 0;
}

// the gadget-digit transform launch the conversion / expansion / folding stages are made of: n_digits unsigned digits of each of
// npolys raw polynomials (gadget_invert + to_ntt_no_reduce), one workgroup per digit polynomial -- the source polynomial is read
// n_digits times (cache hits after the first), every transform writes its 16 KiB
int spiral_gpu_time_ntt_digits(size_t npolys, uint32_t n_digits, int iters, float* ms) {
    if (!ms || iters <= 0 || npolys == 0 || n_digits < 1 || n_digits > 56) return fail("bad argument");
    DeviceTables tb;
    if (current_tables(&tb)) return -1;
    Scratch sc;
    uint64_t* d_raw = sc.get(npolys * kN);
    uint64_t* d_pk = sc.get(npolys * n_digits * kN);
    if (!d_raw || !d_pk) return fail("device allocation failed");
    HIP_OK(hipMemset(d_raw, 0x5a, npolys * kN * sizeof(uint64_t)));
    hipEvent_t e[2];
    for (auto& x : e) HIP_OK(hipEventCreate(&x));
    const FwdJob digits = gadget_digits_job(d_raw, d_pk, (uint32_t)npolys, n_digits);
    launch_job(tb, digits, 0);  // warm
    HIP_OK(hipEventRecord(e[0], 0));
    for (int i = 0; i < iters; i++) launch_job(tb, digits, 0);
    HIP_OK(hipEventRecord(e[1], 0));
    HIP_OK(hipEventSynchronize(e[1]));
    HIP_OK(hipEventElapsedTime(ms, e[0], e[1]));
    *ms /= iters;
    for (auto& x : e) (void)hipEventDestroy(x);
    return 0;
}

int spiral_gpu_multiply(uint64_t* out, const uint64_t* a, const uint64_t* b, size_t rs, size_t ms, size_t cs) {
    Scratch sc;
    uint64_t* da = upload_pk(sc, a, rs * ms);
    uint64_t* db = upload_pk(sc, b, ms * cs);
    uint64_t* dout = sc.get(rs * cs * kN);
    if (!da || !db || !dout) return fail("device allocation/upload failed");
    MatmulParams mp{{da, db, dout, (uint32_t)rs, (uint32_t)ms, (uint32_t)cs, 0, 0, 0}, Lanes{}};
    launch_matmul(mp, 1, 0);
    return download_pk(sc, dout, identity_map(), out, rs * cs);
}

int spiral_gpu_add(uint64_t* out, const uint64_t* a, const uint64_t* b, size_t npolys) {
    Scratch sc;
    uint64_t* da = upload_pk(sc, a, npolys);
    uint64_t* db = upload_pk(sc, b, npolys);
    if (!da || !db) return fail("device allocation/upload failed");
    launch_add(da, db, da, (uint32_t)npolys, 0);
    return download_pk(sc, da, identity_map(), out, npolys);
}

int spiral_gpu_mul_by_const(uint64_t* out, const uint64_t* single_poly, const uint64_t* a, size_t npolys) {
    Scratch sc;
    uint64_t* ds = upload_pk(sc, single_poly, 1);
    uint64_t* da = upload_pk(sc, a, npolys);
    if (!ds || !da) return fail("device allocation/upload failed");
    launch_mul_by_const(ds, da, da, (uint32_t)npolys, 0);
    return download_pk(sc, da, identity_map(), out, npolys);
}

int spiral_gpu_automorph(uint64_t* out, const uint64_t* in, size_t npolys, uint64_t t) {
    if ((t & 1) == 0) return fail("automorphism exponent must be odd");
    Scratch sc;
    uint64_t* di = sc.upload(in, npolys * kN);
    uint64_t* dout = sc.get(npolys * kN);
    if (!di || !dout) return fail("device allocation/upload failed");
    launch_automorph(di, dout, (uint32_t)npolys, (uint32_t)t, 0);
    HIP_OK(hipMemcpy(out, dout, npolys * kN * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

int spiral_gpu_invert(uint64_t* out, const uint64_t* in, size_t npolys) {
    Scratch sc;
    uint64_t* di = sc.upload(in, npolys * kN);
    if (!di) return fail("device allocation/upload failed");
    launch_invert(di, di, (uint32_t)npolys, 0);
    HIP_OK(hipMemcpy(out, di, npolys * kN * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

int spiral_gpu_gadget_invert(uint64_t* out, const uint64_t* in, size_t mx, size_t rdim, size_t cols) {
    if (rdim == 0 || mx % rdim) return fail("mx must be a multiple of rdim");
    Scratch sc;
    uint64_t* di = sc.upload(in, rdim * cols * kN);
    uint64_t* dout = sc.get(mx * cols * kN);
    if (!di || !dout) return fail("device allocation/upload failed");
    launch_gadget_invert(di, dout, (uint32_t)mx, (uint32_t)rdim, (uint32_t)cols, 0);
    HIP_OK(hipMemcpy(out, dout, mx * cols * kN * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

int spiral_gpu_get_rescaled(uint64_t* out, const uint64_t* in, size_t n, uint64_t inp_mod, uint64_t out_mod) {
    Scratch sc;
    uint64_t* di = sc.upload(in, n);
    if (!di) return fail("device allocation/upload failed");
    launch_rescale(di, di, (uint32_t)n, inp_mod, out_mod, 0);
    HIP_OK(hipMemcpy(out, di, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

int spiral_gpu_multiply_query_by_database(uint64_t* output, const uint64_t* reorientedCiphertexts, const uint64_t* database, size_t dim0,
                                          size_t num_per) {
    if (dim0 == 0 || num_per == 0) return fail("empty geometry");
    Scratch sc;
    const size_t db_words = (size_t)kN * dim0 * num_per * 4;
    uint64_t* d_ref = sc.upload(database, db_words);
    uint64_t* d_db = sc.get(db_device_words((uint32_t)(2 * num_per), (uint32_t)dim0));
    uint64_t* d_re = sc.upload(reorientedCiphertexts, (size_t)kN * dim0 * 8);
    uint64_t* d_qs = sc.get((size_t)kN * dim0 * 6);
    uint64_t* d_acc = sc.get(num_per * 6 * kN);
    if (!d_ref || !d_db || !d_re || !d_qs || !d_acc) return fail("device allocation/upload failed");
    launch_db_relayout(d_ref, d_db, (uint32_t)num_per, (uint32_t)dim0, 0, (uint32_t)dim0, 0, kN, 0);
    launch_qs_from_reoriented(d_re, (uint32_t*)d_qs, (uint32_t)(2 * dim0), 0);
    launch_sweep(d_db, (const uint32_t*)d_qs, d_acc, (uint32_t)num_per, (uint32_t)(2 * dim0), 0, 0);
    return download_pk(sc, d_acc, identity_map(), output, num_per * 6);
}

int spiral_gpu_multiply_queries_by_database(uint64_t* outputs, const uint64_t* reorientedCiphertexts, size_t n, const uint64_t* database, size_t dim0,
                                            size_t num_per) {
    if (dim0 == 0 || num_per == 0 || n == 0) return fail("empty geometry");
    if (n > kMaxLanes) return fail("at most %u queries per pass", kMaxLanes);
    Scratch sc;
    const size_t db_words = (size_t)kN * dim0 * num_per * 4, dev_words = db_device_words((uint32_t)(2 * num_per), (uint32_t)dim0);
    const bool mfma = DbLayout::base((uint32_t)num_per, (uint32_t)dim0).limbs_ok();  // (below 64 ciphertexts per slot: option sweep_narrow)
    uint64_t* d_ref = sc.upload(database, db_words);
    uint64_t* d_db = sc.get(dev_words);
    uint64_t* d_limbs = mfma ? sc.get(dev_words) : nullptr;
    uint64_t* d_re = sc.upload(reorientedCiphertexts, n * (size_t)kN * dim0 * 8);
    uint64_t* d_qs = sc.get(n * (size_t)kN * dim0 * 6);
    uint64_t* d_acc = sc.get(n * num_per * 6 * kN);
    if (!d_ref || !d_db || (mfma && !d_limbs) || !d_re || !d_qs || !d_acc) return fail("device allocation/upload failed");
    launch_db_relayout(d_ref, d_db, (uint32_t)num_per, (uint32_t)dim0, 0, (uint32_t)dim0, 0, kN, 0);
    if (mfma) launch_db_limb_planes(d_db, d_limbs, (uint32_t)num_per, (uint32_t)(2 * dim0), 0);
    const uint32_t* qs[kMaxLanes];
    uint64_t* acc[kMaxLanes];
    for (size_t b = 0; b < n; b++) {
        qs[b] = (const uint32_t*)(d_qs + b * (size_t)kN * dim0 * 6);
        acc[b] = d_acc + b * num_per * 6 * kN;
        launch_qs_from_reoriented(d_re + b * (size_t)kN * dim0 * 8, (uint32_t*)qs[b], (uint32_t)(2 * dim0), 0);
    }
    if (sweep_queries(d_db, d_limbs, (uint32_t)num_per, (uint32_t)(2 * dim0), qs, acc, (uint32_t)n, 0, 0)) return -1;
    return download_pk(sc, d_acc, identity_map(), outputs, n * num_per * 6);
}

int spiral_gpu_split_and_crt(uint64_t* out, const uint64_t* in, size_t num_per, uint32_t t_gsw) {
    DeviceTables tb;
    if (current_tables(&tb)) return -1;
    Scratch sc;
    const uint32_t m2 = 3 * t_gsw;
    uint64_t* di = sc.upload(in, num_per * 6 * kN);
    uint64_t* dd = sc.get(num_per * 2 * m2 * 2 * kN);  // fold operand layout, only the low halves are filled
    if (!di || !dd) return fail("device allocation/upload failed");
    launch_job(tb, fold_digits_job(LD_SDIGIT, di, dd, (uint32_t)(num_per * 6), t_gsw, (uint32_t)num_per), 0);  // np = num_per: every ct index < num_per -> low half
    // D[i][row][c] at (i*2*m2 + row)*2 + c  ->  reference [i][row][c]
    return download_pk(sc, dd, IndexMap{2 * m2, 4 * m2, 0}, out, num_per * m2 * 2);
}

int spiral_gpu_fold_one_further_dimension(uint64_t* cts, size_t num_per, const uint64_t* query_ct, const uint64_t* query_ct_neg,
                                          uint32_t t_gsw) {
    DeviceTables tb;
    if (current_tables(&tb)) return -1;
    Scratch sc;
    const uint32_t m2 = 3 * t_gsw;
    uint64_t* d_cts = sc.upload(cts, 2 * num_per * 6 * kN);
    uint64_t* d_q = sc.upload(query_ct, (size_t)kN * 3 * m2);
    uint64_t* d_qn = sc.upload(query_ct_neg, (size_t)kN * 3 * m2);
    uint64_t* d_key = sc.get((size_t)3 * 2 * m2 * kN);
    uint64_t* d_d = sc.get(num_per * 2 * m2 * 2 * kN);
    uint64_t* d_c = sc.get(num_per * 6 * kN);
    if (!d_cts || !d_q || !d_qn || !d_key || !d_d || !d_c) return fail("device allocation/upload failed");
    launch_fold_key_from_reoriented(d_q, d_qn, d_key, m2, 0);
    launch_job(tb, fold_digits_job(LD_SDIGIT, d_cts, d_d, (uint32_t)(2 * num_per * 6), t_gsw, (uint32_t)num_per), 0);
    launch_fold_mac(d_key, d_d, d_c, 2 * m2, (uint32_t)num_per, 0);
    launch_job(tb, lift_job(d_c, d_cts, (uint32_t)(num_per * 6)), 0);
    HIP_OK(hipMemcpy(cts, d_cts, num_per * 6 * kN * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

int spiral_gpu_expand_improved(uint64_t* cv_v, uint32_t g, uint32_t t_exp, const uint64_t* w_left, uint32_t t_exp_right,
                               const uint64_t* w_right, uint32_t n_right, uint32_t max_bits_to_gen_right, uint32_t stopround) {
    DeviceTables tb;
    if (current_tables(&tb)) return -1;
    if (g == 0 || g > kLogN) return fail("g out of range");
    const uint32_t need_right = stopround ? stopround + 1 : g;
    if (n_right < need_right) return fail("W_exp_right has %u matrices, %u needed", n_right, need_right);
    Scratch sc;
    const size_t ncv = (size_t)1 << g;
    uint64_t* d_cv = upload_pk(sc, cv_v, ncv * 2);
    uint64_t* d_wl = upload_pk(sc, w_left, (size_t)g * 2 * t_exp);
    uint64_t* d_wr = upload_pk(sc, w_right, (size_t)n_right * 2 * t_exp_right);
    ExpandWork wk{sc.get(ncv * 2 * kN), sc.get(expand_g_polys(g, t_exp, t_exp_right) * kN)};
    if (!d_cv || !d_wl || !d_wr || !wk.raw || !wk.g) return fail("device allocation/upload failed");
    run_expand(tb, d_cv, g, t_exp, d_wl, t_exp_right, d_wr, max_bits_to_gen_right, stopround, wk, 0);
    return download_pk(sc, d_cv, identity_map(), cv_v, ncv * 2);
}

int spiral_gpu_scal_to_mat(uint64_t* out, const uint64_t* cv, const uint64_t* w, uint32_t t_conv) {
    DeviceTables tb;
    if (current_tables(&tb)) return -1;
    Scratch sc;
    uint64_t* d_cv = upload_pk(sc, cv, 2);
    uint64_t* d_w = upload_pk(sc, w, (size_t)3 * 2 * t_conv);
    uint64_t* d_raw = sc.get(kN);
    uint64_t* d_g = sc.get((size_t)t_conv * kN);
    uint64_t* d_out = sc.get((size_t)6 * kN);
    if (!d_cv || !d_w || !d_raw || !d_g || !d_out) return fail("device allocation/upload failed");
    launch_job(tb, lift_job(d_cv, d_raw, 1), 0);
    launch_job(tb, gadget_digits_job(d_raw, d_g, 1, t_conv), 0);
    Scal2MatParams sp{};
    sp.w = d_w;
    sp.g = d_g;
    sp.cv = d_cv;
    sp.cv_pos = identity_map();
    sp.out = d_out;
    sp.t_conv = t_conv;
    sp.count = 1;
    launch_scal2mat(sp, 0);
    return download_pk(sc, d_out, identity_map(), out, 6);
}

int spiral_gpu_regev_to_gsw(uint64_t* out, const uint64_t* cv_v, const uint64_t* w, const uint64_t* v, uint32_t t_conv, uint32_t ell) {
    DeviceTables tb;
    if (current_tables(&tb)) return -1;
    Scratch sc;
    uint64_t* d_cv = upload_pk(sc, cv_v, (size_t)ell * 2);
    uint64_t* d_w = upload_pk(sc, w, (size_t)3 * 2 * t_conv);
    uint64_t* d_v = upload_pk(sc, v, (size_t)3 * 2 * t_conv);
    uint64_t* d_raw = sc.get((size_t)ell * 2 * kN);
    uint64_t* d_chat = sc.get((size_t)ell * 2 * t_conv * kN);
    uint64_t* d_gsw = sc.get((size_t)3 * 3 * ell * kN);
    if (!d_cv || !d_w || !d_v || !d_raw || !d_chat || !d_gsw) return fail("device allocation/upload failed");
    launch_job(tb, lift_job(d_cv, d_raw, 2 * ell), 0);
    launch_job(tb, gadget_digits_job(d_raw, d_chat, 2 * ell, t_conv), 0);
    GswParams gp{};
    gp.w = d_w;
    gp.v = d_v;
    gp.chat = d_chat;
    gp.cv = d_cv;
    gp.cv_pos = identity_map();
    gp.gsw = d_gsw;
    gp.t_conv = t_conv;
    gp.ell = ell;
    gp.dims = 1;
    launch_regev_to_gsw(gp, 0);
    return download_pk(sc, d_gsw, identity_map(), out, (size_t)9 * ell);
}

size_t spiral_gpu_query_wire_bytes(const spiral_gpu_params* p) { return base_message_bytes(p, query_layout, FORM_WIRE); }
size_t spiral_gpu_query_seeded_bytes(const spiral_gpu_params* p) { return base_message_bytes(p, query_layout, FORM_SEEDED); }
size_t spiral_gpu_pub_params_wire_bytes(const spiral_gpu_params* p) { return base_message_bytes(p, pub_params_layout, FORM_WIRE); }
size_t spiral_gpu_pub_params_seeded_bytes(const spiral_gpu_params* p) { return base_message_bytes(p, pub_params_layout, FORM_SEEDED); }

// the client's half of the seeded form: row-0 polynomials first_k .. first_k + npolys - 1 of `domain` in reference NTT layout, plain host code
// through the same definition as the device's generator (seed_device.h)
int spiral_gpu_seed_expand(const void* seed32, uint32_t domain, uint64_t first_k, size_t npolys, uint64_t* out) {
    if (!seed32 || (!out && npolys)) return fail("seed_expand: null argument");
    const Seed key = seed_words((const uint8_t*)seed32);
    for (size_t j = 0; j < npolys; j++) {
        uint64_t* o = out + j * kRefNtt;
        for (uint32_t c = 0; c < kN / 2; c++) {
            uint64_t r[2];
            seed_slot_pair(key.w, domain, first_k + j, c, r);
            for (uint32_t h = 0; h < 2; h++) {
                o[2 * c + h] = (uint32_t)r[h];
                o[kN + 2 * c + h] = r[h] >> 32;
            }
        }
    }
    return 0;
}

// the client's half of the wire form: plain host code, no device involved
int spiral_gpu_raw_to_wire(const uint64_t* raw, size_t npolys, void* wire) {
    if (!raw || !wire) return fail("raw_to_wire: null argument");
    const size_t n = npolys * kN;
    for (size_t i = 0; i < n; i++)  // checked before anything is written
        if (raw[i] > kQ)
            return fail("raw_to_wire: coefficient %zu (polynomial %zu, index %zu) is %llu, above Q", i, i / kN, i % kN, (unsigned long long)raw[i]);
    uint8_t* b = (uint8_t*)wire;
    for (size_t i = 0; i < n; i++, b += kWireCoeffBytes)
        for (uint32_t k = 0; k < kWireCoeffBytes; k++) b[k] = (uint8_t)(raw[i] >> (8 * k));
    return 0;
}

int spiral_gpu_raw_from_wire(const void* wire, size_t npolys, uint64_t* raw) {
    if (!raw || !wire) return fail("raw_from_wire: null argument");
    const uint8_t* b = (const uint8_t*)wire;
    const size_t n = npolys * kN;
    for (size_t i = 0; i < n; i++, b += kWireCoeffBytes) {
        uint64_t v = 0;
        for (uint32_t k = 0; k < kWireCoeffBytes; k++) v |= (uint64_t)b[k] << (8 * k);
        raw[i] = v;
    }
    return 0;
}

size_t spiral_gpu_response_wire_bytes(const spiral_gpu_params* p, uint32_t out_n) {
    if (!p || out_n < 1 || out_n > 16 || p->qprime_bits < 1 || p->qprime_bits > 36 || p->p_db < 2 || p->p_db > (1ull << 40)) return 0;
    return wire_bytes(p, out_n);
}

// bytes of n items in the item stream of load_db_items / read_db_items (host only)
size_t spiral_gpu_db_items_bytes(const spiral_gpu_params* p, uint32_t out_n, uint32_t coeff_bits, uint64_t n_items) {
    if (!p) return fail("null argument"), 0;
    if (check_export_width(coeff_bits, p->p_db)) return 0;
    return (size_t)n_items * (out_n ? 1u : 4u) * (kN / 8u) * coeff_bits;
}

// ---- fingerprints on the host (include/spiral_gpu.h "Fingerprints"): the function the device computes, from a bit-packed item stream -------------
int spiral_gpu_fingerprint_host(const uint64_t* key, uint64_t p_db, const void* items, uint32_t coeff_bits, uint32_t polys_per_item, uint32_t poly0,
                                uint32_t n_polys, uint64_t first_item, uint64_t n_items, uint64_t* per_item, uint64_t* combined) {
    if (!key || (!items && n_items && n_polys)) return fail("null argument");
    if (!per_item && !combined) return fail("per_item and combined are both null: nothing to compute");
    if (p_db < 2 || p_db > kFpP) return fail("p_db = %llu is not in [2, 2^61 - 1]", (unsigned long long)p_db);
    if (check_export_width(coeff_bits, p_db)) return -1;
    if (polys_per_item < 1 || polys_per_item > kFpMaxPolys) return fail("polys_per_item = %u is not in 1..%u", polys_per_item, kFpMaxPolys);
    if (poly0 > polys_per_item || n_polys > polys_per_item - poly0)
        return fail("polynomials [%u, +%u) outside an item of %u", poly0, n_polys, polys_per_item);
    if (first_item > ~0ull - n_items) return fail("items [%llu, +%llu) overflow the index", (unsigned long long)first_item, (unsigned long long)n_items);
    std::vector<uint64_t> w(kFpWeightWords);
    fp_build_weights(key, w.data());
    const size_t poly_bytes = (size_t)(kN / 8u) * coeff_bits;
    const uint64_t mask = coeff_bits == 64 ? ~0ull : (1ull << coeff_bits) - 1;
    const uint8_t* b = static_cast<const uint8_t*>(items);
    uint64_t F = 0;
    for (uint64_t k = 0; k < n_items; k++) {
        uint64_t f = 0;
        for (uint32_t q = 0; q < n_polys; q++, b += poly_bytes) {
            uint64_t acc = 0;
            size_t bit = 0;
            for (uint32_t c = 0; c < kN; c++, bit += coeff_bits) {
                unsigned __int128 raw = 0;  // up to 64 + 7 bits from a byte boundary, inside the polynomial's own bytes
                const size_t first = bit / 8;
                for (size_t u = 0; u < 9 && first + u < poly_bytes; u++) raw |= (unsigned __int128)b[first + u] << (8 * u);
                const uint64_t x = (uint64_t)(raw >> (bit % 8)) & mask;
                if (x >= p_db)
                    return fail("coefficient %u of polynomial %u of item %llu is %llu: not below p_db = %llu", c, poly0 + q, (unsigned long long)(first_item + k),
                                (unsigned long long)x, (unsigned long long)p_db);
                acc = fp_add(acc, fp_mul(x, w[c]));
            }
            f = fp_add(f, fp_mul(acc, w[kFpW_Poly + poly0 + q]));
        }
        if (per_item) per_item[k] = f;
        F = fp_add(F, fp_mul(f, fp_pow_s(w.data() + kFpW_S, first_item + k + 1)));
    }
    if (combined) *combined = F;
    return 0;
}
// f and F from a table of polynomial sums g (include/spiral_gpu.h "Fingerprints", Tracked): poly_sums[k * n_polys + q] = g(first_item + k, poly0 + q)
int spiral_gpu_fingerprint_of_polys(const uint64_t* key, const uint64_t* poly_sums, uint32_t polys_per_item, uint32_t poly0, uint32_t n_polys, uint64_t first_item,
                                    uint64_t n_items, uint64_t* per_item, uint64_t* combined) {
    if (!key || (!poly_sums && n_items && n_polys)) return fail("null argument");
    if (!per_item && !combined) return fail("per_item and combined are both null: nothing to compute");
    if (polys_per_item < 1 || polys_per_item > kFpMaxPolys) return fail("polys_per_item = %u is not in 1..%u", polys_per_item, kFpMaxPolys);
    if (poly0 > polys_per_item || n_polys > polys_per_item - poly0)
        return fail("polynomials [%u, +%u) outside an item of %u", poly0, n_polys, polys_per_item);
    if (first_item > ~0ull - n_items) return fail("items [%llu, +%llu) overflow the index", (unsigned long long)first_item, (unsigned long long)n_items);
    std::vector<uint64_t> w(kFpWeightWords);
    fp_build_weights(key, w.data());
    uint64_t F = 0;
    for (uint64_t k = 0; k < n_items; k++) {
        uint64_t f = 0;
        for (uint32_t q = 0; q < n_polys; q++) {
            const uint64_t g = poly_sums[k * n_polys + q];
            if (g >= kFpP)
                return fail("the sum of polynomial %u of item %llu is %llu: not below 2^61 - 1", poly0 + q, (unsigned long long)(first_item + k), (unsigned long long)g);
            f = fp_add(f, fp_mul(g, w[kFpW_Poly + poly0 + q]));
        }
        if (per_item) per_item[k] = f;
        F = fp_add(F, fp_mul(f, fp_pow_s(w.data() + kFpW_S, first_item + k + 1)));
    }
    if (combined) *combined = F;
    return 0;
}
uint64_t spiral_gpu_fingerprint_add(uint64_t a, uint64_t b) {
    if (a >= kFpP || b >= kFpP) return fail("a fingerprint is below 2^61 - 1: %llu is none", (unsigned long long)(a >= kFpP ? a : b)), kFpP;
    return fp_add(a, b);
}

// client side of the wire form (load_modswitched_into_ct, src/client.cpp:90-110): plain host code, no device involved
int spiral_gpu_response_from_wire(const spiral_gpu_params* p, uint32_t out_n, const void* wire, uint64_t* response) {
    if (!p || !wire || !response) return fail("null argument");
    if (spiral_gpu_response_wire_bytes(p, out_n) == 0) return fail("unsupported parameters for the wire form");
    const uint8_t* b = (const uint8_t*)wire;
    const size_t total = wire_bytes(p, out_n);
    size_t bit = 0;
    for (uint32_t r = 0; r <= out_n; r++) {
        const uint32_t w = r == 0 ? p->qprime_bits : wire_bits_rest(p);
        for (size_t i = 0; i < (size_t)out_n * kN; i++, bit += w) {
            unsigned __int128 acc = 0;  // up to 42 + 7 bits starting at a byte boundary
            const size_t first = bit / 8;
            for (size_t k = 0; k < 8 && first + k < total; k++) acc |= (unsigned __int128)b[first + k] << (8 * k);
            response[(size_t)r * out_n * kN + i] = (uint64_t)(acc >> (bit % 8)) & ((1ull << w) - 1);
        }
    }
    return 0;
}

}  // extern "C"
