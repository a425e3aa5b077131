// Records on the host side: the layout of include/spiral_gpu.h "Records" as code, the repacking of load_records, and the shared bodies of
// update_records and read_records / read_records_at (records.hip does the device work, db_update.hip the scatter).  Internal to libspiral_gpu.so.
#pragma once
#include "host_common.h"

namespace spiral {
namespace host {

// out_n = 0: a base parameter set (4 polynomials per item); out_n >= 1: SpiralPack, out_n^2 polynomials per item, one per trial image
inline int record_layout(const spiral_gpu_params* p, uint64_t record_bytes, spiral_gpu_record_layout* out, uint32_t out_n = 0) {
    if (!p || !out) return fail("null argument");
    if (out_n > 16) return fail("out_n out of range");
    if (out_n && (p->nu1 < 1 || p->nu2 < 1)) return fail("SpiralPack needs nu1 >= 1 and nu2 >= 1");
    spiral_gpu_shape s;
    spiral_gpu_params q = *p;
    q.direct_upload = 1;  // the layout does not depend on how the query arrives: no query-size rule here
    if (shape_of(&q, &s)) return -1;
    if (record_bytes < 1) return fail("a record has at least one byte");
    uint32_t w = 0;
    while ((2ull << w) <= p->p_db) w++;  // floor(log2 p_db)
    const uint64_t item_bytes = (out_n ? (uint64_t)out_n * out_n : 4ull) * 256u * w;
    spiral_gpu_record_layout l{};
    l.coeff_bits = w;
    l.item_bytes = item_bytes;
    if (record_bytes <= item_bytes) {
        l.per_item = item_bytes / record_bytes;
        l.instances = 1;
    } else {
        const uint64_t inst = (record_bytes + item_bytes - 1) / item_bytes;
        if (inst > 16) return fail("a record of %llu bytes takes %llu instances of %llu-byte items: at most 16", (unsigned long long)record_bytes,
                                   (unsigned long long)inst, (unsigned long long)item_bytes);
        l.per_item = 1;
        l.instances = (uint32_t)inst;
    }
    l.capacity = (uint64_t)s.dim0 * s.num_per * l.per_item;
    *out = l;
    return 0;
}

// the chunk of a record that instance f holds: bytes [first, first + len) of the record, at byte 0 of its item (one instance: the whole record)
struct RecordChunk {
    uint64_t first, len;
};
inline int record_chunk(const spiral_gpu_record_layout& l, uint64_t record_bytes, uint32_t instance, RecordChunk* c) {
    if (instance >= l.instances) return fail("instance %u of a record of %u instance%s", instance, l.instances, l.instances == 1 ? "" : "s");
    c->first = (uint64_t)instance * l.item_bytes;
    c->len = std::min<uint64_t>(record_bytes - c->first, l.item_bytes);
    if (l.instances == 1) c->len = record_bytes;
    return 0;
}

// `count` coefficients of w_in bits, bit-packed little-endian at src, as w_out-bit ones at dst (zeroed by the caller; w_out >= w_in)
inline void widen_coeffs(const uint8_t* src, uint8_t* dst, size_t count, uint32_t w_in, uint32_t w_out) {
    for (size_t i = 0; i < count; i++) {
        uint64_t v = 0;
        for (uint32_t b = 0; b < w_in; b++) {
            const uint64_t bit = (uint64_t)i * w_in + b;
            v |= (uint64_t)((src[bit >> 3] >> (bit & 7u)) & 1u) << b;
        }
        for (uint32_t b = 0; b < w_in; b++) {
            const uint64_t bit = (uint64_t)i * w_out + b;
            dst[bit >> 3] |= (uint8_t)(((v >> b) & 1u) << (bit & 7u));
        }
    }
}

// One staged record (or chunk) and the item bytes it maps to: staged record k is bytes [off, off + len) of the stream of image item (j local, ii)
struct RecordPiece {
    uint64_t pos;  // position in the caller's list
    uint32_t j, ii;
    uint32_t off, len;
};
// The device tables of kernels.h RecordWorkParams for pieces[k0, k0 + cnt), staged at (k - k0) * stride.  Items in (j, ii) order.  all_polys (update):
// four entries per touched item, in polynomial order, kRecordFull where the segments cover the polynomial, and `items` gets one UpdateItem per
// touched item; otherwise only the touched polynomials get an entry.  Returns true when some entry has to gather (update: a read-modify-write).
// buf_of(k): where piece k0 + k is staged, for a staging that is not k * stride (the client's decode: whole records, a chunk per response).
template <class BufOf>
inline bool record_tables(const std::vector<RecordPiece>& pieces, size_t k0, size_t cnt, uint32_t w, bool all_polys, std::vector<uint4>& entries,
                          std::vector<uint4>& segs, std::vector<UpdateItem>* items, BufOf buf_of) {
    const uint32_t poly_bytes = 256u * w;
    std::vector<uint32_t> order(cnt);
    for (size_t k = 0; k < cnt; k++) order[k] = (uint32_t)k;
    auto key = [&](uint32_t k) { return ((uint64_t)pieces[k0 + k].j << 32) | pieces[k0 + k].ii; };
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
    bool gathers = false;
    for (size_t a = 0; a < cnt;) {
        size_t b = a;
        while (b < cnt && key(order[b]) == key(order[a])) b++;
        const RecordPiece& first = pieces[k0 + order[a]];
        if (items) items->push_back(UpdateItem{items->size(), first.j, first.ii});
        for (uint32_t mc = 0; mc < 4; mc++) {
            const uint32_t p0 = mc * poly_bytes, p1 = p0 + poly_bytes, seg0 = (uint32_t)segs.size();
            uint64_t covered = 0;
            for (size_t x = a; x < b; x++) {
                const RecordPiece& pc = pieces[k0 + order[x]];
                const uint32_t lo = std::max(pc.off, p0), hi = std::min(pc.off + pc.len, p1);
                if (lo >= hi) continue;
                const uint64_t buf = buf_of(order[x]) + (lo - pc.off);
                segs.push_back(make_uint4(lo - p0, hi - lo, (uint32_t)buf, (uint32_t)(buf >> 32)));
                covered += hi - lo;
            }
            const uint32_t nseg = (uint32_t)segs.size() - seg0;
            if (!all_polys && nseg == 0) continue;
            const bool full = all_polys && covered == poly_bytes;
            if (nseg && !full) gathers = true;
            entries.push_back(make_uint4(first.j | (mc << kRecordPolyShift) | (full ? kRecordFull : 0u), first.ii, seg0, nseg));
        }
        a = b;
    }
    return gathers;
}
inline bool record_tables(const std::vector<RecordPiece>& pieces, size_t k0, size_t cnt, uint32_t stride, uint32_t w, bool all_polys, std::vector<uint4>& entries,
                          std::vector<uint4>& segs, std::vector<UpdateItem>* items) {
    return record_tables(pieces, k0, cnt, w, all_polys, entries, segs, items, [&](uint32_t k) { return (uint64_t)k * stride; });
}

// The trial images a SpiralPack record call works on (include/spiral_gpu.h "Records", SpiralPack): an item's polynomial t is its plaintext in trial t,
// the server holds the global trials [t0, t0 + nt) back to back, trial_words words apart.  trials = 0: a base image.
struct RecordTrials {
    uint32_t trials = 0, t0 = 0, nt = 0;
    uint64_t trial_words = 0;
};
// record_tables for trial images (kernels.h PackRecordWorkParams): one entry per polynomial that a piece touches AND the server holds, in (j, ii, trial)
// order, kRecordFull (update) where the segments cover it.  Polynomials nothing touches have no entry: the scatter writes single polynomials.
template <class BufOf>
inline bool pack_record_tables(const std::vector<RecordPiece>& pieces, size_t k0, size_t cnt, uint32_t w, const RecordTrials& tr, bool update,
                               std::vector<uint4>& entries, std::vector<uint4>& segs, BufOf buf_of) {
    const uint32_t poly_bytes = 256u * w;
    struct Touch {
        uint64_t item;
        uint32_t t, k;
    };
    std::vector<Touch> touch;
    for (size_t k = 0; k < cnt; k++) {
        const RecordPiece& pc = pieces[k0 + k];
        if (pc.len == 0) continue;
        const uint32_t ta = std::max(pc.off / poly_bytes, tr.t0), tb = std::min((pc.off + pc.len - 1u) / poly_bytes + 1u, tr.t0 + tr.nt);
        for (uint32_t t = ta; t < tb; t++) touch.push_back(Touch{((uint64_t)pc.j << 32) | pc.ii, t, (uint32_t)k});
    }
    std::stable_sort(touch.begin(), touch.end(), [](const Touch& a, const Touch& b) { return a.item != b.item ? a.item < b.item : a.t < b.t; });
    bool gathers = false;
    for (size_t a = 0; a < touch.size();) {
        const uint32_t t = touch[a].t, p0 = t * poly_bytes, p1 = p0 + poly_bytes, seg0 = (uint32_t)segs.size();
        uint64_t covered = 0;
        size_t b = a;
        for (; b < touch.size() && touch[b].item == touch[a].item && touch[b].t == t; b++) {
            const RecordPiece& pc = pieces[k0 + touch[b].k];
            const uint32_t lo = std::max(pc.off, p0), hi = std::min(pc.off + pc.len, p1);
            const uint64_t buf = buf_of(touch[b].k) + (lo - pc.off);
            segs.push_back(make_uint4(lo - p0, hi - lo, (uint32_t)buf, (uint32_t)(buf >> 32)));
            covered += hi - lo;
        }
        const bool full = update && covered == poly_bytes;
        if (!full) gathers = true;
        entries.push_back(make_uint4((uint32_t)(touch[a].item >> 32) | (full ? kRecordFull : 0u), (uint32_t)touch[a].item | ((t - tr.t0) << kPackRecordTrialShift), seg0,
                                     (uint32_t)segs.size() - seg0));
        a = b;
    }
    return gathers;
}
// the scatter's work entries (kernels.h DbUpdateTrialsParams) for the entries of pack_record_tables, entry e = encoded polynomial e
inline void pack_update_entries(const std::vector<uint4>& entries, const UpdateImage& img, std::vector<uint4>& put, std::vector<uint4>& pairs) {
    const size_t n = entries.size();
    auto row = [&](size_t e) { return entries[e].x & kRecordRowMask; };
    if (img.packed) {
        put.reserve(n);
        for (size_t e = 0; e < n; e++) put.push_back(make_uint4((uint32_t)e, row(e), entries[e].y & kPackRecordColMask, entries[e].y >> kPackRecordTrialShift));
    }
    if (img.limbs) {
        std::vector<std::pair<uint64_t, uint32_t>> order(n);  // (column | trial, j of the low partner) -> entry
        for (size_t e = 0; e < n; e++) order[e] = {((uint64_t)entries[e].y << 32) | (row(e) & ~64u), (uint32_t)e};
        std::sort(order.begin(), order.end());
        for (size_t k = 0; k < n; k++) {
            const uint64_t key = order[k].first;
            if (pairs.empty() || (((uint64_t)pairs.back().x << 32) | pairs.back().y) != key)
                pairs.push_back(make_uint4((uint32_t)(key >> 32), (uint32_t)key, kDbUpdateNone, kDbUpdateNone));
            const uint32_t e = order[k].second;
            (row(e) & 64u ? pairs.back().w : pairs.back().z) = e;
        }
    }
}

// the failure a record kernel reports through its error word (kernels.h RecordWorkParams, PackRecordWorkParams)
template <class RecordOf>
inline int record_image_error(unsigned long long err, RecordOf record_of, const RecordTrials& tr = RecordTrials{}) {
    if (tr.trials) {
        const uint64_t poly = err / kN;
        return fail("the image holds no record data at record %llu (trial %u, coefficient %u is no plaintext value below 2^coeff_bits): not a record "
                    "database (fill_db_random, a load_db of arbitrary words, or items loaded with larger coefficients)",
                    (unsigned long long)record_of(poly / tr.trials), (uint32_t)(poly % tr.trials), (uint32_t)(err % kN));
    }
    const uint64_t poly = err / kN, k = poly / 4;
    return fail("the image holds no record data at record %llu (polynomial %u, coefficient %u is no plaintext value below 2^coeff_bits): not a record "
                "database (fill_db_random, a load_db of arbitrary words, or items loaded with larger coefficients)",
                (unsigned long long)record_of(k), (uint32_t)(poly % 4), (uint32_t)(err % kN));
}

// The shared body of update_records: `pieces` are the records (chunks) this image holds, piece k's bytes at records + pos * record_bytes + chunk.first.
// ONE upload, ONE read-modify-write launch (records.hip) and ONE scatter launch (db_update.hip) on `st`.  Where every touched polynomial is covered
// whole or not at all nothing of the image has to be read and the call returns as update_db_items does; otherwise it waits for `st` to read the
// error word, and a coefficient that is no record data fails the call with the image untouched (the scatter skips everything).
template <class RecordOf>
inline int update_record_pieces(UpdateWork& W, const DeviceTables& tb, hipStream_t st, const uint8_t* records, uint64_t record_bytes, const RecordChunk& chunk,
                                uint32_t w, uint64_t p_db, const std::vector<RecordPiece>& pieces, const UpdateImage& img, const ExportImage& src, RecordOf record_of,
                                const RecordTrials& tr = RecordTrials{}, const FpTrackCtx* trk = nullptr) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_OK(hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail("update_records cannot be called while the server's stream is being captured");
    if (pieces.empty()) return 0;
    const uint32_t stride = (uint32_t)chunk.len;
    const size_t n = pieces.size();
    std::vector<uint4> entries, segs, put, pairs;
    std::vector<UpdateItem> items;
    bool gathers;
    if (tr.trials) {
        gathers = pack_record_tables(pieces, 0, n, w, tr, true, entries, segs, [&](uint32_t k) { return (uint64_t)k * stride; });
        if (entries.empty()) return 0;  // (a trial shard that holds none of the touched polynomials)
        pack_update_entries(entries, img, put, pairs);
    } else {
        gathers = record_tables(pieces, 0, n, stride, w, true, entries, segs, &items);
        update_entries(items, img, put, pairs);
    }
    // one buffer: [flag, error word][entries][put][pairs][segments][record bytes] ++ (device only) [encoded polynomials]
    // a tracked image: [..][record bytes][apply entries] ++ (device only) [encoded polynomials][new polynomial sums]
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t o_ent = 16, o_put = o_ent + entries.size() * sizeof(uint4), o_pairs = o_put + put.size() * sizeof(uint4);
    const size_t o_segs = o_pairs + pairs.size() * sizeof(uint4), o_rec = o_segs + segs.size() * sizeof(uint4);
    const size_t o_app = up16(o_rec + n * stride + 16), n_app = trk ? entries.size() : 0;
    const size_t up_bytes = o_app + n_app * sizeof(ulonglong2), o_gnew = up_bytes + entries.size() * kPolyBytes, dev_bytes = o_gnew + n_app * 8;
    if (update_reserve(W, tr.trials ? entries.size() : items.size(), up_bytes, dev_bytes)) return -1;
    uint64_t n_touched = 0;  // table words this call replaces: the entries with segments
    if (trk) {
        ulonglong2* app = reinterpret_cast<ulonglong2*>(W.host + o_app);
        for (size_t e = 0; e < n_app; e++) {
            // (base: entry 4 k + mc is polynomial mc of touched item k; SpiralPack: the entry names row, column and local trial, one polynomial per trial)
            const uint32_t j = tr.trials ? entries[e].x & kRecordRowMask : items[e / 4].j, ii = tr.trials ? entries[e].y & kPackRecordColMask : items[e / 4].ii;
            const uint32_t m = tr.trials ? entries[e].y >> kPackRecordTrialShift : (uint32_t)(e & 3u);
            const bool skip = entries[e].w == 0;
            app[e] = make_ulonglong2(skip ? kFpApplySkip : trk->db_index(j, ii), trk->entry_y(j, ii, img.num_per, m));
            n_touched += skip ? 0 : 1;
        }
    }
    memset(W.host, 0, 8);
    memset(W.host + 8, 0xFF, 8);  // the error word: ~0 = every coefficient read so far is record data
    memcpy(W.host + o_ent, entries.data(), entries.size() * sizeof(uint4));
    if (!put.empty()) memcpy(W.host + o_put, put.data(), put.size() * sizeof(uint4));
    if (!pairs.empty()) memcpy(W.host + o_pairs, pairs.data(), pairs.size() * sizeof(uint4));
    memcpy(W.host + o_segs, segs.data(), segs.size() * sizeof(uint4));
    for (size_t k = 0; k < n; k++) memcpy(W.host + o_rec + k * stride, records + pieces[k].pos * record_bytes + chunk.first, stride);
    uint8_t* d = reinterpret_cast<uint8_t*>(W.dev.p);
    HIP_OK(hipMemcpyAsync(d, W.host, up_bytes, hipMemcpyHostToDevice, st));
    RecordWorkParams rp{};
    rp.db = src.db;
    rp.entries = reinterpret_cast<const uint4*>(d + o_ent);
    rp.segs = reinterpret_cast<const uint4*>(d + o_segs);
    rp.buf = d + o_rec;
    rp.enc = reinterpret_cast<uint64_t*>(d + up_bytes);
    rp.err = reinterpret_cast<unsigned long long*>(d + 8);
    rp.flag = reinterpret_cast<uint32_t*>(d);
    rp.n_entries = (uint32_t)entries.size();
    rp.form = src.form;
    rp.num_per = src.num_per;
    rp.dim0 = src.dim0;
    rp.w = w;
    rp.stride = stride;
    rp.p_db = p_db;
    const RecordTrackParams tk{trk ? trk->t->weights() : nullptr, reinterpret_cast<uint64_t*>(d + o_gnew)};
    if (tr.trials)
        trk ? launch_pack_record_update_tracked(tb, PackRecordWorkParams{rp, tr.trial_words, tr.trials, tr.t0}, tk, st)
            : launch_pack_record_update(tb, PackRecordWorkParams{rp, tr.trial_words, tr.trials, tr.t0}, st);
    else
        trk ? launch_record_update_tracked(tb, rp, tk, st) : launch_record_update(tb, rp, st);
    DbUpdateParams up{};
    up.enc = rp.enc;
    up.err = rp.flag;
    up.packed = img.packed;
    up.limbs = img.limbs;
    up.put = reinterpret_cast<const uint4*>(d + o_put);
    up.pairs = reinterpret_cast<const uint4*>(d + o_pairs);
    up.n_put = (uint32_t)put.size();
    up.n_pairs = (uint32_t)pairs.size();
    up.pack = img.pack;
    up.num_per = img.num_per;
    up.dim0 = img.dim0;
    if (tr.trials)
        launch_db_update_trials(DbUpdateTrialsParams{up, tr.trial_words}, st);
    else
        launch_db_update(up, st);
    if (trk) {  // the table and F follow the scatter, from the sums the read-modify-write launch stored; the flag that stops the scatter stops this too
        FpApplyParams ap{};
        ap.entries = reinterpret_cast<const ulonglong2*>(d + o_app);
        ap.gnew = tk.gnew;
        ap.table = trk->t->table.p;
        ap.weights = tk.weights;
        ap.sums = trk->t->sums();
        ap.err = rp.flag;
        ap.n = (uint32_t)n_app;
        launch_fingerprint_apply(ap, st);
    }
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(W.done, st));
    W.pending = true;
    if (gathers) {
        unsigned long long err = 0;
        HIP_OK(hipMemcpyAsync(&err, d + 8, sizeof(err), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (err != ~0ull) return record_image_error(err, [&](uint64_t k) { return record_of(pieces[k].pos); }, tr);
    }
    if (trk) trk->t->n_updates += n_touched;
    return 0;
}

// The shared body of read_records / read_records_at over the call's n records: piece_at(k, &piece) says whether this image holds record k of the call and
// as what; piece k's bytes go to records + pos * record_bytes + chunk.first, bytes of other records are not touched.  The pieces are built pass by pass
// -- a pass is what option db_stage_bytes stages, at most 2^18 records: one launch and one device-to-host copy -- so the host holds one pass's tables,
// however long the call.  Positions ascend from pass to pass, so the first pass that reports a coefficient ends the call with the call's lowest
// position.  Returns after `st` is synchronised.
template <class PieceAt, class RecordOf>
inline int read_record_pieces(ExportWork& W, const DeviceTables& tb, hipStream_t st, uint8_t* records, uint64_t record_bytes, const RecordChunk& chunk, uint32_t w,
                              uint64_t p_db, uint64_t n, PieceAt piece_at, const ExportImage& src, RecordOf record_of, const RecordTrials& tr = RecordTrials{}) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_OK(hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail("read_records cannot be called while the server's stream is being captured");
    if (n == 0) return 0;
    if (n > 0xFFFFFFFFull) return fail("at most 2^32 - 1 records per read");
    const uint32_t stride = (uint32_t)chunk.len;
    const size_t pass_n = (size_t)std::max<uint64_t>(1, std::min<uint64_t>({options().db_stage_bytes / stride, (uint64_t)(1u << 18), n}));  // (tests force several passes)
    std::vector<RecordPiece> pieces;
    std::vector<uint4> entries, segs;
    pieces.reserve(pass_n);
    for (uint64_t k = 0; k < n;) {
        pieces.clear();
        RecordPiece pc;
        for (; k < n && pieces.size() < pass_n; k++)
            if (piece_at(k, &pc)) pieces.push_back(pc);
        const size_t cnt = pieces.size();
        if (cnt == 0) continue;
        entries.clear();
        segs.clear();
        if (tr.trials)
            pack_record_tables(pieces, 0, cnt, w, tr, false, entries, segs, [&](uint32_t i) { return (uint64_t)i * stride; });
        else
            record_tables(pieces, 0, cnt, stride, w, false, entries, segs, nullptr);
        auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
        const size_t o_ent = 16, o_segs = o_ent + entries.size() * sizeof(uint4), o_stage = up16(o_segs + segs.size() * sizeof(uint4));
        const size_t dev_bytes = o_stage + cnt * stride;
        if (W.dev.words * 8 < dev_bytes) {
            W.dev.release();
            W.dev.words = 0;
            if (W.dev.alloc((dev_bytes + 7) / 8)) {
                (void)hipGetLastError();
                W.dev.p = nullptr;
                W.dev.words = 0;
                return fail("no device memory for the read's staging (%zu bytes)", dev_bytes);
            }
        }
        if (W.host_bytes < cnt * stride) {
            if (W.host) (void)hipHostFree(W.host);
            W.host = nullptr;
            W.host_bytes = 0;
            if (hipHostMalloc((void**)&W.host, cnt * stride, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                return fail("no pinned host memory for the read's bounce buffer (%zu bytes)", cnt * stride);
            }
            W.host_bytes = cnt * stride;
        }
        uint8_t* d = reinterpret_cast<uint8_t*>(W.dev.p);
        HIP_OK(hipMemsetAsync(d, 0xFF, 16, st));  // the error word: ~0 = every coefficient read so far is record data
        HIP_OK(hipMemcpyAsync(d + o_ent, entries.data(), entries.size() * sizeof(uint4), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(d + o_segs, segs.data(), segs.size() * sizeof(uint4), hipMemcpyHostToDevice, st));
        RecordWorkParams rp{};
        rp.db = src.db;
        rp.entries = reinterpret_cast<const uint4*>(d + o_ent);
        rp.segs = reinterpret_cast<const uint4*>(d + o_segs);
        rp.buf = d + o_stage;
        rp.err = reinterpret_cast<unsigned long long*>(d);
        rp.n_entries = (uint32_t)entries.size();
        rp.form = src.form;
        rp.num_per = src.num_per;
        rp.dim0 = src.dim0;
        rp.w = w;
        rp.stride = stride;
        rp.p_db = p_db;
        if (tr.trials)
            launch_pack_record_read(tb, PackRecordWorkParams{rp, tr.trial_words, tr.trials, tr.t0}, st);
        else
            launch_record_read(tb, rp, st);
        HIP_OK(hipGetLastError());
        unsigned long long err = ~0ull;
        HIP_OK(hipMemcpyAsync(W.host, rp.buf, cnt * stride, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(&err, d, sizeof(err), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (err != ~0ull) return record_image_error(err, [&](uint64_t i) { return record_of(pieces[i].pos); }, tr);
        for (size_t i = 0; i < cnt; i++) {
            uint64_t lo = 0, hi = stride;  // the piece's bytes this image holds: all of them, or those in the polynomials of a trial shard's trials
            if (tr.trials) {
                const uint64_t off = pieces[i].off, h0 = (uint64_t)tr.t0 * 256u * w, h1 = (uint64_t)(tr.t0 + tr.nt) * 256u * w;
                lo = std::min(std::max(off, h0), off + stride) - off;
                hi = std::max(std::min(off + stride, h1), off + lo) - off;
            }
            memcpy(records + pieces[i].pos * record_bytes + chunk.first + lo, W.host + i * stride + lo, (size_t)(hi - lo));
        }
    }
    return 0;
}

}  // namespace host
}  // namespace spiral
