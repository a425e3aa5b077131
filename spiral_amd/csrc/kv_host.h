// Keyed records on the host side: the definition of include/spiral_gpu.h "Keyed records" as code -- layout, SipHash-2-4, candidate buckets, the
// placement rule -- and the probe's tables (kv.hip does the device work).  What is written or read afterwards goes through records_host.h's
// update_record_pieces and read_record_pieces unchanged.  Internal to libspiral_gpu.so.
#pragma once
#include <array>

#include "records_host.h"

namespace spiral {
namespace host {

// the buckets of a parameter set, nb = 2^(nu1 + nu2) (r: the record layout they come from); the hash needs no more than this.  out_n = 0: a base
// parameter set; out_n >= 1: SpiralPack, a bucket is an item of out_n^2 polynomials, one per trial image
inline int kv_buckets(const spiral_gpu_params* p, uint32_t out_n, uint64_t* nb, spiral_gpu_record_layout* r = nullptr) {
    if (!p) return fail("null argument");
    spiral_gpu_record_layout l;
    if (record_layout(p, 1, &l, out_n)) return -1;
    *nb = l.capacity / l.per_item;
    if (*nb < 2) return fail("a keyed table needs at least 2 buckets (nu1 + nu2 >= 1)");
    if (r) *r = l;
    return 0;
}

inline int kv_layout(const spiral_gpu_params* p, uint64_t value_bytes, spiral_gpu_kv_layout* out, uint32_t out_n = 0) {
    if (!p || !out) return fail("null argument");
    spiral_gpu_record_layout r;
    uint64_t nb;
    if (kv_buckets(p, out_n, &nb, &r)) return -1;
    if (value_bytes < 1) return fail("a value has at least one byte");
    if (value_bytes > r.item_bytes) return fail("a value of %llu bytes and its tag do not fit a %llu-byte bucket (slots = 0)", (unsigned long long)value_bytes, (unsigned long long)r.item_bytes);
    const uint64_t slots = r.item_bytes / (8 + value_bytes);
    if (slots == 0) return fail("a value of %llu bytes and its tag do not fit a %llu-byte bucket (slots = 0)", (unsigned long long)value_bytes, (unsigned long long)r.item_bytes);
    if (slots > 256) return fail("a value of %llu bytes gives %llu slots per bucket: at most 256", (unsigned long long)value_bytes, (unsigned long long)slots);
    if (8 * slots > 256ull * r.coeff_bits)
        return fail("the %llu tags of a bucket take %llu bytes: the header does not lie inside polynomial 0 (%u bytes)", (unsigned long long)slots,
                    (unsigned long long)(8 * slots), 256u * r.coeff_bits);
    spiral_gpu_kv_layout l{};
    l.coeff_bits = r.coeff_bits;
    l.slots = (uint32_t)slots;
    l.value_bytes = value_bytes;
    l.item_bytes = r.item_bytes;
    l.buckets = nb;
    l.capacity = nb * slots;
    *out = l;
    return 0;
}

// SipHash-2-4, 64-bit output (the public algorithm)
inline uint64_t siphash24(uint64_t k0, uint64_t k1, const uint8_t* m, uint64_t len) {
    uint64_t v0 = k0 ^ 0x736f6d6570736575ull, v1 = k1 ^ 0x646f72616e646f6dull, v2 = k0 ^ 0x6c7967656e657261ull, v3 = k1 ^ 0x7465646279746573ull;
    auto rotl = [](uint64_t x, int b) { return (x << b) | (x >> (64 - b)); };
    auto round = [&] {
        v0 += v1, v1 = rotl(v1, 13), v1 ^= v0, v0 = rotl(v0, 32);
        v2 += v3, v3 = rotl(v3, 16), v3 ^= v2;
        v0 += v3, v3 = rotl(v3, 21), v3 ^= v0;
        v2 += v1, v1 = rotl(v1, 17), v1 ^= v2, v2 = rotl(v2, 32);
    };
    uint64_t i = 0;
    for (; i + 8 <= len; i += 8) {
        uint64_t w = 0;
        for (int b = 0; b < 8; b++) w |= (uint64_t)m[i + b] << (8 * b);
        v3 ^= w;
        round(), round();
        v0 ^= w;
    }
    uint64_t last = len << 56;
    for (int b = 0; i + b < len; b++) last |= (uint64_t)m[i + b] << (8 * b);
    v3 ^= last;
    round(), round();
    v0 ^= last;
    v2 ^= 0xff;
    round(), round(), round(), round();
    return v0 ^ v1 ^ v2 ^ v3;
}

struct KvKey {
    uint64_t tag, b[2];
};
inline KvKey kv_hash(uint64_t nb, const uint8_t* table_key16, const uint8_t* key, uint64_t key_bytes) {
    uint64_t k0 = 0, k1 = 0;
    for (int b = 0; b < 8; b++) k0 |= (uint64_t)table_key16[b] << (8 * b), k1 |= (uint64_t)table_key16[8 + b] << (8 * b);
    KvKey h;
    h.tag = siphash24(k0, k1, key, key_bytes);
    if (h.tag == 0) h.tag = 1;
    const uint64_t u = siphash24(k0, k1 ^ 0xA5ull, key, key_bytes);
    h.b[0] = (u & 0xffffffffull) % nb;
    h.b[1] = (u >> 32) % nb;
    if (h.b[1] == h.b[0]) h.b[1] = h.b[0] ^ 1ull;
    return h;
}
// the n keys of a call, [n][key_bytes]; two equal tags are refused by position
inline int kv_hash_keys(const char* what, uint64_t nb, const void* table_key16, const void* keys, uint64_t key_bytes, uint64_t n, bool distinct,
                        std::vector<KvKey>& out, bool bounded = true) {
    if (!table_key16 || (n && key_bytes && !keys)) return fail("%s: null argument", what);
    if (bounded && n > (1ull << 24)) return fail("%s: at most 2^24 keys per call", what);  // (kv_reconcile takes a whole table's key set: unbounded)
    out.resize((size_t)n);
    static const uint8_t none = 0;
    for (uint64_t k = 0; k < n; k++)
        out[k] = kv_hash(nb, static_cast<const uint8_t*>(table_key16), key_bytes ? static_cast<const uint8_t*>(keys) + k * key_bytes : &none, key_bytes);
    if (distinct && n > 1) {
        std::vector<std::pair<uint64_t, uint64_t>> byt((size_t)n);
        for (uint64_t k = 0; k < n; k++) byt[k] = {out[k].tag, k};
        std::sort(byt.begin(), byt.end());
        uint64_t best = ~0ull, other = 0;  // the lowest position that repeats an earlier tag
        for (uint64_t i = 1; i < n; i++)
            if (byt[i].first == byt[i - 1].first && byt[i].second < best) best = byt[i].second, other = byt[i - 1].second;
        if (best != ~0ull)
            return fail("%s: keys %llu and %llu have equal tags (the same key given twice, or a 64-bit collision: one key to this store)", what,
                        (unsigned long long)other, (unsigned long long)best);
    }
    return 0;
}

// The occupancy of the buckets a call touches, and the rule that places a key ("Placement"): bitmaps[i] belongs to bucket ids[i], ids ascending.
struct KvTable {
    uint32_t slots = 0;
    std::vector<uint64_t> ids;
    std::vector<std::array<uint64_t, 4>> occ;
    size_t at(uint64_t bucket) const { return (size_t)(std::lower_bound(ids.begin(), ids.end(), bucket) - ids.begin()); }
    static uint32_t used(const std::array<uint64_t, 4>& o) { return (uint32_t)(__builtin_popcountll(o[0]) + __builtin_popcountll(o[1]) + __builtin_popcountll(o[2]) + __builtin_popcountll(o[3])); }
    // a new key's (candidate, slot), or false when both buckets are full; marks the slot used
    bool place(const KvKey& h, uint32_t* cand, uint32_t* slot) {
        const size_t i1 = at(h.b[0]), i2 = at(h.b[1]);
        const uint32_t u1 = used(occ[i1]), u2 = used(occ[i2]);
        if (u1 >= slots && u2 >= slots) return false;
        *cand = u2 < u1 ? 1u : 0u;
        std::array<uint64_t, 4>& o = occ[*cand ? i2 : i1];
        for (uint32_t s = 0; s < slots; s++)
            if (!((o[s >> 6] >> (s & 63u)) & 1ull)) {
                o[s >> 6] |= 1ull << (s & 63u);
                *slot = s;
                return true;
            }
        return false;
    }
};

// where a key of a call ends up or was found: candidate 1 or 2 (0: nowhere) and the slot
struct KvSlot {
    uint32_t cand = 0, slot = 0;
};

constexpr uint32_t kKvNoSlot = 0xFFFFFFFFu;

// The probe: ONE launch over the distinct candidate buckets of `keys` (ascending; one workgroup each) on `st`, then one wait.  src: the image that holds
// polynomial 0 of every bucket (a SpiralPack server: trial image 0).  table receives the buckets'
// occupancy, found[k] the (candidate, slot) that holds key k's tag -- candidate 1 first -- or cand = 0.  32 bytes per bucket and 4 per (key, candidate) come back.
inline int kv_probe(const char* what, ExportWork& W, const DeviceTables& tb, hipStream_t st, const ExportImage& src, const spiral_gpu_kv_layout& l, uint64_t p_db,
                    const std::vector<KvKey>& keys, KvTable& table, std::vector<KvSlot>& found) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_OK(hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail("%s cannot be called while the server's stream is being captured", what);
    const size_t n = keys.size();
    found.assign(n, KvSlot{});
    table.slots = l.slots;
    table.ids.clear();
    table.occ.clear();
    if (n == 0) return 0;
    struct Want {
        uint64_t bucket, tag;
        uint32_t out;
    };
    std::vector<Want> want(2 * n);
    for (size_t k = 0; k < n; k++)
        for (uint32_t c = 0; c < 2; c++) want[2 * k + c] = Want{keys[k].b[c], keys[k].tag, (uint32_t)(2 * k + c)};
    std::stable_sort(want.begin(), want.end(), [](const Want& a, const Want& b) { return a.bucket < b.bucket; });
    std::vector<uint4> entries;
    std::vector<ulonglong2> lookups(2 * n);
    for (size_t a = 0; a < want.size();) {
        size_t b = a;
        for (; b < want.size() && want[b].bucket == want[a].bucket; b++) lookups[b] = make_ulonglong2(want[b].tag, want[b].out);
        table.ids.push_back(want[a].bucket);
        entries.push_back(make_uint4((uint32_t)(want[a].bucket / src.num_per), (uint32_t)(want[a].bucket % src.num_per), (uint32_t)a, (uint32_t)(b - a)));
        a = b;
    }
    const size_t nbk = entries.size();
    // one buffer: [error word][entries][lookups] ++ (device writes) [occupancy 4 x u64 per bucket][slot per (key, candidate)]
    const size_t o_ent = 16, o_look = o_ent + nbk * sizeof(uint4), o_occ = o_look + lookups.size() * sizeof(ulonglong2), o_slot = o_occ + nbk * 32;
    const size_t dev_bytes = o_slot + 2 * n * sizeof(uint32_t), back = dev_bytes - o_occ;
    if (W.dev.words * 8 < dev_bytes) {
        W.dev.release();
        W.dev.words = 0;
        if (W.dev.alloc((dev_bytes + 7) / 8)) {
            (void)hipGetLastError();
            W.dev.p = nullptr;
            W.dev.words = 0;
            return fail("no device memory for the probe's tables (%zu bytes)", dev_bytes);
        }
    }
    uint8_t* d = reinterpret_cast<uint8_t*>(W.dev.p);
    HIP_OK(hipMemsetAsync(d, 0xFF, 16, st));  // the error word: ~0 = every coefficient read so far is a plaintext value
    HIP_OK(hipMemcpyAsync(d + o_ent, entries.data(), nbk * sizeof(uint4), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d + o_look, lookups.data(), lookups.size() * sizeof(ulonglong2), hipMemcpyHostToDevice, st));
    KvProbeParams kp{};
    kp.db = src.db;
    kp.entries = reinterpret_cast<const uint4*>(d + o_ent);
    kp.lookups = reinterpret_cast<const ulonglong2*>(d + o_look);
    kp.occ = reinterpret_cast<uint64_t*>(d + o_occ);
    kp.slot_out = reinterpret_cast<uint32_t*>(d + o_slot);
    kp.err = reinterpret_cast<unsigned long long*>(d);
    kp.n_entries = (uint32_t)nbk;
    kp.form = src.form;
    kp.num_per = src.num_per;
    kp.dim0 = src.dim0;
    kp.w = l.coeff_bits;
    kp.slots = l.slots;
    kp.p_db = p_db;
    launch_kv_probe(tb, kp, src.pack != 0, st);
    HIP_OK(hipGetLastError());
    std::vector<uint8_t> host(back);
    unsigned long long err = ~0ull;
    HIP_OK(hipMemcpyAsync(host.data(), d + o_occ, back, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(&err, d, sizeof(err), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (err != ~0ull)
        return fail("%s: the image holds no keyed table at bucket %llu (polynomial 0, coefficient %u is no plaintext value below 2^coeff_bits): not a record "
                    "database (fill_db_random, a load_db of arbitrary words, or items loaded with larger coefficients)",
                    what, (unsigned long long)table.ids[(size_t)(err / kN)], (uint32_t)(err % kN));
    table.occ.resize(nbk);
    memcpy(table.occ.data(), host.data(), nbk * 32);
    const uint32_t* slot = reinterpret_cast<const uint32_t*>(host.data() + nbk * 32);
    for (size_t k = 0; k < n; k++)
        for (uint32_t c = 0; c < 2 && !found[k].cand; c++)
            if (slot[2 * k + c] != kKvNoSlot) found[k] = KvSlot{c + 1, slot[2 * k + c]};
    return 0;
}

// tag and value of a key in slot `slot` of image item (j, ii) as two pieces staged at 2 k and 2 k + 1, `stride` = max(8, V) bytes apart
inline void kv_pieces(const spiral_gpu_kv_layout& l, uint64_t k, uint32_t j, uint32_t ii, uint32_t slot, std::vector<RecordPiece>& pieces) {
    pieces.push_back(RecordPiece{2 * k, j, ii, 8u * slot, 8u});
    pieces.push_back(RecordPiece{2 * k + 1, j, ii, (uint32_t)(8u * l.slots + slot * l.value_bytes), (uint32_t)l.value_bytes});
}

// The image a keyed call works on, as either server states it: a base server's image, or the trial images of a SpiralPack server (tr.trials != 0; src
// and dst name trial 0, where polynomial 0 of every bucket lies)
struct KvImage {
    ExportWork& xwork;
    UpdateWork& upd;
    const DeviceTables& tb;
    hipStream_t st;
    ExportImage src;
    UpdateImage dst;
    RecordTrials tr;
    const FpTrackCtx* trk;  // null: the image's fingerprint is not tracked
    uint32_t num_per;
    uint64_t p_db;
};

// put, and delete (tag and value bytes of the found slots become zero), after the server's own checks: the probe, the placement rule over the host's copy
// of the occupancy, then tag and value of every written key as two pieces through update_record_pieces.  ONE copy of the rule and of its failure message
// for both servers.
inline int kv_write(const KvImage& I, const char* what, bool put, const spiral_gpu_kv_layout& l, const void* table_key16, const void* keys, uint64_t key_bytes,
                    const void* values, uint64_t n, uint64_t* n_deleted) {
    const uint64_t value_bytes = l.value_bytes;
    std::vector<KvKey> hk;
    if (kv_hash_keys(what, l.buckets, table_key16, keys, key_bytes, n, true, hk)) return -1;
    if (n_deleted) *n_deleted = 0;
    if (n == 0) return 0;
    KvTable table;
    std::vector<KvSlot> at;
    if (kv_probe(what, I.xwork, I.tb, I.st, I.src, l, I.p_db, hk, table, at)) return -1;
    if (put)
        for (uint64_t k = 0; k < n; k++) {
            if (at[k].cand) continue;  // present: that slot is overwritten
            uint32_t cand, slot;
            if (!table.place(hk[k], &cand, &slot))
                return fail("%s: key %llu cannot be placed: its buckets %llu and %llu are both full (%u slots each); nothing was written", what, (unsigned long long)k,
                            (unsigned long long)hk[k].b[0], (unsigned long long)hk[k].b[1], l.slots);
            at[k] = KvSlot{cand + 1, slot};
        }
    const uint64_t stride = std::max<uint64_t>(8, value_bytes);
    std::vector<uint64_t> key_of;  // written key -> its position in the call
    for (uint64_t k = 0; k < n; k++)
        if (at[k].cand) key_of.push_back(k);
    const size_t m = key_of.size();
    if (m == 0) return 0;
    std::vector<RecordPiece> pieces;
    pieces.reserve(2 * m);
    std::vector<uint8_t> stage(2 * m * (size_t)stride, 0);  // [tag, value] per written key, `stride` bytes each; a delete writes zeros
    for (size_t i = 0; i < m; i++) {
        const uint64_t k = key_of[i], bucket = hk[k].b[at[k].cand - 1];
        kv_pieces(l, i, (uint32_t)(bucket / I.num_per), (uint32_t)(bucket % I.num_per), at[k].slot, pieces);
        if (put) {
            for (int b = 0; b < 8; b++) stage[2 * i * (size_t)stride + b] = (uint8_t)(hk[k].tag >> (8 * b));
            memcpy(&stage[(2 * i + 1) * (size_t)stride], static_cast<const uint8_t*>(values) + k * value_bytes, (size_t)value_bytes);
        }
    }
    if (update_record_pieces(I.upd, I.tb, I.st, stage.data(), stride, RecordChunk{0, stride}, l.coeff_bits, I.p_db, pieces, I.dst, I.src,
                             [&](uint64_t pos) { return key_of[(size_t)(pos / 2)]; }, I.tr, I.trk))
        return -1;
    if (n_deleted) *n_deleted = m;
    return 0;
}

// get, after the server's own checks: the probe, then the found slots' values through read_record_pieces; a missing key's bytes are left alone
inline int kv_get(const KvImage& I, const spiral_gpu_kv_layout& l, const void* table_key16, const void* keys, uint64_t key_bytes, void* values, uint64_t n,
                  uint8_t* found) {
    const uint64_t value_bytes = l.value_bytes;
    std::vector<KvKey> hk;
    if (kv_hash_keys("kv_get", l.buckets, table_key16, keys, key_bytes, n, false, hk)) return -1;
    KvTable table;
    std::vector<KvSlot> at;
    if (kv_probe("kv_get", I.xwork, I.tb, I.st, I.src, l, I.p_db, hk, table, at)) return -1;
    for (uint64_t k = 0; k < n; k++) found[k] = (uint8_t)at[k].cand;
    return read_record_pieces(
        I.xwork, I.tb, I.st, static_cast<uint8_t*>(values), value_bytes, RecordChunk{0, value_bytes}, l.coeff_bits, I.p_db, n,
        [&](uint64_t k, RecordPiece* pc) {
            if (!at[k].cand) return false;
            const uint64_t bucket = hk[k].b[at[k].cand - 1];
            *pc = RecordPiece{k, (uint32_t)(bucket / I.num_per), (uint32_t)(bucket % I.num_per), (uint32_t)(8u * l.slots + at[k].slot * value_bytes), (uint32_t)value_bytes};
            return true;
        },
        I.src, [&](uint64_t pos) { return pos; }, I.tr);
}

// Table occupancy (include/spiral_gpu.h spiral_gpu_server_kv_stats): ONE launch over buckets [first, first + n) on `st`, the histogram's 257 words back,
// one wait; used, full_buckets and max_used are derived from the histogram here.  src as for kv_probe.
inline int kv_stats(ExportWork& W, const DeviceTables& tb, hipStream_t st, const ExportImage& src, const spiral_gpu_kv_layout& l, uint64_t p_db, uint64_t first, uint64_t n,
                    spiral_gpu_kv_stats* out) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_OK(hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail("kv_stats cannot be called while the server's stream is being captured");
    if (first > l.buckets || n > l.buckets - first)
        return fail("kv_stats: buckets [%llu, +%llu) outside the table of %llu", (unsigned long long)first, (unsigned long long)n, (unsigned long long)l.buckets);
    if (l.buckets > 0x7FFFFFFFull) return fail("kv_stats: a table of %llu buckets, at most 2^31 - 1", (unsigned long long)l.buckets);
    spiral_gpu_kv_stats s{};
    s.buckets = n;
    s.slots = l.slots;
    if (n == 0) {
        *out = s;
        return 0;
    }
    // one buffer: [error word, padding][histogram, 257 words]
    const size_t o_hist = 16, dev_bytes = o_hist + 257 * 8;
    if (W.dev.words * 8 < dev_bytes) {
        W.dev.release();
        W.dev.words = 0;
        if (W.dev.alloc((dev_bytes + 7) / 8)) {
            (void)hipGetLastError();
            W.dev.p = nullptr;
            W.dev.words = 0;
            return fail("no device memory for the histogram (%zu bytes)", dev_bytes);
        }
    }
    uint8_t* d = reinterpret_cast<uint8_t*>(W.dev.p);
    HIP_OK(hipMemsetAsync(d, 0xFF, 16, st));  // the error word: ~0 = every coefficient read so far is a plaintext value
    HIP_OK(hipMemsetAsync(d + o_hist, 0, 257 * 8, st));
    KvStatsParams sp{};
    sp.db = src.db;
    sp.hist = reinterpret_cast<unsigned long long*>(d + o_hist);
    sp.err = reinterpret_cast<unsigned long long*>(d);
    sp.first_bucket = (uint32_t)first;
    sp.n_buckets = (uint32_t)n;
    sp.form = src.form;
    sp.num_per = src.num_per;
    sp.dim0 = src.dim0;
    sp.w = l.coeff_bits;
    sp.slots = l.slots;
    sp.p_db = p_db;
    launch_kv_stats(tb, sp, src.pack != 0, st);
    HIP_OK(hipGetLastError());
    unsigned long long err = ~0ull;
    HIP_OK(hipMemcpyAsync(s.hist, d + o_hist, 257 * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(&err, d, sizeof(err), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (err != ~0ull)
        return fail("kv_stats: the image holds no keyed table at bucket %llu (polynomial 0, coefficient %u is no plaintext value below 2^coeff_bits): not a record "
                    "database (fill_db_random, a load_db of arbitrary words, or items loaded with larger coefficients)",
                    (unsigned long long)(err / kN), (uint32_t)(err % kN));
    for (uint32_t u = 0; u <= l.slots; u++) {
        if (!s.hist[u]) continue;
        s.used += (uint64_t)u * s.hist[u];
        s.max_used = u;
    }
    s.full_buckets = s.hist[l.slots];
    *out = s;
    return 0;
}

// ---- Listing (include/spiral_gpu.h "Listing"): an entry is a slot whose tag is not 0; a listing of a set of buckets is all their entries in the order
// of the buckets, and within a bucket by ascending slot; with values, row k is bytes [8 slots + slot V, + V) of entry k's bucket stream --------------
static_assert(sizeof(spiral_gpu_kv_entry) == 16 && sizeof(ulonglong2) == 16, "an entry is one 16-byte store: {tag, bucket | slot << 32}");

// buckets per pass: option kv_scan_chunk, or the most that keeps a pass's staged tags within 2^22 (32 MiB) and the pass within 2^16 buckets
inline uint32_t kv_scan_pass(uint32_t slots) {
    const uint32_t set = options().kv_scan_chunk;
    return set ? set : std::max<uint32_t>(1u, std::min<uint32_t>(1u << 16, (1u << 22) / slots));
}

// kv_scan (ids == null: buckets [first, first + n)) and kv_scan_at (the n buckets of ids, in that order) after the server's own checks, ONE body for both
// servers.  Passes of kv_scan_pass buckets on I.st, three launches each -- decode, offsets, compact (kv.hip; count-only: no staging, no compact) --
// with nothing read back in between: the running total lives on the device.  Then one copy of the error word, the total and the entries, one wait.
// Values, where wanted and the count fits: one RecordPiece per entry, the one kv_get builds, through read_record_pieces.
inline int kv_scan(const KvImage& I, const char* what, const spiral_gpu_kv_layout& l, uint64_t first, const uint64_t* ids, uint64_t n, spiral_gpu_kv_entry* entries,
                   void* values, uint64_t max_entries, uint64_t* n_entries) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_OK(hipStreamIsCapturing(I.st, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail("%s cannot be called while the server's stream is being captured", what);
    if (l.buckets > 0x7FFFFFFFull) return fail("%s: a table of %llu buckets, at most 2^31 - 1", what, (unsigned long long)l.buckets);
    if (max_entries > 0 && !entries) return fail("%s: entries is NULL with max_entries = %llu (count-only: max_entries = 0, entries = values = NULL)", what, (unsigned long long)max_entries);
    std::vector<uint32_t> id32;
    if (ids) {
        if (n > 0x7FFFFFFFull) return fail("%s: at most 2^31 - 1 buckets per call", what);
        id32.resize((size_t)n);
        for (uint64_t k = 0; k < n; k++) {
            if (ids[k] >= l.buckets) return fail("%s: bucket %llu at position %llu outside the table of %llu", what, (unsigned long long)ids[k], (unsigned long long)k, (unsigned long long)l.buckets);
            id32[(size_t)k] = (uint32_t)ids[k];
        }
    } else if (first > l.buckets || n > l.buckets - first)
        return fail("%s: buckets [%llu, +%llu) outside the table of %llu", what, (unsigned long long)first, (unsigned long long)n, (unsigned long long)l.buckets);
    *n_entries = 0;
    if (n == 0) return 0;
    const bool count_only = max_entries == 0 && !entries && !values;
    const uint64_t cap_entries = count_only ? 0 : std::min<uint64_t>(max_entries, n * l.slots);  // what can come back
    const uint32_t pass = (uint32_t)std::min<uint64_t>(kv_scan_pass(l.slots), n);
    // one buffer: [error word][running total][ids of the call][counts of a pass][offsets of a pass][staged tags of a pass][entries of the call]
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t o_ids = 16, o_counts = up16(o_ids + id32.size() * 4), o_offsets = up16(o_counts + (size_t)pass * 4), o_stage = up16(o_offsets + (size_t)pass * 8);
    const size_t o_entries = up16(o_stage + (count_only ? 0 : (size_t)pass * l.slots * 8)), dev_bytes = o_entries + (size_t)cap_entries * 16;
    ExportWork& W = I.xwork;
    if (W.dev.words * 8 < dev_bytes) {
        W.dev.release();
        W.dev.words = 0;
        if (W.dev.alloc((dev_bytes + 7) / 8)) {
            (void)hipGetLastError();
            W.dev.p = nullptr;
            W.dev.words = 0;
            return fail("no device memory for the listing's staging (%zu bytes)", dev_bytes);
        }
    }
    if (W.host_bytes < cap_entries * 16) {
        if (W.host) (void)hipHostFree(W.host);
        W.host = nullptr;
        W.host_bytes = 0;
        if (hipHostMalloc((void**)&W.host, (size_t)cap_entries * 16, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return fail("no pinned host memory for the listing's bounce buffer (%zu bytes)", (size_t)cap_entries * 16);
        }
        W.host_bytes = (size_t)cap_entries * 16;
    }
    uint8_t* d = reinterpret_cast<uint8_t*>(W.dev.p);
    HIP_OK(hipMemsetAsync(d, 0xFF, 8, I.st));  // the error word: ~0 = every coefficient read so far is a plaintext value
    HIP_OK(hipMemsetAsync(d + 8, 0, 8, I.st));  // the running total
    if (ids) HIP_OK(hipMemcpyAsync(d + o_ids, id32.data(), id32.size() * 4, hipMemcpyHostToDevice, I.st));
    KvScanParams sp{};
    sp.db = I.src.db;
    sp.ids = ids ? reinterpret_cast<const uint32_t*>(d + o_ids) : nullptr;
    sp.stage = count_only ? nullptr : reinterpret_cast<uint64_t*>(d + o_stage);
    sp.counts = reinterpret_cast<uint32_t*>(d + o_counts);
    sp.offsets = reinterpret_cast<unsigned long long*>(d + o_offsets);
    sp.total = reinterpret_cast<unsigned long long*>(d + 8);
    sp.err = reinterpret_cast<unsigned long long*>(d);
    sp.entries = reinterpret_cast<ulonglong2*>(d + o_entries);
    sp.max_entries = cap_entries;
    sp.form = I.src.form;
    sp.num_per = I.src.num_per;
    sp.dim0 = I.src.dim0;
    sp.w = l.coeff_bits;
    sp.slots = l.slots;
    sp.p_db = I.p_db;
    for (uint64_t done = 0; done < n; done += pass) {
        sp.first = (uint32_t)((ids ? 0 : first) + done);
        sp.n_buckets = (uint32_t)std::min<uint64_t>(pass, n - done);
        launch_kv_scan_decode(I.tb, sp, I.src.pack != 0, I.st);
        launch_kv_scan_offsets(sp, I.st);
        if (!count_only) launch_kv_scan_compact(sp, I.st);
        HIP_OK(hipGetLastError());
    }
    unsigned long long back[2] = {~0ull, 0};  // the error word and the total
    HIP_OK(hipMemcpyAsync(back, d, sizeof(back), hipMemcpyDeviceToHost, I.st));
    // (the entries' count is the total, which is not known here: what can come back is copied to the bounce buffer, and min(total, max_entries) of it
    // goes on to the caller.  A caller that sized its buffer by a count-only call copies exactly the live entries.)
    if (cap_entries) HIP_OK(hipMemcpyAsync(W.host, d + o_entries, (size_t)cap_entries * 16, hipMemcpyDeviceToHost, I.st));
    HIP_OK(hipStreamSynchronize(I.st));
    if (back[0] != ~0ull) {
        const uint64_t at = back[0] / kN;
        if (ids)
            return fail("%s: the image holds no keyed table at position %llu of the list, bucket %llu (polynomial 0, coefficient %u is no plaintext value below "
                        "2^coeff_bits): not a record database (fill_db_random, a load_db of arbitrary words, or items loaded with larger coefficients)",
                        what, (unsigned long long)at, (unsigned long long)ids[at], (uint32_t)(back[0] % kN));
        return fail("%s: the image holds no keyed table at bucket %llu (polynomial 0, coefficient %u is no plaintext value below 2^coeff_bits): not a record "
                    "database (fill_db_random, a load_db of arbitrary words, or items loaded with larger coefficients)",
                    what, (unsigned long long)at, (uint32_t)(back[0] % kN));
    }
    const uint64_t total = back[1];
    *n_entries = total;
    if (count_only) return 0;
    if (total > max_entries)
        return fail("%s: the buckets named hold %llu entries, max_entries is %llu; nothing was written", what, (unsigned long long)total, (unsigned long long)max_entries);
    memcpy(entries, W.host, (size_t)total * 16);
    if (!values || total == 0) return 0;
    const uint64_t V = l.value_bytes;
    return read_record_pieces(
        I.xwork, I.tb, I.st, static_cast<uint8_t*>(values), V, RecordChunk{0, V}, l.coeff_bits, I.p_db, total,
        [&](uint64_t k, RecordPiece* pc) {
            const spiral_gpu_kv_entry& e = entries[k];
            *pc = RecordPiece{k, e.bucket / I.num_per, e.bucket % I.num_per, (uint32_t)(8u * l.slots + e.slot * V), (uint32_t)V};
            return true;
        },
        I.src, [&](uint64_t pos) { return pos; }, I.tr);
}

// spiral_gpu_kv_reconcile (include/spiral_gpu.h "Listing"): a whole table's listing against a key set, on the host.  nb: the table's buckets.
inline int kv_reconcile(uint64_t nb, const void* table_key16, const void* keys, uint64_t key_bytes, uint64_t n_keys, const spiral_gpu_kv_entry* entries, uint64_t n_entries,
                        int64_t* where, uint8_t* entry_class, spiral_gpu_kv_reconcile_counts* counts) {
    const char* what = "kv_reconcile";
    if (n_entries && !entries) return fail("%s: null argument", what);
    for (uint64_t e = 0; e < n_entries; e++) {
        if (entries[e].bucket >= nb) return fail("%s: entry %llu names bucket %u outside the table of %llu", what, (unsigned long long)e, entries[e].bucket, (unsigned long long)nb);
        if (entries[e].tag == 0) return fail("%s: entry %llu has tag 0 (an empty slot is no entry)", what, (unsigned long long)e);
        if (e && (entries[e].bucket < entries[e - 1].bucket || (entries[e].bucket == entries[e - 1].bucket && entries[e].slot <= entries[e - 1].slot)))
            return fail("%s: entry %llu (bucket %u, slot %u) does not follow entry %llu (bucket %u, slot %u): a listing ascends strictly in (bucket, slot)", what,
                        (unsigned long long)e, entries[e].bucket, entries[e].slot, (unsigned long long)(e - 1), entries[e - 1].bucket, entries[e - 1].slot);
    }
    std::vector<KvKey> hk;
    if (kv_hash_keys(what, nb, table_key16, keys, key_bytes, n_keys, true, hk, false)) return -1;
    // the entries of bucket b: [lower bound of b, lower bound of b + 1)
    auto bucket_begin = [&](uint64_t b) {
        return (uint64_t)(std::lower_bound(entries, entries + n_entries, b, [](const spiral_gpu_kv_entry& e, uint64_t bucket) { return e.bucket < bucket; }) - entries);
    };
    // what a lookup of key k finds: b1 first, the lowest slot
    auto find = [&](const KvKey& h) -> int64_t {
        for (uint32_t c = 0; c < 2; c++)
            for (uint64_t e = bucket_begin(h.b[c]); e < n_entries && entries[e].bucket == h.b[c]; e++)
                if (entries[e].tag == h.tag) return (int64_t)e;
        return -1;
    };
    spiral_gpu_kv_reconcile_counts ct{};
    std::vector<std::pair<uint64_t, uint64_t>> byt((size_t)n_keys);  // (tag, key), tags distinct
    std::vector<int64_t> at((size_t)n_keys);
    for (uint64_t k = 0; k < n_keys; k++) {
        byt[(size_t)k] = {hk[(size_t)k].tag, k};
        at[(size_t)k] = find(hk[(size_t)k]);
        if (at[(size_t)k] < 0) ct.missing++;
        if (where) where[k] = at[(size_t)k];
    }
    std::sort(byt.begin(), byt.end());
    for (uint64_t e = 0; e < n_entries; e++) {
        uint8_t cls = 3;
        const auto it = std::lower_bound(byt.begin(), byt.end(), std::make_pair(entries[e].tag, (uint64_t)0));
        if (it != byt.end() && it->first == entries[e].tag) {
            const KvKey& h = hk[(size_t)it->second];
            cls = at[(size_t)it->second] == (int64_t)e ? 0 : (entries[e].bucket == h.b[0] || entries[e].bucket == h.b[1]) ? 1 : 2;
        }
        (cls == 0 ? ct.held : cls == 1 ? ct.shadowed : cls == 2 ? ct.misplaced : ct.orphans)++;
        if (entry_class) entry_class[e] = cls;
    }
    if (counts) *counts = ct;
    return 0;
}

}  // namespace host
}  // namespace spiral
