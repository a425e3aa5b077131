// Host-side helpers shared by the host units of both servers (error reporting, device buffers, the
// coefficient-expansion driver).  Internal to libspiral_gpu.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/spiral_gpu.h"
#include "common.h"
#include "fingerprint_math.h"
#include "kernels.h"
#include "seed_device.h"
#include "transform_jobs.h"

namespace spiral {
namespace host {

extern thread_local std::string g_err;
extern std::atomic<uint64_t> g_pack_lane_batches;  // primitives.cpp: what get_option("pack_lane_batches") reads
extern std::atomic<uint64_t> g_db_export_ns;       // primitives.cpp: what get_option("db_export_ns") reads
extern std::atomic<uint64_t> g_db_fingerprint_ns;  // primitives.cpp: what get_option("db_fingerprint_ns") reads

inline int fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return -1;
}

#define HIP_OK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

constexpr size_t kPolyBytes = (size_t)kN * sizeof(uint64_t);  // PK or RAW polynomial
constexpr size_t kRefNtt = 2 * (size_t)kN;                     // words of a reference NTT-form polynomial
constexpr uint64_t kQprimeMods[37] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 12289, 12289, 61441, 65537, 65537, 520193, 786433, 786433,
                                      3604481, 7340033, 16515073, 33292289, 67043329, 132120577, 268369921, 469762049, 1073479681,
                                      2013265921, 4293918721ull, 8588886017ull, 17175674881ull, 34359214081ull, 68718428161ull};  // values.h:74-76

inline uint32_t ceil_log2(uint64_t x) {
    uint32_t r = 0;
    while ((1ull << r) < x) r++;
    return r;
}

inline int shape_of(const spiral_gpu_params* p, spiral_gpu_shape* s) {
    if (!p || !s) return fail("null argument");
    if (p->nu1 > 16 || p->nu2 > 16) return fail("nu1/nu2 out of range");
    // 56 digits at most: the expansion's digit transforms are left lazy ([0, 2m), LD_EXPAND) and expand_mac_round_* sums up to
    // t_exp + t_exp_right of them per u64 accumulator -- raising the cap needs lazy_ok to hold for the new sum
    static_assert(spiral::lazy_ok(56) && spiral::lazy_ok(2 * 56), "the digit-count cap below keeps the lazy expansion digits inside the u64 accumulators");
    if (p->t_gsw < 2 || p->t_gsw > 28 || p->t_conv < 1 || p->t_conv > 56 || p->t_exp < 1 || p->t_exp > 56 || p->t_exp_right < 1 ||
        p->t_exp_right > 56)
        return fail("gadget dimension out of range");
    if (p->qprime_bits >= 37 || kQprimeMods[p->qprime_bits] == 0) return fail("unsupported q' bit width %u", p->qprime_bits);
    if (p->p_db < 2 || p->p_db > (1ull << 40)) return fail("unsupported plaintext modulus");
    s->dim0 = 1u << p->nu1;
    s->num_per = 1u << p->nu2;
    s->ell = p->t_gsw;
    s->m2 = 3 * p->t_gsw;
    s->n_bits = s->dim0 + s->ell * p->nu2;
    s->qprime = kQprimeMods[p->qprime_bits];
    if (p->direct_upload) {
        s->g = s->stopround = s->n_left = s->n_right = 0;
        s->n_query_cts = s->n_bits;
    } else {
        s->g = ceil_log2(s->n_bits);
        s->stopround = p->nu2 ? ceil_log2((uint64_t)s->ell * p->nu2) : 0;
        if (s->ell * p->nu2 > s->dim0) s->stopround = 0;  // src/spiral.cpp:2083
        s->n_left = s->g;
        s->n_right = s->stopround ? s->stopround + 1 : s->g;
        s->n_query_cts = 1;
        if (s->g > kLogN) return fail("query does not fit one polynomial (g = %u)", s->g);
    }
    return 0;
}

// wire form of a switched response (include/spiral_gpu.h): row 0 at qprime_bits, the rest at the bits that hold a value < 4 p_db
inline uint32_t wire_bits_rest(const spiral_gpu_params* p) { return ceil_log2(4 * p->p_db); }
inline size_t wire_bytes(const spiral_gpu_params* p, uint32_t out_n) {
    return ((size_t)out_n * kN * p->qprime_bits + (size_t)out_n * out_n * kN * wire_bits_rest(p)) / 8;
}

inline uint32_t inv_mod_2n(uint32_t t) {  // t odd, inverse modulo 2N = 4096
    uint32_t x = 1;
    for (int i = 0; i < 12; i++) x = x * (2 - t * x);  // Newton, doubles the valid bits
    return x & (2 * kN - 1);
}

struct DevBuf {
    uint64_t* p = nullptr;
    size_t words = 0;
    bool carved = false;  // a piece of an Arena: not freed on its own
    int alloc(size_t w) {
        words = w ? w : 1;
        carved = false;
        HIP_OK(hipMalloc(&p, words * sizeof(uint64_t)));
        return 0;
    }
    void release() {
        if (p && !carved) (void)hipFree(p);
        p = nullptr;
    }
};
// One allocation holding all per-query buffers of a server in a fixed order, so that two servers with the same parameters have the
// same internal layout and lane q's buffer X is lane 0's X + (arena_q - arena_0): what lets one launch serve several query lanes
// (kernels.h Lanes).  Two passes over the same carve sequence: base == nullptr sizes it, then the real base hands out the pieces.  `pieces` records
// where each piece begins, in carve order: the layout itself, which lanes.h compares before it trusts that constant.
struct Arena {
    uint64_t* base = nullptr;
    size_t used = 0;
    std::vector<size_t> pieces;
    uint64_t* take(size_t w) {
        uint64_t* p = base ? base + used : nullptr;
        pieces.push_back(used);
        used += (w + 31u) & ~(size_t)31u;  // 256-byte pieces
        return p;
    }
    void carve(DevBuf& b, size_t w) {
        b.words = w ? w : 1;
        b.carved = true;
        b.p = take(b.words);
    }
};
// the two passes: `buf` becomes one allocation of the words `layout` takes, and holds the pieces `layout` carves, recorded in `pieces`
template <class Layout>
inline int alloc_carved(DevBuf& buf, std::vector<size_t>& pieces, Layout layout) {
    Arena sizing;
    layout(sizing);
    if (buf.alloc(sizing.used)) return -1;
    Arena real{buf.p};
    layout(real);
    pieces = std::move(real.pieces);
    return 0;
}

// scoped device scratch for the host-buffer seams
struct Scratch {
    std::vector<void*> ptrs;
    ~Scratch() {
        for (void* p : ptrs) (void)hipFree(p);
    }
    uint64_t* get(size_t words) {
        void* p = nullptr;
        if (hipMalloc(&p, (words ? words : 1) * sizeof(uint64_t)) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return (uint64_t*)p;
    }
    uint64_t* upload(const uint64_t* host, size_t words) {
        uint64_t* d = get(words);
        if (d && hipMemcpy(d, host, words * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return d;
    }
};

inline int current_tables(DeviceTables* t) {
    int dev = 0;
    HIP_OK(hipGetDevice(&dev));
    if (tables_get(dev, t) != 0) return fail("twiddle table setup failed on device %d", dev);
    return 0;
}

// ---- expansion on PK buffers, shared by the seam and the resident server ---------------------------------
struct ExpandWork {
    uint64_t* raw;  // per active ct a: [2a] = automorph(c_0) RAW, [2a + 1] = NTT(automorph(c_1)) PK
    uint64_t* g;    // per active ct: t digit polynomials, PK
};
inline size_t expand_g_polys(uint32_t g, uint32_t t_exp, uint32_t t_exp_right) {
    size_t half = (size_t)1 << (g ? g - 1 : 0);  // at most 2^(g-1) active cts per parity
    return half * ((size_t)t_exp + 1 + t_exp_right + 1);
}

// What one rank of a G = 2^g_log rank answer expands (all zero: everything).  The expanded ciphertexts end up at cv[2 j]
// (first-dimension index j) and cv[2 i + 1] (GSW bit i) (reorderFromStopround, src/spiral.cpp:2027-2036), and slot index
// bit r is decided in round r.  A rank needs the first-dimension ciphertexts of its own j in [rank J, (rank + 1) J),
// J = 2^j_log: in round r <= j_log those still descend from every even ciphertext of the round, afterwards only from the
// J whose higher slot bits spell the low bits of `rank`.  Of the GSW bits -- all ranks need all of them, for the folding
// keys -- each rank expands those with i = rank mod G from round g_log on, and the ranks exchange them (one all-gather).
struct ExpandShard {
    uint32_t rank, g_log, j_log;
};

// src/spiral.cpp:1664-1743.  cv: 2^g cts (2 PK polys each).
inline void run_expand(const DeviceTables& tb, uint64_t* cv, uint32_t g, uint32_t t_exp, const uint64_t* w_left, uint32_t t_exp_right,
                const uint64_t* w_right, uint32_t max_bits_right, uint32_t stopround, const ExpandWork& wk, hipStream_t st,
                const uint64_t* query = nullptr,  // query: the packed query ciphertext when cv[0] does not hold it yet
                uint32_t r_begin = 0, uint32_t r_end = 0xffffffffu,  // rounds [r_begin, min(r_end, g))
                const ExpandShard& shard = ExpandShard{},
                uint32_t parity = 3,  // bit 0: the even-index ciphertexts, bit 1: the odd-index ones.  After round 0 the two trees never read each
                                      // other (a ciphertext is created from the one num_in = 2^r slots below it: same parity for r >= 1, and in
                                      // round 0 both come from the query), so with stopround > 0 -- evens = first-dimension ciphertexts, odds = GSW
                                      // bits -- the two halves can run as independent launch sequences on their own work buffers
                const Lanes& lanes = Lanes{}) {  // query lanes: cv, w_left, w_right, wk, query are lane 0's (kernels.h)
    // active odd-index ciphertexts of round r (:1701-1702); the even ones are all 2^r
    auto odd_count = [&](uint32_t r) {
        const uint32_t num_in = 1u << r;
        if (stopround > 0 && r > stopround) return 0u;
        if (stopround > 0 && r == stopround) return std::min(num_in, max_bits_right + 1);
        return num_in;
    };
    for (uint32_t r = r_begin; r < std::min(r_end, g); r++) {
        const uint32_t num_in = 1u << r;
        const uint32_t t = (kN >> r) + 1;
        uint32_t cnt_even = (parity & 1u) ? num_in : 0u, cnt_odd = (parity & 2u) ? odd_count(r) : 0u;
        if (cnt_even + cnt_odd == 0) continue;
        ExpandActive act{};
        if (shard.g_log) {
            if (r > shard.j_log && cnt_even) {  // 2^(r - j_log) blocks of J even ciphertexts: this rank's is the one its low bits name
                cnt_even = 1u << shard.j_log;
                act.e_off = (shard.rank & ((1u << (r - shard.j_log)) - 1u)) << shard.j_log;
            }
            if (r >= shard.g_log) {  // every G-th odd ciphertext, starting at `rank`
                const uint32_t G = 1u << shard.g_log;
                cnt_odd = cnt_odd > shard.rank ? (cnt_odd - shard.rank + G - 1u) / G : 0u;
                act.o_stride_m1 = G - 1u;
                act.o_off = shard.rank;
            }
        }
        // 1) INTT + CRT of row 0 and the automorphed row 1 (a slot permutation) of every active ct, both parities;
        //    cts with i >= num_in are neg1 * cv[i - num_in] (:1709): created inside this kernel in round 0, by the
        //    previous round's MAC afterwards
        const uint32_t cnt = cnt_even + cnt_odd;
        InvParams ip{};
        ip.dst = wk.raw;
        ip.src_map = ip.dst_map = identity_map();
        ip.cv = cv;
        ip.neg1 = tb.neg1 + (size_t)r * kN;
        ip.neg1s = tb.neg1s + (size_t)r * kN;
        ip.num_in = num_in;
        ip.cnt_e = cnt_even;
        ip.act = act;
        ip.auto_t = t;
        ip.create_here = r == 0;
        ip.query = query;
        ip.lanes = lanes;
        launch_ntt_inverse_expand(tb, ip, 2 * cnt, st);
        // 2) G^-1(automorph(c)[0]) digits (t_exp / t_exp_right per ct), one launch
        FwdParams fp{};
        fp.src = wk.raw;
        fp.dst = wk.g;
        fp.src_map = fp.dst_map = identity_map();
        fp.n_digits = 1;
        fp.cnt_e = cnt_even;
        fp.t_e = t_exp;
        fp.t_o = t_exp_right;
        fp.lanes = lanes;
        launch_ntt_forward(tb, fp, LD_EXPAND, ST_PK, cnt_even * t_exp + cnt_odd * t_exp_right, st);
        // 3) cv[i] += W * digits + (0, NTT(c'_1))
        ExpandMacParams mp{};
        mp.cv = cv;
        mp.w_e = w_left + (size_t)r * 2 * t_exp * kN;
        mp.w_o = w_right + (size_t)r * 2 * t_exp_right * kN;  // never dereferenced when cnt_odd == 0
        mp.g = wk.g;
        mp.a1 = wk.raw;
        mp.cnt_e = cnt_even;
        mp.cnt_o = cnt_odd;
        mp.act = act;
        mp.t_e = t_exp;
        mp.t_o = t_exp_right;
        if (r + 1 < g) {
            mp.neg1n = tb.neg1 + (size_t)(r + 1) * kN;
            mp.neg1ns = tb.neg1s + (size_t)(r + 1) * kN;
            mp.next_num_in = 2 * num_in;
            mp.next_cnt_o = odd_count(r + 1);
        }
        mp.lanes = lanes;
        launch_expand_mac_round(mp, st);
    }
}


// Raw database ingest shared by the two servers (the first half of load_db, src/spiral.cpp:1083-1171, on the
// device): items [lo, hi) of a host stream whose first item is `first` are staged a chunk at a time and handed to `launch`
// (items_dev, first_item_of_chunk, n_items_of_chunk), which runs the centred lift + batched transform + layout scatter.
// polys_per_item: n0*n2 = 4 (base) or 1 (SpiralPack).  The error word is set by the kernels when a coefficient is >= p_db.
template <class Launch>
inline int ingest_items(const void* items, uint32_t coeff_bits, uint64_t first, uint64_t lo, uint64_t hi, uint32_t polys_per_item, uint64_t p_db,
                        hipStream_t st, Launch launch) {
    if (!items) return fail("null item stream");
    if (coeff_bits != 64 && (coeff_bits < 1 || coeff_bits > 40)) return fail("coefficient width %u not in 1..40 or 64", coeff_bits);
    if (coeff_bits < 64 && (1ull << coeff_bits) < p_db) return fail("%u-bit coefficients cannot hold values below p_db", coeff_bits);
    if (lo >= hi) return 0;
    const size_t item_bytes = (size_t)polys_per_item * kN * coeff_bits / 8;
    const size_t stage_bytes = options().db_stage_bytes;  // (tests force several passes)
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>({stage_bytes / item_bytes, (uint64_t)(1u << 16), hi - lo}));
    uint8_t* d_items = nullptr;
    uint32_t* d_err = nullptr;
    HIP_OK(hipMalloc(&d_items, chunk * item_bytes + 16));
    if (hipMalloc(&d_err, sizeof(uint32_t)) != hipSuccess || hipMemsetAsync(d_err, 0, sizeof(uint32_t), st) != hipSuccess) {
        (void)hipFree(d_items);
        return fail("device allocation failed");
    }
    hipError_t e = hipMemsetAsync(d_items + chunk * item_bytes, 0, 16, st);
    for (uint64_t done = lo; done < hi && e == hipSuccess; done += chunk) {
        const uint64_t n = std::min(chunk, hi - done);
        e = hipMemcpyAsync(d_items, (const uint8_t*)items + (size_t)(done - first) * item_bytes, (size_t)n * item_bytes, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) break;
        launch(d_items, d_err, done, n);
        e = hipStreamSynchronize(st);  // the staging buffer is reused by the next pass
    }
    uint32_t err = 0;
    if (e == hipSuccess) e = hipMemcpy(&err, d_err, sizeof(err), hipMemcpyDeviceToHost);
    (void)hipFree(d_items);
    (void)hipFree(d_err);
    if (e != hipSuccess) return fail("database ingest failed: %s", hipGetErrorString(e));
    if (err) return fail("a plaintext coefficient is not below p_db (the reference asserts, src/spiral.cpp:1117)");
    return 0;
}

// ---- tracked fingerprints (include/spiral_gpu.h "Fingerprints", Tracked) -------------------------------------------------------------------------
// The state an image's holder keeps between fingerprint_track and untrack (or the next loader): the key, its weight table and the accumulator words
// of F on the device ([sums][weights] in `aux`), and the table of polynomial sums, word (local item) * npolys + q.
struct FpTrack {
    bool on = false;
    uint64_t key[2] = {0, 0};
    DevBuf table, aux;
    uint32_t npolys = 0;     // polynomials held of an item
    uint64_t n_updates = 0;  // table words replaced since track
    uint64_t* sums() const { return aux.p; }
    const uint64_t* weights() const { return aux.p + kFpSumWords; }
    void release() {
        table.release();
        aux.release();
        on = false;
        n_updates = 0;
    }
    // room for `items` x `npolys` words and the weights of `key` on the device (uploaded on `st`); not `on` yet
    int reserve(const uint64_t k[2], uint64_t n_items, uint32_t polys, hipStream_t st) {
        release();
        if (table.alloc((size_t)n_items * polys) || aux.alloc(kFpSumWords + kFpWeightWords)) {
            (void)hipGetLastError();
            release();
            return fail("no device memory for the tracked fingerprint table (%llu bytes)", (unsigned long long)(n_items * polys * 8));
        }
        std::vector<uint64_t> w(kFpSumWords + kFpWeightWords, 0);
        fp_build_weights(k, w.data() + kFpSumWords);
        HIP_OK(hipMemcpyAsync(aux.p, w.data(), w.size() * 8, hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));  // (w goes out of scope)
        key[0] = k[0], key[1] = k[1];
        npolys = polys;
        return 0;
    }
};
// What an update call needs to keep a tracked image's table and F current: polynomial m of the call's item (j local, column ii local) is table word
// (j * num_per + ii) * t->npolys + q0 + m and polynomial poly0 + q0 + m of database item db_index(j, ii).  Null where the image is not tracked.
struct FpTrackCtx {
    FpTrack* t = nullptr;
    uint32_t q0 = 0, poly0 = 0;
    std::function<uint64_t(uint32_t, uint32_t)> db_index;
    uint64_t entry_y(uint32_t j, uint32_t ii, uint32_t num_per, uint32_t m) const {
        return ((((uint64_t)j * num_per + ii) * t->npolys + q0 + m) << 8) | (poly0 + q0 + m);
    }
};

// ---- in-place item updates (update_db_items of both servers) ---------------------------------------------------------------------
// The image holder's workspace, reused from call to call: a pinned host buffer holding what goes up (error word, work entries, the raw items) and
// one device buffer holding the same plus the encoded items.  `done` is recorded on the holder's stream after an update's launches: the next
// update waits for it (the previous update only, not the device) before it rewrites either buffer.
struct UpdateWork {
    DevBuf dev;
    uint8_t* host = nullptr;
    size_t host_bytes = 0;
    hipEvent_t done = nullptr;
    bool pending = false;
    void release() {
        if (pending && done) (void)hipEventSynchronize(done);
        dev.release();
        dev.words = 0;
        if (host) (void)hipHostFree(host);
        host = nullptr;
        host_bytes = 0;
        if (done) (void)hipEventDestroy(done);
        done = nullptr;
        pending = false;
    }
};

// the ids of an update call: every one below `total`, no two equal (checked before anything else happens)
inline int check_update_ids(const void* items, const uint64_t* ids, uint64_t n, uint64_t total) {
    if (n == 0) return 0;
    if (!items || !ids) return fail("null argument");
    if (n > (1ull << 24)) return fail("at most 2^24 items per update");
    std::vector<uint64_t> sorted(ids, ids + n);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.back() >= total) return fail("item id %llu outside the database of %llu items", (unsigned long long)sorted.back(), (unsigned long long)total);
    for (uint64_t k = 1; k < n; k++)
        if (sorted[k] == sorted[k - 1]) return fail("item id %llu given twice", (unsigned long long)sorted[k]);
    return 0;
}

// true when every one of the `count` coeff_bits-wide coefficients at `item` (read as packed_coeff reads them) is below p_db
inline bool coeffs_below(const uint8_t* item, size_t count, uint32_t coeff_bits, uint64_t p_db) {
    if (coeff_bits == 64) {
        for (size_t i = 0; i < count; i++) {
            uint64_t v;
            memcpy(&v, item + 8 * i, 8);
            if (v >= p_db) return false;
        }
        return true;
    }
    if ((1ull << coeff_bits) <= p_db) return true;  // (every coefficient of that width is)
    const uint64_t mask = (1ull << coeff_bits) - 1;
    for (size_t i = 0; i < count; i++) {
        const uint64_t bit = (uint64_t)i * coeff_bits;
        const uint32_t sh = (uint32_t)(bit & 7u), nbytes = (sh + coeff_bits + 7u) / 8u;
        uint64_t w = 0;
        memcpy(&w, item + (bit >> 3), nbytes);  // (little-endian host, as the device)
        if (((w >> sh) & mask) >= p_db) return false;
    }
    return true;
}

// One image's items to update: sel[k] = {position of the item in the caller's list, j local to the image, column ii}.
struct UpdateItem {
    uint64_t src;
    uint32_t j, ii;
};
struct UpdateImage {
    uint64_t* packed;  // the image in packed form (null: none)
    uint64_t* limbs;   // the image in limb-plane form (null: none)
    uint32_t pack, num_per, dim0;
};
// the scatter's work entries (kernels.h DbUpdateParams) for the items sel[k] = encoded item k: one per item for the packed form; one per partner pair
// (j, j ^ 32 / j ^ 64 of a column) for the limb planes
inline void update_entries(const std::vector<UpdateItem>& sel, const UpdateImage& img, std::vector<uint4>& put, std::vector<uint4>& pairs) {
    const size_t n = sel.size();
    if (img.packed) {
        put.reserve(n);
        for (size_t k = 0; k < n; k++) put.push_back(make_uint4((uint32_t)k, sel[k].j, sel[k].ii, 0u));
    }
    if (img.limbs) {
        const uint32_t bit = img.pack ? 64u : 32u;
        std::vector<std::pair<uint64_t, uint32_t>> order(n);  // (column, j of the low partner) -> item
        for (size_t k = 0; k < n; k++) order[k] = {((uint64_t)sel[k].ii << 32) | (sel[k].j & ~bit), (uint32_t)k};
        std::sort(order.begin(), order.end());
        for (size_t k = 0; k < n; k++) {
            const uint64_t key = order[k].first;
            if (pairs.empty() || (((uint64_t)pairs.back().x << 32) | pairs.back().y) != key)
                pairs.push_back(make_uint4((uint32_t)(key >> 32), (uint32_t)key, kDbUpdateNone, kDbUpdateNone));
            const uint32_t it = order[k].second;
            (sel[it].j & bit ? pairs.back().w : pairs.back().z) = it;
        }
    }
}
// the workspace of an update of n items: waits for the previous update's launches (they read the buffers), then grows the pinned buffer to up_bytes and
// the device buffer to dev_bytes
inline int update_reserve(UpdateWork& W, size_t n, size_t up_bytes, size_t dev_bytes) {
    if (W.pending) {
        HIP_OK(hipEventSynchronize(W.done));  // the previous update's launches have consumed the buffers
        W.pending = false;
    }
    if (!W.done && hipEventCreateWithFlags(&W.done, hipEventDisableTiming) != hipSuccess) return fail("hipEventCreate failed");
    if (W.host_bytes < up_bytes) {
        if (W.host) (void)hipHostFree(W.host);
        W.host = nullptr;
        W.host_bytes = 0;
        if (hipHostMalloc((void**)&W.host, up_bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return fail("no pinned host memory for an update of %zu items (%zu bytes)", n, up_bytes);
        }
        W.host_bytes = up_bytes;
    }
    if (W.dev.words * 8 < dev_bytes) {
        W.dev.release();
        W.dev.words = 0;
        if (W.dev.alloc((dev_bytes + 7) / 8)) {
            (void)hipGetLastError();
            W.dev.p = nullptr;
            W.dev.words = 0;
            return fail("no device memory for an update of %zu items (%zu bytes)", n, dev_bytes);
        }
    }
    return 0;
}
// The shared body of update_db_items: checks the coefficients on the host, then ONE upload, ONE encode launch (the ingest transform, linear store)
// and ONE scatter launch (db_update.hip) on `st`, and returns -- the caller's buffers are copied by then.  Nothing touches the image before every
// check has passed; the scatter kernel also skips everything when the encode launch flags a coefficient.
inline int update_items(UpdateWork& W, const DeviceTables& tb, hipStream_t st, const void* items, uint32_t coeff_bits, uint64_t p_db,
                        const std::vector<UpdateItem>& sel, const UpdateImage& img, const FpTrackCtx* trk = nullptr) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_OK(hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail("update_db_items cannot be called while the server's stream is being captured");
    if (coeff_bits != 64 && (coeff_bits < 1 || coeff_bits > 40)) return fail("coefficient width %u not in 1..40 or 64", coeff_bits);
    if (coeff_bits < 64 && (1ull << coeff_bits) < p_db) return fail("%u-bit coefficients cannot hold values below p_db", coeff_bits);
    if (sel.empty()) return 0;
    const uint32_t polys = img.pack ? 1u : 4u;
    const size_t item_bytes = (size_t)polys * kN * coeff_bits / 8, n = sel.size();
    const uint8_t* src = static_cast<const uint8_t*>(items);
    for (const UpdateItem& it : sel)
        if (!coeffs_below(src + it.src * item_bytes, (size_t)polys * kN, coeff_bits, p_db))
            return fail("a plaintext coefficient of item %llu of the list is not below p_db", (unsigned long long)it.src);
    std::vector<uint4> put, pairs;
    update_entries(sel, img, put, pairs);
    // one buffer: [error word][put][pairs][raw items + 16 bytes of over-read room] ++ (device only) [encoded items]
    // a tracked image: [..][raw items + 16][apply entries] ++ (device only) [encoded items][new polynomial sums]
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t o_put = 16, o_pairs = o_put + put.size() * sizeof(uint4), o_items = up16(o_pairs + pairs.size() * sizeof(uint4));
    const size_t o_app = up16(o_items + n * item_bytes + 16), n_app = trk ? n * polys : 0;
    const size_t up_bytes = o_app + n_app * sizeof(ulonglong2), o_gnew = up_bytes + n * polys * kPolyBytes, dev_bytes = o_gnew + n_app * 8;
    if (update_reserve(W, n, up_bytes, dev_bytes)) return -1;
    memset(W.host, 0, up_bytes);
    if (trk) {
        ulonglong2* app = reinterpret_cast<ulonglong2*>(W.host + o_app);
        for (size_t k = 0; k < n; k++)
            for (uint32_t m = 0; m < polys; m++) app[k * polys + m] = make_ulonglong2(trk->db_index(sel[k].j, sel[k].ii), trk->entry_y(sel[k].j, sel[k].ii, img.num_per, m));
    }
    if (!put.empty()) memcpy(W.host + o_put, put.data(), put.size() * sizeof(uint4));
    if (!pairs.empty()) memcpy(W.host + o_pairs, pairs.data(), pairs.size() * sizeof(uint4));
    for (size_t k = 0; k < n; k++) memcpy(W.host + o_items + k * item_bytes, src + sel[k].src * item_bytes, item_bytes);
    uint8_t* d = reinterpret_cast<uint8_t*>(W.dev.p);
    HIP_OK(hipMemcpyAsync(d, W.host, up_bytes, hipMemcpyHostToDevice, st));
    uint64_t* enc = reinterpret_cast<uint64_t*>(d + up_bytes);
    FwdJob encode = db_encode_job(img.pack ? LD_DBGEN1 : LD_DBGEN, ST_PK, enc, p_db);  // (a linear store: no geometry)
    db_encode_staged(encode, d + o_items, coeff_bits, reinterpret_cast<uint32_t*>(d), 0, (uint32_t)(n * polys));
    launch_job(tb, encode, st);
    DbUpdateParams up{};
    up.enc = enc;
    up.err = reinterpret_cast<const uint32_t*>(d);
    up.packed = img.packed;
    up.limbs = img.limbs;
    up.put = reinterpret_cast<const uint4*>(d + o_put);
    up.pairs = reinterpret_cast<const uint4*>(d + o_pairs);
    up.n_put = (uint32_t)put.size();
    up.n_pairs = (uint32_t)pairs.size();
    up.pack = img.pack;
    up.num_per = img.num_per;
    up.dim0 = img.dim0;
    launch_db_update(up, st);
    if (trk) {  // the table and F follow, from the staged stream: the image is not read
        FpStreamParams sp{};
        sp.items = d + o_items;
        sp.weights = trk->t->weights();
        sp.gnew = reinterpret_cast<uint64_t*>(d + o_gnew);
        sp.err = up.err;
        sp.n_polys = (uint32_t)n_app;
        sp.coeff_bits = coeff_bits;
        launch_fingerprint_stream(sp, st);
        FpApplyParams ap{};
        ap.entries = reinterpret_cast<const ulonglong2*>(d + o_app);
        ap.gnew = sp.gnew;
        ap.table = trk->t->table.p;
        ap.weights = sp.weights;
        ap.sums = trk->t->sums();
        ap.err = up.err;
        ap.n = (uint32_t)n_app;
        launch_fingerprint_apply(ap, st);
        trk->t->n_updates += n_app;  // (every check has passed on the host: the launches above do apply)
    }
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(W.done, st));
    W.pending = true;
    return 0;
}

// ---- items out of the image as plaintexts (read_db_items / read_db_items_at of both servers): the mirror of ingest_items ------------------------
// the coefficient width of an exported item stream: 1 .. 64 bits, wide enough for every value below p_db (64 always is)
inline int check_export_width(uint32_t coeff_bits, uint64_t p_db) {
    if (coeff_bits < 1 || coeff_bits > 64) return fail("coeff_bits = %u is not in 1..64", coeff_bits);
    if (coeff_bits < 64 && (1ull << coeff_bits) < p_db) return fail("coeff_bits = %u cannot hold values below p_db = %llu", coeff_bits, (unsigned long long)p_db);
    return 0;
}
// A server's workspace, reused from call to call: one device buffer [error word][work table][staged items] and, for the _at form, a pinned bounce
// buffer of one pass.  Per server, not per image: lanes read their owner's image on their own streams.
struct ExportWork {
    DevBuf dev;
    uint8_t* host = nullptr;
    size_t host_bytes = 0;
    std::vector<hipEvent_t> ev;  // two per pass, around its launch: the call's device time without its copies (option "db_export_ns")
    void release() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        ev.clear();
        dev.release();
        dev.words = 0;
        if (host) (void)hipHostFree(host);
        host = nullptr;
        host_bytes = 0;
    }
};
// the image as the export reads it: `db` in the form `form` names (kernels.h DbExportForm), dim0 = the shard's first dimension on the base path
struct ExportImage {
    const uint64_t* db;
    uint32_t pack, form, num_per, dim0;
};
// one item of an _at call that this server holds: its position in the caller's list, j local to the image, column ii
struct ExportItem {
    uint64_t pos;
    uint32_t j, ii;
};
// The shared body.  Range form (sel == null): the n LOCAL items first_l .. first_l + n - 1 (local item = j local * num_per + ii) go to positions
// pos0 .. pos0 + n - 1 of `items`; table form: item sel[k] goes to position sel[k].pos.  Position k of `items` is at byte k * item_bytes; bytes of other
// positions are not touched.  Staged in passes of option db_stage_bytes: one launch and one device-to-host copy per pass, one read of the error word at
// the end.  Returns after `st` is synchronised.  item_of(position): the database index the failure message names.
template <class ItemOf>
inline int export_items(ExportWork& W, const DeviceTables& tb, hipStream_t st, void* items, uint32_t coeff_bits, uint64_t p_db, const ExportImage& img,
                        uint64_t first_l, uint64_t n, uint64_t pos0, const std::vector<ExportItem>* sel, ItemOf item_of) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_OK(hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail("read_db_items cannot be called while the server's stream is being captured");
    if (check_export_width(coeff_bits, p_db)) return -1;
    if (sel) n = sel->size();
    if (n == 0) return 0;
    if (n > 0xFFFFFFFFull) return fail("at most 2^32 - 1 items per read");
    const uint32_t polys = img.pack ? 1u : 4u;
    const size_t item_bytes = (size_t)polys * kN * coeff_bits / 8;
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>({options().db_stage_bytes / item_bytes, (uint64_t)(1u << 18), n}));  // (tests force several passes)
    // the work table of the _at form, in the block order of a range export (db_export.hip): band of rows, group of columns
    std::vector<uint4> table;
    if (sel) {
        const uint32_t rows = img.pack ? 16u : 8u, cols = img.pack ? 8u : 4u;
        std::vector<ExportItem> order(*sel);
        auto key = [&](const ExportItem& e) { return ((uint64_t)(e.j / rows) << 40) | ((uint64_t)(e.ii / cols) << 20) | ((uint64_t)(e.j % rows) << 8) | (e.ii % cols); };
        std::stable_sort(order.begin(), order.end(), [&](const ExportItem& a, const ExportItem& b) { return key(a) < key(b); });
        table.reserve(n);
        for (uint64_t k = 0; k < n; k++) table.push_back(make_uint4(order[k].j, order[k].ii, (uint32_t)(k % chunk), (uint32_t)order[k].pos));
    }
    const size_t o_table = 16, o_stage = o_table + table.size() * sizeof(uint4), dev_bytes = o_stage + chunk * item_bytes;
    if (W.dev.words * 8 < dev_bytes) {
        W.dev.release();
        W.dev.words = 0;
        if (W.dev.alloc((dev_bytes + 7) / 8)) {
            (void)hipGetLastError();
            W.dev.p = nullptr;
            W.dev.words = 0;
            return fail("no device memory for the export's staging (%zu bytes)", dev_bytes);
        }
    }
    if (sel && W.host_bytes < chunk * item_bytes) {
        if (W.host) (void)hipHostFree(W.host);
        W.host = nullptr;
        W.host_bytes = 0;
        if (hipHostMalloc((void**)&W.host, chunk * item_bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return fail("no pinned host memory for the export's bounce buffer (%zu bytes)", (size_t)(chunk * item_bytes));
        }
        W.host_bytes = chunk * item_bytes;
    }
    uint8_t* d = reinterpret_cast<uint8_t*>(W.dev.p);
    uint8_t* out = static_cast<uint8_t*>(items);
    HIP_OK(hipMemsetAsync(d, 0xFF, 16, st));  // the error word: ~0 = every coefficient so far is a plaintext's
    if (sel) HIP_OK(hipMemcpyAsync(d + o_table, table.data(), table.size() * sizeof(uint4), hipMemcpyHostToDevice, st));
    DbExportParams xp{};
    xp.db = img.db;
    xp.out = d + o_stage;
    xp.err = reinterpret_cast<unsigned long long*>(d);
    xp.pack = img.pack;
    xp.form = img.form;
    xp.num_per = img.num_per;
    xp.dim0 = img.dim0;
    xp.coeff_bits = coeff_bits;
    xp.p_db = p_db;
    const size_t passes = (size_t)((n + chunk - 1) / chunk);
    while (W.ev.size() < 2 * passes) {
        hipEvent_t e = nullptr;
        HIP_OK(hipEventCreate(&e));
        W.ev.push_back(e);
    }
    for (uint64_t done = 0; done < n; done += chunk) {
        const uint64_t cnt = std::min(chunk, n - done);
        const size_t pass = (size_t)(done / chunk);
        xp.n = (uint32_t)cnt;
        if (sel) {
            xp.table = reinterpret_cast<const uint4*>(d + o_table) + done;
        } else {
            xp.first = first_l + done;
            xp.pos_base = pos0 + done;
        }
        HIP_OK(hipEventRecord(W.ev[2 * pass], st));
        launch_db_export(tb, xp, st);
        HIP_OK(hipGetLastError());
        HIP_OK(hipEventRecord(W.ev[2 * pass + 1], st));
        if (sel) {  // through the bounce buffer to the items' places
            HIP_OK(hipMemcpyAsync(W.host, xp.out, (size_t)cnt * item_bytes, hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            for (uint64_t k = 0; k < cnt; k++) memcpy(out + (size_t)table[done + k].w * item_bytes, W.host + (size_t)k * item_bytes, item_bytes);
        } else {  // (stream order keeps the next pass's launch behind this copy)
            HIP_OK(hipMemcpyAsync(out + (size_t)(pos0 + done) * item_bytes, xp.out, (size_t)cnt * item_bytes, hipMemcpyDeviceToHost, st));
        }
    }
    unsigned long long err = 0;
    HIP_OK(hipMemcpyAsync(&err, d, sizeof(err), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    double dev_ms = 0;
    for (size_t k = 0; k < passes; k++) {
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, W.ev[2 * k], W.ev[2 * k + 1]));
        dev_ms += ms;
    }
    g_db_export_ns.store((uint64_t)(dev_ms * 1e6));
    if (err != ~0ull) {
        const uint64_t poly = err / kN, pos = poly / polys;
        return fail("the image holds no plaintext at item %llu (polynomial %u, coefficient %u lifts to a value outside the centred range of p_db): "
                    "not a plaintext image (fill_db_random, or a load_db of arbitrary words)",
                    (unsigned long long)item_of(pos), (uint32_t)(poly % polys), (uint32_t)(err % kN));
    }
    return 0;
}

// ---- content fingerprints of the image (fingerprint_items / fingerprint_items_at of both servers; include/spiral_gpu.h "Fingerprints") ----------
// What a server holds of a fingerprint call, as the export's selection plus each item's database index.
//   range form (sel == null): the n LOCAL items first_l .. first_l + n - 1; local item first_l + k is database item idx0 + k * stride and position
//       pos0 + k * stride of the call (stride = the column shards G, else 1) -- affine, so nothing here grows with n;
//   table form: item sel[k] is the call's position sel[k].pos, database item ids[sel[k].pos].
struct FingerprintSel {
    uint64_t first_l = 0, n = 0, idx0 = 0, stride = 1, pos0 = 0;
    const std::vector<ExportItem>* sel = nullptr;
    const uint64_t* ids = nullptr;
};
// A range-form call on behalf of a tracked table (word (local item) * npolys + q, pointers at local item 0):
//   store:   fingerprint_track -- the first launch stores a pass's words straight into the table, and the call's accumulator words go to `sums`;
//   compare: fingerprint_scrub -- a compare launch per pass in place of the combine, the count and the lowest (item * 256 + polynomial) to n_bad, first_bad.
struct FingerprintTable {
    uint64_t* store = nullptr;
    uint64_t* sums = nullptr;
    const uint64_t* compare = nullptr;
    uint64_t n_bad = 0, first_bad = ~0ull;
};
// The shared body, on the export's workspace and with its conventions (passes, error word, events).  img: the image of the first polynomial this server
// holds; it holds npolys of an item's polynomials from poly0 on (base: 4 from 0; SpiralPack: its trial images, trial_words apart).  per_item (null: not
// wanted) has n_call words: every one is written, 0 for an item this server does not hold.  *combined (null: not wanted): this server's partial of F.
// One pass is two launches; a pass's per-polynomial words and item values are staged within option db_stage_bytes.  Returns after `st` is synchronised.
// ft (range form only; null: none): the call serves a tracked table -- FingerprintTable above.
inline int fingerprint_items(ExportWork& W, const DeviceTables& tb, hipStream_t st, const uint64_t key[2], uint64_t p_db, const ExportImage& img,
                             uint64_t trial_words, uint32_t npolys, uint32_t poly0, const FingerprintSel& fs, uint64_t n_call, uint64_t* per_item,
                             uint64_t* combined, FingerprintTable* ft = nullptr) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_OK(hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail("fingerprint_items cannot be called while the server's stream is being captured");
    const uint64_t n = fs.sel ? fs.sel->size() : fs.n, stride = fs.sel ? 1 : fs.stride;
    if (combined) *combined = 0;
    if (n == 0 || npolys == 0) {
        if (per_item) memset(per_item, 0, (size_t)n_call * 8);
        return 0;
    }
    if (n > 0xFFFFFFFFull) return fail("at most 2^32 - 1 items per fingerprint call");
    // a pass: a power of two of items (so that a power-of-two database goes through in whole passes, each of whole bands), within the staging bound
    // and far below the launch limit of 2^31 workgroups
    uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(options().db_stage_bytes / (8ull * (npolys + stride)), 1ull << 28));  // (tests force several passes)
    while (chunk & (chunk - 1)) chunk &= chunk - 1;
    chunk = std::min(chunk, n);
    std::vector<uint4> table;
    std::vector<uint64_t> ids;
    if (fs.sel) {  // the export's sorted work table (export_items), and the database index of each entry
        const uint32_t rows = img.pack ? 16u : 8u, cols = img.pack ? 8u : 4u;
        std::vector<ExportItem> order(*fs.sel);
        auto okey = [&](const ExportItem& e) { return ((uint64_t)(e.j / rows) << 40) | ((uint64_t)(e.ii / cols) << 20) | ((uint64_t)(e.j % rows) << 8) | (e.ii % cols); };
        std::stable_sort(order.begin(), order.end(), [&](const ExportItem& a, const ExportItem& b) { return okey(a) < okey(b); });
        table.reserve(n);
        ids.reserve(n);
        for (uint64_t k = 0; k < n; k++) {
            table.push_back(make_uint4(order[k].j, order[k].ii, (uint32_t)(k % chunk), (uint32_t)order[k].pos));
            ids.push_back(fs.ids[order[k].pos]);
        }
    }
    // [error word][sums][weights][table][ids][a pass's polynomial words][a pass's item values][a scrub's two words]
    const size_t o_sums = 16, o_w = o_sums + kFpSumWords * 8, o_table = o_w + kFpWeightWords * 8, o_ids = o_table + table.size() * sizeof(uint4);
    const size_t o_part = o_ids + ids.size() * 8, o_item = o_part + (size_t)chunk * npolys * 8, item_words = (size_t)(chunk * stride);
    const size_t o_scrub = o_item + item_words * 8, dev_bytes = o_scrub + 16;
    if (W.dev.words * 8 < dev_bytes) {
        W.dev.release();
        W.dev.words = 0;
        if (W.dev.alloc((dev_bytes + 7) / 8)) {
            (void)hipGetLastError();
            W.dev.p = nullptr;
            W.dev.words = 0;
            return fail("no device memory for the fingerprint's staging (%zu bytes)", dev_bytes);
        }
    }
    uint64_t weights[kFpWeightWords];
    fp_build_weights(key, weights);
    uint8_t* d = reinterpret_cast<uint8_t*>(W.dev.p);
    HIP_OK(hipMemsetAsync(d, 0xFF, 16, st));  // the error word: ~0 = every coefficient so far is a plaintext's
    HIP_OK(hipMemsetAsync(d + o_sums, 0, kFpSumWords * 8, st));
    HIP_OK(hipMemcpyAsync(d + o_w, weights, sizeof(weights), hipMemcpyHostToDevice, st));
    if (ft && ft->compare) {
        HIP_OK(hipMemsetAsync(d + o_scrub, 0, 8, st));
        HIP_OK(hipMemsetAsync(d + o_scrub + 8, 0xFF, 8, st));
    }
    if (fs.sel) {
        HIP_OK(hipMemcpyAsync(d + o_table, table.data(), table.size() * sizeof(uint4), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(d + o_ids, ids.data(), ids.size() * 8, hipMemcpyHostToDevice, st));
    }
    DbFingerprintParams fp{};
    fp.db = img.db;
    fp.trial_words = trial_words;
    fp.weights = reinterpret_cast<const uint64_t*>(d + o_w);
    fp.part = reinterpret_cast<uint64_t*>(d + o_part);
    fp.err = reinterpret_cast<unsigned long long*>(d);
    fp.pack = img.pack;
    fp.form = img.form;
    fp.num_per = img.num_per;
    fp.dim0 = img.dim0;
    fp.npolys = npolys;
    fp.p_db = p_db;
    DbFingerprintCombineParams cp{};
    cp.part = fp.part;
    cp.weights = fp.weights;
    cp.item_f = per_item ? reinterpret_cast<uint64_t*>(d + o_item) : nullptr;
    cp.out_stride = stride;
    cp.sums = reinterpret_cast<uint64_t*>(d + o_sums);
    cp.npolys = npolys;
    cp.poly0 = poly0;
    cp.idx_stride = stride;
    const size_t passes = (size_t)((n + chunk - 1) / chunk);
    while (W.ev.size() < 2 * passes) {
        hipEvent_t e = nullptr;
        HIP_OK(hipEventCreate(&e));
        W.ev.push_back(e);
    }
    std::vector<uint64_t> bounce;  // table form: a pass's item values on their way to the positions of the caller's list
    if (per_item) {
        if (fs.sel) {
            memset(per_item, 0, (size_t)n_call * 8);
            bounce.resize(chunk);
        } else {  // what lies before the first and behind the last item held
            const uint64_t end = fs.pos0 + (n - 1) * stride + 1;
            memset(per_item, 0, (size_t)fs.pos0 * 8);
            memset(per_item + end, 0, (size_t)(n_call - end) * 8);
        }
    }
    for (uint64_t done = 0; done < n; done += chunk) {
        const uint64_t cnt = std::min(chunk, n - done);
        const size_t pass = (size_t)(done / chunk);
        fp.n = (uint32_t)cnt;
        cp.n = cnt;
        // a column shard's items lie `stride` apart: every pass but the last also zeroes the stride - 1 words behind its last item, up to the next pass's first
        cp.out_words = done + cnt < n ? cnt * stride : (cnt - 1) * stride + 1;
        if (fs.sel) {
            fp.table = reinterpret_cast<const uint4*>(d + o_table) + done;
            cp.ids = reinterpret_cast<const uint64_t*>(d + o_ids) + done;
        } else {
            fp.first = fs.first_l + done;
            fp.pos_base = done;
            cp.idx0 = fs.idx0 + done * stride;
        }
        if (ft && ft->store) cp.part = fp.part = ft->store + (size_t)(fs.first_l + done) * npolys;
        HIP_OK(hipEventRecord(W.ev[2 * pass], st));
        launch_db_fingerprint(tb, fp, st);
        if (ft && ft->compare) {
            FpCompareParams mp{};
            mp.part = fp.part;
            mp.table = ft->compare + (size_t)(fs.first_l + done) * npolys;
            mp.out = reinterpret_cast<unsigned long long*>(d + o_scrub);
            mp.n_words = cnt * npolys;
            mp.idx0 = cp.idx0;
            mp.idx_stride = stride;
            mp.npolys = npolys;
            mp.poly0 = poly0;
            launch_fingerprint_compare(mp, st);
        } else {
            launch_db_fingerprint_combine(cp, st);
        }
        HIP_OK(hipGetLastError());
        HIP_OK(hipEventRecord(W.ev[2 * pass + 1], st));
        if (!per_item) continue;
        if (fs.sel) {
            HIP_OK(hipMemcpyAsync(bounce.data(), cp.item_f, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            for (uint64_t k = 0; k < cnt; k++) per_item[table[done + k].w] = bounce[k];
        } else {  // (stream order keeps the next pass's launches behind this copy)
            HIP_OK(hipMemcpyAsync(per_item + fs.pos0 + done * stride, cp.item_f, (size_t)cp.out_words * 8, hipMemcpyDeviceToHost, st));
        }
    }
    struct {
        unsigned long long err;
        uint64_t pad, sums[kFpSumWords];
    } back;
    static_assert(sizeof(back) == 16 + kFpSumWords * 8, "the error word and the sums lie back to back");
    HIP_OK(hipMemcpyAsync(&back, d, sizeof(back), hipMemcpyDeviceToHost, st));
    uint64_t scrub[2] = {0, ~0ull};
    if (ft && ft->compare) HIP_OK(hipMemcpyAsync(scrub, d + o_scrub, 16, hipMemcpyDeviceToHost, st));
    if (ft && ft->sums) HIP_OK(hipMemcpyAsync(ft->sums, d + o_sums, kFpSumWords * 8, hipMemcpyDeviceToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
    if (ft) ft->n_bad = scrub[0], ft->first_bad = scrub[1];
    double dev_ms = 0;
    for (size_t k = 0; k < passes; k++) {
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, W.ev[2 * k], W.ev[2 * k + 1]));
        dev_ms += ms;
    }
    g_db_fingerprint_ns.store((uint64_t)(dev_ms * 1e6));
    if (back.err != ~0ull) {
        const uint64_t poly = back.err / kN, pos = poly / npolys;  // (range form: the position among the items held)
        return fail("the image holds no plaintext at item %llu (polynomial %u, coefficient %u lifts to a value outside the centred range of p_db): "
                    "not a plaintext image (fill_db_random, or a load_db of arbitrary words)",
                    (unsigned long long)(fs.sel ? fs.ids[pos] : fs.idx0 + pos * stride), poly0 + (uint32_t)(poly % npolys), (uint32_t)(back.err % kN));
    }
    if (combined) {
        uint64_t F = 0;
        for (uint32_t k = 0; k < kFpSumWords; k++) F = fp_add(F, back.sums[k]);
        *combined = F;
    }
    return 0;
}

// ---- tracked fingerprints: the calls' shared bodies (both servers; include/spiral_gpu.h "Fingerprints", Tracked) ----------------------------------
// The server's local items are database items idx0 + l * stride, l = 0 .. n_local - 1 (fingerprint_items' affine map), and it holds npolys polynomials of
// each from poly0 on.
struct FpTrackGeom {
    uint64_t n_local, idx0, stride;
    uint32_t npolys, poly0;
};
// fingerprint_track: the table and F from the image in its current form (poly_sums null: fingerprint_items' passes, the first launch storing into the
// table), or from an adopted table (one upload and the combine launch; the image is not read).  On failure tracking is off.
inline int fingerprint_track(FpTrack& T, ExportWork& W, const DeviceTables& tb, hipStream_t st, const uint64_t key[2], uint64_t p_db, const ExportImage& img,
                             uint64_t trial_words, const FpTrackGeom& g, const uint64_t* poly_sums) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_OK(hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail("fingerprint_track cannot be called while the server's stream is being captured");
    const uint64_t words = g.n_local * g.npolys;
    if (poly_sums)
        for (uint64_t k = 0; k < words; k++)
            if (poly_sums[k] >= kFpP)
                return fail("word %llu of the polynomial sums is %llu: not below 2^61 - 1", (unsigned long long)k, (unsigned long long)poly_sums[k]);
    T.release();
    if (T.reserve(key, g.n_local, g.npolys, st)) {
        T.release();
        return -1;
    }
    if (!poly_sums) {
        FingerprintSel fs;
        fs.n = g.n_local;
        fs.idx0 = g.idx0;
        fs.stride = g.stride;
        FingerprintTable ft;
        ft.store = T.table.p;
        ft.sums = T.sums();
        uint64_t F = 0;
        if (fingerprint_items(W, tb, st, key, p_db, img, trial_words, g.npolys, g.poly0, fs, 0, nullptr, &F, &ft)) {
            T.release();
            return -1;
        }
    } else {
        DbFingerprintCombineParams cp{};
        cp.part = T.table.p;
        cp.weights = T.weights();
        cp.idx0 = g.idx0;
        cp.idx_stride = g.stride;
        cp.out_stride = 1;
        cp.sums = T.sums();
        cp.n = g.n_local;
        cp.npolys = g.npolys;
        cp.poly0 = g.poly0;
        hipError_t e = hipMemcpyAsync(T.table.p, poly_sums, (size_t)words * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            launch_db_fingerprint_combine(cp, st);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            T.release();
            return fail("adopting the polynomial sums failed: %s", hipGetErrorString(e));
        }
    }
    T.on = true;
    return 0;
}
inline int fingerprint_not_tracked() { return fail("the image's fingerprint is not tracked (fingerprint_track; a loader ends tracking)"); }
// fingerprint_tracked: F as the sum of the accumulator words, after `st`
inline int fingerprint_tracked(const FpTrack& T, hipStream_t st, uint64_t* key_out, uint64_t* combined, uint64_t* n_updates) {
    if (!T.on) return fingerprint_not_tracked();
    uint64_t sums[kFpSumWords];
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipMemcpyAsync(sums, T.sums(), sizeof(sums), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    uint64_t F = 0;
    for (uint32_t k = 0; k < kFpSumWords; k++) F = fp_add(F, sums[k]);
    if (key_out) key_out[0] = T.key[0], key_out[1] = T.key[1];
    if (combined) *combined = F;
    if (n_updates) *n_updates = T.n_updates;
    return 0;
}
// fingerprint_tracked_polys: the table's words of the n local items from first_l on, to items pos0, pos0 + stride, .. of the call's n_call; every other
// word of poly_sums[n_call][npolys] is 0
inline int fingerprint_tracked_polys(const FpTrack& T, hipStream_t st, uint64_t first_l, uint64_t n, uint64_t pos0, uint64_t stride, uint64_t n_call,
                                     uint64_t* poly_sums) {
    if (!T.on) return fingerprint_not_tracked();
    if (!poly_sums) return fail("null argument");
    const uint32_t np = T.npolys;
    HIP_OK(hipStreamSynchronize(st));
    if (stride == 1) {
        memset(poly_sums, 0, (size_t)pos0 * np * 8);
        memset(poly_sums + (pos0 + n) * np, 0, (size_t)(n_call - pos0 - n) * np * 8);
        if (n) HIP_OK(hipMemcpyAsync(poly_sums + pos0 * np, T.table.p + first_l * np, (size_t)n * np * 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        return 0;
    }
    std::vector<uint64_t> tmp((size_t)n * np);
    if (n) HIP_OK(hipMemcpyAsync(tmp.data(), T.table.p + first_l * np, tmp.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    memset(poly_sums, 0, (size_t)n_call * np * 8);
    for (uint64_t k = 0; k < n; k++) memcpy(poly_sums + (pos0 + k * stride) * np, tmp.data() + k * np, (size_t)np * 8);
    return 0;
}
// fingerprint_scrub: fingerprint_items' range form with the compare launch; *n_bad mismatching polynomials, the lowest (database item, polynomial) where any
inline int fingerprint_scrub(const FpTrack& T, ExportWork& W, const DeviceTables& tb, hipStream_t st, uint64_t p_db, const ExportImage& img, uint64_t trial_words,
                             uint32_t poly0, const FingerprintSel& fs, uint64_t* n_bad, uint64_t* first_bad_item, uint32_t* first_bad_poly) {
    if (!T.on) return fingerprint_not_tracked();
    FingerprintTable ft;
    ft.compare = T.table.p;
    if (fingerprint_items(W, tb, st, T.key, p_db, img, trial_words, T.npolys, poly0, fs, 0, nullptr, nullptr, &ft)) return -1;
    if (n_bad) *n_bad = ft.n_bad;
    if (ft.n_bad) {
        if (first_bad_item) *first_bad_item = ft.first_bad / kFpMaxPolys;
        if (first_bad_poly) *first_bad_poly = (uint32_t)(ft.first_bad % kFpMaxPolys);
    }
    return 0;
}

// upload reference NTT-form polynomials and convert to PK / the converse
inline uint64_t* upload_pk(Scratch& sc, const uint64_t* host_ref, size_t npolys) {
    uint64_t* d_ref = sc.upload(host_ref, npolys * kRefNtt);
    uint64_t* d_pk = sc.get(npolys * kN);
    if (!d_ref || !d_pk) return nullptr;
    launch_ref_to_pk(d_ref, d_pk, (uint32_t)npolys, identity_map(), 0);
    return d_pk;
}
inline int download_pk(Scratch& sc, const uint64_t* d_pk, IndexMap map, uint64_t* host_ref, size_t npolys) {
    uint64_t* d_ref = sc.get(npolys * kRefNtt);
    if (!d_ref) return fail("device allocation failed");
    launch_pk_to_ref(d_pk, d_ref, (uint32_t)npolys, map, 0);
    HIP_OK(hipMemcpy(host_ref, d_ref, npolys * kRefNtt * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace host
}  // namespace spiral
