// Keyed records, the server's probe (spiral_gpu_server_kv_put / _delete / _get; the definition is stated once in include/spiral_gpu.h "Keyed
// records", the work tables in kernels.h KvProbeParams).  One workgroup per distinct candidate bucket of a call: the record kernels' gather + inverse
// transform + unlift of polynomial 0 (db_plain_device.h), the header's tags packed at w bits in LDS, then 32 bytes of occupancy per bucket and 4 bytes
// per (key, candidate) go out -- the host never sees the headers.  The launch bounds are the export's and the record kernels' (256, 6): at the
// transforms' (256, 8) the getters' addresses spill.
//
// SpiralPack (spiral_gpu_pack_server_kv_*): the same body with PACK = true.  Polynomial 0 of a bucket is the bucket's item in trial image 0, so the
// launch takes trial 0's image and image_poly_plain<FORM, true> reads the packed or plain layout, the limb planes and the 8-column pair form.  The base
// kernels keep their names, arguments and resources (profiles/pack_kv_resource_usage.txt).
//
// Table occupancy (spiral_gpu_server_kv_stats / spiral_gpu_pack_server_kv_stats; kernels.h KvStatsParams): the probe's gather, transform and header
// packing over a range of buckets, whose (j, ii) come from the block index -- no table goes up -- and ONE integer atomic add per bucket into a
// histogram of used slots, 257 words that come back instead of the headers.
//
// Listing (spiral_gpu_server_kv_scan / _kv_scan_at and the SpiralPack twins; kernels.h KvScanParams): the same gather and header decode over a pass of
// buckets, then a stream compaction in three launches -- per-bucket counts, one workgroup's exclusive scan on top of a running total, entries written
// densely in (bucket, slot) order -- so only live entries come back.  No launch waits for another workgroup.
#include "db_plain_device.h"
#include "kernels.h"
#include "ntt_device.h"

namespace spiral {

namespace {

constexpr uint32_t kKvNoSlot = 0xFFFFFFFFu;

// tag `tid` of the header whose coefficients lie in sh: bits [64 tid, + 64) of the string of w-bit coefficients; w need not divide 64 (the header lies
// inside the polynomial: c < 2048).  0 for tid >= slots.  A header coefficient >= 2^w atomicMin's (err_base + coefficient) into *err.
__device__ __forceinline__ uint64_t kv_header_tag(const uint64_t* sh, uint32_t tid, uint32_t slots, uint32_t w, unsigned long long* err, unsigned long long err_base) {
    uint64_t tag = 0;
    if (tid < slots) {
        const uint32_t bit = 64u * tid;
        uint32_t c = bit / w, off = bit - c * w;
        for (uint32_t got = 0; got < 64u; c++) {
            const uint64_t v = sh[c];
            if (v >> w) atomicMin(err, err_base + c);
            const uint32_t take = min(w - off, 64u - got);  // <= w <= 40
            tag |= ((v >> off) & ((1ull << take) - 1ull)) << got;
            got += take;
            off = 0;
        }
    }
    return tag;
}

template <uint32_t FORM, bool PACK>
__device__ __forceinline__ void kv_probe_body(const Tables& t, const KvProbeParams& p, uint64_t* sh, uint64_t* tags) {
    const uint32_t tid = threadIdx.x, w = p.w;
    const uint4 e = p.entries[blockIdx.x];
    const uint32_t bad = image_poly_plain<FORM, PACK>(p.db, e.x, e.y, 0u, p.num_per, p.dim0, p.p_db, t.inv, sh, tid);
    if (bad < kN) atomicMin(p.err, (unsigned long long)blockIdx.x * kN + bad);
    __syncthreads();
    const uint64_t tag = kv_header_tag(sh, tid, p.slots, w, p.err, (unsigned long long)blockIdx.x * kN);
    tags[tid] = tag;
    const unsigned long long used = __ballot(tag != 0);
    if ((tid & 63u) == 0) p.occ[(size_t)blockIdx.x * 4u + (tid >> 6)] = used;
    __syncthreads();
    for (uint32_t l = tid; l < e.w; l += 256u) {
        const ulonglong2 look = p.lookups[e.z + l];
        uint32_t slot = kKvNoSlot;
        for (uint32_t s = 0; s < p.slots; s++)
            if (tags[s] == look.x) {
                slot = s;
                break;
            }
        p.slot_out[look.y] = slot;
    }
}

template <uint32_t FORM>
__global__ __launch_bounds__(256, 6) void kv_probe_kernel(Tables t, KvProbeParams p) {
    __shared__ uint64_t sh[kLdsWords];
    __shared__ uint64_t tags[256];
    kv_probe_body<FORM, false>(t, p, sh, tags);
}
template <uint32_t FORM>
__global__ __launch_bounds__(256, 6) void pack_kv_probe_kernel(Tables t, KvProbeParams p) {
    __shared__ uint64_t sh[kLdsWords];
    __shared__ uint64_t tags[256];
    kv_probe_body<FORM, true>(t, p, sh, tags);
}

// Workgroup g has bucket first_bucket + g (the host checks the range against nb < 2^31): image item (bucket / num_per, bucket % num_per).  The adds are
// integer, so the histogram is exact whatever the order the workgroups finish in.  (One bucket per workgroup: a loop over a stride of buckets keeps the
// probe's addresses live across iterations and spills at these launch bounds.)
template <uint32_t FORM, bool PACK>
__global__ __launch_bounds__(256, 6) void kv_stats_kernel(Tables t, KvStatsParams p) {
    __shared__ uint64_t sh[kLdsWords];
    __shared__ uint32_t used[4];
    const uint32_t tid = threadIdx.x, bucket = p.first_bucket + blockIdx.x;
    const uint32_t bad = image_poly_plain<FORM, PACK>(p.db, bucket / p.num_per, bucket % p.num_per, 0u, p.num_per, p.dim0, p.p_db, t.inv, sh, tid);
    if (bad < kN) atomicMin(p.err, (unsigned long long)bucket * kN + bad);
    __syncthreads();
    const uint64_t tag = kv_header_tag(sh, tid, p.slots, p.w, p.err, (unsigned long long)bucket * kN);
    const unsigned long long ballot = __ballot(tag != 0);
    if ((tid & 63u) == 0) used[tid >> 6] = (uint32_t)__popcll(ballot);
    __syncthreads();
    if (tid == 0) atomicAdd(&p.hist[used[0] + used[1] + used[2] + used[3]], 1ull);
}

template <uint32_t FORM, bool PACK>
void launch_kv_stats_form(const Tables& tb, const KvStatsParams& p, hipStream_t s) {
    constexpr uint32_t kMaxGrid = 1u << 23;  // workgroups per launch: grid x block stays below 2^32 threads, whatever the range
    for (uint32_t done = 0; done < p.n_buckets; done += kMaxGrid) {
        KvStatsParams q = p;
        q.first_bucket = p.first_bucket + done;
        q.n_buckets = std::min(kMaxGrid, p.n_buckets - done);
        hipLaunchKernelGGL((kv_stats_kernel<FORM, PACK>), dim3(q.n_buckets), dim3(256), 0, s, tb, q);
    }
}

// ---- Listing (kernels.h KvScanParams): decode, offsets, compact; three launches per pass, none of which waits for another workgroup ----------------
// the bucket of workgroup g of a pass: first + g, or the list's ids[first + g]
__device__ __forceinline__ uint32_t kv_scan_bucket(const KvScanParams& p, uint32_t g) { return p.ids ? p.ids[p.first + g] : p.first + g; }

// One bucket per workgroup, as kv_stats_kernel and for its reason.  The error word carries (first + g): the bucket of the range form, the position of
// the list form.
template <uint32_t FORM, bool PACK>
__global__ __launch_bounds__(256, 6) void kv_scan_decode_kernel(Tables t, KvScanParams p) {
    __shared__ uint64_t sh[kLdsWords];
    __shared__ uint32_t used[4];
    const uint32_t tid = threadIdx.x, g = blockIdx.x, bucket = kv_scan_bucket(p, g);
    const unsigned long long err_base = (unsigned long long)(p.first + g) * kN;
    const uint32_t bad = image_poly_plain<FORM, PACK>(p.db, bucket / p.num_per, bucket % p.num_per, 0u, p.num_per, p.dim0, p.p_db, t.inv, sh, tid);
    if (bad < kN) atomicMin(p.err, err_base + bad);
    __syncthreads();
    const uint64_t tag = kv_header_tag(sh, tid, p.slots, p.w, p.err, err_base);
    if (p.stage && tid < p.slots) p.stage[(size_t)g * p.slots + tid] = tag;
    const unsigned long long ballot = __ballot(tag != 0);
    if ((tid & 63u) == 0) used[tid >> 6] = (uint32_t)__popcll(ballot);
    __syncthreads();
    if (tid == 0) p.counts[g] = used[0] + used[1] + used[2] + used[3];
}

// ONE workgroup: the exclusive prefix sums of the pass's counts on top of the running total, 256 buckets a step (a wave's inclusive scan by shuffles,
// the four waves' sums through LDS), then the total moves on by the pass's sum.
__global__ __launch_bounds__(256) void kv_scan_offsets_kernel(KvScanParams p) {
    __shared__ uint32_t wsum[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    unsigned long long run = *p.total;  // (read by every thread; written below, behind the loop's barriers: n_buckets >= 1)
    for (uint32_t i0 = 0; i0 < p.n_buckets; i0 += 256u) {
        const uint32_t i = i0 + tid, c = i < p.n_buckets ? p.counts[i] : 0u;
        uint32_t x = c;
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63u) wsum[wave] = x;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t k = 0; k < 4u; k++) {
            if (k < wave) before += wsum[k];
            all += wsum[k];
        }
        if (i < p.n_buckets) p.offsets[i] = run + before + (x - c);
        run += all;
        __syncthreads();
    }
    if (tid == 0) *p.total = run;
}

// One workgroup per bucket: thread s has tag s of the staged header; its rank among the bucket's non-zero tags is the lower waves' counts plus the
// lower lanes of its own wave's ballot.  An entry goes out as ONE 16-byte vector store, and only where its index is below max_entries (the host's
// buffer holds min(max_entries, every slot of the call) entries).
__global__ __launch_bounds__(256) void kv_scan_compact_kernel(KvScanParams p) {
    __shared__ uint32_t used[4];
    const uint32_t tid = threadIdx.x, g = blockIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t tag = tid < p.slots ? p.stage[(size_t)g * p.slots + tid] : 0ull;
    const unsigned long long ballot = __ballot(tag != 0);
    if (lane == 0) used[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    if (tag == 0) return;
    uint32_t rank = (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
    for (uint32_t k = 0; k < wave; k++) rank += used[k];
    const unsigned long long at = p.offsets[g] + rank;
    if (at < p.max_entries) p.entries[at] = make_ulonglong2(tag, (unsigned long long)kv_scan_bucket(p, g) | ((unsigned long long)tid << 32));
}

}  // namespace

void launch_kv_scan_decode(const DeviceTables& t, const KvScanParams& p, bool pack, hipStream_t s) {
    if (p.n_buckets == 0) return;
    const Tables tb{t.fwd, t.inv};
    const dim3 grid(p.n_buckets), block(256);
    if (!pack) {
        if (p.form == DBX_PACKED)
            hipLaunchKernelGGL((kv_scan_decode_kernel<DBX_PACKED, false>), grid, block, 0, s, tb, p);
        else
            hipLaunchKernelGGL((kv_scan_decode_kernel<DBX_LIMBS, false>), grid, block, 0, s, tb, p);
    } else if (p.form == DBX_PACKED)
        hipLaunchKernelGGL((kv_scan_decode_kernel<DBX_PACKED, true>), grid, block, 0, s, tb, p);
    else if (p.form == DBX_LIMBS)
        hipLaunchKernelGGL((kv_scan_decode_kernel<DBX_LIMBS, true>), grid, block, 0, s, tb, p);
    else
        hipLaunchKernelGGL((kv_scan_decode_kernel<DBX_LIMBS8, true>), grid, block, 0, s, tb, p);
}

void launch_kv_scan_offsets(const KvScanParams& p, hipStream_t s) {
    if (p.n_buckets == 0) return;
    hipLaunchKernelGGL(kv_scan_offsets_kernel, dim3(1), dim3(256), 0, s, p);
}

void launch_kv_scan_compact(const KvScanParams& p, hipStream_t s) {
    if (p.n_buckets == 0) return;
    hipLaunchKernelGGL(kv_scan_compact_kernel, dim3(p.n_buckets), dim3(256), 0, s, p);
}

void launch_kv_probe(const DeviceTables& t, const KvProbeParams& p, bool pack, hipStream_t s) {
    if (p.n_entries == 0) return;
    const Tables tb{t.fwd, t.inv};
    const dim3 grid(p.n_entries), block(256);
    if (!pack) {
        if (p.form == DBX_PACKED)
            hipLaunchKernelGGL((kv_probe_kernel<DBX_PACKED>), grid, block, 0, s, tb, p);
        else
            hipLaunchKernelGGL((kv_probe_kernel<DBX_LIMBS>), grid, block, 0, s, tb, p);
    } else if (p.form == DBX_PACKED)
        hipLaunchKernelGGL((pack_kv_probe_kernel<DBX_PACKED>), grid, block, 0, s, tb, p);
    else if (p.form == DBX_LIMBS)
        hipLaunchKernelGGL((pack_kv_probe_kernel<DBX_LIMBS>), grid, block, 0, s, tb, p);
    else
        hipLaunchKernelGGL((pack_kv_probe_kernel<DBX_LIMBS8>), grid, block, 0, s, tb, p);
}

void launch_kv_stats(const DeviceTables& t, const KvStatsParams& p, bool pack, hipStream_t s) {
    if (p.n_buckets == 0) return;
    const Tables tb{t.fwd, t.inv};
    if (!pack) {
        if (p.form == DBX_PACKED)
            launch_kv_stats_form<DBX_PACKED, false>(tb, p, s);
        else
            launch_kv_stats_form<DBX_LIMBS, false>(tb, p, s);
    } else if (p.form == DBX_PACKED)
        launch_kv_stats_form<DBX_PACKED, true>(tb, p, s);
    else if (p.form == DBX_LIMBS)
        launch_kv_stats_form<DBX_LIMBS, true>(tb, p, s);
    else
        launch_kv_stats_form<DBX_LIMBS8, true>(tb, p, s);
}

}  // namespace spiral
