// Keyed records, the server's probe (spiral_gpu_server_kv_put / _delete / _get; the definition is stated once in include/spiral_gpu.h "Keyed
// records", the work tables in kernels.h KvProbeParams).  One workgroup per distinct candidate bucket of a call: the record kernels' gather + inverse
// transform + unlift of polynomial 0 (db_plain_device.h), the header's tags packed at w bits in LDS, then 32 bytes of occupancy per bucket and 4 bytes
// per (key, candidate) go out -- the host never sees the headers.  The launch bounds are the export's and the record kernels' (256, 6): at the
// transforms' (256, 8) the getters' addresses spill.
#include "db_plain_device.h"
#include "kernels.h"
#include "ntt_device.h"

namespace spiral {

namespace {

constexpr uint32_t kKvNoSlot = 0xFFFFFFFFu;

template <uint32_t FORM>
__global__ __launch_bounds__(256, 6) void kv_probe_kernel(Tables t, KvProbeParams p) {
    __shared__ uint64_t sh[kLdsWords];
    __shared__ uint64_t tags[256];
    const uint32_t tid = threadIdx.x, w = p.w;
    const uint4 e = p.entries[blockIdx.x];
    const uint32_t bad = image_poly_plain<FORM, false>(p.db, e.x, e.y, 0u, p.num_per, p.dim0, p.p_db, t.inv, sh, tid);
    if (bad < kN) atomicMin(p.err, (unsigned long long)blockIdx.x * kN + bad);
    __syncthreads();
    // tag s: bits [64 s, + 64) of the string of w-bit coefficients; w need not divide 64 (the header lies inside the polynomial: c < 2048)
    uint64_t tag = 0;
    if (tid < p.slots) {
        const uint32_t bit = 64u * tid;
        uint32_t c = bit / w, off = bit - c * w;
        for (uint32_t got = 0; got < 64u; c++) {
            const uint64_t v = sh[c];
            if (v >> w) atomicMin(p.err, (unsigned long long)blockIdx.x * kN + c);
            const uint32_t take = min(w - off, 64u - got);  // <= w <= 40
            tag |= ((v >> off) & ((1ull << take) - 1ull)) << got;
            got += take;
            off = 0;
        }
    }
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

}  // namespace

void launch_kv_probe(const DeviceTables& t, const KvProbeParams& p, hipStream_t s) {
    if (p.n_entries == 0) return;
    const Tables tb{t.fwd, t.inv};
    if (p.form == DBX_PACKED)
        hipLaunchKernelGGL((kv_probe_kernel<DBX_PACKED>), dim3(p.n_entries), dim3(256), 0, s, tb, p);
    else
        hipLaunchKernelGGL((kv_probe_kernel<DBX_LIMBS>), dim3(p.n_entries), dim3(256), 0, s, tb, p);
}

}  // namespace spiral
