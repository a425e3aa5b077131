// Client keys from a key store (key_store.h) into the key buffers of the lanes of one call: "lane q now serves the client of slot s" for all lanes
// in ONE launch (gridDim.z = lanes), the device half of spiral_gpu_server_bind_keys / spiral_gpu_pack_server_bind_keys.
//
// A workgroup takes one destination polynomial (16 KiB) at a time, grid-stride over the polynomials of all four parts of the lane.  Which part, and with
// it the destination pointer and the matrix shape, comes from the message layout the host passes: the four key buffers of an arena need not be
// contiguous.  A polynomial is 1024 16-byte words; thread t moves words t, t + 256, t + 512, t + 768, so every wave instruction covers 1 KiB of
// consecutive bytes on both sides, and the four loads are in flight before the first store.
// KEYS_COMPACT: a slot stores rows 1.. of every matrix only.  A row-0 polynomial is generated instead of copied, by the block function and the
// thread-to-word map of seed.hip (seed_device.h seed_store_pair) from the seed the slot opens with -- the words set_pub_params_seeded writes.
#include "common.h"
#include "kernels.h"
#include "seed_device.h"

namespace spiral {

namespace {

template <int FORM>
__global__ __launch_bounds__(256) void key_bind_kernel(KeyBindParams p) {
    const uint32_t z = blockIdx.z, t = threadIdx.x;
    uint32_t slot = p.slot[0];  // (a select chain, as Lanes::here: indexing the by-value argument would put it in scratch memory)
#pragma unroll
    for (uint32_t q = 1; q < kMaxLanes; q++) slot = z == q ? p.slot[q] : slot;
    const uint64_t* src = p.store + (size_t)slot * p.slot_words;
    const int64_t off = p.lanes.here();
    uint32_t key[8] = {};
    if (FORM == KEYS_COMPACT) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint64_t w = src[i];
            key[2 * i] = (uint32_t)w;
            key[2 * i + 1] = (uint32_t)(w >> 32);
        }
    }
    const uint32_t total = p.part[0].polys + p.part[1].polys + p.part[2].polys + p.part[3].polys;
    for (uint32_t j = blockIdx.x; j < total; j += gridDim.x) {
        // the part polynomial j belongs to (uniform over the workgroup; constant indices after unrolling)
        uint64_t* dst = nullptr;
        uint32_t local = 0, rows = 1, cols = 1, first_src = 0, row0 = 0, first = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (j >= first && j - first < p.part[i].polys) {
                dst = p.part[i].dst;
                local = j - first;
                rows = p.part[i].rows;
                cols = p.part[i].cols;
                first_src = p.part[i].src;
                row0 = p.part[i].row0;
            }
            first += p.part[i].polys;
        }
        uint64_t* out = dst + off + (size_t)local * kN;
        uint32_t from = first_src + local;
        if (FORM == KEYS_COMPACT) {
            const uint32_t rc = rows * cols, m = local / rc, w = local % rc;  // matrix m, polynomial w of it
            if (w < cols) {  // row 0: row-0 polynomial row0 + m * cols + w of the message
#pragma unroll
                for (uint32_t u = 0; u < 4; u++) seed_store_pair(key, p.domain, (uint64_t)row0 + (uint64_t)m * cols + w, u * 256u + t, [&] { return out; });
                continue;
            }
            from = first_src + m * (rc - cols) + (w - cols);  // rows 1.. of a matrix: a dense run of (rows - 1) * cols
        }
        const ulonglong2* s = reinterpret_cast<const ulonglong2*>(src + p.head + (size_t)from * kN);
        ulonglong2* d = reinterpret_cast<ulonglong2*>(out);
        const ulonglong2 v0 = s[t], v1 = s[256u + t], v2 = s[512u + t], v3 = s[768u + t];  // (no array: it would be promoted to LDS)
        d[t] = v0;
        d[256u + t] = v1;
        d[512u + t] = v2;
        d[768u + t] = v3;
    }
}

}  // namespace

// workgroups per lane: one polynomial each per pass (eight lanes of 256 fill the chip several times over; a lane of fewer polynomials takes one each)
constexpr uint32_t kKeyBindBlocks = 256;
void launch_key_bind(const KeyBindParams& p, KeyForm form, hipStream_t s) {
    const uint32_t total = p.part[0].polys + p.part[1].polys + p.part[2].polys + p.part[3].polys;
    if (total == 0 || p.lanes.n == 0) return;
    const dim3 grid(total < kKeyBindBlocks ? total : kKeyBindBlocks, 1, p.lanes.n);
    if (form == KEYS_COMPACT)
        hipLaunchKernelGGL(key_bind_kernel<KEYS_COMPACT>, grid, dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL(key_bind_kernel<KEYS_FULL>, grid, dim3(256), 0, s, p);
}

}  // namespace spiral
