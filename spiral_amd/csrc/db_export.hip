// Items out of the database image as plaintexts (spiral_gpu_server_read_db_items, spiral_gpu_pack_server_read_db_items and their _at forms): the
// inverse of the ingest (ntt.hip LD_DBGEN / LD_DBGEN1 with the ST_DB / ST_DB1 stores; load_db, src/spiral.cpp:1116-1153, backwards).  One workgroup per
// polynomial: gather its 2048 words from the image in the form it is in, inverse transform, CRT lift, undo the centred lift, pack coeff_bits wide.
//
// A kernel of its own, not a store mode of ntt_inverse_kernel: the gather is 7 (packed) or 8 (limb planes) byte loads per word through the getters
// of common.h / kernels.h, whose address arithmetic does not belong in the budget of the transforms every query runs; nothing of ntt.hip changes.
//
// Block order of a range export.  In every form the bytes of a word share their 128-byte lines with the words of 8 adjacent image columns and of
// the 8 (base: terms 2 j + m) or 16 (SpiralPack: terms j) rows j of one aligned band -- a packed lane's 112-byte string, a limb plane's 16 terms
// per lane -- so each line is wanted by the polynomials of a GROUP of 8 rows x 4 items x 4 polynomials (16 rows x 8 items x 1 for SpiralPack), 128
// workgroups.  Items are j-major, so in item order those 128 are up to 8 num_per items apart.  The grid is therefore laid out in groups: jobs are
// numbered band by band, column group by column group, and each XCD takes a contiguous run of jobs (ntt_forward_kernel's job-to-XCD map), so that a
// group's workgroups are resident together on one XCD and its L2 serves the re-reads.  The grid covers whole bands; a workgroup whose item is outside
// the launch's range returns at once.
#include "db_plain_device.h"
#include "kernels.h"
#include "ntt_device.h"

namespace spiral {

namespace {

// (6 workgroups per CU: at the transforms' bound of 8 the gather's addresses spill 12 bytes per thread; at 6 every form compiles to 61 .. 74 VGPRs, no scratch)
template <uint32_t FORM, bool PACK>
__global__ __launch_bounds__(256, 6) void db_export_kernel(Tables t, DbExportParams p) {
    __shared__ uint64_t sh[kLdsWords];
    constexpr uint32_t polys = PACK ? 1u : 4u, R = PACK ? 16u : 8u;
    const uint32_t tid = threadIdx.x;
    uint32_t j, ii, mc, slot;
    uint64_t pos;
    if (p.table) {
        const uint32_t k = blockIdx.x / polys;
        const uint4 e = p.table[k];  // {j local, column ii, output slot, position in the call}
        mc = blockIdx.x - k * polys;
        j = e.x, ii = e.y, slot = e.z, pos = e.w;
    } else {
        const uint32_t gi = min(PACK ? 8u : 4u, p.num_per), gjobs = R * gi * polys, gpb = p.num_per / gi;  // items, jobs of a group; groups per band
        const uint32_t b = (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);  // (the grid is whole bands: a multiple of 8)
        const uint32_t grp = b / gjobs, w = b - grp * gjobs, wi = w / polys;
        mc = w - wi * polys;
        const uint32_t band = (uint32_t)(p.first / ((uint64_t)R * p.num_per)) + grp / gpb;
        j = band * R + wi / gi;
        ii = (grp % gpb) * gi + wi % gi;
        const uint64_t item = (uint64_t)j * p.num_per + ii;
        if (item < p.first || item - p.first >= p.n) return;
        slot = (uint32_t)(item - p.first);
        pos = p.pos_base + slot;
    }
    uint32_t lo[8], hi[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const uint64_t v = image_word<FORM, PACK>(p.db, pk_pos_tk(tid, r), j, ii, mc, p.num_per, p.dim0);  // z = pk_pos(slot 8 tid + r), as ST_DB
        lo[r] = lo32(v);
        hi[r] = hi32(v);
    }
    ntt_inverse_block<false>(lo, hi, sh, t.inv, tid);
    __syncthreads();  // the transform's last LDS reads
    uint32_t bad = kN;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        bool ok;
        sh[ix_a(tid, r)] = unlift_coeff(crt_compose_lazy(csub_min(lo[r], kP), hi[r]), p.p_db, ok);
        if (!ok) bad = min(bad, ix_a(tid, r));
    }
    if (bad < kN) atomicMin(p.err, (unsigned long long)((pos * polys + mc) * kN + bad));
    __syncthreads();
    // the polynomial's 256 * coeff_bits bytes, 16 at a time: bits [128 u, 128 u + 128) of the little-endian string of coeff_bits-wide coefficients
    const uint32_t w = p.coeff_bits, runs = 16u * w;
    pk_u64x2* dst = reinterpret_cast<pk_u64x2*>(p.out + ((size_t)slot * polys + mc) * (256u * w));
    for (uint32_t u = tid; u < runs; u += 256u) {
        uint64_t h[2];
#pragma unroll
        for (uint32_t k = 0; k < 2; k++) {
            const uint32_t bit = 128u * u + 64u * k;
            uint32_t c = bit / w, filled = w - (bit - c * w);
            uint64_t acc = sh[c] >> (w - filled);
            while (filled < 64u) {  // (2048 w bits are whole words: c + 1 < 2048 here)
                acc |= sh[++c] << filled;
                filled += w;
            }
            h[k] = acc;
        }
        dst[u] = pk_u64x2{h[0], h[1]};
    }
}

}  // namespace

void launch_db_export(const DeviceTables& t, const DbExportParams& p, hipStream_t s) {
    if (p.n == 0) return;
    const uint32_t polys = p.pack ? 1u : 4u;
    uint64_t blocks = (uint64_t)p.n * polys;
    if (!p.table) {  // whole bands of R rows
        const uint64_t band_items = (uint64_t)(p.pack ? 16u : 8u) * p.num_per;
        blocks = ((p.first + p.n + band_items - 1) / band_items - p.first / band_items) * band_items * polys;
    }
    if (blocks >= (1ull << 31)) abort();  // (the host's passes are far below)
    const Tables tb{t.fwd, t.inv};
    const dim3 grid((uint32_t)blocks), block(256);
    if (p.pack) {
        if (p.form == DBX_PACKED)
            hipLaunchKernelGGL((db_export_kernel<DBX_PACKED, true>), grid, block, 0, s, tb, p);
        else if (p.form == DBX_LIMBS)
            hipLaunchKernelGGL((db_export_kernel<DBX_LIMBS, true>), grid, block, 0, s, tb, p);
        else
            hipLaunchKernelGGL((db_export_kernel<DBX_LIMBS8, true>), grid, block, 0, s, tb, p);
    } else if (p.form == DBX_PACKED) {
        hipLaunchKernelGGL((db_export_kernel<DBX_PACKED, false>), grid, block, 0, s, tb, p);
    } else {
        hipLaunchKernelGGL((db_export_kernel<DBX_LIMBS, false>), grid, block, 0, s, tb, p);
    }
}

}  // namespace spiral
