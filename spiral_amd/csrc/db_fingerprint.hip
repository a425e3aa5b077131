// Content fingerprints of the database image (include/spiral_gpu.h "Fingerprints"; spiral_gpu_server_fingerprint_items, its _at form and the
// SpiralPack pair): the export's gather and inverse transform (db_export.hip) with a reduction modulo P = 2^61 - 1 in place of the byte-wide stores.
// One workgroup per polynomial, in the export's job order (range form) or from the export's sorted table (_at form): gather its 2048 words from the
// image in the form it is in, inverse transform, CRT lift, undo the centred lift, multiply coefficient c by r^(c + 1) and sum.  The polynomial's
// partial leaves as ONE 8-byte word; a second, small launch per pass weighs the partials of an item by r^(2048 q), the item by s^(i + 1), and
// accumulates the pass into a fixed handful of words that the host adds up.
//
// Every value is a canonical residue and modular addition is associative and commutative on those, so the sums below -- across a thread's 8
// coefficients, a wave, a workgroup's four waves, the grid-stride of the second launch, the passes -- give the same bits in any order.
//
// Like db_export_kernel this kernel keeps its own loop around image_word (db_plain_device.h records why), and no existing kernel changes.
#include "db_plain_device.h"
#include "fingerprint_math.h"
#include "kernels.h"
#include "ntt_device.h"

namespace spiral {

namespace {

// (launch bounds as db_export_kernel's: the same gather and transform; the weights take the place of the packing loop)
template <uint32_t FORM, bool PACK>
__global__ __launch_bounds__(256, 6) void db_fingerprint_kernel(Tables t, DbFingerprintParams p) {
    __shared__ uint64_t sh[kLdsWords];
    constexpr uint32_t polys = PACK ? 1u : 4u, R = PACK ? 16u : 8u;
    const uint32_t tid = threadIdx.x;
    uint32_t j, ii, mc, slot;
    uint64_t pos;
    if (p.table) {
        const uint32_t k = blockIdx.x / polys;
        const uint4 e = p.table[k];  // {j local, column ii, slot in the pass, position in the call}
        mc = blockIdx.x - k * polys;
        j = e.x, ii = e.y, slot = e.z, pos = e.w;
    } else {  // db_export.hip's block order: band by band, column group by column group, a contiguous run of jobs per XCD
        const uint32_t gi = min(PACK ? 8u : 4u, p.num_per), gjobs = R * gi * polys, gpb = p.num_per / gi;
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
    const uint32_t q = PACK ? blockIdx.y : mc;  // the polynomial among the npolys this server holds of an item (SpiralPack: its trial images, back to back)
    const uint64_t* db = p.db + (PACK ? (size_t)blockIdx.y * p.trial_words : (size_t)0);
    uint32_t lo[8], hi[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const uint64_t v = image_word<FORM, PACK>(db, pk_pos_tk(tid, r), j, ii, mc, p.num_per, p.dim0);  // z = pk_pos(slot 8 tid + r), as ST_DB
        lo[r] = lo32(v);
        hi[r] = hi32(v);
    }
    ntt_inverse_block<false>(lo, hi, sh, t.inv, tid);
    __syncthreads();  // the transform's last LDS reads
    uint32_t bad = kN;
    uint64_t acc = 0;  // 8 canonical terms, each below 2^61: the sum is below 2^64, reduced once
#pragma unroll
    for (int r = 0; r < 8; r++) {
        bool ok;
        const uint64_t x = unlift_coeff(crt_compose_lazy(csub_min(lo[r], kP), hi[r]), p.p_db, ok);  // < p_db < P
        if (!ok) bad = min(bad, ix_a(tid, r));
        acc += fp_mul(x, p.weights[ix_a(tid, r)]);  // r^(c + 1)
    }
    if (bad < kN) atomicMin(p.err, (unsigned long long)((pos * p.npolys + q) * kN + bad));
    const uint64_t sum = fp_block_sum(fp_reduce(acc), sh, tid);
    if (tid == 0) p.part[(size_t)slot * p.npolys + q] = sum;
}

// Item k of the pass: f = sum over q of part[k][q] r^(2048 (poly0 + q)), written to item_f[k * out_stride] (with out_stride - 1 zeros behind it: the
// items between two of a column shard's, which it does not hold); F's share f s^(i + 1), i the item's database index, summed per workgroup by a
// grid-stride loop and ADDED to sums[blockIdx.x], which the host zeroes before a call's first pass.
__global__ __launch_bounds__(256) void db_fingerprint_combine_kernel(DbFingerprintCombineParams p) {
    __shared__ uint64_t sh[4];
    const uint64_t* wq = p.weights + kFpW_Poly + p.poly0;
    uint64_t acc = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < p.n; k += (uint64_t)gridDim.x * 256u) {
        const uint64_t* part = p.part + k * p.npolys;
        uint64_t f = 0;
        for (uint32_t q = 0; q < p.npolys; q++) f = fp_add(f, fp_mul(part[q], wq[q]));
        if (p.item_f) {
            p.item_f[k * p.out_stride] = f;
            for (uint64_t u = 1; u < p.out_stride && k * p.out_stride + u < p.out_words; u++) p.item_f[k * p.out_stride + u] = 0;
        }
        const uint64_t i = p.ids ? p.ids[k] : p.idx0 + k * p.idx_stride;
        acc = fp_add(acc, fp_mul(f, fp_pow_s(p.weights + kFpW_S, i + 1)));
    }
    const uint64_t sum = fp_block_sum(acc, sh, threadIdx.x);
    if (threadIdx.x == 0) p.sums[blockIdx.x] = fp_add(p.sums[blockIdx.x], sum);
}

}  // namespace

void launch_db_fingerprint(const DeviceTables& t, const DbFingerprintParams& p, hipStream_t s) {
    if (p.n == 0 || p.npolys == 0) return;
    const uint32_t polys = p.pack ? 1u : 4u;
    uint64_t blocks = (uint64_t)p.n * polys;
    if (!p.table) {  // whole bands of R rows
        const uint64_t band_items = (uint64_t)(p.pack ? 16u : 8u) * p.num_per;
        blocks = ((p.first + p.n + band_items - 1) / band_items - p.first / band_items) * band_items * polys;
    }
    if (blocks >= (1ull << 31) || (p.pack ? p.npolys > kFpMaxPolys : p.npolys != 4u)) abort();  // (the host's passes are far below)
    const Tables tb{t.fwd, t.inv};
    const dim3 grid((uint32_t)blocks, p.pack ? p.npolys : 1u), block(256);
    if (p.pack) {
        if (p.form == DBX_PACKED)
            hipLaunchKernelGGL((db_fingerprint_kernel<DBX_PACKED, true>), grid, block, 0, s, tb, p);
        else if (p.form == DBX_LIMBS)
            hipLaunchKernelGGL((db_fingerprint_kernel<DBX_LIMBS, true>), grid, block, 0, s, tb, p);
        else
            hipLaunchKernelGGL((db_fingerprint_kernel<DBX_LIMBS8, true>), grid, block, 0, s, tb, p);
    } else if (p.form == DBX_PACKED) {
        hipLaunchKernelGGL((db_fingerprint_kernel<DBX_PACKED, false>), grid, block, 0, s, tb, p);
    } else {
        hipLaunchKernelGGL((db_fingerprint_kernel<DBX_LIMBS, false>), grid, block, 0, s, tb, p);
    }
}

void launch_db_fingerprint_combine(const DbFingerprintCombineParams& p, hipStream_t s) {
    if (p.n == 0) return;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(kFpSumWords, (p.n + 255u) / 256u);
    hipLaunchKernelGGL(db_fingerprint_combine_kernel, dim3(blocks), dim3(256), 0, s, p);
}

}  // namespace spiral
