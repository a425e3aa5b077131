// In-place update of a few database items (spiral_gpu_server_update_db_items, spiral_gpu_pack_server_update_db_items): the items' words, encoded by
// the ingest transform (ntt.hip LD_DBGEN / LD_DBGEN1 with a linear ST_PK store), are scattered into the image in the form it is in now.
//
// Packed form (common.h db_put_word, kernels.h db1_put_word; the plain layouts of tiny geometries too): every word owns its 7 (or 8) bytes, so one
// thread per word writes them and threads never meet.
// Limb planes (sweep_mfma.hip): the three signed limb bytes of a term sit in planes of their own, but the nibble byte of (column, term t) of a
// 128-term piece holds the top limbs of terms t and t + 64 (low and high nibble).  With the base path's terms k = 2 j + m that is item j and item
// j ^ 32 of the same column; with SpiralPack's terms k = j, item j and j ^ 64.  The host groups the updated items into such partner pairs and one
// thread writes both halves of each nibble byte it owns (keeping the old half when only one of the two items changes): no atomics, and no byte
// is touched by two threads.  A SpiralPack image of 8 columns (the pair form) has 512-byte planes of 32 half-lanes (term block, column): half-lane
// tb 8 + column, 3584-byte pieces, one column block per slot; the partners are the same.
#include "common.h"
#include "kernels.h"

namespace spiral {

namespace {

constexpr uint32_t kLimbBias = 0x808080u;  // (sweep_mfma.hip)

// residue a mod m in limb form: the three limb bytes go to chunk c of the planes (`plane` bytes each) at `b`, the 4-bit top limb is returned
__device__ __forceinline__ uint32_t put_limbs(uint8_t* b, uint32_t c, uint32_t a, uint32_t m, uint32_t plane) {
    const uint32_t w = (a >= (1u << 28) - kLimbBias ? a - m : a) + kLimbBias, x = w ^ kLimbBias;
#pragma unroll
    for (uint32_t i = 0; i < 3; i++) b[(2u * i + c) * plane] = (uint8_t)(x >> (8u * i));
    return w >> 24;
}

// block = (work entry, polynomial mc, 256 slots): entries [0, n_put) write the packed form, [n_put, n_put + n_pairs) the limb planes
__global__ __launch_bounds__(256) void db_update_kernel(DbUpdateParams p) {
    if (*p.err) return;  // a coefficient was not below p_db: the image stays as it was
    const uint32_t polys = p.pack ? 1u : 4u, z = (blockIdx.x & 7u) * 256u + threadIdx.x, q = blockIdx.x >> 3;
    const uint32_t w = q / polys, mc = q - w * polys, m = mc >> 1, c = mc & 1u;
    if (w < p.n_put) {
        const uint4 e = p.put[w];  // {encoded item, j local to the image, column ii, -}
        const uint64_t v = p.enc[((size_t)e.x * polys + mc) * kN + z];
        if (p.pack)
            db1_put_word(p.packed, z, e.y, e.z, p.num_per, p.dim0, v);
        else
            db_put_word(p.packed, z, e.y, e.z * 2u + c, m, 2u * p.num_per, p.dim0, v);
        return;
    }
    if (w - p.n_put >= p.n_pairs) return;
    const uint4 e = p.pairs[w - p.n_put];  // {column ii, j of the low partner, its encoded item, the high partner's} (kDbUpdateNone: unchanged)
    const uint32_t nic = p.pack ? p.num_per : 2u * p.num_per, col = p.pack ? e.x : e.x * 2u + c;
    const uint32_t kt = p.pack ? e.y : 2u * e.y + m, nk2 = (p.pack ? p.dim0 : 2u * p.dim0) >> 7, t = kt & 127u;  // t < 64: the high partner is t + 64
    const bool has_lo = e.z != kDbUpdateNone, has_hi = e.w != kDbUpdateNone;
    const uint64_t v_lo = has_lo ? p.enc[((size_t)e.z * polys + mc) * kN + z] : 0, v_hi = has_hi ? p.enc[((size_t)e.w * polys + mc) * kN + z] : 0;
    const bool c8 = p.pack && p.num_per == 8u;
    const uint32_t plane = c8 ? 512u : 1024u, nblk = c8 ? 1u : nic >> 4, lane = c8 ? ((t >> 4) & 3u) * 8u + col : ((t >> 4) & 3u) * 16u + (col & 15u);
#pragma unroll
    for (uint32_t pr = 0; pr < 2; pr++) {
        const size_t piece = (((size_t)z * nblk + (col >> 4)) * 2u + pr) * nk2 + (kt >> 7);  // 7 planes each
        uint8_t* b = reinterpret_cast<uint8_t*>(p.limbs) + piece * (7u * plane) + (size_t)lane * 16u + (t & 15u);
        const uint32_t mod = pr ? kB : kP;
        uint32_t nib = b[6u * plane];
        if (has_lo) nib = (nib & 0xF0u) | put_limbs(b, 0, pr ? hi32(v_lo) : lo32(v_lo), mod, plane);
        if (has_hi) nib = (nib & 0x0Fu) | (put_limbs(b, 1, pr ? hi32(v_hi) : lo32(v_hi), mod, plane) << 4);
        b[6u * plane] = (uint8_t)nib;
    }
}

// The trial images of a SpiralPack server in one launch (kernels.h DbUpdateTrialsParams): block = (work entry, 256 slots), an encoded item is one
// polynomial and its entry names the trial image it goes to.  A kernel and a body of its own: sharing the nibble loop with db_update_kernel through a
// function changed that kernel's scalar registers (48 -> 44), and no existing kernel changes with this one.
__global__ __launch_bounds__(256) void db_update_trials_kernel(DbUpdateTrialsParams q) {
    const DbUpdateParams& p = q.u;
    if (*p.err) return;
    const uint32_t z = (blockIdx.x & 7u) * 256u + threadIdx.x, w = blockIdx.x >> 3;
    if (w < p.n_put) {
        const uint4 e = p.put[w];  // {encoded polynomial, j, column ii, trial}
        db1_put_word(p.packed + (size_t)e.w * q.trial_words, z, e.y, e.z, p.num_per, p.dim0, p.enc[(size_t)e.x * kN + z]);
        return;
    }
    if (w - p.n_put >= p.n_pairs) return;
    const uint4 e = p.pairs[w - p.n_put];  // {column ii | trial << 24, j of the low partner, its encoded polynomial, the high partner's}
    const uint32_t col = e.x & kPackRecordColMask, kt = e.y, t = kt & 127u;
    const bool has_lo = e.z != kDbUpdateNone, has_hi = e.w != kDbUpdateNone;
    const uint64_t v_lo = has_lo ? p.enc[(size_t)e.z * kN + z] : 0, v_hi = has_hi ? p.enc[(size_t)e.w * kN + z] : 0;
    const bool c8 = p.num_per == 8u;
    const uint32_t plane = c8 ? 512u : 1024u, nblk = c8 ? 1u : p.num_per >> 4, lane = c8 ? ((t >> 4) & 3u) * 8u + col : ((t >> 4) & 3u) * 16u + (col & 15u);
    uint64_t* limbs = p.limbs + (size_t)(e.x >> kPackRecordTrialShift) * q.trial_words;
#pragma unroll
    for (uint32_t pr = 0; pr < 2; pr++) {
        const size_t piece = (((size_t)z * nblk + (col >> 4)) * 2u + pr) * (p.dim0 >> 7) + (kt >> 7);  // 7 planes each
        uint8_t* b = reinterpret_cast<uint8_t*>(limbs) + piece * (7u * plane) + (size_t)lane * 16u + (t & 15u);
        const uint32_t mod = pr ? kB : kP;
        uint32_t nib = b[6u * plane];
        if (has_lo) nib = (nib & 0xF0u) | put_limbs(b, 0, pr ? hi32(v_lo) : lo32(v_lo), mod, plane);
        if (has_hi) nib = (nib & 0x0Fu) | (put_limbs(b, 1, pr ? hi32(v_hi) : lo32(v_hi), mod, plane) << 4);
        b[6u * plane] = (uint8_t)nib;
    }
}

}  // namespace

void launch_db_update(const DbUpdateParams& p, hipStream_t s) {
    const uint64_t blocks = ((uint64_t)p.n_put + p.n_pairs) * (p.pack ? 1u : 4u) * (kN / 256u);
    if (blocks) hipLaunchKernelGGL(db_update_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, p);
}

void launch_db_update_trials(const DbUpdateTrialsParams& p, hipStream_t s) {
    const uint64_t blocks = ((uint64_t)p.u.n_put + p.u.n_pairs) * (kN / 256u);
    if (blocks) hipLaunchKernelGGL(db_update_trials_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, p);
}

}  // namespace spiral
