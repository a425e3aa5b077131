// Tracked fingerprints (include/spiral_gpu.h "Fingerprints", Tracked): what keeps the resident table of polynomial sums g(i, q) and the combined
// value F current under the in-place updates, and what compares the table with a recomputation (kernels.h).  None of these reads the image: an update's
// new sums come from the plaintext coefficients the call already has on the device -- the staged raw item stream here, the spliced coefficients in
// records.hip's TRACK instantiations -- and F moves by (g_new - g_old) r^(2048 q) s^(i + 1), the definition being linear in every g.
//
// As in db_fingerprint.hip every value is a canonical residue, so the sums give the same bits in any order.
#include "common.h"
#include "fingerprint_math.h"
#include "kernels.h"

namespace spiral {

namespace {

// one workgroup per polynomial of the staged stream: thread t takes coefficients t, t + 256, ..
__global__ __launch_bounds__(256) void fingerprint_stream_kernel(FpStreamParams p) {
    __shared__ uint64_t sh[4];
    if (*p.err) return;  // a coefficient was not below p_db: table and F stay as they were
    const uint32_t tid = threadIdx.x;
    uint64_t acc = 0;  // 8 canonical terms, each below 2^61: the sum is below 2^64, reduced once
#pragma unroll
    for (uint32_t r = 0; r < 8; r++) {
        const uint32_t c = r * 256u + tid;
        const uint64_t x = packed_coeff(p.items, (uint64_t)blockIdx.x * kN + c, p.coeff_bits);  // < p_db < P (the host has checked every one)
        acc += fp_mul(x, p.weights[c]);                                                         // r^(c + 1)
    }
    const uint64_t sum = fp_block_sum(fp_reduce(acc), sh, tid);
    if (tid == 0) p.gnew[blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void fingerprint_apply_kernel(FpApplyParams p) {
    __shared__ uint64_t sh[4];
    if (*p.err) return;
    uint64_t acc = 0;
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < p.n; k += gridDim.x * 256u) {
        const ulonglong2 e = p.entries[k];
        if (e.x == kFpApplySkip) continue;
        const uint64_t word = e.y >> 8, g = p.gnew[k], old = p.table[word];
        p.table[word] = g;
        acc = fp_add(acc, fp_mul(fp_mul(fp_sub(g, old), p.weights[kFpW_Poly + (uint32_t)(e.y & 255u)]), fp_pow_s(p.weights + kFpW_S, e.x + 1)));
    }
    const uint64_t sum = fp_block_sum(acc, sh, threadIdx.x);
    if (threadIdx.x == 0) p.sums[blockIdx.x] = fp_add(p.sums[blockIdx.x], sum);
}

__global__ __launch_bounds__(256) void fingerprint_compare_kernel(FpCompareParams p) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x; w < p.n_words; w += (uint64_t)gridDim.x * 256u) {
        if (p.part[w] == p.table[w]) continue;
        const uint64_t k = w / p.npolys;
        atomicAdd(p.out, 1ull);
        atomicMin(p.out + 1, (unsigned long long)((p.idx0 + k * p.idx_stride) * kFpMaxPolys + p.poly0 + (uint32_t)(w - k * p.npolys)));
    }
}

}  // namespace

void launch_fingerprint_stream(const FpStreamParams& p, hipStream_t s) {
    if (p.n_polys) hipLaunchKernelGGL(fingerprint_stream_kernel, dim3(p.n_polys), dim3(256), 0, s, p);
}

void launch_fingerprint_apply(const FpApplyParams& p, hipStream_t s) {
    if (p.n == 0) return;
    const uint32_t blocks = std::min<uint32_t>(kFpSumWords, (p.n + 255u) / 256u);
    hipLaunchKernelGGL(fingerprint_apply_kernel, dim3(blocks), dim3(256), 0, s, p);
}

void launch_fingerprint_compare(const FpCompareParams& p, hipStream_t s) {
    if (p.n_words == 0) return;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(1024u, (p.n_words + 255u) / 256u);
    hipLaunchKernelGGL(fingerprint_compare_kernel, dim3(blocks), dim3(256), 0, s, p);
}

}  // namespace spiral
