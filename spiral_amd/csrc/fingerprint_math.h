// Arithmetic modulo P = 2^61 - 1 of the database fingerprints (include/spiral_gpu.h "Fingerprints"), stated once for the device kernels
// (db_fingerprint.hip, db_track.hip, the TRACK record kernels) and the host functions (spiral_gpu_fingerprint_host, _of_polys), so that they cannot drift.  Every argument and every result is
// canonical, in [0, P - 1], unless a comment says otherwise.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FP_HD __host__ __device__ __forceinline__
#else
#define FP_HD inline
#endif

namespace spiral {

constexpr uint64_t kFpP = (1ull << 61) - 1;

// v < 2^64 folded at bit 61: v = h 2^61 + l == h + l (mod P), h <= 7 and l <= P, so h + l <= P + 7 < 2 P and one conditional subtract reduces it
FP_HD uint64_t fp_reduce(uint64_t v) {
    const uint64_t s = (v >> 61) + (v & kFpP);
    return s >= kFpP ? s - kFpP : s;
}
FP_HD uint64_t fp_add(uint64_t a, uint64_t b) {
    const uint64_t s = a + b;  // < 2 P
    return s >= kFpP ? s - kFpP : s;
}
FP_HD uint64_t fp_sub(uint64_t a, uint64_t b) { return a >= b ? a - b : a + kFpP - b; }
// a b mod P: the 122-bit product is h 2^61 + l with h = product >> 61 <= (P - 1)^2 >> 61 < P - 1 and l <= P, so h + l < 2 P: folded at bit 61 with
// one conditional subtract
FP_HD uint64_t fp_mul(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t hi = __umul64hi(a, b), lo = a * b;
#else
    const unsigned __int128 pr = (unsigned __int128)a * b;
    const uint64_t hi = (uint64_t)(pr >> 64), lo = (uint64_t)pr;
#endif
    const uint64_t s = ((hi << 3) | (lo >> 61)) + (lo & kFpP);
    return s >= kFpP ? s - kFpP : s;
}
FP_HD uint64_t fp_pow(uint64_t b, uint64_t e) {
    uint64_t r = 1;
    for (; e; e >>= 1, b = fp_mul(b, b))
        if (e & 1u) r = fp_mul(r, b);
    return r;
}
// a key word as a base: 2 + k mod (P - 3), in [2, P - 2]
FP_HD uint64_t fp_key_base(uint64_t k) { return 2 + k % (kFpP - 3); }

// The per-call weight table both sides build from a key: [0, 2048) r^(c + 1); [2048, 2048 + 256) r^(2048 q), q = 0 .. 255 (kMaxPackTrials);
// [2304, 2304 + 64) s^(2^k) -- s^(i + 1) is the product of the entries of the set bits of i + 1
constexpr uint32_t kFpCoeffs = 2048, kFpMaxPolys = 256, kFpW_Poly = kFpCoeffs, kFpW_S = kFpW_Poly + kFpMaxPolys, kFpWeightWords = kFpW_S + 64;
inline void fp_build_weights(const uint64_t key[2], uint64_t* w) {
    const uint64_t r = fp_key_base(key[0]), s = fp_key_base(key[1]);
    w[0] = r;
    for (uint32_t c = 1; c < kFpCoeffs; c++) w[c] = fp_mul(w[c - 1], r);
    w[kFpW_Poly] = 1;
    for (uint32_t q = 1; q < kFpMaxPolys; q++) w[kFpW_Poly + q] = fp_mul(w[kFpW_Poly + q - 1], w[kFpCoeffs - 1]);  // w[2047] = r^2048
    w[kFpW_S] = s;
    for (uint32_t k = 1; k < 64; k++) w[kFpW_S + k] = fp_mul(w[kFpW_S + k - 1], w[kFpW_S + k - 1]);
}
// s^e from the table of s^(2^k), e >= 1
FP_HD uint64_t fp_pow_s(const uint64_t* sq, uint64_t e) {
    uint64_t r = 1;
    for (uint32_t k = 0; e; e >>= 1, k++)
        if (e & 1u) r = fp_mul(r, sq[k]);
    return r;
}

#if defined(__HIPCC__)
// the sum of `v` over the workgroup's 256 threads, valid in thread 0; sh: 4 words of LDS nobody reads any more
__device__ __forceinline__ uint64_t fp_block_sum(uint64_t v, uint64_t* sh, uint32_t tid) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fp_add(v, (uint64_t)__shfl_xor((unsigned long long)v, off));  // across the wave of 64
    if ((tid & 63u) == 0) sh[tid >> 6] = v;
    __syncthreads();
    return fp_add(fp_add(sh[0], sh[1]), fp_add(sh[2], sh[3]));  // across the four waves
}
#endif

}  // namespace spiral
