// The randomness of a client session (include/spiral_gpu.h, spiral_gpu_client_*): the one definition the session's kernels (client.hip), its host
// code (client_session.cpp) and the header's documentation use.  Nothing else defines the format.
//
// A session is created from a 32-byte client seed K.  Everything it draws is a function of K and counters, through chacha20_block (seed_device.h,
// RFC 8439 section 2.3); the domain tags below start at 16, clear of SeedDomain.
//
// Noise table.  C_i = sum_{j = -64}^{-64 + i} exp(-pi j^2 / 6.4^2) -- the discrete Gaussian of width 6.4 over [-64, 64] of the command line's
// client (cli/client.cpp, src/core.cpp:182-207).  T[0 .. 127] are 64-bit thresholds, T[i] = floor(2^64 C_i / C_128) (a quotient that rounds to 1
// gives 2^64 - 1), computed once on the host (client_noise_table: plain host code).  A 64-bit draw u gives the sample
//     v = -64 + #{ i : T[i] <= u },   v in [-64, 64];
// its residues are v mod p and v mod b, its raw value v mod Q.
//
// Noise polynomial i under a 32-byte noise key N and domain tag d: coefficient z takes u = w[2 (z & 7)] + w[2 (z & 7) + 1] 2^32 of the block with
// key N, nonce LE32(d) || LE64(i) and block counter z >> 3: one block gives eight consecutive coefficients.
//
// Secret key: noise key K itself under CLIENT_SECRET; polynomial 0 is sr, polynomials 1.. are the rows of Sp (2 rows for base Spiral, out_n for
// SpiralPack).  nonoise: every sample is 0, the secret included (the command line's --nonoise).
//
// The tags of a session's messages are fixed here as well, so that no later use can collide with them: message n (the public parameters are message
// 0, queries 1, 2, ...) has the public row-0 seed = the first 32 bytes of the block with key K, nonce LE32(CLIENT_MSG_SEED) || LE64(n), counter 0,
// and the secret noise key N_n = the first 32 bytes of the block with nonce LE32(CLIENT_NOISE_KEY) || LE64(n); its noise polynomials are drawn
// under N_n with CLIENT_NOISE.  The noise key is a derivation of its own under K: it is never derivable from the public seed.
#pragma once
#include <stdint.h>

#include <cmath>

#include "seed_device.h"

namespace spiral {

enum ClientDomain : uint32_t { CLIENT_SECRET = 16, CLIENT_MSG_SEED = 17, CLIENT_NOISE_KEY = 18, CLIENT_NOISE = 19 };
constexpr int32_t kNoiseBound = 64;       // samples lie in [-kNoiseBound, kNoiseBound]
constexpr uint32_t kNoiseThresholds = 128;

// T[i] = floor(2^64 C_i / C_128) in extended precision (a host function: no kernel calls it)
inline void client_noise_table(uint64_t out[kNoiseThresholds]) {
    long double c[kNoiseThresholds + 1], acc = 0;
    for (int i = 0; i <= (int)kNoiseThresholds; i++) {
        const long double j = (long double)(i - kNoiseBound);
        acc += std::exp(-3.14159265358979323846264338327950288L * j * j / (6.4L * 6.4L));
        c[i] = acc;
    }
    for (uint32_t i = 0; i < kNoiseThresholds; i++) {
        const long double t = std::floor(std::ldexp(c[i] / c[kNoiseThresholds], 64));
        out[i] = t >= 18446744073709551616.0L ? ~0ull : (uint64_t)t;
    }
}

// v = -64 + #{ i : T[i] <= u } by bisection of the non-decreasing table
__host__ __device__ inline int32_t noise_sample(const uint64_t* T, uint64_t u) {
    uint32_t n = 0;  // min(count, 127) after the loop
#pragma unroll
    for (uint32_t step = kNoiseThresholds / 2; step; step >>= 1) n += T[n + step - 1] <= u ? step : 0u;
    n += T[n] <= u ? 1u : 0u;
    return (int32_t)n - kNoiseBound;
}

// the eight 64-bit draws of block c of noise polynomial i: coefficients 8c .. 8c + 7
__host__ __device__ inline void noise_draws(const uint32_t key[8], uint32_t domain, uint64_t i, uint32_t c, uint64_t u[8]) {
    uint32_t w[16];
    chacha20_block(key, c, domain, (uint32_t)i, (uint32_t)(i >> 32), w);
#pragma unroll
    for (int h = 0; h < 8; h++) u[h] = (uint64_t)w[2 * h] | ((uint64_t)w[2 * h + 1] << 32);
}

// the raw value v mod Q of a sample
__host__ __device__ inline uint64_t noise_raw(int32_t v) { return v < 0 ? kQ - (uint64_t)(-v) : (uint64_t)v; }

}  // namespace spiral
