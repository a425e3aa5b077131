// Row 0 of a seeded message (include/spiral_gpu.h, spiral_gpu_query_seeded_bytes): the one definition both sides use.  The server's
// generator kernel (seed.hip) and the client's host function (spiral_gpu_seed_expand, server.cpp) include this header and nothing else
// defines the format.
//
// Slot z of row-0 polynomial k of a message with domain tag d: the ChaCha20 block (RFC 8439 section 2.3) with key = the 32-byte seed,
// nonce = LE32(d) || LE64(k) and block counter z >> 1; of its sixteen words w, half h = z & 1 gives
//     residue mod p = (w[8h] + w[8h+1] 2^32 + w[8h+2] 2^64 + w[8h+3] 2^96) mod p
//     residue mod b = (w[8h+4] + ... + w[8h+7] 2^96) mod b
// directly in NTT / CRT form (128 bits per residue: bias below 2^-100).  One block gives both residues of slots 2c and 2c + 1.
#pragma once
#include <stdint.h>

#include "common.h"

namespace spiral {

// domain tags: which message a seed expands row 0 of
enum SeedDomain : uint32_t { SEED_QUERY = 1, SEED_PUB_PARAMS = 2, SEED_PACK_QUERY = 3, SEED_PACK_PUB_PARAMS = 4 };
constexpr uint32_t kSeedBytes = 32;

struct Seed {  // the key words, LE32 of the seed bytes (a kernel argument)
    uint32_t w[8];
};

__host__ __device__ inline uint32_t chacha_rotl(uint32_t x, uint32_t n) { return (x << n) | (x >> (32u - n)); }  // (a constant n: v_alignbit_b32)

__host__ __device__ inline void chacha_qr(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
    a += b, d = chacha_rotl(d ^ a, 16);
    c += d, b = chacha_rotl(b ^ c, 12);
    a += b, d = chacha_rotl(d ^ a, 8);
    c += d, b = chacha_rotl(b ^ c, 7);
}

// the ChaCha20 block function (RFC 8439 section 2.3): out = the 16 state words after 20 rounds plus the input state
__host__ __device__ inline void chacha20_block(const uint32_t key[8], uint32_t counter, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t out[16]) {
    const uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3],
                             key[4],      key[5],      key[6],      key[7],      counter, n0,   n1,     n2};
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = in[i];
#pragma unroll
    for (int r = 0; r < 10; r++) {
        chacha_qr(x[0], x[4], x[8], x[12]);
        chacha_qr(x[1], x[5], x[9], x[13]);
        chacha_qr(x[2], x[6], x[10], x[14]);
        chacha_qr(x[3], x[7], x[11], x[15]);
        chacha_qr(x[0], x[5], x[10], x[15]);
        chacha_qr(x[1], x[6], x[11], x[12]);
        chacha_qr(x[2], x[7], x[8], x[13]);
        chacha_qr(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = x[i] + in[i];
}

// 2^(32 i) mod m
__host__ __device__ constexpr uint64_t pow2_32i_mod(uint32_t i, uint64_t m) { return i == 0 ? 1u % m : (pow2_32i_mod(i - 1, m) << 32) % m; }

// the 128-bit little-endian integer w[0..3] mod m as sum w_i (2^(32 i) mod m) < 4 * 2^32 * 2^28 = 2^62, then one exact u64 reduction
template <uint32_t M>
__host__ __device__ inline uint32_t mod128(const uint32_t* w) {
    constexpr uint64_t c1 = pow2_32i_mod(1, M), c2 = pow2_32i_mod(2, M), c3 = pow2_32i_mod(3, M);
    static_assert(c1 < (1u << 28) && c2 < (1u << 28) && c3 < (1u << 28), "a 128-bit residue sum must stay below 2^62");
    const uint64_t x = (uint64_t)w[0] + (uint64_t)w[1] * c1 + (uint64_t)w[2] * c2 + (uint64_t)w[3] * c3;
    return (uint32_t)(x % M);  // (= common.h mod_p / mod_b, exact for every u64)
}

// both residues of slots 2c and 2c + 1 of row-0 polynomial k: r[h] = p-residue | b-residue << 32 of slot 2c + h (a PK word)
__host__ __device__ inline void seed_slot_pair(const uint32_t key[8], uint32_t domain, uint64_t k, uint32_t c, uint64_t r[2]) {
    uint32_t w[16];
    chacha20_block(key, c, domain, (uint32_t)k, (uint32_t)(k >> 32), w);
#pragma unroll
    for (int h = 0; h < 2; h++) r[h] = (uint64_t)mod128<kP>(w + 8 * h) | ((uint64_t)mod128<kB>(w + 8 * h + 4) << 32);
}

#ifdef __HIPCC__
// The device's thread-to-word map of a row-0 polynomial (seed.hip seed_rows_kernel, keys.hip key_bind_kernel): thread i of a polynomial (0 .. 1023)
// computes one block -- slots 2c and 2c + 1 with c = (i mod 256) * 4 + i / 256, whose PK words pk_pos(2c), pk_pos(2c + 1) are 2i and 2i + 1 -- and
// writes them with one 16-byte store, so a wave's stores cover 1 KiB of consecutive bytes
template <class Where>  // where(): the polynomial's first word (evaluated after the block function)
__device__ __forceinline__ void seed_store_pair(const uint32_t key[8], uint32_t domain, uint64_t k, uint32_t i, Where where) {
    const uint32_t c = ((i & 255u) << 2) | (i >> 8);  // pk_pos(2c) = (c & 3) * 512 + (c >> 2) * 2 = 2i
    uint64_t r[2];
    seed_slot_pair(key, domain, k, c, r);
    *reinterpret_cast<ulonglong2*>(where() + 2u * i) = make_ulonglong2(r[0], r[1]);
}
#endif

__host__ __device__ inline Seed seed_words(const uint8_t* b) {
    Seed s;
    for (int i = 0; i < 8; i++) s.w[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
    return s;
}

}  // namespace spiral
