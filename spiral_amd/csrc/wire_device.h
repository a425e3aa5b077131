// The decode of one polynomial of a client message in its wire form (include/spiral_gpu.h: 2048 raw coefficients, 56 bits each, little-endian,
// back to back), stated once: ntt.hip's LD_WIRE loader and query_ingest.hip both call it and nothing else reads the format on the device.
#pragma once
#include "kernels.h"
#include "ntt_device.h"

namespace spiral {

// The polynomial's 14 336 bytes at `poly` (16-byte aligned) come into the workgroup's LDS tile `sh` with 16-byte loads (896 per polynomial, coalesced),
// then each thread takes its eight 56-bit coefficients ix_a(tid, r) from there -- one or two LDS words each -- reduced mod p / mod b as LD_RAW does.
// A value above Q atomicMin's (~gen << 32 | first + its index in the polynomial) into the u64 at err: `first` is the message-wide index of the
// polynomial's first coefficient and `gen` the call's generation (a later call's entries compare below every earlier one's, so the word is never
// reset).  Returns with the tile free for the transform.
__device__ __forceinline__ void wire_decode8(const uint8_t* poly, uint64_t* sh, uint32_t tid, uint32_t* lo, uint32_t* hi, uint32_t* err, uint64_t gen,
                                             uint32_t first) {
    const uint4* src = reinterpret_cast<const uint4*>(poly);
    for (uint32_t i = tid; i < kWirePolyBytes / 16u; i += 256u) {
        const uint4 x = src[i];
        sh[2u * i] = pack(x.x, x.y);
        sh[2u * i + 1u] = pack(x.z, x.w);
    }
    __syncthreads();
    uint32_t bad = 0xffffffffu;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const uint32_t idx = ix_a(tid, r), bit = 56u * idx, w = bit >> 6, sft = bit & 63u;
        uint64_t v = sh[w] >> sft;
        if (sft > 8u) v |= sh[w + 1u] << (64u - sft);  // (the last coefficient, sft = 8, ends inside word 1791)
        v &= (1ull << 56) - 1ull;
        if (v > kQ) bad = min(bad, idx);
        lo[r] = mod_p(v);
        hi[r] = mod_b(v);
    }
    if (bad != 0xffffffffu) atomicMin(reinterpret_cast<unsigned long long*>(err), (~gen << 32) | (first + bad));
    __syncthreads();  // the transform reuses the LDS words
}

}  // namespace spiral
