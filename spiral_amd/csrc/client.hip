// The kernels of a client session (include/spiral_gpu.h spiral_gpu_client_*; the format of its randomness: client_device.h).
//
// client_noise_kernel: one workgroup per noise polynomial, one ChaCha20 block -- eight coefficients -- per thread; the 128 thresholds sit in LDS and
// every draw is placed by a 7-step bisection.  The polynomials of all messages of a call come from one launch, each message under its own noise key.
//
// client_sample_kernel: the table-driven sample launch of a message (kernels.h ClientColumn).  A thread computes one ChaCha20 block of the column's
// row 0 -- the two PK words seed_store_pair writes -- takes a = -row 0 and forms b_r = a S_r + e_r + c M for every secret row pointwise: S and M are
// polynomials of the session's secret table, e the transformed noise, c a constant's two residues.  Pointwise work is oblivious to the PK order,
// and row 0 lands where the server's own generator puts it.
//
// client_decode_kernel: check_final's client half.  One workgroup per output polynomial (response, r, col).  The centred secret row Sp_r sits in LDS as
// 8-bit values, the response's row-0 polynomial a of column col as 32-bit values in its negacyclic extension ext[m + N] = a[m] (m >= 0), -a[m + N]
// (m < 0), so that (Sp_r * a)[k] = sum_i s[i] ext[k - i + N] with no sign test.  The product is a direct convolution in 64-bit integers, exact since
// |sum| <= 2048 * 64 * 2^31 < 2^48; one reduction mod q' and check_final's rounding with the row 1 + r value finish a coefficient.  Thread t owns the
// outputs k = t + 256 j, j < 8.  With i = 256 b + r the index k - i = (t - r) + 256 (j - b): for one r the fifteen values ext[t - r + 256 d + N],
// d = -7 .. 7, and the eight s[256 b + r] feed all 64 products of the thread, so the loop reads 23 LDS words per 64 multiply-adds; a wave's lanes
// read consecutive words (no bank conflict), the s reads broadcast.  The WIRE form is unpacked by the same launch: a value is the bit field of its
// position in the stream (primitives.cpp spiral_gpu_response_from_wire).
//
// client_response_noise_kernel: the error e of every coefficient of a response and its record per output polynomial (include/spiral_gpu.h,
// spiral_gpu_client_response_noise).  The decode's workgroup, operands, convolution and rounding as shared device functions; the unswitched form
// runs the convolution once per 28-bit prime; the record is reduced by wave shuffles and across the four waves through LDS.
#include "client_device.h"
#include "common.h"
#include "kernels.h"
#include "ntt_device.h"

namespace spiral {

namespace {

constexpr uint32_t kClientTpb = 256;

__global__ __launch_bounds__(kClientTpb) void client_noise_kernel(const uint32_t* keys, uint32_t domain, uint64_t first, const uint64_t* table, uint64_t* raw,
                                                                  int8_t* centred, const uint64_t* addend, uint32_t per_msg, uint32_t nonoise) {
    __shared__ uint64_t T[kNoiseThresholds];
    const uint32_t t = threadIdx.x, j = blockIdx.x, b = blockIdx.y;
    if (t < kNoiseThresholds) T[t] = table[t];
    __syncthreads();
    uint32_t key[8];
#pragma unroll
    for (int i = 0; i < 8; i++) key[i] = keys[8u * b + i];
    uint64_t u[8];
    noise_draws(key, domain, first + j, t, u);
    const size_t at = ((size_t)b * per_msg + j) * kN + 8u * t;
#pragma unroll
    for (int h = 0; h < 8; h++) {
        const int32_t v = nonoise ? 0 : noise_sample(T, u[h]);
        uint64_t x = noise_raw(v);
        if (addend) {
            x += addend[at + h] % kQ;
            x -= x >= kQ ? kQ : 0;
        }
        raw[at + h] = x;
        if (centred) centred[at + h] = (int8_t)v;
    }
}

// (x y + z) mod m on one residue: x, y, z < m < 2^28
__device__ __forceinline__ uint32_t mad_mod(uint32_t x, uint32_t y, uint32_t z, uint32_t m) { return (uint32_t)(((uint64_t)x * y + z) % m); }

__global__ __launch_bounds__(kClientTpb) void client_sample_kernel(ClientSampleParams p) {
    const uint32_t i = blockIdx.x * kClientTpb + threadIdx.x, b = blockIdx.z;
    const ClientColumn col = p.columns[(size_t)b * p.n_cols + blockIdx.y];
    uint32_t key[8];
#pragma unroll
    for (int w = 0; w < 8; w++) key[w] = p.seeds[8u * b + w];
    uint64_t* out = p.out + (size_t)b * p.msg_polys * kN;
    const uint64_t* noise = p.noise + (size_t)b * p.noise_polys * kN;
    const uint32_t c = ((i & 255u) << 2) | (i >> 8);  // the slot pair of thread i: seed_store_pair's map
    uint64_t r0[2];
    seed_slot_pair(key, p.domain, col.k, c, r0);
    *reinterpret_cast<ulonglong2*>(out + (size_t)col.dst * kN + 2u * i) = make_ulonglong2(r0[0], r0[1]);
    for (uint32_t r = 1; r < col.rows; r++) {
        const uint64_t* S = p.table + (size_t)(col.s_first + r - 1u) * kN + 2u * i;
        const uint64_t* e = noise + (size_t)(col.noise + (r - 1u) * col.noise_stride) * kN + 2u * i;
        const bool with_m = col.m_row == 0u || col.m_row == r;
        const uint64_t* M = p.table + (size_t)(col.m_idx + (r - 1u) * col.m_stride) * kN + 2u * i;
        uint64_t res[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t ap = csub(kP - lo32(r0[h]), kP), ab = csub(kB - hi32(r0[h]), kB);  // a = -row 0
            uint32_t xp = mad_mod(ap, lo32(S[h]), lo32(e[h]), kP), xb = mad_mod(ab, hi32(S[h]), hi32(e[h]), kB);
            if (with_m) {
                xp = mad_mod(col.c_p, lo32(M[h]), xp, kP);
                xb = mad_mod(col.c_b, hi32(M[h]), xb, kB);
            }
            res[h] = pack(xp, xb);
        }
        *reinterpret_cast<ulonglong2*>(out + (size_t)(col.dst + r * col.dst_stride) * kN + 2u * i) = make_ulonglong2(res[0], res[1]);
    }
}

__global__ __launch_bounds__(kClientTpb) void client_mul_kernel(const uint64_t* a, const uint64_t* b, uint64_t* out) {
    const size_t i = (size_t)blockIdx.x * kClientTpb + threadIdx.x;
    out[i] = pack(mod_p((uint64_t)lo32(a[i]) * lo32(b[i])), mod_b((uint64_t)hi32(a[i]) * hi32(b[i])));
}

// eight coefficients -> 56 bytes = seven words per thread
__global__ __launch_bounds__(kClientTpb) void client_wire_encode_kernel(const uint64_t* raw, uint64_t* wire) {
    const size_t g = (size_t)blockIdx.x * kClientTpb + threadIdx.x;
    uint64_t v[8];
#pragma unroll
    for (int h = 0; h < 8; h++) v[h] = raw[8u * g + h];
#pragma unroll
    for (int w = 0; w < 7; w++) wire[7u * g + w] = (v[w] >> (8 * w)) | (v[w + 1] << (56 - 8 * w));
}

// ---- what the decode and the noise measurement share: a response's values, the LDS operands, the convolution, check_final's rounding --------------
// the response's value (row, col, z) of response b: a word of the RAW form, or the bit field of its position in the WIRE stream
__device__ __forceinline__ uint64_t response_value(const ClientDecodeParams& p, uint32_t b, uint32_t col, uint32_t row, uint32_t z) {
    if (!p.wire) return p.resp[(((size_t)b * (p.rows + 1u) + row) * p.cols + col) * kN + z];
    const uint64_t* w = p.resp + (size_t)b * p.wire_words;
    const uint32_t width = row == 0 ? p.w0 : p.w1;
    const uint64_t idx = row == 0 ? (uint64_t)col * kN + z : ((uint64_t)(row - 1u) * p.cols + col) * kN + z;
    const uint64_t bit = (row == 0 ? 0ull : (uint64_t)p.cols * kN * p.w0) + idx * width;
    const uint32_t sh = (uint32_t)(bit & 63u);
    uint64_t v = w[bit >> 6] >> sh;
    if (sh + width > 64u) v |= w[(bit >> 6) + 1u] << (64u - sh);
    return v & ((1ull << width) - 1ull);
}

// acc[j] = (Sp_r * a)[t + 256 j] from the negacyclic extension of a in ext and the secret row in s8 (the loop of the header comment)
__device__ __forceinline__ void secret_row_convolve(const int32_t* ext, const int8_t* s8, uint32_t t, int64_t (&acc)[8]) {
    for (uint32_t rr = 0; rr < 256u; rr++) {
        int32_t e[15], sv[8];
#pragma unroll
        for (int d = 0; d < 15; d++) e[d] = ext[(int32_t)(kN + t) - (int32_t)rr + 256 * (d - 7)];  // index in [1, 4095]
#pragma unroll
        for (int bb = 0; bb < 8; bb++) sv[bb] = s8[256u * bb + rr];
#pragma unroll
        for (int j = 0; j < 8; j++)
#pragma unroll
            for (int bb = 0; bb < 8; bb++) acc[j] += (int64_t)sv[bb] * (int64_t)e[j - bb + 7];
    }
}

// check_final's x = vf 4p + vr q' of one coefficient -- vf the product mod q', centred, vr the row 1 + r value mod 4p, centred -- and its quotient by
// D = 4 q' rounded half away from zero, before the reduction mod p
__device__ __forceinline__ int64_t switched_round(int64_t acc, uint64_t row_value, int64_t qp, int64_t q1, int64_t& x) {
    int64_t vf = acc % qp;
    vf += vf < 0 ? qp : 0;
    vf -= vf >= qp / 2 ? qp : 0;  // to_ntt_qprime's product, centred
    int64_t vr = (int64_t)(row_value % (uint64_t)q1);
    vr -= vr >= q1 / 2 ? q1 : 0;
    const int64_t denom = qp * 4;
    x = vf * q1 + vr * qp;
    return (x + (x >= 0 ? denom / 2 : -(denom / 2))) / denom;  // round half away from zero, truncating division
}

__global__ __launch_bounds__(kClientTpb) void client_decode_kernel(ClientDecodeParams p) {
    __shared__ int32_t ext[2 * kN];
    __shared__ int8_t s8[kN];
    const uint32_t col = blockIdx.x, r = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
    for (uint32_t z = t; z < kN; z += kClientTpb) {
        const int32_t a = (int32_t)(response_value(p, b, col, 0, z) % p.qprime);
        ext[kN + z] = a;
        ext[z] = -a;
        s8[z] = p.sp[(size_t)r * kN + z];
    }
    __syncthreads();
    int64_t acc[8] = {};
    secret_row_convolve(ext, s8, t, acc);
    const int64_t qp = (int64_t)p.qprime, q1 = (int64_t)(4u * p.p_db), pdb = (int64_t)p.p_db;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t k = t + 256u * j;
        int64_t x;
        int64_t res = switched_round(acc[j], response_value(p, b, col, 1u + r, k), qp, q1, x);
        res %= pdb;
        res += res < 0 ? pdb : 0;
        p.out[(((size_t)b * p.rows + r) * p.cols + col) * kN + k] = (uint64_t)res;
    }
}

// The decode of the output polynomials that records touch (kernels.h ClientRecordDecodeParams): client_decode_kernel's operands, convolution and
// rounding through the shared functions; the 2048 values then meet in LDS and the waves store the records' byte ranges of their w-bit string -- a
// 256-byte record of an 8 KiB plaintext is one convolution and 256 bytes out, not four and 64 KiB of words.
__global__ __launch_bounds__(kClientTpb) void client_decode_records_kernel(ClientRecordDecodeParams q) {
    __shared__ int32_t ext[2 * kN];
    __shared__ int8_t s8[kN];
    __shared__ uint64_t vals[kN];
    const ClientDecodeParams& p = q.d;
    const uint4 e = q.entries[blockIdx.x];
    const uint32_t b = e.x, r = e.y & 0xFFu, col = e.y >> 8, t = threadIdx.x, w = q.w;
    for (uint32_t z = t; z < kN; z += kClientTpb) {
        const int32_t a = (int32_t)(response_value(p, b, col, 0, z) % p.qprime);
        ext[kN + z] = a;
        ext[z] = -a;
        s8[z] = p.sp[(size_t)r * kN + z];
    }
    __syncthreads();
    int64_t acc[8] = {};
    secret_row_convolve(ext, s8, t, acc);
    const int64_t qp = (int64_t)p.qprime, q1 = (int64_t)(4u * p.p_db), pdb = (int64_t)p.p_db;
    const uint64_t mask = (1ull << w) - 1ull;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t k = t + 256u * j;
        int64_t x;
        int64_t res = switched_round(acc[j], response_value(p, b, col, 1u + r, k), qp, q1, x);
        res %= pdb;
        res += res < 0 ? pdb : 0;
        vals[k] = (uint64_t)res & mask;
    }
    __syncthreads();
    const uint32_t lane = t & 63u, wave = t >> 6;
    for (uint32_t s = wave; s < e.w; s += kClientTpb / 64u) {
        const uint4 seg = q.segs[e.z + s];
        uint8_t* dst = q.buf + (((uint64_t)seg.w << 32) | seg.z);
        for (uint32_t i = lane; i < seg.y; i += 64u) {  // byte i of the segment: bits [8 (seg.x + i), + 8) of the string of w-bit values
            const uint32_t bit = 8u * (seg.x + i);
            uint32_t c = bit / w, filled = w - (bit - c * w);
            uint64_t v = vals[c] >> (w - filled);
            while (filled < 8u) {  // (the segment ends inside the polynomial's 2048 w bits: c + 1 < 2048 here)
                v |= vals[++c] << filled;
                filled += w;
            }
            dst[i] = (uint8_t)v;
        }
    }
}

// ---- keyed records: the client's find (include/spiral_gpu.h "Keyed records"; kernels.h ClientKvFindParams) ---------------------------------------
// output polynomial (r, col) of response b into vals, masked to w bits: client_decode_records_kernel's steps through the shared functions.  Opens with
// a barrier (the tiles' previous readers are done) and closes with one (vals is complete).
__device__ __forceinline__ void kv_decode_poly(const ClientDecodeParams& p, uint32_t b, uint32_t r, uint32_t col, uint32_t w, int32_t* ext, int8_t* s8, uint64_t* vals,
                                               uint32_t t) {
    __syncthreads();
    for (uint32_t z = t; z < kN; z += kClientTpb) {
        const int32_t a = (int32_t)(response_value(p, b, col, 0, z) % p.qprime);
        ext[kN + z] = a;
        ext[z] = -a;
        s8[z] = p.sp[(size_t)r * kN + z];
    }
    __syncthreads();
    int64_t acc[8] = {};
    secret_row_convolve(ext, s8, t, acc);
    const int64_t qp = (int64_t)p.qprime, q1 = (int64_t)(4u * p.p_db), pdb = (int64_t)p.p_db;
    const uint64_t mask = (1ull << w) - 1ull;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t k = t + 256u * j;
        int64_t x;
        int64_t res = switched_round(acc[j], response_value(p, b, col, 1u + r, k), qp, q1, x);
        res %= pdb;
        res += res < 0 ? pdb : 0;
        vals[k] = (uint64_t)res & mask;
    }
    __syncthreads();
}

// Workgroup b = 2 k + candidate.  Polynomial 0 holds the header (the layout refuses one that does not), and the found slot's value bytes may start in it:
// the polynomials the value touches are taken in ascending order, so polynomial 0's tile is read before a later polynomial reuses it.
__global__ __launch_bounds__(kClientTpb) void client_kv_find_kernel(ClientKvFindParams q) {
    __shared__ int32_t ext[2 * kN];
    __shared__ int8_t s8[kN];
    __shared__ uint64_t vals[kN];
    __shared__ uint32_t hit_slot, arrived;
    const ClientDecodeParams& p = q.d;
    const uint32_t b = blockIdx.x, key = b >> 1, t = threadIdx.x, w = q.w, V = q.value_bytes, poly_bytes = 256u * w;
    if (t == 0) hit_slot = 0xFFFFFFFFu;
    kv_decode_poly(p, b, 0u, 0u, w, ext, s8, vals, t);
    if (t < q.slots) {  // tag t: bits [64 t, + 64) of the string of w-bit values
        const uint32_t bit = 64u * t;
        uint32_t c = bit / w, off = bit - c * w;
        uint64_t tag = 0;
        for (uint32_t got = 0; got < 64u; c++) {
            const uint32_t take = min(w - off, 64u - got);
            tag |= ((vals[c] >> off) & ((1ull << take) - 1ull)) << got;
            got += take;
            off = 0;
        }
        if (tag == q.tags[key]) atomicMin(&hit_slot, t);
    }
    __syncthreads();
    const uint32_t slot = hit_slot;
    if (slot != 0xFFFFFFFFu) {
        const uint32_t v0 = 8u * q.slots + slot * V, v1 = v0 + V;  // the value's bytes of the item's stream
        for (uint32_t poly = v0 / poly_bytes; poly * poly_bytes < v1; poly++) {
            if (poly != 0) kv_decode_poly(p, b, poly / p.cols, poly % p.cols, w, ext, s8, vals, t);
            const uint32_t lo = max(v0, poly * poly_bytes), hi = min(v1, (poly + 1u) * poly_bytes);
            for (uint32_t i = lo + t; i < hi; i += kClientTpb) {  // byte i of the item: bits [8 (i - poly * poly_bytes), + 8) of the polynomial's string
                const uint32_t bit = 8u * (i - poly * poly_bytes);
                uint32_t c = bit / w, filled = w - (bit - c * w);
                uint64_t v = vals[c] >> (w - filled);
                while (filled < 8u) {  // (the byte ends inside the polynomial's 2048 w bits: c + 1 < 2048 here)
                    v |= vals[++c] << filled;
                    filled += w;
                }
                q.stage[(size_t)b * V + (i - v0)] = (uint8_t)v;
            }
        }
    }
    // the second of the key's two workgroups to get here settles it: every thread's staged bytes are visible to the device before thread 0 counts
    __threadfence();
    __syncthreads();
    if (t == 0) {
        q.hit[b] = slot != 0xFFFFFFFFu ? 1u : 0u;
        __threadfence();
        arrived = atomicAdd(&q.arrive[key], 1u);
    }
    __syncthreads();
    if (arrived != 1u) return;
    __threadfence();
    const uint32_t win = q.hit[2u * key] ? 0u : q.hit[2u * key + 1u] ? 1u : 2u;  // candidate 1 wins
    for (uint32_t i = t; i < V; i += kClientTpb) q.values[(size_t)key * V + i] = win < 2u ? q.stage[(size_t)(2u * key + win) * V + i] : (uint8_t)0;
    if (t == 0) q.found[key] = win < 2u ? (uint8_t)(win + 1u) : (uint8_t)0;
}

// ---- response noise (include/spiral_gpu.h, spiral_gpu_client_response_noise: the one definition of e) ------------------------------------------
// One workgroup per output polynomial, as the decode.  Switched forms: the decode's operands, convolution and rounding, then e from x.  FINAL form:
// row 0 is a value mod Q of 56 bits, whose sums against the secret do not fit 64 bits; the same convolution runs once per 28-bit prime on the
// residues of row 0 (every sum below 2048 * 64 * 2^28 < 2^46), and the two residues of the product recombine mod Q through crt_compose_lazy.
// The record: every thread folds its eight e, a wave reduces by shuffles, the four waves meet in LDS.  128-bit sums are pairs of 64-bit words with
// an explicit carry.
__device__ __forceinline__ void add128(uint64_t& lo, uint64_t& hi, uint64_t alo, uint64_t ahi) {
    lo += alo;
    hi += ahi + (lo < alo ? 1ull : 0ull);
}
__device__ __forceinline__ uint64_t shfl_down64(uint64_t v, uint32_t off) {
    return pack((uint32_t)__shfl_down((int)lo32(v), off, 64), (uint32_t)__shfl_down((int)hi32(v), off, 64));
}

template <bool FINAL>
__global__ __launch_bounds__(kClientTpb) void client_response_noise_kernel(ClientResponseNoiseParams q) {
    __shared__ int32_t ext[2 * kN];
    __shared__ int8_t s8[kN];
    __shared__ uint64_t red[kClientTpb / 64][6];
    const ClientDecodeParams& p = q.d;
    const uint32_t col = blockIdx.x, r = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
    const size_t poly = ((size_t)b * p.rows + r) * p.cols + col;
    const uint64_t* expected = q.expected ? q.expected + poly * kN : nullptr;
    const int64_t pdb = (int64_t)p.p_db;
    int64_t e[8];
    uint32_t wrong = 0;
    if constexpr (!FINAL) {
        for (uint32_t z = t; z < kN; z += kClientTpb) {
            const int32_t a = (int32_t)(response_value(p, b, col, 0, z) % p.qprime);
            ext[kN + z] = a;
            ext[z] = -a;
            s8[z] = p.sp[(size_t)r * kN + z];
        }
        __syncthreads();
        int64_t acc[8] = {};
        secret_row_convolve(ext, s8, t, acc);
        const int64_t qp = (int64_t)p.qprime, q1 = (int64_t)(4u * p.p_db), denom = qp * 4, span = denom * pdb;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t k = t + 256u * j;
            int64_t x;
            const int64_t res0 = switched_round(acc[j], response_value(p, b, col, 1u + r, k), qp, q1, x);
            if (!expected) {
                e[j] = x - denom * res0;
            } else {
                const int64_t m = (int64_t)expected[k];
                int64_t res = res0 % pdb;
                res += res < 0 ? pdb : 0;
                wrong += res != m ? 1u : 0u;
                int64_t y = (x - denom * m) % span;  // |x| <= p D and D m < p D < 2^62
                y += y < 0 ? span : 0;
                y -= y >= span / 2 ? span : 0;
                e[j] = y;
            }
        }
    } else {
        uint32_t res_p[8];
        uint64_t prod[8];
#pragma unroll 1
        for (int limb = 0; limb < 2; limb++) {
            const uint32_t mod = limb == 0 ? kP : kB;
            if (limb) __syncthreads();  // every wave is done with the first prime's operands
            for (uint32_t z = t; z < kN; z += kClientTpb) {
                const int32_t a = (int32_t)(response_value(p, b, col, 0, z) % kQ % mod);
                ext[kN + z] = a;
                ext[z] = -a;
                if (limb == 0) s8[z] = p.sp[(size_t)r * kN + z];
            }
            __syncthreads();
            int64_t acc[8] = {};
            secret_row_convolve(ext, s8, t, acc);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                int64_t v = acc[j] % (int64_t)mod;
                v += v < 0 ? (int64_t)mod : 0;
                if (limb == 0)
                    res_p[j] = (uint32_t)v;
                else
                    prod[j] = crt_compose_lazy(res_p[j], (uint32_t)v);
            }
        }
        const uint64_t scale = kQ / p.p_db;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t k = t + 256u * j;
            uint64_t v = response_value(p, b, col, 1u + r, k) % kQ + prod[j];
            v -= v >= kQ ? kQ : 0;
            const uint64_t m0 = (v + scale / 2) / scale % p.p_db;
            uint64_t m = m0;
            if (expected) {
                m = expected[k];
                wrong += m0 != m ? 1u : 0u;
            }
            const uint64_t sm = scale * m;  // below Q: m < p
            const uint64_t d = v >= sm ? v - sm : v + kQ - sm;
            e[j] = d >= kQ / 2 ? (int64_t)d - (int64_t)kQ : (int64_t)d;
        }
    }
    if (q.errors) {
#pragma unroll
        for (int j = 0; j < 8; j++) q.errors[poly * kN + t + 256u * j] = e[j];
    }
    if (!q.stats) return;
    // the record of include/spiral_gpu.h: max |e|, n_wrong, the sum of e (128-bit two's complement), the sum of e^2 (128-bit unsigned)
    uint64_t rec[6] = {0, wrong, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint64_t a = (uint64_t)(e[j] < 0 ? -e[j] : e[j]);
        rec[0] = a > rec[0] ? a : rec[0];
        add128(rec[2], rec[3], (uint64_t)e[j], e[j] < 0 ? ~0ull : 0ull);
        add128(rec[4], rec[5], a * a, __umul64hi(a, a));
    }
    auto fold = [&](const uint64_t (&o)[6]) {
        rec[0] = o[0] > rec[0] ? o[0] : rec[0];
        rec[1] += o[1];
        add128(rec[2], rec[3], o[2], o[3]);
        add128(rec[4], rec[5], o[4], o[5]);
    };
#pragma unroll
    for (uint32_t off = 32; off; off >>= 1) {
        uint64_t o[6];
#pragma unroll
        for (int i = 0; i < 6; i++) o[i] = shfl_down64(rec[i], off);
        fold(o);  // (lanes whose partner lies past the wave fold their own value in: only lane 0's result is used)
    }
    if ((t & 63u) == 0) {
#pragma unroll
        for (int i = 0; i < 6; i++) red[t >> 6][i] = rec[i];
    }
    __syncthreads();
    if (t == 0) {
        for (uint32_t w = 1; w < kClientTpb / 64; w++) {
            uint64_t o[6];
#pragma unroll
            for (int i = 0; i < 6; i++) o[i] = red[w][i];
            fold(o);
        }
#pragma unroll
        for (int i = 0; i < 6; i++) q.stats[poly * 6 + i] = rec[i];
    }
}

}  // namespace

void launch_client_noise(const uint32_t* keys, uint32_t domain, uint64_t first, const uint64_t* table, uint64_t* raw, int8_t* centred, const uint64_t* addend,
                         uint32_t per_msg, uint32_t n_msgs, bool nonoise, hipStream_t s) {
    if (per_msg == 0 || n_msgs == 0) return;
    hipLaunchKernelGGL(client_noise_kernel, dim3(per_msg, n_msgs), dim3(kClientTpb), 0, s, keys, domain, first, table, raw, centred, addend, per_msg, nonoise ? 1u : 0u);
}

void launch_client_sample(const ClientSampleParams& p, uint32_t n_msgs, hipStream_t s) {
    if (p.n_cols == 0 || n_msgs == 0) return;
    hipLaunchKernelGGL(client_sample_kernel, dim3(kN / (2u * kClientTpb), p.n_cols, n_msgs), dim3(kClientTpb), 0, s, p);
}

void launch_client_mul(const uint64_t* a, const uint64_t* b, uint64_t* out, uint32_t npolys, hipStream_t s) {
    if (npolys) hipLaunchKernelGGL(client_mul_kernel, dim3(npolys * (kN / kClientTpb)), dim3(kClientTpb), 0, s, a, b, out);
}

void launch_client_wire_encode(const uint64_t* raw, uint8_t* wire, uint32_t npolys, hipStream_t s) {
    if (npolys) hipLaunchKernelGGL(client_wire_encode_kernel, dim3(npolys), dim3(kClientTpb), 0, s, raw, reinterpret_cast<uint64_t*>(wire));
}

void launch_client_decode(const ClientDecodeParams& p, uint32_t n, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(client_decode_kernel, dim3(p.cols, p.rows, n), dim3(kClientTpb), 0, s, p);
}

void launch_client_decode_records(const ClientRecordDecodeParams& p, uint32_t n_entries, hipStream_t s) {
    if (n_entries) hipLaunchKernelGGL(client_decode_records_kernel, dim3(n_entries), dim3(kClientTpb), 0, s, p);
}

void launch_client_kv_find(const ClientKvFindParams& p, uint32_t n_keys, hipStream_t s) {
    if (n_keys == 0) return;
    hipLaunchKernelGGL(client_kv_find_kernel, dim3(2u * n_keys), dim3(kClientTpb), 0, s, p);
}

void launch_client_response_noise(const ClientResponseNoiseParams& p, uint32_t n, hipStream_t s) {
    if (n == 0) return;
    if (p.final_form)
        hipLaunchKernelGGL(client_response_noise_kernel<true>, dim3(p.d.cols, p.d.rows, n), dim3(kClientTpb), 0, s, p);
    else
        hipLaunchKernelGGL(client_response_noise_kernel<false>, dim3(p.d.cols, p.d.rows, n), dim3(kClientTpb), 0, s, p);
}

}  // namespace spiral
