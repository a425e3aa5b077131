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
#include "client_device.h"
#include "common.h"
#include "kernels.h"

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

__global__ __launch_bounds__(kClientTpb) void client_decode_kernel(ClientDecodeParams p) {
    __shared__ int32_t ext[2 * kN];
    __shared__ int8_t s8[kN];
    const uint32_t col = blockIdx.x, r = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
    // the response's value (row, col, z)
    auto value = [&](uint32_t row, uint32_t z) -> uint64_t {
        if (!p.wire) return p.resp[(((size_t)b * (p.rows + 1u) + row) * p.cols + col) * kN + z];
        const uint64_t* w = p.resp + (size_t)b * p.wire_words;
        const uint32_t width = row == 0 ? p.w0 : p.w1;
        const uint64_t idx = row == 0 ? (uint64_t)col * kN + z : ((uint64_t)(row - 1u) * p.cols + col) * kN + z;
        const uint64_t bit = (row == 0 ? 0ull : (uint64_t)p.cols * kN * p.w0) + idx * width;
        const uint32_t sh = (uint32_t)(bit & 63u);
        uint64_t v = w[bit >> 6] >> sh;
        if (sh + width > 64u) v |= w[(bit >> 6) + 1u] << (64u - sh);
        return v & ((1ull << width) - 1ull);
    };
    for (uint32_t z = t; z < kN; z += kClientTpb) {
        const int32_t a = (int32_t)(value(0, z) % p.qprime);
        ext[kN + z] = a;
        ext[z] = -a;
        s8[z] = p.sp[(size_t)r * kN + z];
    }
    __syncthreads();
    int64_t acc[8] = {};
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
    const int64_t qp = (int64_t)p.qprime, q1 = (int64_t)(4u * p.p_db), pdb = (int64_t)p.p_db, denom = qp * 4;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t k = t + 256u * j;
        int64_t vf = acc[j] % qp;
        vf += vf < 0 ? qp : 0;
        vf -= vf >= qp / 2 ? qp : 0;  // to_ntt_qprime's product, centred
        int64_t vr = (int64_t)(value(1u + r, k) % (uint64_t)q1);
        vr -= vr >= q1 / 2 ? q1 : 0;
        const int64_t x = vf * q1 + vr * qp;
        int64_t res = (x + (x >= 0 ? denom / 2 : -(denom / 2))) / denom;  // round half away from zero, truncating division
        res %= pdb;
        res += res < 0 ? pdb : 0;
        p.out[(((size_t)b * p.rows + r) * p.cols + col) * kN + k] = (uint64_t)res;
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

}  // namespace spiral
