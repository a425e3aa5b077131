// Records of any byte size on a base image (spiral_gpu_server_read_records / _read_records_at / _update_records; the layout is stated once in
// include/spiral_gpu.h "Records", the work tables in kernels.h RecordWorkParams).  One workgroup per touched polynomial, both ways:
//
// read:   the export's gather + inverse transform + unlift (db_plain_device.h, shared with db_export_kernel), then only the records' byte ranges of the
//         polynomial's 256 w byte stream are stored: a 256-byte record of an 8 KiB item costs one transform and 256 bytes.
// update: read-modify-write of a polynomial.  Gather + inverse transform + unlift, splice the record bytes over the coefficients at bit granularity,
//         centred lift + forward transform (ntt.hip LD_DBGEN's arithmetic), and the 2048 words go out in the linear order db_update_kernel scatters
//         from.  The scatter -- packed words, limb planes and the partner nibbles of items j and j ^ 32 -- stays db_update.hip's: nothing of it is
//         restated here.  It writes whole items, so the polynomials of a touched item that no record touches pass their image words through unchanged
//         (for a limb-plane image put_limbs of db_get_word_limbs' residue gives back the bytes it was read from), and a polynomial the records cover
//         whole skips the gather and the inverse transform.
//
// Splice: the segments of a polynomial are disjoint bit ranges (the host refuses duplicate ids), so a coefficient that lies inside one segment is a
// plain LDS store, and one that two segments share, or that a segment covers in part, is cleared and set with LDS atomics on disjoint bits: the
// waves take the segments in any order without a barrier between them.
//
// SpiralPack (spiral_gpu_pack_server_*_records): the same two bodies with PACK = true.  An item's polynomial t is its 1 x 1 plaintext in trial image t,
// so the entry names the trial and the kernel takes the trial stride (kernels.h PackRecordWorkParams); image_word<FORM, true> reads the packed or plain
// layout, the limb planes and the 8-column pair form.  The update has entries for touched polynomials only, and db_update_trials_kernel scatters them
// into every touched trial image in one launch.  The base kernels keep their names, arguments and resources (profiles/pack_records_resource_usage.txt).
#include "db_plain_device.h"
#include "fingerprint_math.h"
#include "kernels.h"
#include "ntt_device.h"

namespace spiral {

namespace {

// the error word's key of coefficient `coeff` of polynomial `poly` of the `polys` an item has, in the staged record the segment belongs to
__device__ __forceinline__ unsigned long long record_err_key(const RecordWorkParams& p, uint4 seg, uint32_t poly, uint32_t polys, uint32_t coeff) {
    const uint64_t k = (((uint64_t)seg.w << 32) | seg.z) / p.stride;
    return (k * polys + poly) * kN + coeff;
}

// Which polynomial a workgroup has.  A base image (PACK = false): polynomial mc of the 4 of item (j, ii).  A SpiralPack server (PACK = true): the one
// polynomial of item (j, ii) in the trial image the entry names; `poly` is the global trial, as the error word counts it.
struct RecordPoly {
    const uint64_t* db;
    uint32_t j, ii, mc, poly, polys;
};
template <bool PACK>
__device__ __forceinline__ RecordPoly record_poly(const RecordWorkParams& p, uint4 e, uint32_t mc, uint64_t trial_words, uint32_t trials, uint32_t trial0) {
    if constexpr (PACK) {
        const uint32_t tl = e.y >> kPackRecordTrialShift;
        return RecordPoly{p.db + (size_t)tl * trial_words, e.x & kRecordRowMask, e.y & kPackRecordColMask, 0u, trial0 + tl, trials};
    } else {
        return RecordPoly{p.db, e.x & kRecordRowMask, e.y, mc, mc, 4u};
    }
}

template <uint32_t FORM, bool PACK>
__device__ __forceinline__ void record_read_body(const Tables& t, const RecordWorkParams& p, uint64_t* sh, uint64_t trial_words, uint32_t trials, uint32_t trial0) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint4 e = p.entries[blockIdx.x];
    const RecordPoly q = record_poly<PACK>(p, e, (e.x >> kRecordPolyShift) & 3u, trial_words, trials, trial0);
    const uint32_t mc = q.poly, polys = q.polys, nseg = e.w, w = p.w;
    const uint32_t bad = image_poly_plain<FORM, PACK>(q.db, q.j, q.ii, q.mc, p.num_per, p.dim0, p.p_db, t.inv, sh, tid);
    if (bad < kN) atomicMin(p.err, record_err_key(p, p.segs[e.z], mc, polys, bad));
    __syncthreads();
    for (uint32_t s = wave; s < nseg; s += 4u) {
        const uint4 seg = p.segs[e.z + s];
        uint8_t* dst = p.buf + (((uint64_t)seg.w << 32) | seg.z);
        for (uint32_t i = lane; i < seg.y; i += 64u) {  // byte i of the segment: bits [8 (seg.x + i), + 8) of the string of w-bit coefficients
            const uint32_t bit = 8u * (seg.x + i);
            uint32_t c = bit / w, filled = w - (bit - c * w);
            uint64_t v = sh[c];
            if (v >> w) atomicMin(p.err, record_err_key(p, seg, mc, polys, c));
            uint64_t acc = v >> (w - filled);
            while (filled < 8u) {  // (the segment ends inside the polynomial's 2048 w bits: c + 1 < 2048 here)
                v = sh[++c];
                if (v >> w) atomicMin(p.err, record_err_key(p, seg, mc, polys, c));
                acc |= v << filled;
                filled += w;
            }
            dst[i] = (uint8_t)acc;
        }
    }
}

// TRACK (the image's fingerprint is tracked, include/spiral_gpu.h "Fingerprints"): an entry with segments also stores its polynomial sum
// k->gnew[entry] = sum over c of x_c r^(c + 1) mod P, from the coefficients it holds after the splice; k is not looked at otherwise
template <uint32_t FORM, bool PACK, bool TRACK = false>
__device__ __forceinline__ void record_update_body(const Tables& t, const RecordWorkParams& p, uint64_t* sh, uint64_t trial_words, uint32_t trials, uint32_t trial0,
                                                   const RecordTrackParams* k = nullptr) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint4 e = p.entries[blockIdx.x];
    const RecordPoly q = record_poly<PACK>(p, e, blockIdx.x & 3u, trial_words, trials, trial0);
    const uint32_t mc = q.poly, polys = q.polys, nseg = e.w, w = p.w;
    uint64_t* dst = p.enc + (size_t)blockIdx.x * kN;
    if (nseg == 0) {  // no record touches it: the image's words as they are (a base item's other polynomials)
        uint64_t v[8];
#pragma unroll
        for (int r = 0; r < 8; r++) v[r] = image_word<FORM, PACK>(q.db, pk_pos_tk(tid, r), q.j, q.ii, q.mc, p.num_per, p.dim0);
        pk_store8(dst, tid, v);
        return;
    }
    const bool full = (e.x & kRecordFull) != 0;
    if (full) {
#pragma unroll
        for (int r = 0; r < 8; r++) sh[ix_a(tid, r)] = 0;
    } else {
        const uint32_t bad = image_poly_plain<FORM, PACK>(q.db, q.j, q.ii, q.mc, p.num_per, p.dim0, p.p_db, t.inv, sh, tid);
        if (bad < kN) {
            atomicMin(p.err, record_err_key(p, p.segs[e.z], mc, polys, bad));
            *p.flag = 1u;
        }
    }
    __syncthreads();
    unsigned long long* coeffs = reinterpret_cast<unsigned long long*>(sh);
    for (uint32_t s = wave; s < nseg; s += 4u) {
        const uint4 seg = p.segs[e.z + s];
        const uint8_t* src = p.buf + (((uint64_t)seg.w << 32) | seg.z);
        const uint32_t b0 = 8u * seg.x, b1 = b0 + 8u * seg.y;  // the segment's bits of the polynomial's string
        for (uint32_t c = b0 / w + lane; c * w < b1; c += 64u) {
            const uint32_t lo = max(c * w, b0), hi = min((c + 1u) * w, b1), nb = hi - lo, rel = lo - b0;  // bits [lo, hi) of coefficient c: nb <= w <= 40
            uint64_t acc = 0;
            for (uint32_t y = rel >> 3, k = 0; y <= (rel + nb - 1u) >> 3; y++, k++) acc |= (uint64_t)src[y] << (8u * k);  // (at most 6 bytes, all inside the segment)
            const uint64_t mask = (1ull << nb) - 1ull, val = (acc >> (rel & 7u)) & mask;
            if (nb == w) {
                coeffs[c] = val;
            } else {
                const uint32_t sft = lo - c * w;
                if (!full && (coeffs[c] >> w)) {  // its kept bits are no part of a record
                    atomicMin(p.err, record_err_key(p, seg, mc, polys, c));
                    *p.flag = 1u;
                }
                atomicAnd(&coeffs[c], ~(mask << sft));
                atomicOr(&coeffs[c], val << sft);
            }
        }
    }
    __syncthreads();
    // the ingest's centred lift (ntt.hip LD_DBGEN): x < half -> x, x >= half -> Q - (p_db - x), as residues mod p and mod b
    const uint64_t half = p.p_db >> 1;
    uint32_t lo[8], hi[8];
    [[maybe_unused]] uint64_t fp_acc = 0;  // TRACK: 8 canonical terms, each below 2^61
#pragma unroll
    for (int r = 0; r < 8; r++) {
        uint64_t v = coeffs[ix_a(tid, r)];
        if (v >= p.p_db) v %= p.p_db;  // (only after an error was flagged: nothing of this launch is scattered)
        if constexpr (TRACK) fp_acc += fp_mul(v, k->weights[ix_a(tid, r)]);
        if (v >= half) {
            const uint64_t d = p.p_db - v;
            lo[r] = kP - mod_p(d);
            hi[r] = kB - mod_b(d);
        } else {
            lo[r] = mod_p(v);
            hi[r] = mod_b(v);
        }
    }
    __syncthreads();  // every coefficient is in registers before the transform reuses the LDS words
    if constexpr (TRACK) {
        const uint64_t sum = fp_block_sum(fp_reduce(fp_acc), sh, tid);
        if (tid == 0) k->gnew[blockIdx.x] = sum;
        __syncthreads();  // the sum's four LDS words are read before the transform writes them
    }
    ntt_forward_block<false>(lo, hi, sh, t.fwd, tid);
    canonicalize8(lo, hi);
    uint64_t v[8];
    pk_pack8(lo, hi, v);
    pk_store8(dst, tid, v);
}

// the kernels: the bodies above on a base image and on the trial images of a SpiralPack server
template <uint32_t FORM>
__global__ __launch_bounds__(256, 6) void record_read_kernel(Tables t, RecordWorkParams p) {
    __shared__ uint64_t sh[kLdsWords];
    record_read_body<FORM, false>(t, p, sh, 0, 4u, 0);
}
template <uint32_t FORM>
__global__ __launch_bounds__(256, 4) void record_update_kernel(Tables t, RecordWorkParams p) {
    __shared__ uint64_t sh[kLdsWords];
    record_update_body<FORM, false>(t, p, sh, 0, 4u, 0);
}
template <uint32_t FORM>
__global__ __launch_bounds__(256, 6) void pack_record_read_kernel(Tables t, PackRecordWorkParams p) {
    __shared__ uint64_t sh[kLdsWords];
    record_read_body<FORM, true>(t, p.r, sh, p.trial_words, p.trials, p.trial0);
}
template <uint32_t FORM>
__global__ __launch_bounds__(256, 4) void pack_record_update_kernel(Tables t, PackRecordWorkParams p) {
    __shared__ uint64_t sh[kLdsWords];
    record_update_body<FORM, true>(t, p.r, sh, p.trial_words, p.trials, p.trial0);
}
// the update kernels on an image whose fingerprint is tracked (kernels.h RecordTrackParams): kernels of their own, so that the two above keep their resources
template <uint32_t FORM>
__global__ __launch_bounds__(256, 4) void record_update_tracked_kernel(Tables t, RecordWorkParams p, RecordTrackParams k) {
    __shared__ uint64_t sh[kLdsWords];
    record_update_body<FORM, false, true>(t, p, sh, 0, 4u, 0, &k);
}
template <uint32_t FORM>
__global__ __launch_bounds__(256, 4) void pack_record_update_tracked_kernel(Tables t, PackRecordWorkParams p, RecordTrackParams k) {
    __shared__ uint64_t sh[kLdsWords];
    record_update_body<FORM, true, true>(t, p.r, sh, p.trial_words, p.trials, p.trial0, &k);
}

}  // namespace

void launch_record_read(const DeviceTables& t, const RecordWorkParams& p, hipStream_t s) {
    if (p.n_entries == 0) return;
    const Tables tb{t.fwd, t.inv};
    if (p.form == DBX_PACKED)
        hipLaunchKernelGGL((record_read_kernel<DBX_PACKED>), dim3(p.n_entries), dim3(256), 0, s, tb, p);
    else
        hipLaunchKernelGGL((record_read_kernel<DBX_LIMBS>), dim3(p.n_entries), dim3(256), 0, s, tb, p);
}

void launch_record_update(const DeviceTables& t, const RecordWorkParams& p, hipStream_t s) {
    if (p.n_entries == 0) return;
    const Tables tb{t.fwd, t.inv};
    if (p.form == DBX_PACKED)
        hipLaunchKernelGGL((record_update_kernel<DBX_PACKED>), dim3(p.n_entries), dim3(256), 0, s, tb, p);
    else
        hipLaunchKernelGGL((record_update_kernel<DBX_LIMBS>), dim3(p.n_entries), dim3(256), 0, s, tb, p);
}

void launch_pack_record_read(const DeviceTables& t, const PackRecordWorkParams& p, hipStream_t s) {
    if (p.r.n_entries == 0) return;
    const Tables tb{t.fwd, t.inv};
    const dim3 grid(p.r.n_entries), block(256);
    if (p.r.form == DBX_PACKED)
        hipLaunchKernelGGL((pack_record_read_kernel<DBX_PACKED>), grid, block, 0, s, tb, p);
    else if (p.r.form == DBX_LIMBS)
        hipLaunchKernelGGL((pack_record_read_kernel<DBX_LIMBS>), grid, block, 0, s, tb, p);
    else
        hipLaunchKernelGGL((pack_record_read_kernel<DBX_LIMBS8>), grid, block, 0, s, tb, p);
}

void launch_pack_record_update(const DeviceTables& t, const PackRecordWorkParams& p, hipStream_t s) {
    if (p.r.n_entries == 0) return;
    const Tables tb{t.fwd, t.inv};
    const dim3 grid(p.r.n_entries), block(256);
    if (p.r.form == DBX_PACKED)
        hipLaunchKernelGGL((pack_record_update_kernel<DBX_PACKED>), grid, block, 0, s, tb, p);
    else if (p.r.form == DBX_LIMBS)
        hipLaunchKernelGGL((pack_record_update_kernel<DBX_LIMBS>), grid, block, 0, s, tb, p);
    else
        hipLaunchKernelGGL((pack_record_update_kernel<DBX_LIMBS8>), grid, block, 0, s, tb, p);
}

void launch_record_update_tracked(const DeviceTables& t, const RecordWorkParams& p, const RecordTrackParams& k, hipStream_t s) {
    if (p.n_entries == 0) return;
    const Tables tb{t.fwd, t.inv};
    if (p.form == DBX_PACKED)
        hipLaunchKernelGGL((record_update_tracked_kernel<DBX_PACKED>), dim3(p.n_entries), dim3(256), 0, s, tb, p, k);
    else
        hipLaunchKernelGGL((record_update_tracked_kernel<DBX_LIMBS>), dim3(p.n_entries), dim3(256), 0, s, tb, p, k);
}

void launch_pack_record_update_tracked(const DeviceTables& t, const PackRecordWorkParams& p, const RecordTrackParams& k, hipStream_t s) {
    if (p.r.n_entries == 0) return;
    const Tables tb{t.fwd, t.inv};
    const dim3 grid(p.r.n_entries), block(256);
    if (p.r.form == DBX_PACKED)
        hipLaunchKernelGGL((pack_record_update_tracked_kernel<DBX_PACKED>), grid, block, 0, s, tb, p, k);
    else if (p.r.form == DBX_LIMBS)
        hipLaunchKernelGGL((pack_record_update_tracked_kernel<DBX_LIMBS>), grid, block, 0, s, tb, p, k);
    else
        hipLaunchKernelGGL((pack_record_update_tracked_kernel<DBX_LIMBS8>), grid, block, 0, s, tb, p, k);
}

}  // namespace spiral
