// A polynomial of the database image back as plaintext coefficients: what db_export.hip (whole items) and records.hip (records) share, stated once.
// image_word reads one word of the image in the form it is in; unlift_coeff undoes the ingest's centred lift (ntt.hip LD_DBGEN backwards);
// image_poly_plain, the record kernels' composition of the two around the inverse transform, leaves a polynomial's values in LDS.  (db_export_kernel
// keeps its own loop around image_word: as a shared function the loop costs its base packed form 9 VGPRs and a wave of occupancy.)
#pragma once
#include "kernels.h"
#include "ntt_device.h"

namespace spiral {

template <uint32_t FORM, bool PACK>
__device__ __forceinline__ uint64_t image_word(const uint64_t* db, uint32_t z, uint32_t j, uint32_t ii, uint32_t mc, uint32_t num_per, uint32_t dim0) {
    if constexpr (PACK) {
        if constexpr (FORM == DBX_PACKED)
            return db1_get_word(db, z, j, ii, num_per, dim0);
        else if constexpr (FORM == DBX_LIMBS)
            return db1_get_word_limbs(db, z, j, ii, num_per, dim0);
        else
            return db1_get_word_limbs8(db, z, j, ii, dim0);
    } else {
        const uint32_t m = mc >> 1, ic = ii * 2u + (mc & 1u), nic = 2u * num_per;
        if constexpr (FORM == DBX_PACKED)
            return db_get_word(db, z, j, ic, m, nic, dim0);
        else
            return db_get_word_limbs(db, z, j, ic, m, nic, dim0);
    }
}

// Undoing the ingest's centred lift, which maps x < half = p_db >> 1 to x and x >= half to Q - (p_db - x): the plaintext value of the lifted coefficient
// v in [0, Q), or 0 with ok = false when v lies between the two ranges (no plaintext coefficient)
__device__ __forceinline__ uint64_t unlift_coeff(uint64_t v, uint64_t p_db, bool& ok) {
    const uint64_t half = p_db >> 1, top = kQ - (p_db - half);
    ok = v < half || v >= top;
    return !ok ? 0ull : v < half ? v : v - (kQ - p_db);
}

// Polynomial mc of image item (j local, column ii) as plaintext values: sh[c] = coefficient c in [0, p_db), c = 0 .. 2047 (plain index, no padding).
// Returns the lowest coefficient that is no plaintext's (its sh[c] is 0), or kN when every one is.  All 256 threads call it; the caller synchronises
// before it reads sh.
template <uint32_t FORM, bool PACK>
__device__ __forceinline__ uint32_t image_poly_plain(const uint64_t* db, uint32_t j, uint32_t ii, uint32_t mc, uint32_t num_per, uint32_t dim0, uint64_t p_db,
                                                     const uint4* inv, uint64_t* sh, uint32_t tid) {
    uint32_t lo[8], hi[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const uint64_t v = image_word<FORM, PACK>(db, pk_pos_tk(tid, r), j, ii, mc, num_per, dim0);  // z = pk_pos(slot 8 tid + r), as ST_DB
        lo[r] = lo32(v);
        hi[r] = hi32(v);
    }
    ntt_inverse_block<false>(lo, hi, sh, inv, tid);
    __syncthreads();  // the transform's last LDS reads
    uint32_t bad = kN;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        bool ok;
        sh[ix_a(tid, r)] = unlift_coeff(crt_compose_lazy(csub_min(lo[r], kP), hi[r]), p_db, ok);
        if (!ok) bad = min(bad, ix_a(tid, r));
    }
    return bad;
}

}  // namespace spiral
