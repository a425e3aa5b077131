// The transform launches of the host units, each KIND stated once (host code only: no .hip file includes this).  A job is the parameter struct of
// launch_ntt_forward / launch_ntt_inverse together with its load mode, store mode and block count, built by a pure function -- a program without a
// device can check what a job contains -- and launched by launch_job().  What the builders decide, so that no call site has to:
//   - the digit width: a digit job derives `bits` from its digit count (raw32_job is the one exception, by name);
//   - lazy outputs: a digit job takes the number of products its reader sums per accumulator (0: canonical outputs) and is the only code that turns
//     that into FwdParams::lazy_out, through lazy_ok (kernels.h);
//   - maps: identity unless the site names one.  Fields a kind's loader does not read stay zero.
// The single-site kinds (LD_EXPAND and the inverse-expand launch, LD_WIRE, LD_LIMBS, the reference-layout inverse seams) fill their struct in place.
#pragma once
#include "kernels.h"

namespace spiral {
namespace host {

struct FwdJob {
    FwdParams p;
    uint32_t load, store, nblocks;
};
struct InvJob {
    InvParams p;
    uint32_t store, nblocks;
};
inline void launch_job(const DeviceTables& tb, const FwdJob& j, hipStream_t st) { launch_ntt_forward(tb, j.p, j.load, j.store, j.nblocks, st); }
inline void launch_job(const DeviceTables& tb, const InvJob& j, hipStream_t st) { launch_ntt_inverse(tb, j.p, j.store, j.nblocks, st); }

// ---- lift: npolys PK polynomials -> CRT-lifted raw coefficients (from_ntt, src/poly.cpp:357) ---------------------------------------------------------
struct LiftOpts {
    IndexMap src_map = identity_map(), dst_map = identity_map();
    bool pre_reduce = false;  // the fields are lazy sums (< 2^32)
    uint32_t split = 0;       // > 0: polynomials b >= split come from src_map2(b - split)
    IndexMap src_map2{};
    Lanes lanes{};
};
inline InvJob lift_job(const uint64_t* src, uint64_t* dst, uint32_t npolys, const LiftOpts& o = {}) {
    InvJob j{{}, IST_CRT, npolys};
    j.p.src = src;
    j.p.dst = dst;
    j.p.src_map = o.src_map;
    j.p.dst_map = o.dst_map;
    j.p.pre_reduce = o.pre_reduce ? 1 : 0;
    j.p.split = o.split;
    j.p.src_map2 = o.src_map2;
    j.p.lanes = o.lanes;
    return j;
}

// ---- raw transform: npolys raw polynomials, reduced mod p / mod b (to_ntt, src/poly.cpp:311) ----------------------------------------------------------
inline FwdJob raw_job(const uint64_t* src, uint64_t* dst, uint32_t npolys, FwdStore store = ST_PK, IndexMap src_map = identity_map(), const Lanes& lanes = {}) {
    FwdJob j{{}, LD_RAW, store, npolys};
    j.p.src = src;
    j.p.dst = dst;
    j.p.src_map = src_map;
    j.p.dst_map = identity_map();
    j.p.n_digits = 1;
    j.p.lanes = lanes;
    return j;
}
// to_ntt_no_reduce copies the raw value into both limbs (src/poly.cpp:291-309): it is digit 0 of width 32, the one digit whose width is not
// get_bits_per of its count
inline FwdJob raw32_job(const uint64_t* src, uint64_t* dst, uint32_t npolys) {
    FwdJob j = raw_job(src, dst, npolys);
    j.load = LD_DIGIT;
    j.p.bits = 32;
    return j;
}

// ---- digit jobs: t digits of each of n_src source polynomials, job b = (source b / t, digit b % t) ----------------------------------------------------
// mac_terms: the products the one reader of these transforms sums per u64 accumulator; the outputs are left in [0, 2m) when lazy_ok allows that many
inline FwdJob digit_job(FwdLoad load, const uint64_t* src, uint64_t* dst, uint32_t n_src, uint32_t t, uint32_t mac_terms, const Lanes& lanes) {
    FwdJob j{{}, load, ST_PK, n_src * t};
    j.p.src = src;
    j.p.dst = dst;
    j.p.src_map = identity_map();
    j.p.n_digits = t;
    j.p.bits = get_bits_per(t);
    j.p.lazy_out = mac_terms && lazy_ok(mac_terms) ? 1 : 0;
    j.p.lanes = lanes;
    return j;
}
// unsigned gadget digits (gadget_invert + to_ntt_no_reduce), digit polynomials in job order
inline FwdJob gadget_digits_job(const uint64_t* src, uint64_t* dst, uint32_t n_src, uint32_t t, uint32_t mac_terms = 0, const Lanes& lanes = {}) {
    FwdJob j = digit_job(LD_DIGIT, src, dst, n_src, t, mac_terms, lanes);
    j.p.dst_map = identity_map();
    return j;
}
// the fold's balanced digits into its operand layout: LD_SDIGIT of n_src polynomials of [2 np][3][2] ciphertexts, or LD_SDIFF of their n_src pairs
inline FwdJob fold_digits_job(FwdLoad load, const uint64_t* src, uint64_t* dst, uint32_t n_src, uint32_t ell, uint32_t np, uint32_t mac_terms = 0,
                              const Lanes& lanes = {}) {
    FwdJob j = digit_job(load, src, dst, n_src, ell, mac_terms, lanes);
    j.p.ell = ell;
    j.p.fold_np = np;
    return j;
}
// SpiralPack's unsigned reduced digits: LD_PDIGIT under the maps of `pmode` (pk_num_per: PM_PACK's ciphertext stride of a trial), or LD_PDIFF, the
// fold round in pair form with np ciphertexts per trial
struct PackDigitOpts {
    PackMap pmode = PM_GSW;
    uint32_t pk_num_per = 0, np = 0, mac_terms = 0;
    Lanes lanes{};
};
inline FwdJob pack_digits_job(FwdLoad load, const uint64_t* src, uint64_t* dst, uint32_t n_src, uint32_t t, const PackDigitOpts& o) {
    FwdJob j = digit_job(load, src, dst, n_src, t, o.mac_terms, o.lanes);
    j.p.dst_map = identity_map();
    j.p.fold_np = o.np;
    j.p.pmode = o.pmode;
    j.p.pk_num_per = o.pk_num_per;
    return j;
}

// ---- database encode: plaintext coefficients, centred lift, transform, store in a database layout or linearly (ST_PK, the in-place update) -------------
// LD_DBGEN: 4 polynomials per item of the shard's j-range [j0, j0 + dim0_shard); LD_DBGEN1: one per item of `trial`, total_n items (dim0_shard = dim0)
// item_stride, item_off (LD_DBGEN): the image's item l is the database's item l * item_stride + item_off -- a column shard of G ranks holds the items
// rank (mod G) in an image of num_per / G columns (num_per here is the IMAGE's); 1, 0: the image's items are the database's
struct DbGeometry {
    uint32_t num_per = 0, dim0_shard = 0, j0 = 0, trial = 0;
    uint64_t total_n = 0;
    uint32_t item_stride = 1, item_off = 0;
};
inline FwdJob db_encode_job(FwdLoad load, FwdStore store, uint64_t* dst, uint64_t p_db, const DbGeometry& g = {}) {
    FwdJob j{{}, load, store, 0};
    j.p.dst = dst;
    j.p.src_map = j.p.dst_map = identity_map();
    j.p.n_digits = 1;
    j.p.p_db = p_db;
    j.p.num_per = g.num_per;
    j.p.dim0_shard = g.dim0_shard;
    j.p.j0 = g.j0;
    j.p.trial = g.trial;
    j.p.total_n = g.total_n;
    j.p.item_stride = g.item_stride;
    j.p.item_off = g.item_off;
    return j;
}
// one launch of it: npolys polynomials from item `first` on, from the seeded generator ...
inline void db_encode_seeded(FwdJob& j, uint64_t seed, uint64_t first, uint32_t npolys) {
    j.p.seed = seed;
    j.p.item_base = first;
    j.nblocks = npolys;
}
// ... or from a staged stream of bit-packed items that starts at the database's item `first`; *err is set when a coefficient is not below p_db.
// image_first: the image's first item of the launch where that is not `first` (a strided geometry: the stream is read at item stride item_stride)
inline void db_encode_staged(FwdJob& j, const uint8_t* items, uint32_t coeff_bits, uint32_t* err, uint64_t first, uint32_t npolys, uint64_t image_first = ~0ull) {
    j.p.items = items;
    j.p.coeff_bits = coeff_bits;
    j.p.err = err;
    j.p.items_first = first;
    j.p.item_base = image_first == ~0ull ? first : image_first;
    j.nblocks = npolys;
}

}  // namespace host
}  // namespace spiral
