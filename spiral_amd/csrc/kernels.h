// Host-callable launchers for the HIP kernels (internal interface between server.cpp and *.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <atomic>

#include "common.h"

namespace spiral {

// block/poly index map: idx(b) = (b / inner) * outer_stride + (b % inner) + off
struct IndexMap {
    uint32_t inner, outer_stride, off;
    __host__ __device__ uint32_t operator()(uint32_t b) const { return (b / inner) * outer_stride + (b % inner) + off; }
};
inline IndexMap identity_map() { return IndexMap{1u, 1u, 0u}; }

// Environment switches.  The shipped library reads exactly three, all documented in README.md: SPIRAL_FOLD_PAIR, SPIRAL_SWEEP_MFMA and
// SPIRAL_DB_STAGE_BYTES (initial values of the options of spiral_gpu_set_option, include/spiral_gpu.h).  The thresholds that only a tuning
// session moves (tools/build_variants.sh builds with -DSPIRAL_TUNING) are read through tuning_env, which is a constant nullptr otherwise.
#ifdef SPIRAL_TUNING
inline const char* tuning_env(const char* name) { return getenv(name); }
#else
inline const char* tuning_env(const char*) { return nullptr; }
#endif
// Process-wide options (spiral_gpu_set_option).  fwd2: -1 = the two-digits-per-workgroup transform kernel from kFwd2Min transforms per
// launch (ntt.hip), 0 / 1 = never / always.  Same results either way; tests force each form.
struct Options {
    int fold_pair = 1, fold_chain = 1, fwd2 = -1;
    uint32_t fold_blocks = 768, sweep_mfma_min = 2, fwd2_min = 8192;
    size_t db_stage_bytes = (size_t)64 << 20;
    int one_image = 1;  // a server that batches on the matrix cores keeps ONLY the limb-plane image of its database (server.cpp)
    uint32_t pack_item_group = 0;  // pack answer_batch_instances: instances per group, 0 = automatic (pack_server.cpp)
    uint32_t pack_batch_lanes = 0;  // SpiralPack batch calls of at least this many clients run as ONE lane-aware launch sequence, 0 = never: the default,
                                    // until the lane form is measured against the per-lane form
    int pack_pair_blocks = 0;  // 1: a SpiralPack image of 8 ciphertexts per slot may TAKE the limb-plane form (the pair form of the matrix-core sweep,
                               // sweep_mfma.hip); read only where that is decided (db_image.h DbLayout::limbs_ok), never by what works on a converted image
    int sweep_narrow = 0;  // 1: a base image of 8, 16 or 32 ciphertexts per slot may TAKE the limb-plane form (the W forms of the matrix-core sweep, sweep_mfma.hip);
                           // read only where that is decided (db_image.h DbLayout::limbs_ok), never by what works on a converted image
    uint32_t query_batch_chunk = 512;  // set_query_batch: message polynomials per lane per staging pass of messages too large to check on the host
                                       // (= message.h kWireChunkPolys / kMaxLanes: all lanes together fill set_query_wire's staging), at least 1
    uint32_t kv_scan_chunk = 0;  // kv_scan / kv_scan_at: buckets per pass, 0 = automatic (kv_host.h kv_scan_pass), else 1 .. 2^16
};
Options& options();  // server.cpp; the three documented environment variables are read once, on first use

// Query lanes of one launch (server.cpp run_query_batch).  The launch-bound stages of a query -- expansion, conversion, lift, folding: ~50
// dependent launches that cost ~5 us each whatever they carry -- take a QUERY dimension: gridDim.z = n <= kMaxLanes queries, each with its own
// keys, ciphertexts and scratch.  Every per-query buffer of a server lives in one arena with the same internal layout (srv_alloc), so lane q's
// buffer is lane 0's pointer + off[q] words: a kernel shifts every non-table pointer of its parameters by off[blockIdx.z] and is otherwise
// unchanged (n = 1, off = 0: the single-query launch).  The reference answers one query per process_crtd_query (src/spiral.cpp:2337-2406).
#ifndef SPIRAL_MAX_LANES
#define SPIRAL_MAX_LANES 8
#endif
constexpr uint32_t kMaxLanes = SPIRAL_MAX_LANES;  // (= the queries one pass of the matrix-core sweep takes, sweep_mfma.hip)
struct Lanes {
    uint32_t n = 1;
    int64_t off[kMaxLanes] = {};  // u64 words from lane 0's arena to lane q's
#ifdef __HIPCC__
    // (a select chain on constant indices: indexing the by-value kernel argument with blockIdx.z would make the compiler keep the whole
    // parameter struct in scratch memory -- 232 bytes per lane and transforms twice as slow, measured)
    __device__ __forceinline__ int64_t here() const {
        const uint32_t z = blockIdx.z;
        int64_t o = 0;
#pragma unroll
        for (uint32_t q = 1; q < kMaxLanes; q++) o = z == q ? off[q] : o;
        return o;
    }
    // lane q's place in a caller's [lane][...] buffer of `stride` words per lane (run_query_batch_instances' outputs)
    __device__ __forceinline__ int64_t at(int64_t stride) const { return (int64_t)blockIdx.z * stride; }
#endif
};
#ifdef __HIPCC__
template <class T>
__device__ __forceinline__ void lane_shift(T*& p, int64_t words) {  // optional (null) pointers stay null
    if (p) p = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + (intptr_t)words * 8);
}
#endif
// ONE query's launches carry no lane machinery at all.  A query is ~50 dependent launch-bound launches, and each pays for every instruction of its
// prologue: with the eight offsets in every launch (eight scalar loads and a select chain before the first address is known) one query took 748 us,
// without them 725 (round 6, same box, alternating builds; 64 bytes of UNUSED kernel arguments cost nothing measurable: it is the dependent prologue).  So every kernel that takes lanes is instantiated twice -- `Lanes` for batches, `NoLanes` (no
// offsets, here() == 0, the shifts fold away) for n == 1 -- and every parameter struct is `XCore` (the fields) + `XT<L>` (the fields and an L); the
// host fills an `X = XT<Lanes>` as before and the launcher picks the instantiation (no_lanes() copies the fields).
struct NoLanes {
    uint32_t n = 1;
#ifdef __HIPCC__
    __device__ __forceinline__ int64_t here() const { return 0; }
    __device__ __forceinline__ int64_t at(int64_t) const { return 0; }
#endif
};
// The n responses of one client's item group (pack_server.cpp answer_batch_instances): slot k = blockIdx.z, `stride` words after slot k - 1 in the
// input, and in the output where the launch takes no stride of its own.  Only the switch and the wire form take it.
struct Slots {
    uint32_t n = 1;
    int64_t stride = 0;
#ifdef __HIPCC__
    __device__ __forceinline__ int64_t here() const { return (int64_t)blockIdx.z * stride; }
    __device__ __forceinline__ int64_t at(int64_t s) const { return (int64_t)blockIdx.z * s; }
#endif
};
template <class P>
inline typename P::NoLanesT no_lanes(const P& p) {
    typename P::NoLanesT q{};
    static_cast<typename P::Core&>(q) = static_cast<const typename P::Core&>(p);
    return q;
}

struct DeviceTables {
    uint4* fwd = nullptr;      // [2048] forward twiddles {W_p, W'_p, W_b, W'_b}
    uint4* inv = nullptr;      // [2048] inverse twiddles psi^-i (row 1 times N^-1, row 0 = N^-1: the stages are unscaled, tables.cpp)
    uint64_t* neg1 = nullptr;  // [11][2048] PK: NTT(-x^(N-2^r))   (src/spiral.cpp:171-190)
    uint64_t* neg1s = nullptr; // the same words' Shoup companions floor(w * 2^32 / m), PK
};
// builds the tables on `device` (host computes psi powers, tables.cpp); idempotent per device
int tables_get(int device, DeviceTables* out);
// host copy of the reference-ordered rows (for the C-ABI's spiral_gpu_get_tables)
void tables_host_rows(uint64_t* out8x2048);

// Lazy digit transforms.  A forward transform of gadget digits may leave its outputs in [0, 2m) instead of [0, m) (FwdParams::lazy_out,
// FoldChainParams::lazy_out, always for LD_EXPAND) ONLY when every reader is a u64 multiply-accumulate (poly.hip Acc2, pack.hip)
// against canonical words summing at most `terms` products per accumulator: terms * (2m - 1) * (m - 1) must stay below 2^64.
// Kernels that add or compare such words (add_pk, csub, canonical stores) need canonical operands and must not be fed lazy ones.
// This is the one place the bound is decided; the hosts call it with the number of products their MAC kernel sums.
constexpr bool lazy_ok(uint32_t terms) { return (unsigned __int128)terms * (2ull * kP - 1ull) * (kP - 1ull) < ((unsigned __int128)1 << 64); }
static_assert(lazy_ok(56) && lazy_ok(2 * 56) && lazy_ok(128) && !lazy_ok(129), "u64 accumulators hold up to 128 lazy products");

// ---- forward NTT ---------------------------------------------------------------------------------
enum FwdLoad : uint32_t {
    LD_RAW = 0,     // raw u64 coefficient, reduced mod p / mod b        (to_ntt, src/poly.cpp:311)
    LD_DIGIT = 1,   // unsigned gadget digit k of a raw coefficient      (gadget_invert + to_ntt_no_reduce)
    LD_SDIGIT = 2,  // balanced digit with the fold's carry rules        (split_and_crt, src/spiral.cpp:270)
    LD_LIMBS = 3,   // reference NTT layout [2][N] u64 taken as per-limb coefficient arrays (ntt_forward)
    LD_DBGEN = 4,   // seeded plaintext coefficient, centred lift        (load_db, src/spiral.cpp:1116-1127)
    LD_PDIGIT = 6,  // SpiralPack: unsigned reduced digit k (gadget_invert + to_ntt, src/testing.cpp:130-131, 226-227, 612-617)
                    // with the source / destination maps of FwdParams::pmode
    LD_DBGEN1 = 7,  // SpiralPack database: 1 x 1 plaintext of (trial, item), centred lift (src/testing.cpp:845-869)
    LD_SDIFF = 8,   // fold round in pair form from lifted ciphertexts: difference of the balanced digits k of raw[np + i] and raw[i]
    LD_PDIFF = 9,   // SpiralPack fold round in pair form from lifted ciphertexts [trial][2 np][2]: difference of the unsigned digits k of
                    // ct np + i and ct i, destination D'[trial][i][row + 2k]  (foldCiphertextsDim1 through the same identity as LD_SDIFF)
    LD_EXPAND = 5,  // one expansion round: digits of automorph(c)[0] and the reduced automorph(c)[1] of every
                    // active ciphertext, both parities, in one launch      (src/spiral.cpp:1711-1720)
    LD_WIRE = 10,   // raw coefficient in its 7-byte wire form (kWirePolyBytes per polynomial at `items`), reduced as LD_RAW; a value above Q
                    // atomicMin's (~seed << 32 | its message-wide index) into the u64 at err (item_base = the chunk's first polynomial, seed = the
                    // call's generation: a later call's entries compare below every earlier one's, so the word is never reset; ST_PK only, no lanes)
};
constexpr uint32_t kWireCoeffBytes = 7;                        // logQ = 56 bits, little-endian
constexpr uint32_t kWirePolyBytes = kWireCoeffBytes * 2048u;   // 14 336: a multiple of 16
enum FwdStore : uint32_t {
    ST_PK = 0,      // packed slot words
    ST_REF = 1,     // reference layout [2][N] u64
    ST_DB = 2,      // scatter into the device DB layout (see sweep)
    ST_DB1 = 3,     // scatter into the SpiralPack device DB layout (pack.hip)
};
enum PackMap : uint32_t {
    PM_GSW = 0,   // s = (input ct, row); dst = chat[ct][row + 2k]                     (regevToSimpleGsw)
    PM_FOLD = 1,  // s = (trial, ct i' < 2np', row); dst = D[trial][i' % np'][(i' / np') * 2ell + row + 2k]
    PM_PACK = 2,  // s = trial; source = row 0 of the trial's folded ct; dst = ginv[trial][k]   (pack)
};
struct FwdParamsCore {
    const uint64_t* src;
    uint64_t* dst;
    IndexMap src_map;   // s -> source polynomial index
    IndexMap dst_map;   // b -> destination polynomial index (ST_PK / ST_REF)
    uint32_t n_digits;  // b -> (s = b / n_digits, k = b % n_digits)
    uint32_t inv_n_digits, inv_te, inv_to;  // 2^32 / d + 1 for the three job-index divisors (filled in by launch_ntt_forward)
    uint32_t bits;      // digit width
    uint32_t ell;       // LD_SDIGIT: digits per value (t_GSW)
    uint32_t tinv;      // automorphism gather x -> x^t folded into the load: t^-1 mod 2N, 0 = none
    uint32_t lazy_out;  // ST_PK: 1 = leave the outputs in [0, 2m) instead of [0, m): allowed when the only readers are u64
                        // multiply-accumulate kernels summing fewer than 128 products (digit operands); LD_EXPAND always does
    uint32_t fold_np;   // LD_SDIGIT: num_per' (destination is the fold operand layout)
    // LD_PDIGIT: map selector; fold_np = np' and num_per (ct stride of a trial in the raw buffer) for PM_FOLD / PM_PACK
    uint32_t pmode, pk_num_per;
    // LD_DBGEN1: trial and total item count
    uint32_t trial;
    uint64_t total_n;
    // LD_EXPAND: active ct a < cnt_e is even (t_e digits), the rest odd (t_o digits); jobs per ct = t
    uint32_t cnt_e, t_e, t_o;
    // LD_DBGEN / LD_DBGEN1: plaintext coefficients come from the seeded generator, or (items != null) from a staged
    // stream of bit-packed items whose first item is items_first (common.h packed_coeff); err: set to 1 when a
    // coefficient is not below p_db (the reference asserts, src/spiral.cpp:1117)
    const uint8_t* items;
    uint32_t coeff_bits;
    uint64_t items_first;
    uint32_t* err;
    // LD_DBGEN / ST_DB
    uint64_t seed, p_db;
    uint64_t item_base;                 // first item (of the image) handled by this launch
    uint32_t num_per, dim0_shard, j0;   // DB geometry of this shard
    uint32_t item_stride, item_off;     // LD_DBGEN: the image's item l is the database's item l * item_stride + item_off (transform_jobs.h DbGeometry)
};
template <class L>
struct FwdParamsT : FwdParamsCore {
    using Core = FwdParamsCore;
    using NoLanesT = FwdParamsT<NoLanes>;
    L lanes;                        // src, dst per query lane
};
using FwdParams = FwdParamsT<Lanes>;
void launch_ntt_forward(const DeviceTables& t, const FwdParams& p, uint32_t load, uint32_t store, uint32_t nblocks, hipStream_t s);

// Which ciphertexts of an expansion round a launch works on (src/spiral.cpp:1700-1702 enumerates i < 2^(r+1), odd i only up to
// `stopround`).  Active ciphertext a < cnt_e is the even one i = 2 (a + e_off); the others are odd, i = 2 ((a - cnt_e) *
// (o_stride_m1 + 1) + o_off) + 1.  All zero = every ciphertext of the round (one GPU).  A rank of a G-GPU answer expands only
// what it needs (server.cpp expand shard): the even subtree above its own first-dimension range (a contiguous block of a),
// and of the odd ciphertexts -- the GSW bits -- every G-th.
struct ExpandActive {
    uint32_t e_off, o_stride_m1, o_off;
    __host__ __device__ uint32_t index(uint32_t a, uint32_t cnt_e) const {
        return a < cnt_e ? 2u * (a + e_off) : 2u * ((a - cnt_e) * (o_stride_m1 + 1u) + o_off) + 1u;
    }
};

// ---- inverse NTT ---------------------------------------------------------------------------------
enum InvStore : uint32_t {
    IST_CRT = 0,    // CRT-lifted raw coefficient in [0, Q)   (from_ntt, src/poly.cpp:357)
    IST_LIMBS = 1,  // reference layout [2][N] u64 residues   (ntt_inverse)
};
struct InvParamsCore {
    const uint64_t* src;
    uint64_t* dst;
    IndexMap src_map, dst_map;
    uint32_t pre_reduce;  // 1: fields are lazy sums (< 2^32), reduce mod m first
    uint32_t src_ref;     // 1: source is reference layout [2][N] u64 instead of PK
    uint32_t split;       // > 0: blocks b >= split take their source from src_map2(b - split) (two source regions, one launch)
    IndexMap src_map2;
    // expansion round (launch_ntt_inverse_expand): block b = (active ct a, row); a < cnt_e -> i = 2a, else
    // i = 2(a - cnt_e) + 1; a ct with i >= num_in is first created as neg1 * cv[i - num_in] (src/spiral.cpp:1709)
    // Row 0 is transformed to dst[2a]; row 1 is not: its automorphed image, a slot permutation, goes to dst[2a + 1] in PK.
    uint64_t* cv;
    const uint64_t* neg1;
    const uint64_t* neg1s;  // Shoup companions of neg1
    uint32_t num_in, cnt_e;
    ExpandActive act;
    uint32_t auto_t;  // the round's automorphism x -> x^t
    uint32_t create_here;  // 1: cts with i >= num_in do not exist yet (round 0); 0: the previous round's MAC wrote them
    const uint64_t* query;  // create_here only, optional: cv[0] is read from here (and written to cv) instead of from cv
};
template <class L>
struct InvParamsT : InvParamsCore {
    using Core = InvParamsCore;
    using NoLanesT = InvParamsT<NoLanes>;
    L lanes;            // src, dst, cv, query per query lane (neg1 / neg1s are shared tables)
};
using InvParams = InvParamsT<Lanes>;
void launch_ntt_inverse(const DeviceTables& t, const InvParams& p, uint32_t store, uint32_t nblocks, hipStream_t s);
void launch_ntt_inverse_expand(const DeviceTables& t, const InvParams& p, uint32_t nblocks, hipStream_t s);

// fold chain (ntt.hip): PK polynomials [2*np][3][2] -> inverse transform, CRT lift, balanced digits, forward transforms
// into the fold operand layout D (as LD_SDIGIT); a workgroup handles one polynomial and dpb consecutive digits
struct FoldChainParamsCore {
    const uint64_t* src;
    uint64_t* dst;
    uint32_t ell, bits, fold_np;
    uint32_t pre_reduce;  // 1: fields are lazy sums (< 2^32), reduce mod m first
    uint32_t dpb;         // digits per block, 1 .. ell
    uint32_t lazy_out;    // 1: digit transforms left in [0, 2m) (the product kernel sums 6 * ell < 128 terms of < 2^57)
    // SpiralPack fold (foldCiphertextsDim1): sources are [trial][2*np][2] 2 x 1 ciphertexts with a trial stride of src_stride
    // ciphertexts, unsigned digits, operand layout as LD_PDIGIT / PM_FOLD
    uint32_t pack, src_stride;
};
template <class L>
struct FoldChainParamsT : FoldChainParamsCore {
    using Core = FoldChainParamsCore;
    using NoLanesT = FoldChainParamsT<NoLanes>;
    L lanes;
};
using FoldChainParams = FoldChainParamsT<Lanes>;
void launch_fold_chain(const DeviceTables& t, const FoldChainParams& p, uint32_t n_src, hipStream_t s);

// The fold round in pair form (ntt.hip LD_SDIFF + launch_fold_mac with an addend): out[i] = C[i] + Q * NTT(G^-1(C[np + i]) - G^-1(C[i])).
// split_and_crt's digits recompose the value exactly -- no borrow is lost at the top of the second carry chain -- when the
// digits cover at least 57 bits (values are below Q < 2^56) and every shift is a defined one
constexpr bool fold_pair_exact(uint32_t ell) { return ell >= 2 && ell * get_bits_per(ell) >= 57 && (ell - 1) * get_bits_per(ell) < 64; }

// ---- layout conversion at the C-ABI boundary -------------------------------------------------------
// reference polynomial b <-> packed polynomial pk_map(b)
void launch_ref_to_pk(const uint64_t* ref, uint64_t* pk, uint32_t npolys, IndexMap pk_map, hipStream_t s);
void launch_pk_to_ref(const uint64_t* pk, uint64_t* ref, uint32_t npolys, IndexMap pk_map, hipStream_t s);
// row 0 of a seeded message (seed.hip, seed_device.h): row-0 polynomials k0 .. k0 + npolys - 1 of domain `domain` under the 32-byte seed, in PK
// form, polynomial j to pk_map(j)
void launch_seed_rows(const uint8_t* seed, uint32_t domain, uint64_t k0, uint64_t* pk, IndexMap pk_map, uint32_t npolys, hipStream_t s);

// ---- client keys from a key store into the lanes of a call (keys.hip; key_store.h) ----------------------
// A slot of a key store holds one client's public parameters in PK form, the parts of their message layout (message.h) back to back after `head`
// words.  KEYS_FULL: every polynomial.  KEYS_COMPACT: the words of the message's 32-byte seed open the slot, and only rows 1.. of every matrix
// follow, densely; the bind generates row 0 from the seed, the words launch_seed_rows writes.
enum KeyForm : int { KEYS_FULL = 0, KEYS_COMPACT = 1 };  // (= SPIRAL_GPU_KEYS_FULL / _COMPACT)
constexpr uint32_t kKeyCompactHead = 32;  // words in front of a COMPACT slot's polynomials: the seed, padded to a 256-byte piece
struct KeyPart {
    uint64_t* dst;       // lane 0's buffer of the part
    uint32_t polys;      // its polynomials in the destination: matrices of [rows][cols], back to back (0: a part the message does not have)
    uint32_t rows, cols;
    uint32_t src;        // the slot's polynomial index of the first one the part stores
    uint32_t row0;       // the row-0 polynomials of the parts before it (the seeded form's k of its first)
};
struct KeyBindParams {
    const uint64_t* store;  // slot 0
    uint64_t slot_words;
    uint32_t head;          // words of a slot in front of its polynomials
    uint32_t domain;        // the seeded form's domain tag
    KeyPart part[4];
    uint32_t slot[kMaxLanes];  // lane q's slot
    Lanes lanes;               // lane q's arena offset (gridDim.z = lanes.n)
};
void launch_key_bind(const KeyBindParams& p, KeyForm form, hipStream_t s);

// ---- the queries of a batch's lanes from their staged messages into their query buffers (query_ingest.hip) ----------------------
// One launch covers destination polynomials first_dst .. first_dst + n_dst - 1 of every lane's query buffer (gridDim.x = n_dst, gridDim.z = lanes).
// The query is matrices of [rows][cols] polynomials back to back (message.h query_layout).  Lane q's staged bytes start at stage + q * lane_stride:
// `head` bytes (the seeded form: the message's 32-byte seed), then the wire form of message polynomials first_msg .. of this pass.  QUERY_WIRE:
// destination polynomial d is message polynomial d, decoded and transformed as LD_WIRE + ST_PK does.  QUERY_SEEDED: the message holds rows 1.. of
// every matrix only; a row-0 destination is generated from the lane's seed (seed_device.h, the words launch_seed_rows writes).  A coefficient above
// Q atomicMin's (~gen << 32 | (lane * msg_polys + message polynomial) * 2048 + index) into the u64 at err (wire_device.h).
enum QueryForm : int { QUERY_WIRE = 0, QUERY_SEEDED = 1 };
struct QueryIngestParams {
    const uint8_t* stage;
    uint64_t lane_stride;  // bytes, a multiple of 16
    uint32_t head;         // bytes of a lane's staging in front of its polynomials, a multiple of 16
    uint64_t* dst;         // lane 0's query buffer
    uint32_t rows, cols;
    uint32_t domain;       // the seeded form's domain tag
    uint32_t first_dst, first_msg;
    uint32_t msg_polys;    // polynomials a lane's whole message sends
    uint32_t* err;
    uint64_t gen;
    Lanes lanes;           // lane q's arena offset
};
void launch_query_ingest(const DeviceTables& t, const QueryIngestParams& p, QueryForm form, uint32_t n_dst, hipStream_t s);

// ---- pointwise polynomial kernels (poly.hip) -------------------------------------------------------
// out[b][r][c] = sum_m A[r][m] * B[b][m][c]  (+ addend), all PK; generic MatPoly multiply (src/poly.cpp:34)
struct MatmulParamsCore {
    const uint64_t* a;  // [rs][ms] polys, stride a_batch polys between batches (0 = shared)
    const uint64_t* b;  // [ms][cs] polys
    uint64_t* out;      // [rs][cs] polys
    uint32_t rs, ms, cs;
    uint32_t a_batch, b_batch, out_batch;  // strides in polynomials
};
template <class L>
struct MatmulParamsT : MatmulParamsCore {
    using Core = MatmulParamsCore;
    using NoLanesT = MatmulParamsT<NoLanes>;
    L lanes;  // a, b, out per query lane (the SpiralPack conversion of a batch: each client's V and digits)
};
using MatmulParams = MatmulParamsT<Lanes>;
void launch_matmul(const MatmulParams& p, uint32_t batch, hipStream_t s);
// fold product: out[i][3][2] = key[3][K] * d[i][K][2], K = 2*m2 (src/spiral.cpp:1361-1383)
// key_stride: polynomials between the key's rows (K when the rows are K long; 2*m2 with K = m2 to take one half of [Q_neg | Q]);
// addend: optional [np][3][2] PK polynomials added to the products (fields may be any u32: lazy sums are fine)
void launch_fold_mac(const uint64_t* key, const uint64_t* d, uint64_t* out, uint32_t K, uint32_t np, hipStream_t s, uint32_t key_stride = 0,
                     const uint64_t* addend = nullptr, const Lanes& lanes = Lanes{});
// the reference's two-product fold round Q_neg D_L + Q D_H from the matrices q[3][m2] alone (Q_neg = G2 - Q is derived: poly.hip fold_mac_two_kernel);
// d: [np][2 halves][m2][2] (the LD_SDIGIT / fold_chain operand layout)
void launch_fold_mac_two(const uint64_t* q, const uint64_t* d, uint64_t* out, uint32_t m2, uint32_t ell, uint32_t bits, uint32_t np, hipStream_t s,
                         const Lanes& lanes = Lanes{});
// out = (a + b) mod m ; out = single * a (src/poly.cpp:138,190)
void launch_add(const uint64_t* a, const uint64_t* b, uint64_t* out, uint32_t npolys, hipStream_t s);
void launch_mul_by_const(const uint64_t* single, const uint64_t* a, uint64_t* out, uint32_t npolys, hipStream_t s);
// raw-domain automorphism / negation (src/poly.cpp:240,269)
void launch_automorph(const uint64_t* in, uint64_t* out, uint32_t npolys, uint32_t t, hipStream_t s);
void launch_invert(const uint64_t* in, uint64_t* out, uint32_t npolys, hipStream_t s);
// unsigned gadget digits in the raw domain (src/util.cpp:114)
void launch_gadget_invert(const uint64_t* in, uint64_t* out, uint32_t mx, uint32_t rdim, uint32_t cols, hipStream_t s);
// response modulus switch (src/poly.cpp:578-601, src/spiral.cpp:1441-1447)
void launch_rescale(const uint64_t* in, uint64_t* out, uint32_t n, uint64_t inp_mod, uint64_t out_mod, hipStream_t s);
// lanes.n > 1: lane q's switched response goes to out + q * out_stride words (out_stride = 0: to lane q's arena, out + lanes.off[q]), and its wire form
// is packed from in + q * in_stride (0: lane q's arena) to out + q * out_stride
void launch_response_wire(const uint64_t* in, uint64_t* out, uint32_t n0, uint32_t w0, uint32_t n1, uint32_t w1, hipStream_t s, const Lanes& lanes = Lanes{},
                          int64_t in_stride = 0, int64_t out_stride = 0);
void launch_rescale2(const uint64_t* in, uint64_t* out, uint32_t n0, uint32_t n, uint64_t inp_mod, uint64_t out_mod0, uint64_t out_mod1, hipStream_t s,
                     const Lanes& lanes = Lanes{}, int64_t out_stride = 0);
// the same for slots.n responses, slot k at in / out + k * slots.stride words (wire: in + k * slots.stride, out + k * out_stride words)
void launch_rescale2_slots(const uint64_t* in, uint64_t* out, uint32_t n0, uint32_t n, uint64_t inp_mod, uint64_t out_mod0, uint64_t out_mod1, const Slots& slots,
                           hipStream_t s);
void launch_response_wire_slots(const uint64_t* in, uint64_t* out, uint32_t n0, uint32_t w0, uint32_t n1, uint32_t w1, const Slots& slots, int64_t out_stride,
                                hipStream_t s);

// ---- expansion / conversion / fold specials ----------------------------------------------------------
// the same for a whole round in one launch: active ct a < cnt_e even (W_left, t_e digits) else odd (W_right, t_o);
// g holds t digit polynomials per ct in LD_EXPAND job order; a1[2a + 1] is NTT(automorph(c_1)) of active ct a
struct ExpandMacParamsCore {
    uint64_t* cv;
    const uint64_t* w_e;
    const uint64_t* w_o;
    const uint64_t* g;
    const uint64_t* a1;
    uint32_t cnt_e, cnt_o, t_e, t_o;
    ExpandActive act;
    // next round's new ciphertexts cv[i + next_num_in] = neg1 * cv[i] (src/spiral.cpp:1709), written while the updated cv[i]
    // is in registers: every even i, and odd i when (i - 1)/2 + next_num_in/2 < next_cnt_o (the whole round's count of odd
    // ciphertexts, not a shard's).  neg1n == null: none.
    const uint64_t* neg1n;
    const uint64_t* neg1ns;  // Shoup companions
    uint32_t next_num_in, next_cnt_o;
};
template <class L>
struct ExpandMacParamsT : ExpandMacParamsCore {
    using Core = ExpandMacParamsCore;
    using NoLanesT = ExpandMacParamsT<NoLanes>;
    L lanes;  // cv, w_e, w_o, g, a1 per query lane (neg1n / neg1ns are shared tables)
};
using ExpandMacParams = ExpandMacParamsT<Lanes>;
void launch_expand_mac_round(const ExpandMacParams& p, hipStream_t s);
// scalToMat product: out[a][r][c] = sum_k W[r][2k+c] * G[a][k] + pad(cv[pos(a)][1])   (src/spiral.cpp:1850-1885)
// qs != null: also (or instead, out may be null) write the sweep's query records (see sweep)
struct Scal2MatParamsCore {
    const uint64_t* w;    // [3][2*t_conv] PK
    const uint64_t* g;    // [count][t_conv] PK digits of cv row 0
    const uint64_t* cv;   // expanded cts
    IndexMap cv_pos;      // a -> ct index in cv
    uint64_t* out;        // [count][3][2] PK or null
    uint32_t* qs;         // sweep query records [N][jm_total/2][12] u32 or null
    uint32_t t_conv, count, jm_total, j_base;
};
template <class L>
struct Scal2MatParamsT : Scal2MatParamsCore {
    using Core = Scal2MatParamsCore;
    using NoLanesT = Scal2MatParamsT<NoLanes>;
    L lanes;  // every pointer per query lane
};
using Scal2MatParams = Scal2MatParamsT<Lanes>;
void launch_scal2mat(const Scal2MatParams& p, hipStream_t s);
// regevToGSW assembly for one dimension: gsw[r][3i] = sum_k V[r][k] * chat[i][k], gsw[r][3i+1+c] = scalToMat(cv_i)[r][c]
struct GswParamsCore {
    const uint64_t* w;     // [3][2*t_conv]
    const uint64_t* v;     // [3][2*t_conv]
    const uint64_t* chat;  // [dims*ell][2*t_conv] PK digits (cv row 0 digits, then row 1 digits)
    const uint64_t* cv;
    IndexMap cv_pos;       // i (over dims*ell) -> ct index
    uint64_t* gsw;         // optional: [dims][3][3*ell] PK, dimension d stored at index (dims-1-d)  (src/spiral.cpp:2324)
    uint64_t* key;         // optional: the fold key of the same matrices, written in the same pass: key[d][r][0..m2) = G2 - gsw (= Q_neg, src/spiral.cpp:2361-2379), key[d][r][m2..2*m2) = gsw
    uint32_t t_conv, ell, dims;
};
template <class L>
struct GswParamsT : GswParamsCore {
    using Core = GswParamsCore;
    using NoLanesT = GswParamsT<NoLanes>;
    L lanes;  // every pointer per query lane
};
using GswParams = GswParamsT<Lanes>;
void launch_regev_to_gsw(const GswParams& p, hipStream_t s);
// both conversion products in one launch when the record-writing ScalToMat applies (else the two launches)
void launch_convert_products(const Scal2MatParams& sp, const GswParams& gp, hipStream_t s);
// the same key from the reference's reoriented (z, r, m) packed matrices (reorient_Q, src/spiral.cpp:388)
void launch_fold_key_from_reoriented(const uint64_t* q_re, const uint64_t* qneg_re, uint64_t* key, uint32_t m2, hipStream_t s);

// ---- first-dimension sweep (sweep.hip) -----------------------------------------------------------------
// device DB layout: common.h (packed 7-byte words for real geometries, plain for tiny ones), ic = ii*2 + c, nic = 2*num_per.
// acc[ii][r][c][z] PK (fields < m).
// g_log: log2 of the number of ranks of a distributed fold (accumulators grouped by ii mod 2^g_log), 0 = natural order
// k_log: log2 of the number of STAGES of a pipelined sweep (0 = one): the accumulators are laid out [stage][rank][ct] so that every
// stage's block can be reduce-scattered on its own (sweep.hip acc_pos); stage >= 0 launches only that stage's column blocks
// (wide packed geometries, sweep_stages_ok), stage < 0 all of them
void launch_sweep(const uint64_t* db, const uint32_t* qs, uint64_t* acc, uint32_t num_per, uint32_t jm_total, uint32_t g_log, hipStream_t s, uint32_t k_log = 0,
                  int stage = -1);
bool sweep_stages_ok(uint32_t num_per, uint32_t jm_total, uint32_t g_log, uint32_t k_log);
// n = 2 .. kSweepMaxBatch queries against one pass over the database (records qs[b] -> accumulators acc[b]); only where
// sweep_batch_ok (the packed layout with at least 64 output columns: every published geometry but the smallest streaming ones)
constexpr uint32_t kSweepMaxBatch = 2;
bool sweep_batch_ok(uint32_t num_per, uint32_t jm_total);
// g_extra > 0: the rank-major accumulators of a batch of a sharded answer -- acc[b] is query b's first chunk of a caller's [rank][lane][k < num_per / G]
// buffer, and rank g's chunk of it is g * g_extra ciphertexts further on than in the one-query layout (g_extra = (lanes - 1) * num_per / G)
void launch_sweep_batch(const uint64_t* db, const uint32_t* const* qs, uint64_t* const* acc, uint32_t n, uint32_t num_per, uint32_t jm_total, uint32_t g_log,
                        hipStream_t s, uint32_t g_extra = 0);
// the same on the matrix cores for n = 1 .. kMaxLanes queries per pass (sweep_mfma.hip): needs the "limb plane" image of the database, built
// from the packed one by launch_db_limb_planes (as many words); where sweep_mfma_ok (>= 8 ciphertexts per slot, first dimension a power of two in
// [64, 2048]; whether an image of fewer than 64 ciphertexts per slot takes the form is option sweep_narrow, DbLayout::limbs_ok).  Returns the launch's error (the > 64 KiB LDS opt-in is per device).  k_log: the accumulators' stage layout, as launch_sweep
bool sweep_mfma_ok(uint32_t num_per, uint32_t jm_total);
// nz slots z (both pointers at the first of them; a slot's region is db_device_words / kN words in either form, so a server converts its image IN PLACE
// a few slots at a time through a staging buffer); launch_db_limb_unplanes is the inverse map (limb planes -> packed), bit-exact both ways
void launch_db_limb_planes(const uint64_t* db_packed_img, uint64_t* db_limbs, uint32_t num_per, uint32_t jm_total, hipStream_t s, uint32_t nz = kN);
void launch_db_limb_unplanes(const uint64_t* db_limbs, uint64_t* db_packed_img, uint32_t num_per, uint32_t jm_total, hipStream_t s, uint32_t nz = kN);
// g_extra: the rank-major batch layout, as launch_sweep_batch (k_log = 0 then)
hipError_t launch_sweep_mfma(const uint64_t* db_limbs, const uint32_t* const* qs, uint64_t* const* acc, uint32_t n, uint32_t num_per, uint32_t jm_total, uint32_t g_log,
                             hipStream_t s, uint32_t k_log = 0, uint32_t g_extra = 0);
// the launch_sweep_mfma / launch_sweep1_mfma calls of this process that returned hipSuccess (get_option "mfma_sweeps"; primitives.cpp).  Host launch calls:
// one made under stream capture counts once, a replay of the captured graph counts nothing
extern std::atomic<uint64_t> g_mfma_sweeps;
// reference DB layout (src/spiral.cpp:1139-1153) -> device layout, for the j-range [j0, j0 + dim0_shard): db_ref holds the nz
// consecutive z slabs z0 .. z0+nz-1, db_dev is the base of the shard's device database
// (col0, col_step: the image's column ii is the reference's column col0 + col_step * ii, of col_step * num_per: a column shard's)
void launch_db_relayout(const uint64_t* db_ref, uint64_t* db_dev, uint32_t num_per, uint32_t dim0, uint32_t j0, uint32_t dim0_shard, uint32_t z0,
                        uint32_t nz, hipStream_t s, uint32_t col0 = 0, uint32_t col_step = 1);
// reference reorientCiphertexts layout (z, j, m, r_pad4) u64 -> sweep query records
void launch_qs_from_reoriented(const uint64_t* reoriented, uint32_t* qs, uint32_t jm_total, hipStream_t s);
void launch_fill_db_random(uint64_t* db_dev, uint32_t num_per, uint32_t dim0_shard, uint64_t seed, hipStream_t s);
// read the device database back in the reference's layouts (tests, spiral_gpu_server_read_db_*): one plaintext item
// (j local to the shard) as n0 x n2 reference NTT-form polynomials, or nz slabs z0.. of load_db's layout restricted to
// the shard's j-range (z in the reference's slot order)
// limbs: the image is in limb-plane form (sweep_mfma.hip) instead of the packed one
void launch_db_read_item(const uint64_t* db_dev, uint64_t* out_ref, uint32_t num_per, uint32_t dim0_shard, uint32_t j_local, uint32_t ii, hipStream_t s,
                         bool limbs = false);
// (restricted to the n_ii plaintext columns ii0 .. ii0 + n_ii - 1: the same layout with num_per = n_ii)
void launch_db_read_slots(const uint64_t* db_dev, uint64_t* out, uint32_t num_per, uint32_t dim0_shard, uint32_t z0, uint32_t nz, uint32_t ii0, uint32_t n_ii,
                          hipStream_t s, bool limbs = false);
void launch_fill_db1_random(uint64_t* db_dev, uint32_t num_per, uint32_t dim0, uint64_t seed, hipStream_t s);
// the GSW-bit ciphertexts (odd slots 2 i + 1 of cv, i < n_bits) a rank of a G-rank answer expanded itself (i = a G + rank) <->
// its block of the all-gather buffer [rank][a < n_max][2 polynomials]; pack: cv -> this rank's block, unpack: all blocks -> cv
void launch_gsw_bits_pack(const uint64_t* cv, uint64_t* block, uint32_t rank, uint32_t n_ranks, uint32_t n_bits, hipStream_t s);
void launch_gsw_bits_unpack(uint64_t* cv, const uint64_t* gathered, uint32_t n_ranks, uint32_t n_bits, hipStream_t s);
// the same for the query lanes of a batch (gridDim.z = lanes.n; cv per lane): pack writes lane q's block to block + q * words, unpack reads rank r's
// block of lane q at gathered + (r * lanes.n + q) * words -- one all-gather of the [lane][words] blocks gives that [rank][lane][words] layout
void launch_gsw_bits_pack_lanes(const uint64_t* cv, uint64_t* block, uint32_t rank, uint32_t n_ranks, uint32_t n_bits, const Lanes& lanes, hipStream_t s);
void launch_gsw_bits_unpack_lanes(uint64_t* cv, const uint64_t* gathered, uint32_t n_ranks, uint32_t n_bits, const Lanes& lanes, hipStream_t s);

// ---- SpiralPack (pack.hip; reference src/testing.cpp) -----------------------------------------------------------
// device DB layout, 1 x 1 plaintexts.  Packed (dim0 % 16 == 0; as the base path's, common.h): a word is two 28-bit
// residues in 7 bytes; a lane's 16 words of 16 consecutive j are one 112-byte string fetched as 7 x 16 bytes:
//     tile -> group j/16 -> chunk k < 7 -> lane -> 16 bytes,
// a tile being W = min(64, num_per) columns x P = 64/W consecutive slots z, lane = (z % P) * W + ii % W.
// Plain (dim0 < 16, tiny geometries): word(z, j, ii) at (((z*nblk + ii/W)*(dim0/2) + j/2)*W + ii%W)*2 + (j&1)
__host__ __device__ inline size_t db1_word_index(uint32_t z, uint32_t j, uint32_t ii, uint32_t num_per, uint32_t dim0) {
    const uint32_t w = num_per < 64u ? num_per : 64u, nblk = num_per / w;
    return ((((size_t)z * nblk + ii / w) * (dim0 / 2) + (j >> 1)) * w + ii % w) * 2u + (j & 1u);
}
__host__ __device__ inline bool db1_packed(uint32_t num_per, uint32_t dim0) { return (dim0 & 15u) == 0u && num_per >= 1u && (num_per & (num_per - 1u)) == 0u; }
__host__ __device__ inline size_t db1_device_words(uint32_t num_per, uint32_t dim0) {  // u64 words per trial
    const size_t words = (size_t)kN * dim0 * num_per;
    return db1_packed(num_per, dim0) ? words / 8u * 7u : words;
}
__host__ __device__ inline size_t db1_packed_byte(uint32_t z, uint32_t j, uint32_t ii, uint32_t by, uint32_t num_per, uint32_t dim0) {
    const uint32_t w = num_per < 64u ? num_per : 64u, pz = 64u / w, nblk = num_per / w;
    const uint32_t tile = (z / pz) * nblk + ii / w, lane = (z % pz) * w + ii % w, b = 7u * (j & 15u) + by;
    return ((((size_t)tile * (dim0 >> 4) + (j >> 4)) * 7u + (b >> 4)) * 64u + lane) * 16u + (b & 15u);
}
#ifdef __HIPCC__
__device__ __forceinline__ void db1_put_word(uint64_t* db, uint32_t z, uint32_t j, uint32_t ii, uint32_t num_per, uint32_t dim0, uint64_t v) {
    if (db1_packed(num_per, dim0)) {
        const uint64_t f = (uint64_t)(uint32_t)v | ((uint64_t)(uint32_t)(v >> 32) << 28);
        uint8_t* bytes = reinterpret_cast<uint8_t*>(db);
#pragma unroll
        for (uint32_t by = 0; by < 7; by++) bytes[db1_packed_byte(z, j, ii, by, num_per, dim0)] = (uint8_t)(f >> (8u * by));
    } else {
        db[db1_word_index(z, j, ii, num_per, dim0)] = v;
    }
}
// read one word of a trial image back (the inverse of db1_put_word): the packed and the plain layout
__device__ __forceinline__ uint64_t db1_get_word(const uint64_t* db, uint32_t z, uint32_t j, uint32_t ii, uint32_t num_per, uint32_t dim0) {
    if (db1_packed(num_per, dim0)) {
        const uint8_t* bytes = reinterpret_cast<const uint8_t*>(db);
        uint64_t f = 0;
#pragma unroll
        for (uint32_t by = 0; by < 7; by++) f |= (uint64_t)bytes[db1_packed_byte(z, j, ii, by, num_per, dim0)] << (8u * by);
        return (f & 0xFFFFFFFull) | ((f >> 28) << 32);
    }
    return db[db1_word_index(z, j, ii, num_per, dim0)];
}
// The same word from the limb-plane form of a trial image (sweep_mfma.hip, db_update.hip; common.h db_get_word_limbs with columns ii and terms
// k = j): [z][16 columns][prime][piece of 128 terms][7 planes], chunk c = (j & 127) >> 6, lane = (((j & 127) >> 4) & 3) * LW + column, byte j & 15.
// PLANE = 1024 (LW = 16: the wide and the narrow form, num_per >= 16) or 512 (LW = 8, one column block per slot: the pair form, num_per = 8).
template <uint32_t PLANE>
__device__ __forceinline__ uint64_t db1_get_word_planes(const uint64_t* db, uint32_t z, uint32_t j, uint32_t ii, uint32_t num_per, uint32_t dim0) {
    constexpr uint32_t LW = PLANE / 64u;
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(db);
    const uint32_t nk2 = dim0 >> 7, t = j & 127u, c = t >> 6, lane = ((t >> 4) & 3u) * LW + (ii & (LW - 1u)), e = t & 15u;
    const uint32_t nblk = PLANE == 512u ? 1u : num_per >> 4, blk = PLANE == 512u ? 0u : ii >> 4;
    uint32_t res[2];
#pragma unroll
    for (uint32_t pr = 0; pr < 2; pr++) {
        const size_t piece = (((size_t)z * nblk + blk) * 2u + pr) * nk2 + (j >> 7);  // 7 planes each
        const uint8_t* b = bytes + piece * (7u * PLANE) + (size_t)lane * 16u + e;
        uint32_t w = 0;
#pragma unroll
        for (uint32_t i = 0; i < 3; i++) w |= (uint32_t)(b[(2u * i + c) * PLANE] ^ 0x80u) << (8u * i);
        w |= ((uint32_t)(b[6u * PLANE] >> (4u * c)) & 0xFu) << 24;
        const int32_t a = (int32_t)w - 0x808080;
        res[pr] = a < 0 ? (uint32_t)(a + (int32_t)(pr ? kB : kP)) : (uint32_t)a;
    }
    return (uint64_t)res[0] | ((uint64_t)res[1] << 32);
}
__device__ __forceinline__ uint64_t db1_get_word_limbs(const uint64_t* db, uint32_t z, uint32_t j, uint32_t ii, uint32_t num_per, uint32_t dim0) {
    return db1_get_word_planes<1024u>(db, z, j, ii, num_per, dim0);
}
__device__ __forceinline__ uint64_t db1_get_word_limbs8(const uint64_t* db, uint32_t z, uint32_t j, uint32_t ii, uint32_t dim0) {
    return db1_get_word_planes<512u>(db, z, j, ii, 8u, dim0);
}
#endif
// fastMultiplyQueryByDatabaseDim1 (src/testing.cpp:364): acc[ii][r][z] PK; qs1 records [z][j] = {p r0, p r1, b r0, b r1}
// `trials` databases db + t*db_stride swept in one launch into acc + t*acc_stride (strides in u64 words)
void launch_sweep1(const uint64_t* db, const uint32_t* qs1, uint64_t* acc, uint32_t num_per, uint32_t dim0, uint32_t trials, size_t db_stride,
                   size_t acc_stride, hipStream_t s);
// query records from the expanded cts: first-dimension ct j is cv[j * idx_factor] (reorientCiphertextsDim1, :342)
// (lanes, here and below: gridDim.z = the clients of a batch, every pointer lane 0's -- kernels.h Lanes; qs1 is shifted by the same bytes)
void launch_qs1_from_cv(const uint64_t* cv, uint32_t* qs1, uint32_t dim0, uint32_t idx_factor, hipStream_t s, const Lanes& lanes = Lanes{});
void launch_qs1_from_reoriented(const uint64_t* re, uint32_t* qs1, uint32_t dim0, hipStream_t s);
// convertDb layout (:316-340) z*(num_per*dim0) + ii*dim0 + j -> device layout
// foldCiphertextsDim1 product for `count` ciphertexts: out[b][2] = key[2][K] * d[b][K]   (src/testing.cpp:596-624)
// key_stride: polynomials between the key's two rows (0 = K); addend (pair form: out = L + F * D'): PK ciphertexts, ciphertext b = t * np + i at
// polynomial (t * add_stride + i) * 2 + r of `addend`.  lanes: `count` ciphertexts per lane, each lane with its own key
void launch_pack_fold_mac(const uint64_t* key, const uint64_t* d, uint64_t* out, uint32_t K, uint32_t count, hipStream_t s, uint32_t key_stride = 0,
                          const uint64_t* addend = nullptr, uint32_t np = 1, uint32_t add_stride = 1, const Lanes& lanes = Lanes{});
void launch_db1_relayout(const uint64_t* ref, uint64_t* dev, uint32_t num_per, uint32_t dim0, hipStream_t s);
// gsw[i][r][2j] = tmp[i*ell+j][r], gsw[i][r][2j+1] = cv[2*(i*ell+j)+1][r]   (regevToSimpleGsw, :108-139)
void launch_pack_gsw_assemble(const uint64_t* tmp, const uint64_t* cv, uint64_t* gsw, uint32_t ell, uint32_t nu2, hipStream_t s, const Lanes& lanes = Lanes{});
void launch_pack_gsw_from_upload(const uint64_t* query, uint64_t* gsw, uint32_t dim0, uint32_t ell, uint32_t nu2, hipStream_t s, const Lanes& lanes = Lanes{});
// key[cur][r][0..2ell) = gadget - F, [2ell..4ell) = F with F = gsw[nu2-1-cur]   (:1027-1032, 611-618)
void launch_pack_fold_key(const uint64_t* gsw, uint64_t* key, uint32_t ell, uint32_t nu2, hipStream_t s, const Lanes& lanes = Lanes{});
// pack (:198-241): result[row][c] = sum_r sum_k W_r[row][k] * ginv[r*out_n+c][k] + (row >= 1 ? ct2[(row-1)*out_n+c] : 0)
// n_inst > 1: n_inst such products in one launch (an item group of answer_batch_instances), instance k's ginv / ct2 / result k x (out_n^2 t_conv,
// out_n^2, (out_n + 1) out_n) polynomials further on, the same v_w.  lanes (n_inst = 1 only): one response per client, each with its own v_w
void launch_pack_mac(const uint64_t* v_w, const uint64_t* ginv, const uint64_t* ct2, uint64_t* result, uint32_t out_n, uint32_t t_conv, hipStream_t s,
                     uint32_t n_inst = 1, const Lanes& lanes = Lanes{});
// The folded ciphertexts of a trial-sharded batch, regrouped for the pack in ONE launch (pack_gathered_batch): src holds n_ranks blocks at a stride of
// block_cts ciphertexts (2 x 2048 raw words each), block r = [lane][k < cuts[r + 1] - cuts[r]] of the trials [cuts[r], cuts[r + 1]); lane q's trial t
// goes to dst + lanes.off[q] + t x 2 x 2048 words -- trial order, in the lane's own arena, where run_pack's readers take it with the same lanes.  cuts[0]
// = 0 < ... < cuts[n_ranks] = trials <= kMaxPackTrials (the host checks); the padding of a block is never read.  src is 16-byte aligned.
constexpr uint32_t kMaxPackTrials = 256;  // out_n <= 16
struct PackRegroupParams {
    const uint64_t* src;
    uint64_t* dst;
    uint64_t block_cts;
    uint32_t n_ranks;
    uint32_t cuts[kMaxPackTrials + 1];
    Lanes lanes;
};
void launch_pack_regroup(const PackRegroupParams& p, uint32_t trials, hipStream_t s);
// the first-dimension sweep of n = 1 .. kMaxLanes queries (records qs1[b] -> accumulators acc[b], launch_sweep1's layouts) on the matrix cores, in ONE
// pass over `trials` trial images (db_stride / acc_stride u64 words apart) in limb-plane form (sweep_mfma.hip, ROWS = 2).  Coverage (sweep1_mfma_ok):
// num_per 8 (the pair form: a wave's operand holds two adjacent trials), 16, 32, 64 (the narrow form: a workgroup's waves take blocks of different
// trials) or a power of two >= 128, dim0 a power of two in [128, 4096], any trials >= 1.  Bit-identical to sweep1_kernel per query.  Returns the launch's
// error.  (sweep1_mfma_ok says what the kernels can sweep; whether an 8-column image takes the form is option pack_pair_blocks, DbLayout::limbs_ok.)
bool sweep1_mfma_ok(uint32_t num_per, uint32_t dim0);
hipError_t launch_sweep1_mfma(const uint64_t* db_limbs, const uint32_t* const* qs1, uint64_t* const* acc, uint32_t n, uint32_t num_per, uint32_t dim0, uint32_t trials,
                              size_t db_stride, size_t acc_stride, hipStream_t s);
// packed trial image <-> limb planes for nz slots z (pointers at the first of them; a slot's region, db1_device_words / kN words, is the same in both
// forms): the base path's conversion kernels, with nic = num_per columns and dim0 terms per column (num_per = 8: their 8-column twins, 512-byte planes).
// num_per < 64: a packed tile holds 64 / num_per slots, so both pointers must be at a multiple of that many slots and nz a multiple of it
void launch_db1_limb_planes(const uint64_t* packed_img, uint64_t* limbs, uint32_t num_per, uint32_t dim0, hipStream_t s, uint32_t nz);
void launch_db1_limb_unplanes(const uint64_t* limbs, uint64_t* packed_img, uint32_t num_per, uint32_t dim0, hipStream_t s, uint32_t nz);

// ---- in-place item update (db_update.hip) ---------------------------------------------------------------------------------
// Scatters encoded items into an image in packed form and / or in limb-plane form, in ONE launch.  enc: the items' words as the ingest transform
// leaves them with a linear ST_PK store (LD_DBGEN: 4 polynomials per item, LD_DBGEN1: 1), word z of a polynomial = database slot z.  Nothing is
// written when *err != 0.  Work entries (built and checked on the host; no two entries may name the same item, pair or column-term):
//   put:   {encoded item, j local to the image, column ii, 0}, one per item, packed form
//   pairs: {column ii, j of the low partner (bit 5 of j clear on the base path, bit 6 on SpiralPack), encoded item of the low partner, of the high
//          partner (j + 32 / j + 64)}, kDbUpdateNone where that partner does not change; limb-plane form
constexpr uint32_t kDbUpdateNone = 0xFFFFFFFFu;
struct DbUpdateParams {
    const uint64_t* enc;
    const uint32_t* err;
    uint64_t* packed;  // the image in packed form (null: none)
    uint64_t* limbs;   // the image in limb-plane form (null: none)
    const uint4* put;
    const uint4* pairs;
    uint32_t n_put, n_pairs;
    uint32_t pack;           // 0: a base image (columns ic = 2 ii + c, terms 2 j + m), 1: a SpiralPack trial image (columns ii, terms j)
    uint32_t num_per, dim0;  // the image's geometry (dim0: the shard's first dimension on the base path)
};
void launch_db_update(const DbUpdateParams& p, hipStream_t s);
// The same scatter over the trial images of a SpiralPack server in ONE launch (update_records): u.pack = 1, u.packed / u.limbs are trial image 0's and
// trial t's lies t * trial_words words further on.  An encoded item is one polynomial, and the work entries carry its trial:
//   put:   {encoded polynomial, j, column ii, trial}
//   pairs: {column ii | trial << kPackRecordTrialShift, j of the low partner (bit 6 clear), encoded polynomial of the low partner, of the high partner}
constexpr uint32_t kPackRecordTrialShift = 24, kPackRecordColMask = (1u << kPackRecordTrialShift) - 1u;  // trials <= kMaxPackTrials = 2^8
struct DbUpdateTrialsParams {
    DbUpdateParams u;
    uint64_t trial_words;
};
void launch_db_update_trials(const DbUpdateTrialsParams& p, hipStream_t s);

// ---- items out of the image as plaintexts (db_export.hip) -------------------------------------------------------------------
// The inverse of the ingest (LD_DBGEN / LD_DBGEN1 with ST_DB / ST_DB1): one workgroup per polynomial gathers its 2048 words from the image in the
// form it is in, inverse transform + CRT lift, undoes the centred lift and bit-packs the coefficients coeff_bits wide (the item stream of
// load_db_items).  Item k of the launch goes to out + k * polys * 256 * coeff_bits bytes, polys = 4 (base: polynomial (m, c) at m * 2 + c) or 1.
// The work is either the n consecutive LOCAL items first .. first + n - 1 (local: j counted from the shard's first row, item = j * num_per + ii) or,
// table != null, the n entries {j local, column ii, output slot k, position in the call} of a device table.  A coefficient that is no centred
// lift of a value below p_db atomicMin's ((position in the call * polys + polynomial) * 2048 + coefficient) into *err (range form: position =
// pos_base + k), which the host sets to ~0 before the first launch of a call.
enum DbExportForm : uint32_t {
    DBX_PACKED = 0,  // db_get_word / db1_get_word: the packed and the plain layouts
    DBX_LIMBS = 1,   // db_get_word_limbs / db1_get_word_limbs: 1 KiB planes
    DBX_LIMBS8 = 2,  // db1_get_word_limbs8: a SpiralPack image of 8 columns, 512-byte planes
};
struct DbExportParams {
    const uint64_t* db;  // the image (SpiralPack: the trial's)
    uint8_t* out;        // 16-byte aligned
    unsigned long long* err;
    const uint4* table;
    uint64_t first, pos_base;
    uint32_t n;
    uint32_t pack, form;        // pack: 1 x 1 plaintexts of a trial image; form: DbExportForm
    uint32_t num_per, dim0;     // the image's geometry (dim0: the shard's first dimension on the base path)
    uint32_t coeff_bits;        // 1 .. 64, 2^coeff_bits >= p_db
    uint64_t p_db;
};
void launch_db_export(const DeviceTables& t, const DbExportParams& p, hipStream_t s);

// ---- content fingerprints of the image (db_fingerprint.hip; the definition: include/spiral_gpu.h "Fingerprints") -----------------------------
// The export's work selection (a range of LOCAL items, or a table {j local, column ii, slot in the pass, position in the call}), gather, inverse
// transform and error word, with one 8-byte word per polynomial in place of the item stream: part[slot * npolys + q] = sum over c of
// x_c r^(c + 1) mod P for polynomial q of the npolys this server holds of an item -- base: npolys = 4, q = 2 m + c; SpiralPack: its nt trial images,
// image q at db + q * trial_words.  weights: the table of fingerprint_math.h fp_build_weights.  The error word takes
// ((position in the call * npolys + q) * 2048 + coefficient).
struct DbFingerprintParams {
    const uint64_t* db;
    uint64_t trial_words;
    const uint64_t* weights;
    uint64_t* part;
    unsigned long long* err;
    const uint4* table;
    uint64_t first, pos_base;
    uint32_t n;
    uint32_t pack, form;     // as DbExportParams
    uint32_t num_per, dim0;  // the image's geometry (dim0: the shard's first dimension on the base path)
    uint32_t npolys;
    uint64_t p_db;
};
void launch_db_fingerprint(const DeviceTables& t, const DbFingerprintParams& p, hipStream_t s);
// The pass's second launch: f of item k = sum over q of part[k * npolys + q] r^(2048 (poly0 + q)) to item_f[k * out_stride] (item_f null: not wanted;
// the out_stride - 1 words behind it, below out_words, are zeroed: items a column shard does not hold), and f s^(i + 1) -- i = ids[k], or
// idx0 + k * idx_stride with ids null -- summed into sums[0 .. kFpSumWords), which ACCUMULATE from pass to pass.
constexpr uint32_t kFpSumWords = 256;
struct DbFingerprintCombineParams {
    const uint64_t* part;
    const uint64_t* weights;
    const uint64_t* ids;
    uint64_t idx0, idx_stride;
    uint64_t* item_f;
    uint64_t out_stride, out_words;
    uint64_t* sums;
    uint64_t n;
    uint32_t npolys, poly0;
};
void launch_db_fingerprint_combine(const DbFingerprintCombineParams& p, hipStream_t s);

// ---- tracked fingerprints (db_track.hip; include/spiral_gpu.h "Fingerprints", Tracked) ------------------------------------------------------
// The resident table holds g(i, q) = sum over c of x_c r^(c + 1) mod P, the word db_fingerprint_kernel stores, for every (local item, polynomial held):
// word (local item) * npolys + q.  An in-place update computes the new words without reading the image, then replaces them and moves F by the difference.
// All three kernels below return at once when *err != 0 (the update's error word or flag, as db_update_kernel).
//
// g of polynomial k of a staged raw item stream (update_db_items' `d + o_items`): gnew[k] from the 2048 coeff_bits-wide coefficients at
// k * 2048 on (common.h packed_coeff: widths 1..40 and 64; the staging buffer's 16 bytes of over-read room).  One workgroup per polynomial.
struct FpStreamParams {
    const uint8_t* items;
    const uint64_t* weights;  // fingerprint_math.h fp_build_weights
    uint64_t* gnew;
    const uint32_t* err;
    uint32_t n_polys, coeff_bits;
};
void launch_fingerprint_stream(const FpStreamParams& p, hipStream_t s);
// Entry k = {database index i of the item (kFpApplySkip: nothing to do, a polynomial no record touches), table word << 8 | polynomial q of the item}:
// delta = (gnew[k] - table[word]) r^(2048 q) s^(i + 1), table[word] = gnew[k], and the workgroup's sum of deltas is ADDED to sums[blockIdx.x]
// (db_fingerprint_combine_kernel's pattern: launches on one stream are ordered).  No two entries of a launch name the same word.
constexpr uint64_t kFpApplySkip = ~0ull;
struct FpApplyParams {
    const ulonglong2* entries;
    const uint64_t* gnew;
    uint64_t* table;
    const uint64_t* weights;
    uint64_t* sums;
    const uint32_t* err;
    uint32_t n;
};
void launch_fingerprint_apply(const FpApplyParams& p, hipStream_t s);
// A scrub pass: word w of the n_words recomputed words `part` (item k = w / npolys of the pass, polynomial q = w % npolys) against table[w]; a mismatch
// adds 1 to out[0] and atomicMin's (database index idx0 + k idx_stride) * 256 + poly0 + q into out[1], which the host sets to 0 and ~0 before a call.
struct FpCompareParams {
    const uint64_t* part;
    const uint64_t* table;
    unsigned long long* out;
    uint64_t n_words, idx0, idx_stride;
    uint32_t npolys, poly0;
};
void launch_fingerprint_compare(const FpCompareParams& p, hipStream_t s);

// ---- records (records.hip; the layout: include/spiral_gpu.h "Records") --------------------------------------------------------
// Work at a record's own granularity on a base image, one workgroup per polynomial.  A record (or its chunk of one instance) is a byte range of its
// item's stream; cut at the polynomial boundaries it is a few SEGMENTS, each a byte range of one polynomial's 256 w byte stream (w = bits per
// coefficient) and a byte range of `buf`, the staging buffer: staged record k at k * stride.  The host builds the two tables:
//   entries: {j local to the image (bits 0..16) | polynomial mc (24..25) | kRecordFull (bit 28), column ii, first segment, segments}: the segment count
//            has a word of its own -- a read may name one record any number of times (ids need not be distinct), a segment each
//   segs:    {byte offset in the polynomial's stream, bytes, byte offset in buf (low, high word)}
// A coefficient that cannot be part of a record -- no centred lift of a value below p_db, or a value >= 2^w inside a range that is read -- atomicMin's
// ((staged record * 4 + polynomial) * 2048 + coefficient) into *err, which the host sets to ~0 before the launch.
// read:   the entries are the touched polynomials; each gathers its words from the image in the form it is in (db_plain_device.h), and stores the
//         segments' bytes to buf.
// update: entry 4 e + mc is polynomial mc of touched item e, and its 2048 encoded words go to enc + (4 e + mc) * 2048, the linear order db_update_kernel
//         scatters from.  No segments: the image's words pass through unchanged.  kRecordFull (the segments cover the polynomial): the coefficients come
//         from buf alone.  Otherwise gather + inverse transform + unlift, splice the segments' bits over the coefficients (a coefficient that lies
//         partly inside a segment keeps its other bits), lift and transform forward.  An error also sets *flag, which makes db_update_kernel skip.
constexpr uint32_t kRecordPolyShift = 24, kRecordFull = 1u << 28, kRecordRowMask = (1u << kRecordPolyShift) - 1u;
struct RecordWorkParams {
    const uint64_t* db;  // the image in the form `form` names (DBX_PACKED or DBX_LIMBS)
    const uint4* entries;
    const uint4* segs;
    uint8_t* buf;   // read: written; update: read
    uint64_t* enc;  // update only
    unsigned long long* err;
    uint32_t* flag;  // update only
    uint32_t n_entries, form;
    uint32_t num_per, dim0;  // the image's geometry (dim0: the shard's first dimension)
    uint32_t w, stride;
    uint64_t p_db;
};
void launch_record_read(const DeviceTables& t, const RecordWorkParams& p, hipStream_t s);
void launch_record_update(const DeviceTables& t, const RecordWorkParams& p, hipStream_t s);
// The same on the trial images of a SpiralPack server (include/spiral_gpu.h "Records", SpiralPack): polynomial t of an item is the item's 1 x 1 plaintext
// in trial t, so a workgroup's polynomial is (trial, j, ii).  r.db is the first trial image the server holds (global trial `trial0`), in the form r.form
// names (DBX_PACKED, DBX_LIMBS or DBX_LIMBS8), the next ones trial_words words apart.  The tables are RecordWorkParams' with two differences:
//   entries: {j | kRecordFull, column ii | local trial << kPackRecordTrialShift, first segment, segments}
//   *err:    ((staged record * trials + global trial) * 2048 + coefficient)
// update: only touched polynomials have an entry (the scatter writes single polynomials), and entry e's words go to enc + e * 2048.
struct PackRecordWorkParams {
    RecordWorkParams r;
    uint64_t trial_words;
    uint32_t trials, trial0;
};
void launch_pack_record_read(const DeviceTables& t, const PackRecordWorkParams& p, hipStream_t s);
void launch_pack_record_update(const DeviceTables& t, const PackRecordWorkParams& p, hipStream_t s);
// The update launches on an image whose fingerprint is tracked (the TRACK instantiations; launched on such an image only): the same work, and entry e
// with segments also stores gnew[e] = sum over c of x_c r^(c + 1) mod P of the coefficients it holds after the splice (an entry without segments
// stores nothing: its table word stays).  weights: fingerprint_math.h fp_build_weights.
struct RecordTrackParams {
    const uint64_t* weights;
    uint64_t* gnew;
};
void launch_record_update_tracked(const DeviceTables& t, const RecordWorkParams& p, const RecordTrackParams& k, hipStream_t s);
void launch_pack_record_update_tracked(const DeviceTables& t, const PackRecordWorkParams& p, const RecordTrackParams& k, hipStream_t s);

// ---- keyed records: the server's probe (kv.hip; the definition: include/spiral_gpu.h "Keyed records") ------------------------------------------
// One workgroup per distinct candidate bucket of a call: polynomial 0 of the bucket's item from the image in the form it is in (db_plain_device.h),
// the header's `slots` 8-byte tags packed at w bits in LDS, then
//   occ[4 e .. 4 e + 3]: entry e's occupancy bitmap, bit s set where tag s is not 0;
//   slot_out[lookup.y]:  for each of the entry's lookups {tag, output index}, the lowest slot that holds the tag, or 0xFFFFFFFF.
// entries: {j local to the image, column ii, first lookup, lookups}, in ascending bucket order.  A coefficient that is no plaintext value, or a header
// coefficient >= 2^w, atomicMin's (entry * 2048 + coefficient) into *err, which the host sets to ~0 before the launch.
struct KvProbeParams {
    const uint64_t* db;  // the image in the form `form` names (DBX_PACKED or DBX_LIMBS)
    const uint4* entries;
    const ulonglong2* lookups;
    uint64_t* occ;
    uint32_t* slot_out;
    unsigned long long* err;
    uint32_t n_entries, form;
    uint32_t num_per, dim0;  // the image's geometry (dim0: the shard's first dimension)
    uint32_t w, slots;
    uint64_t p_db;
};
// pack: the image is trial image 0 of a SpiralPack server (polynomial 0 of a bucket is its item there), in the form DBX_PACKED, DBX_LIMBS or DBX_LIMBS8
void launch_kv_probe(const DeviceTables& t, const KvProbeParams& p, bool pack, hipStream_t s);
// Table occupancy (include/spiral_gpu.h spiral_gpu_server_kv_stats): the probe's work on buckets [first_bucket, + n_buckets) -- bucket b is image item
// (b / num_per, b % num_per), so no table is uploaded -- and one atomic add per bucket: hist[u] += 1 for a bucket with u used slots (tags that are
// not 0).  hist: 257 words, zero before the launch.  *err as for the probe, with the BUCKET in the entry's place: (bucket * 2048 + coefficient).
struct KvStatsParams {
    const uint64_t* db;  // as KvProbeParams
    unsigned long long* hist;
    unsigned long long* err;
    uint32_t first_bucket, n_buckets;  // one workgroup per bucket
    uint32_t form;
    uint32_t num_per, dim0;
    uint32_t w, slots;
    uint64_t p_db;
};
void launch_kv_stats(const DeviceTables& t, const KvStatsParams& p, bool pack, hipStream_t s);
// Listing (include/spiral_gpu.h "Listing", spiral_gpu_server_kv_scan / _kv_scan_at): one pass over n_buckets <= 2^16 buckets, three launches in stream
// order, no workgroup waits for another.  Workgroup g of the pass has bucket first + g (ids == null: the range form), or ids[first + g] (the list form:
// first is the pass's position in the list).
//   decode:  the probe's work on the bucket; stage[g * slots + s] = tag s (stage == null in a count-only call: not stored), counts[g] = tags that are not
//            0.  *err as for kv_stats with (first + g) in the bucket's place: the bucket of the range form, the POSITION of the list form.
//   offsets: ONE workgroup; offsets[g] = *total + the exclusive prefix sum of counts, then *total += the pass's sum: stream order carries the running
//            total from pass to pass.
//   compact: entry offsets[g] + (rank of slot s among the bucket's non-zero tags) = {tag, bucket, s}, where that index is below max_entries.
struct KvScanParams {
    const uint64_t* db;  // as KvProbeParams
    const uint32_t* ids;
    uint64_t* stage;
    uint32_t* counts;
    unsigned long long* offsets;
    unsigned long long* total;
    unsigned long long* err;
    ulonglong2* entries;  // spiral_gpu_kv_entry as one 16-byte store: {tag, bucket | slot << 32}
    unsigned long long max_entries;
    uint32_t first, n_buckets;
    uint32_t form;
    uint32_t num_per, dim0;
    uint32_t w, slots;
    uint64_t p_db;
};
void launch_kv_scan_decode(const DeviceTables& t, const KvScanParams& p, bool pack, hipStream_t s);
void launch_kv_scan_offsets(const KvScanParams& p, hipStream_t s);
void launch_kv_scan_compact(const KvScanParams& p, hipStream_t s);

// ---- client session (client.hip; the format: client_device.h) ---------------------------------------------------------------
// noise polynomials of n_msgs messages, `per_msg` each: polynomial j of message b is noise polynomial first + j under the 32-byte noise key keys[b]
// (device memory, 8 words per key) and domain tag `domain`.  raw[b][j][2048]: the raw values mod Q, plus addend[b][j][2048] (mod Q) where addend !=
// null -- a compressed query's e + sigma; centred (may be null): the samples themselves as 8-bit values.  table: the 128 thresholds on the device.
// nonoise: every sample is 0
void launch_client_noise(const uint32_t* keys, uint32_t domain, uint64_t first, const uint64_t* table, uint64_t* raw, int8_t* centred, const uint64_t* addend,
                         uint32_t per_msg, uint32_t n_msgs, bool nonoise, hipStream_t s);
// One column of a message's matrix: row 0 = row-0 polynomial k of the message's seed (seed_device.h), a = -row 0, and for the secret rows r = 1 ..
// rows - 1:  b_r = a S + e + c M  pointwise in PK form, with S = secret-table polynomial s_first + (r - 1), e = transformed noise polynomial noise +
// (r - 1) noise_stride of the message, and -- on row m_row alone, or on every row for m_row = 0, on none for kClientNoMessage -- the constant c (its
// residues c_p, c_b) times secret-table polynomial m_idx + (r - 1) m_stride.  Row r of the column goes to polynomial dst + r dst_stride of the message.
constexpr uint32_t kClientNoMessage = 0xFFFFFFFFu;
struct ClientColumn {
    uint32_t k, dst, dst_stride, rows;
    uint32_t s_first, noise, noise_stride;
    uint32_t m_row, m_idx, m_stride;
    uint32_t c_p, c_b;
};
struct ClientSampleParams {
    const uint32_t* seeds;        // [n_msgs][8]: the messages' public seeds
    const ClientColumn* columns;  // [n_msgs][n_cols]
    const uint64_t* table;        // the session's secret table, PK polynomials
    const uint64_t* noise;        // [n_msgs][noise_polys][2048] PK
    uint64_t* out;                // [n_msgs][msg_polys][2048] PK
    uint32_t domain, n_cols, noise_polys, msg_polys;
};
void launch_client_sample(const ClientSampleParams& p, uint32_t n_msgs, hipStream_t s);
// out = a * b pointwise, PK polynomials
void launch_client_mul(const uint64_t* a, const uint64_t* b, uint64_t* out, uint32_t npolys, hipStream_t s);
// raw coefficients (below Q) -> their 7-byte wire form, kWirePolyBytes per polynomial, densely
void launch_client_wire_encode(const uint64_t* raw, uint8_t* wire, uint32_t npolys, hipStream_t s);
// check_final's client half (src/spiral.cpp:1451-1491, src/testing.cpp:1086-1122) for n responses in ONE launch: one workgroup per output polynomial
// (response, r, col) = round((Sp_r * row 0 [col] mod q') 4p + row (1 + r)[col] q', / 4 q') mod p_db with the reference's centring and rounding.
// resp: n switched responses [(rows + 1)][cols][2048] words, or (wire) their bit-packed forms wire_words words apart (row 0 at w0 bits, the rest at
// w1), followed by one word of padding; sp: the centred rows of Sp, [rows][2048]; out: [n][rows][cols][2048] coefficients in [0, p_db).
// Exact for q' < 2^31 and |secret| <= 64: the 64-bit sums stay below 2048 * 64 * 2^31.
struct ClientDecodeParams {
    const int8_t* sp;
    const uint64_t* resp;
    uint64_t* out;
    uint32_t rows, cols;
    uint32_t wire, w0, w1;
    uint64_t wire_words;
    uint64_t qprime, p_db;
};
void launch_client_decode(const ClientDecodeParams& p, uint32_t n, hipStream_t s);
// The decode at a record's granularity (include/spiral_gpu.h "Records", spiral_gpu_client_decode_records): one workgroup per output polynomial a record
// touches, the decode's operands, convolution and rounding, then only the record's bytes of the polynomial's w-bit string go out.  d: the decode's
// arguments (d.out unused).  entries: {response, r | col << 8, first segment, segments}; segs as for RecordWorkParams: {byte offset in the polynomial's
// stream, bytes, byte offset in buf (low, high word)}.  A value's low w bits are packed (every value of a power-of-two p_db = 2^w).
struct ClientRecordDecodeParams {
    ClientDecodeParams d;
    const uint4* entries;
    const uint4* segs;
    uint8_t* buf;
    uint32_t w;
};
void launch_client_decode_records(const ClientRecordDecodeParams& p, uint32_t n_entries, hipStream_t s);
// The client's find of keyed records (include/spiral_gpu.h "Keyed records", spiral_gpu_client_kv_decode): ONE launch, workgroup b = 2 k + candidate
// per response.  It decodes output polynomial 0 with the decode's operands, convolution and rounding, packs the header's tags at w bits and looks
// for tags[k]; on a hit it decodes the output polynomials the slot's value bytes touch and stages the V bytes at stage + b * V.  The second of a key's
// two workgroups to finish (arrive[k], zeroed by the host) settles the key: found[k] = 0, 1 or 2 -- candidate 1 wins -- and the winner's bytes, or
// zeros, to values + k * V.  d: the decode's arguments (d.out unused).
struct ClientKvFindParams {
    ClientDecodeParams d;
    const uint64_t* tags;  // [n]
    uint8_t* stage;        // [2 n][V]
    uint32_t* hit;         // [2 n]: 1 where the response holds the tag
    uint32_t* arrive;      // [n], zero before the launch
    uint8_t* values;       // [n][V]
    uint8_t* found;        // [n]
    uint32_t w, slots, value_bytes;
};
void launch_client_kv_find(const ClientKvFindParams& p, uint32_t n_keys, hipStream_t s);
// the error e of every coefficient of n responses and its record per output polynomial (include/spiral_gpu.h, spiral_gpu_client_response_noise: the
// definition), ONE launch, one workgroup per output polynomial.  d: the decode's arguments (d.out unused); with final_form, d.resp holds n
// unswitched ciphertexts [(rows + 1)][cols][2048] of raw values mod Q and d.wire is 0.  expected: null or [n][rows][cols][2048] values below p_db;
// stats: null or [n][rows][cols][6] words; errors: null or [n][rows][cols][2048].  Exact under the decode's conditions and p_db q' < 2^57.
struct ClientResponseNoiseParams {
    ClientDecodeParams d;
    const uint64_t* expected;
    uint64_t* stats;
    int64_t* errors;
    uint32_t final_form;
};
void launch_client_response_noise(const ClientResponseNoiseParams& p, uint32_t n, hipStream_t s);

}  // namespace spiral
