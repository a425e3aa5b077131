/*
 * spiral_gpu.h -- C ABI of libspiral_gpu.so: the MI355X (gfx950) implementation of the Spiral
 * server-answer path.
 *
 * The reference (menonsamir/spiral) has no FFI or plugin interface: it is one C++ executable whose
 * server hot path is a set of free functions over caller-owned uint64_t buffers.
 * This header declares exactly those seams, so that a maintainer can replace the reference function
 * bodies with calls into this library (INTEGRATION.md shows the stubs).  Each entry point cites the
 * reference function it replaces.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 on success and a negative code on error
 *     (spiral_gpu_last_error() gives the message); the reference's error behaviour is assert/exit(1).
 *   - buffers use the REFERENCE layouts:
 *       NTT form : [rows][cols][2 limbs][2048] uint64_t residues (limb 0 mod p, limb 1 mod b), NTT slots
 *                  in the order produced by the reference's ntt_forward          (include/poly.h:24-64)
 *       raw form : [rows][cols][2048] uint64_t in [0, Q]
 *     any re-layout (packed u32 limb pairs, lane-major database) is internal to the library.
 *   - "host" entry points take host pointers and copy; the *_server_* stage entry points keep all
 *     state resident in HBM and are asynchronous on the server's HIP stream.
 *   - there is no CPU fallback: without a usable gfx950 device every compute entry point fails.
 */
#ifndef SPIRAL_GPU_H
#define SPIRAL_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPIRAL_GPU_ABI_VERSION 1

/* Scheme parameters = the reference's compile-time -D values (include/values.h:78-93,
 * select_params.py:337) plus argv[1], argv[2] (src/spiral.cpp:1243-1244). */
typedef struct spiral_gpu_params {
    uint32_t nu1;           /* num_expansions: first dimension is 2^nu1                          */
    uint32_t nu2;           /* further_dims:   2^nu2 plaintexts per first-dimension index        */
    uint32_t t_gsw;         /* TGSW   */
    uint32_t t_conv;        /* TCONV  */
    uint32_t t_exp;         /* TEXP   */
    uint32_t t_exp_right;   /* TEXPRIGHT */
    uint32_t qprime_bits;   /* QPBITS */
    uint32_t direct_upload; /* 0: QNUMFIRST=1, QNUMREST=0;  1: QNUMFIRST=2^nu1, QNUMREST=t_gsw*nu2 */
    uint64_t p_db;          /* PVALUE */
} spiral_gpu_params;

/* sizes derived from the parameters (src/spiral.cpp:2046-2085) */
typedef struct spiral_gpu_shape {
    uint32_t dim0, num_per, ell, m2, g, stopround;
    uint32_t n_left;      /* W_exp_left matrices  (n0 x t_exp each)       */
    uint32_t n_right;     /* W_exp_right matrices (n0 x t_exp_right each) */
    uint32_t n_query_cts; /* Regev ciphertexts (n0 x 1) in the query       */
    uint32_t n_bits;      /* dim0 + ell*nu2 expanded ciphertexts           */
    uint64_t qprime;
} spiral_gpu_shape;

typedef struct spiral_gpu_server spiral_gpu_server;

int spiral_gpu_abi_version(void);
const char *spiral_gpu_last_error(void);
int spiral_gpu_device_count(void);
int spiral_gpu_get_shape(const spiral_gpu_params *p, spiral_gpu_shape *out);
/* 1 when a server of these parameters on the first-dimension shard [j_begin, j_end) ((0, 0): the whole first dimension) may hold its database in the
 * LIMBS form (spiral_gpu_server_set_db_format below), so that a batch shares one matrix-core pass over it and collecting clients into a batch pays;
 * 0 when not; -1 (spiral_gpu_last_error) for bad parameters or a bad shard.  A function of the parameters and of ONE option, "sweep_narrow" as it
 * is when asked (fewer than 64 ciphertexts per slot only), no GPU needed.  The SpiralPack twin is spiral_gpu_pack_has_limb_form. */
int spiral_gpu_has_limb_form(const spiral_gpu_params *p, uint32_t j_begin, uint32_t j_end);
/* The same for the image of a column shard (spiral_gpu_server_create_column_shard): num_per / n_ranks ciphertexts per slot and the whole first
 * dimension -- the answer of spiral_gpu_has_limb_form for the parameters with nu2 - log2 n_ranks, the same rule and the same option "sweep_narrow",
 * read now.  Host only.  A rank count that gives no shard (not a power of two, fewer columns per shard than a shard needs) has no image: 0, and
 * spiral_gpu_last_error says why; -1 for a null or invalid parameter set. */
int spiral_gpu_column_shard_has_limb_form(const spiral_gpu_params *p, uint32_t n_ranks);

/* Process-wide options: schedule forms that compute the same function (the reference has one form of each: its own loops).  A server takes
 * the values in force when it is created; "fwd2" and "db_stage_bytes" apply to every later call.  Unknown names fail.
 *   "fold_pair"       1 (default) foldOneFurtherDimension as C[i] + Q * NTT(G^-1(C[np+i]) - G^-1(C[i])); 0 the reference's two products
 *                     (src/spiral.cpp:1349-1410).  Initial value: environment variable SPIRAL_FOLD_PAIR.
 *   "fold_chain"      1 (default) the two-product form lifts inside its digit transforms; 0 separate lift and digit launches
 *   "fold_blocks"     workgroups a two-product round aims for when it splits a polynomial's digits over workgroups (default 768)
 *   "sweep_mfma_min"  batches of at least this many queries sweep on the matrix cores (default 2; 0 = never).  Initial value: SPIRAL_SWEEP_MFMA.
 *   "one_image"       1 (default) a server that batches on the matrix cores keeps ONE image of its database and converts it in place between the
 *                     packed and the limb-plane form (spiral_gpu_server_set_db_format); 0 = a second image beside the first
 *   "fwd2"            -1 (default) the two-digits-per-workgroup transform kernel from "fwd2_min" transforms per launch; 0 never; 1 always
 *   "fwd2_min"        that threshold (default 8192 transforms per launch, all query lanes together)
 *   "db_stage_bytes"  bytes of the staging buffer of load_db / load_db_items / read_db_items (default 64 MiB).  Initial value: SPIRAL_DB_STAGE_BYTES.
 *   "pack_item_group" instances per group of spiral_gpu_pack_server_answer_batch_instances (default 0: automatic; g: at most g)
 *   "pack_batch_lanes" 0 .. 8 (default 0 = never: opt-in): the smallest number of clients from which spiral_gpu_pack_server_answer_batch and
 *                     ..._answer_batch_instances (and their _wire / _seeded forms) take the lane form -- every launch carries all clients; 0 = never.
 *                     Read per call; same results either way
 *   "pack_pair_blocks" 0 (default: opt-in) or 1: with 1 a SpiralPack geometry of exactly 8 ciphertexts per slot (nu2 = 3: the small-item sets) has a
 *                     LIMBS form too, the PAIR form of the shared pass (two adjacent trials per matrix operand).  Read where an image would TAKE that
 *                     form -- spiral_gpu_pack_has_limb_form, ..._pack_server_set_db_format(LIMBS), the automatic conversion by a batch of two or more
 *                     clients, time_sweep_batch -- and nowhere else: an image that is in the form is swept, updated, reloaded and converted back
 *                     whatever the option says now.  Same results either way
 *   "sweep_narrow"    0 (default: opt-in) or 1: with 1 a base geometry of 8, 16 or 32 ciphertexts per slot (nu2 = 3, 4, 5: the streaming sets) has a
 *                     LIMBS form too: workgroups of 1, 2, 4 waves per slot instead of 8 (csrc/sweep_mfma.hip), so a batch shares one pass over the
 *                     database where it sweeps once per lane today.  Read where an image would TAKE that form -- spiral_gpu_has_limb_form,
 *                     spiral_gpu_server_set_db_format(LIMBS), the automatic conversion by a batch, spiral_gpu_multiply_queries_by_database -- and
 *                     nowhere else: an image that is in the form is swept, updated, read, reloaded and converted back whatever the option says now.
 *                     Same results either way; not measured yet, hence opt-in
 *   "query_batch_chunk" message polynomials per lane per staging pass of spiral_gpu_server_set_query_batch for messages too large to check on the
 *                     host (direct upload); default 512, at least 1.  Read per call; same results whatever the value
 *   "kv_scan_chunk"   buckets per pass of spiral_gpu_server_kv_scan / _kv_scan_at and their SpiralPack twins: 0 (default) = automatic, the most that
 *                     keeps a pass's staged tags within 2^22 (chunk * slots <= 2^22: 32 MiB) and chunk <= 2^16; 1 .. 2^16 sets it.  Read per call; same
 *                     results whatever the value
 *   "graph_captures"  (get only) the hipGraphs the servers of this process have captured so far: a replayed call does not add to it
 *   "pack_lane_batches" (get only) the SpiralPack batch calls of this process that took the lane form
 *   "key_binds"       (get only) the lanes the bind_keys calls of this process have copied keys into (a lane that held them already is not counted)
 *   "db_export_ns"    (get only) device nanoseconds of the launches of this process's last read_db_items / read_db_items_at call, its copies excluded
 *   "db_fingerprint_ns" (get only) the same of its last fingerprint_items / fingerprint_items_at call
 *   "mfma_sweeps"     (get only) the matrix-core sweep launches (csrc/sweep_mfma.hip) this process has made: every call, batch or stage function whose
 *                     first-dimension pass took the limb-plane form adds one per pass; a replayed hipGraph adds nothing.  What tells the
 *                     matrix-core form from the vector-ALU one, whose results are the same
 * These three environment variables are the only ones the library reads. */
int spiral_gpu_set_option(const char *name, int64_t value);
int spiral_gpu_get_option(const char *name, int64_t *value);

/* ------------------------------------------------------------------------------------------------
 * L1/L2 seams: NTT core and polynomial algebra (host buffers)
 * ------------------------------------------------------------------------------------------------ */
/* the 8 x 2048 twiddle rows in the order of `tables[]`, src/constants.cpp:16 (host only, no GPU) */
int spiral_gpu_get_tables(uint64_t *out);
/* void ntt_forward(uint64_t*) / ntt_inverse(uint64_t*), src/core.cpp:247,419; batched over npolys */
int spiral_gpu_ntt_forward(uint64_t *operand, size_t npolys);
int spiral_gpu_ntt_inverse(uint64_t *operand, size_t npolys);
/* to_ntt / to_ntt_no_reduce, src/poly.cpp:311,291 : raw [npolys][N] -> NTT [npolys][2][N] */
int spiral_gpu_to_ntt(uint64_t *out, const uint64_t *in, size_t npolys, int reduce);
/* from_ntt, src/poly.cpp:357 : NTT -> raw in [0, Q) */
int spiral_gpu_from_ntt(uint64_t *out, const uint64_t *in, size_t npolys);
/* measurement helper: average duration (ms) of one batched to_ntt and one batched from_ntt launch over npolys polynomials
 * resident in HBM (HIP events, default stream): the transform kernels' cost per limb-pair transform */
int spiral_gpu_time_ntt(size_t npolys, int iters, float *fwd_ms, float *inv_ms);
/* the same for the digit-transform launch the stages are built from: n_digits gadget digits of each of npolys raw polynomials
 * (gadget_invert + to_ntt_no_reduce), npolys * n_digits transforms per launch; ms per launch */
int spiral_gpu_time_ntt_digits(size_t npolys, uint32_t n_digits, int iters, float *ms);
/* multiply, src/poly.cpp:34 : out(rs x cs) = a(rs x ms) * b(ms x cs), NTT form */
int spiral_gpu_multiply(uint64_t *out, const uint64_t *a, const uint64_t *b, size_t rs, size_t ms, size_t cs);
/* add, mul_by_const, src/poly.cpp:138,190 */
int spiral_gpu_add(uint64_t *out, const uint64_t *a, const uint64_t *b, size_t npolys);
int spiral_gpu_mul_by_const(uint64_t *out, const uint64_t *single_poly, const uint64_t *a, size_t npolys);
/* automorph, invert, src/poly.cpp:240,269 (raw form; negation is Q - a) */
int spiral_gpu_automorph(uint64_t *out, const uint64_t *in, size_t npolys, uint64_t t);
int spiral_gpu_invert(uint64_t *out, const uint64_t *in, size_t npolys);
/* gadget_invert, src/util.cpp:114 : raw [rdim][cols][N] -> raw [mx][cols][N].  A digit whose shift count k*bits is >= 64
 * is defined as 0 here (and in every fused digit loader); the reference shifts a uint64_t by that count (src/util.cpp:136),
 * which is undefined behaviour -- x86 would yield the low digit again.  Unreachable for every published parameter set
 * (k*bits < 64 for all t in all_parameter_choices.txt). */
int spiral_gpu_gadget_invert(uint64_t *out, const uint64_t *in, size_t mx, size_t rdim, size_t cols);
/* getRescaled, src/poly.cpp:593 : element-wise rescale(a % Q, inp_mod, out_mod) */
int spiral_gpu_get_rescaled(uint64_t *out, const uint64_t *in, size_t n, uint64_t inp_mod, uint64_t out_mod);

/* Wire form of a switched response [(out_n+1)][out_n][N] (base Spiral: out_n = 2): one little-endian bit stream written the way
 * write_arbitrary_bits does (src/core.cpp:32-52) along modswitch's walk over rows, columns and coefficients (src/spiral.cpp:
 * 40-76), at the two widths the summary's "Response size" assumes (src/spiral.cpp:231-233): row 0 -- the q' row -- at qprime_bits
 * per coefficient, the other rows at ceil(log2(4 p_db)) bits.  20 480 bytes instead of 98 304 at config 2.
 * spiral_gpu_response_wire_bytes: its size (0 for unsupported parameters); ..._server_read_response_wire: packs the last
 * answer's response on the device and downloads it; spiral_gpu_response_from_wire: the client's half (load_modswitched_into_ct,
 * src/client.cpp:90-110), plain host code. */
size_t spiral_gpu_response_wire_bytes(const spiral_gpu_params *p, uint32_t out_n);
int spiral_gpu_response_from_wire(const spiral_gpu_params *p, uint32_t out_n, const void *wire, uint64_t *response);

/* ------------------------------------------------------------------------------------------------
 * L5 seams: the server hot-path functions (host buffers, reference layouts)
 * ------------------------------------------------------------------------------------------------ */
/* multiplyQueryByDatabase, src/spiral.cpp:628.  reorientedCts: (z, j, m, r_pad4) packed words
 * (reorientCiphertexts, :410); database: load_db's layout (:1139-1153); output: NTT form
 * [num_per][n1][n2][2][N]. */
int spiral_gpu_multiply_query_by_database(uint64_t *output, const uint64_t *reorientedCiphertexts,
                                          const uint64_t *database, size_t dim0, size_t num_per);
/* The same for n <= 8 queries against ONE pass over the database (no reference counterpart: the reference answers one query per
 * call): reorientedCts = the n queries' buffers one after the other, outputs = [n][num_per][n1][n2][2][N].  Where the geometry allows
 * (num_per >= 64, dim0 a multiple of 64, <= 2048) the pass runs on the matrix cores (csrc/sweep_mfma.hip), else as passes of two /
 * one on the vector ALU; every output equals multiply_query_by_database's for that query. */
int spiral_gpu_multiply_queries_by_database(uint64_t *outputs, const uint64_t *reorientedCiphertexts, size_t n,
                                            const uint64_t *database, size_t dim0, size_t num_per);
/* split_and_crt, src/spiral.cpp:270 : raw [num_per][n1][n2][N] -> NTT [num_per][m2][n2][2][N] */
int spiral_gpu_split_and_crt(uint64_t *out, const uint64_t *in, size_t num_per, uint32_t t_gsw);
/* foldOneFurtherDimension, src/spiral.cpp:1349.  cts: raw [2*num_per][n1][n2][N], the first num_per
 * are overwritten; query_ct / query_ct_neg: ONE dimension's reoriented (z, r, m) packed GSW matrices
 * (reorient_Q, :388). */
int spiral_gpu_fold_one_further_dimension(uint64_t *cts, size_t num_per, const uint64_t *query_ct,
                                          const uint64_t *query_ct_neg, uint32_t t_gsw);
/* expandImproved, src/spiral.cpp:1664.  cv_v: 2^g ciphertexts (n0 x 1, NTT form), element 0 is the
 * query, updated in place; W_left: g matrices n0 x t_exp; W_right: n_right matrices n0 x t_exp_right. */
int spiral_gpu_expand_improved(uint64_t *cv_v, uint32_t g, uint32_t t_exp, const uint64_t *w_left,
                               uint32_t t_exp_right, const uint64_t *w_right, uint32_t n_right,
                               uint32_t max_bits_to_gen_right, uint32_t stopround);
/* scalToMat, src/spiral.cpp:1918 : out n1 x n0 from cv n0 x 1 and W n1 x (n0*t_conv) */
int spiral_gpu_scal_to_mat(uint64_t *out, const uint64_t *cv, const uint64_t *w, uint32_t t_conv);
/* regevToGSW, src/spiral.cpp:1985 : out n1 x (n1*ell) from ell ciphertexts, W and V */
int spiral_gpu_regev_to_gsw(uint64_t *out, const uint64_t *cv_v, const uint64_t *w, const uint64_t *v,
                            uint32_t t_conv, uint32_t ell);

/* ------------------------------------------------------------------------------------------------
 * Resident server: do_test's server half (src/spiral.cpp:2337-2406, 1584-1629) with the database,
 * public parameters and all intermediates in HBM.
 * ------------------------------------------------------------------------------------------------ */
/* The server holds first-dimension indices j in [j_begin, j_end) of the database; (j_begin, j_end) = (0, 0) means the
 * whole first dimension [0, 2^nu1) (a single GPU).  Shards are summed by the caller between first_dim and lift (see
 * spiral_gpu_server_acc). */
int spiral_gpu_server_create(const spiral_gpu_params *p, int device, uint32_t j_begin, uint32_t j_end,
                             spiral_gpu_server **out);
/* A COLUMN SHARD: rank `rank` of n_ranks = G (a power of two) holds, for ALL first-dimension indices j, the ciphertext columns ii = rank + G k,
 * k < L = num_per / G -- the chunk the reduce-scatter of a j-sharded answer hands that rank.  Items map to (ii = i % num_per, j = i / num_per) and G
 * divides num_per, so the shard's image is the ordinary image of L columns of the items i = rank (mod G), item i at local index i / G.  Its sweep
 * yields finished sums for its own chunk: a sharded answer needs no accumulator reduce, only the all-gather of the folded ciphertexts (below:
 * spiral_gpu_server_run_column_batch).  The price: every rank expands and converts the whole query.
 * Bound: L >= 1, i.e. n_ranks <= num_per (a base server answers from one column: nu2 = 0); a larger or non-power-of-two n_ranks, or rank >= n_ranks,
 * is refused and the message names the bound.  The fold-rank count is fixed to n_ranks (set_fold_ranks with another count fails); n_ranks = 1 gives a
 * server whose run_column_batch followed by fold_root_batch equals run_query.  create_lane on a column shard yields a lane of the same rank.
 * Database calls on a column shard: gen_db leaves exactly the columns rank + G k of the unsharded gen_db of that seed; load_db takes the full
 * reference layout and keeps its columns; load_db_items takes a run of consecutive items and keeps every G-th; update_db_items writes the ids it
 * holds and skips the rest; read_db_items / read_db_items_at fill in the shard's own items of the caller's buffer and leave every other byte alone
 * (G shards reading into one buffer reassemble the database); fill_db_random, set_db_format, db_format, db_device_bytes as on any image.  The test
 * readers read_db_item, read_db_slots and read_db_columns refuse a column shard by name.
 * Answer calls: bind_keys, set_query_batch, read_response_wire_batch, fold_root(_batch) and the per-server setters and readers take a column shard;
 * the stage calls expand, convert, first_dim(_batch) work on its L columns.  run_query, answer*, run_query_batch*, run_query_instances*,
 * run_pre_sweep(_batch), run_expand_pack(_batch), run_unpack_convert_sweep(_batch), fold_local(_batch), lift, fold, run_post, set_expand_shard and
 * set_sweep_stages refuse it, naming the reason; so does any multi-lane call whose servers are not all column shards of one rank and rank count, or
 * none. */
int spiral_gpu_server_create_column_shard(const spiral_gpu_params *p, int device, uint32_t rank, uint32_t n_ranks, spiral_gpu_server **out);
void spiral_gpu_server_destroy(spiral_gpu_server *s);
/* use an external HIP stream (hipStream_t as void*); NULL = the server's own stream */
int spiral_gpu_server_set_stream(spiral_gpu_server *s, void *hip_stream);
/* the stream the server launches on now (hipStream_t as void*): e.g. to put the lanes of a batch on lanes[0]'s stream */
void *spiral_gpu_server_get_stream(spiral_gpu_server *s);

/* database producers: load_db, src/spiral.cpp:1028-1172 */
int spiral_gpu_server_load_db(spiral_gpu_server *s, const uint64_t *database /* full, reference layout */);
/* explicit DB generated on the device: plaintext coefficient k of item i is
 * splitmix64(seed ^ (i*4N + k)) % p_db (the rand() % p_db of :25-29 with a counter-based generator) */
int spiral_gpu_server_gen_db(spiral_gpu_server *s, uint64_t seed);
/* Raw ingest: the whole of load_db on the device -- plaintext coefficients in, device database out
 * (centred lift :1116-1127, to_ntt, layout :1139-1153), so the host ships log2(p_db) bits per coefficient instead of
 * the 8x larger NTT form.  `items` holds n_items consecutive plaintexts starting at item first_item (item i = database
 * entry (ii = i % num_per, j = i / num_per); a sharded server keeps the items of its own j-range and skips the rest);
 * one plaintext = n0*n2*2048 coefficients in [0, p_db), polynomial (m, c) at (m*n2 + c)*2048, each coeff_bits wide and
 * bit-packed little-endian like read_arbitrary_bits (src/core.cpp:20-30) -- coeff_bits = log2(p_db) is the item size
 * of select_params.py:297 (8192 B at p = 256, 15360 B at p = 2^15) -- or coeff_bits = 64: the reference's raw MatPoly
 * words.  Fails if a coefficient is >= p_db (the reference asserts).  May be called several times (streaming a database
 * larger than host memory). */
int spiral_gpu_server_load_db_items(spiral_gpu_server *s, const void *items, uint32_t coeff_bits, uint64_t first_item,
                                    uint64_t n_items);
/* Replace n items, given by index, of the database this server holds, in place and in the image's CURRENT form (packed or limb
 * planes; with option one_image = 0 a valid second limb-plane image is updated too).  items: n plaintexts laid out as for
 * load_db_items (coeff_bits wide, bit-packed, or coeff_bits = 64 raw words); item_ids[k] is the database index of plaintext k.  Ids
 * must be distinct and < dim0 * num_per.  A sharded server writes the ids in its own j-range and skips the rest.
 * The image is never converted and keeps its address, so graphs captured before replay afterwards and read the new items.
 * Atomic: a bad argument, a duplicate or out-of-range id, a coefficient >= p_db, a call on a lane or share_db server (update through
 * the owner), an allocation failure or a call while the server's stream is being captured fails and leaves the image byte-identical.
 * Ordering: the update is enqueued on this server's stream -- work submitted to that stream earlier reads the old items, work submitted
 * later the new ones (run_query_batch with this server as servers[0] is ordered by it) -- and nothing synchronises the device.  Lanes on
 * other streams are the caller's to order, as for loads.  The call returns once `items` and `item_ids` may be reused; it waits for the
 * previous update's launches (whose workspace it reuses) and for nothing else. */
int spiral_gpu_server_update_db_items(spiral_gpu_server *s, const void *items, uint32_t coeff_bits, const uint64_t *item_ids,
                                      uint64_t n);
/* bytes of n items in the bit-packed item stream of load_db_items / read_db_items: n * polys * 2048 * coeff_bits / 8, polys = 4 for a base
 * server (out_n = 0), 1 for a SpiralPack trial (out_n >= 1).  0 and last_error for coeff_bits outside 1..64 or 2^coeff_bits < p_db.  Host only. */
size_t spiral_gpu_db_items_bytes(const spiral_gpu_params *p, uint32_t out_n, uint32_t coeff_bits, uint64_t n_items);
/* The database back as plaintexts: items first_item .. first_item + n_items - 1 (read_db_items) or items item_ids[0 .. n) (read_db_items_at)
 * of the image this server references, byte for byte what load_db_items / update_db_items take.
 * Layout: item k of the call is at byte k * polys * 256 * coeff_bits of `items` (polys = 4); polynomial (m, c) at (m*n2 + c) * 2048
 * coefficients; coefficients coeff_bits wide in little-endian bit order, coeff_bits = 64: plain u64 words.  A polynomial is a whole number of
 * bytes (256 * coeff_bits), written whole: no byte of a neighbouring item is read or rewritten.
 * Undoing the lift: the ingest maps a plaintext value x < half = p_db >> 1 to x and x >= half to Q - (p_db - x).  So a lifted coefficient
 * v < half gives x = v, v >= Q - (p_db - half) gives x = v - Q + p_db, and any other v is NOT a plaintext image (after fill_db_random or a
 * load_db of arbitrary words): the call fails, the message says so and names the first offending item (lowest position in the call) and
 * coefficient; the contents of `items` are then unspecified.  The image, its form, its epoch and every captured graph are untouched, always.
 * Form: the image is read in the form it is in -- packed or plain, or limb planes (wide, and the 4-, 2- and 1-wave narrow forms) -- no
 * conversion is needed or made.  With option one_image = 0, `db` is read in the form db_format names; a second image is ignored.
 * Shards: a j-sharded server writes only the items of its own j-range and leaves the other items' bytes of `items` untouched, so G shards
 * fill one buffer (the mirror of load_db_items); read_db_items_at skips ids outside the shard the same way.  Ids need not be distinct or
 * sorted; every id must be < dim0 * num_per, which is checked before anything is launched.
 * Who may call: any server that references a loaded image, lanes and share_db servers included (reading does not write); "no database
 * loaded" otherwise.  Fails inside a stream capture.
 * Ordering: enqueued on this server's stream -- an update enqueued earlier on that stream is visible -- and the call returns after that stream
 * is synchronised and `items` is complete.  Staged through device memory in passes of option db_stage_bytes (one launch and one copy each).
 * Before any launch: null pointers, a range outside the database, coeff_bits outside 1..64 or 2^coeff_bits < p_db (64 always passes). */
int spiral_gpu_server_read_db_items(spiral_gpu_server *s, void *items, uint32_t coeff_bits, uint64_t first_item, uint64_t n_items);
int spiral_gpu_server_read_db_items_at(spiral_gpu_server *s, void *items, uint32_t coeff_bits, const uint64_t *item_ids, uint64_t n);

/* ---- Fingerprints: a database image compared with its source, or with another image, in 8 bytes per item or 8 bytes in all -------------------
 * The definition, stated once; the device kernels, the host function, and the Python and test code quote it.
 *
 *   - P = 2^61 - 1.  Every fingerprint is returned fully reduced, in [0, P - 1].
 *   - A key is two words: r = 2 + key[0] mod (P - 3), s = 2 + key[1] mod (P - 3), both in [2, P - 2].
 *   - An item is `polys` polynomials of 2048 plaintext coefficients x in [0, p_db).
 *       base server:  polys = 4, polynomial (m, c) at index q = 2 m + c -- the order of the item stream of load_db_items;
 *       SpiralPack:   polys = trials = out_n^2, polynomial q = the item's plaintext in trial q -- the order of the record layout below.
 *   - The item fingerprint:      f(item) = sum over q, c of x[q][c] * r^(2048 q + c + 1)  mod P.
 *   - The combined fingerprint:  F = sum over the items i of the call of f(item i) * s^(i + 1)  mod P, i the item's DATABASE index, not its
 *     position in the call.  Ranges add: F[a, a + n1) + F[a + n1, a + n1 + n2) = F[a, a + n1 + n2) mod P.  For a list of ids the sum runs over
 *     the list as given: a repeated id counts as often as it is listed.
 *   - A shard returns the partial sums over what it holds: a j-shard or column shard f = 0 for an item it does not hold and the F of its own
 *     items; a trial shard the polynomials q of its trial range.  The partials of all shards add mod P (spiral_gpu_fingerprint_add), per item
 *     and combined, to the unsharded values.
 *   - The function is linear in the coefficients, so an update of some items changes F by sum of (f_new - f_old) * s^(i + 1), and every value is
 *     an exact integer: the same bits in any order of summation.
 *   - Collision bound.  For two DIFFERENT databases of one geometry and a key drawn uniformly AFTER both are fixed, the combined fingerprints
 *     agree with probability at most (2048 * polys + number of items) / (P - 3) -- about 2^-37 at 2^24 items; two independent keys square the
 *     bound.  This is a universal hash, not a cryptographic one: it gives nothing against someone who knows the key.
 *
 * fingerprint_items / fingerprint_items_at compute f of each item of the call into per_item[k] (uint64_t[n], or NULL) and F into *combined (or
 * NULL; at least one of the two is given), on the device, from the image in the form it is in.  Everything else is read_db_items' contract above,
 * word for word -- who may call, the forms read and never converted, one_image = 0, ordering (enqueued on this server's stream; returns after
 * that stream is synchronised), refused inside a capture, the image, its form, its epoch and every captured graph untouched, the checks that
 * come before any launch (null pointers, a range or an id outside the database, both outputs NULL), and an image that holds no plaintexts
 * refused with the first offending item, polynomial and coefficient named, the outputs then unspecified -- except that a shard WRITES 0 for an
 * item it does not hold.  The workspace is the server's, reused from call to call and bounded by option db_stage_bytes (8 bytes per polynomial
 * and per item of a pass). */
int spiral_gpu_server_fingerprint_items(spiral_gpu_server *s, const uint64_t *key, uint64_t first_item, uint64_t n_items, uint64_t *per_item,
                                        uint64_t *combined);
int spiral_gpu_server_fingerprint_items_at(spiral_gpu_server *s, const uint64_t *key, const uint64_t *item_ids, uint64_t n, uint64_t *per_item,
                                           uint64_t *combined);
/* The same function on the host, from a bit-packed item stream (coeff_bits 1..64, 2^coeff_bits >= p_db, as load_db_items takes it); needs no GPU.
 * `items` holds, for each of n_items consecutive items from database index first_item, the polynomials poly0 .. poly0 + n_polys - 1 of an item of
 * polys_per_item (<= 256), 256 * coeff_bits bytes each: a base item stream is (4, 0, 4), one SpiralPack trial's stream (trials, t, 1), a SpiralPack
 * record-layout item (trials, 0, trials).  Fails on a coefficient >= p_db, which it names, on poly0 + n_polys > polys_per_item, on both outputs
 * NULL, and on p_db outside [2, P]. */
int spiral_gpu_fingerprint_host(const uint64_t *key, uint64_t p_db, const void *items, uint32_t coeff_bits, uint32_t polys_per_item, uint32_t poly0,
                                uint32_t n_polys, uint64_t first_item, uint64_t n_items, uint64_t *per_item, uint64_t *combined);
/* (a + b) mod P of two fingerprints.  An argument >= P is refused: the call returns P, which no fingerprint is, and sets last_error. */
uint64_t spiral_gpu_fingerprint_add(uint64_t a, uint64_t b);
#define SPIRAL_GPU_FINGERPRINT_MODULUS ((1ull << 61) - 1)

/* Tracked.  With P, r, s, q, c, x as above:
 *   - the polynomial sum  g(i, q) = sum over c of x[q][c] * r^(c + 1)  mod P  (the word the fingerprint's first launch computes per polynomial),
 *   - f(i) = sum over q of g(i, q) * r^(2048 q),   F = sum over the database indices i of f(i) * s^(i + 1).
 * The tracked state belongs to the image's holder: the key; g for every (local item, polynomial) the server holds, 8 bytes each, resident on the
 * device (4 words per item on a base server, one per held trial on SpiralPack); and F over what the server holds, as accumulator words on the
 * device that the host adds.  A j-shard, column shard or trial shard keeps its partial F; partials add (spiral_gpu_fingerprint_add).
 *
 * fingerprint_track(key, poly_sums): poly_sums NULL computes the table and F from the image in its current form (fingerprint_items' passes and
 *   contract; an image without plaintexts is refused with that call's message and tracking stays off).  poly_sums given adopts a table --
 *   uint64_t[local items][polynomials held], local items in ascending database index, q ascending -- WITHOUT reading the image: every word must
 *   be below P, else the call is refused.  Owner only (a lane or share_db server is refused); refused inside a capture; tracking again replaces
 *   the state.  fingerprint_untrack frees it.
 * Kept current: update_db_items and update_records of a tracked image also replace the table words of the polynomials they write and add
 *   (g_new - g_old) * r^(2048 q) * s^(i + 1) to F, in launches of their own behind the scatter on the holder's stream, from the plaintexts the call
 *   brought -- the image is not read, and no synchronisation is added.  A record call replaces only the polynomials a record touches.  A call that
 *   fails leaves image, table, F and the update count as they were.  set_db_format and a batch's automatic conversion keep the state (the table does
 *   not depend on the form).  gen_db, load_db, load_db_items, load_records and fill_db_random END tracking: keeping partial loads current is out of
 *   scope, track again after them.  With tracking off every call does what it did, with the same kernels.
 * fingerprint_tracked: synchronises this server's stream and returns the key, F (8 bytes: a 2 KiB copy added on the host) and the number of table
 *   words replaced since track (a host counter); any out pointer may be NULL; any server that references the image may call; fails when the image
 *   is not tracked.
 * fingerprint_tracked_polys: the table's words of database items [first_item, + n_items) into poly_sums[n_items][polynomials held]; a j-shard or
 *   column shard writes 0 for an item it does not hold, as fingerprint_items does, so the shards' outputs add to the unsharded table.
 * fingerprint_scrub: recomputes g of the range from the image in its current form (fingerprint_items' kernels, passes and contract: who may call,
 *   forms, ordering, refused in a capture, nothing converted, a coefficient that is no plaintext value fails the call naming item and coefficient)
 *   and compares each word with the table on the device: *n_bad = the polynomials that differ, and with n_bad > 0 the lowest (database item,
 *   polynomial) to *first_bad_item, *first_bad_poly (else untouched; either may be NULL).  Sixteen bytes come back.
 * Measured at 2^15 items of 8 KiB on one MI355X (profiles/db_track.json; tracked / untracked, device ms, packed image): update_db_items of 1 item
 *   0.039 / 0.031, of 4096 items 4.89 / 4.86; update_records of 1 record 0.076 / 0.068, of 4096 records 2.66 / 2.64; fingerprint_tracked 0.037 ms per
 *   call against 5.88 ms for fingerprint_items of the image; track and scrub of the whole image 6.14 and 6.13 ms against 5.82 ms. */
int spiral_gpu_server_fingerprint_track(spiral_gpu_server *s, const uint64_t *key, const uint64_t *poly_sums);
int spiral_gpu_server_fingerprint_untrack(spiral_gpu_server *s);
int spiral_gpu_server_fingerprint_tracked(spiral_gpu_server *s, uint64_t *key_out, uint64_t *combined, uint64_t *n_updates);
int spiral_gpu_server_fingerprint_tracked_polys(spiral_gpu_server *s, uint64_t first_item, uint64_t n_items, uint64_t *poly_sums);
int spiral_gpu_server_fingerprint_scrub(spiral_gpu_server *s, uint64_t first_item, uint64_t n_items, uint64_t *n_bad, uint64_t *first_bad_item,
                                        uint32_t *first_bad_poly);
/* f and F from a table of g, on the host (no GPU): poly_sums[k * n_polys + q] = g(first_item + k, poly0 + q) of an item of polys_per_item
 * polynomials -- an exported table yields every value the other calls return.  (g itself from plaintexts: spiral_gpu_fingerprint_host with
 * polys_per_item = 1 on a stream of single polynomials.)  Fails on a word >= P, on both outputs NULL and on poly0 + n_polys > polys_per_item. */
int spiral_gpu_fingerprint_of_polys(const uint64_t *key, const uint64_t *poly_sums, uint32_t polys_per_item, uint32_t poly0, uint32_t n_polys,
                                    uint64_t first_item, uint64_t n_items, uint64_t *per_item, uint64_t *combined);

/* ---- Records: byte strings of any size S >= 1, packed into the plaintexts of a base or a SpiralPack server ----------------------------------
 * The layout, stated once; every record call below, and the Python and test code, quote it.
 *
 * For a base parameter set:
 *   - w = floor(log2 p_db) bits per coefficient are used.  For a power-of-two p_db this is the item stream of load_db_items at coeff_bits = log2 p_db.
 *   - A polynomial is 256 w bytes.
 *   - An item is item_bytes = 1024 w bytes: polynomial (m, c) at (m*2 + c) * 256 w, bits little-endian, exactly as read_db_items(w) lays it out.
 * For a record size S >= 1 there are two cases.
 *   - S <= item_bytes.  Then per_item = floor(item_bytes / S) and instances = 1.  Record r lives in item r / per_item and occupies bytes
 *     [(r mod per_item) * S, + S) of that item's stream.  Records never straddle items.  They may straddle polynomials, and when 8 S is not a
 *     multiple of w their ends fall inside a coefficient.  The item's last item_bytes - per_item * S bytes are padding.
 *   - S > item_bytes.  Then per_item = 1 and instances = ceil(S / item_bytes) (the reference's `factor`, select_params.py; refused above 16 as
 *     the instance calls refuse it).  Chunk f of record r is bytes [f * item_bytes, ...) of the record; it sits at byte 0 of item r of
 *     instance f.  The tail of the last chunk is padding.
 * In both cases capacity = 2^(nu1 + nu2) * per_item records.  (p = 256, S = 256: 32 records per 8192-byte item; p = 2^15, S = 100 000: 7
 * instances of 15 360-byte items.)
 * Padding: load_records writes it as zero; update_records never changes a bit outside the ranges of the records it is given.
 * A coefficient of the image that is no plaintext value (after fill_db_random), or whose value is >= 2^w (only possible for a p_db that is no
 * power of two), is not part of a record database: every call that would have to read it fails, the message names the first such record (lowest
 * position in the call) and coefficient, and the failing call changes nothing.
 * `instance` (all server calls) selects which chunk of each record this server's image holds: 0 unless instances > 1.  One call is made per
 * instance server on the same buffer, the way shards share one.
 *
 * SpiralPack.  For a SpiralPack parameter set with out_n >= 1 and trials = out_n^2 (the spiral_gpu_pack_server_*_records calls, and a client
 * session created with out_n >= 1):
 *   - w = floor(log2 p_db) bits per coefficient and 256 w bytes per polynomial, as above.
 *   - An item is item_bytes = trials * 256 w bytes: polynomial t of item i is item i of trial t, at byte t * 256 w of the item's stream, bits
 *     little-endian, exactly as pack_server_read_db_items(trial = t, w) lays out that one polynomial.  The stream is ordered by trial index.
 *     In a decoded response trial t is output polynomial (r, col) = (t / out_n, t % out_n), i.e. t = r * out_n + col: polynomial t of what
 *     spiral_gpu_client_decode returns.
 *   - S <= item_bytes: per_item = floor(item_bytes / S) and instances = 1, record r in item r / per_item at bytes [(r mod per_item) * S, + S).
 *     Records never straddle items; they may straddle polynomials -- here: trial images -- and end inside a coefficient; the item's tail is
 *     padding.
 *   - S > item_bytes: per_item = 1 and instances = ceil(S / item_bytes), refused above 16.  The instances are SpiralPack servers, as
 *     spiral_gpu_pack_server_answer_batch_instances takes them; chunk f of record r sits at byte 0 of item r of instance f.
 *   - capacity = 2^(nu1 + nu2) * per_item.
 * The rules for padding and for a coefficient that is not record data are the ones above, word for word; the message names the record, the trial
 * and the coefficient.  (p = 256, out_n = 2: 8192-byte items, as the base server's; out_n = 4: 32 768-byte items, 128 records of 256 bytes.) */
typedef struct spiral_gpu_record_layout {
    uint32_t coeff_bits; /* w */
    uint32_t instances;
    uint64_t per_item;
    uint64_t item_bytes;
    uint64_t capacity;
} spiral_gpu_record_layout;
/* host only, no device needed; fails for parameters get_shape refuses, S = 0, or more than 16 instances */
int spiral_gpu_record_layout_of(const spiral_gpu_params *p, uint64_t record_bytes, spiral_gpu_record_layout *out);
/* the same for a SpiralPack parameter set, out_n in 1 .. 16 ("SpiralPack" above); host only */
int spiral_gpu_pack_record_layout_of(const spiral_gpu_params *p, uint32_t out_n, uint64_t record_bytes, spiral_gpu_record_layout *out);
/* Records first_record .. first_record + n_records - 1 from one contiguous byte array (record k of the call at k * record_bytes), through
 * load_db_items' ingest: the range starts and ends at a multiple of per_item.  The records are repacked into items on the host with zero
 * padding; where per_item * S = item_bytes (and p_db is a power of two) the bytes go through unchanged.  A sharded server keeps what it holds. */
int spiral_gpu_server_load_records(spiral_gpu_server *s, const void *records, uint64_t record_bytes, uint32_t instance, uint64_t first_record,
                                   uint64_t n_records);
/* Replace n records given by id, in place, in the image's CURRENT form, on the holder's stream: update_db_items' contract at a record's
 * granularity.  Ids are distinct and below the capacity; every check runs before anything is launched; a failing call leaves the image
 * byte-identical; no conversion and no new epoch, so graphs captured before still replay and now read the new record; a j-sharded or
 * column-sharded server writes the records it holds and skips the rest; lanes and share_db servers are refused (update through the owner); refused
 * inside a stream capture.  One read-modify-write launch (one workgroup per polynomial of a touched item) and update_db_items' scatter launch.
 * Returns once `records` and `record_ids` may be reused.  Where every touched polynomial is covered whole by the call's records, nothing of the
 * image is read and nothing is synchronised, as for update_db_items; otherwise the call waits for this server's stream (and nothing else) to learn
 * whether the polynomials it read hold record data, and fails with the image untouched if they do not. */
int spiral_gpu_server_update_records(spiral_gpu_server *s, const void *records, uint64_t record_bytes, uint32_t instance,
                                     const uint64_t *record_ids, uint64_t n);
/* The mirror of read_db_items / read_db_items_at: record k of the call to byte k * record_bytes of `records` (an instance server: its chunk of
 * it).  Any server that references a loaded image may call them, lanes included; shards fill in the records they hold and leave the other bytes
 * alone; ids need not be distinct; the call returns synchronised.  One workgroup per touched polynomial, and only the records' bytes are staged and
 * copied.  A range of whole items of a layout without padding is the range export of read_db_items. */
int spiral_gpu_server_read_records(spiral_gpu_server *s, void *records, uint64_t record_bytes, uint32_t instance, uint64_t first_record,
                                   uint64_t n_records);
int spiral_gpu_server_read_records_at(spiral_gpu_server *s, void *records, uint64_t record_bytes, uint32_t instance, const uint64_t *record_ids,
                                      uint64_t n);
/* ---- Keyed records: put, get and delete by key; bucketised two-choice hashing over the items of a base or a SpiralPack server ----------------
 * The definition, stated once; the C++ (csrc/kv_host.h), the Python and the tests' restatement quote it.  Base parameter sets first, then
 * "SpiralPack" below; one instance, an unsharded image.
 *
 * Layout.  w, item_bytes = 1024 w and the item stream are those of "Records".  A bucket is an item: bucket b is item b, in the item order of
 * load_db_items.  For a value size V >= 1, slots = floor(item_bytes / (8 + V)), and the bucket's stream is
 *     [slots x 8-byte tags, little-endian u64][slots x V value bytes][padding]:
 * the tag of slot s at byte 8 s, its value at byte 8 slots + s V.  Refused: slots = 0; slots > 256; a header that does not lie inside polynomial 0
 * (8 slots > 256 w) -- a probe therefore reads one polynomial per bucket; fewer than 2 buckets.  Tag 0 means "empty": an image of all-zero
 * plaintexts is an empty table.  capacity = 2^(nu1 + nu2) * slots.
 *
 * Hash.  SipHash-2-4 (c = 2, d = 4, 64-bit output) under the 16-byte table key: k0 = LE64(bytes 0..7), k1 = LE64(bytes 8..15).
 *     tag = SipHash(k0, k1; key), a result of 0 replaced by 1;   u = SipHash(k0, k1 XOR 0xA5; key);   nb = 2^(nu1 + nu2);
 *     b1 = (u & 0xffffffff) mod nb;   b2 = (u >> 32) mod nb, and b2 = b1 XOR 1 where that equals b1.
 * Two keys with equal tags that share a candidate bucket are ONE key to this store.  For a table key drawn after the key set is fixed the chance
 * of that is at most 2 slots / 2^64 per pair of keys.  The hash runs on the host: the client needs the bucket numbers there to make its queries.
 *
 * Placement.  Keys are placed in the order of the call.  (1) If the tag is present in b1 or b2 (b1 is looked at first), that slot is overwritten.
 * (2) Otherwise the bucket with fewer used slots takes it; a tie goes to b1.  (3) Within the bucket, the lowest free slot.  (4) Both full: the call
 * fails.
 *
 * A coefficient of a probed header that is no plaintext value below 2^w fails the call as a record call fails, naming the first such bucket.
 *
 * SpiralPack.  For a SpiralPack parameter set with out_n >= 1 (the spiral_gpu_pack_server_kv_* calls, and a client session created with
 * out_n >= 1):
 *   - w, item_bytes = out_n^2 * 256 w and the item stream are those of "Records", SpiralPack: polynomial t of bucket b is item b of trial image t.
 *   - A bucket is an item, and nb = 2^(nu1 + nu2).
 *   - slots = floor(item_bytes / (8 + V)), and the bucket's stream is [slots x 8-byte tags][slots x V value bytes][padding], exactly as above.
 *   - Refused, as above: slots = 0; slots > 256; nb < 2; 8 slots > 256 w -- the header lies inside polynomial 0, which is trial 0, so a probe still
 *     reads one polynomial per bucket.  A value may span several polynomials, i.e. trial images.
 *   - Hash and placement are the ones above, word for word.
 *   (p = 256, out_n = 2, V = 248: 32 slots, as the base server's; p = 256, out_n = 4, V = 4088: 8 slots of a 32 768-byte bucket.)
 * Out of scope, each refused by name: trial-sharded servers (create_sharded with fewer than all trials, and their shard lanes); values larger
 * than an item (instances). */
typedef struct spiral_gpu_kv_layout {
    uint32_t coeff_bits; /* w */
    uint32_t slots;
    uint64_t value_bytes;
    uint64_t item_bytes;
    uint64_t buckets;  /* nb */
    uint64_t capacity; /* nb * slots */
} spiral_gpu_kv_layout;
/* host only, no device needed */
int spiral_gpu_kv_layout_of(const spiral_gpu_params *p, uint64_t value_bytes, spiral_gpu_kv_layout *out);
/* host only: the definition's tag, b1 and b2 of one key of key_bytes >= 0 bytes (key may be NULL for 0 bytes) */
int spiral_gpu_kv_hash(const spiral_gpu_params *p, const void *table_key16, const void *key, uint64_t key_bytes, uint64_t *tag, uint64_t *b1,
                       uint64_t *b2);
/* A fresh table from n keys (`keys` is [n][key_bytes], `values` [n][value_bytes]): placement from empty on the host, the item stream built there
 * with every unused byte zero, then load_db_items' ingest of the whole image.  Fails before touching the image where a key cannot be placed or two
 * keys have equal tags (both named by position). */
int spiral_gpu_server_kv_load(spiral_gpu_server *s, const void *table_key16, const void *keys, uint64_t key_bytes, const void *values,
                              uint64_t value_bytes, uint64_t n);
/* put: arguments are checked first (two keys of one call with equal tags are refused by position); ONE probe launch (one workgroup per distinct
 * candidate bucket: it reads polynomial 0 from the image in its current form and returns 32 bytes of occupancy per bucket and 4 bytes per (key,
 * candidate), not the headers) and one wait on this server's stream; the host applies the placement rule; a key with both buckets full fails the
 * call naming the first such key, and nothing is written; otherwise tag and value of every key go through update_records' read-modify-write and
 * scatter: in place, in the current form, no epoch, tracked fingerprints kept current.  Owner only; refused inside a capture; refused on a j-shard or
 * a column shard (both candidates of a key must be probed in one place).
 * delete: the same probe; tag and value bytes of each found slot are written as zero; an absent key is not an error; *n_deleted (may be NULL)
 * counts the keys found.
 * get: the probe, then the found slots' values through read_records' path; found[k] is 0 (absent), 1 or 2 (the candidate that holds it); a missing
 * key's bytes of `values` are left alone.  Any server that references the image may call it, lanes included. */
int spiral_gpu_server_kv_put(spiral_gpu_server *s, const void *table_key16, const void *keys, uint64_t key_bytes, const void *values,
                             uint64_t value_bytes, uint64_t n);
int spiral_gpu_server_kv_delete(spiral_gpu_server *s, const void *table_key16, const void *keys, uint64_t key_bytes, uint64_t value_bytes, uint64_t n,
                                uint64_t *n_deleted);
int spiral_gpu_server_kv_get(spiral_gpu_server *s, const void *table_key16, const void *keys, uint64_t key_bytes, void *values, uint64_t value_bytes,
                             uint64_t n, uint8_t *found);
/* Table occupancy (a base server here, a SpiralPack server: spiral_gpu_pack_server_kv_stats): how full buckets [first_bucket, first_bucket + n_buckets) of a keyed table with values of value_bytes bytes are, computed where
 * the image lives.  ONE launch (one per 2^23 buckets of the range, so that a grid stays below 2^32 threads): the probe's gather, inverse transform and header packing of polynomial 0 per bucket -- the bucket's place comes
 * from the block index, no table is uploaded -- then one integer atomic add per bucket into a histogram, so the result is exact whatever the
 * order; 257 words come back, not the headers, and used, full_buckets and max_used are derived from them on the host.  Any server that references
 * the image may call it, lanes included, on its own stream; the call returns synchronised.  Refused inside a capture, on a j-shard, a column shard
 * and a trial shard, and for a range that is not inside [0, nb]; n_buckets = 0 returns zeros (and `slots`).  A bucket whose polynomial 0 holds a
 * coefficient that is no plaintext value below 2^w fails the call, naming the lowest such bucket. */
typedef struct spiral_gpu_kv_stats {
    uint64_t buckets;      /* n_buckets looked at */
    uint64_t used;         /* slots whose tag is not 0 */
    uint64_t full_buckets; /* buckets with used == slots */
    uint32_t max_used, slots;
    uint64_t hist[257]; /* hist[u] = buckets with exactly u used slots; entries above `slots` are 0 */
} spiral_gpu_kv_stats;
int spiral_gpu_server_kv_stats(spiral_gpu_server *s, uint64_t value_bytes, uint64_t first_bucket, uint64_t n_buckets, spiral_gpu_kv_stats *out);
/* Listing.  The definition, stated once; csrc/kv_host.h, the Python wrappers and the tests' restatement quote it.  An ENTRY is a slot whose tag is not 0,
 * reported as {tag, bucket, slot}.  A LISTING of a set of buckets is all their entries, in the order of the buckets, and within a bucket by ascending
 * slot.  With values, row k of `values` is the value_bytes bytes of entry k: bytes [8 slots + slot V, + V) of the bucket's stream.
 *
 * kv_scan lists buckets [first_bucket, first_bucket + n_buckets) in ascending order; the range is checked against [0, nb] as kv_stats checks it, and
 * n_buckets = 0 returns 0 entries.  kv_scan_at lists the buckets of a list, in the order of the list: ids need not be distinct (a bucket named twice
 * is listed twice), an id >= nb is refused by position before any launch, and entry.bucket is the bucket's id, not its position.
 *   - *n_entries is always the number of entries in the buckets named, whatever max_entries is.
 *   - max_entries = 0 with entries = values = NULL is count-only: the result equals kv_stats(...).used over the same buckets; no tag is staged and no
 *     compaction is launched.
 *   - If the count exceeds max_entries the call fails with both numbers in the message; *n_entries is set and not one byte of `entries` or `values`
 *     is written.
 *   - `values` may be NULL (tags only).  `entries` must not be NULL when max_entries > 0.
 *   - Who may call, and where, is kv_stats' contract: any server that references the image, lanes included, on its own stream; the call returns
 *     synchronised; refused inside a capture; refused by name on a j-shard, a column shard and a trial shard; nb <= 2^31 - 1; the image is read in the
 *     form it is in, nothing is converted, no epoch changes, no graph is re-captured; tracked fingerprints are untouched.
 *   - A header coefficient that is no plaintext value below 2^w fails the call as kv_stats does, naming the lowest such bucket (kv_scan_at: the lowest
 *     position in the list, and its bucket) and the coefficient.
 * The device work runs in passes of option "kv_scan_chunk" buckets, three launches each on the caller's stream, none of which waits for another
 * workgroup: (1) decode, one workgroup per bucket -- the probe's gather, inverse transform and header packing of polynomial 0, the tags staged, the
 * bucket's count from the waves' ballots; (2) ONE workgroup's exclusive scan of the pass's counts on top of a running total that stream order carries
 * from pass to pass; (3) compact, one workgroup per bucket -- each live slot's rank from the ballots, its 16-byte entry stored at offset + rank where
 * that is below max_entries.  Staging is the server's export workspace: 8 bytes per slot of ONE pass (at most 32 MiB by default) and 16 bytes per
 * entry that can come back, min(max_entries, slots of the buckets named).  After the last pass the error word, the total and the entries come back in
 * one copy sequence and one wait; the values of the entries then go through read_records' path (passes of option db_stage_bytes), only where values
 * are wanted and the count fits. */
typedef struct spiral_gpu_kv_entry {
    uint64_t tag;
    uint32_t bucket;
    uint32_t slot;
} spiral_gpu_kv_entry; /* 16 bytes */
int spiral_gpu_server_kv_scan(spiral_gpu_server *s, uint64_t value_bytes, uint64_t first_bucket, uint64_t n_buckets, spiral_gpu_kv_entry *entries,
                              void *values, uint64_t max_entries, uint64_t *n_entries);
int spiral_gpu_server_kv_scan_at(spiral_gpu_server *s, uint64_t value_bytes, const uint64_t *buckets, uint64_t n_buckets, spiral_gpu_kv_entry *entries,
                                 void *values, uint64_t max_entries, uint64_t *n_entries);
/* Host only, no device needed: a listing of the WHOLE table against a key set.  `entries` must be strictly ascending in (bucket, slot), with buckets
 * below nb and tags that are not 0, else the call refuses by position; two keys with equal tags are refused by position, as kv_put refuses them.  The
 * hash is the definition's and depends only on nb and the table key, so base and SpiralPack parameter sets share this function.
 *   where[k]        the position in `entries` of the entry a lookup of key k finds (b1 first, the lowest slot), or -1
 *   entry_class[e]  0 held: some key's where;  1 shadowed: a key's tag in one of that key's candidate buckets, but a lookup finds another entry first;
 *                   2 misplaced: a key's tag in a bucket that is neither of its candidates, so no lookup reaches it;  3 orphan: the tag of no key given
 *   counts          the totals; missing = the number of -1 in where
 * where, entry_class and counts may each be NULL. */
typedef struct spiral_gpu_kv_reconcile_counts {
    uint64_t held, missing, shadowed, misplaced, orphans;
} spiral_gpu_kv_reconcile_counts;
int spiral_gpu_kv_reconcile(const spiral_gpu_params *p, const void *table_key16, const void *keys, uint64_t key_bytes, uint64_t n_keys,
                            const spiral_gpu_kv_entry *entries, uint64_t n_entries, int64_t *where, uint8_t *entry_class,
                            spiral_gpu_kv_reconcile_counts *counts);

/* read the device database back in reference layouts (tests): plaintext `item` as its n0 x n2 NTT-form MatPoly
 * (pts_encd, :1128), or slabs z_begin .. z_begin+nz-1 of load_db's layout restricted to this server's j-range:
 * word (z, ii, c, j, m) at ((((z - z_begin)*num_per + ii)*n2 + c)*(j_end - j_begin) + (j - j_begin))*n0 + m */
int spiral_gpu_server_read_db_item(spiral_gpu_server *s, uint64_t item, uint64_t *out);
int spiral_gpu_server_read_db_slots(spiral_gpu_server *s, uint32_t z_begin, uint32_t nz, uint64_t *out);
/* the same for ALL 2048 slots but only the plaintext columns ii in [ii_begin, ii_begin + n_ii): load_db's layout of a database
 * with num_per = n_ii, i.e. exactly what multiplyQueryByDatabase (src/spiral.cpp:628) needs to produce the full output
 * polynomials of those ciphertexts (2048 * n_ii * n2 * (j_end - j_begin) * n0 words; tests at sizes whose whole image
 * does not fit a host-side reference) */
int spiral_gpu_server_read_db_columns(spiral_gpu_server *s, uint32_t ii_begin, uint32_t n_ii, uint64_t *out);
/* The two forms of the device image.  PACKED (every loader writes it): a word = two 28-bit residues in 7 bytes, streamed by the vector-ALU
 * sweep (the single-query path).  LIMBS: every residue as three signed bytes and a 4-bit top limb, still 3.5 bytes, laid out as MFMA operands
 * for the batched sweep on the matrix cores (csrc/sweep_mfma.hip); single queries then sweep it with the one-query instance of the same kernel.
 * set_db_format converts the holder's image in place through a bounded staging buffer (the maps are bijective: packed -> limbs -> packed
 * reproduces every byte), so one image serves both kernels whatever the database's size; a batch converts to LIMBS by itself (option
 * "one_image"), a partial load_db_items and set_sweep_stages(K > 1) convert back.  LIMBS exists where the matrix-core sweep does (>= 64
 * ciphertexts per slot -- or 8, 16 or 32 with option "sweep_narrow" = 1 --, the shard's first dimension a power of two in [64, 2048]:
 * spiral_gpu_has_limb_form); elsewhere set_db_format(LIMBS) fails.  An image that is in the form stays usable when the option is switched off.  Call it on the
 * image's owner (not on a lane), outside stream capture; the lanes' captured graphs are re-captured by themselves.
 * db_device_bytes: device memory the holder of this server's image keeps for database images (one image, unless "one_image" is 0). */
enum spiral_gpu_db_format { SPIRAL_GPU_DB_PACKED = 0, SPIRAL_GPU_DB_LIMBS = 1 };
int spiral_gpu_server_set_db_format(spiral_gpu_server *s, int format);
int spiral_gpu_server_db_format(spiral_gpu_server *s);
uint64_t spiral_gpu_server_db_device_bytes(spiral_gpu_server *s);
/* --random-data analogue: arbitrary valid NTT-form words, timing only */
int spiral_gpu_server_fill_db_random(spiral_gpu_server *s, uint64_t seed);
/* a second in-flight query on one database: `s` releases its own image and sweeps `owner`'s (same parameters, shard and device;
 * the owner does not reload while `s` answers; loads through `s` fail).  One handle per query lane, each on
 * its own stream: the latency-bound expansion / folding of one query runs under the HBM-bound sweep of another.
 * Lifetime: the image is counted -- the owner and every lane hold a reference.  spiral_gpu_server_destroy(owner) while lanes exist destroys the
 * owner and invalidates the handle like any other; the image itself is freed with its last reference, so a lane never sweeps freed memory. */
int spiral_gpu_server_share_db(spiral_gpu_server *s, spiral_gpu_server *owner);
/* the same in one step and without ever allocating a second image: a new server with `owner`'s parameters, device and shard
 * whose database IS the owner's (a query lane).  Works for images larger than half of HBM, where create + share_db cannot. */
int spiral_gpu_server_create_lane(spiral_gpu_server *owner, spiral_gpu_server **out);

/* public parameters (NTT form): W_exp_left g x (n0 x t_exp), W_exp_right n_right x (n0 x t_exp_right),
 * W n1 x (n0*t_conv), V n1 x (2*t_conv)   (src/spiral.cpp:2091-2092, 2216-2227, 2279-2296).  A null pointer among those the geometry needs
 * fails before anything is written: the previous public parameters stay. */
int spiral_gpu_server_set_pub_params(spiral_gpu_server *s, const uint64_t *w_left, const uint64_t *w_right,
                                     const uint64_t *w, const uint64_t *v);
/* query: n_query_cts Regev ciphertexts, n0 x 1 NTT form */
int spiral_gpu_server_set_query(spiral_gpu_server *s, const uint64_t *query);

/* Wire form of what a client sends: the message is a sequence of polynomials in the raw form's order ([rows][cols][2048]), each
 * coefficient a value in [0, Q] in 7 little-endian bytes (56 bits = logQ, the width the reference's summary counts, src/spiral.cpp:
 * 219-242): 14 336 bytes per polynomial instead of the NTT form's 32 768.  A query is its n_query_cts ciphertexts n0 x 1; public
 * parameters are ONE message holding the matrices of set_pub_params in its argument order (W_exp_left, W_exp_right, W, V; SpiralPack:
 * W_exp_left, W_exp_right, V, v_W) with the same shapes.  The seeded form below also leaves out every matrix's random row 0.
 * *_wire_bytes: the size of such a message (0 for parameters that get_shape / pack_get_shape refuse).
 * raw_to_wire / raw_from_wire: the client's half, plain host code (no device): npolys raw polynomials <-> their wire form; raw_to_wire
 * refuses a value above Q and then writes nothing.
 * set_query_wire / set_pub_params_wire: the server's half.  The bytes go up through a bounded staging buffer and each chunk is decoded and
 * transformed on the device straight into the buffers set_query / set_pub_params fill (so the same device state, and graphs captured
 * before replay the new query without a re-capture; owners and lanes alike); one synchronisation at the end.  A wrong byte count or a
 * coefficient above Q fails, naming the first bad coefficient, and leaves the server with NO query (resp. no public parameters): nothing
 * answers from a half-written buffer.  Not during stream capture. */
size_t spiral_gpu_query_wire_bytes(const spiral_gpu_params *p);
size_t spiral_gpu_pub_params_wire_bytes(const spiral_gpu_params *p);
int spiral_gpu_raw_to_wire(const uint64_t *raw, size_t npolys, void *wire);
int spiral_gpu_raw_from_wire(const void *wire, size_t npolys, uint64_t *raw);
int spiral_gpu_server_set_query_wire(spiral_gpu_server *s, const void *wire, size_t bytes);
int spiral_gpu_server_set_pub_params_wire(spiral_gpu_server *s, const void *wire, size_t bytes);

/* Seeded form: the wire form with the uniformly random row 0 of every matrix replaced by one 32-byte seed.  A message is the seed followed by the
 * wire form of the same matrices (same order and shapes as set_query_wire / set_pub_params_wire) with each matrix's row 0 left out: 32 + (wire
 * polynomials - row-0 polynomials) x 14 336 bytes.  Row 0 is defined in NTT / CRT form: number a message's row-0 polynomials k = 0, 1, ... matrix by
 * matrix, column by column (query ciphertext c: k = c); slot z of polynomial k is ChaCha20 (RFC 8439) with key = the seed, nonce = LE32(d) || LE64(k)
 * and block counter z >> 1; of the block's words w[0..15] with h = z & 1, the residue mod p is the little-endian 128-bit w[8h..8h+3] mod p and the
 * residue mod b is w[8h+4..8h+7] mod b.  Domain tags d: 1 base query, 2 base public parameters, 3 SpiralPack query, 4 SpiralPack public parameters.
 * The client takes row 0 = seed_expand(...) and a = -row 0 for the rows it computes.
 * A QUERY'S SEED MUST BE FRESH FOR EVERY QUERY: two queries under one seed and one key share row 0, and their rows 1.. then differ by the
 * difference of the two messages (plus noise).  The server cannot check this.
 * *_seeded_bytes: the size of such a message (0 for parameters that get_shape / pack_get_shape refuse).
 * seed_expand: the client's half, plain host code (no device): row-0 polynomials first_k .. first_k + npolys - 1 of `domain`, reference NTT layout
 * [k][prime][z].
 * set_query_seeded / set_pub_params_seeded: the server's half.  Row 0 is generated on the device into the buffers set_query / set_pub_params fill,
 * the other rows are decoded as set_query_wire does (so graphs captured before replay the new query without a re-capture).  A wrong byte count or a
 * coefficient above Q (named by its index among the message's coefficients after the seed) fails and leaves NO query (resp. no public parameters).
 * Not during stream capture. */
size_t spiral_gpu_query_seeded_bytes(const spiral_gpu_params *p);
size_t spiral_gpu_pub_params_seeded_bytes(const spiral_gpu_params *p);
int spiral_gpu_seed_expand(const void *seed32, uint32_t domain, uint64_t first_k, size_t npolys, uint64_t *out);
int spiral_gpu_server_set_query_seeded(spiral_gpu_server *s, const void *msg, size_t bytes);
int spiral_gpu_server_set_pub_params_seeded(spiral_gpu_server *s, const void *msg, size_t bytes);

/* stages, asynchronous on the server stream */
int spiral_gpu_server_expand(spiral_gpu_server *s);    /* expandImproved + reorderFromStopround      */
int spiral_gpu_server_convert(spiral_gpu_server *s);   /* scalToMat x dim0, regevToGSW x nu2 (Q_neg = G2 - Q is derived where a fold round needs it) */
int spiral_gpu_server_first_dim(spiral_gpu_server *s); /* multiplyQueryByDatabase on this shard       */
int spiral_gpu_server_lift(spiral_gpu_server *s, int reduce_first); /* nttInvAndCrtLiftCiphertexts     */
/* Throughput, beyond the reference (which answers one query at a time): multiplyQueryByDatabase for the queries of n <= 8
 * servers that share one database image (an owner and its lanes, create_lane) in ONE pass over the database -- server b's
 * converted query against the image into server b's accumulators, each bit-identical to its own first_dim().  The pass runs on
 * the matrix cores (csrc/sweep_mfma.hip: both operands as signed 8-bit limbs, v_mfma_i32_16x16x64_i8, exact recombination mod
 * the primes): at config 2 two to five queries take the time of one (0.30 ms), eight take 0.39 ms.  It reads the database as "limb
 * planes": the image's holder converts its image to that form IN PLACE the first time a batch needs it (option "one_image"; no second
 * image -- see spiral_gpu_server_set_db_format) and again after the database is reloaded; option "sweep_mfma_min" = 0 turns it off.
 * Without it (that option, fewer than 128 output columns, a first dimension -- of this shard -- that is not a power of two in [64, 2048])
 * the call makes passes of two queries on the vector ALU.  Asynchronous:
 * the launch runs on servers[0]'s stream and the other lanes' streams are ordered around it with events, so per lane the
 * sequence run_pre(lane) ... first_dim_batch(all) ... run_post(lane, 0) needs no host synchronisation.  Pays where the sweep is
 * most of a query (large databases); a single query's latency is first_dim().
 * Every server is checked (same image and layout, database present, query converted since its last set_query) before anything is
 * launched: a failing call leaves no lane swept.  Geometries with fewer than 64 output columns (nu2 <= 4: 2 num_per < 64) or without the
 * packed database layout have no batched kernel: the call then runs one first_dim() per server, in order -- same results, no shared pass.
 * The lanes are ordered with hipEventRecord / hipStreamWaitEvent on their streams (a lane on servers[0]'s own stream needs none and
 * costs none): call it OUTSIDE stream capture (none of the lanes' streams may be capturing a hipGraph; run_pre / run_post capture
 * and replay their own groups either side of it). */
int spiral_gpu_server_first_dim_batch(spiral_gpu_server *const *servers, uint32_t n);
/* The same idea for the WHOLE answer: n <= 8 queries -- one per server, an owner and its lanes (create_lane), equal parameters, each with its
 * own client's public parameters and query -- as one launch sequence in which every launch carries all n queries: the expansion, conversion,
 * lift, folding and switch kernels take a query dimension (the reference runs them once per query, src/spiral.cpp:1664-1743, 1850-2025,
 * 1349-1410, inside process_crtd_query :2337-2406) and the sweep is first_dim_batch's: one pass over the database for all n on the matrix
 * cores.  A query's ~50 dependent launches outside the sweep are
 * launch-bound (~5 us each whatever they carry), so n queries cost little more than one there.  Throughput only: each query's latency is the
 * batch's.  Afterwards every server's buffers (accumulators, GSW matrices, final ciphertext, response) hold exactly what its own run_query
 * would have left.  Runs on servers[0]'s stream -- one hipGraph replay per batch when servers[0] has use_graphs on -- with the other lanes'
 * streams ordered around it by events (call it outside stream capture; ~20 us per batch and other stream: put the lanes of a batch on one stream).  Needs the default schedule on every server: own accumulators, no
 * keep_cts, no split / sharded / staged options; every server is checked before anything is launched.  n = 1 is run_query. */
int spiral_gpu_server_run_query_batch(spiral_gpu_server *const *servers, uint32_t n);
/* One query against n INSTANCES of the database.  An item larger than one plaintext -- configs[3]: 100 KB items of 15 360-byte plaintexts -- is
 * factor = ceil(item size / plaintext size) database instances (select_params.py:297-298): the client sends ONE query, the server expands and converts it
 * once and answers it against every instance -- first dimension, folding and response switch per instance, `factor` responses.  (The reference runs a
 * single instance and multiplies its first-dimension time, folding time and response size by the factor, select_params.py:409-418.)  `s` holds the query;
 * instances[k] hold the images: servers of the same geometry on the same device, each with its own database (s may be one of them; lanes are fine).
 * pre != 0 runs expansion + conversion first, else s must have converted its query (run_pre).  responses (device pointer): n x 6 x 2048 words, instance k's
 * switched response n1 x n2 at k * 6 * 2048; finals (device pointer or NULL): the folded ciphertexts likewise.  One launch sequence on s's stream, a
 * hipGraph per instance set when s has use_graphs on.  Across GPUs the instances are independent: rank r holds instances r, r + N, ... and the responses are
 * gathered -- no reduce (spiral_amd/dist.py all_gather_instance_responses). */
int spiral_gpu_server_run_query_instances(spiral_gpu_server *s, spiral_gpu_server *const *instances, uint32_t n, int pre,
                                          void *responses, void *finals);
/* the same from host buffers (as spiral_gpu_server_answer): the query in, the n responses (n x n1 x n2 x 2048 words) and optionally the folded
 * ciphertexts out; total_us (may be NULL): device time of the whole item query */
int spiral_gpu_server_answer_instances(spiral_gpu_server *s, spiral_gpu_server *const *instances, uint32_t n,
                                       const uint64_t *query, uint64_t *responses, uint64_t *finals, double *total_us);
/* Item queries of n_clients <= 8 clients, each against the same n_instances instances: run_query_batch's expansion and conversion of every client's
 * query (one launch sequence for all of them), then per instance ONE sweep of its image for all clients (a matrix-core pass where the geometry has
 * limb planes: the image is converted in place on first use, as run_query_batch does), the folding and the switch.  servers: an owner and its lanes
 * (create_lane), as in run_query_batch, each with its own public parameters and query; instances: as in run_query_instances (the owner may be one).
 * pre: as in run_query_instances.  Device outputs, client q and instance k at slot q * n_instances + k: responses (6 x 2048 words per slot), finals
 * (the folded ciphertexts, likewise; may be NULL), wire (spiral_gpu_response_wire_bytes(p, 2) bytes per slot, contiguous; may be NULL); at least one
 * of responses and wire.  Every argument is checked before anything is launched (a failing call writes no output); not during stream capture.  Runs
 * on servers[0]'s stream, the other clients' streams ordered around it by events; one hipGraph per (clients, instance images and their forms, pre,
 * outputs) with use_graphs on servers[0] -- update_db_items on an instance keeps it.  n_clients = 1 is run_query_instances' launch sequence. */
int spiral_gpu_server_run_query_batch_instances(spiral_gpu_server *const *servers, uint32_t n_clients, spiral_gpu_server *const *instances,
                                                uint32_t n_instances, int pre, void *responses, void *finals, void *wire);
/* the same from host buffers: queries[q] in (set_query's layout), responses (n_clients x n_instances x 6 x 2048 words) and / or wire
 * (n_clients x n_instances wire forms) out; total_us (may be NULL): device time of the item batch */
int spiral_gpu_server_answer_batch_instances(spiral_gpu_server *const *servers, uint32_t n_clients, spiral_gpu_server *const *instances,
                                             uint32_t n_instances, const uint64_t *const *queries, uint64_t *responses, void *wire,
                                             double *total_us);
int spiral_gpu_server_fold(spiral_gpu_server *s);      /* foldOneFurtherDimension x nu2               */
int spiral_gpu_server_finish(spiral_gpu_server *s);    /* response modulus switch, :1441-1447         */
int spiral_gpu_server_sync(spiral_gpu_server *s);
/* stage groups either side of the (possibly distributed) first-dimension reduce: run_pre = expand + convert,
 * run_post = lift + fold + finish.  With use_graphs on, each group is captured once into a hipGraph on the
 * server stream (which must not be the default stream) and replayed afterwards. */
int spiral_gpu_server_use_graphs(spiral_gpu_server *s, int on);
int spiral_gpu_server_run_pre(spiral_gpu_server *s);
/* Schedule option, on = 0 (default: one stream) or 2 (the split schedule; any other value is an error).  After round 0 the even-index and
 * the odd-index trees of expandImproved never read each other (a ciphertext is created from the one 2^r slots below it,
 * src/spiral.cpp:1709), and with stopround > 0 the evens are the first-dimension ciphertexts and the odds the GSW bits -- so the whole GSW
 * side of a query (odd tree + regevToGSW + fold keys) runs as its own launch sequence on an internal side stream, forked when the query is
 * set, beside the even tree + scalToMat + sweep on the server stream; fold / fold_local / fold_root / run_post / sync join it.  run_query
 * then issues three launch groups on two streams instead of one graph.  Needs query compression with stopround > 0 and an unsharded
 * expansion.  Results are identical, only the schedule changes; measured within noise of the in-order schedule
 * (profiles/r04_split_overlap.txt; the forms that forked only the conversion, under the sweep, were slower and are gone). */
int spiral_gpu_server_set_overlap(spiral_gpu_server *s, int on);
int spiral_gpu_server_run_post(spiral_gpu_server *s, int reduce_first);
/* the whole single-GPU answer (run_pre, first_dim, run_post(0)) as one group: with use_graphs on, one hipGraph launch
 * per query and no host-visible seam between the stages */
int spiral_gpu_server_run_query(spiral_gpu_server *s);
/* run_pre + first_dim as one group: everything a rank does before the reduce of a sharded answer */
int spiral_gpu_server_run_pre_sweep(spiral_gpu_server *s);
/* per-shard first-dimension accumulators: num_per*n1*n2*2048 packed words (p-limb | b-limb << 32, each
 * field < 2^28).  Summing the shards' buffers as uint64 (one RCCL reduce) and calling lift with
 * reduce_first = 1 gives the unsharded result.  Returns a device pointer. */
void *spiral_gpu_server_acc(spiral_gpu_server *s, size_t *bytes);
/* Distributed folding over G = 2^k ranks (reduce-scatter variant).  set_fold_ranks(G) makes the
 * sweep group its accumulators by ii mod G, so that ONE reduce-scatter of the acc buffers hands rank g the summed
 * chunk of the num_per/G ciphertexts ii = g + G*k.  fold_local lifts that chunk (device pointer, packed words) and
 * runs the first nu2-k folding rounds, leaving one raw n1 x n2 ciphertext in out_ct (device pointer, 6*2048 words);
 * after an all-gather of those G ciphertexts in rank order, fold_root runs the last k rounds and the response
 * switch on the root.  Bit-identical to lift + fold on one device. */
int spiral_gpu_server_set_fold_ranks(spiral_gpu_server *s, uint32_t n_ranks);
int spiral_gpu_server_fold_local(spiral_gpu_server *s, const void *acc_chunk, void *out_ct);
int spiral_gpu_server_fold_root(spiral_gpu_server *s, const void *gathered_cts);
/* Sharded expansion over G = 2^k ranks (the query expansion is database-independent, so a G-GPU answer would otherwise repeat all
 * of it on every GPU).  set_expand_shard(rank, G): expand() then computes only what this rank needs of expandImproved's tree
 * (src/spiral.cpp:1664-1743): the first-dimension ciphertexts of its own j-range [rank dim0/G, (rank+1) dim0/G) -- the server
 * must have been created on exactly that range -- and every G-th GSW-bit ciphertext (i = rank mod G).  All ranks need all GSW
 * bits (regevToGSW, :2315-2331), so they are exchanged: gsw_bits_pack writes this rank's block (gsw_bits_words() uint64 words,
 * device pointer), ONE all-gather of the blocks in rank order, gsw_bits_unpack stores the gathered blocks; then convert() as
 * usual.  run_expand_pack / run_unpack_convert_sweep are those steps as launch groups (hipGraphs with use_graphs on) either
 * side of the all-gather.  Results are identical to the unsharded expansion.  Needs query compression with stopround > 0. */
int spiral_gpu_server_set_expand_shard(spiral_gpu_server *s, uint32_t rank, uint32_t n_ranks);
size_t spiral_gpu_server_gsw_bits_words(spiral_gpu_server *s);
int spiral_gpu_server_gsw_bits_pack(spiral_gpu_server *s, void *block_out);
int spiral_gpu_server_gsw_bits_unpack(spiral_gpu_server *s, const void *gathered);
int spiral_gpu_server_run_expand_pack(spiral_gpu_server *s, void *bits_out);
int spiral_gpu_server_run_unpack_convert_sweep(spiral_gpu_server *s, const void *gathered);
/* the same work split so that the all-gather can overlap the database-dependent part: run_scal2mat_sweep (ScalToMat + sweep:
 * needs no GSW bit) while the all-gather is in flight, run_unpack_gsw (unpack + regevToGSW + fold keys) once it has landed */
int spiral_gpu_server_run_scal2mat_sweep(spiral_gpu_server *s);
int spiral_gpu_server_run_unpack_gsw(spiral_gpu_server *s, const void *gathered);
/* Pipelined sweep for N > 1.  The output columns of multiplyQueryByDatabase are independent (src/spiral.cpp:628-999: the i and c
 * loops enclose the j loop), so a rank can sweep them in K = 2^k stages of num_per/K ciphertexts and start the reduce-scatter of
 * a stage's accumulators while the next stage streams the database.  set_sweep_stages(K) -- after set_fold_ranks -- lays the
 * accumulator buffer out [stage][rank][ciphertext]: stage s is the contiguous 1/K of the buffer at offset s/K, and reduce-scattering
 * it over the G ranks gives rank g rows [s L/K, (s+1) L/K) of the chunk fold_local expects (L = num_per/G), so K reduce-scatters
 * of 1/K each replace the one.  first_dim_stage(s) launches stage s only; first_dim() all stages at once (same layout).
 * K must leave whole 64-column blocks per stage (K <= num_per/32, max_sweep_stages) and needs the packed database layout.
 * run_scal2mat: ScalToMat alone (run_scal2mat_sweep without the sweep), after which the stages are issued one by one. */
int spiral_gpu_server_set_sweep_stages(spiral_gpu_server *s, uint32_t n_stages);
uint32_t spiral_gpu_server_max_sweep_stages(spiral_gpu_server *s);
int spiral_gpu_server_first_dim_stage(spiral_gpu_server *s, uint32_t stage);
int spiral_gpu_server_run_scal2mat(spiral_gpu_server *s);
/* Batches of a sharded answer: the flow above (run_pre_sweep or run_expand_pack + run_unpack_convert_sweep, reduce-scatter, fold_local,
 * all-gather, fold_root) for n <= 8 clients per step, ONE collective of each kind per batch.  servers: this rank's owner (created on its j-shard,
 * set_fold_ranks(G), optionally set_expand_shard(rank, G)) and its lanes (create_lane), each with its own client's public parameters and query, the
 * same fold ranks and expansion shard.  L = num_per / G, CT = 6 x 2048 words (one n1 x n2 ciphertext).  Device buffers:
 *   acc            n x num_per x CT words, rank-major [rank g][lane b][k < L]: lane b's ciphertext ii = g + G k at (g n + b) L + k (packed words,
 *                  fields < 2^28).  One reduce-scatter(SUM) of it hands rank g its chunk [lane][k < L] (n x L x CT words).
 *   bits_out       [lane][gsw_bits_words()] (sharded expansion); one all-gather gives gathered_bits = [rank][lane][gsw_bits_words()].
 *   chunk          rank g's reduce-scattered [lane][k < L] (lazy sums of G shards; read, never written).
 *   out_cts        [lane][CT]: each lane's ciphertext after the first nu2 - log2 G rounds (raw words); one all-gather gives
 *                  gathered_cts = [rank][lane][CT].
 *   responses      optional [lane][CT]: the switched responses; wire: optional [lane][spiral_gpu_response_wire_bytes(p, 2)] bytes, their wire forms.
 * run_pre_sweep_batch: every lane's expansion and conversion in one launch sequence (ScalToMat for this rank's j-range), then ONE pass over the shard
 * for all n queries (matrix cores where the image has limb planes, else passes of two on the vector ALU) into acc.  With a sharded expansion it is
 * run_expand_pack_batch, the all-gather, then run_unpack_convert_sweep_batch.  fold_local_batch lifts each lane's chunk and runs the first
 * nu2 - log2 G rounds for all lanes; fold_root_batch (the root rank) the last log2 G rounds and the switch: afterwards every lane's own buffers
 * (SPIRAL_GPU_BUF_FINAL, SPIRAL_GPU_BUF_RESPONSE, read_response_wire) hold exactly what its run_query on the unsharded database would have left.
 * set_fold_ranks(1) is the root-fold form: acc is [lane][num_per], reduce(SUM) to the root, fold_local_batch there runs every round and
 * fold_root_batch only the switch.  The library issues no collective.  Every argument and lane is checked before anything is launched (a failing
 * call writes nothing); not during stream capture.  Runs on servers[0]'s stream, the other lanes' streams ordered around it by events; with
 * use_graphs on servers[0] each call is captured once per (lanes, buffers, image form) and replayed (update_db_items keeps the capture). */
int spiral_gpu_server_run_pre_sweep_batch(spiral_gpu_server *const *servers, uint32_t n, void *acc);
int spiral_gpu_server_run_expand_pack_batch(spiral_gpu_server *const *servers, uint32_t n, void *bits_out);
int spiral_gpu_server_run_unpack_convert_sweep_batch(spiral_gpu_server *const *servers, uint32_t n, const void *gathered_bits, void *acc);
int spiral_gpu_server_fold_local_batch(spiral_gpu_server *const *servers, uint32_t n, const void *chunk, void *out_cts);
int spiral_gpu_server_fold_root_batch(spiral_gpu_server *const *servers, uint32_t n, const void *gathered_cts, void *responses, void *wire);
/* Batches on a COLUMN-sharded database (create_column_shard): a rank's whole local share for n <= 8 clients in one call.  servers: this rank's column
 * shard owner and its lanes, each with its client's public parameters and query.  One launch sequence: every lane's expansion and conversion (the
 * sequence of run_pre_sweep_batch; the whole first dimension on every rank), ONE pass over the shard for all lanes straight into each lane's own
 * accumulators (matrix cores where the image has limb planes -- converted in place on first use, as a batch does --, else the vector-ALU passes),
 * the first nu2 - log2 G fold rounds on those L ciphertexts, and each lane's surviving ciphertext to out_cts = [lane][CT], fold_local_batch's
 * layout.  There is no rank-major buffer, no reduce and no chunk copy.  Then, by the caller: one all-gather of out_cts into [rank][lane][CT] and
 * fold_root_batch on the root rank (with G = 1: fold_root_batch on out_cts itself).  n = 1 is the single-query flow.  Every argument and lane is
 * checked before anything is launched (a failing call writes nothing); not during stream capture.  Runs on servers[0]'s stream, the other lanes'
 * streams ordered around it by events; with use_graphs on servers[0] it is one graph per (lanes, out_cts, image form), and update_db_items keeps
 * the capture.  The counter "mfma_sweeps" grows by one per call whose pass ran on the matrix cores, launched or replayed. */
int spiral_gpu_server_run_column_batch(spiral_gpu_server *const *servers, uint32_t n, void *out_cts);
/* make the sweep write into caller-owned device memory (e.g. a torch tensor) */
int spiral_gpu_server_set_acc(spiral_gpu_server *s, void *device_ptr);

/* whole path for one query: set_query, expand, convert, first_dim, lift, fold, finish, sync.
 * final_ct: raw n1 x n2 (may be NULL); response: rescaled n1 x n2 (may be NULL).
 * stage_us (may be NULL): [0] expansion [1] conversion [2] first-dimension multiply (sweep + lift)
 * [3] folding [4] response switch [5] sweep kernel alone [6] total device time [7] ScalToMat share of [1],
 * the reference's buckets of src/spiral.cpp:246-257, measured with HIP events on the server stream. */
int spiral_gpu_server_answer(spiral_gpu_server *s, const uint64_t *query, uint64_t *final_ct,
                             uint64_t *response, double stage_us[8]);
/* the same without touching host memory: the query must have been set; results stay on the device */
int spiral_gpu_server_answer_resident(spiral_gpu_server *s, double stage_us[8]);

/* read back intermediates in reference layouts (stage parity tests) */
enum spiral_gpu_buffer {
    SPIRAL_GPU_BUF_EXPANDED = 0, /* n_bits cts n0 x 1 NTT, in the order scalToMat/regevToGSW consume them */
    SPIRAL_GPU_BUF_CTS = 1,      /* (j_end-j_begin) cts n1 x n0 NTT = expansionLocals.cts (needs keep_cts)  */
    SPIRAL_GPU_BUF_GSW = 2,      /* nu2 matrices n1 x m2 NTT, reference's reversed order (:2324)           */
    SPIRAL_GPU_BUF_ACC = 3,      /* num_per cts n1 x n2 NTT: the sweep output                              */
    SPIRAL_GPU_BUF_RAW = 4,      /* num_per cts n1 x n2 raw: after lift / after folding rounds             */
    SPIRAL_GPU_BUF_FINAL = 5,    /* n1 x n2 raw                                                            */
    SPIRAL_GPU_BUF_RESPONSE = 6, /* n1 x n2 rescaled                                                       */
    SPIRAL_GPU_BUF_QUERY = 7     /* the resident query: n_query_cts cts n0 x 1 NTT (set_query / set_query_wire) */
};
int spiral_gpu_server_keep_cts(spiral_gpu_server *s, int on);
size_t spiral_gpu_server_buffer_words(spiral_gpu_server *s, int which);
int spiral_gpu_server_read(spiral_gpu_server *s, int which, uint64_t *out);
/* the last answer's response in its wire form (see spiral_gpu_response_wire_bytes above): packed on the device, downloaded
 * into `out` (capacity in bytes; fails when it is smaller than the wire form) */
int spiral_gpu_server_read_response_wire(spiral_gpu_server *s, void *out, size_t capacity);
/* overwrite the lifted ciphertexts (raw [num_per][n1][n2][N]) -- lets a test drive fold() alone */
int spiral_gpu_server_write_raw(spiral_gpu_server *s, const uint64_t *raw_cts);
/* overwrite the accumulators (NTT [num_per][n1][n2][2][N], what read(SPIRAL_GPU_BUF_ACC) returns; residues below 4m as for
 * ntt_forward) -- lets a test drive lift(), fold() and run_post() on chosen ciphertexts: with acc = to_ntt(raw), raw < Q, the lift gives
 * raw back exactly */
int spiral_gpu_server_write_acc(spiral_gpu_server *s, const uint64_t *acc_ref);

/* measurement helper: average duration (ms) of the sweep kernel alone over `iters` launches, timed
 * with HIP events on the server stream */
int spiral_gpu_server_time_sweep(spiral_gpu_server *s, int iters, float *avg_ms);
/* the same for first_dim_batch's kernel launch alone: the (already converted) queries of the n servers, `iters` launches */
int spiral_gpu_server_time_sweep_batch(spiral_gpu_server *const *servers, uint32_t n, int iters, float *avg_ms);
/* algorithmic bytes of one sweep on this shard: DB + query records + accumulators */
uint64_t spiral_gpu_server_sweep_bytes(spiral_gpu_server *s);
/* bytes one launch actually has to move on this device: the database in its device layout (two 28-bit residues
 * packed in 7 bytes), the query records and the accumulators -- below the algorithmic figure above */
uint64_t spiral_gpu_server_sweep_device_bytes(spiral_gpu_server *s);

/* ------------------------------------------------------------------------------------------------
 * SpiralPack / SpiralStreamPack (`--high-rate`, src/testing.cpp): base_dim x 1 scalar Regev ciphertexts,
 * 1 x 1 plaintexts, out_n^2 database trials packed into one (out_n+1) x out_n response.
 * ------------------------------------------------------------------------------------------------ */
typedef struct spiral_gpu_pack_shape {
    uint32_t dim0, num_per, ell, g, stopround;
    uint32_t n_left, n_right; /* expansion key-switching matrices n0 x t_exp / n0 x t_exp_right (0 with direct upload) */
    uint32_t n_query_cts;     /* 1, or dim0 + nu2*2*ell uploaded ciphertexts */
    uint32_t trials;          /* out_n^2 */
    uint64_t qprime;
} spiral_gpu_pack_shape;
typedef struct spiral_gpu_pack_server spiral_gpu_pack_server;
int spiral_gpu_pack_get_shape(const spiral_gpu_params *p, uint32_t out_n, spiral_gpu_pack_shape *out);

/* pack, include/testing.h:36-42, src/testing.cpp:198.  v_ct: out_n^2 raw base_dim x 1 ciphertexts; v_W: out_n
 * matrices (out_n+1) x m_conv NTT; result: (out_n+1) x out_n NTT */
int spiral_gpu_pack(uint64_t *result, uint32_t out_n, uint32_t m_conv, const uint64_t *v_ct, const uint64_t *v_W);
/* fastMultiplyQueryByDatabaseDim1, src/testing.cpp:364.  db: convertDb's layout (:316-340); v_firstdim:
 * reorientCiphertextsDim1's layout (:342-362); out: num_per ciphertexts base_dim x 1 NTT */
int spiral_gpu_fast_multiply_query_by_database_dim1(uint64_t *out, const uint64_t *db, const uint64_t *v_firstdim,
                                                    size_t dim0, size_t num_per);
/* The same for n <= 8 queries against `trials` database images in ONE pass, the way a batch of clients sweeps a server's trials (no reference
 * counterpart): dbs = the trials' images one after the other, each in the layout above; v_firstdims = the n queries' buffers one after the other;
 * outs = [n][trials][num_per] ciphertexts base_dim x 1 NTT, each equal to the one-query call's for that (query, trial).  Where the geometry has a
 * limb-plane form (spiral_gpu_pack_has_limb_form: 16 ciphertexts per slot and more -- or 8 with option "pack_pair_blocks" -- and a power-of-two first
 * dimension in [128, 4096]) the pass runs on the matrix cores (csrc/sweep_mfma.hip; "mfma_sweeps" counts it), else as one vector-ALU sweep per query.
 * The device accumulators are followed by guard words that the call checks: a sweep that stored beyond its last trial fails the call ("wrote past
 * the last trial").  Fails, before any device call, for n = 0 or > 8, trials = 0, an odd or zero dim0, num_per = 0. */
int spiral_gpu_fast_multiply_queries_by_database_dim1(uint64_t *outs, const uint64_t *dbs, const uint64_t *v_firstdims, size_t n,
                                                      size_t trials, size_t dim0, size_t num_per);

/* resident server for testHighRate's server half (src/testing.cpp:1009-1081) */
int spiral_gpu_pack_server_create(const spiral_gpu_params *p, uint32_t out_n, int device, spiral_gpu_pack_server **out);
/* N GPUs (pack variant): the out_n^2 trials are independent up to the packing step, so the ranks split THEM -- a server
 * for trials [trial0, trial1) holds only those database images (trial indices in load_db / load_db_items / read_acc stay global).
 * Per query: every rank runs fold_trials (expansion + conversion, replicated; its trials' sweeps and folding; leaves their folded
 * ciphertexts, [n_local][2][N] raw words, in the caller's device buffer), ONE all-gather of out_n^2 x 32 KiB collects them in trial
 * order, the root runs pack_gathered (pack + modulus switch).  No reduction of accumulators is needed: the j-shard + reduce of the
 * base path would move out_n^2 x num_per x 32 KiB here (128 MiB at configs[4]) over point-to-point xGMI, this moves 512 KiB.
 * (0, 0) = all trials = spiral_gpu_pack_server_create.  set_stream: run on the caller's stream (the one its collectives use). */
int spiral_gpu_pack_server_create_sharded(const spiral_gpu_params *p, uint32_t out_n, int device, uint32_t trial0, uint32_t trial1,
                                          spiral_gpu_pack_server **out);
int spiral_gpu_pack_server_set_stream(spiral_gpu_pack_server *s, void *hip_stream);
int spiral_gpu_pack_server_fold_trials(spiral_gpu_pack_server *s, const uint64_t *query, void *folded_dev);
/* stage times (as answer's stage_us) of the last answer or fold_trials from the events between its stages; synchronises */
int spiral_gpu_pack_server_stage_us(spiral_gpu_pack_server *s, double stage_us[8]);
int spiral_gpu_pack_server_pack_gathered(spiral_gpu_pack_server *s, const void *gathered_dev, uint64_t *response, uint64_t *packed_ct);
void spiral_gpu_pack_server_destroy(spiral_gpu_pack_server *s);
/* the out_n^2 trial databases: seeded explicit data generated on the device (coefficient z of item i of trial t =
 * splitmix64(seed ^ ((t*n + i)*N + z)) % p_db), one trial from host memory in convertDb's layout, or arbitrary words */
int spiral_gpu_pack_server_gen_db(spiral_gpu_pack_server *s, uint64_t seed);
int spiral_gpu_pack_server_load_db(spiral_gpu_pack_server *s, uint32_t trial, const uint64_t *db);
int spiral_gpu_pack_server_fill_db_random(spiral_gpu_pack_server *s, uint64_t seed);
/* raw ingest of one trial (src/testing.cpp:845-869 + convertDb :316-340 on the device): 1 x 1 plaintexts of 2048
 * coefficients, bit-packed as for spiral_gpu_server_load_db_items */
int spiral_gpu_pack_server_load_db_items(spiral_gpu_pack_server *s, uint32_t trial, const void *items, uint32_t coeff_bits,
                                         uint64_t first_item, uint64_t n_items);
/* spiral_gpu_server_update_db_items for one trial of this server's trial range (1 x 1 plaintexts of 2048 coefficients): in place, in the
 * trial image's current form, on this server's stream, with the same rules for failure and ordering; any other trial fails. */
int spiral_gpu_pack_server_update_db_items(spiral_gpu_pack_server *s, uint32_t trial, const void *items, uint32_t coeff_bits,
                                           const uint64_t *item_ids, uint64_t n);
/* spiral_gpu_server_read_db_items / _at for one trial of this server's trial range: 1 x 1 plaintexts (polys = 1, item k at byte
 * k * 256 * coeff_bits), from the trial image in its current form -- packed or plain, or limb planes in the wide, narrow and 8-column pair
 * forms -- with the same layout, validity rule, failures and ordering; the owner or a lane may call; any other trial fails, as for the update.
 * (A SpiralPack server holds whole trials: there is no j-shard to skip.) */
int spiral_gpu_pack_server_read_db_items(spiral_gpu_pack_server *s, uint32_t trial, void *items, uint32_t coeff_bits, uint64_t first_item,
                                         uint64_t n_items);
int spiral_gpu_pack_server_read_db_items_at(spiral_gpu_pack_server *s, uint32_t trial, void *items, uint32_t coeff_bits,
                                            const uint64_t *item_ids, uint64_t n);
/* spiral_gpu_server_fingerprint_items / _at over this server's trial images ("Fingerprints": polys = trials, polynomial q = the item's plaintext in
 * trial q), each read in its current form; there is no `trial` argument.  A trial-sharded server sums the polynomials of its own trial range
 * [t0, t0 + nt) only, and the partials of all ranks add (spiral_gpu_fingerprint_add) to the whole fingerprints.  The owner or a lane may call. */
int spiral_gpu_pack_server_fingerprint_items(spiral_gpu_pack_server *s, const uint64_t *key, uint64_t first_item, uint64_t n_items,
                                             uint64_t *per_item, uint64_t *combined);
int spiral_gpu_pack_server_fingerprint_items_at(spiral_gpu_pack_server *s, const uint64_t *key, const uint64_t *item_ids, uint64_t n,
                                                uint64_t *per_item, uint64_t *combined);
/* The tracked fingerprint ("Fingerprints", Tracked) over this server's trial images: the table holds nt words per item, q = t0 .. t0 + nt - 1; a trial
 * shard's weights start at r^(2048 t0) and its F is a partial.  update_db_items of any trial and update_records keep it current. */
int spiral_gpu_pack_server_fingerprint_track(spiral_gpu_pack_server *s, const uint64_t *key, const uint64_t *poly_sums);
int spiral_gpu_pack_server_fingerprint_untrack(spiral_gpu_pack_server *s);
int spiral_gpu_pack_server_fingerprint_tracked(spiral_gpu_pack_server *s, uint64_t *key_out, uint64_t *combined, uint64_t *n_updates);
int spiral_gpu_pack_server_fingerprint_tracked_polys(spiral_gpu_pack_server *s, uint64_t first_item, uint64_t n_items, uint64_t *poly_sums);
int spiral_gpu_pack_server_fingerprint_scrub(spiral_gpu_pack_server *s, uint64_t first_item, uint64_t n_items, uint64_t *n_bad,
                                             uint64_t *first_bad_item, uint32_t *first_bad_poly);
/* Records in the SpiralPack layout ("Records", SpiralPack).  The arguments and the contracts are those of spiral_gpu_server_load_records,
 * _update_records, _read_records and _read_records_at, `instance` included; there is no `trial` argument: a record names its bytes, the layout
 * says which trial images hold them.
 * load_records goes through load_db_items, one ingest per trial.
 * update_records: in place, in each trial image's CURRENT form (packed or plain, limb planes in the wide, narrow and pair forms), no conversion and
 * no new epoch; the owner only (a lane is refused), refused inside a stream capture, every check before anything is launched, a failing call leaves
 * every trial image byte-identical.  ONE upload, ONE read-modify-write launch (one workgroup per touched polynomial = (trial, item)) and ONE scatter
 * launch, whatever number of trials the records touch.  It waits for this server's stream only when a polynomial had to be read (one that the
 * call's records cover in part).
 * read_records / _at: any server that references the image, lanes and shard lanes included; ids need not be distinct; staged in passes of option
 * db_stage_bytes, one launch and one copy per pass; returns synchronised.
 * A trial-sharded server (create_sharded) holds every item but only the polynomials of its trials [trial0, trial1): it writes and reads the bytes
 * that lie in them and skips the rest, so the shards of a database fill one buffer between them, and a record that straddles two shards is updated
 * by one call on each. */
int spiral_gpu_pack_server_load_records(spiral_gpu_pack_server *s, const void *records, uint64_t record_bytes, uint32_t instance,
                                        uint64_t first_record, uint64_t n_records);
int spiral_gpu_pack_server_update_records(spiral_gpu_pack_server *s, const void *records, uint64_t record_bytes, uint32_t instance,
                                          const uint64_t *record_ids, uint64_t n);
int spiral_gpu_pack_server_read_records(spiral_gpu_pack_server *s, void *records, uint64_t record_bytes, uint32_t instance, uint64_t first_record,
                                        uint64_t n_records);
int spiral_gpu_pack_server_read_records_at(spiral_gpu_pack_server *s, void *records, uint64_t record_bytes, uint32_t instance,
                                           const uint64_t *record_ids, uint64_t n);
/* Keyed records for a SpiralPack parameter set and server ("Keyed records", SpiralPack), out_n in 1 .. 16.  layout_of and hash are host only.  The
 * server calls take the base calls' arguments and keep their contracts: load, put and delete are the owner's (a lane refuses); get and stats work
 * on any server that references the image, lanes included, on its own stream; refused inside a capture; a failing call leaves every trial image
 * byte-identical; the images keep their current form (packed or plain, limb planes, the pair form), no epoch, no re-captured graph; tracked
 * fingerprints stay current; a key whose two buckets are full fails the call with the base server's message.  The probe reads polynomial 0 of a
 * bucket from trial image 0; tag and value go through pack_server_update_records' path -- a put that touches many trials is still one upload, one
 * read-modify-write launch and one scatter launch -- and pack_server_read_records' path.  load places every key on the host first (a key that
 * cannot be placed fails the call before anything else is built), then builds the item stream a pass of at most 2^14 buckets at a time -- host
 * memory beyond the caller's keys and values is that pass (512 MiB at 32 KiB buckets) and 24 bytes per key, not the table -- and loads polynomial t
 * of each bucket into trial t through pack_server_load_db_items.  A server that holds fewer than all trials (create_sharded, create_shard_lane) refuses every
 * call by name. */
int spiral_gpu_pack_kv_layout_of(const spiral_gpu_params *p, uint32_t out_n, uint64_t value_bytes, spiral_gpu_kv_layout *out);
int spiral_gpu_pack_kv_hash(const spiral_gpu_params *p, uint32_t out_n, const void *table_key16, const void *key, uint64_t key_bytes, uint64_t *tag,
                            uint64_t *b1, uint64_t *b2);
int spiral_gpu_pack_server_kv_load(spiral_gpu_pack_server *s, const void *table_key16, const void *keys, uint64_t key_bytes, const void *values,
                                   uint64_t value_bytes, uint64_t n);
int spiral_gpu_pack_server_kv_put(spiral_gpu_pack_server *s, const void *table_key16, const void *keys, uint64_t key_bytes, const void *values,
                                  uint64_t value_bytes, uint64_t n);
int spiral_gpu_pack_server_kv_delete(spiral_gpu_pack_server *s, const void *table_key16, const void *keys, uint64_t key_bytes, uint64_t value_bytes,
                                     uint64_t n, uint64_t *n_deleted);
int spiral_gpu_pack_server_kv_get(spiral_gpu_pack_server *s, const void *table_key16, const void *keys, uint64_t key_bytes, void *values,
                                  uint64_t value_bytes, uint64_t n, uint8_t *found);
int spiral_gpu_pack_server_kv_stats(spiral_gpu_pack_server *s, uint64_t value_bytes, uint64_t first_bucket, uint64_t n_buckets,
                                    spiral_gpu_kv_stats *out);
/* "Listing" on a SpiralPack server: the base calls' arguments and contract.  The headers are read from trial image 0; an entry's value spans the trial
 * images and comes back through pack_server_read_records' path.  A trial shard and its shard lane refuse by name. */
int spiral_gpu_pack_server_kv_scan(spiral_gpu_pack_server *s, uint64_t value_bytes, uint64_t first_bucket, uint64_t n_buckets,
                                   spiral_gpu_kv_entry *entries, void *values, uint64_t max_entries, uint64_t *n_entries);
int spiral_gpu_pack_server_kv_scan_at(spiral_gpu_pack_server *s, uint64_t value_bytes, const uint64_t *buckets, uint64_t n_buckets,
                                      spiral_gpu_kv_entry *entries, void *values, uint64_t max_entries, uint64_t *n_entries);
/* W_exp_left / W_exp_right (expansion only), V base_dim x base_dim*t_conv (expansion only), v_W out_n x ((out_n+1) x t_conv).  A null pointer
 * among those the geometry needs fails before anything is written: the previous public parameters stay (as for spiral_gpu_server_set_pub_params). */
int spiral_gpu_pack_server_set_pub_params(spiral_gpu_pack_server *s, const uint64_t *w_left, const uint64_t *w_right,
                                          const uint64_t *v, const uint64_t *v_w);
/* response: (out_n+1) x out_n raw, row 0 mod q', rows 1.. mod 4p; packed_ct (may be NULL): the (out_n+1) x out_n NTT
 * ciphertext before the modulus switch.  stage_us (may be NULL): [0] expansion [1] conversion [2] first dimension
 * (out_n^2 sweeps + lift) [3] folding [4] packing + modulus switch [5] the sweep kernels alone [6] total. */
int spiral_gpu_pack_server_answer(spiral_gpu_pack_server *s, const uint64_t *query, uint64_t *response, uint64_t *packed_ct,
                                  double stage_us[8]);
/* the last answer's response in its wire form ((out_n+1) x out_n, spiral_gpu_response_wire_bytes(p, out_n) bytes) */
int spiral_gpu_pack_server_read_response_wire(spiral_gpu_pack_server *s, void *out, size_t capacity);
/* the first-dimension accumulators of one trial of the last answer (fastMultiplyQueryByDatabaseDim1's output, :1050):
 * num_per ciphertexts base_dim x 1, NTT form (tests) */
int spiral_gpu_pack_server_read_acc(spiral_gpu_pack_server *s, uint32_t trial, uint64_t *out);
uint64_t spiral_gpu_pack_server_sweep_bytes(spiral_gpu_pack_server *s); /* algorithmic bytes of ONE trial's sweep */
/* Batches on the pack path, beyond the reference (one query per call).  create_lane: a new server with the owner's parameters, out_n and
 * device that sweeps the OWNER's trial images and has its own public parameters, query and intermediates (loads through a lane fail; the
 * images are counted and go with their last reference, the owner's or a lane's; trial-sharded owners have no lanes).
 * answer_batch: n <= 8 servers -- an owner and/or its lanes, in any order, each with its own client's public parameters -- answer queries[b] each:
 * expansion and conversion, ONE first-dimension pass over every trial image for all n queries, then folding, packing and the modulus switch, all on
 * servers[0]'s stream (what the other servers' streams hold is ordered in front, what follows on them behind); returns synchronised.  From option
 * "pack_batch_lanes" clients on (default 0: never, set it to 2 for every batch) this is the LANE FORM: every launch of the sequence carries all n clients in its grid -- one
 * expansion, one conversion, the pass, one folding, one packing and switch, as many launches as one answer has; below it the stages other than the pass
 * run per lane, one client after another.  Afterwards every lane's buffers (read_acc of every trial, read_response_wire) hold exactly
 * what its own answer would have left.  responses[b] / packed_cts[b] (or the arrays) may be NULL.  stage_us (may be NULL): [0] expansion [1]
 * conversion [3] folding [4] packing, summed over the lanes (lane form: the whole-batch intervals between servers[0]'s events), [2] = [5] the shared
 * sweep, [6] total, [7] n.  The lane form records events on servers[0] only: afterwards spiral_gpu_pack_server_stage_us of servers[0] gives the batch's
 * intervals, and of any other lane of the call it fails with a message (until that lane answers alone or as servers[0] again) -- after the per-lane form
 * it gives that lane's own share.  The same holds for the clients of a lane-form answer_batch_instances.  Every query is uploaded before the first
 * launch, so [6] (and answer_batch_instances' total_us) is device time of the launches alone, in every form of the queries.  Every server is checked before anything
 * is launched (n in 1 .. 8, no duplicates, same image, parameters, database and public parameters present; and, in every multi-server SpiralPack call --
 * answer_batch in either form, time_sweep_batch, answer_batch_instances -- that every server's buffers are laid out as servers[0]'s, which equal
 * parameters guarantee): a failing check leaves every lane's
 * previous results intact.  n = 1 is answer.
 * The shared pass runs on the matrix cores (csrc/sweep_mfma.hip, the base path's kernel with 2-row records) from the LIMBS form of the trial
 * images, where that form exists (spiral_gpu_pack_has_limb_form): at least 16 ciphertexts per slot (nu2 >= 4) -- or exactly 8 (nu2 = 3) with option
 * "pack_pair_blocks" = 1 -- and a first dimension that is a power of two in [128, 4096] (nu1 = 7 .. 12), whatever out_n.  With 16, 32 or 64
 * ciphertexts per slot -- the large-plaintext sets, many trials of few columns -- a workgroup of the pass takes columns of several trials at once;
 * with 8 -- the small-item sets -- every wave of it takes the columns of two adjacent trials (the pair form); from 128 up, of one trial.  The first
 * batch on such a geometry converts the images in place (set_db_format); elsewhere (8 ciphertexts per slot with the option at 0, 4 or fewer, a first
 * dimension below 128) the batch sweeps once per lane on the vector ALU -- same results, no shared pass.  A single answer on a LIMBS image sweeps it with the one-query instance of the same kernel
 * (bit-identical).
 * has_limb_form: 1 when a batch on this geometry shares its pass (so collecting clients into a batch pays), 0 when not, -1 (spiral_gpu_last_error)
 * for bad parameters; a function of the parameters and of ONE option, "pack_pair_blocks" as it is when asked (8 ciphertexts per slot only), no GPU needed.
 * set_db_format / db_format / db_device_bytes: as spiral_gpu_server_set_db_format, for the out_n^2 trial images (on the owner, not a lane; LIMBS
 * fails where has_limb_form is 0; a trial-sharded server converts the images of its own trials; every loader leaves a correct image whatever form
 * it finds; a conversion that fails partway leaves no database loaded).
 * time_sweep_batch: the batched sweep alone, iters times with the lanes' current records (each answered once), average ms by device events. */
int spiral_gpu_pack_has_limb_form(const spiral_gpu_params *p, uint32_t out_n);
int spiral_gpu_pack_server_create_lane(spiral_gpu_pack_server *owner, spiral_gpu_pack_server **out);
int spiral_gpu_pack_server_answer_batch(spiral_gpu_pack_server *const *servers, uint32_t n, const uint64_t *const *queries,
                                        uint64_t *const *responses, uint64_t *const *packed_cts, double stage_us[8]);
/* Batches of a TRIAL-SHARDED answer (create_sharded above): n <= 8 clients per rank, one pass over the rank's trial images for all of them, ONE
 * all-gather, one pack on the root.  CT below = 2 x 2048 raw words, one folded ciphertext.
 * create_shard_lane: as create_lane, of an owner that holds the trials [t0, t0 + nt) only -- the owner's parameters, out_n, device and trial range,
 * the owner's images, its own keys, query and intermediates.  The owner must own its image and have a database loaded; loads, updates and
 * set_db_format through the lane fail as through any lane, read_db_items* and read_acc of a trial in range work, the images go with their last
 * reference.  Of an owner that holds every trial the result is an ordinary lane.  Shard lanes of a trial-sharded owner are taken by the two calls
 * below and by bind_keys only (every rank holds every client's keys: the store is how a shard's lanes change clients between batches); every other
 * multi-server call refuses them, as it refuses their owner ("trial-sharded").
 * fold_trials_batch (every rank, before the all-gather): servers = n in 1 .. 8 distinct servers, an owner and/or its shard lanes in any order, each
 * with its own public parameters; form = 0 (NTT-form polynomials, bytes_each ignored), SPIRAL_GPU_FORM_WIRE or SPIRAL_GPU_FORM_SEEDED (every query
 * bytes_each long).  Every argument is checked and every query taken before anything is launched: a bad query leaves every lane as it was.  Then
 * answer_batch's front half over the LOCAL trials: expansion and conversion (the lane form from option "pack_batch_lanes" clients on, per lane
 * below it), with n >= 2 the in-place conversion of this shard's images where the geometry has limb planes, ONE first-dimension pass for all lanes,
 * the folding.  Lane b's nt folded ciphertexts are left at folded_dev + (b * nt + k) * CT, k < nt -- the block [lane][k], each ciphertext what the
 * lane's own fold_trials writes; nothing else of folded_dev is written.  The call runs on servers[0]'s stream with the other lanes' streams (and
 * the owner's, when it is not listed) ordered around it and is ASYNCHRONOUS like fold_trials: the caller's collective follows on that stream.
 * Not during stream capture.  Afterwards every lane's read_acc of a local trial is its own fold_trials'.  n = 1 is fold_trials.
 * pack_gathered_batch (the root, after the all-gather): cuts[0 .. n_ranks] are the ranks' trial ranges, cuts[0] = 0 < cuts[1] < ... < cuts[n_ranks] =
 * out_n^2.  gathered_dev (16-byte aligned) holds n_ranks blocks at a stride of block_cts ciphertexts, block r = rank r's [lane][k < cuts[r + 1] -
 * cuts[r]]; block_cts >= n x the longest range, and the surplus of a block is padding that is never read -- unequal ranges go through an equal-size
 * all-gather.  servers: any n lanes of one image on the root, shard lanes or ordinary (the root's own trial range plays no part), each with its own
 * public parameters; lane b is the client that was lane b on every rank.  ONE launch regroups the blocks into every lane's trial order, then ONE
 * lane-aware pack and switch follows: one launch more than pack_gathered, whatever n and n_ranks.  responses[b] / packed_cts[b] (or the arrays)
 * may be NULL; wire (may be NULL): n x spiral_gpu_response_wire_bytes(p, out_n) contiguous host bytes, lane b's wire form at b x that, from one
 * launch and one copy.  At least one of the three must be given.  Every argument is checked before anything is launched: a refused call writes
 * nothing and leaves every lane's previous results intact.  Returns synchronised; afterwards every lane's response, packed ciphertext and
 * read_response_wire equal its own pack_gathered on its own trial-ordered ciphertexts. */
int spiral_gpu_pack_server_create_shard_lane(spiral_gpu_pack_server *owner, spiral_gpu_pack_server **out);
int spiral_gpu_pack_server_fold_trials_batch(spiral_gpu_pack_server *const *servers, uint32_t n, int form, const void *const *queries,
                                             size_t bytes_each, void *folded_dev);
int spiral_gpu_pack_server_pack_gathered_batch(spiral_gpu_pack_server *const *servers, uint32_t n, const void *gathered_dev,
                                               const uint32_t *cuts, uint32_t n_ranks, uint64_t block_cts, uint64_t *const *responses,
                                               uint64_t *const *packed_cts, void *wire);
/* SpiralPack from the wire form (see spiral_gpu_query_wire_bytes above): the sizes of a query and of the public parameters for `out_n`, the
 * public parameters as one message, and answer / answer_batch with the queries in their wire form (there is no set_query on this path).
 * answer_batch_wire checks every argument, each query's byte count included, before anything is uploaded, and runs the batch only when every
 * query decoded cleanly: a bad query leaves every lane's previous results intact. */
size_t spiral_gpu_pack_query_wire_bytes(const spiral_gpu_params *p, uint32_t out_n);
size_t spiral_gpu_pack_pub_params_wire_bytes(const spiral_gpu_params *p, uint32_t out_n);
int spiral_gpu_pack_server_set_pub_params_wire(spiral_gpu_pack_server *s, const void *wire, size_t bytes);
int spiral_gpu_pack_server_answer_wire(spiral_gpu_pack_server *s, const void *query_wire, size_t bytes, uint64_t *response,
                                       uint64_t *packed_ct, double stage_us[8]);
int spiral_gpu_pack_server_answer_batch_wire(spiral_gpu_pack_server *const *servers, uint32_t n, const void *const *query_wires,
                                             size_t bytes_each, uint64_t *const *responses, uint64_t *const *packed_cts,
                                             double stage_us[8]);
/* An item larger than one plaintext is factor = ceil(item size / plaintext size) database INSTANCES (select_params.py:297-298): n_instances pack
 * servers, each holding all out_n^2 trial images of its own database.  n_clients <= 8 clients -- servers[q]: an owner and its lanes (create_lane), as in
 * answer_batch, each with its own public parameters -- send one query each, and every client gets one packed response per instance: slot
 * q * n_instances + k is what answer on a server sweeping instance k's images would return for client q's public parameters and query.  Per call: the
 * expansion and conversion once per client (not per instance; from option "pack_batch_lanes" clients on, all clients' in one lane-aware launch
 * sequence, as answer_batch's); per instance ONE first-dimension pass over its images for all clients (the
 * matrix-core pass of answer_batch where the geometry has limb planes: with two or more clients each instance image is converted in place on first
 * use); then per client and group of G instances ONE folding, packing, switch and wire-form sequence whose launches carry the whole group.  Option
 * "pack_item_group" sets G (0: automatic -- the largest G whose arenas fit a quarter of the free device memory; an allocation that fails halves G,
 * G = 1 uses only the clients' own buffers); the arenas stay on the client servers for the next call and go with destroy.  The clients' own image
 * is read only where it is one of the instances (typically the owner is instance 0).
 * Host buffers: queries[q] as answer's; responses: (out_n + 1) x out_n x 2048 words per slot (answer's layout); wire:
 * spiral_gpu_response_wire_bytes(p, out_n) bytes per slot, contiguous; at least one of the two; total_us (may be NULL): device time of the call.
 * Every argument is checked before anything is uploaded or launched (clients as answer_batch, less the owner's database; instances non-null, same
 * parameters, out_n and device, all trials, a database loaded; the queries and their size; an output): a failing check writes no output.  The _wire
 * form decodes every query first and runs only when all of them decoded cleanly.  Runs on servers[0]'s stream; the other clients' streams and every
 * instance's (and its holder's) stream are ordered in front of it with events, and wait for it afterwards, so an update_db_items enqueued on an
 * instance before the call is seen by it.  Returns synchronised.  n_clients = n_instances = 1 gives answer's words. */
int spiral_gpu_pack_server_answer_batch_instances(spiral_gpu_pack_server *const *servers, uint32_t n_clients,
                                                  spiral_gpu_pack_server *const *instances, uint32_t n_instances,
                                                  const uint64_t *const *queries, uint64_t *responses, void *wire, double *total_us);
int spiral_gpu_pack_server_answer_batch_instances_wire(spiral_gpu_pack_server *const *servers, uint32_t n_clients,
                                                       spiral_gpu_pack_server *const *instances, uint32_t n_instances,
                                                       const void *const *query_wires, size_t bytes_each, uint64_t *responses,
                                                       void *wire, double *total_us);
/* SpiralPack from the seeded form (see spiral_gpu_query_seeded_bytes above): the sizes, the public parameters as one seeded message, and answer /
 * answer_batch / answer_batch_instances with each query a seeded message of bytes_each bytes -- otherwise exactly their _wire forms. */
size_t spiral_gpu_pack_query_seeded_bytes(const spiral_gpu_params *p, uint32_t out_n);
size_t spiral_gpu_pack_pub_params_seeded_bytes(const spiral_gpu_params *p, uint32_t out_n);
int spiral_gpu_pack_server_set_pub_params_seeded(spiral_gpu_pack_server *s, const void *msg, size_t bytes);
int spiral_gpu_pack_server_answer_seeded(spiral_gpu_pack_server *s, const void *query_msg, size_t bytes, uint64_t *response, uint64_t *packed_ct,
                                         double stage_us[8]);
int spiral_gpu_pack_server_answer_batch_seeded(spiral_gpu_pack_server *const *servers, uint32_t n, const void *const *query_msgs, size_t bytes_each,
                                               uint64_t *const *responses, uint64_t *const *packed_cts, double stage_us[8]);
int spiral_gpu_pack_server_answer_batch_instances_seeded(spiral_gpu_pack_server *const *servers, uint32_t n_clients,
                                                         spiral_gpu_pack_server *const *instances, uint32_t n_instances,
                                                         const void *const *query_msgs, size_t bytes_each, uint64_t *responses, void *wire,
                                                         double *total_us);
int spiral_gpu_pack_server_set_db_format(spiral_gpu_pack_server *s, int format);
int spiral_gpu_pack_server_db_format(spiral_gpu_pack_server *s);
uint64_t spiral_gpu_pack_server_db_device_bytes(spiral_gpu_pack_server *s);
int spiral_gpu_pack_server_time_sweep_batch(spiral_gpu_pack_server *const *servers, uint32_t n, int iters, float *avg_ms);

/* ------------------------------------------------------------------------------------------------
 * Key store: the public parameters of a population of clients resident on the device, bound to the lanes of a batch
 * ------------------------------------------------------------------------------------------------
 * A server answers for the client whose public parameters its four key buffers hold, and set_pub_params* -- an upload, the ingest, a
 * synchronisation -- is the only other way to change them.  A key store does the ingest ONCE per client: a pool of `capacity` slots on one device, each
 * holding one client's public parameters already in the device layout, for one parameter set (out_n = 0: the base path's W_exp_left, W_exp_right, W,
 * V; out_n > 0: SpiralPack's W_exp_left, W_exp_right, V, v_W for that out_n).  bind_keys then makes "lane b serves the client of slot slots[b]" ONE
 * launch for all lanes of a batch.  Two slot forms, chosen at creation:
 *   SPIRAL_GPU_KEYS_FULL     every polynomial, the parts back to back: slot_bytes = polynomials of the message x 16 KiB.  Filled from any form.
 *   SPIRAL_GPU_KEYS_COMPACT  the 32-byte seed of a seeded message, padded to 256 bytes, then rows 1.. of every matrix (what the seeded form sends,
 *                            transformed), densely: slot_bytes = 256 + (polynomials - row-0 polynomials) x 16 KiB, about half of FULL for the
 *                            published sets.  Filled from the seeded form only; put and put_wire fail.  Row 0 is regenerated by every bind.
 * slot_bytes is a pure function of the parameters (no device needed); 0, with last_error set, for parameters get_shape / pack_get_shape refuse or
 * an unknown form.
 *
 * put / put_wire / put_seeded: one client's public parameters into a slot, the arguments of set_pub_params / _wire / _seeded (SpiralPack: of the
 * pack server's).  They run on the store's own stream and workspace and return synchronised; they first wait for every bind launched from the
 * store that is still in flight, on whichever streams, so a put never overwrites words a bind still reads.  A put refused for its arguments alone
 * (slot out of range, a form the store does not take, a null buffer) leaves the slot as it was; one that fails later leaves it EMPTY, never
 * half-valid.  Every successful put gives the slot a new generation.  drop empties a slot; has returns 1 for a filled slot, else 0.  The caller
 * owns the slot numbers: there is no eviction.
 *
 * bind_keys: servers[0 .. n) are the lanes of a batch -- n in 1 .. 8 distinct servers, an owner and its lanes as run_query_batch / answer_batch take
 * them (default schedule, no shard), with the store's parameters, out_n and device; slots[b] in range and filled (two lanes may name one slot).
 * Everything is checked before anything is launched, and a failing call changes nothing.  The launch goes on servers[0]'s stream, behind what the
 * other lanes' streams hold and in front of what they are given next; nothing is synchronised, and it must not be called during stream capture.
 * Afterwards each lane's key buffers hold, word for word, what its own set_pub_params* of the slot's message would have left, and the lane counts as
 * having public parameters.  Buffer addresses do not move: a captured graph replays with the new keys.  A bind is a COPY: a later put to the slot
 * does not reach a lane bound before it.  Each server remembers (store, slot, generation) of its last bind -- set_pub_params* forgets it -- and a
 * lane that already holds the slot's present content is left out of the launch; option "key_binds" (get only) counts the lanes actually copied. */
typedef struct spiral_gpu_key_store spiral_gpu_key_store;
#define SPIRAL_GPU_KEYS_FULL 0
#define SPIRAL_GPU_KEYS_COMPACT 1
int spiral_gpu_key_store_create(const spiral_gpu_params *p, uint32_t out_n, int device, uint32_t capacity, int form, spiral_gpu_key_store **out);
void spiral_gpu_key_store_destroy(spiral_gpu_key_store *store);
size_t spiral_gpu_key_store_slot_bytes(const spiral_gpu_params *p, uint32_t out_n, int form);
int spiral_gpu_key_store_put(spiral_gpu_key_store *store, uint32_t slot, const uint64_t *w_left, const uint64_t *w_right, const uint64_t *w_or_v,
                             const uint64_t *v_or_vw);
int spiral_gpu_key_store_put_wire(spiral_gpu_key_store *store, uint32_t slot, const void *wire, size_t bytes);
int spiral_gpu_key_store_put_seeded(spiral_gpu_key_store *store, uint32_t slot, const void *msg, size_t bytes);
int spiral_gpu_key_store_drop(spiral_gpu_key_store *store, uint32_t slot);
int spiral_gpu_key_store_has(spiral_gpu_key_store *store, uint32_t slot);
int spiral_gpu_server_bind_keys(spiral_gpu_server *const *servers, uint32_t n, spiral_gpu_key_store *store, const uint32_t *slots);
int spiral_gpu_pack_server_bind_keys(spiral_gpu_pack_server *const *servers, uint32_t n, spiral_gpu_key_store *store, const uint32_t *slots);

/* ------------------------------------------------------------------------------------------------
 * A batch's queries in one call, its responses in one read (base server)
 * ------------------------------------------------------------------------------------------------
 * set_query_wire / set_query_seeded take one lane's query and return synchronised; read_response_wire packs, copies and synchronises per lane.  These
 * two calls do both for all lanes of a batch at once.  servers[0 .. n) are n in 1 .. 8 distinct servers, an owner and its lanes as run_query_batch
 * takes them (the same image, parameters, device, shard and buffer layout; lanes of a sharded batch and lanes with any schedule are taken too: neither
 * call depends on a query, on public parameters or on a schedule).  Neither may be called during stream capture.
 *
 * set_query_batch: msgs[b] is server b's query in `form` -- SPIRAL_GPU_FORM_WIRE: what set_query_wire takes; SPIRAL_GPU_FORM_SEEDED: what
 * set_query_seeded takes, the 32-byte seed first -- in pageable host memory, bytes_each = spiral_gpu_query_wire_bytes / _seeded_bytes each; the
 * buffers may be reused when the call returns.  The NTT form (0) is refused: it is no byte stream.  The lanes are not reordered: message b lands in
 * server b.  Everything is checked before anything is written; a call refused for its arguments leaves every lane as it was.  Afterwards every
 * lane's query buffer holds, word for word, what its own set_query_wire / set_query_seeded of its message would have left.  Buffer addresses do
 * not move: a captured graph replays with the new queries.
 *   Messages of at most 4 polynomials per lane (every compressed query): the host checks each coefficient while it copies the messages into a
 *   pinned slot (a ring of two, owned by servers[0]); a coefficient above Q fails the call, naming the server and the coefficient, before anything
 *   goes up, and every lane keeps its previous query.  Otherwise: one copy, one launch on servers[0]'s stream behind what the other lanes' streams
 *   hold, and the call returns WITHOUT synchronising.
 *   Larger messages (direct upload): "query_batch_chunk" message polynomials per lane per pass go through a device staging, one launch per pass for
 *   all lanes, one synchronisation at the end.  A coefficient above Q is found on the device: the call fails, naming the server and the coefficient,
 *   and EVERY lane of the call is left without a query (n messages x polynomials x 2048 coefficients must stay below 2^32).
 *
 * read_response_wire_batch: the wire forms of the n lanes' last responses in one launch, one copy and one synchronisation; lane b's
 * spiral_gpu_response_wire_bytes(p, 2) bytes at out + b * that size, equal to what its own read_response_wire returns.  A capacity below n x that
 * size is refused before anything is launched. */
enum spiral_gpu_message_form { SPIRAL_GPU_FORM_WIRE = 1, SPIRAL_GPU_FORM_SEEDED = 2 };
int spiral_gpu_server_set_query_batch(spiral_gpu_server *const *servers, uint32_t n, int form, const void *const *msgs, size_t bytes_each);
int spiral_gpu_server_read_response_wire_batch(spiral_gpu_server *const *servers, uint32_t n, void *out, size_t capacity);

/* ------------------------------------------------------------------------------------------------
 * Client session: one client's secret key on the device; its public parameters, queries and decoded responses in batches
 * ------------------------------------------------------------------------------------------------
 * A session holds one client's secret key -- sr and the rows of Sp, 2 for base Spiral (out_n = 0) and out_n for SpiralPack, as key_store_create
 * selects the path -- on `device`.  It generates that client's public parameters and batches of its queries there, in the forms the server ingests
 * (reference NTT layout, 7-byte wire form, seeded form; compressed and direct-upload queries, SpiralPack and SpiralStreamPack), and decodes batches
 * of responses: check_final's client half (src/spiral.cpp:1451-1491, src/testing.cpp:1086-1122) for n responses in ONE launch, one workgroup per
 * output polynomial, the products Sp_r * row 0 as exact 64-bit negacyclic convolutions instead of the host client's schoolbook product mod q' on
 * one thread.  The values are those of the command line's host client (cli/client.cpp) with the randomness below.
 *
 * Randomness (the one definition: spiral_amd/csrc/client_device.h).  The session is created from a 32-byte client seed K, and everything it draws is
 * a function of K and counters through the ChaCha20 block function (RFC 8439 section 2.3).  Noise table: with C_i = sum_{j=-64}^{-64+i}
 * exp(-pi j^2 / 6.4^2), the 64-bit thresholds T[i] = floor(2^64 C_i / C_128), i < 128 (a quotient that rounds to 1 gives 2^64 - 1), which
 * client_noise_table returns (plain host code, no device); a 64-bit draw u gives the sample v = -64 + #{ i : T[i] <= u } in [-64, 64], raw value
 * v mod Q.  Noise polynomial i under a noise key N and a domain tag d: coefficient z takes u = w[2 (z & 7)] + w[2 (z & 7) + 1] 2^32 of the block
 * with key N, nonce LE32(d) || LE64(i) and block counter z >> 3.  The secret key is drawn under K itself with domain tag 16: polynomial 0 is sr,
 * polynomials 1.. are the rows of Sp.  nonoise = 1: every sample is 0, the secret included (the command line's --nonoise).
 * Message n -- the public parameters are message 0, queries are messages 1, 2, ... from a counter held in the session -- has the PUBLIC row-0 seed =
 * the first 32 bytes of the block with key K, nonce LE32(17) || LE64(n), counter 0: it goes into the seeded message and expands through the seeded
 * form's domains 1 to 4; and the SECRET noise key N_n = the first 32 bytes of the block with nonce LE32(18) || LE64(n), a derivation of its own under
 * K, so the noise is never derivable from the public seed.  The message's noise polynomials are drawn under N_n with domain tag 19 and numbered in
 * the order of the polynomials the seeded form transmits: matrix by matrix, rows 1.., column by column.
 * K IS THE CLIENT'S SECRET: whoever holds it holds the key.  Two sessions from one K hold the same key and emit the same messages.
 * A MESSAGE NUMBER MUST NEVER BE USED FOR TWO DIFFERENT QUERIES: two queries under one number share their row 0 and their noise, and their
 * difference is the difference of their plaintexts.  A session restored from K (and set_secret) must set_counter past every number it has used, as a
 * seeded message's seed must be fresh for every query.  set_counter(0) is refused: message 0 is the public parameters.
 *
 * One content, three forms.  The three forms of one message hold the same matrices: row 0 of every matrix is the expansion of the message seed
 * (spiral_gpu_seed_expand) in every form, rows 1.. in the NTT form are the transforms of the 7-byte values, so a server that ingests any of the three
 * ends up in the same state.  Public parameters are always message 0, whichever form and however often they are asked for; a query's form is one
 * argument of the one call, which consumes one message number per query.
 *
 * pub_params: the reference NTT layout in set_pub_params' argument order and shapes -- base: W_exp_left, W_exp_right, W, V; SpiralPack: W_exp_left,
 * W_exp_right, V, v_W -- a NULL pointer skips that matrix.  pub_params_msg: form SPIRAL_GPU_FORM_WIRE or _SEEDED, the sizes of
 * spiral_gpu_(pack_)pub_params_wire_bytes / _seeded_bytes; a smaller capacity is refused.
 * queries: n queries for the items idx[0 .. n), message numbers counter .. counter + n - 1, query b at out + b * bytes_each; form
 * SPIRAL_GPU_FORM_NTT (set_query's layout, n_query_cts x 2 x 2 x 2048 words), _WIRE or _SEEDED (spiral_gpu_(pack_)query_wire_bytes / _seeded_bytes).
 * A wrong bytes_each or an index >= 2^(nu1 + nu2) is refused before anything is written, and the counter does not move.  All n queries share one
 * launch sequence: the noise of all of them, its transforms, one table-driven sample launch, the lift and the 7-byte encoding on the device, so only
 * message bytes cross to the host.
 *
 * create: fails, with *out = NULL, for parameters get_shape / pack_get_shape refuse, for q' >= 2^31 (the decode keeps row 0 in 32-bit words) and
 * without a device.  get_secret / set_secret: sr [2048] and Sp [rows][2048] as raw values mod Q; get_secret skips a NULL pointer; set_secret
 * refuses, before anything is written, a coefficient outside [-64, 64] mod Q -- the exactness of the decode rests on |Sp| <= 64: every sum stays
 * below 2048 * 64 * 2^31 < 2^48.
 *
 * decode: `responses` holds n in 1 .. 65535 responses, in pageable host memory, in one of two forms --
 *   SPIRAL_GPU_RESPONSE_RAW   the switched response [(rows + 1)][cols][2048] words each, as spiral_gpu_server_read(SPIRAL_GPU_BUF_RESPONSE) and
 *                             the answer calls return it (row 0 mod q', the other rows mod 4 p_db);
 *   SPIRAL_GPU_RESPONSE_WIRE  the bit-packed response of read_response_wire(_batch), spiral_gpu_response_wire_bytes(p, cols) bytes apart (unpacked
 *                             by the same launch);
 * plaintexts: [n][2 x 2 or out_n x out_n][2048] coefficients in [0, p_db), bit for bit what the reference's check_final recovers.  One copy up, one
 * launch, one copy down on the session's own stream; returns synchronised.  Every argument is checked before anything is copied.
 *
 * response_noise: the error e a response carries, per coefficient, and a record of it per output polynomial -- the ONE definition every layer and
 * test uses.  A response has rows + 1 rows and cols columns (3 x 2 for base Spiral, (out_n + 1) x out_n for SpiralPack); an output polynomial is
 * (response b, r < rows, col), k its coefficient, p = p_db.  `expected` is NULL or [n][rows][cols][2048] plaintext values m in [0, p).
 *   Switched forms, SPIRAL_GPU_RESPONSE_RAW and _WIRE (decode's inputs).  With decode's quantities -- vf = (Sp_r * row 0 [col])[k] mod q' centred
 *   (>= q'/2 -> - q'), vr = row (1 + r)[col][k] mod 4p centred (>= 2p -> - 4p), x = vf 4p + vr q', D = 4 q', res0 = the quotient x / D rounded half
 *   away from zero, before its reduction mod p (decode returns res0 mod p):
 *     without expected  e = x - D res0: the rounding residue, |e| <= D / 2, its sign at a tie what the rounding leaves (e = -D/2 for x > 0);
 *     with expected     e = the residue of x - D m modulo p D centred into [-p D / 2, p D / 2): y in [0, p D) maps to y - p D when y >= p D / 2.
 *   The step is D, the decoding radius D / 2.
 *   Unswitched form, SPIRAL_GPU_RESPONSE_FINAL.  The input is the ciphertext before the modulus switch, [(rows + 1)][cols][2048] raw values mod Q
 *   (a word is taken mod Q): what read(SPIRAL_GPU_BUF_FINAL) holds and the answer calls return as their folded ciphertexts; for SpiralPack the
 *   inverse transform of the packed ciphertext.  v = row (1 + r)[col][k] + (Sp_r * row 0 [col])[k] mod Q (* the negacyclic product), scale_k =
 *   floor(Q / p) (the reference's values.h:93):
 *     with expected     e = v - scale_k m mod Q, centred (>= floor(Q / 2) -> - Q);
 *     without expected  m0 = floor((v + floor(scale_k / 2)) / scale_k) mod p, and e is the same expression with m0 in place of m.
 *   The step is scale_k.  This is the reference's get_diffs(from_ntt(Z), from_ntt(scaled_pt), Q_i) (src/spiral.cpp:1517-1534).
 * stats: [n][rows][cols][6] words, per output polynomial over its 2048 coefficients
 *     word 0     max |e|
 *     word 1     n_wrong: 0 without expected; with expected the number of coefficients whose plaintext -- what decode returns in the switched
 *                forms, m0 in the FINAL form -- differs from expected
 *     words 2, 3 the sum of e, low and high word of a 128-bit two's-complement sum
 *     words 4, 5 the sum of e^2, low and high word of an unsigned 128-bit sum
 * errors: [n][rows][cols][2048] values e.  stats or errors may be NULL, not both.  Bounds: |e| <= p D / 2 = 2 p q' < 2^58 in the switched forms
 * (the call refuses a session with p q' >= 2^57; every published set has p q' < 2^47) and |e| <= Q / 2 < 2^55 in the FINAL form, so |e| < 2^63
 * and the sum of e^2 is below 2048 * 2^116 = 2^127: nothing saturates.  All of it is integer arithmetic, hence bit-reproducible and independent
 * of the order of the reduction.  The FINAL form's products are two convolutions of decode's shape, one per 28-bit prime of Q (every sum below
 * 2048 * 64 * 2^28 < 2^46), recombined mod Q.  n in 1 .. 65535; one copy up (two with expected), one launch on the session's stream, one copy down
 * per output; returns synchronised.  Every argument is checked before anything is copied or written: a null session, null responses, both
 * outputs null, an unknown form, n out of range, and an expected value >= p_db, with its position named. */
typedef struct spiral_gpu_client spiral_gpu_client;
enum spiral_gpu_response_form { SPIRAL_GPU_RESPONSE_RAW = 0, SPIRAL_GPU_RESPONSE_WIRE = 1 };
enum { SPIRAL_GPU_RESPONSE_FINAL = 2 }; /* beside spiral_gpu_response_form, for response_noise alone: decode refuses it */
#define SPIRAL_GPU_FORM_NTT 0 /* beside spiral_gpu_message_form: reference NTT-form polynomials */
int spiral_gpu_client_noise_table(uint64_t *out128);
int spiral_gpu_client_create(const spiral_gpu_params *p, uint32_t out_n, int device, const void *seed32, int nonoise, spiral_gpu_client **out);
void spiral_gpu_client_destroy(spiral_gpu_client *c);
int spiral_gpu_client_get_secret(spiral_gpu_client *c, uint64_t *sr, uint64_t *sp);
int spiral_gpu_client_set_secret(spiral_gpu_client *c, const uint64_t *sr, const uint64_t *sp);
int spiral_gpu_client_get_counter(spiral_gpu_client *c, uint64_t *n);
int spiral_gpu_client_set_counter(spiral_gpu_client *c, uint64_t n);
int spiral_gpu_client_pub_params(spiral_gpu_client *c, uint64_t *w_left, uint64_t *w_right, uint64_t *w_or_v, uint64_t *v_or_vw);
int spiral_gpu_client_pub_params_msg(spiral_gpu_client *c, int form, void *msg, size_t capacity);
int spiral_gpu_client_queries(spiral_gpu_client *c, const uint64_t *idx, uint32_t n, int form, void *out, size_t bytes_each);
int spiral_gpu_client_decode(spiral_gpu_client *c, const void *responses, uint32_t n, int form, uint64_t *plaintexts);
int spiral_gpu_client_response_noise(spiral_gpu_client *c, const void *responses, uint32_t n, int form, const uint64_t *expected, uint64_t *stats,
                                     int64_t *errors);
/* Records ("Records" above; a session with out_n = 0 uses the base layout, one with out_n >= 1 the SpiralPack layout).
 * record_queries: spiral_gpu_client_queries for the items the records live in (record r: item r / per_item), one query per record; one query also
 * serves a record of several instances (the same item index in every instance server).
 * decode_records: `responses` holds n x instances responses laid out [record][instance], in RAW or WIRE form as decode takes them (at most 65535 in
 * all); `records` receives n x record_bytes bytes.  The result is bit for bit what decode gives, followed by packing at w bits and cutting out the
 * record's range (chunk f of a record from response f) -- computed by one workgroup per output polynomial a record touches, which writes the record's
 * bytes straight to the output: a record inside one polynomial costs one of the decode's four (SpiralPack: out_n^2) convolutions and returns record_bytes bytes instead of
 * 64 KiB of words.  For a p_db that is no power of two the low w bits of a decoded value are packed.  Returns synchronised; every argument is checked
 * first (null pointers, an unknown form, a record size the layout refuses, an id at or above the capacity). */
int spiral_gpu_client_record_queries(spiral_gpu_client *c, uint64_t record_bytes, const uint64_t *record_ids, uint32_t n, int form, void *out,
                                     size_t bytes_each);
int spiral_gpu_client_decode_records(spiral_gpu_client *c, const void *responses, uint32_t n, int form, uint64_t record_bytes,
                                     const uint64_t *record_ids, void *records);
/* Keyed records ("Keyed records" above; a base session, or one created with out_n >= 1, whose responses are SpiralPack responses: the header is in
 * output polynomial (0, 0), polynomial t of a value at (t / out_n, t % out_n), up to out_n^2 of them, taken in ascending order).
 * kv_queries: spiral_gpu_client_queries for the items b1, b2 of each key: 2 n queries laid out [key][candidate], under 2 n message numbers.  BOTH
 * are always made, whichever bucket holds the key and whether or not it is present: what a server sees does not depend on the table's content.
 * kv_decode: `responses` holds the 2 n responses laid out [key][candidate], in RAW or WIRE form as decode takes them (2 n <= 65535).  One launch,
 * one workgroup per response: it decodes output polynomial 0 as decode does, packs the header at w bits, looks for the key's tag (computed on the
 * host) and, on a hit, decodes only the output polynomials the slot's value bytes touch.  Candidate 1 wins over candidate 2.  found[k] is 0, 1 or
 * 2; values receives n x value_bytes bytes, those of an absent key zero.  n x value_bytes + n bytes come back, not 2 n plaintexts.  The values
 * and found are bit for bit what decode, the header scan and the value cut of the definition give. */
int spiral_gpu_client_kv_queries(spiral_gpu_client *c, const void *table_key16, const void *keys, uint64_t key_bytes, uint32_t n, int form, void *out,
                                 size_t bytes_each);
int spiral_gpu_client_kv_decode(spiral_gpu_client *c, const void *table_key16, const void *keys, uint64_t key_bytes, const void *responses, uint32_t n,
                                int form, uint64_t value_bytes, void *values, uint8_t *found);

#ifdef __cplusplus
}
#endif
#endif
