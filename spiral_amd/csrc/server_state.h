// The resident server's state and what its translation units share: server.cpp (the server object, its database calls, message intake, the
// one-query stages and launch groups, the hipGraph cache) and server_lanes.cpp (the calls that carry several servers); primitives.cpp takes the
// batched sweep from here.  Every function declared here is defined in server.cpp; the templates are whole.  Host only; internal to libspiral_gpu.so.
#pragma once
#include "db_image.h"
#include "key_store.h"
#include "message.h"

using namespace spiral;  // (an internal header of three .cpp files: the struct below has to be the global one the C ABI names)
using namespace spiral::host;

// The launch sequences a server captures into hipGraphs, one graph each, named after the entry point that runs it (the number is the
// SPIRAL_GRAPH_DOT file's).  A batch or shard sequence is kept by the call's servers[0].
enum GraphId : int {
    G_PRE = 0,  // (split schedule: the even tree + ScalToMat on the main stream)
    G_POST = 1,
    G_POST_REDUCE = 2,
    G_PRE_SIDE = 3,  // run_pre, split schedule: the odd tree + Regev->GSW on the side stream
    G_QUERY = 4,
    G_FOLD_LOCAL = 5,
    G_FOLD_ROOT = 6,
    G_PRE_SWEEP = 7,
    G_EXPAND_PACK = 8,
    G_UNPACK_CONVERT_SWEEP = 9,
    G_SCAL2MAT_SWEEP = 10,
    G_UNPACK_GSW = 11,
    G_SCAL2MAT = 12,
    G_BATCH,
    G_INSTANCES,
    G_BATCH_INSTANCES,
    G_SHARD_PRE_SWEEP,  // run_pre_sweep_batch ... fold_root_batch
    G_SHARD_EXPAND_PACK,
    G_SHARD_UNPACK_SWEEP,
    G_SHARD_FOLD_LOCAL,
    G_SHARD_FOLD_ROOT,
    G_COLUMN_BATCH,  // run_column_batch
    G_COUNT
};
// a captured sequence and the words it was captured for beyond the server's own state (the caller's buffers, the lanes, the images; run_graph)
struct Captured {
    hipGraphExec_t exec = nullptr;
    std::vector<uint64_t> key;
};

// A column shard (create_column_shard): of the num_per ciphertext columns of the database this server holds ii = rank + G k, k < L = num_per >> g_log,
// for EVERY first-dimension index -- the base image DbLayout::base(L, dim0) of the items i = rank (mod G), local item i / G.  Its query and fold
// geometry stay the parameters' (s.num_per, nu2); only what touches the image takes L (srv_np).
struct ColumnShard {
    bool on = false;
    uint32_t rank = 0, g_log = 0;
    bool operator==(const ColumnShard& o) const { return on == o.on && rank == o.rank && g_log == o.g_log; }
};

struct spiral_gpu_server : LaneHost {  // (lanes.h: device, stream, img, arena and its layout record, ev_lane)
    spiral_gpu_params p;
    spiral_gpu_shape s;
    uint32_t j0 = 0, j1 = 0, dim0_shard = 0;
    ColumnShard col;  // set at creation, never changed; fold_g_log is then fixed to col.g_log
    hipStream_t own_stream = nullptr;
    DeviceTables tb;
    bool keep_cts = false, have_pp = false, have_query = false;
    bool raw_from_acc = false;  // S->raw holds the lift of what S->acc holds now (lift ran, no sweep / write_raw / fold since): the stage fold may use the pair form
    bool have_records = false;  // the sweep's query records of the current query have been enqueued (ScalToMat ran since set_query)
    DevBuf wire;  // bit-packed response (read_response_wire)
    // img, the database image this server sweeps (db_image.h): its own, or its owner's, of which it holds a reference (create_lane, share_db) and
    // which it never writes
    // expanded-ciphertext positions inside cv: first-dim j at j*pos_stride + pos_first, rest i at i*pos_stride + pos_rest
    uint32_t pos_stride = 1, pos_first = 0, pos_rest = 0, n_cv = 0;

    // every per-query buffer below except the lazily allocated ones (ex_raw2, ex_g2, cts_keep, stage, wire) is a piece of `arena`, carved in one
    // fixed order (srv_alloc): servers with equal parameters and shard have equal layouts, which is what every multi-lane call relies on (lanes.h)
    DevBuf w_left, w_right, w, v, query, cv, ex_raw, ex_g, ex_raw2, ex_g2;  // (the second work set: the odd tree of a split expansion)
    DevBuf cv_raw, cv_g, key, cts_keep;  // key: [d][3][m2]: the GSW matrices Q (src/spiral.cpp:2324) -- the fold key; Q_neg = G2 - Q (:2361-2379) is never stored (poly.hip fold_mac_two_kernel)
    uint64_t *gs_raw_p = nullptr, *gs_chat_p = nullptr;  // the Regev->GSW halves of cv_raw / cv_g
    DevBuf qs, acc_own, raw, fold_d, fold_c, fold_c2, resp, stage;
    WireIn wire_in;  // the staging of the wire and seeded forms (message.h ingest)
    QueryBatchIn query_batch_in;  // ... of set_query_batch, when this server is a batch's servers[0]
    KeyMemo key_memo;  // the store slot the four key buffers were last bound from (bind_keys); none once set_pub_params* has written them
    uint64_t* acc = nullptr;
    hipEvent_t ev[8] = {};
    // captured launch sequences (hipGraph), used while use_graphs is on: captured on first use, re-captured when their key changes, all dropped
    // (srv_drop_graphs) when server state they bake in changes
    bool use_graphs = false;
    Captured graphs[G_COUNT];
    // overlap 2 ("split"): the whole GSW side of the query -- the odd-index tree of the expansion AND the Regev->GSW conversion -- runs as its
    // own launch sequence on side_stream, beside the even tree + ScalToMat + sweep on the main stream; only the folding needs it.
    // (Modes 1 and 3 -- only the conversion forked, under the sweep -- measured slower and were removed in round 5, HISTORY.md.)
    int overlap = 0;
    bool side_pending = false;
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // Fold round forms.  Default: the pair form, unchained (lift launch + LD_SDIFF digit-difference launch + product with addend).
    // fold_pair = false (SPIRAL_FOLD_PAIR=0) or a gadget dimension whose digits do not recompose (!fold_pair_exact): the reference's
    // two-product form, lift chained into the digit transforms (fold_chain_kernel: a block lifts one source polynomial and transforms
    // dpb of its digits; dpb is halved from ell until the round has at least fold_blocks blocks, SPIRAL_FOLD_BLOCKS) or, with
    // SPIRAL_FOLD_CHAIN=0, as separate lift + LD_SDIGIT launches.  (The chained pair forms fold_pair_kernel / fold_team_kernel tied
    // with the unchained one and were removed in round 5; HISTORY.md has the numbers and the commit.)
    bool fold_chain = true;
    bool fold_pair = true;
    uint32_t fold_blocks = 768;
    uint32_t fold_g_log = 0;  // distributed fold over 2^fold_g_log ranks: the sweep groups its output by ii mod G
    uint32_t sweep_k_log = 0; // pipelined sweep in 2^sweep_k_log stages (set_sweep_stages): accumulators laid out [stage][rank][ct]
    ExpandShard ex_shard{};   // sharded expansion (set_expand_shard): what this rank expands itself
    // batched sweeps of sweep_mfma_min or more queries run on the matrix cores (sweep_mfma.hip) from the limb planes of the database (DbImage::limb_view).
    // SPIRAL_SWEEP_MFMA=n sets the threshold (0 = never: at most kSweepMaxBatch queries per pass, on the vector ALU)
    // With the option one_image (default) the one image is converted to limb-plane form IN PLACE the first time a batch wants it (single queries then
    // sweep it with sweep_mfma_kernel<1>, which ties with the vector-ALU kernel) and back when something needs the packed form (a partial reload, a
    // staged sweep); without it the limb planes are a second image, as large as the first, dropped when the database is reloaded.
    uint32_t sweep_mfma_min = 2;
    uint64_t epoch_seen = 0;  // the image's epoch this server's graphs were captured under
};

namespace spiral {
namespace host {

extern std::atomic<uint64_t> g_captures;  // server.cpp: hipGraphs the servers of this process have captured so far (get_option "graph_captures")

// The arguments of the fold (run_fold_rounds), by name: rounds [d0, d0 + rounds) on np0 ciphertexts.  src_pk == nullptr: the ciphertexts are already
// lifted in S->raw.  Otherwise they are the PK polynomials [np0][3][2] at src_pk (accumulators, lazy sums when pre_reduce) and the lift is chained
// into the digit transforms (fold_chain_kernel); later rounds chain from the previous round's product the same way.
// finish: the folded ciphertext is the answer; follow with the response modulus switch (finish_lanes).
// raw_addend: with src_pk == nullptr, the transform-domain words of the ciphertexts lifted in S->raw, when the caller still has them
// (the stage API's fold after lift: the accumulators) -- the first round can then take the pair form too (LD_SDIFF on S->raw).
// lanes: the same rounds for every query lane in the same launches (all pointers are lane 0's, kernels.h Lanes).
struct FoldJob {
    uint32_t np0 = 0, d0 = 0, rounds = 0;
    const uint64_t* src_pk = nullptr;
    bool pre_reduce = false, finish = false;
    const uint64_t* raw_addend = nullptr;
    Lanes lanes{};
};
// the parts of the conversion (convert_part)
enum ConvertWhat : uint32_t { CONV_S2M = 1, CONV_GSW = 2, CONV_BOTH = 3 };

// the column count L of rank `rank` of n_ranks column shards of a database of num_per columns, or 0 and the error.  The bound: a base server answers
// from one ciphertext column (nu2 = 0: one sweep, no fold round; the parity tests' random parameter sets draw it), so L = num_per / n_ranks >= 1
constexpr uint32_t kMinShardColumns = 1;
inline uint32_t column_shard_columns(uint32_t num_per, uint32_t rank, uint32_t n_ranks) {
    if (n_ranks == 0 || (n_ranks & (n_ranks - 1))) return fail("column shards: %u ranks, the rank count must be a power of two", n_ranks), 0u;
    if (num_per / n_ranks < kMinShardColumns)
        return fail("column shards: %u ranks leave %u of %u ciphertext columns per shard, a shard needs at least %u", n_ranks, num_per / n_ranks, num_per,
                    kMinShardColumns),
               0u;
    if (rank >= n_ranks) return fail("column shard %u of %u: no such rank", rank, n_ranks), 0u;
    return num_per / n_ranks;
}
// the ciphertext columns of the image S sweeps: num_per, or a column shard's L
inline uint32_t srv_np(const spiral_gpu_server* S) { return S->s.num_per >> (S->col.on ? S->col.g_log : 0u); }
inline uint32_t col_g_log(const spiral_gpu_server* S) { return S->col.on ? S->col.g_log : 0u; }
inline uint32_t col_ranks(const spiral_gpu_server* S) { return 1u << col_g_log(S); }
inline bool holds_column(const spiral_gpu_server* S, uint32_t ii) { return (ii & (col_ranks(S) - 1u)) == (S->col.on ? S->col.rank : 0u); }
// how a sweep of S's image groups its output: by ii mod G for the distributed fold of a j-shard; a column shard's L columns are one rank's already
inline uint32_t sweep_g_log(const spiral_gpu_server* S) { return S->col.on ? 0u : S->fold_g_log; }
// how a one-server entry point that has no meaning on a column shard opens
inline int refuse_column(const spiral_gpu_server* S, const char* what) {
    if (S && S->col.on)
        return fail("%s: this server is a column shard (create_column_shard): it holds %u of %u ciphertext columns, so it answers through run_column_batch, "
                    "the all-gather and fold_root_batch only", what, srv_np(S), S->s.num_per);
    return 0;
}
void srv_check_epoch(spiral_gpu_server* S);  // (run_graph) drops S's graphs when its image has changed since they were captured
int srv_join_side(spiral_gpu_server* S);
void mark_raw_stale(spiral_gpu_server* const* servers, uint32_t n);
void mark_swept(spiral_gpu_server* const* servers, uint32_t n);
int sweep_mfma(const uint64_t* limbs, const uint32_t* const* qs, uint64_t* const* acc, uint32_t n, uint32_t np, uint32_t jm, uint32_t g_log, hipStream_t st,
               uint32_t k_log = 0, uint32_t g_extra = 0);
int sweep_one(spiral_gpu_server* S, int stage);
int expand_lanes(spiral_gpu_server* S, const Lanes& lanes, uint32_t r_begin = 0, uint32_t r_end = 0xffffffffu);
int convert_part(spiral_gpu_server* S, uint32_t what, hipStream_t st, bool mark_split = false, const Lanes& lanes = Lanes{});
int expand_convert(spiral_gpu_server* S);
int finish_lanes(spiral_gpu_server* S, const Lanes& lanes);
int run_fold_rounds(spiral_gpu_server* S, const FoldJob& job);

// the first-dimension sweep of n queries (records qs[b] -> accumulators acc[b]) against the packed image db of geometry (np, jm): one pass on the matrix
// cores when the limb-plane image `limbs` is given, else passes of up to kSweepMaxBatch queries on the vector ALU (wide packed geometries), else one(b)
// per remaining query.  g_extra: the rank-major batch layout (kernels.h launch_sweep_batch)
template <class One>
int sweep_queries(const uint64_t* db, const uint64_t* limbs, uint32_t np, uint32_t jm, const uint32_t* const* qs, uint64_t* const* acc, uint32_t n, uint32_t g_log,
                  hipStream_t st, uint32_t k_log, uint32_t g_extra, One one) {
    if (limbs) return sweep_mfma(limbs, qs, acc, n, np, jm, g_log, st, k_log, g_extra);
    const uint32_t step = sweep_batch_ok(np, jm) ? kSweepMaxBatch : 1;
    for (uint32_t b0 = 0; b0 < n; b0 += step) {
        const uint32_t nb = n - b0 < step ? n - b0 : step;
        if (nb > 1)
            launch_sweep_batch(db, qs + b0, acc + b0, nb, np, jm, g_log, st, g_extra);
        else if (int rc = one(b0))
            return rc;
    }
    return 0;
}
// the same where a lone query sweeps straight into its accumulators
inline int sweep_queries(const uint64_t* db, const uint64_t* limbs, uint32_t np, uint32_t jm, const uint32_t* const* qs, uint64_t* const* acc, uint32_t n, uint32_t g_log,
                         hipStream_t st, uint32_t k_log = 0) {
    return sweep_queries(db, limbs, np, jm, qs, acc, n, g_log, st, k_log, 0, [&](uint32_t b) {
        launch_sweep(db, qs[b], acc[b], np, jm, g_log, st, k_log);
        return 0;
    });
}

// the key of a captured sequence: the words it bakes in that server state does not cover (a braced list is compared without allocating)
struct GraphKey {
    const uint64_t* p;
    size_t n;
    GraphKey(const uint64_t* p, size_t n) : p(p), n(n) {}
    GraphKey(std::initializer_list<uint64_t> k) : GraphKey(k.begin(), k.size()) {}
    GraphKey(const std::vector<uint64_t>& k) : GraphKey(k.data(), k.size()) {}
};
inline uint64_t word(const void* p) { return (uint64_t)(uintptr_t)p; }

// run `body` (kernel launches on st) directly, or -- with use_graphs on -- replay S's graph `id`, captured from body() first when there is none or it
// was captured for another key.  Host state the sequence changes is the caller's to set: a replay runs no host code.
template <class F>
int run_graph(spiral_gpu_server* S, GraphId id, hipStream_t st, GraphKey key, F body) {
    if (!S->use_graphs) return body();
    srv_check_epoch(S);
    Captured& c = S->graphs[id];
    if (c.exec && !(c.key.size() == key.n && std::equal(key.p, key.p + key.n, c.key.begin()))) {
        (void)hipGraphExecDestroy(c.exec);
        c.exec = nullptr;
    }
    if (!c.exec) {
        if (st == nullptr) return fail("graph capture needs a non-default stream");
        HIP_OK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
        const int rc = body();
        hipGraph_t g = nullptr;
        hipError_t e = hipStreamEndCapture(st, &g);
        if (rc || e != hipSuccess) {
            if (g) (void)hipGraphDestroy(g);
            return rc ? rc : fail("hipStreamEndCapture failed: %s", hipGetErrorString(e));
        }
        if (const char* dot = tuning_env("SPIRAL_GRAPH_DOT")) {  // debugging aid: <prefix>.<id>.dot
            const std::string path = std::string(dot) + "." + std::to_string(id) + ".dot";
            (void)hipGraphDebugDotPrint(g, path.c_str(), 0);
        }
        e = hipGraphInstantiate(&c.exec, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (e != hipSuccess) return fail("hipGraphInstantiate failed: %s", hipGetErrorString(e));
        c.key.assign(key.p, key.p + key.n);
        g_captures++;
    }
    HIP_OK(hipGraphLaunch(c.exec, st));
    return 0;
}

}  // namespace host
}  // namespace spiral
