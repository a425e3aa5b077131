// The lane set of a multi-server call, shared by server_lanes.cpp and pack_server.cpp.  Such a call takes a list of servers -- one owner and its lanes
// (create_lane / share_db) -- and runs ONE launch sequence on servers[0]'s stream that carries all of them in gridDim.z (kernels.h Lanes).  Three
// things hold before its first launch, each established here and nowhere else: the list is well formed and sweeps one image (check_lane_list), every
// lane's arena is laid out as servers[0]'s, so that one word offset per lane is valid for every buffer (lanes_layout), and the lanes' own streams are
// ordered around the sequence (lanes_join / lanes_release).  Host only; internal to libspiral_gpu.so.
#pragma once
#include "db_image.h"

namespace spiral {
namespace host {

// What the code here needs of a server: both server structs derive from it.
struct LaneHost {
    int device = 0;
    hipStream_t stream = nullptr;  // the stream the server's work runs on
    DbImage* img = nullptr;        // the image it sweeps: its own, or its owner's
    DevBuf arena;                  // its per-query buffers, one allocation ...
    std::vector<size_t> pieces;    // ... and where each piece of it begins, in carve order (alloc_carved)
    hipEvent_t ev_lane = nullptr;  // orders this server's stream around a call on another server's; nothing else records it, it is never timed
    ExportWork xwork;              // read_db_items' workspace (its own, also as a lane: reading does not write the image)
};

// How an entry point on one server opens: a null handle is refused, the server's device is made current
static inline int enter(const LaneHost* S) {
    if (!S) return fail("null server");
    HIP_OK(hipSetDevice(S->device));
    return 0;
}

// What a call needs of its lanes beyond the list check.  Each server's own check reads the bits it knows (server_lanes.cpp check_lanes, pack_server.cpp
// pk_check_lanes); NO_CAPTURE and SWEEP_ONLY are read here.
enum LaneNeeds : uint32_t {
    NEED_QUERY = 1,     // each has its query set
    NEED_DB = 2,        // each has a database
    NEED_RECORDS = 4,   // each has converted its query (the sweep's records are enqueued)
    SHARDED = 8,        // the same fold ranks and expansion shard (a batch of a sharded answer), else neither and their own accumulators
    NO_CAPTURE = 16,    // no lane's stream is capturing
    SWEEP_ONLY = 32,    // they share the sweep only (first_dim_batch, on each server's own pointers): no layout check, no offsets
    GIVES_KEYS = 64,    // the call sets the public parameters (bind_keys): they need not be set
    MOVES_DATA = 128,   // the call only moves messages in or responses out (set_query_batch, read_response_wire_batch): it depends on no query, no
                        // public parameters and no schedule, so lanes of a sharded batch and lanes with other schedules are taken too
    TRIAL_SHARDS = 256, // SpiralPack: the lanes may hold a trial range only (fold_trials_batch, pack_gathered_batch, bind_keys); every other call refuses them
    COLUMN_SHARDS = 512, // the base server: the lanes may be column shards (fold_root_batch; the calls that only move data or keys always take them)
    COLUMN_ONLY = 1024,  // ... and must be (run_column_batch)
    SHARD_LANES = SHARDED | NO_CAPTURE,
};

// no lane's stream is capturing
template <class Srv>
static int lanes_not_capturing(Srv* const* servers, uint32_t n, const char* what) {
    for (uint32_t b = 0; b < n; b++) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        HIP_OK(hipStreamIsCapturing(servers[b]->stream, &cs));
        if (cs != hipStreamCaptureStatusNone) return fail("%s: server %u's stream is capturing (call it outside stream capture)", what, b);
    }
    return 0;
}

// The lanes as a kernel takes them: lane b's arena offset from servers[0]'s in u64 words -- of either sign, the caller chooses which server comes first.
// Equal parameters and shard give equal layouts, so this cannot fail today; it is checked on every call all the same, against the exact record of the
// carve, because a launch with a wrong offset writes outside its client's memory.
template <class Srv>
static int lanes_layout(Srv* const* servers, uint32_t n, const char* what, Lanes* lanes) {
    const LaneHost* S = servers[0];
    *lanes = Lanes{};
    lanes->n = n;
    for (uint32_t b = 0; b < n; b++) {
        const LaneHost* L = servers[b];
        if (L->arena.words != S->arena.words || L->pieces.empty() || L->pieces[0] != 0 || L->pieces != S->pieces)
            return fail("%s: server %u's buffers are not laid out as server 0's", what, b);
        lanes->off[b] = L->arena.p - S->arena.p;
    }
    return 0;
}

// The one check of a call's server list.  Before anything is dereferenced: 1 .. kMaxLanes servers, none null, none listed twice.  Then the device is
// made current and each lane b passes the server's own rules, own(b) (parameters, shard, what the call needs of the lane's state: these come first, so
// that a server of other parameters is refused as such and not for its image), and sweeps servers[0]'s image on its device.  Then NO_CAPTURE, and
// unless SWEEP_ONLY the layouts, which fill `lanes`.
template <class Srv, class Own>
static int check_lane_list(Srv* const* servers, uint32_t n, const char* what, uint32_t needs, Lanes* lanes, Own own) {
    if (!servers || n == 0) return fail("%s: no servers", what);
    if (n > kMaxLanes) return fail("%s: at most %u clients per batch", what, kMaxLanes);
    for (uint32_t b = 0; b < n; b++) {
        if (!servers[b]) return fail("%s: null server %u", what, b);
        for (uint32_t c = 0; c < b; c++)
            if (servers[c] == servers[b]) return fail("%s: server %u listed twice", what, b);
    }
    const LaneHost* S = servers[0];
    HIP_OK(hipSetDevice(S->device));
    for (uint32_t b = 0; b < n; b++) {
        if (own(b)) return -1;
        if (servers[b]->device != S->device || servers[b]->img != S->img)
            return fail("%s: server %u does not sweep server 0's database image (create_lane / share_db)", what, b);
    }
    if ((needs & NO_CAPTURE) && lanes_not_capturing(servers, n, what)) return -1;
    if (!(needs & SWEEP_ONLY)) return lanes_layout(servers, n, what, lanes);
    *lanes = Lanes{};
    lanes->n = n;
    return 0;
}

// ---- stream ordering around a sequence on stream `st` ----
// what X's stream holds comes before what `st` gets next (X on `st` is ordered by it: the cheapest arrangement, each other stream costs ~20 us per call)
static inline int stream_before(LaneHost* X, hipStream_t st) {
    if (X->stream == st) return 0;
    HIP_OK(hipEventRecord(X->ev_lane, X->stream));
    HIP_OK(hipStreamWaitEvent(st, X->ev_lane, 0));
    return 0;
}
// what follows on X's stream comes after `done`, an event recorded on `st`
static inline int stream_after(LaneHost* X, hipStream_t st, hipEvent_t done) {
    if (X->stream != st) HIP_OK(hipStreamWaitEvent(X->stream, done, 0));
    return 0;
}

// the lanes' uploads (and whatever else their streams still hold) come before the sequence on servers[0]'s stream ...
template <class Srv>
static int lanes_join(Srv* const* servers, uint32_t n) {
    for (uint32_t b = 1; b < n; b++)
        if (stream_before(servers[b], servers[0]->stream)) return -1;
    return 0;
}
// ... and what follows on their streams after it (servers[0]'s ev_lane, which no join records: servers[0] is never joined to itself; not recorded at
// all when every lane is on its stream)
template <class Srv>
static int lanes_release(Srv* const* servers, uint32_t n) {
    LaneHost* S = servers[0];
    bool other = false;
    for (uint32_t b = 1; b < n; b++) other |= servers[b]->stream != S->stream;
    if (other) HIP_OK(hipEventRecord(S->ev_lane, S->stream));
    for (uint32_t b = 1; b < n; b++)
        if (stream_after(servers[b], S->stream, S->ev_lane)) return -1;
    return 0;
}

}  // namespace host
}  // namespace spiral
