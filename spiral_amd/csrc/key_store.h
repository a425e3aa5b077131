// The key store (include/spiral_gpu.h, spiral_gpu_key_store_*): a device pool of slots, each holding one client's public parameters already in the PK
// layout, and bind_keys of the two servers -- the checks against the store, the one launch (keys.hip) and the memo of a lane's last bind; each server supplies
// its lane check and its four key buffers.
// Internal to libspiral_gpu.so.  The parts of a slot are those of the message layout (message.h pub_params_layout / pack_pub_params_layout): nothing
// here states them again.
#pragma once
#include "lanes.h"
#include "message.h"

struct spiral_gpu_key_store {
    spiral_gpu_params p;
    uint32_t out_n = 0;  // 0: the base path's public parameters, else SpiralPack's for out_n
    int device = 0;
    uint32_t capacity = 0;
    spiral::KeyForm form = spiral::KEYS_FULL;
    spiral::host::MessageLayout m;  // the layout of the message a slot holds
    uint64_t id = 0;                // of this store among the stores of the process (a lane's memo names it; never reused)
    size_t slot_words = 0;
    spiral::host::DevBuf pool;      // [capacity][slot_words]
    std::vector<uint64_t> gen;      // per slot: 0 = empty, else the generation of what it holds (every successful put takes a new one)
    uint64_t last_gen = 0;
    // the store's own ingest workspace and stream (message.h ingest)
    hipStream_t stream = nullptr;
    spiral::DeviceTables tb;
    spiral::host::DevBuf stage;
    spiral::host::WireIn wire_in;
    hipEvent_t bound = nullptr;  // recorded after every bind launch: a put waits for it before it writes a slot.  A bind on another stream than the
                                 // last one's waits for it first, so the latest record stands for every bind in flight
    bool bind_pending = false;
    hipStream_t bound_stream = nullptr;  // the stream `bound` was last recorded on
};

namespace spiral {
namespace host {

extern std::atomic<uint64_t> g_key_binds;  // key_store.cpp: lanes copied by bind_keys so far (get_option "key_binds")

// what a server remembers of its last bind; cleared by set_pub_params* (store 0: none)
struct KeyMemo {
    uint64_t store = 0, gen = 0;
    uint32_t slot = 0;
};

// the lanes of one bind call that are copied (those whose memo does not name the slot's present content), with their arena offsets and slots
struct KeyBindPlan {
    Lanes lanes;                // their offsets from the call's servers[0] (n = 0: nothing to launch)
    uint32_t slot[kMaxLanes];
    uint32_t lane[kMaxLanes];   // their indices in the call's server list
};

// The store's share of a bind's checks, before anything is launched: the store holds keys of these parameters, out_n and device; every part fits
// lane 0's buffer of it (dst_words[i] words); every slot is in range and filled.  `all`: the arena offsets of the call's n lanes; memo[b]: lane b's
// memo, or null when the lane has no keys (have_pp unset).
int key_bind_plan(const spiral_gpu_key_store* K, const spiral_gpu_params& p, uint32_t out_n, int device, const Lanes& all, const uint32_t* slots,
                  const KeyMemo* const* memo, const size_t dst_words[kMessageParts], const char* what, KeyBindPlan* plan);
// the one launch, on `st`: part i of each planned lane's slot into dst[i] + the lane's offset (dst: lane 0's buffers); records the store's `bound`
// event behind it.  Synchronises nothing
int key_bind_launch(spiral_gpu_key_store* K, const KeyBindPlan& plan, uint64_t* const dst[kMessageParts], hipStream_t st);
// the memo lane plan.lane[k] keeps of it
KeyMemo key_bind_memo(const spiral_gpu_key_store* K, const KeyBindPlan& plan, uint32_t k);

// bind_keys of either server, behind its lane check (which gave `lanes`): the keys of slot slots[b] into lane b's four key buffers -- dst[i] and
// dst_words[i]: servers[0]'s buffer of part i and its words -- all lanes in one launch on servers[0]'s stream.  Every check comes before the launch, so a
// failing call changes nothing; a lane whose memo names the slot's present content is left out of the launch.  Nothing is synchronised.  A server
// here has `p`, `have_pp` and `key_memo` beside what lanes.h asks of it.
template <class Srv>
static int bind_keys(Srv* const* servers, const Lanes& lanes, spiral_gpu_key_store* store, const uint32_t* slots, uint32_t out_n, uint64_t* const dst[kMessageParts],
              const size_t dst_words[kMessageParts], const char* what) {
    Srv* S = servers[0];
    const KeyMemo* memo[kMaxLanes];
    for (uint32_t b = 0; b < lanes.n; b++) memo[b] = servers[b]->have_pp ? &servers[b]->key_memo : nullptr;
    KeyBindPlan plan;
    if (key_bind_plan(store, S->p, out_n, S->device, lanes, slots, memo, dst_words, what, &plan)) return -1;
    if (plan.lanes.n == 0) return 0;
    if (lanes_join(servers, lanes.n) || key_bind_launch(store, plan, dst, S->stream) || lanes_release(servers, lanes.n)) return -1;
    for (uint32_t k = 0; k < plan.lanes.n; k++) {
        servers[plan.lane[k]]->key_memo = key_bind_memo(store, plan, k);
        servers[plan.lane[k]]->have_pp = true;
    }
    return 0;
}

}  // namespace host
}  // namespace spiral
