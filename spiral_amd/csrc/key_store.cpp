// The key store of include/spiral_gpu.h: client keys resident on the device in the PK layout, ingested once per client through the one ingest of
// message.h, and the store's share of bind_keys (key_store.h; the servers' shares are in server_lanes.cpp and pack_server.cpp, the kernel in keys.hip).
#include "key_store.h"

using namespace spiral;
using namespace spiral::host;

std::atomic<uint64_t> spiral::host::g_key_binds{0};
static std::atomic<uint64_t> g_store_ids{0};

namespace {

// the layout of the message a slot holds, for parameters the path accepts (out_n = 0: the base path)
int key_layout(const spiral_gpu_params* p, uint32_t out_n, int form, MessageLayout* m) {
    if (!p) return fail("null parameters");
    if (form != KEYS_FULL && form != KEYS_COMPACT) return fail("key store: unknown slot form %d", form);
    if (out_n == 0) {
        spiral_gpu_shape s;
        if (shape_of(p, &s)) return -1;
        *m = pub_params_layout(*p, s);
    } else {
        spiral_gpu_pack_shape s;
        if (spiral_gpu_pack_get_shape(p, out_n, &s)) return -1;
        *m = pack_pub_params_layout(*p, s, out_n);
    }
    for (const MessagePart& t : m->part)
        if (form == KEYS_COMPACT && t.count && t.rows < 2) return fail("key store: a matrix of one row has no compact form");
    if (message_polys(*m, FORM_NTT) >= (1u << 20)) return fail("key store: public parameters of %zu polynomials exceed a slot", message_polys(*m, FORM_NTT));
    return 0;
}
// FULL: every polynomial.  COMPACT: the seed, padded to one 256-byte piece (kKeyCompactHead words), then the polynomials the seeded form sends
size_t key_slot_words(const MessageLayout& m, int form) {
    return form == KEYS_COMPACT ? kKeyCompactHead + message_polys(m, FORM_SEEDED) * kN : message_polys(m, FORM_NTT) * kN;
}

int key_slot(spiral_gpu_key_store* K, uint32_t slot, const char* what) {
    if (!K) return fail("%s: null key store", what);
    if (slot >= K->capacity) return fail("%s: slot %u outside the store of %u slots", what, slot, K->capacity);
    HIP_OK(hipSetDevice(K->device));
    return 0;
}

// One client's public parameters, in any form, into a slot.  The slot is empty from the first write until the ingest has succeeded.
int key_put(spiral_gpu_key_store* K, uint32_t slot, Form form, const MessageIn& in, const char* what) {
    if (key_slot(K, slot, what)) return -1;
    if (K->form == KEYS_COMPACT && form != FORM_SEEDED)
        return fail("%s: a compact store keeps a message's seed and its rows 1..: it is filled from the seeded form only (put_seeded)", what);
    if (form == FORM_NTT && check_ntt_parts(K->m, in, what)) return -1;
    if (K->bind_pending) {  // a bind in flight may still read the slot
        HIP_OK(hipEventSynchronize(K->bound));
        K->bind_pending = false;
    }
    K->gen[slot] = 0;
    uint64_t* base = K->pool.p + (size_t)slot * K->slot_words;
    uint64_t* dst[kMessageParts];
    const IngestOn on{K->stage, K->wire_in, K->tb, K->stream};
    if (K->form == KEYS_FULL) {
        size_t at = 0;
        for (uint32_t i = 0; i < kMessageParts; i++) {
            dst[i] = base + at;
            at += K->m.part[i].polys() * kN;
        }
        if (ingest(form, on, K->m, dst, in, what)) return -1;
    } else {
        // what the seeded message sends is the wire form of the same matrices without their row 0: ingested as that, densely
        const size_t want = message_bytes(K->m, FORM_SEEDED);
        if (!in.msg) return fail("%s: null message", what);
        if (in.bytes != want) return fail("%s: %zu bytes, the seeded form of these public parameters takes %zu", what, in.bytes, want);
        MessageLayout dense = K->m;
        size_t at = kKeyCompactHead;
        for (uint32_t i = 0; i < kMessageParts; i++) {
            dense.part[i].rows -= dense.part[i].count ? 1 : 0;
            dst[i] = base + at;
            at += dense.part[i].polys() * kN;
        }
        HIP_OK(hipMemcpyAsync(base, in.msg, kSeedBytes, hipMemcpyHostToDevice, K->stream));
        if (ingest(FORM_WIRE, on, dense, dst, MessageIn{{}, (const uint8_t*)in.msg + kSeedBytes, in.bytes - kSeedBytes}, what)) return -1;
    }
    HIP_OK(hipStreamSynchronize(K->stream));
    K->gen[slot] = ++K->last_gen;
    return 0;
}

void key_store_free(spiral_gpu_key_store* K) {
    if (K->bind_pending && K->bound) (void)hipEventSynchronize(K->bound);
    K->pool.release();
    K->stage.release();
    K->wire_in.release();
    if (K->bound) (void)hipEventDestroy(K->bound);
    if (K->stream) (void)hipStreamDestroy(K->stream);
    delete K;
}

}  // namespace

int spiral::host::key_bind_plan(const spiral_gpu_key_store* K, const spiral_gpu_params& p, uint32_t out_n, int device, const Lanes& all, const uint32_t* slots,
                                const KeyMemo* const* memo, const size_t dst_words[kMessageParts], const char* what, KeyBindPlan* plan) {
    if (!K || !slots) return fail("%s: null %s", what, K ? "slot list" : "key store");
    if (memcmp(&K->p, &p, sizeof(p)) != 0 || K->out_n != out_n)
        return fail("%s: the store holds keys of other parameters than the servers' (out_n %u, the servers' %u)", what, K->out_n, out_n);
    if (K->device != device) return fail("%s: the store is on device %d, the servers on device %d", what, K->device, device);
    for (uint32_t i = 0; i < kMessageParts; i++)
        if (K->m.part[i].polys() * kN > dst_words[i])
            return fail("%s: part %u of the keys (%zu polynomials) does not fit the server's buffer", what, i, K->m.part[i].polys());
    for (uint32_t b = 0; b < all.n; b++) {
        if (slots[b] >= K->capacity) return fail("%s: slot %u (lane %u) outside the store of %u slots", what, slots[b], b, K->capacity);
        if (!K->gen[slots[b]]) return fail("%s: slot %u (lane %u) is empty", what, slots[b], b);
    }
    *plan = KeyBindPlan{};
    uint32_t k = 0;
    for (uint32_t b = 0; b < all.n; b++) {
        const KeyMemo* mm = memo[b];
        if (mm && mm->store == K->id && mm->slot == slots[b] && mm->gen == K->gen[slots[b]]) continue;  // the lane holds these keys already
        plan->lanes.off[k] = all.off[b];
        plan->slot[k] = slots[b];
        plan->lane[k] = b;
        k++;
    }
    plan->lanes.n = k;
    return 0;
}

int spiral::host::key_bind_launch(spiral_gpu_key_store* K, const KeyBindPlan& plan, uint64_t* const dst[kMessageParts], hipStream_t st) {
    KeyBindParams kp{};
    kp.store = K->pool.p;
    kp.slot_words = K->slot_words;
    kp.head = K->form == KEYS_COMPACT ? kKeyCompactHead : 0;
    kp.domain = K->m.domain;
    // a kernel's lane 0 is the one its pointers name (Lanes::here): the first planned lane, the others relative to it
    const int64_t off0 = plan.lanes.off[0];
    uint32_t src = 0, row0 = 0;
    for (uint32_t i = 0; i < kMessageParts; i++) {
        const MessagePart& t = K->m.part[i];
        kp.part[i] = KeyPart{dst[i] + off0, (uint32_t)t.polys(), t.rows, t.cols, src, row0};
        src += (uint32_t)(t.polys() - (K->form == KEYS_COMPACT ? t.row0() : 0));
        row0 += (uint32_t)t.row0();
    }
    for (uint32_t k = 0; k < plan.lanes.n; k++) kp.slot[k] = plan.slot[k];
    kp.lanes = plan.lanes;
    for (uint32_t k = 0; k < plan.lanes.n; k++) kp.lanes.off[k] -= off0;
    // `bound` is one event, re-recorded by every bind: a bind on another stream than the last goes behind that one, so the newest record covers
    // every bind still in flight -- what a put and the store's release wait for
    if (K->bind_pending && K->bound_stream != st) HIP_OK(hipStreamWaitEvent(st, K->bound, 0));
    launch_key_bind(kp, K->form, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(K->bound, st));
    K->bind_pending = true;
    K->bound_stream = st;
    g_key_binds += plan.lanes.n;
    return 0;
}

KeyMemo spiral::host::key_bind_memo(const spiral_gpu_key_store* K, const KeyBindPlan& plan, uint32_t k) {
    return KeyMemo{K->id, K->gen[plan.slot[k]], plan.slot[k]};
}

extern "C" {

size_t spiral_gpu_key_store_slot_bytes(const spiral_gpu_params* p, uint32_t out_n, int form) {
    MessageLayout m;
    return key_layout(p, out_n, form, &m) ? 0 : key_slot_words(m, form) * sizeof(uint64_t);
}

int spiral_gpu_key_store_create(const spiral_gpu_params* p, uint32_t out_n, int device, uint32_t capacity, int form, spiral_gpu_key_store** out) {
    if (!p || !out) return fail("null argument");
    MessageLayout m;
    if (key_layout(p, out_n, form, &m)) return -1;
    if (capacity == 0) return fail("key store: a capacity of 0 slots");
    HIP_OK(hipSetDevice(device));
    spiral_gpu_key_store* K = new spiral_gpu_key_store();
    K->p = *p;
    K->out_n = out_n;
    K->device = device;
    K->capacity = capacity;
    K->form = (KeyForm)form;
    K->m = m;
    K->id = ++g_store_ids;
    K->slot_words = key_slot_words(m, form);
    K->gen.assign(capacity, 0);
    if (tables_get(device, &K->tb) != 0) {
        key_store_free(K);
        return fail("twiddle table setup failed on device %d", device);
    }
    if (hipStreamCreate(&K->stream) != hipSuccess || hipEventCreateWithFlags(&K->bound, hipEventDisableTiming) != hipSuccess) {
        key_store_free(K);
        return fail("key store: stream setup failed");
    }
    if (K->pool.alloc((size_t)capacity * K->slot_words)) {
        (void)hipGetLastError();
        key_store_free(K);
        return fail("key store: no device memory for %u slots of %zu bytes", capacity, K->slot_words * sizeof(uint64_t));
    }
    *out = K;
    return 0;
}

void spiral_gpu_key_store_destroy(spiral_gpu_key_store* K) {
    if (!K) return;
    (void)hipSetDevice(K->device);
    key_store_free(K);
}

int spiral_gpu_key_store_put(spiral_gpu_key_store* K, uint32_t slot, const uint64_t* w_left, const uint64_t* w_right, const uint64_t* w_or_v,
                             const uint64_t* v_or_vw) {
    return key_put(K, slot, FORM_NTT, MessageIn{{w_left, w_right, w_or_v, v_or_vw}, nullptr, 0}, "key_store_put");
}
int spiral_gpu_key_store_put_wire(spiral_gpu_key_store* K, uint32_t slot, const void* wire, size_t bytes) {
    return key_put(K, slot, FORM_WIRE, MessageIn{{}, wire, bytes}, "key_store_put_wire");
}
int spiral_gpu_key_store_put_seeded(spiral_gpu_key_store* K, uint32_t slot, const void* msg, size_t bytes) {
    return key_put(K, slot, FORM_SEEDED, MessageIn{{}, msg, bytes}, "key_store_put_seeded");
}
int spiral_gpu_key_store_drop(spiral_gpu_key_store* K, uint32_t slot) {
    if (key_slot(K, slot, "key_store_drop")) return -1;
    K->gen[slot] = 0;  // (the words stay: a bind in flight reads them, and a lane bound from them keeps its copy)
    return 0;
}
int spiral_gpu_key_store_has(spiral_gpu_key_store* K, uint32_t slot) { return K && slot < K->capacity && K->gen[slot] != 0; }

}  // extern "C"
