// What a client sends a server -- a query, or its public parameters -- stated once: the layout of each message (which matrices, in which order, how
// many, of which [rows][cols]) and the one ingest that takes it in any of its three forms.  Internal to libspiral_gpu.so; the sizes the ABI reports
// (spiral_gpu_*_{wire,seeded}_bytes), the destinations of an ingest and the NTT-form upload are all derived from the layout.
#pragma once
#include "host_common.h"

namespace spiral {
namespace host {

// ---- the layouts ----------------------------------------------------------------------------------------------------------------------------------
enum Form { FORM_NTT, FORM_WIRE, FORM_SEEDED };  // include/spiral_gpu.h: reference NTT-form polynomials, 7 bytes per raw coefficient, seed + rows 1..
constexpr uint32_t kMessageParts = 4;
struct MessagePart {  // `count` matrices of [rows][cols] polynomials, back to back (count = 0: a part the message does not have)
    size_t count;
    uint32_t rows, cols;
    size_t polys() const { return count * rows * cols; }
    size_t row0() const { return count * cols; }  // the polynomials the seeded form generates instead of sending
};
struct MessageLayout {
    MessagePart part[kMessageParts];
    uint32_t domain;  // the seeded form's row-0 domain tag (seed_device.h)
};

// The four messages, each from (parameters, shape).  A query: its ciphertexts, [2][1] each
inline MessageLayout query_layout(const spiral_gpu_params&, const spiral_gpu_shape& s) { return {{{s.n_query_cts, 2, 1}}, SEED_QUERY}; }
inline MessageLayout pack_query_layout(const spiral_gpu_params&, const spiral_gpu_pack_shape& s, uint32_t) { return {{{s.n_query_cts, 2, 1}}, SEED_PACK_QUERY}; }
// W_exp_left, W_exp_right (one [2][t] key per expansion round), W, V
inline MessageLayout pub_params_layout(const spiral_gpu_params& p, const spiral_gpu_shape& s) {
    return {{{s.n_left, 2, p.t_exp}, {s.n_right, 2, p.t_exp_right}, {1, 3, 2 * p.t_conv}, {1, 3, 2 * p.t_conv}}, SEED_PUB_PARAMS};
}
// W_exp_left, W_exp_right, V, then v_W (one [out_n + 1][t_conv] key per output column).  A direct-upload geometry expands and converts nothing: it
// sends no W_exp and no V
inline MessageLayout pack_pub_params_layout(const spiral_gpu_params& p, const spiral_gpu_pack_shape& s, uint32_t out_n) {
    const size_t ex = p.direct_upload ? 0 : 1;
    return {{{ex * s.n_left, 2, p.t_exp}, {ex * s.n_right, 2, p.t_exp_right}, {ex, 2, 2 * p.t_conv}, {out_n, out_n + 1, p.t_conv}}, SEED_PACK_PUB_PARAMS};
}

// polynomials of the message in the NTT and the wire form / that the seeded form sends
inline size_t message_polys(const MessageLayout& m, Form form) {
    size_t n = 0;
    for (const MessagePart& t : m.part) n += t.polys() - (form == FORM_SEEDED ? t.row0() : 0);
    return n;
}
inline size_t message_bytes(const MessageLayout& m, Form form) {  // (the NTT form is no byte stream: one host buffer per part)
    return form == FORM_NTT ? 0 : (form == FORM_SEEDED ? kSeedBytes : 0) + message_polys(m, form) * kWirePolyBytes;
}

// what the client handed over: the NTT form's host buffers, one per part, or the message of the other two forms
struct MessageIn {
    const uint64_t* ntt[kMessageParts];
    const void* msg;
    size_t bytes;
};
// NTT form: every part the layout sends has its buffer (checked before anything is written)
inline int check_ntt_parts(const MessageLayout& m, const MessageIn& in, const char* what) {
    for (uint32_t i = 0; i < kMessageParts; i++)
        if (m.part[i].polys() && !in.ntt[i]) return fail("%s: null host buffer (part %u of the message)", what, i);
    return 0;
}

// ---- the ingest -------------------------------------------------------------------------------------------------------------------------------------
// NTT form: stage a host buffer of reference NTT-form polynomials ([2][N] u64 each) through `stage` and convert to PK
inline int upload_ref_ntt(DevBuf& stage, hipStream_t st, const uint64_t* host, uint64_t* pk, size_t npolys) {
    if (npolys == 0) return 0;
    if (!host) return fail("null host buffer");
    const size_t chunk = 4096;  // polynomials per staging pass (128 MiB)
    if (stage.words < std::min(npolys, chunk) * kRefNtt) {
        stage.release();
        if (stage.alloc(std::min(npolys, chunk) * kRefNtt)) return -1;
    }
    for (size_t done = 0; done < npolys; done += chunk) {
        const size_t n = std::min(chunk, npolys - done);
        HIP_OK(hipMemcpyAsync(stage.p, host + done * kRefNtt, n * kRefNtt * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        launch_ref_to_pk(stage.p, pk + done * kN, (uint32_t)n, identity_map(), st);
        HIP_OK(hipStreamSynchronize(st));
    }
    return 0;
}

// Wire form (include/spiral_gpu.h): one message = the parts' polynomials back to back, 7 bytes per raw coefficient.  The bytes go up through a
// device staging buffer a chunk at a time and each chunk is decoded + transformed straight into its PK destination by one launch (LD_WIRE); the
// launches and copies are ordered by the stream, so the host waits once, at the end, and then reads the lowest index of a coefficient above Q.
// The error word is tagged with the call's generation instead of being reset, and read back through a pinned word (messages of at most
// kWireHostCheckPolys polynomials are checked on the host instead: one copy up, one launch).  On failure the destinations hold a partial message: the caller drops what they held (have_query / have_pp).
// Seeded form: a 32-byte seed, then the wire form of every matrix without its row 0.  Row 0 of each matrix is generated on the device from the seed
// (seed.hip, one launch per part, queued ahead of the copies), and LD_WIRE's destination map steps over it.  Everything else -- staging, error word,
// the one synchronisation -- is the wire form's.
struct WireIn {  // a server's ingest workspace, reused from call to call
    DevBuf stage;                // [chunk bytes][u64 error word]
    size_t chunk_polys = 0;
    uint64_t* host_err = nullptr;  // pinned
    uint32_t gen = 0;
    void release() {
        stage.release();
        stage.words = 0;
        chunk_polys = 0;
        if (host_err) (void)hipHostFree(host_err);
        host_err = nullptr;
    }
};
constexpr size_t kWireChunkPolys = 4096;  // polynomials per staging pass (56 MiB)
// Up to this many polynomials (a compressed query: 2) the host checks the coefficients before anything goes up -- about 1 ns per coefficient, less
// than the readback of the device's error word, which is then skipped (a 2-polynomial set_query_wire took 34 us with the readback, set_query 28)
constexpr size_t kWireHostCheckPolys = 4;
inline int64_t wire_first_above_q(const uint8_t* b, size_t n) {
    for (size_t i = 0; i < n; i++, b += kWireCoeffBytes) {
        uint64_t v = 0;
        memcpy(&v, b, kWireCoeffBytes);  // (little-endian host)
        if (v > kQ) return (int64_t)i;
    }
    return -1;
}
// the message forms: part i of `m` into dst[i].  seed: null for the wire form; else the message's seed, with `wire` and `bytes` the rest
inline int ingest_message(WireIn& W, const DeviceTables& tb, hipStream_t st, const uint8_t* seed, const void* wire, size_t bytes, const MessageLayout& m,
                          uint64_t* const dst[kMessageParts], const char* what) {
    const size_t npolys = message_polys(m, seed ? FORM_SEEDED : FORM_WIRE);  // polynomials sent
    for (uint32_t i = 0; i < kMessageParts; i++)
        if (seed && m.part[i].count && m.part[i].rows < 2) return fail("%s: part %u is not a run of matrices with rows >= 2", what, i);
    if (!wire) return fail("%s: null wire buffer", what);
    if (seed && bytes != npolys * kWirePolyBytes) {
        const size_t nrow0 = message_polys(m, FORM_WIRE) - npolys;
        return fail("%s: %zu bytes, the seeded form of %zu polynomials (%zu of them row 0) takes %zu", what, bytes + kSeedBytes, npolys + nrow0, nrow0,
                    kSeedBytes + npolys * kWirePolyBytes);
    }
    if (bytes != npolys * kWirePolyBytes)
        return fail("%s: %zu bytes, the wire form of %zu polynomials takes %zu", what, bytes, npolys, npolys * kWirePolyBytes);
    if ((uint64_t)npolys * kN >= 0xffffffffull) return fail("%s: %zu polynomials exceed the coefficient index range", what, npolys);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIP_OK(hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail("%s: the server's stream is capturing (call it outside stream capture)", what);
    if (npolys == 0) return 0;
    const bool host_checked = npolys <= kWireHostCheckPolys;
    if (host_checked) {
        const int64_t i = wire_first_above_q((const uint8_t*)wire, npolys * kN);
        if (i >= 0) return fail("%s: coefficient %u (polynomial %u, index %u) is above Q", what, (uint32_t)i, (uint32_t)i / kN, (uint32_t)i % kN);
    }
    const size_t chunk = std::min(npolys, kWireChunkPolys);
    if (W.chunk_polys < chunk || W.gen == 0xffffffffu) {  // (re)allocated: the error word starts at generation 0 (all ones)
        W.stage.release();
        W.chunk_polys = 0;
        if (W.stage.alloc(chunk * kWirePolyBytes / 8 + 1)) return -1;
        HIP_OK(hipMemset(W.stage.p + chunk * kWirePolyBytes / 8, 0xff, sizeof(uint64_t)));
        W.chunk_polys = chunk;
        W.gen = 0;
    }
    if (!W.host_err) HIP_OK(hipHostMalloc((void**)&W.host_err, sizeof(uint64_t), hipHostMallocDefault));
    const uint32_t gen = ++W.gen;
    uint8_t* d_wire = reinterpret_cast<uint8_t*>(W.stage.p);
    uint64_t* d_err = W.stage.p + W.chunk_polys * kWirePolyBytes / 8;
    if (seed) {  // row 0 first: it needs nothing from the copies, so the device generates it while the host queues them
        size_t k = 0;
        for (uint32_t i = 0; i < kMessageParts; i++) {
            const uint32_t r = m.part[i].rows, c = m.part[i].cols;
            launch_seed_rows(seed, m.domain, k, dst[i], IndexMap{c, r * c, 0u}, (uint32_t)m.part[i].row0(), st);
            k += m.part[i].row0();
        }
    }
    FwdParams fp{};
    fp.src_map = fp.dst_map = identity_map();
    fp.n_digits = 1;
    fp.items = d_wire;
    fp.err = reinterpret_cast<uint32_t*>(d_err);
    fp.seed = gen;
    size_t first = 0;  // message index of the part's first polynomial
    for (uint32_t i = 0; i < kMessageParts; i++) {
        // the polynomials sent of a part: runs of `inner` (rows 1.. of a matrix), `outer` apart in the destination, `off` after its start
        const uint32_t r = seed ? m.part[i].rows : 1u, c = seed ? m.part[i].cols : 1u, inner = seed ? (r - 1u) * c : 1u, outer = r * c, off = seed ? c : 0u;
        const size_t sent = m.part[i].polys() - (seed ? m.part[i].row0() : 0);
        if (sent == 0) continue;  // (an absent matrix: W_exp on a direct-upload geometry)
        const size_t step = W.chunk_polys / inner * inner;  // (whole runs per chunk: a chunk's destination is one map from one base)
        if (step == 0) return fail("%s: a matrix of %u x %u polynomials exceeds the staging chunk", what, r, c);
        fp.dst_map = IndexMap{inner, outer, off};
        for (size_t done = 0; done < sent; done += step) {
            const size_t n = std::min(step, sent - done);
            HIP_OK(hipMemcpyAsync(d_wire, (const uint8_t*)wire + (first + done) * kWirePolyBytes, n * kWirePolyBytes, hipMemcpyHostToDevice, st));
            fp.dst = dst[i] + done / inner * outer * kN;
            fp.item_base = first + done;
            launch_ntt_forward(tb, fp, LD_WIRE, ST_PK, (uint32_t)n, st);
        }
        first += sent;
    }
    HIP_OK(hipGetLastError());
    if (host_checked) {
        HIP_OK(hipStreamSynchronize(st));
        return 0;
    }
    HIP_OK(hipMemcpyAsync(W.host_err, d_err, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const uint64_t err = *W.host_err;
    if ((uint32_t)(err >> 32) == ~gen) {
        const uint32_t i = (uint32_t)err;
        return fail("%s: coefficient %u (polynomial %u, index %u) is above Q", what, i, i / kN, i % kN);
    }
    return 0;
}

// The workspace of the batch ingest (server_lanes.cpp spiral_gpu_server_set_query_batch), owned by the batch's servers[0] and used on its stream only:
// the device staging [u64 error word, padded to 256 bytes][lane][head + chunk polynomials], the generation of the error word as WireIn's, and for
// messages small enough to check on the host a ring of two pinned slots laid out as the staging, each with the event recorded behind the launch
// that read it -- a call waits for that event before it fills the slot again, never for the stream.
struct QueryBatchIn {
    static constexpr size_t kErrWords = 32;
    DevBuf stage;
    size_t stage_bytes = 0;  // behind the error word
    uint64_t* host_err = nullptr;  // pinned
    uint32_t gen = 0;
    struct Slot {
        uint8_t* p = nullptr;  // pinned
        size_t bytes = 0;
        hipEvent_t ev = nullptr;
        bool in_flight = false;
    } ring[2];
    uint32_t next = 0;
    hipStream_t last_stream = nullptr;  // the staging's last user, ordered by `last` in front of a call on another stream (set_stream)
    hipEvent_t last = nullptr;
    uint8_t* bytes() const { return reinterpret_cast<uint8_t*>(stage.p + kErrWords); }
    // at least `need` bytes of staging behind an error word of generation < 0xffffffff
    int reserve(size_t need, hipStream_t st) {
        if (stage.p && stage_bytes >= need && gen != 0xffffffffu) return 0;
        stage.release();  // (hipFree waits for whatever still reads it)
        stage_bytes = 0;
        const size_t words = (need + 7) / 8;
        if (stage.alloc(kErrWords + words)) return -1;
        HIP_OK(hipMemsetAsync(stage.p, 0xff, kErrWords * sizeof(uint64_t), st));  // generation 0: all ones
        stage_bytes = words * 8;
        gen = 0;
        return 0;
    }
    void release() {
        stage.release();
        stage_bytes = 0;
        if (host_err) (void)hipHostFree(host_err);
        host_err = nullptr;
        for (Slot& s : ring) {
            if (s.ev) (void)hipEventSynchronize(s.ev), (void)hipEventDestroy(s.ev);
            if (s.p) (void)hipHostFree(s.p);
            s = Slot{};
        }
        last = nullptr;  // (one of the slots' events)
        last_stream = nullptr;
    }
};

// a server's two ingest workspaces and where its ingests run
struct IngestOn {
    DevBuf& stage;  // the NTT form's staging
    WireIn& wire;   // the message forms'
    const DeviceTables& tb;
    hipStream_t st;
};
// One message in any form: part i of `m` into the PK buffer dst[i], on `on.st`; returns synchronised.  A failure may leave the destinations
// half-written: the servers' take_query / take_pub_params drop what they held (and refuse a null NTT-form buffer, check_ntt_parts, before that).
inline int ingest(Form form, const IngestOn& on, const MessageLayout& m, uint64_t* const dst[kMessageParts], const MessageIn& in, const char* what) {
    if (form == FORM_NTT) {
        for (uint32_t i = 0; i < kMessageParts; i++)
            if (upload_ref_ntt(on.stage, on.st, in.ntt[i], dst[i], m.part[i].polys())) return -1;
        return 0;
    }
    if (form == FORM_WIRE) return ingest_message(on.wire, on.tb, on.st, nullptr, in.msg, in.bytes, m, dst, what);
    if (!in.msg) return fail("%s: null message", what);
    if (in.bytes < kSeedBytes) return fail("%s: %zu bytes, shorter than the %u-byte seed", what, in.bytes, kSeedBytes);
    return ingest_message(on.wire, on.tb, on.st, (const uint8_t*)in.msg, (const uint8_t*)in.msg + kSeedBytes, in.bytes - kSeedBytes, m, dst, what);
}

}  // namespace host
}  // namespace spiral
