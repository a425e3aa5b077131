// The client session of include/spiral_gpu.h (spiral_gpu_client_*): one client's secret key resident on the device, drawn from a 32-byte seed by
// the format of client_device.h; its public parameters and batches of its queries, each one table-driven sample launch between the transforms of
// its noise and the form it leaves in; and the decoding of batches of responses in one launch (the kernels: client.hip).
//
// The values restate Client and PackClient of cli/client.cpp (the reference's src/client.cpp, src/testing.cpp): Regev columns (-a ; a s + e), fresh
// public keys (-A ; Sp A + E), W_exp = encryptions of tau_i(s0) g, W, V, v_W, SpiralPack's V with its s0^2 columns, the query plaintext sigma and
// the direct-upload ciphertexts.  Every plaintext is a constant times one of a handful of secret-derived NTT polynomials -- the session's secret
// table, built once per key -- so a column is (k, destination, noise polynomial, table polynomial, constant): the descriptors are built here, on
// the host, and the device does the rest.
#include "client_device.h"
#include "message.h"
#include "kv_host.h"
#include "records_host.h"

using namespace spiral;
using namespace spiral::host;

struct spiral_gpu_client {
    spiral_gpu_params p{};
    uint32_t out_n = 0;
    uint32_t rows = 0, cols = 0;  // Sp's rows and the response's columns: 2, 2 for base Spiral, out_n, out_n for SpiralPack
    uint64_t qprime = 0;
    int device = 0;
    bool nonoise = false;
    uint8_t seed[kSeedBytes] = {};
    hipStream_t stream = nullptr;
    DevBuf table;    // the 128 thresholds
    DevBuf secret;   // raw values mod Q: sr, then the rows of Sp, [1 + rows][2048]
    DevBuf centred;  // the same samples as 8-bit values, [1 + rows][2048] bytes
    DevBuf in, out;  // decode's staging, grown on demand
    DevBuf expected; // response_noise's expected plaintexts, grown on demand
    // the message half
    DeviceTables tb;
    uint64_t counter = 1;  // the next query's message number (the public parameters are message 0)
    uint32_t n_tau = 0;    // automorphisms tau_i(s0) the expansion keys encrypt
    DevBuf tab;            // the secret table, PK: [ONE, s0, Sp_r.., Sp_r s0.., s0^2, tau_i(s0)..]
    DevBuf keys, columns, sigma, noise_raw, noise_pk, msg, lifted, stage;  // a call's workspace, grown on demand
    uint32_t t_one() const { return 0; }
    uint32_t t_s0() const { return 1; }
    uint32_t t_sp() const { return 2; }
    uint32_t t_sps0() const { return 2 + rows; }
    uint32_t t_s0sq() const { return 2 + 2 * rows; }
    uint32_t t_tau() const { return 3 + 2 * rows; }
    uint32_t t_polys() const { return 3 + 2 * rows + n_tau; }
};

namespace {

void client_free(spiral_gpu_client* c) {
    c->table.release();
    c->secret.release();
    c->centred.release();
    c->in.release();
    c->out.release();
    c->expected.release();
    for (DevBuf* b : {&c->tab, &c->keys, &c->columns, &c->sigma, &c->noise_raw, &c->noise_pk, &c->msg, &c->lifted, &c->stage}) b->release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int client_on(spiral_gpu_client* c, const char* what) {
    if (!c) return fail("%s: null client session", what);
    HIP_OK(hipSetDevice(c->device));
    return 0;
}

int8_t* centred_of(spiral_gpu_client* c) { return reinterpret_cast<int8_t*>(c->centred.p); }

int grow(DevBuf& b, size_t words) {
    if (b.p && b.words >= words) return 0;
    b.release();
    return b.alloc(words);
}


// ---- the secret table ---------------------------------------------------------------------------------------------------------------------------
// from the raw secret on the device: transforms of s0, the rows of Sp and tau_i(s0) (x -> x^(N / 2^i + 1), src/client.cpp:270-293), then the products
int build_table(spiral_gpu_client* c) {
    const uint32_t rows = c->rows, n_raw = 1 + rows + c->n_tau;
    if (grow(c->stage, (size_t)n_raw * kN)) return -1;
    HIP_OK(hipMemcpyAsync(c->stage.p, c->secret.p, (size_t)(1 + rows) * kPolyBytes, hipMemcpyDeviceToDevice, c->stream));
    for (uint32_t i = 0; i < c->n_tau; i++) launch_automorph(c->secret.p, c->stage.p + (size_t)(1 + rows + i) * kN, 1, (kN >> i) + 1, c->stream);
    launch_job(c->tb, raw_job(c->stage.p, c->tab.p + (size_t)c->t_s0() * kN, 1 + rows), c->stream);
    if (c->n_tau) launch_job(c->tb, raw_job(c->stage.p + (size_t)(1 + rows) * kN, c->tab.p + (size_t)c->t_tau() * kN, c->n_tau), c->stream);
    const uint64_t* s0 = c->tab.p + (size_t)c->t_s0() * kN;
    for (uint32_t r = 0; r < rows; r++)
        launch_client_mul(c->tab.p + (size_t)(c->t_sp() + r) * kN, s0, c->tab.p + (size_t)(c->t_sps0() + r) * kN, 1, c->stream);
    launch_client_mul(s0, s0, c->tab.p + (size_t)c->t_s0sq() * kN, 1, c->stream);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- messages -------------------------------------------------------------------------------------------------------------------------------------
uint64_t gadget_const(uint32_t t, uint32_t j) {  // buildGadget's entry j of a row of t digits (src/util.cpp:89-106)
    const uint64_t sh = (uint64_t)get_bits_per(t) * j;
    return sh >= 64 ? 0 : 1ull << sh;
}
void set_const(ClientColumn& col, uint64_t v) {
    col.c_p = (uint32_t)(v % kP);
    col.c_b = (uint32_t)(v % kB);
}
uint64_t inv_mod_q(uint64_t a) {
    __int128 t = 0, nt = 1, r = kQ, nr = a % kQ;
    while (nr != 0) {
        const __int128 q = r / nr;
        __int128 tmp = t - q * nt;
        t = nt, nt = tmp;
        tmp = r - q * nr;
        r = nr, nr = tmp;
    }
    return (uint64_t)(t < 0 ? t + kQ : t);
}

// the columns of a message in layout order, with everything the layout alone fixes: k, destination, noise polynomial (the i-th polynomial the seeded
// form transmits carries noise polynomial i: matrix by matrix, rows 1.., column by column).  fill(part, matrix, column, descriptor) sets the rest
template <class Fill>
std::vector<ClientColumn> message_columns(const MessageLayout& m, Fill fill) {
    std::vector<ClientColumn> cols;
    uint32_t start = 0, k = 0, noise = 0;
    for (uint32_t i = 0; i < kMessageParts; i++) {
        const MessagePart& t = m.part[i];
        for (uint32_t mi = 0; mi < t.count; mi++)
            for (uint32_t cc = 0; cc < t.cols; cc++) {
                ClientColumn col{};
                col.k = k + mi * t.cols + cc;
                col.dst = start + mi * t.rows * t.cols + cc;
                col.dst_stride = t.cols;
                col.rows = t.rows;
                col.noise = noise + mi * (t.rows - 1) * t.cols + cc;
                col.noise_stride = t.cols;
                col.m_row = kClientNoMessage;
                fill(i, mi, cc, col);
                cols.push_back(col);
            }
        start += (uint32_t)t.polys();
        k += (uint32_t)t.row0();
        noise += (uint32_t)(t.polys() - t.row0());
    }
    return cols;
}

std::vector<ClientColumn> pub_params_columns(const spiral_gpu_client* c, const MessageLayout& m) {
    const uint32_t tc = c->p.t_conv;
    return message_columns(m, [&](uint32_t part, uint32_t mi, uint32_t cc, ClientColumn& col) {
        if (part < 2) {  // W_exp: Regev encryptions under s0 of tau_i(s0) g
            col.s_first = c->t_s0();
            col.m_row = 1;
            col.m_idx = c->t_tau() + mi;
            set_const(col, gadget_const(m.part[part].cols, cc));
        } else if (c->out_n == 0 && part == 2) {  // W = P + pad(s0 G_scale): column i + 2 j carries s0 2^(bits j) on row i
            col.s_first = c->t_sp();
            col.m_row = 1 + cc % 2;
            col.m_idx = c->t_s0();
            set_const(col, gadget_const(tc, cc / 2));
        } else if (c->out_n == 0) {  // V = P + pad(Sp [s0 gv | gv])
            col.s_first = c->t_sp();
            col.m_row = 0;
            col.m_idx = cc < tc ? c->t_sps0() : c->t_sp();
            col.m_stride = 1;
            set_const(col, gadget_const(tc, cc % tc));
        } else if (part == 2) {  // SpiralPack's V: Regev encryptions of s0^2 2^(bits j) (even columns) and s0 2^(bits j) (odd)
            col.s_first = c->t_s0();
            col.m_row = 1;
            col.m_idx = cc % 2 == 0 ? c->t_s0sq() : c->t_s0();
            set_const(col, gadget_const(tc, cc / 2));
        } else {  // v_W[i] = P + s0 g on row i
            col.s_first = c->t_sp();
            col.m_row = 1 + mi;
            col.m_idx = c->t_s0();
            set_const(col, gadget_const(tc, cc));
        }
    });
}

// what a query of item idx needs beyond the layout: its columns, and for a compressed query the plaintext sigma (raw, added to the noise)
struct QueryShape {
    uint32_t dim0, num_per, ell, g, stopround, n_query_cts;
    bool packed_layout;  // sigma in the stopround > 0 form (SpiralPack always)
};
void query_sigma(const spiral_gpu_client* c, const QueryShape& s, uint64_t idx, uint64_t* sigma) {  // src/spiral.cpp:2104-2152, src/testing.cpp:991-1006
    typedef unsigned __int128 u128;
    const uint64_t idx_dim0 = idx / s.num_per, idx_further = idx % s.num_per, scale_k = kQ / c->p.p_db;
    const uint32_t bits = get_bits_per(s.ell);
    std::fill(sigma, sigma + kN, 0);
    if (s.packed_layout) {
        sigma[2 * idx_dim0] = scale_k % kQ;
        for (uint32_t i = 0; i < c->p.nu2; i++)
            for (uint32_t j = 0; j < s.ell; j++) sigma[2 * (i * s.ell + j) + 1] = ((1ull << (bits * j)) * ((idx_further >> i) & 1)) % kQ;
        const uint64_t inv_first = inv_mod_q(1ull << s.g), inv_rest = inv_mod_q(1ull << (s.stopround + 1));
        for (uint32_t i = 0; i < kN / 2; i++) {
            sigma[2 * i] = (uint64_t)((u128)sigma[2 * i] * inv_first % kQ);
            sigma[2 * i + 1] = (uint64_t)((u128)sigma[2 * i + 1] * inv_rest % kQ);
        }
    } else {
        sigma[idx_dim0] = scale_k % kQ;
        uint32_t ctr = 0;
        for (uint32_t i = 0; i < c->p.nu2; i++)
            for (uint32_t j = 0; j < s.ell; j++) sigma[s.dim0 + ctr++] = ((1ull << (bits * j)) * ((idx_further >> i) & 1)) % kQ;
        const uint64_t inv = inv_mod_q(1ull << s.g);
        for (uint32_t i = 0; i < kN; i++) sigma[i] = (uint64_t)((u128)sigma[i] * inv % kQ);
    }
}
std::vector<ClientColumn> query_columns(const spiral_gpu_client* c, const MessageLayout& m, const QueryShape& s, uint64_t idx) {
    const uint64_t idx_dim0 = idx / s.num_per, idx_further = idx % s.num_per, scale_k = kQ / c->p.p_db;
    const uint32_t bits = get_bits_per(s.ell);
    return message_columns(m, [&](uint32_t, uint32_t mi, uint32_t, ClientColumn& col) {
        col.s_first = c->t_s0();
        if (!c->p.direct_upload) return;  // one ciphertext of sigma: the plaintext rides on the noise
        col.m_row = 1;
        col.m_idx = c->t_one();
        if (mi < s.dim0) return set_const(col, mi == idx_dim0 ? scale_k : 0);  // src/spiral.cpp:2177-2188
        // the GSW bits.  Base: ciphertext dim0 + i ell + j encrypts bit_i 2^(bits j); SpiralStreamPack: the pair 2 (i ell + j), + 1 encrypts
        // s0 bit_i 2^(bits j) and bit_i 2^(bits j) (src/testing.cpp:966-989)
        const uint32_t t = mi - s.dim0, d = c->out_n ? t / 2 : t, i = d / s.ell, j = d % s.ell;
        if (c->out_n && t % 2 == 0) col.m_idx = c->t_s0();
        set_const(col, (1ull << (bits * j)) * ((idx_further >> i) & 1));
    });
}

void message_keys(const spiral_gpu_client* c, uint64_t number, uint32_t seed[8], uint32_t noise_key[8]) {
    const Seed K = seed_words(c->seed);
    uint32_t w[16];
    chacha20_block(K.w, 0, CLIENT_MSG_SEED, (uint32_t)number, (uint32_t)(number >> 32), w);
    std::copy(w, w + 8, seed);
    chacha20_block(K.w, 0, CLIENT_NOISE_KEY, (uint32_t)number, (uint32_t)(number >> 32), w);
    std::copy(w, w + 8, noise_key);
}
void seed_bytes(const uint32_t seed[8], uint8_t* out) {
    for (int i = 0; i < 32; i++) out[i] = (uint8_t)(seed[i / 4] >> (8 * (i % 4)));
}

// n messages of layout m, numbers first .. first + n - 1, into c->msg as [n][polynomials of the message] PK: the noise of all of them, its transforms,
// one sample launch.  cols: [n][columns]; sigma: null or [n][2048] raw plaintexts added to noise polynomial 0.  seeds_out: [n][8] words
int generate(spiral_gpu_client* c, const MessageLayout& m, const std::vector<ClientColumn>& cols, uint32_t n, uint64_t first, const uint64_t* sigma,
             std::vector<uint32_t>& seeds_out) {
    const uint32_t polys = (uint32_t)message_polys(m, FORM_NTT), n_tx = (uint32_t)message_polys(m, FORM_SEEDED), n_cols = (uint32_t)(cols.size() / n);
    std::vector<uint32_t> keys((size_t)n * 16);  // [n] seeds, then [n] noise keys
    for (uint32_t b = 0; b < n; b++) message_keys(c, first + b, &keys[8 * b], &keys[8 * (n + b)]);
    seeds_out.assign(keys.begin(), keys.begin() + 8 * n);
    if (grow(c->keys, (size_t)n * 8) || grow(c->columns, (cols.size() * sizeof(ClientColumn) + 7) / 8) || grow(c->noise_raw, (size_t)n * n_tx * kN) ||
        grow(c->noise_pk, (size_t)n * n_tx * kN) || grow(c->msg, (size_t)n * polys * kN) || (sigma && grow(c->sigma, (size_t)n * kN)))
        return -1;
    HIP_OK(hipMemcpyAsync(c->keys.p, keys.data(), keys.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->columns.p, cols.data(), cols.size() * sizeof(ClientColumn), hipMemcpyHostToDevice, c->stream));
    if (sigma) HIP_OK(hipMemcpyAsync(c->sigma.p, sigma, (size_t)n * kPolyBytes, hipMemcpyHostToDevice, c->stream));
    const uint32_t* d_keys = reinterpret_cast<const uint32_t*>(c->keys.p);
    launch_client_noise(d_keys + 8 * n, CLIENT_NOISE, 0, c->table.p, c->noise_raw.p, nullptr, sigma ? c->sigma.p : nullptr, n_tx, n, c->nonoise, c->stream);
    launch_job(c->tb, raw_job(c->noise_raw.p, c->noise_pk.p, n * n_tx), c->stream);
    ClientSampleParams sp{};
    sp.seeds = d_keys;
    sp.columns = reinterpret_cast<const ClientColumn*>(c->columns.p);
    sp.table = c->tab.p;
    sp.noise = c->noise_pk.p;
    sp.out = c->msg.p;
    sp.domain = m.domain;
    sp.n_cols = n_cols;
    sp.noise_polys = n_tx;
    sp.msg_polys = polys;
    launch_client_sample(sp, n, c->stream);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(c->stream));  // (the host vectors above go out of scope)
    return 0;
}

// polynomials first .. first + npolys - 1 of c->msg to a host buffer in the reference NTT layout
int emit_ref(spiral_gpu_client* c, size_t first, size_t npolys, uint64_t* host) {
    const size_t chunk = 2048;  // polynomials per staging pass (64 MiB)
    if (npolys == 0) return 0;
    if (grow(c->stage, std::min(npolys, chunk) * kRefNtt)) return -1;
    for (size_t done = 0; done < npolys; done += chunk) {
        const size_t k = std::min(chunk, npolys - done);
        launch_pk_to_ref(c->msg.p + (first + done) * kN, c->stage.p, (uint32_t)k, identity_map(), c->stream);
        HIP_OK(hipMemcpyAsync(host + done * kRefNtt, c->stage.p, k * kRefNtt * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// the n messages of c->msg as bytes: the existing inverse transform + CRT lift of the polynomials the form sends (all of them, or rows 1.. of every
// matrix), encoded to 7 bytes per coefficient on the device; message b's bytes go to out + b * bytes_each, the seeded form's behind its seed.  A
// call of several messages takes a layout of one part (a query): then the matrices of all messages are one run.
int emit_bytes(spiral_gpu_client* c, const MessageLayout& m, uint32_t n, bool seeded, const std::vector<uint32_t>& seeds, uint8_t* out, size_t bytes_each) {
    const size_t sent = message_polys(m, seeded ? FORM_SEEDED : FORM_WIRE), head = seeded ? kSeedBytes : 0;
    if (grow(c->lifted, n * sent * kN) || grow(c->stage, n * sent * kWirePolyBytes / 8)) return -1;
    size_t src = 0, dst = 0;
    for (uint32_t i = 0; i < kMessageParts; i++) {
        const MessagePart& t = m.part[i];
        const size_t part_sent = n * (t.polys() - (seeded ? t.row0() : 0));
        if (part_sent == 0) continue;
        LiftOpts o;
        if (seeded) o.src_map = IndexMap{(t.rows - 1) * t.cols, t.rows * t.cols, t.cols};
        launch_job(c->tb, lift_job(c->msg.p + src * kN, c->lifted.p + dst * kN, (uint32_t)part_sent, o), c->stream);
        src += n * t.polys();
        dst += part_sent;
    }
    launch_client_wire_encode(c->lifted.p, reinterpret_cast<uint8_t*>(c->stage.p), (uint32_t)(n * sent), c->stream);
    HIP_OK(hipGetLastError());
    for (uint32_t b = 0; b < n; b++) {
        if (seeded) seed_bytes(&seeds[8 * b], out + b * bytes_each);
        HIP_OK(hipMemcpyAsync(out + b * bytes_each + head, reinterpret_cast<const uint8_t*>(c->stage.p) + b * sent * kWirePolyBytes, sent * kWirePolyBytes,
                              hipMemcpyDeviceToHost, c->stream));
    }
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

int layouts_of(const spiral_gpu_client* c, MessageLayout* pp, MessageLayout* query, QueryShape* qs) {
    if (c->out_n == 0) {
        spiral_gpu_shape s;
        if (shape_of(&c->p, &s)) return -1;
        if (pp) *pp = pub_params_layout(c->p, s);
        if (query) *query = query_layout(c->p, s);
        if (qs) *qs = QueryShape{s.dim0, s.num_per, s.ell, s.g, s.stopround, s.n_query_cts, s.stopround != 0};
    } else {
        spiral_gpu_pack_shape s;
        if (spiral_gpu_pack_get_shape(&c->p, c->out_n, &s)) return -1;
        if (pp) *pp = pack_pub_params_layout(c->p, s, c->out_n);
        if (query) *query = pack_query_layout(c->p, s, c->out_n);
        if (qs) *qs = QueryShape{s.dim0, s.num_per, s.ell, s.g, s.stopround, s.n_query_cts, true};
    }
    return 0;
}

int make_pub_params(spiral_gpu_client* c, MessageLayout* m, std::vector<uint32_t>* seeds) {
    if (layouts_of(c, m, nullptr, nullptr)) return -1;
    return generate(c, *m, pub_params_columns(c, *m), 1, 0, nullptr, *seeds);
}

}  // namespace

extern "C" {

int spiral_gpu_client_noise_table(uint64_t* out) {
    if (!out) return fail("client_noise_table: null argument");
    client_noise_table(out);
    return 0;
}

int spiral_gpu_client_create(const spiral_gpu_params* p, uint32_t out_n, int device, const void* seed32, int nonoise, spiral_gpu_client** out) {
    if (!out) return fail("client_create: null argument");
    *out = nullptr;
    if (!p || !seed32) return fail("client_create: null argument");
    uint64_t qprime = 0;
    uint32_t n_tau = 0;
    if (out_n == 0) {
        spiral_gpu_shape s;
        if (shape_of(p, &s)) return -1;
        qprime = s.qprime;
        n_tau = std::max(s.n_left, s.n_right);
    } else {
        spiral_gpu_pack_shape s;
        if (spiral_gpu_pack_get_shape(p, out_n, &s)) return -1;
        qprime = s.qprime;
        n_tau = p->direct_upload ? 0 : std::max(s.n_left, s.n_right);
    }
    // the decode's 32-bit operands and 64-bit rounding: |vf| <= q'/2, |vr| <= 2 p_db, so |vf 4p + vr q'| + 2 q' <= 4 p q' + 2 q'
    if (qprime >= (1ull << 31) || (unsigned __int128)qprime * (4 * p->p_db + 2) >= ((unsigned __int128)1 << 62))
        return fail("client_create: q' = %llu with p_db = %llu is outside the exact range of the device decode", (unsigned long long)qprime,
                    (unsigned long long)p->p_db);
    HIP_OK(hipSetDevice(device));
    spiral_gpu_client* c = new spiral_gpu_client();
    c->p = *p;
    c->out_n = out_n;
    c->rows = c->cols = out_n ? out_n : 2u;
    c->qprime = qprime;
    c->device = device;
    c->nonoise = nonoise != 0;
    memcpy(c->seed, seed32, kSeedBytes);
    const size_t polys = 1 + c->rows;
    c->n_tau = n_tau;
    uint64_t table[kNoiseThresholds];
    client_noise_table(table);
    if (hipStreamCreate(&c->stream) != hipSuccess || c->table.alloc(kNoiseThresholds) || c->secret.alloc(polys * kN) || c->centred.alloc(polys * kN / 8) ||
        hipMemcpyAsync(c->table.p, table, sizeof(table), hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        (void)hipGetLastError();
        client_free(c);
        return fail("client_create: stream or device memory setup failed on device %d", device);
    }
    const Seed K = seed_words(c->seed);
    std::vector<uint64_t> one(kN, 1ull | (1ull << 32));  // the constant polynomial 1 in NTT form
    if (tables_get(device, &c->tb) != 0 || c->keys.alloc(8) || c->tab.alloc((size_t)c->t_polys() * kN) ||
        hipMemcpyAsync(c->keys.p, K.w, sizeof(K.w), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(c->tab.p, one.data(), kPolyBytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        (void)hipGetLastError();
        client_free(c);
        return fail("client_create: table setup failed on device %d", device);
    }
    launch_client_noise(reinterpret_cast<const uint32_t*>(c->keys.p), CLIENT_SECRET, 0, c->table.p, c->secret.p, centred_of(c), nullptr, (uint32_t)polys, 1,
                        c->nonoise, c->stream);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess || build_table(c)) {
        client_free(c);
        return fail("client_create: the secret's launches failed on device %d", device);
    }
    *out = c;
    return 0;
}

void spiral_gpu_client_destroy(spiral_gpu_client* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    client_free(c);
}

int spiral_gpu_client_get_secret(spiral_gpu_client* c, uint64_t* sr, uint64_t* sp) {
    if (client_on(c, "client_get_secret")) return -1;
    if (sr) HIP_OK(hipMemcpyAsync(sr, c->secret.p, kPolyBytes, hipMemcpyDeviceToHost, c->stream));
    if (sp) HIP_OK(hipMemcpyAsync(sp, c->secret.p + kN, c->rows * kPolyBytes, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

int spiral_gpu_client_set_secret(spiral_gpu_client* c, const uint64_t* sr, const uint64_t* sp) {
    if (client_on(c, "client_set_secret")) return -1;
    if (!sr || !sp) return fail("client_set_secret: null argument");
    const size_t polys = 1 + c->rows;
    std::vector<uint64_t> raw(polys * kN);
    std::vector<int8_t> cen(polys * kN);
    for (size_t i = 0; i < raw.size(); i++) {
        const uint64_t x = i < kN ? sr[i] : sp[i - kN];
        if (x > (uint64_t)kNoiseBound && (x >= kQ || x < kQ - (uint64_t)kNoiseBound))
            return fail("client_set_secret: coefficient %zu of %s is outside [-%d, %d] mod Q", i < kN ? i : i - kN, i < kN ? "sr" : "Sp", kNoiseBound, kNoiseBound);
        raw[i] = x;
        cen[i] = x <= (uint64_t)kNoiseBound ? (int8_t)x : (int8_t)-(int64_t)(kQ - x);
    }
    HIP_OK(hipMemcpyAsync(c->secret.p, raw.data(), raw.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(c->centred.p, cen.data(), cen.size(), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return build_table(c);
}

int spiral_gpu_client_get_counter(spiral_gpu_client* c, uint64_t* n) {
    if (!c || !n) return fail("client_get_counter: null %s", c ? "argument" : "client session");
    *n = c->counter;
    return 0;
}
int spiral_gpu_client_set_counter(spiral_gpu_client* c, uint64_t n) {
    if (!c) return fail("client_set_counter: null client session");
    if (n == 0) return fail("client_set_counter: message 0 is the public parameters; queries are numbered from 1");
    c->counter = n;
    return 0;
}

int spiral_gpu_client_pub_params(spiral_gpu_client* c, uint64_t* w_left, uint64_t* w_right, uint64_t* w_or_v, uint64_t* v_or_vw) {
    if (client_on(c, "client_pub_params")) return -1;
    MessageLayout m;
    std::vector<uint32_t> seeds;
    if (make_pub_params(c, &m, &seeds)) return -1;
    uint64_t* const outs[kMessageParts] = {w_left, w_right, w_or_v, v_or_vw};
    size_t first = 0;
    for (uint32_t i = 0; i < kMessageParts; i++) {
        if (outs[i] && emit_ref(c, first, m.part[i].polys(), outs[i])) return -1;
        first += m.part[i].polys();
    }
    return 0;
}

int spiral_gpu_client_pub_params_msg(spiral_gpu_client* c, int form, void* msg, size_t capacity) {
    if (client_on(c, "client_pub_params_msg")) return -1;
    if (!msg) return fail("client_pub_params_msg: null argument");
    if (form != SPIRAL_GPU_FORM_WIRE && form != SPIRAL_GPU_FORM_SEEDED) return fail("client_pub_params_msg: form %d is neither WIRE nor SEEDED", form);
    MessageLayout m;
    if (layouts_of(c, &m, nullptr, nullptr)) return -1;
    const size_t bytes = message_bytes(m, form == SPIRAL_GPU_FORM_SEEDED ? FORM_SEEDED : FORM_WIRE);
    if (capacity < bytes) return fail("client_pub_params_msg: a capacity of %zu bytes, the message takes %zu", capacity, bytes);
    std::vector<uint32_t> seeds;
    if (make_pub_params(c, &m, &seeds)) return -1;
    return emit_bytes(c, m, 1, form == SPIRAL_GPU_FORM_SEEDED, seeds, (uint8_t*)msg, bytes);
}

int spiral_gpu_client_queries(spiral_gpu_client* c, const uint64_t* idx, uint32_t n, int form, void* out, size_t bytes_each) {
    if (client_on(c, "client_queries")) return -1;
    if (!idx || !out) return fail("client_queries: null argument");
    if (form != SPIRAL_GPU_FORM_NTT && form != SPIRAL_GPU_FORM_WIRE && form != SPIRAL_GPU_FORM_SEEDED) return fail("client_queries: unknown form %d", form);
    if (n == 0) return fail("client_queries: 0 queries");
    MessageLayout m;
    QueryShape qs;
    if (layouts_of(c, nullptr, &m, &qs)) return -1;
    const size_t polys = message_polys(m, FORM_NTT);
    const size_t want = form == SPIRAL_GPU_FORM_NTT ? polys * kRefNtt * sizeof(uint64_t) : message_bytes(m, form == SPIRAL_GPU_FORM_SEEDED ? FORM_SEEDED : FORM_WIRE);
    if (bytes_each != want) return fail("client_queries: bytes_each = %zu, a query in this form takes %zu", bytes_each, want);
    const uint64_t items = (uint64_t)qs.dim0 * qs.num_per;
    for (uint32_t b = 0; b < n; b++)
        if (idx[b] >= items) return fail("client_queries: index %llu (query %u) outside the database of %llu items", (unsigned long long)idx[b], b, (unsigned long long)items);
    if (c->counter + n < c->counter) return fail("client_queries: the message counter would wrap");
    const uint32_t per_pass = (uint32_t)std::max<size_t>(1, std::min<size_t>(65535, ((size_t)1 << 16) / polys));  // at most 2^16 polynomials (1 GiB) per pass
    std::vector<uint64_t> sigma;
    std::vector<uint32_t> seeds;
    for (uint32_t done = 0; done < n; done += per_pass) {
        const uint32_t k = std::min(per_pass, n - done);
        std::vector<ClientColumn> cols;
        for (uint32_t b = 0; b < k; b++) {
            const std::vector<ClientColumn> one = query_columns(c, m, qs, idx[done + b]);
            cols.insert(cols.end(), one.begin(), one.end());
        }
        if (!c->p.direct_upload) {
            sigma.resize((size_t)k * kN);
            for (uint32_t b = 0; b < k; b++) query_sigma(c, qs, idx[done + b], &sigma[(size_t)b * kN]);
        }
        if (generate(c, m, cols, k, c->counter + done, c->p.direct_upload ? nullptr : sigma.data(), seeds)) return -1;
        uint8_t* dst = (uint8_t*)out + (size_t)done * bytes_each;
        if (form == SPIRAL_GPU_FORM_NTT ? emit_ref(c, 0, (size_t)k * polys, (uint64_t*)dst) : emit_bytes(c, m, k, form == SPIRAL_GPU_FORM_SEEDED, seeds, dst, bytes_each))
            return -1;
    }
    c->counter += n;
    return 0;
}

int spiral_gpu_client_decode(spiral_gpu_client* c, const void* responses, uint32_t n, int form, uint64_t* plaintexts) {
    if (client_on(c, "client_decode")) return -1;
    if (!responses || !plaintexts) return fail("client_decode: null argument");
    if (form != SPIRAL_GPU_RESPONSE_RAW && form != SPIRAL_GPU_RESPONSE_WIRE) return fail("client_decode: unknown response form %d", form);
    if (n == 0 || n > 65535u) return fail("client_decode: %u responses, a call takes 1 .. 65535", n);
    const bool wire = form == SPIRAL_GPU_RESPONSE_WIRE;
    const size_t wire_each = wire_bytes(&c->p, c->cols);  // a multiple of 256 bytes
    const size_t in_words = wire ? wire_each / 8 : (size_t)(c->rows + 1) * c->cols * kN, out_words = (size_t)c->rows * c->cols * kN;
    if (grow(c->in, n * in_words + 1) || grow(c->out, n * out_words)) return -1;
    HIP_OK(hipMemcpyAsync(c->in.p, responses, n * in_words * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemsetAsync(c->in.p + n * in_words, 0, sizeof(uint64_t), c->stream));  // (the word a wire field's window may reach into)
    ClientDecodeParams dp{};
    dp.sp = centred_of(c) + kN;
    dp.resp = c->in.p;
    dp.out = c->out.p;
    dp.rows = c->rows;
    dp.cols = c->cols;
    dp.wire = wire ? 1 : 0;
    dp.w0 = c->p.qprime_bits;
    dp.w1 = wire_bits_rest(&c->p);
    dp.wire_words = wire_each / 8;
    dp.qprime = c->qprime;
    dp.p_db = c->p.p_db;
    launch_client_decode(dp, n, c->stream);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(plaintexts, c->out.p, n * out_words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- records (include/spiral_gpu.h "Records"): a client's queries for, and decode of, records of any byte size; base and SpiralPack sessions --------------------------------
namespace {
int client_record_layout(spiral_gpu_client* c, const char* what, uint64_t record_bytes, const uint64_t* record_ids, uint32_t n, spiral_gpu_record_layout* l) {
    if (record_layout(&c->p, record_bytes, l, c->out_n)) return -1;
    for (uint32_t k = 0; k < n; k++)
        if (record_ids[k] >= l->capacity)
            return fail("%s: record id %llu (position %u) outside the database of %llu records", what, (unsigned long long)record_ids[k], k, (unsigned long long)l->capacity);
    return 0;
}
}  // namespace

// client_queries for the items the records live in: one query per record (it also serves every instance of a record of several)
int spiral_gpu_client_record_queries(spiral_gpu_client* c, uint64_t record_bytes, const uint64_t* record_ids, uint32_t n, int form, void* out, size_t bytes_each) {
    if (client_on(c, "client_record_queries")) return -1;
    if (!record_ids || !out) return fail("client_record_queries: null argument");
    spiral_gpu_record_layout l;
    if (client_record_layout(c, "client_record_queries", record_bytes, record_ids, n, &l)) return -1;
    std::vector<uint64_t> items(record_ids, record_ids + n);
    for (uint64_t& i : items) i /= l.per_item;
    return spiral_gpu_client_queries(c, items.data(), n, form, out, bytes_each);
}

// decode, then packing at w bits and cutting out the record's range -- done per touched output polynomial on the device (client.hip)
int spiral_gpu_client_decode_records(spiral_gpu_client* c, const void* responses, uint32_t n, int form, uint64_t record_bytes, const uint64_t* record_ids,
                                     void* records) {
    if (client_on(c, "client_decode_records")) return -1;
    if (!responses || !record_ids || !records) return fail("client_decode_records: null argument");
    if (form != SPIRAL_GPU_RESPONSE_RAW && form != SPIRAL_GPU_RESPONSE_WIRE) return fail("client_decode_records: unknown response form %d", form);
    spiral_gpu_record_layout l;
    if (client_record_layout(c, "client_decode_records", record_bytes, record_ids, n, &l)) return -1;
    const uint64_t n_resp = (uint64_t)n * l.instances;
    if (n == 0 || n_resp > 65535u) return fail("client_decode_records: %llu responses, a call takes 1 .. 65535", (unsigned long long)n_resp);
    // response k * instances + f holds chunk f of record k: bytes [off, off + len) of its plaintext's stream, staged at the chunk's place in the record
    std::vector<RecordPiece> pieces;
    pieces.reserve(n_resp);
    for (uint32_t k = 0; k < n; k++)
        for (uint32_t f = 0; f < l.instances; f++) {
            RecordChunk ch;
            if (record_chunk(l, record_bytes, f, &ch)) return -1;
            const uint32_t off = l.instances == 1 ? (uint32_t)((record_ids[k] % l.per_item) * record_bytes) : 0u;
            pieces.push_back(RecordPiece{k, k * l.instances + f, 0u, off, (uint32_t)ch.len});
        }
    std::vector<uint4> entries, segs;
    const auto staged_at = [&](uint32_t k) { return (uint64_t)(k / l.instances) * record_bytes + (uint64_t)(k % l.instances) * l.item_bytes; };
    if (c->out_n)  // a SpiralPack item's polynomial t is the response's output polynomial (r, col) = (t / out_n, t % out_n)
        pack_record_tables(pieces, 0, pieces.size(), l.coeff_bits, RecordTrials{c->out_n * c->out_n, 0, c->out_n * c->out_n, 0}, false, entries, segs, staged_at);
    else
        record_tables(pieces, 0, pieces.size(), l.coeff_bits, false, entries, segs, nullptr, staged_at);
    for (uint4& e : entries) {  // {response, r | col << 8, first segment, segments}
        const uint32_t t = c->out_n ? e.y >> kPackRecordTrialShift : (e.x >> kRecordPolyShift) & 3u;
        e = make_uint4(e.x & kRecordRowMask, (t / c->cols) | ((t % c->cols) << 8), e.z, e.w);
    }
    const bool wire = form == SPIRAL_GPU_RESPONSE_WIRE;
    const size_t wire_each = wire_bytes(&c->p, c->cols);  // a multiple of 256 bytes
    const size_t in_words = wire ? wire_each / 8 : (size_t)(c->rows + 1) * c->cols * kN;
    const size_t o_segs = entries.size() * sizeof(uint4), o_buf = o_segs + segs.size() * sizeof(uint4), out_bytes = (size_t)n * record_bytes;
    if (grow(c->in, n_resp * in_words + 1) || grow(c->out, (o_buf + out_bytes + 7) / 8)) return -1;
    uint8_t* d = reinterpret_cast<uint8_t*>(c->out.p);
    HIP_OK(hipMemcpyAsync(c->in.p, responses, n_resp * in_words * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemsetAsync(c->in.p + n_resp * in_words, 0, sizeof(uint64_t), c->stream));  // (the word a wire field's window may reach into)
    HIP_OK(hipMemcpyAsync(d, entries.data(), o_segs, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(d + o_segs, segs.data(), o_buf - o_segs, hipMemcpyHostToDevice, c->stream));
    ClientRecordDecodeParams rp{};
    rp.d.sp = centred_of(c) + kN;
    rp.d.resp = c->in.p;
    rp.d.rows = c->rows;
    rp.d.cols = c->cols;
    rp.d.wire = wire ? 1 : 0;
    rp.d.w0 = c->p.qprime_bits;
    rp.d.w1 = wire_bits_rest(&c->p);
    rp.d.wire_words = wire_each / 8;
    rp.d.qprime = c->qprime;
    rp.d.p_db = c->p.p_db;
    rp.entries = reinterpret_cast<const uint4*>(d);
    rp.segs = reinterpret_cast<const uint4*>(d + o_segs);
    rp.buf = d + o_buf;
    rp.w = l.coeff_bits;
    launch_client_decode_records(rp, (uint32_t)entries.size(), c->stream);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(records, rp.buf, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- keyed records (include/spiral_gpu.h "Keyed records"; kv_host.h): queries for both candidate buckets of each key, and the find on the device -----
// A SpiralPack session (out_n >= 1) takes the same two calls: a bucket is an item of out_n^2 polynomials, the header is in output polynomial (0, 0) and
// the find walks the value's polynomials t as (t / out_n, t % out_n).  The find's byte offsets are 32-bit: 8 slots + slot V < item_bytes <= 16^2 * 256 *
// 40 bytes < 2^22, and the stage of 2 n V bytes is indexed in size_t.
// queries for items b1, b2 of every key, [key][candidate]: both are always made
int spiral_gpu_client_kv_queries(spiral_gpu_client* c, const void* table_key16, const void* keys, uint64_t key_bytes, uint32_t n, int form, void* out, size_t bytes_each) {
    if (client_on(c, "client_kv_queries")) return -1;
    if (!out) return fail("client_kv_queries: null argument");
    if (n == 0 || n > 32767u) return fail("client_kv_queries: %u keys, a call takes 1 .. 32767", n);
    uint64_t nb;
    if (kv_buckets(&c->p, c->out_n, &nb)) return -1;
    std::vector<KvKey> hk;
    if (kv_hash_keys("client_kv_queries", nb, table_key16, keys, key_bytes, n, false, hk)) return -1;
    std::vector<uint64_t> items(2 * (size_t)n);
    for (uint32_t k = 0; k < n; k++) items[2 * k] = hk[k].b[0], items[2 * k + 1] = hk[k].b[1];
    return spiral_gpu_client_queries(c, items.data(), 2 * n, form, out, bytes_each);
}

int spiral_gpu_client_kv_decode(spiral_gpu_client* c, const void* table_key16, const void* keys, uint64_t key_bytes, const void* responses, uint32_t n, int form,
                                uint64_t value_bytes, void* values, uint8_t* found) {
    if (client_on(c, "client_kv_decode")) return -1;
    if (!responses || !values || !found) return fail("client_kv_decode: null argument");
    if (form != SPIRAL_GPU_RESPONSE_RAW && form != SPIRAL_GPU_RESPONSE_WIRE) return fail("client_kv_decode: unknown response form %d", form);
    if (n == 0 || n > 32767u) return fail("client_kv_decode: %u keys (two responses each), a call takes 1 .. 32767", n);
    spiral_gpu_kv_layout l;
    if (kv_layout(&c->p, value_bytes, &l, c->out_n)) return -1;
    std::vector<KvKey> hk;
    if (kv_hash_keys("client_kv_decode", l.buckets, table_key16, keys, key_bytes, n, false, hk)) return -1;
    std::vector<uint64_t> tags(n);
    for (uint32_t k = 0; k < n; k++) tags[k] = hk[k].tag;
    const bool wire = form == SPIRAL_GPU_RESPONSE_WIRE;
    const size_t wire_each = wire_bytes(&c->p, c->cols);  // a multiple of 256 bytes
    const size_t in_words = wire ? wire_each / 8 : (size_t)(c->rows + 1) * c->cols * kN, n_resp = 2 * (size_t)n, V = (size_t)value_bytes;
    // one buffer: [tags][arrival counters][hit flags][staged values, per response] ++ what comes back: [values][found]
    auto up8 = [](size_t b) { return (b + 7) & ~(size_t)7; };
    const size_t o_arr = (size_t)n * 8, o_hit = o_arr + up8((size_t)n * 4), o_stage = o_hit + n_resp * 4, o_val = up8(o_stage + n_resp * V), o_found = o_val + (size_t)n * V;
    const size_t total = o_found + n;
    if (grow(c->in, n_resp * in_words + 1) || grow(c->out, (total + 7) / 8)) return -1;
    uint8_t* d = reinterpret_cast<uint8_t*>(c->out.p);
    HIP_OK(hipMemcpyAsync(c->in.p, responses, n_resp * in_words * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemsetAsync(c->in.p + n_resp * in_words, 0, sizeof(uint64_t), c->stream));  // (the word a wire field's window may reach into)
    HIP_OK(hipMemcpyAsync(d, tags.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemsetAsync(d + o_arr, 0, o_hit - o_arr, c->stream));
    ClientKvFindParams fp{};
    fp.d.sp = centred_of(c) + kN;
    fp.d.resp = c->in.p;
    fp.d.rows = c->rows;
    fp.d.cols = c->cols;
    fp.d.wire = wire ? 1 : 0;
    fp.d.w0 = c->p.qprime_bits;
    fp.d.w1 = wire_bits_rest(&c->p);
    fp.d.wire_words = wire_each / 8;
    fp.d.qprime = c->qprime;
    fp.d.p_db = c->p.p_db;
    fp.tags = reinterpret_cast<const uint64_t*>(d);
    fp.arrive = reinterpret_cast<uint32_t*>(d + o_arr);
    fp.hit = reinterpret_cast<uint32_t*>(d + o_hit);
    fp.stage = d + o_stage;
    fp.values = d + o_val;
    fp.found = d + o_found;
    fp.w = l.coeff_bits;
    fp.slots = l.slots;
    fp.value_bytes = (uint32_t)value_bytes;
    launch_client_kv_find(fp, n, c->stream);
    HIP_OK(hipGetLastError());
    std::vector<uint8_t> back((size_t)n * V + n);
    HIP_OK(hipMemcpyAsync(back.data(), d + o_val, back.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    memcpy(values, back.data(), (size_t)n * V);
    memcpy(found, back.data() + (size_t)n * V, n);
    return 0;
}

int spiral_gpu_client_response_noise(spiral_gpu_client* c, const void* responses, uint32_t n, int form, const uint64_t* expected, uint64_t* stats,
                                     int64_t* errors) {
    if (client_on(c, "client_response_noise")) return -1;
    if (!responses) return fail("client_response_noise: null argument");
    if (!stats && !errors) return fail("client_response_noise: null argument: stats and errors are both null");
    if (form != SPIRAL_GPU_RESPONSE_RAW && form != SPIRAL_GPU_RESPONSE_WIRE && form != SPIRAL_GPU_RESPONSE_FINAL)
        return fail("client_response_noise: unknown response form %d", form);
    if (n == 0 || n > 65535u) return fail("client_response_noise: %u responses, a call takes 1 .. 65535", n);
    // the sum of e^2 below 2^127: |e| <= p D / 2 = 2 p q' in the switched forms
    if ((unsigned __int128)c->qprime * c->p.p_db >= ((unsigned __int128)1 << 57))
        return fail("client_response_noise: q' = %llu with p_db = %llu is outside the exact range of the 128-bit sums", (unsigned long long)c->qprime,
                    (unsigned long long)c->p.p_db);
    const size_t polys = (size_t)n * c->rows * c->cols;
    if (expected)
        for (size_t i = 0; i < polys * kN; i++)
            if (expected[i] >= c->p.p_db) {
                const size_t poly = i / kN;
                return fail("client_response_noise: expected value %llu of response %zu, row %zu, column %zu, coefficient %zu is not below p_db = %llu",
                            (unsigned long long)expected[i], poly / ((size_t)c->rows * c->cols), poly / c->cols % c->rows, poly % c->cols, i % kN,
                            (unsigned long long)c->p.p_db);
            }
    const bool wire = form == SPIRAL_GPU_RESPONSE_WIRE;
    const size_t wire_each = wire_bytes(&c->p, c->cols);  // a multiple of 256 bytes
    const size_t in_words = wire ? wire_each / 8 : (size_t)(c->rows + 1) * c->cols * kN;
    const size_t stats_words = stats ? polys * 6 : 0, err_words = errors ? polys * kN : 0;
    if (grow(c->in, n * in_words + 1) || grow(c->out, stats_words + err_words) || (expected && grow(c->expected, polys * kN))) return -1;
    HIP_OK(hipMemcpyAsync(c->in.p, responses, n * in_words * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemsetAsync(c->in.p + n * in_words, 0, sizeof(uint64_t), c->stream));  // (the word a wire field's window may reach into)
    if (expected) HIP_OK(hipMemcpyAsync(c->expected.p, expected, polys * kPolyBytes, hipMemcpyHostToDevice, c->stream));
    ClientResponseNoiseParams np{};
    np.d.sp = centred_of(c) + kN;
    np.d.resp = c->in.p;
    np.d.rows = c->rows;
    np.d.cols = c->cols;
    np.d.wire = wire ? 1 : 0;
    np.d.w0 = c->p.qprime_bits;
    np.d.w1 = wire_bits_rest(&c->p);
    np.d.wire_words = wire_each / 8;
    np.d.qprime = c->qprime;
    np.d.p_db = c->p.p_db;
    np.expected = expected ? c->expected.p : nullptr;
    np.stats = stats ? c->out.p : nullptr;
    np.errors = errors ? reinterpret_cast<int64_t*>(c->out.p + stats_words) : nullptr;
    np.final_form = form == SPIRAL_GPU_RESPONSE_FINAL ? 1 : 0;
    launch_client_response_noise(np, n, c->stream);
    HIP_OK(hipGetLastError());
    if (stats) HIP_OK(hipMemcpyAsync(stats, c->out.p, stats_words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (errors) HIP_OK(hipMemcpyAsync(errors, c->out.p + stats_words, err_words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
