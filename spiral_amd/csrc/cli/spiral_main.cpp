// ./spiral -- drop-in for the reference executable's command line and text summary (src/spiral.cpp:1228-1346,
// 209-265), with the server-answer path running on an MI355X through libspiral_gpu.so.
//
//   ./spiral <nu1> <nu2> <IDX_TARGET> <dbfile|"a"> [--random-data] [--direct-upload] [--nonoise] [--show-diff] [--seed N] [--batch B] [--instances F]
//            [--wire-input] [--seeded] [--key-store [compact]] [--query-batch] [--device-client [--output-err F]]
//   ./spiral <nu1> <nu2> <RECORD> a --record-bytes S [--device-client]      (a record of S bytes: run_records below)
//   ./spiral <nu1> <nu2> <RECORD> a --high-rate --pack-record-bytes S [--device-client]   (the same on SpiralPack servers: run_pack_records below)
//   ./spiral <nu1> <nu2> <KEY NUMBER> a --kv-value-bytes V --device-client [--high-rate]   (a keyed table of V-byte values: run_kv below)
//
// The reference fixes its scheme parameters at compile time (-DTEXP ... -DOUTN, include/values.h:78-93,
// select_params.py:337); here the same nine values are read at run time from the environment variables or
// flags of the same names (TEXP, TEXPRIGHT, TCONV, TGSW, QPBITS, PVALUE, QNUMFIRST, QNUMREST, OUTN), defaulting
// to the paper's (20, 256) set.  The stdout lines select_params.py scrapes (:386-401) keep their wording.
// --high-rate selects SpiralPack / SpiralStreamPack (testHighRate, src/testing.cpp:777) with OUTN as out_n.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iomanip>
#include <iostream>
#include <random>
#include <string>

#include <hip/hip_runtime_api.h>

#include "client.hpp"

using namespace spiral_cli;
using std::cout;
using std::endl;

static uint64_t now_us() {
    return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static uint64_t param(int argc, char** argv, const char* name, uint64_t dflt) {
    std::string flag = std::string("--") + name;
    for (auto& ch : flag) ch = (char)tolower(ch);
    for (int i = 5; i + 1 < argc; i++)
        if (flag == argv[i]) return strtoull(argv[i + 1], nullptr, 10);
    if (const char* e = getenv(name)) return strtoull(e, nullptr, 10);
    return dflt;
}

#define GPU_OK(x)                                                              \
    do {                                                                       \
        if ((x) != 0) {                                                        \
            fprintf(stderr, "spiral: %s\n", spiral_gpu_last_error());          \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

static size_t bits_to_bytes(size_t bits) { return (size_t)std::llround((double)bits / 8.0); }

// --wire-input: every public parameter and query goes to the server in its wire form (include/spiral_gpu.h): the client takes its NTT-form
// polynomials back to raw form (spiral_gpu_from_ntt) and packs them at 7 bytes per coefficient; the server decodes them on the device
static bool g_wire = false;
static uint64_t g_wire_offline = 0, g_wire_online = 0;  // bytes the first client actually sent
// --seeded (implies --wire-input): the seeded form instead (include/spiral_gpu.h spiral_gpu_query_seeded_bytes): each message is the client's seed
// followed by the wire form of its matrices without their row 0, which the client took from spiral_gpu_seed_expand (client.cpp Row0)
static bool g_seeded = false;
// --device-client: every client of the run is a client session of the library (client.hpp): its keys, its queries and its decoding run on the GPU,
// in the form the other flags choose for the messages
static bool g_device_client = false;
static int client_form() { return !g_device_client ? -1 : g_seeded ? SPIRAL_GPU_FORM_SEEDED : g_wire ? SPIRAL_GPU_FORM_WIRE : SPIRAL_GPU_FORM_NTT; }
// A message is up to four parts, each `count` matrices of [rows][cols] NTT-form polynomials back to back
struct Part {
    const Poly* ntt;
    size_t count;
    uint32_t rows, cols;
};
// the message of `parts`: their wire form (seed null), or the seed and then the wire form of rows 1.. of every matrix
static std::vector<uint8_t> message_of(std::initializer_list<Part> parts, const uint8_t* seed) {
    std::vector<const uint64_t*> sent;  // message order
    for (const Part& g : parts)
        for (size_t i = 0; i < g.count * g.rows * g.cols; i++)
            if (!seed || i % ((size_t)g.rows * g.cols) >= g.cols) sent.push_back(g.ntt->data() + i * 2 * N);
    Poly ntt(sent.size() * 2 * N), raw(sent.size() * N);
    for (size_t i = 0; i < sent.size(); i++) std::copy(sent[i], sent[i] + 2 * N, ntt.begin() + i * 2 * N);
    if (!sent.empty()) GPU_OK(spiral_gpu_from_ntt(raw.data(), ntt.data(), sent.size()));
    const size_t head = seed ? 32 : 0;
    std::vector<uint8_t> w(head + sent.size() * 7 * N);
    if (seed) std::copy(seed, seed + 32, w.begin());
    GPU_OK(spiral_gpu_raw_to_wire(raw.data(), sent.size(), w.data() + head));
    return w;
}
// what a client sends: a query (with the seed its row 0 came from) and its public parameters.  SpiralPack on a direct-upload geometry sends v_W alone
static std::vector<uint8_t> query_msg(const Query& q) {
    if (!q.msg.empty()) return q.msg;  // (--device-client: the session emitted the message)
    return message_of({{&q.cts, q.cts.size() / (4 * N), 2, 1}}, g_seeded ? q.seed.data() : nullptr);
}
static std::vector<uint8_t> pp_msg(const spiral_gpu_params& p, const spiral_gpu_shape& s, const Client& c) {
    if (!c.pp_message.empty()) return c.pp_message;
    return message_of({{&c.w_left, s.n_left, 2, p.t_exp}, {&c.w_right, s.n_right, 2, p.t_exp_right}, {&c.w, 1, 3, 2 * p.t_conv}, {&c.v, 1, 3, 2 * p.t_conv}},
                      g_seeded ? c.pp_seed : nullptr);
}
static std::vector<uint8_t> pack_pp_msg(const spiral_gpu_params& p, const spiral_gpu_pack_shape& s, uint32_t out_n, const PackClient& c) {
    if (!c.pp_message.empty()) return c.pp_message;
    const size_t ex = p.direct_upload ? 0 : 1;
    return message_of({{&c.w_left, ex * s.n_left, 2, p.t_exp}, {&c.w_right, ex * s.n_right, 2, p.t_exp_right}, {&c.v, ex, 2, 2 * p.t_conv},
                       {&c.v_w, out_n, out_n + 1, p.t_conv}},
                      g_seeded ? c.pp_seed : nullptr);
}
static int set_query_msg(spiral_gpu_server* s, const std::vector<uint8_t>& m) {
    return g_seeded ? spiral_gpu_server_set_query_seeded(s, m.data(), m.size()) : spiral_gpu_server_set_query_wire(s, m.data(), m.size());
}
static int set_pp_msg(spiral_gpu_server* s, const std::vector<uint8_t>& m) {
    return g_seeded ? spiral_gpu_server_set_pub_params_seeded(s, m.data(), m.size()) : spiral_gpu_server_set_pub_params_wire(s, m.data(), m.size());
}
static int pack_set_pp_msg(spiral_gpu_pack_server* s, const std::vector<uint8_t>& m) {
    return g_seeded ? spiral_gpu_pack_server_set_pub_params_seeded(s, m.data(), m.size()) : spiral_gpu_pack_server_set_pub_params_wire(s, m.data(), m.size());
}
static void print_wire_bytes() {
    if (g_seeded) {  // (worded apart from the summary's "... query size (b)" lines that drivers scrape)
        cout << "   Seeded public parameters upload (b): " << g_wire_offline << endl;
        cout << "   Seeded query upload (b): " << g_wire_online << endl;
    } else if (g_wire) {
        cout << "   Wire input, uploaded offline / online (b): " << g_wire_offline << " / " << g_wire_online << endl;
    }
}
// --output-err F with --device-client on a one-query run (src/spiral.cpp:1517-1534): the session measures the error the answer carries against the
// true item (include/spiral_gpu.h, spiral_gpu_client_response_noise) -- the variance of the unswitched ciphertext's errors, printed under the
// reference's wording, the bits between the switched response's largest error and its decoding radius, and the unswitched errors appended to F,
// space-separated, as output_diffs writes them.  final_ct: [(rows + 1)][rows][2048] raw values mod Q; wire: the response as received
static std::string g_output_err;
static void report_noise(spiral_gpu_client* c, const uint64_t* final_ct, const std::vector<uint8_t>& wire, const Poly& corr, size_t rows, uint64_t qprime) {
    const size_t polys = rows * rows;
    std::vector<uint64_t> stats(polys * 6);
    std::vector<int64_t> errors(polys * N);
    GPU_OK(spiral_gpu_client_response_noise(c, final_ct, 1, SPIRAL_GPU_RESPONSE_FINAL, corr.data(), stats.data(), errors.data()));
    typedef unsigned __int128 u128;
    u128 sumsq = 0;
    __int128 sum = 0;
    for (size_t i = 0; i < polys; i++) {
        sum += (__int128)(((u128)stats[6 * i + 3] << 64) | stats[6 * i + 2]);
        sumsq += ((u128)stats[6 * i + 5] << 64) | stats[6 * i + 4];
    }
    const long double count = (long double)(polys * N), mean = (long double)sum / count;
    const long double var = (long double)sumsq / count - mean * mean;
    const std::ios::fmtflags flags = cout.flags();
    const std::streamsize prec = cout.precision();
    cout << std::fixed << std::setprecision(4) << "variance of diff w/o modswitching: 2^" << (double)std::log2(var) << endl;
    GPU_OK(spiral_gpu_client_response_noise(c, wire.data(), 1, SPIRAL_GPU_RESPONSE_WIRE, corr.data(), stats.data(), nullptr));
    uint64_t max_abs = 1;
    for (size_t i = 0; i < polys; i++) max_abs = std::max(max_abs, stats[6 * i]);
    const double radius_bits = std::log2(2.0 * (double)qprime);  // step / 2 = 2 q'
    cout << "noise budget: " << radius_bits - std::log2((double)max_abs) << " of " << radius_bits << " bits" << endl;
    cout.flags(flags);
    cout.precision(prec);
    FILE* f = fopen(g_output_err.c_str(), "a");
    if (!f) {
        fprintf(stderr, "spiral: --output-err: cannot open %s\n", g_output_err.c_str());
        exit(1);
    }
    for (int64_t e : errors) fprintf(f, "%lld ", (long long)e);
    fclose(f);
}

// device buffers for the resident entry points the wire path drives (the host-buffer ones take NTT-form queries)
#define HIP_CLI_OK(x)                                                                        \
    do {                                                                                     \
        if ((x) != hipSuccess) {                                                             \
            fprintf(stderr, "spiral: %s failed\n", #x);                                      \
            exit(1);                                                                         \
        }                                                                                    \
    } while (0)

// testHighRate (src/testing.cpp:777-1154): SpiralPack / SpiralStreamPack end to end, summary of :626-733
static int run_high_rate(spiral_gpu_params p, uint32_t out_n, uint64_t idx_target, uint64_t seed, bool nonoise, bool show_diff, uint64_t qnum_first, uint32_t batch,
                         uint32_t instances) {
    cout << "Using n=" << out_n << endl;
    spiral_gpu_pack_shape s;
    GPU_OK(spiral_gpu_pack_get_shape(&p, out_n, &s));
    const uint64_t total_n = (uint64_t)s.dim0 * s.num_per, db_seed = 1234;
    spiral_gpu_pack_server* srv = nullptr;
    GPU_OK(spiral_gpu_pack_server_create(&p, out_n, 0, &srv));
    GPU_OK(spiral_gpu_pack_server_gen_db(srv, db_seed));
    PackClient cl(p, out_n, seed, nonoise);
    cl.seeded = g_seeded;
    cl.form = client_form();
    uint64_t t0 = now_us();
    cl.keygen();
    cl.gen_pub_params();
    const double time_key_gen = (double)(now_us() - t0);
    cout << "query: (" << idx_target / s.num_per << " ";
    for (uint32_t i = 0; i < p.nu2; i++) cout << (((idx_target % s.num_per) >> i) & 1) << " ";
    cout << ")" << endl;
    t0 = now_us();
    const Query query = cl.query(idx_target);
    const double time_query_gen = (double)(now_us() - t0);
    Poly resp((size_t)(out_n + 1) * out_n * N);
    Poly packed(g_output_err.empty() ? 0 : (size_t)(out_n + 1) * out_n * 2 * N);  // (--output-err: the packed ciphertext before the switch, NTT form)
    uint64_t* const packed_out = packed.empty() ? nullptr : packed.data();
    double us[8];
    if (g_wire) {
        const std::vector<uint8_t> pw = pack_pp_msg(p, s, out_n, cl), qw = query_msg(query);
        g_wire_offline = pw.size(), g_wire_online = qw.size();
        GPU_OK(pack_set_pp_msg(srv, pw));
        auto answer = g_seeded ? spiral_gpu_pack_server_answer_seeded : spiral_gpu_pack_server_answer_wire;
        GPU_OK(answer(srv, qw.data(), qw.size(), resp.data(), packed_out, us));  // warm-up
        GPU_OK(answer(srv, qw.data(), qw.size(), resp.data(), packed_out, us));
    } else {
        GPU_OK(spiral_gpu_pack_server_set_pub_params(srv, cl.w_left.data(), cl.w_right.data(), cl.v.data(), cl.v_w.data()));
        GPU_OK(spiral_gpu_pack_server_answer(srv, query.cts.data(), resp.data(), packed_out, us));  // warm-up
        GPU_OK(spiral_gpu_pack_server_answer(srv, query.cts.data(), resp.data(), packed_out, us));
    }
    // the response travels in its wire form (bit-packed on the device, include/spiral_gpu.h); the client unpacks and decodes it
    std::vector<uint8_t> wire(spiral_gpu_response_wire_bytes(&p, out_n));
    GPU_OK(spiral_gpu_pack_server_read_response_wire(srv, wire.data(), wire.size()));
    t0 = now_us();
    GPU_OK(spiral_gpu_response_from_wire(&p, out_n, wire.data(), resp.data()));
    Poly pt = cl.decode(resp.data());
    const double time_decoding = (double)(now_us() - t0);
    Poly corr = pack_db_item(db_seed, idx_target, total_n, out_n, p.p_db);
    // ---- --instances F: the item at idx_target = plaintext idx_target of F databases (instance k seeded db_seed + k; instance 0 is the server above),
    // the one query answered against all of them by ONE call of spiral_gpu_pack_server_answer_batch_instances (expansion and conversion once); every
    // plaintext of the item is decoded from its wire form and checked
    double item_us = 0;
    std::vector<bool> item_ok;
    if (instances >= 2 && instances <= 16) {
        std::vector<spiral_gpu_pack_server*> inst{srv};
        for (uint32_t k = 1; k < instances; k++) {
            spiral_gpu_pack_server* sv = nullptr;
            GPU_OK(spiral_gpu_pack_server_create(&p, out_n, 0, &sv));
            GPU_OK(spiral_gpu_pack_server_gen_db(sv, db_seed + k));
            inst.push_back(sv);
        }
        std::vector<uint8_t> wires((size_t)instances * wire.size());
        const uint64_t* qp[1] = {query.cts.data()};
        for (int it = 0; it < 2; it++)  // a warm-up, the timed call
            GPU_OK(spiral_gpu_pack_server_answer_batch_instances(&srv, 1, inst.data(), instances, qp, nullptr, wires.data(), &item_us));
        Poly r((size_t)(out_n + 1) * out_n * N);
        for (uint32_t k = 0; k < instances; k++) {
            GPU_OK(spiral_gpu_response_from_wire(&p, out_n, wires.data() + (size_t)k * wire.size(), r.data()));
            item_ok.push_back(cl.decode(r.data()) == pack_db_item(db_seed + k, idx_target, total_n, out_n, p.p_db));
        }
        for (uint32_t k = 1; k < instances; k++) spiral_gpu_pack_server_destroy(inst[k]);
    } else if (instances) {
        fprintf(stderr, "spiral: --instances takes 2 .. 16\n");
        spiral_gpu_pack_server_destroy(srv);
        return 1;
    }
    bool item_corr = true;
    for (bool ok : item_ok) item_corr = item_corr && ok;
    const bool is_corr = pt == corr && item_corr;
    cout << "Is correct? : " << (is_corr ? 1 : 0) << endl;
    if (!item_ok.empty()) {
        cout << "Item of " << instances << " plaintexts, Is correct?:";
        for (bool ok : item_ok) cout << " " << (ok ? 1 : 0);
        cout << endl;
    }
    if (show_diff) {
        size_t shown = 0;
        for (size_t i = 0; i < pt.size() && shown < 10; i++)
            if (pt[i] != corr[i]) {
                cout << i << ": " << pt[i] << " " << corr[i] << endl;
                shown++;
            }
    }
    if (!g_output_err.empty()) {
        Poly final_ct((size_t)(out_n + 1) * out_n * N);
        GPU_OK(spiral_gpu_from_ntt(final_ct.data(), packed.data(), (size_t)(out_n + 1) * out_n));
        report_noise(cl.session.get(), final_ct.data(), wire, corr, out_n, s.qprime);
    }
    // print_summary_testing (src/testing.cpp:626-733)
    const size_t logp = (size_t)std::ceil(std::log2((double)p.p_db));
    size_t total_query_size_b = bits_to_bytes((size_t)(((1ull << p.nu1) + 2ull * p.nu2 * p.t_gsw) * N * 56));
    if (qnum_first == 1) total_query_size_b = bits_to_bytes((size_t)N * 56);
    const size_t total_resp_size_b = bits_to_bytes((size_t)out_n * out_n * N * (logp + 2) + (size_t)out_n * N * p.qprime_bits);
    const size_t item_size_b = bits_to_bytes((size_t)out_n * out_n * N * logp);
    const double t_exp = us[0], t_conv = us[1], t_fdim = us[2], t_fold = us[3], t_pack = us[4];
    const double total_time = t_fdim + t_fold + t_pack + t_exp + t_conv;
    cout << "ScalToMat took (CPU·us): 0" << endl;
    cout << "RegevToGSW took (CPU·us): 0" << endl;
    cout << "Expansion took (CPU·us): 0" << endl;
    cout << std::fixed << std::setprecision(0);
    cout << "Database" << endl << endl;
    cout << "                       Number of items: " << total_n << endl;
    cout << "                             Item size: " << item_size_b << endl;
    cout << "Communication" << endl << endl;
    cout << "         Total offline query size (b): " << cl.offline_bytes << endl;
    cout << "          Total online query size (b): " << total_query_size_b << endl;
    cout << "                    Response size (b): " << total_resp_size_b << endl;
    cout << std::fixed << std::setprecision(4);
    cout << "                                Rate : " << ((double)item_size_b / (double)total_resp_size_b) << endl;
    cout << std::fixed << std::setprecision(0);
    cout << endl << endl;
    cout << "Database-independent computation" << endl << endl;
    cout << "              Main expansion  (CPU·us): " << t_exp << endl;
    cout << "                   Conversion (CPU·us): " << t_conv << endl;
    cout << "                        Total (CPU·us): " << (t_exp + t_conv) << endl << endl;
    cout << "Database-dependent computation" << endl << endl;
    cout << "     First dimension multiply (CPU·us): " << t_fdim << endl;
    cout << "                      Folding (CPU·us): " << t_fold << endl;
    cout << "                      Packing (CPU·us): " << t_pack << endl;
    cout << "                        Total (CPU·us): " << (t_fdim + t_fold + t_pack) << endl;
    cout << "                   Throughput (MB / s): " << ((double)total_n * item_size_b / total_time) << endl << endl;
    cout << "Client computation" << endl << endl;
    cout << "               Key generation (CPU·us): " << time_key_gen << endl;
    cout << "             Query generation (CPU·us): " << time_query_gen << endl;
    cout << "                     Decoding (CPU·us): " << time_decoding << endl << endl;
    cout << "GPU extras" << endl << endl;
    cout << "      Sweep kernels alone (GPU·us): " << us[5] << "  (" << (double)out_n * out_n * spiral_gpu_pack_server_sweep_bytes(srv) / us[5] / 1e3 << " GB/s)" << endl;
    cout << "      Whole answer, device (GPU·us): " << us[6] << endl;
    if (item_us > 0) cout << "   Item of " << instances << " plaintexts (one query, " << instances << " database instances), device (GPU·us): " << item_us << endl;
    // ---- --batch B: B more clients (own keys, own indices) answered by ONE spiral_gpu_pack_server_answer_batch call: the server and B - 1 lanes
    // (create_lane), one first-dimension pass over the trial images for all of them
    bool batch_corr = true;
    if (batch >= 2 && batch <= 8) {
        std::vector<spiral_gpu_pack_server*> lanes{srv};
        std::vector<PackClient> clients;
        std::vector<Query> queries;
        std::vector<Poly> resps(batch, Poly((size_t)(out_n + 1) * out_n * N));
        std::vector<uint64_t> idxs;
        clients.reserve(batch);
        for (uint32_t b = 0; b < batch; b++) {
            if (b) {
                spiral_gpu_pack_server* lane = nullptr;
                GPU_OK(spiral_gpu_pack_server_create_lane(srv, &lane));
                lanes.push_back(lane);
            }
            clients.emplace_back(p, out_n, seed + 1 + b, nonoise);
            clients[b].seeded = g_seeded;
            clients[b].form = client_form();
            clients[b].keygen();
            clients[b].gen_pub_params();
            idxs.push_back((idx_target + 1 + 7919ull * b) % total_n);
            if (g_wire) {
                GPU_OK(pack_set_pp_msg(lanes[b], pack_pp_msg(p, s, out_n, clients[b])));
            } else {
                GPU_OK(spiral_gpu_pack_server_set_pub_params(lanes[b], clients[b].w_left.data(), clients[b].w_right.data(), clients[b].v.data(), clients[b].v_w.data()));
            }
            queries.push_back(clients[b].query(idxs[b]));
        }
        std::vector<const uint64_t*> qp;
        std::vector<uint64_t*> rp;
        std::vector<std::vector<uint8_t>> qws;
        std::vector<const void*> qwp;
        for (uint32_t b = 0; b < batch; b++) qp.push_back(queries[b].cts.data()), rp.push_back(resps[b].data());
        if (g_wire)
            for (uint32_t b = 0; b < batch; b++) qws.push_back(query_msg(queries[b]));
        for (uint32_t b = 0; b < qws.size(); b++) qwp.push_back(qws[b].data());
        auto run = [&](uint64_t* const* r, double* u) {
            if (g_seeded) GPU_OK(spiral_gpu_pack_server_answer_batch_seeded(lanes.data(), batch, qwp.data(), qws[0].size(), r, nullptr, u));
            else if (g_wire) GPU_OK(spiral_gpu_pack_server_answer_batch_wire(lanes.data(), batch, qwp.data(), qws[0].size(), r, nullptr, u));
            else GPU_OK(spiral_gpu_pack_server_answer_batch(lanes.data(), batch, qp.data(), r, nullptr, u));
        };
        double bus[8];
        run(nullptr, bus);  // warm-up (converts the image where it can)
        t0 = now_us();
        run(rp.data(), bus);
        const double batch_us = (double)(now_us() - t0);
        cout << "Batch of " << batch << " queries, Is correct?:";
        for (uint32_t b = 0; b < batch; b++) {
            GPU_OK(spiral_gpu_pack_server_read_response_wire(lanes[b], wire.data(), wire.size()));
            GPU_OK(spiral_gpu_response_from_wire(&p, out_n, wire.data(), resps[b].data()));
            const bool ok = clients[b].decode(resps[b].data()) == pack_db_item(db_seed, idxs[b], total_n, out_n, p.p_db);
            batch_corr = batch_corr && ok;
            cout << " " << (ok ? 1 : 0);
        }
        cout << endl;
        cout << "   Batch of " << batch << " queries, wall (GPU·us): " << batch_us << "  (shared sweep " << bus[2] << ")" << endl;
        for (uint32_t b = 1; b < batch; b++) spiral_gpu_pack_server_destroy(lanes[b]);
    } else if (batch) {
        fprintf(stderr, "spiral: --batch takes 2 .. 8\n");
        spiral_gpu_pack_server_destroy(srv);
        return 1;
    }
    print_wire_bytes();
    spiral_gpu_pack_server_destroy(srv);
    return (is_corr && batch_corr) ? 0 : 2;
}

// ---- --record-bytes S: the third argument is a RECORD id (include/spiral_gpu.h "Records") ------------------------------------------------------------
// The database is filled through load_records -- one server per instance of the layout -- from a counter-based byte generator:
//     byte i of record r in generation g  =  the low byte of splitmix64((0x5245434F52445300 + g) ^ (r * S + i))
// (splitmix64 as spiral_gpu_server_gen_db's generator uses it; generation 0 is the loaded database, generation 1 what the update writes).  One query
// for the record's item is answered -- answer_instances when the layout has several instances, the one-query flow otherwise -- and decoded: with
// --device-client by decode_records on the session, with the host client by packing the decoded plaintexts at w bits and cutting on the host.  The
// record is then replaced through update_records, answered again and decoded again; both results are checked against the generator.
static uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
static void record_bytes_of(uint32_t generation, uint64_t r, uint64_t S, uint8_t* out) {
    for (uint64_t i = 0; i < S; i++) out[i] = (uint8_t)splitmix64((0x5245434F52445300ull + generation) ^ (r * S + i));
}
static int run_records(const spiral_gpu_params& p, uint64_t record, uint64_t S, uint64_t seed, bool nonoise) {
    spiral_gpu_record_layout lay;
    GPU_OK(spiral_gpu_record_layout_of(&p, S, &lay));
    if (record >= lay.capacity) {
        fprintf(stderr, "spiral: record %llu out of range (%llu records of %llu bytes)\n", (unsigned long long)record, (unsigned long long)lay.capacity, (unsigned long long)S);
        return 1;
    }
    spiral_gpu_shape s;
    GPU_OK(spiral_gpu_get_shape(&p, &s));
    cout << "Records of " << S << " bytes: " << lay.per_item << " per item of " << lay.item_bytes << " bytes, " << lay.instances << " instance(s), capacity "
         << lay.capacity << endl;
    const uint32_t F = lay.instances;
    std::vector<spiral_gpu_server*> inst(F, nullptr);
    cout << "starting generation of db" << endl;
    const uint64_t pass = lay.per_item * 1024;  // records generated and loaded at a time
    std::vector<uint8_t> buf;
    for (uint32_t f = 0; f < F; f++) GPU_OK(spiral_gpu_server_create(&p, 0, 0, 0, &inst[f]));
    for (uint64_t first = 0; first < lay.capacity; first += pass) {
        const uint64_t n = std::min(pass, lay.capacity - first);
        buf.resize((size_t)(n * S));
        for (uint64_t k = 0; k < n; k++) record_bytes_of(0, first + k, S, buf.data() + k * S);
        for (uint32_t f = 0; f < F; f++) GPU_OK(spiral_gpu_server_load_records(inst[f], buf.data(), S, f, first, n));
    }
    cout << "done loading/generating db." << endl;
    Client cl(p, seed, nonoise);
    cl.form = g_device_client ? SPIRAL_GPU_FORM_NTT : -1;
    cl.keygen();
    cl.gen_pub_params();
    GPU_OK(spiral_gpu_server_set_pub_params(inst[0], cl.w_left.data(), cl.w_right.data(), cl.w.data(), cl.v.data()));
    const uint64_t item = record / lay.per_item;
    Poly final_ct(6 * N), resps((size_t)F * 6 * N);
    std::vector<uint8_t> got((size_t)S), want((size_t)S);
    bool all_ok = true;
    for (uint32_t generation = 0; generation < 2; generation++) {
        if (generation) {  // replace the record in place, in every instance
            record_bytes_of(1, record, S, want.data());
            for (uint32_t f = 0; f < F; f++) GPU_OK(spiral_gpu_server_update_records(inst[f], want.data(), S, f, &record, 1));
        }
        Query query = cl.query(item);
        if (g_device_client)  // the same through the record call: one query per record, serving every instance
            GPU_OK(spiral_gpu_client_record_queries(cl.session.get(), S, &record, 1, SPIRAL_GPU_FORM_NTT, query.cts.data(), query.cts.size() * sizeof(uint64_t)));
        cout << "Beginning query processing..." << endl;
        double us[8], item_us = 0;
        if (F > 1)
            GPU_OK(spiral_gpu_server_answer_instances(inst[0], inst.data(), F, query.cts.data(), resps.data(), nullptr, &item_us));
        else
            GPU_OK(spiral_gpu_server_answer(inst[0], query.cts.data(), final_ct.data(), resps.data(), us));
        cout << "Done with query processing!" << endl;
        if (g_device_client) {
            GPU_OK(spiral_gpu_client_decode_records(cl.session.get(), resps.data(), 1, SPIRAL_GPU_RESPONSE_RAW, S, &record, got.data()));
        } else {  // the plaintexts packed at w bits -- coefficient k of polynomial (m, c) at bit ((m * 2 + c) * N + k) * w -- and the record's range cut out
            const uint32_t w = lay.coeff_bits;
            for (uint32_t f = 0; f < F; f++) {
                const Poly pt = cl.decode(resps.data() + (size_t)f * 6 * N);
                const uint64_t off = F == 1 ? (record % lay.per_item) * S : 0, first = (uint64_t)f * lay.item_bytes;
                const uint64_t len = F == 1 ? S : std::min<uint64_t>(S - first, lay.item_bytes);
                for (uint64_t i = 0; i < len; i++) {
                    uint32_t byte = 0;
                    for (uint32_t b = 0; b < 8; b++) {
                        const uint64_t bit = 8 * (off + i) + b;
                        byte |= (uint32_t)((pt[bit / w] >> (bit % w)) & 1u) << b;
                    }
                    got[(F == 1 ? 0 : first) + i] = (uint8_t)byte;
                }
            }
        }
        record_bytes_of(generation, record, S, want.data());
        const bool ok = got == want;
        all_ok = all_ok && ok;
        cout << "Record " << record << (generation ? " after update_records" : " as loaded") << ", correct: " << (ok ? 1 : 0) << endl;
    }
    cout << "Is correct?: " << (all_ok ? 1 : 0) << endl;
    for (spiral_gpu_server* sv : inst) spiral_gpu_server_destroy(sv);
    return all_ok ? 0 : 2;
}

// ---- --high-rate --pack-record-bytes S: the records run on SpiralPack servers (include/spiral_gpu.h "Records", SpiralPack) -------------------------
// run_records' steps and lines with out_n from OUTN: load_records per instance from the same generator, one query for the record's item -- answered by
// answer_batch_instances when the layout has several instances -- decoded by decode_records (--device-client) or by packing the decoded item's
// out_n^2 polynomials at w bits in trial order and cutting on the host; then update_records, and the same again.
static int run_pack_records(const spiral_gpu_params& p, uint32_t out_n, uint64_t record, uint64_t S, uint64_t seed, bool nonoise) {
    cout << "Using n=" << out_n << endl;
    spiral_gpu_record_layout lay;
    GPU_OK(spiral_gpu_pack_record_layout_of(&p, out_n, S, &lay));
    if (record >= lay.capacity) {
        fprintf(stderr, "spiral: record %llu out of range (%llu records of %llu bytes)\n", (unsigned long long)record, (unsigned long long)lay.capacity, (unsigned long long)S);
        return 1;
    }
    cout << "Records of " << S << " bytes: " << lay.per_item << " per item of " << lay.item_bytes << " bytes, " << lay.instances << " instance(s), capacity "
         << lay.capacity << endl;
    const uint32_t F = lay.instances;
    std::vector<spiral_gpu_pack_server*> inst(F, nullptr);
    cout << "starting generation of db" << endl;
    const uint64_t pass = lay.per_item * 256;  // records generated and loaded at a time
    std::vector<uint8_t> buf;
    for (uint32_t f = 0; f < F; f++) GPU_OK(spiral_gpu_pack_server_create(&p, out_n, 0, &inst[f]));
    for (uint64_t first = 0; first < lay.capacity; first += pass) {
        const uint64_t n = std::min(pass, lay.capacity - first);
        buf.resize((size_t)(n * S));
        for (uint64_t k = 0; k < n; k++) record_bytes_of(0, first + k, S, buf.data() + k * S);
        for (uint32_t f = 0; f < F; f++) GPU_OK(spiral_gpu_pack_server_load_records(inst[f], buf.data(), S, f, first, n));
    }
    cout << "done loading/generating db." << endl;
    PackClient cl(p, out_n, seed, nonoise);
    cl.form = g_device_client ? SPIRAL_GPU_FORM_NTT : -1;
    cl.keygen();
    cl.gen_pub_params();
    GPU_OK(spiral_gpu_pack_server_set_pub_params(inst[0], cl.w_left.data(), cl.w_right.data(), cl.v.data(), cl.v_w.data()));
    const uint64_t item = record / lay.per_item;
    const size_t resp_words = (size_t)(out_n + 1) * out_n * N;
    Poly resps((size_t)F * resp_words);
    std::vector<uint8_t> got((size_t)S), want((size_t)S);
    bool all_ok = true;
    for (uint32_t generation = 0; generation < 2; generation++) {
        if (generation) {  // replace the record in place, in every instance
            record_bytes_of(1, record, S, want.data());
            for (uint32_t f = 0; f < F; f++) GPU_OK(spiral_gpu_pack_server_update_records(inst[f], want.data(), S, f, &record, 1));
        }
        Query query = cl.query(item);
        if (g_device_client)  // the same through the record call: one query per record, serving every instance
            GPU_OK(spiral_gpu_client_record_queries(cl.session.get(), S, &record, 1, SPIRAL_GPU_FORM_NTT, query.cts.data(), query.cts.size() * sizeof(uint64_t)));
        cout << "Beginning query processing..." << endl;
        double us[8], item_us = 0;
        if (F > 1) {
            const uint64_t* qp[1] = {query.cts.data()};
            GPU_OK(spiral_gpu_pack_server_answer_batch_instances(&inst[0], 1, inst.data(), F, qp, resps.data(), nullptr, &item_us));
        } else {
            GPU_OK(spiral_gpu_pack_server_answer(inst[0], query.cts.data(), resps.data(), nullptr, us));
        }
        cout << "Done with query processing!" << endl;
        if (g_device_client) {
            GPU_OK(spiral_gpu_client_decode_records(cl.session.get(), resps.data(), 1, SPIRAL_GPU_RESPONSE_RAW, S, &record, got.data()));
        } else {  // the item's polynomials packed at w bits in trial order -- coefficient k of output polynomial (r, col) at bit ((r * out_n + col) * N + k) * w
            const uint32_t w = lay.coeff_bits;
            for (uint32_t f = 0; f < F; f++) {
                const Poly pt = cl.decode(resps.data() + (size_t)f * resp_words);
                const uint64_t off = F == 1 ? (record % lay.per_item) * S : 0, first = (uint64_t)f * lay.item_bytes;
                const uint64_t len = F == 1 ? S : std::min<uint64_t>(S - first, lay.item_bytes);
                for (uint64_t i = 0; i < len; i++) {
                    uint32_t byte = 0;
                    for (uint32_t b = 0; b < 8; b++) {
                        const uint64_t bit = 8 * (off + i) + b;
                        byte |= (uint32_t)((pt[bit / w] >> (bit % w)) & 1u) << b;
                    }
                    got[(F == 1 ? 0 : first) + i] = (uint8_t)byte;
                }
            }
        }
        record_bytes_of(generation, record, S, want.data());
        const bool ok = got == want;
        all_ok = all_ok && ok;
        cout << "Record " << record << (generation ? " after update_records" : " as loaded") << ", correct: " << (ok ? 1 : 0) << endl;
    }
    cout << "Is correct?: " << (all_ok ? 1 : 0) << endl;
    for (spiral_gpu_pack_server* sv : inst) spiral_gpu_pack_server_destroy(sv);
    return all_ok ? 0 : 2;
}

// ---- --kv-value-bytes V --device-client [--high-rate]: the third argument is a KEY number (include/spiral_gpu.h "Keyed records") ---------------------
// Keys are "key-%08d", the table key is the bytes 00 .. 0f, and the value of key k in generation g is record_bytes_of(g, k, V) -- the record runs'
// generator.  One run: kv_load of keys 0 .. n - 1 with n = half of the capacity -- or, where the placement rule refuses that many (buckets of two or
// three slots overflow early), the longest prefix it accepts, found by bisection over kv_load calls, which fail before they touch the image --; key
// number K is looked up privately (kv_queries, two answers, kv_decode) and compared with the generator, or, for K >= n, must not be found; it is
// written by kv_put in generation 1 and looked up again; one key that was never stored is looked up; kv_stats reports the table's load.  On a base
// server, or with --high-rate on a SpiralPack server with OUTN as out_n.
// --kv-scan: after those steps the whole table is listed with values (kv_scan: a count-only call, then the entries), reconciled against every key the
// run stored -- the key written by kv_put included -- and every held value is compared with the generator.
static int run_kv(const spiral_gpu_params& p, uint32_t out_n, uint64_t key_no, uint64_t V, uint64_t seed, bool nonoise, bool scan) {
    if (out_n) cout << "Using n=" << out_n << endl;
    spiral_gpu_kv_layout lay;
    GPU_OK(out_n ? spiral_gpu_pack_kv_layout_of(&p, out_n, V, &lay) : spiral_gpu_kv_layout_of(&p, V, &lay));
    if (key_no >= 50000000ull) {
        fprintf(stderr, "spiral: key number %llu out of range (below 50000000: keys are \"key-%%08d\")\n", (unsigned long long)key_no);
        return 1;
    }
    cout << "Keyed records of " << V << "-byte values: " << lay.slots << " slots per bucket of " << lay.item_bytes << " bytes, " << lay.buckets << " buckets, capacity "
         << lay.capacity << endl;
    uint8_t tk[16];
    for (int b = 0; b < 16; b++) tk[b] = (uint8_t)b;
    constexpr uint64_t KB = 12;  // bytes of a key
    auto key_of = [](uint64_t k, uint8_t* out) {
        char text[32];
        snprintf(text, sizeof(text), "key-%08llu", (unsigned long long)k);
        memcpy(out, text, KB);
    };
    spiral_gpu_server* base = nullptr;
    spiral_gpu_pack_server* pack = nullptr;
    if (out_n)
        GPU_OK(spiral_gpu_pack_server_create(&p, out_n, 0, &pack));
    else
        GPU_OK(spiral_gpu_server_create(&p, 0, 0, 0, &base));
    cout << "starting generation of db" << endl;
    const uint64_t half = lay.capacity / 2;
    std::vector<uint8_t> keys((size_t)(half * KB)), vals((size_t)(half * V));
    for (uint64_t k = 0; k < half; k++) key_of(k, keys.data() + k * KB), record_bytes_of(0, k, V, vals.data() + k * V);
    auto load = [&](uint64_t n) { return out_n ? spiral_gpu_pack_server_kv_load(pack, tk, keys.data(), KB, vals.data(), V, n) : spiral_gpu_server_kv_load(base, tk, keys.data(), KB, vals.data(), V, n); };
    uint64_t n_loaded = half;
    if (load(half)) {  // the longest prefix the placement rule accepts: [lo places, hi does not)
        uint64_t lo = 0, hi = half;
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            (load(mid) ? hi : lo) = mid;
        }
        n_loaded = lo;
        GPU_OK(load(n_loaded));
    }
    cout << "done loading/generating db: " << n_loaded << " keys (half of the capacity: " << half << ")" << endl;
    // a session for either kind of client; the servers take its public parameters in the NTT form
    std::shared_ptr<spiral_gpu_client> session;
    size_t query_words;
    if (out_n) {
        PackClient cl(p, out_n, seed, nonoise);
        cl.form = SPIRAL_GPU_FORM_NTT;
        cl.keygen();
        cl.gen_pub_params();
        GPU_OK(spiral_gpu_pack_server_set_pub_params(pack, cl.w_left.data(), cl.w_right.data(), cl.v.data(), cl.v_w.data()));
        session = cl.session;
        query_words = cl.query(0).cts.size();
    } else {
        Client cl(p, seed, nonoise);
        cl.form = SPIRAL_GPU_FORM_NTT;
        cl.keygen();
        cl.gen_pub_params();
        GPU_OK(spiral_gpu_server_set_pub_params(base, cl.w_left.data(), cl.w_right.data(), cl.w.data(), cl.v.data()));
        session = cl.session;
        query_words = cl.query(0).cts.size();
    }
    const size_t resp_words = out_n ? (size_t)(out_n + 1) * out_n * N : 6 * N;
    Poly queries(2 * query_words), resps(2 * resp_words), final_ct(6 * N);
    std::vector<uint8_t> got((size_t)V), want((size_t)V);
    // one private lookup: both candidates' queries, two answers, the find on the device
    auto lookup = [&](const uint8_t* key, uint8_t* found) -> int {
        GPU_OK(spiral_gpu_client_kv_queries(session.get(), tk, key, KB, 1, SPIRAL_GPU_FORM_NTT, queries.data(), query_words * sizeof(uint64_t)));
        cout << "Beginning query processing..." << endl;
        double us[8];
        for (int c = 0; c < 2; c++) {
            if (out_n)
                GPU_OK(spiral_gpu_pack_server_answer(pack, queries.data() + c * query_words, resps.data() + c * resp_words, nullptr, us));
            else
                GPU_OK(spiral_gpu_server_answer(base, queries.data() + c * query_words, final_ct.data(), resps.data() + c * resp_words, us));
        }
        cout << "Done with query processing!" << endl;
        GPU_OK(spiral_gpu_client_kv_decode(session.get(), tk, key, KB, resps.data(), 1, SPIRAL_GPU_RESPONSE_RAW, V, got.data(), found));
        return 0;
    };
    uint8_t key[KB], found = 0;
    key_of(key_no, key);
    const std::string name((const char*)key, KB);
    bool all_ok = true;
    for (uint32_t generation = 0; generation < 2; generation++) {
        if (generation) {  // insert or overwrite, in place
            record_bytes_of(1, key_no, V, want.data());
            GPU_OK(out_n ? spiral_gpu_pack_server_kv_put(pack, tk, key, KB, want.data(), V, 1) : spiral_gpu_server_kv_put(base, tk, key, KB, want.data(), V, 1));
        }
        if (lookup(key, &found)) return 1;
        const bool stored = generation || key_no < n_loaded;
        record_bytes_of(generation, key_no, V, want.data());
        if (!stored) std::fill(want.begin(), want.end(), (uint8_t)0);  // (an absent key's value bytes are zero)
        const bool ok = (found != 0) == stored && got == want;
        all_ok = all_ok && ok;
        cout << "Key " << name << (generation ? " after kv_put" : " as loaded") << ", found: " << (int)found << ", correct: " << (ok ? 1 : 0) << endl;
    }
    key_of(50000000ull + key_no, key);  // (never loaded, never put)
    if (lookup(key, &found)) return 1;
    all_ok = all_ok && found == 0;
    cout << "Absent key, found: " << (int)found << endl;
    spiral_gpu_kv_stats st;
    GPU_OK(out_n ? spiral_gpu_pack_server_kv_stats(pack, V, 0, lay.buckets, &st) : spiral_gpu_server_kv_stats(base, V, 0, lay.buckets, &st));
    const uint64_t stored_now = n_loaded + (key_no < n_loaded ? 0 : 1);
    all_ok = all_ok && st.used == stored_now;
    cout << "Table load (kv_stats): " << st.used << " of " << lay.capacity << " slots used, load " << (double)st.used / (double)lay.capacity << ", fullest bucket "
         << st.max_used << " of " << st.slots << ", full buckets " << st.full_buckets << endl;
    if (scan) {
        auto list = [&](spiral_gpu_kv_entry* entries, void* values, uint64_t max_entries, uint64_t* n) {
            return out_n ? spiral_gpu_pack_server_kv_scan(pack, V, 0, lay.buckets, entries, values, max_entries, n)
                         : spiral_gpu_server_kv_scan(base, V, 0, lay.buckets, entries, values, max_entries, n);
        };
        uint64_t count = 0, listed = 0;
        GPU_OK(list(nullptr, nullptr, 0, &count));
        std::vector<spiral_gpu_kv_entry> entries((size_t)count);
        std::vector<uint8_t> listed_vals((size_t)(count * V));
        if (count) GPU_OK(list(entries.data(), listed_vals.data(), count, &listed));
        // the keys the run stored: 0 .. n_loaded - 1, and key K where the put added it (its value is generation 1's either way)
        const bool put_is_new = key_no >= n_loaded;
        const uint64_t n_keys = n_loaded + (put_is_new ? 1 : 0);
        std::vector<uint8_t> all_keys((size_t)(n_keys * KB));
        memcpy(all_keys.data(), keys.data(), (size_t)(n_loaded * KB));
        if (put_is_new) key_of(key_no, all_keys.data() + n_loaded * KB);
        std::vector<int64_t> where((size_t)n_keys);
        std::vector<uint8_t> entry_class((size_t)count);
        spiral_gpu_kv_reconcile_counts rc{};
        GPU_OK(spiral_gpu_kv_reconcile(&p, tk, all_keys.data(), KB, n_keys, entries.data(), listed, where.data(), entry_class.data(), &rc));
        bool values_ok = listed == count && count == st.used;
        for (uint64_t k = 0; k < n_keys && values_ok; k++) {
            if (where[k] < 0) continue;
            const uint64_t number = k < n_loaded ? k : key_no;
            record_bytes_of(number == key_no ? 1 : 0, number, V, want.data());
            values_ok = !memcmp(want.data(), listed_vals.data() + (size_t)where[k] * V, (size_t)V);
        }
        all_ok = all_ok && values_ok && rc.missing == 0 && rc.orphans == 0 && rc.shadowed == 0 && rc.misplaced == 0 && rc.held == n_keys;
        cout << "Scan: " << listed << " entries, missing: " << rc.missing << ", orphans: " << rc.orphans << ", values correct: " << (values_ok ? 1 : 0) << endl;
    }
    cout << "Is correct?: " << (all_ok ? 1 : 0) << endl;
    if (pack) spiral_gpu_pack_server_destroy(pack);
    if (base) spiral_gpu_server_destroy(base);
    return all_ok ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s <nu1> <nu2> <IDX_TARGET> [dbfile|a] [--random-data] [--direct-upload] [--nonoise] [--show-diff] [--output-err F] [--seed N]\n", argv[0]);
        return 1;
    }
    const uint32_t nu1 = (uint32_t)strtol(argv[1], nullptr, 10), nu2 = (uint32_t)strtol(argv[2], nullptr, 10);
    const uint64_t total_n = (1ull << nu1) * (1ull << nu2);
    const uint64_t idx_target = strtoull(argv[3], nullptr, 10);
    bool nonoise = false, random_data = false, show_diff = false, direct_flag = false, high_rate = false;
    uint32_t batch = 0, instances = 0;
    int key_store = -1;  // --key-store: the slot form of the store the batch's keys are bound from (-1: none)
    bool query_batch = false;  // --query-batch: the batch's queries in one set_query_batch call, its responses in one read
    uint64_t record_bytes = 0;  // --record-bytes S: IDX_TARGET is a record id (run_records above)
    bool record_run = false;
    uint64_t pack_record_bytes = 0;  // --high-rate --pack-record-bytes S: the same on SpiralPack servers (run_pack_records above)
    bool pack_record_run = false;
    uint64_t kv_value_bytes = 0;  // --kv-value-bytes V --device-client [--high-rate]: IDX_TARGET is a key number (run_kv above)
    bool kv_run = false, kv_scan = false;  // --kv-scan: list and reconcile the table at the end of the keyed run
    // as the reference (random_device, src/core.cpp:202; it labels its own generator NOT SECURE): two words of it.
    // This client is a test harness for the server path, not a hardened client.
    std::random_device rd;
    uint64_t seed = ((uint64_t)rd() << 32) ^ (uint64_t)rd();
    for (int i = 5; i < argc; i++) {  // flags are only parsed after the db filename (src/spiral.cpp:1250-1303)
        if (!strcmp(argv[i], "--nonoise")) { cout << "Using no noise" << endl; nonoise = true; }
        if (!strcmp(argv[i], "--high-rate")) { cout << "Using high rate variant..." << endl; high_rate = true; }
        if (!strcmp(argv[i], "--random-data")) { cout << "Using random data..." << endl; random_data = true; }
        if (!strcmp(argv[i], "--show-diff")) { cout << "Showing diff..." << endl; show_diff = true; }
        if (!strcmp(argv[i], "--direct-upload")) { cout << "Direct uploading of query (no compression)" << endl; direct_flag = true; }
        if (!strcmp(argv[i], "--seed") && i + 1 < argc) seed = strtoull(argv[++i], nullptr, 10);
        // --batch B (2 .. 8; not a flag of the reference, which answers one query per process): after the reference's own single-query run, B clients --
        // own keys, own indices -- are answered by ONE call of spiral_gpu_server_run_query_batch and each is decoded and checked
        if (!strcmp(argv[i], "--batch") && i + 1 < argc) batch = (uint32_t)strtoul(argv[++i], nullptr, 10);
        // --instances F (2 .. 16; not a flag of the reference either: select_params.py:297-298 runs ONE instance and multiplies by factor = ceil(item size /
        // plaintext size)): an item of F plaintexts = F instances of the database; the one query is converted once and answered against all of them by ONE
        // call of spiral_gpu_server_answer_instances, every plaintext of the item is decoded and checked
        if (!strcmp(argv[i], "--instances") && i + 1 < argc) instances = (uint32_t)strtoul(argv[++i], nullptr, 10);
        // --wire-input (not a flag of the reference): public parameters and queries reach the server in their 7-byte wire form (include/spiral_gpu.h)
        if (!strcmp(argv[i], "--wire-input")) { cout << "Sending public parameters and queries in their wire form" << endl; g_wire = true; }
        // --seeded (implies --wire-input): the same with every matrix's random row 0 replaced by a seed the client draws from its own generator
        if (!strcmp(argv[i], "--seeded")) { cout << "Sending public parameters and queries in their seeded form" << endl; g_wire = g_seeded = true; }
        // --batch B --key-store [compact] (not a flag of the reference): the B clients' keys go into a key store (include/spiral_gpu.h) and the batch is
        // answered twice more with the lanes' keys bound from it, the slot assignment rotated by one lane in between; every client is decoded and
        // checked in both rounds.  compact: the store keeps each message's seed and rows 1.. only, so the keys travel in the seeded form (implies --seeded)
        if (!strcmp(argv[i], "--key-store")) {
            key_store = SPIRAL_GPU_KEYS_FULL;
            if (i + 1 < argc && !strcmp(argv[i + 1], "compact")) key_store = SPIRAL_GPU_KEYS_COMPACT, g_wire = g_seeded = true, i++;
            cout << "Binding the batch's keys from a key store (" << (key_store == SPIRAL_GPU_KEYS_COMPACT ? "compact" : "full") << " slots)" << endl;
        }
        // --batch B --query-batch (not a flag of the reference): after the batch, every client draws a fresh query; all of them go in through ONE
        // spiral_gpu_server_set_query_batch call -- in the wire form, or with --seeded in the seeded form -- and all responses come back through ONE
        // spiral_gpu_server_read_response_wire_batch; every client is decoded and checked.  With --key-store the lanes' keys are bound from the store first
        // --device-client (not a flag of the reference): keys, queries and decoding through client sessions on the GPU, one per client of a --batch
        if (!strcmp(argv[i], "--device-client")) { cout << "Using client sessions on the device for keys, queries and decoding" << endl; g_device_client = true; }
        if (!strcmp(argv[i], "--query-batch")) { cout << "Taking the batch's queries in one call and its responses in one read" << endl; query_batch = true; }
        // --batch B --instances F together: B clients -- own keys, own indices -- each fetch an item of F plaintexts in ONE call of
        // spiral_gpu_server_answer_batch_instances; every plaintext of every client is decoded from its wire form and checked
        // --output-err F (src/spiral.cpp:1287-1291) asks the reference to dump its empirical noise statistics (analyze_err.py's
        // input).  Here a client session measures them (report_noise above), so the flag takes --device-client; the host client has no such
        // path: without --device-client the flag and its file name are consumed so that a driver's command line parses the same way, and the
        // file is not written.
        if (!strcmp(argv[i], "--output-err") && i + 1 < argc) g_output_err = argv[++i];
        // --record-bytes S (not a flag of the reference): IDX_TARGET names a record of S bytes; load_records, one query, decode, update_records, again
        if (!strcmp(argv[i], "--record-bytes")) {
            record_run = true;
            if (i + 1 < argc) record_bytes = strtoull(argv[++i], nullptr, 10);
        }
        // --pack-record-bytes S with --high-rate: the records run on SpiralPack servers, OUTN as out_n
        if (!strcmp(argv[i], "--pack-record-bytes")) {
            pack_record_run = true;
            if (i + 1 < argc) pack_record_bytes = strtoull(argv[++i], nullptr, 10);
        }
        // --kv-value-bytes V with --device-client (and --high-rate for a SpiralPack server): IDX_TARGET names key number K of a keyed table (run_kv above)
        if (!strcmp(argv[i], "--kv-value-bytes")) {
            kv_run = true;
            if (i + 1 < argc) kv_value_bytes = strtoull(argv[++i], nullptr, 10);
        }
        // --kv-scan with --kv-value-bytes: the run ends with a listing of the whole table, reconciled against the keys it stored
        if (!strcmp(argv[i], "--kv-scan")) kv_scan = true;
    }
    if (kv_scan && !kv_run) {
        fprintf(stderr, "spiral: --kv-scan takes --kv-value-bytes V (it lists the keyed table that run builds)\n");
        return 1;
    }
    if (kv_run) {
        if (kv_value_bytes == 0) {
            fprintf(stderr, "spiral: --kv-value-bytes takes a value size of at least 1 byte\n");
            return 1;
        }
        if (!g_device_client) {
            fprintf(stderr, "spiral: --kv-value-bytes takes --device-client (the lookup's queries and its find run in a client session on the device)\n");
            return 1;
        }
        const char* with = record_run ? "--record-bytes" : pack_record_run ? "--pack-record-bytes" : key_store >= 0 ? "--key-store" : query_batch ? "--query-batch"
                           : instances ? "--instances" : batch ? "--batch" : g_wire ? "--wire-input / --seeded" : !g_output_err.empty() ? "--output-err" : nullptr;
        if (with) {
            fprintf(stderr, "spiral: --kv-value-bytes does not go with %s (a run of its own: load, private lookups of one key, kv_put, kv_stats)\n", with);
            return 1;
        }
    }
    if (pack_record_run) {
        if (pack_record_bytes == 0) {
            fprintf(stderr, "spiral: --pack-record-bytes takes a record size of at least 1 byte\n");
            return 1;
        }
        const char* with = !high_rate ? nullptr : record_run ? "--record-bytes" : key_store >= 0 ? "--key-store" : query_batch ? "--query-batch" : instances ? "--instances" : batch ? "--batch" : g_wire ? "--wire-input / --seeded" : nullptr;
        if (!high_rate || with) {
            if (!high_rate) fprintf(stderr, "spiral: --pack-record-bytes takes --high-rate (records on a base server: --record-bytes)\n");
            else fprintf(stderr, "spiral: --pack-record-bytes does not go with %s (a one-query run; the layout chooses its own instances)\n", with);
            return 1;
        }
    }
    if (record_run) {
        if (record_bytes == 0) {
            fprintf(stderr, "spiral: --record-bytes takes a record size of at least 1 byte\n");
            return 1;
        }
        if (show_diff || random_data) cout << "--record-bytes: " << (show_diff ? "--show-diff" : "--random-data") << " has no meaning in a records run (ignored)" << endl;
        if (argc > 4 && strcmp(argv[4], "a")) cout << "--record-bytes: the database is generated, the file argument " << argv[4] << " is not read (ignored)" << endl;
        const char* with = key_store >= 0 ? "--key-store" : query_batch ? "--query-batch" : high_rate ? "--high-rate" : instances ? "--instances" : batch ? "--batch" : nullptr;
        if (with) {
            fprintf(stderr, "spiral: --record-bytes does not go with %s (a one-query run of a base server; the layout chooses its own instances)\n", with);
            return 1;
        }
    }
    if (!g_output_err.empty() && !g_device_client) {
        cout << "--output-err " << g_output_err << ": noise statistics are not produced by this build without --device-client (ignored)" << endl;
        g_output_err.clear();
    }
    if (!g_output_err.empty() && (batch || instances || key_store >= 0 || query_batch)) {
        fprintf(stderr, "spiral: --output-err takes --device-client on a one-query run (not with --batch, --instances, --key-store or --query-batch)\n");
        return 1;
    }
    const bool item_batch = batch && instances;
    if (item_batch && (batch < 2 || batch > 8 || instances < 2 || instances > 16 || high_rate)) {
        fprintf(stderr, "spiral: --batch B --instances F takes B in 2 .. 8 and F in 2 .. 16 (and no --high-rate)\n");
        return 1;
    }
    if (query_batch && (batch < 2 || batch > 8 || instances || high_rate)) {
        fprintf(stderr, "spiral: --query-batch takes --batch B in 2 .. 8 (not with --instances or --high-rate)\n");
        return 1;
    }
    if (query_batch) g_wire = true;  // (the wire form unless --seeded chose the seeded one)
    if (g_wire && ((batch && (batch < 2 || batch > 8)) || (instances && (instances < 2 || instances > 16 || high_rate)))) {
        fprintf(stderr, "spiral: %s takes --batch B in 2 .. 8 and --instances F in 2 .. 16 (not with --high-rate)\n", g_seeded ? "--seeded" : "--wire-input");
        return 1;
    }
    if (key_store >= 0 && (batch < 2 || batch > 8 || instances || high_rate)) {
        fprintf(stderr, "spiral: --key-store takes --batch B in 2 .. 8 (not with --instances or --high-rate)\n");
        return 1;
    }
    if (!record_run && !pack_record_run && !kv_run && idx_target >= total_n) {
        fprintf(stderr, "spiral: IDX_TARGET %llu out of range (n = %llu)\n", (unsigned long long)idx_target, (unsigned long long)total_n);
        return 1;
    }

    spiral_gpu_params p{};
    p.nu1 = nu1;
    p.nu2 = nu2;
    p.t_exp = (uint32_t)param(argc, argv, "TEXP", 8);
    p.t_exp_right = (uint32_t)param(argc, argv, "TEXPRIGHT", 56);
    p.t_conv = (uint32_t)param(argc, argv, "TCONV", 4);
    p.t_gsw = (uint32_t)param(argc, argv, "TGSW", 8);
    p.qprime_bits = (uint32_t)param(argc, argv, "QPBITS", 20);
    p.p_db = param(argc, argv, "PVALUE", 256);
    const uint64_t qnum_first = param(argc, argv, "QNUMFIRST", direct_flag ? (1ull << nu1) : 1);
    const uint64_t qnum_rest = param(argc, argv, "QNUMREST", direct_flag ? (uint64_t)p.t_gsw * nu2 : 0);
    const bool du_first = qnum_first >= (1ull << nu1), du_rest = qnum_rest >= (uint64_t)nu2 * p.t_gsw;  // src/spiral.cpp:2060-2061
    if (du_first != du_rest || (!du_first && (qnum_first != 1 || qnum_rest != 0))) {
        fprintf(stderr, "spiral: unsupported QNUMFIRST/QNUMREST combination (supported: 1/0 and 2^nu1 / t_GSW*nu2)\n");
        return 1;
    }
    p.direct_upload = du_first ? 1 : 0;
    if (du_rest) cout << "directly uploading Regev -> GSW ciphertexts" << endl;

    if (spiral_gpu_device_count() <= 0) {
        fprintf(stderr, "spiral: no ROCm device found; this build has no CPU path\n");
        return 1;
    }
    if (kv_run) return run_kv(p, high_rate ? (uint32_t)param(argc, argv, "OUTN", 2) : 0u, idx_target, kv_value_bytes, seed, nonoise, kv_scan);
    if (record_run) return run_records(p, idx_target, record_bytes, seed, nonoise);
    if (pack_record_run) return run_pack_records(p, (uint32_t)param(argc, argv, "OUTN", 2), idx_target, pack_record_bytes, seed, nonoise);
    if (high_rate) return run_high_rate(p, (uint32_t)param(argc, argv, "OUTN", 2), idx_target, seed, nonoise, show_diff, qnum_first, batch, instances);
    spiral_gpu_shape s;
    GPU_OK(spiral_gpu_get_shape(&p, &s));
    cout << "dim0: " << s.dim0 << endl;
    cout << "num_per: " << s.num_per << endl;

    // ---- database (load_db, src/spiral.cpp:1028-1172): explicit seeded database generated on the device; with
    // --random-data the same (a full-size database is cheap on the GPU, so the result is still checkable)
    const uint64_t db_seed = 1234;
    spiral_gpu_server* srv = nullptr;
    GPU_OK(spiral_gpu_server_create(&p, 0, 0, 0, &srv));
    cout << "starting generation of db" << endl;
    GPU_OK(spiral_gpu_server_gen_db(srv, db_seed));
    cout << "done loading/generating db." << endl;
    (void)random_data;

    // ---- client: keys, public parameters, query
    double time_key_gen = 0, time_query_gen = 0, time_decoding = 0;
    Client cl(p, seed, nonoise);
    cl.seeded = g_seeded;
    cl.form = client_form();
    uint64_t t0 = now_us();
    cl.keygen();
    cl.gen_pub_params();
    time_key_gen = (double)(now_us() - t0);
    if (!p.direct_upload) {
        cout << "g = " << s.g << endl;
        cout << "stopround = " << s.stopround << endl;
    }
    t0 = now_us();
    const Query query = cl.query(idx_target);
    time_query_gen = (double)(now_us() - t0);

    // ---- server
    cout << "Beginning query processing..." << endl;
    Poly final_ct(6 * N), resp(6 * N);
    double us[8];
    std::vector<uint8_t> qwire;  // (--wire-input) the query as sent
    if (g_wire) {
        const std::vector<uint8_t> pw = pp_msg(p, s, cl);
        qwire = query_msg(query);
        g_wire_offline = pw.size(), g_wire_online = qwire.size();
        GPU_OK(set_pp_msg(srv, pw));
        for (int it = 0; it < 2; it++) {  // warm-up (table upload, first launches), then the answer
            GPU_OK(set_query_msg(srv, qwire));
            GPU_OK(spiral_gpu_server_answer_resident(srv, us));
        }
    } else {
        GPU_OK(spiral_gpu_server_set_pub_params(srv, cl.w_left.data(), cl.w_right.data(), cl.w.data(), cl.v.data()));
        GPU_OK(spiral_gpu_server_answer(srv, query.cts.data(), final_ct.data(), resp.data(), us));  // warm-up (table upload, first launches)
        GPU_OK(spiral_gpu_server_answer(srv, query.cts.data(), final_ct.data(), resp.data(), us));
    }
    const double time_expansion_main = us[0], time_conversion = us[1], time_first_multiply = us[2], time_folding = us[3];
    cout << std::fixed << std::setprecision(0);
    cout << "Expansion took (CPU·us): " << time_expansion_main << endl;
    if (p.direct_upload) cout << "directly uploading Regev ciphertexts" << endl;
    cout << "ScalToMat took (CPU·us): " << us[7] << endl;
    cout << "RegevToGSW took (CPU·us): " << (us[1] - us[7]) << endl;
    cout << "done folding" << endl;
    cout << "Done with query processing!" << endl;

    // ---- client decode + check_final (src/spiral.cpp:1412-1494)
    // the response travels in its wire form (bit-packed on the device, include/spiral_gpu.h); the client unpacks and decodes it
    std::vector<uint8_t> wire(spiral_gpu_response_wire_bytes(&p, 2));
    GPU_OK(spiral_gpu_server_read_response_wire(srv, wire.data(), wire.size()));
    t0 = now_us();
    GPU_OK(spiral_gpu_response_from_wire(&p, 2, wire.data(), resp.data()));
    Poly pt = cl.decode(resp.data());
    time_decoding = (double)(now_us() - t0);
    Poly corr = db_item(db_seed, idx_target, p.p_db);
    const bool is_corr = pt == corr;
    cout << "Is correct?: " << (is_corr ? 1 : 0) << endl;
    if (show_diff)
        for (size_t i = 0; i < pt.size(); i++)
            if (pt[i] != corr[i]) cout << i << " " << corr[i] << ", " << pt[i] << endl;
    if (!g_output_err.empty()) {
        GPU_OK(spiral_gpu_server_read(srv, SPIRAL_GPU_BUF_FINAL, final_ct.data()));
        report_noise(cl.session.get(), final_ct.data(), wire, corr, 2, s.qprime);
    }

    // ---- --batch B: the same server, B queries of B clients in one launch sequence (include/spiral_gpu.h, spiral_gpu_server_run_query_batch)
    double batch_us = 0;
    bool batch_corr = true;
    // B clients on srv and B - 1 lanes of it (--batch alone, or with --instances)
    std::vector<spiral_gpu_server*> lanes{srv};
    std::vector<Client> clients;
    std::vector<uint64_t> idxs;
    auto make_clients = [&]() {
        clients.reserve(batch);
        for (uint32_t b = 0; b < batch; b++) {
            if (b) {
                spiral_gpu_server* lane = nullptr;
                GPU_OK(spiral_gpu_server_create_lane(srv, &lane));
                GPU_OK(spiral_gpu_server_set_stream(lane, spiral_gpu_server_get_stream(srv)));  // the lanes of a batch on one stream: no event ordering around the launch sequence
                lanes.push_back(lane);
            }
            clients.emplace_back(p, seed + 1 + b, nonoise);
            clients[b].seeded = g_seeded;
            clients[b].form = client_form();
            clients[b].keygen();
            clients[b].gen_pub_params();
            idxs.push_back((idx_target + 1 + 7919ull * b) % total_n);
            const Query qb = clients[b].query(idxs[b]);
            if (g_wire) {
                GPU_OK(set_pp_msg(lanes[b], pp_msg(p, s, clients[b])));
                GPU_OK(set_query_msg(lanes[b], query_msg(qb)));
            } else {
                GPU_OK(spiral_gpu_server_set_pub_params(lanes[b], clients[b].w_left.data(), clients[b].w_right.data(), clients[b].w.data(), clients[b].v.data()));
                GPU_OK(spiral_gpu_server_set_query(lanes[b], qb.cts.data()));
            }
        }
        return 0;
    };
    if (!item_batch && batch >= 2 && batch <= 8) {
        if (make_clients()) return 1;
        GPU_OK(spiral_gpu_server_use_graphs(srv, 1));
        const int reps = 10;
        for (int it = 0; it < 2 + reps; it++) {  // two untimed passes (graph capture, first replay), then `reps` timed ones
            if (it == 2) {
                GPU_OK(spiral_gpu_server_sync(srv));
                t0 = now_us();
            }
            GPU_OK(spiral_gpu_server_run_query_batch(lanes.data(), batch));
        }
        GPU_OK(spiral_gpu_server_sync(srv));
        batch_us = (double)(now_us() - t0) / reps;
        cout << "Batch of " << batch << " queries, Is correct?:";
        for (uint32_t b = 0; b < batch; b++) {
            GPU_OK(spiral_gpu_server_sync(lanes[b]));
            GPU_OK(spiral_gpu_server_read_response_wire(lanes[b], wire.data(), wire.size()));
            GPU_OK(spiral_gpu_response_from_wire(&p, 2, wire.data(), resp.data()));
            const bool ok = clients[b].decode(resp.data()) == db_item(db_seed, idxs[b], p.p_db);
            batch_corr = batch_corr && ok;
            cout << " " << (ok ? 1 : 0);
        }
        cout << endl;
        spiral_gpu_key_store* store = nullptr;
        if (key_store >= 0) {  // client c's keys into slot c, in the form they travel in; then lane b serves the client of slot (b + round) mod B
            GPU_OK(spiral_gpu_key_store_create(&p, 0, 0, batch, key_store, &store));
            for (uint32_t c = 0; c < batch; c++) {
                const std::vector<uint8_t> m = g_wire ? pp_msg(p, s, clients[c]) : std::vector<uint8_t>();
                if (g_seeded) GPU_OK(spiral_gpu_key_store_put_seeded(store, c, m.data(), m.size()));
                else if (g_wire) GPU_OK(spiral_gpu_key_store_put_wire(store, c, m.data(), m.size()));
                else GPU_OK(spiral_gpu_key_store_put(store, c, clients[c].w_left.data(), clients[c].w_right.data(), clients[c].w.data(), clients[c].v.data()));
            }
            cout << "Key store: " << batch << " slots of " << spiral_gpu_key_store_slot_bytes(&p, 0, key_store) << " bytes" << endl;
            for (uint32_t round = 0; round < 2; round++) {
                std::vector<uint32_t> slots(batch);
                for (uint32_t b = 0; b < batch; b++) slots[b] = (b + round) % batch;
                GPU_OK(spiral_gpu_server_bind_keys(lanes.data(), batch, store, slots.data()));
                for (uint32_t b = 0; b < batch; b++) {
                    const Query qb = clients[slots[b]].query(idxs[slots[b]]);
                    if (g_wire) GPU_OK(set_query_msg(lanes[b], query_msg(qb)));
                    else GPU_OK(spiral_gpu_server_set_query(lanes[b], qb.cts.data()));
                }
                GPU_OK(spiral_gpu_server_run_query_batch(lanes.data(), batch));
                for (uint32_t b = 0; b < batch; b++) {
                    GPU_OK(spiral_gpu_server_sync(lanes[b]));
                    GPU_OK(spiral_gpu_server_read_response_wire(lanes[b], wire.data(), wire.size()));
                    GPU_OK(spiral_gpu_response_from_wire(&p, 2, wire.data(), resp.data()));
                    const bool ok = clients[slots[b]].decode(resp.data()) == db_item(db_seed, idxs[slots[b]], p.p_db);
                    batch_corr = batch_corr && ok;
                    cout << "Key store round " << round << ", client " << slots[b] << " on lane " << b << ", Is correct?: " << (ok ? 1 : 0) << endl;
                }
            }
        }
        if (query_batch) {  // lane b serves client who[b]: its own, or with a key store the client two lanes on, bound from its slot
            std::vector<uint32_t> who(batch);
            for (uint32_t b = 0; b < batch; b++) who[b] = store ? (b + 2) % batch : b;
            if (store) GPU_OK(spiral_gpu_server_bind_keys(lanes.data(), batch, store, who.data()));
            std::vector<uint64_t> fresh(batch);
            std::vector<std::vector<uint8_t>> msgs;
            std::vector<const void*> mp;
            for (uint32_t b = 0; b < batch; b++) {
                fresh[b] = (idxs[who[b]] + 4099ull) % total_n;
                msgs.push_back(query_msg(clients[who[b]].query(fresh[b])));
            }
            for (uint32_t b = 0; b < batch; b++) mp.push_back(msgs[b].data());
            GPU_OK(spiral_gpu_server_set_query_batch(lanes.data(), batch, g_seeded ? SPIRAL_GPU_FORM_SEEDED : SPIRAL_GPU_FORM_WIRE, mp.data(), msgs[0].size()));
            cout << "The batch's " << batch << " queries went in as one set_query_batch call (" << (g_seeded ? "seeded" : "wire") << " form, " << msgs[0].size()
                 << " bytes each)" << endl;
            GPU_OK(spiral_gpu_server_run_query_batch(lanes.data(), batch));
            std::vector<uint8_t> wires(batch * wire.size());
            GPU_OK(spiral_gpu_server_read_response_wire_batch(lanes.data(), batch, wires.data(), wires.size()));
            for (uint32_t b = 0; b < batch; b++) {
                GPU_OK(spiral_gpu_response_from_wire(&p, 2, wires.data() + b * wire.size(), resp.data()));
                const bool ok = clients[who[b]].decode(resp.data()) == db_item(db_seed, fresh[b], p.p_db);
                batch_corr = batch_corr && ok;
                cout << "Query batch, client " << who[b] << " on lane " << b << ", Is correct?: " << (ok ? 1 : 0) << endl;
            }
        }
        if (store) spiral_gpu_key_store_destroy(store);
        GPU_OK(spiral_gpu_server_use_graphs(srv, 0));
        for (uint32_t b = 1; b < batch; b++) spiral_gpu_server_destroy(lanes[b]);
    } else if (!item_batch && batch) {
        fprintf(stderr, "spiral: --batch takes 2 .. 8\n");
        return 1;
    }

    // ---- --instances F: the item at idx_target = plaintext idx_target of F databases (instance k seeded db_seed + k; instance 0 is the server above)
    double item_us = 0;
    bool item_corr = true;
    std::vector<spiral_gpu_server*> inst{srv};
    auto make_instances = [&]() {
        for (uint32_t k = 1; k < instances; k++) {
            spiral_gpu_server* sv = nullptr;
            GPU_OK(spiral_gpu_server_create(&p, 0, 0, 0, &sv));
            GPU_OK(spiral_gpu_server_gen_db(sv, db_seed + k));
            inst.push_back(sv);
        }
        return 0;
    };
    if (!item_batch && instances >= 2 && instances <= 16) {
        if (make_instances()) return 1;
        std::vector<uint64_t> resps((size_t)instances * 6 * N);
        GPU_OK(spiral_gpu_server_use_graphs(srv, 1));
        if (g_wire) {  // the query decoded into srv's buffer, the item answered by the resident entry point into device buffers
            void* d_resp = nullptr;
            HIP_CLI_OK(hipMalloc(&d_resp, resps.size() * sizeof(uint64_t)));
            for (int it = 0; it < 3; it++) {
                GPU_OK(set_query_msg(srv, qwire));
                t0 = now_us();
                GPU_OK(spiral_gpu_server_run_query_instances(srv, inst.data(), instances, 1, d_resp, nullptr));
                GPU_OK(spiral_gpu_server_sync(srv));
                item_us = (double)(now_us() - t0);
            }
            HIP_CLI_OK(hipMemcpy(resps.data(), d_resp, resps.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
            HIP_CLI_OK(hipFree(d_resp));
        } else {
            for (int it = 0; it < 3; it++)  // capture, a replay, the timed replay
                GPU_OK(spiral_gpu_server_answer_instances(srv, inst.data(), instances, query.cts.data(), resps.data(), nullptr, &item_us));
        }
        cout << "Item of " << instances << " plaintexts, Is correct?:";
        for (uint32_t k = 0; k < instances; k++) {
            const bool ok = cl.decode(resps.data() + (size_t)k * 6 * N) == db_item(db_seed + k, idx_target, p.p_db);
            item_corr = item_corr && ok;
            cout << " " << (ok ? 1 : 0);
        }
        cout << endl;
        GPU_OK(spiral_gpu_server_use_graphs(srv, 0));
        for (uint32_t k = 1; k < instances; k++) spiral_gpu_server_destroy(inst[k]);
    } else if (!item_batch && instances) {
        fprintf(stderr, "spiral: --instances takes 2 .. 16\n");
        return 1;
    }

    // ---- --batch B --instances F: B clients' items of F plaintexts (client b's item at idxs[b] of the F databases) in one item batch, wire form out
    double item_batch_us = 0;
    if (item_batch) {
        if (make_clients() || make_instances()) return 1;
        const size_t wb = wire.size();
        std::vector<uint8_t> wires((size_t)batch * instances * wb);
        std::vector<Query> queries;
        std::vector<const uint64_t*> qp;
        for (uint32_t b = 0; b < batch; b++) queries.push_back(clients[b].query(idxs[b]));
        for (uint32_t b = 0; b < batch; b++) qp.push_back(queries[b].cts.data());
        GPU_OK(spiral_gpu_server_use_graphs(srv, 1));
        if (g_wire) {  // each client's query decoded into its lane, the item batch answered by the resident entry point, wire forms to the host
            std::vector<std::vector<uint8_t>> qws;
            for (uint32_t b = 0; b < batch; b++) qws.push_back(query_msg(queries[b]));
            void* d_wire = nullptr;
            HIP_CLI_OK(hipMalloc(&d_wire, wires.size()));
            for (int it = 0; it < 3; it++) {
                for (uint32_t b = 0; b < batch; b++) GPU_OK(set_query_msg(lanes[b], qws[b]));
                t0 = now_us();
                GPU_OK(spiral_gpu_server_run_query_batch_instances(lanes.data(), batch, inst.data(), instances, 1, nullptr, nullptr, d_wire));
                GPU_OK(spiral_gpu_server_sync(srv));
                item_batch_us = (double)(now_us() - t0);
            }
            HIP_CLI_OK(hipMemcpy(wires.data(), d_wire, wires.size(), hipMemcpyDeviceToHost));
            HIP_CLI_OK(hipFree(d_wire));
        } else {
            for (int it = 0; it < 3; it++)  // image conversion + capture, a replay, the timed replay
                GPU_OK(spiral_gpu_server_answer_batch_instances(lanes.data(), batch, inst.data(), instances, qp.data(), nullptr, wires.data(), &item_batch_us));
        }
        cout << "Batch of " << batch << " items of " << instances << " plaintexts, Is correct?:";
        for (uint32_t b = 0; b < batch; b++) {
            bool ok = true;
            for (uint32_t k = 0; k < instances; k++) {
                GPU_OK(spiral_gpu_response_from_wire(&p, 2, wires.data() + ((size_t)b * instances + k) * wb, resp.data()));
                ok = ok && clients[b].decode(resp.data()) == db_item(db_seed + k, idxs[b], p.p_db);
            }
            batch_corr = batch_corr && ok;
            cout << " " << (ok ? 1 : 0);
        }
        cout << "  (device " << item_batch_us << " us)" << endl;
        GPU_OK(spiral_gpu_server_use_graphs(srv, 0));
        for (uint32_t b = 1; b < batch; b++) spiral_gpu_server_destroy(lanes[b]);
        for (uint32_t k = 1; k < instances; k++) spiral_gpu_server_destroy(inst[k]);
    }

    // ---- print_summary (src/spiral.cpp:209-265)
    const double pt_mod = std::log2((double)p.p_db);
    const size_t pt_elem_size = (size_t)((2.0 * 2 * N * pt_mod) / 8.0);
    const size_t b_per_elem = (size_t)((double)N * 56 / 8.0);
    const size_t dim0_query_size = (size_t)(qnum_first + qnum_rest) * 2 * b_per_elem;
    const size_t total_resp_size = wire.size();  // = ((n0 n0 N (log2 p + 2)) + (n0 N q'bits)) / 8, src/spiral.cpp:231-233
    cout << endl;
    cout << "PIR over n=" << total_n << " elements of size " << pt_elem_size << " bytes each." << endl;
    cout << "The database is structured as " << (1 << nu1) << " x 2^" << nu2 << "." << endl;
    cout << endl;
    cout << "Communication" << endl;
    cout << endl;
    cout << "         Total offline query size (b): " << cl.offline_bytes << endl;
    cout << "                  First dimension (b): " << dim0_query_size << endl;
    cout << "       Total for other dimensions (b): " << 0 << endl;
    cout << "          Total online query size (b): " << dim0_query_size << endl;
    cout << "                    Response size (b) : " << total_resp_size << endl;
    cout << endl;
    cout << endl;
    cout << "Database-independent computation" << endl;
    cout << endl;
    cout << "              Main expansion  (CPU·us): " << time_expansion_main << endl;
    cout << "  Further dimension expansion (CPU·us): " << 0 << endl;
    cout << "                   Conversion (CPU·us): " << time_conversion << endl;
    cout << "                        Total (CPU·us): " << (time_expansion_main + time_conversion) << endl;
    cout << endl;
    cout << "Database-dependent computation" << endl;
    cout << endl;
    cout << "     First dimension multiply (CPU·us): " << time_first_multiply << endl;
    cout << "                      Folding (CPU·us): " << time_folding << endl;
    cout << "                        Total (CPU·us): " << (time_first_multiply + time_folding) << endl;
    cout << endl;
    cout << "Client computation" << endl;
    cout << endl;
    cout << "               Key generation (CPU·us): " << time_key_gen << endl;
    cout << "             Query generation (CPU·us): " << time_query_gen << endl;
    cout << "                     Decoding (CPU·us): " << time_decoding << endl;
    cout << endl;
    // MI355X extras (not scraped by select_params.py)
    cout << "GPU extras" << endl;
    cout << endl;
    cout << "        Sweep kernel alone (GPU·us): " << us[5] << endl;
    cout << "      Response switch kernel (GPU·us): " << us[4] << endl;
    cout << "        Whole answer, device (GPU·us): " << us[6] << endl;
    if (batch_us > 0) cout << "   Batch of " << batch << " queries, wall (GPU·us): " << batch_us << endl;
    if (item_batch_us > 0)
        cout << "   Batch of " << batch << " items of " << instances << " plaintexts (" << batch << " clients, " << instances << " database instances), device (GPU·us): "
             << item_batch_us << endl;
    print_wire_bytes();
    if (item_us > 0) cout << "   Item of " << instances << " plaintexts (one query, " << instances << " database instances), device (GPU·us): " << item_us << endl;
    spiral_gpu_server_destroy(srv);
    return (is_corr && batch_corr && item_corr) ? 0 : 2;
}
