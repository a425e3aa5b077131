// Host client for the ./spiral command line: key generation, public parameters, query encoding and response
// decoding (the CLIENT half of the reference: src/client.cpp and the client parts of src/spiral.cpp:2040-2331,
// 1451-1494).  Not part of the server hot path.  All ring arithmetic goes through libspiral_gpu.so's C ABI
// (to_ntt / multiply / add / automorph ...), so this program contains no CPU NTT; the only CPU polynomial
// arithmetic is the final decode product modulo q' (the reference uses HEXL there, src/util.cpp:213-274).
#pragma once
#include <array>
#include <cstdint>
#include <memory>
#include <random>
#include <vector>

#include "../../../include/spiral_gpu.h"

namespace spiral_cli {

constexpr uint32_t N = 2048;
constexpr uint64_t P = 268369921ull, B = 249561089ull, Q = P * B;
using Poly = std::vector<uint64_t>;  // raw: N words per polynomial; NTT form: 2N words per polynomial

// --seeded (include/spiral_gpu.h, spiral_gpu_query_seeded_bytes): row 0 of every matrix of a message -- the -a of its Regev samples -- is
// spiral_gpu_seed_expand under a seed drawn from the client's RNG instead of uniform_polys.  `k` is the message's next row-0 polynomial: whoever
// generates a matrix sets it to the matrix's place in the message first.
struct Row0 {
    bool on = false;
    uint8_t seed[32] = {};
    uint32_t domain = 0;
    uint64_t k = 0;
    void begin(std::mt19937_64& rng, uint32_t d);  // a fresh seed for one message of domain d
    Poly take(size_t m);                           // the next m row-0 polynomials, NTT form
};
// a query as the client sends it: its ciphertexts (NTT form) and, with --seeded, the fresh seed their row 0 was expanded from
struct Query {
    Poly cts;
    std::array<uint8_t, 32> seed{};
    std::vector<uint8_t> msg;  // --device-client with a message form: the query as the session emitted it (cts stays empty)
};

// --device-client: keys, queries and decoding go through a client session of the library (include/spiral_gpu.h spiral_gpu_client_*) instead of the
// host code below.  `form` selects it, before keygen(): -1 the host client (the default), else the form the session emits its messages in --
// SPIRAL_GPU_FORM_NTT (the public parameters land in the NTT-form members, a query in Query::cts), SPIRAL_GPU_FORM_WIRE or _SEEDED (pp_message,
// Query::msg).  The session's 32-byte seed is drawn from mt19937_64(seed).
std::shared_ptr<spiral_gpu_client> open_session(const spiral_gpu_params& p, uint32_t out_n, uint64_t seed, bool nonoise);

struct Client {
    spiral_gpu_params p;
    spiral_gpu_shape s;
    bool nonoise = false;
    std::mt19937_64 rng;
    std::vector<double> cdf;
    Poly sr;  // 1 x 1 raw: Regev secret
    Poly sp;  // n0 x 1 raw: matrix-Regev secret
    Poly w_left, w_right, w, v;  // public parameters, reference NTT layout
    uint64_t offline_bytes = 0;
    bool seeded = false;                       // --seeded: the messages' row 0 from seeds
    Row0 row0;                                 // (while a message is generated)
    uint8_t pp_seed[32] = {};                  // the seed of the public parameters
    int form = -1;                             // --device-client (above)
    uint64_t seed0 = 0;
    std::shared_ptr<spiral_gpu_client> session;
    std::vector<uint8_t> pp_message;

    Client(const spiral_gpu_params& params, uint64_t seed, bool nonoise_);
    void keygen();
    void gen_pub_params();
    Query query(uint64_t idx_target);
    Poly decode(const uint64_t* response) const;  // -> n0 x n2 raw plaintext in [0, p_db)

  private:
    Poly query_cts(uint64_t idx_target);
    uint64_t sample_noise();
    Poly noise_polys(size_t n);
    Poly uniform_polys(size_t n);
    Poly regev_samples(size_t m);                                  // n0 x m NTT
    Poly fresh_public_key(size_t m);                               // n1 x m NTT
    Poly public_encryptions(uint32_t count, uint32_t t_dim);       // count x (n0 x t_dim) NTT
    Poly encrypt_simple_regev(const Poly& sigma_raw);              // n0 x 1 NTT
};

// SpiralPack / SpiralStreamPack client (src/testing.cpp:905-1006, 1086-1122): base_dim x 1 Regev secret sr, out_n x 1
// matrix secret Sp, packing keys v_W, expansion keys, conversion key V.
struct PackClient {
    spiral_gpu_params p;
    spiral_gpu_pack_shape s;
    uint32_t out_n;
    bool nonoise = false;
    std::mt19937_64 rng;
    std::vector<double> cdf;
    Poly sr, sp;
    Poly w_left, w_right, v, v_w;
    uint64_t offline_bytes = 0;
    bool seeded = false;
    Row0 row0;
    uint8_t pp_seed[32] = {};
    int form = -1;  // --device-client (above)
    uint64_t seed0 = 0;
    std::shared_ptr<spiral_gpu_client> session;
    std::vector<uint8_t> pp_message;

    PackClient(const spiral_gpu_params& params, uint32_t out_n_, uint64_t seed, bool nonoise_);
    void keygen();
    void gen_pub_params();
    Query query(uint64_t idx_target);
    Poly decode(const uint64_t* response) const;  // -> out_n x out_n raw plaintexts

  private:
    Poly query_cts(uint64_t idx_target);
    uint64_t sample_noise();
    Poly noise_polys(size_t n);
    Poly uniform_polys(size_t n);
    Poly regev_samples(size_t m);
    Poly expansion_keys(uint32_t count, uint32_t t_dim);
    Poly encrypt_simple_regev(const Poly& sigma_raw);
};
Poly pack_db_item(uint64_t seed, uint64_t item, uint64_t total_n, uint32_t out_n, uint64_t p_db);

// plaintext item of the seeded explicit database (same generator as spiral_gpu_server_gen_db)
Poly db_item(uint64_t seed, uint64_t item, uint64_t p_db);

}  // namespace spiral_cli
