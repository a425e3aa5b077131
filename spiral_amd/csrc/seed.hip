// Row 0 of a seeded message (seed_device.h), generated on the device straight into its PK destinations: the server's half of
// set_query_seeded / set_pub_params_seeded (host_common.h ingest_seeded).  Row 0 is defined in NTT / CRT form, so no transform follows.
//
// One thread computes one ChaCha20 block -- both residues of slots 2c and 2c + 1 -- and writes the two PK words with one 16-byte store.
// The slot pair is taken from the thread index through the inverse of pk_pos: thread i of a polynomial (0 .. 1023) takes c = (i mod 256) * 4 +
// i / 256, whose words pk_pos(2c), pk_pos(2c + 1) are 2i and 2i + 1, so a wave's stores cover 1 KiB of consecutive bytes.
#include "common.h"
#include "kernels.h"
#include "seed_device.h"

namespace spiral {

namespace {

__global__ __launch_bounds__(256) void seed_rows_kernel(Seed key, uint32_t domain, uint64_t k0, uint64_t* pk, IndexMap map, uint32_t j0) {
    const uint32_t j = j0 + blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
    seed_store_pair(key.w, domain, k0 + j, i, [&] { return pk + (size_t)map(j) * kN; });
}

}  // namespace

// polynomials j0 .. j0 + n - 1 per launch, n <= kSeedLaunchPolys: gridDim.y stays below the 65 536 a device may allow
constexpr uint32_t kSeedLaunchPolys = 32768;
void launch_seed_rows(const uint8_t* seed, uint32_t domain, uint64_t k0, uint64_t* pk, IndexMap map, uint32_t npolys, hipStream_t s) {
    const Seed key = seed_words(seed);
    for (uint32_t j0 = 0; j0 < npolys; j0 += kSeedLaunchPolys) {
        const uint32_t n = npolys - j0 < kSeedLaunchPolys ? npolys - j0 : kSeedLaunchPolys;
        hipLaunchKernelGGL(seed_rows_kernel, dim3(kN / 512u, n), dim3(256), 0, s, key, domain, k0, pk, map, j0);
    }
}

}  // namespace spiral
