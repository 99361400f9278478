// aqua_bank.hip -- libaqua_bank.so (include/aqua_bank.h): a bank of the DQN's 5 -> 64 -> 64 -> 3 Q-networks
// (main/impl/dqn.py:301-314) acting on one batch of worlds in one launch on gfx950; network p takes the p-th segment of
// the batch.  Its own translation unit and library: libaqua_policy.so, whose results this one reproduces bit for bit per
// segment, is not touched by it and stays the packer of the weights.
//
// The network itself -- the blob's layout (one slot of the bank is one blob), the forward pass of a tile, the pick and
// its stores -- is stated in aqua_qnet.hpp, once for this library and libaqua_policy.so.  Here:
// the A operands are per wavefront, so a tile belongs to ONE network: the unit of work is the item (network p, tile j of
// p's segment), and every wavefront takes a contiguous run of items, reloading its weights (70 VGPRs, and a 324-float
// LDS part of its own) only where the network changes inside the run.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/aqua_bank.h"
#include "aqua_device.hpp"
#include "aqua_host.hpp"
#include "aqua_qnet.hpp"

namespace aqua_bank {

using namespace aqua::qnet;

static_assert(STREAM_POLICY == AQUABANK_STREAM, "aqua_bank.h names the stream of the policy draws");
static_assert(IN == AQUABANK_INPUTS && HID == AQUABANK_HIDDEN && ACT == AQUABANK_ACTIONS, "aqua_bank.h names the network's sizes");
constexpr int BLOCK = 256, WAVES = BLOCK / 64;
constexpr int WAVES_PER_SIMD = 3;        // resident wavefronts per SIMD = blocks per CU (<= 170 registers each)

struct BankArgs {
    const float* bank;
    const float* in;
    const float* epsilon_dev;
    int64_t seg, tiles;                  // worlds per network, tiles per network (items: live_items() below)
    int64_t share, rem;                  // items / wavefronts of the grid and the remainder: the first `rem` wavefronts take one more
    int64_t ld, N, env_offset, q_ld;
    float epsilon;
    uint64_t seed, tick;
    const uint64_t* tick_base;
    uint8_t* action;
    float* q;
    float* q_taken;
};

// what other lanes of this wavefront wrote to (or still read from) its LDS copy is complete before anything behind this
// point: the fences order the wavefront's own LDS traffic (the compiler may otherwise move a lane's load above another
// lane's store, which it cannot see), the barrier keeps the lanes' instructions on their side of it
__device__ __forceinline__ void wave_sync_lds()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// a wavefront-uniform value as the compiler can see it: in SGPRs, not in a 64-bit VGPR pair
__device__ __forceinline__ int64_t uniform(int64_t v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(static_cast<uint64_t>(v) >> 32));
    return static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
}

// RAW: `in` holds the environment's state rows and is normalised here; EPS: epsilon-greedy (one Philox draw per world)
template <bool RAW, bool EPS>
__global__ __launch_bounds__(BLOCK, WAVES_PER_SIMD) void qbank_kernel(const BankArgs a)
{
    // a copy of the LDS part per wavefront: the network is a property of the wavefront's item, not of the block
    __shared__ float4 lds_all[WAVES][LDS_FLOATS / 4];

    // (the wavefront's number as a scalar: the item bookkeeping below then lives in SGPRs, not in 64-bit VGPR pairs)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, col = lane & 31;
    float4* const lds4 = lds_all[wave];

    uint64_t tick = a.tick;
    if constexpr (EPS) {
        if (a.tick_base != nullptr) tick += *a.tick_base;
    }

    // this wavefront's contiguous run of items
    const int64_t w = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t first = w * a.share + (w < a.rem ? w : a.rem), count = a.share + (w < a.rem ? 1 : 0);
    if (count == 0) return;
    int64_t p = uniform(first / a.tiles), j = uniform(first % a.tiles);

    // the weights stay in registers while the network stays (70 VGPRs)
    float w1[K1_STEPS][2], w2[2][K2_STEPS];
    float eps = a.epsilon;
    int64_t loaded = -1;

    for (int64_t n = 0; n < count; ++n, ++j) {
        if (j == a.tiles) { j = 0; ++p; }
        const int64_t s = j * TILE + col;                     // the lane's world within the segment
        const int64_t i = p * a.seg + s;                      // ... and within the batch (the host counts live tiles only: < N + TILE)
        const bool live = s < a.seg && i < a.N;

        if (p != loaded) {
            loaded = p;
            const float* const blob = a.bank + p * BLOB_FLOATS;
            load_operands(blob, lane, w1, w2);
            const float4* const blob4 = reinterpret_cast<const float4*>(blob + OFF_LDS);
            wave_sync_lds();                                  // the reads of the previous network's copy are done
            static_assert(LDS_FLOATS / 4 > 64 && LDS_FLOATS / 4 <= 128, "two float4 per lane cover the LDS part");
            lds4[lane] = blob4[lane];
            if (lane < LDS_FLOATS / 4 - 64) lds4[64 + lane] = blob4[64 + lane];
            wave_sync_lds();                                  // the copy is complete before any lane reads it
            if constexpr (EPS) {
                if (a.epsilon_dev != nullptr) {
                    // by its bits (the library is built with -fno-honor-nans): NaN, and every negative value, never explore
                    const uint32_t bits = __float_as_uint(a.epsilon_dev[p]);
                    eps = bits > 0x7F800000u ? 0.0f : __uint_as_float(bits);
                }
            }
        }

        // k-step st of layer 1 takes input 2 st + h of the lane's world; dead worlds and the padding row are zero
        float x[K1_STEPS];
        const float* const xin = a.in + (h != 0 ? a.ld : 0) + i;
#pragma unroll
        for (int st = 0; st < K1_STEPS; ++st) x[st] = (live && 2 * st + h < IN) ? xin[2 * st * a.ld] : 0.0f;
        float q[ACT];
        forward<RAW>(lds4, w1, w2, x, h, q);
        if (h == 0 && live)
            pick_and_store<EPS>(q[0], q[1], q[2], eps, a.seed, static_cast<uint64_t>(a.env_offset + i), tick, i, a.action, a.q, a.q_ld, a.q_taken);
    }
}

// ------------------------------------------------------------------ host side
// The items of a launch: the tiles that hold a world below N, so the work follows N however large seg is.  Every network
// but the last one with a world has all its `tiles`; the last one, which N may cut, has those of its n_last worlds.  Item
// t is still (network t / tiles, tile t % tiles), because only the last network is short.
// 1 <= seg, 1 <= N <= networks * seg.  No overflow: (used - 1) * seg < N, so (used - 1) * tiles < N / TILE + used.
int64_t live_items(int64_t seg, int64_t N)
{
    const int64_t used = N / seg + (N % seg != 0 ? 1 : 0), tiles = seg / TILE + (seg % TILE != 0 ? 1 : 0);
    const int64_t n_last = N - (used - 1) * seg;
    return (used - 1) * tiles + n_last / TILE + (n_last % TILE != 0 ? 1 : 0);
}

}  // namespace aqua_bank

using namespace aqua_bank;

extern "C" {

int aquabank_version(void) { return AQUABANK_ABI_VERSION; }
const char* aquabank_last_error(void) { return g_err; }
size_t aquabank_weights_bytes(void) { return sizeof(float) * BLOB_FLOATS; }

int64_t aquabank_items(int64_t seg, int64_t N)
{
    if (seg < 1) return fail(AQUABANK_E_INVALID, "seg=%lld: must be >= 1", (long long)seg);
    if (N < 0) return fail(AQUABANK_E_INVALID, "N=%lld: must be >= 0", (long long)N);
    return N == 0 ? 0 : live_items(seg, N);
}

int aquabank_unpack_weights(const void* blob_host, float* k0, float* b0, float* k1, float* b1, float* k2, float* b2)
{
    if (blob_host == nullptr) return fail(AQUABANK_E_INVALID, "blob is NULL");
    if (k0 == nullptr || b0 == nullptr || k1 == nullptr || b1 == nullptr || k2 == nullptr || b2 == nullptr)
        return fail(AQUABANK_E_INVALID, "a kernel or bias pointer is NULL");
    if (!aligned(blob_host, 4)) return fail(AQUABANK_E_ALIGN, "blob must be 4-byte aligned");
    const float* const w = static_cast<const float*>(blob_host);
    float* const dst[6] = {k0, b0, k1, b1, k2, b2};
    for_each_parameter([&](int b, int a, int i) { dst[a][i] = w[b]; });
    return 0;
}

int aquabank_act_f32(const void* bank_dev, int64_t networks, int64_t seg, const float* in, int64_t ld, int in_is_normalised,
                     int64_t N, int64_t env_offset, float epsilon, const float* epsilon_dev, uint64_t seed, uint64_t tick,
                     const uint64_t* tick_base_dev, uint8_t* action, float* q, int64_t q_ld, float* q_taken, void* stream)
{
    if (bank_dev == nullptr) return fail(AQUABANK_E_INVALID, "the bank is NULL");
    if (!aligned(bank_dev, 16)) return fail(AQUABANK_E_ALIGN, "the bank must be 16-byte aligned");
    if (networks < 1 || networks > AQUABANK_MAX_NETWORKS)
        return fail(AQUABANK_E_INVALID, "networks=%lld: must be in [1, %d]", (long long)networks, AQUABANK_MAX_NETWORKS);
    if (seg < 1) return fail(AQUABANK_E_INVALID, "seg=%lld: must be >= 1", (long long)seg);
    if (N < 0 || ld < N) return fail(AQUABANK_E_INVALID, "bad sizes: N=%lld ld=%lld", (long long)N, (long long)ld);
    // N <= networks * seg without forming the product: the networks N needs, ceil(N / seg), are at most `networks`
    const int64_t used = N / seg + (N % seg != 0 ? 1 : 0);
    if (used > networks)
        return fail(AQUABANK_E_INVALID, "N=%lld worlds: more than networks * seg = %lld * %lld", (long long)N, (long long)networks, (long long)seg);
    if (env_offset < 0) return fail(AQUABANK_E_INVALID, "env_offset < 0");
    uint32_t eps_bits;                   // by its bits, as the kernel does: NaN or below zero (-0 is zero)
    std::memcpy(&eps_bits, &epsilon, sizeof(eps_bits));
    if (eps_bits > 0x7F800000u && eps_bits != 0x80000000u) return fail(AQUABANK_E_INVALID, "epsilon=%g: must be >= 0", (double)epsilon);
    if (action == nullptr && q == nullptr && q_taken == nullptr) return fail(AQUABANK_E_INVALID, "action, q and q_taken are all NULL");
    if (q != nullptr && q_ld < N) return fail(AQUABANK_E_INVALID, "q_ld=%lld < N=%lld", (long long)q_ld, (long long)N);
    if (N > 0 && in == nullptr) return fail(AQUABANK_E_INVALID, "in is NULL");
    if (!aligned(in, 4) || !aligned(q, 4) || !aligned(q_taken, 4)) return fail(AQUABANK_E_ALIGN, "in / q / q_taken must be 4-byte aligned");
    if (!aligned(epsilon_dev, 4)) return fail(AQUABANK_E_ALIGN, "epsilon_dev must be 4-byte aligned");
    if (!aligned(tick_base_dev, 8)) return fail(AQUABANK_E_ALIGN, "tick_base_dev must be 8-byte aligned");
    if (N == 0) return 0;

    int cus = 0;
    if (const int rc = compute_units(&cus, AQUABANK_E_NODEVICE)) return rc;
    BankArgs a;
    a.seg = seg;
    a.tiles = seg / TILE + (seg % TILE != 0 ? 1 : 0);
    const int64_t items = live_items(seg, N);      // not used * tiles: a cut last segment costs what it holds, not what seg allows
    int64_t blocks = (items + WAVES - 1) / WAVES;
    if (blocks > WAVES_PER_SIMD * static_cast<int64_t>(cus)) blocks = WAVES_PER_SIMD * static_cast<int64_t>(cus);     // all resident
    a.share = items / (blocks * WAVES);
    a.rem = items % (blocks * WAVES);

    a.bank = static_cast<const float*>(bank_dev);
    a.in = in; a.ld = ld; a.N = N; a.env_offset = env_offset; a.q_ld = q_ld;
    a.epsilon = epsilon; a.epsilon_dev = epsilon_dev; a.seed = seed; a.tick = tick; a.tick_base = tick_base_dev;
    a.action = action; a.q = q; a.q_taken = q_taken;
    const dim3 grid(static_cast<unsigned>(blocks)), block(BLOCK);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool raw = in_is_normalised == 0, eps = epsilon_dev != nullptr || epsilon > 0.0f;
    if (raw && eps) hipLaunchKernelGGL((qbank_kernel<true, true>), grid, block, 0, s, a);
    else if (raw) hipLaunchKernelGGL((qbank_kernel<true, false>), grid, block, 0, s, a);
    else if (eps) hipLaunchKernelGGL((qbank_kernel<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((qbank_kernel<false, false>), grid, block, 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "qbank_kernel launch");
    return 0;
}

}  // extern "C"
