// aqua_policy.hip -- libaqua_policy.so (include/aqua_policy.h): the DQN's 5 -> 64 -> 64 -> 3 ReLU Q-network
// (main/impl/dqn.py:301-314) evaluated for a batch of worlds on gfx950, greedy or epsilon-greedy (dqn.py:212-228).
// Its own translation unit and library: libaqua_hip.so and its kernels are not touched by it.
//
// The network itself -- the blob's layout, the forward pass of a tile on v_mfma_f32_32x32x2_f32, the pick and its stores --
// is stated in aqua_qnet.hpp, once for this library and libaqua_bank.so.  Here: one network for the whole batch, its LDS
// part copied once per block, its A operands loaded once per wavefront, and a grid-stride loop over the tiles.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/aqua_policy.h"
#include "aqua_device.hpp"
#include "aqua_host.hpp"
#include "aqua_qnet.hpp"

namespace {

using namespace aqua::qnet;

static_assert(STREAM_POLICY == AQUAPOL_STREAM, "aqua_policy.h names the stream of the policy draws");
static_assert(IN == AQUAPOL_INPUTS && HID == AQUAPOL_HIDDEN && ACT == AQUAPOL_ACTIONS, "aqua_policy.h names the network's sizes");
constexpr int BLOCK = 256, WAVES = BLOCK / 64;
constexpr int WAVES_PER_SIMD = 3;        // resident wavefronts per SIMD = blocks per CU (<= 170 registers each): while one wavefront
                                         // is in its VALU phases (layer 3, arg-max, stores) the others keep the matrix pipe busy

struct PolicyArgs {
    const float* blob;
    const float* in;
    int64_t ld, N, env_offset, q_ld;
    float epsilon;
    uint64_t seed, tick;
    const uint64_t* tick_base;
    uint8_t* action;
    float* q;
    float* q_taken;
};

// RAW: `in` holds the environment's state rows and is normalised here; EPS: epsilon-greedy (one Philox draw per world)
template <bool RAW, bool EPS>
__global__ __launch_bounds__(BLOCK, WAVES_PER_SIMD) void qpolicy_kernel(const PolicyArgs a)
{
    __shared__ float4 lds4[LDS_FLOATS / 4];
    const float4* const blob4 = reinterpret_cast<const float4*>(a.blob + OFF_LDS);
    for (int i = threadIdx.x; i < LDS_FLOATS / 4; i += BLOCK) lds4[i] = blob4[i];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, col = lane & 31;

    // the weights stay in registers across the tiles of this wavefront (70 VGPRs)
    float w1[K1_STEPS][2], w2[2][K2_STEPS];
    load_operands(a.blob, lane, w1, w2);
    __syncthreads();

    uint64_t tick = a.tick;
    if constexpr (EPS) {
        if (a.tick_base != nullptr) tick += *a.tick_base;
    }

    const int64_t tiles = (a.N + TILE - 1) / TILE;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * WAVES;
    for (int64_t t = static_cast<int64_t>(blockIdx.x) * WAVES + wave; t < tiles; t += stride) {
        const int64_t i = t * TILE + col;
        const bool live = i < a.N;
        // k-step s of layer 1 takes input 2 s + h of the lane's world; worlds beyond N and the padding row are zero.  (One
        // guard around the three loads: with the tile body called from aqua_qnet.hpp the compiler no longer merges three
        // guarded loads into it by itself, and each then waits in a branch of its own in front of the first MFMA)
        float x[K1_STEPS] = {0.0f, 0.0f, 0.0f};
        if (live) {
#pragma unroll
            for (int s = 0; s < K1_STEPS; ++s)
                if (2 * s + h < IN) x[s] = a.in[(2 * s + h) * a.ld + i];
        }
        float q[ACT];
        forward<RAW>(lds4, w1, w2, x, h, q);
        if (h == 0 && live)
            pick_and_store<EPS>(q[0], q[1], q[2], a.epsilon, a.seed, static_cast<uint64_t>(a.env_offset + i), tick, i, a.action, a.q, a.q_ld, a.q_taken);
    }
}

}  // namespace

extern "C" {

int aquapol_version(void) { return AQUAPOL_ABI_VERSION; }
const char* aquapol_last_error(void) { return g_err; }
size_t aquapol_weights_bytes(void) { return sizeof(float) * BLOB_FLOATS; }

int aquapol_pack_weights(const float* k0, const float* b0, const float* k1, const float* b1, const float* k2,
                         const float* b2, const int* shapes, void* blob_host, size_t blob_bytes)
{
    if (shapes == nullptr) return fail(AQUAPOL_E_INVALID, "shapes is NULL");
    if (shapes[0] != IN || shapes[1] != HID || shapes[2] != HID || shapes[3] != ACT)
        return fail(AQUAPOL_E_INVALID, "network %d-%d-%d-%d: only %d-%d-%d-%d (main/impl/dqn.py:301-314) is supported", shapes[0],
                    shapes[1], shapes[2], shapes[3], IN, HID, HID, ACT);
    if (k0 == nullptr || b0 == nullptr || k1 == nullptr || b1 == nullptr || k2 == nullptr || b2 == nullptr)
        return fail(AQUAPOL_E_INVALID, "a kernel or bias pointer is NULL");
    if (blob_host == nullptr) return fail(AQUAPOL_E_INVALID, "blob is NULL");
    if (blob_bytes < aquapol_weights_bytes())
        return fail(AQUAPOL_E_INVALID, "blob too small: %zu < %zu bytes", blob_bytes, aquapol_weights_bytes());
    if (!aligned(blob_host, 4)) return fail(AQUAPOL_E_ALIGN, "blob must be 4-byte aligned");
    float* const w = static_cast<float*>(blob_host);
    const float* const src[6] = {k0, b0, k1, b1, k2, b2};
    std::memset(w, 0, aquapol_weights_bytes());
    for_each_parameter([&](int b, int a, int i) { w[b] = src[a][i]; });
    return 0;
}

int aquapol_act_f32(const void* weights_dev, const float* in, int64_t ld, int in_is_normalised, int64_t N,
                    int64_t env_offset, float epsilon, uint64_t seed, uint64_t tick, const uint64_t* tick_base_dev,
                    uint8_t* action, float* q, int64_t q_ld, float* q_taken, void* stream)
{
    if (weights_dev == nullptr) return fail(AQUAPOL_E_INVALID, "weights is NULL");
    if (!aligned(weights_dev, 16)) return fail(AQUAPOL_E_ALIGN, "the weight blob must be 16-byte aligned");
    if (N < 0 || ld < N) return fail(AQUAPOL_E_INVALID, "bad sizes: N=%lld ld=%lld", (long long)N, (long long)ld);
    if (env_offset < 0) return fail(AQUAPOL_E_INVALID, "env_offset < 0");
    if (!(epsilon >= 0.0f)) return fail(AQUAPOL_E_INVALID, "epsilon=%g: must be >= 0", (double)epsilon);
    if (action == nullptr && q == nullptr && q_taken == nullptr) return fail(AQUAPOL_E_INVALID, "action, q and q_taken are all NULL");
    if (q != nullptr && q_ld < N) return fail(AQUAPOL_E_INVALID, "q_ld=%lld < N=%lld", (long long)q_ld, (long long)N);
    if (N > 0 && in == nullptr) return fail(AQUAPOL_E_INVALID, "in is NULL");
    if (!aligned(in, 4) || !aligned(q, 4) || !aligned(q_taken, 4)) return fail(AQUAPOL_E_ALIGN, "in / q / q_taken must be 4-byte aligned");
    if (!aligned(tick_base_dev, 8)) return fail(AQUAPOL_E_ALIGN, "tick_base_dev must be 8-byte aligned");
    if (N == 0) return 0;

    int cus = 0;
    if (const int rc = compute_units(&cus, AQUAPOL_E_NODEVICE)) return rc;
    const int64_t tiles = (N + TILE - 1) / TILE;
    int64_t blocks = (tiles + WAVES - 1) / WAVES;
    if (blocks > WAVES_PER_SIMD * static_cast<int64_t>(cus)) blocks = WAVES_PER_SIMD * static_cast<int64_t>(cus);     // all resident

    PolicyArgs a;
    a.blob = static_cast<const float*>(weights_dev);
    a.in = in; a.ld = ld; a.N = N; a.env_offset = env_offset; a.q_ld = q_ld;
    a.epsilon = epsilon; a.seed = seed; a.tick = tick; a.tick_base = tick_base_dev;
    a.action = action; a.q = q; a.q_taken = q_taken;
    const dim3 grid(static_cast<unsigned>(blocks)), block(BLOCK);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool raw = in_is_normalised == 0, eps = epsilon > 0.0f;
    if (raw && eps) hipLaunchKernelGGL((qpolicy_kernel<true, true>), grid, block, 0, s, a);
    else if (raw) hipLaunchKernelGGL((qpolicy_kernel<true, false>), grid, block, 0, s, a);
    else if (eps) hipLaunchKernelGGL((qpolicy_kernel<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((qpolicy_kernel<false, false>), grid, block, 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "qpolicy_kernel launch");
    return 0;
}

}  // extern "C"
