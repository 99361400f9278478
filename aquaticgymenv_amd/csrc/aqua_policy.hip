// aqua_policy.hip -- libaqua_policy.so (include/aqua_policy.h): the DQN's 5 -> 64 -> 64 -> 3 ReLU Q-network
// (main/impl/dqn.py:301-314) evaluated for a batch of worlds on gfx950, greedy or epsilon-greedy (dqn.py:212-228).
// Its own translation unit and library: libaqua_hip.so and its kernels are not touched by it.
//
// Layout (DESIGN.md "Q-network on the device").  v_mfma_f32_32x32x2_f32 computes D[i][j] += A[i][k] B[k][j], k = 0, 1,
// with lane l holding A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31], and D[i][j] in register r of lane l with
// j = l & 31, i = (r & 3) + 8 (r >> 2) + 4 (l >> 5).  WORLDS sit on the column index j (one tile = 32 worlds per
// wavefront), UNITS on the row index i (64 units = two 16-register accumulators).  A layer's output is then, register
// by register, the B operand of the next layer: k-step (M, r) of the 64 x 64 layer feeds each lane its own accumulator
// register r of block M (after bias and ReLU) -- that is unit 32 M + (r & 3) + 8 (r >> 2) + 4 h for lane half h -- and
// the host packer puts the weight of exactly that unit into the A operand of that lane half.  No LDS round trip, no lane
// movement, and the activations never leave the registers.
//
// Numerics: float32, every unit one fmaf chain from its bias (the MFMA is bit for bit a k-ordered fmaf chain); the three
// outputs are two 32-term fmaf chains (one per lane half, the first starting at the bias) added once.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>

#include "../../include/aqua_policy.h"
#include "aqua_device.hpp"
#include "aqua_host.hpp"
#include "aqua_qnet.hpp"

namespace {

using aqua::draw;
using aqua::u_01;
using namespace aqua::qnet;

static_assert(STREAM_POLICY == AQUAPOL_STREAM, "aqua_policy.h names the stream of the policy draws");
static_assert(IN == AQUAPOL_INPUTS && HID == AQUAPOL_HIDDEN && ACT == AQUAPOL_ACTIONS, "aqua_policy.h names the network's sizes");
constexpr int K1_STEPS = 3;              // layer 1: K = 5 padded to 6 (the sixth weight and input are zero)
constexpr int K2_STEPS = HID / 2;        // layer 2: 32 k-steps of 2 for each of the two row blocks
constexpr int BLOCK = 256, WAVES = BLOCK / 64;
constexpr int WAVES_PER_SIMD = 3;        // resident wavefronts per SIMD = blocks per CU (<= 170 registers each): while one wavefront
                                         // is in its VALU phases (layer 3, arg-max, stores) the others keep the matrix pipe busy

// Device-format blob, in floats.  W1 / W2: the A operands, one float per lane and (k-step, row block).  The rest is
// what the kernel keeps in LDS, in the order a lane half reads it: biases of the hidden layers as the accumulators'
// initial values, the output layer's weights per action, its bias.
constexpr int OFF_W1 = 0;                                   // [K1_STEPS][2][64]
constexpr int OFF_W2 = OFF_W1 + K1_STEPS * 2 * 64;          // [2][K2_STEPS][64]
constexpr int OFF_LDS = OFF_W2 + 2 * K2_STEPS * 64;
constexpr int LDS_B0 = 0;                                   // [2 halves][32]
constexpr int LDS_B1 = LDS_B0 + 64;                         // [2 halves][32]
constexpr int LDS_K2 = LDS_B1 + 64;                         // [2 halves][ACT][32]
constexpr int LDS_B2 = LDS_K2 + 2 * ACT * 32;               // [ACT] + 1 pad
constexpr int LDS_FLOATS = LDS_B2 + 4;
constexpr int BLOB_FLOATS = OFF_LDS + LDS_FLOATS;
static_assert(OFF_LDS % 4 == 0 && LDS_FLOATS % 4 == 0, "the LDS part is copied as float4");

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
#pragma clang fp contract(off)
    __shared__ float4 lds4[LDS_FLOATS / 4];
    const float4* const blob4 = reinterpret_cast<const float4*>(a.blob + OFF_LDS);
    for (int i = threadIdx.x; i < LDS_FLOATS / 4; i += BLOCK) lds4[i] = blob4[i];
    const float* const lds = reinterpret_cast<const float*>(lds4);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, col = lane & 31;

    // the weights stay in registers across the tiles of this wavefront (70 VGPRs)
    float w1[K1_STEPS][2], w2[2][K2_STEPS];
#pragma unroll
    for (int s = 0; s < K1_STEPS; ++s)
#pragma unroll
        for (int M = 0; M < 2; ++M) w1[s][M] = a.blob[OFF_W1 + (s * 2 + M) * 64 + lane];
#pragma unroll
    for (int M = 0; M < 2; ++M)
#pragma unroll
        for (int st = 0; st < K2_STEPS; ++st) w2[M][st] = a.blob[OFF_W2 + (M * K2_STEPS + st) * 64 + lane];
    __syncthreads();

    uint64_t tick = a.tick;
    if constexpr (EPS) {
        if (a.tick_base != nullptr) tick += *a.tick_base;
    }

    // k-step s of layer 1 takes input 2 s + h of the lane's world; worlds beyond N and the padding row are zero
    const auto load_inputs = [&](int64_t tile, float (&x)[K1_STEPS]) {
        const int64_t i = tile * TILE + col;
#pragma unroll
        for (int s = 0; s < K1_STEPS; ++s) {
            const int row = 2 * s + h;
            x[s] = (i < a.N && row < IN) ? a.in[row * a.ld + i] : 0.0f;
        }
    };

    const int64_t tiles = (a.N + TILE - 1) / TILE;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * WAVES;
    for (int64_t t = static_cast<int64_t>(blockIdx.x) * WAVES + wave; t < tiles; t += stride) {
        const int64_t i = t * TILE + col;
        const bool live = i < a.N;
        float x[K1_STEPS];
        load_inputs(t, x);
#pragma unroll
        for (int s = 0; s < K1_STEPS; ++s) {
            // AquaStateNormalizer as the step kernels' epilogue writes it: a rounded float32 before the layer sees it
            // (0 stays 0 on the padding row and beyond N, except for the angle's 0.5 which meets a zero weight or no store)
            if constexpr (RAW) x[s] = (2 * s + h == 2) ? fmaf(x[s], 0.15915494309189535f, 0.5f) : x[s] * 0.01f;
        }
        __builtin_amdgcn_sched_barrier(0);

        f32x16 h1[2], h2[2];
#pragma unroll
        for (int M = 0; M < 2; ++M)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 b0 = lds4[(LDS_B0 + h * 32 + M * 16) / 4 + g], b1 = lds4[(LDS_B1 + h * 32 + M * 16) / 4 + g];
                h1[M][4 * g + 0] = b0.x; h1[M][4 * g + 1] = b0.y; h1[M][4 * g + 2] = b0.z; h1[M][4 * g + 3] = b0.w;
                h2[M][4 * g + 0] = b1.x; h2[M][4 * g + 1] = b1.y; h2[M][4 * g + 2] = b1.z; h2[M][4 * g + 3] = b1.w;
            }

        // (scheduling fences in front of the two MFMA layers: without them the LDS reads of all three layers are hoisted to the
        // top of the tile and the kernel spills; with them it fits the 170 registers of three wavefronts per SIMD.  None in
        // front of layer 3: its VALU work on the first row block then runs under the second block's MFMAs)
        __builtin_amdgcn_sched_barrier(0);
        // layer 1: 64 x 5
#pragma unroll
        for (int s = 0; s < K1_STEPS; ++s)
#pragma unroll
            for (int M = 0; M < 2; ++M) h1[M] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[s][M], x[s], h1[M], 0, 0, 0);

        __builtin_amdgcn_sched_barrier(0);
        // layer 2: 64 x 64.  k-step (M, r): B is this lane's own h1[M][r]
#pragma unroll
        for (int M = 0; M < 2; ++M)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float b = fmaxf(h1[M][r], 0.0f);
                h2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2[0][M * 16 + r], b, h2[0], 0, 0, 0);
                h2[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2[1][M * 16 + r], b, h2[1], 0, 0, 0);
            }

        // layer 3: 3 x 64 on the VALU from the 32 units this lane holds, then one add across the lane halves
        float p[ACT];
#pragma unroll
        for (int c = 0; c < ACT; ++c) p[c] = h == 0 ? lds[LDS_B2 + c] : 0.0f;
#pragma unroll
        for (int M = 0; M < 2; ++M)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float v0 = fmaxf(h2[M][4 * g + 0], 0.0f), v1 = fmaxf(h2[M][4 * g + 1], 0.0f);
                const float v2 = fmaxf(h2[M][4 * g + 2], 0.0f), v3 = fmaxf(h2[M][4 * g + 3], 0.0f);
#pragma unroll
                for (int c = 0; c < ACT; ++c) {
                    const float4 k = lds4[(LDS_K2 + (h * ACT + c) * 32 + M * 16) / 4 + g];
                    p[c] = fmaf(k.x, v0, p[c]);
                    p[c] = fmaf(k.y, v1, p[c]);
                    p[c] = fmaf(k.z, v2, p[c]);
                    p[c] = fmaf(k.w, v3, p[c]);
                }
            }
        float q[ACT];
#pragma unroll
        for (int c = 0; c < ACT; ++c) q[c] = p[c] + __shfl_xor(p[c], 32);      // the same bits on both halves

        if (h == 0 && live) {
            int act = 0;                                      // np.argmax: the lowest index on a tie
            float best = q[0];
            if (q[1] > best) { act = 1; best = q[1]; }
            if (q[2] > best) { act = 2; best = q[2]; }
            if constexpr (EPS) {
                uint32_t r[4];
                draw(a.seed, static_cast<uint64_t>(a.env_offset + i), tick, STREAM_POLICY, 0, r);
                if (u_01(r[0]) < a.epsilon) act = static_cast<int>(random_action(r));
            }
            if (a.action != nullptr) a.action[i] = static_cast<uint8_t>(act);
            if (a.q != nullptr) {
#pragma unroll
                for (int c = 0; c < ACT; ++c) a.q[c * a.q_ld + i] = q[c];
            }
            if (a.q_taken != nullptr) a.q_taken[i] = act == 0 ? q[0] : (act == 1 ? q[1] : q[2]);
        }
    }
}

// ------------------------------------------------------------------ host side
// compute units of a device, asked once (an attribute query is no stream operation: legal under capture)
constexpr int MAX_DEVICES = 64;
std::atomic<int> g_cus[MAX_DEVICES];

int compute_units(int* out)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(AQUAPOL_E_NODEVICE, "no HIP device: %s", hipGetErrorString(e));
    }
    int cus = (dev >= 0 && dev < MAX_DEVICES) ? g_cus[dev].load(std::memory_order_relaxed) : 0;
    if (cus <= 0) {
        e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess) return hip_fail(e, "hipDeviceGetAttribute");
        if (cus <= 0) cus = 1;
        if (dev >= 0 && dev < MAX_DEVICES) g_cus[dev].store(cus, std::memory_order_relaxed);
    }
    *out = cus;
    return 0;
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
    std::memset(w, 0, aquapol_weights_bytes());
    for (int lane = 0; lane < 64; ++lane) {
        const int h = lane >> 5, i = lane & 31;
        for (int s = 0; s < K1_STEPS; ++s)
            for (int M = 0; M < 2; ++M) {
                const int k = 2 * s + h;                                  // input of this k-step and lane half
                w[OFF_W1 + (s * 2 + M) * 64 + lane] = k < IN ? k0[k * HID + 32 * M + i] : 0.0f;
            }
        for (int M2 = 0; M2 < 2; ++M2)                                    // row block of the OUTPUT unit 32 M2 + i
            for (int M = 0; M < 2; ++M)
                for (int r = 0; r < 16; ++r)                              // k-step: the input unit register r of block M holds
                    w[OFF_W2 + (M2 * K2_STEPS + M * 16 + r) * 64 + lane] = k1[unit_of(M, r, h) * HID + 32 * M2 + i];
    }
    float* const l = w + OFF_LDS;
    for (int h = 0; h < 2; ++h)
        for (int M = 0; M < 2; ++M)
            for (int r = 0; r < 16; ++r) {
                const int u = unit_of(M, r, h);
                l[LDS_B0 + h * 32 + M * 16 + r] = b0[u];
                l[LDS_B1 + h * 32 + M * 16 + r] = b1[u];
                for (int c = 0; c < ACT; ++c) l[LDS_K2 + (h * ACT + c) * 32 + M * 16 + r] = k2[u * ACT + c];
            }
    for (int c = 0; c < ACT; ++c) l[LDS_B2 + c] = b2[c];
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
    if (const int rc = compute_units(&cus)) return rc;
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
