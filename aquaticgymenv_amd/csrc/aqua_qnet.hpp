// aqua_qnet.hpp -- what the translation units around the DQN's 5 -> 64 -> 64 -> 3 Q-network (main/impl/dqn.py:301-314)
// share: the Philox streams of the policy and the learner, the random action of the epsilon-greedy pick, the geometry of
// the network on v_mfma_f32_32x32x2_f32, and the ACTING network as libaqua_policy.so and libaqua_bank.so evaluate it: the
// device blob's layout with its host-side index map, the float32 forward pass of one tile, and the epsilon-greedy pick
// with its stores.  The learner's forward passes are not here: their last layer is in double and their operands come
// from the canonical parameter vector, by design.
//
// Layout of the acting pass (DESIGN.md "Q-network on the device").  v_mfma_f32_32x32x2_f32 computes
// D[i][j] += A[i][k] B[k][j], k = 0, 1, with lane l holding A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31], and
// D[i][j] in register r of lane l with j = l & 31, i = (r & 3) + 8 (r >> 2) + 4 (l >> 5).  WORLDS sit on the column index j
// (one tile = 32 worlds per wavefront), UNITS on the row index i (64 units = two 16-register accumulators).  A layer's
// output is then, register by register, the B operand of the next layer: k-step (M, r) of the 64 x 64 layer feeds each
// lane its own accumulator register r of block M (after bias and ReLU) -- that is unit 32 M + (r & 3) + 8 (r >> 2) + 4 h
// for lane half h -- and the packer puts the weight of exactly that unit into the A operand of that lane half.  No LDS
// round trip, no lane movement, and the activations never leave the registers.
//
// Numerics: float32, every unit one fmaf chain from its bias (the MFMA is bit for bit a k-ordered fmaf chain); the three
// outputs are two 32-term fmaf chains (one per lane half, the first starting at the bias) added once.
#pragma once
#include <atomic>

#include "aqua_device.hpp"
#include "aqua_host.hpp"

namespace aqua {
namespace qnet {

// ---- Philox streams (aqua_device.hpp: 0, 1, 3, 4 are the environment's)
constexpr uint32_t STREAM_POLICY = 5;    // epsilon-greedy draws of the policy kernel, and of the exploration pass that reproduces them
constexpr uint32_t STREAM_LEARNER = 6;   // minibatch draws
static_assert(STREAM_POLICY != STREAM_LEARNER && STREAM_POLICY != STREAM_STEP && STREAM_POLICY != STREAM_PLACE &&
              STREAM_POLICY != STREAM_POSE && STREAM_POLICY != STREAM_ACT && STREAM_LEARNER != STREAM_STEP &&
              STREAM_LEARNER != STREAM_PLACE && STREAM_LEARNER != STREAM_POSE && STREAM_LEARNER != STREAM_ACT,
              "the policy and minibatch draws need streams of their own");

// ---- the network
constexpr int IN = 5, HID = 64, ACT = 3;
constexpr int TILE = 32;                 // worlds (samples) per wavefront and pass: the MFMA's column count

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the unit (row of the accumulator tile) that register r of row block M holds on lane half h
__host__ __device__ constexpr int unit_of(int M, int r, int h) { return 32 * M + (r & 3) + 8 * (r >> 2) + 4 * h; }

// ---- the random action of an epsilon-greedy pick, from the words r of the world's draw; it is taken when u_01(r[0]) < epsilon
__device__ __forceinline__ uint32_t random_action(const uint32_t (&r)[4]) { return ((r[1] >> 8) * static_cast<uint32_t>(ACT)) >> 24; }

// ---- the acting network's device blob (aquapol_pack_weights() writes it; one slot of a bank is one blob), in floats
constexpr int K1_STEPS = 3;              // layer 1: K = 5 padded to 6 (the sixth weight and input are zero)
constexpr int K2_STEPS = HID / 2;        // layer 2: 32 k-steps of 2 for each of the two row blocks

// W1 / W2: the A operands, one float per lane and (k-step, row block).  The rest is what a kernel keeps in LDS, in the
// order a lane half reads it: biases of the hidden layers as the accumulators' initial values, the output layer's weights
// per action, its bias.
constexpr int OFF_W1 = 0;                                   // [K1_STEPS][2][64]
constexpr int OFF_W2 = OFF_W1 + K1_STEPS * 2 * 64;          // [2][K2_STEPS][64]
constexpr int OFF_LDS = OFF_W2 + 2 * K2_STEPS * 64;
constexpr int LDS_B0 = 0;                                   // [2 halves][32]
constexpr int LDS_B1 = LDS_B0 + 64;                         // [2 halves][32]
constexpr int LDS_K2 = LDS_B1 + 64;                         // [2 halves][ACT][32]
constexpr int LDS_B2 = LDS_K2 + 2 * ACT * 32;               // [ACT] + 1 pad
constexpr int LDS_FLOATS = LDS_B2 + 4;
constexpr int BLOB_FLOATS = OFF_LDS + LDS_FLOATS;
static_assert(OFF_LDS % 4 == 0 && LDS_FLOATS % 4 == 0 && BLOB_FLOATS % 4 == 0, "the LDS part is copied as float4 and every slot of a bank stays 16-byte aligned");

// The blob's index map, host side: visit(b, a, i) for every float b of the blob that holds a parameter, which is element
// i of canonical array a (0 .. 5: k0 [IN][HID], b0 [HID], k1 [HID][HID], b1 [HID], k2 [HID][ACT], b2 [ACT]).  Every parameter
// is visited once; the floats not visited are padding (the packer zeroes them, nothing reads them as parameters).
template <class Visit>
static void for_each_parameter(Visit visit)
{
    for (int lane = 0; lane < 64; ++lane) {
        const int h = lane >> 5, i = lane & 31;
        for (int s = 0; s < K1_STEPS; ++s)
            for (int M = 0; M < 2; ++M) {
                const int k = 2 * s + h;                                  // input of this k-step and lane half
                if (k < IN) visit(OFF_W1 + (s * 2 + M) * 64 + lane, 0, k * HID + 32 * M + i);
            }
        for (int M2 = 0; M2 < 2; ++M2)                                    // row block of the OUTPUT unit 32 M2 + i
            for (int M = 0; M < 2; ++M)
                for (int r = 0; r < 16; ++r)                              // k-step: the input unit register r of block M holds
                    visit(OFF_W2 + (M2 * K2_STEPS + M * 16 + r) * 64 + lane, 2, unit_of(M, r, h) * HID + 32 * M2 + i);
    }
    for (int h = 0; h < 2; ++h)
        for (int M = 0; M < 2; ++M)
            for (int r = 0; r < 16; ++r) {
                const int u = unit_of(M, r, h);
                visit(OFF_LDS + LDS_B0 + h * 32 + M * 16 + r, 1, u);
                visit(OFF_LDS + LDS_B1 + h * 32 + M * 16 + r, 3, u);
                for (int c = 0; c < ACT; ++c) visit(OFF_LDS + LDS_K2 + (h * ACT + c) * 32 + M * 16 + r, 4, u * ACT + c);
            }
    for (int c = 0; c < ACT; ++c) visit(OFF_LDS + LDS_B2 + c, 5, c);
}

// ---- the acting pass on the device
// the A operands of a lane, from a blob: they stay in registers while the wavefront stays with the network (70 VGPRs)
__device__ __forceinline__ void load_operands(const float* blob, int lane, float (&w1)[K1_STEPS][2], float (&w2)[2][K2_STEPS])
{
#pragma unroll
    for (int s = 0; s < K1_STEPS; ++s)
#pragma unroll
        for (int M = 0; M < 2; ++M) w1[s][M] = blob[OFF_W1 + (s * 2 + M) * 64 + lane];
#pragma unroll
    for (int M = 0; M < 2; ++M)
#pragma unroll
        for (int st = 0; st < K2_STEPS; ++st) w2[M][st] = blob[OFF_W2 + (M * K2_STEPS + st) * 64 + lane];
}

// One tile of 32 worlds through the network.  lds4: the blob's LDS part as the wavefront sees it; in[s]: input 2 s + h of
// the lane's world (0 on the padding row and for a world that does not exist), RAW: as the environment's state row holds
// it, normalised here; h: the lane's half.  q: the three Q-values of the lane's world, the same bits on both halves.
template <bool RAW>
__device__ __forceinline__ void forward(const float4* lds4, const float (&w1)[K1_STEPS][2], const float (&w2)[2][K2_STEPS],
                                        const float (&in)[K1_STEPS], int h, float (&q)[ACT])
{
#pragma clang fp contract(off)
    const float* const lds = reinterpret_cast<const float*>(lds4);
    float x[K1_STEPS];
#pragma unroll
    for (int s = 0; s < K1_STEPS; ++s) {
        x[s] = in[s];
        // AquaStateNormalizer as the step kernels' epilogue writes it: a rounded float32 before the layer sees it
        // (0 stays 0 on the padding row and on worlds that do not exist, except for the angle's 0.5 which meets a zero weight or no store)
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
#pragma unroll
    for (int c = 0; c < ACT; ++c) q[c] = p[c] + __shfl_xor(p[c], 32);      // the same bits on both halves
}

// The pick for world i of the batch (one lane per world) and the stores a caller asked for.  EPS: epsilon-greedy with
// threshold eps, one Philox draw per world at (seed, world, tick) on STREAM_POLICY.
template <bool EPS>
__device__ __forceinline__ void pick_and_store(float q0, float q1, float q2, float eps, uint64_t seed, uint64_t world, uint64_t tick,
                                               int64_t i, uint8_t* action, float* q, int64_t q_ld, float* q_taken)
{
    int act = 0;                                      // np.argmax: the lowest index on a tie
    float best = q0;
    if (q1 > best) { act = 1; best = q1; }
    if (q2 > best) { act = 2; best = q2; }
    if constexpr (EPS) {
        uint32_t r[4];
        draw(seed, world, tick, STREAM_POLICY, 0, r);
        if (u_01(r[0]) < eps) act = static_cast<int>(random_action(r));
    }
    if (action != nullptr) action[i] = static_cast<uint8_t>(act);
    if (q != nullptr) {
        const float qs[ACT] = {q0, q1, q2};
#pragma unroll
        for (int c = 0; c < ACT; ++c) q[c * q_ld + i] = qs[c];
    }
    if (q_taken != nullptr) q_taken[i] = act == 0 ? q0 : (act == 1 ? q1 : q2);
}

// ---- host side
// compute units of the current device, asked once per device (an attribute query is no stream operation: legal under capture)
static int compute_units(int* out, int nodevice_code)
{
    constexpr int MAX_DEVICES = 64;
    static std::atomic<int> cached[MAX_DEVICES];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(nodevice_code, "no HIP device: %s", hipGetErrorString(e));
    }
    int cus = (dev >= 0 && dev < MAX_DEVICES) ? cached[dev].load(std::memory_order_relaxed) : 0;
    if (cus <= 0) {
        e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess) return hip_fail(e, "hipDeviceGetAttribute");
        if (cus <= 0) cus = 1;
        if (dev >= 0 && dev < MAX_DEVICES) cached[dev].store(cus, std::memory_order_relaxed);
    }
    *out = cus;
    return 0;
}

}  // namespace qnet
}  // namespace aqua
