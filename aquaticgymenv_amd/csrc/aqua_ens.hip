// aqua_ens.hip -- libaqua_ens.so (aqua_ens.h): the ensemble policy of a bank of the DQN's 5 -> 64 -> 64 -> 3 Q-networks
// (main/impl/dqn.py:301-314) on gfx950: every member network of the bank evaluates every world of the batch, and the
// answers are reduced to one action per world (mean of Q or majority vote), with the across-network variance and the
// vote counts, in one launch.  Its own translation unit and library: libaqua_policy.so and libaqua_bank.so, whose
// per-network Q-values this one reproduces bit for bit, are not touched by it.
//
// The network itself -- the blob's layout (one slot of the bank is one blob), the forward pass of a tile, the pick and
// its stores -- is stated in aqua_qnet.hpp.  Here: the loop order.  A member's A operands are per
// wavefront (70 VGPRs, 19.2 KB), so the loop is MEMBER-OUTER: a wavefront owns a group of GROUP consecutive tiles of 32
// worlds, keeps their inputs and their accumulators in registers, and for every member loads the operands and its own
// copy of the LDS part once and runs the GROUP tiles through forward().  The accumulators of a world are split over the
// two lanes that hold it: the lane of half 0 sums Q, the lane of half 1 sums Q^2 (both get the same bits of Q from
// forward()), and lane half h counts the members whose arg-max is h; the votes for action 2 are M minus the two counts.
#include <hip/hip_runtime.h>

#include <cmath>

#include "aqua_ens.h"
#include "aqua_device.hpp"
#include "aqua_host.hpp"
#include "aqua_qnet.hpp"

namespace aqua_ens {

using namespace aqua;
using namespace aqua::qnet;

static_assert(STREAM_POLICY == AQUAENS_STREAM, "aqua_ens.h names the stream of the policy draws");
static_assert(ACT == AQUAENS_ACTIONS, "aqua_ens.h names the number of actions");
constexpr int BLOCK = 256, WAVES = BLOCK / 64;
constexpr int WAVES_PER_SIMD = 2;        // resident wavefronts per SIMD = blocks per CU (<= 256 registers each)
constexpr int GROUP = AQUAENS_GROUP;     // tiles a wavefront carries through the member loop
constexpr int64_t GROUP_WORLDS = static_cast<int64_t>(GROUP) * TILE;

struct EnsArgs {
    const float* bank;
    const uint8_t* member;
    const float* in;
    const float* epsilon_dev;
    int networks, mode;
    int64_t groups;
    int64_t ld, N, env_offset, q_ld, x_ld;
    float epsilon;
    uint64_t seed, tick;
    const uint64_t* tick_base;
    uint8_t* action;
    float* q;
    float* q_taken;
    float* variance;
    int32_t* votes;
};

// what other lanes of this wavefront wrote to (or still read from) its LDS copy is complete before anything behind this
// point (the bank kernel's pattern: the copy belongs to the wavefront, so no workgroup barrier)
__device__ __forceinline__ void wave_sync_lds()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// One member's Q of one world into the lane's accumulators.  Sequential double adds, nothing contracted: the lane of half 0
// adds double(q), the lane of half 1 the exact double product double(q) * double(q).
__device__ __forceinline__ void accumulate(const float (&q)[ACT], int h, double (&acc)[ACT], uint32_t& count)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < ACT; ++c) {
        const double d = static_cast<double>(q[c]);
        const double sq = d * d;
        acc[c] = acc[c] + (h != 0 ? sq : d);
    }
    int best = 0;                                     // the member's own arg-max: the lowest index on a tie
    float top = q[0];
    if (q[1] > top) { best = 1; top = q[1]; }
    if (q[2] > top) best = 2;
    count += best == h ? 1u : 0u;
}

// the statistics of a world from its sums: Qbar and the population variance, rounded once each
__device__ __forceinline__ void finish(const double (&s1)[ACT], const double (&s2)[ACT], uint32_t members, float (&qbar)[ACT], float (&var)[ACT])
{
#pragma clang fp contract(off)
    const double m = static_cast<double>(members);
#pragma unroll
    for (int c = 0; c < ACT; ++c) {
        if (members == 0) {
            qbar[c] = 0.0f;
            var[c] = 0.0f;
        } else {
            const double mean = s1[c] / m;
            const double second = s2[c] / m;
            const double square = mean * mean;
            const double v = second - square;
            qbar[c] = static_cast<float>(mean);
            var[c] = static_cast<float>(v > 0.0 ? v : 0.0);
        }
    }
}

// RAW: `in` holds the environment's state rows and is normalised in forward(); EPS: epsilon-greedy (one Philox draw per world)
template <bool RAW, bool EPS>
__global__ __launch_bounds__(BLOCK, WAVES_PER_SIMD) void qens_kernel(const EnsArgs a)
{
    // a copy of the LDS part per wavefront: the wavefronts of a block walk the members at their own pace
    __shared__ float4 lds_all[WAVES][LDS_FLOATS / 4];

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, col = lane & 31;
    float4* const lds4 = lds_all[wave];

    uint64_t tick = a.tick;
    float eps = a.epsilon;
    if constexpr (EPS) {
        if (a.tick_base != nullptr) tick += *a.tick_base;
        if (a.epsilon_dev != nullptr) {
            // by its bits (the library is built with -fno-honor-nans): NaN, and every negative value, never explore
            const uint32_t bits = __float_as_uint(*a.epsilon_dev);
            eps = bits > 0x7F800000u ? 0.0f : __uint_as_float(bits);
        }
    }

    const int64_t stride = static_cast<int64_t>(gridDim.x) * WAVES;
    for (int64_t g = static_cast<int64_t>(blockIdx.x) * WAVES + wave; g < a.groups; g += stride) {
        const int64_t base = g * GROUP_WORLDS;             // the group's first world: < N

        // the inputs of the group's worlds, once: k-step s of layer 1 takes input 2 s + h of the lane's world; worlds
        // beyond N and the padding row are zero
        float x[GROUP][K1_STEPS];
        double acc[GROUP][ACT];
        uint32_t count[GROUP];
#pragma unroll
        for (int t = 0; t < GROUP; ++t) {
            const int64_t i = base + t * TILE + col;
#pragma unroll
            for (int s = 0; s < K1_STEPS; ++s) x[t][s] = 0.0f;
            if (i < a.N) {
#pragma unroll
                for (int s = 0; s < K1_STEPS; ++s)
                    if (2 * s + h < IN) x[t][s] = a.in[(2 * s + h) * a.ld + i];
            }
#pragma unroll
            for (int c = 0; c < ACT; ++c) acc[t][c] = 0.0;
            count[t] = 0;
        }

        // the members, in ascending slot order (the mask is read again for every group: aqua_ens.h asks that it does not
        // change while the launch runs)
        uint32_t members = 0;
        for (int p = 0; p < a.networks; ++p) {
            if (a.member != nullptr) {
                // wavefront-uniform: the whole wavefront skips a slot that is no member
                if (__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(a.member[p])) == 0u) continue;
            }
            ++members;
            const float* const blob = a.bank + static_cast<int64_t>(p) * BLOB_FLOATS;
            float w1[K1_STEPS][2], w2[2][K2_STEPS];
            load_operands(blob, lane, w1, w2);
            const float4* const blob4 = reinterpret_cast<const float4*>(blob + OFF_LDS);
            wave_sync_lds();                                  // the reads of the previous member's copy are done
            static_assert(LDS_FLOATS / 4 > 64 && LDS_FLOATS / 4 <= 128, "two float4 per lane cover the LDS part");
            lds4[lane] = blob4[lane];
            if (lane < LDS_FLOATS / 4 - 64) lds4[64 + lane] = blob4[64 + lane];
            wave_sync_lds();                                  // the copy is complete before any lane reads it

#pragma unroll
            for (int t = 0; t < GROUP; ++t) {
                if (base + t * TILE < a.N) {                  // wavefront-uniform: a tile without a world costs nothing
                    float q[ACT];
                    forward<RAW>(lds4, w1, w2, x[t], h, q);
                    accumulate(q, h, acc[t], count[t]);
                }
            }
        }

        // the reduction and the pick, per tile: the two lanes of a world exchange their halves
#pragma unroll
        for (int t = 0; t < GROUP; ++t) {
            if (base + t * TILE >= a.N) continue;
            const int64_t i = base + t * TILE + col;
            double s1[ACT], s2[ACT];
#pragma unroll
            for (int c = 0; c < ACT; ++c) {
                const double other = __shfl_xor(acc[t][c], 32);
                s1[c] = h == 0 ? acc[t][c] : other;
                s2[c] = h == 0 ? other : acc[t][c];
            }
            const uint32_t count_other = __shfl_xor(count[t], 32);
            uint32_t n[ACT];
            n[0] = h == 0 ? count[t] : count_other;
            n[1] = h == 0 ? count_other : count[t];
            n[2] = members - n[0] - n[1];
            float qbar[ACT], var[ACT];
            finish(s1, s2, members, qbar, var);
            if (h != 0 || i >= a.N) continue;

            if (a.variance != nullptr) {
#pragma unroll
                for (int c = 0; c < ACT; ++c) a.variance[c * a.x_ld + i] = var[c];
            }
            if (a.votes != nullptr) {
#pragma unroll
                for (int c = 0; c < ACT; ++c) a.votes[c * a.x_ld + i] = static_cast<int32_t>(n[c]);
            }
            const uint64_t world = static_cast<uint64_t>(a.env_offset + i);
            if (a.mode == AQUAENS_MEAN) {
                pick_and_store<EPS>(qbar[0], qbar[1], qbar[2], eps, a.seed, world, tick, i, a.action, a.q, a.q_ld, a.q_taken);
            } else {
                // the most votes; among equal counts the larger Qbar; still equal, the lowest index
                int act = 0;
#pragma unroll
                for (int c = 1; c < ACT; ++c)
                    if (n[c] > n[act] || (n[c] == n[act] && qbar[c] > qbar[act])) act = c;
                if constexpr (EPS) {                          // the policy's draw (pick_and_store<true>)
                    uint32_t r[4];
                    draw(a.seed, world, tick, STREAM_POLICY, 0, r);
                    if (u_01(r[0]) < eps) act = static_cast<int>(random_action(r));
                }
                if (a.action != nullptr) a.action[i] = static_cast<uint8_t>(act);
                if (a.q != nullptr) {
#pragma unroll
                    for (int c = 0; c < ACT; ++c) a.q[c * a.q_ld + i] = qbar[c];
                }
                if (a.q_taken != nullptr) a.q_taken[i] = act == 0 ? qbar[0] : (act == 1 ? qbar[1] : qbar[2]);
            }
        }
    }
}

// the launch for N >= 1 worlds on `cus` compute units: blocks, groups, the most groups of one wavefront
void launch_shape(int64_t N, int cus, int64_t (&out)[3])
{
    const int64_t groups = N / GROUP_WORLDS + (N % GROUP_WORLDS != 0 ? 1 : 0);
    int64_t blocks = (groups + WAVES - 1) / WAVES;
    if (blocks > WAVES_PER_SIMD * static_cast<int64_t>(cus)) blocks = WAVES_PER_SIMD * static_cast<int64_t>(cus);     // all resident
    out[0] = blocks;
    out[1] = groups;
    out[2] = (groups + blocks * WAVES - 1) / (blocks * WAVES);
}

}  // namespace aqua_ens

using namespace aqua_ens;

extern "C" {

int aquaens_version(void) { return AQUAENS_ABI_VERSION; }
const char* aquaens_last_error(void) { return g_err; }
size_t aquaens_weights_bytes(void) { return sizeof(float) * BLOB_FLOATS; }

int aquaens_shape(int64_t N, int cus, int64_t out[3])
{
    if (out == nullptr) return fail(AQUAENS_E_INVALID, "out is NULL");
    if (N < 0) return fail(AQUAENS_E_INVALID, "N=%lld: must be >= 0", (long long)N);
    if (cus < 1) return fail(AQUAENS_E_INVALID, "cus=%d: must be >= 1", cus);
    int64_t shape[3] = {0, 0, 0};
    if (N > 0) launch_shape(N, cus, shape);
    for (int k = 0; k < 3; ++k) out[k] = shape[k];
    return 0;
}

int aquaens_act_f32(const void* bank_dev, int64_t networks, const uint8_t* member_dev, int mode, const float* in, int64_t ld,
                    int in_is_normalised, int64_t N, int64_t env_offset, float epsilon, const float* epsilon_dev, uint64_t seed,
                    uint64_t tick, const uint64_t* tick_base_dev, uint8_t* action, float* q, int64_t q_ld, float* q_taken,
                    float* variance, int32_t* votes, int64_t x_ld, void* stream)
{
    if (bank_dev == nullptr) return fail(AQUAENS_E_INVALID, "the bank is NULL");
    if (!aligned(bank_dev, 16)) return fail(AQUAENS_E_ALIGN, "the bank must be 16-byte aligned");
    if (networks < 1 || networks > AQUAENS_MAX_NETWORKS)
        return fail(AQUAENS_E_INVALID, "networks=%lld: must be in [1, %d]", (long long)networks, AQUAENS_MAX_NETWORKS);
    if (mode != AQUAENS_MEAN && mode != AQUAENS_VOTE)
        return fail(AQUAENS_E_INVALID, "mode=%d: must be AQUAENS_MEAN (%d) or AQUAENS_VOTE (%d)", mode, AQUAENS_MEAN, AQUAENS_VOTE);
    if (N < 0 || ld < N) return fail(AQUAENS_E_INVALID, "bad sizes: N=%lld ld=%lld", (long long)N, (long long)ld);
    if (env_offset < 0) return fail(AQUAENS_E_INVALID, "env_offset < 0");
    uint32_t eps_bits;                   // by its bits, as the kernel does: NaN or below zero (-0 is zero)
    std::memcpy(&eps_bits, &epsilon, sizeof(eps_bits));
    if (eps_bits > 0x7F800000u && eps_bits != 0x80000000u) return fail(AQUAENS_E_INVALID, "epsilon=%g: must be >= 0", (double)epsilon);
    if (action == nullptr && q == nullptr && q_taken == nullptr && variance == nullptr && votes == nullptr)
        return fail(AQUAENS_E_INVALID, "action, q, q_taken, variance and votes are all NULL");
    if (q != nullptr && q_ld < N) return fail(AQUAENS_E_INVALID, "q_ld=%lld < N=%lld", (long long)q_ld, (long long)N);
    if ((variance != nullptr || votes != nullptr) && x_ld < N) return fail(AQUAENS_E_INVALID, "x_ld=%lld < N=%lld", (long long)x_ld, (long long)N);
    if (N > 0 && in == nullptr) return fail(AQUAENS_E_INVALID, "in is NULL");
    if (!aligned(in, 4) || !aligned(q, 4) || !aligned(q_taken, 4)) return fail(AQUAENS_E_ALIGN, "in / q / q_taken must be 4-byte aligned");
    if (!aligned(variance, 4) || !aligned(votes, 4)) return fail(AQUAENS_E_ALIGN, "variance / votes must be 4-byte aligned");
    if (!aligned(epsilon_dev, 4)) return fail(AQUAENS_E_ALIGN, "epsilon_dev must be 4-byte aligned");
    if (!aligned(tick_base_dev, 8)) return fail(AQUAENS_E_ALIGN, "tick_base_dev must be 8-byte aligned");
    if (N == 0) return 0;

    int cus = 0;
    if (const int rc = compute_units(&cus, AQUAENS_E_NODEVICE)) return rc;
    int64_t shape[3];
    launch_shape(N, cus, shape);

    EnsArgs a;
    a.bank = static_cast<const float*>(bank_dev);
    a.member = member_dev;
    a.networks = static_cast<int>(networks); a.mode = mode; a.groups = shape[1];
    a.in = in; a.ld = ld; a.N = N; a.env_offset = env_offset; a.q_ld = q_ld; a.x_ld = x_ld;
    a.epsilon = epsilon; a.epsilon_dev = epsilon_dev; a.seed = seed; a.tick = tick; a.tick_base = tick_base_dev;
    a.action = action; a.q = q; a.q_taken = q_taken; a.variance = variance; a.votes = votes;
    const dim3 grid(static_cast<unsigned>(shape[0])), block(BLOCK);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool raw = in_is_normalised == 0, eps = epsilon_dev != nullptr || epsilon > 0.0f;
    if (raw && eps) hipLaunchKernelGGL((qens_kernel<true, true>), grid, block, 0, s, a);
    else if (raw) hipLaunchKernelGGL((qens_kernel<true, false>), grid, block, 0, s, a);
    else if (eps) hipLaunchKernelGGL((qens_kernel<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((qens_kernel<false, false>), grid, block, 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "qens_kernel launch");
    return 0;
}

}  // extern "C"
