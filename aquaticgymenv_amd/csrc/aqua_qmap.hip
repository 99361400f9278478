// aqua_qmap.hip -- libaqua_qmap.so (aqua_qmap.h): Q-value maps of the DQN's 5 -> 64 -> 64 -> 3 Q-networks
// (main/impl/dqn.py:301-314) for every network of a bank in one launch on gfx950: what the reference's plotter
// (main/plotting/dqn_qvalue_plotter.py::plot_network_qvalue) shows of one network and one goal -- best action and best
// Q-value at every cell of the world, for a number of headings -- for P networks and G goals.
//
// The network itself -- the blob's layout, the forward pass of a tile -- is stated in aqua_qnet.hpp, once for this library,
// libaqua_policy.so and libaqua_bank.so; this file restates none of it.  Here: every input
// of a map is a function of the state's index, so a lane makes its inputs in registers from four small tables and the
// kernel reads nothing per state.  The unit of work is the item (network p, goal g, tile j of the S * H * W states of one
// map), j running fastest, then g; every wavefront takes a contiguous run of items, reloading its weights (70 VGPRs, and
// a 324-float LDS part of its own) only where the network changes inside the run, and the two goal inputs where the goal
// changes.
#include <hip/hip_runtime.h>

#include "aqua_qmap.h"
#include "aqua_device.hpp"
#include "aqua_host.hpp"
#include "aqua_qnet.hpp"

namespace aqua_qmap {

using namespace aqua::qnet;

static_assert(ACT == AQUAQMAP_ACTIONS, "aqua_qmap.h names the number of actions");
constexpr int BLOCK = 256, WAVES = BLOCK / 64;
constexpr int WAVES_PER_SIMD = 3;        // resident wavefronts per SIMD = blocks per CU (<= 170 registers each)

struct MapArgs {
    const float* bank;
    const float* xs;
    const float* ys;
    const float* angles;
    const float* goals;
    int32_t W, H, states;                // states = S * H * W <= 2^30: a state's index within a map is 32-bit
    int64_t G, tiles;                    // tiles of one map; items = P * G * tiles
    int64_t share, rem;                  // items / wavefronts of the grid and the remainder: the first `rem` wavefronts take one more
    uint8_t* action;
    float* value;
    float* q;
};

// what other lanes of this wavefront wrote to (or still read from) its LDS copy is complete before anything behind this
// point (the fences order the wavefront's own LDS traffic, the barrier keeps the lanes' instructions on
// their side of it)
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

__global__ __launch_bounds__(BLOCK, WAVES_PER_SIMD) void qmap_kernel(const MapArgs a)
{
    // a copy of the LDS part per wavefront: the network is a property of the wavefront's item, not of the block
    __shared__ float4 lds_all[WAVES][LDS_FLOATS / 4];

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, col = lane & 31;
    float4* const lds4 = lds_all[wave];

    // this wavefront's contiguous run of items
    const int64_t w = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t first = w * a.share + (w < a.rem ? w : a.rem), count = a.share + (w < a.rem ? 1 : 0);
    if (count == 0) return;
    const int64_t map0 = uniform(first / a.tiles);            // p * G + g of the first item
    int64_t j = uniform(first % a.tiles), p = uniform(map0 / a.G), g = uniform(map0 % a.G);

    // the weights stay in registers while the network stays (70 VGPRs); the goal while the goal stays
    float w1[K1_STEPS][2], w2[2][K2_STEPS];
    int64_t loaded = -1;
    float goal_x = 0.0f, goal_y = 0.0f;
    bool new_goal = true;
    const uint32_t W = static_cast<uint32_t>(a.W), H = static_cast<uint32_t>(a.H), states = static_cast<uint32_t>(a.states);
    // half 0 supplies input 0 by column, half 1 input 1 by row: one table read for both
    const float* const table0 = h != 0 ? a.ys : a.xs;

    for (int64_t n = 0; n < count; ++n, ++j) {
        if (j == a.tiles) {
            j = 0;
            new_goal = true;
            if (++g == a.G) { g = 0; ++p; }
        }
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
        }
        if (new_goal) {
            new_goal = false;
            goal_x = a.goals[2 * g];
            goal_y = a.goals[2 * g + 1];
        }

        // the lane's state within the map: m = (k * H + r) * W + c (below 2^30 + 32)
        const uint32_t m = static_cast<uint32_t>(j) * TILE + col;
        const bool live = m < states;
        const uint32_t row = m / W, c = m - row * W, k = row / H, r = row - k * H;

        // k-step st of layer 1 takes input 2 st + h of the lane's state; a state that does not exist and the padding input are zero
        float x[K1_STEPS];
        x[0] = live ? table0[h != 0 ? r : c] : 0.0f;
        x[1] = live ? (h != 0 ? goal_x : a.angles[k]) : 0.0f;
        x[2] = (live && h == 0) ? goal_y : 0.0f;
        float q[ACT];
        forward<false>(lds4, w1, w2, x, h, q);

        if (h == 0 && live) {
            int act = 0;                                      // np.argmax: the lowest index on a tie
            float best = q[0];
            if (q[1] > best) { act = 1; best = q[1]; }
            if (q[2] > best) { act = 2; best = q[2]; }
            const int64_t map = p * a.G + g, at = map * a.states + m;
            if (a.action != nullptr) a.action[at] = static_cast<uint8_t>(act);
            if (a.value != nullptr) a.value[at] = best;
            if (a.q != nullptr) {
                float* const qm = a.q + map * ACT * a.states + m;
#pragma unroll
                for (int c3 = 0; c3 < ACT; ++c3) qm[static_cast<int64_t>(c3) * a.states] = q[c3];
            }
        }
    }
}

// ------------------------------------------------------------------ host side
// the sizes of a call, checked: 0, or the error code with the message set; *states = S * H * W, *maps = P * G
static int check_sizes(int64_t P, int64_t G, int64_t H, int64_t W, int64_t S, int64_t* states, int64_t* maps)
{
    if (P < 1 || P > AQUAQMAP_MAX_NETWORKS) return fail(AQUAQMAP_E_INVALID, "P=%lld: must be in [1, %d]", (long long)P, AQUAQMAP_MAX_NETWORKS);
    if (W < 1 || W > AQUAQMAP_MAX_SIDE) return fail(AQUAQMAP_E_INVALID, "W=%lld: must be in [1, %d]", (long long)W, AQUAQMAP_MAX_SIDE);
    if (H < 1 || H > AQUAQMAP_MAX_SIDE) return fail(AQUAQMAP_E_INVALID, "H=%lld: must be in [1, %d]", (long long)H, AQUAQMAP_MAX_SIDE);
    if (S < 1 || S > AQUAQMAP_MAX_SECTORS) return fail(AQUAQMAP_E_INVALID, "S=%lld: must be in [1, %d]", (long long)S, AQUAQMAP_MAX_SECTORS);
    if (G < 1 || G > AQUAQMAP_MAX_GOALS) return fail(AQUAQMAP_E_INVALID, "G=%lld: must be in [1, %d]", (long long)G, AQUAQMAP_MAX_GOALS);
    // every factor is capped, so S * H * W < 2^44 and P * G <= 2^32; the total is compared by division
    *states = S * H * W;
    if (*states > AQUAQMAP_MAX_STATES)
        return fail(AQUAQMAP_E_INVALID, "S * H * W = %lld states per map: more than %lld", (long long)*states, (long long)AQUAQMAP_MAX_STATES);
    *maps = P * G;
    if (*states > AQUAQMAP_MAX_TOTAL / *maps)
        return fail(AQUAQMAP_E_INVALID, "P * G * S * H * W = %lld * %lld states: more than %lld", (long long)*maps, (long long)*states,
                    (long long)AQUAQMAP_MAX_TOTAL);
    return 0;
}

}  // namespace aqua_qmap

using namespace aqua_qmap;

extern "C" {

int aquaqmap_version(void) { return AQUAQMAP_ABI_VERSION; }
const char* aquaqmap_last_error(void) { return g_err; }
size_t aquaqmap_weights_bytes(void) { return sizeof(float) * BLOB_FLOATS; }

int64_t aquaqmap_items(int64_t P, int64_t G, int64_t H, int64_t W, int64_t S)
{
    int64_t states = 0, maps = 0;
    if (const int rc = check_sizes(P, G, H, W, S, &states, &maps)) return rc;
    return maps * ((states + TILE - 1) / TILE);
}

int aquaqmap_maps_f32(const void* bank_dev, int64_t P, const float* xs, int64_t W, const float* ys, int64_t H, const float* angles,
                      int64_t S, const float* goals, int64_t G, uint8_t* action, float* value, float* q, void* stream)
{
    if (bank_dev == nullptr) return fail(AQUAQMAP_E_INVALID, "the bank is NULL");
    if (!aligned(bank_dev, 16)) return fail(AQUAQMAP_E_ALIGN, "the bank must be 16-byte aligned");
    if (xs == nullptr) return fail(AQUAQMAP_E_INVALID, "xs is NULL");
    if (ys == nullptr) return fail(AQUAQMAP_E_INVALID, "ys is NULL");
    if (angles == nullptr) return fail(AQUAQMAP_E_INVALID, "angles is NULL");
    if (goals == nullptr) return fail(AQUAQMAP_E_INVALID, "goals is NULL");
    int64_t states = 0, maps = 0;
    if (const int rc = check_sizes(P, G, H, W, S, &states, &maps)) return rc;
    if (action == nullptr && value == nullptr && q == nullptr) return fail(AQUAQMAP_E_INVALID, "action, value and q are all NULL");
    if (!aligned(xs, 4)) return fail(AQUAQMAP_E_ALIGN, "xs must be 4-byte aligned");
    if (!aligned(ys, 4)) return fail(AQUAQMAP_E_ALIGN, "ys must be 4-byte aligned");
    if (!aligned(angles, 4)) return fail(AQUAQMAP_E_ALIGN, "angles must be 4-byte aligned");
    if (!aligned(goals, 4)) return fail(AQUAQMAP_E_ALIGN, "goals must be 4-byte aligned");
    if (!aligned(value, 4)) return fail(AQUAQMAP_E_ALIGN, "value must be 4-byte aligned");
    if (!aligned(q, 4)) return fail(AQUAQMAP_E_ALIGN, "q must be 4-byte aligned");

    int cus = 0;
    if (const int rc = compute_units(&cus, AQUAQMAP_E_NODEVICE)) return rc;
    MapArgs a;
    a.tiles = (states + TILE - 1) / TILE;
    const int64_t items = maps * a.tiles;
    int64_t blocks = (items + WAVES - 1) / WAVES;
    if (blocks > WAVES_PER_SIMD * static_cast<int64_t>(cus)) blocks = WAVES_PER_SIMD * static_cast<int64_t>(cus);     // all resident
    a.share = items / (blocks * WAVES);
    a.rem = items % (blocks * WAVES);

    a.bank = static_cast<const float*>(bank_dev);
    a.xs = xs; a.ys = ys; a.angles = angles; a.goals = goals;
    a.W = static_cast<int32_t>(W); a.H = static_cast<int32_t>(H); a.states = static_cast<int32_t>(states); a.G = G;
    a.action = action; a.value = value; a.q = q;
    const dim3 grid(static_cast<unsigned>(blocks)), block(BLOCK);
    hipLaunchKernelGGL(qmap_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "qmap_kernel launch");
    return 0;
}

}  // extern "C"
