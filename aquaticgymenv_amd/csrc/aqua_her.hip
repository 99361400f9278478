// aqua_her.hip -- libaqua_her.so (csrc/aqua_her.h): hindsight experience replay on the experience ring.  For every sample of
// a minibatch draw the drawn transition is staged as it is stored or relabelled: replayed under a goal its own world reached
// later in the same episode, with the reward and the termination code recomputed.  Its own translation unit and library: the
// other fourteen libraries and their kernels are not touched.
//
// One kernel, her_relabel_kernel (an instance per action kind and source of the key), one thread per sample, grid-stride
// above MAX_BLOCKS blocks.  With capacity % N == 0 the next step of the world in slot c is slot c + N (mod capacity): every
// address of a walk is known once idx is, so the d and ok loads of CHUNK steps are issued together and the walk then decides
// in registers -- ceil(H / CHUNK) dependent round trips per walk at most, not H (DESIGN.md 5.17 has the measurement that made
// the fold do so).  A batch of fewer than CHUNK steps is straight-line code of its own (walk_batch<STEPS>), and the scheduler
// may not move across the end of the loads.  No LDS, no cross-lane traffic, no atomics; no thread reads what another thread
// of the launch writes (the ring, the header, the counters and the keys are only read).
// Floating point: the reward is computed in double, each operation rounded, nothing contracted: the function that computes
// it carries `#pragma clang fp contract(off)` and is the one the host entry aquaher_reward runs.
#include <hip/hip_runtime.h>

#include <cmath>

#include "aqua_her.h"
#include "aqua_device.hpp"
#include "aqua_host.hpp"

namespace {

constexpr int BLOCK = AQUAHER_BLOCK;
constexpr int MAX_BLOCKS = AQUAHER_MAX_BLOCKS;
constexpr int CHUNK = AQUAHER_CHUNK;
constexpr int ROWS = 5;                               // the observation (main/impl/utils.py:15-33)
constexpr uint32_t STREAM_HER = AQUAHER_STREAM;

static_assert(AQUAHER_MAX_HORIZON <= 255, "k + 1 and M are stored in a byte");
static_assert(AQUAHER_MAX_HORIZON % AQUAHER_CHUNK == 0, "whole batches of loads");
static_assert(STREAM_HER != aqua::STREAM_STEP && STREAM_HER != aqua::STREAM_PLACE && STREAM_HER != aqua::STREAM_POSE &&
              STREAM_HER != aqua::STREAM_ACT && STREAM_HER != 5 && STREAM_HER != 6 && STREAM_HER != 7 && STREAM_HER < 256,
              "a Philox stream of its own: 5 is the policies', 6 the minibatch draws', 7 the selector's and the sum trees'");

struct RelabelArgs {
    const int64_t* header;
    const float* s;
    const void* a;
    const float* r;
    const float* s2;
    const uint8_t* d;
    const uint8_t* ok;
    int64_t ring_ld;
    int32_t capacity, N;                              // (validated sizes that fit 32 bits travel as such)
    const int32_t* idx;
    int32_t P, B;
    int32_t H;
    uint64_t thr;                                     // floor(ratio 2^32)
    const uint64_t* t_dev;
    uint64_t seed;                                    // the key of the scalar form
    const uint64_t* seed_dev;
    float* out_s;
    void* out_a;
    float* out_r;
    float* out_s2;
    uint8_t* out_d;
    uint8_t* out_ok;
    int64_t out_ld;
    uint8_t* out_k;
    uint8_t* out_m;
};

// THE statement of the relabelled reward: the gap between the boat's and the goal's circles before and after the step, in
// the reference's units (the observation is normalised by 100; the radii add up to 5), every operation rounded in double
__host__ __device__ inline double gap_of(float qx, float qy, float gx, float gy)
{
#pragma clang fp contract(off)
    const double dx = static_cast<double>(qx) - static_cast<double>(gx);
    const double dy = static_cast<double>(qy) - static_cast<double>(gy);
    const double xx = dx * dx;
    const double yy = dy * dy;
    return 100.0 * sqrt(xx + yy) - 5.0;
}

__host__ __device__ inline void reward_of(float sx, float sy, float s2x, float s2y, float gx, float gy, float& r, uint8_t& d)
{
#pragma clang fp contract(off)
    const double gap_prev = gap_of(sx, sy, gx, gy);
    const double gap_new = gap_of(s2x, s2y, gx, gy);
    if (gap_new <= 0.0) {
        r = 10.0f;
        d = AQUAHER_TERM_SUCCESS;
    } else {
        const double diff = gap_prev - gap_new;
        r = static_cast<float>(0.7 * diff);
        d = 0;
    }
}

// what the walk of one sample carries from batch to batch
struct Walk {
    bool walking = false, sample = false;
    int M = 0;
    int64_t slot = 0;                                 // the slot of the next batch's first step
};

// STEPS steps of a walk, kb .. kb + STEPS - 1 (the last batch of a walk, or CHUNK of them): first the d and ok loads of every
// step, 2 x STEPS loads in one block with no branch and no wait among them, then the walk over what they brought
template <int STEPS>
__device__ __forceinline__ void walk_batch(const RelabelArgs& a, int kb, int32_t lim, Walk& w)
{
    static_assert(STEPS >= 1 && STEPS <= CHUNK, "a batch is at most CHUNK steps");
    uint8_t dd[STEPS], oo[STEPS];
    int64_t sl = w.slot;
#pragma unroll
    for (int u = 0; u < STEPS; ++u) {
        dd[u] = a.d[sl];
        oo[u] = a.ok[sl];
        sl += a.N;
        if (sl >= a.capacity) sl -= a.capacity;
    }
    // (the scheduler otherwise starts the walk, and its waits, among the last loads)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < STEPS; ++u) {
        // (selects, not branches: the lanes of a wavefront leave the walk at different steps)
        const int k = kb + u;
        if (u == 0 && kb == 0) w.sample = w.walking && oo[0] != 0;     // ok[c] == 0: no sample, and M stays 0
        const bool go = w.walking && k <= lim && oo[u] != 0 && dd[u] == 0;
        w.M = go ? k + 1 : w.M;
        w.walking = go;
    }
    w.slot = sl;
}

// F32X2: the action rows are float32 [2][ld] (else uint8 [ld]); TABLE: the keys come from seed_dev
template <bool F32X2, bool TABLE>
__global__ __launch_bounds__(BLOCK) void her_relabel_kernel(const RelabelArgs a)
{
    const int64_t cursor = a.header[0];
    // capacity < 2^31, so everything below a valid cursor or slot divides in 32 bits
    const uint32_t N32 = static_cast<uint32_t>(a.N);
    const bool ring_ok = cursor >= 0 && cursor < a.capacity && static_cast<uint32_t>(cursor) % N32 == 0;
    const uint32_t B32 = static_cast<uint32_t>(a.B);
    const int64_t total = static_cast<int64_t>(a.P) * a.B;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * BLOCK;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x; i < total; i += stride) {
        const uint32_t p = static_cast<uint32_t>(i) / B32;              // i < P * B <= 2^32
        const uint32_t j = static_cast<uint32_t>(i) - p * B32;
        const uint64_t t_new = a.t_dev[p] + 1;                          // the update this draw is for
        const uint64_t seed = TABLE ? a.seed_dev[p] : a.seed;
        const int64_t c = a.idx[i];
        const bool walking = ring_ok && c >= 0 && c < a.capacity;       // otherwise c is never an address
        int32_t age = 0;
        if (walking) {
            const int64_t round = c - static_cast<int64_t>(static_cast<uint32_t>(c) % N32);
            int64_t x = cursor - a.N - round;                           // in [-capacity, capacity)
            if (x < 0) x += a.capacity;
            age = static_cast<int32_t>(static_cast<uint32_t>(x) / N32);    // rounds written after c's
        }
        const int32_t lim = age < a.H - 1 ? age : a.H - 1;              // the last step this walk may take
        Walk w;
        w.walking = walking;
        w.slot = walking ? c : 0;                                       // in [0, capacity) throughout, N <= capacity
#pragma unroll 1
        for (int kb = 0; kb < a.H && w.walking; kb += CHUNK) {
            // a batch of exactly min(H - kb, CHUNK) steps: the count is uniform, so this is a scalar branch to straight-line code
            const int rem = a.H - kb;
            switch (rem < CHUNK ? rem : CHUNK) {
            case 1: walk_batch<1>(a, kb, lim, w); break;
            case 2: walk_batch<2>(a, kb, lim, w); break;
            case 3: walk_batch<3>(a, kb, lim, w); break;
            case 4: walk_batch<4>(a, kb, lim, w); break;
            case 5: walk_batch<5>(a, kb, lim, w); break;
            case 6: walk_batch<6>(a, kb, lim, w); break;
            case 7: walk_batch<7>(a, kb, lim, w); break;
            default: walk_batch<CHUNK>(a, kb, lim, w); break;
            }
        }
        const bool valid = w.sample;
        const uint32_t M = static_cast<uint32_t>(w.M);                  // <= min(age + 1, H)
        uint32_t rr[4];
        // (the scalar key is a kernel argument: its schedule stays a running pair of scalars instead of twenty hoisted ones)
        aqua::draw<!TABLE>(seed, static_cast<uint64_t>(j), t_new, STREAM_HER, 0u, rr);
        const bool relabel = M > 0 && static_cast<uint64_t>(rr[0]) < a.thr;
        const uint32_t k = static_cast<uint32_t>((static_cast<uint64_t>(rr[1]) * M) >> 32);    // < M
        // (what is no sample reads slot 0, a valid address, and keeps nothing of it: loads without a branch each)
        const int64_t src = valid ? c : 0;
        // k <= age < capacity / N: c + k N < 2 capacity, and one subtraction is the modulo
        int64_t goal = src;
        if (relabel) {
            goal = c + static_cast<int64_t>(k) * a.N;
            if (goal >= a.capacity) goal -= a.capacity;
        }
        uint32_t x[ROWS], x2[ROWS], act0, act1 = 0;
        const uint32_t* ps = reinterpret_cast<const uint32_t*>(a.s) + src;
        const uint32_t* ps2 = reinterpret_cast<const uint32_t*>(a.s2) + src;
#pragma unroll
        for (int row = 0; row < ROWS; ++row) {
            x[row] = *ps;
            x2[row] = *ps2;
            ps += a.ring_ld;
            ps2 += a.ring_ld;
        }
        const uint32_t g0 = reinterpret_cast<const uint32_t*>(a.s2)[goal];
        const uint32_t g1 = reinterpret_cast<const uint32_t*>(a.s2)[a.ring_ld + goal];
        uint32_t rew = reinterpret_cast<const uint32_t*>(a.r)[src];
        uint8_t code = a.d[src];
        if (!F32X2) {
            act0 = static_cast<const uint8_t*>(a.a)[src];
        } else {
            act0 = static_cast<const uint32_t*>(a.a)[src];
            act1 = static_cast<const uint32_t*>(a.a)[a.ring_ld + src];
        }
        if (relabel) {
            float r_new;
            reward_of(__uint_as_float(x[0]), __uint_as_float(x[1]), __uint_as_float(x2[0]), __uint_as_float(x2[1]),
                      __uint_as_float(g0), __uint_as_float(g1), r_new, code);
            rew = __float_as_uint(r_new);
            x[3] = g0; x[4] = g1;
            x2[3] = g0; x2[4] = g1;
        }
        // zeros as bit patterns: the rows are copied, never computed with
#pragma unroll
        for (int row = 0; row < ROWS; ++row) {
            x[row] = valid ? x[row] : 0u;
            x2[row] = valid ? x2[row] : 0u;
        }
        act0 = valid ? act0 : 0u;
        act1 = valid ? act1 : 0u;
        uint32_t* po = reinterpret_cast<uint32_t*>(a.out_s) + i;
        uint32_t* po2 = reinterpret_cast<uint32_t*>(a.out_s2) + i;
#pragma unroll
        for (int row = 0; row < ROWS; ++row) {
            *po = x[row];
            *po2 = x2[row];
            po += a.out_ld;
            po2 += a.out_ld;
        }
        reinterpret_cast<uint32_t*>(a.out_r)[i] = valid ? rew : 0u;
        if (!F32X2) {
            static_cast<uint8_t*>(a.out_a)[i] = static_cast<uint8_t>(act0);
        } else {
            static_cast<uint32_t*>(a.out_a)[i] = act0;
            static_cast<uint32_t*>(a.out_a)[a.out_ld + i] = act1;
        }
        a.out_d[i] = valid ? code : static_cast<uint8_t>(0);
        a.out_ok[i] = valid ? 1 : 0;
        if (a.out_k != nullptr) a.out_k[i] = static_cast<uint8_t>(relabel ? k + 1 : 0);
        if (a.out_m != nullptr) a.out_m[i] = static_cast<uint8_t>(M);
    }
}

// ------------------------------------------------------------------ host side
unsigned grid_of(int64_t n)
{
    int64_t blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
    return static_cast<unsigned>(blocks < 1 ? 1 : blocks);
}

int threshold_of(double ratio, uint64_t& thr)
{
    if (!is_number(ratio) || !(ratio >= 0.0 && ratio <= 1.0)) return fail(AQUAHER_E_INVALID, "ratio=%g: must be in [0, 1]", ratio);
    thr = static_cast<uint64_t>(std::floor(ratio * 4294967296.0));    // (a power of two: the product is exact)
    return 0;
}

}  // namespace

extern "C" {

int aquaher_version(void) { return AQUAHER_ABI_VERSION; }
const char* aquaher_last_error(void) { return g_err; }

int aquaher_threshold(double ratio, uint64_t* thr)
{
    if (thr == nullptr) return fail(AQUAHER_E_INVALID, "thr is NULL");
    return threshold_of(ratio, *thr);
}

int aquaher_reward(const float s[5], const float s2[5], float gx, float gy, float* r, uint8_t* d)
{
    if (s == nullptr || s2 == nullptr || r == nullptr || d == nullptr) return fail(AQUAHER_E_INVALID, "s, s2, r or d is NULL");
    reward_of(s[0], s[1], s2[0], s2[1], gx, gy, *r, *d);
    return 0;
}

int aquaher_relabel(const int64_t* header, const float* s, const void* a, const float* r, const float* s2, const uint8_t* d,
                    const uint8_t* ok, int64_t ring_ld, int64_t capacity, int action_kind, int64_t N,
                    const int32_t* idx, int64_t P, int64_t B, int H, double ratio, const uint64_t* t_dev, uint64_t seed,
                    const uint64_t* seed_dev, float* out_s, void* out_a, float* out_r, float* out_s2, uint8_t* out_d,
                    uint8_t* out_ok, int64_t out_ld, uint8_t* out_k, uint8_t* out_m, void* stream)
{
    if (header == nullptr) return fail(AQUAHER_E_INVALID, "header is NULL");
    if (s == nullptr || a == nullptr || r == nullptr || s2 == nullptr || d == nullptr || ok == nullptr)
        return fail(AQUAHER_E_INVALID, "s, a, r, s2, d or ok is NULL");
    if (capacity <= 0 || capacity > AQUAHER_MAX_CAPACITY)
        return fail(AQUAHER_E_INVALID, "capacity=%lld: must be in [1, %d]", (long long)capacity, AQUAHER_MAX_CAPACITY);
    if (ring_ld < capacity) return fail(AQUAHER_E_INVALID, "ring_ld=%lld: below the capacity %lld", (long long)ring_ld, (long long)capacity);
    if (action_kind != AQUAHER_ACT_U8 && action_kind != AQUAHER_ACT_F32X2)
        return fail(AQUAHER_E_INVALID, "action_kind=%d: AQUAHER_ACT_U8 or AQUAHER_ACT_F32X2", action_kind);
    if (N < 1 || N > capacity) return fail(AQUAHER_E_INVALID, "N=%lld: must be in [1, capacity=%lld]", (long long)N, (long long)capacity);
    if (capacity % N != 0)
        return fail(AQUAHER_E_INVALID, "capacity=%lld is no multiple of N=%lld: a slot must belong to one world", (long long)capacity, (long long)N);
    if (P < 1 || P > AQUAHER_MAX_NETWORKS) return fail(AQUAHER_E_INVALID, "P=%lld: must be in [1, %d]", (long long)P, AQUAHER_MAX_NETWORKS);
    if (B < 0 || B > AQUAHER_MAX_BATCH) return fail(AQUAHER_E_INVALID, "B=%lld: must be in [0, %d]", (long long)B, AQUAHER_MAX_BATCH);
    if (H < 1 || H > AQUAHER_MAX_HORIZON) return fail(AQUAHER_E_INVALID, "H=%d: must be in [1, %d]", H, AQUAHER_MAX_HORIZON);
    uint64_t thr = 0;
    if (int rc = threshold_of(ratio, thr)) return rc;
    if (t_dev == nullptr) return fail(AQUAHER_E_INVALID, "t_dev is NULL");
    if (seed_dev != nullptr && seed != AQUAHER_NO_SEED)
        return fail(AQUAHER_E_INVALID, "seed=%llu and seed_dev: pass one of them (seed = AQUAHER_NO_SEED with a table)", (unsigned long long)seed);
    if (out_ld < P * B) return fail(AQUAHER_E_INVALID, "out_ld=%lld: below P * B = %lld", (long long)out_ld, (long long)(P * B));
    if (!aligned(header, 8) || !aligned(t_dev, 8) || !aligned(seed_dev, 8))
        return fail(AQUAHER_E_ALIGN, "header / t_dev / seed_dev must be 8-byte aligned");
    if (!aligned(idx, 4) || !aligned(s, 4) || !aligned(r, 4) || !aligned(s2, 4) || !aligned(out_s, 4) || !aligned(out_r, 4) || !aligned(out_s2, 4))
        return fail(AQUAHER_E_ALIGN, "idx and the float32 rows must be 4-byte aligned");
    if (action_kind == AQUAHER_ACT_F32X2 && (!aligned(a, 4) || !aligned(out_a, 4)))
        return fail(AQUAHER_E_ALIGN, "float32 action rows must be 4-byte aligned");
    if (B == 0) return 0;
    if (idx == nullptr) return fail(AQUAHER_E_INVALID, "idx is NULL");
    if (out_s == nullptr || out_a == nullptr || out_r == nullptr || out_s2 == nullptr || out_d == nullptr || out_ok == nullptr)
        return fail(AQUAHER_E_INVALID, "out_s, out_a, out_r, out_s2, out_d or out_ok is NULL");

    RelabelArgs k;
    k.header = header; k.s = s; k.a = a; k.r = r; k.s2 = s2; k.d = d; k.ok = ok; k.ring_ld = ring_ld; k.capacity = static_cast<int32_t>(capacity);
    k.N = static_cast<int32_t>(N); k.idx = idx; k.P = static_cast<int32_t>(P); k.B = static_cast<int32_t>(B); k.H = H;
    k.thr = thr; k.t_dev = t_dev; k.seed = seed; k.seed_dev = seed_dev;
    k.out_s = out_s; k.out_a = out_a; k.out_r = out_r; k.out_s2 = out_s2; k.out_d = out_d; k.out_ok = out_ok; k.out_ld = out_ld;
    k.out_k = out_k; k.out_m = out_m;
    const bool f32x2 = action_kind == AQUAHER_ACT_F32X2, table = seed_dev != nullptr;
    auto kernel = f32x2 ? (table ? her_relabel_kernel<true, true> : her_relabel_kernel<true, false>)
                        : (table ? her_relabel_kernel<false, true> : her_relabel_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(grid_of(P * B)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), k);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "her_relabel_kernel launch");
    return 0;
}

}  // extern "C"
