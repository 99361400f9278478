// aqua_prio.hip -- libaqua_prio.so (csrc/aqua_prio.h): prioritised experience replay for every network of a learner bank.
// A sum tree of fan-out 64 per network over the network's own slots of the one experience ring, kept by integer atomics
// (exchange on the leaf, 64-bit add of the signed difference on every ancestor, max on pmax), drawn from by a descent that is
// one wavefront-wide prefix sum per level, and the bank update with the importance weights multiplied in.  Its own
// translation unit and library: the other thirteen libraries and their kernels are not touched.
//
// Kernels: prio_insert_kernel and prio_set_kernel (one thread per slot; lanes that follow each other and share an ancestor
// add their differences in the wavefront and issue one atomic), prio_descend_kernel (one wavefront per sample),
// prio_weight_kernel (one block per network), and the two kernels of the update: the shared bodies of aqua_lrn.hpp, the
// gradient one instantiated with WEIGHTED = true, in the bank form of aqua_lbank.hip (grid y = the network).
// Every sum in the tree is an integer sum: any order of arrival gives the same bits.  The floating point here -- the power
// function, the quantiser, beta and the weights -- is stated once in __host__ __device__ functions under
// `#pragma clang fp contract(off)`: sums, products and quotients in double, each correctly rounded, the same on both sides.
#include <hip/hip_runtime.h>

#include <cmath>

#include "aqua_prio.h"
#include "../../include/aqua_lbank.h"
#include "aqua_device.hpp"
#include "aqua_host.hpp"
#include "aqua_qnet.hpp"
#include "aqua_lrn.hpp"

namespace {

using namespace aqua::lrn;

constexpr int FAN = AQUAPRIO_FANOUT, FAN_BITS = 6;
constexpr int LEVELS = AQUAPRIO_MAX_LEVELS;
constexpr int PBLOCK = AQUAPRIO_BLOCK, PMAX_BLOCKS = AQUAPRIO_MAX_BLOCKS, PWAVES = PBLOCK / 64;
constexpr uint32_t STREAM_PRIO = AQUAPRIO_STREAM;
constexpr int HYPER = AQUALBANK_HYPER_WORDS;
enum { H_GAMMA = 0, H_TAU, H_LR, H_BETA1, H_BETA2, H_EPS };

static_assert(FAN == 64 && (1 << FAN_BITS) == FAN, "a node is one wavefront's load");
static_assert(AQUAPRIO_ONE == 1 << AQUAPRIO_FRAC_BITS && AQUAPRIO_LAYOUT_WORDS == 3 + 3 * LEVELS, "aqua_prio.h restates them");
static_assert(STREAM_PRIO != STREAM_LEARNER && STREAM_PRIO != STREAM_POLICY && STREAM_PRIO != aqua::STREAM_STEP &&
              STREAM_PRIO != aqua::STREAM_PLACE && STREAM_PRIO != aqua::STREAM_POSE && STREAM_PRIO != aqua::STREAM_ACT,
              "the descent draws on a stream of its own");
static_assert(PARAMS == AQUALBANK_PARAMS && AQUAPRIO_MAX_BATCH == AQUALBANK_MAX_BATCH && AQUAPRIO_MAX_NETWORKS == AQUALBANK_MAX_NETWORKS,
              "the update is the learner bank's");
static_assert(AQUAPRIO_MAX_NETWORKS <= 65535, "the network is the grid's y index");

// ------------------------------------------------------------------ the floating point, host and device
__host__ __device__ inline uint64_t bits_of(double x)
{
    uint64_t b;
    memcpy(&b, &x, sizeof(b));
    return b;
}

__host__ __device__ inline double from_bits(uint64_t b)
{
    double x;
    memcpy(&x, &b, sizeof(x));
    return x;
}

// to the nearest integer, ties to even, for |x| < 2^51: two correctly rounded sums
__host__ __device__ inline double round_even(double x)
{
#pragma clang fp contract(off)
    const double big = 6755399441055744.0;                // 1.5 * 2^52
    const double t = x + big;
    return t - big;
}

// THE statement of x^e, for x in [2^-1000, 2^1000] and |e| <= 1: x = m 2^k with m in [sqrt(1/2), sqrt(2));
// ln m = 2 atanh(s), s = (m - 1) / (m + 1), by its series to s^25 (s^2 < 0.0295: the first term left out is below 2^-65 of the
// sum); y = e ln x; exp(y) = 2^n exp(r), n = rint(y / ln 2), r = y - n ln 2 in two pieces (n ln2_hi is exact), |r| < 0.347,
// by the Taylor polynomial of degree 13 (the first term left out is below 2^-55).  Rounding: |ln x| <= 694 carries an absolute
// error of a few 2^-44 at the very ends and of 2^-47 for |ln x| <= 45, which is the relative error of the result.
__host__ __device__ inline double pow_of(double x, double e)
{
#pragma clang fp contract(off)
    const uint64_t b = bits_of(x);
    int k = static_cast<int>((b >> 52) & 0x7FFu) - 1023;
    double m = from_bits((b & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);     // [1, 2)
    if (m >= 1.4142135623730951) {
        m = m * 0.5;
        k += 1;
    }
    const double s = (m - 1.0) / (m + 1.0);
    const double z = s * s;
    double p = 1.0 / 25.0;
    p = p * z + 1.0 / 23.0;
    p = p * z + 1.0 / 21.0;
    p = p * z + 1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z + 1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z + 1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z + 1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z + 1.0 / 3.0;
    p = p * z + 1.0;
    const double ln_m = (2.0 * s) * p;
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;   // ln2_hi: 32 trailing zero bits
    const double kd = static_cast<double>(k);
    const double ln_x = kd * ln2_hi + (kd * ln2_lo + ln_m);
    const double y = e * ln_x;
    const double n = round_even(y * 1.4426950408889634);
    const double r = (y - n * ln2_hi) - n * ln2_lo;
    double q = 1.0 / 6227020800.0;
    q = q * r + 1.0 / 479001600.0;
    q = q * r + 1.0 / 39916800.0;
    q = q * r + 1.0 / 3628800.0;
    q = q * r + 1.0 / 362880.0;
    q = q * r + 1.0 / 40320.0;
    q = q * r + 1.0 / 5040.0;
    q = q * r + 1.0 / 720.0;
    q = q * r + 1.0 / 120.0;
    q = q * r + 1.0 / 24.0;
    q = q * r + 1.0 / 6.0;
    q = q * r + 0.5;
    q = q * r + 1.0;
    q = q * r + 1.0;
    const int64_t ni = static_cast<int64_t>(n);                                    // |n| <= 1001
    return q * from_bits(static_cast<uint64_t>(ni + 1023) << 52);
}

// the leaf of a TD error: td >= 0 and td + eps within the range of pow_of
__host__ __device__ inline uint32_t quantise_of(double td, double alpha, double eps)
{
#pragma clang fp contract(off)
    const double v = td + eps;
    const double x = pow_of(v, alpha) * static_cast<double>(AQUAPRIO_ONE);
    if (x >= static_cast<double>(AQUAPRIO_QMAX)) return AQUAPRIO_QMAX;
    const double r = round_even(x);
    return r < 1.0 ? 1u : static_cast<uint32_t>(r);
}

__host__ __device__ inline double beta_of(uint64_t t, double beta0, int64_t anneal)
{
#pragma clang fp contract(off)
    const uint64_t a = static_cast<uint64_t>(anneal);
    const double f = static_cast<double>(t < a ? t : a) / static_cast<double>(a);
    const double b = beta0 + (1.0 - beta0) * f;
    return b < 1.0 ? b : 1.0;
}

__host__ __device__ inline double weight_of(uint64_t size, uint32_t q, uint64_t T, double beta)
{
#pragma clang fp contract(off)
    const double ratio = static_cast<double>(T) / (static_cast<double>(size) * static_cast<double>(q));
    return pow_of(ratio, beta);
}

// ------------------------------------------------------------------ the trees
struct Tree {
    char* base;
    int32_t levels;                          // the leaves included
    int32_t capacity, N, seg, P;             // (validated sizes that fit 32 bits travel as such)
    int64_t stride[LEVELS];                  // entries per network
    int64_t off[LEVELS];                     // bytes
};

struct Layout {
    int levels;
    int64_t total, L0;
    int64_t n[LEVELS], stride[LEVELS], off[LEVELS];
};

__device__ __forceinline__ uint32_t* leaf_of(const Tree& t, int64_t p) { return reinterpret_cast<uint32_t*>(t.base + t.off[0]) + p * t.stride[0]; }
__device__ __forceinline__ uint64_t* level_of(const Tree& t, int k, int64_t p) { return reinterpret_cast<uint64_t*>(t.base + t.off[k]) + p * t.stride[k]; }

// the worlds of network p: w_p
__device__ __forceinline__ uint32_t worlds_of(const Tree& t, uint32_t p)
{
    const int64_t first = static_cast<int64_t>(p) * t.seg;
    if (first >= t.N) return 0;
    const int64_t left = t.N - first;
    return static_cast<uint32_t>(left < t.seg ? left : t.seg);
}

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d)
{
    const uint32_t lo = __shfl_up(static_cast<uint32_t>(v), d), hi = __shfl_up(static_cast<uint32_t>(v >> 32), d);
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int lane)
{
    const uint32_t lo = __shfl(static_cast<uint32_t>(v), lane), hi = __shfl(static_cast<uint32_t>(v >> 32), lane);
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

// The difference `diff` of leaf c of network p goes to every ancestor.  Called by ALL 64 lanes of a wavefront (an idle lane:
// active == false).  Per level a segmented sum over the runs of lanes that follow each other with the same (network, node):
// the last lane of a run adds the run's sum with one atomic.  Integers throughout: any grouping gives the same tree.
__device__ __forceinline__ void propagate(const Tree& t, bool active, uint32_t p, uint32_t c, int64_t diff)
{
    const int lane = threadIdx.x & 63;
    uint32_t node = c;
    if (!active) diff = 0;
    for (int k = 1; k < t.levels; ++k) {
        node >>= FAN_BITS;
        const uint64_t key = active ? (static_cast<uint64_t>(p) << 32) | node : ~0ull;
        const uint64_t before = shfl_up64(key, 1);
        const bool head = lane == 0 || before != key;
        uint64_t sum = static_cast<uint64_t>(diff);
        uint32_t flag = head ? 1u : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t s_o = shfl_up64(sum, d);
            const uint32_t f_o = __shfl_up(flag, d);
            if (lane >= d) {
                if (flag == 0) sum += s_o;
                flag |= f_o;
            }
        }
        const uint32_t next_head = __shfl_down(head ? 1u : 0u, 1);
        const bool tail = lane == 63 || next_head != 0;
        if (active && tail && sum != 0)
            atomicAdd(reinterpret_cast<unsigned long long*>(level_of(t, k, p) + node), static_cast<unsigned long long>(sum));
    }
}

struct InsertArgs {
    Tree t;
    uint32_t* pmax;
    const int64_t* header;
    const uint8_t* ok;
};

__global__ __launch_bounds__(PBLOCK) void prio_insert_kernel(const InsertArgs a)
{
    const Tree& t = a.t;
    const int64_t base = a.header[2];
    if (base < 0 || base >= t.capacity || static_cast<uint32_t>(base) % static_cast<uint32_t>(t.N) != 0) return;   // (uniform)
    const uint32_t round = static_cast<uint32_t>(base) / static_cast<uint32_t>(t.N);
    const uint32_t seg = static_cast<uint32_t>(t.seg);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * PBLOCK;
    // (every lane of a wavefront takes the same number of turns: propagate() shuffles across all 64)
    for (int64_t i0 = static_cast<int64_t>(blockIdx.x) * PBLOCK; i0 < t.N; i0 += stride) {
        const int64_t i = i0 + threadIdx.x;
        bool active = i < t.N;
        uint32_t p = 0, c = 0;
        int64_t diff = 0;
        if (active) {
            p = static_cast<uint32_t>(i) / seg;
            active = p < static_cast<uint32_t>(t.P);
        }
        if (active) {
            const uint32_t w = worlds_of(t, p);                        // >= 1: world i is one of them
            c = round * w + (static_cast<uint32_t>(i) - p * seg);     // < (capacity / N) seg = L0
            const uint32_t q = a.ok[base + i] != 0 ? a.pmax[p] : 0u;
            const uint32_t old = atomicExch(leaf_of(t, p) + c, q);
            diff = static_cast<int64_t>(q) - static_cast<int64_t>(old);
        }
        propagate(t, active, p, c, diff);
    }
}

struct SetArgs {
    Tree t;
    uint32_t* pmax;
    const int32_t* idx;
    const float* td;
    int64_t B;
    double alpha, eps;
};

__global__ __launch_bounds__(PBLOCK) void prio_set_kernel(const SetArgs a)
{
    const Tree& t = a.t;
    const int64_t total = static_cast<int64_t>(t.P) * a.B;            // <= 2^32
    const uint32_t B32 = static_cast<uint32_t>(a.B), N32 = static_cast<uint32_t>(t.N), seg = static_cast<uint32_t>(t.seg);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * PBLOCK;
    for (int64_t i0 = static_cast<int64_t>(blockIdx.x) * PBLOCK; i0 < total; i0 += stride) {
        const int64_t i = i0 + threadIdx.x;
        bool active = i < total;
        uint32_t p = 0, c = 0;
        int64_t diff = 0;
        if (active) {
            p = static_cast<uint32_t>(static_cast<uint64_t>(i) / B32);
            const int32_t slot = a.idx[i];
            const uint32_t tb = __float_as_uint(a.td[i]);             // by its bits: finite and not negative (+0 and -0 are 0)
            const bool td_ok = (tb & 0x7F800000u) != 0x7F800000u && ((tb >> 31) == 0 || (tb << 1) == 0);
            active = slot >= 0 && slot < t.capacity && td_ok;
            if (active) {
                const uint32_t world = static_cast<uint32_t>(slot) % N32, round = static_cast<uint32_t>(slot) / N32;
                active = world / seg == p;                             // the slot is one of network p's
                if (active) {
                    const uint32_t w = worlds_of(t, p);
                    c = round * w + (world - p * seg);
                    const uint32_t q = quantise_of(static_cast<double>(fabsf(a.td[i])), a.alpha, a.eps);
                    atomicMax(a.pmax + p, q);
                    const uint32_t old = atomicExch(leaf_of(t, p) + c, q);
                    diff = static_cast<int64_t>(q) - static_cast<int64_t>(old);
                }
            }
        }
        propagate(t, active, p, c, diff);
    }
}

struct DrawArgs {
    Tree t;
    const int64_t* header;
    const uint64_t* t_dev;
    const uint64_t* seed;
    int32_t* idx;
    float* weight;
    uint32_t* q_out;
    int64_t B;
    double beta0;
    int64_t anneal;
};

// one wavefront per sample (blockIdx.y = the network): from the root down, one load and one prefix sum per level
__global__ __launch_bounds__(PBLOCK) void prio_descend_kernel(const DrawArgs a)
{
    const Tree& t = a.t;
    const uint32_t p = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t T = level_of(t, t.levels - 1, p)[0];
    const uint64_t t_new = a.t_dev[p] + 1;                             // the update this draw is for
    const uint64_t seed = a.seed[p];
    const uint32_t w = worlds_of(t, p);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * PWAVES;
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * PWAVES + wave; j < a.B; j += stride) {
        int32_t slot = -1;
        uint32_t q = 0;
        if (T != 0 && w != 0) {
            uint32_t rr[4];
            aqua::draw<false>(seed, static_cast<uint64_t>(j), t_new, STREAM_PRIO, 0u, rr);
            uint64_t u = __umul64hi((static_cast<uint64_t>(rr[0]) << 32) | rr[1], T);   // in [0, T)
            uint64_t node = 0;
            bool found = true;
            for (int k = t.levels - 1; k >= 1; --k) {
                const uint64_t child = node * FAN + lane;              // < stride[k - 1]: the levels are padded to whole nodes
                const uint64_t v = k == 1 ? static_cast<uint64_t>(leaf_of(t, p)[child]) : level_of(t, k - 1, p)[child];
                uint64_t prefix = v;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint64_t o = shfl_up64(prefix, d);
                    if (lane >= d) prefix += o;
                }
                const uint64_t mask = __builtin_amdgcn_ballot_w64(prefix > u);
                if (mask == 0) {                                       // (the node's sum is not above u: the invariant is broken)
                    found = false;
                    break;
                }
                const int sel = __ffsll(static_cast<long long>(mask)) - 1;
                u -= shfl64(prefix - v, sel);
                q = static_cast<uint32_t>(shfl64(v, sel));             // (the last level's is the leaf)
                node = node * FAN + sel;
            }
            if (found && q != 0) {
                const uint32_t c = static_cast<uint32_t>(node), round = c / w;
                const int64_t s = static_cast<int64_t>(round) * t.N + static_cast<int64_t>(p) * t.seg + (c - round * w);
                if (s < t.capacity) slot = static_cast<int32_t>(s);
            }
            if (slot < 0) q = 0;
        }
        if (lane == 0) {
            a.idx[static_cast<int64_t>(p) * a.B + j] = slot;
            a.q_out[static_cast<int64_t>(p) * a.B + j] = q;
        }
    }
}

// one block per network: beta from the update counter, the largest raw weight, the normalised weights
__global__ __launch_bounds__(PBLOCK) void prio_weight_kernel(const DrawArgs a)
{
#pragma clang fp contract(off)
    __shared__ double red[PBLOCK];
    const Tree& t = a.t;
    const uint32_t p = blockIdx.x;
    const int tid = threadIdx.x;
    const uint64_t T = level_of(t, t.levels - 1, p)[0];
    const double beta = beta_of(a.t_dev[p], a.beta0, a.anneal);
    int64_t size = a.header[1];
    if (size < 0) size = 0;
    if (size > t.capacity) size = t.capacity;
    uint64_t size_p = static_cast<uint64_t>(size / t.N) * worlds_of(t, p);
    if (size_p < 1) size_p = 1;
    const uint32_t* const q = a.q_out + static_cast<int64_t>(p) * a.B;
    float* const out = a.weight + static_cast<int64_t>(p) * a.B;
    double mx = 0.0;
    for (int64_t j = tid; j < a.B; j += PBLOCK) {
        const uint32_t qj = q[j];
        if (qj != 0) {
            const double wj = weight_of(size_p, qj, T, beta);
            mx = wj > mx ? wj : mx;
        }
    }
    red[tid] = mx;
    __syncthreads();
    for (int s = PBLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid + s] > red[tid] ? red[tid + s] : red[tid];
        __syncthreads();
    }
    const double wmax = red[0];                                        // a maximum: the same whatever the order
    for (int64_t j = tid; j < a.B; j += PBLOCK) {
        const uint32_t qj = q[j];
        out[j] = qj != 0 ? static_cast<float>(weight_of(size_p, qj, T, beta) / wmax) : 0.0f;
    }
}

// ------------------------------------------------------------------ the weighted update: aqua_lbank.hip's wrappers
struct PrioGradArgs {
    const float* theta;                      // [P][PARAMS]
    const float* theta_target;
    const uint64_t* t_dev;                   // [P]
    const float* s;
    const uint8_t* a;
    const float* r;
    const float* s2;
    const uint8_t* d;
    const uint8_t* ok;
    int64_t ld, size, B;
    const int32_t* idx;                      // [P][B]
    const double* hyper;                     // [P][HYPER]
    int tiles_per_wave;
    int loss_ref;
    char* ws;                                // P regions of `region` bytes
    int64_t region;
    int32_t* idx_out;                        // nullable [P][B]
    const float* weight;                     // [P][B]
    float* td_out;                           // [P][B]
};

struct PrioApplyArgs {
    float* theta;
    float* theta_target;
    float* m;
    float* v;
    uint64_t* t_dev;
    const char* ws;
    int64_t region;
    int partials;
    const double* hyper;
    float* blob_online;                      // nullable [P][blob_floats]
    float* blob_target;
    const int32_t* perm;
    int64_t blob_floats;
    float* grad_out;                         // nullable [P][PARAMS]
    float* loss;                             // nullable [P]
};

template <int STRAT>
__global__ __launch_bounds__(BLOCK) void prio_grad_kernel(const PrioGradArgs b)
{
    const int64_t p = blockIdx.y;
    GradArgs a;
    a.theta = b.theta + p * PARAMS;
    a.theta_target = b.theta_target + p * PARAMS;
    a.t_dev = b.t_dev + p;
    a.s = b.s; a.a = b.a; a.r = b.r; a.s2 = b.s2; a.d = b.d; a.ok = b.ok;
    a.ld = b.ld; a.size = b.size; a.B = b.B;
    a.idx = b.idx + p * b.B;
    a.seed = 0;
    a.gamma = static_cast<float>(b.hyper[p * HYPER + H_GAMMA]);
    a.tiles_per_wave = b.tiles_per_wave;
    a.loss_ref = b.loss_ref;
    char* const region = b.ws + p * b.region;
    a.ws_t = reinterpret_cast<uint64_t*>(region);
    a.ws = reinterpret_cast<float*>(region + WS_HEADER);
    a.idx_out = b.idx_out != nullptr ? b.idx_out + p * b.B : nullptr;
    a.weight = b.weight + p * b.B;
    a.td_out = b.td_out + p * b.B;
    grad_body<STRAT, true>(a, blockIdx.x);
}

__global__ __launch_bounds__(APPLY_BLOCK) void prio_apply_kernel(const PrioApplyArgs b)
{
    const int64_t p = blockIdx.y;
    // (p's row of the table through a vector register, as in lbank_apply_kernel: the doubles then live in VGPRs)
    const double* hy = b.hyper + p * HYPER;
    asm volatile("" : "+v"(hy));
    ApplyArgs a;
    a.theta = b.theta + p * PARAMS;
    a.theta_target = b.theta_target + p * PARAMS;
    a.m = b.m + p * PARAMS;
    a.v = b.v + p * PARAMS;
    a.t_dev = b.t_dev + p;
    const char* const region = b.ws + p * b.region;
    a.ws_t = reinterpret_cast<const uint64_t*>(region);
    a.ws = reinterpret_cast<const float*>(region + WS_HEADER);
    a.partials = b.partials;
    a.tau = hy[H_TAU]; a.lr = hy[H_LR]; a.beta1 = hy[H_BETA1]; a.beta2 = hy[H_BETA2]; a.eps = hy[H_EPS];
    a.blob_online = b.blob_online != nullptr ? b.blob_online + p * b.blob_floats : nullptr;
    a.blob_target = b.blob_target != nullptr ? b.blob_target + p * b.blob_floats : nullptr;
    a.perm = b.perm;
    a.blob_floats = b.blob_floats;
    a.grad_out = b.grad_out != nullptr ? b.grad_out + p * PARAMS : nullptr;
    a.loss = b.loss != nullptr ? b.loss + p : nullptr;
    apply_body(a, blockIdx.x);
}

// ------------------------------------------------------------------ host side
int64_t pad64(int64_t n) { return (n + FAN - 1) / FAN * FAN; }

int check_shape(int64_t capacity, int64_t N, int64_t seg, int64_t P)
{
    if (capacity <= 0 || capacity > AQUAPRIO_MAX_CAPACITY)
        return fail(AQUAPRIO_E_INVALID, "capacity=%lld: must be in [1, %d]", (long long)capacity, AQUAPRIO_MAX_CAPACITY);
    if (N < 1 || N > capacity) return fail(AQUAPRIO_E_INVALID, "N=%lld: must be in [1, capacity=%lld]", (long long)N, (long long)capacity);
    if (capacity % N != 0)
        return fail(AQUAPRIO_E_INVALID, "capacity=%lld is no multiple of N=%lld: a slot would not belong to one world", (long long)capacity, (long long)N);
    if (seg < 1 || seg > N) return fail(AQUAPRIO_E_INVALID, "seg=%lld: must be in [1, N=%lld]", (long long)seg, (long long)N);
    if (P < 1 || P > AQUAPRIO_MAX_NETWORKS) return fail(AQUAPRIO_E_INVALID, "P=%lld: must be in [1, %d]", (long long)P, AQUAPRIO_MAX_NETWORKS);
    return 0;
}

// (a validated shape)
Layout layout_of(int64_t capacity, int64_t N, int64_t seg, int64_t P)
{
    Layout y = {};
    y.L0 = capacity / N * seg;
    int k = 0;
    int64_t n = y.L0, off = 0;
    for (;;) {
        y.n[k] = n;
        y.stride[k] = pad64(n);
        y.off[k] = off;
        off += P * y.stride[k] * (k == 0 ? 4 : 8);
        off = (off + 511) / 512 * 512;
        ++k;
        if (k > 1 && n == 1) break;
        n = (n + FAN - 1) / FAN;
    }
    y.levels = k;
    y.total = off;
    return y;
}

int check_tree(const void* tree, size_t tree_bytes, int64_t capacity, int64_t N, int64_t seg, int64_t P, Tree* out)
{
    if (int rc = check_shape(capacity, N, seg, P)) return rc;
    if (tree == nullptr) return fail(AQUAPRIO_E_INVALID, "tree is NULL");
    const Layout y = layout_of(capacity, N, seg, P);
    if (tree_bytes < static_cast<size_t>(y.total))
        return fail(AQUAPRIO_E_INVALID, "tree_bytes=%zu: below the %lld bytes of aquaprio_layout", tree_bytes, (long long)y.total);
    if (!aligned(tree, 512)) return fail(AQUAPRIO_E_ALIGN, "tree must be 512-byte aligned");
    out->base = static_cast<char*>(const_cast<void*>(tree));
    out->levels = y.levels;
    out->capacity = static_cast<int32_t>(capacity); out->N = static_cast<int32_t>(N); out->seg = static_cast<int32_t>(seg);
    out->P = static_cast<int32_t>(P);
    for (int k = 0; k < LEVELS; ++k) { out->stride[k] = y.stride[k]; out->off[k] = y.off[k]; }
    return 0;
}

unsigned grid_of(int64_t n)
{
    int64_t blocks = (n + PBLOCK - 1) / PBLOCK;
    if (blocks > PMAX_BLOCKS) blocks = PMAX_BLOCKS;
    return static_cast<unsigned>(blocks < 1 ? 1 : blocks);
}

bool in_unit(double x) { return is_number(x) && x >= 0.0 && x <= 1.0; }

int check_batch(int64_t B)
{
    if (B < 0 || B > AQUAPRIO_MAX_BATCH) return fail(AQUAPRIO_E_INVALID, "B=%lld: must be in [0, %d]", (long long)B, AQUAPRIO_MAX_BATCH);
    return 0;
}

int check_quantiser(double alpha, double eps)
{
    if (!in_unit(alpha)) return fail(AQUAPRIO_E_INVALID, "alpha=%g: must be in [0, 1]", alpha);
    if (!is_number(eps) || !(eps >= 1e-300 && eps <= 1e300)) return fail(AQUAPRIO_E_INVALID, "eps=%g: must be in [1e-300, 1e300]", eps);
    return 0;
}

int check_anneal(double beta0, int64_t anneal)
{
    if (!in_unit(beta0)) return fail(AQUAPRIO_E_INVALID, "beta0=%g: must be in [0, 1]", beta0);
    if (anneal < 1) return fail(AQUAPRIO_E_INVALID, "anneal=%lld: must be >= 1", (long long)anneal);
    return 0;
}

// do [a, a + bytes) and [b, b + bytes) share a byte?
bool overlap(const void* a, const void* b, size_t bytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y ? y - x < bytes : x - y < bytes;
}

}  // namespace

extern "C" {

int aquaprio_version(void) { return AQUAPRIO_ABI_VERSION; }
const char* aquaprio_last_error(void) { return g_err; }

int aquaprio_layout(int64_t capacity, int64_t N, int64_t seg, int64_t P, int64_t* out_host)
{
    if (int rc = check_shape(capacity, N, seg, P)) return rc;
    if (out_host == nullptr) return fail(AQUAPRIO_E_INVALID, "out is NULL");
    if (!aligned(out_host, 8)) return fail(AQUAPRIO_E_ALIGN, "out must be 8-byte aligned");
    const Layout y = layout_of(capacity, N, seg, P);
    for (int i = 0; i < AQUAPRIO_LAYOUT_WORDS; ++i) out_host[i] = 0;
    out_host[0] = y.levels; out_host[1] = y.total; out_host[2] = y.L0;
    for (int k = 0; k < y.levels; ++k) {
        out_host[3 + 3 * k] = y.n[k];
        out_host[3 + 3 * k + 1] = y.stride[k];
        out_host[3 + 3 * k + 2] = y.off[k];
    }
    return 0;
}

double aquaprio_pow(double x, double e)
{
    if (!is_number(x) || !(x >= 0x1p-1000 && x <= 0x1p1000)) { fail(AQUAPRIO_E_INVALID, "x=%g: must be in [2^-1000, 2^1000]", x); return -1.0; }
    if (!is_number(e) || !(e >= -1.0 && e <= 1.0)) { fail(AQUAPRIO_E_INVALID, "e=%g: must be in [-1, 1]", e); return -1.0; }
    return pow_of(x, e);
}

uint32_t aquaprio_quantise(double td, double alpha, double eps)
{
    if (!is_number(td) || !(td >= 0.0 && td <= 1e300)) { fail(AQUAPRIO_E_INVALID, "td=%g: must be in [0, 1e300]", td); return 0; }
    if (check_quantiser(alpha, eps)) return 0;
    return quantise_of(td, alpha, eps);
}

double aquaprio_beta(uint64_t t, double beta0, int64_t anneal)
{
    if (check_anneal(beta0, anneal)) return -1.0;
    return beta_of(t, beta0, anneal);
}

double aquaprio_weight(uint64_t size, uint32_t q, uint64_t T, double beta)
{
    if (size < 1) { fail(AQUAPRIO_E_INVALID, "size=0: must be >= 1"); return -1.0; }
    if (q < 1 || q > AQUAPRIO_QMAX) { fail(AQUAPRIO_E_INVALID, "q=%u: must be in [1, %d]", q, AQUAPRIO_QMAX); return -1.0; }
    if (T < q || T >= (1ull << 62)) { fail(AQUAPRIO_E_INVALID, "T=%llu: must be in [q, 2^62)", (unsigned long long)T); return -1.0; }
    if (!in_unit(beta)) { fail(AQUAPRIO_E_INVALID, "beta=%g: must be in [0, 1]", beta); return -1.0; }
    return weight_of(size, q, T, beta);
}

int aquaprio_insert(void* tree, size_t tree_bytes, uint32_t* pmax, int64_t capacity, int64_t N, int64_t seg, int64_t P,
                    const int64_t* header, const uint8_t* ok, void* stream)
{
    InsertArgs k;
    if (int rc = check_tree(tree, tree_bytes, capacity, N, seg, P, &k.t)) return rc;
    if (pmax == nullptr) return fail(AQUAPRIO_E_INVALID, "pmax is NULL");
    if (header == nullptr || ok == nullptr) return fail(AQUAPRIO_E_INVALID, "header or ok is NULL");
    if (!aligned(header, 8)) return fail(AQUAPRIO_E_ALIGN, "header must be 8-byte aligned");
    if (!aligned(pmax, 4)) return fail(AQUAPRIO_E_ALIGN, "pmax must be 4-byte aligned");
    k.pmax = pmax; k.header = header; k.ok = ok;
    hipLaunchKernelGGL(prio_insert_kernel, dim3(grid_of(N)), dim3(PBLOCK), 0, static_cast<hipStream_t>(stream), k);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "prio_insert_kernel launch");
    return 0;
}

int aquaprio_set(void* tree, size_t tree_bytes, uint32_t* pmax, int64_t capacity, int64_t N, int64_t seg, int64_t P,
                 const int32_t* idx, const float* td, int64_t B, double alpha, double eps, void* stream)
{
    SetArgs k;
    if (int rc = check_tree(tree, tree_bytes, capacity, N, seg, P, &k.t)) return rc;
    if (pmax == nullptr) return fail(AQUAPRIO_E_INVALID, "pmax is NULL");
    if (int rc = check_batch(B)) return rc;
    if (int rc = check_quantiser(alpha, eps)) return rc;
    if (!aligned(pmax, 4) || !aligned(idx, 4) || !aligned(td, 4)) return fail(AQUAPRIO_E_ALIGN, "pmax / idx / td must be 4-byte aligned");
    if (B == 0) return 0;
    if (idx == nullptr || td == nullptr) return fail(AQUAPRIO_E_INVALID, "idx or td is NULL");
    k.pmax = pmax; k.idx = idx; k.td = td; k.B = B; k.alpha = alpha; k.eps = eps;
    hipLaunchKernelGGL(prio_set_kernel, dim3(grid_of(P * B)), dim3(PBLOCK), 0, static_cast<hipStream_t>(stream), k);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "prio_set_kernel launch");
    return 0;
}

int aquaprio_draw(const void* tree, size_t tree_bytes, int64_t capacity, int64_t N, int64_t seg, int64_t P,
                  const int64_t* header, const uint64_t* t_dev, const uint64_t* seed_dev, int32_t* idx, float* weight,
                  uint32_t* q_out, int64_t B, double beta0, int64_t anneal, void* stream)
{
    DrawArgs k;
    if (int rc = check_tree(tree, tree_bytes, capacity, N, seg, P, &k.t)) return rc;
    if (header == nullptr || t_dev == nullptr || seed_dev == nullptr) return fail(AQUAPRIO_E_INVALID, "header, t_dev or seed_dev is NULL");
    if (int rc = check_batch(B)) return rc;
    if (int rc = check_anneal(beta0, anneal)) return rc;
    if (!aligned(header, 8) || !aligned(t_dev, 8) || !aligned(seed_dev, 8)) return fail(AQUAPRIO_E_ALIGN, "header / t_dev / seed_dev must be 8-byte aligned");
    if (!aligned(idx, 4) || !aligned(weight, 4) || !aligned(q_out, 4)) return fail(AQUAPRIO_E_ALIGN, "idx / weight / q_out must be 4-byte aligned");
    if (B == 0) return 0;
    if (idx == nullptr || weight == nullptr || q_out == nullptr) return fail(AQUAPRIO_E_INVALID, "idx, weight or q_out is NULL");
    k.header = header; k.t_dev = t_dev; k.seed = seed_dev; k.idx = idx; k.weight = weight; k.q_out = q_out; k.B = B;
    k.beta0 = beta0; k.anneal = anneal;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int64_t blocks = (B + PWAVES - 1) / PWAVES;
    if (blocks > PMAX_BLOCKS) blocks = PMAX_BLOCKS;
    hipLaunchKernelGGL(prio_descend_kernel, dim3(static_cast<unsigned>(blocks), static_cast<unsigned>(P)), dim3(PBLOCK), 0, st, k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "prio_descend_kernel launch");
    hipLaunchKernelGGL(prio_weight_kernel, dim3(static_cast<unsigned>(P)), dim3(PBLOCK), 0, st, k);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "prio_weight_kernel launch");
    return 0;
}

int aquaprio_update_f32(float* theta, float* theta_target, float* m, float* v, uint64_t* t_dev, int64_t P,
                        const float* s, const uint8_t* a, const float* r, const float* s2, const uint8_t* d,
                        const uint8_t* ok, int64_t ld, int64_t size,
                        const int32_t* idx, int64_t B, int strategy, const double* hyper_dev,
                        float* blob_online, float* blob_target, const int32_t* perm, int64_t blob_floats,
                        void* workspace, size_t workspace_bytes,
                        int32_t* idx_out, float* grad_out, float* loss,
                        const float* weight, float* td_out, void* stream)
{
    if (P < 1 || P > AQUAPRIO_MAX_NETWORKS) return fail(AQUAPRIO_E_INVALID, "P=%lld: must be in [1, %d]", (long long)P, AQUAPRIO_MAX_NETWORKS);
    if (theta == nullptr || theta_target == nullptr || m == nullptr || v == nullptr || t_dev == nullptr)
        return fail(AQUAPRIO_E_INVALID, "theta, theta_target, m, v or t is NULL");
    const size_t stack = static_cast<size_t>(P) * PARAMS * sizeof(float);
    if (overlap(theta, theta_target, stack) || overlap(theta, m, stack) || overlap(theta, v, stack) || overlap(theta_target, m, stack) ||
        overlap(theta_target, v, stack) || overlap(m, v, stack))
        return fail(AQUAPRIO_E_INVALID, "theta, theta_target, m and v must be four arrays of P x %d floats that do not overlap", PARAMS);
    if (int rc = check_batch(B)) return rc;
    if (ld < 0 || size < 0 || size > ld || ld > INT32_MAX)
        return fail(AQUAPRIO_E_INVALID, "bad ring sizes: size=%lld ld=%lld", (long long)size, (long long)ld);
    const int loss_ref = (strategy & AQUALRN_LOSS_REFERENCE) != 0 ? 1 : 0;
    if (strategy >= 0) strategy &= ~AQUALRN_LOSS_REFERENCE;          // what is left: the bootstrap strategy, no other bit
    if (strategy < AQUALRN_DOUBLE_REF || strategy > AQUALRN_STANDARD) return fail(AQUAPRIO_E_INVALID, "strategy=%d: unknown", strategy);
    if (hyper_dev == nullptr) return fail(AQUAPRIO_E_INVALID, "the hyper-parameter table is NULL");
    if ((blob_online != nullptr || blob_target != nullptr) && perm == nullptr)
        return fail(AQUAPRIO_E_INVALID, "a blob is given without the permutation table");
    if ((blob_online != nullptr || blob_target != nullptr) && blob_floats < AQUALBANK_PARAMS)
        return fail(AQUAPRIO_E_INVALID, "blob_floats=%lld < %d", (long long)blob_floats, AQUALBANK_PARAMS);
    if ((blob_online != nullptr || blob_target != nullptr) && blob_floats > INT32_MAX)
        return fail(AQUAPRIO_E_INVALID, "blob_floats=%lld: above %d", (long long)blob_floats, INT32_MAX);
    if (blob_online != nullptr && blob_target != nullptr && overlap(blob_online, blob_target, static_cast<size_t>(P) * blob_floats * sizeof(float)))
        return fail(AQUAPRIO_E_INVALID, "blob_online and blob_target overlap");
    if (!aligned(theta, 4) || !aligned(theta_target, 4) || !aligned(m, 4) || !aligned(v, 4))
        return fail(AQUAPRIO_E_ALIGN, "theta / theta_target / m / v must be 4-byte aligned");
    if (!aligned(t_dev, 8) || !aligned(hyper_dev, 8)) return fail(AQUAPRIO_E_ALIGN, "t and the hyper-parameter table must be 8-byte aligned");
    if (!aligned(s, 4) || !aligned(s2, 4) || !aligned(r, 4)) return fail(AQUAPRIO_E_ALIGN, "s / s2 / r must be 4-byte aligned");
    if (!aligned(idx, 4) || !aligned(idx_out, 4) || !aligned(perm, 4)) return fail(AQUAPRIO_E_ALIGN, "idx / idx_out / perm must be 4-byte aligned");
    if (!aligned(blob_online, 4) || !aligned(blob_target, 4) || !aligned(grad_out, 4) || !aligned(loss, 4))
        return fail(AQUAPRIO_E_ALIGN, "blobs / grad_out / loss must be 4-byte aligned");
    if (!aligned(weight, 4) || !aligned(td_out, 4)) return fail(AQUAPRIO_E_ALIGN, "weight / td_out must be 4-byte aligned");
    if (!aligned(workspace, 16)) return fail(AQUAPRIO_E_ALIGN, "the workspace must be 16-byte aligned");
    if (B == 0) return 0;
    if (idx == nullptr) return fail(AQUAPRIO_E_INVALID, "idx is NULL: the draw is aquaprio_draw's");
    if (weight == nullptr || td_out == nullptr) return fail(AQUAPRIO_E_INVALID, "weight or td_out is NULL: both are required");
    if (s == nullptr || a == nullptr || r == nullptr || s2 == nullptr || d == nullptr || ok == nullptr)
        return fail(AQUAPRIO_E_INVALID, "a ring buffer is NULL");
    if (workspace == nullptr) return fail(AQUAPRIO_E_INVALID, "workspace is NULL");
    const size_t need = static_cast<size_t>(P) * workspace_region(B);
    if (workspace_bytes < need) return fail(AQUAPRIO_E_INVALID, "workspace too small: %zu < %zu bytes", workspace_bytes, need);

    const Shape sh = shape_of(B);
    PrioGradArgs g;
    g.theta = theta; g.theta_target = theta_target; g.t_dev = t_dev;
    g.s = s; g.a = a; g.r = r; g.s2 = s2; g.d = d; g.ok = ok;
    g.ld = ld; g.size = size; g.B = B; g.idx = idx; g.hyper = hyper_dev;
    g.tiles_per_wave = sh.tiles_per_wave;
    g.loss_ref = loss_ref;
    g.ws = static_cast<char*>(workspace);
    g.region = static_cast<int64_t>(workspace_region(B));
    g.idx_out = idx_out;
    g.weight = weight; g.td_out = td_out;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned>(sh.groups), static_cast<unsigned>(P)), block(BLOCK);
    switch (strategy) {
    case AQUALRN_DOUBLE_REF: hipLaunchKernelGGL((prio_grad_kernel<AQUALRN_DOUBLE_REF>), grid, block, 0, st, g); break;
    case AQUALRN_DOUBLE: hipLaunchKernelGGL((prio_grad_kernel<AQUALRN_DOUBLE>), grid, block, 0, st, g); break;
    case AQUALRN_FIXED: hipLaunchKernelGGL((prio_grad_kernel<AQUALRN_FIXED>), grid, block, 0, st, g); break;
    default: hipLaunchKernelGGL((prio_grad_kernel<AQUALRN_STANDARD>), grid, block, 0, st, g); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "prio_grad_kernel launch");

    PrioApplyArgs q;
    q.theta = theta; q.theta_target = theta_target; q.m = m; q.v = v; q.t_dev = t_dev;
    q.ws = g.ws; q.region = g.region; q.partials = sh.groups; q.hyper = hyper_dev;
    q.blob_online = blob_online; q.blob_target = blob_target; q.perm = perm; q.blob_floats = blob_floats;
    q.grad_out = grad_out; q.loss = loss;
    hipLaunchKernelGGL(prio_apply_kernel, dim3(APPLY_GROUPS, static_cast<unsigned>(P)), dim3(APPLY_BLOCK), 0, st, q);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "prio_apply_kernel launch");
    return 0;
}

}  // extern "C"
