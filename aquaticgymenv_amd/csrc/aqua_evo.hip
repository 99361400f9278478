// aqua_evo.hip -- libaqua_evo.so (csrc/aqua_evo.h): natural evolution strategies on a bank of Q-networks.  Its own
// translation unit and library: the other sixteen libraries and their kernels are not touched.
//
// Six kernels.
//   evo_ask_kernel     grid (parameter chunks, pairs): a thread computes the noise of (pair j, parameter i) once and stores
//                      both signs through perm; row H of an odd P copies the centre.
//   evo_zero_kernel, evo_accumulate_kernel, evo_finish_kernel: the fitness.  The accumulation is one thread per log record
//                      or unfinished world, grid-stride above MAX_BLOCKS blocks, int64 atomic adds on (sum, count,
//                      successes) of the segment: integer sums, the same in any order.
//   evo_rank_kernel    ONE workgroup: the keys in LDS, every thread counts the keys below and equal to its own (no sort, so no
//                      order of a sort enters), the rank differences, and the scalar bookkeeping.
//   evo_step_kernel    one wavefront per parameter: the lanes share the pairs, an integer wave reduction gives G, lane 0 takes
//                      the optimiser step.
// No floating-point atomics, no block waits on another block.  Floating point: float64, every operation rounded, nothing
// contracted -- the functions that compute carry `#pragma clang fp contract(off)` and are the ones the host entries run.
#include <hip/hip_runtime.h>

#include <cmath>

#include "aqua_evo.h"
#include "aqua_host.hpp"

namespace {

constexpr int BLOCK = AQUAEVO_BLOCK;
constexpr int MAX_BLOCKS = AQUAEVO_MAX_BLOCKS;
constexpr int PARAMS = AQUAEVO_PARAMS;
constexpr int RANK_BLOCK = 1024;
constexpr int RANK_OWN = AQUAEVO_MAX_NETWORKS / RANK_BLOCK;      // slots a thread of the ranking owns at most
constexpr int WAVE = 64;
constexpr uint32_t STREAM_EVO = AQUAEVO_STREAM;
constexpr double NOISE_C = AQUAEVO_C;

static_assert(STREAM_EVO != 0 && STREAM_EVO != 1 && STREAM_EVO != 3 && STREAM_EVO != 4 && STREAM_EVO != 5 && STREAM_EVO != 6 &&
              STREAM_EVO != 7 && STREAM_EVO != 8 && STREAM_EVO < 256,
              "a Philox stream of its own: 0, 1, 3, 4 are the environment's, 5 the policies', 6 the minibatch draws', 7 the "
              "selector's and the sum trees', 8 the hindsight draws'");
static_assert(AQUAEVO_MAX_NETWORKS % RANK_BLOCK == 0 && AQUAEVO_MAX_NETWORKS % 4 == 0, "whole quads of keys per thread");
static_assert(BLOCK % WAVE == 0, "whole wavefronts");

// Philox4x32-10 (Salmon et al., SC'11) as aqua_device.hpp states it, for host and device
__host__ __device__ inline void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t (&out)[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = static_cast<uint64_t>(c0) * 0xD2511F53ull;
        const uint64_t p1 = static_cast<uint64_t>(c2) * 0xCD9E8D57ull;
        const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
        c1 = static_cast<uint32_t>(p1);
        c3 = static_cast<uint32_t>(p0);
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// THE statement of the noise: the integer numerator n of (generation g, pair j, parameter i); eps = (double)n * NOISE_C
__host__ __device__ inline int32_t noise_of(uint64_t seed, uint64_t g, uint32_t j, uint32_t i)
{
    uint32_t r[4];
    const uint32_t c3 = (static_cast<uint32_t>(g >> 32) & 0xFFFFu) | (STREAM_EVO << 24);      // attempt 0
    philox4x32_10(static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), i, j, static_cast<uint32_t>(g), c3, r);
    uint32_t S = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) S += (r[w] & 0xFFFFu) + (r[w] >> 16);
    return 2 * static_cast<int32_t>(S) - AQUAEVO_NOISE_OFFSET;
}

// the two members of a pair: (float)(theta + d) and (float)(theta - d), d = sigma * eps
__host__ __device__ inline void perturb_of(float theta, double sigma, int32_t n, float& plus, float& minus)
{
#pragma clang fp contract(off)
    const double e = static_cast<double>(n) * NOISE_C;
    const double d = sigma * e;
    const double c = static_cast<double>(theta);
    const double xp = c + d;
    const double xm = c - d;
    plus = static_cast<float>(xp);
    minus = static_cast<float>(xm);
}

// float32 <-> its bits.  The library is built with -fno-honor-nans: a NaN test on the bits of a FLOAT value is recognised as a
// floating-point class test and folded away, so what may be a NaN travels as the integer it was loaded as, and the host entry
// hides the origin of its argument's bits from the optimiser.
__host__ __device__ inline float float_of(uint32_t u)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float x;
    std::memcpy(&x, &u, sizeof(x));
    return x;
#endif
}

inline uint32_t host_bits_of(float x)
{
    uint32_t u;
    std::memcpy(&u, &x, sizeof(u));
    asm volatile("" : "+r"(u));
    return u;
}

// THE statement of the quantisation
__host__ __device__ inline int64_t quantise_of(uint32_t u)
{
#pragma clang fp contract(off)
    const bool nan = (u & 0x7F800000u) == 0x7F800000u && (u & 0x007FFFFFu) != 0;       // by the bits: -fno-honor-nans
    double x = static_cast<double>(float_of(nan ? 0u : u));
    x = x > static_cast<double>(AQUAEVO_CLAMP) ? static_cast<double>(AQUAEVO_CLAMP) : x;
    x = x < -static_cast<double>(AQUAEVO_CLAMP) ? -static_cast<double>(AQUAEVO_CLAMP) : x;
    return static_cast<int64_t>(rint(x * static_cast<double>(1 << AQUAEVO_FIX_BITS)));   // |.| <= 2^31: ties to even, then exact
}

// THE statement of the key: ascending keys are ascending fitness, every bit pattern has a place (aquapbt_select's)
__host__ __device__ inline uint32_t key_of(uint32_t u) { return (u >> 31) ? ~u : (u | 0x80000000u); }

// b^t in float64 by binary exponentiation, least-significant bit first
__host__ __device__ __forceinline__ double power_of(double b, uint64_t t)
{
#pragma clang fp contract(off)
    double result = 1.0, base = b;
    for (uint64_t n = t; n != 0; n >>= 1) {
        if (n & 1u) result *= base;
        base *= base;
    }
    return result;
}

struct Optimiser {
    double sigma, lr, beta1, beta2, eps, weight_decay;
    int optimizer;
};

struct Stepped {
    float theta, m, v;
    double grad;
};

// THE statement of steps 2 .. 6 for one parameter; t is the incremented counter
__host__ __device__ __forceinline__ Stepped step_of(int64_t G, int64_t H, const Optimiser& o, uint64_t t, float theta, float m, float v)
{
#pragma clang fp contract(off)
    const double D = static_cast<double>(4 * H * (2 * H - 1)) * o.sigma;
    const double scale = NOISE_C / D;
    const double ghat = static_cast<double>(G) * scale;
    const double th = static_cast<double>(theta);
    const double decay = o.weight_decay * th;
    const double grad = decay - ghat;
    if (o.optimizer == AQUAEVO_SGD) {
        const double move = o.lr * grad;
        return {static_cast<float>(th - move), m, v, grad};
    }
    const double a1 = o.beta1 * static_cast<double>(m);
    const double b1 = (1.0 - o.beta1) * grad;
    const double md = a1 + b1;
    const double sq = grad * grad;
    const double a2 = o.beta2 * static_cast<double>(v);
    const double b2 = (1.0 - o.beta2) * sq;
    const double vd = a2 + b2;
    const double c1 = 1.0 - power_of(o.beta1, t);
    const double c2 = 1.0 - power_of(o.beta2, t);
    const double mhat = md / c1;
    const double vhat = vd / c2;
    const double root = sqrt(vhat);
    const double den = root + o.eps;
    const double num = o.lr * mhat;
    const double move = num / den;
    return {static_cast<float>(th - move), static_cast<float>(md), static_cast<float>(vd), grad};
}

// ------------------------------------------------------------------ ask
struct AskArgs {
    const uint32_t* theta;
    const int32_t* perm;
    const unsigned long long* header;
    float* blob;
    double sigma;
    uint64_t seed;
    uint32_t H, odd, blob_floats;
};

__global__ __launch_bounds__(BLOCK) void evo_ask_kernel(const AskArgs a)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x, j = blockIdx.y;      // j <= H, and j == H only with an odd P
    if (i >= static_cast<uint32_t>(PARAMS)) return;
    const int32_t at = a.perm[i];
    if (at < 0 || static_cast<uint32_t>(at) >= a.blob_floats) return;        // never an address
    const uint32_t th = a.theta[i];
    if (j >= a.H) {
        if (a.odd) reinterpret_cast<uint32_t*>(a.blob)[static_cast<size_t>(2) * a.H * a.blob_floats + at] = th;
        return;
    }
    const uint64_t g = a.header[AQUAEVO_H_GENERATION];
    float plus, minus;
    perturb_of(__uint_as_float(th), a.sigma, noise_of(a.seed, g, j, i), plus, minus);
    float* row = a.blob + static_cast<size_t>(2) * j * a.blob_floats;
    row[at] = plus;
    row[a.blob_floats + at] = minus;
}

// ------------------------------------------------------------------ fitness
struct FitnessArgs {
    const uint32_t* log_ret;
    const uint8_t* log_code;
    const int64_t* log_world;
    const unsigned long long* counts;
    const uint32_t* ret;
    const uint8_t* finished;
    int64_t C, env_offset, limit;                     // limit = min(N, P seg): the local worlds that belong to a segment
    uint32_t seg, P;
    int kind;
    long long* acc;
    uint32_t* fitness;
    long long* episodes;
};

__global__ __launch_bounds__(BLOCK) void evo_zero_kernel(long long* acc, uint32_t words)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < words) acc[i] = 0;
}

__device__ __forceinline__ void account(const FitnessArgs& a, int64_t local, uint32_t ret, bool success)
{
    // 0 <= local < limit <= P seg, both below 2^31: a 32-bit division
    const uint32_t p = static_cast<uint32_t>(local) / a.seg;
    long long* row = a.acc + static_cast<size_t>(p) * AQUAEVO_ACC;
    atomicAdd(reinterpret_cast<unsigned long long*>(row), static_cast<unsigned long long>(quantise_of(ret)));
    atomicAdd(reinterpret_cast<unsigned long long*>(row + 1), 1ull);
    if (success) atomicAdd(reinterpret_cast<unsigned long long*>(row + 2), 1ull);
}

__global__ __launch_bounds__(BLOCK) void evo_accumulate_kernel(const FitnessArgs a)
{
    const unsigned long long cursor = a.counts[0];
    const int64_t records = cursor < static_cast<unsigned long long>(a.C) ? static_cast<int64_t>(cursor) : a.C;
    const int64_t worlds = a.finished != nullptr ? a.limit : 0;
    const int64_t total = a.C + worlds;               // items C .. C + worlds - 1 are the local worlds
    const int64_t stride = static_cast<int64_t>(gridDim.x) * BLOCK;
    for (int64_t k = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x; k < total; k += stride) {
        if (k < a.C) {
            if (k >= records) continue;
            const int64_t w = a.log_world[k];
            if (w < a.env_offset || w - a.env_offset >= a.limit) continue;     // (env_offset <= w: no overflow)
            account(a, w - a.env_offset, a.log_ret[k], a.log_code[k] == AQUAEVO_TERM_SUCCESS);
        } else {
            const int64_t w = k - a.C;
            if (a.finished[w] == 0) account(a, w, a.ret[w], false);
        }
    }
}

__global__ __launch_bounds__(BLOCK) void evo_finish_kernel(const FitnessArgs a)
{
#pragma clang fp contract(off)
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.P) return;
    const long long* row = a.acc + static_cast<size_t>(p) * AQUAEVO_ACC;
    const long long sum = row[0], count = row[1], wins = row[2];
    uint32_t out = 0xFF800000u;                       // -infinity: nothing flown
    if (count != 0) {
        const double n = static_cast<double>(count);
        double f;
        if (a.kind == AQUAEVO_MEAN_RETURN) {
            const double s = static_cast<double>(sum) / 1048576.0;
            f = s / n;
        } else {
            f = static_cast<double>(wins) / n;
        }
        out = __float_as_uint(static_cast<float>(f));
    }
    a.fitness[p] = out;
    a.episodes[p] = count;
}

// ------------------------------------------------------------------ tell
struct RankArgs {
    const uint32_t* fitness;
    unsigned long long* header;
    unsigned long long* t;
    int32_t* rank2;
    int32_t* weights;
    uint32_t H;
};

__global__ __launch_bounds__(RANK_BLOCK) void evo_rank_kernel(const RankArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_key[AQUAEVO_MAX_NETWORKS];
    __shared__ int32_t s_rank[AQUAEVO_MAX_NETWORKS];
    __shared__ unsigned long long s_best;
    const uint32_t tid = threadIdx.x, threads = blockDim.x, n = 2 * a.H;

    if (tid == 0) s_best = 0;
    for (uint32_t p = tid; p < n; p += threads) s_key[p] = key_of(a.fitness[p]);
    __syncthreads();

    // this thread's slots: tid, tid + threads, ...; every quad of keys is read once for all of them
    uint32_t mine[RANK_OWN], lt[RANK_OWN], eq[RANK_OWN];
#pragma unroll
    for (int o = 0; o < RANK_OWN; ++o) {
        const uint32_t p = tid + o * threads;
        mine[o] = p < n ? s_key[p] : 0u;
        lt[o] = 0;
        eq[o] = 0;
    }
    if (tid < n) {                                    // (n is even: the tail is a pair or nothing)
        const uint32_t quads = n / 4;
        for (uint32_t q = 0; q < quads; ++q) {
            const uint4 k = reinterpret_cast<const uint4*>(s_key)[q];
#pragma unroll
            for (int o = 0; o < RANK_OWN; ++o) {
                lt[o] += (k.x < mine[o]) + (k.y < mine[o]) + (k.z < mine[o]) + (k.w < mine[o]);
                eq[o] += (k.x == mine[o]) + (k.y == mine[o]) + (k.z == mine[o]) + (k.w == mine[o]);
            }
        }
        for (uint32_t q = quads * 4; q < n; ++q) {
            const uint32_t k = s_key[q];
#pragma unroll
            for (int o = 0; o < RANK_OWN; ++o) {
                lt[o] += k < mine[o];
                eq[o] += k == mine[o];
            }
        }
        unsigned long long best = 0;
#pragma unroll
        for (int o = 0; o < RANK_OWN; ++o) {
            const uint32_t p = tid + o * threads;
            if (p < n) {
                const int32_t r = static_cast<int32_t>(2 * lt[o] + eq[o]) - 1;
                s_rank[p] = r;
                a.rank2[p] = r;
                // the highest key, the lowest index on a tie (p < 4096: the word is never 0)
                const unsigned long long word = (static_cast<unsigned long long>(mine[o]) << 32) | (0xFFFFFFFFu - p);
                best = word > best ? word : best;
            }
        }
        atomicMax(&s_best, best);                     // (an integer maximum in LDS)
    }
    __syncthreads();
    for (uint32_t j = tid; j < a.H; j += threads) a.weights[j] = s_rank[2 * j] - s_rank[2 * j + 1];
    if (tid == 0) {
        const unsigned long long g = a.header[AQUAEVO_H_GENERATION];
        a.header[AQUAEVO_H_GENERATION] = g + 1;
        a.header[AQUAEVO_H_TELLS] = a.header[AQUAEVO_H_TELLS] + 1;
        a.header[AQUAEVO_H_STEPPED] = g;
        a.header[AQUAEVO_H_BEST] = n == 0 ? AQUAEVO_NO_SLOT : static_cast<unsigned long long>(0xFFFFFFFFu - static_cast<uint32_t>(s_best));
        a.header[AQUAEVO_H_RANKED] = n;
        a.t[0] = a.t[0] + 1;
    }
}

struct StepArgs {
    const int32_t* weights;
    const unsigned long long* header;
    const unsigned long long* t;
    float* theta;
    float* m;
    float* v;
    double* grad_out;
    uint64_t seed;
    uint32_t H;
    Optimiser o;
};

__global__ __launch_bounds__(BLOCK) void evo_step_kernel(const StepArgs a)
{
    const uint32_t lane = threadIdx.x % WAVE;
    const uint32_t i = blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;      // one wavefront per parameter
    if (i >= static_cast<uint32_t>(PARAMS)) return;                           // (a whole wavefront leaves)
    const uint64_t g = a.header[AQUAEVO_H_STEPPED];
    long long G = 0;
    for (uint32_t j = lane; j < a.H; j += WAVE)
        G += static_cast<long long>(a.weights[j]) * noise_of(a.seed, g, j, i);
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) G += __shfl_xor(G, off, WAVE);
    if (lane != 0) return;
    const Stepped s = step_of(G, a.H, a.o, a.t[0], a.theta[i], a.m[i], a.v[i]);
    a.theta[i] = s.theta;
    if (a.o.optimizer == AQUAEVO_ADAM) {
        a.m[i] = s.m;
        a.v[i] = s.v;
    }
    if (a.grad_out != nullptr) a.grad_out[i] = s.grad;
}

// ------------------------------------------------------------------ host side
struct Range {
    const void* at;
    size_t bytes;
    const char* name;
};

int overlap(const Range* ranges, int count)
{
    for (int i = 0; i < count; ++i)
        for (int j = i + 1; j < count; ++j) {
            if (ranges[i].at == nullptr || ranges[j].at == nullptr || ranges[i].bytes == 0 || ranges[j].bytes == 0) continue;
            const uintptr_t x = reinterpret_cast<uintptr_t>(ranges[i].at), y = reinterpret_cast<uintptr_t>(ranges[j].at);
            if (x < y ? y - x < ranges[i].bytes : x - y < ranges[j].bytes)
                return fail(AQUAEVO_E_INVALID, "%s and %s overlap", ranges[i].name, ranges[j].name);
        }
    return 0;
}

// finite, by the bits, with their origin hidden from the optimiser: under -fno-honor-nans the exponent test of a double VALUE
// is recognised as a class test and its NaN half dropped (aqua_host.hpp's is_number let sigma = NaN through here)
bool finite(double x)
{
    uint64_t u;
    std::memcpy(&u, &x, sizeof(u));
    asm volatile("" : "+r"(u));
    return ((u >> 52) & 0x7FFu) != 0x7FFu;
}

int check_optimiser(const Optimiser& o, bool tell)
{
    if (!finite(o.sigma) || !(tell ? o.sigma > 0.0 : o.sigma >= 0.0))
        return fail(AQUAEVO_E_INVALID, "sigma=%g: must be finite and %s 0", o.sigma, tell ? ">" : ">=");
    if (!tell) return 0;
    if (!finite(o.lr) || !(o.lr >= 0.0)) return fail(AQUAEVO_E_INVALID, "lr=%g: must be finite and >= 0", o.lr);
    if (!finite(o.beta1) || !(o.beta1 >= 0.0 && o.beta1 < 1.0)) return fail(AQUAEVO_E_INVALID, "beta1=%g: must be in [0, 1)", o.beta1);
    if (!finite(o.beta2) || !(o.beta2 >= 0.0 && o.beta2 < 1.0)) return fail(AQUAEVO_E_INVALID, "beta2=%g: must be in [0, 1)", o.beta2);
    if (!finite(o.eps) || !(o.eps > 0.0)) return fail(AQUAEVO_E_INVALID, "eps=%g: must be finite and > 0", o.eps);
    if (!finite(o.weight_decay) || !(o.weight_decay >= 0.0))
        return fail(AQUAEVO_E_INVALID, "weight_decay=%g: must be finite and >= 0", o.weight_decay);
    if (o.optimizer != AQUAEVO_ADAM && o.optimizer != AQUAEVO_SGD)
        return fail(AQUAEVO_E_INVALID, "optimizer=%d: AQUAEVO_ADAM or AQUAEVO_SGD", o.optimizer);
    return 0;
}

int check_networks(int64_t P)
{
    if (P < 1 || P > AQUAEVO_MAX_NETWORKS) return fail(AQUAEVO_E_INVALID, "P=%lld: must be in [1, %d]", (long long)P, AQUAEVO_MAX_NETWORKS);
    return 0;
}

int launched(const char* what)
{
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? hip_fail(e, what) : 0;
}

}  // namespace

extern "C" {

int aquaevo_version(void) { return AQUAEVO_ABI_VERSION; }
const char* aquaevo_last_error(void) { return g_err; }

int32_t aquaevo_noise(uint64_t seed, uint64_t g, uint32_t j, uint32_t i) { return noise_of(seed, g, j, i); }
int64_t aquaevo_quantise(float ret) { return quantise_of(host_bits_of(ret)); }
uint32_t aquaevo_key(float fitness) { return key_of(host_bits_of(fitness)); }

int aquaevo_step_param(int64_t G, int64_t H, double sigma, double lr, double beta1, double beta2, double eps, double weight_decay,
                       int optimizer, uint64_t t, float io[3], double* grad)
{
    if (io == nullptr) return fail(AQUAEVO_E_INVALID, "io is NULL");
    if (H < 1 || H > AQUAEVO_MAX_NETWORKS / 2) return fail(AQUAEVO_E_INVALID, "H=%lld: must be in [1, %d]", (long long)H, AQUAEVO_MAX_NETWORKS / 2);
    if (t == 0) return fail(AQUAEVO_E_INVALID, "t=0: the incremented counter is at least 1");
    const Optimiser o = {sigma, lr, beta1, beta2, eps, weight_decay, optimizer};
    if (int rc = check_optimiser(o, true)) return rc;
    const Stepped s = step_of(G, H, o, t, io[0], io[1], io[2]);
    io[0] = s.theta; io[1] = s.m; io[2] = s.v;
    if (grad != nullptr) *grad = s.grad;
    return 0;
}

int aquaevo_ask(const float* theta, const int32_t* perm, const uint64_t* header, int64_t P, double sigma, uint64_t seed,
                float* blob, int64_t blob_floats, void* stream)
{
    if (theta == nullptr || perm == nullptr || header == nullptr || blob == nullptr)
        return fail(AQUAEVO_E_INVALID, "theta, perm, header or blob is NULL");
    if (int rc = check_networks(P)) return rc;
    Optimiser o = {};
    o.sigma = sigma;
    if (int rc = check_optimiser(o, false)) return rc;
    if (blob_floats < 4 || blob_floats > AQUAEVO_MAX_BLOB || blob_floats % 4 != 0)
        return fail(AQUAEVO_E_INVALID, "blob_floats=%lld: a multiple of 4 in [4, %d]", (long long)blob_floats, AQUAEVO_MAX_BLOB);
    const Range ranges[] = {{theta, PARAMS * sizeof(float), "theta"}, {perm, PARAMS * sizeof(int32_t), "perm"},
                            {header, AQUAEVO_HEADER * sizeof(uint64_t), "header"},
                            {blob, static_cast<size_t>(P) * static_cast<size_t>(blob_floats) * sizeof(float), "blob"}};
    if (int rc = overlap(ranges, 4)) return rc;
    if (!aligned(theta, 4) || !aligned(perm, 4)) return fail(AQUAEVO_E_ALIGN, "theta / perm must be 4-byte aligned");
    if (!aligned(header, 8)) return fail(AQUAEVO_E_ALIGN, "header must be 8-byte aligned");
    if (!aligned(blob, 16)) return fail(AQUAEVO_E_ALIGN, "blob must be 16-byte aligned");

    AskArgs k;
    k.theta = reinterpret_cast<const uint32_t*>(theta); k.perm = perm; k.header = reinterpret_cast<const unsigned long long*>(header);
    k.blob = blob; k.sigma = sigma; k.seed = seed;
    k.H = static_cast<uint32_t>(P / 2); k.odd = static_cast<uint32_t>(P % 2); k.blob_floats = static_cast<uint32_t>(blob_floats);
    hipLaunchKernelGGL(evo_ask_kernel, dim3((PARAMS + BLOCK - 1) / BLOCK, k.H + k.odd), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), k);
    return launched("evo_ask_kernel launch");
}

int aquaevo_fitness(const float* log_ret, const uint8_t* log_code, const int64_t* log_world, int64_t C, const uint64_t* counts,
                    const float* ret, const uint8_t* finished, int64_t env_offset, int64_t N, int64_t seg, int64_t P, int kind,
                    int64_t* acc, float* fitness, int64_t* episodes, void* stream)
{
    if (log_ret == nullptr || log_code == nullptr || log_world == nullptr || counts == nullptr)
        return fail(AQUAEVO_E_INVALID, "log_ret, log_code, log_world or counts is NULL");
    if ((ret == nullptr) != (finished == nullptr))
        return fail(AQUAEVO_E_INVALID, "ret and finished: give both, or neither if every world has ended");
    if (acc == nullptr || fitness == nullptr || episodes == nullptr) return fail(AQUAEVO_E_INVALID, "acc, fitness or episodes is NULL");
    if (C < 1 || C > AQUAEVO_MAX_WORLDS) return fail(AQUAEVO_E_INVALID, "C=%lld: must be in [1, %d]", (long long)C, AQUAEVO_MAX_WORLDS);
    if (env_offset < 0) return fail(AQUAEVO_E_INVALID, "env_offset=%lld: must be >= 0", (long long)env_offset);
    if (N < 0 || N > AQUAEVO_MAX_WORLDS) return fail(AQUAEVO_E_INVALID, "N=%lld: must be in [0, %d]", (long long)N, AQUAEVO_MAX_WORLDS);
    if (seg < 1 || seg > AQUAEVO_MAX_WORLDS) return fail(AQUAEVO_E_INVALID, "seg=%lld: must be in [1, %d]", (long long)seg, AQUAEVO_MAX_WORLDS);
    if (int rc = check_networks(P)) return rc;
    if (kind != AQUAEVO_MEAN_RETURN && kind != AQUAEVO_SUCCESS_RATE)
        return fail(AQUAEVO_E_INVALID, "kind=%d: AQUAEVO_MEAN_RETURN or AQUAEVO_SUCCESS_RATE", kind);
    const size_t c = static_cast<size_t>(C), n = static_cast<size_t>(N), p = static_cast<size_t>(P);
    const Range ranges[] = {{acc, p * AQUAEVO_ACC * 8, "acc"}, {fitness, p * 4, "fitness"}, {episodes, p * 8, "episodes"},
                            {log_ret, c * 4, "log_ret"}, {log_code, c, "log_code"}, {log_world, c * 8, "log_world"},
                            {counts, 8, "counts"}, {ret, n * 4, "ret"}, {finished, n, "finished"}};
    // (the inputs may share memory among themselves: only pairs with an output count)
    for (int out = 0; out < 3; ++out) {
        Range pair[2];
        pair[0] = ranges[out];
        for (int other = out + 1; other < 9; ++other) {
            pair[1] = ranges[other];
            if (int rc = overlap(pair, 2)) return rc;
        }
    }
    if (!aligned(log_ret, 4) || !aligned(ret, 4) || !aligned(fitness, 4)) return fail(AQUAEVO_E_ALIGN, "log_ret / ret / fitness must be 4-byte aligned");
    if (!aligned(log_world, 8) || !aligned(counts, 8) || !aligned(acc, 8) || !aligned(episodes, 8))
        return fail(AQUAEVO_E_ALIGN, "log_world / counts / acc / episodes must be 8-byte aligned");

    FitnessArgs k;
    k.log_ret = reinterpret_cast<const uint32_t*>(log_ret); k.log_code = log_code; k.log_world = log_world; k.counts = reinterpret_cast<const unsigned long long*>(counts);
    k.ret = reinterpret_cast<const uint32_t*>(ret); k.finished = finished; k.C = C; k.env_offset = env_offset;
    k.limit = N < P * seg ? N : P * seg;              // (P seg < 2^43)
    k.seg = static_cast<uint32_t>(seg); k.P = static_cast<uint32_t>(P); k.kind = kind;
    k.acc = reinterpret_cast<long long*>(acc); k.fitness = reinterpret_cast<uint32_t*>(fitness); k.episodes = reinterpret_cast<long long*>(episodes);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t words = k.P * AQUAEVO_ACC;
    hipLaunchKernelGGL(evo_zero_kernel, dim3((words + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, k.acc, words);
    if (int rc = launched("evo_zero_kernel launch")) return rc;
    int64_t blocks = (C + (finished != nullptr ? k.limit : 0) + BLOCK - 1) / BLOCK;
    blocks = blocks > MAX_BLOCKS ? MAX_BLOCKS : blocks;
    hipLaunchKernelGGL(evo_accumulate_kernel, dim3(static_cast<unsigned>(blocks)), dim3(BLOCK), 0, s, k);
    if (int rc = launched("evo_accumulate_kernel launch")) return rc;
    hipLaunchKernelGGL(evo_finish_kernel, dim3((k.P + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, k);
    return launched("evo_finish_kernel launch");
}

int aquaevo_tell(const float* fitness, int64_t P, uint64_t* header, float* theta, float* m, float* v, uint64_t* t,
                 double sigma, uint64_t seed, double lr, double beta1, double beta2, double eps, double weight_decay, int optimizer,
                 int32_t* rank2, int32_t* weights, double* grad_out, void* stream)
{
    if (fitness == nullptr || header == nullptr) return fail(AQUAEVO_E_INVALID, "fitness or header is NULL");
    if (theta == nullptr || m == nullptr || v == nullptr || t == nullptr) return fail(AQUAEVO_E_INVALID, "theta, m, v or t is NULL");
    if (int rc = check_networks(P)) return rc;
    const Optimiser o = {sigma, lr, beta1, beta2, eps, weight_decay, optimizer};
    if (int rc = check_optimiser(o, true)) return rc;
    const int64_t H = P / 2;
    if (H > 0 && (rank2 == nullptr || weights == nullptr)) return fail(AQUAEVO_E_INVALID, "rank2 or weights is NULL");
    const size_t h = static_cast<size_t>(H), row = PARAMS * sizeof(float);
    const Range ranges[] = {{fitness, static_cast<size_t>(P) * 4, "fitness"}, {header, AQUAEVO_HEADER * 8, "header"}, {theta, row, "theta"},
                            {m, row, "m"}, {v, row, "v"}, {t, 8, "t"}, {rank2, 2 * h * 4, "rank2"}, {weights, h * 4, "weights"},
                            {grad_out, PARAMS * sizeof(double), "grad_out"}};
    if (int rc = overlap(ranges, 9)) return rc;
    if (!aligned(fitness, 4) || !aligned(theta, 4) || !aligned(m, 4) || !aligned(v, 4) || !aligned(rank2, 4) || !aligned(weights, 4))
        return fail(AQUAEVO_E_ALIGN, "fitness / theta / m / v / rank2 / weights must be 4-byte aligned");
    if (!aligned(header, 8) || !aligned(t, 8) || !aligned(grad_out, 8)) return fail(AQUAEVO_E_ALIGN, "header / t / grad_out must be 8-byte aligned");

    const hipStream_t s = static_cast<hipStream_t>(stream);
    RankArgs r;
    r.fitness = reinterpret_cast<const uint32_t*>(fitness); r.header = reinterpret_cast<unsigned long long*>(header);
    r.t = reinterpret_cast<unsigned long long*>(t); r.rank2 = rank2; r.weights = weights; r.H = static_cast<uint32_t>(H);
    // a thread per ranked slot, whole wavefronts
    unsigned threads = WAVE;
    while (threads < RANK_BLOCK && threads < 2 * static_cast<unsigned>(H)) threads <<= 1;
    hipLaunchKernelGGL(evo_rank_kernel, dim3(1), dim3(threads), 0, s, r);
    if (int rc = launched("evo_rank_kernel launch")) return rc;
    if (H == 0) return 0;

    StepArgs k;
    k.weights = weights; k.header = r.header; k.t = r.t; k.theta = theta; k.m = m; k.v = v; k.grad_out = grad_out; k.seed = seed;
    k.H = static_cast<uint32_t>(H); k.o = o;
    constexpr int PER = BLOCK / WAVE;
    hipLaunchKernelGGL(evo_step_kernel, dim3((PARAMS + PER - 1) / PER), dim3(BLOCK), 0, s, k);
    return launched("evo_step_kernel launch");
}

}  // extern "C"
