// aqua_pbt.hip -- libaqua_pbt.so (aquaticgymenv_amd/include/aqua_pbt.h): selection among the networks of a learner bank on
// gfx950, asynchronous population-based training with truncation selection.  Its own translation unit and library.
//
// Two launches.  pbt_plan_kernel is ONE workgroup: the <= 4096 networks are ranked by a bitonic sort of
// 64-bit words in LDS, the bottom quantile's ready networks each draw a parent from the top quantile, and everything
// small is written there.  pbt_copy_kernel has a grid over (chunk, four networks): a block whose networks keep their rows
// leaves after four loads.  No atomics on memory, no floating-point atomics, no block waits on another block.
#include <hip/hip_runtime.h>

#include "../include/aqua_pbt.h"
#include "aqua_device.hpp"
#include "aqua_host.hpp"

namespace {

constexpr int PLAN_BLOCK = 1024;
constexpr int COPY_BLOCK = 256;
constexpr int PARTS = 2;                             // blocks a row of one array is cut into
constexpr uint32_t GROUP = 4;                        // networks a block of the copy looks at
constexpr int ARRAYS = 6;                            // theta, theta_target, m, v, blob_online, blob_target
constexpr uint64_t PAD = ~0ull;                      // sorts behind every scored network

struct PlanArgs {
    const uint32_t* score;
    const unsigned long long* seg_counts;
    int P;
    unsigned long long* header;
    unsigned long long* mark;
    int32_t* origin;
    int32_t* parent;
    double* hyper;
    double* eps_state;
    float* eps_out;
    double fraction;
    unsigned long long ready, every, seed;
    double lr_factor[2], lr_lo, lr_hi, gamma_factor[2], gamma_lo, gamma_hi;
};

struct CopyArgs {
    const int32_t* parent;
    int P;
    float* stacked[4];
    float* blob[2];
    unsigned long long* t;
    uint32_t blob_vecs;                              // float4 of a blob row
};

__global__ __launch_bounds__(PLAN_BLOCK) void pbt_plan_kernel(const PlanArgs a)
{
#pragma clang fp contract(off)
    __shared__ uint64_t s_key[AQUAPBT_MAX_NETWORKS];  // (~key << 32) | network: ascending = best first
    __shared__ int32_t s_parent[AQUAPBT_MAX_NETWORKS];
    __shared__ unsigned long long s_calls;
    __shared__ uint32_t s_scored, s_losers;
    const uint32_t tid = threadIdx.x, threads = blockDim.x, P = static_cast<uint32_t>(a.P);

    if (tid == 0) {
        s_calls = a.header[0];
        s_scored = 0;
        s_losers = 0;
    }
    __syncthreads();
    const unsigned long long c = s_calls;
    if (c % a.every != 0) {                           // (uniform)
        for (uint32_t p = tid; p < P; p += threads) a.parent[p] = static_cast<int32_t>(p);
        if (tid == 0) {
            a.header[0] = c + 1;
            a.header[2] = 0;
        }
        return;
    }

    // the words to sort, padded to a power of two
    uint32_t n2 = 2;
    while (n2 < P) n2 <<= 1;
    for (uint32_t p = tid; p < n2; p += threads) {
        uint64_t word = PAD;
        if (p < P) {
            s_parent[p] = static_cast<int32_t>(p);
            if (a.seg_counts[static_cast<size_t>(p) * AQUAPBT_COUNTS] >= 1) {
                const uint32_t u = a.score[p];
                const uint32_t key = (u >> 31) ? ~u : (u | 0x80000000u);
                word = (static_cast<uint64_t>(~key) << 32) | p;
            }
        }
        s_key[p] = word;
    }
    __syncthreads();
    for (uint32_t size = 2; size <= n2; size <<= 1) {
        for (uint32_t j = size >> 1; j > 0; j >>= 1) {
            for (uint32_t w = tid; w < (n2 >> 1); w += threads) {
                const uint32_t i = ((w & ~(j - 1)) << 1) | (w & (j - 1)), l = i | j;
                const uint64_t x = s_key[i], y = s_key[l];
                const bool up = (i & size) == 0;
                if ((x > y) == up) {
                    s_key[i] = y;
                    s_key[l] = x;
                }
            }
            __syncthreads();
        }
    }
    // S: the scored networks are the words in front of the padding
    for (uint32_t i = tid; i < n2; i += threads)
        if (s_key[i] != PAD && (i + 1 == n2 || s_key[i + 1] == PAD)) s_scored = i + 1;
    __syncthreads();
    const uint32_t S = s_scored;
    const uint32_t k = static_cast<uint32_t>(a.fraction * static_cast<double>(S));

    uint32_t mine = 0;
    for (uint32_t i = S - k + tid; i < S; i += threads) {
        const uint32_t p = static_cast<uint32_t>(s_key[i]);
        const unsigned long long episodes = a.seg_counts[static_cast<size_t>(p) * AQUAPBT_COUNTS];
        if (episodes - a.mark[p] < a.ready) continue;
        uint32_t r[4];
        aqua::draw(a.seed, p, c, AQUAPBT_STREAM, 0, r);
        const uint32_t j = static_cast<uint32_t>((static_cast<uint64_t>(r[0]) * k) >> 32);
        const uint32_t q = static_cast<uint32_t>(s_key[j]);           // j < k <= S - k: a rank no loser holds
        s_parent[p] = static_cast<int32_t>(q);
        a.origin[p] = a.origin[q];
        a.mark[p] = episodes;
        const double* from = a.hyper + static_cast<size_t>(q) * AQUAPBT_HYPER_WORDS;
        double* to = a.hyper + static_cast<size_t>(p) * AQUAPBT_HYPER_WORDS;
        double row[AQUAPBT_HYPER_WORDS];
#pragma unroll
        for (int w = 0; w < AQUAPBT_HYPER_WORDS; ++w) row[w] = from[w];
        double lr = row[AQUAPBT_HYPER_LR] * ((r[1] & 1u) ? a.lr_factor[1] : a.lr_factor[0]);
        lr = lr > a.lr_lo ? lr : a.lr_lo;
        lr = lr < a.lr_hi ? lr : a.lr_hi;
        const double rest = (1.0 - row[AQUAPBT_HYPER_GAMMA]) * ((r[2] & 1u) ? a.gamma_factor[1] : a.gamma_factor[0]);
        double gamma = 1.0 - rest;
        gamma = gamma > a.gamma_lo ? gamma : a.gamma_lo;
        gamma = gamma < a.gamma_hi ? gamma : a.gamma_hi;
        row[AQUAPBT_HYPER_LR] = lr;
        row[AQUAPBT_HYPER_GAMMA] = gamma;
#pragma unroll
        for (int w = 0; w < AQUAPBT_HYPER_WORDS; ++w) to[w] = row[w];
        if (a.eps_state != nullptr) {
            a.eps_state[p] = a.eps_state[q];
            a.eps_out[p] = a.eps_out[q];
        }
        mine += 1;
    }
    if (mine != 0) atomicAdd(&s_losers, mine);        // (an integer add in LDS)
    __syncthreads();
    for (uint32_t p = tid; p < P; p += threads) a.parent[p] = s_parent[p];
    if (tid == 0) {
        const uint32_t n = s_losers;
        a.header[0] = c + 1;
        if (n != 0) a.header[1] = a.header[1] + n;
        a.header[2] = n;
        a.header[3] = S;
    }
}

// block (x, y): array x / PARTS, part x % PARTS of the rows of the networks y * GROUP .. y * GROUP + GROUP - 1.  Most
// networks keep their rows: a block per network would be a grid of mostly idle blocks (16 us of dispatch at P = 4096).
__global__ __launch_bounds__(COPY_BLOCK) void pbt_copy_kernel(const CopyArgs a)
{
    const uint32_t array = blockIdx.x / PARTS, part = blockIdx.x % PARTS;
    const uint32_t P = static_cast<uint32_t>(a.P);
    for (uint32_t p = blockIdx.y * GROUP; p < blockIdx.y * GROUP + GROUP && p < P; ++p) {
        const uint32_t q = static_cast<uint32_t>(a.parent[p]);
        if (q == p || q >= P) continue;
        if (array < 4) {
            // rows of 4739 floats are 4-byte aligned from row to row: coalesced dwords
            constexpr uint32_t PER = (AQUAPBT_PARAMS + PARTS - 1) / PARTS;
            const uint32_t end = (part + 1) * PER < AQUAPBT_PARAMS ? (part + 1) * PER : AQUAPBT_PARAMS;
            float* base = array == 0 ? a.stacked[0] : array == 1 ? a.stacked[1] : array == 2 ? a.stacked[2] : a.stacked[3];
            const float* src = base + static_cast<size_t>(q) * AQUAPBT_PARAMS;
            float* dst = base + static_cast<size_t>(p) * AQUAPBT_PARAMS;
#pragma unroll 4
            for (uint32_t i = part * PER + threadIdx.x; i < end; i += COPY_BLOCK) dst[i] = src[i];
            if (blockIdx.x == 0 && threadIdx.x == 0) a.t[p] = a.t[q];
        } else {
            const uint32_t per = (a.blob_vecs + PARTS - 1) / PARTS;
            const uint32_t end = (part + 1) * per < a.blob_vecs ? (part + 1) * per : a.blob_vecs;
            float4* base = reinterpret_cast<float4*>(array == 4 ? a.blob[0] : a.blob[1]);
            const float4* src = base + static_cast<size_t>(q) * a.blob_vecs;
            float4* dst = base + static_cast<size_t>(p) * a.blob_vecs;
#pragma unroll 4
            for (uint32_t i = part * per + threadIdx.x; i < end; i += COPY_BLOCK) dst[i] = src[i];
        }
    }
}

struct Range {
    const void* at;
    size_t bytes;
    const char* name;
};

}  // namespace

extern "C" {

int aquapbt_version(void) { return AQUAPBT_ABI_VERSION; }
const char* aquapbt_last_error(void) { return g_err; }

int aquapbt_select(const float* score, const uint64_t* seg_counts, int64_t P,
                   uint64_t* header, uint64_t* mark, int32_t* origin, int32_t* parent,
                   float* theta, float* theta_target, float* m, float* v, uint64_t* t,
                   float* blob_online, float* blob_target, int64_t blob_floats,
                   double* hyper, double* eps_state, float* eps_out,
                   double fraction, int64_t ready, int64_t every, uint64_t seed,
                   double lr_factor0, double lr_factor1, double lr_lo, double lr_hi,
                   double gamma_factor0, double gamma_factor1, double gamma_lo, double gamma_hi,
                   void* stream)
{
    if (P < 1 || P > AQUAPBT_MAX_NETWORKS) return fail(AQUAPBT_E_INVALID, "P=%lld: must be in [1, %d]", (long long)P, AQUAPBT_MAX_NETWORKS);
    if (score == nullptr || seg_counts == nullptr) return fail(AQUAPBT_E_INVALID, "score or seg_counts is NULL");
    if (header == nullptr || mark == nullptr || origin == nullptr || parent == nullptr)
        return fail(AQUAPBT_E_INVALID, "header, mark, origin or parent is NULL");
    if (theta == nullptr || theta_target == nullptr || m == nullptr || v == nullptr || t == nullptr)
        return fail(AQUAPBT_E_INVALID, "theta, theta_target, m, v or t is NULL");
    if (blob_online == nullptr || blob_target == nullptr || hyper == nullptr) return fail(AQUAPBT_E_INVALID, "blob_online, blob_target or hyper is NULL");
    if ((eps_state == nullptr) != (eps_out == nullptr))
        return fail(AQUAPBT_E_INVALID, "eps_state and eps_out: give both, or neither if the schedules are not inherited");
    if (blob_floats < 4 || blob_floats > AQUAPBT_MAX_BLOB || blob_floats % 4 != 0)
        return fail(AQUAPBT_E_INVALID, "blob_floats=%lld: a multiple of 4 in [4, %d]", (long long)blob_floats, AQUAPBT_MAX_BLOB);
    if (!is_number(fraction) || !(fraction > 0.0 && fraction <= 0.5)) return fail(AQUAPBT_E_INVALID, "fraction=%g: must be in (0, 0.5]", fraction);
    if (ready < 1) return fail(AQUAPBT_E_INVALID, "ready=%lld: must be >= 1", (long long)ready);
    if (every < 1) return fail(AQUAPBT_E_INVALID, "every=%lld: must be >= 1", (long long)every);
    if (!is_number(lr_factor0) || !is_number(lr_factor1) || !(lr_factor0 > 0.0 && lr_factor1 > 0.0))
        return fail(AQUAPBT_E_INVALID, "lr_factors=(%g, %g): must be finite and > 0", lr_factor0, lr_factor1);
    if (!is_number(lr_lo) || !is_number(lr_hi) || !(lr_lo > 0.0 && lr_lo <= lr_hi))
        return fail(AQUAPBT_E_INVALID, "lr_bounds=(%g, %g): 0 < lo <= hi, finite", lr_lo, lr_hi);
    if (!is_number(gamma_factor0) || !is_number(gamma_factor1) || !(gamma_factor0 > 0.0 && gamma_factor1 > 0.0))
        return fail(AQUAPBT_E_INVALID, "gamma_factors=(%g, %g): must be finite and > 0", gamma_factor0, gamma_factor1);
    if (!is_number(gamma_lo) || !is_number(gamma_hi) || !(gamma_lo >= 0.0 && gamma_lo <= gamma_hi && gamma_hi <= 1.0))
        return fail(AQUAPBT_E_INVALID, "gamma_bounds=(%g, %g): 0 <= lo <= hi <= 1", gamma_lo, gamma_hi);
    const size_t n = static_cast<size_t>(P), stack = n * AQUAPBT_PARAMS * sizeof(float), blob = n * static_cast<size_t>(blob_floats) * sizeof(float);
    const Range ranges[] = {
        {score, n * 4, "score"}, {seg_counts, n * AQUAPBT_COUNTS * 8, "seg_counts"}, {header, AQUAPBT_HEADER * 8, "header"},
        {mark, n * 8, "mark"}, {origin, n * 4, "origin"}, {parent, n * 4, "parent"}, {theta, stack, "theta"},
        {theta_target, stack, "theta_target"}, {m, stack, "m"}, {v, stack, "v"}, {t, n * 8, "t"}, {blob_online, blob, "blob_online"},
        {blob_target, blob, "blob_target"}, {hyper, n * AQUAPBT_HYPER_WORDS * 8, "hyper"}, {eps_state, n * 8, "eps_state"},
        {eps_out, n * 4, "eps_out"}};
    constexpr int R = sizeof(ranges) / sizeof(ranges[0]);
    for (int i = 0; i < R; ++i)
        for (int j = i + 1; j < R; ++j) {
            if (ranges[i].at == nullptr || ranges[j].at == nullptr) continue;
            const uintptr_t x = reinterpret_cast<uintptr_t>(ranges[i].at), y = reinterpret_cast<uintptr_t>(ranges[j].at);
            if (x < y ? y - x < ranges[i].bytes : x - y < ranges[j].bytes)
                return fail(AQUAPBT_E_INVALID, "%s and %s overlap", ranges[i].name, ranges[j].name);
        }
    if (!aligned(score, 4) || !aligned(origin, 4) || !aligned(parent, 4) || !aligned(eps_out, 4))
        return fail(AQUAPBT_E_ALIGN, "score / origin / parent / eps_out must be 4-byte aligned");
    if (!aligned(seg_counts, 8) || !aligned(header, 8) || !aligned(mark, 8) || !aligned(t, 8) || !aligned(hyper, 8) || !aligned(eps_state, 8))
        return fail(AQUAPBT_E_ALIGN, "seg_counts / header / mark / t / hyper / eps_state must be 8-byte aligned");
    if (!aligned(theta, 4) || !aligned(theta_target, 4) || !aligned(m, 4) || !aligned(v, 4))
        return fail(AQUAPBT_E_ALIGN, "theta / theta_target / m / v must be 4-byte aligned");
    if (!aligned(blob_online, 16) || !aligned(blob_target, 16)) return fail(AQUAPBT_E_ALIGN, "blob_online / blob_target must be 16-byte aligned");

    PlanArgs k;
    k.score = reinterpret_cast<const uint32_t*>(score);
    k.seg_counts = reinterpret_cast<const unsigned long long*>(seg_counts);
    k.P = static_cast<int>(P);
    k.header = reinterpret_cast<unsigned long long*>(header);
    k.mark = reinterpret_cast<unsigned long long*>(mark);
    k.origin = origin; k.parent = parent; k.hyper = hyper; k.eps_state = eps_state; k.eps_out = eps_out;
    k.fraction = fraction;
    k.ready = static_cast<unsigned long long>(ready); k.every = static_cast<unsigned long long>(every); k.seed = seed;
    k.lr_factor[0] = lr_factor0; k.lr_factor[1] = lr_factor1; k.lr_lo = lr_lo; k.lr_hi = lr_hi;
    k.gamma_factor[0] = gamma_factor0; k.gamma_factor[1] = gamma_factor1; k.gamma_lo = gamma_lo; k.gamma_hi = gamma_hi;
    // one thread per pair of the sort, whole wavefronts
    unsigned threads = 64;
    while (threads < PLAN_BLOCK && 2 * threads < static_cast<unsigned>(P)) threads <<= 1;
    hipLaunchKernelGGL(pbt_plan_kernel, dim3(1), dim3(threads), 0, static_cast<hipStream_t>(stream), k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "pbt_plan_kernel launch");

    CopyArgs c;
    c.parent = parent; c.P = static_cast<int>(P);
    c.stacked[0] = theta; c.stacked[1] = theta_target; c.stacked[2] = m; c.stacked[3] = v;
    c.blob[0] = blob_online; c.blob[1] = blob_target;
    c.t = reinterpret_cast<unsigned long long*>(t);
    c.blob_vecs = static_cast<uint32_t>(blob_floats / 4);
    hipLaunchKernelGGL(pbt_copy_kernel, dim3(ARRAYS * PARTS, static_cast<unsigned>((P + GROUP - 1) / GROUP)), dim3(COPY_BLOCK), 0, static_cast<hipStream_t>(stream), c);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "pbt_copy_kernel launch");
    return 0;
}

}  // extern "C"
