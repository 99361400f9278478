// aqua_nstep.hip -- libaqua_nstep.so (csrc/aqua_nstep.h): the n-step fold of the experience ring.  For every sample of a
// minibatch draw, the window of up to n consecutive transitions of the sample's world becomes one staged transition
// (s_t, a_t, R, s_{t+L}, d_{t+L-1}, ok), and the bootstrap discount g^n is derived beside it, per network, from the learner
// bank's device table.  Its own translation unit and library: the other twelve libraries and their kernels are not touched.
//
// One kernel, nst_fold_kernel (an instance per action kind and source of gamma), one thread per sample, grid-stride above MAX_BLOCKS blocks.  With capacity % N == 0 the next
// step of the world in slot c is slot c + N (mod capacity): every address of a window is known once idx is, so the d, ok
// and r loads of CHUNK steps are issued together and the walk then decides in registers -- ceil(n / CHUNK) dependent round
// trips per window, not n.  That is a property of the compiled code, to be read in its listing (tools/isa_listing.py): the
// 3 x STEPS loads of a batch stand in one block ahead of the first wait on any of them.  Three things keep it so: a batch
// of fewer than CHUNK steps is straight-line code of its own (fold_batch<STEPS>), r is converted in the walk, and the
// scheduler may not move across the end of the loads.  No LDS, no cross-lane traffic, no atomics; no thread reads what another thread of the launch
// writes (the header is only read; hyper_out may not overlap hyper_dev).
// Floating point: the return and the discount are sums and products in double, each rounded, nothing contracted: the
// functions that compute carry `#pragma clang fp contract(off)`.
#include <hip/hip_runtime.h>

#include "aqua_nstep.h"
#include "aqua_host.hpp"

namespace {

constexpr int BLOCK = AQUANST_BLOCK;
constexpr int MAX_BLOCKS = AQUANST_MAX_BLOCKS;
constexpr int CHUNK = AQUANST_CHUNK;
constexpr int HYPER = AQUANST_HYPER_WORDS;
constexpr int ROWS = 5;                               // the observation (main/impl/utils.py:15-33)

static_assert(AQUANST_MAX_STEPS <= 255, "the window length is stored in a byte");
static_assert(AQUANST_MAX_STEPS % AQUANST_CHUNK == 0, "whole batches of loads");

struct FoldArgs {
    const int64_t* header;
    const float* s;
    const void* a;
    const float* r;
    const float* s2;
    const uint8_t* d;
    const uint8_t* ok;
    int64_t ring_ld;
    int32_t capacity, N;                              // (validated sizes that fit 32 bits travel as such: fewer scalar registers)
    const int32_t* idx;
    int32_t P, B;
    int32_t n;
    double g;                                         // (double)(float)gamma of the scalar form
    const double* hyper;
    float* out_s;
    void* out_a;
    float* out_r;
    float* out_s2;
    uint8_t* out_d;
    uint8_t* out_ok;
    int64_t out_ld;
    uint8_t* out_len;
    double* hyper_out;
};

// the float32 the learners round gamma to, as a double
__host__ __device__ inline double rounded_gamma(double gamma) { return static_cast<double>(static_cast<float>(gamma)); }

// THE statement of the bootstrap discount: g times itself n - 1 times, every product rounded in double
__host__ __device__ inline double discount_of(double g, int n)
{
#pragma clang fp contract(off)
    double out = g;
    for (int i = 1; i < n; ++i) out = out * g;
    return out;
}

// what the walk of one window carries from batch to batch
struct Walk {
    bool walking = false, valid = false;
    int L = 0;
    uint8_t code = 0;
    int64_t last = 0;                                 // slot_{L-1}
    int64_t slot = 0;                                 // the slot of the next batch's first step
    double pw = 1.0, acc = 0.0;
};

// STEPS steps of a window, kb .. kb + STEPS - 1 (the last batch of a window, or CHUNK of them): first the d, ok and r loads
// of every step, 3 x STEPS loads in one block with no branch and no wait among them, then the walk over what they brought.
// An instance per count instead of a load predicated on k < n: that compiles to a branch per step with a wait in each.  r
// stays raw bits until the walk converts it (a conversion at the load is a wait at the load)
template <int STEPS>
__device__ __forceinline__ void fold_batch(const FoldArgs& a, int kb, int32_t lim, double g, Walk& w)
{
#pragma clang fp contract(off)
    static_assert(STEPS >= 1 && STEPS <= CHUNK, "a batch is at most CHUNK steps");
    uint8_t dd[STEPS], oo[STEPS];
    uint32_t rr[STEPS];
    const uint32_t* r_bits = reinterpret_cast<const uint32_t*>(a.r);
    const bool closes = STEPS < CHUNK || a.n - kb == CHUNK;            // this batch holds step n - 1
    int64_t sl = w.slot;
#pragma unroll
    for (int u = 0; u < STEPS; ++u) {
        dd[u] = a.d[sl];
        oo[u] = a.ok[sl];
        rr[u] = r_bits[sl];
        sl += a.N;
        if (sl >= a.capacity) sl -= a.capacity;
    }
    // (the scheduler otherwise starts the walk, and its waits, among the last loads)
    __builtin_amdgcn_sched_barrier(0);
    sl = w.slot;
#pragma unroll
    for (int u = 0; u < STEPS; ++u) {
        // (selects, not branches: the lanes of a wavefront leave the walk at different steps)
        const int k = kb + u;
        const bool first = u == 0 && kb == 0;
        const bool go = w.walking && k <= lim && oo[u] != 0;           // else: past the newest round, or not an experience
        const double r_k = static_cast<double>(__uint_as_float(rr[u]));
        const double pw_k = first ? 1.0 : w.pw * g;
        const double acc_k = first ? r_k : w.acc + pw_k * r_k;
        w.pw = go ? pw_k : w.pw;
        w.acc = go ? acc_k : w.acc;
        const bool end = go && (dd[u] != 0 || (closes && u == STEPS - 1));
        w.valid = w.valid || end;
        w.L = end ? k + 1 : w.L;
        w.code = end ? dd[u] : w.code;
        w.last = end ? sl : w.last;
        w.walking = go && !end;
        sl += a.N;
        if (sl >= a.capacity) sl -= a.capacity;
        // (step by step: the steps' lane masks would otherwise all be formed first and held in scalar registers)
        __builtin_amdgcn_sched_barrier(0);
    }
    w.slot = sl;
}

// F32X2: the action rows are float32 [2][ld] (else uint8 [ld]); TABLE: gamma comes from the learner bank's table.  Four
// instances: what is known at compile time needs no scalar register, and the kernel has none to spare
template <bool F32X2, bool TABLE>
__global__ __launch_bounds__(BLOCK) void nst_fold_kernel(const FoldArgs a)
{
#pragma clang fp contract(off)
    const int64_t cursor = a.header[0];
    // capacity < 2^31, so everything below a valid cursor or slot divides in 32 bits
    const uint32_t N32 = static_cast<uint32_t>(a.N);
    const bool ring_ok = cursor >= 0 && cursor < a.capacity && static_cast<uint32_t>(cursor) % N32 == 0;
    const uint32_t B32 = static_cast<uint32_t>(a.B);
    const int64_t total = static_cast<int64_t>(a.P) * a.B;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * BLOCK;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x; i < total; i += stride) {
        const uint32_t p = static_cast<uint32_t>(i) / B32;              // i < P * B <= 2^32
        double g = a.g;
        if (TABLE) {
            const double* row = a.hyper + static_cast<size_t>(p) * HYPER;
            g = rounded_gamma(row[0]);
            if (a.hyper_out != nullptr && static_cast<uint32_t>(i) == p * B32) {   // sample j == 0 of network p
                double* out = a.hyper_out + static_cast<size_t>(p) * HYPER;
                double word[HYPER];                                    // (read whole, then written: the tables do not overlap)
#pragma unroll
                for (int w = 1; w < HYPER; ++w) word[w] = row[w];
                out[0] = discount_of(g, a.n);
#pragma unroll
                for (int w = 1; w < HYPER; ++w) out[w] = word[w];
            }
        }
        const int64_t c = a.idx[i];
        bool walking = ring_ok && c >= 0 && c < a.capacity;         // otherwise c is never an address
        int32_t age = 0;
        if (walking) {
            const int64_t round = c - static_cast<int64_t>(static_cast<uint32_t>(c) % N32);
            int64_t x = cursor - a.N - round;                          // in [-capacity, capacity)
            if (x < 0) x += a.capacity;
            age = static_cast<int32_t>(static_cast<uint32_t>(x) / N32);   // rounds written after c's
        }
        const int32_t lim = age < a.n - 1 ? age : a.n - 1;             // the last step this window may take
        Walk w;
        w.walking = walking;
        w.slot = walking ? c : 0;                                      // in [0, capacity) throughout, N <= capacity
#pragma unroll 1
        for (int kb = 0; kb < a.n && w.walking; kb += CHUNK) {
            // a batch of exactly min(n - kb, CHUNK) steps: the count is uniform, so this is a scalar branch to straight-line code
            const int rem = a.n - kb;
            switch (rem < CHUNK ? rem : CHUNK) {
            case 1: fold_batch<1>(a, kb, lim, g, w); break;
            case 2: fold_batch<2>(a, kb, lim, g, w); break;
            case 3: fold_batch<3>(a, kb, lim, g, w); break;
            case 4: fold_batch<4>(a, kb, lim, g, w); break;
            case 5: fold_batch<5>(a, kb, lim, g, w); break;
            case 6: fold_batch<6>(a, kb, lim, g, w); break;
            case 7: fold_batch<7>(a, kb, lim, g, w); break;
            default: fold_batch<CHUNK>(a, kb, lim, g, w); break;
            }
        }
        const bool valid = w.valid;
        const int L = w.L;
        const uint8_t code = w.code;
        const int64_t last = w.last;
        const double acc = w.acc;
        // zeros as bit patterns: the rows are copied, never computed with
        // (what is no sample reads slot 0, a valid address, and keeps nothing of it: loads without a branch each)
        uint32_t x[ROWS], x2[ROWS], act0, act1 = 0;
        const int64_t src = valid ? c : 0;
        // (row by row with a moving pointer: five row bases per array would be five loop invariants each)
        const uint32_t* ps = reinterpret_cast<const uint32_t*>(a.s) + src;
        const uint32_t* ps2 = reinterpret_cast<const uint32_t*>(a.s2) + last;
#pragma unroll
        for (int row = 0; row < ROWS; ++row) {
            x[row] = *ps;
            x2[row] = *ps2;
            ps += a.ring_ld;
            ps2 += a.ring_ld;
        }
        if (!F32X2) {
            act0 = static_cast<const uint8_t*>(a.a)[src];
        } else {
            act0 = static_cast<const uint32_t*>(a.a)[src];
            act1 = static_cast<const uint32_t*>(a.a)[a.ring_ld + src];
        }
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
        a.out_r[i] = valid ? static_cast<float>(acc) : 0.0f;
        if (!F32X2) {
            static_cast<uint8_t*>(a.out_a)[i] = static_cast<uint8_t>(act0);
        } else {
            static_cast<uint32_t*>(a.out_a)[i] = act0;
            static_cast<uint32_t*>(a.out_a)[a.out_ld + i] = act1;
        }
        a.out_d[i] = valid ? code : static_cast<uint8_t>(0);
        a.out_ok[i] = valid ? 1 : 0;
        if (a.out_len != nullptr) a.out_len[i] = static_cast<uint8_t>(valid ? L : 0);
    }
}

// ------------------------------------------------------------------ host side
unsigned grid_of(int64_t n)
{
    int64_t blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
    return static_cast<unsigned>(blocks < 1 ? 1 : blocks);
}

int check_steps(int n)
{
    if (n < 1 || n > AQUANST_MAX_STEPS) return fail(AQUANST_E_INVALID, "n=%d: must be in [1, %d]", n, AQUANST_MAX_STEPS);
    return 0;
}

int check_gamma(double gamma)
{
    if (!is_number(gamma) || !(gamma >= 0.0 && gamma <= 1.0)) return fail(AQUANST_E_INVALID, "gamma=%g: must be in [0, 1]", gamma);
    return 0;
}

bool overlap(const void* p, size_t pn, const void* q, size_t qn)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + qn && b < a + pn;
}

}  // namespace

extern "C" {

int aquanst_version(void) { return AQUANST_ABI_VERSION; }
const char* aquanst_last_error(void) { return g_err; }

double aquanst_discount(double gamma, int n)
{
    if (check_gamma(gamma) || check_steps(n)) return -1.0;
    return discount_of(rounded_gamma(gamma), n);
}

int aquanst_fold(const int64_t* header, const float* s, const void* a, const float* r, const float* s2, const uint8_t* d,
                 const uint8_t* ok, int64_t ring_ld, int64_t capacity, int action_kind, int64_t N,
                 const int32_t* idx, int64_t P, int64_t B, int n, double gamma, const double* hyper_dev,
                 float* out_s, void* out_a, float* out_r, float* out_s2, uint8_t* out_d, uint8_t* out_ok, int64_t out_ld,
                 uint8_t* out_len, double* hyper_out, void* stream)
{
    if (header == nullptr) return fail(AQUANST_E_INVALID, "header is NULL");
    if (s == nullptr || a == nullptr || r == nullptr || s2 == nullptr || d == nullptr || ok == nullptr)
        return fail(AQUANST_E_INVALID, "s, a, r, s2, d or ok is NULL");
    if (capacity <= 0 || capacity > AQUANST_MAX_CAPACITY)
        return fail(AQUANST_E_INVALID, "capacity=%lld: must be in [1, %d]", (long long)capacity, AQUANST_MAX_CAPACITY);
    if (ring_ld < capacity) return fail(AQUANST_E_INVALID, "ring_ld=%lld: below the capacity %lld", (long long)ring_ld, (long long)capacity);
    if (action_kind != AQUANST_ACT_U8 && action_kind != AQUANST_ACT_F32X2)
        return fail(AQUANST_E_INVALID, "action_kind=%d: AQUANST_ACT_U8 or AQUANST_ACT_F32X2", action_kind);
    if (N < 1 || N > capacity) return fail(AQUANST_E_INVALID, "N=%lld: must be in [1, capacity=%lld]", (long long)N, (long long)capacity);
    if (capacity % N != 0)
        return fail(AQUANST_E_INVALID, "capacity=%lld is no multiple of N=%lld: a slot must belong to one world", (long long)capacity, (long long)N);
    if (P < 1 || P > AQUANST_MAX_NETWORKS) return fail(AQUANST_E_INVALID, "P=%lld: must be in [1, %d]", (long long)P, AQUANST_MAX_NETWORKS);
    if (B < 0 || B > AQUANST_MAX_BATCH) return fail(AQUANST_E_INVALID, "B=%lld: must be in [0, %d]", (long long)B, AQUANST_MAX_BATCH);
    if (int rc = check_steps(n)) return rc;
    if (hyper_dev == nullptr) {
        if (int rc = check_gamma(gamma)) return rc;                   // (neither: AQUANST_NO_GAMMA is outside [0, 1])
        if (hyper_out != nullptr) return fail(AQUANST_E_INVALID, "hyper_out without hyper_dev: there is no table to derive it from");
    } else {
        if (gamma != AQUANST_NO_GAMMA) return fail(AQUANST_E_INVALID, "gamma=%g and hyper_dev: pass one of them (gamma = AQUANST_NO_GAMMA with a table)", gamma);
        if (hyper_out != nullptr && overlap(hyper_dev, sizeof(double) * HYPER * P, hyper_out, sizeof(double) * HYPER * P))
            return fail(AQUANST_E_INVALID, "hyper_out overlaps hyper_dev: a thread would read what another writes");
    }
    if (out_ld < P * B) return fail(AQUANST_E_INVALID, "out_ld=%lld: below P * B = %lld", (long long)out_ld, (long long)(P * B));
    if (!aligned(header, 8) || !aligned(hyper_dev, 8) || !aligned(hyper_out, 8))
        return fail(AQUANST_E_ALIGN, "header / hyper_dev / hyper_out must be 8-byte aligned");
    if (!aligned(idx, 4) || !aligned(s, 4) || !aligned(r, 4) || !aligned(s2, 4) || !aligned(out_s, 4) || !aligned(out_r, 4) || !aligned(out_s2, 4))
        return fail(AQUANST_E_ALIGN, "idx and the float32 rows must be 4-byte aligned");
    if (action_kind == AQUANST_ACT_F32X2 && (!aligned(a, 4) || !aligned(out_a, 4)))
        return fail(AQUANST_E_ALIGN, "float32 action rows must be 4-byte aligned");
    if (B == 0) return 0;
    if (idx == nullptr) return fail(AQUANST_E_INVALID, "idx is NULL");
    if (out_s == nullptr || out_a == nullptr || out_r == nullptr || out_s2 == nullptr || out_d == nullptr || out_ok == nullptr)
        return fail(AQUANST_E_INVALID, "out_s, out_a, out_r, out_s2, out_d or out_ok is NULL");

    FoldArgs k;
    k.header = header; k.s = s; k.a = a; k.r = r; k.s2 = s2; k.d = d; k.ok = ok; k.ring_ld = ring_ld; k.capacity = static_cast<int32_t>(capacity);
    k.N = static_cast<int32_t>(N); k.idx = idx; k.P = static_cast<int32_t>(P); k.B = static_cast<int32_t>(B); k.n = n;
    k.g = hyper_dev == nullptr ? rounded_gamma(gamma) : 0.0; k.hyper = hyper_dev;
    k.out_s = out_s; k.out_a = out_a; k.out_r = out_r; k.out_s2 = out_s2; k.out_d = out_d; k.out_ok = out_ok; k.out_ld = out_ld;
    k.out_len = out_len; k.hyper_out = hyper_out;
    const bool f32x2 = action_kind == AQUANST_ACT_F32X2, table = hyper_dev != nullptr;
    auto kernel = f32x2 ? (table ? nst_fold_kernel<true, true> : nst_fold_kernel<true, false>)
                        : (table ? nst_fold_kernel<false, true> : nst_fold_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(grid_of(P * B)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), k);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "nst_fold_kernel launch");
    return 0;
}

}  // extern "C"
