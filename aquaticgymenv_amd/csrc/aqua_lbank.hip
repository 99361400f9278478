// aqua_lbank.hip -- libaqua_lbank.so (include/aqua_lbank.h): one DQN update of EVERY network of a Q-network bank in two
// launches, and the minibatch draw of every network from its own slots of the one experience ring in one launch, on
// gfx950.  Its own translation unit and library: the other seven libraries and their kernels are not touched by it.
//
// The update is libaqua_learner.so's, to the bit: both kernel bodies are the forced-inline device functions of
// aqua_lrn.hpp.  A launch has a second grid dimension, the network: block (g, p) builds the GradArgs / ApplyArgs of network
// p -- the stacked base pointers plus p * stride, p's workspace region, p's row of idx, p's row of the hyper-parameter
// table -- and calls the shared body with block index g.  Everything it builds is a function of blockIdx.y and the kernel
// arguments alone, so it is wavefront-uniform and stays in scalar registers.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/aqua_lbank.h"
#include "aqua_device.hpp"
#include "aqua_host.hpp"
#include "aqua_qnet.hpp"
#include "aqua_lrn.hpp"

namespace {

using namespace aqua::lrn;

static_assert(PARAMS == AQUALBANK_PARAMS && AQUALRN_MAX_BATCH == AQUALBANK_MAX_BATCH, "aqua_lbank.h restates the learner's sizes");
static_assert(STREAM_LEARNER == AQUALBANK_STREAM && ATTEMPTS == AQUALBANK_ATTEMPTS, "the draw reproduces the learner's own");
static_assert(AQUALBANK_MAX_NETWORKS <= 65535, "the network is the grid's y index");

constexpr int HYPER = AQUALBANK_HYPER_WORDS;
enum { H_GAMMA = 0, H_TAU, H_LR, H_BETA1, H_BETA2, H_EPS };
constexpr int DRAW_BLOCK = 256, DRAW_MAX_BLOCKS = 2048;

struct BankGradArgs {
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
};

struct BankApplyArgs {
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

struct BankDrawArgs {
    const int64_t* header;
    const uint8_t* ok;
    int64_t capacity, N, seg, used;          // used: the networks that own a world, ceil(N / seg)
    const uint64_t* t_dev;
    const uint64_t* seed;
    int32_t* idx;
    int64_t B;
};

template <int STRAT>
__global__ __launch_bounds__(BLOCK) void lbank_grad_kernel(const BankGradArgs b)
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
    grad_body<STRAT>(a, blockIdx.x);
}

__global__ __launch_bounds__(APPLY_BLOCK) void lbank_apply_kernel(const BankApplyArgs b)
{
    const int64_t p = blockIdx.y;
    // p's row of the table, read through a vector register: the five doubles then live in VGPRs (37 of 512 are in use),
    // not in ten more of the scalar registers that pow() has already filled
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

// network blockIdx.y draws from its own slots: round c / w of the ring, world first + c % w of the batch
__global__ __launch_bounds__(DRAW_BLOCK) void lbank_draw_kernel(const BankDrawArgs a)
{
    const int64_t p = blockIdx.y;
    int64_t size = a.header[1];
    if (size < 0) size = 0;
    if (size > a.capacity) size = a.capacity;
    const int64_t rounds = size / a.N;
    int64_t first = 0, w = 0;
    if (p < a.used) {                                                  // p * seg < N: no overflow
        first = p * a.seg;
        w = a.N - first < a.seg ? a.N - first : a.seg;
    }
    const uint64_t size_p = static_cast<uint64_t>(rounds * w);         // <= capacity < 2^31
    const uint32_t w32 = static_cast<uint32_t>(w);
    const uint64_t t_new = a.t_dev[p] + 1;                             // the update this draw is for
    const uint64_t seed = a.seed[p];
    int32_t* const out = a.idx + p * a.B;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * DRAW_BLOCK;
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * DRAW_BLOCK + threadIdx.x; j < a.B; j += stride) {
        int32_t idx = -1;
#pragma unroll 1
        for (int att = 0; att < ATTEMPTS; ++att) {
            if (idx < 0) {
                uint32_t rr[4];
                draw<true>(seed, static_cast<uint64_t>(j), t_new, STREAM_LEARNER, static_cast<uint32_t>(att), rr);
                const uint64_t c = (static_cast<uint64_t>(rr[0]) * size_p) >> 32;
                if (c < size_p) {                                      // (so w >= 1)
                    const uint32_t c32 = static_cast<uint32_t>(c), round = c32 / w32;
                    const int64_t slot = static_cast<int64_t>(round) * a.N + first + (c32 - round * w32);
                    if (slot < a.capacity && a.ok[slot] != 0) idx = static_cast<int32_t>(slot);
                }
            }
        }
        out[j] = idx;
    }
}

// ------------------------------------------------------------------ host side
// the rules of aqualrn_update_f32 for one row; who: the network, for the message
int check_hyper(const double* h, long long who)
{
    const double gamma = h[H_GAMMA], tau = h[H_TAU], lr = h[H_LR], beta1 = h[H_BETA1], beta2 = h[H_BETA2], eps = h[H_EPS];
    if (!is_number(gamma) || !(gamma >= 0.0 && gamma <= 1.0)) return fail(AQUALBANK_E_INVALID, "network %lld: gamma=%g: must be in [0, 1]", who, gamma);
    if (!is_number(tau) || !(tau >= 0.0 && tau <= 1.0)) return fail(AQUALBANK_E_INVALID, "network %lld: tau=%g: must be in [0, 1]", who, tau);
    if (!is_number(lr) || !(lr >= 0.0)) return fail(AQUALBANK_E_INVALID, "network %lld: lr=%g: must be finite and >= 0", who, lr);
    if (!is_number(beta1) || !(beta1 >= 0.0 && beta1 < 1.0)) return fail(AQUALBANK_E_INVALID, "network %lld: beta1=%g: must be in [0, 1)", who, beta1);
    if (!is_number(beta2) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(AQUALBANK_E_INVALID, "network %lld: beta2=%g: must be in [0, 1)", who, beta2);
    if (!is_number(eps) || !(eps > 0.0)) return fail(AQUALBANK_E_INVALID, "network %lld: eps=%g: must be finite and > 0", who, eps);
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

int aqualbank_version(void) { return AQUALBANK_ABI_VERSION; }
const char* aqualbank_last_error(void) { return g_err; }

size_t aqualbank_workspace_bytes(int64_t P, int64_t B)
{
    if (P < 1 || P > AQUALBANK_MAX_NETWORKS || B < 0 || B > AQUALBANK_MAX_BATCH) return 0;
    return static_cast<size_t>(P) * workspace_region(B);
}

int aqualbank_pack_hyper(const double* in_host, int64_t P, double* out_host)
{
    if (in_host == nullptr || out_host == nullptr) return fail(AQUALBANK_E_INVALID, "in or out is NULL");
    if (P < 1 || P > AQUALBANK_MAX_NETWORKS) return fail(AQUALBANK_E_INVALID, "P=%lld: must be in [1, %d]", (long long)P, AQUALBANK_MAX_NETWORKS);
    if (!aligned(in_host, 8) || !aligned(out_host, 8)) return fail(AQUALBANK_E_ALIGN, "in / out must be 8-byte aligned");
    for (int64_t p = 0; p < P; ++p)
        if (const int rc = check_hyper(in_host + p * AQUALBANK_HYPER_FIELDS, (long long)p)) return rc;
    for (int64_t p = 0; p < P; ++p)
        for (int k = 0; k < HYPER; ++k) out_host[p * HYPER + k] = k < AQUALBANK_HYPER_FIELDS ? in_host[p * AQUALBANK_HYPER_FIELDS + k] : 0.0;
    return 0;
}

int aqualbank_update_f32(float* theta, float* theta_target, float* m, float* v, uint64_t* t_dev, int64_t P,
                         const float* s, const uint8_t* a, const float* r, const float* s2, const uint8_t* d,
                         const uint8_t* ok, int64_t ld, int64_t size,
                         const int32_t* idx, int64_t B, int strategy, const double* hyper_dev,
                         float* blob_online, float* blob_target, const int32_t* perm, int64_t blob_floats,
                         void* workspace, size_t workspace_bytes,
                         int32_t* idx_out, float* grad_out, float* loss, void* stream)
{
    if (P < 1 || P > AQUALBANK_MAX_NETWORKS) return fail(AQUALBANK_E_INVALID, "P=%lld: must be in [1, %d]", (long long)P, AQUALBANK_MAX_NETWORKS);
    if (theta == nullptr || theta_target == nullptr || m == nullptr || v == nullptr || t_dev == nullptr)
        return fail(AQUALBANK_E_INVALID, "theta, theta_target, m, v or t is NULL");
    const size_t stack = static_cast<size_t>(P) * PARAMS * sizeof(float);
    if (overlap(theta, theta_target, stack) || overlap(theta, m, stack) || overlap(theta, v, stack) || overlap(theta_target, m, stack) ||
        overlap(theta_target, v, stack) || overlap(m, v, stack))
        return fail(AQUALBANK_E_INVALID, "theta, theta_target, m and v must be four arrays of P x %d floats that do not overlap", PARAMS);
    if (B < 0 || B > AQUALBANK_MAX_BATCH) return fail(AQUALBANK_E_INVALID, "B=%lld: must be in [0, %d]", (long long)B, AQUALBANK_MAX_BATCH);
    if (ld < 0 || size < 0 || size > ld || ld > INT32_MAX)
        return fail(AQUALBANK_E_INVALID, "bad ring sizes: size=%lld ld=%lld", (long long)size, (long long)ld);
    const int loss_ref = (strategy & AQUALRN_LOSS_REFERENCE) != 0 ? 1 : 0;
    if (strategy >= 0) strategy &= ~AQUALRN_LOSS_REFERENCE;          // what is left: the bootstrap strategy, no other bit
    if (strategy < AQUALRN_DOUBLE_REF || strategy > AQUALRN_STANDARD) return fail(AQUALBANK_E_INVALID, "strategy=%d: unknown", strategy);
    if (hyper_dev == nullptr) return fail(AQUALBANK_E_INVALID, "the hyper-parameter table is NULL");
    if ((blob_online != nullptr || blob_target != nullptr) && perm == nullptr)
        return fail(AQUALBANK_E_INVALID, "a blob is given without the permutation table");
    if ((blob_online != nullptr || blob_target != nullptr) && blob_floats < AQUALBANK_PARAMS)
        return fail(AQUALBANK_E_INVALID, "blob_floats=%lld < %d", (long long)blob_floats, AQUALBANK_PARAMS);
    if ((blob_online != nullptr || blob_target != nullptr) && blob_floats > INT32_MAX)
        return fail(AQUALBANK_E_INVALID, "blob_floats=%lld: above %d", (long long)blob_floats, INT32_MAX);
    if (blob_online != nullptr && blob_target != nullptr && overlap(blob_online, blob_target, static_cast<size_t>(P) * blob_floats * sizeof(float)))
        return fail(AQUALBANK_E_INVALID, "blob_online and blob_target overlap");
    if (!aligned(theta, 4) || !aligned(theta_target, 4) || !aligned(m, 4) || !aligned(v, 4))
        return fail(AQUALBANK_E_ALIGN, "theta / theta_target / m / v must be 4-byte aligned");
    if (!aligned(t_dev, 8) || !aligned(hyper_dev, 8)) return fail(AQUALBANK_E_ALIGN, "t and the hyper-parameter table must be 8-byte aligned");
    if (!aligned(s, 4) || !aligned(s2, 4) || !aligned(r, 4)) return fail(AQUALBANK_E_ALIGN, "s / s2 / r must be 4-byte aligned");
    if (!aligned(idx, 4) || !aligned(idx_out, 4) || !aligned(perm, 4)) return fail(AQUALBANK_E_ALIGN, "idx / idx_out / perm must be 4-byte aligned");
    if (!aligned(blob_online, 4) || !aligned(blob_target, 4) || !aligned(grad_out, 4) || !aligned(loss, 4))
        return fail(AQUALBANK_E_ALIGN, "blobs / grad_out / loss must be 4-byte aligned");
    if (!aligned(workspace, 16)) return fail(AQUALBANK_E_ALIGN, "the workspace must be 16-byte aligned");
    if (B == 0) return 0;
    if (idx == nullptr) return fail(AQUALBANK_E_INVALID, "idx is NULL: the bank has no in-kernel draw (aqualbank_draw)");
    if (s == nullptr || a == nullptr || r == nullptr || s2 == nullptr || d == nullptr || ok == nullptr)
        return fail(AQUALBANK_E_INVALID, "a ring buffer is NULL");
    if (workspace == nullptr) return fail(AQUALBANK_E_INVALID, "workspace is NULL");
    if (workspace_bytes < aqualbank_workspace_bytes(P, B))
        return fail(AQUALBANK_E_INVALID, "workspace too small: %zu < %zu bytes", workspace_bytes, aqualbank_workspace_bytes(P, B));

    const Shape sh = shape_of(B);
    BankGradArgs g;
    g.theta = theta; g.theta_target = theta_target; g.t_dev = t_dev;
    g.s = s; g.a = a; g.r = r; g.s2 = s2; g.d = d; g.ok = ok;
    g.ld = ld; g.size = size; g.B = B; g.idx = idx; g.hyper = hyper_dev;
    g.tiles_per_wave = sh.tiles_per_wave;
    g.loss_ref = loss_ref;
    g.ws = static_cast<char*>(workspace);
    g.region = static_cast<int64_t>(workspace_region(B));
    g.idx_out = idx_out;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned>(sh.groups), static_cast<unsigned>(P)), block(BLOCK);
    switch (strategy) {
    case AQUALRN_DOUBLE_REF: hipLaunchKernelGGL((lbank_grad_kernel<AQUALRN_DOUBLE_REF>), grid, block, 0, st, g); break;
    case AQUALRN_DOUBLE: hipLaunchKernelGGL((lbank_grad_kernel<AQUALRN_DOUBLE>), grid, block, 0, st, g); break;
    case AQUALRN_FIXED: hipLaunchKernelGGL((lbank_grad_kernel<AQUALRN_FIXED>), grid, block, 0, st, g); break;
    default: hipLaunchKernelGGL((lbank_grad_kernel<AQUALRN_STANDARD>), grid, block, 0, st, g); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "lbank_grad_kernel launch");

    BankApplyArgs q;
    q.theta = theta; q.theta_target = theta_target; q.m = m; q.v = v; q.t_dev = t_dev;
    q.ws = g.ws; q.region = g.region; q.partials = sh.groups; q.hyper = hyper_dev;
    q.blob_online = blob_online; q.blob_target = blob_target; q.perm = perm; q.blob_floats = blob_floats;
    q.grad_out = grad_out; q.loss = loss;
    hipLaunchKernelGGL(lbank_apply_kernel, dim3(APPLY_GROUPS, static_cast<unsigned>(P)), dim3(APPLY_BLOCK), 0, st, q);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "lbank_apply_kernel launch");
    return 0;
}

int aqualbank_draw(const int64_t* header, const uint8_t* ok, int64_t capacity, int64_t N, int64_t seg, int64_t P,
                   const uint64_t* t_dev, const uint64_t* seed_dev, int32_t* idx, int64_t B, void* stream)
{
    if (header == nullptr || ok == nullptr || t_dev == nullptr || seed_dev == nullptr)
        return fail(AQUALBANK_E_INVALID, "header, ok, t_dev or seed_dev is NULL");
    if (P < 1 || P > AQUALBANK_MAX_NETWORKS) return fail(AQUALBANK_E_INVALID, "P=%lld: must be in [1, %d]", (long long)P, AQUALBANK_MAX_NETWORKS);
    if (capacity <= 0 || capacity > AQUALBANK_MAX_CAPACITY)
        return fail(AQUALBANK_E_INVALID, "capacity=%lld: must be in [1, %d]", (long long)capacity, AQUALBANK_MAX_CAPACITY);
    if (N < 1 || N > capacity) return fail(AQUALBANK_E_INVALID, "N=%lld: must be in [1, capacity=%lld]", (long long)N, (long long)capacity);
    if (capacity % N != 0)
        return fail(AQUALBANK_E_INVALID, "capacity=%lld is no multiple of N=%lld: a slot would not belong to one world", (long long)capacity, (long long)N);
    if (seg < 1) return fail(AQUALBANK_E_INVALID, "seg=%lld: must be >= 1", (long long)seg);
    if (B < 0 || B > AQUALBANK_MAX_BATCH) return fail(AQUALBANK_E_INVALID, "B=%lld: must be in [0, %d]", (long long)B, AQUALBANK_MAX_BATCH);
    if (!aligned(header, 8) || !aligned(t_dev, 8) || !aligned(seed_dev, 8)) return fail(AQUALBANK_E_ALIGN, "header / t_dev / seed_dev must be 8-byte aligned");
    if (!aligned(idx, 4)) return fail(AQUALBANK_E_ALIGN, "idx must be 4-byte aligned");
    if (B == 0) return 0;
    if (idx == nullptr) return fail(AQUALBANK_E_INVALID, "idx is NULL");

    BankDrawArgs k;
    k.header = header; k.ok = ok; k.capacity = capacity; k.N = N; k.seg = seg;
    k.used = N / seg + (N % seg != 0 ? 1 : 0);
    k.t_dev = t_dev; k.seed = seed_dev; k.idx = idx; k.B = B;
    int64_t blocks = (B + DRAW_BLOCK - 1) / DRAW_BLOCK;
    if (blocks > DRAW_MAX_BLOCKS) blocks = DRAW_MAX_BLOCKS;
    hipLaunchKernelGGL(lbank_draw_kernel, dim3(static_cast<unsigned>(blocks), static_cast<unsigned>(P)), dim3(DRAW_BLOCK), 0,
                       static_cast<hipStream_t>(stream), k);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "lbank_draw_kernel launch");
    return 0;
}

}  // extern "C"
