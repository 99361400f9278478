// aqua_replay.hip -- libaqua_replay.so (include/aqua_replay.h): the experience ring of a batch of worlds with its cursor
// and size in device memory, so that append, draw and update replay correctly from one captured graph.
// Its own translation unit and library: the other five libraries and their kernels are not touched by it.
//
// Four kernels, one launch per entry point, ordered by the stream and by nothing else:
//   rpl_open_kernel     (s, a, ok) of world i into slot header[0] + i (mod capacity); one lane stores header[2] = header[0]
//   rpl_close_kernel    (r, s', d) into the slots that start at header[2]; one lane advances header[0], [1], [3]
//   rpl_draw_kernel     the learner's minibatch draw with the size read from header[1]
//   rpl_gather_kernel   dense [B][5] rows of the slots idx names
// No thread reads a header word that another thread of the same launch writes; no block waits on
// another block; no fence, flag, ticket or atomic; no floating-point arithmetic: the kernels copy and draw integers.
// The cursor is arbitrary, so the ring side of every copy is one dword or one byte per lane; consecutive worlds land in
// consecutive slots, and the wrap splits the store of one wavefront at most.
#include <hip/hip_runtime.h>

#include "../../include/aqua_replay.h"
#include "aqua_device.hpp"
#include "aqua_host.hpp"
#include "aqua_qnet.hpp"

namespace {

using aqua::draw;
using aqua::qnet::STREAM_LEARNER;

static_assert(STREAM_LEARNER == AQUARPL_STREAM, "the draw reproduces the learner's own: the learner's stream");

constexpr int BLOCK = AQUARPL_BLOCK;
constexpr int MAX_BLOCKS = AQUARPL_MAX_BLOCKS;
constexpr int ROWS = 5;                               // the observation (main/impl/utils.py:15-33)

struct OpenArgs {
    int64_t* header;
    float* s;
    void* a;
    uint8_t* ok;
    int64_t ring_ld, capacity;
    const float* obs;
    int64_t obs_ld;
    const void* action;
    int kind;
    int64_t action_ld;
    const int32_t* time;
    int64_t N;
};

struct CloseArgs {
    int64_t* header;
    float* r;
    float* s2;
    uint8_t* d;
    int64_t ring_ld, capacity;
    const float* reward;
    const float* obs;
    int64_t obs_ld;
    const uint8_t* term;
    int64_t N;
};

struct DrawArgs {
    const int64_t* header;
    const uint8_t* ok;
    int64_t capacity;
    const uint64_t* t_dev;
    uint64_t seed;
    int32_t* idx;
    int64_t B;
};

struct GatherArgs {
    const int32_t* idx;
    int64_t B;
    const float* s;
    const void* a;
    const float* r;
    const float* s2;
    const uint8_t* d;
    const uint8_t* ok;
    int64_t ring_ld, capacity;
    int kind;
    float* out_s;
    void* out_a;
    float* out_r;
    float* out_s2;
    uint8_t* out_done;
    uint8_t* out_valid;
};

__global__ __launch_bounds__(BLOCK) void rpl_open_kernel(const OpenArgs a)
{
    const int64_t base = a.header[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) a.header[2] = base;       // (nobody reads [2] in this launch)
    if (base < 0 || base >= a.capacity) return;                        // never an address
    const int64_t stride = static_cast<int64_t>(gridDim.x) * BLOCK;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x; i < a.N; i += stride) {
        int64_t slot = base + i;                                       // base < capacity, i < N <= capacity
        if (slot >= a.capacity) slot -= a.capacity;
#pragma unroll
        for (int row = 0; row < ROWS; ++row) a.s[row * a.ring_ld + slot] = a.obs[row * a.obs_ld + i];
        if (a.kind == AQUARPL_ACT_U8) {
            static_cast<uint8_t*>(a.a)[slot] = static_cast<const uint8_t*>(a.action)[i];
        } else {
            const float* src = static_cast<const float*>(a.action);
            float* dst = static_cast<float*>(a.a);
            dst[slot] = src[i];
            dst[a.ring_ld + slot] = src[a.action_ld + i];
        }
        bool live = true;
        if (a.time != nullptr) {
            const int32_t t = a.time[i];
            live = t >= 0 || t <= -3;                                  // time markers: include/aqua_hip.h
        }
        a.ok[slot] = live ? 1 : 0;
    }
}

__global__ __launch_bounds__(BLOCK) void rpl_close_kernel(const CloseArgs a)
{
    const int64_t base = a.header[2];
    if (base < 0 || base >= a.capacity) return;                        // never an address; the header stays as it was
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the only lane that reads [1] and [3]; nobody reads [0] in this launch
        int64_t next = base + a.N;                                     // < 2 capacity
        if (next >= a.capacity) next -= a.capacity;
        int64_t size = a.header[1];
        if (size < 0) size = 0;
        size = size > a.capacity - a.N ? a.capacity : size + a.N;
        a.header[0] = next;
        a.header[1] = size;
        a.header[3] = a.header[3] + 1;
    }
    const int64_t stride = static_cast<int64_t>(gridDim.x) * BLOCK;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x; i < a.N; i += stride) {
        int64_t slot = base + i;
        if (slot >= a.capacity) slot -= a.capacity;
        a.r[slot] = a.reward[i];
#pragma unroll
        for (int row = 0; row < ROWS; ++row) a.s2[row * a.ring_ld + slot] = a.obs[row * a.obs_ld + i];
        a.d[slot] = a.term[i];
    }
}

__global__ __launch_bounds__(BLOCK) void rpl_draw_kernel(const DrawArgs a)
{
    int64_t size = a.header[1];
    if (size < 0) size = 0;
    if (size > a.capacity) size = a.capacity;
    const uint64_t t_new = *a.t_dev + 1;                               // the update this draw is for
    const int64_t stride = static_cast<int64_t>(gridDim.x) * BLOCK;
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x; j < a.B; j += stride) {
        int32_t idx = -1;
#pragma unroll 1
        for (int att = 0; att < AQUARPL_ATTEMPTS; ++att) {
            if (idx < 0) {
                uint32_t rr[4];
                draw<true>(a.seed, static_cast<uint64_t>(j), t_new, STREAM_LEARNER, static_cast<uint32_t>(att), rr);
                const int64_t c = static_cast<int64_t>((static_cast<uint64_t>(rr[0]) * static_cast<uint64_t>(size)) >> 32);
                if (c < size && a.ok[c] != 0) idx = static_cast<int32_t>(c);
            }
        }
        a.idx[j] = idx;
    }
}

__global__ __launch_bounds__(BLOCK) void rpl_gather_kernel(const GatherArgs a)
{
    const int64_t stride = static_cast<int64_t>(gridDim.x) * BLOCK;
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x; j < a.B; j += stride) {
        const int64_t c = a.idx[j];
        bool valid = c >= 0 && c < a.capacity;
        if (valid) valid = a.ok[c] != 0;
        // zeros as bit patterns: the rows are copied, never computed with
        uint32_t x[ROWS], x2[ROWS], rew = 0, act0 = 0, act1 = 0;
        uint8_t done = 0;
#pragma unroll
        for (int row = 0; row < ROWS; ++row) {
            x[row] = valid ? reinterpret_cast<const uint32_t*>(a.s)[row * a.ring_ld + c] : 0u;
            x2[row] = valid ? reinterpret_cast<const uint32_t*>(a.s2)[row * a.ring_ld + c] : 0u;
        }
        if (valid) {
            rew = reinterpret_cast<const uint32_t*>(a.r)[c];
            done = a.d[c] != 0 ? 1 : 0;
            if (a.kind == AQUARPL_ACT_U8) {
                act0 = static_cast<const uint8_t*>(a.a)[c];
            } else {
                act0 = static_cast<const uint32_t*>(a.a)[c];
                act1 = static_cast<const uint32_t*>(a.a)[a.ring_ld + c];
            }
        }
#pragma unroll
        for (int row = 0; row < ROWS; ++row) {
            reinterpret_cast<uint32_t*>(a.out_s)[j * ROWS + row] = x[row];
            reinterpret_cast<uint32_t*>(a.out_s2)[j * ROWS + row] = x2[row];
        }
        reinterpret_cast<uint32_t*>(a.out_r)[j] = rew;
        if (a.kind == AQUARPL_ACT_U8) {
            static_cast<uint8_t*>(a.out_a)[j] = static_cast<uint8_t>(act0);
        } else {
            static_cast<uint32_t*>(a.out_a)[2 * j] = act0;
            static_cast<uint32_t*>(a.out_a)[2 * j + 1] = act1;
        }
        a.out_done[j] = done;
        a.out_valid[j] = valid ? 1 : 0;
    }
}

// ------------------------------------------------------------------ host side
unsigned grid_of(int64_t n)
{
    int64_t blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
    return static_cast<unsigned>(blocks < 1 ? 1 : blocks);
}

// what open and close share: the header, the ring's shape and the batch
int check_ring(const int64_t* header, int64_t ring_ld, int64_t capacity, int64_t obs_ld, int64_t N)
{
    if (header == nullptr) return fail(AQUARPL_E_INVALID, "header is NULL");
    if (!aligned(header, 8)) return fail(AQUARPL_E_ALIGN, "header must be 8-byte aligned");
    if (capacity <= 0 || capacity > AQUARPL_MAX_CAPACITY)
        return fail(AQUARPL_E_INVALID, "capacity=%lld: must be in [1, %d]", (long long)capacity, AQUARPL_MAX_CAPACITY);
    if (ring_ld < capacity) return fail(AQUARPL_E_INVALID, "ring_ld=%lld: below the capacity %lld", (long long)ring_ld, (long long)capacity);
    if (N < 0 || N > capacity) return fail(AQUARPL_E_INVALID, "N=%lld: the ring must hold one batched step (capacity=%lld)", (long long)N, (long long)capacity);
    if (obs_ld < N) return fail(AQUARPL_E_INVALID, "obs_ld=%lld: below N=%lld", (long long)obs_ld, (long long)N);
    return 0;
}

int check_kind(int kind)
{
    if (kind != AQUARPL_ACT_U8 && kind != AQUARPL_ACT_F32X2) return fail(AQUARPL_E_INVALID, "action_kind=%d: AQUARPL_ACT_U8 or AQUARPL_ACT_F32X2", kind);
    return 0;
}

}  // namespace

extern "C" {

int aquarpl_version(void) { return AQUARPL_ABI_VERSION; }
const char* aquarpl_last_error(void) { return g_err; }

int aquarpl_open(int64_t* header, float* s, void* a, uint8_t* ok, int64_t ring_ld, int64_t capacity,
                 const float* obs, int64_t obs_ld, const void* action, int action_kind, int64_t action_ld,
                 const int32_t* time, int64_t N, void* stream)
{
    if (int rc = check_ring(header, ring_ld, capacity, obs_ld, N)) return rc;
    if (int rc = check_kind(action_kind)) return rc;
    if (action_kind == AQUARPL_ACT_F32X2 && action_ld < N)
        return fail(AQUARPL_E_INVALID, "action_ld=%lld: below N=%lld", (long long)action_ld, (long long)N);
    if (s == nullptr || a == nullptr || ok == nullptr) return fail(AQUARPL_E_INVALID, "s, a or ok is NULL");
    if (!aligned(s, 4) || !aligned(obs, 4) || !aligned(time, 4)) return fail(AQUARPL_E_ALIGN, "s / obs / time must be 4-byte aligned");
    if (action_kind == AQUARPL_ACT_F32X2 && (!aligned(a, 4) || !aligned(action, 4)))
        return fail(AQUARPL_E_ALIGN, "float32 action rows must be 4-byte aligned");
    if (N == 0) return 0;
    if (obs == nullptr || action == nullptr) return fail(AQUARPL_E_INVALID, "obs or action is NULL");

    OpenArgs k;
    k.header = header; k.s = s; k.a = a; k.ok = ok; k.ring_ld = ring_ld; k.capacity = capacity;
    k.obs = obs; k.obs_ld = obs_ld; k.action = action; k.kind = action_kind; k.action_ld = action_ld; k.time = time; k.N = N;
    hipLaunchKernelGGL(rpl_open_kernel, dim3(grid_of(N)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), k);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "rpl_open_kernel launch");
    return 0;
}

int aquarpl_close(int64_t* header, float* r, float* s2, uint8_t* d, int64_t ring_ld, int64_t capacity,
                  const float* reward, const float* obs, int64_t obs_ld, const uint8_t* term, int64_t N, void* stream)
{
    if (int rc = check_ring(header, ring_ld, capacity, obs_ld, N)) return rc;
    if (r == nullptr || s2 == nullptr || d == nullptr) return fail(AQUARPL_E_INVALID, "r, s2 or d is NULL");
    if (!aligned(r, 4) || !aligned(s2, 4) || !aligned(reward, 4) || !aligned(obs, 4))
        return fail(AQUARPL_E_ALIGN, "r / s2 / reward / obs must be 4-byte aligned");
    if (N == 0) return 0;
    if (reward == nullptr || obs == nullptr || term == nullptr) return fail(AQUARPL_E_INVALID, "reward, obs or term is NULL");

    CloseArgs k;
    k.header = header; k.r = r; k.s2 = s2; k.d = d; k.ring_ld = ring_ld; k.capacity = capacity;
    k.reward = reward; k.obs = obs; k.obs_ld = obs_ld; k.term = term; k.N = N;
    hipLaunchKernelGGL(rpl_close_kernel, dim3(grid_of(N)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), k);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "rpl_close_kernel launch");
    return 0;
}

int aquarpl_draw(const int64_t* header, const uint8_t* ok, int64_t capacity, const uint64_t* t_dev, uint64_t seed,
                 int32_t* idx, int64_t B, void* stream)
{
    if (header == nullptr || ok == nullptr || t_dev == nullptr) return fail(AQUARPL_E_INVALID, "header, ok or t_dev is NULL");
    if (capacity <= 0 || capacity > AQUARPL_MAX_CAPACITY)
        return fail(AQUARPL_E_INVALID, "capacity=%lld: must be in [1, %d]", (long long)capacity, AQUARPL_MAX_CAPACITY);
    if (B < 0 || B > AQUARPL_MAX_BATCH) return fail(AQUARPL_E_INVALID, "B=%lld: must be in [0, %d]", (long long)B, AQUARPL_MAX_BATCH);
    if (!aligned(header, 8) || !aligned(t_dev, 8)) return fail(AQUARPL_E_ALIGN, "header / t_dev must be 8-byte aligned");
    if (!aligned(idx, 4)) return fail(AQUARPL_E_ALIGN, "idx must be 4-byte aligned");
    if (B == 0) return 0;
    if (idx == nullptr) return fail(AQUARPL_E_INVALID, "idx is NULL");

    DrawArgs k;
    k.header = header; k.ok = ok; k.capacity = capacity; k.t_dev = t_dev; k.seed = seed; k.idx = idx; k.B = B;
    hipLaunchKernelGGL(rpl_draw_kernel, dim3(grid_of(B)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), k);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "rpl_draw_kernel launch");
    return 0;
}

int aquarpl_gather(const int32_t* idx, int64_t B, const float* s, const void* a, const float* r, const float* s2,
                   const uint8_t* d, const uint8_t* ok, int64_t ring_ld, int64_t capacity, int action_kind,
                   float* out_s, void* out_a, float* out_r, float* out_s2, uint8_t* out_done, uint8_t* out_valid,
                   void* stream)
{
    if (s == nullptr || a == nullptr || r == nullptr || s2 == nullptr || d == nullptr || ok == nullptr)
        return fail(AQUARPL_E_INVALID, "s, a, r, s2, d or ok is NULL");
    if (capacity <= 0 || capacity > AQUARPL_MAX_CAPACITY)
        return fail(AQUARPL_E_INVALID, "capacity=%lld: must be in [1, %d]", (long long)capacity, AQUARPL_MAX_CAPACITY);
    if (ring_ld < capacity) return fail(AQUARPL_E_INVALID, "ring_ld=%lld: below the capacity %lld", (long long)ring_ld, (long long)capacity);
    if (B < 0 || B > AQUARPL_MAX_BATCH) return fail(AQUARPL_E_INVALID, "B=%lld: must be in [0, %d]", (long long)B, AQUARPL_MAX_BATCH);
    if (int rc = check_kind(action_kind)) return rc;
    if (!aligned(idx, 4) || !aligned(s, 4) || !aligned(r, 4) || !aligned(s2, 4) || !aligned(out_s, 4) || !aligned(out_r, 4) || !aligned(out_s2, 4))
        return fail(AQUARPL_E_ALIGN, "idx and the float32 rows must be 4-byte aligned");
    if (action_kind == AQUARPL_ACT_F32X2 && (!aligned(a, 4) || !aligned(out_a, 4)))
        return fail(AQUARPL_E_ALIGN, "float32 action rows must be 4-byte aligned");
    if (B == 0) return 0;
    if (idx == nullptr) return fail(AQUARPL_E_INVALID, "idx is NULL");
    if (out_s == nullptr || out_a == nullptr || out_r == nullptr || out_s2 == nullptr || out_done == nullptr || out_valid == nullptr)
        return fail(AQUARPL_E_INVALID, "out_s, out_a, out_r, out_s2, out_done or out_valid is NULL");

    GatherArgs k;
    k.idx = idx; k.B = B; k.s = s; k.a = a; k.r = r; k.s2 = s2; k.d = d; k.ok = ok; k.ring_ld = ring_ld; k.capacity = capacity;
    k.kind = action_kind; k.out_s = out_s; k.out_a = out_a; k.out_r = out_r; k.out_s2 = out_s2; k.out_done = out_done;
    k.out_valid = out_valid;
    hipLaunchKernelGGL(rpl_gather_kernel, dim3(grid_of(B)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), k);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "rpl_gather_kernel launch");
    return 0;
}

}  // extern "C"
