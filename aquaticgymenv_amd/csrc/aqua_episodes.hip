// aqua_episodes.hip -- libaqua_episodes.so (include/aqua_episodes.h): per-world running return and length, an ordered log
// of finished episodes, counters by termination code and the epsilon schedule of main/impl/dqn.py:139-141,184 for a batch
// of worlds on gfx950, and the exploration pass that applies that device-resident epsilon to greedy actions.
// Its own translation unit and library: the other three libraries and their kernels are not touched by it.
//
// The substance is an ordered stream compaction (DESIGN.md "Episode accounting on the device"): the worlds that end in a
// step take consecutive slots of the log in index order.  Two launches, ordered by the stream and by nothing else:
//   ep_account_kernel   return / length of the counted worlds, ending worlds counted per block (ballot + popcount per
//                       wavefront), block counts into the workspace, shares of counts[] by integer atomics
//   ep_scatter_kernel   offset of a block = sum of the counts below it, rank inside the block from ballots in index order,
//                       records written, ending worlds back to zero; block 0 advances the epsilon schedule
// No block waits on another block; no fence, flag or ticket; no floating-point atomics.
#include <hip/hip_runtime.h>

#include "../../include/aqua_episodes.h"
#include "aqua_device.hpp"
#include "aqua_host.hpp"
#include "aqua_qnet.hpp"

namespace {

using aqua::draw;
using aqua::u_01;
using aqua::qnet::random_action;
using aqua::qnet::STREAM_POLICY;

static_assert(STREAM_POLICY == AQUAEP_STREAM, "the exploration pass reproduces the policy kernel's draw: the policy's stream");

constexpr int BLOCK = 256, WAVES = BLOCK / 64;
constexpr int MAX_BLOCKS = AQUAEP_MAX_BLOCKS;
constexpr int EXPLORE_MAX_BLOCKS = 2048;

struct AccountArgs {
    const float* reward;
    const uint8_t* term;
    const int32_t* time;
    const uint8_t* finished;
    float* ret;
    int32_t* len;
    int64_t N, chunk;
    uint32_t* block_counts;
    unsigned long long* counts;
};

struct ScatterArgs {
    const uint8_t* term;
    uint8_t* finished;
    float* ret;
    int32_t* len;
    int64_t N, chunk, env_offset, C;
    float* log_ret;
    int32_t* log_len;
    uint8_t* log_code;
    int64_t* log_world;
    const uint32_t* block_counts;
    int blocks;
    const unsigned long long* counts;
    double* eps_state;
    float* eps_out;
    double decay, eps_final;
};

struct ExploreArgs {
    uint8_t* action;
    int64_t N, env_offset;
    const float* eps;
    uint64_t seed, tick;
    const uint64_t* tick_base;
};

__device__ __forceinline__ uint32_t popc64(uint64_t m) { return static_cast<uint32_t>(__builtin_popcountll(m)); }

// lanes of `mask` below this lane
__device__ __forceinline__ uint32_t rank_in(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// slot 0: ending worlds, 1..3: by code, 4: counted world-steps
__global__ __launch_bounds__(BLOCK) void ep_account_kernel(const AccountArgs a)
{
#pragma clang fp contract(off)
    __shared__ uint32_t s_cnt[5];
    if (threadIdx.x < 5) s_cnt[threadIdx.x] = 0;
    __syncthreads();

    const int64_t begin = static_cast<int64_t>(blockIdx.x) * a.chunk;
    const int64_t end = begin + a.chunk < a.N ? begin + a.chunk : a.N;
    uint32_t n_end = 0, n1 = 0, n2 = 0, n3 = 0, n_steps = 0;            // wave-uniform
    for (int64_t tile = begin; tile < end; tile += BLOCK) {
        const int64_t i = tile + threadIdx.x;
        bool counted = false;
        uint32_t code = 0;
        if (i < end) {
            code = a.term[i];
            counted = (a.finished == nullptr || a.finished[i] == 0) && (a.time == nullptr || code != 0 || a.time[i] >= 0);
            if (counted) {
                a.ret[i] = a.ret[i] + a.reward[i];
                a.len[i] = a.len[i] + 1;
            }
        }
        const bool ends = counted && code != 0;
        n_steps += popc64(__builtin_amdgcn_ballot_w64(counted));
        const uint64_t m = __builtin_amdgcn_ballot_w64(ends);
        if (m != 0) {
            n_end += popc64(m);
            n1 += popc64(__builtin_amdgcn_ballot_w64(ends && code == 1));
            n2 += popc64(__builtin_amdgcn_ballot_w64(ends && code == 2));
            n3 += popc64(__builtin_amdgcn_ballot_w64(ends && code == 3));
        }
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_end != 0) atomicAdd(&s_cnt[0], n_end);
        if (n1 != 0) atomicAdd(&s_cnt[1], n1);
        if (n2 != 0) atomicAdd(&s_cnt[2], n2);
        if (n3 != 0) atomicAdd(&s_cnt[3], n3);
        if (n_steps != 0) atomicAdd(&s_cnt[4], n_steps);
    }
    __syncthreads();
    if (threadIdx.x == 0) a.block_counts[blockIdx.x] = s_cnt[0];
    if (threadIdx.x < 5) {
        const uint32_t v = s_cnt[threadIdx.x];
        if (v != 0) atomicAdd(&a.counts[threadIdx.x], static_cast<unsigned long long>(v));
    }
}

__global__ __launch_bounds__(BLOCK) void ep_scatter_kernel(const ScatterArgs a)
{
#pragma clang fp contract(off)
    __shared__ uint32_t s_part[2][WAVES];
    __shared__ uint32_t s_wave[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t mine = a.block_counts[blockIdx.x];
    if (mine == 0 && blockIdx.x != 0) return;                          // (the whole block: nothing of it ends)

    // the ending worlds of the blocks below this one, and of all blocks
    uint32_t lower = 0, total = 0;
    for (int j = threadIdx.x; j < a.blocks; j += BLOCK) {
        const uint32_t c = a.block_counts[j];
        total += c;
        if (j < static_cast<int>(blockIdx.x)) lower += c;
    }
    lower = wave_sum(lower);
    total = wave_sum(total);
    if (lane == 0) { s_part[0][wave] = lower; s_part[1][wave] = total; }
    __syncthreads();
    lower = total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) { lower += s_part[0][w]; total += s_part[1][w]; }

    if (blockIdx.x == 0 && threadIdx.x == 0 && a.eps_state != nullptr) {
        double result = 1.0, base = a.decay;                           // decay^total, least-significant bit first
        for (uint32_t n = total; n != 0; n >>= 1) {
            if (n & 1u) result *= base;
            base *= base;
        }
        double e = *a.eps_state * result;
        e = e > a.eps_final ? e : a.eps_final;
        *a.eps_state = e;
        *a.eps_out = static_cast<float>(e);
    }
    if (mine == 0) return;

    // the account launch has advanced counts[0] by `total`: the cursor before the call, then this block's first slot
    const uint64_t C = static_cast<uint64_t>(a.C);
    uint64_t slot0 = ((static_cast<uint64_t>(a.counts[0]) - total) % C + lower) % C;      // uniform: one division per block
    const int64_t begin = static_cast<int64_t>(blockIdx.x) * a.chunk;
    const int64_t end = begin + a.chunk < a.N ? begin + a.chunk : a.N;
    uint32_t logged = 0;
    for (int64_t tile = begin; tile < end && logged < mine; tile += BLOCK) {
        const int64_t i = tile + threadIdx.x;
        uint32_t code = 0;
        bool ends = false;
        if (i < end) {
            code = a.term[i];
            ends = code != 0 && (a.finished == nullptr || a.finished[i] == 0);
        }
        const uint64_t m = __builtin_amdgcn_ballot_w64(ends);
        if (lane == 0) s_wave[wave] = popc64(m);
        __syncthreads();
        uint32_t before = 0, in_tile = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const uint32_t c = s_wave[w];
            in_tile += c;
            if (w < wave) before += c;
        }
        if (ends) {
            uint64_t slot = slot0 + before + rank_in(m);               // < 2 C, see below
            if (slot >= C) slot -= C;
            a.log_ret[slot] = a.ret[i];
            a.log_len[slot] = a.len[i];
            a.log_code[slot] = static_cast<uint8_t>(code);
            a.log_world[slot] = a.env_offset + i;
            a.ret[i] = 0.0f;
            a.len[i] = 0;
            if (a.finished != nullptr) a.finished[i] = 1;
        }
        // slot0 stays reduced: slot0 < C and in_tile <= end - begin <= N <= C, so slot0 + in_tile < 2 C
        slot0 += in_tile;
        if (slot0 >= C) slot0 -= C;
        logged += in_tile;
        __syncthreads();                                               // s_wave is rewritten by the next tile
    }
}

__global__ __launch_bounds__(BLOCK) void ep_explore_kernel(const ExploreArgs a)
{
    const float eps = *a.eps;
    if (!(eps > 0.0f)) return;
    uint64_t tick = a.tick;
    if (a.tick_base != nullptr) tick += *a.tick_base;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * BLOCK;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x; i < a.N; i += stride) {
        uint32_t r[4];
        // (the scalar-key form: the seed is a kernel argument; as plain draw() the ten round keys are hoisted out of the loop
        // into SGPRs that spill.  The same ten rounds, the same bits as the policy kernel's draw)
        draw<true>(a.seed, static_cast<uint64_t>(a.env_offset + i), tick, STREAM_POLICY, 0, r);
        if (u_01(r[0]) < eps) a.action[i] = static_cast<uint8_t>(random_action(r));
    }
}

// ------------------------------------------------------------------ host side
// the launch shape: a function of N alone
struct Shape {
    int64_t chunk;
    int blocks;
};

Shape shape_of(int64_t N)
{
    const int64_t tiles = (N + BLOCK - 1) / BLOCK;
    const int64_t tiles_per_block = (tiles + MAX_BLOCKS - 1) / MAX_BLOCKS;
    Shape s;
    s.chunk = (tiles_per_block < 1 ? 1 : tiles_per_block) * BLOCK;
    s.blocks = static_cast<int>((N + s.chunk - 1) / s.chunk);
    return s;
}

}  // namespace

extern "C" {

int aquaep_version(void) { return AQUAEP_ABI_VERSION; }
const char* aquaep_last_error(void) { return g_err; }

size_t aquaep_workspace_bytes(int64_t N)
{
    if (N < 0 || N > AQUAEP_MAX_WORLDS) return 0;
    // an upper bound of shape_of(N).blocks that never decreases with N: one uint32 per block, in units of 16 bytes
    int64_t blocks = (N + BLOCK - 1) / BLOCK;
    if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
    if (blocks < 4) blocks = 4;
    return static_cast<size_t>((blocks + 3) / 4) * 16;
}

int aquaep_after_step_f32(const float* reward, const uint8_t* term, const int32_t* time, int64_t env_offset, int64_t N,
                          float* ret, int32_t* len, uint8_t* finished,
                          float* log_ret, int32_t* log_len, uint8_t* log_code, int64_t* log_world, int64_t C,
                          uint64_t* counts, double* eps_state, float* eps_out, double decay, double eps_final,
                          void* workspace, size_t workspace_bytes, void* stream)
{
    if (ret == nullptr || len == nullptr || counts == nullptr) return fail(AQUAEP_E_INVALID, "ret, len or counts is NULL");
    if (log_ret == nullptr || log_len == nullptr || log_code == nullptr || log_world == nullptr)
        return fail(AQUAEP_E_INVALID, "log_ret, log_len, log_code or log_world is NULL");
    if (N < 0 || N > AQUAEP_MAX_WORLDS) return fail(AQUAEP_E_INVALID, "N=%lld: must be in [0, %d]", (long long)N, AQUAEP_MAX_WORLDS);
    if (C < N) return fail(AQUAEP_E_INVALID, "C=%lld: the log must hold one batched step (N=%lld)", (long long)C, (long long)N);
    if (env_offset < 0) return fail(AQUAEP_E_INVALID, "env_offset < 0");
    if ((eps_state == nullptr) != (eps_out == nullptr))
        return fail(AQUAEP_E_INVALID, "eps_state and eps_out: give both, or neither to switch the schedule off");
    if (!is_number(decay) || !(decay > 0.0 && decay <= 1.0)) return fail(AQUAEP_E_INVALID, "decay=%g: must be in (0, 1]", decay);
    if (!is_number(eps_final) || !(eps_final >= 0.0)) return fail(AQUAEP_E_INVALID, "eps_final=%g: must be a number >= 0", eps_final);
    if (!aligned(reward, 4) || !aligned(time, 4) || !aligned(ret, 4) || !aligned(len, 4))
        return fail(AQUAEP_E_ALIGN, "reward / time / ret / len must be 4-byte aligned");
    if (!aligned(log_ret, 4) || !aligned(log_len, 4) || !aligned(log_world, 8))
        return fail(AQUAEP_E_ALIGN, "log_ret / log_len must be 4-byte, log_world 8-byte aligned");
    if (!aligned(counts, 8) || !aligned(eps_state, 8) || !aligned(eps_out, 4))
        return fail(AQUAEP_E_ALIGN, "counts / eps_state must be 8-byte, eps_out 4-byte aligned");
    if (!aligned(workspace, 16)) return fail(AQUAEP_E_ALIGN, "the workspace must be 16-byte aligned");
    if (N == 0) return 0;
    if (reward == nullptr || term == nullptr) return fail(AQUAEP_E_INVALID, "reward or term is NULL");
    if (workspace == nullptr) return fail(AQUAEP_E_INVALID, "workspace is NULL");
    if (workspace_bytes < aquaep_workspace_bytes(N))
        return fail(AQUAEP_E_INVALID, "workspace too small: %zu < %zu bytes", workspace_bytes, aquaep_workspace_bytes(N));

    const Shape sh = shape_of(N);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<unsigned>(sh.blocks)), block(BLOCK);

    AccountArgs k;
    k.reward = reward; k.term = term; k.time = time; k.finished = finished; k.ret = ret; k.len = len;
    k.N = N; k.chunk = sh.chunk;
    k.block_counts = static_cast<uint32_t*>(workspace);
    k.counts = reinterpret_cast<unsigned long long*>(counts);
    hipLaunchKernelGGL(ep_account_kernel, grid, block, 0, st, k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "ep_account_kernel launch");

    ScatterArgs s;
    s.term = term; s.finished = finished; s.ret = ret; s.len = len;
    s.N = N; s.chunk = sh.chunk; s.env_offset = env_offset; s.C = C;
    s.log_ret = log_ret; s.log_len = log_len; s.log_code = log_code; s.log_world = log_world;
    s.block_counts = k.block_counts; s.blocks = sh.blocks; s.counts = k.counts;
    s.eps_state = eps_state; s.eps_out = eps_out; s.decay = decay; s.eps_final = eps_final;
    hipLaunchKernelGGL(ep_scatter_kernel, grid, block, 0, st, s);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "ep_scatter_kernel launch");
    return 0;
}

int aquaep_explore_u8(uint8_t* action, int64_t N, int64_t env_offset, const float* eps_dev, uint64_t seed, uint64_t tick,
                      const uint64_t* tick_base_dev, void* stream)
{
    if (N < 0 || N > AQUAEP_MAX_WORLDS) return fail(AQUAEP_E_INVALID, "N=%lld: must be in [0, %d]", (long long)N, AQUAEP_MAX_WORLDS);
    if (env_offset < 0) return fail(AQUAEP_E_INVALID, "env_offset < 0");
    if (eps_dev == nullptr) return fail(AQUAEP_E_INVALID, "eps_dev is NULL");
    if (!aligned(eps_dev, 4)) return fail(AQUAEP_E_ALIGN, "eps_dev must be 4-byte aligned");
    if (!aligned(tick_base_dev, 8)) return fail(AQUAEP_E_ALIGN, "tick_base_dev must be 8-byte aligned");
    if (N == 0) return 0;
    if (action == nullptr) return fail(AQUAEP_E_INVALID, "action is NULL");

    int64_t blocks = (N + BLOCK - 1) / BLOCK;
    if (blocks > EXPLORE_MAX_BLOCKS) blocks = EXPLORE_MAX_BLOCKS;
    ExploreArgs x;
    x.action = action; x.N = N; x.env_offset = env_offset; x.eps = eps_dev; x.seed = seed; x.tick = tick; x.tick_base = tick_base_dev;
    hipLaunchKernelGGL(ep_explore_kernel, dim3(static_cast<unsigned>(blocks)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), x);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "ep_explore_kernel launch");
    return 0;
}

}  // extern "C"
