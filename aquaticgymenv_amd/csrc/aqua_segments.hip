// aqua_segments.hip -- libaqua_segments.so (include/aqua_segments.h): per-segment episode counters, epsilon schedules and a
// window of the last W episodes (mean return, mean length, success rate) for the segments of a batch of worlds on gfx950,
// fed by the episode log of libaqua_episodes.so.  Its own translation unit and library.
//
// One launch, one wavefront per segment.  The records one accounting call appends ascend in world index, so
// a segment's new records are one run of the new range: two searches over the record index find it, 64 probes a round.
// A wavefront with an empty run leaves after its searches.  No block waits on another block: `seen` is read by every
// block before it takes a ticket, and written by the block that takes the last one.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include "../../include/aqua_segments.h"
#include "aqua_host.hpp"

namespace {

constexpr int BLOCK = 256, WAVES = BLOCK / 64;

struct SegArgs {
    const float* log_ret;
    const int32_t* log_len;
    const uint8_t* log_code;
    const int64_t* log_world;
    uint64_t C;
    const unsigned long long* counts;
    int64_t env_offset, seg;
    uint64_t N;
    int P, W;
    unsigned long long* header;
    unsigned long long* seg_counts;
    const double* hyper;
    double* eps_state;
    float* eps_out;
    float* win_ret;
    int32_t* win_len;
    uint8_t* win_code;
    float* mean_ret;
    float* mean_len;
    float* success;
};

__device__ __forceinline__ uint32_t popc64(uint64_t m) { return static_cast<uint32_t>(__builtin_popcountll(m)); }

__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(static_cast<unsigned long long>(v), d);
    return v;
}

// the value lane `l` holds (l wave-uniform), to every lane
__device__ __forceinline__ double from_lane(double v, int l)
{
    const uint64_t bits = static_cast<uint64_t>(__double_as_longlong(v));
    const uint32_t lo = __builtin_amdgcn_readlane(static_cast<uint32_t>(bits), l);
    const uint32_t hi = __builtin_amdgcn_readlane(static_cast<uint32_t>(bits >> 32), l);
    return __longlong_as_double(static_cast<long long>((static_cast<uint64_t>(hi) << 32) | lo));
}

// The schedule of ep_scatter_kernel (aqua_episodes.hip), RESTATED: max(*eps_state * decay^count, eps_final), decay^count in
// float64 by binary exponentiation, least-significant bit first.  Moved into a header that both sources include, the
// episodes library compiles to a listing that differs from its own in a compare and a branch sense, and that library is
// to stay instruction for instruction what it was; tests/test_segments_gpu.py holds the two to the same bits.
__device__ __forceinline__ double schedule_advance(const double* eps_state, double decay, double eps_final, uint32_t count)
{
    double result = 1.0, base = decay;
    for (uint32_t n = count; n != 0; n >>= 1) {
        if (n & 1u) result *= base;
        base *= base;
    }
    double e = *eps_state * result;
    e = e > eps_final ? e : eps_final;
    return e;
}

// log slot of new record k: base < C and k < n <= N <= C, so base + k < 2 C
__device__ __forceinline__ uint64_t slot_of(uint64_t base, uint64_t k, uint64_t C)
{
    const uint64_t s = base + k;
    return s >= C ? s - C : s;
}

// A search for the smallest k in [0, n] such that every new record below it has a world < key; wave-uniform.  Each round probes 64
// evenly spaced records of [lo, hi) and keeps the gap the answer lies in.  Every index stays inside [0, n) whatever the
// log holds, so an unordered range (a caller that broke the contract) gives a wrong run, never a wild read.
struct Search {
    uint32_t lo, hi;                                                   // the answer lies in [lo, hi]; lo == hi: found
    int64_t key;
};

// this lane's probe of a search's round: record lo + lane * step, or none
__device__ __forceinline__ bool probe(const SegArgs& a, uint64_t base, const Search& s, int lane)
{
    const uint32_t step = (s.hi - s.lo + 63u) / 64u;
    const uint64_t k = static_cast<uint64_t>(s.lo) + static_cast<uint64_t>(lane) * step;
    return k < s.hi && a.log_world[slot_of(base, k, a.C)] < s.key;
}

// c of the 64 probes lie below the key: the answer is behind probe c - 1 and not behind probe c
__device__ __forceinline__ void narrow(Search& s, uint32_t c)
{
    const uint32_t step = (s.hi - s.lo + 63u) / 64u;
    if (c == 0) { s.hi = s.lo; return; }
    if (step == 1) { s.lo += c; s.hi = s.lo; return; }
    const uint32_t upper = s.lo + c * step;                            // (c <= ceil(len / step): (c - 1) step < len)
    s.lo = s.lo + (c - 1) * step + 1;
    s.hi = upper < s.hi ? upper : s.hi;
}

// both ends of the run in lockstep, so that the two loads of a round are in flight together
__device__ __forceinline__ void lower_bounds(const SegArgs& a, uint64_t base, Search& s0, Search& s1, int lane)
{
    while (s0.lo < s0.hi || s1.lo < s1.hi) {
        const bool b0 = s0.lo < s0.hi && probe(a, base, s0, lane);
        const bool b1 = s1.lo < s1.hi && probe(a, base, s1, lane);
        const uint32_t c0 = popc64(__builtin_amdgcn_ballot_w64(b0)), c1 = popc64(__builtin_amdgcn_ballot_w64(b1));
        if (s0.lo < s0.hi) narrow(s0, c0);
        if (s1.lo < s1.hi) narrow(s1, c1);
    }
}

__global__ __launch_bounds__(BLOCK) void seg_account_kernel(const SegArgs a)
{
#pragma clang fp contract(off)
    __shared__ uint64_t s_base;
    __shared__ uint32_t s_n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    // the cursor pair, once per block.  n == 0: nothing new; n > N: the caller skipped calls (s_n = 0 as well)
    bool missed = false;
    unsigned long long cursor = 0;
    if (threadIdx.x == 0) {
        const unsigned long long seen = a.header[0];
        cursor = a.counts[0];
        const unsigned long long n = cursor - seen;
        missed = n > a.N;
        s_n = missed ? 0u : static_cast<uint32_t>(n);
        s_base = seen % a.C;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // This block has read `seen` (its value went into LDS in front of the barrier).  The last ticket means every block
        // has: only then is it written, by this thread alone.  Nothing of this launch reads what is written here.
        const unsigned long long ticket = atomicAdd(&a.header[3], 1ull);
        if (ticket == gridDim.x - 1) {
            atomicExch(&a.header[3], 0ull);
            a.header[0] = cursor;
            if (missed) a.header[1] = a.header[1] + 1;
        }
    }
    const uint32_t n = s_n;
    const uint64_t base = s_base;
    const int p = static_cast<int>(blockIdx.x) * WAVES + wave;
    if (n == 0 || p >= a.P) return;

    // the run [first, last) of this segment's records
    const int64_t key0 = a.env_offset + static_cast<int64_t>(p) * a.seg, key1 = key0 + a.seg;
    uint32_t first, last;
    if (n <= 64) {                                                     // one probe round serves both searches
        int64_t world = INT64_MAX;
        if (static_cast<uint32_t>(lane) < n) world = a.log_world[slot_of(base, static_cast<uint64_t>(lane), a.C)];
        first = popc64(__builtin_amdgcn_ballot_w64(world < key0));
        last = popc64(__builtin_amdgcn_ballot_w64(world < key1));
    } else {
        Search s0 = {0u, n, key0}, s1 = {0u, n, key1};
        lower_bounds(a, base, s0, s1, lane);
        first = s0.lo;
        last = s1.lo;
    }
    if (last < first) last = first;                                    // (an unordered range only)
    // records below the first segment and above the last one belong to no segment
    if (lane == 0) {
        const uint32_t stray = (p == 0 ? first : 0u) + (p == a.P - 1 ? n - last : 0u);
        if (stray != 0) atomicAdd(&a.header[2], static_cast<unsigned long long>(stray));
    }
    const uint32_t m = last - first;
    if (m == 0) return;

    const uint32_t W = static_cast<uint32_t>(a.W);
    unsigned long long* counts = a.seg_counts + static_cast<size_t>(p) * AQUASEG_COUNTS;
    const unsigned long long c = counts[0];
    const uint32_t c0 = static_cast<uint32_t>(c % W);
    float* win_ret = a.win_ret + static_cast<size_t>(p) * W;
    int32_t* win_len = a.win_len + static_cast<size_t>(p) * W;
    uint8_t* win_code = a.win_code + static_cast<size_t>(p) * W;

    // the run, 64 records per trip: counters, and the last W records into the window
    uint32_t n1 = 0, n2 = 0, n3 = 0;                                   // wave-uniform
    uint64_t steps = 0;
    const uint32_t keep_from = m > W ? m - W : 0u;
    for (uint32_t j0 = 0; j0 < m; j0 += 64) {
        const uint32_t j = j0 + static_cast<uint32_t>(lane);
        const bool valid = j < m;
        uint32_t code = 0;
        uint64_t len = 0;
        if (valid) {
            const uint64_t s = slot_of(base, static_cast<uint64_t>(first) + j, a.C);
            code = a.log_code[s];
            const int32_t l = a.log_len[s];
            len = static_cast<uint64_t>(static_cast<int64_t>(l));
            if (j >= keep_from) {
                const uint32_t w = (c0 + j) % W;
                win_ret[w] = a.log_ret[s];
                win_len[w] = l;
                win_code[w] = static_cast<uint8_t>(code);
            }
        }
        n1 += popc64(__builtin_amdgcn_ballot_w64(valid && code == 1));
        n2 += popc64(__builtin_amdgcn_ballot_w64(valid && code == 2));
        n3 += popc64(__builtin_amdgcn_ballot_w64(valid && code == 3));
        steps += wave_sum(len);
    }
    if (lane == 0) {
        counts[0] = c + m;
        if (n1 != 0) counts[1] = counts[1] + n1;
        if (n2 != 0) counts[2] = counts[2] + n2;
        if (n3 != 0) counts[3] = counts[3] + n3;
        counts[4] = counts[4] + steps;
        if (a.eps_state != nullptr) {
            const double e = schedule_advance(a.eps_state + p, a.hyper[2 * p], a.hyper[2 * p + 1], m);
            a.eps_state[p] = e;
            a.eps_out[p] = static_cast<float>(e);
        }
    }

    // The statistics of the window as it is after this call.  Slot w was written in this call iff its distance d back
    // from the newest slot is below min(m, W); its value is then that of record m - 1 - d, read from the LOG: no load here
    // depends on a store of this launch.  Every other occupied slot still holds an earlier call's record.
    const unsigned long long filled = c + m;
    const uint32_t k = filled < W ? static_cast<uint32_t>(filled) : W;
    const uint32_t fresh = m < W ? m : W;
    const uint32_t newest = (c0 + (m - 1) % W) % W;
    double sum = 0.0;
    uint64_t len_sum = 0;
    uint32_t won = 0;
    for (uint32_t w = static_cast<uint32_t>(lane); w < k; w += 64) {
        const uint32_t d = newest >= w ? newest - w : newest + W - w;
        float r;
        int32_t l;
        uint32_t code;
        if (d < fresh) {
            const uint64_t s = slot_of(base, static_cast<uint64_t>(first) + (m - 1 - d), a.C);
            r = a.log_ret[s]; l = a.log_len[s]; code = a.log_code[s];
        } else {
            r = win_ret[w]; l = win_len[w]; code = win_code[w];
        }
        sum += static_cast<double>(r);
        len_sum += static_cast<uint64_t>(static_cast<int64_t>(l));
        won += code == 3 ? 1u : 0u;
    }
    double total = 0.0;
#pragma unroll 4                                                       // (fully unrolled, the 128 lane reads are hoisted into SGPRs that spill)
    for (int l = 0; l < 64; ++l) total += from_lane(sum, l);           // ascending lane order
    len_sum = wave_sum(len_sum);
    const uint64_t wins = wave_sum(static_cast<uint64_t>(won));
    if (lane == 0) {
        const double dk = static_cast<double>(k);
        a.mean_ret[p] = static_cast<float>(total / dk);
        a.mean_len[p] = static_cast<float>(static_cast<double>(len_sum) / dk);
        a.success[p] = static_cast<float>(static_cast<double>(wins) / dk);
    }
}

}  // namespace

extern "C" {

int aquaseg_version(void) { return AQUASEG_ABI_VERSION; }
const char* aquaseg_last_error(void) { return g_err; }

int aquaseg_account(const float* log_ret, const int32_t* log_len, const uint8_t* log_code, const int64_t* log_world, int64_t C,
                    const uint64_t* counts, int64_t env_offset, int64_t N, int64_t seg, int64_t P, int64_t W,
                    uint64_t* header, uint64_t* seg_counts, const double* hyper, double* eps_state, float* eps_out,
                    float* win_ret, int32_t* win_len, uint8_t* win_code, float* mean_ret, float* mean_len, float* success,
                    void* stream)
{
    if (log_ret == nullptr || log_len == nullptr || log_code == nullptr || log_world == nullptr || counts == nullptr)
        return fail(AQUASEG_E_INVALID, "log_ret, log_len, log_code, log_world or counts is NULL");
    if (header == nullptr || seg_counts == nullptr) return fail(AQUASEG_E_INVALID, "header or seg_counts is NULL");
    if (win_ret == nullptr || win_len == nullptr || win_code == nullptr) return fail(AQUASEG_E_INVALID, "win_ret, win_len or win_code is NULL");
    if (mean_ret == nullptr || mean_len == nullptr || success == nullptr) return fail(AQUASEG_E_INVALID, "mean_ret, mean_len or success is NULL");
    if (N < 0 || N > AQUASEG_MAX_WORLDS) return fail(AQUASEG_E_INVALID, "N=%lld: must be in [0, %d]", (long long)N, AQUASEG_MAX_WORLDS);
    if (C < 1 || C < N) return fail(AQUASEG_E_INVALID, "C=%lld: the log holds at least one record and one batched step (N=%lld)", (long long)C, (long long)N);
    if (env_offset < 0) return fail(AQUASEG_E_INVALID, "env_offset < 0");
    if (seg < 1 || seg > AQUASEG_MAX_WORLDS) return fail(AQUASEG_E_INVALID, "seg=%lld: must be in [1, %d]", (long long)seg, AQUASEG_MAX_WORLDS);
    if (P < 0 || P > AQUASEG_MAX_SEGMENTS) return fail(AQUASEG_E_INVALID, "P=%lld: must be in [0, %d]", (long long)P, AQUASEG_MAX_SEGMENTS);
    if (W < 1 || W > AQUASEG_MAX_WINDOW) return fail(AQUASEG_E_INVALID, "W=%lld: must be in [1, %d]", (long long)W, AQUASEG_MAX_WINDOW);
    if ((eps_state == nullptr) != (eps_out == nullptr))
        return fail(AQUASEG_E_INVALID, "eps_state and eps_out: give both, or neither to switch the schedule off");
    if (eps_state != nullptr && hyper == nullptr) return fail(AQUASEG_E_INVALID, "hyper is NULL with the schedule on");
    if (!aligned(log_ret, 4) || !aligned(log_len, 4) || !aligned(log_world, 8))
        return fail(AQUASEG_E_ALIGN, "log_ret / log_len must be 4-byte, log_world 8-byte aligned");
    if (!aligned(counts, 8) || !aligned(header, 8) || !aligned(seg_counts, 8))
        return fail(AQUASEG_E_ALIGN, "counts / header / seg_counts must be 8-byte aligned");
    if (!aligned(hyper, 8) || !aligned(eps_state, 8) || !aligned(eps_out, 4))
        return fail(AQUASEG_E_ALIGN, "hyper / eps_state must be 8-byte, eps_out 4-byte aligned");
    if (!aligned(win_ret, 4) || !aligned(win_len, 4) || !aligned(mean_ret, 4) || !aligned(mean_len, 4) || !aligned(success, 4))
        return fail(AQUASEG_E_ALIGN, "win_ret / win_len / mean_ret / mean_len / success must be 4-byte aligned");
    if (N == 0 || P == 0) return 0;

    SegArgs k;
    k.log_ret = log_ret; k.log_len = log_len; k.log_code = log_code; k.log_world = log_world;
    k.C = static_cast<uint64_t>(C);
    k.counts = reinterpret_cast<const unsigned long long*>(counts);
    k.env_offset = env_offset; k.seg = seg; k.N = static_cast<uint64_t>(N);
    k.P = static_cast<int>(P); k.W = static_cast<int>(W);
    k.header = reinterpret_cast<unsigned long long*>(header);
    k.seg_counts = reinterpret_cast<unsigned long long*>(seg_counts);
    k.hyper = hyper; k.eps_state = eps_state; k.eps_out = eps_out;
    k.win_ret = win_ret; k.win_len = win_len; k.win_code = win_code;
    k.mean_ret = mean_ret; k.mean_len = mean_len; k.success = success;
    const unsigned blocks = static_cast<unsigned>((P + WAVES - 1) / WAVES);
    hipLaunchKernelGGL(seg_account_kernel, dim3(blocks), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), k);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "seg_account_kernel launch");
    return 0;
}

}  // extern "C"
