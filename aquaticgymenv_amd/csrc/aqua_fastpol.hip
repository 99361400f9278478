// aqua_fastpol.hip -- libaqua_fastpol.so (aqua_fastpol.h): the acting pass of the DQN's 5 -> 64 -> 64 -> 3 Q-network
// (main/impl/dqn.py:301-314) with its two hidden layers on v_mfma_f32_32x32x16_f16, every operand split into a high and
// a low f16 part.  Its own translation unit and library: libaqua_policy.so and libaqua_bank.so, whose
// float32 pass it stands in for, are not touched by it; the float32 blob they act with stays the source of the weights,
// and aquafast_refresh re-splits it on the device.
//
// Shared with them (aqua_qnet.hpp): the blob's index map, the LDS part's layout, unit_of, the pick with its stores, the
// device query.  The skeleton is the bank kernel's: the unit of work is the item (network p, tile j of p's segment), a
// wavefront takes a contiguous run of items and reloads its weights only where the network changes inside the run.
//
// Layout.  v_mfma_f32_32x32x16_f16 computes D[i][j] += sum_k A[i][k] B[k][j], k = 0 .. 15: lane l (r = l & 31, h = l >> 5)
// holds A[i = r][k = 8 h + e] and B[k = 8 h + e][j = r] in element e of its 8-element fragment, and D as the float32 form
// does.  WORLDS sit on j, UNITS on i.  Registers 8 t .. 8 t + 7 of row block M of a layer's accumulators, converted
// pairwise, are the B fragment of k-step s = 2 M + t of the next layer: element e of lane half h is unit
// unit_of(M, 8 t + e, h) = 16 s + 8 (e >> 2) + 4 h + (e & 3), and aquafast_map() puts the weight of that unit into element e of
// the A fragment.  Layer 1 is one k-step: element e < 3 of lane half h is input 2 e + h (what a lane loads today), the
// other elements are zero on both sides.
#include <hip/hip_runtime.h>

#include <cmath>

#include "aqua_fastpol.h"
#include "aqua_device.hpp"
#include "aqua_host.hpp"
#include "aqua_qnet.hpp"

namespace aqua_fast {

using namespace aqua::qnet;

static_assert(STREAM_POLICY == AQUAFAST_STREAM, "aqua_fastpol.h names the stream of the policy draws");
static_assert(IN == AQUAFAST_INPUTS && HID == AQUAFAST_HIDDEN && ACT == AQUAFAST_ACTIONS, "aqua_fastpol.h names the network's sizes");
constexpr int BLOCK = 256, WAVES = BLOCK / 64;
#ifndef AQUA_FAST_WAVES_PER_SIMD
#define AQUA_FAST_WAVES_PER_SIMD 2       // (a tuning build, -DAQUA_FAST_TUNING, may say 1 or 3; tools/fastpol_bench.py times it through AQUA_FASTPOL_LIB)
#endif
// resident wavefronts per SIMD = blocks per CU.  Two: the kernel needs about 230 registers (80 of A fragments, 128 of
// accumulators), which fits 256 and not the 170 of three -- that build spills and measured 30.4 us at 262 144 worlds --
// and two measured 12.8 us against 17.5 for one: while one wavefront splits activations on the VALU the
// other keeps the matrix pipe busy.
constexpr int WAVES_PER_SIMD = AQUA_FAST_WAVES_PER_SIMD;
#ifndef AQUA_FAST_TUNING
static_assert(WAVES_PER_SIMD == 2, "another occupancy is a tuning build (-DAQUA_FAST_TUNING): three wavefronts per SIMD spill to scratch");
#endif

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ---- the fast blob, in 16-bit elements
constexpr int FRAG = 64 * 8;                               // one A fragment of the wavefront: 8 elements per lane
constexpr int K2S = HID / 16;                              // layer 2: 4 k-steps of 16
constexpr int F_W1 = 0;                                    // [2 row blocks][hi, lo][64 lanes][8]
constexpr int F_W2 = F_W1 + 2 * 2 * FRAG;                  // [2 row blocks][K2S][hi, lo][64 lanes][8]
constexpr int F_LDS = F_W2 + 2 * K2S * 2 * FRAG;           // the LDS part of the float32 blob, as it is
constexpr int FAST_ELEMS = F_LDS + 2 * LDS_FLOATS;
static_assert(F_LDS % 8 == 0 && FAST_ELEMS % 8 == 0, "fragments and the LDS part are read 16 bytes at a time and every slot stays 16-byte aligned");

constexpr float CLAMP = 65504.0f;                          // the largest f16
constexpr float LO_SCALE = 2048.0f, LO_UNSCALE = 1.0f / 2048.0f;
constexpr uint16_t F16_NAN = 0x7E00u;                      // both parts of a NaN weight, on the host and on the device

// ---- the split on the device: c is clamped by the caller
__device__ __forceinline__ void split(float c, _Float16& hi, _Float16& lo)
{
#pragma clang fp contract(off)
    hi = static_cast<_Float16>(c);                                               // round to nearest even
    lo = static_cast<_Float16>((c - static_cast<float>(hi)) * LO_SCALE);         // both operations exact
}

struct FastArgs {
    const uint16_t* bank;
    const float* in;
    const float* epsilon_dev;
    int64_t seg, tiles;                  // worlds per network, tiles per network
    int64_t share, rem;                  // items / wavefronts of the grid and the remainder: the first `rem` wavefronts take one more
    int64_t ld, N, env_offset, q_ld;
    float epsilon;
    uint64_t seed, tick;
    const uint64_t* tick_base;
    uint8_t* action;
    float* q;
    float* q_taken;
};

// (see aqua_bank.hip) the wavefront's own LDS traffic is complete before anything behind this point
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

// the hidden units of two accumulator pairs -> the B fragments (hi, lo) of k-step 2 M + t of the next layer
__device__ __forceinline__ void activate(const f32x16& hi, const f32x16& lo, int t, f16x8& bhi, f16x8& blo)
{
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        // ReLU and the clamp in one med3; the unit is one fused multiply-add of the two accumulators
        const float c = __builtin_amdgcn_fmed3f(fmaf(lo[8 * t + e], LO_UNSCALE, hi[8 * t + e]), 0.0f, CLAMP);
        _Float16 a, b;
        split(c, a, b);
        bhi[e] = a;
        blo[e] = b;
    }
}

// One tile of 32 worlds through the network.  lds4: the LDS part as the wavefront sees it; w1 / w2: the A fragments
// [row block][..][hi, lo]; in[e]: input 2 e + h of the lane's world (0 where there is none); q: the three Q-values of
// the lane's world, the same bits on both halves.
template <bool RAW>
__device__ __forceinline__ void forward_f16(const float4* lds4, const f16x8 (&w1)[2][2], const f16x8 (&w2)[2][K2S][2],
                                            const float (&in)[K1_STEPS], int h, float (&q)[ACT])
{
#pragma clang fp contract(off)
    const float* const lds = reinterpret_cast<const float*>(lds4);
    f16x8 xhi = {0, 0, 0, 0, 0, 0, 0, 0}, xlo = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < K1_STEPS; ++e) {
        float x = in[e];
        // AquaStateNormalizer as the step kernels' epilogue writes it (aqua_qnet.hpp forward<RAW>), before the split
        if constexpr (RAW) x = (2 * e + h == 2) ? fmaf(x, 0.15915494309189535f, 0.5f) : x * 0.01f;
        _Float16 a, b;
        split(__builtin_amdgcn_fmed3f(x, -CLAMP, CLAMP), a, b);
        xhi[e] = a;
        xlo[e] = b;
    }
    __builtin_amdgcn_sched_barrier(0);

    // layer 1: the hi accumulators start at the bias, the lo accumulators at zero
    f32x16 ahi[2], alo[2];
#pragma unroll
    for (int M = 0; M < 2; ++M)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 b0 = lds4[(LDS_B0 + h * 32 + M * 16) / 4 + g];
            ahi[M][4 * g + 0] = b0.x; ahi[M][4 * g + 1] = b0.y; ahi[M][4 * g + 2] = b0.z; ahi[M][4 * g + 3] = b0.w;
            alo[M][4 * g + 0] = 0.0f; alo[M][4 * g + 1] = 0.0f; alo[M][4 * g + 2] = 0.0f; alo[M][4 * g + 3] = 0.0f;
        }
#pragma unroll
    for (int M = 0; M < 2; ++M) {
        ahi[M] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1[M][0], xhi, ahi[M], 0, 0, 0);
        alo[M] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1[M][0], xlo, alo[M], 0, 0, 0);
        alo[M] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1[M][1], xhi, alo[M], 0, 0, 0);
    }

    __builtin_amdgcn_sched_barrier(0);
    // layer 2: k-step s = 2 M + t takes registers 8 t .. 8 t + 7 of row block M
    f32x16 chi[2], clo[2];
#pragma unroll
    for (int M = 0; M < 2; ++M)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 b1 = lds4[(LDS_B1 + h * 32 + M * 16) / 4 + g];
            chi[M][4 * g + 0] = b1.x; chi[M][4 * g + 1] = b1.y; chi[M][4 * g + 2] = b1.z; chi[M][4 * g + 3] = b1.w;
            clo[M][4 * g + 0] = 0.0f; clo[M][4 * g + 1] = 0.0f; clo[M][4 * g + 2] = 0.0f; clo[M][4 * g + 3] = 0.0f;
        }
#pragma unroll
    for (int s = 0; s < K2S; ++s) {
        f16x8 bhi, blo;
        activate(ahi[s >> 1], alo[s >> 1], s & 1, bhi, blo);
#pragma unroll
        for (int M2 = 0; M2 < 2; ++M2) {
            chi[M2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w2[M2][s][0], bhi, chi[M2], 0, 0, 0);
            clo[M2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w2[M2][s][0], blo, clo[M2], 0, 0, 0);
            clo[M2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w2[M2][s][1], bhi, clo[M2], 0, 0, 0);
        }
    }

    __builtin_amdgcn_sched_barrier(0);
    // layer 3: that of aqua_qnet.hpp's forward, on the units this lane holds
    float p[ACT];
#pragma unroll
    for (int c = 0; c < ACT; ++c) p[c] = h == 0 ? lds[LDS_B2 + c] : 0.0f;
#pragma unroll
    for (int M = 0; M < 2; ++M)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(fmaf(clo[M][4 * g + e], LO_UNSCALE, chi[M][4 * g + e]), 0.0f);
#pragma unroll
            for (int c = 0; c < ACT; ++c) {
                const float4 k = lds4[(LDS_K2 + (h * ACT + c) * 32 + M * 16) / 4 + g];
                p[c] = fmaf(k.x, v[0], p[c]);
                p[c] = fmaf(k.y, v[1], p[c]);
                p[c] = fmaf(k.z, v[2], p[c]);
                p[c] = fmaf(k.w, v[3], p[c]);
            }
        }
#pragma unroll
    for (int c = 0; c < ACT; ++c) q[c] = p[c] + __shfl_xor(p[c], 32);      // the same bits on both halves
}

// RAW: `in` holds the environment's state rows and is normalised here; EPS: epsilon-greedy (one Philox draw per world)
template <bool RAW, bool EPS>
__global__ __launch_bounds__(BLOCK, WAVES_PER_SIMD) void qfast_kernel(const FastArgs a)
{
    // a copy of the LDS part per wavefront: the network is a property of the wavefront's item, not of the block
    __shared__ float4 lds_all[WAVES][LDS_FLOATS / 4];

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, col = lane & 31;
    float4* const lds4 = lds_all[wave];

    uint64_t tick = a.tick;
    if constexpr (EPS) {
        if (a.tick_base != nullptr) tick += *a.tick_base;
    }

    // this wavefront's contiguous run of items
    const int64_t w = static_cast<int64_t>(blockIdx.x) * WAVES + wave;
    const int64_t first = w * a.share + (w < a.rem ? w : a.rem), count = a.share + (w < a.rem ? 1 : 0);
    if (count == 0) return;
    int64_t p = uniform(first / a.tiles), j = uniform(first % a.tiles);

    // the A fragments stay in registers while the network stays (80 VGPRs)
    f16x8 w1[2][2], w2[2][K2S][2];
    float eps = a.epsilon;
    int64_t loaded = -1;

    for (int64_t n = 0; n < count; ++n, ++j) {
        if (j == a.tiles) { j = 0; ++p; }
        const int64_t s = j * TILE + col;                     // the lane's world within the segment
        const int64_t i = p * a.seg + s;                      // ... and within the batch (the host counts live tiles only: < N + TILE)
        const bool live = s < a.seg && i < a.N;

        if (p != loaded) {
            loaded = p;
            const uint16_t* const blob = a.bank + p * FAST_ELEMS;
            const f16x8* const frags = reinterpret_cast<const f16x8*>(blob) + lane;
#pragma unroll
            for (int M = 0; M < 2; ++M)
#pragma unroll
                for (int part = 0; part < 2; ++part) w1[M][part] = frags[(F_W1 / FRAG + M * 2 + part) * 64];
#pragma unroll
            for (int M = 0; M < 2; ++M)
#pragma unroll
                for (int st = 0; st < K2S; ++st)
#pragma unroll
                    for (int part = 0; part < 2; ++part) w2[M][st][part] = frags[(F_W2 / FRAG + (M * K2S + st) * 2 + part) * 64];
            const float4* const blob4 = reinterpret_cast<const float4*>(blob + F_LDS);
            wave_sync_lds();                                  // the reads of the previous network's copy are done
            static_assert(LDS_FLOATS / 4 > 64 && LDS_FLOATS / 4 <= 128, "two float4 per lane cover the LDS part");
            lds4[lane] = blob4[lane];
            if (lane < LDS_FLOATS / 4 - 64) lds4[64 + lane] = blob4[64 + lane];
            wave_sync_lds();                                  // the copy is complete before any lane reads it
            if constexpr (EPS) {
                if (a.epsilon_dev != nullptr) {
                    // by its bits (the library is built with -fno-honor-nans): NaN, and every negative value, never explore
                    const uint32_t bits = __float_as_uint(a.epsilon_dev[p]);
                    eps = bits > 0x7F800000u ? 0.0f : __uint_as_float(bits);
                }
            }
        }

        // element e of layer 1's fragment takes input 2 e + h of the lane's world; dead worlds and the padding are zero
        float x[K1_STEPS];
        const float* const xin = a.in + (h != 0 ? a.ld : 0) + i;
#pragma unroll
        for (int e = 0; e < K1_STEPS; ++e) x[e] = (live && 2 * e + h < IN) ? xin[2 * e * a.ld] : 0.0f;
        float q[ACT];
        forward_f16<RAW>(lds4, w1, w2, x, h, q);
        if (h == 0 && live)
            pick_and_store<EPS>(q[0], q[1], q[2], eps, a.seed, static_cast<uint64_t>(a.env_offset + i), tick, i, a.action, a.q, a.q_ld, a.q_taken);
    }
}

// ---- the refresh: one thread per pair of 16-bit elements, one 4-byte store
struct RefreshArgs {
    const char* blobs;
    int64_t stride;
    const int32_t* map;
    uint32_t* fast;
    int64_t total;                       // P * FAST_ELEMS / 2
};

__device__ __forceinline__ uint32_t element(const char* blob, int32_t m)
{
    if (m < 0 || (m >> 2) >= BLOB_FLOATS) return 0u;
    const float v = reinterpret_cast<const float*>(blob)[m >> 2];
    const int part = m & 3;
    if (part == AQUAFAST_PART_BITS0) return __float_as_uint(v) & 0xFFFFu;
    if (part == AQUAFAST_PART_BITS1) return __float_as_uint(v) >> 16;
    // a NaN weight by its bits (the library is built with -fno-honor-nans, and med3 would turn it into a number): both parts
    // are the quiet f16 NaN, as split_host() writes them
    if ((__float_as_uint(v) & 0x7FFFFFFFu) > 0x7F800000u) return F16_NAN;
    _Float16 hi, lo;
    split(__builtin_amdgcn_fmed3f(v, -CLAMP, CLAMP), hi, lo);
    const _Float16 r = part == AQUAFAST_PART_HI ? hi : lo;
    uint16_t bits;
    __builtin_memcpy(&bits, &r, sizeof(bits));
    return bits;
}

__global__ __launch_bounds__(BLOCK) void refresh_kernel(const RefreshArgs a)
{
    const int64_t stride = static_cast<int64_t>(gridDim.x) * BLOCK;
    for (int64_t t = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x; t < a.total; t += stride) {
        const int64_t p = t / (FAST_ELEMS / 2);
        const int e2 = static_cast<int>(t % (FAST_ELEMS / 2));
        const char* const blob = a.blobs + p * a.stride;
        a.fast[t] = element(blob, a.map[2 * e2]) | (element(blob, a.map[2 * e2 + 1]) << 16);
    }
}

// ------------------------------------------------------------------ host side
// (see aqua_bank.hip) the tiles that hold a world below N.  1 <= seg, 1 <= N <= networks * seg
static int64_t live_items(int64_t seg, int64_t N)
{
    const int64_t used = N / seg + (N % seg != 0 ? 1 : 0), tiles = seg / TILE + (seg % TILE != 0 ? 1 : 0);
    const int64_t n_last = N - (used - 1) * seg;
    return (used - 1) * tiles + n_last / TILE + (n_last % TILE != 0 ? 1 : 0);
}

// The map (aqua_fastpol.h), from the one statement of where a parameter lives in the float32 blob
static void build_map(int32_t* map)
{
    static int where0[IN * HID], where2[HID * HID];
    static bool parameter[BLOB_FLOATS];
    for (int b = 0; b < BLOB_FLOATS; ++b) parameter[b] = false;
    for_each_parameter([&](int b, int a, int i) {
        parameter[b] = true;
        if (a == 0) where0[i] = b;
        if (a == 2) where2[i] = b;
    });
    for (int e = 0; e < FAST_ELEMS; ++e) map[e] = -1;
    for (int lane = 0; lane < 64; ++lane) {
        const int h = lane >> 5, row = lane & 31;
        for (int part = 0; part < 2; ++part)
            for (int e = 0; e < 8; ++e) {
                for (int M = 0; M < 2; ++M) {
                    const int k = 2 * e + h;                              // input of this element and lane half
                    if (e < K1_STEPS && k < IN) map[F_W1 + ((M * 2 + part) * 64 + lane) * 8 + e] = 4 * where0[k * HID + 32 * M + row] + part;
                }
                for (int M2 = 0; M2 < 2; ++M2)                            // row block of the OUTPUT unit 32 M2 + row
                    for (int s = 0; s < K2S; ++s) {
                        const int u = unit_of(s >> 1, 8 * (s & 1) + e, h); // the input unit of this element: 16 s + 8 (e >> 2) + 4 h + (e & 3)
                        map[F_W2 + (((M2 * K2S + s) * 2 + part) * 64 + lane) * 8 + e] = 4 * where2[u * HID + 32 * M2 + row] + part;
                    }
            }
    }
    for (int f = 0; f < LDS_FLOATS; ++f)
        if (parameter[OFF_LDS + f]) {
            map[F_LDS + 2 * f] = 4 * (OFF_LDS + f) + AQUAFAST_PART_BITS0;
            map[F_LDS + 2 * f + 1] = 4 * (OFF_LDS + f) + AQUAFAST_PART_BITS1;
        }
}

// float32 -> f16 bits, round to nearest even, subnormal results kept (what v_cvt_f16_f32 gives with f16 denormals on)
static uint16_t f16_bits(float f)
{
    uint32_t x;
    std::memcpy(&x, &f, sizeof(x));
    const uint16_t sign = static_cast<uint16_t>((x >> 16) & 0x8000u);
    x &= 0x7FFFFFFFu;
    if (x > 0x7F800000u) return sign | 0x7E00u;                                  // NaN
    if (x >= 0x47800000u) return sign | 0x7C00u;                                 // 65536 and above (the callers clamp: not reached)
    if (x < 0x38800000u) {                                                       // below 2^-14: a multiple of 2^-24, rounded by the float add
        float a, half = 0.5f;
        std::memcpy(&a, &x, sizeof(a));
        volatile float m = a + half;
        const float mm = m;
        uint32_t mb;
        std::memcpy(&mb, &mm, sizeof(mb));
        return sign | static_cast<uint16_t>(mb - 0x3F000000u);
    }
    const uint32_t odd = (x >> 13) & 1u;
    x += 0xFFFu + odd;
    return sign | static_cast<uint16_t>((x - 0x38000000u) >> 13);                // a carry into the exponent rounds up to the next binade (or infinity)
}

static float f16_value(uint16_t b)
{
    const int e = (b >> 10) & 31, m = b & 1023;
    const float v = e == 0 ? std::ldexp(static_cast<float>(m), -24) : std::ldexp(static_cast<float>(m | 1024), e - 25);
    return (b & 0x8000u) ? -v : v;
}

static void split_host(float v, uint16_t& hi, uint16_t& lo)
{
    uint32_t bits;
    std::memcpy(&bits, &v, sizeof(bits));
    if ((bits & 0x7FFFFFFFu) > 0x7F800000u) { hi = lo = F16_NAN; return; }       // by its bits, as the refresh kernel does
    float c = v;
    if (c > CLAMP) c = CLAMP;
    if (c < -CLAMP) c = -CLAMP;
    hi = f16_bits(c);
    volatile float d = c - f16_value(hi);                                        // exact; volatile: no contraction with the product
    lo = f16_bits(d * LO_SCALE);
}

}  // namespace aqua_fast

using namespace aqua_fast;

extern "C" {

int aquafast_version(void) { return AQUAFAST_ABI_VERSION; }
const char* aquafast_last_error(void) { return g_err; }
size_t aquafast_weights_bytes(void) { return sizeof(uint16_t) * FAST_ELEMS; }

int aquafast_map(int32_t* map_host, size_t bytes)
{
    if (map_host == nullptr) return fail(AQUAFAST_E_INVALID, "map is NULL");
    if (bytes < sizeof(int32_t) * FAST_ELEMS) return fail(AQUAFAST_E_INVALID, "map too small: %zu < %zu bytes", bytes, sizeof(int32_t) * FAST_ELEMS);
    if (!aligned(map_host, 4)) return fail(AQUAFAST_E_ALIGN, "map must be 4-byte aligned");
    build_map(map_host);
    return 0;
}

int aquafast_pack_host(const void* blob_f32_host, void* fast_host, size_t bytes)
{
    if (blob_f32_host == nullptr) return fail(AQUAFAST_E_INVALID, "blob is NULL");
    if (fast_host == nullptr) return fail(AQUAFAST_E_INVALID, "fast blob is NULL");
    if (bytes < aquafast_weights_bytes()) return fail(AQUAFAST_E_INVALID, "fast blob too small: %zu < %zu bytes", bytes, aquafast_weights_bytes());
    if (!aligned(blob_f32_host, 4) || !aligned(fast_host, 4)) return fail(AQUAFAST_E_ALIGN, "blob and fast blob must be 4-byte aligned");
    static thread_local int32_t map[FAST_ELEMS];
    build_map(map);
    const float* const w = static_cast<const float*>(blob_f32_host);
    uint16_t* const out = static_cast<uint16_t*>(fast_host);
    for (int e = 0; e < FAST_ELEMS; ++e) {
        const int32_t m = map[e];
        if (m < 0) { out[e] = 0; continue; }
        const float v = w[m >> 2];
        uint32_t bits;
        std::memcpy(&bits, &v, sizeof(bits));
        uint16_t hi, lo;
        switch (m & 3) {
        case AQUAFAST_PART_BITS0: out[e] = static_cast<uint16_t>(bits & 0xFFFFu); break;
        case AQUAFAST_PART_BITS1: out[e] = static_cast<uint16_t>(bits >> 16); break;
        default: split_host(v, hi, lo); out[e] = (m & 3) == AQUAFAST_PART_HI ? hi : lo;
        }
    }
    return 0;
}

int aquafast_refresh(const void* blobs_f32_dev, int64_t stride_bytes, const int32_t* map_dev, void* fast_dev, int64_t P, void* stream)
{
    if (blobs_f32_dev == nullptr) return fail(AQUAFAST_E_INVALID, "the float32 blobs are NULL");
    if (map_dev == nullptr) return fail(AQUAFAST_E_INVALID, "the map is NULL");
    if (fast_dev == nullptr) return fail(AQUAFAST_E_INVALID, "the fast blobs are NULL");
    if (P < 1 || P > AQUAFAST_MAX_NETWORKS) return fail(AQUAFAST_E_INVALID, "P=%lld: must be in [1, %d]", (long long)P, AQUAFAST_MAX_NETWORKS);
    if (stride_bytes < static_cast<int64_t>(sizeof(float) * BLOB_FLOATS) || stride_bytes % 4 != 0 || stride_bytes > (int64_t(1) << 40))
        return fail(AQUAFAST_E_INVALID, "stride_bytes=%lld: must be a multiple of 4 in [%zu, 2^40]", (long long)stride_bytes, sizeof(float) * BLOB_FLOATS);
    if (!aligned(blobs_f32_dev, 16) || !aligned(fast_dev, 16)) return fail(AQUAFAST_E_ALIGN, "the blobs must be 16-byte aligned");
    if (!aligned(map_dev, 4)) return fail(AQUAFAST_E_ALIGN, "the map must be 4-byte aligned");

    int cus = 0;
    if (const int rc = compute_units(&cus, AQUAFAST_E_NODEVICE)) return rc;
    RefreshArgs a;
    a.blobs = static_cast<const char*>(blobs_f32_dev);
    a.stride = stride_bytes;
    a.map = map_dev;
    a.fast = static_cast<uint32_t*>(fast_dev);
    a.total = P * (FAST_ELEMS / 2);
    int64_t blocks = (a.total + BLOCK - 1) / BLOCK;
    if (blocks > 8 * static_cast<int64_t>(cus)) blocks = 8 * static_cast<int64_t>(cus);
    hipLaunchKernelGGL(refresh_kernel, dim3(static_cast<unsigned>(blocks)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "refresh_kernel launch");
    return 0;
}

int aquafast_act_f16(const void* fast_dev, int64_t networks, int64_t seg, const float* in, int64_t ld, int in_is_normalised,
                     int64_t N, int64_t env_offset, float epsilon, const float* epsilon_dev, uint64_t seed, uint64_t tick,
                     const uint64_t* tick_base_dev, uint8_t* action, float* q, int64_t q_ld, float* q_taken, void* stream)
{
    if (fast_dev == nullptr) return fail(AQUAFAST_E_INVALID, "the fast bank is NULL");
    if (!aligned(fast_dev, 16)) return fail(AQUAFAST_E_ALIGN, "the fast bank must be 16-byte aligned");
    if (networks < 1 || networks > AQUAFAST_MAX_NETWORKS)
        return fail(AQUAFAST_E_INVALID, "networks=%lld: must be in [1, %d]", (long long)networks, AQUAFAST_MAX_NETWORKS);
    if (seg < 1) return fail(AQUAFAST_E_INVALID, "seg=%lld: must be >= 1", (long long)seg);
    if (N < 0 || ld < N) return fail(AQUAFAST_E_INVALID, "bad sizes: N=%lld ld=%lld", (long long)N, (long long)ld);
    // N <= networks * seg without forming the product: the networks N needs, ceil(N / seg), are at most `networks`
    const int64_t used = N / seg + (N % seg != 0 ? 1 : 0);
    if (used > networks)
        return fail(AQUAFAST_E_INVALID, "N=%lld worlds: more than networks * seg = %lld * %lld", (long long)N, (long long)networks, (long long)seg);
    if (env_offset < 0) return fail(AQUAFAST_E_INVALID, "env_offset < 0");
    uint32_t eps_bits;                   // by its bits, as the kernel does: NaN or below zero (-0 is zero)
    std::memcpy(&eps_bits, &epsilon, sizeof(eps_bits));
    if (eps_bits > 0x7F800000u && eps_bits != 0x80000000u) return fail(AQUAFAST_E_INVALID, "epsilon=%g: must be >= 0", (double)epsilon);
    if (action == nullptr && q == nullptr && q_taken == nullptr) return fail(AQUAFAST_E_INVALID, "action, q and q_taken are all NULL");
    if (q != nullptr && q_ld < N) return fail(AQUAFAST_E_INVALID, "q_ld=%lld < N=%lld", (long long)q_ld, (long long)N);
    if (N > 0 && in == nullptr) return fail(AQUAFAST_E_INVALID, "in is NULL");
    if (!aligned(in, 4) || !aligned(q, 4) || !aligned(q_taken, 4)) return fail(AQUAFAST_E_ALIGN, "in / q / q_taken must be 4-byte aligned");
    if (!aligned(epsilon_dev, 4)) return fail(AQUAFAST_E_ALIGN, "epsilon_dev must be 4-byte aligned");
    if (!aligned(tick_base_dev, 8)) return fail(AQUAFAST_E_ALIGN, "tick_base_dev must be 8-byte aligned");
    if (N == 0) return 0;

    int cus = 0;
    if (const int rc = compute_units(&cus, AQUAFAST_E_NODEVICE)) return rc;
    FastArgs a;
    a.seg = seg;
    a.tiles = seg / TILE + (seg % TILE != 0 ? 1 : 0);
    const int64_t items = live_items(seg, N);
    int64_t blocks = (items + WAVES - 1) / WAVES;
    if (blocks > WAVES_PER_SIMD * static_cast<int64_t>(cus)) blocks = WAVES_PER_SIMD * static_cast<int64_t>(cus);     // all resident
    a.share = items / (blocks * WAVES);
    a.rem = items % (blocks * WAVES);

    a.bank = static_cast<const uint16_t*>(fast_dev);
    a.in = in; a.ld = ld; a.N = N; a.env_offset = env_offset; a.q_ld = q_ld;
    a.epsilon = epsilon; a.epsilon_dev = epsilon_dev; a.seed = seed; a.tick = tick; a.tick_base = tick_base_dev;
    a.action = action; a.q = q; a.q_taken = q_taken;
    const dim3 grid(static_cast<unsigned>(blocks)), block(BLOCK);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool raw = in_is_normalised == 0, eps = epsilon_dev != nullptr || epsilon > 0.0f;
    if (raw && eps) hipLaunchKernelGGL((qfast_kernel<true, true>), grid, block, 0, s, a);
    else if (raw) hipLaunchKernelGGL((qfast_kernel<true, false>), grid, block, 0, s, a);
    else if (eps) hipLaunchKernelGGL((qfast_kernel<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((qfast_kernel<false, false>), grid, block, 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "qfast_kernel launch");
    return 0;
}

}  // extern "C"
