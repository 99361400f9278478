// aqua_lrn.hpp -- the device side of the DQN update, stated once for libaqua_learner.so (one network per call) and
// libaqua_lbank.so (a bank of networks per call): the constants, the argument structs, the forward pass of the training
// step, the bodies of the gradient and the apply kernel as forced-inline device functions of (arguments, block index), the
// launch shape and the workspace layout.  The `__global__` wrappers, the entry points and their validation stay with the
// libraries (DESIGN.md sections 5.7 and 5.12).
//
// Gradient body.  The orientation is qpolicy_kernel's: v_mfma_f32_32x32x2_f32 computes
// D[i][j] += A[i][k] B[k][j], k = 0, 1, lane l holding A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31], D[i][j] in
// register r of lane l with j = l & 31, i = (r & 3) + 8 (r >> 2) + 4 (l >> 5).  One tile = 32 SAMPLES on the column index
// j, UNITS on the row index i, so an accumulator is the next layer's B operand register by register; the A operands are
// read straight from the canonical parameter vector (k1[u_h][32 M + i] is coalesced over i).
//   forward  : up to three of them per tile (target / online network on s', online network on s); the last one keeps
//              h1, h2 and Q in registers for the backward.  Layers 1 and 2 are float32 MFMA; layer 3, y and delta are
//              double on the VALU (k2 of both networks sits in LDS as doubles), rounded once, to delta.
//   dh2      : on the VALU from h2 and k2[.][a];  dh1 = k1 dh2: the same register-to-B trick with the untransposed
//              weight as A (read from an LDS copy of k1, its rows strided over the lanes).
//   weight gradients have K over the SAMPLES, the transposed layout: relu(h2), relu(h1), dh2 and dh1 go through LDS once
//   per tile as [unit][sample] and come back as A (or B) operands, two samples per k-step:
//       dk1[u1][u2]        += relu(h1)[u1][s] dh2[u2][s]      four 32 x 32 accumulators
//       db1[u2]            += dh2[u2][s] * 1                  B = a column of ones           (column 0)
//       dk2[u2][c]         += relu(h2)[u2][s] dq[s][c]        B = delta on the action taken   (columns 0..2)
//       dk0[k][u1], db0    += dh1[u1][s] (x[s][k] | 1)        B = the input and a one         (columns 0..5)
//   dk1's accumulators are persistent across the tiles of a wavefront; the other three start from zero in every tile and the
//   lanes of their few parameter columns add them to sums of their own in LDS (`small`).  db2, the loss (double) and the
//   number of valid samples are per-lane sums.
// Determinism: wavefront w of workgroup g takes tiles (g WAVES + w) tpw .. + tpw - 1 with tpw and the grid functions of B
// alone; a wavefront's tiles are added in order, the wavefronts of a workgroup in order through LDS, the workgroups'
// partials in order by the apply body.  No atomics on floats anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/aqua_learner.h"
#include "aqua_device.hpp"
#include "aqua_qnet.hpp"

namespace aqua {
namespace lrn {

using aqua::draw;
using namespace aqua::qnet;

static_assert(STREAM_LEARNER == AQUALRN_STREAM, "aqua_learner.h names the stream of the minibatch draws");

constexpr int OFF_K0 = 0, OFF_B0 = OFF_K0 + IN * HID, OFF_K1 = OFF_B0 + HID, OFF_B1 = OFF_K1 + HID * HID;
constexpr int OFF_K2 = OFF_B1 + HID, OFF_B2 = OFF_K2 + HID * ACT, PARAMS = OFF_B2 + ACT;
static_assert(PARAMS == AQUALRN_PARAMS, "canonical Keras order: k0, b0, k1, b1, k2, b2");

constexpr int WAVES = 2, BLOCK = 64 * WAVES;
constexpr int GMAX = 512;                // workgroups (= partial gradients) at most
constexpr int STR = TILE + 1;            // [unit][sample] staging rows, padded: conflict-free writes and reads
constexpr int K1T_STR = HID + 1;         // the LDS copy of k1, rows padded: conflict-free reads down a column
constexpr int ATTEMPTS = 4;
// The accumulator tiles of dk0 | db0, dk2 and db1 hold parameters in 6, 3 and 1 of their 32 columns.  They start from zero
// in every tile, and the lanes of those columns add them to sums of their own in LDS: 96 registers that need not live
// across the tile.  A lane's slot: column (+ 6, 3 or 1 on the upper lane half) behind the base of its kind.
constexpr int SLOT_K0 = 0, SLOT_K2 = 2 * (IN + 1), SLOT_B1 = SLOT_K2 + 2 * ACT, SMALL_SLOTS = SLOT_B1 + 2;

// workspace: a 16-byte header (uint64 t + 1) and, per workgroup, PARAMS partial sums, the number n of squares in the loss
// (int32 bits: the valid samples, times 3 with AQUALRN_LOSS_REFERENCE, so that the apply kernel's 2 / n and sum / n are
// 2 / (3 B_eff) and sum / (3 B_eff) and that kernel does not know the form) and the partial loss (the squares of the
// unrounded delta -- of the three differences Q_a - T_j with the flag -- summed in double: one number, so its own rounding
// should not show)
constexpr int WS_HEADER = 16;
constexpr int WS_COUNT = PARAMS, WS_LOSS = PARAMS + 1, WS_USED = PARAMS + 3, WS_STRIDE = 4744;   // the loss: a double in two slots
static_assert(WS_USED <= WS_STRIDE && WS_STRIDE % 4 == 0 && WS_LOSS % 2 == 0, "a partial is 16-byte aligned, its loss 8-byte");
static_assert(WS_STRIDE <= WAVES * 2 * HID * STR, "the workgroup's sum lives in the staging area");

constexpr int APPLY_BLOCK = 64;

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

struct GradArgs {
    const float* theta;
    const float* theta_target;
    const uint64_t* t_dev;
    const float* s;
    const uint8_t* a;
    const float* r;
    const float* s2;
    const uint8_t* d;
    const uint8_t* ok;
    int64_t ld, size, B;
    const int32_t* idx;
    uint64_t seed;
    float gamma;
    int tiles_per_wave;
    int loss_ref;                            // AQUALRN_LOSS_REFERENCE: the broadcast of dqn.py:243-247 in place of the squared TD error
    uint64_t* ws_t;
    float* ws;
    int32_t* idx_out;
    // read and written by grad_body<STRAT, true> alone (libaqua_prio.so); the LAST fields: no other kernel loads them
    const float* weight = nullptr;           // [B] importance weights of the samples
    float* td_out = nullptr;                 // [B] |Q(s)[a] - y| of every sample, -1 for what is no sample
};

// One forward pass of the network with parameters P for the 32 samples of a tile.  x[s]: input 2 s + h of the lane's
// sample (0 beyond the fifth).  h1 / h2: pre-activations, unit unit_of(M, r, h) of the lane's sample; q: the same bits on
// both lane halves.
// Numerics: delta = Q(s)[a] - y is the difference of two sums of 64 large terms and multiplies every gradient element, so
// its rounding is what the gradient's error is made of (the sums over the samples add little to it).  Layer 3, y and
// delta are therefore computed in double from the float32 h2 and rounded once, to delta.
// k2d: the last layer's kernel of P as doubles in LDS, [unit][action].
__device__ __forceinline__ void forward(const float* P, const double* k2d, const float (&x)[3], unsigned h, unsigned col,
                                        f32x16 (&h1)[2], f32x16 (&h2)[2], double (&q)[ACT])
{
#pragma clang fp contract(off)
    // h and col are made opaque here: every address below is then one 32-bit add on a lane offset computed in this pass
    // (otherwise the ~250 64-bit addresses of a pass are computed once in front of the tile loop and spilled)
    asm volatile("" : "+v"(h), "+v"(col), "+s"(P));
    const unsigned ub = 4u * h;                    // unit_of(M, r, h) = unit_of(M, r, 0) + ub
#pragma unroll
    for (int M = 0; M < 2; ++M)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            h1[M][r] = P[OFF_B0 + unit_of(M, r, 0) + ub];
            h2[M][r] = P[OFF_B1 + unit_of(M, r, 0) + ub];
        }
    // (scheduling fences: without them every weight load of a pass is hoisted to its top)
    __builtin_amdgcn_sched_barrier(0);
    // layer 1: 64 x 5, K padded to 6
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const unsigned k = 2u * s + h;
#pragma unroll
        for (int M = 0; M < 2; ++M) {
            const float w = k < IN ? P[OFF_K0 + k * HID + 32 * M + col] : 0.0f;
            h1[M] = mfma(w, x[s], h1[M]);
        }
    }
    // layer 2: 64 x 64.  k-step (M, r): B is this lane's own h1[M][r], A the row of k1 of that unit
    const unsigned k1b = ub * HID + col;
#pragma unroll
    for (int M = 0; M < 2; ++M)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if ((r & 7) == 0) __builtin_amdgcn_sched_barrier(0);
            const float b = fmaxf(h1[M][r], 0.0f);
            h2[0] = mfma(P[OFF_K1 + unit_of(M, r, 0) * HID + k1b], b, h2[0]);
            h2[1] = mfma(P[OFF_K1 + unit_of(M, r, 0) * HID + 32 + k1b], b, h2[1]);
        }
    __builtin_amdgcn_sched_barrier(0);
    // layer 3: 3 x 64 on the VALU in double from the 32 units this lane holds, then one add across the lane halves
    double p[ACT];
#pragma unroll
    for (int c = 0; c < ACT; ++c) p[c] = h == 0 ? static_cast<double>(P[OFF_B2 + c]) : 0.0;
    const double* k2h = k2d + ub * ACT;
    asm volatile("" : "+v"(k2h));
#pragma unroll
    for (int M = 0; M < 2; ++M)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if ((r & 3) == 0) __builtin_amdgcn_sched_barrier(0);
            const double v = static_cast<double>(fmaxf(h2[M][r], 0.0f));
#pragma unroll
            for (int c = 0; c < ACT; ++c) p[c] = fma(k2h[unit_of(M, r, 0) * ACT + c], v, p[c]);
        }
#pragma unroll
    for (int c = 0; c < ACT; ++c) q[c] = p[c] + __shfl_xor(p[c], 32);
    __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ int argmax3(const double (&q)[ACT])    // np.argmax: the lowest index on a tie
{
    int a = 0;
    double best = q[0];
    if (q[1] > best) { a = 1; best = q[1]; }
    if (q[2] > best) { a = 2; }
    return a;
}

__device__ __forceinline__ double pick3(const double (&q)[ACT], int a) { return a == 0 ? q[0] : (a == 1 ? q[1] : q[2]); }

// The gradient kernel's body for workgroup `block` of a launch of BLOCK threads: the partial sums of its tiles into
// a.ws + block * WS_STRIDE.  Everything in `a` is wavefront-uniform.  WEIGHTED: the importance weights of prioritised
// replay multiply the TD error's derivative and its square, and the plain TD error is written out (csrc/aqua_prio.h).
template <int STRAT, bool WEIGHTED = false>
__device__ __forceinline__ void grad_body(const GradArgs& a, const unsigned block)
{
#pragma clang fp contract(off)
    __shared__ float k1t[HID * K1T_STR];
    __shared__ __attribute__((aligned(16))) float stage[WAVES * 2 * HID * STR];
    __shared__ float xs[WAVES][6][TILE];           // rows 0..4: the input of the tile's samples; row 5: delta
    __shared__ int act_s[WAVES][TILE];
    __shared__ float sm[WAVES][4][TILE];           // per-lane sums: db2[0..2], number of valid samples (int bits)
    __shared__ double sl[WAVES][TILE];             // per-lane sums of delta^2
    __shared__ double k2d[2][HID * ACT];           // k2 of the online and of the target network, as doubles
    __shared__ float small[WAVES][32 * SMALL_SLOTS];   // the sums of dk0 | db0, dk2 and db1: [register][slot of the lane]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, col = lane & 31;
    const float* const P = a.theta;
    const float* const PT = a.theta_target;

    for (int i = tid; i < HID * HID; i += BLOCK) k1t[(i >> 6) * K1T_STR + (i & 63)] = P[OFF_K1 + i];
    for (int i = tid; i < HID * ACT; i += BLOCK) {
        k2d[0][i] = static_cast<double>(P[OFF_K2 + i]);
        k2d[1][i] = static_cast<double>(PT[OFF_K2 + i]);
    }

    const uint64_t t_new = *a.t_dev + 1;           // the update this launch belongs to
    if (block == 0 && tid == 0) *a.ws_t = t_new;

    f32x16 acc1[2][2];
#pragma unroll
    for (int M = 0; M < 2; ++M)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc1[M][0][r] = 0.0f; acc1[M][1][r] = 0.0f; }
    // zeroed by the wavefront that owns them; in the tile loop every slot is read and written by one lane only, so no
    // barrier guards `small` there
    for (int i = lane; i < 32 * SMALL_SLOTS; i += 64) small[wave][i] = 0.0f;
    float db2[ACT] = {0.0f, 0.0f, 0.0f};
    double loss = 0.0;
    int count = 0;
    __syncthreads();

    const int64_t tile0 = (static_cast<int64_t>(block) * WAVES + wave) * a.tiles_per_wave;
    for (int it = 0; it < a.tiles_per_wave; ++it) {
        // the lane's coordinates again, from the thread index alone: one register lives across the tile, not four
        unsigned tl = threadIdx.x;
        asm volatile("" : "+v"(tl));
        const int wave = tl >> 6, h = (tl >> 5) & 1, col = tl & 31;
        // LDS offsets of this lane, opaque to the compiler so that every access below is base + immediate (otherwise each of
        // the few hundred addresses is computed in front of the loop and kept in a register of its own)
        unsigned wr = wave * 2 * HID * STR + 4 * h * STR + col;     // [unit_of(M, r, h)][col] of buf0: + unit_of(M, r, 0) * STR
        unsigned rd = wave * 2 * HID * STR + col * STR + h;         // [col][2 st + h] of buf0: + 2 st; second row block: + 32 STR
        unsigned kt = col * K1T_STR + 4 * h;                        // k1t[col][unit_of(M, r, h)]: + unit_of(M, r, 0)
        asm volatile("" : "+v"(wr), "+v"(rd), "+v"(kt));
        unsigned o2 = SLOT_K0 + (IN + 1) * h + (col <= IN ? col : 0), o3 = SLOT_K2 + ACT * h + (col < ACT ? col : 0), o4 = SLOT_B1 + h;
        asm volatile("" : "+v"(o2), "+v"(o3), "+v"(o4));
        float* const sm2 = &small[wave][o2];
        float* const sm3 = &small[wave][o3];
        float* const sm4 = &small[wave][o4];
        // ---------------------------------------------------------------- the sample of this column
        const int64_t j = (tile0 + it) * TILE + col;
        int32_t idx = -1;
        if (j < a.B) {
            if (a.idx != nullptr) {
                const int32_t c = a.idx[j];
                if (c >= 0 && c < a.size && a.ok[c] != 0) idx = c;
            } else {
#pragma unroll 1
                for (int att = 0; att < ATTEMPTS; ++att) {
                    if (idx < 0) {
                        uint32_t rr[4];
                        draw<true>(a.seed, static_cast<uint64_t>(j), t_new, STREAM_LEARNER, static_cast<uint32_t>(att), rr);
                        const int64_t c = static_cast<int64_t>((static_cast<uint64_t>(rr[0]) * static_cast<uint64_t>(a.size)) >> 32);
                        if (c < a.size && a.ok[c] != 0) idx = static_cast<int32_t>(c);
                    }
                }
            }
        }
        int act = 0;
        if (idx >= 0) {
            act = a.a[idx];
            if (act >= ACT) { idx = -1; act = 0; }          // not a discrete action: not a sample
        }
        const bool valid = idx >= 0;
        if (h == 0 && j < a.B && a.idx_out != nullptr) a.idx_out[j] = idx;
        float x[3], x2[3], rew = 0.0f;
        bool done = true;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int row = 2 * s + h;
            const bool live = valid && row < IN;
            x[s] = live ? a.s[row * a.ld + idx] : 0.0f;
            x2[s] = live ? a.s2[row * a.ld + idx] : 0.0f;
        }
        if (valid) {
            rew = a.r[idx];
            done = a.d[idx] != 0;
        }

        // ---------------------------------------------------------------- the bootstrap term, then the online forward on s
        f32x16 h1[2], h2[2];
        double q[ACT], qb[ACT], f = 0.0;
        if constexpr (STRAT == AQUALRN_STANDARD) forward(P, k2d[0], x2, h, col, h1, h2, qb);
        else forward(PT, k2d[1], x2, h, col, h1, h2, qb);
        if constexpr (STRAT == AQUALRN_FIXED || STRAT == AQUALRN_STANDARD) f = fmax(fmax(qb[0], qb[1]), qb[2]);
        if constexpr (STRAT == AQUALRN_DOUBLE) {
            double qo[ACT];
            forward(P, k2d[0], x2, h, col, h1, h2, qo);
            f = pick3(qb, argmax3(qo));
        }
        __builtin_amdgcn_sched_barrier(0);
        forward(P, k2d[0], x, h, col, h1, h2, q);
        if constexpr (STRAT == AQUALRN_DOUBLE_REF) f = pick3(qb, argmax3(q));

        const double y = done ? static_cast<double>(rew) : fma(static_cast<double>(a.gamma), f, static_cast<double>(rew));
        const double qa = pick3(q, act);
        double delta64 = valid ? qa - y : 0.0;
        double sq = delta64 * delta64;
        if (a.loss_ref != 0) {
            // T_j = y for the action taken, Q(s)[j] (a constant) for the other two: d/dQ_a of sum_j (Q_a - T_j)^2 over 2
            const double qo1 = act == 0 ? q[1] : q[0], qo2 = act == 2 ? q[1] : q[2];
            const double e1 = qa - qo1, e2 = qa - qo2;
            delta64 = valid ? 3.0 * qa - y - qo1 - qo2 : 0.0;
            sq = valid ? sq + e1 * e1 + e2 * e2 : 0.0;
        }
        if constexpr (WEIGHTED) {
            // (valid implies j < a.B; a weight of exactly 1 leaves both products the bits they had)
            const double w = valid ? static_cast<double>(a.weight[j]) : 0.0;
            if (h == 0 && j < a.B) a.td_out[j] = valid ? static_cast<float>(fabs(qa - y)) : -1.0f;
            delta64 = w * delta64;
            sq = w * sq;
        }
        const float delta = static_cast<float>(delta64);     // the one rounding between h2 and the backward pass
        loss += sq;
        count += valid ? 1 : 0;
#pragma unroll
        for (int c = 0; c < ACT; ++c) db2[c] += act == c ? delta : 0.0f;

        // ---------------------------------------------------------------- dk2: relu(h2) [unit][sample] x dq
#pragma unroll
        for (int s = 0; s < 3; ++s) xs[wave][2 * s + h][col] = 2 * s + h < IN ? x[s] : delta;
        if (h == 0) act_s[wave][col] = act;
#pragma unroll
        for (int M = 0; M < 2; ++M)
#pragma unroll
            for (int r = 0; r < 16; ++r) stage[wr + unit_of(M, r, 0) * STR] = fmaxf(h2[M][r], 0.0f);
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        {
            f32x16 acc3[2];
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc3[0][r] = 0.0f; acc3[1][r] = 0.0f; }
#pragma unroll
            for (int st = 0; st < TILE / 2; ++st) {
                if ((st & 3) == 0) __builtin_amdgcn_sched_barrier(0);
                const int sI = 2 * st + h;
                const float b = col == act_s[wave][sI] ? xs[wave][5][sI] : 0.0f;
                acc3[0] = mfma(stage[rd + 2 * st], b, acc3[0]);
                acc3[1] = mfma(stage[rd + 2 * st + 32 * STR], b, acc3[1]);
            }
            if (col < ACT) {
#pragma unroll
                for (int M = 0; M < 2; ++M)
#pragma unroll
                    for (int r = 0; r < 16; ++r) sm3[(16 * M + r) * SMALL_SLOTS] += acc3[M][r];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // dh2 = relu'(h2) k2[.][a] delta, in h2's registers
        unsigned k2a = 4u * h * ACT + act;
        asm volatile("" : "+v"(k2a));
#pragma unroll
        for (int M = 0; M < 2; ++M)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                h2[M][r] = h2[M][r] > 0.0f ? P[OFF_K2 + unit_of(M, r, 0) * ACT + k2a] * delta : 0.0f;
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);

        // ---------------------------------------------------------------- dk1, db1: relu(h1) x dh2
#pragma unroll
        for (int M = 0; M < 2; ++M)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                stage[wr + unit_of(M, r, 0) * STR] = fmaxf(h1[M][r], 0.0f);
                stage[wr + unit_of(M, r, 0) * STR + HID * STR] = h2[M][r];
            }
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        const float one0 = col == 0 ? 1.0f : 0.0f;
        f32x16 acc4[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc4[0][r] = 0.0f; acc4[1][r] = 0.0f; }
#pragma unroll
        for (int st = 0; st < TILE / 2; ++st) {
            if ((st & 3) == 0) __builtin_amdgcn_sched_barrier(0);
            const float a0 = stage[rd + 2 * st], a1 = stage[rd + 2 * st + 32 * STR];
            const float b0 = stage[rd + 2 * st + HID * STR], b1 = stage[rd + 2 * st + (HID + 32) * STR];
            acc1[0][0] = mfma(a0, b0, acc1[0][0]);
            acc1[0][1] = mfma(a0, b1, acc1[0][1]);
            acc1[1][0] = mfma(a1, b0, acc1[1][0]);
            acc1[1][1] = mfma(a1, b1, acc1[1][1]);
            acc4[0] = mfma(b0, one0, acc4[0]);
            acc4[1] = mfma(b1, one0, acc4[1]);
        }
        if (col == 0) {
#pragma unroll
            for (int M = 0; M < 2; ++M)
#pragma unroll
                for (int r = 0; r < 16; ++r) sm4[(16 * M + r) * SMALL_SLOTS] += acc4[M][r];
        }
        __builtin_amdgcn_sched_barrier(0);
        // dh1 = relu'(h1) (k1 dh2): k-step (M, r) takes this lane's own dh2 register as B and column unit_of(M, r, h) of k1 as A
        f32x16 d1[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) { d1[0][r] = 0.0f; d1[1][r] = 0.0f; }
#pragma unroll
        for (int M = 0; M < 2; ++M)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if ((r & 7) == 0) __builtin_amdgcn_sched_barrier(0);
                d1[0] = mfma(k1t[kt + unit_of(M, r, 0)], h2[M][r], d1[0]);
                d1[1] = mfma(k1t[kt + unit_of(M, r, 0) + 32 * K1T_STR], h2[M][r], d1[1]);
            }
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);

        // ---------------------------------------------------------------- dk0, db0: dh1 x (x | 1)
#pragma unroll
        for (int M = 0; M < 2; ++M)
#pragma unroll
            for (int r = 0; r < 16; ++r) stage[wr + unit_of(M, r, 0) * STR] = h1[M][r] > 0.0f ? d1[M][r] : 0.0f;
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        {
            f32x16 acc2[2];
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc2[0][r] = 0.0f; acc2[1][r] = 0.0f; }
#pragma unroll
            for (int st = 0; st < TILE / 2; ++st) {
                if ((st & 3) == 0) __builtin_amdgcn_sched_barrier(0);
                const int sI = 2 * st + h;
                const float xv = xs[wave][col < IN ? col : 0][sI];
                const float b = col < IN ? xv : (col == IN ? 1.0f : 0.0f);
                acc2[0] = mfma(stage[rd + 2 * st], b, acc2[0]);
                acc2[1] = mfma(stage[rd + 2 * st + 32 * STR], b, acc2[1]);
            }
            if (col <= IN) {
#pragma unroll
                for (int M = 0; M < 2; ++M)
#pragma unroll
                    for (int r = 0; r < 16; ++r) sm2[(16 * M + r) * SMALL_SLOTS] += acc2[M][r];
            }
        }
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
    }

    // -------------------------------------------------------------------- the workgroup's sum, wavefront by wavefront
    if (h == 0) {
#pragma unroll
        for (int c = 0; c < ACT; ++c) sm[wave][c][col] = db2[c];
        // what the apply kernel divides by: the squares the mean runs over, 3 per valid sample with AQUALRN_LOSS_REFERENCE
        sm[wave][3][col] = __int_as_float(a.loss_ref != 0 ? ACT * count : count);
        sl[wave][col] = loss;
    }
    float* const red = stage;
    const int q1 = OFF_K1 + 4 * h * HID + col;
#pragma unroll 1
    for (int w = 0; w < WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int M = 0; M < 2; ++M)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    // the first wavefront stores, the others add
                    const int p1 = q1 + unit_of(M, r, 0) * HID;
                    red[p1] = w == 0 ? acc1[M][0][r] : red[p1] + acc1[M][0][r];
                    red[p1 + 32] = w == 0 ? acc1[M][1][r] : red[p1 + 32] + acc1[M][1][r];
                }
        }
        __syncthreads();
    }
    // the small sums, straight from their slots: register 16 M + r of a lane is unit unit_of(M, r, 0) + 4 h
    for (int i = tid; i < 32 * SMALL_SLOTS; i += BLOCK) {
        const int reg = i / SMALL_SLOTS, slot = i - reg * SMALL_SLOTS;
        const int u = 32 * (reg >> 4) + (reg & 3) + 8 * ((reg & 15) >> 2);
        int p;
        if (slot < SLOT_K2) {
            const int hh = slot / (IN + 1), c = slot - hh * (IN + 1);
            p = (c < IN ? OFF_K0 + c * HID : OFF_B0) + 4 * hh + u;
        } else if (slot < SLOT_B1) {
            const int hh = (slot - SLOT_K2) / ACT, c = slot - SLOT_K2 - hh * ACT;
            p = OFF_K2 + (4 * hh + u) * ACT + c;
        } else {
            p = OFF_B1 + 4 * (slot - SLOT_B1) + u;
        }
        float sum = small[0][i];
        for (int w = 1; w < WAVES; ++w) sum += small[w][i];
        red[p] = sum;
    }
    if (tid < ACT) {
        float sum = 0.0f;
        for (int w = 0; w < WAVES; ++w)
            for (int c = 0; c < TILE; ++c) sum += sm[w][tid][c];
        red[OFF_B2 + tid] = sum;
    } else if (tid == 3) {
        int n = 0;
        for (int w = 0; w < WAVES; ++w)
            for (int c = 0; c < TILE; ++c) n += __float_as_int(sm[w][3][c]);
        red[WS_COUNT] = __int_as_float(n);
    } else if (tid == 4) {
        double sum = 0.0;
        for (int w = 0; w < WAVES; ++w)
            for (int c = 0; c < TILE; ++c) sum += sl[w][c];
        *reinterpret_cast<double*>(red + WS_LOSS) = sum;
    }
    __syncthreads();
    float* const out = a.ws + static_cast<int64_t>(block) * WS_STRIDE;
    for (int p = tid; p < WS_USED; p += BLOCK) out[p] = red[p];
}

struct ApplyArgs {
    float* theta;
    float* theta_target;
    float* m;
    float* v;
    uint64_t* t_dev;
    const uint64_t* ws_t;
    const float* ws;
    int partials;
    double tau, lr, beta1, beta2, eps;
    float* blob_online;
    float* blob_target;
    const int32_t* perm;
    int64_t blob_floats;
    float* grad_out;
    float* loss;
};

// The apply kernel's body for workgroup `block` of a launch of APPLY_BLOCK threads:
// one thread per parameter: the fixed-order sum of the partials, the scale, Adam, the soft update, the scatter
__device__ __forceinline__ void apply_body(const ApplyArgs& a, const unsigned block)
{
#pragma clang fp contract(off)
    __shared__ int n_sh;
    const int tid = threadIdx.x;
    if (tid == 0) n_sh = 0;
    __syncthreads();
    int mine = 0;
    for (int g = tid; g < a.partials; g += APPLY_BLOCK) mine += __float_as_int(a.ws[static_cast<int64_t>(g) * WS_STRIDE + WS_COUNT]);
    if (mine != 0) atomicAdd(&n_sh, mine);             // integers: any order gives the same sum
    __syncthreads();
    const int n = n_sh;
    const int p = block * APPLY_BLOCK + tid;
    if (n == 0) {                                      // an empty batch changes nothing
        if (p < PARAMS && a.grad_out != nullptr) a.grad_out[p] = 0.0f;
        if (p == 0 && a.loss != nullptr) *a.loss = 0.0f;
        return;
    }
    const uint64_t t = *a.ws_t;
    if (p == 0) {
        *a.t_dev = t;
        if (a.loss != nullptr) {
            double sum = 0.0;
            for (int g = 0; g < a.partials; ++g) sum += *reinterpret_cast<const double*>(a.ws + static_cast<int64_t>(g) * WS_STRIDE + WS_LOSS);
            *a.loss = static_cast<float>(sum / static_cast<double>(n));
        }
    }
    if (p >= PARAMS) return;
    float sum = a.ws[p];
    for (int g = 1; g < a.partials; ++g) sum += a.ws[static_cast<int64_t>(g) * WS_STRIDE + p];
    const float grad = sum * static_cast<float>(2.0 / static_cast<double>(n));
    if (a.grad_out != nullptr) a.grad_out[p] = grad;

    const double td = static_cast<double>(t);
    const float lr_t = static_cast<float>(a.lr * sqrt(1.0 - pow(a.beta2, td)) / (1.0 - pow(a.beta1, td)));
    const double g = static_cast<double>(grad);
    const double m = a.beta1 * static_cast<double>(a.m[p]) + (1.0 - a.beta1) * g;
    const double v = a.beta2 * static_cast<double>(a.v[p]) + (1.0 - a.beta2) * (g * g);
    const float th = static_cast<float>(static_cast<double>(a.theta[p]) - static_cast<double>(lr_t) * m / (sqrt(v) + a.eps));
    const float tg = static_cast<float>(a.tau * static_cast<double>(th) + (1.0 - a.tau) * static_cast<double>(a.theta_target[p]));
    a.m[p] = static_cast<float>(m);
    a.v[p] = static_cast<float>(v);
    a.theta[p] = th;
    a.theta_target[p] = tg;
    if (a.perm != nullptr) {
        const int32_t at = a.perm[p];
        if (at >= 0 && at < a.blob_floats) {
            if (a.blob_online != nullptr) a.blob_online[at] = th;
            if (a.blob_target != nullptr) a.blob_target[at] = tg;
        }
    }
}

constexpr int APPLY_GROUPS = (PARAMS + APPLY_BLOCK - 1) / APPLY_BLOCK;

// ------------------------------------------------------------------ host side
// the launch shape: functions of B alone
struct Shape {
    int64_t tiles;
    int tiles_per_wave, groups;
};

static inline Shape shape_of(int64_t B)
{
    Shape s;
    s.tiles = (B + TILE - 1) / TILE;
    s.tiles_per_wave = static_cast<int>((s.tiles + static_cast<int64_t>(WAVES) * GMAX - 1) / (static_cast<int64_t>(WAVES) * GMAX));
    if (s.tiles_per_wave < 1) s.tiles_per_wave = 1;
    const int64_t per_group = static_cast<int64_t>(WAVES) * s.tiles_per_wave;
    s.groups = static_cast<int>((s.tiles + per_group - 1) / per_group);
    return s;
}

// bytes of one workspace region (the header and the partials of one network) for 0 <= B <= AQUALRN_MAX_BATCH: a multiple
// of 16 that never decreases with B
static inline size_t workspace_region(int64_t B)
{
    // an upper bound of shape_of(B).groups that never decreases with B
    int64_t groups = ((B + TILE - 1) / TILE + WAVES - 1) / WAVES;
    if (groups > GMAX) groups = GMAX;
    if (groups < 1) groups = 1;
    return WS_HEADER + static_cast<size_t>(groups) * WS_STRIDE * sizeof(float);
}
static_assert(WS_HEADER % 16 == 0 && (WS_STRIDE * sizeof(float)) % 16 == 0, "regions stacked behind each other stay 16-byte aligned");

}  // namespace lrn
}  // namespace aqua
