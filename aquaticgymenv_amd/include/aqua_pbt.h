/*
 * aqua_pbt.h -- C ABI of libaqua_pbt.so: SELECTION among the networks of a population on MI355X (gfx950).  Asynchronous
 * population-based training (Jaderberg et al. 2017, "Population Based Training of Neural Networks", truncation
 * selection): the worst networks of a learner bank (aqua_lbank.h) take the weights, the optimiser state and the perturbed
 * hyper-parameters of networks drawn from the best, judged by the statistics aqua_segments.h publishes.
 *
 * Conventions are those of aqua_segments.h:
 *  - plain pointers, sizes and numbers only (streams are void*); every DEVICE buffer is owned by the caller and borrowed
 *    until the work queued on `stream` has run; the library allocates nothing and keeps no pointer.  ALL state is device
 *    memory.
 *  - the entry is asynchronous on `stream`: no allocation, no synchronisation, no host read, so it may be captured into a
 *    HIP graph.  It is TWO launches.
 *  - return value: 0 = ok; > 0 = hipError_t; < 0 = AQUAPBT_E_* (the values of AQUA_E_*).
 *  - every argument is validated before the first HIP call.  There is no CPU path.
 *
 * Launch structure.  PLAN is one workgroup of up to 1024 threads: it ranks the networks with a bitonic sort of 64-bit words
 * in LDS (32 KiB at P = 4096), chooses losers and parents and writes everything that is per network and small: parent,
 * origin, mark, the hyper-parameter rows, the epsilon schedules and the header.  COPY has a grid over (chunk, four
 * networks): a block reads parent[p] of its networks and copies its chunk of row parent[p] to row p where that is not p.  Neither launch
 * uses an atomic on memory or a floating-point atomic, neither waits on another block; all stores are plain vector stores.
 * The same inputs give the same bits run to run, eager or replayed from a graph.
 */
#ifndef AQUA_PBT_H
#define AQUA_PBT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQUAPBT_ABI_VERSION 1

/* library error codes (negative): the values of AQUA_E_* in aqua_hip.h */
#define AQUAPBT_E_INVALID   (-1)   /* bad argument (null pointer, size or value out of range, arrays that overlap ...) */
#define AQUAPBT_E_ALIGN     (-2)   /* pointer not usable */
#define AQUAPBT_E_NODEVICE  (-3)   /* no HIP device / wrong architecture */

#define AQUAPBT_MAX_NETWORKS 4096         /* P at most (AQUALBANK_MAX_NETWORKS) */
#define AQUAPBT_PARAMS       4739         /* floats of a row of theta, theta_target, m, v (AQUALBANK_PARAMS) */
#define AQUAPBT_MAX_BLOB     1048576      /* blob_floats at most */
#define AQUAPBT_HEADER       4            /* uint64 slots of header[] */
#define AQUAPBT_COUNTS       8            /* uint64 slots of a row of seg_counts[][] (AQUASEG_COUNTS) */
#define AQUAPBT_HYPER_WORDS  8            /* doubles of a row of hyper[][] (AQUALBANK_HYPER_WORDS) */
#define AQUAPBT_HYPER_GAMMA  0            /* the word of a row that holds gamma */
#define AQUAPBT_HYPER_LR     2            /* the word of a row that holds lr */
#define AQUAPBT_STREAM       7            /* Philox stream of the selection draws (0, 1, 3, 4, 5 and 6 are taken) */

int aquapbt_version(void);                /* AQUAPBT_ABI_VERSION */
const char* aquapbt_last_error(void);

/*
 * One selection.  All pointers are DEVICE pointers.
 *   score          : float32 [P], read only: what the networks are ranked by, higher is better (mean_ret or success of
 *                    aqua_segments.h).
 *   seg_counts     : uint64 [P][AQUAPBT_COUNTS], read only: word 0 of row p is the number of episodes network p has finished
 *                    (aqua_segments.h's seg_counts).
 *   P              : networks, in [1, AQUAPBT_MAX_NETWORKS]
 *   header         : uint64 [AQUAPBT_HEADER], 8-byte aligned: [0] calls so far; [1] networks replaced so far; [2] networks
 *                    replaced by the last call; [3] networks scored by the last call.
 *   mark           : uint64 [P]: seg_counts[p][0] as it was when network p was last replaced; initially 0.
 *   origin         : int32 [P]: the initial network slot p descends from; initially p.
 *   parent         : int32 [P]: written by every call; parent[p] == p where the call left network p alone.
 *   theta, theta_target, m, v
 *                  : float32 [P][AQUAPBT_PARAMS], 4-byte aligned: the stacked state of aqua_lbank.h.
 *   t              : uint64 [P], 8-byte aligned: its update counters.
 *   blob_online, blob_target
 *                  : float32 [P][blob_floats], 16-byte aligned; blob_floats a multiple of 4 in [4, AQUAPBT_MAX_BLOB].
 *   hyper          : float64 [P][AQUAPBT_HYPER_WORDS], 8-byte aligned: the learner bank's device table.
 *   eps_state, eps_out
 *                  : float64 [P] and float32 [P], the schedules of aqua_segments.h; both NULL: they are not inherited
 *                    (exactly one NULL: AQUAPBT_E_INVALID).
 *   fraction       : 0 < fraction <= 0.5, not NaN
 *   ready, every   : >= 1
 *   seed           : the Philox key of the draws
 *   lr_factor0, lr_factor1, lr_lo, lr_hi
 *                  : the two factors lr is perturbed by (finite, > 0) and its bounds, 0 < lr_lo <= lr_hi, finite
 *   gamma_factor0, gamma_factor1, gamma_lo, gamma_hi
 *                  : the two factors 1 - gamma is perturbed by (finite, > 0) and gamma's bounds, 0 <= gamma_lo <= gamma_hi <= 1
 * No two of the arrays above may share a byte (AQUAPBT_E_INVALID).
 *
 * The call, with unsigned 64-bit integers that wrap and IEEE float64 without contraction:
 *  1. c = header[0]; header[0] = c + 1.  If c % every != 0: parent[p] = p for every p, header[2] = 0, and nothing else is
 *     written.
 *  2. Network p is SCORED iff seg_counts[p][0] >= 1; S is their number.  With u the 32 bits of score[p], its key is
 *     (u >> 31) ? ~u : (u | 0x80000000) as a uint32: the order of the floats, -0.0 below +0.0, and every bit pattern (NaNs
 *     too) has a place.  The scored networks are ranked by key, higher first, equal keys by index, lower first; rank 0 is the
 *     best.  net(i) is the network at rank i.
 *  3. k = (uint32)floor(fraction * (double)S).  Network p is READY iff seg_counts[p][0] - mark[p] >= ready.  The LOSERS are
 *     the networks net(i), S - k <= i < S, that are ready; n is their number.  A network of the bottom k that is not ready
 *     is skipped, not substituted.  (The quantile is over all scored networks: a fresh child keeps its stale score and its
 *     place at the bottom until it is ready again, so replacements do not cascade through the population.)
 *  4. For every loser p: r = Philox4x32-10(key = seed, counter = (env = p, tick = c), stream AQUAPBT_STREAM, attempt 0) in
 *     the counter layout of aqua_hip.h's draws; j = (uint64(r[0]) * k) >> 32; q = net(j), one of the best k.  Then
 *       parent[p] = q; origin[p] = origin[q]; mark[p] = seg_counts[p][0];
 *       hyper[p][w] = hyper[q][w] for w = 0..7, except
 *         hyper[p][AQUAPBT_HYPER_LR]    = min(max(lr_q * lr_factor[r[1] & 1], lr_lo), lr_hi)
 *         hyper[p][AQUAPBT_HYPER_GAMMA] = min(max(1.0 - (1.0 - gamma_q) * gamma_factor[r[2] & 1], gamma_lo), gamma_hi)
 *       with lr_q, gamma_q the words of row q; each product, difference, max and min one float64 operation;
 *       eps_state[p] = eps_state[q]; eps_out[p] = eps_out[q], if they are given.
 *     Every other network gets parent[p] = p.  header[1] += n; header[2] = n; header[3] = S.
 *  5. For every p with parent[p] = q != p, row p of theta, theta_target, m, v, t, blob_online and blob_target becomes row q,
 *     byte for byte.  A parent is never a loser of the same call (2 k <= S): every copy reads rows nobody writes.
 * Nothing else is written: not score, not seg_counts, no row of a network that is not a loser.
 */
int aquapbt_select(const float* score, const uint64_t* seg_counts, int64_t P,
                   uint64_t* header, uint64_t* mark, int32_t* origin, int32_t* parent,
                   float* theta, float* theta_target, float* m, float* v, uint64_t* t,
                   float* blob_online, float* blob_target, int64_t blob_floats,
                   double* hyper, double* eps_state, float* eps_out,
                   double fraction, int64_t ready, int64_t every, uint64_t seed,
                   double lr_factor0, double lr_factor1, double lr_lo, double lr_hi,
                   double gamma_factor0, double gamma_factor1, double gamma_lo, double gamma_hi,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
