/*
 * aqua_evo.h -- C ABI of libaqua_evo.so: NATURAL EVOLUTION STRATEGIES on a bank of Q-networks, on MI355X (gfx950).  Salimans
 * et al. 2017, "Evolution Strategies as a Scalable Alternative to Reinforcement Learning": a bank of P = 2H networks holds
 * the antithetic perturbations theta +- sigma eps of one centre theta, every member flies its own segment of worlds, the
 * members are ranked by return and the centre takes one Adam (or SGD) step along sum (rank difference) eps.  No replay ring,
 * no TD target, no backward pass.  The noise is never stored: it is regenerated from Philox when the centre is stepped.
 *
 * The arithmetic is chosen so that every result is an exact integer or a short, stated chain of rounded float64 operations:
 * the noise numerator, the rank differences and the fixed-point fitness sums are integers, so nothing depends on a summation
 * order, integer atomics are harmless, and a numpy model gives the same bits.
 *
 * This header lies beside the source (the listings of include/ and of the package's include/ are pinned by tests).
 *
 * Conventions are those of aqua_pbt.h and aqua_her.h:
 *  - plain pointers and sizes only (streams are void*); every DEVICE buffer is owned by the caller and borrowed until the
 *    work queued on `stream` has run; the library allocates nothing and keeps no pointer.
 *  - aquaevo_ask, aquaevo_fitness and aquaevo_tell are asynchronous on `stream`: no allocation, no synchronisation, no host
 *    read, so each may be captured into a HIP graph.  ask is ONE launch, fitness THREE launches (three graph nodes), tell
 *    TWO launches.
 *  - return value: 0 = ok; > 0 = hipError_t; < 0 = AQUAEVO_E_* (the values of AQUA_E_*).  aquaevo_last_error() returns a
 *    thread-local message for the last failing call on this thread.
 *  - every argument is validated before the first HIP call.  There is no CPU path.
 *
 * THE NOISE, stated once: aquaevo_noise(seed, g, j, i), g the generation, j the antithetic pair, i the parameter.
 *    r = Philox4x32-10(key = seed, counter = (env = (uint64)j << 32 | i, tick = g), stream AQUAEVO_STREAM = 9, attempt 0) in
 *        the counter layout of aqua_device.hpp: key (seed lo, seed hi), counter (env lo, env hi, tick lo,
 *        tick hi[15:0] | attempt << 16 | stream << 24) -- here (i, j, g lo, (g >> 32 & 0xFFFF) | 9 << 24).
 *    S = the sum of the eight 16-bit halves of r[0..3];  n = 2 S - 524280, an integer with |n| <= 524280.
 *    eps = (double)n * C with the literal C = AQUAEVO_C = 0x1.3988e1412ed76p-17 = 1 / (2 sqrt(8 (65536^2 - 1) / 12)).
 * An Irwin-Hall sum: symmetric, |eps| < 4.9, excess kurtosis -0.15, variance 1 up to C's rounding -- NOT a Gaussian; a
 * first-order antithetic estimator needs isotropic unit-covariance noise and no more.  No transcendental is involved: host,
 * device and numpy agree bit for bit.  One __host__ __device__ function of the source computes n for the host entry and for
 * both kernels.  (Streams 0, 1, 3 .. 8 are taken.)
 *
 * ASK, for H = P / 2 rounded down and g = header[0] read on the device.  For j < H and every parameter i < 4739:
 *    d = sigma * eps(seed, g, j, i)                      one float64 product
 *    x = (double)theta[i] + d  for slot 2j,   (double)theta[i] - d  for slot 2j + 1          one add or subtract
 *    blob[slot][perm[i]] = (float)x                      rounded once, nothing contracted
 * If P is odd, slot 2H is the centre: the bits of theta[i].  perm is the learner's permutation (parameter i of the canonical
 * Keras order k0, b0, k1, b1, k2, b2 lives at blob float perm[i]).  Only the 4739 parameter floats of a slot are written; a
 * perm entry outside [0, blob_floats) is skipped and never used as an address.  P = 1 writes the centre alone.  The noise is
 * computed once per pair and both signs are stored from it.
 *
 * FITNESS reduces one EpisodeTracker log (aqua_episodes.h) to a score per segment.  Records 0 .. min(counts[0], C) - 1 are
 * read; a record whose world lies outside [env_offset, env_offset + min(N, P seg)) is skipped, otherwise it belongs to
 * segment p = (world - env_offset) / seg.  If `finished` is given, a local world w < min(N, P seg) with finished[w] == 0
 * counts as one more episode of segment w / seg, with return ret[w] and code 0.
 *    quantisation (aquaevo_quantise): x = (double)ret; x = 0 if ret is a NaN by its bits; x clamped to +-2048;
 *                                     q = llrint(x * 2^20), ties to even
 *    sum of q, count and successes (code 3) per segment: int64, exact in any order (integer atomics)
 *    kind 0 (AQUAEVO_MEAN_RETURN):  fitness[p] = (float)(((double)sum / 1048576.0) / (double)count)
 *    kind 1 (AQUAEVO_SUCCESS_RATE): fitness[p] = (float)((double)successes / (double)count)
 *    count == 0: fitness[p] has the bits of -infinity.       episodes[p] = count.
 * The three launches: acc is zeroed; records and unfinished worlds are accumulated (grid-stride above AQUAEVO_MAX_BLOCKS
 * blocks); fitness and episodes are written.  acc[p] = (sum, count, successes) is left as the accumulation wrote it.
 *
 * TELL is RANK, one workgroup, integers only, then STEP.
 * RANK.  The key of slot p < 2H is aquapbt_select's (aquaevo_key): with u the bits of fitness[p], (u >> 31) ? ~u :
 * (u | 0x80000000) -- every bit pattern, NaNs included, has a place.
 *    rank2[p] = 2 #{q : key_q < key_p} + #{q : key_q = key_p} - 1     the doubled mid-rank: no order of a sort enters, and a
 *                                                                     tied antithetic pair weighs 0
 *    weights[j] = rank2[2j] - rank2[2j + 1]
 * The centre slot of an odd P is not ranked.  The same launch does the scalar bookkeeping, with g = header[0] before it:
 *    header[AQUAEVO_H_GENERATION = 0] = g + 1         header[AQUAEVO_H_TELLS = 1] += 1
 *    header[AQUAEVO_H_STEPPED = 2] = g                 the generation this tell steps with
 *    header[AQUAEVO_H_BEST = 3] = the ranked slot of the highest key, the lowest index on a tie (AQUAEVO_NO_SLOT if H = 0)
 *    header[AQUAEVO_H_RANKED = 4] = 2H                 words 5 .. 7 are not touched
 *    t[0] = t[0] + 1
 * STEP, for parameter i, with g = header[2] and t = t[0] as RANK left them:
 *    1. G = sum_j weights[j] * n(seed, g, j, i)        an int64, |G| < 2^44, exact in any order
 *    2. D = (double)(4 H (2H - 1)) * sigma;  scale = C / D
 *    3. ghat = (double)G * scale                       the ascent direction: 1/(2 H sigma) sum_p u_p s_p eps with centred
 *                                                      ranks u in [-1/2, 1/2]
 *    4. grad = weight_decay * (double)theta[i] - ghat                 (grad_out[i] = grad, if given)
 *    5. Adam (optimizer 0), b^t in float64 by binary exponentiation, least-significant bit first, as aqua_segments.h states it:
 *           md = beta1 * m + (1 - beta1) * grad            vd = beta2 * v + (1 - beta2) * (grad * grad)
 *           theta' = (float)(theta - lr * (md / (1 - beta1^t)) / (sqrt(vd / (1 - beta2^t)) + eps))
 *           m = (float)md, v = (float)vd
 *       every operation one rounded float64 operation, nothing contracted, (lr * mhat) / (...) from left to right
 *    6. SGD (optimizer 1): theta' = (float)(theta - lr * grad); m and v are not touched
 * Steps 2 .. 6 are one __host__ __device__ function: the host entry aquaevo_step_param and the kernel run the same code.
 * H = 0 (P = 1) writes nothing but the bookkeeping.  sigma, seed and the generation must be the ask's.
 */
#ifndef AQUA_EVO_H
#define AQUA_EVO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQUAEVO_ABI_VERSION 1

/* library error codes (negative): the values of AQUA_E_* in aqua_hip.h */
#define AQUAEVO_E_INVALID   (-1)   /* bad argument (null pointer, negative size, value out of range, overlap ...) */
#define AQUAEVO_E_ALIGN     (-2)   /* pointer not usable */
#define AQUAEVO_E_NODEVICE  (-3)   /* no HIP device / wrong architecture */

#define AQUAEVO_PARAMS        4739         /* canonical Keras order k0, b0, k1, b1, k2, b2: the learner's theta layout */
#define AQUAEVO_MAX_NETWORKS  4096         /* P at most */
#define AQUAEVO_STREAM        9            /* the Philox stream of the noise (0, 1, 3, 4, 5, 6, 7 and 8 are taken) */
#define AQUAEVO_FIX_BITS      20           /* fitness sums are in 2^-20 fixed point, as the sum tree of aqua_prio.h */
#define AQUAEVO_CLAMP         2048         /* a return is clamped to +-AQUAEVO_CLAMP before it is quantised */
#define AQUAEVO_NOISE_OFFSET  524280       /* 8 * 65535: n = 2 S - AQUAEVO_NOISE_OFFSET */
#define AQUAEVO_C             0x1.3988e1412ed76p-17
#define AQUAEVO_MAX_BLOB      1048576      /* blob_floats at most: AQUAPBT_MAX_BLOB */
#define AQUAEVO_MAX_WORLDS    2147483647   /* N, C, seg at most */
#define AQUAEVO_BLOCK         256
#define AQUAEVO_MAX_BLOCKS    1024         /* blocks of the accumulation at most (grid-stride above that) */
#define AQUAEVO_TERM_SUCCESS  3            /* AQUA_TERM_SUCCESS */

#define AQUAEVO_MEAN_RETURN   0            /* kind */
#define AQUAEVO_SUCCESS_RATE  1
#define AQUAEVO_ADAM          0            /* optimizer */
#define AQUAEVO_SGD           1

#define AQUAEVO_HEADER        8            /* uint64 words of header[] */
#define AQUAEVO_H_GENERATION  0
#define AQUAEVO_H_TELLS       1
#define AQUAEVO_H_STEPPED     2
#define AQUAEVO_H_BEST        3
#define AQUAEVO_H_RANKED      4
#define AQUAEVO_NO_SLOT       0xFFFFFFFFFFFFFFFFull
#define AQUAEVO_ACC           3            /* int64 words of acc[] per segment: sum, count, successes */

int aquaevo_version(void);                 /* AQUAEVO_ABI_VERSION */
const char* aquaevo_last_error(void);

/* HOST only, no device needed: n of the noise as defined above -- the kernels' own code.  i and j are not range-checked. */
int32_t aquaevo_noise(uint64_t seed, uint64_t g, uint32_t j, uint32_t i);

/* HOST only: q of a return as defined above -- the kernel's own code. */
int64_t aquaevo_quantise(float ret);

/* HOST only: the ranking key of a fitness, by its bits -- the kernel's own code. */
uint32_t aquaevo_key(float fitness);

/*
 * HOST only: steps 2 .. 6 for one parameter -- the kernel's own code.  G as in step 1, H >= 1, t the INCREMENTED counter
 * (>= 1).  io[3] = {theta, m, v} is read and rewritten (SGD leaves m and v); grad, if not NULL, receives step 4's grad.
 * Returns AQUAEVO_E_INVALID for io == NULL, H outside [1, AQUAEVO_MAX_NETWORKS / 2], t == 0 or what aquaevo_tell rejects in
 * sigma, lr, beta1, beta2, eps, weight_decay or optimizer.
 */
int aquaevo_step_param(int64_t G, int64_t H, double sigma, double lr, double beta1, double beta2, double eps, double weight_decay,
                       int optimizer, uint64_t t, float io[3], double* grad);

/*
 * ASK: one launch over (pair, parameter).  All pointers are DEVICE pointers.
 *   theta        : float32 [4739], 4-byte aligned, read only
 *   perm         : int32 [4739], 4-byte aligned, read only
 *   header       : uint64 [AQUAEVO_HEADER], 8-byte aligned; word 0 (the generation) is read, nothing is written
 *   P            : 1 <= P <= AQUAEVO_MAX_NETWORKS
 *   sigma        : finite and >= 0
 *   blob         : float32 [P][blob_floats], 16-byte aligned; blob_floats a multiple of 4 in [4, AQUAEVO_MAX_BLOB]
 * theta, perm, header and blob may not overlap.
 */
int aquaevo_ask(const float* theta, const int32_t* perm, const uint64_t* header, int64_t P, double sigma, uint64_t seed,
                float* blob, int64_t blob_floats, void* stream);

/*
 * FITNESS: three launches.  All pointers are DEVICE pointers.
 *   log_ret, log_code, log_world : float32 [C], uint8 [C], int64 [C]: the tracker's log, read only; 1 <= C <= AQUAEVO_MAX_WORLDS
 *   counts                       : uint64 [>= 1], 8-byte aligned, read only; word 0 is the log's cursor
 *   ret, finished                : both NULL, or float32 [N] and uint8 [N]: the running returns and the once-flags
 *   env_offset, N, seg, P        : env_offset >= 0; 0 <= N <= AQUAEVO_MAX_WORLDS; 1 <= seg <= AQUAEVO_MAX_WORLDS;
 *                                  1 <= P <= AQUAEVO_MAX_NETWORKS
 *   kind                         : AQUAEVO_MEAN_RETURN or AQUAEVO_SUCCESS_RATE
 *   acc                          : int64 [P][AQUAEVO_ACC], 8-byte aligned: the workspace
 *   fitness, episodes            : float32 [P], int64 [P]: the outputs
 * acc, fitness and episodes may overlap neither one another nor an input.
 */
int aquaevo_fitness(const float* log_ret, const uint8_t* log_code, const int64_t* log_world, int64_t C, const uint64_t* counts,
                    const float* ret, const uint8_t* finished, int64_t env_offset, int64_t N, int64_t seg, int64_t P, int kind,
                    int64_t* acc, float* fitness, int64_t* episodes, void* stream);

/*
 * TELL: two launches.  All pointers are DEVICE pointers.
 *   fitness               : float32 [P], read only
 *   header                : uint64 [AQUAEVO_HEADER], 8-byte aligned, read and written as stated above
 *   theta, m, v           : float32 [4739], read and written
 *   t                     : uint64 [1], 8-byte aligned
 *   sigma                 : finite and > 0;  lr finite and >= 0;  0 <= beta1 < 1;  0 <= beta2 < 1;  eps finite and > 0;
 *                           weight_decay finite and >= 0;  optimizer AQUAEVO_ADAM or AQUAEVO_SGD
 *   rank2, weights        : int32 [2H], int32 [H], written (with H = 0 they are not touched and may be NULL)
 *   grad_out              : NULL or float64 [4739], 8-byte aligned
 * No two buffers may overlap.
 */
int aquaevo_tell(const float* fitness, int64_t P, uint64_t* header, float* theta, float* m, float* v, uint64_t* t,
                 double sigma, uint64_t seed, double lr, double beta1, double beta2, double eps, double weight_decay, int optimizer,
                 int32_t* rank2, int32_t* weights, double* grad_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
