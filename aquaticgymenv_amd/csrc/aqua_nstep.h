/*
 * aqua_nstep.h -- C ABI of libaqua_nstep.so: MULTI-STEP RETURNS from the experience ring of aqua_replay.h, on MI355X
 * (gfx950).  One launch folds, for every sample of a minibatch draw, the window of up to n consecutive transitions of the
 * sample's world into ONE staged transition
 *
 *     (s_t, a_t, R, s_{t+L}, d_{t+L-1}, ok),     R = sum_{k<L} g^k r_{t+k},
 *
 * and derives the bootstrap discount g^n that goes with it.  aqualrn_update_f32 and aqualbank_update_f32 then compute the
 * n-step target y = R + g^n f(s_{t+L}) (masked by d) UNCHANGED: they are handed the staged rows as their ring and g^n as
 * their gamma.  With n = 1 the staged rows are the ring's rows of the drawn slots bit for bit, and the discount is g.
 *
 * Reference being extended: the one-step TD target of main/impl/dqn.py:262-292.
 *
 * This header lies beside the source (the listings of include/ and of the package's include/ are pinned by tests).
 *
 * Conventions are those of aqua_replay.h:
 *  - plain pointers and sizes only (streams are void*); every DEVICE buffer is owned by the caller and borrowed until
 *    the work queued on `stream` has run; the library allocates nothing and keeps no pointer.
 *  - aquanst_fold is asynchronous on `stream` and ONE launch: no allocation, no synchronisation, no host read, so it may
 *    be captured into a HIP graph.  No atomics, no LDS, no floating-point reduction across threads: one thread computes one
 *    sample, the same bits eager or replayed.
 *  - return value: 0 = ok; > 0 = hipError_t; < 0 = AQUANST_E_* (the values of AQUA_E_*).  aquanst_last_error() returns a
 *    thread-local message for the last failing call on this thread.
 *  - every argument is validated before the first HIP call.  There is no CPU path.
 *
 * Why the ring makes this cheap: world i of a batch of N worlds lands in slot base + i (aqua_replay.h), so with
 * capacity % N == 0 (REQUIRED here, as in aqualbank_draw) slot c always holds a transition of world c mod N, and the next
 * step of the same world is slot (c + N) mod capacity.  A window of n steps is n strided reads.
 *
 * The discount.  g = (double)(float)gamma: the float32 the learners round gamma to.  aquanst_discount(gamma, n) is g
 * multiplied by itself n - 1 times in double, every product rounded (n = 1: g itself).  It is stated ONCE, in a
 * __host__ __device__ helper of the source: the host entry and the kernel run the same code.
 *
 * The window of sample c = idx[p][j].  It is NOT a sample (out_ok = 0, zero rows, out_len = 0) if
 *    c is outside [0, capacity), or ok[c] == 0, or the cursor header[0] is outside [0, capacity) or no multiple of N.
 * Otherwise age(c) = ((cursor - N - (c - c mod N)) mod capacity) / N, the rounds written after c's round, and for
 * k = 0, 1, ... with slot_k = (c + k N) mod capacity (64-bit arithmetic):
 *    d[slot_k] != 0 : the window ends here: L = k + 1, out_d = d[slot_k], out_s2 = s2[:, slot_k];
 *    else k == n - 1: the window is full:   L = n,     out_d = 0,         out_s2 = s2[:, slot_k];
 *    else the next step must exist: NOT a sample if k + 1 > age(c) (the window would run past the newest round) or
 *         ok[slot_{k+1}] == 0 (a broken chain: a world reset from outside, or a restart tick with no episode end before it).
 * A window cut short at the ring's frontier is dropped, not bootstrapped with g^L.  out_s and out_a come from slot c.  No
 * computed slot is used as an address unless it lies in [0, capacity); a slot never written has ok == 0, so the size
 * word of the header is not needed.
 *
 * The return.  pw = 1; acc = (double)r[slot_0]; for k = 1 .. L - 1: pw = pw * g; acc = acc + pw * (double)r[slot_k];
 * out_r = (float)acc, rounded once.  Every product and sum is rounded in double and nothing is contracted into a fused
 * multiply-add: the functions that compute are compiled under `#pragma clang fp contract(off)` (the library's command
 * line is the common one; the pragma, not a flag, switches contraction off).
 *
 * AQUANST_MAX_STEPS = 32.  The kernel issues the d, ok and r loads of a window in batches of AQUANST_CHUNK = 8 steps
 * held in registers before the walk looks at any of them, so that a window costs ceil(n / 8) dependent round trips, not n;
 * 32 is four batches; the last batch of a window is as many steps as are left.  Beyond that nothing is gained: with the
 * default gamma = 0.98 the bootstrap weighs 0.98^32 = 0.52 already, an episode lasts 284 steps at most, the share of a draw
 * dropped at the frontier grows as (n - 1) / rounds, and the window length has to fit out_len's byte.
 */
#ifndef AQUA_NSTEP_H
#define AQUA_NSTEP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQUANST_ABI_VERSION 1

/* library error codes (negative): the values of AQUA_E_* in aqua_hip.h */
#define AQUANST_E_INVALID   (-1)   /* bad argument (null pointer, negative size, value out of range ...) */
#define AQUANST_E_ALIGN     (-2)   /* pointer not usable */
#define AQUANST_E_NODEVICE  (-3)   /* no HIP device / wrong architecture */

#define AQUANST_MAX_STEPS     32           /* n at most, see above */
#define AQUANST_CHUNK         8            /* steps whose d, ok, r loads are in flight together */
#define AQUANST_MAX_CAPACITY  2147483647   /* slots: AQUARPL_MAX_CAPACITY */
#define AQUANST_MAX_NETWORKS  4096         /* P at most: AQUALBANK_MAX_NETWORKS */
#define AQUANST_MAX_BATCH     1048576      /* B at most: AQUARPL_MAX_BATCH */
#define AQUANST_MAX_BLOCKS    2048         /* blocks of AQUANST_BLOCK threads per launch at most (grid-stride above that) */
#define AQUANST_BLOCK         256
#define AQUANST_HYPER_WORDS   8            /* doubles per row of the learner bank's table (AQUALBANK_HYPER_WORDS); word 0 is gamma */
#define AQUANST_NO_GAMMA      (-1.0)       /* the scalar gamma of a call that passes hyper_dev */

/* what the action rows hold: the values of AQUARPL_ACT_* */
#define AQUANST_ACT_U8        0    /* a uint8 [ring_ld]          -> out_a uint8 [out_ld] */
#define AQUANST_ACT_F32X2     1    /* a float32 [2][ring_ld]     -> out_a float32 [2][out_ld] */

int aquanst_version(void);                 /* AQUANST_ABI_VERSION */
const char* aquanst_last_error(void);

/*
 * HOST only, no device needed: the bootstrap discount of an n-step target, g^n as defined above.  gamma outside [0, 1]
 * or not a number, or n outside [1, AQUANST_MAX_STEPS]: returns -1.0 and sets the error message.
 */
double aquanst_discount(double gamma, int n);

/*
 * The fold: one launch, one thread per sample.  All pointers are DEVICE pointers.
 *   header               : the ring's int64 [4] header, 8-byte aligned; word [0] (the cursor) is read, nothing is written
 *                          (the header rule of aqua_replay.h: no thread of this launch writes a header word)
 *   s, a, r, s2, d, ok   : the ring's six rows, read only; ring_ld >= capacity, 1 <= capacity <= AQUANST_MAX_CAPACITY
 *   action_kind          : AQUANST_ACT_U8 or AQUANST_ACT_F32X2, as in aquarpl_gather
 *   N                    : worlds per batched step, 1 <= N <= capacity and capacity % N == 0
 *   idx, P, B            : int32 [P][B] slots, 1 <= P <= AQUANST_MAX_NETWORKS, 0 <= B <= AQUANST_MAX_BATCH
 *   n                    : the window, 1 <= n <= AQUANST_MAX_STEPS
 *   gamma, hyper_dev     : exactly one of them.  hyper_dev == NULL: the scalar gamma in [0, 1] for every sample.  Otherwise
 *                          gamma must be AQUANST_NO_GAMMA and hyper_dev is float64 [P][AQUANST_HYPER_WORDS], the learner
 *                          bank's table (8-byte aligned): the samples of row p use its word 0, gamma_p
 *   out_ld               : the pitch of the staged rows, >= P * B; sample (p, j) is position p * B + j
 *   out_s, out_s2        : float32 [5][out_ld];  out_r float32 [out_ld];  out_a uint8 [out_ld] or float32 [2][out_ld]
 *   out_d, out_ok        : uint8 [out_ld]: the termination code that ended the window (0: none), and 1 for a sample
 *   out_len              : nullable uint8 [out_ld]: the window length L, 0 for no sample
 *   hyper_out            : nullable float64 [P][AQUANST_HYPER_WORDS], only with hyper_dev and not overlapping it: row p
 *                          of hyper_dev with word 0 replaced by aquanst_discount(gamma_p, n); written by the thread of
 *                          sample j == 0 of row p
 * B == 0 returns 0 without a launch (hyper_out is then not written).
 */
int aquanst_fold(const int64_t* header, const float* s, const void* a, const float* r, const float* s2, const uint8_t* d,
                 const uint8_t* ok, int64_t ring_ld, int64_t capacity, int action_kind, int64_t N,
                 const int32_t* idx, int64_t P, int64_t B, int n, double gamma, const double* hyper_dev,
                 float* out_s, void* out_a, float* out_r, float* out_s2, uint8_t* out_d, uint8_t* out_ok, int64_t out_ld,
                 uint8_t* out_len, double* hyper_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
