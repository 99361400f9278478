/*
 * aqua_her.h -- C ABI of libaqua_her.so: HINDSIGHT EXPERIENCE REPLAY on the experience ring of aqua_replay.h, on MI355X
 * (gfx950).  One launch stages, for every sample of a minibatch draw, the drawn transition -- as it is stored, or RELABELLED:
 * replayed under another goal, a position the sample's own world really reached later in the same episode (Andrychowicz et
 * al., 2017, strategy "future").  aqualrn_update_f32 and aqualbank_update_f32 are then handed the staged rows as their ring,
 * UNCHANGED.
 *
 * Why a relabelled transition is exact here.  The observation is (x, y, theta, gx, gy) (gym_aqua/envs/aqua.py:46-49, 126,
 * 213): the goal is two of its five columns.  Whenever a step ends in neither a collision nor the time limit, reward and
 * termination are a function of (previous position, new position, goal) alone (aqua.py:206-211, 392-395, 421-422).  So a
 * step with d == 0 is replayed under the goal g' by overwriting two columns and recomputing one reward; nothing is
 * approximated.
 *
 * This header lies beside the source (the listings of include/ and of the package's include/ are pinned by tests).
 *
 * Conventions are those of aqua_nstep.h:
 *  - plain pointers and sizes only (streams are void*); every DEVICE buffer is owned by the caller and borrowed until
 *    the work queued on `stream` has run; the library allocates nothing and keeps no pointer.
 *  - aquaher_relabel is asynchronous on `stream` and ONE launch: no allocation, no synchronisation, no host read, so it may
 *    be captured into a HIP graph.  No atomics, no LDS, no reduction across threads: one thread computes one sample, the same
 *    bits eager or replayed.
 *  - return value: 0 = ok; > 0 = hipError_t; < 0 = AQUAHER_E_* (the values of AQUA_E_*).  aquaher_last_error() returns a
 *    thread-local message for the last failing call on this thread.
 *  - every argument is validated before the first HIP call.  There is no CPU path.
 *  - capacity % N == 0 is REQUIRED: slot c then always holds a transition of world c mod N, and the next step of the same
 *    world is slot (c + N) mod capacity.
 *
 * THE RULE, for sample c = idx[p][j] (position i = p B + j of the staged rows).
 *
 * Is it a sample?  It is NOT (out_ok = 0, zero rows, out_k = 0, out_m = 0) if c is outside [0, capacity), or ok[c] == 0, or
 * the cursor header[0] is outside [0, capacity) or no multiple of N: the fold's own rule.  age(c) is the fold's:
 * ((cursor - N - (c - c mod N)) mod capacity) / N, the rounds written after c's round.
 *
 * The walk.  For k = 0 .. H - 1 with slot_k = (c + k N) mod capacity (64-bit arithmetic): stop if k > age(c), or if k > 0
 * and ok[slot_k] == 0, or if d[slot_k] != 0; otherwise M = k + 1.  M is the number of leading non-terminal steps of the
 * sample's world, up to the horizon H: the episode's end, a broken chain and the ring's newest round all cut it short, and
 * -- unlike the fold -- the frontier truncates the walk and drops nothing.  Only steps with d == 0 are candidates: their s2
 * is the position the boat really reached, whatever the restart mode writes at a terminal step, and a boat that has not
 * collided is a legal goal (same radius, same border and obstacle predicates).  A sample whose own step is terminal has
 * M = 0 and is never relabelled.  No computed slot is used as an address unless it lies in [0, capacity).
 * 1 <= H <= AQUAHER_MAX_HORIZON = 64; the kernel issues the d and ok loads of a walk in batches of AQUAHER_CHUNK = 8 steps
 * held in registers before the walk looks at any of them, as the fold does.
 *
 * The draw.  r = Philox4x32-10(key = seed_p, counter = (j, t_p + 1), stream AQUAHER_STREAM, attempt 0) in the layout of
 * aqualbank_draw (streams 0, 1, 3, 4, 5, 6 and 7 are taken).  t_p and seed_p are the learner's or the bank's own device
 * counters and keys: t_dev is uint64 [P]; the key is seed_dev[p], or, with seed_dev == NULL, the scalar `seed` for every row
 * (a single learner keeps its seed on the host).  Relabel if and only if M > 0 and (uint64)r[0] < thr, where
 * thr = aquaher_threshold(ratio) = floor(ratio 2^32) as a uint64: ratio = 1 gives 2^32 (always), ratio = 0 gives 0 (never).
 * k = ((uint64)r[1] M) >> 32.
 *
 * Relabelled.  g' = (s2[0][slot_k], s2[1][slot_k]), the float32 bits as stored.  out_s and out_s2 are the rows of slot c
 * with rows 3 and 4 replaced by g'; out_a is copied.  The reward, in double, every operation rounded, nothing contracted
 * (`#pragma clang fp contract(off)`):
 *    gap(q) = 100.0 * sqrt(dx * dx + dy * dy) - 5.0,   dx = (double)q_x - (double)g'_x,   dy likewise
 *    gap_prev from s[0:2][c], gap_new from s2[0:2][c]
 *    gap_new <= 0 :  out_r = 10, out_d = 3 (AQUA_TERM_SUCCESS)
 *    otherwise    :  out_r = (float)(0.7 * (gap_prev - gap_new)), out_d = 0
 * k = 0 gives gap_new = -5, a success; a path that merely passes within the radius of a later position is one too.
 * out_k = k + 1, out_m = M.  The reward is stated ONCE, in a __host__ __device__ function of the source: the host entry
 * aquaher_reward and the kernel run the same code.
 *
 * Not relabelled.  All six rows of slot c are copied bit for bit, out_k = 0, out_m = M.  With ratio = 0 the staged
 * minibatch is the ring's own rows of the drawn slots.
 */
#ifndef AQUA_HER_H
#define AQUA_HER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQUAHER_ABI_VERSION 1

/* library error codes (negative): the values of AQUA_E_* in aqua_hip.h */
#define AQUAHER_E_INVALID   (-1)   /* bad argument (null pointer, negative size, value out of range ...) */
#define AQUAHER_E_ALIGN     (-2)   /* pointer not usable */
#define AQUAHER_E_NODEVICE  (-3)   /* no HIP device / wrong architecture */

#define AQUAHER_MAX_HORIZON   64           /* H at most */
#define AQUAHER_CHUNK         8            /* steps whose d and ok loads are in flight together */
#define AQUAHER_STREAM        8            /* the Philox stream of the relabelling draws (0, 1, 3, 4, 5, 6 and 7 are taken) */
#define AQUAHER_MAX_CAPACITY  2147483647   /* slots: AQUARPL_MAX_CAPACITY */
#define AQUAHER_MAX_NETWORKS  4096         /* P at most: AQUALBANK_MAX_NETWORKS */
#define AQUAHER_MAX_BATCH     1048576      /* B at most: AQUARPL_MAX_BATCH */
#define AQUAHER_MAX_BLOCKS    2048         /* blocks of AQUAHER_BLOCK threads per launch at most (grid-stride above that) */
#define AQUAHER_BLOCK         256
#define AQUAHER_NO_SEED       0            /* the scalar seed of a call that passes seed_dev */
#define AQUAHER_TERM_SUCCESS  3            /* out_d of a relabelled success: AQUA_TERM_SUCCESS */

/* what the action rows hold: the values of AQUARPL_ACT_* */
#define AQUAHER_ACT_U8        0    /* a uint8 [ring_ld]          -> out_a uint8 [out_ld] */
#define AQUAHER_ACT_F32X2     1    /* a float32 [2][ring_ld]     -> out_a float32 [2][out_ld] */

int aquaher_version(void);                 /* AQUAHER_ABI_VERSION */
const char* aquaher_last_error(void);

/*
 * HOST only, no device needed: thr = floor(ratio 2^32).  ratio outside [0, 1] or not a number, or thr == NULL: returns
 * AQUAHER_E_INVALID and sets the error message.
 */
int aquaher_threshold(double ratio, uint64_t* thr);

/*
 * HOST only, no device needed: the reward and termination code of the transition s -> s2 (normalised observations; words
 * 0 and 1 are read) replayed under the goal (gx, gy), as defined above -- the kernel's own code.  A NULL pointer: returns
 * AQUAHER_E_INVALID.
 */
int aquaher_reward(const float s[5], const float s2[5], float gx, float gy, float* r, uint8_t* d);

/*
 * The relabelling: one launch, one thread per sample.  All pointers are DEVICE pointers.
 *   header               : the ring's int64 [4] header, 8-byte aligned; word [0] (the cursor) is read, nothing is written
 *   s, a, r, s2, d, ok   : the ring's six rows, read only; ring_ld >= capacity, 1 <= capacity <= AQUAHER_MAX_CAPACITY
 *   action_kind          : AQUAHER_ACT_U8 or AQUAHER_ACT_F32X2, as in aquarpl_gather
 *   N                    : worlds per batched step, 1 <= N <= capacity and capacity % N == 0
 *   idx, P, B            : int32 [P][B] slots, 1 <= P <= AQUAHER_MAX_NETWORKS, 0 <= B <= AQUAHER_MAX_BATCH
 *   H                    : the horizon, 1 <= H <= AQUAHER_MAX_HORIZON
 *   ratio                : the share of the eligible samples to relabel, in [0, 1]
 *   t_dev                : uint64 [P], 8-byte aligned: the update counters (the draw is keyed by t_p + 1, as the minibatch
 *                          draw of the same iteration is)
 *   seed, seed_dev       : exactly one of them.  seed_dev == NULL: the scalar seed keys every row.  Otherwise seed must be
 *                          AQUAHER_NO_SEED and seed_dev is uint64 [P], 8-byte aligned: the bank's keys
 *   out_ld               : the pitch of the staged rows, >= P * B; sample (p, j) is position p * B + j
 *   out_s, out_s2        : float32 [5][out_ld];  out_r float32 [out_ld];  out_a uint8 [out_ld] or float32 [2][out_ld]
 *   out_d, out_ok        : uint8 [out_ld]: the termination code of the staged transition, and 1 for a sample
 *   out_k, out_m         : nullable uint8 [out_ld]: k + 1 of a relabelled sample (0: not relabelled), and M
 * B == 0 returns 0 without a launch.
 */
int aquaher_relabel(const int64_t* header, const float* s, const void* a, const float* r, const float* s2, const uint8_t* d,
                    const uint8_t* ok, int64_t ring_ld, int64_t capacity, int action_kind, int64_t N,
                    const int32_t* idx, int64_t P, int64_t B, int H, double ratio, const uint64_t* t_dev, uint64_t seed,
                    const uint64_t* seed_dev, float* out_s, void* out_a, float* out_r, float* out_s2, uint8_t* out_d,
                    uint8_t* out_ok, int64_t out_ld, uint8_t* out_k, uint8_t* out_m, void* stream);

#ifdef __cplusplus
}
#endif
#endif
