/*
 * aqua_replay.h -- C ABI of libaqua_replay.so: the experience ring of a batch of worlds with its cursor and size in DEVICE
 * memory, on MI355X (gfx950), next to the batched environment of aqua_hip.h, the Q-network of aqua_policy.h, the learner
 * of aqua_learner.h and the episode accounting of aqua_episodes.h.
 *
 * Reference being replaced: the DQN's experience buffer, main/impl/dqn.py:174 (`exp_buffer.append([state, pred_action,
 * reward, next_state, done])`) and its sampler, dqn.py:251-260 (`random.sample` + `np.vstack`).  aqua_ring_write_f32/u8 of
 * aqua_hip.h take the cursor by value and aqualrn_update_f32 the size: a captured graph would write the same slots and
 * draw from the same prefix at every replay.  Here both live in a header the kernels read and advance, so one training
 * iteration -- act, explore, open, step, close, account, draw, update -- replays correctly from one graph.
 *
 * Conventions are those of aqua_episodes.h:
 *  - plain pointers and sizes only (streams are void*); every DEVICE buffer is owned by the caller and borrowed until
 *    the work queued on `stream` has run; the library allocates nothing and keeps no pointer.  ALL state is device
 *    memory of the caller: nothing lives on the host.
 *  - every entry is asynchronous on `stream` and ONE launch: no allocation, no synchronisation, no host read, so it may
 *    be captured into a HIP graph.
 *  - return value: 0 = ok; > 0 = hipError_t; < 0 = AQUARPL_E_* (the values of AQUA_E_*).  The last-error entry returns a
 *    thread-local message for the last failing call on this thread.
 *  - every argument is validated before the first HIP call.  There is no CPU path.
 *
 * The header: int64 [AQUARPL_HEADER_WORDS], 8-byte aligned.
 *   [0] cursor: the next slot, in [0, capacity)          [1] size: filled slots, <= capacity
 *   [2] first slot of the batch opened last               [3] batches closed
 * The header rule: no thread reads a word that another thread of the same launch writes.  open reads [0] and stores [2];
 * close reads [2] and stores [0], [1], [3] (the one lane that stores [1] and [3] is the only one that reads them); draw
 * reads [1]; gather reads none.  Order between launches is stream order and nothing else: no block waits on another, no
 * fence, no atomics.  The kernels copy and draw integers: no floating-point arithmetic, the same bits eager or replayed.
 *
 * The rows are ReplayRing's, so aqualrn_update_f32 reads them unchanged (ring_ld is the row pitch in elements):
 *   s, s2 float32 [5][ring_ld]; r float32 [ring_ld]; a uint8 [ring_ld] or float32 [2][ring_ld]; d, ok uint8 [ring_ld].
 * Sizes: 0 <= N <= capacity <= AQUARPL_MAX_CAPACITY (the learner's ld bound), capacity <= ring_ld.  World indices and
 * slots are 64-bit.  World i of a batch lands in slot base + i, minus capacity once if that is >= capacity.
 */
#ifndef AQUA_REPLAY_H
#define AQUA_REPLAY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQUARPL_ABI_VERSION 1

/* library error codes (negative): the values of AQUA_E_* in aqua_hip.h */
#define AQUARPL_E_INVALID   (-1)   /* bad argument (null pointer, negative size, value out of range ...) */
#define AQUARPL_E_ALIGN     (-2)   /* pointer not usable */
#define AQUARPL_E_NODEVICE  (-3)   /* no HIP device / wrong architecture */

#define AQUARPL_HEADER_WORDS  4
#define AQUARPL_MAX_CAPACITY  2147483647   /* slots: INT32_MAX, so that a slot fits the learner's int32 idx */
#define AQUARPL_MAX_BATCH     1048576      /* samples per draw / gather: AQUALRN_MAX_BATCH */
#define AQUARPL_MAX_BLOCKS    2048         /* blocks of AQUARPL_BLOCK threads per launch at most (grid-stride above that) */
#define AQUARPL_BLOCK         256
#define AQUARPL_ATTEMPTS      4            /* draws per sample before it is given up (-1): the learner's */

/* Philox stream of the minibatch draws: the learner's (AQUALRN_STREAM), so that the draw reproduces its own */
#define AQUARPL_STREAM        6

/* what the action rows hold */
#define AQUARPL_ACT_U8        0    /* uint8 [N] -> a uint8 [ring_ld] */
#define AQUARPL_ACT_F32X2     1    /* float32 [2][action_ld] -> a float32 [2][ring_ld] */

int aquarpl_version(void);                 /* AQUARPL_ABI_VERSION */
const char* aquarpl_last_error(void);

/*
 * Before the step: (s, a, ok) of the N transitions about to be made.  All pointers are DEVICE pointers.
 *   header               : read [0], store [2] = [0]
 *   s, a, ok             : the ring's rows, written in the slots of this batch only
 *   obs, obs_ld          : float32 [5][obs_ld] normalised observations (main/impl/utils.py:15-33), obs_ld >= N
 *   action, action_kind, action_ld
 *                        : AQUARPL_ACT_U8: uint8 [N] (action_ld ignored); AQUARPL_ACT_F32X2: float32 [2][action_ld >= N]
 *   time                 : nullable int32 [N], the environment's time markers (aqua_hip.h).  ok = time == NULL ||
 *                          time[i] >= 0 || time[i] <= -3: a world that is about to be restarted instead of stepped
 *                          (next-step mode, markers -1 and -2) makes no experience.
 * A cursor outside [0, capacity) writes no row (it is never used as an address); [2] still receives it, so that the close
 * that follows does nothing either.  N == 0 returns 0 without a launch (in close as well: the header stays as it was).
 */
int aquarpl_open(int64_t* header, float* s, void* a, uint8_t* ok, int64_t ring_ld, int64_t capacity,
                 const float* obs, int64_t obs_ld, const void* action, int action_kind, int64_t action_ld,
                 const int32_t* time, int64_t N, void* stream);

/*
 * After the step: (r, s', d) into the slots of the batch opened last, then the header moves on.
 *   header               : read [2] (the base); store [0] = (base + N) mod capacity, [1] = min(capacity, [1] + N), [3] += 1
 *   r, s2, d             : the ring's rows
 *   reward, term         : float32 [N], uint8 [N] as the step kernels left them;  obs, obs_ld: as above, after the step
 * A base outside [0, capacity) writes nothing and leaves the header as it was; it is never used as an address.
 */
int aquarpl_close(int64_t* header, float* r, float* s2, uint8_t* d, int64_t ring_ld, int64_t capacity,
                  const float* reward, const float* obs, int64_t obs_ld, const uint8_t* term, int64_t N, void* stream);

/*
 * The minibatch draw of aqualrn_update_f32(idx == NULL) for the update that takes *t_dev to *t_dev + 1, with the size read
 * from the device: for sample j < B, attempt a = 0 .. AQUARPL_ATTEMPTS - 1: r = Philox4x32-10(key = seed, counter = (j,
 * *t_dev + 1), stream AQUARPL_STREAM, attempt a), c = (uint64(r[0]) * size) >> 32; the first c with c < size and ok[c] != 0
 * is idx[j]; none: idx[j] = -1.  size is header[1] clamped to [0, capacity].
 *   header : read [1];  ok: uint8 [>= capacity];  t_dev: uint64 [1], 8-byte aligned, read only;  idx: int32 [B], written
 * Calling aqualrn_update_f32 with this idx and size = capacity then performs the update it would have performed with
 * idx == NULL and the true size: a slot never written has ok == 0.  B == 0 returns 0 without a launch.
 */
int aquarpl_draw(const int64_t* header, const uint8_t* ok, int64_t capacity, const uint64_t* t_dev, uint64_t seed,
                 int32_t* idx, int64_t B, void* stream);

/*
 * Dense, fixed-shape minibatch rows for a learner written elsewhere (dqn.py:251-260).
 *   idx, B                 : int32 [B] slots
 *   s, a, r, s2, d, ok     : the ring's rows, read only; action_kind as above
 *   out_s, out_s2          : float32 [B][5];  out_r float32 [B];  out_a uint8 [B] or float32 [B][2]
 *   out_done, out_valid    : uint8 [B]: d != 0, and 1 for a sample that exists
 * A sample with idx outside [0, capacity) or ok[idx] == 0 gives zero rows and valid = 0; such an idx is never used as an
 * address.  B == 0 returns 0 without a launch.
 */
int aquarpl_gather(const int32_t* idx, int64_t B, const float* s, const void* a, const float* r, const float* s2,
                   const uint8_t* d, const uint8_t* ok, int64_t ring_ld, int64_t capacity, int action_kind,
                   float* out_s, void* out_a, float* out_r, float* out_s2, uint8_t* out_done, uint8_t* out_valid,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
