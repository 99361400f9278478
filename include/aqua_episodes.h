/*
 * aqua_episodes.h -- C ABI of libaqua_episodes.so: episode accounting for a batch of worlds on MI355X (gfx950), next to the
 * batched environment of aqua_hip.h, the Q-network of aqua_policy.h and the learner of aqua_learner.h.
 *
 * Reference being replaced: the bookkeeping of the training loop, main/impl/dqn.py:151-200 (episode_reward, episode_steps,
 * reward_list, success_list, epsilon = max(epsilon * decay, final) once per finished episode, dqn.py:139-141,184) and of
 * Policy.test / TestPlotter.run_tests (main/testing/__init__.py:17-36: Reward and Success of one episode per run).
 *
 * Conventions are those of aqua_learner.h:
 *  - plain pointers and sizes only (streams are void*); every DEVICE buffer is owned by the caller and borrowed until
 *    the work queued on `stream` has run; the library allocates nothing and keeps no pointer.  ALL state is device
 *    memory of the caller: nothing lives on the host, so a captured graph replays correctly.
 *  - every entry is asynchronous on `stream`: no allocation, no synchronisation, no host read, so it may be captured
 *    into a HIP graph.  The accounting call is TWO launches, the exploration pass ONE.
 *  - return value: 0 = ok; > 0 = hipError_t; < 0 = AQUAEP_E_* (the values of AQUA_E_*).  The last-error entry returns a
 *    thread-local message for the last failing call on this thread.
 *  - every argument is validated before the first HIP call.  There is no CPU path.
 *
 * Launch structure of the accounting call (no block ever waits on another block; order comes from stream order):
 *   1. account: block b owns the worlds [b * chunk, (b + 1) * chunk) -- chunk a function of N alone, at most
 *      AQUAEP_MAX_BLOCKS blocks.  It accumulates return and length of the counted worlds, counts the ending ones with
 *      one ballot and popcount per wavefront, stores its count in the workspace and adds its shares to counts[]
 *      (integer atomics).
 *   2. scatter: a block with a non-zero count sums the counts of the blocks below it (its offset) and of all blocks
 *      (n; the log cursor before the call is counts[0] - n), then walks its worlds in index order: ballot, rank of
 *      the lane below it, prefix of the wavefronts through LDS, one record per ending world, return and length back
 *      to 0.  Block 0 also advances the epsilon schedule by n.
 * No floating-point atomics and no reassociated sums: the same inputs give the same bits run to run, eager or
 * replayed from a graph, whatever the launch shape.
 */
#ifndef AQUA_EPISODES_H
#define AQUA_EPISODES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQUAEP_ABI_VERSION 1

/* library error codes (negative): the values of AQUA_E_* in aqua_hip.h */
#define AQUAEP_E_INVALID   (-1)   /* bad argument (null pointer, negative size, value out of range ...) */
#define AQUAEP_E_ALIGN     (-2)   /* pointer not usable */
#define AQUAEP_E_NODEVICE  (-3)   /* no HIP device / wrong architecture */

#define AQUAEP_MAX_WORLDS  1073741824    /* worlds per call (2^30) */
#define AQUAEP_MAX_BLOCKS  1024          /* blocks of the two accounting launches at most */
#define AQUAEP_COUNTS      8             /* uint64 slots of counts[] */

/* Philox stream of the exploration draws: the policy's (AQUAPOL_STREAM), so that the pass reproduces its draw */
#define AQUAEP_STREAM      5

int aquaep_version(void);                 /* AQUAEP_ABI_VERSION */
const char* aquaep_last_error(void);

/* bytes of DEVICE workspace the accounting of N worlds needs (non-decreasing in N; 0 for N outside [0, AQUAEP_MAX_WORLDS]) */
size_t aquaep_workspace_bytes(int64_t N);

/*
 * One batched step's accounting.  All pointers are DEVICE pointers.
 *   reward, term, time : float32 [N], uint8 [N], int32 [N] (nullable) as the step kernels left them; read only.
 *   env_offset         : global index of world 0 (>= 0)
 *   ret, len           : float32 [N], int32 [N]: running return and length; read and written.
 *   finished           : nullable uint8 [N].  Non-null selects ONCE mode: a world that has logged an episode is ignored from
 *                        then on (one episode per run: Policy.test / run_tests on a batch without restarts).
 *   log_ret, log_len, log_code, log_world, C
 *                      : float32 / int32 / uint8 / int64 [C], the episode log, a ring; C >= N.  log_world is env_offset + i.
 *   counts             : uint64 [AQUAEP_COUNTS], 8-byte aligned: [0] episodes logged so far (also the log cursor), [1..3]
 *                        episodes by termination code 1..3 (a code above 3 is logged and counted in [0] only), [4] world-steps
 *                        counted; the rest is not touched.
 *   eps_state, eps_out : float64 [1] schedule state and float32 [1] copy published for the policy; both NULL switches the
 *                        schedule off (exactly one NULL: AQUAEP_E_INVALID).
 *   decay, eps_final   : 0 < decay <= 1, 0 <= eps_final, both numbers (otherwise AQUAEP_E_INVALID).
 *   workspace          : 16-byte aligned, at least aquaep_workspace_bytes(N) bytes; contents need not be kept or cleared.
 *
 * World i is COUNTED iff (finished == NULL || finished[i] == 0) && (time == NULL || term[i] != 0 || time[i] >= 0): in
 * next-step restart mode a world that is being restarted or awaits its restart reports reward 0 / term 0 and carries a
 * negative marker in time[] (aqua_hip.h); that tick belongs to no episode.
 *   counted:  ret[i] = ret[i] + reward[i] (one float32 add); len[i] += 1; counts[4] += 1.
 *   counted and term[i] != 0: one record (ret[i], len[i], term[i], env_offset + i); then ret[i] = 0, len[i] = 0 and, in once
 *       mode, finished[i] = 1.  The n worlds ending in this call take the slots (counts[0] + rank) % C, rank = number of
 *       ending worlds with a lower i.  Then counts[0] += n and counts[code] += its share.
 *   schedule: p = decay^n in float64 by binary exponentiation, least-significant bit first (result = 1, base = decay; while
 *       n: if n & 1: result *= base; base *= base; n >>= 1); eps_state = max(eps_state * p, eps_final); *eps_out =
 *       (float)eps_state.  That is dqn.py:184 applied n times, up to the rounding of the product.
 * N == 0 returns 0 without a launch.
 */
int aquaep_after_step_f32(const float* reward, const uint8_t* term, const int32_t* time, int64_t env_offset, int64_t N,
                          float* ret, int32_t* len, uint8_t* finished,
                          float* log_ret, int32_t* log_len, uint8_t* log_code, int64_t* log_world, int64_t C,
                          uint64_t* counts, double* eps_state, float* eps_out, double decay, double eps_final,
                          void* workspace, size_t workspace_bytes, void* stream);

/*
 * Exploration pass over greedy actions with a DEVICE-resident epsilon.  For world i it takes the draw the policy kernel takes:
 * Philox4x32-10(key = seed, counter = (env_offset + i, tick + *tick_base_dev), stream AQUAEP_STREAM, attempt 0) in the counter
 * layout of aqua_hip.h's draws; if u01(r[0]) < *eps_dev it overwrites action[i] with ((r[1] >> 8) * 3) >> 24.  The draw does not
 * depend on Q, so a greedy act of aqua_policy.h (epsilon = 0) followed by this pass equals its act with epsilon = *eps_dev bit
 * for bit.  q_taken written by the greedy call is then STALE for the explored worlds: it is the greedy action's Q-value.
 *   action        : uint8 [N], read and written
 *   eps_dev       : float32 [1], 4-byte aligned, a number >= 0 (0: nothing is overwritten)
 *   tick_base_dev : nullable uint64 [1], 8-byte aligned
 * N == 0 returns 0 without a launch.
 */
int aquaep_explore_u8(uint8_t* action, int64_t N, int64_t env_offset, const float* eps_dev, uint64_t seed, uint64_t tick,
                      const uint64_t* tick_base_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
