/*
 * aqua_segments.h -- C ABI of libaqua_segments.so: episode statistics and epsilon schedules for the SEGMENTS of a batch of
 * worlds on MI355X (gfx950).  A segment is the worlds of one network of a bank (aqua_bank.h): segment p owns the worlds
 * [env_offset + p * seg, env_offset + (p + 1) * seg).
 *
 * Reference being replaced: the bookkeeping of main/impl/dqn.py for ONE training -- epsilon = max(epsilon * decay, final)
 * once per finished episode (dqn.py:139-141,184) and mean_last_100 of reward and success (dqn.py:196-198) -- kept once per
 * segment, for P trainings on one batch.
 *
 * The library does not account steps.  It consumes the records aquaep_after_step_f32 (aqua_episodes.h) has just appended
 * to its log and keeps a cursor of its own, `seen`.  Contract: ONE call after every accounting call.
 *
 * Conventions are those of aqua_episodes.h:
 *  - plain pointers and sizes only (streams are void*); every DEVICE buffer is owned by the caller and borrowed until the
 *    work queued on `stream` has run; the library allocates nothing and keeps no pointer.  ALL state is device memory.
 *  - the entry is asynchronous on `stream`: no allocation, no synchronisation, no host read, so it may be captured into a
 *    HIP graph.  It is ONE launch.
 *  - return value: 0 = ok; > 0 = hipError_t; < 0 = AQUASEG_E_* (the values of AQUA_E_*).
 *  - every argument is validated before the first HIP call.  There is no CPU path.
 *
 * Launch structure: one wavefront per segment, 256-thread blocks, ceil(P / 4) <= 1024 blocks.  No block waits on another
 * block.  Thread 0 of a block reads `seen` and counts[0] and hands them to its four wavefronts through LDS; behind that
 * barrier it takes a ticket (one integer atomic on header[3]).  The block that takes the last ticket knows that every
 * block has read `seen`; it alone writes seen = counts[0] (and missed), and puts the ticket back to 0.  A wavefront finds
 * its run of the new records with two searches over the record index (64 probes per round: one round up to 64 new
 * records) and leaves when the run is empty.  No floating-point atomics; every sum has a fixed order (below): the same
 * inputs give the same bits run to run, eager or replayed from a graph.
 */
#ifndef AQUA_SEGMENTS_H
#define AQUA_SEGMENTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQUASEG_ABI_VERSION 1

/* library error codes (negative): the values of AQUA_E_* in aqua_hip.h */
#define AQUASEG_E_INVALID   (-1)   /* bad argument (null pointer, negative size, value out of range ...) */
#define AQUASEG_E_ALIGN     (-2)   /* pointer not usable */
#define AQUASEG_E_NODEVICE  (-3)   /* no HIP device / wrong architecture */

#define AQUASEG_MAX_WORLDS   1073741824   /* N and seg at most (2^30: AQUAEP_MAX_WORLDS) */
#define AQUASEG_MAX_SEGMENTS 4096         /* P at most (AQUALBANK_MAX_NETWORKS) */
#define AQUASEG_MAX_WINDOW   1024         /* W at most */
#define AQUASEG_HEADER       4            /* uint64 slots of header[] */
#define AQUASEG_COUNTS       8            /* uint64 slots of a row of seg_counts[][] */

int aquaseg_version(void);                /* AQUASEG_ABI_VERSION */
const char* aquaseg_last_error(void);

/*
 * Account the records one aquaep_after_step_f32 call has appended.  All pointers are DEVICE pointers.
 *   log_ret, log_len, log_code, log_world, C, counts
 *                  : the episode log of aqua_episodes.h (float32 / int32 / uint8 / int64 [C], C >= N, C >= 1) and its
 *                    counters uint64 [8], of which counts[0] is the log cursor; all read only.
 *   env_offset     : global index of the first world of segment 0 (>= 0)
 *   N              : worlds of the batch, in [0, AQUASEG_MAX_WORLDS]: one accounting call appends at most N records
 *   seg            : worlds per segment, in [1, AQUASEG_MAX_WORLDS].  P * seg may exceed N: the last segment then holds
 *                    fewer worlds.
 *   P              : segments, in [0, AQUASEG_MAX_SEGMENTS]
 *   W              : slots of a segment's window, in [1, AQUASEG_MAX_WINDOW]
 *   header         : uint64 [AQUASEG_HEADER], 8-byte aligned: [0] seen, the log cursor up to which records are accounted;
 *                    [1] missed; [2] stray; [3] the ticket, 0 between calls.
 *   seg_counts     : uint64 [P][AQUASEG_COUNTS]: [0] episodes of the segment (also its window cursor), [1..3] episodes by
 *                    termination code 1..3, [4] steps of its finished episodes (the sum of log_len); the rest is not touched.
 *   hyper          : float64 [P][2] = (decay, eps_final) of the segment, read only; 0 < decay <= 1 and eps_final >= 0 are the
 *                    caller's to validate before the upload.  Read only when the schedule is on (may be NULL otherwise).
 *   eps_state, eps_out
 *                  : float64 [P] schedule state and float32 [P] copy published for the bank; both NULL switches the
 *                    schedule off (exactly one NULL: AQUASEG_E_INVALID).
 *   win_ret, win_len, win_code
 *                  : float32 / int32 / uint8 [P][W], the window rings.
 *   mean_ret, mean_len, success
 *                  : float32 [P], the published statistics of the window.
 *
 * The call processes the n = counts[0] - seen new records, record k = 0..n-1 in log slot (seen + k) % C, and then sets
 * seen = counts[0].  The records of one accounting call ascend in world index, so those of segment p are one contiguous
 * run of k.  If n > N the caller has skipped calls: nothing is processed, missed += 1, and seen = counts[0] all the same.
 * A record whose world lies outside [env_offset, env_offset + P * seg) belongs to no segment: it is skipped and stray += 1.
 *
 * Segment p with m new records j = 0..m-1 in log order and c = seg_counts[p][0] before the call; m == 0 writes nothing.
 *   window:   record j goes to slot (c + j) % W of the segment's rings; of m > W records only the last W are stored.
 *   counters: seg_counts[p][0] += m, [code] += its share for code 1..3, [4] += the sum of the m lengths.
 *   schedule: aqua_episodes.h's, m in place of n: q = decay^m in float64 by binary exponentiation, least-significant bit
 *             first; eps_state[p] = max(eps_state[p] * q, eps_final); eps_out[p] = (float)eps_state[p].
 *   statistics over the k = min(c + m, W) occupied slots 0..k-1 after the call:
 *             success[p]  = (float)((double)(slots with code 3) / (double)k), the count an integer;
 *             mean_len[p] = (float)((double)(sum of the k lengths) / (double)k), the sum an integer (exact);
 *             mean_ret[p] = (float)(S / (double)k) with S a float64 sum in this order: lane l = 0..63 adds the returns of
 *                           the slots l, l + 64, l + 128, ... < k in ascending order to 0.0, each converted to float64; then
 *                           the 64 lane sums are added to 0.0 in ascending lane order.
 *             A slot written in this call takes its value from the log record, never from the ring in memory.
 * N == 0 or P == 0 returns 0 without a launch.
 */
int aquaseg_account(const float* log_ret, const int32_t* log_len, const uint8_t* log_code, const int64_t* log_world, int64_t C,
                    const uint64_t* counts, int64_t env_offset, int64_t N, int64_t seg, int64_t P, int64_t W,
                    uint64_t* header, uint64_t* seg_counts, const double* hyper, double* eps_state, float* eps_out,
                    float* win_ret, int32_t* win_len, uint8_t* win_code, float* mean_ret, float* mean_len, float* success,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
