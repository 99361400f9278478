/*
 * aqua_ens.h -- C ABI of libaqua_ens.so: the ENSEMBLE POLICY of a bank of the DQN's Q-networks (main/impl/dqn.py:301-314,
 * 5 -> 64 ReLU -> 64 ReLU -> 3) in a single launch on MI355X (gfx950).  Every member network of the bank evaluates EVERY
 * world of the batch, and the answers are reduced on the device to one action per world: by the mean of Q or by
 * majority vote, with the across-network variance of Q and the vote counts as optional outputs.  (aquabank_act_f32
 * evaluates network p on the p-th SEGMENT of the worlds; aquaqmap_maps_f32 evaluates every network on a synthetic grid.)
 *
 * This header lies beside the source (the listings of include/ and of the package's include/ are pinned by tests).
 *
 * Conventions are those of aqua_bank.h:
 *  - plain pointers and sizes only (streams are void*); every DEVICE buffer is owned by the caller and borrowed until
 *    the work queued on `stream` has run; the library allocates nothing and keeps no pointer.
 *  - aquaens_act_f32 is one asynchronous launch on `stream`: no allocation, no synchronisation, no host read, no
 *    atomic, so it may be captured into a HIP graph; the same inputs give the same bits.
 *  - return value: 0 = ok; > 0 = hipError_t; < 0 = AQUAENS_E_* (the values of AQUA_E_*).  aquaens_last_error() returns
 *    a thread-local message for the last failing call on this thread; it names the argument that was wrong.
 *  - every argument is validated before the first HIP call.
 *  - there is no CPU path.
 *
 * THE CONTRACT of aquaens_act_f32.
 *
 *  - bank_dev is a QNetworkBank's tensor: float32 [networks][F] in DEVICE memory, 16-byte aligned, F =
 *    aquaens_weights_bytes() / 4; slot p is byte for byte the blob of aquapol_pack_weights().  It is read when the kernel
 *    runs, with no copy: a load, a learner update or a selection queued before the launch (or the replay) is seen.
 *  - member_dev is a nullable DEVICE uint8 [networks].  Network p is a MEMBER iff member_dev == NULL or
 *    member_dev[p] != 0.  It is read on the device when the kernel runs, so a mask written by an earlier node of a graph
 *    is the one used.  It must not change WHILE the launch runs: a wavefront reads it again for every group of worlds it
 *    takes, so a mask rewritten concurrently (from another stream, say) may give different worlds different members.
 *    M is the number of members.
 *  - Every world i in [0, N) is evaluated by EVERY member.  Q_p(i)[c] is, bit for bit, what aquapol_act_f32 on slot p
 *    writes into q for that world and input form: the one forward<RAW> of csrc/aqua_qnet.hpp, the same normalisation
 *    for in_is_normalised == 0.
 *  - The sums are in double and run over the members IN ASCENDING SLOT ORDER.  They are sequential: one rounded double
 *    add per member, no tree, no fused multiply-add (#pragma clang fp contract(off) around all of it):
 *        S1[c] = sum_p double(Q_p[c])        S2[c] = sum_p double(Q_p[c]) * double(Q_p[c])
 *    The product is exact in double.
 *  - Qbar[c] = float32(S1[c] / M): one double division, rounded once to float32.
 *  - variance[c * x_ld + i] = float32(max(S2[c] / M - (S1[c] / M) * (S1[c] / M), 0)), all of it in double: the
 *    POPULATION variance -- the variance and not its square root, on purpose, so that a numpy model gives the same bits.
 *  - votes[c * x_ld + i] is the number of members whose own arg-max is c; that arg-max takes the lowest index on a tie,
 *    as the policy's pick does.
 *  - The greedy action depends on `mode`:
 *        AQUAENS_MEAN  arg-max of Qbar, the lowest index on a tie;
 *        AQUAENS_VOTE  the action with the most votes; among equal counts the larger Qbar[c] as float32; still equal,
 *                      the lowest index.
 *  - epsilon-greedy is exactly the policy's draw: one Philox draw per world at (seed, env_offset + i,
 *    tick + *tick_base_dev) on stream AQUAENS_STREAM, the same threshold test and the same random action.  epsilon_dev
 *    is a nullable DEVICE float32 [1] that replaces `epsilon`, read when the kernel runs; a NaN or a negative value there
 *    never explores, by its bits, as in the bank.  `epsilon` itself must be >= 0 (NaN or negative: AQUAENS_E_INVALID).
 *  - q [3][q_ld] receives Qbar, q_taken [N] receives Qbar[action], action [N] the action.
 *  - M == 0 (an all-zero mask): Qbar = 0, variance 0, votes 0, greedy action 0.  A draw may still replace it.
 *  - M == 1 with member p: action, q and q_taken are bit for bit those of aquapol_act_f32 on slot p, epsilon-greedy
 *    included.  The variance is 0 and votes is the one-hot of the member's arg-max.
 *  - Results do not depend on `networks` beyond the members, on AQUAENS_GROUP, on the launch shape or on the device.
 *  - Worlds at or beyond N are neither read nor written.
 *  - At least one of action, q, q_taken, variance, votes is non-null; x_ld >= N when variance or votes is given, q_ld >= N
 *    when q is, ld >= N always; 1 <= networks <= AQUAENS_MAX_NETWORKS; env_offset >= 0; an unknown mode is
 *    AQUAENS_E_INVALID.  None of these checks forms a product: they cannot overflow.
 *  - bank_dev 16-byte aligned; in, q, q_taken, variance, votes and epsilon_dev 4-byte, tick_base_dev 8-byte aligned
 *    (AQUAENS_E_ALIGN).
 *  - N == 0 returns 0 without a launch (and needs no device).
 *
 * `in` is float32 [5][ld] (in_is_normalised != 0: the network's input) or [>= 5][ld] state rows of the environment
 * (in_is_normalised == 0: normalised in the kernel), as aquapol_act_f32 takes it.
 */
#ifndef AQUA_ENS_H
#define AQUA_ENS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQUAENS_ABI_VERSION 1

/* library error codes (negative): the values of AQUA_E_* in aqua_hip.h */
#define AQUAENS_E_INVALID   (-1)   /* bad argument (null pointer, size out of range ...) */
#define AQUAENS_E_ALIGN     (-2)   /* pointer not usable */
#define AQUAENS_E_NODEVICE  (-3)   /* no HIP device / wrong architecture */

#define AQUAENS_STREAM 5            /* the policy's draws: aqua_policy.h's stream, no new one */
#define AQUAENS_ACTIONS 3
#define AQUAENS_MAX_NETWORKS 65536  /* AQUABANK_MAX_NETWORKS */
#define AQUAENS_MEAN 0
#define AQUAENS_VOTE 1
/* T: the tiles of 32 consecutive worlds a wavefront carries through the member loop.  A member's operands (19.2 KB per
   wavefront) are loaded once per member and GROUP, not once per member and tile */
#define AQUAENS_GROUP 4

int aquaens_version(void);                  /* AQUAENS_ABI_VERSION */
const char* aquaens_last_error(void);

/* bytes of one slot of the bank: aquapol_weights_bytes() */
size_t aquaens_weights_bytes(void);

/*
 * HOST only, no device needed: the launch aquaens_act_f32 makes for N worlds on a device of `cus` compute units.
 *   out[0] = blocks of 256 threads (four wavefronts): min(ceil(groups / 4), 2 * cus), all resident
 *   out[1] = groups of AQUAENS_GROUP tiles: ceil(N / (32 * AQUAENS_GROUP))
 *   out[2] = the most groups one wavefront takes: ceil(groups / (4 * blocks)); wavefront w of the grid takes groups
 *            w, w + 4 * blocks, ...
 * N == 0: all three are 0.  N < 0, cus < 1 or out == NULL: AQUAENS_E_INVALID.
 */
int aquaens_shape(int64_t N, int cus, int64_t out[3]);

/* The ensemble's actions for N worlds: the contract above. */
int aquaens_act_f32(const void* bank_dev, int64_t networks, const uint8_t* member_dev, int mode,
                    const float* in, int64_t ld, int in_is_normalised, int64_t N, int64_t env_offset,
                    float epsilon, const float* epsilon_dev,
                    uint64_t seed, uint64_t tick, const uint64_t* tick_base_dev,
                    uint8_t* action, float* q, int64_t q_ld, float* q_taken,
                    float* variance, int32_t* votes, int64_t x_ld, void* stream);

#ifdef __cplusplus
}
#endif
#endif
