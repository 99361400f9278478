/*
 * aqua_bank.h -- C ABI of libaqua_bank.so: a BANK of the DQN's Q-networks (main/impl/dqn.py:301-314, 5 -> 64 ReLU ->
 * 64 ReLU -> 3) acting on one batch of worlds in a single launch on MI355X (gfx950).  Where aqua_policy.h evaluates one
 * network per launch, this evaluates network p on the p-th segment of the batch: the reference's test protocol
 * (main/plotting/dqn_test_plotter.py::run_tests: several policies, n_tests episodes each), the evaluation of every
 * checkpoint of a training, or the acting half of a population, without one launch per policy.
 *
 * Conventions are those of aqua_policy.h:
 *  - plain pointers and sizes only (streams are void*); every DEVICE buffer is owned by the caller and borrowed until
 *    the work queued on `stream` has run; the library allocates nothing and keeps no pointer.
 *  - aquabank_act_f32 is one asynchronous launch on `stream`: no allocation, no synchronisation, no host read, so it may
 *    be captured into a HIP graph.
 *  - return value: 0 = ok; > 0 = hipError_t; < 0 = AQUABANK_E_* (the values of AQUA_E_*).  aquabank_last_error() returns
 *    a thread-local message for the last failing call on this thread.
 *  - every argument is validated before the first HIP call.
 *  - there is no CPU path.
 *
 * The bank is float32 [networks][F] in DEVICE memory, 16-byte aligned, F = aquabank_weights_bytes() / 4 = 4804 floats
 * (19216 bytes, a multiple of 16: every slot is aligned when the bank is).  Slot p is, byte for byte, the blob that
 * aquapol_pack_weights() of aqua_policy.h writes for network p: that library stays the packer, and
 * aquabank_weights_bytes() == aquapol_weights_bytes().  Writing a new blob over a slot is how the weights of one network
 * are replaced, also under a captured graph (the DQN learner of aqua_learner.h re-packs into whatever blob it is given,
 * so it trains a slot in place).
 *
 * Numerics: those of aquapol_act_f32, to the bit (see "the contract" below).
 */
#ifndef AQUA_BANK_H
#define AQUA_BANK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQUABANK_ABI_VERSION 1

/* library error codes (negative): the values of AQUA_E_* in aqua_hip.h */
#define AQUABANK_E_INVALID   (-1)   /* bad argument (null pointer, size out of range ...) */
#define AQUABANK_E_ALIGN     (-2)   /* pointer not usable */
#define AQUABANK_E_NODEVICE  (-3)   /* no HIP device / wrong architecture */

/* the one architecture (dqn.py:301-314) and the Philox stream of the epsilon-greedy draws: aqua_policy.h's */
#define AQUABANK_INPUTS   5
#define AQUABANK_HIDDEN   64
#define AQUABANK_ACTIONS  3
#define AQUABANK_STREAM   5

#define AQUABANK_MAX_NETWORKS 65536

int aquabank_version(void);                 /* AQUABANK_ABI_VERSION */
const char* aquabank_last_error(void);

/* bytes of one slot of the bank: aquapol_weights_bytes() */
size_t aquabank_weights_bytes(void);

/*
 * HOST only, no device needed: the tiles of 32 worlds that aquabank_act_f32(.., seg, .., N, ..) evaluates -- a tile
 * belongs to one network, so a segment ends its last tile early.  With used = ceil(N / seg) networks holding a world,
 * that is (used - 1) * ceil(seg / 32) + ceil((N - (used - 1) * seg) / 32): at most N / 32 + used, whatever seg is.
 * N == 0: 0.  seg < 1 or N < 0: AQUABANK_E_INVALID.
 */
int64_t aquabank_items(int64_t seg, int64_t N);

/*
 * HOST only: the inverse of aquapol_pack_weights().  blob_host: one slot (aquabank_weights_bytes() bytes, 4-byte
 * aligned) copied back from the bank; k0 [5][64], k1 [64][64], k2 [64][3] receive the Keras kernels, row-major
 * [in][out]; b0 [64], b1 [64], b2 [3] the biases.  A pure permutation; the padding floats of the blob are not read.
 * A null pointer: AQUABANK_E_INVALID; a misaligned blob: AQUABANK_E_ALIGN.
 */
int aquabank_unpack_weights(const void* blob_host, float* k0, float* b0, float* k1, float* b1, float* k2, float* b2);

/*
 * Q-values and an action for global worlds [env_offset, env_offset + N); local world i in [0, N) is evaluated with
 * network i / seg.
 *   bank_dev        : the bank (above), 16-byte aligned.
 *   networks, seg   : 1 <= networks <= AQUABANK_MAX_NETWORKS slots; seg >= 1 worlds per network; N <= networks * seg
 *                     (checked without overflow).  A network whose segment starts at or beyond N does nothing, a segment
 *                     that N cuts is evaluated up to N.  The work of a launch follows N, not seg: it walks
 *                     aquabank_items(seg, N) tiles of 32 worlds, so one network with a huge seg ("this network for
 *                     whatever batch comes") costs what N worlds cost.
 *   in, ld          : float32 rows of ld >= N elements, 4-byte aligned.
 *                     in_is_normalised == 0: the environment's state rows x, y, theta, goal_x, goal_y (aqua_hip.h; rows
 *                     5.. are not read), normalised in the kernel as the step kernels' obs_norm epilogue does;
 *                     in_is_normalised != 0: float32 [5][ld] holding the networks' input as it is.
 *   epsilon         : used when epsilon_dev is NULL.  0 -> greedy: argmax_a Q[a], the LOWEST index on an exact tie; no
 *                     draw.  > 0 -> r = Philox4x32-10(key = seed, counter = (env_offset + i, tick + *tick_base_dev),
 *                     stream AQUABANK_STREAM, attempt 0) in the counter layout of aqua_hip.h's draws; the world explores
 *                     iff (r[0] >> 8) * 2^-24 < epsilon (float32) and then takes ((r[1] >> 8) * 3) >> 24.  NaN or
 *                     negative: AQUABANK_E_INVALID (also when epsilon_dev is given).
 *   epsilon_dev     : nullable DEVICE float32 [networks], 4-byte aligned: epsilon of network p is epsilon_dev[p], read on
 *                     the device when the kernel runs (a schedule can live there under a graph).  The host cannot
 *                     validate it: an entry that is NaN or negative NEVER explores (its segment is greedy); +infinity and
 *                     anything >= 1 always explore.
 *   tick_base_dev   : nullable device uint64 added to tick on the device (the environment's graph tick base).
 *   action          : uint8 [N]                                             |
 *   q, q_ld         : float32 [3][q_ld], q_ld >= N                          |  each nullable, at least one non-null
 *   q_taken         : float32 [N], Q of the action written                  |
 * N == 0 returns 0 without a launch.  Worlds beyond N are neither read nor written.
 *
 * The contract.  For every network p with p * seg < N, what this call writes for the worlds of segment p is bit for bit
 * what
 *   aquapol_act_f32(bank_dev + p * aquabank_weights_bytes(), in + p * seg, ld, in_is_normalised,
 *                   min(seg, N - p * seg), env_offset + p * seg, eps_p, seed, tick, tick_base_dev,
 *                   action + p * seg, q + p * seg, q_ld, q_taken + p * seg, stream)
 * writes, eps_p = epsilon_dev ? epsilon_dev[p] : epsilon (greedy where that is NaN or negative): the same fused
 * multiply-add chains in the same order, the same normalisation, the lowest index on a tie, the same draw.  Results do
 * not depend on networks, seg, N, the launch shape or the device.
 */
int aquabank_act_f32(const void* bank_dev, int64_t networks, int64_t seg,
                     const float* in, int64_t ld, int in_is_normalised, int64_t N, int64_t env_offset,
                     float epsilon, const float* epsilon_dev,
                     uint64_t seed, uint64_t tick, const uint64_t* tick_base_dev,
                     uint8_t* action, float* q, int64_t q_ld, float* q_taken, void* stream);

#ifdef __cplusplus
}
#endif
#endif
