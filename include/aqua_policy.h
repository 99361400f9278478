/*
 * aqua_policy.h -- C ABI of libaqua_policy.so: the DQN's Q-network evaluated on MI355X (gfx950) next to the batched
 * environment of aqua_hip.h.
 *
 * Reference being replaced: the Keras model of main/impl/dqn.py:301-314 (5 inputs -> 64 ReLU -> 64 ReLU -> 3 linear
 * outputs), its greedy use in main/testing/test_dqn.py:14-22 and its epsilon-greedy use in dqn.py:212-228.  Exactly this
 * architecture: anything else is rejected by aquapol_pack_weights().
 *
 * Conventions are those of aqua_hip.h:
 *  - plain pointers and sizes only (streams are void*); every DEVICE buffer is owned by the caller and borrowed until
 *    the work queued on `stream` has run; the library allocates nothing and keeps no pointer.
 *  - aquapol_act_f32 is one asynchronous launch on `stream`: no allocation, no synchronisation, no host read, so it may
 *    be captured into a HIP graph.
 *  - return value: 0 = ok; > 0 = hipError_t; < 0 = AQUAPOL_E_* (the values of AQUA_E_*).  aquapol_last_error() returns a
 *    thread-local message for the last failing call on this thread.
 *  - every argument is validated before the first HIP call.
 *
 * Numerics: float32 throughout.  Every unit is one fused-multiply-add chain over its inputs in a fixed order with the
 * bias as the initial value (one rounding per term, no reduced-precision operand anywhere); the three outputs add two
 * such chains of 32 terms.  Results are deterministic and independent of N, of the launch shape and of which of the two
 * input forms is used.
 */
#ifndef AQUA_POLICY_H
#define AQUA_POLICY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQUAPOL_ABI_VERSION 1

/* library error codes (negative): the values of AQUA_E_* in aqua_hip.h */
#define AQUAPOL_E_INVALID   (-1)   /* bad argument (null pointer, negative size, other architecture ...) */
#define AQUAPOL_E_ALIGN     (-2)   /* pointer not usable */
#define AQUAPOL_E_NODEVICE  (-3)   /* no HIP device / wrong architecture */

/* the one architecture (dqn.py:301-314) */
#define AQUAPOL_INPUTS   5
#define AQUAPOL_HIDDEN   64
#define AQUAPOL_ACTIONS  3

/* Philox stream of the epsilon-greedy draws (0, 1, 3, 4 belong to the environment) */
#define AQUAPOL_STREAM   5

int aquapol_version(void);                 /* AQUAPOL_ABI_VERSION */
const char* aquapol_last_error(void);

/*
 * Weights.  k0 [5][64], k1 [64][64], k2 [64][3] are Keras kernels, row-major [in][out]; b0 [64], b1 [64], b2 [3] the
 * biases; all HOST float32.  shapes = {5, 64, 64, 3}: the layer widths AS THE CALLER HAS THEM (anything else:
 * AQUAPOL_E_INVALID).  aquapol_pack_weights() writes the device-format blob of aquapol_weights_bytes() bytes into HOST
 * memory; the caller uploads it (16-byte aligned) and passes the device copy to aquapol_act_f32.  Packing is a pure
 * permutation: the same weights give the same bytes.  Writing a new blob over the same device memory is how weights
 * are updated under a captured graph.
 */
size_t aquapol_weights_bytes(void);
int aquapol_pack_weights(const float* k0, const float* b0, const float* k1, const float* b1, const float* k2,
                         const float* b2, const int* shapes, void* blob_host, size_t blob_bytes);

/*
 * Q-values and an action for global worlds [env_offset, env_offset + N).
 *   in, ld          : float32 rows of ld >= N elements, 4-byte aligned.
 *                     in_is_normalised == 0: the environment's state rows x, y, theta, goal_x, goal_y (aqua_hip.h; rows
 *                     5.. are not read), normalised in the kernel as the step kernels' obs_norm epilogue does
 *                     (main/impl/utils.py:15-33) -- bit for bit what feeding that obs_norm buffer gives;
 *                     in_is_normalised != 0: float32 [5][ld] holding the network's input as it is.
 *   epsilon         : 0 -> greedy: argmax_a Q[a], the LOWEST index on an exact tie (np.argmax, dqn.py:224); no draw.
 *                     > 0 -> dqn.py:212-228: r = Philox4x32-10(key = seed, counter = (global world, tick +
 *                     *tick_base_dev), stream AQUAPOL_STREAM, attempt 0) in the counter layout of aqua_hip.h's draws; the
 *                     world explores iff (r[0] >> 8) * 2^-24 < epsilon (float32) and then takes ((r[1] >> 8) * 3) >> 24;
 *                     >= 1 always explores.  NaN or negative: AQUAPOL_E_INVALID.
 *   tick_base_dev   : nullable device uint64 added to tick on the device (the environment's graph tick base).
 *   action          : uint8 [N]  (what AQUA_ACT_U8 reads)                    |
 *   q, q_ld         : float32 [3][q_ld], q_ld >= N                           |  each nullable, at least one non-null
 *   q_taken         : float32 [N], Q of the action written (dqn.py:228)      |
 * N == 0 returns 0 without a launch.  Worlds beyond N are neither read nor written.
 */
int aquapol_act_f32(const void* weights_dev, const float* in, int64_t ld, int in_is_normalised, int64_t N,
                    int64_t env_offset, float epsilon, uint64_t seed, uint64_t tick, const uint64_t* tick_base_dev,
                    uint8_t* action, float* q, int64_t q_ld, float* q_taken, void* stream);

#ifdef __cplusplus
}
#endif
#endif
