/*
 * aqua_learner.h -- C ABI of libaqua_learner.so: one DQN update (TD target, gradient, Adam, soft target update, re-pack
 * of the acting network's weights) for a minibatch of a device experience ring, on MI355X (gfx950), next to the Q-network
 * of aqua_policy.h and the batched environment of aqua_hip.h.
 *
 * Reference being replaced: main/impl/dqn.py:175-176 with its defaults -- LOSS_STRATEGY = _improve_strategy_double
 * (dqn.py:262-272), the Adam of dqn.py:313 as Keras 2.3 applies it, and _improve_target_network (dqn.py:294-299).
 *
 * The loss has three forms (T_bj = y_b for j = a_b, Q(s_b)[j] otherwise, T and y held constant):
 *   "custom_grad", the reference's default IMPROVE_STRATEGY = _improve_network_gradient (dqn.py:238-249), AS IT EXECUTES:
 *       the [B,1] prediction (keepdims, dqn.py:244) is subtracted from the whole [B,3] target array (dqn.py:246), the
 *       difference broadcasts and reduce_mean runs over 3 B elements:
 *           L_ref = 1/(3 B) sum_b sum_j (Q(s_b)[a_b] - T_bj)^2,   dL_ref/dQ(s_b)[a_b] = 2/(3 B) (3 Q_a - y - sum_{j != a} Q_j)
 *       This is AQUALRN_LOSS_REFERENCE.  Its gradient differs from the next two in direction, not only in scale.
 *   "standard", IMPROVE_STRATEGY = _improve_network (dqn.py:230-236): train_on_batch with Keras "mse" (dqn.py:313) on [B,3]
 *       outputs against T, 1/(3 B) sum_b (Q_a - y)^2: the textbook direction with a factor 1/3.  Not offered.
 *   the library's default, the textbook mean squared TD error 1/B sum_b (Q_a - y)^2: gradient 2/B_eff (Q_a - y).  It is
 *       neither of the reference's two paths exactly.
 * tests/_learner_autograd.py differentiates the first and the third with autograd; tests/test_learner_model_cpu.py and
 * tests/test_learner_forms_gpu.py hold the model and the kernels to it.
 *
 * Conventions are those of aqua_policy.h:
 *  - plain pointers and sizes only (streams are void*); every DEVICE buffer is owned by the caller and borrowed until
 *    the work queued on `stream` has run; the library allocates nothing and keeps no pointer.
 *  - aqualrn_update_f32 is two asynchronous launches on `stream`: no allocation, no synchronisation, no host read, so it
 *    may be captured into a HIP graph.
 *  - return value: 0 = ok; > 0 = hipError_t; < 0 = AQUALRN_E_* (the values of AQUA_E_*).  aqualrn_last_error() returns a
 *    thread-local message for the last failing call on this thread.
 *  - every argument is validated before the first HIP call.  There is no CPU path.
 *
 * Parameters: ONE float32 vector of AQUALRN_PARAMS elements per network, in canonical Keras order
 *    k0 [5][64], b0 [64], k1 [64][64], b1 [64], k2 [64][3], b2 [3]        (kernels row-major [in][out])
 * Four such vectors: the online network theta, the target network theta_target, Adam's m and v; and a device uint64
 * update counter t.
 *
 * Numerics: float32 forward and backward, no reduced-precision operand anywhere; the last layer, y and delta_b =
 * Q(s_b)[a_b] - y_b are evaluated in double from the float32 hidden activations and delta_b is rounded once (it is a
 * difference of long sums that multiplies every gradient element; the loss is the mean of the unrounded delta_b^2).
 * Every gradient element is the float32 sum S of its per-sample terms, multiplied ONCE by float32(2.0 / B_eff).  With
 * AQUALRN_LOSS_REFERENCE delta_b = 3 Q_a - y - sum_{j != a} Q_j from the same three double Q-values, rounded once, the
 * factor is float32(2.0 / (3 B_eff)) and the loss the double sum of the 3 B_eff squares over 3 B_eff.  No
 * floating-point atomics: which samples are added into which partial sum, and the order in which the partial sums are
 * added, are functions of B alone (not of the grid, not of the device), so the same inputs give the same bits run to run,
 * eager or replayed from a graph.  Adam and the soft update are evaluated in double from the float32 state and rounded
 * once per stored value.
 */
#ifndef AQUA_LEARNER_H
#define AQUA_LEARNER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQUALRN_ABI_VERSION 1

/* library error codes (negative): the values of AQUA_E_* in aqua_hip.h */
#define AQUALRN_E_INVALID   (-1)   /* bad argument (null pointer, negative size, value out of range ...) */
#define AQUALRN_E_ALIGN     (-2)   /* pointer not usable */
#define AQUALRN_E_NODEVICE  (-3)   /* no HIP device / wrong architecture */

/* the one architecture (dqn.py:301-314): 5 * 64 + 64 + 64 * 64 + 64 + 64 * 3 + 3 parameters */
#define AQUALRN_PARAMS      4739
#define AQUALRN_MAX_BATCH   1048576

/* Philox stream of the minibatch draws (0, 1, 3, 4 belong to the environment, 5 to the policy) */
#define AQUALRN_STREAM      6

/* what the bootstrap term f of the target y = r + (d == 0 ? gamma * f : 0) is */
#define AQUALRN_DOUBLE_REF  0      /* Q_target(s')[argmax Q_online(s)]   what dqn.py:267-268 executes */
#define AQUALRN_DOUBLE      1      /* Q_target(s')[argmax Q_online(s')]  what its comment says */
#define AQUALRN_FIXED       2      /* max Q_target(s')                   dqn.py:274-282 */
#define AQUALRN_STANDARD    3      /* max Q_online(s')                   dqn.py:284-292 */
/* a flag OR-ed into `strategy`: the loss as dqn.py:243-247 executes it (see above); without it the mean squared TD error */
#define AQUALRN_LOSS_REFERENCE 16

int aqualrn_version(void);                 /* AQUALRN_ABI_VERSION */
const char* aqualrn_last_error(void);

/* bytes of DEVICE workspace an update of B samples needs (non-decreasing in B; 0 for B outside [0, AQUALRN_MAX_BATCH]) */
size_t aqualrn_workspace_bytes(int64_t B);

/*
 * One update.  All pointers are DEVICE pointers.
 *   theta, theta_target, m, v : float32 [AQUALRN_PARAMS], 4-byte aligned, read and written.
 *   t_dev                     : uint64, 8-byte aligned: the number of updates applied so far; advanced by one.
 *   s, s2, ld                 : float32 [5][ld] normalised observations before / after the step (the ring's rows)
 *   a, d, ok                  : uint8 [ld]: discrete action (0..2; a slot holding anything else is not a sample),
 *                               termination code (done = d != 0), 1 for a real transition
 *   r                         : float32 [ld]
 *   size                      : filled slots, 0 <= size <= ld
 *   idx, B                    : int32 [B] slots of the minibatch; NULL: drawn on the device -- sample j of the update that
 *                               takes t to t + 1 uses Philox4x32-10(key = seed, counter = (j, t + 1), stream AQUALRN_STREAM,
 *                               attempt a) in the counter layout of aqua_hip.h's draws, idx = (uint64(r[0]) * size) >> 32,
 *                               the first attempt a = 0..3 whose ok[idx] != 0 wins.  In both forms a sample is VALID iff
 *                               0 <= idx < size and ok[idx] != 0; an index outside [0, size) is never dereferenced and an
 *                               invalid sample contributes nothing.  B_eff = number of valid samples.
 *   strategy                  : AQUALRN_DOUBLE_REF .. AQUALRN_STANDARD, optionally | AQUALRN_LOSS_REFERENCE; any other bit is
 *                               AQUALRN_E_INVALID.  arg-max takes the lowest index on a tie.
 *   gamma, tau in [0, 1]; lr >= 0; beta1, beta2 in [0, 1); eps > 0; all finite (otherwise AQUALRN_E_INVALID).
 *       L      = (1 / B_eff) sum_b (Q_online(s_b)[a_b] - y_b)^2, y constant
 *                (AQUALRN_LOSS_REFERENCE: 1 / (3 B_eff) sum_b sum_j (Q_online(s_b)[a_b] - T_bj)^2, T constant)
 *       t     <- t + 1;  lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), in double from the device counter, rounded once
 *       m     <- beta1 m + (1 - beta1) g;  v <- beta2 v + (1 - beta2) g^2;  theta <- theta - lr_t m / (sqrt(v) + eps)
 *       theta_target <- tau theta + (1 - tau) theta_target       (with the NEW theta; tau = 1 copies, tau = 0 leaves it)
 *   blob_online, blob_target  : nullable float32 [blob_floats] device-format weight blobs of aqua_policy.h: parameter p of
 *                               the new theta / theta_target is stored at float index perm[p] (int32 [AQUALRN_PARAMS],
 *                               required if a blob is given; an entry outside [0, blob_floats) is skipped).
 *   workspace                 : 16-byte aligned, at least aqualrn_workspace_bytes(B) bytes; contents need not be kept.
 *   idx_out                   : nullable int32 [B]: the slot used, -1 for an invalid sample
 *   grad_out                  : nullable float32 [AQUALRN_PARAMS]: the gradient applied
 *   loss                      : nullable float32 [1]: L before the update
 * B_eff == 0: theta, theta_target, m, v, t and the blobs are left exactly as they were; loss and grad_out are 0.
 * B == 0 returns 0 without a launch.  B > AQUALRN_MAX_BATCH: AQUALRN_E_INVALID.
 */
int aqualrn_update_f32(float* theta, float* theta_target, float* m, float* v, uint64_t* t_dev,
                       const float* s, const uint8_t* a, const float* r, const float* s2, const uint8_t* d,
                       const uint8_t* ok, int64_t ld, int64_t size,
                       const int32_t* idx, int64_t B, uint64_t seed,
                       int strategy, double gamma, double tau, double lr, double beta1, double beta2, double eps,
                       float* blob_online, float* blob_target, const int32_t* perm, int64_t blob_floats,
                       void* workspace, size_t workspace_bytes,
                       int32_t* idx_out, float* grad_out, float* loss, void* stream);

#ifdef __cplusplus
}
#endif
#endif
