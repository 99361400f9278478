/*
 * aqua_lbank.h -- C ABI of libaqua_lbank.so: the LEARNER BANK, one DQN update of every network of a Q-network bank
 * (aqua_bank.h) in two launches, and the minibatch draw of every network in one, on MI355X (gfx950).  Where
 * aqualrn_update_f32 of aqua_learner.h trains one network per call, this trains network p = 0 .. P - 1 from its own
 * minibatch of ONE shared experience ring: the training half of a population on one batch of worlds (a sweep over lr,
 * gamma, tau or seeds: main/impl/dqn.py:11-13 exists "to allow multiple trainings in parallel").
 *
 * Conventions are those of aqua_learner.h:
 *  - plain pointers and sizes only (streams are void*); every DEVICE buffer is owned by the caller and borrowed until
 *    the work queued on `stream` has run; the library allocates nothing and keeps no pointer.
 *  - aqualbank_update_f32 is two asynchronous launches on `stream`, aqualbank_draw one: no allocation, no
 *    synchronisation, no host read, so they may be captured into a HIP graph.
 *  - return value: 0 = ok; > 0 = hipError_t; < 0 = AQUALBANK_E_* (the values of AQUA_E_*).  aqualbank_last_error()
 *    returns a thread-local message for the last failing call on this thread.
 *  - every argument is validated before the first HIP call.  There is no CPU path.
 *
 * The state of P learners is stacked: theta, theta_target, m, v are float32 [P][AQUALBANK_PARAMS] (the canonical Keras
 * order of aqua_learner.h), t is uint64 [P]; the acting blobs are the bank's own tensor float32 [P][blob_floats]
 * (aqua_bank.h: blob_floats = 4804) and a second tensor of that shape holds the target blobs; the permutation table is
 * shared.  The experience is the one ring of the batch (aqua_replay.h): rows s, a, r, s2, d, ok with ld = capacity.
 *
 * Hyper-parameters are per network, in a DEVICE table float64 [P][AQUALBANK_HYPER_WORDS] that the kernels read: row p is
 * gamma, tau, lr, beta1, beta2, eps and two spare words.  aqualbank_pack_hyper() writes (and validates) it on the host.
 *
 * The update contract.  For every p, slot p of every output -- theta, theta_target, m, v, t, both blobs, loss, grad_out,
 * idx_out -- is bit for bit what
 *   aqualrn_update_f32(theta + p * PARAMS, theta_target + p * PARAMS, m + p * PARAMS, v + p * PARAMS, t + p,
 *                      s, a, r, s2, d, ok, ld, size, idx + p * B, B, <unused seed>, strategy,
 *                      gamma_p, tau_p, lr_p, beta1_p, beta2_p, eps_p,
 *                      blob_online + p * blob_floats, blob_target + p * blob_floats, perm, blob_floats,
 *                      <a workspace of its own>, .., idx_out + p * B, grad_out + p * PARAMS, loss + p, stream)
 * leaves: the kernels run the same device code (csrc/aqua_lrn.hpp), block (g, p) of the launch doing what block g of
 * that call does.  A network whose samples are all invalid is left exactly as it was (loss and grad_out 0) while its
 * neighbours learn.  Results do not depend on P, the launch shape or the device.
 */
#ifndef AQUA_LBANK_H
#define AQUA_LBANK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQUALBANK_ABI_VERSION 1

/* library error codes (negative): the values of AQUA_E_* in aqua_hip.h */
#define AQUALBANK_E_INVALID   (-1)   /* bad argument (null pointer, size out of range, value out of range ...) */
#define AQUALBANK_E_ALIGN     (-2)   /* pointer not usable */
#define AQUALBANK_E_NODEVICE  (-3)   /* no HIP device / wrong architecture */

#define AQUALBANK_PARAMS        4739      /* AQUALRN_PARAMS */
#define AQUALBANK_MAX_BATCH     1048576   /* AQUALRN_MAX_BATCH: samples per network and update */
#define AQUALBANK_MAX_NETWORKS  4096
#define AQUALBANK_MAX_CAPACITY  2147483647   /* AQUARPL_MAX_CAPACITY: a slot fits the int32 idx */
#define AQUALBANK_HYPER_FIELDS  6         /* gamma, tau, lr, beta1, beta2, eps */
#define AQUALBANK_HYPER_WORDS   8         /* doubles per row of the device table: the fields and two spare words */
#define AQUALBANK_STREAM        6         /* Philox stream of the minibatch draws: AQUALRN_STREAM */
#define AQUALBANK_ATTEMPTS      4         /* draws per sample before it is given up (-1): the learner's */

int aqualbank_version(void);                 /* AQUALBANK_ABI_VERSION */
const char* aqualbank_last_error(void);

/* bytes of DEVICE workspace an update of P networks with B samples each needs: P regions of aqualrn_workspace_bytes(B)
 * bytes (each a multiple of 16).  Non-decreasing in P and in B; 0 for P or B out of range. */
size_t aqualbank_workspace_bytes(int64_t P, int64_t B);

/*
 * HOST only, no device needed: in float64 [P][AQUALBANK_HYPER_FIELDS] -> out float64 [P][AQUALBANK_HYPER_WORDS] (the spare
 * words are written as 0), to be copied to the device.  Every row is validated by the rules of aqualrn_update_f32: gamma,
 * tau in [0, 1]; lr >= 0; beta1, beta2 in [0, 1); eps > 0; all finite.  Otherwise AQUALBANK_E_INVALID, and the message
 * names the network and the field.  `out` is written only if every row is valid.
 */
int aqualbank_pack_hyper(const double* in_host, int64_t P, double* out_host);

/*
 * One update of every network.  All pointers but the two of aqualbank_pack_hyper are DEVICE pointers.
 *   theta, theta_target, m, v : float32 [P][AQUALBANK_PARAMS], 4-byte aligned, four arrays that do not overlap.
 *   t_dev                     : uint64 [P], 8-byte aligned: updates applied so far, per network.
 *   P                         : 1 <= P <= AQUALBANK_MAX_NETWORKS.
 *   s .. ok, ld, size         : the ring's rows as aqualrn_update_f32 takes them; size is the capacity when idx comes from
 *                               aqualbank_draw (a slot never written has ok == 0).
 *   idx, B                    : int32 [P][B], REQUIRED (there is no in-kernel draw here): row p is network p's minibatch.
 *                               A sample is valid iff 0 <= idx < size and ok[idx] != 0 and a[idx] < 3.
 *   strategy                  : AQUALRN_DOUBLE_REF .. AQUALRN_STANDARD of aqua_learner.h, optionally | AQUALRN_LOSS_REFERENCE:
 *                               one bootstrap strategy and one loss form per launch.
 *   hyper_dev                 : float64 [P][AQUALBANK_HYPER_WORDS] as aqualbank_pack_hyper() wrote it, 8-byte aligned.  The
 *                               device cannot validate it; gamma is rounded to float32 where aqualrn_update_f32 rounds it.
 *   blob_online, blob_target  : nullable float32 [P][blob_floats]; perm int32 [AQUALBANK_PARAMS] required if one is given.
 *   workspace                 : 16-byte aligned, at least aqualbank_workspace_bytes(P, B) bytes.
 *   idx_out                   : nullable int32 [P][B];  grad_out: nullable float32 [P][AQUALBANK_PARAMS];  loss: nullable
 *                               float32 [P].
 * The gradient launch has grid (groups(B), P), the apply launch (ceil(AQUALBANK_PARAMS / 64), P).  B == 0 returns 0
 * without a launch.
 */
int aqualbank_update_f32(float* theta, float* theta_target, float* m, float* v, uint64_t* t_dev, int64_t P,
                         const float* s, const uint8_t* a, const float* r, const float* s2, const uint8_t* d,
                         const uint8_t* ok, int64_t ld, int64_t size,
                         const int32_t* idx, int64_t B, int strategy, const double* hyper_dev,
                         float* blob_online, float* blob_target, const int32_t* perm, int64_t blob_floats,
                         void* workspace, size_t workspace_bytes,
                         int32_t* idx_out, float* grad_out, float* loss, void* stream);

/*
 * The minibatch draw of every network, confined to its own slots of the ONE ring: one launch.
 * The ring of aqua_replay.h places world i of a batch of N worlds in slot base + i; with capacity % N == 0 (required,
 * otherwise AQUALBANK_E_INVALID) slot s always holds a transition of world s mod N, which belongs to network
 * (s mod N) / seg: the ring is P interleaved rings.
 *   header          : the ring's int64 [4] header, 8-byte aligned; header[1] is the number of filled slots.
 *   ok, capacity    : uint8 [capacity], 1 <= capacity <= AQUALBANK_MAX_CAPACITY.
 *   N, seg          : 1 <= N <= capacity worlds per batched step; seg >= 1 worlds per network.  Network p owns the worlds
 *                     [p * seg, min((p + 1) * seg, N)), w_p of them.
 *   t_dev, seed_dev : uint64 [P] each, 8-byte aligned: the update counters and the keys of the draws.
 *   idx, B          : int32 [P][B] receives the slots, 0 <= B <= AQUALBANK_MAX_BATCH.
 * rounds = clamp(header[1], 0, capacity) / N, size_p = rounds * w_p.  For sample j and attempt a = 0 .. 3:
 *   r    = Philox4x32-10(key = seed[p], counter = (j, t[p] + 1), stream AQUALBANK_STREAM, attempt a), the layout of aquarpl_draw
 *   c    = (uint64(r[0]) * size_p) >> 32
 *   slot = (c / w_p) * N + p * seg + c % w_p
 * the first slot with ok[slot] != 0 is idx[p][j]; none: -1.  Networks with p * seg >= N and rings with rounds == 0 get -1
 * everywhere.  No computed slot is used as an address unless it is below capacity.  With P = 1 and seg >= N this is
 * aquarpl_draw bit for bit.
 */
int aqualbank_draw(const int64_t* header, const uint8_t* ok, int64_t capacity, int64_t N, int64_t seg, int64_t P,
                   const uint64_t* t_dev, const uint64_t* seed_dev, int32_t* idx, int64_t B, void* stream);

#ifdef __cplusplus
}
#endif
#endif
