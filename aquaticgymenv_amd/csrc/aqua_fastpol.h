/*
 * aqua_fastpol.h -- C ABI of libaqua_fastpol.so: the FAST ACTING PATH of the DQN's Q-networks (main/impl/dqn.py:301-314,
 * 5 -> 64 ReLU -> 64 ReLU -> 3) on MI355X (gfx950).  Where aqua_policy.h and aqua_bank.h evaluate the two hidden layers
 * on the float32-input MFMA, this library evaluates them on v_mfma_f32_32x32x16_f16 with every operand split into a high
 * and a low f16 part: three f16 products stand in for one float32 product, at float32-like accuracy.
 *
 * This header lies beside the source (the listings of include/ and of the package's include/ are pinned by tests).
 *
 * Conventions are those of aqua_bank.h:
 *  - plain pointers and sizes only (streams are void*); every DEVICE buffer is owned by the caller and borrowed until
 *    the work queued on `stream` has run; the library allocates nothing and keeps no pointer.
 *  - aquafast_refresh and aquafast_act_f16 are one asynchronous launch each on `stream`: no allocation, no
 *    synchronisation, no host read, no atomic, so they may be captured into a HIP graph.
 *  - return value: 0 = ok; > 0 = hipError_t; < 0 = AQUAFAST_E_* (the values of AQUA_E_*).  aquafast_last_error() returns a
 *    thread-local message for the last failing call on this thread.
 *  - every argument is validated before the first HIP call.
 *  - there is no CPU path.
 *
 * The scheme.  split(v): c = clamp(v, +-65504); hi = f16(c), round to nearest even; lo = f16((c - float(hi)) * 2^11) in
 * float32 arithmetic (both operations are exact).  Every value that becomes f16 is clamped first -- weights in the
 * refresh, inputs and hidden activations in the kernel -- so no infinity arises.  NaN: the libraries are built with
 * -fno-honor-nans and no state of the project holds one.  A NaN WEIGHT is split into two quiet f16 NaNs (0x7E00) by the host
 * and by the device alike, so the refresh stays bit for bit the host's; what aquafast_act_f16 writes for a network with a NaN
 * weight, or for a NaN input, is unspecified (the clamp's med3 may turn a NaN activation into a number): it is not the
 * float32 path's result and is outside the contract below.  For unit u of layers 1 and 2:
 *   acc_hi = bias_u (float32) + sum W_hi X_hi          acc_lo = 0 + sum (W_hi X_lo + W_lo X_hi)
 *   unit   = relu(fmaf(acc_lo, 2^-11, acc_hi))
 * both float32 MFMA accumulators; the lo * lo product is dropped.  Layer 3 is that of aquapol_act_f32: float32 weights,
 * fmaf chains, one add across the lane halves.  The order in which the MFMA sums the 16 products of a k-step is the
 * hardware's: the results are deterministic, and equal among all forms of this library (below), but not bit-equal to a
 * host model.
 *
 * The fast blob of one network: aquafast_weights_bytes() = 21776 bytes, a multiple of 16, in DEVICE memory, 16-byte
 * aligned; a bank is [P] of them, contiguous.  It holds 10240 f16 elements -- the A fragments of the two MFMA layers, hi
 * and lo parts -- followed by the 324 float32 of the acting blob's LDS part (biases, layer-3 weights) as they are.
 * aquafast_map() says where each 16-bit element comes from; nothing else states the layout to a caller.
 */
#ifndef AQUA_FASTPOL_H
#define AQUA_FASTPOL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQUAFAST_ABI_VERSION 1

/* library error codes (negative): the values of AQUA_E_* in aqua_hip.h */
#define AQUAFAST_E_INVALID   (-1)   /* bad argument (null pointer, size out of range ...) */
#define AQUAFAST_E_ALIGN     (-2)   /* pointer not usable */
#define AQUAFAST_E_NODEVICE  (-3)   /* no HIP device / wrong architecture */

/* the one architecture (dqn.py:301-314) and the Philox stream of the epsilon-greedy draws: aqua_policy.h's */
#define AQUAFAST_INPUTS   5
#define AQUAFAST_HIDDEN   64
#define AQUAFAST_ACTIONS  3
#define AQUAFAST_STREAM   5

#define AQUAFAST_MAX_NETWORKS 65536

/* kinds of a map entry (its two low bits) */
#define AQUAFAST_PART_HI    0       /* the hi part of split(float) */
#define AQUAFAST_PART_LO    1       /* the lo part of split(float) */
#define AQUAFAST_PART_BITS0 2       /* bits 0 .. 15 of the float32, copied */
#define AQUAFAST_PART_BITS1 3       /* bits 16 .. 31 of the float32, copied */

int aquafast_version(void);                 /* AQUAFAST_ABI_VERSION */
const char* aquafast_last_error(void);

/* bytes of one fast blob (21776) */
size_t aquafast_weights_bytes(void);

/*
 * HOST only: the map of a fast blob.  map_host: int32 [aquafast_weights_bytes() / 2], 4-byte aligned; `bytes` is its
 * size and must be at least 2 * aquafast_weights_bytes().  Entry e describes 16-bit element e of a fast blob:
 *   -1                 padding, always zero
 *   4 * b + part       element e is made from float b of the float32 acting blob (the aqua::qnet layout that
 *                      aquapol_pack_weights() writes), part = AQUAFAST_PART_*
 * Every parameter of the two hidden kernels appears exactly once as HI and once as LO; every bias and every layer-3
 * weight exactly once as BITS0 and once as BITS1.  The device copy of this map is what aquafast_refresh reads.
 */
int aquafast_map(int32_t* map_host, size_t bytes);

/*
 * HOST only: the split of one network.  blob_f32_host: the float32 acting blob (aquapol_weights_bytes() bytes, 4-byte
 * aligned); fast_host: receives the fast blob (`bytes` >= aquafast_weights_bytes(), 4-byte aligned).
 */
int aquafast_pack_host(const void* blob_f32_host, void* fast_host, size_t bytes);

/*
 * One launch: fast blob p = split of float32 blob p, for p in [0, P), bit for bit what aquafast_pack_host gives.
 *   blobs_f32_dev, stride_bytes : P float32 acting blobs in DEVICE memory, blob p at blobs_f32_dev + p * stride_bytes;
 *                                 16-byte aligned, stride_bytes a multiple of 4 and >= aquapol_weights_bytes().  This is
 *                                 the blob QNetwork.load(), the learners' re-pack and the selector's copy write.
 *   map_dev                     : the map of aquafast_map() in DEVICE memory, 4-byte aligned.  An entry that names a float
 *                                 outside the blob gives zero.
 *   fast_dev                    : P fast blobs, contiguous, 16-byte aligned.
 *   1 <= P <= AQUAFAST_MAX_NETWORKS.
 */
int aquafast_refresh(const void* blobs_f32_dev, int64_t stride_bytes, const int32_t* map_dev, void* fast_dev, int64_t P, void* stream);

/*
 * Q-values and an action for global worlds [env_offset, env_offset + N); local world i in [0, N) is evaluated with
 * network i / seg of the fast bank fast_dev (networks = 1 with a huge seg serves a single network).  The arguments from
 * `in` onwards, their checks, the epsilon-greedy draw and the stores are those of aquabank_act_f32 (aqua_bank.h): the same
 * Philox key, the same random action, so the set of exploring worlds and their actions equal the float32 path's exactly.
 *
 * The contract.  With E_s the error of the scheme's host model against a float64 evaluation on the same batch, the Q
 * written here are within 4 E_s of the float64 ones (tests/_fastpol.py).  Among themselves the forms of this call are bit
 * for bit: one network and a bank's segment, eager and replayed, raw and normalised input.  Results do not depend on
 * networks, seg, N, the launch shape or the device.
 */
int aquafast_act_f16(const void* fast_dev, int64_t networks, int64_t seg,
                     const float* in, int64_t ld, int in_is_normalised, int64_t N, int64_t env_offset,
                     float epsilon, const float* epsilon_dev,
                     uint64_t seed, uint64_t tick, const uint64_t* tick_base_dev,
                     uint8_t* action, float* q, int64_t q_ld, float* q_taken, void* stream);

#ifdef __cplusplus
}
#endif
#endif
