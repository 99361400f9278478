/*
 * aqua_qmap.h -- C ABI of libaqua_qmap.so: Q-VALUE MAPS of the DQN's Q-networks (main/impl/dqn.py:301-314, 5 -> 64 ReLU
 * -> 64 ReLU -> 3) for every network of a bank in a single launch on MI355X (gfx950).  What the reference's plotter
 * (main/plotting/dqn_qvalue_plotter.py::plot_network_qvalue) computes for one network and one goal -- the best action
 * and the best Q-value at every cell of the world, for a number of headings -- is computed here for P networks and G
 * goals at once, with every network input made in registers from four small tables: the kernel reads nothing per state
 * and writes 5 bytes (17 with q).
 *
 * This header lies beside the source (the listings of include/ and of the package's include/ are pinned by tests).
 *
 * Conventions are those of aqua_bank.h:
 *  - plain pointers and sizes only (streams are void*); every DEVICE buffer is owned by the caller and borrowed until
 *    the work queued on `stream` has run; the library allocates nothing and keeps no pointer.
 *  - aquaqmap_maps_f32 is one asynchronous launch on `stream`: no allocation, no synchronisation, no host read, no
 *    atomic, so it may be captured into a HIP graph; the same inputs give the same bits.
 *  - return value: 0 = ok; > 0 = hipError_t; < 0 = AQUAQMAP_E_* (the values of AQUA_E_*).  aquaqmap_last_error() returns
 *    a thread-local message for the last failing call on this thread; it names the argument that was wrong.
 *  - every argument is validated before the first HIP call.
 *  - there is no CPU path.
 *
 * The bank is that of aqua_bank.h: float32 [P][F] in DEVICE memory, 16-byte aligned, F = aquaqmap_weights_bytes() / 4,
 * slot p byte for byte the blob aquapol_pack_weights() writes for network p (P = 1: the blob of one network).
 *
 * The map.  Four tables of float32 network inputs, already normalised, in DEVICE memory:
 *   xs [W], ys [H], angles [S], goals [G][2]
 * For network p, goal g, sector k, row r and column c the state is
 *   (xs[c], ys[r], angles[k], goals[g][0], goals[g][1])
 * and Q = network_p(state), the float32 acting pass of aquapol_act_f32 / aquabank_act_f32 on normalised input, to the
 * bit: the same fused multiply-add chains in the same order.  Nothing is flipped or transposed in the kernel: the
 * orientation of a map is the order of the tables.  With coords = float32(arange(1, n + 1) / n), xs = ys = coords
 * reversed, angles = float32(linspace(0, 1, S, endpoint = False)) and goals = float32(goal / n), action[p][g][k] is the
 * reference's best_action[:, :, k] after its flipud / fliplr, and value[p][g][k] its best_q_val[:, :, k].
 */
#ifndef AQUA_QMAP_H
#define AQUA_QMAP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQUAQMAP_ABI_VERSION 1

/* library error codes (negative): the values of AQUA_E_* in aqua_hip.h */
#define AQUAQMAP_E_INVALID   (-1)   /* bad argument (null pointer, size out of range ...) */
#define AQUAQMAP_E_ALIGN     (-2)   /* pointer not usable */
#define AQUAQMAP_E_NODEVICE  (-3)   /* no HIP device / wrong architecture */

#define AQUAQMAP_ACTIONS      3
#define AQUAQMAP_MAX_NETWORKS 65536          /* P at most (AQUABANK_MAX_NETWORKS) */
#define AQUAQMAP_MAX_GOALS    65536          /* G at most */
#define AQUAQMAP_MAX_SIDE     65536          /* W and H at most */
#define AQUAQMAP_MAX_SECTORS  4096           /* S at most */
#define AQUAQMAP_MAX_STATES   1073741824     /* S * H * W at most (2^30): a state's index within a map is 32-bit */
#define AQUAQMAP_MAX_TOTAL    1099511627776  /* P * G * S * H * W at most (2^40): every offset, q's included, is 64-bit */

int aquaqmap_version(void);                  /* AQUAQMAP_ABI_VERSION */
const char* aquaqmap_last_error(void);

/* bytes of one slot of the bank: aquapol_weights_bytes() */
size_t aquaqmap_weights_bytes(void);

/*
 * HOST only, no device needed: the items of aquaqmap_maps_f32 with these sizes, P * G * ceil(S * H * W / 32) -- an item
 * is (network, goal, tile of 32 states of one map), the tile running fastest, then the goal.  Any size below 1 or above
 * its cap (the products' caps included): AQUAQMAP_E_INVALID.
 *
 * The launch deals the items over its wavefronts in contiguous runs: with n = 4 * min(ceil(items / 4), 3 * CUs)
 * wavefronts (CUs: the device's compute units), wavefront w takes items [w * s + min(w, t), .. + s + (w < t ? 1 : 0))
 * with s = items / n and t = items % n.
 */
int64_t aquaqmap_items(int64_t P, int64_t G, int64_t H, int64_t W, int64_t S);

/*
 * The maps of P networks for G goals.
 *   bank_dev, P     : the bank (above), 16-byte aligned; 1 <= P <= AQUAQMAP_MAX_NETWORKS.
 *   xs, W           : float32 [W], 1 <= W <= AQUAQMAP_MAX_SIDE: network input 0 by column      |
 *   ys, H           : float32 [H], 1 <= H <= AQUAQMAP_MAX_SIDE: network input 1 by row         |  DEVICE memory, 4-byte
 *   angles, S       : float32 [S], 1 <= S <= AQUAQMAP_MAX_SECTORS: network input 2 by sector   |  aligned, read when the
 *   goals, G        : float32 [G][2], 1 <= G <= AQUAQMAP_MAX_GOALS: network inputs 3 and 4     |  kernel runs
 *                     S * H * W <= AQUAQMAP_MAX_STATES and P * G * S * H * W <= AQUAQMAP_MAX_TOTAL (checked without
 *                     overflow).
 *   action          : uint8   [P][G][S][H][W]: arg-max of Q, the LOWEST index on an exact tie    |
 *   value           : float32 [P][G][S][H][W]: max Q, the bits of the Q that action names        |  each nullable, at
 *   q               : float32 [P][G][3][S][H][W]: all three                                      |  least one non-null
 * All row-major, value and q 4-byte aligned.  Nothing outside these extents is written.
 * Results do not depend on P, G, the launch shape or the device.
 */
int aquaqmap_maps_f32(const void* bank_dev, int64_t P,
                      const float* xs, int64_t W, const float* ys, int64_t H, const float* angles, int64_t S,
                      const float* goals, int64_t G,
                      uint8_t* action, float* value, float* q, void* stream);

#ifdef __cplusplus
}
#endif
#endif
