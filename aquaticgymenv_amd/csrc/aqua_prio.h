/*
 * aqua_prio.h -- C ABI of libaqua_prio.so: PRIORITISED EXPERIENCE REPLAY (Schaul et al., 2016, proportional variant)
 * over the experience ring of aqua_replay.h, for every network of a learner bank (aqua_lbank.h), on MI355X (gfx950):
 * a sum tree per network over the network's own slots of the ring, the entries that keep it (insert, set), the draw by
 * descent with its importance weights, and the bank update with the weights multiplied in.
 *
 * Reference being extended: the uniform minibatch draw of main/impl/dqn.py:262-292 (aqualbank_draw).
 *
 * This header lies beside the source (the listings of include/ and of the package's include/ are pinned by tests).
 *
 * Conventions are those of aqua_lbank.h and aqua_nstep.h:
 *  - plain pointers and sizes only (streams are void*); every DEVICE buffer is owned by the caller and borrowed until
 *    the work queued on `stream` has run; the library allocates nothing and keeps no pointer.
 *  - the device entries are asynchronous on `stream`: no allocation, no synchronisation, no host read, so they may be
 *    captured into a HIP graph.  Integer atomics only: every sum is an integer sum and independent of the order of arrival,
 *    the same bits eager or replayed.  No floating-point atomic anywhere.
 *  - return value: 0 = ok; > 0 = hipError_t; < 0 = AQUAPRIO_E_* (the values of AQUA_E_*).  aquaprio_last_error() returns a
 *    thread-local message for the last failing call on this thread.
 *  - every argument is validated before the first HIP call.  There is no CPU path.
 *
 * THE TREE.  The ring is P interleaved rings: with capacity % N == 0 (REQUIRED) slot s holds a transition of world s mod N,
 * which network (s mod N) / seg acted in.  Network p owns w_p = min(seg, N - p seg) worlds (0 if p seg >= N), and its
 * leaf c is the slot aqualbank_draw names,
 *
 *     slot(p, c) = (c / w_p) N + p seg + c mod w_p,          c < (capacity / N) w_p.
 *
 * Every network has one tree of L0 = (capacity / N) seg leaves (1 <= seg <= N); leaves a network has no slot for stay 0.
 *   level 0      : the leaves, uint32 fixed point with AQUAPRIO_FRAC_BITS = 20 fraction bits,
 *                      q = clamp(rint(pi 2^20), 1, 2^31 - 1),   pi = (|td| + eps)^alpha;      q = 0: not an experience
 *   level k >= 1 : uint64, n_k = ceil(n_{k-1} / 64) nodes, node i the sum of entries 64 i .. 64 i + 63 of level k - 1,
 *                  up to the level with a single node, the root.  There is always a root (L0 = 1: one leaf, one root).
 * No sum can overflow: a tree has fewer than 2^31 leaves (L0 <= capacity < 2^31) of less than 2^31 each, so every node is
 * below 2^62; the differences the entries add are above -2^31 and below 2^31.
 * Storage: level k of network p is `stride_k` entries at byte `offset_k + p stride_k size_k` of the tree buffer, with
 * stride_k = n_k rounded up to a multiple of 64: entries beyond n_k are never written and must be 0 (the caller zeroes the
 * buffer once), so a node's 64 children are always one in-bounds load.  aquaprio_layout returns these numbers.
 * pmax is uint32 [P]: the largest q ever set for the network, initialised by the caller to AQUAPRIO_ONE (pi = 1).
 *
 * INVARIANT after every entry has run: every node of every level k >= 1 equals the exact sum of its 64 children.
 * Mechanism: a leaf is written with an atomic exchange; the signed difference against the value that came back is added to
 * every ancestor with a 64-bit atomic add (lanes of a wavefront that follow each other and share an ancestor add their
 * differences first and issue one atomic); pmax is kept with an atomic max.  Any order of arrival gives the same tree, and
 * a slot named twice with the same value counts once (its second arrival sees the difference 0).  Two DIFFERENT values
 * for one slot in one aquaprio_set: one of them wins, and the invariant still holds.
 *
 * THE POWER FUNCTION.  x^e is ONE __host__ __device__ function of the source, shared by the quantiser and the weights:
 * exponent manipulation, then sums, products and quotients in double, each correctly rounded, nothing contracted
 * (`#pragma clang fp contract(off)`); log by the atanh series on [sqrt(1/2), sqrt(2)), exp by Cody-Waite reduction and a
 * Taylor polynomial.  Relative error at most 2^-40 (it is near 2^-46 for |e ln x| <= 45).  The host entries aquaprio_pow,
 * aquaprio_quantise, aquaprio_beta and aquaprio_weight run the same code as the kernels: the device's bits without a device.
 *
 *   quantise(td, alpha, eps) : v = (double)td + eps;  x = v^alpha * 2^20;  x >= 2^31 - 1: 2^31 - 1;  else max(rint(x), 1)
 *                              (rint: to nearest, ties to even)
 *   beta(t, beta0, anneal)   : f = (double)min(t, anneal) / (double)anneal;  b = beta0 + (1 - beta0) * f;  min(b, 1)
 *   weight(size, q, T, beta) : ((double)T / ((double)size * (double)q))^beta      = (size q / T)^-beta
 */
#ifndef AQUA_PRIO_H
#define AQUA_PRIO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQUAPRIO_ABI_VERSION 1

/* library error codes (negative): the values of AQUA_E_* in aqua_hip.h */
#define AQUAPRIO_E_INVALID   (-1)   /* bad argument (null pointer, negative size, value out of range ...) */
#define AQUAPRIO_E_ALIGN     (-2)   /* pointer not usable */
#define AQUAPRIO_E_NODEVICE  (-3)   /* no HIP device / wrong architecture */

#define AQUAPRIO_FANOUT        64           /* children per node: one wavefront's load */
#define AQUAPRIO_FRAC_BITS     20           /* fraction bits of a leaf */
#define AQUAPRIO_ONE           1048576      /* the quantised pi = 1: what pmax starts from */
#define AQUAPRIO_QMAX          2147483647   /* the largest leaf */
#define AQUAPRIO_MAX_LEVELS    7            /* levels at most, the leaves included: 2^31 -> 2^25 -> 2^19 -> 2^13 -> 2^7 -> 2 -> 1 */
#define AQUAPRIO_LAYOUT_WORDS  24           /* int64 words aquaprio_layout writes: 3 + 3 * AQUAPRIO_MAX_LEVELS */
#define AQUAPRIO_STREAM        7            /* the Philox stream of the descent's draws (0, 1, 3, 4, 5 and 6 are taken) */
#define AQUAPRIO_MAX_CAPACITY  2147483647   /* slots: AQUARPL_MAX_CAPACITY */
#define AQUAPRIO_MAX_NETWORKS  4096         /* P at most: AQUALBANK_MAX_NETWORKS */
#define AQUAPRIO_MAX_BATCH     1048576      /* B at most: AQUALBANK_MAX_BATCH */
#define AQUAPRIO_MAX_BLOCKS    2048         /* blocks of AQUAPRIO_BLOCK threads per launch and network at most (grid-stride above that) */
#define AQUAPRIO_BLOCK         256          /* four wavefronts: the descent takes four samples per block and pass */

int aquaprio_version(void);                 /* AQUAPRIO_ABI_VERSION */
const char* aquaprio_last_error(void);

/*
 * HOST only: the storage of the P trees.  1 <= capacity <= AQUAPRIO_MAX_CAPACITY, 1 <= N <= capacity, capacity % N == 0,
 * 1 <= seg <= N, 1 <= P <= AQUAPRIO_MAX_NETWORKS.  out_host: int64 [AQUAPRIO_LAYOUT_WORDS], 8-byte aligned:
 *   [0] levels (the leaves included, 2 .. AQUAPRIO_MAX_LEVELS)   [1] total bytes of the buffer   [2] L0
 *   [3 + 3 k + 0] n_k    [3 + 3 k + 1] stride_k (entries per network)    [3 + 3 k + 2] offset_k (bytes; a multiple of 512)
 * for k < levels, zeros behind.  Level 0 holds 4-byte entries, the others 8-byte entries.
 */
int aquaprio_layout(int64_t capacity, int64_t N, int64_t seg, int64_t P, int64_t* out_host);

/*
 * HOST only, no device needed: the device's bits of the four functions above.
 *   aquaprio_pow      x in [2^-1000, 2^1000], e in [-1, 1]; anything else: returns -1.0 and sets the message
 *   aquaprio_quantise td finite and >= 0, alpha in [0, 1], eps finite and >= 2^-1022; anything else: returns 0
 *   aquaprio_beta     beta0 in [0, 1], anneal >= 1; anything else: returns -1.0
 *   aquaprio_weight   size >= 1, 1 <= q <= AQUAPRIO_QMAX, T >= q and T < 2^62, beta in [0, 1]; anything else: returns -1.0
 */
double aquaprio_pow(double x, double e);
uint32_t aquaprio_quantise(double td, double alpha, double eps);
double aquaprio_beta(uint64_t t, double beta0, int64_t anneal);
double aquaprio_weight(uint64_t size, uint32_t q, uint64_t T, double beta);

/*
 * What every device entry takes of the trees:
 *   tree, tree_bytes  : the buffer, 512-byte aligned, at least aquaprio_layout(...)[1] bytes
 *   pmax              : uint32 [P]
 *   capacity, N, seg, P as in aquaprio_layout.
 *
 * aquaprio_insert: ONE launch, to be queued behind aquarpl_close.  header is the ring's int64 [4] (read only); the batch
 * closed last is the N slots from header[2].  Slot header[2] + i gets the leaf pmax[p] of its network if ok[slot] != 0 and 0
 * otherwise; worlds of no network (i >= P seg) are skipped.  A header[2] outside [0, capacity) or no multiple of N: nothing
 * is written.  ok: the ring's uint8 [>= capacity] row.
 */
int aquaprio_insert(void* tree, size_t tree_bytes, uint32_t* pmax, int64_t capacity, int64_t N, int64_t seg, int64_t P,
                    const int64_t* header, const uint8_t* ok, void* stream);

/*
 * aquaprio_set: ONE launch, to be queued behind the update.  idx int32 [P][B], td float32 [P][B]: the leaf of slot
 * idx[p][j] becomes quantise(td[p][j], alpha, eps) and pmax[p] its maximum with that.  Untouched: idx outside [0, capacity),
 * a slot that is not network p's, td < 0 or not finite.  0 <= B <= AQUAPRIO_MAX_BATCH; B == 0 returns 0 without a launch.
 */
int aquaprio_set(void* tree, size_t tree_bytes, uint32_t* pmax, int64_t capacity, int64_t N, int64_t seg, int64_t P,
                 const int32_t* idx, const float* td, int64_t B, double alpha, double eps, void* stream);

/*
 * aquaprio_draw: TWO launches.  The descent, one wavefront per sample (p, j): r = Philox4x32-10(key = seed[p], counter =
 * (j, t[p] + 1), stream AQUAPRIO_STREAM, attempt 0) in the layout of aquarpl_draw; u = umulhi64(r0 << 32 | r1, T_p) with T_p
 * the root; from the root down, lane l loads child l of the node, an inclusive prefix sum over the wavefront in uint64, the
 * first lane whose prefix exceeds u is the child to follow, and the prefix in front of it is taken off u.  The leaf reached
 * is mapped to its slot -> idx[p][j]; its q -> q_out[p][j].  T_p == 0: idx = -1, q_out = 0.  A leaf of 0 is never reached.
 * The weights, one block per network: beta_p = beta(t[p], beta0, anneal); size_p = (min(header[1], capacity) / N) w_p (at
 * least 1); w_j = weight(size_p, q_j, T_p, beta_p); weight[p][j] = (float)(w_j / max_j w_j), 0 for a sample without a slot.
 *   header            : the ring's int64 [4], 8-byte aligned (word 1, the size, is read)
 *   t_dev, seed_dev   : uint64 [P] each: the learner bank's update counters and seeds
 *   idx int32 [P][B], weight float32 [P][B], q_out uint32 [P][B] (scratch the weights are computed from)
 *   beta0 in [0, 1], anneal >= 1.  0 <= B <= AQUAPRIO_MAX_BATCH; B == 0 returns 0 without a launch.
 */
int aquaprio_draw(const void* tree, size_t tree_bytes, int64_t capacity, int64_t N, int64_t seg, int64_t P,
                  const int64_t* header, const uint64_t* t_dev, const uint64_t* seed_dev, int32_t* idx, float* weight,
                  uint32_t* q_out, int64_t B, double beta0, int64_t anneal, void* stream);

/*
 * aquaprio_update_f32: aqualbank_update_f32 with importance weights, TWO launches; the arguments, their rules and the
 * workspace (aqualbank_workspace_bytes(P, B) bytes, 16-byte aligned) are that entry's, and two more are REQUIRED:
 *   weight  : float32 [P][B], read: the TD error's derivative and its square in the loss are multiplied by weight[p][j]
 *   td_out  : float32 [P][B], written: |Q(s)[a] - y| of sample j (the plain TD error in both loss forms), -1 for what is no
 *             sample
 * With weight == 1 everything else it writes is aqualbank_update_f32's bit for bit.
 */
int aquaprio_update_f32(float* theta, float* theta_target, float* m, float* v, uint64_t* t_dev, int64_t P,
                        const float* s, const uint8_t* a, const float* r, const float* s2, const uint8_t* d,
                        const uint8_t* ok, int64_t ld, int64_t size,
                        const int32_t* idx, int64_t B, int strategy, const double* hyper_dev,
                        float* blob_online, float* blob_target, const int32_t* perm, int64_t blob_floats,
                        void* workspace, size_t workspace_bytes,
                        int32_t* idx_out, float* grad_out, float* loss,
                        const float* weight, float* td_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
