/*
 * aqua_render.h -- C ABI of libaqua_render.so: render(mode="rgb_array") for a batch of worlds on MI355X (gfx950), next to
 * the batched environment of aqua_hip.h.  One kernel rasterises the frames of M worlds; a second, one lane per world,
 * records what the reference keeps between step() and render(): the thrusts and the ICC of the last action.
 *
 * Reference being replaced: gym_aqua/envs/aqua.py:215-365 (the geometry handed to gym's viewer) and aqua.py:151-174 (the
 * thrusts and the ICC).  The viewer itself (gym's rendering.py, pyglet, GL) is not part of the reference tree; the scene
 * below is the specification (DESIGN.md "Frames on the device").
 *
 * Conventions are those of aqua_episodes.h:
 *  - plain pointers and sizes only (streams are void*); every DEVICE buffer is owned by the caller and borrowed until
 *    the work queued on `stream` has run; the library allocates nothing and keeps no pointer.
 *  - every entry is asynchronous on `stream`: ONE launch, no allocation, no synchronisation, no host read, so it may be
 *    captured into a HIP graph.  The same inputs give the same bytes, run to run, eager or replayed.
 *  - return value: 0 = ok; > 0 = hipError_t; < 0 = AQUARND_E_* (the values of AQUA_E_*).  The last-error entry returns a
 *    thread-local message for the last failing call on this thread.
 *  - every argument is validated before the first HIP call.  There is no CPU path.
 *
 * The scene.  A frame of side S pixels is uint8 [S][S][3], RGB; s = S / 100 (the reference: S = 500, view_scale = 5).
 * Row 0 is the TOP of the world.  The pixel in row i, column j is sampled at its centre P = (j + 0.5, S - 1 - i + 0.5) in
 * viewer coordinates (y up).  Background (255, 255, 255).  Opaque shapes, a later one overwrites an earlier one:
 *   1 obstacles in table order (38, 38, 38): circle = 30-gon of radius a s at (cx, cy) s; rectangle = the half-open box
 *     [cx - a/2, cx + a/2) x [cy - b/2, cy + b/2) times s, decided exactly (left / bottom edge in, right / top edge out)
 *   2 goal (0, 0, 204): 30-gon, radius 2.5 s, at goal s
 *   3 boat (0, 153, 102): 30-gon, radius 2.5 s, rotated by theta, at pos s
 *   4 left thrust bar (204, 26, 0): local x in [-1.875 s, -0.625 s], y in [0, 8 s] scaled by tl s, then the boat's
 *     rotation and translation; only if tl > 0
 *   5 right thrust bar: the same with x in [0.625 s, 1.875 s] and tr
 *   6 heading bar (102, 0, 26): local x in [-0.625 s, 0.625 s], y in [0, 2.5 s], boat transform
 *   7 ICC (102, 0, 26): 30-gon, radius 0.625 s, at icc s
 *   8 wave arrow body (0, 128, 166; only if waves): local x in [-s/2, s/2], y in [-8 s, 0] scaled by |wave s|, rotated
 *     by phi = atan2(wave_y, wave_x) - pi/2, translated to (4 s, 4 s); not drawn when wave == (0, 0)
 *   9 wave arrow tip (only if waves): triangle (-1.5 s, 0), (0, 1.5 s), (1.5 s, 0), rotated by phi, translated to (4 s, 4 s)
 * A 30-gon is gym's make_circle(r, res=30): vertices r (cos 2 pi k / 30, sin 2 pi k / 30).  A convex polygon covers P when
 * P is on the inner side of every edge.  Shape parameters are computed in float64 from the float32 inputs, the per-pixel
 * tests in float32: a pixel centre closer than ~1e-4 px to an edge (other than a rectangle obstacle's) may fall on either side.
 * A shape that lies outside the frame (the ICC of a straight action, 1.25e8 s px away) is dropped before the pixel loop.
 */
#ifndef AQUA_RENDER_H
#define AQUA_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQUARND_ABI_VERSION 1

/* library error codes (negative): the values of AQUA_E_* in aqua_hip.h */
#define AQUARND_E_INVALID   (-1)   /* bad argument (null pointer, negative size, value out of range ...) */
#define AQUARND_E_ALIGN     (-2)   /* pointer not usable */
#define AQUARND_E_NODEVICE  (-3)   /* reserved (the value of AQUA_E_NODEVICE): no entry of this library asks for a device before
                                      its launch, so a missing device comes back as the launch's positive hipError_t */

#define AQUARND_MAX_WORLDS  1073741824    /* N and M per call (2^30) */
#define AQUARND_MAX_BLOCKS  16777215      /* blocks of one frames launch (256 threads each: 2^32 - 1 threads at most) */
#define AQUARND_MAX_ROWS    64            /* K: obstacle rows per table */
#define AQUARND_MIN_SIZE    16            /* S: a multiple of 4 in [16, 1000] */
#define AQUARND_MAX_SIZE    1000
#define AQUARND_OVERLAY_ROWS 4            /* overlay rows: tl, tr, icc_x, icc_y */

int aquarnd_version(void);                /* AQUARND_ABI_VERSION */
const char* aquarnd_last_error(void);

/*
 * The overlay of the step ABOUT to be taken (call before the step launch): for world i < N, from the pose in state rows
 * 0..2 and its action, overlay[0][i] = tl, [1][i] = tr, [2][i] = icc_x, [3][i] = icc_y as aqua.py:151-174 computes them.
 *   state      : float32 [7][ld] (aqua_hip.h), 4-byte aligned; ld >= N
 *   action     : _u8: uint8 [N], the step's table (0: (0.2, 0.5), 1: (0.5, 0.2), 2 and above: (0.5, 0.5));
 *                _f32x2: float32 [2][action_ld] thrusts, clipped to [0.2, 0.5] in float32 as the step clips them
 *   overlay    : float32 [4][overlay_ld], 4-byte aligned; overlay_ld >= N
 * thrust_diff = copysign(max(|tr - tl|, 1e-8), tr - tl) and r = 1.25 (tr + tl) / thrust_diff in float64 (a straight action
 * gives the reference's ICC 1.25e8 away, not an infinity); icc = pos + r (-sin(pi/2 + theta), cos(pi/2 + theta)), rounded
 * to float32 once.  N == 0 returns 0 without a launch.
 */
int aquarnd_overlay_u8(const float* state, int64_t ld, int64_t N, const uint8_t* action, float* overlay, int64_t overlay_ld,
                       void* stream);
int aquarnd_overlay_f32x2(const float* state, int64_t ld, int64_t N, const float* action, int64_t action_ld, float* overlay,
                          int64_t overlay_ld, void* stream);

/*
 * Frames of M worlds.  All pointers are DEVICE pointers.
 *   state, ld, N : as above
 *   overlay      : nullable float32 [4][overlay_ld]; NULL = all four 0, the reference after its constructor and reset():
 *                  no thrust bars, the ICC at the origin (a quarter of its circle shows in the bottom-left corner)
 *   rows         : float32 [K][5] (per_world == 0) or [N][K][5] (per_world != 0), rows (cx, cy, kind, a, b) as
 *                  aquaticgymenv_amd/presets.py: kind 0 circle of radius a, kind > 0 rectangle a x b, kind < 0 absent;
 *                  0 <= K <= AQUARND_MAX_ROWS; may be NULL when K == 0
 *   waves        : 0 = no wave arrow, anything else = the arrow of state rows 5..6
 *   worlds       : nullable int32 [M]: frame m shows world worlds[m]; NULL = world m (then M <= N).  An entry outside
 *                  [0, N) gives an all-zero (black) frame and reads nothing.
 *   S            : a multiple of 4 in [AQUARND_MIN_SIZE, AQUARND_MAX_SIZE]
 *   out          : uint8 [M][S][S][3], 4-byte aligned; out_bytes >= 3 M S S (checked before the launch)
 * One launch of M x tiles blocks, tiles = ceil(S / rows per tile) <= S, rows per tile chosen from (M, S) (S <= 20: always one
 * tile per frame; S = 64: one from M = 2 048 on; S = 1000 and many frames: 125).  More than AQUARND_MAX_BLOCKS blocks (the
 * launch limit of 2^32 - 1 threads; 16.7 M frames of S = 16, 134 217 of S = 1000) is AQUARND_E_INVALID: draw such a batch in
 * several calls.
 * Sizes and alignment are checked first; then M == 0 or N == 0 (no frame, or no world to show) returns 0 without a launch
 * and without looking at the pointers.
 */
int aquarnd_frames_u8(const float* state, int64_t ld, int64_t N, const float* overlay, int64_t overlay_ld,
                      const float* rows, int K, int per_world, int waves,
                      const int32_t* worlds, int64_t M, int S, uint8_t* out, size_t out_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
