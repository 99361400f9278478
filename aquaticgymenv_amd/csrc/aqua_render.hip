// aqua_render.hip -- libaqua_render.so (include/aqua_render.h): render(mode="rgb_array") of gym_aqua/envs/aqua.py:215-365 for
// a batch of worlds on gfx950: uint8 [M][S][S][3] frames drawn by one kernel, and the one-lane-per-world kernel that records
// the thrusts and the ICC of the action about to be stepped (aqua.py:151-174).
// Its own translation unit and library: the other four libraries and their kernels are not touched by it.
//
// The frame kernel (DESIGN.md "Frames on the device") is a stream of 3 S S bytes per frame with a little geometry in front:
//   - a block owns a tile of whole rows of one frame: a contiguous run of bytes.  The host picks the rows per tile from
//     (M, S): about 256 pixel quads when there are few frames (M = 1, S = 500: 250 blocks), up to 2 048 quads when there
//     are many (the list below is then built once per eight quads of a lane).
//   - wave 0 builds the world's primitive list in LDS, in pixel space and in draw order: obstacles (one lane per row of
//     the table), then goal, boat, thrust bars, heading bar, ICC, wave arrow (one lane per shape).  Parameters are worked
//     out in float64 from the float32 inputs and rounded once.  A primitive whose bounding box misses the tile's rows or
//     the frame is dropped by a ballot: the list a pixel walks holds what can touch its tile, in order.
//   - a lane owns four consecutive pixels of a row and stores them as three dwords (12 bytes); a wave's stores are one
//     contiguous run of 768 bytes.  No byte stores.
//   - every primitive carries the box of pixels it can touch; a wave none of whose 64 quads (256 pixels of a row at S = 500,
//     four rows at S = 64) meets that box skips it: one scalar-operand compare per primitive instead of its test.
//   - a 30-gon (gym's make_circle) is decided by its inscribed and circumscribed circles; only a wave with a pixel in the
//     thin ring between them runs the edges, folded by the polygon's symmetries to eight terms.
//   - a rectangle obstacle is decided in integers (the half-open rule, exact); the bars and the arrow by edge functions.
#include <hip/hip_runtime.h>

#include "../../include/aqua_render.h"
#include "aqua_device.hpp"
#include "aqua_host.hpp"

namespace {

using aqua::any_lane;
using aqua::sincos_f64;

constexpr int BLOCK = 256;
constexpr int DYNAMIC = 8;                                   // goal, boat, two thrust bars, heading bar, ICC, arrow body, arrow tip
constexpr int MAX_PRIMS = AQUARND_MAX_ROWS + DYNAMIC;
constexpr int QUADS_PER_TILE = 256, MAX_TILE_FACTOR = 8, TARGET_BLOCKS = 2048;

enum : int { P_RECT = 0, P_NGON = 1, P_POLY = 2 };

constexpr uint32_t rgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }
constexpr uint32_t WHITE = rgb(255, 255, 255), C_OBSTACLE = rgb(38, 38, 38), C_GOAL = rgb(0, 0, 204), C_BOAT = rgb(0, 153, 102),
                   C_THRUST = rgb(204, 26, 0), C_DIRECTION = rgb(102, 0, 26), C_WAVE = rgb(0, 128, 166);

// The 30 edge normals of make_circle(r, res=30) are (cos, sin) of 2 pi (k + 1/2) / 30.  They come in pairs +-n and
// mirrored in x, and one of them is (0, 1): max_k n_k . l = max(|l_y|, max_{k < 7} (NX[k] |l_x| + NY[k] |l_y|)).
constexpr float NX[7] = {0x1.fd31fap-1f, 0x1.e6f0e2p-1f, 0x1.bb67aep-1f, 0x1.7c7d7ap-1f, 0x1.2cf230p-1f, 0x1.a07f92p-2f, 0x1.a9cd9ap-3f};
constexpr float NY[7] = {0x1.ac260ap-4f, 0x1.3c6ef4p-2f, 0x1.000000p-1f, 0x1.56984ap-1f, 0x1.9e377ap-1f, 0x1.d3bc3ap-1f, 0x1.f4cfc4p-1f};
constexpr double APOTHEM = 0x1.fd31f94f867c6p-1;             // cos(pi / 30)
// the two circles are moved apart by this much (relative), so that their float32 verdict never contradicts the edges'
constexpr double RING_SLACK = 1.0e-5;

// One primitive: 16 dwords of LDS; i[12..13]: set_reach().  P_RECT: i[0..3] = j0, j1, y0, y1 (columns and rows-from-the-bottom covered: [j0, j1) x [y0, y1)).
// P_NGON: f[0..5] = cx, cy, cos, sin, apothem, inner radius^2; f[6] = outer radius^2.  P_POLY: f[3 e + 0..2] = a, b, c of edge
// e < 4: inside iff a x + b y + c >= 0 for all four.
struct Prim {
    int type;
    uint32_t color;
    union {
        float f[14];
        int i[14];
    };
};
static_assert(sizeof(Prim) == 64, "one primitive is four ds_read_b128");

struct FrameArgs {
    const float* state;
    const float* overlay;
    const float* rows;
    const int32_t* worlds;
    uint8_t* out;
    int64_t ld, N, overlay_ld;
    int K, per_world, waves, S, rows_per_tile, tiles;
};

struct OverlayArgs {
    const float* state;
    const void* action;
    float* overlay;
    int64_t ld, N, action_ld, overlay_ld;
};

__device__ __forceinline__ uint32_t rank_in(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

struct Box { double x0, x1, y0, y1; };

__device__ __forceinline__ Prim make_ngon(double cx, double cy, double r, double cs, double sn, uint32_t color, Box& box)
{
    Prim p;
    p.type = P_NGON; p.color = color;
    const double apo = r * APOTHEM, in = apo * (1.0 - RING_SLACK), out = r * (1.0 + RING_SLACK);
    p.f[0] = static_cast<float>(cx); p.f[1] = static_cast<float>(cy);
    p.f[2] = static_cast<float>(cs); p.f[3] = static_cast<float>(sn);
    p.f[4] = static_cast<float>(apo); p.f[5] = static_cast<float>(in * in); p.f[6] = static_cast<float>(out * out);
    box.x0 = cx - r; box.x1 = cx + r; box.y0 = cy - r; box.y1 = cy + r;
    return p;
}

// edge e of a polygon given in its local frame as nx lx + ny ly + d >= 0, local = R(-angle) (P - t)
__device__ __forceinline__ void set_edge(Prim& p, int e, double nx, double ny, double d, double cs, double sn, double tx, double ty)
{
    const double a = nx * cs - ny * sn, b = nx * sn + ny * cs;
    p.f[3 * e + 0] = static_cast<float>(a);
    p.f[3 * e + 1] = static_cast<float>(b);
    p.f[3 * e + 2] = static_cast<float>(d - (a * tx + b * ty));
}

__device__ __forceinline__ void grow(Box& box, double lx, double ly, double cs, double sn, double tx, double ty)
{
    const double x = cs * lx - sn * ly + tx, y = sn * lx + cs * ly + ty;
    box.x0 = fmin(box.x0, x); box.x1 = fmax(box.x1, x); box.y0 = fmin(box.y0, y); box.y1 = fmax(box.y1, y);
}

// the local box [xl, xr] x [yb, yt], or with tri the triangle (xl, 0), (0, yt), (xr, 0) (xl = -xr, yt = xr), under rotation and translation
__device__ __forceinline__ Prim make_poly(bool tri, double xl, double xr, double yb, double yt, double cs, double sn, double tx, double ty,
                                          uint32_t color, Box& box)
{
    constexpr double R2 = 0x1.6a09e667f3bcdp-1;              // 1 / sqrt(2)
    Prim p;
    p.type = P_POLY; p.color = color;
    set_edge(p, 0, 0.0, 1.0, -yb, cs, sn, tx, ty);
    if (tri) {
        set_edge(p, 1, R2, -R2, yt * R2, cs, sn, tx, ty);
        set_edge(p, 2, -R2, -R2, yt * R2, cs, sn, tx, ty);
        p.f[9] = 0.0f; p.f[10] = 0.0f; p.f[11] = 1.0f;
    } else {
        set_edge(p, 1, 1.0, 0.0, -xl, cs, sn, tx, ty);
        set_edge(p, 2, -1.0, 0.0, xr, cs, sn, tx, ty);
        set_edge(p, 3, 0.0, -1.0, yt, cs, sn, tx, ty);
    }
    box.x0 = box.y0 = 1.0e300; box.x1 = box.y1 = -1.0e300;
    grow(box, xl, yb, cs, sn, tx, ty);
    grow(box, xr, yb, cs, sn, tx, ty);
    grow(box, tri ? 0.0 : xl, yt, cs, sn, tx, ty);
    grow(box, tri ? 0.0 : xr, yt, cs, sn, tx, ty);
    return p;
}

// the pixels a primitive can touch, as two dwords: i[12] = first | last << 16 row-from-the-bottom, i[13] the same for columns
// (one pixel of slack on every side, clamped to the frame): a wave none of whose quads meets that box skips the primitive
__device__ __forceinline__ void set_reach(Prim& p, double x0, double x1, double y0, double y1, int S)
{
    const double last = S - 1;
    const uint32_t j0 = static_cast<uint32_t>(fmin(fmax(floor(x0) - 1.0, 0.0), last)), j1 = static_cast<uint32_t>(fmin(fmax(ceil(x1) + 1.0, 0.0), last));
    const uint32_t r0 = static_cast<uint32_t>(fmin(fmax(floor(y0) - 1.0, 0.0), last)), r1 = static_cast<uint32_t>(fmin(fmax(ceil(y1) + 1.0, 0.0), last));
    p.i[12] = static_cast<int>(r0 | (r1 << 16));
    p.i[13] = static_cast<int>(j0 | (j1 << 16));
}

// four pixels of one row as three dwords: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
struct __attribute__((aligned(4))) Quad { uint32_t a, b, c; };

__global__ __launch_bounds__(BLOCK) void rnd_frames_kernel(const FrameArgs a)
{
    __shared__ Prim s_prim[MAX_PRIMS];
    __shared__ int s_count;

    const uint32_t m = blockIdx.x / static_cast<uint32_t>(a.tiles), tile = blockIdx.x - m * static_cast<uint32_t>(a.tiles);
    const int S = a.S;
    const int r0 = static_cast<int>(tile) * a.rows_per_tile;                       // image rows [r0, r1), row 0 on top
    const int r1 = r0 + a.rows_per_tile < S ? r0 + a.rows_per_tile : S;
    const int64_t w = a.worlds != nullptr ? static_cast<int64_t>(a.worlds[m]) : static_cast<int64_t>(m);
    const bool valid = w >= 0 && w < a.N;                                          // block-uniform

    if (threadIdx.x < 64) {
        int n = 0;
        if (valid) {
            const int lane = threadIdx.x;
            const double s = static_cast<double>(S) / 100.0;
            // rows-from-the-bottom of the tile's pixel centres, and the same as viewer y, with a pixel of slack
            const int yy0 = S - r1, yy1 = S - r0;                                  // [yy0, yy1)
            const double ylo = yy0 - 0.5, yhi = yy1 + 0.5, xlo = -1.0, xhi = S + 1.0;

            // ---- obstacles, in table order
            {
                bool keep = false;
                Prim p;
                if (lane < a.K) {
                    const float* row = a.rows + ((a.per_world ? w * a.K : 0) + lane) * 5;
                    const double cx = row[0], cy = row[1], kind = row[2], da = row[3], db = row[4];
                    if (kind == 0.0) {
                        Box box;
                        p = make_ngon(cx * s, cy * s, da * s, 1.0, 0.0, C_OBSTACLE, box);
                        set_reach(p, box.x0, box.x1, box.y0, box.y1, S);
                        keep = box.y1 >= ylo && box.y0 <= yhi && box.x1 >= xlo && box.x0 <= xhi;
                    } else if (kind > 0.0) {
                        // centre j + 0.5 is covered iff x0 <= j + 0.5 < x1 iff ceil(x0 - 0.5) <= j < ceil(x1 - 0.5); the bounds
                        // round where the reference's float64 expressions round: no contraction
#pragma clang fp contract(off)
                        const double lim = S;
                        const double j0 = fmin(fmax(ceil((cx - da / 2) * s - 0.5), 0.0), lim), j1 = fmin(fmax(ceil((cx + da / 2) * s - 0.5), 0.0), lim);
                        const double y0 = fmin(fmax(ceil((cy - db / 2) * s - 0.5), 0.0), lim), y1 = fmin(fmax(ceil((cy + db / 2) * s - 0.5), 0.0), lim);
                        p.type = P_RECT; p.color = C_OBSTACLE;
                        p.i[0] = static_cast<int>(j0); p.i[1] = static_cast<int>(j1);
                        p.i[2] = static_cast<int>(y0); p.i[3] = static_cast<int>(y1);
                        set_reach(p, j0, j1, y0, y1, S);
                        keep = p.i[0] < p.i[1] && p.i[2] < p.i[3] && p.i[3] > yy0 && p.i[2] < yy1;
                    }
                }
                const uint64_t mask = __builtin_amdgcn_ballot_w64(keep);
                if (keep) s_prim[rank_in(mask)] = p;
                n = __builtin_popcountll(mask);
            }

            // ---- the world's own shapes: one lane each, in draw order
            {
                bool keep = false;
                Prim p;
                if (lane < DYNAMIC) {
                    const float* st = a.state + w;
                    const double x = st[0], y = st[a.ld], th = st[2 * a.ld], gx = st[3 * a.ld], gy = st[4 * a.ld];
                    const double wx = st[5 * a.ld], wy = st[6 * a.ld];
                    double tl = 0.0, tr = 0.0, ix = 0.0, iy = 0.0;
                    if (a.overlay != nullptr) {
                        const float* ov = a.overlay + w;
                        tl = ov[0]; tr = ov[a.overlay_ld]; ix = ov[2 * a.overlay_ld]; iy = ov[3 * a.overlay_ld];
                    }
                    Box box;
                    bool drawn = true;
                    if (lane == 0 || lane == 1 || lane == 5) {
                        double cs = 1.0, sn = 0.0;
                        if (lane == 1) sincos_f64(th, sn, cs);
                        const double cx = lane == 0 ? gx : (lane == 1 ? x : ix), cy = lane == 0 ? gy : (lane == 1 ? y : iy);
                        const double r = lane == 5 ? 0.625 : 2.5;
                        p = make_ngon(cx * s, cy * s, r * s, cs, sn, lane == 0 ? C_GOAL : (lane == 1 ? C_BOAT : C_DIRECTION), box);
                    } else if (lane < 5) {
                        // thrust bars and heading bar: the boat's rotation and translation (aqua.py:284-310, 343-354)
                        double cs, sn;
                        sincos_f64(th, sn, cs);
                        const double thrust = lane == 2 ? tl : tr;
                        const double xl = lane == 2 ? -1.875 * s : (lane == 3 ? 0.625 * s : -0.625 * s);
                        const double yt = lane == 4 ? 2.5 * s : (8.0 * s) * (thrust * s);
                        drawn = lane == 4 || thrust > 0.0;
                        p = make_poly(false, xl, xl + 1.25 * s, 0.0, yt, cs, sn, x * s, y * s, lane == 4 ? C_DIRECTION : C_THRUST, box);
                    } else {
                        // wave arrow (aqua.py:319-335, 360-363): phi = atan2(wy, wx) - pi/2, so cos phi = wy / |w|, sin phi = -wx / |w|
                        const double vx = wx * s, vy = wy * s, len = sqrt(vx * vx + vy * vy);
                        const double cs = len > 0.0 ? vy / len : 0.0, sn = len > 0.0 ? -vx / len : -1.0;
                        drawn = a.waves != 0 && (lane == 7 || len > 0.0);
                        if (lane == 6) p = make_poly(false, -0.5 * s, 0.5 * s, (-8.0 * s) * len, 0.0, cs, sn, 4.0 * s, 4.0 * s, C_WAVE, box);
                        else p = make_poly(true, -1.5 * s, 1.5 * s, 0.0, 1.5 * s, cs, sn, 4.0 * s, 4.0 * s, C_WAVE, box);
                    }
                    set_reach(p, box.x0, box.x1, box.y0, box.y1, S);
                    keep = drawn && box.y1 >= ylo && box.y0 <= yhi && box.x1 >= xlo && box.x0 <= xhi;
                }
                const uint64_t mask = __builtin_amdgcn_ballot_w64(keep);
                if (keep) s_prim[n + rank_in(mask)] = p;
                n += __builtin_popcountll(mask);
            }
        }
        if (threadIdx.x == 0) s_count = n;
    }
    __syncthreads();

    const int n = __builtin_amdgcn_readfirstlane(s_count);
    const uint32_t base = valid ? WHITE : 0u;
    const uint32_t qw = static_cast<uint32_t>(S) >> 2;                             // quads per row
    const uint32_t q_end = static_cast<uint32_t>(r1) * qw;
    Quad* frame = reinterpret_cast<Quad*>(a.out + static_cast<size_t>(m) * 3u * static_cast<size_t>(S) * static_cast<size_t>(S));

    for (uint32_t q = static_cast<uint32_t>(r0) * qw + threadIdx.x; q < q_end; q += BLOCK) {
        const uint32_t i = q / qw;
        const int j = static_cast<int>(q - i * qw) << 2, yy = S - 1 - static_cast<int>(i);
        const float px = static_cast<float>(j) + 0.5f, py = static_cast<float>(yy) + 0.5f;
        uint32_t c0 = base, c1 = base, c2 = base, c3 = base;
        for (int k = 0; k < n; ++k) {
            const Prim& p = s_prim[k];
            const int type = __builtin_amdgcn_readfirstlane(p.type);
            const uint32_t reach_y = __builtin_amdgcn_readfirstlane(p.i[12]), reach_x = __builtin_amdgcn_readfirstlane(p.i[13]);
            const int y_lo = reach_y & 0xffffu, y_hi = reach_y >> 16, j_lo = reach_x & 0xffffu, j_hi = reach_x >> 16;
            if (!any_lane(yy >= y_lo && yy <= y_hi && j + 3 >= j_lo && j <= j_hi)) continue;
            const uint32_t color = p.color;
            bool h0, h1, h2, h3;
            if (type == P_RECT) {
                const int j0 = p.i[0], j1 = p.i[1];
                const bool row = yy >= p.i[2] && yy < p.i[3];
                h0 = row && j >= j0 && j < j1;
                h1 = row && j + 1 >= j0 && j + 1 < j1;
                h2 = row && j + 2 >= j0 && j + 2 < j1;
                h3 = row && j + 3 >= j0 && j + 3 < j1;
            } else if (type == P_NGON) {
                const float dx = px - p.f[0], dy = py - p.f[1], in2 = p.f[5], out2 = p.f[6];
                const float dy2 = dy * dy;
                const float d0 = fmaf(dx, dx, dy2), d1 = fmaf(dx + 1.0f, dx + 1.0f, dy2);
                const float d2 = fmaf(dx + 2.0f, dx + 2.0f, dy2), d3 = fmaf(dx + 3.0f, dx + 3.0f, dy2);
                h0 = d0 <= in2; h1 = d1 <= in2; h2 = d2 <= in2; h3 = d3 <= in2;
                const bool g0 = !h0 && d0 < out2, g1 = !h1 && d1 < out2, g2 = !h2 && d2 < out2, g3 = !h3 && d3 < out2;
                if (any_lane(g0 || g1 || g2 || g3)) {
                    // the ring between the two circles: the edges decide, in the polygon's own frame
                    const float cs = p.f[2], sn = p.f[3], apo = p.f[4];
                    const float lx0 = fmaf(cs, dx, sn * dy), ly0 = fmaf(-sn, dx, cs * dy);
                    bool e[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const float ax = fabsf(fmaf(cs, static_cast<float>(t), lx0)), ay = fabsf(fmaf(-sn, static_cast<float>(t), ly0));
                        float far = ay;
#pragma unroll
                        for (int v = 0; v < 7; ++v) far = fmaxf(far, fmaf(NX[v], ax, NY[v] * ay));
                        e[t] = far <= apo;
                    }
                    h0 = h0 || (g0 && e[0]); h1 = h1 || (g1 && e[1]); h2 = h2 || (g2 && e[2]); h3 = h3 || (g3 && e[3]);
                }
            } else {
                h0 = h1 = h2 = h3 = true;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float ea = p.f[3 * e], row = fmaf(p.f[3 * e + 1], py, p.f[3 * e + 2]);
                    h0 = h0 && fmaf(ea, px, row) >= 0.0f;
                    h1 = h1 && fmaf(ea, px + 1.0f, row) >= 0.0f;
                    h2 = h2 && fmaf(ea, px + 2.0f, row) >= 0.0f;
                    h3 = h3 && fmaf(ea, px + 3.0f, row) >= 0.0f;
                }
            }
            c0 = h0 ? color : c0; c1 = h1 ? color : c1; c2 = h2 ? color : c2; c3 = h3 ? color : c3;
        }
        Quad out;
        out.a = c0 | (c1 << 24);
        out.b = (c1 >> 8) | (c2 << 16);
        out.c = (c2 >> 16) | (c3 << 8);
        frame[q] = out;
    }
}

// tl, tr and the ICC of the action about to be stepped (aqua.py:151-174); U8: the action is an index into the step's table
template <bool U8> __global__ __launch_bounds__(BLOCK) void rnd_overlay_kernel(const OverlayArgs a)
{
#pragma clang fp contract(off)
    const int64_t i = static_cast<int64_t>(blockIdx.x) * BLOCK + threadIdx.x;
    if (i >= a.N) return;
    float tl, tr;
    double r;
    if constexpr (U8) {
        const uint32_t idx = static_cast<const uint8_t*>(a.action)[i];
        tl = idx == 0 ? 0.2f : 0.5f;
        tr = idx == 1 ? 0.2f : 0.5f;
        r = aqua::exact_motion_discrete(idx > 2 ? 2 : static_cast<int>(idx)).r;
    } else {
        const float* act = static_cast<const float*>(a.action);
        tl = fminf(fmaxf(act[i], 0.2f), 0.5f);
        tr = fminf(fmaxf(act[a.action_ld + i], 0.2f), 0.5f);
        double diff = static_cast<double>(tr) - static_cast<double>(tl);
        diff = copysign(fmax(fabs(diff), 1e-8), diff);
        r = 2.5 / 2 * (static_cast<double>(tr) + static_cast<double>(tl)) / diff;
    }
    const double x = a.state[i], y = a.state[a.ld + i], th = a.state[2 * a.ld + i];
    double sn, cs;
    sincos_f64(0x1.921fb54442d18p+0 + th, sn, cs);
    a.overlay[i] = tl;
    a.overlay[a.overlay_ld + i] = tr;
    a.overlay[2 * a.overlay_ld + i] = static_cast<float>(x + r * -sn);
    a.overlay[3 * a.overlay_ld + i] = static_cast<float>(y + r * cs);
}

int check_overlay(const float* state, int64_t ld, int64_t N, const void* action, size_t action_align, int64_t action_ld, float* overlay,
                  int64_t overlay_ld)
{
    if (N < 0 || N > AQUARND_MAX_WORLDS) return fail(AQUARND_E_INVALID, "N=%lld: must be in [0, %d]", (long long)N, AQUARND_MAX_WORLDS);
    if (!aligned(state, 4) || !aligned(overlay, 4) || !aligned(action, action_align))
        return fail(AQUARND_E_ALIGN, "state / overlay / thrusts must be 4-byte aligned");
    if (N == 0) return 0;
    if (state == nullptr || action == nullptr || overlay == nullptr) return fail(AQUARND_E_INVALID, "state, action or overlay is NULL");
    if (ld < N || overlay_ld < N || action_ld < N)
        return fail(AQUARND_E_INVALID, "ld=%lld, overlay_ld=%lld, action_ld=%lld: each must be >= N=%lld", (long long)ld, (long long)overlay_ld,
                    (long long)action_ld, (long long)N);
    return 1;                                                // launch
}

template <bool U8> int launch_overlay(const float* state, int64_t ld, int64_t N, const void* action, int64_t action_ld, float* overlay,
                                      int64_t overlay_ld, void* stream)
{
    OverlayArgs k;
    k.state = state; k.action = action; k.overlay = overlay; k.ld = ld; k.N = N; k.action_ld = action_ld; k.overlay_ld = overlay_ld;
    const unsigned blocks = static_cast<unsigned>((N + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(rnd_overlay_kernel<U8>, dim3(blocks), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), k);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "rnd_overlay_kernel launch");
    return 0;
}

}  // namespace

extern "C" {

int aquarnd_version(void) { return AQUARND_ABI_VERSION; }
const char* aquarnd_last_error(void) { return g_err; }

int aquarnd_overlay_u8(const float* state, int64_t ld, int64_t N, const uint8_t* action, float* overlay, int64_t overlay_ld, void* stream)
{
    const int rc = check_overlay(state, ld, N, action, 1, N, overlay, overlay_ld);
    return rc == 1 ? launch_overlay<true>(state, ld, N, action, 0, overlay, overlay_ld, stream) : rc;
}

int aquarnd_overlay_f32x2(const float* state, int64_t ld, int64_t N, const float* action, int64_t action_ld, float* overlay,
                          int64_t overlay_ld, void* stream)
{
    const int rc = check_overlay(state, ld, N, action, 4, action_ld, overlay, overlay_ld);
    return rc == 1 ? launch_overlay<false>(state, ld, N, action, action_ld, overlay, overlay_ld, stream) : rc;
}

int aquarnd_frames_u8(const float* state, int64_t ld, int64_t N, const float* overlay, int64_t overlay_ld,
                      const float* rows, int K, int per_world, int waves,
                      const int32_t* worlds, int64_t M, int S, uint8_t* out, size_t out_bytes, void* stream)
{
    if (N < 0 || N > AQUARND_MAX_WORLDS) return fail(AQUARND_E_INVALID, "N=%lld: must be in [0, %d]", (long long)N, AQUARND_MAX_WORLDS);
    if (M < 0 || M > AQUARND_MAX_WORLDS) return fail(AQUARND_E_INVALID, "M=%lld: must be in [0, %d]", (long long)M, AQUARND_MAX_WORLDS);
    if (S < AQUARND_MIN_SIZE || S > AQUARND_MAX_SIZE || S % 4 != 0)
        return fail(AQUARND_E_INVALID, "S=%d: must be a multiple of 4 in [%d, %d]", S, AQUARND_MIN_SIZE, AQUARND_MAX_SIZE);
    if (K < 0 || K > AQUARND_MAX_ROWS) return fail(AQUARND_E_INVALID, "K=%d: must be in [0, %d]", K, AQUARND_MAX_ROWS);
    if (!aligned(state, 4) || !aligned(overlay, 4) || !aligned(rows, 4) || !aligned(worlds, 4) || !aligned(out, 4))
        return fail(AQUARND_E_ALIGN, "state / overlay / rows / worlds / out must be 4-byte aligned");
    if (M == 0 || N == 0) return 0;
    if (state == nullptr || out == nullptr) return fail(AQUARND_E_INVALID, "state or out is NULL");
    if (rows == nullptr && K > 0) return fail(AQUARND_E_INVALID, "rows is NULL with K=%d", K);
    if (ld < N) return fail(AQUARND_E_INVALID, "ld=%lld < N=%lld", (long long)ld, (long long)N);
    if (overlay != nullptr && overlay_ld < N) return fail(AQUARND_E_INVALID, "overlay_ld=%lld < N=%lld", (long long)overlay_ld, (long long)N);
    if (worlds == nullptr && M > N) return fail(AQUARND_E_INVALID, "M=%lld frames of N=%lld worlds need a worlds list", (long long)M, (long long)N);
    const size_t frame = 3u * static_cast<size_t>(S) * static_cast<size_t>(S);
    if (out_bytes / frame < static_cast<size_t>(M))
        return fail(AQUARND_E_INVALID, "out_bytes=%zu < 3 M S S = %zu", out_bytes, frame * static_cast<size_t>(M));

    // rows per tile: about QUADS_PER_TILE quads, more (up to MAX_TILE_FACTOR times) once there are TARGET_BLOCKS blocks anyway
    const int qw = S / 4;
    int base_rows = QUADS_PER_TILE / qw;
    base_rows = base_rows < 1 ? 1 : (base_rows > S ? S : base_rows);
    const int64_t base_tiles = (S + base_rows - 1) / base_rows;
    int64_t factor = M * base_tiles / TARGET_BLOCKS;
    factor = factor < 1 ? 1 : (factor > MAX_TILE_FACTOR ? MAX_TILE_FACTOR : factor);
    const int64_t rows_per_tile = base_rows * factor > S ? S : base_rows * factor;
    const int64_t tiles = (S + rows_per_tile - 1) / rows_per_tile;
    if (M * tiles > AQUARND_MAX_BLOCKS)
        return fail(AQUARND_E_INVALID, "M=%lld frames of S=%d are %lld blocks, more than %d: draw them in several calls", (long long)M, S,
                    (long long)(M * tiles), AQUARND_MAX_BLOCKS);

    FrameArgs k;
    k.state = state; k.overlay = overlay; k.rows = rows; k.worlds = worlds; k.out = out;
    k.ld = ld; k.N = N; k.overlay_ld = overlay_ld;
    k.K = K; k.per_world = per_world; k.waves = waves; k.S = S;
    k.rows_per_tile = static_cast<int>(rows_per_tile); k.tiles = static_cast<int>(tiles);
    hipLaunchKernelGGL(rnd_frames_kernel, dim3(static_cast<unsigned>(M * tiles)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), k);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "rnd_frames_kernel launch");
    return 0;
}

}  // extern "C"
