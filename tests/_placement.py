"""Where a world is placed: the reference's acceptance predicates and its reset as plain float64 numpy, a third statement
of this build's float32 reset specification that says WHICH attempt it stopped at, and worlds crowded enough that the
rare branches of the device's placement loop (reset_env_group, aqua_device.hpp) are the common case.  Imports without a
GPU.

The device does not run the serial loop of the specification (oracle/aqua_oracle.c, reset_world): it spreads the
attempts of one world over G lanes and keeps the lowest accepted attempt of a round of G.  A goal found only in a later
round, a boat found in a later round, exhausted goal or boat attempts each take a path of their own there, and with the
acceptance of the suite's other tables (a half or more) a restart in thousands, or none, takes them.  The tables here
are walls: m vertical strips side by side that leave a band of `free` units at the right border, so that a candidate is
accepted with p = free / 95, and is rejected by the one strip it falls in -- every present row decides some attempts.

tests/test_placement_cpu.py ties the specification to the reference's distribution and checks these constructions on
the CPU; tests/test_crowded_restarts.py runs the cells on the GPU.
"""
import collections
import zlib

import numpy as np

from tests import _dispatch as D
from tests import _options as O
from tests.test_dispatch_matrix import T, SEED, _stored_actions

C = D.C
G = C["RESET_GROUP"]                   # lanes that share the attempts of one world (== NS_RESEED_GROUP, checked on the CPU)
TRIES = C["RESET_TRIES"]               # attempts per goal and per boat; index TRIES means "exhausted"
STREAM_PLACE, STREAM_POSE = 1, 3       # oracle/aqua_oracle.c, the stream ids
MARGIN_BAR = -2e-5                     # an accepted placement's margins, evaluated in float64 on the float32 placement
_M32 = np.uint64(0xFFFFFFFF)
_f32, _f64 = np.float32, np.float64

MARGINS = ("goal_border", "goal_obstacle", "boat_goal", "boat_border", "boat_obstacle")
GOAL_MARGINS, BOAT_MARGINS = (0, 1), (2, 3, 4)


# ------------------------------------------------------------------------------------------------ the reference's predicates
def _rows(obstacles):
    o = np.asarray(obstacles, dtype=_f64)
    if o.size == 0:
        return np.zeros((0, 5))
    assert o.shape[-1] == 5 and o.ndim in (2, 3)
    return o


def obstacle_margin(px, py, obstacles, radius=2.5):
    """signed distance from the circle (px, py, radius) to the nearest obstacle, float64, in the reference's operation
    order: a circle row (kind 0): |c - p| - (r + radius); a rectangle row: |p - clip(p, lo, hi)| - radius.  Rows with
    kind < 0 are absent; +inf where no row is present.  obstacles [K][5] (one table) or [n][K][5]."""
    o = _rows(obstacles)
    px, py = np.asarray(px, dtype=_f64), np.asarray(py, dtype=_f64)
    out = np.full(px.shape, np.inf)
    if o.shape[-2] == 0:
        return out
    f = (lambda c: o[:, c][None, :]) if o.ndim == 2 else (lambda c: o[:, :, c])
    cx, cy, kind, a, b = (f(c) for c in range(5))
    x, y = px[:, None], py[:, None]
    dx, dy = cx - x, cy - y
    circle = np.sqrt(dx * dx + dy * dy) - (a + radius)
    left, right, bottom, top = cx - a / 2, cx + a / 2, cy - b / 2, cy + b / 2
    ex, ey = x - np.clip(x, left, right), y - np.clip(y, bottom, top)
    rect = np.sqrt(ex * ex + ey * ey) - radius
    d = np.where(kind == 0, circle, rect)
    d = np.where(kind < 0, np.inf, d)
    return np.minimum(out, d.min(axis=1))


def border_margin(px, py, radius=2.5):
    """min over the four sides; the reference rejects p - r < 0 and p + r > 100, i.e. a margin < 0"""
    px, py = np.asarray(px, dtype=_f64), np.asarray(py, dtype=_f64)
    return np.minimum(np.minimum(px - radius, py - radius), np.minimum(100.0 - (px + radius), 100.0 - (py + radius)))


def goal_margin(px, py, gx, gy, total_radius=5.0):
    dx, dy = np.asarray(gx, dtype=_f64) - px, np.asarray(gy, dtype=_f64) - py
    return np.sqrt(dx * dx + dy * dy) - total_radius


def acceptance_margins(state, obstacles):
    """float64 [5][n] (MARGINS): goal to border, goal to nearest obstacle, boat to goal (centre distance - 5), boat to
    border, boat to nearest obstacle, of the placement state [>=5][n] (x, y, heading, gx, gy, ...) read as float64.  The
    reference accepts a placement whose obstacle and goal margins are > 0 and whose border margins are >= 0."""
    s = np.asarray(state).astype(_f64)
    x, y, gx, gy = s[0], s[1], s[3], s[4]
    return np.stack([border_margin(gx, gy), obstacle_margin(gx, gy, obstacles), goal_margin(x, y, gx, gy),
                     border_margin(x, y), obstacle_margin(x, y, obstacles)])


def reference_reset(rows, n, rng, waves=1, spoil=None):
    """n draws of the reference's reset() (aqua.py:100-126) with one obstacle table, float64 [7][n]: the goal uniform on
    [0, 100]^2 and redrawn while it is on the border or an obstacle, then the boat redrawn while it is on the goal, the
    border or an obstacle, the heading U[-pi, pi], the wave U[-0.05 waves, 0.05 waves]^2.
    spoil (controls of the distribution test, each a plausible mistake): 'exclusion4' -- the boat keeps 4 units from the
    goal, not 5; 'drop_last_row' -- the table's last row is ignored; 'stale_goal' -- the boat is tested against the goal
    candidate before the final one (the final one where the first candidate was accepted)."""
    rows = _rows(rows)
    if spoil == "drop_last_row":
        assert rows.shape[0] >= 1
        rows = rows[:-1]
    total = 4.0 if spoil == "exclusion4" else 5.0

    def off_map(p):
        return (p[0] - 2.5 < 0) | (p[1] - 2.5 < 0) | (p[0] + 2.5 > 100) | (p[1] + 2.5 > 100)

    goal, before = np.empty((2, n)), np.empty((2, n))
    todo, first = np.arange(n), True
    while todo.size:
        c = rng.uniform(0.0, 100.0, (2, todo.size))
        rejected = off_map(c) | (obstacle_margin(c[0], c[1], rows) <= 0)
        goal[:, todo] = c
        if first:
            before[:, todo] = c
            first = False
        before[:, todo[rejected]] = c[:, rejected]
        todo = todo[rejected]
    against = before if spoil == "stale_goal" else goal
    boat = np.empty((3, n))
    todo = np.arange(n)
    while todo.size:
        c = np.stack([rng.uniform(0.0, 100.0, todo.size), rng.uniform(0.0, 100.0, todo.size),
                      rng.uniform(-np.pi, np.pi, todo.size)])
        rejected = (goal_margin(c[0], c[1], against[0, todo], against[1, todo], total) <= 0) | off_map(c) \
            | (obstacle_margin(c[0], c[1], rows) <= 0)
        boat[:, todo] = c
        todo = todo[rejected]
    wave = rng.uniform(-0.05 * waves, 0.05 * waves, (2, n))
    return np.concatenate([boat, goal, wave])


# ------------------------------------------------------------------------------------------------ Philox4x32-10, vectorised
def philox4x32_10(key, ctr):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays: key (k0, k1), ctr (c0, c1, c2, c3), each an integer or an array of
    32-bit values -> four uint64 arrays holding 32-bit words.  32 x 32 -> 64-bit products in uint64 arithmetic."""
    k0, k1 = (np.asarray(k, dtype=np.uint64) & _M32 for k in key)
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & _M32 for c in ctr])
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32
    return c0, c1, c2, c3


def draw(seed, env, tick, stream, attempt):
    """the four words of (world, tick, stream, attempt): the counter layout of aqua_draw, oracle/aqua_oracle.c"""
    env = np.asarray(env, dtype=np.uint64)
    seed, tick = int(seed) & (2 ** 64 - 1), int(tick) & (2 ** 64 - 1)
    c3 = ((tick >> 32) & 0xFFFF) | ((int(attempt) & 0xFF) << 16) | (int(stream) << 24)
    return philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (env & _M32, env >> np.uint64(32), tick & 0xFFFFFFFF, c3))


def u01(r):
    """24-bit uniform in [0, 1): exact in float32"""
    return (r >> np.uint64(8)).astype(_f32) * _f32(2.0 ** -24)


def upm1(r):
    """24-bit uniform in [-1, 1): exact in float32"""
    return ((r >> np.uint64(8)).astype(_f64) * 2.0 ** -23 - 1.0).astype(_f32)


# ------------------------------------------------------------------------------------------------ float32, one rounding per operation
def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: a * b + c rounded ONCE to float32.  The product of two float32 is exact in
    float64; the sum is rounded to float64 and then to float32, which differs from one rounding only where the float64
    sum lands exactly on the midpoint of two float32 values although the exact sum does not.  There the float64 sum is
    moved one step towards the exact one (its rounding error, exact by TwoSum) before the second rounding."""
    a, b, c = (np.asarray(v, dtype=_f32).astype(_f64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    s = np.atleast_1d(s).copy()
    err = np.broadcast_to(err, s.shape)
    tie = ((s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) & (err != 0)
    if tie.any():
        s[tie] = np.nextafter(s[tie], np.where(err[tie] > 0, np.inf, -np.inf))
    return s.astype(_f32)


def rows_f32(obstacles, other_radius=2.5):
    """float32 rows of the specification (oracle/aqua_oracle.c, obst_to_f32): centre, half extents (0 for a circle), the
    squared sum of the radii -> (cx, cy, hx, hy, r2, present), each [K] or [n][K]"""
    o = _rows(obstacles)
    kind, a, b = o[..., 2], o[..., 3], o[..., 4]
    circle = kind == 0
    rs = other_radius + np.where(circle, a, 0.0)
    return (o[..., 0].astype(_f32), o[..., 1].astype(_f32), np.where(circle, 0.0, a / 2).astype(_f32),
            np.where(circle, 0.0, b / 2).astype(_f32), (rs * rs).astype(_f32), kind >= 0)


def hit32(rows, sel, px, py):
    """the specification's hit test (hit_f32) of the float32 points (px, py) against the rows of the worlds `sel`"""
    cx, cy, hx, hy, r2, present = (r if r.ndim == 1 else r[sel] for r in rows)
    if cx.shape[-1] == 0:
        return np.zeros(px.shape, dtype=bool)
    ax, ay = np.abs(px[:, None] - cx), np.abs(py[:, None] - cy)
    dx, dy = np.maximum(ax - hx, _f32(0)), np.maximum(ay - hy, _f32(0))
    assert dx.dtype == _f32 and dy.dtype == _f32
    d2 = fma32(dx, dx, dy * dy).reshape(dx.shape)
    return np.any((d2 <= r2) & present, axis=1)


def placement_trace(seed, env_ids, tick, obstacles, waves=1, random_boat=True, random_goal=True):
    """The float32 reset specification (oracle/aqua_oracle.c, reset_world) for the worlds env_ids at `tick`, against one
    table [K][5] or one table per listed world [len(env_ids)][K][5] -> (state float32 [7][n], a_goal, a_boat): the
    attempt index the serial loops stop at, TRIES where all attempts were rejected (the fixed goal (25, 80) / boat
    (85, 45, 0) then stand), -1 where the flag is off."""
    env = np.asarray(env_ids, dtype=np.uint64)
    n = env.shape[0]
    rows = rows_f32(obstacles)
    a95, a25 = _f32(95.0), _f32(2.5)
    gx, gy = np.full(n, 25.0, dtype=_f32), np.full(n, 80.0, dtype=_f32)
    a_goal = np.full(n, -1, dtype=np.int64)
    if random_goal:
        a_goal[:] = TRIES
        todo = np.arange(n)
        for a in range(TRIES):
            if todo.size == 0:
                break
            r = draw(seed, env[todo], tick, STREAM_PLACE, a)
            cx, cy = fma32(a95, u01(r[0]), a25), fma32(a95, u01(r[1]), a25)
            ok = ~hit32(rows, todo, cx, cy)
            gx[todo[ok]], gy[todo[ok]], a_goal[todo[ok]] = cx[ok], cy[ok], a
            todo = todo[~ok]
    r = draw(seed, env, tick, STREAM_POSE, 0)
    pi_f, two_pi_f = _f32(3.14159274101257324), _f32(6.28318548202514648)
    w = _f32(0.05) * _f32(waves)
    heading = fma32(two_pi_f, u01(r[0]), -pi_f)
    wx, wy = w * upm1(r[1]), w * upm1(r[2])
    bx, by, bt = np.full(n, 85.0, dtype=_f32), np.full(n, 45.0, dtype=_f32), np.zeros(n, dtype=_f32)
    a_boat = np.full(n, -1, dtype=np.int64)
    if random_boat:
        a_boat[:] = TRIES
        todo = np.arange(n)
        for a in range(TRIES):
            if todo.size == 0:
                break
            r = draw(seed, env[todo], tick, STREAM_PLACE, a)
            cx, cy = fma32(a95, u01(r[2]), a25), fma32(a95, u01(r[3]), a25)
            ex, ey = gx[todo] - cx, gy[todo] - cy
            g2 = fma32(ex, ex, ey * ey)
            ok = ~(g2 <= _f32(25.0))
            ok[ok] = ~hit32(rows, todo[ok], cx[ok], cy[ok])
            bx[todo[ok]], by[todo[ok]], bt[todo[ok]], a_boat[todo[ok]] = cx[ok], cy[ok], heading[todo[ok]], a
            todo = todo[~ok]
    state = np.stack([bx, by, bt, gx, gy, wx.astype(_f32), wy.astype(_f32)])
    assert state.dtype == _f32
    return state, a_goal, a_boat


# ------------------------------------------------------------------------------------------------ which branch a world took
CLASSES = ("first_round", "boat_later_round", "goal_later_round", "boat_before_goal_round", "goal_exhausted",
           "boat_exhausted", "both_exhausted")
# with a flag off its index is -1: the loop of that flag is not run, and these are the classes left to reach
CLASSES_FIXED_GOAL = ("first_round", "boat_later_round", "boat_exhausted")
CLASSES_FIXED_BOAT = ("first_round", "goal_later_round", "goal_exhausted")


def branch_classes(a_goal, a_boat, group=G, tries=TRIES):
    """masks of the paths of reset_env_group, from the attempt indices of placement_trace; r(a) = a // group is the
    round an attempt belongs to.  goal_later_round is the serial boat scan; boat_before_goal_round the worlds whose
    accepted boat attempt lies in a round before the goal's (the candidates the device has to throw away)."""
    g, b = np.asarray(a_goal), np.asarray(a_boat)
    return collections.OrderedDict([
        ("first_round", (g < group) & (b < group)),
        ("boat_later_round", (g < group) & (b >= group) & (b < tries)),
        ("goal_later_round", (g >= group) & (g < tries) & (b < tries)),
        ("boat_before_goal_round", (g >= group) & (b // group < g // group)),
        ("goal_exhausted", (g == tries) & (b < tries)),
        ("boat_exhausted", (g < tries) & (b == tries)),
        ("both_exhausted", (g == tries) & (b == tries)),
    ])


def class_counts(a_goal, a_boat):
    return collections.OrderedDict((k, int(v.sum())) for k, v in branch_classes(a_goal, a_boat).items())


def classes_for(opts):
    if not opts["random_goal"]:
        return CLASSES_FIXED_GOAL
    if not opts["random_boat"]:
        return CLASSES_FIXED_BOAT
    return CLASSES


# ------------------------------------------------------------------------------------------------ crowded worlds
FREE_CLASSES = (0.0, 2.0, 4.75, 9.5, 28.5, 95.0)         # free = 95: no row present
FREE_SHARES = (0.04, 0.40, 0.20, 0.16, 0.10, 0.10)       # of the worlds outside the two blocked runs
BLOCKED_RUNS = ((256, 256), (1088, 64))                  # (first world, length): aligned to their length


def _strips(m, free):
    """m vertical strips side by side over x in [0, 95 - free] (free = 0: over the whole map, which blocks every
    candidate), 100 units high: a candidate's centre is free iff x > 95 - free + 2.5"""
    span = 100.0 if free == 0 else 95.0 - free
    w = span / m
    rows = np.zeros((m, 5))
    rows[:, 0] = w * (np.arange(m) + 0.5)
    rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = 50.0, 1.0, w, 100.0
    return rows


def crowded_rows(K, free):
    """one shared table of K rows, acceptance free / 95 (free = 0: the strips cover the map, a blocked world); the
    strips in a scrambled order"""
    rng = np.random.RandomState(7000 + 10 * K + int(free))
    return _strips(K, free)[rng.permutation(K)]


def present_rows(K):
    return K - K // 4 if K > 1 else 1


def crowded_tables(K, n, seed=0):
    """[n][K][5] per-world tables and the free band of each world.  A scrambled class per world (FREE_CLASSES by
    FREE_SHARES) and two runs of blocked worlds (BLOCKED_RUNS: a whole wavefront, a whole block).  present_rows(K) of the
    K rows are strips, in a place and an order of the world's own; the others are absent (kind -1) and hold a rectangle
    that would block the whole map if it were read."""
    rng = np.random.RandomState(9000 + 100 * K + seed)
    free = np.asarray(FREE_CLASSES)[rng.choice(len(FREE_CLASSES), size=n, p=FREE_SHARES)]
    for first, length in BLOCKED_RUNS:
        assert first % length == 0
        free[first:first + length] = 0.0
    m = present_rows(K)
    t = np.zeros((n, K, 5))
    t[:, :, 0:2], t[:, :, 2], t[:, :, 3:5] = 50.0, -1.0, 100.0
    place = np.argsort(rng.uniform(size=(n, K)), axis=1)[:, :m]          # the m rows of each world that are present
    for f in FREE_CLASSES[:-1]:
        w = np.flatnonzero(free == f)
        t[w[:, None], place[w]] = _strips(m, f)[None]
    return t, free


# ------------------------------------------------------------------------------------------------ the cells
Cell = collections.namedtuple("Cell", "fam option free")       # free: the shared table's band; None: per-world tables

SHARED_ENTRIES = ("step", "rollout", "fused", "graph", "graph_fused")
WORLD_ENTRIES = ("step", "rollout", "fused", "graph")
WORLD_K = (8, 9, 11, 17, 24, 33, 64)
RESTART_MODES = (C["AQUA_RESET_SAME_STEP"], C["AQUA_RESET_NEXT_STEP"])
EXTRA_OPTIONS = ("fixed_goal", "fixed_boat")                # for K = 8 shared and K = 11 per world
MIN_PER_CLASS = 30


def _cells():
    cells, i = [], 0
    small, loop = C["NS_TABLE_ROWS"], C["NS_TABLE_ROWS"] + 1

    def add(table, K, mode, entries, option, free):
        nonlocal i
        n, off = O.SIZES[i % 2], O.OFFSETS[i % 3]
        i += 1
        cells.append(Cell(O.Family(table, K, n, off, "u8", mode, tuple(entries), (option,), False), option, free))

    for K in (small, loop):
        for mode in RESTART_MODES:
            add("shared", K, mode, SHARED_ENTRIES, "default", 2.0)
            add("shared", K, mode, SHARED_ENTRIES, "default", 0.0)
            if K == small:
                for option in EXTRA_OPTIONS:
                    add("shared", K, mode, SHARED_ENTRIES, option, 2.0)
    for K in WORLD_K:
        for mode in RESTART_MODES:
            add("world", K, mode, WORLD_ENTRIES, "default", None)
            if K == 11:
                for option in EXTRA_OPTIONS:
                    add("world", K, mode, WORLD_ENTRIES, option, None)
    return cells


CELLS = _cells()


def cell_id(cell):
    return "%s-%s-%s" % (O.family_id(cell.fam), cell.option, "tables" if cell.free is None else "free%g" % cell.free)


def cell_obstacles(cell):
    fam = cell.fam
    if fam.table == "world":
        return crowded_tables(fam.K, fam.N, seed=fam.mode)[0]
    return crowded_rows(fam.K, cell.free)


def start_time(cell):
    """same-step: every world on its last step before the limit, so that all of them restart at tick 0 and whoever
    collides afterwards at ticks 1 and 2.  next-step: half of the worlds marked "finished at tick -1" (re-seeded at tick
    0, stepping from tick 1), the others on their last step (finished at tick 0, re-seeded at tick 1); with a fixed boat
    or goal all of them are marked, so that no world keeps a start state that happens to sit at the fixed values."""
    fam = cell.fam
    tt = np.full(fam.N, O.DEFAULT_LIMIT, dtype=np.int32)
    if fam.mode == C["AQUA_RESET_NEXT_STEP"]:
        marked = np.ones(fam.N, dtype=bool) if cell.option != "default" else np.arange(fam.N) % 2 == 0
        tt[marked] = -1 - ((0 - 1) & 1)
    return tt


def cell_inputs(oracle, cell):
    """-> (obstacles, start state float32 [7][n], start time, stored actions [T][n]) in the form _run_chain(inputs=)
    takes: the start state is the oracle's all-random reset in the cell's own crowded worlds"""
    fam = cell.fam
    obst = cell_obstacles(cell)
    st, tt = np.zeros((7, fam.N), dtype=_f32), np.zeros(fam.N, dtype=np.int32)
    reset = oracle.reset_tables if fam.table == "world" else oracle.reset
    reset(st, tt, obst, waves=1, random_boat=True, random_goal=True, seed=SEED, tick=O.RESET_TICK_BASE,
          env_offset=fam.env_offset)
    rng = np.random.RandomState(zlib.crc32(cell_id(cell).encode()))
    return obst, st, start_time(cell), _stored_actions("u8", fam.N, rng)


def trace_reseeded(cell, obst, reseeded, tick):
    """placement_trace of the worlds a tick re-seeds, under the cell's options -> (worlds, state, a_goal, a_boat)"""
    fam, opts = cell.fam, O.OPTIONS[cell.option]
    w = np.flatnonzero(reseeded)
    env = np.uint64(fam.env_offset) + w.astype(np.uint64)
    mine = obst[w] if fam.table == "world" else obst
    st, ag, ab = placement_trace(SEED, env, tick, mine, opts["waves"], opts["random_boat"], opts["random_goal"])
    return w, st, ag, ab


def oracle_cell(oracle, cell):
    """the cell's T ticks on the CPU alone (the oracle chain of _options.oracle_tick, free-running from the start state)
    -> per tick (worlds re-seeded, their traced a_goal, a_boat, live worlds stepped)"""
    fam, opts = cell.fam, O.OPTIONS[cell.option]
    obst, st, tt, acts = cell_inputs(oracle, cell)
    out = []
    for t in range(T):
        stepped = (tt >= 0) | (tt == -3 - ((t - 1) & 1)) if fam.mode == 2 else tt >= 0
        _, _, reseeded = O.oracle_tick(oracle, st, tt, np.ascontiguousarray(acts[t]), obst, fam.table == "world",
                                       fam.mode, t, fam.env_offset, opts)
        w, traced, ag, ab = trace_reseeded(cell, obst, reseeded, t)
        assert np.array_equal(traced.view(np.uint32), st[:, w].view(np.uint32)), "trace and oracle disagree"
        out.append((w, ag, ab, int(stepped.sum())))
    return out


def cell_class_counts(oracle, cell):
    """per-class counts of the worlds the cell re-seeds, over its ticks, and per tick"""
    ticks = oracle_cell(oracle, cell)
    per_tick = [class_counts(ag, ab) for _, ag, ab, _ in ticks]
    total = collections.OrderedDict((k, sum(c[k] for c in per_tick)) for k in CLASSES)
    return total, per_tick, [w.size for w, _, _, _ in ticks], [s for _, _, _, s in ticks]


def assert_cell_classes(cell, total, reseeded_per_tick):
    """what a cell must reach: every class of its option set, MIN_PER_CLASS worlds each with per-world tables (at least
    one with the shared table); in a blocked shared world every re-seeded world exhausts both loops"""
    what = cell_id(cell)
    n_reseeded = sum(reseeded_per_tick)
    assert n_reseeded >= 100, "%s: only %d worlds re-seeded" % (what, n_reseeded)
    if cell.free == 0.0:
        assert total["both_exhausted"] == n_reseeded, "%s: %s of %d" % (what, dict(total), n_reseeded)
        return
    least = MIN_PER_CLASS if cell.free is None else 1
    for k in classes_for(O.OPTIONS[cell.option]):
        assert total[k] >= least, "%s: class %s has %d worlds (%s)" % (what, k, total[k], dict(total))


def check_acceptance(state, obst, a_goal, a_boat, what):
    """the reference's acceptance on a placement: every margin of a loop that stopped at an accepted attempt is
    >= MARGIN_BAR, an exhausted loop left exactly its fixed values.  The exemptions come from the trace alone.  A flag
    that is off (-1) leaves the fixed values too.  -> the worst margin of the accepted goals and boats."""
    m = acceptance_margins(state, obst)
    goal_ok, boat_ok = (a_goal >= 0) & (a_goal < TRIES), (a_boat >= 0) & (a_boat < TRIES)
    worst = []
    for ok, idx, fixed, rows in ((goal_ok, GOAL_MARGINS, O.FIXED_GOAL, (3, 4)), (boat_ok, BOAT_MARGINS, O.FIXED_BOAT, (0, 1, 2))):
        got = m[list(idx)][:, ok]
        worst.append(float(got.min()) if got.size else float("inf"))
        bad = np.flatnonzero(ok)[np.any(got < MARGIN_BAR, axis=0)]
        assert bad.size == 0, "%s: %d accepted placements violate the reference's predicates (margins %s of world %d: %s)" % (
            what, bad.size, [MARGINS[i] for i in idx], bad[0], m[list(idx)][:, bad[0]])
        want = np.array(fixed, dtype=_f32)[:, None]
        at = np.all(np.asarray(state)[list(rows)] == want, axis=0)
        assert np.all(at[~ok]), "%s: %d worlds without an accepted attempt are not at the fixed rows %s" % (
            what, int((~at[~ok]).sum()), rows)
    return tuple(worst)
