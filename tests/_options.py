"""The runtime options of the kernels -- waves (0, 1, 2), random_boat, random_goal, time_limit, injected noise and the
normalised-observation epilogue -- as test cells, and the oracle side of those cells.  Imports without a GPU.

None of these options is a template argument, so tests/test_kernel_coverage.py cannot see them; each kernel family has
its own copy of the plumbing for them (the flag word of NsArgs, the arguments of every in-launch restart, time_limit in
StepConst, ten call sites of write_norm / ns_write_norm).  FAMILIES holds one representative per plumbing site, chosen
through the dispatch model (tests/_dispatch.py: thresholds read from the sources); OPTIONS the named option sets;
CELLS their product where the family can take the option.  tests/test_option_construct.py checks the construction on
the CPU, tests/test_option_matrix.py runs the cells on the GPU.

The oracle's rollout (oracle.rollout_f32) hard-codes random_boat = random_goal = 1, Philox noise and the 1000-step
limit, so oracle_tick() composes one tick of each restart convention from the oracle's primitives, which take the
options: step / step_tables (waves, noise_u) and the masked reset / reset_tables (random_boat, random_goal, waves).
A time limit L != 1000 needs no change to the oracle: the limit is read once, `time > limit` after the increment, so
the oracle is handed time + (1000 - L) for the worlds that step and the shift is taken off again before any restart.
"""
import collections
import zlib

import numpy as np

from tests import _dispatch as D
from tests.test_dispatch_matrix import T, SEED, _shared_rows, _world_tables, _stored_actions

C = D.C
RESET_TICK_BASE = 1 << 40          # BatchedAqua.RESET_TICK_BASE: where reset() draws (the start states use it too)
NOISE_PAD = 37                     # injected noise: noise_ld = ld + NOISE_PAD
NOISE_GUARD = 0.640625             # what the padding of the noise buffer holds (a valid uniform, exact in float32)
NORM_GUARD = -77.25                # what columns n .. ld of obs_norm_buf hold before a run
FIXED_BOAT = (85.0, 45.0, 0.0)     # aqua.py:107
FIXED_GOAL = (25.0, 80.0)          # aqua.py:117
DEFAULT_LIMIT = 1000               # aqua.py:91

# ------------------------------------------------------------------------------------------------ option sets
_DEFAULT = dict(waves=1, random_boat=True, random_goal=True, time_limit=DEFAULT_LIMIT, noise=None, norm=False)


def _opt(**kw):
    o = dict(_DEFAULT)
    o.update(kw)
    return o


OPTIONS = collections.OrderedDict([
    ("default", _opt()),                                           # random boat, random goal
    ("waves0", _opt(waves=0)),
    ("waves2", _opt(waves=2)),
    ("fixed_boat", _opt(random_boat=False)),
    ("fixed_goal", _opt(random_goal=False)),
    ("fixed_both", _opt(random_boat=False, random_goal=False)),
    ("limit5", _opt(time_limit=5)),
    ("noise", _opt(noise="injected")),
    ("norm", _opt(norm=True)),
    ("all", _opt(waves=2, random_boat=False, random_goal=True, time_limit=5, noise="injected", norm=True)),
])
RESTART_ONLY = ("fixed_boat", "fixed_goal", "fixed_both")      # options only a restart reads: not paired with mode 0
NOISE_ENTRIES = ("step", "graph_step")                         # the entry points that accept injected noise
LARGE_OPTIONS = ("default", "all")
# The families that exist for their action kind (f32x2, sampled) run three option sets, not ten: the kinds differ from
# u8 in where the option fields sit beside the action fields of the kernarg block, not in what the options do.  "all"
# moves every field at once (waves 2, fixed boat, limit 5, noise and norm pointers); "fixed_goal" is the one flag "all"
# leaves at its default; "waves0" is the other end of the waves field, where a wrong read shows as a wave that is not 0.
EXTRA_KIND_OPTIONS = ("all", "fixed_goal", "waves0")

Family = collections.namedtuple("Family", "table K N env_offset kind mode entries options large")

SIZES = (3011, 4099)
OFFSETS = (0, 7, 2 ** 32 - 3)
WORLD_K = (8, 9, 11, 17, 24, 33)       # one K per (KREG, SINK_SPLIT) band of step_tables_kernel and per fused tile


def options_for(mode, names=None):
    names = tuple(OPTIONS) if names is None else names
    return tuple(o for o in names if mode != C["AQUA_RESET_NONE"] or o not in RESTART_ONLY)


def _families():
    fams, i = [], 0
    small, loop = C["NS_TABLE_ROWS"], C["NS_TABLE_ROWS"] + 1           # both sides of NS_TABLE_ROWS / QUICK_MAX

    def add(table, K, kind, mode, entries, names=None):
        nonlocal i
        n, off = SIZES[i % 2], OFFSETS[i % 3]
        i += 1
        fams.append(Family(table, K, n, off, kind, mode, tuple(entries), options_for(mode, names), False))

    # one table: step_kernel (modes 0, 1), step_ns_kernel (mode 2), rollout_kernel (quick table / row loop)
    for K in (small, loop):
        for mode in D.MODES:
            add("shared", K, "u8", mode, D.SHARED_ENTRIES)
    for K, mode, kind in ((small, 1, "f32x2"), (loop, 1, "sample_d"), (small, 2, "sample_c"), (loop, 2, "f32x2")):
        add("shared", K, kind, mode, D.SHARED_ENTRIES, EXTRA_KIND_OPTIONS)
    # per-world tables: every (MODE, KREG, SINK_SPLIT) band of step_tables_kernel, the four fused kernels
    for K in WORLD_K:
        for mode in D.MODES:
            add("world", K, "u8", mode, D.TABLE_ENTRIES)
    for K, mode, kind in ((8, 1, "f32x2"), (8, 2, "sample_d"), (11, 2, "f32x2"), (11, 1, "sample_c"),
                          (17, 1, "f32x2"), (17, 2, "sample_d"), (33, 2, "f32x2"), (33, 1, "sample_c")):
        add("world", K, kind, mode, D.TABLE_ENTRIES, EXTRA_KIND_OPTIONS)
    # the batch-size bands of the one-table step kernels: write-back stores, interleaved tiles, done words written
    # through (N > DONE_WORD_WRITE_THROUGH_MAX_WORLDS)
    big = max(C["STORE_WB_SAME_STEP_MIN"], C["DONE_WORD_WRITE_THROUGH_MAX_WORLDS"] + 1)
    for K in (small, loop):
        for n, mode in ((big, 1), (C["NS_INTERLEAVE_MIN"], 2), (C["STORE_WB_NEXT_STEP_MIN"], 2)):
            fams.append(Family("shared", K, n, 0, "u8", mode, ("step", "rollout"), LARGE_OPTIONS, True))
    return fams


FAMILIES = _families()

# reset() and reset(mask): option set -> (waves, random_boat, random_goal), each for one table and per-world tables
RESET_N = 50000
RESET_OPTIONS = collections.OrderedDict([
    ("random_both", (1, True, True)), ("fixed_boat", (1, False, True)), ("fixed_goal", (1, True, False)),
    ("fixed_both", (1, False, False)), ("waves0", (0, True, True)), ("waves2_fixed_boat", (2, False, True)),
    ("waves2", (2, True, True)),
])
RESET_CELLS = [(table, K, name) for table, K in (("shared", 8), ("world", 9)) for name in RESET_OPTIONS]


def family_id(f):
    return "%s-K%d-N%d-off%d-%s-mode%d" % (f.table, f.K, f.N, f.env_offset, f.kind, f.mode)


CELLS = [(f, o) for f in FAMILIES for o in f.options]


def cell_id(cell):
    return "%s-%s" % (family_id(cell[0]), cell[1])


def entries_for(fam, opts, noise):
    """the family's entry points a chain with (noise=True) / without injected noise is compared with; a device policy
    is captured with capture_rollout(1), which takes no noise buffer"""
    takes = NOISE_ENTRIES if fam.kind in D.STORED else ("step",)
    if noise:
        return tuple(e for e in fam.entries if e in takes)
    if opts["noise"]:
        return tuple(e for e in fam.entries if e not in takes or e == "step")
    return fam.entries


def chains(fam, opts):
    """the step() chains a cell runs: with injected noise where the option set has it, and -- when the set changes
    something else as well -- a chain on Philox noise for the entry points that take no noise buffer"""
    if not opts["noise"]:
        return (False,)
    changes_more = dict(opts, noise=None) != _DEFAULT
    has_other_entries = len(entries_for(fam, opts, False)) > 0
    if changes_more and has_other_entries:
        return (True, False)
    return (True,)


def family_kernels(fam):
    """the dispatch model's prediction for the family's entry points (graphs: one step() ahead of two replays of a
    one-step graph), without the reset: the start state is written with set_state()"""
    per_world = fam.table == "world"
    out = set()
    for e in fam.entries:
        steps = 1 if e in ("graph", "graph_fused", "graph_step") else T
        out |= D.launched(e, fam.kind, fam.mode, fam.K, fam.N, per_world=per_world, T=steps, with_reset=False)
        if steps == 1:
            out |= D.launched("step", fam.kind, fam.mode, fam.K, fam.N, per_world=per_world, with_reset=False)
    return out


def strip_template(name):
    return name.split("<")[0]


# ------------------------------------------------------------------------------------------------ inputs of a cell
def time_row(rng, n, limit):
    """a quarter of the worlds within T steps of the limit (they finish on time at ticks 0 .. T-1, one third each); the
    others far enough below it not to"""
    far = limit - T - 7 if limit >= 20 else limit - T + 1
    return np.where(rng.randint(0, 4, n) == 0, rng.randint(limit - T + 1, limit + 1, n),
                    rng.randint(0, max(far, 1), n)).astype(np.int32)


def cell_inputs(oracle, fam, opts):
    """-> (obstacles, start state float32 [7][n], start time int32 [n], stored actions or None).  The start state is the
    oracle's reset with BOTH random flags on and the cell's waves, whatever the cell's other options: the live worlds
    are spread over the map and the options govern only the restarts inside the launches."""
    per_world = fam.table == "world"
    n = fam.N
    obst = _world_tables(fam.K, n) if per_world else _shared_rows(fam.K)
    rng = np.random.RandomState(zlib.crc32(family_id(fam).encode()))
    st = np.zeros((7, n), dtype=np.float32)
    tt = np.zeros(n, dtype=np.int32)
    reset = oracle.reset_tables if per_world else oracle.reset
    reset(st, tt, obst, waves=opts["waves"], random_boat=True, random_goal=True, seed=SEED, tick=RESET_TICK_BASE,
          env_offset=fam.env_offset)
    tt[:] = time_row(rng, n, opts["time_limit"])
    acts = _stored_actions(fam.kind, n, rng) if fam.kind in D.STORED else None
    return obst, st, tt, acts


def actions_at(oracle, fam, host_acts, t, tick):
    """the step's actions as the oracle takes them: the stored ones, or the device's Philox draws for this tick"""
    if host_acts is not None:
        return np.ascontiguousarray(host_acts[t])
    return oracle.sample_actions(fam.N, fam.kind in D.CONTINUOUS, seed=SEED, tick=tick, env_offset=fam.env_offset)


def noise_at(n, t):
    """float32 [2][n] uniforms k * 2^-23 in [-1, 1), exact in float32, distinct from world to world and between the two
    rows (a kernel that swaps the rows, reads row 1 at the wrong stride or another world's value is off by >= 2^-23)"""
    i = np.arange(n, dtype=np.int64)
    k0 = (i * 40503 + 7919 * t + 12345) % (1 << 24) - (1 << 23)
    k1 = (i * 69069 + 104729 * t + 8000001) % (1 << 24) - (1 << 23)
    u = (np.stack([k0, k1]).astype(np.float64) * 2.0 ** -23).astype(np.float32)
    assert np.array_equal(u.astype(np.float64) * 2.0 ** 23, np.stack([k0, k1])) and u.min() >= -1 and u.max() < 1
    return u


# ------------------------------------------------------------------------------------------------ the oracle side
def oracle_tick(oracle, st, tt, act, obst, per_world, mode, tick, env_offset, opts, noise_u=None):
    """one tick of the restart convention `mode` under the option set `opts`, from the oracle's primitives, on the
    float32 state st [7][n] / time markers tt [n] (both in place) -> (reward float32, term uint8, re-seeded worlds)"""
    waves, rb, rg = opts["waves"], opts["random_boat"], opts["random_goal"]
    shift = DEFAULT_LIMIT - opts["time_limit"]
    kw = dict(waves=waves, seed=SEED, tick=tick, env_offset=env_offset)
    if mode == 2:        # markers carry the parity of the tick that wrote them (oracle/aqua_oracle.c, rollout_f32)
        tt[tt == -3 - ((tick - 1) & 1)] = 0
        restart = tt == -1 - ((tick - 1) & 1)
    else:
        restart = np.zeros(tt.shape[0], dtype=bool)
    pending = tt < 0
    live = ~pending
    s64 = np.ascontiguousarray(st.astype(np.float64))
    t = np.ascontiguousarray(np.where(pending, 0, tt + shift).astype(np.int32))
    if noise_u is not None:
        noise_u = np.ascontiguousarray(noise_u, dtype=np.float64)
    if per_world:
        rew, term, _ = oracle.step_tables(s64, t, act, obst, noise_u=noise_u, **kw)
    else:
        rew, term, _ = oracle.step(s64, t, act, obstacles=obst, noise_u=noise_u, want_margins=False, **kw)
    st[:, live] = s64[:, live].astype(np.float32)
    tt[live] = t[live] - shift
    rew = np.where(live, rew, 0.0).astype(np.float32)
    term = np.where(live, term, 0).astype(np.uint8)
    reset = oracle.reset_tables if per_world else oracle.reset
    if mode == 2:
        tt[live & (term != 0)] = -1 - (tick & 1)
        reset(st, tt, obst, random_boat=rb, random_goal=rg, mask=restart, **kw)
        tt[restart] = -3 - (tick & 1)
        reseeded = restart
    elif mode == 1:
        reseeded = term != 0
        reset(st, tt, obst, random_boat=rb, random_goal=rg, mask=reseeded, **kw)
    else:
        reseeded = restart
    return rew, term, reseeded


def norm_expected(state):
    """float64 obs / (100, 100, 2 pi, 100, 100) + (0, 0, .5, 0, 0) of a float32 state [>=5][n]"""
    scale = np.array([100.0, 100.0, 2 * np.pi, 100.0, 100.0])[:, None]
    shift = np.array([0.0, 0.0, 0.5, 0.0, 0.0])[:, None]
    return state[:5].astype(np.float64) / scale + shift


# ------------------------------------------------------------------------------------------------ conditions
def tick_conditions(fam, opts, t, term, reseeded, stepped):
    """what a tick must exercise, from the oracle's outputs: worlds re-seeded and live worlds stepped"""
    least = 1000 if fam.large else 100
    what = "%s tick %d" % (family_id(fam), t)
    assert int(stepped.sum()) >= least, "%s: only %d live worlds stepped" % (what, stepped.sum())
    if fam.mode == 1 or (fam.mode == 2 and t >= 1):
        assert int(reseeded.sum()) >= least, "%s: only %d worlds re-seeded" % (what, reseeded.sum())


def cell_conditions(fam, opts, terms):
    """over the cell's ticks: with a time limit other than 1000, worlds that run out of time and worlds that do not"""
    if opts["time_limit"] != DEFAULT_LIMIT:
        timed_out = np.zeros(fam.N, dtype=bool)
        for term in terms:
            timed_out |= term == 2
        assert int(timed_out.sum()) >= 100 and int((~timed_out).sum()) >= 100, \
            "%s: %d worlds timed out, %d did not" % (family_id(fam), timed_out.sum(), (~timed_out).sum())


def fixed_pose_conditions(opts, state, reseeded, never, what):
    """from a state alone: with a fixed boat / goal the worlds re-seeded at this tick sit exactly there, and fewer than
    1 % of the others do (boat: the worlds not re-seeded at this tick; goal, which a step does not move: the worlds
    never re-seeded in this cell)"""
    for on, rows, want, others in ((not opts["random_boat"], (0, 1, 2), FIXED_BOAT, ~reseeded),
                                   (not opts["random_goal"], (3, 4), FIXED_GOAL, never)):
        if not on:
            continue
        want = np.array(want, dtype=np.float32)[:, None]
        at = np.all(state[list(rows)] == want, axis=0)
        assert np.all(at[reseeded]), "%s: %d re-seeded worlds are not at the fixed rows %s" % (
            what, (~at[reseeded]).sum(), rows)
        assert at[others].sum() < 0.01 * max(int(others.sum()), 1), "%s: %d other worlds sit at the fixed rows %s" % (
            what, at[others].sum(), rows)


def oracle_cell(oracle, fam, opts, noise=False):
    """the cell's T ticks on the CPU alone, free-running from the cell's start state -> per tick (term, reseeded,
    stepped, state after)"""
    obst, st, tt, acts = cell_inputs(oracle, fam, opts)
    out = []
    for t in range(T):
        stepped = tt >= 0 if fam.mode != 2 else (tt >= 0) | (tt == -3 - ((t - 1) & 1))
        act = actions_at(oracle, fam, acts, t, t)
        u = noise_at(fam.N, t) if noise else None
        rew, term, reseeded = oracle_tick(oracle, st, tt, act, obst, fam.table == "world", fam.mode, t, fam.env_offset,
                                          opts, u)
        out.append((term, reseeded.copy(), stepped, st.copy()))
    return out


# ------------------------------------------------------------------------------------------------ the limit at the knife edge
# The time limit reaches a kernel twice: the fast path reads it from StepConst, and the float64 path (exact_step /
# exact_step_world), which decides the worlds within BAND_TIGHT of a threshold, takes it as an argument of its own --
# one call site per kernel family.  A batch spread over the map puts next to no world there, so these cells start from a
# knife-edge batch (tests/_knife.py) with half of the worlds on their last step before a limit of 5.
KNIFE_N = 65536
KNIFE_MIN = 500                    # as MIN_TIGHT of tests/test_knife_edges.py
KNIFE_FAMILIES = [Family(table, K, KNIFE_N, 0, "u8", mode, ("step", "fused"), ("limit5",), False)
                  for table, K, mode in (("shared", 8, 0), ("shared", 20, 1), ("shared", 8, 2), ("shared", 20, 2),
                                         ("world", 8, 1), ("world", 9, 2), ("world", 11, 0), ("world", 17, 2),
                                         ("world", 33, 1))]


def knife_inputs(oracle, fam):
    """-> (obstacles, state, time, actions [T][n]) of a knife-edge batch under the limit of OPTIONS['limit5'], and the
    worlds the float64 path must decide that run out of time / go on, by the oracle's margins and codes"""
    from tests import _knife as KN
    opts = OPTIONS["limit5"]
    limit, n, per_world = opts["time_limit"], fam.N, fam.table == "world"
    rng = np.random.RandomState(zlib.crc32(("knife" + family_id(fam)).encode()))
    b = KN.build(oracle, fam.kind, n, rng, K=fam.K, per_world=per_world, seed=SEED, tick=0, env_offset=fam.env_offset)
    time0 = np.where(rng.randint(0, 2, n) == 0, limit, rng.randint(0, limit - T + 1, n)).astype(np.int32)
    acts = _stored_actions(fam.kind, n, rng)
    acts[0] = b.action
    st, tt = b.state.copy(), time0.copy()
    _, term, _ = oracle_tick(oracle, st, tt, np.ascontiguousarray(acts[0]), b.obst, per_world, fam.mode, 0, fam.env_offset, opts)
    tight, _ = KN.tiers(KN.nearest(b))
    return (b.obst, b.state, time0, acts), tight & (term == 2), tight & (term == 0)
