"""CPU checks of the option cells (tests/_options.py) that tests/test_option_matrix.py runs on the GPU: the composition
oracle_tick() equals the oracle the rest of the suite trusts where both apply, the options mean on the oracle what
aqua.py:100-126 says, the families reach every kernel family of the built code object, and every cell exercises what it
is there for (restarts, live worlds, time-outs, all termination codes) -- computed from the oracle alone."""
import collections

import numpy as np
import pytest

from tests import _dispatch as D
from tests import _options as O
from tests._parity import _oracle_next_step_tables
from tests.test_dispatch_matrix import _shared_rows, _world_tables

N = 3011
DEFAULT = O.OPTIONS["default"]


def _start(oracle, obst, per_world, n=N, waves=1, env_offset=7):
    st, tt = np.zeros((7, n), dtype=np.float32), np.zeros(n, dtype=np.int32)
    (oracle.reset_tables if per_world else oracle.reset)(st, tt, obst, waves=waves, seed=O.SEED, tick=O.RESET_TICK_BASE,
                                                         env_offset=env_offset)
    tt[:] = O.time_row(np.random.RandomState(5), n, 1000)
    return st, tt


# ------------------------------------------------------------------------------------------------ the composition
@pytest.mark.parametrize("mode", D.MODES)
def test_oracle_tick_is_the_oracles_rollout_under_the_default_options(oracle, mode):
    from aquaticgymenv_amd import presets
    rows = np.asarray(presets.rows_from(presets.BENCH8), dtype=np.float64)
    st, tt = _start(oracle, rows, False)
    s2, t2 = st.copy(), tt.copy()
    rng = np.random.RandomState(11)
    finished = 0
    for tick in range(5):
        act = rng.randint(0, 3, N).astype(np.uint8)
        rew, term, reseeded = O.oracle_tick(oracle, st, tt, act, rows, False, mode, tick, 7, DEFAULT)
        _, r2, c2, _ = oracle.rollout_f32(s2, t2, 1, obstacles=rows, waves=1, actions=act, seed=O.SEED, tick0=tick,
                                          env_offset=7, auto_reset=mode)
        assert rew.dtype == np.float32 and np.array_equal(rew.view(np.uint32), r2.view(np.uint32))
        assert np.array_equal(term, c2) and np.array_equal(tt, t2)
        assert np.array_equal(st.view(np.uint32), s2.view(np.uint32))
        finished += int((term != 0).sum())
    assert finished >= 300


def test_oracle_tick_is_the_per_world_next_step_composition(oracle):
    tables = _world_tables(9, N)
    st, tt = _start(oracle, tables, True)
    s2, t2 = st.copy(), tt.copy()
    rng = np.random.RandomState(12)
    for tick in range(5):
        act = rng.randint(0, 3, N).astype(np.uint8)
        rew, term, _ = O.oracle_tick(oracle, st, tt, act, tables, True, 2, tick, 7, DEFAULT)
        r2, c2 = _oracle_next_step_tables(oracle, s2, t2, act, tables, O.SEED, tick, 7)
        assert np.array_equal(rew.view(np.uint32), r2.view(np.uint32)) and np.array_equal(term, c2)
        assert np.array_equal(tt, t2) and np.array_equal(st.view(np.uint32), s2.view(np.uint32))


@pytest.mark.parametrize("mode", D.MODES)
def test_a_shifted_time_row_is_a_shorter_limit(oracle, mode):
    """limit L on times t == limit 1000 on times t + (1000 - L): the same codes, rewards and states, the times L apart
    for the worlds that were not re-seeded"""
    rows = _shared_rows(8)
    st, _ = _start(oracle, rows, False)
    tt = O.time_row(np.random.RandomState(6), N, 5)
    s2, t2 = st.copy(), (tt + 995).astype(np.int32)
    short = dict(DEFAULT, time_limit=5)
    timed_out = 0
    for tick in range(3):
        act = np.random.RandomState(tick).randint(0, 3, N).astype(np.uint8)
        rew, term, re1 = O.oracle_tick(oracle, st, tt, act, rows, False, mode, tick, 0, short)
        r2, c2, re2 = O.oracle_tick(oracle, s2, t2, act, rows, False, mode, tick, 0, DEFAULT)
        assert np.array_equal(term, c2) and np.array_equal(rew, r2) and np.array_equal(st, s2)
        counted = (tt >= 0) & (t2 >= 995)
        assert np.array_equal(tt[counted] + 995, t2[counted]) and np.array_equal(tt < 0, t2 < 0)
        timed_out += int((term == 2).sum())
    assert timed_out >= 300


# ------------------------------------------------------------------------------------------------ what the options mean
def _reset(oracle, n=N, **kw):
    st, tt = np.zeros((7, n), dtype=np.float32), np.full(n, 9, dtype=np.int32)
    oracle.reset(st, tt, _shared_rows(8), seed=O.SEED, tick=3, env_offset=7, **kw)
    return st


def test_fixed_poses_on_the_oracle(oracle):
    both = _reset(oracle)
    boat = _reset(oracle, random_boat=False)
    goal = _reset(oracle, random_goal=False)
    assert np.all(boat[0:3] == np.array(O.FIXED_BOAT, dtype=np.float32)[:, None])
    assert np.all(goal[3:5] == np.array(O.FIXED_GOAL, dtype=np.float32)[:, None])
    assert not np.any(np.all(both[0:3] == np.array(O.FIXED_BOAT, dtype=np.float32)[:, None], axis=0))
    # the goal loop does not look at the boat: the same goal draws with the boat fixed; the wave draws are the world's own
    assert np.array_equal(boat[3:5], both[3:5])
    assert np.array_equal(boat[5:7], both[5:7])


def test_wave_bounds_on_the_oracle(oracle):
    w0, w1, w2 = (_reset(oracle, waves=w)[5:7] for w in (0, 1, 2))
    assert np.all(w0 == 0)
    assert np.abs(w1).max() <= 0.05 and np.abs(w2).max() <= 0.1 and (np.abs(w2) > 0.05).any()
    # waves = 0: a step leaves the wave at exactly 0 whatever the injected noise
    st = np.ascontiguousarray(_reset(oracle, waves=0).astype(np.float64))
    tt = np.zeros(N, dtype=np.int32)
    oracle.step(st, tt, np.zeros(N, dtype=np.uint8), obstacles=_shared_rows(8), waves=0, noise_u=O.noise_at(N, 1))
    assert np.all(st[5:7] == 0)


def test_injected_noise_values_are_exact_and_distinct():
    u = O.noise_at(4099, 2)
    assert u.dtype == np.float32 and len(np.unique(u[0])) == 4099 and len(np.unique(u[1])) == 4099
    assert not np.any(u[0] == u[1]) and not np.array_equal(u, O.noise_at(4099, 1))


# ------------------------------------------------------------------------------------------------ coverage
def _shipped_families(tmp_path_factory):
    from tests import test_kernel_coverage as K
    missing = [t for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf") if K._tool(t) is None]
    if missing:
        pytest.skip("the ROCm LLVM tools %s are not installed: the code object's kernels cannot be listed" % missing)
    from aquaticgymenv_amd import build
    names = K.code_object_kernels(build.build_hip(), str(tmp_path_factory.mktemp("co_options")))
    skip = {O.strip_template(n) for n in list(K.UNREACHABLE) + list(K.UTILITY)}
    return {O.strip_template(n) for n in names} - skip


def reached_families(families=None, reset_cells=None):
    out = set()
    for f in (O.FAMILIES if families is None else families):
        out |= {O.strip_template(k) for k in O.family_kernels(f)}
    for table, K, name in (O.RESET_CELLS if reset_cells is None else reset_cells):
        out.add("reset_tables_kernel" if table == "world" else "reset_kernel")
    return out


def test_the_families_reach_every_kernel_family(tmp_path_factory):
    shipped = _shipped_families(tmp_path_factory)
    missing = sorted(shipped - reached_families())
    assert not missing, "kernel families without option cells (add a Family to tests/_options.py): %s" % missing
    # the gate bites: without its only families a kernel family is reported by name
    fewer = [f for f in O.FAMILIES if not (f.table == "world" and f.K == 33)]
    assert "rollout_tables64_kernel" in shipped - reached_families(fewer)
    assert "reset_tables_kernel" in shipped - reached_families(reset_cells=[c for c in O.RESET_CELLS if c[0] != "world"])


def test_the_families_reach_every_plumbing_site():
    """the instantiations named in the issue's list, predicted by the dispatch model"""
    got = set()
    for f in O.FAMILIES:
        got |= O.family_kernels(f)
    c = D.C
    want = ["step_kernel<0, %s, %s, %s>" % (s, r, w) for s in ("true", "false")
            for r, w in (("false", "false"), ("true", "false"), ("true", "true"))]
    want += ["step_ns_kernel<0, %s, %s, %s>" % (s, i, w) for s in ("true", "false")
             for i, w in (("false", "false"), ("true", "false"), ("true", "true"))]
    want += ["rollout_kernel<0, %s, %d>" % (s, m) for s in ("true", "false") for m in (1, 2)]
    for K in O.WORLD_K:
        for mode in D.MODES:
            want += sorted(D.step_tables_kernels("u8", mode, K, 4099))
    want += ["%s<0, %d>" % (fam, m) for fam in ("rollout_tables_kernel", "rollout_tables16_kernel", "rollout_tables32_kernel",
                                                "rollout_tables64_kernel") for m in D.MODES]
    missing = sorted(set(want) - got)
    assert not missing, missing
    # every (MODE, KREG, SINK_SPLIT) band the per-world launcher can choose, over every K it accepts
    bands = {D.step_tables_kernels("u8", m, K, 4099).pop() for m in D.MODES for K in range(1, c["FUSED_TABLE_ROWS_MAX"] + 1)}
    assert bands <= got, sorted(bands - got)
    assert any(f.N > c["DONE_WORD_WRITE_THROUGH_MAX_WORLDS"] for f in O.FAMILIES)
    # f32x2 and a sampled kind beside u8 in every stepping kernel family
    kinds = collections.defaultdict(set)
    for f in O.FAMILIES:
        for k in O.family_kernels(f):
            kinds[O.strip_template(k)].add(f.kind)
    for fam, ks in kinds.items():
        if fam != "tick_kernel":
            assert {"u8", "f32x2"} <= ks and ks & {"sample_d", "sample_c"}, (fam, ks)


def test_every_family_is_paired_with_every_option_set_it_can_take():
    # everything changed at once (the goal stays random: with the boat fixed it tells a swap of the two flags)
    assert {k for k, v in O.OPTIONS["all"].items() if v == DEFAULT[k]} == {"random_goal"}
    for name in O.OPTIONS:                                                     # each option set is run somewhere
        assert any(o == name for _, o in O.CELLS), name
    pairs = {(O.family_id(f), o) for f, o in O.CELLS}
    per_site = collections.defaultdict(set)            # kernel instantiation (u8) -> option sets it is run with
    for f in O.FAMILIES:
        if f.kind == "u8":
            for k in O.family_kernels(f):
                per_site[k] |= set(f.options)
    for f in O.FAMILIES:
        want = O.LARGE_OPTIONS if f.large else (O.options_for(f.mode) if f.kind == "u8" else O.EXTRA_KIND_OPTIONS)
        for o in O.options_for(f.mode, want):
            assert (O.family_id(f), o) in pairs, (O.family_id(f), o)
        if opts_noise := [o for o in f.options if O.OPTIONS[o]["noise"]]:
            assert all(O.entries_for(f, O.OPTIONS[o], True) for o in opts_noise)       # noise cells have an entry that takes it
    for k, opts in per_site.items():
        if O.strip_template(k) != "tick_kernel":
            assert {"default", "all"} <= opts, (k, opts)
    for f, o in O.CELLS:                                # injected noise only where the entry point accepts it
        assert set(O.entries_for(f, O.OPTIONS[o], True)) <= set(O.NOISE_ENTRIES)
        assert "step" in f.entries


# ------------------------------------------------------------------------------------------------ every cell exercises something
SMALL = [c for c in O.CELLS if not c[0].large]


@pytest.mark.parametrize("cell", SMALL, ids=[O.cell_id(c) for c in SMALL])
def test_small_cell_meets_its_conditions_on_the_oracle(oracle, cell):
    fam, name = cell
    opts = O.OPTIONS[name]
    for noise in O.chains(fam, opts):
        ticks = O.oracle_cell(oracle, fam, opts, noise)
        never = np.ones(fam.N, dtype=bool)
        for t, (term, reseeded, stepped, state) in enumerate(ticks):
            O.tick_conditions(fam, opts, t, term, reseeded, stepped)
            never &= ~reseeded
            O.fixed_pose_conditions(opts, state, reseeded, never, "%s tick %d" % (O.cell_id(cell), t))
            if opts["waves"] == 0:
                assert np.all(state[5:7] == 0)
            if opts["waves"] == 2 and reseeded.any():
                assert np.abs(state[5:7, reseeded]).max() <= 0.1 and (np.abs(state[5:7, reseeded]) > 0.05).any()
        O.cell_conditions(fam, opts, [x[0] for x in ticks])


def test_every_family_sees_all_three_termination_codes(oracle):
    """over the ticks of a kernel family's cells taken together (computed here, whatever else of this file ran)"""
    counts = collections.defaultdict(lambda: np.zeros(4, dtype=np.int64))
    for fam, name in SMALL:
        opts = O.OPTIONS[name]
        for noise in O.chains(fam, opts):
            for term, _, _, _ in O.oracle_cell(oracle, fam, opts, noise):
                for k in O.family_kernels(fam):
                    counts[O.strip_template(k)] += np.bincount(term, minlength=4)[:4]
    assert len(counts) >= 9
    for fam, c in counts.items():
        assert np.all(c[1:4] >= 10), "%s: termination codes 1/2/3 occur %s times over its cells" % (fam, c[1:4])

@pytest.mark.parametrize("fam", O.KNIFE_FAMILIES, ids=[O.family_id(f) for f in O.KNIFE_FAMILIES])
def test_knife_cells_put_the_time_limit_on_the_float64_path(oracle, fam):
    """worlds within BAND_TIGHT of a threshold that end on the limit of 5 and would not on 1000, and worlds that go on"""
    (obst, st, tt, acts), timed_out, goes_on = O.knife_inputs(oracle, fam)
    assert int(timed_out.sum()) >= O.KNIFE_MIN and int(goes_on.sum()) >= O.KNIFE_MIN, (timed_out.sum(), goes_on.sum())
    assert np.all(tt[timed_out] == 5) and np.all(tt[goes_on] < 5)


def test_knife_cells_reach_every_stepping_kernel_family():
    got = set()
    for f in O.KNIFE_FAMILIES:
        got |= {O.strip_template(k) for k in O.family_kernels(f)}
    want = {O.strip_template(k) for f in O.FAMILIES for k in O.family_kernels(f)} - {"tick_kernel"}
    assert want <= got, sorted(want - got)
