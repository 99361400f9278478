"""GPU parity tests: the HIP path (through the C ABI, libaqua_hip.so) against
 (1) the golden vectors produced from the reference itself (tests/golden/step_golden.npz),
 (2) the float64 CPU oracle (oracle/) on seeded inputs up to the benchmark size,
 (3) size-independent properties at full size.

Bars (BASELINE.json north_star): termination codes / done flags bit-exact; float32 pose and reward
within 1e-5 of the float64 reference (theta compared modulo 2 pi); the float32 reset
specification bit-exact against the oracle's independent restatement.
"""
import numpy as np
import pytest

from tests._golden import StepGolden, load_reset, angle_diff
from tests._parity import (TOL, _make, _host_state, _rollout_against_oracle, _buffered_rollout_against_oracle,
                           _oracle_next_step_tables, _bearing_np)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


@pytest.fixture(scope="module")
def capi():
    from aquaticgymenv_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def golden():
    return StepGolden()


# ------------------------------------------------------------------------------------------------
# (1) golden vectors from the reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(8))
def test_golden_rows(torch, golden, ci):
    cfg = golden.cfg(ci)
    rows = golden.rows(ci)
    n = rows["term"].shape[0]
    env = _make(torch, n, cfg["obstacles"], continuous=cfg["continuous"], waves=cfg["waves"])
    env.set_state(rows["state_in"].astype(np.float32), rows["time_in"])
    noise = torch.zeros((2, env.ld), dtype=torch.float32, device="cuda:0")
    noise[:, :n] = torch.as_tensor(rows["noise_u"].T.astype(np.float32))
    assert np.array_equal(rows["noise_u"].astype(np.float32).astype(np.float64), rows["noise_u"]) or cfg["waves"]
    if cfg["continuous"]:
        action = torch.as_tensor(rows["action_c"].astype(np.float32)).cuda()
    else:
        action = torch.as_tensor(rows["action_i"].astype(np.int64)).cuda()
    obs, reward, term = env.step(action, noise=noise)
    torch.cuda.synchronize()
    obs, reward, term = obs.cpu().numpy(), reward.cpu().numpy(), term.cpu().numpy()
    state, time = _host_state(env)
    # booleans: equal to the reference on EVERY row, knife-edge rows (|margin| down to 0) included
    bad = np.nonzero(term != rows["term"])[0]
    assert bad.size == 0, "term differs on rows %s: margins %s" % (
        rows["index"][bad][:8], [(rows["m_border"][b], rows["m_obst"][b], rows["m_goal"][b]) for b in bad[:8]])
    assert np.array_equal(time, rows["time_out"])
    assert np.max(np.abs(obs[:, 0] - rows["pose"][:, 0])) <= TOL
    assert np.max(np.abs(obs[:, 1] - rows["pose"][:, 1])) <= TOL
    assert np.max(angle_diff(obs[:, 2], rows["pose"][:, 2])) <= TOL
    assert np.array_equal(obs[:, 3:5], rows["state_in"][:, 3:5].astype(np.float32))
    assert np.max(np.abs(reward - rows["reward"])) <= TOL
    assert np.max(np.abs(state[5] - rows["wave_out"][:, 0])) <= 1e-7
    assert np.max(np.abs(state[6] - rows["wave_out"][:, 1])) <= 1e-7
    assert np.array_equal(env.done_mask().cpu().numpy(), (rows["term"] != 0).astype(np.uint8))


def test_int_action_dtypes_agree(torch, golden):
    cfg = golden.cfg(3)
    rows = golden.rows(3)
    n = rows["term"].shape[0]
    outs = []
    for dt in (torch.uint8, torch.int32, torch.int64):
        env = _make(torch, n, cfg["obstacles"])
        env.set_state(rows["state_in"].astype(np.float32), rows["time_in"])
        noise = torch.zeros((2, env.ld), dtype=torch.float32, device="cuda:0")
        obs, reward, term = env.step(torch.as_tensor(rows["action_i"]).to(dt).cuda(), noise=noise)
        outs.append((obs.cpu().numpy().copy(), reward.cpu().numpy().copy(), term.cpu().numpy().copy()))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(a, b)
    # negative indices wrap like the reference's Python list (aqua.py:154)
    env = _make(torch, n, cfg["obstacles"])
    env.set_state(rows["state_in"].astype(np.float32), rows["time_in"])
    noise = torch.zeros((2, env.ld), dtype=torch.float32, device="cuda:0")
    obs, reward, term = env.step(torch.as_tensor(rows["action_i"].astype(np.int64) - 3).cuda(), noise=noise)
    assert np.array_equal(obs.cpu().numpy(), outs[0][0]) and np.array_equal(term.cpu().numpy(), outs[0][2])


# ------------------------------------------------------------------------------------------------
# (2) float64 oracle, Philox noise, sizes up to the benchmark batch
# ------------------------------------------------------------------------------------------------
def _compare_with_oracle(torch, oracle, env, state0, time0, action_np, reward, term, tick, noise_u=None):
    n = env.num_envs
    s64 = np.ascontiguousarray(state0.astype(np.float64))
    t = np.ascontiguousarray(time0.astype(np.int32))
    o_rew, o_term, margins = oracle.step(s64, t, action_np, obstacles=env.obstacle_rows, waves=env.has_waves,
                                         noise_u=noise_u, seed=env.seed, tick=tick, env_offset=env.env_offset)
    k_state, k_time = _host_state(env)
    mism = np.nonzero(o_term != term)[0]
    # any disagreement must sit on a margin below 1e-7 (device vs host libm in the float64 path); expected: none
    for i in mism:
        assert min(abs(margins[0][i]), abs(margins[1][i]), abs(margins[2][i])) < 1e-7, \
            "term mismatch at %d: kernel %d oracle %d margins %s" % (i, term[i], o_term[i], margins[:, i])
    assert mism.size == 0
    ok = np.ones(n, dtype=bool)
    assert np.max(np.abs(k_state[0] - s64[0])[ok]) <= TOL
    assert np.max(np.abs(k_state[1] - s64[1])[ok]) <= TOL
    assert np.max(angle_diff(k_state[2], s64[2])) <= TOL
    assert np.max(np.abs(k_state[5:7] - s64[5:7])) <= 1e-7
    assert np.max(np.abs(reward - o_rew)) <= TOL
    return s64, t, o_term


@pytest.mark.parametrize("obst,mode", [("bench8", 0), ("bench8", 2), ("default5", 0), ("difficult6", 2)])
def test_decisions_at_the_thresholds_at_scale(torch, oracle, obst, mode):
    """400 000 worlds per case whose POST-move position sits within +-3e-5 (log-uniform from 1e-9, both signs, and
    exactly 0) of a border, of the goal radius or of an obstacle surface -- the recipe of the golden knife-edge rows
    (tests/golden/make_golden.py), at the scale at which every band edge of the float32 path (plain 1e-4, compensated
    4e-6 in distance, per obstacle radius) is crossed thousands of times.  Termination codes must equal the
    float64 oracle's on every row; pose and reward within 1e-5."""
    from aquaticgymenv_amd import presets
    rows = {"bench8": presets.BENCH8, "default5": presets.DEFAULT5, "difficult6": presets.DIFFICULT6}[obst]
    n = 400000
    rng = np.random.RandomState(20261003 + mode)
    disc = np.array([(0.2, 0.5), (0.5, 0.2), (0.5, 0.5)])
    a = rng.randint(0, 3, n)
    vl, vr = disc[a, 0], disc[a, 1]
    theta = rng.uniform(-np.pi, np.pi, n).astype(np.float32).astype(np.float64)
    d = vr - vl
    d = np.copysign(np.maximum(np.abs(d), 1e-8), d)
    w = d / 2.5
    h = 0.5 * w
    chord = 0.5 * (vl + vr) * np.sin(h) / h
    dx, dy = -chord * np.sin(theta + h), chord * np.cos(theta + h)
    wave = rng.uniform(-0.05, 0.05, (2, n)).astype(np.float32).astype(np.float64)
    mag = 10.0 ** rng.uniform(-9, np.log10(3e-5), n)
    delta = np.where(rng.randint(0, 50, n) == 0, 0.0, mag * rng.choice([-1.0, 1.0], n))
    goal = rng.uniform(2.5, 97.5, (2, n))
    p = rng.uniform(10, 90, (2, n))
    what = rng.randint(0, 3, n)
    ang = rng.uniform(0, 2 * np.pi, n)
    # border
    b = what == 0
    axis = rng.randint(0, 2, n)
    lowside = rng.randint(0, 2, n) == 1
    val = np.where(lowside, 2.5 + delta, 97.5 - delta)
    p[0] = np.where(b & (axis == 0), val, p[0])
    p[1] = np.where(b & (axis == 1), val, p[1])
    # goal radius
    g = what == 1
    goal[0] = np.where(g, p[0] + (5.0 + delta) * np.cos(ang), goal[0])
    goal[1] = np.where(g, p[1] + (5.0 + delta) * np.sin(ang), goal[1])
    # obstacle surfaces
    o = what == 2
    oi = rng.randint(0, rows.shape[0], n)
    cx, cy, kind, pa, pb = (rows[oi, j] for j in range(5))
    circ = kind == 0
    px = cx + (pa + 2.5 + delta) * np.cos(ang)
    py = cy + (pa + 2.5 + delta) * np.sin(ang)
    hx, hy = pa / 2, pb / 2
    side = rng.randint(0, 5, n)
    u = rng.uniform(-1, 1, n)
    a4 = rng.uniform(0, np.pi / 2, n)
    rx = np.select([side == 0, side == 1, side == 2, side == 3],
                   [cx + hx + 2.5 + delta, cx - hx - 2.5 - delta, cx + u * hx, cx + u * hx], cx + hx + (2.5 + delta) * np.cos(a4))
    ry = np.select([side == 0, side == 1, side == 2, side == 3],
                   [cy + u * hy, cy + u * hy, cy + hy + 2.5 + delta, cy - hy - 2.5 - delta], cy + hy + (2.5 + delta) * np.sin(a4))
    p[0] = np.where(o, np.where(circ, px, rx), p[0])
    p[1] = np.where(o, np.where(circ, py, ry), p[1])
    state = np.stack([p[0] - dx - wave[0], p[1] - dy - wave[1], theta, goal[0], goal[1], wave[0], wave[1]]).astype(np.float32)
    env = _make(torch, n, rows, seed=5150, auto_reset=mode)
    env.reset()
    env.set_state(state, rng.randint(0, 990, n).astype(np.int32), soa=True)
    state0, time0 = _host_state(env)
    tick = env._tick
    act = a.astype(np.uint8)
    obs, reward, term = env.step(torch.as_tensor(act).cuda())
    torch.cuda.synchronize()
    term_h = term.cpu().numpy()
    if mode == 2:                                  # finished worlds keep their terminal pose and are marked
        done = term_h != 0
        tm = env.time[:n].cpu().numpy()
        assert np.all(tm[done] == -1 - (tick & 1)) and np.all(tm[~done] == time0[~done] + 1)
    _compare_with_oracle(torch, oracle, env, state0, time0, act, reward.cpu().numpy(), term_h, tick)
    assert 0.05 < float((term_h == 1).mean()) < 0.6 and float((term_h == 3).mean()) > 0.05      # both sides of each threshold


@pytest.mark.parametrize("n,continuous,obst", [(4096, False, "none"), (262144, False, "bench8"), (262144, True, "bench8"),
                                               (1000, True, "default5"), (65, False, "difficult6")])
def test_step_matches_oracle_philox(torch, oracle, n, continuous, obst):
    from aquaticgymenv_amd import presets
    rows = {"none": presets.NONE, "bench8": presets.BENCH8, "default5": presets.DEFAULT5,
            "difficult6": presets.DIFFICULT6}[obst]
    env = _make(torch, n, rows, continuous=continuous, seed=77, env_offset=3 * n)
    env.reset()
    rng = np.random.RandomState(5)
    # times near the limit for some worlds
    t0 = rng.randint(0, 1003, n).astype(np.int32)
    env.time[:n].copy_(torch.as_tensor(t0))
    for it in range(3):
        state0, time0 = _host_state(env)
        tick = env._tick
        if continuous:
            a = rng.uniform(0.15, 0.55, (n, 2)).astype(np.float32)
            a[::7, 1] = a[::7, 0]                       # epsilon branch
            obs, reward, term = env.step(torch.as_tensor(a).cuda())
            a_or = np.ascontiguousarray(a.T)
        else:
            a = rng.randint(0, 3, n).astype(np.uint8)
            obs, reward, term = env.step(torch.as_tensor(a).cuda())
            a_or = a
        torch.cuda.synchronize()
        _compare_with_oracle(torch, oracle, env, state0, time0, a_or, reward.cpu().numpy(), term.cpu().numpy(), tick)


@pytest.mark.parametrize("n,steps,continuous", [(262144, 10, False), (262144, 10, True), (1 << 19, 4, False)],
                         ids=["configs2_u8_262144", "configs3_f32x2_262144", "interleaved_grid_524288"])
def test_benchmarked_instantiation_against_oracle_at_benchmark_size(torch, oracle, n, steps, continuous):
    """the kernels bench.py times -- step_ns_kernel<U8 | F32X2, small table, head-of-grid roles> at 262 144 worlds
    (BASELINE.json configs[2] and configs[3]) and its interleaved-roles layout (>= 524 288 worlds) -- at THEIR size against
    the oracle: codes and time markers bit-exact, floats within 1e-5, restarted worlds bit for bit"""
    from aquaticgymenv_amd import presets
    finished, restarted = _buffered_rollout_against_oracle(torch, oracle, presets.BENCH8, n, steps, continuous, 2)
    assert finished > n // 100 and restarted > n // 100, "the rollout must exercise the restart path"


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["no_restart", "same_step", "next_step"])
def test_launch_events_bracket_the_rollout(torch, mode):
    """rollout(events=LaunchEvents()): the events ride on the first and the last step launch (hipExtLaunchKernel) -- same
    results as without them, and first kernel start -> last kernel end lies inside two events recorded around the call"""
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.batched import LaunchEvents
    n, steps = 70001, 12
    envs = [_make(torch, n, presets.BENCH8, seed=17, auto_reset=mode) for _ in range(2)]
    ev = LaunchEvents()
    out = []
    for env, events in zip(envs, (None, ev)):
        env.reset()
        env.rollout(3, actions="random")                                  # (warm: code object, buffers)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rew, term = env.rollout(steps, actions="random", events=events)
        e1.record()
        torch.cuda.synchronize()
        out.append((env.state.clone(), env.time.clone(), rew, term))
    for a, b in zip(*out):
        assert torch.equal(a[..., :n], b[..., :n])
    inside, around = ev.elapsed_ms(), e0.elapsed_time(e1)
    assert 0.0 < inside <= around, (inside, around)
    assert inside > steps * 1.0e-3                                        # twelve launches take more than 12 us
    one = LaunchEvents()
    envs[1].rollout(1, actions="random", events=one)                      # first launch == last launch
    torch.cuda.synchronize()
    assert 0.0 < one.elapsed_ms() < inside
    with pytest.raises(ValueError):
        envs[1].rollout(4, actions="random", fused=True, events=one)
    # the same call marshalled once (prepare_rollout): what bench.py's one-block regions launch
    a, b = envs
    pa = a.prepare_rollout(steps, actions="random", keep_all=True)
    pb = b.prepare_rollout(steps, actions="random", keep_all=True, events=ev)
    b.rollout(1, actions="random"); a.rollout(1, actions="random")       # (b is one step ahead of a since `one` above)
    a.rollout(1, actions="random")
    for _ in range(2):
        ra, ta = pa.launch()
        rb, tb = pb.launch()
    torch.cuda.synchronize()
    assert a._tick == b._tick
    assert torch.equal(a.state[:, :n], b.state[:, :n]) and torch.equal(ra[:, :n], rb[:, :n]) and torch.equal(ta[:, :n], tb[:, :n])
    assert ev.elapsed_ms() > 0.0
    ev.close(); one.close()


@pytest.mark.parametrize("mode", [1, 2], ids=["same_step", "next_step"])
def test_large_batch_store_policy_equals_its_shards(torch, mode):
    """From 2 097 152 worlds on the restart kernels leave their stores to the L2's write-back (aqua_hip.hip, STORE_WB_*);
    smaller batches write them through.  A world's trajectory depends on (seed, world index, tick) only, so one batch of
    2 M worlds must equal, bit for bit, the same worlds stepped as shards of at most 262 144 (the oracle-checked kernels)."""
    from aquaticgymenv_amd import presets
    n, steps, shard = (1 << 21) + 1029, 8, 262144
    whole = _make(torch, n, presets.BENCH8, seed=31, auto_reset=mode)
    whole.reset()
    w_rew, w_term = whole.rollout(steps, actions="random", keep_all=True)
    ended = 0
    for first in range(0, n, shard):
        m = min(shard, n - first)
        part = _make(torch, m, presets.BENCH8, seed=31, auto_reset=mode, env_offset=first)
        part.reset()
        p_rew, p_term = part.rollout(steps, actions="random", keep_all=True)
        assert torch.equal(part.state[:, :m], whole.state[:, first:first + m])
        assert torch.equal(part.time[:m], whole.time[first:first + m])
        assert torch.equal(p_rew[:, :m], w_rew[:, first:first + m])
        assert torch.equal(p_term[:, :m], w_term[:, first:first + m])
        ended += int((p_term[:, :m] != 0).sum())
    assert ended > n // 20, "the rollout must exercise the restart path"


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["no_restart", "same_step", "next_step"])
def test_a_batch_beyond_one_launch_is_split_and_equals_its_shards(torch, mode):
    """The step kernels address a world by a 32-bit byte offset from the row pointers of their launch, so the library steps
    a batch of more than 2^28 worlds as several launches (aqua_hip.hip, NS_LAUNCH_MAX_WORLDS), each with its own pointers,
    env_offset and tick housekeeping.  268 M worlds (10 GB of state): the worlds on either side of the seam, and the
    first and last ones, must equal the same worlds stepped as small batches of their own."""
    from aquaticgymenv_amd import presets
    seam = 1 << 28
    n, steps = seam + 3 * 1024 + 77, 3
    whole = _make(torch, n, presets.BENCH8, seed=47, auto_reset=mode)
    whole.reset()
    whole.rollout(steps, actions="random", keep_all=False)
    graph = whole.capture_rollout(2, actions="random")          # (a captured rollout: the tick housekeeping of a split launch)
    graph.launch()
    torch.cuda.synchronize()
    for first, m in ((0, 4096), (seam - 2048, 2048 + 3 * 1024 + 77), (1 << 27, 1000)):
        part = _make(torch, m, presets.BENCH8, seed=47, auto_reset=mode, env_offset=first)
        part.reset()
        part.rollout(steps, actions="random", keep_all=False)
        part.capture_rollout(2, actions="random").launch()
        torch.cuda.synchronize()
        assert torch.equal(part.state[:, :m], whole.state[:, first:first + m])
        assert torch.equal(part.time[:m], whole.time[first:first + m])
        assert torch.equal(part.reward[:m], whole.reward[first:first + m])
        assert torch.equal(part.term[:m], whole.term[first:first + m])
        assert torch.equal(part.done_bits[: m // 64], whole.done_bits[first // 64: first // 64 + m // 64])
    assert int((whole.time[:n] != 0).sum()) > 0
    del whole
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mode,env_offset", [(1, 0), (2, 0), (2, 7)], ids=["same_step", "next_step", "next_step_odd_offset"])
def test_sampled_actions_match_oracle_rollout(torch, oracle, mode, env_offset):
    """40 steps, discrete and continuous.  mode 1: finished worlds are re-seeded in the launch that finished them;
    mode 2 (next-step): they are marked pending (time == -1 - (tick & 1)) and re-seeded during the next step, which
    reports reward 0 / term 0.  (An odd env_offset puts the two worlds of a Philox pair on lanes 2i + 1, 2i + 2:
    the per-lane fallback.)"""
    from aquaticgymenv_amd import presets
    n = 8192 + 37
    for continuous in (False, True):
        finished = _rollout_against_oracle(torch, oracle, presets.BENCH8, n, 40, continuous, mode, env_offset)
        assert finished > n // 4


def _obstacle_mix(n_circles, n_rects, seed):
    """reference-format rows [K][5] in the given order of kinds (circles and rectangles interleaved at random)"""
    rng = np.random.RandomState(seed)
    kinds = np.array([0.0] * n_circles + [1.0] * n_rects)
    rng.shuffle(kinds)
    rows = np.zeros((len(kinds), 5))
    rows[:, 0:2] = rng.uniform(12, 88, (len(kinds), 2))
    rows[:, 2] = kinds
    rows[:, 3] = np.where(kinds == 0, rng.uniform(2, 6, len(kinds)), rng.uniform(4, 12, len(kinds)))
    rows[:, 4] = np.where(kinds == 0, 0.0, rng.uniform(4, 12, len(kinds)))
    return rows


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["no_restart", "same_step", "next_step"])
@pytest.mark.parametrize("mix", [(1, 0), (0, 1), (3, 2), (5, 0), (0, 5), (8, 0), (0, 8), (7, 1), (1, 6), (4, 4), (9, 3), (2, 14)],
                         ids=lambda m: "c%dr%d" % m)
def test_obstacle_table_shapes_match_oracle_rollout(torch, oracle, mix, mode):
    """every shape of the quick table (first groups only, second circle group, second rectangle group, both, none of
    a kind) and tables too long to have one (K > 8: the row loops), in every restart mode, per-step kernels against
    the oracle and the fused rollout against the per-step kernels."""
    rows = _obstacle_mix(mix[0], mix[1], seed=mix[0] * 17 + mix[1])
    n = 3000 + 11
    if mode == 0:
        env = _make(torch, n, rows, seed=5, auto_reset=False)
        env.reset()
        rng = np.random.RandomState(3)
        for it in range(25):
            s0, t0 = _host_state(env)
            tick = env._tick
            act = rng.randint(0, 3, n).astype(np.uint8)
            obs, reward, term = env.step(torch.as_tensor(act).cuda())
            torch.cuda.synchronize()
            s64 = np.ascontiguousarray(s0.astype(np.float64))
            t = np.ascontiguousarray(t0.astype(np.int32))
            o_rew, o_term, margins = oracle.step(s64, t, act, obstacles=rows, waves=1, seed=5, tick=tick)
            k_state, k_time = _host_state(env)
            assert np.array_equal(term.cpu().numpy(), o_term)
            assert np.max(np.abs(k_state[0:2] - s64[0:2])) <= TOL and np.max(np.abs(reward.cpu().numpy() - o_rew)) <= TOL
        return
    finished = _rollout_against_oracle(torch, oracle, rows, n, 25, False, mode, 0, seed=5)
    assert finished > 0
    a = _make(torch, n, rows, seed=6, auto_reset=mode)
    b = _make(torch, n, rows, seed=6, auto_reset=mode)
    a.reset(); b.reset()
    ra, ta = a.rollout(30, fused=False, keep_all=True)
    rb, tb = b.rollout(30, fused=True, keep_all=True)
    assert torch.equal(ra[:, :n], rb[:, :n]) and torch.equal(ta[:, :n], tb[:, :n])          # (columns n.. are padding)
    assert torch.equal(a.state[:, :n], b.state[:, :n]) and torch.equal(a.time[:n], b.time[:n])


FUZZ_CASES = int(__import__("os").environ.get("AQUA_FUZZ_CASES", "12"))
FUZZ_FIRST = int(__import__("os").environ.get("AQUA_FUZZ_FIRST", "0"))      # (a longer campaign continues where the last one stopped)


@pytest.mark.parametrize("case", range(FUZZ_FIRST, FUZZ_FIRST + FUZZ_CASES))
def test_random_configurations_against_the_oracle(torch, oracle, case):
    """Seeded random configurations -- obstacle mix (0-20 rows: every quick-table shape and the row loops), batch size
    (1 to a few thousand, ragged), action space, restart mode, world offset (even, odd, beyond 2^32), sampled or buffered
    actions -- each a teacher-forced rollout against the oracle with the bars of every other test (codes, markers and
    re-seeded states bit for bit, floats within 1e-5).  AQUA_FUZZ_CASES=N runs N of them (default 12; 330 passed on the round-4 build: profiles/r04/fuzz/)."""
    rng = np.random.RandomState(7000 + case)
    if rng.randint(0, 4) == 0:
        n_c, n_r = int(rng.randint(0, 11)), int(rng.randint(0, 11))
    else:
        n_c = int(rng.randint(0, 9))
        n_r = int(rng.randint(0, 9 - n_c))
    rows = _obstacle_mix(n_c, n_r, seed=case) if n_c + n_r else np.zeros((0, 5))
    n = int(rng.choice([1, 2, 63, 64, 65, 255, 257, 1023, int(rng.randint(1000, 6000))]))
    steps = int(rng.randint(12, 31))
    continuous = bool(rng.randint(0, 2))
    env_offset = int(rng.choice([0, 0, 1, 7, 2 ** 32 - 3, 2 ** 33 + 5]))
    seed = int(rng.randint(0, 2 ** 31))
    if rng.randint(0, 3) == 0:
        finished, restarted = _buffered_rollout_against_oracle(torch, oracle, rows, n, steps, continuous, 2, seed=seed)
    else:
        finished = _rollout_against_oracle(torch, oracle, rows, n, steps, continuous, int(rng.randint(1, 3)), env_offset, seed=seed)
    assert finished >= 0


def test_masked_reset_between_steps_does_not_delay_restarts(torch):
    """next-step mode: the restart markers carry the parity of the step tick; a reset(mask) between two steps
    draws from its own tick range, so the worlds that finished in the step before it still restart in the step
    after it (time == -3 - (tick & 1)), and the worlds it placed step normally."""
    from aquaticgymenv_amd import presets
    n = 20000
    env = _make(torch, n, presets.BENCH8, seed=31, auto_reset="next_step")
    env.reset()
    for _ in range(30):
        env.step(sample_actions=True)
    obs, reward, term = env.step(sample_actions=True)
    finished = (term != 0).cpu().numpy()
    assert finished.sum() > 50
    mask = np.zeros(n, dtype=np.uint8)
    mask[np.flatnonzero(~finished)[:100]] = 1
    env.reset(mask=torch.as_tensor(mask).cuda())
    tick = env._tick
    obs, reward, term = env.step(sample_actions=True)
    torch.cuda.synchronize()
    t = env.time[:n].cpu().numpy()
    assert np.all(t[finished] == -3 - (tick & 1))
    assert np.all(reward.cpu().numpy()[finished] == 0) and np.all(term.cpu().numpy()[finished] == 0)
    placed = mask != 0
    assert np.all((t[placed] == 1) | (t[placed] == -1 - (tick & 1)))      # stepped once (or finished at once)


def _random_tables(rng, n, K):
    """[n][K][5] reference-format rows: circles (radius 2..10) and rectangles (5..15 x 5..15), some rows absent.  Tables of
    more than 16 rows hold smaller obstacles (sizes x sqrt(10 / K)), so that about half of a world stays free."""
    t = np.zeros((n, K, 5))
    t[:, :, 0:2] = rng.uniform(10, 90, (n, K, 2))
    kind = rng.randint(0, 2, (n, K)).astype(np.float64)
    t[:, :, 2] = kind
    scale = 1.0 if K <= 16 else (10.0 / K) ** 0.5
    t[:, :, 3] = np.where(kind == 0, rng.uniform(2, 10, (n, K)), rng.uniform(5, 15, (n, K))) * scale
    t[:, :, 4] = np.where(kind == 0, 0.0, rng.uniform(5, 15, (n, K)) * scale)
    t[:, :, 2] = np.where(rng.randint(0, 5, (n, K)) == 0, -1.0, t[:, :, 2])        # ~20 % absent rows
    return t


def test_per_world_tables_equal_the_shared_table_when_all_worlds_hold_the_same_list(torch):
    """every world gets its own copy of BENCH8 (row order shuffled per world): reset and 30 steps are bit-identical
    to the shared-table kernels (auto_reset none)."""
    from aquaticgymenv_amd import presets
    n = 20000 + 13
    rng = np.random.RandomState(8)
    tables = np.stack([presets.BENCH8[rng.permutation(8)] for _ in range(n)])
    shared = _make(torch, n, presets.BENCH8, seed=321, auto_reset=False)
    mine = _make(torch, n, tables, seed=321, auto_reset=False)
    shared.reset(); mine.reset()
    assert torch.equal(shared.state, mine.state) and torch.equal(shared.time, mine.time)
    g = torch.Generator(device="cuda").manual_seed(1)
    for _ in range(30):
        act = torch.randint(0, 3, (n,), device="cuda", generator=g, dtype=torch.int64).to(torch.uint8)
        _, r1, t1 = shared.step(act)
        _, r2, t2 = mine.step(act)
        assert torch.equal(t1, t2) and torch.equal(r1, r2)
    assert torch.equal(shared.state, mine.state) and torch.equal(shared.time, mine.time)
    assert torch.equal(shared.done_mask(), mine.done_mask())


def test_per_world_tables_same_step_restart_is_a_masked_reset_with_the_steps_tick(torch):
    """auto_reset='same_step' with per-world tables (restart inside the step launch, 8 lanes per finished world) ==
    step() followed by the masked reset launch (mask = term, draws of the step's tick) by hand, bit for bit; the
    masked reset itself is pinned to the oracle in the tests below."""
    import ctypes
    from aquaticgymenv_amd import _capi
    n, K = 30000 + 5, 5
    rng = np.random.RandomState(4)
    tables = _random_tables(rng, n, K)
    auto = _make(torch, n, tables, seed=66, auto_reset="same_step", normalized_obs=True)
    hand = _make(torch, n, tables, seed=66, auto_reset=False, normalized_obs=True)
    auto.reset(); hand.reset()
    g = torch.Generator(device="cuda").manual_seed(5)
    ended = 0
    for _ in range(25):
        act = torch.randint(0, 3, (n,), device="cuda", generator=g, dtype=torch.int64).to(torch.uint8)
        tick = hand._tick
        _, r1, t1 = auto.step(act)
        _, r2, t2 = hand.step(act)
        _capi.check(_capi.lib.aqua_reset_tables_f32(ctypes.byref(hand.params), hand._tab32.data_ptr(), hand.K, hand.ld, n,
                                                    hand.env_offset, hand.state.data_ptr(), hand.ld, hand.time.data_ptr(),
                                                    hand.term.data_ptr(), hand.seed, tick, None, hand._stream()),
                    "aqua_reset_tables_f32")
        _capi.check(_capi.lib.aqua_obs_norm_f32(hand.state.data_ptr(), hand.ld, n, hand.term.data_ptr(), hand._norm_ptr(),
                                                hand._stream()), "aqua_obs_norm_f32")
        assert torch.equal(t1, t2) and torch.equal(r1, r2)
        assert torch.equal(auto.done_mask(), hand.done_mask())
        ended += int((t1 != 0).sum())
    assert torch.equal(auto.state[:, :n], hand.state[:, :n]) and torch.equal(auto.time[:n], hand.time[:n])
    assert torch.equal(auto.obs_norm, hand.obs_norm) and ended > n // 10 and int(auto.time[:n].min()) >= 0


@pytest.mark.parametrize("continuous", [False, True])
def test_per_world_tables_match_the_oracle(torch, oracle, continuous):
    """one random obstacle list per world (6 rows, some absent): reset bit for bit, steps against the float64
    oracle with the same per-world lists (termination codes equal, floats within 1e-5), masked reset."""
    n, K = 60000 + 7, 6
    rng = np.random.RandomState(99)
    tables = _random_tables(rng, n, K)
    env = _make(torch, n, tables, continuous=continuous, seed=2024, auto_reset=False, env_offset=128)
    env.reset()
    torch.cuda.synchronize()
    k_state, k_time = _host_state(env)
    st = np.zeros((7, n), dtype=np.float32)
    tt = np.full(n, 7, dtype=np.int32)
    oracle.reset_tables(st, tt, tables, waves=1, seed=2024, tick=env.RESET_TICK_BASE, env_offset=128)
    assert np.array_equal(k_state, st) and np.array_equal(k_time, tt)
    finished = 0
    for it in range(12):
        state0, time0 = _host_state(env)
        tick = env._tick
        if continuous:
            act = (0.2 + 0.3 * rng.uniform(size=(2, env.ld))).astype(np.float32)
            obs, reward, term = env.step(torch.as_tensor(act).cuda(), soa=True)
            act = np.ascontiguousarray(act[:, :n])
        else:
            act = rng.randint(0, 3, n).astype(np.uint8)
            obs, reward, term = env.step(torch.as_tensor(act).cuda())
        torch.cuda.synchronize()
        s64 = np.ascontiguousarray(state0.astype(np.float64))
        t = np.ascontiguousarray(time0.astype(np.int32))
        o_rew, o_term, margins = oracle.step_tables(s64, t, act, tables, waves=1, seed=2024, tick=tick, env_offset=128)
        k_state, k_time = _host_state(env)
        term_h = term.cpu().numpy()
        assert np.array_equal(term_h, o_term)
        assert np.max(np.abs(k_state[0:2] - s64[0:2])) <= TOL and np.max(angle_diff(k_state[2], s64[2])) <= TOL
        assert np.max(np.abs(k_state[5:7] - s64[5:7])) <= 1e-7 and np.max(np.abs(reward.cpu().numpy() - o_rew)) <= TOL
        assert np.array_equal(k_time, t)
        finished += int((o_term != 0).sum())
        mask = term_h != 0
        env.reset(mask=torch.as_tensor(mask).cuda())
        torch.cuda.synchronize()
        k2, t2 = _host_state(env)
        st = k_state.copy(); tt = k_time.copy()
        oracle.reset_tables(st, tt, tables, waves=1, seed=2024, tick=env.RESET_TICK_BASE + it + 1, env_offset=128, mask=mask)
        assert np.array_equal(k2, st) and np.array_equal(t2, tt)
    assert finished > n // 20


@pytest.mark.parametrize("continuous", [False, True])
def test_per_world_tables_next_step_restart_matches_the_oracle(torch, oracle, continuous):
    """auto_reset='next_step' with one obstacle list per world (six rows: the restart inside the stepping tile, the rows handed
    over through LDS to the re-seeding lanes): every tick against the oracle -- termination codes, markers in the time row and the re-seeded
    states bit for bit, floats of the stepped worlds within 1e-5 (teacher-forced: the oracle restarts every tick from the
    kernel's state)."""
    n, K = 40000 + 3, 6
    rng = np.random.RandomState(17)
    tables = _random_tables(rng, n, K)
    env = _make(torch, n, tables, continuous=continuous, seed=515, auto_reset="next_step", env_offset=64)
    env.reset()
    restarted = 0
    for it in range(40):
        st, tt = _host_state(env)
        st, tt = st.copy(), tt.copy()
        tick = env._tick
        if continuous:
            act = (0.2 + 0.3 * rng.uniform(size=(2, env.ld))).astype(np.float32)
            _, reward, term = env.step(torch.as_tensor(act).cuda(), soa=True)
            act = np.ascontiguousarray(act[:, :n])
        else:
            act = rng.randint(0, 3, n).astype(np.uint8)
            _, reward, term = env.step(torch.as_tensor(act).cuda())
        torch.cuda.synchronize()
        was_restart = tt == -1 - ((tick - 1) & 1)
        o_rew, o_term = _oracle_next_step_tables(oracle, st, tt, act, tables, 515, tick, 64)
        k_state, k_time = _host_state(env)
        assert np.array_equal(term.cpu().numpy(), o_term) and np.array_equal(k_time, tt)
        assert np.array_equal(k_state[:, was_restart], st[:, was_restart])                 # re-seeded: bit for bit
        assert np.max(np.abs(k_state[0:2] - st[0:2])) <= TOL and np.max(angle_diff(k_state[2], st[2])) <= TOL
        assert np.max(np.abs(k_state[5:7] - st[5:7])) <= 1e-7 and np.max(np.abs(reward.cpu().numpy() - o_rew)) <= TOL
        assert np.array_equal(env.done_mask().cpu().numpy(), (o_term != 0).astype(np.uint8))
        restarted += int(was_restart.sum())
    assert restarted > n // 20


@pytest.mark.parametrize("mode", ["none", "same_step", "next_step"])
def test_per_world_tables_rollout_and_graph_equal_single_steps(torch, mode):
    """rollout() (T launches from C) and capture_rollout() (HIP graph, replayed) with per-world tables == step() called T
    times, bit for bit, for stored, sampled and bearing-policy actions; the graph's ticks advance across replays."""
    n, K, T = 20000 + 9, 5, 12
    rng = np.random.RandomState(23)
    tables = _random_tables(rng, n, K)
    acts = torch.as_tensor(rng.randint(0, 3, (3 * T, n)).astype(np.uint8)).cuda()
    for actions in ("stored", "random", "bearing"):
        ref = _make(torch, n, tables, seed=31, auto_reset=mode)
        roll = _make(torch, n, tables, seed=31, auto_reset=mode)
        graph_env = _make(torch, n, tables, seed=31, auto_reset=mode)
        for e in (ref, roll, graph_env):
            e.reset()
        want_r, want_t = [], []
        for t in range(3 * T):
            if actions == "stored":
                _, r, c = ref.step(acts[t])
            else:
                _, r, c = ref.step(policy=actions)
            want_r.append(r.clone()); want_t.append(c.clone())
        for rep in range(3):
            a = acts[rep * T:(rep + 1) * T] if actions == "stored" else actions
            r, c = roll.rollout(T, actions=a, keep_all=True)
            for t in range(T):
                assert torch.equal(r[t, :n], want_r[rep * T + t]) and torch.equal(c[t, :n], want_t[rep * T + t])
        assert torch.equal(roll.state, ref.state) and torch.equal(roll.time, ref.time)
        if actions != "stored":
            g = graph_env.capture_rollout(T, actions=actions, keep_all=True)
            for rep in range(3):
                r, c = g.launch()
                torch.cuda.synchronize()
                for t in range(T):
                    assert torch.equal(r[t, :n], want_r[rep * T + t]) and torch.equal(c[t, :n], want_t[rep * T + t])
            assert torch.equal(graph_env.state, ref.state) and torch.equal(graph_env.time, ref.time)
            assert graph_env._tick == ref._tick
        # the fused rollout (state in registers, the block's tables in LDS): eager and as a replayed graph
        fused, fgraph = (_make(torch, n, tables, seed=31, auto_reset=mode) for _ in range(2))
        fused.reset(); fgraph.reset()
        g = fgraph.capture_rollout(T, actions=acts[:T] if actions == "stored" else actions, fused=True, keep_all=True)
        for rep in range(3):
            a = acts[rep * T:(rep + 1) * T] if actions == "stored" else actions
            r, c = fused.rollout(T, actions=a, fused=True, keep_all=True)
            for t in range(T):
                assert torch.equal(r[t, :n], want_r[rep * T + t]) and torch.equal(c[t, :n], want_t[rep * T + t])
            if actions != "stored":                       # (a graph replays the action rows it captured)
                r, c = g.launch()
                torch.cuda.synchronize()
                for t in range(T):
                    assert torch.equal(r[t, :n], want_r[rep * T + t]) and torch.equal(c[t, :n], want_t[rep * T + t])
        assert torch.equal(fused.state, ref.state) and torch.equal(fused.time, ref.time)
        if actions != "stored":
            assert torch.equal(fgraph.state, ref.state) and torch.equal(fgraph.time, ref.time)


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["none", "same_step", "next_step"])
@pytest.mark.parametrize("K", [9, 11, 16, 17, 32, 41, 64])
def test_long_per_world_tables_against_the_oracle_and_fused(torch, oracle, K, mode):
    """per-world tables of more than eight rows (aqua.py:56-68: a list of any length per env object), up to the library's 64:
    the one-launch-per-step kernels against the oracle's step_tables / reset_tables in every restart mode (codes and markers
    bit-exact, restarted worlds bit for bit, floats within 1e-5), and the fused rollout -- its LDS tile of 16 rows x 256
    worlds, 32 x 128 or 64 x 64 -- against those launches, bit for bit, eagerly and as a replayed graph"""
    n, T = (9000 + 5, 24) if K <= 16 else (2300 + 5, 24)     # (ragged against every tile width: 256, 128, 64)
    restarted = _per_world_tables_against_the_oracle_and_fused(torch, oracle, K, mode, n, T, 100 + K)
    if mode:
        assert restarted > n // 20


FUZZ_TABLE_CASES = int(__import__("os").environ.get("AQUA_FUZZ_TABLE_CASES", "6"))


@pytest.mark.parametrize("case", range(FUZZ_FIRST, FUZZ_FIRST + FUZZ_TABLE_CASES))
def test_random_per_world_tables_against_the_oracle_and_fused(torch, oracle, case):
    """the same comparison for seeded random table lengths (1 to 64 rows: every kernel instantiation and every row count
    inside it), batch sizes and restart modes.  AQUA_FUZZ_TABLE_CASES=N runs N of them (default 6)."""
    rng = np.random.RandomState(9000 + case)
    K = int(rng.randint(1, 65)) if rng.randint(0, 2) else int(rng.randint(1, 17))
    n = int(rng.choice([1, 63, 65, 129, 257, int(rng.randint(300, 3000))]))
    _per_world_tables_against_the_oracle_and_fused(torch, oracle, K, int(rng.randint(0, 3)), n, int(rng.randint(8, 25)), 9000 + case)


def _per_world_tables_against_the_oracle_and_fused(torch, oracle, K, mode, n, T, seed):
    rng = np.random.RandomState(seed)
    tables = _random_tables(rng, n, K)
    acts = torch.as_tensor(rng.randint(0, 3, (T, n)).astype(np.uint8)).cuda()
    env = _make(torch, n, tables, seed=77, auto_reset=mode, env_offset=64)
    env.reset()
    want_r, want_t, restarted = [], [], 0
    for it in range(T):
        st, tt = _host_state(env)
        st, tt = st.copy(), tt.copy()
        tick = env._tick
        _, reward, term = env.step(acts[it])
        torch.cuda.synchronize()
        want_r.append(reward.clone()); want_t.append(term.clone())
        act = acts[it].cpu().numpy()
        k_state, k_time = _host_state(env)
        if mode == 2:
            was_restart = tt == -1 - ((tick - 1) & 1)
            o_rew, o_term = _oracle_next_step_tables(oracle, st, tt, act, tables, 77, tick, 64)
            assert np.array_equal(k_time, tt)
            assert np.array_equal(k_state[:, was_restart], st[:, was_restart])
            moved = ~was_restart
            restarted += int(was_restart.sum())
        else:
            s64 = np.ascontiguousarray(st.astype(np.float64))
            o_rew, o_term, _ = oracle.step_tables(s64, tt, act, tables, waves=1, seed=77, tick=tick, env_offset=64)
            moved = np.ones(n, dtype=bool)
            st = s64.astype(np.float32)
            if mode == 1:                                   # same-step restart == masked reset with the step's tick
                fin = o_term != 0
                fresh = np.ascontiguousarray(st.copy())
                oracle.reset_tables(fresh, tt, tables, waves=1, seed=77, tick=tick, env_offset=64, mask=fin)
                assert np.array_equal(k_state[:, fin], fresh[:, fin]) and np.all(k_time[fin] == 0)
                moved = ~fin
                restarted += int(fin.sum())
            o_rew = o_rew.astype(np.float32)
        assert np.array_equal(term.cpu().numpy(), o_term)
        assert np.max(np.abs(reward.cpu().numpy() - o_rew)) <= TOL
        if moved.any():
            assert np.max(np.abs(k_state[0:2, moved] - st[0:2, moved])) <= TOL
            assert np.max(angle_diff(k_state[2, moved], st[2, moved])) <= TOL
            assert np.max(np.abs(k_state[5:7, moved] - st[5:7, moved])) <= 1e-7
    fused, fgraph = (_make(torch, n, tables, seed=77, auto_reset=mode, env_offset=64) for _ in range(2))
    fused.reset(); fgraph.reset()
    r, c = fused.rollout(T, actions=acts, fused=True, keep_all=True)
    g = fgraph.capture_rollout(T, actions=acts, fused=True, keep_all=True)
    r2, c2 = g.launch()
    torch.cuda.synchronize()
    for t in range(T):
        assert torch.equal(r[t, :n], want_r[t]) and torch.equal(c[t, :n], want_t[t]), "fused rollout differs at step %d" % t
        assert torch.equal(r2[t, :n], want_r[t]) and torch.equal(c2[t, :n], want_t[t])
    for other in (fused, fgraph):
        assert torch.equal(other.state[:, :n], env.state[:, :n]) and torch.equal(other.time[:n], env.time[:n])
    return restarted


def test_per_world_next_step_equals_the_shared_table_kernel(torch):
    """all worlds hold (a permutation of) BENCH8: the per-world next-step kernel == step_ns_kernel bit for bit over 60 ticks,
    in both grid layouts (the second batch is large enough to interleave the roles)."""
    from aquaticgymenv_amd import presets
    for n in (20000 + 13, 600000 + 77):
        rng = np.random.RandomState(8)
        tables = np.stack([presets.BENCH8[rng.permutation(8)] for _ in range(n)])
        shared = _make(torch, n, presets.BENCH8, seed=321, auto_reset="next_step")
        mine = _make(torch, n, tables, seed=321, auto_reset="next_step")
        shared.reset(); mine.reset()
        r1, t1 = shared.rollout(60, keep_all=True)
        r2, t2 = mine.rollout(60, keep_all=True)
        assert torch.equal(t1[:, :n], t2[:, :n]) and torch.equal(r1[:, :n], r2[:, :n])      # (columns n.. are padding)
        assert torch.equal(shared.state[:, :n], mine.state[:, :n]) and torch.equal(shared.time[:n], mine.time[:n])
        assert int((t1[:, :n] != 0).sum()) > n // 4


@pytest.mark.parametrize("mode", ["same_step", "next_step"])
@pytest.mark.parametrize("rows", [8, 11, 10, 21, 64], ids=["rows8_handoff", "rows11_handoff16", "rows10_streamed", "rows21_streamed", "rows64_streamed"])
def test_per_world_restart_of_every_world_at_once(torch, mode, rows):
    """every world of every wavefront restarts in the same step (all past the time limit): the LDS hand-off of the rows
    (tables of up to 8 rows, 11..16 with restarts) then takes eight rounds per tile; == the shared-table kernels bit for
    bit.  9, 10 and 17..64 rows: next-step, the rows left in LDS by the lane that streams them (three slots per wavefront:
    22 rounds here, all but the first with the rows read again by their own lane); same-step, the groups read the rows
    from memory.  Odd and even lengths (the re-seeding pass tests two rows at a time)."""
    from aquaticgymenv_amd import presets
    n = 3000 + 7
    extra = {8: None, 11: (2, 1), 10: (1, 1), 21: (6, 7), 64: (30, 26)}[rows]
    base = presets.BENCH8 if extra is None else np.concatenate([presets.BENCH8, _obstacle_mix(extra[0], extra[1], 5)])
    if rows == 64:
        base[8:, 3:5] *= 0.3                                     # (64 obstacles of that size would leave no free place)
    assert base.shape[0] == rows
    tables = np.repeat(base[None], n, axis=0)
    shared = _make(torch, n, base, seed=99, auto_reset=mode)
    mine = _make(torch, n, tables, seed=99, auto_reset=mode)
    for e in (shared, mine):
        e.reset()
        e.time[:n].fill_(1005)
    r1, t1 = shared.rollout(6, keep_all=True)
    r2, t2 = mine.rollout(6, keep_all=True)
    assert int((t1[0, :n] != 0).sum()) == n                      # everybody finished in the first step
    assert torch.equal(t1[:, :n], t2[:, :n]) and torch.equal(r1[:, :n], r2[:, :n])
    assert torch.equal(shared.state[:, :n], mine.state[:, :n]) and torch.equal(shared.time[:n], mine.time[:n])
    if rows == 8:                                                # ... and the fused per-world rollout
        fused = _make(torch, n, tables, seed=99, auto_reset=mode)
        fused.reset()
        fused.time[:n].fill_(1005)
        r3, t3 = fused.rollout(6, fused=True, keep_all=True)
        assert torch.equal(t1[:, :n], t3[:, :n]) and torch.equal(r1[:, :n], r3[:, :n])
        assert torch.equal(shared.state[:, :n], fused.state[:, :n]) and torch.equal(shared.time[:n], fused.time[:n])


@pytest.mark.parametrize("density", [0.002, 0.03, 0.12, 0.13, 0.6, 1.0])
def test_per_world_masked_reset_sparse_and_dense_masks_match_the_oracle(torch, oracle, density):
    """the masked reset re-seeds few selected worlds eight lanes per world and many one world per lane (the switch is
    per 1024-world block at 128 selected): both bit for bit the oracle's, and unselected worlds are untouched.
    Crowded tables (9 rows with large obstacles) so that later attempt rounds are exercised."""
    n, K = 20000 + 333, 9
    rng = np.random.RandomState(int(density * 1000) + 5)
    tables = _random_tables(rng, n, K)
    tables[:, :, 3] *= 2.5                                     # radii / widths: more rejected placements
    env = _make(torch, n, tables, seed=77, auto_reset=False, env_offset=4096)
    env.reset()
    torch.cuda.synchronize()
    st, tt = _host_state(env)
    mask = rng.uniform(size=n) < density
    mask[1024:2048] = rng.uniform(size=1024) < 0.124          # one block just below the switch, one just above
    mask[2048:3072] = rng.uniform(size=1024) < 0.127
    env.reset(mask=torch.as_tensor(mask).cuda())
    torch.cuda.synchronize()
    k2, t2 = _host_state(env)
    want_s, want_t = st.copy(), tt.copy()
    oracle.reset_tables(want_s, want_t, tables, waves=1, seed=77, tick=env.RESET_TICK_BASE + 1, env_offset=4096, mask=mask)
    assert np.array_equal(k2, want_s) and np.array_equal(t2, want_t)
    assert np.array_equal(k2[:, ~mask], st[:, ~mask])


# ------------------------------------------------------------------------------------------------
# reset
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obst", ["none", "default5", "bench8"])
def test_reset_bit_exact_vs_oracle_spec(torch, oracle, obst):
    from aquaticgymenv_amd import presets
    rows = {"none": presets.NONE, "default5": presets.DEFAULT5, "bench8": presets.BENCH8}[obst]
    n = 50000
    env = _make(torch, n, rows, seed=4242, env_offset=17)
    env.reset()
    torch.cuda.synchronize()
    k_state, k_time = _host_state(env)
    st = np.zeros((7, n), dtype=np.float32)
    tt = np.full(n, 5, dtype=np.int32)
    oracle.reset(st, tt, obstacles=rows, waves=1, seed=4242, tick=env.RESET_TICK_BASE, env_offset=17)
    assert np.array_equal(k_state, st)
    assert np.array_equal(k_time, tt)
    # masked reset touches only the masked worlds
    before = k_state.copy()
    mask = (np.arange(n) % 3 == 0)
    env.reset(mask=torch.as_tensor(mask).cuda())
    torch.cuda.synchronize()
    after, _ = _host_state(env)
    assert np.array_equal(after[:, ~mask], before[:, ~mask])
    assert not np.array_equal(after[:, mask], before[:, mask])
    oracle.reset(st, tt, obstacles=rows, waves=1, seed=4242, tick=env.RESET_TICK_BASE + 1, env_offset=17, mask=mask.astype(np.uint8))
    assert np.array_equal(after, st)


def test_reset_fixed_pose_and_distribution(torch):
    from aquaticgymenv_amd import presets
    z = load_reset()
    env = _make(torch, 64, presets.DEFAULT5, random_boat=False, random_goal=False)
    obs = env.reset().cpu().numpy()
    assert np.array_equal(obs, np.tile(z["reset_fixed"].astype(np.float32), (64, 1)))      # aqua.py:107,117
    # distribution of the rejection sampler against 6000 reset() calls of the reference (per marginal)
    from scipy import stats
    for ci, rows in ((0, presets.NONE), (1, presets.DEFAULT5), (3, presets.BENCH8)):
        ref = z["reset_cfg%d" % ci]
        env = _make(torch, 200000, rows, seed=ci + 1)
        env.reset()
        got = env.state[:, :200000].cpu().numpy().T
        for col in range(7):
            ks = stats.ks_2samp(ref[:, col], got[:, col])
            assert ks.pvalue > 1e-4, "reset marginal %d of cfg %d differs from the reference (p=%g)" % (col, ci, ks.pvalue)
        # every sampled pose satisfies the reference's acceptance predicates (aqua.py:104,112-114)
        x, y, gx, gy = got[:, 0], got[:, 1], got[:, 3], got[:, 4]
        assert np.all((x >= 2.5) & (x <= 97.5) & (y >= 2.5) & (y <= 97.5) & (gx >= 2.5) & (gx <= 97.5))
        assert np.all(np.hypot(gx - x, gy - y) > 5.0 - 1e-4)
        assert np.all(np.abs(got[:, 5:7]) <= 0.05) and np.all(np.abs(got[:, 2]) <= np.float32(np.pi))
        # ... the obstacle clauses among them (aqua.py:104,114): all five margins of tests/_placement.py, in float64 on
        # the float32 placement; a world is exempt only where the trace of the specification says its loop was exhausted
        from tests import _placement as P
        traced, a_goal, a_boat = P.placement_trace(ci + 1, np.arange(200000, dtype=np.uint64), env.RESET_TICK_BASE, rows)
        assert np.array_equal(traced.view(np.uint32), np.ascontiguousarray(got.T).view(np.uint32))
        worst = P.check_acceptance(got.T, rows, a_goal, a_boat, "reset(), cfg %d" % ci)
        print("cfg %d: worst acceptance margin goal %+.3g boat %+.3g" % ((ci,) + worst))
        margins = P.acceptance_margins(got.T, rows)
        assert np.all(margins[[1, 4]] >= P.MARGIN_BAR), "a goal or a boat was placed on an obstacle"


# ------------------------------------------------------------------------------------------------
# rollouts: per-step launches == fused launch == graph replay
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2], ids=["same_step", "next_step"])
@pytest.mark.parametrize("continuous", [False, True])
def test_fused_rollout_equals_stepwise(torch, continuous, mode):
    from aquaticgymenv_amd import presets
    n, T = 20000 + 13, 64
    outs = []
    for fused in (False, True):
        env = _make(torch, n, presets.BENCH8, continuous=continuous, seed=31, auto_reset=mode)
        env.reset()
        if continuous:
            g = torch.Generator(device="cuda").manual_seed(3)
            acts = torch.rand((T, 2, env.ld), device="cuda", generator=g) * 0.3 + 0.2
        else:
            g = torch.Generator(device="cuda").manual_seed(3)
            acts = torch.randint(0, 3, (T, env.ld), device="cuda", generator=g, dtype=torch.int64).to(torch.uint8)
        reward, term = env.rollout(T, actions=acts, fused=fused)
        torch.cuda.synchronize()
        outs.append((env.state.cpu().numpy().copy(), env.time.cpu().numpy().copy(), reward[:, :n].cpu().numpy().copy(),
                     term[:, :n].cpu().numpy().copy()))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    assert (outs[0][3] != 0).sum() > 0


@pytest.mark.parametrize("mode", [1, 2], ids=["same_step", "next_step"])
@pytest.mark.parametrize("obstacles", ["none", "bench8", "twenty"])
def test_fused_rollout_in_pieces_equals_stepwise(torch, obstacles, mode):
    """The fused rollout's restart hand-over (next-step: a wavefront of its own that re-seeds, posts two steps ahead of a
    world's next move, sequence numbers in LDS -- round 5) at its edges: launches of ONE and TWO steps (no step to post in,
    the prologue's post and the closing collect only), worlds that come INTO a launch marked done or restarted by the
    launch before, tables with a quick table (8 rows), without one (20 rows) and none at all, a batch that is not a
    multiple of the block -- T steps as launches of 1, 2, 1, 5, 3, 20 against 32 launches of the per-step kernel."""
    from aquaticgymenv_amd import presets
    rows = {"none": presets.NONE, "bench8": presets.BENCH8,
            "twenty": np.array([[5.0 + 4.5 * i, 8.0 + 4.2 * ((7 * i) % 20), i % 2, 2.0 + (i % 3), 1.5 + (i % 2)] for i in range(20)])}[obstacles]
    n, pieces = 5000 + 7, [1, 2, 1, 5, 3, 20]
    T = sum(pieces)
    g = torch.Generator(device="cuda").manual_seed(5)
    acts = torch.randint(0, 3, (T, (n + 63) // 64 * 64), device="cuda", generator=g, dtype=torch.int64).to(torch.uint8)
    ref = _make(torch, n, rows, seed=17, auto_reset=mode, env_offset=128)
    ref.reset()
    ref.time[:n] = torch.randint(0, 1001, (n,), device="cuda", generator=g).to(torch.int32)      # time-outs among the endings
    fused = _make(torch, n, rows, seed=17, auto_reset=mode, env_offset=128)
    fused.reset()
    fused.time.copy_(ref.time)
    want_r, want_c = ref.rollout(T, actions=acts, fused=False)
    t0, restarts = 0, 0
    for piece in pieces:
        r, c = fused.rollout(piece, actions=acts[t0:t0 + piece], fused=True)
        assert torch.equal(r[:, :n], want_r[t0:t0 + piece, :n]) and torch.equal(c[:, :n], want_c[t0:t0 + piece, :n]), \
            "the launch of steps [%d, %d) differs" % (t0, t0 + piece)
        restarts += int((c[:, :n] != 0).sum())
        t0 += piece
    assert torch.equal(fused.state, ref.state) and torch.equal(fused.time, ref.time) and fused._tick == ref._tick == T
    assert restarts > 100


@pytest.mark.parametrize("mode", [1, 2], ids=["same_step", "next_step"])
def test_fused_rollout_of_blocks_that_walk_several_tiles(torch, mode):
    """more than 2 048 x 256 worlds: the fused rollout's grid is capped, every block walks two or three tiles of 256 worlds
    one after the other (the mailbox's sequence numbers run on across the tiles) -- against the per-step kernels, actions
    sampled on the device"""
    from aquaticgymenv_amd import presets
    n, T = 2048 * 256 * 2 + 5000, 12
    outs = []
    for fused in (False, True):
        env = _make(torch, n, presets.BENCH8, seed=23, auto_reset=mode)
        env.reset()
        env.time[:n] = 995                                    # everybody times out inside the rollout: whole wavefronts restart
        reward, term = env.rollout(T, actions="random", fused=fused)
        torch.cuda.synchronize()
        outs.append((env.state.clone(), env.time.clone(), reward[:, :n].clone(), term[:, :n].clone()))
        del env
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    assert int((outs[0][3] != 0).sum()) >= n


@pytest.mark.parametrize("T", [1, 2, 16], ids=["one_step_graph", "two_step_graph", "sixteen_step_graph"])
@pytest.mark.parametrize("reset_mode", [1, 2], ids=["same_step", "next_step"])
def test_graph_replay_equals_eager(torch, reset_mode, T):
    """replays of a captured rollout draw fresh noise: the graph advances its device-resident tick base itself (its first
    launch copies the base, its last one stores base + T; a one-step graph keeps the tick kernel)"""
    from aquaticgymenv_amd import presets
    n = 30000
    res = []
    for mode in ("eager", "graph"):
        env = _make(torch, n, presets.BENCH8, seed=8, auto_reset=reset_mode)
        env.reset()
        if mode == "eager":
            for _ in range(3):
                reward, term = env.rollout(T, keep_all=False)
        else:
            graph = env.capture_rollout(T)
            for _ in range(3):
                reward, term = graph.launch()
        torch.cuda.synchronize()
        res.append((env.state.cpu().numpy().copy(), env.time.cpu().numpy().copy(), reward.cpu().numpy().copy(),
                    term.cpu().numpy().copy(), env._tick))
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)


def test_timed_graph_brackets_its_launches(torch):
    """capture_rollout(timing=True): event-record nodes at the head and the tail of the graph stamp every replay;
    the interval is the captured launches (bench.py's roofline.launch_us) and the results are the untimed graph's"""
    from aquaticgymenv_amd import presets
    n, T = 262144, 20
    res = []
    for timing in (False, True):
        env = _make(torch, n, presets.BENCH8, seed=8, auto_reset=2)
        env.reset()
        graph = env.capture_rollout(T, timing=timing)
        for _ in range(3):
            graph.launch()
        torch.cuda.synchronize()
        if timing:
            ms = graph.elapsed_ms()
            assert 0.02 < ms < 2.0, "20 steps of 262 144 worlds take ~0.1 ms on an MI355X, got %r ms" % ms
        res.append((env.state.cpu().numpy().copy(), env.time.cpu().numpy().copy()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


# ------------------------------------------------------------------------------------------------
# layout / shapes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 1000, 4099])
def test_ragged_sizes_and_done_bits(torch, oracle, n):
    from aquaticgymenv_amd import presets
    env = _make(torch, n, presets.DIFFICULT6, seed=n)
    env.reset()
    env.time[:n] = 1000          # every world ends by the time limit unless it collides
    guard_state = env.state.clone()
    state0, time0 = _host_state(env)
    a = (np.arange(n) % 3).astype(np.uint8)
    tick = env._tick
    obs, reward, term = env.step(torch.as_tensor(a).cuda())
    torch.cuda.synchronize()
    term_h = term.cpu().numpy()
    assert np.all(term_h != 0)
    assert np.array_equal(env.done_mask().cpu().numpy(), np.ones(n, dtype=np.uint8))
    # padding columns [n, ld) are never written
    assert torch.equal(env.state[:, n:], guard_state[:, n:])
    words = env.done_bits.cpu().numpy().view(np.uint64)
    full, rem = divmod(n, 64)
    assert np.all(words[:full] == np.uint64(0xFFFFFFFFFFFFFFFF))
    if rem:
        assert words[full] == np.uint64((1 << rem) - 1)
    _compare_with_oracle(torch, oracle, env, state0, time0, a, reward.cpu().numpy(), term_h, tick)


def test_config5_two_million_worlds_as_eight_sequential_shards(torch, oracle):
    """BASELINE.json configs[4] as far as ONE GPU allows: 2 097 152 worlds, discrete actions, 8 obstacles, range-partitioned
    into 8 shards of 262 144 (sharded.shard_range) that are stepped one after the other with their global env_offset.
    Each shard reproduces its slice of the single 2 M-world run bit for bit (state, time markers, reward, term, ballot
    words); its ballot words go through DoneMaskExchange (side stream, double buffer) and come back unchanged; a window of
    each shard is checked against the float64 oracle tick by tick.  (What is NOT measured here: 8 GPUs.  The 1 -> 8 curve
    is the driver's; the RCCL branch itself runs in tests/test_00_bench_child.py.)"""
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.sharded import DoneMaskExchange, shard_range, unpack_done_words
    total, parts, T, seed = 2097152, 8, 8, 505
    whole = _make(torch, total, presets.BENCH8, seed=seed, auto_reset="next_step")
    whole.reset()
    hist = torch.zeros((T, total // 64), dtype=torch.int64, device="cuda:0")
    w_rew, w_term = whole.rollout(T, keep_all=True, done_history=hist)           # actions sampled on the device (stream 4)
    torch.cuda.synchronize()
    assert int((w_term != 0).sum()) > total // 20
    words = 262144 // 64
    exchange = DoneMaskExchange(T, words, "cuda:0")
    rng = np.random.RandomState(1)
    for r in range(parts):
        off, cnt = shard_range(total, parts, r)
        assert (off, cnt) == (r * 262144, 262144)
        shard = _make(torch, cnt, presets.BENCH8, seed=seed, auto_reset="next_step", env_offset=off)
        shard.reset()
        h = torch.zeros((T, words), dtype=torch.int64, device="cuda:0")
        rew, term = shard.rollout(T, keep_all=True, done_history=h)
        slot = exchange.gather_async(h, source_id=r & 1)
        exchange.wait(slot)
        torch.cuda.synchronize()
        assert torch.equal(shard.state[:, :cnt], whole.state[:, off:off + cnt]) and torch.equal(shard.time[:cnt], whole.time[off:off + cnt])
        assert torch.equal(rew[:, :cnt], w_rew[:, off:off + cnt]) and torch.equal(term[:, :cnt], w_term[:, off:off + cnt])
        assert torch.equal(h, hist[:, off // 64:(off + cnt) // 64])
        assert torch.equal(exchange.gathered[slot][0], h)
        flags = unpack_done_words(h[T - 1].cpu().numpy(), cnt)
        assert np.array_equal(flags, (term[T - 1, :cnt] != 0).cpu().numpy().astype(np.uint8))
        # a window of this shard against the oracle, teacher-forced per tick, with its GLOBAL indices
        w0 = off + int(rng.randint(0, cnt - 1024))
        finished = _rollout_against_oracle(torch, oracle, presets.BENCH8, 1024, T, False, 2, w0, seed=seed)
        assert finished > 0
        del shard
    exchange.finish()


def test_shard_invariance(torch):
    """range-partitioned shards (env_offset) reproduce the single-device batch bit for bit."""
    from aquaticgymenv_amd import presets
    n, parts, T = 16384, 4, 12
    whole = _make(torch, n, presets.BENCH8, seed=2024, auto_reset=2)
    whole.reset()
    whole.rollout(T, keep_all=False)
    torch.cuda.synchronize()
    ref = whole.state[:, :n].cpu().numpy()
    per = n // parts
    for p in range(parts):
        shard = _make(torch, per, presets.BENCH8, seed=2024, auto_reset=2, env_offset=p * per)
        shard.reset()
        shard.rollout(T, keep_all=False)
        torch.cuda.synchronize()
        assert np.array_equal(shard.state[:, :per].cpu().numpy(), ref[:, p * per:(p + 1) * per])


def test_next_step_restart_soak_against_oracle_statistics(torch, oracle):
    """3 000 steps of the benchmark configuration (262 144 worlds, next-step restart, graph replays of 100 steps with
    sampled actions): no world is ever lost (every marker is resolved within a step), the state stays inside its
    invariants, and the episode statistics (terminations per world-step by kind) equal those of a free-running
    oracle rollout of the same specification within sampling error."""
    from aquaticgymenv_amd import presets
    n, steps = 262144, 3000
    env = _make(torch, n, presets.BENCH8, seed=1001, auto_reset="next_step")
    env.reset()
    graph = env.capture_rollout(100, actions="random", keep_all=True)
    counts = np.zeros(4, dtype=np.int64)
    zero_reward_nonterm = 0
    for rep in range(steps // 100):
        reward, term = graph.launch()
        t = term[:, :n]
        counts += torch.bincount(t.reshape(-1).to(torch.int64), minlength=4).cpu().numpy()
    torch.cuda.synchronize()
    tm = env.time[:n]
    st = env.state[:, :n]
    # markers: only the two that can be pending between launches (finished at the last tick / restarted at it)
    last = env._tick - 1
    neg = tm[tm < 0]
    assert bool(((neg == -1 - (last & 1)) | (neg == -3 - (last & 1))).all())
    assert int(tm.max()) <= 1000
    assert float(st[2].min()) >= -np.float32(np.pi) - 1e-6 and float(st[2].max()) < np.float32(np.pi) + 1e-6
    assert float(st[5:7].abs().max()) <= 0.05 + 1e-9 and bool(torch.isfinite(st).all())
    assert float(st[0:2].min()) >= 2.5 - 1.0 and float(st[0:2].max()) <= 97.5 + 1.0
    # free-running oracle, same specification, smaller batch
    m, osteps = 32768, 600
    so = np.zeros((7, m), dtype=np.float32)
    to = np.zeros(m, dtype=np.int32)
    oracle.reset(so, to, obstacles=presets.BENCH8, waves=1, seed=77, tick=1 << 40)
    ep, _, _, oc = oracle.rollout_f32(so, to, osteps, obstacles=presets.BENCH8, waves=1, seed=77, tick0=0, auto_reset=2)
    rate_k = counts[1:] / float(n * steps)
    rate_o = np.asarray(oc, dtype=np.float64) / float(m * osteps)
    for kk in range(3):
        sigma = np.sqrt(rate_o[kk] / (m * osteps) + rate_k[kk] / (n * steps))
        # the first episodes of a run are not yet in the stationary mix: allow 2 % relative on top of 5 sigma
        assert abs(rate_k[kk] - rate_o[kk]) <= 5 * sigma + 0.02 * rate_o[kk], (kk, rate_k, rate_o)
    assert 0.015 < rate_k.sum() < 0.022          # mean episode ~54 steps (+1 restart step) with 8 obstacles


def test_obs_is_a_view_and_invariants_at_full_size(torch):
    from aquaticgymenv_amd import presets
    n = 262144
    env = _make(torch, n, presets.BENCH8, seed=5, auto_reset=True)
    obs0 = env.reset()
    assert obs0.data_ptr() == env.state.data_ptr() and obs0.shape == (n, 5)
    ep = 0
    for _ in range(50):
        obs, reward, term = env.step(sample_actions=True)
        ep += int((term != 0).sum())
    torch.cuda.synchronize()
    st = env.state[:, :n]
    assert float(st[2].min()) >= -np.float32(np.pi) - 1e-6 and float(st[2].max()) < np.float32(np.pi) + 1e-6
    assert float(st[5:7].abs().max()) <= 0.05 + 1e-9
    assert int(env.time[:n].max()) <= 50 and int(env.time[:n].min()) >= 0
    # worlds are inside the border after auto-reset or still alive
    assert float(st[0:2].min()) >= 2.5 - 1.0 and float(st[0:2].max()) <= 97.5 + 1.0
    assert ep > 0.3 * n          # random policy: mean episode ~55 steps with 8 obstacles
    # determinism: same seed, same inputs -> same bits
    env2 = _make(torch, n, presets.BENCH8, seed=5, auto_reset=True)
    env2.reset()
    for _ in range(50):
        env2.step(sample_actions=True)
    assert torch.equal(env.state, env2.state) and torch.equal(env.time, env2.time)


# ------------------------------------------------------------------------------------------------
# on-device bearing policy (main/testing/test_optimal.py:8-28)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2], ids=["no_reset", "next_step"])
def test_bearing_policy_steps_match_oracle(torch, oracle, mode):
    from aquaticgymenv_amd import presets
    n = 30000
    env = _make(torch, n, presets.DEFAULT5, seed=314, auto_reset=mode)
    env.reset()
    for it in range(30):
        s0, t0 = _host_state(env)
        tick = env._tick
        obs, reward, term = env.step(policy="bearing")
        torch.cuda.synchronize()
        act, edge = _bearing_np(s0.astype(np.float64))
        safe = edge > 1e-5                       # float32 vs float64 may disagree on the action only at the threshold
        st = np.ascontiguousarray(s0.copy())
        tt = t0.copy()
        oracle.rollout_f32(st, tt, 1, obstacles=env.obstacle_rows, actions=act.reshape(1, n).copy(), seed=env.seed,
                           tick0=tick, auto_reset=mode)
        k_state, k_time = _host_state(env)
        moved = safe & (t0 >= 0)
        assert (~safe).sum() < 20
        assert np.max(np.abs(k_state[0:2, moved] - st[0:2, moved])) <= TOL
        assert np.max(angle_diff(k_state[2, moved], st[2, moved])) <= TOL
        assert np.array_equal(k_time[safe], tt[safe])


def test_bearing_policy_reproduces_the_reference_success_rate(torch):
    """behavioural check of the whole path (reset distribution, dynamics, termination cascade): one episode per
    world under the bearing policy against 1500 episodes of the reference env under the same policy
    (tests/golden/policy_golden.npz): 91.4 % success without obstacles, 59.3 % with the default five."""
    import os
    from tests._golden import GOLDEN
    from aquaticgymenv_amd import presets
    z = np.load(os.path.join(GOLDEN, "policy_golden.npz"))
    for ci, rows in ((0, presets.NONE), (1, presets.DEFAULT5)):
        ref_term, ref_steps = z["policy_cfg%d_term" % ci], z["policy_cfg%d_steps" % ci]
        n = 65536
        env = _make(torch, n, rows, seed=2718 + ci, auto_reset=False)
        env.reset()
        first = torch.zeros(n, dtype=torch.uint8, device="cuda")
        steps = torch.zeros(n, dtype=torch.int32, device="cuda")
        for chunk in range(11):
            reward, term = env.rollout(100, actions="bearing", keep_all=True)
            t = term[:, :n]
            hit = t != 0
            any_hit = hit.any(dim=0)
            idx = hit.to(torch.uint8).argmax(dim=0)
            code = t.gather(0, idx.unsqueeze(0)).squeeze(0)
            new = (first == 0) & any_hit
            first = torch.where(new, code, first)
            steps = torch.where(new, (chunk * 100 + idx + 1).to(torch.int32), steps)
        assert int((first == 0).sum()) == 0          # every episode ended (time limit 1000 at the latest)
        first, steps = first.cpu().numpy(), steps.cpu().numpy()
        for code in (1, 2, 3):
            p_ref, p_gpu = np.mean(ref_term == code), np.mean(first == code)
            sigma = np.sqrt(max(p_ref * (1 - p_ref), 1e-4) / ref_term.shape[0])
            assert abs(p_ref - p_gpu) < 4 * sigma + 0.004, "cfg %d code %d: reference %.4f batched %.4f" % (ci, code, p_ref, p_gpu)
        sem = ref_steps.std() / np.sqrt(ref_steps.shape[0])
        assert abs(ref_steps.mean() - steps.mean()) < 4 * sem + 1.0


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["no_reset", "same_step", "next_step"])
def test_normalised_observation_epilogue(torch, mode):
    """fused epilogue == main/impl/utils.py:15-33 (AquaStateNormalizer): obs / (high - low), angle + 0.5 --
    also for the worlds re-seeded inside the launch."""
    from aquaticgymenv_amd import presets
    n = 5000
    env = _make(torch, n, presets.BENCH8, seed=55, auto_reset=mode, normalized_obs=True)
    env.reset()
    scale = torch.tensor([100.0, 100.0, 2 * np.pi, 100.0, 100.0], device="cuda", dtype=torch.float64)
    shift = torch.tensor([0.0, 0.0, 0.5, 0.0, 0.0], device="cuda", dtype=torch.float64)
    for it in range(25):
        obs, reward, term = env.step(sample_actions=True)
        want = obs.to(torch.float64) / scale + shift
        assert float((env.obs_norm.to(torch.float64) - want).abs().max()) < 2e-7
    reward, term = env.rollout(10, keep_all=False)
    want = env.obs.to(torch.float64) / scale + shift
    assert float((env.obs_norm.to(torch.float64) - want).abs().max()) < 2e-7
    plain = _make(torch, n, presets.BENCH8, seed=55, auto_reset=mode)
    with pytest.raises(RuntimeError):
        plain.obs_norm


@pytest.mark.parametrize("tag,obstacles", [("no_obs", False), ("with_obs", True)])
def test_trained_dqn_policies_reach_the_published_success_rates(torch, tag, obstacles):
    """The reference's only published numbers (Report p.4, example_policies/test_results.pickle: 93.8 % success
    without obstacles with checkpoint 30, 66.7 % with the default obstacles and checkpoint 32, 1000 runs each)
    replayed on the batched path: Keras weights read without TensorFlow (tests/golden/dqn_policies.npz), greedy
    5-64-64-3 MLP on the device fed by the fused AquaStateNormalizer epilogue, one episode per world."""
    import os
    from tests._golden import GOLDEN
    from aquaticgymenv_amd.tf_import import GreedyQPolicy
    from aquaticgymenv_amd.batched import BatchedAqua
    z = np.load(os.path.join(GOLDEN, "dqn_policies.npz"))
    layers = [(z["%s_kernel%d" % (tag, i)], z["%s_bias%d" % (tag, i)]) for i in range(3)]
    n = 16384
    env = BatchedAqua(n, obstacles=obstacles, seed=9001, auto_reset=False, normalized_obs=True, device="cuda:0")
    env.reset()
    scale = torch.tensor([100.0, 100.0, 2 * np.pi, 100.0, 100.0], device="cuda")
    shift = torch.tensor([0.0, 0.0, 0.5, 0.0, 0.0], device="cuda")
    policy = GreedyQPolicy(layers, "cuda:0")
    first = torch.zeros(n, dtype=torch.uint8, device="cuda")
    total = torch.zeros(n, dtype=torch.float32, device="cuda")
    obs_norm = env.obs_norm                            # reset() and every step write it (AquaStateNormalizer)
    assert float((obs_norm - (env.obs / scale + shift)).abs().max()) < 1e-6
    for step in range(1001):
        action = policy(obs_norm)
        obs, reward, term = env.step(action)
        alive = first == 0
        total += torch.where(alive, reward, torch.zeros_like(reward))
        first = torch.where(alive, term, first)
        obs_norm = env.obs_norm
        if step % 100 == 99 and int((first == 0).sum()) == 0:
            break
    assert int((first == 0).sum()) == 0
    success = float((first == 3).float().mean())
    reward_mean = float(total.mean())
    pub_s, pub_r = z["%s_published_success" % tag], z["%s_published_reward" % tag]
    sigma = np.sqrt(pub_s.mean() * (1 - pub_s.mean()) / pub_s.shape[0])
    assert abs(success - pub_s.mean()) < 4 * sigma + 0.01, "success %.4f vs published %.4f" % (success, pub_s.mean())
    sem = pub_r.std() / np.sqrt(pub_r.shape[0])
    assert abs(reward_mean - pub_r.mean()) < 4 * sem + 0.5, "mean reward %.3f vs published %.3f" % (reward_mean, pub_r.mean())


@pytest.mark.parametrize("continuous", [False, True])
def test_replay_ring_records_the_transitions(torch, continuous):
    """the experience buffer of main/impl/dqn.py:174 on the device: (s, a, r, s', d) of every world and step,
    in consecutive slots, wrapping; restarting worlds (next-step mode) are marked as no experience."""
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.replay import ReplayRing
    from aquaticgymenv_amd.batched import BatchedAqua
    n, steps = 3000 + 17, 7
    env = BatchedAqua(n, obstacles=presets.BENCH8, seed=77, auto_reset="next_step", normalized_obs=True,
                      continuous=continuous, device="cuda:0")
    env.reset()
    for _ in range(40):
        env.step(sample_actions=True)                      # some worlds are restarting by now
    cap = 5 * n + 100                                      # 7 steps wrap around once
    ring = ReplayRing(env, cap)
    g = torch.Generator(device="cuda").manual_seed(3)
    expect = []
    for t in range(steps):
        if continuous:
            act = 0.2 + 0.3 * torch.rand((2, env.ld), device="cuda", generator=g)
        else:
            act = torch.randint(0, 3, (env.ld,), device="cuda", generator=g, dtype=torch.int64).to(torch.uint8)
        s = env.obs_norm.clone()
        live = ((env.time[:n] >= 0) | (env.time[:n] <= -3)).clone()
        ring.before_step(act)
        obs, reward, term = env.step(act, soa=True) if continuous else env.step(act[:n])
        ring.after_step()
        expect.append((s, act[:, :n].t().clone() if continuous else act[:n].clone(), reward.clone(), env.obs_norm.clone(),
                       term.clone(), live))
    torch.cuda.synchronize()
    assert ring.size == cap and ring.cursor == (steps * n) % cap
    for t in range(steps - 5, steps):                     # the last five steps are still in the ring
        slots = (torch.arange(n, device="cuda") + t * n) % cap
        s, a, r, s2, d, live = expect[t]
        assert torch.equal(ring.s[:, slots].t(), s) and torch.equal(ring.s2[:, slots].t(), s2)
        assert torch.equal(ring.a[:, slots].t() if continuous else ring.a[slots], a)
        assert torch.equal(ring.r[slots], r) and torch.equal(ring.d[slots], d)
        assert torch.equal(ring.ok[slots] != 0, live)
        assert int((~live).sum()) > 0 and bool(((r == 0) & (d == 0))[~live].all())
    bs, ba, br, bs2, bd = ring.sample(512, generator=g)
    assert bs.shape == (512, 5) and bs2.shape == (512, 5) and br.shape == (512,) and bd.dtype == torch.bool
    assert ba.shape == ((512, 2) if continuous else (512,))


def test_done_mask_exchange_on_device(torch):
    """the N > 1 plumbing on one GPU (world size 1): side stream, event ordering, double buffer; the gathered
    block equals the ballot words the kernels wrote and those equal term != 0."""
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.sharded import DoneMaskExchange, unpack_done_words
    n, T = 10000, 20
    env = _make(torch, n, presets.BENCH8, seed=12, auto_reset=2)
    env.reset()
    words = env.ld // 64
    ex = DoneMaskExchange(T, words, env.device)
    hist = [torch.zeros((T, words), dtype=torch.int64, device=env.device) for _ in range(2)]
    for c in range(4):
        reward, term = env.rollout(T, keep_all=True, done_history=hist[c & 1])
        slot = ex.gather_async(hist[c & 1])
        ex.wait(slot)
        torch.cuda.synchronize()
        g = ex.gathered[slot][0].cpu().numpy()
        t = term[:, :n].cpu().numpy()
        for s in range(T):
            assert np.array_equal(unpack_done_words(g[s], n), (t[s] != 0).astype(np.uint8))
    ex.finish()


# ------------------------------------------------------------------------------------------------
# the Gym-shaped facade
# ------------------------------------------------------------------------------------------------
def test_gym_facade_single_env_types_and_hand_rows(torch, golden):
    import gym_aqua
    env = gym_aqua.make("AquaEnv-v1", waves=False, seed=3)
    assert env.action_space.n == 3 and env.observation_space.shape == (5,)
    assert np.allclose(env.observation_space.high, [100, 100, np.pi, 100, 100])
    obs = env.reset()
    assert isinstance(obs, np.ndarray) and obs.dtype == np.float64 and obs.shape == (5,)
    h0 = golden.n - golden.n_hand
    z = golden.z
    for i in range(h0, golden.n):
        if z["cfg"][i] != 6:
            continue
        env.core.set_state(z["state_in"][i:i + 1].astype(np.float32), z["time_in"][i:i + 1])
        obs, rew, done, info = env.step(int(z["action_i"][i]))
        code = 1 if info["Termination.collided"] else 2 if info["Termination.time"] else \
            3 if info["Termination.success"] else 0
        assert code == z["term"][i] and done == (code != 0) and isinstance(done, bool)
        assert isinstance(rew, int) == bool(z["reward_is_int"][i])
        assert abs(rew - z["reward"][i]) <= TOL
        assert np.max(np.abs(obs[0:2] - z["pose"][i, 0:2])) <= TOL and angle_diff(obs[2], z["pose"][i, 2]) <= TOL
    with pytest.raises(IndexError):
        env.step(3)
    with pytest.raises(NotImplementedError):
        env.render()
    env.close()


def test_gym_facade_batched_and_continuous(torch, capsys):
    import gym_aqua
    env = gym_aqua.make("AquaContinuousEnv-v2", num_envs=4096, seed=11)
    obs = env.reset()
    assert tuple(obs.shape) == (4096, 5) and obs.is_cuda
    a = torch.rand((4096, 2), device="cuda") * 0.3 + 0.2
    obs, reward, done, info = env.step(a)
    assert done.dtype == torch.bool and reward.shape == (4096,)
    assert torch.equal(info["Termination.collided"] | info["Termination.time"] | info["Termination.success"], done)
    single = gym_aqua.make("AquaContinuousEnv-v0", seed=1)
    single.reset()
    single.step(np.array([0.9, 0.1]))           # out of range: the reference prints and clips (aqua.py:145-150)
    assert "out of bounds" in capsys.readouterr().out


def test_rollout_loop_shape_of_the_reference(torch):
    """main/testing/__init__.py:17-36: reset, then step until done, with the hand-coded bearing policy of
    main/testing/test_optimal.py:8-28 -- it reaches the goal in an obstacle-free world."""
    import gym_aqua
    env = gym_aqua.make("AquaEnv-v0", obstacles=False, seed=21)
    wins = 0
    for ep in range(5):
        state = env.reset()
        for step in range(1, 1200):
            ang = lambda v: (v + 2 * np.pi) % (2 * np.pi)
            boat_angle = ang(state[2] + np.pi / 2)
            goal_angle = ang(np.arctan2(state[4] - state[1], state[3] - state[0]))
            diff = goal_angle - boat_angle
            action = (0 if diff > 0 else 1) if abs(diff) > 8 / 180 * np.pi else 2
            state, reward, done, info = env.step(action)
            if done:
                break
        wins += int(info["Termination.success"])
    assert wins >= 4


# ------------------------------------------------------------------------------------------------
# checkpoint / resume
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["next_step", "same_step", False])
def test_checkpoint_resumes_bit_for_bit(torch, mode):
    """state_dict() after 30 steps, 50 more steps -- against a FRESH batch that loads the checkpoint and runs the same 50
    steps (eagerly, and as a captured graph): rewards, codes, state, time markers and ballot words equal bit for bit"""
    from aquaticgymenv_amd import presets
    n = 5000
    env = _make(torch, n, presets.BENCH8, seed=11, auto_reset=mode)
    env.reset()
    g = torch.Generator(device="cuda:0").manual_seed(5)
    acts = torch.randint(0, 3, (80, env.ld), device="cuda:0", generator=g, dtype=torch.int64).to(torch.uint8)
    env.rollout(30, actions=acts[:30], keep_all=False)
    ckpt = env.state_dict()
    assert ckpt["tick"] == 30 and ckpt["state"].device.type == "cpu"
    rew1, term1 = env.rollout(50, actions=acts[30:], keep_all=True)
    want = (rew1[:, :n].clone(), term1[:, :n].clone(), env.state[:, :n].clone(), env.time[:n].clone(), env.done_bits.clone())
    for graph in (False, True):
        other = _make(torch, n, presets.BENCH8, seed=11, auto_reset=mode)
        other.reset()
        other.rollout(3, actions=acts[:3], keep_all=False)             # some other history first
        other.load_state_dict(ckpt)
        if graph:
            gr = other.capture_rollout(50, actions=acts[30:], keep_all=True)
            rew2, term2 = gr.launch()
        else:
            rew2, term2 = other.rollout(50, actions=acts[30:], keep_all=True)
        torch.cuda.synchronize()
        got = (rew2[:, :n], term2[:, :n], other.state[:, :n], other.time[:n], other.done_bits)   # (columns past n: padding)
        for name, a, b in zip(("reward", "term", "state", "time", "done_bits"), want, got):
            assert torch.equal(a, b), "%s differs after the checkpoint was restored (graph=%s)" % (name, graph)
        assert other._tick == 80
    stranger = _make(torch, n, presets.BENCH8, seed=12, auto_reset=mode)
    with pytest.raises(ValueError):
        stranger.load_state_dict(ckpt)
    with pytest.raises(ValueError):
        _make(torch, n, presets.NONE, seed=11, auto_reset=mode).load_state_dict(ckpt)


@pytest.mark.parametrize("mode", ["next_step", "same_step", False])
def test_snapshot_taken_back_on_the_device(torch, mode):
    """snapshot() after 30 steps, a 20-step look-ahead (a captured graph), restore(): the 50 steps that follow equal the
    50 steps of a batch that never looked ahead -- eagerly and through the graph captured BEFORE the snapshot, bit for bit"""
    from aquaticgymenv_amd import presets
    n = 5000
    g = torch.Generator(device="cuda:0").manual_seed(5)
    acts = torch.randint(0, 3, (80, 5120), device="cuda:0", generator=g, dtype=torch.int64).to(torch.uint8)
    plain = _make(torch, n, presets.BENCH8, seed=11, auto_reset=mode)
    plain.reset()
    plain.rollout(30, actions=acts[:30, :plain.ld].contiguous(), keep_all=False)
    rew1, term1 = plain.rollout(50, actions=acts[30:, :plain.ld].contiguous(), keep_all=True)
    want = (rew1[:, :n].clone(), term1[:, :n].clone(), plain.state[:, :n].clone(), plain.time[:n].clone(), plain.done_bits.clone())
    for graph in (False, True):
        env = _make(torch, n, presets.BENCH8, seed=11, auto_reset=mode)
        env.reset()
        a = acts[:, :env.ld].contiguous()
        ahead = env.capture_rollout(20, actions=a[:20], keep_all=False)
        gr = env.capture_rollout(50, actions=a[30:], keep_all=True) if graph else None
        env.rollout(30, actions=a[:30], keep_all=False)
        snap = env.snapshot()
        assert snap["state"].device.type == "cuda" and snap["_tick"] == 30
        ahead.launch()
        ahead.launch()
        assert env._tick == 70
        env.restore(snap)
        assert env._tick == 30
        rew2, term2 = gr.launch() if graph else env.rollout(50, actions=a[30:], keep_all=True)
        torch.cuda.synchronize()
        got = (rew2[:, :n], term2[:, :n], env.state[:, :n], env.time[:n], env.done_bits)
        for name, x, y in zip(("reward", "term", "state", "time", "done_bits"), want, got):
            assert torch.equal(x, y), "%s differs after the look-ahead was taken back (graph=%s)" % (name, graph)
        assert env._tick == 80


def test_clipped_action_counter(torch):
    """aqua.py:145-150 prints and clips a continuous action outside [0.2, 0.5]; the batched path clips in the kernel and --
    with count_clipped=True -- counts the worlds it clipped for"""
    from aquaticgymenv_amd import presets
    n = 1000
    env = _make(torch, n, presets.NONE, continuous=True, seed=3, count_clipped=True)
    env.reset()
    a = torch.full((n, 2), 0.3, device="cuda:0")
    a[10, 0] = 0.1; a[20, 1] = 0.9; a[30] = torch.tensor([0.0, 1.0], device="cuda:0")      # three worlds, four thrusts
    env.step(a)
    assert int(env.clipped_actions) == 3
    soa = torch.full((2, env.ld), 0.5, device="cuda:0")
    soa[0, 5] = 0.5001
    env.step(soa, soa=True)
    assert int(env.clipped_actions) == 4
    acts = torch.full((6, 2, env.ld), 0.2, device="cuda:0")
    acts[2, 1, 7] = 0.19; acts[4, 0, 7] = 0.6; acts[5, 0, env.ld - 1] = 9.0                 # (the last one is padding: not a world)
    env.rollout(6, actions=acts)
    assert int(env.clipped_actions) == 6
    # replays count too, each with the buffer's content at THAT launch; capturing / preparing counts nothing by itself
    graph = env.capture_rollout(6, actions=acts)
    prepared = env.prepare_rollout(6, actions=acts)
    assert int(env.clipped_actions) == 6
    graph.launch()
    assert int(env.clipped_actions) == 8
    acts[0, 0, 3] = 0.55                                                                     # one more world, from now on
    graph.launch()
    prepared.launch()
    assert int(env.clipped_actions) == 8 + 3 + 3
    # ... and the counter is part of a checkpoint
    ckpt = env.state_dict()
    assert ckpt["clipped_actions"] == 14
    other = _make(torch, n, presets.NONE, continuous=True, seed=3, count_clipped=True)
    other.load_state_dict(ckpt)
    assert int(other.clipped_actions) == 14
    assert _make(torch, n, presets.NONE, continuous=True).clipped_actions is None


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["no_restart", "same_step", "next_step"])
def test_captured_step_equals_step(torch, mode):
    """BatchedAqua.capture_step: ONE step as a HIP graph that re-reads the caller's action buffer at every replay (a policy
    writes into it in between) == step() with the same actions, bit for bit -- shared table and per-world tables of 8 and 20
    rows, discrete and continuous, Philox noise (the graph advances the device's tick base), the clipped-action counter;
    a buffer the graph could not re-read is refused."""
    from aquaticgymenv_amd import presets
    n, T = 3000 + 5, 12
    g = torch.Generator(device="cuda").manual_seed(4)
    rng = np.random.RandomState(6)
    for obstacles, continuous in ((presets.BENCH8, False), (presets.BENCH8, True), (_random_tables(rng, n, 8), False), (_random_tables(rng, n, 20), False)):
        a = _make(torch, n, obstacles, continuous=continuous, seed=12, auto_reset=mode, count_clipped=continuous)
        b = _make(torch, n, obstacles, continuous=continuous, seed=12, auto_reset=mode, count_clipped=continuous)
        a.reset(); b.reset()
        if continuous:
            seq = torch.rand((T, 2, a.ld), device="cuda", generator=g) * 0.34 + 0.18          # some thrusts outside [0.2, 0.5]
            buf = torch.zeros((2, a.ld), dtype=torch.float32, device="cuda")
        else:
            seq = torch.randint(0, 3, (T, n), device="cuda", generator=g, dtype=torch.int64).to(torch.int32)
            buf = torch.zeros(n, dtype=torch.int32, device="cuda")
        graph = b.capture_step(buf, soa=continuous)
        for t in range(T):
            _, r1, c1 = a.step(seq[t], soa=continuous)
            buf.copy_(seq[t])
            r2, c2 = graph.launch()
            assert torch.equal(r1, r2[:n]) and torch.equal(c1, c2[:n]), "step %d differs" % t
        assert torch.equal(a.state, b.state) and torch.equal(a.time, b.time) and a._tick == b._tick == T
        if continuous:
            assert int(a.clipped_actions) == int(b.clipped_actions) > 0
    env = _make(torch, n, presets.BENCH8, seed=1)
    with pytest.raises(ValueError):
        env.capture_step(torch.zeros(n, dtype=torch.int32))                     # a host tensor
    with pytest.raises(ValueError):
        env.capture_step(torch.zeros(2 * n, dtype=torch.int32, device="cuda")[::2])       # not contiguous: step() would copy it
    cont = _make(torch, n, presets.BENCH8, continuous=True, seed=1)
    with pytest.raises(ValueError):
        cont.capture_step(torch.zeros((n, 2), device="cuda"))                   # [N][2] is staged by step(): soa only
