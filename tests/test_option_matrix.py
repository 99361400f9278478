"""Every runtime option in every kernel family, against the float64 oracle.

tests/test_dispatch_matrix.py and tests/test_knife_edges.py pin every kernel instantiation, all with the same runtime
arguments (waves = 1, random boat and goal, the 1000-step limit, Philox noise, no obs_norm buffer).  The cells here
(tests/_options.py: FAMILIES x OPTIONS) change those arguments in one representative of every site that carries its own
copy of their plumbing: waves 0 / 2, a fixed boat and/or goal for the restarts inside the launches, a time limit of 5,
injected noise in a buffer with noise_ld > ld, and the normalised-observation epilogue.

Each cell starts from the oracle's all-random reset written with set_state(), is teacher-forced against
_options.oracle_tick() through a chain of step() calls (bars of tests/_parity.py: codes, time markers, done bits and
re-seeded states bit-exact; pose and reward within 1e-5; wave within 1e-7; goal rows equal), and every other entry point
of the family, run from the same start, must give the chain's per-step outputs and final state bit for bit.  Graphs are
captured after the options are set and replayed twice.  With `norm`, obs_norm_buf must equal bit for bit what
aqua_obs_norm_f32 makes of the state the kernel left, after every step and every entry point.  What a cell must exercise
(re-seeded and live worlds per tick, time-outs) is asserted from the oracle's outputs before the kernel's are looked at;
tests/test_option_construct.py checks the same on the CPU.
"""
import ctypes

import numpy as np
import pytest

from tests import _dispatch as D
from tests import _options as O
from tests._parity import _host_state
from tests.test_dispatch_matrix import T, SEED, _device_actions, _unpack_done, _check

pytestmark = pytest.mark.gpu

GRAPH_ENTRIES = ("graph", "graph_fused", "graph_step")


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _make(torch, n, obst, continuous, mode, env_offset, waves, random_boat, random_goal, time_limit, norm):
    from aquaticgymenv_amd.batched import BatchedAqua
    env = BatchedAqua(n, obstacles=obst, waves=waves, random_boat=random_boat, random_goal=random_goal,
                      continuous=continuous, seed=SEED, auto_reset=mode, env_offset=env_offset, normalized_obs=norm,
                      device="cuda:0")
    # the time limit is a field of the public C ABI (AquaParams.time_limit, include/aqua_hip.h) without a Python
    # keyword: it is set on the parameter block every launch and capture reads, before the first of them
    env.params.time_limit = time_limit
    return env


def _norm_failures(torch, env, what):
    """obs_norm_buf against aqua_obs_norm_f32 run on the state as it is (bit for bit, the guard columns n .. ld
    included) and against the float64 expression (2e-7)"""
    from aquaticgymenv_amd import _capi
    n = env.num_envs
    scratch = torch.full((5, env.ld), O.NORM_GUARD, dtype=torch.float32, device=env.device)
    _capi.check(_capi.lib.aqua_obs_norm_f32(env.state.data_ptr(), env.ld, n, None, scratch.data_ptr(), env._stream()),
                "aqua_obs_norm_f32")
    torch.cuda.synchronize()
    got, want = env.obs_norm_buf.cpu().numpy(), scratch.cpu().numpy()
    assert np.max(np.abs(want[:, :n].astype(np.float64) - O.norm_expected(env.state[:, :n].cpu().numpy()))) <= 2e-7
    assert np.all(got[:, n:] == np.float32(O.NORM_GUARD)), "%s: obs_norm written beyond the batch" % what
    bad = np.flatnonzero(np.any(got.view(np.uint32) != want.view(np.uint32), axis=0))
    assert bad.size == 0, "%s: obs_norm differs from the state's in %d worlds (first %s): stale or wrong" % (
        what, bad.size, bad[:6])
    assert np.max(np.abs(got[:, :n].astype(np.float64) - O.norm_expected(env.state[:, :n].cpu().numpy()))) <= 2e-7, \
        "%s: obs_norm off the float64 expression" % what


@pytest.mark.parametrize("cell", O.CELLS, ids=[O.cell_id(c) for c in O.CELLS])
def test_option_cell_against_the_oracle(torch, oracle, cell):
    fam, name = cell
    opts = O.OPTIONS[name]
    failures = []
    for noise in O.chains(fam, opts):
        _run_chain(torch, oracle, fam, opts, noise, failures)
    assert not failures, "\n".join(failures)


def _run_chain(torch, oracle, fam, opts, noise, failures, inputs=None, observe=None):
    """inputs: (obstacles, state, time, actions) in place of the cell's own start -- a batch built for another purpose,
    which then asserts its own conditions instead of the cells'.  observe(what, tick, state, time, reseeded): called with
    the device's state after every step() of the chain and after the last step of every other entry point, once the
    checks of this function have passed on it."""
    per_world = fam.table == "world"
    n, mode, off = fam.N, fam.mode, fam.env_offset
    continuous = fam.kind in D.CONTINUOUS
    policy = {"sample_d": "random", "sample_c": "random"}.get(fam.kind)
    obst, st0, tt0, host_acts = O.cell_inputs(oracle, fam, opts) if inputs is None else inputs
    rng = np.random.RandomState(n + fam.K)
    tag = "[noise]" if noise else ""

    def fresh():
        env = _make(torch, n, obst, continuous, mode, off, opts["waves"], opts["random_boat"], opts["random_goal"],
                    opts["time_limit"], opts["norm"])
        if opts["norm"]:
            env.obs_norm_buf.fill_(O.NORM_GUARD)
        env.set_state(st0, tt0, soa=True)
        return env

    env = fresh()
    acts = _device_actions(torch, host_acts, env.ld, rng) if host_acts is not None else None
    noise_buf = None
    if noise:       # rows longer than the state's: noise_ld = ld + NOISE_PAD, the padding holds another value
        noise_buf = torch.full((2, env.ld + O.NOISE_PAD), O.NOISE_GUARD, dtype=torch.float32, device="cuda:0")

    def set_noise(t):
        if noise:
            noise_buf[:, :n].copy_(torch.as_tensor(O.noise_at(n, t)))

    def step_action(t):
        kw = {"noise": noise_buf} if noise else {}
        if policy is not None:
            return dict(kw, policy=policy)
        return dict(kw, action=acts[t], soa=True) if continuous else dict(kw, action=acts[t, :n])

    if opts["norm"]:
        try:
            _norm_failures(torch, env, "set_state()%s" % tag)
        except AssertionError as e:
            failures.append(str(e))

    # the chain of step() calls, each step against the oracle
    want, terms = [], []
    never = np.ones(n, dtype=bool)
    safe = np.ones(n, dtype=bool)                    # stored and sampled actions: every world is compared
    st_last = None
    for t in range(T):
        s0, t0 = _host_state(env)
        tick = env._tick
        set_noise(t)
        _, reward, term = env.step(**step_action(t))
        torch.cuda.synchronize()
        assert noise_buf is None or noise_buf.stride(0) > env.ld
        act = O.actions_at(oracle, fam, host_acts, t, tick)
        st, tt = np.ascontiguousarray(s0.copy()), t0.copy()
        stepped = (tt >= 0) | (tt == -3 - ((tick - 1) & 1)) if mode == 2 else tt >= 0
        o_rew, o_term, reseeded = O.oracle_tick(oracle, st, tt, act, obst, per_world, mode, tick, off, opts,
                                                O.noise_at(n, t) if noise else None)
        if inputs is None:
            O.tick_conditions(fam, opts, t, o_term, reseeded, stepped)      # from the oracle, before the kernel's outputs
        terms.append(o_term)
        never &= ~reseeded
        k_state, k_time = _host_state(env)
        k_rew, k_term = reward.cpu().numpy().copy(), term.cpu().numpy().copy()
        what = "step()%s at tick %d" % (tag, tick)
        _check(what, safe, k_rew, k_term, o_rew, o_term, env.done_mask().cpu().numpy(), k_state, k_time, st, tt, reseeded,
               mode, tick)
        O.fixed_pose_conditions(opts, k_state, reseeded, never, what)
        if observe is not None:
            observe(what, tick, k_state, k_time, reseeded)
        if opts["waves"] == 0:
            assert np.all(k_state[5:7] == 0), "%s: waves=0 leaves a wave" % what
        if opts["norm"]:
            _norm_failures(torch, env, what)
        want.append((o_rew, o_term, safe, k_rew, k_term))
        st_last = (st, tt, reseeded, safe, tick)
    if inputs is None:
        O.cell_conditions(fam, opts, terms)
    chain_state, chain_time = _host_state(env)
    del env

    for entry in O.entries_for(fam, opts, noise):
        if entry == "step":
            continue
        try:
            _run_entry(torch, entry + tag, fresh, acts, policy, continuous, step_action, set_noise, noise_buf, n, want,
                       st_last, mode, chain_state, chain_time, opts, observe)
        except AssertionError as e:
            failures.append(str(e))


def _run_entry(torch, entry, fresh, acts, policy, continuous, step_action, set_noise, noise_buf, n, want, st_last, mode,
               chain_state, chain_time, opts, observe=None):
    env = fresh()
    a = policy if policy is not None else acts
    done = None
    name = entry.split("[")[0]

    def one_step_buffer():
        """a one-step action buffer a captured graph re-reads: the caller copies the step's actions in between replays"""
        if policy is not None:
            return None
        return acts[0:1].clone()

    if name == "rollout":
        dh = torch.zeros((T, env.ld // 64), dtype=torch.int64, device=env.device)
        r, c = env.rollout(T, actions=a, keep_all=True, done_history=dh)
        rew, term, done = r[:, :n], c[:, :n], dh
    elif name == "fused":
        r, c = env.rollout(T, actions=a, fused=True, keep_all=True)
        rew, term = r[:, :n], c[:, :n]
    elif name in ("graph", "graph_fused"):
        # captured after the options are set; one step() ahead of it (a tick-base refresh), then two replays, the
        # action row of each copied into the captured buffer
        fused = name == "graph_fused"
        buf = one_step_buffer()
        g = env.capture_rollout(1, actions=policy if policy is not None else buf, fused=fused, keep_all=True,
                                done_history=None if fused else True)
        rs, cs, ds = [], [], []
        for t in range(T):
            if t == 0:
                _, r1, c1 = env.step(**step_action(0))
                d1 = env.done_mask()
            else:
                if buf is not None:
                    buf[0].copy_(acts[t])
                r1, c1 = g.launch(stream=ctypes.c_void_p(0))
                r1, c1 = r1[0], c1[0]
                d1 = None if fused else torch.as_tensor(_unpack_done(g.done_history[:1], n)[0])
                if opts["norm"]:
                    torch.cuda.synchronize()
                    _norm_failures(torch, env, "%s, replay %d" % (entry, t))
            rs.append(r1[:n].clone()); cs.append(c1[:n].clone())
            if d1 is not None:
                ds.append(d1.cpu().clone())
        rew, term = torch.stack(rs), torch.stack(cs)
        done = None if fused else torch.stack(ds)
    elif name == "graph_step":
        if policy is None:
            buf = acts[0].clone() if continuous else acts[0, :n].clone()
            g = env.capture_step(buf, noise=noise_buf, soa=continuous)
        else:
            assert noise_buf is None
            g = env.capture_rollout(1, actions=policy)
        rs, cs, ds = [], [], []
        for t in range(T):
            set_noise(t)
            if t == 0:
                _, r1, c1 = env.step(**step_action(0))
            else:
                if policy is None:
                    buf.copy_(acts[t] if continuous else acts[t, :n])
                r1, c1 = g.launch(stream=ctypes.c_void_p(0))
                if opts["norm"]:
                    torch.cuda.synchronize()
                    _norm_failures(torch, env, "%s, replay %d" % (entry, t))
            rs.append(r1[:n].clone()); cs.append(c1[:n].clone()); ds.append(env.done_mask().clone())
        rew, term, done = torch.stack(rs), torch.stack(cs), torch.stack(ds)
    else:
        raise AssertionError("unknown entry %s" % entry)
    torch.cuda.synchronize()
    rew, term = rew.cpu().numpy(), term.cpu().numpy()
    if done is not None and done.dtype == torch.int64:
        done = _unpack_done(done[:T], n)
    elif done is not None:
        done = done.cpu().numpy()
    for t in range(T):
        o_rew, o_term, safe, k_rew, k_term = want[t]
        _check("%s, step %d" % (entry, t), safe, rew[t], term[t], o_rew, o_term, None if done is None else done[t])
        assert np.array_equal(rew[t], k_rew) and np.array_equal(term[t], k_term), "%s, step %d: differs from step()" % (entry, t)
    k_state, k_time = _host_state(env)
    st, tt, reseeded, safe, tick = st_last
    _check("%s, final state" % entry, safe, rew[T - 1], term[T - 1], want[T - 1][0], want[T - 1][1], None, k_state, k_time,
           st, tt, reseeded, mode, tick)
    assert np.array_equal(k_state, chain_state) and np.array_equal(k_time, chain_time), "%s: final state differs from step()" % entry
    if observe is not None:
        observe("%s, final state" % entry, tick, k_state, k_time, reseeded)
    if opts["norm"]:
        _norm_failures(torch, env, entry)


@pytest.mark.parametrize("fam", O.KNIFE_FAMILIES, ids=[O.family_id(f) for f in O.KNIFE_FAMILIES])
def test_time_limit_on_the_float64_path(torch, oracle, fam):
    """the limit of 5 where the float64 path decides: a knife-edge batch, half of its worlds on their last step"""
    inputs, timed_out, goes_on = O.knife_inputs(oracle, fam)
    assert int(timed_out.sum()) >= O.KNIFE_MIN and int(goes_on.sum()) >= O.KNIFE_MIN
    failures = []
    _run_chain(torch, oracle, fam, O.OPTIONS["limit5"], False, failures, inputs=inputs)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ reset(), reset(mask)
@pytest.mark.parametrize("cell", O.RESET_CELLS, ids=["%s-K%d-%s" % c for c in O.RESET_CELLS])
def test_reset_options_bit_exact_against_the_oracle(torch, oracle, cell):
    from tests.test_dispatch_matrix import _shared_rows, _world_tables
    table, K, name = cell
    waves, rb, rg = O.RESET_OPTIONS[name]
    n, off = O.RESET_N, 17
    per_world = table == "world"
    obst = _world_tables(K, n) if per_world else _shared_rows(K)
    reset = oracle.reset_tables if per_world else oracle.reset
    env = _make(torch, n, obst, False, 0, off, waves, rb, rg, O.DEFAULT_LIMIT, True)
    env.obs_norm_buf.fill_(O.NORM_GUARD)
    env.reset()
    torch.cuda.synchronize()
    st, tt = np.zeros((7, n), dtype=np.float32), np.full(n, 5, dtype=np.int32)
    reset(st, tt, obst, waves=waves, random_boat=rb, random_goal=rg, seed=SEED, tick=env.RESET_TICK_BASE, env_offset=off)
    k_state, k_time = _host_state(env)
    assert np.array_equal(k_state, st) and np.array_equal(k_time, tt), "reset()"
    everyone = np.ones(n, dtype=bool)
    O.fixed_pose_conditions(dict(random_boat=rb, random_goal=rg), k_state, everyone, ~everyone, "reset()")
    if waves == 0:
        assert np.all(k_state[5:7] == 0)
    if waves == 2:
        assert np.abs(k_state[5:7]).max() <= 0.1 and (np.abs(k_state[5:7]) > 0.05).any()
    _norm_failures(torch, env, "reset()")
    # the masked reset: other worlds keep their state and their obs_norm columns (marked here to tell)
    mask = np.arange(n) % 3 == 0
    env.obs_norm_buf[:, :n][:, torch.as_tensor(~mask).cuda()] = 3.5
    norm_before = env.obs_norm_buf.cpu().numpy()
    env.reset(mask=torch.as_tensor(mask).cuda())
    torch.cuda.synchronize()
    reset(st, tt, obst, waves=waves, random_boat=rb, random_goal=rg, seed=SEED, tick=env.RESET_TICK_BASE + 1,
          env_offset=off, mask=mask.astype(np.uint8))
    after, after_time = _host_state(env)
    assert np.array_equal(after, st) and np.array_equal(after_time, tt), "reset(mask)"
    assert np.array_equal(after[:, ~mask], k_state[:, ~mask])
    norm = env.obs_norm_buf.cpu().numpy()
    assert np.array_equal(norm[:, :n][:, ~mask], norm_before[:, :n][:, ~mask]), "reset(mask) wrote unmasked obs_norm columns"
    assert np.all(norm[:, n:] == np.float32(O.NORM_GUARD))
    scratch = torch.full((5, env.ld), O.NORM_GUARD, dtype=torch.float32, device=env.device)
    from aquaticgymenv_amd import _capi
    _capi.check(_capi.lib.aqua_obs_norm_f32(env.state.data_ptr(), env.ld, n, None, scratch.data_ptr(), env._stream()),
                "aqua_obs_norm_f32")
    torch.cuda.synchronize()
    assert np.array_equal(norm[:, :n][:, mask].view(np.uint32), scratch.cpu().numpy()[:, :n][:, mask].view(np.uint32))
    assert np.max(np.abs(norm[:, :n][:, mask].astype(np.float64) - O.norm_expected(after)[:, mask])) <= 2e-7
