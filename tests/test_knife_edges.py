"""Every step and fused kernel family at the knife edge: batches whose post-move positions sit within a few 1e-6 of a
border, the goal radius or an obstacle surface, or whose heading folds at +-pi (tests/_knife.py), against the float64
oracle.

Cases: action kind (u8, i64, f32x2, sample_d, sample_c, bearing) x restart mode x obstacle table (shared: the quick table
and the row loop; per world: one K per kernel band), each at 65 536 worlds through step(), rollout(T), the fused rollout
and a captured rollout's replay; the product is trimmed only where the dispatch model (tests/_dispatch.py) shows that a
case launches no kernel an earlier case has not.  Plus u8 batches at the batch-size thresholds of the one-table step
kernels (NS_INTERLEAVE_MIN, STORE_WB_NEXT_STEP_MIN, STORE_WB_SAME_STEP_MIN).

Each case is teacher-forced against the oracle with the dispatch matrix's helpers: termination codes, time markers, done
bits and re-seeded states bit-exact on every world (no margin allowance), pose and reward within 1e-5, wave within 1e-7,
the heading within 1e-5 WITHOUT reduction modulo 2 pi (a heading folded to the other end of [-pi, pi) is 2 pi off in the
observation), and every multi-step entry point equal to the step() chain bit for bit.  Each case asserts its own
coverage from the oracle's margins: MIN_TIGHT worlds the float64 path must decide and MIN_TIER2 worlds the second look
decides alone.

test_knife_edge_inside_one_launch puts the knife at the third step of a launch: the float32 state after the second step
of a first run, the oracle's float64 third move from it, the goal put at 5 + delta from where it ends; a second run from
the same start with that goal.
"""
import collections
import zlib

import numpy as np
import pytest

from tests import _dispatch as D
from tests import _knife as KN
from tests import test_dispatch_matrix as M
from tests._parity import _host_state

pytestmark = pytest.mark.gpu

T = M.T
SEED = M.SEED
N = 65536
KINDS = ("u8", "i64", "f32x2", "sample_d", "sample_c", "bearing")
ENTRIES = ("step", "rollout", "fused", "graph")
SHARED_K = (8, 20)                     # the quick table, the row loop
WORLD_K = (8, 11, 33, 20, 9)           # rows in registers (8, 16), the streamed loop with splits 2 and 4, split 1
MIN_TIGHT, MIN_TIER2 = 500, 500

Case = collections.namedtuple("Case", "table K N kind mode entries")


def case_kernels(case):
    """the step and fused kernels the case launches (the dispatch model; reset and tick kernels left out)"""
    out = set()
    for e in case.entries:
        out |= M.cell_kernels(M.Cell(case.table, case.K, case.N, 0, case.kind, case.mode, e))
    return {k for k in out if k.startswith(("step", "rollout"))}


def _cases():
    seen, out = set(), []

    def offer(case):
        new = case_kernels(case) - seen
        if new:
            seen.update(new)
            out.append(case)

    for mode in D.MODES:
        for kind in KINDS:
            for K in SHARED_K:
                offer(Case("shared", K, N, kind, mode, ENTRIES))
            for K in WORLD_K:
                offer(Case("world", K, N, kind, mode, ENTRIES))
    c = D.C
    for n, mode in ((c["NS_INTERLEAVE_MIN"], 2), (c["STORE_WB_NEXT_STEP_MIN"], 2), (c["STORE_WB_SAME_STEP_MIN"], 1)):
        for K in SHARED_K:
            offer(Case("shared", K, n, "u8", mode, ("step",)))
    return out


CASES = _cases()


def _cid(case):
    return "%s-K%d-N%d-%s-mode%d" % (case.table, case.K, case.N, case.kind, case.mode)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _actions(kind, batch, n, rng):
    """host actions [T][..] for the stored kinds: the knife batch's at step 0, the matrix's edge values after it"""
    if kind not in D.STORED:
        return None
    rest = M._stored_actions(kind, n, rng)
    rest[0] = batch.action
    return rest


def _raw_theta(what, k_state, st, live):
    if live.any():
        d = np.max(np.abs(k_state[2, live].astype(np.float64) - st[2, live].astype(np.float64)))
        bad = np.flatnonzero(live & (np.abs(k_state[2].astype(np.float64) - st[2]) > M.TOL))
        assert d <= M.TOL, "%s: heading %.3g off without reduction modulo 2 pi (folded at the other end of [-pi, pi)) " \
                           "on %d worlds: %s" % (what, d, bad.size, bad[:8])


def _run(torch, oracle, case, state0, time0, host_acts, obst, rng):
    """the chain of step() against the oracle from (state0, time0) at tick 0, then every other entry point against the
    chain"""
    n, per_world, mode, kind = case.N, case.table == "world", case.mode, case.kind
    continuous = kind in D.CONTINUOUS
    policy = {"sample_d": "random", "sample_c": "random", "bearing": "bearing"}.get(kind)

    def fresh():
        env = M._make(torch, n, obst, continuous=continuous, seed=SEED, auto_reset=mode)
        env.reset()
        env.set_state(state0, time0, soa=True)
        assert env._tick == 0
        return env

    env = fresh()
    acts = M._device_actions(torch, host_acts, env.ld, rng) if host_acts is not None else None

    def step_action(t):
        if policy is not None:
            return {"policy": policy}
        return {"action": acts[t], "soa": True} if continuous else {"action": acts[t, :n]}

    want, st_last = [], None
    for t in range(T):
        s0, t0 = _host_state(env)
        tick = env._tick
        _, reward, term = env.step(**step_action(t))
        torch.cuda.synchronize()
        if kind == "bearing":
            act, safe = M._bearing_safe(s0.astype(np.float64))
        elif policy is not None:
            act, safe = oracle.sample_actions(n, continuous, seed=SEED, tick=tick), np.ones(n, dtype=bool)
        else:
            act, safe = np.ascontiguousarray(host_acts[t]), np.ones(n, dtype=bool)
        st, tt = np.ascontiguousarray(s0.copy()), t0.copy()
        o_rew, o_term, reseeded = M._oracle_tick(oracle, st, tt, act, obst, per_world, mode, tick, 0)
        k_state, k_time = _host_state(env)
        k_rew, k_term = reward.cpu().numpy().copy(), term.cpu().numpy().copy()
        what = "%s step() at tick %d" % (_cid(case), tick)
        M._check(what, safe, k_rew, k_term, o_rew, o_term, env.done_mask().cpu().numpy(), k_state, k_time, st, tt,
                 reseeded, mode, tick)
        _raw_theta(what, k_state, st, safe & ~reseeded)
        want.append((o_rew, o_term, safe, k_rew, k_term))
        st_last = (st, tt, reseeded, safe, tick)
    chain_state, chain_time = _host_state(env)
    del env
    failures = []
    for entry in case.entries:
        if entry == "step":
            continue
        try:
            M._run_entry(torch, entry, fresh, acts, policy, continuous, step_action, n, want, st_last, mode, chain_state,
                         chain_time)
        except AssertionError as e:
            failures.append("%s: %s" % (_cid(case), e))
    assert not failures, "\n".join(failures)


def _coverage(what, margin, safe):
    tight, tier2 = KN.tiers(margin)
    nt, n2 = int((tight & safe).sum()), int((tier2 & safe).sum())
    assert nt >= MIN_TIGHT and n2 >= MIN_TIER2, "%s: only %d worlds need the float64 path and %d the second look" % (
        what, nt, n2)


@pytest.mark.parametrize("case", CASES, ids=[_cid(c) for c in CASES])
def test_knife_edges_against_the_oracle(torch, oracle, case):
    rng = np.random.RandomState(zlib.crc32(_cid(case).encode()))
    b = KN.build(oracle, case.kind, case.N, rng, K=case.K, per_world=case.table == "world", seed=SEED, tick=0)
    _coverage(_cid(case), KN.nearest(b), b.safe)
    _run(torch, oracle, case, b.state, b.time, _actions(case.kind, b, case.N, rng), b.obst, rng)


# ------------------------------------------------------------------------------------------------ knife at step 3
INSIDE = [Case(t, K, N, kind, mode, ("step", "rollout", "fused", "graph"))
          for t, K in (("shared", 8), ("shared", 20), ("world", 8), ("world", 11), ("world", 20), ("world", 33))
          for kind, mode in (("u8", 0), ("f32x2", 1), ("sample_c", 2), ("sample_d", 1), ("i64", 2))]


@pytest.mark.parametrize("case", INSIDE, ids=[_cid(c) for c in INSIDE])
def test_knife_edge_inside_one_launch(torch, oracle, case):
    """the goal radius at 5 + delta from the float64 position after the third step: the fused and captured launches
    take the second look and the float64 path from the state they hold after two steps of their own"""
    rng = np.random.RandomState(zlib.crc32(("inside" + _cid(case)).encode()))
    n, per_world, kind = case.N, case.table == "world", case.kind
    b = KN.build(oracle, kind, n, rng, K=case.K, per_world=per_world, seed=SEED, tick=0, subjects=("wrap",))
    host_acts = _actions(kind, b, n, rng)
    continuous = kind in D.CONTINUOUS
    # run 1: the chain's float32 state after two steps
    env = M._make(torch, n, b.obst, continuous=continuous, seed=SEED, auto_reset=0)
    env.reset()
    env.set_state(b.state, b.time, soa=True)
    tick0 = env._tick
    acts = M._device_actions(torch, host_acts, env.ld, rng) if host_acts is not None else None
    for t in range(T - 1):
        if host_acts is None:
            env.step(policy="random")
        else:
            env.step(acts[t], soa=True) if continuous else env.step(acts[t, :n])
    torch.cuda.synchronize()
    s1, t1 = _host_state(env)
    del env
    # the oracle's float64 third move from it; the goal at 5 + delta from where it ends, on the side it comes from
    act = host_acts[T - 1] if host_acts is not None else oracle.sample_actions(n, continuous, seed=SEED, tick=tick0 + T - 1)
    s64 = np.ascontiguousarray(s1.astype(np.float64))
    tt = np.ascontiguousarray(np.maximum(t1, 0).astype(np.int32))
    p1 = s64[0:2].copy()
    if per_world:
        oracle.step_tables(s64, tt, act, b.obst, waves=1, seed=SEED, tick=tick0 + T - 1)
    else:
        oracle.step(s64, tt, act, obstacles=b.obst, waves=1, seed=SEED, tick=tick0 + T - 1, want_margins=False)
    p2 = s64[0:2]
    u = p2 - p1
    u /= np.maximum(np.hypot(u[0], u[1]), 1e-12)
    goal = p2 + (5.0 + KN._deltas(rng, n)) * u
    state0 = b.state.copy()
    state0[3:5] = goal.astype(np.float32)
    time0 = np.minimum(b.time, 900).astype(np.int32)           # no time-outs before the knife
    # coverage at the third step, from the oracle's margins: run 1's state after two steps with the goal moved (the goal
    # does not move the boat; a world that reaches the moved goal earlier restarts in run 2 and is not counted here)
    s64 = np.ascontiguousarray(s1.astype(np.float64))
    s64[3:5] = state0[3:5]
    tt = np.ascontiguousarray(np.maximum(t1, 0).astype(np.int32))
    if per_world:
        _, _, m = oracle.step_tables(s64, tt, act, b.obst, waves=1, seed=SEED, tick=tick0 + T - 1)
    else:
        _, _, m = oracle.step(s64, tt, act, obstacles=b.obst, waves=1, seed=SEED, tick=tick0 + T - 1)
    _coverage(_cid(case) + " at the third step", m[2], t1 >= 0)
    # run 2: the same start with the goal moved, every entry point against the oracle
    _run(torch, oracle, case, state0, time0, host_acts, b.obst, rng)
