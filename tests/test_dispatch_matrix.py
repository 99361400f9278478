"""Every kernel instantiation the library launches, against the float64 oracle.

The cells (CELLS) are generated from the dispatch model (tests/_dispatch.py): action kind (all seven) x restart mode x
entry point (step(), rollout(), the fused rollout, captured rollouts fused and not, a captured step) x obstacle table
(shared: K = 0, 1, 8, 9, 20 -- the quick table, both sides of QUICK_MAX / NS_TABLE_ROWS, the row loop; per world: K at
every band edge of the per-world kernels) at small ragged batches, and the batch sizes on both sides of every dispatch
threshold of the one-table step kernels.  tests/test_kernel_coverage.py checks on the CPU that the cells reach every
instantiation of the built code object.

Each cell is teacher-forced against the oracle: a chain of step() calls is checked step by step (the oracle restarts
from the kernel's state every step), and the entry point under test, run from the same start, must give the oracle's
per-step outputs and final state -- and the chain's, bit for bit.  Bars of the rest of the suite: termination codes,
time markers, done bits and re-seeded states bit-exact; pose and reward within 1e-5; wave within 1e-7.  Stored actions
carry the values where a decode goes wrong (out-of-range and negative indices, int64 beyond 32 bits, thrusts outside
[0.2, 0.5], exactly on its ends, equal); the rollout buffers' rows are longer than the batch (stride(0) > ld).  Sampled
actions are the oracle's exported Philox stream-4 draws; the bearing policy is _bearing_np, without the worlds at its
decision threshold.  Graph cells replay once with stream=ctypes.c_void_p(0) after a step() (the tick-base refresh).
"""
import collections
import ctypes
import zlib

import numpy as np
import pytest

from tests import _dispatch as D
from tests._golden import angle_diff
from tests._parity import TOL, _make, _host_state, _oracle_next_step_tables, _bearing_np

pytestmark = pytest.mark.gpu

T = 3                     # steps per cell
PAD = 37                  # extra elements per row of a rollout's action buffer (stride(0) > ld)
SEED = 4242
GRAPH_ENTRIES = ("graph", "graph_fused", "graph_step")

Cell = collections.namedtuple("Cell", "table K N env_offset kind mode entry")

SHARED_K = (0, 1, 8, 9, 20)
WORLD_K_ALL_ENTRIES = (8, 9, 11, 17, 24, 33)           # one K per kernel band: every entry point
WORLD_K_EDGES = (10, 16, 23, 32, 64)                   # the other side of each band edge: per-step and fused kernels
OFFSETS = (0, 7, 2 ** 32 - 3)
SIZES = (4099, 3011)


def _large_groups():
    """(K, N, mode, kinds) at the batch-size thresholds of launch_step / launch_step_ns: both sides of each edge with u8
    and i64, every kind inside each band with a table on either side of NS_TABLE_ROWS"""
    c = D.C
    both, every = ("u8", "i64"), tuple(D.KINDS)
    small, loop = c["NS_TABLE_ROWS"], c["NS_TABLE_ROWS"] + 1
    out = []
    for n, mode, kinds, ks in (
            (c["NS_INTERLEAVE_MIN"] - 1, 2, both, (small,)),
            (c["NS_INTERLEAVE_MIN"], 2, every, (small, loop)),
            (c["DONE_WORD_WRITE_THROUGH_MAX_WORLDS"], 1, both, (small,)),
            (c["DONE_WORD_WRITE_THROUGH_MAX_WORLDS"] + 1, 1, both, (small,)),
            (c["STORE_WB_SAME_STEP_MIN"] - 1, 1, both, (small,)),
            (c["STORE_WB_SAME_STEP_MIN"], 1, every, (small, loop)),
            (c["STORE_WB_NEXT_STEP_MIN"] - 1, 2, both, (small,)),
            (c["STORE_WB_NEXT_STEP_MIN"], 2, every, (small, loop)),
            (c["STORE_WB_NEXT_STEP_MAX"], 2, both, (small,)),
            (c["STORE_WB_NEXT_STEP_MAX"] + 1, 2, both, (small,))):
        for k in ks:
            out.append((k, n, mode, kinds))
    return out


def _cells():
    cells, i = [], 0
    for K in SHARED_K:
        for kind in D.KINDS:
            for mode in D.MODES:
                n, off = SIZES[i % 2], OFFSETS[i % 3]
                i += 1
                cells += [Cell("shared", K, n, off, kind, mode, e) for e in D.SHARED_ENTRIES]
    for K in WORLD_K_ALL_ENTRIES + WORLD_K_EDGES:
        entries = D.TABLE_ENTRIES if K in WORLD_K_ALL_ENTRIES else ("step", "fused")
        for kind in D.KINDS:
            for mode in D.MODES:
                n, off = SIZES[i % 2], OFFSETS[i % 3]
                i += 1
                cells += [Cell("world", K, n, off, kind, mode, e) for e in entries]
    for K, n, mode, kinds in _large_groups():
        cells += [Cell("shared", K, n, 0, kind, mode, "step") for kind in kinds]
    return cells


CELLS = _cells()


def cell_kernels(cell):
    """the model's prediction for one cell: the entry point's launches, the reset ahead of it, and -- for a graph -- the
    step() launched eagerly ahead of the replay"""
    per_world = cell.table == "world"
    captured = T - 1 if cell.entry in ("graph", "graph_fused") else T
    out = D.launched(cell.entry, cell.kind, cell.mode, cell.K, cell.N, per_world=per_world, T=captured)
    if cell.entry in GRAPH_ENTRIES:
        out |= D.launched("step", cell.kind, cell.mode, cell.K, cell.N, per_world=per_world)
    return out


def _groups():
    g = collections.OrderedDict()
    for c in CELLS:
        g.setdefault(c[:6], []).append(c.entry)
    return list(g.items())


GROUPS = _groups()


def _gid(group):
    (table, K, N, off, kind, mode), entries = group
    return "%s-K%d-N%d-off%d-%s-mode%d" % (table, K, N, off, kind, mode)


# ------------------------------------------------------------------------------------------------ inputs
def _shared_rows(K):
    if K == 0:
        return np.zeros((0, 5))
    rng = np.random.RandomState(300 + K)
    kinds = rng.permutation(np.arange(K) % 2).astype(np.float64)        # circles and rectangles interleaved
    rows = np.zeros((K, 5))
    rows[:, 0:2] = rng.uniform(12, 88, (K, 2))
    rows[:, 2] = kinds
    rows[:, 3] = np.where(kinds == 0, rng.uniform(2, 5, K), rng.uniform(4, 10, K))
    rows[:, 4] = np.where(kinds == 0, 0.0, rng.uniform(4, 10, K))
    return rows


def _world_tables(K, n):
    """[n][K][5] per-world rows, some absent (kind -1); smaller obstacles for long tables"""
    rng = np.random.RandomState(500 + K)
    t = np.zeros((n, K, 5))
    t[:, :, 0:2] = rng.uniform(10, 90, (n, K, 2))
    kind = rng.randint(0, 2, (n, K)).astype(np.float64)
    scale = 1.0 if K <= 16 else (10.0 / K) ** 0.5
    t[:, :, 2] = np.where(rng.randint(0, 4, (n, K)) == 0, -1.0, kind)
    t[:, :, 3] = np.where(kind == 0, rng.uniform(2, 8, (n, K)), rng.uniform(4, 12, (n, K))) * scale
    t[:, :, 4] = np.where(kind == 0, 0.0, rng.uniform(4, 12, (n, K)) * scale)
    return t


I32_EDGES = (-3, -2, -1, 3, -4, -2 ** 31, 2 ** 31 - 1)
I64_EDGES = I32_EDGES + (2 ** 32 + 1, -2 ** 32, 2 ** 32, -2 ** 32 + 1, -2 ** 63, 2 ** 63 - 1)


def _stored_actions(kind, n, rng):
    """host actions [T][n] (discrete) or [T][2][n] (thrusts), a third of them at the values where decodes go wrong"""
    if kind == "f32x2":
        a = rng.uniform(0.1, 0.6, (T, 2, n)).astype(np.float32)
        pick = rng.randint(0, 10, (T, 2, n))
        a[pick == 0] = np.float32(0.2)
        a[pick == 1] = np.float32(0.5)
        same = rng.randint(0, 6, (T, n)) == 0                    # equal thrusts: the epsilon branch
        a[:, 1][same] = a[:, 0][same]
        return a
    dtype, edges = {"u8": (np.uint8, tuple(range(3, 256))), "i32": (np.int32, I32_EDGES), "i64": (np.int64, I64_EDGES)}[kind]
    a = rng.randint(0, 3, (T, n)).astype(np.int64)
    odd = rng.randint(0, 3, (T, n)) == 0
    a[odd] = np.array(edges, dtype=np.int64)[rng.randint(0, len(edges), int(odd.sum()))]
    return a.astype(dtype)


def _device_actions(torch, host, ld, rng):
    """the host actions in a device buffer whose rows hold PAD more elements than ld (filled with other values)"""
    if host.ndim == 3:
        buf = rng.uniform(0.2, 0.5, (T, 2, ld + PAD)).astype(np.float32)
        buf[:, :, :host.shape[2]] = host
    else:
        buf = rng.randint(0, 3, (T, ld + PAD)).astype(host.dtype)
        buf[:, :host.shape[1]] = host
    dev = torch.as_tensor(buf).cuda()
    assert dev.stride(-2) > ld
    return dev


def _bearing_safe(s):
    """_bearing_np's action and the worlds where float32 and float64 must choose it alike: not within 1e-5 of its
    decision threshold, nor of the points where the boat's or the goal's angle wraps from 2 pi to 0 (at two million
    worlds some sit there, and the two precisions may then put the angle on either side)"""
    act, edge = _bearing_np(s)
    two_pi = 2 * np.pi
    boat = (s[2] + np.pi / 2 + two_pi) % two_pi
    goal = (np.arctan2(s[4] - s[1], s[3] - s[0]) + two_pi) % two_pi
    wrap = np.minimum(np.minimum(boat, two_pi - boat), np.minimum(goal, two_pi - goal))
    return act, (edge > 1e-5) & (wrap > 1e-5)


def _unpack_done(words, n):
    w = words.cpu().numpy().view(np.uint64)
    bits = (w[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(w.shape[:-1] + (-1,))[..., :n].astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the oracle side
def _oracle_tick(oracle, st, tt, act, obst, per_world, mode, tick, env_offset):
    """one tick of the restart convention `mode` on the CPU from the kernel's float32 state st [7][n] / time tt [n]
    (in place) -> (reward, term, re-seeded worlds)"""
    reseeded = (tt == -1 - ((tick - 1) & 1)) if mode == 2 else None
    if not per_world:
        _, rew, term, _ = oracle.rollout_f32(st, tt, 1, obstacles=obst, waves=1, actions=act, seed=SEED, tick0=tick,
                                              env_offset=env_offset, auto_reset=mode)
    elif mode == 2:
        rew, term = _oracle_next_step_tables(oracle, st, tt, act, obst, SEED, tick, env_offset)
    else:
        s64 = np.ascontiguousarray(st.astype(np.float64))
        rew, term, _ = oracle.step_tables(s64, tt, act, obst, waves=1, seed=SEED, tick=tick, env_offset=env_offset)
        st[:] = s64.astype(np.float32)
        if mode == 1:
            oracle.reset_tables(st, tt, obst, waves=1, seed=SEED, tick=tick, env_offset=env_offset, mask=term != 0)
    if mode == 1:
        reseeded = term != 0
    elif mode == 0:
        reseeded = np.zeros(tt.shape[0], dtype=bool)
    return np.asarray(rew, dtype=np.float32), term, reseeded


def _check(what, safe, k_rew, k_term, o_rew, o_term, k_done=None, k_state=None, k_time=None, st=None, tt=None,
           reseeded=None, mode=0, tick=0):
    """the suite's bars, on the worlds in `safe`"""
    assert np.array_equal(k_term[safe], o_term[safe]), "%s: termination codes differ from the oracle at %s" % (
        what, np.flatnonzero(k_term[safe] != o_term[safe])[:8])
    assert np.max(np.abs(k_rew[safe] - o_rew[safe]), initial=0) <= TOL, "%s: reward" % what
    if k_done is not None:
        assert np.array_equal(k_done[safe], (o_term[safe] != 0).astype(np.uint8)), "%s: done bits" % what
    if k_state is None:
        return
    assert np.array_equal(k_time[safe], tt[safe]), "%s: time markers differ at %s" % (
        what, np.flatnonzero(k_time[safe] != tt[safe])[:8])
    re = reseeded & safe
    assert np.array_equal(k_state[:, re], st[:, re]), "%s: re-seeded states differ" % what
    if mode == 2:
        assert np.all(k_rew[re] == 0) and np.all(k_term[re] == 0), what
        assert np.all(k_time[re] == -3 - (tick & 1)), what
    live = safe & ~reseeded
    if live.any():
        assert np.max(np.abs(k_state[0:2, live] - st[0:2, live])) <= TOL, "%s: position" % what
        assert np.max(angle_diff(k_state[2, live], st[2, live])) <= TOL, "%s: heading" % what
        assert np.max(np.abs(k_state[5:7, live] - st[5:7, live])) <= 1e-7, "%s: wave" % what
        assert np.array_equal(k_state[3:5, live], st[3:5, live]), "%s: goal" % what


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


@pytest.mark.parametrize("group", GROUPS, ids=[_gid(g) for g in GROUPS])
def test_dispatch_cell_against_the_oracle(torch, oracle, group):
    (table, K, n, off, kind, mode), entries = group
    per_world = table == "world"
    obst = _world_tables(K, n) if per_world else _shared_rows(K)
    continuous = kind in D.CONTINUOUS
    rng = np.random.RandomState(zlib.crc32(_gid(group).encode()))
    policy = {"sample_d": "random", "sample_c": "random", "bearing": "bearing"}.get(kind)

    def fresh():
        env = _make(torch, n, obst, continuous=continuous, seed=SEED, auto_reset=mode, env_offset=off)
        env.reset()
        env.time[:n].copy_(torch.as_tensor(time0))
        return env

    # a tenth of the worlds finish on time within the cell's steps; others may collide or arrive
    time0 = np.where(rng.randint(0, 10, n) == 0, rng.randint(998, 1001, n), rng.randint(0, 990, n)).astype(np.int32)
    host_acts = _stored_actions(kind, n, rng) if policy is None else None
    env = fresh()
    acts = _device_actions(torch, host_acts, env.ld, rng) if host_acts is not None else None

    def step_action(t):
        if policy is not None:
            return {"policy": policy}
        return {"action": acts[t], "soa": True} if continuous else {"action": acts[t, :n]}

    # the chain of step() calls, each step against the oracle
    want = []                                   # per step: (o_rew, o_term, safe, k_rew, k_term)
    st_last = None
    for t in range(T):
        s0, t0 = _host_state(env)
        tick = env._tick
        _, reward, term = env.step(**step_action(t))
        torch.cuda.synchronize()
        if kind == "bearing":
            act, safe = _bearing_safe(s0.astype(np.float64))
            assert (~safe).sum() <= max(20, n // 1000)
        elif policy is not None:
            act, safe = oracle.sample_actions(n, continuous, seed=SEED, tick=tick, env_offset=off), np.ones(n, dtype=bool)
        else:
            act, safe = np.ascontiguousarray(host_acts[t]), np.ones(n, dtype=bool)
        st, tt = np.ascontiguousarray(s0.copy()), t0.copy()
        o_rew, o_term, reseeded = _oracle_tick(oracle, st, tt, act, obst, per_world, mode, tick, off)
        k_state, k_time = _host_state(env)
        k_rew, k_term = reward.cpu().numpy().copy(), term.cpu().numpy().copy()
        _check("step() at tick %d" % tick, safe, k_rew, k_term, o_rew, o_term, env.done_mask().cpu().numpy(), k_state,
               k_time, st, tt, reseeded, mode, tick)
        want.append((o_rew, o_term, safe, k_rew, k_term))
        st_last = (st, tt, reseeded, safe, tick)
    chain_state, chain_time = _host_state(env)
    del env

    failures = []
    for entry in entries:
        if entry == "step":
            continue
        try:
            _run_entry(torch, entry, fresh, acts, policy, continuous, step_action, n, want, st_last, mode,
                       chain_state, chain_time)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


def _run_entry(torch, entry, fresh, acts, policy, continuous, step_action, n, want, st_last, mode, chain_state, chain_time):
    env = fresh()
    a = policy if policy is not None else acts
    done = None
    if entry == "rollout":
        dh = torch.zeros((T, env.ld // 64), dtype=torch.int64, device=env.device)
        r, c = env.rollout(T, actions=a, keep_all=True, done_history=dh)
        rew, term, done = r[:, :n], c[:, :n], dh
    elif entry == "fused":
        r, c = env.rollout(T, actions=a, fused=True, keep_all=True)
        rew, term = r[:, :n], c[:, :n]
    elif entry in ("graph", "graph_fused"):
        fused = entry == "graph_fused"
        g = env.capture_rollout(T - 1, actions=a if policy is not None else acts[1:], fused=fused, keep_all=True,
                                done_history=None if fused else True)
        _, r0, c0 = env.step(**step_action(0))
        r0, c0, d0 = r0.clone(), c0.clone(), env.done_mask().clone()
        r, c = g.launch(stream=ctypes.c_void_p(0))          # the null stream's handle, after a step(): a tick-base refresh
        rew, term = torch.cat([r0[None], r[:, :n]]), torch.cat([c0[None], c[:, :n]])
        if not fused:
            done = (d0, g.done_history)
    elif entry == "graph_step":
        if policy is None:
            buf = acts[0].clone() if continuous else acts[0, :n].clone()
            g = env.capture_step(buf, soa=continuous)
        else:
            g = env.capture_rollout(1, actions=policy)
        rs, cs, ds = [], [], []
        for t in range(T):
            if t == 0:
                _, r1, c1 = env.step(**step_action(0))
            else:
                if policy is None:
                    buf.copy_(acts[t] if continuous else acts[t, :n])
                r1, c1 = g.launch(stream=ctypes.c_void_p(0))
            rs.append(r1[:n].clone()); cs.append(c1[:n].clone()); ds.append(env.done_mask().clone())
        rew, term, done = torch.stack(rs), torch.stack(cs), torch.stack(ds)
    else:
        raise AssertionError("unknown entry %s" % entry)
    torch.cuda.synchronize()
    rew, term = rew.cpu().numpy(), term.cpu().numpy()
    if isinstance(done, tuple):
        done = np.concatenate([done[0].cpu().numpy()[None], _unpack_done(done[1][:T - 1], n)])
    elif done is not None and done.dtype == torch.int64:
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
