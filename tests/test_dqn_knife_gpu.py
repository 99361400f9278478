"""Knife edges of the DQN libraries that tolerance-free random tests pass by: the exploration threshold AT equality
(libaqua_policy.so, libaqua_bank.so, libaqua_episodes.so) and Adam where its epsilon decides the step (libaqua_learner.so).
tools/mutation_audit.py found the `<=` mutants of the three exploring kernels alive under the earlier suite, and the three
eps mutants of the apply kernel killed only by parameters that happened to have tiny gradients; these tests kill them by
construction, with what else the audit left alive (profiles/LOG.md, "Mutation audit of the DQN libraries").

Exploration.  The contract of include/aqua_policy.h, aqua_bank.h and aqua_episodes.h: a world explores iff
u = (r[0] >> 8) * 2^-24 < epsilon, both float32.  u is a multiple of 2^-24, so the test takes epsilon = u_i of a chosen world
(it must NOT explore) and the next float32 above it (it must, and nothing else may change).  Everything is exact: integer
networks on integer inputs (tests/_qbank.py) make the greedy action a CPU fact, the draws come from the oracle's Philox.

Adam.  See test_adam_where_epsilon_decides_the_step.
"""
import types

import numpy as np
import pytest

from tests import _episodes as E
from tests import _learner as L
from tests import _qbank as B

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 4099                                  # 128 full tiles of 32 worlds and a ragged one of 3
NETWORKS, SEG = 3, 1367                   # the bank: worlds [0, 1367) | [1367, 2734) | [2734, 4099): the last segment is cut by N
OFFSET = (5 << 32) + 12345                # a world index beyond 32 bits
SEED = 0x1234567890ABCDEF
TICK0 = (1 << 32) + 5
F32 = np.float32
ULP24 = F32(2.0 ** -24)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _regions():
    """the first tile, the ragged last tile, and network 1's segment without its first and last tile"""
    return (np.arange(0, 32), np.arange(SEG + 32, 2 * SEG - 32), np.arange(N - N % 32, N))


def _pick(u, drawn, greedy_all):
    """one world per region whose u is unique in the batch, inside (0.05, 0.95), and whose exploring action differs from every
    greedy action in greedy_all -> [i0, i1, i2] or None"""
    values, counts = np.unique(u, return_counts=True)
    unique = np.isin(u, values[counts == 1])
    good = unique & (u > F32(0.05)) & (u < F32(0.95))
    for g in greedy_all:
        good &= drawn != g
    picks = [r[good[r]] for r in _regions()]
    return None if any(p.size == 0 for p in picks) else [int(p[0]) for p in picks]


@pytest.fixture(scope="module")
def knife(torch, oracle):
    """inputs, CPU greedy actions, the draws of a tick at which every region has a candidate world, device objects"""
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.qpolicy import QNetwork
    x = np.concatenate([B.segment_inputs(SEG, 40 + p) for p in range(NETWORKS)])[:N]
    q_single = B.int_eval(B.family(0), x)
    q_bank = np.concatenate([B.int_eval(B.family(p), x[p * SEG:(p + 1) * SEG]) for p in range(NETWORKS)])
    greedy_single, greedy_bank = (np.argmax(q, axis=1).astype(np.uint8) for q in (q_single, q_bank))
    assert (greedy_single != greedy_bank).any()
    for tick in range(TICK0, TICK0 + 16):
        u, drawn = E.draws(oracle, N, SEED, OFFSET, tick)
        chosen = _pick(u, drawn, (greedy_single, greedy_bank))
        if chosen is not None:
            break
    assert chosen is not None, "no tick in 16 with a candidate world in every region"
    ld = N + 37
    buf = torch.full((5, ld), 1.0e30, dtype=torch.float32, device=DEV)
    buf[:, :N] = torch.as_tensor(x.T.astype(np.float32))
    env = types.SimpleNamespace(torch=torch, device=torch.device(DEV), num_envs=N, env_offset=OFFSET, seed=SEED, _tick=tick, continuous=False)
    return types.SimpleNamespace(x=x, buf=buf, ld=ld, tick=tick, u=u, drawn=drawn, chosen=chosen, env=env,
                                 q_single=q_single, q_bank=q_bank, greedy_single=greedy_single, greedy_bank=greedy_bank,
                                 qnet=QNetwork(B.family(0), DEV), bank=QNetworkBank([B.family(p) for p in range(NETWORKS)], SEG, DEV))


def _model(k, eps, greedy):
    """eps: float32 scalar or float32 [N] (per world) -> the actions of the contract, exactly u < epsilon"""
    return np.where(k.u < eps, k.drawn, greedy).astype(np.uint8)


def _launch(torch, k, policy, eps, q_int):
    """one epsilon-greedy launch of a QNetwork or a bank -> actions [N]; q_taken must be the Q of the action TAKEN, nothing
    may be written behind N"""
    a, q, qt = B.outputs(torch, k.ld)
    policy.act(k.buf, n=N, epsilon=float(eps), env_offset=OFFSET, seed=SEED, tick=k.tick, out=a, q=q, q_taken=qt)
    ak, qk, qtk = a.cpu().numpy(), q.cpu().numpy(), qt.cpu().numpy()
    assert B.untouched(ak, qk, qtk, N)
    assert np.array_equal(qk[:, :N], q_int.T.astype(np.float32))
    assert np.array_equal(qtk[:N], q_int[np.arange(N), ak[:N].astype(np.int64)].astype(np.float32))
    return ak[:N]


def _explore(torch, k, eps, greedy):
    from aquaticgymenv_amd.episodes import EpisodeTracker
    act = torch.full((k.ld,), B.ACT_FILL, dtype=torch.uint8, device=DEV)
    act[:N] = torch.as_tensor(greedy)
    EpisodeTracker(k.env).explore(act, epsilon=torch.tensor([eps], dtype=torch.float32, device=DEV))
    got = act.cpu().numpy()
    assert bool((got[N:] == B.ACT_FILL).all())
    return got[:N]


def _per_network(k, i, eps):
    """device epsilons of the bank: world i's network holds eps, the other two hold 0 and 1 -> (float32 [3], float32 [N] per world)"""
    p = i // SEG
    per_net = np.zeros(NETWORKS, dtype=np.float32)
    per_net[p] = eps
    per_net[(p + 1) % NETWORKS], per_net[(p + 2) % NETWORKS] = 0.0, 1.0
    return per_net, np.repeat(per_net, SEG)[:N]


@pytest.mark.parametrize("region", [0, 1, 2], ids=["first_tile", "between", "ragged_last_tile"])
def test_exploration_at_the_threshold_is_strict(torch, knife, region):
    """epsilon = u_i: world i is greedy (u < epsilon is false at equality).  epsilon = nextafter(u_i, 1): world i explores and
    no other world changes.  QNetwork.act, the bank with a uniform and with a per-network device epsilon, and the
    exploration pass of libaqua_episodes.so, each bit for bit against the numpy model."""
    k = knife
    i = k.chosen[region]
    below, above = F32(k.u[i]), np.nextafter(F32(k.u[i]), F32(1))
    assert below.dtype == above.dtype == np.float32 and above - below <= ULP24 and i in _regions()[region]
    results = {}
    for side, eps in (("at", below), ("above", above)):
        want = _model(k, eps, k.greedy_single)
        want_bank = _model(k, eps, k.greedy_bank)
        per_net, per_world = _per_network(k, i, eps)
        want_dev = _model(k, per_world, k.greedy_bank)
        explores = side == "above"
        for w, g in ((want, k.greedy_single), (want_bank, k.greedy_bank), (want_dev, k.greedy_bank)):
            assert (w[i] == k.drawn[i]) == explores and (w[i] == g[i]) != explores        # the model itself sits on the edge
        results[side] = (want, want_bank, want_dev)
        assert np.array_equal(_launch(torch, k, k.qnet, eps, k.q_single), want), ("QNetwork.act", side, i)
        k.bank.epsilon = None
        assert np.array_equal(_launch(torch, k, k.bank, eps, k.q_bank), want_bank), ("bank, uniform epsilon", side, i)
        k.bank.epsilon = torch.as_tensor(per_net).to(DEV)
        # (the call's epsilon is then ignored: 0.5 would let half of the worlds of the network that holds 0 explore)
        assert np.array_equal(_launch(torch, k, k.bank, 0.5, k.q_bank), want_dev), ("bank, device epsilon", side, i)
        k.bank.epsilon = None
        assert np.array_equal(_explore(torch, k, eps, k.greedy_single), want), ("EpisodeTracker.explore", side, i)
    for at, above_ in zip(results["at"], results["above"]):
        assert np.flatnonzero(at != above_).tolist() == [i]                                # every other world is unchanged
    # the device-epsilon model: one network never explores, one always does
    q = i // SEG
    never, always = (q + 1) % NETWORKS, (q + 2) % NETWORKS
    dev = results["at"][2]
    lo, hi = never * SEG, min((never + 1) * SEG, N)
    assert np.array_equal(dev[lo:hi], k.greedy_bank[lo:hi])
    lo, hi = always * SEG, min((always + 1) * SEG, N)
    assert np.array_equal(dev[lo:hi], k.drawn[lo:hi])


@pytest.mark.parametrize("eps", [2.0 ** -24, 1.0 - 2.0 ** -24], ids=["one_step_above_zero", "one_step_below_one"])
def test_exploration_at_the_ends_of_the_unit_interval(torch, knife, eps):
    """epsilon = 2^-24: only a world with u == 0 may explore; epsilon = 1 - 2^-24 = the largest u: only a world with that u
    stays greedy.  Whatever the model says for these 4099 draws is asserted."""
    k = knife
    eps = F32(eps)
    assert float(eps) in (2.0 ** -24, 1.0 - 2.0 ** -24)
    want, want_bank = _model(k, eps, k.greedy_single), _model(k, eps, k.greedy_bank)
    explores = k.u < eps
    print("epsilon %.9g: %d of %d worlds explore" % (eps, int(explores.sum()), N))
    assert np.array_equal(explores, k.u == 0) if eps < 0.5 else np.array_equal(~explores, k.u == F32(1.0 - 2.0 ** -24))
    assert np.array_equal(_launch(torch, k, k.qnet, eps, k.q_single), want)
    assert np.array_equal(_launch(torch, k, k.bank, eps, k.q_bank), want_bank)
    k.bank.epsilon = torch.full((NETWORKS,), float(eps), dtype=torch.float32, device=DEV)
    assert np.array_equal(_launch(torch, k, k.bank, 0.5, k.q_bank), want_bank)
    k.bank.epsilon = None
    assert np.array_equal(_explore(torch, k, eps, k.greedy_single), want)


def _twin(torch, n, seed):
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.batched import BatchedAqua
    envs = [BatchedAqua(n, obstacles=presets.BENCH8, seed=seed, auto_reset="next_step", env_offset=OFFSET, device=DEV) for _ in range(2)]
    for e in envs:
        e.reset()
    return envs


def test_step_with_a_network_policy_at_the_threshold(torch, oracle):
    """env.step(policy=qnet, epsilon) against act-then-step on a twin, at epsilon = u_i and one float32 above, for a world of
    the first tile, of the ragged last tile and of one in between.  Twins of one seed start from the same state, so the greedy
    actions of the first step (one greedy launch) and its draws (the oracle) hold for every pair."""
    from aquaticgymenv_amd.qpolicy import QNetwork
    qnet = QNetwork(B.golden_layers("with_obs"), DEV)
    for seed in range(SEED, SEED + 8):                      # (the first seed whose draws leave a candidate in the three-world last tile)
        probe = _twin(torch, N, seed)[0]
        tick = probe._tick
        greedy = qnet.act(probe).cpu().numpy().copy()
        u, drawn = E.draws(oracle, N, probe.seed, probe.env_offset, tick)
        assert probe.seed == seed and probe.env_offset == OFFSET
        chosen = _pick(u, drawn, (greedy,))
        if chosen is not None:
            break
    assert chosen is not None
    act = torch.zeros(N, dtype=torch.uint8, device=DEV)
    for i in chosen:
        seen = []
        for eps in (F32(u[i]), np.nextafter(F32(u[i]), F32(1))):
            a, b = _twin(torch, N, seed)
            assert a._tick == tick and torch.equal(a.state, probe.state)
            a.step(policy=qnet, epsilon=float(eps))
            qnet.act(b, out=act, epsilon=float(eps))
            b.step(act)
            want = np.where(u < eps, drawn, greedy).astype(np.uint8)
            assert np.array_equal(a.policy_action[:N].cpu().numpy(), want), (i, eps)
            assert torch.equal(a.policy_action[:N], act)
            assert (torch.equal(a.state, b.state) and torch.equal(a.reward, b.reward) and torch.equal(a.term, b.term)
                    and torch.equal(a.done_bits, b.done_bits) and torch.equal(a.time, b.time)), (i, eps)
            seen.append(want)
        assert seen[0][i] == greedy[i] != drawn[i] == seen[1][i] and np.flatnonzero(seen[0] != seen[1]).tolist() == [i]


# ------------------------------------------------------------------------------------------------ what else the audit left alive
def _tie_layers(variant):
    """tests/_qbank.py's integer network with output columns made equal: Q0 == Q1, Q1 == Q2 or all three, on every world"""
    (k0, b0), (k1, b1), (k2, b2) = B.base_layers()
    k2, b2 = k2.copy(), b2.copy()
    for dst, src in {"plain": (), "tie01": ((1, 0),), "tie01_top": ((1, 0), (2, 0)), "tie12": ((2, 1),), "tie012": ((1, 0), (2, 0))}[variant]:
        k2[:, dst], b2[dst] = k2[:, src], b2[src]
    if variant == "tie01_top":
        b2[2] -= 1                                             # Q2 = Q0 - 1: the tie of 0 and 1 is the maximum on every world
    return [(k0, b0), (k1, b1), (k2, b2)]


def test_exact_ties_take_the_lowest_index_in_the_bank_and_the_policy_kernel(torch):
    """np.argmax: the lowest index on a tie.  `>=` in the FIRST comparison of qbank_kernel's arg-max survived the earlier
    suite (its integer banks have no ties; the policy kernel's own tie test did kill its twin).  A bank of the five tie
    variants, 33 worlds each, the last segment cut; every tie class is hit on these inputs (asserted on the CPU)."""
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.qpolicy import QNetwork
    variants, seg = ("plain", "tie01", "tie01_top", "tie12", "tie012"), 33
    n = len(variants) * seg - 5
    x = np.concatenate([B.segment_inputs(seg, 60 + p) for p in range(len(variants))])[:n]
    nets = [_tie_layers(v) for v in variants]
    q = np.concatenate([B.int_eval(nets[p], x[p * seg:(p + 1) * seg]) for p in range(len(variants))])
    want = np.argmax(q, axis=1).astype(np.uint8)
    top = q.max(axis=1)
    tied = lambda a, b: (q[:, a] == top) & (q[:, b] == top)       # noqa: E731
    assert (tied(0, 1) & (q[:, 2] < top)).sum() > 20 and (tied(1, 2) & (q[:, 0] < top)).sum() > 5 and (tied(0, 1) & tied(1, 2)).sum() > 20
    assert ((q[:, 0] == q[:, 1]) & (q[:, 2] > q[:, 0])).sum() > 5   # ... and a tie below the maximum, which decides nothing
    ld = n + 37
    buf = torch.full((5, ld), 1.0e30, dtype=torch.float32, device=DEV)
    buf[:, :n] = torch.as_tensor(x.T.astype(np.float32))
    a, qd, qt = B.outputs(torch, ld)
    QNetworkBank(nets, seg, DEV).act(buf, n=n, out=a, q=qd, q_taken=qt)
    ak, qk, qtk = a.cpu().numpy(), qd.cpu().numpy(), qt.cpu().numpy()
    assert np.array_equal(qk[:, :n], q.T.astype(np.float32)) and B.untouched(ak, qk, qtk, n)
    assert np.array_equal(ak[:n], want), np.flatnonzero(ak[:n] != want)[:8]
    for p, layers in enumerate(nets):                              # the policy kernel, segment by segment
        lo, hi = p * seg, min((p + 1) * seg, n)
        got = QNetwork(layers, DEV).act(buf[:, lo:], n=hi - lo)
        assert np.array_equal(got.cpu().numpy(), want[lo:hi]), variants[p]


@pytest.mark.parametrize("once", [False, True], ids=["every", "once"])
@pytest.mark.parametrize("n", [33, 4099])
def test_a_world_at_time_zero_counts(torch, n, once):
    """include/aqua_episodes.h: a world counts iff term != 0 or time >= 0.  tests/_episodes.py::make_stream never holds time
    == 0 on a step without an end (its clocks start at 1), so `time > 0` survived the earlier suite.  Here every time class
    (0, positive, the four markers) meets every code, bit for bit against the numpy model, over three steps."""
    rng = np.random.RandomState(n)
    steps = 3
    time = rng.choice(np.array([0, 0, 1, 17, -1, -2, -3, -4], dtype=np.int32), (steps, n))
    term = (rng.randint(1, 4, (steps, n)) * (rng.rand(steps, n) < 0.3)).astype(np.uint8)
    reward = rng.uniform(-1, 1, (steps, n)).astype(np.float32)
    assert ((time == 0) & (term == 0)).sum() >= 5 and ((time < 0) & (term == 0)).sum() >= 5 and ((time == 0) & (term != 0)).sum() >= 1
    eps = (1.0, 0.05, 0.9997)
    model, dev = E.Model(n, n, once=once, eps=eps), E.Device(torch, n, n, once=once, eps=eps)
    for t in range(steps):
        model.after_step(reward[t], term[t], time[t], env_offset=OFFSET)
        dev.after_step(torch.as_tensor(reward[t]).to(DEV), torch.as_tensor(term[t]).to(DEV), torch.as_tensor(time[t]).to(DEV), env_offset=OFFSET)
        assert dev.differences(model) == [], t


@pytest.mark.parametrize("strategy", L.STRATEGIES)
@pytest.mark.parametrize("B_", [33, 97])
def test_the_td_error_is_formed_in_double(torch, B_, strategy):
    """include/aqua_learner.h: layer 3, y and delta = Q(s)[a] - y are double, rounded ONCE, to delta.  A kernel that rounds
    Q(s)[a] and y to float32 and then subtracts survived the earlier suite at every B and in every case (the 4 E_g bar of
    tests/test_learner_gpu.py does not see it; profiles/LOG.md).  Here the two are integers of 2^33 that differ by the reward:
    an integer network whose second hidden layer sits at 2^20 (+ small integers, exact in the float32 MFMA) under a last layer
    of 1024 / 1026, s' = s, a = arg-max Q(s), gamma = 1, no terminal slot, target = online network -- so that under every
    strategy y = r + Q(s)[a] and delta = -r EXACTLY in double, while float32(Q_a) - float32(y) is a multiple of 1024.
    With delta = -r every gradient sum below the last layer's kernel is a small integer: those 4547 elements are compared
    bit for bit with the int64 result times float32(2 / n).  dk2 = sum_b relu(h2) delta_b has terms of 2^21 and rounds: any
    float32 summation order of n terms stays within n U of the sum of |terms|."""
    from aquaticgymenv_amd.learner import DQNLearner
    from aquaticgymenv_amd.qpolicy import QNetwork
    cap, size = 300, 257
    (k0, b0), (k1, b1), (k2, b2) = L.int_layers("plain")
    layers = [(k0, b0), (k1, (b1 + np.float32(2 ** 20)).astype(np.float32)), ((1025 * np.abs(k2) + k2).astype(np.float32), b2)]
    theta = L.flatten(layers)
    ring = L.int_ring(cap, size, 3, bad_ok=0.1)
    ring["s2"][:, :size] = ring["s"][:, :size]
    ring["d"][:] = 0
    q_all = L.forward(theta.astype(np.float64), ring["s"][:, :size].T.astype(np.float64))[2]
    assert np.abs(q_all).max() < 2 ** 52 and ((q_all == q_all.max(axis=1, keepdims=True)).sum(axis=1) == 1).all()
    ring["a"][:size] = np.argmax(q_all, axis=1)
    idx = np.random.RandomState(B_).randint(0, size, B_).astype(np.int32)
    eff = L.effective(idx, ring)
    ref = L.gradient(theta, theta, ring, eff, 1.0, strategy, np.float64)
    x, a, r, x2, done = L.batch_of(ring, eff, np.float64)
    n = ref["n"]
    h1, h2, q = L.forward(theta.astype(np.float64), x)
    qa = q[np.arange(n), a]
    # -- the construction does what it says, on the CPU
    assert 0.7 * B_ < n <= B_ and not done.any() and np.array_equal(ref["delta"], -r) and (r != 0).sum() > n // 2
    assert np.abs(qa).min() > 2.0 ** 32 and (h2 > 2 ** 19).all() and np.abs(h2).max() < 2 ** 24 and np.abs(h1).max() < 2 ** 24
    rounded_first = qa.astype(np.float32).astype(np.float64) - (qa + r).astype(np.float32).astype(np.float64)
    assert (rounded_first[r != 0] != -r[r != 0]).all()                                   # the float32 form is wrong on EVERY sample with a reward
    ak1, ak2 = np.abs(k1).astype(np.float64), np.abs(layers[2][0]).astype(np.float64)
    adq = np.zeros((n, 3))
    adq[np.arange(n), a] = np.abs(r)
    adh2 = adq @ ak2.T
    adh1 = adh2 @ ak1.T
    exact = slice(0, 5 * 64 + 64 + 64 * 64 + 64)                                        # k0, b0, k1, b1
    sums = L.flatten([(np.abs(x).T @ adh1, adh1.sum(axis=0)), (np.maximum(h1, 0).T @ adh2, adh2.sum(axis=0)), (np.maximum(h2, 0).T @ adq, adq.sum(axis=0))])
    assert sums[exact].max() < 2 ** 24 and sums[-3:].max() < 2 ** 24 and adh1.max() < 2 ** 24
    S = ref["S"]
    assert np.array_equal(S, np.rint(S)) and np.array_equal(S.astype(np.float32).astype(np.float64)[exact], S[exact])
    # -- the kernel
    lrn = DQNLearner(QNetwork(layers, DEV), gamma=1.0, strategy=strategy)
    out = torch.zeros(B_, dtype=torch.int32, device=DEV)
    lrn.update(L.DeviceRing(torch, ring, DEV), B_, idx=torch.as_tensor(idx).to(DEV), idx_out=out)
    torch.cuda.synchronize()
    grad = lrn.grad.cpu().numpy()
    assert np.array_equal(out.cpu().numpy(), eff)
    scale = np.float32(2.0 / n)
    want = S.astype(np.float32) * scale
    for name, part in (("k0, b0, k1, b1", exact), ("b2", slice(L.PARAMS - 3, L.PARAMS))):
        bad = np.flatnonzero(grad[part].view(np.uint32) != want[part].view(np.uint32))
        assert bad.size == 0, (name, bad[:8], grad[part][bad[:8]], want[part][bad[:8]])
    dk2 = slice(exact.stop, L.PARAMS - 3)
    err = np.abs(grad[dk2].astype(np.float64) - S[dk2] * (2.0 / n))
    assert bool((err <= (n + 2) * U * sums[dk2] * (2.0 / n)).all()), float(np.max(err / (U * sums[dk2] * (2.0 / n) + 1e-300)))
    assert np.count_nonzero(want[exact]) > 500
    want_loss = float((r * r).sum() / n)
    assert abs(float(lrn.loss.cpu()[0]) - want_loss) <= 4 * U * want_loss


# ------------------------------------------------------------------------------------------------ Adam where epsilon decides
U = 2.0 ** -24
V_GRID = (0.0, 1e-18, 1e-16, 1e-14, 1e-12, 1e-8, 1e-4, 1e-2)
M_GRID = (1e-9, -1e-6, 1e-3, -1e-1, -1e-9, 1e-6, -1e-3, 1e-1)
ZERO_GRAD = slice(4 * 64, 5 * 64)         # k0[4][:]: the weights of the fifth input


@pytest.mark.parametrize("t0", [0, 999])
def test_adam_where_epsilon_decides_the_step(torch, t0):
    """The 64 weights of the fifth input see a gradient of exactly 0 when that input row of the ring is 0, so their Adam step
    is lr_t beta1 m / (sqrt(beta2 v) + eps) with m and v free to choose: a grid of eight v (sqrt(beta2 v) from 0 through
    eps = 1e-7 to 0.1) times eight m (both signs, 1e-9 .. 1e-1).  At v = 0 the step is lr_t beta1 m / eps: dropping eps makes
    it infinite, eps = 1e-8 ten times larger, sqrt(v + eps) 3162 times smaller.

    Bound |theta - theta64| <= U (|theta64| + 4 |step64|), U = 2^-24, theta64 from tests/_learner.py::adam64.  The kernel
    evaluates the same float64 formula from the same float32 state with two float32 roundings: lr_t (relative U, so the step
    moves by at most U |step|; adam64 keeps lr_t in double) and the stored theta (at most U |theta| -- half an ulp is
    U/2 .. U of the value).  Together U (|theta64| + |step64|) plus second-order terms; 4 leaves room for the double
    arithmetic's own rounding and is not a measurement.  Measured on one MI355X, (|d| - U |theta64|) / (U |step64|) at its
    worst over the 64 weights: 0.29 at t0 = 0 and 0.50 at t0 = 999, so the 4 stands (steps from 2.8e-12 to 7.2e+02).
    m and v after the step are beta1 m and beta2 v exactly in double, rounded once to float32: 3 U relative."""
    from aquaticgymenv_amd.learner import DQNLearner
    from aquaticgymenv_amd.qpolicy import QNetwork
    ring = L.float_ring(1024, 1000, 17)
    ring["s"][4] = 0.0
    dring = L.DeviceRing(torch, ring, DEV)
    x32 = ring["s"][:, :ring["size"]].T.copy()
    layers, target = L.random_layers(2, x32), L.random_layers(12, x32)
    lr, tau = 1e-3, 0.005
    lrn = DQNLearner(QNetwork(layers, DEV), lr=lr, tau=tau)
    rng = np.random.RandomState(t0)
    m, v = 0.1 * rng.randn(L.PARAMS), 0.01 * rng.rand(L.PARAMS)
    vg, mg = np.meshgrid(np.array(V_GRID), np.array(M_GRID), indexing="ij")
    m[ZERO_GRAD], v[ZERO_GRAD] = mg.reshape(-1), vg.reshape(-1)
    for name, value in (("theta_target", L.flatten(target)), ("m", m), ("v", v)):
        getattr(lrn, name).copy_(torch.as_tensor(np.asarray(value, dtype=np.float32)))
    lrn.t.fill_(t0)
    torch.cuda.synchronize()
    before = {name: getattr(lrn, name).cpu().numpy().copy() for name in ("theta", "theta_target", "m", "v")}
    lrn.update(dring, 97, idx=torch.as_tensor(rng.randint(0, ring["size"], 97).astype(np.int32)).to(DEV))
    torch.cuda.synchronize()
    after = {name: getattr(lrn, name).cpu().numpy().copy() for name in ("theta", "m", "v", "grad")}
    assert int(lrn.t[0]) == t0 + 1
    g = after["grad"]
    assert not g[ZERO_GRAD].any() and np.count_nonzero(g) > 2000      # the 64 see no gradient; most of the rest does (dead units: none)
    th64, m64, v64, _ = L.adam64(before["theta"], before["theta_target"], before["m"], before["v"], t0, g, lr, tau)
    sl = ZERO_GRAD
    theta0 = before["theta"][sl].astype(np.float64)
    # step64 from the formula, not as th64 - theta (a step of 1e-12 next to a theta of 1 would lose its digits there); adam64
    # agrees with it to float64 rounding.  Every step is finite and non-zero
    lr_t = lr * np.sqrt(1.0 - L.BETA2 ** (t0 + 1)) / (1.0 - L.BETA1 ** (t0 + 1))
    step64 = -lr_t * L.BETA1 * before["m"][sl].astype(np.float64) / (np.sqrt(L.BETA2 * before["v"][sl].astype(np.float64)) + L.EPS)
    assert bool((np.abs(th64[sl] - (theta0 + step64)) <= 2.0 ** -50 * (np.abs(theta0) + np.abs(step64))).all())
    assert np.isfinite(step64).all() and (step64 != 0).all()
    # the grid does what it is for: eps decides at small v, not at large v
    root = np.sqrt(L.BETA2 * before["v"][sl].astype(np.float64))
    assert (root[:8] == 0).all() and root[8:].min() > 0 and (root < L.EPS).sum() >= 16 and (root > 100 * L.EPS).sum() >= 24
    err = np.abs(after["theta"][sl].astype(np.float64) - th64[sl])
    bar = U * (np.abs(th64[sl]) + 4 * np.abs(step64))
    worst = float(np.max((err - U * np.abs(th64[sl])) / (U * np.abs(step64))))
    print("t0 %d: worst (|d| - U |theta64|) / (U |step64|) = %.3f of the 4 allowed; largest |step64| %.3e, smallest %.3e"
          % (t0, worst, np.abs(step64).max(), np.abs(step64).min()))
    bad = np.flatnonzero(err > bar)
    assert bad.size == 0, (bad[:8], after["theta"][sl][bad[:8]], th64[sl][bad[:8]], before["m"][sl][bad[:8]], before["v"][sl][bad[:8]])
    a = lambda z: np.abs(np.asarray(z, dtype=np.float64))                                # noqa: E731
    assert bool((a(after["m"][sl] - L.BETA1 * before["m"][sl].astype(np.float64)) <= 3 * U * L.BETA1 * a(before["m"][sl])).all())
    assert bool((a(after["v"][sl] - L.BETA2 * before["v"][sl].astype(np.float64)) <= 3 * U * L.BETA2 * a(before["v"][sl])).all())
    assert np.array_equal(m64[sl], L.BETA1 * before["m"][sl].astype(np.float64))
    # the rest of the vector: the bound of tests/test_learner_gpu.py::_check_step, unchanged
    rest = np.ones(L.PARAMS, dtype=bool)
    rest[sl] = False
    assert bool((a(after["theta"] - th64)[rest] <= U * (a(th64) + 64 * lr)[rest]).all())
