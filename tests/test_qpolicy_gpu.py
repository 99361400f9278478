"""GPU tests of the Q-network on the device (libaqua_policy.so, aquaticgymenv_amd/qpolicy.py, BatchedAqua's network
policy paths).

Numerics contract.  Reference: the network in float64 numpy from the float32 weights and the float32 network input
(q64).  Yardstick: the float32 numpy evaluation of the same thing on the same batch, E = max |q32 - q64|, recomputed by
every test.  The kernel is another float32 evaluation with another summation order: max |q_kernel - q64| <= 4 E.
Actions equal argmax q64 wherever the top-two gap of q64 exceeds 8 E; worlds inside the gap must still pick an action
within 8 E of the maximum, and their share (computed from q64 alone, asserted BEFORE the kernel's output is looked at)
is at most 0.25 % of the batch.
"""
import os

import numpy as np
import pytest

from tests._golden import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GAP_CAP = 0.0025


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _fixture_layers(tag):
    z = np.load(os.path.join(GOLDEN, "dqn_policies.npz"))
    return [(z["%s_kernel%d" % (tag, i)], z["%s_bias%d" % (tag, i)]) for i in range(3)]


def _eval(layers, x32, dtype):
    x = x32.astype(dtype)
    for li, (k, b) in enumerate(layers):
        x = x @ k.astype(dtype) + b.astype(dtype)
        if li < 2:
            x = np.maximum(x, 0)
    return x


def _reference(layers, x32):
    """x32 float32 [N][5] -> (q64 [N][3], E)"""
    q64 = _eval(layers, x32, np.float64)
    q32 = _eval(layers, x32, np.float32)
    assert q32.dtype == np.float32
    return q64, float(np.max(np.abs(q32.astype(np.float64) - q64)))


def _random_layers(seed, x32):
    """N(0, 1) weights, biases of both signs; the last bias is minus each Q column's batch mean (float64, rounded to
    float32) so that no action wins nearly everywhere"""
    rng = np.random.RandomState(seed)
    layers = [(rng.randn(a, b).astype(np.float32), rng.randn(b).astype(np.float32)) for a, b in ((5, 64), (64, 64), (64, 3))]
    assert all((b > 0).any() and (b < 0).any() for _, b in layers[:2])
    layers[2] = (layers[2][0], np.zeros(3, dtype=np.float32))
    q = _eval(layers, x32, np.float64)
    layers[2] = (layers[2][0], (-q.mean(axis=0)).astype(np.float32))
    return layers


def _check_against_reference(layers, x32, q_kernel, action, what):
    """q_kernel float32 [3][N], action uint8 [N] against the contract of the module docstring"""
    q64, E = _reference(layers, x32)
    n = x32.shape[0]
    top = np.sort(q64, axis=1)
    gap = top[:, 2] - top[:, 1]
    close = gap <= 8 * E
    share = close.mean()
    print("%s: N %d  E %.3e  near-tie share %.4f %%" % (what, n, E, 100 * share))
    assert share <= GAP_CAP, "%s: %.4f %% of the batch lies within 8 E of a tie" % (what, 100 * share)
    # -- only now the kernel's output
    err = float(np.max(np.abs(q_kernel.T.astype(np.float64) - q64)))
    print("%s: max |q_kernel - q64| %.3e = %.2f E" % (what, err, err / E))
    assert err <= 4 * E, "%s: max |q - q64| %.3e > 4 E = %.3e" % (what, err, 4 * E)
    want = np.argmax(q64, axis=1)
    assert np.array_equal(action[~close], want[~close]), what
    assert bool((action <= 2).all())
    picked = q64[np.arange(n), action.astype(np.int64)]
    assert bool((picked >= q64.max(axis=1) - 8 * E).all()), what
    return q64, E


def _tables(presets, n, seed=7):
    rng = np.random.RandomState(seed)
    tables = np.repeat(presets.BENCH8[None], n, axis=0).astype(np.float64)
    tables[:, :, 0:2] += rng.uniform(-3, 3, (n, 8, 2))
    return tables


# ------------------------------------------------------------------------------------------------ (a) exact layout
def _int_layers(variant="plain"):
    i5, i64, i3 = np.arange(5)[:, None], np.arange(64)[:, None], np.arange(3)[None, :]
    j64 = np.arange(64)[None, :]
    k0 = ((2 * i5 + 3 * j64) % 7 - 3).astype(np.float32)
    k1 = ((3 * i64 + 5 * j64) % 7 - 3).astype(np.float32)
    k2 = ((5 * i64 + 3 * i3 + (i64 // 7) * i3) % 7 - 3).astype(np.float32)
    b0 = ((np.arange(64) * 3) % 7 - 3).astype(np.float32)
    b1 = ((np.arange(64) * 5 + 1) % 7 - 3).astype(np.float32)
    b2 = np.array([2, -3, 1], dtype=np.float32)
    if variant == "tie01":            # Q0 == Q1 everywhere, Q2 above or below depending on the row
        k2[:, 1], b2[1] = k2[:, 0], b2[0]
    elif variant == "tie12":          # Q1 == Q2 everywhere
        k2[:, 2], b2[2] = k2[:, 1], b2[1]
    elif variant == "tie012":         # all three equal
        k2[:, 1], k2[:, 2], b2[1], b2[2] = k2[:, 0], k2[:, 0], b2[0], b2[0]
    return [(k0, b0), (k1, b1), (k2, b2)]


def _int_eval(layers, x):
    (k0, b0), (k1, b1), (k2, b2) = [(k.astype(np.int64), b.astype(np.int64)) for k, b in layers]
    h = np.maximum(x.astype(np.int64) @ k0 + b0, 0)
    assert np.abs(h).max() < 2 ** 24
    h2 = np.maximum(h @ k1 + b1, 0)
    # every partial sum of every unit is below 2^24 in magnitude: sum of |terms| bounds them all
    assert (h @ np.abs(k1) + np.abs(b1)).max() < 2 ** 24 and (h2 @ np.abs(k2) + np.abs(b2)).max() < 2 ** 24
    return h2 @ k2 + b2


@pytest.mark.parametrize("variant", ["plain", "tie01", "tie12", "tie012"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 4099])
def test_exact_integer_network_every_tail(torch, n, variant):
    """weights, biases and inputs are small integers: every product and partial sum is exact in float32, so q must equal
    the int64 result EXACTLY whatever the summation order -- a wrong k permutation, a row / column swap or a bias on the
    wrong unit cannot pass.  Ragged tails around the 32-world tile, ld > N, guard values behind N untouched; networks whose
    outputs tie exactly (two equal maxima, three equal) give the lowest index."""
    from aquaticgymenv_amd.qpolicy import QNetwork
    layers = _int_layers(variant)
    qnet = QNetwork(layers, DEV)
    ld = n + 37
    rng = np.random.RandomState(n)
    x = rng.randint(0, 4, size=(n, 5))
    x[0] = 0                                              # a row that sees the biases alone
    buf = torch.full((5, ld), 1.0e30, dtype=torch.float32, device=DEV)
    buf[:, :n] = torch.as_tensor(x.T.astype(np.float32))
    act = torch.full((ld,), 0xEE, dtype=torch.uint8, device=DEV)
    q = torch.full((3, ld), -777.0, dtype=torch.float32, device=DEV)
    qt = torch.full((ld,), -777.0, dtype=torch.float32, device=DEV)
    got = qnet.act(buf, n=n, out=act, q=q, q_taken=qt)
    torch.cuda.synchronize()
    want = _int_eval(layers, x)
    assert np.abs(want).max() < 2 ** 24
    qk = q.cpu().numpy()
    assert np.array_equal(qk[:, :n].astype(np.int64), want.T) and np.array_equal(qk[:, :n], want.T.astype(np.float32))
    a = act.cpu().numpy()
    assert np.array_equal(a[:n], np.argmax(want, axis=1).astype(np.uint8))       # np.argmax: the lowest index on a tie
    assert got.data_ptr() == act.data_ptr() and got.shape == (n,)
    assert np.array_equal(qt.cpu().numpy()[:n], want[np.arange(n), a[:n].astype(np.int64)].astype(np.float32))
    assert bool((a[n:] == 0xEE).all()) and bool((qk[:, n:] == -777.0).all()) and bool((qt.cpu().numpy()[n:] == -777.0).all())
    if variant == "tie012":
        assert bool((a[:n] == 0).all())
    elif variant == "tie01":
        assert not bool((a[:n] == 1).any())
    elif variant == "tie12":
        assert not bool((a[:n] == 2).any())
    # q alone (the TD-target path) gives the same bits
    assert torch.equal(qnet.q_values(buf, n=n), q[:, :n])


def test_exact_ties_are_hit():
    """the tie networks above really produce rows whose MAXIMUM is shared (not only equal losers)"""
    rng = np.random.RandomState(4099)
    x = rng.randint(0, 4, size=(4099, 5))
    for variant, cols in (("tie01", (0, 1)), ("tie12", (1, 2)), ("tie012", (0, 1, 2))):
        q = _int_eval(_int_layers(variant), x)
        shared = np.all(q[:, list(cols)] == q.max(axis=1, keepdims=True), axis=1)
        assert shared.sum() > 100, (variant, int(shared.sum()))


# ------------------------------------------------------------------------------------------------ (b) the contract
@pytest.mark.parametrize("n", [262144, 4099])
@pytest.mark.parametrize("net", ["no_obs", "with_obs", "random1", "random2", "random3"])
def test_q_values_and_actions_against_float64(torch, net, n):
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.qpolicy import QNetwork
    env = BatchedAqua(n, obstacles=presets.BENCH8, seed=1234, auto_reset="same_step", normalized_obs=True, device=DEV)
    env.reset()
    for _ in range(20):
        env.step(sample_actions=True)
    torch.cuda.synchronize()
    x32 = env.obs_norm_buf[:, :n].cpu().numpy().T.copy()
    assert x32.dtype == np.float32
    layers = _fixture_layers(net) if not net.startswith("random") else _random_layers(int(net[-1]), x32)
    if net.startswith("random"):
        wins = np.bincount(np.argmax(_eval(layers, x32, np.float64), axis=1), minlength=3) / float(n)
        assert wins.min() >= 0.10, wins
    qnet = QNetwork(layers, DEV)
    outs = {}
    for form in ("raw", "normalised", "buffer"):
        a = torch.full((env.ld,), 0xEE, dtype=torch.uint8, device=DEV)
        q = torch.full((3, env.ld), -777.0, dtype=torch.float32, device=DEV)
        qt = torch.full((env.ld,), -777.0, dtype=torch.float32, device=DEV)
        if form == "buffer":
            qnet.act(env.obs_norm_buf, n=n, out=a, q=q, q_taken=qt)
        else:
            qnet.act(env, normalised=(form == "normalised"), out=a, q=q, q_taken=qt)
        outs[form] = (a, q, qt)
    torch.cuda.synchronize()
    a, q, qt = outs["raw"]
    for form in ("normalised", "buffer"):                  # bit for bit, q and action
        assert torch.equal(outs[form][0], a) and torch.equal(outs[form][1], q) and torch.equal(outs[form][2], qt), form
    assert bool((a[n:] == 0xEE).all()) and bool((q[:, n:] == -777.0).all()) and bool((qt[n:] == -777.0).all())
    ak, qk = a[:n].cpu().numpy(), q[:, :n].cpu().numpy()
    _check_against_reference(layers, x32, qk, ak, "%s/%d" % (net, n))
    assert np.array_equal(qt[:n].cpu().numpy(), qk[ak.astype(np.int64), np.arange(n)])        # exactly


# ------------------------------------------------------------------------------------------------ (c) epsilon-greedy
def test_epsilon_greedy_draws_match_philox(torch, oracle):
    from aquaticgymenv_amd.qpolicy import QNetwork
    n, off, seed = 4096, 3 << 20, 0x1234567890ABCDEF
    layers = _fixture_layers("with_obs")
    qnet = QNetwork(layers, DEV)
    g = torch.Generator(device=DEV).manual_seed(11)
    buf = torch.rand((5, n), device=DEV, generator=g)
    greedy = qnet.act(buf).clone()
    q_all = qnet.q_values(buf).clone()
    for tick in (0, 7, (1 << 32) + 5):
        c3 = ((tick >> 32) & 0xFFFF) | (5 << 24)
        r = np.array([oracle.philox((seed & 0xFFFFFFFF, seed >> 32), ((off + i) & 0xFFFFFFFF, (off + i) >> 32, tick & 0xFFFFFFFF, c3))
                      for i in range(n)], dtype=np.uint64)
        u = (r[:, 0] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
        explore_action = (((r[:, 1] >> np.uint64(8)) * np.uint64(3)) >> np.uint64(24)).astype(np.uint8)
        for eps in (0.0, 0.1, 0.5, 1.0):
            qt = torch.zeros(n, dtype=torch.float32, device=DEV)
            got = qnet.act(buf, epsilon=eps, env_offset=off, seed=seed, tick=tick, q_taken=qt)
            explore = u < np.float32(eps)
            want = np.where(explore, explore_action, greedy.cpu().numpy())
            assert np.array_equal(got.cpu().numpy(), want), (tick, eps)
            assert torch.equal(qt, q_all.gather(0, got.to(torch.int64).unsqueeze(0)).squeeze(0))
            if eps == 0.0:
                assert torch.equal(got, greedy)
            if eps == 1.0:
                assert explore.all()
            if eps in (0.1, 0.5):
                assert abs(explore.mean() - eps) < 5 * np.sqrt(eps * (1 - eps) / n)
            # two halves launched with their own env_offset equal the whole
            halves = torch.empty(n, dtype=torch.uint8, device=DEV)
            h = n // 2
            qnet.act(buf[:, :h], epsilon=eps, env_offset=off, seed=seed, tick=tick, out=halves[:h], n=h)
            qnet.act(buf[:, h:], epsilon=eps, env_offset=off + h, seed=seed, tick=tick, out=halves[h:], n=n - h)
            assert torch.equal(halves, got)
        assert bool((np.bincount(explore_action, minlength=3) > n // 4).all())
    # a device tick base b with tick t == tick t + b without one
    base = torch.tensor([(1 << 32) + 2], dtype=torch.int64, device=DEV)
    with_base = qnet.act(buf, epsilon=0.5, env_offset=off, seed=seed, tick=3, tick_base=base)
    plain = qnet.act(buf, epsilon=0.5, env_offset=off, seed=seed, tick=(1 << 32) + 5)
    other = qnet.act(buf, epsilon=0.5, env_offset=off, seed=seed, tick=3)
    assert torch.equal(with_base, plain) and not torch.equal(with_base, other)
    with pytest.raises(ValueError):
        qnet.act(buf, epsilon=-0.1)
    with pytest.raises(ValueError):
        qnet.act(buf, epsilon=float("nan"))


# ------------------------------------------------------------------------------------------------ (d) in the loop
def _twin(torch, presets, n, mode, per_world, seed=31):
    from aquaticgymenv_amd.batched import BatchedAqua
    obstacles = _tables(presets, n) if per_world else presets.BENCH8
    envs = [BatchedAqua(n, obstacles=obstacles, seed=seed, auto_reset=mode, env_offset=1000, device=DEV) for _ in range(2)]
    for e in envs:
        e.reset()
    return envs


def _same(torch, a, b):
    return (torch.equal(a.state, b.state) and torch.equal(a.reward, b.reward) and torch.equal(a.term, b.term)
            and torch.equal(a.done_bits, b.done_bits) and torch.equal(a.time, b.time))


@pytest.mark.parametrize("eps", [0.0, 0.2])
@pytest.mark.parametrize("per_world", [False, True], ids=["shared", "tables"])
@pytest.mark.parametrize("mode", [False, "same_step", "next_step"])
def test_step_with_network_policy_equals_act_then_step(torch, mode, per_world, eps):
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.qpolicy import QNetwork
    n = 5000 + 13
    qnet = QNetwork(_fixture_layers("with_obs"), DEV)
    a, b = _twin(torch, presets, n, mode, per_world)
    act = torch.zeros(n, dtype=torch.uint8, device=DEV)
    seen = set()
    for it in range(60):
        a.step(policy=qnet, epsilon=eps)
        qnet.act(b, out=act, epsilon=eps)
        b.step(act)
        assert _same(torch, a, b), it
        assert torch.equal(a.policy_action[:n], act), it
        seen.update(int(v) for v in torch.unique(act).cpu())
    assert seen == {0, 1, 2}
    # rollout(actions=qnet): the same 60 steps from here, outputs of every step kept
    reward, term = a.rollout(60, actions=qnet, epsilon=eps, keep_all=True)
    for it in range(60):
        qnet.act(b, out=act, epsilon=eps)
        b.step(act)
        assert torch.equal(reward[it, :n], b.reward[:n]) and torch.equal(term[it, :n], b.term[:n]), it
    # (keep_all=True wrote the per-step outputs into the [T][ld] tensors, not into the batch's own reward / term buffers)
    assert torch.equal(a.state, b.state) and torch.equal(a.time, b.time) and torch.equal(a.done_bits, b.done_bits)
    assert a._tick == b._tick == 120
    with pytest.raises(ValueError):
        a.rollout(4, actions=qnet, fused=True)


def test_network_policy_rejects_continuous_worlds(torch):
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.qpolicy import QNetwork
    qnet = QNetwork(_fixture_layers("no_obs"), DEV)
    env = BatchedAqua(256, obstacles=presets.BENCH8, seed=1, continuous=True, device=DEV)
    env.reset()
    with pytest.raises(ValueError):
        env.step(policy=qnet)
    with pytest.raises(ValueError):
        env.rollout(3, actions=qnet)
    with pytest.raises(ValueError):
        env.capture_policy_step(qnet)
    with pytest.raises(ValueError):
        qnet.act(env)
    with pytest.raises(ValueError):
        QNetwork(_fixture_layers("no_obs")[:2], DEV)


# ------------------------------------------------------------------------------------------------ (e) one graph
@pytest.mark.parametrize("per_world", [False, True], ids=["shared", "tables"])
def test_captured_policy_step_replays_like_eager_steps(torch, per_world):
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.qpolicy import QNetwork
    n, eps = 5000 + 13, 0.2
    first, second = _fixture_layers("with_obs"), _fixture_layers("no_obs")
    qnet = QNetwork(first, DEV)
    a, b = _twin(torch, presets, n, "next_step", per_world)
    for e in (a, b):
        for _ in range(3):
            e.step(policy=qnet, epsilon=eps)              # the graph starts at a tick other than 0
    graph = a.capture_policy_step(qnet, epsilon=eps)
    for it in range(40):
        graph.launch()
        b.step(policy=qnet, epsilon=eps)
        assert _same(torch, a, b), it
        assert torch.equal(a.policy_action, b.policy_action), it
    assert a._tick == b._tick == 43
    # new weights into the same blob: the SAME graph acts with them
    old = QNetwork(first, DEV)
    qnet.load(second)
    would_old = old.act(a, epsilon=eps).clone()
    would_new = qnet.act(a, epsilon=eps).clone()
    assert int((would_old != would_new).sum()) > 10
    graph.launch()
    assert torch.equal(a.policy_action[:n], would_new)
    b.step(policy=qnet, epsilon=eps)
    assert _same(torch, a, b)
    for it in range(10):
        graph.launch()
        b.step(policy=qnet, epsilon=eps)
    assert _same(torch, a, b)
    graph.close()


# ------------------------------------------------------------------------------------------------ (f) published numbers
@pytest.mark.parametrize("tag,obstacles", [("no_obs", False), ("with_obs", True)])
def test_trained_policies_reach_the_published_success_rates_on_the_device_network(torch, tag, obstacles):
    """the loop of tests/test_hip_parity.py::test_trained_dqn_policies_reach_the_published_success_rates with the network
    evaluated by our own kernel (env.step(policy=qnet)) instead of torch's GEMMs: the same bars.  Trajectories are not
    compared world by world with the torch path: one flipped near-tie legitimately diverges an episode."""
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.qpolicy import QNetwork
    z = np.load(os.path.join(GOLDEN, "dqn_policies.npz"))
    n = 16384
    env = BatchedAqua(n, obstacles=obstacles, seed=9001, auto_reset=False, device=DEV)
    env.reset()
    qnet = QNetwork(_fixture_layers(tag), DEV)
    first = torch.zeros(n, dtype=torch.uint8, device=DEV)
    total = torch.zeros(n, dtype=torch.float32, device=DEV)
    for step in range(1001):
        obs, reward, term = env.step(policy=qnet)
        alive = first == 0
        total += torch.where(alive, reward, torch.zeros_like(reward))
        first = torch.where(alive, term, first)
        if step % 100 == 99 and int((first == 0).sum()) == 0:
            break
    assert int((first == 0).sum()) == 0
    success = float((first == 3).float().mean())
    reward_mean = float(total.mean())
    pub_s, pub_r = z["%s_published_success" % tag], z["%s_published_reward" % tag]
    sigma = np.sqrt(pub_s.mean() * (1 - pub_s.mean()) / pub_s.shape[0])
    print("%s: success %.4f (published %.4f), mean reward %.3f (published %.3f)" % (tag, success, pub_s.mean(), reward_mean, pub_r.mean()))
    assert abs(success - pub_s.mean()) < 4 * sigma + 0.01, "success %.4f vs published %.4f" % (success, pub_s.mean())
    sem = pub_r.std() / np.sqrt(pub_r.shape[0])
    assert abs(reward_mean - pub_r.mean()) < 4 * sem + 0.5, "mean reward %.3f vs published %.3f" % (reward_mean, pub_r.mean())


# ------------------------------------------------------------------------------------------------ (g) replay ring
def test_replay_ring_records_the_network_actions_and_q_values_of_its_contents(torch):
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.qpolicy import QNetwork
    from aquaticgymenv_amd.replay import ReplayRing
    n, steps = 3000 + 17, 6
    layers = _fixture_layers("with_obs")
    qnet = QNetwork(layers, DEV)
    env = BatchedAqua(n, obstacles=presets.BENCH8, seed=77, auto_reset="next_step", normalized_obs=True, device=DEV)
    env.reset()
    for _ in range(30):
        env.step(policy=qnet, epsilon=0.3)
    ring = ReplayRing(env, steps * n)
    expect = []
    for t in range(steps):
        s = env.obs_norm.clone()
        qnet.act(env, epsilon=0.3, out=env.policy_action)
        ring.before_step(env.policy_action)
        obs, reward, term = env.step(env.policy_action[:n])
        ring.after_step()
        expect.append((s, env.policy_action[:n].clone(), reward.clone(), env.obs_norm.clone(), term.clone()))
    torch.cuda.synchronize()
    assert ring.size == steps * n
    for t in range(steps):
        sl = slice(t * n, (t + 1) * n)
        s, a, r, s2, d = expect[t]
        assert torch.equal(ring.s[:, sl].t(), s) and torch.equal(ring.a[sl], a) and torch.equal(ring.r[sl], r)
        assert torch.equal(ring.s2[:, sl].t(), s2) and torch.equal(ring.d[sl], d)
    assert len(torch.unique(ring.a)) == 3
    for buf in (ring.s, ring.s2):
        q = qnet.q_values(buf, ring.size)
        x32 = buf[:, :ring.size].cpu().numpy().T.copy()
        q64, E = _reference(layers, x32)
        err = float(np.max(np.abs(q.cpu().numpy().T.astype(np.float64) - q64)))
        print("ring: max |q - q64| %.3e = %.2f E" % (err, err / E))
        assert err <= 4 * E
