"""GPU tests of episode accounting on the device (libaqua_episodes.so, aquaticgymenv_amd/episodes.py).

Everything is exact.  The reference is the numpy model of tests/_episodes.py (itself checked against a per-world loop in
tests/test_episodes_cpu.py): every buffer is compared with np.array_equal, returns as bit patterns -- a return is ONE
float32 add per step, the log order is a function of the inputs alone, the schedule uses float64 multiplications only, so
there is no tolerance to state.  The exploration pass is compared bit for bit with the policy kernel's own epsilon-greedy
mode and with the Philox model.
"""
import os
import types

import numpy as np
import pytest

from tests import _episodes as E
from tests._golden import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OFFSET = (5 << 32) + 12345              # a world index beyond 32 bits
T = 40


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _fixture_layers(tag):
    z = np.load(os.path.join(GOLDEN, "dqn_policies.npz"))
    return [(z["%s_kernel%d" % (tag, i)], z["%s_bias%d" % (tag, i)]) for i in range(3)]


def _upload(torch, reward, term, time):
    return (torch.from_numpy(reward).to(DEV), torch.from_numpy(term).to(DEV), None if time is None else torch.from_numpy(time).to(DEV))


def _as_device(tracker):
    """a tracker's tensors under the names E.Device.differences compares"""
    return types.SimpleNamespace(ret=tracker.ret, len=tracker.len, finished=tracker.finished, log_ret=tracker.log_ret,
                                 log_len=tracker.log_len, log_code=tracker.log_code, log_world=tracker.log_world,
                                 counts=tracker._counts, eps_state=tracker._eps_state, eps_out=tracker.epsilon)


def _equal(torch, a, b):
    """two trackers hold the same bits"""
    pairs = zip(vars(_as_device(a)).values(), vars(_as_device(b)).values())
    return all(torch.equal(x, y) for x, y in pairs if x is not None or y is not None)


def _differences(tracker, model):
    return E.Device.differences(_as_device(tracker), model)


# ------------------------------------------------------------------------------------------------ (a) exact against the model
@pytest.mark.parametrize("once", [False, True], ids=["every", "once"])
@pytest.mark.parametrize("markers", [False, True], ids=["notime", "markers"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1000, 4099])
def test_streams_match_the_model_bit_for_bit(torch, N, markers, once):
    eps = (1.0, 0.05, 0.9997)
    for p in (0.0, 0.02, 0.5, 1.0):
        reward, term, time = E.make_stream(N, T, p, seed=1000 * N + int(100 * p), markers=markers)
        d_reward, d_term, d_time = _upload(torch, reward, term, time)
        for C in (N, 4 * N):
            model, dev = E.Model(N, C, once=once, eps=eps), E.Device(torch, N, C, once=once, eps=eps)
            for t in range(T):
                model.after_step(reward[t], term[t], None if time is None else time[t], env_offset=OFFSET)
                dev.after_step(d_reward[t], d_term[t], None if d_time is None else d_time[t], env_offset=OFFSET)
                if N <= 65 or t % 13 == 5 or t == T - 1:
                    assert dev.differences(model) == [], (p, C, t)
            if p == 1.0 and not once and not markers:
                assert int(model.counts[0]) == N * T > C          # the log wrapped many times
            if p >= 0.5 and once:
                assert int(model.counts[0]) == N == int(model.finished.sum())
        if p > 0 and N >= 63:
            assert int(model.counts[0]) > 0


# ------------------------------------------------------------------------------------------------ (b) ordering
def test_worlds_ending_together_are_logged_by_ascending_index_and_halves_share_a_log(torch):
    N, C, h = 1000, 2500, 437
    rng = np.random.RandomState(2)
    reward = rng.uniform(-1, 1, (3, N)).astype(np.float32)
    term = np.zeros((3, N), dtype=np.uint8)
    term[1] = rng.randint(1, 4, N)                           # every world ends in the second step
    term[2, ::7] = 3
    d_reward, d_term, _ = _upload(torch, reward, term, None)
    model, dev = E.Model(N, C), E.Device(torch, N, C)
    for t in range(3):
        model.after_step(reward[t], term[t], env_offset=OFFSET)
        dev.after_step(d_reward[t], d_term[t], env_offset=OFFSET)
    assert dev.differences(model) == []
    got = dev.log_world.cpu().numpy()
    assert np.array_equal(got[:N], OFFSET + np.arange(N)) and np.array_equal(got[N:N + len(range(0, N, 7))], OFFSET + np.arange(0, N, 7))
    # two halves, two calls with their own env_offset, one log and one set of counters
    model, dev = E.Model(N, C), E.Device(torch, N, C)
    for t in range(3):
        for lo, hi in ((0, h), (h, N)):
            model.after_step(reward[t, lo:hi], term[t, lo:hi], env_offset=OFFSET + lo, lo=lo, hi=hi)
            dev.after_step(d_reward[t, lo:hi], d_term[t, lo:hi], env_offset=OFFSET + lo, lo=lo, hi=hi)
    assert dev.differences(model) == []
    assert np.array_equal(dev.log_world.cpu().numpy()[:N], OFFSET + np.arange(N))        # halves in order == the whole


# ------------------------------------------------------------------------------------------------ (c) the schedule
@pytest.mark.parametrize("decay", [0.9997, 0.5, 1.0])
def test_epsilon_schedule_matches_the_model_and_holds_its_floor(torch, decay):
    N, eps = 4099, (1.0, 0.05, decay)
    ending = [0, 1, 3000, 0, 3000, 3000, 3000, 3000, 1, 0]
    rng = np.random.RandomState(4)
    term = np.zeros((len(ending), N), dtype=np.uint8)
    for t, n in enumerate(ending):
        term[t, rng.permutation(N)[:n]] = rng.randint(1, 4, n)
    reward = rng.uniform(-1, 1, term.shape).astype(np.float32)
    d_reward, d_term, _ = _upload(torch, reward, term, None)
    model, dev = E.Model(N, N, eps=eps), E.Device(torch, N, N, eps=eps)
    seen = []
    for t, n in enumerate(ending):
        assert model.after_step(reward[t], term[t]) == n
        dev.after_step(d_reward[t], d_term[t])
        assert dev.differences(model) == [], t
        assert float(dev.eps_out.cpu()[0]) == float(np.float32(float(dev.eps_state.cpu()[0])))
        seen.append(model.eps_state)
    assert seen[0] == 1.0 and seen[1] == max(decay, 0.05)
    if decay == 1.0:
        assert seen == [1.0] * len(ending)
    else:
        assert seen[-4:] == [0.05] * 4 and all(a >= b for a, b in zip(seen, seen[1:]))      # the floor is reached and held
        assert (seen[2] > 0.05) == (decay == 0.9997)


# ------------------------------------------------------------------------------------------------ (d) exploration
def test_greedy_then_explore_equals_the_epsilon_greedy_kernel(torch, oracle):
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.qpolicy import QNetwork
    n, off, seed = 4096, 3 << 20, 0x1234567890ABCDEF
    qnet = QNetwork(_fixture_layers("with_obs"), DEV)
    g = torch.Generator(device=DEV).manual_seed(11)
    buf = torch.rand((5, n), device=DEV, generator=g)
    greedy = qnet.act(buf).clone()
    env = types.SimpleNamespace(torch=torch, device=torch.device(DEV), num_envs=n, env_offset=off, seed=seed, _tick=0,
                                continuous=False)
    tracker = EpisodeTracker(env)
    eps_dev = torch.zeros(1, dtype=torch.float32, device=DEV)
    for tick in (0, 7, (1 << 32) + 5):
        env._tick = tick
        explored_any = False
        u, drawn = E.draws(oracle, n, seed, off, tick)
        for eps in (0.0, 0.1, 0.5, 1.0):
            eps_dev.fill_(eps)
            want = qnet.act(buf, epsilon=eps, env_offset=off, seed=seed, tick=tick).clone()
            got = qnet.act(buf, epsilon=0.0).clone()
            assert torch.equal(got, greedy)
            out = tracker.explore(got, epsilon=eps_dev)
            assert out.data_ptr() == got.data_ptr() and torch.equal(got, want), (tick, eps)
            model, explored = E.explore(greedy.cpu().numpy(), eps, u, drawn)
            assert np.array_equal(got.cpu().numpy(), model), (tick, eps)
            assert explored.all() if eps == 1.0 else (not explored.any() if eps == 0.0 else 0 < explored.sum() < n)
            explored_any |= bool((got != greedy).any())
        assert explored_any
    # a device tick base b with tick t == tick t + b without one
    base = torch.tensor([(1 << 32) + 2], dtype=torch.int64, device=DEV)
    eps_dev.fill_(0.5)
    want = qnet.act(buf, epsilon=0.5, env_offset=off, seed=seed, tick=3, tick_base=base).clone()
    assert torch.equal(want, qnet.act(buf, epsilon=0.5, env_offset=off, seed=seed, tick=(1 << 32) + 5))
    got = greedy.clone()
    tracker.explore(got, tick=3, tick_base=base, epsilon=eps_dev)
    other = greedy.clone()
    tracker.explore(other, tick=3, epsilon=eps_dev)
    assert torch.equal(got, want) and not torch.equal(other, want)


def _twin(torch, n, mode, seed=31):
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.batched import BatchedAqua
    envs = [BatchedAqua(n, obstacles=presets.BENCH8, seed=seed, auto_reset=mode, env_offset=1000, device=DEV) for _ in range(2)]
    for e in envs:
        e.reset()
    return envs


def _same(torch, a, b):
    return (torch.equal(a.state, b.state) and torch.equal(a.reward, b.reward) and torch.equal(a.term, b.term)
            and torch.equal(a.done_bits, b.done_bits) and torch.equal(a.time, b.time))


@pytest.mark.parametrize("mode", [False, "same_step", "next_step"])
def test_explore_through_an_env_equals_the_epsilon_greedy_policy_on_a_twin(torch, mode):
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.qpolicy import QNetwork
    n = 1000 + 13
    qnet = QNetwork(_fixture_layers("with_obs"), DEV)
    a, b = _twin(torch, n, mode)
    tracker = EpisodeTracker(a, epsilon=(0.4, 0.05, 0.999))
    act_a = torch.zeros(n, dtype=torch.uint8, device=DEV)
    act_b = torch.zeros(n, dtype=torch.uint8, device=DEV)
    greedy_differs = 0
    for it in range(60):
        e = float(tracker.epsilon[0])
        qnet.act(a, epsilon=0.0, out=act_a)
        greedy_differs += int((qnet.act(b, epsilon=e, out=act_b) != act_a).sum())
        tracker.explore(act_a)
        assert torch.equal(act_a, act_b), it
        a.step(act_a)
        b.step(act_b)
        tracker.after_step()
        assert _same(torch, a, b), it
    assert greedy_differs > 60
    # the schedule moved iff an episode ended
    assert (tracker.counts()["episodes"] > 0) == (float(tracker.epsilon[0]) < float(np.float32(0.4)))


# ------------------------------------------------------------------------------------------------ (e) against a real loop
@pytest.fixture(scope="module")
def evaluation_loop(torch):
    """the loop of tests/test_qpolicy_gpu.py::test_trained_policies_reach_the_published_success_rates_on_the_device_network
    at n = 2048, the torch first / total bookkeeping and a tracker in once mode on the same steps"""
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.qpolicy import QNetwork
    n = 2048
    env = BatchedAqua(n, obstacles=True, seed=9001, auto_reset=False, env_offset=77, device=DEV)
    env.reset()
    qnet = QNetwork(_fixture_layers("with_obs"), DEV)
    tracker = EpisodeTracker(env, capacity=n, once=True)
    first = torch.zeros(n, dtype=torch.uint8, device=DEV)
    total = torch.zeros(n, dtype=torch.float32, device=DEV)
    when = torch.zeros(n, dtype=torch.int32, device=DEV)
    for step in range(1001):
        obs, reward, term = env.step(policy=qnet)
        tracker.after_step()
        alive = first == 0
        total += torch.where(alive, reward, torch.zeros_like(reward))
        when = torch.where(alive & (term != 0), torch.full_like(when, step + 1), when)
        first = torch.where(alive, term, first)
        if step % 100 == 99 and int((first == 0).sum()) == 0:
            break
    assert int((first == 0).sum()) == 0
    return dict(n=n, qnet=qnet, tracker=tracker, first=first.cpu().numpy(), total=total.cpu().numpy(), when=when.cpu().numpy(),
                offset=77)


def test_once_mode_equals_the_torch_bookkeeping_of_the_evaluation_loop(torch, evaluation_loop):
    L = evaluation_loop
    n, tracker = L["n"], L["tracker"]
    c = tracker.counts()
    assert c["episodes"] == n and c["collided"] + c["timeout"] + c["success"] == n and c["steps"] == int(L["when"].sum())
    assert c["success"] == int((L["first"] == 3).sum()) > n // 2
    rec = tracker.last(n)
    w = rec["world"] - L["offset"]
    assert np.array_equal(np.sort(w), np.arange(n))
    assert np.array_equal(rec["code"], L["first"][w])                                          # Code == first
    assert np.array_equal(rec["ret"].view(np.uint32), L["total"][w].view(np.uint32))           # Reward == total, bitwise
    assert np.array_equal(rec["len"], L["when"][w])                                            # Steps == step index + 1
    # the log is ordered by the step the episode ended in, then by world
    assert np.array_equal(np.lexsort((w, L["when"][w])), np.arange(n))
    assert bool((tracker.finished[:n] == 1).all()) and bool((tracker.ret == 0).all()) and bool((tracker.len == 0).all())
    assert len(tracker.last(5)["ret"]) == 5 and np.array_equal(tracker.last(5)["world"], rec["world"][-5:])


def test_evaluate_returns_the_arrays_of_the_evaluation_loop(torch, evaluation_loop):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import evaluate
    L = evaluation_loop
    env = BatchedAqua(L["n"], obstacles=True, seed=9001, auto_reset=False, env_offset=L["offset"], device=DEV)
    env.reset()
    out = evaluate(env, L["qnet"])
    assert np.array_equal(out["Code"], L["first"]) and np.array_equal(out["Success"], L["first"] == 3)
    assert np.array_equal(out["Reward"].view(np.uint32), L["total"].view(np.uint32)) and np.array_equal(out["Steps"], L["when"])
    assert out["Reward"].dtype == np.float32 and out["Success"].dtype == bool
    # cut short, the unfinished worlds report code 0 and what they have so far
    env = BatchedAqua(L["n"], obstacles=True, seed=9001, auto_reset=False, env_offset=L["offset"], device=DEV)
    env.reset()
    cut = int(np.median(L["when"]))
    part = evaluate(env, L["qnet"], max_steps=cut)
    done = L["when"] <= cut
    assert done.sum() > 0
    assert np.array_equal(part["Code"], np.where(done, L["first"], 0)) and np.array_equal(part["Steps"], np.where(done, L["when"], cut))
    assert np.array_equal(part["Reward"][done].view(np.uint32), L["total"][done].view(np.uint32))
    with pytest.raises(ValueError):
        evaluate(BatchedAqua(64, seed=1, auto_reset="next_step", device=DEV), L["qnet"])


@pytest.mark.parametrize("mode", ["next_step", "same_step"])
def test_restarting_batches_match_host_accounting_of_the_same_steps(torch, mode):
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.qpolicy import QNetwork
    n, eps = 1000, (1.0, 0.05, 0.999)
    env = BatchedAqua(n, obstacles=presets.BENCH8, seed=5, auto_reset=mode, env_offset=4000, device=DEV)
    env.reset()
    qnet = QNetwork(_fixture_layers("with_obs"), DEV)
    tracker = EpisodeTracker(env, capacity=n, epsilon=eps)
    model = E.Model(n, n, eps=eps)
    skipped = 0
    for step in range(300):
        env.step(policy=qnet, epsilon=0.1)
        tracker.after_step()
        reward, term, time = env.reward[:n].cpu().numpy(), env.term[:n].cpu().numpy(), env.time[:n].cpu().numpy()
        skipped += int(((term == 0) & (time < 0)).sum())
        model.after_step(reward, term, time, env_offset=4000)
        if step % 50 == 49:
            assert _differences(tracker, model) == [], step
    assert _differences(tracker, model) == []
    c = tracker.counts()
    assert c["episodes"] == int(model.counts[0]) > 0 and c["steps"] == 300 * n - skipped
    assert (skipped > 0) == (mode == "next_step")
    if mode == "next_step":
        assert skipped >= c["episodes"] - n                   # every restart costs a tick that belongs to no episode
    k = min(100, c["episodes"])
    rec = tracker.last(100)
    newest = np.arange(c["episodes"] - k, c["episodes"]) % n
    assert rec["ret"].shape == (k,) and np.array_equal(rec["world"], model.log_world[newest])
    assert np.array_equal(rec["ret"].view(np.uint32), model.log_ret[newest].view(np.uint32))


# ------------------------------------------------------------------------------------------------ (f) graphs, resuming
def test_captured_accounting_and_exploration_replay_like_eager_calls(torch):
    from aquaticgymenv_amd.episodes import EpisodeTracker
    N, steps, eps = 1000 + 7, 20, (0.9, 0.05, 0.99)
    reward, term, time = E.make_stream(N, steps, 0.1, seed=8, markers=True)
    d_reward, d_term, d_time = _upload(torch, reward, term, time)
    greedy = torch.from_numpy(np.random.RandomState(1).randint(0, 3, (steps, N)).astype(np.uint8)).to(DEV)

    def stub():
        return types.SimpleNamespace(torch=torch, device=torch.device(DEV), num_envs=N, env_offset=OFFSET, seed=99, _tick=0,
                                     continuous=False, reward=torch.zeros(N, dtype=torch.float32, device=DEV),
                                     term=torch.zeros(N, dtype=torch.uint8, device=DEV), time=torch.zeros(N, dtype=torch.int32, device=DEV))
    a, b = stub(), stub()
    ta, tb = EpisodeTracker(a, capacity=N, epsilon=eps), EpisodeTracker(b, capacity=N, epsilon=eps)
    act_a, act_b = torch.zeros(N, dtype=torch.uint8, device=DEV), torch.zeros(N, dtype=torch.uint8, device=DEV)
    base_a, base_b = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    tb.after_step()                                           # (every kernel has run once before the capture)
    tb.explore(act_b, tick_base=base_b)
    tb.reset_stats()
    assert tb.counts() == {"episodes": 0, "collided": 0, "timeout": 0, "success": 0, "steps": 0} and float(tb.epsilon[0]) == np.float32(0.9)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ta.explore(act_a, tick_base=base_a)
        ta.after_step()
    assert ta.counts()["steps"] == 0                          # captured, not run
    model = E.Model(N, N, eps=eps)
    for t in range(steps):
        for env, act, base in ((a, act_a, base_a), (b, act_b, base_b)):
            env.reward.copy_(d_reward[t]); env.term.copy_(d_term[t]); env.time.copy_(d_time[t]); act.copy_(greedy[t])
            base.fill_(t)
        graph.replay()
        tb.explore(act_b, tick_base=base_b)
        tb.after_step()
        model.after_step(reward[t], term[t], time[t], env_offset=OFFSET)
        assert torch.equal(act_a, act_b), t
        assert _equal(torch, ta, tb), t
    assert _differences(ta, model) == [] and int(model.counts[0]) > N // 2
    assert bool((act_a != greedy[-1]).any())                 # the replays explored


def test_state_dict_resumes_bit_for_bit_and_runs_repeat(torch):
    from aquaticgymenv_amd.episodes import EpisodeTracker
    N, eps = 513, (1.0, 0.05, 200)
    reward, term, time = E.make_stream(N, T, 0.2, seed=12, markers=True)
    d_reward, d_term, d_time = _upload(torch, reward, term, time)
    env = types.SimpleNamespace(torch=torch, device=torch.device(DEV), num_envs=N, env_offset=3, continuous=False)

    def run(tracker, lo, hi):
        for t in range(lo, hi):
            tracker.after_step(d_reward[t], d_term[t], d_time[t])
        return tracker
    whole = run(EpisodeTracker(env, capacity=N, once=False, epsilon=eps), 0, T)
    again = run(EpisodeTracker(env, capacity=N, once=False, epsilon=eps), 0, T)
    first = run(EpisodeTracker(env, capacity=N, once=False, epsilon=eps), 0, 13)
    state = first.state_dict()
    run(first, 13, 20)                                        # the saved state is a copy
    resumed = run(EpisodeTracker(env, capacity=N, once=False, epsilon=eps).load_state_dict(state), 13, T)
    assert _equal(torch, whole, again) and _equal(torch, whole, resumed) and not _equal(torch, whole, first)
    assert whole.decay == (0.05 / 1.0) ** (1 / 200) and whole.counts()["episodes"] > N
    model = E.Model(N, N, eps=(1.0, 0.05, whole.decay))
    for t in range(T):
        model.after_step(reward[t], term[t], time[t], env_offset=3)
    assert _differences(whole, model) == []
    with pytest.raises(ValueError):
        EpisodeTracker(env, capacity=N, once=True, epsilon=eps).load_state_dict(state)


def test_python_layer_rejections(torch):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import EpisodeTracker
    env = BatchedAqua(256, seed=1, continuous=True, device=DEV)
    env.reset()
    with pytest.raises(ValueError):
        EpisodeTracker(env, capacity=255)
    tracker = EpisodeTracker(env, epsilon=(1.0, 0.05, 0.99))
    with pytest.raises(ValueError):
        tracker.explore(torch.zeros(256, dtype=torch.uint8, device=DEV))                       # continuous worlds
    env = BatchedAqua(256, seed=1, device=DEV)
    env.reset()
    tracker = EpisodeTracker(env, epsilon=(1.0, 0.05, 0.99))
    for bad in (torch.zeros(256, dtype=torch.int64, device=DEV), torch.zeros(256, dtype=torch.uint8), torch.zeros(255, dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError):
            tracker.explore(bad)
    for kw in (dict(reward=torch.zeros(256, dtype=torch.float64, device=DEV)), dict(term=torch.zeros(256, dtype=torch.uint8)),
               dict(time=torch.zeros(256, dtype=torch.int64, device=DEV)), dict(reward=torch.zeros(100, dtype=torch.float32, device=DEV))):
        with pytest.raises(ValueError):
            tracker.after_step(**kw)
    with pytest.raises(ValueError):
        tracker.explore(torch.zeros(256, dtype=torch.uint8, device=DEV), epsilon=torch.zeros(1, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError):
        EpisodeTracker(env).explore(torch.zeros(256, dtype=torch.uint8, device=DEV))           # no schedule, no epsilon given
    with pytest.raises(ValueError):
        EpisodeTracker(env, epsilon=(0.05, 1.0, 100))                                          # would grow: decay factor > 1
    assert tracker.counts()["steps"] == 0
