"""GPU tests of the Q-network bank (libaqua_bank.so, aquaticgymenv_amd/qbank.py): P networks act on one batch in a single
launch, network p on worlds [p * seg, (p + 1) * seg).

Two references, both exact.  (1) Integer networks that differ from slot to slot (tests/_qbank.py: a kernel that reads the
wrong slot cannot pass), every segment fed the same inputs, against an int64 numpy evaluation: Q, action (lowest index on a
tie) and q_taken must be EQUAL.  (2) The policy kernel: segment by segment the bank writes bit for bit what QNetwork.act
writes for that network on that slice with env_offset + p * seg -- greedy, with one epsilon, and with a device epsilon per
network.  The explored share of a segment is not asserted here; equality with the policy kernel is the check.
"""
import numpy as np
import pytest

from tests import _qbank as B

pytestmark = pytest.mark.gpu

DEV = B.DEV


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


# ------------------------------------------------------------------------------------------------ 1. exact, every tail
@pytest.mark.parametrize("networks,seg,n", [(1, 100, 100), (7, 33, 231), (7, 33, 100), (64, 1, 64), (3, 4099, 3 * 4099)],
                         ids=["single", "two_tiles", "cut_segment", "one_world_each", "many_tiles"])
def test_exact_integer_bank_every_tail(torch, networks, seg, n):
    """both input forms; worlds behind N -- the rest of a cut segment, the empty segments -- are not written"""
    B.check_integer_bank(torch, networks, seg, n, seed=networks * 1000 + seg)


# ------------------------------------------------------------------------------------------------ 2. the policy kernel
def _float_networks(networks):
    return [B.golden_layers("no_obs"), B.golden_layers("with_obs")][:networks] + [B.random_layers(100 + p) for p in range(2, networks)]


@pytest.mark.parametrize("epsilon", ["greedy", "uniform", "per_network"])
@pytest.mark.parametrize("networks,seg,n", [(5, 700, 3400), (64, 31, 1984)], ids=["5x700", "64x31"])
def test_bit_for_bit_the_policy_kernel(torch, networks, seg, n, epsilon):
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.qpolicy import QNetwork
    nets = _float_networks(networks)
    bank = QNetworkBank(nets, seg, DEV)
    g = torch.Generator(device=DEV).manual_seed(networks)
    ld = n + 64
    buf = torch.rand((5, ld), device=DEV, generator=g)
    off, seed, tick = 5 << 20, 0x0123456789ABCDEF, (1 << 32) + 9
    eps_call, eps_of = 0.0, np.zeros(networks, dtype=np.float32)
    if epsilon == "uniform":
        eps_call = 0.3
        eps_of[:] = 0.3
    elif epsilon == "per_network":
        eps_call = 0.9                                        # ignored: the device values rule
        rng = np.random.RandomState(3)
        eps_of = rng.uniform(0, 1, networks).astype(np.float32)
        eps_of[:4] = [0.0, 0.05, 0.5, 1.0]
        eps_of[networks - 1] = np.nan
        eps_of[4 if networks > 5 else 1] = -0.4               # (five networks: in the place of 0.05)
        bank.epsilon = torch.as_tensor(eps_of, device=DEV)
    a, q, qt = B.outputs(torch, ld)
    bank.act(buf, epsilon=eps_call, n=n, env_offset=off, seed=seed, tick=tick, out=a, q=q, q_taken=qt)
    ra, rq, rqt = B.outputs(torch, ld)
    single = QNetwork(nets[0], DEV)
    explored = 0
    for p in range(networks):
        lo = p * seg
        cnt = min(seg, n - lo)
        if cnt <= 0:
            break
        e = float(eps_of[p])
        e = e if e >= 0 else 0.0                              # NaN or negative: never explores
        single.load(nets[p])
        single.act(buf[:, lo:lo + cnt], epsilon=e, n=cnt, env_offset=off + lo, seed=seed, tick=tick, out=ra[lo:lo + cnt],
                   q=rq[:, lo:lo + cnt], q_taken=rqt[lo:lo + cnt])
        if e == 0.0:
            greedy = single.act(buf[:, lo:lo + cnt], n=cnt)
            assert torch.equal(greedy, ra[lo:lo + cnt])
        else:
            explored += int((single.act(buf[:, lo:lo + cnt], n=cnt) != ra[lo:lo + cnt]).sum())
    torch.cuda.synchronize()
    assert torch.equal(a, ra) and torch.equal(q, rq) and torch.equal(qt, rqt)
    assert B.untouched(a, q, qt, n)
    assert len(torch.unique(a[:n])) == 3
    assert (explored > 0) == (epsilon != "greedy")


# ------------------------------------------------------------------------------------------------ 3. past the grid cap
@pytest.mark.parametrize("networks,seg,n", [(5, 22400, 112000), (3200, 5, 16000), (5, 22432, 112160), (2, 100000, 100005)],
                         ids=["five_networks", "network_per_item", "runs_cross_networks", "cut_last_segment"])
def test_past_the_grid_cap(torch, networks, seg, n):
    """more items than resident wavefronts: wavefronts walk a run of items.  On 256 compute units (3 072 wavefronts) the
    runs are one or two items long and start at even items, so with 700 tiles per network (the first shape) every run
    stays inside one network; a new network, weights and LDS copy reloaded inside the run, comes at every item in the second
    shape, and with 701 tiles per network (the third) where a run of two straddles a boundary.  The fourth shape exceeds the
    cap only because its items are counted right: 3 125 tiles of network 0 and ONE of network 1, which N cuts after 5 worlds."""
    from aquaticgymenv_amd import _bank_capi
    items = _bank_capi.lib.aquabank_items(seg, n)
    assert items == (n // seg) * -(-seg // 32) + -(-(n % seg) // 32)
    cap = B.resident_wavefronts(torch)
    if items <= cap:
        pytest.skip("%d items do not exceed the %d resident wavefronts of this device" % (items, cap))
    B.check_integer_bank(torch, networks, seg, n, seed=seg, forms=("normalised",))


@pytest.mark.parametrize("networks,seg,n", [(1, 2 ** 62, 100), (3, 2 ** 40, 4099), (2, 2 ** 31 + 7, 33)],
                         ids=["one_network_any_batch", "three_of_2^40", "past_int32"])
def test_the_work_of_a_launch_follows_n_not_seg(torch, networks, seg, n):
    """seg far beyond N ("this network for whatever batch comes"): the launch walks the tiles that hold a world, not those
    seg allows (tests/test_qbank_cpu.py holds the count); every world acts with network 0, nothing behind N is written"""
    from aquaticgymenv_amd import _bank_capi
    assert _bank_capi.lib.aquabank_items(seg, n) == -(-n // 32)
    B.check_integer_bank(torch, networks, seg, n, seed=n)


# ------------------------------------------------------------------------------------------------ 4. in the loop
SEG = 640


def _twins(torch, mode, per_world, seed=31):
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.batched import BatchedAqua
    n = 2 * SEG
    if per_world:
        rng = np.random.RandomState(7)
        obstacles = np.repeat(presets.BENCH8[None], n, axis=0).astype(np.float64)
        obstacles[:, :, 0:2] += rng.uniform(-3, 3, (n, 8, 2))
    else:
        obstacles = presets.BENCH8
    envs = [BatchedAqua(n, obstacles=obstacles, seed=seed, auto_reset=mode, env_offset=1000, device=DEV) for _ in range(2)]
    for e in envs:
        e.reset()
    return envs


def _same(torch, a, b):
    return (torch.equal(a.state, b.state) and torch.equal(a.reward, b.reward) and torch.equal(a.term, b.term)
            and torch.equal(a.done_bits, b.done_bits) and torch.equal(a.time, b.time))


def _act_by_halves(nets, env, eps, out):
    """the action tensor of the step `env` is about to take, from one QNetwork.act per half"""
    for p, net in enumerate(nets):
        lo = p * SEG
        net.act(env.state[:, lo:lo + SEG], normalised=False, n=SEG, epsilon=eps, env_offset=env.env_offset + lo, seed=env.seed,
                tick=env._tick, out=out[lo:lo + SEG])
    return out


@pytest.mark.parametrize("eps", [0.0, 0.2])
@pytest.mark.parametrize("per_world", [False, True], ids=["shared", "tables"])
@pytest.mark.parametrize("mode", ["next_step", "same_step"])
def test_step_with_a_bank_equals_act_by_halves_then_step(torch, mode, per_world, eps):
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.qpolicy import QNetwork
    layers = [B.golden_layers("no_obs"), B.golden_layers("with_obs")]
    bank = QNetworkBank(layers, SEG, DEV)
    nets = [QNetwork(l, DEV) for l in layers]
    a, b = _twins(torch, mode, per_world)
    act = torch.zeros(2 * SEG, dtype=torch.uint8, device=DEV)
    for it in range(12):
        a.step(policy=bank, epsilon=eps)
        b.step(_act_by_halves(nets, b, eps, act))
        assert _same(torch, a, b), it
        assert torch.equal(a.policy_action[:2 * SEG], act), it
    # the halves really act differently: the other network on a half gives other actions
    swapped = _act_by_halves(nets[::-1], b, eps, torch.zeros_like(act))
    both = _act_by_halves(nets, b, eps, act)
    assert int((swapped[:SEG] != both[:SEG]).sum()) > 0 and int((swapped[SEG:] != both[SEG:]).sum()) > 0
    # rollout(actions=bank) goes through the same launch
    reward, term = a.rollout(3, actions=bank, epsilon=eps, keep_all=True)
    for it in range(3):
        b.step(_act_by_halves(nets, b, eps, act))
        assert torch.equal(reward[it, :2 * SEG], b.reward[:2 * SEG]) and torch.equal(term[it, :2 * SEG], b.term[:2 * SEG]), it
    assert torch.equal(a.state, b.state) and a._tick == b._tick == 15


def test_a_bank_that_does_not_cover_the_batch_is_an_error_with_the_banks_message(torch):
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.qbank import QNetworkBank
    bank = QNetworkBank([B.family(0), B.family(1)], 100, DEV)
    env = BatchedAqua(201, obstacles=presets.BENCH8, seed=1, device=DEV)
    env.reset()
    with pytest.raises(ValueError):
        env.step(policy=bank)
    assert "networks * seg" in bank.last_error
    with pytest.raises(ValueError, match="networks \\* seg"):
        bank.act(env)
    with pytest.raises(ValueError):
        bank.epsilon = torch.zeros(1, dtype=torch.float32, device=DEV)
    with pytest.raises(IndexError):
        bank.view(2)
    # a bank is no QNetwork for a learner: there is no single blob, the message names view(p)
    with pytest.raises(TypeError, match="view"):
        bank.blob


def test_captured_bank_step_replays_like_eager_steps_and_sees_a_reloaded_slot(torch):
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.qpolicy import QNetwork
    eps = 0.2
    layers = [B.golden_layers("no_obs"), B.golden_layers("with_obs")]
    other = B.random_layers(77)
    bank = QNetworkBank(layers, SEG, DEV)
    a, b = _twins(torch, "next_step", True)
    for e in (a, b):
        for _ in range(3):
            e.step(policy=bank, epsilon=eps)                  # the graph starts at a tick other than 0
    graph = a.capture_policy_step(bank, epsilon=eps)
    for it in range(12):
        graph.launch()
        b.step(policy=bank, epsilon=eps)
        assert _same(torch, a, b), it
        assert torch.equal(a.policy_action, b.policy_action), it
    assert a._tick == b._tick == 15
    # new weights into slot 1 through its view: the SAME graph acts with them on segment 1, and segment 0 does not change
    nets_old = [QNetwork(l, DEV) for l in layers]
    nets_new = [nets_old[0], QNetwork(other, DEV)]
    would_old = _act_by_halves(nets_old, a, eps, torch.zeros(2 * SEG, dtype=torch.uint8, device=DEV))
    would_new = _act_by_halves(nets_new, a, eps, torch.zeros(2 * SEG, dtype=torch.uint8, device=DEV))
    assert torch.equal(would_old[:SEG], would_new[:SEG]) and int((would_old[SEG:] != would_new[SEG:]).sum()) > 10
    view = bank.view(1)
    assert view.blob.data_ptr() == bank.tensor.data_ptr() + bank.tensor.stride(0) and view.device == bank.device and view._aquapol_network
    view.load(other)
    assert torch.equal(view.blob, nets_new[1].blob) and torch.equal(bank.tensor[0], nets_old[0].blob)
    assert all(np.array_equal(k, k2) and np.array_equal(v, v2) for (k, v), (k2, v2) in zip(bank.layers[1], other))
    graph.launch()
    assert torch.equal(a.policy_action[:2 * SEG], would_new)
    b.step(policy=bank, epsilon=eps)
    assert _same(torch, a, b)
    # the view acts like a QNetwork of its own
    assert torch.equal(view.act(a.state[:, SEG:2 * SEG], normalised=False, n=SEG), nets_new[1].act(a.state[:, SEG:2 * SEG], normalised=False, n=SEG))
    graph.close()


# ------------------------------------------------------------------------------------------------ 5. training a slot
def test_a_learner_trains_a_slot_in_place(torch):
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.learner import DQNLearner
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.qpolicy import QNetwork
    from aquaticgymenv_amd.replay import ReplayRing
    n, steps = 256, 4
    layers = B.golden_layers("with_obs")
    bank = QNetworkBank([layers, layers], n // 2, DEV)
    alone = QNetwork(layers, DEV)
    slot0 = bank.tensor[0].clone()
    assert torch.equal(bank.tensor[0], alone.blob) and torch.equal(bank.tensor[1], alone.blob)
    env = BatchedAqua(n, obstacles=presets.BENCH8, seed=77, auto_reset="next_step", normalized_obs=True, device=DEV)
    env.reset()
    ring = ReplayRing(env, steps * n)
    for _ in range(steps):
        bank.act(env, epsilon=0.3, out=env.policy_action)
        ring.before_step(env.policy_action)
        env.step(env.policy_action[:n])
        ring.after_step()
    assert ring.size == steps * n
    view = bank.view(1)
    in_place, reference = DQNLearner(view, seed=5), DQNLearner(alone, seed=5)
    for _ in range(3):
        in_place.update(ring, 64)
        reference.update(ring, 64)
    torch.cuda.synchronize()
    assert torch.equal(in_place.loss, reference.loss)
    assert torch.equal(bank.tensor[1], alone.blob) and not torch.equal(bank.tensor[1], slot0)       # trained, byte for byte
    assert torch.equal(bank.tensor[0], slot0)                                                      # untouched
    for (k, v), (k2, v2) in zip(view.weights(), in_place.weights()):
        assert np.array_equal(k.view(np.uint32), k2.view(np.uint32)) and np.array_equal(v.view(np.uint32), v2.view(np.uint32))
    # the bank acts with the trained slot on its next launch
    half = n // 2
    assert torch.equal(bank.act(env)[half:], alone.act(env.state[:, half:n], normalised=False, n=half, env_offset=env.env_offset + half,
                                                       seed=env.seed, tick=env._tick))


# ------------------------------------------------------------------------------------------------ 6. run_tests in one batch
def test_the_reference_test_protocol_in_one_batch(torch):
    """main/plotting/dqn_test_plotter.py::run_tests for both shipped policies at once: 1000 worlds without obstacles under
    no_obs, 1000 with the obstacle preset under with_obs, one evaluate().  No rate is asserted here (tests/test_qpolicy_gpu.py
    holds the published rates for single networks); equality with that path is the stronger statement."""
    from aquaticgymenv_amd import presets
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import evaluate
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.qpolicy import QNetwork
    seg = 1000
    tables = np.zeros((2 * seg, presets.DEFAULT5.shape[0], 5), dtype=np.float64)
    tables[:seg, :, 2] = -1.0                                 # kind < 0: an absent row
    tables[seg:] = presets.DEFAULT5
    layers = [B.golden_layers("no_obs"), B.golden_layers("with_obs")]
    results = []
    for policy in (lambda: QNetworkBank(layers, seg, DEV), lambda: B.SegmentBySegment([QNetwork(l, DEV) for l in layers], seg)):
        env = BatchedAqua(2 * seg, obstacles=tables, seed=9001, auto_reset=False, device=DEV)
        env.reset()
        results.append(evaluate(env, policy()))
    got, want = results
    for key in ("Reward", "Success", "Steps", "Code"):
        assert got[key].shape == (2 * seg,) and np.array_equal(got[key], want[key]), key
    assert bool((got["Code"] != 0).all())
    bank = QNetworkBank(layers, seg, DEV)
    rate = bank.split(got["Success"]).mean(axis=1)
    assert bank.split(got["Reward"]).shape == (2, seg) and rate.shape == (2,)
    assert bank.split(torch.zeros(3, 2 * seg, device=DEV)).shape == (3, 2, seg)
    print("success no_obs %.3f  with_obs %.3f" % (rate[0], rate[1]))
