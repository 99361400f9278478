"""GPU tests of libaqua_lbank.so (include/aqua_lbank.h), DQNLearnerBank (aquaticgymenv_amd/lbank.py) and PopulationLoop
(aquaticgymenv_amd/trainer.py): one update of every network of a bank in two launches, against the P calls of
aqualrn_update_f32 it replaces; the segmented draw against its numpy model; the Python layer's blobs, resume and loop.
Every comparison is exact: the bank runs the learner's own device code per network.
"""
import numpy as np
import pytest

from tests import _lbank as K
from tests import _learner as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, SEG, ROUNDS = 120, 40, 4
CAP = ROUNDS * N
LOSS_REFERENCE = 16


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


@pytest.fixture(scope="module")
def run(torch):
    return K.Runner(torch, DEV)


@pytest.fixture(scope="module")
def ring_np():
    return L.float_ring(CAP, CAP, 11, bad_ok=0.05)


# ------------------------------------------------------------------------------------------------ the update contract
def _both(torch, run, st, ring_np, idxs, B, strategy, hyper):
    """the same updates through the bank and through single calls -> [(bank outputs, single outputs)] per update"""
    ring = L.DeviceRing(torch, ring_np, DEV)
    a, b = K.to_device(torch, st, B, DEV), K.to_device(torch, st, B, DEV)
    hd = run.hyper_dev(hyper)
    out = []
    for idx in idxs:
        i = torch.as_tensor(np.ascontiguousarray(idx, dtype=np.int32)).to(DEV)
        run.bank_update(a, ring, i, B, strategy, hd)
        run.single_updates(b, ring, i, B, strategy, hyper)
        out.append((K.read(torch, a), K.read(torch, b)))
    return out


def _check_contract(torch, run, ring_np, P, B, strategy, updates=3, seed=0):
    rng = np.random.RandomState(100 + B + seed)
    st = K.make_state(P, 3 + seed)
    idxs = [K.mixed_idx(rng, P, B, ring_np, CAP) for _ in range(updates)]
    before = K.read(torch, K.to_device(torch, st, B, DEV))
    steps = _both(torch, run, st, ring_np, idxs, B, strategy, K.hypers(P))
    for u, (bank, single) in enumerate(steps):
        assert K.differing(bank, single) == [], (u, K.differing(bank, single))
    last = steps[-1][0]
    # something happened, in every slot, and differently per slot
    assert bool((last["t"] == before["t"] + updates).all())
    for name in ("theta", "theta_target", "m", "v", "blob", "blob_target"):
        assert all(last[name][p].tobytes() != before[name][p].tobytes() for p in range(P)), name
    assert bool((last["loss"] > 0).all()) and bool((last["loss"] != 77.0).all())
    assert P > 3 or len(set(last["loss"].tolist())) == P
    assert bool((last["idx_out"][:, :B] != -7).all())
    return steps


@pytest.mark.parametrize("B", [1, 33, 64, 97, 200])
def test_update_equals_three_single_learners_bit_for_bit(torch, run, ring_np, B):
    """P = 3, different hyper-parameters per network, three consecutive updates: a one-lane tile, tile tails, two wavefronts,
    several workgroups.  Every output of the contract, slot by slot."""
    _check_contract(torch, run, ring_np, 3, B, 0)


@pytest.mark.parametrize("strategy", [0, 1, 2, 3, 0 | LOSS_REFERENCE, 2 | LOSS_REFERENCE])
def test_every_strategy_and_both_loss_forms(torch, run, ring_np, strategy):
    """the four template instantiations at B = 64, and the loss flag: the same inputs without it give another gradient"""
    steps = _check_contract(torch, run, ring_np, 3, 64, strategy, updates=2)
    if strategy & LOSS_REFERENCE:
        plain = _check_contract(torch, run, ring_np, 3, 64, strategy & ~LOSS_REFERENCE, updates=2)
        assert all(steps[0][0]["grad"][p].tobytes() != plain[0][0]["grad"][p].tobytes() for p in range(3))
        assert np.array_equal(steps[0][0]["idx_out"], plain[0][0]["idx_out"])


def test_integer_networks_give_the_exact_gradient_in_every_slot(torch, run):
    """integer networks that differ per slot, an integer ring, gamma = 1: the gradient of every slot is the int64 model's
    times float32(2 / B_eff) exactly -- a block that read another network's weights, target or samples cannot pass"""
    P, B, cap, size = 3, 97, 300, 257
    ring_np = L.int_ring(cap, size, 7, bad_ok=0.1)
    layers = [L.int_layers(salt=p) for p in range(P)]
    targets = [L.int_layers(salt=p + 1) for p in range(P)]
    st = K.make_state(P, 1, layers, targets, fresh=True)
    idx = K.mixed_idx(np.random.RandomState(5), P, B, ring_np, cap)
    hyper = K.hypers(P)
    hyper[:, 0] = 1.0
    bank = _both(torch, run, st, ring_np, [idx], B, 0, hyper)[0][0]
    grads = []
    for p in range(P):
        eff = L.effective(idx[p], ring_np)
        worst, S, ref = L.abs_sums(st["theta"][p], st["theta_target"][p], ring_np, eff, "double_ref")
        assert worst < 2 ** 24
        want = S.astype(np.float32) * np.float32(2.0 / ref["n"])
        assert np.array_equal(bank["grad"][p].view(np.uint32), want.view(np.uint32)), p
        assert np.array_equal(bank["idx_out"][p], eff) and np.count_nonzero(want) > 500
        grads.append(want)
    assert not np.array_equal(grads[0], grads[1]) and not np.array_equal(grads[1], grads[2])


def test_an_all_invalid_network_between_two_that_learn(torch, run, ring_np):
    P, B = 3, 64
    st = K.make_state(P, 9)
    idx = K.mixed_idx(np.random.RandomState(2), P, B, ring_np, CAP)
    dead = np.nonzero(ring_np["ok"] == 0)[0]
    idx[1] = np.resize(np.concatenate([[-1, CAP, 2 ** 31 - 1, -2 ** 31], dead]), B)
    before = K.read(torch, K.to_device(torch, st, B, DEV))
    bank, single = _both(torch, run, st, ring_np, [idx], B, 0, K.hypers(P))[0]
    assert K.differing(bank, single) == []
    for name in ("theta", "theta_target", "m", "v", "t", "blob", "blob_target"):
        assert bank[name][1].tobytes() == before[name][1].tobytes(), name
        assert bank[name][0].tobytes() != before[name][0].tobytes() and bank[name][2].tobytes() != before[name][2].tobytes(), name
    assert float(bank["loss"][1]) == 0.0 and bool((bank["grad"][1] == 0).all()) and bool((bank["idx_out"][1] == -1).all())
    # slots 0 and 2 as if they ran alone: a bank of one network each
    for p in (0, 2):
        one = {k: v[p:p + 1] for k, v in st.items()}
        alone = _both(torch, run, one, ring_np, [idx[p:p + 1]], B, 0, K.hypers(P)[p:p + 1])[0][0]
        for name in K.OUTPUTS:
            assert alone[name][0].tobytes() == bank[name][p].tobytes(), (name, p)


def test_more_workgroups_than_the_device_holds_at_once(torch, run, ring_np):
    """P = 600 at B = 64: 600 workgroups of the gradient launch, where 256 CUs hold 512 at once"""
    _check_contract(torch, run, ring_np, 600, 64, 0, updates=1)


def test_above_the_learners_grid_cap(torch, run, ring_np):
    """P = 2 at B = 65 600: 2 050 tiles, more than the 2 x 512 wavefronts of the largest grid take one or two each, so a
    wavefront walks several tiles (tiles_per_wave = ceil(2 050 / 1 024) = 3) and the last workgroups are ragged"""
    B = 65600
    assert L.launch_shape(B) == (2050, 3, 342)
    _check_contract(torch, run, ring_np, 2, B, 0, updates=1)


# ------------------------------------------------------------------------------------------------ the draw
def _draw(torch, run, filled, ok, capacity, n, seg, seeds, t, B):
    header = torch.as_tensor(np.array([filled % capacity, filled, 0, 0], dtype=np.int64)).to(DEV)
    ok_d = torch.as_tensor(ok).to(DEV)
    t_d = torch.as_tensor(np.asarray(t, dtype=np.int64)).to(DEV)
    s_d = torch.as_tensor(np.asarray(seeds, dtype=np.uint64).view(np.int64)).to(DEV)
    out = torch.full((len(seeds), B), 77, dtype=torch.int32, device=DEV)
    rc = run.bank.lib.aqualbank_draw(header.data_ptr(), ok_d.data_ptr(), capacity, n, seg, len(seeds), t_d.data_ptr(), s_d.data_ptr(),
                                     out.data_ptr(), B, run._stream())
    run.bank.check(rc, "aqualbank_draw")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("P,seg", [(3, 40), (3, 50), (5, 40)])
def test_draw_equals_the_numpy_model_and_stays_inside_each_networks_slots(torch, run, P, seg):
    """the short last network (3 x 50 over 120 worlds), two networks beyond N (5 x 40); the ring empty, partly filled,
    wrapped (a size the header overstates is clamped), with holes in ok"""
    rng = np.random.RandomState(P * 100 + seg)
    B = 300
    seeds = [17 + 1000 * p for p in range(P)]
    seeds[-1] = 2 ** 64 - 5
    t = [(5 * p) % 7 for p in range(P)]
    for filled, holes in ((0, 0.0), (2 * N, 0.0), (2 * N, 0.3), (CAP, 0.3), (CAP + 5 * N, 0.9)):
        ok = (rng.rand(CAP) >= holes).astype(np.uint8)
        ok[min(filled, CAP):] = 0                                      # never written
        got = _draw(torch, run, filled, ok, CAP, N, seg, seeds, t, B)
        want = K.draw_model(seeds, t, B, filled, ok, CAP, N, seg)
        assert np.array_equal(got, want), (filled, holes)
        for p in range(P):
            row = got[p]
            live = row[row >= 0]
            if p * seg >= N or filled == 0:
                assert live.size == 0
                continue
            assert bool((K.owner(live, N, seg) == p).all()) and bool((ok[live] != 0).all()) and bool((live < min(filled, CAP)).all())
            assert live.size > 0 and (holes > 0 or live.size == B)
            if holes == 0.9:
                assert live.size < B                                   # four attempts do not always find a transition
        if filled:
            assert not np.array_equal(got[0], got[1])


def test_draw_of_one_network_with_a_huge_segment_is_the_rings_own_draw(torch, run):
    from aquaticgymenv_amd import _replay_capi
    rng = np.random.RandomState(4)
    B, seed, t = 500, 99, 6
    for filled in (0, 3 * N, CAP):
        ok = (rng.rand(CAP) >= 0.3).astype(np.uint8)
        got = _draw(torch, run, filled, ok, CAP, N, 2 ** 40, [seed], [t], B)
        header = torch.as_tensor(np.array([0, filled, 0, 0], dtype=np.int64)).to(DEV)
        ok_d, t_d = torch.as_tensor(ok).to(DEV), torch.as_tensor(np.array([t], dtype=np.int64)).to(DEV)
        out = torch.full((B,), 77, dtype=torch.int32, device=DEV)
        _replay_capi.check(_replay_capi.lib.aquarpl_draw(header.data_ptr(), ok_d.data_ptr(), CAP, t_d.data_ptr(), seed, out.data_ptr(), B,
                                                         run._stream()), "aquarpl_draw")
        torch.cuda.synchronize()
        assert np.array_equal(got[0], out.cpu().numpy()), filled
        ring = dict(ok=ok, size=filled)
        assert np.array_equal(got[0], L.drawn(seed, t + 1, B, ring))


# ------------------------------------------------------------------------------------------------ the Python layer
def _population(torch, seed=0, **kw):
    from aquaticgymenv_amd.lbank import DQNLearnerBank
    from aquaticgymenv_amd.qbank import QNetworkBank
    bank = QNetworkBank([L.glorot_layers(40 + seed + p) for p in range(3)], SEG, DEV)
    kw.setdefault("gamma", [0.98, 0.9, 0.95])
    kw.setdefault("lr", [1e-3, 3e-3, 1e-2])
    kw.setdefault("tau", [0.005, 0.05, 1.0])
    return bank, DQNLearnerBank(bank, seed=21, **kw)


def _single(torch, lb, p, layers):
    from aquaticgymenv_amd.learner import DQNLearner
    from aquaticgymenv_amd.qpolicy import QNetwork
    h = lb.hyper_of(p)
    return DQNLearner(QNetwork(layers, DEV), gamma=h["gamma"], tau=h["tau"], lr=h["lr"], strategy=lb.strategy, seed=lb.seeds[p],
                      loss=lb.loss_form)


def test_bank_acts_with_the_new_weights_and_target_blobs_are_the_single_learners(torch, ring_np):
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.qpolicy import QNetwork
    bank, lb = _population(torch)
    layers0 = [[(k.copy(), b.copy()) for k, b in net] for net in bank.layers]
    singles = [_single(torch, lb, p, layers0[p]) for p in range(3)]
    ring = L.DeviceRing(torch, ring_np, DEV)
    x = torch.as_tensor(np.random.RandomState(1).rand(5, 3 * SEG).astype(np.float32)).to(DEV)
    q_before = bank.q_values(x).clone()
    idx = torch.as_tensor(K.mixed_idx(np.random.RandomState(8), 3, 64, ring_np, CAP)).to(DEV)
    for _ in range(2):
        loss = lb.update(ring, 64, idx)
        for p in range(3):
            singles[p].update(ring, 64, idx=idx[p])
    torch.cuda.synchronize()
    tbank = QNetworkBank(layers0, SEG, DEV)
    tbank.tensor.copy_(lb.target_tensor)
    q_bank, q_target = bank.q_values(x), tbank.q_values(x)
    for p in range(3):
        seg = slice(p * SEG, (p + 1) * SEG)
        xp = x[:, seg].contiguous()
        assert torch.equal(bank.view(p).blob, singles[p].qnet.blob) and torch.equal(lb.target_tensor[p], singles[p].target_blob)
        assert torch.equal(bank.view(p).act(xp), singles[p].qnet.act(xp))
        assert torch.equal(q_bank[:, seg], singles[p].qnet.q_values(xp)) and not torch.equal(q_bank[:, seg], q_before[:, seg])
        target = QNetwork(layers0[p], DEV)
        target.blob.copy_(singles[p].target_blob)
        assert torch.equal(q_target[:, seg], target.q_values(xp))
        assert torch.equal(loss[p:p + 1], singles[p].loss) and torch.equal(lb.grad[p], singles[p].grad)
        for (k, b), (k1, b1) in zip(lb.weights(p), singles[p].weights()):
            assert np.array_equal(k, k1) and np.array_equal(b, b1)
        for (k, b), (k1, b1) in zip(lb.target_weights(p), singles[p].target_weights()):
            assert np.array_equal(k, k1) and np.array_equal(b, b1)
    assert int(lb.t.sum()) == 6


def test_resume_and_interop_with_the_single_learner(torch, ring_np):
    from aquaticgymenv_amd.learner import DQNLearner
    ring = L.DeviceRing(torch, ring_np, DEV)
    idxs = [torch.as_tensor(K.mixed_idx(np.random.RandomState(30 + u), 3, 64, ring_np, CAP)).to(DEV) for u in range(4)]
    bank, lb = _population(torch, strategy="double", loss="reference")
    for u in range(2):
        lb.update(ring, 64, idxs[u])
    lb.set_hyper(2, lr=5e-3, gamma=0.97)
    state = lb.state_dict()
    slot = lb.slot_state_dict(1)
    # a fresh bank of other weights and hyper-parameters takes the state and goes on with the same bits
    bank2, lb2 = _population(torch, seed=50, gamma=0.5, lr=1e-4, tau=0.5)
    lb2.load_state_dict(state)
    assert lb2.strategy == "double" and lb2.loss_form == "reference" and lb2.hyper_of(2)["lr"] == 5e-3 and lb2.seeds == lb.seeds
    assert torch.equal(bank2.tensor, bank.tensor) and torch.equal(lb2.target_tensor, lb.target_tensor) and torch.equal(lb2.hyper, lb.hyper)
    # ... and one member continues alone in a DQNLearner on its slot of a third bank
    bank3, _ = _population(torch, seed=70)
    alone = DQNLearner(bank3.view(1)).load_state_dict(slot)
    assert alone.strategy == "double" and alone.loss_form == "reference" and alone.gamma == 0.9 and int(alone.t[0]) == 2
    for u in (2, 3):
        lb.update(ring, 64, idxs[u])
        lb2.update(ring, 64, idxs[u])
        alone.update(ring, 64, idx=idxs[u][1])
    torch.cuda.synchronize()
    for name in ("theta", "theta_target", "m", "v", "t", "loss", "grad", "target_tensor"):
        assert torch.equal(getattr(lb, name), getattr(lb2, name)), name
    assert torch.equal(bank.tensor, bank2.tensor)
    for name in ("theta", "theta_target", "m", "v"):
        assert torch.equal(getattr(lb, name)[1], getattr(alone, name)), name
    assert int(alone.t[0]) == int(lb.t[1]) == 4 and torch.equal(bank3.tensor[1], bank.tensor[1]) and torch.equal(alone.target_blob, lb.target_tensor[1])
    assert not torch.equal(bank3.tensor[0], bank.tensor[0])
    with pytest.raises(ValueError, match="network 1"):
        lb.set_hyper(1, tau=1.5)
    with pytest.raises(ValueError):
        lb.update(ring, 64, idxs[0][:2].contiguous())


# ------------------------------------------------------------------------------------------------ the loop
WORLDS, SEG_L, BATCH, ITERATIONS = 96, 32, 64, 6


def _parts(torch):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.lbank import DQNLearnerBank
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.replay import DeviceReplayRing
    bank = QNetworkBank([L.glorot_layers(60 + p) for p in range(3)], SEG_L, DEV)
    bank.epsilon = torch.tensor([0.5, 0.1, 1.0], dtype=torch.float32, device=DEV)
    learners = DQNLearnerBank(bank, gamma=[0.98, 0.9, 0.95], lr=[1e-3, 3e-3, 1e-2], tau=[0.005, 0.05, 0.5], seed=5)
    env = BatchedAqua(WORLDS, obstacles=True, seed=23, auto_reset="next_step", normalized_obs=True, device=DEV)
    env.params.time_limit = 4
    env.reset()
    ring = DeviceReplayRing(env, 4 * WORLDS)
    tracker = EpisodeTracker(env)
    return dict(env=env, bank=bank, learners=learners, ring=ring, tracker=tracker)


def _by_hand(p):
    """one iteration from the public pieces"""
    env, bank, ring, tracker, learners = p["env"], p["bank"], p["ring"], p["tracker"], p["learners"]
    action = bank.act(env, epsilon=0.0, out=env.policy_action)
    ring.before_step(env.policy_action)
    env.step(action)
    ring.after_step()
    tracker.after_step()
    idx = learners.draw(ring, BATCH)
    learners.update(ring.learner_view(), BATCH, idx)


def _loop_state(p):
    env, ring, tracker, lb = p["env"], p["ring"], p["tracker"], p["learners"]
    out = {"env.state": env.state, "env.time": env.time, "env.reward": env.reward, "env.term": env.term, "env.obs_norm": env.obs_norm_buf,
           "env.policy_action": env.policy_action, "bank.tensor": p["bank"].tensor, "bank.epsilon": p["bank"].epsilon,
           "ring.header": ring.header}
    for name in ("s", "a", "r", "s2", "d", "ok"):
        out["ring." + name] = getattr(ring, name)
    for name in ("ret", "len", "log_ret", "log_len", "log_code", "log_world", "_counts"):
        out["tracker." + name] = getattr(tracker, name)
    for name in ("theta", "theta_target", "m", "v", "t", "target_tensor", "hyper", "seed_dev"):
        out["learners." + name] = getattr(lb, name)
    return out


def test_population_loop_step_and_graph_equal_the_iteration_by_hand(torch):
    from aquaticgymenv_amd.trainer import PopulationLoop
    a, b, c = _parts(torch), _parts(torch), _parts(torch)
    loop_b = PopulationLoop(b["env"], b["bank"], b["learners"], b["ring"], b["tracker"], BATCH)
    loop_c = PopulationLoop(c["env"], c["bank"], c["learners"], c["ring"], c["tracker"], BATCH)
    before = {k: v.clone() for k, v in _loop_state(c).items() if k != "env.policy_action"}
    eps0, theta0 = c["bank"].epsilon.clone(), c["learners"].theta.clone()
    graph = loop_c.capture()
    torch.cuda.synchronize()
    for k, v in before.items():                                # the capture and its warm-up left no trace
        assert torch.equal(_loop_state(c)[k], v), k
    assert c["env"]._tick == 0 and int(c["learners"].t.sum()) == 0
    for it in range(ITERATIONS):
        _by_hand(a)
        loop_b.step()
        graph.launch()
        sa, sb, sc = _loop_state(a), _loop_state(b), _loop_state(c)
        for name in sa:
            assert torch.equal(sa[name], sb[name]), ("step() differs from the iteration by hand", name, it)
            assert torch.equal(sa[name], sc[name]), ("the graph differs from the iteration by hand", name, it)
        assert a["env"]._tick == b["env"]._tick == c["env"]._tick == it + 1
        assert torch.equal(loop_b.idx, loop_c.idx)
    for p in (a, b, c):
        assert [int(v) for v in p["learners"].t.cpu()] == [ITERATIONS] * 3 and torch.equal(p["bank"].epsilon, eps0)
        assert p["tracker"].counts()["episodes"] > 0 and int(p["ring"].header[3]) == ITERATIONS
        assert all(not torch.equal(p["learners"].theta[k], theta0[k]) for k in range(3))
    # every minibatch came from the network's own worlds
    idx = loop_c.idx.cpu().numpy()
    for k in range(3):
        live = idx[k][idx[k] >= 0]
        assert live.size > 0 and bool((K.owner(live, WORLDS, SEG_L) == k).all())
    graph.close()


def test_population_loop_rejections(torch):
    from aquaticgymenv_amd.replay import DeviceReplayRing
    from aquaticgymenv_amd.trainer import PopulationLoop
    p, other = _parts(torch), _parts(torch)
    args = [p["env"], p["bank"], p["learners"], p["ring"], p["tracker"]]
    PopulationLoop(*args, batch_size=BATCH)
    bad = [args[:1] + [p["bank"].view(0)] + args[2:], args[:2] + [other["learners"]] + args[3:],
           args[:3] + [DeviceReplayRing(p["env"], 4 * WORLDS + 1)] + args[4:], args[:3] + [other["ring"]] + args[4:],
           args[:4] + [other["tracker"]]]
    for case in bad:
        with pytest.raises(ValueError):
            PopulationLoop(*case, batch_size=BATCH)
    for batch in (0, (1 << 20) + 1):
        with pytest.raises(ValueError):
            PopulationLoop(*args, batch_size=batch)
    eps, p["bank"].epsilon = p["bank"].epsilon, None
    with pytest.raises(ValueError):
        PopulationLoop(*args, batch_size=BATCH)
    p["bank"].epsilon = eps
