"""GPU tests of libaqua_her.so (aquaticgymenv_amd/csrc/aqua_her.h), HindsightReplay (aquaticgymenv_amd/hindsight.py) and the
loops' hindsight= (aquaticgymenv_amd/trainer.py).

The kernel copies rows, walks integers, draws Philox words and computes one reward by rounded float64 operations in a fixed
order, and the learners are deterministic: every comparison is of bit patterns, against the numpy model of
tests/_her_model.py or between two runs on the device.  No tolerance anywhere."""
import ctypes
import types

import numpy as np
import pytest

from tests import _her_model as M
from tests import _learner as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = ("s", "a", "r", "s2", "d", "ok")
STAGED = ROWS + ("k", "m")


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


@pytest.fixture(scope="module")
def capi():
    from aquaticgymenv_amd import _her_capi
    return _her_capi


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


# ------------------------------------------------------------------------------------------------ 1. the kernel against the model
POISON = 0x5A


def _run(torch, capi, ring, header, N, idx, H, ratio, t, seeds=None, seed=None, guard=5, with_km=True):
    """aquaher_relabel through the C ABI on a host ring -> the model's dict of outputs, read back.  Exactly one of seeds (the
    table form, P keys) and seed (the scalar form).  The staged rows have the pitch P B + guard and start poisoned; the guard
    columns must come back so."""
    P, B = idx.shape
    m, ld = P * B, P * B + guard
    cont = ring["a"].ndim == 2
    dev = {k: torch.from_numpy(np.ascontiguousarray(ring[k])).to(DEV) for k in ROWS}
    hdr = torch.from_numpy(np.asarray(header, np.int64)).to(DEV)
    idx_dev = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(DEV)
    t_dev = torch.from_numpy(np.asarray(t, np.uint64).view(np.int64)).to(DEV)
    keys = None if seeds is None else torch.from_numpy(np.asarray(seeds, np.uint64).view(np.int64)).to(DEV)
    u8 = lambda *shape: torch.full(shape, POISON, dtype=torch.uint8, device=DEV)        # noqa: E731
    out = dict(s=u8(5, ld * 4), s2=u8(5, ld * 4), r=u8(ld * 4), a=u8(2, ld * 4) if cont else u8(ld), d=u8(ld), ok=u8(ld), k=u8(ld), m=u8(ld))
    rc = capi.lib.aquaher_relabel(hdr.data_ptr(), dev["s"].data_ptr(), dev["a"].data_ptr(), dev["r"].data_ptr(), dev["s2"].data_ptr(),
                                  dev["d"].data_ptr(), dev["ok"].data_ptr(), ring["s"].shape[1], ring["capacity"], 1 if cont else 0, N,
                                  idx_dev.data_ptr(), P, B, H, ratio, t_dev.data_ptr(), capi.NO_SEED if keys is not None else seed,
                                  None if keys is None else keys.data_ptr(),
                                  out["s"].data_ptr(), out["a"].data_ptr(), out["r"].data_ptr(), out["s2"].data_ptr(), out["d"].data_ptr(),
                                  out["ok"].data_ptr(), ld, out["k"].data_ptr() if with_km else None,
                                  out["m"].data_ptr() if with_km else None, None)
    capi.check(rc, "aquaher_relabel")
    torch.cuda.synchronize()
    for k in ROWS:                                            # the ring, the header, the counters and the keys are read only
        assert np.array_equal(_bits(dev[k].cpu().numpy()), _bits(ring[k])), k
    assert hdr.cpu().numpy().tolist() == list(header)
    assert np.array_equal(t_dev.cpu().numpy().view(np.uint64), np.asarray(t, np.uint64))
    got = {}
    for k, tensor in out.items():
        host = tensor.cpu().numpy()
        f32 = k in ("s", "s2", "r") or (k == "a" and cont)
        host = host.view(np.float32) if f32 else host
        if k in ("k", "m") and not with_km:
            assert (host == POISON).all()
            continue
        assert (_bits(host[..., m:]) == POISON).all(), ("guard columns", k)
        got[k] = np.ascontiguousarray(host[..., :m])
    return got


def _same(got, want, what):
    for k, v in got.items():
        assert np.array_equal(_bits(v), _bits(want[k])), (what, k, v, want[k])


# not yet full, just full, wrapped mid-ring, and a cursor that is no multiple of N
HEADERS = ((21, 21, 14, 3), (0, 42, 35, 6), (14, 42, 7, 8), (15, 42, 8, 8))
SEEDS = (17, 2 ** 64 - 3, 0x123456789ABCDEF)
TICKS = (0, 5, 2 ** 40 + 9)


@pytest.mark.parametrize("continuous", [False, True], ids=["u8", "f32x2"])
def test_relabel_equals_the_model_bit_for_bit(torch, capi, continuous):
    """N = 7, capacity 42 (six rounds) with the pitch 48, P = 3 (what a bank of segment 3 over 7 worlds has: one ragged
    network), B = 70: every slot, both neighbours of the range and far outside it, for every header, H in {1, 3, 8, 9, 64}
    (9 is one batch of loads and one step; 64 exceeds the rounds) and ratio in {0, 0.5, 1}, with the keys from a table of three
    and as a scalar.  Every branch the model names occurs."""
    ring = M.crafted_ring(continuous=continuous, ld=48)
    rng = np.random.RandomState(3)
    idx = np.concatenate([np.arange(42), [-1, 42, 43, 47, 10 ** 6, -2 ** 31, 2 ** 31 - 1], rng.randint(0, 42, 210 - 49)]).astype(np.int32)
    idx = idx[rng.permutation(210)].reshape(3, 70)
    cuts, fates = {}, {}
    for header in HEADERS:
        for H in (1, 3, 8, 9, 64):
            for ratio in (0.0, 0.5, 1.0):
                want = M.relabel(ring, header, 7, idx, H, ratio, TICKS, SEEDS)
                _same(_run(torch, capi, ring, header, 7, idx, H, ratio, TICKS, seeds=SEEDS), want, (header, H, ratio, "table"))
                for cut, fate in zip(want["cut"], want["fate"]):
                    cuts[cut] = cuts.get(cut, 0) + 1
                    fates[fate] = fates.get(fate, 0) + 1
                if ratio == 0.0:
                    assert not want["k"].any() and set(want["fate"]) <= {None, M.KEPT, M.NOT_CHOSEN}
                if ratio == 1.0:
                    assert M.NOT_CHOSEN not in want["fate"]
                if header[0] % 7:
                    assert set(want["cut"]) == {M.BAD_CURSOR} and not want["ok"].any()
            # the scalar form: every row keyed by the one seed (its own counter each), with and without k and m
            want = M.relabel(ring, header, 7, idx, H, 0.5, TICKS, (SEEDS[1],) * 3)
            _same(_run(torch, capi, ring, header, 7, idx, H, 0.5, TICKS, seed=SEEDS[1], with_km=(H != 3)), want, (header, H, "scalar"))
    print("cuts:", cuts, "fates:", fates)
    assert set(cuts) == {M.BAD_CURSOR, M.OUTSIDE, M.NOT_OK, M.OWN_TERMINAL, M.EPISODE_END, M.BROKEN, M.FRONTIER, M.CAPPED}
    assert set(fates) == {None, M.KEPT, M.NOT_CHOSEN, M.SUCCESS_K0, M.SUCCESS_LATER, M.SHAPED}
    assert min(cuts.values()) >= 3 and min(fates.values()) >= 3


def test_relabel_past_the_grid_cap(torch, capi):
    """P = 1 and B one block above MAX_BLOCKS x BLOCK, + 5: the grid-stride loop takes a second turn for some threads and not
    for others"""
    B = capi.MAX_BLOCKS * capi.BLOCK + capi.BLOCK + 5
    assert B <= capi.MAX_BATCH and B > capi.MAX_BLOCKS * capi.BLOCK
    ring = M.crafted_ring()
    header = (14, 42, 7, 8)
    rng = np.random.RandomState(8)
    idx = rng.randint(-1, 43, B).astype(np.int32).reshape(1, B)
    idx[0, -1], idx[0, capi.MAX_BLOCKS * capi.BLOCK] = 21, 0        # world 0, which never ends: the last sample, and the first of the second turn
    want = M.relabel(ring, header, 7, idx, 8, 0.5, [3], [99])
    got = _run(torch, capi, ring, header, 7, idx, 8, 0.5, [3], seed=99, guard=3)
    _same(got, want, "grid cap")
    assert len(set(want["cut"])) >= 6 and set(want["fate"]) == {None, M.KEPT, M.NOT_CHOSEN, M.SUCCESS_K0, M.SUCCESS_LATER, M.SHAPED}
    assert got["ok"][-1] == 1 and got["m"][-1] >= 1 and got["m"][capi.MAX_BLOCKS * capi.BLOCK] >= 1
    assert got["k"][capi.MAX_BLOCKS * capi.BLOCK:].any()


# ------------------------------------------------------------------------------------------------ 2. and 3. through the learners
N_L, ROUNDS_L = 16, 12
CAP_L = N_L * ROUNDS_L


def _learner_ring(seed=4):
    """a full, wrapped ring of 16 worlds and 12 rounds with episode ends, gaps, and rewards of a realistic size"""
    rng = np.random.RandomState(seed)
    ring = dict(capacity=CAP_L, s=(rng.rand(5, CAP_L)).astype(np.float32), s2=(rng.rand(5, CAP_L)).astype(np.float32),
                r=(rng.rand(CAP_L) * 2 - 1).astype(np.float32), a=rng.randint(0, 3, CAP_L).astype(np.uint8),
                d=(rng.randint(1, 4, CAP_L) * (rng.rand(CAP_L) < 0.12)).astype(np.uint8), ok=(rng.rand(CAP_L) < 0.93).astype(np.uint8))
    return ring, np.array([5 * N_L, CAP_L, 4 * N_L, 29], np.int64)


def _device_ring(torch, ring, header):
    """the host ring as HindsightReplay and the learners read a DeviceReplayRing: its rows, header, capacity and env"""
    out = types.SimpleNamespace(torch=torch, device=torch.device(DEV), capacity=ring["capacity"], size=ring["capacity"], _kind=0,
                                env=types.SimpleNamespace(num_envs=N_L, continuous=False),
                                header=torch.from_numpy(np.asarray(header, np.int64)).to(DEV))
    for k in ROWS:
        setattr(out, k, torch.from_numpy(ring[k]).to(DEV))
    return out


def _view(torch, rows):
    """host rows (the model's staged minibatch) as a ring the learners read"""
    m = rows["r"].shape[0]
    out = types.SimpleNamespace(capacity=m, size=m)
    for k in ROWS:
        setattr(out, k, torch.from_numpy(np.ascontiguousarray(rows[k])).to(DEV))
    return out


def _draw_with_gaps(B, seed, P=None):
    rng = np.random.RandomState(seed)
    idx = rng.randint(0, CAP_L, (P or 1, B)).astype(np.int32)
    idx[:, ::9] = -1
    idx[:, 5::31] = CAP_L + 3
    return idx if P else idx[0]


def _learner(torch, strategy="double_ref", loss="mse", gamma=0.98):
    from aquaticgymenv_amd.learner import DQNLearner
    from aquaticgymenv_amd.qpolicy import QNetwork
    qnet = QNetwork(L.glorot_layers(3), DEV)
    lrn = DQNLearner(qnet, gamma=gamma, tau=0.05, lr=1e-3, strategy=strategy, seed=17, loss=loss)
    lrn.theta_target.mul_(0.9)                               # the two networks differ, as they do after the first update
    return lrn


def _learner_state(lrn):
    return {"theta": lrn.theta, "theta_target": lrn.theta_target, "m": lrn.m, "v": lrn.v, "t": lrn.t, "blob": lrn.qnet.blob,
            "target_blob": lrn.target_blob, "loss": lrn.loss, "grad": lrn.grad}


def _bank_learners(torch, gamma=(0.98, 0.9, 0.95)):
    from aquaticgymenv_amd.lbank import DQNLearnerBank
    from aquaticgymenv_amd.qbank import QNetworkBank
    bank = QNetworkBank([L.glorot_layers(60 + p) for p in range(3)], 4, DEV)
    lb = DQNLearnerBank(bank, gamma=list(gamma), lr=[1e-3, 3e-3, 1e-2], tau=[0.005, 0.05, 0.5], seed=5)
    lb.theta_target.mul_(0.9)
    return lb


def _bank_state(lb):
    return {"theta": lb.theta, "theta_target": lb.theta_target, "m": lb.m, "v": lb.v, "t": lb.t, "tensor": lb.bank.tensor,
            "target_tensor": lb.target_tensor, "loss": lb.loss, "grad": lb.grad, "hyper": lb.hyper}


def _equal_states(torch, a, b, what):
    for name in a:
        assert torch.equal(a[name], b[name]), (what, name)


@pytest.mark.parametrize("B", [64, 257])
def test_ratio_zero_changes_nothing_for_the_learner(torch, B):
    """relabel with ratio = 0, then update(her.view, B, idx=her.idx): theta, theta_target, m, v, t, both blobs, loss and grad
    bit for bit what update(ring_view, B, idx=idx) leaves from the same start"""
    from aquaticgymenv_amd.hindsight import HindsightReplay
    host, header = _learner_ring()
    ring = _device_ring(torch, host, header)
    idx = torch.from_numpy(_draw_with_gaps(B, B)).to(DEV)
    plain, staged = _learner(torch), _learner(torch)
    her = HindsightReplay(ring, B, ratio=0.0)
    assert tuple(her.idx.shape) == (1, B) and her.threshold == 0
    for call in range(2):
        plain.update(ring, B, idx=idx)
        assert her.relabel(idx, staged) is her.view
        staged.update(her.view, B, idx=her.idx)
        torch.cuda.synchronize()
        _equal_states(torch, _learner_state(plain), _learner_state(staged), (B, call))
    assert int(plain.t[0]) == 2 and 0 < int(her.ok.sum()) < B and float(plain.loss[0]) > 0
    assert not her.k.any() and her.m.any()


@pytest.mark.parametrize("B", [64, 257])
def test_ratio_zero_changes_nothing_for_the_bank(torch, B):
    from aquaticgymenv_amd.hindsight import HindsightReplay
    host, header = _learner_ring()
    ring = _device_ring(torch, host, header)
    idx = torch.from_numpy(_draw_with_gaps(B, B + 1, P=3)).to(DEV)
    plain, staged = _bank_learners(torch), _bank_learners(torch)
    her = HindsightReplay(ring, B, networks=3, ratio=0.0)
    for call in range(2):
        plain.update(ring, B, idx)
        her.relabel(idx, staged)
        staged.update(her.view, B, her.idx)
        torch.cuda.synchronize()
        _equal_states(torch, _bank_state(plain), _bank_state(staged), (B, call))
    assert int(plain.t.min()) == 2 and 0 < int(her.ok.sum()) < 3 * B and not her.k.any()
    # argument errors name the field
    with pytest.raises(ValueError, match="idx"):
        her.relabel(idx[:2], staged)
    with pytest.raises(ValueError, match="idx"):
        her.relabel(idx.long(), staged)
    with pytest.raises(ValueError, match="learner"):
        her.relabel(idx, _learner(torch))                        # one counter for three networks
    with pytest.raises(ValueError, match="learner"):
        her.relabel(idx, object())
    for kw, field in ((dict(batch_size=0), "batch_size"), (dict(networks=0), "networks"), (dict(networks=4097), "networks"),
                      (dict(horizon=0), "horizon"), (dict(horizon=65), "horizon"), (dict(ratio=1.5), "ratio"), (dict(ratio=-0.1), "ratio"),
                      (dict(ratio=float("nan")), "ratio"), (dict(ratio="much"), "ratio")):
        args = dict(batch_size=B)
        args.update(kw)
        with pytest.raises(ValueError, match=field):
            HindsightReplay(ring, **args)
    ring.capacity += 1
    with pytest.raises(ValueError, match="multiple of the batch"):
        HindsightReplay(ring, B)


@pytest.mark.parametrize("strategy,loss", [("double_ref", "mse"), ("fixed", "mse"), ("double_ref", "reference")])
def test_ratio_one_is_the_update_on_the_models_rows(torch, strategy, loss):
    """the update through the relabelling equals DQNLearner.update on a host-built ring that holds the model's staged rows:
    the composition is closed (the target arithmetic itself is the learner's, held to autograd elsewhere)"""
    from aquaticgymenv_amd.hindsight import HindsightReplay
    B = 64
    host, header = _learner_ring()
    ring = _device_ring(torch, host, header)
    draw = _draw_with_gaps(B, 12)
    through, direct = _learner(torch, strategy, loss), _learner(torch, strategy, loss)
    want = M.relabel(host, header, N_L, draw.reshape(1, B), 8, 1.0, [0], [through.seed])
    assert {M.KEPT, M.SUCCESS_K0, M.SHAPED, None} <= set(want["fate"]) and M.NOT_CHOSEN not in want["fate"]
    her = HindsightReplay(ring, B, horizon=8, ratio=1.0)
    her.relabel(torch.from_numpy(draw).to(DEV), through)
    through.update(her.view, B, idx=her.idx)
    direct.update(_view(torch, want), B, idx=torch.arange(B, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    for k in STAGED:
        assert np.array_equal(_bits(getattr(her, k).cpu().numpy()), _bits(want[k])), k
    _equal_states(torch, _learner_state(through), _learner_state(direct), (strategy, loss))
    # and the relabelled rows are used: the ring's own rows give another update
    other = _learner(torch, strategy, loss)
    other.update(ring, B, idx=torch.from_numpy(draw).to(DEV))
    assert not torch.equal(other.theta, through.theta)
    # the next call is keyed by the counter the update has advanced: another draw
    her.relabel(torch.from_numpy(draw).to(DEV), through)
    torch.cuda.synchronize()
    again = M.relabel(host, header, N_L, draw.reshape(1, B), 8, 1.0, [1], [through.seed])
    assert int(through.t[0]) == 1 and np.array_equal(her.k.cpu().numpy(), again["k"]) and not np.array_equal(again["k"], want["k"])


# ------------------------------------------------------------------------------------------------ 4. a real batch
@pytest.mark.parametrize("mode", ["next_step", "same_step"])
def test_a_real_batch(torch, mode):
    """64 worlds with obstacles for 40 steps.  The premise of the rule: wherever d == 0, the new observation of a slot is the
    previous observation of the slot one batch further.  Then the staged rows of a draw over every slot equal the model run on
    the device's own ring, goal columns of s and s2 agree, and every staged success lies within the radius"""
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.hindsight import HindsightReplay
    from aquaticgymenv_amd.learner import DQNLearner
    from aquaticgymenv_amd.qpolicy import QNetwork
    from aquaticgymenv_amd.replay import DeviceReplayRing
    n, steps = 64, 40
    env = BatchedAqua(n, obstacles=True, seed=31, auto_reset=mode, normalized_obs=True, device=DEV)
    env.params.time_limit = 25
    env.reset()
    ring = DeviceReplayRing(env, n * 48)                          # 48 rounds: the ring is not yet full after 40
    rng = np.random.RandomState(2)
    for _ in range(steps):
        action = torch.from_numpy(rng.randint(0, 3, n).astype(np.uint8)).to(DEV)
        ring.before_step(action)
        env.step(action)
        ring.after_step()
    torch.cuda.synchronize()
    host = {k: getattr(ring, k).cpu().numpy() for k in ROWS}
    host["capacity"] = ring.capacity
    header = ring.header.cpu().numpy()
    assert header[0] == steps * n and (host["d"][:steps * n] != 0).sum() > 5
    # the premise: a non-terminal step's s2 is the next step's s (the slot one batch further, where there is one)
    first = np.arange((steps - 1) * n)
    live = (host["d"][first] == 0) & (host["ok"][first] != 0)
    assert live.sum() > 1000
    assert np.array_equal(_bits(host["s2"][:, first[live]]), _bits(host["s"][:, first[live] + n]))
    assert (host["ok"][first[live] + n] != 0).all()
    # the kernel on the device's own ring against the model on its copy: every written slot, and some that are not
    B = steps * n + 64
    qnet = QNetwork(L.glorot_layers(3), DEV)
    learner = DQNLearner(qnet, gamma=0.98, tau=0.05, lr=1e-3, strategy="double_ref", seed=23)
    her = HindsightReplay(ring, B, horizon=32, ratio=0.8)
    idx = torch.arange(B, dtype=torch.int32, device=DEV)
    her.relabel(idx, learner)
    torch.cuda.synchronize()
    want = M.relabel(host, header, n, idx.cpu().numpy().reshape(1, B), 32, 0.8, [0], [23])
    for k in STAGED:
        assert np.array_equal(_bits(getattr(her, k).cpu().numpy()), _bits(want[k])), k
    fates = {f: want["fate"].count(f) for f in set(want["fate"])}
    print("fates:", fates, "cuts:", {c: want["cut"].count(c) for c in set(want["cut"])})
    assert {M.SUCCESS_K0, M.SUCCESS_LATER, M.SHAPED, M.NOT_CHOSEN, M.KEPT, None} == set(fates)
    s, s2, d, k = (getattr(her, name).cpu().numpy() for name in ("s", "s2", "d", "k"))
    # (a terminal step is never relabelled, and in same-step mode its stored s2 is already the observation of the restarted
    # world, with the goal of the next episode: everywhere else the two goals are one)
    own = (k > 0) | (want["d"] == 0) if mode == "same_step" else np.ones(B, bool)
    assert np.array_equal(_bits(s[3:5][:, own]), _bits(s2[3:5][:, own])) and own.sum() > 0.9 * steps * n
    hit, far = (k > 0) & (d == 3), (k > 0) & (d == 0)
    gap = M.gap(s2[0], s2[1], s2[3], s2[4])                       # of the staged rows themselves
    assert hit.sum() > 50 and (gap[hit] <= 0).all() and far.sum() > 50 and (gap[far] > 0).all() and set(d[k > 0]) == {0, 3}


# ------------------------------------------------------------------------------------------------ 5. the loops
WORLDS, BATCH = 64, 64


def _dqn_parts(torch, gamma=0.98):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.learner import DQNLearner
    from aquaticgymenv_amd.qpolicy import QNetwork
    from aquaticgymenv_amd.replay import DeviceReplayRing
    qnet = QNetwork(L.glorot_layers(3), DEV)
    learner = DQNLearner(qnet, gamma=gamma, tau=0.005, lr=1e-3, strategy="double_ref", seed=17)
    env = BatchedAqua(WORLDS, obstacles=True, seed=17, auto_reset="next_step", normalized_obs=True, device=DEV)
    env.params.time_limit = 5
    env.reset()
    ring = DeviceReplayRing(env, WORLDS * 16)
    tracker = EpisodeTracker(env, epsilon=(1.0, 0.05, 0.9))
    return dict(env=env, qnet=qnet, learner=learner, ring=ring, tracker=tracker)


def _her(p, networks=1, batch=BATCH, **kw):
    from aquaticgymenv_amd.hindsight import HindsightReplay
    return HindsightReplay(p["ring"], batch, networks=networks, horizon=kw.pop("horizon", 4), ratio=kw.pop("ratio", 0.8))


def _dqn_loop(p, **kw):
    from aquaticgymenv_amd.trainer import DQNLoop
    return DQNLoop(p["env"], p["qnet"], p["learner"], p["ring"], p["tracker"], BATCH, **kw)


def _dqn_state(p):
    env, ring, tracker, learner = p["env"], p["ring"], p["tracker"], p["learner"]
    out = {"env.state": env.state, "env.time": env.time, "env.obs_norm": env.obs_norm_buf, "qnet.blob": p["qnet"].blob,
           "ring.header": ring.header, "tracker.epsilon": tracker.epsilon, "tracker._counts": tracker._counts}
    for name in ROWS:
        out["ring." + name] = getattr(ring, name)
    for name in ("theta", "theta_target", "m", "v", "t", "target_blob", "loss", "grad"):
        out["learner." + name] = getattr(learner, name)
    return out


def _by_hand(p, her, idx):
    """one iteration call by call: act ... draw, relabel, update"""
    env, qnet, ring, tracker, learner = p["env"], p["qnet"], p["ring"], p["tracker"], p["learner"]
    action = qnet.act(env, epsilon=0.0, out=env.policy_action)
    tracker.explore(env.policy_action)
    ring.before_step(env.policy_action)
    env.step(action)
    ring.after_step()
    tracker.after_step()
    ring.draw(BATCH, learner, out=idx)
    her.relabel(idx, learner)
    learner.update(her.view, BATCH, idx=her.idx)


def test_dqn_loop_with_hindsight_eager_graph_and_by_hand(torch):
    """64 worlds, 16 rounds, B = 64, 40 iterations (the ring wraps twice): step(), the replays of the captured graph and the
    call-by-call composition hold the same bits after every iteration"""
    a, b, c = _dqn_parts(torch), _dqn_parts(torch), _dqn_parts(torch)
    loop_a, loop_b = _dqn_loop(a, hindsight=_her(a)), _dqn_loop(b, hindsight=_her(b))
    assert loop_a.nstep is None and loop_a.hindsight.networks == 1
    hand = _her(c)
    idx = torch.full((BATCH,), -1, dtype=torch.int32, device=DEV)
    before = {k: v.clone() for k, v in _dqn_state(b).items()}
    graph = loop_b.capture()
    torch.cuda.synchronize()
    for k, v in before.items():                                  # the capture and its warm-up left no trace
        assert torch.equal(_dqn_state(b)[k], v), k
    assert not loop_b.hindsight.ok.any() and not loop_b.hindsight.m.any()
    ks, codes = set(), set()
    for it in range(40):
        loop_a.step()
        graph.launch()
        _by_hand(c, hand, idx)
        sa, sb, sc = _dqn_state(a), _dqn_state(b), _dqn_state(c)
        for name in sa:
            assert torch.equal(sa[name], sb[name]), ("the graph differs from step()", name, it)
            assert torch.equal(sa[name], sc[name]), ("the composition differs from step()", name, it)
        for name in STAGED:
            assert torch.equal(getattr(loop_a.hindsight, name), getattr(loop_b.hindsight, name)), (name, it)
            assert torch.equal(getattr(loop_a.hindsight, name), getattr(hand, name)), (name, it)
        her = loop_b.hindsight
        ks |= set(her.k.cpu().numpy().tolist())
        codes |= set(her.d[her.k > 0].cpu().numpy().tolist())
    # (four steps of 0.5 world units stay within the radius of 5: under a goal so near, every relabelled step is a success)
    assert ks == {0, 1, 2, 3, 4} and codes == {3} and int(b["learner"].t[0]) == 40
    assert b["ring"].position() == (40 * WORLDS) % (16 * WORLDS) and b["tracker"].counts()["episodes"] > 0
    graph.close()


P_NETS, SEG = 4, 16


def _population_parts(torch, selector=True):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.lbank import DQNLearnerBank
    from aquaticgymenv_amd.pbt import PopulationSelector
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.replay import DeviceReplayRing
    from aquaticgymenv_amd.segments import SegmentTracker
    bank = QNetworkBank([L.glorot_layers(60 + p) for p in range(P_NETS)], SEG, DEV)
    learners = DQNLearnerBank(bank, gamma=[0.98, 0.9, 0.95, 0.97], lr=[1e-3, 3e-3, 1e-2, 1e-3], tau=[0.005, 0.05, 0.5, 0.01], seed=5)
    env = BatchedAqua(P_NETS * SEG, obstacles=True, seed=23, auto_reset="next_step", normalized_obs=True, device=DEV)
    env.params.time_limit = 4
    env.reset()
    ring = DeviceReplayRing(env, 8 * P_NETS * SEG)
    tracker = EpisodeTracker(env)
    st = SegmentTracker(tracker, SEG, P_NETS, window=100, epsilon=([0.5, 0.1, 1.0, 0.3], [0.05, 0.01, 0.2, 0.05], [0.9, 0.99, 50.0, 0.9]))
    bank.epsilon = st.epsilon
    # ready = 1: a network can be replaced as soon as it has finished one episode, which every world has after four steps
    sel = PopulationSelector(learners, st, ready=1, fraction=0.5, every=1, seed=3) if selector else None
    return dict(env=env, bank=bank, learners=learners, ring=ring, tracker=tracker, st=st, sel=sel)


def _population_loop(p, **kw):
    from aquaticgymenv_amd.trainer import PopulationLoop
    return PopulationLoop(p["env"], p["bank"], p["learners"], p["ring"], p["tracker"], 8, segments=p["st"], selector=p["sel"], **kw)


def _population_state(p, loop):
    env, ring, lb, st, sel = p["env"], p["ring"], p["learners"], p["st"], p["sel"]
    out = {"env.state": env.state, "env.time": env.time, "bank.tensor": p["bank"].tensor, "bank.epsilon": p["bank"].epsilon, "ring.header": ring.header}
    for name in ROWS:
        out["ring." + name] = getattr(ring, name)
    for name in ("theta", "theta_target", "m", "v", "t", "target_tensor", "hyper", "loss", "grad"):
        out["learners." + name] = getattr(lb, name)
    for name in ("header", "mark", "origin", "parent") if sel is not None else ():
        out["selector." + name] = getattr(sel, name)
    out["segments.epsilon"], out["segments._counts"] = st.epsilon, st._counts
    if loop.hindsight is not None:
        for name in STAGED:
            out["hindsight." + name] = getattr(loop.hindsight, name)
    return out


def test_population_loop_with_hindsight_segments_and_a_selector(torch):
    """4 x 16 worlds, segments and a selector: the graph equals step() after every iteration, with a network replaced inside
    the run; the staged rows of the last iteration are the model's on the ring, the draw and the counters as they then were"""
    a, b = _population_parts(torch), _population_parts(torch)
    loop_a, loop_b = _population_loop(a, hindsight=_her(a, P_NETS, 8)), _population_loop(b, hindsight=_her(b, P_NETS, 8))
    assert loop_b.hindsight.networks == P_NETS and tuple(loop_b.hindsight.idx.shape) == (P_NETS, 8)
    before = {k: v.clone() for k, v in _population_state(b, loop_b).items()}
    graph = loop_b.capture()
    torch.cuda.synchronize()
    for k, v in before.items():                                      # the capture and its warm-up left no trace
        assert torch.equal(_population_state(b, loop_b)[k], v), k
    relabelled = 0
    for it in range(20):
        loop_a.step()
        graph.launch()
        sa, sb = _population_state(a, loop_a), _population_state(b, loop_b)
        for name in sa:
            assert torch.equal(sa[name], sb[name]), ("the graph differs from step()", name, it)
        relabelled += int((loop_b.hindsight.k > 0).sum())
    report = b["sel"].report()
    assert report["replaced"] >= 1 and relabelled > 50, (report, relabelled)
    # the last iteration against the model: the ring is not written between the relabelling and this read, and the update has
    # advanced the counter of every network whose minibatch held a sample (the selector copies counters BEFORE the draw)
    her = loop_b.hindsight
    t_used = b["learners"].t.cpu().numpy() - her.ok.reshape(P_NETS, 8).any(dim=1).cpu().numpy().astype(np.int64)
    host = {k: getattr(b["ring"], k).cpu().numpy() for k in ROWS}
    host["capacity"] = b["ring"].capacity
    want = M.relabel(host, b["ring"].header.cpu().numpy(), P_NETS * SEG, loop_b.idx.cpu().numpy(), 4, 0.8, t_used,
                     b["learners"].seed_dev.cpu().numpy().view(np.uint64))
    for k in STAGED:
        assert np.array_equal(_bits(getattr(loop_b.hindsight, k).cpu().numpy()), _bits(want[k])), k
    graph.close()


def _node_count(torch, loop):
    """the nodes of the graph that loop.capture() captures: the same warm-up, the same queue, captured here and counted"""
    # (the HIP runtime this process already runs on, by the path it was loaded from: not a second copy)
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert len(paths) == 1, paths
    hip = ctypes.CDLL(paths[0])
    env = loop.env
    graph, count = ctypes.c_void_p(), ctypes.c_size_t(0)
    with torch.cuda.device(env.device):
        env._sync_device_tick()
        loop._warm_up()
        env._sync_device_tick()
        cap = torch.cuda.Stream(device=env.device)
        cap.wait_stream(torch.cuda.current_stream(env.device))
        with torch.cuda.stream(cap):
            stream = ctypes.c_void_p(cap.cuda_stream)
            assert hip.hipStreamBeginCapture(stream, 1) == 0         # hipStreamCaptureModeThreadLocal
            try:
                loop._queue()
            finally:
                rc = hip.hipStreamEndCapture(stream, ctypes.byref(graph))
            assert rc == 0
        torch.cuda.current_stream(env.device).wait_stream(cap)
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(count)) == 0
    assert hip.hipGraphDestroy(graph) == 0
    loop.ring._open = False
    return int(count.value)


def test_hindsight_is_one_node_more_and_none_builds_nothing(torch, monkeypatch):
    """hindsight=None: no HindsightReplay is built and the graph has the nodes it had -- eleven for DQNLoop, thirteen for
    PopulationLoop with segments and a selector; hindsight= adds exactly one.  The combinations out of scope are ValueErrors"""
    from aquaticgymenv_amd import hindsight as hindsight_module
    built = []
    real = hindsight_module.HindsightReplay.__init__
    monkeypatch.setattr(hindsight_module.HindsightReplay, "__init__", lambda self, *args, **kw: (built.append(1), real(self, *args, **kw))[1])
    one, explicit = _dqn_loop(_dqn_parts(torch)), _dqn_loop(_dqn_parts(torch), hindsight=None)
    pop = _population_loop(_population_parts(torch))
    assert built == [] and one.hindsight is None and explicit.hindsight is None and pop.hindsight is None
    p, q = _dqn_parts(torch), _population_parts(torch)
    with_her, pop_her = _dqn_loop(p, hindsight=_her(p)), _population_loop(q, hindsight=_her(q, P_NETS, 8))
    assert built == [1, 1]
    counts = [_node_count(torch, loop) for loop in (one, explicit, with_her, pop, pop_her)]
    print("graph nodes:", counts)
    assert counts == [11, 11, 12, 13, 14]
    # out of scope, and said so
    p = _dqn_parts(torch)
    with pytest.raises(ValueError, match="n_step"):
        _dqn_loop(p, n_step=3, hindsight=_her(p))
    q = _population_parts(torch)
    with pytest.raises(ValueError, match="n_step"):
        _population_loop(q, n_step=2, hindsight=_her(q, P_NETS, 8))
    from aquaticgymenv_amd.priority import PrioritizedReplay
    q = _population_parts(torch)
    per = PrioritizedReplay(q["ring"], q["learners"])
    with pytest.raises(ValueError, match="priorities"):
        _population_loop(q, priorities=per, hindsight=_her(q, P_NETS, 8))
    # a HindsightReplay of another ring, another batch size or another number of networks is not this loop's
    p, other = _dqn_parts(torch), _dqn_parts(torch)
    with pytest.raises(ValueError, match="ring"):
        _dqn_loop(p, hindsight=_her(other))
    with pytest.raises(ValueError, match="samples"):
        _dqn_loop(p, hindsight=_her(p, batch=32))
    with pytest.raises(ValueError, match="samples"):
        _dqn_loop(p, hindsight=_her(p, networks=2))
    with pytest.raises(ValueError, match="HindsightReplay"):
        _dqn_loop(p, hindsight=object())
