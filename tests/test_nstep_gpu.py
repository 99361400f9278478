"""GPU tests of libaqua_nstep.so (aquaticgymenv_amd/csrc/aqua_nstep.h), NStepReturns (aquaticgymenv_amd/nstep.py), the
learners' gamma= / hyper= keywords and the loops' n_step= (aquaticgymenv_amd/trainer.py).

The fold copies rows, walks integers and sums rounded float64 products in a fixed order, and the learners are deterministic:
every comparison is of bit patterns, against the numpy model of tests/_nstep_model.py or between two runs on the device.  No
tolerance anywhere."""
import ctypes
import types

import numpy as np
import pytest

from tests import _learner as L
from tests import _nstep_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = ("s", "a", "r", "s2", "d", "ok")


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


@pytest.fixture(scope="module")
def capi():
    from aquaticgymenv_amd import _nstep_capi
    return _nstep_capi


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


# ------------------------------------------------------------------------------------------------ 1. the fold against the model
POISON = 0x5A


def _run_fold(torch, capi, ring, header, N, idx, n, gamma=None, hyper=None, guard=5, with_len=True):
    """aquanst_fold through the C ABI on a host ring -> the model's dict of outputs, read back.  The staged rows have the
    pitch P B + guard and start poisoned; the guard columns (and a guard row behind the derived table) must come back so."""
    P, B = idx.shape
    m, ld = P * B, P * B + guard
    cont = ring["a"].ndim == 2
    dev = {k: torch.from_numpy(np.ascontiguousarray(ring[k])).to(DEV) for k in ROWS}
    hdr = torch.from_numpy(np.asarray(header, np.int64)).to(DEV)
    idx_dev = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(DEV)
    u8 = lambda *shape: torch.full(shape, POISON, dtype=torch.uint8, device=DEV)        # noqa: E731
    out = dict(s=u8(5, ld * 4), s2=u8(5, ld * 4), r=u8(ld * 4), a=u8(2, ld * 4) if cont else u8(ld), d=u8(ld), ok=u8(ld), len=u8(ld))
    table = None if hyper is None else torch.from_numpy(np.ascontiguousarray(hyper, np.float64)).to(DEV)
    derived = None if hyper is None else u8(P + 1, 8 * 8)
    rc = capi.lib.aquanst_fold(hdr.data_ptr(), dev["s"].data_ptr(), dev["a"].data_ptr(), dev["r"].data_ptr(), dev["s2"].data_ptr(),
                               dev["d"].data_ptr(), dev["ok"].data_ptr(), ring["s"].shape[1], ring["capacity"], 1 if cont else 0, N,
                               idx_dev.data_ptr(), P, B, n, capi.NO_GAMMA if hyper is not None else gamma,
                               None if table is None else table.data_ptr(),
                               out["s"].data_ptr(), out["a"].data_ptr(), out["r"].data_ptr(), out["s2"].data_ptr(), out["d"].data_ptr(),
                               out["ok"].data_ptr(), ld, out["len"].data_ptr() if with_len else None,
                               None if derived is None else derived.data_ptr(), None)
    capi.check(rc, "aquanst_fold")
    torch.cuda.synchronize()
    for k in ROWS:                                            # the ring is read only
        assert np.array_equal(_bits(dev[k].cpu().numpy()), _bits(ring[k])), k
    assert hdr.cpu().numpy().tolist() == list(header)
    got = {}
    for k, t in out.items():
        host = t.cpu().numpy()
        f32 = k in ("s", "s2", "r") or (k == "a" and cont)
        host = host.view(np.float32) if f32 else host
        if k == "len" and not with_len:
            assert (host == POISON).all()
            continue
        assert (_bits(host[..., m:]) == POISON).all(), ("guard columns", k)
        got[k] = np.ascontiguousarray(host[..., :m])
    if derived is not None:
        d = derived.cpu().numpy()
        assert (d[P] == POISON).all() and np.array_equal(table.cpu().numpy(), hyper)
        got["hyper"] = d[:P].view(np.float64)
    return got


def _same(got, want, what):
    for k, v in got.items():
        assert np.array_equal(_bits(v), _bits(want[k])), (what, k, v, want[k])


# not yet full, just full, wrapped mid-ring, and a cursor that is no multiple of N
HEADERS = ((21, 21, 14, 3), (0, 42, 35, 6), (14, 42, 7, 8), (15, 42, 8, 8))


@pytest.mark.parametrize("continuous", [False, True], ids=["u8", "f32x2"])
def test_fold_equals_the_model_bit_for_bit(torch, capi, continuous):
    """N = 7, capacity 42 (six rounds) with the pitch 48, P = 3, B = 37: every slot, both neighbours of the range and far
    outside it, for every header and n in {1, 2, 3, 5, 8} (8 exceeds the rounds), with gamma from a table of three different
    values and as a scalar.  Every branch of the window rule occurs, by the model's own naming."""
    ring = M.crafted_ring(continuous=continuous, ld=48)
    rng = np.random.RandomState(3)
    idx = np.concatenate([np.arange(42), [-1, 42, 43, 47, 10 ** 6, -2 ** 31, 2 ** 31 - 1], rng.randint(0, 42, 111 - 49)]).astype(np.int32)
    idx = idx[rng.permutation(111)].reshape(3, 37)
    hyper = np.arange(24, dtype=np.float64).reshape(3, 8) / 7 + 2
    hyper[:, 0] = (0.98, 0.5, 0.999)
    seen, wrapped = {}, 0
    for header in HEADERS:
        for n in (1, 2, 3, 5, 8):
            want = M.fold(ring, header, 7, idx, n, hyper=hyper)
            _same(_run_fold(torch, capi, ring, header, 7, idx, n, hyper=hyper), want, (header, n, "table"))
            for branch in want["branch"]:
                seen[branch] = seen.get(branch, 0) + 1
            wrapped += sum(want["wrapped"])
            if n == 1:
                assert np.array_equal(want["hyper"][:, 0], np.float32([0.98, 0.5, 0.999]).astype(np.float64))
            want = M.fold(ring, header, 7, idx, n, gamma=0.9)
            _same(_run_fold(torch, capi, ring, header, 7, idx, n, gamma=0.9, with_len=(n != 3)), want, (header, n, "scalar"))
            if header[0] % 7:
                assert set(want["branch"]) == {M.BAD_CURSOR} and not want["ok"].any()
    print("branches:", seen, "wrapped windows:", wrapped)
    assert set(seen) == {M.FULL, M.DONE_FIRST, M.DONE_MIDDLE, M.DONE_LAST, M.FRONTIER, M.BROKEN, M.NOT_OK, M.OUTSIDE, M.BAD_CURSOR}
    assert min(seen.values()) >= 3 and wrapped >= 3


def test_fold_past_the_grid_cap(torch, capi):
    """P = 1 and B one block above MAX_BLOCKS x BLOCK, + 5: the grid-stride loop takes a second turn for some threads and
    not for others.  The model is evaluated once per distinct slot and spread over the draw."""
    B = capi.MAX_BLOCKS * capi.BLOCK + capi.BLOCK + 5
    assert B <= capi.MAX_BATCH
    ring = M.crafted_ring()
    header = (14, 42, 7, 8)
    probe = np.arange(-1, 43, dtype=np.int32).reshape(1, -1)
    per_slot = M.fold(ring, header, 7, probe, 2, gamma=0.98)
    assert len(set(per_slot["branch"])) >= 6
    rng = np.random.RandomState(8)
    idx = rng.randint(-1, 43, B).astype(np.int32).reshape(1, B)
    idx[0, -1], idx[0, capi.MAX_BLOCKS * capi.BLOCK] = 21, 0        # a full window in the last sample and in the first of the second turn
    got = _run_fold(torch, capi, ring, header, 7, idx, 2, gamma=0.98, guard=3)
    at = idx[0] + 1
    for k in ROWS + ("len",):
        assert np.array_equal(_bits(got[k]), _bits(per_slot[k][..., at])), k
    assert got["ok"][-1] == 1 and got["len"][-1] == 2 and got["len"][capi.MAX_BLOCKS * capi.BLOCK] == 2


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
    """the host ring as NStepReturns and the learners read a DeviceReplayRing: its rows, header, capacity and env"""
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
def test_n_equal_one_changes_nothing_for_the_learner(torch, B):
    """fold with n = 1, then update(nstep.view, B, idx=nstep.idx, gamma=nstep.discount(gamma)): theta, theta_target, m, v, t,
    both blobs, loss and grad bit for bit what update(ring_view, B, idx=idx) leaves from the same start"""
    from aquaticgymenv_amd.nstep import NStepReturns
    host, header = _learner_ring()
    ring = _device_ring(torch, host, header)
    idx = torch.from_numpy(_draw_with_gaps(B, B)).to(DEV)
    plain, staged = _learner(torch), _learner(torch)
    nstep = NStepReturns(ring, 1, B)
    assert nstep.discount(0.98) == float(np.float32(0.98)) and tuple(nstep.idx.shape) == (1, B)
    for call in range(2):
        plain.update(ring, B, idx=idx)
        assert nstep.fold(idx, gamma=staged.gamma) is nstep.view
        staged.update(nstep.view, B, idx=nstep.idx, gamma=nstep.discount(staged.gamma))
        torch.cuda.synchronize()
        _equal_states(torch, _learner_state(plain), _learner_state(staged), (B, call))
    assert int(plain.t[0]) == 2 and 0 < int(nstep.ok.sum()) < B and float(plain.loss[0]) > 0
    assert torch.equal(nstep.length, nstep.ok)


@pytest.mark.parametrize("B", [64, 257])
def test_n_equal_one_changes_nothing_for_the_bank(torch, B):
    from aquaticgymenv_amd.nstep import NStepReturns
    host, header = _learner_ring()
    ring = _device_ring(torch, host, header)
    idx = torch.from_numpy(_draw_with_gaps(B, B + 1, P=3)).to(DEV)
    plain, staged = _bank_learners(torch), _bank_learners(torch)
    nstep = NStepReturns(ring, 1, B, networks=3)
    for call in range(2):
        plain.update(ring, B, idx)
        nstep.fold(idx, hyper=staged.hyper)
        staged.update(nstep.view, B, nstep.idx, hyper=nstep.hyper)
        torch.cuda.synchronize()
        _equal_states(torch, _bank_state(plain), _bank_state(staged), (B, call))
    assert torch.equal(nstep.hyper[:, 1:], staged.hyper[:, 1:])
    assert nstep.hyper[:, 0].cpu().numpy().tolist() == np.float32([0.98, 0.9, 0.95]).astype(np.float64).tolist()
    assert int(plain.t.min()) == 2 and 0 < int(nstep.ok.sum()) < 3 * B
    with pytest.raises(ValueError):
        staged.update(nstep.view, B, nstep.idx, hyper=nstep.hyper[:2])
    with pytest.raises(ValueError):
        staged.update(nstep.view, B, nstep.idx, hyper=nstep.hyper.float())
    with pytest.raises(ValueError):
        nstep.fold(idx)
    with pytest.raises(ValueError):
        nstep.fold(idx, gamma=0.9, hyper=staged.hyper)
    with pytest.raises(ValueError):
        nstep.fold(idx[:2], hyper=staged.hyper)


@pytest.mark.parametrize("strategy,loss", [("double_ref", "mse"), ("fixed", "mse"), ("double_ref", "reference")])
def test_n_equal_three_is_the_n_step_target(torch, strategy, loss):
    """the update through the fold equals DQNLearner.update on a host-built ring that holds the model's staged rows, with the
    model's gamma^3: the composition is closed (the target arithmetic itself is the learner's, held to autograd elsewhere)"""
    from aquaticgymenv_amd.nstep import NStepReturns
    B, gamma = 64, 0.98
    host, header = _learner_ring()
    ring = _device_ring(torch, host, header)
    draw = _draw_with_gaps(B, 12)
    want = M.fold(host, header, N_L, draw.reshape(1, B), 3, gamma=gamma)
    assert {M.FULL, M.DONE_FIRST, M.DONE_MIDDLE, M.DONE_LAST, M.FRONTIER, M.BROKEN, M.OUTSIDE} <= set(want["branch"])
    through, direct = _learner(torch, strategy, loss, gamma), _learner(torch, strategy, loss, gamma)
    nstep = NStepReturns(ring, 3, B)
    nstep.fold(torch.from_numpy(draw).to(DEV), gamma=gamma)
    through.update(nstep.view, B, idx=nstep.idx, gamma=nstep.discount(gamma))
    g3 = float(M.discount(gamma, 3))
    assert g3 == nstep.discount(gamma) and g3 != float(np.float32(gamma))
    direct.update(_view(torch, want), B, idx=torch.arange(B, dtype=torch.int32, device=DEV), gamma=g3)
    torch.cuda.synchronize()
    for k in ROWS:
        assert np.array_equal(_bits(getattr(nstep, k).cpu().numpy()), _bits(want[k])), k
    assert np.array_equal(nstep.length.cpu().numpy(), want["len"])
    _equal_states(torch, _learner_state(through), _learner_state(direct), (strategy, loss))
    # and the discount is used: the same rows with the one-step gamma give another update
    other = _learner(torch, strategy, loss, gamma)
    other.update(nstep.view, B, idx=nstep.idx)
    assert not torch.equal(other.theta, through.theta)


# ------------------------------------------------------------------------------------------------ 4. and 6. the loops
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


def _by_hand(p, nstep, idx):
    """one iteration call by call: act ... draw, fold, update"""
    env, qnet, ring, tracker, learner = p["env"], p["qnet"], p["ring"], p["tracker"], p["learner"]
    action = qnet.act(env, epsilon=0.0, out=env.policy_action)
    tracker.explore(env.policy_action)
    ring.before_step(env.policy_action)
    env.step(action)
    ring.after_step()
    tracker.after_step()
    ring.draw(BATCH, learner, out=idx)
    nstep.fold(idx, gamma=learner.gamma)
    learner.update(nstep.view, BATCH, idx=nstep.idx, gamma=nstep.discount(learner.gamma))


def test_dqn_loop_with_three_steps_eager_graph_and_by_hand(torch):
    """64 worlds, 16 rounds, B = 64, 40 iterations (the ring wraps twice): step(), the replays of the captured graph and the
    call-by-call composition hold the same bits after every iteration"""
    from aquaticgymenv_amd.nstep import NStepReturns
    a, b, c = _dqn_parts(torch), _dqn_parts(torch), _dqn_parts(torch)
    loop_a, loop_b = _dqn_loop(a, n_step=3), _dqn_loop(b, n_step=3)
    assert loop_a.n_step == 3 and loop_a.nstep.n == 3 and loop_a.nstep.networks == 1
    hand = NStepReturns(c["ring"], 3, BATCH)
    idx = torch.full((BATCH,), -1, dtype=torch.int32, device=DEV)
    before = {k: v.clone() for k, v in _dqn_state(b).items()}
    graph = loop_b.capture()
    torch.cuda.synchronize()
    for k, v in before.items():                                  # the capture and its warm-up left no trace
        assert torch.equal(_dqn_state(b)[k], v), k
    assert not loop_b.nstep.ok.any() and not loop_b.nstep.hyper.any()
    lengths, empty = set(), 0
    for it in range(40):
        loop_a.step()
        graph.launch()
        _by_hand(c, hand, idx)
        sa, sb, sc = _dqn_state(a), _dqn_state(b), _dqn_state(c)
        for name in sa:
            assert torch.equal(sa[name], sb[name]), ("the graph differs from step()", name, it)
            assert torch.equal(sa[name], sc[name]), ("the composition differs from step()", name, it)
        for name in ROWS + ("length",):
            assert torch.equal(getattr(loop_a.nstep, name), getattr(loop_b.nstep, name)), (name, it)
            assert torch.equal(getattr(loop_a.nstep, name), getattr(hand, name)), (name, it)
        lengths |= set(loop_b.nstep.length.cpu().numpy().tolist())
        empty += int(not loop_b.nstep.ok.any())
        if it == 0:                                              # one round in the ring and nobody done: no window of three closes
            assert not loop_b.nstep.ok.any() and int(b["learner"].t[0]) == 0
    # (a minibatch without a sample is no update: the learner's t counts the others)
    assert lengths == {0, 1, 2, 3} and 1 <= empty <= 2 and int(b["learner"].t[0]) == 40 - empty and b["ring"].position() == (40 * WORLDS) % (16 * WORLDS)
    assert 0 < int((b["ring"].ok == 0).sum()) and b["tracker"].counts()["episodes"] > 0
    graph.close()


def test_a_graph_keeps_the_discount_of_its_capture(torch):
    """DQNLoop passes gamma and gamma^n by value: a replay sees a change of learner.gamma only through a re-capture.  The
    graph captured with 0.98 goes on as the eager loop that keeps 0.98; captured again it goes on as the eager loop with 0.9."""
    a, b = _dqn_parts(torch), _dqn_parts(torch)
    loop_a, loop_b = _dqn_loop(a, n_step=3), _dqn_loop(b, n_step=3)
    graph = loop_b.capture()
    for it in range(8):
        if it == 4:
            b["learner"].gamma = 0.9                                 # the graph does not see it
        loop_a.step()
        graph.launch()
        _equal_states(torch, _dqn_state(a), _dqn_state(b), it)
    graph.close()
    a["learner"].gamma = 0.9
    theta = a["learner"].theta.clone()
    graph = loop_b.capture()
    for it in range(4):
        loop_a.step()
        graph.launch()
        _equal_states(torch, _dqn_state(a), _dqn_state(b), ("recaptured", it))
    graph.close()
    # and 0.9 is another training than 0.98: from the same state, one eager iteration each
    c, d = _dqn_parts(torch), _dqn_parts(torch)
    d["learner"].gamma = 0.9
    loop_c, loop_d = _dqn_loop(c, n_step=3), _dqn_loop(d, n_step=3)
    for it in range(6):
        loop_c.step()
        loop_d.step()
    assert not torch.equal(c["learner"].theta, d["learner"].theta) and not torch.equal(theta, a["learner"].theta)


P_NETS, SEG = 4, 16


def test_a_graph_reads_the_bank_table_where_it_lives(torch):
    """PopulationLoop hands the fold the learners' device table: a row rewritten between two replays is the one the next
    replay derives gamma^n from and bootstraps with -- no re-capture (unlike DQNLoop's gamma, passed by value)"""
    a, b = _population_parts(torch, selector=False), _population_parts(torch, selector=False)
    loop_a, loop_b = _population_loop(a, n_step=2), _population_loop(b, n_step=2)
    graph = loop_b.capture()
    for it in range(10):
        if it == 6:
            for p in (a, b):
                p["learners"].set_hyper(1, gamma=0.75)
        loop_a.step()
        graph.launch()
        _equal_states(torch, _population_state(a, loop_a), _population_state(b, loop_b), it)
        want = [0.98, 0.9 if it < 6 else 0.75, 0.95, 0.97]
        assert loop_b.nstep.hyper[:, 0].cpu().numpy().tolist() == [float(M.discount(g, 2)) for g in want], it
        assert b["learners"].hyper[:, 0].cpu().numpy().tolist() == want, it
    graph.close()


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
    if loop.nstep is not None:
        for name in ROWS + ("length", "hyper"):
            out["nstep." + name] = getattr(loop.nstep, name)
    return out


def _derived(torch, table, n):
    return torch.from_numpy(M.derived_table(table.cpu().numpy(), n)).to(DEV)


def test_population_loop_with_two_steps_and_a_selector(torch):
    """4 x 16 worlds, n_step = 2, segments and a selector: the graph equals step() after every iteration; a network is
    replaced inside the run and its gamma perturbed, and the table the update read is the model's derivation of the table the
    selector left, which the fold itself does not touch."""
    a, b = _population_parts(torch), _population_parts(torch)
    loop_a, loop_b = _population_loop(a, n_step=2), _population_loop(b, n_step=2)
    assert loop_b.nstep.networks == P_NETS and tuple(loop_b.nstep.idx.shape) == (P_NETS, 8)
    table0 = b["learners"].hyper.clone()
    before = {k: v.clone() for k, v in _population_state(b, loop_b).items()}
    graph = loop_b.capture()
    torch.cuda.synchronize()
    for k, v in before.items():                                      # the capture and its warm-up left no trace
        assert torch.equal(_population_state(b, loop_b)[k], v), k
    perturbed_at = None
    for it in range(20):
        loop_a.step()
        graph.launch()
        sa, sb = _population_state(a, loop_a), _population_state(b, loop_b)
        for name in sa:
            assert torch.equal(sa[name], sb[name]), ("the graph differs from step()", name, it)
        table = b["learners"].hyper
        assert torch.equal(loop_b.nstep.hyper, _derived(torch, table, 2)), it
        if perturbed_at is None and not torch.equal(table[:, 0], table0[:, 0]):
            perturbed_at = it
    report = b["sel"].report()
    assert report["replaced"] >= 1 and perturbed_at is not None, (report, perturbed_at)
    assert set(loop_b.nstep.length.cpu().numpy().tolist()) <= {0, 1, 2} and int(loop_b.nstep.ok.sum()) > 0
    # the fold by itself leaves the learners' table alone
    table = b["learners"].hyper.clone()
    loop_b.nstep.fold(loop_b.idx, hyper=b["learners"].hyper)
    torch.cuda.synchronize()
    assert torch.equal(b["learners"].hyper, table) and torch.equal(loop_b.nstep.hyper, _derived(torch, table, 2))
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


def test_one_step_loops_are_the_chains_they_were(torch, monkeypatch):
    """n_step = 1: no NStepReturns is built and the graph has the nodes it had -- eleven for DQNLoop, thirteen for
    PopulationLoop with segments and a selector (the docstrings' counts); n_step > 1 adds exactly one"""
    from aquaticgymenv_amd import nstep as nstep_module
    built = []
    real = nstep_module.NStepReturns.__init__
    monkeypatch.setattr(nstep_module.NStepReturns, "__init__", lambda self, *args, **kw: (built.append(1), real(self, *args, **kw))[1])
    one, explicit = _dqn_loop(_dqn_parts(torch)), _dqn_loop(_dqn_parts(torch), n_step=1)
    pop = _population_loop(_population_parts(torch))
    assert built == [] and one.nstep is None and explicit.nstep is None and pop.nstep is None and one.n_step == pop.n_step == 1
    three, pop2 = _dqn_loop(_dqn_parts(torch), n_step=3), _population_loop(_population_parts(torch), n_step=2)
    assert built == [1, 1]
    counts = [_node_count(torch, loop) for loop in (one, explicit, three, pop, pop2)]
    print("graph nodes:", counts)
    assert counts == [11, 11, 12, 13, 14]
    # DQNLoop asks for whole rounds only when it folds
    from aquaticgymenv_amd.replay import DeviceReplayRing
    p = _dqn_parts(torch)
    p["ring"] = DeviceReplayRing(p["env"], WORLDS * 16 + 1)
    assert _dqn_loop(p).nstep is None
    with pytest.raises(ValueError, match="multiple of the batch"):
        _dqn_loop(p, n_step=2)
    for bad in (0, -1, 33):
        with pytest.raises(ValueError):
            _dqn_loop(_dqn_parts(torch), n_step=bad)
