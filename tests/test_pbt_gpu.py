"""GPU tests of libaqua_pbt.so (aquaticgymenv_amd/include/aqua_pbt.h), PopulationSelector (aquaticgymenv_amd/pbt.py) and
PopulationLoop(selector=...).  The synthetic cases give every stacked array a value distinct per (array, network, element)
and one poisoned guard row behind row P - 1, so that a wrong row, a short copy or an overrun shows; every buffer a call
may write is compared bit for bit with the numpy model of tests/_pbt.py after every call."""
import types

import numpy as np
import pytest

from tests import _learner as L
from tests import _pbt as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BLOB = 4804               # floats of an acting blob (aqua_bank.h)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


class Rig(object):
    """A learner bank and a segment tracker that are nothing but their device buffers (each with a guard row), a real
    PopulationSelector on them, and the model beside them."""

    def __init__(self, torch, P, eps=True, score="mean_return", **config):
        from aquaticgymenv_amd.lbank import DQNLearnerBank
        from aquaticgymenv_amd.pbt import PopulationSelector
        from aquaticgymenv_amd.segments import SegmentTracker
        self.torch, self.P = torch, P
        self.model = model = T.fill(T.Model(P, BLOB, eps=eps, **config))
        self.guards = {}
        dev = torch.device(DEV)
        lb = DQNLearnerBank.__new__(DQNLearnerBank)
        lb.torch, lb.device, lb.networks, lb.seg, lb.blob_floats = torch, dev, P, 1, BLOB
        for name in ("theta", "theta_target", "m", "v"):
            setattr(lb, name, self._guarded(name, getattr(model, name)))
        lb.t = self._guarded("t", model.t.view(np.int64))
        lb.bank = types.SimpleNamespace(tensor=self._guarded("blob_online", model.blob_online).view(torch.uint8))
        lb.target_tensor = self._guarded("blob_target", model.blob_target).view(torch.uint8)
        lb.hyper = self._guarded("hyper", model.hyper)
        lb._hyper_host = model.hyper[:, :6].copy()
        st = SegmentTracker.__new__(SegmentTracker)
        st.torch, st.device, st.seg, st.segments = torch, dev, 1, P
        st.mean_return = self._guarded("mean_return", np.zeros(P, dtype=np.float32))
        st.success_rate = self._guarded("success_rate", np.zeros(P, dtype=np.float32))
        st._counts = self._guarded("counts", np.zeros((P, 8), dtype=np.int64))
        st._eps_state = self._guarded("eps_state", model.eps_state) if eps else None
        st.epsilon = self._guarded("eps_out", model.eps_out) if eps else None
        self.lb, self.st = lb, st
        self.sel = sel = PopulationSelector(lb, st, score=score, **config)
        for name in ("mark", "origin", "parent"):                    # the selector's own buffers get guard rows as well
            setattr(sel, name, self._guarded(name, getattr(sel, name).cpu().numpy()))
        self.score = getattr(st, score)

    def _guarded(self, name, host):
        """the array on the device with one more row behind it, poisoned -> the view of the rows in front of it"""
        host = np.ascontiguousarray(host)
        poison = np.full(host[:1].nbytes, 0x5A, dtype=np.uint8).view(host.dtype).reshape(host[:1].shape)
        whole = self.torch.from_numpy(np.concatenate([host, poison])).to(DEV)
        self.guards[name] = whole
        return whole[:len(host)]

    def set(self, score, episodes):
        torch = self.torch
        counts = np.zeros((self.P, 8), dtype=np.uint64)
        counts[:, 0] = episodes
        counts[:, 1:] = 7                                            # the other words are not the library's business
        self.score.copy_(torch.from_numpy(np.ascontiguousarray(score, dtype=np.float32)))
        self.st._counts.copy_(torch.from_numpy(counts.view(np.int64)))
        self.inputs = (np.ascontiguousarray(score, dtype=np.float32), counts)

    def snapshot(self):
        return {name: whole.clone() for name, whole in self.guards.items()}

    def check(self, what=""):
        """the model takes the call the device has taken; every buffer, the inputs and the guard rows"""
        self.model.select(*self.inputs)
        bad = T.differences(self.sel, self.lb, self.model)
        assert bad == [], (what, bad)
        assert np.array_equal(self.score.cpu().numpy().view(np.uint32), self.inputs[0].view(np.uint32)), what
        assert np.array_equal(self.st._counts.cpu().numpy().view(np.uint64), self.inputs[1]), what
        for name, whole in self.guards.items():
            assert bool((whole[self.P:].contiguous().view(self.torch.uint8) == 0x5A).all()), ("guard row", name, what)


def scenario(P, seed):
    """scores with ties, negatives and both zeros; episode counts that leave some networks unscored and, with ready = 5, some
    of the worst not ready"""
    rng = np.random.RandomState(seed)
    score = rng.choice(np.array([-2.5, -0.0, 0.0, 0.5, 0.5, 1.0, 3.25], dtype=np.float32), P)
    some = rng.rand(P) < 0.4
    score[some] = rng.uniform(-3.0, 3.0, P).astype(np.float32)[some]
    episodes = rng.choice(np.array([0, 1, 2, 5, 6, 50, 200], dtype=np.uint64), P)
    return score, episodes


@pytest.mark.parametrize("fraction", [0.2, 0.5])
@pytest.mark.parametrize("P", [1, 2, 5, 64, 65, 257, 4096])
def test_one_call_against_the_model(torch, P, fraction):
    rig = Rig(torch, P, fraction=fraction, ready=5, seed=1000 + P)
    rig.set(*scenario(P, P))
    rig.sel.select()
    rig.check((P, fraction))
    m = rig.model
    S = int(m.header[3])
    assert S == int((rig.inputs[1][:, 0] >= 1).sum()) and int(m.header[0]) == 1
    if P >= 64:                                                      # the case holds what it is meant to hold
        k = int(fraction * S)
        assert S < P and 0 < len(m.losers) < k and len(m.winners) == k


@pytest.mark.parametrize("P", [5, 65])
def test_all_scores_equal(torch, P):
    """ties everywhere: the ranking is the index order, the first half wins and the second half loses"""
    for value in (0.25, -0.0):
        rig = Rig(torch, P, fraction=0.5, ready=1, seed=5, score="success_rate")
        rig.set(np.full(P, value, dtype=np.float32), np.full(P, 3, dtype=np.uint64))
        rig.sel.select()
        rig.check((P, value))
        assert rig.model.winners == list(range(P // 2)) and rig.model.losers == list(range(P - P // 2, P))


def test_four_calls_marks_carry_over(torch):
    """a child drops out of the losers until it has finished `ready` episodes of its own; then it is replaced again"""
    P = 64
    rig = Rig(torch, P, fraction=0.25, ready=4, seed=9)
    score = -np.arange(P, dtype=np.float32)                          # the worst are 48 .. 63, call after call
    replaced = []
    for call, episodes in enumerate((10, 12, 13, 14)):
        rig.set(score, np.full(P, episodes, dtype=np.uint64))
        rig.sel.select()
        rig.check(call)
        replaced.append(int(rig.model.header[2]))
    assert replaced == [16, 0, 0, 16] and rig.model.header.tolist() == [4, 32, 16, 64]
    assert rig.model.mark[48:].tolist() == [14] * 16 and rig.model.mark[:48].tolist() == [0] * 48
    report = rig.sel.report()
    assert (report["calls"], report["replaced"], report["last"], report["scored"]) == (4, 32, 16, 64)
    assert np.array_equal(report["origin"], rig.model.origin) and np.array_equal(report["parent"], rig.model.parent)
    assert set(report["origin"][48:].tolist()) <= set(range(16)) and report["origin"][:48].tolist() == list(range(48))
    for p in (0, 50, 63):                                            # report() has brought the host copy of the table up to date
        assert rig.lb.hyper_of(p)["lr"] == float(rig.model.hyper[p, 2]) and rig.lb.hyper_of(p)["gamma"] == float(rig.model.hyper[p, 0])


def test_every_third_call_acts(torch):
    P = 65
    rig = Rig(torch, P, fraction=0.5, ready=1, every=3, seed=2)
    score, _ = scenario(P, 77)
    rig.set(score, np.full(P, 2, dtype=np.uint64))
    rig.sel.select()
    rig.check(0)
    assert int(rig.model.header[2]) == 32
    for call in (1, 2):
        rig.sel.parent.fill_(-1)
        rig.model.parent[:] = -1
        before = rig.snapshot()
        rig.set(score[::-1].copy(), np.full(P, 50, dtype=np.uint64))
        rig.sel.select()
        rig.check(call)
        after = rig.snapshot()
        for name in before:                                          # calls 1 and 2 write header[0], header[2] and parent only
            if name not in ("parent", "mean_return", "counts"):
                assert torch.equal(before[name], after[name]), (name, call)
        assert rig.sel.parent.cpu().tolist() == list(range(P))
        assert rig.model.header.tolist() == [call + 1, 32, 0, 65]
    rig.sel.select()
    rig.check(3)
    assert int(rig.model.header[2]) == 32 and rig.model.header.tolist()[:2] == [4, 64]


@pytest.mark.parametrize("episodes,scored", [(0, 0), (3, 65)])
def test_nobody_is_replaceable(torch, episodes, scored):
    """S = 0, and everybody scored but nobody ready: everything but header and parent keeps its bits"""
    P = 65
    rig = Rig(torch, P, fraction=0.5, ready=5, seed=4)
    rig.set(scenario(P, 5)[0], np.full(P, episodes, dtype=np.uint64))
    rig.sel.parent.fill_(-1)
    before = rig.snapshot()
    rig.sel.select()
    rig.check(episodes)
    after = rig.snapshot()
    for name in before:
        if name != "parent":
            assert torch.equal(before[name], after[name]), name
    assert rig.sel.parent.cpu().tolist() == list(range(P)) and rig.model.header.tolist() == [1, 0, 0, scored]


def test_select_captured_and_replayed_equals_the_eager_calls(torch):
    P = 65
    eager, graphed = (Rig(torch, P, fraction=0.25, ready=2, seed=6) for _ in range(2))
    graphed.sel._warm_up()                                           # both kernels have run before the capture
    graphed.set(np.zeros(P, dtype=np.float32), np.zeros(P, dtype=np.uint64))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.sel.select()
    assert graphed.sel.header.cpu().tolist() == [0, 0, 0, 0]         # captured, not run; the warm-up left no trace
    assert T.differences(graphed.sel, graphed.lb, graphed.model) == []
    for call in range(3):
        score, episodes = scenario(P, 40 + call)
        episodes = episodes + np.uint64(3 * call)
        for rig in (eager, graphed):
            rig.set(score, episodes)
        eager.sel.select()
        graph.replay()
        eager.check(("eager", call))
        graphed.check(("graph", call))
        a, b = eager.snapshot(), graphed.snapshot()
        for name in a:
            assert torch.equal(a[name], b[name]), (name, call)
    assert int(eager.model.header[1]) > 0


# ------------------------------------------------------------------------------------------------ with a real learner bank
NETS, SEG, BATCH = 4, 16, 8


def _real(torch, seed=5):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.lbank import DQNLearnerBank
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.replay import DeviceReplayRing
    from aquaticgymenv_amd.segments import SegmentTracker
    bank = QNetworkBank([L.glorot_layers(80 + p) for p in range(NETS)], SEG, DEV)
    learners = DQNLearnerBank(bank, gamma=[0.98, 0.9, 0.95, 0.97], lr=[1e-3, 3e-3, 1e-2, 2e-3], tau=[0.005, 0.05, 0.5, 0.1], seed=seed)
    env = BatchedAqua(NETS * SEG, obstacles=True, seed=29, auto_reset="next_step", normalized_obs=True, device=DEV)
    env.params.time_limit = 4
    env.reset()
    ring = DeviceReplayRing(env, 4 * NETS * SEG)
    tracker = EpisodeTracker(env)
    st = SegmentTracker(tracker, SEG, NETS, window=100, epsilon=([0.5, 0.1, 1.0, 0.3], [0.05, 0.01, 0.2, 0.1], [0.9, 0.99, 50.0, 0.95]))
    bank.epsilon = st.epsilon
    return dict(env=env, bank=bank, learners=learners, ring=ring, tracker=tracker, st=st)


def _iterate(p, n):
    env, bank, ring, tracker, learners = p["env"], p["bank"], p["ring"], p["tracker"], p["learners"]
    for _ in range(n):
        action = bank.act(env, epsilon=0.0, out=env.policy_action)
        ring.before_step(env.policy_action)
        env.step(action)
        ring.after_step()
        p["st"].after_step()
        learners.update(ring.learner_view(), BATCH, learners.draw(ring, BATCH))


def _by_hand(torch, st, score, episodes):
    st.mean_return.copy_(torch.tensor(score, dtype=torch.float32))
    st._counts[:, 0] = torch.tensor(episodes, dtype=torch.int64)


def test_the_copy_is_complete(torch):
    """network 3 takes network 0 unperturbed; trained on the same minibatch the two stay the same network"""
    from aquaticgymenv_amd.pbt import PopulationSelector
    p = _real(torch)
    lb, bank, ring = p["learners"], p["bank"], p["ring"]
    _iterate(p, 6)                                                   # Adam's moments and counters are no longer zero
    assert not torch.equal(lb.m[3], lb.m[0]) and not torch.equal(bank.tensor[3], bank.tensor[0])
    sel = PopulationSelector(lb, p["st"], fraction=0.25, ready=1, lr_factors=(1.0, 1.0), gamma_factors=(1.0, 1.0))
    _by_hand(torch, p["st"], [3.0, 2.0, 1.0, 0.0], [9, 9, 9, 9])
    seeds = lb.seed_dev.clone()
    sel.select()
    report = sel.report()
    assert report["parent"].tolist() == [0, 1, 2, 0] and report["origin"].tolist() == [0, 1, 2, 0] and report["replaced"] == 1
    assert torch.equal(lb.hyper[3], lb.hyper[0]) and lb.hyper_of(3) == lb.hyper_of(0) and lb.hyper_of(0)["gamma"] == 0.98
    assert torch.equal(lb.seed_dev, seeds) and int(lb.seed_dev[3]) != int(lb.seed_dev[0])      # the child keeps its own draws
    assert float(bank.epsilon[3]) == float(bank.epsilon[0]) and torch.equal(p["st"]._eps_state[3], p["st"]._eps_state[0])
    idx = lb.draw(ring, BATCH)
    idx[3].copy_(idx[0])
    lb.update(ring.learner_view(), BATCH, idx)
    for name in ("theta", "theta_target", "m", "v", "t", "target_tensor"):
        t = getattr(lb, name)
        assert torch.equal(t[3], t[0]), name
        assert not torch.equal(t[1], t[0]) or name == "t", name
    assert torch.equal(bank.tensor[3], bank.tensor[0]) and int(lb.t[3]) == 7
    x = ring.s[:, :64].contiguous()
    assert torch.equal(bank.view(3).q_values(x), bank.view(0).q_values(x))
    assert not torch.equal(bank.view(1).q_values(x), bank.view(0).q_values(x))


def test_state_dict_round_trip_mid_run(torch):
    from aquaticgymenv_amd.pbt import PopulationSelector
    a, b = _real(torch), _real(torch, seed=6)
    sel_a = PopulationSelector(a["learners"], a["st"], score="mean_return", fraction=0.5, ready=2, every=1, seed=77)
    sel_b = PopulationSelector(b["learners"], b["st"], score="success_rate", fraction=0.25, ready=9, every=4, seed=1,
                               lr_factors=(0.5, 2.0), gamma_bounds=(0.6, 0.9))                 # the loaded configuration must win
    scores = ([3.0, 2.0, 1.0, 0.0], [0.0, 5.0, -1.0, 2.0], [1.0, 1.0, -0.0, 0.0], [-4.0, 3.0, 2.0, 9.0])
    for call in range(2):
        _by_hand(torch, a["st"], scores[call], [4 + 3 * call] * NETS)
        sel_a.select()
    stale = a["learners"].hyper_of(3)
    state = sel_a.state_dict()                                       # (calls sync_hyper())
    table = a["learners"].hyper.cpu().numpy()
    assert int(state["header"][1]) >= 2 and a["learners"].hyper_of(3) != stale
    for p in range(NETS):
        h = a["learners"].hyper_of(p)
        assert [h[k] for k in ("gamma", "tau", "lr", "beta1", "beta2", "eps")] == table[p, :6].tolist()
    b["learners"].load_state_dict(a["learners"].state_dict())
    b["st"].load_state_dict(a["st"].state_dict())
    sel_b.load_state_dict(state)
    assert (sel_b.score, sel_b.fraction, sel_b.ready, sel_b.every, sel_b.seed) == ("mean_return", 0.5, 2, 1, 77)
    assert sel_b.lr_factors == (0.8, 1.25) and sel_b.gamma_bounds == (0.5, 0.999)
    assert torch.equal(b["learners"].hyper, a["learners"].hyper)
    for call in range(2, 4):
        for p, sel in ((a, sel_a), (b, sel_b)):
            _by_hand(torch, p["st"], scores[call], [4 + 3 * call] * NETS)
            sel.select()
        for name in ("header", "mark", "origin", "parent"):
            assert torch.equal(getattr(sel_a, name), getattr(sel_b, name)), (name, call)
        for name in ("theta", "theta_target", "m", "v", "t", "hyper", "target_tensor"):
            assert torch.equal(getattr(a["learners"], name), getattr(b["learners"], name)), (name, call)
        assert torch.equal(a["bank"].tensor, b["bank"].tensor) and torch.equal(a["st"].epsilon, b["st"].epsilon)
    assert sel_a.report()["replaced"] >= 4
    with pytest.raises(ValueError):
        sel_b.load_state_dict(dict(state, mark=state["mark"][:2]))
    with pytest.raises(ValueError):
        sel_b.load_state_dict(dict(state, config=dict(state["config"], networks=5)))


# ------------------------------------------------------------------------------------------------ the loop
def _selector_state(p, sel):
    from tests import test_segments_gpu as G
    out = dict(G._loop_state(p))
    for name in ("header", "mark", "origin", "parent"):
        out["selector." + name] = getattr(sel, name)
    out["learners.hyper"] = p["learners"].hyper
    return out


def test_population_loop_with_a_selector_eager_and_graph(torch):
    from tests import test_segments_gpu as G
    from aquaticgymenv_amd import _pbt_capi
    from aquaticgymenv_amd.pbt import PopulationSelector
    from aquaticgymenv_amd.trainer import PopulationLoop
    a, b = G._parts(torch, True), G._parts(torch, True)
    config = dict(ready=1, fraction=0.5, every=1, seed=3)
    sel_a, sel_b = (PopulationSelector(p["learners"], p["st"], **config) for p in (a, b))
    loop_a = PopulationLoop(a["env"], a["bank"], a["learners"], a["ring"], a["tracker"], G.BATCH, segments=a["st"], selector=sel_a)
    loop_b = PopulationLoop(b["env"], b["bank"], b["learners"], b["ring"], b["tracker"], G.BATCH, segments=b["st"], selector=sel_b)
    before = {k: v.clone() for k, v in _selector_state(b, sel_b).items() if k != "env.policy_action"}
    calls = []
    real = _pbt_capi.lib.aquapbt_select
    try:
        _pbt_capi.lib.aquapbt_select = lambda *args: (calls.append(1), real(*args))[1]
        graph = loop_b.capture()
        torch.cuda.synchronize()
        assert len(calls) == 2                                       # the warm-up and the capture
        for k, v in before.items():                                  # the capture and its warm-up left no trace
            assert torch.equal(_selector_state(b, sel_b)[k], v), k
        model = T.Model(3, b["learners"].blob_floats, eps=False, **config)
        model.hyper[:] = b["learners"].hyper.cpu().numpy()
        for it in range(G.ITERATIONS):
            loop_a.step()
            graph.launch()
            sa, sb = _selector_state(a, sel_a), _selector_state(b, sel_b)
            for name in sa:
                assert torch.equal(sa[name], sb[name]), ("the graph differs from step()", name, it)
            # nothing behind the selection writes what it has read: the model on the device's score and counters
            model.select(b["st"].mean_return.cpu().numpy(), b["st"]._counts.cpu().numpy().view(np.uint64))
            assert T.differences(sel_b, b["learners"], model, only=("header", "mark", "origin", "parent", "hyper")) == [], it
        assert len(calls) == 2 + G.ITERATIONS                        # eager: once per iteration; the graph calls nothing
    finally:
        _pbt_capi.lib.aquapbt_select = real
    report = sel_b.report()
    assert report["calls"] == G.ITERATIONS and report["replaced"] >= 1 and report["scored"] == 3
    assert len(set(report["origin"].tolist())) < 3
    graph.close()
    # what a selector must be to be accepted
    c = G._parts(torch, True)
    args = (c["env"], c["bank"], c["learners"], c["ring"], c["tracker"], G.BATCH)
    with pytest.raises(ValueError):
        PopulationLoop(*args, segments=c["st"], selector=object())
    with pytest.raises(ValueError):
        PopulationLoop(*args, segments=None, selector=PopulationSelector(c["learners"], c["st"]))
    with pytest.raises(ValueError):
        PopulationLoop(*args, segments=c["st"], selector=sel_a)      # another bank's, another tracker's
    other = G._parts(torch, True)
    with pytest.raises(ValueError):
        PopulationLoop(*args, segments=c["st"], selector=PopulationSelector(c["learners"], other["st"]))
    with pytest.raises(ValueError):
        PopulationSelector(other["learners"], c["st"], fraction=0.6)
    with pytest.raises(ValueError):
        PopulationSelector(other["learners"], c["st"], lr_bounds=(0.0, 0.1))
    with pytest.raises(ValueError):
        PopulationSelector(other["learners"], c["st"], gamma_bounds=(0.5, 1.5))
    with pytest.raises(ValueError):
        PopulationSelector(other["learners"], c["st"], score="loss")
    assert PopulationLoop(*args, segments=c["st"]).selector is None
