"""GPU tests of the experience ring with a device cursor (libaqua_replay.so, aquaticgymenv_amd/replay.py::DeviceReplayRing).

Everything is exact.  The reference is the numpy model of tests/_replay.py (itself checked against a per-world loop in
tests/test_replay_cpu.py) and, for the draw, tests/_learner.py::drawn: the kernels copy and draw integers, so every buffer
is compared with np.array_equal / torch.equal and there is no tolerance to state.
"""
import types

import numpy as np
import pytest

from tests import _learner as L
from tests import _replay as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAIRS = 7                     # open / close pairs per ring: it wraps at least twice
FILL = 7                      # what every ring row holds before the first write; behind `capacity` it must survive


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


@pytest.fixture(scope="module")
def xcapi(torch):
    from aquaticgymenv_amd import _replay_capi
    return _replay_capi


class Raw(object):
    """the raw C ABI on synthetic torch tensors: a device twin of R.Model with the same layout (ring_ld > capacity)"""

    def __init__(self, torch, xcapi, model):
        self.torch, self.x, self.capacity, self.ring_ld, self.continuous = torch, xcapi, model.capacity, model.ring_ld, model.continuous
        for name in R.ROWS + ("header",):
            setattr(self, name, torch.from_numpy(getattr(model, name).copy()).to(DEV))
        self.kind = xcapi.ACT_F32X2 if model.continuous else xcapi.ACT_U8

    def upload(self, batch):
        return {k: None if v is None else self.torch.from_numpy(v).to(DEV) for k, v in batch.items()}

    def open(self, b, n, src_ld):
        rc = self.x.lib.aquarpl_open(self.header.data_ptr(), self.s.data_ptr(), self.a.data_ptr(), self.ok.data_ptr(), self.ring_ld,
                                     self.capacity, b["obs"].data_ptr(), src_ld, b["action"].data_ptr(), self.kind, src_ld,
                                     None if b["time"] is None else b["time"].data_ptr(), n, None)
        self.x.check(rc, "aquarpl_open")

    def close(self, b, n, src_ld):
        rc = self.x.lib.aquarpl_close(self.header.data_ptr(), self.r.data_ptr(), self.s2.data_ptr(), self.d.data_ptr(), self.ring_ld,
                                      self.capacity, b["reward"].data_ptr(), b["obs2"].data_ptr(), src_ld, b["term"].data_ptr(), n, None)
        self.x.check(rc, "aquarpl_close")

    def differences(self, model):
        """names of the buffers that differ from the model's, the columns behind the capacity included"""
        return [name for name in R.ROWS + ("header",)
                if not np.array_equal(getattr(self, name).cpu().numpy().view(np.uint8), getattr(model, name).view(np.uint8))]


def _stub_env(torch, n, continuous=False):
    ld = (n + 63) // 64 * 64
    return types.SimpleNamespace(torch=torch, device=torch.device(DEV), num_envs=n, ld=ld, continuous=continuous, env_offset=0,
                                 obs_norm_buf=torch.zeros((5, ld), dtype=torch.float32, device=DEV),
                                 time=torch.zeros(ld, dtype=torch.int32, device=DEV),
                                 reward=torch.zeros(ld, dtype=torch.float32, device=DEV),
                                 term=torch.zeros(ld, dtype=torch.uint8, device=DEV))


def _ring_from(torch, model):
    """a DeviceReplayRing (on a stub env) holding the model's rows and header; the model must have ring_ld == capacity"""
    from aquaticgymenv_amd.replay import DeviceReplayRing
    assert model.ring_ld == model.capacity
    ring = DeviceReplayRing(_stub_env(torch, 1, model.continuous), model.capacity)
    for name in R.ROWS + ("header",):
        getattr(ring, name).copy_(torch.from_numpy(getattr(model, name)))
    return ring


def _filled_model(capacity, n, pairs, seed, continuous=False):
    rng, model = np.random.RandomState(seed), R.Model(capacity, continuous=continuous)
    for _ in range(pairs):
        b = R.make_batch(rng, n, n, continuous=continuous)
        model.open(b["obs"], b["action"], b["time"], n)
        model.close(b["reward"], b["obs2"], b["term"], n)
    return model


# ------------------------------------------------------------------------------------------------ (a) append
def _append(torch, xcapi, n, capacity, continuous, with_time, pairs, seed):
    rng = np.random.RandomState(seed)
    model = R.Model(capacity, ring_ld=capacity + 64, continuous=continuous, fill=FILL)
    dev = Raw(torch, xcapi, model)
    src_ld = n + 37                                            # poison in the padding
    for pair in range(pairs):
        b = R.make_batch(rng, n, src_ld, continuous=continuous, with_time=with_time)
        d = dev.upload(b)
        model.open(b["obs"], b["action"], b["time"], n)
        dev.open(d, n, src_ld)
        assert dev.differences(model) == [], ("open", n, capacity, pair)
        model.close(b["reward"], b["obs2"], b["term"], n)
        dev.close(d, n, src_ld)
        assert dev.differences(model) == [], ("close", n, capacity, pair)
    assert int(model.header[R.CLOSED]) == pairs and int(model.header[R.SIZE]) == min(capacity, pairs * n)
    return model, dev, d


@pytest.mark.parametrize("continuous", [False, True], ids=["discrete", "continuous"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1007])
def test_append_matches_the_model_after_every_pair(torch, xcapi, n, continuous):
    for capacity in (n, n + 1, 2 * n + 3, 3 * n):              # a batch that fills the ring, a wrap inside a wavefront, a wrap at exactly capacity
        for with_time in (True, False):
            model, dev, d = _append(torch, xcapi, n, capacity, continuous, with_time, PAIRS, seed=100 * n + capacity)
            assert PAIRS * n >= 2 * capacity or n == 1         # the ring wrapped at least twice (one world in five slots: once)
            for row in (model.s, model.ok, model.d):
                assert (row[..., capacity:] == FILL).all()     # the sentinel behind the capacity survived (in the model; the device equals it)
            if with_time and n >= 63:
                assert 0 < int(model.ok[:capacity].sum()) < capacity
    # a base outside [0, capacity): close writes nothing and leaves the header as it was
    for bad in (-1, capacity, 1 << 40):
        dev.header[R.BASE] = bad
        model.header[R.BASE] = bad
        dev.close(d, n, n + 37)
        assert dev.differences(model) == [], bad
    # ... and so does an open / close pair whose cursor is outside
    dev.header[R.CURSOR] = capacity + 5
    model.header[R.CURSOR] = capacity + 5
    dev.open(d, n, n + 37)
    model.header[R.BASE] = capacity + 5
    assert dev.differences(model) == []
    dev.close(d, n, n + 37)
    assert dev.differences(model) == []


def test_append_beyond_the_grid_cap(torch, xcapi):
    """the launch grid is capped at MAX_BLOCKS blocks: above that a thread owns several worlds"""
    n = xcapi.MAX_BLOCKS * xcapi.BLOCK + 65
    _append(torch, xcapi, n, n + 1, False, True, 3, seed=9)


# ------------------------------------------------------------------------------------------------ (b) the env's ring and its twin
def test_device_ring_equals_the_host_cursor_ring_on_a_twin(torch):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.replay import DeviceReplayRing, ReplayRing
    n, capacity, steps = 300, 700, 12
    envs = [BatchedAqua(n, obstacles=True, seed=21, auto_reset="next_step", normalized_obs=True, device=DEV) for _ in range(2)]
    for env in envs:
        env.params.time_limit = 5
        env.reset()
    dev, host = DeviceReplayRing(envs[0], capacity), ReplayRing(envs[1], capacity)
    assert dev.filled() == 0 and dev.position() == 0
    actions = torch.from_numpy(np.random.RandomState(4).randint(0, 3, (steps, n)).astype(np.uint8)).to(DEV)
    for t in range(steps):
        for env, ring in zip(envs, (dev, host)):
            ring.before_step(actions[t])
            env.step(actions[t])
            ring.after_step()
        for name in R.ROWS:
            assert torch.equal(getattr(dev, name), getattr(host, name)), (name, t)
        assert [int(v) for v in dev.header.cpu()] == [host.cursor, host.size, (host.cursor - n) % capacity, t + 1]
    assert (dev.position(), dev.filled()) == (host.cursor, host.size) == ((steps * n) % capacity, capacity)
    assert steps * n > capacity                                # the ring wrapped
    assert 0 < int((dev.ok == 0).sum()) < capacity             # some worlds were restarting: not experiences
    assert int((dev.d != 0).sum()) > 0
    with pytest.raises(RuntimeError):
        dev.after_step()


# ------------------------------------------------------------------------------------------------ (c) the draw
@pytest.mark.parametrize("batch", [1, 64, 100, 4113])
def test_draw_is_the_learners_own_draw(torch, xcapi, batch):
    capacity, seed = 1000, 0x1234567890ABCDEF
    rng = np.random.RandomState(batch)
    header = torch.zeros(4, dtype=torch.int64, device=DEV)
    t_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    idx = torch.zeros(batch + 3, dtype=torch.int32, device=DEV)
    taken = 0
    for size in (0, 1, 7, capacity):
        for bad in (0.0, 0.3, 1.0):
            ok = (rng.rand(capacity) >= bad).astype(np.uint8)
            d_ok = torch.from_numpy(ok).to(DEV)
            for t in (0, 5):
                header[R.SIZE] = size
                t_dev.fill_(t)
                idx.fill_(-77)
                xcapi.check(xcapi.lib.aquarpl_draw(header.data_ptr(), d_ok.data_ptr(), capacity, t_dev.data_ptr(), seed, idx.data_ptr(),
                                                   batch, None), "aquarpl_draw")
                want = L.drawn(seed, t + 1, batch, dict(ok=ok, size=size))
                got = idx.cpu().numpy()
                assert np.array_equal(got[:batch], want), (size, bad, t)
                assert (got[batch:] == -77).all() and int(t_dev[0]) == t          # nothing behind B, the counter is read only
                taken += int((want >= 0).sum())
                if bad == 1.0 or size == 0:
                    assert (want == -1).all()
    assert taken > 0
    # a size the header should never hold is clamped, not used as a bound of reads: capacity + 1 and -1
    ok = np.ones(capacity, dtype=np.uint8)
    d_ok = torch.from_numpy(ok).to(DEV)
    for size, clamped in ((capacity + 1, capacity), (1 << 40, capacity), (-1, 0)):
        header[R.SIZE] = size
        xcapi.check(xcapi.lib.aquarpl_draw(header.data_ptr(), d_ok.data_ptr(), capacity, t_dev.data_ptr(), seed, idx.data_ptr(), batch, None),
                    "aquarpl_draw")
        assert np.array_equal(idx.cpu().numpy()[:batch], L.drawn(seed, 6, batch, dict(ok=ok, size=clamped)))


def test_draw_then_update_equals_the_learners_own_minibatch(torch):
    from aquaticgymenv_amd.learner import DQNLearner
    from aquaticgymenv_amd.qpolicy import QNetwork
    capacity, size, batch = 900, 500, 100
    np_ring = L.float_ring(capacity, size, seed=3, bad_ok=0.2)
    np_ring["ok"][size:] = 0                                   # what a ring that was never written there holds
    model = R.Model(capacity)
    for name in R.ROWS:
        getattr(model, name)[...] = np_ring[name]
    model.header[R.SIZE] = size
    ring = _ring_from(torch, model)
    host_ring = L.DeviceRing(torch, np_ring, DEV)
    nets = [QNetwork(L.glorot_layers(5), DEV) for _ in range(2)]
    own, fed = (DQNLearner(q, seed=77) for q in nets)
    idx = torch.zeros(batch, dtype=torch.int32, device=DEV)
    view = ring.learner_view()
    assert view.size == view.capacity == capacity and view.ok is ring.ok
    for update in range(3):
        own.update(host_ring, batch)
        got = ring.draw(batch, fed, out=idx)
        assert got.data_ptr() == idx.data_ptr()
        assert np.array_equal(idx.cpu().numpy(), L.drawn(77, update + 1, batch, np_ring))
        fed.update(view, batch, idx=idx)
        for name in ("theta", "theta_target", "m", "v", "t", "loss", "grad", "target_blob"):
            assert torch.equal(getattr(own, name), getattr(fed, name)), (name, update)
        assert torch.equal(nets[0].blob, nets[1].blob), update
    assert int(fed.t[0]) == 3 and not torch.equal(fed.theta, fed.theta_target)


# ------------------------------------------------------------------------------------------------ (d) gather
@pytest.mark.parametrize("continuous", [False, True], ids=["discrete", "continuous"])
def test_gather_equals_numpy_indexing(torch, continuous):
    capacity = 333
    model = _filled_model(capacity, 100, 2, seed=6, continuous=continuous)         # 200 slots written, 133 never
    ring = _ring_from(torch, model)
    dead = np.flatnonzero(model.ok[:200] == 0)
    assert dead.size > 0 and (model.ok[200:] == 0).all()
    rng = np.random.RandomState(1)
    idx = np.concatenate([[-1, capacity, dead[0], 250, -2 ** 31, 2 ** 31 - 1, 0, 199], rng.randint(0, 200, 265)]).astype(np.int32)
    d_idx = torch.from_numpy(idx).to(DEV)
    got = [t.cpu().numpy() for t in ring.gather(d_idx)]
    want = model.gather(idx)
    for g, w, name in zip(got, want, ("s", "a", "r", "s2", "done", "valid")):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), name
    valid = want[5]
    assert list(valid[:6]) == [0] * 6 and 200 < int(valid.sum()) < idx.size
    assert not got[0][valid == 0].any() and not got[3][valid == 0].any() and not got[2][valid == 0].any()
    sel = idx[valid == 1].astype(np.int64)
    assert np.array_equal(got[0][valid == 1], model.s[:, sel].T) and np.array_equal(got[2][valid == 1], model.r[sel])
    # sample(): draw + gather, keyed by a learner or by the ring's own counter
    ring.header[R.SIZE] = 200
    model.header[R.SIZE] = 200
    learner = types.SimpleNamespace(t=torch.full((1,), 4, dtype=torch.int64, device=DEV), seed=9, device=torch.device(DEV))
    out = ring.sample(64, learner)
    want = model.gather(model.draw(9, 4, 64))
    assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(out, want)) and int(out[5].sum()) > 32
    first, second = ring.sample(64, 123), ring.sample(64, 123, out=out)
    assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(first, model.gather(model.draw(123, 0, 64))))
    assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(second, model.gather(model.draw(123, 1, 64))))
    assert second[0].data_ptr() == out[0].data_ptr()


# ------------------------------------------------------------------------------------------------ (e) graphs, resuming
def _write_sources(torch, env, action, b, n):
    env.obs_norm_buf[:, :n].copy_(b["obs"])
    env.time[:n].copy_(b["time"])
    action[:n].copy_(b["action"])


def test_captured_open_close_and_draw_replay_like_eager_calls(torch):
    from aquaticgymenv_amd.replay import DeviceReplayRing
    n, capacity, batch = 257, 600, 100
    rng = np.random.RandomState(8)
    batches = [{k: torch.from_numpy(v).to(DEV) for k, v in R.make_batch(rng, n, n).items()} for _ in range(PAIRS)]
    rings, envs, acts, idxs, learners = [], [], [], [], []
    for _ in range(2):
        env = _stub_env(torch, n)
        envs.append(env)
        rings.append(DeviceReplayRing(env, capacity))
        acts.append(torch.zeros(env.ld, dtype=torch.uint8, device=DEV))
        idxs.append(torch.full((batch,), -5, dtype=torch.int32, device=DEV))
        learners.append(types.SimpleNamespace(t=torch.zeros(1, dtype=torch.int64, device=DEV), seed=31, device=torch.device(DEV)))
    ga, eb = rings                                            # replayed from the graph / the eager twin
    # every kernel has run once before the capture (on the eager twin)
    eb.before_step(acts[1]); eb.after_step(); eb.draw(batch, learners[1], out=idxs[1])
    eb.header.zero_(); eb.ok.zero_(); idxs[1].fill_(-5)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ga.before_step(acts[0])
        ga.after_step()
        ga.draw(batch, learners[0], out=idxs[0])
    assert [int(v) for v in ga.header.cpu()] == [0, 0, 0, 0] and int((idxs[0] != -5).sum()) == 0       # captured, not run
    model = R.Model(capacity)
    for t, b in enumerate(batches):
        for env, act, learner in zip(envs, acts, learners):
            _write_sources(torch, env, act, b, n)
            env.reward[:n].copy_(b["reward"]); env.term[:n].copy_(b["term"])
            learner.t.fill_(t)
        graph.replay()
        eb.before_step(acts[1]); eb.after_step(); eb.draw(batch, learners[1], out=idxs[1])
        np_b = {k: v.cpu().numpy() for k, v in b.items()}
        model.open(np_b["obs"], np_b["action"], np_b["time"], n)
        model.close(np_b["reward"], np_b["obs"], np_b["term"], n)          # (no step in between here: s' is the same row)
        for name in R.ROWS + ("header",):
            assert torch.equal(getattr(ga, name), getattr(eb, name)), (name, t)
            assert np.array_equal(getattr(ga, name).cpu().numpy(), getattr(model, name)), (name, t)
        assert torch.equal(idxs[0], idxs[1]) and np.array_equal(idxs[0].cpu().numpy(), model.draw(31, t, batch)), t
    assert ga.filled() == capacity and int(ga.header[R.CLOSED]) == PAIRS and PAIRS * n >= 2 * capacity
    assert int((idxs[0] >= 0).sum()) > batch // 2


def test_state_dict_resumes_mid_run(torch):
    from aquaticgymenv_amd.replay import DeviceReplayRing
    n, capacity = 130, 300
    rng = np.random.RandomState(5)
    batches = [{k: torch.from_numpy(v).to(DEV) for k, v in R.make_batch(rng, n, n).items()} for _ in range(6)]
    env = _stub_env(torch, n)
    action = torch.zeros(env.ld, dtype=torch.uint8, device=DEV)

    def run(ring, lo, hi, stop_open=False):
        for t in range(lo, hi):
            b = batches[t]
            if not ring._open:
                _write_sources(torch, env, action, b, n)
                ring.before_step(action)
            if stop_open and t == hi - 1:
                return ring
            env.obs_norm_buf[:, :n].copy_(b["obs2"])
            ring.after_step(b["reward"], b["term"])
        return ring
    whole = run(DeviceReplayRing(env, capacity), 0, 6)
    first = run(DeviceReplayRing(env, capacity), 0, 4, stop_open=True)          # saved between open and close of batch 3
    state = first.state_dict()
    assert state["hyper"]["open"] and [int(v) for v in state["header"]] == [90, 300, 90, 3]
    run(first, 3, 5)                                                            # the saved state is a copy
    resumed = run(DeviceReplayRing(env, capacity).load_state_dict(state), 3, 6)
    for name in R.ROWS + ("header",):
        assert torch.equal(getattr(whole, name), getattr(resumed, name)), name
    assert not torch.equal(whole.header, first.header)
    assert [int(v) for v in whole.header.cpu()] == [(6 * n) % capacity, capacity, (5 * n) % capacity, 6]
    with pytest.raises(ValueError):
        DeviceReplayRing(env, capacity + 1).load_state_dict(state)
    bad = dict(state, header=state["header"][:3])
    with pytest.raises(ValueError):
        DeviceReplayRing(env, capacity).load_state_dict(bad)


def test_python_layer_rejections(torch):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.replay import DeviceReplayRing
    plain = BatchedAqua(256, seed=1, device=DEV)
    with pytest.raises(RuntimeError):
        DeviceReplayRing(plain, 1024)                                           # no normalised observation to store
    env = BatchedAqua(256, seed=1, normalized_obs=True, device=DEV)
    env.reset()
    with pytest.raises(ValueError):
        DeviceReplayRing(env, 255)
    with pytest.raises(ValueError):
        DeviceReplayRing(env, 1 << 31)
    ring = DeviceReplayRing(env, 1024)
    for bad in (torch.zeros(256, dtype=torch.int64, device=DEV), torch.zeros(256, dtype=torch.uint8), torch.zeros(255, dtype=torch.uint8, device=DEV),
                torch.zeros((2, 256), dtype=torch.float32, device=DEV), [0] * 256):
        with pytest.raises(ValueError):
            ring.before_step(bad)
    with pytest.raises(RuntimeError):
        ring.after_step()
    ring.before_step(torch.zeros(256, dtype=torch.uint8, device=DEV))
    for kw in (dict(reward=torch.zeros(256, dtype=torch.float64, device=DEV)), dict(term=torch.zeros(256, dtype=torch.uint8)),
               dict(reward=torch.zeros(100, dtype=torch.float32, device=DEV))):
        with pytest.raises(ValueError):
            ring.after_step(**kw)
    learner = types.SimpleNamespace(t=torch.zeros(1, dtype=torch.int64, device=DEV), seed=1, device=torch.device(DEV))
    with pytest.raises(ValueError):
        ring.draw(64, learner, out=torch.zeros(63, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ring.draw(64, learner, out=torch.zeros(64, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        ring.draw((1 << 20) + 1, learner)
    with pytest.raises(ValueError):
        ring.draw(64, types.SimpleNamespace(t=learner.t, seed=1, device=torch.device("cpu")))
    with pytest.raises(ValueError):
        ring.gather(torch.zeros(8, dtype=torch.int32, device=DEV), out=(torch.zeros(8, device=DEV),) * 6)
    assert ring.filled() == 0 and int(ring.header[R.CLOSED]) == 0
    cont = BatchedAqua(64, seed=1, continuous=True, normalized_obs=True, device=DEV)
    cont.reset()
    cring = DeviceReplayRing(cont, 64)
    with pytest.raises(ValueError):
        cring.before_step(torch.zeros(64, dtype=torch.uint8, device=DEV))
    cring.before_step(torch.full((2, 64), 0.3, dtype=torch.float32, device=DEV))
    cont.step(torch.full((2, 64), 0.3, dtype=torch.float32, device=DEV), soa=True)
    cring.after_step()
    assert cring.filled() == 64 and cring.position() == 0 and torch.equal(cring.a, torch.full((2, 64), 0.3, dtype=torch.float32, device=DEV))
    assert torch.equal(cring.s2, cont.obs_norm_buf[:, :64])
