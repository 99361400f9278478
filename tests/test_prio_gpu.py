"""GPU tests of libaqua_prio.so (aquaticgymenv_amd/csrc/aqua_prio.h), PrioritizedReplay (aquaticgymenv_amd/priority.py)
and PopulationLoop(priorities=) (aquaticgymenv_amd/trainer.py).  The trees, pmax and the drawn slots are compared bit for bit
with the integer model tests/_prio_model.py; the weights with the library's own host entries (which tests/test_prio_cpu.py
holds to the float64 formulas); the weighted update with the learner bank (weight == 1), with the exact integer model
(dyadic weights) and, on float networks, with the float64 model inside the float32 model's own error.
"""
import ctypes

import numpy as np
import pytest

from tests import _lbank as K
from tests import _learner as L
from tests import _prio_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BIG = (72 * 160, 160, 64, 3)          # 4 608 leaves, levels 4 608 -> 72 -> 2 -> 1; the last network has 32 worlds
SMALL = (6 * 10, 10, 4, 4)            # 24 leaves: one node; network 2 has 2 worlds, network 3 none
ONE_NODE = (8 * 8, 8, 8, 1)           # 64 leaves, one network
ALPHA, EPS = 0.6, 1e-3


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


@pytest.fixture(scope="module")
def capi():
    from aquaticgymenv_amd import _prio_capi
    return _prio_capi


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


class Trees(object):
    """the device side of direct calls: the tree buffer, pmax, the ring's header and ok row"""

    def __init__(self, torch, capi, shape, seed=0):
        self.torch, self.capi, self.shape = torch, capi, shape
        capacity, N, seg, P = shape
        self.lay = capi.layout(*shape)
        assert self.lay == M.layout(*shape)
        self.tree = torch.zeros(self.lay["bytes"], dtype=torch.uint8, device=DEV)
        assert self.tree.data_ptr() % 512 == 0
        self.pmax = torch.full((P,), M.ONE, dtype=torch.int32, device=DEV)
        self.header = torch.zeros(4, dtype=torch.int64, device=DEV)
        self.ok_np = (np.random.RandomState(seed).rand(capacity) < 0.8).astype(np.uint8)
        self.ok = torch.as_tensor(self.ok_np).to(DEV)
        self.model = M.Trees(*shape)

    def levels(self):
        self.torch.cuda.synchronize()
        raw, P, out = self.tree.cpu().numpy(), self.shape[3], []
        for k in range(self.lay["levels"]):
            n, stride, off = self.lay["n"][k], self.lay["stride"][k], self.lay["offset"][k]
            dtype = np.uint32 if k == 0 else np.uint64
            rows = raw[off:off + P * stride * np.dtype(dtype).itemsize].view(dtype).reshape(P, stride)
            assert not rows[:, n:].any()                               # the padding of a level stays zero
            out.append(rows[:, :n].copy())
        return out

    def load(self, leaves):
        """a crafted tree: leaves uint32 [P][L0] and the exact sums above them, uploaded"""
        raw, P = np.zeros(self.lay["bytes"], dtype=np.uint8), self.shape[3]
        self.model.leaves[:] = leaves
        for k, level in enumerate(self.model.levels()):
            stride, off = self.lay["stride"][k], self.lay["offset"][k]
            rows = np.zeros((P, stride), dtype=np.uint32 if k == 0 else np.uint64)
            rows[:, :level.shape[1]] = level
            raw[off:off + rows.nbytes] = rows.view(np.uint8).reshape(-1)
        self.tree.copy_(self.torch.as_tensor(raw).to(DEV))

    def insert(self, base):
        self.header[2] = base
        rc = self.capi.lib.aquaprio_insert(self.tree.data_ptr(), self.tree.numel(), self.pmax.data_ptr(), *self.shape, self.header.data_ptr(),
                                           self.ok.data_ptr(), _stream(self.torch))
        self.capi.check(rc, "aquaprio_insert")
        self.model.insert(base, self.ok_np)

    def set(self, idx, td):
        torch = self.torch
        i, t = torch.as_tensor(np.ascontiguousarray(idx, dtype=np.int32)).to(DEV), torch.as_tensor(np.ascontiguousarray(td, dtype=np.float32)).to(DEV)
        rc = self.capi.lib.aquaprio_set(self.tree.data_ptr(), self.tree.numel(), self.pmax.data_ptr(), *self.shape, i.data_ptr(), t.data_ptr(),
                                        idx.shape[1], ALPHA, EPS, _stream(torch))
        self.capi.check(rc, "aquaprio_set")
        torch.cuda.synchronize()
        self.model.set(np.asarray(idx), np.asarray(td, dtype=np.float32), lambda x: self.capi.quantise(abs(x), ALPHA, EPS))

    def draw(self, B, t, seeds, size, beta0=0.4, anneal=20):
        torch, P = self.torch, self.shape[3]
        self.header[1] = size
        t_dev = torch.as_tensor(np.array(t, dtype=np.int64)).to(DEV)
        seed_dev = torch.as_tensor(np.array(seeds, dtype=np.uint64).view(np.int64)).to(DEV)
        idx = torch.full((P, B), -7, dtype=torch.int32, device=DEV)
        weight = torch.full((P, B), 7.0, dtype=torch.float32, device=DEV)
        q = torch.full((P, B), 7, dtype=torch.int32, device=DEV)
        rc = self.capi.lib.aquaprio_draw(self.tree.data_ptr(), self.tree.numel(), *self.shape, self.header.data_ptr(), t_dev.data_ptr(),
                                         seed_dev.data_ptr(), idx.data_ptr(), weight.data_ptr(), q.data_ptr(), B, beta0, anneal, _stream(torch))
        self.capi.check(rc, "aquaprio_draw")
        torch.cuda.synchronize()
        return idx.cpu().numpy(), weight.cpu().numpy(), q.cpu().numpy().view(np.uint32)

    def check(self, what):
        """the device's trees are the model's bit for bit, and every node is the exact sum of its children, from the device's
        own leaves"""
        got, want = self.levels(), self.model.levels()
        for k, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (what, "level", k)
        for p in range(self.shape[3]):
            for k, level in enumerate(M.sums_above(got[0][p], self.lay["n"])):
                assert np.array_equal(got[k + 1][p], level), (what, "sum", p, k + 1)
        assert np.array_equal(self.pmax.cpu().numpy().view(np.uint32), self.model.pmax), what
        return got


def _own_slots(shape, p, filled_rounds):
    capacity, N, seg, P = shape
    return [r * N + p * seg + i for r in range(filled_rounds) for i in range(M.worlds(N, seg, p))]


def _set_batch(rng, shape, B, rounds):
    """idx [P][B], td [P][B]: own slots with -1 entries, td == -1 entries, repeated slots with the same td, another network's
    slot and a slot beyond the ring (both untouched)"""
    capacity, N, seg, P = shape
    idx, td = np.full((P, B), -1, dtype=np.int64), rng.exponential(1.0, (P, B)).astype(np.float32)
    for p in range(P):
        own = _own_slots(shape, p, rounds)
        if not own:
            idx[p] = rng.randint(0, capacity, B)                        # none of them is this network's
            continue
        pick = rng.choice(own, size=max(1, min(B - B // 8, len(own))), replace=False)     # an eighth of the row repeats a slot
        idx[p, :len(pick)] = pick
        for j in range(len(pick), B):                                   # repeats, with the td of the first
            src = int(rng.randint(0, len(pick)))
            idx[p, j], td[p, j] = idx[p, src], td[p, src]
        order = rng.permutation(B)
        idx[p], td[p] = idx[p, order], td[p, order]
        hole = rng.rand(B)
        keep_td = td[p].copy()
        for j in np.nonzero(hole < 0.1)[0]:                             # no slot: every copy of that slot goes
            same = idx[p] == idx[p, j]
            idx[p, same] = -1
        for j in np.nonzero((hole >= 0.1) & (hole < 0.2))[0]:           # no TD error: every copy of that slot
            same = (idx[p] == idx[p, j]) & (idx[p] >= 0)
            keep_td[same] = -1.0
        td[p] = keep_td
        other = (p + 1) % max(1, -(-N // seg))
        if other != p and B > 4:
            idx[p, 0], td[p, 0] = _own_slots(shape, other, 1)[0], 5.0
            idx[p, 1], td[p, 1] = capacity, 5.0
            idx[p, 2], td[p, 2] = 2 ** 31 - 1, 5.0
    return idx.astype(np.int32), td


# ------------------------------------------------------------------------------------------------ insert and set
@pytest.mark.parametrize("shape", [BIG, SMALL, ONE_NODE], ids=["4608-leaves", "24-leaves-idle-network", "64-leaves"])
def test_insert_keeps_the_tree_through_the_wrap(torch, capi, shape):
    """77 rounds on the ring of 72 (five past the wrap; the small rings wrap many times), random ok, a set() now and then so
    that pmax moves and old leaves differ from what overwrites them: after every round the leaves, every sum and pmax"""
    capacity, N, seg, P = shape
    trees = Trees(torch, capi, shape, seed=1)
    rng = np.random.RandomState(7)
    rounds = capacity // N
    for it in range(77):
        trees.ok_np[:] = rng.rand(capacity) < 0.8
        trees.ok.copy_(torch.as_tensor(trees.ok_np))
        trees.insert((it % rounds) * N)
        got = trees.check(("insert", it))
        if it % 9 == 4:
            idx, td = _set_batch(rng, shape, 16, min(it + 1, rounds))
            trees.set(idx, td * 3.0)
            trees.check(("set", it))
    assert int(got[-1].sum()) > 0 and bool((trees.model.pmax[:max(1, -(-N // seg))] > M.ONE).any())
    for p in range(-(-N // seg), P):                                    # a network without a world: an empty tree
        assert not got[0][p].any() and int(got[-1][p, 0]) == 0 and int(trees.model.pmax[p]) == M.ONE
    # a header the ring cannot have written: nothing happens
    before = trees.tree.clone()
    for bad in (-N, capacity, N // 2 if N > 1 else capacity + 1):
        trees.insert(bad)
        torch.cuda.synchronize()
        assert torch.equal(trees.tree, before), bad


@pytest.mark.parametrize("shape", [BIG, SMALL], ids=["4608-leaves", "24-leaves-idle-network"])
def test_set_is_the_model_bit_for_bit(torch, capi, shape):
    capacity, N, seg, P = shape
    trees = Trees(torch, capi, shape, seed=2)
    rounds = capacity // N
    for r in range(rounds):
        trees.insert(r * N)
    rng = np.random.RandomState(11)
    for B in (1, 70, 300):
        idx, td = _set_batch(rng, shape, B, rounds)
        before = trees.check(("before", B))[0].copy()
        trees.set(idx, td)
        after = trees.check(("set", B))[0]
        for p in range(P):
            for slot, x in zip(idx[p].tolist(), td[p].tolist()):
                if 0 <= slot < capacity and x >= 0 and M.leaf_of_slot(slot, N, seg)[0] == p:
                    assert after[p, M.leaf_of_slot(slot, N, seg)[1]] == capi.quantise(x, ALPHA, EPS)
        touched = before != after
        assert B == 1 or touched.any()
        # only leaves that were named with a TD error changed
        named = np.zeros_like(touched)
        for p in range(P):
            for slot, x in zip(idx[p].tolist(), td[p].tolist()):
                if 0 <= slot < capacity and x >= 0 and M.leaf_of_slot(slot, N, seg)[0] == p:
                    named[p, M.leaf_of_slot(slot, N, seg)[1]] = True
        assert not (touched & ~named).any()
    # TD errors that are not numbers, or not finite, leave everything as it was
    before = trees.tree.clone()
    own = _own_slots(shape, 0, 1)[:3]
    trees.set(np.array([own] + [[-1] * len(own)] * (P - 1)), np.array([[np.nan, np.inf, -np.inf][:len(own)]] * P, dtype=np.float32))
    assert torch.equal(trees.tree, before)


# ------------------------------------------------------------------------------------------------ the draw
def _check_draw(capi, trees, B, t, seeds, size, beta0=0.4, anneal=20):
    capacity, N, seg, P = trees.shape
    idx, weight, q = trees.draw(B, t, seeds, size, beta0, anneal)
    levels = trees.levels()
    for p in range(P):
        leaves = levels[0][p]
        want_idx, want_q = M.draw(leaves, trees.lay["n"], seeds[p], t[p], B, p, N, seg, capacity)
        assert np.array_equal(idx[p], want_idx), ("idx", p)
        assert np.array_equal(q[p], want_q), ("q", p)
        T = int(levels[-1][p, 0])
        size_p = max(1, min(max(size, 0), capacity) // N * M.worlds(N, seg, p))
        want_w = M.weights(want_q, T, size_p, capi.beta(t[p], beta0, anneal), capi.weight)
        assert np.array_equal(weight[p].view(np.uint32), want_w.view(np.uint32)), ("weight", p)
        live = idx[p] >= 0
        if live.any():
            owner, c = zip(*[M.leaf_of_slot(int(s), N, seg) for s in idx[p][live]])
            assert set(owner) == {p} and bool((leaves[list(c)] != 0).all())         # a leaf of 0 is never drawn
            assert float(weight[p].max()) == 1.0 and bool((weight[p][live] > 0).all())
        assert bool((weight[p][~live] == 0).all())
    return idx, weight, q


@pytest.mark.parametrize("shape", [BIG, SMALL], ids=["4608-leaves", "24-leaves-idle-network"])
def test_draw_is_the_models_descent_and_the_host_weights(torch, capi, shape):
    capacity, N, seg, P = shape
    trees = Trees(torch, capi, shape, seed=3)
    rounds = capacity // N
    filled = rounds - 2
    for r in range(filled):
        trees.insert(r * N)
    rng = np.random.RandomState(13)
    for _ in range(3):
        idx, td = _set_batch(rng, shape, 200, filled)
        trees.set(idx, td)
    trees.check("prepared")
    seeds = [5 + 1000 * p for p in range(P)]
    # update counters before, inside and beyond the annealing: beta0, in between, 1
    for t in ([0] * P, [3 + 4 * p for p in range(P)], [20 + p for p in range(P)], [2 ** 33 + p for p in range(P)]):
        idx, weight, q = _check_draw(capi, trees, 70, t, seeds, filled * N)
        assert all((idx[p] >= 0).all() for p in range(min(P, -(-N // seg)))) and all((idx[p] == -1).all() for p in range(-(-N // seg), P))
    assert shape != BIG or len(set(weight[0].tolist())) >= 3                       # priorities differ, so do the weights
    # another draw for another update, the same draw for the same one
    a = trees.draw(70, [1] * P, seeds, filled * N)[0]
    b = trees.draw(70, [2] * P, seeds, filled * N)[0]
    c = trees.draw(70, [1] * P, seeds, filled * N)[0]
    assert np.array_equal(a, c) and not np.array_equal(a[0], b[0])


def test_draw_corner_cases(torch, capi):
    trees = Trees(torch, capi, BIG, seed=4)
    capacity, N, seg, P = BIG
    L0 = trees.lay["leaves"]
    seeds, t = [9, 10, 11], [4, 5, 6]
    # an all-zero tree
    idx, weight, q = _check_draw(capi, trees, 70, t, seeds, capacity)
    assert bool((idx == -1).all()) and bool((weight == 0).all()) and bool((q == 0).all())
    # all leaves equal: every weight is 1; the last network's leaves end where its worlds end
    leaves = np.zeros((P, L0), dtype=np.uint32)
    for p in range(P):
        leaves[p, :72 * M.worlds(N, seg, p)] = 12345
    trees.load(leaves)
    idx, weight, q = _check_draw(capi, trees, 70, t, seeds, capacity)
    assert bool((weight == 1.0).all()) and bool((idx >= 0).all()) and len(set(idx[2].tolist())) > 50
    # one leaf holds almost all of the mass
    leaves[:] = 0
    for p in range(P):
        leaves[p, :72 * M.worlds(N, seg, p)] = 1
        leaves[p, 1000 + p] = M.QMAX
    trees.load(leaves)
    idx, weight, q = _check_draw(capi, trees, 70, t, seeds, capacity)
    for p in range(P):
        heavy = M.slot_of_leaf(p, 1000 + p, N, seg)
        assert int((idx[p] == heavy).sum()) >= 68
    # the largest sums a tree can hold: every leaf at its maximum
    leaves[:] = 0
    leaves[0, :] = M.QMAX
    trees.load(leaves)
    _check_draw(capi, trees, 70, t, seeds, capacity)
    assert int(trees.levels()[-1][0, 0]) == L0 * M.QMAX


def test_draw_past_the_block_cap(torch, capi):
    """P = 1 on the 64-leaf tree, B a little above the 4 x 2 048 samples one pass of a full grid takes"""
    B = capi.WAVES * capi.MAX_BLOCKS + 5
    trees = Trees(torch, capi, ONE_NODE, seed=5)
    rng = np.random.RandomState(17)
    leaves = (rng.randint(2 ** 18, 2 ** 20, (1, 64)) * (rng.rand(1, 64) < 0.8)).astype(np.uint32)     # every leaf is drawn, 32 times at least on average
    trees.load(leaves)
    idx, weight, q = _check_draw(capi, trees, B, [2], [77], 64)
    assert bool((idx[0, -5:] >= 0).all()) and len(set(idx[0].tolist())) == int((leaves != 0).sum())


# ------------------------------------------------------------------------------------------------ the weighted update
LOSS_REFERENCE = 16
STRATEGIES = [(0, "double_ref"), (1, "double"), (2, "fixed"), (3, "standard")]


def _prio_update(torch, capi, run, d, ring, idx, B, strategy, hyper_dev, weight, td):
    P = d["theta"].shape[0]
    need = int(run.bank.lib.aqualbank_workspace_bytes(P, B))
    ws = run.workspace(need)
    rc = capi.lib.aquaprio_update_f32(
        d["theta"].data_ptr(), d["theta_target"].data_ptr(), d["m"].data_ptr(), d["v"].data_ptr(), d["t"].data_ptr(), P,
        ring.s.data_ptr(), ring.a.data_ptr(), ring.r.data_ptr(), ring.s2.data_ptr(), ring.d.data_ptr(), ring.ok.data_ptr(),
        ring.capacity, ring.size, idx.data_ptr(), B, strategy, hyper_dev.data_ptr(),
        d["blob"].data_ptr(), d["blob_target"].data_ptr(), run.perm.data_ptr(), K.BLOB_FLOATS, ws.data_ptr(), need,
        d["idx_out"].data_ptr(), d["grad"].data_ptr(), d["loss"].data_ptr(), weight.data_ptr(), td.data_ptr(), _stream(torch))
    capi.check(rc, "aquaprio_update_f32")


@pytest.fixture(scope="module")
def run(torch):
    return K.Runner(torch, DEV)


@pytest.fixture(scope="module")
def int_case():
    """P = 3 integer networks on an integer ring, B = 70 with every invalid kind of index, gamma = 1"""
    P, B, cap, size = 3, 70, 300, 257
    ring = L.int_ring(cap, size, 7, bad_ok=0.1)
    st = K.make_state(P, 1, [L.int_layers(salt=p) for p in range(P)], [L.int_layers(salt=p + 1) for p in range(P)], fresh=True)
    idx = K.mixed_idx(np.random.RandomState(5), P, B, ring, cap)
    hyper = K.hypers(P)
    hyper[:, 0] = 1.0
    return dict(P=P, B=B, cap=cap, ring=ring, st=st, idx=idx, hyper=hyper)


@pytest.mark.parametrize("form", [0, LOSS_REFERENCE], ids=["mse", "reference"])
@pytest.mark.parametrize("strategy,name", STRATEGIES)
def test_unit_weights_are_the_bank_update_bit_for_bit(torch, capi, run, int_case, strategy, name, form):
    c = int_case
    P, B = c["P"], c["B"]
    ring = L.DeviceRing(torch, c["ring"], DEV)
    a, b = K.to_device(torch, c["st"], B, DEV), K.to_device(torch, c["st"], B, DEV)
    hd = run.hyper_dev(c["hyper"])
    idx = torch.as_tensor(c["idx"]).to(DEV)
    weight = torch.ones((P, B), dtype=torch.float32, device=DEV)
    td = torch.full((P, B), 7.0, dtype=torch.float32, device=DEV)
    for _ in range(2):
        run.bank_update(a, ring, idx, B, strategy | form, hd)
        _prio_update(torch, capi, run, b, ring, idx, B, strategy | form, hd, weight, td)
        bank, prio = K.read(torch, a), K.read(torch, b)
        assert K.differing(bank, prio) == []
    assert bool((prio["t"] == 2).all()) and bool((prio["loss"] > 0).all())
    # td_out: |Q_a - y| of the integer model exactly (after the first update the networks are no integers any more: a fresh run)
    b = K.to_device(torch, c["st"], B, DEV)
    _prio_update(torch, capi, run, b, ring, idx, B, strategy | form, hd, weight, td)
    got = td.cpu().numpy()
    for p in range(P):
        eff = L.effective(c["idx"][p], c["ring"])
        ref = M.weighted_gradient(c["st"]["theta"][p], c["st"]["theta_target"][p], c["ring"], eff, np.ones(B), 1.0, name, np.float64,
                                  "reference" if form else "mse")
        assert np.array_equal(got[p].astype(np.float64), ref["td"]), p
        assert bool((got[p][eff < 0] == -1.0).all()) and int((eff < 0).sum()) >= 4 and bool((got[p][eff >= 0] >= 0).all())


@pytest.mark.parametrize("form", ["mse", "reference"])
def test_dyadic_weights_on_integer_networks_are_exact(torch, capi, run, int_case, form):
    c = int_case
    P, B = c["P"], c["B"]
    ring = L.DeviceRing(torch, c["ring"], DEV)
    rng = np.random.RandomState(23)
    w = rng.choice([0.25, 0.5, 1.0, 2.0], size=(P, B)).astype(np.float32)
    d = K.to_device(torch, c["st"], B, DEV)
    td = torch.full((P, B), 7.0, dtype=torch.float32, device=DEV)
    _prio_update(torch, capi, run, d, ring, torch.as_tensor(c["idx"]).to(DEV), B, LOSS_REFERENCE if form == "reference" else 0,
                 run.hyper_dev(c["hyper"]), torch.as_tensor(w).to(DEV), td)
    out = K.read(torch, d)
    for p in range(P):
        eff = L.effective(c["idx"][p], c["ring"])
        worst, _, _ = L.abs_sums(c["st"]["theta"][p], c["st"]["theta_target"][p], c["ring"], eff, "double_ref", form=form)
        assert worst * 8 < 2 ** 24                 # weights <= 2 and quarters: every partial sum is exact in float32
        ref = M.weighted_gradient(c["st"]["theta"][p], c["st"]["theta_target"][p], c["ring"], eff, w[p], 1.0, "double_ref", np.float64, form)
        squares = ref["n"] * (3 if form == "reference" else 1)
        want = ref["S"].astype(np.float32) * np.float32(2.0 / squares)
        assert np.array_equal(ref["S"] * 4, np.rint(ref["S"] * 4)) and np.array_equal(ref["S"].astype(np.float32).astype(np.float64), ref["S"])
        assert np.array_equal(out["grad"][p].view(np.uint32), want.view(np.uint32)), p
        sq_sum = float(ref["loss"]) * squares
        assert out["loss"][p] == np.float32(np.rint(sq_sum * 16) / 16 / squares), p
        plain = M.weighted_gradient(c["st"]["theta"][p], c["st"]["theta_target"][p], c["ring"], eff, np.ones(B), 1.0, "double_ref", np.float64, form)
        assert not np.array_equal(plain["S"], ref["S"]) and np.array_equal(td.cpu().numpy()[p].astype(np.float64), plain["td"])


@pytest.mark.parametrize("form", ["mse", "reference"])
def test_weighted_update_on_float_networks_against_float64(torch, capi, run, form):
    """Glorot networks, a float ring, weights in (0, 1] as the draw makes them: the gradient and the loss against the float64
    model.  The bar is the one of tests/test_learner_forms_gpu.py: 4 E, with E the error of the SAME model run in float32
    (here with the weights multiplied in) -- the kernel keeps delta in double and sums in float32 as that model does."""
    P, B, cap = 3, 70, 480
    ring_np = L.float_ring(cap, cap, 11, bad_ok=0.05)
    st = K.make_state(P, 3)
    rng = np.random.RandomState(29)
    idx = K.mixed_idx(rng, P, B, ring_np, cap)
    w = rng.uniform(0.05, 1.0, (P, B)).astype(np.float32)
    w[:, 7] = 1.0
    hyper = K.hypers(P)
    d = K.to_device(torch, st, B, DEV)
    td = torch.full((P, B), 7.0, dtype=torch.float32, device=DEV)
    _prio_update(torch, capi, run, d, L.DeviceRing(torch, ring_np, DEV), torch.as_tensor(idx).to(DEV), B,
                 LOSS_REFERENCE if form == "reference" else 0, run.hyper_dev(hyper), torch.as_tensor(w).to(DEV), td)
    out = K.read(torch, d)
    got_td = td.cpu().numpy()
    for p in range(P):
        eff = L.effective(idx[p], ring_np)
        gamma = float(np.float32(hyper[p, 0]))
        r64 = M.weighted_gradient(st["theta"][p], st["theta_target"][p], ring_np, eff, w[p], gamma, "double_ref", np.float64, form)
        r32 = M.weighted_gradient(st["theta"][p], st["theta_target"][p], ring_np, eff, w[p], gamma, "double_ref", np.float32, form)
        E_g = float(np.max(np.abs(r32["g"].astype(np.float64) - r64["g"])))
        E_l = abs(float(r32["loss"]) - float(r64["loss"]))
        err = float(np.max(np.abs(out["grad"][p].astype(np.float64) - r64["g"])))
        err_l = abs(float(out["loss"][p]) - float(r64["loss"]))
        print("network %d %s: max |grad - g64| %.3e = %.2f E_g; |loss - l64| %.3e = %.2f E_l" % (p, form, err, err / E_g, err_l, err_l / E_l if E_l else np.inf))
        assert err <= 4 * E_g and err_l <= 4 * max(E_l, float(np.spacing(np.float32(r64["loss"])))), (p, err, E_g, err_l, E_l)
        live = eff >= 0
        assert bool((got_td[p][~live] == -1.0).all())
        assert np.allclose(got_td[p][live], r64["td"][live], rtol=0, atol=float(np.max(np.abs(r32["td"][live] - r64["td"][live])) * 4 + 1e-7))


# ------------------------------------------------------------------------------------------------ the loop
P_NETS, SEG = 4, 16


def _parts(torch, selector=True):
    from aquaticgymenv_amd.batched import BatchedAqua
    from aquaticgymenv_amd.episodes import EpisodeTracker
    from aquaticgymenv_amd.lbank import DQNLearnerBank
    from aquaticgymenv_amd.pbt import PopulationSelector
    from aquaticgymenv_amd.priority import PrioritizedReplay
    from aquaticgymenv_amd.qbank import QNetworkBank
    from aquaticgymenv_amd.replay import DeviceReplayRing
    from aquaticgymenv_amd.segments import SegmentTracker
    bank = QNetworkBank([L.glorot_layers(60 + p) for p in range(P_NETS)], SEG, DEV)
    learners = DQNLearnerBank(bank, gamma=[0.98, 0.9, 0.95, 0.97], lr=[1e-3, 3e-3, 1e-2, 1e-3], tau=[0.005, 0.05, 0.5, 0.01], seed=5)
    env = BatchedAqua(P_NETS * SEG, obstacles=True, seed=23, auto_reset="next_step", normalized_obs=True, device=DEV)
    env.params.time_limit = 4
    env.reset()
    ring = DeviceReplayRing(env, 4 * P_NETS * SEG)                     # four rounds: six iterations wrap it
    tracker = EpisodeTracker(env)
    st = sel = None
    if selector:
        st = SegmentTracker(tracker, SEG, P_NETS, window=100, epsilon=([0.5, 0.1, 1.0, 0.3], [0.05, 0.01, 0.2, 0.05], [0.9, 0.99, 50.0, 0.9]))
        bank.epsilon = st.epsilon
        sel = PopulationSelector(learners, st, ready=1, fraction=0.5, every=1, seed=3)
    else:
        bank.epsilon = torch.tensor([0.5, 0.1, 1.0, 0.3], dtype=torch.float32, device=DEV)
    per = PrioritizedReplay(ring, learners, alpha=0.6, beta0=0.4, anneal=4, eps=1e-3)
    return dict(env=env, bank=bank, learners=learners, ring=ring, tracker=tracker, st=st, sel=sel, per=per)


def _loop(p, priorities=True, **kw):
    from aquaticgymenv_amd.trainer import PopulationLoop
    return PopulationLoop(p["env"], p["bank"], p["learners"], p["ring"], p["tracker"], 8, segments=p["st"], selector=p["sel"],
                          priorities=p["per"] if priorities else None, **kw)


def _state(p, loop):
    env, ring, lb, per = p["env"], p["ring"], p["learners"], p["per"]
    out = {"env.state": env.state, "env.time": env.time, "bank.tensor": p["bank"].tensor, "bank.epsilon": p["bank"].epsilon, "ring.header": ring.header}
    for name in ("s", "a", "r", "s2", "d", "ok"):
        out["ring." + name] = getattr(ring, name)
    for name in ("theta", "theta_target", "m", "v", "t", "target_tensor", "hyper", "loss", "grad"):
        out["learners." + name] = getattr(lb, name)
    for name in ("tree", "pmax", "idx", "weight", "td"):
        out["per." + name] = getattr(per, name)
    if loop.nstep is not None:
        for name in ("s", "a", "r", "s2", "d", "ok", "length", "hyper"):
            out["nstep." + name] = getattr(loop.nstep, name)
    return out


def _tree_holds(per):
    """the invariant on the object's own trees, from the device's own leaves"""
    levels = per.levels()
    for p in range(per.networks):
        for k, level in enumerate(M.sums_above(levels[0][p], per.layout["n"])):
            assert np.array_equal(levels[k + 1][p], level), (p, k + 1)
    return levels


@pytest.mark.parametrize("n_step,selector", [(1, False), (3, False), (1, True), (3, True)],
                         ids=["one-step", "three-steps", "one-step-selector", "three-steps-selector"])
def test_population_loop_eager_and_graph_agree(torch, n_step, selector):
    a, b = _parts(torch, selector), _parts(torch, selector)
    loop_a, loop_b = _loop(a, n_step=n_step), _loop(b, n_step=n_step)
    before = {k: v.clone() for k, v in _state(b, loop_b).items()}
    graph = loop_b.capture()
    torch.cuda.synchronize()
    for k, v in before.items():                                      # the capture and its warm-up left no trace: every byte of the tree
        assert torch.equal(_state(b, loop_b)[k], v), k
    for it in range(6):
        loop_a.step()
        graph.launch()
        torch.cuda.synchronize()
        sa, sb = _state(a, loop_a), _state(b, loop_b)
        for name in sa:
            assert torch.equal(sa[name], sb[name]), ("the graph differs from step()", name, it)
        levels = _tree_holds(b["per"])
        # the leaves follow the ring: an experience has a priority, anything else none
        ok, N = b["ring"].ok.cpu().numpy(), P_NETS * SEG
        for slot in range(b["ring"].capacity):
            p, c = M.leaf_of_slot(slot, N, SEG)
            assert (levels[0][p, c] != 0) == (ok[slot] != 0), (it, slot)
    per = b["per"]
    td, idx = per.td.cpu().numpy(), per.idx.cpu().numpy()
    assert bool((idx >= 0).all()) and bool((per.pmax.cpu().numpy() > M.ONE).any() or (td < 1.0).all())
    if n_step == 3:
        dropped = loop_b.nstep.ok.cpu().numpy().reshape(idx.shape) == 0
        assert dropped.any() and bool((td[dropped] == -1.0).all()) and bool((td[~dropped] >= 0).all())
    else:
        assert bool((td >= 0).all())
    w = per.weight.cpu().numpy()
    assert bool((w > 0).all()) and bool((w.max(axis=1) == 1.0).all())
    graph.close()


def _node_count(torch, loop):
    """the nodes of the graph loop.capture() captures: the same warm-up, the same queue, captured here and counted"""
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


def test_node_counts_with_and_without_priorities(torch):
    """priorities=None is the chain it was (ten kernels; thirteen with segments and a selector; one more with n_step > 1,
    what tests/test_nstep_gpu.py counts); priorities= adds three: insert, the second launch of the draw, set"""
    plain = [_loop(_parts(torch, False), priorities=False), _loop(_parts(torch, True), priorities=False),
             _loop(_parts(torch, True), priorities=False, n_step=2)]
    prio = [_loop(_parts(torch, False)), _loop(_parts(torch, True)), _loop(_parts(torch, True), n_step=2)]
    counts = [_node_count(torch, loop) for loop in plain + prio]
    print("graph nodes:", counts)
    assert counts == [10, 13, 14, 13, 16, 17]
    assert all(loop.priorities is None for loop in plain)
    from aquaticgymenv_amd.priority import PrioritizedReplay
    p, q = _parts(torch, False), _parts(torch, False)
    with pytest.raises(ValueError, match="another ring"):
        from aquaticgymenv_amd.trainer import PopulationLoop
        PopulationLoop(p["env"], p["bank"], p["learners"], p["ring"], p["tracker"], 8, priorities=q["per"])
    with pytest.raises(ValueError):
        _loop(dict(p, per=object()))
    for bad in (dict(alpha=1.5), dict(beta0=-0.1), dict(anneal=0), dict(eps=0.0)):
        with pytest.raises(ValueError):
            PrioritizedReplay(p["ring"], p["learners"], **bad)
    from aquaticgymenv_amd.replay import DeviceReplayRing
    with pytest.raises(ValueError, match="multiple of the batch"):
        PrioritizedReplay(DeviceReplayRing(p["env"], 4 * P_NETS * SEG + 1), p["learners"])
    with pytest.raises(ValueError):
        p["per"].draw(8, out=torch.zeros((P_NETS, 9), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        p["per"].update(p["ring"].learner_view(), 9, p["per"].idx)


def test_resume_draws_what_the_original_draws(torch):
    a = _parts(torch, False)
    loop = _loop(a)
    for _ in range(5):
        loop.step()
    torch.cuda.synchronize()
    b = _parts(torch, False)
    for name in ("ring", "learners", "per"):
        b[name].load_state_dict(a[name].state_dict())
    assert torch.equal(a["per"].tree, b["per"].tree) and torch.equal(a["per"].pmax, b["per"].pmax)
    ia, ib = a["per"].draw(8), b["per"].draw(8)
    torch.cuda.synchronize()
    assert torch.equal(ia, ib) and torch.equal(a["per"].weight, b["per"].weight) and bool((ia >= 0).all())
    with pytest.raises(ValueError):
        b["per"].load_state_dict(dict(a["per"].state_dict(), hyper=dict(shape=[1, 1, 1, 1])))
