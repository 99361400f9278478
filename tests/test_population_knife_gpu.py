"""Knife-edge GPU tests of the eight newer device libraries (lbank, segments, pbt, qmap, fastpol, nstep, prio, her): what the
second mutation audit (tools/mutation_audit.py, profiles/LOG.md) found alive under the files that compare random batches
with a model.  A random batch never puts a value ON a decision: every test here constructs an input on the boundary and one
step to either side of it, ASSERTS that it is there before the launch (an input that stops being an edge after a later
change must fail, not pass without testing anything), and takes what it expects from the numpy models under tests/ or from
float64 / exact rational arithmetic written out here -- never from a second run of the library.  The library's host
entries are used to find and to verify the edge only."""
import ctypes
import fractions

import numpy as np
import pytest

from tests import _her_model as HM
from tests import _nstep_model as NM
from tests import _prio_model as PM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHUNK = 8                                                    # AQUAHER_CHUNK == AQUANST_CHUNK: H and n sit at 7, 8 and 9


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _same(got, want, what):
    for k, v in got.items():
        assert np.array_equal(_bits(v), _bits(want[k])), (what, k, v, want[k])


F = fractions.Fraction


# ================================================================================================ her
@pytest.fixture(scope="module")
def her():
    from aquaticgymenv_amd import _her_capi
    from tests import test_her_gpu
    assert _her_capi.CHUNK == CHUNK
    return _her_capi, test_her_gpu._run


def _fused_gap(qx, qy, gx, gy):
    """the gap with the squared distance as ONE fused multiply-add, fma(dx, dx, dy dy): exact rationals, rounded once"""
    dx, dy = np.float64(np.float32(qx)) - np.float64(np.float32(gx)), np.float64(np.float32(qy)) - np.float64(np.float32(gy))
    yy = np.float64(dy * dy)
    ss = np.float64(float(F(float(dx)) * F(float(dx)) + F(float(yy))))       # float(Fraction) rounds correctly
    return np.float64(100.0) * np.sqrt(ss) - np.float64(5.0)


def _gap_edges():
    """Positions q and goals g, float32, at a distance of 0.05 (normalised) to the last bit: the goal is tiny, so q - g has
    the resolution of a float64.  -> dict name -> (qx, qy, gx, gy) with the model's gap: exactly 0 (twice); the smallest value
    above 0 and the largest below it; and a pair (both kinds, where the search meets them) on which fma(dx, dx, dy dy) decides the other way."""
    rng = np.random.RandomState(1)
    q = np.float32([0.03, 0.04])
    short = float(np.hypot(np.float64(q[0]), np.float64(q[1]))) - 0.05              # q is this much too far (or too near)
    th = rng.rand(300000) * 0.6 + 0.6                                                # directions around q's own
    rad = short / np.cos(th - np.arctan2(0.04, 0.03))                                # |q - g| = 0.05 to first order
    GX, GY = (rad * np.cos(th)).astype(np.float32), (rad * np.sin(th)).astype(np.float32)
    gap = HM.gap(q[0], q[1], GX, GY)
    tiny = np.spacing(np.float64(5.0))                                               # one step of 100 sqrt(..) at 5
    zero, above, below = np.nonzero(gap == 0.0)[0], np.nonzero(gap == tiny)[0], np.nonzero(gap == -tiny)[0]
    assert len(zero) >= 2 and len(above) and len(below), "the search met no gap of exactly 0, or no neighbour of it"
    pick = lambda i: (q[0], q[1], GX[i], GY[i])                                      # noqa: E731
    out = dict(zero=pick(zero[0]), zero_too=pick(zero[-1]), above=pick(above[0]), below=pick(below[0]))
    # where one rounding fewer turns the decision (the exact rational sum, rounded once)
    for name, cells, other in (("fused_leaves", zero, lambda v: v > 0.0), ("fused_enters", above, lambda v: v <= 0.0)):
        for i in cells[:3000]:
            if other(_fused_gap(*pick(i))):
                out[name] = pick(i)
                break
    assert "fused_leaves" in out or "fused_enters" in out, "no pair on which the contracted sum decides the other way"
    return out


HER_N, HER_ROUNDS = 16, 12


def _her_ring(edges, continuous):
    """World w holds edge w: its step of round 0 ends at q, and every later step of the world ends at g.  No step ends an
    episode and every slot is an experience, so M = min(12, H) and any k >= 1 replays round 0 under the goal g."""
    cap = HER_N * HER_ROUNDS
    rng = np.random.RandomState(2)
    ring = dict(capacity=cap, s=rng.rand(5, cap).astype(np.float32), s2=rng.rand(5, cap).astype(np.float32),
                r=(rng.rand(cap) * 2 - 1).astype(np.float32), d=np.zeros(cap, np.uint8), ok=np.ones(cap, np.uint8),
                a=(rng.rand(2, cap) * 0.3 + 0.2).astype(np.float32) if continuous else rng.randint(0, 3, cap).astype(np.uint8))
    for w, (qx, qy, gx, gy) in enumerate(edges):
        ring["s"][0:2, w] = np.float32(qx) + np.float32(0.01), np.float32(qy) - np.float32(0.02)
        ring["s2"][0:2, w] = qx, qy
        ring["s2"][0, w + HER_N::HER_N] = gx
        ring["s2"][1, w + HER_N::HER_N] = gy
    return ring, (0, cap, cap - HER_N, 11)                    # full, the cursor back at 0: round 0 is the oldest, age 11


@pytest.mark.parametrize("table", [True, False], ids=["table", "scalar"])
@pytest.mark.parametrize("continuous", [False, True], ids=["u8", "f32x2"])
def test_her_success_at_a_gap_of_exactly_zero(torch, her, continuous, table):
    """gap_new <= 0 is a success: a step that ends EXACTLY one radius sum from the relabelled goal (gap 0.0 in the header's
    rounded float64), one step of the gap inside and outside, one float32 step of the position inside and outside, and
    pairs on which a fused dx dx + dy dy lands on the other side."""
    capi, run = her
    edges = _gap_edges()
    names = sorted(edges)
    cells = [edges[k] for k in names]
    for k in ("zero", "zero_too"):                           # one float32 step of q to either side of the exact zero
        qx, qy, gx, gy = edges[k]
        cells += [(np.nextafter(qx, np.float32(1)), qy, gx, gy), (np.nextafter(qx, np.float32(0)), qy, gx, gy)]
    assert len(cells) <= HER_N
    # the edge, by the model and by the library's own host entry
    for name, (qx, qy, gx, gy) in zip(names, cells):
        g = float(HM.gap(qx, qy, gx, gy))
        assert {"zero": g == 0.0, "zero_too": g == 0.0, "above": 0.0 < g < 1e-15, "below": -1e-15 < g < 0.0}.get(name, True), (name, g)
        r, d = capi.reward([qx + np.float32(0.01), qy - np.float32(0.02), 0, 0, 0], [qx, qy, 0, 0, 0], gx, gy)
        assert d == (HM.TERM_SUCCESS if g <= 0.0 else 0), (name, g, d)
    outside = [float(HM.gap(*c)) for c in cells[len(names):]]
    assert sum(1 for g in outside if g > 0.0) == 2 and sum(1 for g in outside if g < 0.0) == 2, outside
    ring, header = _her_ring(cells, continuous)
    P, B = 2, 8 * len(cells)
    idx = np.tile(np.arange(len(cells), dtype=np.int32), (P, 8))
    t, seeds = [3, 2 ** 33 + 1], [11, 2 ** 63 + 5]
    for H in (CHUNK - 1, CHUNK, CHUNK + 1):
        want = HM.relabel(ring, header, HER_N, idx, H, 1.0, t, seeds if table else [seeds[1]] * P)
        assert (want["m"] == min(H, HER_ROUNDS)).all()
        later = want["k"].reshape(P * 8, len(cells)) >= 2    # samples replayed under g (k >= 1), per edge
        assert later.sum(axis=0).min() >= 2, "an edge no sample looks at"
        hit = want["d"].reshape(P * 8, len(cells))[:, :len(names)]
        for col, name in enumerate(names):                   # what the edge must decide, in the expected rows themselves
            gap = float(HM.gap(*cells[col]))
            assert (hit[later[:, col], col] == (HM.TERM_SUCCESS if gap <= 0.0 else 0)).all(), name
        got = run(torch, capi, ring, header, HER_N, idx, H, 1.0, t, seeds=seeds if table else None, seed=None if table else seeds[1])
        _same(got, want, ("gap", H))


@pytest.mark.parametrize("table", [True, False], ids=["table", "scalar"])
@pytest.mark.parametrize("continuous", [False, True], ids=["u8", "f32x2"])
def test_her_draw_equal_to_the_threshold_does_not_relabel(torch, her, continuous, table):
    """relabel iff r[0] < floor(ratio 2^32): the ratio is chosen so that the threshold IS the first word of one sample of
    the second row, then half a unit above it (the floor), then one above it"""
    capi, run = her
    edges = _gap_edges()
    ring, header = _her_ring([edges["zero"], edges["above"]], continuous)
    P, B, J = 2, 24, 13
    idx = np.tile(np.arange(2, dtype=np.int32), (P, B // 2))
    t, seeds = [7, 2 ** 40], [5, 2 ** 64 - 9]
    keys = seeds if table else [seeds[0]] * P
    word = int(HM.draws(keys[1], t[1], B)[0][J])
    assert 0 < word < 2 ** 32 - 1
    for H in (CHUNK - 1, CHUNK, CHUNK + 1):
        for add, relabelled in ((0.0, False), (0.5, False), (1.0, True)):
            ratio = (word + add) / 4294967296.0              # exact: 33 bits at most
            assert capi.threshold(ratio) == word + int(add) == HM.threshold(ratio), "the draw is not on the threshold"
            want = HM.relabel(ring, header, HER_N, idx, H, ratio, t, keys)
            assert want["m"][B + J] == min(H, HER_ROUNDS) and (want["k"][B + J] != 0) == relabelled
            got = run(torch, capi, ring, header, HER_N, idx, H, ratio, t, seeds=seeds if table else None, seed=None if table else seeds[0])
            _same(got, want, ("threshold", H, add))


# ================================================================================================ nstep
@pytest.fixture(scope="module")
def nstep():
    from aquaticgymenv_amd import _nstep_capi
    from tests import test_nstep_gpu
    assert _nstep_capi.CHUNK == CHUNK
    return _nstep_capi, test_nstep_gpu._run_fold


def _fold_variants(r, g):
    """R of one window computed three wrong ways, exactly: the sum contracted into one fma per step; the product rounded to
    float32 first; gamma not rounded to float32 is the caller's business.  -> (fused, float_product) as float32"""
    pw, fused, fprod = np.float64(1.0), np.float64(r[0]), np.float64(r[0])
    for x in r[1:]:
        pw = np.float64(pw * g)
        fused = np.float64(float(F(float(pw)) * F(float(x)) + F(float(fused))))
        fprod = np.float64(fprod + np.float64(np.float32(np.float64(pw * np.float64(x)))))
    return np.float32(fused), np.float32(fprod)


def _cancelling_rewards(rng, n, g):
    """n float32 rewards whose discounted sum cancels twice at the end: the last two are the float32 nearest to minus what
    has accumulated, over their power of gamma.  What is left is the rounding of the steps before, which a float32 sees."""
    r = list(((rng.rand(n - 2) * 2 - 1) * 3).astype(np.float32))
    for _ in range(2):
        pw, acc = np.float64(1.0), np.float64(r[0])
        for x in r[1:]:
            pw = np.float64(pw * g)
            acc = np.float64(acc + np.float64(pw * np.float64(x)))
        r.append(np.float32(-acc / np.float64(pw * g)))
    return np.array(r, np.float32)


NST_N = 32


@pytest.mark.parametrize("table", [True, False], ids=["table", "scalar"])
@pytest.mark.parametrize("continuous", [False, True], ids=["u8", "f32x2"])
def test_nstep_return_under_cancellation(torch, nstep, continuous, table):
    """R = sum gamma^k r_k in float64, every product and sum rounded, one rounding to float32 at the end.  Rewards that cancel
    leave only those roundings: a fused multiply-add, a float32 product or an unrounded gamma each change the float32 that
    comes out.  Also a first reward of -0.0, which a sum started from +0.0 would lose, alone (n = 1) and behind zeros."""
    capi, run = nstep
    gamma = 0.98 if table else 0.97
    g = NM.rounded_gamma(gamma)
    assert float(g) != gamma
    for n in (CHUNK - 1, CHUNK, CHUNK + 1):
        rounds = n + 1
        cap = NST_N * rounds
        rng = np.random.RandomState(40 + n)
        ring = dict(capacity=cap, s=(rng.rand(5, cap) * 2 - 1).astype(np.float32), s2=(rng.rand(5, cap) * 2 - 1).astype(np.float32),
                    r=np.zeros(cap, np.float32), d=np.zeros(cap, np.uint8), ok=np.ones(cap, np.uint8),
                    a=(rng.rand(2, cap) * 0.3 + 0.2).astype(np.float32) if continuous else rng.randint(0, 3, cap).astype(np.uint8))
        fused_differs = product_differs = gamma_differs = 0
        for w in range(NST_N - 2):
            r = _cancelling_rewards(rng, n, g)
            ring["r"][w:n * NST_N:NST_N] = r
            want = NM.folded_return(ring["r"], list(range(w, n * NST_N, NST_N)), g)
            fused, fprod = _fold_variants(r, g)
            fused_differs += int(fused != want)
            product_differs += int(fprod != want)
            gamma_differs += int(NM.folded_return(ring["r"], list(range(w, n * NST_N, NST_N)), np.float64(gamma)) != want)
        # the input is on the edge: each wrong way of rounding shows in the float32 of several worlds
        assert min(fused_differs, product_differs, gamma_differs) >= 3, (n, fused_differs, product_differs, gamma_differs)
        ring["r"][NST_N - 2] = np.float32(-0.0)              # world 30: -0.0, then zeros; world 31 ends at once with -0.0
        ring["r"][NST_N - 1], ring["d"][NST_N - 1] = np.float32(-0.0), 2
        header = (0, cap, cap - NST_N, n)                    # full: round 0 is the oldest, its windows close n - 1 rounds later
        idx = np.arange(2 * NST_N, dtype=np.int32).reshape(2, NST_N)
        hyper = np.arange(16, dtype=np.float64).reshape(2, 8) / 3 + 1
        hyper[:, 0] = gamma
        want = NM.fold(ring, header, NST_N, idx, n, hyper=hyper) if table else NM.fold(ring, header, NST_N, idx, n, gamma=gamma)
        assert want["len"][:NST_N - 1].tolist() == [n] * (NST_N - 1) and want["len"][NST_N - 1] == 1
        assert np.signbit(want["r"][NST_N - 1]) and want["r"][NST_N - 1] == 0
        got = run(torch, capi, ring, header, NST_N, idx, n, hyper=hyper) if table else run(torch, capi, ring, header, NST_N, idx, n, gamma=gamma)
        _same(got, want, ("cancellation", n))


# ================================================================================================ prio
@pytest.fixture(scope="module")
def prio():
    from aquaticgymenv_amd import _prio_capi
    from tests import test_prio_gpu
    return _prio_capi, test_prio_gpu


def test_prio_quantiser_ties_floor_and_ceiling(torch, prio):
    """q = min(max(rint((td + eps)^alpha 2^20), 1), 2^31 - 1), ties to even.  alpha = 1 makes the float64 reference exact up
    to the library's stated 2^-44: four ties k + 1/2, two with k odd and two with k even (asserted through aquaprio_pow), a priority that rounds to
    0, one far above the ceiling, and plain values on both sides of a half"""
    capi, PG = prio
    shape = PG.ONE_NODE
    capacity, N, seg, P = shape
    cases = []                                               # (td float32, eps, expected leaf)
    for k, eps in PM.ties(capi):
        assert abs(eps * PM.ONE - (k + 0.5)) <= (k + 0.5) * 2.0 ** -44
        cases.append((0.0, eps, k + (k & 1)))               # the even neighbour of k + 1/2
    cases.append((0.0, 1e-9, 1))                             # rint(0.001) = 0: the floor
    cases.append((0.0, 0.4 / PM.ONE, 1))
    cases.append((3000.0, 1e-3, PM.QMAX))                    # 3.1e9: the ceiling
    for v in (2.25, 2.75, 1000.4, 2047.9):
        x = float(PM.pi64(np.float32(v), 1.0, 1e-3)) * PM.ONE
        assert abs(x - np.rint(x)) > 1e-3 and abs(abs(x - np.floor(x)) - 0.5) > 1e-3    # far from an integer's edge: 2^-44 x cannot matter
        cases.append((v, 1e-3, int(min(max(np.rint(x), 1), PM.QMAX))))
    assert all(c[2] % 2 == 0 for c in cases[:4]) and sum(1 for c in cases[:4] if c[2] * 1.0 > c[1] * PM.ONE) == 2      # two round up
    for td, eps, want in cases:                              # the library's host entry agrees with the reference on every case
        assert capi.quantise(float(np.float32(td)), 1.0, eps) == want, (td, eps, want)
    for n, (td, eps, want) in enumerate(cases):
        trees = PG.Trees(torch, capi, shape, seed=3)
        slots = np.array([[n, 8 + n, 63 - n]], dtype=np.int32)
        tds = torch.as_tensor(np.full((1, 3), td, dtype=np.float32)).to(DEV)
        rc = capi.lib.aquaprio_set(trees.tree.data_ptr(), trees.tree.numel(), trees.pmax.data_ptr(), *shape,
                                   torch.as_tensor(slots).to(DEV).data_ptr(), tds.data_ptr(), 3, 1.0, eps, PG._stream(torch))
        capi.check(rc, "aquaprio_set")
        for slot in slots[0]:
            trees.model.leaves[0, PM.leaf_of_slot(int(slot), N, seg)[1]] = want
        trees.model.pmax[0] = max(PM.ONE, want)
        trees.check(("quantiser", td, eps))


# L0 = 1, 64, 65 and 64 * 64 + 1 leaves (one network that owns every world): one node, a full node, and a level boundary
# at each of the two levels above the leaves
PRIO_SHAPES = {1: (1, 1, 1, 1), 64: (64, 8, 8, 1), 65: (65, 13, 13, 1), 4097: (17 * 241, 241, 241, 1)}
PRIO_BOUNDARIES = {1: (), 64: (1, 37, 63), 65: (1, 32, 64), 4097: (63, 64, 2048, 4032, 4096)}


def _leaves_with_front(L0, b, front, total, empty):
    """L0 leaves that sum to `total` with exactly `front` in front of leaf b, both parts spread evenly; empty: leaf b holds
    nothing and leaf b + 1 what it held"""
    leaves = np.zeros(L0, dtype=np.int64)
    leaves[:b] = front // b
    leaves[0] += front % b
    leaves[b:] = (total - front) // (L0 - b)
    leaves[L0 - 1] += (total - front) % (L0 - b)
    if empty and b + 1 < L0:
        leaves[b + 1] += leaves[b]
        leaves[b] = 0
    return leaves


@pytest.mark.parametrize("big", [False, True], ids=["small-sums", "sums-above-2^32"])
@pytest.mark.parametrize("L0", sorted(PRIO_SHAPES))
def test_prio_descent_with_the_draw_on_a_child_boundary(torch, prio, L0, big):
    """The descent takes the first child whose prefix sum EXCEEDS u = (r T) >> 64, r the 64-bit draw.  The leaves are crafted
    so that the sum in front of leaf b is u of sample 0 exactly (leaf b is drawn, not b - 1), one less and one more, for b
    inside a node, at the end of a node and at the boundary between two nodes of either upper level; and the same with leaf b
    empty.  With sums above 2^32 the low word of the draw moves u, so a draw of 32 bits lands in front of the boundary."""
    capi, PG = prio
    shape = PRIO_SHAPES[L0]
    capacity, N, seg, P = shape
    B, t, seed = 8, 5, 2 ** 61 + 3
    rng = np.random.RandomState(L0)
    base = rng.randint(1 << 27, 1 << 29, L0).astype(np.int64) if big else rng.randint(1, 1 << 12, L0).astype(np.int64)
    total = int(base.sum())
    r0 = PM.uniform(seed, t + 1, B)[0]
    u0 = (r0 * total) >> 64
    trees = PG.Trees(torch, capi, shape, seed=1)
    assert trees.lay["leaves"] == L0
    if not PRIO_BOUNDARIES[L0]:
        trees.load(base.astype(np.uint32).reshape(1, L0))
        idx, _, q = trees.draw(B, [t], [seed], capacity)
        want = PM.draw(base.astype(np.uint32), trees.lay["n"], seed, t, B, 0, N, seg, capacity)
        assert np.array_equal(idx[0], want[0]) and np.array_equal(q[0], want[1])
        return
    if big and L0 > 64:
        assert (((r0 >> 32) << 32) * total) >> 64 < u0, "the low word of the draw does not move u"
    ran = 0
    for b in PRIO_BOUNDARIES[L0]:
        for delta in (0, -1, 1):
            for empty in (False, True):
                front = u0 + delta
                if not (b <= front and front + 2 * (L0 - b) <= total):
                    continue
                leaves = _leaves_with_front(L0, b, front, total, empty)
                if leaves.max() > PM.QMAX:                   # (a part too large for its leaves: another b holds this case)
                    continue
                assert leaves.min() >= 0 and int(leaves.sum()) == total and int(leaves[:b].sum()) == front
                assert ((r0 * int(leaves.sum())) >> 64) - int(leaves[:b].sum()) == -delta      # the draw is on (next to) the boundary
                trees.load(leaves.astype(np.uint32).reshape(1, L0))
                idx, _, q = trees.draw(B, [t], [seed], capacity)
                want = PM.draw(leaves.astype(np.uint32), trees.lay["n"], seed, t, B, 0, N, seg, capacity)
                if delta == 0:                               # ON the boundary: leaf b (the next one that holds anything), never b - 1
                    assert want[0][0] == PM.slot_of_leaf(0, b + (1 if empty and b + 1 < L0 else 0), N, seg)
                if delta == 1:
                    assert want[0][0] == PM.slot_of_leaf(0, b - 1, N, seg)
                assert np.array_equal(idx[0], want[0]) and np.array_equal(q[0], want[1]), (b, delta, empty, idx[0], want[0])
                ran += 1
    assert ran >= 6, "too few boundaries fit the leaves"


# ================================================================================================ pbt
@pytest.fixture(scope="module")
def pbt():
    from tests import _pbt
    from tests import test_pbt_gpu
    return _pbt, test_pbt_gpu


def test_pbt_negative_zero_ranks_below_zero(torch, pbt):
    """the ranking orders the float32 BITS: -0.0 lies below +0.0 (aqua_pbt.h's ordered key).  Scores of nothing but the two
    zeros, the negative ones at the lower indices: a ranking that calls them equal would keep the index order"""
    T, PG = pbt
    for P in (4, 65):
        score = np.where(np.arange(P) % 2 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        episodes = np.full(P, 3, dtype=np.uint64)
        order = T.ranking(score, episodes)
        assert order == list(range(1, P, 2)) + list(range(0, P, 2)) and order != sorted(order)
        rig = PG.Rig(torch, P, fraction=0.5, ready=1, seed=3)
        rig.set(score, episodes)
        rig.sel.select()
        rig.check(("zeros", P))
        k = P // 2
        assert rig.model.winners == order[:k] and sorted(rig.model.losers) == sorted(order[P - k:]) and all(p % 2 == 0 for p in rig.model.losers)


def test_pbt_perturbation_clamps_on_both_sides(torch, pbt):
    """lr and gamma of a child are clipped to their bounds: bounds so narrow that the perturbed values of the fill fall below,
    inside and above them (asserted on the model before the launch)"""
    T, PG = pbt
    P = 64
    config = dict(fraction=0.5, ready=1, seed=77, lr_bounds=(4e-4, 6e-4), gamma_bounds=(0.93, 0.95))
    rng = np.random.RandomState(6)
    score, episodes = rng.uniform(-1, 1, P).astype(np.float32), np.full(P, 5, dtype=np.uint64)
    dry = T.fill(T.Model(P, PG.BLOB, **config))
    dry.select(score, episodes)
    assert len(dry.losers) == P // 2
    for col, (lo, hi) in ((T.HYPER_LR, config["lr_bounds"]), (T.HYPER_GAMMA, config["gamma_bounds"])):
        v = dry.hyper[dry.losers, col]
        assert (v == lo).sum() >= 3 and (v == hi).sum() >= 3 and ((v > lo) & (v < hi)).sum() >= 1, (col, v)
    rig = PG.Rig(torch, P, **config)
    rig.set(score, episodes)
    rig.sel.select()
    rig.check("clamps")
    assert np.array_equal(rig.model.hyper.view(np.uint64), dry.hyper.view(np.uint64))


@pytest.mark.parametrize("strategy,name", [(0, "double_ref"), (1, "double"), (2, "fixed"), (3, "standard")])
def test_prio_weighted_td_error_is_rounded_once(torch, prio, strategy, name):
    """aqua_prio.h: the importance weight multiplies the TD error in double, and the product is rounded ONCE to the float32 the
    backward pass starts from.  float32(w) * float32(delta) differs only where delta is no float32: the integer network of
    tests/test_dqn_knife_gpu.py::test_the_td_error_is_formed_in_double (Q at 2^33, exact in the kernel's forward pass), with
    s' = s, a = arg-max Q(s), target = online network and gamma = 1/2, so that delta = Q_a / 2 - r EXACTLY, some 33 bits.
    One valid sample per call: the gradient of the last layer's bias is then 2 float32(w delta) with no sum behind it, and is
    compared bit for bit; so is td_out = float32(|delta|), which carries no weight."""
    capi, PG = prio
    from tests import _lbank as K
    from tests import _learner as L
    cap, size, B, at = 300, 257, 8, 3
    (k0, b0), (k1, b1), (k2, b2) = L.int_layers("plain")
    layers = [(k0, b0), (k1, (b1 + np.float32(2 ** 20)).astype(np.float32)), ((1025 * np.abs(k2) + k2).astype(np.float32), b2)]
    ring = L.int_ring(cap, size, 3, bad_ok=0.1)
    ring["s2"][:, :size] = ring["s"][:, :size]
    ring["d"][:] = 0
    st = K.make_state(1, 1, [layers], [layers], fresh=True)
    theta = st["theta"][0]
    assert np.array_equal(theta, L.flatten(layers)) and np.array_equal(st["theta_target"][0], theta)
    q_all = L.forward(theta.astype(np.float64), ring["s"][:, :size].T.astype(np.float64))[2]
    assert np.abs(q_all).max() < 2 ** 52 and ((q_all == q_all.max(axis=1, keepdims=True)).sum(axis=1) == 1).all()
    ring["a"][:size] = np.argmax(q_all, axis=1)
    gamma = 0.5
    hyper = K.hypers(1)
    hyper[:, 0] = gamma
    # (slot, weight) pairs on which the two ways of rounding differ, found and asserted on the CPU
    rng = np.random.RandomState(9)
    pairs = []
    for slot in np.flatnonzero(ring["ok"][:size] != 0)[:40]:
        qa = q_all[slot].max()
        delta = np.float64(qa - (np.float64(ring["r"][slot]) + gamma * qa))
        assert abs(delta) > 2.0 ** 31 and np.float64(np.float32(delta)) != delta        # no float32 holds it
        for w in rng.uniform(0.1, 1.0, 6).astype(np.float32):
            once, twice = np.float32(np.float64(w) * delta), np.float32(w) * np.float32(delta)
            if once != twice and len(pairs) < 3:
                pairs.append((int(slot), w, delta, once))
                break
    assert len(pairs) == 3, "no sample on which one rounding and two differ"
    run = K.Runner(torch, DEV)
    dev_ring = L.DeviceRing(torch, ring, DEV)
    for slot, w, delta, once in pairs:
        idx = np.full((1, B), -1, dtype=np.int32)
        idx[0, at] = slot
        weight = np.full((1, B), 7.0, dtype=np.float32)
        weight[0, at] = w
        eff = L.effective(idx[0], ring)
        ref = PM.weighted_gradient(theta, theta, ring, eff, weight[0], gamma, name, np.float64, "mse")
        a = int(ring["a"][slot])
        assert ref["n"] == 1 and ref["td"][at] == abs(delta) and (np.delete(ref["td"], at) == -1).all()
        assert ref["S"][-3:][a] == np.float64(w) * delta and not np.delete(ref["S"][-3:], a).any()       # b2's gradient: the one product
        want = ref["S"][-3:].astype(np.float32) * np.float32(2.0)
        assert want[a] == once * np.float32(2.0) != np.float32(w) * np.float32(delta) * np.float32(2.0)
        d = K.to_device(torch, st, B, DEV)
        td = torch.full((1, B), 7.0, dtype=torch.float32, device=DEV)
        PG._prio_update(torch, capi, run, d, dev_ring, torch.as_tensor(idx).to(DEV), B, strategy, run.hyper_dev(hyper),
                        torch.as_tensor(weight).to(DEV), td)
        out = K.read(torch, d)
        assert np.array_equal(out["grad"][0][-3:].view(np.uint32), want.view(np.uint32)), (slot, w, out["grad"][0][-3:], want)
        assert np.array_equal(td.cpu().numpy()[0].view(np.uint32), ref["td"].astype(np.float32).view(np.uint32))


# ================================================================================================ fastpol
def test_fastpol_per_network_epsilon_by_its_bits(torch):
    """aqua_fastpol.h: a per-network epsilon is read on the device by its bits -- NaN and every negative value never explore,
    everything else is compared with the draw, so +infinity (and 1) explore in EVERY world and +0 in none.  The exact dyadic
    network of tests/_fastpol.py gives the greedy actions without a tolerance and tests/_episodes.py the draws: every action
    and q_taken of a bank whose networks differ in nothing but their epsilon"""
    from aquaticgymenv_amd.fastpolicy import FastActor
    from aquaticgymenv_amd.qbank import QNetworkBank
    from tests import _episodes as E
    from tests import _fastpol as FP
    eps = np.array([np.inf, np.nan, -np.inf, 1.0, 0.0, -1.0, -0.0, 0.5], dtype=np.float32)
    P, seg = len(eps), 33
    n, ld, off, seed, tick = P * seg - 5, P * seg + 11, 3 << 20, 0x1234567890ABCDEF, (1 << 32) + 5
    layers = FP.exact_layers("plain")
    x = FP.exact_inputs(n, 7)
    q = FP.exact_reference(layers, x)
    greedy = np.argmax(q, axis=1).astype(np.uint8)
    u, drawn = E.draws_vectorised(n, seed, off, tick)
    net = np.arange(n) // seg
    with np.errstate(invalid="ignore"):
        explores = (~np.isnan(eps[net])) & (~np.signbit(eps[net])) & (u < eps[net])
    want = np.where(explores, drawn, greedy).astype(np.uint8)
    # the edge: +infinity and 1 explore everywhere and visibly, NaN and the negatives nowhere, 1/2 in some worlds
    assert explores[net == 0].all() and explores[net == 3].all() and (want[net == 0] != greedy[net == 0]).sum() >= 10
    assert not explores[np.isin(net, (1, 2, 4, 5, 6))].any() and 0 < explores[net == 7].sum() < (net == 7).sum()
    fast = FastActor(QNetworkBank([layers] * P, seg, DEV))
    fast.epsilon = torch.as_tensor(eps).to(DEV)
    buf = torch.full((5, ld), 1.0e30, dtype=torch.float32, device=DEV)
    buf[:, :n] = torch.as_tensor(x.T.copy())
    act = torch.full((ld,), 0xEE, dtype=torch.uint8, device=DEV)
    qt = torch.full((ld,), -777.0, dtype=torch.float32, device=DEV)
    fast.act(buf, n=n, out=act, q_taken=qt, env_offset=off, seed=seed, tick=tick)
    torch.cuda.synchronize()
    a, t = act.cpu().numpy(), qt.cpu().numpy()
    assert np.array_equal(a[:n], want), np.flatnonzero(a[:n] != want)[:8]
    assert np.array_equal(t[:n].astype(np.float64), q[np.arange(n), want.astype(np.int64)])
    assert bool((a[n:] == 0xEE).all()) and bool((t[n:] == -777.0).all())
