"""The knife-edge batches of tests/_knife.py on the CPU: the oracle's own margins put worlds of every subject and table
class into both tiers of the kernels' decision (|margin| < BAND_TIGHT: the float64 path; [BAND_TIGHT, BAND): the second
look alone) on both sides of the threshold, and the GPU cases of tests/test_knife_edges.py reach every step and fused
kernel family the dispatch matrix reaches."""
import re

import numpy as np
import pytest

from tests import _dispatch as D
from tests import _knife as KN

N = 65536
MIN_PER_CELL = 100            # worlds per subject x tier x side
TABLES = (("shared", 8), ("shared", 20), ("world", 8), ("world", 11), ("world", 20), ("world", 33))
MARGIN_OF = {"border": (0,), "corner": (0,), "goal": (2,), "circle": (1,), "rect_side": (1,), "rect_corner": (1,),
             "obst_border": (0, 1), "two_obst": (1,)}


def _build(oracle, kind, table, K, n=N, seed=7):
    return KN.build(oracle, kind, n, np.random.RandomState(seed + K), K=K, per_world=table == "world", seed=4242, tick=0)


def test_band_constants_are_read_from_the_sources():
    f = D.read_thresholds(floats=True)
    assert 0 < f["BAND_TIGHT"] < f["BAND_TIGHT_GOAL"] < f["BAND"] < 1e-3
    assert 0 < f["WRAP_BAND"] < 1e-5
    assert (KN.BAND, KN.BAND_TIGHT, KN.WRAP_BAND) == (f["BAND"], f["BAND_TIGHT"], f["WRAP_BAND"])
    ints = D.read_thresholds()
    assert all(isinstance(v, int) for v in ints.values()) and ints == D.THRESHOLDS
    assert {k: f[k] for k in ints} == ints


@pytest.mark.parametrize("table,K", TABLES, ids=["%s-K%d" % t for t in TABLES])
@pytest.mark.parametrize("kind", ("u8", "f32x2"))
def test_every_subject_reaches_both_tiers_on_both_sides(oracle, table, K, kind):
    b = _build(oracle, kind, table, K)
    short = []
    for subject, which in MARGIN_OF.items():
        on = b.subject == subject
        for c in which:
            m = b.margins[c]
            tight, tier2 = KN.tiers(m)
            for name, tier in (("float64 path", tight), ("second look", tier2)):
                for side, s in (("inside", m < 0), ("outside", m > 0)):
                    got = int((on & tier & s).sum())
                    if got < MIN_PER_CELL:
                        short.append("%s margin %d, %s, %s: %d" % (subject, c, name, side, got))
    assert not short, "too few worlds (< %d):\n  %s" % (MIN_PER_CELL, "\n  ".join(short))
    # exactly on the threshold, and at the time limit
    assert int((KN.nearest(b) == 0).sum()) + int((np.abs(KN.nearest(b)) < 1e-9).sum()) >= 10
    tight = KN.tiers(KN.nearest(b))[0]
    for t in (KN.TIME_LIMIT - 1, KN.TIME_LIMIT):
        assert int((tight & (b.time == t)).sum()) >= MIN_PER_CELL, "knife worlds stepping at t = %d" % t
    assert int(((b.time == KN.TIME_LIMIT) & (b.term == 2)).sum()) >= MIN_PER_CELL
    assert int(((b.time == KN.TIME_LIMIT) & (b.term == 1)).sum()) >= MIN_PER_CELL      # collided outranks the time limit


@pytest.mark.parametrize("kind", KN.KINDS)
def test_every_action_kind_reaches_both_tiers_and_the_fold(oracle, kind):
    for table, K in (("shared", 8), ("world", 20)):
        b = _build(oracle, kind, table, K)
        assert (~b.safe).sum() <= N // 100, "bearing policy: too many worlds at its own threshold"
        m = KN.nearest(b)
        tight, tier2 = KN.tiers(m)
        for tier in (tight, tier2):
            for side in (m < 0, m > 0):
                assert int((tier & side & b.safe).sum()) >= 5 * MIN_PER_CELL, (kind, table)
        th = b.state[2].astype(np.float64)      # the fold: post-move headings within 3e-7 of +pi and of -pi
        assert int((b.wrap_margin < 3e-7).sum()) >= MIN_PER_CELL, kind
        assert int(((b.wrap_margin < 3e-7) & (th > 0)).sum()) >= 10 and int(((b.wrap_margin < 3e-7) & (th < 0)).sum()) >= 10


def _fold_f32(th, w):
    """theta + w folded the way a float32 evaluation decides: on the rounded float32 sum"""
    pi_f, two_pi = np.float32(np.pi), np.float64(2 * np.pi)
    s = (th.astype(np.float32) + w.astype(np.float32)).astype(np.float32)
    return np.where(s >= pi_f, s - two_pi, np.where(s <= -pi_f, s + two_pi, s))


@pytest.mark.parametrize("kind", ("f32x2", "sample_c"))
def test_the_fold_worlds_tell_a_float32_fold_from_the_reference(oracle, kind):
    """the batches hold worlds whose heading a fold decided on the float32 sum puts at the other end of [-pi, pi) than
    the reference does -- the worlds that tell a wrong fold in the kernel apart from a right one"""
    b = _build(oracle, kind, "shared", 8)
    a = np.clip(b.action.astype(np.float64), 0.2, 0.5)
    d = (a[1] - a[0]).astype(np.float32)
    d = np.copysign(np.maximum(np.abs(d), np.float32(1e-8)), d)
    w = (d * np.float32(0.4)).astype(np.float32)
    th_ref = KN._probe(oracle, b.state[2].astype(np.float64), b.action)[2]
    flips = np.abs(_fold_f32(b.state[2], w) - th_ref) > 1.0
    assert int(flips.sum()) >= 20, "only %d worlds fold differently in float32" % int(flips.sum())


def test_knife_per_world_rows_sit_where_the_bands_change():
    for K in (8, 9, 11, 17, 20, 33, 64):
        rows = KN.knife_rows(K)
        assert rows[0] == 0 and rows[-1] == K - 1 and all(0 <= r < K for r in rows)
        kreg = D.C["TABLES_KREG"]
        if K > kreg:
            assert kreg - 1 in rows and kreg in rows           # the last row in registers and the first past them
        for sl in KN.SL_ROWS:
            if K % sl > 1:
                assert any(r >= K - K % sl for r in rows[:-1]), (K, sl)     # a row of the partial round, not the last


def test_knife_row_is_the_nearest_and_has_absent_neighbours(oracle):
    b = _build(oracle, "u8", "world", 20, n=4096)
    t = b.obst
    on = np.isin(b.subject, ("circle", "rect_side", "rect_corner"))
    p = KN._probe(oracle, b.state[2].astype(np.float64), b.action)
    post = np.stack([b.state[0] + b.state[5] + p[0], b.state[1] + b.state[6] + p[1]])
    d = np.stack([KN._dist_to_rows_each(post, t[:, j]) for j in range(t.shape[1])])
    near = np.argmin(d, axis=0)
    assert np.all(np.sort(d, axis=0)[1][on] > 1.0), "another row is close to the knife row's surface"
    idx = np.flatnonzero(on)
    for nb in (-1, 1):
        j = near[idx] + nb
        ok = (j >= 0) & (j < t.shape[1])
        assert np.all(t[idx[ok], j[ok], 2] < 0)
    assert set(near[idx].tolist()) == set(KN.knife_rows(20))


def _family(name):
    return re.sub(r"<\d+", "<*", name)


def test_knife_cases_reach_every_kernel_family_of_the_matrix():
    """every step and fused kernel template the dispatch matrix reaches, with its non-action template arguments, is
    launched by some knife case; and every one it reaches at ordinary batch sizes, with every action kind of the knife
    cases"""
    from tests import test_dispatch_matrix as M
    from tests import test_kernel_coverage as C
    from tests import test_knife_edges as E
    reached, small = set(), set()
    for cell in M.CELLS:
        for k in M.cell_kernels(cell):
            if k.startswith(("step", "rollout")) and k not in C.UNREACHABLE:
                reached.add(k)
                if cell.N < D.C["NS_INTERLEAVE_MIN"] and cell.kind in E.KINDS:
                    small.add(k)
    knife = set()
    for case in E.CASES:
        knife |= E.case_kernels(case)
    missing = sorted({_family(k) for k in reached} - {_family(k) for k in knife})
    assert not missing, "kernel families without a knife case:\n  " + "\n  ".join(missing)
    missing = sorted(small - knife)
    assert not missing, "kernels without a knife case:\n  " + "\n  ".join(missing)
    assert {c.kind for c in E.CASES} == set(E.KINDS) and {c.mode for c in E.CASES} == set(D.MODES)
    assert all(c.N >= 65536 for c in E.CASES)
