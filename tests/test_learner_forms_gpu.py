"""GPU tests of the learner's loss forms (DQNLearner(loss=...), AQUALRN_LOSS_REFERENCE in include/aqua_learner.h).

"mse" is the textbook mean squared TD error; "reference" is what main/impl/dqn.py:243-247 executes, the [B,1] prediction
broadcast against the [B,3] targets: delta_b = 3 Q_a - y - sum_{j != a} Q_j, scale 2 / (3 B_eff), loss
1 / (3 B_eff) sum_b sum_j (Q_a - T_bj)^2.  The model of both is tests/_learner.py::gradient(form=...), held to autograd on
the CPU by tests/test_learner_model_cpu.py; here the kernels are held to the model under the contracts of
test_learner_gpu.py (bit-exact with integer data; 4 E_g / 4 E_l against float64 otherwise, E from the float32 numpy run
of the SAME form) and, skipping the model, to tests/_learner_autograd.py directly.  test_learner_gpu.py,
test_launch_regimes_gpu.py and test_trainer_gpu.py are unchanged: that "mse" did not move is their evidence.
"""
import numpy as np
import pytest

from tests import _learner as L
from tests import _learner_autograd as A
from tests.test_learner_gpu import (CASES, GAP_CAP, U, _check_step, _float_ring, _idx, _learner, _mixed_indices, _nets, _same,
                                    _set, _state)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEPT = ("theta", "theta_target", "m", "v", "t", "blob", "target_blob")


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


# ------------------------------------------------------------------------------------------------ (1) exact
@pytest.mark.parametrize("strategy", L.STRATEGIES)
@pytest.mark.parametrize("B", [1, 31, 33, 65, 325])
def test_exact_integer_gradient_of_the_reference_form(torch, B, strategy):
    """test_learner_gpu.py::_check_exact's recipe (integer networks, int_ring(300, 257), gamma = 1, invalid indices and a
    duplicate from B = 31 on) with loss="reference": delta = 3 Q_a - y - sum_{j != a} Q_j is an integer below 2^24 like
    every sum behind it (abs_sums' extended bound, asserted in int64 before the launch), so the gradient is
    float32(S_ref) * float32(2 / (3 B_eff)) BIT FOR BIT and the loss, an exact double sum, is within 4 x 2^-24."""
    cap, size = 300, 257
    layers, target = L.int_layers("plain"), L.int_layers("plain", salt=1)
    ring = L.int_ring(cap, size, B, bad_ok=0.1)
    idx = _mixed_indices(np.random.RandomState(B + 1), B, ring, cap)
    eff = L.effective(idx, ring)
    theta, theta_t = L.flatten(layers), L.flatten(target)
    worst, S, ref = L.abs_sums(theta, theta_t, ring, eff, strategy, form="reference")
    worst_mse, S_mse, _ = L.abs_sums(theta, theta_t, ring, eff, strategy)
    print("B %d %s: largest sum of |terms| %d = 2^%.1f (mse form: 2^%.1f)" % (B, strategy, worst, np.log2(worst), np.log2(worst_mse)))
    assert worst_mse < worst < 2 ** 24, worst               # asserted in int64 before the kernel runs
    assert not np.array_equal(S, S_mse) and not np.array_equal(S, 3 * S_mse)
    lrn = _learner(torch, layers, target, gamma=1.0, strategy=strategy, loss="reference")
    out = torch.full((B + 8,), 77, dtype=torch.int32, device=DEV)
    lrn.update(L.DeviceRing(torch, ring, DEV), B, idx=_idx(torch, idx), idx_out=out)
    st = _state(torch, lrn)
    got = out.cpu().numpy()
    assert np.array_equal(got[:B], eff) and bool((got[B:] == 77).all())
    n = int((eff >= 0).sum())
    assert n == ref["n"] and (B < 8 or (n < B and len(set(eff[eff >= 0].tolist())) < n))
    want = S.astype(np.float32) * np.float32(2.0 / (3 * n))
    assert np.array_equal(S.astype(np.float32).astype(np.int64), S)
    bad = np.nonzero(st["grad"].view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (strategy, B, bad.size, bad[:8], st["grad"][bad[:8]], want[bad[:8]])
    assert np.count_nonzero(want) > 500 or B < 31
    assert float(ref["loss"]) > 0 and abs(float(st["loss"][0]) - float(ref["loss"])) <= 4 * U * float(ref["loss"])
    assert int(st["t"][0]) == 1


# ------------------------------------------------------------------------------------------------ (2) against float64
_REFS = {}


def _dense(ring, net, strategy, B, form):
    """the float64 reference and the float32 yardstick of one dense case, computed once: the procedure of
    test_learner_gpu.py::test_gradient_and_loss_against_float64 up to the point where the kernel's output is read.  The
    deciding arg-max does not depend on the form, so neither do the samples taken out as near ties."""
    key = (net, strategy, B, form)
    if key not in _REFS:
        layers, target = _nets(net, ring)
        theta, theta_t = L.flatten(layers), L.flatten(target)
        gamma = 0.98
        idx = np.random.RandomState(B).randint(0, ring["size"], B).astype(np.int32)
        eff = L.effective(idx, ring)
        r64 = L.gradient(theta, theta_t, ring, eff, gamma, strategy, np.float64, form=form)
        r32 = L.gradient(theta, theta_t, ring, eff, gamma, strategy, np.float32, form=form)
        share = 0.0
        if r64["deciding"] is not None:
            E_f = float(np.max(np.abs(r32["deciding"].astype(np.float64) - r64["deciding"])))
            top = np.sort(r64["deciding"], axis=1)
            near = ((top[:, 2] - top[:, 1]) <= 8 * E_f) & ~r64["done"]
            share = near.sum() / float(B)
            print("%s/%s/%d: forward E %.3e, near-tie share %.4f %%" % (net, strategy, B, E_f, 100 * share))
            assert share <= GAP_CAP
            if near.any():                                   # taken out: idx = -1 in the run that is compared
                idx = idx.copy()
                idx[np.nonzero(eff >= 0)[0][near]] = -1
                eff = L.effective(idx, ring)
                r64 = L.gradient(theta, theta_t, ring, eff, gamma, strategy, np.float64, form=form)
                r32 = L.gradient(theta, theta_t, ring, eff, gamma, strategy, np.float32, form=form)
        assert r32["g"].dtype == np.float32 and r32["loss"].dtype == np.float32
        E_g = float(np.max(np.abs(r32["g"].astype(np.float64) - r64["g"])))
        E_l = abs(float(r32["loss"]) - float(r64["loss"]))
        _REFS[key] = dict(layers=layers, target=target, theta=theta, theta_t=theta_t, gamma=gamma, idx=idx, eff=eff, g64=r64["g"],
                          l64=float(r64["loss"]), n=r64["n"], E_g=E_g, E_l=E_l, share=share)
    return _REFS[key]


def _run(torch, dring, ref, strategy, B, form):
    lrn = _learner(torch, ref["layers"], ref["target"], gamma=ref["gamma"], strategy=strategy, loss=form)
    out = torch.zeros(B, dtype=torch.int32, device=DEV)
    lrn.update(dring, B, idx=_idx(torch, ref["idx"]), idx_out=out)
    st = _state(torch, lrn)
    assert np.array_equal(out.cpu().numpy(), ref["eff"]) and 0.9 * B < ref["n"] <= B
    return st


def _hold(tag, st, g64, l64, E_g, E_l):
    err = float(np.max(np.abs(st["grad"].astype(np.float64) - g64)))
    err_l = abs(float(st["loss"][0]) - l64)
    print("%s: max |grad - g64| %.3e = %.2f E_g (E_g %.3e, max |g| %.3e); |loss - l64| %.3e = %.2f E_l (E_l %.3e, loss %.4e)"
          % (tag, err, err / E_g, E_g, np.abs(g64).max(), err_l, err_l / E_l if E_l else np.inf, E_l, l64))
    assert err <= 4 * E_g, "max |grad - g64| %.3e > 4 E_g = %.3e" % (err, 4 * E_g)
    assert err_l <= 4 * E_l, "|loss - l64| %.3e > 4 E_l = %.3e" % (err_l, 4 * E_l)


@pytest.mark.parametrize("B", [64, 4096 + 17])
@pytest.mark.parametrize("net,strategy", CASES)
def test_reference_gradient_and_loss_against_float64(torch, net, strategy, B):
    """test_gradient_and_loss_against_float64 with loss="reference" on both sides: the eight cases at B = 64 and 4 113, the bar
    4 E_g / 4 E_l with E from the float32 numpy run of the reference form, near ties counted (<= 0.25 %) and taken out as
    there.  Measured on one MI355X, max |grad - g64| in units of E_g (the bound stays 4): B = 64: no_obs 0.97, with_obs 0.93,
    random1 0.61, random2 0.78, random3 0.72, random1/double 0.97, random1/fixed 0.78, random1/standard 0.92; B = 4 113:
    0.12 - 0.31.  Loss: 0.14 - 1.00 E_l.  Near-tie share at most 0.049 % (no_obs at 4 113), the form does not enter it."""
    ring, dring = _float_ring(torch)
    ref = _dense(ring, net, strategy, B, "reference")
    st = _run(torch, dring, ref, strategy, B, "reference")
    _hold("%s/%s/%d reference" % (net, strategy, B), st, ref["g64"], ref["l64"], ref["E_g"], ref["E_l"])


@pytest.mark.parametrize("form", L.FORMS)
@pytest.mark.parametrize("strategy", ["double_ref", "standard"])
@pytest.mark.parametrize("net", ["random1", "with_obs"])
def test_kernel_against_autograd_directly(torch, net, strategy, form):
    """the hand-derived model skipped: the kernel's gradient and loss against torch.autograd of the loss restated with the
    reference's array shapes (float64, CPU), both forms, B = 64; the bar is the same 4 E_g / 4 E_l.  Measured on one MI355X:
    "mse" 1.55, 3.06, 0.76, 0.81 E_g (the figures test_learner_gpu.py records against the model), "reference" 0.61, 0.92,
    0.93, 1.05 E_g; loss 0.08 - 1.09 E_l."""
    ring, dring = _float_ring(torch)
    ref = _dense(ring, net, strategy, 64, form)
    g, loss = A.gradient(ref["theta"], ref["theta_t"], ring, ref["eff"], ref["gamma"], strategy, executed=form == "reference")
    st = _run(torch, dring, ref, strategy, 64, form)
    _hold("%s/%s/64 %s against autograd" % (net, strategy, form), st, g, loss, ref["E_g"], ref["E_l"])


def test_reference_form_with_two_tiles_per_wavefront(torch):
    """B = 32 833, random1/double_ref as in test_launch_regimes_gpu.py: 257 partials of two wavefronts of two tiles, so the
    loss partial and delta of the reference form pass through the later-tile loop and every partial.  Measured on one
    MI355X: 0.22 E_g, loss 1.00 E_l (the float32 reference's own bits)."""
    B = 32833
    tiles, tpw, groups = L.launch_shape(B)
    assert tpw == 2 and groups == 257
    ring, dring = _float_ring(torch)
    ref = _dense(ring, "random1", "double_ref", B, "reference")
    st = _run(torch, dring, ref, "double_ref", B, "reference")
    _hold("random1/double_ref/%d reference" % B, st, ref["g64"], ref["l64"], ref["E_g"], ref["E_l"])


# ------------------------------------------------------------------------------------------------ (3) behaviour
def test_forms_differ_twins_agree_and_the_form_travels_with_the_state(torch):
    ring, dring = _float_ring(torch)
    layers, target = _nets("random2", ring)
    mse, ref, twin = (_learner(torch, layers, target, seed=3, loss=form) for form in ("mse", "reference", "reference"))
    for lrn in (mse, ref, twin):
        lrn.update(dring, 97)
        lrn.update(dring, 4096 + 17)
    a, b, c = (_state(torch, lrn) for lrn in (mse, ref, twin))
    assert _same(b, c) == []
    assert {"theta", "m", "v", "grad", "loss", "blob"} <= set(_same(a, b)) and "t" not in _same(a, b)
    g, g_ref = a["grad"].astype(np.float64), b["grad"].astype(np.float64)
    cos = float(g @ g_ref / np.sqrt((g @ g) * (g_ref @ g_ref)))
    assert cos < 0.999, cos                              # another direction, not another scale
    # the form is a hyper-parameter of the checkpoint; one written before the option existed loads as "mse"
    from aquaticgymenv_amd.learner import DQNLearner
    assert ref.state_dict()["hyper"]["loss"] == "reference" and mse.state_dict()["hyper"]["loss"] == "mse"
    fresh = _learner(torch, _nets("random3", ring)[0], seed=99)
    fresh.load_state_dict(ref.state_dict())
    for lrn in (ref, fresh):
        lrn.update(dring, 97)
    assert _same(_state(torch, ref), _state(torch, fresh)) == []
    old = mse.state_dict()
    del old["hyper"]["loss"]
    fresh.load_state_dict(old)
    for lrn in (mse, fresh):
        lrn.update(dring, 97)
    assert _same(_state(torch, mse), _state(torch, fresh)) == []
    with pytest.raises(ValueError):
        DQNLearner(mse.qnet, loss="huber")
    with pytest.raises(ValueError):
        fresh.load_state_dict(dict(old, hyper=dict(old["hyper"], loss="huber")))


def test_all_invalid_batch_changes_nothing_in_the_reference_form(torch):
    ring = L.int_ring(300, 257, 3, bad_ok=0.1)
    dead = np.nonzero(ring["ok"][:257] == 0)[0]
    idx = np.array([-1, 257, 299, 2 ** 31 - 1, -2 ** 31] + dead[:20].tolist(), dtype=np.int64)
    lrn = _learner(torch, L.int_layers(), L.int_layers(salt=1), loss="reference")
    rng = np.random.RandomState(0)
    _set(torch, lrn, m=rng.randn(L.PARAMS), v=rng.rand(L.PARAMS), t=[41], loss=[5.0])
    before = _state(torch, lrn)
    out = torch.zeros(idx.size, dtype=torch.int32, device=DEV)
    lrn.update(L.DeviceRing(torch, ring, DEV), idx.size, idx=_idx(torch, idx.astype(np.int32)), idx_out=out)
    after = _state(torch, lrn)
    assert _same(before, after, KEPT) == []
    assert float(after["loss"][0]) == 0.0 and bool((after["grad"] == 0).all()) and bool((out.cpu().numpy() == -1).all())


def test_captured_reference_updates_replay_like_eager_ones(torch):
    ring, dring = _float_ring(torch)
    layers, target = _nets("random1", ring)
    B = 4096 + 17
    eager, graphed = (_learner(torch, layers, target, seed=11, loss="reference") for _ in range(2))
    graphed._grow(B)                                         # the workspace grows outside of the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(3):
            graphed.update(dring, B)
    assert int(graphed.t[0]) == 0                            # captured, not run
    graph.replay()
    for _ in range(3):
        eager.update(dring, B)
    assert _same(_state(torch, eager), _state(torch, graphed)) == []
    assert int(eager.t[0]) == 3


def test_adam_step_from_the_reference_gradient(torch):
    """one update from t = 0 with the flag: Adam, the soft update and the re-pack from the kernel's own `grad`
    (test_learner_gpu.py::_check_step), and that gradient is the reference form's: the scale applied once"""
    ring, dring = _float_ring(torch)
    ref = _dense(ring, "random2", "double_ref", 64, "reference")
    lr, tau = 1e-3, 0.005
    lrn = _learner(torch, ref["layers"], ref["target"], gamma=ref["gamma"], lr=lr, tau=tau, loss="reference")
    before = _state(torch, lrn)
    lrn.update(dring, 64, idx=_idx(torch, ref["idx"]))
    after = _state(torch, lrn)
    _check_step(before, after, lr, tau)
    _hold("random2/double_ref/64 reference", after, ref["g64"], ref["l64"], ref["E_g"], ref["E_l"])


def test_an_unknown_flag_bit_is_rejected_before_any_launch(torch):
    from aquaticgymenv_amd import _learner_capi as capi
    ring, dring = _float_ring(torch)
    lrn = _learner(torch, *_nets("random1", ring))
    before = _state(torch, lrn)

    def call(strategy):
        need = lrn._grow(64)
        return capi.lib.aqualrn_update_f32(
            lrn.theta.data_ptr(), lrn.theta_target.data_ptr(), lrn.m.data_ptr(), lrn.v.data_ptr(), lrn.t.data_ptr(),
            dring.s.data_ptr(), dring.a.data_ptr(), dring.r.data_ptr(), dring.s2.data_ptr(), dring.d.data_ptr(), dring.ok.data_ptr(),
            dring.capacity, dring.size, None, 64, 1, strategy, 0.98, 0.005, 1e-3, 0.9, 0.999, 1e-7,
            lrn.qnet.blob.data_ptr(), lrn.target_blob.data_ptr(), lrn.perm.data_ptr(), lrn.qnet.blob.numel() // 4,
            lrn._workspace.data_ptr(), need, None, lrn.grad.data_ptr(), lrn.loss.data_ptr(), lrn._stream())

    assert capi.LOSS_REFERENCE == 16 and capi.LOSSES == {"mse": 0, "reference": 16}
    for strategy in (4, 8, 32, 64, 16 | 4, 16 | 8, 16 | 32, 16 << 1 | 1, 1 << 30, -1, -16, -(1 << 31)):
        assert call(strategy) == capi.E_INVALID, strategy
        assert capi.lib.aqualrn_last_error().decode()
    assert _same(before, _state(torch, lrn)) == []
    for strategy in (0, 3, 16, 16 | 3):
        assert call(strategy) == 0, strategy
    assert int(_state(torch, lrn)["t"][0]) == 4
