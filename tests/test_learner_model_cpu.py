"""CPU-only checks of the learner's MODEL: tests/_learner.py::gradient is a hand-derived backward pass and the only
reference the learner kernels have, so it is held here to torch.autograd of the loss restated with the reference's array
shapes (tests/_learner_autograd.py), in float64, in both forms:

  "mse"        L = 1/B sum_b (Q(s_b)[a_b] - y_b)^2                            the textbook loss (executed=False)
  "reference"  L = 1/(3B) sum_b sum_j (Q(s_b)[a_b] - T_bj)^2, T constant      what main/impl/dqn.py:243-247 executes: the
               [B,1] prediction broadcast against the [B,3] targets (executed=True)

The bound 1e-10 of max |g| (and of the loss) is a condition, not a measurement: float64 rounding over at most 325 x 64
terms is below 1e-11 of the sum of |terms| (measured: at most 3.5e-14), the smallest formula error -- a factor, a dropped
mask, a missing term -- is of order 1e-1.  No library is needed: nothing here imports aquaticgymenv_amd.
"""
import inspect

import numpy as np
import pytest

from tests import _learner as L
from tests import _learner_autograd as A

GAMMA = 0.98
BOUND = 1e-10
BATCHES = (1, 2, 64, 325)
NETS = ("random1", "random2", "random3", "glorot1")
_CACHE = {}


def _ring():
    if "ring" not in _CACHE:
        _CACHE["ring"] = L.float_ring(5000, 4800, 23)
    return _CACHE["ring"]


def _nets(net):
    """-> (theta, theta_target) float32"""
    if net not in _CACHE:
        ring = _ring()
        x32 = ring["s"][:, :ring["size"]].T.copy()
        seed = int(net[-1])
        if net.startswith("random"):
            pair = L.random_layers(seed, x32), L.random_layers(10 + seed, x32)
        else:
            pair = L.glorot_layers(seed), L.glorot_layers(10 + seed)
        _CACHE[net] = tuple(L.flatten(p) for p in pair)
    return _CACHE[net]


def _batch(B):
    """B slots of the ring; from 8 on, slots with ok == 0 among them (not samples)"""
    ring = _ring()
    rng = np.random.RandomState(B)
    live = np.nonzero(ring["ok"][:ring["size"]] != 0)[0]
    idx = rng.randint(0, ring["size"], B) if B >= 8 else live[rng.randint(0, live.size, B)]
    return L.effective(idx, ring)


def _autograd(net, strategy, B, executed):
    key = (net, strategy, B, executed)
    if key not in _CACHE:
        theta, theta_t = _nets(net)
        _CACHE[key] = A.gradient(theta, theta_t, _ring(), _batch(B), GAMMA, strategy, executed=executed)
    return _CACHE[key]


def _compare(model, net, strategy, B, form, executed):
    """`model`: L.gradient or a mutant of it -> (gradient error / max |g|, relative loss error), asserted against BOUND"""
    theta, theta_t = _nets(net)
    out = model(theta, theta_t, _ring(), _batch(B), GAMMA, strategy, np.float64, form=form)
    g, loss = _autograd(net, strategy, B, executed)
    assert out["n"] >= 1 and g.shape == out["g"].shape == (L.PARAMS,) and np.abs(g).max() > 0 and loss > 0
    err = float(np.max(np.abs(out["g"] - g)) / np.abs(g).max())
    err_l = abs(float(out["loss"]) - loss) / loss
    assert err <= BOUND, "%s/%s/%d %s: max |g - g_autograd| = %.3e max |g|" % (net, strategy, B, form, err)
    assert err_l <= BOUND, "%s/%s/%d %s: loss off by %.3e" % (net, strategy, B, form, err_l)
    return err, err_l


@pytest.mark.parametrize("strategy", L.STRATEGIES)
@pytest.mark.parametrize("B", BATCHES)
def test_mse_model_is_autograd_of_the_textbook_loss(B, strategy):
    worst = [_compare(L.gradient, net, strategy, B, "mse", False) for net in NETS]
    print("B %d %s: gradient %.1e of max |g|, loss %.1e" % (B, strategy, max(w[0] for w in worst), max(w[1] for w in worst)))


@pytest.mark.parametrize("strategy", L.STRATEGIES)
@pytest.mark.parametrize("B", BATCHES)
def test_reference_model_is_autograd_of_the_loss_as_executed(B, strategy):
    """the [B,1] - [B,3] broadcast and the mean over 3 B elements, differentiated as written"""
    worst = [_compare(L.gradient, net, strategy, B, "reference", True) for net in NETS]
    print("B %d %s: gradient %.1e of max |g|, loss %.1e" % (B, strategy, max(w[0] for w in worst), max(w[1] for w in worst)))


@pytest.mark.parametrize("strategy", L.STRATEGIES)
def test_the_two_forms_differ_in_direction(strategy):
    """otherwise the comparison above could pass with either model: at B = 64 the cosine between the two gradients is below
    0.99 in every case (measured: at most 0.983), in the model and in autograd alike"""
    for net in NETS:
        theta, theta_t = _nets(net)
        pair = [L.gradient(theta, theta_t, _ring(), _batch(64), GAMMA, strategy, np.float64, form=form)["g"] for form in L.FORMS]
        auto = [_autograd(net, strategy, 64, executed)[0] for executed in (False, True)]
        for g, g_ref in (pair, auto):
            cos = float(g @ g_ref / np.sqrt((g @ g) * (g_ref @ g_ref)))
            print("%s/%s: cosine %.3f, |g_ref| / |g| %.2f" % (net, strategy, cos, np.sqrt((g_ref @ g_ref) / (g @ g))))
            assert cos < 0.99


def test_one_sample_by_hand():
    """B = 1, from L.forward alone: g_ref = (2/3) (3 Q_a - y - sum_{j != a} Q_j) grad Q_a and g = 2 (Q_a - y) grad Q_a, with
    grad Q_a by central differences.  Q is affine in any single parameter between two kinks of a relu, so the difference
    quotient is exact up to rounding: |Q| 2^-52 / h with h = 1e-5, which is why the bound here is 1e-6 of max |g|."""
    ring, eff = _ring(), _batch(1)
    theta32, theta_t32 = _nets("random1")
    theta, theta_t = theta32.astype(np.float64), theta_t32.astype(np.float64)
    slot = int(eff[0])
    x, x2 = (ring[k][:, slot].astype(np.float64)[None, :] for k in ("s", "s2"))
    a, r = int(ring["a"][slot]), float(ring["r"][slot])
    ring = dict(ring, d=ring["d"].copy())
    ring["d"][slot] = 0                                               # not terminal: the bootstrap term takes part
    q = L.forward(theta, x)[2][0]
    y = r + GAMMA * L.forward(theta_t, x2)[2][0][int(np.argmax(q))]   # "double_ref"
    h = 1e-5
    grad_q = np.zeros(L.PARAMS)
    for p in range(L.PARAMS):
        up, down = theta.copy(), theta.copy()
        up[p] += h
        down[p] -= h
        grad_q[p] = (L.forward(up, x)[2][0, a] - L.forward(down, x)[2][0, a]) / (2 * h)
    rest = q.sum() - q[a]
    want = {"mse": 2.0 * (q[a] - y) * grad_q, "reference": (2.0 / 3.0) * (3.0 * q[a] - y - rest) * grad_q}
    want_loss = {"mse": (q[a] - y) ** 2, "reference": ((q[a] - y) ** 2 + sum((q[a] - q[j]) ** 2 for j in range(3) if j != a)) / 3.0}
    for form in L.FORMS:
        out = L.gradient(theta32, theta_t32, ring, eff, GAMMA, "double_ref", np.float64, form=form)
        assert np.abs(want[form]).max() > 0
        assert np.max(np.abs(out["g"] - want[form])) <= 1e-6 * np.abs(want[form]).max(), form
        assert abs(float(out["loss"]) - want_loss[form]) <= 1e-12 * want_loss[form], form


def _mutant(old, new):
    """a copy of the model with one piece of its text replaced"""
    src = inspect.getsource(L.gradient)
    assert src.count(old) == 1, old
    scope = dict(vars(L))
    exec(compile(src.replace(old, new), "<mutant of tests/_learner.py::gradient>", "exec"), scope)
    return scope["gradient"]


MUTANTS = {
    "scale 2/n": ("dtype(2.0 / (3 * n)), dtype(1.0 / (3 * n))", "dtype(2.0 / n), dtype(1.0 / (3 * n))"),
    "the other actions' Q dropped": ("- y - rest)", "- y)"),
    "the done mask dropped": ("np.where(done, dtype(0), dtype(gamma) * f)", "(dtype(gamma) * f)"),
    "the forms swapped": ('if form == "reference":', 'if form != "reference":'),
    "relu' of the wrong layer": ("(dq @ k2.T) * (h2 > 0)", "(dq @ k2.T) * (h1 > 0)"),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_the_comparison_rejects_a_wrong_model(name):
    """one wrong piece at a time in a copy of the model: the comparison with autograd must fail, for every network"""
    mutant = _mutant(*MUTANTS[name])
    eff = _batch(64)
    assert (_ring()["d"][eff[eff >= 0]] != 0).any() and (eff < 0).any()
    for net in NETS:
        _compare(L.gradient, net, "double_ref", 64, "reference", True)
        with pytest.raises(AssertionError):
            _compare(mutant, net, "double_ref", 64, "reference", True)
    if name != "the other actions' Q dropped" and name != "scale 2/n":       # these two touch the "reference" branch only
        with pytest.raises(AssertionError):
            _compare(mutant, "random1", "standard", 64, "mse", False)


def test_adam64_against_torch_adam_without_eps():
    """L.adam64 (the formulas test_learner_gpu.py::_check_step holds the apply kernel to) against torch.optim.Adam in
    float64 with eps = 0 in both: Keras's lr_t m / (sqrt(v) + eps) with lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) and torch's
    lr (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps) then coincide, which pins both moments and both bias corrections
    independently, three steps, to 1e-12 relative.  adam64 works from float32 state, so torch's state is set to the same
    rounded values before every step.  Where eps goes is NOT checked here (with eps = 0 it cannot be): that stays pinned by
    reading main/impl/dqn.py:313 against the Keras 2.3 source, lr_t m / (sqrt(v) + eps) with eps outside the correction."""
    import torch
    ring = _ring()
    theta32, theta_t32 = _nets("glorot1")
    grads = [L.gradient(theta32, theta_t32, ring, _batch(B), GAMMA, "double_ref", np.float64)["g"].astype(np.float32) for B in (64, 325, 2)]
    on = np.nonzero(grads[0] != 0)[0]                      # with eps = 0 an entry that never saw a gradient is 0 / 0
    assert on.size > 1000
    lr = 1e-3
    f32 = lambda z: np.asarray(z, dtype=np.float32)
    theta, m, v = f32(theta32[on]), f32(np.zeros(on.size)), f32(np.zeros(on.size))
    p = torch.nn.Parameter(torch.tensor(theta.astype(np.float64)))
    opt = torch.optim.Adam([p], lr=lr, betas=(L.BETA1, L.BETA2), eps=0.0)
    rel = lambda got, want: float(np.max(np.abs(got - want) / np.abs(want)))
    for t, g in enumerate(grads):
        g = g[on]
        th64, m64, v64, t1 = L.adam64(theta, theta, m, v, t, g, lr, 0.005, eps=0.0)
        assert t1 == t + 1
        if t > 0:
            with torch.no_grad():
                p.copy_(torch.tensor(theta.astype(np.float64)))
                opt.state[p]["exp_avg"].copy_(torch.tensor(m.astype(np.float64)))
                opt.state[p]["exp_avg_sq"].copy_(torch.tensor(v.astype(np.float64)))
        p.grad = torch.tensor(g.astype(np.float64))
        opt.step()
        assert int(opt.state[p]["step"]) == t1
        step64, step_t = th64 - theta.astype(np.float64), p.detach().numpy() - theta.astype(np.float64)
        # m is a sum of two terms of either sign: relative to the sum of |terms|, as any rounding bound of a sum is
        terms = L.BETA1 * np.abs(m.astype(np.float64)) + (1 - L.BETA1) * np.abs(g.astype(np.float64))
        errs = (float(np.max(np.abs(opt.state[p]["exp_avg"].numpy() - m64) / terms)), rel(opt.state[p]["exp_avg_sq"].numpy(), v64),
                rel(step_t, step64))
        print("t = %d: m %.1e, v %.1e, step %.1e relative" % ((t1,) + errs))
        assert max(errs[:2]) <= 1e-12
        # the new parameter to 1e-12 of the step size lr (a step near a zero of m is small: no relative bound on it);
        # rounding is 2^-53 |theta| = 4e-17 here
        assert np.max(np.abs(p.detach().numpy() - th64)) <= 1e-12 * lr
        theta, m, v = f32(th64), f32(m64), f32(v64)


# ------------------------------------------------------------------------------------------------ where Adam's eps goes
ADAM_STEPS = (1, 2, 1000)
ADAM_ROOTS = (0.0, 1e-9, 1e-7, 1e-5, 1e-1)        # sqrt(v) after the step: 0, far below eps = 1e-7, at it, above, far above


def _adam_case(t):
    """float32 state whose sqrt(v') after step t is ADAM_ROOTS x eight m of both signs x a gradient that is zero (v' = beta2 v
    exactly on the grid) or not -> (theta, m, v, g) float32 [80]"""
    rng = np.random.RandomState(t)
    roots, ms, gs = np.meshgrid(np.array(ADAM_ROOTS), np.array([1e-9, -1e-6, 1e-3, -1e-1, -1e-9, 1e-6, -1e-3, 1e-1]), np.array([0.0, 1.0]), indexing="ij")
    v = (roots.reshape(-1) ** 2 / L.BETA2).astype(np.float32)
    g = (gs.reshape(-1) * rng.uniform(-1, 1, v.size) * roots.reshape(-1)).astype(np.float32)      # |g| <= sqrt(v): the root stays of its order
    return rng.uniform(-1, 1, v.size).astype(np.float32), ms.reshape(-1).astype(np.float32), v, g


def _adam_compare(model, t, eps=L.EPS, lr=1e-3):
    """`model`: L.adam64 or a mutant of it, one step to t, against torch.optim.Adam in float64 with eps / sqrt(1 - beta2^t)"""
    import torch
    theta, m, v, g = _adam_case(t)
    with np.errstate(divide="ignore", invalid="ignore"):
        th64, m64, v64, t1 = model(theta, theta, m, v, t - 1, g, lr, 0.005, eps=eps)
    assert t1 == t
    p = torch.nn.Parameter(torch.tensor(theta.astype(np.float64)))
    opt = torch.optim.Adam([p], lr=lr, betas=(L.BETA1, L.BETA2), eps=eps / np.sqrt(1.0 - L.BETA2 ** t))
    p.grad = torch.zeros_like(p)
    opt.step()                                             # creates the state; everything it touched is overwritten below
    state = opt.state[p]
    with torch.no_grad():
        p.copy_(torch.tensor(theta.astype(np.float64)))
        state["exp_avg"].copy_(torch.tensor(m.astype(np.float64)))
        state["exp_avg_sq"].copy_(torch.tensor(v.astype(np.float64)))
        if torch.is_tensor(state["step"]):
            state["step"].fill_(t - 1)
        else:
            state["step"] = t - 1
    p.grad = torch.tensor(g.astype(np.float64))
    opt.step()
    assert int(state["step"]) == t
    got, theta64 = p.detach().numpy(), theta.astype(np.float64)
    step_t = got - theta64
    assert np.isfinite(step_t).all() and (step_t != 0).all()
    root = np.sqrt(state["exp_avg_sq"].numpy())
    assert (root == 0).sum() >= 8 and ((root > 0) & (root < 0.1 * eps)).sum() >= 8 and (root > 100 * eps).sum() >= 16
    # float64 rounding: a dozen operations on the step, one on theta -- 1e-12 of the step is a condition, as BOUND is
    err = np.abs(th64 - got)
    bar = 1e-12 * np.abs(step_t) + 2.0 ** -52 * np.abs(theta64)
    assert bool((err <= bar).all()), "t = %d: worst %.3e of the step" % (t, float(np.nanmax(err / np.abs(step_t))))
    assert np.max(np.abs(state["exp_avg"].numpy() - m64)) <= 1e-15 and np.max(np.abs(state["exp_avg_sq"].numpy() - v64) / np.maximum(v64, 1e-300)) <= 1e-12
    return float(np.max(err / np.abs(step_t)))


@pytest.mark.parametrize("t", ADAM_STEPS)
def test_adam64_puts_eps_where_keras_puts_it(t):
    """Keras 2.3 (main/impl/dqn.py:313):  theta -= lr_t m / (sqrt(v) + e),  lr_t = lr sqrt(1 - b2^t) / (1 - b1^t).
    torch.optim.Adam:                    theta -= lr / (1 - b1^t)  m / (sqrt(v) / sqrt(1 - b2^t) + eps).
    Multiply torch's numerator and denominator by sqrt(1 - b2^t):
                                         theta -= lr_t m / (sqrt(v) + eps sqrt(1 - b2^t)),
    so one Keras step with epsilon e at step t IS one torch step with eps = e / sqrt(1 - b2^t): an implementation that
    shares no code with L.adam64 and pins where eps goes -- added to the root, outside the bias correction -- and its
    value, on parameters whose sqrt(v) runs from 0 through e to far above it, where e decides the step."""
    print("t = %d: worst |theta_adam64 - theta_torch| = %.1e of the step" % (t, _adam_compare(L.adam64, t)))


def _adam_mutant(old, new):
    src = inspect.getsource(L.adam64)
    assert src.count(old) == 1, old
    scope = dict(vars(L))
    exec(compile(src.replace(old, new), "<mutant of tests/_learner.py::adam64>", "exec"), scope)
    return scope["adam64"]


ADAM_MUTANTS = {
    "eps dropped": ("(np.sqrt(v2) + eps)", "(np.sqrt(v2) + 0.0)"),
    "eps inside the root": ("(np.sqrt(v2) + eps)", "np.sqrt(v2 + eps)"),
    "eps 1e-8": ("(np.sqrt(v2) + eps)", "(np.sqrt(v2) + 1e-8)"),
}


@pytest.mark.parametrize("t", ADAM_STEPS)
@pytest.mark.parametrize("name", sorted(ADAM_MUTANTS))
def test_the_adam_comparison_rejects_a_misplaced_eps(name, t):
    with pytest.raises(AssertionError):
        _adam_compare(_adam_mutant(*ADAM_MUTANTS[name]), t)
