"""The DQN update of include/aqua_learner.h restated in numpy, for tests/test_learner_*.py: the reference the kernels are
held to (float64), the yardstick (the same formulas in float32) and the exact integer form.

Parameters are the canonical vector k0 [5][64], b0 [64], k1 [64][64], b1 [64], k2 [64][3], b2 [3].  A `ring` here is a
dict of numpy arrays s [5][cap] f32, a [cap] u8, r [cap] f32, s2 [5][cap] f32, d [cap] u8, ok [cap] u8 and "size".
"""
import numpy as np

from tests import _placement as P

PARAMS = 4739
SHAPES = ((5, 64), (64, 64), (64, 3))
STRATEGIES = ("double_ref", "double", "fixed", "standard")
FORMS = ("mse", "reference")     # the loss: the textbook mean squared error / the broadcast main/impl/dqn.py:243-247 executes
STREAM = 6
BETA1, BETA2, EPS = 0.9, 0.999, 1e-7
TILE, WAVES, GMAX = 32, 2, 512     # samples per tile, wavefronts per workgroup, workgroups at most (csrc/aqua_learner.hip)


def launch_shape(B):
    """csrc/aqua_learner.hip's shape_of restated: -> (tiles, tiles_per_wave, groups).  Wavefront w of group g takes tiles
    (g WAVES + w) tiles_per_wave .. + tiles_per_wave - 1.  tests/test_launch_regimes_cpu.py pins GMAX through
    aqualrn_workspace_bytes."""
    tiles = (B + TILE - 1) // TILE
    tpw = max(1, (tiles + WAVES * GMAX - 1) // (WAVES * GMAX))
    return tiles, tpw, (tiles + WAVES * tpw - 1) // (WAVES * tpw)


def flatten(layers):
    return np.concatenate([np.concatenate([np.asarray(k).reshape(-1), np.asarray(b).reshape(-1)]) for k, b in layers])


def unflatten(theta):
    out, at = [], 0
    for i, o in SHAPES:
        k = theta[at:at + i * o].reshape(i, o)
        at += i * o
        out.append((k, theta[at:at + o]))
        at += o
    assert at == PARAMS == theta.shape[0]
    return out


def forward(theta, x):
    """x [B][5] -> (h1, h2 pre-activations [B][64], q [B][3]) in the dtype of theta and x"""
    (k0, b0), (k1, b1), (k2, b2) = unflatten(theta)
    h1 = x @ k0 + b0
    h2 = np.maximum(h1, 0) @ k1 + b1
    return h1, h2, np.maximum(h2, 0) @ k2 + b2


def effective(idx, ring):
    """the slot every sample uses: idx where 0 <= idx < size and ok[idx] != 0, else -1"""
    idx = np.asarray(idx, dtype=np.int64)
    inside = (idx >= 0) & (idx < ring["size"])
    ok = np.zeros(idx.shape, dtype=bool)
    ok[inside] = ring["ok"][idx[inside]] != 0
    return np.where(ok, idx, -1).astype(np.int32)


def drawn(seed, t_new, B, ring):
    """the device draw of update t_new: int32 [B], -1 after four rejected attempts"""
    size = int(ring["size"])
    out = np.full(B, -1, dtype=np.int64)
    for attempt in range(4):
        r0 = P.draw(seed, np.arange(B), t_new, STREAM, attempt)[0]
        cand = ((r0.astype(np.uint64) * np.uint64(size)) >> np.uint64(32)).astype(np.int64)
        take = (out < 0) & (cand < size)
        take[take] = ring["ok"][cand[take]] != 0
        out[take] = cand[take]
    return out.astype(np.int32)


def batch_of(ring, eff, dtype):
    """the valid samples of a minibatch: (x, a, r, x2, done)"""
    sel = eff[eff >= 0].astype(np.int64)
    return (ring["s"][:, sel].T.astype(dtype), ring["a"][sel].astype(np.int64), ring["r"][sel].astype(dtype),
            ring["s2"][:, sel].T.astype(dtype), ring["d"][sel] != 0)


def bootstrap(theta, theta_t, x, x2, strategy):
    """-> (f [B], deciding Q-values [B][3] or None: the ones whose arg-max picks the target's action)"""
    qt = forward(theta_t, x2)[2]
    n = np.arange(x.shape[0])
    if strategy == "double_ref":
        dec = forward(theta, x)[2]
        return qt[n, np.argmax(dec, axis=1)], dec
    if strategy == "double":
        dec = forward(theta, x2)[2]
        return qt[n, np.argmax(dec, axis=1)], dec
    if strategy == "fixed":
        return qt.max(axis=1), None
    assert strategy == "standard"
    return forward(theta, x2)[2].max(axis=1), None


def gradient(theta32, theta_t32, ring, eff, gamma, strategy, dtype, form="mse"):
    """loss and gradient of the valid samples `eff` (effective()'s output), every operation in `dtype`:
    -> dict(g [PARAMS], S (the unscaled sums), loss, n, delta, deciding)
    form "mse": L = 1/n sum_b (Q(s_b)[a_b] - y_b)^2, the textbook loss.  form "reference": what main/impl/dqn.py:243-247
    executes, the [B,1] prediction broadcast against the [B,3] targets T (T_bj = y_b for j = a_b, Q(s_b)[j] otherwise, held
    constant): L = 1/(3n) sum_b sum_j (Q(s_b)[a_b] - T_bj)^2, so dL/dQ(s_b)[a_b] = 2/(3n) (3 Q_a - y - sum_{j != a} Q_j).
    tests/_learner_autograd.py differentiates both without this derivation."""
    assert form in FORMS, form
    theta, theta_t = theta32.astype(dtype), theta_t32.astype(dtype)
    x, a, r, x2, done = batch_of(ring, eff, dtype)
    n = x.shape[0]
    if n == 0:
        z = np.zeros(PARAMS, dtype=dtype)
        return dict(g=z, S=z, loss=dtype(0), n=0, delta=np.zeros(0, dtype=dtype), deciding=None, done=done)
    f, deciding = bootstrap(theta, theta_t, x, x2, strategy)
    y = r + np.where(done, dtype(0), dtype(gamma) * f).astype(dtype)
    h1, h2, q = forward(theta, x)
    (k0, b0), (k1, b1), (k2, b2) = unflatten(theta)
    qa = q[np.arange(n), a]
    if form == "reference":
        taken = np.arange(3)[None, :] == a[:, None]
        rest = np.where(taken, dtype(0), q).sum(axis=1, dtype=dtype)
        delta = (dtype(3) * qa - y - rest).astype(dtype)
        sq = (qa[:, None] - np.where(taken, y[:, None], q)) ** 2
        scale, mean = dtype(2.0 / (3 * n)), dtype(1.0 / (3 * n))
    else:
        delta = (qa - y).astype(dtype)
        sq = delta * delta
        scale, mean = dtype(2.0 / n), dtype(1.0 / n)
    dq = np.zeros((n, 3), dtype=dtype)
    dq[np.arange(n), a] = delta
    dh2 = (dq @ k2.T) * (h2 > 0)
    dh1 = (dh2 @ k1.T) * (h1 > 0)
    S = flatten([(x.T @ dh1, dh1.sum(axis=0)), (np.maximum(h1, 0).T @ dh2, dh2.sum(axis=0)), (np.maximum(h2, 0).T @ dq, dq.sum(axis=0))])
    assert S.dtype == dtype and delta.dtype == dtype and sq.dtype == dtype
    g = S * scale
    loss = sq.sum(dtype=dtype) * mean
    return dict(g=g, S=S, loss=loss, n=n, delta=delta, deciding=deciding, done=done)


def abs_sums(theta_i, theta_t_i, ring, eff, strategy, form="mse"):
    """Integer networks and data: the largest sum of |terms| over every intermediate and every gradient element, in int64
    (an upper bound of every partial sum in any order), and the exact unscaled gradient sums S."""
    out = gradient(theta_i.astype(np.int64).astype(np.float64), theta_t_i.astype(np.float64), ring, eff, 1.0, strategy, np.float64, form)
    x, a, r, x2, done = batch_of(ring, eff, np.int64)
    n = x.shape[0]
    worst = 0
    for th, inp in ((theta_i, x), (theta_i, x2), (theta_t_i, x2)):
        (k0, b0), (k1, b1), (k2, b2) = unflatten(th.astype(np.int64))
        h1 = np.abs(inp) @ np.abs(k0) + np.abs(b0)
        h2 = h1 @ np.abs(k1) + np.abs(b1)
        q = h2 @ np.abs(k2) + np.abs(b2)
        worst = max(worst, int(h1.max()), int(h2.max()), int(q.max()))
        qmax = q
    (k0, b0), (k1, b1), (k2, b2) = unflatten(np.abs(theta_i.astype(np.int64)))
    h1, h2, q = forward(np.abs(theta_i.astype(np.int64)), np.abs(x))
    delta = q.max(axis=1) + np.abs(r) + qmax.max(axis=1)                 # |Q(s)[a]| + |r| + |f|, each bounded by its sum of |terms|
    if form == "reference":
        delta = delta + 2 * q.max(axis=1) + q.sum(axis=1)                # 3 |Q_a| + |r| + |f| + sum_j |Q_j|, bounded the same way
    dq = np.repeat(delta[:, None], 3, axis=1)
    dh2 = dq @ k2.T
    dh1 = dh2 @ k1.T
    sums = flatten([(np.abs(x).T @ dh1, dh1.sum(axis=0)), (h1.T @ dh2, dh2.sum(axis=0)), (h2.T @ dq, dq.sum(axis=0))])
    worst = max(worst, int(delta.max()), int(dh2.max()), int(dh1.max()), int(sums.max()))
    S = np.rint(out["S"]).astype(np.int64)
    assert np.array_equal(S.astype(np.float64), out["S"])
    return worst, S, out


def adam64(theta, theta_t, m, v, t, g, lr, tau, beta1=BETA1, beta2=BETA2, eps=EPS):
    """float64 formulas on the float32 state: -> (theta', theta_t', m', v', t + 1), all float64"""
    theta, theta_t, m, v, g = (np.asarray(z, dtype=np.float32).astype(np.float64) for z in (theta, theta_t, m, v, g))
    t = int(t) + 1
    lr_t = lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
    m2 = beta1 * m + (1.0 - beta1) * g
    v2 = beta2 * v + (1.0 - beta2) * g * g
    th = theta - lr_t * m2 / (np.sqrt(v2) + eps)
    return th, m2, v2, t


def soft64(theta_new32, theta_t32, tau):
    return tau * theta_new32.astype(np.float64) + (1.0 - tau) * theta_t32.astype(np.float64)


# ------------------------------------------------------------------------------------------------ inputs
def int_layers(variant="plain", salt=0):
    """banded integer networks: entries in {-1, 0, 1}, at most 8 non-zeros per row and column"""
    def band(rows, cols, width, step, mul):
        i, j = np.arange(rows)[:, None], np.arange(cols)[None, :]
        inside = ((j - step * i) % cols) < width
        return (inside * (((mul[0] * i + mul[1] * j + (i * j) // 5 + salt) % 3 != 0) * 2 - 1)).astype(np.float32)
    k0 = band(5, 64, 8, 13, (2, 1))
    k1 = band(64, 64, 8, 1, (1, 2))
    i, c = np.arange(64)[:, None], np.arange(3)[None, :]
    k2 = ((((3 * i + c) % 8) == 0) * ((i // 8 + c + salt) % 2 * 2 - 1)).astype(np.float32)
    b0 = np.array([1, 0, 1, -1], dtype=np.float32)[(np.arange(64) + salt) % 4]
    b1 = np.array([1, 1, -1, 0, 1], dtype=np.float32)[(np.arange(64) + 2 * salt) % 5]
    b2 = np.array([1, -1, 0], dtype=np.float32)
    if variant == "tie01":
        k2[:, 1], b2[1] = k2[:, 0], b2[0]
    elif variant == "tie012":
        k2[:, 1], k2[:, 2], b2[1], b2[2] = k2[:, 0], k2[:, 0], b2[0], b2[0]
    layers = [(k0, b0), (k1, b1), (k2, b2)]
    for k, _ in layers:
        assert (np.count_nonzero(k, axis=0) <= 8).all() and (np.count_nonzero(k, axis=1) <= 8).all()
    return layers


def int_ring(cap, size, seed, bad_ok=0.0):
    """observations in {0, 1}, integer rewards, every termination code; slots behind `size` hold values that would
    break any sum they entered"""
    rng = np.random.RandomState(seed)
    ring = dict(s=rng.randint(0, 2, (5, cap)).astype(np.float32), s2=rng.randint(0, 2, (5, cap)).astype(np.float32),
                a=rng.randint(0, 3, cap).astype(np.uint8), r=rng.randint(-3, 4, cap).astype(np.float32),
                d=(rng.randint(0, 4, cap) * (rng.rand(cap) < 0.4)).astype(np.uint8),
                ok=(rng.rand(cap) >= bad_ok).astype(np.uint8), size=size)
    for key in ("s", "s2"):
        ring[key][:, size:] = 3.0e30
    ring["r"][size:] = 3.0e30
    ring["ok"][size:] = 1
    return ring


VALID_MAX = 4096                   # samples other than -1 in a sparse batch: keeps every integer sum below 2^24


def wave_span(B, W, first, last=None):
    """the samples [lo, hi) of tiles `first` .. `last` (counted inside the wavefront) of wavefront W = group * WAVES + wave"""
    tpw = launch_shape(B)[1]
    last = first if last is None else last
    return min(B, TILE * (W * tpw + first)), min(B, TILE * (W * tpw + last + 1))


def sparse_indices(B, ring, cap, seed):
    """An index vector for a batch whose wavefronts take several tiles each, with at most VALID_MAX entries other than -1,
    placed by launch_shape(B): -> (idx int64 [B], plan).  plan names the wavefronts check_sparse() then looks at:
      full    wavefronts whose every sample is a live slot: both of the last group, and wavefront 0 of group 0 unless one
              wavefront alone is a quarter of VALID_MAX (then the last wavefront of the last group only)
      spread  wavefront 1: a few live samples in its tiles 0, 1 and tiles_per_wave - 1, nothing else
      late    wavefront 3: nothing in its first tile; its second holds the invalid kinds and the duplicate of
              tests/test_learner_gpu.py::_mixed_indices
      mid     both wavefronts of the middle group, every tile partly filled with any slot below size (ok == 0 among them)
    and 2 400 samples (1 000 where a wavefront has more than four tiles) are scattered over the whole batch."""
    tiles, tpw, groups = launch_shape(B)
    assert tpw >= 2 and groups >= 8, (B, tpw, groups)
    rng = np.random.RandomState(seed)
    size = int(ring["size"])
    live = np.nonzero(ring["ok"][:size] != 0)[0]
    dead = np.nonzero(ring["ok"][:size] == 0)[0]
    idx = np.full(B, -1, dtype=np.int64)
    at = rng.choice(B, 2400 if tpw <= 4 else 1000, replace=False)
    idx[at] = rng.randint(0, size, at.size)
    last = groups - 1
    full = [W for W in (WAVES * last, WAVES * last + 1) if wave_span(B, W, 0)[0] < B]
    full = full[-1:] if 4 * tpw * TILE >= VALID_MAX else [0] + full
    for W in full:
        lo, hi = wave_span(B, W, 0, tpw - 1)
        idx[lo:hi] = live[rng.randint(0, live.size, hi - lo)]
    for it in sorted({0, 1, tpw - 1}):
        lo, hi = wave_span(B, 1, it)
        idx[lo:hi] = -1
        idx[lo + rng.choice(hi - lo, 5, replace=False)] = live[rng.randint(0, live.size, 5)]
    lo, hi = wave_span(B, 3, 0)
    idx[lo:hi] = -1
    lo, hi = wave_span(B, 3, 1)
    tile = rng.randint(0, size, TILE).astype(np.int64)
    tile[0] = live[0]
    tile[1], tile[3], tile[4], tile[5], tile[6], tile[7] = -1, size, cap - 1, 2 ** 31 - 1, tile[0], dead[0]
    idx[lo:hi] = tile
    mid = groups // 2
    share = 0.5 if tpw <= 4 else 0.125
    for W in (WAVES * mid, WAVES * mid + 1):
        lo, hi = wave_span(B, W, 0, tpw - 1)
        idx[lo:hi] = np.where(rng.rand(hi - lo) < share, rng.randint(0, size, hi - lo), -1)
    return idx, dict(full=full, spread=1, late=3, mid=mid)


def check_sparse(B, idx, ring, cap, plan):
    """what sparse_indices() promises, asserted from launch_shape(B) and the vector alone -> effective(idx)"""
    tiles, tpw, groups = launch_shape(B)
    size = int(ring["size"])
    eff = effective(idx, ring)
    live = eff >= 0
    assert tpw >= 2, "B = %d no longer gives a wavefront a second tile" % B
    assert idx.shape == (B,) and int((idx != -1).sum()) <= VALID_MAX
    # a wavefront with every tile fully valid in the last group, and in group 0 where the budget allows both
    assert plan["full"] and plan["full"][-1] // WAVES == groups - 1
    assert 4 * tpw * TILE >= VALID_MAX or plan["full"][0] // WAVES == 0
    for W in plan["full"]:
        lo, hi = wave_span(B, W, 0, tpw - 1)
        assert hi > lo and live[lo:hi].all(), W
    # valid samples at tiles 0, 1 and tiles_per_wave - 1 of one wavefront
    for it in (0, 1, tpw - 1):
        lo, hi = wave_span(B, plan["spread"], it)
        assert 0 < live[lo:hi].sum() < TILE, it
    # the last tile, ragged unless B is a multiple of the tile
    lo = TILE * (tiles - 1)
    assert live[lo:B].any() and (B - lo < TILE) == (B % TILE != 0)
    # a wavefront whose first tile is empty and whose second is not; the second is the mixed tile
    lo, hi = wave_span(B, plan["late"], 0)
    assert hi - lo == TILE and not live[lo:hi].any()
    lo, hi = wave_span(B, plan["late"], 1)
    tile, tile_eff = idx[lo:hi], eff[lo:hi]
    assert hi - lo == TILE and live[lo:hi].any()
    assert {-1, size, cap - 1, 2 ** 31 - 1} <= set(tile.tolist())
    assert ((tile >= 0) & (tile < size) & (tile_eff < 0)).any()                       # a slot with ok == 0
    assert len(set(tile_eff[tile_eff >= 0].tolist())) < int((tile_eff >= 0).sum())    # a duplicate
    # the middle group: partly filled tiles, first and later ones, in both wavefronts
    for W in (WAVES * plan["mid"], WAVES * plan["mid"] + 1):
        touched = [bool(live[slice(*wave_span(B, W, it))].any()) for it in range(tpw)]
        assert sum(touched) > tpw // 2 and any(touched[1:]), W
        lo, hi = wave_span(B, W, 0, tpw - 1)
        assert not live[lo:hi].all()
    with_valid = np.unique((np.nonzero(live)[0] // TILE) // (WAVES * tpw))
    assert with_valid.size >= 3 and {0, 1, plan["mid"], groups - 1} <= set(with_valid.tolist())
    return eff


def float_ring(cap, size, seed, bad_ok=0.02):
    rng = np.random.RandomState(seed)
    ring = dict(s=rng.rand(5, cap).astype(np.float32), s2=rng.rand(5, cap).astype(np.float32),
                a=rng.randint(0, 3, cap).astype(np.uint8), r=rng.uniform(-1, 1, cap).astype(np.float32),
                d=(rng.randint(1, 4, cap) * (rng.rand(cap) < 0.1)).astype(np.uint8),
                ok=(rng.rand(cap) >= bad_ok).astype(np.uint8), size=size)
    return ring


def random_layers(seed, x32):
    """N(0, 1) weights, biases of both signs; the last bias is minus each Q column's batch mean (the recipe of
    tests/test_qpolicy_gpu.py::_random_layers, restated)"""
    rng = np.random.RandomState(seed)
    layers = [(rng.randn(a, b).astype(np.float32), rng.randn(b).astype(np.float32)) for a, b in SHAPES]
    layers[2] = (layers[2][0], np.zeros(3, dtype=np.float32))
    q = forward(flatten(layers).astype(np.float64), x32.astype(np.float64))[2]
    layers[2] = (layers[2][0], (-q.mean(axis=0)).astype(np.float32))
    return layers


def glorot_layers(seed):
    rng = np.random.RandomState(seed)
    out = []
    for i, o in SHAPES:
        lim = np.sqrt(6.0 / (i + o))
        out.append((rng.uniform(-lim, lim, (i, o)).astype(np.float32), np.zeros(o, dtype=np.float32)))
    return out


class DeviceRing(object):
    """what DQNLearner.update reads of a ReplayRing, from a numpy ring"""

    def __init__(self, torch, ring, device):
        for key in ("s", "s2", "r", "a", "d", "ok"):
            setattr(self, key, torch.as_tensor(np.ascontiguousarray(ring[key])).to(device))
        self.capacity = int(ring["a"].shape[0])
        self.size = int(ring["size"])
