"""What the fast acting path's tests share (tests/test_fastpol_cpu.py, tests/test_fastpol_gpu.py): the numpy model of the
scheme (csrc/aqua_fastpol.h), the float64 reference, the contract, the networks and inputs of the contract tests, the
numpy reading of a fast blob through aquafast_map and the lane maps, and the exact dyadic network.

The scheme.  split(v): c = clamp(v, +-65504); hi = f16(c), round to nearest even; lo = f16((c - float(hi)) * 2^11).  For
unit u of layers 1 and 2: acc_hi = bias + sum W_hi X_hi, acc_lo = sum (W_hi X_lo + W_lo X_hi), both accumulated in
np.float32; unit = relu(fmaf(acc_lo, 2^-11, acc_hi)).  Layer 3 in float32 from float32 weights.
"""
import os

import numpy as np

from tests._golden import GOLDEN

CLAMP = np.float32(65504.0)
SCALE = np.float32(2048.0)
GAP_CAP = 0.0025
NETS = ("no_obs", "with_obs", "random1", "random2", "random3")
SIZES = (4099, 65536)
TILE = 32
F16_MIN_NORMAL = 2.0 ** -14

# the fast blob in 16-bit elements (csrc/aqua_fastpol.hip restates nothing else to a caller than aquafast_map())
FRAG = 64 * 8
F_W1, F_W2, F_LDS = 0, 4 * FRAG, 20 * FRAG
FAST_ELEMS = F_LDS + 2 * 324
PART_HI, PART_LO, PART_BITS0, PART_BITS1 = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------ networks and inputs
def fixture_layers(tag):
    z = np.load(os.path.join(GOLDEN, "dqn_policies.npz"))
    return [(z["%s_kernel%d" % (tag, i)], z["%s_bias%d" % (tag, i)]) for i in range(3)]


_INPUTS = {}


def inputs(n):
    """the first n rows of RandomState(3).uniform(0, 1, (262144, 5)) as float32: made once, never written"""
    if "x" not in _INPUTS:
        x = np.random.RandomState(3).uniform(0, 1, (262144, 5)).astype(np.float32)
        x.setflags(write=False)
        _INPUTS["x"] = x
    return _INPUTS["x"][:n]


def evaluate(layers, x32, dtype):
    x = x32.astype(dtype)
    for li, (k, b) in enumerate(layers):
        x = x @ k.astype(dtype) + b.astype(dtype)
        if li < 2:
            x = np.maximum(x, 0)
    return x


def random_layers(seed, x32):
    """tests/test_qpolicy_gpu.py::_random_layers: N(0, 1) weights, biases of both signs; the last bias is minus each Q
    column's batch mean so that no action wins nearly everywhere"""
    rng = np.random.RandomState(seed)
    layers = [(rng.randn(a, b).astype(np.float32), rng.randn(b).astype(np.float32)) for a, b in ((5, 64), (64, 64), (64, 3))]
    assert all((b > 0).any() and (b < 0).any() for _, b in layers[:2])
    layers[2] = (layers[2][0], np.zeros(3, dtype=np.float32))
    q = evaluate(layers, x32, np.float64)
    layers[2] = (layers[2][0], (-q.mean(axis=0)).astype(np.float32))
    return layers


def network(net, x32):
    """the layers of one of NETS on the batch x32; a random network's winner share is asserted here"""
    if not net.startswith("random"):
        return fixture_layers(net)
    layers = random_layers(int(net[-1]), x32)
    wins = np.bincount(np.argmax(evaluate(layers, x32, np.float64), axis=1), minlength=3) / float(x32.shape[0])
    assert wins.min() >= 0.10, wins
    return layers


# ------------------------------------------------------------------------------------------------ the model
def _flush(h):
    """f16 subnormals to zero (a control, not the scheme)"""
    h = h.copy()
    h[np.abs(h.astype(np.float64)) < F16_MIN_NORMAL] = 0
    return h


def split(v, scaled=True, flush=False):
    """float32 array -> (hi, lo) float16 arrays"""
    c = np.clip(np.asarray(v, dtype=np.float32), -CLAMP, CLAMP)
    assert c.dtype == np.float32
    hi = c.astype(np.float16)
    rest = c - hi.astype(np.float32)
    lo = ((rest * SCALE) if scaled else rest).astype(np.float16)
    if flush:
        hi, lo = _flush(hi), _flush(lo)
    nan = np.isnan(c)
    if nan.any():                                         # a NaN weight: both parts the quiet f16 NaN, whatever its sign or payload
        hi, lo = hi.copy(), lo.copy()
        hi.view(np.uint16)[nan] = 0x7E00
        lo.view(np.uint16)[nan] = 0x7E00
    return hi, lo


def _fma(a, b, c):
    """fmaf on float32 arrays whose product is exact in float64 (b is a power of two)"""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)


def hidden(w_hi, w_lo, bias, x32, scheme="scaled"):
    """one hidden layer of the model: w_hi / w_lo float16 [in][out], bias float32 [out], x32 float32 [N][in] (split here)
    -> float32 [N][out].  scheme: "scaled" (the scheme), "flushed" (no 2^11, f16 subnormals flushed), "onepass" (hi only)"""
    x_hi, x_lo = split(x32, scaled=scheme == "scaled", flush=scheme == "flushed")
    wh, wl = w_hi.astype(np.float32), w_lo.astype(np.float32)
    xh, xl = x_hi.astype(np.float32), x_lo.astype(np.float32)
    n = x32.shape[0]
    acc_hi = np.repeat(bias.astype(np.float32)[None], n, axis=0)
    acc_lo = np.zeros_like(acc_hi)
    for k in range(wh.shape[0]):                          # products of two f16 are exact in float32; the sums round
        acc_hi = acc_hi + xh[:, k:k + 1] * wh[k][None]
        if scheme != "onepass":
            acc_lo = acc_lo + xl[:, k:k + 1] * wh[k][None]
            acc_lo = acc_lo + xh[:, k:k + 1] * wl[k][None]
    assert acc_hi.dtype == acc_lo.dtype == np.float32
    unit = _fma(acc_lo, 2.0 ** -11, acc_hi) if scheme == "scaled" else acc_hi + acc_lo
    return np.maximum(unit, np.float32(0))


# layer 3 as the kernel orders it: lane half h holds units unit_of(M, r, h), one chain per half, the first from the bias
def unit_of(M, r, h):
    return 32 * M + (r & 3) + 8 * (r >> 2) + 4 * h


HALF_UNITS = [[unit_of(M, r, h) for M in range(2) for r in range(16)] for h in range(2)]


def output(k2, b2, h2):
    """float32 [N][64] -> float32 [N][3]: two 32-term fused chains (one per lane half) added once"""
    k2, b2 = k2.astype(np.float32), b2.astype(np.float32)
    p = [np.repeat(b2[None], h2.shape[0], axis=0), np.zeros((h2.shape[0], 3), dtype=np.float32)]
    for h in range(2):
        for u in HALF_UNITS[h]:
            p[h] = (k2[u][None].astype(np.float64) * h2[:, u:u + 1].astype(np.float64) + p[h].astype(np.float64)).astype(np.float32)
    return p[0] + p[1]


def model(layers, x32, scheme="scaled", parts=None):
    """the scheme's evaluation of the network on x32 float32 [N][5] -> float32 [N][3].  parts: None (the weights are
    split here) or [(w_hi, w_lo)] * 2 float16, as read back from a fast blob"""
    (k0, b0), (k1, b1), (k2, b2) = layers
    if parts is None:
        parts = [split(k, scaled=scheme == "scaled", flush=scheme == "flushed") for k in (k0, k1)]
    h1 = hidden(parts[0][0], parts[0][1], b0, np.asarray(x32, dtype=np.float32), scheme)
    h2 = hidden(parts[1][0], parts[1][1], b1, h1, scheme)
    return output(k2, b2, h2)


def reference(layers, x32):
    """-> (q64 [N][3], E of numpy's float32 evaluation, E_s of the scheme's model, the model's q)"""
    q64 = evaluate(layers, x32, np.float64)
    q32 = evaluate(layers, x32, np.float32)
    assert q32.dtype == np.float32
    qm = model(layers, x32)
    assert qm.dtype == np.float32
    E = float(np.max(np.abs(q32.astype(np.float64) - q64)))
    E_s = float(np.max(np.abs(qm.astype(np.float64) - q64)))
    return q64, E, E_s, qm


def near_tie_share(q64, E_s):
    top = np.sort(q64, axis=1)
    close = (top[:, 2] - top[:, 1]) <= 8 * E_s
    return close, float(close.mean())


def check_contract(q64, E_s, q_kernel, action, what):
    """The numerics of the issue, in its order.  q_kernel float32 [3][N], action uint8 [N]"""
    n = q64.shape[0]
    close, share = near_tie_share(q64, E_s)
    print("%s: N %d  E_s %.3e  near-tie share %.4f %%" % (what, n, E_s, 100 * share))
    assert share <= GAP_CAP, "%s: %.4f %% of the batch lies within 8 E_s of a tie" % (what, 100 * share)
    # -- only now the kernel's output
    err = float(np.max(np.abs(q_kernel.T.astype(np.float64) - q64)))
    print("%s: max |q_kernel - q64| %.3e = %.2f E_s" % (what, err, err / E_s))
    assert err <= 4 * E_s, "%s: max |q - q64| %.3e > 4 E_s = %.3e" % (what, err, 4 * E_s)
    want = np.argmax(q64, axis=1)
    assert np.array_equal(action[~close], want[~close]), what
    assert bool((action <= 2).all())
    picked = q64[np.arange(n), action.astype(np.int64)]
    assert bool((picked >= q64.max(axis=1) - 8 * E_s).all()), what
    return err, share


# ------------------------------------------------------------------------------------------------ a fast blob, read in numpy
def counting_layers():
    """the parameters numbered 1 .. 4739 in canonical order (k0, b0, k1, b1, k2, b2): every value distinct and exact"""
    out, at = [], 1
    for a, b in ((5, 64), (64, 64), (64, 3)):
        out.append((np.arange(at, at + a * b, dtype=np.float32).reshape(a, b), np.arange(at + a * b, at + a * b + b, dtype=np.float32)))
        at += a * b + b
    return out


def expected_ids():
    """int64 [FAST_ELEMS]: for every 16-bit element of a fast blob, the number (counting_layers()) of the parameter the LANE
    MAPS of the kernel put there, or 0.  Stated from the MFMA's operand layout, not from the library: lane l (row = l & 31,
    h = l >> 5) holds A[row][k = 8 h + e] in element e; layer 1's element e < 3 of half h is input 2 e + h; layer 2's k-step
    s, element e of half h is unit 16 s + 8 (e >> 2) + 4 h + (e & 3)."""
    (k0, _), (k1, _), _ = counting_layers()
    ids = np.zeros(FAST_ELEMS, dtype=np.int64)
    for lane in range(64):
        h, row = lane >> 5, lane & 31
        for part in range(2):
            for e in range(8):
                for M in range(2):
                    k = 2 * e + h
                    if e < 3 and k < 5:
                        ids[F_W1 + ((M * 2 + part) * 64 + lane) * 8 + e] = int(k0[k][32 * M + row])
                    for s in range(4):
                        u = 16 * s + 8 * (e >> 2) + 4 * h + (e & 3)
                        ids[F_W2 + (((M * 4 + s) * 2 + part) * 64 + lane) * 8 + e] = int(k1[u][32 * M + row])
    return ids


def read_fast_blob(fast, fmap, id_blob):
    """fast: uint8 fast blob; fmap: aquafast_map(); id_blob: the float32 blob of counting_layers() (float index -> number).
    -> ([(w_hi, w_lo)] * 2 float16 in canonical shape, the float32 values of the copied parameters by number {id: value},
    counts {(number, part): occurrences})"""
    h = np.ascontiguousarray(fast).view(np.uint16)
    assert h.size == fmap.size == FAST_ELEMS
    flat = {PART_HI: np.zeros(4740, dtype=np.float16), PART_LO: np.zeros(4740, dtype=np.float16)}
    bits = {PART_BITS0: np.zeros(4740, dtype=np.uint32), PART_BITS1: np.zeros(4740, dtype=np.uint32)}
    counts = {}
    for e in np.nonzero(fmap >= 0)[0]:
        m = int(fmap[e])
        number, part = int(id_blob[m >> 2]), m & 3
        assert number >= 1, "the map names a padding float of the float32 blob"
        counts[(number, part)] = counts.get((number, part), 0) + 1
        if part in flat:
            flat[part][number] = h[e:e + 1].view(np.float16)[0]
        else:
            bits[part][number] = h[e]
    words = (bits[PART_BITS0] | (bits[PART_BITS1] << 16)).astype(np.uint32).view(np.float32)
    parts = [(flat[PART_HI][1:321].reshape(5, 64), flat[PART_LO][1:321].reshape(5, 64)),
             (flat[PART_HI][385:385 + 4096].reshape(64, 64), flat[PART_LO][385:385 + 4096].reshape(64, 64))]
    return parts, words, counts


# ------------------------------------------------------------------------------------------------ the exact network
DELTA = 2.0 ** -12                    # the lo part of every hidden activation of layer 1, and of every weight (times a sign)
LAMBDA1 = np.array([1, -1, 1, -2, 1], dtype=np.float64)        # signs and sizes of layer 1's weight lo parts: they sum to 0


def exact_layers(variant="plain"):
    """Dyadic-rational weights whose lo parts are non-zero at every position of every k-step, built so that the lo * lo
    products the scheme drops cancel exactly:
      layer 1  W[k][u] = a[k][u] + LAMBDA1[k] 2^-12 with integers a >= 2 and sum LAMBDA1 = 0; the inputs are
               x[k] = m[k] + 2^-11 with integers m and sum LAMBDA1[k] m[k] = 0 (exact_inputs), so every hidden unit of layer 1
               is an integer >= 1 plus, through its bias, the constant DELTA: its lo part is DELTA for every unit and world;
      layer 2  W[u][v] = a'[u][v] + sign[u][v] 2^-12 with sum_u sign[u][v] = 0, so sum_u W_lo[u][v] DELTA = 0.
    The layer-2 matrix is not symmetric.  variant: as the tie variants of tests/test_qpolicy_gpu.py."""
    k5, u64, v64, c3 = np.arange(5)[:, None], np.arange(64)[None, :], np.arange(64)[None, :], np.arange(3)[None, :]
    a0 = 2 + (k5 * (u64 % 7 + 1) + u64 // 5) % 2
    k0 = a0 + LAMBDA1[:, None] * 2.0 ** -12
    # the bias takes the fraction 2^-11 sum_k a0[k][u] away and leaves DELTA
    b0 = ((u64[0] * 3) % 4 - 30).astype(np.float64) - 2.0 ** -11 * a0.sum(axis=0) + DELTA
    u = np.arange(64)[:, None]
    a1 = ((3 * u + 7 * v64 + (u // 9) * (v64 % 3)) % 5 - 2).astype(np.float64)
    a1[a1 == 0] = 1 - 2 * ((u + v64) % 2)[a1 == 0]
    sign = (1 - 2 * ((u + v64 // 3) % 2)).astype(np.float64)
    k1 = a1 + sign * 2.0 ** -12
    assert not np.array_equal(k1, k1.T) and np.abs(sign.sum(axis=0)).max() == 0
    # layer 2's bias centres every unit on the middle input m = 5, so that its ReLU cuts some worlds and passes others
    middle = 5.0 * a0.sum(axis=0) + np.round(b0)
    b1 = ((np.arange(64) * 5 + 1) % 7 - 3).astype(np.float64) - middle @ a1
    k2 = np.array([1, -1, 2, -2, 1, -1], dtype=np.float64)[(u * (c3 + 1) + (u // 7) * (c3 + 2) + c3) % 6]
    b2 = np.array([2, -3, 1], dtype=np.float64)
    if variant == "tie01":
        k2[:, 1], b2[1] = k2[:, 0], b2[0]
    elif variant == "tie12":
        k2[:, 2], b2[2] = k2[:, 1], b2[1]
    elif variant == "tie012":
        k2[:, 1], k2[:, 2], b2[1], b2[2] = k2[:, 0], k2[:, 0], b2[0], b2[0]
    layers = [(k0, b0), (k1, b1), (k2, b2)]
    out = [(k.astype(np.float32), b.astype(np.float32)) for k, b in layers]
    for (k, b), (k32, b32) in zip(layers, out):
        assert np.array_equal(k32.astype(np.float64), k) and np.array_equal(b32.astype(np.float64), b)
    return out


def exact_inputs(n, seed=0):
    """float32 [n][5]: x[k] = m[k] + 2^-11, m integers in 4 .. 7 with sum LAMBDA1[k] m[k] = 0"""
    grid = np.array(np.meshgrid(*[np.arange(4, 8)] * 5, indexing="ij")).reshape(5, -1).T
    good = grid[(grid @ LAMBDA1) == 0]
    assert len(good) >= 50
    rng = np.random.RandomState(seed)
    m = good[rng.randint(0, len(good), size=n)]
    return (m + 2.0 ** -11).astype(np.float32)


def exact_reference(layers, x32):
    """The plain float64 evaluation of the exact network, with everything the construction promises asserted in float64:
    non-zero lo parts everywhere, nothing at the clamp, every partial sum within 24 bits.  -> q64 [N][3]"""
    (k0, b0), (k1, b1), (k2, b2) = [(k.astype(np.float64), b.astype(np.float64)) for k, b in layers]
    x = x32.astype(np.float64)

    def lo_nonzero(v32):
        hi, lo = split(v32)
        assert bool((lo.astype(np.float64) != 0).all()) and bool((np.abs(lo.astype(np.float64)) >= F16_MIN_NORMAL).all())
        assert bool((hi.astype(np.float64) != 0).all())
        # hi + lo 2^-11 is the value: the split loses nothing
        assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64) * 2.0 ** -11, v32.astype(np.float64))
        return hi.astype(np.float64), lo.astype(np.float64)

    def fits24(v, what):
        v = np.asarray(v, dtype=np.float64)
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v), what
        assert float(np.abs(v).max()) < 65504.0, what

    h = x
    for li, (k, b) in enumerate(((k0, b0), (k1, b1))):
        w_hi, w_lo = lo_nonzero(k.astype(np.float32))
        x_hi, x_lo = lo_nonzero(h.astype(np.float32))
        # whatever the order of the sums: the sum of the magnitudes of the terms bounds every partial sum, and every term is a
        # multiple of the same power of two, so a bound below 2^24 of that unit means every partial sum is exact
        hi_terms = np.abs(x_hi) @ np.abs(w_hi) + np.abs(b)
        unit_hi = 2.0 ** -12 if li == 0 else 1.0              # layer 1's bias carries the fraction; layer 2 sums integers
        assert np.array_equal(np.round(b / unit_hi), b / unit_hi) and float(hi_terms.max()) / unit_hi < 2 ** 24
        lo_terms = np.abs(x_lo) @ np.abs(w_hi) + np.abs(x_hi) @ np.abs(w_lo)
        assert float(lo_terms.max()) / 0.5 < 2 ** 24
        acc_hi = x_hi @ w_hi + b
        acc_lo = x_lo @ w_hi + x_hi @ w_lo
        fits24(acc_hi, "acc_hi of layer %d" % (li + 1))
        fits24(acc_lo, "acc_lo of layer %d" % (li + 1))
        unit = acc_hi + acc_lo * 2.0 ** -11
        fits24(unit, "the units of layer %d" % (li + 1))
        # the dropped lo * lo products cancel: the scheme's value is the plain one
        plain = h @ k + b
        assert np.array_equal(unit, plain), "layer %d: the lo * lo products do not cancel" % (li + 1)
        h = np.maximum(plain, 0)
        if li == 0:
            assert float(plain.min()) >= 1.0                     # every activation of layer 1 has its lo part
    if x.shape[0] >= 1000:                                       # layer 2's ReLU is active somewhere, no unit is dead
        assert bool((h > 0).any(axis=0).all()) and bool((h == 0).any())
    # layer 3 in the kernel's order: every partial sum of the two chains, and their sum
    for half in range(2):
        p = np.repeat((b2 if half == 0 else 0 * b2)[None], x.shape[0], axis=0)
        for u in HALF_UNITS[half]:
            p = p + h[:, u:u + 1] * k2[u][None]
            fits24(p, "a partial sum of layer 3")
    q = h @ k2 + b2
    fits24(q, "q")
    return q
