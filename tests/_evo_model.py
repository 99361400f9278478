"""The rule of libaqua_evo.so (aquaticgymenv_amd/csrc/aqua_evo.h) as plain numpy, on the Philox of tests/_placement.py: the
noise, ask, the quantisation, the fitness, the key, the doubled mid-ranks, the rank differences, STEP and the bookkeeping.
Every result of the library is an exact integer or a stated chain of rounded float64 operations, so the comparison is bit for
bit and no tolerance exists.  Imports without a GPU.

Every function takes mutant=<name>: the same rule with one deliberate mistake (MUTANTS).  tests/test_evo_cpu.py shows that each
mutant changes a result on the fixtures below; tests/test_evo_gpu.py shows that the device disagrees with each."""
import numpy as np

from tests import _placement as PL

PARAMS = 4739
STREAM = 9
C = float.fromhex("0x1.3988e1412ed76p-17")
OFFSET = 524280
FIX = 1048576.0
CLAMP = 2048.0
HEADER = 8
NO_SLOT = (1 << 64) - 1
NEG_INF = 0xFF800000
MEAN_RETURN, SUCCESS_RATE = 0, 1
ADAM, SGD = 0, 1

MUTANTS = {
    "odd_sign": "the sign of the odd slot is not flipped",
    "g_not_advanced": "tell leaves the generation where it was",
    "swap_ji": "(j, i) swapped in the Philox counter",
    "seven_halves": "seven of the eight 16-bit halves are summed",
    "ties_by_index": "tied keys are ranked by index instead of sharing the mid-rank",
    "no_4": "D = H (2H - 1) sigma, without the 4",
    "t_not_incremented": "the bias corrections use t before the increment",
    "drop_unfinished": "worlds that have not ended are not counted",
    "empty_zero": "an empty segment scores 0 instead of -infinity",
    "no_clamp": "a return is quantised without the clamp to +-2048",
    "rank_centre": "the centre slot of an odd P is ranked with the others",
}


def _mutant(mutant):
    assert mutant is None or mutant in MUTANTS, mutant
    return mutant


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the noise
def noise(seed, g, j, i, mutant=None):
    """the integer numerator n of (generation g, pair j, parameter i); j and i broadcast -> int64"""
    _mutant(mutant)
    j, i = np.broadcast_arrays(np.asarray(j, dtype=np.uint64), np.asarray(i, dtype=np.uint64))
    if mutant == "swap_ji":
        j, i = i, j
    r = PL.draw(seed, (j << np.uint64(32)) | i, g, STREAM, 0)
    halves = []
    for w in r:
        halves += [w & np.uint64(0xFFFF), w >> np.uint64(16)]
    if mutant == "seven_halves":
        halves = halves[:7]
    s = np.zeros(j.shape, dtype=np.int64)
    for h in halves:
        s = s + h.astype(np.int64)
    return 2 * s - OFFSET


def epsilon(n):
    return np.asarray(n, dtype=np.int64).astype(np.float64) * C


# ------------------------------------------------------------------------------------------------ ask
def ask(theta, P, sigma, seed, g, slots=None, mutant=None):
    """the population's parameters in canonical order: float32 [len(slots)][PARAMS] (slots: default all P)"""
    _mutant(mutant)
    theta = np.ascontiguousarray(theta, dtype=np.float32)
    H = P // 2
    slots = list(range(P)) if slots is None else [int(s) for s in slots]
    out = np.empty((len(slots), PARAMS), dtype=np.float32)
    i = np.arange(PARAMS)
    c = theta.astype(np.float64)
    for row, slot in enumerate(slots):
        if slot >= 2 * H:
            out[row] = theta
            continue
        d = np.float64(sigma) * epsilon(noise(seed, g, slot // 2, i, mutant))
        x = c + d if (slot % 2 == 0 or mutant == "odd_sign") else c - d
        out[row] = x.astype(np.float32)
    return out


def scatter(rows, perm, blob_floats, before):
    """what ask leaves in the blob: float32 [P][blob_floats] `before` with row's parameters at perm (an entry outside
    [0, blob_floats) is skipped)"""
    out = np.array(before, dtype=np.float32, copy=True).reshape(len(rows), blob_floats)
    perm = np.asarray(perm, dtype=np.int64)
    ok = (perm >= 0) & (perm < blob_floats)
    out.view(np.uint32)[:, perm[ok]] = bits(rows)[:, ok]
    return out


# ------------------------------------------------------------------------------------------------ fitness
def quantise(ret, mutant=None):
    """float32 returns -> int64 in 2^-20 fixed point"""
    _mutant(mutant)
    ret = np.ascontiguousarray(ret, dtype=np.float32)
    u = ret.view(np.uint32)
    nan = ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)
    with np.errstate(invalid="ignore"):                           # (a signalling NaN in the cast; it is replaced below)
        x = np.where(nan, 0.0, ret.astype(np.float64))
    bound = CLAMP if mutant != "no_clamp" else 2.0 ** 42           # (the mutant still has to fit an int64)
    x = np.minimum(np.maximum(x, -bound), bound)
    return np.rint(x * FIX).astype(np.int64)


def fitness(log_ret, log_code, log_world, cursor, ret, finished, env_offset, N, seg, P, kind, mutant=None):
    """-> (fitness bits uint32 [P], episodes int64 [P], acc int64 [P][3])"""
    _mutant(mutant)
    C_ = len(log_ret)
    records = min(int(cursor), C_)
    limit = min(N, P * seg)
    acc = np.zeros((P, 3), dtype=np.int64)
    w = np.asarray(log_world[:records], dtype=np.int64) - env_offset
    keep = (w >= 0) & (w < limit)
    p = w[keep] // seg
    np.add.at(acc[:, 0], p, quantise(np.asarray(log_ret[:records])[keep], mutant))
    np.add.at(acc[:, 1], p, 1)
    np.add.at(acc[:, 2], p, (np.asarray(log_code[:records])[keep] == 3).astype(np.int64))
    if finished is not None and mutant != "drop_unfinished":
        open_ = np.nonzero(np.asarray(finished[:limit]) == 0)[0]
        np.add.at(acc[:, 0], open_ // seg, quantise(np.asarray(ret)[open_], mutant))
        np.add.at(acc[:, 1], open_ // seg, 1)
    out = np.full(P, 0 if mutant == "empty_zero" else NEG_INF, dtype=np.uint32)
    some = acc[:, 1] != 0
    n = acc[some, 1].astype(np.float64)
    if kind == MEAN_RETURN:
        f = (acc[some, 0].astype(np.float64) / FIX) / n
    else:
        f = acc[some, 2].astype(np.float64) / n
    out[some] = bits(f.astype(np.float32))
    return out, acc[:, 1].copy(), acc


# ------------------------------------------------------------------------------------------------ ranks
def key(u):
    u = np.asarray(u, dtype=np.uint32)
    return np.where((u >> np.uint32(31)) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def rank2(fitness_bits, P, mutant=None):
    """-> (rank2 int32 [2H], weights int32 [H], best slot)"""
    _mutant(mutant)
    H = P // 2
    n = P if mutant == "rank_centre" else 2 * H
    k = key(np.asarray(fitness_bits, dtype=np.uint32)[:n]).astype(np.int64)
    lt = (k[None, :] < k[:, None]).sum(axis=1)
    eq = (k[None, :] == k[:, None]).sum(axis=1)
    if mutant == "ties_by_index":
        before = (np.tril(k[None, :] == k[:, None], -1)).sum(axis=1)      # equal keys at a lower index
        r = 2 * (lt + before)
    else:
        r = 2 * lt + eq - 1
    r = r[:2 * H].astype(np.int32)
    w = (r[0::2] - r[1::2]).astype(np.int32)
    if H == 0:
        return r, w, NO_SLOT
    k = k[:2 * H]
    return r, w, int(np.nonzero(k == k.max())[0][0])


# ------------------------------------------------------------------------------------------------ STEP
def power(b, t):
    result, base, n = 1.0, float(b), int(t)
    while n:
        if n & 1:
            result = result * base
        base = base * base
        n >>= 1
    return result


def gsum(weights, seed, g, idx=None, mutant=None, chunk=64):
    """G of the parameters idx (default all): int64"""
    i = np.arange(PARAMS) if idx is None else np.asarray(idx)
    G = np.zeros(i.shape, dtype=np.int64)
    w = np.asarray(weights, dtype=np.int64)
    for j0 in range(0, len(w), chunk):
        j = np.arange(j0, min(j0 + chunk, len(w)))
        G += (w[j][:, None] * noise(seed, g, j[:, None], i[None, :], mutant)).sum(axis=0)
    return G


def step(G, H, theta, m, v, t, sigma, lr, beta1, beta2, eps, weight_decay, optimizer, mutant=None):
    """steps 2 .. 6 on arrays; t is the incremented counter -> (theta', m', v', grad, ghat)"""
    _mutant(mutant)
    f64 = np.float64
    theta, m, v = (np.ascontiguousarray(x, dtype=np.float32) for x in (theta, m, v))
    D = f64((1 if mutant == "no_4" else 4) * H * (2 * H - 1)) * f64(sigma)
    scale = f64(C) / D
    ghat = np.asarray(G, dtype=np.int64).astype(f64) * scale
    th = theta.astype(f64)
    grad = f64(weight_decay) * th - ghat
    if optimizer == SGD:
        return (th - f64(lr) * grad).astype(np.float32), m.copy(), v.copy(), grad, ghat
    if mutant == "t_not_incremented":
        t = t - 1
    md = f64(beta1) * m.astype(f64) + (f64(1.0) - f64(beta1)) * grad
    vd = f64(beta2) * v.astype(f64) + (f64(1.0) - f64(beta2)) * (grad * grad)
    c1 = f64(1.0) - f64(power(beta1, t))
    c2 = f64(1.0) - f64(power(beta2, t))
    with np.errstate(all="ignore"):
        move = (f64(lr) * (md / c1)) / (np.sqrt(vd / c2) + f64(eps))
    return (th - move).astype(np.float32), md.astype(np.float32), vd.astype(np.float32), grad, ghat


def fresh(theta, g=0):
    """the state a tell works on: theta, m, v float32 [PARAMS], t, header (a list of HEADER integers)"""
    header = [0] * HEADER
    header[0] = int(g)
    theta = np.array(theta, dtype=np.float32, copy=True)
    return {"theta": theta, "m": np.zeros_like(theta), "v": np.zeros_like(theta), "t": 0, "header": header}


def tell(state, fitness_bits, P, seed, sigma, lr, beta1, beta2, eps, weight_decay, optimizer, idx=None, mutant=None):
    """one tell on a copy of `state` -> the new state, with "rank2", "weights", "grad", "ghat" of this tell besides; idx:
    only these parameters are stepped (the others keep their values: for shapes whose full noise is too much for a test)"""
    _mutant(mutant)
    H = P // 2
    out = {k: (np.array(x, copy=True) if isinstance(x, np.ndarray) else (list(x) if isinstance(x, list) else x)) for k, x in state.items()}
    r, w, best = rank2(fitness_bits, P, mutant)
    g = state["header"][0]
    h = out["header"]
    h[0] = g if mutant == "g_not_advanced" else (g + 1) & NO_SLOT
    h[1] = state["header"][1] + 1
    h[2], h[3], h[4] = g, best, 2 * H
    out["t"] = t = state["t"] + 1
    out["rank2"], out["weights"] = r, w
    i = np.arange(PARAMS) if idx is None else np.asarray(idx)
    out["grad"] = out["ghat"] = None
    if H > 0:
        G = gsum(w, seed, g, i, mutant)
        th, m, v, grad, ghat = step(G, H, state["theta"][i], state["m"][i], state["v"][i], t, sigma, lr, beta1, beta2, eps, weight_decay,
                                    optimizer, mutant)
        out["theta"][i], out["m"][i], out["v"][i], out["grad"], out["ghat"], out["G"] = th, m, v, grad, ghat, G
    return out


# ------------------------------------------------------------------------------------------------ fixtures
def fixture_theta(seed=3):
    rng = np.random.RandomState(seed)
    theta = (rng.randn(PARAMS) * 0.3).astype(np.float32)
    theta[:4] = [0.0, -0.0, 1e-30, -2.5]
    return theta


def fixture_log(N, seg, P, C_, seed, env_offset=0, short=0, strays=True):
    """a log of C_ slots with N - short records in a shuffled order, the other `short` worlds unfinished; special returns,
    a foreign world and (with strays) worlds beyond P seg are part of it"""
    rng = np.random.RandomState(seed)
    worlds = rng.permutation(N)
    done = worlds[:N - short]
    finished = np.zeros(max(N, 1), dtype=np.uint8)
    finished[done] = 1
    ret = (rng.randn(max(N, 1)) * 30).astype(np.float32)
    records = len(done)
    log_ret = np.zeros(C_, dtype=np.float32)
    log_code = np.zeros(C_, dtype=np.uint8)
    log_world = np.zeros(C_, dtype=np.int64)
    log_ret[:records] = (rng.randn(records) * 40).astype(np.float32)
    log_code[:records] = rng.randint(1, 4, records)
    log_world[:records] = done + env_offset
    special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 2048.0, -2048.0, 2049.0, -0.0, 2.0 ** -21, 3 * 2.0 ** -21, 1.5], dtype=np.float32)
    k = min(len(special), records)
    log_ret[:k] = special[:k]
    if short:
        open_ = worlds[N - short:]
        ret[open_[:min(len(special), short)]] = special[:min(len(special), short)]
    if records > 2:
        log_world[records - 1] = env_offset + N + 12345          # a foreign world
        finished[done[records - 1]] = 1
    # slots past the cursor hold stale records that must not be read
    log_ret[records:] = 777.0
    log_world[records:] = env_offset
    log_code[records:] = 3
    return {"log_ret": log_ret, "log_code": log_code, "log_world": log_world, "cursor": records, "ret": ret, "finished": finished,
            "env_offset": env_offset, "N": N, "seg": seg, "P": P}


def fixture_fitness(P, seed=0):
    """fitness bits with ties, NaNs, both infinities and both zeros among ordinary values"""
    rng = np.random.RandomState(100 + seed)
    f = np.round(rng.randn(P) * 4).astype(np.float32) / 2          # many ties
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, np.inf, -np.inf], dtype=np.float32)
    at = rng.permutation(P)[:min(len(special), P)]
    f[at] = special[:len(at)]
    u = bits(f).copy()
    if P > 8:
        u[rng.permutation(P)[0]] = 0xFFC00001                     # a negative NaN with a payload
    return u


# ------------------------------------------------------------------------------------------------ what the mutants are judged on
RESULT_CFG = dict(sigma=0.05, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0)
RESULT_SEED = 77
RESULT_IDX = np.arange(0, PARAMS, 37)
RESULT_LOG = dict(N=130, seg=64, P=4, C_=256, seed=5, short=9)      # segment 2 is short, segment 3 empty
RESULT_TELLS = ((5, 4), (66, 4))                               # (P, the generation before the first of two tells)


def pack_tell(s):
    """what is compared of a tell's state: theta, m, v at RESULT_IDX, rank2, weights and the header, as uint32 words"""
    return np.concatenate([bits(s["theta"][RESULT_IDX]), bits(s["m"][RESULT_IDX]), bits(s["v"][RESULT_IDX]), s["rank2"].view(np.uint32),
                           s["weights"].view(np.uint32), np.array(s["header"], dtype=np.uint64).view(np.uint32)])


def results(mutant=None):
    """everything the fixtures give under one mutant (None: the rule), as a dict of arrays: a population of 5, both fitness
    kinds of a log with a short last segment, an empty one and unfinished worlds, and two Adam tells in a row for an odd and
    an even P.  tests/test_evo_gpu.py computes the same dict on the device"""
    theta = fixture_theta()
    c = RESULT_CFG
    out = {"ask5": bits(ask(theta, 5, c["sigma"], RESULT_SEED, 3, mutant=mutant))}
    log = fixture_log(**RESULT_LOG)
    for kind in (MEAN_RETURN, SUCCESS_RATE):
        f, episodes, _ = fitness(log["log_ret"], log["log_code"], log["log_world"], log["cursor"], log["ret"], log["finished"], 0, log["N"],
                                 log["seg"], log["P"], kind, mutant=mutant)
        out["fitness%d" % kind], out["episodes%d" % kind] = f, episodes
    for P, g in RESULT_TELLS:
        s = fresh(theta, g)
        for k, name in enumerate("ab"):
            s = tell({key: s[key] for key in ("theta", "m", "v", "t", "header")}, fixture_fitness(P, 2 + k), P, RESULT_SEED, c["sigma"], c["lr"],
                     c["beta1"], c["beta2"], c["eps"], c["weight_decay"], ADAM, idx=RESULT_IDX, mutant=mutant)
            out["tell%d%s" % (P, name)] = pack_tell(s)
    return out
