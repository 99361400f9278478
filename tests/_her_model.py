"""The hindsight relabelling of aquaticgymenv_amd/csrc/aqua_her.h restated in numpy, written from the header's text, for
tests/test_her_cpu.py and tests/test_her_gpu.py: the walk, the draw, the relabelled rows and the reward.  Every quantity is a
copy, an integer or a float64 expression of rounded float64 operations (numpy's float64 scalars neither contract nor
reassociate, and its sqrt is correctly rounded), so the tests compare with np.array_equal on bit patterns and state no
tolerance.
"""
import numpy as np

from tests import _placement

MAX_HORIZON = 64
STREAM = 8
TERM_SUCCESS = 3

# the branch a sample takes, named for the tests that want every branch to occur.  A sample has one CUT (why its walk ended)
# and one FATE (what became of it); what is no sample has neither.
BAD_CURSOR, OUTSIDE, NOT_OK = "bad_cursor", "outside", "not_ok"                       # no sample
OWN_TERMINAL, EPISODE_END, BROKEN, FRONTIER, CAPPED = "own_terminal", "episode_end", "broken", "frontier", "capped"   # cuts
NOT_CHOSEN, SUCCESS_K0, SUCCESS_LATER, SHAPED, KEPT = "not_chosen", "success_k0", "success_later", "shaped", "kept"   # fates
NO_SAMPLE = (BAD_CURSOR, OUTSIDE, NOT_OK)


def threshold(ratio):
    """aquaher_threshold: floor(ratio 2^32), an integer"""
    ratio = float(ratio)
    assert 0.0 <= ratio <= 1.0
    return int(np.floor(np.float64(ratio) * np.float64(4294967296.0)))


def gap(qx, qy, gx, gy):
    """100 sqrt(dx^2 + dy^2) - 5 in float64, every operation rounded; the inputs are float32 (arrays or scalars)"""
    dx = np.asarray(qx, np.float32).astype(np.float64) - np.asarray(gx, np.float32).astype(np.float64)
    dy = np.asarray(qy, np.float32).astype(np.float64) - np.asarray(gy, np.float32).astype(np.float64)
    return np.float64(100.0) * np.sqrt(dx * dx + dy * dy) - np.float64(5.0)


def reward(sx, sy, s2x, s2y, gx, gy):
    """aquaher_reward on arrays -> (r float32, d uint8)"""
    gap_prev, gap_new = gap(sx, sy, gx, gy), gap(s2x, s2y, gx, gy)
    hit = gap_new <= 0.0
    shaped = (np.float64(0.7) * (gap_prev - gap_new)).astype(np.float32)
    return np.where(hit, np.float32(10.0), shaped).astype(np.float32), np.where(hit, TERM_SUCCESS, 0).astype(np.uint8)


def walk(ring, cursor, N, c, H):
    """The walk of slot c.  ring: dict(d, ok) of [>= capacity] rows and `capacity`.  -> (what, M): what is one of NO_SAMPLE
    (then M = 0) or the cut of a sample's walk."""
    cap = int(ring["capacity"])
    cursor, N, c, H = int(cursor), int(N), int(c), int(H)
    if not 0 <= cursor < cap or cursor % N != 0:
        return BAD_CURSOR, 0
    if not 0 <= c < cap:
        return OUTSIDE, 0
    if ring["ok"][c] == 0:
        return NOT_OK, 0
    age = ((cursor - N - (c - c % N)) % cap) // N
    M = 0
    for k in range(H):
        slot = (c + k * N) % cap
        if k > age:
            return FRONTIER, M
        if k > 0 and ring["ok"][slot] == 0:
            return BROKEN, M
        if ring["d"][slot] != 0:
            return (OWN_TERMINAL if k == 0 else EPISODE_END), M
        M = k + 1
    return CAPPED, M


def draws(seed, t, B):
    """the words r[0], r[1] of samples j = 0 .. B - 1 of a row whose key is `seed` and whose update counter is `t`"""
    r = _placement.draw(seed, np.arange(B, dtype=np.uint64), int(t) + 1, STREAM, 0)
    return r[0], r[1]


def relabel(ring, header, N, idx, H, ratio, t, seeds):
    """aquaher_relabel.  ring: dict(s [5][ld], a [ld] | [2][ld], r, s2 [5][ld], d, ok, capacity); header: int64 [4]; idx: int32
    [P][B]; t: the P update counters; seeds: the P keys (the scalar form is P equal keys).
    -> dict(s [5][P B], a, r, s2, d, ok, k, m, cut: list of P B names, fate: list of P B names (None for no sample))"""
    assert 1 <= H <= MAX_HORIZON
    idx = np.asarray(idx)
    P, B = idx.shape
    m = P * B
    cap = int(ring["capacity"])
    thr = threshold(ratio)
    cont = ring["a"].ndim == 2
    out = dict(s=np.zeros((5, m), np.float32), s2=np.zeros((5, m), np.float32), r=np.zeros(m, np.float32),
               a=np.zeros((2, m), np.float32) if cont else np.zeros(m, np.uint8), d=np.zeros(m, np.uint8), ok=np.zeros(m, np.uint8),
               k=np.zeros(m, np.uint8), m=np.zeros(m, np.uint8), cut=[], fate=[])
    # the walk, once per distinct slot of the draw (it does not depend on the sample's position)
    flat = idx.reshape(-1).astype(np.int64)
    walks = {c: walk(ring, header[0], N, c, H) for c in set(flat.tolist())}
    out["cut"] = [walks[c][0] for c in flat.tolist()]
    M = np.array([walks[c][1] for c in flat.tolist()], np.uint64)
    valid = np.array([what not in NO_SAMPLE for what in out["cut"]], bool)
    at = np.where(valid, flat, 0)
    for name in ("s", "a", "r", "s2", "d"):
        out[name][..., valid] = ring[name][..., at[valid]]
    out["ok"][valid] = 1
    out["m"][:] = M
    # the draw: row p keyed by (seeds[p], t[p] + 1), sample j its counter
    words = [draws(seeds[p], t[p], B) for p in range(P)]
    r0, r1 = (np.concatenate([w[i] for w in words]).astype(np.uint64) for i in (0, 1))
    chosen = valid & (M > 0) & (r0 < np.uint64(thr))
    k = (r1 * M) >> np.uint64(32)                              # < 2^32 x 64: no overflow
    slot = (at + k.astype(np.int64) * int(N)) % cap
    g = ring["s2"][0:2][:, slot[chosen]]
    out["s"][3:5, chosen] = g
    out["s2"][3:5, chosen] = g
    src = at[chosen]
    rew, code = reward(ring["s"][0, src], ring["s"][1, src], ring["s2"][0, src], ring["s2"][1, src], g[0], g[1])
    out["r"][chosen], out["d"][chosen] = rew, code
    out["k"][chosen] = (k[chosen] + np.uint64(1)).astype(np.uint8)
    for i in range(m):
        if not valid[i]:
            out["fate"].append(None)
        elif M[i] == 0:
            out["fate"].append(KEPT)
        elif not chosen[i]:
            out["fate"].append(NOT_CHOSEN)
        elif out["d"][i] == 0:
            out["fate"].append(SHAPED)
        else:
            out["fate"].append(SUCCESS_K0 if k[i] == 0 else SUCCESS_LATER)
    return out


def per_world(ring, cursor, N, c, H):
    """A restatement of M that shares no line with walk(): unroll the ring into the transitions of c's world in the order they
    were made, oldest first, and count the leading non-terminal experiences from c's on, H at most.  Assumes a valid cursor
    and 0 <= c < capacity."""
    cap, N = int(ring["capacity"]), int(N)
    rounds, world = cap // N, c % N
    newest = (cursor // N - 1) % rounds                      # the round closed last
    order = [((newest + 1 + i) % rounds) * N + world for i in range(rounds)]     # oldest ... newest
    ahead = order[order.index(c):][:H]
    count = 0
    for slot in ahead:
        if ring["ok"][slot] == 0 or ring["d"][slot] != 0:
            break
        count += 1
    return count


def crafted_ring(capacity=42, N=7, continuous=False, seed=5, ld=None):
    """A synthetic ring for the kernel test: positions uniform in [0, 1] (so gaps of both signs occur under a relabelled
    goal), with termination codes and ok holes sprinkled in, and one world (0) without either."""
    rng = np.random.RandomState(seed)
    ld = capacity if ld is None else ld
    ring = dict(capacity=capacity,
                s=rng.rand(5, ld).astype(np.float32), s2=rng.rand(5, ld).astype(np.float32),
                r=((rng.rand(ld) * 2 - 1) * 3).astype(np.float32),
                a=(rng.rand(2, ld) * 0.3 + 0.2).astype(np.float32) if continuous else rng.randint(0, 3, ld).astype(np.uint8),
                d=(rng.randint(1, 4, ld) * (rng.rand(ld) < 0.15)).astype(np.uint8), ok=(rng.rand(ld) >= 0.1).astype(np.uint8))
    ring["d"][0:capacity:N] = 0
    ring["ok"][0:capacity:N] = 1
    # some steps short enough that the boat stays within the radius (0.05 normalised) of where it later is: successes with k > 0
    near = rng.rand(ld) < 0.5
    for row in (0, 1):
        ring["s2"][row, near] = (ring["s"][row, near] + (rng.rand(int(near.sum())) - 0.5) * 0.02).astype(np.float32)
    for c in range(capacity - N):
        if rng.rand() < 0.5:
            ring["s"][0:2, c + N] = ring["s2"][0:2, c]
            if near[c + N]:
                ring["s2"][0:2, c + N] = ring["s"][0:2, c + N] + np.float32(0.004)
    return ring
