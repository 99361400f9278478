"""The device-cursor experience ring of include/aqua_replay.h restated in numpy, for tests/test_replay_*.py and
tests/test_trainer_gpu.py: the header rule, the four kernels and the `ok` rule of aquaticgymenv_amd/replay.py.  Everything
is a copy or an integer draw, so the GPU tests compare with np.array_equal and state no tolerance.
"""
import numpy as np

from tests import _learner as L

HEADER_WORDS = 4
CURSOR, SIZE, BASE, CLOSED = 0, 1, 2, 3
ROWS = ("s", "a", "r", "s2", "d", "ok")


def live(time, n):
    """the `ok` row: a world whose time marker is -1 or -2 is about to be restarted instead of stepped (next-step mode)"""
    if time is None:
        return np.ones(n, dtype=np.uint8)
    t = np.asarray(time[:n])
    return ((t >= 0) | (t <= -3)).astype(np.uint8)


class Model(object):
    def __init__(self, capacity, ring_ld=None, continuous=False, fill=0):
        """rows of pitch ring_ld >= capacity; everything, the columns behind `capacity` included, starts as `fill`"""
        self.capacity, self.continuous = int(capacity), bool(continuous)
        ld = self.ring_ld = self.capacity if ring_ld is None else int(ring_ld)
        assert ld >= self.capacity >= 1
        self.header = np.zeros(HEADER_WORDS, dtype=np.int64)
        self.s = np.full((5, ld), fill, dtype=np.float32)
        self.s2 = np.full((5, ld), fill, dtype=np.float32)
        self.r = np.full(ld, fill, dtype=np.float32)
        self.a = np.full((2, ld), fill, dtype=np.float32) if continuous else np.full(ld, fill, dtype=np.uint8)
        self.d = np.full(ld, fill, dtype=np.uint8)
        self.ok = np.full(ld, fill, dtype=np.uint8)

    def slots(self, base, n):
        return (int(base) + np.arange(n, dtype=np.int64)) % self.capacity

    def open(self, obs, action, time, n):
        """obs [5][>= n], action [>= n] | [2][>= n], time [>= n] or None"""
        base = int(self.header[CURSOR])
        self.header[BASE] = base
        if not 0 <= base < self.capacity:
            return
        at = self.slots(base, n)
        self.s[:, at] = obs[:, :n]
        if self.continuous:
            self.a[:, at] = action[:, :n]
        else:
            self.a[at] = action[:n]
        self.ok[at] = live(time, n)

    def close(self, reward, obs, term, n):
        base = int(self.header[BASE])
        if not 0 <= base < self.capacity:
            return
        at = self.slots(base, n)
        self.r[at] = reward[:n]
        self.s2[:, at] = obs[:, :n]
        self.d[at] = term[:n]
        self.header[CURSOR] = (base + n) % self.capacity
        self.header[SIZE] = min(self.capacity, max(int(self.header[SIZE]), 0) + n)
        self.header[CLOSED] += 1

    def ring(self, size=None):
        """the ring as tests/_learner.py reads it; size: default the header's, clamped as the draw kernel clamps it"""
        c = self.capacity
        size = min(max(int(self.header[SIZE]), 0), c) if size is None else size
        return dict(s=self.s[:, :c], a=self.a[..., :c], r=self.r[:c], s2=self.s2[:, :c], d=self.d[:c], ok=self.ok[:c], size=size)

    def draw(self, seed, t, batch):
        """idx of the update that takes t to t + 1"""
        return L.drawn(seed, int(t) + 1, batch, self.ring())

    def gather(self, idx):
        """-> (s [B][5], a [B] | [B][2], r [B], s2 [B][5], done [B], valid [B])"""
        eff = L.effective(idx, self.ring(size=self.capacity))
        valid = eff >= 0
        at = np.where(valid, eff, 0).astype(np.int64)
        z = lambda x: np.where(valid.reshape((-1,) + (1,) * (x.ndim - 1)), x, np.zeros((), dtype=x.dtype))     # noqa: E731
        a = self.a[:, at].T if self.continuous else self.a[at]
        return (z(self.s[:, at].T), z(a), z(self.r[at]), z(self.s2[:, at].T), z((self.d[at] != 0).astype(np.uint8)),
                valid.astype(np.uint8))


def naive_loop(batches, capacity):
    """The same ring one world at a time, the way main/impl/dqn.py:174 appends: -> (list of capacity slots, each None or
    the tuple (s, a, r, s2, d, ok); cursor; size).  batches: [(obs, action, time, reward, obs2, term, n)]"""
    slots, cursor, size = [None] * capacity, 0, 0
    for obs, action, time, reward, obs2, term, n in batches:
        for i in range(n):
            t = None if time is None else int(time[i])
            ok = 1 if (t is None or t >= 0 or t <= -3) else 0
            a = tuple(action[:, i]) if np.ndim(action) == 2 else int(action[i])
            slots[(cursor + i) % capacity] = (tuple(obs[:, i]), a, float(reward[i]), tuple(obs2[:, i]), int(term[i]), ok)
        cursor = (cursor + n) % capacity
        size = min(capacity, size + n)
    return slots, cursor, size


def make_batch(rng, n, src_ld, continuous=False, with_time=True, poison=None):
    """one batched step's inputs with pitch src_ld >= n; the padding holds `poison` values that must never reach the ring
    -> dict(obs, action, time, reward, obs2, term)"""
    def row(shape, draw, dtype, bad):
        x = np.full(shape, bad, dtype=dtype)
        x[..., :n] = draw(shape[:-1] + (n,)).astype(dtype)
        return x
    f = lambda shape: rng.rand(*shape) * 2 - 1          # noqa: E731
    bad_f = -7.0e30 if poison is None else poison
    out = dict(obs=row((5, src_ld), f, np.float32, bad_f), obs2=row((5, src_ld), f, np.float32, bad_f),
               reward=row((src_ld,), f, np.float32, bad_f),
               term=row((src_ld,), lambda sh: rng.randint(0, 4, sh) * (rng.rand(*sh) < 0.3), np.uint8, 0xEE))
    if continuous:
        out["action"] = row((2, src_ld), lambda sh: rng.rand(*sh) * 0.3 + 0.2, np.float32, bad_f)
    else:
        out["action"] = row((src_ld,), lambda sh: rng.randint(0, 3, sh), np.uint8, 0xEE)
    # every class of time marker: running (>= 0), about to restart (-1, -2: not an experience), restarted (-3, -4)
    out["time"] = row((src_ld,), lambda sh: rng.choice(np.array([0, 3, 17, -1, -2, -3, -4]), sh), np.int32, -1) if with_time else None
    return out
