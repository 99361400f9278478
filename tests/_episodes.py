"""The numpy model of libaqua_episodes.so (include/aqua_episodes.h) -- after_step and explore exactly as the header states
them -- generators of synthetic (reward, term, time) streams, and a thin device harness that calls the C ABI on torch
tensors laid out like the model's arrays.  Shared by tests/test_episodes_cpu.py and tests/test_episodes_gpu.py."""
import numpy as np

STREAM = 5
BUFFERS = ("ret", "len", "finished", "log_ret", "log_len", "log_code", "log_world", "counts")


def eps_decay(init, final, decay):
    """main/impl/dqn.py:139-140"""
    return decay if decay < 1 else (final / init) ** (1 / decay)


def pow_lsb_first(decay, n):
    """decay^n by binary exponentiation, least-significant bit first: multiplications only, so Python floats reproduce the
    device's float64 bit for bit"""
    result, base = 1.0, float(decay)
    while n:
        if n & 1:
            result *= base
        base *= base
        n >>= 1
    return result


class Model(object):
    """State of one tracker: N worlds, a log of C records, optionally once mode and an epsilon schedule (init, final, decay)"""

    def __init__(self, N, C, once=False, eps=None):
        self.N, self.C = N, C
        self.ret = np.zeros(N, dtype=np.float32)
        self.len = np.zeros(N, dtype=np.int32)
        self.finished = np.zeros(N, dtype=np.uint8) if once else None
        self.log_ret = np.zeros(C, dtype=np.float32)
        self.log_len = np.zeros(C, dtype=np.int32)
        self.log_code = np.zeros(C, dtype=np.uint8)
        self.log_world = np.zeros(C, dtype=np.int64)
        self.counts = np.zeros(8, dtype=np.uint64)
        self.eps = eps
        self.eps_state = None if eps is None else float(eps[0])
        self.eps_out = None if eps is None else np.float32(eps[0])

    def after_step(self, reward, term, time=None, env_offset=0, lo=0, hi=None):
        """account worlds [lo, hi) of this state from reward / term / time of that many elements"""
        hi = self.N if hi is None else hi
        ret, ln = self.ret[lo:hi], self.len[lo:hi]                     # views
        fin = None if self.finished is None else self.finished[lo:hi]
        counted = np.ones(hi - lo, dtype=bool)
        if fin is not None:
            counted &= fin == 0
        if time is not None:
            counted &= (term != 0) | (time >= 0)
        ret[counted] = ret[counted] + reward[counted]                  # one float32 add per world
        ln[counted] += 1
        idx = np.nonzero(counted & (term != 0))[0]
        n = int(idx.shape[0])
        slots = (int(self.counts[0]) + np.arange(n, dtype=np.int64)) % self.C
        self.log_ret[slots], self.log_len[slots], self.log_code[slots] = ret[idx], ln[idx], term[idx]
        self.log_world[slots] = env_offset + idx
        ret[idx], ln[idx] = 0, 0
        if fin is not None:
            fin[idx] = 1
        self.counts[0] += np.uint64(n)
        for code in (1, 2, 3):
            self.counts[code] += np.uint64(int((term[idx] == code).sum()))
        self.counts[4] += np.uint64(int(counted.sum()))
        if self.eps is not None:
            self.eps_state = max(self.eps_state * pow_lsb_first(self.eps[2], n), float(self.eps[1]))
            self.eps_out = np.float32(self.eps_state)
        return n


def draws(oracle, n, seed, env_offset, tick):
    """the policy kernel's draw for n worlds through the oracle's Philox, as tests/test_qpolicy_gpu.py models it
    -> (the uniform float32 [n], the exploring action uint8 [n])"""
    c3 = ((tick >> 32) & 0xFFFF) | (STREAM << 24)
    r = np.array([oracle.philox((seed & 0xFFFFFFFF, seed >> 32),
                                ((env_offset + i) & 0xFFFFFFFF, (env_offset + i) >> 32, tick & 0xFFFFFFFF, c3)) for i in range(n)],
                 dtype=np.uint64)
    u = (r[:, 0] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u, (((r[:, 1] >> np.uint64(8)) * np.uint64(3)) >> np.uint64(24)).astype(np.uint8)


def draws_vectorised(n, seed, env_offset, tick):
    """draws() for worlds env_offset .. env_offset + n - 1 at once, through tests/_placement.py's array Philox (stream 5,
    attempt 0) -> (the uniform float32 [n], the exploring action uint8 [n])"""
    from tests import _placement as P
    r = P.draw(seed, env_offset + np.arange(n, dtype=np.int64), tick, STREAM, 0)
    u = (r[0] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u, (((r[1] >> np.uint64(8)) * np.uint64(3)) >> np.uint64(24)).astype(np.uint8)


BLOCK, MAX_BLOCKS, EXPLORE_MAX_BLOCKS = 256, 1024, 2048    # csrc/aqua_episodes.hip


def launch_shape(N):
    """csrc/aqua_episodes.hip's shape_of restated: -> (chunk, blocks).  Block b accounts worlds [b chunk, (b + 1) chunk), a
    tile of BLOCK worlds per trip.  tests/test_launch_regimes_cpu.py pins BLOCK and MAX_BLOCKS through
    aquaep_workspace_bytes."""
    tiles = (N + BLOCK - 1) // BLOCK
    chunk = max(1, (tiles + MAX_BLOCKS - 1) // MAX_BLOCKS) * BLOCK
    return chunk, (N + chunk - 1) // chunk


def explore(action, eps, u, drawn):
    """the exploration pass on a numpy uint8 action array -> (the new actions, which worlds explored)"""
    return np.where(u < np.float32(eps), drawn, action).astype(np.uint8), u < np.float32(eps)


# ------------------------------------------------------------------------------------------------ streams
def make_stream(N, T, p_finish, seed, markers=False):
    """-> reward float32 [T][N], term uint8 [T][N], time int32 [T][N] or None.
    Rewards are random float32 with full mantissas: their running sums round at every add, so another order of adds shows.
    markers: the time row of next-step restart mode (include/aqua_hip.h) -- a world that ends at tick t carries -1 - (t & 1),
    is restarted during the next tick (-3 - (t & 1), that tick is no part of an episode) and steps again the tick after;
    one restart in five waits a second tick with its end marker.  The ticks outside episodes carry a NON-zero reward here, so
    that a wrong counted-world rule shows in the returns as well as in the lengths."""
    rng = np.random.RandomState(seed)
    reward = (rng.uniform(-1.0, 1.0, (T, N)) * rng.choice([1e-3, 0.37, 11.0], (T, N))).astype(np.float32)
    ends = rng.random_sample((T, N)) < p_finish
    codes = rng.randint(1, 4, (T, N)).astype(np.uint8)
    if not markers:
        return reward, np.where(ends, codes, 0).astype(np.uint8), None
    term = np.zeros((T, N), dtype=np.uint8)
    time = np.zeros((T, N), dtype=np.int32)
    phase = np.zeros(N, dtype=np.int64)            # 0 stepping, 1 ended at the last tick, 2 waits one more tick
    clock = np.zeros(N, dtype=np.int32)
    waits = rng.random_sample((T, N)) < 0.2
    for t in range(T):
        stepping = phase == 0
        wait = (phase == 1) & waits[t]
        restart = (phase != 0) & ~wait
        term[t] = np.where(stepping & ends[t], codes[t], 0)
        clock = np.where(stepping, clock + 1, clock)
        clock = np.where(term[t] != 0, -1 - (t & 1), clock)
        clock = np.where(restart, -3 - (t & 1), clock)           # (a waiting world keeps its end marker)
        time[t] = clock
        phase = np.where(term[t] != 0, 1, np.where(wait, 2, 0))
        clock = np.where(restart, 0, clock)
    assert (time[term != 0] < 0).all()
    return reward, term, time


def naive_loop(reward, term, time, once, eps):
    """The same accounting the way main/impl/dqn.py:151-186 reads: one world at a time, episode_reward += reward,
    episode_steps += 1 until done; the episodes of the batch are then ordered by (step, world).
    -> records [(step, world, return, steps, code)], epsilon after every episode in that order"""
    T, N = reward.shape
    records = []
    for w in range(N):
        episode_reward, episode_steps = np.float32(0), 0
        for t in range(T):
            if time is not None and term[t, w] == 0 and time[t, w] < 0:
                continue                                          # the world is being restarted: no step was taken
            episode_reward = np.float32(episode_reward + reward[t, w])
            episode_steps += 1
            if term[t, w] != 0:
                records.append((t, w, episode_reward, episode_steps, int(term[t, w])))
                episode_reward, episode_steps = np.float32(0), 0
                if once:
                    break
    records.sort(key=lambda r: (r[0], r[1]))
    epsilons = []
    if eps is not None:
        epsilon, decay = eps[0], eps_decay(*eps)
        for _ in records:
            epsilon = max(epsilon * decay, eps[1])                # dqn.py:184
            epsilons.append(epsilon)
    return records, epsilons


# ------------------------------------------------------------------------------------------------ the device side
class Device(object):
    """The model's arrays as torch tensors on the GPU and aquaep_after_step_f32 on them"""

    def __init__(self, torch, N, C, once=False, eps=None, device="cuda:0"):
        from aquaticgymenv_amd import _episodes_capi
        self.torch, self.capi, self.N, self.C = torch, _episodes_capi, N, C
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=device)          # noqa: E731
        self.ret, self.len = z(N, torch.float32), z(N, torch.int32)
        self.finished = z(N, torch.uint8) if once else None
        self.log_ret, self.log_len, self.log_code, self.log_world = z(C, torch.float32), z(C, torch.int32), z(C, torch.uint8), z(C, torch.int64)
        self.counts = z(8, torch.int64)
        self.eps = eps
        self.eps_state = None if eps is None else torch.full((1,), eps[0], dtype=torch.float64, device=device)
        self.eps_out = None if eps is None else torch.full((1,), eps[0], dtype=torch.float32, device=device)
        self.workspace = torch.full((int(_episodes_capi.lib.aquaep_workspace_bytes(N)),), 0xA5, dtype=torch.uint8, device=device)

    def after_step(self, reward, term, time=None, env_offset=0, lo=0, hi=None):
        torch = self.torch
        hi = self.N if hi is None else hi
        sched = self.eps is not None
        rc = self.capi.lib.aquaep_after_step_f32(
            reward.data_ptr(), term.data_ptr(), None if time is None else time.data_ptr(), env_offset, hi - lo,
            self.ret[lo:].data_ptr(), self.len[lo:].data_ptr(), None if self.finished is None else self.finished[lo:].data_ptr(),
            self.log_ret.data_ptr(), self.log_len.data_ptr(), self.log_code.data_ptr(), self.log_world.data_ptr(), self.C,
            self.counts.data_ptr(), self.eps_state.data_ptr() if sched else None, self.eps_out.data_ptr() if sched else None,
            self.eps[2] if sched else 1.0, self.eps[1] if sched else 0.0,
            self.workspace.data_ptr(), self.workspace.numel(), torch.cuda.current_stream().cuda_stream)
        self.capi.check(rc, "aquaep_after_step_f32")

    def differences(self, model):
        """names of the buffers that differ from the model's, bit for bit (returns compared as their bit patterns)"""
        bad = []
        for name in BUFFERS:
            want, got = getattr(model, name), getattr(self, name)
            if want is None:
                continue
            got = got.cpu().numpy()
            if name in ("ret", "log_ret"):
                want, got = want.view(np.uint32), got.view(np.uint32)
            if name == "counts":
                got = got.view(np.uint64)
            if not np.array_equal(got, want):
                bad.append(name)
        if model.eps is not None:
            if float(self.eps_state.cpu().numpy()[0]).hex() != float(model.eps_state).hex():
                bad.append("eps_state")
            if self.eps_out.cpu().numpy().view(np.uint32)[0] != np.float32(model.eps_out).view(np.uint32):
                bad.append("eps_out")
        return bad
