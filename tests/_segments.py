"""The numpy model of libaqua_segments.so (include/aqua_segments.h) -- one account() call exactly as the header states it,
fed with the episode log as it is after the accounting call -- and the small harness the GPU tests share: an env-like
object whose reward / term / time rows a test fills by hand, so that a real EpisodeTracker writes the log.
Shared by tests/test_segments_cpu.py and tests/test_segments_gpu.py."""
import numpy as np

from tests._episodes import pow_lsb_first

LANES = 64


def window_sum(values):
    """the float64 sum in the library's order: lane l adds the slots l, l + 64, ... ascending to 0.0; then the 64 lane sums
    are added to 0.0 in ascending lane order"""
    lanes = [0.0] * LANES
    for l in range(LANES):
        s = 0.0
        for v in values[l::LANES]:
            s = s + float(v)
        lanes[l] = s
    total = 0.0
    for s in lanes:
        total = total + s
    return total


class Model(object):
    """State of one SegmentTracker: P segments of seg worlds from env_offset, windows of W, a batch of N worlds.
    eps: None or (init [P], final [P], decay factor [P])"""

    def __init__(self, N, seg, P, W, env_offset=0, eps=None, seen=0):
        self.N, self.seg, self.P, self.W, self.env_offset = N, seg, P, W, env_offset
        self.header = np.array([seen, 0, 0, 0], dtype=np.uint64)
        self.counts = np.zeros((P, 8), dtype=np.uint64)
        self.win_ret = np.zeros((P, W), dtype=np.float32)
        self.win_len = np.zeros((P, W), dtype=np.int32)
        self.win_code = np.zeros((P, W), dtype=np.uint8)
        self.mean_ret = np.zeros(P, dtype=np.float32)
        self.mean_len = np.zeros(P, dtype=np.float32)
        self.success = np.zeros(P, dtype=np.float32)
        self.eps = eps
        self.eps_state = None if eps is None else np.array(eps[0], dtype=np.float64).copy()
        self.eps_out = None if eps is None else np.array(eps[0], dtype=np.float64).astype(np.float32)

    def account(self, log_ret, log_len, log_code, log_world, cursor):
        """the log arrays (numpy, C records) and counts[0] as the accounting call left them"""
        C = int(log_world.shape[0])
        seen, cursor = int(self.header[0]), int(cursor)
        n = (cursor - seen) % (1 << 64)
        self.header[0] = np.uint64(cursor)
        if n > self.N:
            self.header[1] += np.uint64(1)
            return
        slots = (seen + np.arange(n, dtype=np.int64)) % C
        owner = (log_world[slots] - self.env_offset) // self.seg
        self.header[2] += np.uint64(int(((owner < 0) | (owner >= self.P)).sum()))
        W = self.W
        for p in range(self.P):
            mine = slots[owner == p]                                # in log order
            m = int(mine.shape[0])
            if m == 0:
                continue
            c = int(self.counts[p, 0])
            for j in range(max(0, m - W), m):
                w = (c + j) % W
                self.win_ret[p, w], self.win_len[p, w], self.win_code[p, w] = log_ret[mine[j]], log_len[mine[j]], log_code[mine[j]]
            self.counts[p, 0] += np.uint64(m)
            for code in (1, 2, 3):
                self.counts[p, code] += np.uint64(int((log_code[mine] == code).sum()))
            self.counts[p, 4] += np.uint64(int(log_len[mine].astype(np.int64).sum()))
            if self.eps is not None:
                e = max(float(self.eps_state[p]) * pow_lsb_first(float(self.eps[2][p]), m), float(self.eps[1][p]))
                self.eps_state[p] = e
                self.eps_out[p] = np.float32(e)
            k = min(c + m, W)
            self.mean_ret[p] = np.float32(window_sum(self.win_ret[p, :k]) / float(k))
            self.mean_len[p] = np.float32(float(int(self.win_len[p, :k].astype(np.int64).sum())) / float(k))
            self.success[p] = np.float32(float(int((self.win_code[p, :k] == 3).sum())) / float(k))


def eps_factor(init, final, decay):
    """main/impl/dqn.py:139-140 in Python floats"""
    return decay if decay < 1 else (final / init) ** (1 / decay)


# ------------------------------------------------------------------------------------------------ the device side
class Rows(object):
    """What EpisodeTracker needs of an env: N worlds whose reward / term / time rows the test writes"""

    def __init__(self, torch, N, env_offset=0, device="cuda:0"):
        self.torch, self.device, self.num_envs, self.env_offset = torch, torch.device(device), N, env_offset
        self.reward = torch.zeros(N, dtype=torch.float32, device=device)
        self.term = torch.zeros(N, dtype=torch.uint8, device=device)
        self.time = torch.zeros(N, dtype=torch.int32, device=device)

    def set(self, reward, term):
        torch = self.torch
        self.reward.copy_(torch.from_numpy(np.ascontiguousarray(reward, dtype=np.float32)))
        self.term.copy_(torch.from_numpy(np.ascontiguousarray(term, dtype=np.uint8)))


def feed(model, tracker):
    """one model.account() on the tracker's log read back"""
    model.account(tracker.log_ret.cpu().numpy(), tracker.log_len.cpu().numpy(), tracker.log_code.cpu().numpy(),
                  tracker.log_world.cpu().numpy(), int(tracker._counts.cpu().numpy().view(np.uint64)[0]))


def differences(st, model):
    """names of the SegmentTracker's buffers that differ from the model's, bit for bit"""
    pairs = [("header", st.header, model.header), ("counts", st._counts, model.counts), ("win_ret", st.win_ret, model.win_ret),
             ("win_len", st.win_len, model.win_len), ("win_code", st.win_code, model.win_code), ("mean_ret", st.mean_return, model.mean_ret),
             ("mean_len", st.mean_length, model.mean_len), ("success", st.success_rate, model.success)]
    if model.eps is not None:
        pairs += [("eps_state", st._eps_state, model.eps_state), ("eps_out", st.epsilon, model.eps_out)]
    bad = []
    for name, got, want in pairs:
        got = got.cpu().numpy()
        if not np.array_equal(got.view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1)):
            bad.append(name)
    return bad
