"""GPU tests of every kernel family ABOVE its grid cap, where a wavefront, block or thread takes several tiles in a loop:
the learner with tiles_per_wave >= 2 (B > 32 768), episode accounting with a chunk of several tiles (N > 262 144), the
exploration pass and the ring's draw and gather in their grid-stride loops (> 2 048 blocks x 256).

The sizes, and where the samples and endings sit, come from the Python mirrors of the two `shape_of` functions
(tests/_learner.py::launch_shape, tests/_episodes.py::launch_shape), pinned on the CPU by tests/test_launch_regimes_cpu.py;
every test asserts from them that its size really is past the cap, so raising a cap makes the test say so instead of
passing with one trip.  References and contracts are those of test_learner_gpu.py, test_episodes_gpu.py and
test_replay_gpu.py: exact wherever the arithmetic is exact, 4 E_g / 4 E_l against float64 for the dense gradient.
"""
import numpy as np
import pytest

from tests import _episodes as E
from tests import _learner as L
from tests import _replay as R
from tests.test_learner_gpu import CASES, GAP_CAP, U, _float_ring, _idx, _learner, _nets, _same, _set, _state
from tests.test_replay_gpu import _filled_model, _ring_from

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096                               # bytes behind a workspace that must keep their pattern
OFFSET = (5 << 32) + 12345                 # a world index beyond 32 bits
STRIDE_N = 2048 * 256 + 65                 # one grid-stride trip of 2 048 blocks x 256 and a ragged second one


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def _guarded(torch, need):
    """-> (a uint8 tensor of need + GUARD bytes, its first `need` bytes as the workspace, the pattern behind them)"""
    whole = torch.zeros(need + GUARD, dtype=torch.uint8, device=DEV)
    pattern = torch.from_numpy((np.arange(GUARD) % 251 + 1).astype(np.uint8)).to(DEV)
    whole[need:] = pattern
    assert need % 16 == 0 and whole.data_ptr() % 16 == 0
    return whole, whole[:need], pattern


# ================================================================================================ 1. the learner
def _check_exact_idx(torch, layers, target, strategy, B, ring, cap, idx, eff):
    """tests/test_learner_gpu.py::_check_exact for a given index vector (its effective form computed by the caller)"""
    theta, theta_t = L.flatten(layers), L.flatten(target)
    worst, S, ref = L.abs_sums(theta, theta_t, ring, eff, strategy)
    assert worst < 2 ** 24, worst                       # asserted in int64 before the kernel runs
    lrn = _learner(torch, layers, target, gamma=1.0, strategy=strategy)
    out = torch.full((B + 8,), 77, dtype=torch.int32, device=DEV)
    lrn.update(L.DeviceRing(torch, ring, DEV), B, idx=_idx(torch, idx), idx_out=out)
    st = _state(torch, lrn)
    got = out.cpu().numpy()
    assert np.array_equal(got[:B], eff) and bool((got[B:] == 77).all())
    n = int((eff >= 0).sum())
    assert n == ref["n"] and n < B and len(set(eff[eff >= 0].tolist())) < n
    want = S.astype(np.float32) * np.float32(2.0 / n)
    assert np.array_equal(S.astype(np.float32).astype(np.int64), S)
    bad = np.nonzero(st["grad"].view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (strategy, B, bad.size, bad[:8], st["grad"][bad[:8]], want[bad[:8]])
    assert np.count_nonzero(want) > 500
    assert abs(float(st["loss"][0]) - float(ref["loss"])) <= 4 * U * float(ref["loss"])
    assert int(st["t"][0]) == 1
    return worst, ref


@pytest.mark.parametrize("strategy", L.STRATEGIES)
@pytest.mark.parametrize("B", [32769, 65601, 1 << 20])
def test_exact_integer_gradient_with_several_tiles_per_wavefront(torch, B, strategy):
    """The recipe of test_exact_integer_gradient_every_tail (integer networks, int_ring(300, 257), gamma = 1: the gradient is
    float32(S) * float32(2 / B_eff) bit for bit in any order) at 2, 3 and 32 tiles per wavefront.  At most 4 096 entries
    are not -1 -- an invalid sample adds an exact zero, so exactness survives any B -- and tests/_learner.py::sparse_indices
    places them by launch_shape(B): whole wavefronts of live samples in the first and the last group (dk1's accumulators and
    the `small` sums carried over every tile; at 2^20 the one of the 512th partial), samples in tiles 0, 1 and the last of
    one wavefront, the ragged last tile, a wavefront whose first tile is empty, the invalid kinds and a duplicate in a
    second tile, partly filled tiles in a middle group.  check_sparse asserts all of it before the launch."""
    tiles, tpw, groups = L.launch_shape(B)
    assert tpw >= 2 and tpw == {32769: 2, 65601: 3, 1 << 20: 32}[B]
    cap, size = 300, 257
    ring = L.int_ring(cap, size, B % 1000, bad_ok=0.1)
    idx, plan = L.sparse_indices(B, ring, cap, seed=B % 1000 + 1)
    eff = L.check_sparse(B, idx, ring, cap, plan)
    worst, ref = _check_exact_idx(torch, L.int_layers("plain"), L.int_layers("plain", salt=1), strategy, B, ring, cap, idx, eff)
    print("B %d %s: %d tiles per wavefront, %d groups, %d valid samples, largest sum of |terms| 2^%.1f"
          % (B, strategy, tpw, groups, ref["n"], np.log2(worst)))


_REFS = {}


def _dense_reference(ring, net, strategy, B):
    """the float64 reference and the float32 yardstick of one dense case, computed once: the procedure of
    test_gradient_and_loss_against_float64 up to the point where the kernel's output is read"""
    key = (net, strategy, B)
    if key not in _REFS:
        layers, target = _nets(net, ring)
        theta, theta_t = L.flatten(layers), L.flatten(target)
        gamma = 0.98
        idx = np.random.RandomState(B).randint(0, ring["size"], B).astype(np.int32)
        eff = L.effective(idx, ring)
        r64 = L.gradient(theta, theta_t, ring, eff, gamma, strategy, np.float64)
        r32 = L.gradient(theta, theta_t, ring, eff, gamma, strategy, np.float32)
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
                r64 = L.gradient(theta, theta_t, ring, eff, gamma, strategy, np.float64)
                r32 = L.gradient(theta, theta_t, ring, eff, gamma, strategy, np.float32)
        assert r32["g"].dtype == np.float32 and r32["loss"].dtype == np.float32
        E_g = float(np.max(np.abs(r32["g"].astype(np.float64) - r64["g"])))
        E_l = abs(float(r32["loss"]) - float(r64["loss"]))
        _REFS[key] = dict(layers=layers, target=target, gamma=gamma, idx=idx, eff=eff, g64=r64["g"], l64=float(r64["loss"]),
                          n=r64["n"], E_g=E_g, E_l=E_l, share=share)
    return _REFS[key]


@pytest.mark.parametrize("B", [32833, 65577])
@pytest.mark.parametrize("net,strategy", CASES)
def test_dense_gradient_and_loss_against_float64_with_several_tiles_per_wavefront(torch, net, strategy, B):
    """test_gradient_and_loss_against_float64, procedure and contract unchanged (near-tie share <= 0.25 % asserted before the
    kernel's output is read; max |grad - g64| <= 4 E_g and |loss - l64| <= 4 E_l with the yardsticks recomputed here from
    float32 numpy), with every sample valid at 2 and 3 tiles per wavefront: 257 and 342 partials, each the sum of two
    wavefronts of 2 or 3 tiles.  Two learners from the same state must end with identical bits in every tensor.

    Measured on one MI355X, max |grad - g64| in units of E_g (the bound stays 4):
        case                  B = 32 833   B = 65 577
        no_obs/double_ref        0.17         0.08
        with_obs/double_ref      0.32         0.06
        random1/double_ref       0.50         0.16
        random2/double_ref       0.17         0.08
        random3/double_ref       0.07         0.05
        random1/double           0.27         0.06
        random1/fixed            0.20         0.06
        random1/standard         0.16         0.09
    Loss: 0.11 - 1.00 E_l (1.00 where the kernel's float32 loss is the float32 reference's own bits).  The near-tie share
    was at most 0.088 % (no_obs at 32 833).  A long float32 sum in numpy's order is the worse one here: E_g grows with B
    (1.1e-4 .. 2.0e-3) while the kernel adds 2 x 2 or 2 x 3 tiles per partial and then at most 342 partials."""
    tiles, tpw, groups = L.launch_shape(B)
    assert tpw >= 2 and (tpw, groups) == {32833: (2, 257), 65577: (3, 342)}[B]
    ring, dring = _float_ring(torch)
    ref = _dense_reference(ring, net, strategy, B)
    # -- only now the kernel's output
    states = []
    for _ in range(2):
        lrn = _learner(torch, ref["layers"], ref["target"], gamma=ref["gamma"], strategy=strategy)
        out = torch.zeros(B, dtype=torch.int32, device=DEV)
        lrn.update(dring, B, idx=_idx(torch, ref["idx"]), idx_out=out)
        states.append(_state(torch, lrn))
        assert np.array_equal(out.cpu().numpy(), ref["eff"]) and 0.9 * B < ref["n"] <= B
    st = states[0]
    E_g, E_l = ref["E_g"], ref["E_l"]
    err = float(np.max(np.abs(st["grad"].astype(np.float64) - ref["g64"])))
    err_l = abs(float(st["loss"][0]) - ref["l64"])
    print("%s/%s/%d: max |grad - g64| %.3e = %.2f E_g (E_g %.3e, max |g| %.3e); |loss - l64| %.3e = %.2f E_l (E_l %.3e, loss %.4e)"
          % (net, strategy, B, err, err / E_g, E_g, np.abs(ref["g64"]).max(), err_l, err_l / E_l if E_l else np.inf, E_l, ref["l64"]))
    assert err <= 4 * E_g, "max |grad - g64| %.3e > 4 E_g = %.3e" % (err, 4 * E_g)
    assert err_l <= 4 * E_l, "|loss - l64| %.3e > 4 E_l = %.3e" % (err_l, 4 * E_l)
    assert _same(states[0], states[1]) == []


def test_device_drawn_indices_with_several_tiles_per_wavefront(torch):
    """test_device_drawn_indices_match_philox at B = 32 833: the draw inside the tile loop is keyed by the sample number
    (tile0 + it) * 32 + column, and a twin fed the same indices explicitly ends with the same bits"""
    B, seed, t0 = 32833, 0x1234567890ABCDEF, 7
    assert L.launch_shape(B)[1] >= 2
    ring = L.float_ring(1000, 1000, 5, bad_ok=0.3)
    dring = L.DeviceRing(torch, ring, DEV)
    layers, target = _nets("random1", ring)
    drawn, twin = _learner(torch, layers, target, seed=seed), _learner(torch, layers, target, seed=seed)
    for lrn in (drawn, twin):
        _set(torch, lrn, t=[t0])
    seen = []
    for step in range(2):
        out = torch.full((B + 8,), -77, dtype=torch.int32, device=DEV)
        drawn.update(dring, B, idx_out=out)
        want = L.drawn(seed, t0 + 1 + step, B, ring)
        got = out.cpu().numpy()
        assert np.array_equal(got[:B], want) and bool((got[B:] == -77).all())
        assert bool((ring["ok"][want[want >= 0]] != 0).all()) and 0 < int((want < 0).sum()) < B // 50      # 0.3^4 = 0.8 %
        twin.update(dring, B, idx=_idx(torch, want))
        assert _same(_state(torch, drawn), _state(torch, twin)) == []
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1]) and int(drawn.t[0]) == t0 + 2


@pytest.mark.parametrize("B", [32768, 32769, 65537, 1 << 20])
def test_learner_workspace_bound_holds_at_the_group_cap(torch, B):
    """the workspace is exactly the bytes aqualrn_workspace_bytes(B) asks for, with a pattern behind them: 512 groups of one
    tile per wavefront, 257 of two, 342 of three and 512 of thirty-two all stay inside"""
    from aquaticgymenv_amd import _learner_capi
    tiles, tpw, groups = L.launch_shape(B)
    assert (tpw >= 2) == (B > 32768) and groups == {32768: 512, 32769: 257, 65537: 342, 1 << 20: 512}[B]
    ring, dring = _float_ring(torch)
    layers, target = _nets("random1", ring)
    lrn = _learner(torch, layers, target, seed=3)
    need = lrn._grow(B)
    assert need == int(_learner_capi.lib.aqualrn_workspace_bytes(B)) >= 16 + groups * 4 * L.PARAMS
    whole, lrn._workspace, pattern = _guarded(torch, need)
    out = torch.full((B + 8,), -77, dtype=torch.int32, device=DEV)
    lrn.update(dring, B, idx_out=out)
    torch.cuda.synchronize()
    assert lrn._workspace.data_ptr() == whole.data_ptr() and lrn._workspace.numel() == need       # _grow kept it
    assert torch.equal(whole[need:], pattern)
    got = out.cpu().numpy()
    assert int((got[:B] >= 0).sum()) > 0.9 * B and bool((got[B:] == -77).all())
    assert int(lrn.t[0]) == 1 and bool(np.isfinite(_state(torch, lrn)["grad"]).all())


# ================================================================================================ 2. episode accounting
class _Run(object):
    """E.Model and E.Device side by side through the C ABI, the device's workspace guarded, compared after every step"""

    def __init__(self, torch, N, C, once=False, eps=(1.0, 0.05, 0.9997)):
        self.torch, self.N, self.C = torch, N, C
        self.model, self.dev = E.Model(N, C, once=once, eps=eps), E.Device(torch, N, C, once=once, eps=eps)
        need = self.dev.workspace.numel()
        assert need >= 4 * E.launch_shape(N)[1]
        self.whole, self.dev.workspace, self.pattern = _guarded(torch, need)
        self.need = need

    def step(self, reward, term, time=None):
        """-> (records logged by this step, the cursor before it)"""
        torch = self.torch
        before = int(self.model.counts[0])
        d = [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (reward, term, time)]
        n = self.model.after_step(reward, term, time, env_offset=OFFSET)
        self.dev.after_step(d[0], d[1], d[2], env_offset=OFFSET)
        assert self.dev.differences(self.model) == []
        assert torch.equal(self.whole[self.need:], self.pattern)
        return n, before

    def logged(self, n, before):
        """the n records a step logged, oldest first, read from the DEVICE's log: (world - OFFSET, code)"""
        at = (before + np.arange(n, dtype=np.int64)) % self.C
        return self.dev.log_world.cpu().numpy()[at] - OFFSET, self.dev.log_code.cpu().numpy()[at]

    def counts(self):
        return [int(v) for v in self.dev.counts.cpu().numpy().view(np.uint64)]


def _past_the_block_cap(N):
    chunk, blocks = E.launch_shape(N)
    assert (chunk > E.BLOCK) == (N > E.MAX_BLOCKS * E.BLOCK), (N, chunk, blocks)
    return chunk, blocks


@pytest.mark.parametrize("markers,once", [(False, False), (True, True)], ids=["notime-every", "markers-once"])
@pytest.mark.parametrize("N", [262144, 262145, 524588])
def test_streams_match_the_model_with_several_tiles_per_block(torch, N, markers, once):
    """test_streams_match_the_model_bit_for_bit at the last size with one tile per block (1 024 blocks of 256) and at the
    first sizes with two and three (chunk 512 and 768): four steps at p = 0.02 and at p = 1.0 with C = N, where the log
    wraps inside the step; every buffer, the counters and the schedule compared after every step"""
    chunk, blocks = _past_the_block_cap(N)
    assert (chunk, blocks) == {262144: (256, 1024), 262145: (512, 513), 524588: (768, 684)}[N]
    T = 4
    for p in (0.02, 1.0):
        reward, term, time = E.make_stream(N, T, p, seed=N % 1000 + int(100 * p), markers=markers)
        run = _Run(torch, N, N, once=once)
        for t in range(T):
            run.step(reward[t], term[t], None if time is None else time[t])
        total = int(run.model.counts[0])
        if p == 1.0 and not markers:
            assert total == N * T > N                      # the log wrapped in every step after the first
        if p == 1.0 and once:
            assert total == N == int(run.model.finished.sum())
        assert total > 0


def _rows(N, seed):
    rng = np.random.RandomState(seed)
    reward = (rng.uniform(-1.0, 1.0, (2, N)) * rng.choice([1e-3, 0.37, 11.0], (2, N))).astype(np.float32)
    return rng, reward, rng.randint(1, 4, N).astype(np.uint8)


def _plain_words(run, n, before, term):
    """what the model implies, read from the device: the step's records are its ending worlds in ascending order, and the
    counters by code add up"""
    world, code = run.logged(n, before)
    ending = np.nonzero(term)[0]
    assert n == ending.size and np.array_equal(world, ending) and bool((np.diff(world) > 0).all())
    assert np.array_equal(code, term[ending])
    c = run.counts()
    assert c[1] + c[2] + c[3] == c[0] == before + n


@pytest.mark.parametrize("N", [262145, 524588])
def test_endings_only_behind_the_first_tile_of_a_block(torch, N):
    chunk, _ = _past_the_block_cap(N)
    assert chunk > E.BLOCK
    rng, reward, codes = _rows(N, 1)
    later = np.arange(N) % chunk >= E.BLOCK
    run = _Run(torch, N, N)
    for t in range(2):
        term = np.where(later & (rng.rand(N) < 0.3), codes, 0).astype(np.uint8)
        assert term.any() and not term[~later].any()
        n, before = run.step(reward[t], term)
        _plain_words(run, n, before, term)
    assert int(run.model.counts[0]) > N // 8


@pytest.mark.parametrize("N", [262145, 524588])
def test_only_the_last_world_ends(torch, N):
    chunk, blocks = _past_the_block_cap(N)
    assert chunk > E.BLOCK
    rng, reward, codes = _rows(N, 2)
    run = _Run(torch, N, N)
    for t in range(2):
        term = np.zeros(N, dtype=np.uint8)
        term[N - 1] = codes[t]
        n, before = run.step(reward[t], term)
        assert (n, before) == (1, t)
        _plain_words(run, n, before, term)
    assert (N - 1) // chunk == blocks - 1
    assert run.model.eps_state == 1.0 * 0.9997 * 0.9997


@pytest.mark.parametrize("N", [262145, 524588])
def test_no_ending_in_block_zero_still_advances_the_schedule(torch, N):
    """block 0 advances epsilon by the total of all blocks, also when none of its own worlds ends"""
    chunk, _ = _past_the_block_cap(N)
    assert chunk > E.BLOCK
    rng, reward, codes = _rows(N, 3)
    run = _Run(torch, N, N)
    eps = 1.0
    for t in range(2):
        term = np.where((np.arange(N) >= chunk) & (rng.rand(N) < 0.5), codes, 0).astype(np.uint8)
        assert not term[:chunk].any() and term[chunk:].any()
        n, before = run.step(reward[t], term)
        _plain_words(run, n, before, term)
        eps = max(eps * E.pow_lsb_first(0.9997, n), 0.05)
        assert float(run.dev.eps_state.cpu()[0]) == eps and n > N // 3
    assert eps == 0.05                                       # 0.9997^(N / 3) is far below the floor: held there


@pytest.mark.parametrize("N", [262145, 524588])
def test_the_log_wraps_inside_the_second_tile_of_a_block(torch, N):
    """C = N and a cursor advanced by k worlds: when every world ends, the record of world N - k takes slot 0, and k is
    chosen so that this world sits in the second tile of its block"""
    chunk, _ = _past_the_block_cap(N)
    assert chunk > E.BLOCK
    wrap_at = 5 * chunk + E.BLOCK + 77
    k = N - wrap_at
    assert 0 < k < N and k % E.BLOCK != 0 and E.BLOCK <= wrap_at % chunk < 2 * E.BLOCK
    rng, reward, codes = _rows(N, 4)
    run = _Run(torch, N, N)
    term = np.zeros(N, dtype=np.uint8)
    first = np.sort(rng.permutation(N)[:k])
    term[first] = codes[first]
    n, before = run.step(reward[0], term)
    assert (n, before) == (k, 0)
    _plain_words(run, n, before, term)
    n, before = run.step(reward[1], codes)
    assert (n, before) == (N, k)
    _plain_words(run, n, before, codes)
    log = run.dev.log_world.cpu().numpy() - OFFSET
    assert log[0] == wrap_at and log[N - 1] == wrap_at - 1 and log[k] == 0
    assert bool((run.dev.ret.cpu().numpy() == 0).all()) and bool((run.dev.len.cpu().numpy() == 0).all())


# ================================================================================================ 3. the exploration pass
@pytest.mark.parametrize("tick", [7, (1 << 32) + 5])
def test_exploration_pass_in_its_grid_stride_loop(torch, tick):
    from aquaticgymenv_amd import _episodes_capi as capi
    N, off, seed = STRIDE_N, 3 << 20, 0x1234567890ABCDEF
    assert N > E.EXPLORE_MAX_BLOCKS * E.BLOCK and N % E.BLOCK != 0
    u, drawn = E.draws_vectorised(N, seed, off, tick)
    eps_dev = torch.zeros(1, dtype=torch.float32, device=DEV)
    for eps in (0.3, 1.0):
        eps_dev.fill_(eps)
        action = torch.full((N + 64,), 7, dtype=torch.uint8, device=DEV)
        action[N:] = 9
        rc = capi.lib.aquaep_explore_u8(action.data_ptr(), N, off, eps_dev.data_ptr(), seed, tick, None,
                                        torch.cuda.current_stream().cuda_stream)
        capi.check(rc, "aquaep_explore_u8")
        got = action.cpu().numpy()
        want, explored = E.explore(np.full(N, 7, dtype=np.uint8), eps, u, drawn)
        assert np.array_equal(got[:N], want) and bool((got[N:] == 9).all()), (tick, eps)
        assert bool((got[:N][~explored] == 7).all()) and bool((got[:N][explored] < 3).all())
        assert explored.all() if eps == 1.0 else 0 < int(explored.sum()) < N
        # both trips of the loop explored
        assert explored[:E.EXPLORE_MAX_BLOCKS * E.BLOCK].any() and explored[E.EXPLORE_MAX_BLOCKS * E.BLOCK:].any()


# ================================================================================================ 4. the ring's draw and gather
@pytest.mark.parametrize("bad", [0.0, 0.3])
@pytest.mark.parametrize("size", [7, 1000])
@pytest.mark.parametrize("B", [STRIDE_N, 1 << 20])
def test_draw_in_its_grid_stride_loop(torch, B, size, bad):
    from aquaticgymenv_amd import _replay_capi as xcapi
    capacity, seed, t = 1000, 0x1234567890ABCDEF, 5
    assert xcapi.MAX_BLOCKS * xcapi.BLOCK < B <= xcapi.MAX_BATCH
    ok = (np.random.RandomState(size).rand(capacity) >= bad).astype(np.uint8)
    d_ok = torch.from_numpy(ok).to(DEV)
    header = torch.zeros(4, dtype=torch.int64, device=DEV)
    header[R.SIZE] = size
    t_dev = torch.full((1,), t, dtype=torch.int64, device=DEV)
    idx = torch.full((B + 3,), -77, dtype=torch.int32, device=DEV)
    xcapi.check(xcapi.lib.aquarpl_draw(header.data_ptr(), d_ok.data_ptr(), capacity, t_dev.data_ptr(), seed, idx.data_ptr(), B, None),
                "aquarpl_draw")
    want = L.drawn(seed, t + 1, B, dict(ok=ok, size=size))
    got = idx.cpu().numpy()
    assert np.array_equal(got[:B], want), (B, size, bad)
    assert bool((got[B:] == -77).all()) and int(t_dev[0]) == t              # nothing behind B, the counter is read only
    assert [int(v) for v in header.cpu()] == [0, size, 0, 0]
    tail = want[xcapi.MAX_BLOCKS * xcapi.BLOCK:]
    assert (tail >= 0).any() and len(set(want[want >= 0].tolist())) == int(ok[:size].sum())


@pytest.mark.parametrize("continuous", [False, True], ids=["discrete", "continuous"])
@pytest.mark.parametrize("B", [STRIDE_N, 1 << 20])
def test_gather_in_its_grid_stride_loop(torch, B, continuous):
    from aquaticgymenv_amd import _replay_capi as xcapi
    assert xcapi.MAX_BLOCKS * xcapi.BLOCK < B <= xcapi.MAX_BATCH
    capacity = 333
    model = _filled_model(capacity, 100, 2, seed=6, continuous=continuous)         # 200 slots written, 133 never
    ring = _ring_from(torch, model)
    dead = np.flatnonzero(model.ok[:200] == 0)
    assert dead.size > 0 and (model.ok[200:] == 0).all()
    rng = np.random.RandomState(B % 1000)
    idx = rng.randint(0, 200, B).astype(np.int64)
    kinds = np.array([-1, capacity, dead[0], 250, -2 ** 31, 2 ** 31 - 1, 0, 199], dtype=np.int64)
    for base in (0, xcapi.MAX_BLOCKS * xcapi.BLOCK - 4, B - 8):                    # in the first trip, across the trips, at the end
        idx[base:base + 8] = kinds
    idx = idx.astype(np.int32)
    got = [t.cpu().numpy() for t in ring.gather(torch.from_numpy(idx).to(DEV))]
    want = model.gather(idx)
    for g, w, name in zip(got, want, ("s", "a", "r", "s2", "done", "valid")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), name
    valid = want[5]
    assert list(valid[B - 8:B - 2]) == [0] * 6 and 0.5 * B < int(valid.sum()) < B
    assert not got[0][valid == 0].any() and not got[3][valid == 0].any()
