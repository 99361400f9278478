"""CPU-only checks of libaqua_episodes.so (include/aqua_episodes.h), the episode accounting library: it builds and loads,
exports what its header declares and leaves the other three libraries' interfaces alone, rejects bad arguments before
touching a device, sizes its workspace monotonically, has no CPU path; the numpy model the GPU tests compare against is
itself checked against a per-world loop written the way main/impl/dqn.py:151-186 reads; and the compiled kernels have no
scratch, no spills and no floating-point atomics."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests import _episodes as E
from tests import _isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000            # a "device pointer" for calls that must fail (or return) before anything dereferences it

# every kernel of the gfx950 code object, and the test of tests/test_episodes_gpu.py that launches it
KERNELS = {"ep_account_kernel": "test_streams_match_the_model_bit_for_bit",
           "ep_scatter_kernel": "test_streams_match_the_model_bit_for_bit",
           "ep_explore_kernel": "test_greedy_then_explore_equals_the_epsilon_greedy_kernel"}


@pytest.fixture(scope="module")
def ecapi():
    from aquaticgymenv_amd.build import build_episodes, build_hip, build_learner, build_policy
    assert os.path.exists(build_episodes())
    assert os.path.exists(build_hip()) and os.path.exists(build_policy()) and os.path.exists(build_learner())
    from aquaticgymenv_amd import _episodes_capi
    return _episodes_capi


@pytest.fixture(scope="module")
def isa():
    return _isa.kernels("episodes")


def test_library_builds_loads_and_exports_its_header(ecapi):
    text = open(os.path.join(ROOT, "include", "aqua_episodes.h")).read()
    declared = set(re.findall(r"\b(aquaep_[a-z0-9_]+)\s*\(", text))
    assert declared == set(ecapi.SYMBOLS), declared ^ set(ecapi.SYMBOLS)
    raw = ctypes.CDLL(ecapi.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    assert ecapi.lib.aquaep_version() == ecapi.ABI_VERSION == 1

    def define(name):
        return int(re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, text).group(1))
    assert define("AQUAEP_ABI_VERSION") == 1
    assert [define("AQUAEP_E_" + n) for n in ("INVALID", "ALIGN", "NODEVICE")] == [-1, -2, -3]
    assert [ecapi.E_INVALID, ecapi.E_ALIGN, ecapi.E_NODEVICE] == [-1, -2, -3]
    assert define("AQUAEP_MAX_WORLDS") == ecapi.MAX_WORLDS >= 1 << 28
    assert define("AQUAEP_MAX_BLOCKS") == ecapi.MAX_BLOCKS and define("AQUAEP_COUNTS") == ecapi.COUNTS == 8
    from aquaticgymenv_amd import _policy_capi
    assert define("AQUAEP_STREAM") == ecapi.STREAM == E.STREAM == _policy_capi.STREAM == 5


def test_the_other_three_bindings_are_unchanged(ecapi):
    from aquaticgymenv_amd import _capi, _learner_capi, _policy_capi
    assert len(_capi.SYMBOLS) == 38 and len(_policy_capi.SYMBOLS) == 5 and len(_learner_capi.SYMBOLS) == 4
    for other in ("aqua_hip.h", "aqua_policy.h", "aqua_learner.h"):
        assert "aquaep_" not in open(os.path.join(ROOT, "include", other)).read().lower()
    for name in ecapi.SYMBOLS:
        assert not hasattr(_capi.lib, name) and not hasattr(_policy_capi.lib, name) and not hasattr(_learner_capi.lib, name)
    for other in (_capi, _policy_capi, _learner_capi):
        assert not any(s.startswith("aquaep_") for s in other.SYMBOLS)


def test_build_recipe_is_separate_from_the_other_libraries():
    from aquaticgymenv_amd import build
    assert len({build.LIB, build.POLICY_LIB, build.LEARNER_LIB, build.EPISODES_LIB}) == 4
    assert "-cuid=aqua_episodes" in build.EPISODES_FLAGS
    assert [f for f in build.EPISODES_FLAGS if f.startswith("-cuid")] == ["-cuid=aqua_episodes"]
    plain = sorted(f for f in build.COMMON_FLAGS if not f.startswith("-cuid"))
    assert sorted(f for f in build.EPISODES_FLAGS if not f.startswith("-cuid")) == plain
    assert not set(build.EPISODES_SRC) & (set(build.SRC) | set(build.POLICY_SRC) | set(build.LEARNER_SRC))
    assert set(build.EPISODES_SRC) <= set(build.EPISODES_DEPS)
    assert os.path.join(ROOT, "include", "aqua_episodes.h") in build.EPISODES_DEPS
    assert callable(build.episodes_needs_build) and build.episodes_needs_build() in (True, False)


def _after(lib, **kw):
    a = dict(reward=FAKE, term=FAKE, time=FAKE, env_offset=0, N=1000, ret=FAKE + 0x10000, len=FAKE + 0x20000, finished=None,
             log_ret=FAKE + 0x30000, log_len=FAKE + 0x40000, log_code=FAKE + 0x50000, log_world=FAKE + 0x60000, C=1000,
             counts=FAKE + 0x70000, eps_state=FAKE + 0x80000, eps_out=FAKE + 0x90000, decay=0.9997, eps_final=0.05,
             ws=FAKE, ws_bytes=1 << 20)
    a.update(kw)
    return lib.aquaep_after_step_f32(a["reward"], a["term"], a["time"], a["env_offset"], a["N"], a["ret"], a["len"], a["finished"],
                                     a["log_ret"], a["log_len"], a["log_code"], a["log_world"], a["C"], a["counts"], a["eps_state"],
                                     a["eps_out"], a["decay"], a["eps_final"], a["ws"], a["ws_bytes"], None)


def test_argument_validation_without_touching_a_device(ecapi):
    lib = ecapi.lib
    nan, inf = float("nan"), float("inf")
    invalid = [dict(reward=None), dict(term=None), dict(ret=None), dict(len=None), dict(log_ret=None), dict(log_len=None),
               dict(log_code=None), dict(log_world=None), dict(counts=None), dict(ws=None), dict(C=999), dict(C=0), dict(N=-1),
               dict(N=ecapi.MAX_WORLDS + 1, C=ecapi.MAX_WORLDS + 1), dict(env_offset=-1),
               dict(decay=0.0), dict(decay=-0.5), dict(decay=1.0000001), dict(decay=nan), dict(decay=inf),
               dict(eps_final=-0.01), dict(eps_final=nan), dict(eps_state=None), dict(eps_out=None),
               dict(ws_bytes=lib.aquaep_workspace_bytes(1000) - 1), dict(ws_bytes=0)]
    for kw in invalid:
        assert _after(lib, **kw) == ecapi.E_INVALID, kw
        assert lib.aquaep_last_error().decode(), kw
    misaligned = [dict(reward=FAKE + 2), dict(time=FAKE + 1), dict(ret=FAKE + 0x10002), dict(len=FAKE + 0x20001),
                  dict(log_ret=FAKE + 0x30002), dict(log_len=FAKE + 0x40003), dict(log_world=FAKE + 0x60004),
                  dict(counts=FAKE + 0x70004), dict(eps_state=FAKE + 0x80004), dict(eps_out=FAKE + 0x90002), dict(ws=FAKE + 8)]
    for kw in misaligned:
        assert _after(lib, **kw) == ecapi.E_ALIGN, kw
        assert lib.aquaep_last_error().decode(), kw
    # N == 0: nothing to do, no launch, no device, neither inputs nor workspace needed; the schedule may be off
    assert _after(lib, N=0) == 0
    assert _after(lib, N=0, reward=None, term=None, time=None, ws=None, ws_bytes=0, C=0) == 0
    assert _after(lib, N=0, eps_state=None, eps_out=None) == 0
    # the exploration pass
    ex = lib.aquaep_explore_u8
    assert ex(FAKE, 0, 0, FAKE, 1, 2, None, None) == 0 and ex(None, 0, 0, FAKE, 1, 2, FAKE, None) == 0
    for args in ((None, 10, 0, FAKE, 1, 2, None, None), (FAKE, -1, 0, FAKE, 1, 2, None, None), (FAKE, 10, -1, FAKE, 1, 2, None, None),
                 (FAKE, 10, 0, None, 1, 2, None, None), (FAKE, ecapi.MAX_WORLDS + 1, 0, FAKE, 1, 2, None, None)):
        assert ex(*args) == ecapi.E_INVALID, args
        assert lib.aquaep_last_error().decode(), args
    for args in ((FAKE, 10, 0, FAKE + 2, 1, 2, None, None), (FAKE, 10, 0, FAKE, 1, 2, FAKE + 4, None)):
        assert ex(*args) == ecapi.E_ALIGN, args


def test_workspace_grows_with_the_batch(ecapi):
    lib = ecapi.lib
    ns = list(range(0, 2100)) + [2 ** k + d for k in range(12, 31) for d in (-1, 0, 1) if 2 ** k + d <= ecapi.MAX_WORLDS]
    sizes = [lib.aquaep_workspace_bytes(n) for n in ns]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[1] >= 4 and sizes[-1] > sizes[1]
    assert all(s % 16 == 0 and s > 0 for s in sizes) and sizes[-1] == 4 * ecapi.MAX_BLOCKS
    assert lib.aquaep_workspace_bytes(-1) == 0 and lib.aquaep_workspace_bytes(ecapi.MAX_WORLDS + 1) == 0


def test_no_cpu_fallback_for_the_tracker(ecapi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from aquaticgymenv_amd.episodes import EpisodeTracker
    for device in ("cuda:0", "cpu"):
        env = types.SimpleNamespace(torch=torch, device=torch.device(device), num_envs=8, env_offset=0, continuous=False)
        with pytest.raises(RuntimeError):
            EpisodeTracker(env)
    src = open(os.path.join(ROOT, "aquaticgymenv_amd", "episodes.py")).read()
    assert "torch.where" not in src and "cumsum" not in src and ".sum(" not in src


@pytest.mark.parametrize("markers,once", [(False, False), (True, False), (False, True), (True, True)])
def test_the_model_is_the_per_world_loop_of_the_reference(markers, once):
    N, T, C, eps = 23, 60, 512, (1.0, 0.05, 0.97)
    reward, term, time = E.make_stream(N, T, 0.15, seed=5, markers=markers)
    if markers:                                               # the stream exercises what it is for
        assert ((term == 0) & (time < 0)).sum() > 20
        waited = [(t, w) for t in range(1, T - 1) for w in range(N)
                  if term[t - 1, w] != 0 and time[t, w] == time[t - 1, w] and time[t + 1, w] <= -3]
        assert waited, "no world waits two ticks for its restart"
    model = E.Model(N, C, once=once, eps=eps)
    order, eps_seen = [], []
    for t in range(T):
        n = model.after_step(reward[t], term[t], None if time is None else time[t], env_offset=100)
        order += [t] * n
        eps_seen += [model.eps_state] * n
    records, epsilons = E.naive_loop(reward, term, time, once, eps)
    assert len(records) == int(model.counts[0]) > (N if not once else 10) and len(records) <= C
    if once:
        assert len(records) <= N and int(model.finished.sum()) == len(records)
    k = len(records)
    assert [r[0] for r in records] == order
    assert np.array_equal(model.log_world[:k], 100 + np.array([r[1] for r in records]))
    assert np.array_equal(model.log_ret[:k].view(np.uint32), np.array([r[2] for r in records], dtype=np.float32).view(np.uint32))
    assert np.array_equal(model.log_len[:k], [r[3] for r in records]) and np.array_equal(model.log_code[:k], [r[4] for r in records])
    assert [int(model.counts[c]) for c in (1, 2, 3)] == [sum(1 for r in records if r[4] == c) for c in (1, 2, 3)]
    counted = np.ones_like(term, dtype=bool) if time is None else ((term != 0) | (time >= 0))
    if not once:
        assert int(model.counts[4]) == int(counted.sum())
    # epsilon after the last episode of every step: n applications of dqn.py:184 within 1e-12 relative
    for i in range(k):
        if i + 1 == k or order[i + 1] != order[i]:
            assert abs(eps_seen[i] - epsilons[i]) <= 1e-12 * epsilons[i], (i, eps_seen[i], epsilons[i])
    assert model.eps_out == np.float32(model.eps_state)


def test_the_model_schedule_is_n_applications_of_the_reference_rule():
    for init, final, decay, n in ((1.0, 0.05, 10000, 3000), (1.0, 0.05, 0.9997, 20000), (0.8, 0.1, 0.5, 7), (1.0, 0.05, 1.0, 50)):
        d = E.eps_decay(init, final, decay)
        assert d == (decay if decay < 1 else (final / init) ** (1 / decay))
        epsilon = init
        for _ in range(n):
            epsilon = max(epsilon * d, final)
        got = max(init * E.pow_lsb_first(d, n), final)
        assert abs(got - epsilon) <= 1e-12 * epsilon, (init, final, decay, n, got, epsilon)
    assert E.pow_lsb_first(0.5, 0) == 1.0 and E.pow_lsb_first(0.5, 5) == 0.5 ** 5


def test_codegen_has_no_scratch_no_spills_and_no_float_atomics(isa):
    names = {n: [k for k in KERNELS if k in n] for n in isa}
    assert all(len(v) == 1 for v in names.values()) and len(isa) == len(KERNELS) == 3, sorted(isa)
    assert {v[0] for v in names.values()} == set(KERNELS)
    gpu_tests = open(os.path.join(ROOT, "tests", "test_episodes_gpu.py")).read()
    for kernel, test in KERNELS.items():
        assert re.search(r"^def %s\(" % test, gpu_tests, re.M), (kernel, test)
    for name, k in isa.items():
        m = k["meta"]
        assert m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert "scratch_" not in k["body"], name
        assert not re.search(r"atomic_\w*(f32|f64)|atomic_(fadd|fmin|fmax|pk_add)", k["body"]), name      # no float atomics
        assert m["group_segment_fixed_size"] <= 1024, (name, m)
        assert "s_sleep" not in k["body"] and "buffer_wbl2" not in k["body"], name        # no spin, no fence: nothing waits
    account = [k for n, k in isa.items() if "ep_account_kernel" in n][0]
    scatter = [k for n, k in isa.items() if "ep_scatter_kernel" in n][0]
    assert re.search(r"global_atomic_add_(x2|u64)", account["body"]) and "global_atomic" not in scatter["body"]
    assert "s_bcnt1_i32_b64" in account["body"] and "v_mbcnt_hi_u32_b32" in scatter["body"]     # ballot + popcount, rank
