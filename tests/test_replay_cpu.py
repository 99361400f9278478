"""CPU-only checks of libaqua_replay.so (include/aqua_replay.h), the experience ring with a device cursor: it builds and
loads, exports what its header declares, rejects bad arguments before touching a device, has a build-table entry of its own
that leaves the pinned tables alone, and has no CPU path; the numpy model the GPU tests compare against is itself checked
against a per-world loop written the way main/impl/dqn.py:174 appends; and the compiled kernels have no scratch, no
spills, no LDS and no floating-point atomics."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests import _isa
from tests import _replay as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000            # a "device pointer" for calls that must fail (or return) before anything dereferences it

# every kernel of the gfx950 code object, and the test of tests/test_replay_gpu.py that launches it
KERNELS = {"rpl_open_kernel": "test_append_matches_the_model_after_every_pair",
           "rpl_close_kernel": "test_append_matches_the_model_after_every_pair",
           "rpl_draw_kernel": "test_draw_is_the_learners_own_draw",
           "rpl_gather_kernel": "test_gather_equals_numpy_indexing"}


@pytest.fixture(scope="module")
def xcapi():
    from aquaticgymenv_amd.build import build_library
    assert os.path.exists(build_library("replay"))
    from aquaticgymenv_amd import _replay_capi
    return _replay_capi


@pytest.fixture(scope="module")
def isa():
    return _isa.kernels("replay")


def test_library_builds_loads_and_exports_its_header(xcapi):
    text = open(os.path.join(ROOT, "include", "aqua_replay.h")).read()
    declared = set(re.findall(r"\b(aquarpl_[a-z0-9_]+)\s*\(", text))
    assert declared == set(xcapi.SYMBOLS), declared ^ set(xcapi.SYMBOLS)
    raw = ctypes.CDLL(xcapi.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    assert xcapi.lib.aquarpl_version() == xcapi.ABI_VERSION == 1
    assert set(xcapi._SIGNATURES) == set(xcapi.SYMBOLS) - {"aquarpl_version", "aquarpl_last_error"}

    def define(name):
        return int(re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, text).group(1))
    assert define("AQUARPL_ABI_VERSION") == 1
    assert [define("AQUARPL_E_" + n) for n in ("INVALID", "ALIGN", "NODEVICE")] == [-1, -2, -3]
    assert [xcapi.E_INVALID, xcapi.E_ALIGN, xcapi.E_NODEVICE] == [-1, -2, -3]
    assert define("AQUARPL_HEADER_WORDS") == xcapi.HEADER_WORDS == R.HEADER_WORDS == 4
    assert define("AQUARPL_MAX_CAPACITY") == xcapi.MAX_CAPACITY == 2 ** 31 - 1
    assert define("AQUARPL_MAX_BLOCKS") == xcapi.MAX_BLOCKS and define("AQUARPL_BLOCK") == xcapi.BLOCK == 256
    assert define("AQUARPL_ATTEMPTS") == xcapi.ATTEMPTS == 4
    assert [define("AQUARPL_ACT_U8"), define("AQUARPL_ACT_F32X2")] == [xcapi.ACT_U8, xcapi.ACT_F32X2] == [0, 1]
    from aquaticgymenv_amd import _learner_capi
    from tests import _learner
    assert define("AQUARPL_STREAM") == xcapi.STREAM == _learner_capi.STREAM == _learner.STREAM == 6
    assert define("AQUARPL_MAX_BATCH") == xcapi.MAX_BATCH == _learner_capi.MAX_BATCH


def test_the_other_bindings_do_not_know_the_new_symbols(xcapi):
    from aquaticgymenv_amd import _capi, _episodes_capi, _learner_capi, _policy_capi, _render_capi
    for other in (_capi, _policy_capi, _learner_capi, _episodes_capi, _render_capi):
        assert not any(s.startswith("aquarpl_") for s in other.SYMBOLS)
        for name in xcapi.SYMBOLS:
            assert not hasattr(other.lib, name)
    for other in ("aqua_hip.h", "aqua_policy.h", "aqua_learner.h", "aqua_episodes.h", "aqua_render.h"):
        assert "aquarpl_" not in open(os.path.join(ROOT, "include", other)).read().lower()


def test_build_table_entry_and_the_pinned_tables():
    from aquaticgymenv_amd import build
    assert list(build.LIBRARIES) == ["hip", "policy", "learner", "episodes"] and set(build.EXTRA_LIBRARIES) == {"render"}
    assert build.all_libraries() == ["hip", "policy", "learner", "episodes", "render"]
    assert list(build.ADDON_LIBRARIES) == ["replay"]
    assert build.every_library() == build.all_libraries() + ["replay"]
    entry = build.library("replay")
    assert entry is build.ADDON_LIBRARIES["replay"]
    assert build.library("hip") is build.LIBRARIES["hip"] and build.library("render") is build.EXTRA_LIBRARIES["render"]
    with pytest.raises(KeyError):
        build.library("nothing")
    csrc = os.path.join(ROOT, "aquaticgymenv_amd", "csrc")
    src = os.path.join(csrc, "aqua_replay.hip")
    lib = os.path.join(ROOT, "aquaticgymenv_amd", "lib", "libaqua_replay.so")
    assert entry["src"] == [src] and entry["lib"] == lib and entry["cuid"] == "aqua_replay"
    assert entry["deps"] == [src] + [os.path.join(csrc, h) for h in ("aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp")] + \
        [os.path.join(ROOT, "include", "aqua_replay.h")]
    assert all(os.path.exists(p) for p in entry["deps"])
    # the command line, token by token: the common one with the library's own compilation-unit id
    assert build.build_command("replay") == [
        build.hipcc_path(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-fno-honor-nans", "-cuid=aqua_replay",
        "-Wall", "-Wno-unused-function", "-o", lib + ".tmp", src]
    assert (build.REPLAY_SRC, build.REPLAY_DEPS, build.REPLAY_LIB, build.REPLAY_FLAGS) == \
        (entry["src"], entry["deps"], entry["lib"], entry["flags"])
    assert callable(build.build_replay) and build.replay_needs_build() in (True, False)
    included = set(re.findall(r'#include "([a-z_]+\.hpp)"', open(src).read()))
    assert included == {"aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp"}


def test_graft_entry_builds_and_checks_every_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "every_library()" in text and "_replay_capi" in text and "aquarpl_version" in text


def _open(lib, **kw):
    a = dict(header=FAKE, s=FAKE + 0x1000, a=FAKE + 0x2000, ok=FAKE + 0x3000, ring_ld=1000, capacity=1000, obs=FAKE + 0x4000,
             obs_ld=512, action=FAKE + 0x5000, kind=0, action_ld=512, time=FAKE + 0x6000, N=500)
    a.update(kw)
    return lib.aquarpl_open(a["header"], a["s"], a["a"], a["ok"], a["ring_ld"], a["capacity"], a["obs"], a["obs_ld"], a["action"],
                            a["kind"], a["action_ld"], a["time"], a["N"], None)


def _close(lib, **kw):
    a = dict(header=FAKE, r=FAKE + 0x1000, s2=FAKE + 0x2000, d=FAKE + 0x3000, ring_ld=1000, capacity=1000, reward=FAKE + 0x4000,
             obs=FAKE + 0x5000, obs_ld=512, term=FAKE + 0x6000, N=500)
    a.update(kw)
    return lib.aquarpl_close(a["header"], a["r"], a["s2"], a["d"], a["ring_ld"], a["capacity"], a["reward"], a["obs"], a["obs_ld"],
                             a["term"], a["N"], None)


def _draw(lib, **kw):
    a = dict(header=FAKE, ok=FAKE + 0x1000, capacity=1000, t=FAKE + 0x2000, seed=3, idx=FAKE + 0x3000, B=64)
    a.update(kw)
    return lib.aquarpl_draw(a["header"], a["ok"], a["capacity"], a["t"], a["seed"], a["idx"], a["B"], None)


def _gather(lib, **kw):
    a = dict(idx=FAKE, B=64, s=FAKE + 0x1000, a=FAKE + 0x2000, r=FAKE + 0x3000, s2=FAKE + 0x4000, d=FAKE + 0x5000, ok=FAKE + 0x6000,
             ring_ld=1000, capacity=1000, kind=0, out_s=FAKE + 0x7000, out_a=FAKE + 0x8000, out_r=FAKE + 0x9000,
             out_s2=FAKE + 0xA000, out_done=FAKE + 0xB000, out_valid=FAKE + 0xC000)
    a.update(kw)
    return lib.aquarpl_gather(a["idx"], a["B"], a["s"], a["a"], a["r"], a["s2"], a["d"], a["ok"], a["ring_ld"], a["capacity"],
                              a["kind"], a["out_s"], a["out_a"], a["out_r"], a["out_s2"], a["out_done"], a["out_valid"], None)


def test_argument_validation_without_touching_a_device(xcapi):
    lib = xcapi.lib
    big = xcapi.MAX_CAPACITY + 1
    cases = [
        (_open, [dict(header=None), dict(s=None), dict(a=None), dict(ok=None), dict(obs=None), dict(action=None),
                 dict(N=1001), dict(N=-1), dict(ring_ld=999), dict(obs_ld=499), dict(capacity=0, N=0), dict(capacity=-5, N=0),
                 dict(capacity=big, ring_ld=big), dict(kind=2), dict(kind=-1), dict(kind=1, action_ld=499)],
         [dict(header=FAKE + 4), dict(s=FAKE + 0x1002), dict(obs=FAKE + 0x4001), dict(time=FAKE + 0x6002),
          dict(kind=1, a=FAKE + 0x2002), dict(kind=1, action=FAKE + 0x5001)]),
        (_close, [dict(header=None), dict(r=None), dict(s2=None), dict(d=None), dict(reward=None), dict(obs=None), dict(term=None),
                  dict(N=1001), dict(N=-1), dict(ring_ld=999), dict(obs_ld=499), dict(capacity=0, N=0), dict(capacity=big, ring_ld=big)],
         [dict(header=FAKE + 4), dict(r=FAKE + 0x1002), dict(s2=FAKE + 0x2001), dict(reward=FAKE + 0x4002), dict(obs=FAKE + 0x5003)]),
        (_draw, [dict(header=None), dict(ok=None), dict(t=None), dict(idx=None), dict(B=-1), dict(B=xcapi.MAX_BATCH + 1),
                 dict(capacity=0), dict(capacity=big)],
         [dict(header=FAKE + 4), dict(t=FAKE + 0x2004), dict(idx=FAKE + 0x3002)]),
        (_gather, [dict(idx=None), dict(s=None), dict(a=None), dict(r=None), dict(s2=None), dict(d=None), dict(ok=None),
                   dict(out_s=None), dict(out_a=None), dict(out_r=None), dict(out_s2=None), dict(out_done=None), dict(out_valid=None),
                   dict(B=-1), dict(B=xcapi.MAX_BATCH + 1), dict(ring_ld=999), dict(capacity=0), dict(kind=7)],
         [dict(idx=FAKE + 2), dict(s=FAKE + 0x1001), dict(out_s2=FAKE + 0xA002), dict(kind=1, out_a=FAKE + 0x8002)]),
    ]
    for call, invalid, misaligned in cases:
        for kw in invalid:
            assert call(lib, **kw) == xcapi.E_INVALID, (call.__name__, kw)
            assert lib.aquarpl_last_error().decode(), (call.__name__, kw)
        for kw in misaligned:
            assert call(lib, **kw) == xcapi.E_ALIGN, (call.__name__, kw)
            assert lib.aquarpl_last_error().decode(), (call.__name__, kw)
    # nothing to do: no launch, no device, the inputs are not needed
    assert _open(lib, N=0, obs=None, action=None, time=None) == 0 and _close(lib, N=0, reward=None, obs=None, term=None) == 0
    assert _draw(lib, B=0, idx=None) == 0 and _gather(lib, B=0, idx=None, out_s=None, out_valid=None) == 0
    # the Python layer turns E_INVALID into ValueError and everything else into the binding's error
    with pytest.raises(ValueError):
        xcapi.check(_open(lib, N=1001), "aquarpl_open")
    with pytest.raises(xcapi.AquaReplayError):
        xcapi.check(_open(lib, header=FAKE + 4), "aquarpl_open")


def test_no_cpu_fallback_for_the_ring_and_the_loop(xcapi):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from aquaticgymenv_amd.replay import DeviceReplayRing
    from aquaticgymenv_amd.trainer import DQNLoop
    for device in ("cuda:0", "cpu"):
        env = types.SimpleNamespace(torch=torch, device=torch.device(device), num_envs=8, env_offset=0, continuous=False, ld=64,
                                    obs_norm_buf=object())
        with pytest.raises(RuntimeError):
            DeviceReplayRing(env, 64)
    # the loop is made of the facades, each of which has no CPU path; with none of them constructible it rejects its parts
    env = types.SimpleNamespace(torch=torch, device=torch.device("cpu"), continuous=False, obs_norm_buf=None)
    with pytest.raises(ValueError):
        DQNLoop(env, None, None, None, None, 64)
    for name in ("replay.py", "trainer.py"):
        src = open(os.path.join(ROOT, "aquaticgymenv_amd", name)).read()
        assert "torch.where" not in src and "index_select" not in src and "randint" not in src.split("class DeviceReplayRing")[-1]


@pytest.mark.parametrize("continuous", [False, True], ids=["discrete", "continuous"])
@pytest.mark.parametrize("with_time", [True, False], ids=["markers", "notime"])
def test_the_model_is_the_per_world_append_of_the_reference(continuous, with_time):
    rng = np.random.RandomState(11)
    capacity, model, batches = 53, R.Model(53, ring_ld=60, continuous=continuous, fill=0), []
    for n in (20, 1, 20, 53, 7, 20, 19):
        b = R.make_batch(rng, n, n + 5, continuous=continuous, with_time=with_time)
        model.open(b["obs"], b["action"], b["time"], n)
        assert model.header[R.BASE] == model.header[R.CURSOR]
        model.close(b["reward"], b["obs2"], b["term"], n)
        batches.append((b["obs"], b["action"], b["time"], b["reward"], b["obs2"], b["term"], n))
    slots, cursor, size = R.naive_loop(batches, capacity)
    assert list(model.header) == [cursor, size, (cursor - 19) % capacity, 7] and size == capacity and all(s is not None for s in slots)
    for c, (s, a, r, s2, d, ok) in enumerate(slots):
        assert tuple(model.s[:, c]) == s and tuple(model.s2[:, c]) == s2 and float(model.r[c]) == r
        assert (tuple(model.a[:, c]) if continuous else int(model.a[c])) == a
        assert int(model.d[c]) == d and int(model.ok[c]) == ok
    for row in (model.s, model.s2, model.r, model.d, model.ok, model.a):
        assert not row[..., capacity:].any()                 # nothing behind the capacity, none of the poison anywhere
        assert not (np.abs(row.astype(np.float64)) > 1e30).any()
    if with_time:
        assert 0 < int(model.ok[:capacity].sum()) < capacity
        assert np.array_equal(R.live(np.array([5, 0, -1, -2, -3, -4], dtype=np.int32), 6), [1, 1, 0, 0, 1, 1])
    else:
        assert int(model.ok[:capacity].sum()) == capacity
    # an invalid base: nothing moves
    before = {k: getattr(model, k).copy() for k in R.ROWS}
    model.header[R.BASE] = -1
    header = model.header.copy()
    model.close(b["reward"], b["obs2"], b["term"], 19)
    assert np.array_equal(model.header, header) and all(np.array_equal(getattr(model, k), before[k]) for k in R.ROWS)


def test_the_model_draw_and_gather():
    rng = np.random.RandomState(2)
    model = R.Model(40)
    assert np.array_equal(model.draw(5, 0, 16), np.full(16, -1))          # an empty ring gives no sample
    for _ in range(3):
        b = R.make_batch(rng, 12, 12)
        model.open(b["obs"], b["action"], b["time"], 12)
        model.close(b["reward"], b["obs2"], b["term"], 12)
    idx = model.draw(5, 3, 200)
    assert idx.dtype == np.int32 and ((idx >= -1) & (idx < 36)).all() and (model.ok[idx[idx >= 0]] != 0).all() and (idx >= 0).sum() > 100
    probe = np.array([-1, 40, 39, 0, int(np.flatnonzero(model.ok[:36] == 0)[0]), int(idx[idx >= 0][0])], dtype=np.int32)
    s, a, r, s2, done, valid = model.gather(probe)
    assert list(valid) == [0, 0, 0, int(model.ok[0]), 0, 1]
    assert not s[valid == 0].any() and not s2[valid == 0].any() and not r[valid == 0].any() and not done[valid == 0].any()
    j = int(probe[5])
    assert np.array_equal(s[5], model.s[:, j]) and np.array_equal(s2[5], model.s2[:, j]) and r[5] == model.r[j] and a[5] == model.a[j]
    assert done[5] == (model.d[j] != 0)


def test_codegen_has_no_scratch_no_spills_no_lds_and_no_atomics(isa):
    names = {n: [k for k in KERNELS if k in n] for n in isa}
    assert all(len(v) == 1 for v in names.values()) and len(isa) == len(KERNELS) == 4, sorted(isa)
    assert {v[0] for v in names.values()} == set(KERNELS)
    gpu_tests = open(os.path.join(ROOT, "tests", "test_replay_gpu.py")).read()
    for kernel, test in KERNELS.items():
        assert re.search(r"^def %s\(" % test, gpu_tests, re.M), (kernel, test)
    for name, k in isa.items():
        m = k["meta"]
        assert m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert "scratch_" not in k["body"], name
        assert m["group_segment_fixed_size"] == 0, (name, m)                       # no LDS planned
        assert not re.search(r"atomic_\w*(f32|f64)|atomic_(fadd|fmin|fmax|pk_add)", k["body"]), name      # no float atomics
        assert "global_atomic" not in k["body"] and "ds_" not in k["body"], name   # no atomics at all, no LDS traffic
        assert "s_sleep" not in k["body"] and "buffer_wbl2" not in k["body"], name # no spin, no fence: nothing waits
        assert not re.search(r"\bv_(add|mul|fma|mac|sub)_f(16|32|64)\b", k["body"]), name     # copies and integer draws only
