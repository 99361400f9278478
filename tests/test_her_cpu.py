"""CPU-only checks of libaqua_her.so (aquaticgymenv_amd/csrc/aqua_her.h), hindsight relabelling of the experience ring: it
builds and loads, exports what its header declares, rejects bad arguments before touching a device and names the field, has a
build-table entry of its own behind the pinned ones and a Philox stream of its own, and has no CPU path; aquaher_threshold is
floor(ratio 2^32); aquaher_reward -- the kernel's own code on the host -- equals the numpy model bit for bit and the reference's
own rewards and termination codes (tests/golden/step_golden.npz) within the float32 rounding of the observation; the model the
GPU tests compare against (tests/_her_model.py) is itself checked on hand-made rings and against a per-world restatement; and
the compiler's resource metadata of the kernel shows no scratch and no spills."""
import ctypes
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from tests import _golden
from tests import _her_model as M
from tests import _isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aquaticgymenv_amd", "csrc")
HEADER = os.path.join(CSRC, "aqua_her.h")
FAKE = 0x10000            # a "device pointer" for calls that must fail (or return) before anything dereferences it


@pytest.fixture(scope="module")
def capi():
    from aquaticgymenv_amd.build import build_library
    assert os.path.exists(build_library("her"))
    from aquaticgymenv_amd import _her_capi
    return _her_capi


# ------------------------------------------------------------------------------------------------ the library and its table
def test_library_builds_loads_and_exports_its_header(capi):
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(aquaher_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(capi.SYMBOLS) == {"aquaher_version", "aquaher_last_error", "aquaher_threshold", "aquaher_reward",
                                            "aquaher_relabel"}, declared ^ set(capi.SYMBOLS)
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    assert capi.lib.aquaher_version() == capi.ABI_VERSION == 1
    assert set(capi._SIGNATURES) == set(capi.SYMBOLS) - {"aquaher_version", "aquaher_last_error"}

    def define(name):
        return int(re.search(r"#define\s+%s\s+\(?(-?\d+)" % name, text).group(1))
    assert define("AQUAHER_ABI_VERSION") == 1
    assert [define("AQUAHER_E_" + n) for n in ("INVALID", "ALIGN", "NODEVICE")] == [-1, -2, -3] == [capi.E_INVALID, capi.E_ALIGN, capi.E_NODEVICE]
    from aquaticgymenv_amd import _capi, _lbank_capi, _nstep_capi, _replay_capi
    assert define("AQUAHER_MAX_HORIZON") == capi.MAX_HORIZON == M.MAX_HORIZON == 64 and define("AQUAHER_CHUNK") == capi.CHUNK == _nstep_capi.CHUNK
    assert capi.MAX_HORIZON % capi.CHUNK == 0
    assert define("AQUAHER_MAX_CAPACITY") == capi.MAX_CAPACITY == _replay_capi.MAX_CAPACITY
    assert define("AQUAHER_MAX_NETWORKS") == capi.MAX_NETWORKS == _lbank_capi.MAX_NETWORKS == 4096
    assert define("AQUAHER_MAX_BATCH") == capi.MAX_BATCH == _replay_capi.MAX_BATCH == 1048576
    assert define("AQUAHER_MAX_BLOCKS") == capi.MAX_BLOCKS == _replay_capi.MAX_BLOCKS and define("AQUAHER_BLOCK") == capi.BLOCK == _replay_capi.BLOCK
    assert [define("AQUAHER_ACT_U8"), define("AQUAHER_ACT_F32X2")] == [capi.ACT_U8, capi.ACT_F32X2] == [_replay_capi.ACT_U8, _replay_capi.ACT_F32X2]
    assert define("AQUAHER_NO_SEED") == capi.NO_SEED == 0
    assert define("AQUAHER_TERM_SUCCESS") == capi.TERM_SUCCESS == M.TERM_SUCCESS == _capi.TERM_SUCCESS == 3
    if shutil.which("nm"):
        nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True)
        assert nm.returncode == 0 and set(re.findall(r"\b(aquaher_\w+)", nm.stdout)) == declared


def test_the_stream_is_eight_and_nobody_elses(capi):
    text = open(HEADER).read()
    assert int(re.search(r"#define\s+AQUAHER_STREAM\s+(\d+)", text).group(1)) == capi.STREAM == M.STREAM == 8
    from aquaticgymenv_amd import (_bank_capi, _episodes_capi, _fastpol_capi, _lbank_capi, _learner_capi, _pbt_capi, _policy_capi, _prio_capi,
                                   _replay_capi)
    taken = {m.__name__: m.STREAM for m in (_bank_capi, _episodes_capi, _fastpol_capi, _lbank_capi, _learner_capi, _pbt_capi, _policy_capi,
                                            _prio_capi, _replay_capi)}
    assert set(taken.values()) == {5, 6, 7}, taken
    # the streams of the environment itself (aqua_device.hpp) and every stream a header or a source of csrc/ and include/ names
    device = open(os.path.join(CSRC, "aqua_device.hpp")).read()
    env_streams = re.search(r"enum : uint32_t \{ STREAM_STEP = (\d+), STREAM_PLACE = (\d+), STREAM_POSE = (\d+), STREAM_ACT = (\d+) \}", device)
    assert sorted(int(v) for v in env_streams.groups()) == [0, 1, 3, 4]
    named = {}
    for folder in (CSRC, os.path.join(ROOT, "include"), os.path.join(ROOT, "aquaticgymenv_amd", "include")):
        for name in sorted(os.listdir(folder)):
            for macro, value in re.findall(r"#define\s+(AQUA[A-Z]*_STREAM)\s+(\d+)", open(os.path.join(folder, name)).read()):
                named[macro] = int(value)
            for const, value in re.findall(r"constexpr uint32_t (STREAM_[A-Z]+) = (\d+);", open(os.path.join(folder, name)).read()):
                named[const] = int(value)
    assert named["AQUAHER_STREAM"] == 8 and [k for k, v in named.items() if v == 8] == ["AQUAHER_STREAM"], named
    assert len(named) >= 8


def test_the_other_bindings_do_not_know_the_new_symbols(capi):
    from aquaticgymenv_amd import (_bank_capi, _capi, _episodes_capi, _fastpol_capi, _lbank_capi, _learner_capi, _nstep_capi, _pbt_capi,
                                   _policy_capi, _prio_capi, _qmap_capi, _render_capi, _replay_capi, _segments_capi)
    others = (_capi, _policy_capi, _learner_capi, _episodes_capi, _render_capi, _replay_capi, _bank_capi, _lbank_capi, _segments_capi,
              _pbt_capi, _qmap_capi, _fastpol_capi, _nstep_capi, _prio_capi)
    for other in others:
        assert not any(s.startswith("aquaher_") for s in other.SYMBOLS)
        for name in capi.SYMBOLS:
            assert not hasattr(other.lib, name)


def test_build_table_entry_behind_the_pinned_tables():
    from aquaticgymenv_amd import build
    assert list(build.HINDSIGHT_LIBRARIES) == ["her"]
    assert build.fourteen_libraries() == ["hip", "policy", "learner", "episodes", "render", "replay", "bank", "lbank", "segments", "pbt", "qmap",
                                          "fastpol", "nstep", "prio"]
    assert build.fifteen_libraries() == build.fourteen_libraries() + ["her"] and len(build.fifteen_libraries()) == 15
    entry = build.library("her")
    assert entry is build.HINDSIGHT_LIBRARIES["her"] and build.library("prio") is build.PRIORITY_LIBRARIES["prio"]
    src = os.path.join(CSRC, "aqua_her.hip")
    lib = os.path.join(ROOT, "aquaticgymenv_amd", "lib", "libaqua_her.so")
    headers = ["aqua_device.hpp", "aqua_host.hpp"]
    assert entry["src"] == [src] and entry["lib"] == lib and entry["cuid"] == "aqua_her"
    assert re.findall(r'#include "([a-z_]+\.hpp)"', open(src).read()) == headers and '#include "aqua_her.h"' in open(src).read()
    assert entry["deps"] == [src] + [os.path.join(CSRC, h) for h in headers] + [HEADER] and all(os.path.exists(p) for p in entry["deps"])
    assert build.build_command("her") == [
        build.hipcc_path(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-fno-honor-nans", "-cuid=aqua_her",
        "-Wall", "-Wno-unused-function", "-o", lib + ".tmp", src]
    assert (build.HER_SRC, build.HER_DEPS, build.HER_LIB, build.HER_FLAGS) == (entry["src"], entry["deps"], entry["lib"], entry["flags"])
    assert callable(build.build_her) and build.her_needs_build() in (True, False)
    assert len({build.library(n)["lib"] for n in build.fifteen_libraries()}) == 15
    main = open(os.path.join(ROOT, "aquaticgymenv_amd", "build.py")).read().split('if __name__ == "__main__":')[1]
    assert "+ list(FAST_LIBRARIES) + list(NSTEP_LIBRARIES) + list(PRIORITY_LIBRARIES)" in main and "+ list(HINDSIGHT_LIBRARIES)" in main
    for name in build.fourteen_libraries():
        assert not any("aqua_her" in os.path.basename(d) for d in build.library(name)["deps"]), name
    # the learners' shared device code is not part of this library: it hands them rows, it does not restate them
    assert "aqua_lrn.hpp" not in open(src).read() and "aqua_qnet.hpp" not in open(src).read()


def test_graft_entry_builds_and_checks_the_new_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    build_body = text.split("def build():")[1].split("def smoke():")[0]
    assert "fifteen_libraries()[14:]" in build_body and "_her_capi" in build_body and "aquaher_version" in build_body
    assert "fourteen_libraries()[13:]" in build_body
    import __graft_entry__ as entry
    from aquaticgymenv_amd import build
    assert entry.build() is None and os.path.exists(build.HER_LIB)


# ------------------------------------------------------------------------------------------------ the C API without a device
ORDER = ("header", "s", "a", "r", "s2", "d", "ok", "ring_ld", "capacity", "kind", "N", "idx", "P", "B", "H", "ratio", "t_dev", "seed",
         "seed_dev", "out_s", "out_a", "out_r", "out_s2", "out_d", "out_ok", "out_ld", "out_k", "out_m")


def _relabel(lib, **kw):
    a = dict(header=FAKE, s=FAKE + 0x1000, a=FAKE + 0x2000, r=FAKE + 0x3000, s2=FAKE + 0x4000, d=FAKE + 0x5000, ok=FAKE + 0x6000,
             ring_ld=1000, capacity=1000, kind=0, N=50, idx=FAKE + 0x7000, P=3, B=64, H=32, ratio=0.8, t_dev=FAKE + 0xF000, seed=17,
             seed_dev=None, out_s=FAKE + 0x8000, out_a=FAKE + 0x9000, out_r=FAKE + 0xA000, out_s2=FAKE + 0xB000, out_d=FAKE + 0xC000,
             out_ok=FAKE + 0xD000, out_ld=192, out_k=FAKE + 0xE000, out_m=FAKE + 0xE800)
    a.update(kw)
    return lib.aquaher_relabel(*[a[name] for name in ORDER], None)


def test_argument_validation_without_touching_a_device(capi):
    """every call here fails (or returns) before the first HIP call: nothing is launched, no pointer is dereferenced; the
    message names the offending field"""
    lib = capi.lib
    table = dict(seed=capi.NO_SEED, seed_dev=FAKE + 0x10000)
    big = capi.MAX_CAPACITY + 1
    nan, inf = float("nan"), float("inf")
    invalid = [("H", dict(H=0)), ("H", dict(H=-1)), ("H", dict(H=capi.MAX_HORIZON + 1)), ("H", dict(H=2 ** 31 - 1)),
               ("N", dict(N=51)), ("N", dict(N=7)), ("N", dict(N=0)), ("N", dict(N=-50)), ("N", dict(N=1001)), ("N", dict(capacity=999, N=50)),
               ("out_ld", dict(out_ld=191)), ("out_ld", dict(out_ld=0)), ("out_ld", dict(out_ld=-1)),
               ("header", dict(header=None)), ("s", dict(s=None)), ("a", dict(a=None)), ("r", dict(r=None)), ("s2", dict(s2=None)),
               ("d", dict(d=None)), ("ok", dict(ok=None)), ("idx", dict(idx=None)), ("t_dev", dict(t_dev=None)),
               ("out_s", dict(out_s=None)), ("out_a", dict(out_a=None)), ("out_r", dict(out_r=None)), ("out_s2", dict(out_s2=None)),
               ("out_d", dict(out_d=None)), ("out_ok", dict(out_ok=None)),
               ("seed_dev", dict(seed=17, seed_dev=FAKE + 0x10000)), ("seed_dev", dict(seed=2 ** 64 - 1, seed_dev=FAKE + 0x10000)),   # both
               ("ratio", dict(ratio=nan)), ("ratio", dict(ratio=inf)), ("ratio", dict(ratio=1.0000001)), ("ratio", dict(ratio=-1e-9)),
               ("ratio", dict(ratio=-inf)),
               ("capacity", dict(capacity=0)), ("capacity", dict(capacity=-5)), ("capacity", dict(capacity=big, ring_ld=big)),
               ("ring_ld", dict(ring_ld=999)), ("action_kind", dict(kind=2)), ("action_kind", dict(kind=-1)),
               ("P", dict(P=0)), ("P", dict(P=-1)), ("P", dict(P=capi.MAX_NETWORKS + 1)), ("B", dict(B=-1)), ("B", dict(B=capi.MAX_BATCH + 1))]
    for field, kw in invalid:
        assert _relabel(lib, **kw) == capi.E_INVALID, kw
        assert re.search(r"\b%s\b" % field, capi.last_error()), (kw, capi.last_error())
    misaligned = [("header", dict(header=FAKE + 4)), ("header", dict(header=FAKE + 1)), ("float32", dict(s=FAKE + 0x1002)),
                  ("float32", dict(r=FAKE + 0x3001)), ("float32", dict(s2=FAKE + 0x4002)), ("idx", dict(idx=FAKE + 0x7002)),
                  ("float32", dict(out_s=FAKE + 0x8001)), ("float32", dict(out_r=FAKE + 0xA002)), ("float32", dict(out_s2=FAKE + 0xB003)),
                  ("action", dict(kind=1, a=FAKE + 0x2002)), ("action", dict(kind=1, out_a=FAKE + 0x9001)),
                  ("t_dev", dict(t_dev=FAKE + 0xF004)), ("seed_dev", dict(seed=0, seed_dev=FAKE + 0x10004))]
    for field, kw in misaligned:
        assert _relabel(lib, **kw) == capi.E_ALIGN, kw
        assert re.search(r"\b%s\b" % field, capi.last_error()), (kw, capi.last_error())
    # the limits themselves pass the size checks (and then meet the alignment check); so do the table form and both ends of ratio
    assert _relabel(lib, H=capi.MAX_HORIZON, P=capi.MAX_NETWORKS, B=capi.MAX_BATCH, out_ld=2 ** 32, header=FAKE + 4) == capi.E_ALIGN
    assert _relabel(lib, H=1, N=1000, header=FAKE + 4) == capi.E_ALIGN and _relabel(lib, N=1, header=FAKE + 4) == capi.E_ALIGN
    assert _relabel(lib, header=FAKE + 4, **table) == capi.E_ALIGN
    assert _relabel(lib, ratio=0.0, header=FAKE + 4) == capi.E_ALIGN and _relabel(lib, ratio=1.0, header=FAKE + 4) == capi.E_ALIGN
    assert _relabel(lib, out_k=None, out_m=None, header=FAKE + 4) == capi.E_ALIGN
    assert _relabel(lib, seed=0, header=FAKE + 4) == capi.E_ALIGN and _relabel(lib, seed=2 ** 64 - 1, header=FAKE + 4) == capi.E_ALIGN
    # nothing to do: no launch, no device, neither idx nor the staged rows are needed
    assert _relabel(lib, B=0, out_ld=0, idx=None, out_s=None, out_ok=None) == 0 and _relabel(lib, B=0, **table) == 0
    # the Python layer turns E_INVALID into ValueError and everything else into the binding's error
    with pytest.raises(ValueError, match="^aquaher_relabel: H=0"):
        capi.check(_relabel(lib, H=0), "aquaher_relabel")
    with pytest.raises(ValueError, match="no multiple of N"):
        capi.check(_relabel(lib, N=7), "aquaher_relabel")
    with pytest.raises(capi.AquaHerError):
        capi.check(_relabel(lib, header=FAKE + 4), "aquaher_relabel")
    # the host entries
    r, d = ctypes.c_float(0), ctypes.c_uint8(0)
    row = (ctypes.c_float * 5)()
    for kw in (dict(s=None), dict(s2=None), dict(r=None), dict(d=None)):
        a = dict(s=ctypes.addressof(row), s2=ctypes.addressof(row), r=ctypes.addressof(r), d=ctypes.addressof(d))
        a.update(kw)
        assert lib.aquaher_reward(a["s"], a["s2"], 0.5, 0.5, a["r"], a["d"]) == capi.E_INVALID and capi.last_error()
    assert lib.aquaher_threshold(0.5, None) == capi.E_INVALID and "thr" in capi.last_error()


def test_no_cpu_path_and_argument_errors_of_the_class(capi):
    import torch
    from aquaticgymenv_amd.hindsight import HindsightReplay
    for bad in (object(), None, 3):
        with pytest.raises(ValueError):
            HindsightReplay(bad, 64)
    env = types.SimpleNamespace(num_envs=8, continuous=False)
    ring = types.SimpleNamespace(torch=torch, env=env, header=object(), device=torch.device("cpu"), capacity=64, _kind=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        HindsightReplay(ring, 64)
    if not torch.cuda.is_available():
        ring.device = torch.device("cuda:0")
        with pytest.raises(RuntimeError, match="no CPU path"):
            HindsightReplay(ring, 64)
    assert not hasattr(HindsightReplay, "state_dict")


# ------------------------------------------------------------------------------------------------ the threshold
def test_threshold_is_the_floor_of_ratio_times_two_to_the_32(capi):
    for ratio, want in ((0.0, 0), (1.0, 2 ** 32), (0.8, 3435973836), (2.0 ** -33, 0), (1.0 - 2.0 ** -33, 2 ** 32 - 1), (0.5, 2 ** 31),
                        (2.0 ** -32, 1)):
        assert capi.threshold(ratio) == want == M.threshold(ratio), ratio
    assert 3435973836 == (8 * 2 ** 32) // 10                       # 0.8 as a double lies above 4/5 by less than 2^-32
    for word in (1, 12345, 2 ** 31, 2 ** 32 - 2):                  # half a unit above a word: the floor, not the ceiling or the nearest
        assert capi.threshold((word + 0.5) / 2.0 ** 32) == word == M.threshold((word + 0.5) / 2.0 ** 32)
    for bad in (-1e-300, 1.0 + 2.0 ** -52, float("nan"), float("inf"), -float("inf"), 2.0, -0.5):
        out = ctypes.c_uint64(77)
        assert capi.lib.aquaher_threshold(bad, ctypes.byref(out)) == capi.E_INVALID and "ratio" in capi.last_error() and out.value == 77
        with pytest.raises(ValueError, match="ratio"):
            capi.threshold(bad)


# ------------------------------------------------------------------------------------------------ the reward
def _rewards(capi, s, s2, g):
    """aquaher_reward row by row.  s, s2: float32 [n][5]; g: float32 [n][2] -> (r float32 [n], d uint8 [n])"""
    n = s.shape[0]
    s, s2, g = (np.ascontiguousarray(x, np.float32) for x in (s, s2, g))
    r, d = np.full(n, -77, np.float32), np.full(n, 77, np.uint8)
    fn = capi.lib.aquaher_reward
    ps, ps2, pr, pd = s.ctypes.data, s2.ctypes.data, r.ctypes.data, d.ctypes.data
    gx, gy = g[:, 0].tolist(), g[:, 1].tolist()
    for i in range(n):
        assert fn(ps + 20 * i, ps2 + 20 * i, gx[i], gy[i], pr + 4 * i, pd + i) == 0
    return r, d


def test_reward_equals_the_model_bit_for_bit(capi):
    """10^5 normalised triples (previous position, new position, goal): uniform ones, steps of a realistic length, coincident
    points, and new positions placed at the radius +- a few 1e-7, where gap_new changes sign"""
    rng = np.random.RandomState(11)
    n = 100000
    s, s2 = rng.rand(n, 5).astype(np.float32), rng.rand(n, 5).astype(np.float32)
    g = rng.rand(n, 2).astype(np.float32)
    step = slice(20000, 60000)                                    # a step of up to 0.5 world units
    s2[step, 0:2] = s[step, 0:2] + ((rng.rand(40000, 2) - 0.5) * 0.01).astype(np.float32)
    edge = slice(60000, 90000)                                    # the new position on the circle of radius 0.05 about the goal
    phi = rng.rand(30000) * 2 * np.pi
    off = rng.randint(-4, 5, 30000) * 1e-7
    s2[edge, 0] = (g[edge, 0] + (0.05 + off) * np.cos(phi)).astype(np.float32)
    s2[edge, 1] = (g[edge, 1] + (0.05 + off) * np.sin(phi)).astype(np.float32)
    same = slice(90000, 95000)                                    # the new position IS the goal (k = 0), bit for bit
    g[same] = s2[same, 0:2]
    s[95000:97000] = s2[95000:97000]                              # no move at all
    g[97000:98000] = s[97000:98000, 0:2]                          # the previous position is the goal
    s[98000:99000, 0:2] = s2[98000:99000, 0:2] = g[98000:99000]   # all three coincide
    got_r, got_d = _rewards(capi, s, s2, g)
    want_r, want_d = M.reward(s[:, 0], s[:, 1], s2[:, 0], s2[:, 1], g[:, 0], g[:, 1])
    assert np.array_equal(got_r.view(np.uint32), want_r.view(np.uint32)) and np.array_equal(got_d, want_d)
    gap_new = M.gap(s2[:, 0], s2[:, 1], g[:, 0], g[:, 1])
    close = np.abs(gap_new[edge]) < 5e-5
    print("edge rows: %d within 5e-5 of the radius, %d inside, %d outside" % (close.sum(), (got_d[edge] == 3).sum(), (got_d[edge] == 0).sum()))
    assert close.sum() > 20000 and (got_d[edge] == 3).sum() > 5000 and (got_d[edge] == 0).sum() > 5000
    assert set(np.unique(got_d)) == {0, 3} and (got_d[same] == 3).all() and (got_r[same] == 10).all() and (gap_new[same] == -5).all()
    assert (got_r[got_d == 3] == 10).all() and (got_d[98000:99000] == 3).all()
    assert (got_r[95000:97000][got_d[95000:97000] == 0] == 0).all()             # no move, no reward
    # the binding's own wrapper is the same call
    assert capi.reward(s[7], s2[7], g[7, 0], g[7, 1]) == (float(got_r[7]), int(got_d[7]))


def test_reward_equals_the_reference_on_its_own_steps(capi):
    """the 3 948 rows of the golden step file that end in neither a collision nor the time limit, normalised as the step kernel
    normalises the observation (float32, x 0.01f), replayed under the row's own goal: the code is the reference's wherever its
    margin is not a knife edge, and the reward is within 4e-5 -- one float32 rounding of each coordinate and one of the product,
    about 9e-6 per coordinate, <= 2.5e-5 per gap, x 1.4 for 0.7 (gap_prev - gap_new)"""
    z = _golden.StepGolden().z
    keep = (z["term"] == 0) | (z["term"] == 3)
    assert int(keep.sum()) == 3948
    norm = lambda x: (np.asarray(x, np.float64).astype(np.float32) * np.float32(0.01)).astype(np.float32)       # noqa: E731
    state, pose, m_goal = z["state_in"][keep], z["pose"][keep], z["m_goal"][keep]
    s, s2 = np.zeros((3948, 5), np.float32), np.zeros((3948, 5), np.float32)
    s[:, 0:2], s2[:, 0:2] = norm(state[:, 0:2]), norm(pose[:, 0:2])
    g = norm(state[:, 3:5])
    got_r, got_d = _rewards(capi, s, s2, g)
    compared = np.abs(m_goal) >= 3e-5
    assert int((~compared).sum()) <= int((np.abs(m_goal) < 1e-4).sum()) <= 608       # the file's hand-made knife edges
    assert np.array_equal(got_d[compared], z["term"][keep][compared].astype(np.uint8))
    err = np.abs(got_r.astype(np.float64) - z["reward"][keep])[compared]
    wrong = got_d != z["term"][keep]
    print("compared %d rows, largest reward error %.3g; codes differ on %d rows, the widest at |m_goal| = %.3g"
          % (compared.sum(), err.max(), wrong.sum(), np.abs(m_goal[wrong]).max() if wrong.any() else 0.0))
    assert err.max() <= 4e-5
    assert (got_d[compared] == 3).sum() > 100 and (got_d[compared] == 0).sum() > 3000


# ------------------------------------------------------------------------------------------------ the model
def _hand_ring():
    """N = 2 worlds, capacity 8 (4 rounds), cursor 6: rounds 0 .. 2 written, round 3 never (ok == 0).  World 0 moves along x
    by 0.1 a step and never ends; world 1 creeps by 0.01 a step and its episode ends in round 1"""
    s, s2 = np.zeros((5, 8), np.float32), np.zeros((5, 8), np.float32)
    for rnd in range(4):
        s[0, 2 * rnd], s2[0, 2 * rnd] = 0.1 * rnd, 0.1 * (rnd + 1)
        s[0, 2 * rnd + 1], s2[0, 2 * rnd + 1] = 0.01 * rnd, 0.01 * (rnd + 1)
    s[1], s2[1] = 0.5, 0.5
    s[3:5], s2[3:5] = 0.9, 0.9
    ring = dict(capacity=8, s=s, s2=s2, r=np.array([1, 10, 2, 20, 4, 40, 0, 0], np.float32), a=np.array([0, 1, 2, 0, 1, 2, 0, 0], np.uint8),
                d=np.array([0, 0, 0, 3, 0, 0, 0, 0], np.uint8), ok=np.array([1, 1, 1, 1, 1, 1, 0, 0], np.uint8))
    return ring, np.array([6, 6, 4, 3], np.int64)


def test_the_model_on_a_hand_made_ring():
    ring, header = _hand_ring()
    idx = np.array([[0, 1, 2, 3, 4, 5, 6, -1, 8]], np.int32)
    walks = [M.walk(ring, 6, 2, c, 8) for c in idx[0]]
    assert walks == [(M.FRONTIER, 3), (M.EPISODE_END, 1), (M.FRONTIER, 2), (M.OWN_TERMINAL, 0), (M.FRONTIER, 1), (M.FRONTIER, 1),
                     (M.NOT_OK, 0), (M.OUTSIDE, 0), (M.OUTSIDE, 0)]
    assert [M.walk(ring, 6, 2, c, 2) for c in (0, 2, 4)] == [(M.CAPPED, 2), (M.CAPPED, 2), (M.FRONTIER, 1)]
    assert M.walk(ring, 6, 2, 0, 3) == (M.CAPPED, 3) and M.walk(ring, 6, 2, 4, 1) == (M.CAPPED, 1)
    # ratio 0: the ring's own rows, k = 0 everywhere, m the walk's
    out = M.relabel(ring, header, 2, idx, 8, 0.0, [5], [17])
    assert list(out["ok"]) == [1, 1, 1, 1, 1, 1, 0, 0, 0] and list(out["m"]) == [3, 1, 2, 0, 1, 1, 0, 0, 0] and not out["k"].any()
    assert out["fate"] == [M.NOT_CHOSEN, M.NOT_CHOSEN, M.NOT_CHOSEN, M.KEPT, M.NOT_CHOSEN, M.NOT_CHOSEN, None, None, None]
    for name in ("s", "a", "r", "s2", "d"):
        assert np.array_equal(out[name][..., :6], ring[name][..., :6]) and not out[name][..., 6:].any(), name
    # ratio 1: everything with M > 0 is relabelled; world 0's steps of 0.1 reach the goal only with k = 0, world 1 creeps
    # within the radius of where it is one step later
    out = M.relabel(ring, header, 2, idx, 8, 1.0, [5], [17])
    assert list(out["m"]) == [3, 1, 2, 0, 1, 1, 0, 0, 0] and list(out["ok"]) == [1, 1, 1, 1, 1, 1, 0, 0, 0]
    r0, r1 = M.draws(17, 5, 9)
    for i, c in enumerate(idx[0][:6]):
        m = int(out["m"][i])
        if m == 0:
            assert out["k"][i] == 0 and out["r"][i] == ring["r"][c] and out["d"][i] == ring["d"][c] and out["fate"][i] == M.KEPT
            continue
        k = (int(r1[i]) * m) >> 32
        goal = ring["s2"][0:2, (c + 2 * k) % 8]
        assert out["k"][i] == k + 1 and np.array_equal(out["s"][3:5, i], goal) and np.array_equal(out["s2"][3:5, i], goal)
        assert np.array_equal(out["s"][0:3, i], ring["s"][0:3, c]) and np.array_equal(out["s2"][0:3, i], ring["s2"][0:3, c])
        if k == 0:
            assert out["r"][i] == 10 and out["d"][i] == 3 and out["fate"][i] == M.SUCCESS_K0
        else:                                                     # world 0, a goal 0.1 k further along x: 100 x 0.1 x 0.7 = 7
            assert c % 2 == 0 and out["d"][i] == 0 and abs(float(out["r"][i]) - 7.0) < 1e-4 and out["fate"][i] == M.SHAPED
    # the draw is keyed by t + 1 and the key: another counter or another key is another draw
    assert not np.array_equal(M.draws(17, 5, 64)[0], M.draws(17, 6, 64)[0]) and not np.array_equal(M.draws(17, 5, 64)[0], M.draws(18, 5, 64)[0])
    # a full ring that has wrapped: cursor 2, so round 0 is the newest and round 1 the oldest; the walk of slot 6 wraps
    ring["ok"][6:] = 1
    assert [M.walk(ring, 2, 2, c, 8) for c in (6, 4, 0, 7, 2)] == [(M.FRONTIER, 2), (M.FRONTIER, 3), (M.FRONTIER, 1), (M.FRONTIER, 2), (M.FRONTIER, 4)]
    # a cursor that is no multiple of N, or outside the ring: nothing is a sample
    for cursor in (3, 8, -2):
        header[0] = cursor
        out = M.relabel(ring, header, 2, idx, 8, 1.0, [5], [17])
        assert set(out["cut"]) == {M.BAD_CURSOR} and not out["ok"].any() and not out["r"].any() and not out["m"].any() and not out["k"].any()
    # a broken chain: slot 2 (world 0, round 1) is no experience; with cursor 0 (round 3 the newest) slot 0's walk meets it
    ring["ok"][2] = 0
    assert [M.walk(ring, 0, 2, c, 8) for c in (0, 2, 4)] == [(M.BROKEN, 1), (M.NOT_OK, 0), (M.FRONTIER, 2)]


@pytest.mark.parametrize("H", [1, 2, 3, 5, 8])
def test_the_model_is_the_per_world_walk(H):
    """walk() against per_world(), which unrolls the ring into each world's transitions in the order they were made and counts
    from the sample's on: the same M for every slot of the crafted ring under every valid cursor, and for random rings"""
    rng = np.random.RandomState(H)
    rings = [(M.crafted_ring(), 7)]
    for _ in range(6):
        N = int(rng.randint(1, 6))
        cap = N * int(rng.randint(1, 9))
        ring = dict(capacity=cap, d=(rng.randint(0, 4, cap) * (rng.rand(cap) < 0.2)).astype(np.uint8), ok=(rng.rand(cap) < 0.85).astype(np.uint8))
        rings.append((ring, N))
    seen = set()
    for ring, N in rings:
        cap = ring["capacity"]
        for cursor in range(0, cap, N):
            for c in range(cap):
                what, m = M.walk(ring, cursor, N, c, H)
                assert m == M.per_world(ring, cursor, N, c, H), (N, cap, cursor, c, what)
                assert 0 <= m <= H and (what != M.CAPPED or m == H) and (what not in M.NO_SAMPLE + (M.OWN_TERMINAL,) or m == 0)
                seen.add(what)
    # (a horizon of 8 is as long as the longest of these rings has rounds: no walk of theirs reaches it)
    want = {1: {M.NOT_OK, M.OWN_TERMINAL, M.CAPPED}, 8: {M.NOT_OK, M.OWN_TERMINAL, M.EPISODE_END, M.BROKEN, M.FRONTIER}}
    assert seen >= want.get(H, {M.NOT_OK, M.OWN_TERMINAL, M.EPISODE_END, M.BROKEN, M.FRONTIER, M.CAPPED}), seen


# ------------------------------------------------------------------------------------------------ the compiler's metadata
def test_codegen_has_no_scratch_no_spills_and_no_lds():
    """the resource metadata of the code object's notes: one instance of the kernel per action kind and source of the key,
    none with a private segment, a spilled register or LDS.  The register counts are printed for the record"""
    isa = _isa.kernels("her")
    assert len(isa) == 4 and all("her_relabel_kernel" in name for name in isa), sorted(isa)
    for name, k in isa.items():
        m = k["meta"]
        print("registers:", name, m)
        assert m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0 and m["agpr_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)                 # four wavefronts per SIMD at least
        assert k["stats"]["ScratchSize"] == 0, (name, k["stats"])
