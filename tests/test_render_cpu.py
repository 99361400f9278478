"""CPU-only checks of libaqua_render.so (include/aqua_render.h) and of the model the GPU tests hold it to: the library
builds, loads and exports what its header declares without touching the other four; bad arguments are rejected before a
device is touched; the compiled kernels have no scratch and no spills; tests/_render.py, the float64 restatement of
gym_aqua/envs/aqua.py:215-365, gives the pixels worked out by hand for one scene; the comparison rejects six deliberate
mistakes; the scenes of tests/test_render_gpu.py keep their knife-edge share under 0.2 % and reach the launch shapes they are chosen for; the facade without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _isa
from tests import _render as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000            # a "device pointer" for calls that must fail (or return) before anything dereferences it

# every kernel of the gfx950 code object, and the test of tests/test_render_gpu.py that launches it
KERNELS = {"rnd_frames_kernel": "test_frames_equal_the_model",
           "rnd_overlay_kernelILb1E": "test_overlay_equals_the_reference_arithmetic",
           "rnd_overlay_kernelILb0E": "test_overlay_equals_the_reference_arithmetic"}


@pytest.fixture(scope="module")
def rcapi():
    from aquaticgymenv_amd.build import build_library
    for name in ("hip", "policy", "learner", "episodes", "render"):
        assert os.path.exists(build_library(name))
    from aquaticgymenv_amd import _render_capi
    return _render_capi


# ------------------------------------------------------------------ the library
def test_library_builds_loads_and_exports_its_header(rcapi):
    text = open(os.path.join(ROOT, "include", "aqua_render.h")).read()
    declared = set(re.findall(r"\b(aquarnd_[a-z0-9_]+)\s*\(", text))
    assert declared == set(rcapi.SYMBOLS), declared ^ set(rcapi.SYMBOLS)
    raw = ctypes.CDLL(rcapi.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    assert rcapi.lib.aquarnd_version() == rcapi.ABI_VERSION == 1

    def define(name):
        return int(re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, text).group(1))
    assert define("AQUARND_ABI_VERSION") == 1
    assert [define("AQUARND_E_" + n) for n in ("INVALID", "ALIGN", "NODEVICE")] == [-1, -2, -3]
    assert [rcapi.E_INVALID, rcapi.E_ALIGN, rcapi.E_NODEVICE] == [-1, -2, -3]
    assert define("AQUARND_MAX_WORLDS") == rcapi.MAX_WORLDS and define("AQUARND_MAX_ROWS") == rcapi.MAX_ROWS == 64
    assert (define("AQUARND_MIN_SIZE"), define("AQUARND_MAX_SIZE")) == (rcapi.MIN_SIZE, rcapi.MAX_SIZE) == (16, 1000)
    assert define("AQUARND_OVERLAY_ROWS") == rcapi.OVERLAY_ROWS == 4 and define("AQUARND_MAX_BLOCKS") == rcapi.MAX_BLOCKS == 2 ** 24 - 1


def test_the_four_libraries_and_their_recipes_are_unchanged(rcapi):
    from aquaticgymenv_amd import _capi, _episodes_capi, _learner_capi, _policy_capi, build
    names = ["hip", "policy", "learner", "episodes"]
    assert list(build.LIBRARIES) == names and list(build.EXTRA_LIBRARIES) == ["render"]
    assert build.all_libraries() == names + ["render"]
    pkg = os.path.join(ROOT, "aquaticgymenv_amd")
    for name in names + ["render"]:
        lib = os.path.join(pkg, "lib", "libaqua_%s.so" % name)
        assert build.build_command(name) == [
            build.hipcc_path(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-fno-honor-nans",
            "-cuid=aqua_" + name, "-Wall", "-Wno-unused-function", "-o", lib + ".tmp", os.path.join(pkg, "csrc", "aqua_%s.hip" % name)]
        assert build.library(name) is (build.LIBRARIES if name != "render" else build.EXTRA_LIBRARIES)[name]
        assert build.needs_build(name) is False
    extra = build.EXTRA_LIBRARIES["render"]
    assert [f for f in extra["flags"] if f.startswith("-cuid")] == ["-cuid=aqua_render"] and extra["cuid"] == "aqua_render"
    assert sorted(f for f in extra["flags"] if not f.startswith("-cuid")) == sorted(f for f in build.COMMON_FLAGS if not f.startswith("-cuid"))
    for name in names:
        assert not set(extra["src"]) & set(build.LIBRARIES[name]["src"]) and extra["lib"] != build.LIBRARIES[name]["lib"]
    assert set(extra["src"]) <= set(extra["deps"]) and all(os.path.exists(d) for d in extra["deps"])
    assert os.path.join(ROOT, "include", "aqua_render.h") in extra["deps"] and os.path.join(pkg, "csrc", "aqua_host.hpp") in extra["deps"]
    assert (build.RENDER_SRC, build.RENDER_LIB) == (extra["src"], extra["lib"]) and build.build_render() == extra["lib"]
    # no aquarnd_ name in the other headers, bindings or libraries
    assert len(_capi.SYMBOLS) == 38 and len(_policy_capi.SYMBOLS) == 5 and len(_learner_capi.SYMBOLS) == 4 and len(_episodes_capi.SYMBOLS) == 5
    for header in ("aqua_hip.h", "aqua_policy.h", "aqua_learner.h", "aqua_episodes.h"):
        assert "aquarnd_" not in open(os.path.join(ROOT, "include", header)).read().lower()
    for other in (_capi, _policy_capi, _learner_capi, _episodes_capi):
        assert not any(s.startswith("aquarnd_") for s in other.SYMBOLS)
        assert "aquarnd_" not in open(other.__file__).read()
        for name in rcapi.SYMBOLS:
            assert not hasattr(other.lib, name)


def _frames(lib, **kw):
    a = dict(state=FAKE, ld=128, N=100, overlay=FAKE + 0x10000, overlay_ld=128, rows=FAKE + 0x20000, K=5, per_world=0, waves=1,
             worlds=FAKE + 0x30000, M=4, S=64, out=FAKE + 0x40000, out_bytes=4 * 3 * 64 * 64)
    a.update(kw)
    return lib.aquarnd_frames_u8(a["state"], a["ld"], a["N"], a["overlay"], a["overlay_ld"], a["rows"], a["K"], a["per_world"], a["waves"],
                                 a["worlds"], a["M"], a["S"], a["out"], a["out_bytes"], None)


def test_argument_validation_without_touching_a_device(rcapi):
    lib = rcapi.lib
    invalid = [dict(state=None), dict(out=None), dict(S=12), dict(S=18), dict(S=1004), dict(S=0), dict(K=65), dict(K=-1), dict(N=-1),
               dict(M=-1), dict(out_bytes=4 * 3 * 64 * 64 - 1), dict(S=500, out_bytes=4 * 3 * 500 * 500 - 1), dict(overlay_ld=99),
               dict(ld=99), dict(rows=None), dict(worlds=None, M=101, out_bytes=1 << 40), dict(N=rcapi.MAX_WORLDS + 1),
               dict(M=rcapi.MAX_WORLDS + 1, out_bytes=1 << 62)]
    for kw in invalid:
        assert _frames(lib, **kw) == rcapi.E_INVALID, kw
        assert lib.aquarnd_last_error().decode(), kw
    for kw in (dict(state=FAKE + 2), dict(overlay=FAKE + 0x10001), dict(worlds=FAKE + 0x30002), dict(out=FAKE + 0x40003), dict(rows=FAKE + 0x20002)):
        assert _frames(lib, **kw) == rcapi.E_ALIGN, kw
        assert lib.aquarnd_last_error().decode(), kw
    # more blocks than one launch holds (2^32 - 1 threads): rejected by validation, not by the launch
    assert _frames(lib, S=16, M=1 << 24, out_bytes=1 << 62) == rcapi.E_INVALID and b"several calls" in lib.aquarnd_last_error()
    assert _frames(lib, S=1000, M=134218, out_bytes=1 << 62) == rcapi.E_INVALID
    # nothing to draw: no launch, no device, no pointer looked at
    assert _frames(lib, M=0) == 0 and _frames(lib, N=0) == 0
    assert _frames(lib, M=0, state=None, overlay=None, rows=None, worlds=None, out=None, out_bytes=0) == 0
    assert _frames(lib, N=0, state=None, overlay=None, rows=None, worlds=None, out=None, out_bytes=0) == 0
    # the overlay entries
    u8, f32 = lib.aquarnd_overlay_u8, lib.aquarnd_overlay_f32x2
    assert u8(None, 0, 0, None, None, 0, None) == 0 and f32(None, 0, 0, None, 0, None, 0, None) == 0
    for args in ((None, 128, 100, FAKE, FAKE, 128, None), (FAKE, 128, 100, None, FAKE, 128, None), (FAKE, 128, 100, FAKE, None, 128, None),
                 (FAKE, 99, 100, FAKE, FAKE, 128, None), (FAKE, 128, 100, FAKE, FAKE, 99, None), (FAKE, 128, -1, FAKE, FAKE, 128, None)):
        assert u8(*args) == rcapi.E_INVALID, args
        assert lib.aquarnd_last_error().decode(), args
    for args in ((FAKE, 128, 100, None, 128, FAKE, 128, None), (FAKE, 128, 100, FAKE, 99, FAKE, 128, None), (FAKE, 128, 100, FAKE, 128, FAKE, 99, None)):
        assert f32(*args) == rcapi.E_INVALID, args
    assert u8(FAKE + 1, 128, 100, FAKE, FAKE, 128, None) == rcapi.E_ALIGN and u8(FAKE, 128, 100, FAKE + 1, FAKE + 2, 128, None) == rcapi.E_ALIGN
    assert f32(FAKE, 128, 100, FAKE + 2, 128, FAKE, 128, None) == rcapi.E_ALIGN and lib.aquarnd_last_error().decode()


def test_codegen_has_no_scratch_and_no_spills():
    isa = _isa.kernels("render")
    names = {n: [k for k in KERNELS if k in n] for n in isa}
    assert all(len(v) == 1 for v in names.values()) and len(isa) == len(KERNELS) == 3, sorted(isa)
    assert {v[0] for v in names.values()} == set(KERNELS)
    gpu_tests = open(os.path.join(ROOT, "tests", "test_render_gpu.py")).read()
    for kernel, test in KERNELS.items():
        assert re.search(r"^def %s\(" % test, gpu_tests, re.M), (kernel, test)
    for name, k in isa.items():
        m, st = k["meta"], k["stats"]
        assert st["ScratchSize"] == 0 and m["private_segment_fixed_size"] == 0, (name, m, st)
        assert m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert "scratch_" not in k["body"] and "global_atomic" not in k["body"], name
    frames = [k for n, k in isa.items() if "rnd_frames_kernel" in n][0]
    # four pixels leave as three dwords in one store; no byte or short stores anywhere; the list lives in LDS
    assert "global_store_dwordx3" in frames["body"], "the frame kernel does not store 12 bytes per lane"
    assert not re.search(r"(global|flat|buffer)_store_(byte|short)", frames["body"])
    assert 4096 <= frames["meta"]["group_segment_fixed_size"] <= 8192 and frames["stats"]["Occupancy"] == 8, frames["meta"]


# ------------------------------------------------------------------ the model against rows worked out by hand
S5 = 500
HAND_STATE = np.array([50, 50, 0, 25, 80, 0.03, -0.04], dtype=np.float32)


@pytest.fixture(scope="module")
def hand():
    from aquaticgymenv_amd import presets
    overlay = R.overlay_model(HAND_STATE, 2, False)
    assert overlay[:2] == (0.5, 0.5) and overlay[2] < -1e8
    return R.draw(HAND_STATE, overlay, presets.DEFAULT5, 1, S5), R.draw(HAND_STATE, None, presets.DEFAULT5, 1, S5)


def _px(frame, x, y):
    """the pixel whose centre is (x + 0.5, y + 0.5) in viewer coordinates (y up)"""
    return tuple(int(v) for v in frame[S5 - 1 - y, x])


def test_model_hand_rows(hand):
    sc, sc0 = hand
    f = sc.frame
    # the boat is a 30-gon of radius 12.5 px at (250, 250); the heading bar [246.875, 253.125] x [250, 262.5] lies over its centre
    assert _px(f, 250, 250) == R.C_DIRECTION and _px(f, 250, 245) == R.C_BOAT and _px(f, 250, 236) == R.WHITE
    # its tip is the line y = 262.5: centre 261.5 is inside, 263.5 outside (and outside the boat: |(0.5, 13.5)| > 12.5); 262.5 is a tie
    assert _px(f, 250, 261) == R.C_DIRECTION and _px(f, 250, 263) == R.WHITE and sc.margin[S5 - 1 - 262, 250] < R.DELTA
    # rectangle (65, 85) 5 x 5 -> [312.5, 337.5) x [412.5, 437.5): left and bottom in, right and top out
    assert _px(f, 312, 420) == R.C_OBSTACLE and _px(f, 311, 420) == R.WHITE
    assert _px(f, 336, 420) == R.C_OBSTACLE and _px(f, 337, 420) == R.WHITE
    assert _px(f, 320, 412) == R.C_OBSTACLE and _px(f, 320, 411) == R.WHITE
    assert _px(f, 320, 436) == R.C_OBSTACLE and _px(f, 320, 437) == R.WHITE
    assert np.isinf(sc.margin[S5 - 1 - 420, 312]) and np.isinf(sc.margin[S5 - 1 - 437, 320])      # exact: no band around a rectangle
    # thrust bars: 8 * 5 * (0.5 * 5) = 100 px long from y = 250, x in [240.625, 246.875] and [253.125, 259.375]
    assert _px(f, 243, 349) == R.C_THRUST and _px(f, 243, 350) == R.WHITE and _px(f, 256, 349) == R.C_THRUST and _px(f, 256, 350) == R.WHITE
    assert _px(f, 240, 300) == R.WHITE and _px(f, 241, 300) == R.C_THRUST and _px(f, 246, 300) == R.C_THRUST
    assert _px(f, 247, 300) == R.WHITE and _px(f, 259, 300) == R.WHITE and _px(f, 258, 300) == R.C_THRUST
    # a straight action: the ICC is 6.25e8 px away and nowhere in the frame; with a zero overlay a quarter of it sits in the corner
    assert _px(f, 0, 0) == R.WHITE and not np.any(sc.shape == 5 + 5)
    f0 = sc0.frame
    assert _px(f0, 0, 0) == R.C_DIRECTION and _px(f0, 2, 0) == R.C_DIRECTION and _px(f0, 2, 2) == R.WHITE      # |(2.5, 2.5)| > 3.125 > |(2.5, 0.5)|
    assert _px(f0, 243, 300) == R.WHITE and _px(f0, 250, 255) == R.C_DIRECTION                                  # no bars, the heading bar stays
    assert int((sc0.shape == 5 + 5).sum()) in range(6, 10)                                                     # pi 3.125^2 / 4 = 7.7 px
    # wave (0.03, -0.04) * 5 = 0.25 px/s along (0.6, -0.8): the tip's apex is (20, 20) + 7.5 (0.6, -0.8) = (24.5, 14)
    assert _px(f, 23, 14) == R.C_WAVE and _px(f, 25, 12) == R.WHITE
    assert _px(f, 21, 17) == R.C_WAVE                                # (21.5, 17.5): 2.9 px up the tip's axis, 0.3 px beside it
    # the body, 5 px wide, runs 40 * 0.25 = 10 px back from (20, 20): (17.5, 24.5) is 5.1 px behind the base, (12.5, 29.5) 12.1 px
    assert _px(f, 17, 24) == R.C_WAVE and _px(f, 12, 29) == R.WHITE
    # row 0 is the top: the goal at (125, 400) is in image row 99
    assert tuple(f[99, 125]) == R.C_GOAL and tuple(f[400, 125]) == R.WHITE
    assert sc.shape[99, 125] == 5 + 0 and sc.shape[S5 - 1 - 250, 250] == 5 + 4


def test_make_circle_is_a_polygon_not_a_disc():
    v = R.make_circle(50.0)
    assert v.shape == (30, 2) and np.allclose(v[0], (50, 0)) and np.allclose(np.hypot(v[:, 0], v[:, 1]), 50)
    X, Y = np.meshgrid(np.array([49.8 * np.cos(np.pi / 30)]), np.array([49.8 * np.sin(np.pi / 30)]))
    inside, dist = R.cover(v, X, Y)                                  # inside the disc, outside the polygon (mid-edge sagitta 0.27 px)
    assert not inside[0, 0] and abs(dist[0, 0] - (49.8 - 50 * np.cos(np.pi / 30))) < 1e-9


# ------------------------------------------------------------------ controls: the comparison must reject these
def _control_state():
    st = HAND_STATE.copy()
    st[3:5] = (51.5, 51.0)                                           # the goal overlaps the boat
    st[2] = 0.7
    return st


@pytest.mark.parametrize("mutant", ["goal_last", "disc", "no_flip", "right_inclusive", "thrust_once"] + ["shift:" + n for n in R.SHAPES])
def test_comparison_rejects_the_mutant(mutant):
    from aquaticgymenv_amd import presets
    st = _control_state()
    overlay = R.overlay_model(st, 0, False)
    assert abs(overlay[2]) < 100 and abs(overlay[3]) < 100           # the ICC of a turn is in the frame
    good = R.draw(st, overlay, presets.DEFAULT5, 1, S5)
    ok, msg, share = R.compare([good], good.frame[None])
    assert ok and share <= R.MAX_SHARE, msg
    bad = R.draw(st, overlay, presets.DEFAULT5, 1, S5, mutant=mutant)
    ok, msg, _ = R.compare([good], bad.frame[None])
    assert not ok and "differ outside the band" in msg, (mutant, msg)


def test_comparison_tolerates_only_the_shapes_meeting_at_a_knife_edge(hand):
    sc, _ = hand
    i, j = S5 - 1 - 262, 250                                         # the tie on the heading bar's tip: bar or background
    assert sc.knife()[i, j] and R.allowed_colours(sc, i, j) == {R.C_DIRECTION, R.WHITE}
    for colour, verdict in ((R.WHITE, True), (R.C_DIRECTION, True), (R.C_BOAT, False), ((0, 0, 0), False)):
        got = sc.frame.copy()
        got[i, j] = colour
        assert R.compare([sc], got[None])[0] is verdict, colour


# ------------------------------------------------------------------ the scenes of the GPU tests
def _cases():
    for kind in R.TABLE_KINDS:
        for S in R.SIZES:
            for M in (R.BATCHES if S < 500 else R.BATCHES[:2]):
                yield kind, S, M


@pytest.mark.parametrize("kind", R.TABLE_KINDS)
def test_knife_edge_share_of_the_gpu_scenes(kind):
    worst = 0.0
    for k, S, M in _cases():
        if k != kind:
            continue
        seed = R.case_seed(kind, S, M)
        case = R.make_case(kind, M, seed, waves=(0, 2, 1)[seed % 3])
        overlay = R.case_overlay(case, seed)
        scenes = R.case_scenes(case, S, overlay)
        knife = sum(int(sc.knife().sum()) for sc in scenes)
        share = knife / (M * S * S)
        worst = max(worst, share)
        assert share <= R.MAX_SHARE, (kind, S, M, share)
        assert all(np.isfinite(sc.margin).any() for sc in scenes)                      # there is something to get wrong
    assert 0.0 <= worst <= R.MAX_SHARE


def _launch_shape(M, S):
    """(rows per tile, tiles per frame) as include/aqua_render.h's host code picks them: what the big cases are chosen for"""
    qw = S // 4
    base_rows = min(max(256 // qw, 1), S)
    base_tiles = -(-S // base_rows)
    factor = min(max(M * base_tiles // 2048, 1), 8)
    rows = min(base_rows * factor, S)
    return rows, -(-S // rows)


@pytest.mark.parametrize("kind,S,M,N", R.BIG_CASES)
def test_knife_edge_share_of_the_large_batches(kind, S, M, N):
    case, overlay, worlds = R.big_case(kind, S, M, N)
    scenes = R.case_scenes(case, S, overlay)
    assert len(worlds) == M and set(worlds) == set(range(N))
    knife = sum(int(scenes[w].knife().sum()) for w in worlds)
    assert knife / (M * S * S) <= R.MAX_SHARE, (kind, S, M, knife / (M * S * S))


def test_large_batches_reach_the_launch_shapes_the_small_cases_do_not():
    for kind, S, M in _cases():
        rows, tiles = _launch_shape(M, S)
        assert rows * (S // 4) <= 256                                # one quad per lane: every small case
    shapes = {(S, M): _launch_shape(M, S) for _, S, M, _ in R.BIG_CASES}
    assert shapes == {(64, 1100): (32, 2), (64, 2100): (64, 1), (100, 1700): (80, 2), (500, 66): (16, 32)}
    quads_per_lane = {k: -(-rows * (k[0] // 4) // 256) for k, (rows, _) in shapes.items()}
    assert quads_per_lane == {(64, 1100): 2, (64, 2100): 4, (100, 1700): 8, (500, 66): 8}
    assert 100 % 80 == 20 and 500 % 16 == 4                         # ragged last tiles


def test_gpu_cases_cover_what_they_are_for():
    kinds = set()
    for kind, S, M in _cases():
        seed = R.case_seed(kind, S, M)
        kinds.add((0, 2, 1)[seed % 3])
        case = R.make_case(kind, M, seed)
        st = case["state"]
        if M >= 3:
            assert st[0, 2] == np.float32(np.pi) and st[1, 2] == np.float32(-np.pi) and st[1, 0] > 97.5           # half outside
            assert np.hypot(*(st[2, 3:5] - st[2, 0:2])) < 5.0                                                        # goal on boat
        if M >= 4:
            assert tuple(st[3, 5:7]) == (0.0, 0.0)
        if case["per_world"]:
            assert case["obstacles"].shape == (M, int(kind[9:]), 5)
            if M > 1:
                assert any(not np.array_equal(case["obstacles"][0], case["obstacles"][w]) for w in range(1, M))
    assert kinds == {0, 1, 2}
    pinned = {tuple(np.round(R.make_case("none", 1, s)["state"][0, [2, 5, 6]], 5)) for s in range(4)}
    assert len(pinned) == 4                                          # M == 1 cycles through the pinned worlds by seed


# ------------------------------------------------------------------ the facade without a GPU
def test_facade_without_a_gpu():
    import torch
    from gym_aqua.envs.aqua import AquaContinuousEnv, AquaEnv
    assert AquaEnv.metadata["render.modes"] == ["human", "rgb_array"] and "rgb_array" in AquaContinuousEnv.metadata["render.modes"]
    env = AquaEnv.__new__(AquaEnv)                                   # (the constructor needs a device)
    env._renderer = None
    for args in ((), ("human",)):
        with pytest.raises(NotImplementedError):
            env.render(*args)
    with pytest.raises(NotImplementedError):
        env.render(mode="ansi")
    if not torch.cuda.is_available():
        import types
        from aquaticgymenv_amd.render import FrameRenderer
        core = types.SimpleNamespace(torch=torch, device=torch.device("cpu"), per_world=False, obstacle_rows=np.zeros((0, 5)), ld=64, num_envs=1)
        with pytest.raises(RuntimeError, match="no CPU path"):
            FrameRenderer(core)
        core.device = torch.device("cuda:0")
        with pytest.raises(RuntimeError, match="no CPU path"):
            FrameRenderer(core)
        with pytest.raises(ValueError, match="size=18"):
            FrameRenderer(core, size=18)


def test_the_product_never_imports_the_tests_or_the_oracle():
    for path in ("aquaticgymenv_amd/render.py", "aquaticgymenv_amd/_render_capi.py", "gym_aqua/envs/aqua.py", "examples/render_episode.py"):
        src = open(os.path.join(ROOT, path)).read()
        assert not re.search(r"^\s*(from|import)\s+(tests|oracle)\b", src, re.M), path
    src = open(os.path.join(ROOT, "aquaticgymenv_amd", "render.py")).read()
    assert ".cpu()" not in src and "synchronize" not in src and ".item()" not in src       # nothing is read back
