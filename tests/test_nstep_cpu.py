"""CPU-only checks of libaqua_nstep.so (aquaticgymenv_amd/csrc/aqua_nstep.h), the n-step fold of the experience ring: it
builds and loads, exports what its header declares, rejects bad arguments before touching a device, has a build-table entry
of its own behind the pinned ones, and has no CPU path; aquanst_discount equals the numpy model; the model the GPU tests
compare against (tests/_nstep_model.py) is itself checked on hand-made rings, with n = 1 as the identity, and against a
per-world restatement; and the compiler's resource metadata of the kernel shows no scratch and no spills."""
import ctypes
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from tests import _isa
from tests import _nstep_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aquaticgymenv_amd", "csrc")
HEADER = os.path.join(CSRC, "aqua_nstep.h")
FAKE = 0x10000            # a "device pointer" for calls that must fail (or return) before anything dereferences it


@pytest.fixture(scope="module")
def ncapi():
    from aquaticgymenv_amd.build import build_library
    assert os.path.exists(build_library("nstep"))
    from aquaticgymenv_amd import _nstep_capi
    return _nstep_capi


# ------------------------------------------------------------------------------------------------ the library and its table
def test_library_builds_loads_and_exports_its_header(ncapi):
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(aquanst_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(ncapi.SYMBOLS) == {"aquanst_version", "aquanst_last_error", "aquanst_discount", "aquanst_fold"}, declared ^ set(ncapi.SYMBOLS)
    raw = ctypes.CDLL(ncapi.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    assert ncapi.lib.aquanst_version() == ncapi.ABI_VERSION == 1
    assert set(ncapi._SIGNATURES) == set(ncapi.SYMBOLS) - {"aquanst_version", "aquanst_last_error"}

    def define(name):
        return int(re.search(r"#define\s+%s\s+\(?(-?\d+)" % name, text).group(1))
    assert define("AQUANST_ABI_VERSION") == 1
    assert [define("AQUANST_E_" + n) for n in ("INVALID", "ALIGN", "NODEVICE")] == [-1, -2, -3] == [ncapi.E_INVALID, ncapi.E_ALIGN, ncapi.E_NODEVICE]
    from aquaticgymenv_amd import _lbank_capi, _replay_capi
    assert define("AQUANST_MAX_STEPS") == ncapi.MAX_STEPS == M.MAX_STEPS == 32 and define("AQUANST_CHUNK") == ncapi.CHUNK
    assert ncapi.MAX_STEPS % ncapi.CHUNK == 0
    assert define("AQUANST_MAX_CAPACITY") == ncapi.MAX_CAPACITY == _replay_capi.MAX_CAPACITY
    assert define("AQUANST_MAX_NETWORKS") == ncapi.MAX_NETWORKS == _lbank_capi.MAX_NETWORKS == 4096
    assert define("AQUANST_MAX_BATCH") == ncapi.MAX_BATCH == _replay_capi.MAX_BATCH == 1048576
    assert define("AQUANST_MAX_BLOCKS") == ncapi.MAX_BLOCKS == _replay_capi.MAX_BLOCKS and define("AQUANST_BLOCK") == ncapi.BLOCK == _replay_capi.BLOCK
    assert define("AQUANST_HYPER_WORDS") == ncapi.HYPER_WORDS == M.HYPER_WORDS == _lbank_capi.HYPER_WORDS
    assert _lbank_capi.HYPER_FIELDS[0] == "gamma"
    assert [define("AQUANST_ACT_U8"), define("AQUANST_ACT_F32X2")] == [ncapi.ACT_U8, ncapi.ACT_F32X2] == [_replay_capi.ACT_U8, _replay_capi.ACT_F32X2]
    assert float(re.search(r"#define\s+AQUANST_NO_GAMMA\s+\((-?[0-9.]+)\)", text).group(1)) == ncapi.NO_GAMMA == -1.0
    if shutil.which("nm"):
        nm = subprocess.run(["nm", "-D", "--defined-only", ncapi.LIB_PATH], capture_output=True, text=True)
        assert nm.returncode == 0 and set(re.findall(r"\b(aquanst_\w+)", nm.stdout)) == declared


def test_the_other_bindings_do_not_know_the_new_symbols(ncapi):
    from aquaticgymenv_amd import (_bank_capi, _capi, _episodes_capi, _fastpol_capi, _lbank_capi, _learner_capi, _pbt_capi, _policy_capi,
                                   _qmap_capi, _render_capi, _replay_capi, _segments_capi)
    for other in (_capi, _policy_capi, _learner_capi, _episodes_capi, _render_capi, _replay_capi, _bank_capi, _lbank_capi, _segments_capi,
                  _pbt_capi, _qmap_capi, _fastpol_capi):
        assert not any(s.startswith("aquanst_") for s in other.SYMBOLS)
        for name in ncapi.SYMBOLS:
            assert not hasattr(other.lib, name)


def test_build_table_entry_behind_the_pinned_tables():
    from aquaticgymenv_amd import build
    assert list(build.NSTEP_LIBRARIES) == ["nstep"]
    assert build.twelve_libraries() == ["hip", "policy", "learner", "episodes", "render", "replay", "bank", "lbank", "segments", "pbt", "qmap",
                                        "fastpol"]
    assert build.thirteen_libraries() == build.twelve_libraries() + ["nstep"] and len(build.thirteen_libraries()) == 13
    entry = build.library("nstep")
    assert entry is build.NSTEP_LIBRARIES["nstep"] and build.library("fastpol") is build.FAST_LIBRARIES["fastpol"]
    src = os.path.join(CSRC, "aqua_nstep.hip")
    lib = os.path.join(ROOT, "aquaticgymenv_amd", "lib", "libaqua_nstep.so")
    assert entry["src"] == [src] and entry["lib"] == lib and entry["cuid"] == "aqua_nstep"
    included = re.findall(r'#include "([a-z_]+\.hpp)"', open(src).read())
    assert included == ["aqua_host.hpp"] and '#include "aqua_nstep.h"' in open(src).read()
    assert entry["deps"] == [src, os.path.join(CSRC, "aqua_host.hpp"), HEADER] and all(os.path.exists(p) for p in entry["deps"])
    assert build.build_command("nstep") == [
        build.hipcc_path(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-fno-honor-nans", "-cuid=aqua_nstep",
        "-Wall", "-Wno-unused-function", "-o", lib + ".tmp", src]
    assert (build.NSTEP_SRC, build.NSTEP_DEPS, build.NSTEP_LIB, build.NSTEP_FLAGS) == (entry["src"], entry["deps"], entry["lib"], entry["flags"])
    assert callable(build.build_nstep) and build.nstep_needs_build() in (True, False)
    assert len({build.library(n)["lib"] for n in build.thirteen_libraries()}) == 13
    main = open(os.path.join(ROOT, "aquaticgymenv_amd", "build.py")).read().split('if __name__ == "__main__":')[1]
    assert "+ list(FAST_LIBRARIES) + list(NSTEP_LIBRARIES)" in main
    for name in build.twelve_libraries():
        assert not any("nstep" in d for d in build.library(name)["deps"]), name
    # the learners' shared device code is not part of this library: the fold hands them rows, it does not restate them
    assert "aqua_lrn.hpp" not in open(src).read()


def test_graft_entry_builds_and_checks_the_new_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    build_body = text.split("def build():")[1].split("def smoke():")[0]
    assert "NSTEP_LIBRARIES" in build_body and "_nstep_capi" in build_body and "aquanst_version" in build_body
    tables = re.findall(r"\b([A-Z]+_LIBRARIES)\b", build_body)
    assert tables[-1] == "NSTEP_LIBRARIES"                       # build()'s list ends with the new library
    import __graft_entry__ as entry
    from aquaticgymenv_amd import build
    assert entry.build() is None and os.path.exists(build.NSTEP_LIB)


# ------------------------------------------------------------------------------------------------ the C API without a device
ORDER = ("header", "s", "a", "r", "s2", "d", "ok", "ring_ld", "capacity", "kind", "N", "idx", "P", "B", "n", "gamma", "hyper", "out_s", "out_a",
         "out_r", "out_s2", "out_d", "out_ok", "out_ld", "out_len", "hyper_out")


def _fold(lib, **kw):
    a = dict(header=FAKE, s=FAKE + 0x1000, a=FAKE + 0x2000, r=FAKE + 0x3000, s2=FAKE + 0x4000, d=FAKE + 0x5000, ok=FAKE + 0x6000,
             ring_ld=1000, capacity=1000, kind=0, N=50, idx=FAKE + 0x7000, P=3, B=64, n=3, gamma=0.98, hyper=None,
             out_s=FAKE + 0x8000, out_a=FAKE + 0x9000, out_r=FAKE + 0xA000, out_s2=FAKE + 0xB000, out_d=FAKE + 0xC000,
             out_ok=FAKE + 0xD000, out_ld=192, out_len=FAKE + 0xE000, hyper_out=None)
    a.update(kw)
    return lib.aquanst_fold(*[a[name] for name in ORDER], None)


def test_argument_validation_without_touching_a_device(ncapi):
    """every call here fails (or returns) before the first HIP call: nothing is launched, no pointer is dereferenced"""
    lib = ncapi.lib
    table = dict(gamma=ncapi.NO_GAMMA, hyper=FAKE + 0xF000)
    big = ncapi.MAX_CAPACITY + 1
    nan, inf = float("nan"), float("inf")
    invalid = [dict(n=0), dict(n=-1), dict(n=ncapi.MAX_STEPS + 1), dict(n=2 ** 31 - 1),
               dict(N=51), dict(N=7), dict(N=0), dict(N=-50), dict(N=1001), dict(capacity=999, N=50),
               dict(out_ld=191), dict(out_ld=0), dict(out_ld=-1),
               dict(header=None), dict(s=None), dict(a=None), dict(r=None), dict(s2=None), dict(d=None), dict(ok=None), dict(idx=None),
               dict(out_s=None), dict(out_a=None), dict(out_r=None), dict(out_s2=None), dict(out_d=None), dict(out_ok=None),
               dict(gamma=0.98, hyper=FAKE + 0xF000), dict(gamma=0.0, hyper=FAKE + 0xF000),             # both
               dict(gamma=ncapi.NO_GAMMA), dict(gamma=nan), dict(gamma=inf), dict(gamma=1.5), dict(gamma=-0.1),  # neither, or no discount
               dict(hyper_out=FAKE + 0x10000),                                                           # no table to derive it from
               dict(hyper_out=FAKE + 0xF000, **table), dict(hyper_out=FAKE + 0xF000 + 8 * 23, **table),   # overlapping tables
               dict(capacity=0), dict(capacity=-5), dict(capacity=big, ring_ld=big), dict(ring_ld=999), dict(kind=2), dict(kind=-1),
               dict(P=0), dict(P=-1), dict(P=ncapi.MAX_NETWORKS + 1), dict(B=-1), dict(B=ncapi.MAX_BATCH + 1)]
    for kw in invalid:
        assert _fold(lib, **kw) == ncapi.E_INVALID, kw
        assert ncapi.last_error(), kw
    misaligned = [dict(header=FAKE + 4), dict(header=FAKE + 1), dict(s=FAKE + 0x1002), dict(r=FAKE + 0x3001), dict(s2=FAKE + 0x4002),
                  dict(idx=FAKE + 0x7002), dict(out_s=FAKE + 0x8001), dict(out_r=FAKE + 0xA002), dict(out_s2=FAKE + 0xB003),
                  dict(kind=1, a=FAKE + 0x2002), dict(kind=1, out_a=FAKE + 0x9001), dict(hyper=FAKE + 0xF004, gamma=ncapi.NO_GAMMA),
                  dict(hyper_out=FAKE + 0x20004, **table)]
    for kw in misaligned:
        assert _fold(lib, **kw) == ncapi.E_ALIGN, kw
        assert ncapi.last_error(), kw
    # the limits themselves pass the size checks (and then meet the alignment check); so does the table form
    assert _fold(lib, n=ncapi.MAX_STEPS, P=ncapi.MAX_NETWORKS, B=ncapi.MAX_BATCH, out_ld=2 ** 32, header=FAKE + 4) == ncapi.E_ALIGN
    assert _fold(lib, n=1, N=1000, header=FAKE + 4) == ncapi.E_ALIGN and _fold(lib, N=1, header=FAKE + 4) == ncapi.E_ALIGN
    assert _fold(lib, hyper_out=FAKE + 0xF000 + 8 * 24, header=FAKE + 4, **table) == ncapi.E_ALIGN
    assert _fold(lib, out_len=None, header=FAKE + 4) == ncapi.E_ALIGN
    # nothing to do: no launch, no device, neither idx nor the staged rows are needed
    assert _fold(lib, B=0, out_ld=0, idx=None, out_s=None, out_ok=None) == 0 and _fold(lib, B=0, **table) == 0
    # the Python layer turns E_INVALID into ValueError and everything else into the binding's error
    with pytest.raises(ValueError, match="^aquanst_fold: n=0"):
        ncapi.check(_fold(lib, n=0), "aquanst_fold")
    with pytest.raises(ValueError, match="no multiple of N"):
        ncapi.check(_fold(lib, N=7), "aquanst_fold")
    with pytest.raises(ncapi.AquaNStepError):
        ncapi.check(_fold(lib, header=FAKE + 4), "aquanst_fold")


def test_no_cpu_path_for_the_fold(ncapi):
    import torch
    from aquaticgymenv_amd.nstep import NStepReturns
    for bad in (object(), None, 3):
        with pytest.raises(ValueError):
            NStepReturns(bad, 3, 64)
    env = types.SimpleNamespace(num_envs=8, continuous=False)
    ring = types.SimpleNamespace(torch=torch, env=env, header=object(), device=torch.device("cpu"), capacity=64, _kind=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        NStepReturns(ring, 3, 64)
    if not torch.cuda.is_available():
        ring.device = torch.device("cuda:0")
        with pytest.raises(RuntimeError, match="no CPU path"):
            NStepReturns(ring, 3, 64)


# ------------------------------------------------------------------------------------------------ the discount
@pytest.mark.parametrize("gamma", [0.0, 0.5, 0.98, 0.999, 1.0])
def test_discount_equals_the_model(ncapi, gamma):
    for n in (1, 2, 5, ncapi.MAX_STEPS):
        got, want = ncapi.lib.aquanst_discount(gamma, n), M.discount(gamma, n)
        assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (gamma, n, got, want)
        assert ncapi.discount(gamma, n) == got
    g = float(np.float32(gamma))
    assert ncapi.lib.aquanst_discount(gamma, 1) == g                      # the float32 the learners round gamma to
    assert ncapi.lib.aquanst_discount(gamma, 2) == g * g
    # a window of 5 is four rounded products, not pow(): the two differ for 0.98
    if gamma == 0.98:
        assert ncapi.lib.aquanst_discount(gamma, 5) == (((g * g) * g) * g) * g
        assert any(ncapi.lib.aquanst_discount(gamma, n) != g ** n for n in range(2, 33))
        assert float(np.float32(ncapi.lib.aquanst_discount(gamma, 1))) == g


def test_discount_rejects_what_the_learner_rejects(ncapi):
    for gamma, n in ((-0.1, 3), (1.0001, 3), (float("nan"), 3), (float("inf"), 1), (0.98, 0), (0.98, ncapi.MAX_STEPS + 1), (0.98, -2)):
        assert ncapi.lib.aquanst_discount(gamma, n) == -1.0 and ncapi.last_error(), (gamma, n)
        with pytest.raises(ValueError):
            ncapi.discount(gamma, n)


# ------------------------------------------------------------------------------------------------ the model
def _hand_ring():
    """N = 2 worlds, capacity 8 (4 rounds), cursor 6: rounds 0 .. 2 written, round 3 never (ok == 0).
    world 0: r = 1, 2, 4 and no end; world 1: r = 10, 20, 40 with the episode ending in round 1"""
    ring = dict(capacity=8, s=np.arange(40, dtype=np.float32).reshape(5, 8), s2=100 + np.arange(40, dtype=np.float32).reshape(5, 8),
                r=np.array([1, 10, 2, 20, 4, 40, 0, 0], np.float32), a=np.array([0, 1, 2, 0, 1, 2, 0, 0], np.uint8),
                d=np.array([0, 0, 0, 3, 0, 0, 0, 0], np.uint8), ok=np.array([1, 1, 1, 1, 1, 1, 0, 0], np.uint8))
    return ring, np.array([6, 6, 4, 3], np.int64)


def test_the_model_on_a_hand_made_ring():
    ring, header = _hand_ring()
    idx = np.array([[0, 1, 2, 3, 4, 5, 6, -1, 8]], np.int32)
    out = M.fold(ring, header, 2, idx, 2, gamma=0.5)
    assert out["branch"] == [M.FULL, M.DONE_LAST, M.FULL, M.DONE_FIRST, M.FRONTIER, M.FRONTIER, M.NOT_OK, M.OUTSIDE, M.OUTSIDE]
    assert list(out["ok"]) == [1, 1, 1, 1, 0, 0, 0, 0, 0] and list(out["len"]) == [2, 2, 2, 1, 0, 0, 0, 0, 0]
    assert list(out["r"]) == [1 + 0.5 * 2, 10 + 0.5 * 20, 2 + 0.5 * 4, 20, 0, 0, 0, 0, 0]
    assert list(out["d"]) == [0, 3, 0, 3, 0, 0, 0, 0, 0]
    assert np.array_equal(out["s"][:, :4], ring["s"][:, :4]) and not out["s"][:, 4:].any()
    assert np.array_equal(out["s2"][:, :4], ring["s2"][:, [2, 3, 4, 3]]) and not out["s2"][:, 4:].any()
    assert list(out["a"]) == [0, 1, 2, 0, 0, 0, 0, 0, 0]
    # n = 3: world 0's window from round 0 is full (1 + 2 g + 4 g^2), from round 1 it runs past the newest round
    out = M.fold(ring, header, 2, idx, 3, gamma=0.5)
    assert out["branch"][:6] == [M.FULL, M.DONE_MIDDLE, M.FRONTIER, M.DONE_FIRST, M.FRONTIER, M.FRONTIER]
    assert list(out["r"][:4]) == [1 + 0.5 * 2 + 0.25 * 4, 10 + 0.5 * 20, 0, 20] and list(out["len"][:4]) == [3, 2, 0, 1]
    # a full ring that has wrapped: cursor 2, so round 0 is the newest and round 1 the oldest; the window of slot 6 wraps
    ring["ok"][6:] = 1
    ring["r"][6:] = (8, 80)
    header[:2] = (2, 8)
    out = M.fold(ring, header, 2, np.array([[6, 4, 0, 7, 2]], np.int32), 2, gamma=0.5)
    assert out["branch"] == [M.FULL, M.FULL, M.FRONTIER, M.FULL, M.FULL]
    assert list(out["r"]) == [8 + 0.5 * 1, 4 + 0.5 * 8, 0, 80 + 0.5 * 10, 2 + 0.5 * 4]
    assert np.array_equal(out["s2"][:, 0], ring["s2"][:, 0]) and np.array_equal(out["s"][:, 0], ring["s"][:, 6])
    # a cursor that is no multiple of N, or outside the ring: nothing is a sample
    for cursor in (3, 8, -2):
        header[0] = cursor
        out = M.fold(ring, header, 2, idx, 2, gamma=0.5)
        assert set(out["branch"]) == {M.BAD_CURSOR} and not out["ok"].any() and not out["r"].any() and not out["len"].any()
    # a broken chain: slot 2 (world 0, round 1) is no experience; with cursor 0 (round 3 the newest) slot 0's window meets it
    header[0] = 0
    ring["ok"][2] = 0
    out = M.fold(ring, header, 2, np.array([[0, 2, 4]], np.int32), 2, gamma=0.5)
    assert out["branch"] == [M.BROKEN, M.NOT_OK, M.FULL]
    # the table form: a discount per row, the other words copied
    hyper = np.arange(24, dtype=np.float64).reshape(3, 8) / 100
    hyper[:, 0] = (0.5, 0.25, 1.0)
    ring["ok"][2] = 1
    out = M.fold(ring, header, 2, np.array([[0], [0], [0]], np.int32), 3, hyper=hyper)
    assert list(out["r"]) == [1 + 0.5 * 2 + 0.25 * 4, 1 + 0.25 * 2 + 0.0625 * 4, 7]
    assert list(out["hyper"][:, 0]) == [0.125, 0.015625, 1.0] and np.array_equal(out["hyper"][:, 1:], hyper[:, 1:])


@pytest.mark.parametrize("continuous", [False, True], ids=["discrete", "continuous"])
def test_n_equal_one_is_the_identity_in_the_model(continuous):
    ring = M.crafted_ring(continuous=continuous)
    idx = np.arange(-2, 46, dtype=np.int32).reshape(3, 16)
    for header in ((21, 21, 14, 3), (0, 42, 35, 6), (14, 42, 7, 8)):
        out = M.fold(ring, np.array(header, np.int64), 7, idx, 1, gamma=0.98)
        flat = idx.reshape(-1)
        real = (flat >= 0) & (flat < 42)
        real[real] = ring["ok"][flat[real]] != 0
        at = np.where(real, flat, 0)
        assert np.array_equal(out["ok"], real.astype(np.uint8)) and np.array_equal(out["len"], real.astype(np.uint8))
        for name in ("s", "a", "r", "s2", "d"):
            want = np.ascontiguousarray(np.where(real, ring[name][..., at], np.zeros((), ring[name].dtype)))
            assert np.array_equal(out[name].view(np.uint8), want.view(np.uint8)), name
        assert set(out["branch"]) <= {M.FULL, M.DONE_FIRST, M.NOT_OK, M.OUTSIDE}
    assert M.discount(0.98, 1) == np.float64(np.float32(0.98))


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_the_model_is_the_per_world_walk(n):
    """window() against per_world(), which unrolls the ring into each world's transitions in the order they were made and
    follows them until done or n: the same slots for every slot of the crafted ring under every header of the GPU test, and
    for random rings"""
    rng = np.random.RandomState(n)
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
                branch, slots = M.window(ring, cursor, N, c, n)
                assert slots == M.per_world(ring, cursor, N, c, n), (N, cap, cursor, c, branch)
                assert (branch in M.VALID) == bool(slots) and all(0 <= x < cap for x in slots) and len(slots) <= n
                seen.add(branch)
    # (a window of 8 is longer than most of these rings have rounds: it is full or ends at its last step in few of them)
    want = {1: {M.FULL, M.DONE_FIRST, M.NOT_OK}, 8: {M.DONE_FIRST, M.DONE_MIDDLE, M.FRONTIER, M.BROKEN, M.NOT_OK}}
    assert seen >= want.get(n, {M.FULL, M.DONE_FIRST, M.DONE_LAST, M.FRONTIER, M.BROKEN, M.NOT_OK})


# ------------------------------------------------------------------------------------------------ the compiler's metadata
def test_codegen_has_no_scratch_no_spills_and_no_lds():
    """the resource metadata of the code object's notes: one instance of the kernel per action kind and source of gamma,
    none with a private segment, a spilled register or LDS"""
    isa = _isa.kernels("nstep")
    assert len(isa) == 4 and all("nst_fold_kernel" in name for name in isa), sorted(isa)
    for name, k in isa.items():
        m = k["meta"]
        print("registers:", name, m)
        assert m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0 and m["agpr_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)                 # four wavefronts per SIMD at least
        assert k["stats"]["ScratchSize"] == 0, (name, k["stats"])
