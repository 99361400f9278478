"""CPU-only checks of libaqua_lbank.so (include/aqua_lbank.h), the learner bank: it builds and loads, exports what its
header declares and leaves the other seven libraries alone, has a build-table entry of its own behind the pinned tables,
shares the learner's device code (one statement in csrc/aqua_lrn.hpp), rejects bad arguments before touching a device,
validates and packs the hyper-parameter table on the host, sizes its workspace as P regions of the learner's, keeps the
weight gradients on v_mfma_f32_32x32x2_f32 without scratch or spills in six kernels, and has no CPU path."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _isa
from tests import _lbank as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x100000           # a "device pointer" for calls that must fail (or return) before anything dereferences it
STACK = 0x1000000         # far enough apart for 64 stacked networks


@pytest.fixture(scope="module")
def ncapi():
    from aquaticgymenv_amd.build import build_library
    assert os.path.exists(build_library("lbank"))
    from aquaticgymenv_amd import _lbank_capi
    return _lbank_capi


@pytest.fixture(scope="module")
def lcapi():
    from aquaticgymenv_amd.build import build_learner, build_policy
    assert os.path.exists(build_policy()) and os.path.exists(build_learner())
    from aquaticgymenv_amd import _learner_capi
    return _learner_capi


@pytest.fixture(scope="module")
def isa():
    return _isa.kernels("lbank")


def test_library_builds_loads_and_exports_its_header(ncapi, lcapi):
    text = open(os.path.join(ROOT, "include", "aqua_lbank.h")).read()
    declared = set(re.findall(r"\b(aqualbank_[a-z0-9_]+)\s*\(", text))
    assert declared == set(ncapi.SYMBOLS), declared ^ set(ncapi.SYMBOLS)
    raw = ctypes.CDLL(ncapi.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    assert ncapi.lib.aqualbank_version() == ncapi.ABI_VERSION == 1
    assert set(ncapi._SIGNATURES) == set(ncapi.SYMBOLS) - {"aqualbank_version", "aqualbank_last_error"}

    def define(name):
        return int(re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, text).group(1))
    assert define("AQUALBANK_ABI_VERSION") == 1
    assert [define("AQUALBANK_E_" + n) for n in ("INVALID", "ALIGN", "NODEVICE")] == [-1, -2, -3]
    assert [ncapi.E_INVALID, ncapi.E_ALIGN, ncapi.E_NODEVICE] == [-1, -2, -3]
    assert define("AQUALBANK_PARAMS") == ncapi.PARAMS == lcapi.PARAMS == K.PARAMS
    assert define("AQUALBANK_MAX_BATCH") == ncapi.MAX_BATCH == lcapi.MAX_BATCH
    assert define("AQUALBANK_MAX_NETWORKS") == ncapi.MAX_NETWORKS == 4096
    assert define("AQUALBANK_MAX_CAPACITY") == ncapi.MAX_CAPACITY == 2 ** 31 - 1
    assert define("AQUALBANK_HYPER_FIELDS") == len(ncapi.HYPER_FIELDS) == 6 and define("AQUALBANK_HYPER_WORDS") == ncapi.HYPER_WORDS == 8
    assert define("AQUALBANK_STREAM") == ncapi.STREAM == lcapi.STREAM == 6 and define("AQUALBANK_ATTEMPTS") == ncapi.ATTEMPTS == 4


def test_the_other_bindings_and_headers_do_not_know_the_new_symbols(ncapi):
    from aquaticgymenv_amd import _bank_capi, _capi, _episodes_capi, _learner_capi, _policy_capi, _render_capi, _replay_capi
    for other in (_capi, _policy_capi, _learner_capi, _episodes_capi, _render_capi, _replay_capi, _bank_capi):
        assert not any(s.startswith("aqualbank_") for s in other.SYMBOLS)
        for name in ncapi.SYMBOLS:
            assert not hasattr(other.lib, name)
    for other in ("aqua_hip.h", "aqua_policy.h", "aqua_learner.h", "aqua_episodes.h", "aqua_render.h", "aqua_replay.h", "aqua_bank.h"):
        assert "aqualbank_" not in open(os.path.join(ROOT, "include", other)).read().lower()
    # the learner keeps its four symbols
    assert _learner_capi.SYMBOLS == ("aqualrn_version", "aqualrn_last_error", "aqualrn_workspace_bytes", "aqualrn_update_f32")


def test_build_table_entry_and_the_pinned_lists():
    from aquaticgymenv_amd import build
    assert list(build.POPULATION_LIBRARIES) == ["lbank"]
    assert build.all_libraries() == ["hip", "policy", "learner", "episodes", "render"]
    assert build.every_library() == build.all_libraries() + ["replay"]
    assert build.each_library() == build.every_library() + ["bank"]
    assert build.libraries() == build.each_library() + ["lbank"] and len(build.libraries()) == 8
    entry = build.library("lbank")
    assert entry is build.POPULATION_LIBRARIES["lbank"] and build.library("bank") is build.BANK_LIBRARIES["bank"]
    with pytest.raises(KeyError):
        build.library("nothing")
    csrc = os.path.join(ROOT, "aquaticgymenv_amd", "csrc")
    src = os.path.join(csrc, "aqua_lbank.hip")
    lib = os.path.join(ROOT, "aquaticgymenv_amd", "lib", "libaqua_lbank.so")
    headers = ("aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp", "aqua_lrn.hpp")
    assert entry["src"] == [src] and entry["lib"] == lib and entry["cuid"] == "aqua_lbank"
    assert entry["deps"] == [src] + [os.path.join(csrc, h) for h in headers] + [os.path.join(ROOT, "include", "aqua_lbank.h")]
    assert all(os.path.exists(p) for p in entry["deps"])
    assert build.build_command("lbank") == [
        build.hipcc_path(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-fno-honor-nans", "-cuid=aqua_lbank",
        "-Wall", "-Wno-unused-function", "-o", lib + ".tmp", src]
    assert (build.LBANK_SRC, build.LBANK_DEPS, build.LBANK_LIB, build.LBANK_FLAGS) == (entry["src"], entry["deps"], entry["lib"], entry["flags"])
    assert callable(build.build_lbank) and build.lbank_needs_build() in (True, False)
    # both includers of the shared device code name it as a dependency, and it is stated once
    for name in ("learner", "lbank"):
        e = build.library(name)
        included = set(re.findall(r'#include "([a-z_]+\.hpp)"', open(e["src"][0]).read()))
        assert included == set(headers) and os.path.join(csrc, "aqua_lrn.hpp") in e["deps"], name
    texts = {name: open(os.path.join(csrc, name)).read() for name in sorted(os.listdir(csrc))}
    for once in ("void grad_body(", "void apply_body(", "WS_STRIDE = 4744", "struct GradArgs", "struct ApplyArgs"):
        assert {name: t.count(once) for name, t in texts.items() if once in t} == {"aqua_lrn.hpp": 1}, once
    for name in ("aqua_learner.hip", "aqua_lbank.hip"):
        assert "v_mfma" not in texts[name] and "__builtin_amdgcn_mfma" not in texts[name] and "grad_body<" in texts[name], name


def test_graft_entry_builds_and_checks_the_new_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "every_library()" in text and "POPULATION_LIBRARIES" in text and "_lbank_capi" in text and "aqualbank_version" in text


def _update(lib, **kw):
    a = dict(theta=FAKE, target=FAKE + STACK, m=FAKE + 2 * STACK, v=FAKE + 3 * STACK, t=FAKE + 4 * STACK, P=3, s=FAKE, a=FAKE, r=FAKE,
             s2=FAKE, d=FAKE, ok=FAKE, ld=1000, size=900, idx=FAKE, B=64, strategy=0, hyper=FAKE, blob=None, blob_t=None, perm=None,
             blob_floats=0, ws=FAKE, ws_bytes=1 << 40, idx_out=None, grad=None, loss=None)
    a.update(kw)
    return lib.aqualbank_update_f32(a["theta"], a["target"], a["m"], a["v"], a["t"], a["P"], a["s"], a["a"], a["r"], a["s2"], a["d"],
                                    a["ok"], a["ld"], a["size"], a["idx"], a["B"], a["strategy"], a["hyper"], a["blob"], a["blob_t"],
                                    a["perm"], a["blob_floats"], a["ws"], a["ws_bytes"], a["idx_out"], a["grad"], a["loss"], None)


def test_update_validates_before_touching_a_device(ncapi):
    lib = ncapi.lib
    stack3 = 3 * 4 * K.PARAMS
    invalid = [dict(P=0), dict(P=-1), dict(P=ncapi.MAX_NETWORKS + 1), dict(theta=None), dict(target=None), dict(m=None), dict(v=None),
               dict(t=None), dict(m=FAKE), dict(target=FAKE + stack3 - 4), dict(v=FAKE + 2 * STACK + 4 * K.PARAMS), dict(B=-1),
               dict(B=ncapi.MAX_BATCH + 1), dict(ld=-1), dict(size=-1), dict(size=1001), dict(ld=2 ** 31, size=5), dict(strategy=-1),
               dict(strategy=4), dict(strategy=8), dict(strategy=32), dict(strategy=16 | 4), dict(strategy=-16), dict(hyper=None),
               dict(idx=None), dict(blob=FAKE + 5 * STACK), dict(blob=FAKE + 5 * STACK, perm=FAKE, blob_floats=100),
               dict(blob=FAKE + 5 * STACK, blob_t=FAKE + 5 * STACK, perm=FAKE, blob_floats=4804),
               dict(blob=FAKE + 5 * STACK, blob_t=FAKE + 5 * STACK + 4 * 4804, perm=FAKE, blob_floats=4804),
               dict(blob=FAKE + 5 * STACK, perm=FAKE, blob_floats=2 ** 31), dict(s=None), dict(ok=None), dict(a=None), dict(ws=None),
               dict(ws_bytes=lib.aqualbank_workspace_bytes(3, 64) - 1)]
    for kw in invalid:
        assert _update(lib, **kw) == ncapi.E_INVALID, kw
        assert ncapi.last_error(), kw
    # a single network's arrays may follow each other directly; the same distance overlaps for three
    near = dict(target=FAKE + 4 * K.PARAMS, m=FAKE + 8 * K.PARAMS, v=FAKE + 12 * K.PARAMS, ws=FAKE + 8)
    assert _update(lib, P=1, **near) == ncapi.E_ALIGN and _update(lib, P=3, **near) == ncapi.E_INVALID
    misaligned = [dict(theta=FAKE + 2), dict(v=FAKE + 3 * STACK + 1), dict(t=FAKE + 4 * STACK + 4), dict(hyper=FAKE + 4), dict(s=FAKE + 1),
                  dict(r=FAKE + 2), dict(s2=FAKE + 3), dict(idx=FAKE + 2), dict(idx_out=FAKE + 1), dict(grad=FAKE + 2), dict(loss=FAKE + 2),
                  dict(ws=FAKE + 8), dict(blob=FAKE + 5 * STACK + 2, perm=FAKE, blob_floats=4804),
                  dict(blob=FAKE + 5 * STACK, perm=FAKE + 2, blob_floats=4804)]
    for kw in misaligned:
        assert _update(lib, **kw) == ncapi.E_ALIGN, kw
        assert ncapi.last_error(), kw
    # B == 0: nothing to do, no launch, no device, no ring, idx or workspace needed; every strategy with either loss form
    assert _update(lib, B=0) == 0
    for strategy in (0, 1, 2, 3):
        assert _update(lib, B=0, strategy=strategy | 16) == 0
    assert _update(lib, B=0, s=None, a=None, r=None, s2=None, d=None, ok=None, idx=None, ws=None, ws_bytes=0, ld=0, size=0) == 0
    with pytest.raises(ValueError):
        ncapi.check(_update(lib, P=0), "aqualbank_update_f32")
    with pytest.raises(ncapi.AquaLearnerBankError):
        ncapi.check(_update(lib, ws=FAKE + 8), "aqualbank_update_f32")


def _draw(lib, **kw):
    a = dict(header=FAKE, ok=FAKE, capacity=480, N=120, seg=40, P=3, t=FAKE, seed=FAKE, idx=FAKE, B=64)
    a.update(kw)
    return lib.aqualbank_draw(a["header"], a["ok"], a["capacity"], a["N"], a["seg"], a["P"], a["t"], a["seed"], a["idx"], a["B"], None)


def test_draw_validates_before_touching_a_device(ncapi):
    lib = ncapi.lib
    invalid = [dict(header=None), dict(ok=None), dict(t=None), dict(seed=None), dict(P=0), dict(P=ncapi.MAX_NETWORKS + 1), dict(capacity=0),
               dict(capacity=2 ** 31), dict(N=0), dict(N=-5), dict(N=481), dict(capacity=481), dict(capacity=500), dict(N=119), dict(seg=0),
               dict(seg=-1), dict(B=-1), dict(B=ncapi.MAX_BATCH + 1), dict(idx=None)]
    for kw in invalid:
        assert _draw(lib, **kw) == ncapi.E_INVALID, kw
        assert ncapi.last_error(), kw
    assert _draw(lib, capacity=500) == ncapi.E_INVALID and "multiple" in ncapi.last_error()
    for kw in (dict(header=FAKE + 4), dict(t=FAKE + 4), dict(seed=FAKE + 2), dict(idx=FAKE + 2)):
        assert _draw(lib, **kw) == ncapi.E_ALIGN, kw
        assert ncapi.last_error(), kw
    # B == 0 returns before any launch; a segment far beyond N and more networks than own a world are fine
    assert _draw(lib, B=0) == 0 and _draw(lib, B=0, idx=None, seg=2 ** 62, P=4096) == 0 and _draw(lib, B=0, N=480) == 0


def test_pack_hyper_rejects_each_bad_field_and_names_the_network(ncapi):
    good = [0.98, 0.005, 1e-3, 0.9, 0.999, 1e-7]
    table = ncapi.pack_hyper(np.array([good, K.HYPER3[1], K.HYPER3[2]]))
    assert table.shape == (3, 8) and table.dtype == np.float64
    assert np.array_equal(table[:, :6], np.array([good, K.HYPER3[1], K.HYPER3[2]])) and bool((table[:, 6:] == 0).all())
    assert np.array_equal(ncapi.pack_hyper(np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 5e-324]]))[0, :6], [0, 0, 0, 0, 0, 5e-324])   # the ends
    assert np.array_equal(ncapi.pack_hyper(np.array([[1.0, 1.0, 1e300, 0.0, 0.0, 1.0]]))[0, :3], [1.0, 1.0, 1e300])
    nan, inf = float("nan"), float("inf")
    bad = {"gamma": (-0.1, 1.5, nan, inf), "tau": (-0.1, 1.01, nan), "lr": (-1e-3, nan, inf), "beta1": (1.0, -0.1, nan),
           "beta2": (1.0, -1e-9, nan), "eps": (0.0, -1e-7, nan, inf)}
    for field, values in bad.items():
        k = ncapi.HYPER_FIELDS.index(field)
        for value in values:
            for who in (0, 2):
                rows = np.array([good, good, good])
                rows[who, k] = value
                out = np.full((3, 8), 7.0)
                rc = ncapi.lib.aqualbank_pack_hyper(rows.ctypes.data, 3, out.ctypes.data)
                msg = ncapi.last_error()
                assert rc == ncapi.E_INVALID and ("network %d: %s=" % (who, field)) in msg, (field, value, who, msg)
                assert bool((out == 7.0).all())                         # nothing is written unless every row is valid
                with pytest.raises(ValueError, match="network %d" % who):
                    ncapi.pack_hyper(rows)
    one = np.array([good])
    out = np.zeros((1, 8))
    assert ncapi.lib.aqualbank_pack_hyper(None, 1, out.ctypes.data) == -1 and ncapi.lib.aqualbank_pack_hyper(one.ctypes.data, 1, None) == -1
    assert ncapi.lib.aqualbank_pack_hyper(one.ctypes.data, 0, out.ctypes.data) == -1
    assert ncapi.lib.aqualbank_pack_hyper(one.ctypes.data, ncapi.MAX_NETWORKS + 1, out.ctypes.data) == -1
    assert ncapi.lib.aqualbank_pack_hyper(one.ctypes.data + 4, 1, out.ctypes.data) == -2
    with pytest.raises(ValueError):
        ncapi.pack_hyper(np.zeros((3, 5)))


def test_workspace_is_p_regions_of_the_learners(ncapi, lcapi):
    ws, one = ncapi.lib.aqualbank_workspace_bytes, lcapi.lib.aqualrn_workspace_bytes
    batches = list(range(0, 200)) + [2 ** k + d for k in range(8, 21) for d in (-1, 0, 1) if 2 ** k + d <= ncapi.MAX_BATCH]
    for P in (1, 2, 3, 600, ncapi.MAX_NETWORKS):
        sizes = [ws(P, b) for b in batches]
        assert sizes == [P * one(b) for b in batches] and all(s % 16 == 0 and s > 0 for s in sizes)
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert all(ws(P + 1, 64) > ws(P, 64) for P in range(1, 50))
    assert one(64) % 16 == 0                                          # every region starts 16-byte aligned
    for P, B in ((0, 64), (-1, 64), (ncapi.MAX_NETWORKS + 1, 64), (3, -1), (3, ncapi.MAX_BATCH + 1)):
        assert ws(P, B) == 0


def test_codegen_six_kernels_on_the_f32_mfma_without_scratch(isa):
    grad = {n: k for n, k in isa.items() if "lbank_grad_kernel" in n}
    apply_ = {n: k for n, k in isa.items() if "lbank_apply_kernel" in n}
    draw = {n: k for n, k in isa.items() if "lbank_draw_kernel" in n}
    assert len(grad) == 4 and len(apply_) == 1 and len(draw) == 1 and len(isa) == 6, sorted(isa)
    for name, k in isa.items():
        m = k["meta"]
        assert m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert "scratch_" not in k["body"], name
        assert not re.search(r"v_mfma_\w*(bf16|f16|fp8|bf8|f8f6f4|i8)|v_cvt_\w*(bf16|f16|fp8|bf8|bf6|fp6|fp4)", k["body"]), name
        assert not re.search(r"atomic_\w*(f32|f64)|atomic_(fadd|fmin|fmax|pk_add)", k["body"]), name      # no float atomics
        assert m["group_segment_fixed_size"] <= 65536, (name, m)
    counts = {n: len(re.findall(r"\bv_mfma_f32_32x32x2_f32\b", k["body"])) for n, k in grad.items()}
    print("static v_mfma_f32_32x32x2_f32 per gradient kernel:", counts)
    print("registers:", {n: (k["meta"]["vgpr_count"], k["meta"]["agpr_count"], k["meta"]["sgpr_count"]) for n, k in isa.items()})
    # the learner's: per tile 70 per forward (two of them, three for "double"), 64 for dh1, 16 k-steps x 10
    learner = _isa.kernels("learner")
    theirs = sorted(len(re.findall(r"\bv_mfma_f32_32x32x2_f32\b", k["body"])) for n, k in learner.items() if "lrn_grad_kernel" in n)
    assert sorted(counts.values()) == theirs == [2 * 70 + 64 + 160] * 3 + [3 * 70 + 64 + 160], (counts, theirs)
    for k in list(apply_.values()) + list(draw.values()):
        assert "v_mfma" not in k["body"]
    # the same LDS as the learner's kernels: the bodies are the same code
    assert sorted(k["meta"]["group_segment_fixed_size"] for k in grad.values()) == \
        sorted(k["meta"]["group_segment_fixed_size"] for n, k in learner.items() if "lrn_grad_kernel" in n)


def test_no_cpu_fallback_for_the_learner_bank(ncapi):
    import torch
    from aquaticgymenv_amd.lbank import DQNLearnerBank
    with pytest.raises(ValueError):
        DQNLearnerBank(object())
    if not torch.cuda.is_available():
        from aquaticgymenv_amd.qbank import QNetworkBank
        from tests import _learner as L
        with pytest.raises(RuntimeError):
            DQNLearnerBank(QNetworkBank([L.int_layers(), L.int_layers(salt=1)], 32, device="cuda:0"))
    for name in ("lbank.py", "trainer.py"):
        src = open(os.path.join(ROOT, "aquaticgymenv_amd", name)).read()
        assert "autograd" not in src and "torch.optim" not in src and "backward(" not in src and "matmul" not in src and " @ " not in src, name


def test_the_draw_model_confines_every_network_to_its_own_slots():
    """a self-check of tests/_lbank.py::draw_model (it runs no code of the library): slots of the right network, real
    transitions only, nothing from beyond the filled rounds, and the one-network case is tests/_learner.py::drawn"""
    from tests import _learner as L
    rng = np.random.RandomState(0)
    cap, n = 480, 120
    ok = (rng.rand(cap) >= 0.3).astype(np.uint8)
    for P, seg in ((3, 40), (3, 50), (5, 40)):
        got = K.draw_model(list(range(P)), [0] * P, 200, 240, ok, cap, n, seg)
        for p in range(P):
            live = got[p][got[p] >= 0]
            assert (live.size == 0) == (p * seg >= n)
            assert bool((K.owner(live, n, seg) == p).all()) and bool((ok[live] != 0).all()) and bool((live < 240).all())
        assert bool((K.draw_model(list(range(P)), [0] * P, 50, 119, ok, cap, n, seg) == -1).all())       # not one full round
    one = K.draw_model([9], [4], 300, 360, ok, cap, n, 2 ** 40)[0]
    assert np.array_equal(one, L.drawn(9, 5, 300, dict(ok=ok, size=360)))
