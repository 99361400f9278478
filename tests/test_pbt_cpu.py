"""CPU-only checks of libaqua_pbt.so (aquaticgymenv_amd/include/aqua_pbt.h), selection among the networks of a population:
it builds and loads, exports what its header declares and leaves the other nine libraries alone, has a build-table entry of
its own behind the pinned tables, rejects bad arguments before touching a device, its kernels have no scratch, spill or
floating-point atomic, the numpy model keeps its own invariants, and there is no CPU path."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _isa
from tests import _pbt as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "aquaticgymenv_amd", "include", "aqua_pbt.h")
FAKE = 0x10000000         # a "device pointer" for calls that must fail before anything dereferences it
GAP = 0x10000000          # between two fake arrays: more than the largest of them (4096 x 4804 floats)


@pytest.fixture(scope="module")
def tcapi():
    from aquaticgymenv_amd.build import build_library
    assert os.path.exists(build_library("pbt"))
    from aquaticgymenv_amd import _pbt_capi
    return _pbt_capi


def test_library_builds_loads_and_exports_its_header(tcapi):
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(aquapbt_[a-z0-9_]+)\s*\(", text))
    assert declared == set(tcapi.SYMBOLS) == {"aquapbt_version", "aquapbt_last_error", "aquapbt_select"}, declared ^ set(tcapi.SYMBOLS)
    raw = ctypes.CDLL(tcapi.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    assert tcapi.lib.aquapbt_version() == tcapi.ABI_VERSION == 1
    assert set(tcapi._SIGNATURES) == set(tcapi.SYMBOLS) - {"aquapbt_version", "aquapbt_last_error"}

    def define(name):
        return int(re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, text).group(1))
    assert define("AQUAPBT_ABI_VERSION") == 1
    assert [define("AQUAPBT_E_" + n) for n in ("INVALID", "ALIGN", "NODEVICE")] == [-1, -2, -3]
    assert [tcapi.E_INVALID, tcapi.E_ALIGN, tcapi.E_NODEVICE] == [-1, -2, -3]
    from aquaticgymenv_amd import _lbank_capi, _segments_capi
    assert define("AQUAPBT_MAX_NETWORKS") == tcapi.MAX_NETWORKS == _lbank_capi.MAX_NETWORKS == _segments_capi.MAX_SEGMENTS == 4096
    assert define("AQUAPBT_PARAMS") == tcapi.PARAMS == _lbank_capi.PARAMS == T.PARAMS == 4739
    assert define("AQUAPBT_HEADER") == tcapi.HEADER == 4 and define("AQUAPBT_COUNTS") == tcapi.COUNTS == _segments_capi.COUNTS == 8
    assert define("AQUAPBT_HYPER_WORDS") == tcapi.HYPER_WORDS == _lbank_capi.HYPER_WORDS == T.HYPER_WORDS == 8
    assert define("AQUAPBT_HYPER_GAMMA") == tcapi.HYPER_GAMMA == T.HYPER_GAMMA == _lbank_capi.HYPER_FIELDS.index("gamma")
    assert define("AQUAPBT_HYPER_LR") == tcapi.HYPER_LR == T.HYPER_LR == _lbank_capi.HYPER_FIELDS.index("lr")
    assert define("AQUAPBT_MAX_BLOB") == tcapi.MAX_BLOB
    # the Philox stream is one no other library draws from
    assert define("AQUAPBT_STREAM") == tcapi.STREAM == T.STREAM == 7
    from aquaticgymenv_amd import _bank_capi, _episodes_capi, _learner_capi, _policy_capi, _replay_capi
    taken = {m.STREAM for m in (_bank_capi, _episodes_capi, _learner_capi, _policy_capi, _replay_capi, _lbank_capi)} | {0, 1, 3, 4}
    assert tcapi.STREAM not in taken
    # the arguments of the declaration and of the binding, one for one
    decl = re.search(r"int aquapbt_select\((.*?)\);", text, re.S).group(1)
    kinds = []
    for arg in (a.strip() for a in decl.split(",")):
        kinds.append(ctypes.c_void_p if "*" in arg else {"int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double}[arg.split()[0]])
    argtypes, restype = tcapi._SIGNATURES["aquapbt_select"]
    assert argtypes == kinds and restype is ctypes.c_int and len(kinds) == 31
    # the exported dynamic symbols with the prefix are exactly the declared ones
    import shutil
    import subprocess
    if shutil.which("nm"):
        nm = subprocess.run(["nm", "-D", "--defined-only", tcapi.LIB_PATH], capture_output=True, text=True)
        assert nm.returncode == 0 and set(re.findall(r"\b(aquapbt_\w+)", nm.stdout)) == declared


def test_the_other_nine_bindings_and_headers_do_not_know_the_new_symbols(tcapi):
    from aquaticgymenv_amd import (_bank_capi, _capi, _episodes_capi, _lbank_capi, _learner_capi, _policy_capi, _render_capi, _replay_capi,
                                   _segments_capi)
    others = (_capi, _policy_capi, _learner_capi, _episodes_capi, _render_capi, _replay_capi, _bank_capi, _lbank_capi, _segments_capi)
    for other in others:
        assert not any(s.startswith("aquapbt_") for s in other.SYMBOLS)
        for name in tcapi.SYMBOLS:
            assert not hasattr(other.lib, name)
    for other in os.listdir(os.path.join(ROOT, "include")):
        assert "aquapbt_" not in open(os.path.join(ROOT, "include", other)).read().lower()
    assert os.listdir(os.path.join(ROOT, "aquaticgymenv_amd", "include")) == ["aqua_pbt.h"]


def test_build_table_entry_and_the_lists():
    from aquaticgymenv_amd import build
    assert list(build.SELECTION_LIBRARIES) == ["pbt"]
    assert build.ten_libraries() == build.nine_libraries() + ["pbt"] and len(build.ten_libraries()) == 10
    assert "pbt" not in build.nine_libraries()
    entry = build.library("pbt")
    assert entry is build.SELECTION_LIBRARIES["pbt"] and build.library("segments") is build.SEGMENT_LIBRARIES["segments"]
    with pytest.raises(KeyError):
        build.library("nothing")
    csrc = os.path.join(ROOT, "aquaticgymenv_amd", "csrc")
    src = os.path.join(csrc, "aqua_pbt.hip")
    lib = os.path.join(ROOT, "aquaticgymenv_amd", "lib", "libaqua_pbt.so")
    assert entry["src"] == [src] and entry["lib"] == lib and entry["cuid"] == "aqua_pbt"
    assert entry["deps"] == [src, os.path.join(csrc, "aqua_device.hpp"), os.path.join(csrc, "aqua_host.hpp"), HEADER]
    assert all(os.path.exists(p) for p in entry["deps"])
    assert build.build_command("pbt") == [
        build.hipcc_path(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-fno-honor-nans", "-cuid=aqua_pbt",
        "-Wall", "-Wno-unused-function", "-o", lib + ".tmp", src]
    assert (build.PBT_SRC, build.PBT_DEPS, build.PBT_LIB, build.PBT_FLAGS) == (entry["src"], entry["deps"], entry["lib"], entry["flags"])
    assert callable(build.build_pbt) and build.pbt_needs_build() in (True, False)
    text = open(src).read()
    assert set(re.findall(r'#include "([a-z_]+\.hpp)"', text)) == {"aqua_device.hpp", "aqua_host.hpp"}
    assert '#include "../include/aqua_pbt.h"' in text
    assert len({build.library(n)["lib"] for n in build.ten_libraries()}) == 10
    main = open(os.path.join(ROOT, "aquaticgymenv_amd", "build.py")).read().split('if __name__ == "__main__":')[1]
    assert "nine_libraries() + list(SELECTION_LIBRARIES)" in main


def test_graft_entry_builds_and_checks_the_new_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "every_library()" in text and "list(SELECTION_LIBRARIES)" in text and "_pbt_capi" in text and "aquapbt_version" in text


POINTERS = ("score", "seg_counts", "header", "mark", "origin", "parent", "theta", "theta_target", "m", "v", "t", "blob_online", "blob_target",
            "hyper", "eps_state", "eps_out")
ORDER = ("score", "seg_counts", "P", "header", "mark", "origin", "parent", "theta", "theta_target", "m", "v", "t", "blob_online", "blob_target",
         "blob_floats", "hyper", "eps_state", "eps_out", "fraction", "ready", "every", "seed", "lr_f0", "lr_f1", "lr_lo", "lr_hi",
         "g_f0", "g_f1", "g_lo", "g_hi")


def _select(lib, **kw):
    """a call that must fail before the first HIP call: the pointers are not memory"""
    a = {name: FAKE + i * GAP for i, name in enumerate(POINTERS)}
    a.update(P=64, blob_floats=4804, fraction=0.25, ready=100, every=1, seed=0, lr_f0=0.8, lr_f1=1.25, lr_lo=1e-5, lr_hi=0.1,
             g_f0=0.8, g_f1=1.25, g_lo=0.5, g_hi=0.999)
    a.update(kw)
    return lib.aquapbt_select(*[a[name] for name in ORDER], None)


def test_select_validates_before_touching_a_device(tcapi):
    """every call here fails: nothing is launched and the pointers are never dereferenced"""
    lib = tcapi.lib
    nan, inf = float("nan"), float("inf")
    invalid = [{name: None} for name in POINTERS if name not in ("eps_state", "eps_out")]
    invalid += [dict(P=0), dict(P=-1), dict(P=tcapi.MAX_NETWORKS + 1), dict(fraction=0.0), dict(fraction=0.51), dict(fraction=nan),
                dict(fraction=-0.25), dict(ready=0), dict(ready=-1), dict(every=0), dict(every=-5),
                dict(lr_lo=0.1, lr_hi=1e-5), dict(lr_lo=0.0), dict(lr_lo=-1.0), dict(lr_hi=inf), dict(lr_lo=nan),
                dict(g_lo=0.999, g_hi=0.5), dict(g_lo=-0.1), dict(g_hi=1.5), dict(g_hi=nan),
                dict(lr_f0=0.0), dict(lr_f1=-1.0), dict(lr_f0=nan), dict(lr_f1=inf), dict(g_f0=0.0), dict(g_f1=nan),
                dict(eps_state=None), dict(eps_out=None),
                dict(blob_floats=0), dict(blob_floats=4803), dict(blob_floats=-4), dict(blob_floats=tcapi.MAX_BLOB + 4)]
    stack = 64 * 4 * tcapi.PARAMS
    overlapping = [dict(theta_target=FAKE + 6 * GAP), dict(m=FAKE + 6 * GAP + stack - 4), dict(v=FAKE + 8 * GAP - stack + 4),
                   dict(blob_target=FAKE + 11 * GAP + 64 * 4 * 4804 - 16), dict(t=FAKE + 6 * GAP + 8), dict(hyper=FAKE + 9 * GAP + stack - 8),
                   dict(parent=FAKE + 4 * GAP), dict(mark=FAKE + 2 * GAP + 24), dict(score=FAKE + 15 * GAP), dict(seg_counts=FAKE + 13 * GAP + 64)]
    for kw in invalid + overlapping:
        assert _select(lib, **kw) == tcapi.E_INVALID, kw
        assert tcapi.last_error(), kw
    assert "overlap" in tcapi.last_error()
    # arrays that touch do not overlap: the alignment of the next check is what fails then
    assert _select(lib, theta_target=FAKE + 6 * GAP + stack, header=FAKE + 2 * GAP + 4) == tcapi.E_ALIGN
    misaligned = [dict(hyper=FAKE + 13 * GAP + 4), dict(t=FAKE + 10 * GAP + 4), dict(header=FAKE + 2 * GAP + 4), dict(mark=FAKE + 3 * GAP + 4),
                  dict(seg_counts=FAKE + GAP + 4), dict(eps_state=FAKE + 14 * GAP + 4), dict(score=FAKE + 2), dict(origin=FAKE + 4 * GAP + 1),
                  dict(parent=FAKE + 5 * GAP + 2), dict(eps_out=FAKE + 15 * GAP + 2), dict(theta=FAKE + 6 * GAP + 2), dict(theta_target=FAKE + 7 * GAP + 1),
                  dict(m=FAKE + 8 * GAP + 3), dict(v=FAKE + 9 * GAP + 2), dict(blob_online=FAKE + 11 * GAP + 4), dict(blob_target=FAKE + 12 * GAP + 8)]
    for kw in misaligned:
        assert _select(lib, **kw) == tcapi.E_ALIGN, kw
        assert tcapi.last_error(), kw
    with pytest.raises(ValueError, match="^aquapbt_select: fraction="):
        tcapi.check(_select(lib, fraction=0.75), "aquapbt_select")
    with pytest.raises(tcapi.AquaSelectionError):
        tcapi.check(_select(lib, header=FAKE + 2 * GAP + 4), "aquapbt_select")


# ------------------------------------------------------------------------------------------------ the model's own invariants
def _model(P, **kw):
    return T.fill(T.Model(P, 8, **kw))


def test_model_winners_and_losers_are_disjoint_and_parents_are_winners():
    rng = np.random.RandomState(11)
    replaced = 0
    for P in (1, 2, 3, 5, 8, 64, 65, 257):
        for fraction in (0.2, 0.25, 0.5):
            model = _model(P, fraction=fraction, ready=3, seed=P)
            episodes = np.zeros(P, dtype=np.uint64)
            for call in range(6):
                episodes += rng.randint(0, 4, P).astype(np.uint64)
                score = rng.choice([-1.5, -0.0, 0.0, 0.25, 0.25, 2.0], P).astype(np.float32)
                before = {name: getattr(model, name).copy() for name in T.STACKED + ("hyper", "origin", "mark", "eps_state", "eps_out")}
                model.select(score, episodes)
                S = int((episodes >= 1).sum())
                k = int(fraction * S)
                assert int(model.header[3]) == S and len(model.winners) == k and int(model.header[2]) == len(model.losers) <= k
                assert not set(model.winners) & set(model.losers)
                for p in range(P):
                    q = int(model.parent[p])
                    assert (q != p) == (p in model.losers)
                    if q != p:
                        assert q in model.winners and episodes[p] - before["mark"][p] >= 3 and model.mark[p] == episodes[p]
                        assert model.origin[p] == before["origin"][q]
                        for name in T.STACKED + ("eps_state", "eps_out"):
                            assert np.array_equal(getattr(model, name)[p], before[name][q]), name
                        assert np.array_equal(np.delete(model.hyper[p], [0, 2]), np.delete(before["hyper"][q], [0, 2]))
                        assert 1e-5 <= model.hyper[p, 2] <= 0.1 and 0.5 <= model.hyper[p, 0] <= 0.999
                    else:
                        for name in before:
                            assert np.array_equal(getattr(model, name)[p], before[name][p]), name
                replaced += len(model.losers)
            assert int(model.header[0]) == 6
    assert replaced > 50


def test_model_with_k_zero_writes_only_the_header_and_parent():
    for P, fraction, episodes in ((1, 0.5, [5]), (3, 0.25, [5, 5, 5]), (8, 0.5, [0] * 8), (8, 0.5, [0, 0, 0, 9, 0, 0, 0, 0])):
        model = _model(P, fraction=fraction, ready=1)
        model.header[1] = 17
        model.parent[:] = -1
        before = {name: getattr(model, name).copy() for name in T.STACKED + ("hyper", "origin", "mark", "eps_state", "eps_out")}
        model.select(np.linspace(-1, 1, P).astype(np.float32), np.array(episodes, dtype=np.uint64))
        assert model.header.tolist() == [1, 17, 0, sum(1 for e in episodes if e >= 1)]
        assert model.parent.tolist() == list(range(P))
        for name, want in before.items():
            assert np.array_equal(getattr(model, name), want), name


def test_model_ties_fall_to_the_lower_index_and_every_bit_pattern_has_a_place():
    score = np.array([1.0, 2.0, 1.0, 2.0, -0.0, 0.0, -3.0, 1.0], dtype=np.float32)
    assert T.ranking(score, np.ones(8)) == [1, 3, 0, 2, 7, 5, 4, 6]
    assert T.ranking(score, np.array([1, 0, 1, 1, 1, 0, 1, 1])) == [3, 0, 2, 7, 4, 6]
    assert T.ranking(np.zeros(5, dtype=np.float32), np.ones(5)) == [0, 1, 2, 3, 4]
    bits = np.array([0x7FC00000, 0x7F800000, 0x3F800000, 0x00000001, 0x00000000, 0x80000000, 0x80000001, 0xFF800000, 0xFFC00000], dtype=np.uint32)
    assert T.ranking(bits.view(np.float32), np.ones(9)) == list(range(9))
    k = T.keys(bits.view(np.float32))
    assert len(set(k.tolist())) == 9 and all(0 <= int(x) < 2 ** 32 for x in k)
    # all scores equal, fraction 0.5: the first half wins, the second half loses
    model = _model(6, fraction=0.5, ready=1)
    model.select(np.full(6, 0.5, dtype=np.float32), np.full(6, 2, dtype=np.uint64))
    assert model.winners == [0, 1, 2] and model.losers == [3, 4, 5]
    # every = 3: calls 1 and 2 write only header[0], header[2] and parent
    model = _model(6, fraction=0.5, ready=1, every=3)
    counts = np.full(6, 2, dtype=np.uint64)
    model.select(np.arange(6, dtype=np.float32), counts)
    assert int(model.header[2]) == 3
    hyper, mark = model.hyper.copy(), model.mark.copy()
    for call in (1, 2):
        model.select(np.arange(6, dtype=np.float32), counts + np.uint64(10))
        assert model.header.tolist() == [call + 1, 3, 0, 6] and model.parent.tolist() == list(range(6))
        assert np.array_equal(model.hyper, hyper) and np.array_equal(model.mark, mark)
    model.select(np.arange(6, dtype=np.float32), counts + np.uint64(10))
    assert model.header.tolist() == [4, 6, 3, 6]


def test_codegen_two_kernels_without_scratch_spills_or_float_atomics():
    isa = _isa.kernels("pbt")
    assert len(isa) == 2 and sorted(n.split("pbt_")[1][:4] for n in isa) == ["copy", "plan"], sorted(isa)
    for name, k in isa.items():
        m = k["meta"]
        print("registers:", name, m)
        assert m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert "scratch_" not in k["body"], name
        assert not re.search(r"atomic_\w*(f32|f64)|atomic_(fadd|fmin|fmax|pk_add)", k["body"]), name      # no float atomics
        assert not re.search(r"\b(global|flat|buffer)_atomic", k["body"]), name                            # none on memory at all
        if "plan" in name:
            assert 32768 <= m["group_segment_fixed_size"] <= 65536, m                                     # the 4096 words, and parent
            assert m["vgpr_count"] <= 128, m                                                               # 1024 threads fit a CU
            assert not re.search(r"\bv_fma_f64\b|\bv_fmac_f64\b", k["body"]), name                         # contraction is off
        else:
            assert m["group_segment_fixed_size"] == 0, m
            assert re.search(r"global_load_dwordx4", k["body"]) and re.search(r"global_store_dwordx4", k["body"]), name
    src = open(os.path.join(ROOT, "aquaticgymenv_amd", "csrc", "aqua_pbt.hip")).read()
    assert "asm" not in re.sub(r"//[^\n]*", "", src) and "__threadfence" not in src and "fp contract(off)" in src


def test_no_cpu_path_for_the_selector(tcapi):
    from aquaticgymenv_amd.pbt import PopulationSelector
    with pytest.raises(ValueError):
        PopulationSelector(object(), object())
    src = open(os.path.join(ROOT, "aquaticgymenv_amd", "pbt.py")).read()
    path = src.split("def _launch")[1].split("def report")[0]
    assert ".cpu()" not in path and "argsort" not in src and "index_copy" not in src     # the path reads nothing back
    assert ".cpu()" in src.split("def report")[1] and "sync_hyper()" in src.split("def report")[1].split("def load_state_dict")[0]
    lbank = open(os.path.join(ROOT, "aquaticgymenv_amd", "lbank.py")).read()
    assert "def sync_hyper" in lbank and "sync_hyper" in src.split("def select")[1].split("def _warm_up")[0]
