"""CPU-only checks of libaqua_qmap.so (aquaticgymenv_amd/csrc/aqua_qmap.h), the Q-value maps of every network of a bank: it
builds and loads, exports what its header declares, has a build-table entry of its own behind the pinned tables, uses the
one statement of the acting network (csrc/aqua_qnet.hpp) and no matrix instruction of its own, rejects bad arguments before
touching a device, counts its items as the header says, its tables reproduce the reference plotter's states bit for bit
(and the transposed assignment does not), and its kernel has no scratch or spill within three wavefronts per SIMD."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import _isa
from tests import _qmaps as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aquaticgymenv_amd", "csrc")
HEADER = os.path.join(CSRC, "aqua_qmap.h")
FAKE = 0x10000            # a "device pointer" for calls that must fail before anything dereferences it


@pytest.fixture(scope="module")
def mcapi():
    from aquaticgymenv_amd.build import build_library
    assert os.path.exists(build_library("qmap"))
    from aquaticgymenv_amd import _qmap_capi
    return _qmap_capi


def test_library_builds_loads_and_exports_its_header(mcapi):
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(aquaqmap_[a-z0-9_]+)\s*\(", text))
    assert declared == set(mcapi.SYMBOLS) == {"aquaqmap_version", "aquaqmap_last_error", "aquaqmap_weights_bytes", "aquaqmap_items",
                                              "aquaqmap_maps_f32"}, declared ^ set(mcapi.SYMBOLS)
    raw = ctypes.CDLL(mcapi.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    assert mcapi.lib.aquaqmap_version() == mcapi.ABI_VERSION == 1
    assert set(mcapi._SIGNATURES) == set(mcapi.SYMBOLS) - {"aquaqmap_version", "aquaqmap_last_error"}

    def define(name):
        return int(re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, text).group(1))
    assert define("AQUAQMAP_ABI_VERSION") == 1
    assert [define("AQUAQMAP_E_" + n) for n in ("INVALID", "ALIGN", "NODEVICE")] == [-1, -2, -3]
    assert [mcapi.E_INVALID, mcapi.E_ALIGN, mcapi.E_NODEVICE] == [-1, -2, -3]
    from aquaticgymenv_amd import _bank_capi, _policy_capi
    assert define("AQUAQMAP_MAX_NETWORKS") == mcapi.MAX_NETWORKS == _bank_capi.MAX_NETWORKS
    assert define("AQUAQMAP_ACTIONS") == mcapi.ACTIONS == _bank_capi.SHAPES[-1]
    assert (define("AQUAQMAP_MAX_GOALS"), define("AQUAQMAP_MAX_SIDE"), define("AQUAQMAP_MAX_SECTORS")) == \
        (mcapi.MAX_GOALS, mcapi.MAX_SIDE, mcapi.MAX_SECTORS)
    assert define("AQUAQMAP_MAX_STATES") == mcapi.MAX_STATES == 2 ** 30 and define("AQUAQMAP_MAX_TOTAL") == mcapi.MAX_TOTAL == 2 ** 40
    # q's last offset, 3 * MAX_TOTAL floats, and the item count at the caps stay inside int64; a state's index inside uint32
    assert 4 * 3 * mcapi.MAX_TOTAL < 2 ** 63 and mcapi.MAX_STATES + M.TILE < 2 ** 32
    assert mcapi.lib.aquaqmap_weights_bytes() == _policy_capi.lib.aquapol_weights_bytes() == _bank_capi.lib.aquabank_weights_bytes()
    # the arguments of the declarations and of the binding, one for one
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "size_t": ctypes.c_size_t}
    for name in ("aquaqmap_items", "aquaqmap_maps_f32", "aquaqmap_weights_bytes"):
        ret, decl = re.search(r"^(\w+) %s\((.*?)\);" % name, text, re.S | re.M).groups()
        args = [] if decl.strip() == "void" else [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in (a.strip() for a in decl.split(","))]
        argtypes, restype = mcapi._SIGNATURES[name]
        assert (argtypes or []) == args and restype is kinds[ret], name
    assert len(mcapi._SIGNATURES["aquaqmap_maps_f32"][0]) == 14
    # the exported dynamic symbols with the prefix are exactly the declared ones
    if shutil.which("nm"):
        nm = subprocess.run(["nm", "-D", "--defined-only", mcapi.LIB_PATH], capture_output=True, text=True)
        assert nm.returncode == 0 and set(re.findall(r"\b(aquaqmap_\w+)", nm.stdout)) == declared


def test_the_other_ten_bindings_do_not_know_the_new_symbols(mcapi):
    from aquaticgymenv_amd import (_bank_capi, _capi, _episodes_capi, _lbank_capi, _learner_capi, _pbt_capi, _policy_capi, _render_capi,
                                   _replay_capi, _segments_capi)
    for other in (_capi, _policy_capi, _learner_capi, _episodes_capi, _render_capi, _replay_capi, _bank_capi, _lbank_capi, _segments_capi,
                  _pbt_capi):
        assert not any(s.startswith("aquaqmap_") for s in other.SYMBOLS)
        for name in mcapi.SYMBOLS:
            assert not hasattr(other.lib, name)


def test_build_table_entry_and_the_lists():
    from aquaticgymenv_amd import build
    assert list(build.MAP_LIBRARIES) == ["qmap"]
    assert build.eleven_libraries() == build.ten_libraries() + ["qmap"] and len(build.eleven_libraries()) == 11
    assert "qmap" not in build.ten_libraries()
    entry = build.library("qmap")
    assert entry is build.MAP_LIBRARIES["qmap"] and build.library("pbt") is build.SELECTION_LIBRARIES["pbt"]
    with pytest.raises(KeyError):
        build.library("nothing")
    src = os.path.join(CSRC, "aqua_qmap.hip")
    lib = os.path.join(ROOT, "aquaticgymenv_amd", "lib", "libaqua_qmap.so")
    assert entry["src"] == [src] and entry["lib"] == lib and entry["cuid"] == "aqua_qmap"
    assert entry["deps"] == [src] + [os.path.join(CSRC, h) for h in ("aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp")] + [HEADER]
    assert all(os.path.exists(p) for p in entry["deps"])
    # the command line, token by token: the common one with the library's own compilation-unit id
    assert build.build_command("qmap") == [
        build.hipcc_path(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-fno-honor-nans", "-cuid=aqua_qmap",
        "-Wall", "-Wno-unused-function", "-o", lib + ".tmp", src]
    assert (build.QMAP_SRC, build.QMAP_DEPS, build.QMAP_LIB, build.QMAP_FLAGS) == (entry["src"], entry["deps"], entry["lib"], entry["flags"])
    assert callable(build.build_qmap) and build.qmap_needs_build() in (True, False)
    assert len({build.library(n)["lib"] for n in build.eleven_libraries()}) == 11
    main = open(os.path.join(ROOT, "aquaticgymenv_amd", "build.py")).read().split('if __name__ == "__main__":')[1]
    assert "nine_libraries() + list(SELECTION_LIBRARIES) + list(MAP_LIBRARIES)" in main


def test_graft_entry_builds_and_checks_the_new_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "every_library()" in text and "MAP_LIBRARIES" in text and "_qmap_capi" in text and "aquaqmap_version" in text


def test_the_source_uses_the_one_statement_of_the_network():
    text = open(os.path.join(CSRC, "aqua_qmap.hip")).read()
    assert set(re.findall(r'#include "([a-z_]+\.hpp)"', text)) == {"aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp"}
    assert '#include "aqua_qmap.h"' in text
    assert "forward<false>(" in text and "load_operands(" in text and "pick_and_store" not in text
    assert "v_mfma" not in text and "__builtin_amdgcn_mfma" not in text
    code = re.sub(r"//[^\n]*", "", text)
    assert "asm" not in code and "atomic" not in code.lower().replace("__atomic_release", "").replace("__atomic_acquire", "")
    assert not re.search(r"hipMalloc|hipFree|Synchronize|hipMemcpy|hipMemset", text)
    # what existing tests count across csrc/ is still stated once, elsewhere
    for name in ("aqua_qmap.hip", "aqua_qmap.h"):
        t = open(os.path.join(CSRC, name)).read()
        for once in ("constexpr int OFF_W1", "int compute_units(", "void grad_body(", "void apply_body(", "WS_STRIDE = 4744", "struct GradArgs",
                     "struct ApplyArgs"):
            assert once not in t, (name, once)


ORDER = ("bank", "P", "xs", "W", "ys", "H", "angles", "S", "goals", "G", "action", "value", "q")


def _maps(lib, **kw):
    """a call that must fail before the first HIP call: the pointers are not memory"""
    a = dict(bank=FAKE, P=4, xs=FAKE + 0x1000, W=7, ys=FAKE + 0x2000, H=5, angles=FAKE + 0x3000, S=3, goals=FAKE + 0x4000, G=2,
             action=FAKE + 0x100000, value=FAKE + 0x200000, q=FAKE + 0x300000)
    a.update(kw)
    return lib.aquaqmap_maps_f32(*[a[name] for name in ORDER], None)


def test_argument_validation_without_touching_a_device(mcapi):
    """every call here fails: nothing is launched and the pointers are never dereferenced; the message names the argument"""
    lib = mcapi.lib
    invalid = [(dict(bank=None), "bank"), (dict(xs=None), "xs"), (dict(ys=None), "ys"), (dict(angles=None), "angles"), (dict(goals=None), "goals"),
               (dict(P=0), "P="), (dict(P=-1), "P="), (dict(P=mcapi.MAX_NETWORKS + 1), "P="),
               (dict(W=0), "W="), (dict(W=-7), "W="), (dict(W=mcapi.MAX_SIDE + 1), "W="), (dict(W=2 ** 63 - 1), "W="),
               (dict(H=0), "H="), (dict(H=mcapi.MAX_SIDE + 1), "H="), (dict(H=-2 ** 63), "H="),
               (dict(S=0), "S="), (dict(S=mcapi.MAX_SECTORS + 1), "S="), (dict(G=0), "G="), (dict(G=-1), "G="), (dict(G=mcapi.MAX_GOALS + 1), "G="),
               (dict(W=32768, H=32768, S=2), "S * H * W"), (dict(W=65536, H=65536, S=4096), "S * H * W"),
               (dict(P=65536, G=65536, W=1024, H=1024, S=1), "P * G"), (dict(P=1024, G=1024, W=1024, H=1025, S=1), "P * G"),
               (dict(action=None, value=None, q=None), "all NULL")]
    for kw, names in invalid:
        assert _maps(lib, **kw) == mcapi.E_INVALID, kw
        assert names in mcapi.last_error(), (kw, mcapi.last_error())
    misaligned = [(dict(bank=FAKE + 8), "bank"), (dict(bank=FAKE + 4), "bank"), (dict(xs=FAKE + 0x1002), "xs"), (dict(ys=FAKE + 0x2001), "ys"),
                  (dict(angles=FAKE + 0x3003), "angles"), (dict(goals=FAKE + 0x4002), "goals"), (dict(value=FAKE + 0x200002), "value"),
                  (dict(q=FAKE + 0x300001), "q must")]
    for kw, names in misaligned:
        assert _maps(lib, **kw) == mcapi.E_ALIGN, kw
        assert names in mcapi.last_error(), (kw, mcapi.last_error())
    # sizes exactly at the caps pass the size checks: the call gets as far as the alignment of q
    assert _maps(lib, W=32768, H=32768, S=1, P=1, G=1, q=FAKE + 1) == mcapi.E_ALIGN
    assert _maps(lib, P=1024, G=1024, W=1024, H=1024, S=1, q=FAKE + 1) == mcapi.E_ALIGN
    assert _maps(lib, P=65536, G=65536, W=16, H=16, S=1, q=FAKE + 1) == mcapi.E_ALIGN
    # each output alone is enough, and action has no alignment
    assert _maps(lib, action=FAKE + 1, value=None, q=FAKE + 2) == mcapi.E_ALIGN and "q must" in mcapi.last_error()
    assert _maps(lib, action=None, q=None, value=FAKE + 2) == mcapi.E_ALIGN and _maps(lib, action=None, value=None, q=FAKE + 2) == mcapi.E_ALIGN
    # the Python layer turns E_INVALID into ValueError and everything else into the binding's error
    with pytest.raises(ValueError, match="^aquaqmap_maps_f32: S=0"):
        mcapi.check(_maps(lib, S=0), "aquaqmap_maps_f32")
    with pytest.raises(mcapi.AquaMapError):
        mcapi.check(_maps(lib, bank=FAKE + 8), "aquaqmap_maps_f32")


def test_the_items_of_a_launch(mcapi):
    """aquaqmap_items(P, G, H, W, S) = P * G * ceil(S * H * W / 32), also where the products are near their caps"""
    items = mcapi.lib.aquaqmap_items
    for P, G, H, W, S in ((1, 1, 1, 1, 1), (1, 1, 1, 31, 1), (1, 1, 1, 32, 1), (2, 2, 1, 33, 1), (2, 2, 3, 5, 5), (2, 2, 8, 8, 8), (6, 2, 5, 7, 3),
                          (2048, 2, 2, 2, 1), (3, 2, 100, 100, 8), (256, 1, 100, 100, 8), (16, 16, 100, 100, 8),
                          (1, 1, 32768, 32768, 1), (1, 1, 65536, 4, 4096), (1, 1, 16384, 16, 4096), (65536, 65536, 16, 16, 1),
                          (65536, 65536, 1, 1, 1), (1024, 1024, 1024, 1024, 1), (65536, 1, 4096, 4096, 1), (1, 1024, 65536, 16384, 1)):
        want = sum(1 for _ in range(P * G)) * len(range(0, S * H * W, 32)) if P * G <= 4096 else P * G * -(-(S * H * W) // 32)
        assert items(P, G, H, W, S) == want, (P, G, H, W, S)
    assert items(3, 2, 100, 100, 8) == 15000 and items(2048, 2, 2, 2, 1) == 4096 and items(65536, 65536, 16, 16, 1) == 2 ** 35
    for bad in ((0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0), (65537, 1, 1, 1, 1), (1, 65537, 1, 1, 1),
                (1, 1, 65537, 1, 1), (1, 1, 1, 65537, 1), (1, 1, 1, 1, 4097), (1, 1, 32768, 32768, 2), (1, 1, 32768, 32769, 1),
                (65536, 65536, 16, 17, 1), (1024, 1024, 1024, 1024, 2), (1, 1, 65536, 65536, 4096), (-1, 1, 1, 1, 1), (1, 1, 2 ** 62, 4, 1)):
        assert items(*bad) == mcapi.E_INVALID and mcapi.last_error(), bad
    # ... and the documented split covers every item once, in order, whatever the device
    for n_items, cus in ((1, 256), (5, 256), (4096, 256), (15000, 256), (15000, 304), (12289, 1), (3072 * 7 + 5, 256)):
        runs = M.runs(n_items, cus)
        assert len(runs) == 4 * min(-(-n_items // 4), 3 * cus) and runs[0][0] == 0 and sum(c for _, c in runs) == n_items
        assert all(runs[i][0] + runs[i][1] == runs[i + 1][0] for i in range(len(runs) - 1))
        assert max(c for _, c in runs) - min(c for _, c in runs) <= 1


@pytest.mark.parametrize("world_size,sectors", [(6, 4), (5, 3), (100, 8)])
def test_the_tables_reproduce_the_plotters_states_bit_for_bit(world_size, sectors):
    """dqn_qvalue_plotter.py:12-16 restated literally (float64, then the float32 the model is given), reshaped and flipped as
    :22-23 flip the results, against the states composed from QValueMaps.reference's tables in [S][H][W] order"""
    from aquaticgymenv_amd.qmaps import QValueMaps
    n, S = world_size, sectors
    goal = np.array([0.3 * n, 0.8 * n]) if n != 100 else np.array([20, 80])
    states = M.plotter_states(goal, n, S)
    assert states.dtype == np.float64 and states.shape == (n * n * S, 5)
    want = M.plotter_flips(states.astype(np.float32), n, S)                       # [n][n][S][5]
    xs, ys, angles = QValueMaps.reference_tables(n, S)
    goals = QValueMaps.normalised_goals([goal, goal[::-1]], n)
    assert all(t.dtype == np.float32 for t in (xs, ys, angles, goals)) and (len(xs), len(ys), len(angles)) == (n, n, S)
    got = M.composed(xs, ys, angles, goals[0])                                    # [S][H][W][5]
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.transpose(2, 0, 1, 3).view(np.uint32))
    assert not np.array_equal(M.composed(xs, ys, angles, goals[0], transposed=True), want.transpose(2, 0, 1, 3))
    # the host-side goal normalisation: float64 division, then the cast (:14), for both goals
    assert np.array_equal(goals[0].view(np.uint32), states[0, 3:].astype(np.float32).view(np.uint32))
    assert np.array_equal(goals[1].view(np.uint32), (goal[::-1] / n).astype(np.float32).view(np.uint32))
    assert not np.array_equal(goals[0], goals[1])
    # as_reference() is the permutation from [S][H][W] back to the reference's [H][W][S]
    import torch
    t = torch.arange(2 * S * n * n).reshape(2, S, n, n)
    assert torch.equal(QValueMaps.as_reference(t), t.permute(0, 2, 3, 1)) and QValueMaps.as_reference(t[0]).shape == (n, n, S)


def test_the_model_tells_its_mutations_apart():
    """the int64 model on the shapes of the GPU test: an x/y swap, a goal-coordinate swap, a sector/row mix-up and a wrong
    network per item each change the expected arrays (a self-check of tests/_qmaps.py)"""
    from tests._qbank import family
    nets = [family(p) for p in range(5)] + [M.tie_layers()]
    xs, ys, angles, goals = [3, 0, 2, 1, 1, 3, 0], [1, 2, 0, 3, 2], [2, 3, 1], [(1, 3), (2, 0)]
    want = M.int_maps(nets, xs, ys, angles, goals)
    assert want.shape == (6, 2, 3, 3, 5, 7) and np.abs(want).max() < 2 ** 24
    assert (want[5] == 4).all() and (M.picks(want)[0][5] == 0).all() and len(np.unique(M.picks(want)[0][:5])) == 3
    for mutation in M.MUTATIONS:
        wrong = M.int_maps(nets, xs, ys, angles, goals, mutation)
        assert not np.array_equal(wrong, want), mutation
        assert not np.array_equal(M.picks(wrong)[1], M.picks(want)[1]), mutation


def test_codegen_one_kernel_on_the_f32_mfma_without_scratch():
    isa = _isa.kernels("qmap")
    assert len(isa) == 1 and all("qmap_kernel" in n for n in isa), sorted(isa)
    for name, k in isa.items():
        m = k["meta"]
        print("registers:", name, m)
        assert m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert "scratch_" not in k["body"], name
        assert m["vgpr_count"] + m["agpr_count"] <= 170, (name, m)      # three wavefronts per SIMD (512 registers per lane)
        # 6 (64 x 5, K padded to 6) + 64 (64 x 64) in the tile body, which is there once
        assert len(re.findall(r"\bv_mfma_f32_32x32x2_f32\b", k["body"])) == 70, name
        assert len(re.findall(r"\bv_mfma_\w+", k["body"])) == 70, name                         # no other matrix instruction
        assert not re.search(r"v_cvt_\w*(bf16|f16|fp8|bf8|bf6|fp6|fp4)", k["body"]), name     # no reduced-precision conversion
        assert not re.search(r"\b(global|flat|buffer|ds)_\w*atomic|\bds_(add|sub|inc|dec|min|max|and|or|xor|cmpst)_", k["body"]), name
        assert m["group_segment_fixed_size"] == 4 * 1296, (name, m)     # the LDS part, one copy per wavefront
        assert re.search(r"global_store_byte", k["body"]) and re.search(r"global_store_dword\b", k["body"]), name


def test_no_cpu_path_for_the_maps():
    import torch
    from aquaticgymenv_amd.qmaps import QValueMaps
    with pytest.raises(ValueError, match="policy"):
        QValueMaps(object(), [0.5], [0.5], [0.0])
    from aquaticgymenv_amd.qpolicy import QNetwork
    stub = QNetwork.__new__(QNetwork)
    stub.torch, stub.device = torch, torch.device("cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        QValueMaps(stub, [0.5], [0.5], [0.0])
    src = open(os.path.join(ROOT, "aquaticgymenv_amd", "qmaps.py")).read()
    assert "matmul" not in src and "torch.relu" not in src and " @ " not in src and "addmm" not in src and "argmax" not in src
    assert ".cpu()" not in src and "synchronize" not in src
