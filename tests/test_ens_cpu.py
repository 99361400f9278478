"""CPU-only checks of libaqua_ens.so (aquaticgymenv_amd/csrc/aqua_ens.h), the ensemble policy of a Q-network bank: it builds
and loads, exports what its header declares, has a build-table entry of its own behind the pinned ones, draws on the policy's
stream, rejects bad arguments before touching a device and names the field; aquaens_shape states the launch; the numpy model
the GPU tests compare against (tests/_ens_model.py) is itself checked on constructions where a float32 accumulator, another
summation order or another tie rule gives another answer; and the compiler's resource metadata of the kernel shows no
scratch and two wavefronts per SIMD."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import _ens_model as M
from tests import _isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aquaticgymenv_amd", "csrc")
HEADER = os.path.join(CSRC, "aqua_ens.h")
FAKE = 0x10000            # a "device pointer" for calls that must fail (or return) before anything dereferences it


@pytest.fixture(scope="module")
def capi():
    from aquaticgymenv_amd.build import build_library
    assert os.path.exists(build_library("ens"))
    from aquaticgymenv_amd import _ens_capi
    return _ens_capi


# ------------------------------------------------------------------------------------------------ the library and its table
def test_library_builds_loads_and_exports_its_header(capi):
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(aquaens_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(capi.SYMBOLS) == {"aquaens_version", "aquaens_last_error", "aquaens_weights_bytes", "aquaens_shape",
                                            "aquaens_act_f32"}, declared ^ set(capi.SYMBOLS)
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    assert capi.lib.aquaens_version() == capi.ABI_VERSION == 1
    assert set(capi._SIGNATURES) == set(capi.SYMBOLS) - {"aquaens_version", "aquaens_last_error"}

    def define(name):
        return int(re.search(r"#define\s+%s\s+\(?(-?\d+)" % name, text).group(1))
    assert define("AQUAENS_ABI_VERSION") == 1
    assert [define("AQUAENS_E_" + n) for n in ("INVALID", "ALIGN", "NODEVICE")] == [-1, -2, -3] == [capi.E_INVALID, capi.E_ALIGN, capi.E_NODEVICE]
    from aquaticgymenv_amd import _bank_capi
    assert define("AQUAENS_MAX_NETWORKS") == capi.MAX_NETWORKS == _bank_capi.MAX_NETWORKS == 65536
    assert [define("AQUAENS_MEAN"), define("AQUAENS_VOTE")] == [capi.MEAN, capi.VOTE] == [M.MEAN, M.VOTE] == [0, 1]
    assert capi.MODES == {"mean": 0, "vote": 1}
    assert define("AQUAENS_GROUP") == capi.GROUP >= 1 and define("AQUAENS_ACTIONS") == capi.ACTIONS == 3
    assert '"AQUA_ENS_LIB"' in open(os.path.join(ROOT, "aquaticgymenv_amd", "_ens_capi.py")).read()
    if shutil.which("nm"):
        nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True)
        assert nm.returncode == 0 and set(re.findall(r"\b(aquaens_\w+)", nm.stdout)) == declared


def test_the_stream_is_the_policys_and_the_blob_is_the_policys(capi):
    text = open(HEADER).read()
    from aquaticgymenv_amd import _bank_capi, _policy_capi
    assert int(re.search(r"#define\s+AQUAENS_STREAM\s+(\d+)", text).group(1)) == capi.STREAM == _policy_capi.STREAM == _bank_capi.STREAM == 5
    assert capi.lib.aquaens_weights_bytes() == _policy_capi.lib.aquapol_weights_bytes() == _bank_capi.lib.aquabank_weights_bytes()
    # the forward pass, the blob's layout and the compute-unit query are not restated: they come from aqua_qnet.hpp
    src = open(os.path.join(CSRC, "aqua_ens.hip")).read()
    assert "forward<RAW>(" in src and "load_operands(" in src and "pick_and_store<EPS>(" in src and "compute_units(" in src
    assert "__builtin_amdgcn_mfma" not in src and "hipDeviceGetAttribute" not in src and "OFF_W2 =" not in src


def test_the_other_bindings_do_not_know_the_new_symbols(capi):
    from aquaticgymenv_amd import (_bank_capi, _capi, _episodes_capi, _fastpol_capi, _her_capi, _lbank_capi, _learner_capi, _nstep_capi,
                                   _pbt_capi, _policy_capi, _prio_capi, _qmap_capi, _render_capi, _replay_capi, _segments_capi)
    others = (_capi, _policy_capi, _learner_capi, _episodes_capi, _render_capi, _replay_capi, _bank_capi, _lbank_capi, _segments_capi,
              _pbt_capi, _qmap_capi, _fastpol_capi, _nstep_capi, _prio_capi, _her_capi)
    for other in others:
        assert not any(s.startswith("aquaens_") for s in other.SYMBOLS)
        for name in capi.SYMBOLS:
            assert not hasattr(other.lib, name)


def test_build_table_entry_behind_the_pinned_tables():
    from aquaticgymenv_amd import build
    assert list(build.ENSEMBLE_LIBRARIES) == ["ens"]
    assert build.fifteen_libraries() == ["hip", "policy", "learner", "episodes", "render", "replay", "bank", "lbank", "segments", "pbt", "qmap",
                                         "fastpol", "nstep", "prio", "her"]
    assert build.sixteen_libraries() == build.fifteen_libraries() + ["ens"] and len(build.sixteen_libraries()) == 16
    entry = build.library("ens")
    assert entry is build.ENSEMBLE_LIBRARIES["ens"] and build.library("her") is build.HINDSIGHT_LIBRARIES["her"]
    src = os.path.join(CSRC, "aqua_ens.hip")
    lib = os.path.join(ROOT, "aquaticgymenv_amd", "lib", "libaqua_ens.so")
    headers = ["aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp"]
    assert entry["src"] == [src] and entry["lib"] == lib and entry["cuid"] == "aqua_ens"
    assert re.findall(r'#include "([a-z_]+\.hpp)"', open(src).read()) == headers and '#include "aqua_ens.h"' in open(src).read()
    assert entry["deps"] == [src] + [os.path.join(CSRC, h) for h in headers] + [HEADER] and all(os.path.exists(p) for p in entry["deps"])
    assert build.build_command("ens") == [
        build.hipcc_path(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-fno-honor-nans", "-cuid=aqua_ens",
        "-Wall", "-Wno-unused-function", "-o", lib + ".tmp", src]
    assert (build.ENS_SRC, build.ENS_DEPS, build.ENS_LIB, build.ENS_FLAGS) == (entry["src"], entry["deps"], entry["lib"], entry["flags"])
    assert callable(build.build_ens) and build.ens_needs_build() in (True, False)
    assert len({build.library(n)["lib"] for n in build.sixteen_libraries()}) == 16
    main = open(os.path.join(ROOT, "aquaticgymenv_amd", "build.py")).read().split('if __name__ == "__main__":')[1]
    assert "+ list(HINDSIGHT_LIBRARIES) + list(ENSEMBLE_LIBRARIES)" in main
    for name in build.fifteen_libraries():
        assert not any("aqua_ens" in os.path.basename(d) for d in build.library(name)["deps"]), name
    # the header lies beside the source: neither include/ directory has a new file
    for folder in (os.path.join(ROOT, "include"), os.path.join(ROOT, "aquaticgymenv_amd", "include")):
        assert not any("ens" in name for name in os.listdir(folder))


def test_graft_entry_builds_and_checks_the_new_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    build_body = text.split("def build():")[1].split("def smoke():")[0]
    assert "sixteen_libraries()[15:]" in build_body and "_ens_capi" in build_body and "aquaens_version" in build_body
    assert "fifteen_libraries()[14:]" in build_body
    import __graft_entry__ as entry
    from aquaticgymenv_amd import build
    assert entry.build() is None and os.path.exists(build.ENS_LIB)


# ------------------------------------------------------------------------------------------------ the C API without a device
ORDER = ("bank", "networks", "member", "mode", "inp", "ld", "norm", "N", "env_offset", "epsilon", "epsilon_dev", "seed", "tick", "tick_base",
         "action", "q", "q_ld", "q_taken", "variance", "votes", "x_ld")


def _act(lib, **kw):
    a = dict(bank=FAKE, networks=4, member=FAKE + 0x100, mode=0, inp=FAKE + 0x1000, ld=1000, norm=1, N=1000, env_offset=0, epsilon=0.0,
             epsilon_dev=None, seed=17, tick=3, tick_base=None, action=FAKE + 0x3000, q=FAKE + 0x4000, q_ld=1000, q_taken=FAKE + 0x8000,
             variance=FAKE + 0xA000, votes=FAKE + 0xE000, x_ld=1000)
    a.update(kw)
    return lib.aquaens_act_f32(*[a[name] for name in ORDER], None)


def test_argument_validation_without_touching_a_device(capi):
    """every call here fails (or returns) before the first HIP call: nothing is launched, no pointer is dereferenced; the
    message names the offending field"""
    lib = capi.lib
    nan = float("nan")
    invalid = [("bank", dict(bank=None)), ("in", dict(inp=None)),
               ("networks", dict(networks=0)), ("networks", dict(networks=-1)), ("networks", dict(networks=65537)),
               ("networks", dict(networks=2 ** 63 - 1)),
               ("mode", dict(mode=2)), ("mode", dict(mode=-1)),
               ("ld", dict(ld=999)), ("ld", dict(ld=-(2 ** 63))), ("N", dict(N=-1)), ("N", dict(N=2 ** 63 - 1)),
               ("q_ld", dict(q_ld=999)), ("q_ld", dict(q_ld=-(2 ** 63))), ("x_ld", dict(x_ld=999)), ("x_ld", dict(x_ld=999, votes=None)),
               ("x_ld", dict(x_ld=0, variance=None)), ("env_offset", dict(env_offset=-1)),
               ("epsilon", dict(epsilon=nan)), ("epsilon", dict(epsilon=-0.25)), ("epsilon", dict(epsilon=-float("inf"))),
               ("action", dict(action=None, q=None, q_taken=None, variance=None, votes=None))]
    for field, kw in invalid:
        assert _act(lib, **kw) == capi.E_INVALID, kw
        assert re.search(r"\b%s\b" % field, capi.last_error()), (kw, capi.last_error())
    misaligned = [("bank", dict(bank=FAKE + 8)), ("bank", dict(bank=FAKE + 4)), ("in", dict(inp=FAKE + 0x1002)), ("q", dict(q=FAKE + 0x4001)),
                  ("q_taken", dict(q_taken=FAKE + 0x8002)), ("variance", dict(variance=FAKE + 0xA002)), ("votes", dict(votes=FAKE + 0xE001)),
                  ("epsilon_dev", dict(epsilon_dev=FAKE + 0x202)), ("tick_base_dev", dict(tick_base=FAKE + 0x304))]
    for field, kw in misaligned:
        assert _act(lib, **kw) == capi.E_ALIGN, kw
        assert re.search(r"\b%s\b" % field, capi.last_error()), (kw, capi.last_error())
    # the limits themselves pass the size checks (and then meet an alignment check): every output alone, x_ld unused
    # without variance and votes, q_ld unused without q, -0.0 is zero, no mask
    ok_sizes = [dict(networks=1), dict(networks=65536), dict(mode=1), dict(member=None), dict(epsilon=-0.0), dict(epsilon=1.5),
                dict(x_ld=0, variance=None, votes=None), dict(q_ld=0, q=None), dict(N=1, ld=1, q_ld=1, x_ld=1),
                dict(action=None, q=None, q_taken=None, votes=None), dict(action=None, q=None, q_taken=None, variance=None),
                dict(q=None, q_taken=None, variance=None, votes=None, x_ld=-5), dict(env_offset=2 ** 62)]
    for kw in ok_sizes:
        assert _act(lib, tick_base=FAKE + 0x304, **kw) == capi.E_ALIGN, kw
    # nothing to do: no launch, no device, no input needed
    assert _act(lib, N=0) == 0 and _act(lib, N=0, inp=None, ld=0, q_ld=0, x_ld=0) == 0
    # the Python layer turns E_INVALID into ValueError and everything else into the binding's error
    with pytest.raises(ValueError, match="^aquaens_act_f32: mode=2"):
        capi.check(_act(lib, mode=2), "aquaens_act_f32")
    with pytest.raises(capi.AquaEnsError):
        capi.check(_act(lib, bank=FAKE + 8), "aquaens_act_f32")


def test_no_cpu_path_and_argument_errors_of_the_class(capi):
    import types
    import torch
    from aquaticgymenv_amd.ensemble import QEnsemble
    for bad in (object(), None, 3, [1, 2]):
        with pytest.raises(ValueError, match="QNetworkBank"):
            QEnsemble(bad)
    if not torch.cuda.is_available():
        from aquaticgymenv_amd.qbank import QNetworkBank
        from tests._qbank import family
        with pytest.raises(RuntimeError, match="no CPU path"):
            QNetworkBank([family(0)], 1, "cuda:0")
    fake = types.SimpleNamespace(_aquapol_network=True, networks=2, seg=1, view=None, torch=torch, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="mode"):
        QEnsemble(fake, mode="median")
    assert not hasattr(QEnsemble, "seg") and not hasattr(QEnsemble, "state_dict")


# ------------------------------------------------------------------------------------------------ the launch shape
def test_shape_states_the_launch(capi):
    world = 32 * capi.GROUP
    assert capi.shape(0, 256) == (0, 0, 0)
    assert capi.shape(1, 256) == (1, 1, 1) and capi.shape(world, 256) == (1, 1, 1) and capi.shape(world + 1, 256) == (1, 2, 1)
    assert capi.shape(4 * world + 1, 256) == (2, 5, 1)
    cap = 2 * 256                                              # blocks: two wavefronts per SIMD, four SIMDs, four wavefronts a block
    assert capi.shape(4 * cap * world, 256) == (cap, 4 * cap, 1)
    big = 4 * cap * world + 77                                  # the size the GPU test takes on a device of 256 compute units
    assert capi.shape(big, 256) == (cap, 4 * cap + 1, 2)
    for cus in (1, 2, 64, 256, 304):
        for n in (1, 31, 1000, 16384, 262144, 10 ** 7, 2 ** 40, 2 ** 62):
            blocks, groups, most = capi.shape(n, cus)
            assert 1 <= blocks <= 2 * cus and groups == -(-n // world) and most == -(-groups // (4 * blocks))
            assert blocks == min(-(-groups // 4), 2 * cus)
    out = (ctypes.c_int64 * 3)(7, 7, 7)
    for n, cus, ptr, field in ((-1, 256, ctypes.addressof(out), "N"), (5, 0, ctypes.addressof(out), "cus"), (5, -3, ctypes.addressof(out), "cus"),
                               (5, 256, None, "out")):
        assert capi.lib.aquaens_shape(n, cus, ptr) == capi.E_INVALID and re.search(r"\b%s\b" % field, capi.last_error())
    assert list(out) == [7, 7, 7]
    with pytest.raises(ValueError, match="N=-2"):
        capi.shape(-2, 256)


# ------------------------------------------------------------------------------------------------ the model
def _constant_members(values):
    """members whose Q is the same constant for all three actions and one world: float32 [M][3][1]"""
    return np.array([[[v]] * 3 for v in values], dtype=np.float32)


def test_the_model_sums_in_double():
    """[2^30, 1, -2^30]: the double sum is 1 and the mean float32(1/3); a float32 accumulator loses the 1 and gives 0"""
    q = _constant_members([2.0 ** 30, 1.0, -2.0 ** 30])
    out = M.ensemble(q)
    assert (M.bits(out["qbar"]) == M.bits(np.float32(1.0 / 3.0))).all()
    acc = np.float32(0)
    for v in q[:, 0, 0]:
        acc = np.float32(acc + v)
    assert acc == 0
    # the variance is the population's, from the same sums: S2 = 2^61 + 1 rounds to 2^61
    want = np.float32(max(2.0 ** 61 / 3.0 - (1.0 / 3.0) * (1.0 / 3.0), 0.0))
    assert (M.bits(out["variance"]) == M.bits(want)).all()


def test_the_model_sums_in_ascending_order_one_add_per_member():
    """[2^60, 1, -2^60, 1] sums to 1 front to back; back to front and pairwise both give 0"""
    values = [2.0 ** 60, 1.0, -2.0 ** 60, 1.0]
    out = M.ensemble(_constant_members(values))
    assert (M.bits(out["qbar"]) == M.bits(np.float32(0.25))).all()
    s1, _ = M.sums(_constant_members(values))
    assert (s1 == 1.0).all()
    rev = np.float64(0)
    for v in reversed(values):
        rev = rev + np.float64(v)
    pair = (np.float64(values[0]) + np.float64(values[1])) + (np.float64(values[2]) + np.float64(values[3]))
    assert rev == 0 and pair == 0


def test_the_model_breaks_vote_ties_by_qbar_then_index():
    def world(rows):
        return np.array(rows, dtype=np.float32)[:, :, None]
    # 1-1: member 0 says action 2, member 1 says action 0; Qbar = (2.5, 0, 2): action 0 has the larger mean
    out = M.ensemble(world([[1, 0, 4], [4, 0, 0]]))
    assert out["votes"][:, 0].tolist() == [1, 0, 1] and out["qbar"][:, 0].tolist() == [2.5, 0, 2] and out["action_vote"][0] == 0
    # 1-1 the other way round: Qbar = (2, 0, 2.5) -> action 2, although 0 is the lower index
    out = M.ensemble(world([[0, 0, 4], [4, 0, 1]]))
    assert out["votes"][:, 0].tolist() == [1, 0, 1] and out["action_vote"][0] == 2 and out["action_mean"][0] == 2
    # 2-2 between actions 1 and 2 with Qbar equal as well: the lowest index
    out = M.ensemble(world([[0, 2, 0], [0, 2, 0], [0, 0, 2], [0, 0, 2]]))
    assert out["votes"][:, 0].tolist() == [0, 2, 2] and out["qbar"][:, 0].tolist() == [0, 1, 1] and out["action_vote"][0] == 1
    # the vote and the mean disagree: two members prefer action 1 by a hair, one prefers action 0 by a lot
    out = M.ensemble(world([[0, 1, 0], [0, 1, 0], [16, 0, 0]]))
    assert out["action_vote"][0] == 1 and out["action_mean"][0] == 0 and out["taken_vote"][0] == np.float32(2.0 / 3.0)
    # equal everywhere: action 0 in both modes, and every member votes 0
    out = M.ensemble(world([[3, 3, 3], [3, 3, 3]]))
    assert out["action_vote"][0] == 0 and out["action_mean"][0] == 0 and out["votes"][:, 0].tolist() == [2, 0, 0]


def test_the_model_with_one_member_and_with_none():
    rng = np.random.RandomState(5)
    q = rng.randn(1, 3, 50).astype(np.float32)
    q[0, :, 7] = q[0, 1, 7]                                    # a tie: the lowest index
    out = M.ensemble(q)
    assert np.array_equal(M.bits(out["qbar"]), M.bits(q[0])) and not out["variance"].any()
    best = np.argmax(q[0], axis=0)
    assert np.array_equal(out["action_mean"], best) and np.array_equal(out["action_vote"], best) and best[7] == 0
    assert np.array_equal(out["votes"], (np.arange(3)[:, None] == best[None, :]).astype(np.int32))
    assert np.array_equal(M.bits(out["taken_mean"]), M.bits(q[0][best, np.arange(50)]))
    none = M.ensemble(np.zeros((0, 3, 9), np.float32))
    for key in ("qbar", "variance", "votes", "action_mean", "action_vote", "taken_mean", "taken_vote"):
        assert not none[key].any(), key
    # many members: the sequential loop equals Python's own float arithmetic, member by member
    q = rng.randn(17, 3, 4).astype(np.float32)
    out = M.ensemble(q)
    for c in range(3):
        for i in range(4):
            s1 = s2 = 0.0
            for p in range(17):
                s1 += float(q[p, c, i])
                s2 += float(q[p, c, i]) * float(q[p, c, i])
            assert out["qbar"][c, i] == np.float32(s1 / 17) and out["variance"][c, i] == np.float32(max(s2 / 17 - (s1 / 17) * (s1 / 17), 0.0))


# ------------------------------------------------------------------------------------------------ the compiler's metadata
def test_codegen_has_no_scratch_and_two_wavefronts_per_simd():
    """the resource metadata of the code object's notes: one instance of the kernel per input form and exploration, none with
    a private segment or a spilled vector register, every one within the 256 registers of two wavefronts per SIMD, GROUP tiles
    of the 70 MFMAs of aqua_qnet.hpp's forward pass each.  The register counts are printed for the record"""
    from aquaticgymenv_amd import _ens_capi
    isa = _isa.kernels("ens")
    assert len(isa) == 4 and all("qens_kernel" in name for name in isa), sorted(isa)
    for name, k in isa.items():
        m = k["meta"]
        print("registers:", name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] + m["agpr_count"] <= 256, (name, m)
        assert k["stats"]["ScratchSize"] == 0 and k["stats"]["Occupancy"] >= 2, (name, k["stats"])
        assert m["group_segment_fixed_size"] == 4 * 4 * 324, (name, m)           # the LDS part, once per wavefront of the block
        assert len(re.findall(r"\bv_mfma_f32_32x32x2_f32\b", k["body"])) == 70 * _ens_capi.GROUP, name
        assert "scratch_" not in k["body"]
