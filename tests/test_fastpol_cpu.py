"""CPU-only checks of the fast acting path, libaqua_fastpol.so (aquaticgymenv_amd/csrc/aqua_fastpol.h): the numerics of
the scheme on its numpy model (tests/_fastpol.py) against float64, with two controls that show the check can fail; the
fast blob read back in numpy through aquafast_map and the lane maps; an exact dyadic network; the C API without a device;
the compiler's listing; the build recipe."""
import ctypes
import functools
import hashlib
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import _fastpol as F
from tests import _isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aquaticgymenv_amd", "csrc")
HEADER = os.path.join(CSRC, "aqua_fastpol.h")
FAKE = 0x10000            # a "device pointer" for calls that must fail before anything dereferences it


@pytest.fixture(scope="module")
def fcapi():
    from aquaticgymenv_amd.build import build_library
    assert os.path.exists(build_library("fastpol"))
    from aquaticgymenv_amd import _fastpol_capi
    return _fastpol_capi


@pytest.fixture(scope="module")
def pcapi():
    from aquaticgymenv_amd.build import build_library
    assert os.path.exists(build_library("policy"))
    from aquaticgymenv_amd import _policy_capi
    return _policy_capi


@functools.lru_cache(maxsize=None)
def _case(net, n):
    """(layers, x32, q64, E, E_s, the model's q) of one contract case: computed once, shared, never written"""
    x = F.inputs(n)
    layers = F.network(net, x)
    return (layers, x) + F.reference(layers, x)


# ------------------------------------------------------------------------------------------------ the scheme's numerics
@pytest.mark.parametrize("n", F.SIZES)
@pytest.mark.parametrize("net", F.NETS)
def test_model_contract(net, n):
    """the scheme itself, before any kernel: its model is within 4 E of float64 (E: numpy's float32 evaluation on the same
    batch), and the near-tie share at 8 E_s, from q64 alone, stays inside the cap the kernel's test asserts"""
    _, _, q64, E, E_s, _ = _case(net, n)
    _, share = F.near_tie_share(q64, E_s)
    print("%s/%d: E %.3e  E_s %.3e = %.2f E  near-tie share %.4f %%" % (net, n, E, E_s, E_s / E, 100 * share))
    assert E_s <= 4 * E, "%s/%d: the model's error %.3e > 4 E = %.3e" % (net, n, E_s, 4 * E)
    assert share <= F.GAP_CAP


@pytest.mark.parametrize("net", F.NETS)
def test_controls_fail_the_contract(net):
    """the same model without the 2^11 scaling and with f16 subnormals flushed exceeds 100 E; one f16 pass exceeds 1000 E"""
    layers, x, q64, E, _, _ = _case(net, 4099)
    flushed = float(np.max(np.abs(F.model(layers, x, "flushed").astype(np.float64) - q64)))
    onepass = float(np.max(np.abs(F.model(layers, x, "onepass").astype(np.float64) - q64)))
    print("%s: flushed %.0f E  one pass %.0f E" % (net, flushed / E, onepass / E))
    assert flushed > 100 * E and onepass > 1000 * E


def test_split_is_exact_and_clamped():
    v = np.array([0.0, 1.0, 1.0 / 3.0, -2.7182817, 6.1e-5, 3.0e-5, 1.0e-8, 65504.0, 65519.9, 7.0e4, -1.0e9, 2049.0, 1.0 + 2.0 ** -11,
                  1.0 + 3 * 2.0 ** -12], dtype=np.float32)
    hi, lo = F.split(v)
    c = np.clip(v, -65504, 65504).astype(np.float64)
    assert np.isfinite(hi.astype(np.float64)).all() and np.isfinite(lo.astype(np.float64)).all()
    assert float(np.abs(hi.astype(np.float64)).max()) == 65504.0
    # hi + lo 2^-11 carries at least 21 bits of the clamped value
    back = hi.astype(np.float64) + lo.astype(np.float64) * 2.0 ** -11
    assert np.all(np.abs(back - c) <= np.abs(c) * 2.0 ** -21 + 2.0 ** -36)
    assert hi[-2] == 1.0 and lo[-2] == 1.0                       # the tie goes to the even f16, the rest is the lo part


# ------------------------------------------------------------------------------------------------ the blob
def test_blob_layout_through_the_map_and_the_lane_maps(fcapi, pcapi):
    """aquafast_pack_host of a packed float32 blob, read in numpy: every hidden-layer weight once as hi and once as lo, every
    other parameter once as each half of its float32, padding zero, each at the element the MFMA's lane maps name; and the
    network evaluated from what was read equals the model bit for bit"""
    fmap = fcapi.blob_map()
    assert fmap.dtype == np.int32 and fmap.size == F.FAST_ELEMS == fcapi.lib.aquafast_weights_bytes() // 2
    id_blob = pcapi.pack_weights(F.counting_layers()).view(np.float32)
    numbers = np.where(fmap >= 0, id_blob[np.maximum(fmap, 0) >> 2].astype(np.int64), 0)
    want = F.expected_ids()
    assert np.array_equal(numbers[:F.F_LDS], want[:F.F_LDS])
    # the LDS part: the float32 blob's, float by float, low half first
    lds = fmap[F.F_LDS:].reshape(-1, 2)
    named = lds[:, 0] >= 0
    assert np.array_equal(lds[named, 0] & 3, np.full(named.sum(), F.PART_BITS0)) and np.array_equal(lds[named, 1], lds[named, 0] + 1)
    assert np.array_equal(lds[named, 0] >> 2, (id_blob.size - 324 + np.arange(324))[named]) and np.array_equal(lds[~named], np.full(((~named).sum(), 2), -1))
    assert int((~named).sum()) == 1                              # the pad behind the three output biases
    layers, x = _case("with_obs", 4099)[:2]
    for net_layers in (layers, F.random_layers(2, x), F.exact_layers()):
        fast = fcapi.pack_host(pcapi.pack_weights(net_layers))
        parts, words, counts = F.read_fast_blob(fast, fmap, id_blob)
        hidden = set(range(1, 321)) | set(range(385, 385 + 4096))
        assert counts == dict([((i, F.PART_HI), 1) for i in hidden] + [((i, F.PART_LO), 1) for i in hidden] +
                              [((i, part), 1) for i in set(range(1, 4740)) - hidden for part in (F.PART_BITS0, F.PART_BITS1)])
        assert bool((np.ascontiguousarray(fast).view(np.uint16)[fmap < 0] == 0).all())
        for (w_hi, w_lo), k in zip(parts, (net_layers[0][0], net_layers[1][0])):
            hi, lo = F.split(k)
            assert np.array_equal(w_hi.view(np.uint16), hi.view(np.uint16)) and np.array_equal(w_lo.view(np.uint16), lo.view(np.uint16))
        flat = np.concatenate([a.reshape(-1) for kb in net_layers for a in kb]).astype(np.float32)
        rest = np.array(sorted(set(range(1, 4740)) - hidden))
        assert np.array_equal(words[rest].view(np.uint32), flat[rest - 1].view(np.uint32))
        got = F.model(net_layers, x[:257], parts=parts)
        assert np.array_equal(got.view(np.uint32), F.model(net_layers, x[:257]).view(np.uint32))
    # a transposed layer-2 matrix is another blob: the map is not symmetric in (input, output)
    t = [layers[0], (np.ascontiguousarray(layers[1][0].T), layers[1][1]), layers[2]]
    assert not np.array_equal(fcapi.pack_host(pcapi.pack_weights(t)), fcapi.pack_host(pcapi.pack_weights(layers)))


def test_host_split_of_edge_values(fcapi, pcapi):
    """aquafast_pack_host's own float -> f16 conversion against numpy's on values at the clamp, in the f16 subnormal range,
    on rounding ties and below everything"""
    edge = np.array([65504.0, 65519.9, 65520.0, 7.0e4, -3.0e38, 6.1035156e-5, 6.0e-5, 5.9604645e-8, 2.9802322e-8, 2.98e-8, 1.0e-10, 1.0e-38,
                     -0.0, 0.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2049.0, 2051.0, -1.0 / 3.0, 0.1, 1.0e-5, 1.0e-6, np.nan], dtype=np.float32)
    layers = [(k.copy(), b.copy()) for k, b in F.random_layers(1, F.inputs(64))]
    layers[0][0].reshape(-1)[:edge.size] = edge
    layers[1][0].reshape(-1)[7:7 + edge.size] = -edge
    fmap, id_blob = fcapi.blob_map(), pcapi.pack_weights(F.counting_layers()).view(np.float32)
    parts, _, _ = F.read_fast_blob(fcapi.pack_host(pcapi.pack_weights(layers)), fmap, id_blob)
    for (w_hi, w_lo), k in zip(parts, (layers[0][0], layers[1][0])):
        hi, lo = F.split(k)
        assert np.array_equal(w_hi.view(np.uint16), hi.view(np.uint16)) and np.array_equal(w_lo.view(np.uint16), lo.view(np.uint16))
        # nothing but the NaN weight (0x7E00 in both parts, also for the negated one) is not finite
        was_nan = np.isnan(k)
        assert was_nan.sum() == 1 and bool((w_hi.view(np.uint16)[was_nan] == 0x7E00).all()) and bool((w_lo.view(np.uint16)[was_nan] == 0x7E00).all())
        assert np.isfinite(w_hi.astype(np.float64)[~was_nan]).all() and np.isfinite(w_lo.astype(np.float64)[~was_nan]).all()


# ------------------------------------------------------------------------------------------------ the exact network
@pytest.mark.parametrize("variant", ["plain", "tie01", "tie12", "tie012"])
def test_exact_network_model_equals_float64(variant):
    """dyadic weights and inputs with a non-zero lo part at every position of every k-step (asserted, with every partial sum
    within 24 bits and nothing at the clamp, inside exact_reference): the model equals the plain float64 evaluation exactly,
    for the asymmetric layer-2 matrix and not for its transpose"""
    layers = F.exact_layers(variant)
    assert not np.array_equal(layers[1][0], layers[1][0].T)
    x = F.exact_inputs(4099, 4099)
    q64 = F.exact_reference(layers, x)
    q = F.model(layers, x)
    assert q.dtype == np.float32 and np.array_equal(q.astype(np.float64), q64)
    swapped = [layers[0], (np.ascontiguousarray(layers[1][0].T), layers[1][1]), layers[2]]
    assert not np.array_equal(F.model(swapped, x).astype(np.float64), q64)
    want = np.argmax(q64, axis=1)
    top = np.sort(q64, axis=1)
    shared = int((top[:, 2] == top[:, 1]).sum())
    if variant == "plain":
        assert len(np.unique(want)) == 3 and shared == 0
    else:
        assert shared > 100                                       # the maximum itself is shared, the lowest index wins
        assert not bool((want == {"tie01": 1, "tie12": 2, "tie012": 1}[variant]).any())


# ------------------------------------------------------------------------------------------------ the C API without a device
def test_library_builds_loads_and_exports_its_header(fcapi, pcapi):
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(aquafast_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(fcapi.SYMBOLS) == {"aquafast_version", "aquafast_last_error", "aquafast_weights_bytes", "aquafast_map",
                                              "aquafast_pack_host", "aquafast_refresh", "aquafast_act_f16"}, declared ^ set(fcapi.SYMBOLS)
    raw = ctypes.CDLL(fcapi.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    assert fcapi.lib.aquafast_version() == fcapi.ABI_VERSION == 1
    assert set(fcapi._SIGNATURES) == set(fcapi.SYMBOLS) - {"aquafast_version", "aquafast_last_error"}

    def define(name):
        return int(re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, text).group(1))
    assert define("AQUAFAST_ABI_VERSION") == 1
    assert [define("AQUAFAST_E_" + n) for n in ("INVALID", "ALIGN", "NODEVICE")] == [-1, -2, -3] == [fcapi.E_INVALID, fcapi.E_ALIGN, fcapi.E_NODEVICE]
    from aquaticgymenv_amd import _bank_capi
    assert define("AQUAFAST_MAX_NETWORKS") == fcapi.MAX_NETWORKS == _bank_capi.MAX_NETWORKS
    assert (define("AQUAFAST_INPUTS"), define("AQUAFAST_HIDDEN"), define("AQUAFAST_HIDDEN"), define("AQUAFAST_ACTIONS")) == fcapi.SHAPES
    assert define("AQUAFAST_STREAM") == fcapi.STREAM == _bank_capi.STREAM
    assert [define("AQUAFAST_PART_" + n) for n in ("HI", "LO", "BITS0", "BITS1")] == [fcapi.PART_HI, fcapi.PART_LO, fcapi.PART_BITS0, fcapi.PART_BITS1]
    assert fcapi.lib.aquafast_weights_bytes() == 21776 == 2 * F.FAST_ELEMS and fcapi.lib.aquafast_weights_bytes() % 16 == 0
    assert pcapi.lib.aquapol_weights_bytes() == 19216
    # the acting entry takes aquabank_act_f32's arguments, one for one
    assert fcapi._SIGNATURES["aquafast_act_f16"] == _bank_capi._SIGNATURES["aquabank_act_f32"]
    bank_h = open(os.path.join(ROOT, "include", "aqua_bank.h")).read()
    args = lambda t, name: re.sub(r"\s+", " ", re.search(r"^int %s\((.*?)\);" % name, t, re.S | re.M).group(1))     # noqa: E731
    assert args(text, "aquafast_act_f16").replace("fast_dev", "bank_dev") == args(bank_h, "aquabank_act_f32")
    if shutil.which("nm"):
        nm = subprocess.run(["nm", "-D", "--defined-only", fcapi.LIB_PATH], capture_output=True, text=True)
        assert nm.returncode == 0 and set(re.findall(r"\b(aquafast_\w+)", nm.stdout)) == declared


def test_the_other_bindings_do_not_know_the_new_symbols(fcapi):
    from aquaticgymenv_amd import (_bank_capi, _capi, _episodes_capi, _lbank_capi, _learner_capi, _pbt_capi, _policy_capi, _qmap_capi,
                                   _render_capi, _replay_capi, _segments_capi)
    for other in (_capi, _policy_capi, _learner_capi, _episodes_capi, _render_capi, _replay_capi, _bank_capi, _lbank_capi, _segments_capi,
                  _pbt_capi, _qmap_capi):
        assert not any(s.startswith("aquafast_") for s in other.SYMBOLS)
        for name in fcapi.SYMBOLS:
            assert not hasattr(other.lib, name)


def _refresh(lib, **kw):
    a = dict(blobs=FAKE, stride=19216, map=FAKE + 0x100000, fast=FAKE + 0x200000, P=3)
    a.update(kw)
    return lib.aquafast_refresh(a["blobs"], a["stride"], a["map"], a["fast"], a["P"], None)


ACT_ORDER = ("fast", "networks", "seg", "inp", "ld", "normalised", "N", "env_offset", "epsilon", "epsilon_dev", "seed", "tick", "tick_base",
             "action", "q", "q_ld", "q_taken")


def _act(lib, **kw):
    a = dict(fast=FAKE, networks=4, seg=100, inp=FAKE + 0x100000, ld=512, normalised=1, N=400, env_offset=0, epsilon=0.0, epsilon_dev=None,
             seed=1, tick=2, tick_base=None, action=FAKE + 0x200000, q=FAKE + 0x300000, q_ld=512, q_taken=FAKE + 0x400000)
    a.update(kw)
    return lib.aquafast_act_f16(*[a[name] for name in ACT_ORDER], None)


def test_argument_validation_without_touching_a_device(fcapi):
    """every call here fails before the first HIP call: nothing is launched, the pointers are never dereferenced"""
    lib = fcapi.lib
    for kw in (dict(blobs=None), dict(map=None), dict(fast=None), dict(P=0), dict(P=-1), dict(P=fcapi.MAX_NETWORKS + 1), dict(P=2 ** 63 - 1),
               dict(stride=0), dict(stride=-19216), dict(stride=19212), dict(stride=19218), dict(stride=2 ** 62), dict(stride=-2 ** 63)):
        assert _refresh(lib, **kw) == fcapi.E_INVALID and fcapi.last_error(), kw
    for kw in (dict(blobs=FAKE + 8), dict(blobs=FAKE + 4), dict(fast=FAKE + 0x200008), dict(fast=FAKE + 0x200002), dict(map=FAKE + 0x100002),
               dict(map=FAKE + 0x100001)):
        assert _refresh(lib, **kw) == fcapi.E_ALIGN and fcapi.last_error(), kw
    assert _refresh(lib, P=fcapi.MAX_NETWORKS, stride=19216 + 4, map=FAKE + 1) == fcapi.E_ALIGN      # the caps pass the size checks

    nan, inf = float("nan"), float("inf")
    for kw in (dict(fast=None), dict(networks=0), dict(networks=-1), dict(networks=fcapi.MAX_NETWORKS + 1), dict(seg=0), dict(seg=-5),
               dict(N=-1), dict(ld=399), dict(N=401), dict(networks=2 ** 20, seg=2 ** 62, N=5), dict(seg=2 ** 61, networks=3, N=2 ** 63 - 1, ld=2 ** 63 - 1, q_ld=2 ** 63 - 1),
               dict(env_offset=-1), dict(epsilon=-0.5), dict(epsilon=nan), dict(epsilon=-inf), dict(epsilon=nan, epsilon_dev=FAKE),
               dict(action=None, q=None, q_taken=None), dict(q_ld=399), dict(inp=None)):
        assert _act(lib, **kw) == fcapi.E_INVALID and fcapi.last_error(), kw         # (the last size case: networks * seg overflows, N / seg does not)
    for kw in (dict(fast=FAKE + 8), dict(fast=FAKE + 2), dict(inp=FAKE + 0x100002), dict(q=FAKE + 0x300001), dict(q_taken=FAKE + 0x400002),
               dict(epsilon_dev=FAKE + 0x500002), dict(tick_base=FAKE + 0x600004)):
        assert _act(lib, **kw) == fcapi.E_ALIGN and fcapi.last_error(), kw
    # N == 0 returns 0 without a launch; one network with a huge seg and -0.0 pass the checks as far as the alignment
    assert _act(lib, N=0) == 0 and _act(lib, N=0, inp=None) == 0
    assert _act(lib, networks=1, seg=2 ** 62, epsilon=-0.0, q=FAKE + 0x300001) == fcapi.E_ALIGN
    # the host entries
    buf = np.zeros(4 * F.FAST_ELEMS + 8, dtype=np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 8
    assert lib.aquafast_map(None, 4 * F.FAST_ELEMS) == fcapi.E_INVALID and lib.aquafast_map(base, 4 * F.FAST_ELEMS - 1) == fcapi.E_INVALID
    assert lib.aquafast_map(base + 2, 4 * F.FAST_ELEMS) == fcapi.E_ALIGN and lib.aquafast_map(base, 4 * F.FAST_ELEMS) == 0
    src = np.zeros(19216 + 8, dtype=np.uint8)
    sbase = src.ctypes.data + (-src.ctypes.data) % 8
    assert lib.aquafast_pack_host(None, base, 21776) == fcapi.E_INVALID and lib.aquafast_pack_host(sbase, None, 21776) == fcapi.E_INVALID
    assert lib.aquafast_pack_host(sbase, base, 21775) == fcapi.E_INVALID and lib.aquafast_pack_host(sbase + 1, base, 21776) == fcapi.E_ALIGN
    assert lib.aquafast_pack_host(sbase, base + 2, 21776) == fcapi.E_ALIGN and lib.aquafast_pack_host(sbase, base, 21776) == 0
    with pytest.raises(ValueError, match="^aquafast_refresh: P=0"):
        fcapi.check(_refresh(lib, P=0), "aquafast_refresh")
    with pytest.raises(fcapi.AquaFastError):
        fcapi.check(_refresh(lib, blobs=FAKE + 8), "aquafast_refresh")
    with pytest.raises(ValueError):
        fcapi.pack_host(np.zeros(100, dtype=np.uint8))


def test_no_cpu_path_for_the_fast_actor(fcapi):
    from aquaticgymenv_amd.fastpolicy import FastActor
    from aquaticgymenv_amd.qpolicy import QNetwork
    layers = F.fixture_layers("no_obs")
    with pytest.raises(RuntimeError) as fast:
        FastActor(layers, device="cpu")
    with pytest.raises(RuntimeError) as plain:
        QNetwork(layers, device="cpu")
    assert str(fast.value) == str(plain.value) and "no CPU path" in str(fast.value)
    for bad in (object(), None, 3):
        with pytest.raises(ValueError):
            FastActor(bad)
    assert issubclass(FastActor, QNetwork) and FastActor._aquapol_network is True
    import inspect
    assert inspect.signature(FastActor.launch) == inspect.signature(QNetwork.launch)
    src = open(os.path.join(ROOT, "aquaticgymenv_amd", "fastpolicy.py")).read()
    assert "matmul" not in src and "torch.relu" not in src and " @ " not in src and "addmm" not in src and "argmax" not in src
    assert ".cpu()" not in src and "synchronize" not in src


# ------------------------------------------------------------------------------------------------ the compiler's listing
def test_codegen_f16_mfma_without_scratch_and_the_recorded_budget():
    isa = _isa.kernels("fastpol")
    acting = {n: k for n, k in isa.items() if "qfast_kernel" in n}
    assert len(acting) == 4 and len(isa) == 5 and any("refresh_kernel" in n for n in isa), sorted(isa)
    with open(os.path.join(ROOT, "profiles", "isa_budget.json")) as f:
        row = json.load(f)["qfast"]
    from aquaticgymenv_amd import build
    h = hashlib.sha256()
    for d in build.FASTPOL_DEPS:
        with open(d, "rb") as f:
            h.update(f.read())
    assert row["source_sha16"] == h.hexdigest()[:16], "run tools/make_fastpol_isa_budget.py"
    assert set(row["kernels"]) == set(isa)
    for name, k in isa.items():
        m = k["meta"]
        print("registers:", name, m)
        assert m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert "scratch_" not in k["body"], name
        assert not re.search(r"\b(global|flat|buffer|ds)_\w*atomic|\bds_(add|sub|inc|dec|min|max|and|or|xor|cmpst)_", k["body"]), name
        rec = row["kernels"][name]
        assert (rec["vgpr_count"], rec["agpr_count"], rec["sgpr_count"]) == (m["vgpr_count"], m["agpr_count"], m["sgpr_count"]), name
    for name, k in acting.items():
        m = k["meta"]
        # 6 (64 x 5: one k-step, two row blocks, three products) + 24 (64 x 64: four k-steps) in the tile body, which is there once
        assert len(re.findall(r"\bv_mfma_f32_32x32x16_f16\b", k["body"])) == 30, name
        assert len(re.findall(r"\bv_mfma_\w+", k["body"])) == 30 and "v_mfma_f32_32x32x2_f32" not in k["body"], name
        assert m["vgpr_count"] + m["agpr_count"] <= 256, (name, m)       # two wavefronts per SIMD (512 registers per lane)
        assert m["group_segment_fixed_size"] == 4 * 1296, (name, m)      # the LDS part, one copy per wavefront
        assert not re.search(r"v_cvt_\w*(bf16|fp8|bf8|bf6|fp6|fp4)", k["body"]) and "v_cvt_pkrtz" not in k["body"], name   # f16, rounded to nearest
    assert not any("v_mfma" in k["body"] for n, k in isa.items() if n not in acting)


def test_the_source_shares_the_network_and_states_nothing_twice():
    text = open(os.path.join(CSRC, "aqua_fastpol.hip")).read()
    assert set(re.findall(r'#include "([a-z_]+\.hpp)"', text)) == {"aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp"}
    assert '#include "aqua_fastpol.h"' in text
    assert "pick_and_store<EPS>(" in text and "for_each_parameter(" in text and "compute_units(" in text and "unit_of(" in text
    assert "__builtin_amdgcn_mfma_f32_32x32x16_f16" in text and "mfma_f32_32x32x2f32" not in text
    code = re.sub(r"//[^\n]*", "", text)
    assert "asm" not in code and "atomic" not in code.lower().replace("__atomic_release", "").replace("__atomic_acquire", "")
    assert not re.search(r"hipMalloc|hipFree|Synchronize|hipMemcpy|hipMemset", text)
    for name in ("aqua_fastpol.hip", "aqua_fastpol.h"):
        t = open(os.path.join(CSRC, name)).read()
        for once in ("constexpr int OFF_W1", "int compute_units(", "void grad_body(", "void apply_body(", "WS_STRIDE = 4744", "struct GradArgs",
                     "struct ApplyArgs"):
            assert once not in t, (name, once)


# ------------------------------------------------------------------------------------------------ the build recipe
KEPT = {"aqua_qnet.hpp": "27e07e1c95f0e0aec664a5fbd4938576853e04313cdebcc24a926d7ca2e682ed",
        "aqua_policy.hip": "49ec1b205c2840a6d8a03d7ede1d99fcddcbdf71069e6cc975c80e2275b8158e",
        "aqua_bank.hip": "adb98330ab14ef3ebb1fb21ac8d799e1650cb3a518e963519899980669c0568c",
        "aqua_qmap.hip": "456aa5127655f3855a22e2bbdf6c354906dec047631ed5cef37f2f987e8bd51e"}


def test_build_table_entry_and_the_lists():
    from aquaticgymenv_amd import build
    assert list(build.FAST_LIBRARIES) == ["fastpol"]
    assert build.twelve_libraries() == build.eleven_libraries() + ["fastpol"] and len(build.twelve_libraries()) == 12
    assert "fastpol" not in build.eleven_libraries()
    entry = build.library("fastpol")
    assert entry is build.FAST_LIBRARIES["fastpol"] and build.library("qmap") is build.MAP_LIBRARIES["qmap"]
    src = os.path.join(CSRC, "aqua_fastpol.hip")
    lib = os.path.join(ROOT, "aquaticgymenv_amd", "lib", "libaqua_fastpol.so")
    assert entry["src"] == [src] and entry["lib"] == lib and entry["cuid"] == "aqua_fastpol"
    included = re.findall(r'#include "([a-z_]+\.hpp)"', open(src).read())
    assert entry["deps"] == [src] + [os.path.join(CSRC, h) for h in sorted(included)] + [HEADER]
    assert sorted(included) == ["aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp"] and all(os.path.exists(p) for p in entry["deps"])
    assert build.build_command("fastpol") == [
        build.hipcc_path(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-fno-honor-nans", "-cuid=aqua_fastpol",
        "-Wall", "-Wno-unused-function", "-o", lib + ".tmp", src]
    assert (build.FASTPOL_SRC, build.FASTPOL_DEPS, build.FASTPOL_LIB, build.FASTPOL_FLAGS) == (entry["src"], entry["deps"], entry["lib"], entry["flags"])
    assert callable(build.build_fastpol) and build.fastpol_needs_build() in (True, False)
    assert len({build.library(n)["lib"] for n in build.twelve_libraries()}) == 12
    main = open(os.path.join(ROOT, "aquaticgymenv_amd", "build.py")).read().split('if __name__ == "__main__":')[1]
    assert "+ list(MAP_LIBRARIES) + list(FAST_LIBRARIES)" in main
    # the sources the acting libraries share or are stay byte for byte what they were when this library was added: policy,
    # bank and qmap then compile to the code they compiled to (the compiler's input is these files and their command lines)
    for name, sha in KEPT.items():
        with open(os.path.join(CSRC, name), "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == sha, "%s has changed: the fast path was built beside it, not into it" % name
    # the eleven others: names, order, sources and command lines as they were
    assert build.eleven_libraries() == ["hip", "policy", "learner", "episodes", "render", "replay", "bank", "lbank", "segments", "pbt", "qmap"]
    for name in build.eleven_libraries():
        e = build.library(name)
        assert e["src"] == [os.path.join(CSRC, "aqua_%s.hip" % name)] and not any("fastpol" in d for d in e["deps"]), name
        assert build.build_command(name)[1:-3] == ["-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-fno-honor-nans",
                                                   "-cuid=aqua_" + name, "-Wall", "-Wno-unused-function"], name


def test_graft_entry_builds_and_checks_the_new_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "every_library()" in text and "FAST_LIBRARIES" in text and "_fastpol_capi" in text and "aquafast_version" in text
    build_body = text.split("def build():")[1].split("def smoke():")[0]
    tables = re.findall(r"\b([A-Z]+_LIBRARIES)\b", build_body.split("aqua_oracle")[0])
    assert tables[-1] == "FAST_LIBRARIES"                        # build()'s list ends with the new library
