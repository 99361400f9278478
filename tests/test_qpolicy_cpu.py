"""CPU-only checks of libaqua_policy.so (include/aqua_policy.h), the Q-network library: it builds and loads, exports
what its header declares and leaves libaqua_hip.so's interface alone, rejects bad arguments before touching a device,
packs weights deterministically in the layout the kernel's MFMA orientation needs (re-stated here lane by lane), and
the compiled kernel keeps the 64 x 64 layer on v_mfma_f32_32x32x2_f32 without scratch or spills."""
import ctypes
import hashlib
import json
import os
import re

import numpy as np
import pytest

from tests import _isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000            # a "device pointer" for calls that must fail (or return) before anything dereferences it


@pytest.fixture(scope="module")
def pcapi():
    from aquaticgymenv_amd.build import build_policy
    path = build_policy()
    assert os.path.exists(path)
    from aquaticgymenv_amd import _policy_capi
    return _policy_capi


@pytest.fixture(scope="module")
def isa():
    return _isa.kernels("policy")


def _int_layers():
    """small asymmetric integers, a different formula per layer, biases of both signs"""
    i5, i64, i3 = np.arange(5)[:, None], np.arange(64)[:, None], np.arange(3)[None, :]
    j64 = np.arange(64)[None, :]
    k0 = ((2 * i5 + 3 * j64) % 5 - 2).astype(np.float32)
    k1 = ((3 * i64 + 5 * j64) % 7 - 3).astype(np.float32)
    k2 = ((5 * i64 + 2 * i3) % 7 - 3).astype(np.float32)
    b0 = ((np.arange(64) * 3) % 5 - 2).astype(np.float32)
    b1 = ((np.arange(64) * 5) % 7 - 3).astype(np.float32)
    b2 = np.array([2, -1, 1], dtype=np.float32)
    return [(k0, b0), (k1, b1), (k2, b2)]


def test_library_builds_loads_and_exports_its_header(pcapi):
    text = open(os.path.join(ROOT, "include", "aqua_policy.h")).read()
    declared = set(re.findall(r"\b(aquapol_[a-z0-9_]+)\s*\(", text))
    assert declared == set(pcapi.SYMBOLS), declared ^ set(pcapi.SYMBOLS)
    raw = ctypes.CDLL(pcapi.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    assert pcapi.lib.aquapol_version() == pcapi.ABI_VERSION == 1
    assert int(re.search(r"#define\s+AQUAPOL_ABI_VERSION\s+(\d+)", text).group(1)) == 1
    assert [int(re.search(r"#define\s+AQUAPOL_E_%s\s+\((-\d+)\)" % n, text).group(1)) for n in ("INVALID", "ALIGN", "NODEVICE")] \
        == [-1, -2, -3]
    # the environment's library is not touched: its header declares nothing of this one, its binding is as long as before
    from aquaticgymenv_amd import _capi
    assert "aquapol_" not in open(os.path.join(ROOT, "include", "aqua_hip.h")).read()
    assert len(_capi.SYMBOLS) == 38 and not any(s.startswith("aquapol") for s in _capi.SYMBOLS)
    for name in pcapi.SYMBOLS:
        assert not hasattr(_capi.lib, name)


def test_build_recipe_is_separate_from_the_environment_library():
    from aquaticgymenv_amd import build
    assert build.POLICY_LIB != build.LIB and "-cuid=aqua_policy" in build.POLICY_FLAGS and "-cuid=aqua_hip" in build.COMMON_FLAGS
    assert sorted(f for f in build.POLICY_FLAGS if not f.startswith("-cuid")) == sorted(f for f in build.COMMON_FLAGS if not f.startswith("-cuid"))
    assert not set(build.POLICY_SRC) & set(build.SRC)


def test_packing_is_deterministic_and_sized(pcapi):
    n = pcapi.lib.aquapol_weights_bytes()
    layers = _int_layers()
    a, b = pcapi.pack_weights(layers), pcapi.pack_weights([(k.copy(), v.copy()) for k, v in layers])
    assert a.nbytes == n == b.nbytes and np.array_equal(a, b)
    # exactly n bytes are written: a guard behind the blob survives
    ks = [np.ascontiguousarray(k) for k, _ in layers]
    bs = [np.ascontiguousarray(v) for _, v in layers]
    buf = np.full(n + 64, 0xA5, dtype=np.uint8)
    shapes = (ctypes.c_int * 4)(5, 64, 64, 3)
    rc = pcapi.lib.aquapol_pack_weights(ks[0].ctypes.data, bs[0].ctypes.data, ks[1].ctypes.data, bs[1].ctypes.data,
                                        ks[2].ctypes.data, bs[2].ctypes.data, shapes, buf.ctypes.data, n + 64)
    assert rc == 0 and np.array_equal(buf[:n], a) and bool((buf[n:] == 0xA5).all())
    # a pure permutation (plus zero padding): every weight and bias is somewhere in the blob, nothing else is
    f = a.view(np.float32)
    want = np.concatenate([np.concatenate([k.reshape(-1), v]) for k, v in layers])
    assert sorted(f[f != 0].tolist()) == sorted(want[want != 0].tolist())


def _emulate(blob, x):
    """The kernel re-stated lane by lane in int64 from the BLOB alone (aqua_qnet.hpp's layout comment): worlds on the
    MFMA's column index, units on its rows, accumulator register r of lane half h = row (r & 3) + 8 (r >> 2) + 4 h,
    A operand lane l = A[l & 31][k = l >> 5], B operand lane l = B[k = l >> 5][l & 31].  x: int [5][32] -> q int64 [3][32]."""
    f = blob.view(np.float32).astype(np.int64)
    w1 = f[0:384].reshape(3, 2, 64)
    w2 = f[384:384 + 4096].reshape(2, 32, 64)
    lds = f[4480:]
    b0, b1 = lds[0:64].reshape(2, 32), lds[64:128].reshape(2, 32)
    k2, b2 = lds[128:320].reshape(2, 3, 32), lds[320:323]
    rows = np.array([[(r & 3) + 8 * (r >> 2) + 4 * h for r in range(16)] for h in range(2)])      # [h][r]

    def mfma(a_lane, b_lane, acc):
        """acc[h][r][col] += sum_k A[row(r, h)][k] B[k][col]"""
        a = a_lane.reshape(2, 32)                  # [k][i]
        b = b_lane.reshape(2, 32)                  # [k][j]
        for h in range(2):
            for r in range(16):
                acc[h, r] += a[0, rows[h, r]] * b[0] + a[1, rows[h, r]] * b[1]
        return acc

    xin = np.zeros((3, 64), dtype=np.int64)        # k-step s, lane (h, col): input 2 s + h
    for s in range(3):
        for h in range(2):
            if 2 * s + h < 5:
                xin[s, 32 * h:32 * h + 32] = x[2 * s + h]
    h1 = [np.repeat(b0[:, 16 * m:16 * m + 16, None], 32, axis=2).copy() for m in range(2)]      # [M][h][r][col]
    h2 = [np.repeat(b1[:, 16 * m:16 * m + 16, None], 32, axis=2).copy() for m in range(2)]
    for s in range(3):
        for m in range(2):
            h1[m] = mfma(w1[s, m], xin[s], h1[m])
    for m in range(2):
        for r in range(16):
            b = np.maximum(h1[m][:, r, :], 0).reshape(64)                # each lane's own register r of block m
            for m2 in range(2):
                h2[m2] = mfma(w2[m2, m * 16 + r], b, h2[m2])
    q = np.zeros((3, 32), dtype=np.int64)
    for c in range(3):
        for h in range(2):
            p = np.full(32, b2[c] if h == 0 else 0, dtype=np.int64)
            for m in range(2):
                for r in range(16):
                    p += k2[h, c, m * 16 + r] * np.maximum(h2[m][h, r], 0)
            q[c] += p
    return q


def test_blob_layout_computes_the_network(pcapi):
    """the packer's permuted k order against the MFMA lane maps the kernel relies on, in exact integer arithmetic"""
    layers = _int_layers()
    blob = pcapi.pack_weights(layers)
    rng = np.random.RandomState(5)
    x = rng.randint(0, 4, size=(5, 32)).astype(np.int64)
    (k0, b0), (k1, b1), (k2, b2) = [(k.astype(np.int64), b.astype(np.int64)) for k, b in layers]
    h = np.maximum(x.T @ k0 + b0, 0)
    h = np.maximum(h @ k1 + b1, 0)
    want = (h @ k2 + b2).T
    assert np.array_equal(_emulate(blob, x), want)
    assert len(np.unique(want)) > 20                 # not a degenerate case


def test_argument_validation_without_touching_a_device(pcapi):
    lib = pcapi.lib
    layers = _int_layers()
    ks = [np.ascontiguousarray(k) for k, _ in layers]
    bs = [np.ascontiguousarray(v) for _, v in layers]
    n = lib.aquapol_weights_bytes()
    buf = np.zeros(n, dtype=np.uint8)

    def err():
        return lib.aquapol_last_error().decode()

    def pack(shapes=(5, 64, 64, 3), nbytes=n, k1=ks[1].ctypes.data, out=buf.ctypes.data):
        return lib.aquapol_pack_weights(ks[0].ctypes.data, bs[0].ctypes.data, k1, bs[1].ctypes.data, ks[2].ctypes.data,
                                        bs[2].ctypes.data, (ctypes.c_int * 4)(*shapes) if shapes else None, out, nbytes)

    assert pack() == 0
    for shapes in ((5, 64, 64, 2), (4, 64, 64, 3), (5, 32, 64, 3), (5, 64, 128, 3)):
        assert pack(shapes=shapes) == -1 and "5-64-64-3" in err()
    assert pack(shapes=None) == -1 and err()
    assert pack(nbytes=n - 1) == -1 and "small" in err()
    assert pack(k1=None) == -1 and err()
    assert pack(out=None) == -1 and err()
    with pytest.raises(ValueError):
        pcapi.pack_weights(layers[:2])
    with pytest.raises(ValueError):
        pcapi.pack_weights([(np.zeros((5, 32), np.float32), np.zeros(32, np.float32)), (np.zeros((32, 64), np.float32), np.zeros(64, np.float32)),
                            layers[2]])

    def act(w=FAKE, inp=FAKE, ld=128, norm=1, N=100, off=0, eps=0.0, tb=None, action=FAKE, q=None, q_ld=0, qt=None):
        return lib.aquapol_act_f32(w, inp, ld, norm, N, off, eps, 1, 2, tb, action, q, q_ld, qt, None)

    cases = [(dict(w=None), -1), (dict(w=FAKE + 8), -2), (dict(N=-1), -1), (dict(ld=99), -1), (dict(off=-1), -1),
             (dict(eps=float("nan")), -1), (dict(eps=-0.25), -1), (dict(action=None), -1), (dict(q=FAKE, q_ld=99), -1),
             (dict(inp=None), -1), (dict(inp=FAKE + 2), -2), (dict(q=FAKE + 1, q_ld=100), -2), (dict(qt=FAKE + 3), -2),
             (dict(tb=FAKE + 4), -2)]
    for kw, code in cases:
        assert act(**kw) == code, kw
        assert err(), kw
    # N == 0: nothing to do, no launch, no device needed
    assert act(N=0, ld=0) == 0
    assert act(N=0, ld=0, action=None, q=FAKE, q_ld=0, qt=FAKE) == 0


def test_codegen_keeps_the_hidden_layer_on_the_f32_mfma_without_scratch(isa):
    ks = isa
    assert len(ks) == 4, sorted(ks)                    # raw / normalised input x greedy / epsilon-greedy
    counts = {}
    for name, k in ks.items():
        m = k["meta"]
        assert m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert "scratch_" not in k["body"], name
        counts[name] = len(re.findall(r"\bv_mfma_f32_32x32x2_f32\b", k["body"]))
        assert counts[name] >= 1, name
        # no reduced-precision matrix or conversion instruction anywhere in the network
        assert not re.search(r"v_mfma_\w*(bf16|f16|fp8|bf8|f8f6f4|i8)|v_cvt_\w*(bf16|f16|fp8|bf8)", k["body"]), name
        assert m["vgpr_count"] + m["agpr_count"] <= 170, (name, m)      # three wavefronts per SIMD (512 registers per lane)
    print("static v_mfma_f32_32x32x2_f32 per instantiation:", counts)
    assert set(counts.values()) == {70}                # 6 (64 x 5, K padded to 6) + 64 (64 x 64) per tile of 32 worlds, unrolled


def test_committed_isa_record_is_of_this_source():
    with open(os.path.join(ROOT, "profiles", "isa_budget.json")) as f:
        row = json.load(f)["qpolicy"]
    from aquaticgymenv_amd import build
    h = hashlib.sha256()                               # the kernel's body is in aqua_qnet.hpp: every dependency, in table order
    for dep in build.POLICY_DEPS:
        with open(dep, "rb") as f:
            h.update(f.read())
    assert row["source_sha16"] == h.hexdigest()[:16], "run tools/make_policy_isa_budget.py"
    assert row["source"] == [os.path.relpath(dep, ROOT) for dep in build.POLICY_DEPS] and len(row["source"]) == 5
    assert len(row["kernels"]) == 4
    for k in row["kernels"].values():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["occupancy_waves_per_simd"] >= 3


def test_no_cpu_fallback_for_the_network():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from aquaticgymenv_amd.qpolicy import QNetwork
    with pytest.raises(RuntimeError):
        QNetwork(_int_layers(), device="cuda:0")
    with pytest.raises(RuntimeError):
        QNetwork(_int_layers(), device="cpu")
