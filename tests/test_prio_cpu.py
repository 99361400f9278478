"""CPU-only checks of libaqua_prio.so (aquaticgymenv_amd/csrc/aqua_prio.h), prioritised experience replay: it builds and
loads, exports what its header declares, has a build-table entry of its own behind the pinned ones, rejects bad arguments
before touching a device and names the field, lays the trees out as the model does, computes x^e within 2^-40 of float64's and
the quantiser, beta and the weights from it; the model the GPU tests compare against (tests/_prio_model.py) descends as
np.searchsorted does on the cumulative sums; and the compiler's listing shows the weighted gradient kernels to be the
learner's, without scratch, spills, reduced precision or a float atomic."""
import ctypes
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from tests import _isa
from tests import _prio_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aquaticgymenv_amd", "csrc")
HEADER = os.path.join(CSRC, "aqua_prio.h")
FAKE = 0x100000           # a 512-byte aligned "device pointer" for calls that must fail (or return) before anything dereferences it
STACK = 0x1000000


@pytest.fixture(scope="module")
def capi():
    from aquaticgymenv_amd.build import build_library
    assert os.path.exists(build_library("prio"))
    from aquaticgymenv_amd import _prio_capi
    return _prio_capi


# ------------------------------------------------------------------------------------------------ the library and its table
def test_library_builds_loads_and_exports_its_header(capi):
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(aquaprio_[a-z0-9_]+)\s*\(", code))
    assert declared == set(capi.SYMBOLS) and len(declared) == 11, declared ^ set(capi.SYMBOLS)
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    assert capi.lib.aquaprio_version() == capi.ABI_VERSION == 1
    assert set(capi._SIGNATURES) == set(capi.SYMBOLS) - {"aquaprio_version", "aquaprio_last_error"}

    def define(name):
        return int(re.search(r"#define\s+%s\s+\(?(-?\d+)" % name, text).group(1))
    assert define("AQUAPRIO_ABI_VERSION") == 1
    assert [define("AQUAPRIO_E_" + n) for n in ("INVALID", "ALIGN", "NODEVICE")] == [-1, -2, -3] == [capi.E_INVALID, capi.E_ALIGN, capi.E_NODEVICE]
    from aquaticgymenv_amd import _lbank_capi, _learner_capi, _replay_capi
    assert define("AQUAPRIO_FANOUT") == capi.FANOUT == M.FAN == 64 and define("AQUAPRIO_FRAC_BITS") == capi.FRAC_BITS == 20
    assert define("AQUAPRIO_ONE") == capi.ONE == M.ONE == 2 ** 20 and define("AQUAPRIO_QMAX") == capi.QMAX == M.QMAX == 2 ** 31 - 1
    assert define("AQUAPRIO_MAX_LEVELS") == capi.MAX_LEVELS == 7 and define("AQUAPRIO_LAYOUT_WORDS") == capi.LAYOUT_WORDS == 24
    assert define("AQUAPRIO_MAX_CAPACITY") == capi.MAX_CAPACITY == _replay_capi.MAX_CAPACITY
    assert define("AQUAPRIO_MAX_NETWORKS") == capi.MAX_NETWORKS == _lbank_capi.MAX_NETWORKS
    assert define("AQUAPRIO_MAX_BATCH") == capi.MAX_BATCH == _lbank_capi.MAX_BATCH
    assert define("AQUAPRIO_MAX_BLOCKS") == capi.MAX_BLOCKS and define("AQUAPRIO_BLOCK") == capi.BLOCK == 64 * capi.WAVES
    # a stream of its own: 0, 1, 3, 4 are the environment's, 5 the policy's, 6 the learners'
    assert define("AQUAPRIO_STREAM") == capi.STREAM == M.STREAM == 7 and capi.STREAM not in (0, 1, 3, 4, 5, _learner_capi.STREAM, _lbank_capi.STREAM)
    if shutil.which("nm"):
        nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True)
        assert nm.returncode == 0 and set(re.findall(r"\b(aquaprio_\w+)", nm.stdout)) == declared


def test_the_other_bindings_do_not_know_the_new_symbols(capi):
    from aquaticgymenv_amd import (_bank_capi, _capi, _episodes_capi, _fastpol_capi, _lbank_capi, _learner_capi, _nstep_capi, _pbt_capi,
                                   _policy_capi, _qmap_capi, _render_capi, _replay_capi, _segments_capi)
    others = (_capi, _policy_capi, _learner_capi, _episodes_capi, _render_capi, _replay_capi, _bank_capi, _lbank_capi, _segments_capi,
              _pbt_capi, _qmap_capi, _fastpol_capi, _nstep_capi)
    for other in others:
        assert not any(s.startswith("aquaprio_") for s in other.SYMBOLS)
        for name in capi.SYMBOLS:
            assert not hasattr(other.lib, name)


def test_build_table_entry_behind_the_pinned_tables():
    from aquaticgymenv_amd import build
    assert list(build.PRIORITY_LIBRARIES) == ["prio"]
    assert build.fourteen_libraries() == build.thirteen_libraries() + ["prio"] and len(build.fourteen_libraries()) == 14
    entry = build.library("prio")
    assert entry is build.PRIORITY_LIBRARIES["prio"] and build.library("nstep") is build.NSTEP_LIBRARIES["nstep"]
    src = os.path.join(CSRC, "aqua_prio.hip")
    lib = os.path.join(ROOT, "aquaticgymenv_amd", "lib", "libaqua_prio.so")
    headers = ["aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp", "aqua_lrn.hpp"]
    assert entry["src"] == [src] and entry["lib"] == lib and entry["cuid"] == "aqua_prio"
    assert re.findall(r'#include "([a-z_]+\.hpp)"', open(src).read()) == headers and '#include "aqua_prio.h"' in open(src).read()
    assert entry["deps"] == [src] + [os.path.join(CSRC, h) for h in headers] + [HEADER] and all(os.path.exists(p) for p in entry["deps"])
    assert build.build_command("prio") == [
        build.hipcc_path(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-fno-honor-nans", "-cuid=aqua_prio",
        "-Wall", "-Wno-unused-function", "-o", lib + ".tmp", src]
    assert (build.PRIO_SRC, build.PRIO_DEPS, build.PRIO_LIB, build.PRIO_FLAGS) == (entry["src"], entry["deps"], entry["lib"], entry["flags"])
    assert callable(build.build_prio) and build.prio_needs_build() in (True, False)
    assert len({build.library(n)["lib"] for n in build.fourteen_libraries()}) == 14
    main = open(os.path.join(ROOT, "aquaticgymenv_amd", "build.py")).read().split('if __name__ == "__main__":')[1]
    assert "+ list(FAST_LIBRARIES) + list(NSTEP_LIBRARIES) + list(PRIORITY_LIBRARIES)" in main
    for name in build.thirteen_libraries():
        assert not any("prio" in os.path.basename(d) for d in build.library(name)["deps"]), name
    # the update's device code is the learner's: instantiated here, stated in aqua_lrn.hpp
    text = open(src).read()
    assert "grad_body<STRAT, true>" in text and "apply_body(" in text and "__builtin_amdgcn_mfma" not in text


def test_graft_entry_builds_and_checks_the_new_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    build_body = text.split("def build():")[1].split("def smoke():")[0]
    assert "fourteen_libraries()[13:]" in build_body and "_prio_capi" in build_body and "aquaprio_version" in build_body
    import __graft_entry__ as entry
    from aquaticgymenv_amd import build
    assert entry.build() is None and os.path.exists(build.PRIO_LIB)


# ------------------------------------------------------------------------------------------------ the C API without a device
SHAPE = dict(capacity=11520, N=160, seg=64, P=3)
TREE = dict(tree=FAKE, tree_bytes=1 << 20)


def _call(lib, entry, order, defaults, kw):
    a = dict(defaults)
    a.update(kw)
    return getattr(lib, entry)(*[a[name] for name in order], None)


def _insert(lib, **kw):
    order = ("tree", "tree_bytes", "pmax", "capacity", "N", "seg", "P", "header", "ok")
    return _call(lib, "aquaprio_insert", order, dict(TREE, pmax=FAKE + STACK, header=FAKE + 2 * STACK, ok=FAKE + 3 * STACK, **SHAPE), kw)


def _set(lib, **kw):
    order = ("tree", "tree_bytes", "pmax", "capacity", "N", "seg", "P", "idx", "td", "B", "alpha", "eps")
    return _call(lib, "aquaprio_set", order, dict(TREE, pmax=FAKE + STACK, idx=FAKE + 2 * STACK, td=FAKE + 3 * STACK, B=64, alpha=0.6, eps=1e-3,
                                                  **SHAPE), kw)


def _draw(lib, **kw):
    order = ("tree", "tree_bytes", "capacity", "N", "seg", "P", "header", "t", "seed", "idx", "weight", "q", "B", "beta0", "anneal")
    return _call(lib, "aquaprio_draw", order, dict(TREE, header=FAKE + STACK, t=FAKE + 2 * STACK, seed=FAKE + 3 * STACK, idx=FAKE + 4 * STACK,
                                                   weight=FAKE + 5 * STACK, q=FAKE + 6 * STACK, B=64, beta0=0.4, anneal=1000, **SHAPE), kw)


def _update(lib, **kw):
    a = dict(theta=FAKE, target=FAKE + STACK, m=FAKE + 2 * STACK, v=FAKE + 3 * STACK, t=FAKE + 4 * STACK, P=3, s=FAKE, a=FAKE, r=FAKE,
             s2=FAKE, d=FAKE, ok=FAKE, ld=1000, size=900, idx=FAKE, B=64, strategy=0, hyper=FAKE, blob=None, blob_t=None, perm=None,
             blob_floats=0, ws=FAKE, ws_bytes=1 << 40, idx_out=None, grad=None, loss=None, weight=FAKE + 6 * STACK, td=FAKE + 7 * STACK)
    a.update(kw)
    return lib.aquaprio_update_f32(a["theta"], a["target"], a["m"], a["v"], a["t"], a["P"], a["s"], a["a"], a["r"], a["s2"], a["d"],
                                   a["ok"], a["ld"], a["size"], a["idx"], a["B"], a["strategy"], a["hyper"], a["blob"], a["blob_t"],
                                   a["perm"], a["blob_floats"], a["ws"], a["ws_bytes"], a["idx_out"], a["grad"], a["loss"], a["weight"],
                                   a["td"], None)


# what every entry that takes the trees rejects, with the word its message must hold
BAD_SHAPES = [(dict(capacity=0), "capacity"), (dict(capacity=-5), "capacity"), (dict(capacity=2 ** 31), "capacity"),
              (dict(capacity=11521), "multiple"), (dict(capacity=11500), "multiple"), (dict(N=0), "N="), (dict(N=-160), "N="),
              (dict(N=11521), "N="), (dict(N=7), "multiple"), (dict(seg=0), "seg"), (dict(seg=-1), "seg"), (dict(seg=161), "seg"),
              (dict(P=0), "P="), (dict(P=-1), "P="), (dict(P=4097), "P="), (dict(tree=None), "tree"), (dict(tree_bytes=61439), "tree_bytes")]


def test_argument_validation_without_touching_a_device(capi):
    """every call here fails (or returns) before the first HIP call: nothing is launched, no pointer is dereferenced"""
    lib = capi.lib
    assert capi.layout(**SHAPE)["bytes"] == 61440
    nan, inf = float("nan"), float("inf")
    for fn in (_insert, _set, _draw):
        for kw, word in BAD_SHAPES:
            assert fn(lib, **kw) == capi.E_INVALID, (fn.__name__, kw)
            assert word in capi.last_error(), (fn.__name__, kw, capi.last_error())
        assert fn(lib, tree=FAKE + 256) == capi.E_ALIGN and "tree" in capi.last_error()
        assert fn(lib, tree_bytes=61440, header=FAKE + 4, idx=FAKE + 2) == capi.E_ALIGN     # the exact size passes the size check
    per_entry = [
        (_insert, [(dict(pmax=None), "pmax"), (dict(header=None), "header"), (dict(ok=None), "ok")], [dict(header=FAKE + 4), dict(pmax=FAKE + 2)]),
        (_set, [(dict(pmax=None), "pmax"), (dict(idx=None), "idx"), (dict(td=None), "td"), (dict(B=-1), "B="), (dict(B=capi.MAX_BATCH + 1), "B="),
                (dict(alpha=-0.1), "alpha"), (dict(alpha=1.01), "alpha"), (dict(alpha=nan), "alpha"), (dict(eps=0.0), "eps"),
                (dict(eps=-1e-3), "eps"), (dict(eps=nan), "eps"), (dict(eps=inf), "eps")],
         [dict(pmax=FAKE + 1), dict(idx=FAKE + 2), dict(td=FAKE + 3)]),
        (_draw, [(dict(header=None), "header"), (dict(t=None), "t_dev"), (dict(seed=None), "seed_dev"), (dict(idx=None), "idx"),
                 (dict(weight=None), "weight"), (dict(q=None), "q_out"), (dict(B=-1), "B="), (dict(B=capi.MAX_BATCH + 1), "B="),
                 (dict(beta0=-0.1), "beta0"), (dict(beta0=1.5), "beta0"), (dict(beta0=nan), "beta0"), (dict(anneal=0), "anneal"),
                 (dict(anneal=-3), "anneal")],
         [dict(header=FAKE + 4), dict(t=FAKE + 4), dict(seed=FAKE + 2), dict(idx=FAKE + 2), dict(weight=FAKE + 1), dict(q=FAKE + 2)]),
    ]
    for fn, invalid, misaligned in per_entry:
        for kw, word in invalid:
            assert fn(lib, **kw) == capi.E_INVALID, (fn.__name__, kw)
            assert word in capi.last_error(), (fn.__name__, kw, capi.last_error())
        for kw in misaligned:
            assert fn(lib, **kw) == capi.E_ALIGN, (fn.__name__, kw)
            assert capi.last_error()
    # nothing to do: no launch, no device, no rows needed; the ends of the ranges pass
    assert _set(lib, B=0, idx=None, td=None) == 0 and _draw(lib, B=0, idx=None, weight=None, q=None) == 0
    assert _set(lib, B=0, alpha=0.0, eps=1e-300) == 0 and _set(lib, B=0, alpha=1.0) == 0
    assert _draw(lib, B=0, beta0=0.0, anneal=1) == 0 and _draw(lib, B=0, beta0=1.0, anneal=2 ** 62) == 0
    assert _set(lib, B=0, seg=160, P=4096, tree_bytes=1 << 40) == 0 and _set(lib, B=0, seg=1, P=1) == 0
    # the update: the learner bank's rules, and both new rows are required
    stack3 = 3 * 4 * 4739
    invalid = [dict(P=0), dict(P=4097), dict(theta=None), dict(t=None), dict(m=FAKE), dict(target=FAKE + stack3 - 4), dict(B=-1),
               dict(B=capi.MAX_BATCH + 1), dict(ld=-1), dict(size=1001), dict(ld=2 ** 31, size=5), dict(strategy=-1), dict(strategy=4),
               dict(strategy=16 | 4), dict(hyper=None), dict(idx=None), dict(blob=FAKE + 5 * STACK), dict(s=None), dict(ok=None), dict(ws=None),
               dict(ws_bytes=3 * (16 + 4 * 4744) - 1), dict(weight=None), dict(td=None)]
    for kw in invalid:
        assert _update(lib, **kw) == capi.E_INVALID, kw
        assert capi.last_error(), kw
    assert _update(lib, weight=None) == capi.E_INVALID and "weight" in capi.last_error()
    for kw in (dict(theta=FAKE + 2), dict(t=FAKE + 4 * STACK + 4), dict(hyper=FAKE + 4), dict(s=FAKE + 1), dict(idx=FAKE + 2), dict(ws=FAKE + 8),
               dict(weight=FAKE + 2), dict(td=FAKE + 1), dict(loss=FAKE + 2)):
        assert _update(lib, **kw) == capi.E_ALIGN, kw
    assert _update(lib, B=0) == 0 and _update(lib, B=0, weight=None, td=None, idx=None, ws=None, ws_bytes=0) == 0
    assert _update(lib, ws_bytes=3 * (16 + 4 * 4744), ws=FAKE + 8) == capi.E_ALIGN      # the exact workspace passes the size check
    for strategy in (0, 1, 2, 3):
        assert _update(lib, B=0, strategy=strategy | 16) == 0
    with pytest.raises(ValueError, match="^aquaprio_set: alpha="):
        capi.check(_set(lib, alpha=2.0), "aquaprio_set")
    with pytest.raises(capi.AquaPriorityError):
        capi.check(_insert(lib, header=FAKE + 4), "aquaprio_insert")
    # the layout entry itself
    out = np.zeros(capi.LAYOUT_WORDS, dtype=np.int64)
    for kw, word in BAD_SHAPES[:15]:
        a = dict(SHAPE)
        a.update(kw)
        assert lib.aquaprio_layout(a["capacity"], a["N"], a["seg"], a["P"], out.ctypes.data) == capi.E_INVALID and word in capi.last_error(), kw
    assert lib.aquaprio_layout(11520, 160, 64, 3, None) == capi.E_INVALID and lib.aquaprio_layout(11520, 160, 64, 3, out.ctypes.data + 4) == capi.E_ALIGN


def test_no_cpu_path(capi):
    import torch
    from aquaticgymenv_amd.priority import PrioritizedReplay
    for bad in (object(), None, 3):
        with pytest.raises(ValueError):
            PrioritizedReplay(bad, object())
    env = types.SimpleNamespace(num_envs=8, continuous=False)
    ring = types.SimpleNamespace(torch=torch, env=env, header=object(), device=torch.device("cpu"), capacity=64)
    learners = types.SimpleNamespace(networks=2, seed_dev=None, hyper=None, seg=4, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="DQNLearnerBank"):
        PrioritizedReplay(ring, object())
    with pytest.raises(RuntimeError, match="no CPU path"):
        PrioritizedReplay(ring, learners)
    if not torch.cuda.is_available():
        ring.device = torch.device("cuda:0")
        with pytest.raises(RuntimeError, match="no CPU path"):
            PrioritizedReplay(ring, learners)
    src = open(os.path.join(ROOT, "aquaticgymenv_amd", "priority.py")).read()
    assert "cumsum" not in src and "searchsorted" not in src and "multinomial" not in src and ".pow(" not in src


# ------------------------------------------------------------------------------------------------ the layout
@pytest.mark.parametrize("L0", [1, 64, 65, 4096, 4097, 2 ** 24])
def test_layout_equals_the_model(capi, L0):
    # one world per network and L0 rounds; then the same leaves from more worlds per network, ragged, and with idle networks
    shapes = [(L0 * 3, 3, 1, 3), (L0 * 3, 3, 1, 5)]
    if L0 % 4 == 0:
        shapes += [(L0 // 4 * 10, 10, 4, 3), (L0 // 4 * 10, 10, 4, 7), (L0 // 4 * 4, 4, 4, 1)]
    for capacity, N, seg, P in shapes:
        got, want = capi.layout(capacity, N, seg, P), M.layout(capacity, N, seg, P)
        assert got == want, (capacity, N, seg, P, got, want)
        assert got["leaves"] == L0 and got["n"][-1] == 1 and got["levels"] >= 2 and got["levels"] <= capi.MAX_LEVELS
        assert all(b == -(-a // 64) for a, b in zip(got["n"], got["n"][1:])) and all(s % 64 == 0 and s >= n for s, n in zip(got["stride"], got["n"]))
        assert all(o % 512 == 0 for o in got["offset"])
        sizes = [P * s * (4 if k == 0 else 8) for k, s in enumerate(got["stride"])]
        assert all(o + z <= o2 for o, z, o2 in zip(got["offset"], sizes, got["offset"][1:] + [got["bytes"]]))
    assert capi.layout(72 * 160, 160, 64, 3)["n"] == [4608, 72, 2, 1]
    assert capi.layout(2 ** 31 - 1, 1, 1, 1)["levels"] == capi.MAX_LEVELS


# ------------------------------------------------------------------------------------------------ the floating point
EXPONENTS = (0.0, 0.25, 0.4, 0.5, 0.6, 0.7, 1.0)


def test_pow_is_within_two_to_the_minus_forty_of_float64(capi):
    rng = np.random.RandomState(1)
    xs = np.concatenate([2.0 ** rng.uniform(-30, 12, 4000), 2.0 ** np.arange(-30, 13, dtype=np.float64), [np.sqrt(2.0), np.sqrt(0.5), 1.0, 1e-3]])
    worst = 0.0
    for e in EXPONENTS:
        want = xs ** np.float64(e)
        got = np.array([capi.lib.aquaprio_pow(float(x), e) for x in xs])
        worst = max(worst, float(np.max(np.abs(got - want) / want)))
    print("largest relative error of aquaprio_pow: 2^%.1f" % np.log2(worst))
    assert worst <= 2.0 ** -40
    assert all(capi.lib.aquaprio_pow(float(x), 0.0) == 1.0 for x in xs[:50])
    # negative exponents (the weights) and the ends of the range
    for x in (2.0 ** -31, 2.0 ** 62, 2.0 ** -1000, 2.0 ** 1000):
        for e in (-1.0, -0.4, 0.4, 1.0):
            got, want = capi.pow_(x, e), float(np.float64(x) ** np.float64(e))
            assert abs(got - want) <= want * 2.0 ** -40, (x, e)
    for x, e in ((0.0, 0.5), (-1.0, 0.5), (float("nan"), 0.5), (float("inf"), 0.5), (2.0 ** -1001, 0.5), (2.0, 1.5), (2.0, float("nan"))):
        assert capi.lib.aquaprio_pow(x, e) == -1.0 and capi.last_error()
        with pytest.raises(ValueError):
            capi.pow_(x, e)


def test_quantiser_equals_the_float64_model_away_from_ties(capi):
    rng = np.random.RandomState(2)
    tds = np.concatenate([rng.exponential(1.0, 3000), 10.0 ** rng.uniform(-8, 4, 1000), [0.0, 1.0, 0.5]]).astype(np.float32).astype(np.float64)
    checked = near = 0
    for alpha in EXPONENTS:
        for eps in (1e-3, 1e-6):
            x = M.pi64(tds, alpha, eps) * 2.0 ** 20
            want = np.clip(np.rint(x), 1, M.QMAX).astype(np.int64)
            got = np.array([capi.lib.aquaprio_quantise(float(t), alpha, eps) for t in tds], dtype=np.int64)
            tie = np.abs(x - np.floor(x) - 0.5) <= x * 2.0 ** -39
            assert np.array_equal(got[~tie], want[~tie]), (alpha, eps)
            assert bool((np.abs(got - want) <= 1).all())
            checked += int((~tie).sum())
            near += int(tie.sum())
    print("quantiser: %d values equal, %d within 1 next to a tie" % (checked, near))
    # the clamps, hit on purpose
    assert capi.quantise(0.0, 1.0, 1e-9) == 1 and capi.quantise(0.0, 1.0, 2.0 ** -22) == 1 and capi.quantise(0.0, 0.5, 1e-300) == 1
    assert capi.quantise(1e30, 1.0, 1e-3) == M.QMAX and capi.quantise(2048.0, 1.0, 1e-3) == M.QMAX and capi.quantise(3.4e38, 0.5, 1e-3) == M.QMAX
    assert capi.quantise(2047.0, 1.0, 0.5) == int(2047.5 * 2 ** 20) < M.QMAX
    assert capi.quantise(5.0, 0.0, 1e-3) == M.ONE                                  # alpha = 0: uniform replay
    for td, alpha, eps in ((-1.0, 0.6, 1e-3), (float("nan"), 0.6, 1e-3), (float("inf"), 0.6, 1e-3), (1.0, -0.1, 1e-3), (1.0, 1.1, 1e-3),
                           (1.0, 0.6, 0.0), (1.0, 0.6, -1.0), (1.0, 0.6, float("nan"))):
        assert capi.lib.aquaprio_quantise(td, alpha, eps) == 0 and capi.last_error()
        with pytest.raises(ValueError):
            capi.quantise(td, alpha, eps)


def test_quantiser_rounds_ties_to_even(capi):
    """the values the test above leaves out: eps (td = 0, alpha = 1) whose scaled priority is exactly k + 1/2 by the library's
    own x^e (tests/_prio_model.py::ties finds two odd and two even k) quantises to the even neighbour"""
    ties = M.ties(capi)
    assert sorted(k & 1 for k, _ in ties) == [0, 0, 1, 1]
    for k, eps in ties:
        assert capi.pow_(eps, 1.0) * M.ONE == k + 0.5 and abs(eps * M.ONE - (k + 0.5)) <= (k + 0.5) * 2.0 ** -44
        assert capi.quantise(0.0, 1.0, eps) == k + (k & 1), (k, eps)


def test_beta_is_the_formula_bit_for_bit_and_the_weights_are_close(capi):
    for beta0 in (0.0, 0.4, 0.7, 1.0):
        for anneal in (1, 3, 1000, 100000, 2 ** 40):
            for t in (0, 1, 2, anneal // 3, anneal - 1, anneal, anneal + 1, 2 ** 50):
                got, want = capi.lib.aquaprio_beta(t, beta0, anneal), M.beta64(t, beta0, anneal)
                assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (t, beta0, anneal)
                assert beta0 <= got <= 1.0 and (t < anneal or got == 1.0)
    for beta0, anneal in ((-0.1, 10), (1.1, 10), (float("nan"), 10), (0.4, 0), (0.4, -1)):
        assert capi.lib.aquaprio_beta(5, beta0, anneal) == -1.0 and capi.last_error()
    rng = np.random.RandomState(3)
    worst = 0.0
    for _ in range(3000):
        size = int(rng.randint(1, 2 ** 31 - 1))
        q = int(rng.randint(1, 2 ** 31 - 1))
        T = q + int(rng.randint(0, 2 ** 31)) * int(rng.randint(0, 2 ** 30))
        beta = float(rng.choice([0.0, 0.4, 0.55, 1.0, rng.rand()]))
        got, want = capi.weight(size, q, T, beta), M.weight64(size, q, T, beta)
        worst = max(worst, abs(got - want) / want)
    print("largest relative error of aquaprio_weight: 2^%.1f" % np.log2(worst))
    assert worst <= 2.0 ** -39
    assert capi.weight(7, 5, 35, 0.4) == 1.0 and capi.weight(100, M.ONE, M.ONE, 0.0) == 1.0
    for size, q, T, beta in ((0, 5, 35, 0.4), (7, 0, 35, 0.4), (7, 5, 4, 0.4), (7, 5, 2 ** 62, 0.4), (7, 5, 35, 1.5), (7, 5, 35, -0.1)):
        assert capi.lib.aquaprio_weight(size, q, T, beta) == -1.0 and capi.last_error()


# ------------------------------------------------------------------------------------------------ the model itself
def test_the_model_descends_as_searchsorted_does():
    rng = np.random.RandomState(4)
    lay = M.layout(72 * 160, 160, 64, 3)
    leaves = (rng.randint(1, 2 ** 31, lay["leaves"]) * (rng.rand(lay["leaves"]) < 0.7)).astype(np.uint32)
    leaves[4000:] = 0                                                   # a ragged network: nothing behind its last leaf
    cum = [int(x) for x in np.cumsum(leaves.astype(np.uint64), dtype=np.uint64)]
    total = cum[-1]
    assert int(M.sums_above(leaves, lay["n"])[-1][0]) == total and len(M.sums_above(leaves, lay["n"])) == 3
    cum64 = np.array(cum, dtype=np.uint64)
    us = [int(rng.randint(0, 2 ** 31)) * 2 ** 31 % total for _ in range(3000)] + [int(x) % total for x in rng.randint(0, 2 ** 62, 97000)]
    want = np.searchsorted(cum64, np.array(us, dtype=np.uint64), side="right")
    levels = [leaves.astype(np.uint64)] + M.sums_above(leaves, lay["n"])
    for u, c in zip(us[:4000], want[:4000]):
        assert M.descend(leaves, lay["n"], u) == c and leaves[c] != 0
    # all 10^5 through a vectorised restatement of the same descent
    node, rest = np.zeros(len(us), dtype=np.int64), np.array(us, dtype=np.uint64)
    for k in range(len(levels) - 1, 0, -1):
        below = np.zeros(lay["stride"][k - 1], dtype=np.uint64)
        below[:levels[k - 1].size] = levels[k - 1]
        kids = below[(node[:, None] * 64 + np.arange(64)[None, :])]
        prefix = np.cumsum(kids, axis=1, dtype=np.uint64)
        sel = (prefix <= rest[:, None]).sum(axis=1)
        assert bool((sel < 64).all())
        rest = rest - (prefix[np.arange(len(us)), sel] - kids[np.arange(len(us)), sel])
        node = node * 64 + sel
    assert np.array_equal(node, want) and bool((leaves[node] != 0).all())
    # a small tree, every u on a prefix boundary and next to it
    small = np.array([3, 0, 0, 5, 1, 0, 7] + [0] * 60 + [2, 0, 9], dtype=np.uint32)
    n = [small.size, 2, 1]
    cs = np.cumsum(small.astype(np.uint64), dtype=np.uint64)
    for u in range(int(cs[-1])):
        c = M.descend(small, n, u)
        assert c == int(np.searchsorted(cs, np.uint64(u), side="right")) and small[c] != 0
    with pytest.raises(AssertionError):
        M.descend(small, n, int(cs[-1]))
    # the slots: leaf <-> slot is a bijection on a network's slots
    for N, seg, P in ((160, 64, 3), (10, 4, 3), (10, 4, 7), (5, 5, 1)):
        seen = set()
        for slot in range(4 * N):
            p, c = M.leaf_of_slot(slot, N, seg)
            assert p < -(-N // seg) and M.slot_of_leaf(p, c, N, seg) == slot and (p, c) not in seen and c < 4 * seg
            seen.add((p, c))
        assert all(M.worlds(N, seg, p) == 0 for p in range(-(-N // seg), P))


# ------------------------------------------------------------------------------------------------ the compiler's listing
def test_codegen_weighted_gradient_kernels_are_the_learners():
    isa = _isa.kernels("prio")
    grad = {n: k for n, k in isa.items() if "prio_grad_kernel" in n}
    assert len(grad) == 4 and len(isa) == 9, sorted(isa)
    for kernel in ("prio_insert_kernel", "prio_set_kernel", "prio_descend_kernel", "prio_weight_kernel", "prio_apply_kernel"):
        assert sum(kernel in n for n in isa) == 1, kernel
    for name, k in isa.items():
        m = k["meta"]
        print("registers:", name, m)
        assert m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert "scratch_" not in k["body"] and k["stats"]["ScratchSize"] == 0, name
        assert not re.search(r"v_mfma_\w*(bf16|f16|fp8|bf8|f8f6f4|i8)|v_cvt_\w*(bf16|f16|fp8|bf8|bf6|fp6|fp4)", k["body"]), name
        assert not re.search(r"atomic_\w*(f32|f64)|atomic_(fadd|fmin|fmax|pk_add)", k["body"]), name      # no float atomics
    learner = _isa.kernels("learner")
    theirs = {n: k for n, k in learner.items() if "lrn_grad_kernel" in n}
    count = lambda k: len(re.findall(r"\bv_mfma_f32_32x32x2_f32\b", k["body"]))
    assert sorted(count(k) for k in grad.values()) == sorted(count(k) for k in theirs.values()) == [2 * 70 + 64 + 160] * 3 + [3 * 70 + 64 + 160]
    assert sorted(k["meta"]["group_segment_fixed_size"] for k in grad.values()) == sorted(k["meta"]["group_segment_fixed_size"] for k in theirs.values())
    for n, k in isa.items():
        if n not in grad:
            assert "v_mfma" not in k["body"], n
    # the tree is kept by integer atomics: an exchange on the leaf, 64-bit adds above it, a max on pmax
    set_body = next(k["body"] for n, k in isa.items() if "prio_set_kernel" in n)
    assert re.search(r"atomic_swap\b", set_body) and re.search(r"atomic_add_(x2|u64)\b", set_body) and re.search(r"atomic_(u)?max(_u32)?\b", set_body)
