"""CPU-only checks of libaqua_evo.so (aquaticgymenv_amd/csrc/aqua_evo.h), evolution strategies on a Q-network bank: it builds
and loads, exports what its header declares, has a build-table entry of its own behind the pinned ones, draws on a Philox
stream nobody else has, rejects bad arguments before touching a device and names the field; the host entries -- the noise, the
quantisation, the key and the optimiser step, the kernels' own code -- equal the numpy model the GPU tests compare against
(tests/_evo_model.py) bit for bit; the noise has the mean and variance it claims; the model obeys its exact identities and
every one of its mutants changes a result; and the compiler's resource metadata of the kernels shows no scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import _evo_model as M
from tests import _isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aquaticgymenv_amd", "csrc")
HEADER = os.path.join(CSRC, "aqua_evo.h")
FAKE = 0x100000           # a "device pointer" for calls that must fail (or return) before anything dereferences it
CFG = dict(sigma=0.05, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0)


@pytest.fixture(scope="module")
def capi():
    from aquaticgymenv_amd.build import build_library
    assert os.path.exists(build_library("evo"))
    from aquaticgymenv_amd import _evo_capi
    return _evo_capi


# ------------------------------------------------------------------------------------------------ the library and its table
def test_library_builds_loads_and_exports_its_header(capi):
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(aquaevo_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(capi.SYMBOLS) == {"aquaevo_version", "aquaevo_last_error", "aquaevo_noise", "aquaevo_quantise", "aquaevo_key",
                                            "aquaevo_step_param", "aquaevo_ask", "aquaevo_fitness", "aquaevo_tell"}, declared ^ set(capi.SYMBOLS)
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    assert capi.lib.aquaevo_version() == capi.ABI_VERSION == 1
    assert set(capi._SIGNATURES) == set(capi.SYMBOLS) - {"aquaevo_version", "aquaevo_last_error"}

    def define(name):
        return int(re.search(r"#define\s+%s\s+\(?(-?\d+)" % name, text).group(1))
    assert define("AQUAEVO_ABI_VERSION") == 1
    assert [define("AQUAEVO_E_" + n) for n in ("INVALID", "ALIGN", "NODEVICE")] == [-1, -2, -3] == [capi.E_INVALID, capi.E_ALIGN, capi.E_NODEVICE]
    from aquaticgymenv_amd import _learner_capi, _pbt_capi
    assert define("AQUAEVO_PARAMS") == capi.PARAMS == M.PARAMS == _learner_capi.PARAMS == 4739
    assert define("AQUAEVO_MAX_NETWORKS") == capi.MAX_NETWORKS == _pbt_capi.MAX_NETWORKS == 4096
    assert define("AQUAEVO_FIX_BITS") == capi.FIX_BITS == 20 and M.FIX == 2.0 ** 20
    assert define("AQUAEVO_CLAMP") == capi.CLAMP == M.CLAMP == 2048 and define("AQUAEVO_NOISE_OFFSET") == capi.NOISE_OFFSET == M.OFFSET == 8 * 65535
    assert define("AQUAEVO_MAX_BLOB") == capi.MAX_BLOB == _pbt_capi.MAX_BLOB and define("AQUAEVO_MAX_WORLDS") == capi.MAX_WORLDS == 2 ** 31 - 1
    assert define("AQUAEVO_BLOCK") == capi.BLOCK == 256 and define("AQUAEVO_MAX_BLOCKS") == capi.MAX_BLOCKS == 1024
    assert [define("AQUAEVO_MEAN_RETURN"), define("AQUAEVO_SUCCESS_RATE")] == [capi.MEAN_RETURN, capi.SUCCESS_RATE] == [M.MEAN_RETURN, M.SUCCESS_RATE] == [0, 1]
    assert [define("AQUAEVO_ADAM"), define("AQUAEVO_SGD")] == [capi.ADAM, capi.SGD] == [M.ADAM, M.SGD] == [0, 1]
    assert define("AQUAEVO_HEADER") == capi.HEADER == M.HEADER == 8 and define("AQUAEVO_ACC") == capi.ACC == 3
    assert [define("AQUAEVO_H_" + n) for n in ("GENERATION", "TELLS", "STEPPED", "BEST", "RANKED")] == [0, 1, 2, 3, 4] == \
        [capi.H_GENERATION, capi.H_TELLS, capi.H_STEPPED, capi.H_BEST, capi.H_RANKED]
    literal = re.search(r"#define\s+AQUAEVO_C\s+(\S+)", text).group(1)
    assert literal == "0x1.3988e1412ed76p-17" and float.fromhex(literal) == capi.C == M.C == 1.0 / (2.0 * np.sqrt(8.0 * (65536.0 ** 2 - 1.0) / 12.0))
    assert '"AQUA_EVO_LIB"' in open(os.path.join(ROOT, "aquaticgymenv_amd", "_evo_capi.py")).read()
    if shutil.which("nm"):
        nm = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True)
        assert nm.returncode == 0 and set(re.findall(r"\b(aquaevo_\w+)", nm.stdout)) == declared


def test_the_stream_is_nine_and_nobody_elses(capi):
    text = open(HEADER).read()
    assert int(re.search(r"#define\s+AQUAEVO_STREAM\s+(\d+)", text).group(1)) == capi.STREAM == M.STREAM == 9
    from aquaticgymenv_amd import (_bank_capi, _ens_capi, _episodes_capi, _fastpol_capi, _her_capi, _lbank_capi, _learner_capi, _pbt_capi,
                                   _policy_capi, _prio_capi, _replay_capi)
    taken = {m.__name__: m.STREAM for m in (_bank_capi, _ens_capi, _episodes_capi, _fastpol_capi, _her_capi, _lbank_capi, _learner_capi,
                                            _pbt_capi, _policy_capi, _prio_capi, _replay_capi)}
    assert set(taken.values()) == {5, 6, 7, 8}, taken
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
    assert named["AQUAEVO_STREAM"] == 9 and [k for k, v in named.items() if v == 9] == ["AQUAEVO_STREAM"], named
    assert [k for k, v in named.items() if v == 8] == ["AQUAHER_STREAM"]


def test_the_other_bindings_do_not_know_the_new_symbols(capi):
    from aquaticgymenv_amd import (_bank_capi, _capi, _ens_capi, _episodes_capi, _fastpol_capi, _her_capi, _lbank_capi, _learner_capi,
                                   _nstep_capi, _pbt_capi, _policy_capi, _prio_capi, _qmap_capi, _render_capi, _replay_capi, _segments_capi)
    others = (_capi, _policy_capi, _learner_capi, _episodes_capi, _render_capi, _replay_capi, _bank_capi, _lbank_capi, _segments_capi,
              _pbt_capi, _qmap_capi, _fastpol_capi, _nstep_capi, _prio_capi, _her_capi, _ens_capi)
    for other in others:
        assert not any(s.startswith("aquaevo_") for s in other.SYMBOLS)
        for name in capi.SYMBOLS:
            assert not hasattr(other.lib, name)


def test_build_table_entry_behind_the_pinned_tables():
    from aquaticgymenv_amd import build
    assert list(build.EVOLUTION_LIBRARIES) == ["evo"]
    assert build.sixteen_libraries() == ["hip", "policy", "learner", "episodes", "render", "replay", "bank", "lbank", "segments", "pbt", "qmap",
                                         "fastpol", "nstep", "prio", "her", "ens"]
    assert build.seventeen_libraries() == build.sixteen_libraries() + ["evo"] and len(build.seventeen_libraries()) == 17
    entry = build.library("evo")
    assert entry is build.EVOLUTION_LIBRARIES["evo"] and build.library("ens") is build.ENSEMBLE_LIBRARIES["ens"]
    src = os.path.join(CSRC, "aqua_evo.hip")
    lib = os.path.join(ROOT, "aquaticgymenv_amd", "lib", "libaqua_evo.so")
    headers = ["aqua_host.hpp"]
    assert entry["src"] == [src] and entry["lib"] == lib and entry["cuid"] == "aqua_evo"
    assert re.findall(r'#include "([a-z_]+\.hpp)"', open(src).read()) == headers and '#include "aqua_evo.h"' in open(src).read()
    assert entry["deps"] == [src] + [os.path.join(CSRC, h) for h in headers] + [HEADER] and all(os.path.exists(p) for p in entry["deps"])
    assert build.build_command("evo") == [
        build.hipcc_path(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-fno-honor-nans", "-cuid=aqua_evo",
        "-Wall", "-Wno-unused-function", "-o", lib + ".tmp", src]
    assert (build.EVO_SRC, build.EVO_DEPS, build.EVO_LIB, build.EVO_FLAGS) == (entry["src"], entry["deps"], entry["lib"], entry["flags"])
    assert callable(build.build_evo) and build.evo_needs_build() in (True, False)
    assert len({build.library(n)["lib"] for n in build.seventeen_libraries()}) == 17
    main = open(os.path.join(ROOT, "aquaticgymenv_amd", "build.py")).read().split('if __name__ == "__main__":')[1]
    assert "+ list(ENSEMBLE_LIBRARIES) + list(EVOLUTION_LIBRARIES)" in main
    for name in build.sixteen_libraries():
        assert not any("aqua_evo" in os.path.basename(d) for d in build.library(name)["deps"]), name
    # the header lies beside the source: neither include/ directory has a new file
    for folder in (os.path.join(ROOT, "include"), os.path.join(ROOT, "aquaticgymenv_amd", "include")):
        assert not any("evo" in name for name in os.listdir(folder))


def test_graft_entry_builds_and_checks_the_new_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    build_body = text.split("def build():")[1].split("def smoke():")[0]
    assert "seventeen_libraries()[16:]" in build_body and "_evo_capi" in build_body and "aquaevo_version" in build_body
    assert "sixteen_libraries()[15:]" in build_body
    import __graft_entry__ as entry
    from aquaticgymenv_amd import build
    assert entry.build() is None and os.path.exists(build.EVO_LIB)


def test_the_package_exports_the_class_lazily():
    import aquaticgymenv_amd
    from aquaticgymenv_amd.evolution import EvolutionStrategy
    assert aquaticgymenv_amd.EvolutionStrategy is EvolutionStrategy and "EvolutionStrategy" in aquaticgymenv_amd.__all__
    with pytest.raises(AttributeError):
        aquaticgymenv_amd.no_such_name
    for bad in (object(), None, 3, [1, 2]):
        with pytest.raises(ValueError, match="QNetworkBank"):
            EvolutionStrategy(bad)


# ------------------------------------------------------------------------------------------------ the C API without a device
ASK = ("theta", "perm", "header", "P", "sigma", "seed", "blob", "blob_floats")
FITNESS = ("log_ret", "log_code", "log_world", "C", "counts", "ret", "finished", "env_offset", "N", "seg", "P", "kind", "acc", "fitness", "episodes")
TELL = ("fitness", "P", "header", "theta", "m", "v", "t", "sigma", "seed", "lr", "beta1", "beta2", "eps", "weight_decay", "optimizer", "rank2",
        "weights", "grad_out")
MB = 0x100000             # every fake buffer has a megabyte of its own, or far more where it is large


def _ask(lib, **kw):
    a = dict(theta=FAKE, perm=FAKE + MB, header=FAKE + 2 * MB, P=6, sigma=0.05, seed=3, blob=FAKE + 0x10000000, blob_floats=4752)
    a.update(kw)
    return lib.aquaevo_ask(*[a[n] for n in ASK], None)


def _fitness(lib, **kw):
    a = dict(log_ret=FAKE, log_code=FAKE + MB, log_world=FAKE + 2 * MB, C=1000, counts=FAKE + 3 * MB, ret=FAKE + 4 * MB, finished=FAKE + 5 * MB,
             env_offset=0, N=1000, seg=100, P=10, kind=0, acc=FAKE + 6 * MB, fitness=FAKE + 7 * MB, episodes=FAKE + 8 * MB)
    a.update(kw)
    return lib.aquaevo_fitness(*[a[n] for n in FITNESS], None)


def _tell(lib, **kw):
    a = dict(fitness=FAKE, P=6, header=FAKE + MB, theta=FAKE + 2 * MB, m=FAKE + 3 * MB, v=FAKE + 4 * MB, t=FAKE + 5 * MB, sigma=0.05, seed=3,
             lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, optimizer=0, rank2=FAKE + 6 * MB, weights=FAKE + 7 * MB,
             grad_out=FAKE + 8 * MB)
    a.update(kw)
    return lib.aquaevo_tell(*[a[n] for n in TELL], None)


def test_argument_validation_without_touching_a_device(capi):
    """every call here fails before the first HIP call: nothing is launched, no pointer is dereferenced; the message names
    the offending field.  A call that passed every check would launch on the fake pointers: each probe below that is meant
    to PASS a size check carries a misaligned pointer and must come back with E_ALIGN, the last check of all."""
    lib = capi.lib
    nan, inf = float("nan"), float("inf")
    cases = [
        (_ask, "theta", dict(theta=None)), (_ask, "perm", dict(perm=None)), (_ask, "header", dict(header=None)), (_ask, "blob", dict(blob=None)),
        (_ask, "P", dict(P=0)), (_ask, "P", dict(P=-1)), (_ask, "P", dict(P=4097)), (_ask, "P", dict(P=2 ** 63 - 1)),
        (_ask, "sigma", dict(sigma=nan)), (_ask, "sigma", dict(sigma=inf)), (_ask, "sigma", dict(sigma=-0.01)), (_ask, "sigma", dict(sigma=-inf)),
        (_ask, "blob_floats", dict(blob_floats=4750)), (_ask, "blob_floats", dict(blob_floats=0)), (_ask, "blob_floats", dict(blob_floats=-4)),
        (_ask, "blob_floats", dict(blob_floats=2 ** 20 + 4)),
        (_ask, "overlap", dict(perm=FAKE + 4 * 4738)), (_ask, "overlap", dict(header=FAKE + 0x10000000 + 19008 * 5)),
        (_ask, "overlap", dict(blob=FAKE + 2 * MB - 19008 * 6 + 16)),
        (_fitness, "log_ret", dict(log_ret=None)), (_fitness, "log_code", dict(log_code=None)), (_fitness, "log_world", dict(log_world=None)),
        (_fitness, "counts", dict(counts=None)), (_fitness, "finished", dict(finished=None)), (_fitness, "ret", dict(ret=None)),
        (_fitness, "acc", dict(acc=None)), (_fitness, "fitness", dict(fitness=None)), (_fitness, "episodes", dict(episodes=None)),
        (_fitness, "C", dict(C=0)), (_fitness, "C", dict(C=2 ** 31)), (_fitness, "env_offset", dict(env_offset=-1)),
        (_fitness, "N", dict(N=-1)), (_fitness, "N", dict(N=2 ** 31)), (_fitness, "seg", dict(seg=0)), (_fitness, "seg", dict(seg=-3)),
        (_fitness, "seg", dict(seg=2 ** 31)), (_fitness, "P", dict(P=0)), (_fitness, "P", dict(P=4097)),
        (_fitness, "kind", dict(kind=2)), (_fitness, "kind", dict(kind=-1)),
        (_fitness, "overlap", dict(fitness=FAKE + 6 * MB + 8)), (_fitness, "overlap", dict(episodes=FAKE + 7 * MB + 36)),
        (_fitness, "overlap", dict(acc=FAKE + 4 * MB - 8)), (_fitness, "overlap", dict(fitness=FAKE + 3 * MB + 4)),
        (_tell, "fitness", dict(fitness=None)), (_tell, "header", dict(header=None)), (_tell, "theta", dict(theta=None)), (_tell, "m", dict(m=None)),
        (_tell, "v", dict(v=None)), (_tell, "t", dict(t=None)), (_tell, "rank2", dict(rank2=None)), (_tell, "weights", dict(weights=None)),
        (_tell, "P", dict(P=0)), (_tell, "P", dict(P=4097)), (_tell, "P", dict(P=-(2 ** 63))),
        (_tell, "sigma", dict(sigma=0.0)), (_tell, "sigma", dict(sigma=-0.0)), (_tell, "sigma", dict(sigma=nan)), (_tell, "sigma", dict(sigma=inf)),
        (_tell, "sigma", dict(sigma=-1.0)),
        (_tell, "lr", dict(lr=nan)), (_tell, "lr", dict(lr=-1e-3)), (_tell, "lr", dict(lr=inf)),
        (_tell, "beta1", dict(beta1=1.0)), (_tell, "beta1", dict(beta1=-0.1)), (_tell, "beta1", dict(beta1=nan)),
        (_tell, "beta2", dict(beta2=1.0)), (_tell, "beta2", dict(beta2=-0.1)), (_tell, "beta2", dict(beta2=nan)),
        (_tell, "eps", dict(eps=0.0)), (_tell, "eps", dict(eps=-1e-8)), (_tell, "eps", dict(eps=nan)), (_tell, "eps", dict(eps=inf)),
        (_tell, "weight_decay", dict(weight_decay=-0.1)), (_tell, "weight_decay", dict(weight_decay=nan)), (_tell, "weight_decay", dict(weight_decay=inf)),
        (_tell, "optimizer", dict(optimizer=2)), (_tell, "optimizer", dict(optimizer=-1)),
        (_tell, "overlap", dict(m=FAKE + 2 * MB + 4 * 4738)), (_tell, "overlap", dict(weights=FAKE + 6 * MB + 20)),
        (_tell, "overlap", dict(t=FAKE + MB + 56)), (_tell, "overlap", dict(grad_out=FAKE + 4 * MB - 8)),
    ]
    for call, field, kw in cases:
        assert call(lib, **kw) == capi.E_INVALID, (call.__name__, kw)
        assert re.search(r"\b%s\b" % field, capi.last_error()), (call.__name__, kw, capi.last_error())
    misaligned = [
        (_ask, "theta", dict(theta=FAKE + 2)), (_ask, "perm", dict(perm=FAKE + MB + 1)), (_ask, "header", dict(header=FAKE + 2 * MB + 4)),
        (_ask, "blob", dict(blob=FAKE + 0x10000000 + 8)),
        (_fitness, "log_ret", dict(log_ret=FAKE + 2)), (_fitness, "ret", dict(ret=FAKE + 4 * MB + 1)), (_fitness, "fitness", dict(fitness=FAKE + 7 * MB + 2)),
        (_fitness, "log_world", dict(log_world=FAKE + 2 * MB + 4)), (_fitness, "counts", dict(counts=FAKE + 3 * MB + 4)),
        (_fitness, "acc", dict(acc=FAKE + 6 * MB + 4)), (_fitness, "episodes", dict(episodes=FAKE + 8 * MB + 4)),
        (_tell, "fitness", dict(fitness=FAKE + 2)), (_tell, "theta", dict(theta=FAKE + 2 * MB + 1)), (_tell, "m", dict(m=FAKE + 3 * MB + 2)),
        (_tell, "v", dict(v=FAKE + 4 * MB + 3)), (_tell, "rank2", dict(rank2=FAKE + 6 * MB + 2)), (_tell, "weights", dict(weights=FAKE + 7 * MB + 1)),
        (_tell, "header", dict(header=FAKE + MB + 4)), (_tell, "t", dict(t=FAKE + 5 * MB + 4)), (_tell, "grad_out", dict(grad_out=FAKE + 8 * MB + 4)),
    ]
    for call, field, kw in misaligned:
        assert call(lib, **kw) == capi.E_ALIGN, (call.__name__, kw)
        assert re.search(r"\b%s\b" % field, capi.last_error()), (call.__name__, kw, capi.last_error())
    # the limits themselves pass the size checks (and then meet an alignment check)
    for kw in (dict(P=1), dict(P=4096), dict(sigma=0.0), dict(sigma=-0.0), dict(blob_floats=4), dict(blob_floats=2 ** 20), dict(seed=2 ** 64 - 1)):
        assert _ask(lib, header=FAKE + 2 * MB + 4, **kw) == capi.E_ALIGN, kw
    for kw in (dict(P=1), dict(P=4096, acc=FAKE + 16 * MB), dict(C=1), dict(C=2 ** 31 - 1, log_world=FAKE + 2 ** 36, log_ret=FAKE + 2 ** 37, log_code=FAKE + 2 ** 38),
               dict(N=0), dict(N=2 ** 31 - 1, ret=FAKE + 2 ** 36, finished=FAKE + 2 ** 37), dict(seg=1), dict(seg=2 ** 31 - 1), dict(kind=1),
               dict(ret=None, finished=None), dict(env_offset=2 ** 62)):
        assert _fitness(lib, counts=FAKE + 3 * MB + 4, **kw) == capi.E_ALIGN, kw
    for kw in (dict(P=1, rank2=None, weights=None), dict(P=1), dict(P=4096), dict(lr=0.0), dict(beta1=0.0, beta2=0.0), dict(weight_decay=3.0),
               dict(optimizer=1), dict(grad_out=None), dict(sigma=5e-324)):
        assert _tell(lib, t=FAKE + 5 * MB + 4, **kw) == capi.E_ALIGN, kw
    # the Python layer turns E_INVALID into ValueError and everything else into the binding's error
    with pytest.raises(ValueError, match="^aquaevo_tell: optimizer=2"):
        capi.check(_tell(lib, optimizer=2), "aquaevo_tell")
    with pytest.raises(capi.AquaEvoError):
        capi.check(_ask(lib, blob=FAKE + 0x10000000 + 8), "aquaevo_ask")
    # the host entry of the step validates as tell does
    io = (ctypes.c_float * 3)(1, 2, 3)
    good = dict(G=5, H=3, sigma=0.05, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, optimizer=0, t=1)
    order = ("G", "H", "sigma", "lr", "beta1", "beta2", "eps", "weight_decay", "optimizer", "t")
    for field, kw in (("H", dict(H=0)), ("H", dict(H=2049)), ("t", dict(t=0)), ("sigma", dict(sigma=0.0)), ("lr", dict(lr=nan)),
                      ("beta1", dict(beta1=1.0)), ("beta2", dict(beta2=1.5)), ("eps", dict(eps=0.0)), ("weight_decay", dict(weight_decay=-1.0)),
                      ("optimizer", dict(optimizer=7))):
        a = dict(good, **kw)
        assert lib.aquaevo_step_param(*[a[n] for n in order], ctypes.addressof(io), None) == capi.E_INVALID and re.search(r"\b%s\b" % field, capi.last_error())
    assert lib.aquaevo_step_param(*[good[n] for n in order], None, None) == capi.E_INVALID and list(io) == [1, 2, 3]


def test_argument_errors_of_the_class():
    import types
    import torch
    from aquaticgymenv_amd.evolution import EvolutionStrategy
    if not torch.cuda.is_available():
        from aquaticgymenv_amd.qbank import QNetworkBank
        from tests._qbank import family
        with pytest.raises(RuntimeError, match="no CPU path"):
            QNetworkBank([family(0)], 1, "cuda:0")
    es = types.SimpleNamespace()
    good = dict(sigma=0.05, lr=0.01, seed=0, optimizer="adam", betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, score="mean_return")
    EvolutionStrategy._configure(es, **good)
    assert es.betas == (0.9, 0.999) and es.seed == 0 and es.score == "mean_return"
    EvolutionStrategy._configure(es, **dict(good, seed=-1))
    assert es.seed == 2 ** 64 - 1
    for field, kw in (("sigma", dict(sigma=0.0)), ("sigma", dict(sigma=float("nan"))), ("lr", dict(lr=-1.0)), ("betas", dict(betas=(0.9,))),
                      ("betas", dict(betas=(1.0, 0.5))), ("eps", dict(eps=0.0)), ("weight_decay", dict(weight_decay=-1.0)),
                      ("optimizer", dict(optimizer="rmsprop")), ("score", dict(score="median"))):
        with pytest.raises(ValueError, match=field):
            EvolutionStrategy._configure(es, **dict(good, **kw))


# ------------------------------------------------------------------------------------------------ the host entries against the model
GRID_SEEDS = (0, 1, 0xDEADBEEFCAFEF00D, 2 ** 64 - 1, 0x8000000000000000)
GRID_G = (0, 1, 2 ** 32, 2 ** 32 + 5, 2 ** 48 - 1)


def test_noise_equals_the_model_on_a_grid(capi):
    js = np.array([0, 1, 2, 1023, 2046, 2047])
    iv = np.array([0, 1, 63, 64, 4096, 4737, 4738])
    for seed in GRID_SEEDS:
        for g in GRID_G:
            want = M.noise(seed, g, js[:, None], iv[None, :])
            got = np.array([[capi.noise(seed, g, int(j), int(i)) for i in iv] for j in js])
            assert np.array_equal(got, want), (seed, g)
            assert (np.abs(want) <= 524280).all() and (want % 2 == 0).all()
    # the generation enters with 48 bits, the pair and the parameter are not interchangeable
    assert capi.noise(5, 2 ** 48 + 7, 3, 4) == capi.noise(5, 7, 3, 4) and capi.noise(5, 2 ** 47 + 7, 3, 4) != capi.noise(5, 7, 3, 4)
    assert capi.noise(5, 7, 3, 4) != capi.noise(5, 7, 4, 3)
    rng = np.random.RandomState(11)
    for _ in range(200):
        seed, g, j, i = int(rng.randint(0, 2 ** 62)) * 3, int(rng.randint(0, 2 ** 47)), int(rng.randint(0, 2048)), int(rng.randint(0, 4739))
        assert capi.noise(seed, g, j, i) == int(M.noise(seed, g, j, i))


def test_noise_has_mean_zero_and_variance_one(capi):
    """2^21 noises of the MODEL (which the grid above ties to the library): both bounds are five standard errors of this
    distribution -- the mean's is 1 / sqrt(n), the sample variance's sqrt((kurtosis - 1) / n) = sqrt(1.85 / n) with the
    Irwin-Hall sum's excess kurtosis -0.15"""
    n = 2 ** 21
    j, i = np.divmod(np.arange(n), 4096)
    e = M.epsilon(M.noise(12345, 3, j, i))
    mean, var = float(e.mean()), float(e.var(ddof=1))
    print("noise: mean %.5f (bound %.5f)  variance %.5f (bound +-%.5f)" % (mean, 5 / np.sqrt(n), var, 5 * np.sqrt(1.85 / n)))
    assert abs(mean) < 5 / np.sqrt(n)
    assert abs(var - 1.0) < 5 * np.sqrt(1.85 / n)
    assert np.abs(e).max() < 4.9
    # a sample of the library's own draws of the same indices is the model's
    for k in range(0, n, n // 257):
        assert capi.noise(12345, 3, int(j[k]), int(i[k])) * capi.C == e[k]


def test_quantise_equals_the_model(capi):
    f32 = np.float32
    x = np.array([np.nan, -np.nan, np.inf, -np.inf, 2048.0, -2048.0, 2049.0, -2049.0, 1e30, -1e30, 0.0, -0.0, 1.0, -1.0, 1.5,
                  2.0 ** -21, -2.0 ** -21, 3 * 2.0 ** -21, -3 * 2.0 ** -21, 5 * 2.0 ** -21, 2.0 ** -22, 3 * 2.0 ** -22, 1e-45, 2047.9999], dtype=f32)
    want = M.quantise(x)
    got = np.array([capi.quantise(float(v)) for v in x])
    assert np.array_equal(got, want), (got, want)
    # NaN -> 0; +-inf and everything beyond -> +-2^31; exact ties to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2; -0.0 -> 0
    assert want[:4].tolist() == [0, 0, 2 ** 31, -2 ** 31] and want[4:10].tolist() == [2 ** 31, -2 ** 31] * 3
    assert want[15:20].tolist() == [0, 0, 2, -2, 2] and want[11] == 0 and want[14] == 3 * 2 ** 19
    rng = np.random.RandomState(2)
    x = (rng.randn(2000) * 10.0 ** rng.randint(-8, 5, 2000)).astype(f32)
    assert np.array_equal(np.array([capi.quantise(float(v)) for v in x]), M.quantise(x))


def test_key_equals_the_model_and_orders_every_bit_pattern(capi):
    u = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF,
                  0x3F800000, 0xBF800000, 0xFFC00001, 0x7F800001], dtype=np.uint32)
    want = M.key(u)
    assert np.array_equal(np.array([capi.key_of_bits(int(v)) for v in u], dtype=np.uint32), want)
    # negative NaNs < -inf < -1 < -0.0 < +0.0 < 1 < +inf < positive NaNs
    order = [0xFFFFFFFF, 0xFFC00001, 0xFFC00000, 0xFF800000, 0xBF800000, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x3F800000, 0x7F800000,
             0x7F800001, 0x7FC00000, 0x7FFFFFFF]
    keys = [int(M.key(np.uint32(v))) for v in order]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert capi.key(1.5) == int(M.key(M.bits([1.5])[0])) and capi.key(-0.0) == 0x7FFFFFFF and capi.key(0.0) == 0x80000000


def _step_both(capi, G, H, theta, m, v, t, optimizer, **cfg):
    c = dict(CFG, **cfg)
    got = capi.step_param(G, H, c["sigma"], c["lr"], c["beta1"], c["beta2"], c["eps"], c["weight_decay"], optimizer, t, theta, m, v)
    want = M.step(np.array([G]), H, [theta], [m], [v], t, c["sigma"], c["lr"], c["beta1"], c["beta2"], c["eps"], c["weight_decay"], optimizer)
    for k in range(3):
        assert M.bits([got[k]])[0] == M.bits(want[k])[0], (k, G, H, theta, m, v, t, optimizer, cfg, got, [w[0] for w in want[:3]])
    assert np.float64(got[3]).view(np.uint64) == np.float64(want[3][0]).view(np.uint64)
    return got


def test_step_param_equals_the_model(capi):
    rng = np.random.RandomState(7)
    f = lambda x: float(np.float32(x))            # noqa: E731
    for k in range(400):
        G = int(rng.randint(-2 ** 43, 2 ** 43))
        H = int(rng.choice([1, 2, 32, 65, 2048]))
        theta, m, v = f(rng.randn()), f(rng.randn() * 0.1), f(abs(rng.randn()) * 0.01)
        t = int(rng.choice([1, 2, 3, 1000, 10 ** 6, 2 ** 40 + 1]))
        cfg = dict(weight_decay=float(rng.choice([0.0, 0.01])), sigma=float(rng.choice([0.05, 1e-3, 2.0])), lr=float(rng.choice([0.01, 0.0, 1.0])))
        _step_both(capi, G, H, theta, m, v, t, k % 2, **cfg)
    for optimizer in (M.ADAM, M.SGD):
        for t in (1, 10 ** 6):
            _step_both(capi, 12345, 5, 0.25, 0.0, 0.0, t, optimizer)                       # v = 0
            _step_both(capi, 0, 5, 0.25, 0.125, 0.5, t, optimizer)                         # grad = 0
            _step_both(capi, 0, 5, -0.0, 0.0, 0.0, t, optimizer)                           # everything 0
            _step_both(capi, 0, 5, 0.25, 0.0, 0.0, t, optimizer, weight_decay=0.5)         # the decay alone
            _step_both(capi, -2 ** 43, 2048, 1e30, 1e-30, 1e30, t, optimizer, beta1=0.0, beta2=0.0)
    # grad = 0 and v = 0 with Adam: theta does not move (0 / (0 + eps)); SGD leaves m and v alone
    assert _step_both(capi, 0, 3, 0.75, 0.0, 0.0, 1, M.ADAM)[:3] == (0.75, 0.0, 0.0)
    assert _step_both(capi, 999, 3, 0.75, 0.5, 0.25, 4, M.SGD)[1:3] == (0.5, 0.25)


# ------------------------------------------------------------------------------------------------ the model's identities
def _tell_model(theta, fbits, P, g=0, mutant=None, optimizer=M.SGD, idx=None, **cfg):
    c = dict(CFG, **cfg)
    return M.tell(M.fresh(theta, g), fbits, P, 77, c["sigma"], c["lr"], c["beta1"], c["beta2"], c["eps"], c["weight_decay"], optimizer, idx=idx,
                  mutant=mutant)


def test_identities_of_the_model():
    theta = M.fixture_theta()
    # H = 1, fitness (1, 0): rank2 = (2, 0), weights = 2, D = 4 sigma, ghat_i = (2 n_i) (C / (4 sigma)) -- eps_i / (2 sigma) up
    # to that rounding chain
    out = _tell_model(theta, M.bits([1.0, 0.0]), 2)
    n = M.noise(77, 0, 0, np.arange(M.PARAMS))
    assert out["rank2"].tolist() == [2, 0] and out["weights"].tolist() == [2] and out["header"][3] == 0
    assert np.array_equal(out["ghat"], (2 * n).astype(np.float64) * (M.C / (4.0 * 0.05)))
    assert np.allclose(out["ghat"], M.epsilon(n) / (2 * 0.05), rtol=1e-15, atol=0)
    # swapping the fitness flips the sign of every ghat, bit for bit
    back = _tell_model(theta, M.bits([0.0, 1.0]), 2)
    assert back["weights"].tolist() == [-2] and back["header"][3] == 1
    assert np.array_equal((-back["ghat"]).view(np.uint64), out["ghat"].view(np.uint64))
    f = M.fixture_fitness(66, 1)
    a, b = _tell_model(theta, f, 66), _tell_model(theta, f.reshape(33, 2)[:, ::-1].reshape(-1).copy(), 66)
    assert np.array_equal(a["weights"], -b["weights"]) and np.array_equal((-b["ghat"]).view(np.uint64), a["ghat"].view(np.uint64))
    # all-equal fitness: G = 0 and theta is unchanged under SGD without decay; the mid-ranks are all 2H - 1
    for P in (2, 7, 64):
        same = _tell_model(theta, M.bits(np.full(P, 2.5)), P)
        assert not same["weights"].any() and not same["G"].any() and (same["rank2"] == 2 * (P // 2) - 1).all()
        assert np.array_equal(M.bits(same["theta"])[2:], M.bits(theta)[2:]) and same["theta"][0] == 0 and same["theta"][1] == 0
    # the doubled mid-ranks are a permutation's when nothing ties, sum to 2H (2H - 1) always, and the weights sum to what they must
    r, w, best = M.rank2(M.bits(np.arange(10, 0, -1)), 10)
    assert r.tolist() == list(range(18, -1, -2)) and w.tolist() == [2] * 5 and best == 0
    for seed in range(5):
        r, w, best = M.rank2(M.fixture_fitness(131, seed), 131)
        assert len(r) == 130 and r.sum() == 130 * 129 and (np.abs(w) <= 2 * 129).all()
    # P = 1: nothing but the bookkeeping
    one = _tell_model(theta, M.bits([3.0]), 1, g=9)
    assert np.array_equal(M.bits(one["theta"]), M.bits(theta)) and one["header"][:5] == [10, 1, 9, M.NO_SLOT, 0] and one["t"] == 1
    # the population: antithetic about the centre, the centre slot of an odd P is theta's bits, sigma = 0 gives the centre
    pop = M.ask(theta, 5, 0.05, 77, 3)
    mid = (pop[0].astype(np.float64) + pop[1].astype(np.float64)) / 2
    assert np.allclose(mid[4:], theta[4:], rtol=1e-6, atol=1e-9) and np.array_equal(M.bits(pop[4]), M.bits(theta))
    assert not np.array_equal(pop[0], pop[2]) and not np.array_equal(pop[0], M.ask(theta, 5, 0.05, 77, 4)[0])
    flat = M.ask(theta, 4, 0.0, 77, 3)
    assert (flat == theta).all()
    # computed, not copied: d = 0 * eps carries the sign of eps, and -0.0 + d keeps its sign in one member of the pair only
    assert M.noise(77, 3, 0, 1) != 0 and {int(M.bits(flat[0])[1]), int(M.bits(flat[1])[1])} == {0, 0x80000000}
    # the scatter: a perm entry out of range skips that parameter only
    perm = np.arange(M.PARAMS)[::-1] + 3
    bad = perm.copy()
    bad[17] = 4752
    before = np.full((5, 4752), 7.0, dtype=np.float32)
    blob, skipped = M.scatter(pop, perm, 4752, before), M.scatter(pop, bad, 4752, before)
    assert np.array_equal(M.bits(blob[:, perm]), M.bits(pop)) and (blob[:, :3] == 7).all() and (blob[:, 4742:] == 7).all()
    differ = np.nonzero((M.bits(blob) != M.bits(skipped)).any(axis=0))[0]
    assert differ.tolist() == [perm[17]] and (skipped[:, perm[17]] == 7).all()


def test_fitness_of_the_model_on_a_hand_made_log():
    log_ret = np.array([1.0, 3.0, -2.0, 5000.0, np.nan, 9.0], dtype=np.float32)
    log_code = np.array([3, 1, 3, 2, 3, 3], dtype=np.uint8)
    log_world = np.array([10, 11, 13, 12, 14, 99], dtype=np.int64)             # env_offset 10, seg 2: p = 0, 0, 1, 1, 2; 99 is foreign
    ret = np.array([0, 0, 0, 0, 0, 0.5, 7.0], dtype=np.float32)
    finished = np.array([1, 1, 1, 1, 1, 0, 0], dtype=np.uint8)                 # world 5 is open (p = 2); world 6 lies beyond N
    f, episodes, acc = M.fitness(log_ret, log_code, log_world, 6, ret, finished, 10, 6, 2, 4, M.MEAN_RETURN)
    assert episodes.tolist() == [2, 2, 2, 0] and acc[:, 2].tolist() == [1, 1, 1, 0]
    assert f.tolist() == M.bits([2.0, (2048.0 - 2.0) / 2, 0.25]).tolist() + [M.NEG_INF]
    f, _, _ = M.fitness(log_ret, log_code, log_world, 6, ret, finished, 10, 6, 2, 4, M.SUCCESS_RATE)
    assert f.tolist() == M.bits([0.5, 0.5, 0.5]).tolist() + [M.NEG_INF]
    # the cursor, not the capacity, bounds the records; a cursor beyond the capacity reads the whole log
    f, episodes, _ = M.fitness(log_ret, log_code, log_world, 2, None, None, 10, 6, 2, 4, M.MEAN_RETURN)
    assert episodes.tolist() == [2, 0, 0, 0] and f[0] == M.bits([2.0])[0]
    assert M.fitness(log_ret, log_code, log_world, 600, None, None, 10, 6, 2, 4, M.MEAN_RETURN)[1].tolist() == [2, 2, 1, 0]


# ------------------------------------------------------------------------------------------------ every mutant changes a result
def test_every_mutant_changes_a_result_on_the_fixtures():
    assert set(M.MUTANTS) >= {"odd_sign", "g_not_advanced", "swap_ji", "seven_halves", "ties_by_index", "no_4", "t_not_incremented",
                              "drop_unfinished", "empty_zero", "no_clamp", "rank_centre"}
    base = M.results(None)
    again = M.results(None)
    assert all(np.array_equal(base[k], again[k]) for k in base)
    for mutant in M.MUTANTS:
        got = M.results(mutant)
        changed = [k for k in base if not np.array_equal(base[k], got[k])]
        print(mutant, "changes", changed)
        assert changed, mutant
    with pytest.raises(AssertionError):
        M.noise(1, 2, 3, 4, mutant="no_such_mutant")


# ------------------------------------------------------------------------------------------------ the compiler's metadata
def test_codegen_has_no_scratch():
    """the resource metadata of the code object's notes: six kernels, none with a private segment or a spilled register; the
    ranking's LDS is the keys, the ranks and one word.  The register counts are printed for the record"""
    isa = _isa.kernels("evo")
    names = ("evo_ask_kernel", "evo_zero_kernel", "evo_accumulate_kernel", "evo_finish_kernel", "evo_rank_kernel", "evo_step_kernel")
    assert len(isa) == 6 and all(any(n in name for name in isa) for n in names), sorted(isa)
    for name, k in isa.items():
        m = k["meta"]
        print("registers:", name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert k["stats"]["ScratchSize"] == 0, (name, k["stats"])
        lds = 2 * 4 * 4096 + 8 if "evo_rank_kernel" in name else 0
        assert lds <= m["group_segment_fixed_size"] <= lds + 8, (name, m)
