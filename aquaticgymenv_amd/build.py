"""Build libaqua_hip.so (hand-written HIP for gfx950) in-tree with hipcc.

The shared object lands in aquaticgymenv_amd/lib/ so that it travels with the source tree to the
GPU box (a JIT cache under $HOME would not).  hipcc cross-compiles for gfx950 without a GPU.
"""
import functools
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ARCH = "gfx950"
# -fno-honor-nans: no state ever holds a NaN; it drops the v_max(x, x) canonicalisation in front of every
# fmin/fmax (results for non-NaN inputs are unchanged; contraction is controlled per function by pragmas)
# -cuid=...: clang derives the compilation-unit id it bakes into the fat binary's symbols from the source's absolute path
# by default -- the same source built in another directory is then another file.  Fixed, the library's hash (the build
# tag of bench.py and profiles/traffic.json) depends on the sources and this command line only.
COMMON_FLAGS = ["-O3", "--offload-arch=" + ARCH, "-std=c++17", "-shared", "-fPIC", "-fno-honor-nans", "-cuid=aqua_hip"]


def _library(name, headers):
    """csrc/aqua_<name>.hip + include/aqua_<name>.h -> lib/libaqua_<name>.so, a translation unit and a library of its own:
    the common flags with its own compilation-unit id.  headers: what the source includes from csrc/."""
    src, cuid = [os.path.join(HERE, "csrc", "aqua_%s.hip" % name)], "aqua_" + name
    return {"src": src,
            "deps": src + [os.path.join(HERE, "csrc", h) for h in headers] + [os.path.join(os.path.dirname(HERE), "include", "aqua_%s.h" % name)],
            "lib": os.path.join(HERE, "lib", "libaqua_%s.so" % name),
            "cuid": cuid,
            "flags": [f for f in COMMON_FLAGS if not f.startswith("-cuid=")] + ["-cuid=" + cuid]}


# In build order.  hip: the environment (include/aqua_hip.h); its command line and hash depend on none of the others.
# policy: the Q-network kernel; learner: the DQN update; episodes: episode accounting and the exploration pass.
LIBRARIES = {
    "hip": _library("hip", ["aqua_device.hpp", "aqua_tuning.inc"]),
    "policy": _library("policy", ["aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp"]),
    "learner": _library("learner", ["aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp", "aqua_lrn.hpp"]),
    "episodes": _library("episodes", ["aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp"]),
}
# Libraries added since, in build order behind the four above (whose table, order and command lines are pinned).
# render: render(mode="rgb_array") frames and the thrust / ICC overlay (include/aqua_render.h).
EXTRA_LIBRARIES = {
    "render": _library("render", ["aqua_device.hpp", "aqua_host.hpp"]),
}
# Libraries behind those (both tables above and what all_libraries() returns are pinned too).
# replay: the experience ring with its cursor and size on the device (include/aqua_replay.h).
ADDON_LIBRARIES = {
    "replay": _library("replay", ["aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp"]),
}
# Libraries behind those (the three tables above and what every_library() returns are pinned as well).
# bank: a bank of Q-networks acting on one batch in one launch (include/aqua_bank.h).
BANK_LIBRARIES = {
    "bank": _library("bank", ["aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp"]),
}
# Libraries behind those (the four tables above and what each_library() returns are pinned as well).
# lbank: the learner bank, one DQN update of every network of a bank in two launches (include/aqua_lbank.h); its device
# code is the learner's, stated once in aqua_lrn.hpp.
POPULATION_LIBRARIES = {
    "lbank": _library("lbank", ["aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp", "aqua_lrn.hpp"]),
}


# Libraries behind those (the five tables above and what libraries() returns are pinned as well).
# segments: per-segment episode counters, epsilon schedules and windowed statistics from the episode log
# (include/aqua_segments.h).
SEGMENT_LIBRARIES = {
    "segments": _library("segments", ["aqua_host.hpp"]),
}


def _package_library(name, headers):
    """_library()'s entry with the header at aquaticgymenv_amd/include/aqua_<name>.h"""
    entry = _library(name, headers)
    entry["deps"] = entry["deps"][:-1] + [os.path.join(HERE, "include", "aqua_%s.h" % name)]
    return entry


# Libraries behind those (the six tables above and what nine_libraries() returns are pinned as well).
# pbt: selection among the networks of a population, population-based training (aquaticgymenv_amd/include/aqua_pbt.h).
# Its header lies in the package's own include/, not in the top-level one: the listing of that directory is pinned to the
# nine headers above (tests/test_segments_cpu.py), so a tenth header there would break a test that is to stay as it is.
SELECTION_LIBRARIES = {
    "pbt": _package_library("pbt", ["aqua_device.hpp", "aqua_host.hpp"]),
}


def _source_library(name, headers):
    """_library()'s entry with the header beside the source, at aquaticgymenv_amd/csrc/aqua_<name>.h"""
    entry = _library(name, headers)
    entry["deps"] = entry["deps"][:-1] + [os.path.join(HERE, "csrc", "aqua_%s.h" % name)]
    return entry


# Libraries behind those (the seven tables above and what ten_libraries() returns are pinned as well).
# qmap: Q-value maps of every network of a bank, the reference's Q-value plotter on the device (csrc/aqua_qmap.h).  Its
# header lies beside its source: the listings of both include/ directories are pinned (tests/test_segments_cpu.py,
# tests/test_pbt_cpu.py).
MAP_LIBRARIES = {
    "qmap": _source_library("qmap", ["aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp"]),
}


# Libraries behind those (the eight tables above and what eleven_libraries() returns are pinned as well).
# fastpol: the fast acting path, the Q-network's hidden layers on the f16 MFMA with operands split hi / lo
# (csrc/aqua_fastpol.h, beside its source as aqua_qmap.h is and for the same reason).
FAST_LIBRARIES = {
    "fastpol": _source_library("fastpol", ["aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp"]),
}


# Libraries behind those (the nine tables above and what twelve_libraries() returns are pinned as well).
# nstep: multi-step returns, the n-step fold of the experience ring and the bootstrap discount of every network
# (csrc/aqua_nstep.h, beside its source as aqua_qmap.h and aqua_fastpol.h are and for the same reason).
NSTEP_LIBRARIES = {
    "nstep": _source_library("nstep", ["aqua_host.hpp"]),
}


# Libraries behind those (the ten tables above and what thirteen_libraries() returns are pinned as well).
# prio: prioritised experience replay, a sum tree per network over the ring and the bank update with importance weights
# (csrc/aqua_prio.h, beside its source for the same reason); its update kernels are the learner's, stated once in aqua_lrn.hpp.
PRIORITY_LIBRARIES = {
    "prio": _source_library("prio", ["aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp", "aqua_lrn.hpp"]),
}


# Libraries behind those (the eleven tables above and what fourteen_libraries() returns are pinned as well).
# her: hindsight experience replay, the goals of a minibatch draw relabelled from the ring with the reward recomputed
# (csrc/aqua_her.h, beside its source for the same reason).
HINDSIGHT_LIBRARIES = {
    "her": _source_library("her", ["aqua_device.hpp", "aqua_host.hpp"]),
}


# Libraries behind those (the twelve tables above and what fifteen_libraries() returns are pinned as well).
# ens: the ensemble policy, every member network of a bank on every world of a batch reduced to one action per world
# (csrc/aqua_ens.h, beside its source for the same reason).
ENSEMBLE_LIBRARIES = {
    "ens": _source_library("ens", ["aqua_device.hpp", "aqua_host.hpp", "aqua_qnet.hpp"]),
}


# Libraries behind those (the thirteen tables above and what sixteen_libraries() returns are pinned as well).
# evo: natural evolution strategies on a bank, antithetic perturbations of one centre, mid-rank fitness shaping and the
# centre's optimiser step (csrc/aqua_evo.h, beside its source for the same reason).
EVOLUTION_LIBRARIES = {
    "evo": _source_library("evo", ["aqua_host.hpp"]),
}


def library(name):
    """the table entry of library `name`, from any of the twelve tables"""
    for table in (LIBRARIES, EXTRA_LIBRARIES, BANK_LIBRARIES, POPULATION_LIBRARIES, SEGMENT_LIBRARIES, SELECTION_LIBRARIES, MAP_LIBRARIES,
                  FAST_LIBRARIES, NSTEP_LIBRARIES, PRIORITY_LIBRARIES, HINDSIGHT_LIBRARIES, ENSEMBLE_LIBRARIES, EVOLUTION_LIBRARIES):
        if name in table:
            return table[name]
    return ADDON_LIBRARIES[name]


def all_libraries():
    """every library's name, in build order"""
    return list(LIBRARIES) + list(EXTRA_LIBRARIES)


def every_library():
    """every library's name up to the add-ons, in build order"""
    return all_libraries() + list(ADDON_LIBRARIES)


def each_library():
    """every library's name up to BANK_LIBRARIES, in build order"""
    return every_library() + list(BANK_LIBRARIES)


def libraries():
    """the eight libraries' names up to POPULATION_LIBRARIES, in build order"""
    return each_library() + list(POPULATION_LIBRARIES)


def nine_libraries():
    """all nine libraries' names, those of SEGMENT_LIBRARIES included, in build order (what build() and `python -m` compile)"""
    return libraries() + list(SEGMENT_LIBRARIES)


def ten_libraries():
    """all ten libraries' names, the one of SELECTION_LIBRARIES included, in build order"""
    return nine_libraries() + list(SELECTION_LIBRARIES)


def eleven_libraries():
    """all eleven libraries' names, the one of MAP_LIBRARIES included, in build order"""
    return ten_libraries() + list(MAP_LIBRARIES)


def twelve_libraries():
    """all twelve libraries' names, the one of FAST_LIBRARIES included, in build order (what build() and `python -m` compile)"""
    return eleven_libraries() + list(FAST_LIBRARIES)


def thirteen_libraries():
    """all thirteen libraries' names, the one of NSTEP_LIBRARIES included, in build order (what build() and `python -m` compile)"""
    return twelve_libraries() + list(NSTEP_LIBRARIES)


def fourteen_libraries():
    """all fourteen libraries' names, the one of PRIORITY_LIBRARIES included, in build order"""
    return thirteen_libraries() + list(PRIORITY_LIBRARIES)


def fifteen_libraries():
    """all fifteen libraries' names, the one of HINDSIGHT_LIBRARIES included, in build order (what build() and `python -m` compile)"""
    return fourteen_libraries() + list(HINDSIGHT_LIBRARIES)


def sixteen_libraries():
    """all sixteen libraries' names, the one of ENSEMBLE_LIBRARIES included, in build order (what build() and `python -m` compile)"""
    return fifteen_libraries() + list(ENSEMBLE_LIBRARIES)


def seventeen_libraries():
    """all seventeen libraries' names, the one of EVOLUTION_LIBRARIES included, in build order (what build() and `python -m` compile)"""
    return sixteen_libraries() + list(EVOLUTION_LIBRARIES)


def hipcc_path():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm)")


def needs_build(name="hip"):
    entry = library(name)
    if not os.path.exists(entry["lib"]):
        return True
    t = os.path.getmtime(entry["lib"])
    return any(os.path.getmtime(d) > t for d in entry["deps"])


def build_command(name, extra_flags=()):
    """the hipcc command line of build_library(name), without running it"""
    entry = library(name)
    return [hipcc_path(), *entry["flags"], "-Wall", "-Wno-unused-function", *extra_flags, "-o", entry["lib"] + ".tmp", *entry["src"]]


def build_library(name, force=False, verbose=False, extra_flags=()):
    """Compile the library's source -> lib/libaqua_<name>.so for gfx950.  Returns the library path."""
    lib = library(name)["lib"]
    if not force and not needs_build(name):
        return lib
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    cmd = build_command(name, extra_flags)
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    os.replace(lib + ".tmp", lib)
    return lib


# the names that tests, tools and __graft_entry__ use, bound from the table
SRC, DEPS, LIB = (LIBRARIES["hip"][k] for k in ("src", "deps", "lib"))
POLICY_SRC, POLICY_DEPS, POLICY_LIB, POLICY_FLAGS = (LIBRARIES["policy"][k] for k in ("src", "deps", "lib", "flags"))
LEARNER_SRC, LEARNER_DEPS, LEARNER_LIB, LEARNER_FLAGS = (LIBRARIES["learner"][k] for k in ("src", "deps", "lib", "flags"))
EPISODES_SRC, EPISODES_DEPS, EPISODES_LIB, EPISODES_FLAGS = (LIBRARIES["episodes"][k] for k in ("src", "deps", "lib", "flags"))
build_hip, build_policy, build_learner, build_episodes = (functools.partial(build_library, n) for n in LIBRARIES)
policy_needs_build, learner_needs_build, episodes_needs_build = (functools.partial(needs_build, n) for n in ("policy", "learner", "episodes"))
RENDER_SRC, RENDER_DEPS, RENDER_LIB, RENDER_FLAGS = (EXTRA_LIBRARIES["render"][k] for k in ("src", "deps", "lib", "flags"))
build_render, render_needs_build = functools.partial(build_library, "render"), functools.partial(needs_build, "render")
REPLAY_SRC, REPLAY_DEPS, REPLAY_LIB, REPLAY_FLAGS = (ADDON_LIBRARIES["replay"][k] for k in ("src", "deps", "lib", "flags"))
build_replay, replay_needs_build = functools.partial(build_library, "replay"), functools.partial(needs_build, "replay")
BANK_SRC, BANK_DEPS, BANK_LIB, BANK_FLAGS = (BANK_LIBRARIES["bank"][k] for k in ("src", "deps", "lib", "flags"))
build_bank, bank_needs_build = functools.partial(build_library, "bank"), functools.partial(needs_build, "bank")
LBANK_SRC, LBANK_DEPS, LBANK_LIB, LBANK_FLAGS = (POPULATION_LIBRARIES["lbank"][k] for k in ("src", "deps", "lib", "flags"))
build_lbank, lbank_needs_build = functools.partial(build_library, "lbank"), functools.partial(needs_build, "lbank")
SEGMENTS_SRC, SEGMENTS_DEPS, SEGMENTS_LIB, SEGMENTS_FLAGS = (SEGMENT_LIBRARIES["segments"][k] for k in ("src", "deps", "lib", "flags"))
build_segments, segments_needs_build = functools.partial(build_library, "segments"), functools.partial(needs_build, "segments")
PBT_SRC, PBT_DEPS, PBT_LIB, PBT_FLAGS = (SELECTION_LIBRARIES["pbt"][k] for k in ("src", "deps", "lib", "flags"))
build_pbt, pbt_needs_build = functools.partial(build_library, "pbt"), functools.partial(needs_build, "pbt")
QMAP_SRC, QMAP_DEPS, QMAP_LIB, QMAP_FLAGS = (MAP_LIBRARIES["qmap"][k] for k in ("src", "deps", "lib", "flags"))
build_qmap, qmap_needs_build = functools.partial(build_library, "qmap"), functools.partial(needs_build, "qmap")
FASTPOL_SRC, FASTPOL_DEPS, FASTPOL_LIB, FASTPOL_FLAGS = (FAST_LIBRARIES["fastpol"][k] for k in ("src", "deps", "lib", "flags"))
build_fastpol, fastpol_needs_build = functools.partial(build_library, "fastpol"), functools.partial(needs_build, "fastpol")
NSTEP_SRC, NSTEP_DEPS, NSTEP_LIB, NSTEP_FLAGS = (NSTEP_LIBRARIES["nstep"][k] for k in ("src", "deps", "lib", "flags"))
build_nstep, nstep_needs_build = functools.partial(build_library, "nstep"), functools.partial(needs_build, "nstep")
PRIO_SRC, PRIO_DEPS, PRIO_LIB, PRIO_FLAGS = (PRIORITY_LIBRARIES["prio"][k] for k in ("src", "deps", "lib", "flags"))
build_prio, prio_needs_build = functools.partial(build_library, "prio"), functools.partial(needs_build, "prio")
HER_SRC, HER_DEPS, HER_LIB, HER_FLAGS = (HINDSIGHT_LIBRARIES["her"][k] for k in ("src", "deps", "lib", "flags"))
build_her, her_needs_build = functools.partial(build_library, "her"), functools.partial(needs_build, "her")
ENS_SRC, ENS_DEPS, ENS_LIB, ENS_FLAGS = (ENSEMBLE_LIBRARIES["ens"][k] for k in ("src", "deps", "lib", "flags"))
build_ens, ens_needs_build = functools.partial(build_library, "ens"), functools.partial(needs_build, "ens")
EVO_SRC, EVO_DEPS, EVO_LIB, EVO_FLAGS = (EVOLUTION_LIBRARIES["evo"][k] for k in ("src", "deps", "lib", "flags"))
build_evo, evo_needs_build = functools.partial(build_library, "evo"), functools.partial(needs_build, "evo")


def build_variant(name, flags, verbose=False):
    """Tuning builds for A/B timing (tools/ablate.py): lib/variants/libaqua_hip_<name>.so with extra -D flags.
    Select one at run time with AQUA_HIP_LIB=<path>."""
    out = os.path.join(HERE, "lib", "variants", "libaqua_hip_%s.so" % name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [hipcc_path(), *COMMON_FLAGS, *flags, "-o", out, *SRC]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


class NoSanitizerRuntime(RuntimeError):
    pass


def build_hostsan(verbose=False):
    """lib/variants/libaqua_hip_hostsan.so: the HOST half of the library (argument validation, the blob / table packers,
    graph / event / IPC handle bookkeeping) instrumented with AddressSanitizer + UBSan; device code untouched
    (-fno-gpu-sanitize: no instrumented kernels, no xnack code objects -- GPU ASan does not exist on this pool and is never
    asked for).  CPU box only: tests/test_sanitizers.py runs tests/test_capi_cpu.py against it in a child process with the
    runtime preloaded.  -> (library path, path of clang's shared ASan runtime to preload)."""
    cc = hipcc_path()
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(cc))), "lib", "llvm", "bin", "clang")
    if not os.path.exists(clang):
        clang = shutil.which("amdclang") or shutil.which("clang") or ""
    runtime = ""
    if clang:
        runtime = subprocess.run([clang, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
        if not os.path.isabs(runtime):           # newer layouts: lib/<triple>/libclang_rt.asan.so
            runtime = subprocess.run([clang, "-print-file-name=libclang_rt.asan.so"], capture_output=True, text=True).stdout.strip()
    if not runtime or not os.path.isabs(runtime) or not os.path.exists(runtime):
        raise NoSanitizerRuntime("hipcc's clang has no shared AddressSanitizer runtime (looked for libclang_rt.asan-x86_64.so)")
    out = os.path.join(HERE, "lib", "variants", "libaqua_hip_hostsan.so")
    if os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in DEPS + [os.path.abspath(__file__)]):
        return out, runtime
    # -DAQUA_DEV_U8_ONLY: the device side is compiled for one action kind instead of seven (a sixth of the compile time);
    # the host code under test -- validation, packers, handles -- is the same, only the launch tables are shorter
    flags = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
             "-fno-gpu-sanitize", "-shared-libsan", "-DAQUA_DEV_U8_ONLY"]
    return build_variant("hostsan", flags, verbose=verbose), runtime


if __name__ == "__main__":
    if "--variants" in sys.argv:
        for name, flags in (("stamps", ["-DAQUA_STAMPS=1"]), ("nw", ["-DAQUA_NS_NOWORK"]), ("nm", ["-DAQUA_NS_NOMAIN"])):
            print(build_variant(name, flags, verbose=True))
    for name in nine_libraries() + list(SELECTION_LIBRARIES) + list(MAP_LIBRARIES) + list(FAST_LIBRARIES) + list(NSTEP_LIBRARIES) + list(PRIORITY_LIBRARIES) \
            + list(HINDSIGHT_LIBRARIES) + list(ENSEMBLE_LIBRARIES) + list(EVOLUTION_LIBRARIES):
        print(build_library(name, force="--force" in sys.argv, verbose=True))
