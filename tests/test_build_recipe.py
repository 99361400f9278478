"""CPU-only checks of what the four HIP libraries share: the build table of aquaticgymenv_amd/build.py (command lines
pinned token by token, the old names bound from the table), the loader of the ctypes bindings, and the kernel bodies
tools/isa_listing.py hands to the codegen tests."""
import os
import re

import pytest

from tests import _isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aquaticgymenv_amd")
NAMES = ("hip", "policy", "learner", "episodes")


@pytest.mark.parametrize("name", NAMES)
def test_command_line_is_pinned(name):
    from aquaticgymenv_amd import build
    lib = os.path.join(PKG, "lib", "libaqua_%s.so" % name)
    assert build.build_command(name) == [
        build.hipcc_path(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-fno-honor-nans",
        "-cuid=aqua_" + name, "-Wall", "-Wno-unused-function", "-o", lib + ".tmp", os.path.join(PKG, "csrc", "aqua_%s.hip" % name)]
    assert build.build_command(name, ["-DX=1"])[10:12] == ["-DX=1", "-o"]      # extra flags: behind the warnings, before -o


def test_old_names_are_bound_from_the_table():
    from aquaticgymenv_amd import build
    assert list(build.LIBRARIES) == list(NAMES)                                # the build order
    t = build.LIBRARIES
    assert (build.SRC, build.DEPS, build.LIB) == (t["hip"]["src"], t["hip"]["deps"], t["hip"]["lib"])
    assert build.COMMON_FLAGS == t["hip"]["flags"]
    for name in NAMES[1:]:
        for key in ("src", "deps", "lib", "flags"):
            assert getattr(build, "%s_%s" % (name.upper(), key.upper())) == t[name][key], (name, key)
        assert getattr(build, name + "_needs_build")() == build.needs_build(name)
    assert build.needs_build() == build.needs_build("hip")
    for name in NAMES:
        assert t[name]["cuid"] == "aqua_" + name and t[name]["flags"].count("-cuid=aqua_" + name) == 1
        assert set(t[name]["src"]) <= set(t[name]["deps"]) and all(os.path.exists(d) for d in t[name]["deps"])
        fn = getattr(build, "build_" + name)
        assert callable(fn) and (build.needs_build(name) or fn() == t[name]["lib"])      # current: returns the path, compiles nothing
    assert len({t[n]["lib"] for n in NAMES}) == 4
    for a in NAMES:
        for b in NAMES:
            assert a == b or not set(t[a]["src"]) & set(t[b]["src"])


def test_shared_headers_are_dependencies_of_exactly_their_includers():
    from aquaticgymenv_amd import build
    for name in NAMES:
        text = open(build.LIBRARIES[name]["src"][0]).read()
        for header in ("aqua_host.hpp", "aqua_qnet.hpp"):
            included = re.search(r'^#include "%s"' % re.escape(header), text, re.M) is not None
            assert included == (os.path.join(PKG, "csrc", header) in build.LIBRARIES[name]["deps"]), (name, header)
            assert included == (name != "hip"), (name, header)


def _mnemonics(lines):
    return [ln.split()[0] for ln in lines if re.match(r"\s+[a-z]\w+", ln)]


@pytest.mark.parametrize("name", NAMES[1:])
def test_every_kernel_body_runs_to_the_end_of_its_function(name):
    """The body of a kernel is everything from its label to .Lfunc_end, so that the codegen tests see all of it: a body cut
    at the first s_endpgm has no s_endpgm in it, and of lrn_apply_kernel (two exits) it holds 138 of 788 instructions.
    The last instruction is the closing s_endpgm for 11 of the 12 kernels.  ep_scatter_kernel is laid out with five
    instructions of two basic blocks BEHIND its only s_endpgm (instruction 672 of 677); they end in an unconditional branch
    back, which is then the last line.  So: the body is, line for line, the function as a plain scan of the listing finds
    it, its exit is in it, and it ends in s_endpgm or, behind one, in s_branch."""
    ks = _isa.kernels(name)
    assert len(ks) == {"policy": 4, "learner": 5, "episodes": 3}[name], sorted(ks)
    text = _isa.listing(name).splitlines()
    for kernel, k in ks.items():
        begin = [i for i, ln in enumerate(text) if ln.startswith(kernel + ":")]
        assert len(begin) == 1, kernel
        end = next(i for i in range(begin[0], len(text)) if text[i].startswith(".Lfunc_end"))
        ins = _mnemonics(k["body"].splitlines())
        assert ins == _mnemonics(text[begin[0] + 1:end]), kernel
        assert "s_endpgm" in ins and ins.count("s_endpgm") == _mnemonics(text[begin[0] + 1:end]).count("s_endpgm"), kernel
        assert ins[-1] == "s_endpgm" or ins[-1] == "s_branch", (kernel, ins[-3:])


def test_loader_errors(tmp_path):
    from aquaticgymenv_amd import _episodes_capi as ecapi
    from aquaticgymenv_amd import _loader
    with pytest.raises(ImportError, match="libaqua_episodes.so is not built"):
        _loader.load("libaqua_episodes.so", str(tmp_path / "libaqua_episodes.so"), "aquaep", ecapi.ABI_VERSION, {})
    with pytest.raises(ImportError, match=r"libaqua_episodes.so ABI %d != binding %d: rebuild" % (ecapi.ABI_VERSION, ecapi.ABI_VERSION + 1)):
        _loader.load("libaqua_episodes.so", ecapi.LIB_PATH, "aquaep", ecapi.ABI_VERSION + 1, {})
    assert _loader.lib_path("AQUA_NO_SUCH_VARIABLE", "libaqua_episodes.so") == os.path.join(PKG, "lib", "libaqua_episodes.so")

    class Error(RuntimeError):
        pass
    check = _loader.checker(ecapi.lib, "aquaep", Error)
    assert check(0, "nothing") is None
    rc = ecapi.lib.aquaep_explore_u8(None, -1, 0, None, 0, 0, None, None)
    assert rc == ecapi.E_INVALID
    with pytest.raises(ValueError, match="^aquaep_explore_u8: N=-1"):
        check(rc, "aquaep_explore_u8")
    with pytest.raises(Error, match=r"^aquaep_explore_u8 failed \(code -2\): "):
        check(ecapi.E_ALIGN, "aquaep_explore_u8")
