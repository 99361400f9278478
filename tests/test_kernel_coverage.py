"""Coverage gate (CPU, no GPU needed): every kernel instantiation in the built library's gfx950 code object is launched by
at least one cell of the GPU matrix (tests/test_dispatch_matrix.py, predicted by the dispatch model tests/_dispatch.py),
or is listed below with the reason it is not; and every name the model predicts exists in the code object.  A kernel
instantiation added without a test cell fails here, by name.

The kernel names come from the code object itself: the .hip_fatbin section of libaqua_hip.so, unbundled for gfx950 with
clang-offload-bundler, its kernel descriptors (<name>.kd) listed by llvm-readelf --demangle.
"""
import ast
import os
import re
import shutil
import subprocess

import pytest

from tests import _dispatch as D

ROOT = D.ROOT
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"

# instantiations no cell of the matrix can reach, and why
UNREACHABLE = {
    "step_tables_ns_kernel<%d, %s>" % (ak, il): "the per-world next-step launch split by role: launch_step_tables selects it "
    "only in a build with -DAQUA_TABLES_ROLE_SPLIT (ns_sink takes every table that does not fit the registers)"
    for ak in sorted(D.KINDS.values()) for il in ("false", "true")
}

# the utility kernels the matrix does not launch, and the existing tests that do
UTILITY = {
    # (aqua_copy_async / aqua_copy_fanout_async: the done-mask exchange by peer copies, sharded.DoneMaskExchange(kind="ipc"))
    "copy_words_kernel<Word16>": "tests/test_00_bench_child.py::test_ipc_done_mask_exchange_between_two_processes_on_one_gpu",
    "copy_words_kernel<unsigned long long>": "tests/test_00_bench_child.py::test_ipc_done_mask_exchange_between_two_processes_on_one_gpu",
    "copy_fanout_kernel<Word16>": "tests/test_00_bench_child.py::test_ipc_done_mask_exchange_between_two_processes_on_one_gpu",
    "copy_fanout_kernel<unsigned long long>": "tests/test_00_bench_child.py::test_ipc_done_mask_exchange_between_two_processes_on_one_gpu",
    "ring_write_kernel<float>": "tests/test_hip_parity.py::test_replay_ring_records_the_transitions",
    "ring_write_kernel<unsigned char>": "tests/test_hip_parity.py::test_replay_ring_records_the_transitions",
    "obs_norm_kernel": "tests/test_hip_parity.py::test_normalised_observation_epilogue",
}


def _tool(name):
    for cand in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name), shutil.which(name)):
        if cand and os.path.exists(cand):
            return cand
    return None


def code_object_kernels(lib, workdir):
    """canonical names of the kernels (their .kd descriptors) in the gfx950 code object of `lib`"""
    objcopy, bundler, readelf = _tool("llvm-objcopy"), _tool("clang-offload-bundler"), _tool("llvm-readelf")
    fatbin, co = os.path.join(workdir, "fatbin.bin"), os.path.join(workdir, "gfx950.co")
    subprocess.check_call([objcopy, "--dump-section=.hip_fatbin=" + fatbin, lib, os.path.join(workdir, "host.o")])
    subprocess.check_call([bundler, "--unbundle", "--type=o", "--input=" + fatbin, "--targets=" + TARGET, "--output=" + co])
    out = subprocess.run([readelf, "--syms", "--demangle", co], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        m = re.search(r"\b(?:OBJECT|FUNC)\s+\w+\s+\w+\s+\w+\s+(.*\(\.kd\))\s*$", line)
        if m:
            names.add(D.canonical(m.group(1)))
    return names


@pytest.fixture(scope="module")
def shipped(tmp_path_factory):
    missing = [t for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf") if _tool(t) is None]
    if missing:
        pytest.skip("the ROCm LLVM tools %s are not installed: the code object's kernels cannot be listed" % missing)
    from aquaticgymenv_amd import build
    lib = build.build_hip()                 # (no-op when the library is current)
    names = code_object_kernels(lib, str(tmp_path_factory.mktemp("co")))
    assert names, "no kernel descriptors found in %s" % lib
    return names


def _matrix_prediction():
    from tests import test_dispatch_matrix as M
    reached = {}
    for cell in M.CELLS:
        for name in M.cell_kernels(cell):
            reached.setdefault(name, cell)
    return reached


def test_every_instantiation_has_a_cell_or_a_reason(shipped):
    for name, reason in UNREACHABLE.items():
        assert isinstance(reason, str) and reason.strip(), "UNREACHABLE[%r] needs a reason" % name
    reached = _matrix_prediction()
    untested = sorted(n for n in shipped if n not in reached and n not in UNREACHABLE and n not in UTILITY)
    assert not untested, "kernel instantiations with no test cell (add one to tests/test_dispatch_matrix.py, or list " \
                         "them in UNREACHABLE with the reason):\n  " + "\n  ".join(untested)
    both = sorted(n for n in UNREACHABLE if n in reached)
    assert not both, "listed as unreachable, but the matrix launches them: %s" % both


def test_every_predicted_name_exists(shipped):
    reached = _matrix_prediction()
    phantom = sorted("%s (cell %s)" % (n, tuple(reached[n])) for n in reached if n not in shipped)
    assert not phantom, "the dispatch model predicts kernels the code object does not hold:\n  " + "\n  ".join(phantom)
    stale = sorted(n for n in list(UNREACHABLE) + list(UTILITY) if n not in shipped)
    assert not stale, "listed kernels that the code object does not hold: %s" % stale


def test_utility_kernels_name_existing_tests():
    for name, ref in UTILITY.items():
        path, test = ref.split("::")
        with open(os.path.join(ROOT, path)) as f:
            tree = ast.parse(f.read())
        assert test in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}, "%s: %s does not exist" % (name, ref)


def test_model_reads_the_thresholds_from_the_sources():
    """the model's inputs are parsed, not copied: each threshold the launch rules use must be found"""
    for name in ("NS_TABLE_ROWS", "QUICK_MAX", "NS_INTERLEAVE_MIN", "DONE_WORD_WRITE_THROUGH_MAX_WORLDS",
                 "STORE_WB_SAME_STEP_MIN", "STORE_WB_NEXT_STEP_MIN", "STORE_WB_NEXT_STEP_MAX", "NS_LAUNCH_MAX_WORLDS",
                 "TABLES_KREG", "TABLES_KREG_WIDE", "TABLES_KREG_WIDE_MIN", "SINK_SPLIT_SHORT", "SINK_SPLIT_LONG",
                 "SINK_SPLIT_LONG_MIN_ROWS", "TABLES_NEXT_STEP_TILE", "FUSED_TABLE_ROWS_MAX", "AQUA_ACT_BEARING",
                 "AQUA_RESET_NEXT_STEP"):
        assert isinstance(D.THRESHOLDS.get(name), int), name
    c = D.THRESHOLDS
    assert c["NS_INTERLEAVE_MIN"] <= c["STORE_WB_NEXT_STEP_MIN"] <= c["STORE_WB_NEXT_STEP_MAX"]   # (wb implies interleave)
    assert D.read_thresholds([]) == {}


def test_model_classifies_the_edges():
    """K = 0 is a small table for step() but not for the fused rollout; the batch-size edges flip exactly at the threshold"""
    c = D.THRESHOLDS
    assert D.step_kernels("u8", 0, 0, 4099) == {"step_kernel<0, true, false, false>"}
    assert D.fused_kernels("u8", 0, 0) == {"rollout_kernel<0, false, 0>"}
    assert D.fused_kernels("i64", 2, c["QUICK_MAX"]) == {"rollout_kernel<2, true, 2>"}
    n = c["NS_INTERLEAVE_MIN"]
    assert D.step_kernels("u8", 2, 8, n - 1) != D.step_kernels("u8", 2, 8, n)
    n = c["STORE_WB_NEXT_STEP_MAX"]
    assert D.step_kernels("i64", 2, 8, n) == {"step_ns_kernel<2, true, true, true>"}
    assert D.step_kernels("i64", 2, 8, n + 1) == {"step_ns_kernel<2, true, true, false>"}
    assert D.step_tables_kernels("i32", 2, 9, 100) == {"step_tables_kernel<1, 3, 0, 2>"}
    assert D.step_tables_kernels("i32", 1, 11, 100) == {"step_tables_kernel<1, 1, 16, 2>"}
    assert D.step_tables_kernels("i32", 0, 11, 100) == {"step_tables_kernel<1, 0, 0, 2>"}
    assert D.fused_tables_kernels("u8", 1, 9) == {"rollout_tables16_kernel<0, 1>"}
    assert D.canonical("void (anonymous namespace)::step_kernel<0, true, false, false>((anonymous namespace)::NsArgs) (.kd)") \
        == "step_kernel<0, true, false, false>"
    assert D.canonical("(anonymous namespace)::tick_kernel(unsigned long*, unsigned long)") == "tick_kernel"
