"""The device assembly of one of the project's HIP libraries and its kernels, as the compiler reports them (no GPU
needed).  tools/make_policy_isa_budget.py, tools/learner_isa.py and tools/episodes_isa.py print it; tests/test_qpolicy_cpu.py,
tests/test_learner_cpu.py, tests/test_episodes_cpu.py, tests/test_replay_cpu.py, tests/test_qbank_cpu.py and
tests/test_lbank_cpu.py gate the same listing.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def listing(name):
    """-> the device assembly of library `name` of aquaticgymenv_amd.build (any of its tables) as text, compiled with the library's flags"""
    from aquaticgymenv_amd import build
    entry = build.library(name)
    flags = [f for f in entry["flags"] if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "aqua_%s.s" % name)
        subprocess.check_call([build.hipcc_path(), *flags, "--cuda-device-only", "-S", "-o", out, *entry["src"]],
                              stderr=subprocess.DEVNULL)
        return open(out).read()


def kernels(text):
    """-> {mangled name: {"body": str, "meta": {key: int}, "stats": {key: int}}} for every kernel of the code object; the
    body runs from the kernel's label to the end of the function (a kernel with early exits has several s_endpgm)"""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    out = {}
    for name in names:
        m = re.search(r"^%s:[^\n]*\n(.*?)\n\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S)
        out[name] = {"body": m.group(1), "meta": {}, "stats": {}}
        tail = text[m.start():]
        for key in ("NumVgprs", "NumAgprs", "TotalNumVgprs", "NumSgprs", "ScratchSize", "Occupancy", "LDSByteSize"):
            mm = re.search(r"^; %s: (\d+)" % key, tail, re.M)
            if mm:
                out[name]["stats"][key] = int(mm.group(1))
    # the code object's own metadata (what the loader reads)
    for block in re.split(r"\n  - \.agpr_count:", text)[1:]:
        mm = re.search(r"\.name:\s+(\S+)", block)
        if mm and mm.group(1) in out:
            block = ".agpr_count:" + block
            for key in ("agpr_count", "vgpr_count", "sgpr_count", "private_segment_fixed_size", "sgpr_spill_count",
                        "vgpr_spill_count", "group_segment_fixed_size"):
                m2 = re.search(r"\.%s:\s+(\d+)" % key, block)
                if m2:
                    out[mm.group(1)]["meta"][key] = int(m2.group(1))
    return out
