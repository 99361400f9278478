#!/usr/bin/env python3
"""What the compiler reports for the kernels of libaqua_episodes.so (no GPU needed): compiles
aquaticgymenv_amd/csrc/aqua_episodes.hip device-only with the library's flags and prints, per kernel, registers, scratch,
spills, LDS, occupancy and the static counts of ballots and atomics.  tests/test_episodes_cpu.py gates the same listing.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def listing():
    """-> the device assembly of aqua_episodes.hip as text"""
    from aquaticgymenv_amd import build
    flags = [f for f in build.EPISODES_FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "aqua_episodes.s")
        subprocess.check_call([build.hipcc_path(), *flags, "--cuda-device-only", "-S", "-o", out, *build.EPISODES_SRC],
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


def main():
    rows = {}
    for name, k in sorted(kernels(listing()).items()):
        rows[name] = dict(k["meta"], occupancy_waves_per_simd=k["stats"].get("Occupancy"),
                          ballots=len(re.findall(r"\bv_cmp\w*\s+s\[", k["body"])),
                          global_atomics=len(re.findall(r"\bglobal_atomic_\w+", k["body"])),
                          lds_atomics=len(re.findall(r"\bds_add_\w+", k["body"])),
                          instructions=len(re.findall(r"^\s+[a-z]\w+", k["body"], re.M)))
    print(json.dumps(rows, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
