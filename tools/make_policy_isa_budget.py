#!/usr/bin/env python3
"""Row "qpolicy" of profiles/isa_budget.json for the CURRENT source of the Q-network kernel (no GPU needed).

Compiles aquaticgymenv_amd/csrc/aqua_policy.hip device-only with the library's flags and records, per qpolicy_kernel
instantiation, what the compiler reports (VGPRs, AGPRs, SGPRs, scratch, spills, LDS, occupancy) and the static count of
v_mfma_f32_32x32x2_f32 (70 per tile of 32 worlds: 6 for the 64 x 5 layer, 64 for the 64 x 64 layer, fully unrolled).
tests/test_qpolicy_cpu.py gates the same listing; this script only writes the record.
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def listing():
    """-> the device assembly of aqua_policy.hip as text"""
    from aquaticgymenv_amd import build
    flags = [f for f in build.POLICY_FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "aqua_policy.s")
        subprocess.check_call([build.hipcc_path(), *flags, "--cuda-device-only", "-S", "-o", out, *build.POLICY_SRC],
                              stderr=subprocess.DEVNULL)
        return open(out).read()


def kernels(text):
    """-> {mangled name: {"body": str, "meta": {key: int}, "stats": {key: int}}} for every qpolicy_kernel instantiation"""
    out = {}
    for m in re.finditer(r"^(_Z\w*qpolicy_kernel\w*):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.M | re.S):
        out[m.group(1)] = {"body": m.group(2), "meta": {}, "stats": {}}
    for name, k in out.items():
        tail = text[text.index("\n" + name + ":"):]
        for key in ("NumVgprs", "NumAgprs", "TotalNumVgprs", "NumSgprs", "ScratchSize", "Occupancy", "LDSByteSize"):
            mm = re.search(r"^; %s: (\d+)" % key, tail, re.M)
            if mm:
                k["stats"][key] = int(mm.group(1))
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


def main():
    from aquaticgymenv_amd import build
    ks = kernels(listing())
    if not ks:
        sys.exit("no qpolicy_kernel in the listing")
    with open(build.POLICY_SRC[0], "rb") as f:
        tag = hashlib.sha256(f.read()).hexdigest()[:16]
    row = {"source_sha16": tag, "source": "aquaticgymenv_amd/csrc/aqua_policy.hip", "kernels": {}}
    for name, k in sorted(ks.items()):
        row["kernels"][name] = dict(k["meta"], occupancy_waves_per_simd=k["stats"].get("Occupancy"),
                                    mfma_f32_32x32x2_f32=len(re.findall(r"\bv_mfma_f32_32x32x2_f32\b", k["body"])),
                                    instructions=len(re.findall(r"^\s+[a-z]\w+", k["body"], re.M)))
    path = os.path.join(ROOT, "profiles", "isa_budget.json")
    with open(path) as f:
        table = json.load(f)
    table["qpolicy"] = row
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
    print(json.dumps(row, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
