#!/usr/bin/env python3
"""Row "qpolicy" of profiles/isa_budget.json for the CURRENT source of the Q-network kernel (no GPU needed).

Compiles aquaticgymenv_amd/csrc/aqua_policy.hip device-only with the library's flags and records, per qpolicy_kernel
instantiation, what the compiler reports (VGPRs, AGPRs, SGPRs, scratch, spills, LDS, occupancy) and the static count of
v_mfma_f32_32x32x2_f32 (70 per tile of 32 worlds: 6 for the 64 x 5 layer, 64 for the 64 x 64 layer, fully unrolled).
The kernel's body is in csrc/aqua_qnet.hpp, so the record is keyed by one hash over every file of build.POLICY_DEPS.
tests/test_qpolicy_cpu.py gates the same listing; this script only writes the record.
"""
import hashlib
import json
import os
import re
import sys

from isa_listing import ROOT, kernels, listing


def source_tag(deps):
    """one hash over the contents of every dependency, in table order"""
    h = hashlib.sha256()
    for d in deps:
        with open(d, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def main():
    from aquaticgymenv_amd import build
    ks = kernels(listing("policy"))
    if not ks:
        sys.exit("no qpolicy_kernel in the listing")
    row = {"source_sha16": source_tag(build.POLICY_DEPS), "source": [os.path.relpath(d, ROOT) for d in build.POLICY_DEPS], "kernels": {}}
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
