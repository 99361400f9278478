#!/usr/bin/env python3
"""Row "qfast" of profiles/isa_budget.json for the CURRENT source of the fast acting path (no GPU needed).

Compiles aquaticgymenv_amd/csrc/aqua_fastpol.hip device-only with the library's flags and records, per kernel, what the
compiler reports (VGPRs, AGPRs, SGPRs, scratch, spills, LDS, occupancy), the static count of v_mfma_f32_32x32x16_f16 (30
per tile of 32 worlds: 6 for the 64 x 5 layer, 24 for the 64 x 64 layer, fully unrolled) and, by tools/isa_budget.py's
classes, the vector-issue cycles of the whole kernel.  The record is keyed by one hash over every file of
build.FASTPOL_DEPS.  tests/test_fastpol_cpu.py gates the same listing; this script only writes the record.
"""
import json
import os
import re
import sys

from isa_budget import tally
from isa_listing import ROOT, kernels, listing
from make_policy_isa_budget import source_tag


def row():
    from aquaticgymenv_amd import build
    ks = kernels(listing("fastpol"))
    if not ks:
        sys.exit("no kernel in the listing")
    out = {"source_sha16": source_tag(build.FASTPOL_DEPS), "source": [os.path.relpath(d, ROOT) for d in build.FASTPOL_DEPS], "kernels": {}}
    for name, k in sorted(ks.items()):
        ops = re.findall(r"^\s+([a-z]\w+)", k["body"], re.M)
        t = tally([op for op in ops if not op.startswith("v_mfma")])          # the matrix pipe is counted apart
        out["kernels"][name] = dict(k["meta"], occupancy_waves_per_simd=k["stats"].get("Occupancy"),
                                    mfma_f32_32x32x16_f16=len(re.findall(r"\bv_mfma_f32_32x32x16_f16\b", k["body"])),
                                    mfma_f32_32x32x2_f32=len(re.findall(r"\bv_mfma_f32_32x32x2_f32\b", k["body"])),
                                    instructions=len(ops), valu=t.get("valu", 0), valu_issue_cycles=t["valu_issue_cycles"])
    return out


def main():
    record = row()
    path = os.path.join(ROOT, "profiles", "isa_budget.json")
    with open(path) as f:
        table = json.load(f)
    table["qfast"] = record
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
    print(json.dumps(record, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
