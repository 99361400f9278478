#!/usr/bin/env python3
"""What the compiler reports for the kernels of libaqua_learner.so (no GPU needed): compiles
aquaticgymenv_amd/csrc/aqua_learner.hip device-only with the library's flags and prints, per kernel, registers, scratch,
spills, LDS, occupancy and the static count of v_mfma_f32_32x32x2_f32.  tests/test_learner_cpu.py gates the same listing.
"""
import json
import re

from isa_listing import kernels, listing


def main():
    rows = {}
    for name, k in sorted(kernels(listing("learner")).items()):
        rows[name] = dict(k["meta"], occupancy_waves_per_simd=k["stats"].get("Occupancy"),
                          mfma_f32_32x32x2_f32=len(re.findall(r"\bv_mfma_f32_32x32x2_f32\b", k["body"])),
                          instructions=len(re.findall(r"^\s+[a-z]\w+", k["body"], re.M)))
    print(json.dumps(rows, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
