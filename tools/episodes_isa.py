#!/usr/bin/env python3
"""What the compiler reports for the kernels of libaqua_episodes.so (no GPU needed): compiles
aquaticgymenv_amd/csrc/aqua_episodes.hip device-only with the library's flags and prints, per kernel, registers, scratch,
spills, LDS, occupancy and the static counts of ballots and atomics.  tests/test_episodes_cpu.py gates the same listing.
"""
import json
import re

from isa_listing import kernels, listing


def main():
    rows = {}
    for name, k in sorted(kernels(listing("episodes")).items()):
        rows[name] = dict(k["meta"], occupancy_waves_per_simd=k["stats"].get("Occupancy"),
                          ballots=len(re.findall(r"\bv_cmp\w*\s+s\[", k["body"])),
                          global_atomics=len(re.findall(r"\bglobal_atomic_\w+", k["body"])),
                          lds_atomics=len(re.findall(r"\bds_add_\w+", k["body"])),
                          instructions=len(re.findall(r"^\s+[a-z]\w+", k["body"], re.M)))
    print(json.dumps(rows, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
