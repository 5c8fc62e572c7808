#!/usr/bin/env python3
"""Prints VGPR / SGPR / scratch / LDS / occupancy per kernel of librsx_hip.so (hipcc remarks), unit by unit, compiled as
__graft_entry__.HIP_UNITS says (tools/build_variant.py: compile_units).  Extra arguments are passed to the compiler."""
import re
import shutil
import sys
import tempfile

from build_variant import compile_units


def kernel_rows(extra=()):
    """[(unit, kernel, {remark name: value})] in the order the compiler reports them"""
    work = tempfile.mkdtemp(prefix="rsx_probe_")
    try:
        compiled = compile_units(["-Rpass-analysis=kernel-resource-usage"] + list(extra), work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    rows = []
    for unit, _, log in compiled:
        for line in log.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                rows.append((unit, m.group(1), {}))
                continue
            m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[.*?\])?: (\d+)", line)
            if m and rows:
                rows[-1][2][m.group(1).strip()] = m.group(2)
    return rows


if __name__ == "__main__":
    rows = kernel_rows(sys.argv[1:])
    print("%-14s %-70s %5s %5s %7s %6s %4s" % ("unit", "kernel", "VGPR", "SGPR", "scratch", "LDS", "occ"))
    for unit, k, v in rows:
        print("%-14s %-70s %5s %5s %7s %6s %4s" % (unit, k[:70], v.get("VGPRs"), v.get("TotalSGPRs"), v.get("ScratchSize"),
                                                   v.get("LDS Size"), v.get("Occupancy")))
    print(f"{len(rows)} kernels")
