"""Development tools that produce committed evidence get a functional check of their own (CPU)."""
import csv
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernel_stats_by_grid_separates_batch_sizes_of_one_symbol(tmp_path):
    """tools/kernel_stats_by_grid.py: launches of ONE kernel symbol at two grid sizes (bench.py steps VSS-v0 at 4096 and at 65 536 envs
    with the same task_step_kernel<0,8,1,6,0>) end up in two rows with their own averages — rocprofv3's --stats table pools them"""
    trace = tmp_path / "x_kernel_trace.csv"
    name = "void rsx::task_step_kernel<0, 8, 1, 6, 0>(float*)"
    with open(trace, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Kind", "Kernel_Name", "Start_Timestamp", "End_Timestamp", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"])
        t = 1000
        for i in range(10):
            w.writerow(["KERNEL_DISPATCH", name, t, t + 9000 + i, 32768, 1, 1]); t += 20000
        for i in range(4):
            w.writerow(["KERNEL_DISPATCH", name, t, t + 25000, 524288, 1, 1]); t += 40000
        w.writerow(["KERNEL_DISPATCH", "other_kernel()", t, t + 500, 64, 1, 1])
    out = tmp_path / "by_grid.csv"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "kernel_stats_by_grid.py"), str(tmp_path), str(out)])
    rows = {(r["Name"], int(float(r["Grid_Size"]))): r for r in csv.DictReader(open(out))}
    assert len(rows) == 3
    small, big = rows[(name, 32768)], rows[(name, 524288)]
    assert int(float(small["Calls"])) == 10 and abs(float(small["AverageNs"]) - 9004.5) < 1e-6
    assert int(float(big["Calls"])) == 4 and float(big["AverageNs"]) == 25000.0
    assert float(small["MinNs"]) == 9000 and float(small["MaxNs"]) == 9009


def _tool_module(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return __import__(name)
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))


def test_variant_build_links_every_unit(monkeypatch, tmp_path):
    """tools/build_variant.py: the development builds (-DRSX_TIMING, A/B variants) compile __graft_entry__.HIP_UNITS, all of
    them — the library has no undefined rsx:: symbol (a unit left out of the link: -shared accepts that, the loader does not) and
    exports every name of the C-ABI"""
    if not shutil.which(os.environ.get("HIPCC", "hipcc")):
        pytest.skip("hipcc is not installed")
    bv = _tool_module("build_variant")
    monkeypatch.setattr(bv, "DEV", str(tmp_path))
    lib = bv.build("hip_timing", ["-DRSX_TIMING"])
    assert lib == str(tmp_path / "librsx_hip_timing.so") and os.path.exists(lib)
    defined, undefined = bv.dynamic_symbols(lib)
    assert not [s for s in undefined if "rsx" in s], "undefined symbols of the library's own namespace"
    assert any(s.startswith("_ZN3rsx") for s in defined), "the symbol listing does not see namespace rsx at all"
    from rsoccer_amd import _lib
    assert not [s for s in _lib.SYMBOLS if s not in defined]


def test_resource_table_compiles_the_units_of_the_build():
    """tools/kernel_resources.py has no unit list of its own: it compiles through build_variant.compile_units, which walks
    __graft_entry__.HIP_UNITS with HIPCC_COMMON (the full table takes a compile of every unit: not run here)"""
    import __graft_entry__ as g
    bv, kr = _tool_module("build_variant"), _tool_module("kernel_resources")
    assert bv.HIP_UNITS is g.HIP_UNITS and bv.HIPCC_COMMON is g.HIPCC_COMMON
    assert kr.compile_units is bv.compile_units
