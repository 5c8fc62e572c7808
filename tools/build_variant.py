#!/usr/bin/env python3
"""Development build of librsx_hip.so with extra compiler flags -> tools/_dev/librsx_<name>.so:

    python tools/build_variant.py <name> [-DFOO=1 ...]
    python tools/build_variant.py hip_timing -DRSX_TIMING      (in-kernel time stamps: tools/exp_timeline2.py, exp_timeline_epl.py)
    python tools/build_variant.py qstats -DRSX_QSTATS          (contact-path counters: tools/exp_quad_stats.py)

The translation units and their flags are __graft_entry__.HIP_UNITS / HIPCC_COMMON, the list build() itself compiles: there is
no second copy here.  Select the result with RSX_LIB=tools/_dev/librsx_<name>.so (tools/ab_bench.py, bench.py, tests).  Fails
if the linked library is left with an undefined rsx:: symbol (-shared tolerates them; the loader does not)."""
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS  # noqa: E402

DEV = os.path.join(ROOT, "tools", "_dev")
HIPCC = os.environ.get("HIPCC", "hipcc")


def llvm_tool(name):
    """an LLVM binutil of the ROCm installation hipcc belongs to, or of the PATH"""
    hipcc = shutil.which(HIPCC)
    rocm = os.environ.get("ROCM_PATH") or (os.path.dirname(os.path.dirname(os.path.realpath(hipcc))) if hipcc else "")
    for d in (os.path.join(rocm, "lib", "llvm", "bin"), os.path.join(rocm, "llvm", "bin")):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return shutil.which(name)


def compile_units(extra, work, jobs=16):
    """every unit of HIP_UNITS with its own flags plus `extra`, at most `jobs` at a time -> [(unit, object file, compiler stderr)]"""
    def one(unit):
        src, flags = unit
        obj = os.path.join(work, os.path.splitext(src)[0] + ".o")
        p = subprocess.run([HIPCC] + HIPCC_COMMON + flags + list(extra) + ["-c", "-o", obj, os.path.join(CSRC, src)],
                           stderr=subprocess.PIPE, text=True)
        if p.returncode:
            sys.stderr.write(p.stderr)
            raise SystemExit(f"{src}: hipcc failed ({p.returncode})")
        return src, obj, p.stderr
    with ThreadPoolExecutor(min(jobs, 16, len(HIP_UNITS))) as pool:
        return list(pool.map(one, HIP_UNITS))


def dynamic_symbols(lib):
    """(defined, undefined) names of the library's dynamic symbol table (llvm-readelf --dyn-syms: what `llvm-nm -D` prints)"""
    out = subprocess.check_output([llvm_tool("llvm-readelf"), "--dyn-syms", "-W", lib], text=True)
    rows = [r for r in (line.split() for line in out.splitlines()) if len(r) == 8 and r[0].rstrip(":").isdigit()]
    return {r[7].split("@")[0] for r in rows if r[6] != "UND"}, {r[7].split("@")[0] for r in rows if r[6] == "UND"}


def undefined_rsx(lib):
    """undefined symbols of namespace rsx: what one unit calls and no unit of the link defines"""
    return sorted(s for s in dynamic_symbols(lib)[1] if s.startswith("_ZN3rsx"))


def build(name, extra):
    os.makedirs(DEV, exist_ok=True)
    out = os.path.join(DEV, f"librsx_{name}.so")
    work = tempfile.mkdtemp(prefix="rsx_variant_")
    try:
        compiled = compile_units(extra, work)
        sys.stderr.write("".join(log for _, _, log in compiled))   # the compiler's warnings
        objs = [obj for _, obj, _ in compiled]
        tmp = os.path.join(work, "lib.so")
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", tmp] + objs)
        missing = undefined_rsx(tmp)
        if missing:
            raise SystemExit(f"{out}: undefined rsx:: symbols (a unit is missing from the link): {missing}")
        shutil.move(tmp, out)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return out


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1].startswith("-"):
        raise SystemExit(__doc__)
    print("built", os.path.relpath(build(sys.argv[1], sys.argv[2:])))
