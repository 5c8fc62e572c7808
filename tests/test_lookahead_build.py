"""rsx_task_lookahead as a build product (no GPU): the symbol is declared, listed and exported, and the gfx950 code object holds a
lookahead kernel for every fused task in both physics forms, with the register budget profiles/LABBOOK.md records."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# task ids of include/rsx.h that have kernels of their own (the crowded scrimmage shares the scrimmage's)
TASKS = {1: "VSS-v0", 2: "SSLStaticDefenders", 3: "SSLDribbling", 4: "SSLContestedPossession", 5: "SSLPassEndurance", 6: "scrimmage"}
KERNEL = re.compile(r"task_lookahead_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])E")


def test_symbol_is_declared_listed_and_exported():
    from build_variant import dynamic_symbols
    from rsoccer_amd import _lib
    header = open(os.path.join(ROOT, "include", "rsx.h")).read()
    assert re.search(r"^int rsx_task_lookahead\(rsx_sim\* h, const float\* actions_dev, int n_candidates, int horizon, float gamma,", header, re.M)
    assert "the handle is left exactly as it was" in header
    assert "rsx_task_lookahead" in _lib.SYMBOLS
    defined, _ = dynamic_symbols(_lib.LIB_PATH)
    assert "rsx_task_lookahead" in defined


@pytest.fixture(scope="module")
def plan_kernels():
    """{(kind, task, L, NR, phys): {remark: value}} of rsx_plan.hip, compiled with the flags build() gives it — the compiler's
    kernel-resource-usage remarks, read the way tools/kernel_resources.py reads them"""
    from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS
    flags = dict(HIP_UNITS)["rsx_plan.hip"]
    work = tempfile.mkdtemp(prefix="rsx_plan_probe_")
    try:
        p = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_COMMON + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                           os.path.join(work, "rsx_plan.o"), os.path.join(CSRC, "rsx_plan.hip")], stderr=subprocess.PIPE, text=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = KERNEL.search(m.group(1))
            cur = rows.setdefault(tuple(int(x) for x in k.groups()), {"name": m.group(1)}) if k else None
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[.*?\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return rows


def test_code_object_holds_every_task_in_both_physics_forms(plan_kernels):
    from rsoccer_amd import _lib
    assert plan_kernels, "rsx_plan.hip compiled to no task_lookahead_kernel"
    for task, name in TASKS.items():
        for phys in (0, 1):
            have = [k for k in plan_kernels if k[1] == task and k[4] == phys]
            assert have, f"no lookahead kernel for {name} (physics form {phys})"
            assert all(k[0] == (0 if task == 1 else 1) for k in have)
    # the variants the two headline tasks step with, and the wide lane groups (5v5: 16 lanes, 11v11: 32 lanes)
    for key in ((0, 1, 8, 6), (1, 2, 8, 7), (0, 1, 16, 10), (1, 6, 32, 22), (1, 3, 8, 5), (1, 4, 8, 2), (1, 5, 8, 2)):
        for phys in (0, 1):
            assert key + (phys,) in plan_kernels, key
    assert all(k[2] <= 32 for k in plan_kernels)   # MAX_L 32, as in the physics and sysid units
    # ... and the library build() linked carries each of them
    blob = open(_lib.LIB_PATH, "rb").read()
    for k, v in plan_kernels.items():
        assert v["name"].encode() in blob, f"librsx_hip.so lacks {v['name']}"


def test_headline_variants_use_no_scratch_memory(plan_kernels):
    for key in ((0, 1, 8, 6, 0), (1, 2, 8, 7, 0)):   # VSS-v0 3v3 and SSLStaticDefenders 1v6, literal physics
        v = plan_kernels[key]
        print(key, {n: v.get(n) for n in ("VGPRs", "TotalSGPRs", "ScratchSize", "LDS Size", "Occupancy")})
        assert v["ScratchSize"] == 0, v


def test_labbook_records_every_variant(plan_kernels):
    text = open(os.path.join(ROOT, "profiles", "LABBOOK.md")).read()
    rows = re.findall(r"^\| `<(\d), (\d), (\d+), (\d+), (false|true)>` \|", text, re.M)
    recorded = {(int(a), int(b), int(c), int(d), 1 if e == "true" else 0) for a, b, c, d, e in rows}
    assert recorded == set(plan_kernels), sorted(set(plan_kernels) ^ recorded)
