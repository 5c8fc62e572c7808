"""Sampled planning as a build product (no GPU): the three symbols are declared, listed and exported, and the gfx950 code object of
rsx_plan_sampled.hip holds a sampled-lookahead kernel for every fused task in both physics forms — the variant set of
task_lookahead_kernel — plus the two elementwise kernels, with the register budget profiles/LABBOOK.md records."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

UNIT = "rsx_plan_sampled.hip"
# task ids of include/rsx.h that have kernels of their own (the crowded scrimmage shares the scrimmage's)
TASKS = {1: "VSS-v0", 2: "SSLStaticDefenders", 3: "SSLDribbling", 4: "SSLContestedPossession", 5: "SSLPassEndurance", 6: "scrimmage"}
KERNEL = re.compile(r"task_lookahead_sampled_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])E")
# the variants the two headline tasks step with, the wide lane groups (5v5: 16 lanes, 11v11: 32 lanes) and the fixed-team tasks
KEY_VARIANTS = ((0, 1, 8, 6), (1, 2, 8, 7), (0, 1, 16, 10), (1, 6, 32, 22), (1, 3, 8, 5), (1, 4, 8, 2), (1, 5, 8, 2))
SYMBOLS = ("rsx_task_lookahead_sampled", "rsx_plan_candidates", "rsx_plan_update")


def test_symbols_are_declared_listed_and_exported():
    from build_variant import dynamic_symbols
    from rsoccer_amd import _lib
    header = open(os.path.join(ROOT, "include", "rsx.h")).read()
    assert re.search(r"^typedef struct rsx_plan_sampler \{\s*uint64_t sample_seed;\s*float sigma;[^}]*int32_t hold;[^}]*\} rsx_plan_sampler;", header, re.M)
    assert re.search(r"^int rsx_task_lookahead_sampled\(rsx_sim\* h, const float\* mean_dev, const rsx_plan_sampler\* s, int n_candidates, int horizon, float gamma,", header, re.M)
    assert re.search(r"^int rsx_plan_candidates\(rsx_sim\* h, const float\* mean_dev, const rsx_plan_sampler\* s, int n_candidates, int horizon,", header, re.M)
    assert re.search(r"^int rsx_plan_update\(rsx_sim\* h, const float\* mean_dev, const rsx_plan_sampler\* s, int n_candidates, int horizon,", header, re.M)
    defined, _ = dynamic_symbols(_lib.LIB_PATH)
    for sym in SYMBOLS:
        assert sym in _lib.SYMBOLS and sym in defined, sym
    # the ctypes mirror of the struct has the header's layout: u64, f32, i32
    import ctypes as C
    assert [(n, t) for n, t in _lib.PlanSampler._fields_] == [("sample_seed", C.c_uint64), ("sigma", C.c_float), ("hold", C.c_int32)]
    assert C.sizeof(_lib.PlanSampler) == 16


def test_the_existing_lookahead_kernel_shares_the_loop_and_the_sampler_is_one_function():
    from __graft_entry__ import CSRC, HIP_UNITS
    assert UNIT in dict(HIP_UNITS)
    plan, sampled = (open(os.path.join(CSRC, f)).read() for f in ("rsx_plan.hip", UNIT))
    for text in (plan, sampled):
        assert text.count('#include "rsx_plan_body.inc"') == 1
    # every kernel that needs a candidate's action goes through the header's two functions
    common = open(os.path.join(CSRC, "rsx_plan_common.hpp")).read()
    assert common.count("void plan_noise4(") == 1 and common.count("float plan_action(") == 1
    assert sampled.count("plan_noise4(") >= 4 and sampled.count("plan_action(") >= 4 and "philox4x32" not in sampled


@pytest.fixture(scope="module")
def sampled_kernels():
    """({(kind, task, L, NR, phys): {remark: value}}, [other kernel names]) of rsx_plan_sampled.hip, compiled with the flags build()
    gives it — the compiler's kernel-resource-usage remarks, read the way tools/kernel_resources.py reads them"""
    from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS
    flags = dict(HIP_UNITS)[UNIT]
    work = tempfile.mkdtemp(prefix="rsx_plan_sampled_probe_")
    try:
        p = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_COMMON + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                           os.path.join(work, "unit.o"), os.path.join(CSRC, UNIT)], stderr=subprocess.PIPE, text=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows, others, cur = {}, {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = KERNEL.search(m.group(1))
            cur = (rows.setdefault(tuple(int(x) for x in k.groups()), {"name": m.group(1)}) if k
                   else others.setdefault(m.group(1), {"name": m.group(1)}))
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[.*?\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return rows, others


def test_code_object_holds_every_task_in_both_physics_forms(sampled_kernels):
    from rsoccer_amd import _lib
    rows, others = sampled_kernels
    assert rows, UNIT + " compiled to no task_lookahead_sampled_kernel"
    for task, name in TASKS.items():
        for phys in (0, 1):
            have = [k for k in rows if k[1] == task and k[4] == phys]
            assert have, f"no sampled lookahead kernel for {name} (physics form {phys})"
            assert all(k[0] == (0 if task == 1 else 1) for k in have)
    for key in KEY_VARIANTS:
        for phys in (0, 1):
            assert key + (phys,) in rows, key
    assert all(k[2] <= 32 for k in rows)   # MAX_L 32, as in rsx_plan.hip
    for kernel in ("plan_candidates_kernel", "plan_update_kernel"):
        assert sum(kernel in n for n in others) == 1, kernel
    # ... and the library build() linked carries each of them
    blob = open(_lib.LIB_PATH, "rb").read()
    for v in list(rows.values()) + list(others.values()):
        assert v["name"].encode() in blob, f"librsx_hip.so lacks {v['name']}"


def test_same_variant_set_as_the_loading_kernel():
    """rsx_plan.hip and rsx_plan_sampled.hip select their variants through the same table (rsx_variants.hpp) with the same MAX_L"""
    from __graft_entry__ import CSRC
    pat = re.compile(r"with_task_variant<task, nrs, fixed, (\d+)>\(L, NR,")
    widths = [pat.findall(open(os.path.join(CSRC, f)).read()) for f in ("rsx_plan.hip", UNIT)]
    assert widths == [["32"], ["32"]]


def test_headline_variants_use_no_scratch_memory(sampled_kernels):
    rows, others = sampled_kernels
    for key in ((0, 1, 8, 6, 0), (1, 2, 8, 7, 0)):   # VSS-v0 3v3 and SSLStaticDefenders 1v6, literal physics
        v = rows[key]
        print(key, {n: v.get(n) for n in ("VGPRs", "TotalSGPRs", "ScratchSize", "LDS Size", "Occupancy")})
        assert v["ScratchSize"] == 0, v
    for v in others.values():
        assert v["ScratchSize"] == 0, v


def test_labbook_records_every_variant(sampled_kernels):
    rows, _ = sampled_kernels
    text = open(os.path.join(ROOT, "profiles", "LABBOOK.md")).read()
    found = re.findall(r"^\| sampled `<(\d), (\d), (\d+), (\d+), (false|true)>` \|", text, re.M)
    recorded = {(int(a), int(b), int(c), int(d), 1 if e == "true" else 0) for a, b, c, d, e in found}
    assert recorded == set(rows), sorted(set(rows) ^ recorded)
    for kernel in ("plan_candidates_kernel", "plan_update_kernel"):
        assert re.search(r"^\| `" + kernel + r"` \|", text, re.M), kernel
