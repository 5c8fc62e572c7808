"""rsx_task_lookahead_policy as a build product (no GPU): the symbols are declared, listed and exported, and the gfx950 code object
holds a policy-lookahead kernel for every single-agent fused task in both physics forms, with the register budget
profiles/LABBOOK.md records."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# task ids of include/rsx.h the call serves (the scrimmage commands every robot: refused)
TASKS = {1: "VSS-v0", 2: "SSLStaticDefenders", 3: "SSLDribbling", 4: "SSLContestedPossession", 5: "SSLPassEndurance"}
KERNEL = re.compile(r"task_lookahead_policy_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])E")


def test_symbols_are_declared_listed_and_exported():
    from build_variant import dynamic_symbols
    from rsoccer_amd import _lib
    header = open(os.path.join(ROOT, "include", "rsx.h")).read()
    assert re.search(r"^int rsx_policy_num_params\(const rsx_sim\* h, const rsx_policy_mlp\* p, int64_t\* out\);", header, re.M)
    assert re.search(r"^int rsx_task_lookahead_policy\(rsx_sim\* h, const rsx_policy_mlp\* p, const float\* params_dev, int n_policies, "
                     r"int horizon, float gamma,", header, re.M)
    body = re.search(r"typedef struct rsx_policy_mlp \{(.*?)\} rsx_policy_mlp;", header, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in _lib.PolicyMLP._fields_]
    for name, value in (("RELU", _lib.ACT_RELU), ("TANH", _lib.ACT_TANH), ("CLIP", _lib.ACT_CLIP)):
        assert re.search(r"^#define RSX_ACT_%s %d\b" % (name, value), header, re.M), name
    assert "scrimmage task: it commands every robot" in header
    defined, _ = dynamic_symbols(_lib.LIB_PATH)
    for sym in ("rsx_policy_num_params", "rsx_task_lookahead_policy"):
        assert sym in _lib.SYMBOLS and sym in defined, sym


@pytest.fixture(scope="module")
def policy_kernels():
    """{(kind, task, L, NR, phys): {remark: value}} of rsx_policy.hip, compiled with the flags build() gives it — the compiler's
    kernel-resource-usage remarks, read the way tools/kernel_resources.py reads them"""
    from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS
    units = dict(HIP_UNITS)
    assert units["rsx_policy.hip"] == units["rsx_plan.hip"]
    work = tempfile.mkdtemp(prefix="rsx_policy_probe_")
    try:
        p = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_COMMON + units["rsx_policy.hip"] +
                           ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(work, "rsx_policy.o"),
                            os.path.join(CSRC, "rsx_policy.hip")], stderr=subprocess.PIPE, text=True)
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


def test_code_object_holds_every_task_in_both_physics_forms(policy_kernels):
    from rsoccer_amd import _lib
    assert policy_kernels, "rsx_policy.hip compiled to no task_lookahead_policy_kernel"
    for task, name in TASKS.items():
        for phys in (0, 1):
            have = [k for k in policy_kernels if k[1] == task and k[4] == phys]
            assert have, f"no policy-lookahead kernel for {name} (physics form {phys})"
            assert all(k[0] == (0 if task == 1 else 1) for k in have)
    assert not [k for k in policy_kernels if k[1] not in TASKS], "a kernel for a task the call refuses"
    for key in ((0, 1, 8, 6), (1, 2, 8, 7), (0, 1, 16, 10), (0, 1, 16, 6), (1, 3, 8, 5), (1, 4, 8, 2), (1, 5, 8, 2)):
        for phys in (0, 1):
            assert key + (phys,) in policy_kernels, key
    assert all(k[2] <= 32 for k in policy_kernels)   # MAX_L 32, as in the lookahead units
    blob = open(_lib.LIB_PATH, "rb").read()
    for k, v in policy_kernels.items():
        assert v["name"].encode() in blob, f"librsx_hip.so lacks {v['name']}"


def test_headline_variants_use_no_scratch_memory(policy_kernels):
    for key in ((0, 1, 8, 6, 0), (1, 2, 8, 7, 0)):   # VSS-v0 3v3 and SSLStaticDefenders 1v6, literal physics
        v = policy_kernels[key]
        print(key, {n: v.get(n) for n in ("VGPRs", "TotalSGPRs", "ScratchSize", "LDS Size", "Occupancy")})
        assert v["ScratchSize"] == 0, v


def test_labbook_records_every_variant(policy_kernels):
    text = open(os.path.join(ROOT, "profiles", "LABBOOK.md")).read()
    rows = re.findall(r"^\| policy `<(\d), (\d), (\d+), (\d+), (false|true)>` \|", text, re.M)
    recorded = {(int(a), int(b), int(c), int(d), 1 if e == "true" else 0) for a, b, c, d, e in rows}
    assert recorded == set(policy_kernels), sorted(set(policy_kernels) ^ recorded)
