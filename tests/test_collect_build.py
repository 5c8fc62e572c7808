"""rsx_task_collect_policy as a build product (no GPU): the symbol is declared, listed and exported, the C struct and its ctypes mirror
agree, and the gfx950 code object holds a collect kernel for every single-agent fused task in both physics forms, with the register
budget profiles/LABBOOK.md records.  The MLP pieces live in one header that both policy units include."""
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
KERNEL = re.compile(r"task_collect_policy_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])E")


def test_symbol_is_declared_listed_and_exported():
    from build_variant import dynamic_symbols
    from rsoccer_amd import _lib
    header = open(os.path.join(ROOT, "include", "rsx.h")).read()
    assert re.search(r"^int rsx_task_collect_policy\(rsx_sim\* h, const rsx_policy_mlp\* p, const float\* params_dev", header, re.M)
    body = re.search(r"typedef struct rsx_collect_out \{(.*?)\} rsx_collect_out;", header, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in _lib.CollectOut._fields_] == ["obs", "actions", "rewards", "flags", "final_obs", "mean", "sample"]
    assert re.search(r"^#define RSX_ABI_VERSION 6\b", header, re.M)   # additive: the ABI stays 6
    math = open(os.path.join(ROOT, "rsoccer_amd", "csrc", "rsx_math.hpp")).read()
    assert re.search(r"constexpr uint32_t DOM_POLICY = 7u;", math)
    defined, _ = dynamic_symbols(_lib.LIB_PATH)
    assert "rsx_task_collect_policy" in _lib.SYMBOLS and "rsx_task_collect_policy" in defined
    from rsoccer_amd.vec.fused import VecFusedEnv
    assert callable(VecFusedEnv.collect)


def test_the_mlp_is_stated_once():
    csrc = os.path.join(ROOT, "rsoccer_amd", "csrc")
    shared = open(os.path.join(csrc, "rsx_policy_mlp.hpp")).read()
    pieces = ("struct PolicyImage", "PolicyImage policy_image(", "float tanh_f32(", "float policy_act(", "void load_units(", "void hidden_layer(",
              "void stage_layer(", "float policy_forward(", "struct PolicyArgs")
    for piece in pieces:
        assert shared.count(piece) == 1, piece
    for unit in ("rsx_policy.hip", "rsx_collect.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "rsx_policy_mlp.hpp"' in text, unit
        for piece in pieces:
            assert piece not in text, (unit, piece)
        for frag in ("rsx_step_commands.inc", "rsx_step_wire.inc", "rsx_step_xr.inc"):   # the shared step fragments: included, not restated
            assert f'#include "{frag}"' in text, (unit, frag)


@pytest.fixture(scope="module")
def collect_kernels():
    """{(kind, task, L, NR, phys): {remark: value}} of rsx_collect.hip, compiled with the flags build() gives it — the compiler's
    kernel-resource-usage remarks, read the way tools/kernel_resources.py reads them"""
    from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS
    units = dict(HIP_UNITS)
    assert units["rsx_collect.hip"] == units["rsx_policy.hip"]
    work = tempfile.mkdtemp(prefix="rsx_collect_probe_")
    try:
        p = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_COMMON + units["rsx_collect.hip"] +
                           ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(work, "rsx_collect.o"),
                            os.path.join(CSRC, "rsx_collect.hip")], stderr=subprocess.PIPE, text=True)
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


def test_code_object_holds_every_task_in_both_physics_forms(collect_kernels):
    from rsoccer_amd import _lib
    assert collect_kernels, "rsx_collect.hip compiled to no task_collect_policy_kernel"
    for task, name in TASKS.items():
        for phys in (0, 1):
            have = [k for k in collect_kernels if k[1] == task and k[4] == phys]
            assert have, f"no collect kernel for {name} (physics form {phys})"
            assert all(k[0] == (0 if task == 1 else 1) for k in have)
    assert not [k for k in collect_kernels if k[1] not in TASKS], "a kernel for a task the call refuses"
    for key in ((0, 1, 8, 6), (1, 2, 8, 7), (0, 1, 16, 10), (0, 1, 16, 6), (1, 3, 8, 5), (1, 4, 8, 2), (1, 5, 8, 2)):
        for phys in (0, 1):
            assert key + (phys,) in collect_kernels, key
    assert all(k[2] <= 32 for k in collect_kernels)   # MAX_L 32, as in the lookahead units
    blob = open(_lib.LIB_PATH, "rb").read()
    for k, v in collect_kernels.items():
        assert v["name"].encode() in blob, f"librsx_hip.so lacks {v['name']}"


def test_headline_variants_use_no_scratch_memory(collect_kernels):
    for key in ((0, 1, 8, 6, 0), (1, 2, 8, 7, 0)):   # VSS-v0 3v3 and SSLStaticDefenders 1v6, literal physics
        v = collect_kernels[key]
        print(key, {n: v.get(n) for n in ("VGPRs", "TotalSGPRs", "ScratchSize", "LDS Size", "Occupancy")})
        assert v["ScratchSize"] == 0, v


def test_labbook_records_every_variant(collect_kernels):
    text = open(os.path.join(ROOT, "profiles", "LABBOOK.md")).read()
    rows = re.findall(r"^\| collect `<(\d), (\d), (\d+), (\d+), (false|true)>` \|", text, re.M)
    recorded = {(int(a), int(b), int(c), int(d), 1 if e == "true" else 0) for a, b, c, d, e in rows}
    assert recorded == set(collect_kernels), sorted(set(collect_kernels) ^ recorded)
