"""rsx_task_advantages as a build product (no GPU): the symbols are declared, listed and exported, the two C structs and their ctypes
mirrors agree field for field, the unit is one of build()'s and none of its kernels uses scratch memory, and MLPCritic's parameter
layout is torch's own."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _header():
    return open(os.path.join(ROOT, "include", "rsx.h")).read()


def _fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    return re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_symbols_are_declared_listed_and_exported():
    from build_variant import dynamic_symbols
    from rsoccer_amd import _lib
    header = _header()
    assert re.search(r"^int rsx_task_advantages\(rsx_sim\* h, const rsx_policy_mlp\* critic, const float\* critic_params_dev", header, re.M)
    assert re.search(r"^int rsx_critic_num_params\(const rsx_sim\* h, const rsx_policy_mlp\* critic, int64_t\* out\);", header, re.M)
    defined, _ = dynamic_symbols(_lib.LIB_PATH)
    for sym in ("rsx_task_advantages", "rsx_critic_num_params"):
        assert sym in _lib.SYMBOLS and sym in defined, sym
    from rsoccer_amd.vec.fused import VecFusedEnv
    assert callable(VecFusedEnv.advantages) and callable(_lib.Sim.task_advantages)


def test_structs_agree_with_their_ctypes_mirrors():
    import ctypes as C
    from rsoccer_amd import _lib
    header = _header()
    assert _fields(header, "rsx_adv_in") == [f[0] for f in _lib.AdvIn._fields_] == ["obs", "rewards", "terminated", "truncated", "final_obs", "last_obs"]
    assert _fields(header, "rsx_adv_out") == [f[0] for f in _lib.AdvOut._fields_] == ["values", "advantages", "returns", "next_values"]
    for cls in (_lib.AdvIn, _lib.AdvOut):   # every member is a pointer
        assert all(f[1] is C.c_void_p for f in cls._fields_) and C.sizeof(cls) == len(cls._fields_) * C.sizeof(C.c_void_p)


def test_act_none_is_3_and_the_abi_stays_6():
    from rsoccer_amd import _lib
    header = _header()
    assert re.search(r"^#define RSX_ACT_NONE 3\b", header, re.M) and _lib.ACT_NONE == 3
    assert re.search(r"^#define RSX_ABI_VERSION 6\b", header, re.M)
    for name, value in (("RELU", 0), ("TANH", 1), ("CLIP", 2)):   # the existing ones keep their values
        assert re.search(r"^#define RSX_ACT_%s %d\b" % (name, value), header, re.M), name


def test_the_unit_is_one_of_build_and_restates_no_mlp_piece():
    from __graft_entry__ import CSRC, HIP_UNITS
    assert "rsx_gae.hip" in dict(HIP_UNITS)
    text = open(os.path.join(CSRC, "rsx_gae.hip")).read()
    assert '#include "rsx_policy_mlp.hpp"' in text
    for piece in ("float tanh_f32(", "float policy_act(", "void stage_layer(", "float policy_forward(", "struct PolicyImage"):
        assert piece not in text, piece
    units = open(os.path.join(CSRC, "rsx_units.hpp")).read()
    assert "void launch_advantages(" in units and "rsx_gae.hip" in units


def test_no_kernel_uses_scratch_memory():
    """compiled with the flags build() gives the unit; the compiler's kernel-resource-usage remarks, read the way
    tools/kernel_resources.py reads them"""
    from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS
    work = tempfile.mkdtemp(prefix="rsx_gae_probe_")
    try:
        p = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_COMMON + dict(HIP_UNITS)["rsx_gae.hip"] +
                           ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(work, "rsx_gae.o"),
                            os.path.join(CSRC, "rsx_gae.hip")], stderr=subprocess.PIPE, text=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[.*?\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    kernels = {k: v for k, v in rows.items() if "gae_" in k}
    # the rows form of the values kernel at both widths with one and two waves per workgroup, the groups form at both widths, the scan
    assert sum("gae_values_rows_kernel" in k for k in kernels) == 4 and sum("gae_values_groups_kernel" in k for k in kernels) == 2
    assert sum("gae_scan_kernel" in k for k in kernels) == 1 and len(kernels) == 7, sorted(kernels)
    for k, v in kernels.items():
        print(k, {n: v.get(n) for n in ("VGPRs", "TotalSGPRs", "ScratchSize", "Occupancy")})
        assert v["ScratchSize"] == 0, (k, v)


@pytest.mark.parametrize("obs_dim,hidden,layers,act", [(40, 64, 2, "tanh"), (21, 32, 1, "relu"), (14, 32, 2, "tanh")])
def test_critic_layout_is_parameters_to_vector(obs_dim, hidden, layers, act):
    import torch
    from rsoccer_amd import _lib
    from rsoccer_amd.vec.policy import MLPCritic
    c = MLPCritic(obs_dim, hidden=hidden, layers=layers, hidden_act=act)
    A = torch.nn.ReLU if act == "relu" else torch.nn.Tanh
    mods = [torch.nn.Linear(obs_dim, hidden), A()]
    if layers == 2:
        mods += [torch.nn.Linear(hidden, hidden), A()]
    mods += [torch.nn.Linear(hidden, 1)]
    torch.manual_seed(3)
    net = torch.nn.Sequential(*mods)
    flat = c.from_module(net)
    assert flat.dtype == torch.float32 and tuple(flat.shape) == (c.num_params,)
    assert torch.equal(flat, torch.nn.utils.parameters_to_vector(net.parameters()).detach())
    assert c.shapes[-2:] == [(1, hidden), (1,)] and c.act_dim == 1
    assert [tuple(t.shape) for t in c.unpack(flat)] == c.shapes and torch.equal(c.pack(c.unpack(flat)), flat)
    x = torch.randn(5, obs_dim)
    want = net.double()(x.double())   # a linear output: values outside [-1, 1] pass
    assert torch.allclose(c.forward(x, flat), want, rtol=0, atol=1e-12) and c.forward(x, flat).dtype == torch.float64
    assert c.forward(x, flat, dtype=torch.float32).dtype == torch.float32 and tuple(c.forward(x, flat).shape) == (5, 1)
    big = c.forward(100.0 * x, 10.0 * flat)
    assert float(big.abs().max()) > 1.0 or act == "tanh"
    s = c.spec()
    assert (s.n_hidden_layers, s.hidden, s.hidden_act, s.out_act) == (layers, hidden, _lib.ACT_RELU if act == "relu" else _lib.ACT_TANH, 3)


def test_policy_still_refuses_a_linear_output():
    from rsoccer_amd.vec.policy import MLPCritic, MLPPolicy
    with pytest.raises(ValueError, match="out_act"):
        MLPPolicy(40, 2, out_act="none")
    for kw in (dict(hidden=48), dict(layers=3), dict(hidden_act="gelu")):
        with pytest.raises(ValueError):
            MLPCritic(40, **kw)
    with pytest.raises(ValueError):
        MLPCritic(0)
    assert np.isfinite(MLPCritic(40).num_params) and MLPCritic(40).num_params == 64 * 40 + 64 + 64 * 64 + 64 + 64 + 1
