"""rsx_task_ppo_gradient as a build product (no GPU): the symbols are declared, listed and exported, the three C structs and their ctypes
mirrors agree field for field, the unit is one of build()'s, restates no piece of the MLP and none of its kernels uses scratch memory;
and the yardstick of the GPU tests — MLPPolicy.forward in float64 plus torch autograd on the loss of include/rsx.h — has the tie and
bound behaviour the header states."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _header():
    return open(os.path.join(ROOT, "include", "rsx.h")).read()


def _members(header, name):
    """[(type, name)] of a typedef'd struct, comments dropped"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(re.sub(r"\s+", " ", t.strip()), n) for t, n in re.findall(r"([\w\s\*]+?)\s*\b(\w+)\s*;", body)]


def test_symbols_are_declared_listed_and_exported():
    from build_variant import dynamic_symbols
    from rsoccer_amd import _lib
    header = _header()
    assert re.search(r"^int rsx_ppo_gradient_workspace\(const rsx_sim\* h, const rsx_policy_mlp\* actor, const rsx_policy_mlp\* critic,", header, re.M)
    assert re.search(r"^int rsx_task_ppo_gradient\(rsx_sim\* h, const rsx_policy_mlp\* actor, const float\* actor_params_dev, const float\* log_std_dev,", header, re.M)
    defined, _ = dynamic_symbols(_lib.LIB_PATH)
    for sym in ("rsx_ppo_gradient_workspace", "rsx_task_ppo_gradient"):
        assert sym in _lib.SYMBOLS and sym in defined, sym
    from rsoccer_amd.vec.fused import VecFusedEnv
    assert callable(VecFusedEnv.ppo_gradient) and callable(_lib.Sim.task_ppo_gradient) and callable(_lib.Sim.ppo_gradient_workspace)


def test_structs_agree_with_their_ctypes_mirrors_and_the_abi_stays_6():
    from rsoccer_amd import _lib
    header = _header()
    ctype_of = {"const float*": C.c_void_p, "float*": C.c_void_p, "const int32_t*": C.c_void_p, "void*": C.c_void_p,
                "int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    want = {"rsx_ppo_in": ["obs", "sample", "old_log_prob", "advantage", "ret", "rows", "n_batch_rows", "n_rows"],
            "rsx_ppo_cfg": ["clip", "vf_coef", "ent_coef", "max_workgroups"],
            "rsx_ppo_out": ["grad_actor", "grad_log_std", "grad_critic", "stats", "mean", "value", "workspace"]}
    for name, cls in (("rsx_ppo_in", _lib.PpoIn), ("rsx_ppo_cfg", _lib.PpoCfg), ("rsx_ppo_out", _lib.PpoOut)):
        members = _members(header, name)
        assert [n for _, n in members] == [f[0] for f in cls._fields_] == want[name], name
        assert [ctype_of[t] for t, _ in members] == [f[1] for f in cls._fields_], name
    assert C.sizeof(_lib.PpoIn) == 64 and C.sizeof(_lib.PpoCfg) == 16 and C.sizeof(_lib.PpoOut) == 56
    assert len(_lib.PPO_STATS) == 8
    assert re.search(r"^#define RSX_ABI_VERSION 6\b", header, re.M)


def test_the_unit_is_one_of_build_and_restates_no_mlp_piece():
    from __graft_entry__ import CSRC, HIP_UNITS
    assert "rsx_ppo.hip" in dict(HIP_UNITS)
    text = open(os.path.join(CSRC, "rsx_ppo.hip")).read()
    assert '#include "rsx_policy_mlp.hpp"' in text
    for piece in ("float tanh_f32(", "void hidden_layer(", "void stage_layer(", "float policy_act(", "struct PolicyImage"):
        assert piece not in text, piece
    units = open(os.path.join(CSRC, "rsx_units.hpp")).read()
    assert "void launch_ppo_gradient(" in units and "rsx_ppo.hip" in units


def test_no_kernel_uses_scratch_memory():
    """compiled with the flags build() gives the unit; the compiler's kernel-resource-usage remarks, read the way
    tests/test_advantages_build.py reads them"""
    from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS
    work = tempfile.mkdtemp(prefix="rsx_ppo_probe_")
    try:
        p = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_COMMON + dict(HIP_UNITS)["rsx_ppo.hip"] +
                           ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(work, "rsx_ppo.o"),
                            os.path.join(CSRC, "rsx_ppo.hip")], stderr=subprocess.PIPE, text=True)
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
    kernels = {k: v for k, v in rows.items() if "mlp_grad_kernel" in k or "ppo_reduce_kernel" in k}
    # the row kernel at both widths with both heads, and the reduce
    assert sum("mlp_grad_kernel" in k for k in kernels) == 4 and sum("ppo_reduce_kernel" in k for k in kernels) == 1, sorted(rows)
    for k, v in kernels.items():
        print(k, {n: v.get(n) for n in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "Occupancy")})
        assert v["ScratchSize"] == 0, (k, v)


def _loss(torch, pol, params, log_std, obs, sample, old_lp, adv, clip):
    """L_pi of include/rsx.h on MLPPolicy.forward in float64 (the pre-out_act mean: the policy's output activation taken off)"""
    import copy
    pre = copy.copy(pol)
    hid = pol._torch_acts()[0]
    pre._torch_acts = lambda: (hid, (lambda v: v))
    mean = pre.forward(obs, params, dtype=torch.float64)
    z = (sample - mean) / log_std.exp()
    lp = (-0.5 * z * z - log_std - 0.9189385332046727).sum(-1)
    ratio = (lp - old_lp).exp()
    return -(torch.minimum(ratio * adv, ratio.clamp(1.0 - clip, 1.0 + clip) * adv)).mean(), ratio


@pytest.mark.parametrize("where", ["one", "upper", "lower"])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_autograd_of_the_yardstick_has_the_stated_tie_and_bound_behaviour(where, sign):
    """rows whose ratio is EXACTLY 1, 1 + clip or 1 - clip (old_log_prob is set from the row's own lp in float64, so that the
    difference is an exact 0, log(1 + clip) or log(1 - clip) up to what the assertion on ratio allows): dL/dratio = -A / M there for both
    signs of A, i.e. the gradient with respect to the parameters equals that of the unclipped surrogate -mean(ratio * A)"""
    import torch
    from rsoccer_amd.vec.policy import MLPPolicy
    torch.manual_seed(5)
    clip = 0.25   # (1 +- clip are exact binary fractions)
    pol = MLPPolicy(14, 2, hidden=32, layers=2, hidden_act="tanh", out_act="tanh")
    M = 6
    obs = torch.randn(M, 14, dtype=torch.float64)
    sample = torch.randn(M, 2, dtype=torch.float64)
    adv = sign * (0.5 + torch.rand(M, dtype=torch.float64))
    log_std = torch.full((2,), -0.5, dtype=torch.float64, requires_grad=True)
    params = (0.3 * torch.randn(pol.num_params, dtype=torch.float64)).requires_grad_(True)
    target = {"one": 1.0, "upper": 1.0 + clip, "lower": 1.0 - clip}[where]
    with torch.no_grad():
        _, r0 = _loss(torch, pol, params, log_std, obs, sample, torch.zeros(M, dtype=torch.float64), adv, clip)
        old_lp = r0.log()   # ratio = exp(lp - lp) == 1 exactly
    loss, ratio = _loss(torch, pol, params, log_std, obs, sample, old_lp, adv, clip)
    assert torch.equal(ratio.detach(), torch.ones(M, dtype=torch.float64))
    # scale through the advantage instead of through old_log_prob: ratio' = target * ratio is exact in float64 for these targets
    def surrogate(clipped):
        _, r = _loss(torch, pol, params, log_std, obs, sample, old_lp, adv, clip)
        r = target * r
        assert torch.equal(r.detach(), torch.full((M,), target, dtype=torch.float64))
        s1 = r * adv
        return -(torch.minimum(s1, r.clamp(1.0 - clip, 1.0 + clip) * adv)).mean() if clipped else -s1.mean()
    g_clip = torch.autograd.grad(surrogate(True), [params, log_std])
    g_open = torch.autograd.grad(surrogate(False), [params, log_std])
    for a, b in zip(g_clip, g_open):
        assert float(b.abs().max()) > 0.0
        assert torch.allclose(a, b, rtol=1e-12, atol=0.0), (where, sign, float((a - b).abs().max()))
    # and just outside the bound on the clipped side the gradient is exactly 0
    if where != "one":
        def outside():
            _, r = _loss(torch, pol, params, log_std, obs, sample, old_lp, adv, clip)
            r = (target + (1e-9 if where == "upper" else -1e-9)) * r
            return -(torch.minimum(r * adv, r.clamp(1.0 - clip, 1.0 + clip) * adv)).mean()
        g_out = torch.autograd.grad(outside(), [params, log_std])
        blocked = (where == "upper") == (sign > 0)   # min() picks the clamped branch: A > 0 above the bound, A < 0 below it
        for a, b in zip(g_out, g_open):
            if blocked:
                assert float(a.abs().max()) == 0.0
            else:
                assert torch.allclose(a, b, rtol=1e-6, atol=0.0)
