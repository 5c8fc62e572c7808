"""rsx_task_dpg_gradient as a build product (no GPU): the symbols are declared, listed and exported, the three C structs and their ctypes
mirrors agree field for field, the unit is one of build()'s, restates no piece of the MLP and none of its kernels uses scratch memory;
and the yardstick of the GPU tests (tests/dpg_helpers.py: torch autograd on the losses of include/rsx.h) has the behaviour the header
states at a clip actor's bounds and at a tie of the two target critics; and its kink filter stays within 2 % on every case's seed."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

import dpg_helpers as DH

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
    assert re.search(r"^int rsx_dpg_gradient_workspace\(const rsx_sim\* h, const rsx_policy_mlp\* actor, const rsx_policy_mlp\* critic, int n_critics,", header, re.M)
    assert re.search(r"^int rsx_task_dpg_gradient\(rsx_sim\* h, const rsx_policy_mlp\* actor, const float\* actor_params_dev, const float\* target_actor_params_dev,", header, re.M)
    defined, _ = dynamic_symbols(_lib.LIB_PATH)
    for sym in ("rsx_dpg_gradient_workspace", "rsx_task_dpg_gradient"):
        assert sym in _lib.SYMBOLS and sym in defined, sym
    from rsoccer_amd.vec.fused import VecFusedEnv
    from rsoccer_amd.vec.policy import MLPQCritic
    from rsoccer_amd.vec.replay import ReplayBuffer
    assert callable(VecFusedEnv.dpg_gradient) and callable(_lib.Sim.task_dpg_gradient) and callable(_lib.Sim.dpg_gradient_workspace)
    assert callable(MLPQCritic) and callable(ReplayBuffer)


def test_structs_agree_with_their_ctypes_mirrors_and_the_abi_stays_6():
    from rsoccer_amd import _lib
    header = _header()
    ctype_of = {"const float*": C.c_void_p, "float*": C.c_void_p, "const int32_t*": C.c_void_p, "void*": C.c_void_p,
                "const uint8_t*": C.c_void_p, "const int64_t*": C.c_void_p, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
                "int32_t": C.c_int32, "float": C.c_float}
    want = {"rsx_dpg_in": ["obs", "action", "reward", "next_obs", "terminated", "rows", "n_batch_rows", "n_rows"],
            "rsx_dpg_cfg": ["noise_step_dev", "noise_seed", "noise_step", "gamma", "sigma", "noise_clip", "n_critics", "max_workgroups"],
            "rsx_dpg_out": ["grad_actor", "grad_critics", "stats", "target", "q", "action", "target_noise", "workspace"]}
    for name, cls in (("rsx_dpg_in", _lib.DpgIn), ("rsx_dpg_cfg", _lib.DpgCfg), ("rsx_dpg_out", _lib.DpgOut)):
        members = _members(header, name)
        assert [n for _, n in members] == [f[0] for f in cls._fields_] == want[name], name
        assert [ctype_of[t] for t, _ in members] == [f[1] for f in cls._fields_], name
    assert C.sizeof(_lib.DpgIn) == 64 and C.sizeof(_lib.DpgCfg) == 48 and C.sizeof(_lib.DpgOut) == 64
    assert len(_lib.DPG_STATS) == 9 and set(DH.FLOAT_STATS) | {"rows_used", "rows_skipped"} == set(_lib.DPG_STATS)
    assert re.search(r"^#define RSX_ABI_VERSION 6\b", header, re.M)


def test_the_unit_is_one_of_build_and_restates_no_mlp_piece():
    from __graft_entry__ import CSRC, HIP_UNITS
    units_of = dict(HIP_UNITS)
    assert "rsx_dpg.hip" in units_of and units_of["rsx_dpg.hip"] == units_of["rsx_ppo.hip"]
    text = open(os.path.join(CSRC, "rsx_dpg.hip")).read()
    assert '#include "rsx_policy_mlp.hpp"' in text
    for piece in ("float tanh_f32(", "void hidden_layer(", "void stage_layer(", "float policy_act(", "struct PolicyImage", "void stage_policy(",
                  "void plan_normal_pair(", "philox4x32(uint32_t"):
        assert piece not in text, piece
    units = open(os.path.join(CSRC, "rsx_units.hpp")).read()
    assert "void launch_dpg_gradient(" in units and "rsx_dpg.hip" in units


def test_no_kernel_uses_scratch_memory():
    """compiled with the flags build() gives the unit; the compiler's kernel-resource-usage remarks, read the way
    tests/test_ppo_build.py reads them"""
    from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS
    work = tempfile.mkdtemp(prefix="rsx_dpg_probe_")
    try:
        p = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_COMMON + dict(HIP_UNITS)["rsx_dpg.hip"] +
                           ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(work, "rsx_dpg.o"),
                            os.path.join(CSRC, "rsx_dpg.hip")], stderr=subprocess.PIPE, text=True)
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
    count = lambda s: sum(s in k for k in rows)   # noqa: E731
    # the target and the actor kernel at both widths of both networks, the critic kernel at both widths, and the reduce
    assert (count("dpg_target_kernel"), count("dpg_critic_kernel"), count("dpg_actor_kernel"), count("dpg_reduce_kernel")) == (4, 2, 4, 1), sorted(rows)
    for k, v in rows.items():
        if "dpg_" in k:
            print(k, {n: v.get(n) for n in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "Occupancy")})
            assert v["ScratchSize"] == 0, (k, v)


def test_mlpqcritic_has_the_layout_of_the_matching_sequential():
    import torch
    from rsoccer_amd.vec.policy import MLPQCritic
    torch.manual_seed(3)
    for layers in (1, 2):
        crit = MLPQCritic(14, 5, hidden=32, layers=layers, hidden_act="relu")
        mods = [torch.nn.Linear(19, 32), torch.nn.ReLU()] + ([torch.nn.Linear(32, 32), torch.nn.ReLU()] if layers == 2 else []) + [torch.nn.Linear(32, 1)]
        seq = torch.nn.Sequential(*mods).double()
        flat = torch.nn.utils.parameters_to_vector(seq.parameters())
        assert flat.numel() == crit.num_params and torch.equal(crit.from_module(seq), flat.float())
        obs, act = torch.randn(7, 14, dtype=torch.float64), torch.randn(7, 5, dtype=torch.float64)
        assert torch.allclose(crit.forward(obs, act, flat), seq(torch.cat([obs, act], -1)), rtol=1e-12, atol=1e-12)
        assert crit.spec().out_act == 3
    with pytest.raises(ValueError):
        crit.forward(torch.zeros(2, 13), torch.zeros(2, 5), flat)


# ---- the yardstick ----
def _tiny(torch, out_act="clip"):
    from rsoccer_amd.vec.policy import MLPPolicy, MLPQCritic
    torch.manual_seed(5)
    pol = MLPPolicy(14, 2, hidden=32, layers=1, hidden_act="tanh", out_act=out_act)
    crit = MLPQCritic(14, 2, hidden=32, layers=2, hidden_act="tanh")
    return pol, crit


@pytest.mark.parametrize("bound", [1.0, -1.0])
def test_the_gradient_passes_a_clip_actor_at_its_bounds_and_is_zero_just_outside(bound):
    """zero hidden-to-output weights make the mean the output bias: set EXACTLY to +-1 the gradient of L_pi with respect to that bias is
    dQ/da itself (torch's clamp passes its bounds); one step of 1e-9 further out it is exactly 0"""
    import torch
    pol, crit = _tiny(torch)
    M = 6
    obs = torch.randn(M, 14, dtype=torch.float64)
    cp = 0.3 * torch.randn(1, crit.num_params, dtype=torch.float64)
    ts = [0.3 * torch.randn(s, dtype=torch.float64) for s in pol.shapes]
    ts[-2].zero_()

    def grad_bias(value):
        ts[-1][:] = value
        p = torch.cat([t.reshape(-1) for t in ts]).requires_grad_(True)
        rows_of = {"obs": obs, "actions": torch.zeros(M, 2, dtype=torch.float64), "reward": torch.zeros(M), "next_obs": obs,
                   "terminated": torch.zeros(M, dtype=torch.bool)}
        _, l_pi, _ = DH.losses(torch, pol, crit, p, p.detach(), cp, cp, rows_of, None, 0.9, torch.float64, M)
        return pol.unpack(torch.autograd.grad(l_pi, [p])[0])[-1]

    a = torch.full((M, 2), bound, dtype=torch.float64, requires_grad=True)
    dq_da = torch.autograd.grad(-crit.forward(obs, a, cp[0])[..., 0].sum() / M, [a])[0].sum(0)
    at = grad_bias(bound)
    assert float(dq_da.abs().min()) > 0.0 and torch.allclose(at, dq_da, rtol=1e-12, atol=0.0)
    assert float(grad_bias(bound * (1.0 + 1e-9)).abs().max()) == 0.0
    assert torch.allclose(grad_bias(bound * (1.0 - 1e-9)), dq_da, rtol=1e-6, atol=0.0)


def test_a_tie_of_the_two_target_critics_leaves_y_unchanged():
    import torch
    pol, crit = _tiny(torch, out_act="tanh")
    M = 9
    obs, rew = torch.randn(M, 14, dtype=torch.float64), torch.randn(M, dtype=torch.float64)
    term = torch.arange(M) % 4 == 0
    tp = 0.3 * torch.randn(pol.num_params, dtype=torch.float64)
    one = 0.3 * torch.randn(1, crit.num_params, dtype=torch.float64)
    y1, a1 = DH.targets(torch, pol, crit, tp, one, obs, rew, term, None, 0.9, torch.float64)
    y2, a2 = DH.targets(torch, pol, crit, tp, torch.cat([one, one]), obs, rew, term, None, 0.9, torch.float64)
    assert torch.equal(y1, y2) and torch.equal(a1, a2)
    assert torch.equal(y1[term], rew[term]) and not torch.equal(y1[~term], rew[~term])
    # the smaller critic decides, and the clamped noise moves a' by at most the clip
    other = one + 0.05 * torch.randn(1, crit.num_params, dtype=torch.float64)
    y3, _ = DH.targets(torch, pol, crit, tp, torch.cat([one, other]), obs, rew, term, None, 0.9, torch.float64)
    y4, _ = DH.targets(torch, pol, crit, tp, other, obs, rew, term, None, 0.9, torch.float64)
    assert torch.equal(y3, torch.minimum(y1, y4))
    noise = (0.2 * torch.randn(M, 2, dtype=torch.float64)).clamp(-0.1, 0.1)
    _, a5 = DH.targets(torch, pol, crit, tp, one, obs, rew, term, noise, 0.9, torch.float64)
    assert float((a5 - a1).abs().max()) <= 0.1 and float(a5.abs().max()) <= 1.0


@pytest.mark.parametrize("case", DH.CASES, ids=[str(i) for i in range(len(DH.CASES))])
def test_the_kink_filter_stays_within_two_percent_on_every_gpu_case(case):
    """a condition of the GPU test, checked here on the float64 reference alone"""
    import torch
    pol, _, data, removed, n = DH.case_data(torch, case)
    print(case, "removed", removed, "of", n)
    assert removed <= 0.02 * n and data["obs"].shape[0] >= case[6]
    if pol.out_act == "clip" and n > 1000:   # the clamp binds on a share of the rows, and not on all
        import copy
        pre = copy.copy(pol)
        hid = pol._torch_acts()[0]
        pre._torch_acts = lambda: (hid, (lambda v: v))
        share = float((pre.forward(data["obs"], data["params"]).abs() > 1.0).double().mean())
        print("share of means outside [-1, 1]:", share)
        assert 0.02 < share < 0.9
