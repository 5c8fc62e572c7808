"""The soft actor-critic pieces as build products and in torch (no GPU): rsx_task_collect_gaussian, rsx_sac_gradient_workspace and
rsx_task_sac_gradient are declared, listed and exported, the new structs and their ctypes mirrors agree, the ABI stays 6, both units are
built with their siblings' flags from the shared MLP pieces, no kernel of either uses scratch memory, MLPGaussianPolicy has the layout
and the head include/rsx.h states, and the torch yardstick of the GPU test (tests/sac_helpers.py) has the properties the losses state."""
import math
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

import sac_helpers as SH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

UNIT = "rsx_collect_gaussian.hip"
TASKS = {1: "VSS-v0", 2: "SSLStaticDefenders", 3: "SSLDribbling", 4: "SSLContestedPossession", 5: "SSLPassEndurance"}
KERNEL = re.compile(r"task_collect_gaussian_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])E")


def _struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):   # `float a, b` declares two fields
        decl = decl.strip()
        if decl:
            first, *more = decl.split(",")
            names += [first.split()[-1].lstrip("*")] + [m.strip().lstrip("*") for m in more]
    return names


def test_symbol_is_declared_listed_and_exported():
    from build_variant import dynamic_symbols
    from rsoccer_amd import _lib
    header = open(os.path.join(ROOT, "include", "rsx.h")).read()
    assert re.search(r"^int rsx_task_collect_gaussian\(rsx_sim\* h, const rsx_policy_mlp\* p, const float\* params_dev", header, re.M)
    assert _struct_fields(header, "rsx_collect_gaussian_cfg") == [f[0] for f in _lib.CollectGaussianCfg._fields_] == \
        ["noise_seed", "log_std_min", "log_std_max", "deterministic", "reserved"]
    import ctypes
    assert ctypes.sizeof(_lib.CollectGaussianCfg) == 24   # uint64, two floats, two int32: no padding
    assert _struct_fields(header, "rsx_collect_out") == [f[0] for f in _lib.CollectOut._fields_]   # reused as it is
    assert re.search(r"^#define RSX_ABI_VERSION 6\b", header, re.M)   # additive: the ABI stays 6
    defined, _ = dynamic_symbols(_lib.LIB_PATH)
    assert "rsx_task_collect_gaussian" in _lib.SYMBOLS and "rsx_task_collect_gaussian" in defined
    import inspect
    from rsoccer_amd.vec.fused import VecFusedEnv
    sig = inspect.signature(VecFusedEnv.collect)
    assert sig.parameters["deterministic"].default is False
    assert list(sig.parameters)[-1] == "deterministic"   # appended: every existing positional call means what it meant


def test_the_unit_is_built_from_the_shared_mlp():
    from __graft_entry__ import CSRC, HIP_UNITS
    units = dict(HIP_UNITS)
    assert units[UNIT] == units["rsx_collect.hip"]
    shared = open(os.path.join(CSRC, "rsx_policy_mlp.hpp")).read()
    pieces = ("struct PolicyImage", "PolicyImage policy_image(", "float tanh_f32(", "float policy_act(", "void load_units(", "void hidden_layer(",
              "void stage_layer(", "float policy_forward(", "struct PolicyArgs", "void stage_policy(")
    for piece in pieces:
        assert shared.count(piece) == 1, piece
    for name in (UNIT, "rsx_gaussian_head.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "rsx_policy_mlp.hpp"' in text, name
        for piece in pieces:
            assert piece not in text, (name, piece)
    text = open(os.path.join(CSRC, UNIT)).read()
    for frag in ("rsx_step_commands.inc", "rsx_step_wire.inc", "rsx_step_xr.inc", "rsx_step_reward.inc", "rsx_step_ball_load.inc",
                 "rsx_step_vss_metrics.inc"):   # the shared step fragments: included, not restated
        assert f'#include "{frag}"' in text, frag
    head = open(os.path.join(CSRC, "rsx_gaussian_head.hpp")).read()
    for piece in ("float exp_f32(", "PolicyImage gaussian_image(", "float gaussian_forward("):
        assert head.count(piece) == 1 and piece not in text, piece
    assert "DOM_POLICY" in text   # the collector's own draw


@pytest.fixture(scope="module")
def kernels():
    """{(kind, task, L, NR, phys): {remark: value}} of the unit, compiled with the flags build() gives it"""
    from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS
    work = tempfile.mkdtemp(prefix="rsx_sac_probe_")
    try:
        p = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_COMMON + dict(HIP_UNITS)[UNIT] +
                           ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(work, "unit.o"), os.path.join(CSRC, UNIT)],
                           stderr=subprocess.PIPE, text=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows, cur, others = {}, None, []
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = KERNEL.search(m.group(1))
            if not k:
                others.append(m.group(1))
            cur = rows.setdefault(tuple(int(x) for x in k.groups()), {"name": m.group(1)}) if k else None
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[.*?\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    assert not others, others   # the unit holds this one kernel family and nothing else
    return rows


def test_code_object_serves_every_handle_the_collector_serves(kernels):
    from rsoccer_amd import _lib
    assert kernels
    for task, name in TASKS.items():
        for phys in (0, 1):
            assert [k for k in kernels if k[1] == task and k[4] == phys], f"no kernel for {name} (physics form {phys})"
    assert not [k for k in kernels if k[1] not in TASKS], "a kernel for a task the call refuses"
    # the collector's own variants, one for one (tests/test_collect_build.py lists its headline keys)
    for key in ((0, 1, 8, 6), (1, 2, 8, 7), (0, 1, 16, 10), (0, 1, 16, 6), (1, 3, 8, 5), (1, 4, 8, 2), (1, 5, 8, 2)):
        for phys in (0, 1):
            assert key + (phys,) in kernels, key
    assert {k[2] for k in kernels} == {8, 16, 32}
    labbook = open(os.path.join(ROOT, "profiles", "LABBOOK.md")).read()
    rows = re.findall(r"^\| collect `<(\d), (\d), (\d+), (\d+), (false|true)>` \|", labbook, re.M)
    assert {(int(a), int(b), int(c), int(d), 1 if e == "true" else 0) for a, b, c, d, e in rows} == set(kernels)
    blob = open(_lib.LIB_PATH, "rb").read()
    for v in kernels.values():
        assert v["name"].encode() in blob, f"librsx_hip.so lacks {v['name']}"


def test_no_kernel_uses_scratch_memory(kernels):
    for key, v in sorted(kernels.items()):
        assert v["ScratchSize"] == 0, (key, v)
    v = kernels[(0, 1, 8, 6, 0)]   # VSS-v0 3v3: the static block include/rsx.h adds to the image's 36 928 B
    print({n: v.get(n) for n in ("VGPRs", "TotalSGPRs", "ScratchSize", "LDS Size", "Occupancy")})
    assert v["LDS Size"] == 6272
    header = open(os.path.join(ROOT, "include", "rsx.h")).read()
    assert "36 928 B of image" in header and "+ 6 272 B = 43 200 B, three workgroups per CU" in header
    assert 3 * 43200 <= 163840 < 4 * 43200


# ---- the policy shape ----
@pytest.mark.parametrize("layers,hidden,act", [(1, 32, "relu"), (2, 64, "tanh")])
def test_layout_is_the_sequentials(layers, hidden, act):
    import torch
    from rsoccer_amd import _lib
    from rsoccer_amd.vec.policy import MLPGaussianPolicy, MLPPolicy
    OD, AD = 11, 3
    pol = MLPGaussianPolicy(OD, AD, hidden=hidden, layers=layers, hidden_act=act)
    assert isinstance(pol, MLPPolicy) and pol.act_dim == AD
    torch.manual_seed(3)
    A = torch.nn.ReLU if act == "relu" else torch.nn.Tanh
    mods = [torch.nn.Linear(OD, hidden), A()] + ([torch.nn.Linear(hidden, hidden), A()] if layers == 2 else []) + [torch.nn.Linear(hidden, 2 * AD)]
    net = torch.nn.Sequential(*mods).double()
    with torch.no_grad():
        net[-1].weight[AD:] *= 8.0   # log-std rows that reach both bounds of the narrow setting below
    flat = torch.nn.utils.parameters_to_vector(net.parameters())
    assert pol.num_params == flat.numel() == plain_params(OD, AD, hidden, layers) + AD * hidden + AD
    assert torch.equal(pol.from_module(net), flat.float())
    assert [tuple(t.shape) for t in pol.unpack(flat)] == pol.shapes and pol.shapes[-2:] == [(2 * AD, hidden), (2 * AD,)]
    assert torch.equal(pol.pack(pol.unpack(flat)), flat.float())
    s = pol.spec()
    assert (s.n_hidden_layers, s.hidden, s.out_act) == (layers, hidden, _lib.ACT_NONE)
    obs = torch.randn(50, OD, dtype=torch.float64)
    mu, raw = net(obs).chunk(2, -1)
    got_mu, got_ls = pol.forward(obs, flat)
    assert got_mu.dtype == torch.float64 and torch.allclose(got_mu, mu, rtol=0, atol=1e-12)
    assert torch.allclose(got_ls, raw.clamp(-20.0, 2.0), rtol=0, atol=1e-12)
    narrow = MLPGaussianPolicy(OD, AD, hidden=hidden, layers=layers, hidden_act=act, log_std_min=-1.0, log_std_max=0.5)
    ls = narrow.forward(obs, flat)[1]
    assert ls.min() == -1.0 and ls.max() == 0.5 and ((ls > -1.0) & (ls < 0.5)).any()
    assert narrow.forward(obs, flat.float(), dtype=torch.float32)[0].dtype == torch.float32


def plain_params(OD, AD, hidden, layers):
    from rsoccer_amd.vec.policy import MLPPolicy
    return MLPPolicy(OD, AD, hidden=hidden, layers=layers).num_params


def test_sample_is_torch_distributions():
    import torch
    from torch.distributions import Normal
    from torch.distributions.transforms import TanhTransform
    from rsoccer_amd.vec.policy import MLPGaussianPolicy, squashed_log_prob
    OD, AD = 7, 4
    pol = MLPGaussianPolicy(OD, AD, hidden=32, layers=1, log_std_min=-3.0, log_std_max=1.0)
    g = torch.Generator().manual_seed(11)
    params = (torch.rand(pol.num_params, generator=g, dtype=torch.float64) - 0.5)
    obs = torch.randn(4000, OD, generator=g, dtype=torch.float64)
    eps = torch.randn(4000, AD, generator=g, dtype=torch.float64)
    mu, ls = pol.forward(obs, params)
    a, lp, u = pol.sample(obs, params, eps)
    assert torch.equal(u, mu + ls.exp() * eps) and torch.equal(a, u.tanh())
    keep = (u.abs() <= 5.0).all(-1)   # beyond that 1 - tanh^2 underflows in the distribution's own formula for the inverse
    assert keep.float().mean() > 0.9 and u[keep].abs().max() > 4.0, "uninformative: the samples do not reach the tails"
    # Normal + TanhTransform, evaluated at u itself (TransformedDistribution.log_prob would first invert tanh, which loses digits)
    want = (Normal(mu, ls.exp()).log_prob(u) - TanhTransform().log_abs_det_jacobian(u, a)).sum(-1)
    err = (lp - want).abs()[keep].max().item()
    print(f"log_prob against Normal + TanhTransform in float64: max error {err:.3e} over {int(keep.sum())} rows, |u| up to {u[keep].abs().max():.2f}")
    assert err <= 1e-9
    # the naive form the header warns against agrees where tanh is far from saturation, so the stable form is the same quantity
    mild = (u.abs() <= 2.0).all(-1)
    naive = (Normal(mu, ls.exp()).log_prob(u) - torch.log(1.0 - a * a)).sum(-1)
    assert (lp - naive).abs()[mild].max() <= 1e-9
    # with the reparameterisation d logp / d u_k = 2 a_k (eps and log_std constants)
    uu = u[:64].clone().requires_grad_(True)
    squashed_log_prob(eps[:64], ls[:64], uu).sum().backward()
    assert torch.allclose(uu.grad, 2.0 * uu.detach().tanh(), rtol=0, atol=1e-12)


def test_clamp_gradient_is_torch_clamps():
    """the log-std gradient is exactly 0 one step of 1e-9 outside a bound and passes at the bound"""
    import torch
    from rsoccer_amd.vec.policy import MLPGaussianPolicy
    OD, AD, H = 3, 2, 32
    pol = MLPGaussianPolicy(OD, AD, hidden=H, layers=1, hidden_act="relu", log_std_min=-1.0, log_std_max=0.5)
    obs = torch.zeros(1, OD, dtype=torch.float64)
    for bound in (-1.0, 0.5):
        for step, passes in ((0.0, True), (1e-9 * math.copysign(1.0, bound), False), (-1e-9 * math.copysign(1.0, bound), True)):
            ts = [torch.zeros(s, dtype=torch.float64) for s in pol.shapes]
            ts[-1][AD:] = bound + step   # zero weights: raw is the bias
            flat = torch.cat([t.reshape(-1) for t in ts]).requires_grad_(True)
            mu, ls = pol.forward(obs, flat)
            assert ls[0, 0].item() == (bound if not passes or step == 0.0 else bound + step)
            ls.sum().backward()
            grad_raw_bias = flat.grad[-AD:]
            assert torch.equal(grad_raw_bias, torch.full((AD,), 1.0 if passes else 0.0, dtype=torch.float64)), (bound, step)


def test_refused_shapes():
    from rsoccer_amd.vec.policy import MLPGaussianPolicy
    MLPGaussianPolicy(40, 8)
    for kw in (dict(act_dim=9), dict(act_dim=0), dict(hidden=48), dict(layers=3), dict(hidden_act="gelu"), dict(log_std_min=2.0),
               dict(log_std_min=2.0, log_std_max=2.0), dict(log_std_min=float("-inf")), dict(log_std_max=float("nan")),
               dict(log_std_max=float("inf"))):
        args = dict(obs_dim=40, act_dim=2)
        args.update(kw)
        with pytest.raises(ValueError):
            MLPGaussianPolicy(**args)
    with pytest.raises(TypeError):
        MLPGaussianPolicy(40, 2, out_act="clip")   # the head is the output activation


# ---- rsx_task_sac_gradient as a build product ----
def test_gradient_symbols_structs_and_unit():
    import ctypes as C
    from __graft_entry__ import CSRC, HIP_UNITS
    from build_variant import dynamic_symbols
    from rsoccer_amd import _lib
    header = open(os.path.join(ROOT, "include", "rsx.h")).read()
    assert re.search(r"^int rsx_sac_gradient_workspace\(const rsx_sim\* h, const rsx_policy_mlp\* actor, const rsx_policy_mlp\* critic, int n_critics,", header, re.M)
    assert re.search(r"^int rsx_task_sac_gradient\(rsx_sim\* h, const rsx_policy_mlp\* actor, const float\* actor_params_dev,", header, re.M)
    defined, _ = dynamic_symbols(_lib.LIB_PATH)
    for sym in ("rsx_task_collect_gaussian", "rsx_sac_gradient_workspace", "rsx_task_sac_gradient"):
        assert sym in _lib.SYMBOLS and sym in defined, sym
    assert _struct_fields(header, "rsx_sac_cfg") == [f[0] for f in _lib.SacCfg._fields_] == \
        ["noise_step_dev", "noise_seed", "noise_step", "gamma", "target_entropy", "log_std_min", "log_std_max", "n_critics", "max_workgroups"]
    assert _struct_fields(header, "rsx_sac_out") == [f[0] for f in _lib.SacOut._fields_] == \
        ["grad_actor", "grad_critics", "grad_log_alpha", "stats", "target", "q", "action", "log_prob", "next_log_prob", "eps", "next_eps",
         "mean", "log_std", "workspace"]
    assert C.sizeof(_lib.SacCfg) == 48 and C.sizeof(_lib.SacOut) == 14 * 8
    assert all(f[1] is C.c_void_p for f in _lib.SacOut._fields_)
    assert [f[1] for f in _lib.SacCfg._fields_] == [C.c_void_p, C.c_uint64, C.c_int64] + [C.c_float] * 4 + [C.c_int32] * 2
    assert len(_lib.SAC_STATS) == 12 and set(SH.FLOAT_STATS) | {"rows_used", "rows_skipped"} == set(_lib.SAC_STATS)
    stats_doc = re.search(r"stats\s+\[12\]:(.*?)per entry", header, flags=re.S).group(1)
    for slot, word in enumerate(("L_q", "L_q", "mean Q_0", "Q_1", "L_pi", "L_alpha", "mean y", "mean logp", "mean logp'", "alpha", "entries used",
                                 "entries skipped")):
        assert word in stats_doc, (slot, word)
    assert re.search(r"^#define RSX_ABI_VERSION 6\b", header, re.M)
    units = dict(HIP_UNITS)
    assert units["rsx_sac.hip"] == units["rsx_dpg.hip"]
    text = open(os.path.join(CSRC, "rsx_sac.hip")).read()
    for inc in ("rsx_policy_mlp.hpp", "rsx_gaussian_head.hpp", "rsx_qnet.hpp"):
        assert f'#include "{inc}"' in text, inc
    for piece in ("float tanh_f32(", "void hidden_layer(", "void stage_layer(", "float policy_act(", "struct PolicyImage", "void stage_policy(",
                  "void plan_normal_pair(", "philox4x32(uint32_t", "float exp_f32(", "float log1p_f32(", "void forward_hidden(", "void backward(",
                  "void wgrad_tile(", "void bias_grad("):
        assert piece not in text, piece
    dpg, shared = open(os.path.join(CSRC, "rsx_dpg.hip")).read(), open(os.path.join(CSRC, "rsx_qnet.hpp")).read()
    for piece in ("void forward_hidden(", "void backward(", "void wgrad_tile(", "void bias_grad(", "void fold_stats("):   # stated once, shared
        assert shared.count(piece) == 1 and piece not in dpg and '#include "rsx_qnet.hpp"' in dpg, piece
    from rsoccer_amd.vec.fused import VecFusedEnv
    assert callable(VecFusedEnv.sac_gradient) and callable(_lib.Sim.task_sac_gradient) and callable(_lib.Sim.sac_gradient_workspace)


def test_no_gradient_kernel_uses_scratch_memory():
    from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS
    work = tempfile.mkdtemp(prefix="rsx_sac_probe_")
    try:
        p = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_COMMON + dict(HIP_UNITS)["rsx_sac.hip"] +
                           ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(work, "rsx_sac.o"),
                            os.path.join(CSRC, "rsx_sac.hip")], stderr=subprocess.PIPE, text=True)
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
    # the target kernel at both widths of both networks, the four one-network kernels at both widths, and the reduce
    assert [count(f"sac_{k}_kernel") for k in ("target", "critic", "sample", "qa", "actor", "reduce")] == [4, 2, 2, 2, 2, 1], sorted(rows)
    assert all("sac_" in k for k in rows), sorted(rows)
    for k, v in rows.items():
        print(k, {n: v.get(n) for n in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "Occupancy")})
        assert v["ScratchSize"] == 0, (k, v)


# ---- the yardstick ----
def _tiny(torch, C=2, act="tanh", lo=-1.0, hi=0.5):
    from rsoccer_amd.vec.policy import MLPGaussianPolicy, MLPQCritic
    pol = MLPGaussianPolicy(14, 2, hidden=32, layers=1, hidden_act=act, log_std_min=lo, log_std_max=hi)
    crit = MLPQCritic(14, 2, hidden=32, layers=2, hidden_act=act)
    g = torch.Generator().manual_seed(5)
    M = 9
    rows_of = {"obs": torch.randn(M, 14, generator=g, dtype=torch.float64), "actions": torch.rand(M, 2, generator=g, dtype=torch.float64) * 2 - 1,
               "reward": torch.randn(M, generator=g, dtype=torch.float64), "next_obs": torch.randn(M, 14, generator=g, dtype=torch.float64),
               "terminated": torch.arange(M) % 4 == 0}
    eps, neps = torch.randn(M, 2, generator=g, dtype=torch.float64), torch.randn(M, 2, generator=g, dtype=torch.float64)
    p = 0.3 * torch.randn(pol.num_params, generator=g, dtype=torch.float64)
    cp = 0.3 * torch.randn(C, crit.num_params, generator=g, dtype=torch.float64)
    return pol, crit, rows_of, eps, neps, p, cp, torch.tensor([-0.7], dtype=torch.float64), M


@pytest.mark.parametrize("bound", [-1.0, 0.5])
def test_the_log_std_gradient_is_zero_one_step_outside_a_bound_and_passes_at_it(bound):
    import torch
    pol, crit, rows_of, eps, neps, p, cp, la, M = _tiny(torch)
    ts = [t.clone() for t in pol.unpack(p)]
    ts[-2][2:] = 0.0   # zero log-std rows: raw is the bias

    def grad_raw_bias(value):
        ts[-1][2:] = value
        flat = torch.cat([t.reshape(-1) for t in ts]).requires_grad_(True)
        _, l_pi, _, _ = SH.losses(torch, pol, crit, flat, cp, cp, la, rows_of, eps, neps, 0.9, -2.0, torch.float64, M)
        return pol.unpack(torch.autograd.grad(l_pi, [flat])[0])[-1][2:]

    out = 1e-9 if bound > 0 else -1e-9   # one step further out
    at = grad_raw_bias(bound)
    assert float(at.abs().min()) > 0.0
    assert float(grad_raw_bias(bound + out).abs().max()) == 0.0
    assert torch.allclose(grad_raw_bias(bound - out), at, rtol=1e-6, atol=0.0)


def test_a_tie_of_the_critics_gives_the_gradient_either_gives_and_terminated_rows_have_y_equal_reward():
    import torch
    pol, crit, rows_of, eps, neps, p, cp, la, M = _tiny(torch, C=1)
    grads = []
    for cps in (cp, torch.cat([cp, cp])):
        flat = p.clone().requires_grad_(True)
        _, l_pi, _, stats = SH.losses(torch, pol, crit, flat, cps, cps, la, rows_of, eps, neps, 0.9, -2.0, torch.float64, M)
        grads.append(torch.autograd.grad(l_pi, [flat])[0])
    assert float(grads[0].abs().max()) > 0.0 and torch.equal(grads[0], grads[1])
    y, logp = SH.targets(torch, pol, crit, p, cp, la, rows_of["next_obs"], rows_of["reward"], rows_of["terminated"], neps, 0.9, torch.float64)
    term = rows_of["terminated"]
    assert torch.equal(y[term], rows_of["reward"][term]) and not torch.equal(y[~term], rows_of["reward"][~term])
    # the entropy term enters y with a minus sign and the temperature
    y2, _ = SH.targets(torch, pol, crit, p, cp, la + math.log(2.0), rows_of["next_obs"], rows_of["reward"], rows_of["terminated"], neps, 0.9, torch.float64)
    assert torch.allclose((y2 - y)[~term], (-0.9 * math.exp(-0.7) * logp)[~term], rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("case", SH.CASES, ids=[str(i) for i in range(len(SH.CASES))])
def test_the_kink_filter_cap_and_the_clamp_share_hold_on_every_gpu_case(oracle_mod, case):
    """conditions of the GPU test, checked here on the float64 reference alone"""
    import torch
    b = SH.case_data(torch, oracle_mod, case)
    marked, share = int(b["mark"].sum()), SH.clamp_share(torch, b)
    print(case, "seed", b["seed"], "removed", b["removed"], "marked", marked, "of", b["n0"], "clamp share", share)
    assert b["seed"] in SH.SEEDS and SH.within_cap(case, b)
    assert b["removed"] + marked <= 0.02 * b["n0"] and (case[5] >= 100 or marked == 0)
    assert b["data"]["obs"].shape[0] >= (case[5] if case[6] != "none" else 1)
    if case[8] == "narrow":
        assert 0.02 < share < 0.9
    else:
        assert share == 0.0
    if marked:
        assert b["rows"] is not None and int((b["rows"] == -1).sum()) == marked


def test_every_draw_domain_of_the_engine_is_taken_once_and_12_13_are_this_units():
    """tests/test_dpg_update_build.py pins the DOM_* words 1, 3 .. 11; this unit's two draws take the next two free words"""
    from __graft_entry__ import CSRC
    taken = {}
    for name in sorted(os.listdir(CSRC)):
        for word in re.findall(r"constexpr uint32_t (?:(?:DOM|SAC_DRAW)_\w+ = \d+u(?:, )?)+", open(os.path.join(CSRC, name)).read()):
            for dom, value in re.findall(r"((?:DOM|SAC_DRAW)_\w+) = (\d+)u", word):
                if dom != "DOM_OPPONENT" or name == "rsx_selfplay.hip":   # (rsx_teamplay.hip repeats rsx_selfplay.hip's on purpose)
                    assert int(value) not in taken, (name, dom, value, taken[int(value)])
                    taken[int(value)] = (name, dom)
    assert set(taken) == {1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13}
    assert taken[12] == ("rsx_sac.hip", "SAC_DRAW_NEXT") and taken[13] == ("rsx_sac.hip", "SAC_DRAW_OBS")
    header = open(os.path.join(ROOT, "include", "rsx.h")).read()
    assert "domain word 12 (eps', on next_obs) and 13 (eps, on obs)" in header
