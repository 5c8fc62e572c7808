"""The soft actor-critic update phase (rsx_sac_adam_step, rsx_sac_update_workspace, rsx_task_sac_update) as a build product, no GPU:
the symbols are declared, listed and exported, the C structs and their ctypes mirrors agree member for member, the unit is one of
build()'s with rsx_dpg_update.hip's flags, calls the row draw and the gradient launch without restating either, and compiles to exactly
two kernels without scratch memory; and the Python layer refuses invalid arguments with a ValueError naming the offender before anything
touches a device."""
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

NEW = ("rsx_sac_adam_step", "rsx_sac_update_workspace", "rsx_task_sac_update")
KERNELS = ("sac_grad_norm_kernel", "sac_adam_update_kernel")
UNIT = "rsx_sac_update.hip"


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
    defined, _ = dynamic_symbols(_lib.LIB_PATH)
    for sym in NEW:
        assert re.search(r"^int %s\(" % sym, header, re.M), sym
        assert sym in _lib.SYMBOLS and sym in defined, sym
    from rsoccer_amd.vec.fused import VecFusedEnv
    from rsoccer_amd.vec.optim import SACOptimizer
    for f in (VecFusedEnv.sac_update, SACOptimizer.step, SACOptimizer.state_dict, SACOptimizer.load_state_dict, _lib.Sim.task_sac_update,
              _lib.Sim.sac_update_workspace, _lib.sac_adam_step):
        assert callable(f)
    assert isinstance(SACOptimizer.steps, property)


def test_structs_agree_with_their_ctypes_mirrors_and_the_abi_stays_6():
    from rsoccer_amd import _lib
    header = _header()
    ctype_of = {"const float*": C.c_void_p, "float*": C.c_void_p, "int64_t*": C.c_void_p, "const int64_t*": C.c_void_p, "void*": C.c_void_p,
                "double": C.c_double, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "int32_t": C.c_int32, "float": C.c_float}
    want = {"rsx_sac_adam_cfg": ["beta1", "beta2", "lr_actor_dev", "lr_critic_dev", "lr_alpha_dev", "lr_actor", "lr_critic", "lr_alpha", "eps",
                                 "max_grad_norm", "tau"],
            "rsx_sac_adam_state": ["m_actor", "v_actor", "m_critic", "v_critic", "m_alpha", "v_alpha", "counters", "n_actor", "n_critic"],
            "rsx_sac_adam_io": ["actor_params", "critic_params", "target_critic_params", "log_alpha", "grad_actor", "grad_critic",
                                "grad_log_alpha", "stats", "workspace", "update_targets"],
            "rsx_sac_update_cfg": ["fill_dev", "seed", "fill", "grad_steps", "learn_alpha"]}
    for name, cls in (("rsx_sac_adam_cfg", _lib.SacAdamCfg), ("rsx_sac_adam_state", _lib.SacAdamState), ("rsx_sac_adam_io", _lib.SacAdamIo),
                      ("rsx_sac_update_cfg", _lib.SacUpdateCfg)):
        members = _members(header, name)
        assert [n for _, n in members] == [f[0] for f in cls._fields_] == want[name], name
        assert [ctype_of[t] for t, _ in members] == [f[1] for f in cls._fields_], name
        assert "target_actor" not in " ".join(n for _, n in members)   # there is no target actor
    assert (C.sizeof(_lib.SacAdamCfg), C.sizeof(_lib.SacAdamState), C.sizeof(_lib.SacAdamIo), C.sizeof(_lib.SacUpdateCfg)) == (64, 72, 80, 32)
    for macro, value in (("RSX_SAC_ADAM_WORKSPACE_BYTES", _lib.SAC_ADAM_WORKSPACE_BYTES), ("RSX_SAC_UPDATE_STATS", len(_lib.SAC_UPDATE_STATS))):
        assert re.search(r"^#define %s %d\b" % (macro, value), header, re.M), macro
    assert _lib.SAC_COUNTERS == ("t_critic", "t_actor", "t_alpha", "steps")
    for k, name in enumerate(_lib.SAC_COUNTERS):   # RSX_SAC_T_CRITIC, _T_ACTOR, _T_ALPHA, _STEPS
        assert re.search(r"^#define RSX_SAC_%s\s+%d\b" % (name.upper(), k), header, re.M), name
    assert _lib.SAC_UPDATE_STATS[:12] == _lib.SAC_STATS and _lib.SAC_UPDATE_STATS[12:] == _lib.SAC_ADAM_STATS and len(_lib.SAC_UPDATE_STATS) == 16
    assert _lib.SAC_ADAM_STATS == ("grad_norm_critic", "grad_norm_actor", "log_alpha", "targets_moved")
    assert re.search(r"^#define RSX_ABI_VERSION 6\b", header, re.M)


def test_the_unit_is_one_of_build_with_the_flags_of_the_dpg_update_unit_and_restates_neither_launch():
    from __graft_entry__ import CSRC, HIP_UNITS
    units_of = dict(HIP_UNITS)
    assert UNIT in units_of and units_of[UNIT] == units_of["rsx_dpg_update.hip"] == units_of["rsx_ppo_update.hip"] == []
    text = open(os.path.join(CSRC, UNIT)).read()
    code = re.sub(r"//[^\n]*", "", text)   # (the comments may speak of what the code must not hold)
    # called, not restated: the row draw is rsx_dpg_update.hip's, the gradients are rsx_sac.hip's
    assert "launch_replay_sample_rows(" in code and "sample_rows_kernel" not in code
    assert "launch_sac_gradient(" in code and not re.search(r"sac_(target|critic|sample|qa|actor|reduce)_kernel", code)
    assert len(re.findall(r"__global__", code)) == 2
    # no Philox, no atomic, no domain word
    assert "philox" not in code.lower() and "rsx_math.hpp" not in code
    assert "atomic" not in code.lower()
    assert not re.search(r"\b(DOM_|SAC_DRAW_)\w*", code)
    units = open(os.path.join(CSRC, "rsx_units.hpp")).read()
    for fn in ("void launch_sac_adam_step(", "void launch_sac_update(", "long long sac_update_workspace_bytes("):
        assert fn in units, fn
    api = open(os.path.join(CSRC, "rsx_api_task.hip")).read()
    assert api.index("int rsx_task_dpg_update(") < api.index("int rsx_sac_adam_step(") < api.index("int rsx_task_sac_update(")
    # rsx_dpg_update.hip keeps its three kernels: this phase's live here
    assert len(re.findall(r"__global__", open(os.path.join(CSRC, "rsx_dpg_update.hip")).read())) == 3


def test_exactly_two_kernels_and_neither_uses_scratch_memory():
    """compiled with the flags build() gives the unit; the compiler's kernel-resource-usage remarks, read the way
    tests/test_dpg_update_build.py reads them"""
    from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS
    work = tempfile.mkdtemp(prefix="rsx_sac_update_probe_")
    try:
        p = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_COMMON + dict(HIP_UNITS)[UNIT] +
                           ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(work, "rsx_sac_update.o"),
                            os.path.join(CSRC, UNIT)], stderr=subprocess.PIPE, text=True)
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
    for kernel in KERNELS:
        hits = [k for k in rows if kernel in k]
        assert len(hits) == 1, (kernel, sorted(rows))
        v = rows[hits[0]]
        print(kernel, {n: v.get(n) for n in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "Occupancy", "LDS Size")})
        assert v["ScratchSize"] == 0, (kernel, v)
    assert len(rows) == len(KERNELS) == 2, sorted(rows)


# ---- the Python layer's refusals that need no device ----
def _nets():
    from rsoccer_amd.vec.policy import MLPGaussianPolicy, MLPQCritic
    return (MLPGaussianPolicy(40, 2, hidden=64, layers=2, hidden_act="tanh"), MLPQCritic(40, 2, hidden=64, layers=2, hidden_act="tanh"))


@pytest.mark.parametrize("kw,word", [
    (dict(lr_actor=float("nan")), "lr_actor"), (dict(lr_critic=float("inf")), "lr_critic"), (dict(lr_critic=-1e-3), "lr_critic"),
    (dict(lr_alpha=float("nan")), "lr_alpha"), (dict(lr_alpha=-1e-3), "lr_alpha"), (dict(lr_alpha=float("inf")), "lr_alpha"),
    (dict(betas=(1.0, 0.999)), "betas[0]"), (dict(betas=(0.9, float("nan"))), "betas[1]"), (dict(betas=(0.9,)), "betas"),
    (dict(eps=float("nan")), "eps"), (dict(eps=-1e-8), "eps"),
    (dict(max_grad_norm=float("nan")), "max_grad_norm"), (dict(max_grad_norm=float("inf")), "max_grad_norm"),
    (dict(tau=-0.01), "tau"), (dict(tau=1.01), "tau"), (dict(tau=float("nan")), "tau"),
    (dict(n_critics=3), "n_critics"), (dict(n_critics=0), "n_critics"),
])
def test_the_optimiser_refuses_invalid_hyper_parameters_before_it_allocates(kw, word):
    from rsoccer_amd.vec.optim import SACOptimizer
    pol, critic = _nets()
    kw = {"n_critics": 2, **kw}
    with pytest.raises(ValueError, match=re.escape(word)):
        SACOptimizer(pol, critic, device=0, **kw)


def test_the_optimiser_refuses_networks_of_the_wrong_kind():
    from rsoccer_amd.vec.optim import SACOptimizer
    from rsoccer_amd.vec.policy import MLPCritic, MLPPolicy
    pol, critic = _nets()
    with pytest.raises(ValueError, match="policy"):
        SACOptimizer(critic, critic, 2)
    with pytest.raises(ValueError, match="MLPGaussianPolicy"):   # TD3's deterministic actor is not SAC's
        SACOptimizer(MLPPolicy(40, 2, hidden=64, layers=2, hidden_act="tanh", out_act="tanh"), critic, 2)
    with pytest.raises(ValueError, match="critic"):
        SACOptimizer(pol, pol, 2)
    with pytest.raises(ValueError, match="critic"):
        SACOptimizer(pol, MLPCritic(40, hidden=64, layers=2, hidden_act="tanh"), 2)


def test_sac_update_refuses_bad_arguments_by_name_before_it_touches_the_env():
    """the checks that come before the first use of the env's handle or device, on an object that has neither"""
    import torch
    from rsoccer_amd.vec.fused import VecFusedEnv
    from rsoccer_amd.vec.optim import DPGOptimizer, SACOptimizer
    from rsoccer_amd.vec.policy import MLPPolicy
    pol, critic = _nets()
    env = object.__new__(VecFusedEnv)
    env._torch = torch
    with pytest.raises(ValueError, match="opt must be"):
        VecFusedEnv.sac_update(env, {}, pol, None, critic, None, None, None, object())
    with pytest.raises(ValueError, match="SACOptimizer"):
        VecFusedEnv.sac_update(env, {}, pol, None, critic, None, None, None, object.__new__(DPGOptimizer))
    opt = object.__new__(SACOptimizer)
    with pytest.raises(ValueError, match="policy"):
        VecFusedEnv.sac_update(env, {}, critic, None, critic, None, None, None, opt)
    with pytest.raises(ValueError, match="MLPGaussianPolicy"):
        VecFusedEnv.sac_update(env, {}, MLPPolicy(40, 2, hidden=64, layers=2, hidden_act="tanh", out_act="tanh"), None, critic, None, None,
                               None, opt)
    with pytest.raises(ValueError, match="critic"):
        VecFusedEnv.sac_update(env, {}, pol, None, pol, None, None, None, opt)
