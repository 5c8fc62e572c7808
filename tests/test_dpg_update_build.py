"""The off-policy update phase (rsx_replay_sample_rows, rsx_dpg_adam_step, rsx_dpg_update_workspace, rsx_task_dpg_update) as a build
product, no GPU: the symbols are declared, listed and exported, the C structs and their ctypes mirrors agree member for member, the
unit is one of build()'s with rsx_ppo_update.hip's flags and none of its kernels uses scratch memory; and the Python layer refuses
invalid arguments with a ValueError naming the offender before anything touches a device."""
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

NEW = ("rsx_replay_sample_rows", "rsx_dpg_adam_step", "rsx_dpg_update_workspace", "rsx_task_dpg_update")
KERNELS = ("sample_rows_kernel", "dpg_grad_norm_kernel", "dpg_adam_update_kernel")


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
    from rsoccer_amd.vec.optim import DPGOptimizer
    from rsoccer_amd.vec.replay import ReplayBuffer
    for f in (VecFusedEnv.dpg_update, DPGOptimizer.step, DPGOptimizer.state_dict, DPGOptimizer.load_state_dict, ReplayBuffer.sample_rows_device,
              ReplayBuffer.sample_rows, _lib.Sim.task_dpg_update, _lib.Sim.dpg_update_workspace, _lib.replay_sample_rows, _lib.dpg_adam_step):
        assert callable(f)
    assert isinstance(DPGOptimizer.steps, property)


def test_structs_agree_with_their_ctypes_mirrors_and_the_abi_stays_6():
    from rsoccer_amd import _lib
    header = _header()
    ctype_of = {"const float*": C.c_void_p, "float*": C.c_void_p, "int64_t*": C.c_void_p, "const int64_t*": C.c_void_p, "void*": C.c_void_p,
                "double": C.c_double, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "int32_t": C.c_int32, "float": C.c_float}
    want = {"rsx_dpg_adam_cfg": ["beta1", "beta2", "lr_actor_dev", "lr_critic_dev", "lr_actor", "lr_critic", "eps", "max_grad_norm", "tau"],
            "rsx_dpg_adam_state": ["m_actor", "v_actor", "m_critic", "v_critic", "counters", "n_actor", "n_critic"],
            "rsx_dpg_adam_io": ["actor_params", "target_actor_params", "critic_params", "target_critic_params", "grad_actor", "grad_critic",
                                "stats", "workspace", "update_targets"],
            "rsx_dpg_update_cfg": ["fill_dev", "seed", "fill", "grad_steps", "policy_delay"]}
    for name, cls in (("rsx_dpg_adam_cfg", _lib.DpgAdamCfg), ("rsx_dpg_adam_state", _lib.DpgAdamState), ("rsx_dpg_adam_io", _lib.DpgAdamIo),
                      ("rsx_dpg_update_cfg", _lib.DpgUpdateCfg)):
        members = _members(header, name)
        assert [n for _, n in members] == [f[0] for f in cls._fields_] == want[name], name
        assert [ctype_of[t] for t, _ in members] == [f[1] for f in cls._fields_], name
    assert (C.sizeof(_lib.DpgAdamCfg), C.sizeof(_lib.DpgAdamState), C.sizeof(_lib.DpgAdamIo), C.sizeof(_lib.DpgUpdateCfg)) == (56, 56, 72, 32)
    for macro, value in (("RSX_DPG_ADAM_WORKSPACE_BYTES", _lib.DPG_ADAM_WORKSPACE_BYTES), ("RSX_DPG_UPDATE_STATS", len(_lib.DPG_UPDATE_STATS))):
        assert re.search(r"^#define %s %d\b" % (macro, value), header, re.M), macro
    for k, name in enumerate(_lib.DPG_COUNTERS):   # RSX_DPG_T_CRITIC, _T_ACTOR, _STEPS, _SPARE
        assert re.search(r"^#define RSX_DPG_%s\s+%d\b" % (name.upper(), k), header, re.M), name
    assert _lib.DPG_UPDATE_STATS[:9] == _lib.DPG_STATS and _lib.DPG_UPDATE_STATS[9:] == _lib.DPG_ADAM_STATS and len(_lib.DPG_UPDATE_STATS) == 12
    assert re.search(r"^#define RSX_ABI_VERSION 6\b", header, re.M)
    # the header states the row draw's domain word, and no other draw of the engine uses it
    assert "counter = (t >> 2, step >> 32, step & 0xFFFFFFFF, 11)" in header


def test_the_unit_is_one_of_build_with_the_flags_of_the_ppo_update_unit_and_restates_no_philox():
    from __graft_entry__ import CSRC, HIP_UNITS
    units_of = dict(HIP_UNITS)
    assert "rsx_dpg_update.hip" in units_of and units_of["rsx_dpg_update.hip"] == units_of["rsx_ppo_update.hip"]
    text = open(os.path.join(CSRC, "rsx_dpg_update.hip")).read()
    assert '#include "rsx_math.hpp"' in text and "philox4x32(uint32_t" not in text
    assert "launch_dpg_gradient(" in text and "dpg_critic_kernel" not in text   # (called, not restated)
    assert "atomic" not in text.replace("uses an atomic", "")
    assert "DOM_ROWS = 11u" in text
    taken = set()
    for name in os.listdir(CSRC):   # every Philox domain word of the engine is defined once
        for word in re.findall(r"constexpr uint32_t (?:DOM_\w+ = \d+u(?:, )?)+", open(os.path.join(CSRC, name)).read()):
            for dom, value in re.findall(r"(DOM_\w+) = (\d+)u", word):
                if dom != "DOM_OPPONENT" or name == "rsx_selfplay.hip":   # (rsx_teamplay.hip repeats rsx_selfplay.hip's on purpose)
                    assert int(value) not in taken, (name, dom, value)
                    taken.add(int(value))
    assert taken == {1, 3, 4, 5, 6, 7, 8, 9, 10, 11}
    units = open(os.path.join(CSRC, "rsx_units.hpp")).read()
    for fn in ("void launch_replay_sample_rows(", "void launch_dpg_adam_step(", "void launch_dpg_update(", "long long dpg_update_workspace_bytes("):
        assert fn in units, fn


def test_no_kernel_uses_scratch_memory():
    """compiled with the flags build() gives the unit; the compiler's kernel-resource-usage remarks, read the way
    tests/test_ppo_update_build.py reads them"""
    from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS
    work = tempfile.mkdtemp(prefix="rsx_dpg_update_probe_")
    try:
        p = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_COMMON + dict(HIP_UNITS)["rsx_dpg_update.hip"] +
                           ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(work, "rsx_dpg_update.o"),
                            os.path.join(CSRC, "rsx_dpg_update.hip")], stderr=subprocess.PIPE, text=True)
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
    assert len(rows) == len(KERNELS), sorted(rows)


# ---- the Python layer's refusals that need no device ----
def _nets():
    from rsoccer_amd.vec.policy import MLPPolicy, MLPQCritic
    return (MLPPolicy(40, 2, hidden=64, layers=2, hidden_act="tanh", out_act="clip"),
            MLPQCritic(40, 2, hidden=64, layers=2, hidden_act="tanh"))


@pytest.mark.parametrize("kw,word", [
    (dict(lr_actor=float("nan")), "lr_actor"), (dict(lr_critic=float("inf")), "lr_critic"), (dict(lr_critic=-1e-3), "lr_critic"),
    (dict(betas=(1.0, 0.999)), "betas[0]"), (dict(betas=(0.9, float("nan"))), "betas[1]"), (dict(betas=(0.9,)), "betas"),
    (dict(eps=float("nan")), "eps"), (dict(eps=-1e-8), "eps"),
    (dict(max_grad_norm=float("nan")), "max_grad_norm"), (dict(max_grad_norm=float("inf")), "max_grad_norm"),
    (dict(tau=-0.01), "tau"), (dict(tau=1.01), "tau"), (dict(tau=float("nan")), "tau"),
    (dict(n_critics=3), "n_critics"), (dict(n_critics=0), "n_critics"),
])
def test_the_optimiser_refuses_invalid_hyper_parameters_before_it_allocates(kw, word):
    from rsoccer_amd.vec.optim import DPGOptimizer
    pol, critic = _nets()
    kw = {"n_critics": 2, **kw}
    with pytest.raises(ValueError, match=re.escape(word)):
        DPGOptimizer(pol, critic, device=0, **kw)


def test_the_optimiser_refuses_networks_of_the_wrong_kind():
    from rsoccer_amd.vec.optim import DPGOptimizer
    from rsoccer_amd.vec.policy import MLPCritic
    pol, critic = _nets()
    with pytest.raises(ValueError, match="policy"):
        DPGOptimizer(critic, critic, 2)
    with pytest.raises(ValueError, match="critic"):
        DPGOptimizer(pol, pol, 2)
    with pytest.raises(ValueError, match="critic"):
        DPGOptimizer(pol, MLPCritic(40, hidden=64, layers=2, hidden_act="tanh"), 2)


def test_the_device_row_draw_refuses_bad_arguments_by_name_and_the_torch_one_is_untouched():
    import torch
    from rsoccer_amd.vec.replay import ReplayBuffer
    buf = ReplayBuffer(16, 4, 2, "cpu")
    with pytest.raises(ValueError, match="m must be"):
        buf.sample_rows_device(0)
    with pytest.raises(ValueError, match="m must be"):
        buf.sample_rows_device(2 ** 31)
    with pytest.raises(ValueError, match="GPU"):
        buf.sample_rows_device(4)
    assert torch.equal(buf.sample_rows(5), torch.full((5,), -1, dtype=torch.int32))   # (an empty ring, as before)
    assert "fill" not in buf.data()


def test_dpg_update_refuses_bad_arguments_by_name_before_it_touches_the_env():
    """the checks that come before the first use of the env's handle or device, on an object that has neither"""
    from rsoccer_amd.vec.fused import VecFusedEnv
    from rsoccer_amd.vec.optim import DPGOptimizer
    pol, critic = _nets()
    env = object.__new__(VecFusedEnv)
    import torch
    env._torch = torch
    with pytest.raises(ValueError, match="opt must be"):
        VecFusedEnv.dpg_update(env, {}, pol, None, None, critic, None, None, object())
    opt = object.__new__(DPGOptimizer)
    with pytest.raises(ValueError, match="policy"):
        VecFusedEnv.dpg_update(env, {}, critic, None, None, critic, None, None, opt)
    with pytest.raises(ValueError, match="critic"):
        VecFusedEnv.dpg_update(env, {}, pol, None, None, pol, None, None, opt)
