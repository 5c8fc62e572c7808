"""The update phase (rsx_ppo_normalize, rsx_ppo_permutation, rsx_adam_step, rsx_adam_mark, rsx_task_ppo_update) as a build product, no
GPU: the symbols are declared, listed and exported, the C structs and their ctypes mirrors agree field for field, the unit is one of
build()'s and none of its kernels uses scratch memory; and the Python layer refuses invalid arguments with a ValueError naming the
offender before anything touches a device."""
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

NEW = ("rsx_ppo_normalize", "rsx_ppo_permutation", "rsx_adam_step", "rsx_adam_mark", "rsx_ppo_update_workspace", "rsx_task_ppo_update")
KERNELS = ("adv_moments_kernel", "adv_normalize_kernel", "permutation_kernel", "grad_norm_kernel", "adam_update_kernel", "update_mark_kernel")


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
    from rsoccer_amd.vec.optim import PPOOptimizer
    for f in (VecFusedEnv.normalize_advantages, VecFusedEnv.minibatch_rows, VecFusedEnv.ppo_update, PPOOptimizer.step,
              PPOOptimizer.state_dict, PPOOptimizer.load_state_dict, _lib.Sim.task_ppo_update, _lib.Sim.ppo_update_workspace,
              _lib.ppo_normalize, _lib.ppo_permutation, _lib.adam_step, _lib.adam_mark):
        assert callable(f)


def test_structs_agree_with_their_ctypes_mirrors_and_the_abi_stays_6():
    from rsoccer_amd import _lib
    header = _header()
    ctype_of = {"const float*": C.c_void_p, "float*": C.c_void_p, "int64_t*": C.c_void_p, "void*": C.c_void_p, "double": C.c_double,
                "int64_t": C.c_int64, "uint64_t": C.c_uint64, "int32_t": C.c_int32, "float": C.c_float}
    want = {"rsx_adam_cfg": ["beta1", "beta2", "lr_dev", "lr", "eps", "max_grad_norm", "target_kl"],
            "rsx_adam_state": ["m_actor", "v_actor", "m_log_std", "v_log_std", "m_critic", "v_critic", "counters", "n_actor", "n_log_std",
                               "n_critic"],
            "rsx_adam_io": ["actor_params", "log_std", "critic_params", "grad_actor", "grad_log_std", "grad_critic", "approx_kl", "stats",
                            "workspace"],
            "rsx_ppo_update_cfg": ["seed", "epochs", "minibatches", "normalize_advantage", "norm_eps"]}
    for name, cls in (("rsx_adam_cfg", _lib.AdamCfg), ("rsx_adam_state", _lib.AdamState), ("rsx_adam_io", _lib.AdamIo),
                      ("rsx_ppo_update_cfg", _lib.PpoUpdateCfg)):
        members = _members(header, name)
        assert [n for _, n in members] == [f[0] for f in cls._fields_] == want[name], name
        assert [ctype_of[t] for t, _ in members] == [f[1] for f in cls._fields_], name
    assert C.sizeof(_lib.AdamCfg) == 40 and C.sizeof(_lib.AdamState) == 80 and C.sizeof(_lib.AdamIo) == 72 and C.sizeof(_lib.PpoUpdateCfg) == 24
    for macro, value in (("RSX_PPO_NORMALIZE_WORKSPACE_BYTES", _lib.PPO_NORMALIZE_WORKSPACE_BYTES),
                         ("RSX_ADAM_WORKSPACE_BYTES", _lib.ADAM_WORKSPACE_BYTES), ("RSX_PPO_UPDATE_STATS", len(_lib.PPO_UPDATE_STATS))):
        assert re.search(r"^#define %s %d\b" % (macro, value), header, re.M), macro
    for k, name in enumerate(_lib.ADAM_COUNTERS):   # RSX_ADAM_T, _UPDATES, _APPLIED, _STOPPED
        assert re.search(r"^#define RSX_ADAM_%s\s+%d\b" % (name.upper(), k), header, re.M), name
    assert _lib.PPO_UPDATE_STATS[:8] == _lib.PPO_STATS and _lib.PPO_UPDATE_STATS[8:] == ("grad_norm", "applied")
    assert re.search(r"^#define RSX_ABI_VERSION 6\b", header, re.M)


def test_the_unit_is_one_of_build_and_leaves_the_gradient_unit_alone():
    from __graft_entry__ import CSRC, HIP_UNITS
    assert "rsx_ppo_update.hip" in dict(HIP_UNITS)
    text = open(os.path.join(CSRC, "rsx_ppo_update.hip")).read()
    assert "launch_ppo_gradient(" in text and "mlp_grad_kernel" not in text   # (called, not restated)
    assert "atomic" not in text.replace("uses an atomic", "")
    units = open(os.path.join(CSRC, "rsx_units.hpp")).read()
    for fn in ("void launch_ppo_normalize(", "void launch_ppo_permutation(", "void launch_adam_step(", "void launch_ppo_update("):
        assert fn in units, fn


def test_no_kernel_uses_scratch_memory():
    """compiled with the flags build() gives the unit; the compiler's kernel-resource-usage remarks, read the way
    tests/test_ppo_build.py reads them"""
    from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS
    work = tempfile.mkdtemp(prefix="rsx_ppo_update_probe_")
    try:
        p = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_COMMON + dict(HIP_UNITS)["rsx_ppo_update.hip"] +
                           ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(work, "rsx_ppo_update.o"),
                            os.path.join(CSRC, "rsx_ppo_update.hip")], stderr=subprocess.PIPE, text=True)
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
        print(kernel, {n: v.get(n) for n in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "Occupancy")})
        assert v["ScratchSize"] == 0, (kernel, v)
    assert len(rows) == len(KERNELS), sorted(rows)


# ---- the Python layer's refusals that need no device ----
def _nets():
    from rsoccer_amd.vec.policy import MLPCritic, MLPPolicy
    return MLPPolicy(40, 2, hidden=64, layers=2, hidden_act="tanh", out_act="clip"), MLPCritic(40, hidden=64, layers=2, hidden_act="tanh")


@pytest.mark.parametrize("kw,word", [
    (dict(lr=float("nan")), "lr"), (dict(lr=float("inf")), "lr"), (dict(lr=-1e-3), "lr"),
    (dict(betas=(1.0, 0.999)), "betas[0]"), (dict(betas=(0.9, -0.1)), "betas[1]"), (dict(betas=(0.9, float("nan"))), "betas[1]"),
    (dict(betas=(0.9,)), "betas"),
    (dict(eps=float("nan")), "eps"), (dict(eps=-1e-8), "eps"),
    (dict(max_grad_norm=float("nan")), "max_grad_norm"), (dict(max_grad_norm=float("inf")), "max_grad_norm"),
])
def test_the_optimiser_refuses_invalid_hyper_parameters_before_it_allocates(kw, word):
    from rsoccer_amd.vec.optim import PPOOptimizer
    pol, critic = _nets()
    with pytest.raises(ValueError, match=re.escape(word)):
        PPOOptimizer(pol, critic, device=0, **kw)


def test_the_optimiser_refuses_networks_of_the_wrong_kind():
    from rsoccer_amd.vec.optim import PPOOptimizer
    pol, critic = _nets()
    with pytest.raises(ValueError, match="policy"):
        PPOOptimizer(critic, critic)
    with pytest.raises(ValueError, match="critic"):
        PPOOptimizer(pol, pol)


@pytest.mark.parametrize("value", [float("nan"), float("inf"), 0.0, -0.01])
def test_target_kl_must_be_finite_and_positive(value):
    from rsoccer_amd.vec.optim import check_target_kl
    assert check_target_kl(None) == 0.0 and check_target_kl(0.02) == 0.02
    with pytest.raises(ValueError, match="target_kl"):
        check_target_kl(value)


def test_chunks_are_torch_chunks_and_an_empty_last_chunk_is_refused():
    import torch
    from rsoccer_amd.vec.fused import VecFusedEnv
    for n in (1, 2, 5, 64, 65, 1025, 4097):
        for mb in (1, 2, 3, 4, 7, 64):
            sizes = [len(c) for c in torch.arange(n).chunk(mb)]
            if len(sizes) != mb:   # torch returns fewer chunks exactly where the last of `mb` would be empty
                with pytest.raises(ValueError, match="minibatches"):
                    VecFusedEnv.minibatch_chunks(n, mb)
                continue
            got = VecFusedEnv.minibatch_chunks(n, mb)
            assert [hi - lo for lo, hi in got] == sizes and got[0][0] == 0 and got[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(got, got[1:]))
    with pytest.raises(ValueError, match="minibatches"):
        VecFusedEnv.minibatch_chunks(10, 0)
    with pytest.raises(ValueError, match="n must be"):
        VecFusedEnv.minibatch_chunks(0, 1)
