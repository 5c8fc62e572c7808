"""rsx_task_collect_selfplay as a build product and VecFusedEnv.collect(opponent=...)'s refusals (no GPU): the symbol is declared, listed
and exported, the C struct and its ctypes mirror agree, the unit is registered in the build recipe and compiles to a kernel per VSS-v0
variant without scratch memory; the Python layer refuses what it must before it touches a device; and the mirror map restated in
tests/selfplay_helpers.py is an involution."""
import os
import re
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest

import selfplay_helpers as SH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNEL = re.compile(r"task_collect_selfplay_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])E")


# ---- 1. header, binding, exports, build recipe ----
def test_symbol_is_declared_listed_and_exported():
    from build_variant import dynamic_symbols
    from rsoccer_amd import _lib
    header = open(os.path.join(ROOT, "include", "rsx.h")).read()
    decl = re.search(r"^int rsx_task_collect_selfplay\((.*?)\);", header, flags=re.M | re.S)
    assert decl, "include/rsx.h does not declare rsx_task_collect_selfplay"
    names = [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert names == ["h", "actor", "actor_params_dev", "sigma_dev", "opponent", "opponent_params_dev", "opponent_sigma_dev", "noise_seed",
                     "n_steps", "out", "sp", "stream"]
    body = re.search(r"typedef struct rsx_selfplay_out \{(.*?)\} rsx_selfplay_out;", header, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.SelfplayOut._fields_] == ["opp_obs", "opp_actions", "opp_mean", "opp_sample"]
    assert re.search(r"^#define RSX_ABI_VERSION 6\b", header, re.M)   # additive: the ABI stays 6
    defined, _ = dynamic_symbols(_lib.LIB_PATH)
    assert "rsx_task_collect_selfplay" in _lib.SYMBOLS and "rsx_task_collect_selfplay" in defined
    lib = _lib.load()
    assert len(lib.rsx_task_collect_selfplay.argtypes) == len(names)
    assert callable(_lib.Sim.task_collect_selfplay)


def test_the_unit_is_a_sibling_of_the_collector():
    from __graft_entry__ import CSRC, HIP_UNITS
    units = dict(HIP_UNITS)
    assert units["rsx_selfplay.hip"] == units["rsx_collect.hip"]
    text = open(os.path.join(CSRC, "rsx_selfplay.hip")).read()
    assert '#include "rsx_policy_mlp.hpp"' in text
    for piece in ("struct PolicyImage", "float policy_forward(", "void hidden_layer(", "float tanh_f32("):   # the MLP stays stated once
        assert piece not in text, piece
    for frag in ("rsx_step_commands.inc", "rsx_step_wire.inc", "rsx_step_xr.inc", "rsx_step_reward.inc", "rsx_step_ball_load.inc",
                 "rsx_step_vss_metrics.inc"):
        assert f'#include "{frag}"' in text, frag
    assert text.count("s_waitcnt(0x0F70)") == 1   # every load lands behind one vmcnt(0), ahead of the loop
    loop = text[text.index("for (int it = 0; it < n_steps; ++it)"):text.index("// ---- store: the state in wire format")]
    assert "bufs.obs[" not in loop and "S.params" not in loop and "sigma_dev[" not in loop   # no load inside the loop


@pytest.fixture(scope="module")
def selfplay_kernels():
    """{(kind, task, L, NR, phys): {remark: value}} of rsx_selfplay.hip, compiled with the flags build() gives it"""
    from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS
    work = tempfile.mkdtemp(prefix="rsx_selfplay_probe_")
    try:
        p = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_COMMON + dict(HIP_UNITS)["rsx_selfplay.hip"] +
                           ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(work, "rsx_selfplay.o"),
                            os.path.join(CSRC, "rsx_selfplay.hip")], stderr=subprocess.PIPE, text=True)
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


def test_code_object_holds_every_vss_variant_without_scratch(selfplay_kernels):
    from rsoccer_amd import _lib
    want = {(0, 1, L, NR, phys) for (L, NR) in ((8, 6), (16, 6), (16, 10), (8, 0), (16, 0), (32, 0)) for phys in (0, 1)}
    assert set(selfplay_kernels) == want, sorted(set(selfplay_kernels) ^ want)   # VSS-v0 only, MAX_L 32, both physics forms
    blob = open(_lib.LIB_PATH, "rb").read()
    for k, v in selfplay_kernels.items():
        assert v["name"].encode() in blob, f"librsx_hip.so lacks {v['name']}"
        assert v["ScratchSize"] == 0, (k, v)
    # the occupancy statement of the unit's header and of profiles/LABBOOK.md: static LDS + two 40-64-64-2 images at 8 lanes per env
    image = 4 * (40 * 68 + 64 + 64 * 68 + 64 + 192 + 8 + 3 * 8 * 68 + 8 * 8)
    total = selfplay_kernels[(0, 1, 8, 6, 0)]["LDS Size"] + 2 * image
    assert image == 36384 and total == 79040 and 163840 // total == 2
    for text in (open(os.path.join(ROOT, "rsoccer_amd", "csrc", "rsx_selfplay.hip")).read(),
                 open(os.path.join(ROOT, "profiles", "LABBOOK.md")).read()):
        assert "79 040 B" in text


# ---- 2. the Python layer's refusals, before any device is touched ----
def _fake_env(cls_name="VecVSSEnv", obs_dim=40, act_dim=2):
    import torch
    from rsoccer_amd import vec
    env = object.__new__(getattr(vec, cls_name))   # no handle, no device: the refusals must fire before either is needed
    env._torch = torch
    env.num_envs = 5
    env.device = torch.device("cpu")
    env.sim = types.SimpleNamespace(obs_dim=obs_dim, act_dim=act_dim)
    env._seed = 0
    return env


def test_python_refusals_fire_without_a_device():
    import torch
    from rsoccer_amd.vec.policy import MLPPolicy
    env = _fake_env()
    pol = MLPPolicy(40, 2, **SH.SHAPE_SMALL)
    opp = MLPPolicy(40, 2, **SH.SHAPE_LARGE)
    params, oparams = torch.zeros(pol.num_params), torch.zeros(opp.num_params)
    with pytest.raises(ValueError, match="opponent_params given without an opponent"):
        env.collect(pol, params, 2, opponent_params=oparams)
    with pytest.raises(ValueError, match="opponent_log_std given without an opponent"):
        env.collect(pol, params, 2, opponent_log_std=-1.0)
    with pytest.raises(ValueError, match="opponent_params must not be None"):
        env.collect(pol, params, 2, opponent=opp)
    for shape in ((opp.num_params - 1,), (1, opp.num_params), (pol.num_params,)):
        with pytest.raises(ValueError, match=r"opponent_params must be \[%d\]" % opp.num_params):
            env.collect(pol, params, 2, opponent=opp, opponent_params=torch.zeros(*shape))
    with pytest.raises(ValueError, match="opponent must be an rsoccer_amd.vec.policy.MLPPolicy"):
        env.collect(pol, params, 2, opponent="self", opponent_params=oparams)
    with pytest.raises(ValueError, match="the opponent maps 24 -> 5"):
        env.collect(pol, params, 2, opponent=MLPPolicy(24, 5), opponent_params=torch.zeros(MLPPolicy(24, 5).num_params))
    with pytest.raises(ValueError, match="opponent_log_std must be finite"):
        env.collect(pol, params, 2, opponent=opp, opponent_params=oparams, opponent_log_std=[0.0, float("nan")])
    # a non-VSS env, with policies of its own dims
    sd = _fake_env("VecSSLStaticDefendersEnv", 24, 5)
    p5 = MLPPolicy(24, 5)
    with pytest.raises(ValueError, match="VSS-v0.*VecSSLStaticDefendersEnv"):
        sd.collect(p5, torch.zeros(p5.num_params), 2, opponent=p5, opponent_params=torch.zeros(p5.num_params))


# ---- 3. the mirror map ----
@pytest.mark.parametrize("n", [3, 5])
def test_the_mirror_map_is_an_involution(n):
    rng = np.random.default_rng(7)
    obs = rng.uniform(-1.2, 1.2, (11, 4 + 12 * n)).astype(np.float32)
    sc = rng.uniform(-1.0, 1.0, (11, n, 2)).astype(np.float32)
    m, back = SH.mirror(obs, sc, n)
    assert m.dtype == np.float32 and not np.array_equal(m, obs)
    again, sc2 = SH.mirror(m, back, n)
    assert np.array_equal(again.view(np.uint32), obs.view(np.uint32)) and np.array_equal(sc2.view(np.uint32), sc.view(np.uint32))
    # the layout of include/rsx.h, 3v3: ball [0:4], own robot i at 4 + 7 i, other robot j at 25 + 5 j
    assert [SH.own(3, i) for i in range(3)] == [4, 11, 18] and [SH.other(3, j) for j in range(3)] == [25, 30, 35]
    a, b = SH.own(n, 1), SH.other(n, 1)
    assert np.array_equal(m[:, 0:4], -obs[:, 0:4])
    assert np.array_equal(m[:, a:a + 2], -obs[:, b:b + 2]) and np.array_equal(m[:, a + 4:a + 6], -obs[:, b + 2:b + 4])
    assert np.array_equal(m[:, a + 6], obs[:, b + 4]) and np.array_equal(m[:, b + 4], obs[:, a + 6])   # angular velocity: unchanged
    assert np.array_equal(m[:, a + 2:a + 4], -sc[:, 1])
