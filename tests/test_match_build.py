"""rsx_task_lookahead_match as a build product, VecFusedEnv.lookahead_match()'s refusals and rsoccer_amd.vec.policy.match_table (no
GPU): the symbol is declared, listed and exported, the C struct and its ctypes mirror agree, the unit is registered in the build recipe
with rsx_policy.hip's flags and compiles to a kernel per VSS-v0 variant without scratch memory and within self-play's LDS; the Python
layer refuses what it must before it touches a device; and match_table folds a hand-made result."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

import selfplay_helpers as SH
import test_selfplay_build as SB   # _fake_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNEL = re.compile(r"task_lookahead_match_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])E")
FIELDS = ["returns", "steps", "flags", "result", "last_obs", "actions", "obs", "opp_actions", "opp_obs"]


# ---- 1. header, binding, exports, build recipe ----
def test_symbol_is_declared_listed_and_exported():
    import ctypes
    from build_variant import dynamic_symbols
    from rsoccer_amd import _lib
    header = open(os.path.join(ROOT, "include", "rsx.h")).read()
    decl = re.search(r"^int rsx_task_lookahead_match\((.*?)\);", header, flags=re.M | re.S)
    assert decl, "include/rsx.h does not declare rsx_task_lookahead_match"
    names = [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert names == ["h", "actor", "actor_params_dev", "n_actors", "actor_seats", "opponent", "opponent_params_dev", "n_opponents",
                     "opponent_seats", "horizon", "gamma", "out", "stream"]
    body = re.search(r"typedef struct rsx_match_out \{(.*?)\} rsx_match_out;", header, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.MatchOut._fields_] == FIELDS
    assert ctypes.sizeof(_lib.MatchOut) == len(FIELDS) * ctypes.sizeof(ctypes.c_void_p)
    assert re.search(r"^#define RSX_ABI_VERSION 6\b", header, re.M)   # additive: the ABI stays 6
    defined, _ = dynamic_symbols(_lib.LIB_PATH)
    assert "rsx_task_lookahead_match" in _lib.SYMBOLS and "rsx_task_lookahead_match" in defined
    lib = _lib.load()
    assert len(lib.rsx_task_lookahead_match.argtypes) == len(names)
    assert callable(_lib.Sim.task_lookahead_match)


def test_the_unit_is_a_sibling_of_the_policy_lookahead():
    from __graft_entry__ import CSRC, HIP_UNITS
    units = dict(HIP_UNITS)
    assert units["rsx_match.hip"] == units["rsx_policy.hip"]
    text = open(os.path.join(CSRC, "rsx_match.hip")).read()
    assert '#include "rsx_policy_mlp.hpp"' in text and '#include "rsx_seats.hpp"' in text
    for piece in ("struct PolicyImage", "float policy_forward(", "void hidden_layer(", "float tanh_f32(", "PolicyImage policy_image("):
        assert piece not in text, piece   # the MLP stays stated once
    for piece in ("void write_obs_mirrored(", "int seat_ix(", "void exchange_own("):   # ... and the unit takes the seat helpers from the header
        assert piece not in text and piece in open(os.path.join(CSRC, "rsx_seats.hpp")).read(), piece
    for frag in ("rsx_step_commands.inc", "rsx_step_wire.inc", "rsx_step_xr.inc"):
        assert f'#include "{frag}"' in text, frag
    assert text.count("s_waitcnt(0x0F70)") == 1   # every load lands behind one vmcnt(0), ahead of the loop
    loop = text[text.index("for (int it = 0; it < horizon; ++it)"):text.index("if (live && b == N) {")]
    for load in ("Q.obs[", ".params", "load_raw", "load_coefs", "stage_policy", "auxe(", "A.ticks["):
        assert load not in loop, load   # no load inside the loop
    assert text.index("s_waitcnt(0x0F70)") < text.index("for (int it = 0; it < horizon; ++it)")
    # the seats are a run-time loop: one inlined forward per hidden width, not one per seat
    assert "#pragma nounroll\n        for (int j = 0; j < SA + SO; ++j)" in text
    assert loop.count("policy_forward<64") == 1 and loop.count("policy_forward<32") == 1
    # the handle is read only: the state, the scalar arena and the obs buffer arrive as pointers to const
    assert "store_body" not in text and "bufs." not in text


@pytest.fixture(scope="module")
def match_kernels():
    """{(kind, task, L, NR, phys): {remark: value}} of rsx_match.hip, compiled with the flags build() gives it"""
    from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS
    work = tempfile.mkdtemp(prefix="rsx_match_probe_")
    try:
        p = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_COMMON + dict(HIP_UNITS)["rsx_match.hip"] +
                           ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(work, "rsx_match.o"),
                            os.path.join(CSRC, "rsx_match.hip")], stderr=subprocess.PIPE, text=True)
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


def test_code_object_holds_every_vss_variant_without_scratch(match_kernels):
    from rsoccer_amd import _lib
    # the set of (L, NR, phys) of the self-play unit (tests/test_selfplay_build.py)
    want = {(0, 1, L, NR, phys) for (L, NR) in ((8, 6), (16, 6), (16, 10), (8, 0), (16, 0), (32, 0)) for phys in (0, 1)}
    assert set(match_kernels) == want, sorted(set(match_kernels) ^ want)   # VSS-v0 only, MAX_L 32, both physics forms
    blob = open(_lib.LIB_PATH, "rb").read()
    for k, v in match_kernels.items():
        assert v["name"].encode() in blob, f"librsx_hip.so lacks {v['name']}"
        assert v["ScratchSize"] == 0, (k, v)
    # the occupancy statement of the unit's header and of profiles/LABBOOK.md: static LDS + two 40-64-64-2 images at 8 lanes per env
    # with an action slot of max(8, round4(2 * 3)) = 8 floats per env — two workgroups per CU need at most 81 920 B
    pitch = max(8, (2 * 3 + 3) & ~3)
    image = 4 * (40 * 68 + 64 + 64 * 68 + 64 + 192 + 8 + 3 * 8 * 68 + 8 * pitch)
    total = match_kernels[(0, 1, 8, 6, 0)]["LDS Size"] + 2 * image
    assert image == 36384 and total == 79040 and 163840 // total == 2
    for text in (open(os.path.join(ROOT, "rsoccer_amd", "csrc", "rsx_match.hip")).read(),
                 open(os.path.join(ROOT, "profiles", "LABBOOK.md")).read().split("Matches", 1)[-1]):
        assert "79 040 B" in text


# ---- 2. the Python layer's refusals, before any device is touched ----
def test_python_refusals_fire_without_a_device():
    import numpy as np
    import torch
    from rsoccer_amd.vec.policy import MLPPolicy
    env = SB._fake_env()
    pol = MLPPolicy(40, 2, **SH.SHAPE_SMALL)
    opp = MLPPolicy(40, 2, **SH.SHAPE_LARGE)
    P, P2 = pol.num_params, opp.num_params
    params, oparams = torch.zeros(2, P), torch.zeros(3, P2)
    with pytest.raises(ValueError, match="policy must be an rsoccer_amd.vec.policy.MLPPolicy"):
        env.lookahead_match("me", params, opp, oparams, 4)
    with pytest.raises(ValueError, match="opponent must be an rsoccer_amd.vec.policy.MLPPolicy"):
        env.lookahead_match(pol, params, "self", oparams, 4)
    with pytest.raises(ValueError, match="opponent must be an rsoccer_amd.vec.policy.MLPPolicy"):
        env.lookahead_match(pol, params, None, oparams, 4)
    # a 1-D tensor is NOT promoted: refused with the shape in the message
    with pytest.raises(ValueError, match=r"params must be \[K >= 1, %d\], got \(%d,\)" % (P, P)):
        env.lookahead_match(pol, torch.zeros(P), opp, oparams, 4)
    with pytest.raises(ValueError, match=r"opponent_params must be \[M >= 1, %d\], got \(%d,\)" % (P2, P2)):
        env.lookahead_match(pol, params, opp, torch.zeros(P2), 4)
    for shape in ((2, P - 1), (0, P), (1, 2, P), (2, P2)):
        with pytest.raises(ValueError, match=r"params must be \[K >= 1, %d\]" % P):
            env.lookahead_match(pol, torch.zeros(*shape), opp, oparams, 4)
    for shape in ((3, P2 + 1), (0, P2), (1, 3, P2), (3, P)):
        with pytest.raises(ValueError, match=r"opponent_params must be \[M >= 1, %d\]" % P2):
            env.lookahead_match(pol, params, opp, np.zeros(shape, dtype=np.float32), 4, team=True, opponent_team=True)
    with pytest.raises(ValueError, match="params and opponent_params must not be None"):
        env.lookahead_match(pol, params, opp, None, 4)
    with pytest.raises(ValueError, match="horizon must be >= 1, got 0"):
        env.lookahead_match(pol, params, opp, oparams, 0)
    for gamma in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gamma must be finite"):
            env.lookahead_match(pol, params, opp, oparams, 4, gamma=gamma)
    with pytest.raises(ValueError, match="the policy maps 24 -> 5"):
        env.lookahead_match(MLPPolicy(24, 5), params, opp, oparams, 4)
    with pytest.raises(ValueError, match="the opponent maps 24 -> 5"):
        env.lookahead_match(pol, params, MLPPolicy(24, 5), oparams, 4)
    # a non-VSS env, with policies of its own dims
    sd = SB._fake_env("VecSSLStaticDefendersEnv", 24, 5)
    p5 = MLPPolicy(24, 5)
    with pytest.raises(ValueError, match="lookahead_match: .*VSS-v0.*VecSSLStaticDefendersEnv"):
        sd.lookahead_match(p5, torch.zeros(1, p5.num_params), p5, torch.zeros(1, p5.num_params), 4)
    # unequal teams
    lop = SB._fake_env()
    lop.N_YELLOW = 2
    with pytest.raises(ValueError, match="lookahead_match: .*equal teams.*VecVSSEnv"):
        lop.lookahead_match(pol, params, opp, oparams, 4)


# ---- 3. match_table ----
def test_match_table_folds_the_envs():
    import torch
    from rsoccer_amd.vec.policy import match_table
    # B = 4 envs, K = 2 actors, M = 3 opponents
    result = torch.tensor([[[1, 0, -1], [1, 1, 1]],
                           [[1, 0, -1], [0, -1, 1]],
                           [[-1, 0, -1], [0, -1, 1]],
                           [[0, 0, 1], [0, 0, 1]]], dtype=torch.int8)
    ret = torch.arange(24, dtype=torch.float32).reshape(4, 2, 3)
    t = match_table({"result": result, "return": ret, "steps": None})
    assert set(t) == {"wins", "draws", "losses", "mean_return"}
    assert t["wins"].tolist() == [[2, 0, 1], [1, 1, 4]]
    assert t["losses"].tolist() == [[1, 0, 3], [0, 2, 0]]
    assert t["draws"].tolist() == [[1, 4, 0], [3, 1, 0]]
    assert torch.equal(t["wins"] + t["draws"] + t["losses"], torch.full((2, 3), 4))
    assert t["mean_return"].dtype == torch.float32 and torch.equal(t["mean_return"], ret.mean(0))
    assert t["mean_return"].tolist() == [[9.0, 10.0, 11.0], [12.0, 13.0, 14.0]]
    with pytest.raises(ValueError, match="lacks 'result'"):
        match_table({"return": ret})
    with pytest.raises(ValueError, match=r"\[B, K, M\]"):
        match_table({"result": result[0], "return": ret[0]})
