"""rsx_task_collect_team as a build product, VecFusedEnv.collect(team=..., opponent_team=...)'s refusals and
rsoccer_amd.vec.policy.seat_rows (no GPU): the symbol is declared, listed and exported, the C structs and their ctypes mirrors agree, the
unit is registered in the build recipe and compiles to a kernel per VSS-v0 variant without scratch memory and within self-play's LDS; the
Python layer refuses what it must before it touches a device; and the seat map restated in tests/teamplay_helpers.py is the identity
for seat 0, an involution in bits, and commutes with the mirror map."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import selfplay_helpers as SH
import teamplay_helpers as TH
import test_selfplay_build as SB   # _fake_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNEL = re.compile(r"task_collect_team_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])E")
SIDE_FIELDS = ["obs", "actions", "mean", "sample", "final_obs", "next_obs"]


def _struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    return re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


# ---- 1. header, binding, exports, build recipe ----
def test_symbol_is_declared_listed_and_exported():
    import ctypes
    from build_variant import dynamic_symbols
    from rsoccer_amd import _lib
    header = open(os.path.join(ROOT, "include", "rsx.h")).read()
    decl = re.search(r"^int rsx_task_collect_team\((.*?)\);", header, flags=re.M | re.S)
    assert decl, "include/rsx.h does not declare rsx_task_collect_team"
    names = [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert names == ["h", "actor", "actor_params_dev", "sigma_dev", "actor_seats", "opponent", "opponent_params_dev", "opponent_sigma_dev",
                     "opponent_seats", "noise_seed", "n_steps", "out", "stream"]
    assert _struct_fields(header, "rsx_team_side_out") == [f[0] for f in _lib.TeamSideOut._fields_] == SIDE_FIELDS
    assert _struct_fields(header, "rsx_team_out") == [f[0] for f in _lib.TeamOut._fields_] == ["rewards", "flags", "actor", "opponent"]
    assert ctypes.sizeof(_lib.TeamSideOut) == 6 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.TeamOut) == 14 * ctypes.sizeof(ctypes.c_void_p)
    assert _lib.TeamOut.actor.offset == 2 * ctypes.sizeof(ctypes.c_void_p) and _lib.TeamOut.opponent.offset == 8 * ctypes.sizeof(ctypes.c_void_p)
    assert re.search(r"^#define RSX_ABI_VERSION 6\b", header, re.M)   # additive: the ABI stays 6
    # the seat map and the counter layout are written out, as the mirror map is
    assert "j + 7 i" in header and "j - 7 i" in header and "(global env id, seat, tick of that step, dom | (i >> 2) << 8)" in header
    defined, _ = dynamic_symbols(_lib.LIB_PATH)
    assert "rsx_task_collect_team" in _lib.SYMBOLS and "rsx_task_collect_team" in defined
    lib = _lib.load()
    assert len(lib.rsx_task_collect_team.argtypes) == len(names)
    assert callable(_lib.Sim.task_collect_team)


def test_the_unit_is_a_sibling_of_the_collector():
    from __graft_entry__ import CSRC, HIP_UNITS
    units = dict(HIP_UNITS)
    assert units["rsx_teamplay.hip"] == units["rsx_collect.hip"] == units["rsx_selfplay.hip"]
    text = open(os.path.join(CSRC, "rsx_teamplay.hip")).read()
    assert '#include "rsx_policy_mlp.hpp"' in text
    for piece in ("struct PolicyImage", "float policy_forward(", "void hidden_layer(", "float tanh_f32(", "PolicyImage policy_image("):
        assert piece not in text, piece   # the MLP stays stated once
    for frag in ("rsx_step_commands.inc", "rsx_step_wire.inc", "rsx_step_xr.inc", "rsx_step_reward.inc", "rsx_step_ball_load.inc",
                 "rsx_step_vss_metrics.inc"):
        assert f'#include "{frag}"' in text, frag
    assert text.count("s_waitcnt(0x0F70)") == 1   # every load lands behind one vmcnt(0), ahead of the loop
    loop = text[text.index("for (int it = 0; it < n_steps; ++it)"):text.index("// ---- store: the state in wire format")]
    for load in ("bufs.obs[", "A.params", "O.params", ".sigma[", "load_raw", "load_coefs", "stage_policy"):
        assert load not in loop, load   # no load inside the loop
    # the seats are a run-time loop: one inlined forward per hidden width, not one per seat
    assert "#pragma nounroll\n        for (int k = 0; k < SA + SO; ++k)" in text
    assert loop.count("policy_forward<64") == 1 and loop.count("policy_forward<32") == 1


@pytest.fixture(scope="module")
def team_kernels():
    """{(kind, task, L, NR, phys): {remark: value}} of rsx_teamplay.hip, compiled with the flags build() gives it"""
    from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS
    work = tempfile.mkdtemp(prefix="rsx_teamplay_probe_")
    try:
        p = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_COMMON + dict(HIP_UNITS)["rsx_teamplay.hip"] +
                           ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(work, "rsx_teamplay.o"),
                            os.path.join(CSRC, "rsx_teamplay.hip")], stderr=subprocess.PIPE, text=True)
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


def test_code_object_holds_every_vss_variant_without_scratch(team_kernels):
    from rsoccer_amd import _lib
    want = {(0, 1, L, NR, phys) for (L, NR) in ((8, 6), (16, 6), (16, 10), (8, 0), (16, 0), (32, 0)) for phys in (0, 1)}
    assert set(team_kernels) == want, sorted(set(team_kernels) ^ want)   # VSS-v0 only, MAX_L 32, both physics forms
    blob = open(_lib.LIB_PATH, "rb").read()
    for k, v in team_kernels.items():
        assert v["name"].encode() in blob, f"librsx_hip.so lacks {v['name']}"
        assert v["ScratchSize"] == 0, (k, v)
    # the headline variant: static LDS + the dynamic bytes of two 40-64-64-2 images at 8 lanes per env with an action slot of
    # max(8, round4(2 * 3)) = 8 floats per env (the host's images_bytes, restated) — two workgroups per CU need at most 81 920 B
    pitch = max(8, (2 * 3 + 3) & ~3)
    image = 4 * (40 * 68 + 64 + 64 * 68 + 64 + 192 + 8 + 3 * 8 * 68 + 8 * pitch)
    total = team_kernels[(0, 1, 8, 6, 0)]["LDS Size"] + 2 * image
    assert image == 36384 and total == 79040 and total <= 81920
    # ... and 5v5 (pitch 12) stays under the CU's 160 KB, one workgroup per CU as in self-play
    image5 = 4 * (64 * 68 + 64 + 64 * 68 + 64 + 192 + 8 + 3 * 4 * 68 + 4 * max(8, (2 * 5 + 3) & ~3))
    assert team_kernels[(0, 1, 16, 10, 0)]["LDS Size"] + 2 * image5 == 84736
    for text in (open(os.path.join(ROOT, "rsoccer_amd", "csrc", "rsx_teamplay.hip")).read(),
                 open(os.path.join(ROOT, "profiles", "LABBOOK.md")).read().split("Team play", 1)[-1]):
        assert "79 040 B" in text and "84 736 B" in text


# ---- 2. the Python layer's refusals, before any device is touched ----
def test_python_refusals_fire_without_a_device():
    import torch
    from rsoccer_amd.vec.policy import MLPPolicy
    env = SB._fake_env()
    pol = MLPPolicy(40, 2, **SH.SHAPE_SMALL)
    opp = MLPPolicy(40, 2, **SH.SHAPE_LARGE)
    params, oparams = torch.zeros(pol.num_params), torch.zeros(opp.num_params)
    with pytest.raises(ValueError, match="opponent_team given without an opponent"):
        env.collect(pol, params, 2, opponent_team=True)
    with pytest.raises(ValueError, match="opponent_team given without an opponent"):
        env.collect(pol, params, 2, team=True, opponent_team=True)
    # whatever self-play refuses, with the flags set
    with pytest.raises(ValueError, match="opponent_params must not be None"):
        env.collect(pol, params, 2, opponent=opp, team=True, opponent_team=True)
    with pytest.raises(ValueError, match=r"opponent_params must be \[%d\]" % opp.num_params):
        env.collect(pol, params, 2, opponent=opp, opponent_params=params, opponent_team=True)
    with pytest.raises(ValueError, match="opponent must be an rsoccer_amd.vec.policy.MLPPolicy"):
        env.collect(pol, params, 2, opponent="self", opponent_params=oparams, team=True)
    with pytest.raises(ValueError, match="opponent_log_std must be finite"):
        env.collect(pol, params, 2, opponent=opp, opponent_params=oparams, opponent_log_std=float("inf"), opponent_team=True)
    with pytest.raises(ValueError, match=r"params must be \[%d\]" % pol.num_params):
        env.collect(pol, oparams, 2, team=True)
    # a non-VSS-v0 env
    sd = SB._fake_env("VecSSLStaticDefendersEnv", 24, 5)
    p5 = MLPPolicy(24, 5)
    with pytest.raises(ValueError, match="team: .*VSS-v0.*VecSSLStaticDefendersEnv"):
        sd.collect(p5, torch.zeros(p5.num_params), 2, team=True)
    # unequal teams
    lop = SB._fake_env()
    lop.N_YELLOW = 2
    with pytest.raises(ValueError, match="team: .*equal teams.*VecVSSEnv"):
        lop.collect(pol, params, 2, team=True)
    with pytest.raises(ValueError, match="equal teams"):
        lop.collect(pol, params, 2, opponent=opp, opponent_params=oparams, opponent_team=True)


# ---- 3. the seat map ----
@pytest.mark.parametrize("n", [3, 5])
def test_the_seat_map_is_an_involution_that_commutes_with_the_mirror(n):
    rng = np.random.default_rng(11)
    obs = rng.uniform(-1.2, 1.2, (11, 4 + 12 * n)).astype(np.float32)
    obs[0, 4:11] = np.float32(-0.0)   # signed zeros travel as they are
    sc = rng.uniform(-1.0, 1.0, (11, n, 2)).astype(np.float32)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)   # noqa: E731
    assert np.array_equal(bits(TH.seat_map(obs, 0)), bits(obs))   # seat 0 is the identity
    for i in range(1, n):
        s = TH.seat_map(obs, i)
        assert s.dtype == np.float32 and not np.array_equal(bits(s), bits(obs))
        assert np.array_equal(bits(TH.seat_map(s, i)), bits(obs))   # an involution in bits
        a, b = SH.own(n, 0), SH.own(n, i)
        assert np.array_equal(bits(s[:, a:a + 7]), bits(obs[:, b:b + 7])) and np.array_equal(bits(s[:, b:b + 7]), bits(obs[:, a:a + 7]))
        rest = np.ones(obs.shape[1], dtype=bool)
        rest[a:a + 7] = rest[b:b + 7] = False
        assert np.array_equal(bits(s[:, rest]), bits(obs[:, rest]))   # the ball, the other own slots and every "other" slot stay
        # It commutes with the mirror in the sense the layouts allow.  The mirror turns a side's "own" slots (7 floats) into the other
        # side's "other" slots (5 floats; sine and cosine travel in its second argument), so the exchange of own slots 0 and i on one
        # side of the mirror is the exchange of "other" slots 0 and i, and of the sine / cosine pairs, on the other side of it:
        p, q = SH.other(n, 0), SH.other(n, i)

        def swap_other(row, pairs):
            row, pairs = row.copy(), pairs.copy()
            row[:, p:p + 5], row[:, q:q + 5] = row[:, q:q + 5].copy(), row[:, p:p + 5].copy()
            pairs[:, 0], pairs[:, i] = pairs[:, i].copy(), pairs[:, 0].copy()
            return row, pairs

        m, back = SH.mirror(obs, sc, n)
        # mirror(seat_map(blue's row)) == the relabelled mirror: blue seat i's view, seen from yellow
        sm, sback = SH.mirror(s, sc, n)
        want, wback = swap_other(m, back)
        assert np.array_equal(bits(sm), bits(want)) and np.array_equal(bits(sback), bits(wback))
        # seat_map(mirror(row)) == mirror(the row with yellow 0 and yellow i relabelled): yellow seat i's row
        relabelled, rsc = swap_other(obs, sc)
        ym, yback = SH.mirror(relabelled, rsc, n)
        assert np.array_equal(bits(TH.seat_map(m, i)), bits(ym)) and np.array_equal(bits(yback), bits(back))


# ---- 4. seat_rows ----
def test_seat_rows_shapes_and_values():
    import torch
    from rsoccer_amd.vec.policy import seat_rows
    T, B, S, OD = 4, 5, 3, 40
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    batch = {"obs": r(T, B, S, OD), "actions": r(T, B, S, 2), "mean": r(T, B, S, 2), "sample": r(T, B, S, 2), "log_prob": r(T, B, S),
             "final_obs": r(T, B, S, OD), "next_obs": r(B, S, OD), "reward": r(T, B), "terminated": r(T, B) > 1.0, "truncated": r(T, B) > 1.0,
             "value": r(T, B, S), "advantage": r(T, B, S), "return": r(T, B, S), "opponent_obs": r(T, B, 1, OD),
             "opponent_actions": r(T, B, 1, 2), "opponent_next_obs": r(B, 1, OD)}
    rows = seat_rows(batch)
    assert set(rows) == {"obs", "actions", "mean", "sample", "log_prob", "final_obs", "next_obs", "reward", "terminated", "truncated",
                         "value", "advantage", "return"}
    for k, v in rows.items():
        assert v.is_contiguous(), k
        assert v.shape[:2] == ((B * S, OD) if k == "next_obs" else (T, B * S)), (k, v.shape)
    for e in range(B):
        for s in range(S):
            c = e * S + s   # an (env, seat) pair is column e * S + s
            for k in ("obs", "actions", "mean", "sample", "log_prob", "final_obs", "value", "advantage", "return"):
                assert torch.equal(rows[k][:, c], batch[k][:, e, s]), (k, e, s)
            assert torch.equal(rows["next_obs"][c], batch["next_obs"][e, s])
            for k in ("reward", "terminated", "truncated"):   # shared by the seats of an env
                assert torch.equal(rows[k][:, c], batch[k][:, e]), (k, e, s)
    assert rows["terminated"].dtype == torch.bool and rows["reward"].dtype == torch.float32
    opp = seat_rows(batch, opponent=True)
    assert set(opp) == {"obs", "actions", "next_obs", "reward", "terminated", "truncated"}
    assert torch.equal(opp["obs"], batch["opponent_obs"][:, :, 0]) and opp["obs"].shape == (T, B, OD)
    with pytest.raises(ValueError, match="team batch"):
        seat_rows({**batch, "obs": batch["obs"][:, :, 0]})
    with pytest.raises(ValueError, match="lacks 'next_obs'"):
        seat_rows({k: v for k, v in batch.items() if k != "next_obs"})
