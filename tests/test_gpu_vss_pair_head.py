"""The head of the paired VSS-v0 3v3 single step and the second pass over its sub-step control flow (rsoccer_amd/csrc/
rsx_task_step_body.inc: RSX_PAIR_HEAD; rsx_contact.hpp: SubstepCuts, exchange_all and act_select) against the f32 oracle, bit for bit
after every step, on a paired handle (task_pair_step_kernel) and on an RSX_SERVICE_WAVE=0 handle (task_step_kernel): observations,
rewards, flags, info rows, terminal observations, step counts, the episode row, the full state and the folded metrics.

The head: the physics wave issues every load in front of its first barrier (state rows, the ball's spin row, the step and episode rows,
the OU rows, the env-step counter, fed actions) ahead of one wait, and the loaded scalars are used behind it only.  So: device-drawn
and caller-fed actions, a device-keyed handle, the first step of an episode (steps == 0), truncation and auto-reset on exactly the
third step, padded rows, and 9 envs with dense rows (the dead lane groups of the second tile sit behind the last column of every row,
and the last row ends where the handle's allocation does, as far as the handle API decides that; shown by results alone).

The exchange on all lanes: one tile of eight holds a deep pair (second sweep), a shallow pair that must be walked once, a free env, a
robot next to the origin (where the idle lane's zeros sit) in an env with a shallow pair elsewhere, and a ball next to the origin
likewise: an idle lane that acted on its test would give its env a second sweep and change the shallow pair's bits.
(Exactly AT the origin the overlap key of the idle lane wraps like a lane's own slot, d2 == 0, and the test cannot fire: the bodies
stand a centimetre off.)

Actuation by select: balls with spin and velocity, and with -0.0 in vx, vy and the spin; the velocities' zeros keep their sign through a
step (asserted on the oracle), the spin's becomes +0.0 in the once-per-step decay of every implementation, the oracle's included.

Every case is run on the oracle first and asserts, in numpy on the oracle's states, that it is the case it says it is.
Batches as in tests/test_gpu_vss_substep_paths.py: 8 envs (one tile), 9 (a second tile with seven dead env slots) and 72 (nine tiles)."""
import functools

import numpy as np
import pytest

from helpers import f32_equal, mismatch_report

pytestmark = pytest.mark.gpu

BATCHES = (8, 9, 72)
KEYS = ("obs", "reward", "terminated", "truncated", "info", "final_obs", "steps")
R_ROBOT, R_BALL, PEN2 = 0.0375, 0.0215, 0.005   # rsx_params.hpp: ModelD<VSS>, KC
RS_RB, RS_RR = R_ROBOT + R_BALL, 2 * R_ROBOT
VX, VY, SPIN = 3, 4, 42            # full state of a 3v3 env: ball x y z vx vy, six robots x y theta vx vy omega, ball vz, ball spin
SEED = 33


def _rob(s, k):
    return s[..., 5 + 6 * k: 11 + 6 * k]


def _lineup(B):
    """robots on two lines far from each other, from the walls and from the origin, the ball rolling slowly away from everything"""
    e = np.arange(B)
    ball = np.c_[0.15 + 0.01 * (e % 7), 0.2 + 0.01 * (e % 5), 0.1 + 0 * e, 0.02 * (e % 3)]
    rob = np.zeros((B, 6, 3))
    for k in range(6):
        rob[:, k] = np.c_[(-0.4, 0.4)[k // 3] + 0 * e, -0.4 + 0.4 * (k % 3) + 0.003 * (e % 4), 30.0 * k + e]
    return ball, rob


def _pairs(s):
    """[B,6,6] robot-robot distances (9 on the diagonal), [B,6] robot-ball distances"""
    x = np.stack([_rob(s, k)[:, 0] for k in range(6)], 1); y = np.stack([_rob(s, k)[:, 1] for k in range(6)], 1)
    return np.hypot(x[:, :, None] - x[:, None], y[:, :, None] - y[:, None]) + 9.0 * np.eye(6), np.hypot(x - s[:, :1], y - s[:, 1:2])


# ---- the cases: name -> (ball [B,4], robots [B,6,3], state patch or None, fed actions [T,B,2] or None, steps, check) ----
# `check(S, out)`: S[t] = the oracle's full states [B,43] BEFORE step t (S[0]: as patched), S[T] after the last step; out[t] its outputs

def _case_head(B, fed, T=4):
    ball, rob = _lineup(B)

    def check(S, out):
        assert all(o["steps"] == 1 for o in out[0]), "the first step of an episode: the step row read 0"
    acts = np.random.default_rng(7).uniform(-1, 1, (T, B, 2)).astype(np.float32) if fed else None
    return ball, rob, None, acts, T, check


def _case_truncation(B):
    ball, rob, _, _, _, _ = _case_head(B, False)

    def check(S, out):
        trunc = np.array([[o["truncated"] for o in row] for row in out])
        term = np.array([[o["terminated"] for o in row] for row in out])
        assert not term.any() and np.array_equal(trunc.any(1), [False, False, True, False, False]) and trunc[2].all(), "the third step ends every episode"
        assert [row[0]["steps"] for row in out] == [1, 2, 0, 1, 2]
    return ball, rob, None, None, 5, check


def _case_exchange(B):
    ball, rob = _lineup(B)
    e = np.arange(B)
    k = e % 8
    rob[k == 0, 1] = rob[k == 0, 0] + (0.0, 0.060, 0.0)             # 15 mm into each other: deep, a second sweep
    for kk in (1, 3, 4):
        rob[k == kk, 1] = rob[k == kk, 0] + (0.0, 0.0735, 0.0)      # 1.5 mm: touching, one walk
    rob[k == 3, 2] = (0.03, 0.02, 10.0)                              # a robot's centre 36 mm from the origin
    ball[k == 4] = (0.01, 0.005, 0.0, 0.0)                           # the ball 11 mm from the origin, at rest

    def check(S, out):
        s = S[0]
        d, db = _pairs(s)
        near = d.min((1, 2))
        assert (RS_RR - near[k == 0] > PEN2 + 0.005).all(), "env 0 of a tile: a deep pair"
        for kk in (1, 3, 4):
            assert ((RS_RR - near[k == kk] > 0.0005) & (RS_RR - near[k == kk] < PEN2 - 0.002)).all(), "a touching pair below pen2"
        assert (near[(k == 2) | (k >= 5)] > RS_RR + 0.1).all() and (db.min(1) > RS_RB + 0.05).all(), "nothing else touches"
        ro = np.hypot(_rob(s, 2)[:, 0], _rob(s, 2)[:, 1])
        assert (ro[k == 3] < RS_RR - PEN2 - 0.02).all() and (ro[k == 3] > 0).all(), "a robot deep inside the idle lane's circle"
        bo = np.hypot(s[:, 0], s[:, 1])
        assert (bo[k == 4] < RS_RB - PEN2 - 0.02).all() and (bo[k == 4] > 0).all() and (bo[k != 4] > RS_RB + 0.05).all(), "a ball likewise"
        far = np.hypot(*[np.stack([_rob(s, j)[:, c] for j in range(6)], 1) for c in (0, 1)])
        far[k == 3, 2] = 9.0
        assert (far > RS_RR + 0.1).all(), "no other robot near the origin"
    return ball, rob, None, None, 3, check


def _case_ball_keeps_its_bits(B):
    ball, rob = _lineup(B)
    e = np.arange(B)

    def patch(s):
        s[:, SPIN] = np.where(e % 4 == 0, 7.5, np.where(e % 4 == 1, -3.25, -0.0))
        s[e % 4 == 2, VX] = -0.0; s[e % 4 == 2, VY] = -0.0     # at rest, minus zeros
        s[e % 4 == 3, VX] = -0.0; s[e % 4 == 3, VY] = 0.05     # one component, the other one moving

    def check(S, out):
        a, b = S[0], S[1]
        assert (a[e % 4 < 2, SPIN] != 0).all() and (b[e % 4 < 2, SPIN] != 0).all() and (np.hypot(b[e % 4 < 2, VX], b[e % 4 < 2, VY]) > 0.05).all()
        assert np.signbit(a[e % 4 >= 2, SPIN]).all() and (a[e % 4 >= 2, SPIN] == 0).all()
        for col, envs in ((VX, e % 4 >= 2), (VY, e % 4 == 2)):
            assert (a[envs, col] == 0).all() and np.signbit(a[envs, col]).all(), "-0.0 going in"
            assert (b[envs, col] == 0).all() and np.signbit(b[envs, col]).all(), "-0.0 after a step"
        assert (b[e % 4 == 3, VY] != 0).all()
    return ball, rob, patch, None, 2, check


# name -> (case, max_episode_steps, device-keyed handle, RSX_ROW_PAD)
CASES = {
    "drawn_actions": (lambda B: _case_head(B, False), 0, False, None),
    "fed_actions": (lambda B: _case_head(B, True), 0, False, None),
    "device_keyed": (lambda B: _case_head(B, False), 0, True, None),
    "device_keyed_fed": (lambda B: _case_head(B, True), 0, True, None),
    "truncation_on_the_third_step": (_case_truncation, 3, False, None),
    "padded_rows": (lambda B: _case_head(B, True), 3, False, "200"),
    "exchange_on_all_lanes": (_case_exchange, 0, False, None),
    "ball_keeps_its_bits": (_case_ball_keeps_its_bits, 0, False, None),
}


@functools.lru_cache(maxsize=None)
def reference(O, name, B):
    """the case on B oracle envs: (ball, robots, patched start states or None, actions, outputs [T][B], states [T+1][B][43] float32,
    metrics [T], episode ends so far [T][B]); the case's own precondition is asserted here, on the oracle's states alone"""
    case, max_steps, _, _ = CASES[name]
    ball, rob, patch, acts, T, check = case(B)
    ball = np.float32(ball).astype(np.float64); rob = np.float32(rob).astype(np.float64)   # the float state holds the same bits
    refs = [O.OracleEnv(0, 0, 3, 3, 25, "f32") for _ in range(B)]
    for e, r in enumerate(refs):
        r.task_attach(1, SEED, e, max_steps)
        r.task_reset()
        r.task_reset_to(ball[e], rob[e, :3], rob[e, 3:])
    start = None
    if patch is not None:
        start = np.array([r.get_state_full() for r in refs])
        patch(start)
        start = np.float32(start).astype(np.float64)
        for e, r in enumerate(refs):
            r.set_state_full(start[e])
    S, out, met, ends = [np.array([r.get_state_full() for r in refs], dtype=np.float32)], [], [], []
    for t in range(T):
        for e, r in enumerate(refs):
            r.task_step(None if acts is None else acts[t, e])
        out.append([r.task_out() for r in refs])
        S.append(np.array([r.get_state_full() for r in refs], dtype=np.float32))
        met.append(sum(o["metrics"] for o in out[-1]))
        ends.append((ends[-1] if ends else 0) + np.array([int(o["terminated"] or o["truncated"]) for o in out[-1]]))
    for r in refs:
        r.close()
    S = np.array(S)
    check(S, out)
    return ball, rob, start, acts, out, S, met, ends


def _handles(monkeypatch, B, max_steps, pad):
    from rsoccer_amd import _lib as L
    sims = []
    monkeypatch.delenv("RSX_ROW_PAD", raising=False)
    if pad is not None:
        monkeypatch.setenv("RSX_ROW_PAD", pad)   # rounded up to 256 floats
    for on in ("1", "0"):
        monkeypatch.setenv("RSX_SERVICE_WAVE", on)   # read by rsx_task_attach
        sim = L.Sim(0, 0, 3, 3, 25, B)
        sim.task_attach(1, SEED, 0, max_steps)
        assert sim.task_layout() == "8-lanes-per-env" and sim.task_service_wave() == (on == "1")
        assert sim._view.row_stride == sim._tview.row_stride == (B if pad is None else B + 256)
        sim.task_reset()
        sims.append(sim)
    return sims


def _episodes(sim):
    """the episode row of the scalar arena, the row behind the step row (rsx_params.hpp: ROW_STEPS, ROW_EPISODE), as integers"""
    import torch
    rows = sim._rows(sim._tview.steps, 2, sim._tview.row_stride)
    return rows[1].contiguous().view(torch.int32).cpu().numpy().copy()


def _snapshot(sim):
    import torch
    torch.cuda.synchronize()
    t = sim.task_tensors()
    got = {k: t[k].cpu().numpy().copy() for k in KEYS}
    got["state"] = np.ascontiguousarray(sim.get_state_full(), dtype=np.float32)
    got["metrics"] = np.asarray(sim.read_metrics()).copy()
    got["episode"] = _episodes(sim)
    return got


def _compare(a, out, state, metrics, episode, what):
    for e, o in enumerate(out):
        assert f32_equal(a["obs"][e], o["obs"]), mismatch_report(a["obs"][e], o["obs"], f"{what}: obs env {e}")
        assert f32_equal(a["reward"][e], o["reward"]), f"{what}: reward env {e}: {a['reward'][e]} vs {o['reward']}"
        assert a["terminated"][e] == o["terminated"] and a["truncated"][e] == o["truncated"], f"{what}: flags env {e}"
        assert f32_equal(a["info"][:, e], o["info"]), mismatch_report(a["info"][:, e], o["info"], f"{what}: info env {e}")
        assert a["steps"][e] == o["steps"], f"{what}: steps env {e}"
        if o["terminated"] or o["truncated"]:
            assert f32_equal(a["final_obs"][e], o["final_obs"]), f"{what}: final_obs env {e}"
        assert np.array_equal(a["state"][e].view(np.uint32), state[e].view(np.uint32)), mismatch_report(a["state"][e], state[e], f"{what}: state env {e}")
    assert np.array_equal(a["metrics"], metrics), f"{what}: metrics {a['metrics']} vs {metrics}"
    assert np.array_equal(a["episode"], episode), f"{what}: episode row {a['episode']} vs {episode}"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_the_oracle_on_both_kernels(oracle_mod, monkeypatch, name, B):
    import torch
    ball, rob, start, acts, out, S, met, ends = reference(oracle_mod, name, B)
    _, max_steps, keyed, pad = CASES[name]
    sims = _handles(monkeypatch, B, max_steps, pad)
    for kernel, sim in zip(("paired", "one wave"), sims):
        sim.task_reset_to(ball, rob[:, :3], rob[:, 3:])
        if start is not None:
            sim.set_state(start)
        if keyed:
            sim.task_enable_capture()
        torch.cuda.synchronize()
        episode0 = _episodes(sim)   # the episode the placement started; every end after it adds one
        assert (episode0 == episode0[0]).all()
        buf = sim.task_tensors()["actions"]
        for t in range(len(out)):
            if acts is None:
                sim.task_step(None)
            else:
                buf.copy_(torch.from_numpy(acts[t]))
                sim.task_step(buf.data_ptr())
            _compare(_snapshot(sim), out[t], S[t + 1], met[t], episode0 + ends[t], f"{name}, {kernel} kernel, step {t}")
        sim.close()
