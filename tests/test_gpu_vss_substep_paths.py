"""Both sub-step loops of the VSS-v0 3v3 eight-lane single-step kernels (rsoccer_amd/csrc/rsx_contact.hpp: SubstepCuts) against the f32
oracle, bit for bit after every step, on a paired handle (task_pair_step_kernel) and on an RSX_SERVICE_WAVE=0 handle (task_step_kernel):
observations, rewards, flags, info rows, terminal observations, step counts, the full state and the folded metrics.

A wave whose balls are all down runs the sub-steps without the flight gate and the ball-height ballot; a wave with a ball in flight runs
the general loop.  Nothing in VSS launches the ball, so the airborne states are written with Sim.set_state / the oracle's set_state_full
(the simulator state only: the bodies are placed with task_reset_to, which starts the episode the task scalars belong to, and the
state write then changes heights and velocities, not the ball's position).  The walk cases put lanes through two partners, through
separating pairs (vn >= 0, also with -0.0 components: the impulse is selected away, not branched around) and through a second sweep.

Every case is run on the oracle first and asserts, in numpy on the oracle's states, that it is the case it says it is.
Batches as in tests/test_gpu_service_wave.py: 8 envs (one tile), 9 (a second tile with seven dead env slots) and 72 (nine tiles).

(VSS has two sweeps per sub-step, not four — KC::held, rsx_params.hpp; the third and fourth are SSL's — so the pile case asserts an
overlap beyond pen2 on a body with two partners, one of them at a wall: what takes the second sweep.)"""
import functools
import os

import numpy as np
import pytest

from helpers import f32_equal, mismatch_report

pytestmark = pytest.mark.gpu

BATCHES = (8, 9, 72)
KEYS = ("obs", "reward", "terminated", "truncated", "info", "final_obs", "steps")
R_ROBOT, R_BALL, ROBOT_H, VZ_MIN, PEN2 = 0.0375, 0.0215, 0.15, 0.2, 0.005   # rsx_params.hpp: ModelD<VSS>, KC
RS_RB, RS_RR = R_ROBOT + R_BALL, 2 * R_ROBOT
HALF_LEN, HALF_WID = 0.75, 0.65
Z, VZ, SPIN = 2, 41, 42            # full state of a 3v3 env: ball x y z vx vy, six robots x y theta vx vy omega, ball vz, ball spin
PILES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_v2_vss_piles.npz")


def _rob(s, k):
    return s[..., 5 + 6 * k: 11 + 6 * k]


def _lineup(B):
    """robots on two lines far from each other and from the walls, the ball rolling slowly in midfield; a little different per env"""
    e = np.arange(B)
    ball = np.c_[0.01 * (e % 7) - 0.03, 0.05 + 0.01 * (e % 5), 0.1 + 0 * e, 0.02 * (e % 3)]
    rob = np.zeros((B, 6, 3))
    for k in range(6):
        rob[:, k] = np.c_[(-0.4, 0.4)[k // 3] + 0 * e, -0.4 + 0.4 * (k % 3) + 0.003 * (e % 4), 30.0 * k + e]
    return ball, rob


# ---- the cases: (ball [B,4], robots [B,6,3], state patch or None, fed actions [T,B,2] or None, steps, max_episode_steps, check) ----
# `check(S)`: S[t] = the oracle's full states [B,43] BEFORE step t (S[0]: as patched), S[T] after the last step; `out[t]` its outputs

def _case_one_airborne(B):
    ball, rob = _lineup(B)

    def patch(s):
        s[3, Z] = R_BALL + 0.3; s[3, VZ] = 1.0

    def check(S, out):
        z = S[:, :, Z] - np.float32(R_BALL)
        assert z[0, 3] > 0 and z[:15, 3].min() > 0 and z[-1, 3] == 0 and S[-1, 3, VZ] == 0, "env 3: in flight, then down"
        assert (np.delete(z, 3, axis=1) == 0).all() and (np.delete(S[:, :, VZ], 3, axis=1) == 0).all(), "every other ball stays down"
    return ball, rob, patch, None, 40, 0, check


def _case_lands_mid_step(B):
    ball, rob = _lineup(B)

    def patch(s):
        e = np.arange(B)
        s[:, Z] = R_BALL + 0.003 + 0.004 * (e % 5); s[:, VZ] = -1.0 - 0.1 * (e % 3)   # down within the first one to five sub-steps

    def check(S, out):
        assert (S[0, :, Z] > np.float32(R_BALL)).all() and (S[0, :, VZ] < 0).all()
        assert (S[1, :, VZ] > VZ_MIN).all(), "landed inside the first step and bounced"
        assert (S[-1, :, Z] == np.float32(R_BALL)).all() and (S[-1, :, VZ] == 0).all(), "at rest on the ground in the end"
    return ball, rob, patch, None, 20, 0, check


def _case_over_a_robot(B):
    ball, rob = _lineup(B)
    e = np.arange(B)
    ball[:, 0] = rob[:, 0, 0] + 0.01 + 0.002 * (e % 4); ball[:, 1] = rob[:, 0, 1] - 0.004 * (e % 3)
    ball[:, 2:] = (-0.03, 0.0)   # drifting towards the robot's centre: closing when they meet

    def patch(s):
        s[:, Z] = R_BALL + 0.25 + 0.01 * (e % 4)

    def check(S, out):
        z = S[:, :, Z] - np.float32(R_BALL)
        d = np.hypot(S[:, :, 0] - _rob(S, 0)[:, :, 0], S[:, :, 1] - _rob(S, 0)[:, :, 1])
        still = (S[:, :, 3] == S[0, :, 3]) & (S[:, :, 4] == S[0, :, 4])   # (no rolling resistance in flight)
        for env in range(B):
            above = z[:, env] >= ROBOT_H
            assert above[:4].all() and (d[above, env] < RS_RB).all() and still[above, env].all(), "over the robot, above its top: no contact"
            assert (~still[~above, env]).any(), "pushed off the robot once below its top"
        assert (z[-1] == 0).all()
    return ball, rob, patch, np.zeros((30, B, 2), np.float32), 30, 0, check   # (the agent, robot 0, stands still)


def _case_airborne_at_episode_end(B):
    ball, rob = _lineup(B)
    e = np.arange(B)
    goal = e % 4 == 1   # one sub-step short of the goal line and moving out (tests/test_gpu_service_wave.py), in flight
    ball[goal] = np.c_[np.where(e % 8 == 1, 0.7475, -0.7475), 0.01 * (e % 5) - 0.02, np.where(e % 8 == 1, 1.0, -1.0), 0 * e][goal]

    def patch(s):
        fly = e % 2 == 1   # every odd env; the even ones stay down: mixed waves
        s[fly, Z] = R_BALL + 0.1 + 0.02 * (e[fly] % 3); s[fly, VZ] = 2.0

    def check(S, out):
        ended = np.array([[o["terminated"] or o["truncated"] for o in row] for row in out])   # [T][B]
        flying = S[:-1, :, Z] > np.float32(R_BALL)
        assert (ended[0] & flying[0])[goal].all(), "a goal with the ball in flight"
        assert (ended[2] & flying[2])[(e % 2 == 1) & ~goal].all(), "a truncation with the ball in flight"
        assert (S[-1, :, Z] == np.float32(R_BALL)).all(), "the new episodes start on the ground"
    return ball, rob, patch, None, 9, 3, check


def _case_squeezed_ball(B):
    ball, rob = _lineup(B)
    e = np.arange(B)
    ball[:, :2] = np.c_[0 * e, 0.002 * (e % 3)]; ball[:, 2:] = np.c_[0.2 - 0.1 * (e % 5), 0.05 * (e % 2)]
    rob[:, 0] = np.c_[-0.050 - 0.001 * (e % 4), 0 * e, 0 * e]          # the ball overlaps a blue robot on its left
    rob[:, 3] = np.c_[0.049 + 0.001 * (e % 3), 0.001 * (e % 5), 180 + 0 * e]   # and a yellow one on its right

    def check(S, out):
        d = np.stack([np.hypot(S[0, :, 0] - _rob(S[0], k)[:, 0], S[0, :, 1] - _rob(S[0], k)[:, 1]) for k in range(6)], 1)
        assert ((d < RS_RB - 0.003).sum(1) >= 2).all(), "the ball lane walks two partners"
        assert (RS_RB - d.min(1) > PEN2 + 0.002).all(), "and its env takes the second sweep"
    return ball, rob, None, None, 10, 0, check


def _separating(B, minus_zero):
    ball, rob = _lineup(B)
    e = np.arange(B)
    ang = 0.7 * (e % 9)
    ball[:, 0] = rob[:, 0, 0] + 0.052 * np.cos(ang); ball[:, 1] = rob[:, 0, 1] + 0.052 * np.sin(ang)   # 7 mm into the agent's circle
    speed = np.where(e % 3 == 2, -0.4, 0.5)   # every third env closes in instead: both kinds of lane in one walk
    ball[:, 2] = speed * np.cos(ang); ball[:, 3] = speed * np.sin(ang)
    sep = e % 3 != 2

    def patch(s):
        if minus_zero:
            s[e % 3 == 0, 3] = -0.0; s[e % 3 == 0, 4] = -0.0      # vn = -0.0: not closing
            s[e % 3 == 1, 4] = -0.0                                # one component
            _rob(s, 0)[:, 3] = -0.0; _rob(s, 0)[:, 4] = -0.0      # the robot's own velocity
            s[:, SPIN] = -0.0

    def check(S, out):
        s = S[0].astype(np.float32)
        dx, dy = s[:, 0] - _rob(s, 0)[:, 0], s[:, 1] - _rob(s, 0)[:, 1]
        d = np.hypot(dx, dy)
        vn = ((s[:, 3] - _rob(s, 0)[:, 3]) * dx + (s[:, 4] - _rob(s, 0)[:, 4]) * dy) / d
        assert (d < RS_RB - 0.004).all(), "overlapping"
        assert (vn[sep] >= 0).all() and (vn[~sep] < -0.1).all(), "separating (closing in every third env)"
        if minus_zero:
            assert np.signbit(s[e % 3 == 0, 3]).all() and np.signbit(s[e % 3 != 2, 4]).all() and (vn[e % 3 == 0] == 0).all()
            assert np.signbit(_rob(s, 0)[:, 3]).all()
    return ball, rob, patch, np.zeros((6, B, 2), np.float32), 6, 0, check   # (the agent stands still: the pair's normal speed is the ball's)


def _case_separating_pair(B):
    return _separating(B, False)


def _case_separating_pair_minus_zero(B):
    return _separating(B, True)


def _case_pile_on_a_wall(B):
    """even envs: three robots in a column pressed on the +y touch line, 7 to 8 mm into each other, the ball against the middle one;
    odd envs: a recorded goal-mouth scrum (tests/golden/model_v2_vss_piles.npz) with the ball moved to midfield"""
    ball, rob = _lineup(B)
    z = np.load(PILES)
    rec = np.concatenate([z["vss0_states"], z["vss1_states"]])
    e = np.arange(B)
    vel = np.zeros((B, 6, 3))
    for env in range(B):
        if env % 2:
            s = rec[(env // 2) % len(rec)]
            rob[env] = s[5:41].reshape(6, 6)[:, :3]; vel[env] = s[5:41].reshape(6, 6)[:, 3:]
            ball[env] = (0.0, 0.3, 0.0, 0.0)
        else:
            x0, gap = -0.2 + 0.05 * (env % 5), 0.067 + 0.0005 * (env % 3)
            for k, row in ((0, 0), (1, 1), (3, 2)):
                rob[env, k] = (x0 + 0.002 * row, HALF_WID - R_ROBOT - row * gap, 90.0)
            ball[env] = (x0 + 0.053, HALF_WID - R_ROBOT - gap, -0.3, 0.0)
            vel[env, 3] = (0.0, 0.4, 0.0)   # the last of the column drives the pile into the wall

    def patch(s):
        _rob(s, 0)[:, 3:] = vel[:, 0]
        for k in range(1, 6):
            _rob(s, k)[:, 3:] = vel[:, k]

    def check(S, out):
        s = S[0]
        x = np.stack([_rob(s, k)[:, 0] for k in range(6)], 1); y = np.stack([_rob(s, k)[:, 1] for k in range(6)], 1)
        d = np.hypot(x[:, :, None] - x[:, None], y[:, :, None] - y[:, None]) + 9.0 * np.eye(6)
        db = np.hypot(x - s[:, :1], y - s[:, 1:2])
        partners = (d < RS_RR).sum(2) + (db < RS_RB)
        at_wall = (np.abs(y) > HALF_WID - R_ROBOT - 0.001) | (np.abs(x) > HALF_LEN - R_ROBOT - 0.001)
        built = e % 2 == 0
        assert (partners[built].max(1) >= 3).all() and (RS_RR - d[built].min((1, 2)) > PEN2 + 0.001).all(), "a body with three partners, a deep pair"
        assert (at_wall & ((d < RS_RR).sum(2) > 0))[built].any(1).all(), "a touching robot held by the wall"
        if B > 1:
            assert (partners[~built].max(1) >= 2).sum() >= max(1, (B // 2) // 2), "recorded scrums: a body with two partners in most"
            assert (at_wall & ((d < RS_RR).sum(2) > 0))[~built].any(1).sum() >= max(1, (B // 2) // 2)
    fed = np.clip(np.random.default_rng(5).uniform(0.2, 1.0, (12, B, 2)), -1, 1).astype(np.float32)   # the agent (top of the column) keeps driving
    return ball, rob, patch, fed, 12, 0, check


CASES = {f.__name__[6:]: f for f in (_case_one_airborne, _case_lands_mid_step, _case_over_a_robot, _case_airborne_at_episode_end,
                                     _case_squeezed_ball, _case_separating_pair, _case_separating_pair_minus_zero, _case_pile_on_a_wall)}
SEED = 21


@functools.lru_cache(maxsize=None)
def reference(O, name, B):
    """the case on B oracle envs: (ball, robots, patched start states or None, actions, outputs [T][B], states [T+1][B][43] float32,
    metrics [T]); the case's own precondition is asserted here, on the oracle's states alone"""
    ball, rob, patch, acts, T, max_steps, check = CASES[name](B)
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
    S, out, met = [np.array([r.get_state_full() for r in refs], dtype=np.float32)], [], []
    for t in range(T):
        for e, r in enumerate(refs):
            r.task_step(None if acts is None else acts[t, e])
        out.append([r.task_out() for r in refs])
        S.append(np.array([r.get_state_full() for r in refs], dtype=np.float32))
        met.append(sum(o["metrics"] for o in out[-1]))
    for r in refs:
        r.close()
    S = np.array(S)
    check(S, out)
    return ball, rob, start, acts, out, S, met


def _handles(monkeypatch, B, max_steps):
    from rsoccer_amd import _lib as L
    sims = []
    for on in ("1", "0"):
        monkeypatch.setenv("RSX_SERVICE_WAVE", on)   # read by rsx_task_attach
        sim = L.Sim(0, 0, 3, 3, 25, B)
        sim.task_attach(1, SEED, 0, max_steps)
        assert sim.task_layout() == "8-lanes-per-env" and sim.task_service_wave() == (on == "1")
        sim.task_reset()
        sims.append(sim)
    return sims


def _snapshot(sim):
    import torch
    torch.cuda.synchronize()
    t = sim.task_tensors()
    got = {k: t[k].cpu().numpy().copy() for k in KEYS}
    got["state"] = np.ascontiguousarray(sim.get_state_full(), dtype=np.float32)
    got["metrics"] = np.asarray(sim.read_metrics()).copy()
    return got


def _compare(a, out, state, metrics, what):
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


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_the_oracle_on_both_kernels(oracle_mod, monkeypatch, name, B):
    import torch
    ball, rob, start, acts, out, S, met = reference(oracle_mod, name, B)
    sims = _handles(monkeypatch, B, CASES[name](B)[5])
    for kernel, sim in zip(("paired", "one wave"), sims):
        sim.task_reset_to(ball, rob[:, :3], rob[:, 3:])
        if start is not None:
            sim.set_state(start)
        buf = sim.task_tensors()["actions"]
        for t in range(len(out)):
            if acts is None:
                sim.task_step(None)
            else:
                buf.copy_(torch.from_numpy(acts[t]))
                sim.task_step(buf.data_ptr())
            _compare(_snapshot(sim), out[t], S[t + 1], met[t], f"{name}, {kernel} kernel, step {t}")
        sim.close()
