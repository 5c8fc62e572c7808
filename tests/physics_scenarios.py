"""Scenarios of the per-env physics parity tests (tests/test_gpu_physics_parity.py) and the oracle-only computation of which
parameters each of them can see.

A scenario is everything but the simulator: the line-up, every step's commands or actions (all drawn beforehand: nothing depends
on the state), and one parameter set per env.  `run_raw` / `run_task` step f32 oracle envs carrying the derived coefficients
through it; the GPU tests hook into the same loops.  A parameter is LIVE in a scenario when putting it back to its default in
every env changes the final state of at least one env: a kernel that reads the literal in its place then cannot agree with the
oracle over that scenario."""
import functools

import numpy as np

from helpers import random_placement
from physics_helpers import DEFAULTS, NAMES, derive, random_params, set_oracle_coefs

# tests/test_gpu_parity.py: CASES (kind, field_type, nb, ny, B, steps, spread) and TASKS (task, kind, ft, nb, ny, B, steps, max_steps)
from test_gpu_parity import CASES, TASKS


def valid_params(kind):
    return [n for n in NAMES if kind == 0 or n != "a_lat"]


def hetero_params(kind, B, seed):
    raw = random_params(kind, np.random.default_rng(seed), B)
    if kind == 1:
        raw[:, NAMES.index("a_lat")] = 0.0
    return raw


def parity_commands(rng, kind, B, N):
    """the command generator of test_gpu_parity.py::test_raw_step_bitexact (same draws in the same order)"""
    if kind == 0:
        return rng.uniform(-60, 60, (B, N, 2))
    cmds = np.zeros((B, N, 8))
    use_wheels = rng.random((B, N)) < 0.3
    cmds[..., 0] = use_wheels
    cmds[..., 1:5] = np.where(use_wheels[..., None], rng.uniform(-120, 120, (B, N, 4)),
                              np.concatenate([rng.uniform(-3, 3, (B, N, 2)), rng.uniform(-12, 12, (B, N, 1)), np.zeros((B, N, 1))], -1))
    cmds[..., 5] = np.where(rng.random((B, N)) < 0.3, 4.0, 0.0)
    cmds[..., 6] = np.where(rng.random((B, N)) < 0.1, 2.0, 0.0)
    cmds[..., 7] = rng.random((B, N)) < 0.5
    return cmds


def _field(O, kind, ft, nb, ny):
    r = O.OracleEnv(kind, ft, nb, ny, 25, "f32")
    fp = r.field_params()   # rsoccer_amd/_lib.py: FIELD_KEYS
    r.close()
    return dict(hl=fp[0] / 2, hw=fp[1] / 2, r=fp[14], margin=0.3 if kind == 1 else 0.0)


class RawScenario:
    """ball [B,4], blue [B,nb,3], yellow [B,ny,3], spin [B] (rad/s, written into the full state after the reset) or None,
    cmds [steps,B,N,C], raw [B,14]"""

    def __init__(self, name, kind, ft, nb, ny, B, steps, ball, blue, yellow, spin, cmds, raw):
        self.name, self.kind, self.ft, self.nb, self.ny, self.B, self.steps = name, kind, ft, nb, ny, B, steps
        self.ball, self.blue, self.yellow, self.spin, self.cmds, self.raw = ball, blue, yellow, spin, cmds, raw


def _raw_name(case):
    return f"{'vss' if case[0] == 0 else 'ssl'}-{case[2]}v{case[3]}"


RAW_SEEDS = {"ssl-4v3": 7, "ssl-2v0": 20}   # (at their 11 and 5 envs: the first seeds whose line-ups bring the ball into play; 0 elsewhere)


def _borrowed_raw(O, case, seed=0):
    kind, ft, nb, ny, B, steps, spread = case
    f = _field(O, kind, ft, nb, ny)
    rng = np.random.default_rng(1234 + kind * 10 + nb + 1000 * seed)
    ball, blue, yellow = random_placement(rng, B, nb, ny, f["hl"], f["hw"], 2.2 * f["r"], spread)
    cmds = np.stack([parity_commands(rng, kind, B, nb + ny) for _ in range(steps)])
    return RawScenario(_raw_name(case), kind, ft, nb, ny, B, steps, ball, blue, yellow, None, cmds, hetero_params(kind, B, 500 + nb + ny))


def _directed_raw(O, kind):
    """3v3 on the small field of the class, 24 steps, every env a variation of one line-up: robot 0 drives into the +y wall (e_wr);
    robots 1 and 2 drive at each other with their centre lines a little apart (e_rr, mu_rr); robot 4 rams the flank of robot 3,
    which stands across its path (VSS: a_lat); robot 5 drives on its own (SSL: dribbler on, kicker armed, no ball in reach); the ball
    starts spinning and flies obliquely into the -y wall (mu_wb, spin_dec, e_wb).  No robot meets the ball here: m_robot, m_ball, e_rb
    and mu_rb are what the borrowed line-ups see."""
    ft, nb, ny, B, steps = (0, 3, 3, 24, 24) if kind == 0 else (2, 3, 3, 24, 24)
    f = _field(O, kind, ft, nb, ny)
    r, yl = f["r"], f["hw"] + f["margin"] - f["r"]
    rng = np.random.default_rng(900 + kind)
    j = lambda s: rng.uniform(-s, s, B)
    rob = np.zeros((B, 6, 3))
    rob[:, 0] = np.c_[-0.5 + j(0.02), yl - 0.5 * r + j(0.2 * r), 90 + j(15)]
    rob[:, 1] = np.c_[-0.2 - 1.6 * r + j(0.01), 0.1 + j(0.3 * r), j(5)]
    rob[:, 2] = np.c_[-0.2 + 1.6 * r + j(0.01), 0.1 + j(0.3 * r), 180 + j(5)]
    rob[:, 3] = np.c_[0.35 + j(0.01), 0.1 + j(0.3 * r), 90 + j(10)]
    rob[:, 4] = np.c_[0.35 - 3.0 * r + j(0.01), 0.1 + j(0.3 * r), j(5)]
    rob[:, 5] = np.c_[0.0 + j(0.02), -0.25 + j(0.02), -90 + j(20)]
    ball = np.c_[0.3 + j(0.05), -yl + 0.15 + j(0.03), rng.uniform(0.4, 1.2, B), rng.uniform(-2.0, -1.0, B)]
    spin = rng.uniform(20.0, 60.0, B) * np.where(rng.random(B) < 0.5, -1.0, 1.0)
    N = 6
    if kind == 0:
        cmds = np.full((steps, B, N, 2), 35.0) + rng.uniform(-6, 6, (steps, B, N, 2))
        cmds[:, :, 3] = rng.uniform(-3, 3, (steps, B, 2))      # the rammed robot barely drives
    else:
        cmds = np.zeros((steps, B, N, 8))
        cmds[..., 1] = 1.5 + rng.uniform(-0.3, 0.3, (steps, B, N))   # robot-local forward velocity
        cmds[..., 2] = rng.uniform(-0.2, 0.2, (steps, B, N))
        cmds[..., 3] = rng.uniform(-2, 2, (steps, B, N))
        cmds[:, :, 3, 1:4] *= 0.1
        cmds[:, :, 5, 7] = 1.0                                   # robot 5 dribbles
        cmds[steps // 2:, :, 5, 5] = 3.0                         # and kicks in the second half
    name = ("vss" if kind == 0 else "ssl") + "-3v3-directed"
    return RawScenario(name, kind, ft, nb, ny, B, steps, ball, rob[:, :3].copy(), rob[:, 3:].copy(), spin, cmds, hetero_params(kind, B, 700 + kind))


@functools.lru_cache(maxsize=None)
def raw_scenarios(O):
    return tuple([_borrowed_raw(O, c, RAW_SEEDS.get(_raw_name(c), 0)) for c in CASES] + [_directed_raw(O, 0), _directed_raw(O, 1)])


RAW_NAMES = [_raw_name(c) for c in CASES] + ["vss-3v3-directed", "ssl-3v3-directed"]   # raw_scenarios(O), in order


def raw_oracles(O, sc, raw):
    """oracle envs carrying `raw`, reset to the scenario's line-up"""
    refs = []
    for e in range(sc.B):
        r = O.OracleEnv(sc.kind, sc.ft, sc.nb, sc.ny, 25, "f32")
        set_oracle_coefs(r, derive(sc.kind, 25, raw[e]))
        r.reset(sc.ball[e], sc.blue[e], sc.yellow[e] if sc.ny else np.zeros(0))
        if sc.spin is not None:
            st = r.get_state_full()
            st[-1] = sc.spin[e]
            r.set_state_full(st)
        refs.append(r)
    return refs


def run_raw(O, sc, raw, on_step=None):
    """final full states [B, state_dim + 2] float32; on_step(t, refs) after every step"""
    refs = raw_oracles(O, sc, raw)
    for t in range(sc.steps):
        for e, r in enumerate(refs):
            r.step(sc.cmds[t, e])
        if on_step:
            on_step(t, refs)
    out = np.array([r.get_state_full() for r in refs], dtype=np.float32)
    for r in refs:
        r.close()
    return out


class TaskScenario:
    """One handle's whole run: `placement` (ball, blue, yellow) for a task_reset_to after the reset or None; `program`: a list of
    ("fed", actions [n,B,A]) / ("step_n", n) / ("rollout", n) / ("random", n) / ("reset_to", (ball, blue, yellow))"""

    def __init__(self, name, task, kind, ft, nb, ny, B, max_steps, placement, program, raw, seed=0x1234567890ABCDEF, base=1000):
        self.name, self.task, self.kind, self.ft, self.nb, self.ny, self.B, self.max_steps = name, task, kind, ft, nb, ny, B, max_steps
        self.placement, self.program, self.raw, self.seed, self.base = placement, program, raw, seed, base


_TASK_LABEL = {1: "vss-v0", 2: "static-defenders", 3: "dribbling", 4: "contested", 5: "pass-endurance", 6: "scrimmage", 7: "crowded"}


def _task_name(row):
    return f"{_TASK_LABEL[row[0]]}-{row[3]}v{row[4]}"


TASK_NAMES = [_task_name(row) for row in TASKS]   # task_scenarios(O), in order


def _act_dim(task, N):
    return {1: 2, 2: 5, 3: 4, 4: 5, 5: 3, 6: 4 * N, 7: 4 * N}[task]


def _cluster_at_a_wall(O, kind, ft, nb, ny, B, rng):
    """every env: all robots on a grid 2.3 radii apart whose first row stands a few millimetres to centimetres off a side wall, the
    agent (robot 0) in that row, the ball beside it flying obliquely into the wall"""
    f = _field(O, kind, ft, nb, ny)
    N, r = nb + ny, f["r"]
    yl = f["hw"] + f["margin"]
    s = 2.3 * r
    cols = min(N, 6)
    rob = np.zeros((B, N, 3)); ball = np.zeros((B, 4))
    for e in range(B):
        sy = 1.0 if rng.random() < 0.5 else -1.0
        x0 = rng.uniform(-0.3, 0.3) * f["hl"]
        off = rng.uniform(0.002, 0.06)
        for k in range(N):
            row, col = k // cols, k % cols
            rob[e, k] = (x0 + col * s + rng.uniform(-0.1, 0.1) * r, sy * (yl - r - off - row * s), rng.uniform(-180, 180))
        ball[e] = (x0 - rng.uniform(0.6, 1.2) * s, sy * (yl - rng.uniform(0.06, 0.2)), rng.uniform(0.3, 1.5), sy * rng.uniform(0.5, 2.0))
    return ball, rob[:, :nb].copy(), rob[:, nb:].copy()


def _cluster_in_the_field(O, task, kind, ft, nb, ny, B, rng):
    """the single-agent SSL tasks end an episode when the agent or the ball leaves the field lines, so their walls are out of reach:
    every env has the ball fly at the agent a little off-centre from 20 to 30 cm (contact, friction, spin) and the other robots
    stand 2.3 radii and more behind the agent, where its drive may take it"""
    f = _field(O, kind, ft, nb, ny)
    N, r = nb + ny, f["r"]
    rob = np.zeros((B, N, 3)); ball = np.zeros((B, 4))
    for e in range(B):
        a = np.array([rng.uniform(0.5, 1.0) * (-1.0 if task == 3 else 1.0), rng.uniform(-0.5, 0.5)])
        phi = rng.uniform(-np.pi, np.pi)
        if task == 5:   # the receiver; the ball has to stay inside the box the two robots span
            d = np.array([rng.choice([-1.0, 1.0]) * rng.uniform(0.6, 1.0), rng.choice([-1.0, 1.0]) * rng.uniform(0.6, 1.0)])
            phi = np.arctan2(d[1], d[0]) + rng.uniform(-0.4, 0.4)
        u = np.array([np.cos(phi), np.sin(phi)]); t = np.array([-u[1], u[0]])
        rob[e, 0] = (a[0], a[1], rng.uniform(-180, 180))
        for k in range(1, N):
            if task == 5:
                rob[e, k] = (a[0] + d[0], a[1] + d[1], rng.uniform(-180, 180))
                continue
            ring, slot = (k - 1) // 3, (k - 1) % 3
            ang = phi + np.pi + (slot - 1) * (1.1 if ring == 0 else 0.55) + rng.uniform(-0.03, 0.03)
            rad = (2.3 + 2.4 * ring) * r + rng.uniform(0.0, 0.1) * r
            rob[e, k] = (a[0] + rad * np.cos(ang), a[1] + rad * np.sin(ang), rng.uniform(-180, 180))
        sp = rng.uniform(0.8, 2.0)
        ball[e, :2] = a + u * rng.uniform(0.2, 0.3)
        ball[e, 2:] = -u * sp + t * sp * rng.uniform(-0.3, 0.3)
    return ball, rob[:, :nb].copy(), rob[:, nb:].copy()


def directed_lineup(O, task, kind, ft, nb, ny, B, rng):
    """(ball, blue, yellow) of a line-up made for contacts: a cluster at a side wall, or, for the single-agent SSL tasks, in the field"""
    if task in (2, 3, 4, 5):
        return _cluster_in_the_field(O, task, kind, ft, nb, ny, B, rng)
    return _cluster_at_a_wall(O, kind, ft, nb, ny, B, rng)


TAIL = 20   # steps after the directed line-up: shorter than every row's max_episode_steps


def _borrowed_task(O, i, row, seed=0):
    """40 fed actions through task_step, device-drawn actions through task_step_n (17), task_rollout (23) and single steps up to the row's
    step count (auto-resets on the way), then a masked-for-all task_reset_to onto a cluster at a wall and TAIL steps of fed actions: one drive direction per
    env (and robot), a little noise per step"""
    task, kind, ft, nb, ny, B, steps, max_steps = row
    A = _act_dim(task, nb + ny)
    fed = np.random.default_rng(5).uniform(-1, 1, (40, B, A)).astype(np.float32)
    rng = np.random.default_rng(8000 + 100 * i + seed)
    place = directed_lineup(O, task, kind, ft, nb, ny, B, rng)
    tail = np.clip(rng.uniform(-1, 1, (1, B, A)) + rng.uniform(-0.15, 0.15, (TAIL, B, A)), -1, 1).astype(np.float32)
    program = [("fed", fed), ("step_n", 17), ("rollout", 23), ("random", steps - 80), ("reset_to", place), ("fed", tail)]
    return TaskScenario(_task_name(row), task, kind, ft, nb, ny, B, max_steps, None, program, hetero_params(kind, B, 300 + i))


TASK_SEEDS = {"dribbling-1v4": 7, "contested-1v1": 1, "pass-endurance-2v0": 6}   # (line-ups in which the agent meets the ball and a robot; 0 elsewhere)


@functools.lru_cache(maxsize=None)
def task_scenarios(O):
    return tuple(_borrowed_task(O, i, row, TASK_SEEDS.get(_task_name(row), 0)) for i, row in enumerate(TASKS))


def task_oracles(O, sc, raw):
    refs = []
    for e in range(sc.B):
        r = O.OracleEnv(sc.kind, sc.ft, sc.nb, sc.ny, 25, "f32")
        r.task_attach(sc.task, sc.seed, sc.base + e, sc.max_steps)
        set_oracle_coefs(r, derive(sc.kind, 25, raw[e]))
        r.task_reset()
        if sc.placement is not None:
            r.task_reset_to(sc.placement[0][e], sc.placement[1][e], sc.placement[2][e])
        refs.append(r)
    return refs


def task_steps(sc):
    """the scenario's program as one entry per oracle step: (index of the program entry, actions [B,A] or None, last step of its entry)"""
    out = []
    for i, (mode, arg) in enumerate(sc.program):
        if mode == "reset_to":
            out.append((i, arg, True))
            continue
        n = len(arg) if mode == "fed" else arg
        for t in range(n):
            out.append((i, arg[t] if mode == "fed" else None, t == n - 1))
    return out


def run_task(O, sc, raw):
    """final full states [B, state_dim + 2] float32 of the oracle alone"""
    refs = task_oracles(O, sc, raw)
    for i, a, _ in task_steps(sc):
        if sc.program[i][0] == "reset_to":
            for e, r in enumerate(refs):
                r.task_reset_to(a[0][e], a[1][e], a[2][e])
        elif a is None:
            O.vec_task_step(refs, 1)
        else:
            for e, r in enumerate(refs):
                r.task_step(a[e])
    out = np.array([r.get_state_full() for r in refs], dtype=np.float32)
    for r in refs:
        r.close()
    return out


_LIVE = {}


def live_params(O, sc):
    """names of the parameters that are live in `sc` (oracle only; computed once per scenario and process)"""
    key = (type(sc).__name__, sc.name)
    if key not in _LIVE:
        run = run_raw if isinstance(sc, RawScenario) else run_task
        base = run(O, sc, sc.raw).view(np.uint32)
        live = []
        for n in valid_params(sc.kind):
            alt = sc.raw.copy()
            alt[:, NAMES.index(n)] = np.float32(DEFAULTS[sc.kind][n])
            if (run(O, sc, alt).view(np.uint32) != base).any():
                live.append(n)
        _LIVE[key] = live
    return _LIVE[key]


MIN_LIVE = 8   # of its kind's parameters, in every scenario
