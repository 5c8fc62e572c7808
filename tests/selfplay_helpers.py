"""What the self-play tests share (VecFusedEnv.collect(opponent=...) / rsx_task_collect_selfplay): a numpy restatement of the mirror map
of include/rsx.h, selector opponents, the opponent head's noise restated in float64, and the lockstep reference of one self-play step
built from the oracle's existing entry points."""
import numpy as np

DOM_OPPONENT = 9          # the opponent head's Philox domain word (include/rsx.h); the agent's is 7
B_SIZES = (5, 13)         # ragged against tiles of 8 envs (8 lanes per env) and of 4 (16 lanes per env)
T = 6
WARM = 3
# the two shapes of include/rsx.h's smallest and largest image: a wrong image offset cannot cancel between them
SHAPE_SMALL = dict(hidden=32, layers=1, hidden_act="relu")
SHAPE_LARGE = dict(hidden=64, layers=2, hidden_act="tanh")


def own(n, i):
    """first entry of "own" robot i: (x, y, sin, cos, vx, vy, w)"""
    return 4 + 7 * i


def other(n, j):
    """first entry of "other" robot j: (x, y, vx, vy, w)"""
    return 4 + 7 * n + 5 * j


def mirror(obs, other_sincos, n=3):
    """The mirror map: VSS-v0's observation [..., 4 + 12 n] of one team and the sine / cosine of the OTHER team's robots [..., n, 2]
    (which that team's row does not carry) -> the other team's observation and the sine / cosine of the first team's robots.  Team
    colours swapped, the field turned by 180 degrees: positions, linear velocities, sines and cosines negated, angular velocities kept."""
    obs = np.asarray(obs)
    sc = np.asarray(other_sincos)
    out = np.empty_like(obs)
    back = np.empty_like(sc)
    out[..., 0:4] = -obs[..., 0:4]
    for k in range(n):
        a, b = own(n, k), other(n, k)
        # the other team's robot k becomes "own" robot k
        out[..., a + 0:a + 2] = -obs[..., b + 0:b + 2]
        out[..., a + 2:a + 4] = -sc[..., k, :]
        out[..., a + 4:a + 6] = -obs[..., b + 2:b + 4]
        out[..., a + 6] = obs[..., b + 4]
        # this team's robot k becomes "other" robot k
        out[..., b + 0:b + 2] = -obs[..., a + 0:a + 2]
        out[..., b + 2:b + 4] = -obs[..., a + 4:a + 6]
        out[..., b + 4] = obs[..., a + 6]
        back[..., k, :] = -obs[..., a + 2:a + 4]
    return out, back


def own_sincos_entries(n=3):
    """the entries of a row that the other team's row has no counterpart for"""
    return [own(n, k) + c for k in range(n) for c in (2, 3)]


def selector_params(torch, pol, i0, i1):
    """A relu / clip policy whose every fmaf is exact and whose output is (clip(x[i0]), clip(x[i1])): hidden units 2 a and 2 a + 1
    carry +x and -x of component a's entry (relu of each, the difference is x), a second hidden layer copies them (they are >= 0),
    weights 0 or +-1, biases 0."""
    assert pol.hidden_act == "relu" and pol.out_act == "clip" and pol.act_dim == 2
    ts = [torch.zeros(s) for s in pol.shapes]
    for a, i in enumerate((i0, i1)):
        ts[0][2 * a, i] = 1.0
        ts[0][2 * a + 1, i] = -1.0
        ts[-2][a, 2 * a] = 1.0
        ts[-2][a, 2 * a + 1] = -1.0
    if pol.layers == 2:
        for j in range(4):
            ts[2][j, j] = 1.0
    return pol.pack(ts)


def _normal_pair(w0, w1):
    u1 = ((w0 >> 8) + 1) * 2.0 ** -24
    ang = ((w1 >> 8) * 2.0 ** -24 - 0.5) * 2.0 * np.pi
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(ang), rad * np.sin(ang)


def head_eps64(O, dom, seed64, base, tick0, steps, n, act_dim=2):
    """a Gaussian head's standard normals of include/rsx.h in float64, [steps, n, act_dim]: block i >> 2 of philox4x32-7 with counter
    (global env id, 0, tick, dom | block << 8) and key (seed lo, seed hi); component i takes normal i & 3"""
    key = (seed64 & 0xFFFFFFFF, seed64 >> 32)
    eps = np.zeros((steps, n, act_dim))
    for t in range(steps):
        for e in range(n):
            for q in range((act_dim + 3) // 4):
                w = O.philox((base + e, 0, tick0 + t, dom | (q << 8)), key, rounds=7)
                nn = _normal_pair(w[0], w[1]) + _normal_pair(w[2], w[3])
                for c in range(min(4, act_dim - 4 * q)):
                    eps[t, e, 4 * q + c] = nn[c]
    return eps


def oracle_envs(O, n, seed, base=0, warm=WARM, nb=3):
    """n oracle envs of VSS-v0 (f32: the model the GPU implements bit for bit) where VecVSSEnv(n, seed=seed, env_id_base=base) stands
    after reset() and `warm` steps with the engine's own random actions"""
    envs = []
    for e in range(n):
        r = O.OracleEnv(0, 0 if nb == 3 else 1, nb, nb, 25, "f32")
        r.task_attach(1, seed, base + e, 0)
        r.task_reset()
        for _ in range(warm):
            r.task_step(None)
        envs.append(r)
    return envs


def lockstep_step(r, agent_action, opponent_action):
    """One self-play step of oracle env r: the engine's step with yellow 0's command replaced.  task_step(agent_action) yields the
    step's commands and advances every draw (the Ornstein-Uhlenbeck states, yellow 0's included, the step count and the tick); the
    state and the task scalar are then put back, yellow 0's command becomes cmds_eval(opponent_action) and the raw step runs.
    -> (observation, reward, ended): `ended` when either trajectory ended its episode at this step (the row is then not comparable:
    the oracle has re-placed the env, or would not have)."""
    full, scalar = r.get_state_full(), r.get_scalar()
    first_step = r.task_out()["steps"] == 0
    r.task_step(np.asarray(agent_action, dtype=np.float32))
    o = r.task_out()
    ended = bool(o["terminated"]) or bool(o["truncated"])
    cmds = r.task_last_cmds()
    r.set_state_full(full)
    r.set_scalar(scalar)
    acts = np.zeros(2 * r.N)
    acts[0:2] = np.asarray(opponent_action, dtype=np.float64)
    cmds[r.n_blue] = r.cmds_eval(acts)[0]
    r.step(cmds)
    obs = r.obs_eval().astype(np.float32)
    reward, done = r.reward_eval(full[:r.state_dim], cmds, first_step)
    return obs, np.float32(reward), ended or done


def oracle_alone_ends(O, n, seed, steps=T, warm=WARM):
    """how many of n envs end an episode within warm + steps steps of the oracle under its own random actions (the seed's check)"""
    count = 0
    for r in oracle_envs(O, n, seed, warm=0):
        hit = False
        for _ in range(warm + steps):
            r.task_step(None)
            o = r.task_out()
            hit = hit or bool(o["terminated"]) or bool(o["truncated"])
        count += hit
    return count
