"""What the self-play tests share (VecFusedEnv.collect(opponent=...) / rsx_task_collect_selfplay): a numpy restatement of the mirror map
of include/rsx.h, selector opponents, the opponent head's noise restated in float64, the lockstep reference of one self-play step
built from the oracle's existing entry points — up to the first episode end (lockstep_step) and through ends (episode_step,
lockstep_episode_step) —, the directed goal line-up, and the C call on pattern-filled outputs."""
import numpy as np

DOM_OPPONENT = 9          # the opponent head's Philox domain word (include/rsx.h); the agent's is 7
B_SIZES = (5, 13)         # ragged against tiles of 8 envs (8 lanes per env) and of 4 (16 lanes per env)
T = 6
WARM = 3
# the two shapes of include/rsx.h's smallest and largest image: a wrong image offset cannot cancel between them
SHAPE_SMALL = dict(hidden=32, layers=1, hidden_act="relu")
SHAPE_LARGE = dict(hidden=64, layers=2, hidden_act="tanh")
# (robots a side, envs, seed, env_id_base) of every handle tests/test_gpu_selfplay_shapes.py compares with the oracle; what the oracle
# alone does on them (no termination, three truncations per env) is shown in tests/test_selfplay_reference.py
SHAPE_CONFIGS = [(3, 131, 2025, 0), (3, 131, 9, 0), (3, 13, 2025, 0), (2, 37, 23, 0), (3, 37, 2025, 5000), (5, 13, 2025, 0)]


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


def oracle_envs(O, n, seed, base=0, warm=WARM, nb=3, limit=0):
    """n oracle envs of VSS-v0 (f32: the model the GPU implements bit for bit) where VecVSSEnv(n, seed=seed, env_id_base=base) stands
    after reset() and `warm` steps with the engine's own random actions"""
    envs = []
    for e in range(n):
        r = O.OracleEnv(0, 0 if nb <= 3 else 1, nb, nb, 25, "f32")   # (2v2 is VecVSSEnv's field with fewer robots, 5v5 field type 1)
        r.task_attach(1, seed, base + e, limit)
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


def yellow_sincos(r):
    """(sin, cos) of the yellow robots' headings where oracle env r stands, [n_yellow, 2] float32, by the oracle's own sincos_f32 on
    the argument task_obs gives it: what the mirror map needs and the agent's row does not carry"""
    from oracle import oracle as O
    st = r.get_state_full()
    deg2rad = np.float32(np.pi / 180.0)
    out = np.empty((r.n_yellow, 2), dtype=np.float32)
    for k in range(r.n_yellow):
        out[k] = O.sincos(float(np.float32(st[5 + 6 * (r.n_blue + k) + 2]) * deg2rad), "f32")
    return out


def _steps_and_flags(r):
    """(steps, terminated, truncated) of task_out() without its arrays (rsxo_task_out takes NULL for what is not wanted)"""
    import ctypes as C
    term, trunc, steps = C.c_uint8(), C.c_uint8(), C.c_int()
    r._f("rsxo_task_out")(r.h, None, None, C.byref(term), C.byref(trunc), None, None, C.byref(steps), None)
    return steps.value, bool(term.value), bool(trunc.value)


def episode_step(r, agent_action, seated, opponent_rows=False):
    """The lockstep step that goes through episode ends, for any seats (lockstep_episode_step here and in teamplay_helpers).  `seated`:
    [(body index, action [2])], the commands replaced behind task_step.  The oracle's own step yields the commands, advances every draw,
    the step count and the tick and — where ITS trajectory ended — opens the next episode: the state read behind it is then the
    re-placement, which depends on (env id, episode, draw index) alone and not on the trajectory.  The pre-step state and the task
    scalar are put back, the seated commands replaced and the raw step run: obs_eval() / reward_eval() are the replaced step's.  It is
    truncated when the oracle's own step was (the step counts agree as long as both trajectories ended at the same steps) and
    terminated when reward_eval says so.  Then
      both ended                the saved re-placement is put back; the reset row is obs_eval() of it;
      only the replaced one     task_reset(): opens episode + 1, places, clears OU / steps / info, does not move the tick;
      only the oracle's own     its episode counter and OU states cannot be put back: the env is dropped from here on.
    -> (obs row t + 1, reward, terminated, truncated, final_obs or None, dropped); with opponent_rows a seventh entry, the mirror
    images (opponent's obs row t + 1, opponent's final_obs or None)."""
    full, scalar = r.get_state_full(), r.get_scalar()
    first_step = _steps_and_flags(r)[0] == 0
    r.task_step(np.asarray(agent_action, dtype=np.float32))
    _, own_terminated, truncated = _steps_and_flags(r)
    own_ended = own_terminated or truncated
    cmds = r.task_last_cmds()
    placed = r.get_state_full()
    r.set_state_full(full)
    r.set_scalar(scalar)
    for body, action in seated:
        acts = np.zeros(2 * r.N)
        acts[0:2] = np.asarray(action, dtype=np.float64)
        cmds[body] = r.cmds_eval(acts)[0]
    r.step(cmds)
    obs = r.obs_eval().astype(np.float32)
    reward, terminated = r.reward_eval(full[:r.state_dim], cmds, first_step)
    reward = np.float32(reward)
    mir = (lambda row: mirror(row, yellow_sincos(r), r.n_blue)[0]) if opponent_rows else (lambda row: None)   # noqa: E731
    if not (terminated or truncated):
        res = (obs, reward, False, False, None, own_ended)
        return res + ((mir(obs), None),) if opponent_rows else res
    final_opp = mir(obs)   # (the mirror reads the yellow headings of the terminal state: before the env is re-placed)
    if own_ended:
        r.set_state_full(placed)
    else:
        r.task_reset()
    row = r.obs_eval().astype(np.float32)
    res = (row, reward, bool(terminated), truncated, obs, False)
    return res + ((mir(row), final_opp),) if opponent_rows else res


def lockstep_episode_step(r, agent_action, opponent_action, opponent_rows=False):
    """lockstep_step through episode ends (episode_step): yellow 0's command replaced by cmds_eval(opponent_action); with
    opponent_action None no command is replaced and the step is task_step's own (tests/test_selfplay_reference.py)"""
    seated = [] if opponent_action is None else [(r.n_blue, opponent_action)]
    return episode_step(r, agent_action, seated, opponent_rows)


def goal_lineup(n, nb, half_length):
    """The directed line-up of n envs with a goal at rows 1, 2 and 4 of a launch that starts on it (resting robots; checked on the
    oracle in tests/test_selfplay_reference.py): the ball at x = s (half_length - gap), y = 0.02 with velocity (s, 0) m/s, s = +-1
    alternating, gap cycling 0.03 / 0.06 / 0.10 m; blue robots on x = -0.3 and yellow on x = +0.3, facing each other.
    -> (ball [n, 4], blue [n, nb, 3], yellow [n, nb, 3], s [n], gap [n]) as reset_to takes them"""
    e = np.arange(n)
    s = np.where(e % 2 == 0, 1.0, -1.0)
    gap = np.array([0.03, 0.06, 0.10])[e % 3]
    ball = np.stack([s * (half_length - gap), np.full(n, 0.02), s, np.zeros(n)], 1)
    ys = (np.arange(nb) - (nb - 1) / 2.0) * 0.25
    blue = np.zeros((n, nb, 3)); yellow = np.zeros((n, nb, 3))
    blue[:, :, 0], blue[:, :, 1], blue[:, :, 2] = -0.3, ys, 0.0
    yellow[:, :, 0], yellow[:, :, 1], yellow[:, :, 2] = 0.3, ys, 180.0
    return ball, blue, yellow, s, gap


def oracle_alone_ends(O, n, seed, steps=T, warm=WARM, nb=3):
    """how many of n envs end an episode within warm + steps steps of the oracle under its own random actions (the seed's check)"""
    count = 0
    for r in oracle_envs(O, n, seed, warm=0, nb=nb):
        hit = False
        for _ in range(warm + steps):
            r.task_step(None)
            o = r.task_out()
            hit = hit or bool(o["terminated"]) or bool(o["truncated"])
        count += hit
    return count


def filled(torch, dev, fill):
    """shape -> a float32 device tensor whose every word holds the 32-bit pattern `fill`"""
    return lambda shape: torch.full(tuple(shape), 0 if fill is None else fill, dtype=torch.int32, device=dev).view(torch.float32)


def raw_selfplay(torch, _lib, env, pol, params, sigma, opp, opp_params, opp_sigma, noise_seed, steps, fill):
    """env.sim.task_collect_selfplay on outputs every word of which holds the pattern `fill` first (the flags its low byte); returns the
    records under collect()'s names and "flags", device tensors (teamplay_helpers.raw_team's sibling)"""
    dev, B, OD, AD = env.device, env.num_envs, env.sim.obs_dim, env.sim.act_dim
    new = filled(torch, dev, fill)
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    keep = [params.to(dev), None if sigma is None else sigma.to(dev), opp_params.to(dev), None if opp_sigma is None else opp_sigma.to(dev)]
    head = lambda sig: None if sig is None else new((steps, B, AD))   # noqa: E731
    t = {"obs": new((steps, B, OD)), "actions": new((steps, B, AD)), "reward": new((steps, B)),
         "flags": torch.full((steps, B), fill & 0xFF, dtype=torch.uint8, device=dev), "final_obs": new((steps, B, OD)),
         "mean": head(keep[1]), "sample": head(keep[1]), "opponent_obs": new((steps, B, OD)), "opponent_actions": new((steps, B, AD)),
         "opponent_mean": head(keep[3]), "opponent_sample": head(keep[3])}
    rec = _lib.CollectOut(*(ptr(t[k]) for k in ("obs", "actions", "reward", "flags", "final_obs", "mean", "sample")))
    sp = _lib.SelfplayOut(*(ptr(t[k]) for k in ("opponent_obs", "opponent_actions", "opponent_mean", "opponent_sample")))
    env.sim.task_collect_selfplay(pol.spec(), keep[0].data_ptr(), ptr(keep[1]), opp.spec(), keep[2].data_ptr(), ptr(keep[3]), noise_seed, steps,
                                  rec, sp, env._stream())
    torch.cuda.synchronize()   # (the parameter tensors above live until here)
    out = {k: v for k, v in t.items() if v is not None}
    out["terminated"], out["truncated"] = (t["flags"] & 1).bool(), (t["flags"] & 2).bool()
    return out
