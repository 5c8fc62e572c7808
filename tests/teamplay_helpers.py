"""What the team-play tests share (VecFusedEnv.collect(team=..., opponent_team=...) / rsx_task_collect_team): a numpy restatement of the
seat map of include/rsx.h, a Gaussian head's noise with the seat in counter word 1 restated in float64, the lockstep reference of one
team step built from the oracle's existing entry points, and a direct call of the C entry point with seat counts of the caller's choice."""
import numpy as np

import selfplay_helpers as SH

DOM_AGENT, DOM_OPPONENT = 7, SH.DOM_OPPONENT
B_SIZES, T, WARM = SH.B_SIZES, SH.T, SH.WARM


def seat_map(row, i):
    """seat i's row of a side's row [..., 4 + 12 n]: "own" slots 0 and i (7 floats at 4 + 7 k) exchanged, everything else in place.
    Moves float32 values and does no arithmetic on them."""
    row = np.asarray(row)
    out = row.copy()
    a, b = SH.own(0, 0), SH.own(0, i)
    out[..., a:a + 7] = row[..., b:b + 7]
    out[..., b:b + 7] = row[..., a:a + 7]
    return out


def head_eps64(O, dom, seed64, base, tick0, steps, n, seat, act_dim=2):
    """selfplay_helpers.head_eps64 with the seat in counter word 1: the standard normals of seat `seat`'s head in float64,
    [steps, n, act_dim]: philox4x32-7 with counter (global env id, seat, tick, dom | block << 8) and key (seed lo, seed hi)"""
    key = (seed64 & 0xFFFFFFFF, seed64 >> 32)
    eps = np.zeros((steps, n, act_dim))
    for t in range(steps):
        for e in range(n):
            for q in range((act_dim + 3) // 4):
                w = O.philox((base + e, seat, tick0 + t, dom | (q << 8)), key, rounds=7)
                nn = SH._normal_pair(w[0], w[1]) + SH._normal_pair(w[2], w[3])
                for c in range(min(4, act_dim - 4 * q)):
                    eps[t, e, 4 * q + c] = nn[c]
    return eps


def lockstep_step(r, blue_actions, yellow_actions):
    """One team step of oracle env r: the engine's step with the seated robots' commands replaced (selfplay_helpers.lockstep_step for
    any number of seats).  blue_actions [SA, 2]: seat i drives blue i, seat 0 through task_step itself (the engine's own path);
    yellow_actions [SO, 2] (SO may be 0): seat i drives yellow i.  task_step yields the step's commands and advances every draw
    (every Ornstein-Uhlenbeck state, the step count, the tick); the state and the task scalar are then put back, each seated robot's
    command becomes cmds_eval(its action)[0] and the raw step runs.  -> (observation, reward, ended) as selfplay_helpers.lockstep_step."""
    blue = np.asarray(blue_actions, dtype=np.float32).reshape(-1, 2)
    yellow = np.asarray(yellow_actions, dtype=np.float32).reshape(-1, 2)
    full, scalar = r.get_state_full(), r.get_scalar()
    first_step = r.task_out()["steps"] == 0
    r.task_step(blue[0])
    o = r.task_out()
    ended = bool(o["terminated"]) or bool(o["truncated"])
    cmds = r.task_last_cmds()
    r.set_state_full(full)
    r.set_scalar(scalar)
    seated = [(i, blue[i]) for i in range(1, len(blue))] + [(r.n_blue + i, yellow[i]) for i in range(len(yellow))]
    for body, action in seated:
        acts = np.zeros(2 * r.N)
        acts[0:2] = np.asarray(action, dtype=np.float64)
        cmds[body] = r.cmds_eval(acts)[0]
    r.step(cmds)
    obs = r.obs_eval().astype(np.float32)
    reward, done = r.reward_eval(full[:r.state_dim], cmds, first_step)
    return obs, np.float32(reward), ended or done


def lockstep_episode_step(r, blue_actions, yellow_actions, opponent_rows=False):
    """lockstep_step through episode ends (selfplay_helpers.episode_step) for any number of seats: blue seat 0 through task_step itself,
    blue seats 1.. and every yellow seat by replaced commands.  One blue seat and no yellow seat: no command is replaced and the step
    is task_step's own.  -> (obs row t + 1, reward, terminated, truncated, final_obs or None, dropped): seat 0's rows; the other
    seats' are their seat_map, the opponent's the mirror (opponent_rows)."""
    blue = np.asarray(blue_actions, dtype=np.float32).reshape(-1, 2)
    yellow = np.asarray(yellow_actions, dtype=np.float32).reshape(-1, 2)
    seated = [(i, blue[i]) for i in range(1, len(blue))] + [(r.n_blue + i, yellow[i]) for i in range(len(yellow))]
    return SH.episode_step(r, blue[0], seated, opponent_rows)


def raw_team(torch, _lib, env, pol, params, sigma, seats, opp, opp_params, opp_sigma, opp_seats, noise_seed, steps, final_obs=True, fill=None):
    """env.sim.task_collect_team with the seat counts as given — (1, 0) and (1, 1) included, which collect() never asks for — on tensors
    made here; returns the batch under collect()'s names, seat axis behind B, device tensors.  `fill`: a 32-bit pattern every output
    word holds before the call (the flags its low byte), instead of torch.empty's memory and final_obs's zeros; "flags" is then
    returned too."""
    dev, B, OD, AD = env.device, env.num_envs, env.sim.obs_dim, env.sim.act_dim
    f32 = dict(dtype=torch.float32, device=dev)
    empty = zeros = SH.filled(torch, dev, fill)
    if fill is None:
        empty, zeros = (lambda s: torch.empty(s, **f32)), (lambda s: torch.zeros(s, **f32))   # noqa: E731
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    keep = [params.to(dev), None if sigma is None else sigma.to(dev), None if opp_params is None else opp_params.to(dev),
            None if opp_sigma is None else opp_sigma.to(dev)]

    def side(S, sig):
        if S == 0:
            return {}, _lib.TeamSideOut()
        t = {"obs": empty((steps, B, S, OD)), "actions": empty((steps, B, S, AD)),
             "mean": None if sig is None else empty((steps, B, S, AD)), "sample": None if sig is None else empty((steps, B, S, AD)),
             "final_obs": zeros((steps, B, S, OD)) if final_obs else None, "next_obs": empty((B, S, OD))}
        return t, _lib.TeamSideOut(*(ptr(t[k]) for k in ("obs", "actions", "mean", "sample", "final_obs", "next_obs")))

    rew = empty((steps, B))
    flags = torch.full((steps, B), (fill or 0) & 0xFF, dtype=torch.uint8, device=dev)
    a, a_out = side(seats, keep[1])
    o, o_out = side(opp_seats, keep[3])
    env.sim.task_collect_team(pol.spec(), keep[0].data_ptr(), ptr(keep[1]), seats, None if opp is None else opp.spec(), ptr(keep[2]),
                              ptr(keep[3]), opp_seats, noise_seed, steps, _lib.TeamOut(ptr(rew), ptr(flags), a_out, o_out), env._stream())
    torch.cuda.synchronize()   # (the parameter tensors above live until here)
    out = {"reward": rew, "terminated": (flags & 1).bool(), "truncated": (flags & 2).bool()}
    if fill is not None:
        out["flags"] = flags
    out.update({k: v for k, v in a.items() if v is not None})
    out.update({"opponent_" + k: v for k, v in o.items() if v is not None})
    return out
