"""VecFusedEnv.collect(team=..., opponent_team=...) / rsx_task_collect_team: VSS-v0 collection with every robot of a side driven by that
side's policy, each seat from its own row.  Self-play's sizes, at which nothing divides evenly: B = 5 and 13 envs (ragged against tiles of
8 and of 4 envs), T = 6, WARM = 3, 1 x 32 relu against 2 x 64 tanh and the reverse.  Comparisons are on bit patterns (or `==`, where
signed zeros are to compare equal) unless a bound is named next to them."""
import numpy as np
import pytest

import selfplay_helpers as SH
import teamplay_helpers as TH
import test_gpu_policy_lookahead as PL   # _same, _dense, _make and the float32 bound of dense policies (taken from there, not re-derived)
import test_gpu_selfplay as SP           # _host, _policies, _start, _check_mirror

pytestmark = pytest.mark.gpu

T, WARM = TH.T, TH.WARM
_same, _dense = PL._same, PL._dense
_host, _policies, _start, _check_mirror = SP._host, SP._policies, SP._start, SP._check_mirror
CASES, IDS = SP.CASES, SP.IDS
# (actor seats, opponent seats) with n robots a side: None stands for n
SEATS = [(None, 0), (None, 1), (None, None), (1, None)]
SEAT_IDS = ["n-0", "n-1", "n-n", "1-n"]


def _team_kw(sa, so, po, o, n=3, **head):
    """collect()'s keywords for seat counts (sa, so), sa in (1, n), so in (0, 1, n)"""
    kw = dict(team=sa == n, opponent_team=so == n)
    if so:
        kw.update(opponent=po, opponent_params=o, **head)
    return kw


def _check_seat_rows(rows, n, tag):
    """[..., S, obs_dim]: every seat's row is the seat map of seat 0's, in bits"""
    for i in range(rows.shape[-2]):
        assert _same(rows[..., i, :], TH.seat_map(rows[..., 0, :], i)), (tag, i)
    if rows.shape[-2] > 1:
        assert not _same(rows[..., 1, :], rows[..., 0, :]), (tag, "uninformative: seats 0 and 1 see the same row")


# ---- 1. reduction to the verified kernels ----
@pytest.mark.parametrize("B,agent,opp", CASES, ids=IDS)
def test_one_seat_a_side_is_selfplay_and_one_seat_is_the_collector(B, agent, opp):
    import torch
    from rsoccer_amd import _lib, vec
    kw = dict(device=0, seed=2025, max_episode_steps=7)   # TimeLimit 7, three warm steps: every env is re-placed at row 3
    ls, ols = torch.tensor([-1.0, -0.7]), torch.tensor([-0.5, -1.2])
    for so in (1, 0):
        env, twin = vec.VecVSSEnv(B, **kw), vec.VecVSSEnv(B, **kw)
        for e in (env, twin):
            _start(torch, e)
        pa, a, po, o = _policies(torch, env, agent, opp)
        got = _host(TH.raw_team(torch, _lib, env, pa, a, ls.exp(), 1, po if so else None, o if so else None, ols.exp() if so else None, so,
                                17, T))
        more = dict(opponent=po, opponent_params=o, opponent_log_std=ols) if so else {}
        want = _host(twin.collect(pa, a, T, log_std=ls, noise_seed=17, return_final_obs=True, **more))
        assert want["truncated"][3].all()
        for k in ("reward", "terminated", "truncated"):
            assert _same(got[k], want[k]), (so, k)
        names = ["obs", "actions", "mean", "sample", "final_obs"]
        if so:
            names += ["opponent_obs", "opponent_actions", "opponent_mean", "opponent_sample"]
        else:
            assert not any(k.startswith("opponent_") for k in got)
        for k in names:
            assert got[k].shape[2] == 1 and _same(got[k][:, :, 0], want[k]), (so, k)
        assert _same(got["next_obs"][:, 0], want["next_obs"]) and _same(env._t["obs"].cpu().numpy(), want["next_obs"])
        assert np.array_equal(env.checkpoint(), twin.checkpoint()) and env.metrics() == twin.metrics(), so
        assert env.sim.task_tick() == twin.sim.task_tick() == WARM + T
        env.close(); twin.close()


# ---- 2. seat rows ----
@pytest.mark.parametrize("B,agent,opp", CASES, ids=IDS)
def test_every_seat_sees_its_own_row(B, agent, opp):
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(B, device=0, seed=2025, max_episode_steps=7)
    _start(torch, env)
    pa, a, po, o = _policies(torch, env, agent, opp)
    out = _host(env.collect(pa, a, T, return_final_obs=True, opponent=po, opponent_params=o, team=True, opponent_team=True))
    assert set(out) == {"obs", "actions", "reward", "terminated", "truncated", "next_obs", "final_obs", "opponent_obs", "opponent_actions",
                        "opponent_next_obs", "opponent_final_obs"}
    for pre in ("", "opponent_"):
        assert out[pre + "obs"].shape == (T, B, 3, 40) and out[pre + "actions"].shape == (T, B, 3, 2)
        assert out[pre + "final_obs"].shape == (T, B, 3, 40) and out[pre + "next_obs"].shape == (B, 3, 40)
        for k in ("obs", "final_obs", "next_obs"):
            _check_seat_rows(out[pre + k], 3, pre + k)
    assert out["reward"].shape == out["terminated"].shape == out["truncated"].shape == (T, B)
    # seat 0 of the two sides: self-play's mirror check
    _check_mirror({"obs": out["obs"][:, :, 0], "opponent_obs": out["opponent_obs"][:, :, 0]}, tag="obs")
    _check_mirror({"obs": out["final_obs"][3][:, 0], "opponent_obs": out["opponent_final_obs"][3][:, 0]}, tag="final_obs")
    _check_mirror({"obs": out["next_obs"][:, 0], "opponent_obs": out["opponent_next_obs"][:, 0]}, tag="next_obs")
    # final_obs: rows of ended steps only (TimeLimit 7 after three warm steps: row 3), every seat's
    assert out["truncated"][3].all() and out["truncated"].sum() == B and not out["terminated"].any()
    for pre in ("", "opponent_"):
        f = out[pre + "final_obs"]
        assert np.all(np.abs(f[3]).max(axis=-1) > 0.05) and not f[np.arange(T) != 3].any(), pre
    # the handle's buffers hold seat 0's rows
    assert _same(env._t["obs"].cpu().numpy(), out["next_obs"][:, 0])
    assert _same(env._t["final_obs"].cpu().numpy(), out["final_obs"][3][:, 0])
    env.close()


# ---- 3. forwards ----
@pytest.mark.parametrize("layers,hidden", [(2, 64), (1, 32)])
def test_selector_policies_are_evaluated_exactly_on_every_seat(layers, hidden):
    import torch
    from rsoccer_amd import vec
    from rsoccer_amd.vec.policy import MLPPolicy
    B = 13 if layers == 2 else 5
    env = vec.VecVSSEnv(B, device=0, seed=11)
    _start(torch, env)
    pa = MLPPolicy(40, 2, hidden=hidden, layers=layers, hidden_act="relu", out_act="clip")
    po = MLPPolicy(40, 2, hidden=96 - hidden, layers=3 - layers, hidden_act="relu", out_act="clip")
    # own slot 0 first (where a missing exchange shows: every seat would answer with robot 0's entries), then the ball, another own
    # slot, an other robot
    for i0, i1 in ((SH.own(3, 0), SH.own(3, 0) + 2), (0, SH.own(3, 0) + 6), (SH.own(3, 1) + 1, SH.own(3, 2) + 3), (SH.other(3, 0) + 4, SH.other(3, 1))):
        a, o = SH.selector_params(torch, pa, i0, i1), SH.selector_params(torch, po, i1, i0)
        out = _host(env.collect(pa, a, T, opponent=po, opponent_params=o, team=True, opponent_team=True))
        for pre, pol, w, (j0, j1) in (("", pa, a, (i0, i1)), ("opponent_", po, o, (i1, i0))):
            rows, acts = out[pre + "obs"], out[pre + "actions"]
            want = np.clip(rows[..., [j0, j1]], -1.0, 1.0)
            assert np.all(acts == want), (pre, i0, i1)   # (a selected zero comes out as +0.0 whatever its sign: ==)
            host = pol.forward(torch.from_numpy(rows), w, dtype=torch.float32).numpy()
            assert _same(acts, host), (pre, i0, i1)       # in bits: the host's float32 forward of the RECORDED row, every operation exact
            assert (want != 0.0).mean() > 0.5 and np.abs(want).max() > 0.01, (pre, i0, i1, "uninformative")
        if i0 == SH.own(3, 0):   # the seats answered with different robots' entries
            assert not np.array_equal(out["actions"][:, :, 0], out["actions"][:, :, 1]) and not np.array_equal(out["actions"][:, :, 1], out["actions"][:, :, 2])
            # seat 1 answered with blue 1's entries, which seat 0's row holds in own slot 1
            assert np.all(out["actions"][:, :, 1] == np.clip(out["obs"][:, :, 0][..., [SH.own(3, 1), SH.own(3, 1) + 2]], -1.0, 1.0))
    env.close()


@pytest.mark.parametrize("B,agent,opp", CASES, ids=IDS)
def test_dense_policies_are_within_the_float32_bound_on_every_seat(B, agent, opp):
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(B, device=0, seed=2025)
    _start(torch, env)
    pa, a, po, o = _policies(torch, env, agent, opp)
    out = _host(env.collect(pa, a, T, log_std=-1.0, noise_seed=3, opponent=po, opponent_params=o, opponent_log_std=-1.0, team=True,
                            opponent_team=True))
    for pre, pol, w in (("", pa, a), ("opponent_", po, o)):
        for s in range(3):
            rows = torch.from_numpy(np.ascontiguousarray(out[pre + "obs"][:, :, s])).reshape(-1, 40)
            want, bound = PL._forward_with_bound(torch, pol, rows, w)   # MLPPolicy.forward in float64 and the dense policy test's bound
            # mean is the output accumulator BEFORE out_act: the activation is applied here in float64 (1-Lipschitz, exact to 1e-16)
            got = torch.tanh(torch.from_numpy(np.ascontiguousarray(out[pre + "mean"][:, :, s])).reshape(-1, 2).double())
            err = (got - want).abs().numpy()
            print(f"B={B} {pre or 'agent_'}seat {s}: largest error {err.max():.3e}, worst error / bound {(err / bound.numpy()).max():.3f}")
            assert np.all(err <= bound.numpy()), (pre, s)
    env.close()


# ---- 4. heads ----
def test_every_seats_gaussian_head(oracle_mod):
    import torch
    from rsoccer_amd import vec
    from rsoccer_amd.vec.policy import MLPPolicy
    B, base, seed64 = 13, 11, 0x0123456789ABCDEF   # (distinct halves: the key is (lo, hi))
    envs = [vec.VecVSSEnv(B, device=0, seed=9, env_id_base=base) for _ in range(2)]
    for e in envs:
        _start(torch, e)
    env, twin = envs
    pols, ws, biases = [], [], [torch.tensor([0.3, -0.7]), torch.tensor([-0.2, 0.5])]
    for shape, bias in zip((SH.SHAPE_SMALL, SH.SHAPE_LARGE), biases):   # zero weights and a bias: every seat's mean is the bias, in bits
        p = MLPPolicy(40, 2, out_act="clip", **shape)
        ts = [torch.zeros(s) for s in p.shapes]
        ts[-1][:] = bias
        pols.append(p); ws.append(p.pack(ts))
    sigs = [np.array([0.5, 0.25], dtype=np.float32), np.array([0.125, 2.0], dtype=np.float32)]
    tick0 = env.sim.task_tick()
    assert tick0 == WARM
    got = _host(env.collect(pols[0], ws[0], T, log_std=np.log(sigs[0]), noise_seed=seed64, opponent=pols[1], opponent_params=ws[1],
                            opponent_log_std=np.log(sigs[1]), team=True, opponent_team=True))
    eps = {}
    for pre, dom, bias, sig in (("", TH.DOM_AGENT, biases[0], sigs[0]), ("opponent_", TH.DOM_OPPONENT, biases[1], sigs[1])):
        assert got[pre + "mean"].shape == got[pre + "sample"].shape == (T, B, 3, 2) and got[pre + "log_prob"].shape == (T, B, 3)
        assert _same(got[pre + "mean"], np.broadcast_to(bias.numpy(), (T, B, 3, 2)).copy())
        bound = 1e-5 * max(float(sig.max()), 1.0)   # test_gpu_collect.py::test_the_gaussian_head's (sigma = exp(log(sig)): maybe an ulp off sig)
        for s in range(3):
            eps[pre, s] = TH.head_eps64(oracle_mod, dom, seed64, base, tick0, T, B, s)
            want = got[pre + "mean"][:, :, s].astype(np.float64) + sig.astype(np.float64) * eps[pre, s]
            err = np.abs(got[pre + "sample"][:, :, s].astype(np.float64) - want)
            print(f"{pre or 'agent_'}seat {s}: max |sample - float64 restatement with the seat in counter word 1| {err.max():.3e} (bound {bound:.1e})")
            assert err.max() <= bound, (pre, s)
            assert 0.7 < eps[pre, s].std() < 1.3 and abs(eps[pre, s].mean()) < 0.3
        assert _same(got[pre + "actions"], np.clip(got[pre + "sample"], -1.0, 1.0))
        z = (got[pre + "sample"].astype(np.float64) - got[pre + "mean"]) / sig
        lp = (-0.5 * z * z - np.log(sig.astype(np.float64)) - 0.5 * np.log(2 * np.pi)).sum(-1)
        assert np.abs(got[pre + "log_prob"] - lp).max() <= 1e-4 * max(1.0, np.abs(lp).max())
    # the noise differs between seats and between the two sides
    keys = list(eps)
    for i, k in enumerate(keys):
        for q in keys[i + 1:]:
            assert (np.abs(eps[k] - eps[q]) > 1e-3).mean() > 0.9, (k, q)
            dev = (got[k[0] + "sample"][:, :, k[1]] - got[k[0] + "mean"][:, :, k[1]]) / (sigs[0] if k[0] == "" else sigs[1])
            deq = (got[q[0] + "sample"][:, :, q[1]] - got[q[0] + "mean"][:, :, q[1]]) / (sigs[0] if q[0] == "" else sigs[1])
            assert (np.abs(dev - deq) > 1e-3).mean() > 0.9, (k, q)
    # a twin collected WITHOUT seats or an opponent: at step 0 the states still agree, so seat 0's row, mean and sample are the same bits
    plain = _host(twin.collect(pols[0], ws[0], T, log_std=np.log(sigs[0]), noise_seed=seed64))
    for k in ("obs", "mean", "sample", "actions"):
        assert _same(got[k][0][:, 0], plain[k][0]), k
    assert _same(got["sample"][:, :, 0], plain["sample"]), "seat 0 draws what collect() draws at every step (the mean is the bias)"
    assert not _same(got["obs"][T - 1][:, 0], plain["obs"][T - 1]), "uninformative: the seats did not change the trajectory"
    for e in envs:
        e.close()


# ---- 5. the step is the engine's step with the seated commands replaced ----
def _lockstep(oracle_mod, torch, vec, B, agent, opp, sa, so, n=3, make=None, seed=2025, steps=T, tail=0):
    """collect() with seats (sa, so) against the lockstep oracle; returns (env, refs, out, left_out) with env and refs after the call"""
    assert sa == n or so == n, "a seat count of n on one side at least: collect() takes its other paths otherwise"
    env = make() if make else vec.VecVSSEnv(B, device=0, seed=seed)
    _start(torch, env)
    refs = SH.oracle_envs(oracle_mod, B, seed, nb=n)
    torch.cuda.synchronize()
    obs0 = env._t["obs"].cpu().numpy()
    for e, r in enumerate(refs):   # the two sides start from the same instant
        assert _same(obs0[e], r.task_out()["obs"].astype(np.float32)), e
    pa, a, po, o = _policies(torch, env, agent, opp)
    out = _host(env.collect(pa, a, steps, log_std=-1.0, noise_seed=17, **_team_kw(sa, so, po, o, n=n, opponent_log_std=-0.5)))
    rows = np.concatenate([out["obs"][:, :, 0], out["next_obs"][None, :, 0]], 0)   # seat 0's row t + 1; behind the last step: next_obs
    none = np.zeros((steps, B, 0, 2), dtype=np.float32)
    yellow = out["opponent_actions"] if so else none
    left_out, compared = set(), 0
    for t in range(steps):
        for e, r in enumerate(refs):
            if e in left_out:
                continue
            obs, reward, ended = TH.lockstep_step(r, out["actions"][t, e], yellow[t, e])
            if ended or out["terminated"][t, e] or out["truncated"][t, e]:
                left_out.add(e)   # from the first step on at which either trajectory ends an episode
                continue
            assert _same(rows[t + 1, e], obs), (t, e, np.argwhere(rows[t + 1, e] != obs)[:4].tolist())
            assert _same(out["reward"][t, e], reward), (t, e, out["reward"][t, e], reward)
            compared += 1
    print(f"B={B} seats ({sa}, {so}): {compared} rows equal the lockstep oracle bit for bit, envs left out {sorted(left_out)}")
    assert len(left_out) * 8 <= B, left_out
    return env, refs, out, left_out


# Seed 2025: under the oracle's own random actions none of the 13 (nor of the 5) envs ends an episode within WARM + T = 9 steps of its
# reset (selfplay_helpers.oracle_alone_ends, run on the CPU: 0 of 13, 0 of 5), so the cap of one env in eight is the team trajectories'
# to keep: nine steps after a placement no robot has carried the ball into a goal under these policies either.
@pytest.mark.parametrize("seats", SEATS, ids=SEAT_IDS)
@pytest.mark.parametrize("B,agent,opp", CASES, ids=IDS)
def test_the_step_is_the_engines_step_with_the_seated_commands_replaced(oracle_mod, B, agent, opp, seats):
    import torch
    from rsoccer_amd import vec
    assert SH.oracle_alone_ends(oracle_mod, B, 2025) * 8 <= B
    sa, so = (3 if s is None else s for s in seats)
    env, _, out, _ = _lockstep(oracle_mod, torch, vec, B, agent, opp, sa, so)
    # informative: a seated robot other than blue 0 and yellow 0 moved under its policy and not under its Ornstein-Uhlenbeck noise — a
    # twin stepped with the SAME blue-0 (and yellow-0) actions but without the other seats ends up elsewhere
    twin = vec.VecVSSEnv(B, device=0, seed=2025)
    _start(torch, twin)
    pa, a, po, o = _policies(torch, twin, agent, opp)
    plain = _host(twin.collect(pa, a, T, log_std=-1.0, noise_seed=17, **({"opponent": po, "opponent_params": o, "opponent_log_std": -0.5} if so else {})))
    slot = SH.own(3, 1) if sa == 3 else SH.other(3, 1)   # blue 1 in seat 0's row, or yellow 1
    assert _same(out["obs"][0][:, 0], plain["obs"][0])
    assert not _same(out["obs"][2][:, 0, slot:slot + 2], plain["obs"][2][:, slot:slot + 2]), "the seated robot moved as under its noise"
    moved = out["actions"][:, :, 1:] if sa == 3 else out["opponent_actions"][:, :, 1:]
    assert np.abs(moved).max() > 0.05
    env.close(); twin.close()


# ---- 6. ends inside the launch ----
def test_episodes_end_inside_the_launch():
    import torch
    from rsoccer_amd import vec
    B, limit = 5, 4
    kw = dict(device=0, seed=4, max_episode_steps=limit)
    env, twin = vec.VecVSSEnv(B, **kw), vec.VecVSSEnv(B, **kw)
    for e in (env, twin):
        e.reset()
        e.step(None)   # one step with a plain step(): the time limit falls on row 2 of the launch, and again on row 6, outside it
    torch.cuda.synchronize()
    before = env.metrics()
    pa, a, po, o = _policies(torch, env, SH.SHAPE_SMALL, SH.SHAPE_LARGE)
    out = _host(env.collect(pa, a, T, return_final_obs=True, opponent=po, opponent_params=o, team=True, opponent_team=True))
    row = limit - 2
    assert out["truncated"][row].all() and not out["terminated"].any(), (out["truncated"], out["terminated"])
    assert out["truncated"].sum() == B, "every env is truncated at the same row, and only there"
    for pre in ("", "opponent_"):
        f = out[pre + "final_obs"]
        assert np.all(np.abs(f[row]).max(axis=-1) > 0.05) and not f[np.arange(T) != row].any(), pre
        _check_seat_rows(f[row], 3, pre + "final_obs")
        _check_seat_rows(out[pre + "obs"], 3, pre + "obs")
    assert _same(out["final_obs"][row][:, 0], env._t["final_obs"].cpu().numpy())
    vel = [2, 3] + [SH.own(3, k) + c for k in range(3) for c in (4, 5, 6)] + [SH.other(3, k) + c for k in range(3) for c in (2, 3, 4)]
    for pre in ("", "opponent_"):   # the first rows of the next episode: everything at rest, on every seat
        assert np.all(out[pre + "obs"][row + 1][..., vel] == 0.0) and np.abs(out[pre + "obs"][row][..., vel]).max() > 0.0, pre
    _check_mirror({"obs": out["obs"][:, :, 0], "opponent_obs": out["opponent_obs"][:, :, 0]}, tag="across the reset")
    # placement depends only on env id and episode: seat 0's row behind the reset is a plain-collect twin's reset row
    plain = _host(twin.collect(pa, a, T, return_final_obs=True))
    assert plain["truncated"][row].all()
    assert _same(out["obs"][row + 1][:, 0], plain["obs"][row + 1])
    assert not _same(out["obs"][row][:, 0], plain["obs"][row]), "uninformative: the trajectories did not differ before the reset"
    after = env.metrics()
    assert after["episodes"] - before["episodes"] == B and after["truncated_episodes"] - before["truncated_episodes"] == B
    assert after["env_steps"] - before["env_steps"] == B * T
    env.close(); twin.close()


# ---- 7. handing back ----
def test_the_env_can_be_handed_back(oracle_mod):
    import torch
    from rsoccer_amd import vec
    B = 5
    env, refs, _, left_out = _lockstep(oracle_mod, torch, vec, B, SH.SHAPE_LARGE, SH.SHAPE_SMALL, 3, 3)
    blob = env.checkpoint()
    fresh = vec.VecVSSEnv(B, device=0, seed=2025)
    fresh.reset()
    fresh.restore(blob)
    acts = np.random.default_rng(3).uniform(-1, 1, (4, B, 2)).astype(np.float32)
    compared = 0
    for t in range(4):   # step() continues where the lockstep oracle, continued by task_step, continues
        for e in (env, fresh):
            e.step(torch.from_numpy(acts[t]).to(env.device))
        torch.cuda.synchronize()
        for k in ("obs", "reward", "terminated", "truncated", "final_obs"):
            assert torch.equal(env._t[k], fresh._t[k]), (t, k)
        obs, rew = fresh._t["obs"].cpu().numpy(), fresh._t["reward"].cpu().numpy()
        for e, r in enumerate(refs):
            if e in left_out:
                continue
            r.task_step(acts[t, e])
            o = r.task_out()
            if o["terminated"] or o["truncated"]:
                left_out.add(e)
                continue
            assert _same(obs[e], o["obs"].astype(np.float32)), (t, e)
            assert _same(rew[e], np.float32(o["reward"])), (t, e)
            compared += 1
    assert len(left_out) * 8 <= B and compared >= 4 * (B - 1)
    # ... and so do plain collect() and collect(opponent=)
    pa, a, po, o = _policies(torch, env, SH.SHAPE_LARGE, SH.SHAPE_SMALL)
    for more in ({}, dict(opponent=po, opponent_params=o)):
        outs = [_host(e.collect(pa, a, T, log_std=-1.0, noise_seed=5, **more)) for e in (env, fresh)]
        for k, v in outs[0].items():
            assert _same(v, outs[1][k]), k
    assert np.array_equal(env.checkpoint(), fresh.checkpoint())
    env.close(); fresh.close()


# ---- 8. shapes ----
def _shape_run(torch, env, B=13):
    _start(torch, env)
    pa, a, po, o = _policies(torch, env, SH.SHAPE_SMALL, SH.SHAPE_LARGE)
    out = _host(env.collect(pa, a, T, log_std=-1.0, noise_seed=5, return_final_obs=True, opponent=po, opponent_params=o, opponent_log_std=-1.0,
                            team=True, opponent_team=True))
    blob = env.checkpoint()
    env.close()
    return out, blob


def test_every_handle_shape_gives_the_same_bits(monkeypatch):
    import torch
    from rsoccer_amd import vec
    kw = dict(device=0, seed=29, max_episode_steps=7)   # TimeLimit 7, three warm steps: every env is re-placed at row 3
    want, blob = _shape_run(torch, vec.VecVSSEnv(13, **kw))
    assert want["truncated"][3].all() and want["obs"].shape == (T, 13, 3, 40)
    monkeypatch.setenv("RSX_LANES_PER_ENV", "16")
    env = vec.VecVSSEnv(13, **kw)
    assert env.sim.task_layout() == "16-lanes-per-env"
    got, blob16 = _shape_run(torch, env)
    monkeypatch.delenv("RSX_LANES_PER_ENV")
    for k in want:
        assert _same(got[k], want[k]), ("16 lanes per env", k)
    assert np.array_equal(blob16, blob)
    monkeypatch.setenv("RSX_LAYOUT", "epl")
    env = vec.VecVSSEnv(13, **kw)
    assert env.sim.task_layout() == "one-lane-per-env"
    got, blob1 = _shape_run(torch, env)
    monkeypatch.delenv("RSX_LAYOUT")
    for k in want:
        assert _same(got[k], want[k]), ("one lane per env", k)
    env = vec.VecVSSEnv(13, physics={}, **kw)   # per-env physics on, at the compiled-in values
    got, _ = _shape_run(torch, env)
    for k in want:
        assert _same(got[k], want[k]), ("per-env physics", k)


def test_5v5_runs_the_native_16_lane_variant(oracle_mod):
    import torch
    from rsoccer_amd import vec
    B = 5
    make = lambda: PL._make(vec, "VecVSS5v5", B, device=0, seed=2025)   # noqa: E731
    assert SH.oracle_alone_ends(oracle_mod, B, 2025, nb=5) * 8 <= B
    env, _, out, _ = _lockstep(oracle_mod, torch, vec, B, SH.SHAPE_LARGE, SH.SHAPE_LARGE, 5, 5, n=5, make=make)   # check 5
    assert env.sim.obs_dim == 64 and env.sim.task_layout() == "16-lanes-per-env"
    assert out["obs"].shape == (T, B, 5, 64) and out["opponent_actions"].shape == (T, B, 5, 2)
    for pre in ("", "opponent_"):                                                                                   # check 2
        for k in ("obs", "next_obs"):
            _check_seat_rows(out[pre + k], 5, pre + k)
    _check_mirror({"obs": out["obs"][:, :, 0], "opponent_obs": out["opponent_obs"][:, :, 0]}, n=5, tag="5v5")
    assert np.abs(out["actions"][:, :, 4]).max() > 0.05 and np.abs(out["opponent_actions"][:, :, 4]).max() > 0.05
    env.close()


# ---- 9. graph capture ----
def test_team_play_replays_from_a_graph():
    import torch
    from rsoccer_amd import vec
    B = 5
    envs = [vec.VecVSSEnv(B, device=0, seed=17, max_episode_steps=7) for _ in range(2)]
    for e in envs:
        _start(torch, e)
        e.enable_graph_capture()
    env, twin = envs
    pa, a, po, o = _policies(torch, env, SH.SHAPE_SMALL, SH.SHAPE_LARGE)
    a, o = a.to(env.device), o.to(env.device)
    ls = torch.full((2,), -1.0, device=env.device)

    def run(e):
        return e.collect(pa, a, T, log_std=ls, noise_seed=99, return_final_obs=True, opponent=po, opponent_params=o, opponent_log_std=ls,
                         team=True, opponent_team=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # the eager call, which is also torch's warm-up before a capture
        run(env)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run(env)
    assert env.sim.task_tick() == WARM + T   # capturing enqueued nothing
    run(twin)
    for i in range(2):
        g.replay()
        want = run(twin)
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(out[k], want[k]), (f"replay {i}", k)
    assert env.sim.task_tick() == twin.sim.task_tick() == WARM + 3 * T
    assert np.array_equal(env.checkpoint(), twin.checkpoint()) and env.metrics() == twin.metrics()
    for e in envs:
        e.close()


# ---- 10. downstream ----
def test_seat_rows_feed_advantages_and_ppo_update():
    import torch
    import test_gpu_ppo_update as PU   # _nets, _params, _piecewise, _state_bits, _bits
    from rsoccer_amd import vec
    from rsoccer_amd.vec.optim import PPOOptimizer
    from rsoccer_amd.vec.policy import seat_rows
    B = 13
    env = vec.VecVSSEnv(B, device=0, seed=2025, max_episode_steps=7)
    _start(torch, env)
    dev = env.device
    pol, critic = PU._nets()
    start = PU._params(torch, pol, critic, 31, dev)
    p, ls, cp = start
    batch = env.collect(pol, p, T, log_std=ls, noise_seed=8, critic=critic, critic_params=cp, gamma=0.97, lam=0.9, team=True)
    assert batch["value"].shape == batch["advantage"].shape == batch["return"].shape == (T, B, 3) and "final_obs" in batch
    rows = seat_rows(batch)
    assert rows["obs"].shape == (T, B * 3, 40) and rows["reward"].shape == (T, B * 3)
    want = env.advantages(rows, critic, cp, gamma=0.97, lam=0.9)
    torch.cuda.synchronize()
    for k in ("value", "advantage", "return"):
        assert torch.equal(PU._bits(batch[k].reshape(T, B * 3)), PU._bits(want[k])), k
        assert torch.equal(PU._bits(rows[k]), PU._bits(want[k])), k
    assert bool(batch["truncated"][3].all()) and float(batch["advantage"].abs().max()) > 0.0
    # the seats of an env share reward and flags and differ in what they saw: their values differ
    assert not torch.equal(batch["value"][:, :, 0], batch["value"][:, :, 1])
    # one ppo_update on the seat rows equals the sequence of its public pieces on the same rows
    loss = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01)
    EPOCHS, MB, SEED = 2, 2, 77
    a, b = [x.clone() for x in start], [x.clone() for x in start]
    oa, ob = (PPOOptimizer(pol, critic, device=dev, lr=1e-3, max_grad_norm=0.5) for _ in range(2))
    out = env.ppo_update(rows, pol, *a[:2], critic, a[2], oa, epochs=EPOCHS, minibatches=MB, normalize_advantage=True, seed=SEED, **loss)
    piece, _ = PU._piecewise(torch, env, rows, pol, critic, b, ob, EPOCHS, MB, SEED, True, None, **loss)
    torch.cuda.synchronize()
    assert tuple(out["stats"].shape) == (EPOCHS, MB, 10)
    assert torch.equal(PU._bits(out["stats"][:, :, :8].reshape(EPOCHS * MB, 8)), PU._bits(piece))
    assert torch.equal(PU._state_bits(torch, a, oa), PU._state_bits(torch, b, ob))
    assert not torch.equal(PU._bits(a[0]), PU._bits(start[0]))
    assert int(out["stats"][0, :, 6].sum()) == T * B * 3   # every (t, env, seat) row was a sample of the epoch
    env.close()


# ---- 11. the C boundary ----
def test_the_c_boundary_refuses_bad_seat_counts_other_tasks_and_null_opponents():
    import torch
    from rsoccer_amd import _lib, vec
    from rsoccer_amd.vec.policy import MLPPolicy
    f = lambda *s: torch.zeros(*s, device="cuda:0")   # noqa: E731
    rew, fl = f(2, 5), torch.zeros(2, 5, dtype=torch.uint8, device="cuda:0")

    def record(od, ad, S=3):
        keep = [f(2, 5, S, od), f(2, 5, S, ad), f(2, 5, S, od), f(2, 5, S, ad)]
        side = lambda o, a: _lib.TeamSideOut(o.data_ptr(), a.data_ptr())   # noqa: E731
        return _lib.TeamOut(rew.data_ptr(), fl.data_ptr(), side(keep[0], keep[1]), side(keep[2], keep[3])), keep

    sd = vec.VecSSLStaticDefendersEnv(5, device=0, seed=1)
    sd.reset()
    torch.cuda.synchronize()
    before = sd.checkpoint()
    p = MLPPolicy(sd.sim.obs_dim, sd.sim.act_dim)
    w = torch.zeros(p.num_params, device=sd.device)
    rec, keep = record(sd.sim.obs_dim, sd.sim.act_dim)
    with pytest.raises(_lib.RsxError, match="VSS-v0 only"):
        sd.sim.task_collect_team(p.spec(), w.data_ptr(), None, 1, None, None, None, 0, 0, 2, rec, sd._stream())
    torch.cuda.synchronize()
    assert np.array_equal(sd.checkpoint(), before)
    sd.close()
    env = vec.VecVSSEnv(5, device=0, seed=1)
    env.reset()
    torch.cuda.synchronize()
    before, tick = env.checkpoint(), env.sim.task_tick()
    p = MLPPolicy(40, 2)
    w = torch.zeros(p.num_params, device=env.device)
    rec, keep = record(40, 2)
    norec = _lib.TeamOut(rew.data_ptr(), fl.data_ptr())
    bad = _lib.PolicyMLP(2, 48, _lib.ACT_TANH, _lib.ACT_TANH)
    sp, wp = p.spec(), w.data_ptr()
    for args, why in (((sp, wp, None, 0, None, None, None, 0, 0, 2, rec), "actor_seats"),
                      ((sp, wp, None, 2, None, None, None, 0, 0, 2, rec), "actor_seats"),
                      ((sp, wp, None, 4, None, None, None, 0, 0, 2, rec), "actor_seats"),
                      ((sp, wp, None, 3, sp, wp, None, 2, 0, 2, rec), "opponent_seats"),
                      ((sp, wp, None, 3, sp, wp, None, -1, 0, 2, rec), "opponent_seats"),
                      ((sp, wp, None, 3, sp, wp, None, 4, 0, 2, rec), "opponent_seats"),
                      ((sp, wp, None, 3, None, wp, None, 3, 0, 2, rec), "null exactly when"),    # a NULL opponent with seats
                      ((sp, wp, None, 3, None, None, None, 1, 0, 2, rec), "null exactly when"),
                      ((sp, wp, None, 3, sp, wp, None, 0, 0, 2, rec), "null exactly when"),      # an opponent without seats
                      ((sp, wp, None, 3, sp, None, None, 3, 0, 2, rec), "opponent_params_dev"),
                      ((sp, wp, None, 3, bad, wp, None, 3, 0, 2, rec), "hidden"),
                      ((sp, None, None, 3, None, None, None, 0, 0, 2, rec), "actor_params_dev"),
                      ((sp, wp, None, 3, None, None, None, 0, 0, 0, rec), "n_steps"),
                      ((sp, wp, None, 3, None, None, None, 0, 0, 2, norec), "actor.obs"),
                      ((sp, wp, None, 3, None, None, None, 0, 0, 2, None), "out")):
        with pytest.raises(_lib.RsxError, match=why):
            env.sim.task_collect_team(*args, env._stream())
    torch.cuda.synchronize()
    assert np.array_equal(env.checkpoint(), before) and env.sim.task_tick() == tick   # nothing was enqueued
    env.sim.task_collect_team(sp, wp, None, 3, sp, wp, None, 3, 0, 2, rec, env._stream())   # the optional members may be NULL
    torch.cuda.synchronize()
    assert env.sim.task_tick() == tick + 2 and float(keep[0].abs().max()) > 0.0 and float(keep[2].abs().max()) > 0.0
    env.close()
