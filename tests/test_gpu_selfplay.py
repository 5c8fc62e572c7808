"""VecFusedEnv.collect(opponent=...) / rsx_task_collect_selfplay: VSS-v0 collection with yellow robot 0 driven by a second MLP policy from
the mirrored observation.  Sizes at which nothing divides evenly: B = 5 and 13 envs (ragged against tiles of 8 and of 4 envs), T = 6, the
agent 1 x 32 relu and the opponent 2 x 64 tanh, and the reverse.  Comparisons are on bit patterns (or `==`, where signed zeros are to
compare equal) unless a bound is named next to them."""
import math

import numpy as np
import pytest

import selfplay_helpers as SH
import test_gpu_policy_lookahead as PL   # _same, _dense, and the float32 bound of dense policies (taken from there, not re-derived)

pytestmark = pytest.mark.gpu

T, WARM = SH.T, SH.WARM
_same, _dense = PL._same, PL._dense
SINCOS_BOUND = 2.5e-7   # tests/test_oracle_golden.py::test_elementary_functions: sincos_f32 against the float64 functions
# (B, the agent's shape, the opponent's shape)
CASES = [(5, SH.SHAPE_SMALL, SH.SHAPE_LARGE), (13, SH.SHAPE_LARGE, SH.SHAPE_SMALL)]
IDS = ["B5-agent1x32relu-opp2x64tanh", "B13-agent2x64tanh-opp1x32relu"]


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _policies(torch, env, agent, opp, seed=5):
    from rsoccer_amd.vec.policy import MLPPolicy
    pa = MLPPolicy(env.sim.obs_dim, env.sim.act_dim, **agent)
    po = MLPPolicy(env.sim.obs_dim, env.sim.act_dim, **opp)
    return pa, _dense(torch, pa, 1, seed=seed)[0], po, _dense(torch, po, 1, seed=seed + 1)[0]


def _start(torch, env, warm=WARM):
    env.reset()
    for _ in range(warm):
        env.step(None)
    torch.cuda.synchronize()


def _check_mirror(out, n=3, tag=""):
    """opponent_obs[t] against obs[t]: the map of include/rsx.h on every entry both rows carry, compared with == (signed zeros are equal)"""
    obs, opp = out["obs"], out["opponent_obs"]
    want, _ = SH.mirror(obs, np.zeros(obs.shape[:-1] + (n, 2), dtype=np.float32), n)
    shared = np.ones(obs.shape[-1], dtype=bool)
    shared[SH.own_sincos_entries(n)] = False
    assert np.all(opp[..., shared] == want[..., shared]), (tag, np.argwhere(opp[..., shared] != want[..., shared])[:4].tolist())
    # ... spelled out once more without the helper: ball and positions negated, w equal, the slots swapped
    assert np.all(opp[..., 0:4] == -obs[..., 0:4]), tag
    for k in range(n):
        a, b = SH.own(n, k), SH.other(n, k)
        assert np.all(opp[..., a:a + 2] == -obs[..., b:b + 2]) and np.all(opp[..., a + 4:a + 6] == -obs[..., b + 2:b + 4]), (tag, k)
        assert np.all(opp[..., b:b + 2] == -obs[..., a:a + 2]) and np.all(opp[..., b + 2:b + 4] == -obs[..., a + 4:a + 6]), (tag, k)
        assert np.all(opp[..., a + 6] == obs[..., b + 4]) and np.all(opp[..., b + 4] == obs[..., a + 6]), (tag, k)
        s, c = opp[..., a + 2].astype(np.float64), opp[..., a + 3].astype(np.float64)
        assert np.all(np.abs(s * s + c * c - 1.0) < 1e-6), (tag, k)
    assert np.abs(obs).max() > 0.05 and np.abs(opp[..., SH.own_sincos_entries(n)]).max() > 0.5, (tag, "uninformative")


# ---- 1. the mirror, exactly ----
@pytest.mark.parametrize("B,agent,opp", CASES, ids=IDS)
def test_opponent_obs_is_the_mirror_exactly(B, agent, opp):
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(B, device=0, seed=2025)
    _start(torch, env)
    pa, a, po, o = _policies(torch, env, agent, opp)
    out = _host(env.collect(pa, a, T, opponent=po, opponent_params=o))
    assert out["opponent_obs"].shape == (T, B, 40) and out["opponent_actions"].shape == (T, B, 2)
    assert set(out) == {"obs", "actions", "reward", "terminated", "truncated", "next_obs", "opponent_obs", "opponent_actions"}
    _check_mirror(out, tag=f"B={B}")
    # the yellow sine / cosine have no counterpart in the agent's row: against the heading stored in env.state, T = 1 calls
    deg2rad = np.float32(math.pi / 180.0)
    for call in range(4):
        torch.cuda.synchronize()
        st = env.state.cpu().numpy()
        one = _host(env.collect(pa, a, 1, opponent=po, opponent_params=o))
        _check_mirror(one, tag=f"T = 1, call {call}")
        for k in range(3):
            th = st[5 + 6 * (3 + k) + 2]                     # yellow k's heading in degrees, float32, [B]
            arg = (th * deg2rad).astype(np.float32)          # what sincos_f32 is given
            at = SH.own(3, k)
            got_s, got_c = one["opponent_obs"][0, :, at + 2].astype(np.float64), one["opponent_obs"][0, :, at + 3].astype(np.float64)
            err = max(np.abs(got_s + np.sin(arg.astype(np.float64))).max(), np.abs(got_c + np.cos(arg.astype(np.float64))).max())
            print(f"call {call} yellow {k}: |(-sin, -cos)(heading) - opponent_obs| <= {err:.3e} (bound {SINCOS_BOUND:.1e})")
            assert err < SINCOS_BOUND, (call, k, err)
        # ... and the blue ones, which the agent's row carries, against the same state: the two rows describe one instant
        for k in range(3):
            arg = (st[5 + 6 * k + 2] * deg2rad).astype(np.float64)
            assert np.abs(one["obs"][0, :, SH.own(3, k) + 2] - np.sin(arg)).max() < SINCOS_BOUND
    env.close()


# ---- 2. selector opponents are exact ----
@pytest.mark.parametrize("layers,hidden", [(2, 64), (1, 32)])
def test_selector_opponents_are_evaluated_exactly(layers, hidden):
    import torch
    from rsoccer_amd import vec
    from rsoccer_amd.vec.policy import MLPPolicy
    B = 13 if layers == 2 else 5
    env = vec.VecVSSEnv(B, device=0, seed=11)
    _start(torch, env)
    pa = MLPPolicy(40, 2, **(SH.SHAPE_SMALL if layers == 2 else SH.SHAPE_LARGE))
    a = _dense(torch, pa, 1)[0]
    po = MLPPolicy(40, 2, hidden=hidden, layers=layers, hidden_act="relu", out_act="clip")
    # an entry of each slot group: the ball, an own robot (a position, its sine, its angular velocity), an other robot
    for i0, i1 in ((0, 1), (SH.own(3, 1), SH.own(3, 2) + 2), (SH.own(3, 0) + 6, SH.other(3, 2) + 1), (SH.other(3, 0) + 4, SH.other(3, 1) + 2)):
        params = SH.selector_params(torch, po, i0, i1)
        out = _host(env.collect(pa, a, T, opponent=po, opponent_params=params))
        want = np.clip(out["opponent_obs"][..., [i0, i1]], -1.0, 1.0)
        nz = want != 0.0
        assert _same(out["opponent_actions"][nz], want[nz]), (i0, i1, out["opponent_actions"][0, :2], want[0, :2])
        # a selected zero comes out as +0.0 whatever its sign (relu(x) - relu(-x)): there the comparison is ==, and the bits are those of
        # the host's float32 forward pass, every operation of which is exact
        assert np.all(out["opponent_actions"] == want) and nz.mean() > 0.5, (i0, i1)
        host = po.forward(torch.from_numpy(out["opponent_obs"]), params, dtype=torch.float32).numpy()
        assert _same(out["opponent_actions"], host), (i0, i1)
        assert np.abs(want).max() > 0.01, (i0, i1, "uninformative: the selected entries are zero")
    env.close()


# ---- 3. dense opponents ----
@pytest.mark.parametrize("B,agent,opp", CASES, ids=IDS)
def test_dense_opponents_are_within_the_float32_bound(B, agent, opp):
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(B, device=0, seed=2025)
    _start(torch, env)
    pa, a, po, o = _policies(torch, env, agent, opp)
    out = _host(env.collect(pa, a, T, opponent=po, opponent_params=o, opponent_log_std=-1.0, noise_seed=3))
    rows = torch.from_numpy(out["opponent_obs"]).reshape(-1, 40)
    want, bound = PL._forward_with_bound(torch, po, rows, o)   # MLPPolicy.forward in float64 and that test's bound
    assert torch.allclose(want, po.forward(rows, o), rtol=0, atol=1e-12)
    # opponent_mean is the output accumulator BEFORE out_act: the activation is applied here in float64 (1-Lipschitz, exact to 1e-16)
    got = torch.tanh(torch.from_numpy(out["opponent_mean"]).reshape(-1, 2).double())
    err = (got - want).abs().numpy()
    print(f"B={B}: largest error {err.max():.3e}, smallest bound {float(bound.min()):.3e}, worst error / bound {(err / bound.numpy()).max():.3f}")
    assert np.all(err <= bound.numpy())
    # ... and the agent's own answers keep the bound with an opponent staged behind its image
    rows = torch.from_numpy(out["obs"]).reshape(-1, 40)
    want, bound = PL._forward_with_bound(torch, pa, rows, a)
    err = (torch.from_numpy(out["actions"]).reshape(-1, 2).double() - want).abs().numpy()
    assert np.all(err <= bound.numpy())
    env.close()


# ---- 4. the opponent's head ----
def test_the_opponents_gaussian_head(oracle_mod):
    import torch
    from rsoccer_amd import vec
    from rsoccer_amd.vec.policy import MLPPolicy
    B, base, seed64 = 13, 11, 0x0123456789ABCDEF   # (distinct halves: the key is (lo, hi))
    envs = [vec.VecVSSEnv(B, device=0, seed=9, env_id_base=base) for _ in range(2)]
    for e in envs:
        _start(torch, e)
    env, twin = envs
    pa, a, _, _ = _policies(torch, env, SH.SHAPE_SMALL, SH.SHAPE_LARGE)
    po = MLPPolicy(40, 2, out_act="clip", **SH.SHAPE_LARGE)
    ts = [torch.zeros(s) for s in po.shapes]   # zero weights and a bias: the opponent's mean is the bias, in bits
    bias = torch.tensor([0.3, -0.7])
    ts[-1][:] = bias
    o = po.pack(ts)
    sig = np.array([0.5, 0.25], dtype=np.float32)
    tick0 = env.sim.task_tick()
    assert tick0 == WARM
    got = _host(env.collect(pa, a, T, log_std=-1.0, noise_seed=seed64, opponent=po, opponent_params=o, opponent_log_std=np.log(sig)))
    assert {"opponent_mean", "opponent_sample", "opponent_log_prob"} <= set(got)
    assert _same(got["opponent_mean"], np.broadcast_to(bias.numpy(), (T, B, 2)).copy())
    eps = SH.head_eps64(oracle_mod, SH.DOM_OPPONENT, seed64, base, tick0, T, B)
    want = got["opponent_mean"].astype(np.float64) + sig.astype(np.float64) * eps
    bound = 1e-5 * max(float(sig.max()), 1.0)   # test_gpu_collect.py::test_the_gaussian_head's (sigma = exp(log(sig)): maybe an ulp off sig)
    err = np.abs(got["opponent_sample"].astype(np.float64) - want)
    print(f"max |device opponent_sample - float64 restatement under domain 9| {err.max():.3e} (bound {bound:.1e}); eps std {eps.std():.3f}")
    assert err.max() <= bound
    assert 0.7 < eps.std() < 1.3 and abs(eps.mean()) < 0.3
    assert _same(got["opponent_actions"], np.clip(got["opponent_sample"], -1.0, 1.0))
    # the agent's head under its own domain word: the two heads never share a draw
    eps7 = SH.head_eps64(oracle_mod, 7, seed64, base, tick0, T, B)
    s_a = np.float32(np.exp(np.float32(-1.0)))
    assert np.abs(got["sample"].astype(np.float64) - (got["mean"].astype(np.float64) + float(s_a) * eps7)).max() <= bound
    assert (np.abs(eps7 - eps) > 1e-3).mean() > 0.9
    z = (got["opponent_sample"].astype(np.float64) - got["opponent_mean"]) / sig
    lp = (-0.5 * z * z - np.log(sig.astype(np.float64)) - 0.5 * np.log(2 * np.pi)).sum(-1)
    assert np.abs(got["opponent_log_prob"] - lp).max() <= 1e-4 * max(1.0, np.abs(lp).max())
    # a twin collected WITHOUT an opponent: at step 0 the states still agree, so the agent's row, mean and sample are the same bits
    plain = _host(twin.collect(pa, a, T, log_std=-1.0, noise_seed=seed64))
    for k in ("obs", "mean", "sample", "actions"):
        assert _same(got[k][0], plain[k][0]), k
    assert not _same(got["obs"][T - 1], plain["obs"][T - 1]), "uninformative: the opponent did not change the trajectory"
    for e in envs:
        e.close()


# ---- 5. the step is the engine's step with one command replaced ----
# Seed 2025: under the oracle's own random actions none of the 13 (nor of the 5) envs ends an episode within WARM + T = 9 steps of its
# reset (checked on the CPU with selfplay_helpers.oracle_alone_ends: 0 of 13, 0 of 5), so the cap of one env in eight is the self-play
# trajectories' to keep.
@pytest.mark.parametrize("B,agent,opp", CASES, ids=IDS)
def test_the_step_is_the_engines_step_with_one_command_replaced(oracle_mod, B, agent, opp):
    import torch
    from rsoccer_amd import vec
    seed = 2025
    assert SH.oracle_alone_ends(oracle_mod, B, seed) * 8 <= B
    env = vec.VecVSSEnv(B, device=0, seed=seed)
    _start(torch, env)
    refs = SH.oracle_envs(oracle_mod, B, seed)
    torch.cuda.synchronize()
    obs0 = env._t["obs"].cpu().numpy()
    for e, r in enumerate(refs):   # the two sides start from the same instant
        assert _same(obs0[e], r.task_out()["obs"].astype(np.float32)), e
    pa, a, po, o = _policies(torch, env, agent, opp)
    out = _host(env.collect(pa, a, T, log_std=-1.0, noise_seed=17, opponent=po, opponent_params=o, opponent_log_std=-0.5))
    rows = np.concatenate([out["obs"], out["next_obs"][None]], 0)   # row t + 1 of obs; behind the last step: next_obs
    left_out, compared = set(), 0
    for t in range(T):
        for e, r in enumerate(refs):
            if e in left_out:
                continue
            obs, reward, ended = SH.lockstep_step(r, out["actions"][t, e], out["opponent_actions"][t, e])
            if ended or out["terminated"][t, e] or out["truncated"][t, e]:
                left_out.add(e)   # from the first step on at which either trajectory ends an episode
                continue
            assert _same(rows[t + 1, e], obs), (t, e, np.argwhere(rows[t + 1, e] != obs)[:4].tolist())
            assert _same(out["reward"][t, e], reward), (t, e, out["reward"][t, e], reward)
            compared += 1
    print(f"B={B}: {compared} rows equal the lockstep oracle bit for bit, envs left out {sorted(left_out)}")
    assert len(left_out) * 8 <= B, left_out
    # informative: yellow 0 moved under the opponent (its OU command would have moved it elsewhere: see test 4's last assertion)
    assert np.abs(out["opponent_actions"]).max() > 0.05
    env.close()


# ---- 6. episode ends inside the launch ----
def test_episodes_end_inside_the_launch():
    import torch
    from rsoccer_amd import vec
    B, limit = 5, 8
    env = vec.VecVSSEnv(B, device=0, seed=4, max_episode_steps=limit)
    env.reset()
    for _ in range(limit - 3):   # three steps before the time limit, with a plain step() loop
        env.step(None)
    torch.cuda.synchronize()
    before = env.metrics()
    pa, a, po, o = _policies(torch, env, SH.SHAPE_SMALL, SH.SHAPE_LARGE)
    out = _host(env.collect(pa, a, T, return_final_obs=True, opponent=po, opponent_params=o))
    row = 2
    assert out["truncated"][row].all() and not out["terminated"].any(), (out["truncated"], out["terminated"])
    assert out["truncated"].sum() == B, "every env is truncated at the same row, and only there"
    assert np.abs(out["final_obs"][row]).max() > 0.05 and not out["final_obs"][np.arange(T) != row].any()
    vel = [2, 3] + [SH.own(3, k) + c for k in range(3) for c in (4, 5, 6)] + [SH.other(3, k) + c for k in range(3) for c in (2, 3, 4)]
    assert np.all(out["obs"][row + 1][:, vel] == 0.0) and np.all(out["opponent_obs"][row + 1][:, vel] == 0.0)
    assert np.abs(out["obs"][row][:, vel]).max() > 0.0
    _check_mirror(out, tag="across the reset")
    after = env.metrics()
    assert after["episodes"] - before["episodes"] == B and after["truncated_episodes"] - before["truncated_episodes"] == B
    assert after["env_steps"] - before["env_steps"] == B * T
    env.close()


# ---- 7. handing back ----
def test_the_env_can_be_handed_back():
    import torch
    from rsoccer_amd import vec
    B = 13
    env = vec.VecVSSEnv(B, device=0, seed=21, max_episode_steps=13)
    _start(torch, env)
    pa, a, po, o = _policies(torch, env, SH.SHAPE_LARGE, SH.SHAPE_SMALL)
    env.collect(pa, a, T, log_std=-1.0, opponent=po, opponent_params=o, opponent_log_std=-1.0)
    blob = env.checkpoint()
    twin = vec.VecVSSEnv(B, device=0, seed=21, max_episode_steps=13)
    twin.reset()
    twin.restore(blob)
    acts = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (4, B, 2)).astype(np.float32)).to(env.device)
    for t in range(4):   # (TimeLimit 13: the fourth of these steps ends every episode)
        for e in (env, twin):
            e.step(acts[t])
        torch.cuda.synchronize()
        for k in ("obs", "reward", "terminated", "truncated", "final_obs"):
            assert torch.equal(env._t[k], twin._t[k]), (t, k)
    assert bool(env._t["truncated"].all())
    outs = [_host(e.collect(pa, a, T, log_std=-1.0, noise_seed=5, return_final_obs=True)) for e in (env, twin)]
    for k, v in outs[0].items():
        assert _same(v, outs[1][k]), k
    assert "opponent_obs" not in outs[0]
    assert np.array_equal(env.checkpoint(), twin.checkpoint()) and env.metrics()["env_steps"] == B * (WARM + T + 4 + T)
    env.close(); twin.close()


# ---- 8. shapes and capture ----
def _shape_run(torch, env, B=13):
    _start(torch, env)
    pa, a, po, o = _policies(torch, env, SH.SHAPE_SMALL, SH.SHAPE_LARGE)
    out = _host(env.collect(pa, a, T, log_std=-1.0, noise_seed=5, return_final_obs=True, opponent=po, opponent_params=o, opponent_log_std=-1.0))
    blob = env.checkpoint()
    env.close()
    return {k: (v[:, :B] if v.ndim >= 2 and k != "next_obs" else v[:B]) for k, v in out.items()}, blob


def test_every_handle_shape_gives_the_same_bits(monkeypatch):
    import torch
    from rsoccer_amd import vec
    kw = dict(device=0, seed=29, max_episode_steps=7)   # TimeLimit 7, three warm steps: every env is re-placed at row 3
    want, blob = _shape_run(torch, vec.VecVSSEnv(13, **kw))
    assert want["truncated"][3].all()
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


def test_5v5_runs_the_native_16_lane_variant():
    import torch
    from rsoccer_amd import vec
    env = PL._make(vec, "VecVSS5v5", 5, device=0, seed=29, max_episode_steps=7)
    assert env.sim.obs_dim == 64
    _start(torch, env)
    pa, a, po, o = _policies(torch, env, SH.SHAPE_LARGE, SH.SHAPE_LARGE)
    out = _host(env.collect(pa, a, T, opponent=po, opponent_params=o))
    _check_mirror(out, n=5, tag="5v5")
    assert out["truncated"][3].all()
    env.close()


def test_selfplay_replays_from_a_graph():
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
        return e.collect(pa, a, T, log_std=ls, noise_seed=99, return_final_obs=True, opponent=po, opponent_params=o, opponent_log_std=ls)

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


# ---- 9. the C boundary's refusals ----
def test_the_c_boundary_refuses_other_tasks_and_null_opponents():
    import torch
    from rsoccer_amd import _lib, vec
    from rsoccer_amd.vec.policy import MLPPolicy
    sd = vec.VecSSLStaticDefendersEnv(5, device=0, seed=1)
    sd.reset()
    torch.cuda.synchronize()
    before = sd.checkpoint()
    p = MLPPolicy(sd.sim.obs_dim, sd.sim.act_dim)
    w = torch.zeros(p.num_params, device=sd.device)
    f = lambda *s: torch.zeros(*s, device=sd.device)   # noqa: E731
    obs, acts, rew, fl = f(2, 5, sd.sim.obs_dim), f(2, 5, sd.sim.act_dim), f(2, 5), torch.zeros(2, 5, dtype=torch.uint8, device=sd.device)
    rec = _lib.CollectOut(obs.data_ptr(), acts.data_ptr(), rew.data_ptr(), fl.data_ptr())
    with pytest.raises(_lib.RsxError, match="VSS-v0 only"):
        sd.sim.task_collect_selfplay(p.spec(), w.data_ptr(), None, p.spec(), w.data_ptr(), None, 0, 2, rec, None, sd._stream())
    torch.cuda.synchronize()
    assert np.array_equal(sd.checkpoint(), before)
    sd.close()
    env = vec.VecVSSEnv(5, device=0, seed=1)
    env.reset()
    torch.cuda.synchronize()
    before, tick = env.checkpoint(), env.sim.task_tick()
    p = MLPPolicy(40, 2)
    w = torch.zeros(p.num_params, device=env.device)
    obs, acts = f(2, 5, 40), f(2, 5, 2)
    rec = _lib.CollectOut(obs.data_ptr(), acts.data_ptr(), rew.data_ptr(), fl.data_ptr())
    bad = _lib.PolicyMLP(2, 48, _lib.ACT_TANH, _lib.ACT_TANH)
    for args in ((p.spec(), w.data_ptr(), None, None, w.data_ptr(), None, 0, 2, rec, None),       # null opponent
                 (p.spec(), w.data_ptr(), None, p.spec(), None, None, 0, 2, rec, None),           # null opponent parameters
                 (p.spec(), w.data_ptr(), None, bad, w.data_ptr(), None, 0, 2, rec, None),        # an opponent spec outside the listed values
                 (p.spec(), w.data_ptr(), None, p.spec(), w.data_ptr(), None, 0, 0, rec, None),   # n_steps
                 (p.spec(), w.data_ptr(), None, p.spec(), w.data_ptr(), None, 0, 2, None, None)):  # no record
        with pytest.raises(_lib.RsxError):
            env.sim.task_collect_selfplay(*args, env._stream())
    torch.cuda.synchronize()
    assert np.array_equal(env.checkpoint(), before) and env.sim.task_tick() == tick   # nothing was enqueued
    env.sim.task_collect_selfplay(p.spec(), w.data_ptr(), None, p.spec(), w.data_ptr(), None, 0, 2, rec, None, env._stream())   # sp may be NULL
    torch.cuda.synchronize()
    assert env.sim.task_tick() == tick + 2
    env.close()
