"""VecFusedEnv.collect with an MLPGaussianPolicy / rsx_task_collect_gaussian: soft actor-critic's actor driving the envs inside one launch.
Three things are pinned.  (1) With a unit sigma (zero log-std rows) the call IS the plain collector's Gaussian head with out_act = tanh:
every record and the checkpoint behind it agree in bits, so the loop is the collector's loop.  (2) mean and log_std are the bits
rsx_policy_mlp's arithmetic gives for output units k and act_dim + k, and the head is include/rsx.h's formula within a derived bound.
(3) The commit guarantee: a twin stepped with the recorded actions reproduces every row and the checkpoint, on every lane width, with
per-env physics, on a handle that steps one lane per env, and through graph replays.  Comparisons are on bit patterns unless a bound
is derived next to them."""
import numpy as np
import pytest

import test_gpu_collect as TC   # the twin check, the host restatement of the collector's draw, the raw call's record layout
import test_gpu_policy_lookahead as PL

pytestmark = pytest.mark.gpu

B, WARM = TC.B, TC.WARM   # 9 envs: one full 8-env tile and a ragged one at 8 lanes per env
_same, _dense, _make, _host, _start, _twin_check = PL._same, PL._dense, PL._make, TC._host, TC._start, TC._twin_check
U = 2.0 ** -24
# exp_f32's stated relative error (include/rsx.h); measured below and printed
EXP_REL = 5e-7


def _gauss(env, **kw):
    from rsoccer_amd.vec.policy import MLPGaussianPolicy
    return MLPGaussianPolicy(env.sim.obs_dim, env.sim.act_dim, **kw)


def _plain(env, gp, out_act="tanh"):
    from rsoccer_amd.vec.policy import MLPPolicy
    return MLPPolicy(env.sim.obs_dim, env.sim.act_dim, hidden=gp.hidden, layers=gp.layers, hidden_act=gp.hidden_act, out_act=out_act)


def _halves(gp, plain, params):
    """the plain policies that share the hidden layers and take output rows [0, AD) and [AD, 2 AD) of a Gaussian policy's parameters"""
    ts = gp.unpack(params)
    AD = gp.act_dim
    return plain.pack(ts[:-2] + [ts[-2][:AD], ts[-1][:AD]]), plain.pack(ts[:-2] + [ts[-2][AD:], ts[-1][AD:]])


def _scaled(gp, params, scale, shift=0.0):
    """the log-std rows of the output layer scaled (and the bias shifted), so that the raw log-std spreads over the bounds"""
    ts = [t.clone() for t in gp.unpack(params)]
    AD = gp.act_dim
    ts[-2][AD:] *= scale
    ts[-1][AD:] = ts[-1][AD:] * scale + shift
    return gp.pack(ts)


# ---- 1. a unit sigma: the call is the plain collector's, bit for bit ----
@pytest.mark.parametrize("name,layers,hidden,act", [("VecVSSEnv", 2, 64, "tanh"), ("VecSSLStaticDefendersEnv", 1, 32, "relu"),
                                                    ("VecSSLDribblingEnv", 2, 32, "tanh")])
def test_unit_sigma_is_the_plain_collector(name, layers, hidden, act):
    import torch
    from rsoccer_amd import vec
    T = 12
    env = _make(vec, name, B, device=0, seed=2025, max_episode_steps=5)
    _start(torch, env)
    gp = _gauss(env, hidden=hidden, layers=layers, hidden_act=act)
    plain = _plain(env, gp)
    AD = gp.act_dim
    ts = [t.clone() for t in gp.unpack(_dense(torch, gp, 1)[0])]
    ts[-2][AD:] = 0.0
    ts[-1][AD:] = 0.0   # raw = fmaf(0, h, 0) = 0 exactly: sigma = exp2(0) * (1 + 0) = 1
    params = gp.pack(ts)
    mu_params, _ = _halves(gp, plain, params)
    blob0 = env.checkpoint()
    for det in (False, True):
        env.restore(blob0)
        got = _host(env.collect(gp, params, T, noise_seed=77, return_final_obs=True, deterministic=det))
        blob1, met1 = env.checkpoint(), env.metrics()
        env.restore(blob0)
        want = _host(env.collect(plain, mu_params, T, log_std=0.0, noise_seed=77, return_final_obs=True) if not det else
                     env.collect(plain, mu_params, T, return_final_obs=True))
        assert np.array_equal(env.checkpoint(), blob1) and env.metrics() == met1, (name, det)
        keys = ["obs", "actions", "reward", "terminated", "truncated", "next_obs", "final_obs"] + ([] if det else ["mean", "sample"])
        for k in keys:
            assert _same(got[k], want[k]), (name, det, k, TC._where(got[k], want[k]))
        assert not got["log_std"].any()
        if det:
            assert _same(got["sample"], got["mean"])
        else:
            assert not _same(got["sample"], got["mean"])
        ends = (got["terminated"] | got["truncated"]).sum(0)
        assert np.all(ends >= 2), "uninformative: an env was not re-placed twice inside the launch"
    env.close()


# ---- 2. mean and log_std are rsx_policy_mlp's bits; the head is the header's formula ----
@pytest.mark.parametrize("name", ["VecVSSEnv", "VecSSLStaticDefendersEnv"])   # act_dim 2 and 5: one noise block and two
def test_the_squashed_head(oracle_mod, name):
    import torch
    from rsoccer_amd import vec
    from rsoccer_amd.vec.policy import squashed_log_prob
    T, base, seed64 = 6, 11, 0x0123456789ABCDEF
    LO, HI = -1.0, 0.5
    env = _make(vec, name, B, device=0, seed=9, env_id_base=base, max_episode_steps=5)
    _start(torch, env)
    AD = env.sim.act_dim
    gp = _gauss(env, log_std_min=LO, log_std_max=HI)
    plain = _plain(env, gp, out_act="clip")
    params = _scaled(gp, _dense(torch, gp, 1, seed=21)[0], 0.5, -0.25)
    mu_params, raw_params = _halves(gp, plain, params)
    blob0 = env.checkpoint()
    tick0 = env.sim.task_tick()
    got = _host(env.collect(gp, params, T, noise_seed=seed64))
    assert set(got) == {"obs", "actions", "reward", "terminated", "truncated", "next_obs", "mean", "log_std", "sample", "log_prob"}
    # row 0 answers the handle's observation: the plain collector records the output layer's accumulator for the same rows of Wo
    env.restore(blob0)
    as_mu = _host(env.collect(plain, mu_params, 1, log_std=0.0, noise_seed=seed64))
    env.restore(blob0)
    as_raw = _host(env.collect(plain, raw_params, 1, log_std=0.0, noise_seed=seed64))
    assert _same(as_mu["obs"], got["obs"][:1])
    assert _same(as_mu["mean"], got["mean"][:1]), TC._where(as_mu["mean"], got["mean"][:1])
    assert _same(np.clip(as_raw["mean"], np.float32(LO), np.float32(HI)), got["log_std"][:1])
    # every later row: the same statement through the float32 bound of dense policies (out_act clip at the bounds is the clamp)
    obs = torch.from_numpy(got["obs"]).reshape(-1, gp.obs_dim)
    for half, key, lo, hi in ((mu_params, "mean", None, None), (raw_params, "log_std", LO, HI)):
        ts = [t.double() for t in plain.unpack(half)]
        x, delta = obs.double(), torch.zeros_like(obs, dtype=torch.float64)
        for li in range(len(ts) // 2):   # PL._forward_with_bound's recurrence with a linear output
            w, b = ts[2 * li], ts[2 * li + 1]
            pre = x @ w.T + b
            delta = delta @ w.abs().T + (w.shape[1] + 1) * U * ((x.abs() + delta) @ w.abs().T + b.abs())
            if li + 1 < len(ts) // 2:
                x, delta = torch.tanh(pre), delta + 4 * PL.TANH_DEV
        want = pre if lo is None else pre.clamp(lo, hi)   # (the clamp is 1-Lipschitz)
        err = (torch.from_numpy(got[key]).reshape(-1, AD).double() - want).abs()
        print(f"{name} {key}: largest error {err.max():.3e}, smallest bound {delta.min():.3e}")
        assert bool((err <= delta).all()), key
    ls = got["log_std"].astype(np.float64)
    inside = (ls > LO) & (ls < HI)
    print(f"{name}: clamp binds on {1.0 - inside.mean():.3f} of the entries (low {np.mean(ls == LO):.3f}, high {np.mean(ls == HI):.3f})")
    assert 0.02 < 1.0 - inside.mean() < 0.9 and (ls == LO).any() and (ls == HI).any() and ls.min() >= LO and ls.max() <= HI
    # u = mu + exp(ls) * eps: eps within the collector's 1e-5 of the float64 restatement, exp within its stated relative error, two roundings
    eps = TC._eps64(oracle_mod, seed64, base, tick0, T, B, AD)
    sigma = np.exp(ls)
    mu, u = got["mean"].astype(np.float64), got["sample"].astype(np.float64)
    bound = sigma * 1e-5 + (sigma * np.abs(eps)) * (EXP_REL + 2 * U) + U * (np.abs(mu) + sigma * np.abs(eps))
    err = np.abs(u - (mu + sigma * eps))
    print(f"{name}: max |device sample - float64 restatement| {err.max():.3e}, worst error / bound {(err / bound).max():.3f}")
    assert np.all(err <= bound)
    # a = tanh(u) within the engine's measured tanh allowance, |a| <= 1
    a = got["actions"].astype(np.float64)
    assert np.abs(a - np.tanh(u)).max() <= 4 * PL.TANH_DEV and np.abs(a).max() <= 1.0
    # log_prob: the header's formula on the recorded tensors in float64 (the float32 torch expression: 1e-4 relative, as the plain head's)
    e64 = torch.from_numpy((u - mu) / sigma)
    lp = squashed_log_prob(e64, torch.from_numpy(ls), torch.from_numpy(u)).numpy()
    assert got["log_prob"].shape == (T, B) and np.abs(got["log_prob"] - lp).max() <= 1e-4 * max(1.0, np.abs(lp).max())
    # the same call again: the same bits; deterministic: no draw, the same observation 0, log_std still recorded
    env.restore(blob0)
    again = _host(env.collect(gp, params, T, noise_seed=seed64))
    for k in got:
        assert _same(got[k], again[k]), k
    env.restore(blob0)
    det = _host(env.collect(gp, params, T, noise_seed=seed64, deterministic=True))
    assert _same(det["sample"], det["mean"]) and _same(det["mean"][0], got["mean"][0]) and _same(det["log_std"][0], got["log_std"][0])
    assert np.abs(det["actions"].astype(np.float64) - np.tanh(det["mean"].astype(np.float64))).max() <= 4 * PL.TANH_DEV
    # the batch split: env e of a handle shifted by 4 IS global env e + 4
    sh = _make(vec, name, B - 4, device=0, seed=9, env_id_base=base + 4, max_episode_steps=5)
    _start(torch, sh)
    shifted = _host(sh.collect(gp, params, T, noise_seed=seed64))
    for k in got:
        assert _same(shifted[k], got[k][:, 4:] if got[k].ndim >= 2 and k != "next_obs" else got[k][4:]), k
    sh.close()
    env.close()


def test_exp_is_within_its_stated_error():
    """exp_f32 measured through the head itself.  The plain collector with an all-zero policy and sigma = 1 records sample = 0 + 1 * eps:
    the device's own eps in bits (the draw depends on seed, env id and tick only, not on the state).  A Gaussian policy with zero mean rows
    records u = 0 + sigma * eps = fl(sigma * eps): one rounding away from exp_f32(log_std) * eps."""
    import torch
    from rsoccer_amd import vec
    T = 16
    env = vec.VecSSLStaticDefendersEnv(70, device=0, seed=4, max_episode_steps=5)
    _start(torch, env)
    AD = env.sim.act_dim
    gp = _gauss(env)   # the default bounds (-20, 2)
    plain = _plain(env, gp)
    ts = [t.clone() for t in gp.unpack(_scaled(gp, _dense(torch, gp, 1, seed=8)[0], 4.0, -6.0))]
    ts[-2][:AD] = 0.0
    ts[-1][:AD] = 0.0
    blob0 = env.checkpoint()
    eps = _host(env.collect(plain, torch.zeros(plain.num_params), T, log_std=0.0, noise_seed=123))
    assert not eps["mean"].any()
    env.restore(blob0)
    got = _host(env.collect(gp, gp.pack(ts), T, noise_seed=123))
    assert not got["mean"].any()
    e, u, ls = eps["sample"].astype(np.float64), got["sample"].astype(np.float64), got["log_std"].astype(np.float64)
    ok = e != 0.0
    rel = np.abs(u[ok] / e[ok] / np.exp(ls[ok]) - 1.0)
    print(f"exp_f32 over log_std in [{ls.min():.2f}, {ls.max():.2f}] ({ok.sum()} entries, {np.mean(ls == 2.0):.2f} at the upper bound, "
          f"{np.mean(ls == -20.0):.3f} at the lower): largest relative error {rel.max():.3e} (stated {EXP_REL:.0e} + one rounding)")
    assert ls.min() < -12.0 and ls.max() == 2.0, "uninformative: the log-std does not cover the range"
    assert rel.max() <= EXP_REL + U
    env.close()


# ---- 3. the commit guarantee on every handle shape ----
@pytest.mark.parametrize("name", PL.CLASSES)
def test_collect_commits_like_step(name):
    import torch
    from rsoccer_amd import vec
    env = _make(vec, name, B, device=0, seed=2025, max_episode_steps=5)
    _start(torch, env)
    gp = _gauss(env, log_std_min=-2.0, log_std_max=0.0)
    out = _twin_check(torch, env, gp, _dense(torch, gp, 1)[0], 12, tag=name, noise_seed=5)
    assert np.all((out["terminated"] | out["truncated"]).sum(0) >= 2), "uninformative: an env was not re-placed twice inside the launch"
    assert not _same(out["sample"], out["mean"])
    env.close()


def test_lane_widths_give_the_same_bits(monkeypatch):
    import torch
    from rsoccer_amd import vec
    outs = []
    for lanes in (None, "16", "32"):
        if lanes:
            monkeypatch.setenv("RSX_LANES_PER_ENV", lanes)
        env = vec.VecVSSEnv(70, device=0, seed=29, max_episode_steps=5)   # 70 envs: a ragged last tile at every width (8, 4, 2 per tile)
        assert env.sim.task_layout() == f"{lanes or 8}-lanes-per-env", env.sim.task_layout()
        _start(torch, env)
        gp = _gauss(env, log_std_min=-2.0, log_std_max=0.0)
        outs.append(_twin_check(torch, env, gp, _dense(torch, gp, 1)[0], 8, tag=f"lanes {lanes}", noise_seed=5))
        env.close()
    for other in outs[1:]:
        for k, v in outs[0].items():
            assert _same(v, other[k]), k


def test_vss_5v5_native_16_lanes():
    import torch
    from rsoccer_amd import vec
    env = _make(vec, "VecVSS5v5", B, device=0, seed=29, max_episode_steps=5)
    assert env.sim.obs_dim == 64
    _start(torch, env)
    gp = _gauss(env)
    out = _twin_check(torch, env, gp, _scaled(gp, _dense(torch, gp, 1)[0], 0.25, -1.0), 8, tag="5v5", noise_seed=5)
    assert out["truncated"].any()
    env.close()


@pytest.mark.parametrize("id_,ranges", [("VSS-v0", {"m_ball": (0.04, 0.05), "mu_g": (0.2, 0.4)}),
                                        ("SSLStaticDefenders-v0", {"m_ball": (0.04, 0.05), "e_rb": (0.2, 0.6)})])
def test_per_env_physics_is_redrawn_inside_the_launch(id_, ranges):
    import torch
    import rsoccer_amd
    env = rsoccer_amd.make_vec(id_, B, device=0, seed=31, max_episode_steps=5, physics_ranges=ranges)
    _start(torch, env, 7)
    before = env.physics()["m_ball"].cpu().numpy()
    gp = _gauss(env, log_std_min=-2.0, log_std_max=0.0)
    params = _dense(torch, gp, 1)[0]
    blob0 = env.checkpoint()
    env.collect(gp, params, 12, noise_seed=5)
    phys1 = {k: v.cpu().numpy() for k, v in env.physics().items()}
    assert not _same(phys1["m_ball"], before), "uninformative: no redraw inside the launch"
    env.restore(blob0)
    _twin_check(torch, env, gp, params, 12, tag=id_, noise_seed=5)
    for k, v in env.physics().items():
        assert _same(v.cpu().numpy(), phys1[k]), k
    env.close()


def test_handle_that_steps_one_lane_per_env():
    """tests/test_gpu_collect.py's case under this head: the stepped twin takes every auto-reset in the one-lane-per-env kernel"""
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(98304, device=0, seed=5, max_episode_steps=5)
    assert env.sim.task_layout() == "one-lane-per-env"
    _start(torch, env, 2)
    gp = _gauss(env, log_std_min=-2.0, log_std_max=0.0)
    out = _twin_check(torch, env, gp, _dense(torch, gp, 1)[0], 3, tag="98304 envs", noise_seed=3)
    assert (out["terminated"][2] | out["truncated"][2]).mean() >= 0.9, "uninformative: the last recorded row does not end (nearly) every env"
    env.close()


# ---- 4. device-keyed handles and graphs ----
def test_collect_replays_from_a_graph():
    import torch
    from rsoccer_amd import vec
    T = 6
    envs = [vec.VecVSSEnv(B, device=0, seed=17, max_episode_steps=5) for _ in range(2)]
    for e in envs:
        _start(torch, e)
        e.enable_graph_capture()
    env, twin = envs
    gp = _gauss(env, log_std_min=-2.0, log_std_max=0.0)
    params = _dense(torch, gp, 1)[0].to(env.device)

    def run(e):
        return e.collect(gp, params, T, noise_seed=99, return_final_obs=True)

    def follow(out, tag):
        """the twin takes the recorded actions step by step and must see what the call recorded"""
        torch.cuda.synchronize()
        rec = {k: v.clone() for k, v in out.items()}
        for t in range(T):
            assert torch.equal(twin._t["obs"], rec["obs"][t]), (tag, "obs", t)
            twin.step(rec["actions"][t])
            assert torch.equal(twin._t["reward"], rec["reward"][t]), (tag, "reward", t)
            assert torch.equal(twin._t["terminated"].bool(), rec["terminated"][t]), (tag, t)
            assert torch.equal(twin._t["truncated"].bool(), rec["truncated"][t]), (tag, t)
        assert torch.equal(twin._t["obs"], env._t["obs"]), tag
        return rec

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # the eager call, which is also torch's warm-up before a capture
        first = run(env)
    torch.cuda.current_stream().wait_stream(side)
    recs = [follow(first, "eager")]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run(env)
    assert env.sim.task_tick() == twin.sim.task_tick() == WARM + T   # capturing enqueued nothing
    for i in range(2):
        g.replay()
        recs.append(follow(out, f"replay {i}"))
    assert env.sim.task_tick() == twin.sim.task_tick() == WARM + 3 * T
    assert np.array_equal(env.checkpoint(), twin.checkpoint())
    assert env.metrics() == twin.metrics()
    noise = [((r["sample"] - r["mean"]) / r["log_std"].exp())[0] for r in recs]
    for a, b in ((0, 1), (1, 2)):
        assert ((noise[a] - noise[b]).abs() > 1e-4).float().mean() > 0.9, "a replay repeated its noise"
    for e in envs:
        e.close()


# ---- 5. the batch feeds the ring ----
def test_replay_buffer_takes_the_batch():
    import torch
    from rsoccer_amd import vec
    from rsoccer_amd.vec.replay import ReplayBuffer
    env = vec.VecVSSEnv(B, device=0, seed=3, max_episode_steps=5)
    _start(torch, env)
    gp = _gauss(env)
    out = env.collect(gp, _dense(torch, gp, 1)[0], 8, noise_seed=1, return_final_obs=True)
    buf = ReplayBuffer(100, env.sim.obs_dim, env.sim.act_dim, device=env.device)
    n = buf.add(out)
    torch.cuda.synchronize()
    assert n == 8 * B and int(buf.fill) == n
    assert torch.equal(buf.actions[:n], out["actions"].reshape(n, -1)) and torch.equal(buf.obs[:n], out["obs"].reshape(n, -1))
    ended = (out["terminated"] | out["truncated"]).reshape(n)
    assert ended.any() and torch.equal(buf.next_obs[:n][ended], out["final_obs"].reshape(n, -1)[ended])
    env.close()


# ---- 6. refusals: nothing is enqueued ----
def test_refusals(monkeypatch):
    import torch
    from rsoccer_amd import _lib, vec
    from rsoccer_amd.vec.policy import MLPCritic, MLPGaussianPolicy
    env = vec.VecVSSEnv(B, device=0, seed=1, max_episode_steps=5)
    gp = _gauss(env)
    plain = _plain(env, gp)
    params = _dense(torch, gp, 1)[0]
    with pytest.raises(_lib.RsxError, match="reset"):
        env.collect(gp, params, 3)
    _start(torch, env)
    before, tick = env.checkpoint(), env.sim.task_tick()
    dev, n, OD, AD = env.device, env.num_envs, env.sim.obs_dim, env.sim.act_dim
    t = {"obs": torch.zeros((2, n, OD), device=dev), "actions": torch.full((2, n, AD), 7.0, device=dev), "rewards": torch.zeros((2, n), device=dev),
         "flags": torch.zeros((2, n), dtype=torch.uint8, device=dev)}
    p = params.to(dev)
    good_out = lambda skip=None: _lib.CollectOut(*[None if k == skip else t[k].data_ptr() for k in ("obs", "actions", "rewards", "flags")])   # noqa: E731
    good_cfg = lambda **kw: _lib.CollectGaussianCfg(**{**dict(noise_seed=1, log_std_min=-20.0, log_std_max=2.0, deterministic=0, reserved=0), **kw})   # noqa: E731
    call = lambda spec=gp.spec(), pp=p.data_ptr(), cfg=good_cfg(), T=2, out=good_out(): env.sim.task_collect_gaussian(   # noqa: E731
        spec, pp, cfg, T, out, None, env._stream())
    bad = [dict(spec=None), dict(spec=plain.spec()), dict(spec=_lib.PolicyMLP(2, 64, _lib.ACT_TANH, _lib.ACT_CLIP)),
           dict(spec=_lib.PolicyMLP(2, 48, _lib.ACT_TANH, _lib.ACT_NONE)), dict(spec=_lib.PolicyMLP(3, 64, _lib.ACT_TANH, _lib.ACT_NONE)),
           dict(spec=_lib.PolicyMLP(2, 64, 7, _lib.ACT_NONE)), dict(pp=None), dict(cfg=None), dict(cfg=good_cfg(reserved=1)),
           dict(cfg=good_cfg(log_std_min=2.0)), dict(cfg=good_cfg(log_std_min=3.0)), dict(cfg=good_cfg(log_std_min=float("nan"))),
           dict(cfg=good_cfg(log_std_max=float("inf"))), dict(cfg=good_cfg(log_std_min=float("-inf"))), dict(T=0), dict(T=-1), dict(T=1 << 30),
           dict(out=None)] + [dict(out=good_out(k)) for k in ("obs", "actions", "rewards", "flags")]
    for kw in bad:
        with pytest.raises(_lib.RsxError):
            call(**kw)
    # the Python layer: keywords of the other heads, shapes, and `deterministic` on a plain policy
    critic = MLPCritic(OD)
    for kw in (dict(log_std=0.0), dict(critic=critic, critic_params=torch.zeros(critic.num_params)), dict(critic_params=torch.zeros(3)),
               dict(opponent=plain, opponent_params=torch.zeros(plain.num_params)), dict(opponent_params=torch.zeros(3)),
               dict(opponent_log_std=0.0), dict(team=True), dict(opponent_team=True)):
        with pytest.raises(ValueError):
            env.collect(gp, params, 2, **kw)
    for shape in ((gp.num_params - 1,), (plain.num_params,), (1, gp.num_params)):
        with pytest.raises(ValueError):
            env.collect(gp, torch.zeros(*shape), 2)
    with pytest.raises(ValueError):
        env.collect(gp, params, 0)
    with pytest.raises(ValueError):   # a policy for another task's dims
        env.collect(MLPGaussianPolicy(24, 5), torch.zeros(MLPGaussianPolicy(24, 5).num_params), 2)
    for flag in (True, 1, None):
        with pytest.raises(ValueError):
            env.collect(plain, torch.zeros(plain.num_params), 2, deterministic=flag)
    torch.cuda.synchronize()
    assert np.array_equal(env.checkpoint(), before) and env.sim.task_tick() == tick   # nothing was enqueued
    assert (t["actions"] == 7.0).all()
    call()   # the optional arrays may all be NULL
    torch.cuda.synchronize()
    assert env.sim.task_tick() == tick + 2 and not (t["actions"] == 7.0).any()
    out = env.collect(gp, params.double().numpy(), 2)   # numpy / float64 parameters are converted
    assert out["log_prob"].shape == (2, B) and env.sim.task_tick() == tick + 4
    env.close()
    # the collector's own refusals: the scrimmage task, 64 lanes per env
    scr = vec.VecSSLScrimmageEnv(B, device=0, seed=1)
    scr.reset()
    if scr.sim.act_dim <= 8:
        spol = MLPGaussianPolicy(scr.sim.obs_dim, scr.sim.act_dim)
        with pytest.raises(_lib.RsxError, match="scrimmage"):
            scr.collect(spol, torch.zeros(spol.num_params), 3)
    scr.close()
    monkeypatch.setenv("RSX_LANES_PER_ENV", "64")
    wide = vec.VecVSSEnv(B, device=0, seed=1)
    assert wide.sim.task_layout() == "64-lanes-per-env"
    wide.reset()
    with pytest.raises(_lib.RsxError, match="64-lanes-per-env"):
        wide.collect(gp, params, 2)
    wide.close()


# =====================================================================================================================================
# VecFusedEnv.sac_gradient / rsx_task_sac_gradient.  The gradients and stats are checked against float64 autograd with torch's own float32
# autograd as the yardstick (tests/sac_helpers.py), the draws against a host restatement, the forward pass against collect()'s own
# record bit for bit; then determinism, capture, out-of-range rows and refusals.
# =====================================================================================================================================
import sac_helpers as SH   # noqa: E402


@pytest.fixture(scope="module")
def handles():
    """handles that are never reset and never stepped: the call needs only their device, obs_dim and act_dim"""
    from rsoccer_amd import vec
    made = {}

    def get(name):
        if name not in made:
            made[name] = _make(vec, name, 9, device=0, seed=1)
        return made[name]
    yield get
    for env in made.values():
        env.close()


def _rows_of(data, dev):
    return {k: data[k].to(dev).contiguous() for k in SH.ROW_KEYS}


def _grad(env, pol, critic, data, rows, wg=None, rows_of=None, **kw):
    dev = env.device
    args = dict(rows=None if rows is None else rows.to(dev), gamma=SH.GAMMA, noise_seed=SH.SEED64, noise_step=SH.STEP, max_workgroups=wg,
                return_rows=True)
    args.update(kw)
    return env.sac_gradient(_rows_of(data, dev) if rows_of is None else rows_of, pol, data["params"].to(dev), critic, data["cparams"].to(dev),
                            data["tcparams"].to(dev), data["log_alpha"].to(dev), **args)


PER_ENTRY = ("target", "q", "action", "log_prob", "next_log_prob", "eps", "next_eps", "mean", "log_std")


def _flat_bits(torch, out):
    return torch.cat([out[k].reshape(-1) for k in ("grad_params", "grad_critic_params", "grad_log_alpha") + PER_ENTRY] +
                     [torch.stack(list(out["stats"].values()))]).clone().view(torch.int32)


def _rel(x, ref):
    scale = float(ref.abs().max())
    err = float((x - ref).abs().max())
    if scale == 0.0:
        assert err == 0.0, "the reference is exactly zero, the result is not"
        return 0.0
    return err / scale


# ---- 7. gradients and stats against float64 autograd, torch's float32 autograd as the yardstick ----
@pytest.mark.parametrize("case", SH.CASES, ids=["-".join(str(v) for v in c) for c in SH.CASES])
def test_gradients_and_stats_stay_within_4x_of_torchs_float32_error(handles, oracle_mod, case):
    """Criterion (tests/test_gpu_dpg_grad.py's, unchanged): for every parameter tensor of the actor and of each critic, grad_log_alpha and
    every float stat, the kernel's relative error against float64 autograd is at most 4x the LARGEST relative error any tensor of torch's
    float32 autograd on the device shows in the same case.  The yardstick is fed the call's own eps / next_eps (pinned by the test below)."""
    import torch
    (od, ad), hidden, layers, act, C, M, mode, wg, bounds = case
    env = handles(SH.ENVS[(od, ad)])
    assert (env.sim.obs_dim, env.sim.act_dim) == (od, ad)
    b = SH.case_data(torch, oracle_mod, case)
    assert SH.within_cap(case, b)
    pol, critic, data, rows, idx, mark = b["pol"], b["critic"], b["data"], b["rows"], b["idx"], b["mark"]
    got = _grad(env, pol, critic, data, rows, wg=wg)
    torch.cuda.synchronize()
    marked = int(mark.sum())
    used, skipped = int(got["stats"]["rows_used"]), int(got["stats"]["rows_skipped"])
    assert used + skipped == M and skipped == marked
    keep = ~mark
    for k in PER_ENTRY:   # a skipped entry is zero in every per-entry output
        t = got[k].cpu()
        t = t[:, mark] if k == "q" else t[mark]
        assert not t.any(), k
    eps, neps = got["eps"].cpu()[keep], got["next_eps"].cpu()[keep]
    ref = SH.autograd(torch, pol, critic, data, idx[keep], eps, neps, torch.float64, "cpu", M)
    yard = SH.autograd(torch, pol, critic, data, idx[keep], eps, neps, torch.float32, env.device, M)
    ker = {f"actor.{i}": t for i, t in enumerate(pol.unpack(got["grad_params"].cpu().double()))}
    for c in range(C):
        ker.update({f"critic{c}.{i}": t for i, t in enumerate(critic.unpack(got["grad_critic_params"][c].cpu().double()))})
    ker["log_alpha"] = got["grad_log_alpha"].cpu().double()
    ker.update({k: got["stats"][k].cpu().double() for k in SH.FLOAT_STATS})
    assert set(ref) <= set(ker) and len(ref) == 2 * (layers + 1) * (1 + C) + 1 + 2 * C + 6
    e_yard = {k: _rel(yard[k], ref[k]) for k in ref}
    e_ker = {k: _rel(ker[k], ref[k]) for k in ref}
    pooled = max(e_yard.values())
    worst = max(e_ker, key=e_ker.get)
    print(f"{case}: seed {b['seed']}, removed {b['removed']}, marked {marked}, torch f32 pooled {pooled:.3e}, kernel worst {e_ker[worst]:.3e} "
          f"({worst}), ratio {e_ker[worst] / pooled:.2f}")
    assert pooled > 0.0
    for k in ref:
        assert e_ker[k] <= 4.0 * pooled, (k, e_ker[k], pooled, e_ker[k] / pooled)
    if C == 1:
        assert float(got["stats"]["loss_q1"]) == 0.0 and float(got["stats"]["q1"]) == 0.0


# ---- 8. the draws ----
@pytest.mark.parametrize("od_ad", [(40, 2), (14, 5)])   # one noise block and two
def test_the_draws(handles, oracle_mod, od_ad):
    import torch
    import test_gpu_dpg_grad as DG
    import dpg_helpers as DH
    env = handles(SH.ENVS[od_ad])
    dev, AD = env.device, od_ad[1]
    M = 150
    pol, critic = SH.case_nets((od_ad, 32, 1, "tanh", 2, M, "perm", None, "default"))
    data, _ = SH.make_data(torch, pol, critic, 2, M + 64, 21, False)
    n = data["obs"].shape[0]
    rows = DH.make_rows(torch, "perm", M, n, 1)
    got = _grad(env, pol, critic, data, rows)
    torch.cuda.synchronize()
    eps, neps = got["eps"].cpu().numpy(), got["next_eps"].cpu().numpy()
    for name, dev_eps, dom in (("eps", eps, SH.DOM_OBS), ("next_eps", neps, SH.DOM_NEXT)):
        want = SH.eps_host(oracle_mod, SH.SEED64, SH.STEP, M, AD, dom)
        err = np.abs(dev_eps.astype(np.float64) - want)
        print(f"{od_ad} {name}: max |device - restatement| {err.max():.3e} (bound 1e-5); std {want.std():.3f}")
        assert err.max() <= 1e-5 and 0.7 < want.std() < 1.3   # (test_the_gaussian_head's bound for the collector's head)
    # the two never share a draw with each other or with rsx_task_dpg_gradient's domain 10
    dpg_eps = DG._noise_host(oracle_mod, SH.SEED64, SH.STEP, M, AD, 0.2, 0.1)[1]
    far = lambda a, b: (np.abs(a.astype(np.float64) - b) > 1e-3).mean() > 0.9   # noqa: E731
    assert far(eps, neps.astype(np.float64)) and far(eps, dpg_eps) and far(neps, dpg_eps)
    # functions of (seed, step, t) alone: not of the grid, not of the rows' contents
    other_rows = DH.make_rows(torch, "repeats", M, n, 2)
    for kw in (dict(wg=1), dict(rows=other_rows.to(torch.int32)), dict(wg=2, rows=None, rows_of={k: v[:M].contiguous() for k, v in _rows_of(data, dev).items()})):
        again = _grad(env, pol, critic, data, kw.pop("rows", rows), **kw)
        assert _same(again["eps"].cpu().numpy(), eps) and _same(again["next_eps"].cpu().numpy(), neps), kw
    # another step or another seed: other draws; the step's high word is a counter word of its own
    for kw in (dict(noise_step=SH.STEP + 1), dict(noise_seed=SH.SEED64 + 1), dict(noise_step=SH.STEP + 2 ** 32)):
        o = _grad(env, pol, critic, data, rows, **kw)
        assert not _same(o["eps"].cpu().numpy(), eps) and not _same(o["next_eps"].cpu().numpy(), neps), kw
    o = _grad(env, pol, critic, data, rows, noise_step=SH.STEP + 2 ** 32)
    assert np.abs(o["eps"].cpu().numpy().astype(np.float64) - SH.eps_host(oracle_mod, SH.SEED64, SH.STEP + 2 ** 32, M, AD, SH.DOM_OBS)).max() <= 1e-5
    # the same call again, and another grid: the result bits are a function of the inputs and G alone
    assert torch.equal(_flat_bits(torch, _grad(env, pol, critic, data, rows)), _flat_bits(torch, got))
    one = _grad(env, pol, critic, data, rows, wg=1)
    for k in PER_ENTRY:
        assert torch.equal(one[k], got[k]), k
    # the step as a device tensor, advanced between two replays of one captured call
    static = _rows_of(data, dev)
    r, step = rows.to(dev), torch.tensor([SH.STEP], dtype=torch.int64, device=dev)
    eager = [_flat_bits(torch, _grad(env, pol, critic, data, r, rows_of=static, noise_step=SH.STEP + i)) for i in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # torch's warm-up before a capture
        _grad(env, pol, critic, data, r, rows_of=static, noise_step=step)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    p = {k: data[k].to(dev) for k in ("params", "cparams", "tcparams", "log_alpha")}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = env.sac_gradient(static, pol, p["params"], critic, p["cparams"], p["tcparams"], p["log_alpha"], rows=r, gamma=SH.GAMMA,
                               noise_seed=SH.SEED64, noise_step=step, return_rows=True)
    seen = []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        seen.append(_flat_bits(torch, out))
        step += 1
    assert torch.equal(seen[0], eager[0]) and torch.equal(seen[1], eager[1]) and not torch.equal(seen[0], seen[1])


# ---- 9. the forward pass on a real batch ----
@pytest.mark.parametrize("name", ["VecVSSEnv", "VecSSLDribblingEnv"])   # act_dim 2 and 4
def test_forward_bits_on_a_real_batch(name):
    import torch
    from rsoccer_amd import vec
    from rsoccer_amd.vec.policy import MLPQCritic
    import dpg_helpers as DH
    T, Bn = 8, 64
    env = _make(vec, name, Bn, device=0, seed=2025, max_episode_steps=5)
    _start(torch, env)
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    gp = _gauss(env, log_std_min=-1.0, log_std_max=0.5)
    critic = MLPQCritic(OD, AD, hidden=64, layers=2)
    gen = torch.Generator().manual_seed(3)
    params = _scaled(gp, DH.init(torch, gp, gen), 6.0).to(dev)
    cparams = torch.stack([DH.init(torch, critic, gen) for _ in range(2)]).to(dev)
    batch = env.collect(gp, params, T, noise_seed=9, return_final_obs=True)
    n = T * Bn
    flat = {"obs": batch["obs"].reshape(n, OD).contiguous(), "actions": batch["actions"].reshape(n, AD).contiguous(),
            "reward": batch["reward"].reshape(n).contiguous(), "next_obs": batch["obs"].reshape(n, OD).contiguous(),
            "terminated": batch["terminated"].reshape(n).contiguous()}
    out = env.sac_gradient(flat, gp, params, critic, cparams, cparams.clone(), torch.tensor([-0.7], device=dev), rows=None, return_rows=True)
    torch.cuda.synchronize()
    mean, ls = batch["mean"].reshape(n, AD), batch["log_std"].reshape(n, AD)
    assert _same(out["mean"].cpu().numpy(), mean.cpu().numpy()), TC._where(out["mean"].cpu().numpy(), mean.cpu().numpy())
    assert _same(out["log_std"].cpu().numpy(), ls.cpu().numpy())
    share = float(((ls == -1.0) | (ls == 0.5)).float().mean())
    assert 0.02 < share < 0.9, share   # the clamp binds on a share of the recorded entries, and the bits still agree
    assert int(out["stats"]["rows_used"]) == n and int(out["stats"]["rows_skipped"]) == 0
    env.close()


# ---- 10. out-of-range rows, and the refusals ----
def test_out_of_range_rows_contribute_nothing(handles, oracle_mod):
    import torch
    case = SH.CASES[3]   # (40, 2), 2 x 32 tanh, C = 2, M = 64, narrow bounds
    env = handles(SH.ENVS[case[0]])
    b = SH.case_data(torch, oracle_mod, case)
    pol, critic, data = b["pol"], b["critic"], b["data"]
    n, M = data["obs"].shape[0], 70
    rows = torch.arange(M, dtype=torch.int32) % n
    bad = rows.clone()
    hole = torch.tensor([0, 5, 63, 64, 69])
    bad[hole] = torch.tensor([-1, n, 2 ** 31 - 1, -2 ** 31, n + 7], dtype=torch.int32)
    got = _grad(env, pol, critic, data, bad)
    torch.cuda.synchronize()
    assert int(got["stats"]["rows_used"]) == M - 5 and int(got["stats"]["rows_skipped"]) == 5
    for k in PER_ENTRY:
        t = got[k].cpu()
        assert not (t[:, hole] if k == "q" else t[hole]).any(), k
    keep = torch.ones(M, dtype=torch.bool)
    keep[hole] = False
    eps, neps = got["eps"].cpu()[keep], got["next_eps"].cpu()[keep]
    ref = SH.autograd(torch, pol, critic, data, rows.long()[keep], eps, neps, torch.float64, "cpu", M)   # the divisor stays M
    yard = SH.autograd(torch, pol, critic, data, rows.long()[keep], eps, neps, torch.float32, env.device, M)
    pooled = max(_rel(yard[k], ref[k]) for k in ref)
    for i, t in enumerate(pol.unpack(got["grad_params"].cpu().double())):
        assert _rel(t, ref[f"actor.{i}"]) <= 4.0 * pooled, i
    assert _rel(got["grad_log_alpha"].cpu().double(), ref["log_alpha"]) <= 4.0 * pooled


def test_gradient_refusals(handles):
    import torch
    from rsoccer_amd import _lib
    from rsoccer_amd.vec.policy import MLPGaussianPolicy, MLPPolicy, MLPQCritic
    env = handles("VecVSSEnv")
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    pol, critic = MLPGaussianPolicy(OD, AD, hidden=32, layers=1), MLPQCritic(OD, AD, hidden=32, layers=1)
    N = 10
    data = {"obs": torch.zeros(N, OD, device=dev), "actions": torch.zeros(N, AD, device=dev), "reward": torch.zeros(N, device=dev),
            "next_obs": torch.zeros(N, OD, device=dev), "terminated": torch.zeros(N, dtype=torch.bool, device=dev)}
    p, cp, la = torch.zeros(pol.num_params, device=dev), torch.zeros(2, critic.num_params, device=dev), torch.zeros(1, device=dev)
    ok = env.sac_gradient(data, pol, p, critic, cp, cp.clone(), la)
    assert set(ok) == {"grad_params", "grad_critic_params", "grad_log_alpha", "stats"} and set(ok["stats"]) == set(_lib.SAC_STATS)
    plain = MLPPolicy(OD, AD, hidden=32, layers=1)
    for args, kw in (((data, plain, torch.zeros(plain.num_params, device=dev), critic, cp, cp, la), {}),
                     ((data, pol, p, plain, cp, cp, la), {}),
                     ((data, pol, p[:-1], critic, cp, cp, la), {}),
                     ((data, pol, p, critic, cp[0], cp[0], la), {}),
                     ((data, pol, p, critic, cp, cp[:1], la), {}),
                     ((data, pol, p, critic, cp, cp, torch.zeros(2, device=dev)), {}),
                     ((data, pol, p, critic, cp, cp, la.cpu()), {}),
                     ((data, pol, p, critic, cp, cp, 0.0), {}),
                     ((data, pol, p, critic, cp, cp, la), dict(gamma=1.5)),
                     ((data, pol, p, critic, cp, cp, la), dict(target_entropy=float("nan"))),
                     ((data, pol, p, critic, cp, cp, la), dict(max_workgroups=0)),
                     ((data, pol, p, critic, cp, cp, la), dict(rows=[0, N])),
                     (({k: v for k, v in data.items() if k != "reward"}, pol, p, critic, cp, cp, la), {})):
        with pytest.raises(ValueError):
            env.sac_gradient(*args, **kw)
    # the C layer: what the Python layer cannot send
    ws = torch.empty(env.sim.sac_gradient_workspace(pol.spec(), critic.spec(), 2, N) // 4 + 1, device=dev)
    g = [torch.full((k,), 7.0, device=dev) for k in (pol.num_params, 2 * critic.num_params, 1, 12)]
    inp = _lib.DpgIn(*(data[k].data_ptr() for k in ("obs", "actions", "reward", "next_obs", "terminated")), None, N, N)
    good_cfg = lambda **kw: _lib.SacCfg(**{**dict(noise_step_dev=None, noise_seed=1, noise_step=0, gamma=0.99, target_entropy=-2.0,   # noqa: E731
                                                  log_std_min=-20.0, log_std_max=2.0, n_critics=2, max_workgroups=0), **kw})
    good_out = lambda **kw: _lib.SacOut(**{**dict(grad_actor=g[0].data_ptr(), grad_critics=g[1].data_ptr(), grad_log_alpha=g[2].data_ptr(),   # noqa: E731
                                                  stats=g[3].data_ptr(), workspace=ws.data_ptr()), **kw})

    def call(actor=pol.spec(), cr=critic.spec(), la_ptr=la.data_ptr(), cfg=good_cfg(), out=good_out(), i=inp):
        env.sim.task_sac_gradient(actor, p.data_ptr(), cr, cp.data_ptr(), cp.data_ptr(), la_ptr, i, cfg, out, env._stream())

    for kw in (dict(actor=None), dict(actor=plain.spec()), dict(cr=None), dict(cr=plain.spec()), dict(la_ptr=None), dict(cfg=None), dict(out=None),
               dict(i=None), dict(cfg=good_cfg(n_critics=3)), dict(cfg=good_cfg(gamma=-0.1)), dict(cfg=good_cfg(target_entropy=float("inf"))),
               dict(cfg=good_cfg(log_std_min=2.0)), dict(cfg=good_cfg(log_std_max=float("nan"))), dict(cfg=good_cfg(max_workgroups=-1)),
               dict(out=good_out(grad_actor=None)), dict(out=good_out(grad_log_alpha=None)), dict(out=good_out(workspace=None)),
               dict(i=_lib.DpgIn(*(data[k].data_ptr() for k in ("obs", "actions", "reward", "next_obs", "terminated")), None, N, 0))):
        with pytest.raises(_lib.RsxError):
            call(**kw)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in g)   # nothing was enqueued
    call()
    torch.cuda.synchronize()
    assert not any(bool((t == 7.0).any()) for t in g[:3])
