"""VecFusedEnv.collect / rsx_task_collect_policy: on-policy rollouts with the MLP policy inside one launch.  The call's contract is
its own check: restoring the checkpoint taken before the call and stepping a twin with the recorded actions must reproduce every
recorded row and end in the very checkpoint the call left — byte for byte.  Comparisons are on bit patterns unless a bound is derived
next to them."""
import numpy as np
import pytest

import test_gpu_policy_lookahead as PL   # the selector family, the float32 bound of dense policies and its measured tanh allowance

pytestmark = pytest.mark.gpu

B, WARM = 9, 3   # one full 8-env tile and a ragged one at 8 lanes per env
CLASSES = PL.CLASSES
DOM_POLICY = 7
_same, _policy, _dense, _make = PL._same, PL._policy, PL._dense, PL._make


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}   # (next_obs is a view of the engine's buffer: copied here)


def _where(a, b):
    """where two arrays differ in bits, for an assertion message"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shapes {a.shape} / {b.shape}, dtypes {a.dtype} / {b.dtype}"
    d = PL._bits(a) != PL._bits(b)
    idx = np.argwhere(d)
    return f"{int(d.sum())} of {d.size} entries differ, first at {idx[:4].tolist()}: {a[d][:4].tolist()} / {b[d][:4].tolist()}"


def _start(torch, env, warm=WARM):
    env.reset()
    if warm:
        env.step_random(warm)
    torch.cuda.synchronize()


def _raw(torch, env, pol, params, T, sigma=None, seed=0, spec="default", out="default", skip=()):
    """rsx_task_collect_policy itself, all seven records asked for -> host arrays (sigma: [act_dim] values or None)"""
    from rsoccer_amd import _lib
    dev, n, OD, AD = env.device, env.num_envs, env.sim.obs_dim, env.sim.act_dim
    rows = max(T, 1)   # (a refused T still gets real arrays)
    t = {"obs": torch.full((rows, n, OD), 7.0, device=dev), "actions": torch.full((rows, n, AD), 7.0, device=dev),
         "rewards": torch.full((rows, n), 7.0, device=dev), "flags": torch.full((rows, n), 77, dtype=torch.uint8, device=dev),
         "final_obs": torch.zeros((rows, n, OD), device=dev), "mean": torch.full((rows, n, AD), 7.0, device=dev),
         "sample": torch.full((rows, n, AD), 7.0, device=dev)}
    rec = _lib.CollectOut(*[None if k in skip else t[k].data_ptr() for k in ("obs", "actions", "rewards", "flags", "final_obs", "mean", "sample")])
    p = None if params is None else params.to(dev).contiguous()
    s = None if sigma is None else torch.tensor(sigma, dtype=torch.float32, device=dev)
    env.sim.task_collect_policy(pol.spec() if spec == "default" else spec, None if p is None else p.data_ptr(),
                                None if s is None else s.data_ptr(), seed, T, rec if out == "default" else out, env._stream())
    torch.cuda.synchronize()
    return _host(t)


def _twin_check(torch, env, pol, params, T, tag="", after=0, **kw):
    """collect, then restore and step a twin with the recorded actions: every row and the final checkpoint agree"""
    blob0 = env.checkpoint()
    tick0 = env.sim.task_tick()
    out = _host(env.collect(pol, params, T, return_final_obs=True, **kw))
    blob1 = env.checkpoint()
    met1 = env.metrics()
    assert env.sim.task_tick() == tick0 + T, tag
    later = []
    for _ in range(after):   # more single steps behind the call (the placement cache after a collect)
        env.step(None)
        torch.cuda.synchronize()
        later.append({k: env._t[k].cpu().numpy() for k in ("obs", "reward", "terminated", "truncated")})
    blob2 = env.checkpoint()
    env.restore(blob0)
    acts = torch.from_numpy(out["actions"]).to(env.device)
    for t in range(T):
        torch.cuda.synchronize()
        assert _same(env._t["obs"].cpu().numpy(), out["obs"][t]), (tag, "obs", t)
        _, rew, term, trunc, info = env.step(acts[t])
        torch.cuda.synchronize()
        assert _same(rew.cpu().numpy(), out["reward"][t]), (tag, "reward", t)
        assert np.array_equal(term.cpu().numpy().astype(bool), out["terminated"][t]), (tag, "terminated", t)
        assert np.array_equal(trunc.cpu().numpy().astype(bool), out["truncated"][t]), (tag, "truncated", t)
        ended = out["terminated"][t] | out["truncated"][t]
        fin = info["final_obs"].cpu().numpy()
        assert _same(fin[ended], out["final_obs"][t][ended]), (tag, "final_obs", t, _where(fin[ended], out["final_obs"][t][ended]))
        assert not out["final_obs"][t][~ended].any(), (tag, "final_obs written at a row that did not end", t)
    torch.cuda.synchronize()
    assert _same(env._t["obs"].cpu().numpy(), out["next_obs"]), (tag, "next_obs")
    assert np.array_equal(env.checkpoint(), blob1), (tag, "checkpoint")
    assert env.metrics() == met1, (tag, "metrics")
    for i, want in enumerate(later):
        env.step(None)
        torch.cuda.synchronize()
        for k, v in want.items():
            assert _same(env._t[k].cpu().numpy(), v), (tag, "after", i, k)
    if after:
        assert np.array_equal(env.checkpoint(), blob2), (tag, "checkpoint after the later steps")
    assert np.all(np.abs(out["actions"]) <= 1.0) and out["actions"].any(), tag
    return out


# ---- 1. the contract, every task class ----
@pytest.mark.parametrize("name", CLASSES)
def test_collect_is_n_steps_with_the_recorded_actions(name):
    import torch
    from rsoccer_amd import vec
    env = _make(vec, name, B, device=0, seed=2025, max_episode_steps=5)
    _start(torch, env)
    pol = _policy(env)
    out = _twin_check(torch, env, pol, _dense(torch, pol, 1)[0], 12, tag=name)
    ends = (out["terminated"] | out["truncated"]).sum(0)
    print(name, "episode ends per env inside the launch", ends, "truncated", out["truncated"].sum(0))
    # 3 warm steps, TimeLimit 5, 12 steps: truncations at rows 1, 6 and 11 — unless a termination restarts the count in between
    # (SSLPassEndurance ends episodes early), which is one more episode end and re-placement inside the launch
    assert np.all(ends >= 2), "uninformative: an env was not re-placed twice inside the launch"
    assert np.all((out["truncated"].sum(0) >= 2) | out["terminated"].any(0)) and np.all(out["truncated"].sum(0) >= 1), \
        "uninformative: an env that never terminated was not truncated twice inside the launch"
    env.close()


# ---- 2. terminations, and single steps behind the call ----
@pytest.mark.parametrize("name", ["VecSSLStaticDefendersEnv", "VecSSLContestedPossessionEnv"])
def test_terminations_inside_the_launch(name):
    import torch
    from rsoccer_amd import vec
    env = getattr(vec, name)(256, device=0, seed=7)
    _start(torch, env, 25)
    pol = _policy(env)
    out = _twin_check(torch, env, pol, _dense(torch, pol, 1, seed=101)[0], 40, tag=name, after=5)
    per_env = out["terminated"].any(0)
    print(name, "terminated rows", int(out["terminated"].sum()), "envs that never terminated", int((~per_env).sum()))
    assert per_env.any() and not per_env.all(), "uninformative: no mix of terminated and running envs"
    env.close()


# ---- 3. the actions are the policy's answer to the recorded observations ----
@pytest.mark.parametrize("layers,hidden", [(1, 32), (2, 64)])
def test_selector_policies_are_evaluated_exactly(layers, hidden):
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(B, device=0, seed=11, max_episode_steps=5)
    _start(torch, env)
    pol = _policy(env, hidden=hidden, layers=layers, hidden_act="relu", out_act="clip")
    params = PL._selector(torch, pol, 1)
    out = _host(env.collect(pol, params, 8))
    want = pol.forward(torch.from_numpy(out["obs"]), params, dtype=torch.float32).numpy()   # on the host: every operation is exact
    assert _same(out["actions"], want)
    assert out["actions"].any() and out["truncated"].any()
    env.close()


@pytest.mark.parametrize("name", CLASSES)
def test_dense_policies_are_within_the_float32_bound(name):
    import torch
    from rsoccer_amd import vec
    env = _make(vec, name, B, device=0, seed=2025, max_episode_steps=5)
    _start(torch, env)
    pol = _policy(env)
    params = _dense(torch, pol, 1)[0]
    out = _host(env.collect(pol, params, 8))
    obs = torch.from_numpy(out["obs"]).reshape(-1, pol.obs_dim)
    want, bound = PL._forward_with_bound(torch, pol, obs, params)   # (4 x the measured tanh deviation per tanh, as there)
    err = (torch.from_numpy(out["actions"]).reshape(-1, pol.act_dim).double() - want).abs().numpy()
    print(name, "largest error", err.max(), "smallest bound", float(bound.min()), "worst error / bound", (err / bound.numpy()).max())
    assert np.all(err <= bound.numpy())
    env.close()


# ---- 4. the head ----
def _normal_pair(w0, w1):
    u1 = ((w0 >> 8) + 1) * 2.0 ** -24
    ang = ((w1 >> 8) * 2.0 ** -24 - 0.5) * 2.0 * np.pi
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(ang), rad * np.sin(ang)


def _eps64(O, seed64, base, tick0, T, n, AD):
    """the head's standard normals of include/rsx.h in float64: [T, n, AD]; words from the oracle's Philox (7 rounds)"""
    key = (seed64 & 0xFFFFFFFF, seed64 >> 32)
    eps = np.zeros((T, n, AD))
    for t in range(T):
        for e in range(n):
            for q in range((AD + 3) // 4):
                w = O.philox((base + e, 0, tick0 + t, DOM_POLICY | (q << 8)), key, rounds=7)
                nn = _normal_pair(w[0], w[1]) + _normal_pair(w[2], w[3])
                for c in range(min(4, AD - 4 * q)):
                    eps[t, e, 4 * q + c] = nn[c]
    return eps


@pytest.mark.parametrize("name", ["VecVSSEnv", "VecSSLStaticDefendersEnv"])   # act_dim 2 and 5: one noise block and two
def test_the_gaussian_head(oracle_mod, name):
    import torch
    from rsoccer_amd import vec
    T, base, seed64 = 6, 11, 0x0123456789ABCDEF   # (distinct halves: the key is (lo, hi))
    env = _make(vec, name, B, device=0, seed=9, env_id_base=base, max_episode_steps=5)
    _start(torch, env)
    AD = env.sim.act_dim
    pol = _policy(env, out_act="clip")
    # zero weights and a bias: the mean is the bias, in bits
    ts = [torch.zeros(s) for s in pol.shapes]
    bias = torch.tensor([0.3, -0.7, 0.11, 1.5, -2.25][:AD])
    ts[-1][:] = bias
    blob0 = env.checkpoint()
    flat = _raw(torch, env, pol, pol.pack(ts), T)
    assert _same(flat["mean"], np.broadcast_to(bias.numpy(), (T, B, AD)).copy())
    assert _same(flat["sample"], flat["mean"]) and _same(flat["actions"], np.clip(flat["mean"], -1.0, 1.0))
    # sigma NULL: sample == mean, and the call is the call with sigma = 0
    params = _dense(torch, pol, 1)[0]
    env.restore(blob0)
    det = _raw(torch, env, pol, params, T)
    blob_det = env.checkpoint()
    assert _same(det["sample"], det["mean"])
    env.restore(blob0)
    zero = _raw(torch, env, pol, params, T, sigma=[0.0] * AD, seed=seed64)
    for k in det:
        assert _same(det[k], zero[k]), k
    assert np.array_equal(env.checkpoint(), blob_det)
    # sigma = 0.5 (0.25 for the last component): the formula, within the plan sampler's bound
    sig = np.array(([0.5] * AD)[:AD - 1] + [0.25], dtype=np.float32)
    env.restore(blob0)
    tick0 = env.sim.task_tick()
    assert tick0 == WARM
    got = _raw(torch, env, pol, params, T, sigma=list(sig), seed=seed64)
    eps = _eps64(oracle_mod, seed64, base, tick0, T, B, AD)
    want = got["mean"].astype(np.float64) + sig.astype(np.float64) * eps
    bound = 1e-5 * max(float(sig.max()), 1.0)
    err = np.abs(got["sample"].astype(np.float64) - want)
    print(f"{name}: max |device sample - float64 restatement| {err.max():.3e} (bound {bound:.1e}); eps std {eps.std():.3f}")
    assert err.max() <= bound
    assert 0.7 < eps.std() < 1.3 and abs(eps.mean()) < 0.3   # the restatement itself draws standard normals
    assert _same(got["actions"], np.clip(got["sample"], -1.0, 1.0))
    assert _same(got["obs"][0], det["obs"][0]) and not _same(got["actions"], det["actions"])
    # the same call again gives the same bits; another seed or another tick gives other noise
    env.restore(blob0)
    again = _raw(torch, env, pol, params, T, sigma=list(sig), seed=seed64)
    for k in got:
        assert _same(got[k], again[k]), k
    nxt = _raw(torch, env, pol, params, T, sigma=list(sig), seed=seed64)   # (behind it: ticks tick0 + T ...)
    env.restore(blob0)
    other = _raw(torch, env, pol, params, T, sigma=list(sig), seed=seed64 + 1)
    noise = lambda o: (o["sample"].astype(np.float64) - o["mean"]) / sig   # noqa: E731
    differs = lambda a, b: (np.abs(a - b) > 1e-3).mean() > 0.9   # noqa: E731  (independent normals: all but a few entries apart)
    assert differs(noise(other)[0], noise(got)[0]), "another noise_seed drew the same noise"
    assert differs(noise(nxt)[0], noise(got)[0]), "another tick drew the same noise"
    assert np.abs(noise(nxt) - _eps64(oracle_mod, seed64, base, tick0 + T, T, B, AD)).max() <= 1e-5 / float(sig.min())
    # env_id_base shifted by 4: env e of the shifted handle IS global env e + 4 — its noise, and with it everything else
    sh = _make(vec, name, B - 4, device=0, seed=9, env_id_base=base + 4, max_episode_steps=5)
    _start(torch, sh)
    shifted = _raw(torch, sh, pol, params, T, sigma=list(sig), seed=seed64)
    for k in got:
        assert _same(shifted[k], got[k][:, 4:]), k
    sh.close()
    # the twin check holds with noise on
    env.restore(blob0)
    out = _twin_check(torch, env, pol, params, T, tag=name + " noise", log_std=np.log(sig), noise_seed=seed64)
    assert _same(out["obs"][0], got["obs"][0]) and _same(out["mean"][0], got["mean"][0])   # (sigma = exp(log(sig)): maybe an ulp off sig)
    assert np.abs(out["sample"][0] - got["sample"][0]).max() <= 1e-5
    z = (out["sample"].astype(np.float64) - out["mean"]) / sig
    lp = (-0.5 * z * z - np.log(sig.astype(np.float64)) - 0.5 * np.log(2 * np.pi)).sum(-1)
    assert np.abs(out["log_prob"] - lp).max() <= 1e-4 * max(1.0, np.abs(lp).max())
    env.close()


# ---- 5. the batch split ----
def test_envs_do_not_see_the_batch():
    import torch
    from rsoccer_amd import vec
    outs = []
    for n in (B, 17):
        env = vec.VecSSLStaticDefendersEnv(n, device=0, seed=8, max_episode_steps=5)
        _start(torch, env)
        pol = _policy(env)
        outs.append(_host(env.collect(pol, _dense(torch, pol, 1)[0], 8, log_std=-1.0, noise_seed=5, return_final_obs=True)))
        env.close()
    for k, v in outs[0].items():
        assert _same(v, outs[1][k][:, :B] if v.ndim >= 2 and k != "next_obs" else outs[1][k][:B]), k
    assert outs[0]["truncated"].any()


# ---- 6. lane width ----
def test_16_lanes_per_env_give_the_same_bits(monkeypatch):
    import torch
    from rsoccer_amd import vec
    outs = []
    for lanes in (None, "16"):
        if lanes:
            monkeypatch.setenv("RSX_LANES_PER_ENV", lanes)
        env = vec.VecVSSEnv(B, device=0, seed=29, max_episode_steps=5)
        assert env.sim.task_layout() == ("16-lanes-per-env" if lanes else "8-lanes-per-env"), env.sim.task_layout()
        _start(torch, env)
        pol = _policy(env)
        outs.append(_twin_check(torch, env, pol, _dense(torch, pol, 1)[0], 8, tag=f"lanes {lanes}", log_std=-1.0, noise_seed=5))
        env.close()
    for k, v in outs[0].items():
        assert _same(v, outs[1][k]), k


def test_vss_5v5_native_16_lanes():
    import torch
    from rsoccer_amd import vec
    env = _make(vec, "VecVSS5v5", B, device=0, seed=29, max_episode_steps=5)
    assert env.sim.obs_dim == 64
    _start(torch, env)
    pol = _policy(env)
    out = _twin_check(torch, env, pol, _dense(torch, pol, 1)[0], 8, tag="5v5")
    assert out["truncated"].any()
    env.close()


# ---- 7. per-env physics ----
@pytest.mark.parametrize("id_,ranges", [("VSS-v0", {"m_ball": (0.04, 0.05), "mu_g": (0.2, 0.4)}),
                                        ("SSLStaticDefenders-v0", {"m_ball": (0.04, 0.05), "e_rb": (0.2, 0.6)})])
def test_per_env_physics_is_redrawn_inside_the_launch(id_, ranges):
    import torch
    import rsoccer_amd
    env = rsoccer_amd.make_vec(id_, B, device=0, seed=31, max_episode_steps=5, physics_ranges=ranges)
    _start(torch, env, 7)
    before = env.physics()["m_ball"].cpu().numpy()
    assert len(np.unique(before)) > 1
    pol = _policy(env)
    blob0 = env.checkpoint()
    env.collect(pol, _dense(torch, pol, 1)[0], 12)
    phys1 = {k: v.cpu().numpy() for k, v in env.physics().items()}
    assert not _same(phys1["m_ball"], before), "uninformative: no redraw inside the launch"
    env.restore(blob0)
    _twin_check(torch, env, pol, _dense(torch, pol, 1)[0], 12, tag=id_)
    for k, v in env.physics().items():
        assert _same(v.cpu().numpy(), phys1[k]), k
    env.close()


# ---- 8. device-keyed handles and graphs ----
def test_collect_replays_from_a_graph():
    import torch
    from rsoccer_amd import vec
    T = 6
    envs = [vec.VecVSSEnv(B, device=0, seed=17, max_episode_steps=5) for _ in range(2)]
    for e in envs:
        _start(torch, e)
        e.enable_graph_capture()
    env, twin = envs
    pol = _policy(env)
    params = _dense(torch, pol, 1)[0].to(env.device)
    log_std = torch.full((env.sim.act_dim,), -1.0, device=env.device)

    def run(e):
        return e.collect(pol, params, T, log_std=log_std, noise_seed=99, return_final_obs=True)

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
    noise = [(r["sample"] - r["mean"])[0] for r in recs]
    for a, b in ((0, 1), (1, 2)):
        assert ((noise[a] - noise[b]).abs() > 1e-4).float().mean() > 0.9, "a replay repeated its noise"
    for e in envs:
        e.close()


def test_captured_call_on_a_host_keyed_handle_is_refused():
    import torch
    from rsoccer_amd import _lib, vec
    env = vec.VecVSSEnv(B, device=0, seed=3)
    env.reset()
    env.step(None)
    torch.cuda.synchronize()
    before = env.checkpoint()
    pol = _policy(env)
    params = _dense(torch, pol, 1)[0].to(env.device)
    side = torch.cuda.Stream()
    with pytest.raises(_lib.RsxError, match="rsx_task_enable_capture"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
            env.collect(pol, params, 4)
    torch.cuda.synchronize()
    _lib.drop_pending_hip_error()   # what the aborted capture leaves behind
    assert np.array_equal(env.checkpoint(), before)   # nothing ran
    out = env.collect(pol, params, 4)                 # the env still collects, eagerly
    torch.cuda.synchronize()
    assert env.sim.task_tick() == 5 and out["obs"].shape == (4, B, env.sim.obs_dim)
    env.close()


# ---- 9. a handle whose single steps run one lane per env ----
def test_handle_that_steps_one_lane_per_env():
    """The collect kernel is the lane-group kernel; what this case adds is that it reads and leaves the arrays as the one-lane-per-env
    step keeps them (VSS-v0's task scalar row is not kept up to date there).  TimeLimit 5, two warm steps and T = 3: the last recorded row
    ends every episode, so the stepped twin takes all 98 304 auto-resets in the one-lane-per-env kernel and must reproduce collect's
    terminal observations and the checkpoint behind them."""
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(98304, device=0, seed=5, max_episode_steps=5)
    assert env.sim.task_layout() == "one-lane-per-env"
    _start(torch, env, 2)
    pol = _policy(env)
    out = _twin_check(torch, env, pol, _dense(torch, pol, 1)[0], 3, tag="98304 envs", log_std=-1.0, noise_seed=3)
    assert out["obs"].shape == (3, 98304, env.sim.obs_dim)
    assert (out["terminated"][2] | out["truncated"][2]).mean() >= 0.9, "uninformative: the last recorded row does not end (nearly) every env"
    env.close()


# ---- 10. edges and refusals ----
def test_a_single_step_and_the_refusals(monkeypatch):
    import torch
    from rsoccer_amd import _lib, vec
    from rsoccer_amd.vec.policy import MLPPolicy
    env = vec.VecVSSEnv(B, device=0, seed=1, max_episode_steps=5)
    pol = _policy(env)
    params = _dense(torch, pol, 1)[0]
    with pytest.raises(_lib.RsxError, match="reset"):
        env.collect(pol, params, 3)
    _start(torch, env)
    out = _twin_check(torch, env, pol, params, 1, tag="T = 1")   # (asserts that the tick advanced by exactly T)
    assert out["obs"].shape == (1, B, env.sim.obs_dim)
    before, tick = env.checkpoint(), env.sim.task_tick()
    bad_specs = [_lib.PolicyMLP(2, 48, _lib.ACT_TANH, _lib.ACT_TANH), _lib.PolicyMLP(3, 64, _lib.ACT_TANH, _lib.ACT_TANH),
                 _lib.PolicyMLP(2, 64, 7, _lib.ACT_TANH), _lib.PolicyMLP(2, 64, _lib.ACT_TANH, _lib.ACT_RELU)]
    for bad in [dict(spec=b) for b in bad_specs] + [dict(spec=None), dict(T=0), dict(T=-1), dict(out=None)] + \
               [dict(skip=(k,)) for k in ("obs", "actions", "rewards", "flags")]:
        T = bad.pop("T", 2)
        with pytest.raises(_lib.RsxError):
            _raw(torch, env, pol, params, T, **bad)
    with pytest.raises(_lib.RsxError):   # n_steps above RSX_N_STEPS_MASK (no array of that size is touched: refused first)
        env.sim.task_collect_policy(pol.spec(), params.to(env.device).data_ptr(), None, 0, 1 << 30, _lib.CollectOut(1, 1, 1, 1), env._stream())
    with pytest.raises(_lib.RsxError):   # null params
        _raw(torch, env, pol, None, 2)
    untouched = _raw(torch, env, pol, params, 2, skip=("final_obs", "mean", "sample"))   # the optional arrays may be NULL
    assert (untouched["mean"] == 7.0).all() and (untouched["sample"] == 7.0).all() and not (untouched["actions"] == 7.0).any()
    env.restore(before)
    # the Python layer
    for kw in (dict(steps=0), dict(steps=2, log_std=float("nan")), dict(steps=2, log_std=[0.0, float("inf")]), dict(steps=2, log_std=[0.0] * 3)):
        with pytest.raises(ValueError):
            env.collect(pol, params, **kw)
    for shape in ((pol.num_params - 1,), (1, pol.num_params), (2, pol.num_params)):
        with pytest.raises(ValueError):
            env.collect(pol, torch.zeros(*shape), 2)
    with pytest.raises(ValueError):   # a policy for another task's dims
        env.collect(MLPPolicy(24, 5), torch.zeros(MLPPolicy(24, 5).num_params), 2)
    torch.cuda.synchronize()
    assert np.array_equal(env.checkpoint(), before) and env.sim.task_tick() == tick   # nothing was enqueued
    out = env.collect(pol, params.double().numpy(), 2, log_std=0.0)   # numpy / float64 parameters and a scalar log_std are converted
    assert set(out) == {"obs", "actions", "reward", "terminated", "truncated", "next_obs", "mean", "sample", "log_prob"}
    assert env.sim.task_tick() == tick + 2
    env.close()

    # the scrimmage commands every robot: refused by the engine even for a policy of its dims
    scr = vec.VecSSLScrimmageEnv(B, device=0, seed=1)
    scr.reset()
    spol = MLPPolicy(scr.sim.obs_dim, scr.sim.act_dim)
    with pytest.raises(_lib.RsxError, match="scrimmage"):
        scr.collect(spol, torch.zeros(spol.num_params), 3)
    scr.close()
    # a handle forced to 64 lanes per env: no such kernels
    monkeypatch.setenv("RSX_LANES_PER_ENV", "64")
    wide = vec.VecVSSEnv(B, device=0, seed=1)
    assert wide.sim.task_layout() == "64-lanes-per-env"
    wide.reset()
    with pytest.raises(_lib.RsxError, match="64-lanes-per-env"):
        wide.collect(pol, params, 2)
    wide.close()
