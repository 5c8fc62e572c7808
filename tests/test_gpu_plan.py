"""Planning with candidates drawn on the device: VecFusedEnv.plan / plan_candidates, rsx_task_lookahead_sampled / rsx_plan_candidates /
rsx_plan_update (include/rsx.h: rsx_plan_sampler).

The sampled lookahead is pinned against the EXISTING lookahead of the candidates it says it used (bit for bit; test_gpu_lookahead.py pins
that one against step()), the candidates against a numpy restatement of the sampler, and the update against a float64 fold of the
dumped candidates.  Bounds, where a comparison is not on bit patterns, are derived in the test that uses them."""
import numpy as np
import pytest

from test_gpu_lookahead import CLASSES, _check, _host, _make, _same

pytestmark = pytest.mark.gpu

DOM_PLAN = 6
ARG, STATE = "librsx_hip error -1:", "librsx_hip error -4:"   # RSX_ERR_ARG, RSX_ERR_STATE (include/rsx.h) as _lib reports them


def _mean(torch, env, H, seed, scale=0.8):
    """[B, H, act_dim] normal * scale: with scale 0.8 a fifth of the entries lie beyond +-1, so the clamp acts"""
    m = (np.random.default_rng(seed).standard_normal((env.num_envs, H, env.sim.act_dim)) * scale).astype(np.float32)
    return torch.from_numpy(m).to(env.device)


def _sampled_equals_lookahead(torch, env, mean, K, H, tag, gammas=(1.0, 0.97), **smp):
    cand = env.plan_candidates(mean=mean, horizon=H, K=K, **smp)
    assert cand.shape == (env.num_envs, K, H, env.sim.act_dim)
    for gamma in gammas:
        got = _host(env.plan(mean=mean, horizon=H, K=K, gamma=gamma, return_obs=True, **smp))
        want = _host(env.lookahead(cand, gamma=gamma, return_obs=True))
        print(f"{tag} gamma {gamma}: pairs ended inside the horizon {int((want['terminated'] | want['truncated']).sum())} of {want['steps'].size}")
        _check(got, want, f"{tag} gamma {gamma}")
    return cand


# ---- 1. the sampled launch is the lookahead of its own candidates ----
@pytest.mark.parametrize("name", CLASSES)
def test_sampled_lookahead_equals_lookahead_of_its_candidates(name):
    import torch
    from rsoccer_amd import vec
    env = _make(vec, name, 9, device=0, seed=2025)
    env.reset()
    env.step_random(200)
    cand = _sampled_equals_lookahead(torch, env, _mean(torch, env, 7, 5), K=3, H=7, tag=name, sigma=0.5, hold=3)
    c = cand.cpu().numpy()
    assert np.abs(c).max() <= 1.0 and (np.abs(c) == 1.0).any(), "uninformative: the clamp never acted"
    assert not _same(c[:, 1], c[:, 2])
    env.close()


@pytest.mark.parametrize("id_,ranges", [("VSS-v0", {"m_ball": (0.04, 0.05), "mu_g": (0.2, 0.4)}),
                                        ("SSLStaticDefenders-v0", {"m_ball": (0.04, 0.05), "e_rb": (0.2, 0.6)})])
def test_sampled_lookahead_with_per_env_physics(id_, ranges):
    import torch
    import rsoccer_amd
    env = rsoccer_amd.make_vec(id_, 9, device=0, seed=31, max_episode_steps=60, physics_ranges=ranges)
    env.reset()
    env.step_random(200)   # >= 3 auto-resets per env: the coefficients were redrawn and differ per env
    torch.cuda.synchronize()
    assert len(np.unique(env.physics()["m_ball"].cpu().numpy())) > 5
    _sampled_equals_lookahead(torch, env, _mean(torch, env, 7, 6), K=3, H=7, tag=id_ + " physics", sigma=0.5, hold=3)
    env.close()


# ---- 2. the candidates follow the formula ----
def _normal_pair(w0, w1):
    u1 = ((w0 >> 8) + 1) * 2.0 ** -24
    ang = ((w1 >> 8) * 2.0 ** -24 - 0.5) * 2.0 * np.pi
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(ang), rad * np.sin(ang)


def _restated(O, seed64, sigma, hold, tick, base, mean, K):
    """the sampler of include/rsx.h in float64, before the clamp: [B, K, H, AD]; words from the oracle's Philox (7 rounds)"""
    B, H, AD = mean.shape
    nblk = (AD + 3) // 4
    key = (seed64 & 0xFFFFFFFF, seed64 >> 32)
    out = np.repeat(mean.astype(np.float64)[:, None], K, axis=1)
    for e in range(B):
        for k in range(1, K):
            for s in range((H + hold - 1) // hold):
                for j in range(nblk):
                    w = O.philox((base + e, k, tick, DOM_PLAN | ((s * nblk + j) << 8)), key, rounds=7)
                    n = _normal_pair(w[0], w[1]) + _normal_pair(w[2], w[3])
                    for c in range(min(4, AD - 4 * j)):
                        out[e, k, s * hold:(s + 1) * hold, 4 * j + c] += sigma * n[c]
    return out


@pytest.mark.parametrize("name", ["VecVSSEnv", "VecSSLStaticDefendersEnv", "VecSSLDribblingEnv", "VecSSLScrimmageEnv"])
def test_candidates_follow_the_formula(oracle_mod, name):
    import torch
    from rsoccer_amd import _lib, vec
    B, K, H, hold, sigma, base = 5, 4, 7, 3, 0.3, 11
    env = _make(vec, name, B, device=0, seed=9, env_id_base=base)
    env.reset()
    env.step_random(3)
    tick = env.sim.task_tick()
    assert tick == 3
    AD = env.sim.act_dim
    mean = np.random.default_rng(1).uniform(-0.3, 0.3, (B, H, AD)).astype(np.float32)
    m = torch.from_numpy(mean).to(env.device)
    seed64 = 0x0123456789ABCDEF   # (distinct halves: the key is (lo, hi))
    out = torch.empty(B, K, H, AD, device=env.device)
    env.sim.plan_candidates(m.data_ptr(), _lib.PlanSampler(seed64, sigma, hold), K, H, out.data_ptr(), env._stream())
    got = out.cpu().numpy()
    want = _restated(oracle_mod, seed64, sigma, hold, tick, base, mean, K)
    # candidate 0 is the clamped plan, exactly
    assert _same(got[:, 0], np.clip(mean, -1.0, 1.0))
    # k >= 1: away from the clamp.  The excluded share is a condition checked on the restatement: |mean| <= 0.3 and sigma 0.3 put
    # +-1 at 2.3 sigma and beyond
    bound = 1e-5 * max(sigma, 1.0)
    away = np.abs(np.abs(want[:, 1:]) - 1.0) > bound
    share = 1.0 - away.mean()
    print(f"{name}: act_dim {AD}, entries left out at the clamp {share:.4f}")
    assert share <= 0.05
    err = np.abs(got[:, 1:].astype(np.float64) - np.clip(want[:, 1:], -1.0, 1.0))[away]
    print(f"{name}: max |device - float64 restatement| {err.max():.3e} (bound {bound:.1e})")
    assert err.max() <= bound
    # a segment repeats its noise `hold` times (the last one is ragged: 7 = 3 + 3 + 1), consecutive segments differ
    noise = got[:, 1:].astype(np.float64) - mean[:, None]
    inside = np.abs(got[:, 1:]) < 1.0
    for t in (1, 2, 4, 5):
        ok = inside[:, :, t] & inside[:, :, t - 1]
        assert np.abs(noise[:, :, t] - noise[:, :, t - 1])[ok].max() <= 2.0 ** -22   # same eps: two roundings of |a| < 1 apart
    for t in (3, 6):
        assert np.abs(noise[:, :, t] - noise[:, :, t - 1]).min(axis=-1).max() > 1e-3
    env.close()


# ---- 3. keyed by what, not where ----
def test_candidates_are_keyed_by_global_env_id_tick_and_iteration():
    import torch
    from rsoccer_amd import vec
    kw = dict(horizon=6, K=5, sigma=0.7, hold=2)
    part = vec.VecVSSEnv(4, device=0, seed=3, env_id_base=5)
    full = vec.VecVSSEnv(9, device=0, seed=3)
    part.reset()
    full.reset()
    a, b = part.plan_candidates(**kw), full.plan_candidates(**kw)
    assert torch.equal(a, b[5:9])
    assert not torch.equal(b[0], b[1])
    assert torch.equal(full.plan_candidates(**kw), b)          # two calls at one tick
    assert not torch.equal(full.plan_candidates(iteration=1, **kw)[:, 1:], b[:, 1:])
    assert not torch.equal(full.plan_candidates(seed=4, **kw)[:, 1:], b[:, 1:])
    full.step(None)
    c = full.plan_candidates(**kw)
    assert not torch.equal(c[:, 1:], b[:, 1:])                 # after a step: fresh ones
    assert torch.equal(c[:, 0], b[:, 0])                       # (candidate 0 is the plan itself)
    part.close()
    full.close()


# ---- 4. the update ----
def _plan_and_dump(torch, env, mean, **kw):
    cand = env.plan_candidates(mean=mean, **{k: v for k, v in kw.items() if k not in ("temperature", "gamma")})
    out = env.plan(mean=mean, **kw)
    torch.cuda.synchronize()
    return cand.cpu().numpy(), _host(out)


@pytest.mark.parametrize("K", [3, 130])
def test_update_folds_the_returns_into_a_plan(K):
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(9, device=0, seed=14)
    env.reset()
    env.step_random(60)
    B, H = 9, 7
    mean = _mean(torch, env, H, 8, scale=0.5)
    kw = dict(K=K, sigma=0.5, hold=3, gamma=0.97)
    rows = np.arange(B)
    # temperature 0: the first argmax, and that candidate bit for bit
    cand, out = _plan_and_dump(torch, env, mean, temperature=0.0, **kw)
    best = np.argmax(out["return"], axis=1)   # (numpy: the first maximum)
    assert out["best"].dtype == np.int32 and np.array_equal(out["best"], best)
    assert _same(out["mean"], cand[rows, best])
    assert _same(out["action"], cand[rows, best, 0])
    assert len(np.unique(best)) > 1 or K == 3
    # a forced tie: sigma 0 makes all candidates equal, so all returns are, and the lowest index wins
    _, tie = _plan_and_dump(torch, env, mean, temperature=0.0, **dict(kw, sigma=0.0))
    assert np.all(tie["return"] == tie["return"][:, :1]) and np.all(tie["best"] == 0)
    assert _same(tie["mean"], np.clip(mean.cpu().numpy(), -1.0, 1.0))
    # temperature 0.5: the softmax-weighted mean.  Bound: K float32 products of magnitude <= 1 under weights that sum to 1, plus the
    # weights' own rounding: (K + 8) * 2^-23
    cand, out = _plan_and_dump(torch, env, mean, temperature=0.5, **kw)
    R = out["return"].astype(np.float64)
    w = np.exp((R - R.max(axis=1, keepdims=True)) / 0.5)
    w /= w.sum(axis=1, keepdims=True)
    want = np.einsum("bk,bkhd->bhd", w, cand.astype(np.float64))
    err = np.abs(out["mean"].astype(np.float64) - want).max()
    bound = (K + 8) * 2.0 ** -23
    print(f"K {K}: max |new mean - float64 softmax mean| {err:.3e} (bound {bound:.3e}); largest weight {w.max():.3f}, smallest {w.min():.2e}")
    assert err <= bound
    assert np.array_equal(out["best"], np.argmax(out["return"], axis=1))
    # the same call twice: the same bits
    _, again = _plan_and_dump(torch, env, mean, temperature=0.5, **kw)
    for key in ("mean", "best", "return", "action"):
        assert _same(again[key], out[key]), key
    env.close()


def test_update_in_place_and_overlap():
    import torch
    from rsoccer_amd import _lib, vec
    env = vec.VecSSLStaticDefendersEnv(9, device=0, seed=2)
    env.reset()
    B, K, H, AD = 9, 6, 5, env.sim.act_dim
    smp = _lib.PlanSampler(77, 0.4, 2)
    mean = _mean(torch, env, H, 3, scale=0.4)
    ret = torch.from_numpy(np.random.default_rng(5).standard_normal((B, K)).astype(np.float32)).to(env.device)
    new = torch.empty_like(mean)
    best = torch.empty(B, dtype=torch.int32, device=env.device)
    for temp in (0.0, 0.5):
        env.sim.plan_update(mean.data_ptr(), smp, K, H, ret.data_ptr(), temp, new.data_ptr(), best.data_ptr(), env._stream())
        inplace = mean.clone()
        env.sim.plan_update(inplace.data_ptr(), smp, K, H, ret.data_ptr(), temp, inplace.data_ptr(), None, env._stream())   # best_dev may be NULL
        torch.cuda.synchronize()
        assert torch.equal(inplace, new) and not torch.equal(new, mean)
        assert torch.equal(best.long(), ret.argmax(dim=1))
    buf = torch.zeros(B * H * AD + 4, device=env.device)
    buf[:B * H * AD] = mean.reshape(-1)
    torch.cuda.synchronize()
    before = buf.clone()
    with pytest.raises(_lib.RsxError, match="overlaps"):
        env.sim.plan_update(buf.data_ptr(), smp, K, H, ret.data_ptr(), 0.5, buf.data_ptr() + 16, None, env._stream())
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    env.close()


# ---- 5. no side effects ----
@pytest.mark.parametrize("device_keyed", [False, True])
def test_plan_leaves_the_handle_exactly_as_it_was(device_keyed):
    import torch
    from rsoccer_amd import vec
    for name in ("VecVSSEnv", "VecSSLStaticDefendersEnv"):   # (static defenders at this batch: placement cache, helper slots)
        env, twin = (getattr(vec, name)(200, device=0, seed=12, max_episode_steps=30) for _ in range(2))
        for e in (env, twin):
            e.reset()
            e.step_random(50)
            if device_keyed:
                e.enable_graph_capture()
                e.step(None)
        torch.cuda.synchronize()
        before = env.checkpoint()
        views = {k: env._t[k].clone() for k in ("obs", "reward", "terminated", "truncated", "final_obs", "info", "steps")}
        tick = env.sim.task_tick()
        out = env.plan(mean=_mean(torch, env, 20, 3), K=6, sigma=0.5, hold=4, temperature=0.3, gamma=0.9, return_obs=True)
        env.plan_candidates(horizon=20, K=6)
        torch.cuda.synchronize()
        assert int(out["steps"].max()) > 0
        assert np.array_equal(env.checkpoint(), before), name   # state, counters, noise, metrics, step counter
        assert env.sim.task_tick() == tick
        for k, v in views.items():
            assert torch.equal(env._t[k], v), (name, k)
        env.step(None)      # the next step does what it would have done without the call
        twin.step(None)
        torch.cuda.synchronize()
        for k in ("obs", "reward", "terminated", "truncated"):
            assert torch.equal(env._t[k], twin._t[k]), (name, k)
        assert np.array_equal(env.checkpoint(), twin.checkpoint())
        env.close()
        twin.close()


# ---- 6. graph ----
def test_plan_then_step_replays_from_a_graph():
    import torch
    from rsoccer_amd import vec
    B, K, H = 64, 8, 6
    envs = [vec.VecVSSEnv(B, device=0, seed=17, max_episode_steps=40) for _ in range(2)]
    for env in envs:
        env.reset()
        env.step_random(10)
        env.enable_graph_capture()
    env, twin = envs
    AD = env.sim.act_dim
    plans = [torch.zeros(B, H, AD, device=env.device) for _ in envs]

    def plan_and_act(e, plan):
        noise = e.plan_candidates(horizon=H, K=K, sigma=0.4, hold=2)   # (zero mean: what differs between calls is the noise alone)
        out = e.plan(mean=plan, K=K, sigma=0.4, hold=2, temperature=0.5, gamma=0.97)
        e.step(out["action"])
        plan.copy_(out["mean"])   # warm start
        return out, noise

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # torch's warm-up before a capture: real calls, the twin makes them too
        for _ in range(2):
            plan_and_act(env, plans[0])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(2):
        plan_and_act(twin, plans[1])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # one stream, no forked branches
        out, noise = plan_and_act(env, plans[0])
    assert env.sim.task_tick() == twin.sim.task_tick() == 12   # capturing enqueued nothing
    seen = []
    for i in range(3):
        g.replay()
        want, wnoise = plan_and_act(twin, plans[1])
        torch.cuda.synchronize()
        for key in ("return", "steps", "terminated", "truncated", "best", "mean", "action"):
            assert torch.equal(out[key], want[key]), (i, key)
        assert torch.equal(noise, wnoise) and torch.equal(plans[0], plans[1])
        for key in ("obs", "reward", "terminated", "truncated", "final_obs"):
            assert torch.equal(env._t[key], twin._t[key]), (i, key)
        seen.append(noise.clone())
    assert not torch.equal(seen[0][:, 1:], seen[1][:, 1:]) and not torch.equal(seen[1][:, 1:], seen[2][:, 1:]) and not torch.equal(seen[0][:, 1:], seen[2][:, 1:])
    assert env.sim.task_tick() == twin.sim.task_tick() == 15
    assert np.array_equal(env.checkpoint(), twin.checkpoint())
    for e in envs:
        e.close()


# ---- 7. large batch: stepping runs the one-lane-per-env layout, the sampled lookahead the lane groups ----
def test_large_batch_other_layout():
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(98304, device=0, seed=6)
    assert env.sim.task_layout() == "one-lane-per-env"
    env.reset()
    env.step_random(30)
    _sampled_equals_lookahead(torch, env, _mean(torch, env, 3, 2), K=2, H=3, tag="98304 envs", gammas=(0.97,), sigma=0.5, hold=2)
    env.close()


# ---- 8. refusals ----
def test_refusals(monkeypatch):
    import torch
    from rsoccer_amd import _lib, vec
    dev = torch.device("cuda", 0)
    B, K, H, AD = 16, 2, 3, 2
    sim = _lib.Sim(_lib.KIND_VSS, 0, 3, 3, 25, B, 0)
    sim.task_attach(_lib.TASK_VSS_V0, 1, 0, 0)
    m = torch.zeros(B, H, AD, device=dev)
    a = torch.full((B, K, H, AD), 7.0, device=dev)
    new = torch.full((B, H, AD), 7.0, device=dev)
    r = torch.full((B, K), 7.0, device=dev)
    s = torch.full((B, K), 7, dtype=torch.int32, device=dev)
    f = torch.zeros(B, K, dtype=torch.uint8, device=dev)
    good = _lib.PlanSampler(1, 0.5, 1)

    def look(K=K, H=H, smp=good, gamma=1.0, rp=r.data_ptr(), sp=s.data_ptr(), fp=f.data_ptr()):
        sim.task_lookahead_sampled(m.data_ptr(), smp, K, H, gamma, rp, sp, fp, None, None)

    def cands(K=K, H=H, smp=good, op=a.data_ptr()):
        sim.plan_candidates(m.data_ptr(), smp, K, H, op, None)

    def update(K=K, H=H, smp=good, temp=0.0, rp=r.data_ptr(), np_=new.data_ptr()):
        sim.plan_update(m.data_ptr(), smp, K, H, rp, temp, np_, None, None)

    def nothing_ran():
        torch.cuda.synchronize()
        return int(s.min()) == 7 and float(a.min()) == 7.0 and float(new.min()) == 7.0

    for call in (look, cands, update):   # before the first reset
        with pytest.raises(_lib.RsxError, match=STATE + ".*reset"):
            call()
    sim.task_reset()
    bad_samplers = [None, _lib.PlanSampler(1, 0.5, 0), _lib.PlanSampler(1, -0.1, 1), _lib.PlanSampler(1, float("nan"), 1),
                    _lib.PlanSampler(1, float("inf"), 1)]
    for call in (look, cands, update):
        for bad in [dict(K=0), dict(H=0)] + [dict(smp=b) for b in bad_samplers]:
            with pytest.raises(_lib.RsxError, match=ARG):
                call(**bad)
    for bad in (dict(gamma=float("nan")), dict(rp=None), dict(sp=None), dict(fp=None)):
        with pytest.raises(_lib.RsxError, match=ARG):
            look(**bad)
    with pytest.raises(_lib.RsxError, match=ARG):
        cands(op=None)
    for bad in (dict(temp=-1.0), dict(temp=float("nan")), dict(temp=float("inf")), dict(rp=None), dict(np_=None)):
        with pytest.raises(_lib.RsxError, match=ARG):
            update(**bad)
    # a block index that does not fit in 24 bits: ceil(H / hold) * ceil(act_dim / 4) > 2^24 (refused before anything is touched)
    with pytest.raises(_lib.RsxError, match=ARG + ".*24 bits"):
        cands(H=(1 << 24) + 1)
    assert nothing_ran()
    # a host-keyed handle inside a capture
    for call in (look, cands, update):
        side = torch.cuda.Stream()
        with pytest.raises(_lib.RsxError, match=STATE + ".*rsx_task_enable_capture"):
            with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
                st = torch.cuda.current_stream().cuda_stream
                if call is look:
                    sim.task_lookahead_sampled(m.data_ptr(), good, K, H, 1.0, r.data_ptr(), s.data_ptr(), f.data_ptr(), None, st)
                elif call is cands:
                    sim.plan_candidates(m.data_ptr(), good, K, H, a.data_ptr(), st)
                else:
                    sim.plan_update(m.data_ptr(), good, K, H, r.data_ptr(), 0.0, new.data_ptr(), None, st)
        torch.cuda.synchronize()
        _lib.drop_pending_hip_error()   # what the aborted capture leaves behind
    assert nothing_ran()
    look(); cands(); update()   # the valid calls run
    torch.cuda.synchronize()
    assert int(s.min()) == 3 and float(a.abs().max()) <= 1.0 and float(new.abs().max()) <= 1.0
    sim.close()

    # a handle forced to 64 lanes per env has no lookahead kernels
    monkeypatch.setenv("RSX_LANES_PER_ENV", "64")
    wide = _lib.Sim(_lib.KIND_VSS, 0, 3, 3, 25, B, 0)
    monkeypatch.delenv("RSX_LANES_PER_ENV")
    wide.task_attach(_lib.TASK_VSS_V0, 1, 0, 0)
    wide.task_reset()
    with pytest.raises(_lib.RsxError, match=ARG + ".*64-lanes-per-env"):
        wide.task_lookahead_sampled(m.data_ptr(), good, K, H, 1.0, r.data_ptr(), s.data_ptr(), f.data_ptr(), None, None)
    wide.close()

    # Python: wrong shapes and values raise ValueError before any call
    env = vec.VecVSSEnv(B, device=0, seed=1)
    with pytest.raises(_lib.RsxError, match="reset"):
        env.plan(horizon=3)
    env.reset()
    for shape in ((B, 3), (B - 1, 3, AD), (B, 3, AD + 1), (B, 0, AD), (3, AD)):
        with pytest.raises(ValueError):
            env.plan(mean=torch.zeros(*shape, device=dev))
        with pytest.raises(ValueError):
            env.plan_candidates(mean=torch.zeros(*shape, device=dev))
    for bad in (dict(), dict(horizon=0), dict(horizon=3, K=0), dict(horizon=3, sigma=-1.0), dict(horizon=3, hold=0),
                dict(horizon=3, temperature=-0.5), dict(horizon=3, gamma=float("nan")), dict(mean=torch.zeros(B, 3, AD, device=dev), horizon=4)):
        with pytest.raises(ValueError):
            env.plan(**bad)
    # numpy and float64 plans are converted the way step() converts; the default K is 64
    out64 = env.plan(mean=np.zeros((B, 3, AD)), return_obs=True)
    ref = env.plan(horizon=3, return_obs=True)
    assert ref["return"].shape == (B, 64) and ref["mean"].shape == (B, 3, AD) and ref["action"].shape == (B, AD) and ref["best"].shape == (B,)
    for k in ref:
        assert torch.equal(out64[k], ref[k]), k
    env.close()
