"""VecFusedEnv.lookahead / rsx_task_lookahead against the API that already exists: checkpoint(), then for each candidate restore()
and H calls of step(actions), discounted in numpy float32 by the rule of include/rsx.h (ret = ret + disc * reward; disc = disc *
gamma) up to each env's first episode end.  The engine's guarantee is bit-exactness, so every comparison is on bit patterns."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _actions(torch, env, K, H, seed):
    """[B, K, H, act_dim] uniform in [-1, 1), drawn on the host (the same on every box)"""
    a = np.random.default_rng(seed).uniform(-1.0, 1.0, (env.num_envs, K, H, env.sim.act_dim)).astype(np.float32)
    return torch.from_numpy(a).to(env.device)


def _reference(torch, env, actions, gamma):
    """the stepping reference; leaves the env where it was (restored from the checkpoint it starts from)"""
    B, K, H, _ = actions.shape
    OD = env.sim.obs_dim
    blob = env.checkpoint()
    g = np.float32(gamma)
    ret = np.zeros((B, K), np.float32)
    steps = np.zeros((B, K), np.int32)
    term = np.zeros((B, K), bool)
    trunc = np.zeros((B, K), bool)
    last = np.zeros((B, K, OD), np.float32)
    for k in range(K):
        env.restore(blob)
        disc = np.ones(B, np.float32)
        done = np.zeros(B, bool)
        for t in range(H):
            obs, rew, te, tr, info = env.step(actions[:, k, t])
            torch.cuda.synchronize()
            obs, rew, fin = obs.cpu().numpy(), rew.cpu().numpy(), info["final_obs"].cpu().numpy()
            te, tr = te.cpu().numpy() != 0, tr.cpu().numpy() != 0
            run = ~done
            ret[run, k] = ret[run, k] + disc[run] * rew[run]
            disc = disc * g
            steps[run, k] = t + 1
            end = run & (te | tr)
            term[end, k], trunc[end, k] = te[end], tr[end]
            last[end, k] = fin[end]
            if t == H - 1:
                keep = run & ~end
                last[keep, k] = obs[keep]
            done |= end
    env.restore(blob)
    torch.cuda.synchronize()
    return {"return": ret, "steps": steps, "terminated": term, "truncated": trunc, "last_obs": last}


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(got, want, tag):
    for key in ("steps", "terminated", "truncated", "return", "last_obs"):
        a, b = got[key], want[key]
        if not _same(a, b):
            bad = np.argwhere(_bits(a) != _bits(b))
            raise AssertionError(f"{tag}: {key} differs in {len(bad)} of {a.size} values, first at {bad[0].tolist()}: "
                                 f"{a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}")


def _parity(torch, env, K, H, warm, gammas=(1.0, 0.97), seed=77, tag=""):
    env.reset()
    if warm:
        env.step_random(warm)
    torch.cuda.synchronize()
    acts = _actions(torch, env, K, H, seed)
    outs = []
    for gamma in gammas:
        got = _host(env.lookahead(acts, gamma=gamma, return_obs=True))
        want = _reference(torch, env, acts, gamma)
        print(f"{tag} gamma {gamma}: pairs ended inside the horizon {int((want['terminated'] | want['truncated']).sum())} of {want['steps'].size}, "
              f"steps min {want['steps'].min()} max {want['steps'].max()}")
        _check(got, want, f"{tag} gamma {gamma}")
        outs.append(want)
    return outs


def _make(vec, name, B, **kw):
    if name == "VecVSS5v5":
        cls = type("VecVSS5v5Env", (vec.VecVSSEnv,), dict(N_BLUE=5, N_YELLOW=5))
        return cls(B, field_type=1, **kw)
    return getattr(vec, name)(B, **kw)


CLASSES = ["VecVSSEnv", "VecSSLStaticDefendersEnv", "VecSSLDribblingEnv", "VecSSLContestedPossessionEnv", "VecSSLPassEnduranceEnv",
           "VecSSLScrimmageEnv",   # 11v11: 32 lanes per env
           "VecVSS5v5"]            # 16 lanes per env


# ---- 1. parity, every task ----
@pytest.mark.parametrize("name", CLASSES)
def test_lookahead_equals_restore_and_step(name):
    import torch
    from rsoccer_amd import vec
    env = _make(vec, name, 37, device=0, seed=2025)
    _parity(torch, env, K=5, H=12, warm=200, tag=name)
    env.close()


# ---- 2. truncation inside the horizon ----
def test_pairs_stop_at_the_time_limit():
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(37, device=0, seed=4, max_episode_steps=7)
    env.reset()
    for warm in (0, 3):   # from an episode's first step (7 steps to the limit), then three steps in (4 steps)
        if warm:
            env.step_random(warm)
        acts = _actions(torch, env, 5, 12, 5 + warm)
        got = _host(env.lookahead(acts, gamma=0.97, return_obs=True))
        assert got["steps"].max() <= 7
        assert np.all(got["truncated"] | got["terminated"])
        assert got["truncated"].any()
        _check(got, _reference(torch, env, acts, 0.97), f"time limit, {warm} steps in")
    env.close()


# ---- 3. termination inside the horizon ----
# Seed, warm-up and action seed were picked with the CPU oracle (OracleEnv.task_step: attach(seed 7, env e), reset, 25 random
# steps, then the candidate's 40 actions): of the 1024 pairs 251 (static defenders) and 250 (contested possession) end inside the
# horizon, all of them terminated.
@pytest.mark.parametrize("name", ["VecSSLStaticDefendersEnv", "VecSSLContestedPossessionEnv"])
def test_pairs_stop_at_a_termination(name):
    import torch
    from rsoccer_amd import vec
    env = getattr(vec, name)(256, device=0, seed=7)
    env.reset()
    env.step_random(25)
    a = np.random.default_rng(101).uniform(-1.0, 1.0, (256, 4, 40, env.sim.act_dim)).astype(np.float32)
    acts = torch.from_numpy(a).to(env.device)
    got = _host(env.lookahead(acts, gamma=1.0, return_obs=True))
    want = _reference(torch, env, acts, 1.0)
    print(name, "reference: terminated pairs", int(want["terminated"].sum()), "of", want["terminated"].size)
    assert want["terminated"].any() and not want["terminated"].all(), "uninformative: the reference saw no mix of ended and running pairs"
    _check(got, want, name)
    assert np.all((got["steps"] < 40) <= got["terminated"])
    env.close()


# ---- 4. the handle is untouched ----
@pytest.mark.parametrize("device_keyed", [False, True])
def test_the_handle_is_left_exactly_as_it_was(device_keyed):
    import torch
    from rsoccer_amd import vec
    for name in ("VecVSSEnv", "VecSSLStaticDefendersEnv"):   # (static defenders at this batch: placement cache, helper slots)
        env = getattr(vec, name)(200, device=0, seed=12, max_episode_steps=30)
        env.reset()
        env.step_random(50)
        if device_keyed:
            env.enable_graph_capture()
            env.step(None)
        torch.cuda.synchronize()
        before = env.checkpoint()
        views = {k: env._t[k].clone() for k in ("obs", "reward", "terminated", "truncated", "final_obs", "info", "steps")}
        tick = env.sim.task_tick()
        out = env.lookahead(_actions(torch, env, 6, 20, 3), gamma=0.9, return_obs=True)
        torch.cuda.synchronize()
        assert int(out["steps"].max()) > 0
        assert np.array_equal(env.checkpoint(), before), name   # state, counters, noise, metrics, step counter
        assert env.sim.task_tick() == tick
        for k, v in views.items():
            assert torch.equal(env._t[k], v), (name, k)
        env.close()


# ---- 5. independence ----
def test_candidates_do_not_see_each_other():
    import torch
    from rsoccer_amd import vec
    env = vec.VecSSLStaticDefendersEnv(37, device=0, seed=8)
    env.reset()
    env.step_random(40)
    acts = _actions(torch, env, 5, 30, 21)
    full = _host(env.lookahead(acts, gamma=0.97, return_obs=True))
    for k in range(5):
        one = _host(env.lookahead(acts[:, k:k + 1].contiguous(), gamma=0.97, return_obs=True))
        for key, v in one.items():
            assert _same(v[:, 0], full[key][:, k]), (k, key)
    perm = [3, 0, 4, 2, 1]
    shuffled = _host(env.lookahead(acts[:, perm].contiguous(), gamma=0.97, return_obs=True))
    for key, v in shuffled.items():
        assert _same(v, np.ascontiguousarray(full[key][:, perm])), key
    env.close()


# ---- 6. per-env physics ----
@pytest.mark.parametrize("id_,ranges", [("VSS-v0", {"m_ball": (0.04, 0.05), "mu_g": (0.2, 0.4)}),
                                        ("SSLStaticDefenders-v0", {"m_ball": (0.04, 0.05), "e_rb": (0.2, 0.6)})])
def test_lookahead_with_per_env_physics(id_, ranges):
    import torch
    import rsoccer_amd
    env = rsoccer_amd.make_vec(id_, 37, device=0, seed=31, max_episode_steps=60, physics_ranges=ranges)
    env.reset()
    env.step_random(200)   # >= 3 auto-resets per env: the coefficients were redrawn and differ per env
    torch.cuda.synchronize()
    p = env.physics()["m_ball"].cpu().numpy()
    assert len(np.unique(p)) > 30
    acts = _actions(torch, env, 5, 12, 9)
    for gamma in (1.0, 0.97):
        got = _host(env.lookahead(acts, gamma=gamma, return_obs=True))
        _check(got, _reference(torch, env, acts, gamma), f"{id_} physics gamma {gamma}")
    env.close()


# ---- 7. large batch: stepping runs the one-lane-per-env layout, lookahead the lane groups ----
def test_large_batch_other_layout():
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(98304, device=0, seed=6)
    assert env.sim.task_layout() == "one-lane-per-env"
    env.reset()
    env.step_random(30)
    acts = _actions(torch, env, 2, 3, 13)
    got = _host(env.lookahead(acts, gamma=0.97, return_obs=True))
    _check(got, _reference(torch, env, acts, 0.97), "98304 envs")
    env.close()


# ---- 8. graph ----
def test_lookahead_then_step_replays_from_a_graph():
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
    acts = torch.zeros(B, K, H, AD, device=env.device)
    best = torch.zeros(B, AD, device=env.device)
    rows = torch.arange(B, device=env.device)

    def plan_and_act(e, a, b):
        out = e.lookahead(a, gamma=0.97)
        b.copy_(a[rows, out["return"].argmax(dim=1), 0])
        e.step(b)
        return out

    feeds = [_actions(torch, env, K, H, 100 + i) for i in range(8)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # torch's warm-up before a capture: real calls, the twin makes them too
        for i in range(2):
            acts.copy_(feeds[i])
            plan_and_act(env, acts, best)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    tbest = torch.zeros_like(best)
    for i in range(2):
        plan_and_act(twin, feeds[i], tbest)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = plan_and_act(env, acts, best)
    assert env.sim.task_tick() == twin.sim.task_tick() == 12   # capturing enqueued nothing
    for i in range(2, 7):
        acts.copy_(feeds[i])
        g.replay()
        want = plan_and_act(twin, feeds[i], tbest)
        torch.cuda.synchronize()
        for key in ("return", "steps", "terminated", "truncated"):
            assert torch.equal(out[key], want[key]), (i, key)
        assert torch.equal(best, tbest)
        for key in ("obs", "reward", "terminated", "truncated", "final_obs"):
            assert torch.equal(env._t[key], twin._t[key]), (i, key)
        assert torch.equal(env.state, twin.state)
    assert env.sim.task_tick() == twin.sim.task_tick() == 17
    assert np.array_equal(env.checkpoint(), twin.checkpoint())
    for e in envs:
        e.close()


def test_captured_lookahead_on_a_host_keyed_handle_is_refused():
    import torch
    from rsoccer_amd import _lib, vec
    env = vec.VecVSSEnv(64, device=0, seed=3)
    env.reset()
    env.step(None)
    torch.cuda.synchronize()
    before = env.checkpoint()
    acts = _actions(torch, env, 3, 4, 1)
    side = torch.cuda.Stream()
    with pytest.raises(_lib.RsxError, match="rsx_task_enable_capture"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
            env.lookahead(acts)
    torch.cuda.synchronize()
    _lib.drop_pending_hip_error()   # what the aborted capture leaves behind
    assert np.array_equal(env.checkpoint(), before)   # nothing ran
    env.step(None)                                    # the env still steps ...
    out = env.lookahead(acts)                         # ... and plans, eagerly
    torch.cuda.synchronize()
    assert env.sim.task_tick() == 2 and int(out["steps"].min()) == 4
    env.close()


# ---- 9. refusals ----
def test_refusals():
    import torch
    from rsoccer_amd import _lib, vec
    dev = torch.device("cuda", 0)
    sim = _lib.Sim(_lib.KIND_VSS, 0, 3, 3, 25, 16, 0)
    sim.task_attach(_lib.TASK_VSS_V0, 1, 0, 0)
    a = torch.zeros(16, 2, 3, 2, device=dev)
    r = torch.zeros(16, 2, device=dev)
    s = torch.zeros(16, 2, dtype=torch.int32, device=dev)
    f = torch.zeros(16, 2, dtype=torch.uint8, device=dev)
    call = lambda K=2, H=3, gamma=1.0, ap=a.data_ptr(), rp=r.data_ptr(): sim.task_lookahead(ap, K, H, gamma, rp, s.data_ptr(), f.data_ptr(), None, None)
    with pytest.raises(_lib.RsxError, match="reset"):
        call()
    sim.task_reset()
    call()
    for bad in (dict(K=0), dict(H=0), dict(gamma=float("nan")), dict(gamma=float("inf")), dict(ap=None), dict(rp=None)):
        with pytest.raises(_lib.RsxError):
            call(**bad)
    torch.cuda.synchronize()
    assert int(s.min()) == 3   # the valid call ran
    sim.close()

    env = vec.VecVSSEnv(16, device=0, seed=1)
    good = torch.zeros(16, 64, 3, 2, device=dev)
    with pytest.raises(_lib.RsxError, match="reset"):
        env.lookahead(good)
    env.reset()
    for shape in ((16, 2, 3), (15, 2, 3, 2), (16, 2, 3, 3), (16, 0, 3, 2), (16, 2, 0, 2), (2, 3, 2)):
        with pytest.raises(ValueError):
            env.lookahead(torch.zeros(*shape, device=dev))
    with pytest.raises(ValueError):
        env.lookahead(good, gamma=float("nan"))
    # numpy and float64 inputs are converted the way step() converts
    out64 = env.lookahead(np.zeros((16, 64, 3, 2)), return_obs=True)
    ref = env.lookahead(good, return_obs=True)
    for k in ref:
        assert torch.equal(out64[k], ref[k])
    # return_obs=False allocates no observation tensor
    del out64, ref
    torch.cuda.synchronize()
    obs_bytes = 16 * 64 * env.sim.obs_dim * 4
    m0 = torch.cuda.memory_allocated(dev)
    out = env.lookahead(good)
    grown = torch.cuda.memory_allocated(dev) - m0
    assert "last_obs" not in out and grown < obs_bytes // 2, grown
    with_obs = env.lookahead(good, return_obs=True)
    assert with_obs["last_obs"].shape == (16, 64, env.sim.obs_dim)
    # caller-owned results: the next call does not overwrite them
    keep = out["return"].clone()
    env.step(None)
    env.lookahead(torch.ones(16, 64, 3, 2, device=dev))
    torch.cuda.synchronize()
    assert torch.equal(out["return"], keep)
    env.close()
