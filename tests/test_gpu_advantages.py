"""VecFusedEnv.advantages / rsx_task_advantages: values of an MLP critic on a [T][B] batch and its GAE advantages.  The recurrence is
checked against the header's float32 formula in numpy on the call's own values, the critic's arithmetic against the engine's own
policy evaluation (collect()'s mean), against exactly representable selector critics and against the float32 forward bound.
Comparisons are on bit patterns unless a bound is derived next to them."""
import numpy as np
import pytest

import test_gpu_policy_lookahead as PL   # the selector family, the bit comparison, the measured tanh allowance

pytestmark = pytest.mark.gpu

_same, _bits, _dense, _make = PL._same, PL._bits, PL._dense, PL._make
U, TANH_DEV = PL.U, PL.TANH_DEV
GAMMA_LAM = ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0), (0.0, 0.5))
NONE, TERM, TRUNC, BOTH = 0, 1, 2, 3


def _critic(env, **kw):
    from rsoccer_amd.vec.policy import MLPCritic
    return MLPCritic(env.sim.obs_dim, **kw)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _batch(torch, dev, obs, rew, term, trunc, last, fin=None, flag_dtype=None):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    b = {"obs": t(obs), "reward": t(rew), "terminated": t(term), "truncated": t(trunc), "next_obs": t(last)}
    if flag_dtype is not None:
        b["terminated"], b["truncated"] = b["terminated"].to(flag_dtype), b["truncated"].to(flag_dtype)
    if fin is not None:
        b["final_obs"] = t(fin)
    return b


def _recurrence(value, nv, rew, end, gamma, lam):
    """include/rsx.h's float32 recurrence, every operation rounded on its own: advantages and returns from values and bootstrap values"""
    g = np.float32(gamma)
    gl = np.float32(np.float32(gamma) * np.float32(lam))
    T, B = value.shape
    adv, nxt = np.empty((T, B), np.float32), np.zeros(B, np.float32)
    for t in reversed(range(T)):
        delta = ((rew[t] + (g * nv[t]).astype(np.float32)).astype(np.float32) - value[t]).astype(np.float32)
        carried = (delta + (gl * nxt).astype(np.float32)).astype(np.float32)
        adv[t] = np.where(end[t], delta, carried)
        nxt = adv[t]
    return adv, (adv + value).astype(np.float32)


def _flags(rng, T, B, shift):
    """[T][B] kinds: random, with every combination forced into row 0, row T - 1 and an interior row (env e takes kind
    (e + shift) % 4 there), and env 0 ending in two successive rows (truncated only, then terminated) when T >= 4"""
    kind = rng.choice([NONE, NONE, NONE, NONE, NONE, TERM, TRUNC, TRUNC, BOTH], size=(T, B)).astype(np.int64)
    forced = sorted({0, T - 1} | ({T // 2} if 0 < T // 2 < T - 1 else set()))
    for t in forced:
        kind[t] = (np.arange(B) + shift + t) % 4
    if T >= 4:
        rows = [t for t in range(T - 1) if t not in forced and t + 1 not in forced]
        if rows:
            kind[rows[0], 0], kind[rows[0] + 1, 0] = TRUNC, TERM
    return kind, forced


@pytest.fixture(scope="module")
def handle():
    """a handle that is never reset and never stepped: the call needs only its device and obs_dim"""
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(9, device=0, seed=1)
    yield env
    env.close()


# ---- 1. the recurrence, exact, on synthetic batches ----
@pytest.mark.parametrize("T", [1, 2, 9, 33])
@pytest.mark.parametrize("B", [1, 67, 130])
def test_recurrence_is_the_headers_bit_for_bit(handle, B, T):
    import torch
    env, dev, OD = handle, handle.device, handle.sim.obs_dim
    critic = _critic(env)
    params = _dense(torch, critic, 1, seed=7)[0].to(dev)
    seen = set()
    for shift in (range(4) if B < 4 else (0,)):   # a lone env takes the four kinds in turn
        rng = np.random.default_rng(1000 * B + 10 * T + shift)
        kind, forced = _flags(rng, T, B, shift)
        term, trunc = (kind & 1).astype(bool), (kind & 2).astype(bool)
        end, only = term | trunc, trunc & ~term
        for t in forced:
            places = [p for p, hit in (("first", t == 0), ("last", t == T - 1), ("interior", 0 < t < T - 1)) if hit]
            seen |= {(p, int(k)) for p in places for k in kind[t]}
        obs = rng.uniform(-1.2, 1.2, (T, B, OD)).astype(np.float32)
        last = rng.uniform(-1.2, 1.2, (B, OD)).astype(np.float32)
        rew = rng.normal(0.0, 1.0, (T, B)).astype(np.float32)
        fin = np.full((T, B, OD), np.nan, np.float32)   # NaN wherever the call must not look
        fin[only] = rng.uniform(-1.2, 1.2, (int(only.sum()), OD)).astype(np.float32)
        batch = _batch(torch, dev, obs, rew, term, trunc, last, fin)
        # what the bootstrap values must be: the critic on final_obs (NaN rows blanked: they are not compared) and on last_obs
        blank = _batch(torch, dev, np.where(np.isnan(fin), np.float32(0), fin), rew, np.zeros_like(term), np.zeros_like(trunc), last)
        v_fin = env.advantages(blank, critic, params)["value"].cpu().numpy()
        one = _batch(torch, dev, last[None], rew[:1], np.zeros((1, B), bool), np.zeros((1, B), bool), last)
        v_last = env.advantages(one, critic, params)["value"].cpu().numpy()[0]
        for gamma, lam in GAMMA_LAM:
            for with_final in (True, False):
                b = dict(batch)
                if not with_final:
                    del b["final_obs"]
                out = _host(env.advantages(b, critic, params, gamma=gamma, lam=lam, return_next_values=True))
                tag = (B, T, shift, gamma, lam, with_final)
                v, nv = out["value"], out["next_value"]
                for k in ("value", "advantage", "return", "next_value"):
                    assert out[k].shape == (T, B) and out[k].dtype == np.float32 and np.all(np.isfinite(out[k])), (tag, k)
                adv, ret = _recurrence(v, nv, rew, end, gamma, lam)
                assert _same(out["advantage"], adv), (tag, "advantage")
                assert _same(out["return"], ret), (tag, "return")
                run = ~end
                assert _same(nv[:-1][run[:-1]], v[1:][run[:-1]]), (tag, "interior rows bootstrap from the next row's value")
                assert not _bits(nv[term]).any(), (tag, "terminated rows bootstrap from exactly 0")
                assert _same(nv[-1][run[-1]], v_last[run[-1]]), (tag, "the last row bootstraps from V(last_obs)")
                if with_final:
                    assert _same(nv[only], v_fin[only]), (tag, "truncated-only rows bootstrap from V(final_obs)")
                else:
                    assert not _bits(nv[only]).any(), (tag, "without final_obs truncated-only rows bootstrap from exactly 0")
                assert _same(v, env.advantages(b, critic, params)["value"].cpu().numpy()), (tag, "values do not depend on gamma / lam")
        if T >= 4:
            two = end[:-1, 0] & end[1:, 0]
            assert two.any(), "uninformative: no env ended in two successive rows"
    places = ("first", "last") + (("interior",) if T >= 3 else ())
    assert seen >= {(p, k) for p in places for k in (NONE, TERM, TRUNC, BOTH)}, sorted(seen)


def test_byte_flags_and_bool_flags_are_the_same_call(handle):
    import torch
    env, dev, OD = handle, handle.device, handle.sim.obs_dim
    critic = _critic(env, hidden=32, layers=1, hidden_act="relu")
    params = _dense(torch, critic, 1, seed=9)[0]
    rng = np.random.default_rng(4)
    T, B = 5, 70
    kind, _ = _flags(rng, T, B, 0)
    args = (rng.uniform(-1, 1, (T, B, OD)).astype(np.float32), rng.normal(0, 1, (T, B)).astype(np.float32), (kind & 1).astype(bool),
            (kind & 2).astype(bool), rng.uniform(-1, 1, (B, OD)).astype(np.float32), rng.uniform(-1, 1, (T, B, OD)).astype(np.float32))
    a = _host(env.advantages(_batch(torch, dev, *args), critic, params, return_next_values=True))
    u8 = _batch(torch, dev, *args, flag_dtype=torch.uint8)
    u8["terminated"], u8["truncated"] = u8["terminated"] * 255, u8["truncated"] * 7   # non-zero = true
    b = _host(env.advantages(u8, critic, params.numpy().astype(np.float64), return_next_values=True))   # (host parameters are converted)
    for k in a:
        assert _same(a[k], b[k]), k


# ---- 2. the critic's arithmetic is the engine's: a critic that shares the actor's hidden layers and output row 0 ----
def _shared(torch, pol, critic, seed=5):
    """dense actor parameters and the critic cut out of them"""
    params = _dense(torch, pol, 1, seed=seed)[0]
    ts = pol.unpack(params)
    return params, critic.pack(ts[:-2] + [ts[-2][:1], ts[-1][:1]])


@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("layers,hidden", [(1, 32), (1, 64), (2, 32), (2, 64)])
@pytest.mark.parametrize("name", ["VecVSSEnv", "VecSSLDribblingEnv", "VecSSLContestedPossessionEnv"])   # obs_dim 40, 21, 14
def test_values_equal_the_collectors_mean(name, layers, hidden, act, monkeypatch):
    import torch
    from rsoccer_amd import vec
    from rsoccer_amd.vec.policy import MLPPolicy
    env = _make(vec, name, 9, device=0, seed=2025, max_episode_steps=5)
    assert env.sim.obs_dim == {"VecVSSEnv": 40, "VecSSLDribblingEnv": 21, "VecSSLContestedPossessionEnv": 14}[name]
    PL._start(torch, env)
    pol = MLPPolicy(env.sim.obs_dim, env.sim.act_dim, hidden=hidden, layers=layers, hidden_act=act, out_act="clip")
    critic = _critic(env, hidden=hidden, layers=layers, hidden_act=act)
    params, cparams = _shared(torch, pol, critic)
    batch = env.collect(pol, params, 7, log_std=-1.0, noise_seed=3, return_final_obs=True)
    out = env.advantages(batch, critic, cparams)
    mean0 = batch["mean"][..., 0].cpu().numpy()
    assert _same(out["value"].cpu().numpy(), mean0), _where(out["value"].cpu().numpy(), mean0)
    monkeypatch.setenv("RSX_GAE_FORM", "groups")   # eight lanes per row, the collector's own evaluation: the same bits
    again = env.advantages(batch, critic, cparams)
    for k in out:
        assert _same(out[k].cpu().numpy(), again[k].cpu().numpy()), ("groups", k)
    env.close()


@pytest.mark.parametrize("layers,hidden", [(1, 32), (2, 64)])
def test_values_equal_the_collectors_mean_at_64_floats(layers, hidden, monkeypatch):
    """VSS 5v5: obs_dim 64, where two hidden layers of 64 leave room for one wave per workgroup only (another launch shape)"""
    import torch
    from rsoccer_amd import vec
    from rsoccer_amd.vec.policy import MLPPolicy
    env = _make(vec, "VecVSS5v5", 9, device=0, seed=4, max_episode_steps=5)
    assert env.sim.obs_dim == 64
    PL._start(torch, env)
    pol = MLPPolicy(64, env.sim.act_dim, hidden=hidden, layers=layers, hidden_act="tanh", out_act="tanh")
    critic = _critic(env, hidden=hidden, layers=layers)
    params, cparams = _shared(torch, pol, critic, seed=8)
    batch = env.collect(pol, params, 7, log_std=-1.0, noise_seed=3, return_final_obs=True)
    out = env.advantages(batch, critic, cparams, return_next_values=True)
    assert _same(out["value"].cpu().numpy(), batch["mean"][..., 0].cpu().numpy())
    only = (batch["truncated"] & ~batch["terminated"]).cpu().numpy()
    v_fin = env.advantages({**batch, "obs": batch["final_obs"]}, critic, cparams)["value"].cpu().numpy()
    assert only.any() and _same(out["next_value"].cpu().numpy()[only], v_fin[only])
    monkeypatch.setenv("RSX_GAE_FORM", "groups")
    again = env.advantages(batch, critic, cparams, return_next_values=True)
    for k in out:
        assert _same(out[k].cpu().numpy(), again[k].cpu().numpy()), ("groups", k)
    env.close()


def _where(a, b):
    d = _bits(a) != _bits(b)
    return f"{int(d.sum())} of {d.size} differ, first at {np.argwhere(d)[:3].tolist()}: {a[d][:3].tolist()} / {b[d][:3].tolist()}"


# ---- 3. selector critics: every fmaf is exact ----
@pytest.mark.parametrize("layers,hidden", [(1, 32), (1, 64), (2, 32), (2, 64)])
def test_selector_critics_are_evaluated_exactly(layers, hidden):
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(9, device=0, seed=11, max_episode_steps=5)
    PL._start(torch, env)
    pol = PL._policy(env)
    batch = env.collect(pol, _dense(torch, pol, 1)[0], 8)
    critic = _critic(env, hidden=hidden, layers=layers, hidden_act="relu")
    for k in range(3):
        params = PL._selector(torch, critic, k)
        got = env.advantages(batch, critic, params)["value"].cpu().numpy()
        want = critic.forward(batch["obs"].cpu(), params, dtype=torch.float32).numpy()[..., 0]   # on the host: every operation is exact
        assert _same(got, want), (k, _where(got, want))
        assert got.any()
    env.close()


# ---- 4. dense critics: the float32 forward bound ----
def _forward_with_bound(torch, critic, obs, params):
    """test_gpu_policy_lookahead._forward_with_bound for a linear output (identity: no further term): the float64 value and, per row,
    what sequential float32 fmaf accumulation may deviate from it — per unit (n + 1) u (|b| + sum |w_i x_i|), the error inherited from
    the layer below through |w|, and 4 TANH_DEV per tanh"""
    ts = [t.double() for t in critic.unpack(params)]
    x, delta = obs.double(), torch.zeros_like(obs, dtype=torch.float64)
    n_layers = len(ts) // 2
    for li in range(n_layers):
        w, b = ts[2 * li], ts[2 * li + 1]
        n = w.shape[1]
        pre = x @ w.T + b
        mag = (x.abs() + delta) @ w.abs().T + b.abs()
        delta = delta @ w.abs().T + (n + 1) * U * mag
        if li + 1 == n_layers:
            x = pre
        elif critic.hidden_act == "tanh":
            x, delta = torch.tanh(pre), delta + 4 * TANH_DEV
        else:
            x = torch.relu(pre)
    return x, delta


@pytest.mark.parametrize("name", PL.CLASSES)
def test_dense_critics_are_within_the_float32_bound(name):
    import torch
    from rsoccer_amd import vec
    env = _make(vec, name, 9, device=0, seed=2025, max_episode_steps=5)
    PL._start(torch, env)
    pol = PL._policy(env)
    batch = env.collect(pol, _dense(torch, pol, 1)[0], 8)
    critic = _critic(env)
    params = _dense(torch, critic, 1, seed=21)[0]
    got = env.advantages(batch, critic, params)["value"].cpu().double().reshape(-1, 1)
    obs = batch["obs"].cpu().reshape(-1, critic.obs_dim)
    want, bound = _forward_with_bound(torch, critic, obs, params)
    assert torch.allclose(want, critic.forward(obs, params), rtol=0, atol=1e-12)
    err = (got - want).abs().numpy()
    print(name, "largest error", err.max(), "smallest bound", float(bound.min()), "worst error / bound", (err / bound.numpy()).max())
    assert np.all(err <= bound.numpy())
    env.close()


# ---- 5. a real batch with episode ends: collect(critic=...) is collect() + advantages() ----
@pytest.mark.parametrize("name", ["VecVSSEnv", "VecSSLPassEnduranceEnv"])
def test_collect_with_a_critic_is_collect_then_advantages(name):
    import torch
    from rsoccer_amd import vec
    T, B = 12, 24
    envs = [_make(vec, name, B, device=0, seed=2025, max_episode_steps=5) for _ in range(2)]
    for e in envs:
        PL._start(torch, e)
    env, twin = envs
    pol, critic = PL._policy(env), _critic(env)
    params, cparams = _dense(torch, pol, 1)[0], _dense(torch, critic, 1, seed=33)[0]
    plain = env.collect(pol, params, T, log_std=-1.0, noise_seed=5, return_final_obs=True)
    adv = env.advantages(plain, critic, cparams, gamma=0.97, lam=0.9)
    both = twin.collect(pol, params, T, log_std=-1.0, noise_seed=5, critic=critic, critic_params=cparams, gamma=0.97, lam=0.9)
    torch.cuda.synchronize()
    term, trunc = plain["terminated"].cpu().numpy(), plain["truncated"].cpu().numpy()
    print(name, "terminated rows", int(term.sum()), "truncated-only rows", int((trunc & ~term).sum()))
    assert (trunc & ~term).any(), "uninformative: no row was truncated only"
    if name == "VecSSLPassEnduranceEnv":
        assert term.any(), "uninformative: no row terminated (the seed is chosen so that one does)"
    assert set(both) == set(plain) | {"value", "advantage", "return"}
    for k in plain:
        assert _same(both[k].cpu().numpy(), plain[k].cpu().numpy()), k
    for k in ("value", "advantage", "return"):
        assert _same(both[k].cpu().numpy(), adv[k].cpu().numpy()), k
        assert np.all(np.isfinite(adv[k].cpu().numpy())), k
    assert np.array_equal(env.checkpoint(), twin.checkpoint())   # the critic touches nothing of the env
    # a truncated-only row bootstraps from the terminal observation and not from the next episode's first one
    full = _host(env.advantages(plain, critic, cparams, gamma=0.97, lam=0.9, return_next_values=True))
    v_fin = env.advantages({**plain, "obs": plain["final_obs"]}, critic, cparams)["value"].cpu().numpy()
    only = trunc & ~term
    assert _same(full["next_value"][only], v_fin[only]) and not _bits(full["next_value"][term]).any()
    # without a critic the call returns what it returned before
    assert set(env.collect(pol, params, 2)) == {"obs", "actions", "reward", "terminated", "truncated", "next_obs"}
    assert set(env.collect(pol, params, 2, log_std=0.0, return_final_obs=True)) == \
        {"obs", "actions", "reward", "terminated", "truncated", "next_obs", "final_obs", "mean", "sample", "log_prob"}
    for e in envs:
        e.close()


# ---- 6. capture ----
def test_collect_and_advantages_replay_from_a_graph():
    import torch
    from rsoccer_amd import vec
    T, B = 6, 9
    env = vec.VecVSSEnv(B, device=0, seed=17, max_episode_steps=5)
    PL._start(torch, env)
    env.enable_graph_capture()
    pol, critic = PL._policy(env), _critic(env)
    params = _dense(torch, pol, 1)[0].to(env.device)
    cparams = _dense(torch, critic, 1, seed=33)[0].to(env.device)
    log_std = torch.full((env.sim.act_dim,), -1.0, device=env.device)

    def run():
        batch = env.collect(pol, params, T, log_std=log_std, noise_seed=99, return_final_obs=True)
        return batch, env.advantages(batch, critic, cparams, return_next_values=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # the eager call, which is also torch's warm-up before a capture
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        batch, out = run()
    seen = []
    for i in range(2):
        g.replay()
        torch.cuda.synchronize()
        rec = {k: v.clone() for k, v in batch.items()}
        got = {k: v.clone() for k, v in out.items()}
        want = env.advantages(rec, critic, cparams, return_next_values=True)   # eager, on this replay's recorded batch
        for k in want:
            assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (i, k)
        assert rec["truncated"].any()
        seen.append(got["value"])
    assert not torch.equal(seen[0], seen[1]), "the replays saw the same batch"
    assert env.sim.task_tick() == PL.WARM + 3 * T
    env.close()


# ---- 7. refusals ----
def test_refusals_enqueue_nothing():
    import torch
    from rsoccer_amd import _lib, vec
    env = vec.VecVSSEnv(9, device=0, seed=1, max_episode_steps=5)
    dev, OD = env.device, env.sim.obs_dim
    critic = _critic(env)
    params = _dense(torch, critic, 1)[0].to(dev)
    T, B = 3, 5
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)   # noqa: E731
    inp = {"obs": z(T, B, OD), "rewards": z(T, B), "terminated": z(T, B, dt=torch.uint8), "truncated": z(T, B, dt=torch.uint8),
           "final_obs": z(T, B, OD), "last_obs": z(B, OD)}
    out = {k: torch.full((T, B), 7.0, device=dev) for k in ("values", "advantages", "returns", "next_values")}

    def raw(sim=env.sim, spec="default", p="default", gamma=0.99, lam=0.95, T_=T, B_=B, skip=(), no_in=False, no_out=False):
        i = _lib.AdvIn(*[None if k in skip else inp[k].data_ptr() for k in ("obs", "rewards", "terminated", "truncated", "final_obs", "last_obs")])
        o = _lib.AdvOut(*[None if k in skip else out[k].data_ptr() for k in ("values", "advantages", "returns", "next_values")])
        sim.task_advantages(critic.spec() if spec == "default" else spec, params.data_ptr() if p == "default" else p, gamma, lam, T_, B_,
                            None if no_in else i, None if no_out else o, env._stream())

    ok = _lib.PolicyMLP(2, 64, _lib.ACT_TANH, _lib.ACT_NONE)
    assert env.sim.critic_num_params(ok) == critic.num_params
    bad = [dict(skip=(k,)) for k in ("obs", "rewards", "terminated", "truncated", "last_obs", "values", "advantages", "returns")]
    bad += [dict(no_in=True), dict(no_out=True), dict(p=None), dict(spec=None), dict(T_=0), dict(T_=-3), dict(B_=0), dict(B_=-1)]
    bad += [dict(gamma=v) for v in (float("nan"), float("inf"), -0.01, 1.01)] + [dict(lam=v) for v in (float("nan"), -float("inf"), -0.5, 2.0)]
    bad += [dict(spec=_lib.PolicyMLP(2, 48, _lib.ACT_TANH, _lib.ACT_NONE)), dict(spec=_lib.PolicyMLP(3, 64, _lib.ACT_TANH, _lib.ACT_NONE)),
            dict(spec=_lib.PolicyMLP(0, 64, _lib.ACT_TANH, _lib.ACT_NONE)), dict(spec=_lib.PolicyMLP(2, 64, 7, _lib.ACT_NONE)),
            dict(spec=_lib.PolicyMLP(2, 64, _lib.ACT_CLIP, _lib.ACT_NONE))]
    bad += [dict(spec=_lib.PolicyMLP(2, 64, _lib.ACT_TANH, a)) for a in (_lib.ACT_TANH, _lib.ACT_CLIP, _lib.ACT_RELU, 4)]
    for kw in bad:
        with pytest.raises(_lib.RsxError):
            raw(**kw)
    bare = _lib.Sim(_lib.KIND_VSS, 0, 3, 3, 25, 9, 0)   # a handle without a task
    with pytest.raises(_lib.RsxError, match="task"):
        raw(sim=bare)
    with pytest.raises(_lib.RsxError):
        bare.critic_num_params(ok)
    bare.close()
    torch.cuda.synchronize()
    for k, v in out.items():
        assert (v == 7.0).all(), f"a refused call wrote {k}"
    raw(skip=("final_obs", "next_values"))   # the optional arrays may be NULL
    torch.cuda.synchronize()
    assert (out["next_values"] == 7.0).all() and not (out["values"] == 7.0).any() and not (out["returns"] == 7.0).any()

    # every existing call that takes an rsx_policy_mlp still refuses the linear output
    PL._start(torch, env)
    pol = PL._policy(env)
    pp = _dense(torch, pol, 1).to(dev)
    lin = _lib.PolicyMLP(2, 64, _lib.ACT_TANH, _lib.ACT_NONE)
    before, tick = env.checkpoint(), env.sim.task_tick()
    r, s, f = z(9, 1), z(9, 1, dt=torch.int32), z(9, 1, dt=torch.uint8)
    with pytest.raises(_lib.RsxError, match="out_act"):
        env.sim.task_lookahead_policy(lin, pp.data_ptr(), 1, 2, 1.0, r.data_ptr(), s.data_ptr(), f.data_ptr(), None, None, None, env._stream())
    rec = _lib.CollectOut(z(2, 9, OD).data_ptr(), z(2, 9, env.sim.act_dim).data_ptr(), z(2, 9).data_ptr(), z(2, 9, dt=torch.uint8).data_ptr())
    with pytest.raises(_lib.RsxError, match="out_act"):
        env.sim.task_collect_policy(lin, pp.data_ptr(), None, 0, 2, rec, env._stream())
    with pytest.raises(_lib.RsxError, match="out_act"):
        env.sim.policy_num_params(lin)
    assert np.array_equal(env.checkpoint(), before) and env.sim.task_tick() == tick

    # the Python layer names the offender
    good = {"obs": inp["obs"], "reward": inp["rewards"], "terminated": inp["terminated"], "truncated": inp["truncated"], "next_obs": inp["last_obs"]}
    for key, value in (("obs", z(T, B, OD + 1)), ("reward", z(T, B + 1)), ("reward", z(T, B, dt=torch.float64)), ("terminated", z(T, B)),
                       ("truncated", z(B, T, dt=torch.uint8)), ("next_obs", z(B + 1, OD)), ("final_obs", z(T, B, OD - 1)),
                       ("reward", torch.zeros(T, B)), ("obs", z(T, B, 2 * OD)[..., ::2]), ("next_obs", np.zeros((B, OD), np.float32))):
        with pytest.raises(ValueError, match=key):
            env.advantages({**good, key: value}, critic, params)
    with pytest.raises(ValueError, match="next_obs"):
        env.advantages({k: v for k, v in good.items() if k != "next_obs"}, critic, params)
    for kw in (dict(gamma=1.5), dict(lam=-0.1), dict(gamma=float("nan"))):
        with pytest.raises(ValueError):
            env.advantages(good, critic, params, **kw)
    with pytest.raises(ValueError):
        env.advantages(good, pol, params)
    with pytest.raises(ValueError):
        env.advantages(good, critic, params[:-1])
    with pytest.raises(ValueError):
        env.advantages(good, type(critic)(OD + 1), torch.zeros(type(critic)(OD + 1).num_params))   # a critic for another obs_dim
    with pytest.raises(ValueError):
        env.collect(pol, pp[0], 2, critic_params=params)
    with pytest.raises(ValueError):
        env.collect(pol, pp[0], 2, critic=critic, critic_params=None)
    assert env.sim.task_tick() == tick
    env.close()
