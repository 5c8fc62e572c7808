"""VecFusedEnv.dpg_gradient / rsx_task_dpg_gradient: gradients of the TD3 / DDPG losses of include/rsx.h with respect to an MLP actor and
its one or two Q critics.  The gradients and stats are checked against float64 autograd with torch's own float32 autograd as the
yardstick (tests/dpg_helpers.py), the smoothing noise against a host restatement, the forward pass against collect()'s own actions bit
for bit; then the delayed actor, determinism, capture, out-of-range rows and refusals."""
import numpy as np
import pytest

import dpg_helpers as DH
import test_gpu_policy_lookahead as PL   # the env factory, the bit comparison

pytestmark = pytest.mark.gpu

_same, _make = PL._same, PL._make
DOM_DPG = 10
SEED64 = 0x0123456789ABCDEF   # (distinct halves: the key is (lo, hi))
STEP = 3


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
    return {k: data[k].to(dev).contiguous() for k in DH.ROW_KEYS}


def _call(env, pol, critic, data, rows, sigma=0.2, wg=None, rows_of=None, **kw):
    dev = env.device
    args = dict(rows=None if rows is None else rows.to(dev), gamma=DH.GAMMA, target_noise=sigma, noise_clip=DH.NOISE_CLIP, noise_seed=SEED64,
                noise_step=STEP, max_workgroups=wg, return_rows=True)
    args.update(kw)
    return env.dpg_gradient(_rows_of(data, dev) if rows_of is None else rows_of, pol, data["params"].to(dev), data["tparams"].to(dev), critic,
                            data["cparams"].to(dev), data["tcparams"].to(dev), **args)


def _kernel(pol, critic, got):
    out = {f"actor.{i}": t for i, t in enumerate(pol.unpack(got["grad_params"].cpu().double()))}
    for c in range(got["grad_critic_params"].shape[0]):
        out.update({f"critic{c}.{i}": t for i, t in enumerate(critic.unpack(got["grad_critic_params"][c].cpu().double()))})
    out.update({k: got["stats"][k].cpu().double() for k in DH.FLOAT_STATS})
    return out


def _rel(x, ref):
    scale = float(ref.abs().max())
    err = float((x - ref).abs().max())
    if scale == 0.0:
        assert err == 0.0, "the reference is exactly zero, the result is not"
        return 0.0
    return err / scale


def _flat(torch, out):
    keys = [k for k in ("grad_params", "grad_critic_params", "target", "q", "action", "target_noise") if k in out]
    return torch.cat([out[k].reshape(-1) for k in keys] + [torch.stack(list(out["stats"].values()))]).clone().view(torch.int32)


# ---- 1. gradients and stats against float64 autograd, torch's float32 autograd as the yardstick ----
@pytest.mark.parametrize("case", DH.CASES, ids=["-".join(str(v) for v in c) for c in DH.CASES])
def test_gradients_and_stats_stay_within_4x_of_torchs_float32_error(handles, case):
    """Criterion (tests/test_gpu_ppo_grad.py's, unchanged): for every parameter tensor and every float stat, the kernel's relative error
    against float64 autograd is at most 4x the LARGEST relative error any tensor of torch's float32 autograd on the device shows in
    the same case.  The yardstick is fed the call's own target_noise (pinned by the test below)."""
    import torch
    (od, ad), hidden, layers, act, out_act, C, M, mode, wg, sigma = case
    env = handles(DH.ENVS[(od, ad)])
    assert (env.sim.obs_dim, env.sim.act_dim) == (od, ad)
    pol, critic, data, removed, n0 = DH.case_data(torch, case)
    assert removed <= 0.02 * n0, f"the kink filter removed {removed} of {n0} rows"
    assert data["obs"].shape[0] >= M
    if mode == "none":   # rows=None is the whole batch: the batch has M rows
        for k in DH.ROW_KEYS:
            data[k] = data[k][:M].contiguous()
    n = data["obs"].shape[0]
    rows = DH.make_rows(torch, mode, M, n, DH.case_seed(case))
    idx = torch.arange(M) if rows is None else rows.long()
    got = _call(env, pol, critic, data, rows, sigma=sigma, wg=wg)
    torch.cuda.synchronize()
    assert int(got["stats"]["rows_used"]) == M and int(got["stats"]["rows_skipped"]) == 0
    noise = got["target_noise"].cpu() if sigma > 0.0 else None
    if noise is None:
        assert not got["target_noise"].any()
    ref = DH.autograd(torch, pol, critic, data, idx, noise, DH.GAMMA, torch.float64, "cpu")
    yard = DH.autograd(torch, pol, critic, data, idx, noise, DH.GAMMA, torch.float32, env.device)
    ker = _kernel(pol, critic, got)
    assert set(ref) <= set(ker) and len(ref) == 2 * (layers + 1) * (1 + C) + 2 * C + 3
    e_yard = {k: _rel(yard[k], ref[k]) for k in ref}
    e_ker = {k: _rel(ker[k], ref[k]) for k in ref}
    pooled = max(e_yard.values())
    worst = max(e_ker, key=e_ker.get)
    print(f"{case}: removed {removed}, torch f32 pooled {pooled:.3e}, kernel worst {e_ker[worst]:.3e} ({worst}), "
          f"ratio {e_ker[worst] / pooled:.2f}")
    assert pooled > 0.0
    for k in ref:
        assert e_ker[k] <= 4.0 * pooled, (k, e_ker[k], pooled, e_ker[k] / pooled)


# ---- 2. the smoothing noise ----
def _normal_pair(w0, w1):
    u1 = ((w0 >> 8) + 1) * 2.0 ** -24
    ang = ((w1 >> 8) * 2.0 ** -24 - 0.5) * 2.0 * np.pi
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(ang), rad * np.sin(ang)


def _noise_host(O, seed64, step, M, AD, sigma, clip):
    """the header's recipe: eps in float64 from the oracle's Philox (7 rounds), then sigma * eps and the clamp in float32"""
    key = (seed64 & 0xFFFFFFFF, seed64 >> 32)
    eps = np.zeros((M, AD))
    for t in range(M):
        for q in range((AD + 3) // 4):
            w = O.philox((t, step >> 32, step & 0xFFFFFFFF, DOM_DPG | (q << 8)), key, rounds=7)
            nn = _normal_pair(w[0], w[1]) + _normal_pair(w[2], w[3])
            for c in range(min(4, AD - 4 * q)):
                eps[t, 4 * q + c] = nn[c]
    f = np.float32
    return np.clip(f(sigma) * eps.astype(f), -f(clip), f(clip)).astype(f), eps


@pytest.mark.parametrize("od_ad", [(40, 2), (14, 5)])   # one noise block and two
def test_the_smoothing_noise(handles, oracle_mod, od_ad):
    import torch
    env = handles(DH.ENVS[od_ad])
    dev, AD = env.device, od_ad[1]
    case = (od_ad, 32, 1, "tanh", "tanh", 2, 150, "perm", None, 0.2)
    pol, critic, data, _, _ = DH.case_data(torch, case)
    M, n = 150, data["obs"].shape[0]
    rows = DH.make_rows(torch, "perm", M, n, 1)
    got = _call(env, pol, critic, data, rows)
    torch.cuda.synchronize()
    noise = got["target_noise"].cpu().numpy()
    want, eps = _noise_host(oracle_mod, SEED64, STEP, M, AD, 0.2, DH.NOISE_CLIP)
    bound = 1e-5 * max(0.2, 1.0)   # (test_the_gaussian_head's bound for the collector's head)
    err = np.abs(noise.astype(np.float64) - want.astype(np.float64))
    bind = float((np.abs(want) == np.float32(DH.NOISE_CLIP)).mean())
    print(f"{od_ad}: max |device noise - restatement| {err.max():.3e} (bound {bound:.1e}); eps std {eps.std():.3f}; the clamp binds on {bind:.2f}")
    assert err.max() <= bound and np.abs(noise).max() <= np.float32(DH.NOISE_CLIP)
    assert 0.7 < eps.std() < 1.3 and 0.3 < bind < 0.9
    # a function of the position alone: not of the grid, not of the rows' contents
    other_rows = DH.make_rows(torch, "repeats", M, n, 2)
    for kw in (dict(wg=1), dict(rows=other_rows.to(torch.int32)), dict(wg=2, rows=None, rows_of={k: v[:M].contiguous() for k, v in _rows_of(data, dev).items()})):
        again = _call(env, pol, critic, data, kw.pop("rows", rows), **kw)
        assert _same(again["target_noise"].cpu().numpy(), noise), kw
    # another step or another seed: other noise; the step's high word is a counter word of its own
    for kw in (dict(noise_step=STEP + 1), dict(noise_seed=SEED64 + 1), dict(noise_step=STEP + 2 ** 32)):
        assert not _same(_call(env, pol, critic, data, rows, **kw)["target_noise"].cpu().numpy(), noise), kw
    far = _call(env, pol, critic, data, rows, noise_step=STEP + 2 ** 32)["target_noise"].cpu().numpy()
    assert np.abs(far.astype(np.float64) - _noise_host(oracle_mod, SEED64, STEP + 2 ** 32, M, AD, 0.2, DH.NOISE_CLIP)[0]).max() <= bound
    # sigma = 0: no noise, and a' is the target actor's answer
    ddpg = _call(env, pol, critic, data, rows, sigma=0.0)
    assert not ddpg["target_noise"].any()
    # the step as a device tensor, advanced between two replays of one captured call
    static = _rows_of(data, dev)
    r, step = rows.to(dev), torch.tensor([STEP], dtype=torch.int64, device=dev)
    eager = [_flat(torch, _call(env, pol, critic, data, r, rows_of=static, noise_step=STEP + i)) for i in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # torch's warm-up before a capture
        _call(env, pol, critic, data, r, rows_of=static, noise_step=step)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    p = {k: data[k].to(dev) for k in ("params", "tparams", "cparams", "tcparams")}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = env.dpg_gradient(static, pol, p["params"], p["tparams"], critic, p["cparams"], p["tcparams"], rows=r, gamma=DH.GAMMA,
                               target_noise=0.2, noise_clip=DH.NOISE_CLIP, noise_seed=SEED64, noise_step=step, return_rows=True)
    seen = []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        seen.append(_flat(torch, out))
        step += 1
    assert torch.equal(seen[0], eager[0]) and torch.equal(seen[1], eager[1]) and not torch.equal(seen[0], seen[1])


# ---- 3. the forward pass on a real batch ----
def test_forward_bits_on_a_real_batch():
    import torch
    from rsoccer_amd import vec
    from rsoccer_amd.vec.policy import MLPPolicy, MLPQCritic
    from rsoccer_amd.vec.replay import ReplayBuffer
    T, B = 8, 64
    env = _make(vec, "VecVSSEnv", B, device=0, seed=2025, max_episode_steps=5)
    PL._start(torch, env)
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    pol, critic = MLPPolicy(OD, AD, hidden=64, layers=2), MLPQCritic(OD, AD, hidden=64, layers=2)
    gen = torch.Generator().manual_seed(3)
    params = DH.init(torch, pol, gen).to(dev)
    cparams = torch.stack([DH.init(torch, critic, gen) for _ in range(2)]).to(dev)
    batch = env.collect(pol, params, T, log_std=None, return_final_obs=True)
    buf = ReplayBuffer(T * B, OD, AD, dev)
    buf.add(batch)
    data = buf.data()
    before = env.checkpoint()
    out = env.dpg_gradient(data, pol, params, params, critic, cparams, cparams, gamma=0.99, return_rows=True)
    torch.cuda.synchronize()
    assert int(out["stats"]["rows_used"]) == T * B
    # the same policy, the same arithmetic
    assert _same(out["action"].cpu().numpy(), batch["actions"].reshape(T * B, AD).cpu().numpy())
    ended = (batch["terminated"] | batch["truncated"]).reshape(-1)
    assert 0 < int(ended.sum()) < T * B
    assert torch.equal(data["next_obs"][ended], batch["final_obs"].reshape(T * B, OD)[ended])
    assert torch.equal(data["next_obs"][:(T - 1) * B][~ended[:(T - 1) * B]], batch["obs"][1:].reshape(-1, OD)[~ended[:(T - 1) * B]])
    term = data["terminated"]
    assert _same(out["target"][term].cpu().numpy(), data["reward"][term].cpu().numpy())
    assert not bool((out["target"][~term] == data["reward"][~term]).all())
    # every row terminated (also rewards of -0.0): the target is the reward in bits
    forced = dict(data, terminated=torch.ones_like(term), reward=torch.where(torch.arange(T * B, device=dev) % 7 == 0, -0.0, 1.0) * data["reward"])
    all_term = env.dpg_gradient(forced, pol, params, params, critic, cparams, cparams, gamma=0.99, return_rows=True)
    assert _same(all_term["target"].cpu().numpy(), forced["reward"].cpu().numpy())
    assert np.array_equal(env.checkpoint(), before)   # no side effects
    env.close()


def _medium(torch, od_ad=(40, 2), act="tanh", out_act="tanh", C=2, M=700):
    case = (od_ad, 64, 2, act, out_act, C, M, "repeats", None, 0.2)
    pol, critic, data, _, _ = DH.case_data(torch, case)
    return pol, critic, data, DH.make_rows(torch, "repeats", M, data["obs"].shape[0], 5).to(torch.int32)


# ---- 4. the delayed actor ----
def test_without_the_actor_everything_else_keeps_its_bits(handles):
    import torch
    env = handles("VecVSSEnv")
    pol, critic, data, rows = _medium(torch)
    full = _call(env, pol, critic, data, rows, wg=3)
    crit = _call(env, pol, critic, data, rows, wg=3, actor=False)
    torch.cuda.synchronize()
    assert "grad_params" not in crit and "action" not in crit and "loss_pi" not in crit["stats"]
    assert "grad_params" in full and float(full["stats"]["loss_pi"]) != 0.0
    for k in ("grad_critic_params", "target", "q", "target_noise"):
        assert _same(full[k].cpu().numpy(), crit[k].cpu().numpy()), k
    for k in crit["stats"]:
        assert _same(full["stats"][k].cpu().numpy(), crit["stats"][k].cpu().numpy()), k


# ---- 5. determinism, eagerly and from a graph ----
def test_two_calls_and_a_replayed_graph_return_the_same_bits(handles):
    import torch
    env = handles("VecVSSEnv")
    dev = env.device
    pol, critic, data, _ = _medium(torch, act="relu", out_act="clip")
    _, _, other, _ = _medium(torch, act="relu", out_act="clip", M=701)
    n = min(data["obs"].shape[0], other["obs"].shape[0])
    rows = DH.make_rows(torch, "repeats", 700, n, 5).to(torch.int32)
    static = {k: v[:n].contiguous() for k, v in _rows_of(data, dev).items()}
    p = {k: data[k].to(dev) for k in ("params", "tparams", "cparams", "tcparams")}
    r = rows.to(dev)

    def run():
        return env.dpg_gradient(static, pol, p["params"], p["tparams"], critic, p["cparams"], p["tcparams"], rows=r, gamma=DH.GAMMA,
                                target_noise=0.2, noise_clip=DH.NOISE_CLIP, noise_seed=7, noise_step=1, return_rows=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # eager calls, which are also torch's warm-up before a capture
        a, b = _flat(torch, run()), _flat(torch, run())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run()
    for k in static:   # the inputs overwritten in place
        static[k].copy_(other[k][:n].to(dev))
    for k in p:
        p[k].copy_(other[k].to(dev))
    seen = []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        seen.append(_flat(torch, out))
    want = _flat(torch, run())
    torch.cuda.synchronize()
    assert torch.equal(seen[0], want) and torch.equal(seen[1], want) and not torch.equal(want, a)


# ---- 6. out-of-range and padding rows ----
def test_out_of_range_rows_contribute_nothing_and_nothing_outside_is_read(handles):
    """tests/test_gpu_ppo_grad.py's scheme: 41 of the M entries are out of range; the call with every one of them a plain -1 has the
    same bits, and the gradients are those of float64 autograd over the valid entries with the divisor M.  Every input array is a view
    into the middle of an allocation filled with NaN (the flags: with ones), and the fill is still there afterwards."""
    import torch
    env = handles("VecSSLDribblingEnv")
    dev = env.device
    case = ((21, 4), 64, 2, "relu", "clip", 2, 400, "repeats", None, 0.2)
    pol, critic, data, _, _ = DH.case_data(torch, case)
    M, BAD = 300, 41
    n = data["obs"].shape[0]
    gen = torch.Generator().manual_seed(9)
    rows = torch.randint(0, n, (M,), generator=gen).to(torch.int32)
    bad_at = torch.cat([torch.randperm(M - 10, generator=gen)[:BAD - 10], torch.arange(M - 10, M)])
    bad_values = torch.tensor([-1, -7, n, n + 1, n + 100, 2 ** 31 - 1, -2 ** 31, -n], dtype=torch.int64)
    with_bad = rows.clone()
    with_bad[bad_at] = bad_values[torch.arange(BAD) % len(bad_values)].to(torch.int32)
    padded = rows.clone()
    padded[bad_at] = -1
    valid = torch.ones(M, dtype=torch.bool)
    valid[bad_at] = False
    PAD, guards = 1000, []

    def guarded(t):
        t = t.to(dev)
        fill = float("nan") if t.dtype == torch.float32 else 1
        big = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype, device=dev)
        view = big[PAD:PAD + t.numel()].view(t.shape)
        view.copy_(t)
        guards.append((big, t.numel()))
        return view

    rows_of = {k: guarded(data[k].to(torch.uint8) if k == "terminated" else data[k]) for k in DH.ROW_KEYS}
    pdata = {k: guarded(data[k]) for k in ("params", "tparams", "cparams", "tcparams")}
    got = _call(env, pol, critic, pdata, guarded(with_bad), wg=2, rows_of=rows_of)
    alone = _call(env, pol, critic, pdata, guarded(padded), wg=2, rows_of=rows_of)
    torch.cuda.synchronize()
    assert int(got["stats"]["rows_skipped"]) == BAD and int(got["stats"]["rows_used"]) == M - BAD
    for k in ("grad_params", "grad_critic_params", "target", "q", "action", "target_noise"):
        assert bool(torch.isfinite(got[k]).all()), k
        assert _same(got[k].cpu().numpy(), alone[k].cpu().numpy()), k
    for k, v in got["stats"].items():
        assert np.isfinite(float(v)) and _same(v.cpu().numpy(), alone["stats"][k].cpu().numpy()), k
    off = ~valid.to(dev)
    assert not got["target"][off].any() and not got["q"][:, off].any() and not got["action"][off].any() and not got["target_noise"][off].any()
    for big, numel in guards:
        for pad in (big[:PAD], big[PAD + numel:]):
            assert bool(torch.isnan(pad).all() if big.dtype == torch.float32 else (pad == 1).all())
    noise = torch.zeros(M, 4)
    noise[valid] = got["target_noise"].cpu()[valid]
    idx = rows[valid].long()
    ref = DH.autograd(torch, pol, critic, data, idx, noise[valid], DH.GAMMA, torch.float64, "cpu", n_rows=M)
    yard = DH.autograd(torch, pol, critic, data, idx, noise[valid], DH.GAMMA, torch.float32, dev, n_rows=M)
    ker = _kernel(pol, critic, got)
    pooled = max(_rel(yard[k], ref[k]) for k in ref)
    for k in ref:
        assert _rel(ker[k], ref[k]) <= 4.0 * pooled, (k, _rel(ker[k], ref[k]), pooled)


# ---- 7. refusals ----
def test_refusals_enqueue_nothing(handles):
    import torch
    from rsoccer_amd import _lib, vec
    from rsoccer_amd.vec.policy import MLPCritic, MLPPolicy, MLPQCritic
    env = handles("VecVSSEnv")
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    pol, critic = MLPPolicy(OD, AD), MLPQCritic(OD, AD)
    N, M, C = 40, 24, 2
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)   # noqa: E731
    inp = {"obs": z(N, OD), "action": z(N, AD), "reward": z(N), "next_obs": z(N, OD), "terminated": z(N, dt=torch.uint8), "rows": z(M, dt=torch.int32)}
    aspec, cspec = pol.spec(), critic.spec()
    ws = z(env.sim.dpg_gradient_workspace(aspec, cspec, C, M, 0) // 4)
    seven = lambda *s: torch.full(s, 7.0, device=dev)   # noqa: E731
    out = {"grad_actor": seven(pol.num_params), "grad_critics": seven(C, critic.num_params), "stats": seven(9), "target": seven(M),
           "q": seven(C, M), "action": seven(M, AD), "target_noise": seven(M, AD), "workspace": ws}
    par = {"p": z(pol.num_params), "tp": z(pol.num_params), "cp": z(C, critic.num_params), "tcp": z(C, critic.num_params)}

    def raw(sim=env.sim, actor=aspec, crit=cspec, skip=(), n=N, m=M, gamma=0.99, sigma=0.2, clip=0.5, c=C, wg=0, no_in=False, no_cfg=False,
            no_out=False):
        ptr = lambda d, k, pre="": None if pre + k in skip else d[k].data_ptr()   # noqa: E731  (outputs are skipped as "out.<name>")
        i = _lib.DpgIn(*[ptr(inp, k) for k in ("obs", "action", "reward", "next_obs", "terminated", "rows")], n, m)
        o = _lib.DpgOut(*[ptr(out, k, "out.") for k in ("grad_actor", "grad_critics", "stats", "target", "q", "action", "target_noise", "workspace")])
        sim.task_dpg_gradient(actor, ptr(par, "p"), ptr(par, "tp"), crit, ptr(par, "cp"), ptr(par, "tcp"), None if no_in else i,
                              None if no_cfg else _lib.DpgCfg(None, 1, 0, gamma, sigma, clip, c, wg), None if no_out else o, env._stream())

    nan, inf = float("nan"), float("inf")
    bad = [dict(skip=(k,)) for k in ("obs", "action", "reward", "next_obs", "terminated", "out.grad_critics", "out.stats", "out.workspace", "p", "tp", "cp", "tcp")]
    bad += [dict(no_in=True), dict(no_cfg=True), dict(no_out=True), dict(actor=None), dict(crit=None)]
    bad += [dict(m=0), dict(m=-1), dict(n=0), dict(n=-5), dict(m=2 ** 31), dict(n=2 ** 31)]
    bad += [dict(c=v) for v in (0, 3, -1)] + [dict(gamma=v) for v in (nan, inf, -0.1, 1.5)]
    bad += [dict(sigma=v) for v in (nan, inf, -0.2)] + [dict(clip=v) for v in (nan, inf, -0.5)] + [dict(wg=-1)]
    bad += [dict(actor=_lib.PolicyMLP(*s)) for s in ((2, 48, _lib.ACT_TANH, _lib.ACT_TANH), (3, 64, _lib.ACT_TANH, _lib.ACT_TANH),
                                                     (2, 64, _lib.ACT_CLIP, _lib.ACT_TANH), (2, 64, _lib.ACT_TANH, _lib.ACT_NONE),
                                                     (2, 64, _lib.ACT_TANH, _lib.ACT_RELU))]
    bad += [dict(crit=_lib.PolicyMLP(*s)) for s in ((2, 48, _lib.ACT_TANH, _lib.ACT_NONE), (0, 64, _lib.ACT_TANH, _lib.ACT_NONE),
                                                    (2, 64, 7, _lib.ACT_NONE), (2, 64, _lib.ACT_TANH, _lib.ACT_TANH))]
    for kw in bad:
        with pytest.raises(_lib.RsxError):
            raw(**kw)
    bare = _lib.Sim(_lib.KIND_VSS, 0, 3, 3, 25, 9, 0)   # a handle without a task
    with pytest.raises(_lib.RsxError, match="task"):
        raw(sim=bare)
    with pytest.raises(_lib.RsxError, match="task"):
        bare.dpg_gradient_workspace(aspec, cspec, C, M, 0)
    bare.close()
    scrim = vec.VecSSLScrimmageEnv(2, device=0, seed=1)   # the scrimmage task commands every robot
    with pytest.raises(_lib.RsxError, match="scrimmage"):
        raw(sim=scrim.sim)
    scrim.close()
    for kw in (dict(n_rows=0), dict(n_rows=2 ** 31), dict(max_workgroups=-1), dict(c=3)):
        with pytest.raises(_lib.RsxError):
            env.sim.dpg_gradient_workspace(aspec, cspec, kw.get("c", C), kw.get("n_rows", M), kw.get("max_workgroups", 0))
    torch.cuda.synchronize()
    for k, v in out.items():
        if k != "workspace":
            assert (v == 7.0).all(), f"a refused call wrote {k}"
    raw(skip=("rows", "out.grad_actor", "out.target", "out.q", "out.action", "out.target_noise"))   # the optional arrays may be NULL
    torch.cuda.synchronize()
    for k in ("grad_actor", "target", "q", "action", "target_noise"):
        assert (out[k] == 7.0).all(), k
    assert not (out["grad_critics"] == 7.0).any() and float(out["stats"][7]) == M and float(out["stats"][8]) == 0
    raw()
    torch.cuda.synchronize()
    assert not any((out[k] == 7.0).any() for k in ("grad_actor", "target", "q", "action", "target_noise"))

    # the Python layer names the offender
    good = {"obs": z(N, OD), "actions": z(N, AD), "reward": z(N), "next_obs": z(N, OD), "terminated": z(N, dt=torch.bool)}
    a = (pol, par["p"], par["tp"], critic, par["cp"], par["tcp"])
    env.dpg_gradient(good, *a)
    for key, value in (("obs", z(N, OD + 1)), ("actions", z(N, AD + 1)), ("reward", z(N + 1)), ("next_obs", z(N, OD, dt=torch.float64)),
                       ("terminated", z(N)), ("reward", torch.zeros(N)), ("actions", z(N, 2 * AD)[..., ::2]), ("next_obs", np.zeros((N, OD), np.float32))):
        with pytest.raises(ValueError, match=key):
            env.dpg_gradient({**good, key: value}, *a)
    with pytest.raises(ValueError, match="next_obs"):
        env.dpg_gradient({k: v for k, v in good.items() if k != "next_obs"}, *a)
    for rows in ([0, N], [-1, 2], np.zeros((2, 2), np.int64), [], [0.5, 1.0], z(3), z(2, 2, dt=torch.int32)):
        with pytest.raises(ValueError, match="rows"):
            env.dpg_gradient(good, *a, rows=rows)
    env.dpg_gradient(good, *a, rows=[0, N - 1, 3, 3])
    for kw in (dict(gamma=1.5), dict(gamma=nan), dict(target_noise=-0.1), dict(target_noise=inf), dict(noise_clip=-1.0), dict(max_workgroups=0),
               dict(noise_step=z(1, dt=torch.int32)), dict(noise_step=torch.zeros(1, dtype=torch.int64))):
        with pytest.raises(ValueError, match=list(kw)[0]):
            env.dpg_gradient(good, *a, **kw)
    with pytest.raises(ValueError, match="policy"):
        env.dpg_gradient(good, critic, *a[1:])
    with pytest.raises(ValueError, match="critic"):
        env.dpg_gradient(good, pol, par["p"], par["tp"], MLPCritic(OD), par["cp"], par["tcp"])
    with pytest.raises(ValueError, match="critic"):
        env.dpg_gradient(good, pol, par["p"], par["tp"], MLPQCritic(OD, AD + 1), par["cp"], par["tcp"])
    with pytest.raises(ValueError, match="params"):
        env.dpg_gradient(good, pol, par["p"][:-1], par["tp"], critic, par["cp"], par["tcp"])
    with pytest.raises(ValueError, match="target_params"):
        env.dpg_gradient(good, pol, par["p"], par["tp"].cpu(), critic, par["cp"], par["tcp"])
    with pytest.raises(ValueError, match="critic_params"):
        env.dpg_gradient(good, pol, par["p"], par["tp"], critic, par["cp"][0], par["tcp"])
    with pytest.raises(ValueError, match="critic_params"):
        env.dpg_gradient(good, pol, par["p"], par["tp"], critic, z(3, critic.num_params), z(3, critic.num_params))
    with pytest.raises(ValueError, match="target_critic_params"):
        env.dpg_gradient(good, pol, par["p"], par["tp"], critic, par["cp"], par["tcp"][:1])
    one = env.dpg_gradient(good, pol, par["p"], par["tp"], critic, par["cp"][:1], par["tcp"][:1])   # DDPG: one critic
    torch.cuda.synchronize()
    assert one["grad_critic_params"].shape == (1, critic.num_params)
