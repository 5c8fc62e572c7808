"""VecFusedEnv.ppo_gradient / rsx_task_ppo_gradient: gradients of the PPO loss of include/rsx.h with respect to an MLP actor, its log_std
and an MLP critic.  The gradients and stats are checked against float64 autograd with torch's own float32 autograd as the yardstick,
the forward pass against collect()'s own mean and value bit for bit; then determinism, capture, out-of-range rows, side effects and
refusals."""
import copy

import numpy as np
import pytest

import test_gpu_policy_lookahead as PL   # the env factory, the bit comparison

pytestmark = pytest.mark.gpu

_same, _make = PL._same, PL._make
HALF_LOG_2PI = 0.9189385332046727
CLIP, VF, ENT = 0.2, 0.5, 0.01
KINK = 1e-5
STATS = ("loss_pi", "loss_v", "entropy", "approx_kl", "clip_fraction", "ratio")


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


def _pre(pol):
    """the policy with its output activation taken off: MLPPolicy.forward then returns the mean the Gaussian head is built on"""
    pre = copy.copy(pol)
    hid = pol._torch_acts()[0]
    pre._torch_acts = lambda: (hid, (lambda v: v))
    return pre


def _loss(torch, pol, critic, params, log_std, cparams, obs, sample, old_lp, adv, ret, rows, dtype, n_rows):
    """the loss of include/rsx.h on MLPPolicy.forward in ``dtype``; means are sums over the given rows divided by n_rows"""
    c = lambda t: t.to(dtype)   # noqa: E731
    x = c(obs)[rows]
    mean = _pre(pol).forward(x, params, dtype=dtype)
    value = critic.forward(x, cparams, dtype=dtype)[..., 0]
    z = (c(sample)[rows] - mean) / log_std.exp()
    lp = (-0.5 * z * z - log_std - HALF_LOG_2PI).sum(-1)
    logr = lp - c(old_lp)[rows]
    ratio = logr.exp()
    A = c(adv)[rows]
    lo, hi = (1.0 - CLIP, 1.0 + CLIP) if dtype == torch.float64 else (float(np.float32(1) - np.float32(CLIP)), float(np.float32(1) + np.float32(CLIP)))
    l_pi = -torch.minimum(ratio * A, ratio.clamp(lo, hi) * A).sum() / n_rows
    l_v = 0.5 * ((value - c(ret)[rows]) ** 2).sum() / n_rows
    ent = (log_std + 0.5 + HALF_LOG_2PI).sum()
    stats = {"loss_pi": l_pi, "loss_v": l_v, "entropy": ent, "approx_kl": ((ratio - 1.0) - logr).sum() / n_rows,
             "clip_fraction": ((ratio < lo) | (ratio > hi)).to(dtype).sum() / n_rows, "ratio": ratio.sum() / n_rows}
    return l_pi + VF * l_v - ENT * ent, stats, mean, value


def _autograd(torch, pol, critic, data, rows, dtype, device, n_rows=None):
    """{name: tensor} of the gradients per parameter tensor (each layer's W and b of both networks, log_std) and the six stats"""
    p = data["params"].to(device=device, dtype=dtype).requires_grad_(True)
    ls = data["log_std"].to(device=device, dtype=dtype).requires_grad_(True)
    cp = data["cparams"].to(device=device, dtype=dtype).requires_grad_(True)
    batch = [data[k].to(device) for k in ("obs", "sample", "old_lp", "adv", "ret")]
    r = rows.to(device).long()
    loss, stats, _, _ = _loss(torch, pol, critic, p, ls, cp, *batch, r, dtype, len(r) if n_rows is None else n_rows)
    loss.backward()
    out = {f"actor.{i}": t for i, t in enumerate(pol.unpack(p.grad.detach().cpu().double()))}
    out.update({f"critic.{i}": t for i, t in enumerate(critic.unpack(cp.grad.detach().cpu().double()))})
    out["log_std"] = ls.grad.detach().cpu().double()
    out.update({k: stats[k].detach().cpu().double() for k in STATS})
    return out


def _kernel(pol, critic, got):
    out = {f"actor.{i}": t for i, t in enumerate(pol.unpack(got["grad_params"].cpu().double()))}
    out.update({f"critic.{i}": t for i, t in enumerate(critic.unpack(got["grad_critic_params"].cpu().double()))})
    out["log_std"] = got["grad_log_std"].cpu().double()
    out.update({k: got["stats"][k].cpu().double() for k in STATS})
    return out


def _init(torch, net, gen):
    """flat float32 parameters of torch.nn.Linear's own initialisation"""
    ts = []
    for s in net.shapes:
        fan_in = s[1] if len(s) == 2 else None
        if fan_in is not None:
            bound = 1.0 / np.sqrt(fan_in)
        ts.append((torch.rand(s, generator=gen, dtype=torch.float64) * 2 - 1) * bound)
    return net.pack(ts)


def _data(torch, pol, critic, n, seed):
    """a flattened batch as collect() builds it and the parameters of the update: the old policy's perturbed by 0.02; rows within KINK
    of a kink in float64 (a relu pre-activation at 0, ratio at a clip bound) are taken out of the batch before anything is computed"""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)   # noqa: E731
    old_p, old_c = _init(torch, pol, gen), _init(torch, critic, gen)
    old_ls = (-0.5 + 0.1 * rnd(pol.act_dim)).float()
    obs = (torch.rand(n, pol.obs_dim, generator=gen, dtype=torch.float64) * 2 - 1).float()
    mean_old = _pre(pol).forward(obs, old_p, dtype=torch.float32)
    sigma = old_ls.exp()
    sample = mean_old + sigma * rnd(n, pol.act_dim).float()
    z = (sample - mean_old) / sigma
    old_lp = (-0.5 * z * z - old_ls - HALF_LOG_2PI).sum(-1)   # (collect()'s own expression, in float32)
    adv = rnd(n).float()
    ret = (critic.forward(obs, old_c, dtype=torch.float32)[..., 0] + 0.5 * rnd(n).float())
    data = {"params": (old_p + 0.02 * rnd(pol.num_params).float()), "cparams": (old_c + 0.02 * rnd(critic.num_params).float()),
            "log_std": (old_ls + 0.02 * rnd(pol.act_dim).float()), "obs": obs, "sample": sample, "old_lp": old_lp, "adv": adv, "ret": ret}
    # the kinks, in float64
    near = torch.zeros(n, dtype=torch.bool)
    for net, flat in ((pol, data["params"]), (critic, data["cparams"])):
        if net.hidden_act == "relu":
            ts = [t.double() for t in net.unpack(flat)]
            x = obs.double()
            for li in range(len(ts) // 2 - 1):
                pre_act = x @ ts[2 * li].T + ts[2 * li + 1]
                near |= (pre_act.abs() < KINK).any(-1)
                x = torch.relu(pre_act)
    mean = _pre(pol).forward(obs, data["params"], dtype=torch.float64)
    z = (sample.double() - mean) / data["log_std"].double().exp()
    ratio = ((-0.5 * z * z - data["log_std"].double() - HALF_LOG_2PI).sum(-1) - old_lp.double()).exp()
    near |= ((ratio - (1.0 - CLIP)).abs() < KINK) | ((ratio - (1.0 + CLIP)).abs() < KINK)
    removed = int(near.sum())
    assert removed <= 0.02 * n, f"the kink filter removed {removed} of {n} rows"
    keep = ~near
    for k in ("obs", "sample", "old_lp", "adv", "ret"):
        data[k] = data[k][keep].contiguous()
    clipped = float(((ratio[keep] < 1.0 - CLIP) | (ratio[keep] > 1.0 + CLIP)).double().mean())
    return data, removed, clipped


def _rows(torch, mode, m, n, seed):
    gen = torch.Generator().manual_seed(seed + 1000)
    if mode == "none":
        return None
    if mode == "perm":
        return torch.randperm(n, generator=gen)[:m].to(torch.int32)
    return torch.randint(0, n, (m,), generator=gen).to(torch.int64)   # repeats (int64: converted by the method)


def _batch(data, dev, T=1):
    n = data["obs"].shape[0]
    shp = lambda t: t.reshape((T, n // T) + tuple(t.shape[1:])).contiguous().to(dev)   # noqa: E731
    return {"obs": shp(data["obs"]), "sample": shp(data["sample"]), "log_prob": shp(data["old_lp"]), "advantage": shp(data["adv"]),
            "return": shp(data["ret"])}


def _call(env, pol, critic, data, rows, max_workgroups=None, **kw):
    dev = env.device
    return env.ppo_gradient(_batch(data, dev), pol, data["params"].to(dev), data["log_std"].to(dev), critic, data["cparams"].to(dev),
                            rows=None if rows is None else rows.to(dev), clip=CLIP, vf_coef=VF, ent_coef=ENT,
                            max_workgroups=max_workgroups, **kw)


def _nets(env, hidden, layers, act):
    from rsoccer_amd.vec.policy import MLPCritic, MLPPolicy
    return (MLPPolicy(env.sim.obs_dim, env.sim.act_dim, hidden=hidden, layers=layers, hidden_act=act, out_act="tanh"),
            MLPCritic(env.sim.obs_dim, hidden=hidden, layers=layers, hidden_act=act))


def _rel(x, ref):
    scale = float(ref.abs().max())
    err = float((x - ref).abs().max())
    if scale == 0.0:
        assert err == 0.0, "the reference is exactly zero, the result is not"
        return 0.0
    return err / scale


# ---- 1. gradients and stats against float64 autograd, torch's float32 autograd as the yardstick ----
# obs_dim 40 / 21 / 14 / 64 with act_dim 2 / 4 / 5 / 2; M around the block of 64 rows and at 65 blocks; with max_workgroups = 2 a
# workgroup makes several trips and ends on a partial block
CASES = [
    ("VecVSSEnv", 64, 2, "tanh", 4097, "perm", None),
    ("VecVSSEnv", 64, 2, "relu", 4097, "repeats", 2),
    ("VecVSSEnv", 64, 1, "tanh", 65, "none", 1),
    ("VecVSSEnv", 32, 2, "tanh", 64, "perm", 2),
    ("VecVSSEnv", 32, 1, "relu", 63, "repeats", None),
    ("VecVSSEnv", 64, 2, "tanh", 1, "perm", 1),
    ("VecSSLDribblingEnv", 64, 2, "tanh", 4097, "none", 2),
    ("VecSSLDribblingEnv", 32, 2, "relu", 65, "perm", 1),
    ("VecSSLDribblingEnv", 64, 1, "tanh", 64, "repeats", 2),
    ("VecSSLContestedPossessionEnv", 64, 1, "relu", 4097, "repeats", None),
    ("VecSSLContestedPossessionEnv", 32, 2, "tanh", 1, "none", None),
    ("VecSSLContestedPossessionEnv", 32, 1, "tanh", 63, "perm", 2),
    ("VecVSS5v5", 64, 2, "tanh", 4097, "perm", 2),
    ("VecVSS5v5", 64, 2, "relu", 65, "repeats", None),
    ("VecVSS5v5", 32, 1, "tanh", 63, "none", 1),
]


@pytest.mark.parametrize("name,hidden,layers,act,M,mode,wg", CASES)
def test_gradients_and_stats_stay_within_4x_of_torchs_float32_error(handles, name, hidden, layers, act, M, mode, wg):
    """Criterion (the issue's): for every parameter tensor and the first six stats, the kernel's relative error against float64
    autograd is at most 4x the LARGEST relative error any tensor of torch's float32 autograd on the device shows in the same case."""
    import torch
    env = handles(name)
    assert (env.sim.obs_dim, env.sim.act_dim) == {"VecVSSEnv": (40, 2), "VecSSLDribblingEnv": (21, 4),
                                                  "VecSSLContestedPossessionEnv": (14, 5), "VecVSS5v5": (64, 2)}[name]
    pol, critic = _nets(env, hidden, layers, act)
    seed = 7 + M + hidden + layers
    data, removed, clipped = _data(torch, pol, critic, M + 64, seed)
    assert data["obs"].shape[0] >= M
    if mode == "none":   # rows=None is the whole batch: the batch has M rows
        for k in ("obs", "sample", "old_lp", "adv", "ret"):
            data[k] = data[k][:M].contiguous()
    n = data["obs"].shape[0]
    rows = _rows(torch, mode, M, n, seed)
    idx = torch.arange(M) if rows is None else rows.long()
    ref = _autograd(torch, pol, critic, data, idx, torch.float64, "cpu")
    yard = _autograd(torch, pol, critic, data, idx, torch.float32, env.device)
    got = _call(env, pol, critic, data, rows, max_workgroups=wg)
    torch.cuda.synchronize()
    assert int(got["stats"]["rows_used"]) == M and int(got["stats"]["rows_skipped"]) == 0
    ker = _kernel(pol, critic, got)
    e_yard = {k: _rel(yard[k], ref[k]) for k in ref}
    e_ker = {k: _rel(ker[k], ref[k]) for k in ref}
    pooled = max(e_yard.values())
    worst = max(e_ker, key=e_ker.get)
    print(f"{name} {hidden}x{layers} {act} M={M} {mode} wg={wg}: removed {removed}, clipped {clipped:.3f}, torch f32 pooled {pooled:.3e}, "
          f"kernel worst {e_ker[worst]:.3e} ({worst}), ratio {e_ker[worst] / pooled:.2f}")
    assert pooled > 0.0
    for k in ref:
        assert e_ker[k] <= 4.0 * pooled, (k, e_ker[k], pooled, e_ker[k] / pooled)


# ---- 2. the forward pass on a real batch: collect()'s own mean and value, bit for bit ----
@pytest.mark.parametrize("name,B", [("VecVSSEnv", 64), ("VecSSLStaticDefendersEnv", 16)])
def test_forward_equals_collects_mean_and_value_bit_for_bit(name, B):
    import torch
    from rsoccer_amd import vec
    T = 8
    env = _make(vec, name, B, device=0, seed=2025, max_episode_steps=5)
    PL._start(torch, env)
    dev = env.device
    pol, critic = _nets(env, 64, 2, "tanh")
    gen = torch.Generator().manual_seed(3)
    params, cparams = _init(torch, pol, gen).to(dev), _init(torch, critic, gen).to(dev)
    log_std = torch.full((env.sim.act_dim,), -0.7, device=dev)
    batch = env.collect(pol, params, T, log_std=log_std, noise_seed=11, critic=critic, critic_params=cparams)
    before = env.checkpoint()
    for rows in (None, torch.randperm(T * B, generator=gen)[:T * B - 29].to(torch.int32).to(dev),
                 torch.randint(0, T * B, (70,), generator=gen).to(dev)):
        out = env.ppo_gradient(batch, pol, params, log_std, critic, cparams, rows=rows, return_forward=True)
        torch.cuda.synchronize()
        at = slice(None) if rows is None else rows.long()
        assert _same(out["mean"].cpu().numpy(), batch["mean"].reshape(-1, env.sim.act_dim)[at].cpu().numpy())
        assert _same(out["value"].cpu().numpy(), batch["value"].reshape(-1)[at].cpu().numpy())
        # the same parameters: ratio is 1 up to the rounding of log_prob, whose float32 error is eps * its magnitude
        bound = float(np.finfo(np.float32).eps) * float(batch["log_prob"].abs().max())
        kl = float(out["stats"]["approx_kl"])
        print(name, "approx_kl", kl, "bound", bound, "ratio", float(out["stats"]["ratio"]))
        assert abs(kl) < bound and float(out["stats"]["clip_fraction"]) == 0.0
        for k in ("grad_params", "grad_log_std", "grad_critic_params"):
            assert bool(torch.isfinite(out[k]).all()), k
    # ---- 5. no side effects ----
    assert np.array_equal(env.checkpoint(), before)
    env.close()


# ---- 3. determinism, eagerly and from a graph ----
def test_two_calls_and_a_replayed_graph_return_the_same_bits(handles):
    import torch
    env = handles("VecVSSEnv")
    dev = env.device
    pol, critic = _nets(env, 64, 2, "tanh")
    M = 700
    data, _, _ = _data(torch, pol, critic, M + 64, 31)
    other, _, _ = _data(torch, pol, critic, M + 64, 32)
    n = min(data["obs"].shape[0], other["obs"].shape[0])
    for d in (data, other):
        for k in ("obs", "sample", "old_lp", "adv", "ret"):
            d[k] = d[k][:n].contiguous()
    rows = _rows(torch, "repeats", M, n, 5).to(torch.int32).to(dev)
    static = _batch(data, dev)
    p, ls, cp = (data[k].to(dev) for k in ("params", "log_std", "cparams"))

    def run():
        return env.ppo_gradient(static, pol, p, ls, critic, cp, rows=rows, clip=CLIP, vf_coef=VF, ent_coef=ENT, return_forward=True)

    def flat(out):
        return torch.cat([out[k].reshape(-1) for k in ("grad_params", "grad_log_std", "grad_critic_params", "mean", "value")] +
                         [torch.stack(list(out["stats"].values()))]).clone().view(torch.int32)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # eager calls, which are also torch's warm-up before a capture
        a, b = flat(run()), flat(run())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run()
    fresh = _batch(other, dev)
    for k in static:   # the inputs overwritten in place
        static[k].copy_(fresh[k])
    for t, k in ((p, "params"), (ls, "log_std"), (cp, "cparams")):
        t.copy_(other[k].to(dev))
    seen = []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        seen.append(flat(out))
    want = flat(run())
    torch.cuda.synchronize()
    assert torch.equal(seen[0], want) and torch.equal(seen[1], want) and not torch.equal(want, a)


# ---- 4. out-of-range and padding rows ----
def test_out_of_range_rows_contribute_nothing_and_nothing_outside_is_read(handles):
    """The minibatch keeps its M entries; 41 of them are out of range (negative, >= N, the int32 extremes), scattered and as a padded
    tail.  The call on the valid entries alone is the same minibatch with every other entry a plain -1 padding: the same M and the
    same positions (the summation order is by position), so the bits must agree; and its gradients are those of float64 autograd over
    the valid entries with the divisor M.  The batch tensors are views into the middle of NaN-filled allocations."""
    import torch
    env = handles("VecSSLDribblingEnv")
    dev = env.device
    pol, critic = _nets(env, 64, 2, "relu")
    M, BAD = 300, 41
    data, _, _ = _data(torch, pol, critic, 400, 77)
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

    def guarded(t, pad=1000):
        big = torch.full((t.numel() + 2 * pad,), float("nan"), dtype=t.dtype, device=dev)
        view = big[pad:pad + t.numel()].view(t.shape)
        view.copy_(t)
        return view

    batch = {k: guarded(v) for k, v in _batch(data, dev).items()}
    args = (pol, guarded(data["params"].to(dev)), guarded(data["log_std"].to(dev)), critic, guarded(data["cparams"].to(dev)))
    kw = dict(clip=CLIP, vf_coef=VF, ent_coef=ENT, return_forward=True, max_workgroups=2)
    got = env.ppo_gradient(batch, *args, rows=with_bad.to(dev), **kw)
    alone = env.ppo_gradient(batch, *args, rows=padded.to(dev), **kw)
    torch.cuda.synchronize()
    assert int(got["stats"]["rows_skipped"]) == BAD and int(got["stats"]["rows_used"]) == M - BAD
    for k in ("grad_params", "grad_log_std", "grad_critic_params", "mean", "value"):
        assert bool(torch.isfinite(got[k]).all()), k
        assert _same(got[k].cpu().numpy(), alone[k].cpu().numpy()), k
    for k, v in got["stats"].items():
        assert np.isfinite(float(v)) and _same(v.cpu().numpy(), alone["stats"][k].cpu().numpy()), k
    assert not got["mean"][~valid.to(dev)].any() and not got["value"][~valid.to(dev)].any()
    ref = _autograd(torch, pol, critic, data, rows[valid].long(), torch.float64, "cpu", n_rows=M)
    yard = _autograd(torch, pol, critic, data, rows[valid].long(), torch.float32, dev, n_rows=M)
    ker = _kernel(pol, critic, got)
    pooled = max(_rel(yard[k], ref[k]) for k in ref)
    for k in ref:
        assert _rel(ker[k], ref[k]) <= 4.0 * pooled, (k, _rel(ker[k], ref[k]), pooled)


# ---- 6. refusals ----
def test_refusals_enqueue_nothing(handles):
    import torch
    from rsoccer_amd import _lib, vec
    env = handles("VecVSSEnv")
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    pol, critic = _nets(env, 64, 2, "tanh")
    N, M = 40, 24
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)   # noqa: E731
    inp = {"obs": z(N, OD), "sample": z(N, AD), "old_log_prob": z(N), "advantage": z(N), "ret": z(N), "rows": z(M, dt=torch.int32)}
    aspec, cspec = pol.spec(), critic.spec()
    ws = z(env.sim.ppo_gradient_workspace(aspec, cspec, M, 0) // 4)
    out = {"grad_actor": torch.full((pol.num_params,), 7.0, device=dev), "grad_log_std": torch.full((AD,), 7.0, device=dev),
           "grad_critic": torch.full((critic.num_params,), 7.0, device=dev), "stats": torch.full((8,), 7.0, device=dev),
           "mean": torch.full((M, AD), 7.0, device=dev), "value": torch.full((M,), 7.0, device=dev), "workspace": ws}
    par = {"p": z(pol.num_params), "ls": z(AD), "cp": z(critic.num_params)}

    def raw(sim=env.sim, actor=aspec, crit=cspec, skip=(), n=N, m=M, clip=0.2, vf=0.5, ent=0.0, wg=0, no_in=False, no_cfg=False, no_out=False):
        ptr = lambda d, k: None if k in skip else d[k].data_ptr()   # noqa: E731
        i = _lib.PpoIn(*[ptr(inp, k) for k in ("obs", "sample", "old_log_prob", "advantage", "ret", "rows")], n, m)
        o = _lib.PpoOut(*[ptr(out, k) for k in ("grad_actor", "grad_log_std", "grad_critic", "stats", "mean", "value", "workspace")])
        sim.task_ppo_gradient(actor, ptr(par, "p"), ptr(par, "ls"), crit, ptr(par, "cp"), None if no_in else i,
                              None if no_cfg else _lib.PpoCfg(clip, vf, ent, wg), None if no_out else o, env._stream())

    nan, inf = float("nan"), float("inf")
    bad = [dict(skip=(k,)) for k in ("obs", "sample", "old_log_prob", "advantage", "ret", "grad_actor", "grad_log_std", "grad_critic", "stats",
                                     "workspace", "p", "ls", "cp")]
    bad += [dict(no_in=True), dict(no_cfg=True), dict(no_out=True), dict(actor=None), dict(crit=None)]
    bad += [dict(m=0), dict(m=-1), dict(n=0), dict(n=-5), dict(m=2 ** 31), dict(n=2 ** 31)]
    bad += [dict(clip=v) for v in (nan, inf, 0.0, 1.0, -0.2, 1.5)] + [dict(vf=v) for v in (nan, inf)] + [dict(ent=v) for v in (nan, -inf)]
    bad += [dict(wg=-1)]
    bad += [dict(actor=_lib.PolicyMLP(*s)) for s in ((2, 48, _lib.ACT_TANH, _lib.ACT_TANH), (3, 64, _lib.ACT_TANH, _lib.ACT_TANH),
                                                     (2, 64, _lib.ACT_CLIP, _lib.ACT_TANH), (2, 64, _lib.ACT_TANH, _lib.ACT_NONE))]
    bad += [dict(crit=_lib.PolicyMLP(*s)) for s in ((2, 48, _lib.ACT_TANH, _lib.ACT_NONE), (0, 64, _lib.ACT_TANH, _lib.ACT_NONE),
                                                    (2, 64, 7, _lib.ACT_NONE), (2, 64, _lib.ACT_TANH, _lib.ACT_TANH))]
    for kw in bad:
        with pytest.raises(_lib.RsxError):
            raw(**kw)
    bare = _lib.Sim(_lib.KIND_VSS, 0, 3, 3, 25, 9, 0)   # a handle without a task
    with pytest.raises(_lib.RsxError, match="task"):
        raw(sim=bare)
    with pytest.raises(_lib.RsxError, match="task"):
        bare.ppo_gradient_workspace(aspec, cspec, M, 0)
    bare.close()
    scrim = vec.VecSSLScrimmageEnv(2, device=0, seed=1)   # the scrimmage task commands every robot
    with pytest.raises(_lib.RsxError, match="scrimmage"):
        raw(sim=scrim.sim)
    scrim.close()
    for kw in (dict(n_rows=0), dict(n_rows=2 ** 31), dict(max_workgroups=-1)):
        with pytest.raises(_lib.RsxError):
            env.sim.ppo_gradient_workspace(aspec, cspec, kw.get("n_rows", M), kw.get("max_workgroups", 0))
    torch.cuda.synchronize()
    for k, v in out.items():
        if k != "workspace":
            assert (v == 7.0).all(), f"a refused call wrote {k}"
    raw(skip=("rows", "mean", "value"))   # the optional arrays may be NULL
    torch.cuda.synchronize()
    assert (out["mean"] == 7.0).all() and (out["value"] == 7.0).all() and not (out["grad_actor"] == 7.0).any()
    assert float(out["stats"][6]) == M and float(out["stats"][7]) == 0

    # the Python layer names the offender
    T, B = 2, N // 2
    good = {"obs": z(T, B, OD), "sample": z(T, B, AD), "log_prob": z(T, B), "advantage": z(T, B), "return": z(T, B)}
    a = (pol, par["p"], par["ls"], critic, par["cp"])
    env.ppo_gradient(good, *a)
    for key, value in (("obs", z(T, B, OD + 1)), ("sample", z(T, B, AD + 1)), ("log_prob", z(T, B + 1)), ("return", z(T, B, dt=torch.float64)),
                       ("advantage", torch.zeros(T, B)), ("sample", z(T, B, 2 * AD)[..., ::2]), ("return", np.zeros((T, B), np.float32))):
        with pytest.raises(ValueError, match=key):
            env.ppo_gradient({**good, key: value}, *a)
    with pytest.raises(ValueError, match="return"):
        env.ppo_gradient({k: v for k, v in good.items() if k != "return"}, *a)
    with pytest.raises(ValueError, match="advantage"):
        env.ppo_gradient(good, *a, advantage=z(T, B + 1))
    env.ppo_gradient({k: v for k, v in good.items() if k != "advantage"}, *a, advantage=z(T, B))
    for rows in ([0, N], [-1, 2], np.zeros((2, 2), np.int64), [], [0.5, 1.0], z(3), z(2, 2, dt=torch.int32), torch.zeros(3, dtype=torch.int64)[:0].to(dev)):
        with pytest.raises(ValueError, match="rows"):
            env.ppo_gradient(good, *a, rows=rows)
    env.ppo_gradient(good, *a, rows=[0, N - 1, 3, 3])
    for kw in (dict(clip=0.0), dict(clip=1.0), dict(clip=nan), dict(vf_coef=inf), dict(ent_coef=nan), dict(max_workgroups=0), dict(max_workgroups=-2)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            env.ppo_gradient(good, *a, **kw)
    with pytest.raises(ValueError, match="policy"):
        env.ppo_gradient(good, critic, par["p"], par["ls"], critic, par["cp"])
    with pytest.raises(ValueError, match="critic"):
        env.ppo_gradient(good, pol, par["p"], par["ls"], pol, par["cp"])
    with pytest.raises(ValueError, match="params"):
        env.ppo_gradient(good, pol, par["p"][:-1], par["ls"], critic, par["cp"])
    with pytest.raises(ValueError, match="log_std"):
        env.ppo_gradient(good, pol, par["p"], z(AD + 1), critic, par["cp"])
    with pytest.raises(ValueError, match="critic_params"):
        env.ppo_gradient(good, pol, par["p"], par["ls"], critic, par["cp"].cpu())
    with pytest.raises(ValueError):
        env.ppo_gradient(good, type(pol)(OD + 1, AD), z(type(pol)(OD + 1, AD).num_params), par["ls"], critic, par["cp"])
    torch.cuda.synchronize()
