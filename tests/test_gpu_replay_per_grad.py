"""Per-row discounts, per-entry weights and the TD error in VecFusedEnv.dpg_gradient and VecFusedEnv.sac_gradient
(rsx_task_dpg_gradient_w, rsx_task_sac_gradient_w): neutral inputs leave every bit alone, random ones are held against float64
autograd of the weighted loss with torch's own float32 autograd as the yardstick (tests/dpg_helpers.py, tests/sac_helpers.py: their
data, their kink filter, their cap), the TD error is max_c |q_c - target| of the per-entry outputs in bits, and a weight of 0 takes
an entry out of the critics' gradient exactly as an index of -1 does while the actor's gradient does not see weights at all."""
import numpy as np
import pytest

import dpg_helpers as DH
import sac_helpers as SH
import test_gpu_policy_lookahead as PL   # the env factory

pytestmark = pytest.mark.gpu

SEED64, STEP = 0x0123456789ABCDEF, 3
SHAPES = [(9, 1), (9, 3), (64, 1), (64, 3), (65, 1), (65, 3), (200, 1), (200, 3)]   # (M, max_workgroups)


@pytest.fixture(scope="module")
def env():
    """never reset and never stepped: the calls need only its device, obs_dim and act_dim"""
    from rsoccer_amd import vec
    e = PL._make(vec, "VecVSSEnv", 9, device=0, seed=1)
    yield e
    e.close()


def _dpg_case(M, wg):
    """the smallest networks of the existing gradient tests (hidden 32); relu and repeats on half of the shapes"""
    odd = M in (64, 200)
    return ((40, 2), 32, 2 if odd else 1, "relu" if odd else "tanh", "clip" if odd else "tanh", 2, M, "repeats" if odd else "perm", wg, 0.2)


def _sac_case(M, wg):
    odd = M in (64, 200)
    return ((40, 2), 32, 2 if odd else 1, "relu" if odd else "tanh", 2, M, "repeats" if odd else "perm", wg, "narrow" if odd else "default")


def _extras(torch, n, M, seed):
    """random discounts by row [n] and weights by position [M], float32"""
    gen = torch.Generator().manual_seed(seed + 77)
    return (0.5 + 0.5 * torch.rand(n, generator=gen)).float(), (0.1 + 0.9 * torch.rand(M, generator=gen)).float()


def _rel(x, ref):
    scale = float(ref.abs().max())
    err = float((x - ref).abs().max())
    if scale == 0.0:
        assert err == 0.0, "the reference is exactly zero, the result is not"
        return 0.0
    return err / scale


def _bits_equal(torch, a, b, keys):
    for k in keys:
        x, y = (torch.stack(list(o[k].values())) if k == "stats" else o[k] for o in (a, b))
        assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)), k


def _within(ref, yard, ker, what):
    e_yard = {k: _rel(yard[k], ref[k]) for k in ref}
    e_ker = {k: _rel(ker[k], ref[k]) for k in ref}
    pooled = max(e_yard.values())
    worst = max(e_ker, key=e_ker.get)
    print(f"{what}: torch f32 pooled {pooled:.3e}, kernel worst {e_ker[worst]:.3e} ({worst}), ratio {e_ker[worst] / pooled:.2f}")
    assert pooled > 0.0
    for k in ref:
        assert e_ker[k] <= 4.0 * pooled, (k, e_ker[k], pooled, e_ker[k] / pooled)


def _td_of(got):
    q, y = got["q"].cpu().numpy(), got["target"].cpu().numpy()
    return np.abs(q - y[None, :]).max(axis=0)


# ---- TD3 / DDPG ----
def _dpg_call(env, pol, critic, data, rows, wg, extra=None, **kw):
    dev = env.device
    rows_of = {k: data[k].to(dev).contiguous() for k in DH.ROW_KEYS}
    rows_of.update(extra or {})
    args = dict(rows=None if rows is None else rows.to(dev), gamma=DH.GAMMA, target_noise=0.2, noise_clip=DH.NOISE_CLIP, noise_seed=SEED64,
                noise_step=STEP, max_workgroups=wg, return_rows=True)
    args.update(kw)
    return env.dpg_gradient(rows_of, pol, data["params"].to(dev), data["tparams"].to(dev), critic, data["cparams"].to(dev),
                            data["tcparams"].to(dev), **args)


def _dpg_autograd_w(torch, pol, critic, data, idx, noise, disc, w, dtype, device, n_rows):
    """DH.autograd with the weighted critic loss 0.5 * sum(w (Q_c - y)^2) / M and y discounted by the row's own discount"""
    p = data["params"].to(device=device, dtype=dtype).requires_grad_(True)
    cp = data["cparams"].to(device=device, dtype=dtype).requires_grad_(True)
    tp, tcp = data["tparams"].to(device=device, dtype=dtype), data["tcparams"].to(device=device, dtype=dtype)
    idx = idx.to(device).long()
    r = {k: data[k].to(device)[idx] for k in DH.ROW_KEYS}
    w, g = w.to(device=device, dtype=dtype), disc.to(device)[idx].to(dtype)
    x, a = r["obs"].to(dtype), r["actions"].to(dtype)
    with torch.no_grad():
        y, _ = DH.targets(torch, pol, critic, tp, tcp, r["next_obs"].to(dtype), r["reward"], r["terminated"], noise.to(device), g, dtype)
    stats, l_q = {}, 0.0
    for c in range(cp.shape[0]):
        q = critic.forward(x, a, cp[c], dtype=dtype)[..., 0]
        stats[f"loss_q{c}"] = 0.5 * (w * (q - y) ** 2).sum() / n_rows
        stats[f"q{c}"] = q.sum() / n_rows
        l_q = l_q + stats[f"loss_q{c}"]
    l_pi = -critic.forward(x, pol.forward(x, p, dtype=dtype), cp[0].detach(), dtype=dtype)[..., 0].sum() / n_rows
    stats["loss_pi"], stats["target"] = l_pi, y.sum() / n_rows
    g_c, = torch.autograd.grad(l_q, [cp])
    g_a, = torch.autograd.grad(l_pi, [p])
    out = {f"actor.{i}": t for i, t in enumerate(pol.unpack(g_a.detach().cpu().double()))}
    for c in range(cp.shape[0]):
        out.update({f"critic{c}.{i}": t for i, t in enumerate(critic.unpack(g_c[c].detach().cpu().double()))})
    out.update({k: v.detach().cpu().double() for k, v in stats.items()})
    return out


DPG_KEYS = ("grad_params", "grad_critic_params", "target", "q", "action", "target_noise", "stats")


@pytest.mark.parametrize("M,wg", SHAPES)
def test_dpg_gradient_with_discounts_weights_and_td_error(env, M, wg):
    import torch
    case = _dpg_case(M, wg)
    pol, critic, data, removed, n0 = DH.case_data(torch, case)
    assert removed <= 0.02 * n0, f"the kink filter removed {removed} of {n0} rows"
    n = data["obs"].shape[0]
    rows = DH.make_rows(torch, case[7], M, n, DH.case_seed(case))
    idx, dev = rows.long(), env.device
    disc, w = _extras(torch, n, M, M)
    # neutral inputs: the bits of the call without either, for every output
    plain = _dpg_call(env, pol, critic, data, rows, wg)
    neutral = _dpg_call(env, pol, critic, data, rows, wg, extra={"discount": torch.full((n,), DH.GAMMA, device=dev)},
                        weights=torch.ones(M, device=dev), return_td_error=True)
    _bits_equal(torch, plain, neutral, DPG_KEYS)
    assert "td_error" not in plain
    # random ones against float64 autograd of the weighted loss with per-row discounts
    got = _dpg_call(env, pol, critic, data, rows, wg, extra={"discount": disc.to(dev)}, weights=w.to(dev), return_td_error=True)
    torch.cuda.synchronize()
    assert int(got["stats"]["rows_used"]) == M and int(got["stats"]["rows_skipped"]) == 0
    noise = got["target_noise"].cpu()
    ref = _dpg_autograd_w(torch, pol, critic, data, idx, noise, disc, w, torch.float64, "cpu", M)
    yard = _dpg_autograd_w(torch, pol, critic, data, idx, noise, disc, w, torch.float32, dev, M)
    ker = {f"actor.{i}": t for i, t in enumerate(pol.unpack(got["grad_params"].cpu().double()))}
    for c in range(2):
        ker.update({f"critic{c}.{i}": t for i, t in enumerate(critic.unpack(got["grad_critic_params"][c].cpu().double()))})
    ker.update({k: got["stats"][k].cpu().double() for k in ("loss_q0", "loss_q1", "q0", "q1", "loss_pi", "target")})
    assert set(ref) == set(ker)
    _within(ref, yard, ker, f"dpg M={M} wg={wg}")
    assert not torch.equal(got["grad_critic_params"], plain["grad_critic_params"]) and not torch.equal(got["target"], plain["target"])
    # the TD error is max_c |q_c - target| of the per-entry outputs, in bits
    assert np.array_equal(got["td_error"].cpu().numpy().view(np.uint32), _td_of(got).view(np.uint32))
    assert np.array_equal(neutral["td_error"].cpu().numpy().view(np.uint32), _td_of(plain).view(np.uint32))
    # a weight of 0 on an entry: the critics' gradient of the call with that entry's index at -1; the actor's does not see weights
    off = torch.zeros(M, dtype=torch.bool)
    off[[0, M // 2, M - 1]] = True
    w0 = torch.where(off, torch.zeros(()), w)
    r_off = rows.to(torch.int32).clone()
    r_off[off] = -1
    zero = _dpg_call(env, pol, critic, data, rows, wg, extra={"discount": disc.to(dev)}, weights=w0.to(dev), return_td_error=True)
    skip = _dpg_call(env, pol, critic, data, r_off, wg, extra={"discount": disc.to(dev)}, weights=w0.to(dev), return_td_error=True)
    torch.cuda.synchronize()
    assert torch.equal(zero["grad_critic_params"], skip["grad_critic_params"])   # (values: a -0.0 may stand where the other has +0.0)
    assert torch.equal(zero["grad_params"].view(torch.int32), got["grad_params"].view(torch.int32))
    assert int(skip["stats"]["rows_skipped"]) == int(off.sum())
    td = skip["td_error"].cpu()
    assert not td[off].any() and bool((td[~off] > 0).all())
    assert np.array_equal(td.numpy().view(np.uint32), _td_of(skip).view(np.uint32))


def test_the_td_error_needs_no_other_output_and_the_old_call_is_untouched(env):
    import torch
    case = _dpg_case(65, 1)
    pol, critic, data, _, _ = DH.case_data(torch, case)
    rows = DH.make_rows(torch, case[7], 65, data["obs"].shape[0], DH.case_seed(case))
    a = _dpg_call(env, pol, critic, data, rows, 1, return_rows=False, return_td_error=True)
    b = _dpg_call(env, pol, critic, data, rows, 1)
    assert "target" not in a and "q" not in a
    assert np.array_equal(a["td_error"].cpu().numpy().view(np.uint32), _td_of(b).view(np.uint32))
    dev = env.device
    with pytest.raises(ValueError, match="weights"):
        _dpg_call(env, pol, critic, data, rows, 1, weights=torch.ones(64, device=dev))
    with pytest.raises(ValueError, match="discount"):
        _dpg_call(env, pol, critic, data, rows, 1, extra={"discount": torch.ones(3, device=dev)})
    with pytest.raises(ValueError, match="weights"):
        _dpg_call(env, pol, critic, data, rows, 1, weights=torch.ones(65, device=dev, dtype=torch.float64))


# ---- soft actor-critic ----
def _sac_call(env, b, rows, wg, extra=None, **kw):
    dev = env.device
    data = b["data"]
    rows_of = {k: data[k].to(dev).contiguous() for k in SH.ROW_KEYS}
    rows_of.update(extra or {})
    args = dict(rows=None if rows is None else rows.to(dev), gamma=SH.GAMMA, noise_seed=SH.SEED64, noise_step=SH.STEP, max_workgroups=wg,
                return_rows=True)
    args.update(kw)
    return env.sac_gradient(rows_of, b["pol"], data["params"].to(dev), b["critic"], data["cparams"].to(dev), data["tcparams"].to(dev),
                            data["log_alpha"].to(dev), **args)


def _sac_autograd_w(torch, pol, critic, data, idx, eps, next_eps, disc, w, dtype, device, n_rows):
    """SH.autograd with the weighted critic loss and y discounted by the row's own discount; L_pi and L_alpha unweighted"""
    p = data["params"].to(device=device, dtype=dtype).requires_grad_(True)
    cp = data["cparams"].to(device=device, dtype=dtype).requires_grad_(True)
    la = data["log_alpha"].to(device=device, dtype=dtype).requires_grad_(True)
    tcp = data["tcparams"].to(device=device, dtype=dtype)
    idx = idx.to(device).long()
    r = {k: data[k].to(device)[idx] for k in SH.ROW_KEYS}
    w, g = w.to(device=device, dtype=dtype), disc.to(device)[idx].to(dtype)
    eps, next_eps = eps.to(device), next_eps.to(device)
    te = -float(pol.act_dim)
    x, a = r["obs"].to(dtype), r["actions"].to(dtype)
    with torch.no_grad():
        y, next_logp = SH.targets(torch, pol, critic, p.detach(), tcp, la.detach(), r["next_obs"].to(dtype), r["reward"], r["terminated"],
                                  next_eps.to(dtype), g, dtype)
    stats, l_q = {}, 0.0
    q = SH.q_all(torch, critic, cp, x, a, dtype)
    for c in range(cp.shape[0]):
        stats[f"loss_q{c}"] = 0.5 * (w * (q[c] - y) ** 2).sum() / n_rows
        stats[f"q{c}"] = q[c].sum() / n_rows
        l_q = l_q + stats[f"loss_q{c}"]
    alpha = la.detach().exp()
    a_new, logp, _ = pol.sample(x, p, eps.to(dtype), dtype=dtype)
    l_pi = (alpha * logp - SH.q_all(torch, critic, cp.detach(), x, a_new, dtype).min(0).values).sum() / n_rows
    l_alpha = -(la * ((logp.detach() + te).sum() / n_rows)).sum()
    stats.update({"loss_pi": l_pi, "loss_alpha": l_alpha, "target": y.sum() / n_rows, "log_prob": logp.detach().sum() / n_rows,
                  "next_log_prob": next_logp.sum() / n_rows})
    g_c, = torch.autograd.grad(l_q, [cp])
    g_a, = torch.autograd.grad(l_pi, [p])
    g_l, = torch.autograd.grad(l_alpha, [la])
    out = {f"actor.{i}": t for i, t in enumerate(pol.unpack(g_a.detach().cpu().double()))}
    for c in range(cp.shape[0]):
        out.update({f"critic{c}.{i}": t for i, t in enumerate(critic.unpack(g_c[c].detach().cpu().double()))})
    out["log_alpha"] = g_l.detach().cpu().double()
    out.update({k: v.detach().cpu().double() for k, v in stats.items()})
    return out


SAC_KEYS = ("grad_params", "grad_critic_params", "grad_log_alpha", "target", "q", "action", "log_prob", "next_log_prob", "eps", "next_eps",
            "mean", "log_std", "stats")


@pytest.mark.parametrize("M,wg", SHAPES)
def test_sac_gradient_with_discounts_weights_and_td_error(env, oracle_mod, M, wg):
    import torch
    case = _sac_case(M, wg)
    b = SH.case_data(torch, oracle_mod, case)
    assert SH.within_cap(case, b)
    pol, critic, data, rows, idx, mark = b["pol"], b["critic"], b["data"], b["rows"], b["idx"], b["mark"]
    n, dev, keep = data["obs"].shape[0], env.device, ~mark
    disc, w = _extras(torch, n, M, M + 1)
    plain = _sac_call(env, b, rows, wg)
    neutral = _sac_call(env, b, rows, wg, extra={"discount": torch.full((n,), SH.GAMMA, device=dev)}, weights=torch.ones(M, device=dev),
                        return_td_error=True)
    _bits_equal(torch, plain, neutral, SAC_KEYS)
    got = _sac_call(env, b, rows, wg, extra={"discount": disc.to(dev)}, weights=w.to(dev), return_td_error=True)
    torch.cuda.synchronize()
    assert int(got["stats"]["rows_skipped"]) == int(mark.sum()) and int(got["stats"]["rows_used"]) == M - int(mark.sum())
    eps, neps = got["eps"].cpu()[keep], got["next_eps"].cpu()[keep]
    ref = _sac_autograd_w(torch, pol, critic, data, idx[keep], eps, neps, disc, w[keep], torch.float64, "cpu", M)
    yard = _sac_autograd_w(torch, pol, critic, data, idx[keep], eps, neps, disc, w[keep], torch.float32, dev, M)
    ker = {f"actor.{i}": t for i, t in enumerate(pol.unpack(got["grad_params"].cpu().double()))}
    for c in range(2):
        ker.update({f"critic{c}.{i}": t for i, t in enumerate(critic.unpack(got["grad_critic_params"][c].cpu().double()))})
    ker["log_alpha"] = got["grad_log_alpha"].cpu().double()
    ker.update({k: got["stats"][k].cpu().double() for k in ("loss_q0", "loss_q1", "q0", "q1", "loss_pi", "loss_alpha", "target", "log_prob",
                                                           "next_log_prob")})
    assert set(ref) == set(ker)
    _within(ref, yard, ker, f"sac M={M} wg={wg}")
    assert not torch.equal(got["grad_critic_params"], plain["grad_critic_params"]) and not torch.equal(got["target"], plain["target"])
    # the actor's and the temperature's losses are unweighted: with the plain discount their gradients keep the plain call's bits
    only_w = _sac_call(env, b, rows, wg, weights=w.to(dev))
    _bits_equal(torch, plain, only_w, ("grad_params", "grad_log_alpha", "target", "q"))
    assert np.array_equal(got["td_error"].cpu().numpy().view(np.uint32), _td_of(got).view(np.uint32))
    assert not got["td_error"].cpu()[mark].any()
    off = torch.zeros(M, dtype=torch.bool)
    off[[0, M // 2, M - 1]] = True
    w0 = torch.where(off, torch.zeros(()), w)
    r_off = (idx.to(torch.int32) if rows is None else rows.to(torch.int32)).clone()
    r_off[off] = -1
    zero = _sac_call(env, b, rows, wg, extra={"discount": disc.to(dev)}, weights=w0.to(dev), return_td_error=True)
    skip = _sac_call(env, b, r_off, wg, extra={"discount": disc.to(dev)}, weights=w0.to(dev), return_td_error=True)
    torch.cuda.synchronize()
    assert torch.equal(zero["grad_critic_params"], skip["grad_critic_params"])   # (values: a -0.0 may stand where the other has +0.0)
    assert torch.equal(zero["grad_params"].view(torch.int32), got["grad_params"].view(torch.int32))
    td = skip["td_error"].cpu()
    assert not td[off | mark].any() and bool((td[~(off | mark)] > 0).all())
    assert np.array_equal(td.numpy().view(np.uint32), _td_of(skip).view(np.uint32))
