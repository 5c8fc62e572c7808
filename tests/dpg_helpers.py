"""The torch yardstick of the rsx_task_dpg_gradient tests: the TD3 / DDPG losses of include/rsx.h on MLPPolicy.forward and
MLPQCritic.forward in a chosen dtype, torch autograd on them, and the synthetic transitions of the GPU test with its kink filter (host
tensors only: the CPU build test checks the same functions and the same seeds)."""
import numpy as np

KINK = 1e-5
FLOAT_STATS = ("loss_q0", "loss_q1", "q0", "q1", "loss_pi", "target", "abs_next_action")
ROW_KEYS = ("obs", "actions", "reward", "next_obs", "terminated")


def targets(torch, pol, critic, tp, tcp, next_obs, reward, terminated, noise, gamma, dtype):
    """(y, a') of include/rsx.h; ``noise`` is the clamped sigma * eps as added, or None"""
    a = pol.forward(next_obs, tp, dtype=dtype)
    if noise is not None:
        a = (a + noise.to(dtype)).clamp(-1.0, 1.0)
    q = critic.forward(next_obs, a, tcp[0], dtype=dtype)[..., 0]
    for c in range(1, tcp.shape[0]):
        q = torch.minimum(q, critic.forward(next_obs, a, tcp[c], dtype=dtype)[..., 0])
    r = reward.to(dtype)
    return torch.where(terminated.bool(), r, r + gamma * q), a


def losses(torch, pol, critic, p, tp, cp, tcp, rows_of, noise, gamma, dtype, n_rows):
    """(L_q, L_pi, stats) on the gathered rows ``rows_of`` (a dict of ROW_KEYS); means are sums divided by n_rows"""
    x, a = rows_of["obs"].to(dtype), rows_of["actions"].to(dtype)
    with torch.no_grad():
        y, a_next = targets(torch, pol, critic, tp, tcp, rows_of["next_obs"].to(dtype), rows_of["reward"], rows_of["terminated"], noise, gamma, dtype)
    stats, l_q = {}, 0.0
    for c in range(cp.shape[0]):
        q = critic.forward(x, a, cp[c], dtype=dtype)[..., 0]
        stats[f"loss_q{c}"] = 0.5 * ((q - y) ** 2).sum() / n_rows
        stats[f"q{c}"] = q.sum() / n_rows
        l_q = l_q + stats[f"loss_q{c}"]
    l_pi = -critic.forward(x, pol.forward(x, p, dtype=dtype), cp[0].detach(), dtype=dtype)[..., 0].sum() / n_rows
    stats["loss_pi"] = l_pi
    stats["target"] = y.sum() / n_rows
    stats["abs_next_action"] = a_next.abs().sum() / n_rows / pol.act_dim
    return l_q, l_pi, stats


def autograd(torch, pol, critic, data, idx, noise, gamma, dtype, device, n_rows=None):
    """{name: tensor} of the gradients per parameter tensor (each layer's W and b of the actor and of each critic) and the float stats"""
    p = data["params"].to(device=device, dtype=dtype).requires_grad_(True)
    cp = data["cparams"].to(device=device, dtype=dtype).requires_grad_(True)
    tp, tcp = data["tparams"].to(device=device, dtype=dtype), data["tcparams"].to(device=device, dtype=dtype)
    idx = idx.to(device).long()
    rows_of = {k: data[k].to(device)[idx] for k in ROW_KEYS}
    l_q, l_pi, stats = losses(torch, pol, critic, p, tp, cp, tcp, rows_of, None if noise is None else noise.to(device), gamma, dtype,
                              len(idx) if n_rows is None else n_rows)
    g_c, = torch.autograd.grad(l_q, [cp])
    g_a, = torch.autograd.grad(l_pi, [p])
    out = {f"actor.{i}": t for i, t in enumerate(pol.unpack(g_a.detach().cpu().double()))}
    for c in range(cp.shape[0]):
        out.update({f"critic{c}.{i}": t for i, t in enumerate(critic.unpack(g_c[c].detach().cpu().double()))})
    out.update({k: v.detach().cpu().double() for k, v in stats.items()})
    return out


def init(torch, net, gen, out_scale=1.0):
    """flat float32 parameters of torch.nn.Linear's own initialisation, the output layer scaled by ``out_scale``"""
    ts = []
    for s in net.shapes:
        if len(s) == 2:
            bound = 1.0 / np.sqrt(s[1])
        ts.append((torch.rand(s, generator=gen, dtype=torch.float64) * 2 - 1) * bound)
    ts[-1], ts[-2] = ts[-1] * out_scale, ts[-2] * out_scale
    return net.pack(ts)


def _near_relu(torch, net, flat, x):
    """[n] bool: a hidden pre-activation of relu network ``net`` on input rows x (float64) lies within KINK of 0"""
    near = torch.zeros(x.shape[0], dtype=torch.bool)
    if net.hidden_act != "relu":
        return near
    ts = [t.double() for t in net.unpack(flat)]
    for li in range(len(ts) // 2 - 1):
        pre = x @ ts[2 * li].T + ts[2 * li + 1]
        near |= (pre.abs() < KINK).any(-1)
        x = torch.relu(pre)
    return near


def make_data(torch, pol, critic, n_critics, n, seed):
    """N <= n transitions and the parameters of the update: live parameters and targets 0.02 apart; a clip actor's output layer is
    scaled up so that a share of its means lies outside [-1, 1].  Rows within KINK, in float64, of a kink on a differentiated path (a relu
    pre-activation at 0 in the actor on obs, a critic on (obs, action) or critic 0 on (obs, pi(obs)); a clip actor's |mean| = 1) are taken
    out before anything is computed.  Returns (data, removed)."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)   # noqa: E731
    uni = lambda *s: (torch.rand(*s, generator=gen, dtype=torch.float64) * 2 - 1)   # noqa: E731
    p0 = init(torch, pol, gen, out_scale=(10.0 if pol.hidden_act == "relu" else 4.0) if pol.out_act == "clip" else 1.0)
    c0 = torch.stack([init(torch, critic, gen) for _ in range(n_critics)])
    data = {"params": p0 + 0.02 * rnd(pol.num_params).float(), "tparams": p0,
            "cparams": c0 + 0.02 * rnd(n_critics, critic.num_params).float(), "tcparams": c0}
    obs = uni(n, pol.obs_dim).float()
    act = (pol.forward(obs, p0, dtype=torch.float32) + 0.3 * rnd(n, pol.act_dim).float()).clamp(-1.0, 1.0)
    data.update({"obs": obs, "actions": act, "reward": rnd(n).float(), "next_obs": uni(n, pol.obs_dim).float(),
                 "terminated": torch.rand(n, generator=gen) < 0.15})
    x = obs.double()
    near = _near_relu(torch, pol, data["params"], x)
    pi = pol.forward(x, data["params"], dtype=torch.float64)
    for c in range(n_critics):
        near |= _near_relu(torch, critic, data["cparams"][c], torch.cat([x, act.double()], -1))
    near |= _near_relu(torch, critic, data["cparams"][0], torch.cat([x, pi], -1))
    if pol.out_act == "clip":
        import copy
        pre = copy.copy(pol)
        hid = pol._torch_acts()[0]
        pre._torch_acts = lambda: (hid, (lambda v: v))
        mean = pre.forward(x, data["params"], dtype=torch.float64)
        near |= ((mean.abs() - 1.0).abs() < KINK).any(-1)
    removed = int(near.sum())
    keep = ~near
    for k in ROW_KEYS:
        data[k] = data[k][keep].contiguous()
    return data, removed


def make_rows(torch, mode, m, n, seed):
    gen = torch.Generator().manual_seed(seed + 1000)
    if mode == "none":
        return None
    if mode == "perm":
        return torch.randperm(n, generator=gen)[:m].to(torch.int32)
    return torch.randint(0, n, (m,), generator=gen).to(torch.int64)   # repeats (int64: converted by the method)


# ---- the cases of the gradient test: (OD, AD) -> the env that has it; about 15 drawn from the issue's grid ----
ENVS = {(40, 2): "VecVSSEnv", (21, 4): "VecSSLDribblingEnv", (14, 5): "VecSSLContestedPossessionEnv", (64, 2): "VecVSS5v5"}
# (OD, AD), hidden, layers, hidden_act, out_act, C, M, rows, max_workgroups, sigma
CASES = [
    ((40, 2), 64, 2, "tanh", "tanh", 2, 4097, "perm", None, 0.2),
    ((40, 2), 64, 2, "relu", "clip", 2, 4097, "repeats", 2, 0.2),
    ((40, 2), 64, 1, "tanh", "tanh", 1, 65, "none", 1, 0.0),
    ((40, 2), 32, 2, "tanh", "clip", 2, 64, "perm", 2, 0.2),
    ((40, 2), 32, 1, "relu", "tanh", 1, 63, "repeats", None, 0.2),
    ((40, 2), 64, 2, "tanh", "clip", 2, 1, "perm", 1, 0.0),
    ((21, 4), 64, 2, "tanh", "clip", 2, 4097, "none", 2, 0.2),
    ((21, 4), 32, 2, "relu", "tanh", 1, 65, "perm", 1, 0.2),
    ((21, 4), 64, 1, "tanh", "tanh", 2, 64, "repeats", 2, 0.0),
    ((14, 5), 64, 1, "relu", "clip", 2, 4097, "repeats", None, 0.2),
    ((14, 5), 32, 2, "tanh", "tanh", 1, 1, "none", None, 0.2),
    ((14, 5), 32, 1, "tanh", "clip", 2, 63, "perm", 2, 0.0),
    ((64, 2), 64, 2, "tanh", "tanh", 2, 4097, "perm", 2, 0.2),
    ((64, 2), 64, 2, "relu", "tanh", 1, 65, "repeats", None, 0.2),
    ((64, 2), 32, 1, "tanh", "clip", 2, 63, "none", 1, 0.2),
]
GAMMA, NOISE_CLIP = 0.97, 0.1


def case_seed(case):
    """the case's seed; the constant was chosen among 11 .. 15 as the one for which the float64 reference's kink filter removes the
    fewest rows (at most 1.5 % in every case): a property of the reference alone, asserted without a GPU in tests/test_dpg_build.py"""
    (od, ad), hidden, layers, _, _, C, M, _, _, _ = case
    return 15 + M + hidden + layers + od + 3 * C


def case_nets(case):
    from rsoccer_amd.vec.policy import MLPPolicy, MLPQCritic
    (od, ad), hidden, layers, act, out_act = case[:5]
    return (MLPPolicy(od, ad, hidden=hidden, layers=layers, hidden_act=act, out_act=out_act),
            MLPQCritic(od, ad, hidden=hidden, layers=layers, hidden_act=act))


def case_data(torch, case):
    """(pol, critic, data, removed, n) of a case: n = M + 64 + M // 10 rows before the filter, so that at least M are left"""
    pol, critic = case_nets(case)
    n = case[6] + 64 + case[6] // 10
    data, removed = make_data(torch, pol, critic, case[5], n, case_seed(case))
    return pol, critic, data, removed, n
