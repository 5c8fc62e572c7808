"""The PPO update phase on the device (VecFusedEnv.normalize_advantages / minibatch_rows / ppo_update, PPOOptimizer): the permutation
against its numpy restatement bit for bit, the normalisation and clip + Adam against float64 with torch's float32 as the yardstick (and
against their restatements bit for bit), ppo_update against the sequence of public pieces bit for bit, the KL stop, a captured
collect + ppo_update against an eager twin, the optimiser's state dict, and the refusals."""
import numpy as np
import pytest

import ppo_update_helpers as H

pytestmark = pytest.mark.gpu

HALF_LOG_2PI = 0.9189385332046727


@pytest.fixture(scope="module")
def env():
    """never reset, never stepped: the calls need only its device, obs_dim (40) and act_dim (2)"""
    from rsoccer_amd import vec
    e = vec.VecVSSEnv(16, device=0, seed=3)
    yield e
    e.close()


def _nets(obs_dim=40, act_dim=2, hidden=64, layers=2):
    from rsoccer_amd.vec.policy import MLPCritic, MLPPolicy
    return (MLPPolicy(obs_dim, act_dim, hidden=hidden, layers=layers, hidden_act="tanh", out_act="clip"),
            MLPCritic(obs_dim, hidden=hidden, layers=layers, hidden_act="tanh"))


def _params(torch, pol, critic, seed, dev):
    """torch.nn.Linear's own initialisation, as the example's networks have it"""
    torch.manual_seed(seed)

    def seq(net, out):
        dims = [net.obs_dim] + [net.hidden] * net.layers
        mods = []
        for a, b in zip(dims, dims[1:]):
            mods += [torch.nn.Linear(a, b), torch.nn.Tanh()]
        return torch.nn.Sequential(*mods, torch.nn.Linear(net.hidden, out))
    return (pol.from_module(seq(pol, pol.act_dim)).to(dev), torch.full((pol.act_dim,), -0.5, device=dev),
            critic.from_module(seq(critic, 1)).to(dev))


def _batch(torch, env, pol, critic, params, T, B, seed, lp_noise=0.05):
    """a synthetic [T, B] batch whose samples and old log-densities belong to `params` (ratio near 1, like a collected one)"""
    dev = env.device
    p, ls, cp = params
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)   # noqa: E731
    batch = {"obs": (0.5 * r(T, B, pol.obs_dim)).to(dev), "sample": torch.zeros(T, B, pol.act_dim, device=dev),
             "log_prob": torch.zeros(T, B, device=dev), "advantage": (2.0 * r(T, B) + 0.3).to(dev), "return": r(T, B).to(dev)}
    mean = env.ppo_gradient(batch, pol, p, ls, critic, cp, return_forward=True)["mean"].reshape(T, B, pol.act_dim)
    eps = r(T, B, pol.act_dim).to(dev)
    batch["sample"] = (mean + ls.exp() * eps).contiguous()
    z = (batch["sample"] - mean) / ls.exp()
    batch["log_prob"] = ((-0.5 * z * z - ls - HALF_LOG_2PI).sum(-1) + lp_noise * r(T, B).to(dev)).contiguous()
    return batch


def _bits(t):
    return t.detach().clone().contiguous().view(torch_int(t))


def torch_int(t):
    import torch
    return {4: torch.int32, 8: torch.int64}[t.element_size()]


def _rel(x, ref):
    scale = float(ref.abs().max())
    err = float((x.double().cpu() - ref.double().cpu()).abs().max())
    if scale == 0.0:
        assert err == 0.0, "the reference is exactly zero, the result is not"
        return 0.0
    return err / scale


# ---- 1. the permutation ----
@pytest.mark.parametrize("n", [1, 64, 65, 1025])
def test_the_permutation_equals_its_numpy_restatement_bit_for_bit(env, n):
    import torch
    from rsoccer_amd.vec.optim import PPOOptimizer
    for seed, update, epoch in ((0, 0, 0), (0x1234567890ABCDEF, 7, 3), (2 ** 64 - 1, 2 ** 31 + 5, 2 ** 32 - 1)):
        rows = env.minibatch_rows(n, seed, update, epoch)
        torch.cuda.synchronize()
        assert rows.dtype == torch.int32 and tuple(rows.shape) == (n,)
        assert np.array_equal(rows.cpu().numpy().astype(np.int64), H.permutation(n, seed, update, epoch)), (n, seed, update, epoch)
    # the update count taken from an optimiser's device counters
    opt = PPOOptimizer(*_nets(), device=env.device)
    opt.counters[1] = 5
    rows = env.minibatch_rows(n, 42, opt, 1)
    torch.cuda.synchronize()
    assert np.array_equal(rows.cpu().numpy().astype(np.int64), H.permutation(n, 42, 5, 1))
    if n > 1:
        parts = env.minibatch_rows(n, 42, opt, 1, minibatches=2)
        assert [int(p.shape[0]) for p in parts] == [hi - lo for lo, hi in H.chunks(n, 2)]
        assert torch.equal(torch.cat(parts), rows)


# ---- 2. the normalisation ----
@pytest.mark.parametrize("shape", [(5, 13), (17, 241)])
def test_normalised_advantages_stay_within_4x_of_torchs_float32_error(env, shape):
    """Criterion (the issue's, ppo_gradient's): the error against float64 is at most 4x the error of torch's float32
    (adv - adv.mean()) / (adv.std() + eps) on the device against the same float64 value."""
    import torch
    n = shape[0] * shape[1]
    assert n in (65, 4097)
    gen = torch.Generator().manual_seed(n)
    adv = (3.0 * torch.randn(shape, generator=gen) + 1.5).to(env.device)
    a64 = adv.double().cpu()
    ref = (a64 - a64.mean()) / (a64.std() + 1e-8)
    yard = (adv - adv.mean()) / (adv.std() + 1e-8)
    got, ms = env.normalize_advantages(adv, return_moments=True)
    again = env.normalize_advantages(adv)
    torch.cuda.synchronize()
    assert got.shape == adv.shape and got.dtype == torch.float32
    e_yard, e_got = _rel(yard, ref), _rel(got, ref)
    print(f"n = {n}: torch f32 {e_yard:.3e}, kernel {e_got:.3e}, ratio {e_got / e_yard:.2f}")
    assert e_yard > 0.0 and e_got <= 4.0 * e_yard, (e_got, e_yard)
    assert abs(float(ms[0]) - float(a64.mean())) <= 1e-6 and abs(float(ms[1]) - float(a64.std())) <= 1e-6
    assert torch.equal(_bits(got), _bits(again)), "two runs differ"
    # the arithmetic of include/rsx.h, restated on the host
    want, mean, std = H.normalize(adv.cpu().numpy())
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(ms.cpu().numpy().view(np.int32), np.array([mean, std], dtype=np.float32).view(np.int32))


# ---- 3. clip + Adam ----
ADAM_CASES = [("vss", 40, 2, 64, 2, 1.0), ("vss", 40, 2, 64, 2, 1e-5), ("small", 14, 5, 32, 1, 1.0), ("small", 14, 5, 32, 1, 1e-5)]


@pytest.mark.parametrize("name,obs_dim,act_dim,hidden,layers,gscale", ADAM_CASES)
def test_clip_and_adam_stay_within_4x_of_torchs_float32_error(env, name, obs_dim, act_dim, hidden, layers, gscale):
    """Five successive steps with random gradients.  Criterion (the issue's, ppo_gradient's): after every step — the first, where the
    bias correction is the sensitive part, included — the relative error of every parameter, m and v tensor against a float64
    clip_grad_norm_ + Adam is at most 4x the LARGEST relative error any tensor of torch's float32 clip_grad_norm_ + Adam on the device
    shows at that step.  gscale 1.0: the norm is far above max_norm (the clip acts); 1e-5: far below it."""
    import torch
    from rsoccer_amd.vec.optim import PPOOptimizer
    dev = env.device
    pol, critic = _nets(obs_dim, act_dim, hidden, layers)
    sizes = (pol.num_params, act_dim, critic.num_params)
    assert sizes == ({"vss": (6914, 2, 6849), "small": (645, 5, 513)}[name])
    LR, MAXN = 3e-3, 0.5
    opt = PPOOptimizer(pol, critic, device=dev, lr=LR, max_grad_norm=MAXN)
    mine = list(_params(torch, pol, critic, 11, dev))
    t32 = [torch.nn.Parameter(x.clone()) for x in mine]
    t64 = [torch.nn.Parameter(x.double().cpu()) for x in mine]
    o32, o64 = torch.optim.Adam(t32, lr=LR), torch.optim.Adam(t64, lr=LR)
    host = [[x.cpu().numpy().copy() for x in mine], [np.zeros(n, np.float32) for n in sizes], [np.zeros(n, np.float32) for n in sizes]]
    gen = torch.Generator().manual_seed(5)
    worst = 0.0
    for step in range(1, 6):
        grads = [gscale * torch.randn(n, generator=gen) for n in sizes]
        for x, g in zip(t32, grads):
            x.grad = g.to(dev)
        for x, g in zip(t64, grads):
            x.grad = g.double()
        n32 = torch.nn.utils.clip_grad_norm_(t32, MAXN)
        n64 = torch.nn.utils.clip_grad_norm_(t64, MAXN)
        o32.step(), o64.step()
        out = opt.step(*mine, *[g.to(dev) for g in grads])
        torch.cuda.synchronize()
        assert (float(n64) > MAXN) == (gscale == 1.0)
        assert float(out["applied"]) == 1.0 and abs(float(out["grad_norm"]) - float(n64)) <= 4.0 * max(abs(float(n32) - float(n64)), 2.0 ** -24 * float(n64))
        assert opt.counters.tolist() == [step, 0, step, 0]
        ref = {"p": [x.detach() for x in t64], "m": [o64.state[x]["exp_avg"] for x in t64], "v": [o64.state[x]["exp_avg_sq"] for x in t64]}
        yard = {"p": [x.detach() for x in t32], "m": [o32.state[x]["exp_avg"] for x in t32], "v": [o32.state[x]["exp_avg_sq"] for x in t32]}
        ker = {"p": mine, "m": opt.m, "v": opt.v}
        e_yard = {(k, i): _rel(yard[k][i], ref[k][i]) for k in ref for i in range(3)}
        e_ker = {(k, i): _rel(ker[k][i], ref[k][i]) for k in ref for i in range(3)}
        pooled = max(e_yard.values())
        w = max(e_ker, key=e_ker.get)
        worst = max(worst, e_ker[w] / pooled)
        print(f"{name} gscale {gscale} step {step}: torch f32 pooled {pooled:.3e}, kernel worst {e_ker[w]:.3e} {w}, ratio {e_ker[w] / pooled:.2f}")
        assert pooled > 0.0
        for k in e_ker:
            assert e_ker[k] <= 4.0 * pooled, (step, k, e_ker[k], pooled)
        # the arithmetic of include/rsx.h, restated on the host
        P, M, V, norm = H.clip_adam(host[0], [g.numpy() for g in grads], host[1], host[2], step, LR, max_norm=MAXN)
        host = [P, M, V]
        for k, want in (("p", P), ("m", M), ("v", V)):
            for i in range(3):
                assert np.array_equal(ker[k][i].cpu().numpy().view(np.int32), want[i].view(np.int32)), (step, k, i)
        assert np.float32(float(out["grad_norm"])) == norm
    print(f"{name} gscale {gscale}: worst ratio over the five steps {worst:.2f}")


def test_a_zero_gradient_entry_leaves_its_parameter_unchanged_and_lr_dev_equals_lr_by_value(env):
    import torch
    from rsoccer_amd.vec.optim import PPOOptimizer
    dev = env.device
    pol, critic = _nets()
    sizes = (pol.num_params, 2, critic.num_params)
    gen = torch.Generator().manual_seed(9)
    grads = [torch.randn(n, generator=gen).to(dev) for n in sizes]
    zeros = [(0, 3), (0, sizes[0] - 1), (1, 1), (2, 0), (2, 300)]
    for i, k in zeros:
        grads[i][k] = 0.0
    grads[0][5] = -0.0
    LR = 1e-2
    runs = []
    for lr in (LR, torch.tensor([LR], dtype=torch.float32, device=dev)):
        opt = PPOOptimizer(pol, critic, device=dev, lr=lr, max_grad_norm=0.5)
        start = list(_params(torch, pol, critic, 21, dev))
        p = [x.clone() for x in start]
        for _ in range(3):
            opt.step(*p, *grads)
        torch.cuda.synchronize()
        runs.append(torch.cat([_bits(x) for x in p + opt.m + opt.v]))
    assert torch.equal(runs[0], runs[1]), "lr_dev and lr by value differ"
    # t = 1 from a fresh state: m = 0 and g = 0 -> the parameter keeps its bits (every step here, as g stays 0), the others move
    for i, k in zeros + [(0, 5)]:
        assert torch.equal(_bits(p[i][k]), _bits(start[i][k])), (i, k)
    moved = torch.cat([(a != b) for a, b in zip(p, start)])
    assert int(moved.sum()) == sum(sizes) - len(zeros) - 1


# ---- 4. composition: ppo_update is the sequence of the public pieces ----
def _piecewise(torch, env, batch, pol, critic, params, opt, epochs, mb, seed, normalize, wg, target_kl=None, host_stop=False, **loss):
    """the update as calls of the public pieces; with host_stop the KL stop is decided on the HOST from each minibatch's approx_kl
    (steps after the first minibatch over the target are not taken).  Returns (stats rows [epochs * mb, 8], index of the stop or None)"""
    p, ls, cp = params
    T, B = batch["obs"].shape[:2]
    opt.begin_update()
    adv = env.normalize_advantages(batch["advantage"]) if normalize else batch["advantage"]
    rows_out, stop = [], None
    for e in range(epochs):
        for chunk in env.minibatch_rows(T * B, seed, opt, e, minibatches=mb):
            out = env.ppo_gradient(batch, pol, p, ls, critic, cp, rows=chunk, advantage=adv, max_workgroups=wg, **loss)
            rows_out.append(torch.stack([out["stats"][k] for k in out["stats"]]))
            if host_stop:
                if stop is None and float(out["stats"]["approx_kl"]) > target_kl:
                    stop = len(rows_out) - 1
                if stop is not None:
                    continue
            opt.step(p, ls, cp, out["grad_params"], out["grad_log_std"], out["grad_critic_params"])
    opt.end_update()
    return torch.stack(rows_out), stop


def _state_bits(torch, params, opt):
    return torch.cat([_bits(x) for x in list(params) + opt.m + opt.v])


@pytest.mark.parametrize("T,B,mb", [(5, 13, 2), (25, 41, 4)])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("wg", [1, None])
def test_ppo_update_equals_the_sequence_of_public_pieces_bit_for_bit(env, T, B, mb, normalize, wg):
    import torch
    from rsoccer_amd.vec.optim import PPOOptimizer
    dev = env.device
    pol, critic = _nets()
    start = _params(torch, pol, critic, 31, dev)
    batch = _batch(torch, env, pol, critic, start, T, B, seed=T * B)
    before = {k: v.clone() for k, v in batch.items()}
    loss = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01)
    EPOCHS, SEED = 2, 77
    chunks = H.chunks(T * B, mb)
    assert [hi - lo for lo, hi in chunks] == {65: [33, 32], 1025: [257, 257, 257, 254]}[T * B]
    a, b = [x.clone() for x in start], [x.clone() for x in start]
    oa, ob = (PPOOptimizer(pol, critic, device=dev, lr=1e-3, max_grad_norm=0.5) for _ in range(2))
    for o in (oa, ob):
        o.counters[1] = 3   # (not the first update of a run)
    out = env.ppo_update(batch, pol, *a[:2], critic, a[2], oa, epochs=EPOCHS, minibatches=mb, normalize_advantage=normalize, seed=SEED,
                         max_workgroups=wg, **loss)
    want, _ = _piecewise(torch, env, batch, pol, critic, b, ob, EPOCHS, mb, SEED, normalize, wg, **loss)
    torch.cuda.synchronize()
    stats = out["stats"]
    assert tuple(stats.shape) == (EPOCHS, mb, 10)
    assert torch.equal(_bits(stats[:, :, :8].reshape(EPOCHS * mb, 8)), _bits(want))
    assert torch.equal(_state_bits(torch, a, oa), _state_bits(torch, b, ob))
    assert oa.counters.tolist() == ob.counters.tolist() == [EPOCHS * mb, 4, EPOCHS * mb, 0]
    assert bool((stats[:, :, 9] == 1.0).all()) and bool((stats[:, :, 8] > 0.0).all())
    assert not torch.equal(_bits(a[0]), _bits(start[0])) and not torch.equal(_bits(a[1]), _bits(start[1])) and not torch.equal(_bits(a[2]), _bits(start[2]))
    # the rows the call leaves are the last epoch's permutation; the batch is not written
    assert np.array_equal(out["rows"].cpu().numpy().astype(np.int64), H.permutation(T * B, SEED, 3, EPOCHS - 1))
    for k in batch:
        assert torch.equal(_bits(batch[k]), _bits(before[k])), k
    for row, (lo, hi) in zip(stats[0], chunks):
        assert int(row[6]) == hi - lo and int(row[7]) == 0


# ---- 5. the KL stop ----
def test_the_kl_stop_withholds_every_later_step_and_the_next_call_steps_again(env):
    import torch
    from rsoccer_amd.vec.optim import PPOOptimizer
    dev = env.device
    pol, critic = _nets()
    start = _params(torch, pol, critic, 41, dev)
    T, B, EPOCHS, MB, SEED, TARGET = 25, 41, 2, 4, 5, 0.01
    batch = _batch(torch, env, pol, critic, start, T, B, seed=8, lp_noise=0.0)
    loss = dict(clip=0.2, vf_coef=0.5, ent_coef=0.0)
    a, b = [x.clone() for x in start], [x.clone() for x in start]
    oa, ob = (PPOOptimizer(pol, critic, device=dev, lr=0.05, max_grad_norm=0.5) for _ in range(2))
    want, stop = _piecewise(torch, env, batch, pol, critic, b, ob, EPOCHS, MB, SEED, True, None, target_kl=TARGET, host_stop=True, **loss)
    print("approx_kl per minibatch of the host-stopped run:", [f"{float(x):.3e}" for x in want[:, 3]], "stop at", stop)
    assert stop is not None and 0 < stop < EPOCHS * MB, "the case would pass vacuously"
    out = env.ppo_update(batch, pol, *a[:2], critic, a[2], oa, epochs=EPOCHS, minibatches=MB, target_kl=TARGET, seed=SEED, **loss)
    torch.cuda.synchronize()
    applied = out["stats"][:, :, 9].reshape(-1).tolist()
    assert applied == [1.0] * stop + [0.0] * (EPOCHS * MB - stop)
    assert torch.equal(_state_bits(torch, a, oa), _state_bits(torch, b, ob))
    assert oa.counters.tolist() == [stop, 1, stop, 1] and ob.counters.tolist()[:2] == [stop, 1]
    assert torch.equal(_bits(out["stats"][:, :, :8].reshape(-1, 8)), _bits(want))   # (the withheld minibatches still ran, on the stopped parameters)
    # the flag is cleared when the next call starts: it applies steps again
    again = env.ppo_update(batch, pol, *a[:2], critic, a[2], oa, epochs=1, minibatches=MB, target_kl=None, seed=SEED, **loss)
    torch.cuda.synchronize()
    assert again["stats"][:, :, 9].reshape(-1).tolist() == [1.0] * MB
    assert oa.counters.tolist() == [stop + MB, 2, MB, 0]
    assert not torch.equal(_state_bits(torch, a, oa), _state_bits(torch, b, ob))


# ---- 6. one graph replay is one PPO iteration ----
def test_a_captured_collect_and_ppo_update_replays_as_an_eager_twins_iterations():
    import torch
    from rsoccer_amd import vec
    from rsoccer_amd.vec.optim import PPOOptimizer
    T, EPOCHS, MB = 8, 2, 2
    envs = [vec.VecVSSEnv(64, device=0, seed=17, max_episode_steps=20) for _ in range(2)]
    for e in envs:
        e.reset()
        e.enable_graph_capture()
    env, twin = envs
    dev = env.device
    pol, critic = _nets()
    start = _params(torch, pol, critic, 51, dev)
    sides = []
    for e in envs:
        sides.append(([x.clone() for x in start], PPOOptimizer(pol, critic, device=dev, lr=1e-3, max_grad_norm=0.5)))

    def iteration(e, params, opt):
        p, ls, cp = params
        batch = e.collect(pol, p, T, log_std=ls, noise_seed=99, critic=critic, critic_params=cp)
        return e.ppo_update(batch, pol, p, ls, critic, cp, opt, epochs=EPOCHS, minibatches=MB, seed=123)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # one eager iteration, which is also torch's warm-up before a capture
        first = iteration(env, *sides[0])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    seen = [(first["stats"].clone(), first["rows"].clone())]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = iteration(env, *sides[0])
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        seen.append((out["stats"].clone(), out["rows"].clone()))
    want = []
    for _ in range(4):
        o = iteration(twin, *sides[1])
        torch.cuda.synchronize()
        want.append((o["stats"].clone(), o["rows"].clone()))
    for i, ((s, r), (ws, wr)) in enumerate(zip(seen, want)):
        assert torch.equal(_bits(s), _bits(ws)), ("stats", i)
        assert torch.equal(r, wr), ("rows", i)
    assert torch.equal(_state_bits(torch, *sides[0]), _state_bits(torch, *sides[1]))
    assert sides[0][1].counters.tolist() == sides[1][1].counters.tolist() == [4 * EPOCHS * MB, 4, EPOCHS * MB, 0]
    assert np.array_equal(env.checkpoint(), twin.checkpoint())
    # every replay drew its own permutation: the update count on the device keys it
    N = T * 64
    for i, (_, r) in enumerate(seen):
        assert np.array_equal(r.cpu().numpy().astype(np.int64), H.permutation(N, 123, i, EPOCHS - 1)), i
    for i in range(1, 4):
        assert not torch.equal(seen[i][1], seen[i - 1][1])
    for e in envs:
        e.close()


# ---- 7. the optimiser's state dict ----
def test_a_state_dict_round_trip_continues_with_equal_bits(env):
    import torch
    from rsoccer_amd.vec.optim import PPOOptimizer
    dev = env.device
    pol, critic = _nets()
    start = _params(torch, pol, critic, 61, dev)
    batch = _batch(torch, env, pol, critic, start, 5, 13, seed=3)
    kw = dict(epochs=1, minibatches=2, seed=9)

    def make():
        return PPOOptimizer(pol, critic, device=dev, lr=2e-3, betas=(0.8, 0.99), eps=1e-7, max_grad_norm=0.3)
    a, oa = [x.clone() for x in start], make()
    for _ in range(4):
        env.ppo_update(batch, pol, *a[:2], critic, a[2], oa, **kw)
    b, ob = [x.clone() for x in start], make()
    for _ in range(2):
        env.ppo_update(batch, pol, *b[:2], critic, b[2], ob, **kw)
    sd = ob.state_dict()
    saved = [x.clone() for x in b]
    env.ppo_update(batch, pol, *b[:2], critic, b[2], ob, **kw)   # (the saved state is a copy: going on does not change it)
    oc = PPOOptimizer(pol, critic, device=dev)   # other hyper-parameters: the state dict carries them
    oc.load_state_dict(sd)
    assert oc.counters.tolist() == [4, 2, 2, 0] and oc.betas == (0.8, 0.99) and oc.eps == 1e-7 and oc.max_grad_norm == 0.3 and oc.lr == 2e-3
    for _ in range(2):
        env.ppo_update(batch, pol, *saved[:2], critic, saved[2], oc, **kw)
    torch.cuda.synchronize()
    assert torch.equal(_state_bits(torch, a, oa), _state_bits(torch, saved, oc))
    assert oa.counters.tolist() == oc.counters.tolist() == [8, 4, 2, 0]
    with pytest.raises(ValueError, match=r"m\[0\]"):
        oc.load_state_dict({**sd, "m": [sd["m"][0][:-1], sd["m"][1], sd["m"][2]]})
    with pytest.raises(ValueError, match="counters"):
        oc.load_state_dict({"m": sd["m"], "v": sd["v"]})


# ---- 8. refusals: a ValueError naming the offender, or RSX_ERR_ARG, and nothing is enqueued ----
def test_refusals_change_nothing(env):
    import torch
    from rsoccer_amd import _lib
    from rsoccer_amd.vec.optim import PPOOptimizer
    dev = env.device
    pol, critic = _nets()
    start = _params(torch, pol, critic, 71, dev)
    batch = _batch(torch, env, pol, critic, start, 5, 13, seed=4)
    p = [x.clone() for x in start]
    opt = PPOOptimizer(pol, critic, device=dev)
    ok = dict(epochs=1, minibatches=2)

    def call(o=opt, **kw):
        return env.ppo_update(batch, pol, *p[:2], critic, p[2], o, **{**ok, **kw})
    for kw, word in ((dict(epochs=0), "epochs"), (dict(minibatches=0), "minibatches"), (dict(minibatches=64), "minibatches"),
                     (dict(target_kl=float("nan")), "target_kl"), (dict(target_kl=-1.0), "target_kl"), (dict(target_kl=0.0), "target_kl"),
                     (dict(clip=1.5), "clip"), (dict(vf_coef=float("inf")), "vf_coef"), (dict(max_workgroups=0), "max_workgroups")):
        with pytest.raises(ValueError, match=word):
            call(**kw)
    small = PPOOptimizer(*_nets(40, 2, 32, 1), device=dev)
    with pytest.raises(ValueError, match="state tensors"):
        call(o=small)
    with pytest.raises(ValueError, match="opt must be"):
        call(o=torch.optim.Adam([torch.nn.Parameter(p[0].clone())]))
    with pytest.raises(ValueError, match="at least 2"):
        env.normalize_advantages(torch.zeros(1, device=dev))
    with pytest.raises(ValueError, match="float32"):
        env.normalize_advantages(torch.zeros(4, device=dev, dtype=torch.float64))
    with pytest.raises(ValueError, match="n must be"):
        env.minibatch_rows(0, 1, 0, 0)
    with pytest.raises(ValueError, match="epoch"):
        env.minibatch_rows(8, 1, 0, 2 ** 32)
    g = [torch.ones_like(x) for x in p]
    with pytest.raises(ValueError, match="grad_log_std"):
        opt.step(*p, g[0], g[1][:1], g[2])
    with pytest.raises(ValueError, match="lr"):
        opt.step(*p, *g, lr=float("nan"))
    # the C-ABI itself: RSX_ERR_ARG before anything is enqueued
    ws = torch.zeros(256, dtype=torch.float64, device=dev)
    rows = torch.full((8,), -7, dtype=torch.int32, device=dev)
    adv, outn = torch.randn(8, device=dev), torch.full((8,), 5.0, device=dev)
    with torch.cuda.device(dev):
        for bad in (lambda: _lib.ppo_normalize(adv.data_ptr(), 1, 1e-8, outn.data_ptr(), None, ws.data_ptr()),
                    lambda: _lib.ppo_normalize(adv.data_ptr(), 8, float("nan"), outn.data_ptr(), None, ws.data_ptr()),
                    lambda: _lib.ppo_normalize(adv.data_ptr(), 8, 1e-8, None, None, ws.data_ptr()),
                    lambda: _lib.ppo_permutation(rows.data_ptr(), 0, 1, 0, None, 0),
                    lambda: _lib.ppo_permutation(rows.data_ptr(), 2 ** 31, 1, 0, None, 0),
                    lambda: _lib.ppo_permutation(None, 8, 1, 0, None, 0),
                    lambda: _lib.ppo_permutation(rows.data_ptr(), 8, 1, 0, None, -1)):
            with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):
                bad()
        st, io = opt.state(), _lib.AdamIo(*[x.data_ptr() for x in p], *[x.data_ptr() for x in g], None, None, opt._ws.data_ptr())
        for cfg in (_lib.AdamCfg(0.9, 0.999, None, float("nan"), 1e-8, 0.5, 0.0), _lib.AdamCfg(1.0, 0.999, None, 1e-3, 1e-8, 0.5, 0.0),
                    _lib.AdamCfg(0.9, 0.999, None, 1e-3, -1.0, 0.5, 0.0), _lib.AdamCfg(0.9, 0.999, None, 1e-3, 1e-8, float("inf"), 0.0),
                    _lib.AdamCfg(0.9, 0.999, None, 1e-3, 1e-8, 0.5, float("nan"))):
            with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):
                _lib.adam_step(cfg, st, io)
        with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):
            _lib.adam_step(opt.cfg(), st, _lib.AdamIo(p[0].data_ptr(), None, p[2].data_ptr(), *[x.data_ptr() for x in g], None, None, opt._ws.data_ptr()))
    # rsx_task_ppo_update with a state of the wrong sizes, past the Python layer
    nbytes, _ = env.sim.ppo_update_workspace(pol.spec(), critic.spec(), 65, 2, 0)
    wsu, stats = torch.zeros(nbytes // 4 + 1, device=dev), torch.zeros(1, 2, 10, device=dev)
    inp = _lib.PpoIn(batch["obs"].data_ptr(), batch["sample"].data_ptr(), batch["log_prob"].data_ptr(), batch["advantage"].data_ptr(),
                     batch["return"].data_ptr(), None, 65, 65)
    for ucfg, state in ((_lib.PpoUpdateCfg(1, 1, 2, 1, 1e-8), small.state()), (_lib.PpoUpdateCfg(1, 0, 2, 1, 1e-8), opt.state()),
                        (_lib.PpoUpdateCfg(1, 1, 64, 1, 1e-8), opt.state()), (_lib.PpoUpdateCfg(1, 1, 2, 1, float("nan")), opt.state())):
        with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):
            env.sim.task_ppo_update(pol.spec(), p[0].data_ptr(), p[1].data_ptr(), critic.spec(), p[2].data_ptr(), inp,
                                    _lib.PpoCfg(0.2, 0.5, 0.0, 0), ucfg, opt.cfg(), state, stats.data_ptr(), wsu.data_ptr(), env._stream())
    with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):
        env.sim.ppo_update_workspace(pol.spec(), critic.spec(), 65, 64, 0)
    torch.cuda.synchronize()
    for a, b in zip(p, start):
        assert torch.equal(_bits(a), _bits(b))
    assert opt.counters.tolist() == [0, 0, 0, 0] and float(torch.cat(opt.m + opt.v).abs().max()) == 0.0
    assert bool((rows == -7).all()) and bool((outn == 5.0).all()) and float(stats.abs().max()) == 0.0
