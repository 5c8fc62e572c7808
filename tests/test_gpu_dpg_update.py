"""The TD3 / DDPG update phase on the device (ReplayBuffer.sample_rows_device, DPGOptimizer, VecFusedEnv.dpg_update): the row draw and
the two-group clip + Adam + Polyak step against their numpy restatements bit for bit, the optimiser against float64 with torch's float32
as the yardstick, a critic-only step leaving the actor and the targets alone, dpg_update against the sequence of public pieces bit for
bit, a captured collect + add + dpg_update against an eager twin, the optimiser's state dict, the empty ring, and the refusals."""
import numpy as np
import pytest

import dpg_helpers as DH
import dpg_update_helpers as H

pytestmark = pytest.mark.gpu

CAPACITY = 1024
LOSS = dict(gamma=0.97, noise_clip=0.1)


@pytest.fixture(scope="module")
def env():
    from rsoccer_amd import vec
    e = vec.VecVSSEnv(16, device=0, seed=3)
    yield e
    e.close()


def _nets(obs_dim=40, act_dim=2, hidden=64, layers=2):
    from rsoccer_amd.vec.policy import MLPPolicy, MLPQCritic
    return (MLPPolicy(obs_dim, act_dim, hidden=hidden, layers=layers, hidden_act="tanh", out_act="tanh"),
            MLPQCritic(obs_dim, act_dim, hidden=hidden, layers=layers, hidden_act="tanh"))


def _params(torch, pol, crit, C, seed, dev):
    """(actor, its target, critics [C, Pc], their target): torch.nn.Linear's initialisation, live and target 0.02 apart"""
    gen = torch.Generator().manual_seed(seed)
    p0 = DH.init(torch, pol, gen)
    c0 = torch.stack([DH.init(torch, crit, gen) for _ in range(C)])
    p = p0 + 0.02 * torch.randn(pol.num_params, generator=gen)
    c = c0 + 0.02 * torch.randn(C, crit.num_params, generator=gen)
    return [x.float().contiguous().to(dev) for x in (p, p0, c, c0)]


@pytest.fixture(scope="module")
def ring(env):
    """a ring of 1024 rows partly filled by ONE collect of 19 steps on 16 envs (304 rows); read only"""
    import torch
    from rsoccer_amd.vec.replay import ReplayBuffer
    pol, crit = _nets()
    p = _params(torch, pol, crit, 1, 5, env.device)[0]
    env.reset()
    batch = env.collect(pol, p, 19, log_std=torch.full((2,), -1.0, device=env.device), noise_seed=7, return_final_obs=True)
    buf = ReplayBuffer(CAPACITY, 40, 2, env.device)
    assert buf.add(batch) == 304
    torch.cuda.synchronize()
    assert int(buf.fill) == 304 and int(buf.head) == 304
    return buf


def _bits(t):
    import torch
    t = t.detach().clone().contiguous()
    return t.view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[t.element_size()]).reshape(-1)


def _state_bits(torch, P, opt):
    return torch.cat([_bits(x).to(torch.int64) for x in list(P) + opt.m + opt.v + [opt.counters]])


def _rel(x, ref):
    scale = float(ref.abs().max())
    err = float((x.double().cpu() - ref.double().cpu()).abs().max())
    if scale == 0.0:
        assert err == 0.0, "the reference is exactly zero, the result is not"
        return 0.0
    return err / scale


# ---- 1. the rows ----
@pytest.mark.parametrize("m", [1, 3, 4, 5, 257])
def test_the_rows_equal_their_numpy_restatement_bit_for_bit(env, m):
    """m: the word-index boundary (3, 4, 5) and the 256-thread workgroup's (257); fill and step by value and through device tensors"""
    import torch
    from rsoccer_amd import _lib
    from rsoccer_amd.vec.replay import ReplayBuffer
    dev = env.device
    buf = ReplayBuffer(CAPACITY, 40, 2, dev)
    step_t = torch.zeros(1, dtype=torch.int64, device=dev)
    for fill in (1, 3, 1000, CAPACITY):
        for seed, step in ((0, 0), (0x1234567890ABCDEF, 7), (2 ** 64 - 1, 2 ** 40 + 5)):
            want = H.sample_rows(m, fill, seed, step)
            buf.fill[0] = fill
            step_t[0] = step
            by_value = buf.sample_rows_device(m, seed=seed, step=step)
            by_tensor = buf.sample_rows_device(m, seed=seed, step=step_t)
            raw = torch.full((m + 1,), -7, dtype=torch.int32, device=dev)   # the fill by value, and one entry behind the rows
            with torch.cuda.device(dev):
                _lib.replay_sample_rows(raw.data_ptr(), m, CAPACITY, fill, None, seed, step, None, env._stream())
            torch.cuda.synchronize()
            for got in (by_value, by_tensor, raw[:m]):
                assert got.dtype == torch.int32 and tuple(got.shape) == (m,)
                assert np.array_equal(got.cpu().numpy().astype(np.int64), want), (m, fill, seed, step)
            assert int(raw[m]) == -7
    # an empty ring gives -1 everywhere, a fill count above the ring is clamped to it
    buf.fill[0] = 0
    empty = buf.sample_rows_device(m, seed=3, step=1)
    buf.fill[0] = CAPACITY + 4000
    over = buf.sample_rows_device(m, seed=3, step=1)
    buf.fill[0] = -5
    under = buf.sample_rows_device(m, seed=3, step=1)
    torch.cuda.synchronize()
    assert bool((empty == -1).all()) and bool((under == -1).all())
    assert np.array_equal(over.cpu().numpy().astype(np.int64), H.sample_rows(m, CAPACITY, 3, 1))


# ---- 2. the optimiser step against the restatement ----
# "vss": 40-64-64-2 actor, twin 42-64-64-1 critics; "wide": a critic group of 17 410 floats, more than one trip of the norm
# reduction's 64 workgroups of 256 threads covers
OPT_SHAPES = {"vss": (40, 2, 6914, 2 * 6977), "wide": (64, 5, 8645, 17410)}


def _host(P):
    return [x.cpu().numpy().reshape(-1).copy() for x in P]


@pytest.mark.parametrize("shape", ["vss", "wide"])
@pytest.mark.parametrize("max_norm", [0.5, None])
@pytest.mark.parametrize("lr_by", ["value", "tensor"])
def test_optimiser_steps_equal_the_restatement_bit_for_bit(env, shape, max_norm, lr_by):
    """three consecutive steps: critic-only, actor, critic-only; parameters, targets, moments, counters and stats"""
    import torch
    from rsoccer_amd.vec.optim import DPGOptimizer
    dev = env.device
    od, ad, na, nc = OPT_SHAPES[shape]
    pol, crit = _nets(od, ad)
    assert (pol.num_params, 2 * crit.num_params) == (na, nc) and (shape != "wide" or nc > 64 * 256)
    LR_A, LR_C, TAU = 1e-3, 3e-3, 0.05
    lrs = (LR_A, LR_C) if lr_by == "value" else tuple(torch.tensor([v], dtype=torch.float32, device=dev) for v in (LR_A, LR_C))
    opt = DPGOptimizer(pol, crit, 2, device=dev, lr_actor=lrs[0], lr_critic=lrs[1], max_grad_norm=max_norm, tau=TAU)
    P = _params(torch, pol, crit, 2, 11, dev)
    host, st = _host(P), H.fresh_state(na, nc)
    gen = torch.Generator().manual_seed(5)
    for step, actor in enumerate((False, True, False), 1):
        ga, gc = torch.randn(na, generator=gen), torch.randn(2, crit.num_params, generator=gen)
        out = opt.step(*P, ga.to(dev) if actor else None, gc.to(dev))
        torch.cuda.synchronize()
        *host, stats = H.dpg_adam_step(st, *host, ga.numpy() if actor else None, gc.numpy(), LR_A, LR_C, max_norm=max_norm, tau=TAU)
        for name, got, want in zip(("params", "target_params", "critic_params", "target_critic_params"), P, host):
            assert np.array_equal(got.cpu().numpy().reshape(-1).view(np.int32), want.view(np.int32)), (step, name)
        for k, name in enumerate(("actor", "critics")):
            assert np.array_equal(opt.m[k].cpu().numpy().view(np.int32), st["m"][k].view(np.int32)), (step, "m", name)
            assert np.array_equal(opt.v[k].cpu().numpy().view(np.int32), st["v"][k].view(np.int32)), (step, "v", name)
        assert opt.counters.tolist() == st["counters"] == [step, 1 if step >= 2 else 0, step, 0]
        assert int(opt.steps) == step and opt.steps.data_ptr() == opt.counters.data_ptr() + 16
        got = np.array([float(out[k]) for k in ("grad_norm_critic", "grad_norm_actor", "targets_moved")], dtype=np.float32)
        assert np.array_equal(got.view(np.int32), stats.view(np.int32)), (step, got, stats)
        assert stats[0] > 0.5 and (stats[1] > 0.5) == actor and stats[2] == (1.0 if actor else 0.0)   # (the clip binds where there is one)


# ---- 3. the optimiser step against torch ----
def test_three_steps_stay_within_4x_of_torchs_float32_error(env):
    """Criterion (docs/VERIFICATION.md f13): after three steps (critic-only, actor, critic-only) the relative error of every tensor
    against float64 clip_grad_norm_ + Adam + lerp_ is at most 4x the LARGEST relative error any tensor of torch's float32
    clip_grad_norm_ + Adam + lerp_ on the device shows."""
    import torch
    from rsoccer_amd.vec.optim import DPGOptimizer
    dev = env.device
    pol, crit = _nets()
    LR_A, LR_C, TAU, MAXN = 1e-3, 3e-3, 0.05, 0.5
    opt = DPGOptimizer(pol, crit, 2, device=dev, lr_actor=LR_A, lr_critic=LR_C, max_grad_norm=MAXN, tau=TAU)
    P = _params(torch, pol, crit, 2, 13, dev)
    runs = {}
    for dt, where in ((torch.float32, dev), (torch.float64, "cpu")):
        live = [torch.nn.Parameter(P[0].to(where, dt).clone()), torch.nn.Parameter(P[2].to(where, dt).clone())]   # (to() may return P itself)
        runs[dt] = (live, [P[1].to(where, dt).clone(), P[3].to(where, dt).clone()],
                    [torch.optim.Adam([live[0]], lr=LR_A), torch.optim.Adam([live[1]], lr=LR_C)], where)
    gen = torch.Generator().manual_seed(6)
    for actor in (False, True, False):
        ga, gc = torch.randn(pol.num_params, generator=gen), torch.randn(2, crit.num_params, generator=gen)
        for dt, (live, targ, opts, where) in runs.items():
            for k, g in ((0, ga), (1, gc)):
                if k == 0 and not actor:
                    continue
                live[k].grad = g.to(where, dt)
                torch.nn.utils.clip_grad_norm_([live[k]], MAXN)
                opts[k].step()
            if actor:
                with torch.no_grad():
                    for k in (0, 1):
                        targ[k].lerp_(live[k].detach(), TAU)
        opt.step(*P, ga.to(dev) if actor else None, gc.to(dev))
    torch.cuda.synchronize()

    def tensors(dt):
        live, targ, opts, _ = runs[dt]
        return {"params": live[0].detach(), "target_params": targ[0], "critic_params": live[1].detach(), "target_critic_params": targ[1],
                "m_actor": opts[0].state[live[0]]["exp_avg"], "v_actor": opts[0].state[live[0]]["exp_avg_sq"],
                "m_critics": opts[1].state[live[1]]["exp_avg"], "v_critics": opts[1].state[live[1]]["exp_avg_sq"]}
    ref, yard = tensors(torch.float64), tensors(torch.float32)
    ker = {"params": P[0], "target_params": P[1], "critic_params": P[2], "target_critic_params": P[3], "m_actor": opt.m[0], "v_actor": opt.v[0],
           "m_critics": opt.m[1].reshape(2, -1), "v_critics": opt.v[1].reshape(2, -1)}
    pooled = max(_rel(yard[k], ref[k]) for k in ref)
    assert pooled > 0.0
    for k in ref:
        e = _rel(ker[k], ref[k])
        print(f"{k}: kernel {e:.3e}, torch f32 pooled {pooled:.3e}, ratio {e / pooled:.2f}")
        assert e <= 4.0 * pooled, (k, e, pooled)


# ---- 4. a critic-only step ----
def test_a_critic_only_step_leaves_the_actor_and_both_targets_byte_for_byte(env):
    import torch
    from rsoccer_amd.vec.optim import DPGOptimizer
    dev = env.device
    pol, crit = _nets()
    opt = DPGOptimizer(pol, crit, 2, device=dev, max_grad_norm=0.5, tau=0.05)
    P = _params(torch, pol, crit, 2, 17, dev)
    gen = torch.Generator().manual_seed(8)
    ga, gc = torch.randn(pol.num_params, generator=gen).to(dev), torch.randn(2, crit.num_params, generator=gen).to(dev)
    opt.step(*P, ga, gc)   # an actor step first: the actor's moments and t are not zero
    torch.cuda.synchronize()
    keep = [_bits(x) for x in (P[0], P[1], P[3], opt.m[0], opt.v[0])]
    critics, t_actor = _bits(P[2]), int(opt.counters[1])
    out = opt.step(*P, None, gc)
    torch.cuda.synchronize()
    for name, was, now in zip(("params", "target_params", "target_critic_params", "m_actor", "v_actor"), keep, (P[0], P[1], P[3], opt.m[0], opt.v[0])):
        assert torch.equal(was, _bits(now)), name
    assert opt.counters.tolist() == [2, 1, 2, 0] and t_actor == 1
    assert not torch.equal(critics, _bits(P[2])) and float(out["grad_norm_actor"]) == 0.0 and float(out["targets_moved"]) == 0.0
    # update_targets=True without an actor step: both targets move, the actor itself still does not
    opt.step(*P, None, gc, update_targets=True)
    torch.cuda.synchronize()
    assert torch.equal(keep[0], _bits(P[0])) and torch.equal(keep[3], _bits(opt.m[0])) and torch.equal(keep[4], _bits(opt.v[0]))
    assert not torch.equal(keep[1], _bits(P[1])) and not torch.equal(keep[2], _bits(P[3])) and opt.counters.tolist() == [3, 1, 3, 0]
    want = H.polyak(P[0].cpu().numpy(), keep[1].cpu().numpy().view(np.float32), 0.05)
    assert np.array_equal(P[1].cpu().numpy().view(np.int32), want.view(np.int32))


# ---- 5. composition: dpg_update is the sequence of the public pieces ----
def _piecewise(torch, env, buf, pol, crit, P, opt, grad_steps, delay, batch, seed, wg, sigma):
    """the update as calls of the public pieces.  Returns (stats [grad_steps, 12], the last step's rows, each step's target noise)"""
    from rsoccer_amd import _lib
    zero = torch.zeros((), device=env.device)
    rows_out, noises, rows = [], [], None
    for j in range(grad_steps):
        actor = (j + 1) % delay == 0
        rows = buf.sample_rows_device(batch, seed=seed, step=opt.steps)
        out = env.dpg_gradient(buf.data(), pol, P[0], P[1], crit, P[2], P[3], rows=rows, target_noise=sigma, noise_seed=seed,
                               noise_step=opt.steps, actor=actor, max_workgroups=wg, return_rows=True, **LOSS)
        o = opt.step(*P, out["grad_params"] if actor else None, out["grad_critic_params"])
        rows_out.append(torch.stack([out["stats"].get(k, zero) for k in _lib.DPG_STATS] + [o[k] for k in _lib.DPG_ADAM_STATS]))
        noises.append(out["target_noise"])
    return torch.stack(rows_out), rows, noises


@pytest.mark.parametrize("grad_steps,delay,C,sigma", [(4, 2, 2, 0.2), (3, 1, 1, 0.0), (2, 2, 2, 0.2)])
@pytest.mark.parametrize("batch", [63, 65])
@pytest.mark.parametrize("wg", [1, None])
def test_dpg_update_equals_the_sequence_of_public_pieces_bit_for_bit(env, ring, grad_steps, delay, C, sigma, batch, wg):
    import torch
    from rsoccer_amd.vec.optim import DPGOptimizer
    dev = env.device
    pol, crit = _nets()
    start = _params(torch, pol, crit, C, 31, dev)
    before = {k: _bits(v) for k, v in ring.data().items()}
    SEED = 77
    a, b = [x.clone() for x in start], [x.clone() for x in start]
    oa, ob = (DPGOptimizer(pol, crit, C, device=dev, lr_actor=1e-3, lr_critic=2e-3, max_grad_norm=0.5, tau=0.05) for _ in range(2))
    for o in (oa, ob):
        o.counters[2] = 5   # (not the first gradient step of a run)
    seen = []
    for call in range(2):
        out = env.dpg_update(ring, pol, a[0], a[1], crit, a[2], a[3], oa, grad_steps=grad_steps, batch_size=batch, policy_delay=delay,
                             target_noise=sigma, seed=SEED, max_workgroups=wg, **LOSS)
        want, rows, noises = _piecewise(torch, env, ring, pol, crit, b, ob, grad_steps, delay, batch, SEED, wg, sigma)
        torch.cuda.synchronize()
        stats = out["stats"]
        assert tuple(stats.shape) == (grad_steps, 12) and out["rows"].dtype == torch.int32
        assert torch.equal(_bits(stats), _bits(want)), call
        assert torch.equal(out["rows"], rows)
        assert torch.equal(_state_bits(torch, a, oa), _state_bits(torch, b, ob)), call
        n_actor = grad_steps // delay
        done = (call + 1) * grad_steps
        assert oa.counters.tolist() == ob.counters.tolist() == [done, (call + 1) * n_actor, 5 + done, 0]
        last = 5 + done - 1
        assert np.array_equal(rows.cpu().numpy().astype(np.int64), H.sample_rows(batch, 304, SEED, last))
        for j in range(grad_steps):
            actor = (j + 1) % delay == 0
            assert int(stats[j, 7]) == batch and int(stats[j, 8]) == 0 and float(stats[j, 9]) > 0.0
            assert float(stats[j, 11]) == (1.0 if actor else 0.0) and (float(stats[j, 10]) > 0.0) == actor
            assert (float(stats[j, 4]) != 0.0) == actor
        seen.append((out["rows"].clone(), noises[-1].clone()))
    # the second call drew other rows and other noise: the device's count of finished steps keys both
    assert not torch.equal(seen[0][0], seen[1][0])
    if sigma > 0.0:
        assert float(seen[0][1].abs().max()) > 0.0 and not torch.equal(seen[0][1], seen[1][1])
    else:
        assert float(seen[0][1].abs().max()) == 0.0
    for x, s in zip(a, start):
        assert not torch.equal(_bits(x), _bits(s))
    for k, v in ring.data().items():   # the transitions are not written
        assert torch.equal(_bits(v), before[k]), k
    # a mapping with a fill entry is the same call
    c, oc = [x.clone() for x in start], DPGOptimizer(pol, crit, C, device=dev, lr_actor=1e-3, lr_critic=2e-3, max_grad_norm=0.5, tau=0.05)
    oc.counters[2] = 5
    for _ in range(2):
        env.dpg_update(dict(ring.data(), fill=ring.fill), pol, c[0], c[1], crit, c[2], c[3], oc, grad_steps=grad_steps, batch_size=batch,
                       policy_delay=delay, target_noise=sigma, seed=SEED, max_workgroups=wg, **LOSS)
    torch.cuda.synchronize()
    assert torch.equal(_state_bits(torch, a, oa), _state_bits(torch, c, oc))


def test_an_empty_ring_moves_no_parameter_and_advances_the_counters(env):
    import torch
    from rsoccer_amd.vec.optim import DPGOptimizer
    from rsoccer_amd.vec.replay import ReplayBuffer
    dev = env.device
    pol, crit = _nets()
    P = _params(torch, pol, crit, 2, 37, dev)
    start = [x.clone() for x in P]
    opt = DPGOptimizer(pol, crit, 2, device=dev, tau=0.05)
    out = env.dpg_update(ReplayBuffer(64, 40, 2, dev), pol, P[0], P[1], crit, P[2], P[3], opt, grad_steps=2, batch_size=33, policy_delay=2)
    torch.cuda.synchronize()
    assert bool((out["rows"] == -1).all()) and out["stats"][:, 7].tolist() == [0.0, 0.0] and out["stats"][:, 8].tolist() == [33.0, 33.0]
    assert out["stats"][:, 9].tolist() == [0.0, 0.0] and out["stats"][:, 10].tolist() == [0.0, 0.0]
    assert torch.equal(_bits(P[0]), _bits(start[0])) and torch.equal(_bits(P[2]), _bits(start[2]))
    assert opt.counters.tolist() == [2, 1, 2, 0] and float(torch.cat(opt.m + opt.v).abs().max()) == 0.0
    # the targets take their Polyak step on the actor step, as the header says
    assert np.array_equal(P[1].cpu().numpy().view(np.int32), H.polyak(start[0].cpu().numpy(), start[1].cpu().numpy(), 0.05).view(np.int32))


# ---- 6. one graph replay is one off-policy iteration ----
def test_a_captured_collect_add_and_dpg_update_replays_as_an_eager_twins_iterations():
    """one stream, no parallel branches: the off-policy twin of the PPO update's capture test"""
    import torch
    from rsoccer_amd import vec
    from rsoccer_amd.vec.optim import DPGOptimizer
    from rsoccer_amd.vec.replay import ReplayBuffer
    T, B, STEPS, BATCH = 4, 16, 2, 32
    envs = [vec.VecVSSEnv(B, device=0, seed=17, max_episode_steps=10) for _ in range(2)]
    for e in envs:
        e.reset()
        e.enable_graph_capture()
    env, twin = envs
    dev = env.device
    pol, crit = _nets()
    start = _params(torch, pol, crit, 2, 51, dev)
    log_std = torch.full((2,), -1.0, device=dev)
    sides = [([x.clone() for x in start], DPGOptimizer(pol, crit, 2, device=dev, lr_actor=1e-3, lr_critic=1e-3, max_grad_norm=0.5, tau=0.05),
              ReplayBuffer(160, 40, 2, dev)) for _ in envs]   # 160 rows: the fourth iteration's 64 wrap around the end

    def iteration(e, P, opt, buf):
        batch = e.collect(pol, P[0], T, log_std=log_std, noise_seed=99, return_final_obs=True)
        buf.add(batch)
        return e.dpg_update(buf, pol, P[0], P[1], crit, P[2], P[3], opt, grad_steps=STEPS, batch_size=BATCH, policy_delay=2, seed=123,
                            target_noise=0.2, **LOSS)

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
    (Pa, oa, ba), (Pb, ob, bb) = sides
    assert torch.equal(_state_bits(torch, Pa, oa), _state_bits(torch, Pb, ob))
    assert oa.counters.tolist() == ob.counters.tolist() == [4 * STEPS, 4 * STEPS // 2, 4 * STEPS, 0]
    for k in ("obs", "actions", "reward", "next_obs", "terminated"):
        assert torch.equal(_bits(ba.data()[k]), _bits(bb.data()[k])), k
    assert int(ba.head) == int(bb.head) == (4 * T * B) % 160 and int(ba.fill) == int(bb.fill) == 160
    assert np.array_equal(env.checkpoint(), twin.checkpoint())
    # every replay drew its own rows from the ring as it was filled by then: the step count on the device keys them
    for i, (_, r) in enumerate(seen):
        assert np.array_equal(r.cpu().numpy().astype(np.int64), H.sample_rows(BATCH, min((i + 1) * T * B, 160), 123, (i + 1) * STEPS - 1)), i
    for e in envs:
        e.close()


# ---- 7. the optimiser's state dict ----
def test_a_state_dict_round_trip_continues_with_equal_bits(env, ring):
    import torch
    from rsoccer_amd.vec.optim import DPGOptimizer
    dev = env.device
    pol, crit = _nets()
    start = _params(torch, pol, crit, 2, 61, dev)
    kw = dict(grad_steps=2, batch_size=33, policy_delay=2, seed=9, target_noise=0.2, **LOSS)

    def make():
        return DPGOptimizer(pol, crit, 2, device=dev, lr_actor=2e-3, lr_critic=1e-3, betas=(0.8, 0.99), eps=1e-7, max_grad_norm=0.3, tau=0.1)

    def update(P, o):
        env.dpg_update(ring, pol, P[0], P[1], crit, P[2], P[3], o, **kw)
    a, oa = [x.clone() for x in start], make()
    for _ in range(3):
        update(a, oa)
    b, ob = [x.clone() for x in start], make()
    for _ in range(2):
        update(b, ob)
    sd = ob.state_dict()
    saved = [x.clone() for x in b]
    update(b, ob)   # (the saved state is a copy: going on does not change it)
    oc = DPGOptimizer(pol, crit, 2, device=dev)   # other hyper-parameters: the state dict carries them
    addresses = [t.data_ptr() for t in oc.m + oc.v + [oc.counters]]
    oc.load_state_dict(sd)
    assert addresses == [t.data_ptr() for t in oc.m + oc.v + [oc.counters]]
    assert oc.counters.tolist() == [4, 2, 4, 0] and oc.betas == (0.8, 0.99) and oc.eps == 1e-7 and oc.max_grad_norm == 0.3
    assert (oc.lr_actor, oc.lr_critic, oc.tau) == (2e-3, 1e-3, 0.1)
    update(saved, oc)
    torch.cuda.synchronize()
    assert torch.equal(_state_bits(torch, a, oa), _state_bits(torch, saved, oc))
    assert oa.counters.tolist() == oc.counters.tolist() == [6, 3, 6, 0]
    with pytest.raises(ValueError, match=r"m\[0\]"):
        oc.load_state_dict({**sd, "m": [sd["m"][0][:-1], sd["m"][1]]})
    with pytest.raises(ValueError, match="counters"):
        oc.load_state_dict({"m": sd["m"], "v": sd["v"]})


# ---- 8. refusals: a ValueError naming the offender, or RSX_ERR_ARG, and nothing is enqueued ----
def test_refusals_change_nothing(env, ring):
    import torch
    from rsoccer_amd import _lib
    from rsoccer_amd.vec.optim import DPGOptimizer
    dev = env.device
    pol, crit = _nets()
    start = _params(torch, pol, crit, 2, 71, dev)
    P = [x.clone() for x in start]
    opt = DPGOptimizer(pol, crit, 2, device=dev)
    ok = dict(grad_steps=2, batch_size=33, policy_delay=2)

    def call(o=opt, buf=ring, **kw):
        return env.dpg_update(buf, pol, P[0], P[1], crit, P[2], P[3], o, **{**ok, **kw})
    for kw, word in ((dict(grad_steps=3), "multiple of policy_delay"), (dict(grad_steps=0), "grad_steps"), (dict(grad_steps=-2), "grad_steps"),
                     (dict(policy_delay=0), "policy_delay"), (dict(batch_size=0), "batch_size"), (dict(batch_size=-4), "batch_size"),
                     (dict(gamma=1.5), "gamma"), (dict(target_noise=float("nan")), "target_noise"), (dict(max_workgroups=0), "max_workgroups")):
        with pytest.raises(ValueError, match=word):
            call(**kw)
    for tau in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="tau"):
            DPGOptimizer(pol, crit, 2, device=dev, tau=tau)
        opt.tau = tau   # (set behind the constructor's back: the call checks it again)
        with pytest.raises(ValueError, match="tau"):
            call()
        opt.tau = 0.005
    with pytest.raises(ValueError, match="state tensors"):
        call(o=DPGOptimizer(pol, crit, 1, device=dev))
    with pytest.raises(ValueError, match="state tensors"):
        call(o=DPGOptimizer(*_nets(40, 2, 32, 1), 2, device=dev))
    with pytest.raises(ValueError, match="opt must be"):
        call(o=torch.optim.Adam([torch.nn.Parameter(P[0].clone())]))
    elsewhere = DPGOptimizer(pol, crit, 2, device=dev)
    elsewhere.device = torch.device("cuda", dev.index + 1)   # what an optimiser built on another device reports
    with pytest.raises(ValueError, match="optimiser is on"):
        call(o=elsewhere)
    with pytest.raises(ValueError, match="'fill'"):
        call(buf=ring.data())
    with pytest.raises(ValueError, match=r"buf\['fill'\]"):
        call(buf=dict(ring.data(), fill=ring.fill.to(torch.int32)))
    g = [torch.ones_like(x) for x in P]
    with pytest.raises(ValueError, match="grad_critic_params"):
        opt.step(*P, g[0], g[2][:1])
    with pytest.raises(ValueError, match="target_params"):
        opt.step(P[0], P[1][:-1], P[2], P[3], g[0], g[2])
    with pytest.raises(ValueError, match="step"):
        ring.sample_rows_device(4, step=torch.zeros(1, dtype=torch.int32, device=dev))
    # the C-ABI itself: RSX_ERR_ARG before anything is enqueued
    rows = torch.full((8,), -7, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        for bad in (lambda: _lib.replay_sample_rows(None, 8, 64, 8, None, 1, 0, None),
                    lambda: _lib.replay_sample_rows(rows.data_ptr(), 0, 64, 8, None, 1, 0, None),
                    lambda: _lib.replay_sample_rows(rows.data_ptr(), 8, 0, 8, None, 1, 0, None),
                    lambda: _lib.replay_sample_rows(rows.data_ptr(), 8, 2 ** 31, 8, None, 1, 0, None),
                    lambda: _lib.replay_sample_rows(rows.data_ptr(), 8, 64, -1, None, 1, 0, None)):
            with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):
                bad()
        st = opt.state()
        ptrs = [x.data_ptr() for x in P]
        io = _lib.DpgAdamIo(*ptrs, g[0].data_ptr(), g[2].data_ptr(), None, opt._ws.data_ptr(), 1)
        good = (0.9, 0.999, None, None, 1e-3, 1e-3, 1e-8, 0.5, 0.005)
        for k, v in ((8, -0.1), (8, 1.1), (8, float("nan")), (4, float("nan")), (5, -1.0), (6, float("inf")), (0, 1.0), (7, float("inf"))):
            cfg = _lib.DpgAdamCfg(*[v if i == k else x for i, x in enumerate(good)])
            with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):
                _lib.dpg_adam_step(cfg, st, io)
        for io_bad in (_lib.DpgAdamIo(ptrs[0], None, ptrs[2], ptrs[3], g[0].data_ptr(), g[2].data_ptr(), None, opt._ws.data_ptr(), 1),
                       _lib.DpgAdamIo(ptrs[0], ptrs[1], ptrs[2], None, None, g[2].data_ptr(), None, opt._ws.data_ptr(), 1),
                       _lib.DpgAdamIo(*ptrs, g[0].data_ptr(), None, None, opt._ws.data_ptr(), 0),
                       _lib.DpgAdamIo(*ptrs, g[0].data_ptr(), g[2].data_ptr(), None, None, 0)):
            with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):
                _lib.dpg_adam_step(opt.cfg(), st, io_bad)
    # rsx_task_dpg_update past the Python layer
    nbytes, _ = env.sim.dpg_update_workspace(pol.spec(), crit.spec(), 2, 33, 0)
    ws, stats = torch.zeros(nbytes // 4 + 1, device=dev), torch.zeros(2, 12, device=dev)
    d = ring.data()
    inp = lambda r=None: _lib.DpgIn(d["obs"].data_ptr(), d["actions"].data_ptr(), d["reward"].data_ptr(), d["next_obs"].data_ptr(),   # noqa: E731
                                    d["terminated"].data_ptr(), r, CAPACITY, 33)
    cfg = _lib.DpgCfg(None, 1, 0, 0.99, 0.2, 0.5, 2, 0)
    fill = ring.fill.data_ptr()
    small = DPGOptimizer(pol, crit, 1, device=dev)
    for i, ucfg, state in ((inp(), _lib.DpgUpdateCfg(fill, 1, 0, 3, 2), opt.state()), (inp(), _lib.DpgUpdateCfg(fill, 1, 0, 0, 1), opt.state()),
                           (inp(), _lib.DpgUpdateCfg(fill, 1, 0, 2, 0), opt.state()), (inp(), _lib.DpgUpdateCfg(None, 1, -1, 2, 2), opt.state()),
                           (inp(rows.data_ptr()), _lib.DpgUpdateCfg(fill, 1, 0, 2, 2), opt.state()),
                           (inp(), _lib.DpgUpdateCfg(fill, 1, 0, 2, 2), small.state())):
        with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):
            env.sim.task_dpg_update(pol.spec(), P[0].data_ptr(), P[1].data_ptr(), crit.spec(), P[2].data_ptr(), P[3].data_ptr(), i, cfg, ucfg,
                                    opt.cfg(), state, stats.data_ptr(), ws.data_ptr(), env._stream())
    with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):
        env.sim.dpg_update_workspace(pol.spec(), crit.spec(), 3, 33, 0)
    torch.cuda.synchronize()
    for a, b in zip(P, start):
        assert torch.equal(_bits(a), _bits(b))
    assert opt.counters.tolist() == [0, 0, 0, 0] and float(torch.cat(opt.m + opt.v).abs().max()) == 0.0
    assert bool((rows == -7).all()) and float(stats.abs().max()) == 0.0
