"""The soft actor-critic update phase on the device (SACOptimizer, VecFusedEnv.sac_update): the three-group clip + Adam + Polyak step
against its numpy restatement bit for bit, against float64 with torch's float32 as the yardstick, frozen groups leaving their bytes
alone, sac_update against the sequence of public pieces bit for bit, the empty ring as include/rsx.h states it, a captured
collect + add + sac_update against an eager twin, the optimiser's state dict, and the refusals."""
import numpy as np
import pytest

import dpg_helpers as DH
import dpg_update_helpers as DU
import sac_update_helpers as H

pytestmark = pytest.mark.gpu

CAPACITY = 1024
LOSS = dict(gamma=0.97, target_entropy=-1.5)


@pytest.fixture(scope="module")
def env():
    from rsoccer_amd import vec
    e = vec.VecVSSEnv(16, device=0, seed=3)
    yield e
    e.close()


def _nets(obs_dim=40, act_dim=2, hidden=64, layers=2):
    from rsoccer_amd.vec.policy import MLPGaussianPolicy, MLPQCritic
    return (MLPGaussianPolicy(obs_dim, act_dim, hidden=hidden, layers=layers, hidden_act="tanh", log_std_min=-5.0, log_std_max=1.0),
            MLPQCritic(obs_dim, act_dim, hidden=hidden, layers=layers, hidden_act="tanh"))


def _params(torch, pol, crit, C, seed, dev):
    """[actor, critics [C, Pc], their target, log_alpha [1]]: torch.nn.Linear's initialisation, live and target critics 0.02 apart"""
    gen = torch.Generator().manual_seed(seed)
    p = DH.init(torch, pol, gen)
    c0 = torch.stack([DH.init(torch, crit, gen) for _ in range(C)])
    c = c0 + 0.02 * torch.randn(C, crit.num_params, generator=gen)
    return [x.float().contiguous().to(dev) for x in (p, c, c0, torch.tensor([-0.7]))]


@pytest.fixture(scope="module")
def ring(env):
    """a ring of 1024 rows partly filled by ONE collect of 19 steps on 16 envs (304 rows); read only"""
    import torch
    from rsoccer_amd.vec.replay import ReplayBuffer
    pol, crit = _nets()
    p = _params(torch, pol, crit, 1, 5, env.device)[0]
    env.reset()
    batch = env.collect(pol, p, 19, noise_seed=7, return_final_obs=True)
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


def _host(P):
    return [x.cpu().numpy().reshape(-1).copy() for x in P]


def _same(got, want):
    return np.array_equal(got.detach().cpu().numpy().reshape(-1).view(np.int32), np.asarray(want, np.float32).reshape(-1).view(np.int32))


# ---- 1. the optimiser step against the restatement ----
# "tiny": 3-32-2 actor (194 parameters: below one workgroup) and one 4-32-1 critic; "vss": 40-64-64-4 actor, twin 42-64-64-1 critics;
# "wide": a critic group of 17 410 floats, more than one trip of the norm reduction's 64 workgroups of 256 threads covers
OPT_SHAPES = {"tiny": (3, 1, 32, 1, 1, 194, 193), "vss": (40, 2, 64, 2, 2, 7044, 2 * 6977), "wide": (64, 5, 64, 2, 2, 8970, 17410)}
LRS, TAU = (1e-3, 3e-3, 2e-3), 0.05


def _opt(torch, shape, max_norm, lr_by, dev):
    from rsoccer_amd.vec.optim import SACOptimizer
    od, ad, hidden, layers, C, na, nc = OPT_SHAPES[shape]
    pol, crit = _nets(od, ad, hidden, layers)
    assert (pol.num_params, C * crit.num_params) == (na, nc)
    lrs = LRS if lr_by == "value" else tuple(torch.tensor([v], dtype=torch.float32, device=dev) for v in LRS)
    opt = SACOptimizer(pol, crit, C, device=dev, lr_actor=lrs[0], lr_critic=lrs[1], lr_alpha=lrs[2], max_grad_norm=max_norm, tau=TAU)
    return pol, crit, C, opt


@pytest.mark.parametrize("shape", ["tiny", "vss", "wide"])
@pytest.mark.parametrize("max_norm", [0.5, None])
@pytest.mark.parametrize("lr_by", ["value", "tensor"])
def test_optimiser_steps_equal_the_restatement_bit_for_bit(env, shape, max_norm, lr_by):
    """three consecutive steps of all three groups; parameters, targets, log_alpha, moments, counters and stats"""
    import torch
    dev = env.device
    pol, crit, C, opt = _opt(torch, shape, max_norm, lr_by, dev)
    na, nc = opt.sizes
    assert shape != "wide" or nc > 64 * 256
    assert shape != "tiny" or (na < 256 and nc < 256)
    P = _params(torch, pol, crit, C, 11, dev)
    host, st = _host(P), H.fresh_state(na, nc)
    gen = torch.Generator().manual_seed(5)
    for step in (1, 2, 3):
        ga, gc, gl = torch.randn(na, generator=gen), torch.randn(C, crit.num_params, generator=gen), torch.randn(1, generator=gen)
        out = opt.step(*P, ga.to(dev), gc.to(dev), gl.to(dev))
        torch.cuda.synchronize()
        *host, stats = H.sac_adam_step(st, *host, ga.numpy(), gc.numpy(), gl.numpy(), *LRS, max_norm=max_norm, tau=TAU)
        for name, got, want in zip(("params", "critic_params", "target_critic_params", "log_alpha"), P, host):
            assert _same(got, want), (step, name)
        for k, name in enumerate(("actor", "critics", "log_alpha")):
            assert _same(opt.m[k], st["m"][k]), (step, "m", name)
            assert _same(opt.v[k], st["v"][k]), (step, "v", name)
        assert opt.counters.tolist() == st["counters"] == [step] * 4
        assert int(opt.steps) == step and opt.steps.data_ptr() == opt.counters.data_ptr() + 24
        got = np.array([float(out[k]) for k in ("grad_norm_critic", "grad_norm_actor", "log_alpha", "targets_moved")], dtype=np.float32)
        assert np.array_equal(got.view(np.int32), stats.view(np.int32)), (step, got, stats)
        assert stats[0] > 0.5 and stats[1] > 0.5 and stats[3] == 1.0   # (the clip binds where there is one)


# ---- 2. the optimiser step against torch ----
def test_three_steps_stay_within_4x_of_torchs_float32_error(env):
    """Criterion (docs/VERIFICATION.md f13): after each of three steps the relative error of every tensor against float64 — three
    torch.optim.Adam behind two clip_grad_norm_ calls plus lerp_ — is at most 4 x the LARGEST relative error any tensor of torch's own
    float32 run shows."""
    import torch
    dev = env.device
    pol, crit, C, opt = _opt(torch, "vss", 0.5, "value", dev)
    P = _params(torch, pol, crit, C, 13, dev)
    start = [P[0].cpu(), P[1].cpu().reshape(-1), P[2].cpu().reshape(-1), P[3].cpu()]
    gen = torch.Generator().manual_seed(6)
    grads = [(torch.randn(opt.sizes[0], generator=gen), torch.randn(opt.sizes[1], generator=gen), torch.randn(1, generator=gen))
             for _ in range(3)]
    ref64 = H.torch_steps(start, grads, LRS, 0.5, TAU, torch.float64)
    yard32 = H.torch_steps(start, grads, LRS, 0.5, TAU, torch.float32)
    worst = 0.0
    for k, (ga, gc, gl) in enumerate(grads):
        opt.step(*P, ga.to(dev), gc.reshape(C, -1).to(dev), gl.to(dev))
        torch.cuda.synchronize()
        got = H.tensors_of({"m": _host(opt.m), "v": _host(opt.v)}, *_host(P))
        worst = max(worst, H.check_against_torch(got, ref64[k], yard32[k], k + 1, "kernel"))
    print(f"worst tensor: {worst:.2f} x torch's float32 error")


# ---- 3. frozen groups ----
def test_a_frozen_group_keeps_its_bytes_and_its_own_step_count(env):
    import torch
    dev = env.device
    pol, crit, C, opt = _opt(torch, "vss", 0.5, "value", dev)
    na, nc = opt.sizes
    P = _params(torch, pol, crit, C, 17, dev)
    host, st = _host(P), H.fresh_state(na, nc)
    gen = torch.Generator().manual_seed(8)
    draw = lambda: (torch.randn(na, generator=gen), torch.randn(C, crit.num_params, generator=gen), torch.randn(1, generator=gen))  # noqa: E731

    def both(ga, gc, gl, update_targets=True):
        nonlocal host
        out = opt.step(*P, None if ga is None else ga.to(dev), gc.to(dev), None if gl is None else gl.to(dev), update_targets=update_targets)
        torch.cuda.synchronize()
        *host, stats = H.sac_adam_step(st, *host, None if ga is None else ga.numpy(), gc.numpy(), None if gl is None else gl.numpy(), *LRS,
                                       max_norm=0.5, tau=TAU, update_targets=update_targets)
        for name, got, want in zip(("params", "critic_params", "target_critic_params", "log_alpha"), P, host):
            assert _same(got, want), name
        for k in range(3):
            assert _same(opt.m[k], st["m"][k]) and _same(opt.v[k], st["v"][k]), k
        assert opt.counters.tolist() == st["counters"]
        assert np.array_equal(np.array([float(v) for v in out.values()], np.float32).view(np.int32), stats.view(np.int32))
        return out

    both(*draw())   # a full step first: no moment and no t is zero
    # without grad_params: the actor, its moments and its t keep their bytes
    keep = [_bits(x) for x in (P[0], opt.m[0], opt.v[0])]
    others = [_bits(x) for x in (P[1], P[2], P[3])]
    ga, gc, gl = draw()
    out = both(None, gc, gl)
    assert all(torch.equal(a, _bits(b)) for a, b in zip(keep, (P[0], opt.m[0], opt.v[0])))
    assert not any(torch.equal(a, _bits(b)) for a, b in zip(others, (P[1], P[2], P[3])))
    assert opt.counters.tolist() == [2, 1, 2, 2] and float(out["grad_norm_actor"]) == 0.0
    # without grad_log_alpha (a fixed temperature): log_alpha, its moments and its t keep their bytes
    keep = [_bits(x) for x in (P[3], opt.m[2], opt.v[2])]
    actor = _bits(P[0])
    ga, gc, gl = draw()
    out = both(ga, gc, None)
    assert all(torch.equal(a, _bits(b)) for a, b in zip(keep, (P[3], opt.m[2], opt.v[2])))
    assert not torch.equal(actor, _bits(P[0])) and opt.counters.tolist() == [3, 2, 2, 3]
    assert _bits(out["log_alpha"].reshape(1)).tolist() == keep[0].tolist()
    # update_targets=False: the targets keep their bytes
    targ = _bits(P[2])
    out = both(*draw(), update_targets=False)
    assert torch.equal(targ, _bits(P[2])) and float(out["targets_moved"]) == 0.0
    # and the step after the frozen ones used each group's own t (the restatement's counters are [4, 3, 3, 4]: both() compared the bits)
    assert opt.counters.tolist() == [4, 3, 3, 4]
    both(*draw())
    assert opt.counters.tolist() == [5, 4, 4, 5]


# ---- 4. composition: sac_update is the sequence of the public pieces ----
def _piecewise(torch, env, buf, pol, crit, P, opt, grad_steps, batch, seed, wg, learn_alpha):
    """the update as calls of the public pieces.  Returns (stats [grad_steps, 16], the last step's rows)"""
    from rsoccer_amd import _lib
    table, rows = [], None
    for _ in range(grad_steps):
        rows = buf.sample_rows_device(batch, seed=seed, step=opt.steps)
        out = env.sac_gradient(buf.data(), pol, P[0], crit, P[1], P[2], P[3], rows=rows, noise_seed=seed, noise_step=opt.steps,
                               max_workgroups=wg, **LOSS)
        o = opt.step(*P, out["grad_params"], out["grad_critic_params"], out["grad_log_alpha"] if learn_alpha else None)
        table.append(torch.stack([out["stats"][k] for k in _lib.SAC_STATS] + [o[k] for k in _lib.SAC_ADAM_STATS]))
    return torch.stack(table), rows


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("batch", [63, 65])
@pytest.mark.parametrize("wg", [1, None])
@pytest.mark.parametrize("learn_alpha", [True, False])
def test_sac_update_equals_the_sequence_of_public_pieces_bit_for_bit(env, ring, C, batch, wg, learn_alpha):
    import torch
    from rsoccer_amd import _lib
    from rsoccer_amd.vec.optim import SACOptimizer
    dev = env.device
    pol, crit = _nets()
    start = _params(torch, pol, crit, C, 31, dev)
    before = {k: _bits(v) for k, v in ring.data().items()}
    SEED, STEPS = 77, 3
    a, b = [x.clone() for x in start], [x.clone() for x in start]
    make = lambda: SACOptimizer(pol, crit, C, device=dev, lr_actor=1e-3, lr_critic=2e-3, lr_alpha=5e-3, max_grad_norm=0.5, tau=0.05)  # noqa: E731
    oa, ob = make(), make()
    for o in (oa, ob):
        o.counters[3] = 5   # (not the first gradient step of a run)
    seen = []
    for call in range(2):
        out = env.sac_update(ring, pol, a[0], crit, a[1], a[2], a[3], oa, grad_steps=STEPS, batch_size=batch, learn_alpha=learn_alpha,
                             seed=SEED, max_workgroups=wg, **LOSS)
        want, rows = _piecewise(torch, env, ring, pol, crit, b, ob, STEPS, batch, SEED, wg, learn_alpha)
        torch.cuda.synchronize()
        table = out["table"]
        assert tuple(table.shape) == (STEPS, 16) and out["rows"].dtype == torch.int32
        assert torch.equal(_bits(table), _bits(want)), call
        assert list(out["stats"]) == list(_lib.SAC_UPDATE_STATS)
        for k, name in enumerate(_lib.SAC_UPDATE_STATS):
            assert tuple(out["stats"][name].shape) == (STEPS,) and torch.equal(_bits(out["stats"][name]), _bits(table[:, k])), name
        assert torch.equal(out["rows"], rows)
        assert torch.equal(_state_bits(torch, a, oa), _state_bits(torch, b, ob)), call
        done = (call + 1) * STEPS
        assert oa.counters.tolist() == ob.counters.tolist() == [done, done, done if learn_alpha else 0, 5 + done]
        assert np.array_equal(rows.cpu().numpy().astype(np.int64), DU.sample_rows(batch, 304, SEED, 5 + done - 1))
        s = out["stats"]
        assert s["rows_used"].tolist() == [float(batch)] * STEPS and s["rows_skipped"].tolist() == [0.0] * STEPS
        assert bool((s["grad_norm_critic"] > 0).all()) and bool((s["grad_norm_actor"] > 0).all()) and s["targets_moved"].tolist() == [1.0] * STEPS
        assert s["log_alpha"][-1].item() == a[3].item()
        seen.append(out["rows"].clone())
    assert not torch.equal(seen[0], seen[1])   # the second call drew other rows: the device's count of finished steps keys them
    for k, (x, s0) in enumerate(zip(a, start)):
        assert torch.equal(_bits(x), _bits(s0)) == (k == 3 and not learn_alpha), k
    if not learn_alpha:
        assert float(torch.cat([oa.m[2], oa.v[2]]).abs().max()) == 0.0
    for k, v in ring.data().items():   # the transitions are not written
        assert torch.equal(_bits(v), before[k]), k
    # a mapping with a fill entry is the same call
    c, oc = [x.clone() for x in start], make()
    oc.counters[3] = 5
    for _ in range(2):
        env.sac_update(dict(ring.data(), fill=ring.fill), pol, c[0], crit, c[1], c[2], c[3], oc, grad_steps=STEPS, batch_size=batch,
                       learn_alpha=learn_alpha, seed=SEED, max_workgroups=wg, **LOSS)
    torch.cuda.synchronize()
    assert torch.equal(_state_bits(torch, a, oa), _state_bits(torch, c, oc))


def test_an_empty_ring_moves_no_parameter_and_advances_the_counters(env):
    """as include/rsx.h states it: every row skipped, the critics' and the actor's gradients +0, grad_log_alpha -0.0f, which Adam treats
    as 0; no parameter moves, log_alpha included; the four counters advance and the target critics take their Polyak steps"""
    import torch
    from rsoccer_amd.vec.optim import SACOptimizer
    from rsoccer_amd.vec.replay import ReplayBuffer
    dev = env.device
    pol, crit = _nets()
    P = _params(torch, pol, crit, 2, 37, dev)
    start = [x.clone() for x in P]
    opt = SACOptimizer(pol, crit, 2, device=dev, tau=0.05)
    empty = ReplayBuffer(64, 40, 2, dev)
    out = env.sac_update(empty, pol, P[0], crit, P[1], P[2], P[3], opt, grad_steps=2, batch_size=33)
    torch.cuda.synchronize()
    s = out["stats"]
    assert bool((out["rows"] == -1).all()) and s["rows_used"].tolist() == [0.0, 0.0] and s["rows_skipped"].tolist() == [33.0, 33.0]
    assert s["grad_norm_critic"].tolist() == [0.0, 0.0] and s["grad_norm_actor"].tolist() == [0.0, 0.0] and s["targets_moved"].tolist() == [1.0, 1.0]
    for k in (0, 1, 3):
        assert torch.equal(_bits(P[k]), _bits(start[k])), k
    assert s["log_alpha"].tolist() == [start[3].item()] * 2
    assert opt.counters.tolist() == [2, 2, 2, 2] and float(torch.cat(opt.m + opt.v).abs().max()) == 0.0
    # the gradient of the temperature on an all-skipped minibatch is minus a sum of nothing
    g = env.sac_gradient(empty.data(), pol, P[0], crit, P[1], P[2], P[3], rows=out["rows"])
    torch.cuda.synchronize()
    assert _bits(g["grad_log_alpha"]).tolist() == [-2 ** 31] and float(g["grad_params"].abs().max()) == 0.0
    # the targets took two Polyak steps towards the unmoved critics
    want = start[2].cpu().numpy().reshape(-1)
    for _ in range(2):
        want = DU.polyak(start[1].cpu().numpy().reshape(-1), want, 0.05)
    assert _same(P[2], want) and not torch.equal(_bits(P[2]), _bits(start[2]))


# ---- 5. one graph replay is one off-policy iteration ----
def test_a_captured_collect_add_and_sac_update_replays_as_an_eager_twins_iterations():
    """one stream, no parallel branches: the twin of the TD3 update's capture test"""
    import torch
    from rsoccer_amd import vec
    from rsoccer_amd.vec.optim import SACOptimizer
    from rsoccer_amd.vec.replay import ReplayBuffer
    T, B, STEPS, BATCH = 4, 16, 2, 64
    envs = [vec.VecVSSEnv(B, device=0, seed=17, max_episode_steps=10) for _ in range(2)]
    for e in envs:
        e.reset()
        e.enable_graph_capture()
    env, twin = envs
    dev = env.device
    pol, crit = _nets()
    start = _params(torch, pol, crit, 2, 51, dev)
    sides = [([x.clone() for x in start], SACOptimizer(pol, crit, 2, device=dev, lr_actor=1e-3, lr_critic=1e-3, lr_alpha=3e-3, max_grad_norm=0.5,
                                                       tau=0.05),
              ReplayBuffer(160, 40, 2, dev)) for _ in envs]   # 160 rows: the third iteration's 64 wrap around the end

    def iteration(e, P, opt, buf):
        batch = e.collect(pol, P[0], T, noise_seed=99, return_final_obs=True)
        buf.add(batch)
        return e.sac_update(buf, pol, P[0], crit, P[1], P[2], P[3], opt, grad_steps=STEPS, batch_size=BATCH, seed=123, **LOSS)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # torch's warm-up before a capture: an iteration of BOTH sides, so that they stay twins
        iteration(env, *sides[0])
    torch.cuda.current_stream().wait_stream(side)
    iteration(twin, *sides[1])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = iteration(env, *sides[0])
    seen, want = [], []
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        seen.append((out["table"].clone(), out["rows"].clone()))
    for _ in range(3):
        o = iteration(twin, *sides[1])
        torch.cuda.synchronize()
        want.append((o["table"].clone(), o["rows"].clone()))
    for i, ((s, r), (ws, wr)) in enumerate(zip(seen, want)):
        assert torch.equal(_bits(s), _bits(ws)), ("stats", i)
        assert torch.equal(r, wr), ("rows", i)
    (Pa, oa, ba), (Pb, ob, bb) = sides
    assert torch.equal(_state_bits(torch, Pa, oa), _state_bits(torch, Pb, ob))
    assert oa.counters.tolist() == ob.counters.tolist() == [4 * STEPS] * 4
    for k in ("obs", "actions", "reward", "next_obs", "terminated"):
        assert torch.equal(_bits(ba.data()[k]), _bits(bb.data()[k])), k
    assert int(ba.head) == int(bb.head) == (4 * T * B) % 160 and int(ba.fill) == int(bb.fill) == 160
    assert np.array_equal(env.checkpoint(), twin.checkpoint())
    # every replay drew its own rows from the ring as it was filled by then: the step count on the device keys them
    for i, (_, r) in enumerate(seen, 1):
        assert np.array_equal(r.cpu().numpy().astype(np.int64), DU.sample_rows(BATCH, min((i + 1) * T * B, 160), 123, (i + 1) * STEPS - 1)), i
    assert not torch.equal(seen[0][1], seen[1][1])
    for e in envs:
        e.close()


# ---- 6. the optimiser's state dict ----
def test_a_state_dict_round_trip_continues_with_equal_bits(env, ring):
    import torch
    from rsoccer_amd.vec.optim import SACOptimizer
    dev = env.device
    pol, crit = _nets()
    start = _params(torch, pol, crit, 2, 61, dev)
    kw = dict(grad_steps=2, batch_size=33, seed=9, **LOSS)

    def make():
        return SACOptimizer(pol, crit, 2, device=dev, lr_actor=2e-3, lr_critic=1e-3, lr_alpha=4e-3, betas=(0.8, 0.99), eps=1e-7,
                            max_grad_norm=0.3, tau=0.1)

    def update(P, o):
        env.sac_update(ring, pol, P[0], crit, P[1], P[2], P[3], o, **kw)
    a, oa = [x.clone() for x in start], make()
    for _ in range(3):
        update(a, oa)
    b, ob = [x.clone() for x in start], make()
    for _ in range(2):
        update(b, ob)
    sd = ob.state_dict()
    assert len(sd["m"]) == len(sd["v"]) == 3
    saved = [x.clone() for x in b]
    update(b, ob)   # (the saved state is a copy: going on does not change it)
    oc = SACOptimizer(pol, crit, 2, device=dev)   # other hyper-parameters: the state dict carries them
    addresses = [t.data_ptr() for t in oc.m + oc.v + [oc.counters]]
    oc.load_state_dict(sd)
    assert addresses == [t.data_ptr() for t in oc.m + oc.v + [oc.counters]]
    assert oc.counters.tolist() == [4, 4, 4, 4] and oc.betas == (0.8, 0.99) and oc.eps == 1e-7 and oc.max_grad_norm == 0.3
    assert (oc.lr_actor, oc.lr_critic, oc.lr_alpha, oc.tau) == (2e-3, 1e-3, 4e-3, 0.1)
    update(saved, oc)
    torch.cuda.synchronize()
    assert torch.equal(_state_bits(torch, a, oa), _state_bits(torch, saved, oc))
    assert oa.counters.tolist() == oc.counters.tolist() == [6, 6, 6, 6]
    with pytest.raises(ValueError, match=r"m\[0\]"):
        oc.load_state_dict({**sd, "m": [sd["m"][0][:-1], sd["m"][1], sd["m"][2]]})
    with pytest.raises(ValueError, match="three tensors"):
        oc.load_state_dict({**sd, "v": sd["v"][:2]})
    with pytest.raises(ValueError, match="counters"):
        oc.load_state_dict({"m": sd["m"], "v": sd["v"]})


# ---- 7. refusals: a ValueError naming the offender, or RSX_ERR_ARG, and nothing is enqueued ----
def test_refusals_change_nothing(env, ring):
    import torch
    from rsoccer_amd import _lib
    from rsoccer_amd.vec.optim import DPGOptimizer, SACOptimizer
    from rsoccer_amd.vec.policy import MLPPolicy
    dev = env.device
    pol, crit = _nets()
    start = _params(torch, pol, crit, 2, 71, dev)
    P = [x.clone() for x in start]
    opt = SACOptimizer(pol, crit, 2, device=dev)
    ok = dict(grad_steps=2, batch_size=33)

    def call(o=opt, buf=ring, la=P[3], **kw):
        return env.sac_update(buf, pol, P[0], crit, P[1], P[2], la, o, **{**ok, **kw})
    for kw, word in ((dict(grad_steps=0), "grad_steps"), (dict(grad_steps=-2), "grad_steps"), (dict(batch_size=0), "batch_size"),
                     (dict(batch_size=-4), "batch_size"), (dict(gamma=1.5), "gamma"), (dict(target_entropy=float("nan")), "target_entropy"),
                     (dict(max_workgroups=0), "max_workgroups"), (dict(la=P[3].reshape(())), "log_alpha"), (dict(la=P[3].double()), "log_alpha")):
        with pytest.raises(ValueError, match=word):
            call(**kw)
    for tau in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="tau"):
            SACOptimizer(pol, crit, 2, device=dev, tau=tau)
        opt.tau = tau   # (set behind the constructor's back: the call checks it again)
        with pytest.raises(ValueError, match="tau"):
            call()
        opt.tau = 0.005
    with pytest.raises(ValueError, match="state tensors"):
        call(o=SACOptimizer(pol, crit, 1, device=dev))
    with pytest.raises(ValueError, match="state tensors"):
        call(o=SACOptimizer(*_nets(40, 2, 32, 1), 2, device=dev))
    with pytest.raises(ValueError, match="opt must be"):
        call(o=DPGOptimizer(MLPPolicy(40, 2, hidden=64, layers=2, hidden_act="tanh", out_act="tanh"), crit, 2, device=dev))
    elsewhere = SACOptimizer(pol, crit, 2, device=dev)
    elsewhere.device = torch.device("cuda", dev.index + 1)   # what an optimiser built on another device reports
    with pytest.raises(ValueError, match="optimiser is on"):
        call(o=elsewhere)
    with pytest.raises(ValueError, match="'fill'"):
        call(buf=ring.data())
    with pytest.raises(ValueError, match=r"buf\['fill'\]"):
        call(buf=dict(ring.data(), fill=ring.fill.to(torch.int32)))
    g = [torch.ones_like(x) for x in P]
    with pytest.raises(ValueError, match="grad_critic_params"):
        opt.step(*P, g[0], g[1][:1], g[3])
    with pytest.raises(ValueError, match="grad_log_alpha"):
        opt.step(*P, g[0], g[1], torch.ones(2, device=dev))
    with pytest.raises(ValueError, match="target_critic_params"):
        opt.step(P[0], P[1], P[2][:, :-1], P[3], g[0], g[1], g[3])
    # the C-ABI itself: RSX_ERR_ARG before anything is enqueued
    with torch.cuda.device(dev):
        st = opt.state()
        ptrs = [x.data_ptr() for x in P]
        gp = [x.data_ptr() for x in (g[0], g[1], g[3])]
        ws = opt._ws.data_ptr()
        good = (0.9, 0.999, None, None, None, 1e-3, 1e-3, 1e-3, 1e-8, 0.5, 0.005)
        for k, v in ((10, -0.1), (10, 1.1), (10, float("nan")), (5, float("nan")), (6, -1.0), (7, -1.0), (7, float("nan")), (7, float("inf")),
                     (8, float("inf")), (0, 1.0), (1, -0.1), (9, float("inf"))):
            cfg = _lib.SacAdamCfg(*[v if i == k else x for i, x in enumerate(good)])
            with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):
                _lib.sac_adam_step(cfg, st, _lib.SacAdamIo(*ptrs, *gp, None, ws, 1))
        for io_bad in (_lib.SacAdamIo(None, ptrs[1], ptrs[2], ptrs[3], *gp, None, ws, 1),
                       _lib.SacAdamIo(ptrs[0], None, ptrs[2], ptrs[3], *gp, None, ws, 1),
                       _lib.SacAdamIo(ptrs[0], ptrs[1], None, ptrs[3], *gp, None, ws, 1),      # update_targets without a target
                       _lib.SacAdamIo(ptrs[0], ptrs[1], ptrs[2], None, *gp, None, ws, 1),      # a null log_alpha
                       _lib.SacAdamIo(*ptrs, gp[0], None, gp[2], None, ws, 0),
                       _lib.SacAdamIo(*ptrs, *gp, None, None, 0)):
            with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):
                _lib.sac_adam_step(opt.cfg(), st, io_bad)
        fields = [f[0] for f in _lib.SacAdamState._fields_]
        for name, v in (("m_alpha", None), ("v_alpha", None), ("m_actor", None), ("v_critic", None), ("counters", None), ("n_actor", 0),
                        ("n_critic", 2 ** 31)):
            bad = _lib.SacAdamState(*[v if f == name else getattr(st, f) for f in fields])
            with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):
                _lib.sac_adam_step(opt.cfg(), bad, _lib.SacAdamIo(*ptrs, *gp, None, ws, 1))
        for args in ((None, st), (opt.cfg(), None)):
            with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):
                _lib.sac_adam_step(*args, _lib.SacAdamIo(*ptrs, *gp, None, ws, 1))
        with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):
            _lib.sac_adam_step(opt.cfg(), st, None)
    # rsx_task_sac_update past the Python layer
    nbytes, _ = env.sim.sac_update_workspace(pol.spec(), crit.spec(), 2, 33, 0)
    wsp, stats = torch.zeros(nbytes // 4 + 1, device=dev), torch.zeros(2, 16, device=dev)
    rows = torch.full((33,), -7, dtype=torch.int32, device=dev)
    d = ring.data()
    inp = lambda r=None: _lib.DpgIn(d["obs"].data_ptr(), d["actions"].data_ptr(), d["reward"].data_ptr(), d["next_obs"].data_ptr(),   # noqa: E731
                                    d["terminated"].data_ptr(), r, CAPACITY, 33)
    cfg = _lib.SacCfg(None, 1, 0, 0.99, -2.0, pol.log_std_min, pol.log_std_max, 2, 0)
    fill = ring.fill.data_ptr()
    small = SACOptimizer(pol, crit, 1, device=dev)
    U = _lib.SacUpdateCfg
    for i, c, ucfg, state, sp, wp in ((inp(), cfg, U(fill, 1, 0, 0, 1), opt.state(), stats.data_ptr(), wsp.data_ptr()),
                                      (inp(), cfg, U(None, 1, -1, 2, 1), opt.state(), stats.data_ptr(), wsp.data_ptr()),
                                      (inp(rows.data_ptr()), cfg, U(fill, 1, 0, 2, 1), opt.state(), stats.data_ptr(), wsp.data_ptr()),
                                      (inp(), cfg, U(fill, 1, 0, 2, 1), small.state(), stats.data_ptr(), wsp.data_ptr()),
                                      (inp(), cfg, None, opt.state(), stats.data_ptr(), wsp.data_ptr()),
                                      (inp(), cfg, U(fill, 1, 0, 2, 1), opt.state(), None, wsp.data_ptr()),
                                      (inp(), cfg, U(fill, 1, 0, 2, 1), opt.state(), stats.data_ptr(), None),
                                      (inp(), _lib.SacCfg(None, 1, 0, 0.99, float("nan"), -5.0, 1.0, 2, 0), U(fill, 1, 0, 2, 1), opt.state(),
                                       stats.data_ptr(), wsp.data_ptr())):
        with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):
            env.sim.task_sac_update(pol.spec(), P[0].data_ptr(), crit.spec(), P[1].data_ptr(), P[2].data_ptr(), P[3].data_ptr(), i, c, ucfg,
                                    opt.cfg(), state, sp, wp, env._stream())
    with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):   # a null log_alpha
        env.sim.task_sac_update(pol.spec(), P[0].data_ptr(), crit.spec(), P[1].data_ptr(), P[2].data_ptr(), None, inp(), cfg, U(fill, 1, 0, 2, 1),
                                opt.cfg(), opt.state(), stats.data_ptr(), wsp.data_ptr(), env._stream())
    with pytest.raises(_lib.RsxError, match="librsx_hip error -1"):
        env.sim.sac_update_workspace(pol.spec(), crit.spec(), 3, 33, 0)
    torch.cuda.synchronize()
    for x, y in zip(P, start):
        assert torch.equal(_bits(x), _bits(y))
    assert opt.counters.tolist() == [0, 0, 0, 0] and float(torch.cat(opt.m + opt.v).abs().max()) == 0.0
    assert bool((rows == -7).all()) and float(stats.abs().max()) == 0.0
