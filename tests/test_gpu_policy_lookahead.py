"""VecFusedEnv.lookahead_policy / rsx_task_lookahead_policy.  The oracle does not know the policy; exactness comes from the call's own
contract instead: the actions it records, fed to lookahead() — and to step() — from the same state, reproduce its results bit for
bit, and the recorded actions are the policy's answer to the recorded observations.  Comparisons are on bit patterns unless a bound
is derived next to them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, K, H, WARM = 9, 3, 6, 3   # one full 8-env tile and a ragged one at 8 lanes per env
U = 2.0 ** -24               # unit roundoff of float32
# Largest |kernel tanh - float64 tanh| over exactly-known inputs covering [-4.8, 4.8], measured on an MI355X by
# test_tanh_allowance_is_measured below (profiles/LABBOOK.md, "Closed-loop lookahead"): 6.4e-8.  The dense test allows 4 x this
# per tanh application, so that a different but equally good rounding on another compiler does not fail.
TANH_DEV = 6.4e-8

CLASSES = ["VecVSSEnv", "VecSSLStaticDefendersEnv", "VecSSLDribblingEnv", "VecSSLContestedPossessionEnv", "VecSSLPassEnduranceEnv"]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _make(vec, name, n, **kw):
    if name == "VecVSS5v5":
        cls = type("VecVSS5v5Env", (vec.VecVSSEnv,), dict(N_BLUE=5, N_YELLOW=5))
        return cls(n, field_type=1, **kw)
    return getattr(vec, name)(n, **kw)


def _policy(env, **kw):
    from rsoccer_amd.vec.policy import MLPPolicy
    return MLPPolicy(env.sim.obs_dim, env.sim.act_dim, **kw)


def _dense(torch, pol, k, seed=5):
    """[k, P] uniform in [-0.5, 0.5), drawn on the host (the same on every machine)"""
    p = np.random.default_rng(seed).uniform(-0.5, 0.5, (k, pol.num_params)).astype(np.float32)
    return torch.from_numpy(p)


def _start(torch, env, warm=WARM):
    env.reset()
    if warm:
        env.step_random(warm)
    torch.cuda.synchronize()


def _call(env, pol, params, horizon=H, gamma=0.97):
    return _host(env.lookahead_policy(pol, params, horizon, gamma=gamma, return_obs=True, return_actions=True, return_policy_obs=True))


def _simulated(out):
    """[B, K, H] bool: the steps a pair simulated"""
    return np.arange(out["actions"].shape[2])[None, None, :] < out["steps"][:, :, None]


def _check_contract(torch, env, out, gamma=0.97, tag=""):
    """lookahead(actions) and restore + step(actions) reproduce the call"""
    acts = torch.from_numpy(out["actions"]).to(env.device)
    la = _host(env.lookahead(acts, gamma=gamma, return_obs=True))
    for key in ("steps", "terminated", "truncated", "return", "last_obs"):
        assert _same(out[key], la[key]), (tag, key, out[key], la[key])
    sim = _simulated(out)
    blob = env.checkpoint()
    for k in range(acts.shape[1]):
        env.restore(blob)
        for t in range(acts.shape[2]):
            torch.cuda.synchronize()
            seen = env._t["obs"].cpu().numpy()
            run = sim[:, k, t]
            assert _same(seen[run], out["policy_obs"][run, k, t]), (tag, "policy_obs", k, t)
            env.step(acts[:, k, t])
    env.restore(blob)
    torch.cuda.synchronize()
    # entries of steps a pair did not simulate are not written: the tensors are handed out zeroed
    assert not out["actions"][~sim].any() and not out["policy_obs"][~sim].any(), tag
    assert out["actions"][sim].any() and np.all(np.abs(out["actions"]) <= 1.0), tag


# ---- 1. the contract, every task class ----
@pytest.mark.parametrize("name", CLASSES)
def test_recorded_actions_reproduce_the_call(name):
    import torch
    from rsoccer_amd import vec
    env = _make(vec, name, B, device=0, seed=2025)
    _start(torch, env)
    pol = _policy(env)
    out = _call(env, pol, _dense(torch, pol, K))
    print(name, "steps", out["steps"].min(), out["steps"].max(), "return", out["return"].min(), out["return"].max())
    assert out["steps"].max() == H
    _check_contract(torch, env, out, tag=name)
    env.close()


# ---- 2. the policy's arithmetic, exact ----
def _selector(torch, pol, k, scale_exp=0, signed_pair=False):
    """Policy k of a family whose every fmaf is exact: weights 0 or +-2^n, biases 0.  Hidden unit j of layer 1 copies observation
    component (7 j + 3 k + 1) mod obs_dim, negated when j + k is odd; a second hidden layer is a permutation of the first; output a
    is h_i - h_j.  signed_pair: hidden units 2 a and 2 a + 1 carry +-2^scale_exp times one component, so that after the relu
    output a is exactly 2^scale_exp * obs_i (the tanh measurement)."""
    OD, AD, h = pol.obs_dim, pol.act_dim, pol.hidden
    ts = [torch.zeros(s) for s in pol.shapes]
    w1 = ts[0]
    for j in range(h):
        if signed_pair:
            w1[j, (5 * (j // 2) + 3 * k + 1) % OD] = (1.0 if j % 2 == 0 else -1.0) * 2.0 ** scale_exp
        else:
            w1[j, (7 * j + 3 * k + 1) % OD] = 1.0 if (j + k) % 2 == 0 else -1.0
    perm = lambda j: j
    if pol.layers == 2:
        perm = lambda j: (5 * j + k) % h   # unit j of layer 2 copies unit perm(j) of layer 1 (5 is coprime to 32 and 64)
        for j in range(h):
            ts[2][j, perm(j)] = 1.0
    inv = {perm(j): j for j in range(h)}
    wo = ts[-2]
    for a in range(AD):
        i, j = (2 * a, 2 * a + 1) if signed_pair else ((2 * a + k) % h, (2 * a + 9 + 3 * k) % h)
        wo[a, inv[i]] = 1.0
        wo[a, inv[j]] = -1.0
    return pol.pack(ts)


@pytest.mark.parametrize("layers,hidden", [(1, 32), (1, 64), (2, 32), (2, 64)])
def test_selector_policies_are_evaluated_exactly(layers, hidden):
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(B, device=0, seed=11)
    _start(torch, env)
    pol = _policy(env, hidden=hidden, layers=layers, hidden_act="relu", out_act="clip")
    params = torch.stack([_selector(torch, pol, k) for k in range(K)])
    out = _call(env, pol, params)
    sim = _simulated(out)
    pobs = torch.from_numpy(out["policy_obs"])
    for k in range(K):
        want = pol.forward(pobs[:, k], params[k], dtype=torch.float32).numpy()   # on the host: every operation is exact
        assert _same(out["actions"][:, k][sim[:, k]], want[sim[:, k]]), k
    # informative: the policies differ and act
    assert out["actions"][sim].any()
    assert not _same(out["actions"][:, 0], out["actions"][:, 1]) and not _same(out["actions"][:, 1], out["actions"][:, 2])
    _check_contract(torch, env, out, tag=f"selector {layers}x{hidden}")
    env.close()


# ---- 3. the policy's arithmetic, dense ----
def _tanh_deviation(torch, env):
    """largest |kernel tanh - float64 tanh| on inputs 2^n * obs_i, which the kernel forms exactly (see _selector)"""
    pol = _policy(env, hidden=64, layers=1, hidden_act="relu", out_act="tanh")
    exps = [-3, -2, -1, 0, 1, 2]   # |obs| <= 1.2: inputs cover [-4.8, 4.8]
    kk = 24
    params = torch.stack([_selector(torch, pol, k, scale_exp=exps[k % len(exps)], signed_pair=True) for k in range(kk)])
    out = _call(env, pol, params)
    sim = _simulated(out)
    worst, lo, hi = 0.0, 0.0, 0.0
    for k in range(kk):
        x = torch.from_numpy(out["policy_obs"][:, k]).double()
        pre = pol.forward(x, params[k].double().clone(), dtype=torch.float64)   # only to assert the construction below
        idx = [(5 * a + 3 * k + 1) % pol.obs_dim for a in range(pol.act_dim)]
        arg = x[..., idx] * 2.0 ** exps[k % len(exps)]
        assert torch.equal(torch.tanh(arg), pre)
        dev = (torch.from_numpy(out["actions"][:, k]).double() - torch.tanh(arg)).abs().numpy()[sim[:, k]]
        worst = max(worst, float(dev.max()))
        lo, hi = min(lo, float(arg.min())), max(hi, float(arg.max()))
    return worst, lo, hi


def test_tanh_allowance_is_measured():
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(B, device=0, seed=2025)
    _start(torch, env)
    worst, lo, hi = _tanh_deviation(torch, env)
    print(f"kernel tanh vs float64 tanh: largest deviation {worst:.3e} over inputs in [{lo:.2f}, {hi:.2f}]")
    assert lo < -2.0 and hi > 2.0, "uninformative: the inputs do not reach the tails"
    assert worst <= 4 * TANH_DEV
    env.close()


def _forward_with_bound(torch, pol, obs, params):
    """float64 forward pass and, per output, a bound on what sequential float32 fmaf accumulation may deviate from it: per unit
    (n + 1) u (|b| + sum |w_i x_i|) rounding (standard forward error, x the float32 inputs the kernel sees, bounded by |x| + delta),
    sum |w_i| delta_i inherited from the layer below, and 4 TANH_DEV per tanh; the activations are 1-Lipschitz."""
    ts = [t.double() for t in pol.unpack(params)]
    x, delta = obs.double(), torch.zeros_like(obs, dtype=torch.float64)
    n_layers = len(ts) // 2
    for li in range(n_layers):
        w, b = ts[2 * li], ts[2 * li + 1]
        n = w.shape[1]
        pre = x @ w.T + b
        mag = (x.abs() + delta) @ w.abs().T + b.abs()
        delta = delta @ w.abs().T + (n + 1) * U * mag
        act = (pol.hidden_act if li + 1 < n_layers else pol.out_act)
        if act == "tanh":
            x, delta = torch.tanh(pre), delta + 4 * TANH_DEV
        elif act == "relu":
            x = torch.relu(pre)
        else:
            x = pre.clamp(-1.0, 1.0)
    return x, delta


@pytest.mark.parametrize("name", CLASSES)
def test_dense_policies_are_within_the_float32_bound(name):
    import torch
    from rsoccer_amd import vec
    env = _make(vec, name, B, device=0, seed=2025)
    _start(torch, env)
    pol = _policy(env)
    params = _dense(torch, pol, K)
    out = _call(env, pol, params)
    sim = _simulated(out)
    for k in range(K):
        want, bound = _forward_with_bound(torch, pol, torch.from_numpy(out["policy_obs"][:, k]), params[k])
        assert torch.allclose(want, pol.forward(torch.from_numpy(out["policy_obs"][:, k]), params[k]), rtol=0, atol=1e-12)
        err = (torch.from_numpy(out["actions"][:, k]).double() - want).abs().numpy()
        print(name, k, "largest error", err[sim[:, k]].max(), "smallest bound", float(bound.min()), "worst error / bound",
              (err / bound.numpy())[sim[:, k]].max())
        assert np.all(err[sim[:, k]] <= bound.numpy()[sim[:, k]]), (name, k)
    env.close()


# ---- 4. stops ----
@pytest.mark.parametrize("warm", [0, 2])
def test_pairs_stop_at_the_time_limit(warm):
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(B, device=0, seed=4, max_episode_steps=4)
    _start(torch, env, warm)
    done = env._t["steps"].cpu().numpy().astype(np.int64)
    assert np.all(done == warm)
    pol = _policy(env)
    out = _call(env, pol, _dense(torch, pol, K))
    assert np.array_equal(out["steps"], np.broadcast_to((4 - done)[:, None], (B, K)))
    assert out["truncated"].all()
    sim = _simulated(out)
    assert not out["actions"][~sim].any() and not out["policy_obs"][~sim].any()
    _check_contract(torch, env, out, tag=f"time limit, {warm} steps in")
    env.close()


@pytest.mark.parametrize("name", ["VecSSLStaticDefendersEnv", "VecSSLContestedPossessionEnv"])
def test_pairs_stop_at_a_termination(name):
    import torch
    from rsoccer_amd import vec
    env = getattr(vec, name)(256, device=0, seed=7)
    env.reset()
    env.step_random(25)
    torch.cuda.synchronize()
    pol = _policy(env)
    out = _call(env, pol, _dense(torch, pol, 4, seed=101), horizon=40, gamma=1.0)
    print(name, "terminated pairs", int(out["terminated"].sum()), "of", out["terminated"].size)
    assert out["terminated"].any() and not out["terminated"].all(), "uninformative: no mix of ended and running pairs"
    assert np.all((out["steps"] < 40) <= out["terminated"])
    acts = torch.from_numpy(out["actions"]).to(env.device)
    la = _host(env.lookahead(acts, gamma=1.0, return_obs=True))
    for key in ("steps", "terminated", "truncated", "return", "last_obs"):
        assert _same(out[key], la[key]), key
    sim = _simulated(out)
    assert not out["actions"][~sim].any() and not out["policy_obs"][~sim].any()
    env.close()


# ---- 5. independence ----
def test_policies_and_envs_do_not_see_each_other():
    import torch
    from rsoccer_amd import vec
    env = vec.VecSSLStaticDefendersEnv(B, device=0, seed=8)
    _start(torch, env)
    pol = _policy(env)
    params = _dense(torch, pol, K)
    full = _call(env, pol, params)
    for k in range(K):
        one = _call(env, pol, params[k:k + 1])
        for key, v in one.items():
            assert _same(v[:, 0], full[key][:, k]), (k, key)
    env.close()
    big = vec.VecSSLStaticDefendersEnv(17, device=0, seed=8)
    _start(torch, big)
    wide = _call(big, pol, params)
    for key, v in full.items():
        assert _same(v, wide[key][:B]), key
    big.close()


# ---- 6. the handle is untouched ----
@pytest.mark.parametrize("device_keyed", [False, True])
def test_the_handle_is_left_exactly_as_it_was(device_keyed):
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(B, device=0, seed=12, max_episode_steps=30)
    _start(torch, env)
    if device_keyed:
        env.enable_graph_capture()
        env.step(None)
    torch.cuda.synchronize()
    before = env.checkpoint()
    views = {k: env._t[k].clone() for k in ("obs", "reward", "terminated", "truncated", "final_obs", "info", "steps")}
    tick = env.sim.task_tick()
    pol = _policy(env)
    out = _call(env, pol, _dense(torch, pol, K))
    assert out["steps"].max() > 0
    assert np.array_equal(env.checkpoint(), before)
    assert env.sim.task_tick() == tick
    for k, v in views.items():
        assert torch.equal(env._t[k], v), k
    env.close()


# ---- 7. layouts and physics ----
def test_16_lanes_per_env_give_the_same_bits(monkeypatch):
    import torch
    from rsoccer_amd import vec
    outs = []
    for lanes in (None, "16"):
        if lanes:
            monkeypatch.setenv("RSX_LANES_PER_ENV", lanes)
        env = vec.VecVSSEnv(B, device=0, seed=29)
        assert env.sim.task_layout() == ("16-lanes-per-env" if lanes else "8-lanes-per-env"), env.sim.task_layout()
        _start(torch, env)
        pol = _policy(env)
        outs.append(_call(env, pol, _dense(torch, pol, K)))
        if lanes:
            _check_contract(torch, env, outs[-1], tag="16 lanes")
        env.close()
    for key, v in outs[0].items():
        assert _same(v, outs[1][key]), key


def test_vss_5v5_native_16_lanes():
    import torch
    from rsoccer_amd import vec
    env = _make(vec, "VecVSS5v5", B, device=0, seed=29)
    assert env.sim.obs_dim == 64
    _start(torch, env)
    pol = _policy(env)
    _check_contract(torch, env, _call(env, pol, _dense(torch, pol, K)), tag="5v5")
    env.close()


@pytest.mark.parametrize("id_,ranges", [("VSS-v0", {"m_ball": (0.04, 0.05), "mu_g": (0.2, 0.4)}),
                                        ("SSLStaticDefenders-v0", {"m_ball": (0.04, 0.05), "e_rb": (0.2, 0.6)})])
def test_per_env_physics(id_, ranges):
    import torch
    import rsoccer_amd
    env = rsoccer_amd.make_vec(id_, B, device=0, seed=31, max_episode_steps=20, physics_ranges=ranges)
    _start(torch, env, 45)   # two auto-resets per env: the coefficients were redrawn and differ per env
    assert len(np.unique(env.physics()["m_ball"].cpu().numpy())) > 1
    pol = _policy(env)
    _check_contract(torch, env, _call(env, pol, _dense(torch, pol, K)), tag=id_)
    env.close()


# ---- 8. graph ----
def test_policy_lookahead_then_step_replays_from_a_graph():
    import torch
    from rsoccer_amd import vec
    envs = [vec.VecVSSEnv(B, device=0, seed=17, max_episode_steps=40) for _ in range(2)]
    for env in envs:
        _start(torch, env)
        env.enable_graph_capture()
    env, twin = envs
    pol = _policy(env)
    params = _dense(torch, pol, K).to(env.device)

    def evaluate_and_act(e):
        out = e.lookahead_policy(pol, params, H, gamma=0.97, return_obs=True, return_actions=True, return_policy_obs=True)
        e.step(out["actions"][:, 0, 0])
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # torch's warm-up before a capture: real calls, the twin makes them too
        evaluate_and_act(env)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    evaluate_and_act(twin)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = evaluate_and_act(env)
    assert env.sim.task_tick() == twin.sim.task_tick() == WARM + 1   # capturing enqueued nothing
    for i in range(3):
        g.replay()
        want = evaluate_and_act(twin)
        torch.cuda.synchronize()
        for key in want:
            assert torch.equal(out[key], want[key]), (i, key)
        for key in ("obs", "reward", "terminated", "truncated", "final_obs"):
            assert torch.equal(env._t[key], twin._t[key]), (i, key)
    assert env.sim.task_tick() == twin.sim.task_tick() == WARM + 4
    assert np.array_equal(env.checkpoint(), twin.checkpoint())
    for e in envs:
        e.close()


def test_captured_call_on_a_host_keyed_handle_is_refused():
    import torch
    from rsoccer_amd import _lib, vec
    env = vec.VecVSSEnv(B, device=0, seed=3)
    env.reset()
    env.step(None)
    torch.cuda.synchronize()
    before = env.checkpoint()
    pol = _policy(env)
    params = _dense(torch, pol, K).to(env.device)
    side = torch.cuda.Stream()
    with pytest.raises(_lib.RsxError, match="rsx_task_enable_capture"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
            env.lookahead_policy(pol, params, 4)
    torch.cuda.synchronize()
    _lib.drop_pending_hip_error()   # what the aborted capture leaves behind
    assert np.array_equal(env.checkpoint(), before)   # nothing ran
    env.step(None)                                    # the env still steps ...
    out = env.lookahead_policy(pol, params, 4)        # ... and evaluates, eagerly
    torch.cuda.synchronize()
    assert env.sim.task_tick() == 2 and int(out["steps"].min()) == 4
    env.close()


# ---- 9. refusals ----
def test_refusals():
    import torch
    from rsoccer_amd import _lib, vec
    from rsoccer_amd.vec.policy import MLPPolicy
    dev = torch.device("cuda", 0)
    sim = _lib.Sim(_lib.KIND_VSS, 0, 3, 3, 25, 16, 0)
    sim.task_attach(_lib.TASK_VSS_V0, 1, 0, 0)
    pol = MLPPolicy(sim.obs_dim, sim.act_dim)
    assert sim.policy_num_params(pol.spec()) == pol.num_params
    p = torch.zeros(2, pol.num_params, device=dev)
    r = torch.full((16, 2), 7.0, device=dev)
    s = torch.full((16, 2), -1, dtype=torch.int32, device=dev)
    f = torch.zeros(16, 2, dtype=torch.uint8, device=dev)

    def call(spec=pol.spec(), K=2, H=3, gamma=1.0, pp=p.data_ptr(), rp=r.data_ptr()):
        sim.task_lookahead_policy(spec, pp, K, H, gamma, rp, s.data_ptr(), f.data_ptr(), None, None, None, None)

    with pytest.raises(_lib.RsxError, match="reset"):
        call()
    sim.task_reset()
    bad_specs = [_lib.PolicyMLP(2, 48, _lib.ACT_TANH, _lib.ACT_TANH), _lib.PolicyMLP(3, 64, _lib.ACT_TANH, _lib.ACT_TANH),
                 _lib.PolicyMLP(0, 64, _lib.ACT_TANH, _lib.ACT_TANH), _lib.PolicyMLP(2, 64, 7, _lib.ACT_TANH),
                 _lib.PolicyMLP(2, 64, _lib.ACT_CLIP, _lib.ACT_TANH), _lib.PolicyMLP(2, 64, _lib.ACT_TANH, _lib.ACT_RELU),
                 _lib.PolicyMLP(2, 64, _lib.ACT_TANH, -1)]
    for bad in [dict(spec=b) for b in bad_specs] + [dict(spec=None), dict(K=0), dict(H=0), dict(gamma=float("nan")),
                                                      dict(gamma=float("inf")), dict(pp=None), dict(rp=None)]:
        with pytest.raises(_lib.RsxError):
            call(**bad)
    for b in bad_specs:
        with pytest.raises(_lib.RsxError):
            sim.policy_num_params(b)
    torch.cuda.synchronize()
    assert int(s.max()) == -1 and float(r.min()) == 7.0   # nothing was enqueued
    call()
    torch.cuda.synchronize()
    assert int(s.min()) == 3   # the valid call ran
    sim.close()

    # the scrimmage commands every robot: refused by the engine even for a policy of its dims
    scr = vec.VecSSLScrimmageEnv(B, device=0, seed=1)
    scr.reset()
    spol = MLPPolicy(scr.sim.obs_dim, scr.sim.act_dim)
    with pytest.raises(_lib.RsxError, match="scrimmage"):
        scr.lookahead_policy(spol, torch.zeros(1, spol.num_params), 3)
    with pytest.raises(_lib.RsxError, match="scrimmage"):
        scr.sim.policy_num_params(spol.spec())
    scr.close()

    env = vec.VecVSSEnv(16, device=0, seed=1)
    good = torch.zeros(2, pol.num_params, device=dev)
    with pytest.raises(_lib.RsxError, match="reset"):
        env.lookahead_policy(pol, good, 3)
    env.reset()
    torch.cuda.synchronize()
    before = env.checkpoint()
    for kw in (dict(hidden=48), dict(layers=3), dict(hidden_act="gelu"), dict(out_act="relu")):
        with pytest.raises(ValueError):
            MLPPolicy(env.sim.obs_dim, env.sim.act_dim, **kw)
    for shape in ((2, pol.num_params - 1), (2, pol.num_params + 1), (pol.num_params,), (0, pol.num_params), (1, 2, pol.num_params)):
        with pytest.raises(ValueError):
            env.lookahead_policy(pol, torch.zeros(*shape, device=dev), 3)
    for kw in (dict(horizon=0), dict(horizon=3, gamma=float("nan")), dict(horizon=3, gamma=float("inf"))):
        with pytest.raises(ValueError):
            env.lookahead_policy(pol, good, **kw)
    with pytest.raises(ValueError):   # a policy for another task's dims
        env.lookahead_policy(MLPPolicy(24, 5), torch.zeros(2, MLPPolicy(24, 5).num_params), 3)
    assert np.array_equal(env.checkpoint(), before)
    # numpy and float64 parameters are converted the way step() converts actions
    a = env.lookahead_policy(pol, np.zeros((2, pol.num_params)), 3, return_obs=True, return_actions=True)
    b = env.lookahead_policy(pol, good, 3, return_obs=True, return_actions=True)
    for k in b:
        assert torch.equal(a[k], b[k])
    assert "policy_obs" not in b and b["actions"].shape == (16, 2, 3, 2)
    env.close()
