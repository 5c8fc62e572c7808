"""The training-side kernels beyond one trip of their grids.  Six kernels walk their input with a grid-stride loop whose grid is capped
by a constant of the build (docs/VERIFICATION.md, "Beyond one trip of the grid"): gae_values_rows_kernel<H, 2> (512 workgroups x 2 waves
x 64 rows), gae_values_rows_kernel<H, 1> (768 x 64), gae_values_groups_kernel (768 x 8), adv_moments_kernel (128 x 256),
grad_norm_kernel (64 x 256) and mlp_grad_kernel at the default max_workgroups (512 x 64, then ppo_reduce_kernel over 512 partials).
Every case here passes a size at which the loop takes a second trip and compares with what the single-trip sizes of
test_gpu_advantages.py, test_gpu_ppo_grad.py and test_gpu_ppo_update.py pin: on bit patterns, or under those files' own criteria
taken over unchanged.  The permutation beyond 11 bits and inputs that start one float into an allocation belong with it."""
import functools

import numpy as np
import pytest

import ppo_update_helpers as H
import test_gpu_advantages as A
import test_gpu_policy_lookahead as PL
import test_gpu_ppo_grad as G
import test_gpu_ppo_update as UP

pytestmark = pytest.mark.gpu

_same, _bits, _dense, _make, _host = PL._same, PL._bits, PL._dense, PL._make, A._host
NONE, TERM, TRUNC, BOTH = A.NONE, A.TERM, A.TRUNC, A.BOTH


@pytest.fixture(scope="module")
def handles():
    """handles that are never reset and never stepped, made on first use: the calls need only their device, obs_dim and act_dim
    (n_envs is the batch's and not the handle's)"""
    from rsoccer_amd import vec
    made = {}

    def get(name):
        if name not in made:
            made[name] = _make(vec, name, 9, device=0, seed=1)
        return made[name]
    yield get
    for env in made.values():
        env.close()


# ---- 1. values and advantages beyond one trip ----
T_BIG, B_BIG = 9, 14571          # T B = 131 139 = 2 049 * 64 + 3; T B + B = 145 710
# the three launches of the values: (rows per chunk, rows per trip of the whole grid); a chunk is what one wave takes per trip
FORMS = {"rows, two waves": (64, 512 * 2 * 64), "rows, one wave": (64, 768 * 64), "groups": (8, 768 * 8)}
# truncated-only rows forced where chance (one row in 500) might leave a trip of a form without one: behind the first 4 096 rows in the
# groups form's first trip; in the second trip of each form in a chunk whose wave took a chunk of the first 4 096 rows before (rows
# 6 144 + 20, 49 152 + 70, 65 536 + 70); in the groups form's last trip; in chunk 2 048, the first of the two-wave form's ragged third trip
FORCED_TRUNC = (5000, 6164, 49222, 65606, 129100, 131080)


@functools.lru_cache(maxsize=None)
def _big_kinds():
    """[T][B] kinds: truncated-only rows about one in 500 and none in the first 4 096 flat rows; terminated and both-flags rows at
    6 % and 4 %, so that every bootstrap rule has thousands of rows"""
    n = T_BIG * B_BIG
    rng = np.random.default_rng(20251)
    kind = rng.choice([NONE, TERM, BOTH], p=[0.90, 0.06, 0.04], size=n).astype(np.int64)
    kind[rng.random(n) < 1.0 / 500.0] = TRUNC
    head = kind[:4096]
    head[head == TRUNC] = NONE
    kind[list(FORCED_TRUNC)] = TRUNC
    tail = kind[2049 * 64:]   # the 3 rows of the ragged last chunk: a chunk without such a row next to chunk 2 048, which has one
    tail[tail == TRUNC] = NONE
    return kind.reshape(T_BIG, B_BIG)


def _census(only_flat, chunk, stride):
    """per trip of a form the chunks with and without a truncated-only row in the tail pass (which walks the T B rows), and whether
    some wave meets a chunk without one and, on a later trip, one with"""
    n = only_flat.size
    slots = stride // chunk
    n_chunks = -(-n // chunk)
    trips = -(-n_chunks // slots)
    rows = np.zeros(trips * slots * chunk, dtype=bool)
    rows[:n] = only_flat
    has = rows.reshape(trips, slots, chunk).any(-1)
    exists = (np.arange(trips * slots) < n_chunks).reshape(trips, slots)
    without = ~has & exists
    per_trip = [(int((has[k] & exists[k]).sum()), int(without[k].sum())) for k in range(trips)]
    skipped_before = np.cumsum(without, axis=0) - without > 0   # a chunk without one on an earlier trip of the same wave
    return per_trip, bool((has & skipped_before).any())


def _check_the_flags_exercise_every_trip(kind):
    only = (kind == TRUNC).reshape(-1)
    n = only.size
    assert n == 131139 == 2049 * 64 + 3 and n + B_BIG == 145710
    assert not only[:4096].any() and 0.5 / 500 < only.mean() < 2.0 / 500
    want_trips = {"rows, two waves": (3, 3), "rows, one wave": (3, 3), "groups": (22, 24)}   # (tail pass, main pass)
    for form, (chunk, stride) in FORMS.items():
        per_trip, skip_then_work = _census(only, chunk, stride)
        assert (len(per_trip), -(-(n + B_BIG) // stride)) == want_trips[form], (form, len(per_trip))
        for k, (with_, without) in enumerate(per_trip):
            assert with_ > 0 and without > 0, (form, "trip", k, with_, without)
        assert skip_then_work, (form, "no wave skips a chunk and works on a later one")
    # the obs / last_obs boundary lies inside a wave (and inside a group of eight rows) of the last trip
    assert n % 64 != 0 and n % 8 != 0 and n // 65536 == 2 and n // 49152 == 2


def _values_in_slices(torch, env, critic, params, rows, step=4096):
    """V of every row of ``rows`` [n, obs_dim], passed as T = 1 batches of at most 4 096 rows: single-trip launches of the default form"""
    dev, out = env.device, []
    for lo in range(0, rows.shape[0], step):
        x = rows[lo:lo + step]
        b = x.shape[0]
        z = torch.zeros((1, b), dtype=torch.bool, device=dev)
        batch = {"obs": x[None], "reward": torch.zeros((1, b), device=dev), "terminated": z, "truncated": z, "next_obs": x}
        out.append(env.advantages(batch, critic, params)["value"][0])
    return torch.cat(out).cpu().numpy()


def _all_values(env, batch, critic, params):
    """V of the T B rows of obs and the B rows of next_obs through ONE call on flags that end nothing (next_value's last row is V(next_obs))"""
    out = env.advantages(batch, critic, params, return_next_values=True)
    return np.concatenate([out["value"].cpu().numpy().reshape(-1), out["next_value"][-1].cpu().numpy()])


BIG_CASES = [("VecVSSEnv", 40, 64, 2, "tanh", "rows, two waves"), ("VecVSSEnv", 40, 32, 1, "relu", "rows, two waves"),
             ("VecVSS5v5", 64, 64, 2, "tanh", "rows, one wave"), ("VecSSLDribblingEnv", 21, 64, 2, "tanh", "rows, two waves")]


@pytest.mark.parametrize("name,obs_dim,hidden,layers,act,default_form", BIG_CASES)
def test_values_and_advantages_do_not_depend_on_the_trip(handles, name, obs_dim, hidden, layers, act, default_form, monkeypatch):
    """9 x 14 571 rows: a ragged third trip in both rows forms and 24 trips in the groups form.  (The selector critics are relu ones of
    the case's layers and units — the kernel's instantiation; with tanh no float32 host forward is exact.)"""
    import torch
    T, B = T_BIG, B_BIG
    kind = _big_kinds()
    _check_the_flags_exercise_every_trip(kind)   # a precondition on the inputs, before any device call
    env = handles(name)
    dev, OD = env.device, env.sim.obs_dim
    assert OD == obs_dim
    critic = A._critic(env, hidden=hidden, layers=layers, hidden_act=act)
    assert default_form in FORMS   # (which rows launch the case's default is: two hidden layers of 64 at 64 floats leave LDS for one wave)
    params_host = _dense(torch, critic, 1, seed=7)[0]
    params = params_host.to(dev)
    term, trunc = (kind & 1).astype(bool), (kind & 2).astype(bool)
    end, only, run = term | trunc, trunc & ~term, ~(term | trunc)
    rng = np.random.default_rng(1000 * OD + hidden)
    obs = rng.uniform(-1.2, 1.2, (T, B, OD)).astype(np.float32)
    last = rng.uniform(-1.2, 1.2, (B, OD)).astype(np.float32)
    rew = rng.normal(0.0, 1.0, (T, B)).astype(np.float32)
    fin = np.full((T, B, OD), np.nan, np.float32)   # NaN wherever the call must not look
    fin[only] = rng.uniform(-1.2, 1.2, (int(only.sum()), OD)).astype(np.float32)
    batch = A._batch(torch, dev, obs, rew, term, trunc, last, fin)
    quiet = {k: v for k, v in batch.items() if k != "final_obs"}
    quiet["terminated"] = quiet["truncated"] = torch.zeros((T, B), dtype=torch.bool, device=dev)
    every_row = torch.cat([batch["obs"].reshape(-1, OD), batch["next_obs"]])
    assert every_row.shape[0] == 145710

    # the references, each computed once: the single-trip slices (default form), the float32 host forward of the selectors, float64
    monkeypatch.delenv("RSX_GAE_FORM", raising=False)
    v_slices = _values_in_slices(torch, env, critic, params, every_row)
    v_fin = _values_in_slices(torch, env, critic, params, batch["final_obs"][torch.from_numpy(only).to(dev)])
    assert v_slices.shape == (145710,) and v_fin.shape == (int(only.sum()),) and np.all(np.isfinite(v_slices)) and np.all(np.isfinite(v_fin))
    host_rows = every_row.cpu()
    sel = A._critic(env, hidden=hidden, layers=layers, hidden_act="relu")
    selectors = [PL._selector(torch, sel, k) for k in range(3)]
    sel_want = [sel.forward(host_rows, p, dtype=torch.float32).numpy()[..., 0] for p in selectors]
    want64, bound = A._forward_with_bound(torch, critic, host_rows, params_host)
    want64, bound = want64.numpy()[:, 0], bound.numpy()[:, 0]

    outs = {}
    for form in ("default", "groups"):
        if form == "groups":
            monkeypatch.setenv("RSX_GAE_FORM", "groups")
        # ---- independent arithmetic, on every one of the 145 710 rows ----
        for k, (p, want) in enumerate(zip(selectors, sel_want)):
            got = _all_values(env, quiet, sel, p)
            assert _same(got, want), (form, "selector", k, A._where(got, want))
            assert got.any()
        got = _all_values(env, quiet, critic, params)
        assert _same(got, v_slices), (form, "one call on flags that end nothing", A._where(got, v_slices))
        err = np.abs(got.astype(np.float64) - want64)
        print(name, hidden, layers, act, form, "worst error / bound", float((err / bound).max()))
        assert np.all(err <= bound), (form, "dense critic", float((err / bound).max()))
        # ---- the batch with its flags ----
        for gamma, lam in ((0.99, 0.95), (1.0, 1.0)):
            for with_final in (True, False):
                b = dict(batch)
                if not with_final:
                    del b["final_obs"]
                out = _host(env.advantages(b, critic, params, gamma=gamma, lam=lam, return_next_values=True))
                tag = (name, form, gamma, lam, with_final)
                v, nv = out["value"], out["next_value"]
                for key in ("value", "advantage", "return", "next_value"):
                    assert out[key].shape == (T, B) and out[key].dtype == np.float32 and np.all(np.isfinite(out[key])), (tag, key)
                # independence of the grid
                assert _same(v.reshape(-1), v_slices[:T * B]), (tag, "value", A._where(v.reshape(-1), v_slices[:T * B]))
                assert _same(nv[-1][run[-1]], v_slices[T * B:][run[-1]]), (tag, "the last row bootstraps from V(last_obs)")
                if with_final:
                    assert _same(nv[only], v_fin), (tag, "truncated-only rows bootstrap from V(final_obs)", A._where(nv[only], v_fin))
                else:
                    assert not _bits(nv[only]).any(), (tag, "without final_obs truncated-only rows bootstrap from exactly 0")
                assert _same(nv[:-1][run[:-1]], v[1:][run[:-1]]), (tag, "interior rows bootstrap from the next row's value")
                assert not _bits(nv[term]).any(), (tag, "terminated rows bootstrap from exactly 0")
                # the recurrence
                adv, ret = A._recurrence(v, nv, rew, end, gamma, lam)
                assert _same(out["advantage"], adv), (tag, "advantage", A._where(out["advantage"], adv))
                assert _same(out["return"], ret), (tag, "return", A._where(out["return"], ret))
                outs[(form, gamma, lam, with_final)] = out
    for (form, *rest), out in outs.items():
        if form == "groups":
            for key in out:
                assert _same(out[key], outs[("default", *rest)][key]), ("the two forms differ", rest, key)


def test_a_collected_batch_of_73800_rows_with_episode_ends():
    """test_gpu_advantages.py's real-batch and shared-layer checks at a size that takes a second trip: 8 x 8 200 + 8 200 rows"""
    import torch
    from rsoccer_amd import vec
    from rsoccer_amd.vec.policy import MLPPolicy
    T, B = 8, 8200
    envs = [vec.VecVSSEnv(B, device=0, seed=2025, max_episode_steps=5) for _ in range(2)]
    for e in envs:
        PL._start(torch, e, warm=2)   # rows 2 and 7 reach the TimeLimit: the tail pass's second trip (rows 65 536 ..., all of row 7) is live
    env, twin = envs
    pol = MLPPolicy(env.sim.obs_dim, env.sim.act_dim, hidden=64, layers=2, hidden_act="tanh", out_act="clip")
    critic = A._critic(env)
    params, cparams = A._shared(torch, pol, critic)
    plain = env.collect(pol, params, T, log_std=-1.0, noise_seed=5, return_final_obs=True)
    adv = env.advantages(plain, critic, cparams, gamma=0.97, lam=0.9)
    both = twin.collect(pol, params, T, log_std=-1.0, noise_seed=5, critic=critic, critic_params=cparams, gamma=0.97, lam=0.9)
    torch.cuda.synchronize()
    assert T * B == 65600 and T * B + B == 73800
    term, trunc = plain["terminated"].cpu().numpy(), plain["truncated"].cpu().numpy()
    only = (trunc & ~term).reshape(-1)
    print("terminated rows", int(term.sum()), "truncated-only rows", int(only.sum()), "of them behind row 65 536:", int(only[65536:].sum()))
    assert only[:65536].any() and only[65536:].any(), "uninformative: a trip of the tail pass without a truncated-only row"
    assert not only[:64].any(), "uninformative: the wave of chunk 0 does not skip before it works on chunk 1 024"
    for k in plain:
        assert _same(both[k].cpu().numpy(), plain[k].cpu().numpy()), k
    for k in ("value", "advantage", "return"):
        assert _same(both[k].cpu().numpy(), adv[k].cpu().numpy()), k
        assert np.all(np.isfinite(adv[k].cpu().numpy())), k
    value, mean0 = adv["value"].cpu().numpy(), plain["mean"][..., 0].cpu().numpy()
    assert _same(value, mean0), A._where(value, mean0)
    for e in envs:
        e.close()


# ---- 2. the two float64 reductions beyond one trip ----
@pytest.mark.parametrize("n", [32768, 32769, 65537, 100003, 786432])
def test_normalised_advantages_beyond_one_trip_of_128_workgroups(handles, n):
    """32 768 is the last single trip; 100 003 a ragged fourth one; 786 432 the workload's batch.  Mean 3 and standard deviation 0.5:
    Q - S * mean cancels five of every six leading bits.  The criterion is test_gpu_ppo_update.py's."""
    import torch
    env = handles("VecVSSEnv")
    gen = torch.Generator().manual_seed(n)
    adv = (0.5 * torch.randn(n, generator=gen) + 3.0).to(env.device)
    a64 = adv.double().cpu()
    ref = (a64 - a64.mean()) / (a64.std() + 1e-8)
    yard = (adv - adv.mean()) / (adv.std() + 1e-8)
    got, ms = env.normalize_advantages(adv, return_moments=True)
    again, ms2 = env.normalize_advantages(adv, return_moments=True)
    torch.cuda.synchronize()
    want, mean, std = H.normalize(adv.cpu().numpy())
    assert np.array_equal(ms.cpu().numpy().view(np.int32), np.array([mean, std], dtype=np.float32).view(np.int32)), (ms.tolist(), mean, std)
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    e_yard, e_got = UP._rel(yard, ref), UP._rel(got, ref)
    print(f"n = {n}: torch f32 {e_yard:.3e}, kernel {e_got:.3e}, ratio {e_got / e_yard:.2f}")
    assert e_yard > 0.0 and e_got <= 4.0 * e_yard, (e_got, e_yard)
    assert abs(float(ms[0]) - float(a64.mean())) <= 1e-6 and abs(float(ms[1]) - float(a64.std())) <= 1e-6
    assert torch.equal(UP._bits(got), UP._bits(again)) and torch.equal(UP._bits(ms), UP._bits(ms2)), "two runs differ"


# 8 450 / 2 / 8 385: VSS 5v5 with 2 x 64, what a user reaches (16 837 entries: a second trip of 64 workgroups x 256).  The others go
# through the C call, which takes free sizes: 16 384 entries, exactly 64 x 256 (the last single trip); 16 385, one thread's second
# element; 49 305, three trips and a ragged fourth with both tensor boundaries inside the second
ADAM_SIZES = [(8450, 2, 8385), (16382, 1, 1), (16382, 2, 1), (20000, 5, 29300)]


@pytest.mark.parametrize("gscale", [1.0, 1e-5])
@pytest.mark.parametrize("sizes", ADAM_SIZES)
def test_clip_and_adam_beyond_one_trip_of_64_workgroups(handles, sizes, gscale):
    """Three successive steps, the norm far above and far below max_norm as in test_gpu_ppo_update.ADAM_CASES, under that file's
    criterion; p, m, v and the norm equal the restatement in bits after every step."""
    import torch
    from rsoccer_amd import _lib
    from rsoccer_amd.vec.optim import PPOOptimizer
    env = handles("VecVSSEnv")
    dev = env.device
    LR, MAXN = 3e-3, 0.5
    f32 = dict(dtype=torch.float32, device=dev)
    if sizes == (8450, 2, 8385):
        pol, critic = UP._nets(64, 2, 64, 2)
        assert (pol.num_params, 2, critic.num_params) == sizes
        opt = PPOOptimizer(pol, critic, device=dev, lr=LR, max_grad_norm=MAXN)
        mine = list(UP._params(torch, pol, critic, 11, dev))
        m, v = opt.m, opt.v

        def step(grads):
            return opt.step(*mine, *grads)["grad_norm"]
    else:
        gen0 = torch.Generator().manual_seed(sum(sizes))
        mine = [(0.1 * torch.randn(n, generator=gen0)).to(dev) for n in sizes]
        m, v = [torch.zeros(n, **f32) for n in sizes], [torch.zeros(n, **f32) for n in sizes]
        counters = torch.zeros(4, dtype=torch.int64, device=dev)
        ws = torch.zeros(_lib.ADAM_WORKSPACE_BYTES // 8, dtype=torch.float64, device=dev)
        cfg = _lib.AdamCfg(0.9, 0.999, None, LR, 1e-8, MAXN, 0.0)
        state = _lib.AdamState(m[0].data_ptr(), v[0].data_ptr(), m[1].data_ptr(), v[1].data_ptr(), m[2].data_ptr(), v[2].data_ptr(),
                               counters.data_ptr(), *sizes)

        def step(grads):
            stats = torch.empty(2, **f32)
            io = _lib.AdamIo(*[x.data_ptr() for x in mine], *[g.data_ptr() for g in grads], None, stats.data_ptr(), ws.data_ptr())
            with torch.cuda.device(dev):
                _lib.adam_step(cfg, state, io, env._stream())
            return stats[0]
    t32 = [torch.nn.Parameter(x.clone()) for x in mine]
    t64 = [torch.nn.Parameter(x.double().cpu()) for x in mine]
    o32, o64 = torch.optim.Adam(t32, lr=LR), torch.optim.Adam(t64, lr=LR)
    host = [[x.cpu().numpy().copy() for x in mine], [np.zeros(n, np.float32) for n in sizes], [np.zeros(n, np.float32) for n in sizes]]
    gen = torch.Generator().manual_seed(5)
    for t in range(1, 4):
        grads = [gscale * torch.randn(n, generator=gen) for n in sizes]
        for x, g in zip(t32, grads):
            x.grad = g.to(dev)
        for x, g in zip(t64, grads):
            x.grad = g.double()
        torch.nn.utils.clip_grad_norm_(t32, MAXN)
        n64 = torch.nn.utils.clip_grad_norm_(t64, MAXN)
        o32.step(), o64.step()
        norm_dev = step([g.to(dev) for g in grads])
        torch.cuda.synchronize()
        assert (float(n64) > MAXN) == (gscale == 1.0)
        ref = {"p": [x.detach() for x in t64], "m": [o64.state[x]["exp_avg"] for x in t64], "v": [o64.state[x]["exp_avg_sq"] for x in t64]}
        yard = {"p": [x.detach() for x in t32], "m": [o32.state[x]["exp_avg"] for x in t32], "v": [o32.state[x]["exp_avg_sq"] for x in t32]}
        ker = {"p": mine, "m": m, "v": v}
        # the arithmetic of include/rsx.h, restated on the host
        P, M, V, norm = H.clip_adam(host[0], [g.numpy() for g in grads], host[1], host[2], t, LR, max_norm=MAXN)
        host = [P, M, V]
        assert np.float32(float(norm_dev)).tobytes() == np.float32(norm).tobytes(), (t, float(norm_dev), float(norm))
        for k, want in (("p", P), ("m", M), ("v", V)):
            for i in range(3):
                assert np.array_equal(ker[k][i].cpu().numpy().view(np.int32), want[i].view(np.int32)), (t, k, i)
        e_yard = {(k, i): UP._rel(yard[k][i], ref[k][i]) for k in ref for i in range(3)}
        e_ker = {(k, i): UP._rel(ker[k][i], ref[k][i]) for k in ref for i in range(3)}
        pooled = max(e_yard.values())
        w = max(e_ker, key=e_ker.get)
        print(f"{sizes} gscale {gscale} step {t}: torch f32 pooled {pooled:.3e}, kernel worst {e_ker[w]:.3e} {w}, ratio {e_ker[w] / pooled:.2f}")
        assert pooled > 0.0
        for k in e_ker:
            assert e_ker[k] <= 4.0 * pooled, (t, k, e_ker[k], pooled)


# ---- 3. the gradient launch at the default grid beyond 512 workgroups ----
M_BIG = 32833   # 514 blocks of 64 rows over 512 workgroups: workgroups 0 and 1 take a second block, the last block holds one row
GRAD_CASES = [("VecVSSEnv", "tanh", "perm"), ("VecVSS5v5", "relu", "repeats")]


@pytest.mark.parametrize("name,act,mode", GRAD_CASES)
def test_gradients_beyond_512_workgroups_at_the_default_grid(handles, name, act, mode):
    """test_gpu_ppo_grad.py's criterion, unchanged, with the inputs built as that file builds them (1 024 spare rows for its kink
    filter instead of 64: it may take 2 % out); the forward outputs against calls of at most 4 096 rows and against advantages()"""
    import torch
    env = handles(name)
    dev, M = env.device, M_BIG
    assert -(-M // 64) == 514
    pol, critic = G._nets(env, 64, 2, act)
    seed = 7 + M + 64 + 2
    data, removed, clipped = G._data(torch, pol, critic, M + 1024, seed)
    n = data["obs"].shape[0]
    assert n >= M
    rows = G._rows(torch, mode, M, n, seed)
    idx = rows.long()
    ref = G._autograd(torch, pol, critic, data, idx, torch.float64, "cpu")
    yard = G._autograd(torch, pol, critic, data, idx, torch.float32, dev)
    got = G._call(env, pol, critic, data, rows, max_workgroups=None, return_forward=True)
    again = G._call(env, pol, critic, data, rows, max_workgroups=None, return_forward=True)
    torch.cuda.synchronize()
    assert float(got["stats"]["rows_used"]) == float(M) and float(got["stats"]["rows_skipped"]) == 0.0
    flat = lambda o: torch.cat([o[k].reshape(-1) for k in ("grad_params", "grad_log_std", "grad_critic_params", "mean", "value")] +   # noqa: E731
                               [torch.stack(list(o["stats"].values()))]).view(torch.int32)
    assert torch.equal(flat(got), flat(again)), "two calls differ"
    ker = G._kernel(pol, critic, got)
    e_yard = {k: G._rel(yard[k], ref[k]) for k in ref}
    e_ker = {k: G._rel(ker[k], ref[k]) for k in ref}
    pooled = max(e_yard.values())
    worst = max(e_ker, key=e_ker.get)
    print(f"{name} 64x2 {act} M={M} {mode} wg=None: removed {removed}, clipped {clipped:.3f}, torch f32 pooled {pooled:.3e}, "
          f"kernel worst {e_ker[worst]:.3e} ({worst}), ratio {e_ker[worst] / pooled:.2f}")
    assert pooled > 0.0
    for k in ref:
        assert e_ker[k] <= 4.0 * pooled, (k, e_ker[k], pooled, e_ker[k] / pooled)
    # the forward pass: the same rows in calls of at most 4 096, and advantages()'s value
    mean, value = [], []
    for lo in range(0, M, 4096):
        part = G._call(env, pol, critic, data, rows[lo:lo + 4096], max_workgroups=None, return_forward=True)
        mean.append(part["mean"])
        value.append(part["value"])
    assert torch.equal(UP._bits(got["mean"]), UP._bits(torch.cat(mean))) and torch.equal(UP._bits(got["value"]), UP._bits(torch.cat(value)))
    obs = data["obs"].to(dev)
    z = torch.zeros((1, n), dtype=torch.bool, device=dev)
    adv = env.advantages({"obs": obs[None], "reward": torch.zeros((1, n), device=dev), "terminated": z, "truncated": z, "next_obs": obs},
                         critic, data["cparams"].to(dev))
    assert torch.equal(UP._bits(got["value"]), UP._bits(adv["value"][0][idx.to(dev)]))


# ---- 4. the permutation beyond 11 bits ----
@pytest.mark.parametrize("n", [32769, 65536, 65537, 786432, 1048577])
def test_the_permutation_beyond_11_bits(handles, n):
    """16 bits; 16 bits with slack 0; 17 bits (halves of 8 and 9) with the largest slack of that domain; 20 bits; 21 bits"""
    import torch
    from rsoccer_amd.vec.optim import PPOOptimizer
    env = handles("VecVSSEnv")
    assert H.perm_bits(n) == {32769: 16, 65536: 16, 65537: 17, 786432: 20, 1048577: 21}[n]
    seed, update, epoch = 0x1234567890ABCDEF, 2 ** 31 + 5, 3
    rows = env.minibatch_rows(n, seed, update, epoch)
    opt = PPOOptimizer(*UP._nets(), device=env.device)
    opt.counters[1] = update
    keyed = env.minibatch_rows(n, seed, opt, epoch)
    torch.cuda.synchronize()
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (n,)
    assert torch.equal(torch.sort(rows).values, torch.arange(n, dtype=torch.int32, device=env.device))
    assert torch.equal(rows, keyed), "update by value and update from the device's counters differ"
    assert np.array_equal(rows.cpu().numpy().astype(np.int64), H.permutation(n, seed, update, epoch))


# ---- 5. the whole update at a size where every piece trips ----
def test_ppo_update_equals_its_pieces_where_every_piece_trips():
    """A collected VSS-v0 batch of 26 x 2 693 = 70 018 rows, one epoch of two minibatches of 35 009 rows (548 blocks over 512
    workgroups), normalisation over 70 018 entries (three trips), 13 765 optimiser entries (one trip: section 2 has the others):
    test_gpu_ppo_update.py's composition case at this size"""
    import torch
    from rsoccer_amd import vec
    from rsoccer_amd.vec.optim import PPOOptimizer
    T, B, EPOCHS, MB, SEED = 26, 2693, 1, 2, 77
    env = vec.VecVSSEnv(B, device=0, seed=9, max_episode_steps=20)
    PL._start(torch, env)
    dev = env.device
    pol, critic = UP._nets()
    start = UP._params(torch, pol, critic, 31, dev)
    batch = env.collect(pol, start[0], T, log_std=start[1], noise_seed=4, critic=critic, critic_params=start[2])
    assert T * B == 70018 and [hi - lo for lo, hi in H.chunks(T * B, MB)] == [35009, 35009] and -(-35009 // 64) > 512
    before = {k: v.clone() for k, v in batch.items()}
    loss = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01)
    a, b = [x.clone() for x in start], [x.clone() for x in start]
    oa, ob = (PPOOptimizer(pol, critic, device=dev, lr=1e-3, max_grad_norm=0.5) for _ in range(2))
    for o in (oa, ob):
        o.counters[1] = 3
    out = env.ppo_update(batch, pol, *a[:2], critic, a[2], oa, epochs=EPOCHS, minibatches=MB, normalize_advantage=True, seed=SEED,
                         max_workgroups=None, **loss)
    want, _ = UP._piecewise(torch, env, batch, pol, critic, b, ob, EPOCHS, MB, SEED, True, None, **loss)
    torch.cuda.synchronize()
    stats = out["stats"]
    assert tuple(stats.shape) == (EPOCHS, MB, 10)
    assert torch.equal(UP._bits(stats[:, :, :8].reshape(EPOCHS * MB, 8)), UP._bits(want))
    assert torch.equal(UP._state_bits(torch, a, oa), UP._state_bits(torch, b, ob))
    assert oa.counters.tolist() == ob.counters.tolist() == [EPOCHS * MB, 4, EPOCHS * MB, 0]
    assert bool((stats[:, :, 9] == 1.0).all()) and bool((stats[:, :, 8] > 0.0).all())
    for x, s in zip(a, start):
        assert not torch.equal(UP._bits(x), UP._bits(s))
    assert np.array_equal(out["rows"].cpu().numpy().astype(np.int64), H.permutation(T * B, SEED, 3, EPOCHS - 1))
    for k in batch:   # (the collected batch carries its flags too: one byte per entry)
        assert torch.equal(batch[k].view(torch.uint8), before[k].view(torch.uint8)), k
    for row in stats[0]:
        assert float(row[6]) == 35009.0 and float(row[7]) == 0.0
    env.close()


# ---- 6. inputs that start one float into an allocation: the scalar loads at obs_dim % 4 == 0 ----
def _off_by_one_float(torch, t):
    """a contiguous view of t's contents that starts 4 bytes into a fresh allocation (the Python layer passes its address on)"""
    big = torch.full((t.numel() + 8,), float("nan"), dtype=t.dtype, device=t.device)
    view = big[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and t.data_ptr() % 16 == 0
    return view


@pytest.mark.parametrize("name,obs_dim", [("VecVSSEnv", 40), ("VecVSS5v5", 64)])
def test_misaligned_observations_give_the_aligned_calls_bits(handles, name, obs_dim, monkeypatch):
    import torch
    env = handles(name)
    dev, OD = env.device, env.sim.obs_dim
    assert OD == obs_dim and OD % 4 == 0
    # advantages: obs, final_obs and next_obs, each alone and all three
    T, B = 5, 70
    rng = np.random.default_rng(OD)
    kind, _ = A._flags(rng, T, B, 0)
    args = (rng.uniform(-1, 1, (T, B, OD)).astype(np.float32), rng.normal(0, 1, (T, B)).astype(np.float32), (kind & 1).astype(bool),
            (kind & 2).astype(bool), rng.uniform(-1, 1, (B, OD)).astype(np.float32), rng.uniform(-1, 1, (T, B, OD)).astype(np.float32))
    batch = A._batch(torch, dev, *args)
    critic = A._critic(env)
    cparams = _dense(torch, critic, 1, seed=9)[0].to(dev)
    for form in ("default", "groups"):
        if form == "groups":
            monkeypatch.setenv("RSX_GAE_FORM", "groups")
        want = _host(env.advantages(batch, critic, cparams, return_next_values=True))
        for keys in (("obs",), ("final_obs",), ("next_obs",), ("obs", "final_obs", "next_obs")):
            moved = {**batch, **{k: _off_by_one_float(torch, batch[k]) for k in keys}}
            got = _host(env.advantages(moved, critic, cparams, return_next_values=True))
            for k in want:
                assert _same(got[k], want[k]), (form, keys, k)
    # ppo_gradient: obs; two blocks and a ragged third
    pol, gcritic = G._nets(env, 64, 2, "tanh")
    M = 150
    data, _, _ = G._data(torch, pol, gcritic, M + 64, 11)
    rows = G._rows(torch, "perm", M, data["obs"].shape[0], 11).to(dev)
    gb = G._batch(data, dev)
    par = (pol, data["params"].to(dev), data["log_std"].to(dev), gcritic, data["cparams"].to(dev))
    kw = dict(rows=rows, clip=G.CLIP, vf_coef=G.VF, ent_coef=G.ENT, return_forward=True)
    want = env.ppo_gradient(gb, *par, **kw)
    got = env.ppo_gradient({**gb, "obs": _off_by_one_float(torch, gb["obs"])}, *par, **kw)
    torch.cuda.synchronize()
    for k in ("grad_params", "grad_log_std", "grad_critic_params", "mean", "value"):
        assert torch.equal(UP._bits(got[k]), UP._bits(want[k])), k
    for k in want["stats"]:
        assert torch.equal(UP._bits(got["stats"][k]), UP._bits(want["stats"][k])), k
