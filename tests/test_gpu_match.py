"""VecFusedEnv.lookahead_match / rsx_task_lookahead_match: K actors against M opponents per env of VSS-v0 inside one lookahead launch.

The reference is the committed path: per (k, m) checkpoint(), collect(actor k, opponent m, deterministic heads, the same seats),
restore().  From the same handle state the rows before a pair's end are the same bits (include/rsx.h, "Exactness"); the return is
recomputed in numpy float32 with the header's recurrence.  One seat a side is also compared with the oracle directly
(selfplay_helpers.lockstep_step fed the recorded actions).  Every comparison is on bit patterns.

Common unless a case says otherwise: H = 6, K = 2, M = 2, distinct random parameters per k and m, 1 x 32 relu against 2 x 64 tanh or the
reverse (a wrong image offset cannot cancel), reset() and three warm step(None)."""
import numpy as np
import pytest

import selfplay_helpers as SH
import test_gpu_policy_lookahead as PL
import test_gpu_selfplay as SP
from test_gpu_feature_shapes import _run_time_count
from test_gpu_policy_shapes import RANGES

pytestmark = pytest.mark.gpu

H, K, M, WARM = 6, 2, 2, 3
SEATS = [(False, False), (True, False), (False, True), (True, True)]
KEYS = ("return", "steps", "terminated", "truncated", "result", "last_obs", "actions", "opponent_actions", "policy_obs", "opponent_obs")
_same, _host = PL._same, PL._host


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _policies(torch, env, swap=False, k=K, m=M):
    """(actor policy, params [k, P], opponent policy, params [m, P2]): distinct rows, the two shapes of selfplay_helpers"""
    from rsoccer_amd.vec.policy import MLPPolicy
    sa, so = (SH.SHAPE_LARGE, SH.SHAPE_SMALL) if swap else (SH.SHAPE_SMALL, SH.SHAPE_LARGE)
    pa = MLPPolicy(env.sim.obs_dim, env.sim.act_dim, **sa)
    po = MLPPolicy(env.sim.obs_dim, env.sim.act_dim, **so)
    return pa, PL._dense(torch, pa, k, seed=5), po, PL._dense(torch, po, m, seed=6)


def _match(env, pols, seats, gamma=1.0, horizon=H, host=True):
    pa, a, po, o = pols
    out = env.lookahead_match(pa, a, po, o, horizon, gamma=gamma, team=seats[0], opponent_team=seats[1], return_obs=True, return_actions=True,
                              return_policy_obs=True)
    return _host(out) if host else out


def _with_seats(out, seats):
    """the result with a seat axis on both sides' recordings, whatever the flags"""
    s = dict(out)
    for flag, keys in ((seats[0], ("actions", "policy_obs")), (seats[1], ("opponent_actions", "opponent_obs"))):
        if not flag:
            for key in keys:
                s[key] = out[key][:, :, :, :, None]
    return s


def _committed(torch, env, pols, seats, horizon=H):
    """{(k, m): collect()'s batch on the host, with a seat axis}: the committed path, pair by pair, the env restored behind each"""
    pa, a, po, o = pols
    blob = env.checkpoint()
    ref = {}
    for k in range(a.shape[0]):
        for m in range(o.shape[0]):
            b = _host(env.collect(pa, a[k], horizon, return_final_obs=True, opponent=po, opponent_params=o[m], team=seats[0],
                                  opponent_team=seats[1]))
            if not (seats[0] or seats[1]):   # (collect() gives both sides a seat axis as soon as one flag is set)
                for key in ("obs", "actions", "final_obs", "opponent_obs", "opponent_actions"):
                    b[key] = b[key][:, :, None]
                b["next_obs"] = b["next_obs"][:, None].copy()
            ref[k, m] = b
            env.restore(blob)
    torch.cuda.synchronize()
    return ref


def _returns(reward, n, gamma):
    """the header's recurrence in numpy float32 over rows t < n: ret = ret + disc * r_t; disc = disc * gamma.  reward [T, B], n [B]"""
    g = np.float32(gamma)
    ret, disc = np.zeros(reward.shape[1], dtype=np.float32), np.ones(reward.shape[1], dtype=np.float32)
    for t in range(reward.shape[0]):
        ret = np.where(t < n, (ret + disc * reward[t].astype(np.float32)).astype(np.float32), ret)
        disc = (disc * g).astype(np.float32)
    return ret


def _compare(out, ref, gamma, tag, horizon=H):
    """The Exactness paragraph, for every (k, m): rows t < steps of both sides' obs and actions, the return through the recurrence, the
    flags at the last row (and none before it), last_obs against final_obs (ended) or next_obs (ran out of horizon), result against the
    side of the terminal ball, zeros behind the end.  -> (rows compared, pairs that ended inside the horizon)"""
    s = out
    B = s["steps"].shape[0]
    rows = ended_pairs = 0
    for (k, m), b in ref.items():
        n = s["steps"][:, k, m].astype(np.int64)
        at = (tag, "actor", k, "opponent", m)
        assert n.min() >= 1 and n.max() <= horizon, at
        sim = np.arange(horizon)[None, :] < n[:, None]                       # [B, H]
        for got, want in (("policy_obs", "obs"), ("actions", "actions"), ("opponent_obs", "opponent_obs"),
                          ("opponent_actions", "opponent_actions")):
            g, w = s[got][:, k, m], np.swapaxes(b[want], 0, 1)               # [B, H, S, n]
            assert g.shape == w.shape, at + (got, g.shape, w.shape)
            bad = (_bits(g) != _bits(w)).any(axis=(-1, -2)) & sim
            assert not bad.any(), at + (got, "first (env, row)", np.argwhere(bad)[:4].tolist())
            assert not g[~sim].any(), at + (got, "written behind the pair's end")
        flags = (b["terminated"] | b["truncated"]).T                          # [B, H]
        last = n - 1
        env = np.arange(B)
        assert not (flags & (np.arange(horizon)[None, :] < last[:, None])).any(), at + ("the committed path ended earlier",)
        assert np.array_equal(s["terminated"][:, k, m], b["terminated"][last, env]), at + ("terminated",)
        assert np.array_equal(s["truncated"][:, k, m], b["truncated"][last, env]), at + ("truncated",)
        ended = flags[env, last]
        assert np.all(ended | (n == horizon)), at + ("a pair stopped without an end",)
        want_ret = _returns(b["reward"], n, gamma)
        assert _same(s["return"][:, k, m], want_ret), at + ("return", s["return"][:, k, m], want_ret)
        want_last = np.where(ended[:, None], b["final_obs"][last, env, 0], b["next_obs"][:, 0])
        assert _same(s["last_obs"][:, k, m], want_last), at + ("last_obs",)
        ball_x = b["final_obs"][last, env, 0, 0]
        want_res = np.where(b["terminated"][last, env], np.sign(ball_x), 0).astype(np.int8)
        assert s["result"].dtype == np.int8 and np.array_equal(s["result"][:, k, m], want_res), at + ("result", s["result"][:, k, m], want_res)
        rows += int(sim.sum())
        ended_pairs += int(ended.sum())
    return rows, ended_pairs


def _exact_case(torch, env, tag, swap=False, seats=SEATS, prepare=None):
    """every seat combination of `seats` on a prepared handle: gamma 1.0 with everything compared, gamma 0.97 for the return"""
    (prepare or (lambda e: SP._start(torch, e, WARM)))(env)
    pols = _policies(torch, env, swap)
    rows = ends = 0
    for st in seats:
        ref = _committed(torch, env, pols, st)
        out = _with_seats(_match(env, pols, st, gamma=1.0), st)
        r, e = _compare(out, ref, 1.0, f"{tag} seats {st}")
        rows, ends = rows + r, ends + e
        disc = _with_seats(_match(env, pols, st, gamma=0.97), st)
        for key in KEYS:
            if key != "return":
                assert _same(disc[key], out[key]), (tag, st, "gamma moved", key)
        _compare(disc, ref, 0.97, f"{tag} seats {st} gamma 0.97")
        # the pairs differ: distinct parameters per k and m give distinct trajectories
        assert not _same(out["actions"][:, 0, 0], out["actions"][:, 1, 0]) and not _same(out["opponent_actions"][:, 0, 0], out["opponent_actions"][:, 0, 1]), tag
        assert not _same(out["policy_obs"][:, 0, 0, 2], out["policy_obs"][:, 0, 1, 2]), (tag, "the opponent does not move the agent's row")
    print(f"{tag}: {rows} rows equal the committed path bit for bit, {ends} pairs ended inside the horizon")
    return rows, ends


# ---- 1. bit-exact against the committed path ----
@pytest.mark.parametrize("B", SH.B_SIZES)
def test_3v3_at_8_lanes_equals_collect(B):
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(B, device=0, seed=2025)
    assert env.sim.task_layout() == "8-lanes-per-env"
    _exact_case(torch, env, f"3v3 B={B}", swap=B == 13)
    env.close()


@pytest.mark.parametrize("B", SH.B_SIZES)
def test_5v5_at_16_lanes_equals_collect(B):
    import torch
    from rsoccer_amd import vec
    env = PL._make(vec, "VecVSS5v5", B, device=0, seed=2025)
    assert env.sim.obs_dim == 64 and env.sim.task_layout() == "16-lanes-per-env"
    _exact_case(torch, env, f"5v5 B={B}", swap=B == 5)
    env.close()


@pytest.mark.parametrize("B", SH.B_SIZES)
def test_32_lanes_per_env_equal_collect_and_8_lanes(monkeypatch, B):
    import torch
    from rsoccer_amd import vec
    kw = dict(device=0, seed=29, max_episode_steps=7)   # TimeLimit 7, three warm steps: every pair is truncated after 4 steps
    base = vec.VecVSSEnv(B, **kw)
    SP._start(torch, base, WARM)
    want = _match(base, _policies(torch, base), (True, True))
    base.close()
    monkeypatch.setenv("RSX_LANES_PER_ENV", "32")
    env = vec.VecVSSEnv(B, **kw)
    assert env.sim.task_layout() == "32-lanes-per-env", env.sim.task_layout()
    _, ends = _exact_case(torch, env, f"32 lanes B={B}")
    assert ends == len(SEATS) * B * K * M   # (every pair of every seat combination)
    got = _match(env, _policies(torch, env), (True, True))
    for key in KEYS:
        assert _same(got[key], want[key]), ("32 lanes against 8", key)
    assert np.all(got["steps"] == 4) and got["truncated"].all()
    env.close()


@pytest.mark.parametrize("cfg", SH.SHAPE_CONFIGS, ids=[f"{c[0]}v{c[0]}-B{c[1]}-seed{c[2]}-base{c[3]}" for c in SH.SHAPE_CONFIGS])
def test_every_handle_configuration_equals_collect(cfg):
    """selfplay_helpers.SHAPE_CONFIGS: more than one tile per XCD, the run-time robot count (2v2), env_id_base 5000, 5v5; TimeLimit 7:
    pairs are truncated after 4 steps unless a goal ends them earlier"""
    import torch
    from rsoccer_amd import vec
    nb, B, seed, base = cfg
    kw = dict(device=0, seed=seed, env_id_base=base, max_episode_steps=7)
    env = (vec.VecVSSEnv(B, **kw) if nb == 3 else _run_time_count(vec, "vss-2v2", B, **kw) if nb == 2 else PL._make(vec, "VecVSS5v5", B, **kw))
    assert env.sim.obs_dim == 4 + 12 * nb
    _, ends = _exact_case(torch, env, f"config {cfg}", swap=nb == 2)
    assert ends == len(SEATS) * B * K * M
    env.close()


@pytest.mark.parametrize("B", SH.B_SIZES)
def test_per_env_physics_equals_collect(B):
    import torch
    import rsoccer_amd
    env = rsoccer_amd.make_vec("VSS-v0", B, device=0, seed=31, max_episode_steps=20, physics_ranges=RANGES)

    def prepare(e):   # two auto-resets per env (the coefficients were redrawn and differ per env), then 17 steps into the third episode
        e.reset()
        e.step_random(57)
        torch.cuda.synchronize()

    _, ends = _exact_case(torch, env, f"per-env physics B={B}", swap=B == 5, prepare=prepare)
    assert len(np.unique(env.physics()["m_ball"].cpu().numpy())) > 1
    assert ends > 0   # (three steps to the time limit)
    env.close()


@pytest.mark.parametrize("B", SH.B_SIZES)
def test_device_keyed_handles_equal_collect_and_replay_from_a_graph(B):
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(B, device=0, seed=17, max_episode_steps=12)
    SP._start(torch, env, WARM)
    env.enable_graph_capture()
    _exact_case(torch, env, f"device-keyed B={B}", swap=B == 13, prepare=lambda e: None)
    pa, a, po, o = _policies(torch, env, B == 13)
    pols = (pa, a.to(env.device), po, o.to(env.device))
    st = (True, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # torch's warm-up before a capture
        _match(env, pols, st, host=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    tick = env.sim.task_tick()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _match(env, pols, st, host=False)
    assert env.sim.task_tick() == tick
    seen = []
    for i in range(2):   # each replay starts from where the env stands then: it reads the step counter on the device
        env.step(None)
        g.replay()
        torch.cuda.synchronize()
        got = {key: v.clone() for key, v in out.items()}
        want = _match(env, pols, st, host=False)
        torch.cuda.synchronize()
        for key in want:
            assert torch.equal(got[key], want[key]), (f"replay {i}", key)
        seen.append(got["policy_obs"])
    assert not torch.equal(seen[0], seen[1])   # (the replays were not one and the same result)
    ref = _committed(torch, env, pols, st)     # ... and the second replay is the committed path from that state
    _compare(_with_seats({k: v.cpu().numpy() for k, v in got.items()}, st), ref, 1.0, f"replayed B={B}")
    assert env.sim.task_tick() == tick + 2
    env.close()


# ---- 2. the handle is untouched ----
@pytest.mark.parametrize("device_keyed", [False, True])
def test_the_handle_is_left_exactly_as_it_was(device_keyed):
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(13, device=0, seed=12, max_episode_steps=8)
    SP._start(torch, env, WARM)
    if device_keyed:
        env.enable_graph_capture()
        env.step(None)
    torch.cuda.synchronize()
    before, metrics, tick = env.checkpoint(), env.metrics(), env.sim.task_tick()
    views = {k: env._t[k].clone() for k in ("obs", "reward", "terminated", "truncated", "final_obs", "info", "steps")}
    pols = _policies(torch, env)
    for st in SEATS:
        out = _match(env, pols, st, horizon=8)
        assert out["truncated"].all() and out["steps"].max() < 8   # pairs ran into the time limit: nothing of that reached the handle
    assert np.array_equal(env.checkpoint(), before) and env.metrics() == metrics and env.sim.task_tick() == tick
    for k, v in views.items():
        assert torch.equal(env._t[k], v), k
    env.close()


# ---- 3. against the oracle directly ----
# Seeds 2025 (3v3, 13 envs) and 23 (2v2, 37 envs): under the oracle's own random actions no env ends an episode within WARM + H = 9 steps
# of its reset (selfplay_helpers.oracle_alone_ends, run on the CPU: 0 of 13 and 0 of 37), so the 90 % of rows the test demands are the
# policies' trajectories' to keep.
@pytest.mark.parametrize("cfg", [(3, 13, 2025, 0), (2, 37, 23, 0)], ids=["3v3-B13", "2v2-B37"])
def test_one_seat_a_side_against_the_lockstep_oracle(oracle_mod, cfg):
    import torch
    from rsoccer_amd import vec
    assert cfg in SH.SHAPE_CONFIGS
    nb, B, seed, base = cfg
    assert SH.oracle_alone_ends(oracle_mod, B, seed, steps=H, warm=WARM, nb=nb) == 0
    env = vec.VecVSSEnv(B, device=0, seed=seed) if nb == 3 else _run_time_count(vec, "vss-2v2", B, device=0, seed=seed)
    SP._start(torch, env, WARM)
    out = _match(env, _policies(torch, env, swap=nb == 2), (False, False))
    obs0 = env._t["obs"].cpu().numpy()
    compared = 0
    for k in range(K):
        for m in range(M):
            refs = SH.oracle_envs(oracle_mod, B, seed, base=base, warm=WARM, nb=nb)
            for e, r in enumerate(refs):
                at = (cfg, k, m, e)
                assert _same(obs0[e], r.task_out()["obs"].astype(np.float32)), at + ("the two sides do not start from the same instant",)
                assert _same(out["policy_obs"][e, k, m, 0], obs0[e]), at
                n = int(out["steps"][e, k, m])
                ret, disc = np.float32(0.0), np.float32(1.0)
                for t in range(n):
                    obs, reward, ended = SH.lockstep_step(r, out["actions"][e, k, m, t], out["opponent_actions"][e, k, m, t])
                    if ended:   # the row of an episode end is not comparable (the oracle re-places the env): rows up to the pair's end
                        break
                    got = out["policy_obs"][e, k, m, t + 1] if t + 1 < n else out["last_obs"][e, k, m]
                    assert _same(got, obs), at + (t, np.argwhere(got != obs)[:4].tolist())
                    ret = np.float32(ret + disc * reward)
                    compared += 1
                else:
                    assert n == H and not out["terminated"][e, k, m] and not out["truncated"][e, k, m], at
                    assert _same(out["return"][e, k, m], ret), at + ("return", out["return"][e, k, m], ret)
    total = B * K * M * H
    print(f"{cfg}: {compared} of {total} (env, k, m, t) rows equal the lockstep oracle bit for bit")
    assert compared * 10 >= total * 9, (compared, total)
    env.close()


# ---- 4. ends ----
@pytest.mark.parametrize("seats", [(False, False), (True, True)], ids=["seats-1-1", "seats-n-n"])
def test_pairs_stop_at_a_goal(seats):
    """selfplay_helpers.goal_lineup: goals at rows 1, 2 and 4 by the env's gap, on the side of its sign s"""
    import torch
    from rsoccer_amd import vec
    B = 13
    env = vec.VecVSSEnv(B, device=0, seed=2025)
    ball, blue, yellow, s, gap = SH.goal_lineup(B, 3, env.field["length"] / 2)

    def prepare(e):
        e.reset()
        e.reset_to(ball, blue, yellow)
        torch.cuda.synchronize()

    prepare(env)
    pols = _policies(torch, env)
    out = _with_seats(_match(env, pols, seats), seats)
    ref = _committed(torch, env, pols, seats)
    _compare(out, ref, 1.0, f"goals {seats}")
    row = np.array([1, 2, 4])[np.arange(B) % 3]
    want = np.broadcast_to((row + 1)[:, None, None], (B, K, M))
    assert np.array_equal(out["steps"], want), out["steps"][:, 0, 0]
    assert out["terminated"].all() and not out["truncated"].any()
    assert np.array_equal(out["result"], np.broadcast_to(s.astype(np.int8)[:, None, None], (B, K, M))), out["result"][:, 0, 0]
    assert (out["result"] == 1).any() and (out["result"] == -1).any()
    for k in range(K):
        for m in range(M):
            fin = ref[k, m]["final_obs"][row, np.arange(B), 0]
            assert _same(out["last_obs"][:, k, m], fin), (k, m)
            assert np.all(np.sign(out["last_obs"][:, k, m, 0]) == s)   # the terminal ball lies on the goal's side
            assert np.all(out["return"][:, k, m][s > 0] > 5.0) and np.all(out["return"][:, k, m][s < 0] < -5.0)
    behind = np.arange(H)[None, None, None, :] >= out["steps"][..., None]
    for key in ("actions", "policy_obs", "opponent_actions", "opponent_obs"):
        assert not out[key][behind].any() and out[key][~behind].any(), key   # nothing is recorded behind the end
    env.close()


@pytest.mark.parametrize("seats", [(False, False), (True, True)], ids=["seats-1-1", "seats-n-n"])
def test_pairs_stop_at_the_time_limit(seats):
    import torch
    from rsoccer_amd import vec
    B = 13
    env = vec.VecVSSEnv(B, device=0, seed=4, max_episode_steps=4)
    SP._start(torch, env, 0)
    pols = _policies(torch, env)
    out = _with_seats(_match(env, pols, seats), seats)
    assert np.all(out["steps"] == 4) and out["truncated"].all() and not out["terminated"].any()
    assert np.all(out["result"] == 0)
    _compare(out, _committed(torch, env, pols, seats), 1.0, f"time limit {seats}")
    env.close()


# ---- 5. the layout of the pair axis ----
def test_the_pair_axis_follows_the_parameter_rows():
    import torch
    from rsoccer_amd import vec
    env = vec.VecVSSEnv(13, device=0, seed=2025, max_episode_steps=8)
    SP._start(torch, env, WARM)
    pa, a, po, o = _policies(torch, env)
    st = (True, True)
    full = _match(env, (pa, a, po, o), st, gamma=0.97)
    assert full["return"].shape == (13, K, M) and full["actions"].shape == (13, K, M, H, 3, 2) and full["opponent_obs"].shape == (13, K, M, H, 3, 40)
    perm = _match(env, (pa, a[[1, 0]], po, o[[1, 0]]), st, gamma=0.97)
    half = _match(env, (pa, a[[1, 0]], po, o), st, gamma=0.97)
    for key in KEYS:
        assert _same(perm[key], full[key][:, ::-1, ::-1]), ("both axes permuted", key)
        assert _same(half[key], full[key][:, ::-1]), ("the actors permuted", key)
        assert not _same(full[key][:, 0, 1], full[key][:, 1, 0]) or key in ("steps", "terminated", "truncated", "result"), key
    for k in range(K):
        for m in range(M):
            one = _match(env, (pa, a[k:k + 1], po, o[m:m + 1]), st, gamma=0.97)
            for key in KEYS:
                assert _same(one[key][:, 0, 0], full[key][:, k, m]), (k, m, key)
    # the seat axis is there only where that side's flag is set
    mixed = _match(env, (pa, a, po, o), (False, True))
    assert mixed["actions"].shape == (13, K, M, H, 2) and mixed["opponent_actions"].shape == (13, K, M, H, 3, 2)
    assert mixed["policy_obs"].shape == (13, K, M, H, 40) and mixed["opponent_obs"].shape == (13, K, M, H, 3, 40)
    bare = env.lookahead_match(pa, a, po, o, H)
    assert set(bare) == {"return", "steps", "terminated", "truncated", "result"}
    for key, v in _host(bare).items():
        assert _same(v, _match(env, (pa, a, po, o), (False, False))[key]), key
    env.close()


# ---- 6. refusals through the C call ----
def test_the_c_boundary_refuses_and_writes_nothing():
    import torch
    from rsoccer_amd import _lib, vec
    from rsoccer_amd.vec.policy import MLPPolicy
    dev = torch.device("cuda", 0)
    FILL = 0x5A5A5A5A
    new = SH.filled(torch, dev, FILL)
    B = 5

    def outputs(od, S=3, S2=3, k=K, m=M):
        t = {"returns": new((B, k, m)), "steps": new((B, k, m)), "flags": torch.full((B, k, m), FILL & 0xFF, dtype=torch.uint8, device=dev),
             "result": torch.full((B, k, m), FILL & 0x7F, dtype=torch.int8, device=dev), "last_obs": new((B, k, m, od)),
             "actions": new((B, k, m, H, S, 2)), "obs": new((B, k, m, H, S, od)), "opp_actions": new((B, k, m, H, S2, 2)),
             "opp_obs": new((B, k, m, H, S2, od))}
        return t, _lib.MatchOut(*(t[f].data_ptr() for f, _ in _lib.MatchOut._fields_))

    def untouched(t):
        torch.cuda.synchronize()
        for key, v in t.items():
            w = v.view(torch.int32) if v.dtype == torch.float32 else v
            want = FILL if v.dtype == torch.float32 else (FILL & 0xFF if v.dtype == torch.uint8 else FILL & 0x7F)
            assert bool((w == want).all()), key

    # another task
    sd = vec.VecSSLStaticDefendersEnv(B, device=0, seed=1)
    sd.reset()
    p5 = MLPPolicy(sd.sim.obs_dim, sd.sim.act_dim)
    w5 = torch.zeros(1, p5.num_params, device=dev)
    t, rec = outputs(sd.sim.obs_dim, 1, 1, 1, 1)
    with pytest.raises(_lib.RsxError, match="VSS-v0 only"):
        sd.sim.task_lookahead_match(p5.spec(), w5.data_ptr(), 1, 1, p5.spec(), w5.data_ptr(), 1, 1, H, 1.0, rec, sd._stream())
    untouched(t)
    sd.close()
    # unequal teams
    lop = _lib.Sim(_lib.KIND_VSS, 0, 3, 2, 25, B, 0)
    lop.task_attach(_lib.TASK_VSS_V0, 1, 0, 0)
    lop.task_reset()
    pl = MLPPolicy(lop.obs_dim, lop.act_dim)
    wl = torch.zeros(1, pl.num_params, device=dev)
    t, rec = outputs(lop.obs_dim, 1, 1, 1, 1)
    with pytest.raises(_lib.RsxError, match="equal teams"):
        lop.task_lookahead_match(pl.spec(), wl.data_ptr(), 1, 1, pl.spec(), wl.data_ptr(), 1, 1, H, 1.0, rec, None)
    untouched(t)
    lop.close()

    env = vec.VecVSSEnv(B, device=0, seed=1)
    pol, opp = MLPPolicy(40, 2, **SH.SHAPE_SMALL), MLPPolicy(40, 2, **SH.SHAPE_LARGE)
    w, w2 = torch.zeros(K, pol.num_params, device=dev), torch.zeros(M, opp.num_params, device=dev)
    sp, sp2, wp, wp2 = pol.spec(), opp.spec(), w.data_ptr(), w2.data_ptr()
    t, rec = outputs(40)
    with pytest.raises(_lib.RsxError, match="reset"):
        env.sim.task_lookahead_match(sp, wp, K, 3, sp2, wp2, M, 3, H, 1.0, rec, env._stream())
    env.reset()
    torch.cuda.synchronize()
    before, tick = env.checkpoint(), env.sim.task_tick()
    bad = _lib.PolicyMLP(2, 48, _lib.ACT_TANH, _lib.ACT_TANH)
    lacking = {f: _lib.MatchOut(*(None if g == f else t[g].data_ptr() for g, _ in _lib.MatchOut._fields_)) for f in ("returns", "steps", "flags")}
    cases = [((sp, wp, K, 0, sp2, wp2, M, 3, H, 1.0, rec), "actor_seats"), ((sp, wp, K, 2, sp2, wp2, M, 3, H, 1.0, rec), "actor_seats"),
             ((sp, wp, K, 4, sp2, wp2, M, 3, H, 1.0, rec), "actor_seats"), ((sp, wp, K, 3, sp2, wp2, M, 0, H, 1.0, rec), "opponent_seats"),
             ((sp, wp, K, 3, sp2, wp2, M, 2, H, 1.0, rec), "opponent_seats"), ((sp, wp, K, 3, sp2, wp2, M, -1, H, 1.0, rec), "opponent_seats"),
             ((sp, wp, 0, 3, sp2, wp2, M, 3, H, 1.0, rec), "n_actors"), ((sp, wp, K, 3, sp2, wp2, 0, 3, H, 1.0, rec), "n_opponents"),
             ((sp, wp, -1, 3, sp2, wp2, M, 3, H, 1.0, rec), "n_actors"), ((sp, wp, K, 3, sp2, wp2, M, 3, 0, 1.0, rec), "horizon"),
             ((sp, wp, K, 3, sp2, wp2, M, 3, H, float("nan"), rec), "gamma"), ((sp, wp, K, 3, sp2, wp2, M, 3, H, float("inf"), rec), "gamma"),
             ((None, wp, K, 3, sp2, wp2, M, 3, H, 1.0, rec), "must not be null"), ((sp, wp, K, 3, None, wp2, M, 3, H, 1.0, rec), "opponent"),
             ((sp, None, K, 3, sp2, wp2, M, 3, H, 1.0, rec), "actor_params_dev"), ((sp, wp, K, 3, sp2, None, M, 3, H, 1.0, rec), "opponent_params_dev"),
             ((bad, wp, K, 3, sp2, wp2, M, 3, H, 1.0, rec), "hidden"), ((sp, wp, K, 3, bad, wp2, M, 3, H, 1.0, rec), "hidden"),
             ((sp, wp, K, 3, sp2, wp2, M, 3, H, 1.0, None), "out"),
             # lane_grid x K x M workgroups over the launch limit: refused before any array is looked at
             ((sp, wp, 1 << 15, 3, sp2, wp2, 1 << 15, 3, H, 1.0, rec), "launch limit"), ((sp, wp, 1 << 20, 3, sp2, wp2, 1 << 20, 3, H, 1.0, rec), "launch limit")]
    cases += [((sp, wp, K, 3, sp2, wp2, M, 3, H, 1.0, r), f) for f, r in lacking.items()]
    for args, why in cases:
        with pytest.raises(_lib.RsxError, match=why):
            env.sim.task_lookahead_match(*args, env._stream())
    untouched(t)
    assert np.array_equal(env.checkpoint(), before) and env.sim.task_tick() == tick   # nothing was enqueued
    # a captured call on a host-keyed handle is refused like the policy lookahead's
    side = torch.cuda.Stream()
    with pytest.raises(_lib.RsxError, match="rsx_task_enable_capture"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
            env.lookahead_match(pol, w, opp, w2, H)
    torch.cuda.synchronize()
    _lib.drop_pending_hip_error()   # what the aborted capture leaves behind
    untouched(t)
    # the optional members may be NULL, and the valid call writes every word of the required ones
    only = _lib.MatchOut(t["returns"].data_ptr(), t["steps"].data_ptr(), t["flags"].data_ptr())
    env.sim.task_lookahead_match(sp, wp, K, 3, sp2, wp2, M, 3, H, 1.0, only, env._stream())
    torch.cuda.synchronize()
    assert int(t["steps"].view(torch.int32).min()) == H and int(t["steps"].view(torch.int32).max()) == H and not bool(t["flags"].any())
    untouched({k: v for k, v in t.items() if k not in ("returns", "steps", "flags")})
    assert np.array_equal(env.checkpoint(), before) and env.sim.task_tick() == tick
    env.close()
