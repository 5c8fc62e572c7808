"""The two launches that restate the collector's loop in translation units of their own — collect(opponent=) / rsx_task_collect_selfplay
and collect(team=, opponent_team=) / rsx_task_collect_team — THROUGH episode ends and on the handle shapes their tests had not given
them: more than one tile per XCD, padded rows, the run-time robot count (VSS-v0 2v2), env_id_base != 0, one lane per env, per-env
physics redrawn inside the launch, 5v5 at 16 lanes per env; goals next to truncations; the C calls on pattern-filled outputs; split calls.

The reference is the lockstep oracle that goes through ends (selfplay_helpers.episode_step, proven on the CPU in
tests/test_selfplay_reference.py), fed the recorded actions of every seat.  Common to every case unless it says otherwise: TimeLimit 5,
three warm step(None), T = 12 (every env ends at rows 1, 6 and 11 inside the launch), Gaussian heads on both sides, 1 x 32 relu against
2 x 64 tanh (self-play) and the reverse (team play).  Every comparison is on bit patterns."""
import numpy as np
import pytest

import selfplay_helpers as SH
import teamplay_helpers as TH
import test_gpu_policy_lookahead as PL
import test_gpu_selfplay as SP
from mass_end_helpers import SENTINEL, final_obs_faults
from physics_helpers import DEFAULTS, NAMES, derive, set_oracle_coefs
from test_gpu_feature_shapes import B_PAD, _run_time_count, _twins
from test_gpu_physics_params import _expected_draw
from test_gpu_policy_shapes import RANGES

pytestmark = pytest.mark.gpu

T, WARM, LIMIT, TAIL = 12, 3, 5, 4
LOG_STD, OPP_LOG_STD, NOISE_SEED = -1.0, -0.5, 17
_same, _host = PL._same, SP._host
SELF = "selfplay"   # a case's kind: collect(opponent=), or the seat counts (actor seats, opponent seats) of collect(team=, opponent_team=)


def _kinds(n, more=True):
    """self-play and team play with every robot seated; `more`: also seats (n, 1) and (1, n).  n = "n": the case sets the count"""
    kinds = [SELF, (n, n)] + ([(n, 1), (1, n)] if more else [])
    return pytest.mark.parametrize("kind", kinds, ids=[k if k == SELF else f"seats-{k[0]}-{k[1]}" for k in kinds])


def _shapes(kind):
    return (SH.SHAPE_SMALL, SH.SHAPE_LARGE) if kind == SELF else (SH.SHAPE_LARGE, SH.SHAPE_SMALL)


def _call(torch, env, kind, n, steps=T, noise_seed=NOISE_SEED):
    pa, a, po, o = SP._policies(torch, env, *_shapes(kind))
    kw = dict(opponent=po, opponent_params=o, opponent_log_std=OPP_LOG_STD)
    if kind != SELF:
        kw.update(team=kind[0] == n, opponent_team=kind[1] == n)
    return _host(env.collect(pa, a, steps, log_std=LOG_STD, noise_seed=noise_seed, return_final_obs=True, **kw))


def _plain(torch, env, kind):
    """the twin without seats: plain collect() under the same agent, head and noise"""
    pa, a, _, _ = SP._policies(torch, env, *_shapes(kind))
    return _host(env.collect(pa, a, T, log_std=LOG_STD, noise_seed=NOISE_SEED, return_final_obs=True))


def _seated(out, kind):
    """the batch with a seat axis whatever the kind: [T, B, S, ...] and next_obs [B, S, obs_dim]"""
    if kind != SELF:
        return out
    s = dict(out)
    for k in ("obs", "actions", "final_obs", "opponent_obs", "opponent_actions"):
        s[k] = out[k][:, :, None]
    s["next_obs"] = out["next_obs"][:, None]
    return s


def _warm(torch):
    return lambda env: SP._start(torch, env, WARM)


def _same_instant(torch, env, refs):
    torch.cuda.synchronize()
    obs0 = env._t["obs"].cpu().numpy()
    for e, r in enumerate(refs):
        assert _same(obs0[e], r.task_out()["obs"].astype(np.float32)), ("the two sides do not start from the same instant", e)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _through_ends(out, refs, kind, tag, on_end=None):
    """The through-ends check of one call: every (t, env) that is not dropped against the reference fed the recorded actions — row t + 1
    of every seat of both sides, reward, both flags, final_obs at ended rows (and zeros elsewhere).  The reference's rows are gathered
    env by env and row by row, then compared with the records in whole arrays; -> the dropped envs"""
    s = _seated(out, kind)
    steps, B, SA = s["actions"].shape[:3]
    SO, OD = s["opponent_actions"].shape[2], s["obs"].shape[-1]
    rows = np.concatenate([s["obs"], s["next_obs"][None]], 0)
    orows = s["opponent_obs"]
    if "opponent_next_obs" in s:
        orows = np.concatenate([orows, s["opponent_next_obs"][None]], 0)
    want = {k: np.zeros((steps + 1, B, OD), dtype=np.float32) for k in ("row", "orow", "fin", "ofin")}
    reward = np.zeros((steps, B), dtype=np.float32)
    term, trunc, live = (np.zeros((steps + 1, B), dtype=bool) for _ in range(3))
    for e, r in enumerate(refs):   # row 0: the instant both sides start from, and its mirror
        want["row"][0, e] = r.obs_eval()
        want["orow"][0, e] = SH.mirror(want["row"][0, e], SH.yellow_sincos(r), r.n_blue)[0]
    dropped, ends = set(), 0
    for t in range(steps):
        for e, r in enumerate(refs):
            if e in dropped:
                continue
            row, reward[t, e], term[t, e], trunc[t, e], fin, drop, (orow, ofin) = TH.lockstep_episode_step(
                r, s["actions"][t, e], s["opponent_actions"][t, e], True)
            if drop:   # the oracle's own trajectory ended where the replaced one did not: the one reason left
                dropped.add(e)
                continue
            live[t, e] = True
            want["row"][t + 1, e], want["orow"][t + 1, e] = row, orow
            if fin is not None:
                want["fin"][t, e], want["ofin"][t, e] = fin, ofin
                ends += 1
                if on_end:
                    on_end(e)
    live_next = np.concatenate([np.ones((1, B), dtype=bool), live[:steps]], 0)   # row t + 1 is judged where step t was

    def same(name, got, ref, mask):
        """got [n, B, S, ...] against the seat maps of ref [n', B, ...] in the rows of mask [n', B] (n <= n': self-play records no
        opponent row behind the last step)"""
        n = got.shape[0]
        for i in range(got.shape[2]):
            bad = (_bits(got[:, :, i]) != _bits(TH.seat_map(ref[:n], i))).any(-1) & mask[:n]
            where = np.argwhere(bad)
            assert not bad.any(), (tag, name, f"seat {i}", f"{len(where)} rows, first (row, env) {where[:4].tolist()}",
                                   "entries", np.flatnonzero(_bits(got[:, :, i])[tuple(where[0])] != _bits(TH.seat_map(ref[:n], i))[tuple(where[0])])[:6].tolist())

    same("obs (row t + 1; behind the last row next_obs)", rows, want["row"], live_next)
    for name, got, ref in (("terminated", s["terminated"], term[:steps]), ("truncated", s["truncated"], trunc[:steps]),
                           ("reward", _bits(s["reward"]), _bits(reward))):
        bad = (got != ref) & live[:steps]
        assert not bad.any(), (tag, name, "first (row, env)", np.argwhere(bad)[:4].tolist())
    same("final_obs (zeros at rows that did not end)", s["final_obs"], want["fin"], live)
    same("opponent_obs", orows, want["orow"], live_next)
    if "opponent_final_obs" in s:
        same("opponent_final_obs", s["opponent_final_obs"], want["ofin"], live)
    compared = int(live.sum())
    print(f"{tag}: {compared} rows of {steps * B} equal the reference through {ends} episode ends; dropped {len(dropped)} of {B} envs {sorted(dropped)}")
    assert len(dropped) * 8 <= B, (tag, "dropped", sorted(dropped))
    return dropped


def _check_metrics(before, after, out, tag):
    term, trunc = out["terminated"], out["truncated"]
    d = {k: after[k] - before[k] for k in ("episodes", "truncated_episodes", "env_steps")}
    assert d["episodes"] == int((term | trunc).sum()), (tag, d)
    assert d["truncated_episodes"] == int((trunc & ~term).sum()), (tag, d)
    assert d["env_steps"] == term.size, (tag, d)


def _informative(out, plain, kind, tag):
    """each env ended at least twice inside the launch, and the rows before the first reset differ from the twin's without seats"""
    ends = (out["terminated"] | out["truncated"]).sum(0)
    assert ends.min() >= 2, (tag, "uninformative: an env ended fewer than two episodes inside the launch", ends.tolist())
    assert (out["terminated"] | out["truncated"])[0].sum() == 0, tag   # (no case ends an episode at row 0)
    seat0 = _seated(out, kind)["obs"][:, :, 0]
    assert _same(seat0[0], plain["obs"][0]), (tag, "the twin does not start where the handle starts")
    differ = (seat0[1] != plain["obs"][1]).any(-1)
    assert differ.all(), (tag, "uninformative: envs whose row 1 is the twin's without seats", np.flatnonzero(~differ).tolist())


def _tail(torch, env, refs, dropped, tag, on_end=None):
    """TAIL more step(actions) calls equal the reference continued by task_step"""
    B = env.num_envs
    acts = np.random.default_rng(3).uniform(-1, 1, (TAIL, B, 2)).astype(np.float32)
    for t in range(TAIL):
        env.step(torch.from_numpy(acts[t]).to(env.device))
        torch.cuda.synchronize()
        got = {k: env._t[k].cpu().numpy() for k in ("obs", "reward", "terminated", "truncated", "final_obs")}
        for e, r in enumerate(refs):
            if e in dropped:
                continue
            r.task_step(acts[t, e])
            o = r.task_out()
            at = (tag, "step behind the call", t, e)
            assert _same(got["obs"][e], o["obs"].astype(np.float32)) and _same(got["reward"][e], np.float32(o["reward"])), at
            assert (bool(got["terminated"][e]), bool(got["truncated"][e])) == (bool(o["terminated"]), bool(o["truncated"])), at
            if o["terminated"] or o["truncated"]:
                assert _same(got["final_obs"][e], o["final_obs"].astype(np.float32)), at
                if on_end:
                    on_end(e)


def _through_case(torch, env, twin, refs, kind, tag, prepare=None, on_end=None, between=None):
    """prepare both handles, collect on `env`, the through-ends check, metrics(), the twin without seats, the steps behind the call"""
    prepare = prepare or _warm(torch)
    for h in (env, twin):
        prepare(h)
    _same_instant(torch, env, refs)
    n = refs[0].n_blue
    before = env.metrics()
    out = _call(torch, env, kind, n)
    after = env.metrics()
    if between:
        between(out)
    dropped = _through_ends(out, refs, kind, tag, on_end)
    _check_metrics(before, after, out, tag)
    plain = _plain(torch, twin, kind)
    _informative(out, plain, kind, tag)
    _tail(torch, env, refs, dropped, tag, on_end)
    return dict(out=out, plain=plain, before=before, after=after, dropped=dropped)


def _refs(O, cfg, warm=WARM):
    nb, B, seed, base = cfg
    assert cfg in SH.SHAPE_CONFIGS   # (what the oracle alone does on it is shown in tests/test_selfplay_reference.py)
    return SH.oracle_envs(O, B, seed, base=base, warm=warm, nb=nb, limit=LIMIT)


def _check_seats(out, kind, n, tag):
    """team play: every seat's row is the seat map of seat 0's; both kinds: seat 0 of the opponent's side is the mirror"""
    s = _seated(out, kind)
    if kind != SELF:
        for pre in ("", "opponent_"):
            for k in ("obs", "final_obs", "next_obs"):
                rows = s[pre + k]
                for i in range(rows.shape[-2]):
                    assert _same(rows[..., i, :], TH.seat_map(rows[..., 0, :], i)), (tag, pre + k, i)
    SP._check_mirror({"obs": s["obs"][:, :, 0], "opponent_obs": s["opponent_obs"][:, :, 0]}, n=n, tag=tag)


# ---- a. more than one tile per XCD ----
@_kinds(3)
def test_more_than_one_tile_per_xcd(oracle_mod, kind):
    """B = 131: 17 tiles of 8 envs, the last one ragged, three tiles per XCD where every earlier case has one"""
    import torch
    from rsoccer_amd import vec
    cfg = (3, 131, 2025, 0)
    env, twin = (vec.VecVSSEnv(cfg[1], device=0, seed=cfg[2], max_episode_steps=LIMIT) for _ in range(2))
    res = _through_case(torch, env, twin, _refs(oracle_mod, cfg), kind, f"a {kind}")
    _check_seats(res["out"], kind, 3, f"a {kind}")
    env.close(); twin.close()


# ---- b. padded rows ----
@_kinds(3, more=False)
def test_padded_rows(oracle_mod, monkeypatch, kind):
    """auxe(ROW) with P.row_stride: every output, the checkpoint and the metrics equal the dense twin's, and the padded handle passes the
    through-ends check"""
    import torch
    from rsoccer_amd import vec
    cfg = (3, B_PAD, 9, 0)
    make = lambda: vec.VecVSSEnv(B_PAD, device=0, seed=cfg[2], max_episode_steps=LIMIT)   # noqa: E731
    dense, padded = _twins(monkeypatch, make)
    twin = make()
    _warm(torch)(dense)

    def between(out):
        want = _call(torch, dense, kind, 3)
        assert out.keys() == want.keys()
        for k in want:
            assert _same(out[k], want[k]), ("padded against dense", k)
        assert np.array_equal(padded.checkpoint(), dense.checkpoint()) and padded.metrics() == dense.metrics()

    _through_case(torch, padded, twin, _refs(oracle_mod, cfg), kind, f"b {kind}", between=between)
    for h in (dense, padded, twin):
        h.close()


# ---- c. terminations ----
def _line_up(torch, env, refs):
    """reset(), then reset_to of the directed line-up (selfplay_helpers.goal_lineup), no step in between: the launch's first row has
    steps == 0.  -> (prepare for _through_case, s [B]: the side of each env's goal)"""
    half = refs[0].field_params()[0] / 2
    assert abs(env.field["length"] / 2 - half) < 1e-12
    ball, blue, yellow, s, _ = SH.goal_lineup(env.num_envs, refs[0].n_blue, half)
    for e, r in enumerate(refs):
        r.task_reset_to(ball[e], blue[e], yellow[e])

    def prepare(h):
        h.reset()
        h.reset_to(ball, blue, yellow)
        torch.cuda.synchronize()

    return prepare, s


def _goal_asserts(res, kind, s, tag):
    out = res["out"]
    term, trunc, rew = out["terminated"], out["truncated"], out["reward"]
    fin_x = _seated(out, kind)["final_obs"][:, :, 0, 0]   # the ball's x of the terminal observation, seat 0's row
    scored, conceded = term & (fin_x > 0), term & (fin_x < 0)
    print(f"{tag}: goals scored {int(scored.sum())}, conceded {int(conceded.sum())}, rows with both flags {int((term & trunc).sum())}")
    assert scored.any() and conceded.any() and (term & trunc).any(), tag
    assert (scored | conceded).sum() == term.sum() and np.all(rew[scored] == 10.0) and np.all(rew[conceded] == -10.0), tag
    assert np.all(np.sign(fin_x[0:5][term[0:5]]) == np.broadcast_to(s, term.shape)[0:5][term[0:5]]), (tag, "a goal on the other side")
    assert res["after"]["goals_for"] - res["before"]["goals_for"] == int(scored.sum()), tag
    assert res["after"]["goals_against"] - res["before"]["goals_against"] == int(conceded.sum()), tag
    assert (term.sum(0) >= 1).all(), (tag, "an env without a goal")


@pytest.mark.parametrize("n", [3, 5], ids=["3v3", "5v5"])
@_kinds("n", more=False)
def test_terminations(oracle_mod, kind, n):
    """goals at rows 1, 2 and 4 (the last with both flags set), scored and conceded, and the episodes behind them"""
    import torch
    from rsoccer_amd import vec
    kind = kind if kind == SELF else (n, n)
    cfg = (n, 13, 2025, 0)
    make = (lambda: vec.VecVSSEnv(13, device=0, seed=2025, max_episode_steps=LIMIT)) if n == 3 else (
        lambda: PL._make(vec, "VecVSS5v5", 13, device=0, seed=2025, max_episode_steps=LIMIT))
    env, twin = make(), make()
    refs = _refs(oracle_mod, cfg, warm=0)
    prepare, s = _line_up(torch, env, refs)
    res = _through_case(torch, env, twin, refs, kind, f"c {n}v{n} {kind}", prepare=prepare)
    _goal_asserts(res, kind, s, f"c {n}v{n} {kind}")
    env.close(); twin.close()


# ---- d. the run-time robot count: VSS-v0 2v2 ----
@pytest.mark.parametrize("kind", [SELF, (2, 2), (2, 1), "line-up"], ids=["selfplay", "seats-2-2", "seats-2-1", "line-up-seats-2-2"])
def test_vss_2v2(oracle_mod, kind):
    """NR = 0: NB = P.n_blue, opposes = b == NB, write_obs_mirrored(..., NB, ...) and the seat loop with a run-time n"""
    import torch
    from rsoccer_amd import vec
    cfg = (2, 37, 23, 0)
    env, twin = (_run_time_count(vec, "vss-2v2", 37, device=0, seed=23, max_episode_steps=LIMIT) for _ in range(2))
    assert env.sim.obs_dim == 28
    if kind == "line-up":
        refs = _refs(oracle_mod, cfg, warm=0)
        prepare, s = _line_up(torch, env, refs)
        res = _through_case(torch, env, twin, refs, (2, 2), "d line-up", prepare=prepare)
        _goal_asserts(res, (2, 2), s, "d line-up")
    else:
        res = _through_case(torch, env, twin, _refs(oracle_mod, cfg), kind, f"d {kind}")
        _check_seats(res["out"], kind, 2, f"d {kind}")
    env.close(); twin.close()


# ---- e. env_id_base ----
@_kinds(3, more=False)
def test_env_id_base_5000(oracle_mod, kind):
    """the re-placements, the OU draws and both heads' noise are keyed by the global env id"""
    import torch
    from rsoccer_amd import vec
    cfg = (3, 37, 2025, 5000)
    env, twin = (vec.VecVSSEnv(37, device=0, seed=2025, env_id_base=5000, max_episode_steps=LIMIT) for _ in range(2))
    res = _through_case(torch, env, twin, _refs(oracle_mod, cfg), kind, f"e {kind}")
    at0 = vec.VecVSSEnv(37, device=0, seed=2025, env_id_base=0, max_episode_steps=LIMIT)
    _warm(torch)(at0)
    other = _call(torch, at0, kind, 3)
    assert res["out"]["truncated"][1].all() and other["truncated"][1].all()
    a, b = _seated(res["out"], kind)["obs"][2, :, 0], _seated(other, kind)["obs"][2, :, 0]   # the reset rows behind row 1
    assert (a != b).any(-1).all(), "the base does not matter: envs re-placed as at base 0"
    for h in (env, twin, at0):
        h.close()


# ---- f. one lane per env ----
@_kinds(3, more=False)
def test_one_lane_per_env(oracle_mod, monkeypatch, kind):
    """straight behind steps of the one-lane-per-env kernel: ROW_PREV_POT is stale and the launch derives it (the first row's reward
    sees it); ROW_STEPS, ROW_OU and ROW_EPISODE as that kernel leaves them, and as the launch leaves them for it (the steps behind)"""
    import torch
    from rsoccer_amd import vec
    cfg = (3, 131, 2025, 0)
    monkeypatch.setenv("RSX_LAYOUT", "epl")
    env, twin = (vec.VecVSSEnv(131, device=0, seed=2025, max_episode_steps=LIMIT) for _ in range(2))
    monkeypatch.delenv("RSX_LAYOUT")
    assert env.sim.task_layout() == "one-lane-per-env"
    res = _through_case(torch, env, twin, _refs(oracle_mod, cfg), kind, f"f {kind}")
    assert np.abs(res["out"]["reward"][0]).max() > 0.0
    env.close(); twin.close()


# ---- g. per-env physics with ranges ----
class _Physics:
    """the oracle envs carry each env's coefficients, redrawn at every episode end by the Philox formula (tests/test_gpu_physics_parity.py)"""

    def __init__(self, O, refs, seed, base=0):
        self.O, self.refs, self.seed, self.base = O, refs, seed, base
        self.cur = np.tile(np.array([DEFAULTS[0][k] for k in NAMES], dtype=np.float32), (len(refs), 1))
        self.episode = np.zeros(len(refs), int)
        for e in range(len(refs)):
            self.redraw(e, 0)

    def redraw(self, e, step=1):
        self.episode[e] += step
        for k, (lo, hi) in RANGES.items():
            p = NAMES.index(k)
            self.cur[e, p] = _expected_draw(self.O, self.seed, self.base + e, int(self.episode[e]), p, lo, hi)
        set_oracle_coefs(self.refs[e], derive(0, 25, self.cur[e]))

    def warm(self, steps):
        for e, r in enumerate(self.refs):
            for _ in range(steps):
                r.task_step(None)
                o = r.task_out()
                if o["terminated"] or o["truncated"]:
                    self.redraw(e)

    def raw_of(self, env):
        phys = env.physics()
        return np.stack([phys[k].cpu().numpy() for k in NAMES], 1)


@pytest.mark.parametrize("padded", [False, True], ids=["B37", "padded-B131"])
@_kinds(3, more=False)
def test_per_env_physics_with_ranges(oracle_mod, monkeypatch, kind, padded):
    """load_coefs and phys_redraw inside these launches with values other than the compiled-in ones; seven warm steps under TimeLimit 5,
    so the block has been redrawn once and the launch starts at steps == 2: ends at rows 2 and 7"""
    import torch
    import rsoccer_amd
    B, seed = (B_PAD if padded else 37), 31
    make = lambda: rsoccer_amd.make_vec("VSS-v0", B, device=0, seed=seed, max_episode_steps=LIMIT, physics_ranges=RANGES)   # noqa: E731
    refs = SH.oracle_envs(oracle_mod, B, seed, warm=0, limit=LIMIT)
    phys = _Physics(oracle_mod, refs, seed)
    phys.warm(7)
    assert phys.episode.min() >= 1
    prepare = lambda h: SP._start(torch, h, 7)   # noqa: E731
    if padded:
        dense, env = _twins(monkeypatch, make)
        prepare(dense)
    else:
        dense, env = None, make()
    twin = make()
    start = {}

    def between(out):
        if dense is not None:
            want = _call(torch, dense, kind, 3)
            for k in want:
                assert _same(out[k], want[k]), ("padded against dense", k)
            assert np.array_equal(env.checkpoint(), dense.checkpoint()) and env.metrics() == dense.metrics()
            assert _same(phys.raw_of(env), phys.raw_of(dense))

    def prepare_and_note(h):
        prepare(h)
        if h is env:
            start["raw"] = phys.raw_of(env)
            assert _same(start["raw"], phys.cur), "the handle's parameters at the start are not the reference's draws"

    # (the oracle alone, carrying these coefficients, is not among SHAPE_CONFIGS: the cap on dropped envs is checked as everywhere)
    _through_case(torch, env, twin, refs, kind, f"g {kind} padded {padded}", prepare=prepare_and_note, on_end=phys.redraw, between=between)
    last = phys.raw_of(env)
    assert _same(last, phys.cur), "physics() behind the call and the steps behind it is not the reference's last draw"
    p = NAMES.index("m_ball")
    assert (last[:, p] != start["raw"][:, p]).all() and len(np.unique(last[:, p])) > B // 2
    for h in (dense, env, twin):
        if h is not None:
            h.close()


# ---- h. 5v5 at 16 lanes per env ----
@pytest.mark.parametrize("kind", [SELF, (5, 5)], ids=["selfplay", "seats-5-5"])
def test_5v5_through_ends(oracle_mod, kind):
    import torch
    from rsoccer_amd import vec
    cfg = (5, 13, 2025, 0)
    env, twin = (PL._make(vec, "VecVSS5v5", 13, device=0, seed=2025, max_episode_steps=LIMIT) for _ in range(2))
    assert env.sim.obs_dim == 64 and env.sim.task_layout() == "16-lanes-per-env"
    res = _through_case(torch, env, twin, _refs(oracle_mod, cfg), kind, f"h {kind}")
    _check_seats(res["out"], kind, 5, f"h {kind}")
    env.close(); twin.close()


# ---- i. the C calls on pattern-filled outputs ----
def _raw(torch, env, kind, n):
    from rsoccer_amd import _lib
    pa, a, po, o = SP._policies(torch, env, *_shapes(kind))
    sig, osig = (torch.full((2,), v).exp() for v in (LOG_STD, OPP_LOG_STD))
    if kind == SELF:
        return SH.raw_selfplay(torch, _lib, env, pa, a, sig, po, o, osig, NOISE_SEED, T, SENTINEL)
    return TH.raw_team(torch, _lib, env, pa, a, sig, kind[0], po, o, osig, kind[1], NOISE_SEED, T, fill=SENTINEL)


def _pattern_rules(torch, raw, tag):
    """include/rsx.h: every word of every per-row record is written, flags stay within 0 - 3, final_obs / opponent_final_obs are written
    in the rows that ended and only there, on every seat"""
    bits = lambda t: t.contiguous().view(torch.int32)   # noqa: E731
    fl = raw["flags"]
    assert int(fl.max()) <= 3, (tag, "flags", (fl > 3).nonzero()[:4].tolist())
    ended = (fl & 3) != 0
    assert int(ended.sum(0).min()) >= 2 and bool((~ended).any(0).all()), (tag, "uninformative")
    finals = [k for k in raw if k.endswith("final_obs")]
    assert "final_obs" in finals
    for k, v in raw.items():
        if k in finals or v.dtype != torch.float32:
            continue
        left = bits(v) == SENTINEL
        assert not bool(left.any()), (tag, k, f"{int(left.sum())} words were not written, first at {left.nonzero()[:4].tolist()}")
    for k in finals:
        f = bits(raw[k])
        f = f if f.dim() == 4 else f[:, :, None]
        for t in range(f.shape[0]):
            for i in range(f.shape[2]):
                faults = final_obs_faults(f[t, :, i], fl[t] & 1, fl[t] & 2)
                assert not faults, (tag, k, "row", t, "seat", i, faults)


@pytest.mark.parametrize("shape", ["a", "b", "d"])
@_kinds("n", more=False)
def test_the_c_calls_on_pattern_filled_outputs(monkeypatch, kind, shape):
    """the records of cases a, b and d with every output word holding a NaN pattern before the call; the same call through collect()
    from the same state then records the same bits"""
    import torch
    from rsoccer_amd import vec
    n = 2 if shape == "d" else 3
    kind = kind if kind == SELF else (n, n)
    if shape == "a":
        env = vec.VecVSSEnv(131, device=0, seed=2025, max_episode_steps=LIMIT)
    elif shape == "b":
        dense, env = _twins(monkeypatch, lambda: vec.VecVSSEnv(B_PAD, device=0, seed=9, max_episode_steps=LIMIT))
        dense.close()
    else:
        env = _run_time_count(vec, "vss-2v2", 37, device=0, seed=23, max_episode_steps=LIMIT)
    _warm(torch)(env)
    blob = env.checkpoint()
    raw = _raw(torch, env, kind, n)
    _pattern_rules(torch, raw, f"i {shape} {kind}")
    behind = (env.checkpoint(), env.metrics())
    env.restore(blob)
    out = _call(torch, env, kind, n)
    ended = out["terminated"] | out["truncated"]
    for k, v in out.items():
        if k.endswith("log_prob") or k not in raw:   # (computed by collect() in torch; next_obs: the self-play call has no such record)
            assert k.endswith("log_prob") or (kind == SELF and k == "next_obs"), k
            continue
        got = raw[k].cpu().numpy()
        if k.endswith("final_obs"):
            assert _same(got[ended], v[ended]), (shape, k)
        else:
            assert _same(got, v), (shape, k)
    assert np.array_equal(env.checkpoint(), behind[0]) and env.metrics() == behind[1]
    env.close()


# ---- j. split calls ----
@_kinds(3, more=False)
def test_split_calls(kind):
    """collect(T = 5) then collect(T = 7) equals one collect(T = 12) on a twin in every record, checkpoint and metrics: the noise is keyed
    by the handle's tick, the scalars the first call stores are the ones the second loads"""
    import torch
    from rsoccer_amd import vec
    env, twin = (vec.VecVSSEnv(37, device=0, seed=2025, max_episode_steps=LIMIT) for _ in range(2))
    for h in (env, twin):
        _warm(torch)(h)
    first, second = _call(torch, env, kind, 3, steps=5), _call(torch, env, kind, 3, steps=7)
    want = _call(torch, twin, kind, 3)
    assert (want["truncated"].sum(0) == 3).all() and want["truncated"][6].all()   # an end inside each part, one at the second's row 1
    for k, v in want.items():
        got = second[k] if k.endswith("next_obs") else np.concatenate([first[k], second[k]], 0)
        assert _same(got, v), k
    assert not _same(first["sample"][:5], second["sample"][:5])
    assert np.array_equal(env.checkpoint(), twin.checkpoint()) and env.metrics() == twin.metrics()
    assert env.sim.task_tick() == twin.sim.task_tick() == WARM + T
    env.close(); twin.close()
