"""Per-env physics (rsx_physics_enable) against the f32 oracle on EVERY kernel variant: the handle runs task_step_phys_kernel /
sim_step_phys_kernel, one instantiation per row of rsx_variants.hpp, and a coefficient that one of them takes from the compiled-in
literal instead of the env's row is wrong only for non-default values.  So: every env its own values, the oracle env carrying the
same derived coefficients (tests/physics_helpers.py), bit patterns compared after every step — and, before anything is compared,
the oracle alone establishes that the scenario CAN fail: which parameters change its outcome (tests/physics_scenarios.py; the
table is in docs/VERIFICATION.md)."""
import numpy as np
import pytest

import physics_scenarios as S
from helpers import f32_equal, mismatch_report
from physics_helpers import NAMES, derive, set_oracle_coefs
from test_gpu_parity import TASKS, _cmp_task
from test_gpu_physics_params import _expected_draw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from rsoccer_amd import _lib
    return _lib


def _assert_live(O, sc):
    live = S.live_params(O, sc)
    print(f"{sc.name}: live {live}")
    assert len(live) >= S.MIN_LIVE, f"{sc.name} cannot see enough: only {live} change its outcome"


def _assert_params(L, sim, kind, raw, tag):
    got_raw, got_coef = sim.physics_get(L.PHYS_RAW), sim.physics_get(L.PHYS_COEF)
    for e in range(raw.shape[0]):
        assert got_raw[:, e].tobytes() == raw[e].tobytes(), (tag, "raw", e, got_raw[:, e], raw[e])
        assert got_coef[:, e].tobytes() == derive(kind, 25, raw[e]).tobytes(), (tag, "coef", e)


# ---- 1. raw step ----
@pytest.mark.parametrize("i", range(len(S.RAW_NAMES)), ids=S.RAW_NAMES)
def test_raw_step_with_heterogeneous_physics_is_bit_exact(L, oracle_mod, i):
    """sim_step_phys_kernel of every variant (wheel and local commands, kicks, chips, dribbler): full state after every step; one
    handle switched to per-env physics before its reset, one after"""
    O = oracle_mod
    sc = S.raw_scenarios(O)[i]
    assert sc.name == S.RAW_NAMES[i]
    _assert_live(O, sc)
    sims = []
    for after in (False, True):
        sim = L.Sim(sc.kind, sc.ft, sc.nb, sc.ny, 25, sc.B)
        if not after:
            sim.physics_enable()
        sim.reset(sc.ball, sc.blue, sc.yellow if sc.ny else None)
        if after:
            sim.physics_enable()
        if sc.spin is not None:
            st = sim.get_state_full()
            st[:, -1] = sc.spin
            sim.set_state(st)
        sim.physics_set(sc.raw.T.copy())
        _assert_params(L, sim, sc.kind, sc.raw, sc.name)
        sims.append(sim)

    def compare(t, refs):
        want = np.stack([r.get_state_full() for r in refs])
        for k, sim in enumerate(sims):
            sim.step(sc.cmds[t])
            got = sim.get_state_full()
            if not f32_equal(got, want):
                e = int(np.argwhere((got.astype(np.float32) != want.astype(np.float32)).any(axis=1))[0, 0])
                raise AssertionError(mismatch_report(got[e], want[e], f"{sc.name} handle {k} env {e} step {t}"))

    S.run_raw(O, sc, sc.raw, compare)
    for sim in sims:
        sim.close()


# ---- 2. fused tasks ----
def _feed(torch, sim, tens, a):
    tens["actions"].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    sim.task_step(tens["actions"].data_ptr())


def _assert_metrics(sim, refs, tag):
    got, want = sim.read_metrics(), sum(r.task_out()["metrics"] for r in refs)
    assert np.array_equal(got, want), (tag, got, want)


@pytest.mark.parametrize("i", range(len(S.TASK_NAMES)), ids=S.TASK_NAMES)
def test_fused_task_with_heterogeneous_physics_is_bit_exact(L, oracle_mod, i):
    """task_step_phys_kernel of every variant: fed actions through task_step, device-drawn actions through task_step_n, task_rollout and
    single steps with auto-resets on the way, a task_reset_to onto a line-up that brings every contact kind into play"""
    import torch
    O = oracle_mod
    sc = S.task_scenarios(O)[i]
    assert sc.name == S.TASK_NAMES[i]
    _assert_live(O, sc)
    sim = L.Sim(sc.kind, sc.ft, sc.nb, sc.ny, 25, sc.B)
    sim.task_attach(sc.task, sc.seed, sc.base, sc.max_steps)
    sim.physics_enable()
    sim.physics_set(sc.raw.T.copy())
    _assert_params(L, sim, sc.kind, sc.raw, sc.name)
    tens = sim.task_tensors()
    refs = S.task_oracles(O, sc, sc.raw)
    sim.task_reset()
    t = 0
    for k, (mode, arg) in enumerate(sc.program):
        if mode == "fed":
            for a in arg:
                _feed(torch, sim, tens, a)
                for e, r in enumerate(refs):
                    r.task_step(a[e])
                _cmp_task(sim, refs, tens, (k, t))
                t += 1
        elif mode == "random":
            for _ in range(arg):
                sim.task_step(None)
                O.vec_task_step(refs, 1)
                _cmp_task(sim, refs, tens, (k, t))
                t += 1
        elif mode == "reset_to":
            sim.task_reset_to(*arg)
            for e, r in enumerate(refs):
                r.task_reset_to(arg[0][e], arg[1][e], arg[2][e])
            torch.cuda.synchronize()
            obs, st = tens["obs"].cpu().numpy(), sim.get_state_full()
            for e, r in enumerate(refs):
                assert f32_equal(obs[e], r.task_out()["obs"]) and f32_equal(st[e], r.get_state_full()), (sc.name, "reset_to", e)
        else:
            (sim.task_step_n if mode == "step_n" else sim.task_rollout)(arg)
            O.vec_task_step(refs, arg)
            t += arg
            _cmp_task(sim, refs, tens, (k, mode))
        _assert_metrics(sim, refs, (sc.name, k, mode))
    assert sim.read_metrics()[1] > 0   # auto-resets on the way
    _assert_params(L, sim, sc.kind, sc.raw, sc.name)   # nothing redraws without ranges
    sim.close()


# ---- 4. every parameter is seen somewhere ----
@pytest.mark.parametrize("part", ["raw", "tasks"])
def test_every_parameter_is_live_in_some_scenario(oracle_mod, part):
    O = oracle_mod
    scs = S.raw_scenarios(O) if part == "raw" else S.task_scenarios(O)
    for kind in (0, 1):
        seen = set()
        for sc in scs:
            if sc.kind == kind:
                seen |= set(S.live_params(O, sc))
        missing = [n for n in S.valid_params(kind) if n not in seen]
        assert not missing, f"{part}, kind {kind}: no scenario sees {missing}"


# ---- 3. randomisation ----
RANGES = {"m_ball": (0.04, 0.05), "e_rb": (0.1, 0.9), "e_wr": (0.0, 0.5), "mu_rr": (0.1, 0.4), "mu_g": (0.2, 0.6), "spin_dec": (15.0, 45.0),
          "a_lin": (4.0, 9.0), "a_lat": (10.0, 30.0)}
SEED, BASE = 0xFEEDFACE12345, 1000


def _randomised_run(L, O, i, row, n_total, reset_at, launches=(5, 1, 9, 3)):
    """two handles of one randomised configuration — one stepped, one advanced by task_rollout launches — against oracle envs whose
    coefficients the test redraws itself: at task_reset (episode 0), after every reported episode end and for the envs flagged in a
    task_reset_to"""
    import torch
    task, kind, ft, nb, ny, B, _, max_steps = row
    names = [n for n in RANGES if kind == 0 or n != "a_lat"]
    lo = np.zeros(len(NAMES), np.float32); hi = np.zeros(len(NAMES), np.float32); mask = 0
    for n in names:
        p = NAMES.index(n); lo[p], hi[p] = RANGES[n]; mask |= 1 << p
    cur = S.hetero_params(kind, B, 600 + i)
    sims = []
    for _ in range(2):
        s = L.Sim(kind, ft, nb, ny, 25, B)
        s.task_attach(task, SEED, BASE, max_steps)
        s.physics_enable()
        s.physics_set(cur.T.copy())
        s.physics_randomize(lo, hi, mask)
        s.task_reset()
        sims.append(s)
    stepper, roller = sims
    tens = [s.task_tensors() for s in sims]
    refs = []
    for e in range(B):
        r = O.OracleEnv(kind, ft, nb, ny, 25, "f32")
        r.task_attach(task, SEED, BASE + e, max_steps)
        r.task_reset()
        refs.append(r)
    episode = np.zeros(B, int)

    def redraw(e):
        for n in names:
            p = NAMES.index(n)
            cur[e, p] = _expected_draw(O, SEED, BASE + e, int(episode[e]), p, lo[p], hi[p])
        set_oracle_coefs(refs[e], derive(kind, 25, cur[e]))

    for e in range(B):
        redraw(e)
    for s in sims:
        _assert_params(L, s, kind, cur, "episode 0")
    rng = np.random.default_rng(70 + i)
    place = S.directed_lineup(O, task, kind, ft, nb, ny, B, rng)
    flagged = (rng.random(B) < 0.5).astype(np.uint8)
    flagged[0], flagged[-1] = 1, 0
    behind, launch = 0, 0
    for t in range(n_total):
        if t == reset_at:
            if behind:
                roller.task_rollout(behind); behind = 0
                _cmp_task(roller, refs, tens[1], ("rollout before reset_to", t))
            for s in sims:
                s.task_reset_to(place[0], place[1], place[2], flagged)
            for e in np.flatnonzero(flagged):
                refs[e].task_reset_to(place[0][e], place[1][e], place[2][e])
                episode[e] += 1
                redraw(e)
            for k, s in enumerate(sims):
                _assert_params(L, s, kind, cur, ("reset_to", k))
                st = s.get_state_full()
                for e, r in enumerate(refs):
                    assert f32_equal(st[e], r.get_state_full()), ("reset_to", k, e)
        stepper.task_step(None)
        O.vec_task_step(refs, 1)
        _cmp_task(stepper, refs, tens[0], t)
        ended = [e for e, r in enumerate(refs) if r.task_out()["terminated"] or r.task_out()["truncated"]]
        for e in ended:
            episode[e] += 1
            redraw(e)
        if ended:
            _assert_params(L, stepper, kind, cur, ("step", t))
        behind += 1
        if behind == launches[launch % len(launches)] or t == n_total - 1:
            roller.task_rollout(behind); behind = 0; launch += 1
            _cmp_task(roller, refs, tens[1], ("rollout", t))
            _assert_params(L, roller, kind, cur, ("rollout", t))
    for k, s in enumerate(sims):
        got, want = s.read_metrics(), sum(r.task_out()["metrics"] for r in refs)
        assert np.array_equal(got, want), (k, got, want)
    assert episode.min() >= 2, episode   # every env stepped with redrawn values, more than once
    return sims


@pytest.mark.parametrize("i", range(len(TASKS)), ids=S.TASK_NAMES)
def test_randomised_physics_follows_the_oracle_through_redraws(L, oracle_mod, i):
    """the redraw at auto-resets (single steps and inside task_rollout launches) and at a masked task_reset_to is the documented
    Philox draw, a_lat stays 0 on SSL handles, and the steps after a redraw use the new coefficients: the oracle carries them"""
    row = TASKS[i]
    max_steps = row[7]
    for s in _randomised_run(L, oracle_mod, i, row, 2 * max_steps + 12, max_steps + 5):
        if row[1] == 1:
            assert (s.physics_get(L.PHYS_RAW)[NAMES.index("a_lat")] == 0).all()
        s.close()


@pytest.mark.parametrize("cache", [True, False], ids=["placement-cache", "no-placement-cache"])
def test_randomised_static_defenders_next_to_the_placement_cache(L, oracle_mod, monkeypatch, cache):
    """a handle that owns a placement cache (and its counters) and one without: the per-env physics kernels launch tiles only and place
    every reset inline (rsx_task_step_body.inc: PC is off for PHYS), so both follow the oracle through the redraws and the cache, where
    there is one, is never consulted — its counters stay at zero while episodes end"""
    monkeypatch.setenv("RSX_PCACHE_STATS", "1")
    if not cache:
        monkeypatch.setenv("RSX_NO_PCACHE", "1")
    else:
        monkeypatch.delenv("RSX_NO_PCACHE", raising=False)
    row = (2, 1, 2, 1, 6, 37, 0, 9)
    sims = _randomised_run(L, oracle_mod, 1, row, 64, 30)
    for s in sims:
        hits, inline = s.placement_cache_stats()
        print("placement cache:", hits, inline)
        assert s.read_metrics()[1] > 0   # resets happened
        # (counters are handed out only together with a cache buffer: (0, 0) says that the handle owns one, (-1, -1) that it does not)
        assert (hits, inline) == ((0, 0) if cache else (-1, -1))
        s.close()
