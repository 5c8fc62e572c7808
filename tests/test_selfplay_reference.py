"""The lockstep reference that goes through episode ends (selfplay_helpers.episode_step: lockstep_episode_step there and in
teamplay_helpers), proven on the CPU before it judges a kernel (tests/test_gpu_selfplay_shapes.py): with no command replaced it is
task_step, bit for bit, through every end; its re-placement by task_reset() is the one an episode end gives; and the conditions the
GPU cases lean on hold — under the oracle's own actions nothing terminates on the shapes used there, every env is truncated three
times, and the directed line-up scores at rows 1, 2 and 4 whoever drives the robots."""
import numpy as np
import pytest

import selfplay_helpers as SH
import teamplay_helpers as TH

LIMIT, WARM, STEPS = 5, 3, 12   # tests/test_gpu_selfplay_shapes.py: TimeLimit 5, three warm steps, T = 12
# (robots a side, envs, seed, env_id_base): every handle the GPU cases compare with the oracle
CONFIGS = SH.SHAPE_CONFIGS


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _pair(O, n, seed, base, nb, warm):
    return (SH.oracle_envs(O, n, seed, base=base, warm=warm, nb=nb, limit=LIMIT) for _ in range(2))


def _follow(refs, twins, actions, step, tag):
    """`step(r, action)` on refs against task_step(action) on twins, every record of every step; -> (terminated rows, truncated rows)"""
    n_term = n_trunc = 0
    for t in range(actions.shape[0]):
        for e, (r, w) in enumerate(zip(refs, twins)):
            row, reward, term, trunc, fin, dropped = step(r, actions[t, e])
            w.task_step(actions[t, e])
            o = w.task_out()
            at = (tag, t, e)
            assert not dropped, at
            assert _same(row, o["obs"]), at                                    # behind an end: the reset row
            assert _same(reward, o["reward"]), at
            assert (term, trunc) == (bool(o["terminated"]), bool(o["truncated"])), at
            assert (fin is not None) == (term or trunc), at
            if fin is not None:
                assert _same(fin, o["final_obs"]), at
            assert r.task_out()["steps"] == o["steps"], at
            assert _same(r.get_state_full(), w.get_state_full()), at
            n_term += term
            n_trunc += trunc
    return n_term, n_trunc


@pytest.mark.parametrize("nb,n,seed,base", CONFIGS, ids=[f"{c[0]}v{c[0]}-B{c[1]}-seed{c[2]}-base{c[3]}" for c in CONFIGS])
def test_with_no_command_replaced_the_reference_is_task_step(oracle_mod, nb, n, seed, base):
    refs, twins = _pair(oracle_mod, n, seed, base, nb, WARM)
    acts = np.random.default_rng(seed).uniform(-1, 1, (STEPS, n, 2)).astype(np.float32)
    team = nb != 3   # the two spellings of "no command replaced": one blue seat and no yellow seat, or no opponent action
    step = (lambda r, a: TH.lockstep_episode_step(r, a[None], np.zeros((0, 2)))) if team else (lambda r, a: SH.lockstep_episode_step(r, a, None))
    n_term, n_trunc = _follow(refs, twins, acts, step, (nb, n))
    # what tests/test_gpu_selfplay_shapes.py leans on: the oracle alone terminates nothing here, every env is truncated at rows 1, 6, 11
    print(f"{nb}v{nb} B={n} seed {seed} base {base}: {n_term} terminated and {n_trunc} truncated rows")
    assert n_term == 0 and n_trunc == 3 * n


@pytest.mark.parametrize("nb", [2, 3, 5])
def test_the_oracle_alone_ends_no_episode_early(oracle_mod, nb):
    """oracle_alone_ends with its nb argument, on the shapes' oracle field; under TimeLimit 1200 nothing ends in 15 steps"""
    assert SH.oracle_alone_ends(oracle_mod, 13, 2025, steps=STEPS, nb=nb) == 0


def _lined_up(O, n, nb, seed=2025):
    refs = SH.oracle_envs(O, n, seed, warm=0, nb=nb, limit=LIMIT)
    half = refs[0].field_params()[0] / 2
    ball, blue, yellow, s, gap = SH.goal_lineup(n, nb, half)
    for e, r in enumerate(refs):
        r.task_reset_to(ball[e], blue[e], yellow[e])
    return refs, half, s, gap


GOAL_ROW = {0.03: 1, 0.06: 2, 0.10: 4}


@pytest.mark.parametrize("nb,half", [(2, 0.75), (3, 0.75), (5, 1.1)])
def test_the_directed_line_up_scores_at_rows_1_2_and_4(oracle_mod, nb, half):
    """resting robots, then every robot under random commands through the reference: the goals fall at the same rows with the same
    rewards, the row-4 goals with both flags set, and with no command replaced the reference is task_step through all of them"""
    n = 13
    refs, got_half, s, gap = _lined_up(oracle_mod, n, nb)
    assert abs(got_half - half) < 1e-12
    twins = _lined_up(oracle_mod, n, nb)[0]
    rest = np.zeros((STEPS, n, 2), dtype=np.float32)
    flags = np.zeros((STEPS, n), int)
    rewards = np.zeros((STEPS, n))

    for t in range(STEPS):   # (one row at a time: the flags of every row are wanted below)
        for e, (r, w) in enumerate(zip(refs, twins)):
            row, reward, term, trunc, fin, dropped = SH.lockstep_episode_step(r, rest[t, e], None)
            w.task_step(rest[t, e])
            o = w.task_out()
            assert not dropped and _same(row, o["obs"]) and _same(reward, o["reward"]), (t, e)
            assert (term, trunc) == (bool(o["terminated"]), bool(o["truncated"])), (t, e)
            assert (fin is None and not (term or trunc)) or _same(fin, o["final_obs"]), (t, e)
            assert _same(r.get_state_full(), w.get_state_full()) and r.task_out()["steps"] == o["steps"], (t, e)
            flags[t, e], rewards[t, e] = term + 2 * trunc, reward
    for e in range(n):
        row = GOAL_ROW[float(gap[e])]
        assert flags[row, e] == (3 if row == 4 else 1) and not flags[:row, e].any(), (e, flags[:, e])
        assert rewards[row, e] == 10.0 * s[e], (e, rewards[row, e])
        assert (flags[row + 1:, e] & 1).sum() == 0   # the episodes behind the goal end at their TimeLimit
    assert (flags == 3).any() and (rewards == 10.0).any() and (rewards == -10.0).any()
    # every robot driven: the reference with all seats replaced by random commands scores at the same rows
    refs = _lined_up(oracle_mod, n, nb)[0]
    rng = np.random.default_rng(nb)
    for t in range(5):
        for e, r in enumerate(refs):
            if t > GOAL_ROW[float(gap[e])]:
                continue
            out = TH.lockstep_episode_step(r, rng.uniform(-1, 1, (nb, 2)), rng.uniform(-1, 1, (nb, 2)))
            assert not out[5], (t, e)
            assert out[2] == (t == GOAL_ROW[float(gap[e])]), ("driven", nb, t, e)
            if out[2]:
                assert out[1] == np.float32(10.0 * s[e]) and out[3] == (t == 4) and np.sign(out[4][0]) == s[e]


@pytest.mark.parametrize("nb", [2, 3, 5])
def test_task_reset_is_the_re_placement_of_an_episode_end(oracle_mod, nb):
    """the reference's branch for a replaced step that ended where the oracle's own did not: task_reset() behind a step leaves the env
    where a twin stands whose own step ended at the same tick — state, reset row, step count, and every later step"""
    n = 6
    ended = _lined_up(oracle_mod, n, nb)[0]                    # gap 0.03 (envs 0 and 3): a goal at row 1
    other = SH.oracle_envs(oracle_mod, n, 2025, warm=0, nb=nb, limit=LIMIT)
    half = other[0].field_params()[0] / 2
    ball, blue, yellow, _, _ = SH.goal_lineup(n, nb, half)
    ball[:, 0], ball[:, 2] = 0.0, 0.0                          # the same robots, the ball at rest in the centre: no goal
    acts = np.random.default_rng(1).uniform(-1, 1, (8, n, 2)).astype(np.float32)
    for e in (0, 3):
        a, b = ended[e], other[e]
        b.task_reset_to(ball[e], blue[e], yellow[e])
        for t in range(2):
            a.task_step(acts[t, e]); b.task_step(acts[t, e])
        assert a.task_out()["terminated"] and not (b.task_out()["terminated"] or b.task_out()["truncated"])
        assert not _same(a.get_state_full(), b.get_state_full())
        b.task_reset()
        assert _same(a.get_state_full(), b.get_state_full()) and _same(a.task_out()["obs"], b.obs_eval())
        assert a.task_out()["steps"] == b.task_out()["steps"] == 0
        for t in range(2, 8):   # OU states, step count, tick and info: everything a later step reads (a truncation at the fifth)
            a.task_step(acts[t, e]); b.task_step(acts[t, e])
            oa, ob = a.task_out(), b.task_out()
            for k in ("obs", "reward", "info") + (("final_obs",) if ob["truncated"] else ()):   # (final_obs: written at ends only)
                assert _same(oa[k], ob[k]), (e, t, k)
            assert (oa["terminated"], oa["truncated"], oa["steps"]) == (ob["terminated"], ob["truncated"], ob["steps"]), (e, t)
        assert ob["truncated"] or ob["steps"] < LIMIT


def test_the_opponent_rows_are_the_mirror_of_a_mirrored_env(oracle_mod):
    """yellow_sincos and the mirror map against the oracle itself: an env built from the point-mirrored placement with the colours
    swapped observes, as blue, what the reference hands out as the opponent's row (== : the placement's -0.0 and +0.0 are equal)"""
    O = oracle_mod
    r = SH.oracle_envs(O, 1, 7, warm=0)[0]
    st = r.get_state_full()
    rob = np.stack([st[5 + 6 * k: 8 + 6 * k] for k in range(6)])
    turned = rob.copy()
    turned[:, 0:2] *= -1.0
    turned[:, 2] = (rob[:, 2] + 180.0) % 360.0
    w = O.OracleEnv(0, 0, 3, 3, 25, "f32")
    w.task_attach(1, 7, 0, 0)
    w.task_reset_to([-st[0], -st[1], 0.0, 0.0], turned[3:], turned[:3])
    got = SH.mirror(r.obs_eval().astype(np.float32), SH.yellow_sincos(r), 3)[0]
    want = w.obs_eval().astype(np.float32)
    shared = np.ones(40, dtype=bool)
    shared[SH.own_sincos_entries(3)] = False
    assert np.all(got[shared] == want[shared])
    assert np.abs(got[~shared] - want[~shared]).max() < 1e-6   # (sin, cos)(th + 180) against -(sin, cos)(th): another argument, not bits
    assert np.abs(got[~shared]).max() > 0.5
