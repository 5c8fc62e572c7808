"""The numpy restatements of prioritised and n-step replay (tests/per_helpers.py) against definitions, no GPU: the n-step fold against a
brute-force float64 loop over the episode, the descent on trees whose answer is known, and the draw's empirical frequencies against
leaf / total."""
import numpy as np
import pytest

import per_helpers as PH

f32 = np.float32


@pytest.mark.parametrize("n_step", [1, 2, 3, 4, 16])
@pytest.mark.parametrize("T,B", [(5, 1), (5, 3), (5, 65), (1, 4)])
def test_the_fold_is_the_brute_force_n_step_transition(T, B, n_step):
    """the batch holds an end at t = 0 and at t = T - 1, two ends closer together than n, a truncation with terminated = 0, n > T
    (n = 16) and n = 1"""
    rng = np.random.default_rng(100 * T + B)
    b = PH.fold_case(rng, T, B) if T > 1 else PH.make_batch(rng, T, B, 3, 2, ends=((0, 1),))
    if T > 1:
        assert b["terminated"][0].any() and b["terminated"][T - 1].any() and (b["truncated"] & ~b["terminated"]).any()
    gamma = 0.97
    R, G, term, m, kind, at = PH.fold(b["reward"], b["terminated"], b["truncated"], n_step, gamma)
    R64, G64, term64, m64, kind64, at64 = PH.brute_nstep(b["reward"], b["terminated"], b["truncated"], n_step, gamma)
    assert np.array_equal(m, m64) and np.array_equal(term, term64) and np.array_equal(kind, kind64) and np.array_equal(at, at64)
    assert m.max() <= min(n_step, T) and m.min() == 1
    # float32 rounding: m terms of magnitude <= sum |r|, each rounded a bounded number of times
    mag = np.abs(b["reward"]).astype(np.float64).sum(axis=0, keepdims=True)
    assert np.all(np.abs(R.astype(np.float64) - R64) <= 2.0 ** -23 * n_step * mag + 1e-30)
    assert np.all(np.abs(G.astype(np.float64) / G64 - 1.0) <= 2.0 ** -23 * (n_step + 1))
    if n_step == 1:
        assert np.array_equal(R, b["reward"]) and np.all(G == f32(gamma)) and np.array_equal(term, b["terminated"])


def test_a_window_never_crosses_an_episode_end_and_the_tail_rows_get_fewer_steps():
    T, B = 6, 2
    rew = np.arange(1, T * B + 1, dtype=f32).reshape(T, B)
    term, trunc = np.zeros((T, B), bool), np.zeros((T, B), bool)
    term[2, 0] = True
    R, G, t_out, m, kind, at = PH.fold(rew, term, trunc, 3, 0.5)
    assert m[:, 0].tolist() == [3, 2, 1, 3, 2, 1] and m[:, 1].tolist() == [3, 3, 3, 3, 2, 1]
    assert R[0, 0] == f32(1 + 0.5 * 3 + 0.25 * 5) and R[1, 0] == f32(3 + 0.5 * 5) and R[3, 0] == f32(7 + 0.5 * 9 + 0.25 * 11)
    assert t_out[:, 0].tolist() == [True, True, True, False, False, False]
    assert kind[:, 0].tolist() == [0, 0, 0, 2, 2, 2] and at[:3, 0].tolist() == [2 * B, 2 * B, 2 * B]
    assert kind[:, 1].tolist() == [1, 1, 1, 2, 2, 2] and at[:3, 1].tolist() == [3 * B + 1, 4 * B + 1, 5 * B + 1]
    assert G[5, 1] == f32(0.5) and G[4, 1] == f32(0.25) and G[0, 1] == f32(0.125)


def test_the_ring_add_places_rows_step_major_and_wraps():
    rng = np.random.default_rng(3)
    ring = PH.new_ring(10, 3, 2)
    b = PH.make_batch(rng, 2, 3, 3, 2)
    assert PH.ring_add(ring, b, 1, 0.9).tolist() == [0, 1, 2, 3, 4, 5]
    assert PH.ring_add(ring, b, 1, 0.9).tolist() == [6, 7, 8, 9, 0, 1] and (ring["head"], ring["fill"]) == (2, 10)
    assert np.array_equal(ring["obs"][9], b["obs"][1, 0]) and np.array_equal(ring["next_obs"][6], b["obs"][1, 0])
    assert np.array_equal(ring["next_obs"][9], b["next_obs"][0])


@pytest.mark.parametrize("capacity,levels", [(1, 1), (63, 1), (64, 1), (65, 2), (4096, 2), (4097, 3), (5000, 3), (2 ** 31 - 1, 6)])
def test_the_tree_geometry(capacity, levels):
    floats, lv, off = PH.tree_geometry(capacity)
    assert lv == levels and off[0] == 0 and all(o % 64 == 0 for o in off) and floats == off[-1] + 64
    assert off[1] >= capacity and off[1] - capacity < 64


@pytest.mark.parametrize("capacity", [1, 63, 64, 65, 4097, 5000])
def test_on_equal_priorities_the_descent_returns_the_stratums_own_row(capacity):
    tree = PH.build_tree(np.ones(capacity, f32), capacity)
    PH.check_tree(tree, capacity)
    for step in range(3):
        assert np.array_equal(PH.descend(tree, capacity, capacity, capacity, 7, step), np.arange(capacity))


def test_the_descent_never_returns_a_zero_leaf_and_an_empty_tree_gives_minus_one():
    rng = np.random.default_rng(5)
    for capacity in (65, 700, 4097):
        leaves = rng.uniform(0.1, 2.0, capacity).astype(f32)
        leaves[rng.random(capacity) < 0.7] = 0
        leaves[capacity - 1] = 0
        leaves[3] = f32(1e9)   # one leaf that swallows its neighbours' sums in float32
        tree = PH.build_tree(leaves, capacity)
        for step in range(4):
            rows = PH.descend(tree, capacity, capacity, 257, 11, step)
            assert rows.min() >= 0 and rows.max() < capacity and np.all(leaves[rows] > 0)
            assert np.all(np.diff(rows) >= 0)   # strata are ordered
        w = PH.weights64(tree, capacity, capacity, rows, 0.4)
        assert w.max() == 1.0 and w.min() > 0
        assert np.array_equal(PH.descend(PH.build_tree(np.zeros(capacity, f32), capacity), capacity, capacity, 9, 1, 0), np.full(9, -1))
        assert np.array_equal(PH.descend(tree, capacity, 0, 9, 1, 0), np.full(9, -1))
    # u pushed to the total: the last stratum's word at its largest still lands on a leaf that holds something
    leaves = np.zeros(130, f32)
    leaves[[0, 70]] = f32(0.1), f32(0.2)
    tree = PH.build_tree(leaves, 130)
    assert set(PH.descend(tree, 130, 130, 64, 0, 0).tolist()) == {0, 70}


def test_the_draws_frequencies_follow_the_leaves():
    """m = 8 strata over 40 leaves, 4000 steps: 32 000 draws.  A stratified draw's count of a leaf is a sum of independent Bernoulli
    variables whose variance is at most the binomial's, so five binomial standard deviations hold a fortiori; the smallest expected
    count is 32 000 * 0.5 / 61 = 262, far from the small-count regime."""
    capacity, m, steps = 40, 8, 4000
    leaves = np.linspace(0.5, 2.5, capacity).astype(f32)
    tree = PH.build_tree(leaves, capacity)
    counts = np.zeros(capacity, np.int64)
    for step in range(steps):
        np.add.at(counts, PH.descend(tree, capacity, capacity, m, 2024, step), 1)
    n = m * steps
    p = leaves.astype(np.float64) / leaves.astype(np.float64).sum()
    z = (counts - n * p) / np.sqrt(n * p * (1 - p))
    print("largest |z|", np.abs(z).max())
    assert counts.sum() == n and np.abs(z).max() < 5.0


def test_duplicates_keep_the_largest_value_and_bad_indices_are_skipped():
    leaves = np.zeros(8, f32)
    skipped = PH.set_priorities_rows(leaves, [1, 1, 1, -1, 8, 5], np.array([0.3, 0.9, 0.5, 7, 7, 0.2], f32))
    assert skipped == 2 and leaves[1] == f32(0.9) and leaves[5] == f32(0.2) and leaves.sum() == f32(0.9) + f32(0.2)
    PH.set_priorities_rows(leaves, [1], np.array([0.1], f32))   # a later call overwrites: the maximum is over one call's entries
    assert leaves[1] == f32(0.1)
