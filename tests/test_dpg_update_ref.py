"""The numpy restatement of the off-policy update phase (tests/dpg_update_helpers.py, the yardstick of tests/test_gpu_dpg_update.py)
checked on its own, without a GPU: the row draw stays inside the filled part, is uniform, is keyed by (seed, step, t) alone; the
two-group Adam with the Polyak step agrees with torch.optim.Adam + clip_grad_norm_ + lerp_ in float64."""
import numpy as np
import pytest

import dpg_update_helpers as H
import ppo_update_helpers as PH


def test_the_four_word_philox_agrees_with_the_one_word_restatement_and_its_words_differ():
    rng = np.random.default_rng(1)
    c = [rng.integers(0, 2 ** 32, size=257, dtype=np.uint64) for _ in range(6)]
    w = H.philox4(*c)
    assert np.array_equal(w[0], PH.philox_word0(*c))
    for a in range(4):
        assert int(w[a].max()) < 2 ** 32
        for b in range(a + 1, 4):
            assert not np.array_equal(w[a], w[b])


@pytest.mark.parametrize("fill", [1, 2, 3, 1000, 2 ** 31 - 1])
def test_every_index_lies_in_the_filled_part(fill):
    rows = H.sample_rows(4099, fill, seed=0xC0FFEE, step=5)
    assert rows.dtype == np.int64 and int(rows.min()) >= 0 and int(rows.max()) < fill
    seen = len(np.unique(rows))
    assert seen == fill if fill <= 3 else seen > 900   # (every row of a small ring is drawn; a large one is covered widely)
    # a fill above the ring is clamped to it, a negative one to 0
    assert np.array_equal(H.sample_rows(64, fill + 7, 1, 2, n_batch_rows=fill), H.sample_rows(64, fill, 1, 2))
    assert np.array_equal(H.sample_rows(64, -3, 1, 2, n_batch_rows=fill), np.full(64, -1))


def test_an_empty_ring_gives_minus_one():
    assert np.array_equal(H.sample_rows(9, 0, seed=3, step=4), np.full(9, -1))


def test_the_draw_is_uniform_by_chi_square():
    """2^16 draws over a fill of 4096 in 64 bins of 64 consecutive rows: the statistic stays under the 0.999 quantile of chi-square with
    63 degrees of freedom (a fixed seed, checked to pass: a uniform draw fails this one time in a thousand)"""
    n, fill, bins = 2 ** 16, 4096, 64
    rows = H.sample_rows(n, fill, seed=20240607, step=11)
    counts = np.bincount(rows // (fill // bins), minlength=bins)
    assert counts.sum() == n and len(counts) == bins
    expect = n / bins
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    bound = PH.chi2_quantile(0.999, bins - 1)
    print(f"chi2 = {chi2:.2f}, bound {bound:.2f}")
    assert 100.0 < bound < 110.0   # (the tabulated value is 103.44)
    assert chi2 < bound
    # and a fill that is no power of two: 1000 rows in 64 bins of unequal width
    rows = H.sample_rows(n, 1000, seed=20240607, step=12)
    edges = (np.arange(bins + 1) * 1000) // bins
    counts = np.histogram(rows, bins=edges)[0]
    expect = n * np.diff(edges) / 1000.0
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print(f"chi2 (fill 1000) = {chi2:.2f}")
    assert counts.sum() == n and chi2 < bound


def test_the_draw_is_keyed_by_seed_step_and_entry_alone():
    a = H.sample_rows(1025, 1000, seed=7, step=40)
    assert not np.array_equal(a, H.sample_rows(1025, 1000, seed=7, step=41))
    assert not np.array_equal(a, H.sample_rows(1025, 1000, seed=8, step=40))
    assert not np.array_equal(a, H.sample_rows(1025, 1000, seed=7, step=40 + 2 ** 32))   # (the high half of the step is part of the key)
    for m in (1, 3, 4, 5, 257):
        assert np.array_equal(H.sample_rows(m, 1000, seed=7, step=40), a[:m])
    assert np.array_equal(H.sample_rows_at(np.array([1024, 5, 0]), 1000, 7, 40), a[[1024, 5, 0]])
    # entries 4 q .. 4 q + 3 are the four words of ONE block: counter word 0 is t >> 2
    w = H.philox4(3, 0, 40, H.DOM_ROWS, 7, 0)
    assert [int((int(x) * 1000) >> 32) for x in w] == a[12:16].tolist()
    # a negative step is its two's complement bits
    assert np.array_equal(H.sample_rows(8, 1000, 7, -1), H.sample_rows(8, 1000, 7, 2 ** 64 - 1))


def _rel(x, ref):
    scale = float(np.abs(ref).max())
    return float(np.abs(np.asarray(x, np.float64) - ref).max()) / scale


@pytest.mark.parametrize("max_norm", [None, 0.5])
def test_the_restated_adam_and_polyak_agree_with_torch_in_float64(max_norm):
    """Criterion (docs/VERIFICATION.md f13): after each of three steps (critic-only, actor, critic-only) the error of every tensor
    against float64 torch.optim.Adam + clip_grad_norm_ + lerp_ is at most 4x the largest error torch's own float32 run shows."""
    import torch
    na, nc, LR_A, LR_C, TAU = 645, 1300, 1e-3, 3e-3, 0.05
    gen = torch.Generator().manual_seed(4)
    start = [torch.randn(n, generator=gen) * 0.3 for n in (na, na, nc, nc)]   # actor, its target, critics, their target
    st = H.fresh_state(na, nc)
    mine = [x.numpy().copy() for x in start]
    runs = {}
    for dt in (torch.float32, torch.float64):
        live = [torch.nn.Parameter(start[0].to(dt).clone()), torch.nn.Parameter(start[2].to(dt).clone())]
        runs[dt] = (live, [start[1].to(dt).clone(), start[3].to(dt).clone()],
                    [torch.optim.Adam([live[0]], lr=LR_A), torch.optim.Adam([live[1]], lr=LR_C)])
    for step, actor in enumerate((False, True, False), 1):
        ga, gc = torch.randn(na, generator=gen), torch.randn(nc, generator=gen)
        for dt, (live, targ, opts) in runs.items():
            for k, g in ((0, ga), (1, gc)):
                if k == 0 and not actor:
                    continue
                live[k].grad = g.to(dt)
                if max_norm is not None:
                    torch.nn.utils.clip_grad_norm_([live[k]], max_norm)
                opts[k].step()
            if actor:
                with torch.no_grad():
                    for k in (0, 1):
                        targ[k].lerp_(live[k].detach(), TAU)
        pa, ta, pc, tc, stats = H.dpg_adam_step(st, mine[0], mine[1], mine[2], mine[3], ga.numpy() if actor else None, gc.numpy(), LR_A, LR_C,
                                                max_norm=max_norm, tau=TAU)
        if not actor:
            assert np.array_equal(pa, mine[0]) and np.array_equal(ta, mine[1]) and np.array_equal(tc, mine[3]) and stats[1] == 0.0 and stats[2] == 0.0
        mine = [pa, ta, pc, tc]
        l64, t64, o64 = runs[torch.float64]
        l32, t32, o32 = runs[torch.float32]
        ref = [l64[0].detach().numpy(), t64[0].numpy(), l64[1].detach().numpy(), t64[1].numpy()]
        yard = [l32[0].detach().numpy(), t32[0].numpy(), l32[1].detach().numpy(), t32[1].numpy()]
        names = ["actor", "target_actor", "critics", "target_critics"]
        if o64[1].state:
            ref += [o64[1].state[l64[1]]["exp_avg"].numpy(), o64[1].state[l64[1]]["exp_avg_sq"].numpy()]
            yard += [o32[1].state[l32[1]]["exp_avg"].numpy(), o32[1].state[l32[1]]["exp_avg_sq"].numpy()]
            mine_mv = [st["m"][1], st["v"][1]]
            names += ["m_critics", "v_critics"]
        if o64[0].state:
            ref += [o64[0].state[l64[0]]["exp_avg"].numpy(), o64[0].state[l64[0]]["exp_avg_sq"].numpy()]
            yard += [o32[0].state[l32[0]]["exp_avg"].numpy(), o32[0].state[l32[0]]["exp_avg_sq"].numpy()]
            mine_mv += [st["m"][0], st["v"][0]]
            names += ["m_actor", "v_actor"]
        got = mine + mine_mv
        e_yard = max(_rel(y, r) for y, r in zip(yard, ref))
        for name, g, r in zip(names, got, ref):
            e = _rel(g, r)
            print(f"step {step} {name}: restatement {e:.3e}, torch f32 pooled {e_yard:.3e}")
            assert e <= 4.0 * e_yard, (step, name, e, e_yard)
        assert e_yard > 0.0
    assert st["counters"] == [3, 1, 3, 0]


def test_the_polyak_step_rounds_each_of_its_three_operations():
    f32 = np.float32
    p, targ = np.array([1.0000001, -3.5, 0.25], f32), np.array([1.0, 2.0, 0.25], f32)
    out = H.polyak(p, targ, 0.005)
    d = (p - targ).astype(f32)
    assert np.array_equal(out, (targ + (f32(0.005) * d).astype(f32)).astype(f32))
    assert np.array_equal(H.polyak(p, targ, 0.0), targ) and np.array_equal(H.polyak(p, targ, 1.0), (targ + d).astype(f32))
    assert out[2] == f32(0.25)
