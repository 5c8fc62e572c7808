"""The construction of rsx_ppo_permutation (include/rsx.h) checked on its numpy restatement, no GPU: it is an exact bijection, its
chunks are torch.chunk's, its three key parts all matter and single outputs and pair differences are uniform over the keys; and the
restatements of the normalisation and of clip + Adam agree with float64 / torch to rounding."""
import numpy as np
import pytest

import ppo_update_helpers as H


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_the_permutation_is_an_exact_bijection(n):
    for seed, update, epoch in ((0, 0, 0), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1), (0x1234567890ABCDEF, 7, 3)):
        rows = H.permutation(n, seed, update, epoch)
        assert rows.shape == (n,) and np.array_equal(np.sort(rows), np.arange(n)), (n, seed, update, epoch)


def test_the_feistel_network_is_a_bijection_of_its_whole_domain():
    for bits in (8, 9, 11):
        x = H.feistel(np.arange(1 << bits), bits, 99, 5, 2).astype(np.int64)
        assert np.array_equal(np.sort(x), np.arange(1 << bits)), bits


@pytest.mark.parametrize("n,mb", [(65, 2), (1025, 4), (64, 4), (4097, 3)])
def test_chunk_boundaries_equal_torch_chunk(n, mb):
    import torch
    rows = H.permutation(n, 1, 2, 3)
    want = torch.from_numpy(rows).chunk(mb)
    got = H.chunks(n, mb)
    assert len(want) == len(got) == mb
    for (lo, hi), w in zip(got, want):
        assert np.array_equal(rows[lo:hi], w.numpy())


def test_every_part_of_the_key_changes_the_permutation():
    n = 1025
    base = H.permutation(n, 11, 4, 2)
    assert np.array_equal(base, H.permutation(n, 11, 4, 2))
    others = [H.permutation(n, 12, 4, 2), H.permutation(n, 11 + (1 << 32), 4, 2), H.permutation(n, 11, 5, 2), H.permutation(n, 11, 4, 3)]
    for k, o in enumerate(others):
        # (two independent uniform permutations of 1025 agree in one place on average; half of the places is far from that)
        assert int((o == base).sum()) < n // 2, k
    for a in range(len(others)):
        for b in range(a + 1, len(others)):
            assert not np.array_equal(others[a], others[b])
    # the update count enters with its low 32 bits, as the header says
    assert np.array_equal(H.permutation(n, 11, 4 + (1 << 32), 2), base)


@pytest.mark.parametrize("n", [64, 65])
def test_single_outputs_and_pair_differences_are_uniform_over_4096_keys(n):
    """4096 keys (64 seeds x 8 updates x 8 epochs).  Histogram 1: rows[0], n cells.  Histogram 2: (rows[1] - rows[0]) mod n, which
    cannot be 0: n - 1 cells.  Each chi-square statistic stays below the 1 - 1e-6 quantile of its distribution."""
    s, u, e = (a.ravel() for a in np.meshgrid(np.arange(64) * 7919 + 1, np.arange(8), np.arange(8), indexing="ij"))
    K = s.size
    assert K == 4096
    r0, r1 = H.permute(0, n, s, u, e), H.permute(1, n, s, u, e)
    h0 = np.bincount(r0, minlength=n)
    diff = np.bincount((r1 - r0) % n, minlength=n)
    assert diff[0] == 0 and h0.sum() == K and diff.sum() == K
    for name, hist in (("rows[0]", h0), ("rows[1] - rows[0]", diff[1:])):
        expect = K / hist.size
        stat = float(((hist - expect) ** 2 / expect).sum())
        bound = H.chi2_quantile(1.0 - 1e-6, hist.size - 1)
        print(f"n = {n}, {name}: chi-square {stat:.1f} with {hist.size - 1} degrees of freedom, bound {bound:.1f}")
        assert stat < bound, (name, stat, bound)


def test_the_quantile_is_the_chi_square_distributions():
    # known values: the 0.95 quantile with 10 degrees of freedom is 18.307, the 0.999 quantile with 63 is 103.442
    assert abs(H.chi2_quantile(0.95, 10) - 18.3070) < 1e-3
    assert abs(H.chi2_quantile(0.999, 63) - 103.442) < 1e-2
    assert 130.0 < H.chi2_quantile(1.0 - 1e-6, 63) < 135.0


@pytest.mark.parametrize("n", [2, 65, 4097, 70001])
def test_the_normalisation_restatement_is_float64s_to_rounding(n):
    rng = np.random.default_rng(n)
    a = (rng.standard_normal(n) * 3.0 + 1.5).astype(np.float32)
    out, mean, std = H.normalize(a)
    a64 = a.astype(np.float64)
    ref = (a64 - a64.mean()) / (a64.std(ddof=1) + 1e-8)
    assert abs(float(mean) - a64.mean()) <= 2.0 ** -24 * abs(a64.mean()) and abs(float(std) - a64.std(ddof=1)) <= 2.0 ** -24 * a64.std(ddof=1)
    # mean and std each half an ulp, then three float32 roundings per entry
    assert np.abs(out - ref).max() <= 4.0 * 2.0 ** -24 * max(1.0, np.abs(ref).max())


def _header_order_sum(x, cap):
    """include/rsx.h's reduction order as the header words it, one scalar float64 addition at a time: thread j of workgroup w adds its
    elements 256 w + j, + 256 G, ... from 0.0; the 64 lanes of a wave ascending from 0.0; the waves ((w0 + w1) + w2) + w3; the G
    partials in workgroup order from 0.0"""
    x = [float(v) for v in x]
    n = len(x)
    G = min((n + 255) // 256, cap)
    total = 0.0
    for w in range(G):
        waves = []
        for wave in range(4):
            acc = 0.0
            for lane in range(64):
                mine, i = 0.0, 256 * w + 64 * wave + lane
                while i < n:
                    mine += x[i]
                    i += 256 * G
                acc += mine
            waves.append(acc)
        total += ((waves[0] + waves[1]) + waves[2]) + waves[3]
    return total


def _wide_input(n, seed):
    """float64 entries of both signs spread over 30 binary orders of magnitude"""
    rng = np.random.default_rng(seed)
    return rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-15, 16, n)) * rng.choice([-1.0, 1.0], n)


FIXED_SUM_CASES = [(cap, n) for cap in (1, 2, 3) for n in (255, 256, 257, 513, 1500, 2049)] + [(128, 32769), (64, 16385)]


@pytest.mark.parametrize("cap,n", FIXED_SUM_CASES)
def test_fixed_sum_is_the_headers_order_beyond_one_trip(cap, n):
    """fixed_sum's array code against the scalar loop above, on bit patterns, at sizes where a thread holds two and more elements;
    both within the float64 bound of recursive summation in any order, (n - 1) u / (1 - (n - 1) u) * sum |x| with u = 2^-53"""
    import math
    for k, x in enumerate((_wide_input(n, 100 * cap + n), np.random.default_rng(n + cap).normal(3.0, 0.5, n).astype(np.float32).astype(np.float64))):
        got, want = H.fixed_sum(x, cap), _header_order_sum(x, cap)
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), (cap, n, k, float(got), want)
        u = 2.0 ** -53
        bound = (n - 1) * u / (1.0 - (n - 1) * u) * math.fsum(abs(v) for v in x)
        exact = math.fsum(x)
        assert abs(float(got) - exact) <= bound and abs(want - exact) <= bound, (cap, n, k)


def test_another_order_gives_other_bits():
    """the proof that the comparison above can fail: on the wide input a plain ascending sum differs from the fixed order in bits"""
    n, cap = 2049, 3
    x = _wide_input(n, 100 * cap + n)
    plain = 0.0
    for v in x:
        plain += float(v)
    fixed = _header_order_sum(x, cap)
    assert np.float64(plain).tobytes() != np.float64(fixed).tobytes()
    assert np.float64(H.fixed_sum(x, cap)).tobytes() == np.float64(fixed).tobytes()
    # one trip fewer (a cap that holds every element in a first trip) is another order as well
    assert np.float64(_header_order_sum(x, 9)).tobytes() != np.float64(fixed).tobytes()


def test_the_clip_adam_restatement_follows_torch():
    import torch
    rng = np.random.default_rng(3)
    sizes = (300, 5, 77)
    p = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    m = [np.zeros(n, np.float32) for n in sizes]
    v = [np.zeros(n, np.float32) for n in sizes]
    tp = [torch.nn.Parameter(torch.from_numpy(x.astype(np.float64))) for x in p]
    opt = torch.optim.Adam(tp, lr=1e-2)
    for t in range(1, 6):
        g = [(rng.standard_normal(n) * (3.0 if t % 2 else 0.01)).astype(np.float32) for n in sizes]
        for x, gi in zip(tp, g):
            x.grad = torch.from_numpy(gi.astype(np.float64))
        want_norm = float(torch.nn.utils.clip_grad_norm_(tp, 0.5))
        opt.step()
        p, m, v, norm = H.clip_adam(p, g, m, v, t, 1e-2, max_norm=0.5)
        assert abs(float(norm) - want_norm) <= 2.0 ** -23 * want_norm
        for a, b in zip(p, tp):
            assert np.abs(a - b.detach().numpy()).max() <= 1e-6
    # no clipping: max_norm None and <= 0 give the same bits
    g = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    a, b = H.clip_adam(p, g, m, v, 6, 1e-2, max_norm=None), H.clip_adam(p, g, m, v, 6, 1e-2, max_norm=0.0)
    for x, y in zip(a[0] + a[1] + a[2], b[0] + b[1] + b[2]):
        assert np.array_equal(x, y)
