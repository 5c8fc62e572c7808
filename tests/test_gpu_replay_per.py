"""Prioritised and n-step replay on the device (PrioritizedReplayBuffer): add() against the fold's numpy restatement bit for bit, the
tree's invariants after every operation, sample() against the descent's restatement on the tree read back, update_priorities()
(duplicates, skipped indices, the running maximum) with leaf and weight values held against float64 under torch.pow's own float32
error, and a captured collect + add + sample + dpg_gradient + step + update_priorities against eager iterations."""
import numpy as np
import pytest

import per_helpers as PH

pytestmark = pytest.mark.gpu

f32 = np.float32
ULP = 2.0 ** -23
RING_KEYS = ("obs", "actions", "reward", "next_obs", "terminated", "discount")


def _dev():
    import torch
    return torch.device("cuda", 0)


def _to(torch, batch, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in batch.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _ring_equal(buf, ring):
    import torch
    torch.cuda.synchronize()
    for k in RING_KEYS:
        got = getattr(buf, k).cpu().numpy()
        assert got.dtype == ring[k].dtype and np.array_equal(_bits(got), _bits(ring[k])), k
    assert (int(buf.head), int(buf.fill)) == (ring["head"], ring["fill"])
    assert int(buf.state[3]) == 0   # the add's ticket is back at 0


def _tree(buf):
    import torch
    torch.cuda.synchronize()
    tree = buf.tree.cpu().numpy()
    PH.check_tree(tree, buf.capacity)
    floats, levels, off = PH.tree_geometry(buf.capacity)
    assert (floats, levels, off) == (int(buf.tree.shape[0]), buf.tree_levels, buf.tree_offsets)
    return tree


def _pow_bound(torch, base, expo, dev):
    """4 x the worst relative error of torch.pow in float32 on the same inputs on the same device, at least one float32 ulp; and
    that worst error itself"""
    base = np.asarray(base, f32).reshape(-1)
    ref = base.astype(np.float64) ** float(f32(expo))
    got = torch.pow(torch.from_numpy(base).to(dev), torch.tensor(f32(expo), device=dev)).cpu().numpy().astype(np.float64)
    ok = ref > 0
    worst = float(np.max(np.abs(got[ok] - ref[ok]) / ref[ok])) if ok.any() else 0.0
    return max(4.0 * worst, ULP), worst


def _worst(got, ref):
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    ok = ref > 0
    assert np.array_equal(got[~ok], ref[~ok])
    return float(np.max(np.abs(got[ok] - ref[ok]) / ref[ok])) if ok.any() else 0.0


# ---- a. add() ----
@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("n_step", [1, 3, 16])
def test_add_equals_the_fold_restatement_in_every_ring_array_bit_for_bit(B, n_step):
    """T = 5; three adds into a ring of 2 * T * B + 2 rows: the third wraps around the end and overwrites rows whose priorities were
    raised in between.  New rows carry the running maximum; with n_step = 1 a plain ReplayBuffer twin holds the same bytes."""
    import torch
    from rsoccer_amd.vec.replay import PrioritizedReplayBuffer, ReplayBuffer
    dev, T, OD, AD, gamma = _dev(), 5, 3, 2, 0.97
    cap = 2 * T * B + 2
    buf = PrioritizedReplayBuffer(cap, OD, AD, dev, alpha=0.7, n_step=n_step, gamma=gamma)
    twin = ReplayBuffer(cap, OD, AD, dev) if n_step == 1 else None
    ring, leaves, top = PH.new_ring(cap, OD, AD), np.zeros(cap, f32), f32(1.0)
    rng = np.random.default_rng(1000 * B + n_step)
    for i in range(3):
        b = PH.fold_case(rng, T, B, OD, AD)
        tb = _to(torch, b, dev)
        assert buf.add(tb) == T * B
        rows = PH.ring_add(ring, b, n_step, gamma)
        leaves[rows] = top
        _ring_equal(buf, ring)
        tree = _tree(buf)
        assert np.array_equal(_bits(tree[:cap]), _bits(leaves)), i
        if twin is not None:
            twin.add(tb)
            torch.cuda.synchronize()
            for k in ("obs", "actions", "reward", "next_obs", "terminated"):
                assert torch.equal(getattr(buf, k).view(torch.uint8), getattr(twin, k).view(torch.uint8)), k
            assert int(twin.head) == int(buf.head) and int(twin.fill) == int(buf.fill)
            assert bool((buf.discount[:ring["fill"]] == f32(gamma)).all())
        if i == 1:   # raise some of the rows the next add overwrites, and the running maximum with them
            some = torch.tensor([0, 1, cap - 3, cap // 2], dtype=torch.int32, device=dev)
            buf.update_priorities(some, torch.tensor([3.0, 0.5, 9.0, 2.0], device=dev))
            tree = _tree(buf)
            leaves[:] = tree[:cap]
            top = f32(tree[:cap].max())
            assert top > 1 and int(np.float32(top).view(np.uint32)) == int(buf.state[0]) & 0xFFFFFFFF
    assert ring["fill"] == cap and ring["head"] == (3 * T * B) % cap


def test_add_refuses_bad_batches_by_name():
    import torch
    from rsoccer_amd import _lib
    from rsoccer_amd.vec.replay import PrioritizedReplayBuffer
    dev = _dev()
    buf = PrioritizedReplayBuffer(16, 3, 2, dev, n_step=2)
    b = _to(torch, PH.make_batch(np.random.default_rng(0), 2, 4, 3, 2), dev)
    with pytest.raises(ValueError, match="final_obs"):
        buf.add({k: v for k, v in b.items() if k != "final_obs"})
    with pytest.raises(ValueError, match="reward"):
        buf.add({**b, "reward": b["reward"].double()})
    with pytest.raises(ValueError, match="is on cpu"):
        buf.add({**b, "obs": b["obs"].cpu()})
    with pytest.raises(ValueError, match="holds 16"):
        buf.add(_to(torch, PH.make_batch(np.random.default_rng(0), 5, 4, 3, 2), dev))
    ring = _lib.ReplayRing(*(getattr(buf, k).data_ptr() for k in RING_KEYS), buf.head.data_ptr(), buf.fill.data_ptr(),
                           buf.state.data_ptr() + 12, 16, 3, 2)
    batch = _lib.ReplayBatch(*(b[k].data_ptr() for k in ("obs", "actions", "reward", "terminated", "truncated", "final_obs", "next_obs")), 2, 4)
    for bad in (lambda: _lib.replay_add_nstep(batch, ring, 0, 0.9), lambda: _lib.replay_add_nstep(batch, ring, 17, 0.9),
                lambda: _lib.replay_add_nstep(batch, ring, 2, 1.5), lambda: _lib.replay_add_nstep(None, ring, 2, 0.9),
                lambda: _lib.replay_set_priorities(buf.tree.data_ptr(), buf.state.data_ptr(), 16, None, None, None, 4, 0.6, 1e-6),
                lambda: _lib.replay_set_priorities(buf.tree.data_ptr(), buf.state.data_ptr(), 16, None, None, buf.head.data_ptr(), 17, 0.6, 1e-6),
                lambda: _lib.replay_sample_prioritized(buf.tree.data_ptr(), buf.state.data_ptr(), 16, 0, buf.fill.data_ptr(), None, None, 4,
                                                       0.4, None, 0, 0, None)):
        with pytest.raises(_lib.RsxError):
            bad()
    torch.cuda.synchronize()
    assert int(buf.fill) == 0 and float(buf.tree.sum()) == 0.0   # nothing was enqueued


# ---- b. the tree's invariants ----
@pytest.mark.parametrize("cap", [1, 63, 64, 65, 64 * 64 + 1, 5000])
def test_every_inner_node_is_the_stated_sum_of_its_children_after_every_operation(cap):
    """fill counts below, at and wrapped past the capacity; after every add and every update_priorities the tree read back is
    recomputed from its leaves in numpy, in bits"""
    import torch
    from rsoccer_amd.vec.replay import PrioritizedReplayBuffer
    dev, OD, AD = _dev(), 2, 1
    buf = PrioritizedReplayBuffer(cap, OD, AD, dev, alpha=0.6)
    rng = np.random.default_rng(cap)
    first = max(cap // 3, 1)
    sizes = [first] + ([cap - first] if cap > first else []) + [min(cap, 5)]
    fill, head = 0, 0
    for n in sizes:
        buf.add(_to(torch, PH.make_batch(rng, 1, n, OD, AD), dev))
        tree = _tree(buf)
        fill, head = min(fill + n, cap), (head + n) % cap
        assert (int(buf.fill), int(buf.head)) == (fill, head)
        assert np.all(tree[:fill] > 0) and np.all(tree[fill:cap] == 0)
        m = min(fill, 37) + 3
        rows = rng.integers(0, fill, m).astype(np.int32)
        rows[:2] = rows[2]   # duplicates
        td = rng.uniform(0, 4, m).astype(f32)
        before = tree[:cap].copy()
        buf.update_priorities(torch.from_numpy(rows).to(dev), torch.from_numpy(td).to(dev))
        tree = _tree(buf)
        untouched = np.ones(cap, bool)
        untouched[rows] = False
        assert np.array_equal(_bits(tree[:cap][untouched]), _bits(before[untouched]))
    assert fill == cap
    _, levels, off = PH.tree_geometry(cap)
    assert tree[off[levels]] > 0


# ---- c. sample() ----
def _filled(torch, cap, fill, dev, **kw):
    from rsoccer_amd.vec.replay import PrioritizedReplayBuffer
    buf = PrioritizedReplayBuffer(cap, 2, 1, dev, **kw)
    if fill:
        buf.add(_to(torch, PH.make_batch(np.random.default_rng(fill), 1, fill, 2, 1), dev))
    return buf


def _check_sample(torch, buf, m, beta, seed, step, beta_arg=None, step_arg=None):
    rows, w = buf.sample(m, beta=beta if beta_arg is None else beta_arg, seed=seed, step=step if step_arg is None else step_arg)
    tree = _tree(buf)
    fill = int(buf.fill)
    assert rows.dtype == torch.int32 and w.dtype == torch.float32 and tuple(rows.shape) == tuple(w.shape) == (m,)
    rows, w = rows.cpu().numpy().astype(np.int64), w.cpu().numpy()
    want = PH.descend(tree, buf.capacity, fill, m, seed, step)
    assert np.array_equal(rows, want), (m, seed, step)
    ref = PH.weights64(tree, buf.capacity, fill, rows, beta)
    live = rows >= 0
    if live.any():
        _, levels, off = PH.tree_geometry(buf.capacity)
        x = (f32(fill) * tree[rows[live]]) / tree[off[levels]]
        bound, torch_worst = _pow_bound(torch, x, -beta, _dev())
        worst = _worst(w, ref)
        print(f"weights m={m} beta={beta}: worst rel err {worst:.3e}, torch.pow {torch_worst:.3e}, bound {bound:.3e}")
        assert worst <= bound
        assert np.all(tree[rows[live]] > 0) and w.max() <= 1.0
    else:
        assert np.array_equal(w, np.zeros(m, f32))
    return rows, w


@pytest.mark.parametrize("m", [1, 64, 257])
def test_sample_equals_the_descents_restatement_on_the_tree_read_back(m):
    import torch
    dev = _dev()
    rng = np.random.default_rng(m)
    buf = _filled(torch, 5000, 3000, dev, alpha=0.6)
    rows = torch.from_numpy(rng.integers(0, 3000, 900).astype(np.int32)).to(dev)
    buf.update_priorities(rows, torch.from_numpy(rng.exponential(1.0, 900).astype(f32)).to(dev))
    for seed, step, beta in ((0, 0, 0.4), (0x1234567890ABCDEF, 7, 1.0), (2 ** 64 - 1, 2 ** 40 + 5, 0.0)):
        r, w = _check_sample(torch, buf, m, beta, seed, step)
        assert r.max() < 3000
        if beta == 0.0:
            assert np.all(w == 1.0)
    # step and beta as device tensors, read when the launches run
    step_t, beta_t = torch.tensor([11], dtype=torch.int64, device=dev), torch.tensor([0.5], dtype=torch.float32, device=dev)
    a, _ = _check_sample(torch, buf, m, 0.5, 5, 11, beta_arg=beta_t, step_arg=step_t)
    step_t += 1
    beta_t.fill_(0.75)
    b, _ = _check_sample(torch, buf, m, 0.75, 5, 12, beta_arg=beta_t, step_arg=step_t)
    assert m == 1 or not np.array_equal(a, b)


def test_sample_on_hard_trees():
    """more entries than rows; one leaf 10^9 times the others; leaves that are 0 inside the filled part; an empty ring"""
    import torch
    dev = _dev()
    buf = _filled(torch, 200, 5, dev)
    r, _ = _check_sample(torch, buf, 64, 0.4, 1, 0)   # m larger than the fill count
    assert set(r.tolist()) == set(range(5))
    buf = _filled(torch, 4097, 4097, dev, alpha=1.0, eps=0.0)
    buf.update_priorities(torch.tensor([70], dtype=torch.int32, device=dev), torch.tensor([1e9], device=dev))
    r, w = _check_sample(torch, buf, 257, 0.4, 2, 3)
    assert (r == 70).sum() > 200 and np.all(buf.priorities().cpu().numpy()[r] > 0)
    zero = torch.arange(64, 3000, dtype=torch.int32, device=dev)   # whole nodes and parts of nodes become 0 (eps = 0)
    buf.update_priorities(zero, torch.zeros(zero.shape[0], device=dev))
    tree = _tree(buf)
    assert np.all(tree[64:3000] == 0) and tree[70] == 0 and tree[63] > 0
    for step in range(3):
        r, _ = _check_sample(torch, buf, 257, 0.4, 2, step)
        assert np.all((r < 64) | (r >= 3000))
    empty = _filled(torch, 130, 0, dev)
    r, w = _check_sample(torch, empty, 9, 0.4, 0, 0)
    assert np.all(r == -1) and np.all(w == 0)
    # a ring whose filled rows all hold 0
    buf = _filled(torch, 130, 100, dev, eps=0.0)
    buf.update_priorities(torch.arange(100, dtype=torch.int32, device=dev), torch.zeros(100, device=dev))
    r, w = _check_sample(torch, buf, 9, 0.4, 0, 0)
    assert np.all(r == -1) and np.all(w == 0)


# ---- d. update_priorities() ----
def test_update_priorities_duplicates_skipped_indices_and_the_running_maximum():
    import torch
    dev = _dev()
    cap, alpha, eps = 300, 0.6, 1e-6
    buf = _filled(torch, cap, 300, dev, alpha=alpha, eps=eps)
    rng = np.random.default_rng(8)
    rows = rng.integers(0, cap, 500).astype(np.int32)
    rows[10:20] = 7                                 # a row that occurs ten times
    rows[20:24] = (-1, cap, 2 ** 31 - 1, -2 ** 31)  # skipped
    td = (rng.standard_normal(500) * np.exp(rng.uniform(-12, 6, 500))).astype(f32)
    td[30] = 0.0
    before = _tree(buf)[:cap].copy()
    guard = torch.full((4,), 5.0, device=dev)
    buf.update_priorities(torch.from_numpy(rows).to(dev), torch.from_numpy(td).to(dev))
    tree = _tree(buf)
    assert int(buf.skipped()) == 4 and bool((guard == 5.0).all())
    ok = (rows >= 0) & (rows < cap)
    ref = np.zeros(cap, np.float64)
    np.maximum.at(ref, rows[ok].astype(np.int64), PH.leaf_value64(td[ok], alpha, eps))
    touched = np.zeros(cap, bool)
    touched[rows[ok]] = True
    assert np.array_equal(_bits(tree[:cap][~touched]), _bits(before[~touched]))   # skipped indices change nothing
    base = (np.abs(td[ok]) + f32(eps)).astype(f32)
    bound, torch_worst = _pow_bound(torch, base, alpha, dev)
    worst = _worst(tree[:cap][touched], ref[touched])
    print(f"leaves: worst rel err {worst:.3e}, torch.pow {torch_worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
    # the order of the entries does not matter: the largest value wins
    perm = rng.permutation(500)
    twin = _filled(torch, cap, 300, dev, alpha=alpha, eps=eps)
    twin.update_priorities(torch.from_numpy(rows[perm]).to(dev), torch.from_numpy(td[perm]).to(dev))
    assert np.array_equal(_bits(_tree(twin)), _bits(tree))
    # the running maximum grew to the largest leaf written, and a smaller update does not shrink it
    top = float(buf.max_priority())
    assert top == float(tree[:cap].max()) > 1.0
    buf.update_priorities(torch.arange(cap, dtype=torch.int32, device=dev), torch.full((cap,), 1e-3, device=dev))
    assert float(buf.max_priority()) == top and float(_tree(buf)[:cap].max()) < 1.0
    buf.add(_to(torch, PH.make_batch(rng, 1, 3, 2, 1), dev))   # new rows carry it
    assert np.array_equal(_tree(buf)[:3], np.full(3, top, f32))
    with pytest.raises(ValueError, match="rows must be"):
        buf.update_priorities(torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(3, device=dev))
    with pytest.raises(ValueError, match="one shape"):
        buf.update_priorities(torch.zeros(3, dtype=torch.int32, device=dev), torch.zeros(4, device=dev))


# ---- e. capture ----
def test_a_captured_per_iteration_replays_as_eager_iterations_bit_for_bit():
    """collect + add + sample + dpg_gradient(weights=, return_td_error=True) + opt.step + update_priorities captured once and replayed
    three times against four eager iterations of a twin: the ring, the tree and the parameters in bits"""
    import torch
    from rsoccer_amd import vec
    from rsoccer_amd.vec.optim import DPGOptimizer
    from rsoccer_amd.vec.policy import MLPPolicy, MLPQCritic
    from rsoccer_amd.vec.replay import PrioritizedReplayBuffer
    import dpg_helpers as DH
    T, B, BATCH = 4, 16, 32
    envs = [vec.VecVSSEnv(B, device=0, seed=17, max_episode_steps=10) for _ in range(2)]
    for e in envs:
        e.reset()
        e.enable_graph_capture()
    env, twin = envs
    dev = env.device
    pol = MLPPolicy(40, 2, hidden=64, layers=2, hidden_act="tanh", out_act="tanh")
    crit = MLPQCritic(40, 2, hidden=64, layers=2, hidden_act="tanh")
    gen = torch.Generator().manual_seed(51)
    p0 = DH.init(torch, pol, gen)
    c0 = torch.stack([DH.init(torch, crit, gen) for _ in range(2)])
    start = [x.float().contiguous().to(dev) for x in (p0 + 0.02 * torch.randn(pol.num_params, generator=gen), p0,
                                                      c0 + 0.02 * torch.randn(2, crit.num_params, generator=gen), c0)]
    log_std = torch.full((2,), -1.0, device=dev)
    sides = [([x.clone() for x in start], DPGOptimizer(pol, crit, 2, device=dev, lr_actor=1e-3, lr_critic=1e-3, max_grad_norm=0.5, tau=0.05),
              PrioritizedReplayBuffer(160, 40, 2, dev, alpha=0.6, n_step=3, gamma=0.97), torch.tensor([0.4], device=dev)) for _ in envs]

    def iteration(e, P, opt, buf, beta):
        batch = e.collect(pol, P[0], T, log_std=log_std, noise_seed=99, return_final_obs=True)
        buf.add(batch)
        rows, w = buf.sample(BATCH, beta=beta, seed=123, step=opt.steps)
        g = e.dpg_gradient(buf.data(), pol, P[0], P[1], crit, P[2], P[3], rows=rows, gamma=0.97, target_noise=0.2, noise_clip=0.1,
                           noise_seed=5, noise_step=opt.steps, weights=w, return_td_error=True)
        opt.step(P[0], P[1], P[2], P[3], g["grad_params"], g["grad_critic_params"])
        buf.update_priorities(rows, g["td_error"])
        beta.add_(0.1)
        return rows, w, g["td_error"]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # one eager iteration, which is also torch's warm-up before a capture
        first = iteration(env, *sides[0])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    seen = [[x.clone() for x in first]]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = iteration(env, *sides[0])
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        seen.append([x.clone() for x in out])
    for i in range(4):
        want = iteration(twin, *sides[1])
        torch.cuda.synchronize()
        for name, a, b in zip(("rows", "weights", "td_error"), seen[i], want):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, i)
        assert bool((seen[i][0] >= 0).all()) and float(seen[i][2].max()) > 0
    (Pa, oa, ba, _), (Pb, ob, bb, _) = sides
    for a, b in zip(list(Pa) + oa.m + oa.v, list(Pb) + ob.m + ob.v):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert oa.counters.tolist() == ob.counters.tolist()
    for k in RING_KEYS:
        assert torch.equal(getattr(ba, k).view(torch.uint8), getattr(bb, k).view(torch.uint8)), k
    assert torch.equal(ba.tree.view(torch.int32), bb.tree.view(torch.int32)) and torch.equal(ba.state, bb.state)
    assert int(ba.head) == int(bb.head) == (4 * T * B) % 160 and int(ba.fill) == int(bb.fill) == 160
    PH.check_tree(ba.tree.cpu().numpy(), 160)
    assert np.array_equal(env.checkpoint(), twin.checkpoint())
    for e in envs:
        e.close()
