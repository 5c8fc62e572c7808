"""rsx_task_transfer / VecFusedEnv.copy_envs_from against the checkpoint path that already exists and is verified against the oracle:
the destination's checkpoint after a transfer equals, byte for byte, the blob tests/transfer_helpers.py assembles in numpy from the
two checkpoints taken before it, and a twin handle that restored that blob steps on exactly like the destination.  Every comparison
is on bit patterns; nothing here has a tolerance."""
import numpy as np
import pytest

from transfer_helpers import blob_layout, expected_blob, section

pytestmark = pytest.mark.gpu

# name: (task, kind, field_type, n_blue, n_yellow)
CONFIGS = {
    "VSS-v0": (1, 0, 0, 3, 3),
    "SSLStaticDefenders": (2, 1, 2, 1, 6),
    "SSLDribbling": (3, 1, 2, 1, 4),
    "SSLContestedPossession": (4, 1, 2, 1, 1),
    "SSLPassEndurance": (5, 1, 2, 2, 0),
    "scrimmage11v11": (6, 1, 1, 11, 11),
}
SRC_B, DST_B, MAX_STEPS = 37, 21, 40
SRC_SEED, DST_SEED, SRC_BASE, DST_BASE = 4242, 977, 31, 1000


def _L():
    from rsoccer_amd import _lib
    return _lib


def _make(name, B, seed, base, monkeypatch=None, layout=None, pad=None, max_steps=MAX_STEPS, phys=False, reset=True):
    L = _L()
    task, kind, ft, nb, ny = CONFIGS[name]
    if monkeypatch is not None:
        for var, val in (("RSX_LAYOUT", layout), ("RSX_ROW_PAD", pad)):
            if val is None:
                monkeypatch.delenv(var, raising=False)
            else:
                monkeypatch.setenv(var, str(val))
    sim = L.Sim(kind, ft, nb, ny, 25, B)
    if phys:
        sim.physics_enable()
    sim.task_attach(task, seed, base, max_steps)
    if reset:
        sim.task_reset()
    return sim


def _fed(torch, sim, steps, seed):
    """`steps` fed steps with actions drawn on the host (the same for every handle of that shape)"""
    acts = np.random.default_rng(seed).uniform(-1.0, 1.0, (steps, sim.num_envs, sim.act_dim)).astype(np.float32)
    dev = torch.from_numpy(acts).cuda()
    for t in range(steps):
        sim.task_step(dev[t].data_ptr())
    torch.cuda.synchronize()


def _warm_src(torch, sim):
    """~50 mixed steps with a 40-step TimeLimit: some envs have just been auto-reset; the last launch is a single-step one"""
    sim.task_step_n(20)
    sim.task_rollout(15)
    _fed(torch, sim, 14, 5)
    sim.task_step(None)
    torch.cuda.synchronize()


def _snapshot(torch, sim):
    torch.cuda.synchronize()
    t = sim.task_tensors()
    parts = [sim.get_state_full().astype(np.float32).view(np.uint32).ravel()]
    for k in ("obs", "reward", "info", "final_obs"):
        parts.append(np.ascontiguousarray(t[k].cpu().numpy()).view(np.uint32).ravel())
    for k in ("terminated", "truncated", "steps"):
        parts.append(t[k].cpu().numpy().astype(np.uint32).ravel())
    parts.append(sim.read_metrics().astype(np.uint64).view(np.uint32))
    return np.concatenate(parts)


def _pairs(n=13, seed=3, src_B=SRC_B, dst_B=DST_B):
    """n pairs in scrambled order, one source used twice"""
    rng = np.random.default_rng(seed)
    d = rng.permutation(dst_B)[:n].astype(np.int32)
    s = rng.permutation(src_B)[:n].astype(np.int32)
    s[5] = s[2]
    return d, s


def _transfer(torch, dst, src, d, s, n=None):
    dd = None if d is None else torch.from_numpy(np.asarray(d, dtype=np.int32)).cuda()
    sd = None if s is None else torch.from_numpy(np.asarray(s, dtype=np.int32)).cuda()
    if n is None:
        n = len(d) if d is not None else len(s)
    dst.task_transfer(src, None if dd is None else dd.data_ptr(), None if sd is None else sd.data_ptr(), n)
    torch.cuda.synchronize()


def _first_diff(a, b, lay):
    for name in lay:
        x, y = section(a, lay, name), section(b, lay, name)
        if not np.array_equal(x, y):
            bad = np.argwhere(x != y)
            return f"section {name}: {len(bad)} words differ, first at {bad[0].tolist()}"
    return "header differs" if not np.array_equal(a[:176], b[:176]) else "physics header differs"


def _check_transfer(torch, name, src, dst, make_twin, steps_after=30):
    """(a) blob equality, (b) step-on equality with a twin that restored the expected blob, (c) source unchanged, (d) the
    destination's step counter and metrics unchanged"""
    d, s = _pairs()
    src_blob, dst_blob = src.task_checkpoint(), dst.task_checkpoint()
    tick, metrics = dst.task_tick(), dst.read_metrics()
    want = expected_blob(dst_blob, src_blob, d, s)
    assert not np.array_equal(want, dst_blob)
    _transfer(torch, dst, src, d, s)
    assert dst.task_transfer_errors() == 0
    got = dst.task_checkpoint()
    lay, _ = blob_layout(got)
    assert np.array_equal(got, want), f"{name} (a): {_first_diff(got, want, lay)}"
    assert np.array_equal(src.task_checkpoint(), src_blob), f"{name} (c): the source changed"
    assert dst.task_tick() == tick and np.array_equal(dst.read_metrics(), metrics), f"{name} (d)"
    twin = make_twin()
    twin.task_restore(want)
    _fed(torch, dst, steps_after, 11)
    _fed(torch, twin, steps_after, 11)
    a, b = _snapshot(torch, dst), _snapshot(torch, twin)
    assert np.array_equal(a, b), f"{name} (b): {int((a != b).sum())} of {a.size} words differ after {steps_after} more steps"
    twin.close()


# ---- 1. every fused task ----
@pytest.mark.parametrize("name", list(CONFIGS))
def test_transfer_equals_the_blob_and_steps_on_like_a_restored_twin(name):
    import torch
    src = _make(name, SRC_B, SRC_SEED, SRC_BASE)
    _warm_src(torch, src)
    dst = _make(name, DST_B, DST_SEED, DST_BASE)
    dst.task_step_n(23)
    _check_transfer(torch, name, src, dst, lambda: _make(name, DST_B, DST_SEED, DST_BASE, reset=False))
    src.close(); dst.close()


# ---- 2. kernel layouts and row padding ----
@pytest.mark.parametrize("name,src_layout,dst_layout,pad_side", [
    ("VSS-v0", "epl", "lanes", "src"), ("VSS-v0", "lanes", "epl", "dst"),
    ("SSLStaticDefenders", "epl", "lanes", "dst"), ("SSLStaticDefenders", "lanes", "epl", "src"),
    ("scrimmage11v11", "quad", "lanes", "src"), ("scrimmage11v11", "lanes", "quad", "dst"),
])
def test_transfer_across_kernel_layouts_and_row_strides(monkeypatch, name, src_layout, dst_layout, pad_side):
    """the source stepped by one kernel layout, the destination by another, rows padded on one side only: the step-on comparison is
    the one that sees a row a layout leaves stale in memory (the checkpoint patches VSS-v0's previous potential, the kernels of the
    destination read what the transfer wrote)"""
    import torch
    names = {"epl": "one-lane-per-env", "quad": "four-lanes-per-env"}
    src = _make(name, SRC_B, SRC_SEED, SRC_BASE, monkeypatch, src_layout, 64 if pad_side == "src" else 0)
    dst = _make(name, DST_B, DST_SEED, DST_BASE, monkeypatch, dst_layout, 64 if pad_side == "dst" else 0)
    for sim, lay in ((src, src_layout), (dst, dst_layout)):
        assert (sim.task_layout() == names[lay]) if lay in names else sim.task_layout().endswith("-lanes-per-env"), sim.task_layout()
    assert (src._view.row_stride != SRC_B) == (pad_side == "src") and (dst._view.row_stride != DST_B) == (pad_side == "dst")
    _warm_src(torch, src)   # (ends with a single-step launch)
    dst.task_step_n(23)
    _check_transfer(torch, f"{name} {src_layout}->{dst_layout}", src, dst,
                    lambda: _make(name, DST_B, DST_SEED, DST_BASE, monkeypatch, dst_layout, 64 if pad_side == "dst" else 0, reset=False))
    src.close(); dst.close()


# ---- 3. per-env physics ----
@pytest.mark.parametrize("name", ["VSS-v0", "SSLStaticDefenders"])
def test_transfer_carries_per_env_physics(name):
    import torch
    L = _L()
    P = len(L.PHYSICS_PARAMS)
    i_mb, i_mu = L.PHYSICS_PARAMS.index("m_ball"), L.PHYSICS_PARAMS.index("mu_g")

    def make(B, seed, base, scale, reset=True):
        sim = _make(name, B, seed, base, phys=True, reset=False)
        vals = np.full((P, B), np.nan, dtype=np.float32)
        vals[i_mb] = 0.046 * (1.0 + scale * np.arange(B) / B)
        vals[i_mu] = 0.3 + scale * np.arange(B) / B
        sim.physics_set(vals)
        lo, hi = np.zeros(P, np.float32), np.zeros(P, np.float32)
        lo[i_mb], hi[i_mb] = 0.04 + 0.01 * scale, 0.05 + 0.01 * scale
        sim.physics_randomize(lo, hi, 1 << i_mb)
        if reset:
            sim.task_reset()
        return sim

    src, dst = make(SRC_B, SRC_SEED, SRC_BASE, 0.2), make(DST_B, DST_SEED, DST_BASE, 0.5)
    _warm_src(torch, src)
    dst.task_step_n(23)
    d, s = _pairs()
    raw_s, coef_s = src.physics_get(L.PHYS_RAW), src.physics_get(L.PHYS_COEF)
    raw_d = dst.physics_get(L.PHYS_RAW)
    assert not np.array_equal(raw_d[:, d], raw_s[:, s])
    # (a) - (d); the 30 steps behind the transfer cross the 40-step TimeLimit: episode ends redraw m_ball under dst's ranges
    _check_transfer(torch, name + " physics", src, dst, lambda: make(DST_B, DST_SEED, DST_BASE, 0.5, reset=False))
    src.close(); dst.close()
    # the rows themselves, right after a transfer
    src, dst = make(SRC_B, SRC_SEED, SRC_BASE, 0.2), make(DST_B, DST_SEED, DST_BASE, 0.5)
    raw_s, coef_s, raw_d = src.physics_get(L.PHYS_RAW), src.physics_get(L.PHYS_COEF), dst.physics_get(L.PHYS_RAW)
    _transfer(torch, dst, src, d, s)
    got_raw, got_coef = dst.physics_get(L.PHYS_RAW), dst.physics_get(L.PHYS_COEF)
    assert np.array_equal(got_raw[:, d].view(np.uint32), raw_s[:, s].view(np.uint32))
    assert np.array_equal(got_coef[:, d].view(np.uint32), coef_s[:, s].view(np.uint32))
    rest = np.setdiff1d(np.arange(DST_B), d)
    assert np.array_equal(got_raw[:, rest].view(np.uint32), raw_d[:, rest].view(np.uint32))
    # physics on one side only
    plain = _make(name, DST_B, DST_SEED, DST_BASE)
    blob = plain.task_checkpoint()
    with pytest.raises(L.RsxError, match="one handle only"):
        plain.task_transfer(src, None, None, 5)
    with pytest.raises(L.RsxError, match="one handle only"):
        dst.task_transfer(plain, None, None, 5)
    assert np.array_equal(plain.task_checkpoint(), blob)
    for sim in (src, dst, plain):
        sim.close()


# ---- 4. same handle ----
@pytest.mark.parametrize("name", ["VSS-v0", "SSLStaticDefenders"])
def test_same_handle_maps_read_everything_before_they_write(name):
    import torch
    B = SRC_B
    sim = _make(name, B, SRC_SEED, SRC_BASE)
    _warm_src(torch, sim)
    rng = np.random.default_rng(8)
    maps = [
        ("identity", None, None, B),
        ("reversal", None, np.arange(B)[::-1].copy(), B),
        ("swap", np.array([3, 17]), np.array([17, 3]), 2),
        ("resample", None, rng.integers(0, B, B), B),                       # multinomial, with duplicates
        ("partial", rng.permutation(B)[:9], rng.integers(0, B, 9), 9),
    ]
    for tag, d, s, n in maps:
        before = sim.task_checkpoint()
        want = expected_blob(before, before, d if d is not None else np.arange(n), s if s is not None else np.arange(n))
        _transfer(torch, sim, sim, d, s, n)
        got = sim.task_checkpoint()
        lay, _ = blob_layout(got)
        assert np.array_equal(got, want), f"{tag}: {_first_diff(got, want, lay)}"   # (envs outside dst_ids included)
        if tag == "identity":
            assert np.array_equal(got, before)
        else:
            assert not np.array_equal(got, before), tag
        sim.task_step_n(3)   # the handle steps on
    assert sim.task_transfer_errors() == 0
    sim.close()


# ---- 5. refusals and skipped pairs ----
def test_out_of_range_pairs_are_skipped_and_counted():
    import torch
    name = "SSLStaticDefenders"
    src = _make(name, SRC_B, SRC_SEED, SRC_BASE)
    _warm_src(torch, src)
    dst = _make(name, DST_B, DST_SEED, DST_BASE)
    dst.task_step_n(23)
    d = np.array([4, -1, 7, DST_B, 0, 9, 20], dtype=np.int32)
    s = np.array([36, 3, SRC_B, 5, 11, -7, 0], dtype=np.int32)       # pairs 1, 2, 3, 5 are bad; their neighbours are good
    want = expected_blob(dst.task_checkpoint(), src.task_checkpoint(), d, s)
    _transfer(torch, dst, src, d, s)
    assert dst.task_transfer_errors() == 4
    assert dst.task_transfer_errors() == 0                              # read and cleared
    assert np.array_equal(dst.task_checkpoint(), want)
    # the same on one handle (gather + scatter: counted once)
    before = src.task_checkpoint()
    d = np.array([4, SRC_B, 7, 1], dtype=np.int32)
    s = np.array([7, 3, 4, -1], dtype=np.int32)
    want = expected_blob(before, before, d, s)
    _transfer(torch, src, src, d, s)
    assert src.task_transfer_errors() == 2
    assert np.array_equal(src.task_checkpoint(), want)
    src.close(); dst.close()


def test_mismatched_or_unready_handles_are_refused(monkeypatch):
    import torch
    L = _L()
    dst = _make("SSLStaticDefenders", DST_B, DST_SEED, DST_BASE)
    dst.task_step_n(5)
    torch.cuda.synchronize()
    blob = dst.task_checkpoint()
    ok = _make("SSLStaticDefenders", SRC_B, SRC_SEED, SRC_BASE)

    def refused(src, match, n=3):
        with pytest.raises(L.RsxError, match=match):
            dst.task_transfer(src, None, None, n)
        torch.cuda.synchronize()
        assert np.array_equal(dst.task_checkpoint(), blob), match

    other_task = _make("SSLContestedPossession", SRC_B, 1, 0)
    refused(other_task, "kind, task or team sizes")
    five = L.Sim(1, 2, 1, 5, 25, SRC_B)                                 # static defenders 1v5
    five.task_attach(2, 1, 0, MAX_STEPS); five.task_reset()
    refused(five, "kind, task or team sizes")
    refused(_make("SSLStaticDefenders", SRC_B, 1, 0, max_steps=41), "max_episode_steps")
    refused(_make("SSLStaticDefenders", SRC_B, 1, 0, reset=False), "must come before rsx_task_transfer")
    raw = L.Sim(1, 2, 1, 6, 25, SRC_B)
    refused(raw, "no task attached")
    refused(ok, "n must be >= 0", n=-1)
    refused(ok, "exceeds num_envs", n=DST_B + 1)                        # identity map on both sides: the smaller handle bounds n
    # a never-reset destination
    fresh = _make("SSLStaticDefenders", DST_B, DST_SEED, DST_BASE, reset=False)
    with pytest.raises(L.RsxError, match="must come before rsx_task_transfer"):
        fresh.task_transfer(ok, None, None, 3)
    # n == 0 is a no-op
    dst.task_transfer(ok, None, None, 0)
    torch.cuda.synchronize()
    assert np.array_equal(dst.task_checkpoint(), blob)
    # scrimmage and its crowded line-up are different tasks
    a = L.Sim(1, 1, 2, 2, 25, 8); a.task_attach(6, 1, 0, 40); a.task_reset()
    b = L.Sim(1, 1, 2, 2, 25, 8); b.task_attach(7, 1, 0, 40); b.task_reset()
    with pytest.raises(L.RsxError, match="kind, task or team sizes"):
        a.task_transfer(b, None, None, 8)


# ---- 6. stream capture ----
def test_captured_transfer_and_step_replays_like_the_eager_calls():
    import torch
    from rsoccer_amd import _lib, vec

    def pair():
        src = vec.VecVSSEnv(SRC_B, device=0, seed=SRC_SEED, env_id_base=SRC_BASE, max_episode_steps=MAX_STEPS)
        dst = vec.VecVSSEnv(DST_B, device=0, seed=DST_SEED, env_id_base=DST_BASE, max_episode_steps=MAX_STEPS)
        src.reset(); dst.reset()
        src.step_random(30); dst.step_random(7)
        src.enable_graph_capture(); dst.enable_graph_capture()
        torch.cuda.synchronize()
        return src, dst

    d, s = _pairs()
    d_dev, s_dev = torch.from_numpy(d).cuda(), torch.from_numpy(s).cuda()
    acts = torch.from_numpy(np.random.default_rng(2).uniform(-1, 1, (DST_B, 2)).astype(np.float32)).cuda()
    src, dst = pair()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dst.copy_envs_from(src, src_ids=s_dev, dst_ids=d_dev)
        dst.step(acts)
    assert dst.sim.task_tick() == 7                                     # capturing enqueued nothing
    g.replay(); g.replay()
    torch.cuda.synchronize()
    src2, dst2 = pair()
    for _ in range(2):
        dst2.copy_envs_from(src2, src_ids=s_dev, dst_ids=d_dev)
        dst2.step(acts)
    torch.cuda.synchronize()
    assert dst.sim.task_tick() == dst2.sim.task_tick() == 9
    assert np.array_equal(dst.checkpoint(), dst2.checkpoint())
    assert np.array_equal(src.checkpoint(), src2.checkpoint())

    # same handle: refused in a capture while its staging buffer would have to grow, accepted after one eager call of that size
    perm = torch.from_numpy(np.random.default_rng(4).permutation(DST_B).astype(np.int32)).cuda()
    side = torch.cuda.Stream()
    with pytest.raises(_lib.RsxError, match="one eager call"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
            dst.copy_envs_from(dst, src_ids=perm)
    _lib.drop_pending_hip_error()
    torch.cuda.synchronize()
    assert np.array_equal(dst.checkpoint(), dst2.checkpoint())          # nothing ran
    dst.copy_envs_from(dst, src_ids=perm); dst2.copy_envs_from(dst2, src_ids=perm)      # the eager call of that size
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        dst.copy_envs_from(dst, src_ids=perm)
        dst.step(acts)
    g2.replay()
    dst2.copy_envs_from(dst2, src_ids=perm); dst2.step(acts)
    torch.cuda.synchronize()
    assert np.array_equal(dst.checkpoint(), dst2.checkpoint())
    for e in (src, dst, src2, dst2):
        e.close()


# ---- 7. composition with lookahead ----
def test_broadcast_then_lookahead_returns_the_source_row_for_every_env():
    """SSLStaticDefenders: with fed actions nothing in an episode depends on the env id — the defenders stand still (no OU noise),
    the only per-step draw (rsx_task.hpp: draw_for_step) is the random action that a candidate's action replaces, and a pair stops
    at its episode end, before any placement — so every env that holds env j's episode scores the candidates as env j did."""
    import torch
    from rsoccer_amd import vec
    B, K, H, j = 37, 6, 10, 11
    env = vec.VecSSLStaticDefendersEnv(B, device=0, seed=5, max_episode_steps=MAX_STEPS)
    env.reset()
    env.step_random(17)
    cand = np.random.default_rng(6).uniform(-1, 1, (1, K, H, env.sim.act_dim)).astype(np.float32)
    acts = torch.from_numpy(np.repeat(cand, B, axis=0)).cuda()
    first = {k: v.cpu().numpy() for k, v in env.lookahead(acts, gamma=0.97, return_obs=True).items()}
    assert len({first["return"][e].tobytes() for e in range(B)}) > 1    # the envs did differ
    env.copy_envs_from(env, src_ids=np.full(B, j))
    torch.cuda.synchronize()
    second = {k: v.cpu().numpy() for k, v in env.lookahead(acts, gamma=0.97, return_obs=True).items()}
    for k, v in second.items():
        want = np.repeat(first[k][j:j + 1], B, axis=0)
        assert v.dtype == want.dtype and np.array_equal(v.view(np.uint8), want.view(np.uint8)), k
    env.close()


# ---- 8. Python surface ----
def _classes(vec):
    return [(vec.VecVSSEnv, {}), (vec.VecSSLStaticDefendersEnv, {}), (vec.VecSSLDribblingEnv, {}), (vec.VecSSLContestedPossessionEnv, {}),
            (vec.VecSSLPassEnduranceEnv, {}), (vec.VecSSLScrimmageEnv, dict(n_blue=5, n_yellow=7, field_type=0, crowded=True))]


def test_fork_returns_a_ready_sibling_of_every_env_class():
    import torch
    from rsoccer_amd import vec
    for cls, kw in _classes(vec):
        env = cls(16, device=0, seed=9, env_id_base=3, max_episode_steps=33, **kw)
        env.reset(); env.step_random(5)
        bank = env.fork(num_envs=8, seed=12)
        assert type(bank) is type(env) and bank.num_envs == 8 and bank.device == env.device
        assert bank.max_episode_steps == 33 and bank.sim.task == env.sim.task
        assert (bank.sim.n_blue, bank.sim.n_yellow, bank.sim.field_type) == (env.sim.n_blue, env.sim.n_yellow, env.sim.field_type)
        assert bank._physics == env._physics
        obs = bank.copy_envs_from(env, src_ids=[2, 9, 2], dst_ids=[7, 0, 4])       # already reset: ready to receive
        torch.cuda.synchronize()
        assert obs is bank._t["obs"]
        assert torch.equal(obs[[7, 0, 4]], env._t["obs"][[2, 9, 2]])
        assert torch.equal(bank.state[:, [7, 0, 4]], env.state[:, [2, 9, 2]])
        same = env.fork()
        assert same.num_envs == 16
        same.copy_envs_from(env)
        torch.cuda.synchronize()
        assert torch.equal(same.state, env.state) and torch.equal(same._t["steps"], env._t["steps"])
        for e in (env, bank, same):
            e.close()
    # per-env physics: on in the fork, with the parent's ranges
    env = vec.VecVSSEnv(16, device=0, seed=9, physics={"m_ball": 0.05}, physics_ranges={"mu_g": (0.2, 0.4)})
    env.reset()
    bank = env.fork(num_envs=4)
    assert bank._physics and bank._ranges == {"mu_g": (0.2, 0.4)}
    bank.copy_envs_from(env, src_ids=[5], dst_ids=[1])
    torch.cuda.synchronize()
    assert float(bank.physics()["m_ball"][1]) == float(np.float32(0.05))
    env.close(); bank.close()


def test_copy_envs_from_takes_tensors_arrays_lists_and_masks():
    import torch
    from rsoccer_amd import vec
    env = vec.VecSSLContestedPossessionEnv(SRC_B, device=0, seed=1, max_episode_steps=MAX_STEPS)
    env.reset(); env.step_random(25)
    bank = env.fork(num_envs=DST_B, seed=2)
    base = bank.checkpoint()
    src_blob = env.checkpoint()
    d, s = _pairs()
    want = expected_blob(base, src_blob, d, s)
    mask = np.zeros(DST_B, bool); mask[d] = True
    want_mask = expected_blob(base, src_blob, np.nonzero(mask)[0], s)
    forms = [
        (torch.from_numpy(s).cuda(), torch.from_numpy(d).cuda(), want),
        (torch.from_numpy(s.astype(np.int64)).cuda(), torch.from_numpy(d.astype(np.int64)).cuda(), want),
        (s, d, want), (s.astype(np.int64), d.tolist(), want), (s.tolist(), torch.from_numpy(d), want),
        (s, mask, want_mask), (s.tolist(), torch.from_numpy(mask).cuda(), want_mask),
    ]
    for i, (si, di, w) in enumerate(forms):
        bank.restore(base)
        bank.copy_envs_from(env, src_ids=si, dst_ids=di)
        torch.cuda.synchronize()
        assert np.array_equal(bank.checkpoint(), w), i
    bank.restore(base)
    with pytest.raises(ValueError, match="twice"):
        bank.copy_envs_from(env, src_ids=[1, 2, 3], dst_ids=[4, 5, 4])
    with pytest.raises(ValueError, match="outside"):
        bank.copy_envs_from(env, src_ids=[1, 2], dst_ids=[4, DST_B])
    with pytest.raises(ValueError, match="outside"):
        bank.copy_envs_from(env, src_ids=[1, SRC_B], dst_ids=[4, 5])
    with pytest.raises(ValueError, match="differ in length"):
        bank.copy_envs_from(env, src_ids=[1, 2, 3], dst_ids=[4, 5])
    with pytest.raises(ValueError, match="different num_envs"):
        bank.copy_envs_from(env)
    torch.cuda.synchronize()
    assert np.array_equal(bank.checkpoint(), base)
    env.close(); bank.close()
