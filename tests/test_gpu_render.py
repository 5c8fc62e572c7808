"""env.render() of the batched envs (rsx_render, rsoccer_amd/csrc/rsx_render.hip) against rsoccer_amd/Render/raster.py drawn on a
padded canvas and fed the env's own float32 state (tests/render_helpers.py, which also states the condition frames must meet)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from render_helpers import compare_frames, reference_frames  # noqa: E402

pytestmark = pytest.mark.gpu


def _state(env):
    return env.state.cpu().numpy()


# the division-A field (include/rsx.h: field_type 1 of the SSL class) in the window of Render.view_for_field, written out by hand: the
# expected view does not come from the code under test
DIV_A_VIEW = dict(length=12.0, width=9.0, margin=0.35, circle=1.0, pen_len=1.8, pen_wid=3.6, goal_wid=1.8, goal_dep=0.18,
                  scale=40, robot=0.09, ball=0.0215, square=False)


def _check_env(env, vss, tag, want_view, **kw):
    """``want_view``: the view the frames must show, as the test states it"""
    got = env.render(**kw).cpu().numpy()
    from rsoccer_amd.Render import FieldRaster
    w, h = FieldRaster(want_view).window_size
    assert got.shape[1:3] == (h, w) == env.render_shape(**kw)
    ref = reference_frames(want_view, _state(env), env.sim.n_blue, env.sim.n_yellow, vss)
    return compare_frames(got, ref, tag)


@pytest.mark.parametrize("config", ["vss-500", "vss-100", "vss-64", "ssl-100", "ssl-20", "scrimmage-field-40"])
def test_frames_equal_the_rasterisers_after_a_rollout(config):
    from rsoccer_amd.vec import VecSSLScrimmageEnv, VecSSLStaticDefendersEnv, VecVSSEnv
    kind, *rest = config.split("-")
    if kind == "vss":
        env, kw = VecVSSEnv(64, seed=11), dict(scale=float(rest[0]))
    elif kind == "ssl":
        env, kw = VecSSLStaticDefendersEnv(64, seed=12), dict(scale=float(rest[0]))
    else:
        env, kw = VecSSLScrimmageEnv(32, n_blue=11, n_yellow=11, seed=13), dict(view="field", scale=40)
    from rsoccer_amd.Render import SSL_VIEW, VSS_VIEW, view_for_field
    if kind == "scrimmage":
        view = DIV_A_VIEW
        assert view_for_field(env.sim.kind, env.sim.get_field_params(), scale=40) == view    # the handle's own field table
        assert env.render_shape() == (int(9.0 * 100 + 70), int(12.0 * 100 + 70))             # its default view is "field", not the 9 x 6 m window
    else:
        view = dict(VSS_VIEW if kind == "vss" else SSL_VIEW, scale=kw["scale"])
    env.reset()
    env.step_random(50)
    _check_env(env, kind == "vss", config, view, **kw)
    assert env.sim.render_errors() == 0
    env.close()


def _edge_placements(B, rng, half_x, half_y, r, nb, ny):
    """every body of env e straddles, touches or lies beyond one border of the window (half_x x half_y metres around the origin)"""
    offs = np.array([-r, -0.5 * r, 0.0, 0.5 * r, r, 3.0 * r])
    ball = np.zeros((B, 4)); blue = np.zeros((B, nb, 3)); yellow = np.zeros((B, ny, 3))
    for e in range(B):
        for k in range(nb + ny + 1):
            side = (e + k) % 4
            off = offs[(e // 4 + k) % len(offs)]
            along = rng.uniform(-1.0, 1.0)
            if side < 2:
                x, y = (half_x + off) * (1 if side == 0 else -1), along * half_y
            else:
                x, y = along * half_x, (half_y + off) * (1 if side == 2 else -1)
            if k == nb + ny:
                ball[e, :2] = x, y
            else:
                (blue[e, k] if k < nb else yellow[e, k - nb])[:] = x, y, rng.uniform(-180.0, 180.0)
    return ball, blue, yellow


def test_window_edges_and_guard_bytes():
    """bodies straddling every border of the window and beyond it; the frames are written into the middle of a larger buffer whose
    size is not a multiple of 16, and nothing around them is touched"""
    import torch
    from rsoccer_amd.Render import VSS_VIEW
    from rsoccer_amd.vec import VecVSSEnv
    B = 21
    env = VecVSSEnv(B, seed=3)
    env.reset()
    rng = np.random.default_rng(5)
    # the reference window: 1.5 x 1.3 m field + 0.1 m margin
    env.reset_to(*_edge_placements(B, rng, 0.85, 0.75, 0.04, 3, 3))
    guard = 4096
    for scale, ids in ((100.0, None), (500.0, [20, 1, 7, 12, 18])):
        H, W = env.render_shape(scale=scale)
        n = B if ids is None else len(ids)
        nbytes = n * H * W * 3
        assert nbytes % 16 != 0
        big = torch.full((guard + nbytes + guard,), 0xA5, dtype=torch.uint8, device=env.device)
        out = big[guard:guard + nbytes].view(n, H, W, 3)
        assert env.render(ids, scale=scale, out=out) is out
        ref = reference_frames(dict(VSS_VIEW, scale=scale), _state(env), 3, 3, True, ids)
        compare_frames(out.cpu().numpy(), ref, f"edges-{scale}")
        assert bool((big[:guard] == 0xA5).all()) and bool((big[guard + nbytes:] == 0xA5).all())
        # the same through the channels-first layout
        big.fill_(0xA5)
        out = big[guard:guard + nbytes].view(n, 3, H, W)
        env.render(ids, scale=scale, out=out, channels_first=True)
        compare_frames(out.permute(0, 2, 3, 1).cpu().numpy(), ref, f"edges-chw-{scale}")
        assert bool((big[:guard] == 0xA5).all()) and bool((big[guard + nbytes:] == 0xA5).all())
    env.close()


def test_env_ids():
    import torch
    from rsoccer_amd import _lib as L
    from rsoccer_amd.Render import VSS_VIEW
    from rsoccer_amd.vec import VecVSSEnv
    env = VecVSSEnv(64, seed=21)
    env.reset()
    env.step_random(30)
    full = env.render(scale=100)
    ids = [5, 3, 60, 3, 17, 0, 63]
    for given in (ids, np.asarray(ids), torch.tensor(ids), torch.tensor(ids, device=env.device, dtype=torch.int32),
                  torch.tensor(ids, device=env.device, dtype=torch.int64)):
        for cf in (False, True):
            sub = env.render(given, scale=100, channels_first=cf)
            want = full[ids].permute(0, 3, 1, 2) if cf else full[ids]
            assert torch.equal(sub, want)
    assert env.sim.render_errors() == 0
    bad = env.render([2, 64, -1, 7], scale=100)
    field = torch.from_numpy(L.render_field(dict(VSS_VIEW, scale=100))).to(env.device)
    assert torch.equal(bad[0], full[2]) and torch.equal(bad[3], full[7])
    assert torch.equal(bad[1], field) and torch.equal(bad[2], field)
    assert env.sim.render_errors() == 2 and env.sim.render_errors() == 0
    with pytest.raises(ValueError):
        env.render(torch.tensor([0.5, 1.0]), scale=100)
    with pytest.raises(ValueError):
        env.render([], scale=100)
    env.close()


def test_layouts_and_out():
    import torch
    from rsoccer_amd.vec import VecSSLStaticDefendersEnv
    env = VecSSLStaticDefendersEnv(33, seed=2)
    env.reset()
    env.step_random(20)
    for scale in (20, 100):
        hwc = env.render(scale=scale)
        chw = env.render(scale=scale, channels_first=True)
        H, W = env.render_shape(scale=scale)
        assert hwc.shape == (33, H, W, 3) and chw.shape == (33, 3, H, W) and hwc.dtype == torch.uint8 and hwc.device == env.device
        assert torch.equal(chw, hwc.permute(0, 3, 1, 2))
    H, W = env.render_shape()
    assert (H, W) == (670, 970)     # the reference's window (Render/raster.py)
    out = torch.zeros(4, H, W, 3, dtype=torch.uint8, device=env.device)
    ptr = out.data_ptr()
    got = env.render([1, 2, 3, 4], out=out)
    assert got is out and out.data_ptr() == ptr and torch.equal(out, env.render([1, 2, 3, 4]))
    before = out.clone()
    for wrong in (torch.zeros(4, W, H, 3, dtype=torch.uint8, device=env.device),            # shape
                  torch.zeros(3, H, W, 3, dtype=torch.uint8, device=env.device),            # frames
                  torch.zeros(4, H, W, 3, dtype=torch.int8, device=env.device),             # dtype
                  torch.zeros(4, H, W, 3, dtype=torch.uint8),                               # device
                  torch.zeros(4, 3, H, W, dtype=torch.uint8, device=env.device).permute(0, 2, 3, 1)):   # not dense
        with pytest.raises(ValueError):
            env.render([1, 2, 3, 4], out=wrong)
    with pytest.raises(ValueError):
        env.render(view="window")
    assert torch.equal(out, before)
    env.close()


def test_rendering_is_read_only():
    import torch
    from rsoccer_amd.vec import VecVSSEnv
    a, b = VecVSSEnv(256, seed=77), VecVSSEnv(256, seed=77)
    oa, _ = a.reset()
    ob, _ = b.reset()
    assert torch.equal(oa, ob)
    g = torch.Generator(device="cpu").manual_seed(1)
    for t in range(100):
        act = (torch.rand(256, 2, generator=g) * 2 - 1).to(a.device)
        ra = a.step(act)
        frames = a.render(scale=64, channels_first=True)
        rb = b.step(act)
        for x, y in zip(ra[:4], rb[:4]):
            assert torch.equal(x, y), t
        assert torch.equal(a.state, b.state), t
    assert torch.equal(frames, a.render(scale=64, channels_first=True))
    assert torch.equal(frames, b.render(scale=64, channels_first=True))
    a.close(); b.close()


def test_step_and_render_replay_from_one_graph():
    """step(actions) -> render(out=buf) captured into one graph (a linear one) and replayed: the frames and the state of the same
    steps issued eagerly"""
    import torch
    from rsoccer_amd.vec import VecVSSEnv
    B = 128
    envs = [VecVSSEnv(B, seed=5), VecVSSEnv(B, seed=5)]
    actions = (torch.rand(B, 2, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(envs[0].device)
    bufs = []
    for env in envs:
        env.reset()
        H, W = env.render_shape(scale=64)
        bufs.append(torch.zeros(B, 3, H, W, dtype=torch.uint8, device=env.device))
    cap, eag = envs
    cap.enable_graph_capture()
    cap.render(scale=64, channels_first=True, out=bufs[0])      # opens the view (a synchronising call) outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        cap.step(actions)
        cap.render(scale=64, channels_first=True, out=bufs[0])
    for _ in range(20):
        g.replay()
    for _ in range(20):
        eag.step(actions)
        eag.render(scale=64, channels_first=True, out=bufs[1])
    torch.cuda.synchronize()
    assert torch.equal(cap.state, eag.state)
    assert torch.equal(bufs[0], bufs[1])
    assert int((bufs[0] != bufs[0][:1]).sum()) > 0      # (the envs differ: the frames are not all one picture)
    for env in envs:
        env.close()


def test_hook_layers_render_with_the_same_call():
    import torch
    from rsoccer_amd.Render import VSS_VIEW
    from rsoccer_amd.vec import VecScalarHookEnv, VecVSSBaseEnv
    from rsoccer_amd.vss.env_vss import VSSEnv
    B = 32

    class Task(VecVSSBaseEnv):
        def __init__(self):
            super().__init__(0, 3, 3, 0.025, B)

        def _get_commands(self, action):
            self.commands[:, :, :].copy_(action.t().reshape(6, 2, B) * 30.0)

        def _frame_to_observations(self):
            return torch.stack([self.frame.ball.x, self.frame.ball.y], 1)

        def _calculate_reward_and_done(self):
            return self.frame.ball.x, self.frame.ball.x > 10.0

        def _get_initial_positions(self):
            e = torch.arange(B, device="cuda", dtype=torch.float32)
            ball = torch.zeros(B, 4, device="cuda"); ball[:, 0] = 0.01 * e - 0.15; ball[:, 1] = 0.3 - 0.02 * e
            blue = torch.zeros(B, 3, 3, device="cuda"); yellow = torch.zeros(B, 3, 3, device="cuda")
            for k in range(3):
                blue[:, k, 0] = -0.2 - 0.15 * k; blue[:, k, 1] = 0.02 * e - 0.3; blue[:, k, 2] = 11.0 * e + 40.0 * k
                yellow[:, k, 0] = 0.2 + 0.15 * k; yellow[:, k, 1] = 0.3 - 0.02 * e; yellow[:, k, 2] = -7.0 * e - 40.0 * k
            return ball, blue, yellow

    env = Task()
    env.reset()
    g = torch.Generator().manual_seed(8)
    for _ in range(25):
        env.step((torch.rand(B, 12, generator=g) * 2 - 1).to(env.device))
    got = env.render(scale=100).cpu().numpy()
    assert got.shape[1:3] == env.render_shape(scale=100)
    ref = reference_frames(dict(VSS_VIEW, scale=100), env.frame.state.cpu().numpy(), 3, 3, True)   # the CURRENT buffer after the flips
    compare_frames(got, ref, "hooks-vss-100")
    env.close()

    np.random.seed(4)
    venv = VecScalarHookEnv(VSSEnv, 6)
    venv.reset()
    for when in ("after reset", "after steps"):
        got = venv.render(scale=100)
        assert got.is_cuda and got.dtype == torch.uint8
        ref = reference_frames(dict(VSS_VIEW, scale=100), venv.pool.sim.get_state().T, 3, 3, True)
        compare_frames(got.cpu().numpy(), ref, f"scalar-hooks-vss-100 {when}")
        for _ in range(10):
            venv.step(np.random.uniform(-1, 1, (6, 2)))
    venv.close()


def test_views_of_a_handle_stay_alive_next_to_a_captured_render():
    """observations at one scale from a graph, a video grid at another in between: the graph keeps drawing its own view into its own
    buffer (the handle never frees or moves a view's template), the eager call draws the other; both equal a second env's frames"""
    import torch
    from rsoccer_amd.vec import VecVSSEnv
    B = 64
    cap, eag = VecVSSEnv(B, seed=9), VecVSSEnv(B, seed=9)
    actions = (torch.rand(B, 2, generator=torch.Generator().manual_seed(4)) * 2 - 1).to(cap.device)
    for env in (cap, eag):
        env.reset()
    H, W = cap.render_shape(scale=64)
    pix = torch.zeros(B, 3, H, W, dtype=torch.uint8, device=cap.device)
    cap.enable_graph_capture()
    cap.render(scale=64, channels_first=True, out=pix)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        cap.step(actions)
        cap.render(scale=64, channels_first=True, out=pix)
    # a view the handle has not seen cannot be opened inside a capture: refused, nothing enqueued
    from rsoccer_amd import _lib as L
    side = torch.cuda.Stream()
    with pytest.raises(L.RsxError, match="captur"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
            cap.render(scale=96)
    L.drop_pending_hip_error()
    torch.cuda.synchronize()
    for i in range(12):
        g.replay()
        eag.step(actions)
        if i % 3 == 0:      # another view in between (new at i == 0, selected afterwards), and the reference window once
            grid = cap.render([0, 1, 2, 3], scale=128)
            assert torch.equal(grid, eag.render([0, 1, 2, 3], scale=128))
            assert grid.shape == (4, 192, 217, 3)
        if i == 6:
            assert torch.equal(cap.render([5]), eag.render([5]))
    torch.cuda.synchronize()
    assert torch.equal(cap.state, eag.state)
    assert torch.equal(pix, eag.render(scale=64, channels_first=True))
    assert cap.sim.render_errors() == 0
    # the frame size is the handle's: a view opened on the Sim directly is the one the next render of that size draws, and the env's
    # own call selects its view again (no stale size on the env)
    from rsoccer_amd.Render import VSS_VIEW
    assert cap.sim.render_open(dict(VSS_VIEW, scale=37.5)) == (56, 63)
    assert cap.render(scale=64).shape == (B, 96, 108, 3)
    # at most 16 views per handle; the refusal leaves the current view in place
    with pytest.raises(L.RsxError, match="16"):
        for k in range(20):
            cap.sim.render_open(dict(VSS_VIEW, scale=20 + k))
    assert torch.equal(cap.render(scale=64, channels_first=True), pix)
    cap.close(); eag.close()
