"""The numpy restatement of rsx_sac_adam_step (tests/sac_update_helpers.py) pinned without a GPU: against torch's own optimisers in
float64 by the project's standing criterion, and in the two places where the three groups could leak into each other — a group's step
count and the clip coefficient."""
import numpy as np
import pytest

import ppo_update_helpers as PH
import sac_update_helpers as H


def _start(na, nc, seed):
    import torch
    gen = torch.Generator().manual_seed(seed)
    start = [torch.randn(n, generator=gen) * 0.3 for n in (na, nc, nc)] + [torch.tensor([-1.2])]   # actor, critics, their target, log_alpha
    grads = [(torch.randn(na, generator=gen), torch.randn(nc, generator=gen), torch.randn(1, generator=gen)) for _ in range(3)]
    return start, grads


@pytest.mark.parametrize("max_norm", [None, 0.5])
def test_three_restated_steps_agree_with_torch_in_float64(max_norm):
    """Criterion (docs/VERIFICATION.md f13): after each of three steps the error of every tensor against float64 — three
    torch.optim.Adam behind two clip_grad_norm_ calls plus lerp_ — is at most 4 x the largest error torch's own float32 run shows."""
    import torch
    na, nc, LRS, TAU = 645, 1300, (1e-3, 3e-3, 2e-3), 0.05
    start, grads = _start(na, nc, 4)
    ref64 = H.torch_steps(start, grads, LRS, max_norm, TAU, torch.float64)
    yard32 = H.torch_steps(start, grads, LRS, max_norm, TAU, torch.float32)
    st = H.fresh_state(na, nc)
    pa, pc, tc, la = (x.numpy().copy() for x in start)
    for k, (ga, gc, gl) in enumerate(grads):
        pa, pc, tc, la, stats = H.sac_adam_step(st, pa, pc, tc, la, ga.numpy(), gc.numpy(), gl.numpy(), *LRS, max_norm=max_norm, tau=TAU)
        H.check_against_torch(H.tensors_of(st, pa, pc, tc, la), ref64[k], yard32[k], k + 1, "restatement")
        assert stats[2] == la[0] and stats[3] == 1.0
        assert abs(float(stats[0]) - float(np.linalg.norm(gc.double().numpy()))) <= 1e-6 * float(stats[0])
    assert st["counters"] == [3, 3, 3, 3]


def test_a_step_without_grad_log_alpha_then_one_with_it_uses_t_alpha_1():
    na, nc = 70, 90
    rng = np.random.default_rng(3)
    f32 = np.float32
    pa, pc, tc = (rng.standard_normal(n).astype(f32) for n in (na, nc, nc))
    la = np.array([0.4], f32)
    st = H.fresh_state(na, nc)
    g = lambda n: rng.standard_normal(n).astype(f32)   # noqa: E731
    pa, pc, tc, la1, stats = H.sac_adam_step(st, pa, pc, tc, la, g(na), g(nc), None, 1e-3, 1e-3, 1e-2)
    assert np.array_equal(la1, la) and stats[2] == la[0]
    assert st["counters"] == [1, 1, 0, 1] and not st["m"][2].any() and not st["v"][2].any()
    gl = np.array([0.7], f32)
    pa, pc, tc, la2, stats = H.sac_adam_step(st, pa, pc, tc, la1, g(na), g(nc), gl, 1e-3, 1e-3, 1e-2)
    assert st["counters"] == [2, 2, 1, 2]
    z = [np.zeros(0, f32)] * 2
    want = {t: PH.clip_adam([la, *z], [gl, *z], [np.zeros(1, f32), *z], [np.zeros(1, f32), *z], t, 1e-2, max_norm=None)[0][0] for t in (1, 2)}
    assert want[1][0] != want[2][0]          # (the two step counts give different bits: the test can tell them apart)
    assert np.array_equal(la2, want[1])
    # the first Adam step of a scalar moves it by lr * sign(g) to within eps
    assert abs(float(la2[0]) - (0.4 - 1e-2)) < 1e-6


def test_a_clip_that_binds_on_the_actor_leaves_log_alphas_step_unclipped():
    na, nc = 300, 500
    rng = np.random.default_rng(5)
    f32 = np.float32
    pa, pc, tc = (rng.standard_normal(n).astype(f32) for n in (na, nc, nc))
    la, gl = np.array([-0.3], f32), np.array([2.5], f32)
    ga, gc = (10.0 * rng.standard_normal(na)).astype(f32), (10.0 * rng.standard_normal(nc)).astype(f32)
    out = {}
    for max_norm in (None, 0.5):
        st = H.fresh_state(na, nc)
        res = H.sac_adam_step(st, pa, pc, tc, la, ga, gc, gl, 1e-3, 1e-3, 1e-2, max_norm=max_norm)
        out[max_norm] = (res, st)
        assert res[4][1] > 100.0   # the actor's norm before the clip: the bound of 0.5 binds
    (free, st_free), (clipped, st_clip) = out[None], out[0.5]
    assert np.array_equal(free[3], clipped[3])                                        # log_alpha: the same bits
    assert np.array_equal(st_free["m"][2], st_clip["m"][2]) and np.array_equal(st_free["v"][2], st_clip["v"][2])
    assert st_clip["m"][2][0] == f32(f32(1.0 - 0.9) * gl[0])                           # m = omb1 * g with coef 1
    assert not np.array_equal(st_free["m"][0], st_clip["m"][0])                       # while the actor's moments are the clipped gradient's
    assert not np.array_equal(st_free["m"][1], st_clip["m"][1])
