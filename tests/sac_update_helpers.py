"""numpy restatement of the soft actor-critic optimiser step as include/rsx.h writes it out (rsx_sac_adam_step), shared by
tests/test_sac_update_ref.py (no GPU) and tests/test_gpu_sac_update.py.  The Adam step of a group is ppo_update_helpers.clip_adam's on
that group's tensor alone (log_alpha: the same on one element with max_norm=None); the Polyak step is dpg_update_helpers.polyak's; the
rows of the whole call are dpg_update_helpers.sample_rows."""
import numpy as np

import dpg_update_helpers as DH
import ppo_update_helpers as PH

COUNTERS = ("t_critic", "t_actor", "t_alpha", "steps")
T_CRITIC, T_ACTOR, T_ALPHA, STEPS = range(4)


def fresh_state(n_actor, n_critic):
    """the optimiser state of rsx_sac_adam_step at the start of training: m and v per group (actor, critics, log_alpha) and the
    counters [4]"""
    z = lambda n: np.zeros(n, dtype=np.float32)   # noqa: E731
    return {"m": [z(n_actor), z(n_critic), z(1)], "v": [z(n_actor), z(n_critic), z(1)], "counters": [0, 0, 0, 0]}


def _group(state, k, p, g, t, lr, betas, eps, max_norm):
    f32 = np.float32
    empty = np.zeros(0, f32)   # clip_adam takes three tensors: the group, and two empty ones that add nothing to the norm
    (p, _, _), (m, _, _), (v, _, _), norm = PH.clip_adam([p, empty, empty], [np.asarray(g, f32).reshape(-1), empty, empty],
                                                         [state["m"][k], empty, empty], [state["v"][k], empty, empty], t, lr,
                                                         betas=betas, eps=eps, max_norm=max_norm)
    state["m"][k], state["v"][k] = m, v
    return p, norm


def sac_adam_step(state, p_actor, p_critic, targ_critic, log_alpha, g_actor, g_critic, g_log_alpha, lr_actor, lr_critic, lr_alpha,
                  betas=(0.9, 0.999), eps=1e-8, max_norm=None, tau=0.005, update_targets=True):
    """one rsx_sac_adam_step on flat float32 arrays; g_actor None: no actor step; g_log_alpha None: a fixed temperature.  `state`
    (fresh_state) is updated in place.  Returns (p_actor, p_critic, targ_critic, log_alpha [1], stats [4] float32)."""
    f32 = np.float32
    c = state["counters"]
    p_actor, p_critic, targ_critic, log_alpha = (np.asarray(x, dtype=f32).reshape(-1).copy() for x in (p_actor, p_critic, targ_critic, log_alpha))
    assert log_alpha.shape == (1,)
    c[T_CRITIC] += 1
    p_critic, norm_c = _group(state, 1, p_critic, g_critic, c[T_CRITIC], lr_critic, betas, eps, max_norm)
    norm_a = f32(0.0)
    if g_actor is not None:
        c[T_ACTOR] += 1
        p_actor, norm_a = _group(state, 0, p_actor, g_actor, c[T_ACTOR], lr_actor, betas, eps, max_norm)
    if g_log_alpha is not None:
        c[T_ALPHA] += 1
        log_alpha, _ = _group(state, 2, log_alpha, g_log_alpha, c[T_ALPHA], lr_alpha, betas, eps, None)   # never clipped
    c[STEPS] += 1
    if update_targets:
        targ_critic = DH.polyak(p_critic, targ_critic, tau)
    return p_actor, p_critic, targ_critic, log_alpha, np.array([norm_c, norm_a, log_alpha[0], 1.0 if update_targets else 0.0], dtype=f32)


# ---- the torch yardstick: three torch.optim.Adam behind two clip_grad_norm_ calls plus lerp_, in float64 and float32 ----
NAMES = ("actor", "critics", "target_critics", "log_alpha", "m_actor", "v_actor", "m_critics", "v_critics", "m_alpha", "v_alpha")


def rel(x, ref):
    scale = float(np.abs(ref).max())
    return float(np.abs(np.asarray(x, np.float64) - ref).max()) / scale


def torch_steps(start, grads, lrs, max_norm, tau, dtype):
    """`start`: float32 torch tensors (actor, critics, target critics, log_alpha [1]); `grads`: per step (g_actor, g_critic, g_alpha),
    every group stepping on every step; lrs (actor, critic, alpha).  Returns per step a dict NAMES -> numpy array in `dtype`."""
    import torch
    live = [torch.nn.Parameter(start[k].to(dtype).clone()) for k in (0, 1, 3)]   # actor, critics, log_alpha
    targ = start[2].to(dtype).clone()
    opts = [torch.optim.Adam([p], lr=lr) for p, lr in zip(live, lrs)]
    out = []
    for gs in grads:
        for k, (p, g) in enumerate(zip(live, gs)):
            p.grad = g.to(dtype).reshape(p.shape).clone()   # (clip_grad_norm_ scales it in place: never the caller's tensor)
            if max_norm is not None and k < 2:   # log_alpha is never clipped
                torch.nn.utils.clip_grad_norm_([p], max_norm)
            opts[k].step()
        with torch.no_grad():
            targ.lerp_(live[1].detach(), tau)
        mv = [opts[k].state[live[k]][key].numpy().copy() for k in (0, 1, 2) for key in ("exp_avg", "exp_avg_sq")]
        vals = [live[0].detach().numpy().copy(), live[1].detach().numpy().copy(), targ.numpy().copy(), live[2].detach().numpy().copy()] + mv
        out.append(dict(zip(NAMES, vals)))
    return out


def tensors_of(state, p_actor, p_critic, targ_critic, log_alpha):
    """the NAMES dict of a restated (or downloaded) optimiser state and its four tensors"""
    vals = [p_actor, p_critic, targ_critic, log_alpha, state["m"][0], state["v"][0], state["m"][1], state["v"][1], state["m"][2], state["v"][2]]
    return dict(zip(NAMES, (np.asarray(v).reshape(-1) for v in vals)))


def check_against_torch(got, ref64, yard32, step, what):
    """the project's standing criterion: every tensor of `got` within 4 x the largest relative error any tensor of torch's own float32
    run shows against float64"""
    e_yard = max(rel(yard32[n], ref64[n]) for n in NAMES)
    assert e_yard > 0.0
    worst = 0.0
    for n in NAMES:
        e = rel(got[n], ref64[n])
        print(f"step {step} {n}: {what} {e:.3e}, torch f32 pooled {e_yard:.3e} ({e / e_yard:.2f} x)")
        assert e <= 4.0 * e_yard, (step, n, e, e_yard)
        worst = max(worst, e / e_yard)
    return worst
