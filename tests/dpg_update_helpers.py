"""numpy restatements of the off-policy update phase's arithmetic as include/rsx.h writes it out (rsx_replay_sample_rows,
rsx_dpg_adam_step), shared by tests/test_dpg_update_ref.py (no GPU) and tests/test_gpu_dpg_update.py.  The row draw is integer
arithmetic only; the Adam step of a group is ppo_update_helpers.clip_adam's on that group's tensor alone."""
import numpy as np

import ppo_update_helpers as PH

M32 = np.uint64(0xFFFFFFFF)
DOM_ROWS = 11
COUNTERS = ("t_critic", "t_actor", "steps", "spare")


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox4(c0, c1, c2, c3, k0, k1):
    """the four words of philox4x32-7(counter = (c0, c1, c2, c3), key = (k0, k1)); every argument a uint64 array of 32-bit values
    (broadcast).  Word 0 is ppo_update_helpers.philox_word0 (tests/test_dpg_update_ref.py compares them)."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(a) for a in (c0, c1, c2, c3, k0, k1)))
    for _ in range(7):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2   # (32 x 32 bits: no overflow in 64)
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def sample_rows_at(t, fill, seed, step, n_batch_rows=None):
    """rows[t] of rsx_replay_sample_rows for an array of entries t: int64.  fill is clamped to [0, n_batch_rows] when that is given;
    fill == 0 gives -1.  step: a signed or unsigned 64-bit integer (its two's complement bits key the draw)."""
    t = np.asarray(t, dtype=np.int64)
    fill = int(fill)
    if n_batch_rows is not None:
        fill = min(max(fill, 0), int(n_batch_rows))
    assert 0 <= fill <= 2 ** 31 - 1
    if fill == 0:
        return np.full(t.shape, -1, dtype=np.int64)
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    words = philox4(t.astype(np.uint64) >> np.uint64(2), step >> 32, step & 0xFFFFFFFF, DOM_ROWS, seed & 0xFFFFFFFF, seed >> 32)
    word = np.choose(t & 3, words)
    return ((word * np.uint64(fill)) >> np.uint64(32)).astype(np.int64)   # (32 x 31 bits: no overflow in 64)


def sample_rows(m, fill, seed, step, n_batch_rows=None):
    """the whole rows [m] of rsx_replay_sample_rows"""
    return sample_rows_at(np.arange(m), fill, seed, step, n_batch_rows)


def polyak(p, targ, tau):
    """d = p - targ; targ + tau * d in float32, each operation rounded"""
    p, targ = np.asarray(p, dtype=np.float32), np.asarray(targ, dtype=np.float32)
    d = p - targ
    out = targ + np.float32(tau) * d
    assert out.dtype == np.float32
    return out


def fresh_state(n_actor, n_critic):
    """the optimiser state of rsx_dpg_adam_step at the start of training: m and v per group (actor, critics) and the counters [4]"""
    z = lambda n: np.zeros(n, dtype=np.float32)   # noqa: E731
    return {"m": [z(n_actor), z(n_critic)], "v": [z(n_actor), z(n_critic)], "counters": [0, 0, 0, 0]}


def dpg_adam_step(state, p_actor, targ_actor, p_critic, targ_critic, g_actor, g_critic, lr_actor, lr_critic, betas=(0.9, 0.999),
                  eps=1e-8, max_norm=None, tau=0.005, update_targets=None):
    """one rsx_dpg_adam_step on flat float32 arrays; g_actor None: no actor step; update_targets None: iff the actor stepped.
    `state` (fresh_state) is updated in place.  Returns (p_actor, targ_actor, p_critic, targ_critic, stats [3] float32)."""
    f32 = np.float32
    c = state["counters"]
    move = (g_actor is not None) if update_targets is None else bool(update_targets)
    p_actor, targ_actor, p_critic, targ_critic = (np.asarray(x, dtype=f32).reshape(-1).copy() for x in (p_actor, targ_actor, p_critic, targ_critic))
    empty = np.zeros(0, f32)   # clip_adam takes three tensors: the group, and two empty ones that add nothing to the norm
    c[0] += 1
    (p_critic, _, _), (mc, _, _), (vc, _, _), norm_c = PH.clip_adam([p_critic, empty, empty], [np.asarray(g_critic, f32).reshape(-1), empty, empty],
                                                                  [state["m"][1], empty, empty], [state["v"][1], empty, empty], c[0], lr_critic,
                                                                  betas=betas, eps=eps, max_norm=max_norm)
    state["m"][1], state["v"][1] = mc, vc
    norm_a = f32(0.0)
    if g_actor is not None:
        c[1] += 1
        (p_actor, _, _), (ma, _, _), (va, _, _), norm_a = PH.clip_adam([p_actor, empty, empty], [np.asarray(g_actor, f32).reshape(-1), empty, empty],
                                                                      [state["m"][0], empty, empty], [state["v"][0], empty, empty], c[1], lr_actor,
                                                                      betas=betas, eps=eps, max_norm=max_norm)
        state["m"][0], state["v"][0] = ma, va
    c[2] += 1
    if move:
        targ_actor, targ_critic = polyak(p_actor, targ_actor, tau), polyak(p_critic, targ_critic, tau)
    return p_actor, targ_actor, p_critic, targ_critic, np.array([norm_c, norm_a, 1.0 if move else 0.0], dtype=f32)
