"""What tests/test_gpu_mass_end.py compares with (tests only): the oracle's sample of env ids and the rules of `final_obs` after a step
whose buffer was filled with a NaN pattern first.  The functions take torch tensors on any device; tests/test_mass_end_helpers.py shows
on synthetic host arrays that each rule can fail."""
import numpy as np

SENTINEL = 0x7FC0BEEF   # a quiet NaN no kernel computes: every comparison of final_obs is on int32 views


def sample_ids(B):
    """env ids stepped by the oracle too: the first 70 (a tile and a piece of the next), the last 64 + 37 (the ragged tail and the tile
    before it) and three further whole tiles"""
    full = B // 64
    assert B % 64 == 37 and full >= 8
    tiles = np.random.default_rng(2718).choice(np.arange(2, full - 1), 3, replace=False)
    ids = np.concatenate([np.arange(70), np.arange(B - 101, B)] + [64 * int(t) + np.arange(64) for t in sorted(tiles)])
    assert len(np.unique(ids)) == len(ids) == 70 + 101 + 192
    return ids


# ---- the comparison helpers: torch tensors on any device ----
def _where(bad, a, b=None, limit=8):
    """which (env, column) entries of a [B, C] comparison are bad: the first pairs with their bit patterns, how many envs, and the env ids
    modulo 64 (the lane inside a 64-env tile: sixteen consecutive ones are one pass of a wave's store)"""
    import torch
    idx = bad.nonzero()
    envs = torch.unique(idx[:, 0])
    first = []
    for e, c in idx[:limit].tolist():
        pat = f"{int(a[e, c]) & 0xFFFFFFFF:#010x}"
        if b is not None:
            pat += f" / {int(b[e, c]) & 0xFFFFFFFF:#010x}"
        first.append(f"(env {e}, column {c}): {pat}")
    return (f"{int(idx.shape[0])} words in {int(envs.numel())} envs; first " + "; ".join(first) + f"; columns {torch.unique(idx[:, 1]).tolist()}"
            + f"; env ids modulo 64: {torch.unique(envs % 64).tolist()}; first envs {envs[:20].tolist()}")


def _bits(t):
    """[B, C] integer view of a tensor's bit patterns (rows = envs)"""
    import torch
    if t.dtype == torch.float32:
        t = t.view(torch.int32) if t.is_contiguous() else t.contiguous().view(torch.int32)
    return t if t.dim() == 2 else t[:, None]


def same_bits(name, a, b):
    """None, or how tensor `name` of handle A differs from its twin's"""
    import torch
    a, b = _bits(a), _bits(b)
    if torch.equal(a, b):
        return None
    return f"{name}: A / T differ in " + _where(a != b, a, b)


def final_obs_faults(fin, term, trunc, twin=None):
    """the rules of final_obs after one step, on int32 views ([B, OD]; term, trunc: [B] uint8): a row whose flags are both 0 holds the
    sentinel in every word, a row that ended holds it in none, and (twin given) the twin's row holds the same bits.  -> messages"""
    import torch
    out = []
    ended = ((term | trunc) != 0)[:, None]
    is_s = fin == SENTINEL
    bad = ~ended & ~is_s
    if bool(bad.any()):
        out.append("final_obs written at a row that did not end: " + _where(bad, fin))
    bad = ended & is_s
    if bool(bad.any()):
        out.append("final_obs of an ended row keeps the sentinel: " + _where(bad, fin))
    if twin is not None and not torch.equal(fin, twin):
        out.append("final_obs: A / T differ in " + _where(fin != twin, fin, twin))
    return out
