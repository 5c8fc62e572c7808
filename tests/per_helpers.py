"""numpy restatements of prioritised and n-step replay as include/rsx.h writes it out (rsx_replay_add_nstep, the priority tree,
rsx_replay_sample_prioritized), shared by tests/test_replay_per_ref.py (no GPU) and tests/test_gpu_replay_per.py; and a brute-force
float64 definition of the n-step transition, a plain loop over the episode, that the fold is checked against."""
import numpy as np

import dpg_update_helpers as UH

FAN = 64
PER_DRAW_WORD = 14
STATE = ("max", "wmax", "skipped", "ticket")
f32 = np.float32


# ---- the n-step fold ----
def fold(reward, terminated, truncated, n_step, gamma):
    """per row (t, b) of a [T, B] batch: (reward, discount, terminated, m, kind, at) in the header's float32 order.  kind / at: the
    successor is final_obs[at] (kind 0), obs[at] (1) with at = (t', b) flattened to t' * B + b, or next_obs[b] (2, at = b)."""
    reward = np.asarray(reward, dtype=f32)
    term, trunc = np.asarray(terminated).astype(bool), np.asarray(truncated).astype(bool)
    T, B = reward.shape
    g0 = f32(gamma)
    R, G = np.zeros((T, B), f32), np.zeros((T, B), f32)
    term_out, m_out = np.zeros((T, B), bool), np.zeros((T, B), np.int64)
    kind, at = np.zeros((T, B), np.int64), np.zeros((T, B), np.int64)
    for t in range(T):
        for b in range(B):
            r, g, m = reward[t, b], g0, 1
            while not (term[t + m - 1, b] or trunc[t + m - 1, b]) and m < n_step and t + m < T:
                r = f32(r + f32(g * reward[t + m, b]))
                g = f32(g * g0)
                m += 1
            last = t + m - 1
            R[t, b], G[t, b], term_out[t, b], m_out[t, b] = r, g, term[last, b], m
            if term[last, b] or trunc[last, b]:
                kind[t, b], at[t, b] = 0, last * B + b
            elif t + m < T:
                kind[t, b], at[t, b] = 1, (t + m) * B + b
            else:
                kind[t, b], at[t, b] = 2, b
    return R, G, term_out, m_out, kind, at


def brute_nstep(reward, terminated, truncated, n_step, gamma):
    """the definition, in float64: from step t walk the episode forward, collecting at most n_step rewards, stopping after the step
    that ends the episode and at the end of the batch.  Returns (return, discount, terminated, m, kind, at) per row."""
    reward = np.asarray(reward, dtype=np.float64)
    T, B = reward.shape
    out = [np.zeros((T, B), np.float64), np.zeros((T, B), np.float64), np.zeros((T, B), bool), np.zeros((T, B), np.int64),
           np.zeros((T, B), np.int64), np.zeros((T, B), np.int64)]
    for b in range(B):
        for t in range(T):
            steps = []
            for s in range(t, T):
                steps.append(s)
                if terminated[s][b] or truncated[s][b] or len(steps) == n_step:
                    break
            m, last = len(steps), steps[-1]
            ret = sum(float(gamma) ** k * reward[s, b] for k, s in enumerate(steps))
            ended = bool(terminated[last][b] or truncated[last][b])
            k, a = (0, last * B + b) if ended else (1, (last + 1) * B + b) if last + 1 < T else (2, b)
            for o, v in zip(out, (ret, float(gamma) ** m, bool(terminated[last][b]), m, k, a)):
                o[t, b] = v
    return tuple(out)


def new_ring(capacity, obs_dim, act_dim):
    return {"obs": np.zeros((capacity, obs_dim), f32), "actions": np.zeros((capacity, act_dim), f32), "reward": np.zeros(capacity, f32),
            "next_obs": np.zeros((capacity, obs_dim), f32), "terminated": np.zeros(capacity, bool), "discount": np.zeros(capacity, f32),
            "head": 0, "fill": 0}


def ring_add(ring, batch, n_step, gamma):
    """rsx_replay_add_nstep on a numpy ring (new_ring), in place; returns the rows written, in order"""
    obs = np.asarray(batch["obs"], f32)
    T, B, OD = obs.shape
    n, cap = T * B, ring["reward"].shape[0]
    R, G, term, _, kind, at = fold(batch["reward"], batch["terminated"], batch["truncated"], n_step, gamma)
    sources = (np.asarray(batch["final_obs"], f32).reshape(n, OD), obs.reshape(n, OD), np.asarray(batch["next_obs"], f32))
    succ = np.stack([sources[k][a] for k, a in zip(kind.reshape(n), at.reshape(n))])
    rows = (ring["head"] + np.arange(n)) % cap
    ring["obs"][rows], ring["actions"][rows] = obs.reshape(n, OD), np.asarray(batch["actions"], f32).reshape(n, -1)
    ring["reward"][rows], ring["discount"][rows], ring["terminated"][rows], ring["next_obs"][rows] = R.reshape(n), G.reshape(n), term.reshape(n), succ
    ring["head"], ring["fill"] = (ring["head"] + n) % cap, min(ring["fill"] + n, cap)
    return rows


def make_batch(rng, T, B, obs_dim, act_dim, ends=(), truncs=()):
    """a random [T, B] batch; ends / truncs: (t, b) pairs with terminated / truncated set"""
    b = {"obs": rng.standard_normal((T, B, obs_dim)).astype(f32), "actions": rng.uniform(-1, 1, (T, B, act_dim)).astype(f32),
         "reward": rng.standard_normal((T, B)).astype(f32), "terminated": np.zeros((T, B), bool), "truncated": np.zeros((T, B), bool),
         "final_obs": rng.standard_normal((T, B, obs_dim)).astype(f32), "next_obs": rng.standard_normal((B, obs_dim)).astype(f32)}
    for t, e in ends:
        b["terminated"][t, e % B] = True
    for t, e in truncs:
        b["truncated"][t, e % B] = True
    return b


def fold_case(rng, T, B, obs_dim=3, act_dim=2):
    """the batch every fold test uses: an end at t = 0 and at t = T - 1, two ends closer together than any n > 2, a truncation with
    terminated = 0, and columns without an end (all columns modulo B)"""
    return make_batch(rng, T, B, obs_dim, act_dim, ends=((0, 0), (T - 1, 1), (1, 2), (2, 2)), truncs=((2, 0), (T - 2, 1), (3, 5)))


# ---- the tree ----
def tree_geometry(capacity):
    """(floats, levels, offsets): level 0 the leaves, level `levels` the root, every level padded to a multiple of 64 floats"""
    n, off, offsets = int(capacity), 0, []
    while True:
        size = (n + FAN - 1) // FAN * FAN
        offsets.append(off)
        off += size
        if len(offsets) > 1 and n == 1:
            break
        n = size // FAN
    return off, len(offsets) - 1, offsets


def node_sums(children):
    """[n, 64] float32 -> [n]: ((c_0 + c_1) + c_2) + ... + c_63, every addition rounded, from 0"""
    children = np.asarray(children, dtype=f32)
    acc = np.zeros(children.shape[0], f32)
    for j in range(FAN):
        acc = acc + children[:, j]
    assert acc.dtype == f32
    return acc


def build_tree(leaves, capacity):
    """the whole array from the leaves [capacity]"""
    floats, levels, off = tree_geometry(capacity)
    tree = np.zeros(floats, f32)
    tree[:capacity] = np.asarray(leaves, f32)
    for l in range(1, levels + 1):
        n = (off[l] - off[l - 1]) // FAN
        tree[off[l]:off[l] + n] = node_sums(tree[off[l - 1]:off[l]].reshape(n, FAN))
    return tree


def check_tree(tree, capacity):
    """every inner node of a tree read back equals the stated-order sum of its children, in bits, and the padding is 0"""
    tree = np.asarray(tree, f32)
    floats, levels, off = tree_geometry(capacity)
    assert tree.shape == (floats,)
    want = build_tree(tree[:capacity], capacity)
    assert np.array_equal(tree[capacity:off[1]], np.zeros(off[1] - capacity, f32))
    assert np.array_equal(tree.view(np.uint32), want.view(np.uint32)), np.flatnonzero(tree.view(np.uint32) != want.view(np.uint32))[:8]


def leaf_value64(td_error, alpha, eps):
    """(|td| + eps)^alpha in float64 from the float32 sum the device forms"""
    a = (np.abs(np.asarray(td_error, f32)) + f32(eps)).astype(f32)
    return a.astype(np.float64) ** float(f32(alpha))


def set_priorities_rows(leaves, rows, values):
    """leaf[rows[t]] = the largest values[t] among the entries of that row; rows outside [0, capacity) are skipped.  In place; returns
    the number skipped."""
    rows, values = np.asarray(rows, np.int64), np.asarray(values, f32)
    ok = (rows >= 0) & (rows < leaves.shape[0])
    leaves[rows[ok]] = 0
    np.maximum.at(leaves, rows[ok], values[ok])
    return int((~ok).sum())


# ---- the draw ----
def draw_words(m, seed, step):
    t = np.arange(m, dtype=np.int64)
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    words = UH.philox4(t.astype(np.uint64) >> np.uint64(2), step >> 32, step & 0xFFFFFFFF, PER_DRAW_WORD, seed & 0xFFFFFFFF, seed >> 32)
    return np.choose(t & 3, words)


def descend(tree, capacity, fill, m, seed, step):
    """rows [m] of rsx_replay_sample_prioritized for a tree array (-1 everywhere with fill == 0 or a total that is not > 0)"""
    tree = np.asarray(tree, f32)
    _, levels, off = tree_geometry(capacity)
    total = tree[off[levels]]
    fill = min(max(int(fill), 0), capacity)
    if fill == 0 or not total > 0:
        return np.full(m, -1, np.int64)
    t = np.arange(m, dtype=np.float64)
    u = np.float64(total) * ((t + draw_words(m, seed, step).astype(np.float64) * 2.0 ** -32) / np.float64(m))
    node = np.zeros(m, np.int64)
    for l in range(levels, 0, -1):
        c = tree[off[l - 1] + node[:, None] * FAN + np.arange(FAN)[None, :]]   # [m, 64]
        p = np.zeros(m, f32)
        pick, before = np.full(m, -1, np.int64), np.zeros(m, f32)
        last, last_before = np.zeros(m, np.int64), np.zeros(m, f32)
        for j in range(FAN):
            pn = p + c[:, j]
            pos = c[:, j] > 0
            last, last_before = np.where(pos, j, last), np.where(pos, p, last_before)
            take = pos & (pick < 0) & (u < pn.astype(np.float64))
            pick, before = np.where(take, j, pick), np.where(take, p, before)
            p = pn
        none = pick < 0
        pick, before = np.where(none, last, pick), np.where(none, last_before, before)
        u = u - before.astype(np.float64)
        node = node * FAN + pick
    return node


def weights64(tree, capacity, fill, rows, beta):
    """the importance weights in float64 from the float32 quotient the device forms: ((float)fill * leaf / total)^(-beta) over the
    largest of the live entries; 0 for an entry of -1"""
    tree = np.asarray(tree, f32)
    _, levels, off = tree_geometry(capacity)
    rows = np.asarray(rows, np.int64)
    live = rows >= 0
    w = np.zeros(rows.shape, np.float64)
    if live.any():
        x = (f32(min(max(int(fill), 0), capacity)) * tree[rows[live]]) / tree[off[levels]]
        assert x.dtype == f32
        w[live] = x.astype(np.float64) ** (-float(f32(beta)))
        w[live] /= w[live].max()
    return w
