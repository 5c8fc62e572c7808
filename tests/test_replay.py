"""rsoccer_amd.vec.replay.ReplayBuffer on CPU tensors: successor rows against a scalar loop, the ring's wrap, sample_rows inside the
filled part, and the refusals."""
import numpy as np
import pytest

OD, AD = 5, 2


def _batch(torch, T, B, seed):
    """a synthetic collect(..., return_final_obs=True) batch with terminated, truncated (and both) rows, some of them at the last step"""
    gen = torch.Generator().manual_seed(seed)
    term = torch.rand(T, B, generator=gen) < 0.2
    trunc = torch.rand(T, B, generator=gen) < 0.2
    term[T - 1, 0], trunc[T - 1, 0] = True, False
    term[T - 1, 1], trunc[T - 1, 1] = False, True
    term[T - 1, 2], trunc[T - 1, 2] = False, False
    term[T - 1, 3], trunc[T - 1, 3] = True, True
    term[0, 0], trunc[0, 0] = True, False
    term[0, 1], trunc[0, 1] = False, True
    term[0, 2], trunc[0, 2] = False, False
    term[0, 3], trunc[0, 3] = True, True
    ended = term | trunc
    final = torch.randn(T, B, OD, generator=gen) * ended.unsqueeze(-1)   # zeros except at ended rows, as collect() leaves it
    return {"obs": torch.randn(T, B, OD, generator=gen), "actions": torch.randn(T, B, AD, generator=gen), "reward": torch.randn(T, B, generator=gen),
            "terminated": term, "truncated": trunc, "final_obs": final, "next_obs": torch.randn(B, OD, generator=gen)}


def _scalar_rows(batch):
    """the T * B transitions of a batch, one at a time, step-major"""
    T, B = batch["reward"].shape
    rows = []
    for t in range(T):
        for e in range(B):
            if bool(batch["terminated"][t, e]) or bool(batch["truncated"][t, e]):
                nxt = batch["final_obs"][t, e]
            elif t + 1 < T:
                nxt = batch["obs"][t + 1, e]
            else:
                nxt = batch["next_obs"][e]
            rows.append((batch["obs"][t, e], batch["actions"][t, e], float(batch["reward"][t, e]), nxt, bool(batch["terminated"][t, e])))
    return rows


def _assert_row(torch, data, at, row):
    obs, act, rew, nxt, term = row
    assert torch.equal(data["obs"][at], obs) and torch.equal(data["actions"][at], act) and float(data["reward"][at]) == rew
    assert torch.equal(data["next_obs"][at], nxt) and bool(data["terminated"][at]) == term


def test_successor_rows_against_a_scalar_loop():
    import torch
    from rsoccer_amd.vec.replay import ReplayBuffer
    T, B = 6, 7
    batch = _batch(torch, T, B, 1)
    buf = ReplayBuffer(100, OD, AD, "cpu")
    assert buf.add(batch) == T * B and int(buf.head) == T * B and int(buf.fill) == T * B
    data = buf.data()
    assert set(data) == {"obs", "actions", "reward", "next_obs", "terminated"} and data["obs"].shape == (100, OD)
    want = _scalar_rows(batch)
    kinds = set()
    for i, row in enumerate(want):
        _assert_row(torch, data, i, row)
        t, e = divmod(i, B)
        kinds.add((bool(batch["terminated"][t, e]), bool(batch["truncated"][t, e]), t == T - 1))
    assert len(kinds) == 8, kinds   # every combination of terminated, truncated and last step occurs
    # a row that ended on the time limit only bootstraps: terminated = 0 and the terminal observation
    only = (~batch["terminated"] & batch["truncated"]).reshape(-1)
    assert bool(only.any()) and not bool(data["terminated"][:T * B][only].any())
    assert torch.equal(data["next_obs"][:T * B][only], batch["final_obs"].reshape(-1, OD)[only])
    assert not bool(data["obs"][T * B:].any())


def test_the_ring_wraps_across_two_adds_that_straddle_the_capacity():
    import torch
    from rsoccer_amd.vec.replay import ReplayBuffer
    T, B, cap = 4, 5, 33
    a, b = _batch(torch, T, B, 2), _batch(torch, T, B, 3)
    buf = ReplayBuffer(cap, OD, AD, "cpu")
    gen = torch.Generator().manual_seed(0)
    assert bool((buf.sample_rows(50, generator=gen) == -1).all())   # empty: nothing valid to draw
    buf.add(a)
    rows = buf.sample_rows(4000, generator=gen)
    assert rows.dtype == torch.int32 and rows.shape == (4000,) and int(rows.min()) == 0 and int(rows.max()) == T * B - 1
    buf.add(b)
    assert int(buf.head) == (2 * T * B) % cap == 7 and int(buf.fill) == cap
    data = buf.data()
    wa, wb = _scalar_rows(a), _scalar_rows(b)
    for i, row in enumerate(wb):   # the second batch from row 20 on, its tail at rows 0 .. 6
        _assert_row(torch, data, (T * B + i) % cap, row)
    for i in range(7, T * B):      # what is left of the first
        _assert_row(torch, data, i, wa[i])
    rows = buf.sample_rows(8000, generator=gen)
    assert int(rows.min()) == 0 and int(rows.max()) == cap - 1
    counts = np.bincount(rows.numpy(), minlength=cap)
    assert counts.min() > 0.5 * 8000 / cap   # uniform over the filled part
    buf.add(a)
    assert int(buf.head) == 27 and int(buf.fill) == cap
    assert torch.equal(buf.sample_rows(16, generator=torch.Generator().manual_seed(4)), buf.sample_rows(16, generator=torch.Generator().manual_seed(4)))


def test_refusals():
    import torch
    from rsoccer_amd.vec.replay import ReplayBuffer
    batch = _batch(torch, 4, 5, 6)
    buf = ReplayBuffer(19, OD, AD, "cpu")
    with pytest.raises(ValueError, match="final_obs"):
        buf.add({k: v for k, v in batch.items() if k != "final_obs"})
    with pytest.raises(ValueError, match="final_obs"):
        buf.add({**batch, "final_obs": None})
    with pytest.raises(ValueError, match="holds 19"):
        buf.add(batch)
    with pytest.raises(ValueError, match="truncated"):
        buf.add({k: v for k, v in batch.items() if k != "truncated"})
    roomy = ReplayBuffer(20, OD, AD, "cpu")
    for key, value in (("obs", torch.zeros(4, 5, OD + 1)), ("actions", torch.zeros(4, 5, AD + 1)), ("reward", torch.zeros(4, 6)),
                       ("next_obs", torch.zeros(4, OD)), ("final_obs", torch.zeros(4, 5, OD + 1))):
        with pytest.raises(ValueError, match=key):
            roomy.add({**batch, key: value})
    assert int(roomy.fill) == 0 and int(roomy.head) == 0
    roomy.add(batch)
    assert int(roomy.fill) == 20 and int(roomy.head) == 0
    with pytest.raises(ValueError):
        roomy.sample_rows(0)
    for bad in (dict(capacity=0), dict(obs_dim=0), dict(act_dim=0)):
        with pytest.raises(ValueError):
            ReplayBuffer(**{**dict(capacity=4, obs_dim=OD, act_dim=AD, device="cpu"), **bad})
