"""The comparison rules of tests/mass_end_helpers.py can fail: synthetic arrays on the host, no GPU."""
from mass_end_helpers import SENTINEL, final_obs_faults, same_bits, sample_ids


def test_sample_ids_cover_both_ends_and_whole_tiles():
    for B in (64 * 257 + 37, 98304 + 37):
        ids = sample_ids(B)
        assert list(ids[:70]) == list(range(70)) and list(ids[70:171]) == list(range(B - 101, B)) and (B - 101) % 64 == 0
        mid = ids[171:].reshape(3, 64)
        assert (mid == mid[:, :1] + range(64)).all() and not (mid[:, 0] % 64).any() and mid.min() >= 128 and mid.max() < B - 101


def test_final_obs_rules_can_fail():
    """synthetic arrays on the host: each rule of final_obs_faults fires on its own, names what the failure message must name, and a
    clean array passes"""
    import torch
    B, OD = 64 * 3 + 37, 40
    gen = torch.Generator().manual_seed(1)
    term = (torch.arange(B) % 5 == 0).to(torch.uint8)
    trunc = (torch.arange(B) % 3 == 0).to(torch.uint8)
    ended = (term | trunc) != 0
    good = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, OD), generator=gen, dtype=torch.int64).to(torch.int32)
    good[good == SENTINEL] = 0
    good[~ended] = SENTINEL
    assert final_obs_faults(good, term, trunc, good.clone()) == []
    # 1. a row that did not end lost its sentinel in one word
    e = int((~ended).nonzero()[7])
    a = good.clone(); a[e, 36] = 0x3F800000
    msgs = final_obs_faults(a, term, trunc)
    assert len(msgs) == 1 and "did not end" in msgs[0] and f"(env {e}, column 36): 0x3f800000" in msgs[0] and "1 words in 1 envs" in msgs[0]
    assert f"modulo 64: [{e % 64}]" in msgs[0]
    # 2. an ended row kept a sentinel word
    e = int(ended.nonzero()[11])
    a = good.clone(); a[e, 39] = SENTINEL
    msgs = final_obs_faults(a, term, trunc)
    assert len(msgs) == 1 and "keeps the sentinel" in msgs[0] and f"(env {e}, column 39): 0x7fc0beef" in msgs[0]
    # 3. a 64-bit 1 in columns 36 and 37 of sixteen consecutive envs of one tile, all of them ended: only the twin tells
    term1 = torch.ones(B, dtype=torch.uint8)
    full = good.clone(); full[~ended] = 12345
    a = full.clone(); a[64 + 16:64 + 32, 36] = 1; a[64 + 16:64 + 32, 37] = 0
    assert final_obs_faults(full, term1, trunc, full.clone()) == [] and final_obs_faults(a, term1, trunc) == []
    msgs = final_obs_faults(a, term1, trunc, full)
    assert len(msgs) == 1 and "A / T differ" in msgs[0] and "32 words in 16 envs" in msgs[0] and "columns [36, 37]" in msgs[0]
    assert "(env 80, column 36): 0x00000001 / " in msgs[0] and "(env 80, column 37): 0x00000000 / " in msgs[0]
    assert f"modulo 64: {list(range(16, 32))}" in msgs[0]
    assert same_bits("obs", a, full).startswith("obs: A / T differ in 32 words in 16 envs")
    # 1-D tensors and float32 (NaN patterns compare as bits)
    r = torch.tensor([1.0, float("nan"), 3.0])
    assert same_bits("reward", r, r.clone()) is None and "column 0" in same_bits("reward", r, torch.tensor([1.0, 2.0, 3.0]))
