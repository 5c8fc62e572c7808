"""The expected result of a transfer of episodes (rsx_task_transfer), built in numpy from two checkpoint blobs: the destination's
blob with the columns ``dst_ids`` of every per-env section overwritten by the columns ``src_ids`` of the source's blob.  Section
sizes come from the blob header (the offsets tests/test_gpu_parity.py reads: ten int32 from byte 8, four uint64 section sizes
from byte 80); everything else of the destination's blob — header, step counter, metrics, physics ranges — stays."""
import numpy as np

HEADER_BYTES = 176          # magic u64 | 14 int32 | key0, key1, env_id_base, tick u32 | 4 u64 section sizes | 8 i64 metrics
PHYS_HEADER_BYTES = 256     # ranges, mask, error word (rsx_phys.hpp: PhysHeader)
PHYS_ROWS = 14 + 18         # RSX_PHYS_PARAMS + RSX_PHYS_COEFS
MODEL_PHYS = 1 << 16        # bit of the header's model word: the blob has a physics section


def blob_layout(blob):
    """{name: (byte offset, shape, dtype, env axis)} of the per-env sections of a checkpoint blob, and the batch size"""
    blob = np.asarray(blob, dtype=np.uint8)
    i32 = blob[8:64].view(np.int32)
    B, SR, AR, OD, model = int(i32[6]), int(i32[7]), int(i32[8]), int(i32[9]), int(i32[13])
    sb, ab, ob, fb = (int(x) for x in blob[80:112].view(np.uint64))
    assert (sb, ab, ob, fb) == (4 * SR * B, 4 * AR * B, 4 * B * OD, 2 * B), "section sizes do not match the configuration"
    lay, off = {}, HEADER_BYTES
    lay["state"] = (off, (SR, B), np.float32, 1); off += sb
    lay["aux"] = (off, (AR, B), np.float32, 1); off += ab
    lay["obs"] = (off, (B, OD), np.float32, 0); off += ob
    lay["final_obs"] = (off, (B, OD), np.float32, 0); off += ob
    lay["flags"] = (off, (2, B), np.uint8, 1); off += fb
    if model & MODEL_PHYS:
        off += PHYS_HEADER_BYTES
        lay["phys"] = (off, (PHYS_ROWS, B), np.float32, 1); off += 4 * PHYS_ROWS * B
    assert off == blob.size, (off, blob.size)
    return lay, B


def section(blob, lay, name):
    """a VIEW of one section of ``blob`` (uint32 words for the float sections: comparisons and copies are on bit patterns)"""
    off, shape, dtype, _ = lay[name]
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = blob[off:off + n]
    return (raw.view(np.uint32) if dtype == np.float32 else raw).reshape(shape)


def expected_blob(dst_blob, src_blob, dst_ids=None, src_ids=None):
    """``dst_blob`` after env ``src_ids[i]`` of ``src_blob`` went into env ``dst_ids[i]`` (None = 0..n-1); pairs with an id out of
    range are skipped.  ``src_blob`` may be ``dst_blob`` itself: every read comes from the unchanged input."""
    dst_blob = np.asarray(dst_blob, dtype=np.uint8)
    src_blob = np.array(src_blob, dtype=np.uint8, copy=True)
    out = np.array(dst_blob, copy=True)
    dl, DB = blob_layout(dst_blob)
    sl, SB = blob_layout(src_blob)
    assert set(dl) == set(sl), "physics on one side only"
    n = len(dst_ids) if dst_ids is not None else len(src_ids) if src_ids is not None else min(DB, SB)
    d = np.arange(n) if dst_ids is None else np.asarray(dst_ids, dtype=np.int64)
    s = np.arange(n) if src_ids is None else np.asarray(src_ids, dtype=np.int64)
    assert d.shape == s.shape == (n,)
    ok = (d >= 0) & (d < DB) & (s >= 0) & (s < SB)
    d, s = d[ok], s[ok]
    assert np.unique(d).size == d.size, "destination ids must be distinct"
    for name, (_, shape, _, axis) in dl.items():
        assert shape[1 - axis] == sl[name][1][1 - axis], name
        to, frm = section(out, dl, name), section(src_blob, sl, name)
        if axis == 1:
            to[:, d] = frm[:, s]
        else:
            to[d] = frm[s]
    return out


def synthetic_blob(B, state_rows, aux_rows, obs_dim, phys, rng):
    """a blob of the checkpoint format with random payload (for the helper's self-check: no device needed)"""
    body = 4 * (state_rows + aux_rows) * B + 2 * 4 * B * obs_dim + 2 * B + (PHYS_HEADER_BYTES + 4 * PHYS_ROWS * B if phys else 0)
    blob = rng.integers(0, 256, HEADER_BYTES + body, dtype=np.uint8)
    i32 = blob[8:64].view(np.int32)
    i32[6], i32[7], i32[8], i32[9] = B, state_rows, aux_rows, obs_dim
    i32[13] = 2 | (MODEL_PHYS if phys else 0)
    blob[80:112].view(np.uint64)[:] = (4 * state_rows * B, 4 * aux_rows * B, 4 * B * obs_dim, 2 * B)
    return blob
