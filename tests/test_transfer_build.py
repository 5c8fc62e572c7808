"""rsx_task_transfer as a build product (no GPU): the two symbols are declared, listed and exported, rsx_xfer.hip compiles with the
flags build() gives it into kernels without scratch memory whose register counts profiles/LABBOOK.md records, and the numpy blob
helper of the GPU tests is checked on a synthetic blob."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNEL = re.compile(r"transfer_kernelILi(\d+)EE")
MODES = {0: "direct", 1: "gather", 2: "scatter"}


def test_symbols_are_declared_listed_and_exported():
    from build_variant import dynamic_symbols
    from rsoccer_amd import _lib
    header = open(os.path.join(ROOT, "include", "rsx.h")).read()
    assert re.search(r"^int rsx_task_transfer\(rsx_sim\* dst, rsx_sim\* src, const int32_t\* dst_ids_dev, const int32_t\* src_ids_dev, int n, void\* stream\);",
                     header, re.M)
    assert re.search(r"^int rsx_task_transfer_errors\(rsx_sim\* dst, int64_t\* out, void\* stream\);", header, re.M)
    assert "unspecified mixture" in header and "as if every read happened before every write" in header
    defined, _ = dynamic_symbols(_lib.LIB_PATH)
    for sym in ("rsx_task_transfer", "rsx_task_transfer_errors"):
        assert sym in _lib.SYMBOLS and sym in defined, sym
    assert hasattr(_lib.Sim, "task_transfer") and hasattr(_lib.Sim, "task_transfer_errors")


@pytest.fixture(scope="module")
def xfer_kernels():
    """{mode: {remark: value}} of rsx_xfer.hip, compiled with the flags build() gives it (the compiler's kernel-resource-usage remarks)"""
    from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS
    units = dict(HIP_UNITS)
    assert "rsx_xfer.hip" in units, "rsx_xfer.hip is not a unit of librsx_hip.so"
    work = tempfile.mkdtemp(prefix="rsx_xfer_probe_")
    try:
        p = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_COMMON + units["rsx_xfer.hip"] +
                           ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(work, "rsx_xfer.o"),
                            os.path.join(CSRC, "rsx_xfer.hip")], stderr=subprocess.PIPE, text=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = KERNEL.search(m.group(1))
            cur = rows.setdefault(int(k.group(1)), {"name": m.group(1)}) if k else None
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[.*?\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return rows


def test_unit_compiles_to_the_three_transfer_kernels_without_scratch(xfer_kernels):
    from rsoccer_amd import _lib
    assert set(xfer_kernels) == set(MODES), sorted(xfer_kernels)
    blob = open(_lib.LIB_PATH, "rb").read()
    for mode, v in xfer_kernels.items():
        print(MODES[mode], {n: v.get(n) for n in ("VGPRs", "TotalSGPRs", "ScratchSize", "LDS Size", "Occupancy")})
        assert v["ScratchSize"] == 0, v
        assert v["LDS Size"] == 0, v
        assert v["name"].encode() in blob, f"librsx_hip.so lacks {v['name']}"


def test_labbook_records_the_register_counts(xfer_kernels):
    text = open(os.path.join(ROOT, "profiles", "LABBOOK.md")).read()
    rows = {m: (int(v), int(s)) for m, v, s in re.findall(r"^\| `transfer_kernel<(\w+)>` \| (\d+) \| (\d+) \|", text, re.M)}
    assert set(rows) == set(MODES.values()), rows
    for mode, v in xfer_kernels.items():
        assert rows[MODES[mode]] == (v["VGPRs"], v["TotalSGPRs"]), (MODES[mode], rows[MODES[mode]], v)


@pytest.mark.parametrize("phys", [False, True])
def test_blob_helper_on_a_synthetic_blob(phys):
    from transfer_helpers import HEADER_BYTES, PHYS_HEADER_BYTES, PHYS_ROWS, blob_layout, expected_blob, section, synthetic_blob
    rng = np.random.default_rng(1)
    SB, DB, SR, AR, OD = 37, 21, 43, 27, 40
    src, dst = synthetic_blob(SB, SR, AR, OD, phys, rng), synthetic_blob(DB, SR, AR, OD, phys, rng)
    lay, B = blob_layout(dst)
    assert B == DB and set(lay) == {"state", "aux", "obs", "final_obs", "flags"} | ({"phys"} if phys else set())
    # section sizes round-trip: header + sections (+ physics header) = the blob, in the header's order and without gaps
    total = HEADER_BYTES + sum(int(np.prod(shape)) * np.dtype(dt).itemsize for _, shape, dt, _ in lay.values()) + (PHYS_HEADER_BYTES if phys else 0)
    assert total == dst.size
    assert lay["state"][0] == HEADER_BYTES and lay["aux"][0] == HEADER_BYTES + 4 * SR * DB and lay["flags"][1] == (2, DB)
    if phys:
        assert lay["phys"][1] == (PHYS_ROWS, DB) and lay["phys"][0] + 4 * PHYS_ROWS * DB == dst.size
    d = np.array([4, 20, 0, 7, -1, 9, DB], dtype=np.int32)
    s = np.array([36, 3, 36, 5, 2, SB, 1], dtype=np.int32)      # a duplicated source; pairs 4, 5, 6 are out of range
    out = expected_blob(dst, src, d, s)
    sl, _ = blob_layout(src)
    good = [0, 1, 2, 3]
    rest = np.setdiff1d(np.arange(DB), d[good])
    for name, (_, _, _, axis) in lay.items():
        o, a, b = section(out, lay, name), section(dst, lay, name), section(src, sl, name)
        take = (lambda x, i: x[:, i]) if axis == 1 else (lambda x, i: x[i])
        assert np.array_equal(take(o, d[good]), take(b, s[good])), name
        assert np.array_equal(take(o, rest), take(a, rest)), name
    assert np.array_equal(out[:HEADER_BYTES], dst[:HEADER_BYTES])
    if phys:
        off = lay["phys"][0] - PHYS_HEADER_BYTES
        assert np.array_equal(out[off:off + PHYS_HEADER_BYTES], dst[off:off + PHYS_HEADER_BYTES])
    # identity on one blob is a no-op; a reversal applied twice gives the blob back (every read before every write)
    assert np.array_equal(expected_blob(dst, dst), dst)
    rev = np.arange(DB)[::-1]
    once = expected_blob(dst, dst, None, rev)
    assert not np.array_equal(once, dst) and np.array_equal(expected_blob(once, once, None, rev), dst)
    with pytest.raises(AssertionError):
        expected_blob(dst, src, [1, 1], [2, 3])
    if phys:
        with pytest.raises(AssertionError):
            expected_blob(dst, synthetic_blob(SB, SR, AR, OD, False, rng), [1], [2])
