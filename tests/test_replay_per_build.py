"""Prioritised and n-step replay (rsx_replay_add_nstep, rsx_replay_tree_geometry, rsx_replay_set_priorities,
rsx_replay_sample_prioritized, rsx_task_dpg_gradient_w, rsx_task_sac_gradient_w) as a build product, no GPU: the symbols are declared,
listed and exported, the C structs and their ctypes mirrors agree member for member, the unit is one of build()'s with
rsx_dpg_update.hip's flags, none of its kernels uses scratch memory, it names no atomic on floats, its draw's domain word is 14 and
escapes both existing domain scans; and the Python layer refuses invalid arguments by name before anything touches a device."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW = ("rsx_replay_add_nstep", "rsx_replay_tree_geometry", "rsx_replay_set_priorities", "rsx_replay_sample_prioritized",
       "rsx_task_dpg_gradient_w", "rsx_task_sac_gradient_w")
KERNELS = ("replay_add_nstep_kernel", "replay_leaf_kernel", "replay_node_kernel", "replay_draw_kernel", "replay_weights_kernel",
           "replay_td_error_kernel")
UNIT = "rsx_replay.hip"


def _header():
    return open(os.path.join(ROOT, "include", "rsx.h")).read()


def _members(header, name):
    """[(type, name)] of a typedef'd struct, comments dropped"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(re.sub(r"\s+", " ", t.strip()), n) for t, n in re.findall(r"([\w\s\*]+?)\s*\b(\w+)\s*;", body)]


def test_symbols_are_declared_listed_and_exported():
    from build_variant import dynamic_symbols
    from rsoccer_amd import _lib
    header = _header()
    defined, _ = dynamic_symbols(_lib.LIB_PATH)
    for sym in NEW:
        assert re.search(r"^int %s\(" % sym, header, re.M), sym
        assert sym in _lib.SYMBOLS and sym in defined, sym
    from rsoccer_amd.vec.replay import PrioritizedReplayBuffer, ReplayBuffer
    assert issubclass(PrioritizedReplayBuffer, ReplayBuffer)
    for f in (PrioritizedReplayBuffer.add, PrioritizedReplayBuffer.sample, PrioritizedReplayBuffer.update_priorities,
              PrioritizedReplayBuffer.priorities, PrioritizedReplayBuffer.data, PrioritizedReplayBuffer.sample_rows,
              PrioritizedReplayBuffer.sample_rows_device, _lib.replay_add_nstep, _lib.replay_tree_geometry, _lib.replay_set_priorities,
              _lib.replay_sample_prioritized, _lib.Sim.task_dpg_gradient_w, _lib.Sim.task_sac_gradient_w):
        assert callable(f)
    assert PrioritizedReplayBuffer.sample_rows is ReplayBuffer.sample_rows   # the uniform draws are the base class's own


def test_structs_agree_with_their_ctypes_mirrors_and_the_abi_stays_6():
    from rsoccer_amd import _lib
    header = _header()
    ctype_of = {"const float*": C.c_void_p, "float*": C.c_void_p, "int64_t*": C.c_void_p, "int32_t*": C.c_void_p, "uint8_t*": C.c_void_p,
                "const uint8_t*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32}
    want = {"rsx_replay_batch": ["obs", "actions", "reward", "terminated", "truncated", "final_obs", "next_obs", "T", "B"],
            "rsx_replay_ring": ["obs", "actions", "reward", "next_obs", "terminated", "discount", "head_dev", "fill_dev", "ticket_dev",
                                "capacity", "obs_dim", "act_dim"],
            "rsx_grad_per": ["discount", "weight", "td_error"]}
    for name, cls in (("rsx_replay_batch", _lib.ReplayBatch), ("rsx_replay_ring", _lib.ReplayRing), ("rsx_grad_per", _lib.GradPer)):
        members = _members(header, name)
        assert [n for _, n in members] == [f[0] for f in cls._fields_] == want[name], name
        assert [ctype_of[t] for t, _ in members] == [f[1] for f in cls._fields_], name
    assert (C.sizeof(_lib.ReplayBatch), C.sizeof(_lib.ReplayRing), C.sizeof(_lib.GradPer)) == (64, 88, 24)
    for k, name in enumerate(_lib.REPLAY_STATE):
        assert re.search(r"^#define RSX_REPLAY_STATE_%s\s+%d\b" % (name.upper(), k), header, re.M), name
    assert re.search(r"^#define RSX_REPLAY_STATE_WORDS\s+%d\b" % len(_lib.REPLAY_STATE), header, re.M)
    assert re.search(r"^#define RSX_ABI_VERSION 6\b", header, re.M)
    # the structs the existing entry points take keep their layout (the existing build tests pin the members; the sizes here)
    assert (C.sizeof(_lib.DpgIn), C.sizeof(_lib.DpgCfg), C.sizeof(_lib.DpgOut), C.sizeof(_lib.SacCfg), C.sizeof(_lib.SacOut)) == (64, 48, 64, 48, 112)


def test_the_unit_is_one_of_build_with_the_flags_of_the_dpg_update_unit_and_restates_no_philox():
    from __graft_entry__ import CSRC, HIP_UNITS
    units_of = dict(HIP_UNITS)
    assert UNIT in units_of and units_of[UNIT] == units_of["rsx_dpg_update.hip"]
    text = open(os.path.join(CSRC, UNIT)).read()
    assert '#include "rsx_math.hpp"' in text and "philox4x32(uint32_t" not in text and "0xD2511F53" not in text
    units = open(os.path.join(CSRC, "rsx_units.hpp")).read()
    for fn in ("void launch_replay_add_nstep(", "void launch_replay_set_priorities(", "hipError_t launch_replay_sample_prioritized(",
               "void launch_replay_td_error(", "void replay_tree_geometry("):
        assert fn in units and fn.split()[-1] in text, fn
    # the gradient units gained no kernel and no instantiation for the weighted calls: run-time pointers in the existing kernels
    for name, kernels in (("rsx_dpg.hip", 4), ("rsx_sac.hip", 6)):
        code = open(os.path.join(CSRC, name)).read()
        assert len(re.findall(r"\b__global__\b", code)) == kernels, name
        assert "G.discount != nullptr ? G.discount[e.idx] : G.gamma" in code and "(diff * w) * G.inv_m" in code, name


def test_the_unit_names_no_atomic_on_floats():
    """its atomics are integer ones: a maximum of bit patterns (uint32_t) and two int counters"""
    from __graft_entry__ import CSRC
    text = open(os.path.join(CSRC, UNIT)).read()
    code = re.sub(r"//[^\n]*", "", text)
    calls = re.findall(r"\b(atomic\w+)\s*\(([^;]*);", code)
    assert calls and {name for name, _ in calls} <= {"atomicMax", "atomicAdd"}
    for name, args in calls:
        first = args.split(",")[0]
        assert "float*" not in first and "double" not in first, (name, args)
        if name == "atomicMax":
            assert "__float_as_uint(" in args and ("uint32_t*" in first or "A.state" in first), args
        else:
            assert "int*" in first or "ticket_dev" in first, args
    assert not re.search(r"atomic\w*(?:_f32|_f64|Float|Double)|unsafeAtomic|__hip_atomic", code)


def test_the_draws_domain_word_is_14_and_escapes_both_existing_scans():
    from __graft_entry__ import CSRC
    text = open(os.path.join(CSRC, UNIT)).read()
    assert re.search(r"constexpr uint32_t PER_DRAW_WORD = 14u;", text)
    assert "PER_DRAW_WORD, A.k0, A.k1" in text
    # the two scans of the existing build tests, word for word, find nothing in this unit
    assert not re.findall(r"constexpr uint32_t (?:DOM_\w+ = \d+u(?:, )?)+", text)
    assert not re.findall(r"constexpr uint32_t (?:(?:DOM|SAC_DRAW)_\w+ = \d+u(?:, )?)+", text)
    header = _header()
    assert "counter = (t >> 2, step >> 32, step & 0xFFFFFFFF, 14)" in header and "14 (1 and 3 .. 13 are taken)" in header
    import per_helpers as PH
    assert PH.PER_DRAW_WORD == 14


def test_no_kernel_uses_scratch_memory():
    """compiled with the flags build() gives the unit; the compiler's kernel-resource-usage remarks, read the way
    tests/test_dpg_update_build.py reads them"""
    from __graft_entry__ import CSRC, HIPCC_COMMON, HIP_UNITS
    work = tempfile.mkdtemp(prefix="rsx_replay_probe_")
    try:
        p = subprocess.run([os.environ.get("HIPCC", "hipcc")] + HIPCC_COMMON + dict(HIP_UNITS)[UNIT] +
                           ["-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(work, "rsx_replay.o"),
                            os.path.join(CSRC, UNIT)], stderr=subprocess.PIPE, text=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[.*?\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    for kernel in KERNELS:
        hits = [k for k in rows if kernel in k]
        assert len(hits) == 1, (kernel, sorted(rows))
        v = rows[hits[0]]
        print(kernel, {n: v.get(n) for n in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "Occupancy", "LDS Size")})
        assert v["ScratchSize"] == 0, (kernel, v)
    assert len(rows) == len(KERNELS), sorted(rows)


# ---- the Python layer's refusals that need no device ----
@pytest.mark.parametrize("kw,word", [
    (dict(alpha=-0.1), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(alpha=float("inf")), "alpha"),
    (dict(n_step=0), "n_step"), (dict(n_step=17), "n_step"), (dict(n_step=2.5), "n_step"),
    (dict(gamma=1.01), "gamma"), (dict(gamma=-0.1), "gamma"), (dict(gamma=float("nan")), "gamma"),
    (dict(eps=-1e-6), "eps"), (dict(eps=float("nan")), "eps"),
    (dict(capacity=2 ** 31), "capacity"), (dict(capacity=0), "capacity"),
])
def test_the_buffer_refuses_invalid_hyper_parameters_before_it_allocates(kw, word):
    from rsoccer_amd.vec.replay import PrioritizedReplayBuffer
    kw = {"capacity": 16, **kw}
    with pytest.raises(ValueError, match=re.escape(word)):
        PrioritizedReplayBuffer(kw.pop("capacity"), 4, 2, "cuda:0", **kw)


def test_the_buffer_refuses_a_cpu_device_by_name_and_the_base_class_is_untouched():
    from rsoccer_amd.vec.replay import PrioritizedReplayBuffer, ReplayBuffer
    with pytest.raises(ValueError, match="device must be a GPU"):
        PrioritizedReplayBuffer(16, 4, 2, "cpu")
    buf = ReplayBuffer(16, 4, 2, "cpu")
    assert sorted(buf.data()) == ["actions", "next_obs", "obs", "reward", "terminated"] and not hasattr(buf, "discount")


def test_the_gradient_calls_take_the_new_arguments_with_defaults_that_change_nothing():
    import inspect
    from rsoccer_amd.vec.fused import VecFusedEnv
    for f in (VecFusedEnv.dpg_gradient, VecFusedEnv.sac_gradient):
        sig = inspect.signature(f).parameters
        assert sig["weights"].default is None and sig["return_td_error"].default is False
        assert "gamma`` then only validates" in re.sub(r"\s+", " ", f.__doc__)
