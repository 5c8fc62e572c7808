"""The paired form of the VSS-v0 3v3 single step (rsoccer_amd/csrc/rsx_pair.hpp: a physics wave and a service wave per workgroup,
RSX_SERVICE_WAVE=1) against the CPU oracle and against the unpaired kernel on a second handle (RSX_SERVICE_WAVE=0), bit for bit after
every step: observations, rewards, flags, info rows, terminal observations, step counts, the full state and the folded metrics.

Batches: 8 envs (one full tile), 9 (a second tile with seven dead env slots — its waves still meet at both barriers) and 72."""
import numpy as np
import pytest

from helpers import f32_equal, mismatch_report

pytestmark = pytest.mark.gpu

BATCHES = (8, 9, 72)
KEYS = ("obs", "reward", "terminated", "truncated", "info", "final_obs", "steps")


def _handles(monkeypatch, oracle_mod, B, seed, max_steps):
    """(paired handle, unpaired handle, one oracle env per env id), all reset"""
    from rsoccer_amd import _lib as L
    sims = []
    for on in ("1", "0"):
        monkeypatch.setenv("RSX_SERVICE_WAVE", on)   # read by rsx_task_attach
        sim = L.Sim(0, 0, 3, 3, 25, B)
        sim.task_attach(1, seed, 0, max_steps)
        assert sim.task_layout() == "8-lanes-per-env"
        assert sim.task_service_wave() == (on == "1")   # the plan the dispatch reads: the "1" handle runs task_pair_step_kernel
        sim.task_reset()
        sims.append(sim)
    refs = [oracle_mod.OracleEnv(0, 0, 3, 3, 25, "f32") for _ in range(B)]
    for e, r in enumerate(refs):
        r.task_attach(1, seed, e, max_steps)
        r.task_reset()
    return sims[0], sims[1], refs


def _snapshot(sim):
    import torch
    torch.cuda.synchronize()
    t = sim.task_tensors()
    out = {k: t[k].cpu().numpy().copy() for k in KEYS}
    out["state"] = np.ascontiguousarray(sim.get_state_full(), dtype=np.float32)
    out["metrics"] = np.asarray(sim.read_metrics()).copy()   # folds the per-workgroup partial sums first
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _check(paired, plain, refs, what):
    a, b = _snapshot(paired), _snapshot(plain)
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs between the paired and the unpaired kernel"
    for e, r in enumerate(refs):
        o = r.task_out()
        assert f32_equal(a["obs"][e], o["obs"]), mismatch_report(a["obs"][e], o["obs"], f"{what}: obs env {e}")
        assert f32_equal(a["reward"][e], o["reward"]), f"{what}: reward env {e}: {a['reward'][e]} vs {o['reward']}"
        assert a["terminated"][e] == o["terminated"] and a["truncated"][e] == o["truncated"], f"{what}: flags env {e}"
        assert f32_equal(a["info"][:, e], o["info"]), mismatch_report(a["info"][:, e], o["info"], f"{what}: info env {e}")
        assert a["steps"][e] == o["steps"], f"{what}: steps env {e}"
        if o["terminated"] or o["truncated"]:
            assert f32_equal(a["final_obs"][e], o["final_obs"]), f"{what}: final_obs env {e}"
        w = r.get_state_full()
        assert f32_equal(a["state"][e], w), mismatch_report(a["state"][e], w, f"{what}: state env {e}")
    want = sum(r.task_out()["metrics"] for r in refs)
    assert np.array_equal(a["metrics"], want), f"{what}: metrics {a['metrics']} vs {want}"
    return a


@pytest.mark.parametrize("B", BATCHES)
def test_random_action_steps_with_short_episodes(oracle_mod, monkeypatch, B):
    """max_episode_steps = 3: a truncation, a terminal observation, a placement and the episode counters in every third launch"""
    paired, plain, refs = _handles(monkeypatch, oracle_mod, B, 11, 3)
    ends = 0
    for t in range(40):
        paired.task_step(None); plain.task_step(None)
        for r in refs:
            r.task_step(None)
        ends += int(_check(paired, plain, refs, f"step {t}")["truncated"].sum())
    assert ends >= 12 * B   # (13 per env unless a goal cut an episode short)
    paired.close(); plain.close()


@pytest.mark.parametrize("B", BATCHES)
def test_caller_fed_actions(oracle_mod, monkeypatch, B):
    import torch
    paired, plain, refs = _handles(monkeypatch, oracle_mod, B, 12, 25)
    rng = np.random.default_rng(3)
    bufs = [s.task_tensors()["actions"] for s in (paired, plain)]
    for t in range(40):
        a = rng.uniform(-1, 1, (B, 2)).astype(np.float32)
        for s, buf in zip((paired, plain), bufs):
            buf.copy_(torch.from_numpy(a))
            s.task_step(buf.data_ptr())
        for e, r in enumerate(refs):
            r.task_step(a[e])
        _check(paired, plain, refs, f"step {t}")
    paired.close(); plain.close()


@pytest.mark.parametrize("B", BATCHES)
def test_goals_for_and_against(oracle_mod, monkeypatch, B):
    """The ball one sub-step short of a goal line and moving out: the physics wave decides the termination (terminal observation,
    placement), the service wave adds the goal counters.  Every third env keeps its ball in midfield."""
    paired, plain, refs = _handles(monkeypatch, oracle_mod, B, 13, 50)
    ball = np.zeros((B, 4)); rob = np.zeros((B, 6, 3))
    for e in range(B):
        side = (1.0, -1.0, 0.0)[e % 3]
        ball[e] = (side * 0.7475, 0.01 * (e % 5) - 0.02, side * 1.0, 0.0) if side else (0.0, 0.05, 0.1, 0.0)
        for k in range(6):
            rob[e, k] = ((-0.4, 0.4)[k // 3], -0.4 + 0.4 * (k % 3), 30.0 * k)
    ball = np.float32(ball).astype(np.float64); rob = np.float32(rob).astype(np.float64)   # the float state holds the same bits
    for s in (paired, plain):
        s.task_reset_to(ball, rob[:, :3], rob[:, 3:])
    for e, r in enumerate(refs):
        r.task_reset_to(ball[e], rob[e, :3], rob[e, 3:])
    first = None
    for t in range(4):
        paired.task_step(None); plain.task_step(None)
        for r in refs:
            r.task_step(None)
        snap = _check(paired, plain, refs, f"step {t}")
        first = first or snap
    scored = np.arange(B) % 3 != 2
    assert np.array_equal(first["terminated"] != 0, scored)
    assert np.array_equal(first["reward"][scored], np.where(np.arange(B)[scored] % 3 == 0, 10.0, -10.0).astype(np.float32))
    assert first["metrics"][2] == (np.arange(B) % 3 == 0).sum() and first["metrics"][3] == (np.arange(B) % 3 == 1).sum()
    paired.close(); plain.close()


@pytest.mark.parametrize("B", BATCHES)
def test_device_keyed_handle_stepped_eagerly(oracle_mod, monkeypatch, B):
    """rsx_task_enable_capture: the physics wave reads and advances the workgroup's step-counter slot and hands the tick to the service wave"""
    paired, plain, refs = _handles(monkeypatch, oracle_mod, B, 14, 4)
    for s in (paired, plain):
        s.task_step(None)
        s.task_enable_capture()
    for r in refs:
        r.task_step(None)
    for t in range(10):
        paired.task_step(None); plain.task_step(None)
        for r in refs:
            r.task_step(None)
        _check(paired, plain, refs, f"step {t}")
    assert paired.task_tick() == 11 and plain.task_tick() == 11
    paired.close(); plain.close()
