"""The four newest features — per-env physics, trace evaluation, rendering, lookahead — on the handle shapes they had not run on.

  * padded rows (RSX_ROW_PAD: what every handle of 786 432 envs and more has by default): the physics block, rsx_trace_eval,
    rsx_render and rsx_task_lookahead each against a dense twin handle, bit for bit;
  * rsx_task_lookahead on handles whose scalar-arena rows were written by the one-lane-per-env and four-lanes-per-env stepping
    kernels, on the run-time-robot-count variants, with 16 lanes per env and with env_id_base != 0, each against checkpoint + restore
    + H x step (tests/test_gpu_lookahead.py: _reference)."""
import numpy as np
import pytest

from physics_helpers import NAMES, derive, random_params
from test_gpu_lookahead import _actions, _check, _host, _reference
from test_gpu_sysid import _random_trace

pytestmark = pytest.mark.gpu
B_PAD, PAD = 131, "200"   # rounded up to 256 floats (tests/test_gpu_rowpad.py)


@pytest.fixture(scope="module")
def L():
    from rsoccer_amd import _lib
    return _lib


def _twins(monkeypatch, make):
    """(dense, padded): the same construction without and with RSX_ROW_PAD (read when the handle is created)"""
    monkeypatch.delenv("RSX_ROW_PAD", raising=False)
    dense = make()
    monkeypatch.setenv("RSX_ROW_PAD", PAD)
    padded = make()
    monkeypatch.delenv("RSX_ROW_PAD", raising=False)
    sd, sp = getattr(dense, "sim", dense), getattr(padded, "sim", padded)
    assert sd._view.row_stride == B_PAD and sp._view.row_stride == B_PAD + 256
    return dense, padded


def _bits(t):
    import torch
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_run(torch, a, b, tag):
    torch.cuda.synchronize()
    assert torch.equal(_bits(a.state_tensor()), _bits(b.state_tensor())), (tag, "state")
    ta, tb = a.task_tensors(), b.task_tensors()
    for k in ("obs", "reward", "terminated", "truncated", "info", "steps", "final_obs"):
        assert torch.equal(_bits(ta[k]), _bits(tb[k])), (tag, k)


def _hetero(kind, B, seed):
    raw = random_params(kind, np.random.default_rng(seed), B)
    if kind == 1:
        raw[:, NAMES.index("a_lat")] = 0.0
    return raw


# ---- 5 (a): the physics block ----
@pytest.mark.parametrize("kind,ft,nb,ny,task", [(0, 0, 3, 3, 1), (1, 1, 11, 11, 7)], ids=["vss-v0", "crowded-11v11"])
def test_physics_block_with_padded_rows(L, monkeypatch, kind, ft, nb, ny, task):
    """rows [rows][S] of the parameter and coefficient blocks: phys_set_kernel's strides (host and device values, with and without a
    mask), load_coefs in the step kernels, the redraw, the checkpoint"""
    import torch
    B = B_PAD

    def make():
        s = L.Sim(kind, ft, nb, ny, 25, B)
        s.task_attach(task, 5, 0, 25)
        s.physics_enable()
        return s

    dense, padded = _twins(monkeypatch, make)
    want = np.tile(L.physics_defaults(kind), (B, 1))

    def check(tag):
        for s in (dense, padded):
            raw, coef = s.physics_get(L.PHYS_RAW), s.physics_get(L.PHYS_COEF)
            assert raw.T.tobytes() == want.tobytes(), (tag, "raw", s is padded)
            for e in range(B):
                assert coef[:, e].tobytes() == derive(kind, 25, want[e]).tobytes(), (tag, "coef", e, s is padded)

    check("defaults")
    rng = np.random.default_rng(8)
    v = _hetero(kind, B, 1)                                   # host values, every env
    want = v.copy()
    for s in (dense, padded):
        s.physics_set(v.T.copy())
    check("host")
    v, m = _hetero(kind, B, 2), (rng.random(B) < 0.5).astype(np.uint8)   # host values, masked, NaN = keep
    v[:, NAMES.index("mu_g")] = np.nan
    keep = want[:, NAMES.index("mu_g")].copy()
    want[m != 0] = v[m != 0]
    want[:, NAMES.index("mu_g")] = keep
    for s in (dense, padded):
        s.physics_set(v.T.copy(), m)
    check("host, masked")
    v = _hetero(kind, B, 3)                                   # device values, every env
    v[:, NAMES.index("e_rb")] = np.nan
    keep = want[:, NAMES.index("e_rb")].copy()
    want = v.copy()
    want[:, NAMES.index("e_rb")] = keep
    dv = torch.from_numpy(v.T.copy()).cuda()
    for s in (dense, padded):
        s.physics_set(dv)
    check("device")
    v, m = _hetero(kind, B, 4), (rng.random(B) < 0.5).astype(np.uint8)   # device values, masked; one env invalid: refused whole
    bad = int(np.flatnonzero(m)[3])
    v[bad, NAMES.index("e_wb")] = 1.5
    ok = (m != 0)
    ok[bad] = False
    want[ok] = v[ok]
    dv, dm = torch.from_numpy(v.T.copy()).cuda(), torch.from_numpy(m).cuda()
    for s in (dense, padded):
        s.physics_set(dv, dm)
        assert s.physics_errors() == 1
    check("device, masked")

    lo = np.zeros(len(NAMES), np.float32); hi = np.zeros(len(NAMES), np.float32)
    p = NAMES.index("mu_g"); lo[p], hi[p] = 0.2, 0.6
    for s in (dense, padded):
        s.physics_randomize(lo, hi, 1 << p)
        s.task_reset()
    td, tp = dense.task_tensors(), padded.task_tensors()
    for t in range(40):   # TimeLimit 25: a redraw in every env on the way
        a = torch.from_numpy(rng.uniform(-1, 1, tuple(td["actions"].shape)).astype(np.float32)).cuda()
        td["actions"].copy_(a); tp["actions"].copy_(a)
        dense.task_step(td["actions"].data_ptr()); padded.task_step(tp["actions"].data_ptr())
        _same_run(torch, dense, padded, t)
    assert dense.read_metrics()[1] >= B
    raws = [s.physics_get(L.PHYS_RAW) for s in (dense, padded)]
    assert raws[0].tobytes() == raws[1].tobytes() and len(np.unique(raws[0][p])) > B // 2
    assert dense.physics_get(L.PHYS_COEF).tobytes() == padded.physics_get(L.PHYS_COEF).tobytes()
    other = [q for q in range(len(NAMES)) if q != p]
    assert raws[1][other].T.tobytes() == want[:, other].tobytes()

    blob = padded.task_checkpoint()
    assert len(blob) == len(dense.task_checkpoint())
    for _ in range(7):
        dense.task_step(None)   # the dense handle moves on, then comes back through the padded handle's checkpoint
    dense.task_restore(blob)
    for s in (dense, padded):
        s.task_rollout(9)
        s.task_step_n(20)
    _same_run(torch, dense, padded, "after the checkpoint")
    assert dense.physics_get(L.PHYS_RAW).tobytes() == padded.physics_get(L.PHYS_RAW).tobytes()
    assert np.array_equal(dense.read_metrics(), padded.read_metrics())
    dense.close(); padded.close()


# ---- 5 (b): trace evaluation ----
@pytest.mark.parametrize("kind,ft,nb,ny", [(0, 0, 3, 3), (1, 0, 6, 6)], ids=["vss-3v3", "ssl-6v6"])
def test_trace_eval_with_padded_rows(L, monkeypatch, kind, ft, nb, ny):
    import torch
    B, H = B_PAD, 16
    tr = _random_trace(L, kind, ft, nb, ny, 30, seed=3 + nb)
    rows = _hetero(kind, B, 12)

    def make():
        s = L.Sim(kind, ft, nb, ny, 25, B)
        s.physics_enable()
        s.physics_set(rows.T.copy())
        s.trace_load(tr.frames, tr.cmds, np.array([5], dtype=np.int32))
        return s

    dense, padded = _twins(monkeypatch, make)
    out = []
    for s in (dense, padded):
        loss = torch.full((6, B), -1.0, dtype=torch.float32, device="cuda")
        s.trace_eval(H, loss)
        torch.cuda.synchronize()
        out.append((loss.cpu().numpy(), s.get_state_full()))
    assert (out[0][0] >= 0).all() and len(np.unique(out[0][0][0])) > B // 2   # every env its own physics, its own loss
    assert out[0][0].tobytes() == out[1][0].tobytes()
    assert out[0][1].tobytes() == out[1][1].tobytes()
    dense.close(); padded.close()


# ---- 5 (c): render ----
@pytest.mark.parametrize("name", ["VecVSSEnv", "VecSSLStaticDefendersEnv"])
def test_render_with_padded_rows(monkeypatch, name):
    import torch
    from rsoccer_amd import vec
    dense, padded = _twins(monkeypatch, lambda: getattr(vec, name)(B_PAD, device=0, seed=3))
    for env in (dense, padded):
        env.reset()
        env.step_random(25)
    ids = [130, 0, 77, 5, 77]
    for channels_first in (False, True):
        for env_ids in (None, ids):
            a = dense.render(env_ids, channels_first=channels_first)
            b = padded.render(env_ids, channels_first=channels_first)
            torch.cuda.synchronize()
            assert a.dtype == torch.uint8 and a.shape[0] == (B_PAD if env_ids is None else len(ids))
            assert torch.equal(a, b), (channels_first, env_ids)
            if env_ids is None:
                assert not torch.equal(a[0], a[1])   # frames show their own env
    assert padded.sim.render_errors() == 0
    dense.close(); padded.close()


# ---- 5 (d): lookahead ----
@pytest.mark.parametrize("name", ["VecVSSEnv", "VecSSLStaticDefendersEnv"])
def test_lookahead_with_padded_rows(monkeypatch, name):
    import torch
    from rsoccer_amd import vec
    dense, padded = _twins(monkeypatch, lambda: getattr(vec, name)(B_PAD, device=0, seed=9, max_episode_steps=34))
    for env in (dense, padded):
        _warm_up(torch, env, 25, 5)   # TimeLimit 34: the envs that never ended have 4 steps left, the re-started ones 29
    before = padded.checkpoint()
    acts = _actions(torch, dense, 3, 8, 5)
    got = _host(padded.lookahead(acts, gamma=0.97, return_obs=True))
    want = _host(dense.lookahead(acts, gamma=0.97, return_obs=True))
    assert (want["steps"] < 8).any() and (want["steps"] == 8).any()
    _check(got, want, name)
    torch.cuda.synchronize()
    assert np.array_equal(padded.checkpoint(), before)
    assert np.array_equal(before, dense.checkpoint())
    dense.close(); padded.close()


# ---- 6: lookahead on the handles it had not seen ----
class _SimEnv:
    """what _reference needs of an env, on a bare _lib.Sim handle"""

    def __init__(self, torch, sim):
        self._torch, self.sim, self.num_envs = torch, sim, sim.num_envs
        self.device = torch.device("cuda", 0)
        self._t = sim.task_tensors()

    def reset(self):
        self.sim.task_reset()

    def step_random(self, n):
        self.sim.task_step_n(n)

    def reset_to(self, ball, blue, yellow, env_mask=None):
        self.sim.task_reset_to(ball, blue, yellow, env_mask)

    def step(self, actions):
        self._keep = actions.contiguous()
        self.sim.task_step(self._keep.data_ptr())
        t = self._t
        return t["obs"], t["reward"], t["terminated"], t["truncated"], {"final_obs": t["final_obs"]}

    def checkpoint(self):
        return self.sim.task_checkpoint()

    def restore(self, blob):
        self.sim.task_restore(blob)

    def lookahead(self, actions, gamma=1.0, return_obs=False):
        torch, B, (K, H) = self._torch, self.num_envs, actions.shape[1:3]
        ret = torch.empty((B, K), dtype=torch.float32, device=self.device)
        steps = torch.empty((B, K), dtype=torch.int32, device=self.device)
        flags = torch.empty((B, K), dtype=torch.uint8, device=self.device)
        obs = torch.empty((B, K, self.sim.obs_dim), dtype=torch.float32, device=self.device)
        self.sim.task_lookahead(actions.data_ptr(), K, H, float(gamma), ret.data_ptr(), steps.data_ptr(), flags.data_ptr(), obs.data_ptr())
        return {"return": ret, "steps": steps, "terminated": (flags & 1).bool(), "truncated": (flags & 2).bool(), "last_obs": obs}

    def close(self):
        self.sim.close()


def _warm_up(torch, env, first, then):
    """`first` random steps, a new episode for every other env where it stands (masked reset_to), `then` more steps"""
    sim = env.sim
    env.reset()
    env.step_random(first)
    st = sim.get_state_full()
    rs, N, nb = (6 if sim.kind == 0 else 11), sim.n_robots, sim.n_blue
    rob = np.stack([st[:, 5 + rs * k: 8 + rs * k] for k in range(N)], 1)
    mask = (np.arange(sim.num_envs) % 2).astype(np.uint8)
    env.reset_to(st[:, [0, 1, 3, 4]], rob[:, :nb], rob[:, nb:], mask)
    env.step_random(then)
    torch.cuda.synchronize()
    steps = env._t["steps"].cpu().numpy()
    assert (steps[1::2] <= then).all() and (steps[0::2] > then).any()


LIMIT = 66   # TimeLimit of the lookahead cases: after the warm-up of 60 steps an env that never ended has 6 steps left


def _lookahead_parity(torch, env, tag, K=4, H=12):
    """warm-up of 60 steps by the handle's own stepping layout; after 52 of them every other env starts a new episode where it stands
    (masked reset_to), so that the batch holds envs 6 steps and 58 steps away from the TimeLimit: pairs that end inside the horizon
    next to pairs that run through it"""
    _warm_up(torch, env, 52, 8)
    acts = _actions(torch, env, K, H, 77)
    for gamma in (1.0, 0.97):
        got = _host(env.lookahead(acts, gamma=gamma, return_obs=True))
        want = _reference(torch, env, acts, gamma)
        ended = want["terminated"] | want["truncated"]
        print(f"{tag} gamma {gamma}: pairs ended inside the horizon {int(ended.sum())} of {ended.size}")
        assert ended.any() and not ended.all(), f"{tag}: uninformative, the reference saw no mix of ended and running pairs"
        _check(got, want, f"{tag} gamma {gamma}")


@pytest.mark.parametrize("name,layout,want", [
    ("VecSSLStaticDefendersEnv", "epl", "one-lane-per-env"), ("VecSSLDribblingEnv", "epl", "one-lane-per-env"),
    ("VecSSLContestedPossessionEnv", "epl", "one-lane-per-env"), ("VecSSLPassEnduranceEnv", "epl", "one-lane-per-env"),
    ("spread", "quad", "four-lanes-per-env"), ("crowded", "quad", "four-lanes-per-env")])
def test_lookahead_after_steps_of_the_large_batch_layouts(monkeypatch, name, layout, want):
    """ROW_STEPS, ROW_OU, ROW_INFO and ROW_PREV_POT as the one-lane-per-env and four-lanes-per-env kernels leave them"""
    import torch
    from rsoccer_amd import vec
    monkeypatch.setenv("RSX_LAYOUT", layout)
    if layout == "quad":
        env = vec.VecSSLScrimmageEnv(131, crowded=name == "crowded", device=0, seed=41, max_episode_steps=LIMIT)
    else:
        env = getattr(vec, name)(131, device=0, seed=41, max_episode_steps=LIMIT)
    assert env.sim.task_layout() == want
    _lookahead_parity(torch, env, f"{name} {layout}")
    env.close()


def _run_time_count(vec, name, B, **kw):
    if name == "vss-2v2":
        return type("VecVSS2v2Env", (vec.VecVSSEnv,), dict(N_BLUE=2, N_YELLOW=2))(B, **kw)
    if name == "static-defenders-1v4":
        return type("VecSD1v4Env", (vec.VecSSLStaticDefendersEnv,), dict(N_YELLOW=4))(B, **kw)
    if name == "scrimmage-3v2":
        return vec.VecSSLScrimmageEnv(B, n_blue=3, n_yellow=2, field_type=2, crowded=True, **kw)
    return vec.VecSSLScrimmageEnv(B, n_blue=8, n_yellow=8, field_type=1, crowded=True, **kw)   # 32 lanes per env, generic


@pytest.mark.parametrize("name", ["vss-2v2", "static-defenders-1v4", "scrimmage-3v2", "scrimmage-8v8"])
def test_lookahead_on_the_run_time_robot_count_variants(name):
    import torch
    from rsoccer_amd import vec
    env = _run_time_count(vec, name, 37, device=0, seed=23, max_episode_steps=LIMIT)
    _lookahead_parity(torch, env, name)
    env.close()


def test_lookahead_with_16_lanes_per_env(monkeypatch):
    import torch
    from rsoccer_amd import vec
    monkeypatch.setenv("RSX_LANES_PER_ENV", "16")
    env = vec.VecVSSEnv(37, device=0, seed=29, max_episode_steps=LIMIT)
    assert env.sim.task_layout() == "16-lanes-per-env"
    _lookahead_parity(torch, env, "VSS 3v3, 16 lanes")
    env.close()


def test_lookahead_with_a_global_env_id_base(L):
    """the OU draws of the other robots are keyed by env_id_base + env: the lookahead kernel has to add the base like the step kernel"""
    import torch
    sim = L.Sim(0, 0, 3, 3, 25, 37)
    sim.task_attach(1, 31, 5000, LIMIT)
    env = _SimEnv(torch, sim)
    _lookahead_parity(torch, env, "env_id_base 5000")
    other = L.Sim(0, 0, 3, 3, 25, 37)   # the base does matter: the same handle at base 0 moves differently
    other.task_attach(1, 31, 0, LIMIT)
    other.task_reset(); other.task_step_n(10)
    sim.task_reset(); sim.task_step_n(10)
    assert not np.array_equal(other.get_state_full(), sim.get_state_full())
    env.close(); other.close()
