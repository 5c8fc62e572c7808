"""Per-env physics parameters and on-device domain randomisation on the MI355X (include/rsx.h: rsx_physics_*).

  * a physics-enabled handle at its defaults steps bit for bit like a plain one (every fused task, single steps and rollouts,
    the raw simulator);
  * every env with its own random parameters equals, step for step and bit for bit, an f32 oracle env carrying the same
    coefficients (tests/physics_helpers.py);
  * closed forms with a different value in every env of one launch;
  * the redraw at episode starts is the documented Philox formula, independent of sharding;
  * checkpoints and graph replay carry the parameters."""
import numpy as np
import pytest

from physics_helpers import NAMES, derive, random_params, set_oracle_coefs

pytestmark = pytest.mark.gpu

# (kind, field, n_blue, n_yellow, task)
TASKS = [(0, 0, 3, 3, 1), (1, 2, 1, 6, 2), (1, 2, 1, 4, 3), (1, 2, 1, 1, 4), (1, 2, 2, 0, 5), (1, 1, 11, 11, 6)]


@pytest.fixture(scope="module")
def L():
    import os

    import __graft_entry__ as g
    if not os.path.exists(g.HIP_SO):
        g.build()
    from rsoccer_amd import _lib
    return _lib


def _pair(L, kind, field, nb, ny, task, B, seed=11, max_steps=0, env_id_base=0):
    out = []
    for phys in (False, True):
        s = L.Sim(kind, field, nb, ny, 25, B, 0)
        s.task_attach(task, seed, env_id_base, max_steps)
        if phys:
            s.physics_enable()
        out.append(s)
    return out


def _outputs(s):
    import torch
    torch.cuda.synchronize()
    t = s.task_tensors()
    return [s.get_state_full(), t["obs"].cpu().numpy(), t["reward"].cpu().numpy(), t["terminated"].cpu().numpy(),
            t["truncated"].cpu().numpy(), t["info"].cpu().numpy(), t["final_obs"].cpu().numpy(), t["steps"].cpu().numpy(),
            s.read_metrics()]


def _same(a, b):
    for x, y in zip(_outputs(a), _outputs(b)):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


@pytest.mark.parametrize("cfg", TASKS)
def test_defaults_step_bit_identically_to_the_literal_kernels(L, cfg):
    kind, field, nb, ny, task = cfg
    B = 256 if nb + ny < 22 else 64
    plain, phys = _pair(L, kind, field, nb, ny, task, B, max_steps=60)   # short episodes: auto-resets on the way
    assert phys.task_layout().endswith("lanes-per-env")
    for s in (plain, phys):
        s.task_reset()
    for _ in range(150):
        plain.task_step(None)
        phys.task_step(None)
    _same(plain, phys)
    for _ in range(3):
        plain.task_rollout(50)
        phys.task_rollout(50)
    _same(plain, phys)
    plain.close(); phys.close()


@pytest.mark.parametrize("kind,field,nb,ny", [(0, 0, 3, 3), (0, 1, 5, 5), (1, 2, 1, 6), (1, 1, 11, 11)])
def test_raw_simulator_defaults_bit_identical(L, kind, field, nb, ny):
    B = 128
    rng = np.random.default_rng(3)
    f = 0.6 if kind == 0 else 2.5
    ball = np.c_[rng.uniform(-f, f, (B, 2)), rng.uniform(-1, 1, (B, 2))]
    blue = np.dstack([rng.uniform(-f, f, (B, nb, 2)), rng.uniform(0, 360, (B, nb, 1))])
    yellow = np.dstack([rng.uniform(-f, f, (B, ny, 2)), rng.uniform(0, 360, (B, ny, 1))])
    sims = []
    for phys in (False, True):
        s = L.Sim(kind, field, nb, ny, 25, B, 0)
        if phys:
            s.physics_enable()
        s.reset(ball, blue, yellow)
        s.step_dev_random(300, seed=5)
        sims.append(s.get_state_full())
    assert sims[0].tobytes() == sims[1].tobytes()


def _hetero_check(L, oracle_mod, kind, field, nb, ny, task, B, n_steps, seed=21):
    rng = np.random.default_rng(B + task)
    raw = random_params(kind, rng, B)
    if kind == 1:
        raw[:, NAMES.index("a_lat")] = 0.0
    s = L.Sim(kind, field, nb, ny, 25, B, 0)
    s.task_attach(task, seed, 0, 0)
    s.physics_enable()
    s.physics_set(raw.T.copy())
    coef = s.physics_get(L.PHYS_COEF)
    s.task_reset()
    refs = []
    for e in range(B):
        r = oracle_mod.OracleEnv(kind, field, nb, ny, 25, "f32")
        r.task_attach(task, seed, e, 0)
        c = derive(kind, 25, raw[e])
        assert c.tobytes() == coef[:, e].tobytes()
        set_oracle_coefs(r, c)
        r.task_reset()
        refs.append(r)
    for step in range(n_steps):
        s.task_step(None)
        oracle_mod.vec_task_step(refs, 1)
        if step % 10 == 9 or step == n_steps - 1:
            st = s.get_state_full()
            obs = s.task_tensors()["obs"].cpu().numpy()
            for e, r in enumerate(refs):
                assert st[e].astype(np.float32).tobytes() == r.get_state_full().astype(np.float32).tobytes(), (step, e)
                assert obs[e].tobytes() == r.task_out()["obs"].astype(np.float32).tobytes(), (step, e)
    for r in refs:
        r.close()
    s.close()


@pytest.mark.parametrize("B", [1, 37, 4096])
def test_heterogeneous_physics_matches_the_oracle_vss(L, oracle_mod, B):
    _hetero_check(L, oracle_mod, 0, 0, 3, 3, 1, B, 100 if B < 4096 else 30)


@pytest.mark.parametrize("B", [1, 37, 4096])
def test_heterogeneous_physics_matches_the_oracle_static_defenders(L, oracle_mod, B):
    _hetero_check(L, oracle_mod, 1, 2, 1, 6, 2, B, 100 if B < 4096 else 30)


def test_heterogeneous_physics_matches_the_oracle_crowded_11v11(L, oracle_mod):
    _hetero_check(L, oracle_mod, 1, 1, 11, 11, 7, 37, 40)


def test_rolling_stop_distance_per_env(L):
    """a ball rolling alone stops after v^2 / (2 mu_g) (up to the per-step discretisation), each env with its own mu_g"""
    B = 64
    s = L.Sim(0, 0, 1, 0, 25, B, 0)
    s.physics_enable()
    mu = np.linspace(0.1, 1.0, B).astype(np.float32)
    vals = np.full((len(NAMES), B), np.nan, dtype=np.float32)
    vals[NAMES.index("mu_g")] = mu
    s.physics_set(vals)
    v0 = 0.3   # stops within 0.45 m: inside the field for every mu_g
    ball = np.tile([-0.6, 0.0, v0, 0.0], (B, 1))
    blue = np.tile([0.0, 0.6, 0.0], (B, 1, 1))
    s.reset(ball, blue, np.zeros((B, 0, 3)))
    for _ in range(200):
        s.step(np.zeros((B, 1, 2)))
    x = s.get_state()[:, 0]
    dt = 0.025
    # per step the speed drops by mu_g dt (applied before the step's motion): distance = dt * sum_k (v0 - k mu dt)
    n = np.floor(v0 / (mu * dt)).astype(int)
    want = -0.6 + dt * (n * v0 - mu * dt * n * (n + 1) / 2)
    assert np.allclose(x, want, atol=2e-4), np.c_[x, want][:5]
    assert np.allclose(x + 0.6, v0 ** 2 / (2 * mu), rtol=0.1)


def test_two_body_impulse_with_per_env_masses_and_restitution(L):
    """a ball hitting the back of a resting SSL robot: v' = v (1 - (1 + e_rb) w_b), w_b = (1/m_b) / (1/m_r + 1/m_b), per env"""
    B = 32
    s = L.Sim(1, 0, 1, 0, 25, B, 0)
    s.physics_enable()
    rng = np.random.default_rng(1)
    vals = np.full((len(NAMES), B), np.nan, dtype=np.float32)
    vals[NAMES.index("m_robot")] = rng.uniform(1.0, 4.0, B)
    vals[NAMES.index("m_ball")] = rng.uniform(0.03, 0.08, B)
    vals[NAMES.index("e_rb")] = rng.uniform(0.2, 0.9, B)   # the ball clearly bounces back (no second contact)
    vals[NAMES.index("mu_rb")] = 0.0
    vals[NAMES.index("mu_g")] = 0.0
    s.physics_set(vals)
    s.reset(np.tile([-0.4, 0.0, 2.0, 0.0], (B, 1)), np.tile([0.0, 0.0, 0.0], (B, 1, 1)), np.zeros((B, 0, 3)))
    v_out = np.full(B, np.nan)
    prev = s.get_state()[:, 3].copy()
    for _ in range(30):
        s.step(np.zeros((B, 1, 8)))
        cur = s.get_state()[:, 3]
        hit = (prev > 0) & (cur < 1.9) & np.isnan(v_out)
        v_out[hit] = cur[hit]
        prev = cur.copy()
    w_b = (1 / vals[1]) / (1 / vals[0] + 1 / vals[1])
    want = 2.0 * (1.0 - (1.0 + vals[3]) * w_b)
    assert np.allclose(v_out, want, atol=4e-3), np.c_[v_out, want][:5]


def test_wall_rebound_and_acceleration_ramp_per_env(L):
    B = 32
    s = L.Sim(0, 0, 1, 0, 25, B, 0)
    s.physics_enable()
    e = np.linspace(0.0, 1.0, B).astype(np.float32)
    a = np.linspace(1.0, 16.0, B).astype(np.float32)
    vals = np.full((len(NAMES), B), np.nan, dtype=np.float32)
    vals[NAMES.index("e_wb")] = e
    vals[NAMES.index("mu_wb")] = 0.0
    vals[NAMES.index("mu_g")] = 0.0
    vals[NAMES.index("a_lin")] = a
    s.physics_set(vals)
    # ball towards the +y wall (no goal there), robot at rest facing +x commanded to full wheel speed
    s.reset(np.tile([0.2, 0.55, 0.0, 1.0], (B, 1)), np.tile([-0.4, -0.3, 0.0], (B, 1, 1)), np.zeros((B, 0, 3)))
    cmd = np.full((B, 1, 2), 20.0)
    s.step(cmd)
    st = s.get_state()
    # one step = 5 sub-steps of 5 ms: the robot's forward speed grows by a_lin h per sub-step (targets far above)
    assert np.allclose(st[:, 8], np.minimum(a * 0.025, 20.0 * 0.026), atol=1e-5), np.c_[st[:, 8], a * 0.025][:5]
    for _ in range(10):
        s.step(cmd)
    vy = s.get_state()[:, 4]
    assert np.allclose(vy, -e * 1.0, atol=1e-5), np.c_[vy, -e][:5]


def _expected_draw(oracle_mod, seed, env_id, episode, p, lo, hi):
    x = oracle_mod.philox([env_id, episode, p, 5], [seed & 0xFFFFFFFF, seed >> 32], rounds=7)[0]
    u = np.float32((x >> 8) * 5.9604644775390625e-08)
    return np.float32(np.float32(lo) + (np.float32(hi) - np.float32(lo)) * u)


def test_randomisation_follows_the_philox_formula(L, oracle_mod):
    B, seed = 64, 1234
    ranges = {"m_ball": (0.04, 0.05), "mu_g": (0.2, 0.4), "e_wb": (0.3, 0.9), "a_lin": (6.0, 10.0)}
    lo = np.zeros(len(NAMES), np.float32); hi = np.zeros(len(NAMES), np.float32); mask = 0
    for k, (a, b) in ranges.items():
        i = NAMES.index(k); lo[i], hi[i] = a, b; mask |= 1 << i
    shards = []
    for base, n in ((0, B), (0, B // 2), (B // 2, B // 2)):
        s = L.Sim(0, 0, 3, 3, 25, n, 0)
        s.task_attach(1, seed, base, 20)
        s.physics_enable()
        s.physics_randomize(lo, hi, mask)
        s.task_reset()
        shards.append(s)
    def check(s, base, n, episode):
        raw = s.physics_get(L.PHYS_RAW)
        coef = s.physics_get(L.PHYS_COEF)
        d = L.physics_defaults(0)
        for e in range(n):
            want = d.copy()
            for k in ranges:
                i = NAMES.index(k)
                want[i] = _expected_draw(oracle_mod, seed, base + e, episode, i, lo[i], hi[i])
            assert raw[:, e].tobytes() == want.tobytes(), e
            assert coef[:, e].tobytes() == derive(0, 25, want).tobytes(), e
    check(shards[0], 0, B, 0)
    for s in shards:
        s.task_step_n(20)   # every episode ends by step 20 (TimeLimit 20): the auto-reset redraws
    steps = shards[0].task_tensors()["steps"].cpu().numpy()
    assert (steps == 0).all()
    check(shards[0], 0, B, 1)
    whole = shards[0].physics_get(L.PHYS_RAW)
    halves = np.concatenate([shards[1].physics_get(L.PHYS_RAW), shards[2].physics_get(L.PHYS_RAW)], axis=1)
    assert whole.tobytes() == halves.tobytes()
    for s in shards:
        s.close()


def test_vec_env_surface_and_device_tensors(L):
    import torch

    import rsoccer_amd
    env = rsoccer_amd.make_vec("VSS-v0", 16, physics={"m_ball": 0.05}, physics_ranges={"mu_g": (0.2, 0.3)})
    env.reset()
    p = env.physics()
    assert set(p) == set(NAMES)
    assert torch.all(p["m_ball"] == np.float32(0.05))
    assert torch.all((p["mu_g"] >= 0.2) & (p["mu_g"] <= 0.3))
    env.set_physics(env_ids=[1, 3], m_robot=torch.tensor([0.2, 0.25], device=env.device))
    env.set_physics(a_lin=np.arange(16, dtype=np.float32) + 1)
    p = env.physics()
    assert p["m_robot"][1].item() == np.float32(0.2) and p["m_robot"][3].item() == np.float32(0.25)
    assert p["m_robot"][0].item() == np.float32(0.18)
    env.set_physics(env_ids=[2], e_rb=torch.tensor([2.0], device=env.device))   # invalid on the device: refused, counted
    assert env.sim.physics_errors() == 1 and env.physics()["e_rb"][2].item() == np.float32(0.3)
    with pytest.raises(L.RsxError):
        env.set_physics(e_rb=1.5)
    env.set_physics_randomization(mu_g=None)
    env.step()
    plain = rsoccer_amd.make_vec("VSS-v0", 16)
    assert plain.sim.task_layout() == env.sim.task_layout()
    with pytest.raises(RuntimeError):
        plain.set_physics(m_ball=0.05)


def test_checkpoint_carries_the_parameters(L):
    B = 64
    lo = np.zeros(len(NAMES), np.float32); hi = np.zeros(len(NAMES), np.float32)
    i = NAMES.index("m_robot"); lo[i], hi[i] = 0.15, 0.25
    def make():
        s = L.Sim(0, 0, 3, 3, 25, B, 0)
        s.task_attach(1, 9, 0, 30)
        s.physics_enable()
        return s
    a = make()
    a.physics_randomize(lo, hi, 1 << i)
    a.task_reset()
    a.task_step_n(17)
    blob = a.task_checkpoint()
    b = make()
    b.task_restore(blob)
    for s in (a, b):
        s.task_step_n(40)
    _same(a, b)
    assert a.physics_get(L.PHYS_RAW).tobytes() == b.physics_get(L.PHYS_RAW).tobytes()
    plain = L.Sim(0, 0, 3, 3, 25, B, 0)
    plain.task_attach(1, 9, 0, 30)
    with pytest.raises(L.RsxError):
        plain.task_restore(blob)
    with pytest.raises(L.RsxError):
        b.task_restore(plain.task_checkpoint())


def test_graph_replay_sees_values_set_between_replays(L):
    import torch
    B = 64
    sims = []
    for _ in range(2):
        s = L.Sim(0, 0, 3, 3, 25, B, 0)
        s.task_attach(1, 4, 0, 0)
        s.physics_enable()
        sims.append(s)
    g_sim, e_sim = sims
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for s in sims:
            s.task_enable_capture(stream.cuda_stream)
            s.task_reset(stream.cuda_stream)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            g_sim.task_step(None, stream.cuda_stream)
        vals = np.full((len(NAMES), B), np.nan, dtype=np.float32)
        for k in range(6):
            vals[NAMES.index("mu_g")] = 0.1 + 0.1 * k
            vals[NAMES.index("e_rb")] = 0.1 * k
            for s in sims:
                s.physics_set(vals, stream=stream.cuda_stream)
            if k == 3:
                lo = np.zeros(len(NAMES), np.float32); hi = np.zeros(len(NAMES), np.float32)
                lo[1], hi[1] = 0.03, 0.06
                for s in sims:
                    s.physics_randomize(lo, hi, 2, stream.cuda_stream)
            for _ in range(5):
                g.replay()
                e_sim.task_step(None, stream.cuda_stream)
        stream.synchronize()
    _same(g_sim, e_sim)


def test_soak_under_randomisation(L):
    """+-30 % on every parameter (restitutions clipped to 1): finite, inside the walls, overlaps bounded"""
    for kind, field, nb, ny, task, B in ((0, 0, 3, 3, 1, 4096), (1, 2, 1, 6, 2, 2048)):
        d = L.physics_defaults(kind)
        lo, hi = (d * 0.7).astype(np.float32), np.minimum(d * 1.3, [1 if 2 <= i <= 5 else np.inf for i in range(len(NAMES))]).astype(np.float32)
        s = L.Sim(kind, field, nb, ny, 25, B, 0)
        s.task_attach(task, 77, 0, 0)
        s.physics_enable()
        s.physics_randomize(lo, hi, (1 << len(NAMES)) - 1 if kind == 0 else (1 << (len(NAMES) - 1)) - 1)
        s.task_reset()
        worst = 0.0
        for _ in range(20):
            s.task_rollout(100)
            st = s.get_state_full()
            assert np.isfinite(st).all()
            f = s.get_field_params()
            rs = 6 if kind == 0 else 11
            r = f["rbt_radius"]
            xs = np.stack([st[:, 5 + rs * k] for k in range(nb + ny)], 1)
            ys = np.stack([st[:, 6 + rs * k] for k in range(nb + ny)], 1)
            assert (np.abs(ys) <= f["width"] / 2 + (0.3 if kind else 0) - r + 1e-4).all()
            assert (np.abs(xs) <= f["length"] / 2 + f["goal_depth"] + (0.3 if kind else 0)).all()
            dx = xs[:, :, None] - xs[:, None, :]
            dy = ys[:, :, None] - ys[:, None, :]
            d2 = np.sqrt(dx * dx + dy * dy) + np.eye(nb + ny)[None] * 10
            worst = max(worst, float((2 * r - d2).max()))
        print(f"kind {kind}: worst robot-robot overlap {worst * 1000:.2f} mm")
        assert worst < 0.02
        s.close()
