"""Trace evaluation and fitting on the MI355X (include/rsx.h: rsx_trace_load / rsx_trace_eval; rsoccer_amd/sysid.py).

  * after one trace_eval launch every env's state equals, bit for bit, `horizon` step_dev calls from the same anchor with the
    same per-env parameters, and the loss equals a torch computation from those states and the f32-oracle restatement;
  * a trace recorded from rsoccer_amd.robosim scores exactly 0 at the defaults;
  * a seeded perturbed parameter set is recovered from the deck recorded by the f32 oracle carrying it, with and without noise;
  * the fitted values go into make_vec(..., physics=...) as they are; every refusal of the C-ABI."""
import numpy as np
import pytest

from physics_helpers import NAMES, random_params
from sysid_helpers import oracle_loss, oracle_module, params_vector

pytestmark = pytest.mark.gpu

# (kind, field, n_blue, n_yellow): VSS 3v3 (8 lanes), VSS 5v5 (16), SSL 1v6 (8), SSL 6v6 (16), SSL 11v11 (32)
CONFIGS = [(0, 0, 3, 3), (0, 1, 5, 5), (1, 2, 1, 6), (1, 0, 6, 6), (1, 1, 11, 11)]


@pytest.fixture(scope="module")
def L():
    import os

    import __graft_entry__ as g
    if not os.path.exists(g.HIP_SO):
        g.build()
    from rsoccer_amd import _lib
    return _lib


def _random_trace(L, kind, field, nb, ny, T, seed):
    """a trace of random commands recorded from a one-env handle"""
    from rsoccer_amd import sysid as S
    rng = np.random.default_rng(seed)
    s = L.Sim(kind, field, nb, ny, 25, 1, 0)
    hl, hw = (0.5, 0.4) if kind == 0 else (1.5, 1.2)
    n = nb + ny
    xy = rng.permutation([(x, y) for x in np.linspace(-hl, hl, 6) for y in np.linspace(-hw, hw, 4)])[:n + 1]
    ball = np.array([xy[n][0], xy[n][1], rng.uniform(-1, 1), rng.uniform(-1, 1)])
    pos = np.c_[xy[:n], rng.uniform(-180, 180, n)]
    s.reset(ball[None], pos[None, :nb], pos[None, nb:] if ny else None)
    C = s.cmd_dim
    cmds = np.zeros((T, n, C))
    if kind == 0:
        cmds[:] = rng.uniform(-40, 40, (T, n, 2))
    else:
        cmds[:, :, 1:4] = rng.uniform(-2, 2, (T, n, 3))
        cmds[:, :, 7] = rng.integers(0, 2, (T, n))
    frames = [s.get_state_full()[0]]
    for t in range(T):
        s.step(cmds[t][None])
        frames.append(s.get_state_full()[0])
    s.close()
    return S.Trace(kind, field, nb, ny, 25, np.array(frames), cmds, "random")


def _torch_terms(kind, n_robots, states, frames):
    """[B, 6] float64 from per-step states [H, B, rows] and the frames they are compared with [H, B, rows]"""
    import torch
    rs = 6 if kind == 0 else 11
    s = torch.as_tensor(states, dtype=torch.float64)
    f = torch.as_tensor(np.asarray(frames, dtype=np.float32), dtype=torch.float64)
    d = s - f
    r = 5 + rs * torch.arange(n_robots)
    d2r = np.pi / 180.0
    dth = d[:, :, r + 2]
    dth = (dth - 360.0 * torch.round(dth / 360.0)) * d2r
    t = torch.stack([(d[:, :, 0] ** 2 + d[:, :, 1] ** 2), (d[:, :, 3] ** 2 + d[:, :, 4] ** 2),
                     (d[:, :, r] ** 2 + d[:, :, r + 1] ** 2).sum(-1), (dth ** 2).sum(-1),
                     (d[:, :, r + 3] ** 2 + d[:, :, r + 4] ** 2).sum(-1), ((d[:, :, r + 5] * d2r) ** 2).sum(-1)], -1)
    return t.sum(0)


@pytest.mark.parametrize("cfg", CONFIGS)
def test_trace_eval_is_bit_exact_with_step_dev_and_the_loss_matches(L, cfg):
    import torch
    kind, field, nb, ny = cfg
    T, H, anchors = 40, 16, np.array([0, 7, 24], dtype=np.int32)
    tr = _random_trace(L, kind, field, nb, ny, T, seed=sum(cfg))
    nA, nC = anchors.size, 5
    B = nA * nC
    raw = random_params(kind, np.random.default_rng(kind * 7 + nb), nC)
    if kind == 1:
        raw[:, NAMES.index("a_lat")] = 0.0
    rows = np.repeat(raw, nA, axis=0)   # env e: candidate e // nA
    s = L.Sim(kind, field, nb, ny, 25, B, 0)
    s.physics_enable()
    s.physics_set(rows.T.copy())
    s.trace_load(tr.frames, tr.cmds, anchors)
    loss = torch.full((6, B), -1.0, dtype=torch.float32, device="cuda")
    s.trace_eval(H, loss)
    torch.cuda.synchronize()
    got_state = s.get_state_full()
    got = loss.cpu().numpy().astype(np.float64).T

    ref = L.Sim(kind, field, nb, ny, 25, B, 0)
    ref.physics_enable()
    ref.physics_set(rows.T.copy())
    a_of = anchors[np.arange(B) % nA]
    ref.set_state(tr.frames[a_of])
    cm = ref.cmds_tensor()
    states, cmp = [], []
    for t in range(H):
        c = tr.cmds[a_of + t].reshape(B, -1).T.astype(np.float32)   # [N*C, B]
        cm.copy_(torch.from_numpy(np.ascontiguousarray(c)).cuda())
        torch.cuda.synchronize()
        ref.step_dev()
        torch.cuda.synchronize()
        states.append(ref.get_state_full())
        cmp.append(tr.frames[a_of + t + 1])
    assert got_state.astype(np.float32).tobytes() == states[-1].astype(np.float32).tobytes()
    want = _torch_terms(kind, nb + ny, np.array(states), np.array(cmp)).numpy()
    assert (got >= 0).all() and got.sum() > 0
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-30)
    if cfg in [(0, 0, 3, 3), (1, 2, 1, 6)]:   # the host restatement over f32-oracle rollouts
        for c in range(nC):
            o = oracle_loss(tr, raw[c], anchors, H)
            np.testing.assert_allclose(got[c * nA:(c + 1) * nA], o, rtol=1e-6, atol=1e-30)
    s.close()
    ref.close()


@pytest.mark.parametrize("kind", ["vss", "ssl"])
def test_robosim_trace_scores_zero_at_the_defaults(L, kind):
    import rsoccer_amd.robosim as robosim
    from rsoccer_amd import sysid as S
    for tr in S.record_deck(robosim, kind, seed=1):
        ev = S.TraceEvaluator(tr, 3, horizon=10)
        total, terms = ev.evaluate({}, terms=True)
        assert (terms.cpu().numpy() == 0.0).all(), tr.scenario
        assert ev.errors() == 0
        ev.close()


def _truth(kind, seed):
    rng = np.random.default_rng(seed)
    t = params_vector(kind)
    for n in ("mu_g", "a_lin", "a_ang"):
        t[NAMES.index(n)] *= rng.uniform(0.7, 1.3)
    for n in ("e_wb", "e_rb"):
        t[NAMES.index(n)] = rng.uniform(0.05, 0.95)
    return t


FIT = {0: ("mu_g", "e_wb", "e_rb", "a_lin", "a_ang"), 1: ("mu_g", "e_rb", "a_lin", "a_ang")}


def _recovery(kind, noise, tol):
    from rsoccer_amd import sysid as S
    truth = _truth(kind, 100 + kind)
    deck = S.record_deck(oracle_module({kind: truth}), kind, seed=2)
    if noise:
        rng = np.random.default_rng(9)
        rs = 6 if kind == 0 else 11
        for tr in deck:
            n = tr.n_robots
            f = tr.frames
            pos = [0, 1] + [5 + rs * k + i for k in range(n) for i in (0, 1)]
            vel = [3, 4] + [5 + rs * k + i for k in range(n) for i in (3, 4)]
            hd = [5 + rs * k + 2 for k in range(n)]
            f[:, pos] += rng.normal(0, 0.001, (f.shape[0], len(pos)))
            f[:, vel] += rng.normal(0, 0.01, (f.shape[0], len(vel)))
            f[:, hd] += rng.normal(0, 0.5, (f.shape[0], len(hd)))
    fixed = {n: float(v) for n, v in zip(NAMES, truth) if n not in FIT[kind] and not (kind == 1 and n == "a_lat")}
    res = S.fit(deck, params=FIT[kind], fixed=fixed, population=1024, iterations=40, seed=0)
    rows = []
    for n in FIT[kind]:
        t, g = float(truth[NAMES.index(n)]), res.values[n]
        ok = abs(g - t) <= (0.03 if n.startswith("e_") else 0.05) * (2 if noise else 1) * (1 if n.startswith("e_") else abs(t))
        rows.append((n, t, g, ok))
    print(f"kind {kind} noise {noise}: " + ", ".join(f"{n} true {t:.4f} fit {g:.4f}" for n, t, g, _ in rows) + f"; loss {res.loss:.3e}")
    return res, rows


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("noise", [False, True])
def test_fit_recovers_perturbed_parameters(L, kind, noise):
    res, rows = _recovery(kind, noise, None)
    bad = [r for r in rows if not r[3]]
    assert not bad, bad
    assert res.history[-1] <= res.history[0]


def test_fitted_values_round_trip_through_make_vec(L):
    import rsoccer_amd
    from rsoccer_amd import sysid as S
    tr = S.record(rsoccer_amd.robosim, "vss", "roll_medium", seed=0)
    res = S.fit([tr], params=("mu_g",), population=64, iterations=3)
    env = rsoccer_amd.make_vec("VSS-v0", 64, physics=res.values)
    got = env.physics()
    for n, v in res.values.items():
        assert (got[n].cpu().numpy() == np.float32(v)).all(), n
    env.close()


def test_refusals(L):
    import torch
    from rsoccer_amd import sysid as S
    tr = _random_trace(L, 0, 0, 3, 3, 12, seed=4)
    loss = torch.zeros((6, 4), dtype=torch.float32, device="cuda")

    def code(fn):
        with pytest.raises(L.RsxError) as e:
            fn()
        return str(e.value).split(":")[0]

    STATE, ARG = "librsx_hip error -4", "librsx_hip error -1"
    s = L.Sim(0, 0, 3, 3, 25, 4, 0)
    assert code(lambda: s.trace_load(tr.frames, tr.cmds, [0, 1])) == STATE   # physics off
    assert code(lambda: s.trace_eval(1, loss)) == STATE
    s.physics_enable()
    assert code(lambda: s.trace_eval(1, loss)) == STATE                       # no trace loaded
    assert code(lambda: s.trace_load(tr.frames, tr.cmds, [0, 1, 2])) == ARG   # 4 % 3 != 0
    assert code(lambda: s.trace_load(tr.frames, tr.cmds, [0, 12])) == ARG     # anchor beyond n_frames - 2
    f = tr.frames.copy()
    f[2, 3] = np.inf
    assert code(lambda: s.trace_load(f, tr.cmds, [0, 1])) == ARG
    c = tr.cmds.copy()
    c[1, 0, 0] = np.nan
    assert code(lambda: s.trace_load(tr.frames, c, [0, 1])) == ARG
    s.trace_load(tr.frames, tr.cmds, [0, 4])
    assert code(lambda: s.trace_eval(0, loss)) == ARG                          # horizon < 1
    assert code(lambda: s.trace_eval(9, loss)) == ARG                          # 4 + 9 > 12
    s.trace_eval(8, loss)
    torch.cuda.synchronize()
    assert np.isfinite(loss.cpu().numpy()).all()
    t = L.Sim(0, 0, 3, 3, 25, 4, 0)
    t.physics_enable()
    t.task_attach(L.TASK_VSS_V0, 1, 0, 0)
    assert code(lambda: t.trace_load(tr.frames, tr.cmds, [0, 1])) == STATE    # a task attached
    s.close()
    t.close()
    # evaluate() clips to the valid domain instead of letting an env keep stale values
    ev = S.TraceEvaluator(tr, 2, horizon=4)
    x = torch.as_tensor(np.stack([params_vector(0)] * 2)).cuda()
    x[1, NAMES.index("e_rb")] = 1.7
    x[1, NAMES.index("m_ball")] = -1.0
    ev.evaluate(x)
    assert ev.errors() == 0
    raw = ev.sim.physics_get(L.PHYS_RAW)
    assert raw[NAMES.index("e_rb"), ev.n_anchors:].tolist() == [1.0] * ev.n_anchors
    assert (raw[NAMES.index("m_ball"), ev.n_anchors:] > 0).all()
    ev.close()
