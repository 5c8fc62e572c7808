"""System identification on the CPU (rsoccer_amd/sysid.py): trace format and recorder, the scenario deck, the loss restated over
f32-oracle rollouts, and the cross-entropy search with an analytic loss."""
import numpy as np
import pytest

import fake_robosim
from physics_helpers import NAMES
from rsoccer_amd import sysid as S
from sysid_helpers import oracle_loss, oracle_module, params_vector


@pytest.mark.parametrize("kind", ["vss", "ssl"])
def test_deck_shapes_and_determinism(kind):
    k = S.KINDS[kind]
    cfg = S.DECK_CONFIG[k]
    n = cfg["n_blue"] + cfg["n_yellow"]
    sd = 5 + (6 if k == 0 else 11) * n
    names = [s.name for s in S.deck(kind)]
    assert len(names) == len(set(names)) and "random_play" in names
    assert ("arc" in names) == (kind == "vss") and ("kick" in names) == (kind == "ssl")
    a = S.record_deck(fake_robosim, kind, seed=3)
    b = S.record_deck(fake_robosim, kind, seed=3)
    c = S.record_deck(fake_robosim, kind, seed=4)
    for ta, tb in zip(a, b):
        assert (ta.kind, ta.field_type, ta.n_blue, ta.n_yellow) == (k, cfg["field_type"], cfg["n_blue"], cfg["n_yellow"])
        assert ta.frames.shape == (ta.steps + 1, sd + 2) and ta.cmds.shape == (ta.steps, n, 2 if k == 0 else 8)
        assert ta.steps >= 40
        assert not ta.frames[:, sd:].any()   # the stand-in exposes no internal rows
        assert np.array_equal(ta.frames, tb.frames) and np.array_equal(ta.cmds, tb.cmds)
    assert next(t for t in a if t.scenario == "random_play").steps == 200
    assert any(not np.array_equal(ta.frames, tc.frames) for ta, tc in zip(a, c))


def test_save_load_round_trip_and_refusals(tmp_path):
    tr = S.record(oracle_module(), "ssl", "hit_oblique", seed=1)
    assert tr.frames[:, -1].any()   # the module exposes the ball spin row
    p = str(tmp_path / "t.npz")
    tr.save(p)
    t2 = S.Trace.load(p)
    assert (t2.kind, t2.field_type, t2.n_blue, t2.n_yellow, t2.time_step_ms, t2.scenario) == \
        (tr.kind, tr.field_type, tr.n_blue, tr.n_yellow, tr.time_step_ms, tr.scenario)
    assert np.array_equal(t2.frames, tr.frames) and np.array_equal(t2.cmds, tr.cmds)

    f = tr.frames.copy()
    f[3, 7] = np.nan
    with pytest.raises(ValueError):
        S.Trace(tr.kind, tr.field_type, tr.n_blue, tr.n_yellow, 25, f, tr.cmds)
    with pytest.raises(ValueError):
        S.Trace(tr.kind, tr.field_type, tr.n_blue, tr.n_yellow, 25, tr.frames[:, :-1], tr.cmds)
    with pytest.raises(ValueError):
        S.Trace(tr.kind, tr.field_type, tr.n_blue, tr.n_yellow, 25, tr.frames, tr.cmds[:-1])
    with pytest.raises(ValueError):
        S.Trace("rugby", 0, 3, 3, 25, tr.frames, tr.cmds)
    bad = dict(np.load(p))
    bad["kind"] = np.array(7)
    np.savez(str(tmp_path / "bad.npz"), **bad)
    with pytest.raises(ValueError):
        S.Trace.load(str(tmp_path / "bad.npz"))

    # anchors: every horizon frames, none airborne, none without a full window
    chip = S.record(oracle_module(), "ssl", "chip", seed=1)
    air = chip.airborne()
    assert air.any()
    for h in (5, 10, 40):
        an = S.default_anchors(chip, h)
        assert (an % h == 0).all() and (an + h <= chip.steps).all() and not air[an].any()
    with pytest.raises(ValueError):
        S.default_anchors(chip, chip.steps + 1)


@pytest.mark.parametrize("kind,scenario", [(0, "hit_oblique"), (0, "wall_bounce"), (1, "kick"), (1, "push")])
def test_restated_loss_is_zero_at_the_recording_parameters(kind, scenario):
    rng = np.random.default_rng(5)
    truth = params_vector(kind)
    for n in ("mu_g", "a_lin", "a_ang", "e_rb"):
        truth[NAMES.index(n)] *= rng.uniform(0.7, 1.3)
    tr = S.record(oracle_module({kind: truth}), kind, scenario, seed=2)
    anchors = [0, 10]
    z = oracle_loss(tr, truth, anchors, 20)
    assert (z == 0.0).all()
    other = oracle_loss(tr, params_vector(kind), anchors, 20)
    assert other.sum() > 0.0


def test_cross_entropy_search_finds_the_minimum_of_a_quadratic():
    import torch
    target = torch.tensor([0.37, 0.61, 9.3])
    scale = torch.tensor([1.0, 1.0, 0.01])

    def loss(x):
        return (((x - target) * scale) ** 2).sum(1)

    res = S.fit([], params=("mu_g", "e_wb", "a_lin"), kind="vss", loss=loss, population=256, iterations=60, seed=3)
    got = torch.tensor([res.values[n] for n in ("mu_g", "e_wb", "a_lin")])
    assert torch.allclose(got, target, rtol=1e-3, atol=1e-4), res
    assert res.history == sorted(res.history, reverse=True) and res.loss == res.history[-1]
    assert set(res.values) == set(NAMES)
    # untouched parameters stay at the defaults, fixed ones at their values; the same seed repeats itself
    res2 = S.fit([], params=("mu_g", "e_wb", "a_lin"), kind="vss", loss=loss, population=256, iterations=60, seed=3,
                 fixed={"m_ball": 0.05})
    assert res2.values["m_ball"] == 0.05 and res2.values["mu_rr"] == pytest.approx(0.2)
    assert [res2.values[n] for n in ("mu_g", "e_wb", "a_lin")] == [res.values[n] for n in ("mu_g", "e_wb", "a_lin")]
    ssl = S.fit([], params=("mu_g",), kind="ssl", loss=lambda x: (x[:, 0] - 0.5) ** 2, population=64, iterations=30)
    assert "a_lat" not in ssl.values and ssl.values["mu_g"] == pytest.approx(0.5, abs=1e-3)
    with pytest.raises(KeyError):
        S.fit([], params=("a_lat",), kind="ssl", loss=loss)
