"""Per-env physics parameters, host side (no GPU): defaults, the coefficient derivation and the range checks of
rsx_physics_defaults / rsx_physics_derive (include/rsx.h)."""
import numpy as np
import pytest

from physics_helpers import COEFS, DEFAULTS, NAMES, derive, oracle_coefs, random_params


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    import os
    if not os.path.exists(g.HIP_SO):
        g.build()
    from rsoccer_amd import _lib
    _lib.load()
    return _lib


def test_names_match_the_binding(L):
    assert L.PHYSICS_PARAMS == NAMES and L.PHYSICS_COEFS == COEFS


@pytest.mark.parametrize("kind", [0, 1])
def test_defaults_are_the_documented_constants(L, kind):
    got = L.physics_defaults(kind)
    want = np.array([DEFAULTS[kind][n] for n in NAMES], dtype=np.float32)
    assert np.array_equal(got, want)
    import rsoccer_amd
    d = rsoccer_amd.physics_defaults("vss" if kind == 0 else "ssl")
    assert ("a_lat" in d) == (kind == 0)
    assert all(np.float32(d[n]) == np.float32(DEFAULTS[kind][n]) for n in d)


@pytest.mark.parametrize("kind,field,nb,ny", [(0, 0, 3, 3), (1, 2, 1, 6), (1, 1, 11, 11)])
@pytest.mark.parametrize("ts", [25, 16, 40])
def test_derived_defaults_are_the_oracles_typed_constants(L, oracle_mod, kind, field, nb, ny, ts):
    """the derivation of the defaults equals, bit for bit, what a fresh f32 oracle env holds (which also pins the mirror's layout)"""
    env = oracle_mod.OracleEnv(kind, field, nb, ny, ts, "f32")
    got = L.physics_derive(kind, ts, L.physics_defaults(kind))
    want = oracle_coefs(env)
    bad = [n for n, a, b in zip(COEFS, got, want) if a.tobytes() != b.tobytes()]
    assert not bad, bad
    env.close()


@pytest.mark.parametrize("kind", [0, 1])
def test_numpy_derivation_matches_the_library_bit_for_bit(L, kind):
    rng = np.random.default_rng(7 + kind)
    sets = random_params(kind, rng, 10000)
    if kind == 1:
        sets[:, NAMES.index("a_lat")] = 0.0
    sets[::97] = L.physics_defaults(kind)   # some at the defaults (the exact-default rule)
    for ts in (25, 16):
        for raw in sets:
            got = L.physics_derive(kind, ts, raw)
            assert got.tobytes() == derive(kind, ts, raw).tobytes(), (ts, raw)


@pytest.mark.parametrize("kind", [0, 1])
def test_out_of_range_values_are_refused(L, kind):
    d = L.physics_defaults(kind)
    bad = [("m_robot", 0.0), ("m_ball", -1.0), ("e_rb", 1.5), ("e_rr", -0.1), ("mu_g", -0.01), ("a_lin", np.inf),
           ("spin_dec", np.nan)]
    if kind == 1:
        bad.append(("a_lat", 1.0))
    for name, v in bad:
        raw = d.copy()
        raw[NAMES.index(name)] = v
        with pytest.raises(L.RsxError):
            L.physics_derive(kind, 25, raw)
    with pytest.raises(L.RsxError):
        L.physics_derive(2, 25, d)
