"""Helpers of the per-env physics tests: a numpy restatement of the coefficient derivation (rsx_phys.hpp: derive_coefs) and a
ctypes mirror of the f32 oracle env up to its typed constants (oracle/rsx_oracle.c: rsxo_cfg, oracle/rsx_oracle_impl.h:
rsxo_env), so that an oracle env can carry the coefficients of a non-default parameter set and check the kernels."""
import ctypes as C

import numpy as np

# docs/PHYSICS.md section 3, in the order of rsoccer_amd._lib.PHYSICS_PARAMS
DEFAULTS = {
    0: dict(m_robot=0.18, m_ball=0.046, e_rr=0.1, e_rb=0.3, e_wb=0.6, e_wr=0.1, mu_rr=0.2, mu_rb=0.35, mu_wb=0.3, mu_g=0.3,
            spin_dec=30.0, a_lin=8.0, a_ang=300.0, a_lat=20.0),
    1: dict(m_robot=2.2, m_ball=0.046, e_rr=0.1, e_rb=0.2, e_wb=0.5, e_wr=0.1, mu_rr=0.2, mu_rb=0.35, mu_wb=0.3, mu_g=0.4,
            spin_dec=30.0, a_lin=5.0, a_ang=50.0, a_lat=0.0),
}
NAMES = ("m_robot", "m_ball", "e_rr", "e_rb", "e_wb", "e_wr", "mu_rr", "mu_rb", "mu_wb", "mu_g", "spin_dec", "a_lin", "a_ang", "a_lat")
COEFS = ("w_rb_r", "w_rb_b", "kt_rb_r", "kt_rb_b", "ope_rr", "ope_rb", "ope_wb", "e_wb", "e_wr", "mu_rr", "mu_rb", "mu_wb",
         "a_lin_h", "a_lin_h2", "a_lat_h", "a_ang_h", "mu_g_dt", "spin_dec_dt")


def derive(kind, ts_ms, raw):
    """float64 expressions, one rounding to float32; a value equal to its default's float32 stands for the exact default"""
    v = {}
    for n, x in zip(NAMES, np.asarray(raw, dtype=np.float32)):
        d = DEFAULTS[kind][n]
        v[n] = d if np.float32(d) == x else float(x)
    n_sub = (ts_ms + 4) // 5
    dt = ts_ms * 0.001
    h = dt / n_sub if n_sub else 0.0
    imr, imb = 1.0 / v["m_robot"], 1.0 / v["m_ball"]
    mt = 1.0 / (imr + 3.5 * imb)
    c = dict(w_rb_r=imr / (imr + imb), w_rb_b=imb / (imr + imb), kt_rb_r=mt * imr, kt_rb_b=mt * imb,
             ope_rr=1.0 + v["e_rr"], ope_rb=1.0 + v["e_rb"], ope_wb=1.0 + v["e_wb"], e_wb=v["e_wb"], e_wr=v["e_wr"],
             mu_rr=v["mu_rr"], mu_rb=v["mu_rb"], mu_wb=v["mu_wb"], a_lin_h=v["a_lin"] * h,
             a_lin_h2=(v["a_lin"] * h) * (v["a_lin"] * h), a_lat_h=v["a_lat"] * h, a_ang_h=v["a_ang"] * h,
             mu_g_dt=v["mu_g"] * (ts_ms * 0.001), spin_dec_dt=v["spin_dec"] * (ts_ms * 0.001))
    return np.array([c[n] for n in COEFS], dtype=np.float32)


def random_params(kind, rng, n):
    """n random valid parameter sets around the defaults, [n, 14] float32"""
    d = np.array([DEFAULTS[kind][k] for k in NAMES])
    x = d * rng.uniform(0.5, 1.5, size=(n, len(NAMES)))
    e = [NAMES.index(k) for k in ("e_rr", "e_rb", "e_wb", "e_wr")]
    x[:, e] = rng.uniform(0.0, 1.0, size=(n, 4))
    return x.astype(np.float32)


D, F = C.c_double, C.c_float


class OracleCfg(C.Structure):   # oracle/rsx_oracle.c: rsxo_cfg
    _fields_ = [(n, C.c_int) for n in ("kind", "field_type", "n_blue", "n_yellow", "n_robots", "n_bodies", "time_step_ms", "n_sub")] + [
        ("field", D * 17)] + [(n, D) for n in (
            "half_len", "half_wid", "goal_half_wid", "goal_depth", "margin", "r_robot", "r_ball", "h", "m_robot", "m_ball",
            "a_lin", "a_lat", "a_ang", "mu_g", "e_rr", "e_rb", "e_wall_ball", "e_wall_robot", "beta", "w_max", "r_wheel", "lever",
            "grav", "e_ground", "vz_min", "robot_h", "dck", "half_kw", "ir_tol", "drib_vmax", "mu_rr", "mu_rb", "mu_wb", "spin_dec",
            "pen2")] + [("wheel_ang", D * 4), ("pinv", D * 12)]


class OracleEnvF(C.Structure):   # oracle/rsx_oracle_impl.h: rsxo_env (R = float), up to the typed constants
    _fields_ = [("cfg", OracleCfg), ("RS", C.c_int), ("state_dim", C.c_int)] + [(n, F) for n in (
        "h", "half_len", "half_wid", "ghw", "gd", "margin", "r_robot", "r_ball", "rs_rr", "rs_rr2", "rs_rb", "rs_rb2",
        "w_rr", "w_rb_r", "w_rb_b", "ope_rr", "ope_rb", "e_wb", "e_wr", "beta")] + [("wall_aware", C.c_int)] + [(n, F) for n in (
        "r_held", "w_max", "half_rw", "rw_2b", "inv_rw", "r_wheel", "a_lin_h", "a_lin_h2", "a_lat_h", "a_ang_h", "mu_g_dt", "g_h",
        "e_ground", "vz_min", "robot_h", "dck_rb", "half_kw", "ir_tol", "drib_gain", "drib_vmax", "drib_vmax2", "dck", "mu_rr",
        "mu_rb", "mu_wb", "kt_rr", "kt_rb_r", "kt_rb_b", "kw", "spin_c", "ope_wb", "spin_dec_dt", "pen2")]


def oracle_consts(env):
    """the typed-constant view of an f32 OracleEnv (memory of the oracle's own struct)"""
    assert env.sfx == "_f32"
    return C.cast(env.h, C.POINTER(OracleEnvF)).contents


def oracle_coefs(env):
    s = oracle_consts(env)
    return np.array([getattr(s, n) for n in COEFS], dtype=np.float32)


def set_oracle_coefs(env, coef):
    s = oracle_consts(env)
    for n, v in zip(COEFS, np.asarray(coef, dtype=np.float32)):
        setattr(s, n, float(v))
