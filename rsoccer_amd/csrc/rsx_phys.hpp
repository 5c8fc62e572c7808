// rsx_phys.hpp — per-env physics parameters (include/rsx.h: rsx_physics_*).
//
// The kernels read the model constants that a user may want to vary per env through a COEFFICIENT PROVIDER, a template
// parameter of the body routines (rsx_body.hpp) and of the lane-group kernels (rsx_kernels.hpp):
//   * LitCoef<KIND>: today's compile-time literals (KC<KIND>) and Params fields — the instantiations every existing kernel
//     uses, instruction for instruction what they were before the provider existed;
//   * EnvCoef: the env's derived coefficients in registers, loaded once per launch from the handle's coefficient rows
//     (the *_phys_kernel entry points).
// Derived coefficients come from the parameters by the expressions of KC<> and derive_model_k, in double, rounded to
// float once (derive_coefs: one function for the host and the device, -ffp-contract=off: the same bits on both).
#pragma once
#include <hip/hip_runtime.h>

#include "rsx.h"
#include "rsx_params.hpp"

namespace rsx {

constexpr int NPHYS = RSX_PHYS_PARAMS, NCOEF = RSX_PHYS_COEFS;
// coefficient rows
enum : int {
    CF_W_RB_R, CF_W_RB_B, CF_KT_RB_R, CF_KT_RB_B, CF_OPE_RR, CF_OPE_RB, CF_OPE_WB, CF_E_WB, CF_E_WR,
    CF_MU_RR, CF_MU_RB, CF_MU_WB, CF_A_LIN_H, CF_A_LIN_H2, CF_A_LAT_H, CF_A_ANG_H, CF_MU_G_DT, CF_SPIN_DEC_DT
};
static_assert(CF_SPIN_DEC_DT + 1 == NCOEF, "coefficient rows");

// the defaults (ModelD<KIND>) in the order of RSX_PHYS_*
template <int KIND>
__host__ __device__ inline double phys_default_k(const int p) {
    using D = ModelD<KIND>;
    switch (p) {
        case RSX_PHYS_M_ROBOT: return D::m_robot;
        case RSX_PHYS_M_BALL: return D::m_ball;
        case RSX_PHYS_E_RR: return D::e_rr;
        case RSX_PHYS_E_RB: return D::e_rb;
        case RSX_PHYS_E_WB: return D::e_wb;
        case RSX_PHYS_E_WR: return D::e_wr;
        case RSX_PHYS_MU_RR: return D::mu_rr;
        case RSX_PHYS_MU_RB: return D::mu_rb;
        case RSX_PHYS_MU_WB: return D::mu_wb;
        case RSX_PHYS_MU_G: return D::mu_g;
        case RSX_PHYS_SPIN_DEC: return D::spin_dec;
        case RSX_PHYS_A_LIN: return D::a_lin;
        case RSX_PHYS_A_ANG: return D::a_ang;
        default: return D::a_lat;
    }
}
__host__ __device__ inline double phys_default(const int kind, const int p) {
    return kind == RSX_KIND_VSS ? phys_default_k<RSX_KIND_VSS>(p) : phys_default_k<RSX_KIND_SSL>(p);
}

// Validity of one value (rsx.h): masses > 0, restitutions in [0, 1], everything else >= 0, all finite; SSL: a_lat == 0.
__host__ __device__ inline bool phys_valid(const int kind, const int p, const float v) {
    if (!(v >= 0.0f && v <= 3.4028234663852886e38f)) return false;   // NaN, negative, infinite
    if (p == RSX_PHYS_M_ROBOT || p == RSX_PHYS_M_BALL) return v > 0.0f;
    if (p >= RSX_PHYS_E_RR && p <= RSX_PHYS_E_WR) return v <= 1.0f;
    if (p == RSX_PHYS_A_LAT && kind == RSX_KIND_SSL) return v == 0.0f;
    return true;
}

// parameters -> coefficients, the expressions of KC<KIND> (masses, restitutions, friction) and derive_model_k (the per-sub-step
// and per-step changes).  A value equal to the float rounding of its default is read as the exact default, so that the defaults
// derive the compiled-in literals bit for bit (rounding the parameter to float first would move some of them by one ulp).
__host__ __device__ inline void derive_coefs(const int kind, const int ts_ms, const float* raw, float* c) {
    double v[NPHYS];
    for (int p = 0; p < NPHYS; ++p) {
        const double d = phys_default(kind, p);
        v[p] = raw[p] == (float)d ? d : (double)raw[p];
    }
    const int n_sub = (ts_ms + 4) / 5;
    const double dt = ts_ms * 0.001;
    const double h = n_sub ? dt / n_sub : 0.0;
    const double imr = 1.0 / v[RSX_PHYS_M_ROBOT], imb = 1.0 / v[RSX_PHYS_M_BALL];
    const double mt_rb = 1.0 / (imr + 3.5 * imb);
    c[CF_W_RB_R] = (float)(imr / (imr + imb)); c[CF_W_RB_B] = (float)(imb / (imr + imb));
    c[CF_KT_RB_R] = (float)(mt_rb * imr); c[CF_KT_RB_B] = (float)(mt_rb * imb);
    c[CF_OPE_RR] = (float)(1.0 + v[RSX_PHYS_E_RR]); c[CF_OPE_RB] = (float)(1.0 + v[RSX_PHYS_E_RB]);
    c[CF_OPE_WB] = (float)(1.0 + v[RSX_PHYS_E_WB]);
    c[CF_E_WB] = (float)v[RSX_PHYS_E_WB]; c[CF_E_WR] = (float)v[RSX_PHYS_E_WR];
    c[CF_MU_RR] = (float)v[RSX_PHYS_MU_RR]; c[CF_MU_RB] = (float)v[RSX_PHYS_MU_RB]; c[CF_MU_WB] = (float)v[RSX_PHYS_MU_WB];
    const double a_lin = v[RSX_PHYS_A_LIN];
    c[CF_A_LIN_H] = (float)(a_lin * h); c[CF_A_LIN_H2] = (float)((a_lin * h) * (a_lin * h));
    c[CF_A_LAT_H] = (float)(v[RSX_PHYS_A_LAT] * h); c[CF_A_ANG_H] = (float)(v[RSX_PHYS_A_ANG] * h);
    c[CF_MU_G_DT] = (float)(v[RSX_PHYS_MU_G] * (ts_ms * 0.001));
    c[CF_SPIN_DEC_DT] = (float)(v[RSX_PHYS_SPIN_DEC] * (ts_ms * 0.001));
}

// Device block of a physics-enabled handle (one allocation; S = the handle's row stride):
//   PhysHeader | raw rows [NPHYS][S] | coefficient rows [NCOEF][S] | staging rows [NPHYS][S] | staging mask [S] bytes
struct PhysHeader {
    float lo[16], hi[16];   // randomisation ranges (RSX_PHYS_* order)
    uint32_t mask;          // bit p: parameter p is redrawn at every episode start
    uint32_t err;           // envs refused by device-side rsx_physics_set (rsx_physics_errors)
    int32_t kind, ts_ms;
    uint32_t pad[28];       // -> 256 bytes: the rows start on a 256-byte boundary
};
static_assert(sizeof(PhysHeader) == 256, "physics header");
constexpr int PHYS_HDR_FLOATS = (int)(sizeof(PhysHeader) / 4);
__host__ __device__ inline float* phys_raw(float* blk) { return blk + PHYS_HDR_FLOATS; }
__host__ __device__ inline float* phys_coef(float* blk, const size_t S) { return blk + PHYS_HDR_FLOATS + (size_t)NPHYS * S; }
__host__ __device__ inline float* phys_stage(float* blk, const size_t S) { return blk + PHYS_HDR_FLOATS + (size_t)(NPHYS + NCOEF) * S; }
__host__ __device__ inline uint8_t* phys_stage_mask(float* blk, const size_t S) {
    return reinterpret_cast<uint8_t*>(blk + PHYS_HDR_FLOATS + (size_t)(2 * NPHYS + NCOEF) * S);
}
inline size_t phys_block_bytes(const size_t S) { return sizeof(PhysHeader) + (size_t)(2 * NPHYS + NCOEF) * S * 4 + S; }

// ---- coefficient providers ----
template <int KIND>
struct LitCoef {
    using K = KC<KIND>;
    __device__ __forceinline__ float w_rb_r() const { return K::w_rb_r; }
    __device__ __forceinline__ float w_rb_b() const { return K::w_rb_b; }
    __device__ __forceinline__ float kt_rb_r() const { return K::kt_rb_r; }
    __device__ __forceinline__ float kt_rb_b() const { return K::kt_rb_b; }
    __device__ __forceinline__ float ope_rr() const { return K::ope_rr; }
    __device__ __forceinline__ float ope_rb() const { return K::ope_rb; }
    __device__ __forceinline__ float ope_wb() const { return K::ope_wb; }
    __device__ __forceinline__ float e_wb() const { return K::e_wb; }
    __device__ __forceinline__ float e_wr() const { return K::e_wr; }
    __device__ __forceinline__ float mu_rr() const { return K::mu_rr; }
    __device__ __forceinline__ float mu_rb() const { return K::mu_rb; }
    __device__ __forceinline__ float mu_wb() const { return K::mu_wb; }
    __device__ __forceinline__ float a_lin_h(const Params& P) const { return P.a_lin_h; }
    __device__ __forceinline__ float a_lin_h2(const Params& P) const { return P.a_lin_h2; }
    __device__ __forceinline__ float a_lat_h(const Params& P) const { return P.a_lat_h; }
    __device__ __forceinline__ float a_ang_h(const Params& P) const { return P.a_ang_h; }
    __device__ __forceinline__ float mu_g_dt(const Params& P) const { return P.mu_g_dt; }
    __device__ __forceinline__ float spin_dec_dt(const Params& P) const { return P.spin_dec_dt; }
};

struct EnvCoef {
    float c[NCOEF];
    __device__ __forceinline__ float w_rb_r() const { return c[CF_W_RB_R]; }
    __device__ __forceinline__ float w_rb_b() const { return c[CF_W_RB_B]; }
    __device__ __forceinline__ float kt_rb_r() const { return c[CF_KT_RB_R]; }
    __device__ __forceinline__ float kt_rb_b() const { return c[CF_KT_RB_B]; }
    __device__ __forceinline__ float ope_rr() const { return c[CF_OPE_RR]; }
    __device__ __forceinline__ float ope_rb() const { return c[CF_OPE_RB]; }
    __device__ __forceinline__ float ope_wb() const { return c[CF_OPE_WB]; }
    __device__ __forceinline__ float e_wb() const { return c[CF_E_WB]; }
    __device__ __forceinline__ float e_wr() const { return c[CF_E_WR]; }
    __device__ __forceinline__ float mu_rr() const { return c[CF_MU_RR]; }
    __device__ __forceinline__ float mu_rb() const { return c[CF_MU_RB]; }
    __device__ __forceinline__ float mu_wb() const { return c[CF_MU_WB]; }
    __device__ __forceinline__ float a_lin_h(const Params&) const { return c[CF_A_LIN_H]; }
    __device__ __forceinline__ float a_lin_h2(const Params&) const { return c[CF_A_LIN_H2]; }
    __device__ __forceinline__ float a_lat_h(const Params&) const { return c[CF_A_LAT_H]; }
    __device__ __forceinline__ float a_ang_h(const Params&) const { return c[CF_A_ANG_H]; }
    __device__ __forceinline__ float mu_g_dt(const Params&) const { return c[CF_MU_G_DT]; }
    __device__ __forceinline__ float spin_dec_dt(const Params&) const { return c[CF_SPIN_DEC_DT]; }
};

}  // namespace rsx
