// rsx_state_io.hpp — the state of a lane's body in wire format (the [rows][B] SoA array: degrees, deg/s; SSL: infrared flag
// and wheel speeds): load, interpretation into the working record (rsx_body.hpp: Body), and the store.
#pragma once
#include <hip/hip_runtime.h>

#include "rsx_math.hpp"
#include "rsx_params.hpp"
#include "rsx_body.hpp"
#include "rsx_lane_map.hpp"

namespace rsx {

// ---------------------------------------------------------------------------------------------
// SoA state access
// ---------------------------------------------------------------------------------------------
// Raw wire values of the lane's body.  Robot and ball lanes run the SAME load instructions (only
// the row index differs: ball rows 0..4 + the vz row, robot rows 5+RS*b .. +5), so all loads of a
// wave are in flight together; nothing is computed here (a use would park the wave on vmcnt
// between the two roles' loads).
struct RawBody { float v0, v1, v2, v3, v4, v5, ir /* ball: spin */, w[4]; };

template <int KIND>
__device__ __forceinline__ RawBody load_raw(const Params& P, const float* __restrict__ st, int e,
                                            int b, bool is_robot, bool is_ball) {
    constexpr int RS = ModelD<KIND>::rs;
    const ix_t B4 = (ix_t)4 * (ix_t)P.row_stride, e4 = (ix_t)4 * (ix_t)e;   // bytes per row, this env's column
    RawBody r{};
    if (is_robot || is_ball) {
        const int row0 = is_ball ? 0 : 5 + RS * b;
        const int row5 = is_ball ? P.state_dim : row0 + 5;
        const ix_t i0 = (ix_t)row0 * B4 + e4;
        r.v0 = at_byte(st, i0); r.v1 = at_byte(st, i0 + B4); r.v2 = at_byte(st, i0 + 2 * B4); r.v3 = at_byte(st, i0 + 3 * B4); r.v4 = at_byte(st, i0 + 4 * B4);
        r.v5 = at_byte(st, (ix_t)row5 * B4 + e4);
    }
    if (KIND == RSX_KIND_SSL) {   // robots: infrared flag; ball: spin row (same load instruction)
        if (is_robot || is_ball) r.ir = at_byte(st, (ix_t)(is_ball ? P.state_dim + 1 : 5 + RS * b + 6) * B4 + e4);
        if (is_robot) {
            const ix_t i7 = (ix_t)(5 + RS * b + 7) * B4 + e4;
#pragma unroll
            for (int i = 0; i < 4; ++i) r.w[i] = at_byte(st, i7 + (ix_t)i * B4);
        }
    } else if (is_ball) {
        r.ir = at_byte(st, (ix_t)(P.state_dim + 1) * B4 + e4);
    }
    return r;
}

// wire values -> the lane's working record (heading in degrees, rate in rad/s, exact sin / cos)
template <int KIND>
__device__ __forceinline__ void interpret_body(const RawBody& r, bool is_robot, bool is_ball, Body& o,
                                               float& th_deg, float& om_deg, float w[4]) {
    using K = KC<KIND>;
    o = Body{};
    th_deg = 0.0f; om_deg = 0.0f;
    w[0] = w[1] = w[2] = w[3] = 0.0f;
    o.x = r.v0; o.y = r.v1; o.vx = r.v3; o.vy = r.v4;
    if (is_robot) {
        th_deg = r.v2; om_deg = r.v5;
        if (KIND == RSX_KIND_SSL) {
            o.ir = r.ir != 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = r.w[i];
        }
        o.th = th_deg;
        o.om = om_deg * K::deg2rad;
        sincos_f32(o.th * K::deg2rad, o.s, o.c);
    } else if (is_ball) {
        o.z = r.v2 - K::r_ball;
        o.vz = r.v5;
        o.om = r.ir;   // spin about the vertical axis, rad/s
    }
}

// SSL wheel speeds (rad/s) implied by the body velocity — Entities/Frame.py:73-76
template <int KIND>
__device__ __forceinline__ void wheel_speeds(const Params& P, const Body& o, float w[4]) {
    using K = KC<KIND>;
    float vf = o.vx * o.c + o.vy * o.s;
    float vl = o.vy * o.c - o.vx * o.s;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = ((vl * P.wc[i] - vf * P.ws[i]) + o.om * K::r_robot) * K::inv_rw;
}

// store in wire format; th_deg / om_deg / w are the values to write for a robot.  Same row
// trick as load_raw: one store sequence for both roles.
template <int KIND>
__device__ __forceinline__ void store_body(const Params& P, float* __restrict__ st, int e, int b,
                                           bool is_robot, bool is_ball, const Body& o,
                                           float th_deg, float om_deg, const float w[4],
                                           bool write_ir) {
    using K = KC<KIND>;
    constexpr int RS = ModelD<KIND>::rs;
    const ix_t B4 = (ix_t)4 * (ix_t)P.row_stride, e4 = (ix_t)4 * (ix_t)e;
    if (is_robot || is_ball) {
        const int row0 = is_ball ? 0 : 5 + RS * b;
        const int row5 = is_ball ? P.state_dim : row0 + 5;
        const ix_t i0 = (ix_t)row0 * B4 + e4;
        at_byte(st, i0) = o.x; at_byte(st, i0 + B4) = o.y; at_byte(st, i0 + 2 * B4) = is_ball ? K::r_ball + o.z : th_deg;
        at_byte(st, i0 + 3 * B4) = o.vx; at_byte(st, i0 + 4 * B4) = o.vy;
        at_byte(st, (ix_t)row5 * B4 + e4) = is_ball ? o.vz : om_deg;
    }
    if (is_ball) at_byte(st, (ix_t)(P.state_dim + 1) * B4 + e4) = o.om;
    if (KIND == RSX_KIND_SSL && is_robot) {
        const ix_t i6 = (ix_t)(5 + RS * b + 6) * B4 + e4;
        if (write_ir) at_byte(st, i6) = o.ir ? 1.0f : 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) at_byte(st, i6 + (ix_t)(1 + i) * B4) = w[i];
    }
}

}  // namespace rsx
