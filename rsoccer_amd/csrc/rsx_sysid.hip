// rsx_sysid.hip — trace evaluation for system identification (include/rsx.h: rsx_trace_load / rsx_trace_eval), in a translation
// unit of its own so that the instantiations of every existing kernel stay exactly what they were.
//
// trace_eval_phys_kernel runs, per env, `horizon` raw simulator steps from an anchor frame of a recorded trace with the env's own
// physics coefficients (rsx_phys.hpp: EnvCoef), all in registers, and sums the squared deviation of every body from the trace's
// next frame after each step.  Lanes per env and variants are those of sim_step_phys_kernel (rsx_variants.hpp: with_sim_variant).
//
// Between two steps the lane's record goes through exactly what a store_body -> load_raw -> interpret_body round trip applies
// (wire_of below, then interpret_body): heading kept in degrees, rate stored in deg/s and converted back, ball height stored as
// r_ball + z.  The final state is therefore bit for bit what `horizon` separate sim_step_phys_kernel launches leave behind.
//
// Trace layout on the device: the state SoA with frames in place of envs — frames [state_dim + 2][n_frames], commands
// [N * C][n_frames - 1], f32 — so load_raw and the command reads address frame f the way they address env e.  Every candidate of
// an anchor reads the same frames: they stay L2-resident.
#include <hip/hip_runtime.h>

#include "rsx.h"
#include "rsx_units.hpp"
#include "rsx_variants.hpp"

namespace rsx {

namespace {

static_assert(RSX_TRACE_TERMS == 6, "loss terms");

struct TraceArgs {
    const float* frames;      // [state_dim + 2][n_frames]
    const float* cmds;        // [N * C][n_frames - 1]
    const int32_t* anchors;   // [n_anchors]
    int n_frames, n_anchors;
};

// the wire values store_body writes for the lane's body (robots: th_deg, om_deg and the wheel speeds w; ball: r_ball + z, vz, spin),
// as the RawBody load_raw would read back.  `prev`: the values loaded before this step (an SSL robot's infrared row is not
// rewritten by an in-place step without sub-steps, sim_step_body: write_ir)
template <int KIND>
__device__ __forceinline__ RawBody wire_of(const Params& P, const bool is_robot, const bool is_ball, const Body& o, const float th_deg,
                                           const float om_deg, const float w[4], const RawBody& prev) {
    using K = KC<KIND>;
    RawBody r{};
    if (is_robot || is_ball) {
        r.v0 = o.x; r.v1 = o.y; r.v2 = is_ball ? K::r_ball + o.z : th_deg;
        r.v3 = o.vx; r.v4 = o.vy; r.v5 = is_ball ? o.vz : om_deg;
    }
    if (is_ball) r.ir = o.om;
    if (KIND == RSX_KIND_SSL && is_robot) {
        r.ir = P.n_sub != 0 ? (o.ir ? 1.0f : 0.0f) : prev.ir;
#pragma unroll
        for (int i = 0; i < 4; ++i) r.w[i] = w[i];
    }
    return r;
}

// squared deviation of the lane's body from trace frame f, added to the accumulators (SI units; double: the terms are small
// differences of nearby floats, summed over up to hundreds of bodies and steps).  Both roles add through selects: a role branch
// into an indexed accumulator array sends the array to scratch memory
struct Acc { double bp, bv, rp, rth, rv, rom; };
template <int KIND>
__device__ __forceinline__ void add_deviation(const Params& PT, const float* __restrict__ frames, const int f, const int b,
                                              const bool is_robot, const bool is_ball, const RawBody& s, Acc& a) {
    constexpr int RS = ModelD<KIND>::rs;
    constexpr double D2R = 3.14159265358979323846 / 180.0;
    if (!(is_robot || is_ball)) return;
    const ix_t B4 = (ix_t)4 * (ix_t)PT.row_stride, f4 = (ix_t)4 * (ix_t)f;
    const int row0 = is_ball ? 0 : 5 + RS * b;
    const ix_t i0 = (ix_t)row0 * B4 + f4;
    const double dx = (double)s.v0 - (double)at_byte(frames, i0), dy = (double)s.v1 - (double)at_byte(frames, i0 + B4);
    const double dvx = (double)s.v3 - (double)at_byte(frames, i0 + 3 * B4), dvy = (double)s.v4 - (double)at_byte(frames, i0 + 4 * B4);
    double dth = (double)s.v2 - (double)at_byte(frames, i0 + 2 * B4);
    dth = (dth - 360.0 * rint(dth * (1.0 / 360.0))) * D2R;   // wrapped to [-pi, pi]
    const double dom = ((double)s.v5 - (double)at_byte(frames, i0 + 5 * B4)) * D2R;
    const double p2 = dx * dx + dy * dy, v2 = dvx * dvx + dvy * dvy;
    a.bp += is_ball ? p2 : 0.0; a.bv += is_ball ? v2 : 0.0;
    a.rp += is_ball ? 0.0 : p2; a.rv += is_ball ? 0.0 : v2;
    a.rth += is_ball ? 0.0 : dth * dth; a.rom += is_ball ? 0.0 : dom * dom;
}

// hot arguments: the handle's state (final state of every env), the loss rows [RSX_TRACE_TERMS][num_envs], the tile map, horizon
template <int KIND, int L, int NR>
__global__ __launch_bounds__(64) void trace_eval_phys_kernel(float* __restrict__ state, float* __restrict__ loss, const int per_xcd,
                                                             const int horizon, const Params P, const float* __restrict__ phys,
                                                             const TraceArgs tr) {
    using K = KC<KIND>;
    constexpr int G = 64 / L;
    constexpr int CD = ModelD<KIND>::cmd_dim;
    __shared__ Shared<L> sh;
    __shared__ double red[RSX_TRACE_TERMS][64];
#ifdef RSX_TIMING
    if (threadIdx.x == 0) sh.dbg = nullptr;
#endif
    const int lane = threadIdx.x;
    const int b = LaneMap<L>::body(lane), g = LaneMap<L>::env(lane);
    const int e = tile_of_block(per_xcd) * G + g;
    const int N = NR ? NR : P.n_robots;
    const bool live = e < P.num_envs;
    const bool is_robot = live && b < N, is_ball = live && b == N;
    Params PT = P;
    PT.row_stride = tr.n_frames;   // the trace's frame rows: frame f where the state has env e
    const int f0 = live ? tr.anchors[e % tr.n_anchors] : 0;
    const ix_t C4 = (ix_t)4 * (ix_t)(tr.n_frames - 1);   // bytes per command row of the trace

    RawBody cur = load_raw<KIND>(PT, tr.frames, f0, b, is_robot, is_ball);
    EnvCoef cf{};
    if (live) load_coefs(P, phys, e, cf);
    Acc acc{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    Body o; float od, wd, w[4];
    for (int t = 0; t < horizon; ++t) {
        const int f = f0 + t;
        float q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (is_robot) {
            const ix_t c0 = (ix_t)(b * CD) * C4 + (ix_t)4 * (ix_t)f;
#pragma unroll
            for (int i = 0; i < CD; ++i) q[i] = at_byte(tr.cmds, c0 + (ix_t)i * C4);
        }
        interpret_body<KIND>(cur, is_robot, is_ball, o, od, wd, w);
        if (is_robot) robot_targets<KIND>(P, o, q);
        physics<KIND, L, NR>(P, o, b, g, live, sh, cf);
        if (is_robot) {
            od = o.th; wd = o.om * K::rad2deg;
            if (KIND == RSX_KIND_SSL) wheel_speeds<KIND>(P, o, w);
        }
        cur = wire_of<KIND>(P, is_robot, is_ball, o, od, wd, w, cur);
        add_deviation<KIND>(PT, tr.frames, f + 1, b, is_robot, is_ball, cur, acc);
    }
    store_body<KIND>(P, state, e, b, is_robot, is_ball, o, od, wd, w, true);
    if (KIND == RSX_KIND_SSL && is_robot && P.n_sub == 0) {   // (see wire_of)
        constexpr int RS = ModelD<KIND>::rs;
        at_byte(state, (ix_t)(5 + RS * b + 6) * ((ix_t)4 * (ix_t)P.row_stride) + (ix_t)4 * (ix_t)e) = cur.ir;
    }

    // the env's lanes -> one value per term, in body order
    red[0][lane] = acc.bp; red[1][lane] = acc.bv; red[2][lane] = acc.rp; red[3][lane] = acc.rth; red[4][lane] = acc.rv; red[5][lane] = acc.rom;
    __syncthreads();
    if (live && b == 0) {
#pragma unroll
        for (int k = 0; k < RSX_TRACE_TERMS; ++k) {
            double sum = 0.0;
#pragma unroll
            for (int j = 0; j < L; ++j) sum += red[k][LaneMap<L>::slot(j, g)];
            loss[(size_t)k * (size_t)P.num_envs + (size_t)e] = (float)sum;
        }
    }
}

template <int KIND>
void trace_k(const Params& P, const int L, const int NR, const float* phys, float* state, float* loss, const TraceArgs& tr,
             const int horizon, hipStream_t s) {
    const int grid = lane_grid(L, P.num_envs);
    with_sim_variant<KIND, 32>(L, NR, [&](auto l, auto nr) {
        rsx_launch((trace_eval_phys_kernel<KIND, l, nr>), dim3((unsigned)grid), dim3(64), 0, s, state, loss, grid >> 3, horizon, P, phys, tr);
    });
}

}  // namespace

void launch_trace_eval(const Params& P, const int L, const int NR, const float* phys, float* state, float* loss, const float* frames,
                       const float* cmds, const int32_t* anchors, const int n_frames, const int n_anchors, const int horizon,
                       hipStream_t s) {
    const TraceArgs tr{frames, cmds, anchors, n_frames, n_anchors};
    if (P.kind == RSX_KIND_VSS) trace_k<RSX_KIND_VSS>(P, L, NR, phys, state, loss, tr, horizon, s);
    else trace_k<RSX_KIND_SSL>(P, L, NR, phys, state, loss, tr, horizon, s);
}

}  // namespace rsx
