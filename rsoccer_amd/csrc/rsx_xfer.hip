// rsx_xfer.hip — transfer of running episodes between envs and handles (include/rsx.h: rsx_task_transfer), in a translation unit of
// its own so that the instantiations of every existing kernel stay exactly what they were.
//
// transfer_kernel copies, for pair i, everything per-env that a checkpoint blob carries from env src_ids[i] of one side to env
// dst_ids[i] of the other: the state rows, the scalar arena, (PHYS) the parameter and coefficient rows, the obs / final_obs rows and
// the terminated / truncated bytes.  A side is a handle's buffers or a staging buffer of the same shape addressed by the pair index
// (same-handle transfers: a GATHER launch into the staging buffer, then a SCATTER launch out of it, so that every read happens
// before every write).  It is a copy: no arithmetic but one row, see below.
//
// Grid: x = blocks of 256 consecutive pairs, y = what is copied.
//   y < n_slices      the SoA rows [rows][stride], one lane per pair, 16 rows per slice: consecutive pairs sit on consecutive lanes,
//                     so a run of consecutive env ids (identity map, contiguous blocks, sorted resampling) is one 256-byte request
//                     per row and wave; the 16 loads of a lane are independent and all in flight before the first store.  The row
//                     axis is cut into slices, not walked by one lane, so that a small batch still puts enough waves on the chip.
//                     Slice 0 also copies the two flag bytes and counts the pairs it skips.
//   y - n_slices = 0  obs, 1 final_obs: AoS [B][obs_dim] — lanes run across the floats of the block's rows (a lane per env would
//                     read 64 rows obs_dim floats apart), 8 independent loads per lane before the first store.
// Offsets are 32-bit element counts: rsx_create / rsx_task_attach keep every array of a handle below 4 GB.
//
// The one row that is not copied: VSS-v0's previous ball potential (ROW_PREV_POT).  The one-lane-per-env VSS kernel derives it from
// the ball position and never stores it (rsx_epl.hpp), so the row of a source stepped by that kernel is stale; the destination may be
// stepped by a lane-group kernel, which reads it.  The launch that reads a HANDLE (DIRECT, GATHER) therefore recomputes it from the
// source's ball position (rsx_math.hpp: vss_ball_potential, the expression of the step kernels and of rsx_task_checkpoint_save).  No
// other layout leaves a row stale: the one-lane-per-env SSL kernels and the four-lane kernel store every row they change, and the
// rows they skip (VSS-v0: the goal counters and the ball's height rows off a terminal step / a chip) hold the value they would write.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rsx.h"
#include "rsx_launch.hpp"
#include "rsx_math.hpp"
#include "rsx_units.hpp"

namespace rsx {

namespace {

constexpr int TPB = 256;   // lanes per workgroup = pairs per block
constexpr int RPS = 16;    // SoA rows per slice: loads in flight per lane
constexpr int OPL = 8;     // obs floats per lane and round

struct XferArgs {
    XferSide d, s;
    const int32_t* dst_ids;   // device, or nullptr = 0..n-1
    const int32_t* src_ids;
    uint32_t* err;            // pairs skipped (an id out of range)
    int n, dst_envs, src_envs;   // pairs; envs of the two HANDLES (the range check is the same in all three modes)
    int state_rows, aux_rows, phys_rows, obs_dim;
    int pot_row;              // index in state | aux | phys of the row to recompute (VSS-v0: ROW_PREV_POT), or -1
    float hl_goal, inv_len_cm;
};

// row r of state | aux | phys of a side (wave-uniform)
__device__ __forceinline__ uint32_t* row_of(const XferSide& sd, const XferArgs& a, const int r) {
    float* base = sd.state;
    int rr = r;
    if (r >= a.state_rows + a.aux_rows) { base = sd.phys; rr = r - a.state_rows - a.aux_rows; }
    else if (r >= a.state_rows) { base = sd.aux; rr = r - a.state_rows; }
    return reinterpret_cast<uint32_t*>(base) + (uint32_t)rr * (uint32_t)sd.stride;
}

// ids of pair i; false: skipped whole (before any access)
__device__ __forceinline__ bool pair_ids(const XferArgs& a, const int i, int& sid, int& did) {
    sid = a.src_ids ? a.src_ids[i] : i;
    did = a.dst_ids ? a.dst_ids[i] : i;
    return (unsigned)sid < (unsigned)a.src_envs && (unsigned)did < (unsigned)a.dst_envs;
}

template <int MODE>
__global__ __launch_bounds__(TPB) void transfer_kernel(const XferArgs a) {
    const int n_rows = a.state_rows + a.aux_rows + a.phys_rows;
    const int n_slices = (n_rows + RPS - 1) / RPS;
    const int y = blockIdx.y;
    const int base = blockIdx.x * TPB;
    if (y < n_slices) {
        const int i = base + (int)threadIdx.x;
        if (i >= a.n) return;
        int sid, did;
        if (!pair_ids(a, i, sid, did)) {
            if (MODE != XFER_SCATTER && y == 0) atomicAdd(a.err, 1u);   // (the scatter launch skips the pairs its gather launch counted)
            return;
        }
        const uint32_t so = MODE == XFER_SCATTER ? (uint32_t)i : (uint32_t)sid;   // a staging buffer is addressed by the pair index
        const uint32_t dof = MODE == XFER_GATHER ? (uint32_t)i : (uint32_t)did;
        const int r0 = y * RPS;
        uint32_t v[RPS];
#pragma unroll
        for (int k = 0; k < RPS; ++k)
            if (r0 + k < n_rows) v[k] = row_of(a.s, a, r0 + k)[so];
        uint8_t f0 = 0, f1 = 0;
        if (y == 0) { f0 = a.s.flags[so]; f1 = a.s.flags[(uint32_t)a.s.flag_pitch + so]; }
        if (MODE != XFER_SCATTER && a.pot_row >= r0 && a.pot_row < r0 + RPS) {
            // vss_gym.py:256-283 as the step kernels evaluate it (rsx_epl.hpp, rsx_task_step_body.inc)
            const float bx = a.s.state[so], by = a.s.state[(uint32_t)a.s.stride + so];
            const uint32_t pot = __float_as_uint(vss_ball_potential(bx, by, a.hl_goal, a.inv_len_cm));
#pragma unroll
            for (int k = 0; k < RPS; ++k) v[k] = r0 + k == a.pot_row ? pot : v[k];
        }
#pragma unroll
        for (int k = 0; k < RPS; ++k)
            if (r0 + k < n_rows) row_of(a.d, a, r0 + k)[dof] = v[k];
        if (y == 0) { a.d.flags[dof] = f0; a.d.flags[(uint32_t)a.d.flag_pitch + dof] = f1; }
        return;
    }
    // ---- obs (y == n_slices) / final_obs: the floats of this block's rows, lanes across them ----
    const bool fin = y != n_slices;
    const uint32_t* const src = reinterpret_cast<const uint32_t*>(fin ? a.s.final_obs : a.s.obs);
    uint32_t* const dst = reinterpret_cast<uint32_t*>(fin ? a.d.final_obs : a.d.obs);
    const uint32_t od = (uint32_t)a.obs_dim;
    const uint32_t total = (uint32_t)(a.n - base < TPB ? a.n - base : TPB) * od;
    for (uint32_t g0 = threadIdx.x; g0 < total; g0 += OPL * TPB) {
        uint32_t v[OPL], to[OPL];
        bool ok[OPL];
#pragma unroll
        for (int k = 0; k < OPL; ++k) {
            const uint32_t g = g0 + (uint32_t)k * TPB;
            ok[k] = false;
            if (g < total) {
                const uint32_t p = g / od, c = g - p * od;
                const int i = base + (int)p;
                int sid, did;
                ok[k] = pair_ids(a, i, sid, did);
                if (ok[k]) {
                    v[k] = src[(MODE == XFER_SCATTER ? (uint32_t)i : (uint32_t)sid) * od + c];
                    to[k] = (MODE == XFER_GATHER ? (uint32_t)i : (uint32_t)did) * od + c;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < OPL; ++k)
            if (ok[k]) dst[to[k]] = v[k];
    }
}

}  // namespace

void launch_transfer(const int mode, const XferSide& dst, const XferSide& src, const int dst_envs, const int src_envs,
                     const int32_t* dst_ids, const int32_t* src_ids, const int n, uint32_t* err, const int state_rows,
                     const int aux_rows, const int phys_rows, const int obs_dim, const int pot_row, const float hl_goal,
                     const float inv_len_cm, hipStream_t s) {
    XferArgs a{};
    a.d = dst; a.s = src;
    a.dst_ids = dst_ids; a.src_ids = src_ids; a.err = err;
    a.n = n; a.dst_envs = dst_envs; a.src_envs = src_envs;
    a.state_rows = state_rows; a.aux_rows = aux_rows; a.phys_rows = phys_rows; a.obs_dim = obs_dim;
    a.pot_row = pot_row; a.hl_goal = hl_goal; a.inv_len_cm = inv_len_cm;
    const int n_rows = state_rows + aux_rows + phys_rows;
    const dim3 grid((unsigned)((n - 1) / TPB + 1), (unsigned)((n_rows + RPS - 1) / RPS + 2));
    if (mode == XFER_GATHER) rsx_launch(transfer_kernel<XFER_GATHER>, grid, dim3(TPB), 0, s, a);
    else if (mode == XFER_SCATTER) rsx_launch(transfer_kernel<XFER_SCATTER>, grid, dim3(TPB), 0, s, a);
    else rsx_launch(transfer_kernel<XFER_DIRECT>, grid, dim3(TPB), 0, s, a);
}

}  // namespace rsx
