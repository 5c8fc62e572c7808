// rsx_gae.hip — values and GAE advantages of a collected [T][B] batch (include/rsx.h: rsx_task_advantages).  Two launches, no
// state of an env is read or written; a translation unit of its own so that the instantiations of every existing kernel stay exactly
// what they were.
//
// 1. gae_values_*_kernel: V(x) of the critic (rsx_policy_mlp.hpp's arithmetic: per unit acc = bias, then fmaf over the inputs in
//    ascending order, policy_act / tanh_f32 on the hidden layers, no activation on the output) for
//      the T * B rows of obs                 -> values[t][e]
//      the B rows of last_obs                -> advantages[T - 1][e]   (a stash: the scan reads it before it writes that row)
//      the rows truncated && !terminated of final_obs (a tail pass of the same launch, skipped by waves that hold none)
//                                            -> returns[t][e]          (a stash as well, read back by the lane that overwrites it)
//    so the call needs no memory of its own.  Two forms of the same arithmetic (the bits are the same, test_gpu_advantages.py):
//      rows    one row per lane.  The H accumulators of a layer are registers; the input is streamed: layer 1 reads the lane's row from
//              global memory (16-byte loads when obs_dim and the arrays allow, one block ahead of the arithmetic), layer 2 reads the
//              lane's hidden vector from an LDS array kept transposed ([unit][lane]: lanes on consecutive banks, private to the lane —
//              no synchronisation).  The weights of input i are one row of the transposed image stage_layer builds: the same address
//              for every lane, read as 16-byte broadcasts (sixteen reads feed 64 fmaf of 64 lanes, where hidden_layer reads one LDS
//              float per fmaf of a lane), the next input's weights in flight while the current one's fmaf issue.  One or two waves per
//              workgroup share an image: LDS leaves a SIMD one wave at most, so registers are free and latency is hidden in the wave.
//      groups  eight lanes per row, policy_forward<H, 8, 1, false> over LDS rows, as rsx_collect.hip evaluates its policy: the A/B
//              (RSX_GAE_FORM=groups; profiles/LABBOOK.md has both times).
// 2. gae_scan_kernel: one lane per env walks t downwards.  Rewards, values, flags and the stash rows do not depend on the carried
//    advantage: four steps' loads are issued ahead of the four steps' arithmetic, the recurrence is the only serial chain.
#include <hip/hip_runtime.h>

#include "rsx.h"
#include "rsx_launch.hpp"
#include "rsx_policy_mlp.hpp"
#include "rsx_units.hpp"

namespace rsx {

namespace {

struct ValueArgs {
    const float* obs;         // [T * B][OD]
    const float* last_obs;    // [B][OD]
    const float* final_obs;   // [T * B][OD] or nullptr
    const uint8_t* term;      // [T * B]
    const uint8_t* trunc;     // [T * B]
    float* values;            // [T * B]
    float* last_stash;        // [B]: row T - 1 of the advantages
    float* final_stash;       // [T * B]: the returns
    long long n_tb;           // T * B
    int n_envs, obs_dim, layers, hidden_act;
    int wide;                 // obs_dim % 4 == 0 and all three arrays 16-byte aligned: rows are read four floats at a time
};

// row r of the main pass (obs, then last_obs) / of the tail pass (final_obs of rows that were truncated only): where its input starts
// and where its value goes; false: nothing to evaluate
__device__ __forceinline__ bool main_row(const ValueArgs& A, const long long r, const float*& x, float*& dst) {
    if (r < A.n_tb) { x = A.obs + (size_t)r * (size_t)A.obs_dim; dst = A.values + r; return true; }
    const long long e = r - A.n_tb;
    if (e < (long long)A.n_envs) { x = A.last_obs + (size_t)e * (size_t)A.obs_dim; dst = A.last_stash + e; return true; }
    return false;
}
__device__ __forceinline__ bool tail_row(const ValueArgs& A, const long long r, const float*& x, float*& dst) {
    if (r < A.n_tb && A.trunc[r] != 0 && A.term[r] == 0) { x = A.final_obs + (size_t)r * (size_t)A.obs_dim; dst = A.final_stash + r; return true; }
    return false;
}

// ---- form "rows": one row per lane ----
// acc[j] = fmaf(W[j][i], xi, acc[j]) for all H units j; wrow: row i of the transposed image (16-byte aligned, the same for every lane)
template <int H>
__device__ __forceinline__ void fma_units(const float* wrow, const float xi, float (&acc)[H]) {
#pragma unroll
    for (int q = 0; q < H / 4; ++q) {
        const float4 w = reinterpret_cast<const float4*>(wrow)[q];
        acc[4 * q] = fma_(w.x, xi, acc[4 * q]);
        acc[4 * q + 1] = fma_(w.y, xi, acc[4 * q + 1]);
        acc[4 * q + 2] = fma_(w.z, xi, acc[4 * q + 2]);
        acc[4 * q + 3] = fma_(w.w, xi, acc[4 * q + 3]);
    }
}
// the same in two halves, so that the reads of the next input's weights can be in flight while this one's fmaf issue: left to itself
// the scheduler keeps one or two 16-byte reads ahead of their fmaf and the wave — the only one on its SIMD — waits out every LDS latency
template <int H>
__device__ __forceinline__ void load_weights(const float* wrow, float (&w)[H]) {
#pragma unroll
    for (int q = 0; q < H / 4; ++q) {
        const float4 v = reinterpret_cast<const float4*>(wrow)[q];
        w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
}
template <int H>
__device__ __forceinline__ void fma_loaded(const float (&w)[H], const float xi, float (&acc)[H]) {
#pragma unroll
    for (int j = 0; j < H; ++j) acc[j] = fma_(w[j], xi, acc[j]);
}
// four inputs against rows r .. r + 3 of a transposed weight matrix; wa arrives holding row r and leaves holding row r + 4 (the row
// behind a matrix is its bias in the image: readable, and dropped).  The scheduling barriers keep each group of reads in front of
// the fmaf of the previous row
template <int H>
__device__ __forceinline__ void fma_block(const float* wt, const int r, const float (&x)[4], float (&wa)[H], float (&wb)[H], float (&acc)[H]) {
    constexpr int WS = H + 4;
    load_weights<H>(wt + (r + 1) * WS, wb);
    __builtin_amdgcn_sched_barrier(0);
    fma_loaded<H>(wa, x[0], acc);
    __builtin_amdgcn_sched_barrier(0);
    load_weights<H>(wt + (r + 2) * WS, wa);
    __builtin_amdgcn_sched_barrier(0);
    fma_loaded<H>(wb, x[1], acc);
    __builtin_amdgcn_sched_barrier(0);
    load_weights<H>(wt + (r + 3) * WS, wb);
    __builtin_amdgcn_sched_barrier(0);
    fma_loaded<H>(wa, x[2], acc);
    __builtin_amdgcn_sched_barrier(0);
    load_weights<H>(wt + (r + 4) * WS, wa);
    __builtin_amdgcn_sched_barrier(0);
    fma_loaded<H>(wb, x[3], acc);
    __builtin_amdgcn_sched_barrier(0);
}
template <int H>
__device__ __forceinline__ void load_bias(const float* bias, float (&acc)[H]) {
#pragma unroll
    for (int q = 0; q < H / 4; ++q) {
        const float4 v = reinterpret_cast<const float4*>(bias)[q];
        acc[4 * q] = v.x; acc[4 * q + 1] = v.y; acc[4 * q + 2] = v.z; acc[4 * q + 3] = v.w;
    }
}
// policy_act on a layer's units, the (uniform) kind decided once and not per unit
template <int H>
__device__ __forceinline__ void activate(float (&h)[H], const int kind) {
    if (kind == RSX_ACT_RELU) {
#pragma unroll
        for (int j = 0; j < H; ++j) h[j] = policy_act(h[j], RSX_ACT_RELU);
    } else {
#pragma unroll
        for (int j = 0; j < H; ++j) h[j] = policy_act(h[j], RSX_ACT_TANH);
    }
}
// inputs i .. i + 3 of the lane's row, all inside it
__device__ __forceinline__ void load_inputs(const float* __restrict__ x, const int i, const bool wide, float (&v)[4]) {
    if (wide) {
        const float4 q = *reinterpret_cast<const float4*>(x + i);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = x[i + c];
    }
}

// V(x) of the lane's row.  hT: the lane's column of this wave's transposed hidden array ([H][64] floats, + lane)
template <int H>
__device__ __forceinline__ float value_of_row(const float* lds, const PolicyImage& m, const ValueArgs& A, const float* __restrict__ x, float* hT) {
    constexpr int WS = H + 4;
    constexpr int AHEAD = 3;   // blocks of four inputs in flight ahead of the arithmetic (a block is 4 * H fmaf: a third of a microsecond)
    const int OD = A.obs_dim;
    const bool wide = A.wide != 0;
    float h[H], wa[H], wb[H];
    load_bias<H>(lds + m.b1, h);
    {
        const float* w1 = lds + m.w1;
        const int full = OD & ~3;   // inputs in whole blocks; the one to three behind them are loaded first and used last
        float rest[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (full + c < OD) rest[c] = x[full + c];
        float q[AHEAD + 1][4] = {};
#pragma unroll
        for (int d = 0; d <= AHEAD; ++d)
            if (4 * d < full) load_inputs(x, 4 * d, wide, q[d]);
        load_weights<H>(w1, wa);
#pragma nounroll
        for (int i = 0; i < full; i += 4) {
            float cur[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) cur[c] = q[0][c];
#pragma unroll
            for (int d = 0; d < AHEAD; ++d)
#pragma unroll
                for (int c = 0; c < 4; ++c) q[d][c] = q[d + 1][c];
            if (i + 4 * (AHEAD + 1) < full) load_inputs(x, i + 4 * (AHEAD + 1), wide, q[AHEAD]);
            fma_block<H>(w1, i, cur, wa, wb, h);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (full + c < OD) fma_units<H>(w1 + (full + c) * WS, rest[c], h);
    }
    activate<H>(h, A.hidden_act);
    if (A.layers == 2) {
#pragma unroll
        for (int j = 0; j < H; ++j) hT[j * 64] = h[j];
        load_bias<H>(lds + m.b2, h);
        const float* w2 = lds + m.w2;
        load_weights<H>(w2, wa);
#pragma nounroll
        for (int i = 0; i < H; i += 4) {
            const float xs[4] = {hT[i * 64], hT[(i + 1) * 64], hT[(i + 2) * 64], hT[(i + 3) * 64]};
            fma_block<H>(w2, i, xs, wa, wb, h);
        }
        activate<H>(h, A.hidden_act);
    }
    // the output unit (act_dim = 1: its weights are consecutive floats of the image)
    float acc = lds[m.bo];
#pragma unroll
    for (int q = 0; q < H / 4; ++q) {
        const float4 w = reinterpret_cast<const float4*>(lds + m.wo)[q];
        acc = fma_(w.x, h[4 * q], acc);
        acc = fma_(w.y, h[4 * q + 1], acc);
        acc = fma_(w.z, h[4 * q + 2], acc);
        acc = fma_(w.w, h[4 * q + 3], acc);
    }
    return acc;
}

// W waves per workgroup share one image of the weights (W = 2 where that fits 64 KB: two workgroups, i.e. four waves, per CU)
template <int H, int W>
__global__ __launch_bounds__(64 * W) void gae_values_rows_kernel(const float* __restrict__ params, const ValueArgs A) {
    extern __shared__ float4 gae_lds4[];
    float* const lds = reinterpret_cast<float*>(gae_lds4);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const PolicyImage m = policy_image(0, A.obs_dim, 1, A.layers, H);   // (no rows: the image ends behind the output bias)
    const PolicyArgs Q{params, nullptr, nullptr, nullptr, 0, A.layers, H, A.hidden_act, RSX_ACT_NONE};
    if (wave == 0) stage_policy(params, lds, m, Q, A.obs_dim, 1, lane);
    float* const hT = lds + m.total + wave * (H * 64) + lane;
    if constexpr (W > 1) __syncthreads(); else wave_sync();   // the image is in place; from here on the waves go their own ways
    const long long n_main = A.n_tb + (long long)A.n_envs;
#pragma nounroll   // (one copy of the forward pass serves both passes)
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && A.final_obs == nullptr) break;
        const long long n = pass == 0 ? n_main : A.n_tb;
#pragma nounroll
        for (long long c = (long long)blockIdx.x * W + wave; c * 64 < n; c += (long long)gridDim.x * W) {
            const float* x; float* dst;
            const bool live = pass == 0 ? main_row(A, c * 64 + lane, x, dst) : tail_row(A, c * 64 + lane, x, dst);
            if (pass == 1 && !__any(live)) continue;   // truncated-only rows are rare: most waves hold none
            if (!live) x = A.obs;   // (a row that exists; its value is dropped)
            const float v = value_of_row<H>(lds, m, A, x, hT);
            if (live) *dst = v;
        }
    }
}

// ---- form "groups": eight lanes per row, the collector's policy_forward over LDS rows ----
template <int H>
__global__ __launch_bounds__(64) void gae_values_groups_kernel(const float* __restrict__ params, const ValueArgs A) {
    constexpr int L = 8, G = 8;
    extern __shared__ float4 gae_lds4[];
    float* const lds = reinterpret_cast<float*>(gae_lds4);
    const int lane = threadIdx.x, b = lane & (L - 1), g = lane / L;
    const int OD = A.obs_dim;
    const PolicyImage m = policy_image(G, OD, 1, A.layers, H);
    const PolicyArgs Q{params, nullptr, nullptr, nullptr, 0, A.layers, H, A.hidden_act, RSX_ACT_NONE};
    stage_policy(params, lds, m, Q, OD, 1, lane);
    float* const row = lds + m.rows + g * m.xs;
    wave_sync();
    const long long n_main = A.n_tb + (long long)A.n_envs;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && A.final_obs == nullptr) break;
        const long long n = pass == 0 ? n_main : A.n_tb;
        for (long long c = blockIdx.x; c * G < n; c += gridDim.x) {
            const float* x; float* dst;
            const bool live = pass == 0 ? main_row(A, c * G + g, x, dst) : tail_row(A, c * G + g, x, dst);
            if (pass == 1 && !__any(live)) continue;
            for (int i = b; i < OD; i += L) row[i] = live ? x[i] : 0.0f;
            wave_sync();
            const float v = policy_forward<H, L, 1, false>(lds, m, Q, OD, b, g);
            if (live && b == 0) *dst = v;
            wave_sync();   // the rows are read: the next trip may overwrite them
        }
    }
}

// ---- the reverse scan ----
struct ScanArgs {
    const float* rewards;      // [T][B]
    const uint8_t* term;       // [T][B]
    const uint8_t* trunc;      // [T][B]
    const float* values;       // [T][B]
    float* adv;                // [T][B]; row T - 1 arrives holding V(last_obs)
    float* ret;                // [T][B]; rows truncated only arrive holding V(final_obs) (has_final)
    float* next_values;        // [T][B] or nullptr
    int T, B, has_final;
    float gamma, gl;
};

struct ScanRow { float r, v, fin; int term, trunc; };

__device__ __forceinline__ ScanRow scan_load(const ScanArgs& S, const size_t at) {
    ScanRow w;
    w.r = S.rewards[at]; w.v = S.values[at];
    w.term = S.term[at]; w.trunc = S.trunc[at];
    w.fin = S.has_final ? S.ret[at] : 0.0f;   // (of a row that was not truncated only: whatever the array held, never selected)
    return w;
}
// one row of the recurrence of rsx.h, by selects; v_next / adv_next: the carried value and advantage of row t + 1
__device__ __forceinline__ void scan_row(const ScanArgs& S, const size_t at, const ScanRow& w, float& v_next, float& adv_next) {
    const bool term = w.term != 0, end = term || w.trunc != 0;
    const float nv = term ? 0.0f : (end ? w.fin : v_next);
    const float delta = (w.r + S.gamma * nv) - w.v;
    const float carried = delta + S.gl * adv_next;
    const float adv = end ? delta : carried;
    S.adv[at] = adv;
    S.ret[at] = adv + w.v;
    if (S.next_values != nullptr) S.next_values[at] = nv;
    v_next = w.v; adv_next = adv;
}

__global__ __launch_bounds__(64) void gae_scan_kernel(const ScanArgs S) {
    constexpr int U = 4;
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= S.B) return;
    const size_t B = (size_t)S.B;
    int t = S.T - 1;
    float v_next = S.adv[(size_t)t * B + e];   // V(last_obs[e])
    float adv_next = 0.0f;
    for (; ((t + 1) & (U - 1)) != 0; --t) {   // the rows above the last multiple of U
        const size_t at = (size_t)t * B + e;
        scan_row(S, at, scan_load(S, at), v_next, adv_next);
    }
    for (; t >= 0; t -= U) {
        ScanRow w[U];
#pragma unroll
        for (int k = 0; k < U; ++k) w[k] = scan_load(S, (size_t)(t - k) * B + e);
#pragma unroll
        for (int k = 0; k < U; ++k) scan_row(S, (size_t)(t - k) * B + e, w[k], v_next, adv_next);
    }
}

// workgroups of a values launch: one per trip of rows_per_trip rows, at most `resident` (what 256 CUs hold at once by LDS: a workgroup
// stages the image once and walks the rows with that stride)
int values_grid(const long long rows_per_trip, const long long n_rows, const int resident) {
    const long long trips = (n_rows + rows_per_trip - 1) / rows_per_trip;
    return (int)(trips < resident ? trips : resident);
}
long long rows_lds_bytes(const int waves, const int obs_dim, const PolicySpec& c) {
    return (long long)sizeof(float) * (policy_image(0, obs_dim, 1, c.layers, c.hidden).total + (c.layers == 2 ? waves * c.hidden * 64 : 0));
}

}  // namespace

long long gae_lds_bytes(const int form, const int obs_dim, const PolicySpec& c) {
    if (form == GAE_FORM_GROUPS) return (long long)sizeof(float) * policy_image(8, obs_dim, 1, c.layers, c.hidden).total;
    return rows_lds_bytes(1, obs_dim, c);   // (the smallest form of the rows kernel: one wave per workgroup)
}

void launch_advantages(const int form, const PolicySpec& c, const float* params, const int obs_dim, const float gamma, const float gl,
                       const int T, const int B, const rsx_adv_in& in, const rsx_adv_out& out, hipStream_t s) {
    const long long n_tb = (long long)T * (long long)B;
    const auto aligned16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    const int wide = obs_dim % 4 == 0 && aligned16(in.obs) && aligned16(in.last_obs) && aligned16(in.final_obs);
    const ValueArgs A{in.obs, in.last_obs, in.final_obs, in.terminated, in.truncated, out.values, out.advantages + (size_t)(T - 1) * (size_t)B,
                      out.returns, n_tb, B, obs_dim, c.layers, c.hidden_act, wide};
    if (form == GAE_FORM_GROUPS) {
        const size_t lds = (size_t)gae_lds_bytes(form, obs_dim, c);
        const int grid = values_grid(8, n_tb + B, 768);
        if (c.hidden == 64) rsx_launch(gae_values_groups_kernel<64>, dim3((unsigned)grid), dim3(64), lds, s, params, A);
        else rsx_launch(gae_values_groups_kernel<32>, dim3((unsigned)grid), dim3(64), lds, s, params, A);
    } else if (rows_lds_bytes(2, obs_dim, c) <= 65536ll) {
        const size_t lds = (size_t)rows_lds_bytes(2, obs_dim, c);
        const int grid = values_grid(128, n_tb + B, 512);
        if (c.hidden == 64) rsx_launch((gae_values_rows_kernel<64, 2>), dim3((unsigned)grid), dim3(128), lds, s, params, A);
        else rsx_launch((gae_values_rows_kernel<32, 2>), dim3((unsigned)grid), dim3(128), lds, s, params, A);
    } else {
        const size_t lds = (size_t)rows_lds_bytes(1, obs_dim, c);
        const int grid = values_grid(64, n_tb + B, 768);
        if (c.hidden == 64) rsx_launch((gae_values_rows_kernel<64, 1>), dim3((unsigned)grid), dim3(64), lds, s, params, A);
        else rsx_launch((gae_values_rows_kernel<32, 1>), dim3((unsigned)grid), dim3(64), lds, s, params, A);
    }
    const ScanArgs S{in.rewards, in.terminated, in.truncated, out.values, out.advantages, out.returns, out.next_values, T, B,
                     in.final_obs != nullptr ? 1 : 0, gamma, gl};
    rsx_launch(gae_scan_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, S);
}

}  // namespace rsx
