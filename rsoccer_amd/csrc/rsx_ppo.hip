// rsx_ppo.hip — gradients of the PPO loss of include/rsx.h (rsx_task_ppo_gradient) with respect to an MLP actor, its log_std and an
// MLP critic.  Three launches, no state of an env is read or written; a translation unit of its own so that the instantiations of
// every existing kernel stay exactly what they were.
//
// 1. / 2. mlp_grad_kernel<H, HEAD>, once for the actor (HEAD_ACTOR: the Gaussian head and the clipped surrogate) and once for the
//    critic (HEAD_CRITIC: the squared error).  One wave per workgroup; a workgroup walks blocks of 64 minibatch rows with the stride of
//    the grid and keeps ONE running partial gradient [P] (and its stats terms) in the workspace.  Per block:
//      gather    lane r takes minibatch row block * 64 + r through `rows`; an index outside [0, N) (and a lane behind M) evaluates
//                row 0 instead and its every derivative is SELECTED to zero, so nothing outside the arrays is read.
//      forward   one row per lane, rsx_policy_mlp.hpp's arithmetic (per unit acc = bias, ascending fmaf, policy_act): the H
//                accumulators of a layer are registers, the weights of input i one row of the transposed image stage_layer builds, read
//                as 16-byte LDS broadcasts (rsx_gae.hip's scheme).  The activations of hidden layer 1 go to the LDS array A
//                ([row][H + 4]), those of the top hidden layer stay in registers.
//      head      dL/dmean (dL/dvalue) of the lane's row into the LDS array O ([row][act_dim | 1]), the stats terms and the row's
//                log_std derivative into per-lane sums.
//      backward  dz = (W^T d(next)) * act' per lane: the output weights against O, the second layer's image rows against the lane's
//                dz2 registers (four partial sums per input, combined (s0 + s1) + (s2 + s3)).  dz1 replaces h1 in A.
//      weights   dW[j][i] += sum over the block's rows of dz[r][j] * in[r][i] on v_mfma_f32_32x32x2_f32, a tile of 32 units x 32
//                inputs at a time: the MFMA's A operand is dz (lane -> unit), its B operand the layer's input (lane -> input; h1 from A,
//                the observation from global memory), K walks the block's rows in ascending order, and the accumulator STARTS as
//                the workgroup's running partial.  An MFMA on f32 is a k-ordered fmaf chain, so a partial is one fmaf chain over all
//                rows of its workgroup, in the order the workgroup met them.  dz2 passes through the LDS array D in slices of 32
//                units ([row][33]), which is what keeps two layers of 64 units at 64 observation floats inside 64 KB.
//                Bias gradients and the output layer's weight gradient (act_dim rows) are plain fmaf chains of the lanes 0 .. 31
//                over the block's rows, continuing the running partial the same way.
//    Every lane re-reads only what it wrote itself of the partial, so the read-modify-write needs no ordering beyond the program's.
// 3. ppo_reduce_kernel: one thread per output element sums the partials in workgroup order from 0.0f; one more thread folds the stats.
// The grid of the row launches is min(ceil(M / 64), max_workgroups): the bits depend on the inputs and that number alone.
#include <hip/hip_runtime.h>

#include "rsx.h"
#include "rsx_launch.hpp"
#include "rsx_policy_mlp.hpp"
#include "rsx_units.hpp"

namespace rsx {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

enum : int { HEAD_ACTOR = 0, HEAD_CRITIC = 1 };
enum : int { PPO_STATS = 8, PPO_DEFAULT_WORKGROUPS = 512 };   // (two workgroups per CU by LDS on 256 CUs; a constant, not the device's)
// the stats terms of a partial.  actor: 0 sum of -min(.), 1 sum of (ratio - 1) - log ratio, 2 rows outside the clip bounds, 3 sum of
// ratio, 4 rows used (int bits), 5 rows skipped (int bits).  critic: 0 sum of (value - ret)^2

struct GradArgs {
    const float* params;     // [P]
    const float* log_std;    // [act_dim]   (actor)
    const float* obs;        // [N][obs_dim]
    const float* sample;     // [N][act_dim] (actor)
    const float* old_lp;     // [N]          (actor)
    const float* adv;        // [N]          (actor)
    const float* ret;        // [N]          (critic)
    const int32_t* rows;     // [M] or nullptr
    float* part;             // [grid][stride]: weights [P], (actor: log_std [act_dim],) stats [PPO_STATS]
    float* fwd_out;          // [M][act_dim] or nullptr
    long long N, M;
    int stride, n_params;
    int obs_dim, act_dim, layers, hidden_act;
    int wide;                // obs_dim % 4 == 0 and obs 16-byte aligned: rows are read four floats at a time
    float clip_lo, clip_hi;  // 1 - clip, 1 + clip in float32
    float coef;              // critic: vf_coef
    float inv_m;             // 1.0f / M
};

// what one workgroup keeps in LDS behind the image of its network (offsets in floats)
struct GradLds { int A, D, O, LS, idx, sg, total; };
__host__ __device__ inline GradLds grad_lds(const PolicyImage& m, const int H, const int AD) {
    GradLds g;
    const int op = AD | 1;
    g.A = m.rows;                 // [64][H + 4]: h1, then dz1 (one layer: dz of the only layer); the final stats fold
    g.D = g.A + 64 * (H + 4);     // [64][33]: a slice of 32 units of the top activations, then of dz2
    g.O = g.D + 64 * 33;          // [64][op]: the mean, then dL/dmean
    g.LS = g.O + 64 * op;         // [64][op]: per-lane sums of the log_std derivative
    g.idx = g.LS + 64 * op;       // [64] int: the rows of the block
    g.sg = g.idx + 64;            // [2][round4(AD)]: log_std, sigma
    g.total = g.sg + 2 * round4(AD);
    return g;
}

template <int H>
__device__ __forceinline__ void load_vec(const float* p, float (&v)[H]) {
#pragma unroll
    for (int q = 0; q < H / 4; ++q) {
        const float4 w = reinterpret_cast<const float4*>(p)[q];
        v[4 * q] = w.x; v[4 * q + 1] = w.y; v[4 * q + 2] = w.z; v[4 * q + 3] = w.w;
    }
}
template <int H>
__device__ __forceinline__ void store_vec(float* p, const float (&v)[H]) {
#pragma unroll
    for (int q = 0; q < H / 4; ++q) reinterpret_cast<float4*>(p)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}
// acc[j] = fmaf(W[j][i], xi, acc[j]) for all H units j; wrow: row i of the transposed image (the same address for every lane)
template <int H>
__device__ __forceinline__ void fma_row(const float* wrow, const float xi, float (&acc)[H]) {
#pragma unroll
    for (int q = 0; q < H / 4; ++q) {
        const float4 w = reinterpret_cast<const float4*>(wrow)[q];
        acc[4 * q] = fma_(w.x, xi, acc[4 * q]);
        acc[4 * q + 1] = fma_(w.y, xi, acc[4 * q + 1]);
        acc[4 * q + 2] = fma_(w.z, xi, acc[4 * q + 2]);
        acc[4 * q + 3] = fma_(w.w, xi, acc[4 * q + 3]);
    }
}
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
// the activation's derivative from the stored activation
__device__ __forceinline__ float act_deriv(const float h, const int kind) {
    return kind == RSX_ACT_RELU ? (h > 0.0f ? 1.0f : 0.0f) : fma_(-h, h, 1.0f);
}

// one tile of a weight gradient: units u0 .. u0 + 31 x inputs i0 .. i0 + 31 of W [n_out][n_in] (the workgroup's partial).  av / bv: the
// MFMA operands of the 32 k-steps, step s holding rows 2 s (lanes 0 .. 31) and 2 s + 1 (lanes 32 .. 63) of the block:
// av[s] = dz[row][u0 + (lane & 31)], bv[s] = in[row][i0 + (lane & 31)] (0 behind n_in).  The result has its input on the lane
// (lane & 31) and its unit in the register: unit = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
__device__ __forceinline__ void wgrad_tile(float* W, const int n_in, const int u0, const int i0, const bool first, const int lane,
                                           const float (&av)[32], const float (&bv)[32]) {
    const int col = i0 + (lane & 31), hi = lane >> 5;
    const bool in_range = col < n_in;
    f32x16 c;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int unit = u0 + (reg & 3) + 8 * (reg >> 2) + 4 * hi;
        c[reg] = (!first && in_range) ? W[unit * n_in + col] : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < 32; ++s) c = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], c, 0, 0, 0);
    if (in_range) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int unit = u0 + (reg & 3) + 8 * (reg >> 2) + 4 * hi;
            W[unit * n_in + col] = c[reg];
        }
    }
}
// column `col` of an LDS array [64][pitch] as an MFMA operand (see wgrad_tile)
__device__ __forceinline__ void operand_lds(const float* buf, const int pitch, const int col, const int lane, float (&v)[32]) {
    const float* p = buf + (lane >> 5) * pitch + col;
#pragma unroll
    for (int s = 0; s < 32; ++s) v[s] = p[2 * s * pitch];
}
// db[j] += sum over the block's rows of buf[r][col], r ascending, continuing the running partial (one lane per unit)
__device__ __forceinline__ void bias_grad(float* b, const float* buf, const int pitch, const int col, const bool first) {
    float acc = first ? 0.0f : *b;
#pragma unroll 8
    for (int r = 0; r < 64; ++r) acc += buf[r * pitch + col];
    *b = acc;
}

template <int H, int HEAD>
__global__ __launch_bounds__(64) void mlp_grad_kernel(const float* __restrict__ params, const GradArgs G) {
    constexpr int WS = H + 4, AP = H + 4, DP = 33, NS = H / 32;
    extern __shared__ float4 ppo_lds4[];
    float* const lds = reinterpret_cast<float*>(ppo_lds4);
    const int lane = threadIdx.x;
    const int OD = G.obs_dim, AD = G.act_dim, OP = AD | 1, kind = G.hidden_act;
    const PolicyImage m = policy_image(0, OD, AD, G.layers, H);   // (no rows: the image ends behind the output bias)
    const GradLds L = grad_lds(m, H, AD);
    const PolicyArgs Q{params, nullptr, nullptr, nullptr, 0, G.layers, H, kind, RSX_ACT_NONE};
    stage_policy(params, lds, m, Q, OD, AD, lane);
    float* const A = lds + L.A;
    float* const D = lds + L.D;
    float* const O = lds + L.O;
    float* const LS = lds + L.LS;
    int* const idxs = reinterpret_cast<int*>(lds + L.idx);
    float* const lsv = lds + L.sg;
    float* const sgv = lsv + round4(AD);
    if (HEAD == HEAD_ACTOR && lane < AD) {
        const float ls = G.log_std[lane];
        lsv[lane] = ls;
        sgv[lane] = expf(ls);
    }
    for (int a = 0; a < AD; ++a) LS[lane * OP + a] = 0.0f;
    wave_sync();

    float* const part = G.part + (size_t)blockIdx.x * (size_t)G.stride;
    // the partial in torch's layout: W1 [H][OD], b1, (W2 [H][H], b2,) Wo [AD][H], bo
    float* const pW1 = part;
    float* const pb1 = pW1 + H * OD;
    float* const pW2 = pb1 + H;
    float* const pb2 = pW2 + (G.layers == 2 ? H * H : 0);
    float* const pWo = G.layers == 2 ? pb2 + H : pW2;
    float* const pbo = pWo + AD * H;

    float st0 = 0.0f, st1 = 0.0f, st2 = 0.0f, st3 = 0.0f;
    int used = 0, skipped = 0;
    bool first = true;
#pragma nounroll
    for (long long blk = blockIdx.x; blk * 64 < G.M; blk += gridDim.x, first = false) {
        // ---- gather ----
        const long long t = blk * 64 + lane;
        const bool in_m = t < G.M;
        long long idx = 0;
        if (in_m) idx = G.rows != nullptr ? (long long)G.rows[t] : t;
        const bool live = in_m && idx >= 0 && idx < G.N;
        if (!live) idx = 0;   // (a row that exists; everything it contributes is selected away)
        used += live ? 1 : 0;
        skipped += (in_m && !live) ? 1 : 0;
        idxs[lane] = (int)idx;
        const float* __restrict__ x = G.obs + (size_t)idx * (size_t)OD;

        // ---- forward ----
        float h[H];
        load_vec<H>(lds + m.b1, h);
        {
            const float* w1 = lds + m.w1;
            int i = 0;
#pragma nounroll
            for (; i + 4 <= OD; i += 4) {
                float xv[4];
                if (G.wide) {
                    const float4 q = *reinterpret_cast<const float4*>(x + i);
                    xv[0] = q.x; xv[1] = q.y; xv[2] = q.z; xv[3] = q.w;
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) xv[c] = x[i + c];
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) fma_row<H>(w1 + (i + c) * WS, xv[c], h);
            }
#pragma nounroll
            for (; i < OD; ++i) fma_row<H>(w1 + i * WS, x[i], h);
        }
        activate<H>(h, kind);
        if (G.layers == 2) {
            store_vec<H>(A + lane * AP, h);
            load_vec<H>(lds + m.b2, h);
            const float* w2 = lds + m.w2;
#pragma nounroll
            for (int i = 0; i < H; i += 4) {
                const float4 q = *reinterpret_cast<const float4*>(A + lane * AP + i);   // (the lane's own row: no synchronisation)
                fma_row<H>(w2 + i * WS, q.x, h);
                fma_row<H>(w2 + (i + 1) * WS, q.y, h);
                fma_row<H>(w2 + (i + 2) * WS, q.z, h);
                fma_row<H>(w2 + (i + 3) * WS, q.w, h);
            }
            activate<H>(h, kind);
        }
        // the output layer: unit a's weights are lds[m.wo + i * m.as + a]
#pragma nounroll
        for (int a = 0; a < AD; ++a) {
            float acc = lds[m.bo + a];
#pragma unroll
            for (int i = 0; i < H; ++i) acc = fma_(lds[m.wo + i * m.as + a], h[i], acc);
            O[lane * OP + a] = acc;
            if (G.fwd_out != nullptr && in_m) G.fwd_out[(size_t)t * (size_t)AD + a] = live ? acc : 0.0f;
        }

        // ---- head: O := dL/d(output) ----
        if constexpr (HEAD == HEAD_ACTOR) {
            float lp = 0.0f;
#pragma nounroll
            for (int a = 0; a < AD; ++a) {
                const float z = (G.sample[(size_t)idx * (size_t)AD + a] - O[lane * OP + a]) / sgv[a];
                const float term = ((-0.5f * z) * z - lsv[a]) - 0.9189385332046727f;
                lp = a == 0 ? term : lp + term;
            }
            const float logr = lp - G.old_lp[idx];
            const float ratio = expf(logr);
            const float adv = G.adv[idx];
            const float s1 = ratio * adv, s2 = clampf(ratio, G.clip_lo, G.clip_hi) * adv;
            const bool inside = ratio >= G.clip_lo && ratio <= G.clip_hi;
            const bool open = inside || s1 < s2;
            const float dlp = (live && open) ? (-(adv * G.inv_m)) * ratio : 0.0f;   // dL/dlp
#pragma nounroll
            for (int a = 0; a < AD; ++a) {
                const float sg = sgv[a];
                const float z = (G.sample[(size_t)idx * (size_t)AD + a] - O[lane * OP + a]) / sg;
                O[lane * OP + a] = live ? dlp * (z / sg) : 0.0f;
                LS[lane * OP + a] += live ? dlp * fma_(z, z, -1.0f) : 0.0f;
            }
            if (live) {
                st0 += -fminf(s1, s2);
                st1 += (ratio - 1.0f) - logr;
                st2 += inside ? 0.0f : 1.0f;
                st3 += ratio;
            }
        } else {
            const float diff = O[lane * OP] - G.ret[idx];
            O[lane * OP] = live ? (diff * G.coef) * G.inv_m : 0.0f;
            if (live) st0 += diff * diff;
        }
        wave_sync();

        // ---- the output layer's gradient: the top activations pass through D in slices of 32 units ----
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int q = 0; q < 32; ++q) D[lane * DP + q] = h[32 * s + q];
            wave_sync();
            if (lane < 32) {
#pragma nounroll
                for (int a = 0; a < AD; ++a) {
                    float* w = pWo + a * H + 32 * s + lane;
                    float acc = first ? 0.0f : *w;
#pragma unroll 8
                    for (int r = 0; r < 64; ++r) acc = fma_(O[r * OP + a], D[r * DP + lane], acc);
                    *w = acc;
                }
            }
            wave_sync();
        }
        if (lane < AD) bias_grad(pbo + lane, O, OP, lane, first);

        // ---- dz of the top hidden layer, in h ----
        {
            float g[H];
#pragma unroll
            for (int j = 0; j < H; ++j) g[j] = 0.0f;
#pragma nounroll
            for (int a = 0; a < AD; ++a) {
                const float d = O[lane * OP + a];
#pragma unroll
                for (int j = 0; j < H; ++j) g[j] = fma_(lds[m.wo + j * m.as + a], d, g[j]);
            }
#pragma unroll
            for (int j = 0; j < H; ++j) h[j] = live ? g[j] * act_deriv(h[j], kind) : 0.0f;
        }

        if (G.layers == 2) {
            // ---- W2, b2: dz2 through D in slices, against h1 in A ----
#pragma unroll
            for (int s = 0; s < NS; ++s) {
#pragma unroll
                for (int q = 0; q < 32; ++q) D[lane * DP + q] = h[32 * s + q];
                wave_sync();
                {
                    float av[32], bv[32];
                    operand_lds(D, DP, lane & 31, lane, av);
#pragma unroll
                    for (int ib = 0; ib < NS; ++ib) {
                        operand_lds(A, AP, 32 * ib + (lane & 31), lane, bv);
                        wgrad_tile(pW2, H, 32 * s, 32 * ib, first, lane, av, bv);
                    }
                }
                if (lane < 32) bias_grad(pb2 + 32 * s + lane, D, DP, lane, first);
                wave_sync();
            }
            // ---- dz1 = (W2^T dz2) * act'(h1), in place of h1 ----
            const float* w2 = lds + m.w2;
#pragma unroll 2
            for (int i = 0; i < H; ++i) {
                float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
                for (int q = 0; q < H / 4; ++q) {
                    const float4 w = reinterpret_cast<const float4*>(w2 + i * WS)[q];
                    s0 = fma_(w.x, h[4 * q], s0);
                    s1 = fma_(w.y, h[4 * q + 1], s1);
                    s2 = fma_(w.z, h[4 * q + 2], s2);
                    s3 = fma_(w.w, h[4 * q + 3], s3);
                }
                const float dh = (s0 + s1) + (s2 + s3);
                const float h1 = A[lane * AP + i];
                A[lane * AP + i] = live ? dh * act_deriv(h1, kind) : 0.0f;
            }
        } else {
            store_vec<H>(A + lane * AP, h);
        }
        wave_sync();

        // ---- W1, b1: dz1 in A against the observations ----
#pragma nounroll
        for (int i0 = 0; i0 < OD; i0 += 32) {
            float av[32], bv[32];
            const int col = i0 + (lane & 31);
#pragma unroll
            for (int s = 0; s < 32; ++s) {
                const int row = idxs[2 * s + (lane >> 5)];
                bv[s] = col < OD ? G.obs[(size_t)row * (size_t)OD + col] : 0.0f;
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                operand_lds(A, AP, 32 * s + (lane & 31), lane, av);
                wgrad_tile(pW1, OD, 32 * s, i0, first, lane, av, bv);
            }
        }
        if (lane < H) bias_grad(pb1 + lane, A, AP, lane, first);
        wave_sync();   // A, D, O and idxs are read: the next trip may overwrite them
    }

    // ---- the workgroup's log_std and stats terms: lanes in ascending order ----
    float* const pls = part + G.n_params;
    if constexpr (HEAD == HEAD_ACTOR) {
        if (lane < AD) {
            float acc = 0.0f;
            for (int r = 0; r < 64; ++r) acc += LS[r * OP + lane];
            pls[lane] = acc;
        }
    }
    float* const pst = pls + (HEAD == HEAD_ACTOR ? AD : 0);
    A[lane * 8 + 0] = st0; A[lane * 8 + 1] = st1; A[lane * 8 + 2] = st2; A[lane * 8 + 3] = st3;
    A[lane * 8 + 4] = __int_as_float(used); A[lane * 8 + 5] = __int_as_float(skipped);
    A[lane * 8 + 6] = 0.0f; A[lane * 8 + 7] = 0.0f;
    wave_sync();
    if (lane < PPO_STATS) {
        if (lane == 4 || lane == 5) {
            int acc = 0;
            for (int r = 0; r < 64; ++r) acc += __float_as_int(A[r * 8 + lane]);
            pst[lane] = __int_as_float(acc);
        } else {
            float acc = 0.0f;
            for (int r = 0; r < 64; ++r) acc += A[r * 8 + lane];
            pst[lane] = acc;
        }
    }
}

struct ReduceArgs {
    const float* part_a;     // [grid][stride_a]
    const float* part_c;     // [grid][stride_c]
    const float* log_std;    // [AD]
    float* grad_a;           // [Pa]
    float* grad_ls;          // [AD]
    float* grad_c;           // [Pc]
    float* stats;            // [8]
    int grid, stride_a, stride_c, Pa, Pc, AD;
    float inv_m, ent_coef;
};

__device__ __forceinline__ float sum_partials(const float* p, const int n, const int stride) {
    float acc = 0.0f;
#pragma unroll 8
    for (int g = 0; g < n; ++g) acc += p[(size_t)g * (size_t)stride];
    return acc;
}
__device__ __forceinline__ int sum_partials_int(const float* p, const int n, const int stride) {
    int acc = 0;
    for (int g = 0; g < n; ++g) acc += __float_as_int(p[(size_t)g * (size_t)stride]);
    return acc;
}

__global__ __launch_bounds__(256) void ppo_reduce_kernel(const ReduceArgs R) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int n_a = R.Pa + R.AD, n = n_a + R.Pc;
    if (e < R.Pa) {
        R.grad_a[e] = sum_partials(R.part_a + e, R.grid, R.stride_a);
    } else if (e < n_a) {
        R.grad_ls[e - R.Pa] = sum_partials(R.part_a + e, R.grid, R.stride_a) - R.ent_coef;   // (d(-ent_coef * entropy) / dlog_std = -ent_coef)
    } else if (e < n) {
        R.grad_c[e - n_a] = sum_partials(R.part_c + (e - n_a), R.grid, R.stride_c);
    } else if (e == n) {
        const float* sa = R.part_a + n_a;
        const float* sc = R.part_c + R.Pc;
        float ent = 0.0f;
        for (int a = 0; a < R.AD; ++a) {
            const float term = (R.log_std[a] + 0.5f) + 0.9189385332046727f;
            ent = a == 0 ? term : ent + term;
        }
        R.stats[0] = sum_partials(sa + 0, R.grid, R.stride_a) * R.inv_m;
        R.stats[1] = (0.5f * sum_partials(sc + 0, R.grid, R.stride_c)) * R.inv_m;
        R.stats[2] = ent;
        R.stats[3] = sum_partials(sa + 1, R.grid, R.stride_a) * R.inv_m;
        R.stats[4] = sum_partials(sa + 2, R.grid, R.stride_a) * R.inv_m;
        R.stats[5] = sum_partials(sa + 3, R.grid, R.stride_a) * R.inv_m;
        R.stats[6] = (float)sum_partials_int(sa + 4, R.grid, R.stride_a);
        R.stats[7] = (float)sum_partials_int(sa + 5, R.grid, R.stride_a);
    }
}

int stride_of(const long long n_params, const int extra) { return (int)(n_params + extra + PPO_STATS); }

template <int HEAD>
void launch_grad(const PolicySpec& c, const int grid, const size_t lds, hipStream_t s, const GradArgs& G) {
    if (c.hidden == 64) rsx_launch((mlp_grad_kernel<64, HEAD>), dim3((unsigned)grid), dim3(64), lds, s, G.params, G);
    else rsx_launch((mlp_grad_kernel<32, HEAD>), dim3((unsigned)grid), dim3(64), lds, s, G.params, G);
}

}  // namespace

long long ppo_lds_bytes(const int obs_dim, const int act_dim, const PolicySpec& c) {
    return (long long)sizeof(float) * grad_lds(policy_image(0, obs_dim, act_dim, c.layers, c.hidden), c.hidden, act_dim).total;
}

int ppo_grid(const long long n_rows, const int max_workgroups) {
    const long long trips = (n_rows + 63) / 64;
    const long long cap = max_workgroups > 0 ? max_workgroups : (int)PPO_DEFAULT_WORKGROUPS;
    return (int)(trips < cap ? trips : cap);
}

long long ppo_workspace_bytes(const long long n_params_actor, const long long n_params_critic, const int act_dim, const long long n_rows,
                              const int max_workgroups) {
    return (long long)sizeof(float) * ppo_grid(n_rows, max_workgroups) *
           ((long long)stride_of(n_params_actor, act_dim) + stride_of(n_params_critic, 0));
}

void launch_ppo_gradient(const PolicySpec& actor, const long long n_params_actor, const float* actor_params, const float* log_std,
                         const PolicySpec& critic, const long long n_params_critic, const float* critic_params, const int obs_dim,
                         const int act_dim, const rsx_ppo_in& in, const rsx_ppo_cfg& cfg, const rsx_ppo_out& out, hipStream_t s) {
    const int grid = ppo_grid(in.n_rows, cfg.max_workgroups);
    const int stride_a = stride_of(n_params_actor, act_dim), stride_c = stride_of(n_params_critic, 0);
    float* const part_a = static_cast<float*>(out.workspace);
    float* const part_c = part_a + (size_t)grid * (size_t)stride_a;
    const int wide = obs_dim % 4 == 0 && (reinterpret_cast<uintptr_t>(in.obs) & 15u) == 0;
    const float inv_m = 1.0f / (float)in.n_rows;
    GradArgs G{};
    G.obs = in.obs; G.sample = in.sample; G.old_lp = in.old_log_prob; G.adv = in.advantage; G.ret = in.ret; G.rows = in.rows;
    G.N = in.n_batch_rows; G.M = in.n_rows;
    G.obs_dim = obs_dim; G.wide = wide;
    G.clip_lo = 1.0f - cfg.clip; G.clip_hi = 1.0f + cfg.clip; G.inv_m = inv_m;
    // the actor
    G.params = actor_params; G.log_std = log_std; G.part = part_a; G.fwd_out = out.mean;
    G.stride = stride_a; G.n_params = (int)n_params_actor; G.act_dim = act_dim; G.layers = actor.layers; G.hidden_act = actor.hidden_act;
    G.coef = 0.0f;
    launch_grad<HEAD_ACTOR>(actor, grid, (size_t)ppo_lds_bytes(obs_dim, act_dim, actor), s, G);
    // the critic
    G.params = critic_params; G.log_std = nullptr; G.part = part_c; G.fwd_out = out.value;
    G.stride = stride_c; G.n_params = (int)n_params_critic; G.act_dim = 1; G.layers = critic.layers; G.hidden_act = critic.hidden_act;
    G.coef = cfg.vf_coef;
    launch_grad<HEAD_CRITIC>(critic, grid, (size_t)ppo_lds_bytes(obs_dim, 1, critic), s, G);
    const ReduceArgs R{part_a, part_c, log_std, out.grad_actor, out.grad_log_std, out.grad_critic, out.stats, grid, stride_a, stride_c,
                       (int)n_params_actor, (int)n_params_critic, act_dim, inv_m, cfg.ent_coef};
    const int n = (int)(n_params_actor + act_dim + n_params_critic) + 1;
    rsx_launch(ppo_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, R);
}

}  // namespace rsx
