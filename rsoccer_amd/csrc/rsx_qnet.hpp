// rsx_qnet.hpp — the row kernels' device pieces that rsx_dpg.hip (TD3 / DDPG gradients) and rsx_sac.hip (soft actor-critic gradients)
// share: one network evaluated one row per lane from its transposed LDS image (rsx_policy_mlp's arithmetic), its backward pass on a block
// of 64 entries with the hidden layers' weight gradients on the f32 MFMA continuing ONE running partial per workgroup, the float64 block
// sums of the bias gradients, the stats fold, the sums of the reduce and the grant of dynamic LDS beyond 64 KB.  Moved here from
// rsx_dpg.hip word for word, so that unit's kernels are what they were; the scheme is rsx_ppo.hip's (that unit stays untouched and keeps
// its own copy of the small pieces).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

#include "rsx.h"
#include "rsx_launch.hpp"
#include "rsx_policy_mlp.hpp"

namespace rsx {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

enum : int { DPG_PART_STATS = 8, DPG_MAX_ACT = 8 };   // the stats terms of a partial; the widest action

// ---- rsx_ppo.hip's device pieces ----
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
__device__ __forceinline__ float act_deriv(const float h, const int kind) {
    return kind == RSX_ACT_RELU ? (h > 0.0f ? 1.0f : 0.0f) : fma_(-h, h, 1.0f);
}
// one tile of a weight gradient: units u0 .. u0 + 31 x inputs i0 .. i0 + 31 of W [n_out][n_in] (the workgroup's partial); av / bv: the
// MFMA operands of the 32 k-steps, step s holding rows 2 s (lanes 0 .. 31) and 2 s + 1 (lanes 32 .. 63) of the block
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
__device__ __forceinline__ void operand_lds(const float* buf, const int pitch, const int col, const int lane, float (&v)[32]) {
    const float* p = buf + (lane >> 5) * pitch + col;
#pragma unroll
    for (int s = 0; s < 32; ++s) v[s] = p[2 * s * pitch];
}
// db[j]: the running partial plus the block's 64 terms buf[r][col], r ascending, summed in float64 and rounded to float32 ONCE per
// trip (one lane per unit).  Unlike rsx_ppo.hip's float32 chain: a critic's output bias gradient is the scalar mean(Q - y), whose
// terms cancel; a float32 chain rounds at every partial sum of that random walk (measured on 63 rows with |mean| 1 / 46 of mean |.|:
// 2.4e-6 relative with the float32 chain, 1.05e-6 with this sum, 6.8e-7 of it the forward passes' own error)
__device__ __forceinline__ void bias_grad(float* b, const float* buf, const int pitch, const int col, const bool first) {
    double acc = first ? 0.0 : (double)*b;
#pragma unroll 8
    for (int r = 0; r < 64; ++r) acc += (double)buf[r * pitch + col];
    *b = (float)acc;
}

// ---- one network, one row per lane ----
// the hidden layers on the input row [x[0 .. OD) | ext[0 .. n_ext)]: rsx_policy_mlp's arithmetic (per unit acc = bias, ascending fmaf).
// Two layers: h1 goes to the lane's row `arow` of an LDS array [64][H + 4]; the top activations end in h
template <int H>
__device__ __forceinline__ void forward_hidden(const float* img, const PolicyImage& m, const int layers, const int kind,
                                               const float* __restrict__ x, const int OD, const int wide, const float (&ext)[DPG_MAX_ACT],
                                               const int n_ext, float* arow, float (&h)[H]) {
    constexpr int WS = H + 4;
    load_vec<H>(img + m.b1, h);
    const float* w1 = img + m.w1;
    int i = 0;
#pragma nounroll
    for (; i + 4 <= OD; i += 4) {
        float xv[4];
        if (wide) {
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
#pragma unroll
    for (int k = 0; k < DPG_MAX_ACT; ++k)
        if (k < n_ext) fma_row<H>(w1 + (OD + k) * WS, ext[k], h);
    activate<H>(h, kind);
    if (layers == 2) {
        store_vec<H>(arow, h);
        load_vec<H>(img + m.b2, h);
        const float* w2 = img + m.w2;
#pragma nounroll
        for (int j = 0; j < H; j += 4) {
            const float4 q = *reinterpret_cast<const float4*>(arow + j);   // (the lane's own row: no synchronisation)
            fma_row<H>(w2 + j * WS, q.x, h);
            fma_row<H>(w2 + (j + 1) * WS, q.y, h);
            fma_row<H>(w2 + (j + 2) * WS, q.z, h);
            fma_row<H>(w2 + (j + 3) * WS, q.w, h);
        }
        activate<H>(h, kind);
    }
}
// output unit a: acc = bias, ascending fmaf over the top activations
template <int H>
__device__ __forceinline__ float output_unit(const float* img, const PolicyImage& m, const int a, const float (&h)[H]) {
    float acc = img[m.bo + a];
#pragma unroll
    for (int i = 0; i < H; ++i) acc = fma_(img[m.wo + i * m.as + a], h[i], acc);
    return acc;
}

// where the input rows of a block's first layer come from, for the B operand of its weight gradient
struct InputRows {
    const float* obs;   // [N][OD]
    const float* ext;   // [N][n_ext] or nullptr
    int OD, n_ext;
};

// the backward pass of one network on a block: O [64][OP] holds dL/d(output) (0 for a dead lane), h the lane's top activations, A
// [64][H + 4] h1 of two layers.  WEIGHTS: the gradients continue the workgroup's running partial `part` (torch's layout: W1 [H][n_in],
// b1, (W2 [H][H], b2,) Wo [n_out][H], bo).  On return A holds dz of the first layer
template <int H, bool WEIGHTS>
__device__ __forceinline__ void backward(const float* img, const PolicyImage& m, const int layers, const int kind, float* A, float* D,
                                         const float* O, const int OP, const int n_out, float (&h)[H], const bool live, const bool first,
                                         const int lane, float* part, const InputRows& X, const int* idxs) {
    constexpr int WS = H + 4, AP = H + 4, DP = 33, NS = H / 32;
    const int n_in = X.OD + X.n_ext;
    float* const pW1 = part;
    float* const pb1 = pW1 + H * n_in;
    float* const pW2 = pb1 + H;
    float* const pb2 = pW2 + (layers == 2 ? H * H : 0);
    float* const pWo = layers == 2 ? pb2 + H : pW2;
    float* const pbo = pWo + n_out * H;
    wave_sync();   // O is complete
    if constexpr (WEIGHTS) {
        // ---- the output layer's gradient: the top activations pass through D in slices of 32 units ----
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int q = 0; q < 32; ++q) D[lane * DP + q] = h[32 * s + q];
            wave_sync();
            if (lane < 32) {
#pragma nounroll
                for (int a = 0; a < n_out; ++a) {
                    float* w = pWo + a * H + 32 * s + lane;
                    float acc = first ? 0.0f : *w;
#pragma unroll 8
                    for (int r = 0; r < 64; ++r) acc = fma_(O[r * OP + a], D[r * DP + lane], acc);
                    *w = acc;
                }
            }
            wave_sync();
        }
        if (lane < n_out) bias_grad(pbo + lane, O, OP, lane, first);
    }
    // ---- dz of the top hidden layer, in h ----
    {
        float g[H];
#pragma unroll
        for (int j = 0; j < H; ++j) g[j] = 0.0f;
#pragma nounroll
        for (int a = 0; a < n_out; ++a) {
            const float d = O[lane * OP + a];
#pragma unroll
            for (int j = 0; j < H; ++j) g[j] = fma_(img[m.wo + j * m.as + a], d, g[j]);
        }
#pragma unroll
        for (int j = 0; j < H; ++j) h[j] = live ? g[j] * act_deriv(h[j], kind) : 0.0f;
    }
    if (layers == 2) {
        if constexpr (WEIGHTS) {
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
        }
        // ---- dz1 = (W2^T dz2) * act'(h1), in place of h1 ----
        const float* w2 = img + m.w2;
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
    if constexpr (WEIGHTS) {
        // ---- W1, b1: dz1 in A against the input rows ----
#pragma nounroll
        for (int i0 = 0; i0 < n_in; i0 += 32) {
            float av[32], bv[32];
            const int col = i0 + (lane & 31);
#pragma unroll
            for (int s = 0; s < 32; ++s) {
                const int row = idxs[2 * s + (lane >> 5)];
                float v = 0.0f;
                if (col < X.OD) v = X.obs[(size_t)row * (size_t)X.OD + col];
                else if (col < n_in) v = X.ext[(size_t)row * (size_t)X.n_ext + (col - X.OD)];
                bv[s] = v;
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                operand_lds(A, AP, 32 * s + (lane & 31), lane, av);
                wgrad_tile(pW1, n_in, 32 * s, i0, first, lane, av, bv);
            }
        }
        if (lane < H) bias_grad(pb1 + lane, A, AP, lane, first);
        wave_sync();   // A, D, O and idxs are read: the next trip may overwrite them
    }
}

// the workgroup's stats terms: per-lane sums, then the lanes in ascending order (A: at least [64][8] floats)
__device__ __forceinline__ void fold_stats(float* A, float* pst, const int lane, const float st0, const float st1, const float st2,
                                           const float st3, const int used, const int skipped) {
    wave_sync();
    A[lane * 8 + 0] = st0; A[lane * 8 + 1] = st1; A[lane * 8 + 2] = st2; A[lane * 8 + 3] = st3;
    A[lane * 8 + 4] = __int_as_float(used); A[lane * 8 + 5] = __int_as_float(skipped);
    A[lane * 8 + 6] = 0.0f; A[lane * 8 + 7] = 0.0f;
    wave_sync();
    if (lane < DPG_PART_STATS) {
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

struct Net {
    const float* params;   // [P] (critics: [C][P])
    int n_params, layers, hidden_act, out_act;
};

__host__ __device__ inline int max_i(const int a, const int b) { return a > b ? a : b; }

__device__ __forceinline__ PolicyArgs stage_args(const Net& n, const int H) {
    return PolicyArgs{n.params, nullptr, nullptr, nullptr, 0, n.layers, H, n.hidden_act, n.out_act};
}

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

// dynamic LDS beyond 64 KB is the kernel's to be granted first: once per kernel (ID) and device, and again for a larger image
template <int ID>
void grant_lds(const void* kernel, const size_t lds) {
    static std::atomic<int> granted[64];
    int dev = 0;
    if (lds > 65536 && hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 && granted[dev].load(std::memory_order_relaxed) < (int)lds) {
        const hipError_t rc = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (rc == hipSuccess) granted[dev].store((int)lds, std::memory_order_relaxed);
        else if (g_launch_status == hipSuccess) g_launch_status = rc;
    }
}

inline long long round4ll(const long long n) { return (n + 3) & ~3ll; }

}  // namespace

}  // namespace rsx
