// rsx_ppo_update.hip — what a PPO update does around rsx_task_ppo_gradient (include/rsx.h: rsx_ppo_normalize, rsx_ppo_permutation,
// rsx_adam_step, rsx_task_ppo_update): advantage normalisation, a keyed permutation of the batch's rows, the global-norm clip with the
// Adam step, and the host loop that enqueues a whole update.  A translation unit of its own so that the instantiations of every
// existing kernel stay exactly what they were; rsx_ppo.hip is called, not changed.
//
// Every kernel here is elementwise or a reduction in a FIXED order; none uses an atomic.
//   reductions   a thread sums its elements (index ascending, stride = the grid) in float64; block_sum adds the 64 lanes of each wave in
//                ascending order and the four waves as ((w0 + w1) + w2) + w3; the workgroups' partials are added in workgroup order
//                from 0.0 by whoever needs the total.  The grids of the reducing launches are min(ceil(n / 256), a constant of the
//                build): the bits are a function of the inputs alone.
//   permutation  one thread per output index: a keyed Feistel network on the next power-of-two domain, the round function a word of
//                the engine's Philox, with cycle walking — a loop of at most 2^bits - N + 1 trips, which is what a walk on a
//                permutation's cycle can need.
//   Adam         launch 1 writes the partial sums of g^2 and (one thread) decides from the device's counters and the minibatch's
//                approx_kl whether this step is applied and which step count it carries; launch 2 folds the partials itself (thread
//                0 of every workgroup, the same chain, the same bits), derives the clip coefficient and the bias corrections and
//                updates one element per thread.  Launch 2 reads nothing of the counters, so its one writer races with nobody.
#include <hip/hip_runtime.h>

#include "rsx.h"
#include "rsx_launch.hpp"
#include "rsx_math.hpp"
#include "rsx_units.hpp"

namespace rsx {

namespace {

enum : int { UPD_THREADS = 256, NORMALIZE_WORKGROUPS = 128, GRADNORM_WORKGROUPS = 64, PERM_ROUNDS = 8, PERM_MIN_BITS = 8 };
// PERM: the round function of the row permutation, counter (half, epoch, update, PERM | round << 8), keyed by the call's seed
constexpr uint32_t DOM_PERM = 8u;

// the sum of one value per thread of a 256-thread workgroup, in every thread: lanes of a wave ascending, then the waves in order
__device__ __forceinline__ double block_sum(const double v, double* lds /* [260] */) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    if ((t & 63) == 0) {
        double acc = 0.0;
#pragma unroll 8
        for (int l = 0; l < 64; ++l) acc += lds[t + l];
        lds[UPD_THREADS + (t >> 6)] = acc;
    }
    __syncthreads();
    return ((lds[UPD_THREADS] + lds[UPD_THREADS + 1]) + lds[UPD_THREADS + 2]) + lds[UPD_THREADS + 3];
}

// ---- advantage normalisation ----
__global__ __launch_bounds__(UPD_THREADS) void adv_moments_kernel(const float* __restrict__ adv, const long long N, double* __restrict__ part) {
    __shared__ double lds[2][UPD_THREADS + 4];
    double s = 0.0, q = 0.0;
    const long long stride = (long long)gridDim.x * UPD_THREADS;
    for (long long i = (long long)blockIdx.x * UPD_THREADS + threadIdx.x; i < N; i += stride) {
        const double x = (double)adv[i];
        s += x;
        q += x * x;   // (exact: 48 bits of product)
    }
    const double S = block_sum(s, lds[0]), Q = block_sum(q, lds[1]);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = S;
        part[2 * blockIdx.x + 1] = Q;
    }
}

__global__ __launch_bounds__(UPD_THREADS) void adv_normalize_kernel(const float* __restrict__ adv, const long long N,
                                                                    const double* __restrict__ part, const int n_part, const float eps,
                                                                    float* __restrict__ out, float* __restrict__ mean_std) {
    __shared__ float ms[2];
    if (threadIdx.x == 0) {
        double S = 0.0, Q = 0.0;
        for (int g = 0; g < n_part; ++g) {
            S += part[2 * g];
            Q += part[2 * g + 1];
        }
        const double n = (double)N, mean = S / n;
        double var = (Q - S * mean) / (n - 1.0);   // (Bessel; sum (x - mean)^2 = Q - S * mean)
        if (var < 0.0) var = 0.0;
        ms[0] = (float)mean;
        ms[1] = (float)sqrt(var);
        if (blockIdx.x == 0 && mean_std != nullptr) {
            mean_std[0] = ms[0];
            mean_std[1] = ms[1];
        }
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * UPD_THREADS + threadIdx.x;
    if (i < N) out[i] = (adv[i] - ms[0]) / (ms[1] + eps);
}

// ---- the permutation ----
struct PermArgs {
    int32_t* rows;               // [N]
    const long long* update_dev; // the device's update count, or nullptr = `update`
    uint32_t N, update, epoch, k0, k1;
    int bits;                    // max(PERM_MIN_BITS, ceil(log2 N))
};

__global__ __launch_bounds__(UPD_THREADS) void permutation_kernel(const PermArgs A) {
    const uint32_t i = blockIdx.x * (uint32_t)UPD_THREADS + threadIdx.x;
    if (i >= A.N) return;
    const uint32_t upd = A.update_dev != nullptr ? (uint32_t)(unsigned long long)A.update_dev[0] : A.update;
    const uint32_t slack = (1u << A.bits) - A.N;   // domain values outside [0, N): a walk leaves them after at most that many trips
    uint32_t x = i;
#pragma nounroll
    for (uint32_t w = 0; w <= slack; ++w) {
        int wa = A.bits >> 1, wb = A.bits - wa;
        uint32_t a = x & ((1u << wa) - 1u), b = x >> wa;   // a: the low wa bits, b: the high wb bits
#pragma unroll
        for (int r = 0; r < PERM_ROUNDS; ++r) {
            const uint32_t f = philox4x32(b, A.epoch, upd, DOM_PERM | ((uint32_t)r << 8), A.k0, A.k1).x;
            const uint32_t nb = (a ^ f) & ((1u << wa) - 1u);
            a = b; b = nb;
            const int t = wa; wa = wb; wb = t;
        }
        x = a | (b << wa);
        if (x < A.N) break;
    }
    A.rows[i] = (int32_t)x;
}

// ---- global-norm clip + Adam ----
struct AdamArgs {
    float *p0, *p1, *p2;              // actor parameters, log_std, critic parameters
    const float *g0, *g1, *g2;        // their gradients
    float *m0, *m1, *m2, *v0, *v1, *v2;
    long long* counters;              // [4]: RSX_ADAM_T, _UPDATES, _APPLIED, _STOPPED
    const float* kl;                  // [1] or nullptr
    const float* lr_dev;              // [1] or nullptr
    float* stats;                     // [2] or nullptr: the norm before the clip, 1.0f when the step was applied
    double* part;                     // [GRADNORM_WORKGROUPS] partial sums of g^2 ...
    long long* gate;                  // ... and [2] behind them: the step count this step carries, whether it is withheld
    double beta1, beta2;
    int n0, n01, n;                   // the ends of the three tensors in the concatenation
    int n_part;
    float lr, eps, max_norm, target_kl;
    float b1, omb1, b2, omb2;         // the betas and 1 - beta (subtracted in float64) in float32
};

// beta^t by squaring: plain float64 multiplications in a fixed order, so that a host restatement reproduces the bits
__device__ __forceinline__ double powi(double b, long long t) {
    double r = 1.0;
    while (t > 0) {
        if (t & 1) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

__global__ __launch_bounds__(UPD_THREADS) void grad_norm_kernel(const AdamArgs A) {
    __shared__ double lds[UPD_THREADS + 4];
    double s = 0.0;
    const int stride = gridDim.x * UPD_THREADS;
    for (int e = blockIdx.x * UPD_THREADS + threadIdx.x; e < A.n; e += stride) {
        const double g = (double)(e < A.n0 ? A.g0[e] : e < A.n01 ? A.g1[e - A.n0] : A.g2[e - A.n01]);
        s += g * g;
    }
    const double S = block_sum(s, lds);
    if (threadIdx.x == 0) {
        A.part[blockIdx.x] = S;
        if (blockIdx.x == 0) {
            const long long t = A.counters[0];
            // a minibatch over the target stops the update before its own step; !(kl <= target) also stops on a NaN
            const bool over = A.kl != nullptr && A.target_kl > 0.0f && !(A.kl[0] <= A.target_kl);
            const bool stop = A.counters[3] != 0 || over;
            A.gate[0] = stop ? t : t + 1;
            A.gate[1] = stop ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(UPD_THREADS) void adam_update_kernel(const AdamArgs A) {
    __shared__ float sc[3];
    __shared__ int held;
    if (threadIdx.x == 0) {
        double S = 0.0;
        for (int g = 0; g < A.n_part; ++g) S += A.part[g];
        const float norm = (float)sqrt(S);
        float coef = 1.0f;
        if (A.max_norm > 0.0f) {
            const float c = A.max_norm / (norm + 1e-6f);
            coef = c < 1.0f ? c : 1.0f;
        }
        const long long t = A.gate[0];
        const bool stop = A.gate[1] != 0;
        const long long tt = t < 1 ? 1 : t;   // (a withheld first step: the corrections are computed and not used)
        const double bc1 = 1.0 - powi(A.beta1, tt), bc2 = 1.0 - powi(A.beta2, tt);
        const float lr = A.lr_dev != nullptr ? A.lr_dev[0] : A.lr;
        sc[0] = coef;
        sc[1] = (float)((double)lr / bc1);
        sc[2] = (float)sqrt(bc2);
        held = stop ? 1 : 0;
        if (blockIdx.x == 0) {
            A.counters[0] = t;
            A.counters[3] = stop ? 1 : 0;
            if (!stop) A.counters[2] += 1;
            if (A.stats != nullptr) {
                A.stats[0] = norm;
                A.stats[1] = stop ? 0.0f : 1.0f;
            }
        }
    }
    __syncthreads();
    const int e = blockIdx.x * UPD_THREADS + threadIdx.x;
    if (e >= A.n || held != 0) return;   // (a withheld step writes nothing: selected, not scaled by 0)
    float *p, *m, *v;
    const float* gp;
    if (e < A.n0) { p = A.p0 + e; gp = A.g0 + e; m = A.m0 + e; v = A.v0 + e; }
    else if (e < A.n01) { const int k = e - A.n0; p = A.p1 + k; gp = A.g1 + k; m = A.m1 + k; v = A.v1 + k; }
    else { const int k = e - A.n01; p = A.p2 + k; gp = A.g2 + k; m = A.m2 + k; v = A.v2 + k; }
    const float g = *gp * sc[0];
    const float mn = A.b1 * *m + A.omb1 * g;
    const float vn = A.b2 * *v + (A.omb2 * g) * g;
    *m = mn;
    *v = vn;
    *p = *p - sc[1] * (mn / (sqrtf(vn) / sc[2] + A.eps));
}

// op 0: an update begins (the steps applied and the stopped flag are cleared); op 1: it ends (the update count advances)
__global__ void update_mark_kernel(long long* counters, const int op) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (op == 0) {
        counters[2] = 0;
        counters[3] = 0;
    } else {
        counters[1] += 1;
    }
}

size_t up16(const size_t n) { return (n + 15) & ~(size_t)15; }

// the workspace of rsx_task_ppo_update (offsets in bytes)
struct UpdateWs { size_t grad, rows, adv, ga, gl, gc, adam, norm, total; };
UpdateWs update_ws(const long long na, const long long nc, const int act_dim, const long long N, const long long chunk, const int max_workgroups) {
    UpdateWs w;
    w.grad = 0;
    w.rows = up16((size_t)ppo_workspace_bytes(na, nc, act_dim, chunk, max_workgroups));
    w.adv = w.rows + up16((size_t)N * sizeof(int32_t));
    w.ga = w.adv + up16((size_t)N * sizeof(float));
    w.gl = w.ga + up16((size_t)na * sizeof(float));
    w.gc = w.gl + up16((size_t)act_dim * sizeof(float));
    w.adam = w.gc + up16((size_t)nc * sizeof(float));
    w.norm = w.adam + RSX_ADAM_WORKSPACE_BYTES;
    w.total = w.norm + RSX_PPO_NORMALIZE_WORKSPACE_BYTES;
    return w;
}

}  // namespace

void launch_ppo_normalize(const float* adv, const long long n, const float eps, float* out, float* mean_std, void* workspace, hipStream_t s) {
    static_assert(NORMALIZE_WORKGROUPS * 2 * sizeof(double) <= RSX_PPO_NORMALIZE_WORKSPACE_BYTES, "workspace");
    const long long blocks = (n + UPD_THREADS - 1) / UPD_THREADS;
    const int g1 = (int)(blocks < NORMALIZE_WORKGROUPS ? blocks : (long long)NORMALIZE_WORKGROUPS);
    double* const part = static_cast<double*>(workspace);
    rsx_launch(adv_moments_kernel, dim3((unsigned)g1), dim3(UPD_THREADS), 0, s, adv, n, part);
    rsx_launch(adv_normalize_kernel, dim3((unsigned)blocks), dim3(UPD_THREADS), 0, s, adv, n, part, g1, eps, out, mean_std);
}

void launch_ppo_permutation(int32_t* rows, const long long n, const uint64_t seed, const uint32_t update, const long long* update_dev,
                            const uint32_t epoch, hipStream_t s) {
    int bits = PERM_MIN_BITS;   // (halves of at least four bits: narrower ones mix too slowly for eight rounds)
    while ((1ll << bits) < n) ++bits;
    const PermArgs A{rows, update_dev, (uint32_t)n, update, epoch, (uint32_t)seed, (uint32_t)(seed >> 32), bits};
    rsx_launch(permutation_kernel, dim3((unsigned)((n + UPD_THREADS - 1) / UPD_THREADS)), dim3(UPD_THREADS), 0, s, A);
}

void launch_adam_step(const rsx_adam_cfg& c, const rsx_adam_state& st, const rsx_adam_io& io, hipStream_t s) {
    static_assert((GRADNORM_WORKGROUPS + 2) * sizeof(double) <= RSX_ADAM_WORKSPACE_BYTES, "workspace");
    AdamArgs A{};
    A.p0 = io.actor_params; A.p1 = io.log_std; A.p2 = io.critic_params;
    A.g0 = io.grad_actor; A.g1 = io.grad_log_std; A.g2 = io.grad_critic;
    A.m0 = st.m_actor; A.m1 = st.m_log_std; A.m2 = st.m_critic;
    A.v0 = st.v_actor; A.v1 = st.v_log_std; A.v2 = st.v_critic;
    A.counters = reinterpret_cast<long long*>(st.counters);
    A.kl = io.approx_kl; A.lr_dev = c.lr_dev; A.stats = io.stats;
    A.part = static_cast<double*>(io.workspace);
    A.gate = reinterpret_cast<long long*>(A.part + GRADNORM_WORKGROUPS);
    A.beta1 = c.beta1; A.beta2 = c.beta2;
    A.n0 = (int)st.n_actor; A.n01 = A.n0 + (int)st.n_log_std; A.n = A.n01 + (int)st.n_critic;
    const int blocks = (A.n + UPD_THREADS - 1) / UPD_THREADS;
    A.n_part = blocks < GRADNORM_WORKGROUPS ? blocks : (int)GRADNORM_WORKGROUPS;
    A.lr = c.lr; A.eps = c.eps; A.max_norm = c.max_grad_norm; A.target_kl = c.target_kl;
    A.b1 = (float)c.beta1; A.omb1 = (float)(1.0 - c.beta1); A.b2 = (float)c.beta2; A.omb2 = (float)(1.0 - c.beta2);
    rsx_launch(grad_norm_kernel, dim3((unsigned)A.n_part), dim3(UPD_THREADS), 0, s, A);
    rsx_launch(adam_update_kernel, dim3((unsigned)blocks), dim3(UPD_THREADS), 0, s, A);
}

void launch_update_mark(int64_t* counters, const int op, hipStream_t s) {
    rsx_launch(update_mark_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<long long*>(counters), op);
}

long long ppo_update_chunk(const long long n_batch_rows, const int minibatches) { return (n_batch_rows + minibatches - 1) / minibatches; }

long long ppo_update_workspace_bytes(const long long n_params_actor, const long long n_params_critic, const int act_dim,
                                     const long long n_batch_rows, const int minibatches, const int max_workgroups, long long* rows_offset) {
    const UpdateWs w = update_ws(n_params_actor, n_params_critic, act_dim, n_batch_rows, ppo_update_chunk(n_batch_rows, minibatches), max_workgroups);
    if (rows_offset != nullptr) *rows_offset = (long long)w.rows;
    return (long long)w.total;
}

void launch_ppo_update(const PolicySpec& actor, const long long n_params_actor, float* actor_params, float* log_std, const PolicySpec& critic,
                       const long long n_params_critic, float* critic_params, const int obs_dim, const int act_dim, const rsx_ppo_in& in,
                       const rsx_ppo_cfg& cfg, const rsx_ppo_update_cfg& u, const rsx_adam_cfg& adam, const rsx_adam_state& st, float* stats,
                       void* workspace, hipStream_t s) {
    const long long N = in.n_batch_rows, chunk = ppo_update_chunk(N, u.minibatches);
    const UpdateWs w = update_ws(n_params_actor, n_params_critic, act_dim, N, chunk, cfg.max_workgroups);
    char* const base = static_cast<char*>(workspace);
    int32_t* const rows = reinterpret_cast<int32_t*>(base + w.rows);
    float* const adv = reinterpret_cast<float*>(base + w.adv);
    launch_update_mark(st.counters, 0, s);
    if (u.normalize_advantage) launch_ppo_normalize(in.advantage, N, u.norm_eps, adv, nullptr, base + w.norm, s);
    rsx_ppo_in mb = in;
    mb.advantage = u.normalize_advantage ? adv : in.advantage;
    rsx_ppo_out out{};
    out.grad_actor = reinterpret_cast<float*>(base + w.ga);
    out.grad_log_std = reinterpret_cast<float*>(base + w.gl);
    out.grad_critic = reinterpret_cast<float*>(base + w.gc);
    out.workspace = base + w.grad;
    rsx_adam_io io{};
    io.actor_params = actor_params; io.log_std = log_std; io.critic_params = critic_params;
    io.grad_actor = out.grad_actor; io.grad_log_std = out.grad_log_std; io.grad_critic = out.grad_critic;
    io.workspace = base + w.adam;
    for (int e = 0; e < u.epochs; ++e) {
        // keyed by the DEVICE's update count: a replayed graph draws a new permutation on every replay
        launch_ppo_permutation(rows, N, u.seed, 0u, reinterpret_cast<const long long*>(st.counters) + 1, (uint32_t)e, s);
        for (int k = 0; k < u.minibatches; ++k) {
            float* const row = stats + ((size_t)e * (size_t)u.minibatches + (size_t)k) * RSX_PPO_UPDATE_STATS;
            const long long lo = (long long)k * chunk, hi = lo + chunk < N ? lo + chunk : N;
            mb.rows = rows + lo;
            mb.n_rows = hi - lo;
            out.stats = row;
            launch_ppo_gradient(actor, n_params_actor, actor_params, log_std, critic, n_params_critic, critic_params, obs_dim, act_dim, mb,
                                cfg, out, s);
            io.approx_kl = row + 3;
            io.stats = row + 8;
            launch_adam_step(adam, st, io, s);
        }
    }
    launch_update_mark(st.counters, 1, s);
}

}  // namespace rsx
