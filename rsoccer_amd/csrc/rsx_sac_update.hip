// rsx_sac_update.hip — what a soft actor-critic gradient step does around rsx_task_sac_gradient (include/rsx.h: rsx_sac_adam_step,
// rsx_task_sac_update): the three-group clip + Adam step (critics, actor, the scalar log-temperature) with the Polyak step of the target
// critics behind it, and the host loop that enqueues a whole update phase.  A translation unit of its own so that the instantiations of
// every existing kernel stay exactly what they were; rsx_sac.hip, rsx_dpg_update.hip and rsx_ppo_update.hip are not changed.  The row draw
// is rsx_dpg_update.hip's launch_replay_sample_rows and the gradients rsx_sac.hip's launch_sac_gradient, both called through
// rsx_units.hpp; this unit draws nothing itself.
//
// Both kernels are elementwise or a reduction in a FIXED order; neither uses an atomic.
//   reductions   rsx_dpg_update.hip's, restated (block_sum, powi, fold_norm and the per-element Adam line are stated once more here, as
//                that unit did for rsx_ppo_update.hip: a shared header would have to leave its kernels' code untouched): a thread sums its
//                elements (index ascending, stride = its group's grid) in float64; block_sum adds the 64 lanes of each wave ascending and
//                the four waves as ((w0 + w1) + w2) + w3; the partials of a GROUP are added in workgroup order from 0.0.  The critics'
//                tensor and the actor's are two groups with partials, norms, clip coefficients and step counts of their own; one launch
//                reduces both (the critics' workgroups first)
//   Adam         launch 1 writes the partials and (one thread) takes the three step counts this step carries from the device's counters
//                into the workspace; launch 2 folds its group's partials in thread 0 of every workgroup (the same chain, the same
//                bits), updates one element per thread and, with update_targets, moves a critic element's target towards the NEW
//                parameter.  Launch 2 reads nothing of the counters, so their one writer races with nobody.
//   log_alpha    a group of one element without a clip: thread 0 of workgroup 0 of launch 2 — the counters' writer — steps it with the same
//                line and its own step count; no workgroup of its own
#include <hip/hip_runtime.h>

#include "rsx.h"
#include "rsx_launch.hpp"
#include "rsx_units.hpp"

namespace rsx {

namespace {

enum : int { UPD_THREADS = 256, GRADNORM_WORKGROUPS = 64 };

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

// group 0: the critics [n_c]; group 1: the actor [n_a]; group 2: log_alpha [1]
struct SacAdamArgs {
    float *pc, *pa, *pl, *tc;            // live parameters (critics, actor, log_alpha), the target critics
    const float *gc, *ga, *gl;           // gradients; ga == nullptr: no actor step; gl == nullptr: no temperature step
    float *mc, *ma, *ml, *vc, *va, *vl;
    long long* counters;                 // [4]: RSX_SAC_T_CRITIC, _T_ACTOR, _T_ALPHA, _STEPS
    const float *lrc_dev, *lra_dev, *lrl_dev;   // [1] or nullptr
    float* stats;                        // [4] or nullptr
    double* part;                        // [2 * GRADNORM_WORKGROUPS]: the critics' partial sums of g^2, the actor's ...
    long long* gate;                     // ... and [3] behind them: the step counts this step carries
    double beta1, beta2;
    int n_c, n_a;
    int part_c, part_a;                  // workgroups of the norm launch per group (part_a = 0: no actor step)
    int blocks_c;                        // workgroups of the update launch that belong to the critics; the actor's follow
    int polyak;                          // update_targets
    float lrc, lra, lrl, eps, max_norm, tau;
    float b1, omb1, b2, omb2;            // the betas and 1 - beta (subtracted in float64) in float32
};

__global__ __launch_bounds__(UPD_THREADS) void sac_grad_norm_kernel(const SacAdamArgs A) {
    __shared__ double lds[UPD_THREADS + 4];
    const bool actor = (int)blockIdx.x >= A.part_c;
    const int w = actor ? (int)blockIdx.x - A.part_c : (int)blockIdx.x;
    const int n = actor ? A.n_a : A.n_c;
    const float* const g = actor ? A.ga : A.gc;
    const int stride = (actor ? A.part_a : A.part_c) * UPD_THREADS;
    double s = 0.0;
    for (int e = w * UPD_THREADS + threadIdx.x; e < n; e += stride) {
        const double x = (double)g[e];
        s += x * x;
    }
    const double S = block_sum(s, lds);
    if (threadIdx.x == 0) {
        A.part[(actor ? GRADNORM_WORKGROUPS : 0) + w] = S;
        if (blockIdx.x == 0) {
            A.gate[0] = A.counters[RSX_SAC_T_CRITIC] + 1;
            A.gate[1] = A.ga != nullptr ? A.counters[RSX_SAC_T_ACTOR] + 1 : A.counters[RSX_SAC_T_ACTOR];
            A.gate[2] = A.gl != nullptr ? A.counters[RSX_SAC_T_ALPHA] + 1 : A.counters[RSX_SAC_T_ALPHA];
        }
    }
}

__device__ __forceinline__ float fold_norm(const double* part, const int n_part) {
    double S = 0.0;
    for (int g = 0; g < n_part; ++g) S += part[g];
    return (float)sqrt(S);
}

// one element's Adam step with its group's clip coefficient c, step = (float)(lr / bc1) and s2 = (float)sqrt(bc2); returns the new value
__device__ __forceinline__ float adam_element(const SacAdamArgs& A, float* const p, float* const m, float* const v, const float grad,
                                              const float c, const float step, const float s2) {
    const float g = grad * c;
    const float mn = A.b1 * *m + A.omb1 * g;
    const float vn = A.b2 * *v + (A.omb2 * g) * g;
    *m = mn;
    *v = vn;
    const float pn = *p - step * (mn / (sqrtf(vn) / s2 + A.eps));
    *p = pn;
    return pn;
}

__global__ __launch_bounds__(UPD_THREADS) void sac_adam_update_kernel(const SacAdamArgs A) {
    __shared__ float sc[3];
    const bool actor = (int)blockIdx.x >= A.blocks_c;   // (the actor's workgroups exist on an actor step only: it has no target)
    if (threadIdx.x == 0) {
        const float norm = fold_norm(A.part + (actor ? GRADNORM_WORKGROUPS : 0), actor ? A.part_a : A.part_c);
        float coef = 1.0f;
        if (A.max_norm > 0.0f) {
            const float c = A.max_norm / (norm + 1e-6f);
            coef = c < 1.0f ? c : 1.0f;
        }
        const long long t = A.gate[actor ? 1 : 0];
        const double bc1 = 1.0 - powi(A.beta1, t), bc2 = 1.0 - powi(A.beta2, t);
        const float* const lr_dev = actor ? A.lra_dev : A.lrc_dev;
        const float lr = lr_dev != nullptr ? lr_dev[0] : actor ? A.lra : A.lrc;
        sc[0] = coef;
        sc[1] = (float)((double)lr / bc1);
        sc[2] = (float)sqrt(bc2);
        if (blockIdx.x == 0) {
            // the scalar group: never clipped (coef = 1), its own t, its own lr
            float la = A.pl[0];
            if (A.gl != nullptr) {
                const long long tl = A.gate[2];
                const double l1 = 1.0 - powi(A.beta1, tl), l2 = 1.0 - powi(A.beta2, tl);
                const float lrl = A.lrl_dev != nullptr ? A.lrl_dev[0] : A.lrl;
                la = adam_element(A, A.pl, A.ml, A.vl, A.gl[0], 1.0f, (float)((double)lrl / l1), (float)sqrt(l2));
            }
            A.counters[RSX_SAC_T_CRITIC] = A.gate[0];
            A.counters[RSX_SAC_T_ACTOR] = A.gate[1];
            A.counters[RSX_SAC_T_ALPHA] = A.gate[2];
            A.counters[RSX_SAC_STEPS] += 1;
            if (A.stats != nullptr) {
                A.stats[0] = norm;
                A.stats[1] = A.ga != nullptr ? fold_norm(A.part + GRADNORM_WORKGROUPS, A.part_a) : 0.0f;
                A.stats[2] = la;
                A.stats[3] = A.polyak ? 1.0f : 0.0f;
            }
        }
    }
    __syncthreads();
    const int e = (actor ? (int)blockIdx.x - A.blocks_c : (int)blockIdx.x) * UPD_THREADS + threadIdx.x;
    if (e >= (actor ? A.n_a : A.n_c)) return;
    const float pn = adam_element(A, (actor ? A.pa : A.pc) + e, (actor ? A.ma : A.mc) + e, (actor ? A.va : A.vc) + e,
                                  (actor ? A.ga : A.gc)[e], sc[0], sc[1], sc[2]);
    if (A.polyak && !actor) {
        float* const targ = A.tc + e;
        const float d = pn - *targ;
        *targ = *targ + A.tau * d;
    }
}

size_t up16(const size_t n) { return (n + 15) & ~(size_t)15; }

// the workspace of rsx_task_sac_update (offsets in bytes)
struct UpdateWs { size_t grad, rows, ga, gc, gl, adam, total; };
UpdateWs update_ws(const long long na, const long long nc, const int n_critics, const long long m, const int max_workgroups) {
    UpdateWs w;
    w.grad = 0;
    w.rows = up16((size_t)sac_workspace_bytes(na, nc, n_critics, m, max_workgroups));
    w.ga = w.rows + up16((size_t)m * sizeof(int32_t));
    w.gc = w.ga + up16((size_t)na * sizeof(float));
    w.gl = w.gc + up16((size_t)n_critics * (size_t)nc * sizeof(float));
    w.adam = w.gl + 16;
    w.total = w.adam + RSX_SAC_ADAM_WORKSPACE_BYTES;
    return w;
}

}  // namespace

void launch_sac_adam_step(const rsx_sac_adam_cfg& c, const rsx_sac_adam_state& st, const rsx_sac_adam_io& io, hipStream_t s) {
    static_assert((2 * GRADNORM_WORKGROUPS + 3) * sizeof(double) <= RSX_SAC_ADAM_WORKSPACE_BYTES, "workspace");
    SacAdamArgs A{};
    A.pc = io.critic_params; A.pa = io.actor_params; A.pl = io.log_alpha; A.tc = io.target_critic_params;
    A.gc = io.grad_critic; A.ga = io.grad_actor; A.gl = io.grad_log_alpha;
    A.mc = st.m_critic; A.ma = st.m_actor; A.ml = st.m_alpha; A.vc = st.v_critic; A.va = st.v_actor; A.vl = st.v_alpha;
    A.counters = reinterpret_cast<long long*>(st.counters);
    A.lrc_dev = c.lr_critic_dev; A.lra_dev = c.lr_actor_dev; A.lrl_dev = c.lr_alpha_dev; A.stats = io.stats;
    A.part = static_cast<double*>(io.workspace);
    A.gate = reinterpret_cast<long long*>(A.part + 2 * GRADNORM_WORKGROUPS);
    A.beta1 = c.beta1; A.beta2 = c.beta2;
    A.n_c = (int)st.n_critic; A.n_a = (int)st.n_actor;
    const int blocks_c = (A.n_c + UPD_THREADS - 1) / UPD_THREADS, blocks_a = (A.n_a + UPD_THREADS - 1) / UPD_THREADS;
    const bool actor = io.grad_actor != nullptr;
    A.part_c = blocks_c < GRADNORM_WORKGROUPS ? blocks_c : (int)GRADNORM_WORKGROUPS;
    A.part_a = !actor ? 0 : blocks_a < GRADNORM_WORKGROUPS ? blocks_a : (int)GRADNORM_WORKGROUPS;
    A.blocks_c = blocks_c;
    A.polyak = io.update_targets != 0 ? 1 : 0;
    A.lrc = c.lr_critic; A.lra = c.lr_actor; A.lrl = c.lr_alpha; A.eps = c.eps; A.max_norm = c.max_grad_norm; A.tau = c.tau;
    A.b1 = (float)c.beta1; A.omb1 = (float)(1.0 - c.beta1); A.b2 = (float)c.beta2; A.omb2 = (float)(1.0 - c.beta2);
    rsx_launch(sac_grad_norm_kernel, dim3((unsigned)(A.part_c + A.part_a)), dim3(UPD_THREADS), 0, s, A);
    rsx_launch(sac_adam_update_kernel, dim3((unsigned)(blocks_c + (actor ? blocks_a : 0))), dim3(UPD_THREADS), 0, s, A);
}

long long sac_update_workspace_bytes(const long long n_params_actor, const long long n_params_critic, const int n_critics, const long long n_rows,
                                     const int max_workgroups, long long* rows_offset) {
    const UpdateWs w = update_ws(n_params_actor, n_params_critic, n_critics, n_rows, max_workgroups);
    if (rows_offset != nullptr) *rows_offset = (long long)w.rows;
    return (long long)w.total;
}

void launch_sac_update(const PolicySpec& actor, const long long n_params_actor, float* actor_params, const PolicySpec& critic,
                       const long long n_params_critic, float* critic_params, float* target_critic_params, float* log_alpha,
                       const int obs_dim, const int act_dim, const rsx_dpg_in& in, const rsx_sac_cfg& cfg, const rsx_sac_update_cfg& u,
                       const rsx_sac_adam_cfg& adam, const rsx_sac_adam_state& st, float* stats, void* workspace, hipStream_t s) {
    const long long m = in.n_rows;
    const UpdateWs w = update_ws(n_params_actor, n_params_critic, cfg.n_critics, m, cfg.max_workgroups);
    char* const base = static_cast<char*>(workspace);
    int32_t* const rows = reinterpret_cast<int32_t*>(base + w.rows);
    // keyed by the DEVICE's count of finished gradient steps: a replayed graph draws new rows and new noise on every replay
    const long long* const steps = reinterpret_cast<const long long*>(st.counters) + RSX_SAC_STEPS;
    rsx_dpg_in mb = in;
    mb.rows = rows;
    rsx_sac_cfg gcfg = cfg;
    gcfg.noise_step_dev = reinterpret_cast<const int64_t*>(steps);
    rsx_sac_out out{};
    out.grad_actor = reinterpret_cast<float*>(base + w.ga);
    out.grad_critics = reinterpret_cast<float*>(base + w.gc);
    out.grad_log_alpha = reinterpret_cast<float*>(base + w.gl);
    out.workspace = base + w.grad;
    rsx_sac_adam_io io{};
    io.actor_params = actor_params; io.critic_params = critic_params; io.target_critic_params = target_critic_params;
    io.log_alpha = log_alpha;
    io.grad_actor = out.grad_actor; io.grad_critic = out.grad_critics;
    io.grad_log_alpha = u.learn_alpha != 0 ? out.grad_log_alpha : nullptr;
    io.workspace = base + w.adam;
    io.update_targets = 1;
    for (int j = 0; j < u.grad_steps; ++j) {
        float* const row = stats + (size_t)j * RSX_SAC_UPDATE_STATS;
        launch_replay_sample_rows(rows, m, in.n_batch_rows, u.fill, reinterpret_cast<const long long*>(u.fill_dev), u.seed, 0, steps, s);
        out.stats = row;
        launch_sac_gradient(actor, n_params_actor, actor_params, critic, n_params_critic, critic_params, target_critic_params, log_alpha,
                            obs_dim, act_dim, mb, gcfg, out, s);
        io.stats = row + 12;
        launch_sac_adam_step(adam, st, io, s);
    }
}

}  // namespace rsx
