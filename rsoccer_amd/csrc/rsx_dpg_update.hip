// rsx_dpg_update.hip — what a TD3 / DDPG gradient step does around rsx_task_dpg_gradient (include/rsx.h: rsx_replay_sample_rows,
// rsx_dpg_adam_step, rsx_task_dpg_update): the minibatch's rows drawn from the engine's Philox, the two-group clip + Adam step with the
// Polyak step of the targets behind it, and the host loop that enqueues a whole update phase.  A translation unit of its own so that the
// instantiations of every existing kernel stay exactly what they were; rsx_dpg.hip and rsx_ppo_update.hip are not changed.
//
// Every kernel here is elementwise or a reduction in a FIXED order; none uses an atomic.
//   rows         one thread per entry: a word of a Philox block scaled into [0, fill) by a 32 x 32 -> 64 bit multiply, no float
//   reductions   rsx_ppo_update.hip's, restated: a thread sums its elements (index ascending, stride = its group's grid) in float64;
//                block_sum adds the 64 lanes of each wave ascending and the four waves as ((w0 + w1) + w2) + w3; the partials of a
//                GROUP are added in workgroup order from 0.0.  The critics' tensor and the actor's are two groups with partials,
//                norms, clip coefficients and step counts of their own; one launch reduces both (the critics' workgroups first)
//   Adam         launch 1 writes the partials and (one thread) takes the two step counts this step carries from the device's counters
//                into the workspace; launch 2 folds its group's partials in thread 0 of every workgroup (the same chain, the same
//                bits), updates one element per thread and, with update_targets, moves that element's target towards the NEW
//                parameter.  Launch 2 reads nothing of the counters, so their one writer races with nobody.
#include <hip/hip_runtime.h>

#include "rsx.h"
#include "rsx_launch.hpp"
#include "rsx_math.hpp"
#include "rsx_units.hpp"

namespace rsx {

namespace {

enum : int { UPD_THREADS = 256, GRADNORM_WORKGROUPS = 64 };
// ROWS: the replayed minibatch's rows, counter (entry >> 2, step hi, step lo, ROWS), keyed by the call's seed
// (rsx_math.hpp: 1, 3 .. 7; rsx_ppo_update.hip: 8; rsx_selfplay.hip: 9; rsx_dpg.hip: 10)
constexpr uint32_t DOM_ROWS = 11u;

// ---- the rows ----
struct RowsArgs {
    int32_t* rows;               // [m]
    const long long* fill_dev;   // the device's fill count, or nullptr = `fill`
    const long long* step_dev;   // the device's step, or nullptr = `step`
    long long fill, step, N;
    uint32_t m, k0, k1;
};

__global__ __launch_bounds__(UPD_THREADS) void sample_rows_kernel(const RowsArgs A) {
    const uint32_t t = blockIdx.x * (uint32_t)UPD_THREADS + threadIdx.x;
    if (t >= A.m) return;
    long long fill = A.fill_dev != nullptr ? A.fill_dev[0] : A.fill;
    fill = fill < 0 ? 0 : fill > A.N ? A.N : fill;
    if (fill == 0) {
        A.rows[t] = -1;
        return;
    }
    const unsigned long long step = (unsigned long long)(A.step_dev != nullptr ? A.step_dev[0] : A.step);
    const u32x4 u = philox4x32(t >> 2, (uint32_t)(step >> 32), (uint32_t)step, DOM_ROWS, A.k0, A.k1);
    const uint32_t k = t & 3u;
    const uint32_t word = k == 0u ? u.x : k == 1u ? u.y : k == 2u ? u.z : u.w;
    A.rows[t] = (int32_t)(uint32_t)(((unsigned long long)word * (unsigned long long)fill) >> 32);   // (< fill <= 2^31 - 1)
}

// ---- global-norm clip + Adam on two groups, and the Polyak step ----
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

// group 0: the critics [n_c]; group 1: the actor [n_a]
struct DpgAdamArgs {
    float *pc, *pa, *tc, *ta;         // live parameters, targets
    const float *gc, *ga;             // gradients; ga == nullptr: no actor step
    float *mc, *ma, *vc, *va;
    long long* counters;              // [4]: RSX_DPG_T_CRITIC, _T_ACTOR, _STEPS, spare
    const float *lrc_dev, *lra_dev;   // [1] or nullptr
    float* stats;                     // [3] or nullptr
    double* part;                     // [2 * GRADNORM_WORKGROUPS]: the critics' partial sums of g^2, the actor's ...
    long long* gate;                  // ... and [2] behind them: the step counts this step carries
    double beta1, beta2;
    int n_c, n_a;
    int part_c, part_a;               // workgroups of the norm launch per group (part_a = 0: no actor step)
    int blocks_c;                     // workgroups of the update launch that belong to the critics; the actor's follow
    int polyak;                       // update_targets
    float lrc, lra, eps, max_norm, tau;
    float b1, omb1, b2, omb2;         // the betas and 1 - beta (subtracted in float64) in float32
};

__global__ __launch_bounds__(UPD_THREADS) void dpg_grad_norm_kernel(const DpgAdamArgs A) {
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
            A.gate[0] = A.counters[0] + 1;
            A.gate[1] = A.ga != nullptr ? A.counters[1] + 1 : A.counters[1];
        }
    }
}

__device__ __forceinline__ float fold_norm(const double* part, const int n_part) {
    double S = 0.0;
    for (int g = 0; g < n_part; ++g) S += part[g];
    return (float)sqrt(S);
}

__global__ __launch_bounds__(UPD_THREADS) void dpg_adam_update_kernel(const DpgAdamArgs A) {
    __shared__ float sc[3];
    const bool actor = (int)blockIdx.x >= A.blocks_c;
    const bool adam = !actor || A.ga != nullptr;   // (the actor's workgroups of a critic-only step move its target only)
    if (threadIdx.x == 0) {
        const float norm = adam ? fold_norm(A.part + (actor ? GRADNORM_WORKGROUPS : 0), actor ? A.part_a : A.part_c) : 0.0f;
        float coef = 1.0f;
        if (A.max_norm > 0.0f) {
            const float c = A.max_norm / (norm + 1e-6f);
            coef = c < 1.0f ? c : 1.0f;
        }
        const long long t = A.gate[actor ? 1 : 0];
        const long long tt = t < 1 ? 1 : t;   // (an actor that never stepped: the corrections are computed and not used)
        const double bc1 = 1.0 - powi(A.beta1, tt), bc2 = 1.0 - powi(A.beta2, tt);
        const float* const lr_dev = actor ? A.lra_dev : A.lrc_dev;
        const float lr = lr_dev != nullptr ? lr_dev[0] : actor ? A.lra : A.lrc;
        sc[0] = coef;
        sc[1] = (float)((double)lr / bc1);
        sc[2] = (float)sqrt(bc2);
        if (blockIdx.x == 0) {
            A.counters[0] = A.gate[0];
            A.counters[1] = A.gate[1];
            A.counters[2] += 1;
            if (A.stats != nullptr) {
                A.stats[0] = norm;
                A.stats[1] = A.ga != nullptr ? fold_norm(A.part + GRADNORM_WORKGROUPS, A.part_a) : 0.0f;
                A.stats[2] = A.polyak ? 1.0f : 0.0f;
            }
        }
    }
    __syncthreads();
    const int e = (actor ? (int)blockIdx.x - A.blocks_c : (int)blockIdx.x) * UPD_THREADS + threadIdx.x;
    if (e >= (actor ? A.n_a : A.n_c)) return;
    float* const p = (actor ? A.pa : A.pc) + e;
    float pn = *p;
    if (adam) {
        float* const m = (actor ? A.ma : A.mc) + e;
        float* const v = (actor ? A.va : A.vc) + e;
        const float g = (actor ? A.ga : A.gc)[e] * sc[0];
        const float mn = A.b1 * *m + A.omb1 * g;
        const float vn = A.b2 * *v + (A.omb2 * g) * g;
        *m = mn;
        *v = vn;
        pn = pn - sc[1] * (mn / (sqrtf(vn) / sc[2] + A.eps));
        *p = pn;
    }
    if (A.polyak) {
        float* const targ = (actor ? A.ta : A.tc) + e;
        const float d = pn - *targ;
        *targ = *targ + A.tau * d;
    }
}

size_t up16(const size_t n) { return (n + 15) & ~(size_t)15; }

// the workspace of rsx_task_dpg_update (offsets in bytes)
struct UpdateWs { size_t grad, rows, ga, gc, adam, total; };
UpdateWs update_ws(const long long na, const long long nc, const int n_critics, const long long m, const int max_workgroups) {
    UpdateWs w;
    w.grad = 0;
    w.rows = up16((size_t)dpg_workspace_bytes(na, nc, n_critics, m, max_workgroups));
    w.ga = w.rows + up16((size_t)m * sizeof(int32_t));
    w.gc = w.ga + up16((size_t)na * sizeof(float));
    w.adam = w.gc + up16((size_t)n_critics * (size_t)nc * sizeof(float));
    w.total = w.adam + RSX_DPG_ADAM_WORKSPACE_BYTES;
    return w;
}

}  // namespace

void launch_replay_sample_rows(int32_t* rows, const long long m, const long long n_batch_rows, const long long fill, const long long* fill_dev,
                               const uint64_t seed, const long long step, const long long* step_dev, hipStream_t s) {
    const RowsArgs A{rows, fill_dev, step_dev, fill, step, n_batch_rows, (uint32_t)m, (uint32_t)seed, (uint32_t)(seed >> 32)};
    rsx_launch(sample_rows_kernel, dim3((unsigned)((m + UPD_THREADS - 1) / UPD_THREADS)), dim3(UPD_THREADS), 0, s, A);
}

void launch_dpg_adam_step(const rsx_dpg_adam_cfg& c, const rsx_dpg_adam_state& st, const rsx_dpg_adam_io& io, hipStream_t s) {
    static_assert((2 * GRADNORM_WORKGROUPS + 2) * sizeof(double) <= RSX_DPG_ADAM_WORKSPACE_BYTES, "workspace");
    DpgAdamArgs A{};
    A.pc = io.critic_params; A.pa = io.actor_params; A.tc = io.target_critic_params; A.ta = io.target_actor_params;
    A.gc = io.grad_critic; A.ga = io.grad_actor;
    A.mc = st.m_critic; A.ma = st.m_actor; A.vc = st.v_critic; A.va = st.v_actor;
    A.counters = reinterpret_cast<long long*>(st.counters);
    A.lrc_dev = c.lr_critic_dev; A.lra_dev = c.lr_actor_dev; A.stats = io.stats;
    A.part = static_cast<double*>(io.workspace);
    A.gate = reinterpret_cast<long long*>(A.part + 2 * GRADNORM_WORKGROUPS);
    A.beta1 = c.beta1; A.beta2 = c.beta2;
    A.n_c = (int)st.n_critic; A.n_a = (int)st.n_actor;
    const int blocks_c = (A.n_c + UPD_THREADS - 1) / UPD_THREADS, blocks_a = (A.n_a + UPD_THREADS - 1) / UPD_THREADS;
    const bool actor = io.grad_actor != nullptr, polyak = io.update_targets != 0;
    A.part_c = blocks_c < GRADNORM_WORKGROUPS ? blocks_c : (int)GRADNORM_WORKGROUPS;
    A.part_a = !actor ? 0 : blocks_a < GRADNORM_WORKGROUPS ? blocks_a : (int)GRADNORM_WORKGROUPS;
    A.blocks_c = blocks_c;
    A.polyak = polyak ? 1 : 0;
    A.lrc = c.lr_critic; A.lra = c.lr_actor; A.eps = c.eps; A.max_norm = c.max_grad_norm; A.tau = c.tau;
    A.b1 = (float)c.beta1; A.omb1 = (float)(1.0 - c.beta1); A.b2 = (float)c.beta2; A.omb2 = (float)(1.0 - c.beta2);
    rsx_launch(dpg_grad_norm_kernel, dim3((unsigned)(A.part_c + A.part_a)), dim3(UPD_THREADS), 0, s, A);
    rsx_launch(dpg_adam_update_kernel, dim3((unsigned)(blocks_c + (actor || polyak ? blocks_a : 0))), dim3(UPD_THREADS), 0, s, A);
}

long long dpg_update_workspace_bytes(const long long n_params_actor, const long long n_params_critic, const int n_critics, const long long n_rows,
                                     const int max_workgroups, long long* rows_offset) {
    const UpdateWs w = update_ws(n_params_actor, n_params_critic, n_critics, n_rows, max_workgroups);
    if (rows_offset != nullptr) *rows_offset = (long long)w.rows;
    return (long long)w.total;
}

void launch_dpg_update(const PolicySpec& actor, const long long n_params_actor, float* actor_params, float* target_actor_params,
                       const PolicySpec& critic, const long long n_params_critic, float* critic_params, float* target_critic_params,
                       const int obs_dim, const int act_dim, const rsx_dpg_in& in, const rsx_dpg_cfg& cfg, const rsx_dpg_update_cfg& u,
                       const rsx_dpg_adam_cfg& adam, const rsx_dpg_adam_state& st, float* stats, void* workspace, hipStream_t s) {
    const long long m = in.n_rows;
    const UpdateWs w = update_ws(n_params_actor, n_params_critic, cfg.n_critics, m, cfg.max_workgroups);
    char* const base = static_cast<char*>(workspace);
    int32_t* const rows = reinterpret_cast<int32_t*>(base + w.rows);
    float* const ga = reinterpret_cast<float*>(base + w.ga);
    // keyed by the DEVICE's count of finished gradient steps: a replayed graph draws new rows and new noise on every replay
    const long long* const steps = reinterpret_cast<const long long*>(st.counters) + RSX_DPG_STEPS;
    rsx_dpg_in mb = in;
    mb.rows = rows;
    rsx_dpg_cfg gcfg = cfg;
    gcfg.noise_step_dev = reinterpret_cast<const int64_t*>(steps);
    rsx_dpg_out out{};
    out.grad_critics = reinterpret_cast<float*>(base + w.gc);
    out.workspace = base + w.grad;
    rsx_dpg_adam_io io{};
    io.actor_params = actor_params; io.target_actor_params = target_actor_params;
    io.critic_params = critic_params; io.target_critic_params = target_critic_params;
    io.grad_critic = out.grad_critics;
    io.workspace = base + w.adam;
    for (int j = 0; j < u.grad_steps; ++j) {
        float* const row = stats + (size_t)j * RSX_DPG_UPDATE_STATS;
        const bool actor_step = (j + 1) % u.policy_delay == 0;
        launch_replay_sample_rows(rows, m, in.n_batch_rows, u.fill, reinterpret_cast<const long long*>(u.fill_dev), u.seed, 0, steps, s);
        out.grad_actor = actor_step ? ga : nullptr;
        out.stats = row;
        launch_dpg_gradient(actor, n_params_actor, actor_params, target_actor_params, critic, n_params_critic, critic_params,
                            target_critic_params, obs_dim, act_dim, mb, gcfg, out, s);
        io.grad_actor = out.grad_actor;
        io.update_targets = actor_step ? 1 : 0;
        io.stats = row + 9;
        launch_dpg_adam_step(adam, st, io, s);
    }
}

}  // namespace rsx
