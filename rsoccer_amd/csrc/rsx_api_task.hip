// rsx_api_task.hip — the fused tasks of the C-ABI (include/rsx.h: rsx_task_*, rsx_read_metrics): attach, reseed, capture, tick,
// layout, view, reset, step, rollout, lookahead, sampled planning, metrics, checkpoint and transfer.  Host code only.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "rsx_handle.hpp"
#include "rsx_math.hpp"
#include "rsx_plan_common.hpp"

using namespace rsx;

// largest batch whose single-step launches carry placement-helper workgroups (rsx_placement.hpp: placement_helper): where a
// launch is as long as its slowest wave and half of the SIMDs are idle anyway
#ifndef RSX_PCACHE_MAX_ENVS
#define RSX_PCACHE_MAX_ENVS 16384
#endif

namespace {

// workgroups of the handle's lane-group launches, and the placement helpers behind them in a single-step launch of a handle
// with a placement cache (rsx_task_attach: 8 lanes per env, exact robot count): one per 64 envs; none with per-env physics
int grid_for(const rsx_sim* h) { return lane_grid(h->L, h->P.num_envs); }
int helpers_for(const rsx_sim* h, int mode) { return mode == MODE_STEP && h->d_pcache && !h->d_phys ? (h->P.num_envs + 63) / 64 : 0; }

// The layout of one launch of the handle's task kernels (the plan of rsx_task_attach); what is not a step runs on the lane-group kernels.
// step_grid and the dispatch read it and nothing else: the grid a launch gets is the grid the tick slots are kept in sync by (step_tick)
Layout stepping_layout(const rsx_sim* h, int mode) { return mode == MODE_STEP ? h->plan.step : mode == MODE_ROLLOUT ? h->plan.rollout : Layout::Lanes; }
int step_grid(const rsx_sim* h, int mode) {
    switch (stepping_layout(h, mode)) {
        case Layout::Epl: return epl_grid(h->P.num_envs);
        case Layout::Quad: return ssl_quad_grid(h->P.num_envs);
        default: return grid_for(h) + helpers_for(h, mode);   // (LanesBig: 32 lanes per env, no helpers)
    }
}
void launch_task_of(const rsx_sim* h, const float* actions, int n_steps, int mode, hipStream_t s) {
    const Buffers b = buffers_of(h, mode == MODE_STEP ? actions : nullptr);   // only a single step reads fed actions
    const bool rollout = mode == MODE_ROLLOUT;
    switch (stepping_layout(h, mode)) {
        case Layout::Epl:
            if (h->P.task == RSX_TASK_VSS_V0) launch_vss_epl(rollout, h->P, b, n_steps, s); else launch_ssl_epl(h->P.task, rollout, h->P, b, n_steps, s);
            break;
        case Layout::Quad: launch_ssl_quad(h->P, b, n_steps, s); break;
        case Layout::LanesBig: launch_scrimmage_big(rollout, h->P, b, n_steps, s); break;
        case Layout::Lanes:
            if (h->d_phys) launch_task_phys(h->P, b, h->L, h->NR, h->d_phys, n_steps, mode, s);
            else if (mode == MODE_STEP && h->plan.service_wave) launch_task_pair(h->P, b, n_steps, s);   // (same grid, two waves per workgroup)
            else launch_task(h->P, b, h->L, h->NR, helpers_for(h, mode), n_steps, mode, s);
            break;
    }
}
bool rollout_as_steps(const rsx_sim* h) { return h->plan.rollout_as_steps || (h->tick_dev && h->plan.step == Layout::Quad); }   // (device-keyed four-lane handle: one grid for all launches)

}  // namespace

void rsx::plan_stepping(rsx_sim* h) {
    const Params& P = h->P;
    h->plan = plan_layout(LayoutQuery{P.task, P.kind, h->L, h->NR, P.n_blue, P.num_envs, P.row_stride, P.state_dim, P.obs_dim, P.n_sub,
                                      h->d_phys != nullptr, std::getenv("RSX_LAYOUT"), std::getenv("RSX_SERVICE_WAVE")});
    h->tick_slots = step_grid(h, MODE_STEP);
}

extern "C" {

int rsx_task_attach(rsx_sim* h, int task, uint64_t seed, uint64_t env_id_base, int max_episode_steps) {
    RSX_ENTER(h);
    if (h->P.task != RSX_TASK_NONE) return fail(RSX_ERR_STATE, "a task is already attached");
    // global env ids are 32-bit words of the Philox counter: the whole range of this handle has to fit
    if (env_id_base > 0xFFFFFFFFull || env_id_base + (uint64_t)h->P.num_envs > 0x100000000ull)
        return fail(RSX_ERR_ARG, "env_id_base + num_envs exceeds 2^32 (global env ids are 32-bit)");
    Params P = h->P;
    if (derive_task(task, seed, env_id_base, max_episode_steps, h->M, P))
        return fail(RSX_ERR_ARG, "task does not match the simulator (VSS_V0: VSS, n_blue >= 1; STATIC_DEFENDERS: SSL 1vN; DRIBBLING: SSL 1v4; CONTESTED: SSL 1v1; PASS_ENDURANCE: SSL 2v0; SCRIMMAGE: SSL)");
    if (P.obs_dim > 64) return fail(RSX_ERR_ARG, "observation wider than 64 floats is not supported");
    if (task >= RSX_TASK_SSL_DRIBBLING && task <= RSX_TASK_SSL_PASS_ENDURANCE && h->L != 8)
        return fail(RSX_ERR_ARG, "this task runs with 8 lanes per env only (unset RSX_LANES_PER_ENV)");
    const size_t B = (size_t)P.num_envs, S = (size_t)P.row_stride;
    const size_t n_aux = align_up((size_t)aux_rows(P.n_robots) * S * sizeof(float));
    if (n_aux >= ((size_t)1 << 32) || B * (size_t)P.obs_dim * sizeof(float) >= ((size_t)1 << 32))
        return fail(RSX_ERR_ARG, "num_envs too large for a fused task: the per-env scalar arena or the observation array would reach 4 GB (see rsx.h, limits)");
    const size_t n_obs = align_up(B * P.obs_dim * sizeof(float));
    const size_t n_flags = align_up(3 * B);   // terminated | truncated | the env mask of rsx_task_reset_to (read by the MODE_REFRESH launch only)
    const size_t n_act = align_up(B * h->M.act_dim * sizeof(float));
    // metrics[8] | error word | (256 bytes in) one step-counter slot per workgroup of the largest stepping launch any layout
    // of this batch could use (rsx_hot_args.hpp: step_tick; only the first tick_slots are kept in sync)
    const size_t n_met = align_up((size_t)TICK_SLOT_WORD0 * 4 + ((size_t)grid_for(h) + (B + 63) / 64) * sizeof(uint32_t));
    const size_t n_slots = align_up((size_t)MSLOTS * RSX_METRICS * sizeof(unsigned long long));
    // placement cache: static defenders 1v6 (short episodes: several resetting waves per launch) at latency-bound batches
    const bool pc = !std::getenv("RSX_NO_PCACHE") && h->L == 8 && P.num_envs <= RSX_PCACHE_MAX_ENVS && P.n_sub > 0 &&
                    task == RSX_TASK_SSL_STATIC_DEFENDERS && h->NR == 7;
    const size_t n_pc = pc ? align_up((size_t)2 * (3 * (P.n_robots + 1) + 1) * B * sizeof(float)) : 0;
    const size_t n_pcs = pc && std::getenv("RSX_PCACHE_STATS") ? align_up(2 * sizeof(unsigned long long)) : 0;
    const size_t total = n_aux + 2 * n_obs + n_flags + n_act + n_met + n_slots + n_pc + n_pcs;
    HIP_TRY(hipMalloc((void**)&h->arena_task, total));
    HIP_TRY(hipMemset(h->arena_task, 0, total));
    h->arena_task_bytes = total; h->pcache_bytes = n_pc;
    char* p = h->arena_task;
    h->d_aux = (float*)p; p += n_aux;
    h->d_obs = (float*)p; p += n_obs;
    h->d_final_obs = (float*)p; p += n_obs;
    h->d_flags = (uint8_t*)p; p += n_flags;
    h->d_actions = (float*)p; p += n_act;
    h->d_metrics = (unsigned long long*)p; p += n_met;
    h->d_mslots = (unsigned long long*)p; p += n_slots;
    if (n_pc) {
        h->d_pcache = (float*)p; p += n_pc;
        HIP_TRY(hipMemset(h->d_pcache, 0xFF, n_pc));   // tags 0xFFFFFFFF: no entry is valid yet
    }
    if (n_pcs) h->d_pcstats = (unsigned long long*)p;
    // episode ids start at 0xFFFFFFFF so that the first reset() opens episode 0
    HIP_TRY(hipMemset(h->d_aux + (size_t)ROW_EPISODE * S, 0xFF, B * sizeof(uint32_t)));
    h->P = P;
    plan_stepping(h);
    h->task_ready = false;
    h->tick_dev = false;
    h->tick_slots_alloc = std::max(h->tick_slots, grid_for(h) + (P.num_envs + 63) / 64);
    HIP_TRY(hipDeviceSynchronize());   // null-stream memsets done before any caller stream steps
    return RSX_OK;
}

int rsx_task_reseed(rsx_sim* h, uint64_t seed, void* stream) {
    RSX_ENTER_TASK(h);
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) return fail(RSX_ERR_STATE, "rsx_task_reseed changes host state (seed, step counter) and cannot be captured");
    // what rsx_task_attach leaves behind, with the new key: every per-env buffer and counter cleared, episode ids at 0xFFFFFFFF,
    // placement cache empty, step counter 0 (device-keyed handles: every slot), no episode open
    HIP_TRY(hipMemsetAsync(h->arena_task, 0, h->arena_task_bytes, s));
    if (h->d_pcache) HIP_TRY(hipMemsetAsync(h->d_pcache, 0xFF, h->pcache_bytes, s));
    HIP_TRY(hipMemsetAsync(h->d_aux + (size_t)ROW_EPISODE * h->P.row_stride, 0xFF, (size_t)h->P.num_envs * sizeof(uint32_t), s));
    h->P.key0 = (uint32_t)seed; h->P.key1 = (uint32_t)(seed >> 32);
    h->tick = 0; h->P.tick_base = 0;
    h->task_ready = false;
    return RSX_OK;
}

int rsx_task_enable_capture(rsx_sim* h, void* stream) {
    RSX_ENTER_TASK(h);
    // The one place where the thread's pending HIP error is dropped: the usual way to get here is a capture attempt that this library
    // refused (host-keyed handle) and that the caller's framework then aborted — which leaves `invalid argument` in the slot for the
    // NEXT capture to trip over (torch.cuda.graph does).  A set-up call, not a stepping path; rsx.h says so.
    (void)hipGetLastError();
    if (h->tick_dev) return RSX_OK;
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s))
        return fail(RSX_ERR_STATE, "rsx_task_enable_capture must be called BEFORE the capture begins (it writes the step counter once; a captured write would reset it on every replay)");
    launch_tick_fill(tick_slot0(h), 0, h->tick_slots_alloc, h->tick, 0, s);
    HIP_TRY(launch_status());
    h->tick_dev = true;
    h->host_state_cache = false; h->host_state_valid = false;   // a replayed graph changes the state without passing through this API
    return RSX_OK;
}

int rsx_task_tick(rsx_sim* h, uint32_t* out, void* stream) {
    RSX_ENTER(h);
    if (!out) return fail(RSX_ERR_ARG, "out is null");
    if (h->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached (rsx_task_attach)");
    if (!h->tick_dev) { *out = h->tick; return RSX_OK; }
    uint32_t w[2] = {0, 0};   // slot 0, error word
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(&w[0], tick_slot0(h), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&w[1], tick_words(h) + TICK_ERR_WORD, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = w[0];
    h->tick = w[0];
    if (w[1]) return fail(RSX_ERR_STATE, "step counter exhausted: a launch that would have wrapped it was refused on the device (a handle takes at most 2^32 - 1 fused steps)");
    return RSX_OK;
}

int rsx_task_placement_cache_stats(rsx_sim* h, int64_t out[2], void* stream) {
    RSX_ENTER_TASK(h);
    if (!out) return fail(RSX_ERR_ARG, "out is null");
    out[0] = out[1] = -1;   // -1: no cache on this handle, or the counters are off (RSX_PCACHE_STATS=1 before rsx_task_attach)
    if (!h->d_pcstats) return RSX_OK;
    HIP_TRY(hipMemcpyAsync(out, h->d_pcstats, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return RSX_OK;
}

int rsx_task_layout(rsx_sim* h, char* out, size_t n) {
    if (!h || !out || n == 0) return fail(RSX_ERR_ARG, "null argument");
    if (h->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached (rsx_task_attach)");
    const Layout lay = h->plan.step;
    const char* name = lay == Layout::Epl ? "one-lane-per-env" : lay == Layout::Quad ? "four-lanes-per-env" : lay == Layout::LanesBig ? "32-lanes-per-env-large-batch"
                     : h->L == 8 ? "8-lanes-per-env" : h->L == 16 ? "16-lanes-per-env" : h->L == 32 ? "32-lanes-per-env" : "64-lanes-per-env";
    std::snprintf(out, n, "%s", name);
    return RSX_OK;
}

int rsx_task_service_wave(rsx_sim* h, int* out) {
    if (!h || !out) return fail(RSX_ERR_ARG, "null argument");
    if (h->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached (rsx_task_attach)");
    *out = h->plan.step == Layout::Lanes && h->plan.service_wave && !h->d_phys ? 1 : 0;   // (what launch_task_of dispatches on)
    return RSX_OK;
}

int rsx_task_view_get(rsx_sim* h, rsx_task_view* out) {
    if (!h || !out) return fail(RSX_ERR_ARG, "null argument");
    if (h->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached (rsx_task_attach)");
    const size_t B = (size_t)h->P.num_envs;
    out->task = h->P.task; out->obs_dim = h->P.obs_dim; out->act_dim = h->M.act_dim;
    out->info_dim = h->M.info_dim; out->max_episode_steps = h->P.max_steps;
    const size_t S = (size_t)h->P.row_stride;
    out->obs = h->d_obs; out->reward = h->d_aux + (size_t)ROW_REWARD * S;
    out->terminated = h->d_flags; out->truncated = h->d_flags + B;
    out->info = h->d_aux + (size_t)ROW_INFO * S; out->final_obs = h->d_final_obs;
    out->steps = (int32_t*)(h->d_aux + (size_t)ROW_STEPS * S); out->actions = h->d_actions;
    out->metrics = (int64_t*)h->d_metrics; out->row_stride = h->P.row_stride;
    return RSX_OK;
}

int rsx_task_reset(rsx_sim* h, void* stream) {
    RSX_ENTER_TASK(h);
    launch_task_of(h, nullptr, 1, MODE_RESET, (hipStream_t)stream);
    HIP_TRY(launch_status());
    h->task_ready = true;
    return RSX_OK;
}

int rsx_task_reset_to(rsx_sim* h, const double* ball, const double* blue, const double* yellow,
                      const uint8_t* env_mask, void* stream) {
    RSX_ENTER_TASK(h);
    if (int rc = rsx_reset(h, ball, blue, yellow, env_mask, stream)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t B = (size_t)h->P.num_envs;
    // the kernel takes the env mask through the third row of the flags array: `terminated` / `truncated` of the envs the mask leaves
    // alone stay what their last step made them (until round 6 the mask travelled through the `truncated` row, which was cleared
    // afterwards — for EVERY env: found by tests/test_gpu_api_fuzz.py)
    if (env_mask) HIP_TRY(hipMemcpyAsync(h->d_flags + 2 * B, env_mask, B, hipMemcpyHostToDevice, s));
    else HIP_TRY(hipMemsetAsync(h->d_flags + 2 * B, 1, B, s));
    launch_task_of(h, nullptr, 1, MODE_REFRESH, s);
    HIP_TRY(launch_status());
    HIP_TRY(hipStreamSynchronize(s));   // the host mask / placement arrays may be reused by the caller
    h->task_ready = true;
    return RSX_OK;
}

// The handle's step counter keys the per-step random draws and is one 32-bit word of the Philox counter: a handle that
// has taken 2^32 - 1 fused steps refuses further ones instead of silently replaying its random streams.
// Host-keyed handles (the default) check that here and bake the count into the launch — which is why they refuse to be
// captured: a replayed graph would step with one tick for ever.  Device-keyed handles (rsx_task_enable_capture) pass
// RSX_TICK_DEV instead: the kernels read, check and advance the counter themselves (rsx_hot_args.hpp: step_tick).
static int step_prologue(rsx_sim* h, hipStream_t s, uint64_t n, int* flags) {
    *flags = 0;
    if (h->tick_dev) { *flags = RSX_TICK_DEV; return RSX_OK; }
    if (stream_is_capturing(s))
        return fail(RSX_ERR_STATE, "this stream is being captured, and the handle's step counter (the key of its per-step random draws) is still a host-side "
                                   "launch argument: a replayed graph would repeat one random stream. Call rsx_task_enable_capture(h, stream) once, before the capture begins");
    if ((uint64_t)h->tick + n > 0xFFFFFFFFull)
        return fail(RSX_ERR_STATE, "step counter exhausted: a handle takes at most 2^32 - 1 fused steps (it keys the per-step random draws); attach a fresh handle with another seed");
    return RSX_OK;
}
// device-keyed handles: slots the launch did not cover (a grid without the placement helpers) follow slot 0
static void tick_resync(const rsx_sim* h, int mode, hipStream_t s) {
    if (h->tick_dev) launch_tick_fill(tick_slot0(h), step_grid(h, mode), h->tick_slots, 0u, 1, s);
}

static int single_steps(rsx_sim* h, const float* actions_dev, int n, hipStream_t s, const char* where) {   // n single-step launches, tick by tick
    int fl = 0;
    if (int rc = step_prologue(h, s, (uint64_t)n, &fl)) return rc;
    for (int i = 0; i < n; ++i) { h->P.tick_base = h->tick++; launch_task_of(h, actions_dev, 1 | fl, MODE_STEP, s); }
    HIP_TRY(launch_status());
    return debug_finite(h, s, where);
}

int rsx_task_step(rsx_sim* h, const float* actions_dev, void* stream) {
    RSX_ENTER_TASK(h);
    RSX_NEED_RESET(h);
    return single_steps(h, actions_dev, 1, (hipStream_t)stream, "rsx_task_step");
}

int rsx_task_step_n(rsx_sim* h, int n, void* stream) {
    RSX_ENTER_TASK(h);
    RSX_NEED_RESET(h);
    if (n < 1) return fail(RSX_ERR_ARG, "n must be >= 1");
    return single_steps(h, nullptr, n, (hipStream_t)stream, "rsx_task_step_n");
}

int rsx_task_rollout(rsx_sim* h, int n, void* stream) {
    RSX_ENTER_TASK(h);
    RSX_NEED_RESET(h);
    if (n < 0 || n > RSX_N_STEPS_MASK) return fail(RSX_ERR_ARG, "n must be in 0 .. 2^30 - 1");  // 0 = load + store only (profiling)
    if (n >= 1 && rollout_as_steps(h)) return single_steps(h, nullptr, n, (hipStream_t)stream, "rsx_task_rollout");   // 11v11 at large batches (rsx_layout.hpp)
    int fl = 0;
    if (int rc = step_prologue(h, (hipStream_t)stream, (uint64_t)n, &fl)) return rc;
    h->P.tick_base = h->tick; h->tick += (uint32_t)n;
    launch_task_of(h, nullptr, n | fl, MODE_ROLLOUT, (hipStream_t)stream);
    tick_resync(h, MODE_ROLLOUT, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return debug_finite(h, (hipStream_t)stream, "rsx_task_rollout");
}

int rsx_task_lookahead(rsx_sim* h, const float* actions_dev, int n_candidates, int horizon, float gamma, float* returns_dev,
                       int32_t* steps_dev, uint8_t* flags_dev, float* last_obs_dev, void* stream) {
    RSX_ENTER(h);   // (not RSX_ENTER_TASK: nothing the handle owns changes, the host's copy of the state included)
    if (h->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached (rsx_task_attach)");
    RSX_NEED_RESET(h);
    if (n_candidates < 1 || horizon < 1) return fail(RSX_ERR_ARG, "n_candidates and horizon must be >= 1");
    if (!actions_dev || !returns_dev || !steps_dev || !flags_dev) return fail(RSX_ERR_ARG, "actions_dev, returns_dev, steps_dev and flags_dev must not be null");
    if (!std::isfinite(gamma)) return fail(RSX_ERR_ARG, "gamma must be finite");
    if (h->L > 32) return fail(RSX_ERR_ARG, "rsx_task_lookahead has no 64-lanes-per-env kernels (unset RSX_LANES_PER_ENV)");
    if (lookahead_grid(h->L, h->P.num_envs, n_candidates) > 0x7FFFFFFFll)
        return fail(RSX_ERR_ARG, "num_envs x n_candidates exceeds the launch limit (2^31 - 1 workgroups): split the candidates over several calls");
    int fl = 0;
    if (int rc = step_prologue(h, (hipStream_t)stream, (uint64_t)horizon, &fl)) return rc;   // capture of a host-keyed handle, counter limit
    Params P = h->P;
    P.tick_base = h->tick;   // the tick the next step would take; not advanced
    launch_task_lookahead(P, h->L, h->NR, h->d_state, h->d_aux, h->tick_dev ? tick_slot0(h) : nullptr, h->d_phys,
                          actions_dev, n_candidates, horizon, gamma, returns_dev, steps_dev, flags_dev, last_obs_dev, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

// ---- the lookahead with an MLP policy as its action source (rsx.h: rsx_policy_mlp) ----
// what both calls check of a policy; on success S is the spec as the kernels take it and *n_params the floats of one policy
static int policy_prologue(const rsx_sim* h, const rsx_policy_mlp* p, PolicySpec* S, int64_t* n_params) {
    if (h->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached (rsx_task_attach)");
    if (!p) return fail(RSX_ERR_ARG, "the policy (rsx_policy_mlp) must not be null");
    if (h->P.task == RSX_TASK_SSL_SCRIMMAGE || h->P.task == RSX_TASK_SSL_SCRIMMAGE_CROWDED)
        return fail(RSX_ERR_ARG, "the scrimmage task commands every robot (act_dim = 4 N): one policy per env does not drive it");
    if (p->n_hidden_layers != 1 && p->n_hidden_layers != 2) return fail(RSX_ERR_ARG, "n_hidden_layers must be 1 or 2");
    if (p->hidden != 32 && p->hidden != 64) return fail(RSX_ERR_ARG, "hidden must be 32 or 64");
    if (p->hidden_act != RSX_ACT_RELU && p->hidden_act != RSX_ACT_TANH) return fail(RSX_ERR_ARG, "hidden_act must be RSX_ACT_RELU or RSX_ACT_TANH");
    if (p->out_act != RSX_ACT_CLIP && p->out_act != RSX_ACT_TANH) return fail(RSX_ERR_ARG, "out_act must be RSX_ACT_CLIP or RSX_ACT_TANH");
    *S = PolicySpec{p->n_hidden_layers, p->hidden, p->hidden_act, p->out_act};
    const int64_t H = p->hidden;
    *n_params = H * h->P.obs_dim + H + (p->n_hidden_layers == 2 ? H * H + H : 0) + (int64_t)h->M.act_dim * H + h->M.act_dim;
    return RSX_OK;
}

int rsx_policy_num_params(const rsx_sim* h, const rsx_policy_mlp* p, int64_t* out) {
    if (!h) return fail(RSX_ERR_ARG, "null handle");
    if (!out) return fail(RSX_ERR_ARG, "out must not be null");
    PolicySpec S;
    return policy_prologue(h, p, &S, out);
}

int rsx_task_lookahead_policy(rsx_sim* h, const rsx_policy_mlp* p, const float* params_dev, int n_policies, int horizon, float gamma,
                              float* returns_dev, int32_t* steps_dev, uint8_t* flags_dev, float* last_obs_dev, float* actions_out_dev,
                              float* obs_out_dev, void* stream) {
    RSX_ENTER(h);   // (as rsx_task_lookahead: nothing the handle owns changes)
    PolicySpec S; int64_t n_params = 0;
    if (int rc = policy_prologue(h, p, &S, &n_params)) return rc;
    RSX_NEED_RESET(h);
    if (n_policies < 1 || horizon < 1) return fail(RSX_ERR_ARG, "n_policies and horizon must be >= 1");
    if (!params_dev || !returns_dev || !steps_dev || !flags_dev) return fail(RSX_ERR_ARG, "params_dev, returns_dev, steps_dev and flags_dev must not be null");
    if (!std::isfinite(gamma)) return fail(RSX_ERR_ARG, "gamma must be finite");
    if (h->L > 32) return fail(RSX_ERR_ARG, "rsx_task_lookahead_policy has no 64-lanes-per-env kernels (unset RSX_LANES_PER_ENV)");
    if (lookahead_grid(h->L, h->P.num_envs, n_policies) > 0x7FFFFFFFll)
        return fail(RSX_ERR_ARG, "num_envs x n_policies exceeds the launch limit (2^31 - 1 workgroups): split the policies over several calls");
    if (policy_lds_bytes(h->L, h->P.obs_dim, h->M.act_dim, S) > 65536ll)
        return fail(RSX_ERR_ARG, "the policy's weights do not fit a workgroup's 64 KB of LDS at this observation width: use fewer or smaller hidden layers");
    int fl = 0;
    if (int rc = step_prologue(h, (hipStream_t)stream, (uint64_t)horizon, &fl)) return rc;   // capture of a host-keyed handle, counter limit
    Params P = h->P;
    P.tick_base = h->tick;   // the tick the next step would take; not advanced
    launch_task_lookahead_policy(P, h->L, h->NR, h->d_state, h->d_aux, h->d_obs, h->tick_dev ? tick_slot0(h) : nullptr, h->d_phys, S, params_dev,
                                 (int)n_params, h->M.act_dim, n_policies, horizon, gamma, returns_dev, steps_dev, flags_dev, last_obs_dev,
                                 actions_out_dev, obs_out_dev, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

// ---- the same against an opponent: K actors x M opponents per env of VSS-v0 in one launch (rsx.h: rsx_task_lookahead_match) ----
int rsx_task_lookahead_match(rsx_sim* h, const rsx_policy_mlp* actor, const float* actor_params_dev, int n_actors, int actor_seats,
                             const rsx_policy_mlp* opponent, const float* opponent_params_dev, int n_opponents, int opponent_seats,
                             int horizon, float gamma, const rsx_match_out* out, void* stream) {
    RSX_ENTER(h);   // (as rsx_task_lookahead: nothing the handle owns changes)
    PolicySpec S, S2; int64_t n_params = 0, n_opp_params = 0;
    if (int rc = policy_prologue(h, actor, &S, &n_params)) return rc;
    if (h->P.task != RSX_TASK_VSS_V0)
        return fail(RSX_ERR_ARG, "rsx_task_lookahead_match serves VSS-v0 only: a seat drives a robot of that task");
    if (h->P.n_blue != h->P.n_yellow)
        return fail(RSX_ERR_ARG, "rsx_task_lookahead_match needs equal teams: the mirrored observation has the agent's layout");
    if (actor_seats != 1 && actor_seats != h->P.n_blue) return fail(RSX_ERR_ARG, "actor_seats must be 1 or n_blue");
    if (opponent_seats != 1 && opponent_seats != h->P.n_yellow)
        return fail(RSX_ERR_ARG, "opponent_seats must be 1 or n_yellow (without an opponent the call is rsx_task_lookahead_policy)");
    if (!opponent) return fail(RSX_ERR_ARG, "the opponent (rsx_policy_mlp) must not be null");
    if (int rc = policy_prologue(h, opponent, &S2, &n_opp_params)) return rc;
    RSX_NEED_RESET(h);
    if (n_actors < 1 || n_opponents < 1 || horizon < 1) return fail(RSX_ERR_ARG, "n_actors, n_opponents and horizon must be >= 1");
    if (!actor_params_dev || !opponent_params_dev) return fail(RSX_ERR_ARG, "actor_params_dev and opponent_params_dev must not be null");
    if (!out || !out->returns || !out->steps || !out->flags)
        return fail(RSX_ERR_ARG, "out and its returns, steps and flags arrays must not be null");
    if (!std::isfinite(gamma)) return fail(RSX_ERR_ARG, "gamma must be finite");
    if (h->L > 32) return fail(RSX_ERR_ARG, "rsx_task_lookahead_match has no 64-lanes-per-env kernels (unset RSX_LANES_PER_ENV)");
    const long long pairs = (long long)n_actors * (long long)n_opponents;
    if (pairs > 0x7FFFFFFFll || lookahead_grid(h->L, h->P.num_envs, (int)pairs) > 0x7FFFFFFFll)
        return fail(RSX_ERR_ARG, "num_envs x n_actors x n_opponents exceeds the launch limit (2^31 - 1 workgroups): split the policies over several calls");
    if (match_lds_bytes(h->L, h->P.obs_dim, h->M.act_dim, h->P.n_blue, S, S2) > 163840ll)
        return fail(RSX_ERR_ARG, "the policies' weights do not fit a CU's 160 KB of LDS at this observation width: use fewer or smaller hidden layers");
    int fl = 0;
    if (int rc = step_prologue(h, (hipStream_t)stream, (uint64_t)horizon, &fl)) return rc;   // capture of a host-keyed handle, counter limit
    Params P = h->P;
    P.tick_base = h->tick;   // the tick the next step would take; not advanced
    launch_task_lookahead_match(P, h->L, h->NR, h->d_state, h->d_aux, h->d_obs, h->tick_dev ? tick_slot0(h) : nullptr, h->d_phys, S,
                                actor_params_dev, (int)n_params, n_actors, actor_seats, S2, opponent_params_dev, (int)n_opp_params, n_opponents,
                                opponent_seats, h->M.act_dim, horizon, gamma, *out, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

// ---- on-policy collection: n steps under the policy in one launch, the [T][B] batch written out (rsx.h: rsx_task_collect_policy) ----
int rsx_task_collect_policy(rsx_sim* h, const rsx_policy_mlp* p, const float* params_dev, const float* sigma_dev, uint64_t noise_seed,
                            int n_steps, const rsx_collect_out* out, void* stream) {
    RSX_ENTER(h);
    PolicySpec S; int64_t n_params = 0;
    if (int rc = policy_prologue(h, p, &S, &n_params)) return rc;
    RSX_NEED_RESET(h);
    if (n_steps < 1 || n_steps > RSX_N_STEPS_MASK) return fail(RSX_ERR_ARG, "n_steps must be in 1 .. 2^30 - 1");
    if (!params_dev) return fail(RSX_ERR_ARG, "params_dev must not be null");
    if (!out || !out->obs || !out->actions || !out->rewards || !out->flags)
        return fail(RSX_ERR_ARG, "out and its obs, actions, rewards and flags arrays must not be null");
    if (h->L > 32) return fail(RSX_ERR_ARG, "rsx_task_collect_policy has no 64-lanes-per-env kernels (unset RSX_LANES_PER_ENV)");
    if (policy_lds_bytes(h->L, h->P.obs_dim, h->M.act_dim, S) > 65536ll)
        return fail(RSX_ERR_ARG, "the policy's weights do not fit a workgroup's 64 KB of LDS at this observation width: use fewer or smaller hidden layers");
    hipStream_t s = (hipStream_t)stream;
    int fl = 0;
    if (int rc = step_prologue(h, s, (uint64_t)n_steps, &fl)) return rc;   // capture of a host-keyed handle, counter limit
    h->host_state_valid = false;   // (from here on the call changes the state, as every stepping call does)
    // device-keyed handles: the launch reads, checks and advances the slots of its lane_grid workgroups.  Where the handle's steps run
    // on a smaller grid (one lane per env), the slots behind that grid are not kept in sync by them: they follow slot 0 first
    const int grid = grid_for(h);
    if (h->tick_dev) launch_tick_fill(tick_slot0(h), h->tick_slots, grid, 0u, 1, s);
    h->P.tick_base = h->tick; h->tick += (uint32_t)n_steps;
    launch_task_collect_policy(h->P, buffers_of(h, nullptr), h->L, h->NR, h->d_phys, S, params_dev, (int)n_params, h->M.act_dim, sigma_dev,
                               noise_seed, n_steps | fl, out->obs, out->actions, out->rewards, out->flags, out->final_obs, out->mean,
                               out->sample, s);
    // ... and the slots the launch did not cover (placement helpers behind the tiles) follow slot 0 afterwards, as after a rollout
    if (h->tick_dev) launch_tick_fill(tick_slot0(h), grid, h->tick_slots, 0u, 1, s);
    HIP_TRY(launch_status());
    return debug_finite(h, s, "rsx_task_collect_policy");
}

// ---- the same under a state-dependent tanh-squashed Gaussian head: the output layer gives mean and log-std (rsx.h: rsx_task_collect_gaussian) ----
int rsx_task_collect_gaussian(rsx_sim* h, const rsx_policy_mlp* p, const float* params_dev, const rsx_collect_gaussian_cfg* cfg, int n_steps,
                              const rsx_collect_out* out, float* log_std_out, void* stream) {
    RSX_ENTER(h);
    PolicySpec S; int64_t n_params = 0;
    if (!p) return fail(RSX_ERR_ARG, "the policy (rsx_policy_mlp) must not be null");
    rsx_policy_mlp shape = *p;
    shape.out_act = RSX_ACT_TANH;   // (what the head applies; the shape's own checks are rsx_task_collect_policy's)
    if (int rc = policy_prologue(h, &shape, &S, &n_params)) return rc;
    if (p->out_act != RSX_ACT_NONE)
        return fail(RSX_ERR_ARG, "rsx_task_collect_gaussian: out_act must be RSX_ACT_NONE (the head clamps the log-std and squashes the sample itself)");
    S.out_act = RSX_ACT_NONE;
    n_params += (int64_t)h->M.act_dim * p->hidden + h->M.act_dim;   // the output layer is 2 * act_dim units wide
    RSX_NEED_RESET(h);
    if (!cfg) return fail(RSX_ERR_ARG, "cfg (rsx_collect_gaussian_cfg) must not be null");
    if (!std::isfinite(cfg->log_std_min) || !std::isfinite(cfg->log_std_max) || !(cfg->log_std_min < cfg->log_std_max))
        return fail(RSX_ERR_ARG, "log_std_min and log_std_max must be finite with log_std_min < log_std_max");
    if (cfg->reserved != 0) return fail(RSX_ERR_ARG, "rsx_collect_gaussian_cfg.reserved must be 0");
    if (n_steps < 1 || n_steps > RSX_N_STEPS_MASK) return fail(RSX_ERR_ARG, "n_steps must be in 1 .. 2^30 - 1");
    if (!params_dev) return fail(RSX_ERR_ARG, "params_dev must not be null");
    if (!out || !out->obs || !out->actions || !out->rewards || !out->flags)
        return fail(RSX_ERR_ARG, "out and its obs, actions, rewards and flags arrays must not be null");
    if (h->L > 32) return fail(RSX_ERR_ARG, "rsx_task_collect_gaussian has no 64-lanes-per-env kernels (unset RSX_LANES_PER_ENV)");
    if (gaussian_lds_bytes(h->L, h->P.obs_dim, h->M.act_dim, S) > 65536ll)
        return fail(RSX_ERR_ARG, "the policy's weights do not fit a workgroup's 64 KB of LDS at this observation width: use fewer or smaller hidden layers");
    hipStream_t s = (hipStream_t)stream;
    int fl = 0;
    if (int rc = step_prologue(h, s, (uint64_t)n_steps, &fl)) return rc;   // capture of a host-keyed handle, counter limit
    h->host_state_valid = false;
    const int grid = grid_for(h);   // (the tick slots: as rsx_task_collect_policy, the launch has its grid)
    if (h->tick_dev) launch_tick_fill(tick_slot0(h), h->tick_slots, grid, 0u, 1, s);
    h->P.tick_base = h->tick; h->tick += (uint32_t)n_steps;
    launch_task_collect_gaussian(h->P, buffers_of(h, nullptr), h->L, h->NR, h->d_phys, S, params_dev, (int)n_params, h->M.act_dim, *cfg,
                                 n_steps | fl, *out, log_std_out, s);
    if (h->tick_dev) launch_tick_fill(tick_slot0(h), grid, h->tick_slots, 0u, 1, s);
    HIP_TRY(launch_status());
    return debug_finite(h, s, "rsx_task_collect_gaussian");
}

// ---- the same with yellow robot 0 of VSS-v0 driven by a second policy from the mirrored observation (rsx.h: rsx_task_collect_selfplay) ----
int rsx_task_collect_selfplay(rsx_sim* h, const rsx_policy_mlp* actor, const float* actor_params_dev, const float* sigma_dev,
                              const rsx_policy_mlp* opponent, const float* opponent_params_dev, const float* opponent_sigma_dev,
                              uint64_t noise_seed, int n_steps, const rsx_collect_out* out, const rsx_selfplay_out* sp, void* stream) {
    RSX_ENTER(h);
    PolicySpec S, S2; int64_t n_params = 0, n_opp_params = 0;
    if (int rc = policy_prologue(h, actor, &S, &n_params)) return rc;
    if (h->P.task != RSX_TASK_VSS_V0)
        return fail(RSX_ERR_ARG, "rsx_task_collect_selfplay serves VSS-v0 only: the opponent drives yellow robot 0 of that task");
    if (h->P.n_blue != h->P.n_yellow)
        return fail(RSX_ERR_ARG, "rsx_task_collect_selfplay needs equal teams: the mirrored observation has the agent's layout");
    if (!opponent) return fail(RSX_ERR_ARG, "the opponent (rsx_policy_mlp) must not be null");
    if (int rc = policy_prologue(h, opponent, &S2, &n_opp_params)) return rc;
    RSX_NEED_RESET(h);
    if (n_steps < 1 || n_steps > RSX_N_STEPS_MASK) return fail(RSX_ERR_ARG, "n_steps must be in 1 .. 2^30 - 1");
    if (!actor_params_dev || !opponent_params_dev) return fail(RSX_ERR_ARG, "actor_params_dev and opponent_params_dev must not be null");
    if (!out || !out->obs || !out->actions || !out->rewards || !out->flags)
        return fail(RSX_ERR_ARG, "out and its obs, actions, rewards and flags arrays must not be null");
    if (h->L > 32) return fail(RSX_ERR_ARG, "rsx_task_collect_selfplay has no 64-lanes-per-env kernels (unset RSX_LANES_PER_ENV)");
    if (selfplay_lds_bytes(h->L, h->P.obs_dim, h->M.act_dim, S, S2) > 163840ll)
        return fail(RSX_ERR_ARG, "the two policies' weights do not fit a CU's 160 KB of LDS at this observation width: use fewer or smaller hidden layers");
    hipStream_t s = (hipStream_t)stream;
    int fl = 0;
    if (int rc = step_prologue(h, s, (uint64_t)n_steps, &fl)) return rc;   // capture of a host-keyed handle, counter limit
    h->host_state_valid = false;
    const int grid = grid_for(h);   // (the tick slots: as rsx_task_collect_policy, the launch has its grid)
    if (h->tick_dev) launch_tick_fill(tick_slot0(h), h->tick_slots, grid, 0u, 1, s);
    h->P.tick_base = h->tick; h->tick += (uint32_t)n_steps;
    const rsx_selfplay_out none{nullptr, nullptr, nullptr, nullptr};
    launch_task_collect_selfplay(h->P, buffers_of(h, nullptr), h->L, h->NR, h->d_phys, S, actor_params_dev, (int)n_params, S2,
                                 opponent_params_dev, (int)n_opp_params, h->M.act_dim, sigma_dev, opponent_sigma_dev, noise_seed, n_steps | fl,
                                 *out, sp ? *sp : none, s);
    if (h->tick_dev) launch_tick_fill(tick_slot0(h), grid, h->tick_slots, 0u, 1, s);
    HIP_TRY(launch_status());
    return debug_finite(h, s, "rsx_task_collect_selfplay");
}

// ---- the same with every robot of a side seated under that side's policy (rsx.h: rsx_task_collect_team) ----
int rsx_task_collect_team(rsx_sim* h, const rsx_policy_mlp* actor, const float* actor_params_dev, const float* sigma_dev, int actor_seats,
                          const rsx_policy_mlp* opponent, const float* opponent_params_dev, const float* opponent_sigma_dev,
                          int opponent_seats, uint64_t noise_seed, int n_steps, const rsx_team_out* out, void* stream) {
    RSX_ENTER(h);
    PolicySpec S, S2; int64_t n_params = 0, n_opp_params = 0;
    if (int rc = policy_prologue(h, actor, &S, &n_params)) return rc;
    if (h->P.task != RSX_TASK_VSS_V0)
        return fail(RSX_ERR_ARG, "rsx_task_collect_team serves VSS-v0 only: a seat drives a robot of that task");
    if (h->P.n_blue != h->P.n_yellow)
        return fail(RSX_ERR_ARG, "rsx_task_collect_team needs equal teams: the mirrored observation has the agent's layout");
    if (actor_seats != 1 && actor_seats != h->P.n_blue) return fail(RSX_ERR_ARG, "actor_seats must be 1 or n_blue");
    if (opponent_seats != 0 && opponent_seats != 1 && opponent_seats != h->P.n_yellow)
        return fail(RSX_ERR_ARG, "opponent_seats must be 0, 1 or n_yellow");
    if ((opponent != nullptr) != (opponent_seats > 0))
        return fail(RSX_ERR_ARG, "the opponent (rsx_policy_mlp) must be null exactly when opponent_seats is 0");
    if (opponent)
        if (int rc = policy_prologue(h, opponent, &S2, &n_opp_params)) return rc;
    RSX_NEED_RESET(h);
    if (n_steps < 1 || n_steps > RSX_N_STEPS_MASK) return fail(RSX_ERR_ARG, "n_steps must be in 1 .. 2^30 - 1");
    if (!actor_params_dev || (opponent && !opponent_params_dev))
        return fail(RSX_ERR_ARG, "actor_params_dev and, with an opponent, opponent_params_dev must not be null");
    if (!out || !out->rewards || !out->flags || !out->actor.obs || !out->actor.actions)
        return fail(RSX_ERR_ARG, "out and its rewards, flags, actor.obs and actor.actions arrays must not be null");
    if (h->L > 32) return fail(RSX_ERR_ARG, "rsx_task_collect_team has no 64-lanes-per-env kernels (unset RSX_LANES_PER_ENV)");
    if (team_lds_bytes(h->L, h->P.obs_dim, h->M.act_dim, h->P.n_blue, S, opponent ? &S2 : nullptr) > 163840ll)
        return fail(RSX_ERR_ARG, "the policies' weights do not fit a CU's 160 KB of LDS at this observation width: use fewer or smaller hidden layers");
    hipStream_t s = (hipStream_t)stream;
    int fl = 0;
    if (int rc = step_prologue(h, s, (uint64_t)n_steps, &fl)) return rc;   // capture of a host-keyed handle, counter limit
    h->host_state_valid = false;
    const int grid = grid_for(h);   // (the tick slots: as rsx_task_collect_policy, the launch has its grid)
    if (h->tick_dev) launch_tick_fill(tick_slot0(h), h->tick_slots, grid, 0u, 1, s);
    h->P.tick_base = h->tick; h->tick += (uint32_t)n_steps;
    launch_task_collect_team(h->P, buffers_of(h, nullptr), h->L, h->NR, h->d_phys, S, actor_params_dev, (int)n_params, sigma_dev, actor_seats,
                             opponent ? &S2 : nullptr, opponent_params_dev, (int)n_opp_params, opponent_sigma_dev, opponent_seats,
                             h->M.act_dim, noise_seed, n_steps | fl, *out, s);
    if (h->tick_dev) launch_tick_fill(tick_slot0(h), grid, h->tick_slots, 0u, 1, s);
    HIP_TRY(launch_status());
    return debug_finite(h, s, "rsx_task_collect_team");
}

// ---- values and GAE advantages of a [T][B] batch (rsx.h: rsx_task_advantages).  The handle gives the device and obs_dim; nothing of it is touched ----
// what both calls check of a critic; on success S is the spec as the kernels take it and *n_params the floats of one critic
static int critic_prologue(const rsx_sim* h, const rsx_policy_mlp* c, PolicySpec* S, int64_t* n_params) {
    if (h->P.task == RSX_TASK_NONE) return fail(RSX_ERR_ARG, "no task attached (rsx_task_attach): the critic's obs_dim is the task's");
    if (!c) return fail(RSX_ERR_ARG, "the critic (rsx_policy_mlp) must not be null");
    if (c->n_hidden_layers != 1 && c->n_hidden_layers != 2) return fail(RSX_ERR_ARG, "n_hidden_layers must be 1 or 2");
    if (c->hidden != 32 && c->hidden != 64) return fail(RSX_ERR_ARG, "hidden must be 32 or 64");
    if (c->hidden_act != RSX_ACT_RELU && c->hidden_act != RSX_ACT_TANH) return fail(RSX_ERR_ARG, "hidden_act must be RSX_ACT_RELU or RSX_ACT_TANH");
    if (c->out_act != RSX_ACT_NONE) return fail(RSX_ERR_ARG, "a critic's out_act must be RSX_ACT_NONE (a linear output)");
    *S = PolicySpec{c->n_hidden_layers, c->hidden, c->hidden_act, c->out_act};
    const int64_t H = c->hidden;
    *n_params = H * h->P.obs_dim + H + (c->n_hidden_layers == 2 ? H * H + H : 0) + H + 1;
    return RSX_OK;
}

int rsx_critic_num_params(const rsx_sim* h, const rsx_policy_mlp* critic, int64_t* out) {
    if (!h) return fail(RSX_ERR_ARG, "null handle");
    if (!out) return fail(RSX_ERR_ARG, "out must not be null");
    PolicySpec S;
    return critic_prologue(h, critic, &S, out);
}

int rsx_task_advantages(rsx_sim* h, const rsx_policy_mlp* critic, const float* critic_params_dev, float gamma, float lam, int n_steps,
                        int n_envs, const rsx_adv_in* in, const rsx_adv_out* out, void* stream) {
    RSX_ENTER(h);   // (nothing the handle owns is read or written by the launches)
    PolicySpec S; int64_t n_params = 0;
    if (int rc = critic_prologue(h, critic, &S, &n_params)) return rc;
    if (n_steps < 1 || n_envs < 1) return fail(RSX_ERR_ARG, "n_steps and n_envs must be >= 1");
    if (!(std::isfinite(gamma) && gamma >= 0.0f && gamma <= 1.0f)) return fail(RSX_ERR_ARG, "gamma must be in [0, 1]");
    if (!(std::isfinite(lam) && lam >= 0.0f && lam <= 1.0f)) return fail(RSX_ERR_ARG, "lam must be in [0, 1]");
    if (!critic_params_dev) return fail(RSX_ERR_ARG, "critic_params_dev must not be null");
    if (!in || !in->obs || !in->rewards || !in->terminated || !in->truncated || !in->last_obs)
        return fail(RSX_ERR_ARG, "in and its obs, rewards, terminated, truncated and last_obs arrays must not be null");
    if (!out || !out->values || !out->advantages || !out->returns)
        return fail(RSX_ERR_ARG, "out and its values, advantages and returns arrays must not be null");
    const char* form_env = std::getenv("RSX_GAE_FORM");
    const int form = form_env && std::strcmp(form_env, "groups") == 0 ? GAE_FORM_GROUPS : GAE_FORM_ROWS;
    if (gae_lds_bytes(form, h->P.obs_dim, S) > 65536ll)
        return fail(RSX_ERR_ARG, "the critic's weights do not fit a workgroup's 64 KB of LDS at this observation width: use fewer or smaller hidden layers");
    const float gl = gamma * lam;   // (one rounding; the unit is built with -ffp-contract=off like every other)
    launch_advantages(form, S, critic_params_dev, h->P.obs_dim, gamma, gl, n_steps, n_envs, *in, *out, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

// ---- PPO loss gradients of an actor and a critic on a minibatch (rsx.h: rsx_task_ppo_gradient).  The handle as for rsx_task_advantages ----
// what both calls check of the two networks; on success the specs as the kernels take them and the floats of each
static int ppo_prologue(const rsx_sim* h, const rsx_policy_mlp* actor, const rsx_policy_mlp* critic, PolicySpec* SA, int64_t* n_actor,
                        PolicySpec* SC, int64_t* n_critic) {
    if (h->P.task == RSX_TASK_NONE) return fail(RSX_ERR_ARG, "no task attached (rsx_task_attach): obs_dim and act_dim are the task's");
    if (int rc = policy_prologue(h, actor, SA, n_actor)) return rc;
    if (int rc = critic_prologue(h, critic, SC, n_critic)) return rc;
    if (ppo_lds_bytes(h->P.obs_dim, h->M.act_dim, *SA) > 65536ll || ppo_lds_bytes(h->P.obs_dim, 1, *SC) > 65536ll)
        return fail(RSX_ERR_ARG, "a network's weights and row buffers do not fit a workgroup's 64 KB of LDS at this observation width: use fewer or smaller hidden layers");
    return RSX_OK;
}

int rsx_ppo_gradient_workspace(const rsx_sim* h, const rsx_policy_mlp* actor, const rsx_policy_mlp* critic, int64_t n_rows,
                               int max_workgroups, int64_t* bytes_out) {
    if (!h) return fail(RSX_ERR_ARG, "null handle");
    if (!bytes_out) return fail(RSX_ERR_ARG, "bytes_out must not be null");
    PolicySpec SA, SC; int64_t na = 0, nc = 0;
    if (int rc = ppo_prologue(h, actor, critic, &SA, &na, &SC, &nc)) return rc;
    if (n_rows < 1 || n_rows > 0x7FFFFFFFll) return fail(RSX_ERR_ARG, "n_rows must be in 1 .. 2^31 - 1");
    if (max_workgroups < 0) return fail(RSX_ERR_ARG, "max_workgroups must be >= 0");
    *bytes_out = ppo_workspace_bytes(na, nc, h->M.act_dim, n_rows, max_workgroups);
    return RSX_OK;
}

int rsx_task_ppo_gradient(rsx_sim* h, const rsx_policy_mlp* actor, const float* actor_params_dev, const float* log_std_dev,
                          const rsx_policy_mlp* critic, const float* critic_params_dev, const rsx_ppo_in* in, const rsx_ppo_cfg* cfg,
                          const rsx_ppo_out* out, void* stream) {
    RSX_ENTER(h);   // (nothing the handle owns is read or written by the launches)
    PolicySpec SA, SC; int64_t na = 0, nc = 0;
    if (int rc = ppo_prologue(h, actor, critic, &SA, &na, &SC, &nc)) return rc;
    if (!actor_params_dev || !log_std_dev || !critic_params_dev)
        return fail(RSX_ERR_ARG, "actor_params_dev, log_std_dev and critic_params_dev must not be null");
    if (!in || !in->obs || !in->sample || !in->old_log_prob || !in->advantage || !in->ret)
        return fail(RSX_ERR_ARG, "in and its obs, sample, old_log_prob, advantage and ret arrays must not be null");
    if (in->n_rows < 1 || in->n_batch_rows < 1 || in->n_rows > 0x7FFFFFFFll || in->n_batch_rows > 0x7FFFFFFFll)
        return fail(RSX_ERR_ARG, "n_rows and n_batch_rows must be in 1 .. 2^31 - 1");
    if (!cfg) return fail(RSX_ERR_ARG, "cfg must not be null");
    if (!(std::isfinite(cfg->clip) && cfg->clip > 0.0f && cfg->clip < 1.0f)) return fail(RSX_ERR_ARG, "clip must be in (0, 1)");
    if (!std::isfinite(cfg->vf_coef) || !std::isfinite(cfg->ent_coef)) return fail(RSX_ERR_ARG, "vf_coef and ent_coef must be finite");
    if (cfg->max_workgroups < 0) return fail(RSX_ERR_ARG, "max_workgroups must be >= 0");
    if (!out || !out->grad_actor || !out->grad_log_std || !out->grad_critic || !out->stats || !out->workspace)
        return fail(RSX_ERR_ARG, "out and its grad_actor, grad_log_std, grad_critic, stats and workspace must not be null");
    launch_ppo_gradient(SA, na, actor_params_dev, log_std_dev, SC, nc, critic_params_dev, h->P.obs_dim, h->M.act_dim, *in, *cfg, *out,
                        (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

// ---- TD3 / DDPG loss gradients of an actor and its Q critics on a minibatch (rsx.h: rsx_task_dpg_gradient).  The handle as above ----
// what both calls check of the networks; on success the specs as the kernels take them and the floats of one network of each kind
static int dpg_prologue(const rsx_sim* h, const rsx_policy_mlp* actor, const rsx_policy_mlp* critic, int n_critics, PolicySpec* SA,
                        int64_t* n_actor, PolicySpec* SC, int64_t* n_critic) {
    if (h->P.task == RSX_TASK_NONE) return fail(RSX_ERR_ARG, "no task attached (rsx_task_attach): obs_dim and act_dim are the task's");
    if (int rc = policy_prologue(h, actor, SA, n_actor)) return rc;
    if (int rc = critic_prologue(h, critic, SC, n_critic)) return rc;
    if (n_critics != 1 && n_critics != 2) return fail(RSX_ERR_ARG, "n_critics must be 1 or 2");
    const int OD = h->P.obs_dim, AD = h->M.act_dim;
    if (AD > 8) return fail(RSX_ERR_ARG, "act_dim above 8 is not supported");
    const int64_t H = critic->hidden;
    *n_critic = H * (OD + AD) + H + (critic->n_hidden_layers == 2 ? H * H + H : 0) + H + 1;   // (the input row is [obs | action])
    static const char* const names[3] = {"target", "critic", "actor"};
    for (int l = 0; l < 3; ++l) {
        const long long bytes = dpg_lds_bytes(l, OD, AD, *SA, *SC, n_critics);
        if (bytes > 163840ll) {
            char msg[200];
            std::snprintf(msg, sizeof msg, "the %s launch needs %lld bytes of LDS per workgroup, a CU has 163840: use fewer or smaller hidden layers",
                          names[l], bytes);
            return fail(RSX_ERR_ARG, msg);
        }
    }
    return RSX_OK;
}

int rsx_dpg_gradient_workspace(const rsx_sim* h, const rsx_policy_mlp* actor, const rsx_policy_mlp* critic, int n_critics, int64_t n_rows,
                               int max_workgroups, int64_t* bytes_out) {
    if (!h) return fail(RSX_ERR_ARG, "null handle");
    if (!bytes_out) return fail(RSX_ERR_ARG, "bytes_out must not be null");
    PolicySpec SA, SC; int64_t na = 0, nc = 0;
    if (int rc = dpg_prologue(h, actor, critic, n_critics, &SA, &na, &SC, &nc)) return rc;
    if (n_rows < 1 || n_rows > 0x7FFFFFFFll) return fail(RSX_ERR_ARG, "n_rows must be in 1 .. 2^31 - 1");
    if (max_workgroups < 0) return fail(RSX_ERR_ARG, "max_workgroups must be >= 0");
    *bytes_out = dpg_workspace_bytes(na, nc, n_critics, n_rows, max_workgroups);
    return RSX_OK;
}

// what the weighted calls check of rsx_grad_per against the per-entry outputs (q, target) the TD error is computed from
static int grad_per_check(const rsx_grad_per* per, const float* q, const float* target) {
    if (per && per->td_error && (!q || !target)) return fail(RSX_ERR_ARG, "per->td_error needs out->q and out->target: it is computed from them");
    return RSX_OK;
}

int rsx_task_dpg_gradient(rsx_sim* h, const rsx_policy_mlp* actor, const float* actor_params_dev, const float* target_actor_params_dev,
                          const rsx_policy_mlp* critic, const float* critic_params_dev, const float* target_critic_params_dev,
                          const rsx_dpg_in* in, const rsx_dpg_cfg* cfg, const rsx_dpg_out* out, void* stream) {
    return rsx_task_dpg_gradient_w(h, actor, actor_params_dev, target_actor_params_dev, critic, critic_params_dev, target_critic_params_dev, in,
                                   cfg, out, nullptr, stream);
}

int rsx_task_dpg_gradient_w(rsx_sim* h, const rsx_policy_mlp* actor, const float* actor_params_dev, const float* target_actor_params_dev,
                            const rsx_policy_mlp* critic, const float* critic_params_dev, const float* target_critic_params_dev,
                            const rsx_dpg_in* in, const rsx_dpg_cfg* cfg, const rsx_dpg_out* out, const rsx_grad_per* per, void* stream) {
    RSX_ENTER(h);   // (nothing the handle owns is read or written by the launches)
    if (!cfg) return fail(RSX_ERR_ARG, "cfg must not be null");
    PolicySpec SA, SC; int64_t na = 0, nc = 0;
    if (int rc = dpg_prologue(h, actor, critic, cfg->n_critics, &SA, &na, &SC, &nc)) return rc;
    if (!actor_params_dev || !target_actor_params_dev || !critic_params_dev || !target_critic_params_dev)
        return fail(RSX_ERR_ARG, "actor_params_dev, target_actor_params_dev, critic_params_dev and target_critic_params_dev must not be null");
    if (!in || !in->obs || !in->action || !in->reward || !in->next_obs || !in->terminated)
        return fail(RSX_ERR_ARG, "in and its obs, action, reward, next_obs and terminated arrays must not be null");
    if (in->n_rows < 1 || in->n_batch_rows < 1 || in->n_rows > 0x7FFFFFFFll || in->n_batch_rows > 0x7FFFFFFFll)
        return fail(RSX_ERR_ARG, "n_rows and n_batch_rows must be in 1 .. 2^31 - 1");
    if (!(std::isfinite(cfg->gamma) && cfg->gamma >= 0.0f && cfg->gamma <= 1.0f)) return fail(RSX_ERR_ARG, "gamma must be in [0, 1]");
    if (!(std::isfinite(cfg->sigma) && cfg->sigma >= 0.0f)) return fail(RSX_ERR_ARG, "sigma must be finite and >= 0");
    if (!(std::isfinite(cfg->noise_clip) && cfg->noise_clip >= 0.0f)) return fail(RSX_ERR_ARG, "noise_clip must be finite and >= 0");
    if (cfg->max_workgroups < 0) return fail(RSX_ERR_ARG, "max_workgroups must be >= 0");
    if (!out || !out->grad_critics || !out->stats || !out->workspace)
        return fail(RSX_ERR_ARG, "out and its grad_critics, stats and workspace must not be null");
    if (int rc = grad_per_check(per, out->q, out->target)) return rc;
    launch_dpg_gradient(SA, na, actor_params_dev, target_actor_params_dev, SC, nc, critic_params_dev, target_critic_params_dev, h->P.obs_dim,
                        h->M.act_dim, *in, *cfg, *out, (hipStream_t)stream, per);
    if (per && per->td_error) launch_replay_td_error(out->q, out->target, cfg->n_critics, in->n_rows, per->td_error, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

// ---- soft actor-critic loss gradients of a squashed Gaussian actor, its Q critics and the temperature (rsx.h: rsx_task_sac_gradient) ----
// what both calls check of the networks (dpg_prologue's checks with the actor's output layer 2 * act_dim wide and out_act = RSX_ACT_NONE)
static int sac_prologue(const rsx_sim* h, const rsx_policy_mlp* actor, const rsx_policy_mlp* critic, int n_critics, PolicySpec* SA,
                        int64_t* n_actor, PolicySpec* SC, int64_t* n_critic) {
    if (h->P.task == RSX_TASK_NONE) return fail(RSX_ERR_ARG, "no task attached (rsx_task_attach): obs_dim and act_dim are the task's");
    if (!actor) return fail(RSX_ERR_ARG, "the actor (rsx_policy_mlp) must not be null");
    rsx_policy_mlp shape = *actor;
    shape.out_act = RSX_ACT_TANH;   // (what the head applies; the shape's own checks are rsx_task_dpg_gradient's)
    if (int rc = policy_prologue(h, &shape, SA, n_actor)) return rc;
    if (actor->out_act != RSX_ACT_NONE)
        return fail(RSX_ERR_ARG, "rsx_task_sac_gradient: the actor's out_act must be RSX_ACT_NONE (the head clamps the log-std and squashes the sample itself)");
    SA->out_act = RSX_ACT_NONE;
    if (int rc = critic_prologue(h, critic, SC, n_critic)) return rc;
    if (n_critics != 1 && n_critics != 2) return fail(RSX_ERR_ARG, "n_critics must be 1 or 2");
    const int OD = h->P.obs_dim, AD = h->M.act_dim;
    if (AD > 8) return fail(RSX_ERR_ARG, "act_dim above 8 is not supported");
    *n_actor += (int64_t)AD * actor->hidden + AD;   // the output layer is 2 * act_dim units wide
    const int64_t H = critic->hidden;
    *n_critic = H * (OD + AD) + H + (critic->n_hidden_layers == 2 ? H * H + H : 0) + H + 1;   // (the input row is [obs | action])
    static const char* const names[5] = {"target", "critic", "sample", "critic-on-sample", "actor"};
    for (int l = 0; l < 5; ++l) {
        const long long bytes = sac_lds_bytes(l, OD, AD, *SA, *SC, n_critics);
        if (bytes > 163840ll) {
            char msg[200];
            std::snprintf(msg, sizeof msg, "the %s launch needs %lld bytes of LDS per workgroup, a CU has 163840: use fewer or smaller hidden layers",
                          names[l], bytes);
            return fail(RSX_ERR_ARG, msg);
        }
    }
    return RSX_OK;
}

int rsx_sac_gradient_workspace(const rsx_sim* h, const rsx_policy_mlp* actor, const rsx_policy_mlp* critic, int n_critics, int64_t n_rows,
                               int max_workgroups, int64_t* bytes_out) {
    if (!h) return fail(RSX_ERR_ARG, "null handle");
    if (!bytes_out) return fail(RSX_ERR_ARG, "bytes_out must not be null");
    PolicySpec SA, SC; int64_t na = 0, nc = 0;
    if (int rc = sac_prologue(h, actor, critic, n_critics, &SA, &na, &SC, &nc)) return rc;
    if (n_rows < 1 || n_rows > 0x7FFFFFFFll) return fail(RSX_ERR_ARG, "n_rows must be in 1 .. 2^31 - 1");
    if (max_workgroups < 0) return fail(RSX_ERR_ARG, "max_workgroups must be >= 0");
    *bytes_out = sac_workspace_bytes(na, nc, n_critics, n_rows, max_workgroups);
    return RSX_OK;
}

int rsx_task_sac_gradient(rsx_sim* h, const rsx_policy_mlp* actor, const float* actor_params_dev, const rsx_policy_mlp* critic,
                          const float* critic_params_dev, const float* target_critic_params_dev, const float* log_alpha_dev,
                          const rsx_dpg_in* in, const rsx_sac_cfg* cfg, const rsx_sac_out* out, void* stream) {
    return rsx_task_sac_gradient_w(h, actor, actor_params_dev, critic, critic_params_dev, target_critic_params_dev, log_alpha_dev, in, cfg, out,
                                   nullptr, stream);
}

int rsx_task_sac_gradient_w(rsx_sim* h, const rsx_policy_mlp* actor, const float* actor_params_dev, const rsx_policy_mlp* critic,
                            const float* critic_params_dev, const float* target_critic_params_dev, const float* log_alpha_dev,
                            const rsx_dpg_in* in, const rsx_sac_cfg* cfg, const rsx_sac_out* out, const rsx_grad_per* per, void* stream) {
    RSX_ENTER(h);   // (nothing the handle owns is read or written by the launches)
    if (!cfg) return fail(RSX_ERR_ARG, "cfg must not be null");
    PolicySpec SA, SC; int64_t na = 0, nc = 0;
    if (int rc = sac_prologue(h, actor, critic, cfg->n_critics, &SA, &na, &SC, &nc)) return rc;
    if (!actor_params_dev || !critic_params_dev || !target_critic_params_dev || !log_alpha_dev)
        return fail(RSX_ERR_ARG, "actor_params_dev, critic_params_dev, target_critic_params_dev and log_alpha_dev must not be null");
    if (!in || !in->obs || !in->action || !in->reward || !in->next_obs || !in->terminated)
        return fail(RSX_ERR_ARG, "in and its obs, action, reward, next_obs and terminated arrays must not be null");
    if (in->n_rows < 1 || in->n_batch_rows < 1 || in->n_rows > 0x7FFFFFFFll || in->n_batch_rows > 0x7FFFFFFFll)
        return fail(RSX_ERR_ARG, "n_rows and n_batch_rows must be in 1 .. 2^31 - 1");
    if (!(std::isfinite(cfg->gamma) && cfg->gamma >= 0.0f && cfg->gamma <= 1.0f)) return fail(RSX_ERR_ARG, "gamma must be in [0, 1]");
    if (!std::isfinite(cfg->target_entropy)) return fail(RSX_ERR_ARG, "target_entropy must be finite");
    if (!std::isfinite(cfg->log_std_min) || !std::isfinite(cfg->log_std_max) || !(cfg->log_std_min < cfg->log_std_max))
        return fail(RSX_ERR_ARG, "log_std_min and log_std_max must be finite with log_std_min < log_std_max");
    if (cfg->max_workgroups < 0) return fail(RSX_ERR_ARG, "max_workgroups must be >= 0");
    if (!out || !out->grad_actor || !out->grad_critics || !out->grad_log_alpha || !out->stats || !out->workspace)
        return fail(RSX_ERR_ARG, "out and its grad_actor, grad_critics, grad_log_alpha, stats and workspace must not be null");
    if (int rc = grad_per_check(per, out->q, out->target)) return rc;
    launch_sac_gradient(SA, na, actor_params_dev, SC, nc, critic_params_dev, target_critic_params_dev, log_alpha_dev, h->P.obs_dim,
                        h->M.act_dim, *in, *cfg, *out, (hipStream_t)stream, per);
    if (per && per->td_error) launch_replay_td_error(out->q, out->target, cfg->n_critics, in->n_rows, per->td_error, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

// ---- the off-policy update phase around it (rsx.h: rsx_replay_sample_rows, rsx_dpg_adam_step, rsx_task_dpg_update) ----
// what rsx_replay_sample_rows and rsx_task_dpg_update check of a row draw
static int sample_rows_check(int64_t m, int64_t n_batch_rows, int64_t fill, const int64_t* fill_dev) {
    if (m < 1 || m > 0x7FFFFFFFll) return fail(RSX_ERR_ARG, "m (the rows to draw) must be in 1 .. 2^31 - 1");
    if (n_batch_rows < 1 || n_batch_rows > 0x7FFFFFFFll) return fail(RSX_ERR_ARG, "n_batch_rows must be in 1 .. 2^31 - 1");
    if (!fill_dev && fill < 0) return fail(RSX_ERR_ARG, "fill must be >= 0");
    return RSX_OK;
}

int rsx_replay_sample_rows(int32_t* rows_dev, int64_t m, int64_t n_batch_rows, int64_t fill, const int64_t* fill_dev, uint64_t seed,
                           int64_t step, const int64_t* step_dev, void* stream) {
    (void)launch_status();
    if (!rows_dev) return fail(RSX_ERR_ARG, "rows_dev must not be null");
    if (int rc = sample_rows_check(m, n_batch_rows, fill, fill_dev)) return rc;
    launch_replay_sample_rows(rows_dev, m, n_batch_rows, fill, reinterpret_cast<const long long*>(fill_dev), seed, step,
                              reinterpret_cast<const long long*>(step_dev), (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

// what rsx_dpg_adam_step and rsx_task_dpg_update check of the two-group optimiser's configuration and state
static int dpg_adam_prologue(const rsx_dpg_adam_cfg* c, const rsx_dpg_adam_state* st) {
    if (!c) return fail(RSX_ERR_ARG, "the optimiser's configuration (rsx_dpg_adam_cfg) must not be null");
    if (!(std::isfinite(c->lr_actor) && c->lr_actor >= 0.0f)) return fail(RSX_ERR_ARG, "lr_actor must be finite and >= 0");
    if (!(std::isfinite(c->lr_critic) && c->lr_critic >= 0.0f)) return fail(RSX_ERR_ARG, "lr_critic must be finite and >= 0");
    if (!(std::isfinite(c->eps) && c->eps >= 0.0f)) return fail(RSX_ERR_ARG, "eps must be finite and >= 0");
    if (!(c->beta1 >= 0.0 && c->beta1 < 1.0) || !(c->beta2 >= 0.0 && c->beta2 < 1.0)) return fail(RSX_ERR_ARG, "beta1 and beta2 must be in [0, 1)");
    if (!std::isfinite(c->max_grad_norm)) return fail(RSX_ERR_ARG, "max_grad_norm must be finite (<= 0: no clipping)");
    if (!(c->tau >= 0.0f && c->tau <= 1.0f)) return fail(RSX_ERR_ARG, "tau must be in [0, 1]");   // (a NaN fails both comparisons)
    if (!st) return fail(RSX_ERR_ARG, "the optimiser's state (rsx_dpg_adam_state) must not be null");
    if (!st->m_actor || !st->v_actor || !st->m_critic || !st->v_critic || !st->counters)
        return fail(RSX_ERR_ARG, "the state's m, v and counters arrays must not be null");
    if (st->n_actor < 1 || st->n_critic < 1 || st->n_actor > 0x7FFFFFFFll || st->n_critic > 0x7FFFFFFFll)
        return fail(RSX_ERR_ARG, "n_actor and n_critic must be in 1 .. 2^31 - 1");
    return RSX_OK;
}

int rsx_dpg_adam_step(const rsx_dpg_adam_cfg* cfg, const rsx_dpg_adam_state* st, const rsx_dpg_adam_io* io, void* stream) {
    (void)launch_status();
    if (int rc = dpg_adam_prologue(cfg, st)) return rc;
    if (!io || !io->actor_params || !io->critic_params || !io->grad_critic || !io->workspace)
        return fail(RSX_ERR_ARG, "io and its actor_params, critic_params, grad_critic and workspace must not be null");
    if (io->update_targets && (!io->target_actor_params || !io->target_critic_params))
        return fail(RSX_ERR_ARG, "update_targets needs target_actor_params and target_critic_params");
    launch_dpg_adam_step(*cfg, *st, *io, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_dpg_update_workspace(const rsx_sim* h, const rsx_policy_mlp* actor, const rsx_policy_mlp* critic, int n_critics, int64_t n_rows,
                             int max_workgroups, int64_t* bytes_out, int64_t* rows_offset_out) {
    if (!h) return fail(RSX_ERR_ARG, "null handle");
    if (!bytes_out) return fail(RSX_ERR_ARG, "bytes_out must not be null");
    PolicySpec SA, SC; int64_t na = 0, nc = 0;
    if (int rc = dpg_prologue(h, actor, critic, n_critics, &SA, &na, &SC, &nc)) return rc;
    if (n_rows < 1 || n_rows > 0x7FFFFFFFll) return fail(RSX_ERR_ARG, "n_rows must be in 1 .. 2^31 - 1");
    if (max_workgroups < 0) return fail(RSX_ERR_ARG, "max_workgroups must be >= 0");
    long long off = 0;
    *bytes_out = dpg_update_workspace_bytes(na, nc, n_critics, n_rows, max_workgroups, &off);
    if (rows_offset_out) *rows_offset_out = off;
    return RSX_OK;
}

int rsx_task_dpg_update(rsx_sim* h, const rsx_policy_mlp* actor, float* actor_params_dev, float* target_actor_params_dev,
                        const rsx_policy_mlp* critic, float* critic_params_dev, float* target_critic_params_dev, const rsx_dpg_in* in,
                        const rsx_dpg_cfg* cfg, const rsx_dpg_update_cfg* u, const rsx_dpg_adam_cfg* adam, const rsx_dpg_adam_state* st,
                        float* stats_dev, void* workspace, void* stream) {
    RSX_ENTER(h);   // (nothing the handle owns is read or written by the launches)
    if (!cfg) return fail(RSX_ERR_ARG, "cfg must not be null");
    PolicySpec SA, SC; int64_t na = 0, nc = 0;
    if (int rc = dpg_prologue(h, actor, critic, cfg->n_critics, &SA, &na, &SC, &nc)) return rc;
    if (!actor_params_dev || !target_actor_params_dev || !critic_params_dev || !target_critic_params_dev)
        return fail(RSX_ERR_ARG, "actor_params_dev, target_actor_params_dev, critic_params_dev and target_critic_params_dev must not be null");
    if (!in || !in->obs || !in->action || !in->reward || !in->next_obs || !in->terminated)
        return fail(RSX_ERR_ARG, "in and its obs, action, reward, next_obs and terminated arrays must not be null");
    if (in->rows) return fail(RSX_ERR_ARG, "in->rows must be NULL: the update draws its own rows");
    if (!(std::isfinite(cfg->gamma) && cfg->gamma >= 0.0f && cfg->gamma <= 1.0f)) return fail(RSX_ERR_ARG, "gamma must be in [0, 1]");
    if (!(std::isfinite(cfg->sigma) && cfg->sigma >= 0.0f)) return fail(RSX_ERR_ARG, "sigma must be finite and >= 0");
    if (!(std::isfinite(cfg->noise_clip) && cfg->noise_clip >= 0.0f)) return fail(RSX_ERR_ARG, "noise_clip must be finite and >= 0");
    if (cfg->max_workgroups < 0) return fail(RSX_ERR_ARG, "max_workgroups must be >= 0");
    if (!u) return fail(RSX_ERR_ARG, "the update's configuration (rsx_dpg_update_cfg) must not be null");
    if (u->grad_steps < 1) return fail(RSX_ERR_ARG, "grad_steps must be >= 1");
    if (u->policy_delay < 1) return fail(RSX_ERR_ARG, "policy_delay must be >= 1");
    if (u->grad_steps % u->policy_delay != 0) return fail(RSX_ERR_ARG, "grad_steps must be a multiple of policy_delay");
    if (int rc = sample_rows_check(in->n_rows, in->n_batch_rows, u->fill, u->fill_dev)) return rc;
    if (int rc = dpg_adam_prologue(adam, st)) return rc;
    if (st->n_actor != na || st->n_critic != (int64_t)cfg->n_critics * nc)
        return fail(RSX_ERR_ARG, "the optimiser state's sizes (n_actor, n_critic) are not those of the actor and of n_critics critics");
    if (!stats_dev || !workspace) return fail(RSX_ERR_ARG, "stats_dev and workspace must not be null");
    launch_dpg_update(SA, na, actor_params_dev, target_actor_params_dev, SC, nc, critic_params_dev, target_critic_params_dev, h->P.obs_dim,
                      h->M.act_dim, *in, *cfg, *u, *adam, *st, stats_dev, workspace, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

// ---- prioritised and n-step replay (rsx.h: rsx_replay_add_nstep, rsx_replay_set_priorities, rsx_replay_sample_prioritized) ----
int rsx_replay_add_nstep(const rsx_replay_batch* b, const rsx_replay_ring* r, int n_step, float gamma, void* stream) {
    (void)launch_status();
    if (!b || !b->obs || !b->actions || !b->reward || !b->terminated || !b->truncated || !b->final_obs || !b->next_obs)
        return fail(RSX_ERR_ARG, "the batch and its obs, actions, reward, terminated, truncated, final_obs and next_obs arrays must not be null");
    if (!r || !r->obs || !r->actions || !r->reward || !r->next_obs || !r->terminated || !r->discount || !r->head_dev || !r->fill_dev || !r->ticket_dev)
        return fail(RSX_ERR_ARG, "the ring and its obs, actions, reward, next_obs, terminated, discount, head_dev, fill_dev and ticket_dev must not be null");
    if (r->capacity < 1 || r->capacity > 0x7FFFFFFFll) return fail(RSX_ERR_ARG, "capacity must be in 1 .. 2^31 - 1");
    if (r->obs_dim < 1 || r->act_dim < 1) return fail(RSX_ERR_ARG, "obs_dim and act_dim must be >= 1");
    if (b->T < 1 || b->B < 1) return fail(RSX_ERR_ARG, "T and B must be >= 1");
    if ((long long)b->T * b->B > r->capacity) return fail(RSX_ERR_ARG, "the batch has more rows (T * B) than the ring's capacity");
    if (n_step < 1 || n_step > 16) return fail(RSX_ERR_ARG, "n_step must be in 1 .. 16");
    if (!(std::isfinite(gamma) && gamma >= 0.0f && gamma <= 1.0f)) return fail(RSX_ERR_ARG, "gamma must be in [0, 1]");
    launch_replay_add_nstep(*b, *r, n_step, gamma, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_replay_tree_geometry(int64_t capacity, int64_t* floats_out, int32_t* levels_out, int64_t* offsets_out) {
    if (capacity < 1 || capacity > 0x7FFFFFFFll) return fail(RSX_ERR_ARG, "capacity must be in 1 .. 2^31 - 1");
    long long floats = 0, off[8];
    int levels = 0;
    replay_tree_geometry(capacity, &floats, &levels, off);
    if (floats_out) *floats_out = floats;
    if (levels_out) *levels_out = levels;
    if (offsets_out)
        for (int l = 0; l < 8; ++l) offsets_out[l] = off[l];
    return RSX_OK;
}

int rsx_replay_set_priorities(float* tree_dev, void* state_dev, int64_t capacity, const int32_t* rows_dev, const float* td_error_dev,
                              const int64_t* head_dev, int64_t m, float alpha, float eps, void* stream) {
    (void)launch_status();
    if (!tree_dev || !state_dev) return fail(RSX_ERR_ARG, "tree_dev and state_dev must not be null");
    if (!rows_dev && !head_dev) return fail(RSX_ERR_ARG, "rows_dev and head_dev must not both be null");
    if (capacity < 1 || capacity > 0x7FFFFFFFll) return fail(RSX_ERR_ARG, "capacity must be in 1 .. 2^31 - 1");
    if (m < 1 || m > 0x7FFFFFFFll) return fail(RSX_ERR_ARG, "m (the entries) must be in 1 .. 2^31 - 1");
    if (!rows_dev && m > capacity) return fail(RSX_ERR_ARG, "m must not exceed the capacity when the rows are those behind the write head");
    if (!(std::isfinite(alpha) && alpha >= 0.0f)) return fail(RSX_ERR_ARG, "alpha must be finite and >= 0");
    if (!(std::isfinite(eps) && eps >= 0.0f)) return fail(RSX_ERR_ARG, "eps must be finite and >= 0");
    launch_replay_set_priorities(tree_dev, state_dev, capacity, rows_dev, td_error_dev, reinterpret_cast<const long long*>(head_dev), m, alpha,
                                 eps, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_replay_sample_prioritized(const float* tree_dev, void* state_dev, int64_t capacity, int64_t fill, const int64_t* fill_dev,
                                  int32_t* rows_out, float* weights_out, int64_t m, float beta, const float* beta_dev, uint64_t seed,
                                  int64_t step, const int64_t* step_dev, void* stream) {
    (void)launch_status();
    if (!tree_dev || !state_dev || !rows_out || !weights_out)
        return fail(RSX_ERR_ARG, "tree_dev, state_dev, rows_out and weights_out must not be null");
    if (int rc = sample_rows_check(m, capacity, fill, fill_dev)) return rc;
    if (!beta_dev && !(std::isfinite(beta) && beta >= 0.0f)) return fail(RSX_ERR_ARG, "beta must be finite and >= 0");
    HIP_TRY(launch_replay_sample_prioritized(tree_dev, state_dev, capacity, fill, reinterpret_cast<const long long*>(fill_dev), rows_out,
                                             weights_out, m, beta, beta_dev, seed, step, reinterpret_cast<const long long*>(step_dev),
                                             (hipStream_t)stream));
    HIP_TRY(launch_status());
    return RSX_OK;
}

// ---- the soft actor-critic update phase (rsx.h: rsx_sac_adam_step, rsx_task_sac_update) ----
// what rsx_sac_adam_step and rsx_task_sac_update check of the three-group optimiser's configuration and state
static int sac_adam_prologue(const rsx_sac_adam_cfg* c, const rsx_sac_adam_state* st) {
    if (!c) return fail(RSX_ERR_ARG, "the optimiser's configuration (rsx_sac_adam_cfg) must not be null");
    if (!(std::isfinite(c->lr_actor) && c->lr_actor >= 0.0f)) return fail(RSX_ERR_ARG, "lr_actor must be finite and >= 0");
    if (!(std::isfinite(c->lr_critic) && c->lr_critic >= 0.0f)) return fail(RSX_ERR_ARG, "lr_critic must be finite and >= 0");
    if (!(std::isfinite(c->lr_alpha) && c->lr_alpha >= 0.0f)) return fail(RSX_ERR_ARG, "lr_alpha must be finite and >= 0");
    if (!(std::isfinite(c->eps) && c->eps >= 0.0f)) return fail(RSX_ERR_ARG, "eps must be finite and >= 0");
    if (!(c->beta1 >= 0.0 && c->beta1 < 1.0) || !(c->beta2 >= 0.0 && c->beta2 < 1.0)) return fail(RSX_ERR_ARG, "beta1 and beta2 must be in [0, 1)");
    if (!std::isfinite(c->max_grad_norm)) return fail(RSX_ERR_ARG, "max_grad_norm must be finite (<= 0: no clipping)");
    if (!(c->tau >= 0.0f && c->tau <= 1.0f)) return fail(RSX_ERR_ARG, "tau must be in [0, 1]");   // (a NaN fails both comparisons)
    if (!st) return fail(RSX_ERR_ARG, "the optimiser's state (rsx_sac_adam_state) must not be null");
    if (!st->m_actor || !st->v_actor || !st->m_critic || !st->v_critic || !st->m_alpha || !st->v_alpha || !st->counters)
        return fail(RSX_ERR_ARG, "the state's m, v (actor, critic, alpha) and counters arrays must not be null");
    if (st->n_actor < 1 || st->n_critic < 1 || st->n_actor > 0x7FFFFFFFll || st->n_critic > 0x7FFFFFFFll)
        return fail(RSX_ERR_ARG, "n_actor and n_critic must be in 1 .. 2^31 - 1");
    return RSX_OK;
}

int rsx_sac_adam_step(const rsx_sac_adam_cfg* cfg, const rsx_sac_adam_state* st, const rsx_sac_adam_io* io, void* stream) {
    (void)launch_status();
    if (int rc = sac_adam_prologue(cfg, st)) return rc;
    if (!io || !io->actor_params || !io->critic_params || !io->log_alpha || !io->grad_critic || !io->workspace)
        return fail(RSX_ERR_ARG, "io and its actor_params, critic_params, log_alpha, grad_critic and workspace must not be null");
    if (io->update_targets && !io->target_critic_params) return fail(RSX_ERR_ARG, "update_targets needs target_critic_params");
    launch_sac_adam_step(*cfg, *st, *io, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_sac_update_workspace(const rsx_sim* h, const rsx_policy_mlp* actor, const rsx_policy_mlp* critic, int n_critics, int64_t n_rows,
                             int max_workgroups, int64_t* bytes_out, int64_t* rows_offset_out) {
    if (!h) return fail(RSX_ERR_ARG, "null handle");
    if (!bytes_out) return fail(RSX_ERR_ARG, "bytes_out must not be null");
    PolicySpec SA, SC; int64_t na = 0, nc = 0;
    if (int rc = sac_prologue(h, actor, critic, n_critics, &SA, &na, &SC, &nc)) return rc;
    if (n_rows < 1 || n_rows > 0x7FFFFFFFll) return fail(RSX_ERR_ARG, "n_rows must be in 1 .. 2^31 - 1");
    if (max_workgroups < 0) return fail(RSX_ERR_ARG, "max_workgroups must be >= 0");
    long long off = 0;
    *bytes_out = sac_update_workspace_bytes(na, nc, n_critics, n_rows, max_workgroups, &off);
    if (rows_offset_out) *rows_offset_out = off;
    return RSX_OK;
}

int rsx_task_sac_update(rsx_sim* h, const rsx_policy_mlp* actor, float* actor_params_dev, const rsx_policy_mlp* critic,
                        float* critic_params_dev, float* target_critic_params_dev, float* log_alpha_dev, const rsx_dpg_in* in,
                        const rsx_sac_cfg* cfg, const rsx_sac_update_cfg* u, const rsx_sac_adam_cfg* adam, const rsx_sac_adam_state* st,
                        float* stats_dev, void* workspace, void* stream) {
    RSX_ENTER(h);   // (nothing the handle owns is read or written by the launches)
    if (!cfg) return fail(RSX_ERR_ARG, "cfg must not be null");
    PolicySpec SA, SC; int64_t na = 0, nc = 0;
    if (int rc = sac_prologue(h, actor, critic, cfg->n_critics, &SA, &na, &SC, &nc)) return rc;
    if (!actor_params_dev || !critic_params_dev || !target_critic_params_dev || !log_alpha_dev)
        return fail(RSX_ERR_ARG, "actor_params_dev, critic_params_dev, target_critic_params_dev and log_alpha_dev must not be null");
    if (!in || !in->obs || !in->action || !in->reward || !in->next_obs || !in->terminated)
        return fail(RSX_ERR_ARG, "in and its obs, action, reward, next_obs and terminated arrays must not be null");
    if (in->rows) return fail(RSX_ERR_ARG, "in->rows must be NULL: the update draws its own rows");
    if (!(std::isfinite(cfg->gamma) && cfg->gamma >= 0.0f && cfg->gamma <= 1.0f)) return fail(RSX_ERR_ARG, "gamma must be in [0, 1]");
    if (!std::isfinite(cfg->target_entropy)) return fail(RSX_ERR_ARG, "target_entropy must be finite");
    if (!std::isfinite(cfg->log_std_min) || !std::isfinite(cfg->log_std_max) || !(cfg->log_std_min < cfg->log_std_max))
        return fail(RSX_ERR_ARG, "log_std_min and log_std_max must be finite with log_std_min < log_std_max");
    if (cfg->max_workgroups < 0) return fail(RSX_ERR_ARG, "max_workgroups must be >= 0");
    if (!u) return fail(RSX_ERR_ARG, "the update's configuration (rsx_sac_update_cfg) must not be null");
    if (u->grad_steps < 1) return fail(RSX_ERR_ARG, "grad_steps must be >= 1");
    if (int rc = sample_rows_check(in->n_rows, in->n_batch_rows, u->fill, u->fill_dev)) return rc;
    if (int rc = sac_adam_prologue(adam, st)) return rc;
    if (st->n_actor != na || st->n_critic != (int64_t)cfg->n_critics * nc)
        return fail(RSX_ERR_ARG, "the optimiser state's sizes (n_actor, n_critic) are not those of the actor and of n_critics critics");
    if (!stats_dev || !workspace) return fail(RSX_ERR_ARG, "stats_dev and workspace must not be null");
    launch_sac_update(SA, na, actor_params_dev, SC, nc, critic_params_dev, target_critic_params_dev, log_alpha_dev, h->P.obs_dim,
                      h->M.act_dim, *in, *cfg, *u, *adam, *st, stats_dev, workspace, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

// ---- the update phase around it (rsx.h: rsx_ppo_normalize, rsx_ppo_permutation, rsx_adam_step, rsx_adam_mark, rsx_task_ppo_update) ----
// what rsx_adam_step and rsx_task_ppo_update check of an optimiser's configuration and state
static int adam_prologue(const rsx_adam_cfg* c, const rsx_adam_state* st) {
    if (!c) return fail(RSX_ERR_ARG, "the optimiser's configuration (rsx_adam_cfg) must not be null");
    if (!(std::isfinite(c->lr) && c->lr >= 0.0f)) return fail(RSX_ERR_ARG, "lr must be finite and >= 0");
    if (!(std::isfinite(c->eps) && c->eps >= 0.0f)) return fail(RSX_ERR_ARG, "eps must be finite and >= 0");
    if (!(c->beta1 >= 0.0 && c->beta1 < 1.0) || !(c->beta2 >= 0.0 && c->beta2 < 1.0)) return fail(RSX_ERR_ARG, "beta1 and beta2 must be in [0, 1)");
    if (!std::isfinite(c->max_grad_norm)) return fail(RSX_ERR_ARG, "max_grad_norm must be finite (<= 0: no clipping)");
    if (!(std::isfinite(c->target_kl) && c->target_kl >= 0.0f)) return fail(RSX_ERR_ARG, "target_kl must be finite and >= 0 (0: no KL stop)");
    if (!st) return fail(RSX_ERR_ARG, "the optimiser's state (rsx_adam_state) must not be null");
    if (!st->m_actor || !st->v_actor || !st->m_log_std || !st->v_log_std || !st->m_critic || !st->v_critic || !st->counters)
        return fail(RSX_ERR_ARG, "the state's m, v and counters arrays must not be null");
    if (st->n_actor < 1 || st->n_log_std < 1 || st->n_critic < 1 || st->n_actor > 0x7FFFFFFFll || st->n_log_std > 0x7FFFFFFFll ||
        st->n_critic > 0x7FFFFFFFll || st->n_actor + st->n_log_std + st->n_critic > 0x7FFFFFFFll)
        return fail(RSX_ERR_ARG, "n_actor, n_log_std and n_critic must be >= 1 and their sum at most 2^31 - 1");
    return RSX_OK;
}

int rsx_ppo_normalize(const float* adv_dev, int64_t n, float eps, float* out_dev, float* mean_std_dev, void* workspace_dev, void* stream) {
    (void)launch_status();
    if (!adv_dev || !out_dev || !workspace_dev) return fail(RSX_ERR_ARG, "adv_dev, out_dev and workspace_dev must not be null");
    if (n < 2 || n > 0x7FFFFFFFll) return fail(RSX_ERR_ARG, "n must be in 2 .. 2^31 - 1 (one entry has no standard deviation)");
    if (!(std::isfinite(eps) && eps >= 0.0f)) return fail(RSX_ERR_ARG, "eps must be finite and >= 0");
    launch_ppo_normalize(adv_dev, n, eps, out_dev, mean_std_dev, workspace_dev, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_ppo_permutation(int32_t* rows_dev, int64_t n, uint64_t seed, uint64_t update, const int64_t* update_dev, int64_t epoch, void* stream) {
    (void)launch_status();
    if (!rows_dev) return fail(RSX_ERR_ARG, "rows_dev must not be null");
    if (n < 1 || n > 0x7FFFFFFFll) return fail(RSX_ERR_ARG, "n must be in 1 .. 2^31 - 1");
    if (epoch < 0 || epoch > 0xFFFFFFFFll) return fail(RSX_ERR_ARG, "epoch must be in 0 .. 2^32 - 1");
    launch_ppo_permutation(rows_dev, n, seed, (uint32_t)update, reinterpret_cast<const long long*>(update_dev), (uint32_t)epoch, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_adam_step(const rsx_adam_cfg* cfg, const rsx_adam_state* st, const rsx_adam_io* io, void* stream) {
    (void)launch_status();
    if (int rc = adam_prologue(cfg, st)) return rc;
    if (!io || !io->actor_params || !io->log_std || !io->critic_params || !io->grad_actor || !io->grad_log_std || !io->grad_critic || !io->workspace)
        return fail(RSX_ERR_ARG, "io and its parameter, gradient and workspace arrays must not be null");
    launch_adam_step(*cfg, *st, *io, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_adam_mark(const rsx_adam_state* st, int end, void* stream) {
    (void)launch_status();
    if (!st || !st->counters) return fail(RSX_ERR_ARG, "the state and its counters must not be null");
    launch_update_mark(st->counters, end ? 1 : 0, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

// what both calls check of the batch's size and its split
static int update_split(int64_t n_batch_rows, int minibatches) {
    if (n_batch_rows < 1 || n_batch_rows > 0x7FFFFFFFll) return fail(RSX_ERR_ARG, "n_batch_rows must be in 1 .. 2^31 - 1");
    if (minibatches < 1) return fail(RSX_ERR_ARG, "minibatches must be >= 1");
    if ((int64_t)(minibatches - 1) * ppo_update_chunk(n_batch_rows, minibatches) >= n_batch_rows)
        return fail(RSX_ERR_ARG, "minibatches: the last chunk of ceil(n / minibatches) rows would be empty");
    return RSX_OK;
}

int rsx_ppo_update_workspace(const rsx_sim* h, const rsx_policy_mlp* actor, const rsx_policy_mlp* critic, int64_t n_batch_rows,
                             int minibatches, int max_workgroups, int64_t* bytes_out, int64_t* rows_offset_out) {
    if (!h) return fail(RSX_ERR_ARG, "null handle");
    if (!bytes_out) return fail(RSX_ERR_ARG, "bytes_out must not be null");
    PolicySpec SA, SC; int64_t na = 0, nc = 0;
    if (int rc = ppo_prologue(h, actor, critic, &SA, &na, &SC, &nc)) return rc;
    if (int rc = update_split(n_batch_rows, minibatches)) return rc;
    if (max_workgroups < 0) return fail(RSX_ERR_ARG, "max_workgroups must be >= 0");
    long long off = 0;
    *bytes_out = ppo_update_workspace_bytes(na, nc, h->M.act_dim, n_batch_rows, minibatches, max_workgroups, &off);
    if (rows_offset_out) *rows_offset_out = off;
    return RSX_OK;
}

int rsx_task_ppo_update(rsx_sim* h, const rsx_policy_mlp* actor, float* actor_params_dev, float* log_std_dev, const rsx_policy_mlp* critic,
                        float* critic_params_dev, const rsx_ppo_in* in, const rsx_ppo_cfg* cfg, const rsx_ppo_update_cfg* u,
                        const rsx_adam_cfg* adam, const rsx_adam_state* st, float* stats_dev, void* workspace, void* stream) {
    RSX_ENTER(h);   // (nothing the handle owns is read or written by the launches)
    PolicySpec SA, SC; int64_t na = 0, nc = 0;
    if (int rc = ppo_prologue(h, actor, critic, &SA, &na, &SC, &nc)) return rc;
    if (!actor_params_dev || !log_std_dev || !critic_params_dev)
        return fail(RSX_ERR_ARG, "actor_params_dev, log_std_dev and critic_params_dev must not be null");
    if (!in || !in->obs || !in->sample || !in->old_log_prob || !in->advantage || !in->ret)
        return fail(RSX_ERR_ARG, "in and its obs, sample, old_log_prob, advantage and ret arrays must not be null");
    if (in->rows) return fail(RSX_ERR_ARG, "in->rows must be NULL: the update draws its own rows");
    if (!cfg) return fail(RSX_ERR_ARG, "cfg must not be null");
    if (!(std::isfinite(cfg->clip) && cfg->clip > 0.0f && cfg->clip < 1.0f)) return fail(RSX_ERR_ARG, "clip must be in (0, 1)");
    if (!std::isfinite(cfg->vf_coef) || !std::isfinite(cfg->ent_coef)) return fail(RSX_ERR_ARG, "vf_coef and ent_coef must be finite");
    if (cfg->max_workgroups < 0) return fail(RSX_ERR_ARG, "max_workgroups must be >= 0");
    if (!u) return fail(RSX_ERR_ARG, "the update's configuration (rsx_ppo_update_cfg) must not be null");
    if (u->epochs < 1) return fail(RSX_ERR_ARG, "epochs must be >= 1");
    if (int rc = update_split(in->n_batch_rows, u->minibatches)) return rc;
    if (u->normalize_advantage && in->n_batch_rows < 2) return fail(RSX_ERR_ARG, "normalize_advantage needs at least 2 rows");
    if (!(std::isfinite(u->norm_eps) && u->norm_eps >= 0.0f)) return fail(RSX_ERR_ARG, "norm_eps must be finite and >= 0");
    if (int rc = adam_prologue(adam, st)) return rc;
    if (st->n_actor != na || st->n_log_std != h->M.act_dim || st->n_critic != nc)
        return fail(RSX_ERR_ARG, "the optimiser state's sizes (n_actor, n_log_std, n_critic) are not those of the two networks and act_dim");
    if (!stats_dev || !workspace) return fail(RSX_ERR_ARG, "stats_dev and workspace must not be null");
    launch_ppo_update(SA, na, actor_params_dev, log_std_dev, SC, nc, critic_params_dev, h->P.obs_dim, h->M.act_dim, *in, *cfg, *u, *adam, *st,
                      stats_dev, workspace, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

// ---- planning with candidates drawn on the device (rsx.h: rsx_plan_sampler) ----
// what the three calls check alike; on success S is the sampler as the kernels take it and P the handle's parameters with the step
// counter the next step would take (not advanced).  n_steps: what the counter limit is checked against (0: the call simulates nothing)
static int plan_prologue(rsx_sim* h, const rsx_plan_sampler* s, int n_candidates, int horizon, int n_steps, hipStream_t stream, Params* P,
                         PlanSampler* S) {
    if (h->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached (rsx_task_attach)");
    RSX_NEED_RESET(h);
    if (n_candidates < 1 || horizon < 1) return fail(RSX_ERR_ARG, "n_candidates and horizon must be >= 1");
    if (!s) return fail(RSX_ERR_ARG, "the sampler (rsx_plan_sampler) must not be null");
    if (s->hold < 1) return fail(RSX_ERR_ARG, "hold must be >= 1");
    if (!std::isfinite(s->sigma) || s->sigma < 0.0f) return fail(RSX_ERR_ARG, "sigma must be finite and >= 0");
    const int nblk = (h->M.act_dim + 3) / 4;
    if ((long long)((horizon + s->hold - 1) / s->hold) * (long long)nblk > (1ll << 24))
        return fail(RSX_ERR_ARG, "too many noise blocks: ceil(horizon / hold) * ceil(act_dim / 4) must fit in 24 bits");
    int fl = 0;
    if (int rc = step_prologue(h, stream, (uint64_t)n_steps, &fl)) return rc;   // capture of a host-keyed handle, counter limit
    *P = h->P;
    P->tick_base = h->tick;
    *S = PlanSampler{(uint32_t)s->sample_seed, (uint32_t)(s->sample_seed >> 32), s->sigma, s->hold, nblk};
    return RSX_OK;
}

int rsx_task_lookahead_sampled(rsx_sim* h, const float* mean_dev, const rsx_plan_sampler* s, int n_candidates, int horizon, float gamma,
                               float* returns_dev, int32_t* steps_dev, uint8_t* flags_dev, float* last_obs_dev, void* stream) {
    RSX_ENTER(h);   // (as rsx_task_lookahead: nothing the handle owns changes)
    if (!returns_dev || !steps_dev || !flags_dev) return fail(RSX_ERR_ARG, "returns_dev, steps_dev and flags_dev must not be null");
    if (!std::isfinite(gamma)) return fail(RSX_ERR_ARG, "gamma must be finite");
    if (h->L > 32) return fail(RSX_ERR_ARG, "rsx_task_lookahead_sampled has no 64-lanes-per-env kernels (unset RSX_LANES_PER_ENV)");
    if (lookahead_grid(h->L, h->P.num_envs, n_candidates > 0 ? n_candidates : 1) > 0x7FFFFFFFll)
        return fail(RSX_ERR_ARG, "num_envs x n_candidates exceeds the launch limit (2^31 - 1 workgroups): split the candidates over several calls");
    Params P; PlanSampler S;
    if (int rc = plan_prologue(h, s, n_candidates, horizon, horizon, (hipStream_t)stream, &P, &S)) return rc;
    launch_task_lookahead_sampled(P, h->L, h->NR, h->d_state, h->d_aux, h->tick_dev ? tick_slot0(h) : nullptr, h->d_phys, mean_dev, S,
                                  n_candidates, horizon, gamma, returns_dev, steps_dev, flags_dev, last_obs_dev, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_plan_candidates(rsx_sim* h, const float* mean_dev, const rsx_plan_sampler* s, int n_candidates, int horizon, float* actions_out_dev,
                        void* stream) {
    RSX_ENTER(h);
    if (!actions_out_dev) return fail(RSX_ERR_ARG, "actions_out_dev must not be null");
    Params P; PlanSampler S;
    if (int rc = plan_prologue(h, s, n_candidates, horizon, 0, (hipStream_t)stream, &P, &S)) return rc;
    if (plan_flat_grid(P.num_envs, n_candidates, horizon, S.nblk) > 0x7FFFFFFFll)
        return fail(RSX_ERR_ARG, "num_envs x n_candidates x horizon exceeds the launch limit: split the candidates over several calls");
    launch_plan_candidates(P, h->tick_dev ? tick_slot0(h) : nullptr, mean_dev, S, n_candidates, horizon, h->M.act_dim, actions_out_dev,
                           (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_plan_update(rsx_sim* h, const float* mean_dev, const rsx_plan_sampler* s, int n_candidates, int horizon, const float* returns_dev,
                    float temperature, float* new_mean_dev, int32_t* best_dev, void* stream) {
    RSX_ENTER(h);
    if (!returns_dev || !new_mean_dev) return fail(RSX_ERR_ARG, "returns_dev and new_mean_dev must not be null");
    if (!std::isfinite(temperature) || temperature < 0.0f) return fail(RSX_ERR_ARG, "temperature must be finite and >= 0");
    Params P; PlanSampler S;
    if (int rc = plan_prologue(h, s, n_candidates, horizon, 0, (hipStream_t)stream, &P, &S)) return rc;
    if (plan_flat_grid(P.num_envs, 1, horizon, S.nblk) > 0x7FFFFFFFll)
        return fail(RSX_ERR_ARG, "num_envs x horizon exceeds the launch limit");
    // in place is safe (every element is read and written by one thread); any other overlap of the two plans is not
    if (mean_dev && mean_dev != new_mean_dev) {
        const size_t bytes = (size_t)P.num_envs * (size_t)horizon * (size_t)h->M.act_dim * sizeof(float);
        const char *a = (const char*)mean_dev, *b = (const char*)new_mean_dev;
        if (a < b + bytes && b < a + bytes) return fail(RSX_ERR_ARG, "new_mean_dev overlaps mean_dev: pass the same pointer (in place) or disjoint arrays");
    }
    launch_plan_update(P, h->tick_dev ? tick_slot0(h) : nullptr, mean_dev, S, n_candidates, horizon, h->M.act_dim, returns_dev, temperature,
                       new_mean_dev, best_dev, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

// ---- task checkpoint: everything a fused run needs to continue bit-identically ----
namespace {
struct CkptHeader {
    uint64_t magic;            // "RSXCKPT2"
    int32_t abi, kind, field_rows, task, n_blue, n_yellow, num_envs, state_rows, aux_rows, obs_dim;
    int32_t field_type, time_step_ms, max_steps, model;   // model: RSX_PHYSICS_MODEL of the saving library
    uint32_t key0, key1, env_id_base, tick;
    uint64_t state_bytes, aux_bytes, obs_bytes, flag_bytes;
    int64_t metrics[RSX_METRICS];
};
constexpr uint64_t CKPT_MAGIC = 0x3254504B43585352ull;   // "RSXCKPT2", little endian
// model word of a physics-enabled handle's blob: a section follows the others — the physics header (ranges), the parameter rows
// and the coefficient rows (dense, like the rest); a blob of either kind is refused by a handle of the other
constexpr int32_t CKPT_MODEL_PHYS = 1 << 16;
size_t ckpt_phys_bytes(const CkptHeader& k) {
    return (k.model & CKPT_MODEL_PHYS) ? sizeof(PhysHeader) + (size_t)(NPHYS + NCOEF) * (size_t)k.num_envs * sizeof(float) : 0;
}
CkptHeader ckpt_header(const rsx_sim* h) {
    CkptHeader k{};
    const size_t B = (size_t)h->P.num_envs;
    k.magic = CKPT_MAGIC; k.abi = RSX_ABI_VERSION; k.kind = h->P.kind; k.field_rows = h->M.rs; k.task = h->P.task;
    k.n_blue = h->P.n_blue; k.n_yellow = h->P.n_yellow; k.num_envs = h->P.num_envs;
    k.state_rows = state_rows(h); k.aux_rows = aux_rows(h->P.n_robots); k.obs_dim = h->P.obs_dim;
    k.field_type = h->field_type; k.time_step_ms = h->time_step_ms; k.max_steps = h->P.max_steps; k.model = RSX_PHYSICS_MODEL | (h->d_phys ? CKPT_MODEL_PHYS : 0);
    k.key0 = h->P.key0; k.key1 = h->P.key1; k.env_id_base = h->P.env_id_base; k.tick = h->tick;
    k.state_bytes = (uint64_t)k.state_rows * B * sizeof(float);
    k.aux_bytes = (uint64_t)k.aux_rows * B * sizeof(float);
    k.obs_bytes = (uint64_t)B * k.obs_dim * sizeof(float);
    k.flag_bytes = 2 * B;
    return k;
}
size_t ckpt_size(const CkptHeader& k) { return sizeof(CkptHeader) + k.state_bytes + k.aux_bytes + 2 * k.obs_bytes + k.flag_bytes + ckpt_phys_bytes(k); }
}  // namespace

int rsx_task_checkpoint_size(rsx_sim* h, size_t* bytes) {
    if (!h || !bytes) return fail(RSX_ERR_ARG, "null argument");
    if (h->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached (rsx_task_attach)");
    *bytes = ckpt_size(ckpt_header(h));
    return RSX_OK;
}

int rsx_task_checkpoint_save(rsx_sim* h, void* blob, size_t bytes, void* stream) {
    RSX_ENTER_TASK(h);
    if (!blob) return fail(RSX_ERR_ARG, "blob is null");
    CkptHeader k = ckpt_header(h);
    if (bytes < ckpt_size(k)) return fail(RSX_ERR_ARG, "blob is smaller than rsx_task_checkpoint_size");
    hipStream_t s = (hipStream_t)stream;
    launch_fold_metrics(h->d_metrics, h->d_mslots, s);
    HIP_TRY(launch_status());
    char* p = (char*)blob + sizeof(CkptHeader);
    // (the blob's rows are dense — B floats — whatever the row pad of this handle: it restores into any layout)
    const size_t rowb = (size_t)h->P.num_envs * sizeof(float), pitch = (size_t)h->P.row_stride * sizeof(float);
    HIP_TRY(hipMemcpy2DAsync(p, rowb, h->d_state, pitch, rowb, (size_t)k.state_rows, hipMemcpyDeviceToHost, s)); p += k.state_bytes;
    HIP_TRY(hipMemcpy2DAsync(p, rowb, h->d_aux, pitch, rowb, (size_t)k.aux_rows, hipMemcpyDeviceToHost, s)); p += k.aux_bytes;
    HIP_TRY(hipMemcpyAsync(p, h->d_obs, k.obs_bytes, hipMemcpyDeviceToHost, s)); p += k.obs_bytes;
    HIP_TRY(hipMemcpyAsync(p, h->d_final_obs, k.obs_bytes, hipMemcpyDeviceToHost, s)); p += k.obs_bytes;
    HIP_TRY(hipMemcpyAsync(p, h->d_flags, k.flag_bytes, hipMemcpyDeviceToHost, s));
    if (h->d_phys) {
        p += k.flag_bytes;
        HIP_TRY(hipMemcpyAsync(p, h->d_phys, sizeof(PhysHeader), hipMemcpyDeviceToHost, s)); p += sizeof(PhysHeader);
        HIP_TRY(hipMemcpy2DAsync(p, rowb, phys_raw(h->d_phys), pitch, rowb, (size_t)(NPHYS + NCOEF), hipMemcpyDeviceToHost, s));   // raw rows, then the coefficient rows
    }
    HIP_TRY(hipMemcpyAsync(k.metrics, h->d_metrics, sizeof(k.metrics), hipMemcpyDeviceToHost, s));
    if (h->tick_dev)   // device-keyed handle: the step counter is slot 0 of the per-workgroup slots (all equal between launches)
        HIP_TRY(hipMemcpyAsync(&k.tick, tick_slot0(h), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h->tick_dev) h->tick = k.tick;
    std::memcpy(blob, &k, sizeof(k));
    if (h->P.task == RSX_TASK_VSS_V0) {
        // The task scalar of VSS-v0 (previous ball potential, vss_gym.py:256-283) is a function of the ball position
        // the next step starts from; the one-lane-per-env kernel recomputes it instead of keeping the row up to date.
        // The blob always carries the value, so that it restores into either kernel layout.  Same float expression
        // as the kernels' (rsx_math.hpp: vss_ball_potential).
        const size_t B = (size_t)h->P.num_envs;
        const float* st = reinterpret_cast<const float*>((const char*)blob + sizeof(CkptHeader));
        float* aux = reinterpret_cast<float*>((char*)blob + sizeof(CkptHeader) + k.state_bytes);
        for (size_t e = 0; e < B; ++e) aux[(size_t)ROW_PREV_POT * B + e] = vss_ball_potential(st[e], st[B + e], h->P.hl_goal, h->P.inv_len_cm);
    }
    return RSX_OK;
}

int rsx_task_checkpoint_load(rsx_sim* h, const void* blob, size_t bytes, void* stream) {
    RSX_ENTER_TASK(h);
    if (!blob || bytes < sizeof(CkptHeader)) return fail(RSX_ERR_ARG, "blob is null or truncated");
    CkptHeader k;
    std::memcpy(&k, blob, sizeof(k));
    CkptHeader want = ckpt_header(h);
    if (k.magic != CKPT_MAGIC || k.abi != want.abi) return fail(RSX_ERR_ARG, "not a checkpoint of this library version");
    if ((k.model & CKPT_MODEL_PHYS) != (want.model & CKPT_MODEL_PHYS))
        return fail(RSX_ERR_ARG, "the checkpoint was taken from a handle with per-env physics on / off and this one has it off / on (rsx_physics_enable)");
    if (k.model != want.model) return fail(RSX_ERR_ARG, "the checkpoint was taken under another version of the physics model (RSX_PHYSICS_MODEL)");
    if (k.kind != want.kind || k.task != want.task || k.n_blue != want.n_blue || k.n_yellow != want.n_yellow ||
        k.num_envs != want.num_envs || k.state_rows != want.state_rows || k.aux_rows != want.aux_rows || k.obs_dim != want.obs_dim)
        return fail(RSX_ERR_ARG, "the checkpoint was taken from a different configuration (simulator kind, team sizes, batch or task)");
    if (k.field_type != want.field_type || k.time_step_ms != want.time_step_ms || k.field_rows != want.field_rows)
        return fail(RSX_ERR_ARG, "the checkpoint was taken with another field type or time step");
    if (k.max_steps != want.max_steps)
        return fail(RSX_ERR_ARG, "the checkpoint was taken with another max_episode_steps (TimeLimit)");
    if (k.key0 != want.key0 || k.key1 != want.key1 || k.env_id_base != want.env_id_base)
        return fail(RSX_ERR_ARG, "the checkpoint was taken with another seed or env_id_base: attach the task with the same ones");
    // the section sizes follow from the configuration checked above; they are used for pointer arithmetic and as copy lengths below,
    // so a header that disagrees (a damaged file) is refused instead of being trusted
    if (k.state_bytes != want.state_bytes || k.aux_bytes != want.aux_bytes || k.obs_bytes != want.obs_bytes || k.flag_bytes != want.flag_bytes)
        return fail(RSX_ERR_ARG, "the checkpoint header is damaged (section sizes do not match its configuration)");
    if (bytes < ckpt_size(k)) return fail(RSX_ERR_ARG, "blob is truncated");
    hipStream_t s = (hipStream_t)stream;
    const char* p = (const char*)blob + sizeof(CkptHeader);
    h->host_state_valid = false;
    const size_t rowb = (size_t)h->P.num_envs * sizeof(float), pitch = (size_t)h->P.row_stride * sizeof(float);
    HIP_TRY(hipMemcpy2DAsync(h->d_state, pitch, p, rowb, rowb, (size_t)k.state_rows, hipMemcpyHostToDevice, s)); p += k.state_bytes;
    HIP_TRY(hipMemcpy2DAsync(h->d_aux, pitch, p, rowb, rowb, (size_t)k.aux_rows, hipMemcpyHostToDevice, s)); p += k.aux_bytes;
    HIP_TRY(hipMemcpyAsync(h->d_obs, p, k.obs_bytes, hipMemcpyHostToDevice, s)); p += k.obs_bytes;
    HIP_TRY(hipMemcpyAsync(h->d_final_obs, p, k.obs_bytes, hipMemcpyHostToDevice, s)); p += k.obs_bytes;
    HIP_TRY(hipMemcpyAsync(h->d_flags, p, k.flag_bytes, hipMemcpyHostToDevice, s));
    if (h->d_phys) {   // ranges and mask of the blob, this handle's error word
        p += k.flag_bytes;
        PhysHeader hd;
        std::memcpy(&hd, p, sizeof(hd)); p += sizeof(PhysHeader);
        if (hd.kind != h->P.kind || hd.ts_ms != h->time_step_ms) return fail(RSX_ERR_ARG, "the checkpoint's physics section is damaged");
        launch_phys_ranges(h->d_phys, hd.lo, hd.hi, hd.mask, s);
        HIP_TRY(launch_status());
        HIP_TRY(hipMemcpy2DAsync(phys_raw(h->d_phys), pitch, p, rowb, rowb, (size_t)(NPHYS + NCOEF), hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemsetAsync(h->d_mslots, 0, (size_t)MSLOTS * RSX_METRICS * sizeof(unsigned long long), s));
    HIP_TRY(hipMemcpyAsync(h->d_metrics, k.metrics, sizeof(k.metrics), hipMemcpyHostToDevice, s));
    if (h->tick_dev) {   // device-keyed handle: every slot takes the blob's step counter; a refused-launch mark is cleared with it
        launch_tick_fill(tick_slot0(h), 0, h->tick_slots_alloc, k.tick, 0, s);
        HIP_TRY(launch_status());
        HIP_TRY(hipMemsetAsync(tick_words(h) + TICK_ERR_WORD, 0, sizeof(uint32_t), s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    h->tick = k.tick;
    h->task_ready = true;
    return RSX_OK;
}

int rsx_metrics_fold(rsx_sim* h, void* stream) {
    RSX_ENTER_TASK(h);
    launch_fold_metrics(h->d_metrics, h->d_mslots, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_read_metrics(rsx_sim* h, int64_t out[RSX_METRICS], void* stream) {
    RSX_ENTER_TASK(h);
    if (!out) return fail(RSX_ERR_ARG, "out is null");
    hipStream_t s = (hipStream_t)stream;
    launch_fold_metrics(h->d_metrics, h->d_mslots, s);
    HIP_TRY(launch_status());
    HIP_TRY(hipMemcpyAsync(out, h->d_metrics, RSX_METRICS * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    uint32_t refused = 0;
    if (h->tick_dev) HIP_TRY(hipMemcpyAsync(&refused, tick_words(h) + TICK_ERR_WORD, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (refused) return fail(RSX_ERR_STATE, "step counter exhausted: stepping launches of this device-keyed handle were refused on the device (out[] is valid; a handle takes at most 2^32 - 1 fused steps)");
    return RSX_OK;
}

// ---- transfer of running episodes between envs and handles ----
// the count of skipped pairs lives in a spare word of the task arena's metrics block (metrics[8] | ... | step-counter slots from
// TICK_SLOT_WORD0), zeroed by rsx_task_attach / rsx_task_reseed: a cross-handle transfer allocates nothing
constexpr int XFER_ERR_WORD = 20;
static_assert(XFER_ERR_WORD >= 2 * RSX_METRICS && XFER_ERR_WORD != TICK_ERR_WORD && XFER_ERR_WORD < TICK_SLOT_WORD0, "spare word of the metrics block");

static XferSide xfer_side_of(const rsx_sim* h) {
    return XferSide{h->d_state, h->d_aux, h->d_phys ? phys_raw(h->d_phys) : nullptr, h->d_obs, h->d_final_obs, h->d_flags,
                    h->P.row_stride, h->P.num_envs};
}

int rsx_task_transfer(rsx_sim* dst, rsx_sim* src, const int32_t* dst_ids_dev, const int32_t* src_ids_dev, int n, void* stream) {
    if (!src) return fail(RSX_ERR_ARG, "null handle");
    RSX_ENTER_TASK(dst);
    if (src->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached to the source (rsx_task_attach)");
    if (!dst->task_ready || !src->task_ready)
        return fail(RSX_ERR_STATE, "rsx_task_reset / rsx_task_reset_to must come before rsx_task_transfer, on both handles");
    if (src->device != dst->device) return fail(RSX_ERR_ARG, "the handles live on different devices");
    const Params &D = dst->P, &S = src->P;
    if (D.kind != S.kind || D.task != S.task || D.n_blue != S.n_blue || D.n_yellow != S.n_yellow)
        return fail(RSX_ERR_ARG, "the handles differ in simulator kind, task or team sizes");
    if (dst->field_type != src->field_type || dst->time_step_ms != src->time_step_ms)
        return fail(RSX_ERR_ARG, "the handles differ in field type or time step");
    if (D.max_steps != S.max_steps) return fail(RSX_ERR_ARG, "the handles differ in max_episode_steps (TimeLimit)");
    if ((dst->d_phys != nullptr) != (src->d_phys != nullptr))
        return fail(RSX_ERR_ARG, "per-env physics is enabled on one handle only (rsx_physics_enable)");
    if (n < 0) return fail(RSX_ERR_ARG, "n must be >= 0");
    if ((!dst_ids_dev && n > D.num_envs) || (!src_ids_dev && n > S.num_envs))
        return fail(RSX_ERR_ARG, "n exceeds num_envs of a side without an id array (NULL = envs 0..n-1)");
    if (n == 0) return RSX_OK;
    hipStream_t s = (hipStream_t)stream;
    const int SR = state_rows(dst), AR = aux_rows(D.n_robots), PR = dst->d_phys ? NPHYS + NCOEF : 0, OD = D.obs_dim;
    const int pot_row = D.task == RSX_TASK_VSS_V0 ? SR + ROW_PREV_POT : -1;
    uint32_t* const err = tick_words(dst) + XFER_ERR_WORD;
    // (the placement cache of either handle needs no invalidation: an entry is tagged with the episode id it was made for and is a
    // pure function of (seed, global env id, episode) — a tag that no longer matches takes the inline path, one that matches by
    // coincidence holds the right placement)
    if (dst != src) {
        launch_transfer(XFER_DIRECT, xfer_side_of(dst), xfer_side_of(src), D.num_envs, S.num_envs, dst_ids_dev, src_ids_dev, n, err,
                        SR, AR, PR, OD, pot_row, D.hl_goal, D.inv_len_cm, s);
        HIP_TRY(launch_status());
        return RSX_OK;
    }
    // same handle: every read before every write — gather the n records into the staging buffer, then scatter them
    rsx_sim* const h = dst;
    if (n > h->xfer_cap) {
        if (stream_is_capturing(s))
            return fail(RSX_ERR_STATE, "a same-handle rsx_task_transfer whose staging buffer has to grow cannot be captured: make one eager call with n = " +
                                       std::to_string(n) + " (or more) before the capture");
        HIP_TRY(hipStreamSynchronize(s));
        char* p = nullptr;
        HIP_TRY(hipMalloc((void**)&p, carve_xfer_stage(nullptr, (size_t)n, SR, AR, OD)));
        h->xfer_stage.push_back(p);
        h->xfer_cap = n;
    }
    XferSide st{};
    carve_xfer_stage(h->xfer_stage.back(), (size_t)h->xfer_cap, SR, AR, OD, &st);
    launch_transfer(XFER_GATHER, st, xfer_side_of(h), D.num_envs, D.num_envs, dst_ids_dev, src_ids_dev, n, err, SR, AR, PR, OD, pot_row,
                    D.hl_goal, D.inv_len_cm, s);
    launch_transfer(XFER_SCATTER, xfer_side_of(h), st, D.num_envs, D.num_envs, dst_ids_dev, src_ids_dev, n, err, SR, AR, PR, OD, -1,
                    D.hl_goal, D.inv_len_cm, s);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_task_transfer_errors(rsx_sim* dst, int64_t* out, void* stream) {
    RSX_ENTER(dst);
    if (dst->P.task == RSX_TASK_NONE) return fail(RSX_ERR_STATE, "no task attached (rsx_task_attach)");
    if (!out) return fail(RSX_ERR_ARG, "out is null");
    return read_and_clear_word(tick_words(dst) + XFER_ERR_WORD, out, (hipStream_t)stream);
}

}  // extern "C"
