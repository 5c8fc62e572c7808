// rsx_api_ext.hip — the extensions of the C-ABI that work on a handle's state from outside the step: per-env physics parameters
// (rsx_physics_*), trace evaluation (rsx_trace_*) and batched rgb frames (rsx_render_*).  Host code only.
#include <cmath>
#include <cstring>

#include "rsx_handle.hpp"

using namespace rsx;

// ---- per-env physics parameters (rsx.h: rsx_physics_*; kernels and block layout: rsx_phys.hip, rsx_phys.hpp) ----
extern "C" {

int rsx_physics_defaults(int kind, float out[RSX_PHYS_PARAMS]) {
    if (kind != RSX_KIND_VSS && kind != RSX_KIND_SSL) return fail(RSX_ERR_ARG, "kind must be RSX_KIND_VSS or RSX_KIND_SSL");
    if (!out) return fail(RSX_ERR_ARG, "out is null");
    for (int p = 0; p < NPHYS; ++p) out[p] = (float)phys_default(kind, p);
    return RSX_OK;
}

int rsx_physics_derive(int kind, int time_step_ms, const float raw[RSX_PHYS_PARAMS], float coef[RSX_PHYS_COEFS]) {
    if (kind != RSX_KIND_VSS && kind != RSX_KIND_SSL) return fail(RSX_ERR_ARG, "kind must be RSX_KIND_VSS or RSX_KIND_SSL");
    if (!raw || !coef || time_step_ms < 0) return fail(RSX_ERR_ARG, "null argument or negative time step");
    for (int p = 0; p < NPHYS; ++p)
        if (!phys_valid(kind, p, raw[p])) return fail(RSX_ERR_ARG, "physics parameter " + std::to_string(p) + " out of range (rsx.h: rsx_physics_*)");
    derive_coefs(kind, time_step_ms, raw, coef);
    return RSX_OK;
}

int rsx_physics_enable(rsx_sim* h, void* stream) {
    RSX_ENTER(h);
    if (h->d_phys) return RSX_OK;
    if (h->L > 32) return fail(RSX_ERR_ARG, "per-env physics runs with up to 32 lanes per env (unset RSX_LANES_PER_ENV=64)");
    if (h->tick_dev) return fail(RSX_ERR_STATE, "call rsx_physics_enable before rsx_task_enable_capture");
    hipStream_t s = (hipStream_t)stream;
    const size_t S = (size_t)h->P.row_stride;
    HIP_TRY(hipMalloc((void**)&h->d_phys, phys_block_bytes(S)));
    HIP_TRY(hipMemsetAsync(h->d_phys, 0, phys_block_bytes(S), s));
    PhysHeader hd{};
    hd.kind = h->P.kind; hd.ts_ms = h->time_step_ms;
    HIP_TRY(hipMemcpyAsync(h->d_phys, &hd, sizeof(hd), hipMemcpyHostToDevice, s));
    launch_phys_init(h->d_phys, h->P.num_envs, (int)S, h->P.kind, h->time_step_ms, s);
    HIP_TRY(launch_status());
    HIP_TRY(hipStreamSynchronize(s));   // (the header travels from the stack)
    if (h->P.task != RSX_TASK_NONE) plan_stepping(h);   // attached already: the layout of a physics-enabled handle
    return RSX_OK;
}

int rsx_physics_set(rsx_sim* h, const float* values, int on_device, const uint8_t* env_mask, void* stream) {
    RSX_ENTER(h);
    if (!h->d_phys) return fail(RSX_ERR_STATE, "per-env physics is off (rsx_physics_enable)");
    if (!values) return fail(RSX_ERR_ARG, "values is null");
    hipStream_t s = (hipStream_t)stream;
    const int B = h->P.num_envs;
    const size_t S = (size_t)h->P.row_stride;
    h->host_state_valid = false;
    if (on_device) {
        launch_phys_set(h->d_phys, values, env_mask, B, (int)S, B, s);
        HIP_TRY(launch_status());
        return RSX_OK;
    }
    // host values: checked here (NaN = keep), then staged and written by the same kernel
    for (int e = 0; e < B; ++e) {
        if (env_mask && !env_mask[e]) continue;
        for (int p = 0; p < NPHYS; ++p) {
            const float v = values[(size_t)p * B + e];
            if (v == v && !phys_valid(h->P.kind, p, v))
                return fail(RSX_ERR_ARG, "physics parameter " + std::to_string(p) + " of env " + std::to_string(e) + " out of range (rsx.h: rsx_physics_*)");
        }
    }
    float* const stage = phys_stage(h->d_phys, S);
    uint8_t* const smask = phys_stage_mask(h->d_phys, S);
    HIP_TRY(hipMemcpyAsync(stage, values, (size_t)NPHYS * B * sizeof(float), hipMemcpyHostToDevice, s));
    if (env_mask) HIP_TRY(hipMemcpyAsync(smask, env_mask, (size_t)B, hipMemcpyHostToDevice, s));
    launch_phys_set(h->d_phys, stage, env_mask ? smask : nullptr, B, (int)S, B, s);
    HIP_TRY(launch_status());
    HIP_TRY(hipStreamSynchronize(s));   // the caller's arrays may go away on return
    return RSX_OK;
}

int rsx_physics_get(rsx_sim* h, int which, float* out, void* stream) {
    RSX_ENTER(h);
    if (!h->d_phys) return fail(RSX_ERR_STATE, "per-env physics is off (rsx_physics_enable)");
    if (!out || (which != RSX_PHYS_RAW && which != RSX_PHYS_COEF)) return fail(RSX_ERR_ARG, "out is null or `which` unknown");
    hipStream_t s = (hipStream_t)stream;
    const size_t S = (size_t)h->P.row_stride, rowb = (size_t)h->P.num_envs * sizeof(float);
    const float* src = which == RSX_PHYS_RAW ? phys_raw(h->d_phys) : phys_coef(h->d_phys, S);
    HIP_TRY(hipMemcpy2DAsync(out, rowb, src, S * sizeof(float), rowb, (size_t)(which == RSX_PHYS_RAW ? NPHYS : NCOEF), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return RSX_OK;
}

int rsx_physics_randomize(rsx_sim* h, const float* lo, const float* hi, uint32_t param_mask, void* stream) {
    RSX_ENTER(h);
    if (!h->d_phys) return fail(RSX_ERR_STATE, "per-env physics is off (rsx_physics_enable)");
    if (param_mask >> NPHYS) return fail(RSX_ERR_ARG, "param_mask names a parameter that does not exist");
    if (param_mask && (!lo || !hi)) return fail(RSX_ERR_ARG, "lo / hi are null");
    for (int p = 0; p < NPHYS; ++p) {
        if (!((param_mask >> p) & 1u)) continue;
        if (!phys_valid(h->P.kind, p, lo[p]) || !phys_valid(h->P.kind, p, hi[p]) || !(lo[p] <= hi[p]))
            return fail(RSX_ERR_ARG, "randomisation range of physics parameter " + std::to_string(p) + " is invalid (lo <= hi, both valid values)");
    }
    launch_phys_ranges(h->d_phys, param_mask ? lo : nullptr, param_mask ? hi : nullptr, param_mask, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_physics_errors(rsx_sim* h, int64_t* out, void* stream) {
    RSX_ENTER(h);
    if (!h->d_phys) return fail(RSX_ERR_STATE, "per-env physics is off (rsx_physics_enable)");
    if (!out) return fail(RSX_ERR_ARG, "out is null");
    return read_and_clear_word(&reinterpret_cast<PhysHeader*>(h->d_phys)->err, out, (hipStream_t)stream);
}

// ---- trace evaluation (rsx.h: rsx_trace_*; kernel: rsx_sysid.hip) ----
int rsx_trace_load(rsx_sim* h, const double* frames, const double* cmds, int n_frames, const int32_t* anchors, int n_anchors,
                   void* stream) {
    RSX_ENTER(h);
    if (!h->d_phys) return fail(RSX_ERR_STATE, "trace evaluation needs per-env physics (rsx_physics_enable)");
    if (h->P.task != RSX_TASK_NONE) return fail(RSX_ERR_STATE, "trace evaluation runs on a raw handle: a task is attached");
    if (!frames || !cmds || !anchors) return fail(RSX_ERR_ARG, "null argument");
    if (n_frames < 2 || n_anchors < 1) return fail(RSX_ERR_ARG, "a trace needs n_frames >= 2 and n_anchors >= 1");
    if (h->P.num_envs % n_anchors != 0) return fail(RSX_ERR_ARG, "num_envs must be a multiple of n_anchors");
    const int rows = state_rows(h), NC = h->P.n_robots * h->M.cmd_dim;
    const size_t F = (size_t)n_frames, T = F - 1;
    if ((size_t)rows * F * sizeof(float) >= ((size_t)1 << 32) || (size_t)NC * T * sizeof(float) >= ((size_t)1 << 32))
        return fail(RSX_ERR_ARG, "trace too long: its arrays would reach 4 GB");
    int amax = 0;
    for (int a = 0; a < n_anchors; ++a) {
        if (anchors[a] < 0 || anchors[a] > n_frames - 2) return fail(RSX_ERR_ARG, "anchor " + std::to_string(a) + " outside [0, n_frames - 2]");
        amax = std::max(amax, (int)anchors[a]);
    }
    const size_t fbytes = align_up((size_t)rows * F * sizeof(float)), cbytes = align_up((size_t)NC * T * sizeof(float));
    std::vector<char> host(fbytes + cbytes + (size_t)n_anchors * sizeof(int32_t), 0);
    float* const hf = reinterpret_cast<float*>(host.data());
    float* const hc = reinterpret_cast<float*>(host.data() + fbytes);
    for (size_t f = 0; f < F; ++f)
        for (int r = 0; r < rows; ++r) {
            const double v = frames[f * rows + r];
            if (!std::isfinite(v)) return fail(RSX_ERR_ARG, "non-finite value in frame " + std::to_string(f));
            hf[(size_t)r * F + f] = (float)v;
        }
    for (size_t t = 0; t < T; ++t)
        for (int j = 0; j < NC; ++j) {
            const double v = cmds[t * NC + j];
            if (!std::isfinite(v)) return fail(RSX_ERR_ARG, "non-finite value in the commands of step " + std::to_string(t));
            hc[(size_t)j * T + t] = (float)v;
        }
    std::memcpy(host.data() + fbytes + cbytes, anchors, (size_t)n_anchors * sizeof(int32_t));
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipStreamSynchronize(s));   // a trace loaded before may still be read by a launch in flight
    if (h->d_trace) { HIP_TRY(hipFree(h->d_trace)); h->d_trace = nullptr; h->trace_frames = 0; }
    HIP_TRY(hipMalloc((void**)&h->d_trace, host.size()));
    HIP_TRY(hipMemcpyAsync(h->d_trace, host.data(), host.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    h->trace_frames = n_frames; h->trace_anchors = n_anchors; h->trace_anchor_max = amax;
    h->trace_cmds_off = fbytes; h->trace_anchors_off = fbytes + cbytes;
    return RSX_OK;
}

int rsx_trace_eval(rsx_sim* h, int horizon, float* loss_dev, void* stream) {
    RSX_ENTER(h);
    if (!h->d_phys) return fail(RSX_ERR_STATE, "trace evaluation needs per-env physics (rsx_physics_enable)");
    if (h->P.task != RSX_TASK_NONE) return fail(RSX_ERR_STATE, "trace evaluation runs on a raw handle: a task is attached");
    if (!h->d_trace) return fail(RSX_ERR_STATE, "no trace loaded (rsx_trace_load)");
    if (!loss_dev) return fail(RSX_ERR_ARG, "loss_dev is null");
    if (horizon < 1 || (int64_t)h->trace_anchor_max + horizon > (int64_t)h->trace_frames - 1)
        return fail(RSX_ERR_ARG, "horizon must be >= 1 and every anchor + horizon <= n_frames - 1");
    h->host_state_valid = false;
    const char* const base = reinterpret_cast<const char*>(h->d_trace);
    launch_trace_eval(h->P, h->L, h->NR, h->d_phys, h->d_state, loss_dev, h->d_trace, reinterpret_cast<const float*>(base + h->trace_cmds_off),
                      reinterpret_cast<const int32_t*>(base + h->trace_anchors_off), h->trace_frames, h->trace_anchors, horizon, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return debug_finite(h, (hipStream_t)stream, "rsx_trace_eval");
}

// ---- batched rgb frames (rsx.h: rsx_render_*; field image and kernel: rsx_render.hip) ----
int rsx_render_view_reference(int kind, rsx_render_view* out) {
    if (!out || (kind != RSX_KIND_VSS && kind != RSX_KIND_SSL)) return fail(RSX_ERR_ARG, "out is null or `kind` unknown");
    // Render/raster.py: VSS_VIEW / SSL_VIEW (raster.py is the specification and stays as it is, so the values stand here once more;
    // tests/test_render_batch.py::test_views holds the two, and Render.reference_view, together)
    if (kind == RSX_KIND_VSS) *out = rsx_render_view{1.5, 1.3, 0.1, 0.2, 0.15, 0.7, 0.4, 0.1, 500.0, 0.04, 0.0215, 1};
    else *out = rsx_render_view{9.0, 6.0, 0.35, 1.0, 1.0, 2.0, 1.0, 0.18, 100.0, 0.09, 0.0215, 0};
    return RSX_OK;
}

int rsx_render_size(const rsx_render_view* v, int* width, int* height) {
    if (!width || !height) return fail(RSX_ERR_ARG, "null argument");
    if (const char* msg = render_check_view(v, width, height)) return fail(RSX_ERR_ARG, msg);
    return RSX_OK;
}

int rsx_render_field(const rsx_render_view* v, uint8_t* out_hwc) {
    int W = 0, H = 0;
    if (const char* msg = render_check_view(v, &W, &H)) return fail(RSX_ERR_ARG, msg);
    if (!out_hwc) return fail(RSX_ERR_ARG, "out_hwc is null");
    render_field_host(*v, W, H, out_hwc);
    return RSX_OK;
}

// views a handle may hold (none is freed before rsx_destroy: see rsx_sim::render_views)
#ifndef RSX_RENDER_MAX_VIEWS
#define RSX_RENDER_MAX_VIEWS 16
#endif

int rsx_render_open(rsx_sim* h, const rsx_render_view* v, void* stream) {
    RSX_ENTER(h);
    int W = 0, H = 0;
    if (const char* msg = render_check_view(v, &W, &H)) return fail(RSX_ERR_ARG, msg);
    for (size_t i = 0; i < h->render_views.size(); ++i) {   // a view the handle already holds: selected, nothing else happens
        const rsx_render_view& o = h->render_views[i].view;
        if (o.length == v->length && o.width == v->width && o.margin == v->margin && o.circle == v->circle && o.pen_len == v->pen_len &&
            o.pen_wid == v->pen_wid && o.goal_wid == v->goal_wid && o.goal_dep == v->goal_dep && o.scale == v->scale &&
            o.robot == v->robot && o.ball == v->ball && o.square == v->square) {
            h->render_cur = (int)i;
            return RSX_OK;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s))   // a new view allocates, uploads and synchronises: not inside a capture
        return fail(RSX_ERR_STATE, "rsx_render_open of a new view cannot be captured: open it before the capture");
    if ((int)h->render_views.size() >= RSX_RENDER_MAX_VIEWS)
        return fail(RSX_ERR_STATE, "the handle holds " + std::to_string(RSX_RENDER_MAX_VIEWS) + " render views already (views live until rsx_destroy: captured launches may read them)");
    const size_t HW = (size_t)W * (size_t)H, fb = 3 * HW, tpl = align_up(fb);
    std::vector<uint8_t> host(2 * tpl, 0);
    uint8_t* const hwc = host.data();
    uint8_t* const chw = hwc + tpl;
    render_field_host(*v, W, H, hwc);
    for (size_t p = 0; p < HW; ++p)
        for (size_t c = 0; c < 3; ++c) chw[c * HW + p] = hwc[3 * p + c];
    if (!h->d_render_err) {
        HIP_TRY(hipMalloc((void**)&h->d_render_err, 256));
        HIP_TRY(hipMemsetAsync(h->d_render_err, 0, 256, s));
    }
    rsx_sim::RenderSlot rv{*v, render_geom(*v, W, H), nullptr, tpl};
    HIP_TRY(hipMalloc((void**)&rv.tpl, host.size()));
    hipError_t e = hipMemcpyAsync(rv.tpl, host.data(), host.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipFree(rv.tpl); return fail(RSX_ERR_HIP, std::string("rsx_render_open upload: ") + hipGetErrorString(e)); }
    h->render_views.push_back(rv);
    h->render_cur = (int)h->render_views.size() - 1;
    return RSX_OK;
}

int rsx_render(rsx_sim* h, const int32_t* env_ids_dev, int n, int channels_first, uint8_t* out_dev, void* stream) {
    RSX_ENTER(h);
    if (h->render_cur < 0) return fail(RSX_ERR_STATE, "no render view (rsx_render_open)");
    if (!out_dev || ((uintptr_t)out_dev & 15u)) return fail(RSX_ERR_ARG, "out_dev must be a 16-byte aligned device pointer");
    if (n < 1 || (!env_ids_dev && n > h->P.num_envs)) return fail(RSX_ERR_ARG, "n must be >= 1, and <= num_envs without env_ids_dev");
    const rsx_sim::RenderSlot& rv = h->render_views[(size_t)h->render_cur];
    launch_render(rv.geom, h->d_state, h->P.num_envs, h->P.row_stride, h->P.kind, h->P.n_blue, h->P.n_yellow,
                  rv.tpl + (channels_first ? rv.tpl_bytes : 0), h->d_render_err, env_ids_dev, n, channels_first != 0, out_dev, (hipStream_t)stream);
    HIP_TRY(launch_status());
    return RSX_OK;
}

int rsx_render_errors(rsx_sim* h, int64_t* out, void* stream) {
    RSX_ENTER(h);
    if (!h->d_render_err) return fail(RSX_ERR_STATE, "no render view (rsx_render_open)");
    if (!out) return fail(RSX_ERR_ARG, "out is null");
    return read_and_clear_word(h->d_render_err, out, (hipStream_t)stream);
}

}  // extern "C"
