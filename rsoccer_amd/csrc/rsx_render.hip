// rsx_render.hip — batched rgb frames of the current state (include/rsx.h: rsx_render_*), in a translation unit of its own so that
// the instantiations of every existing kernel stay exactly what they were.
//
// Specification: rsoccer_amd/Render/raster.py.  The static field image (FieldRaster._draw_field) is restated on the host in double
// precision, expression for expression (render_field_host), and uploaded once per view as the background template; the moving bodies
// (FieldRaster.draw) are restated per pixel in float32 by rsx_render_frames_kernel.
//
// Shape of the kernel: a pure store stream.  The output ([n][H][W][3] or [n][3][H][W] bytes) is one flat byte stream cut into aligned
// 16-byte chunks; a lane owns CPL chunks, 4 KB apart, so that every store instruction of a wave writes 1 KB of consecutive bytes as
// dwordx4.  A workgroup's span (16 KB) touches one or two frames (more when the frames are tiny): one wave per touched frame puts that
// env's bodies — centre, cos / sin, radius, heading-mark samples, colour — into LDS, keeping only those whose bounding box meets the
// span's pixel rows.  A span that meets none copies the template (the common case once a frame is many workgroups: measured in profiles/render_throughput.md); otherwise a chunk tests the boxes
// of the kept bodies and classifies its pixels (6 in HWC, 16 in a channels-first plane) only when one is near.  H * W * 3 is not a
// multiple of 16 in general, so a chunk can straddle two frames (or two planes): those few, and the last partial chunk of the buffer,
// are assembled byte by byte.  The template of either layout is indexed by the byte's offset inside its frame, so the copy is one
// (unaligned) 16-byte load per chunk from an L2-resident image.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "rsx.h"
#include "rsx_launch.hpp"
#include "rsx_units.hpp"

namespace rsx {

namespace {

constexpr int TPB = 256;               // lanes per workgroup
#ifndef RSX_RENDER_CPL
#define RSX_RENDER_CPL 4
#endif
constexpr int CPL = RSX_RENDER_CPL;    // chunks per lane (1 / 4 / 8 measured: profiles/LABBOOK.md)
constexpr int SPAN = TPB * CPL * 16;   // bytes per workgroup
constexpr int MAX_BODIES = 23;         // 22 robots + the ball
constexpr int SLOTS = 3;               // frames whose bodies are resident at once: two start frames + the one a straddling chunk ends in

// colours of raster.py, packed r | g << 8 | b << 16; code 0 = background (the template's byte)
constexpr uint32_t rgb_of(int r, int g, int b) { return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16); }
constexpr uint32_t C_BLUE = rgb_of(0, 64, 255), C_YELLOW = rgb_of(250, 218, 94), C_BALL = rgb_of(253, 106, 2), C_MARK = rgb_of(25, 25, 25);
enum : int { CODE_BG = 0, CODE_BLUE = 1, CODE_YELLOW = 2, CODE_MARK = 3, CODE_BALL = 4 };
enum : int { SHAPE_SQUARE = 0, SHAPE_DISC = 1 };

struct Entry {
    float px, py, c, sn, r, half;   // centre (pixels), cos / sin of the heading, radius, half side of the bounding box
    float stepx, stepy, xb, yb;     // heading mark: sample k is (k * step + centre), the last one (xb, yb)
    int n;                          // samples of the mark (0: the ball has none)
    int shape_code;                 // shape | code << 8
};
struct Slot {
    int count;
    Entry e[MAX_BODIES];
};

struct RenderArgs {
    const float* state;
    const uint8_t* tpl;       // the template in the layout of the output, FB bytes
    uint32_t* err;            // frames whose env id was out of range
    const int32_t* env_ids;   // [n] or null
    uint8_t* out;
    unsigned long long total; // n * FB
    uint32_t FB, HW;          // bytes per frame, pixels per frame
    int W, H;
    int num_envs, row_stride, n_blue, n_yellow, rs;
    float s, cx, cy, r, rb, inv_w;
    int square;
};

__device__ __forceinline__ uint32_t colour_of(const int code) {
    return code == CODE_BLUE ? C_BLUE : code == CODE_YELLOW ? C_YELLOW : code == CODE_MARK ? C_MARK : C_BALL;
}

// p / W for p < 2^24 * (any W >= 8): one multiply and a correction instead of an integer division
__device__ __forceinline__ void row_col(const RenderArgs& a, const uint32_t p, int& X, int& Y) {
    int q = (int)((float)p * a.inv_w);
    int r = (int)p - q * a.W;
    if (r < 0) { r += a.W; --q; }
    if (r < 0) { r += a.W; --q; }
    if (r >= a.W) { r -= a.W; ++q; }
    if (r >= a.W) { r -= a.W; ++q; }
    X = r; Y = q;
}

// FieldRaster.draw for NP consecutive pixels starting at (X0, Y0) (row-major, wrapping at W): blue robots by id, yellow robots, the
// ball; each robot its body, then its heading mark; the last hit wins.  code[j] stays CODE_BG where nothing is drawn.
template <int NP>
__device__ __forceinline__ bool classify(const RenderArgs& a, const Slot& sl, const int X0, const int Y0, int (&code)[NP]) {
    float xf[NP], yf[NP];
    {
        int x = X0, y = Y0;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            xf[j] = (float)x; yf[j] = (float)y; code[j] = CODE_BG;
            if (++x == a.W) { x = 0; ++y; }
        }
    }
    const bool one_row = yf[NP - 1] == yf[0];
    const float bx0 = one_row ? xf[0] : 0.0f, bx1 = one_row ? xf[NP - 1] : (float)(a.W - 1);
    const float by0 = yf[0], by1 = yf[NP - 1];
    bool any = false;
    const int cnt = sl.count;
    for (int i = 0; i < cnt; ++i) {
        const Entry& e = sl.e[i];
        const float px = e.px, py = e.py, half = e.half;
        if (bx1 < px - half || bx0 > px + half || by1 < py - half || by0 > py + half) continue;
        const float c = e.c, sn = e.sn, r = e.r;
        const int shape = e.shape_code & 0xff, col = e.shape_code >> 8;
        const float rr = r * r;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const float dx = xf[j] - px, dy = yf[j] - py;
            bool hit;
            if (shape == SHAPE_SQUARE) {
                const float u = dx * c + dy * sn, w = (-dx) * sn + dy * c;
                hit = fabsf(u) <= r && fabsf(w) <= r;
            } else {
                hit = dx * dx + dy * dy <= rr;
            }
            code[j] = hit ? col : code[j];
            any |= hit;
        }
        const int n = e.n;
        if (n > 0) {   // _line: n samples of linspace, rounded with ties to even; a sample outside the window meets no pixel
            const float mx0 = fminf(px, e.xb) - 1.0f, mx1 = fmaxf(px, e.xb) + 1.0f;
            const float my0 = fminf(py, e.yb) - 1.0f, my1 = fmaxf(py, e.yb) + 1.0f;
            if (bx1 < mx0 || bx0 > mx1 || by1 < my0 || by0 > my1) continue;
            for (int k = 0; k < n; ++k) {
                const bool last = k == n - 1 && n > 1;
                const float sx = rintf(last ? e.xb : (float)k * e.stepx + px);
                const float sy = rintf(last ? e.yb : (float)k * e.stepy + py);
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    const bool hit = xf[j] == sx && yf[j] == sy;
                    code[j] = hit ? CODE_MARK : code[j];
                    any |= hit;
                }
            }
        }
    }
    return any;
}

// byte `rel` of a frame whose bodies are in `sl` (the chunks that straddle two frames or planes, and the buffer's last partial one)
template <bool CHW>
__device__ __forceinline__ uint32_t render_byte(const RenderArgs& a, const Slot& sl, const uint32_t rel) {
    uint32_t p, ch;
    if (CHW) { ch = rel / a.HW; p = rel - ch * a.HW; }
    else { p = rel / 3u; ch = rel - 3u * p; }
    int X, Y;
    row_col(a, p, X, Y);
    int code[1];
    if (sl.count != 0 && classify<1>(a, sl, X, Y, code)) return (colour_of(code[0]) >> (8u * ch)) & 0xffu;
    return a.tpl[rel];
}

// the 16 bytes of an HWC chunk that starts at channel PH of its first pixel: byte i belongs to pixel (PH + i) / 3
template <int PH>
__device__ __forceinline__ void paint_hwc(uint32_t (&w)[4], const int (&code)[6]) {
    uint32_t rgb[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) rgb[j] = colour_of(code[j]);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int j = (PH + i) / 3, ch = (PH + i) % 3, sh = 8 * (i & 3);
        const uint32_t b = (rgb[j] >> (8 * ch)) & 0xffu;
        w[i >> 2] = code[j] != CODE_BG ? ((w[i >> 2] & ~(0xffu << sh)) | (b << sh)) : w[i >> 2];
    }
}

// wave `wv` (< SLOTS) fills slot `wv` with the bodies of frame f that can touch the span's bytes [lo, hi] of that frame
template <bool CHW>
__device__ __forceinline__ void fill_slot(const RenderArgs& a, Slot& sl, const int lane, const bool valid, const uint32_t f,
                                          const uint32_t lo, const uint32_t hi, const bool owns_first_byte) {
    const int nb = a.n_blue + a.n_yellow;
    int env = 0;
    bool ok = false;
    if (valid) {
        env = a.env_ids ? a.env_ids[f] : (int)f;
        ok = env >= 0 && env < a.num_envs;
        if (!ok && lane == 0 && owns_first_byte) atomicAdd(a.err, 1u);   // once per frame: by the workgroup that writes its first byte
    }
    // pixel rows of the span inside this frame
    int ya = 0, yb = a.H - 1;
    if (valid) {
        uint32_t pa, pb;
        bool rows = true;
        if (CHW) {
            const uint32_t ca = lo / a.HW, cb = hi / a.HW;
            pa = lo - ca * a.HW; pb = hi - cb * a.HW;
            rows = ca == cb;
        } else {
            pa = lo / 3u; pb = hi / 3u;
        }
        if (rows) {
            int x;
            row_col(a, pa, x, ya);
            row_col(a, pb, x, yb);
        }
    }
    const bool body = valid && ok && lane <= nb;
    Entry e{};
    bool keep = false;
    if (body) {
        const bool ball = lane == nb;
        const size_t row = ball ? 0 : (size_t)(5 + a.rs * lane);
        const float* const p = a.state + row * (size_t)a.row_stride + (size_t)env;
        const float x = p[0], y = p[(size_t)a.row_stride];
        e.px = x * a.s + a.cx;
        e.py = y * a.s + a.cy;
        if (ball) {
            e.r = a.rb; e.c = 1.0f; e.sn = 0.0f; e.n = 0;
            e.half = a.rb + 1.5f;
            e.shape_code = SHAPE_DISC | (CODE_BALL << 8);
            e.xb = e.px; e.yb = e.py;
        } else {
            const float th = p[2 * (size_t)a.row_stride] * 0.017453292519943295f;
            e.c = cosf(th); e.sn = sinf(th);
            e.r = a.r;
            e.half = (a.square ? a.r * 1.4143f : a.r) + 1.5f;
            e.shape_code = (a.square ? SHAPE_SQUARE : SHAPE_DISC) | ((lane < a.n_blue ? CODE_BLUE : CODE_YELLOW) << 8);
            e.xb = e.px + e.r * e.c;
            e.yb = e.py + e.r * e.sn;
            const float ddx = e.xb - e.px, ddy = e.yb - e.py;
            const float m = fmaxf(fabsf(ddx), fabsf(ddy));
            // (a non-finite pose draws nothing: NaN fails every comparison below)
            e.n = m < 16384.0f ? (int)m + 1 : 0;
            const float div = (float)(e.n - 1);
            e.stepx = e.n > 1 ? ddx / div : 0.0f;
            e.stepy = e.n > 1 ? ddy / div : 0.0f;
        }
        keep = e.py + e.half >= (float)ya && e.py - e.half <= (float)yb && e.px + e.half >= 0.0f && e.px - e.half <= (float)(a.W - 1);
    }
#ifdef RSX_RENDER_NO_CULL   // experiment: every body of the frame stays in the list (profiles/LABBOOK.md)
    keep = body;
#endif
    const unsigned long long mask = __ballot(keep);
    if (keep) sl.e[__popcll(mask & ((1ull << lane) - 1ull))] = e;   // in drawing order
    if (lane == 0) sl.count = __popcll(mask);
}

template <bool CHW>
__global__ __launch_bounds__(TPB) void rsx_render_frames_kernel(const RenderArgs a) {
    __shared__ Slot sh[SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned long long span0 = (unsigned long long)blockIdx.x * SPAN;
    const unsigned long long span1 = span0 + SPAN < a.total ? span0 + SPAN : a.total;
    const uint32_t f_first = (uint32_t)(span0 / a.FB), f_last = (uint32_t)((span1 - 1) / a.FB);
    for (uint32_t fb = f_first; fb <= f_last; fb += 2) {
        if (fb != f_first) __syncthreads();
        if (wv < SLOTS) {
            const uint32_t f = fb + (uint32_t)wv;
            const bool valid = f <= f_last;
            const unsigned long long f0 = (unsigned long long)f * a.FB, f1 = f0 + a.FB;
            const uint32_t lo = valid ? (uint32_t)((span0 > f0 ? span0 : f0) - f0) : 0u;
            const uint32_t hi = valid ? (uint32_t)((span1 < f1 ? span1 : f1) - 1 - f0) : 0u;
            fill_slot<CHW>(a, sh[wv], lane, valid, f, lo, hi, span0 <= f0 && wv < 2);   // (slot 2 comes round again as a start frame)
        }
        __syncthreads();
        const unsigned long long base = (unsigned long long)fb * a.FB;
        const bool bare = (sh[0].count | sh[1].count | sh[2].count) == 0;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const unsigned long long o = span0 + (unsigned long long)((k * TPB + tid) * 16);
            if (o >= span1 || o < base) continue;
            unsigned long long rel64 = o - base;
            int slot = 0;
            if (rel64 >= a.FB) { rel64 -= a.FB; slot = 1; }
            if (rel64 >= a.FB) continue;   // starts in a frame of the next round
            const uint32_t rel = (uint32_t)rel64;
            uint8_t* const dst = a.out + o;
            // whole chunk inside one frame (HWC) / one plane (CHW)?
            uint32_t p0, ph;
            bool whole;
            if (CHW) { ph = rel / a.HW; p0 = rel - ph * a.HW; whole = p0 + 16u <= a.HW; }
            else { p0 = rel / 3u; ph = rel - 3u * p0; whole = rel + 16u <= a.FB; }
            if (whole) {
                uint32_t w[4];
                __builtin_memcpy(w, a.tpl + rel, 16);
                const Slot& sl = sh[slot];
                if (!bare && sl.count != 0) {
                    int X, Y;
                    row_col(a, p0, X, Y);
                    if (CHW) {
                        int code[16];
                        if (classify<16>(a, sl, X, Y, code)) {
#pragma unroll
                            for (int i = 0; i < 16; ++i) {
                                const int sh8 = 8 * (i & 3);
                                const uint32_t b = (colour_of(code[i]) >> (8u * ph)) & 0xffu;
                                w[i >> 2] = code[i] != CODE_BG ? ((w[i >> 2] & ~(0xffu << sh8)) | (b << sh8)) : w[i >> 2];
                            }
                        }
                    } else {
                        int code[6];
                        if (classify<6>(a, sl, X, Y, code)) {
                            if (ph == 0) paint_hwc<0>(w, code);
                            else if (ph == 1) paint_hwc<1>(w, code);
                            else paint_hwc<2>(w, code);
                        }
                    }
                }
                *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
                // byte by byte: each byte in its own frame (the chunk may end in the next one)
                const bool full = o + 16 <= a.total;
                uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
                for (int i = 0; i < 16; ++i) {
                    if (o + (unsigned long long)i >= a.total) break;
                    uint32_t r = rel + (uint32_t)i;
                    int s2 = slot;
                    if (r >= a.FB) { r -= a.FB; ++s2; }
                    const uint32_t b = render_byte<CHW>(a, sh[s2], r);
                    if (full) {
                        const uint32_t v = b << (8 * (i & 3));
                        w[0] |= (i >> 2) == 0 ? v : 0u; w[1] |= (i >> 2) == 1 ? v : 0u;
                        w[2] |= (i >> 2) == 2 ? v : 0u; w[3] |= (i >> 2) == 3 ? v : 0u;
                    } else {
                        dst[i] = (uint8_t)b;
                    }
                }
                if (full) *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
    }
}

// Python's round(): ties to even (the default rounding mode)
inline long py_round(const double v) { return (long)std::nearbyint(v); }

struct Canvas {
    uint8_t* img;
    int w, h;
    void px(const long x, const long y) const {
        uint8_t* p = img + ((size_t)y * (size_t)w + (size_t)x) * 3;
        p[0] = 255; p[1] = 255; p[2] = 255;
    }
    // FieldRaster._rect
    void rect(const double fx0, const double fy0, const double fw, const double fh) const {
        const long x0 = py_round(fx0), y0 = py_round(fy0), x1 = py_round(fx0 + fw), y1 = py_round(fy0 + fh);
        const long x0c = x0 > 0 ? x0 : 0, x1c = x1 < w - 1 ? x1 : w - 1;
        const long y0c = y0 > 0 ? y0 : 0, y1c = y1 < h - 1 ? y1 : h - 1;
        const long ys[2] = {y0, y1}, xs[2] = {x0, x1};
        for (const long y : ys)
            if (0 <= y && y < h)
                for (long x = x0c; x <= x1c; ++x) px(x, y);
        for (const long x : xs)
            if (0 <= x && x < w)
                for (long y = y0c; y <= y1c; ++y) px(x, y);
    }
    // FieldRaster._line: numpy.linspace (arange * step + start, the last sample the stop itself), rint, clipped onto the window
    void line(const double xa, const double ya, const double xb, const double yb) const {
        const double m = std::fmax(std::fabs(xb - xa), std::fabs(yb - ya));
        const long n = (long)m + 1;
        const double div = (double)(n - 1);
        const double stx = n > 1 ? (xb - xa) / div : 0.0, sty = n > 1 ? (yb - ya) / div : 0.0;
        for (long k = 0; k < n; ++k) {
            const bool last = k == n - 1 && n > 1;
            const double x = last ? xb : (double)k * stx + xa, y = last ? yb : (double)k * sty + ya;
            long xi = (long)std::nearbyint(x), yi = (long)std::nearbyint(y);
            xi = xi < 0 ? 0 : xi > w - 1 ? w - 1 : xi;
            yi = yi < 0 ? 0 : yi > h - 1 ? h - 1 : yi;
            px(xi, yi);
        }
    }
};

}  // namespace

const char* render_check_view(const rsx_render_view* v, int* W, int* H) {
    if (!v) return "view is null";
    const double vals[11] = {v->length, v->width, v->margin, v->circle, v->pen_len, v->pen_wid, v->goal_wid, v->goal_dep, v->scale, v->robot, v->ball};
    for (const double x : vals)
        if (!std::isfinite(x)) return "render view: every value must be finite";
    if (!(v->scale > 0.0)) return "render view: scale (pixels per metre) must be > 0";
    if (v->square != 0 && v->square != 1) return "render view: square must be 0 or 1";
    const double s = v->scale;
    const double w = v->length * s + 2 * (v->margin * s), h = v->width * s + 2 * (v->margin * s);
    if (!(w >= 8.0 && w < 4097.0 && h >= 8.0 && h < 4097.0)) return "render view: the frame must be between 8 and 4096 pixels on each side";
    if (W) *W = (int)w;
    if (H) *H = (int)h;
    return nullptr;
}

void render_field_host(const rsx_render_view& v, const int W, const int H, uint8_t* out_hwc) {
    const double s = v.scale;
    const double cx = (v.length / 2 + v.margin) * s, cy = (v.width / 2 + v.margin) * s;
    for (size_t i = 0; i < (size_t)W * (size_t)H; ++i) { out_hwc[3 * i] = 20; out_hwc[3 * i + 1] = 90; out_hwc[3 * i + 2] = 45; }
    const Canvas cv{out_hwc, W, H};
    const double m = v.margin * s, L = v.length * s, Wd = v.width * s;
    cv.rect(m, m, L, Wd);                                   // touch / goal lines
    cv.line(cx, m, cx, m + Wd);                             // halfway line
    const double cr = v.circle * s;
    for (int y = 0; y < H; ++y)                             // centre circle
        for (int x = 0; x < W; ++x)
            if (std::fabs(std::hypot((double)x - cx, (double)y - cy) - cr) <= 0.6) cv.px(x, y);
    const double pl = v.pen_len * s, pw = v.pen_wid * s;
    cv.rect(m, cy - pw / 2, pl, pw);                        // penalty areas
    cv.rect(m + L - pl, cy - pw / 2, pl, pw);
    const double gd = v.goal_dep * s, gw = v.goal_wid * s;
    cv.rect(m - gd, cy - gw / 2, gd, gw);                   // goals
    cv.rect(m + L, cy - gw / 2, gd, gw);
}

RenderGeom render_geom(const rsx_render_view& v, const int W, const int H) {
    RenderGeom g{};
    const double s = v.scale;
    g.W = W; g.H = H;
    g.s = (float)s;
    g.cx = (float)((v.length / 2 + v.margin) * s);
    g.cy = (float)((v.width / 2 + v.margin) * s);
    g.r = (float)(v.robot * s);
    const double rb = v.ball * s;
    g.rb = (float)(rb > 2.0 ? rb : 2.0);
    g.square = v.square;
    return g;
}

void launch_render(const RenderGeom& g, const float* state, const int num_envs, const int row_stride, const int kind, const int n_blue,
                   const int n_yellow, const uint8_t* tpl, uint32_t* err, const int32_t* env_ids, const int n, const int channels_first,
                   uint8_t* out, hipStream_t s) {
    RenderArgs a{};
    a.state = state; a.tpl = tpl; a.err = err; a.env_ids = env_ids; a.out = out;
    a.HW = (uint32_t)g.W * (uint32_t)g.H;
    a.FB = 3u * a.HW;
    a.total = (unsigned long long)n * a.FB;
    a.W = g.W; a.H = g.H;
    a.num_envs = num_envs; a.row_stride = row_stride; a.n_blue = n_blue; a.n_yellow = n_yellow;
    a.rs = kind == RSX_KIND_VSS ? 6 : 11;
    a.s = g.s; a.cx = g.cx; a.cy = g.cy; a.r = g.r; a.rb = g.rb; a.inv_w = 1.0f / (float)g.W;
    a.square = g.square;
    const unsigned grid = (unsigned)((a.total + SPAN - 1) / SPAN);
    if (channels_first) rsx_launch(rsx_render_frames_kernel<true>, dim3(grid), dim3(TPB), 0, s, a);
    else rsx_launch(rsx_render_frames_kernel<false>, dim3(grid), dim3(TPB), 0, s, a);
}

}  // namespace rsx
