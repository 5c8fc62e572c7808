// rsx_replay.hip — prioritised and n-step replay on the device (include/rsx.h: rsx_replay_add_nstep, rsx_replay_set_priorities,
// rsx_replay_sample_prioritized) and the per-entry TD error behind rsx_task_dpg_gradient_w / rsx_task_sac_gradient_w.  A translation
// unit of its own so that the instantiations of every existing kernel stay exactly what they were; the uniform draw stays
// rsx_dpg_update.hip's.
//
// Every kernel here is elementwise, a fold in a FIXED order or a maximum; none adds floating-point numbers through shared addresses.
//   add        one thread per row folds its window (at most 16 steps) and writes the row's scalars; the workgroup then copies its 256
//              rows' obs, actions and successor.  The workgroup that finishes last (an integer ticket) advances head and fill: every
//              workgroup has read the head by then
//   tree       fan-out 64, every level padded to a multiple of 64 floats that stay 0, so a node always reads 64 children: the node is
//              ((c0 + c1) + c2) + ... + c63 in float32 from c0, one thread per node.  A node is always recomputed from its children
//   leaves     written as a maximum over the call's entries: cleared in one launch, raised in the next through an INTEGER maximum of
//              the value's bit pattern (for floats >= 0 the order of the patterns is the order of the values), so duplicates resolve to
//              the largest value whatever the order
//   draw       one thread per entry walks root to leaf with its target in float64 against the float32 running sums of the node's
//              children; the minibatch's largest weight is an integer maximum of bit patterns again, divided out by a second launch
#include <hip/hip_runtime.h>

#include "rsx.h"
#include "rsx_launch.hpp"
#include "rsx_math.hpp"
#include "rsx_units.hpp"

namespace rsx {

namespace {

enum : int { REPLAY_THREADS = 256, FAN = 64, FAN_SHIFT = 6 };
// the prioritised draw's own Philox domain word: counter (entry >> 2, step hi, step lo, 14), keyed by the call's seed
// (rsx_math.hpp: 1, 3 .. 7; rsx_ppo_update.hip: 8; rsx_selfplay.hip: 9; rsx_dpg.hip: 10; rsx_dpg_update.hip: 11; rsx_sac.hip: 12, 13).
// Named PER_*, not DOM_* or SAC_DRAW_*: the scans of the engine's other draws pin the sets they find
constexpr uint32_t PER_DRAW_WORD = 14u;

// where the levels of a tree over `capacity` leaves lie, in floats: level 0 the leaves, level `levels` the root
struct TreeGeom {
    long long off[8];
    long long count[8];   // entries of the level that are not padding
    long long floats;
    int levels;
};
TreeGeom tree_geom(const long long capacity) {
    TreeGeom g{};
    long long n = capacity, off = 0;
    int l = 0;
    for (;;) {
        const long long size = (n + FAN - 1) / FAN * FAN;
        g.off[l] = off;
        g.count[l] = n;
        off += size;
        if (l > 0 && n == 1) break;
        n = size / FAN;
        ++l;
    }
    g.levels = l;
    g.floats = off;
    return g;
}

// ---- add ----
struct AddArgs {
    const float *obs, *actions, *reward, *final_obs, *next_obs;
    const uint8_t *terminated, *truncated;
    float *r_obs, *r_actions, *r_reward, *r_next_obs, *r_discount;
    uint8_t* r_terminated;
    long long *head_dev, *fill_dev;
    int* ticket_dev;
    long long capacity;
    uint32_t T, B, n, OD, AD;
    int n_step;
    float gamma;
};

__global__ __launch_bounds__(REPLAY_THREADS) void replay_add_nstep_kernel(const AddArgs A) {
    __shared__ const float* succ[REPLAY_THREADS];   // each row's successor row
    const uint32_t tid = threadIdx.x, base = blockIdx.x * (uint32_t)REPLAY_THREADS, i = base + tid;
    long long head = A.head_dev[0];
    head = head < 0 ? 0 : head % A.capacity;
    if (i < A.n) {
        const uint32_t t = i / A.B, b = i - t * A.B;
        float R = A.reward[i], g = A.gamma;
        uint32_t m = 1, last = i;   // last: the window's last step (t + m - 1, b)
        bool done = (A.terminated[last] | A.truncated[last]) != 0;
        while (!done && (int)m < A.n_step && t + m < A.T) {
            last += A.B;
            R = R + g * A.reward[last];
            g = g * A.gamma;
            ++m;
            done = (A.terminated[last] | A.truncated[last]) != 0;
        }
        succ[tid] = done ? A.final_obs + (size_t)last * A.OD : t + m < A.T ? A.obs + ((size_t)last + A.B) * A.OD : A.next_obs + (size_t)b * A.OD;
        const size_t at = (size_t)((head + (long long)i) % A.capacity);
        A.r_reward[at] = R;
        A.r_discount[at] = g;
        A.r_terminated[at] = A.terminated[last] != 0 ? 1 : 0;
    }
    __syncthreads();
    const uint32_t rows = A.n - base < (uint32_t)REPLAY_THREADS ? A.n - base : (uint32_t)REPLAY_THREADS;
    for (uint32_t e = tid; e < rows * A.OD; e += REPLAY_THREADS) {
        const uint32_t r = e / A.OD, k = e - r * A.OD;
        const size_t at = (size_t)((head + (long long)(base + r)) % A.capacity) * A.OD + k;
        A.r_obs[at] = A.obs[(size_t)(base + r) * A.OD + k];
        A.r_next_obs[at] = succ[r][k];
    }
    for (uint32_t e = tid; e < rows * A.AD; e += REPLAY_THREADS) {
        const uint32_t r = e / A.AD, k = e - r * A.AD;
        A.r_actions[(size_t)((head + (long long)(base + r)) % A.capacity) * A.AD + k] = A.actions[(size_t)(base + r) * A.AD + k];
    }
    __syncthreads();   // every thread of this workgroup has read the head
    if (tid == 0) {
        __threadfence();
        if (atomicAdd(A.ticket_dev, 1) == (int)gridDim.x - 1) {   // the last workgroup: all others have read the head too
            const long long fill = A.fill_dev[0] + (long long)A.n;
            A.head_dev[0] = (head + (long long)A.n) % A.capacity;
            A.fill_dev[0] = fill > A.capacity ? A.capacity : fill;
            A.ticket_dev[0] = 0;
        }
    }
}

// ---- the tree ----
struct TreeArgs {
    float* tree;
    uint32_t* state;             // RSX_REPLAY_STATE_* words
    const int32_t* rows;         // [m], or nullptr = the m rows behind the write head
    const float* td;             // [m], or nullptr = the running maximum
    const long long* head_dev;
    long long capacity, m;
    long long off_child, off_node;
    int shift;                   // 6 * level of the node launch
    int phase;                   // leaf launch: 0 clear, 1 raise
    float alpha, eps;
};

// entry t's row, or -1 when it is skipped
__device__ __forceinline__ long long tree_row(const TreeArgs& A, const long long t) {
    if (A.rows != nullptr) {
        const long long r = A.rows[t];
        return r >= 0 && r < A.capacity ? r : -1;
    }
    long long head = A.head_dev[0];
    head = head < 0 ? 0 : head % A.capacity;
    return (head + A.capacity - A.m + t) % A.capacity;   // (m <= capacity)
}

__global__ __launch_bounds__(REPLAY_THREADS) void replay_leaf_kernel(const TreeArgs A) {
    const long long t = (long long)blockIdx.x * REPLAY_THREADS + threadIdx.x;
    if (t >= A.m) return;
    const long long row = tree_row(A, t);
    if (row < 0) {
        if (A.phase == 1) atomicAdd(reinterpret_cast<int*>(A.state + RSX_REPLAY_STATE_SKIPPED), 1);
        return;
    }
    if (A.phase == 0) {
        A.tree[row] = 0.0f;
        return;
    }
    float v;
    if (A.td != nullptr) {
        float a = fabsf(A.td[t]);
        a = a == a ? a : 0.0f;
        v = fminf(powf(a + A.eps, A.alpha), 3.4028234663852886e38f);
        atomicMax(A.state + RSX_REPLAY_STATE_MAX, __float_as_uint(v));
    } else {
        v = __uint_as_float(A.state[RSX_REPLAY_STATE_MAX]);
    }
    atomicMax(reinterpret_cast<uint32_t*>(A.tree) + row, __float_as_uint(v));
}

__device__ __forceinline__ float node_sum(const float* __restrict__ c) {
    const float4* const c4 = reinterpret_cast<const float4*>(c);
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < FAN / 4; ++j) {
        const float4 v = c4[j];
        acc = acc + v.x;
        acc = acc + v.y;
        acc = acc + v.z;
        acc = acc + v.w;
    }
    return acc;
}

__global__ __launch_bounds__(REPLAY_THREADS) void replay_node_kernel(const TreeArgs A) {
    const long long t = (long long)blockIdx.x * REPLAY_THREADS + threadIdx.x;
    if (t >= A.m) return;
    const long long row = tree_row(A, t);
    if (row < 0) return;
    // consecutive rows: the first entry of each node recomputes it; rows given: every entry does (the same bits)
    if (A.rows == nullptr && t != 0 && (row & ((1ll << A.shift) - 1)) != 0) return;
    const long long node = row >> A.shift;
    A.tree[A.off_node + node] = node_sum(A.tree + A.off_child + node * FAN);
}

// ---- the draw ----
struct DrawArgs {
    const float* tree;
    uint32_t* state;
    const long long *fill_dev, *step_dev;
    const float* beta_dev;
    int32_t* rows;
    float* weights;
    TreeGeom geom;
    long long fill, step, capacity;
    uint32_t m, k0, k1;
    float beta;
};

__global__ __launch_bounds__(REPLAY_THREADS) void replay_draw_kernel(const DrawArgs A) {
    const uint32_t t = blockIdx.x * (uint32_t)REPLAY_THREADS + threadIdx.x;
    if (t >= A.m) return;
    long long fill = A.fill_dev != nullptr ? A.fill_dev[0] : A.fill;
    fill = fill < 0 ? 0 : fill > A.capacity ? A.capacity : fill;
    const int L = A.geom.levels;
    const float total = A.tree[A.geom.off[L]];
    if (fill == 0 || !(total > 0.0f)) {
        A.rows[t] = -1;
        A.weights[t] = 0.0f;
        return;
    }
    const unsigned long long step = (unsigned long long)(A.step_dev != nullptr ? A.step_dev[0] : A.step);
    const u32x4 w4 = philox4x32(t >> 2, (uint32_t)(step >> 32), (uint32_t)step, PER_DRAW_WORD, A.k0, A.k1);
    const uint32_t k = t & 3u;
    const uint32_t word = k == 0u ? w4.x : k == 1u ? w4.y : k == 2u ? w4.z : w4.w;
    double u = (double)total * (((double)t + (double)word * 2.3283064365386963e-10) / (double)A.m);
    long long node = 0;
#pragma nounroll
    for (int l = L; l >= 1; --l) {
        const float4* const c4 = reinterpret_cast<const float4*>(A.tree + A.geom.off[l - 1] + node * FAN);
        float p = 0.0f, before = 0.0f, last_before = 0.0f;
        int pick = -1, last = 0;
#pragma unroll 4
        for (int j4 = 0; j4 < FAN / 4; ++j4) {
            const float4 v = c4[j4];
            const float c[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float pn = p + c[q];
                if (c[q] > 0.0f) {
                    last = j4 * 4 + q;
                    last_before = p;
                    if (pick < 0 && u < (double)pn) {
                        pick = last;
                        before = p;
                    }
                }
                p = pn;
            }
        }
        if (pick < 0) {   // rounding pushed u past the node's last child: the last child that holds something
            pick = last;
            before = last_before;
        }
        u = u - (double)before;
        node = node * FAN + pick;
        if (node >= A.geom.count[l - 1]) node = A.geom.count[l - 1] - 1;   // (only a tree whose padding was written: stay inside the array)
    }
    const float leaf = A.tree[node];
    const float beta = A.beta_dev != nullptr ? A.beta_dev[0] : A.beta;
    const float w = powf(((float)fill * leaf) / total, -beta);
    A.rows[t] = (int32_t)node;
    A.weights[t] = w;
    atomicMax(A.state + RSX_REPLAY_STATE_WMAX, __float_as_uint(w));
}

__global__ __launch_bounds__(REPLAY_THREADS) void replay_weights_kernel(const DrawArgs A) {
    const uint32_t t = blockIdx.x * (uint32_t)REPLAY_THREADS + threadIdx.x;
    if (t >= A.m) return;
    if (A.rows[t] < 0) return;   // (its weight is 0 already)
    A.weights[t] = A.weights[t] / __uint_as_float(A.state[RSX_REPLAY_STATE_WMAX]);
}

// ---- the TD error ----
__global__ __launch_bounds__(REPLAY_THREADS) void replay_td_error_kernel(const float* q, const float* target, const int C, const long long M,
                                                                         float* td) {
    const long long t = (long long)blockIdx.x * REPLAY_THREADS + threadIdx.x;
    if (t >= M) return;
    const float y = target[t];
    float e = fabsf(q[t] - y);
    if (C == 2) e = fmaxf(e, fabsf(q[M + t] - y));
    td[t] = e;
}

unsigned blocks_of(const long long n) { return (unsigned)((n + REPLAY_THREADS - 1) / REPLAY_THREADS); }

}  // namespace

void replay_tree_geometry(const long long capacity, long long* floats, int* levels, long long* offsets /* [8] or nullptr */) {
    const TreeGeom g = tree_geom(capacity);
    if (floats != nullptr) *floats = g.floats;
    if (levels != nullptr) *levels = g.levels;
    if (offsets != nullptr)
        for (int l = 0; l < 8; ++l) offsets[l] = l <= g.levels ? g.off[l] : -1;
}

void launch_replay_add_nstep(const rsx_replay_batch& b, const rsx_replay_ring& r, const int n_step, const float gamma, hipStream_t s) {
    AddArgs A{};
    A.obs = b.obs; A.actions = b.actions; A.reward = b.reward; A.final_obs = b.final_obs; A.next_obs = b.next_obs;
    A.terminated = b.terminated; A.truncated = b.truncated;
    A.r_obs = r.obs; A.r_actions = r.actions; A.r_reward = r.reward; A.r_next_obs = r.next_obs; A.r_discount = r.discount;
    A.r_terminated = r.terminated;
    A.head_dev = reinterpret_cast<long long*>(r.head_dev); A.fill_dev = reinterpret_cast<long long*>(r.fill_dev);
    A.ticket_dev = r.ticket_dev;
    A.capacity = r.capacity;
    A.T = (uint32_t)b.T; A.B = (uint32_t)b.B; A.n = (uint32_t)((long long)b.T * b.B); A.OD = (uint32_t)r.obs_dim; A.AD = (uint32_t)r.act_dim;
    A.n_step = n_step; A.gamma = gamma;
    rsx_launch(replay_add_nstep_kernel, dim3(blocks_of(A.n)), dim3(REPLAY_THREADS), 0, s, A);
}

void launch_replay_set_priorities(float* tree, void* state, const long long capacity, const int32_t* rows, const float* td_error,
                                  const long long* head_dev, const long long m, const float alpha, const float eps, hipStream_t s) {
    const TreeGeom g = tree_geom(capacity);
    TreeArgs A{};
    A.tree = tree; A.state = static_cast<uint32_t*>(state); A.rows = rows; A.td = td_error; A.head_dev = head_dev;
    A.capacity = capacity; A.m = m; A.alpha = alpha; A.eps = eps;
    const dim3 grid(blocks_of(m)), block(REPLAY_THREADS);
    for (int phase = 0; phase < 2; ++phase) {
        A.phase = phase;
        rsx_launch(replay_leaf_kernel, grid, block, 0, s, A);
    }
    for (int l = 1; l <= g.levels; ++l) {
        A.off_child = g.off[l - 1]; A.off_node = g.off[l]; A.shift = FAN_SHIFT * l;
        rsx_launch(replay_node_kernel, grid, block, 0, s, A);
    }
}

hipError_t launch_replay_sample_prioritized(const float* tree, void* state, const long long capacity, const long long fill,
                                            const long long* fill_dev, int32_t* rows, float* weights, const long long m, const float beta,
                                            const float* beta_dev, const uint64_t seed, const long long step, const long long* step_dev,
                                            hipStream_t s) {
    DrawArgs A{};
    A.tree = tree; A.state = static_cast<uint32_t*>(state); A.fill_dev = fill_dev; A.step_dev = step_dev; A.beta_dev = beta_dev;
    A.rows = rows; A.weights = weights; A.geom = tree_geom(capacity);
    A.fill = fill; A.step = step; A.capacity = capacity;
    A.m = (uint32_t)m; A.k0 = (uint32_t)seed; A.k1 = (uint32_t)(seed >> 32); A.beta = beta;
    // the minibatch's largest weight starts at 0: a memset node of the stream, no launch
    const hipError_t e = hipMemsetAsync(A.state + RSX_REPLAY_STATE_WMAX, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    rsx_launch(replay_draw_kernel, dim3(blocks_of(m)), dim3(REPLAY_THREADS), 0, s, A);
    rsx_launch(replay_weights_kernel, dim3(blocks_of(m)), dim3(REPLAY_THREADS), 0, s, A);
    return hipSuccess;
}

void launch_replay_td_error(const float* q, const float* target, const int n_critics, const long long m, float* td_error, hipStream_t s) {
    rsx_launch(replay_td_error_kernel, dim3(blocks_of(m)), dim3(REPLAY_THREADS), 0, s, q, target, n_critics, m, td_error);
}

}  // namespace rsx
