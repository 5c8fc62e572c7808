// rsx_hot_args.hpp — the launch ABI of the stepping kernels: the block -> tile map, the preloaded leading kernel arguments
// (RSX_HOT_ARGS) with the kernarg offset of the parameter block behind them, the metrics line of a workgroup and the step
// counter of a launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rsx_params.hpp"

namespace rsx {

// block -> tile map: block b runs on XCD b % 8 (observed dispatch order; used for L2 affinity
// only, never for correctness), so give each XCD one contiguous range of tiles.
__device__ __forceinline__ int tile_of_block(const int per /* gridDim.x / 8: the grid is a multiple of 8 */) {
    return (blockIdx.x & 7) * per + (blockIdx.x >> 3);
}
// The large-batch single-step kernels walk an XCD's tiles in ALTERNATING directions from one launch to the next (the
// launcher negates `per` on odd ticks): the tiles a launch starts with are then the ones the previous launch wrote
// last, i.e. the part of the batch that still sits in the 256 MB memory-side cache (Infinity Cache survives kernel
// boundaries; the L2s do not).  Which wave steps which env changes nothing in the results.
__device__ __forceinline__ int tile_of_block_zigzag(const int per_signed) {
    const int per = per_signed < 0 ? -per_signed : per_signed;
    const int q = blockIdx.x >> 3;
    return (blockIdx.x & 7) * per + (per_signed < 0 ? per - 1 - q : q);
}
// who picks the direction: host-keyed launches get it as the sign of `per` (the launcher negates it on odd ticks);
// device-keyed launches (step_tick below) get a negative `per` for "alternate" and decide from the tick they read
__device__ __forceinline__ int zigzag_per(const bool dev, const uint32_t tick, const int per_signed) {
    if (!dev || per_signed >= 0) return per_signed;
    return (tick & 1u) ? per_signed : -per_signed;
}

// Kernel arguments.  The first twelve dwords are plain pointers / ints so that the command
// processor PRELOADS them into SGPRs (-amdgpu-kernarg-preload-count=12, gfx940+): what the first
// global loads of a wave need (base pointers, row stride, tile map) is then in registers when
// the wave starts, instead of behind a scalar-cache miss on the kernarg segment — with two waves
// per CU nearly every wave would pay that miss on its critical path.  The by-value structs that
// follow carry everything else and are fetched while the state loads are in flight.
#define RSX_HOT_ARGS float* hp_state, float* hp_aux, const float* hp_in, uint8_t* hp_flags, \
                     const int hp_num_envs, const int hp_state_dim, const int hp_per_xcd, const int hp_n_steps
// The two counts of the batch travel in the hot dwords: hp_num_envs = B, and the row pad of the [rows][B] arrays (a multiple of 64
// floats, rsx_api.hip: row_pad_for) in the upper half of hp_state_dim — scalar shifts, no wait for the parameter block.
#define RSX_HOT_DIM(state_dim, row_stride, num_envs) ((int)((unsigned)(state_dim) | ((unsigned)(((row_stride) - (num_envs)) >> 6) << 16)))
#define RSX_UNPACK_HOT(P) do { (P).num_envs = hp_num_envs; (P).state_dim = hp_state_dim & 0xFFFF; \
                               (P).row_stride = hp_num_envs + (int)(((unsigned)hp_state_dim >> 16) << 6); } while (0)
// bytes of the kernarg segment RSX_HOT_ARGS occupies: the by-value Params block starts at the next multiple of its alignment
// (the late parameter fetch of rsx_task_step_body.inc and of rsx_quad_ssl.hpp reads it from there — keep the two in step when a hot argument is added)
constexpr size_t RSX_HOT_ARGS_BYTES = 4 * sizeof(void*) + 4 * sizeof(int);
constexpr size_t RSX_PARAMS_KERNARG_OFFSET = (RSX_HOT_ARGS_BYTES + alignof(Params) - 1) / alignof(Params) * alignof(Params);
namespace hot_args_check {   // the macro and the constant cannot drift apart: a function with exactly these parameters
inline void probe(RSX_HOT_ARGS) {}
template <typename... A> constexpr size_t bytes_of(void (*)(A...)) { return (sizeof(A) + ... + 0); }
static_assert(bytes_of(&probe) == RSX_HOT_ARGS_BYTES, "RSX_HOT_ARGS changed: update RSX_HOT_ARGS_BYTES (kernarg offset of Params)");
}

// Episode counters (metrics[1..6]) are summed with atomics.  Device-scope atomics on ONE cache line
// serialise at about 8 ns each, whatever wave issues them: with a reset in most waves of a 10^6-env launch
// (pass endurance, contested possession) that was the whole step time (605 us instead of 82 us).  The step
// kernels therefore add into one of MSLOTS 64-byte lines, picked by block id, and fold_metrics_kernel
// (rsx_read_metrics / rsx_metrics_fold) adds the lines into metrics[] and clears them.
// (MSLOTS: rsx_params.hpp)
__device__ __forceinline__ unsigned long long* metric_slot(const Buffers& b) {
    return b.mslots + (size_t)(blockIdx.x & (MSLOTS - 1)) * RSX_METRICS;
}

// ---------------------------------------------------------------------------------------------
// The step counter that keys the per-step random draws (and the parity of the placement cache).
//
// Host-keyed (default): the host counts the stepping launches of a handle and passes the count as Params::tick_base.
// That value is baked into the launch — a hipGraph that captured the launch would replay ONE tick for ever.
// Device-keyed (rsx_task_enable_capture; flagged by RSX_TICK_DEV in the n_steps argument, a preloaded SGPR): the
// counter lives in device memory, one 32-bit slot PER WORKGROUP behind the metrics vector.  Workgroup b reads slot b
// and writes slot b + n back; launches of a handle are stream-ordered, nobody else touches that slot, so this needs no
// atomic and cannot race with late-starting workgroups of the same launch (a single shared word could: a workgroup
// that starts after another one finished would read the next launch's tick).  All slots of a handle hold the same
// value between launches (the host re-syncs the slots a smaller grid did not cover, rsx_api_task.hip: tick_resync).
// A counter about to wrap refuses the launch: every workgroup sees the same value, sets the error word and returns
// before touching any state (rsx.h: "checked, never wrapped").
// ---------------------------------------------------------------------------------------------
// (RSX_TICK_DEV, RSX_N_STEPS_MASK, TICK_ERR_WORD, TICK_SLOT_WORD0: rsx_params.hpp)
struct StepTick { uint32_t t; bool ok; };
__device__ __forceinline__ StepTick step_tick(const bool dev, const Params& P, const Buffers& bufs, const uint32_t n) {
    if (!dev) return StepTick{P.tick_base, true};
    uint32_t* const w = reinterpret_cast<uint32_t*>(bufs.metrics);
    uint32_t* const slot = w + TICK_SLOT_WORD0 + blockIdx.x;
    const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)__atomic_load_n(slot, __ATOMIC_RELAXED));
    if (t > 0xFFFFFFFFu - n) {
        if (threadIdx.x == 0) w[TICK_ERR_WORD] = 1u;
        return StepTick{t, false};
    }
    if (threadIdx.x == 0) __atomic_store_n(slot, t + n, __ATOMIC_RELAXED);
    return StepTick{t, true};
}

// development builds (-DRSX_TIMING): cycle stamp i of the workgroup, written by its lane 0 into Buffers::dbg; expands in a kernel
// body that names `lane` and `bufs` (the lane-group task step and the one-lane-per-env SSL step)
#ifdef RSX_TIMING
#define RSX_STAMP(i) do { if (lane == 0) bufs.dbg[(size_t)(i) * gridDim.x + blockIdx.x] = __builtin_readcyclecounter(); } while (0)
#else
#define RSX_STAMP(i) do {} while (0)
#endif

}  // namespace rsx
