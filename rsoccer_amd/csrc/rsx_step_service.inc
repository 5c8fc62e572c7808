// rsx_step_service.inc — the service wave of the paired single step (rsx_pair.hpp), included as text by rsx_task_step_body.inc where
// the lane map is known and before anything is loaded.  Everything here runs on wave 1; the block is the body of the includer's
// `if (wv != 0)` and MUST end in `return` (see there).
// Expects in scope: KIND, TASK, L, NR, MODE (template parameters), mode, ID, P, bufs, sh (Shared<L>), pb (PairBox), lane, b, g, e, N, B,
// live, is_robot, is_ball, env_id, tick0, auxe(ROW).
// Both waves of a workgroup execute both barriers on every path that reaches this point (dead env slots, fed actions, a device-keyed
// tick, an episode end): the barriers below, like the two of the physics wave, stand outside every condition.
    {
        // ---- start of the step: what only the reward needs, the code touch, and the draws in the shadow of those loads ----
        float info[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        float prev_pot = 0.0f, ep_ret = 0.0f;
#include "rsx_step_ball_load.inc"
        int steps = 0;
        if (is_ball) steps = __float_as_int(auxe(ROW_STEPS));
        // the first 8 KB of the kernel's code, a lane per 128-byte line (see CODE_PF in the body: the physics wave of this form leaves it to this one)
        const uint32_t code_touch = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(code_pc) + 128u * (unsigned)lane));
        const bool fed = bufs.actions != nullptr;
        const StepDraw dr = draw_for_step<KIND, TASK>(P, env_id, tick0, b, is_robot, fed);   // same function, same arguments: same bits
        pb.dr[lane] = make_float2(dr.v[0], dr.v[1]);
        // the loads have landed before the physics wave can pass barrier 1, so long before it stores the step counter
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
        asm volatile("" :: "v"(code_touch));
        RSX_STAMP(19);
        pair_barrier();   // barrier 1 (both waves, unconditionally): the draws are published

        // ---- end of the step ----
        pair_barrier();   // barrier 2 (both waves, unconditionally): sh.x0[g] and pb.ball[g] of this step are published
        RSX_STAMP(20);
        float reward = 0.0f; int term = 0, trunc = 0;
        bool success = false, against = false, ended;
        const bool first_step = steps == 0;
        if (first_step) {
#pragma unroll
            for (int i = 0; i < 10; ++i) info[i] = 0.0f;
        }
        const float4 bl = pb.ball[g];
        const struct { float x, y; } o = {bl.x, bl.y};
        const float lastx = bl.z, lasty = bl.w;
#include "rsx_step_reward.inc"
        if (__any(ended)) {
#include "rsx_step_vss_metrics.inc"
        }
        if (is_ball) auxe(ROW_PREV_POT) = prev_pot;
        RSX_STAMP(21);
        return;
    }
