// rsx_step_pair_tail.inc — the physics wave's end of a paired single step (rsx_pair.hpp), included as text by rsx_task_step_body.inc in
// place of its own wire / observation / reward sequence.  The hand-over to the service wave comes FIRST, right behind physics(): what
// the reward needs of the robots (rsx_step_xr.inc: position, velocity and command of robot 0) and of the ball (position before and
// after the step) does not pass through the wire format — rsx_step_wire.inc rewrites heading, yaw rate and the ball's height only —
// so the service wave computes reward, info and flags while this wave still has the wire format, the observation, the episode end
// and the stores in front of it.  Measured (profiles/LABBOOK.md, "A service wave for the VSS-v0 3v3 single step"): barrier 2 behind
// the observation 9.32 us per step at 4096 envs, here 9.17; the one-wave kernel 9.45.
// Expects in scope: what the three fragments expect, pb (PairBox), lastx / lasty, term, trunc, steps, ended, live, N, L, OD, obs_ts.
#include "rsx_step_xr.inc"
            if (is_ball) pb.ball[g] = make_float4(o.x, o.y, lastx, lasty);
            RSX_STAMP(23);
            // barrier 2 (both waves, unconditionally: MODE_STEP runs this branch of the step on every launch): sh.x0[g] and pb.ball[g] are published
            pair_barrier();
            // the episode end, decided here from the comparisons task_reward and the TimeLimit make on the same floats (no wait for the reward)
            term = is_ball && (o.x > P.half_len || o.x < -P.half_len);
            steps += 1;
            trunc = steps >= P.max_steps;
            const unsigned long long endm = __ballot(is_ball && (term | trunc));
            ended = live && ((endm >> (LaneMap<L>::slot(N, g))) & 1ull) != 0;
#include "rsx_step_wire.inc"
            write_obs<KIND, TASK>(P, bufs.obs + (size_t)e * OD, b, is_robot, is_ball, o.x, o.y, o.vx, o.vy, o.s, o.c, wd, o.ir, obs_ts);
