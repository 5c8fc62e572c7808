// rsx_step_reward.inc — the end of a lane-group task step on the reward lane (the ball's): reward, termination and info terms
// (task_reward, rsx_task.hpp) from the robots' row sh.x0[g], the TimeLimit, the env's episode-end flag, and the info / reward / flag
// stores.  Included as text by rsx_task_step_body.inc and, in the paired form, by the service wave instead (rsx_step_service.inc).
// Expects in scope: KIND, TASK, L, MODE (template parameters), ID, P, bufs, sh (Shared<L>), g, e, N, B, live, is_ball, auxe(ROW), o.x / o.y
// (the ball after the step), lastx / lasty (before it), first_step, steps (incremented), prev_pot, info[10], ep_ret, reward, term, trunc,
// success, against, ended (all written).
            if (is_ball) {
                const float* xr = sh.x0[g];
                task_reward<KIND, TASK>(P, xr, o.x, o.y, lastx, lasty, first_step, prev_pot, info, reward, term, success, against);
                ep_ret = ep_ret + reward;
            }
            steps += 1;
            trunc = steps >= P.max_steps;
            // episode-end flag of the env: held by its ball lane (lane N*G + g), spread with one
            // ballot instead of an LDS round trip
            const unsigned long long endm = __ballot(is_ball && (term | trunc));
            ended = live && ((endm >> (LaneMap<L>::slot(N, g))) & 1ull) != 0;
            if (is_ball) {
                // info is reported as it stands after this step (cleared lazily at the next
                // episode's first step), like the dict the reference returns with `done`
#pragma unroll
                for (int i = 0; i < ID; ++i)
                    if (!(TASK == RSX_TASK_VSS_V0 && (i == 0 || i >= 4)) || term || first_step) auxe(ROW_INFO + i) = info[i];
                auxe(ROW_REWARD) = reward;
                if (MODE == MODE_STEP) { bufs.flags[(ix_t)e] = (uint8_t)term; bufs.flags[(ix_t)P.num_envs + (ix_t)e] = (uint8_t)trunc; }
                else { bufs.flags[e] = (uint8_t)term; bufs.flags[B + e] = (uint8_t)trunc; }
            }
