// rsx_step_xr.inc — what the reward lane (the ball's) needs from the robots' lanes, published in sh.x0[g]; the includer synchronises
// the wave and hands the row to task_reward (rsx_task.hpp) as xr[].  Included as text by rsx_task_step_body.inc and rsx_plan_body.inc.
// Expects in scope: TASK (template parameter), sh (Shared<L>), g, b, is_robot, o (Body, after the wire-format round trip), q[8] (this
// step's command), lastx / lasty (the lane's pre-step position), wheels[4].
            if (is_robot && b == 0) {
                float* xr = sh.x0[g];
                xr[0] = o.x; xr[1] = o.y;
                if (TASK == RSX_TASK_VSS_V0) { xr[2] = o.vx; xr[3] = o.vy; xr[4] = q[0]; xr[5] = q[1]; }
                else if (TASK == RSX_TASK_SSL_STATIC_DEFENDERS || TASK == RSX_TASK_SSL_CONTESTED) {
                    xr[6] = lastx; xr[7] = lasty;
                    xr[8] = wheels[0]; xr[9] = wheels[1]; xr[10] = wheels[2]; xr[11] = wheels[3];
                }
            } else if (is_robot) {
                float* xr = sh.x0[g];
                if (TASK == RSX_TASK_SSL_DRIBBLING) xr[1 + b] = (fabsf(o.vx) > 0.05f || fabsf(o.vy) > 0.05f) ? 1.0f : 0.0f;
                if (TASK == RSX_TASK_SSL_CONTESTED && b == 1) xr[2] = (fabsf(o.vx) > 0.1f || fabsf(o.vy) > 0.1f) ? 1.0f : 0.0f;
                if (TASK == RSX_TASK_SSL_PASS_ENDURANCE && b == 1) { xr[2] = o.x; xr[3] = o.y; xr[4] = o.ir ? 1.0f : 0.0f; }
            }
