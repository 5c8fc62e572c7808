// rsx_step_commands.inc — actions -> commands of one lane-group task step: the lane's action (fed, drawn, or its Ornstein-Uhlenbeck
// noise) becomes the robot command q and the body's targets.  Included as text by rsx_task_step_body.inc and rsx_plan_body.inc (a
// shared device function changed the instructions of both: profiles/LABBOOK.md).
// Expects in scope: KIND, TASK (template parameters), T = TC<TASK>, AD = T::act_dim, P, o (Body), b, is_robot, fed (bool: the agent's
// action comes from act[]), act[AD], dr (StepDraw of this step), ou0 / ou1 (the lane's OU state, updated), q[8] (zeroed, filled).
            if (TASK == RSX_TASK_VSS_V0) {
                if (is_robot) {
                    float a0, a1;
                    if (b == 0) {   // the agent: fed action or the step's uniform draw
                        if (fed) { a0 = act[0]; a1 = act[1]; }
                        else { a0 = dr.v[0]; a1 = dr.v[1]; }
                    } else {  // Ornstein-Uhlenbeck noise, Utils/Utils.py:14-21, on the step's two normals
                        ou0 = (ou0 + P.ou_theta_dt * (0.0f - ou0)) + P.ou_sig_sqdt * dr.v[0];
                        ou1 = (ou1 + P.ou_theta_dt * (0.0f - ou1)) + P.ou_sig_sqdt * dr.v[1];
                        a0 = ou0; a1 = ou1;
                    }
                    q[0] = vss_wheel(a0); q[1] = vss_wheel(a1);
                }
            } else if (TASK == RSX_TASK_SSL_SCRIMMAGE) {  // every robot: (v_x, v_y, v_theta, kick), block b of the step
                if (is_robot) {
                    float a[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) a[i] = fed ? act[i] : dr.v[i];
                    q[1] = a[0] * T::max_v; q[2] = a[1] * T::max_v; q[3] = a[2] * 10.0f;
                    q[5] = a[3] > 0.9f ? 5.0f : 0.0f;
                }
            } else {  // the SSL tasks: only blue 0 is driven by the agent
                if (is_robot && b == 0) {
                    float a[5] = {0, 0, 0, 0, 0};
#pragma unroll
                    for (int i = 0; i < AD; ++i) a[i] = fed ? act[i] : dr.v[i];
                    ssl_agent_commands<TASK>(a, o.s, o.c, q);
                }
                if (TASK == RSX_TASK_SSL_PASS_ENDURANCE && is_robot && b == 1) q[7] = 1.0f;  // receiver: dribbler on
            }
            if (is_robot) robot_targets<KIND>(P, o, q);
