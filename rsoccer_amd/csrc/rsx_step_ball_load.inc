// rsx_step_ball_load.inc — the reward lane's (the ball's) loads of a lane-group task step: the info rows and the task scalars.  Included
// as text by rsx_task_step_body.inc and, in the paired form, by the service wave instead (rsx_step_service.inc).
// Expects in scope: TASK (template parameter), ID = TC<TASK>::info_dim, is_ball, auxe(ROW), info[10], prev_pot, ep_ret (zeroed, filled).
    if (is_ball) {
        // VSS-v0: rows 0, 4, 5 (goal counters) are zero except on a terminal step, and the step after it
        // clears them: they are neither read nor — in the common case — written
#pragma unroll
        for (int i = 0; i < ID; ++i)
            if (!(TASK == RSX_TASK_VSS_V0 && (i == 0 || i >= 4))) info[i] = auxe(ROW_INFO + i);
        prev_pot = auxe(ROW_PREV_POT);
        if (TASK != RSX_TASK_VSS_V0) ep_ret = auxe(ROW_EP_RET);   // VSS-v0: derived from the info terms
    }
