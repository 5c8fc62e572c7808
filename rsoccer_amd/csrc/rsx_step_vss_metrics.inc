// rsx_step_vss_metrics.inc — the episode counters of an ended VSS env, added by its reward lane (the ball's) into the workgroup's
// metrics line.  Included as text by rsx_task_step_body.inc and, in the paired form, by the service wave instead (rsx_step_service.inc).
// Expects in scope: mode, bufs, ended, is_ball, info[10], steps (of the episode that ended), term, trunc.
                if (ended && is_ball && mode == 0) {
                    unsigned long long* const ms = metric_slot(bufs);
                    atomicAdd(&ms[1], 1ull);
                    if (info[4] > 0.0f) atomicAdd(&ms[2], 1ull);
                    if (info[5] > 0.0f) atomicAdd(&ms[3], 1ull);
                    atomicAdd(&ms[4], (unsigned long long)__float2ll_rn(vss_episode_return(info) * 1048576.0f));
                    atomicAdd(&ms[5], (unsigned long long)steps);
                    if (trunc && !term) atomicAdd(&ms[6], 1ull);
                }
