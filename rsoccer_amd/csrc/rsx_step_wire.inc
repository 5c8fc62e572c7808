// rsx_step_wire.inc — the lane's body goes through the wire format after physics(): what the observation reports, what the store
// writes and what a reload (the next launch, or the next step of the same one) starts from are the same floats.  Included as text by
// rsx_task_step_body.inc and rsx_plan_body.inc.
// Expects in scope: KIND (template parameter), K = KC<KIND>, P, o (Body, updated), is_robot, is_ball, od / wd (heading in degrees,
// rate in deg/s: written), wheels[4] (SSL: written).
            if (is_robot) {
                od = o.th; wd = o.om * K::rad2deg;
                if (KIND == RSX_KIND_SSL) wheel_speeds<KIND>(P, o, wheels);
                // omega lives in HBM as deg/s: keep the lane's copy equal to what a reload gives.
                o.om = wd * K::deg2rad;
                // the sub-steps carried (c, s) by small rotations; re-derive them exactly from the
                // stored heading: this is what the observation reports and what a reload (the next
                // launch, or the next step of a multi-step launch) starts from
                sincos_f32(o.th * K::deg2rad, o.s, o.c);
            } else if (is_ball) {
                o.z = (K::r_ball + o.z) - K::r_ball;  // height goes through the wire format too
            }
