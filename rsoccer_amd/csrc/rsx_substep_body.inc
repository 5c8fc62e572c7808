// rsx_substep_body.inc — one sub-step of physics() (rsx_contact.hpp): actuation + integration, the contact sweeps, the walls.
// Text, included into the sub-step loop(s) of physics(): the kernels that take no cut (SubstepCuts) then compile to the instructions
// they had when this was the loop's body (a lambda called from the loops was built: it moved instructions in 244 of the 363 kernels).
// Expects in scope: everything physics() declares ahead of its loop, `sub`, SC (SubstepCuts) and
//   constexpr bool ON_GROUND — no ball of the wave is in flight in this step() (SubstepCuts::grounded): no flight gate, and the
//   ball-height ballot is the constant true.
#ifdef RSX_TIMING_SUB
        ts0 = __builtin_readcyclecounter();
#endif
        // ---- A: actuation + integration ----
        if constexpr (SC::act_select) {   // every lane computes, the robots keep the result (the ball and the idle lanes: their own bits)
            Body t = o;
            actuate_robot<KIND>(P, t, cf);
            t.th = advance_heading(P, t.om, t.th);
            rotate_heading(t.om * P.h, t.c, t.s);
            o.vx = is_robot ? t.vx : o.vx; o.vy = is_robot ? t.vy : o.vy; o.om = is_robot ? t.om : o.om;
            o.th = is_robot ? t.th : o.th; o.c = is_robot ? t.c : o.c; o.s = is_robot ? t.s : o.s;
        } else
        if (is_robot) {   // rsx_body.hpp: the per-body arithmetic is stated once for all kernel layouts
            actuate_robot<KIND>(P, o, cf);
            o.th = advance_heading(P, o.om, o.th);
            rotate_heading(o.om * P.h, o.c, o.s);
        }
        if constexpr (!ON_GROUND)
        if (RSX_RARE_B(KIND, 1, is_ball && (o.z > 0.0f || o.vz > 0.0f))) ball_flight(P, o, K::e_ground, K::vz_min);   // the ball in flight
        // the position advance is the same instruction pair for robots and the ball, outside the role branches
        // (every role branch of a lane group costs a save / branch / restore of the exec mask; idle lanes hold zeros)
        o.x = fma_(o.vx, P.h, o.x);
        o.y = fma_(o.vy, P.h, o.y);
#ifdef RSX_TIMING_SUB
        ts1 = __builtin_readcyclecounter();
#endif

        // ---- B: contacts — one Jacobi sweep over the post-integration snapshot, and a second one
        // over the corrected snapshot for the envs in which some pair overlapped by more than pen2
        // (impacts at speed, jammed piles; resting contacts stay far below).  The second sweep is
        // the same loop body again: the instructions are in the cache (a separate copy never is) ----
        // is the env's ball low enough to be touched?  One ballot of the ball lanes' answer, each lane picks its env's bit
        // (was: the height through LDS — a write, a dependent read and its wait in every sub-step)
        // ON_GROUND: every ball of the wave has z <= 0 < robot_h — the constant true, and what it gates below folds away
        bool ball_low = true;
        if constexpr (!ON_GROUND) {
            const unsigned long long lowm = __ballot(is_ball && o.z < K::robot_h);
            ball_low = ((lowm >> (LaneMap<L>::slot(N, g))) & 1ull) != 0;
        }
        bool active = is_robot || is_ball;   // lanes whose env takes part in the current sweep
        BallOverride bo{false, false, 0.0f, 0.0f, 0.0f};
        for (int sweep = 0;; ++sweep) {
            float2 fo = float2{0.0f, 0.0f};   // VSS: this body's held axes in the snapshot of this sweep (robots; the ball publishes zeros)
            if (SC::exchange_all || active) {   // (exchange_all: every lane, its own slots)
                sh.A[lane] = make_float4(o.x, o.y, o.vx, o.vy);
                sh.W[lane] = o.om;   // yaw rate / spin: read on the contact path only
                sh.X[g * L + b] = o.x; sh.Y[g * L + b] = o.y;
            }
            wave_sync();
            // VSS: the held axes of this snapshot are computed and published BEHIND the exchange — the arithmetic fills the wait for the
            // partners' positions (overlap_keys_packed: `fill`).  Read on the contact path only; no second exchange point is needed: a
            // wave's LDS accesses execute in issue order, and the compiler keeps this write ahead of the later reads of the same array
            // (they may alias).  (A wave_sync() at the head of the contact branch was measured: it pins the body's position in scratch
            // memory, 8.9 -> 12.8 us.)
            auto publish_held = [&]() {
                if constexpr (K::held) { fo = held_axes<KIND>(P, o.x, o.y, is_robot); sh.F[lane] = fo; }
            };
            bool deep = false;   // this lane saw a deep contact
            bool wallp = false;  // ... a touching robot - robot pair with a wall-blocked axis (model v2: wall_shares)

            if (KIND == RSX_KIND_VSS) {
                // every pair is circle-circle; only the constants depend on the pair type
                if (SC::exchange_all || active) {
                    if (NR) {
                        // Overlap test of the whole sweep, exact and with ONE compare per partner class:
                        // d2 is a sum of squares (>= +0), and non-negative floats order like their bit
                        // patterns, so with u = bits(d2) - 1 (d2 == 0, the lane's own slot, wraps to
                        // 0xFFFFFFFF)   0 < d2 < thr   <=>   u < bits(thr) - 1   (unsigned).
                        // The minimum of u over the robot slots is compared once; contacts are rare, so
                        // the common case is ~5 instructions per partner and one untaken branch.
                        constexpr uint32_t T_RR = __builtin_bit_cast(uint32_t, K::rs_rr2) - 1u;
                        constexpr uint32_t T_RB = __builtin_bit_cast(uint32_t, K::rs_rb2) - 1u;
                        uint32_t u[NR + 1];
                        if constexpr (K::held) overlap_keys_packed<NR + 1, L>(sh, g, o.x, o.y, u, publish_held);
                        else overlap_keys_packed<NR + 1, L>(sh, g, o.x, o.y, u);
                        uint32_t um = u[0];
#pragma unroll
                        for (int j = 1; j < NR; ++j) um = min(um, u[j]);
                        // robot lane: robot slots are robot-robot pairs, slot NR the ball; ball lane:
                        // every robot slot is a robot-ball pair, slot NR itself (u = 0xFFFFFFFF)
                        bool any = ((um < (is_ball ? T_RB : T_RR)) & (!is_ball | ball_low)) | ((u[NR] < T_RB) & ball_low);
                        // exchange_all: an idle lane (zeros: a body at the origin) and a lane of an env that sits this sweep out have
                        // tested as well; `active` holds the lane's role and its env's part in the sweep
                        if constexpr (SC::exchange_all) any = any & active;
                        if (RSX_RARE_B(KIND, 2, any)) {
                            // Each lane walks ITS partners in body-index order; lanes with different
                            // partners share an iteration, so a wave pays for the deepest lane (one
                            // response, rarely two) instead of one response block per distinct partner
                            // index present anywhere in the wave.  The wave that finishes last sets a
                            // single-step launch's duration, and it is always one with contacts.
                            // slot j ends at bit j: shifted in from the right, highest slot first — a compare and an add-with-
                            // carry per slot, no bit constant in a register; the ball's height gates its pairs afterwards
                            unsigned todo = 0;
                            const uint32_t thr_r = is_ball ? T_RB : T_RR;   // robot slots: robot-ball pairs for the ball lane
#pragma unroll
                            for (int j = NR; j >= 0; --j) {
                                if (j == NR) asm("v_cmp_gt_u32_e32 vcc, %2, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc" : "+v"(todo) : "v"(u[j]), "s"(T_RB) : "vcc");
                                else asm("v_cmp_gt_u32_e32 vcc, %2, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc" : "+v"(todo) : "v"(u[j]), "v"(thr_r) : "vcc");
                            }
                            if (!ball_low) todo = is_ball ? 0u : (todo & ~(1u << NR));
                            const bool v2w = K::wall_aware && __ballot(is_robot && at_wall<KIND>(P, o.x, o.y)) != 0ull;   // (rsx_body.hpp: contact_response)
                            float avx = 0.0f, avy = 0.0f, apx = 0.0f, apy = 0.0f, aw = 0.0f;
                            const float lever = is_ball ? K::r_ball : K::r_robot;
                            // software-pipelined: the next partner's slot is fetched while the current
                            // response is being computed
                            int jn = __builtin_ctz(todo);
                            todo &= todo - 1;
                            float4 nxt = sh.A[LaneMap<L>::slot(jn, g)];
                            float nxw = sh.W[LaneMap<L>::slot(jn, g)];
                            float2 nxf = sh.F[LaneMap<L>::slot(jn, g)];
                            for (;;) {
                                const int j = jn;
                                const float4 oj = nxt;
                                const float wj = nxw;
                                const float2 fj = nxf;
                                const bool more = todo != 0;
                                if constexpr (SC::prefetch) {
                                    // fetched in every iteration; no partner left: the current one's slot again (three LDS reads
                                    // nobody uses, instead of an exec-mask branch per iteration)
                                    jn = more ? __builtin_ctz(todo) : j;
                                    todo &= todo - 1;
                                    nxt = sh.A[LaneMap<L>::slot(jn, g)];
                                    nxw = sh.W[LaneMap<L>::slot(jn, g)];
                                    nxf = sh.F[LaneMap<L>::slot(jn, g)];
                                } else
                                if (more) {
                                    jn = __builtin_ctz(todo);
                                    todo &= todo - 1;
                                    nxt = sh.A[LaneMap<L>::slot(jn, g)];
                                    nxw = sh.W[LaneMap<L>::slot(jn, g)];
                                    nxf = sh.F[LaneMap<L>::slot(jn, g)];
                                }
                                const float dx = oj.x - o.x, dy = oj.y - o.y;
                                const float d2 = fma_(dx, dx, dy * dy);   // the value the sweep above saw
                                const bool rb = is_ball || j == NR;
                                contact_response<KIND, SC::vn_select>(P, o, oj, d2, rb ? K::rs_rb : K::rs_rr, rb ? cf.ope_rb() : cf.ope_rr(),
                                                       is_ball ? cf.w_rb_b() : (j == NR ? cf.w_rb_r() : K::w_rr),
                                                       is_ball ? cf.kt_rb_b() : (j == NR ? cf.kt_rb_r() : K::kt_rr),
                                                       rb ? cf.mu_rb() : cf.mu_rr(), is_ball ? K::spin_c : 0.0f,
                                                       fma_(wj, j == NR ? K::r_ball : K::r_robot, o.om * lever), K::beta, K::pen2, !rb, v2w,
                                                       avx, avy, apx, apy, aw, deep, wallp, fo, fj);
                                if (!more) break;
                            }
                            // only a body that touched something is updated (the others keep their bits)
                            o.vx = o.vx + avx; o.vy = o.vy + avy;
                            o.x = o.x + apx; o.y = o.y + apy;
                            if (is_ball) o.om = o.om + aw;
                        }
                    } else {
                        publish_held();
                        deep = vss_sweep_loop<KIND, L>(P, o, N, g, is_ball, ball_low, sh, wallp, fo, cf);
                    }
                }
            } else {
                deep = ssl_sweep<KIND, L, NR>(P, o, N, g, lane, is_robot && active, is_ball && active, ball_low, sweep == 0, sh, bo, wallp, cf);
            }
            // second sweep for the envs in which some pair was deep: one ballot, usually no lane; a third and a fourth one for the
            // envs in which the last sweep also saw a wall pair (model v2: piles pressed against a wall)
            const unsigned long long dmask = __ballot(deep);
            if (sweep == 3 || !RSX_RARE_B(KIND, 2, dmask != 0)) break;
            bool again = (L == 64 ? dmask : (dmask & env_lane_mask<L>(g))) != 0;
            if (sweep >= 1) {
                const unsigned long long wmask = __ballot(wallp);
                again = again && (L == 64 ? wmask : (wmask & env_lane_mask<L>(g))) != 0;
            }
            active = active && again;
            if (sweep >= 1 && !__any(active)) break;
            wave_sync();   // every lane has read the first snapshot before it is republished
        }
        if (KIND == RSX_KIND_SSL && bo.ovr) {   // kicker / dribbler: decided in the first sweep, applied after the impulses
            o.vx = bo.ovx; o.vy = bo.ovy; o.om = 0.0f;
            if (bo.okick && bo.ovz > 0.0f) o.vz = bo.ovz;
        }

        // ---- C: walls ----
        // SSL: every lane, no role branch (idle lanes hold zeros: inside every wall) — measured 1-3 % on the SSL tasks;
        // the VSS-v0 3v3 single-step kernel measured 1.5 % slower that way and keeps the branch
        // (SSL also: only when some body of the wave is near a wall — near_walls, rsx_body.hpp: the clamp is the identity elsewhere)
#ifdef RSX_TIMING_SUB
        ts2 = __builtin_readcyclecounter();
#endif
        if (KIND == RSX_KIND_SSL ? __any(near_walls<KIND>(P, o.x, o.y)) : (is_robot || is_ball)) {
            const float vx0 = o.vx, vy0 = o.vy;
            int hit = 0;
            if constexpr (KIND == RSX_KIND_VSS) {
                // the goal-post response shares the rare branch of the ball's wall friction (one exec-mask branch at the end of every
                // sub-step instead of two: a lone wave pays for each one's compare -> scalar -> branch chain)
                const float rb = is_ball ? K::r_ball : K::r_robot, eb = is_ball ? cf.e_wb() : cf.e_wr();
                walls<KIND, true>(P, rb, eb, o.x, o.y, o.vx, o.vy, hit);
                if (RSX_RARE_B(KIND, 2, (is_ball && (hit & 3)) || (hit & 8))) {
                    if (hit & 8) post_response(P, rb, eb, o.x, o.y, o.vx, o.vy, hit);
                    if (is_ball && (hit & 3)) ball_wall_spin<KIND>(hit, vx0, vy0, o.vx, o.vy, o.om, cf.mu_wb(), cf.ope_wb());
                }
            } else {
            walls<KIND>(P, is_ball ? K::r_ball : K::r_robot, is_ball ? cf.e_wb() : cf.e_wr(), o.x, o.y, o.vx, o.vy, hit);
            if (RSX_RARE_B(KIND, 2, is_ball && hit)) ball_wall_spin<KIND>(hit, vx0, vy0, o.vx, o.vy, o.om, cf.mu_wb(), cf.ope_wb());
            }
        }
        wave_sync();  // A / W / Bq / Cq / Dq are rewritten by the next sub-step
#ifdef RSX_TIMING
        if (threadIdx.x == 0 && sh.dbg) sh.dbg[(size_t)(8 + sub) * gridDim.x + blockIdx.x] = __builtin_readcyclecounter();
#endif
#ifdef RSX_TIMING_SUB
        if (sub >= 1) { const unsigned long long t3 = __builtin_readcyclecounter(); tsA += ts1 - ts0; tsB += ts2 - ts1; tsC += t3 - ts2; }
#endif
