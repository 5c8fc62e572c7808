// rsx_sim_step_body.inc — the body of sim_step_kernel and sim_step_phys_kernel (rsx_kernels.hpp), included into both.
// Textual inclusion, not a shared device function: the literal kernels then compile to the instructions they had before the
// per-env variant existed (an inlined body function moved registers and instructions around: -2 % on the VSS-v0 headline).
// Expects PHYS (constexpr bool) and `phys` (the physics block, or nullptr) in scope.
    Params P = P_; RSX_UNPACK_HOT(P);
    Buffers bufs = bufs_; bufs.state = hp_state; bufs.cmds = hp_in;   // hp_in: the command buffer
    float* const state_out = hp_aux;   // this kernel's second pointer slot: where the new state goes (== hp_state: in place)
    // fourth pointer slot: a second copy of the new state, or nullptr.  The host-format calls of small batches
    // (rsx_step / rsx_step_state: the robosim-shaped single-env path) hand in pinned host memory here and read their
    // commands from pinned host memory too: one launch + one synchronisation per step instead of copy, launch, copy
    float* const mirror = reinterpret_cast<float*>(hp_flags);
    using K = KC<KIND>;
    constexpr int G = 64 / L;
    constexpr int CD = ModelD<KIND>::cmd_dim;
    __shared__ Shared<L> sh;
#ifdef RSX_TIMING
    if (threadIdx.x == 0) sh.dbg = nullptr;
#endif
    const int lane = threadIdx.x;
    const int b = LaneMap<L>::body(lane), g = LaneMap<L>::env(lane);
    const int e = tile_of_block(hp_per_xcd) * G + g;
    const int N = NR ? NR : P.n_robots;
    const bool live = e < P.num_envs;
    const bool is_robot = live && b < N, is_ball = live && b == N;
    const size_t B = (size_t)P.num_envs;

    Body o; float od, wd, w[4];
    const RawBody raw = load_raw<KIND>(P, bufs.state, e, b, is_robot, is_ball);
    std::conditional_t<PHYS, EnvCoef, LitCoef<KIND>> cf{};
    if constexpr (PHYS) if (live) load_coefs(P, phys, e, cf);
    float q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int rand_tick = hp_n_steps;   // >= 0: commands are drawn here (rsx_step_dev_random), < 0: read from memory
    if (is_robot) {
        if (rand_tick >= 0) {
            const u32x4 u = philox4x32(P.env_id_base + (uint32_t)e, (uint32_t)rand_tick, (uint32_t)b, DOM_RAW, P.key0, P.key1);
            const float a0 = u01(u.x) * 2.0f - 1.0f, a1 = u01(u.y) * 2.0f - 1.0f, a2 = u01(u.z) * 2.0f - 1.0f;
            if (KIND == RSX_KIND_SSL) { q[1] = a0 * 2.5f; q[2] = a1 * 2.5f; q[3] = a2 * 10.0f; }
            else { q[0] = a0 * K::w_max; q[1] = a1 * K::w_max; }
        } else {
            const ix_t B4 = (ix_t)4 * (ix_t)P.row_stride, c0 = (ix_t)(b * CD) * B4 + (ix_t)4 * (ix_t)e;
#pragma unroll
            for (int i = 0; i < CD; ++i) q[i] = at_byte(bufs.cmds, c0 + (ix_t)i * B4);
        }
    }
    interpret_body<KIND>(raw, is_robot, is_ball, o, od, wd, w);
    if (is_robot) robot_targets<KIND>(P, o, q);
    physics<KIND, L, NR>(P, o, b, g, live, sh, cf);
    if (is_robot) {
        od = o.th; wd = o.om * K::rad2deg;
        if (KIND == RSX_KIND_SSL) wheel_speeds<KIND>(P, o, w);
    }
    store_body<KIND>(P, state_out, e, b, is_robot, is_ball, o, od, wd, w, P.n_sub != 0 || state_out != hp_state);
    if (mirror) store_body<KIND>(P, mirror, e, b, is_robot, is_ball, o, od, wd, w, true);

