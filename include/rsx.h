/*
 * rsx.h — C-ABI of the MI355X-native vectorised rSoccer step engine (librsx_hip.so).
 *
 * This is the drop-in boundary for the hot path of robocin/rSoccer: it takes the place of the
 * third-party `robosim` module (rc-robosim / rSim) that the reference binds in
 * rsoccer_gym/Simulators/rsim.py.  Every entry point cites the reference call site it replaces.
 * Plain pointers and sizes only; no torch / C++ types cross this boundary.
 *
 * Conventions
 *   - every function returns int: 0 = ok, <0 = error (text via rsx_last_error(), thread-local);
 *     no exception crosses the ABI.
 *   - "host" pointers are ordinary CPU memory owned by the caller (the reference wire format:
 *     float64, C-contiguous, rows = blue ids then yellow ids — rsim.py:92-101,129-153).
 *   - "dev" pointers are HIP device memory owned by the handle (valid until rsx_destroy); all
 *     device work is stream-ordered on the hipStream_t passed as `void* stream` (NULL = the
 *     null stream) and never synchronises implicitly, except the host-format calls
 *     (rsx_step / rsx_step_state / rsx_step_wire / rsx_get_state / rsx_get_state_full / rsx_reset / rsx_set_state /
 *     rsx_task_reset_to / rsx_read_metrics), which take or return host arrays and therefore
 *     synchronise that stream; rsx_create and rsx_task_attach synchronise the device once
 *     (their buffers are initialised before any caller stream can touch them).
 *   - no call changes the calling thread's current HIP device: the handle's device is made
 *     current for the duration of the call and the previous one is restored on return.
 *   - a caller compiled against this header checks rsx_abi_version() == RSX_ABI_VERSION BEFORE any other call: rsx_dev_view_get /
 *     rsx_task_view_get fill the caller's struct in the LIBRARY's layout (ABI 5 appended row_stride to both views — a caller built
 *     against an older header would have its stack overwritten), and every entry point assumes this header's argument lists.
 *   - rows of the device arrays are dense (row_stride == num_envs) below 786 432 envs; consumers that index base + f * num_envs on
 *     larger handles either use row_stride or set RSX_ROW_PAD=0 in the environment before rsx_create (dense rows at every batch,
 *     at the measured cost of DESIGN.md 3).
 *   - a handle is not thread-safe; distinct handles are independent.
 *   - there is NO CPU fallback: creation fails (RSX_ERR_NO_DEVICE) without a gfx950 device.
 *
 * Precision: the engine computes in float32.  Stated tolerance against the float64 instantiation
 * of the same model (the reference's boundary type, rsim.py:105), from the same state under the same
 * commands over 1 s (40 steps): |position| <= 1e-4 m, |velocity| <= 1e-3 m/s for every body
 * (tests/test_model_tolerance.py; crowded 22-robot scrums: 1e-2 m / 0.1 m/s, >= 95 % of the envs
 * within the tight bound).  The physics is this project's own 2-D model: rc-robosim's
 * sources are not part of the reference tree, so trajectories are not comparable with rSim's.
 *
 * Units (Entities/Frame.py:8): m, m/s, degrees, degrees/s.  VSS commands are wheel rad/s
 * (vss_gym.py:250-252); SSL commands are robot-local m/s and rad/s or wheel rad/s
 * (rsim.py:137-153).
 */
#ifndef RSX_H
#define RSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSX_ABI_VERSION 6
/* version of the 2-D step model the library implements (docs/PHYSICS.md): 1 = rounds 1-4; 2 = wall-aware contacts —
 * the SSL class since ABI 5 (probed shares, goal posts), the VSS class since ABI 6 (held axes, chord posts).  Stored in checkpoints:
 * a blob saved under another model version is refused (its trajectories would not continue bit-identically). */
#define RSX_PHYSICS_MODEL 2

/* kind: which robosim class the handle stands for (rsim.py:116 robosim.VSS, :169 robosim.SSL) */
#define RSX_KIND_VSS 0
#define RSX_KIND_SSL 1

/* fused task epilogues (obs / reward / done / OU noise / auto-reset computed on device) */
#define RSX_TASK_NONE                 0 /* raw simulator only                                         */
#define RSX_TASK_VSS_V0               1 /* rsoccer_gym/vss/env_vss/vss_gym.py:13  (obs 40, act 2)     */
#define RSX_TASK_SSL_STATIC_DEFENDERS 2 /* ssl/ssl_hw_challenge/static_defenders.py:12 (obs 24, act 5)*/
#define RSX_TASK_SSL_DRIBBLING        3 /* ssl/ssl_hw_challenge/dribbling.py:11         (obs 21, act 4)*/
#define RSX_TASK_SSL_CONTESTED        4 /* ssl/ssl_hw_challenge/contested_possession.py:11 (obs 14, act 5)*/
#define RSX_TASK_SSL_PASS_ENDURANCE   5 /* ssl/ssl_hw_challenge/pass_endurance.py:11    (obs 16, act 3)*/
/* synthetic SSL task in the style of the reference's example env (README.md:78-110) for team sizes no
 * registered id covers (BASELINE.json configs[3]: 11v11 on the division-A field): EVERY robot is
 * commanded — action [N][4] = v_x, v_y (robot-local, x 2.5 m/s), v_theta (x 10 rad/s), kick (5 m/s
 * when > 0.9) — obs = normalised ball and robot positions (2 + 2N), reward +1 / -1 and done on a goal
 * for blue / yellow.  Line-up: jittered 6 x 4 grid over the field (SCRIMMAGE) or packed around the ball,
 * the worst case for the all-pairs contact sweep (SCRIMMAGE_CROWDED). */
#define RSX_TASK_SSL_SCRIMMAGE         6
#define RSX_TASK_SSL_SCRIMMAGE_CROWDED 7

/* error codes */
#define RSX_OK              0
#define RSX_ERR_ARG        -1
#define RSX_ERR_NO_DEVICE  -2
#define RSX_ERR_HIP        -3
#define RSX_ERR_STATE      -4

/* number of entries of get_field_params(), in the order of Entities/Field.py:5-21 */
#define RSX_FIELD_PARAMS 17
/* internal state rows that follow the get_state() rows: ball vertical velocity (m/s), ball spin
 * about the vertical axis (rad/s) */
#define RSX_STATE_EXTRA_ROWS 2
/* metrics vector length (int64 each; see rsx_read_metrics) */
#define RSX_METRICS 8

typedef struct rsx_sim rsx_sim; /* opaque */

/* Device-side views, zero-copy.  SoA: row f of an [F][B] array is the contiguous run of B floats at
 * base + f*row_stride (one float per env).  row_stride >= num_envs: handles of 786 432 envs and more pad their rows
 * (64 KB + 256 B, 256 KB + 256 B from 1 572 864 envs) so that the rows of an env do not all sit at the same address modulo a large power of two (DRAM banks;
 * ABI 5).  Treat the arrays as strided 2-D views (torch: as_strided); a row by itself is dense.  state rows 0..state_dim-1 are exactly the reference's
 * get_state() layout (Entities/Frame.py:20-47 VSS, :55-92 SSL) transposed; rows state_dim and
 * state_dim + 1 hold the ball's vertical velocity and its spin (internal, needed to checkpoint
 * a chipped / spinning ball). */
typedef struct rsx_dev_view {
    int32_t num_envs;    /* B                                                                */
    int32_t n_robots;    /* N = n_blue + n_yellow                                            */
    int32_t state_dim;   /* 5 + 6N (VSS) | 5 + 11N (SSL)                                     */
    int32_t cmd_dim;     /* C: 2 (VSS) | 8 (SSL)  — per robot                                */
    float*  state;       /* [state_dim + 2][B] f32 SoA                                       */
    float*  cmds;        /* [N*C][B] f32 SoA, row = robot*C + col; read by rsx_step_dev      */
    int32_t row_stride;  /* floats from one row of state / cmds to the next (>= num_envs)    */
} rsx_dev_view;

typedef struct rsx_task_view {
    int32_t  task;
    int32_t  obs_dim;       /* 40 | 24 | 21 | 14 | 16 | 2 + 2N                               */
    int32_t  act_dim;       /* 2 | 5 | 4 | 5 | 3 | 4N                                        */
    int32_t  info_dim;      /* 6 | 8 | 1 | 9 | 2 | 2 : cumulative reward-shaping terms, order of the
                               reference's reward_shaping_total dict (dribbling, which has
                               none: its checkpoint counter)                                 */
    int32_t  max_episode_steps;
    float*   obs;           /* [B][obs_dim] f32 row-major (what a policy consumes)           */
    float*   reward;        /* [B] f32                                                       */
    uint8_t* terminated;    /* [B] u8 — task `done` of the step just taken                   */
    uint8_t* truncated;     /* [B] u8 — TimeLimit hit (rsoccer_gym/__init__.py:4,11)         */
    float*   info;          /* [info_dim][B] f32 SoA, values AFTER the step, BEFORE any
                               auto-reset clears them                                        */
    float*   final_obs;     /* [B][obs_dim] f32: terminal observation, written only for envs
                               whose episode ended in this step                              */
    int32_t* steps;         /* [B] i32: steps taken in the current episode                   */
    float*   actions;       /* [B][act_dim] f32: staging buffer callers may fill and pass to
                               rsx_task_step (any device pointer of that shape works)        */
    int64_t* metrics;       /* [RSX_METRICS] i64 device counters, maintained by the step kernels
                               (stream-ordered).  [0] is exact after every launch; the episode
                               counters [1..6] are exact after rsx_metrics_fold /
                               rsx_read_metrics (the kernels add into per-block partial sums) */
    int32_t  row_stride;    /* floats from one row of `info` to the next (>= num_envs; the same value
                               as rsx_dev_view.row_stride)                                   */
} rsx_task_view;

/* ---- diagnostics ---------------------------------------------------------------------- */
int         rsx_abi_version(void);
const char* rsx_last_error(void);
/* number of visible HIP devices (0 when none); never fails */
int         rsx_device_count(void);

/* ---- robosim.VSS / robosim.SSL replacement (batched) ------------------------------------ */

/* ctor — replaces robosim.VSS(...) rsim.py:116-124 and robosim.SSL(...) rsim.py:169-177.
 * field_type: VSS 0 = 3v3, 1 = 5v5; SSL 0 = div-B, 1 = div-A 11v11, 2 = hardware-challenge.
 * num_envs independent copies live on device `device_id`.  Initial poses are the adapter's
 * dummy line-up (rsim.py:20-24): ball at origin, blue at x = -0.2*(i+1), yellow x = +0.2*(i+1). */
int rsx_create(rsx_sim** out, int kind, int field_type, int n_blue, int n_yellow,
               int time_step_ms, int num_envs, int device_id);
/* destructor — replaces `del self.simulator` rsim.py:41 */
int rsx_destroy(rsx_sim* h);

/* get_field_params() — rsim.py:50; out[17] in the order of Entities/Field.py:5-21 */
int rsx_get_field_params(const rsx_sim* h, double out[RSX_FIELD_PARAMS]);

/* reset(ball, blue, yellow) — rsim.py:38,52-75.  Host f64: ball [B][4] = x,y,vx,vy;
 * blue [B][n_blue][3], yellow [B][n_yellow][3] = x,y,theta(deg) (NULL allowed when that team
 * is empty).  env_mask [B] u8 or NULL (= all): only envs with a non-zero mask are teleported.
 * Robot velocities, wheel speeds, infrared and ball height are zeroed. */
int rsx_reset(rsx_sim* h, const double* ball, const double* blue, const double* yellow,
              const uint8_t* env_mask, void* stream);

/* step(cmds) — rsim.py:102 (VSS, [B][N][2]) and rsim.py:155 (SSL, [B][N][8]); host f64.
 * The device-side command buffer (rsx_dev_view.cmds, what rsx_step_dev reads) is UNSPECIFIED after this call: handles of at
 * most 64 envs read the commands straight from pinned host memory and never write them there.  Callers that mix the host-format
 * and the device-resident calls fill view.cmds themselves before rsx_step_dev (results of rsx_step itself do not depend on the
 * path: tests/test_gpu_parity.py::test_host_format_step_with_and_without_zero_copy). */
int rsx_step(rsx_sim* h, const double* cmds, void* stream);

/* get_state() — rsim.py:105,158; out [B][state_dim] host f64 */
int rsx_get_state(rsx_sim* h, double* out, void* stream);

/* step(cmds) followed by get_state() — rsim.py:102,105 / :155,158 are always called as a pair (RSim*.send_commands,
 * RSim*.get_frame): one FFI crossing instead of two.  Handles of at most 64 envs (the robosim-shaped single-env
 * objects) run rsx_step / rsx_step_state without any copy: the kernel reads the commands from, and mirrors the new
 * state into, pinned host memory — one launch and one synchronisation per step. */
int rsx_step_state(rsx_sim* h, const double* cmds, double* state_out, void* stream);

/* The same pair for batches of more than 64 envs WITHOUT any pass of a CPU thread over the data (ABI 6).  Such handles own two pinned
 * host buffers in the reference's wire format — commands [B][N][C] float64 (what rsim.py:92-101 / :129-153 build), state
 * [B][state_dim + RSX_STATE_EXTRA_ROWS] float64 (the get_state() vector of rsim.py:105,158 followed by the two internal rows) — and
 * convert between them and the device's float32 row layout ON THE DEVICE: small kernels read / write the pinned buffers across PCIe
 * around the step kernel; one synchronisation.  rsx_wire_buffers returns the two buffers (valid until rsx_destroy; either pointer
 * argument may be NULL); the caller writes commands into *cmds, calls rsx_step_wire, and reads the new state from *state.
 * rsx_step / rsx_get_state / rsx_step_state on such handles are one memcpy in front of / behind the same path (before ABI 6: a
 * transposing float64 <-> float32 loop on the calling thread plus two staging copies — 192 us per step + state at 4096 envs).
 * Handles of at most 64 envs have no wire buffers (RSX_ERR_STATE): their rsx_step_state is already copy-free. */
int rsx_wire_buffers(rsx_sim* h, double** cmds, double** state);
int rsx_step_wire(rsx_sim* h, void* stream);

/* full-state restore (checkpoint/resume, also used by parity tests): state
 * [B][state_dim + RSX_STATE_EXTRA_ROWS] host f64 = get_state() layout + ball vertical velocity
 * + ball spin. rsx_get_state_full is its inverse.  (The infrared entry of an SSL robot is a flag, Entities/Frame.py:86: give 0 or 1.
 * Any other non-zero value reads as "on"; a step WITH physics rewrites the entry as 0 / 1, a step of a handle with time_step_ms 0
 * leaves what it finds when it steps in place and writes 1 when it writes another buffer, rsx_step_dev_flip.)
 * On a handle with a task attached this overwrites the SIMULATOR state only: observations, episode bookkeeping and the per-episode
 * task scalars (previous ball potential, checkpoint / stalled-step counters) are left as the last step wrote them, so the shaping
 * terms of the next step's reward refer to a frame that no longer exists — and how they do differs between kernel layouts (the
 * one-lane-per-env VSS kernel derives the previous potential from the ball position it finds).  To move envs of a fused run use
 * rsx_task_reset_to (new episode) or rsx_task_checkpoint_load (everything). */
int rsx_set_state(rsx_sim* h, const double* state, void* stream);
int rsx_get_state_full(rsx_sim* h, double* out, void* stream);

/* ---- device-resident path (no host copies) -------------------------------------------- */
int rsx_dev_view_get(rsx_sim* h, rsx_dev_view* out);
/* advance all envs by time_step_ms using the commands currently in view.cmds */
int rsx_step_dev(rsx_sim* h, void* stream);

/* The same step, double-buffered: the new state is written to the handle's second state buffer,
 * which then becomes the current one — the buffer that was current holds the PREVIOUS frame
 * (the reference's `last_frame`, vss_gym_base.py:80) without a copy.  rsx_state_buffers returns both
 * pointers (layout of rsx_dev_view.state); after every flip they trade places. */
int rsx_step_dev_flip(rsx_sim* h, void* stream);
int rsx_state_buffers(rsx_sim* h, float** current, float** other);
/* reset(ball, blue, yellow) of rsim.py:38 from DEVICE arrays (f32, same shapes as rsx_reset),
 * env_mask_dev [B] u8 device or NULL: stream-ordered, no host copy, no synchronisation. */
int rsx_reset_dev(rsx_sim* h, const float* ball_dev, const float* blue_dev, const float* yellow_dev,
                  const uint8_t* env_mask_dev, void* stream);

/* n steps with commands drawn on the device instead of read from view.cmds (benchmark / soak mode of
 * the raw simulator): robot k of env e takes Philox block
 * (e, first_tick + i, k, 4) keyed by `seed` in launch i — VSS: wheel speeds U(-1, 1) x the motor
 * limit; SSL: robot-local velocities U(-1, 1) x (2.5 m/s, 2.5 m/s, 10 rad/s). */
int rsx_step_dev_random(rsx_sim* h, int n, uint64_t seed, uint32_t first_tick, void* stream);

/* ---- fused task epilogues -------------------------------------------------------------- */

/* Attach a task to a handle whose kind / robot counts match it (VSS_V0: VSS, n_blue >= 1;
 * STATIC_DEFENDERS: SSL 1vN; DRIBBLING: SSL 1v4; CONTESTED: SSL 1v1; PASS_ENDURANCE: SSL 2v0;
 * SCRIMMAGE / SCRIMMAGE_CROWDED: SSL, any team sizes).  seed + (env_id_base + local env index) key every random draw,
 * so results do not depend on batch size, batch position or sharding.
 * max_episode_steps <= 0 selects the registry value (1200 / 1000 / 4800 / 1200 / 1200; scrimmage 1200). */
/* Random streams: placement draws are keyed by (seed, global env id, episode, index); the per-step draws
 * (random actions, OU noise) by (seed, global env id, number of fused steps the handle has taken since
 * attach) — a run is reproducible from its seed and its sequence of calls.
 * Limits (both are 32-bit words of the Philox counter, and both are checked, never wrapped):
 *   - env_id_base + num_envs <= 2^32, else RSX_ERR_ARG;
 *   - every [rows][num_envs] float array of a handle stays below 4 GB (rows x num_envs < 2^30: VSS 3v3 ~21 M envs,
 *     SSL 1v6 ~12 M, SSL 11v11 ~4 M), else RSX_ERR_ARG from rsx_create / rsx_task_attach: the kernels address a
 *     row with a 32-bit byte offset;
 *   - a handle takes at most 2^32 - 1 fused steps (rsx_task_step / _step_n / _rollout; about 11 h at 10^5 calls/s);
 *     the call that would exceed it returns RSX_ERR_STATE and changes nothing.  The counter is part of the checkpoint. */
int rsx_task_attach(rsx_sim* h, int task, uint64_t seed, uint64_t env_id_base,
                    int max_episode_steps);
int rsx_task_view_get(rsx_sim* h, rsx_task_view* out);
/* Start over with another seed (ABI 6): afterwards the handle is what a fresh rsx_task_attach(task, seed, same env_id_base, same
 * max_episode_steps) would have left — every random stream re-keyed, step counter 0, episode ids, per-env scalars, metrics and
 * placement cache cleared; the buffers (and every pointer of rsx_task_view) stay where they are; a handle switched by
 * rsx_task_enable_capture stays switched.  The next call must be rsx_task_reset / rsx_task_reset_to.  Stream-ordered; not
 * capturable (it changes host state).  What `reset(seed=...)` of a gymnasium-style vector env maps to (README.md:116-133 seeds
 * through `env.reset(seed=...)`; the reference's own tasks ignore it: SURVEY.md appendix D-1). */
int rsx_task_reseed(rsx_sim* h, uint64_t seed, void* stream);
/* Which tile layout steps this handle's envs (chosen at attach from task and batch size; results are identical in all):
 * "8-lanes-per-env" / "16-..." / "32-..." / "64-...", "32-lanes-per-env-large-batch", "one-lane-per-env",
 * "four-lanes-per-env".  NUL-terminated into out[n] — for profiles and benchmark lines, so that nothing outside the
 * library restates its thresholds.
 * VSS-v0 3v3 handles of at most 4096 envs run the single steps of "8-lanes-per-env" in its PAIRED form: workgroups of two
 * waves, the lane-group wave (loads, commands, physics, observation, episode end and placement, state stores) and a service
 * wave with the same lane map that takes the rest off it: the step's random draws and the touch of the kernel's code at the
 * start; the reward, the info terms, the reward / flag / info stores, the task scalar and the episode counters at the end
 * (RSX_SERVICE_WAVE=0|1 before rsx_task_attach overrides the batch rule).  It is still that layout — same lane map, same grid,
 * same results bit for bit — and this call names it so; rollouts, resets and every other handle run the one-wave kernels. */
int rsx_task_layout(rsx_sim* h, char* out, size_t n);
/* Whether the handle's single steps run in that paired form: *out = 1 or 0 (the plan made by rsx_task_attach /
 * rsx_physics_enable from task, batch and RSX_SERVICE_WAVE).  For tests and profiles: the layout name does not tell. */
int rsx_task_service_wave(rsx_sim* h, int* out);
/* Introspection of the placement cache (handles of STATIC_DEFENDERS 1v6 with at most 16 384 envs: every
 * single-step launch carries helper workgroups that compute each env's NEXT episode's random placement ahead of time —
 * a pure function of seed, global env id and episode — so that the wave that resets an env only copies it; results are
 * those of the inline placement, bit for bit).  out[0] = resets served from the cache, out[1] = placed inline; both -1
 * when the handle has no cache or the counters are off (set RSX_PCACHE_STATS=1 before rsx_task_attach; RSX_NO_PCACHE=1
 * disables the cache).  Synchronises `stream`. */
int rsx_task_placement_cache_stats(rsx_sim* h, int64_t out[2], void* stream);

/* reset(): new random placement for every env (vss_gym.py:194-233, static_defenders.py:214-254),
 * episode counters cleared, obs written. */
int rsx_task_reset(rsx_sim* h, void* stream);
/* reset() onto an explicit placement (same arrays as rsx_reset); obs written.  env_mask (host, num_envs bytes, or NULL = all): only
 * the envs with a non-zero byte are touched.
 * Both resets open a new episode for the envs they touch: observation written, step count 0, info rows and episode sums zero, noise
 * state cleared.  `reward`, `terminated` and `truncated` are outputs of step(): they keep what each env's LAST step wrote — for the
 * envs a mask leaves alone and for the re-placed ones alike — until that env's next step (reset() returns (obs, {}):
 * vss_gym_base.py:92-106). */
int rsx_task_reset_to(rsx_sim* h, const double* ball, const double* blue, const double* yellow,
                      const uint8_t* env_mask, void* stream);

/* The three stepping calls below return RSX_ERR_STATE until rsx_task_reset or
 * rsx_task_reset_to has opened the first episode.
 *
 * step(action): actions_dev [B][act_dim] f32 device memory, or NULL = uniform random actions
 * drawn on device (the "random actions" benchmark configuration).  One kernel launch does
 * action -> commands (+ OU noise for the non-agent robots), physics, observation, reward,
 * done, TimeLimit and same-step auto-reset. */
int rsx_task_step(rsx_sim* h, const float* actions_dev, void* stream);
/* n consecutive random-action steps = n kernel launches issued from C (no per-step FFI cost). */
int rsx_task_step_n(rsx_sim* h, int n, void* stream);
/* n consecutive random-action steps inside ONE launch (state stays in registers between
 * steps; obs / reward / done buffers hold the values of the last step).  Same results as n single steps; the
 * library may issue it that way where that is faster (SSL 11v11 handles of >= 49 152 envs do; the crowded line-up from 196 608). */
int rsx_task_rollout(rsx_sim* h, int n, void* stream);

/* ---- hipGraph / stream capture ------------------------------------------------------------------
 * A trainer steps once per policy action (vss_gym_base.py:72-90; the loop of the reference's README.md:116-133), and
 * with a small policy network that loop is bound by launch overheads: the usual cure is to capture
 * policy(obs) -> step(actions) into one hipGraph (torch.cuda.CUDAGraph) and replay it.
 *
 * By default the handle's step counter — the key of the per-step random draws (random actions, OU noise) and the
 * parity of the placement cache — is a HOST count baked into each launch's arguments.  A captured launch would replay
 * one tick for ever, so the three stepping calls REFUSE to be captured in that mode: RSX_ERR_STATE, nothing enqueued
 * (the capture itself stays valid).
 *
 * rsx_task_enable_capture(h, stream) moves the counter to device memory for the rest of the handle's life (one 32-bit
 * slot per workgroup behind the metrics vector: every workgroup of a stepping launch reads its slot and writes it back
 * advanced, no atomics, no extra launch).  Call it once, OUTSIDE any capture, stream-ordered after the handle's earlier
 * work.  From then on rsx_task_step / _step_n / _rollout (and rsx_task_reset) may be captured and replayed any number
 * of times, mixed freely with eager calls; every replay advances the counter exactly as the eager call would have, so a
 * run is bit-identical whether its steps were issued eagerly, captured, or both.  Costs nothing on handles that never
 * call it; on handles that did, a stepping launch reads one more dword.
 *   - the 2^32 - 1 step limit is then enforced on the device: a launch that would wrap the counter changes nothing and
 *     sets a mark that rsx_task_tick / rsx_read_metrics report as RSX_ERR_STATE;
 *   - rsx_task_checkpoint_save / _load carry the counter in either mode;
 *   - RSX_DEBUG_FINITE=1 (a synchronous scan) makes captured stepping calls fail with RSX_ERR_STATE;
 *   - calls that keep host-side state stay uncapturable and say so: rsx_step_dev_flip (buffer roles).  The raw
 *     rsx_step_dev / rsx_reset_dev launches hold no host state and can be captured as they are;
 *   - HIP's per-thread last-error slot: kernel launches of this library report through their own return values and never read or
 *     clear the slot (a caller's pending error stays the caller's) — with ONE exception: rsx_task_enable_capture clears it.  A
 *     capture that a stepping call refused is usually aborted by the caller's framework, and the aborted capture leaves
 *     `invalid argument` behind for the next capture to trip over (torch.cuda.graph does); the call that prepares the next
 *     attempt is where it is dropped. */
int rsx_task_enable_capture(rsx_sim* h, void* stream);
/* Reads AND clears the calling thread's pending HIP error; returns its hipError_t value (0 = none was pending).  For callers that
 * recover from an aborted capture without going through rsx_task_enable_capture (e.g. hook-written envs on the raw step, whose
 * rsx_step_dev_flip refused to be captured). */
int rsx_drop_pending_hip_error(void);
/* fused steps this handle has taken since attach (the counter above).  Device-keyed handles: synchronises `stream`. */
int rsx_task_tick(rsx_sim* h, uint32_t* out, void* stream);

/* ---- exact lookahead over candidate action sequences (additive extension of ABI 6) ------------------------------------
 * Every random draw of a fused task — the OU noise of the robots the agent does not control included — is keyed by (seed, global env
 * id, episode, step counter), so the future of an env under a given action sequence is a fixed function of its current state.  This
 * call evaluates it: from where each env stands NOW, what would each of n_candidates action sequences earn over the next `horizon`
 * steps?  (The planning primitive of model-predictive control, random shooting / MPPI and tree search.)  One launch, one lane group
 * per (env, candidate) pair, all steps in registers.
 *   actions_dev  [num_envs][n_candidates][horizon][act_dim] f32 device memory, dense; act_dim as rsx_task_view reports it (4 N
 *                for the scrimmage).  Step t of a pair uses the candidate's action t in place of the fed action and the handle's real
 *                draws for step counter + t for everything else.
 *   returns_dev  [num_envs][n_candidates] f32: the discounted return up to the pair's episode end or `horizon`, accumulated in
 *                float32 in this order: ret = ret + disc * reward; disc = disc * gamma (disc starts at 1).
 *   steps_dev    [num_envs][n_candidates] int32: steps simulated; < horizon exactly when the episode ended inside the horizon.
 *   flags_dev    [num_envs][n_candidates] uint8: bit 0 terminated, bit 1 truncated, at the last simulated step.
 *   last_obs_dev [num_envs][n_candidates][obs_dim] f32, or NULL: the observation after the last simulated step; the terminal one
 *                (what rsx_task_step leaves in final_obs) if the pair ended.
 * Exactness: rewards, flags and observations of a pair are bit for bit those of `horizon` rsx_task_step calls with the candidate's
 * actions from the same state (the wire-format round trip between two steps is applied in registers), on every kernel layout
 * and with per-env physics (rsx_physics_enable: each env with its own coefficients).
 * A pair STOPS at its env's first episode end (terminated, or truncated = steps >= max_episode_steps): no placement, no auto-reset
 * and no physics redraw is simulated; the pair's outputs are those of its last simulated step.
 * No side effects: the call reads the state, the per-env task scalars and the step counter and writes nothing but the four output
 * arrays — no state, no observations / rewards / flags / final_obs, no metrics, no step counter, no placement cache:
 * the handle is left exactly as it was, and the next step does what it would have done without the call.
 * Stream-ordered, never synchronises.  Refusals (nothing is enqueued): RSX_ERR_STATE before the first reset, when step counter +
 * horizon would pass the 2^32 - 1 limit, and on a host-keyed handle inside a stream capture (like the stepping calls: the counter
 * is then a launch argument); RSX_ERR_ARG for n_candidates < 1, horizon < 1, a null required pointer, a non-finite gamma, a grid
 * beyond the launch limit (workgroups = tiles of the batch x n_candidates <= 2^31 - 1) or a handle forced to 64 lanes per env.
 * Device-keyed handles (rsx_task_enable_capture): the call reads the counter on the device without advancing it and may be captured
 * and replayed; there the counter limit is checked on the device, and a launch that would pass it simulates nothing: every pair
 * reports 0 steps, return 0, flags 0, and last_obs_dev is not written. */
int rsx_task_lookahead(rsx_sim* h, const float* actions_dev, int n_candidates, int horizon, float gamma,
                       float* returns_dev, int32_t* steps_dev, uint8_t* flags_dev, float* last_obs_dev, void* stream);

/* ---- planning with candidates drawn on the device (additive extension of ABI 6) ---------------------------------------------
 * The candidates of random shooting / CEM / MPPI carry no information that has to live in memory: each is a plan mean plus noise.
 * Here the noise is a counter-based draw like every other random number of the engine, recomputed where it is needed, so the caller
 * exchanges only [num_envs][H][act_dim] plans and [num_envs][K] returns with the engine; one planning iteration is two launches
 * (rsx_task_lookahead_sampled, rsx_plan_update).
 *
 * The sampler — ONE definition for the three calls below.  For global env id g = env_id_base + e, candidate k in [0, K), step t in
 * [0, H) and action component i in [0, act_dim) (act_dim as rsx_task_view reports it; scrimmage: 4 N, robot b owns 4 b .. 4 b + 3):
 *     a[e][k][t][i] = clamp(mean[e][t][i] + sigma * eps(g, k, tick, t / hold, i), -1, 1)      for k >= 1
 *     a[e][0][t][i] = clamp(mean[e][t][i], -1, 1)                                              (candidate 0: the unperturbed plan)
 *   mean   [num_envs][H][act_dim] f32 device memory, dense; NULL = all zeros.
 *   hold   >= 1: one drawn perturbation serves `hold` consecutive steps (segment s = t / hold, integer; H need not be a multiple).
 *   tick   the handle's step counter as rsx_task_lookahead reads it (host-keyed handles: the host's count; device-keyed handles: read
 *          on the device), never advanced: calls between the same two steps see the same candidates, after a step fresh ones, and a
 *          captured call draws new noise on every replay.
 *   eps    blocks of four standard normals.  Block q = s * ceil(act_dim / 4) + (i >> 2) is
 *              philox4x32-7(counter = (g, k, tick, 6 | q << 8), key = (sample_seed lo, sample_seed hi))
 *          whose words (x, y) and (z, w) each go through the Box-Muller of the engine's OU noise in float32: u1 = ((w0 >> 8) + 1) *
 *          2^-24, ang = ((w1 >> 8) * 2^-24 - 0.5) * 2 pi, rad = sqrt(-2 ln u1) -> (rad cos ang, rad sin ang).  The four normals are
 *          those of the first pair, then of the second; component i takes normal i & 3.  q must fit in 24 bits.
 *   sample_seed  independent of the handle's seed: several refinement passes at one tick use different noise by passing different seeds. */
typedef struct rsx_plan_sampler {
    uint64_t sample_seed;
    float sigma;    /* >= 0, finite */
    int32_t hold;   /* >= 1 */
} rsx_plan_sampler;

/* rsx_task_lookahead with each candidate's actions produced by the sampler instead of loaded.  Outputs (returns_dev, steps_dev,
 * flags_dev, last_obs_dev or NULL) and guarantees are rsx_task_lookahead's: exact (bit for bit rsx_task_lookahead of the actions
 * rsx_plan_candidates writes, hence `horizon` rsx_task_step calls with them), a pair stops at its env's first episode end, no side
 * effects (the handle is left exactly as it was), stream-ordered, never synchronises; on a device-keyed handle a launch that would pass
 * the counter limit simulates nothing.  Refusals (nothing is enqueued): those of rsx_task_lookahead, and RSX_ERR_ARG for a null
 * `s`, hold < 1, a negative or non-finite sigma, or ceil(horizon / hold) * ceil(act_dim / 4) > 2^24. */
int rsx_task_lookahead_sampled(rsx_sim* h, const float* mean_dev, const rsx_plan_sampler* s, int n_candidates, int horizon, float gamma,
                               float* returns_dev, int32_t* steps_dev, uint8_t* flags_dev, float* last_obs_dev, void* stream);
/* Writes the very floats rsx_task_lookahead_sampled uses, for the same handle state: for tests, debugging and callers who want a
 * sequence's neighbours.  Same refusals (the checks on the lookahead's own outputs and lane width apart); the handle is not touched. */
int rsx_plan_candidates(rsx_sim* h, const float* mean_dev, const rsx_plan_sampler* s, int n_candidates, int horizon,
                        float* actions_out_dev /* [num_envs][K][H][act_dim] */, void* stream);
/* Folds returns_dev [num_envs][n_candidates] (finite) into a new plan without reading a candidate tensor: the candidates are drawn again.
 *   best_dev      [num_envs] int32, or NULL: the index of the largest return, the lowest such index on ties.
 *   temperature   == 0: new_mean[e] = a[e][best[e]], copied bit for bit (random shooting).
 *                 >  0: w_k = exp((R_k - R_best) / temperature), new_mean[e][t][i] = sum_k w_k a[e][k][t][i] / sum_k w_k (MPPI).
 *   new_mean_dev  [num_envs][H][act_dim] f32.  It may be mean_dev itself (in place: every element is read and written by the same
 *                 thread); any other overlap of the two arrays is refused.
 * The arithmetic is fixed, so the same call gives the same bits: weights in float32, sums over k = 0, 1, ..., K - 1 accumulated in
 * float64 by one thread per (env, step, block of four components), one division, one rounding; no atomics.
 * Reads the step counter the way the other two calls do, so lookahead_sampled -> update with no step in between agree on the
 * candidates, on host-keyed and device-keyed handles, eager or replayed.  Refusals as rsx_plan_candidates, and RSX_ERR_ARG for a
 * negative or non-finite temperature or a null returns_dev / new_mean_dev. */
int rsx_plan_update(rsx_sim* h, const float* mean_dev, const rsx_plan_sampler* s, int n_candidates, int horizon,
                    const float* returns_dev, float temperature, float* new_mean_dev, int32_t* best_dev, void* stream);

/* ---- closed-loop lookahead: MLP policies inside the lookahead launch (additive extension of ABI 6) -----------------------------
 * rsx_task_lookahead with a policy as the action source: pair (e, k) is env e under policy k, and the action of a simulated step is
 * the policy's answer to the observation the pair itself just produced:  a_t = pi_k(obs_t);  obs_{t+1}, r_t = step(a_t).  With
 * horizon = max_episode_steps straight after rsx_task_reset one launch scores whole episodes of K parameter vectors from the same B
 * start states against the same future draws (evolution strategies, CEM over parameters, paired evaluation of checkpoints).
 *
 * The policy is a small MLP, the same for all envs: */
#define RSX_ACT_RELU 0   /* max(x, 0) */
#define RSX_ACT_TANH 1   /* one float32 tanh (fixed operation order, |result| <= 1, absolute error about 1e-7) */
#define RSX_ACT_CLIP 2   /* clamp to [-1, 1] */
typedef struct rsx_policy_mlp {
    int32_t n_hidden_layers;  /* 1 or 2 */
    int32_t hidden;           /* 32 or 64 units per hidden layer */
    int32_t hidden_act;       /* RSX_ACT_RELU | RSX_ACT_TANH */
    int32_t out_act;          /* RSX_ACT_CLIP (clamp to [-1, 1]) | RSX_ACT_TANH */
} rsx_policy_mlp;
/*   params_dev   [n_policies][P] f32 device memory, dense.  One policy is laid out like torch.nn.Linear.weight and .bias, in this
 *                order: W1 [hidden][obs_dim] row-major (the weights of unit j contiguous), b1 [hidden]; with two hidden layers W2
 *                [hidden][hidden], b2 [hidden]; Wo [act_dim][hidden], bo [act_dim].  P is the sum of these sizes
 *                (rsx_policy_num_params; obs_dim and act_dim as rsx_task_view reports them).  Non-finite parameters are not checked,
 *                as fed actions are not.
 *   arithmetic   unit j of a layer: acc = bias[j]; for i = 0 .. n_in - 1 ascending: acc = fmaf(W[j][i], x[i], acc), in float32, then
 *                the activation.  One lane computes a whole unit and nothing is reduced across lanes, so the bits do not depend on the
 *                kernel layout or on per-env physics.  No stochastic head in this call (parameter noise is the caller's);
 *                rsx_task_collect_policy below has one.
 *   what it sees at step 0 of a pair the env's row of the handle's obs buffer — what the caller's own policy would have seen after the
 *                last rsx_task_step / reset / reset_to / transfer (NOT a recomputation from the state: SSLDribbling's observation
 *                carries a task scalar that lags the state by design); at step t >= 1 the observation simulated step t - 1 produced,
 *                the floats rsx_task_step would have written to obs.
 *   returns_dev, steps_dev, flags_dev, last_obs_dev   exactly rsx_task_lookahead's ([num_envs][n_policies] ...), the same float32
 *                return recurrence; a pair stops at its env's first episode end.
 *   actions_out_dev  [num_envs][n_policies][horizon][act_dim] f32, or NULL: the action the policy produced at each simulated step.
 *   obs_out_dev      [num_envs][n_policies][horizon][obs_dim] f32, or NULL: the observation that action was computed from.
 *                Entries of steps a pair did not simulate are not written.
 * Exactness: feeding actions_out_dev to rsx_task_lookahead from the same handle state gives the same returns, steps, flags and
 * last_obs bit for bit — hence also `horizon` rsx_task_step calls with those actions — on every lane width (8, 16, 32), with and without
 * per-env physics, on host-keyed and device-keyed handles.
 * No side effects: the call reads the state, the scalar arena, the obs buffer, the step counter and params_dev and writes only its
 * outputs; the handle is left exactly as it was.  Stream-ordered, never synchronises, capturable under rsx_task_lookahead's conditions
 * (a launch at the counter limit of a device-keyed handle simulates nothing).
 * Refusals (nothing is enqueued): all of rsx_task_lookahead's, and RSX_ERR_ARG for a null p or params_dev, n_hidden_layers, hidden or
 * an activation outside the listed values, a policy whose weights do not fit a workgroup's 64 KB of LDS (2 x 64 units fit every
 * observation of at most 100 floats), and the scrimmage task: it commands every robot (act_dim = 4 N), which one agent's policy per env
 * does not drive — a different feature. */
int rsx_policy_num_params(const rsx_sim* h, const rsx_policy_mlp* p, int64_t* out);
int rsx_task_lookahead_policy(rsx_sim* h, const rsx_policy_mlp* p, const float* params_dev, int n_policies, int horizon, float gamma,
                              float* returns_dev, int32_t* steps_dev, uint8_t* flags_dev, float* last_obs_dev,
                              float* actions_out_dev, float* obs_out_dev, void* stream);

/* ---- on-policy collection: the envs advanced under an MLP policy inside one launch (additive extension of ABI 6) ------------------
 * What an on-policy trainer (PPO, A2C) calls between two updates: advance the REAL envs n_steps steps under the current policy, keep
 * going through episode ends, and hand back the [T][B] batch (T = n_steps, B = num_envs) of observations, actions, rewards and done
 * flags.  One launch: rsx_task_rollout's multi-step trip with auto-reset, rsx_task_lookahead_policy's policy between the steps.
 *   p, params_dev    the policy of rsx_task_lookahead_policy (rsx_policy_mlp, the same parameter layout and arithmetic), ONE parameter
 *                    vector [P].
 *   step 0           sees the env's row of the handle's obs buffer, as rsx_task_lookahead_policy does; step t >= 1 the observation
 *                    step t - 1 wrote — for an env whose episode ended at t - 1, the first observation of its next episode.
 *   the head         mean_i = the output layer's accumulator (bias and ascending fmaf, before out_act);
 *                    sample_i = mean_i + sigma_i * eps_i in float32, a multiplication and an addition (two roundings); with
 *                    sigma_dev == NULL, sample_i = mean_i (deterministic); action_i = out_act(sample_i).
 *   sigma_dev        [act_dim] f32 device memory, >= 0 and finite, or NULL.  Device memory is NOT checked (as params_dev and fed
 *                    actions are not): a negative or non-finite sigma is the caller's to refuse before it is uploaded.
 *   eps              a standard normal from the sampler's recipe above (rsx_plan_sampler: Philox 4x32-7, the same Box-Muller), with
 *                    domain word 7:  block (i >> 2) is philox4x32-7(counter = (g, 0, tick of that step, 7 | (i >> 2) << 8), key =
 *                    (noise_seed lo, noise_seed hi)), g the global env id; component i takes normal i & 3.  Keyed by global env id
 *                    and step counter like every other draw: independent of the batch split, and a captured call draws fresh noise
 *                    on every replay.  Pass another noise_seed per training run; the handle's seed is not involved. */
typedef struct rsx_collect_out {
    float*   obs;        /* [T][B][obs_dim]  the observation each action answered            required */
    float*   actions;    /* [T][B][act_dim]  the action fed to the step                      required */
    float*   rewards;    /* [T][B]                                                           required */
    uint8_t* flags;      /* [T][B] bit 0 terminated, bit 1 truncated (as rsx_task_lookahead) required */
    float*   final_obs;  /* [T][B][obs_dim] or NULL: written ONLY in rows whose flags != 0 (the terminal observation) */
    float*   mean;       /* [T][B][act_dim] or NULL: the output layer before noise and before out_act */
    float*   sample;     /* [T][B][act_dim] or NULL: mean + sigma * eps, before out_act */
} rsx_collect_out;
/* Commit: the call advances the handle exactly as n_steps calls of rsx_task_step(h, out->actions[t]) would.  Bit-identical to that
 * sequence of calls are the state, every per-env task scalar (steps, episode, OU noise, info terms, task scalar, episode return),
 * obs / reward / terminated / truncated / final_obs (the last step's values, final_obs per env that of its latest episode end), the
 * metrics, the step counter (advanced by n_steps) and, with per-env physics, the physics block (redrawn at every episode start inside
 * the launch): a checkpoint taken afterwards is byte for byte the checkpoint of the stepped twin.  Episode ends are handled inside the
 * launch as in rsx_task_rollout (the placement cache of small SSLStaticDefenders handles is left as that call leaves it: entries are
 * tagged and stay valid).  The results do not depend on the lane width (8, 16, 32) or on the physics form, and the call serves every
 * handle rsx_task_lookahead_policy serves, those whose single steps run one lane per env included (the arrays are the same).
 * Step counter: host-keyed handles check the 2^32 - 1 limit here and refuse to be captured (RSX_ERR_STATE, like the stepping calls);
 * device-keyed handles (rsx_task_enable_capture) read, check and advance it on the device — a launch that would wrap it changes
 * nothing, writes none of the outputs and sets the mark rsx_task_tick / rsx_read_metrics report — and the call may be captured and
 * replayed.  Stream-ordered, never synchronises (RSX_DEBUG_FINITE=1 scans afterwards as for the other stepping calls).
 * Refusals (nothing is enqueued): RSX_ERR_STATE before the first reset, at the counter limit and for a capture of a host-keyed handle;
 * RSX_ERR_ARG for everything rsx_task_lookahead_policy refuses of a policy and a handle (null p or params_dev, a spec outside the
 * listed values, an LDS image over 64 KB, the scrimmage task, 64 lanes per env), n_steps < 1 or > 2^30 - 1, a null `out` or a null
 * required array. */
int rsx_task_collect_policy(rsx_sim* h, const rsx_policy_mlp* p, const float* params_dev /* [P], one policy */,
                            const float* sigma_dev /* [act_dim] >= 0, or NULL = deterministic */, uint64_t noise_seed,
                            int n_steps, const rsx_collect_out* out, void* stream);

/* ---- collection under a state-dependent, tanh-squashed Gaussian head (additive extension of ABI 6) ---------------------------------
 * rsx_task_collect_policy with another action source: the actor of soft actor-critic, whose output layer gives a mean AND a log-std per
 * state and whose sample is squashed by tanh.  Everything else is that call's: the multi-step trip with same-step auto-reset inside
 * one launch, rsx_collect_out (mean = mu, sample = u, actions = a), the step counter on host-keyed and device-keyed handles, capture on
 * device-keyed handles, and the commit guarantee — the handle ends up bit for bit where n_steps calls of rsx_task_step(h,
 * out->actions[t]) leave it, checkpoint, metrics and the per-env physics block included.
 *   p, params_dev    an rsx_policy_mlp with out_act = RSX_ACT_NONE whose OUTPUT LAYER IS 2 * act_dim UNITS WIDE: rows [0, AD) of Wo / bo
 *                    are the mean mu, rows [AD, 2 AD) the raw log-std.  P = rsx_policy_num_params of the shape + act_dim * hidden + act_dim.
 *                    Hidden layers and arithmetic are rsx_policy_mlp's (bias, ascending fmaf, float32): mu_k and raw_k are output
 *                    units k and AD + k as every other evaluation of these parameters computes them, bit for bit.
 *   the head         all float32, each operation rounded (the unit is built with -ffp-contract=off):
 *                      ls_k    = clamp(raw_k, log_std_min, log_std_max)       gradient as torch.clamp: 1 inside, bounds included, else 0
 *                      sigma_k = exp(ls_k)
 *                      u_k     = mu_k + sigma_k * eps_k                       a multiplication and an addition (two roundings)
 *                      a_k     = tanh(u_k)                                    RSX_ACT_TANH's tanh, unchanged
 *                      logp    = sum_k [ -0.5 eps_k^2 - ls_k - 0.5 ln(2 pi) - 2 (ln 2 - u_k - softplus(-2 u_k)) ]
 *                      softplus(z) = max(z, 0) + log1p(exp(-|z|))
 *                    The tanh correction is in the stable form and not log(1 - a^2 + 1e-6): the tanh has an absolute error near 1e-7,
 *                    so 1 - a^2 is useless near saturation.  With the reparameterisation (eps a constant), d logp / d u_k = 2 a_k.
 *                    This call computes ls, sigma, u and a; logp is the caller's, from mean, log_std and sample (eps_k = (u_k - mu_k) /
 *                    sigma_k), in whatever precision it wants.
 *   exp              exp(x) = e + e * (r * ln 2) with t = fl(x * c), c = fl(log2 e), r = fmaf(x, log2 e - c, fmaf(x, c, -t)), e =
 *                    exp2(t) on the hardware (1 ulp): the exponent's rounding error is carried in r, so the relative error does not
 *                    grow with |x|.  Relative error below 5e-7 for |x| <= 80.
 *   cfg->deterministic != 0   u_k = mu_k, no draw; log_std_out is still written.
 *   eps              the collector's own draw, unchanged: domain word 7, counter (global env id, 0, tick of that step, 7 | (k >> 2) << 8),
 *                    key noise_seed, component k takes normal k & 3.  For one noise_seed the recorded sample differs from
 *                    rsx_task_collect_policy's only by the state-dependent sigma.
 *   log_std_out      [T][B][act_dim] f32 or NULL: ls, the clamped log-std.
 * Handles: every handle rsx_task_collect_policy serves — lane widths 8 / 16 / 32, handles whose single steps run one lane per env, with
 * and without per-env physics.  Lane b < act_dim of an env computes output units b and act_dim + b, so act_dim <= lanes per env stays
 * the only lane condition.
 * LDS: the policy image with the wider output layer (pitch (2 act_dim) | 1, a bias slot of 16 floats) plus the step's own block.  VSS-v0
 * 3v3 with 2 x 64 units: 36 928 B of image (rsx_task_collect_policy: 36 384 B) + 6 272 B = 43 200 B, three workgroups per CU, as there.
 * Refusals (nothing is enqueued): all of rsx_task_collect_policy's, and RSX_ERR_ARG for a null cfg, out_act != RSX_ACT_NONE, log-std
 * bounds that are not finite or not log_std_min < log_std_max, and reserved != 0. */
typedef struct rsx_collect_gaussian_cfg {
    uint64_t noise_seed;
    float    log_std_min, log_std_max;
    int32_t  deterministic;   /* != 0: a = tanh(mu), no draw */
    int32_t  reserved;        /* 0 */
} rsx_collect_gaussian_cfg;
int rsx_task_collect_gaussian(rsx_sim* h, const rsx_policy_mlp* p, const float* params_dev /* [P], 2 * act_dim outputs */,
                              const rsx_collect_gaussian_cfg* cfg, int n_steps, const rsx_collect_out* out,
                              float* log_std_out /* [T][B][act_dim] or NULL */, void* stream);

/* ---- self-play collection for VSS-v0: a policy-driven opponent inside the launch (additive extension of ABI 6) ---------------------
 * rsx_task_collect_policy with ONE command replaced: yellow robot 0 (body index n_blue) is driven by a second MLP policy, the opponent
 * — typically a frozen earlier copy of the learner — instead of its Ornstein-Uhlenbeck noise.  The opponent is evaluated inside the same
 * launch from the mirrored observation.  Everything else is rsx_task_collect_policy's: the agent's batch, same-step auto-reset, the
 * Gaussian head, the step counter, capture, and every handle shape that call serves.
 *   scope            VSS-v0 with equal teams only (3v3, 5v5): every other task is refused.
 *   actor ...        the agent (blue 0): rsx_task_collect_policy's p, params_dev and sigma_dev.
 *   opponent ...     an rsx_policy_mlp of its own (layers and hidden may differ from the actor's), opponent_params_dev [P2] in the same
 *                    layout for the same obs_dim and act_dim, opponent_sigma_dev [2] or NULL = deterministic; unchecked like the actor's.
 *   mirrored obs     what VSS-v0's observation would be with the team colours swapped and the field turned by 180 degrees, in the same
 *                    layout and obs_dim as the agent's row.  With n = n_blue = n_yellow: ball [0:4]; "own" robot i at 4 + 7 i as
 *                    (x, y, sin, cos, vx, vy, w) holds YELLOW i; "other" robot j at 4 + 7 n + 5 j as (x, y, vx, vy, w) holds BLUE j
 *                    (3v3: 25 + 5 j).  Positions and linear velocities are the float32 negations of the values the agent's normaliser
 *                    produces for the same body (clamp(-v) == -clamp(v) exactly); the angular velocity is unchanged; sin and cos are the
 *                    negations of the body's own sine and cosine (of the stored heading in degrees).  The row is written from the same
 *                    registers, at the same point, as the agent's row: opponent row t and agent row t describe the same instant.  Row 0
 *                    is computed from the state the call starts from.
 *   opponent action  mean = the opponent's output accumulator in rsx_policy_mlp's arithmetic, unchanged; sample = mean + sigma * eps
 *                    (or mean); action = out_act(sample).  eps follows the agent's recipe — the same key (noise_seed), global env id and
 *                    step counter — under domain word 9 instead of 7: the two heads never share a draw.  The opponent's forward is
 *                    computed BEFORE the agent's action is applied: both policies answer observation t.
 *   the command      the two action components go through VSS-v0's action -> wheel-speed map (vss_gym.py:235-254) and replace the
 *                    command of yellow 0 for that step, and only that.  Yellow 0's Ornstein-Uhlenbeck state keeps advancing on its usual
 *                    draws, unused: the handle can be handed back to rsx_task_step or rsx_task_collect_policy at any time, and the
 *                    checkpoint format and every other robot's stream are untouched.
 *   rewards          reward, flags, metrics, final_obs and the handle's obs buffer stay the agent's (blue's). */
typedef struct rsx_selfplay_out {
    float* opp_obs;      /* [T][B][obs_dim] or NULL: the mirrored observation each opponent action answered */
    float* opp_actions;  /* [T][B][2] or NULL: the action that drove yellow 0 */
    float* opp_mean;     /* [T][B][2] or NULL: the opponent's output layer before noise and before out_act */
    float* opp_sample;   /* [T][B][2] or NULL: mean + sigma * eps, before out_act */
} rsx_selfplay_out;
/* Commit: the call advances the handle exactly as n_steps steps of the engine with out->actions[t] for blue 0 and the wheel speeds of
 * opp_actions[t] for yellow 0 would — the step is the engine's step with one command replaced.  `sp` may be NULL (nothing of the
 * opponent is recorded).  LDS: both policies' images share a workgroup (two 40-64-64-2 policies at 8 lanes per env: 79 040 B, two workgroups per CU
 * against the collector's three; 5v5 at 16 lanes per env: 84 608 B, one).
 * Refusals (nothing is enqueued): all of rsx_task_collect_policy's, applied to both policies (the LDS limit is the CU's 160 KB for both
 * images together), and RSX_ERR_ARG for a task other than VSS-v0, unequal teams, a null opponent or opponent_params_dev. */
int rsx_task_collect_selfplay(rsx_sim* h, const rsx_policy_mlp* actor, const float* actor_params_dev, const float* sigma_dev,
                              const rsx_policy_mlp* opponent, const float* opponent_params_dev, const float* opponent_sigma_dev,
                              uint64_t noise_seed, int n_steps, const rsx_collect_out* out, const rsx_selfplay_out* sp, void* stream);

/* ---- team play for VSS-v0: every robot of a side driven by that side's policy inside the launch (additive extension of ABI 6) ------
 * rsx_task_collect_selfplay extended from one seat per side to all of them.  A SEAT is a robot driven by a policy: blue seat i is blue
 * robot i, yellow seat i is yellow robot i (body index n_blue + i).  All blue seats share the actor's parameters, all yellow seats the
 * opponent's.  Equal teams (n = n_blue = n_yellow), VSS-v0 only.
 *   seat counts      actor_seats is 1 or n_blue; opponent_seats is 0 (opponent must then be NULL), 1 or n_yellow (opponent non-NULL).
 *                    (1, 0) is rsx_task_collect_policy and (1, 1) rsx_task_collect_selfplay, bit for bit in every output and in the
 *                    checkpoint afterwards.  Robots that are not seated keep their Ornstein-Uhlenbeck commands.
 *   seat map         blue seat i sees VSS-v0's row with "own" slots 0 and i exchanged: entry j of the seat's row is entry
 *                      j + 7 i   for 4 <= j < 11            (slot 0 <- slot i)
 *                      j - 7 i   for 4 + 7 i <= j < 11 + 7 i  (slot i <- slot 0)
 *                      j         otherwise                   (the ball [0:4], the remaining "own" slots, every "other" slot)
 *                    of the side's row.  Seat 0's row is the engine's observation bit for bit.  Yellow seat i sees the mirrored row of
 *                    rsx_task_collect_selfplay under the same exchange.  The exchange moves float32 values and does no arithmetic.
 *   forward, head    the arithmetic is rsx_policy_mlp's, unchanged, once per seat on the seat's row.  The Gaussian head is
 *                    rsx_task_collect_policy's with the seat in Philox counter word 1:
 *                      counter = (global env id, seat, tick of that step, dom | (i >> 2) << 8),  key = (noise_seed lo, noise_seed hi)
 *                    dom = 7 for the actor's seats and 9 for the opponent's; component i takes normal i & 3.  Seat 0 therefore draws
 *                    exactly what rsx_task_collect_policy and rsx_task_collect_selfplay draw.  All seats answer observation t.
 *   the commands     each seat's two outputs go through VSS-v0's action -> wheel-speed map and replace the command of its robot for
 *                    that step (blue 0's action takes the engine's own path).  Every Ornstein-Uhlenbeck state keeps advancing on its
 *                    usual draws, unused: the handle can go back to rsx_task_step, rsx_task_collect_policy or
 *                    rsx_task_collect_selfplay at any time, and the checkpoint format is untouched.
 *   everything else  stays the engine's: VSS-v0's ONE reward per env (its energy term on blue 0's command), flags, metrics, same-step
 *                    auto-reset, the step counter, per-env physics redraws, and the handle's obs / final_obs buffers, which hold seat
 *                    0's rows. */
typedef struct rsx_team_side_out {   /* S = that side's seat count */
    float* obs;       /* [T][B][S][obs_dim]  the row each seat's action answered; required for the actor */
    float* actions;   /* [T][B][S][2]        required for the actor */
    float* mean;      /* [T][B][S][2]  or NULL */
    float* sample;    /* [T][B][S][2]  or NULL */
    float* final_obs; /* [T][B][S][obs_dim] or NULL: rows of ended (t, env) only */
    float* next_obs;  /* [B][S][obs_dim]    or NULL: the seats' rows after the last step */
} rsx_team_side_out;
typedef struct rsx_team_out {
    float*   rewards;   /* [T][B]  required */
    uint8_t* flags;     /* [T][B]  bit 0 terminated, bit 1 truncated; required */
    rsx_team_side_out actor, opponent;   /* opponent: every member optional, ignored when opponent_seats == 0 */
} rsx_team_out;
/* LDS: one image per side in a workgroup, the seat rows made in place (two 40-64-64-2 policies at 8 lanes per env, 3v3: 79 040 B, two
 * workgroups per CU, what rsx_task_collect_selfplay takes; 5v5 at 16 lanes per env: 84 736 B, one).
 * Refusals (nothing is enqueued, RSX_ERR_ARG): everything rsx_task_collect_selfplay refuses (of the opponent only when it is seated),
 * an actor_seats outside {1, n_blue}, an opponent_seats outside {0, 1, n_yellow}, opponent_seats > 0 with a NULL opponent or
 * opponent_params_dev, opponent_seats == 0 with a non-NULL opponent, a NULL out, rewards, flags, actor.obs or actor.actions. */
int rsx_task_collect_team(rsx_sim* h, const rsx_policy_mlp* actor, const float* actor_params_dev, const float* sigma_dev, int actor_seats,
                          const rsx_policy_mlp* opponent /* NULL iff opponent_seats == 0 */, const float* opponent_params_dev,
                          const float* opponent_sigma_dev, int opponent_seats, uint64_t noise_seed, int n_steps,
                          const rsx_team_out* out, void* stream);

/* ---- matches for VSS-v0: policy against policy inside the lookahead launch (additive extension of ABI 6) --------------------------
 * What a self-play loop asks after every snapshot — did the learner get better, and against whom? — and what a population method
 * needs to run against a frozen opponent: rsx_task_lookahead_policy with rsx_task_collect_team's opponent.  Triple (e, k, m) is env e
 * played by actor k (blue) against opponent m (yellow) from where env e stands now to its first episode end, for all K x M pairs of
 * every env in ONE launch, from the same start states and against the same future draws.  The handle is left exactly as it was.
 *   scope            VSS-v0 with equal teams only (3v3, 5v5 and the run-time counts such as 2v2).  actor_seats is 1 or n_blue,
 *                    opponent_seats is 1 or n_yellow.  There is no 0: without an opponent the call is rsx_task_lookahead_policy.
 *   actor ...        an rsx_policy_mlp and actor_params_dev [K][P], K = n_actors: rsx_task_lookahead_policy's p and params_dev.
 *   opponent ...     an rsx_policy_mlp of its own (layers and hidden may differ) and opponent_params_dev [M][P2], M = n_opponents, in
 *                    the same layout for the same obs_dim and act_dim.  Device memory is not checked.
 *   a step           rsx_task_collect_team's step with deterministic heads: sample = mean, action = out_act(mean).  Every seat of
 *                    both sides answers observation t.  Blue seat i sees the side's row with "own" slots 0 and i exchanged (that
 *                    section's seat map), yellow seats the mirrored row of rsx_task_collect_selfplay under the same exchange.  Each
 *                    seated robot's command is replaced (blue 0's action takes the engine's own path); every Ornstein-Uhlenbeck state
 *                    advances on its usual draws, unused.  The draws are the env's real future ones, at tick (current tick) + t, as in
 *                    rsx_task_lookahead_policy.  No stochastic heads in this call: evaluation noise is the caller's parameter noise.
 *   step 0           sees the env's row of the handle's obs buffer, as rsx_task_lookahead_policy does, and its mirror computed from
 *                    the state the call starts from, as rsx_task_collect_selfplay does.
 *   a pair           stops at its env's first episode end.  returns, steps, flags and last_obs follow rsx_task_lookahead's rules
 *                    (the same float32 recurrence: ret = ret + disc * r_t; disc = disc * gamma; blue's reward).  result is what the task's
 *                    reward reports of the ending step: the goal for (+1) or against (-1) that the metrics' goals_for /
 *                    goals_against count, 0 for a pair that ran into the time limit or the horizon.  Recording rows behind a pair's
 *                    end are not written. */
typedef struct rsx_match_out {          /* pair index p = (e * K + k) * M + m;  S = actor_seats, S2 = opponent_seats */
    float*   returns;      /* [B][K][M]  required: blue's return, rsx_task_lookahead's float32 recurrence */
    int32_t* steps;        /* [B][K][M]  required */
    uint8_t* flags;        /* [B][K][M]  required: bit 0 terminated, bit 1 truncated */
    int8_t*  result;       /* [B][K][M]  or NULL: +1 a goal FOR blue (the actor) ended the pair, -1 a goal against it, 0 otherwise */
    float*   last_obs;     /* [B][K][M][obs_dim] or NULL: blue seat 0's row after the pair's last step (terminal if it ended) */
    float*   actions;      /* [B][K][M][H][S][2]  or NULL */
    float*   obs;          /* [B][K][M][H][S][obs_dim] or NULL: the row each actor seat's action answered */
    float*   opp_actions;  /* [B][K][M][H][S2][2] or NULL */
    float*   opp_obs;      /* [B][K][M][H][S2][obs_dim] or NULL */
} rsx_match_out;
/* Exactness: from the same handle state, rsx_task_collect_team(actor = params[k], sigma = NULL, opponent = params2[m], sigma = NULL,
 * the same seat counts, n_steps = H) produces per env the same bits in rows t < steps[e][k][m]: obs, actions, opp_obs, opp_actions,
 * rewards (through the return recurrence) and flags at the last row; with final_obs recorded, last_obs of an ended pair equals it.
 * This holds on every lane width (8, 16, 32), with and without per-env physics, on host-keyed and device-keyed handles.
 * No side effects: the call reads what rsx_task_lookahead_policy reads (the state, the scalar arena, the obs buffer, the step counter)
 * and both parameter arrays, and writes only `out`.  Stream-ordered, never synchronises, capturable under that call's conditions (a
 * launch at the counter limit of a device-keyed handle simulates nothing).
 * LDS: one image per side in a workgroup, as rsx_task_collect_team (two 40-64-64-2 policies at 8 lanes per env, 3v3: 79 040 B, two
 * workgroups per CU; 5v5 at 16 lanes per env: 84 736 B, one).  One 64-lane workgroup per (tile of envs, k, m).
 * Refusals (RSX_ERR_ARG, nothing is enqueued): everything rsx_task_lookahead_policy refuses of a handle and of each policy (the LDS
 * limit is the CU's 160 KB for both images together, the check rsx_task_collect_team makes); a task other than VSS-v0, or unequal
 * teams; an actor_seats outside {1, n_blue} or an opponent_seats outside {1, n_yellow}; n_actors or n_opponents < 1; a null opponent,
 * actor_params_dev, opponent_params_dev, out, returns, steps or flags; lane_grid x K x M workgroups over the launch limit (2^31 - 1,
 * the check rsx_task_lookahead makes for n_candidates). */
int rsx_task_lookahead_match(rsx_sim* h, const rsx_policy_mlp* actor, const float* actor_params_dev /* [K][P] */, int n_actors, int actor_seats,
                             const rsx_policy_mlp* opponent, const float* opponent_params_dev /* [M][P2] */, int n_opponents, int opponent_seats,
                             int horizon, float gamma, const rsx_match_out* out, void* stream);

/* ---- values and GAE advantages of a collected batch (additive extension of ABI 6) ------------------------------------------------
 * What an on-policy trainer does between rsx_task_collect_policy and its gradient step: evaluate a critic on the [T][B] batch and run
 * the reverse recurrence of generalised advantage estimation — two launches instead of a torch critic plus a Python loop over T.
 *   the handle       supplies only the device, obs_dim and the error string: the call reads and writes NOTHING of the envs, works on any
 *                    handle with a task attached, before or after rsx_task_reset, and needs no step counter — host-keyed and
 *                    device-keyed handles both capture.
 *   critic           an rsx_policy_mlp with act_dim = 1 and out_act = RSX_ACT_NONE (a linear output); critic_params_dev [P] in
 *                    rsx_policy_mlp's layout with act_dim = 1: W1 [hidden][obs_dim], b1, (W2, b2,) Wo [1][hidden], bo [1];
 *                    P = rsx_critic_num_params (rsx_policy_num_params counts a policy of the TASK's act_dim and keeps refusing
 *                    RSX_ACT_NONE, so the critic has a call of its own).
 *   terminated, truncated   separate byte arrays, non-zero = true: the bool tensors of a collected batch and the flag tensors of a
 *                    stepping loop both go in as they are.  n_envs is the batch's B, any >= 1 (not the handle's num_envs).
 * The arithmetic is fixed, all float32, the unit is built with -ffp-contract=off:
 *   V(x)             the critic's output accumulator in exactly rsx_policy_mlp's order: per unit acc = bias; for i ascending:
 *                    acc = fmaf(W[j][i], x[i], acc); hidden activations as there; no activation on the output.  Hence, for a critic
 *                    that shares its hidden layers with an actor and whose output row is the actor's output row 0, values[t][e]
 *                    equals rsx_collect_out.mean[t][e][0] bit for bit.
 *   end              terminated || truncated
 *   nv               terminated: 0;  truncated only: V(final_obs[t][e]), or 0 when final_obs == NULL;  otherwise values[t + 1][e]
 *                    for t < T - 1 and V(last_obs[e]) for the last row.  (With same-step auto-reset obs[t + 1] of an env that ended
 *                    at t belongs to the next episode: the bootstrap of a time limit comes from the terminal observation.)
 *   delta            (r + gamma * nv) - v: one multiplication, one addition, one subtraction, each rounded
 *   adv              end ? delta : delta + gl * adv_next, with adv_next = 0 behind the last row and gl = (float)gamma * (float)lam,
 *                    computed once on the host
 *   ret              adv + v
 * Selection is by select, never by a multiplication with 0: final_obs rows that were never written and the carried advantage of an
 * ended row (NaN included) reach no output.
 * The call owns no memory: V(last_obs) passes through row T - 1 of `advantages` and V(final_obs) through the truncated-only rows of
 * `returns` before those rows receive their results, so the three required outputs must not overlap each other or an input.
 * RSX_GAE_FORM=groups in the environment evaluates the critic eight lanes per row as the collector does (the same bits; the default is
 * one row per lane, profiles/LABBOOK.md has the comparison).
 * Stream-ordered, never synchronises, never allocates, capturable.  Refusals (nothing is enqueued, rsx_last_error says why), all
 * RSX_ERR_ARG: a null critic, critic_params_dev, in, out or required array; n_steps < 1 or n_envs < 1; gamma or lam non-finite or
 * outside [0, 1]; n_hidden_layers, hidden or hidden_act outside rsx_policy_mlp's listed values; out_act != RSX_ACT_NONE; a handle
 * without a task; a critic whose weights and hidden rows do not fit a workgroup's 64 KB of LDS (2 x 64 units fit every observation a
 * task can have). */
#define RSX_ACT_NONE 3   /* identity: accepted as out_act by rsx_task_advantages ONLY; every other call keeps refusing it */
typedef struct rsx_adv_in {
    const float*   obs;         /* [T][B][obs_dim]   required */
    const float*   rewards;     /* [T][B]            required */
    const uint8_t* terminated;  /* [T][B] non-zero = true   required */
    const uint8_t* truncated;   /* [T][B] non-zero = true   required */
    const float*   final_obs;   /* [T][B][obs_dim] or NULL; read ONLY in rows truncated && !terminated */
    const float*   last_obs;    /* [B][obs_dim]: the observation after step T - 1   required */
} rsx_adv_in;
typedef struct rsx_adv_out {
    float* values;       /* [T][B] V(obs[t])                       required */
    float* advantages;   /* [T][B]                                 required */
    float* returns;      /* [T][B] advantages + values             required */
    float* next_values;  /* [T][B] or NULL: the value row t bootstrapped from */
} rsx_adv_out;
int rsx_critic_num_params(const rsx_sim* h, const rsx_policy_mlp* critic, int64_t* out);
int rsx_task_advantages(rsx_sim* h, const rsx_policy_mlp* critic, const float* critic_params_dev /* [P] with act_dim = 1 */,
                        float gamma, float lam, int n_steps /* T */, int n_envs /* B, any >= 1 */,
                        const rsx_adv_in* in, const rsx_adv_out* out, void* stream);

/* ---- PPO loss gradients of an MLP actor and critic on a collected batch (additive extension of ABI 6) ------------------------------
 * What an on-policy trainer does with a minibatch between rsx_task_advantages and its optimiser step: the forward pass of both
 * networks on the minibatch's rows, the clipped-surrogate and value losses, and their gradients — three launches instead of torch's
 * gather, two MLP forwards, a few dozen elementwise kernels and backward().
 *   the handle       supplies only the device, obs_dim, act_dim and the error string, as for rsx_task_advantages: the call reads and
 *                    writes NOTHING of the envs; host-keyed and device-keyed handles both capture.
 *   actor            an rsx_policy_mlp as rsx_task_collect_policy takes it, actor_params_dev [P_actor] (rsx_policy_num_params); its
 *                    out_act plays no part: the density is that of the pre-out_act sample, as collected.  log_std_dev [act_dim].
 *   critic           as for rsx_task_advantages (out_act = RSX_ACT_NONE), critic_params_dev [P_critic] (rsx_critic_num_params).
 *   rows             the minibatch as flat indices into the N = T * B rows of the batch, repeats allowed; NULL: rows 0 .. M - 1.  Device
 *                    memory is NOT checked: an index outside [0, N) (a padding entry, say -1) contributes nothing to any output, is
 *                    counted in stats[7], and nothing outside the arrays is read for it.
 * The loss, with every mean a sum over the M entries divided by M (skipped entries do not change the divisor):
 *   mean_a           the actor's output accumulator before out_act;  value = the critic's output
 *   z_a              (sample_a - mean_a) / exp(log_std_a)
 *   lp               sum over a of (-0.5 z_a^2 - log_std_a - 0.5 log 2 pi)
 *   ratio            exp(lp - old_log_prob)
 *   L_pi             -mean(min(ratio * A, clamp(ratio, 1 - clip, 1 + clip) * A))
 *   L_v              0.5 * mean((value - ret)^2)
 *   entropy          sum over a of (log_std_a + 0.5 + 0.5 log 2 pi)
 *   L                L_pi + vf_coef * L_v - ent_coef * entropy
 * The outputs are the gradients of L.  Through the min they follow torch's autograd (a tie splits in half and both halves reach
 * ratio; clamp passes the gradient at its bounds):  dL_pi / dratio = -A / M  where  1 - clip <= ratio <= 1 + clip  or
 * ratio * A < clamp(ratio) * A,  else 0 — so at ratio == 1 and at ratio == 1 +- clip the gradient flows for both signs of A.
 * The bounds 1 - clip and 1 + clip are computed in float32.  Activation derivatives come from the stored activation: tanh 1 - h^2,
 * relu h > 0.
 * Arithmetic, all float32, the unit is built with -ffp-contract=off.  Forward: rsx_policy_mlp's, bit for bit (per unit acc = bias,
 * ascending fmaf, the same tanh), so `mean` equals rsx_collect_out.mean and `value` equals rsx_adv_out.values on the same parameters
 * and rows.  Backward: minibatch entries are taken in blocks of 64; workgroup w of G = min(ceil(M / 64), max_workgroups) takes blocks
 * w, w + G, ...  Per entry dL/dmean_a = dlp * (z_a / sigma_a) and dL/dlog_std_a = dlp * (z_a^2 - 1) with dlp = (-(A / M)) * ratio where
 * the gradient flows, dL/dvalue = ((value - ret) * vf_coef) / M (the division by M is a multiplication by the float32 1 / M);
 * dz = (W^T d(next)) * act', the product with the second layer's weights summed as four interleaved fmaf chains over the units,
 * combined (s0 + s1) + (s2 + s3).  A weight or bias gradient is ONE fmaf (bias: addition) chain per workgroup over all its entries in
 * the order it met them, starting from 0 (v_mfma_f32_32x32x2_f32, which is a k-ordered fmaf chain, for the hidden layers' weights); the
 * per-workgroup partials are then added in workgroup order, starting from 0.  The stats and the log_std gradient are summed per lane
 * (entry mod 64), then over the lanes in ascending order, then over the workgroups.  Hence the result bits are a function of the inputs
 * and of G alone — not of the device, its CU count or the timing.
 *   stats            [8]: 0 L_pi, 1 L_v, 2 entropy, 3 approx_kl = mean((ratio - 1) - log ratio), 4 clip_fraction = the share of entries
 *                    with ratio outside [1 - clip, 1 + clip], 5 mean ratio, 6 entries used, 7 entries skipped
 *   mean, value      optional: the forward pass's outputs per minibatch entry (0 for a skipped entry)
 *   workspace        at least rsx_ppo_gradient_workspace bytes (one partial per workgroup and network), 16-byte aligned, for the same
 *                    n_rows and max_workgroups; its contents before the call do not matter
 *   max_workgroups   0: the default, a constant of the build (512), not the device's CU count; > 0: caps G
 * Stream-ordered, never synchronises, never allocates, capturable.  Refusals (nothing is enqueued, rsx_last_error says why), all
 * RSX_ERR_ARG: a null actor, critic, parameter or log_std array, in, cfg, out or required array; n_rows < 1, n_batch_rows < 1 or
 * either above 2^31 - 1; clip non-finite or outside (0, 1); vf_coef or ent_coef non-finite; max_workgroups < 0; a spec outside
 * rsx_policy_mlp's listed values (the critic's out_act != RSX_ACT_NONE); a handle without a task; the scrimmage task; a network whose
 * weights and row buffers do not fit a workgroup's 64 KB of LDS (2 x 64 units fit 64 observation floats). */
typedef struct rsx_ppo_in {
    const float*   obs;           /* [N][obs_dim]   required */
    const float*   sample;        /* [N][act_dim]   the pre-out_act sample rsx_task_collect_policy records   required */
    const float*   old_log_prob;  /* [N]            log-density under the collecting policy   required */
    const float*   advantage;     /* [N]            required */
    const float*   ret;           /* [N]            returns   required */
    const int32_t* rows;          /* [M] flat row indices, repeats allowed, or NULL = rows 0 .. M - 1 */
    int64_t        n_batch_rows;  /* N */
    int64_t        n_rows;        /* M */
} rsx_ppo_in;
typedef struct rsx_ppo_cfg {
    float   clip;            /* in (0, 1) */
    float   vf_coef;         /* finite */
    float   ent_coef;        /* finite */
    int32_t max_workgroups;  /* 0 = the build's default; > 0 caps the grid */
} rsx_ppo_cfg;
typedef struct rsx_ppo_out {
    float* grad_actor;    /* [P_actor]    required */
    float* grad_log_std;  /* [act_dim]    required */
    float* grad_critic;   /* [P_critic]   required */
    float* stats;         /* [8]          required */
    float* mean;          /* [M][act_dim] or NULL */
    float* value;         /* [M] or NULL */
    void*  workspace;     /* rsx_ppo_gradient_workspace bytes   required */
} rsx_ppo_out;
int rsx_ppo_gradient_workspace(const rsx_sim* h, const rsx_policy_mlp* actor, const rsx_policy_mlp* critic,
                               int64_t n_rows, int max_workgroups, int64_t* bytes_out);
int rsx_task_ppo_gradient(rsx_sim* h, const rsx_policy_mlp* actor, const float* actor_params_dev, const float* log_std_dev,
                          const rsx_policy_mlp* critic, const float* critic_params_dev,
                          const rsx_ppo_in* in, const rsx_ppo_cfg* cfg, const rsx_ppo_out* out, void* stream);

/* ---- the PPO update phase on the device: normalise, shuffle, clip, Adam, KL stop (additive extension of ABI 6) ---------------------
 * What an on-policy trainer does around rsx_task_ppo_gradient: normalise the advantages once per batch, draw a fresh permutation of
 * the rows per epoch, and per minibatch clip the gradient's global norm and take an Adam step — here stream-ordered and keyed by
 * counters that live on the device, so that rsx_task_collect_policy + rsx_task_ppo_update captured once is one whole PPO iteration
 * per replay.  rsx_ppo_normalize, rsx_ppo_permutation, rsx_adam_step and rsx_adam_mark take no handle: they run on the thread's current
 * device.  Every call is stream-ordered, never synchronises, never allocates and is capturable; invalid arguments are refused with
 * RSX_ERR_ARG before anything is enqueued (rsx_last_error says why); no float atomics: the result bits are a function of the inputs
 * (and, for rsx_task_ppo_update, of max_workgroups) alone.
 *
 * Reductions (the two moments of the advantages, the squared gradient norm) share one FIXED order, in float64: thread j of workgroup w
 * (256 threads, G workgroups, G = min(ceil(n / 256), C) with C a constant of the build: 128 for the moments, 64 for the norm) adds
 * its elements i = 256 w + j, + 256 G, ... ascending, from 0.0; a workgroup adds the 64 lanes of each of its four waves ascending
 * from 0.0 and then the waves ((w0 + w1) + w2) + w3; the G partials are added in workgroup order from 0.0.
 *
 * rsx_ppo_normalize:  out[i] = (adv[i] - mean) / (std + eps)  over n entries, in two launches.
 *   S = sum x, Q = sum x * x (the float32 entries widened; reduced as above);  mean64 = S / n;  var64 = (Q - S * mean64) / (n - 1)
 *   (Bessel's correction, as torch's std()), a negative var64 is 0;  mean = (float)mean64, std = (float)sqrt(var64);  then per entry a
 *   float32 subtraction, addition and division, each rounded.  mean_std_dev [2] or NULL receives mean and std.  out_dev must not
 *   overlap adv_dev.  workspace_dev: RSX_PPO_NORMALIZE_WORKSPACE_BYTES, 8-byte aligned.  Refused: a null adv_dev, out_dev or
 *   workspace_dev, n < 2 (no standard deviation) or n > 2^31 - 1, eps negative or non-finite. */
#define RSX_PPO_NORMALIZE_WORKSPACE_BYTES 2048
int rsx_ppo_normalize(const float* adv_dev, int64_t n, float eps, float* out_dev, float* mean_std_dev, void* workspace_dev, void* stream);
/* rsx_ppo_permutation:  rows_dev [n] int32 := a permutation of 0 .. n - 1, every entry computed on its own from (seed, update, epoch,
 * i) — no sort, no state.  All arithmetic is on 32-bit unsigned integers:
 *   bits = max(8, ceil(log2 n)), the domain is [0, 2^bits);  wa = bits / 2 (integer), wb = bits - wa  (at least 8 bits: halves
 *          narrower than four bits mix too slowly for eight rounds — measured on the host restatement, profiles/LABBOOK.md)
 *   E(x):  a = x & (2^wa - 1), b = x >> wa;  for r = 0 .. 7:  f = word 0 of philox4x32-7(counter = (b, epoch, update, 8 | r << 8), key =
 *          (seed lo, seed hi));  (a, b) := (b, (a ^ f) & (2^wa - 1));  swap wa and wb.   E(x) = a | b << wa
 *          (an unbalanced Feistel network: each round is invertible whatever f is, so E is a bijection of the domain)
 *   rows[i]:  x = E(i); while x >= n: x = E(x)      (cycle walking: the walk follows i's cycle of E, which holds at most 2^bits - n
 *          values outside [0, n), so it ends within 2^bits - n + 1 applications — the bound of the kernel's loop; for n >= 128,
 *          2^bits < 2 n makes the expected number less than 2)
 *   update   the low 32 bits of `update`, or, with update_dev != NULL, of the int64 it points to, read on the device when the launch
 *            runs: pass rsx_adam_state.counters + RSX_ADAM_UPDATES and a replayed graph draws a new permutation on every replay (the
 *            tick design of the engine's other draws).
 * Minibatch k of M covers rows[k c .. min((k + 1) c, n)) with c = ceil(n / M): torch.chunk's sizes.
 * Refused: a null rows_dev, n < 1 or n > 2^31 - 1, epoch outside [0, 2^32). */
int rsx_ppo_permutation(int32_t* rows_dev, int64_t n, uint64_t seed, uint64_t update, const int64_t* update_dev, int64_t epoch, void* stream);
/* rsx_adam_step:  torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam (no amsgrad, no weight decay) on three flat tensors —
 * the actor's parameters, log_std and the critic's parameters — in two launches.
 *   counters   int64 [4] device memory, part of the optimiser state (zero at the start of training): */
#define RSX_ADAM_T       0   /* Adam's step count t */
#define RSX_ADAM_UPDATES 1   /* updates finished (rsx_adam_mark end / rsx_task_ppo_update): the permutation's key */
#define RSX_ADAM_APPLIED 2   /* steps applied since the last update began */
#define RSX_ADAM_STOPPED 3   /* non-zero: the KL stop was hit in the current update; every later step is withheld */
/*   norm   = (float)sqrt(sum g^2) over the concatenation actor | log_std | critic, reduced as above (each g widened, g * g exact)
 *   coef   = min(1, max_grad_norm / (norm + 1e-6f)) in float32;  max_grad_norm <= 0: coef = 1 (no clipping)
 *   the gate   with target_kl > 0 and approx_kl != NULL, a step whose approx_kl[0] is not <= target_kl (a NaN included) sets STOPPED
 *          before its own step.  A step with STOPPED set is WITHHELD: it changes no parameter, no moment and not t (selected, never
 *          multiplied by 0; its launches still run — the price of not asking the host).  Otherwise t := t + 1, APPLIED += 1 and
 *   bc1 = 1 - beta1^t, bc2 = 1 - beta2^t in float64 from the device's t;  beta^t by squaring (r = 1; while t: if t & 1: r *= b;
 *          b *= b; t >>= 1), so that the bits can be restated on a host
 *   g' = g * coef;   m = b1 * m + omb1 * g';   v = b2 * v + (omb2 * g') * g';   p = p - step * (m / (sqrtf(v) / s2 + eps))
 *          in float32, every operation rounded, with b = (float)beta, omb = (float)(1.0 - beta), step = (float)((double)lr / bc1),
 *          s2 = (float)sqrt(bc2).  A gradient entry that is 0 while its m is 0 leaves its parameter as it was.
 *   lr     cfg->lr, or with cfg->lr_dev != NULL the float it points to, read on the device (a schedule under graph replay).
 *   stats  [2] or NULL: the norm before the clip; 1.0f when the step was applied, 0.0f when it was withheld.
 *   workspace   RSX_ADAM_WORKSPACE_BYTES, 8-byte aligned.
 * Refused: a null cfg, st, io or required array; a size < 1 or a total above 2^31 - 1; lr or eps negative or non-finite; a beta outside
 * [0, 1); max_grad_norm or target_kl non-finite, target_kl negative. */
#define RSX_ADAM_WORKSPACE_BYTES 1024
typedef struct rsx_adam_cfg {
    double       beta1;          /* in [0, 1) */
    double       beta2;          /* in [0, 1) */
    const float* lr_dev;         /* [1] device memory, or NULL = lr */
    float        lr;             /* >= 0, finite */
    float        eps;            /* >= 0, finite */
    float        max_grad_norm;  /* <= 0: no clipping */
    float        target_kl;      /* 0: no KL stop; > 0: see the gate */
} rsx_adam_cfg;
typedef struct rsx_adam_state {
    float*   m_actor;     /* [n_actor] */
    float*   v_actor;
    float*   m_log_std;   /* [n_log_std] */
    float*   v_log_std;
    float*   m_critic;    /* [n_critic] */
    float*   v_critic;
    int64_t* counters;    /* [4], RSX_ADAM_* */
    int64_t  n_actor;
    int64_t  n_log_std;
    int64_t  n_critic;
} rsx_adam_state;
typedef struct rsx_adam_io {
    float*       actor_params;   /* [n_actor]    updated in place   required */
    float*       log_std;        /* [n_log_std]  updated in place   required */
    float*       critic_params;  /* [n_critic]   updated in place   required */
    const float* grad_actor;     /* required */
    const float* grad_log_std;   /* required */
    const float* grad_critic;    /* required */
    const float* approx_kl;      /* [1] or NULL: what the gate compares with target_kl */
    float*       stats;          /* [2] or NULL */
    void*        workspace;      /* RSX_ADAM_WORKSPACE_BYTES   required */
} rsx_adam_io;
int rsx_adam_step(const rsx_adam_cfg* cfg, const rsx_adam_state* st, const rsx_adam_io* io, void* stream);
/* end == 0: an update begins (APPLIED := 0, STOPPED := 0);  end != 0: it ends (UPDATES += 1).  One tiny launch. */
int rsx_adam_mark(const rsx_adam_state* st, int end, void* stream);
/* rsx_task_ppo_update:  the whole update phase in one call.  It enqueues, in this order: rsx_adam_mark(begin); with
 * normalize_advantage, rsx_ppo_normalize of in->advantage into the workspace (once per batch); per epoch e = 0 .. epochs - 1
 * rsx_ppo_permutation(n = n_batch_rows, seed, update = the DEVICE's counters[RSX_ADAM_UPDATES], epoch = e) into the workspace, and per
 * minibatch k rsx_task_ppo_gradient on rows[k c .. min((k + 1) c, n)) (c = ceil(n / minibatches)) with the normalised advantages,
 * followed by rsx_adam_step with approx_kl = that gradient call's stats[3];  rsx_adam_mark(end).  The results equal that sequence of
 * calls bit for bit.
 *   the handle, actor, critic, in, cfg    as for rsx_task_ppo_gradient; in->rows must be NULL and in->n_rows is ignored.
 *   actor_params_dev, log_std_dev, critic_params_dev   updated in place.  Nothing `in` points to is written.
 *   stats_dev   [epochs][minibatches][RSX_PPO_UPDATE_STATS]: rsx_task_ppo_gradient's eight, 8 the gradient norm before the clip, 9
 *               whether the step was applied
 *   workspace   rsx_ppo_update_workspace bytes, 16-byte aligned: rsx_task_ppo_gradient's for c rows, the rows, the normalised
 *               advantages, the three gradients and the partials.  rows_offset_out (or NULL): where in it the int32 rows [n] of the
 *               last epoch lie after the call.
 * Refused: everything rsx_task_ppo_gradient and rsx_adam_step refuse; a null u, stats_dev or workspace; epochs < 1; minibatches < 1 or
 * so many that the last chunk would be empty ((minibatches - 1) * c >= n); n_batch_rows < 2 with normalize_advantage; norm_eps negative
 * or non-finite; a non-NULL in->rows; state sizes (st->n_*) that are not the two networks' and act_dim. */
#define RSX_PPO_UPDATE_STATS 10
typedef struct rsx_ppo_update_cfg {
    uint64_t seed;                 /* the permutations' key */
    int32_t  epochs;               /* >= 1 */
    int32_t  minibatches;          /* >= 1 */
    int32_t  normalize_advantage;  /* 0 | 1 */
    float    norm_eps;             /* rsx_ppo_normalize's eps */
} rsx_ppo_update_cfg;
int rsx_ppo_update_workspace(const rsx_sim* h, const rsx_policy_mlp* actor, const rsx_policy_mlp* critic, int64_t n_batch_rows,
                             int minibatches, int max_workgroups, int64_t* bytes_out, int64_t* rows_offset_out);
int rsx_task_ppo_update(rsx_sim* h, const rsx_policy_mlp* actor, float* actor_params_dev, float* log_std_dev,
                        const rsx_policy_mlp* critic, float* critic_params_dev, const rsx_ppo_in* in, const rsx_ppo_cfg* cfg,
                        const rsx_ppo_update_cfg* u, const rsx_adam_cfg* adam, const rsx_adam_state* st, float* stats_dev,
                        void* workspace, void* stream);

/* ---- TD3 / DDPG loss gradients of an MLP actor and one or two Q critics on replayed transitions (additive extension of ABI 6) ------
 * What an off-policy trainer does with a minibatch between sampling it and its optimiser steps: the target actor and target critics
 * on next_obs, the critics on (obs, action), the actor through critic 0, and the gradients of both losses — four launches instead of
 * torch's gather, six MLP forwards and two backward().
 *   the handle       supplies only the device, obs_dim (OD), act_dim (AD) and the error string, as for rsx_task_ppo_gradient: the call
 *                    reads and writes NOTHING of the envs.
 *   transitions      N flat rows: obs [N][OD], action [N][AD] (the executed action, after out_act), reward [N], next_obs [N][OD],
 *                    terminated [N] bytes (non-zero = true).  A row that ended on a time limit carries terminated = 0 and its terminal
 *                    observation as next_obs: the target bootstraps through it.
 *   rows             the minibatch, rsx_ppo_in's rules: flat indices into the N rows, repeats allowed, NULL = rows 0 .. M - 1; an index
 *                    outside [0, N) contributes nothing to any output, is counted in stats[8], and nothing outside the arrays is read for it.
 *   actor            an rsx_policy_mlp with out_act RSX_ACT_TANH or RSX_ACT_CLIP, actor_params_dev [Pa] (rsx_policy_num_params) and
 *                    target_actor_params_dev [Pa].
 *   critics          C = cfg->n_critics in {1, 2} networks of ONE shape: an rsx_policy_mlp with out_act = RSX_ACT_NONE whose input row is
 *                    the OD observation floats followed by the AD action floats — torch's Linear(OD + AD, hidden) layout, so
 *                    Pc = hidden * (OD + AD) + hidden (+ hidden * hidden + hidden) + hidden + 1.  critic_params_dev and
 *                    target_critic_params_dev are [C][Pc].
 * The loss; mu is the actor's output accumulator before out_act, pi = out_act(mu), a mean is the sum over the M entries times the
 * float32 1 / M (skipped entries do not change the divisor), t is an entry's POSITION in the minibatch:
 *   noise_k          clamp(sigma * eps_k, -noise_clip, noise_clip) in float32.  eps: the collector's standard-normal recipe (Philox, 7
 *                    rounds, the two-word Box-Muller pair of rsx_task_collect_policy) under domain word 10: counter (t, noise_step >> 32,
 *                    noise_step & 0xFFFFFFFF, 10 | (k >> 2) << 8), key = noise_seed (lo, hi); component k takes normal k & 3 of its
 *                    block.  A draw depends on the position in the minibatch — not on rows[t], the grid or the device.  noise_step is
 *                    cfg->noise_step, or, with noise_step_dev non-NULL, the int64 it points to, read on the device when the launch
 *                    runs: a replayed graph draws fresh noise when that counter was advanced.
 *   a'_k             clamp(pi_targ(next_obs)_k + noise_k, -1, 1); with sigma == 0 no draw is made and a' = pi_targ(next_obs) (DDPG).
 *   y                terminated ? reward : reward + gamma * min over c of Q_targ_c(next_obs, a')   (two roundings).  No gradient flows
 *                    into y; min and both clamps are continuous, a tie of the two critics leaves y what either gives.
 *   L_q              sum over c of 0.5 * mean((Q_c(obs, action) - y)^2): grad_critics[c] = dL_q / d(critic c's parameters).
 *   L_pi             -mean(Q_0(obs, pi(obs))): grad_actor = dL_pi / d(actor's parameters).  Critic 0 is differentiated with respect to
 *                    its action inputs, dQ/da_k = sum over j of W1[j][OD + k] * dz1[j], not its weights.  Through out_act: tanh passes
 *                    1 - pi^2; clip follows torch's clamp: 1 where -1 <= mu <= 1, bounds included, else 0.
 * With out->grad_actor == NULL the actor launch is skipped (TD3's delayed policy update): stats[4] is 0, out->action is not written and
 * every other output has the bits it has with the actor launch.
 * Arithmetic, all float32, the unit is built with -ffp-contract=off.  Forwards: rsx_policy_mlp's, bit for bit (per unit acc = bias,
 * ascending fmaf over the OD observation floats, then over the AD action floats; the same tanh), so out->action equals what
 * rsx_task_collect_policy records without noise.  Backward: rsx_task_ppo_gradient's rules — entries in blocks of 64, workgroup w of
 * G = min(ceil(M / 64), max_workgroups) takes blocks w, w + G, ...; dL_q/dQ_c = (Q_c - y) * (1 / M), dL_pi/dQ_0 = -(1 / M);
 * dz = (W^T d(next)) * act' with the second layer's product summed as four interleaved fmaf chains over the units, combined
 * (s0 + s1) + (s2 + s3), and dQ/da_k summed the same way over the units j; a weight gradient is ONE fmaf chain per workgroup over all its
 * entries in the order it met them, starting from 0 (v_mfma_f32_32x32x2_f32 for the hidden layers' weights); a bias gradient — unlike
 * rsx_task_ppo_gradient's — adds, per block of 64 entries, the workgroup's running sum and the block's terms in ascending order in
 * float64 and rounds to float32 once (a critic's output bias gradient is mean(Q - y), whose terms cancel); the per-workgroup partials
 * are then added in workgroup order from 0; the stats are summed per lane (entry mod 64), then over
 * the lanes in ascending order, then over the workgroups.  The result bits are a function of the inputs and of G alone.
 *   stats            [9]: 0 / 1 L_q of critic 0 / 1 (0.5 * mean((Q_c - y)^2); 0 for an absent critic), 2 / 3 mean Q_0 / Q_1, 4 L_pi,
 *                    5 mean y, 6 mean |a'| (the mean over the entries of sum_k |a'_k|, divided by AD), 7 entries used, 8 entries skipped
 *   per entry        optional, 0 for a skipped entry: target [M] = y; q [C][M]; action [M][AD] = pi(obs) (actor launch only);
 *                    target_noise [M][AD] = noise as added (0 with sigma == 0)
 *   workspace        at least rsx_dpg_gradient_workspace bytes (y, one float per entry more, one partial per workgroup and network),
 *                    16-byte aligned, for the same n_critics, n_rows and max_workgroups; its contents before the call do not matter
 *   max_workgroups   0: the default, a constant of the build (256), not the device's CU count; > 0: caps G
 * LDS per workgroup at the largest shape (2 x 64 units, OD = 64, AD = 5, C = 2): targets 128 000 B, critic 63 344 B, actor 136 080 B;
 * gfx950 has 160 KB per CU.  A shape that needs more than 163 840 B in a launch is refused with the byte count in the error string.
 * Stream-ordered, never synchronises, never allocates, capturable.  Refusals (nothing is enqueued, rsx_last_error says why), all
 * RSX_ERR_ARG: a null actor, critic, parameter array, in, cfg, out or required array; n_rows < 1, n_batch_rows < 1 or either above
 * 2^31 - 1; n_critics outside {1, 2}; gamma outside [0, 1]; sigma or noise_clip negative or non-finite; max_workgroups < 0; a spec
 * outside rsx_policy_mlp's listed values (the actor's out_act neither tanh nor clip, the critic's not RSX_ACT_NONE); act_dim > 8; a
 * handle without a task; the scrimmage task; a shape whose launches do not fit a CU's LDS. */
typedef struct rsx_dpg_in {
    const float*   obs;           /* [N][obs_dim]   required */
    const float*   action;        /* [N][act_dim]   the executed action   required */
    const float*   reward;        /* [N]            required */
    const float*   next_obs;      /* [N][obs_dim]   the row's true successor   required */
    const uint8_t* terminated;    /* [N] non-zero = true   required */
    const int32_t* rows;          /* [M] flat row indices, repeats allowed, or NULL = rows 0 .. M - 1 */
    int64_t        n_batch_rows;  /* N */
    int64_t        n_rows;        /* M */
} rsx_dpg_in;
typedef struct rsx_dpg_cfg {
    const int64_t* noise_step_dev;  /* NULL: noise_step; else the device address of the step */
    uint64_t       noise_seed;
    int64_t        noise_step;
    float          gamma;           /* in [0, 1] */
    float          sigma;           /* >= 0; 0: no smoothing noise */
    float          noise_clip;      /* >= 0 */
    int32_t        n_critics;       /* 1 or 2 */
    int32_t        max_workgroups;  /* 0 = the build's default; > 0 caps the grid */
} rsx_dpg_cfg;
typedef struct rsx_dpg_out {
    float* grad_actor;    /* [Pa] or NULL: no actor launch */
    float* grad_critics;  /* [C][Pc]   required */
    float* stats;         /* [9]       required */
    float* target;        /* [M] or NULL */
    float* q;             /* [C][M] or NULL */
    float* action;        /* [M][act_dim] or NULL */
    float* target_noise;  /* [M][act_dim] or NULL */
    void*  workspace;     /* rsx_dpg_gradient_workspace bytes   required */
} rsx_dpg_out;
int rsx_dpg_gradient_workspace(const rsx_sim* h, const rsx_policy_mlp* actor, const rsx_policy_mlp* critic, int n_critics,
                               int64_t n_rows, int max_workgroups, int64_t* bytes_out);
int rsx_task_dpg_gradient(rsx_sim* h, const rsx_policy_mlp* actor, const float* actor_params_dev, const float* target_actor_params_dev,
                          const rsx_policy_mlp* critic, const float* critic_params_dev, const float* target_critic_params_dev,
                          const rsx_dpg_in* in, const rsx_dpg_cfg* cfg, const rsx_dpg_out* out, void* stream);

/* ---- soft actor-critic loss gradients of a squashed Gaussian actor, one or two Q critics and the temperature (additive extension of ABI 6) ----
 * rsx_task_dpg_gradient's counterpart for SAC: the handle, the transitions, `rows` and the critics are that call's (rsx_dpg_in is reused as
 * it is: repeats allowed, NULL = rows 0 .. M - 1, an index outside [0, N) contributes nothing, is counted in stats[11] and nothing outside
 * the arrays is read for it, the divisor stays M).  There is no target actor.
 *   actor            the policy of rsx_task_collect_gaussian: out_act = RSX_ACT_NONE, an output layer of 2 * act_dim units (rows [0, AD)
 *                    the mean, rows [AD, 2 AD) the raw log-std), actor_params_dev [Pa]; the head is the one stated there.
 *   log_alpha_dev    [1] f32 on the device; alpha = exp(*log_alpha_dev) (that section's exp), read when the launches run.
 * The losses; t is an entry's POSITION in the minibatch, a mean is the sum over the M entries times the float32 1 / M:
 *   eps', eps        the collector's standard-normal recipe under domain word 12 (eps', on next_obs) and 13 (eps, on obs), the next two
 *                    free ones (1 and 3 .. 11 are taken): counter (t, noise_step >> 32, noise_step & 0xFFFFFFFF, dom | (k >> 2) << 8), key =
 *                    noise_seed (lo, hi); component k takes normal k & 3 of its block.  noise_step as in rsx_dpg_cfg.
 *   a', logp'        head(actor(next_obs), eps')                                       no gradient
 *   y                terminated ? reward : reward + gamma * (min_c Q_targ_c(next_obs, a') - alpha * logp')
 *   L_q              sum over c of 0.5 * mean((Q_c(obs, action) - y)^2): grad_critics[c]
 *   a~, logp         head(actor(obs), eps)
 *   L_pi             mean(alpha * logp - min_c Q_c(obs, a~)): grad_actor.  Both critics are differentiated with respect to their action
 *                    inputs, not their weights; per entry the critic that gives the minimum passes its dQ/da, on an exact tie critic 0.
 *                    The gradient flows through tanh, the reparameterisation (eps a constant) and the log-std clamp into all 2 AD output
 *                    rows:  dL/du_k = (alpha * 2 a_k - dQ/da_k * (1 - a_k^2)) / M  with 1 - a_k^2 computed as fmaf(-a_k, a_k, 1);
 *                    dL/dmu_k = dL/du_k;  dL/dls_k = dL/du_k * (sigma_k * eps_k) - alpha / M;  dL/draw_k = dL/dls_k where
 *                    log_std_min <= raw_k <= log_std_max (bounds included, as torch.clamp), else 0.  alpha and y carry no gradient.
 *   L_alpha          -log_alpha * mean(logp + target_entropy): grad_log_alpha[0] = -mean(logp + target_entropy)
 *   log1p            on [0, 1]: w = fl(1 + y), d = w - 1 (exact), log2(w) * ln 2 * (y / d) on the hardware's log2 and reciprocal, y itself
 *                    when d == 0.  Absolute error below 3e-7.  logp sums its AD terms in ascending k.
 * Forwards are rsx_policy_mlp's arithmetic bit for bit, so out->mean and out->log_std equal what rsx_task_collect_gaussian records for
 * the same observation.  Backward: rsx_task_dpg_gradient's rules, word for word (blocks of 64 entries, G = min(ceil(M / 64),
 * max_workgroups) workgroups with default cap 256, one fmaf chain per workgroup for a weight gradient — the f32 MFMA for the hidden
 * layers —, float64 block sums rounded once for bias gradients, dz and dQ/da as four interleaved chains combined (s0 + s1) + (s2 + s3),
 * per-workgroup partials added in workgroup order from 0, stats per lane, then over the lanes, then over the workgroups; no float
 * atomics).  The result bits are a function of the inputs and of G alone.
 * Six launches: (1) the targets — the actor and the C target critics in one workgroup's LDS; (2) the critics' gradients, grid.y = critic;
 * (3) the actor's sample a~, logp into the workspace; (4) each critic on (obs, a~) with its dQ/da, grid.y = critic; (5) the actor's
 * backward pass with the selected dQ/da; (6) the reduce.  The actor and the online critics never share a workgroup's LDS.  LDS per
 * workgroup at the largest shape (2 x 64 units, OD = 64, AD = 5, C = 2): targets 129 568 B, critic 63 344 B, sample 55 616 B,
 * critic-on-sample 54 640 B, actor 67 136 B.  A shape that needs more than 163 840 B in a launch is refused with the byte count in the
 * error string.  No kernel uses scratch memory.
 *   stats            [12]: 0 / 1 L_q of critic 0 / 1 (0 for an absent critic), 2 / 3 mean Q_0 / Q_1 (obs, action), 4 L_pi, 5 L_alpha,
 *                    6 mean y, 7 mean logp, 8 mean logp', 9 alpha, 10 entries used, 11 entries skipped
 *   per entry        optional, 0 for a skipped entry: target [M]; q [C][M]; action [M][AD] = a~; log_prob [M]; next_log_prob [M];
 *                    eps, next_eps, mean, log_std [M][AD]
 *   workspace        at least rsx_sac_gradient_workspace bytes, 16-byte aligned; its contents before the call do not matter
 * Stream-ordered, never synchronises, never allocates, capturable; a replayed graph draws fresh noise when noise_step_dev's counter was
 * advanced.  Refusals (nothing is enqueued), all RSX_ERR_ARG: rsx_task_dpg_gradient's, and a null log_alpha_dev, grad_actor or
 * grad_log_alpha, a non-finite target_entropy, log-std bounds that are not finite or not ordered, an actor whose out_act is not
 * RSX_ACT_NONE. */
typedef struct rsx_sac_cfg {
    const int64_t* noise_step_dev;  /* NULL: noise_step; else the device address of the step */
    uint64_t       noise_seed;
    int64_t        noise_step;
    float          gamma;           /* in [0, 1] */
    float          target_entropy;  /* finite; SAC's usual choice is -act_dim */
    float          log_std_min;
    float          log_std_max;
    int32_t        n_critics;       /* 1 or 2 */
    int32_t        max_workgroups;  /* 0 = the build's default; > 0 caps the grid */
} rsx_sac_cfg;
typedef struct rsx_sac_out {
    float* grad_actor;      /* [Pa]      required */
    float* grad_critics;    /* [C][Pc]   required */
    float* grad_log_alpha;  /* [1]       required */
    float* stats;           /* [12]      required */
    float* target;          /* [M] or NULL */
    float* q;               /* [C][M] or NULL */
    float* action;          /* [M][act_dim] or NULL */
    float* log_prob;        /* [M] or NULL */
    float* next_log_prob;   /* [M] or NULL */
    float* eps;             /* [M][act_dim] or NULL */
    float* next_eps;        /* [M][act_dim] or NULL */
    float* mean;            /* [M][act_dim] or NULL */
    float* log_std;         /* [M][act_dim] or NULL */
    void*  workspace;       /* rsx_sac_gradient_workspace bytes   required */
} rsx_sac_out;
int rsx_sac_gradient_workspace(const rsx_sim* h, const rsx_policy_mlp* actor, const rsx_policy_mlp* critic, int n_critics,
                               int64_t n_rows, int max_workgroups, int64_t* bytes_out);
int rsx_task_sac_gradient(rsx_sim* h, const rsx_policy_mlp* actor, const float* actor_params_dev,
                          const rsx_policy_mlp* critic, const float* critic_params_dev, const float* target_critic_params_dev,
                          const float* log_alpha_dev /* [1] */, const rsx_dpg_in* in, const rsx_sac_cfg* cfg,
                          const rsx_sac_out* out, void* stream);

/* ---- the TD3 / DDPG update phase on the device: sample, Adam, Polyak (additive extension of ABI 6) ---------------------------------
 * What an off-policy trainer does around rsx_task_dpg_gradient, per gradient step: draw the minibatch's rows, clip and step the critics
 * (and, every policy_delay-th step, the actor) with Adam, and move the targets — here stream-ordered and keyed by counters that live on
 * the device, so that rsx_task_collect_policy + the ring's writes + rsx_task_dpg_update captured once is one whole off-policy iteration
 * per replay.  rsx_replay_sample_rows and rsx_dpg_adam_step take no handle: they run on the thread's current device.  Every call is
 * stream-ordered, never synchronises, never allocates and is capturable; invalid arguments are refused with RSX_ERR_ARG before anything
 * is enqueued (rsx_last_error says why); no float atomics: the result bits are a function of the inputs (and, for rsx_task_dpg_update,
 * of max_workgroups) alone.
 *
 * rsx_replay_sample_rows:  rows_dev [m] int32 := indices uniform over the first `fill` rows of a ring of n_batch_rows rows, with
 * repeats, every entry computed on its own from (seed, step, t) — no generator state, no floating point.  One launch.
 *   word     entry t takes word t & 3 of philox4x32-7(counter = (t >> 2, step >> 32, step & 0xFFFFFFFF, 11), key = (seed lo, seed hi));
 *            11 is this draw's own domain word (1 and 3 .. 10 are the engine's other draws)
 *   rows[t]  (uint32_t)(((uint64_t)word * (uint64_t)fill) >> 32): exact integer arithmetic.  Of the 2^32 words, floor(2^32 / fill) or
 *            one more map to each index, so every index has a probability within 2^-32 of 1 / fill.  A draw depends on (seed, step, t)
 *            and fill — not on m, the grid or the device.
 *   fill     the argument, or, with fill_dev != NULL, the int64 it points to, read on the device when the launch runs (the ring's own
 *            fill count); either is clamped to [0, n_batch_rows].  fill == 0 writes -1 to every entry: rsx_task_dpg_gradient skips
 *            such an entry and counts it.
 *   step     the argument, or, with step_dev != NULL, the int64 it points to, read on the device: pass
 *            rsx_dpg_adam_state.counters + RSX_DPG_STEPS and a replayed graph draws new rows once the counter has advanced.
 * Refused: a null rows_dev; m < 1 or m > 2^31 - 1; n_batch_rows < 1 or > 2^31 - 1; a negative `fill` argument (with fill_dev == NULL). */
int rsx_replay_sample_rows(int32_t* rows_dev, int64_t m, int64_t n_batch_rows, int64_t fill, const int64_t* fill_dev, uint64_t seed,
                           int64_t step, const int64_t* step_dev, void* stream);
/* rsx_dpg_adam_step:  the optimiser step of TD3 — two torch.optim.Adam (no amsgrad, no weight decay), one on the critics' flat tensor
 * [C * Pc] and one on the actor's [Pa], each behind its own torch.nn.utils.clip_grad_norm_, and the Polyak step of the two target
 * tensors — in two launches (the norms, then the update).
 *   counters   int64 [4] device memory, part of the optimiser state (zero at the start of training): */
#define RSX_DPG_T_CRITIC 0   /* the critics' Adam step count t */
#define RSX_DPG_T_ACTOR  1   /* the actor's: it advances on actor steps only, so its bias corrections are its own */
#define RSX_DPG_STEPS    2   /* gradient steps finished (calls of rsx_dpg_adam_step): the key of the row draws and the smoothing noise */
#define RSX_DPG_SPARE    3   /* not read, not written */
/*   groups   the critics always step; the actor steps when io->grad_actor != NULL.  A call without grad_actor leaves the actor's
 *          parameters, its moments and counters[RSX_DPG_T_ACTOR] exactly as they were.
 *   per group, rsx_adam_step's arithmetic, word for word, on that group's tensor alone:
 *     norm   = (float)sqrt(sum g^2), the float64 reduction in rsx_adam_step's fixed order (G = min(ceil(n / 256), 64) workgroups of the
 *              GROUP's n; each g widened, g * g exact)
 *     coef   = min(1, max_grad_norm / (norm + 1e-6f)) in float32;  max_grad_norm <= 0: coef = 1 (no clipping)
 *     t := t + 1 (the group's own);  bc1 = 1 - beta1^t, bc2 = 1 - beta2^t in float64 from the device's t, beta^t by squaring
 *     g' = g * coef;   m = b1 * m + omb1 * g';   v = b2 * v + (omb2 * g') * g';   p = p - step * (m / (sqrtf(v) / s2 + eps))
 *              in float32, every operation rounded, with b = (float)beta, omb = (float)(1.0 - beta), step = (float)((double)lr / bc1),
 *              s2 = (float)sqrt(bc2).  A gradient entry that is 0 while its m is 0 leaves its parameter as it was.
 *     lr     the group's: lr_actor / lr_critic, or with the matching *_dev != NULL the float it points to, read on the device.
 *   Polyak   with io->update_targets != 0, after the Adam step of the same call, on the NEW parameters, per entry of both target
 *          tensors:  d = p - targ;  targ = targ + tau * d   in float32, each of the three operations rounded.  Without a grad_actor
 *          the actor's target moves towards the unchanged actor.  With update_targets == 0 no target is read or written.
 *   counters[RSX_DPG_STEPS] advances by one per call.
 *   stats  [3] or NULL: the critics' norm before the clip; the actor's (0.0f without an actor step); 1.0f when the targets moved,
 *          else 0.0f.
 *   workspace   RSX_DPG_ADAM_WORKSPACE_BYTES, 8-byte aligned.
 * Refused: a null cfg, st, io, counters, workspace, critic array (parameters, gradient, m, v) or actor array (parameters, m, v); a
 * size < 1 or above 2^31 - 1; lr_actor, lr_critic or eps negative or non-finite; a beta outside [0, 1); max_grad_norm non-finite; tau
 * outside [0, 1] or non-finite; update_targets != 0 with a null target. */
#define RSX_DPG_ADAM_WORKSPACE_BYTES 2048
typedef struct rsx_dpg_adam_cfg {
    double       beta1;          /* in [0, 1) */
    double       beta2;          /* in [0, 1) */
    const float* lr_actor_dev;   /* [1] device memory, or NULL = lr_actor */
    const float* lr_critic_dev;  /* [1] device memory, or NULL = lr_critic */
    float        lr_actor;       /* >= 0, finite */
    float        lr_critic;      /* >= 0, finite */
    float        eps;            /* >= 0, finite */
    float        max_grad_norm;  /* <= 0: no clipping; else the bound of EACH group's own norm */
    float        tau;            /* in [0, 1] */
} rsx_dpg_adam_cfg;
typedef struct rsx_dpg_adam_state {
    float*   m_actor;     /* [n_actor] */
    float*   v_actor;
    float*   m_critic;    /* [n_critic] */
    float*   v_critic;
    int64_t* counters;    /* [4], RSX_DPG_* */
    int64_t  n_actor;     /* Pa */
    int64_t  n_critic;    /* C * Pc */
} rsx_dpg_adam_state;
typedef struct rsx_dpg_adam_io {
    float*       actor_params;          /* [n_actor]   updated in place on an actor step   required */
    float*       target_actor_params;   /* [n_actor]   required with update_targets */
    float*       critic_params;         /* [n_critic]  updated in place   required */
    float*       target_critic_params;  /* [n_critic]  required with update_targets */
    const float* grad_actor;            /* [n_actor] or NULL: no actor step */
    const float* grad_critic;           /* [n_critic]  required */
    float*       stats;                 /* [3] or NULL */
    void*        workspace;             /* RSX_DPG_ADAM_WORKSPACE_BYTES   required */
    int32_t      update_targets;        /* != 0: the Polyak step */
} rsx_dpg_adam_io;
int rsx_dpg_adam_step(const rsx_dpg_adam_cfg* cfg, const rsx_dpg_adam_state* st, const rsx_dpg_adam_io* io, void* stream);
/* rsx_task_dpg_update:  the whole update phase in one call.  For j = 0 .. grad_steps - 1 it enqueues, in this order:
 * rsx_replay_sample_rows(m = in->n_rows, n_batch_rows = in->n_batch_rows, fill / fill_dev = u's, seed = u->seed, step_dev = the DEVICE's
 * counters[RSX_DPG_STEPS]) into the workspace;  rsx_task_dpg_gradient on those rows with noise_step_dev = the same counter
 * (cfg->noise_step and cfg->noise_step_dev are ignored) and grad_actor only on an actor step;  rsx_dpg_adam_step with grad_actor and
 * update_targets on an actor step only.  Step j is an actor step when (j + 1) % policy_delay == 0 — decided on the host from the index;
 * grad_steps must be a multiple of policy_delay, so every call has the same launch sequence, a captured call replays exactly what
 * an eager one does, and no launch is wasted.  policy_delay = 1, one critic and sigma = 0 is DDPG.  The results equal that sequence of
 * calls bit for bit.
 *   the handle, actor, critic, in, cfg    as for rsx_task_dpg_gradient; in->rows must be NULL, in->n_rows is the minibatch size m.
 *   the four parameter tensors   updated in place.  Nothing `in` points to is written.
 *   stats_dev   [grad_steps][RSX_DPG_UPDATE_STATS]: rsx_task_dpg_gradient's nine, then rsx_dpg_adam_step's three
 *   workspace   rsx_dpg_update_workspace bytes, 16-byte aligned: rsx_task_dpg_gradient's for m rows, the rows, the two gradient tensors
 *               and the optimiser's partials.  rows_offset_out (or NULL): where in it the int32 rows [m] of the last step lie.
 *   an empty ring   with a device fill of 0 every row is -1 and skipped, every gradient is 0, and no PARAMETER moves (a zero gradient on
 *               a zero moment leaves its parameter alone; with moments from earlier steps Adam goes on as torch's would); the counters
 *               advance and the targets take their Polyak steps as always.
 * Refused: everything rsx_replay_sample_rows, rsx_task_dpg_gradient and rsx_dpg_adam_step refuse; a null u, stats_dev or workspace; a
 * non-NULL in->rows; grad_steps < 1; policy_delay < 1; grad_steps % policy_delay != 0; a negative u->fill with fill_dev == NULL; state
 * sizes (st->n_actor, st->n_critic) that are not Pa and C * Pc. */
#define RSX_DPG_UPDATE_STATS 12
typedef struct rsx_dpg_update_cfg {
    const int64_t* fill_dev;      /* the ring's fill count on the device, or NULL = fill */
    uint64_t       seed;          /* the row draws' key */
    int64_t        fill;          /* >= 0 */
    int32_t        grad_steps;    /* >= 1, a multiple of policy_delay */
    int32_t        policy_delay;  /* >= 1 */
} rsx_dpg_update_cfg;
int rsx_dpg_update_workspace(const rsx_sim* h, const rsx_policy_mlp* actor, const rsx_policy_mlp* critic, int n_critics, int64_t n_rows,
                             int max_workgroups, int64_t* bytes_out, int64_t* rows_offset_out);
int rsx_task_dpg_update(rsx_sim* h, const rsx_policy_mlp* actor, float* actor_params_dev, float* target_actor_params_dev,
                        const rsx_policy_mlp* critic, float* critic_params_dev, float* target_critic_params_dev, const rsx_dpg_in* in,
                        const rsx_dpg_cfg* cfg, const rsx_dpg_update_cfg* u, const rsx_dpg_adam_cfg* adam, const rsx_dpg_adam_state* st,
                        float* stats_dev, void* workspace, void* stream);

/* ---- the soft actor-critic update phase on the device: sample, Adam, alpha, Polyak (additive extension of ABI 6) --------------------
 * What a SAC trainer does around rsx_task_sac_gradient, per gradient step: draw the minibatch's rows, clip and step the critics and the
 * actor with Adam, step the log-temperature, and move the target critics — the TD3 section's twin, stream-ordered and keyed by counters
 * that live on the device, so that rsx_task_collect_gaussian + the ring's writes + rsx_task_sac_update captured once is one whole
 * off-policy iteration per replay.  rsx_sac_adam_step takes no handle: it runs on the thread's current device.  Every call is
 * stream-ordered, never synchronises, never allocates and is capturable; invalid arguments are refused with RSX_ERR_ARG before anything
 * is enqueued (rsx_last_error says why); no float atomics: the result bits are a function of the inputs (and, for rsx_task_sac_update,
 * of max_workgroups) alone.  The rows are rsx_replay_sample_rows' (domain word 11); this phase draws nothing else of its own.
 *
 * rsx_sac_adam_step:  the optimiser step of SAC — three torch.optim.Adam (no amsgrad, no weight decay), one on the critics' flat tensor
 * [C * Pc], one on the actor's [Pa] and one on log_alpha [1], the first two each behind its own torch.nn.utils.clip_grad_norm_, and the
 * Polyak step of the target critics — in two launches (the norms, then the update).  There is no target actor.
 *   counters   int64 [4] device memory, part of the optimiser state (zero at the start of training): */
#define RSX_SAC_T_CRITIC 0   /* the critics' Adam step count t */
#define RSX_SAC_T_ACTOR  1   /* the actor's: it advances on steps with a grad_actor only */
#define RSX_SAC_T_ALPHA  2   /* log_alpha's: it advances on steps with a grad_log_alpha only */
#define RSX_SAC_STEPS    3   /* gradient steps finished (calls of rsx_sac_adam_step): the key of the row draws and the sampling noise */
/*   groups   the critics always step.  The actor steps when io->grad_actor != NULL; a call without it leaves the actor's parameters,
 *          its moments and counters[RSX_SAC_T_ACTOR] exactly as they were.  log_alpha steps when io->grad_log_alpha != NULL; a call
 *          without it (a fixed temperature) leaves log_alpha, m_alpha, v_alpha and counters[RSX_SAC_T_ALPHA] exactly as they were.
 *   per group, rsx_dpg_adam_step's arithmetic — rsx_adam_step's — word for word, on that group's tensor alone:
 *     norm   = (float)sqrt(sum g^2), the float64 reduction in rsx_adam_step's fixed order (G = min(ceil(n / 256), 64) workgroups of the
 *              GROUP's n; each g widened, g * g exact); the critics and the actor only
 *     coef   = min(1, max_grad_norm / (norm + 1e-6f)) in float32;  max_grad_norm <= 0: coef = 1 (no clipping).  log_alpha is never
 *              clipped: its coef is 1 whatever the other groups' norms are
 *     t := t + 1 (the group's own);  bc1 = 1 - beta1^t, bc2 = 1 - beta2^t in float64 from the device's t, beta^t by squaring
 *     g' = g * coef;   m = b1 * m + omb1 * g';   v = b2 * v + (omb2 * g') * g';   p = p - step * (m / (sqrtf(v) / s2 + eps))
 *              in float32, every operation rounded, with b = (float)beta, omb = (float)(1.0 - beta), step = (float)((double)lr / bc1),
 *              s2 = (float)sqrt(bc2).  A gradient entry that is 0 (of either sign) while its m is 0 leaves its parameter as it was.
 *     lr     the group's: lr_critic / lr_actor / lr_alpha, or with the matching *_dev != NULL the float it points to, read on the device.
 *   Polyak   with io->update_targets != 0, after the Adam step of the same call, on the NEW parameters, per entry of the target critics:
 *          d = p - targ;  targ = targ + tau * d   in float32, each of the three operations rounded.  With update_targets == 0 the
 *          targets are neither read nor written.
 *   counters[RSX_SAC_STEPS] advances by one per call.
 *   stats  [4] or NULL: the critics' norm before the clip; the actor's (0.0f without an actor step); log_alpha after the step; 1.0f
 *          when the targets moved, else 0.0f.
 *   workspace   RSX_SAC_ADAM_WORKSPACE_BYTES, 8-byte aligned.
 * Refused: a null cfg, st, io, counters, workspace, critic array (parameters, gradient, m, v), actor array (parameters, m, v) or
 * log_alpha, m_alpha, v_alpha; a size < 1 or above 2^31 - 1; lr_actor, lr_critic, lr_alpha or eps negative or non-finite; a beta
 * outside [0, 1); max_grad_norm non-finite; tau outside [0, 1] or non-finite; update_targets != 0 with a null target_critic_params. */
#define RSX_SAC_ADAM_WORKSPACE_BYTES 2048
typedef struct rsx_sac_adam_cfg {
    double       beta1;          /* in [0, 1) */
    double       beta2;          /* in [0, 1) */
    const float* lr_actor_dev;   /* [1] device memory, or NULL = lr_actor */
    const float* lr_critic_dev;  /* [1] device memory, or NULL = lr_critic */
    const float* lr_alpha_dev;   /* [1] device memory, or NULL = lr_alpha */
    float        lr_actor;       /* >= 0, finite */
    float        lr_critic;      /* >= 0, finite */
    float        lr_alpha;       /* >= 0, finite */
    float        eps;            /* >= 0, finite */
    float        max_grad_norm;  /* <= 0: no clipping; else the bound of the critics' norm and of the actor's, each on its own */
    float        tau;            /* in [0, 1] */
} rsx_sac_adam_cfg;
typedef struct rsx_sac_adam_state {
    float*   m_actor;     /* [n_actor] */
    float*   v_actor;
    float*   m_critic;    /* [n_critic] */
    float*   v_critic;
    float*   m_alpha;     /* [1] */
    float*   v_alpha;
    int64_t* counters;    /* [4], RSX_SAC_* */
    int64_t  n_actor;     /* Pa */
    int64_t  n_critic;    /* C * Pc */
} rsx_sac_adam_state;
typedef struct rsx_sac_adam_io {
    float*       actor_params;          /* [n_actor]   updated in place with a grad_actor   required */
    float*       critic_params;         /* [n_critic]  updated in place   required */
    float*       target_critic_params;  /* [n_critic]  required with update_targets */
    float*       log_alpha;             /* [1]         updated in place with a grad_log_alpha   required */
    const float* grad_actor;            /* [n_actor] or NULL: no actor step */
    const float* grad_critic;           /* [n_critic]  required */
    const float* grad_log_alpha;        /* [1] or NULL: a fixed temperature */
    float*       stats;                 /* [4] or NULL */
    void*        workspace;             /* RSX_SAC_ADAM_WORKSPACE_BYTES   required */
    int32_t      update_targets;        /* != 0: the Polyak step */
} rsx_sac_adam_io;
int rsx_sac_adam_step(const rsx_sac_adam_cfg* cfg, const rsx_sac_adam_state* st, const rsx_sac_adam_io* io, void* stream);
/* rsx_task_sac_update:  the whole update phase in one call.  For j = 0 .. grad_steps - 1 it enqueues, in this order:
 * rsx_replay_sample_rows(m = in->n_rows, n_batch_rows = in->n_batch_rows, fill / fill_dev = u's, seed = u->seed, step_dev = the DEVICE's
 * counters[RSX_SAC_STEPS]) into the workspace;  rsx_task_sac_gradient on those rows with noise_step_dev = the same counter
 * (cfg->noise_step and cfg->noise_step_dev are ignored; cfg->noise_seed keys the sampling noise);  rsx_sac_adam_step with
 * update_targets = 1, all three gradients when u->learn_alpha != 0 and without grad_log_alpha otherwise.  Every step is an actor step
 * and moves the targets, so every call — eager, captured or replayed — has the same launch sequence (nine launches per gradient step:
 * one row draw, the gradient's six, the optimiser's two).  The results equal that sequence of calls bit for bit.
 *   the handle, actor, critic, in, cfg    as for rsx_task_sac_gradient; in->rows must be NULL, in->n_rows is the minibatch size m.
 *   the four parameter tensors   actor, critics, target critics and log_alpha [1]: updated in place.  Nothing `in` points to is written.
 *   stats_dev   [grad_steps][RSX_SAC_UPDATE_STATS]: rsx_task_sac_gradient's twelve, then rsx_sac_adam_step's four
 *   workspace   rsx_sac_update_workspace bytes, 16-byte aligned: rsx_task_sac_gradient's for m rows, the rows, the three gradients and
 *               the optimiser's partials.  rows_offset_out (or NULL): where in it the int32 rows [m] of the last step lie.
 *   an empty ring   with a device fill of 0 every row is -1 and skipped; the critics' and the actor's gradients are +0 everywhere and
 *               rsx_task_sac_gradient's grad_log_alpha is -0.0f (minus a sum of nothing: skipped entries add neither logp nor
 *               target_entropy), which Adam treats as 0: no PARAMETER moves, log_alpha included (a zero gradient on a zero moment
 *               leaves its parameter alone; with moments from earlier steps Adam goes on as torch's would); the four counters
 *               advance and the target critics take their Polyak steps as always.
 * Refused: everything rsx_replay_sample_rows, rsx_task_sac_gradient and rsx_sac_adam_step refuse; a null u, stats_dev or workspace; a
 * non-NULL in->rows; grad_steps < 1; a negative u->fill with fill_dev == NULL; state sizes (st->n_actor, st->n_critic) that are not Pa
 * and C * Pc.
 * Not here: delayed actor or target steps, prioritised or n-step replay. */
#define RSX_SAC_UPDATE_STATS 16
typedef struct rsx_sac_update_cfg {
    const int64_t* fill_dev;      /* the ring's fill count on the device, or NULL = fill */
    uint64_t       seed;          /* the row draws' key */
    int64_t        fill;          /* >= 0 */
    int32_t        grad_steps;    /* >= 1 */
    int32_t        learn_alpha;   /* != 0: log_alpha is stepped; 0: a fixed temperature */
} rsx_sac_update_cfg;
int rsx_sac_update_workspace(const rsx_sim* h, const rsx_policy_mlp* actor, const rsx_policy_mlp* critic, int n_critics, int64_t n_rows,
                             int max_workgroups, int64_t* bytes_out, int64_t* rows_offset_out);
int rsx_task_sac_update(rsx_sim* h, const rsx_policy_mlp* actor, float* actor_params_dev, const rsx_policy_mlp* critic,
                        float* critic_params_dev, float* target_critic_params_dev, float* log_alpha_dev, const rsx_dpg_in* in,
                        const rsx_sac_cfg* cfg, const rsx_sac_update_cfg* u, const rsx_sac_adam_cfg* adam, const rsx_sac_adam_state* st,
                        float* stats_dev, void* workspace, void* stream);

/* ---- prioritised and n-step replay on the device (additive extension of ABI 6) --------------------------------------------------------
 * The ring of transitions that rsx_task_dpg_gradient and rsx_task_sac_gradient read, filled with n-step transitions and drawn from in
 * proportion to per-row priorities, with everything an off-policy trainer keeps around it on the device.  No call here takes a handle:
 * they run on the thread's current device.  Every call is stream-ordered, never synchronises, never allocates and is capturable; invalid
 * arguments are refused with RSX_ERR_ARG before anything is enqueued (rsx_last_error says why); no atomic on floating-point numbers: the
 * result bits are a function of the inputs alone; no kernel uses scratch memory.  The number of launches of a call depends on the
 * capacity only.
 *
 * rsx_replay_add_nstep:  folds a [T][B] batch, as rsx_task_collect_* records it with final_obs, into n-step transitions and writes them
 * into the ring at the device's write head, in one launch.  Row (t, b) lands at (head + t * B + b) % capacity (step-major); then head :=
 * (head + T * B) % capacity and fill := min(fill + T * B, capacity), on the device.  With done(s) = terminated[s][b] | truncated[s][b]:
 *   m            starts at 1 and grows by one while !done(t + m - 1) and m < n_step and t + m < T: a window never crosses an episode end
 *                or the end of the batch, so the tail rows of a batch get fewer steps and a larger discount
 *   reward       R = r[t];  g = gamma;  then for k = 1 .. m - 1:  R = R + g * r[t + k];  g = g * gamma   — float32, every operation
 *                rounded (no fused multiply-add), in this order
 *   discount     g after the loop: gamma^m as that running product (gamma itself for m = 1)
 *   terminated   terminated[t + m - 1][b] != 0
 *   next_obs     done(t + m - 1): final_obs[t + m - 1][b];  else t + m < T: obs[t + m][b];  else the batch's next_obs[b]
 *   obs, action  those of (t, b)
 * With n_step = 1 the obs, action, reward, next_obs and terminated bytes are what a one-step ring stores, and discount is gamma.
 *   ticket_dev   int32 [1] device memory, 0 before the first call and between calls (the workgroup that finishes last advances head and
 *                fill and clears it): RSX_REPLAY_STATE_TICKET of a state block will do.
 * Refused: a null batch, ring or member; T < 1, B < 1; T * B > capacity; capacity < 1 or > 2^31 - 1; obs_dim or act_dim < 1; n_step
 * outside 1 .. 16; gamma outside [0, 1] or not finite. */
typedef struct rsx_replay_batch {
    const float*   obs;         /* [T][B][obs_dim] */
    const float*   actions;     /* [T][B][act_dim] */
    const float*   reward;      /* [T][B] */
    const uint8_t* terminated;  /* [T][B] */
    const uint8_t* truncated;   /* [T][B] */
    const float*   final_obs;   /* [T][B][obs_dim] */
    const float*   next_obs;    /* [B][obs_dim] */
    int32_t        T;
    int32_t        B;
} rsx_replay_batch;
typedef struct rsx_replay_ring {
    float*   obs;         /* [capacity][obs_dim] */
    float*   actions;     /* [capacity][act_dim] */
    float*   reward;      /* [capacity] */
    float*   next_obs;    /* [capacity][obs_dim] */
    uint8_t* terminated;  /* [capacity] */
    float*   discount;    /* [capacity] */
    int64_t* head_dev;    /* [1] the next row to write */
    int64_t* fill_dev;    /* [1] rows that hold a transition */
    int32_t* ticket_dev;  /* [1] */
    int64_t  capacity;
    int32_t  obs_dim;
    int32_t  act_dim;
} rsx_replay_ring;
int rsx_replay_add_nstep(const rsx_replay_batch* batch, const rsx_replay_ring* ring, int n_step, float gamma, void* stream);
/* The sum structure over per-row priorities: a tree of fan-out 64 in one float32 array.
 *   levels   level 0 holds the capacity leaves, level l + 1 one node per 64 entries of level l, up to the first level above the leaves
 *            that has one node, the root (a capacity of 1 .. 64 has the leaves and the root).  Every level is padded to a multiple of 64
 *            floats; the padding stays 0.  Level l starts where level l - 1 ends.  rsx_replay_tree_geometry gives the floats of the
 *            whole array, the index `levels` of the root's level and each level's first float (offsets_out [8], -1 past the root).
 *   leaf     priority^alpha; a row behind the fill count holds 0 (the array starts zeroed and only rsx_replay_set_priorities writes it)
 *   node     ((c_0 + c_1) + c_2) + ... + c_63 over its 64 children in float32, from c_0, every addition rounded.  A node is always
 *            recomputed from its children, never adjusted by a difference, so the tree never drifts from its leaves.
 *   state    RSX_REPLAY_STATE_WORDS 32-bit words of device memory: */
#define RSX_REPLAY_STATE_MAX     0   /* f32: the running maximum leaf value; 1.0f at the start, it only grows */
#define RSX_REPLAY_STATE_WMAX    1   /* f32: the last draw's largest weight before the division */
#define RSX_REPLAY_STATE_SKIPPED 2   /* i32: entries of rsx_replay_set_priorities skipped for their index, since the state was zeroed */
#define RSX_REPLAY_STATE_TICKET  3   /* i32: rsx_replay_add_nstep's ticket */
#define RSX_REPLAY_STATE_WORDS   4
/* rsx_replay_set_priorities:  leaf[rows[t]] := (|td_error[t]| + eps)^alpha for the m entries, powf of the device's math library on
 * float32 (a NaN td_error counts as 0; the value is capped at FLT_MAX), and the running maximum is raised to the largest value written.
 * With td_error_dev == NULL the leaf gets the running maximum instead: what newly added rows get.  With rows_dev == NULL the rows are
 * the m rows behind the write head, (head - m + t) mod capacity with head read from head_dev on the device: rsx_replay_add_nstep
 * followed by this call with m = T * B and both NULL is a prioritised ring's add().
 *   skipped      an index outside [0, capacity) (-1 included) is skipped: nothing is read or written for it, and it is counted in
 *                state[RSX_REPLAY_STATE_SKIPPED]
 *   duplicates   where an index occurs more than once the largest value wins, so the result does not depend on the order
 *   launches     2 + levels: the touched leaves cleared; raised to their values (an integer maximum of the bit patterns, whose order is
 *                that of the values for floats >= 0); then per level, bottom up, every ancestor of a touched leaf recomputed
 * Refused: a null tree_dev or state_dev; rows_dev and head_dev both null; capacity < 1 or > 2^31 - 1; m < 1 or m > 2^31 - 1; m >
 * capacity with rows_dev == NULL; alpha or eps negative or not finite. */
int rsx_replay_tree_geometry(int64_t capacity, int64_t* floats_out, int32_t* levels_out, int64_t* offsets_out /* [8] or NULL */);
int rsx_replay_set_priorities(float* tree_dev, void* state_dev, int64_t capacity, const int32_t* rows_dev, const float* td_error_dev,
                              const int64_t* head_dev, int64_t m, float alpha, float eps, void* stream);
/* rsx_replay_sample_prioritized:  m stratified draws in proportion to the leaves, with their importance weights.
 *   word     entry t takes word t & 3 of philox4x32-7(counter = (t >> 2, step >> 32, step & 0xFFFFFFFF, 14), key = (seed lo, seed hi)):
 *            rsx_replay_sample_rows' counter shape under a domain word of its own, 14 (1 and 3 .. 13 are taken)
 *   target   u = total * ((t + word * 2^-32) / m) in float64, in this order; total is the root as a double
 *   descent  from the root down, at a node with children c_0 .. c_63 and the float32 running sums p_j = p_(j-1) + c_j (p_(-1) = 0, the
 *            node's own additions): the child is the smallest j with c_j > 0 and u < p_j (p_j widened); if there is none, the largest j
 *            with c_j > 0.  Then u := u - p_(j-1) in float64.  An entry therefore never returns a leaf that holds 0, even when rounding
 *            pushes u to the total or past a node's last child.
 *   weights  w_t = powf(((float)fill * leaf) / total, -beta) in float32, then divided by the largest w of the call's entries
 *            (a second launch; the largest is kept in state[RSX_REPLAY_STATE_WMAX])
 *   empty    with fill == 0 or a total that is not > 0, every index is -1 and every weight 0
 *   fill, step   as for rsx_replay_sample_rows (fill clamped to [0, capacity]);  beta: the argument, or with beta_dev != NULL the float it
 *            points to, read on the device, so a replayed graph anneals beta and draws anew
 *   launches 2, behind a 4-byte memset node that clears the largest weight
 * Refused: a null tree_dev, state_dev, rows_out or weights_out; capacity or m outside 1 .. 2^31 - 1; a negative fill with fill_dev ==
 * NULL; beta negative or not finite (with beta_dev == NULL). */
int rsx_replay_sample_prioritized(const float* tree_dev, void* state_dev, int64_t capacity, int64_t fill, const int64_t* fill_dev,
                                  int32_t* rows_out, float* weights_out, int64_t m, float beta, const float* beta_dev, uint64_t seed,
                                  int64_t step, const int64_t* step_dev, void* stream);
/* rsx_task_dpg_gradient_w, rsx_task_sac_gradient_w:  rsx_task_dpg_gradient and rsx_task_sac_gradient with per-row discounts, per-entry
 * importance weights and the per-entry TD error.  Every member of rsx_grad_per may be NULL, per == NULL is all three NULL, and with all
 * three NULL the call is the plain one, bit for bit (the plain entry points are these with per == NULL).
 *   discount   [N], by ROW: replaces cfg->gamma in the target, y = terminated ? r : r + discount[row] * (...); cfg->gamma is still checked
 *   weight     [M], by POSITION in the minibatch: scales the critic loss only.  dL_q/dQ_c = ((Q_c - y) * w_t) * (1 / M), in this order,
 *              so a weight of exactly 1 leaves the bits alone; stats L_q becomes 0.5 * mean(w (Q_c - y)^2), summed as (w_t * d) * d.
 *              The actor's loss and the temperature's stay unweighted.
 *   td_error   [M], out: max over c of |Q_c - y| from the per-entry q and target the call writes, 0 for a skipped entry; one more
 *              launch.  Needs out->q and out->target. */
typedef struct rsx_grad_per {
    const float* discount;  /* [N] or NULL */
    const float* weight;    /* [M] or NULL */
    float*       td_error;  /* [M] or NULL */
} rsx_grad_per;
int rsx_task_dpg_gradient_w(rsx_sim* h, const rsx_policy_mlp* actor, const float* actor_params_dev, const float* target_actor_params_dev,
                            const rsx_policy_mlp* critic, const float* critic_params_dev, const float* target_critic_params_dev,
                            const rsx_dpg_in* in, const rsx_dpg_cfg* cfg, const rsx_dpg_out* out, const rsx_grad_per* per, void* stream);
int rsx_task_sac_gradient_w(rsx_sim* h, const rsx_policy_mlp* actor, const float* actor_params_dev,
                            const rsx_policy_mlp* critic, const float* critic_params_dev, const float* target_critic_params_dev,
                            const float* log_alpha_dev /* [1] */, const rsx_dpg_in* in, const rsx_sac_cfg* cfg,
                            const rsx_sac_out* out, const rsx_grad_per* per, void* stream);

/* Debugging aid: number of non-finite floats in the state rows and, with a task attached, in the
 * observations, rewards and info rows.  Synchronises `stream`.  With RSX_DEBUG_FINITE=1 in the
 * environment every stepping call (rsx_step_dev, rsx_task_step, rsx_task_step_n, rsx_task_rollout, rsx_task_collect_policy)
 * runs this scan afterwards and returns RSX_ERR_STATE when it finds one (the reference has no such
 * guard: e.g. rsoccer_gym/vss/env_vss/vss_gym.py:298 divides by a distance that can be zero). */
int rsx_check_finite(rsx_sim* h, int64_t* n_bad, void* stream);

/* ---- checkpoint / resume of a fused run ----------------------------------------------------
 * (the reference cannot: robosim exposes no way to restore velocities, rsim.py:52-75, and its tasks keep their
 * episode state — OU noise, step counters, cumulative reward terms — in Python attributes.)
 * The blob holds every per-env buffer of the handle (state incl. the two internal rows, step / episode counters,
 * OU noise, cumulative info terms, last observation / reward / flags), the handle's step counter (the key of the
 * per-step random draws) and the metrics.  Loading it into a handle created with the same simulator kind, team
 * sizes, batch size and attached with the same task, seed and env_id_base makes every following step bit-identical
 * to what the saving handle would have produced — across kernel layouts (RSX_LAYOUT) and processes.  Host blob,
 * both calls synchronise `stream`. */
/* Handles switched by rsx_physics_enable: the blob also holds the parameter rows, the coefficient rows and the
 * randomisation ranges, and it loads only into another such handle (a blob of the other kind: RSX_ERR_ARG). */
int rsx_task_checkpoint_size(rsx_sim* h, size_t* bytes);
int rsx_task_checkpoint_save(rsx_sim* h, void* blob, size_t bytes, void* stream);
int rsx_task_checkpoint_load(rsx_sim* h, const void* blob, size_t bytes, void* stream);

/* metrics, int64[RSX_METRICS], accumulated on device since attach (payload of the multi-GPU
 * all-reduce): 0 env_steps, 1 episodes, 2 goals_for (blue), 3 goals_against (yellow),
 * 4 sum of episode returns in 2^-20 fixed point, 5 sum of episode lengths,
 * 6 truncated episodes, 7 reserved.  Synchronises `stream`. */
int rsx_read_metrics(rsx_sim* h, int64_t out[RSX_METRICS], void* stream);
/* Device-side readers of rsx_task_view.metrics (e.g. an RCCL all-reduce of the 64 bytes) call this
 * first: one tiny launch on `stream` that adds the step kernels' partial episode counters into
 * metrics[1..6].  (Atomics of a whole grid on one cache line serialise: at 10^6 envs they, not the
 * physics, set the step time.)  rsx_read_metrics does it itself. */
int rsx_metrics_fold(rsx_sim* h, void* stream);

/* ---- per-env physics parameters / domain randomisation (additive extension of ABI 6) ---------------------------
 * By default every env steps with the model constants of docs/PHYSICS.md section 3, compiled into the kernels.  A handle
 * switched by rsx_physics_enable carries one float32 value per env of each parameter below instead, and steps with kernels
 * that read them (always the lane-group layouts, "<L>-lanes-per-env" in rsx_task_layout, at any batch size; a handle
 * forced to RSX_LANES_PER_ENV=64 is refused).  Units and defaults are those of docs/PHYSICS.md section 3.
 * Valid values: masses > 0, restitutions in [0, 1], friction coefficients, rolling deceleration, spin deceleration and
 * acceleration limits >= 0, all finite; RSX_PHYS_A_LAT is a VSS parameter and stays 0 for the SSL class.
 * Values are rows [RSX_PHYS_PARAMS][num_envs].  The kernels use derived coefficients ([RSX_PHYS_COEFS][num_envs]: shares of
 * the impulse, 1 + e, per-sub-step velocity changes), computed in double and rounded to float by the same expressions as
 * the compiled-in constants; a value equal to the float32 rounding of its default stands for the exact default, so a
 * handle at its defaults steps bit for bit like one that never called rsx_physics_enable. */
#define RSX_PHYS_PARAMS   14
#define RSX_PHYS_M_ROBOT   0 /* kg */
#define RSX_PHYS_M_BALL    1 /* kg */
#define RSX_PHYS_E_RR      2 /* restitution robot - robot */
#define RSX_PHYS_E_RB      3 /* restitution robot - ball */
#define RSX_PHYS_E_WB      4 /* restitution wall - ball */
#define RSX_PHYS_E_WR      5 /* restitution wall - robot */
#define RSX_PHYS_MU_RR     6 /* Coulomb friction robot - robot */
#define RSX_PHYS_MU_RB     7 /* Coulomb friction robot - ball */
#define RSX_PHYS_MU_WB     8 /* Coulomb friction wall - ball */
#define RSX_PHYS_MU_G      9 /* rolling deceleration of the ball on the ground, m/s^2 */
#define RSX_PHYS_SPIN_DEC 10 /* spin deceleration of the ball, rad/s^2 */
#define RSX_PHYS_A_LIN    11 /* linear acceleration limit of a robot, m/s^2 */
#define RSX_PHYS_A_ANG    12 /* angular acceleration limit of a robot, rad/s^2 */
#define RSX_PHYS_A_LAT    13 /* VSS: lateral grip, m/s^2 (SSL: 0) */
#define RSX_PHYS_COEFS    18
#define RSX_PHYS_RAW       0 /* rsx_physics_get: the parameter rows */
#define RSX_PHYS_COEF      1 /* rsx_physics_get: the derived coefficient rows */
/* The defaults of a robot class (no device needed). */
int rsx_physics_defaults(int kind, float out[RSX_PHYS_PARAMS]);
/* The coefficients the kernels derive from one parameter set (no device needed); RSX_ERR_ARG for an invalid set. */
int rsx_physics_derive(int kind, int time_step_ms, const float raw[RSX_PHYS_PARAMS], float coef[RSX_PHYS_COEFS]);
/* Switch the handle to per-env physics, every env at the defaults.  Before or after rsx_task_attach, but before
 * rsx_task_enable_capture (RSX_ERR_STATE otherwise); synchronises `stream`.  Handles that never call it allocate nothing for it. */
int rsx_physics_enable(rsx_sim* h, void* stream);
/* values [RSX_PHYS_PARAMS][num_envs]: NaN = keep the env's current value; env_mask [num_envs] bytes or NULL = every env.
 * on_device = 0: both are host memory, checked here (RSX_ERR_ARG, nothing changed, for an invalid value); synchronises
 * `stream`.  on_device = 1:
 * both are device memory and the write is one kernel launch (capturable); an env with an invalid value keeps all of its
 * values and is counted in the handle's error word (rsx_physics_errors). */
int rsx_physics_set(rsx_sim* h, const float* values, int on_device, const uint8_t* env_mask, void* stream);
/* which = RSX_PHYS_RAW: out [RSX_PHYS_PARAMS][num_envs]; RSX_PHYS_COEF: out [RSX_PHYS_COEFS][num_envs].  Host memory;
 * synchronises `stream`. */
int rsx_physics_get(rsx_sim* h, int which, float* out, void* stream);
/* Domain randomisation: from the next episode start on (rsx_task_reset, rsx_task_reset_to, same-step auto-reset), the
 * parameters p of param_mask (bit p) are redrawn per env on the device as lo[p] + (hi[p] - lo[p]) * u01(x) in float32, x the
 * first word of philox4x32(counter = (env_id_base + env, episode, p, 5), key = seed), u01(x) = (x >> 8) * 2^-24 — independent of
 * batch size and sharding; the others keep their values.  param_mask = 0 switches it off.  lo / hi: host [RSX_PHYS_PARAMS]
 * (bits outside param_mask are ignored); RSX_ERR_ARG when lo > hi or either bound is invalid.  Stream-ordered. */
int rsx_physics_randomize(rsx_sim* h, const float* lo, const float* hi, uint32_t param_mask, void* stream);
/* envs refused by device-side rsx_physics_set calls since the last read (read and cleared; synchronises `stream`). */
int rsx_physics_errors(rsx_sim* h, int64_t* out, void* stream);

/* ---- trace evaluation for system identification (additive extension of ABI 6) --------------------------------------
 * A trace is one recorded run: frames [n_frames][state_dim + RSX_STATE_EXTRA_ROWS] (the rsx_get_state_full layout) and the
 * commands between them, cmds [n_frames - 1][N][C] (the rsx_step layout).  Evaluating it replays, in every env at once, the
 * recorded commands from an anchor frame with the env's own physics parameters and measures how far the bodies drift from the
 * recorded frames — the inner loop of fitting the parameters of docs/PHYSICS.md section 3 to another simulator. */
#define RSX_TRACE_TERMS 6   /* ball xy (m^2), ball v (m^2/s^2), robot xy, robot heading (rad^2, wrapped), robot v, robot omega */
/* Load a trace onto a physics-enabled raw handle (rsx_physics_enable, no task attached).  frames [n_frames][state_dim + 2] f64,
 * cmds [n_frames - 1][N][C] f64, anchors [n_anchors] int32 frame indices.  num_envs % n_anchors == 0: env e evaluates
 * candidate e / n_anchors from anchor e % n_anchors, with that env's physics row.  Host memory, converted to float32 once;
 * replaces a trace loaded before.  RSX_ERR_STATE: physics off or a task attached; RSX_ERR_ARG: n_frames < 2, n_anchors < 1,
 * num_envs % n_anchors != 0, an anchor outside [0, n_frames - 2] or a non-finite value.  Synchronises `stream`. */
int rsx_trace_load(rsx_sim* h, const double* frames, const double* cmds, int n_frames,
                   const int32_t* anchors, int n_anchors, void* stream);
/* One launch: every env starts from its anchor frame, steps `horizon` times with the trace's commands and accumulates the
 * squared deviation from the trace's frames.  loss_dev: device [RSX_TRACE_TERMS][num_envs] f32, dense.  Does not synchronise.
 * The final state of each env is left in the handle's state buffer, bit for bit what set_state(anchor frame) followed by
 * `horizon` rsx_step_dev calls with the trace's commands leaves there.  Terms are in SI units (converted from the wire format:
 * degrees -> rad), summed over steps 1..horizon and over bodies; SSL wheel speeds and infrared are not part of them.
 * RSX_ERR_STATE: physics off, a task attached or no trace loaded; RSX_ERR_ARG: horizon < 1, an anchor + horizon > n_frames - 1,
 * loss_dev null. */
int rsx_trace_eval(rsx_sim* h, int horizon, float* loss_dev, void* stream);

/* ---- batched rgb frames (additive extension of ABI 6) ----------------------------------------------------------------
 * render() of the base envs (vss_gym_base.py:108-181, ssl_gym_base.py:108-181) for a whole batch, on the device: frame i is the
 * top-down picture of one env's current state, uint8 rgb, drawn by the rules of rsoccer_amd/Render/raster.py (same window
 * geometry, same world -> pixel map px = x * scale + centre, no y flip, same drawing order: field, blue robots by id, yellow
 * robots, ball; each robot its body and then its heading mark).  The static field is drawn once per view on the host in double
 * precision and equals FieldRaster(view)._field byte for byte; the bodies are evaluated per pixel in float32.  One deliberate
 * difference: pixels of a body or a heading mark that fall outside the window are dropped (raster.py clamps the samples of a
 * heading mark onto the border). */
typedef struct rsx_render_view {   /* the keys of Render/raster.py's VSS_VIEW / SSL_VIEW, metres unless noted */
    double length, width, margin, circle, pen_len, pen_wid, goal_wid, goal_dep;
    double scale;                  /* pixels per metre */
    double robot, ball;            /* drawn radii */
    int32_t square;                /* 1: robots are rotated squares (VSS), 0: discs (SSL) */
} rsx_render_view;
/* The reference's fixed window of a robot class (raster.py: VSS_VIEW / SSL_VIEW).  No device needed. */
int rsx_render_view_reference(int kind, rsx_render_view* out);
/* Frame size of a view: width = int(length * scale + 2 * (margin * scale)), height likewise from `width`.  A view is valid when
 * every value is finite, scale > 0 and both sides are between 8 and 4096 pixels; RSX_ERR_ARG otherwise.  No device needed. */
int rsx_render_size(const rsx_render_view* v, int* width, int* height);
/* The static field image of a view, out_hwc [height][width][3] host memory.  No device needed. */
int rsx_render_field(const rsx_render_view* v, uint8_t* out_hwc);
/* Make `v` the view rsx_render draws (raw handles and handles with a task alike).  A view the handle has not been given before is
 * checked (RSX_ERR_ARG), its field drawn on the host and uploaded as a background template: that synchronises `stream` and is refused
 * inside a stream capture (RSX_ERR_STATE).  A view the handle was given before is only selected: no allocation, no copy, no
 * synchronisation.  Templates are never freed or moved before rsx_destroy — a captured rsx_render holds its view's template and
 * geometry in the graph, and keeps drawing THAT view on every replay, whatever rsx_render_open selects in between — so a handle takes
 * at most 16 different views (RSX_ERR_STATE beyond).  Handles that never call it allocate nothing for it. */
int rsx_render_open(rsx_sim* h, const rsx_render_view* v, void* stream);
/* One launch: n frames of the CURRENT state buffer (the one rsx_state_buffers reports as current) into out_dev — [n][H][W][3]
 * uint8, or [n][3][H][W] with channels_first != 0; dense, 16-byte aligned (RSX_ERR_ARG otherwise).  Frame i shows env
 * env_ids_dev[i] (device int32 [n]; NULL = envs 0..n-1, then n <= num_envs); any order, duplicates allowed.  An id outside
 * [0, num_envs) leaves its frame as the bare field and is counted (rsx_render_errors).  Stream-ordered, never synchronises, holds
 * no host state (capturable into a hipGraph); reads the state, writes nothing but out_dev.  RSX_ERR_STATE before rsx_render_open. */
int rsx_render(rsx_sim* h, const int32_t* env_ids_dev, int n, int channels_first, uint8_t* out_dev, void* stream);
/* frames with an out-of-range env id since the last read (read and cleared; synchronises `stream`). */
int rsx_render_errors(rsx_sim* h, int64_t* out, void* stream);

/* ---- transfer of running episodes between envs and handles (additive extension of ABI 6) --------------------------------
 * Branching: for i in 0..n-1, env src_ids_dev[i] of `src` is copied into env dst_ids_dev[i] of `dst`, on the device, in stream order
 * (what population methods, particle resampling, restarts from an archive of states and tree search need; the only other route is
 * rsx_task_checkpoint_save + _load of whole handles through the host).  A handle that is never stepped serves as a device-resident
 * bank of states; rsx_task_lookahead works on it unchanged.
 * What travels is everything per-env that the checkpoint blob carries: the state rows (the two internal rows included), every row of
 * the scalar arena (last reward, task scalar, episode return, step count, EPISODE ID, cumulative info terms, OU noise), the obs and
 * final_obs rows, the terminated and truncated bytes and, on physics-enabled handles, the env's parameter and coefficient rows.
 * What stays with the handle: metrics, the step counter, seed and env_id_base, the randomisation ranges, the rsx_task_reset_to mask,
 * the action buffer and the placement cache (which needs no invalidation: its entries are tagged by episode and are a pure function
 * of seed, global env id and episode).  The destination env continues the source's episode under the DESTINATION's random streams:
 * its per-step draws stay keyed by dst's seed, dst's global env id and dst's step counter; its next placement and physics redraw by
 * dst's seed and env id and the copied episode id.
 * The copy is exact and layout-independent: rsx_task_checkpoint_save of `dst` afterwards holds src's columns byte for byte, and the
 * task scalar that the one-lane-per-env VSS-v0 kernel does not keep in memory is written for the destination as the checkpoint
 * writes it — source and destination may be stepped by different kernel layouts and differ in row_stride (RSX_ROW_PAD) and num_envs.
 *   ids         device int32 [n]; NULL = the identity map 0..n-1 on that side (then n <= that handle's num_envs).  Source ids may
 *               repeat (broadcast).  Destination ids must be pairwise distinct — NOT checked: an env named twice receives an
 *               unspecified mixture of its sources.  A pair with either id outside its handle is skipped whole, before any access,
 *               and counted (rsx_task_transfer_errors).  n == 0 succeeds without a launch.
 *   dst != src  one launch; holds no host state, never synchronises, capturable on any handle (a captured launch keeps BOTH handles'
 *               buffer pointers: neither may be destroyed while the graph is replayed).
 *   dst == src  any map is defined, as if every read happened before every write (swaps, permutations, resampling under the identity
 *               destination): a gather launch into a staging buffer of n records owned by the handle, then a scatter launch.  The
 *               buffer only grows; a call that has to grow it synchronises `stream`, and inside a stream capture such a call is
 *               refused (RSX_ERR_STATE: make one eager call of that size first, as with a new view of rsx_render_open).  Handles that
 *               never make a same-handle transfer allocate nothing.
 * The caller orders earlier work of both handles before `stream`.  Refusals (nothing is enqueued): RSX_ERR_ARG for a null handle,
 * n < 0, n beyond num_envs of a NULL side, handles on different devices or handles that differ in simulator kind, task, team sizes,
 * field type, time step, max_episode_steps, physics model or in whether rsx_physics_enable was called; RSX_ERR_STATE when either
 * handle has no task attached or has not been reset yet.  Seeds and env_id_base may differ. */
int rsx_task_transfer(rsx_sim* dst, rsx_sim* src, const int32_t* dst_ids_dev, const int32_t* src_ids_dev, int n, void* stream);
/* pairs skipped by transfers INTO `dst` since the last read (read and cleared; synchronises `stream`). */
int rsx_task_transfer_errors(rsx_sim* dst, int64_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RSX_H */
