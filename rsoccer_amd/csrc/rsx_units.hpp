// rsx_units.hpp — what one translation unit of librsx_hip.so defines and another calls.  The defining unit includes this header
// too, so a signature that drifts is a compile error in that unit, not an undefined symbol when the library is loaded.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct rsx_render_view;   // include/rsx.h
struct rsx_collect_out;
struct rsx_collect_gaussian_cfg;
struct rsx_selfplay_out;
struct rsx_team_out;
struct rsx_adv_in;
struct rsx_adv_out;
struct rsx_ppo_in;
struct rsx_ppo_cfg;
struct rsx_ppo_out;
struct rsx_ppo_update_cfg;
struct rsx_dpg_in;
struct rsx_dpg_cfg;
struct rsx_dpg_out;
struct rsx_sac_cfg;
struct rsx_sac_out;
struct rsx_adam_cfg;
struct rsx_adam_state;
struct rsx_adam_io;
struct rsx_dpg_update_cfg;
struct rsx_dpg_adam_cfg;
struct rsx_dpg_adam_state;
struct rsx_dpg_adam_io;
struct rsx_sac_update_cfg;
struct rsx_sac_adam_cfg;
struct rsx_sac_adam_state;
struct rsx_sac_adam_io;
struct rsx_replay_batch;
struct rsx_replay_ring;
struct rsx_grad_per;

namespace rsx {

struct Params;
struct Buffers;

// rsx_lanes.hip: the lane-group kernels (8 / 16 / 32 / 64 lanes per env) of a handle with `L` lanes per env and kernels specialised for
// `NR` robots (rsx_params.hpp: specialised_robots; 0 = generic), `helpers` placement-helper workgroups behind the lane_grid tiles; and the utility kernels
// of the C-ABI (count of non-finite floats, metrics fold, device-side teleport, wire format <-> device layout, tick slots [from, to) :=
// value or := slot 0)
void launch_sim(const Params& P, const Buffers& b, int L, int NR, float* state_out, int rand_tick, hipStream_t s);
void launch_task(const Params& P, const Buffers& b, int L, int NR, int helpers, int n_steps, int mode, hipStream_t s);
void launch_count_nonfinite(const float* p, size_t n, unsigned long long* out, hipStream_t s);
void launch_fold_metrics(unsigned long long* metrics, unsigned long long* slots, hipStream_t s);
void launch_reset_dev(float* st, const float* ball, const float* blue, const float* yellow, const uint8_t* mask, int B, int S, int rows,
                      int rs, int nb, int ny, float r_ball, hipStream_t s);
void launch_wire_cmds_in(const double* wire, float* cmds, unsigned B, unsigned NC, unsigned S, hipStream_t s);
void launch_wire_state_out(const float* st, double* wire, unsigned B, unsigned rows, unsigned S, hipStream_t s);
void launch_tick_fill(uint32_t* slots, int from, int to, uint32_t value, int copy, hipStream_t s);
#ifdef RSX_TIMING
inline unsigned long long* g_dbg = nullptr;   // development builds: where the kernels' time stamps go (rsx_lanes.hip: rsx_dbg_set)
#endif
// rsx_epl.hip: the one-lane-per-env kernels (large batches) and the four-lanes-per-env kernel of the SSL 11v11 scrimmage task
// (single-step launches, n_steps = 1 | flags); *_grid: workgroups of those launches (the host sizes the per-workgroup tick slots
// from these: rsx_hot_args.hpp, step_tick)
void launch_vss_epl(bool rollout, const Params& P, const Buffers& b, int n_steps, hipStream_t s);
void launch_ssl_epl(int task, bool rollout, const Params& P, const Buffers& b, int n_steps, hipStream_t s);
void launch_ssl_quad(const Params& P, const Buffers& b, int n_steps, hipStream_t s);
int epl_grid(int num_envs);
int ssl_quad_grid(int num_envs);
// rsx_big.hip: the 32-lanes-per-env kernel of the scrimmage task built for large batches
void launch_scrimmage_big(bool rollout, const Params& P, const Buffers& b, int n_steps, hipStream_t s);
// rsx_pair.hip: the paired form of the VSS-v0 3v3 single step (8 lanes per env, literal coefficients; n_steps = 1 | flags): launch_task's
// grid with workgroups of two waves, a physics wave and a service wave (rsx_pair.hpp; chosen by rsx_layout.hpp: StepPlan::service_wave)
void launch_task_pair(const Params& P, const Buffers& b, int n_steps, hipStream_t s);
// rsx_phys.hip: the kernels of physics-enabled handles (rsx_physics_enable)
void launch_task_phys(const Params& P, const Buffers& b, int L, int NR, float* phys, int n_steps, int mode, hipStream_t s);
void launch_sim_phys(const Params& P, const Buffers& b, int L, int NR, float* phys, float* state_out, int rand_tick, hipStream_t s);
void launch_phys_init(float* blk, int B, int S, int kind, int ts_ms, hipStream_t s);
void launch_phys_set(float* blk, const float* vals, const uint8_t* mask, int B, int S, int vstride, hipStream_t s);
void launch_phys_ranges(float* blk, const float* lo, const float* hi, uint32_t mask, hipStream_t s);
// rsx_sysid.hip: trace evaluation (rsx_trace_eval)
void launch_trace_eval(const Params& P, int L, int NR, const float* phys, float* state, float* loss, const float* frames,
                       const float* cmds, const int32_t* anchors, int n_frames, int n_anchors, int horizon, hipStream_t s);
// rsx_plan.hip: exact lookahead over candidate action sequences (rsx_task_lookahead).  state / aux: the handle's buffers, read only;
// ticks: the step-counter slots of a device-keyed handle (slot 0 is read) or nullptr = P.tick_base; phys: the physics block or nullptr.
// lookahead_grid: workgroups of that launch
long long lookahead_grid(int L, int num_envs, int n_candidates);
void launch_task_lookahead(const Params& P, int L, int NR, const float* state, const float* aux, const uint32_t* ticks, const float* phys,
                           const float* actions, int n_candidates, int horizon, float gamma, float* returns, int32_t* steps,
                           uint8_t* flags, float* last_obs, hipStream_t s);
// rsx_plan_sampled.hip: the same with candidates drawn on the device (rsx_task_lookahead_sampled), those candidates written out
// (rsx_plan_candidates) and returns folded into a new plan (rsx_plan_update).  PlanSampler: rsx_plan_common.hpp; mean: [num_envs][H][act_dim]
// or nullptr = zeros; plan_flat_grid: workgroups of the two elementwise launches (n_candidates = 1 for the update)
struct PlanSampler;
void launch_task_lookahead_sampled(const Params& P, int L, int NR, const float* state, const float* aux, const uint32_t* ticks, const float* phys,
                                   const float* mean, const PlanSampler& S, int n_candidates, int horizon, float gamma, float* returns,
                                   int32_t* steps, uint8_t* flags, float* last_obs, hipStream_t s);
long long plan_flat_grid(int num_envs, int n_candidates, int horizon, int nblk);
void launch_plan_candidates(const Params& P, const uint32_t* ticks, const float* mean, const PlanSampler& S, int n_candidates, int horizon,
                            int act_dim, float* out, hipStream_t s);
void launch_plan_update(const Params& P, const uint32_t* ticks, const float* mean, const PlanSampler& S, int n_candidates, int horizon,
                        int act_dim, const float* returns, float temperature, float* new_mean, int32_t* best, hipStream_t s);
// rsx_policy.hip: the lookahead with each step's action computed by an MLP policy from the observation the pair just produced
// (rsx_task_lookahead_policy).  PolicySpec: rsx_policy_mlp, checked; params: [n_policies][n_params]; obs: the handle's obs buffer, read
// only; actions_out / obs_out: optional.  policy_lds_bytes: LDS of one workgroup of that launch (the host refuses more than 64 KB)
struct PolicySpec { int layers, hidden, hidden_act, out_act; };
long long policy_lds_bytes(int L, int obs_dim, int act_dim, const PolicySpec& p);
void launch_task_lookahead_policy(const Params& P, int L, int NR, const float* state, const float* aux, const float* obs, const uint32_t* ticks,
                                  const float* phys, const PolicySpec& p, const float* params, int n_params, int act_dim, int n_policies,
                                  int horizon, float gamma, float* returns, int32_t* steps, uint8_t* flags, float* last_obs,
                                  float* actions_out, float* obs_out, hipStream_t s);
// rsx_collect.hip: on-policy collection (rsx_task_collect_policy): n_steps fused steps with auto-reset in one launch on the handle's own
// buffers `b` (as a rollout: state, scalars, obs, flags, metrics and the tick slots of the lane_grid workgroups are advanced), each step's
// action computed by the policy (one parameter vector [n_params]) and, with sigma [act_dim] non-null, perturbed by Gaussian noise keyed by
// noise_seed.  obs / actions / rewards / flags: the [n_steps][num_envs] record; final_obs / mean / sample: optional.  LDS: policy_lds_bytes
void launch_task_collect_policy(const Params& P, const Buffers& b, int L, int NR, float* phys, const PolicySpec& p, const float* params,
                                int n_params, int act_dim, const float* sigma, uint64_t noise_seed, int n_steps, float* obs, float* actions,
                                float* rewards, uint8_t* flags, float* final_obs, float* mean, float* sample, hipStream_t s);
// rsx_collect_gaussian.hip: the same collection under a state-dependent tanh-squashed Gaussian head (rsx_task_collect_gaussian): params
// [n_params] with an output layer of 2 * act_dim units; cfg and out checked; log_std_out optional.  gaussian_lds_bytes: LDS of one
// workgroup of that launch (Shared<L> and the wider image: the host refuses more than 64 KB)
long long gaussian_lds_bytes(int L, int obs_dim, int act_dim, const PolicySpec& p);
void launch_task_collect_gaussian(const Params& P, const Buffers& b, int L, int NR, float* phys, const PolicySpec& p, const float* params,
                                  int n_params, int act_dim, const rsx_collect_gaussian_cfg& cfg, int n_steps, const rsx_collect_out& out,
                                  float* log_std_out, hipStream_t s);
// rsx_selfplay.hip: the same collection for VSS-v0 with yellow robot 0 driven by a second policy, the opponent, from the mirrored observation
// (rsx_task_collect_selfplay).  p / params / sigma: the agent's, as above; opp / opp_params / opp_sigma: the opponent's (a shape of its own);
// out: the agent's record, checked; sp: the opponent's, every member optional.  selfplay_lds_bytes: LDS of one workgroup of that launch
// (Shared<L> and both images: the host refuses more than a CU's 160 KB; beyond 64 KB the launch raises the kernel's limit itself)
long long selfplay_lds_bytes(int L, int obs_dim, int act_dim, const PolicySpec& agent, const PolicySpec& opponent);
void launch_task_collect_selfplay(const Params& P, const Buffers& b, int L, int NR, float* phys, const PolicySpec& p, const float* params,
                                  int n_params, const PolicySpec& opp, const float* opp_params, int n_opp_params, int act_dim,
                                  const float* sigma, const float* opp_sigma, uint64_t noise_seed, int n_steps, const rsx_collect_out& out,
                                  const rsx_selfplay_out& sp, hipStream_t s);
// rsx_teamplay.hip: the same collection with every robot of a side driven by that side's policy (rsx_task_collect_team).  seats: 1 or
// n_blue blue robots under p / params / sigma; opp_seats: 0 (opp is null: no opponent), 1 or n_yellow yellow robots under opp / opp_params /
// opp_sigma; out: both sides' records with a seat axis, checked.  team_lds_bytes: LDS of one workgroup of that launch (Shared<L> and one
// image per side, the action slot sized for n_blue seats: the host refuses more than a CU's 160 KB)
long long team_lds_bytes(int L, int obs_dim, int act_dim, int n_blue, const PolicySpec& agent, const PolicySpec* opponent);
void launch_task_collect_team(const Params& P, const Buffers& b, int L, int NR, float* phys, const PolicySpec& p, const float* params,
                              int n_params, const float* sigma, int seats, const PolicySpec* opp, const float* opp_params, int n_opp_params,
                              const float* opp_sigma, int opp_seats, int act_dim, uint64_t noise_seed, int n_steps, const rsx_team_out& out,
                              hipStream_t s);
// rsx_match.hip: the policy lookahead with an opponent (rsx_task_lookahead_match): pair (env, k, m) under actor k of params [n_actors][n_params]
// and opponent m of opp_params [n_opponents][n_opp_params], seats / opp_seats robots of a side seated; state / aux / obs / ticks / phys as for
// launch_task_lookahead_policy, read only; out: the call's arrays, checked.  match_lds_bytes: LDS of one workgroup of that launch
// (team_lds_bytes with both sides seated: the host refuses more than a CU's 160 KB)
long long match_lds_bytes(int L, int obs_dim, int act_dim, int n_blue, const PolicySpec& actor, const PolicySpec& opponent);
void launch_task_lookahead_match(const Params& P, int L, int NR, const float* state, const float* aux, const float* obs, const uint32_t* ticks,
                                 const float* phys, const PolicySpec& p, const float* params, int n_params, int n_actors, int seats,
                                 const PolicySpec& opp, const float* opp_params, int n_opp_params, int n_opponents, int opp_seats, int act_dim,
                                 int horizon, float gamma, const rsx_match_out& out, hipStream_t s);
// rsx_gae.hip: values and GAE advantages of a [T][B] batch (rsx_task_advantages).  critic: rsx_policy_mlp with act_dim = 1 and a linear
// output, checked; params: [P]; gl: (float)gamma * (float)lam; in / out: the call's arrays, checked.  Two launches: the critic over
// T * B + B rows (and the rows truncated only of final_obs), then the reverse scan.  form: which values kernel (GAE_FORM_ROWS: one row per
// lane, the default; GAE_FORM_GROUPS: eight lanes per row, the collector's policy_forward — the same bits).  gae_lds_bytes: LDS of one
// workgroup of the values launch (the host refuses more than 64 KB)
enum : int { GAE_FORM_ROWS = 0, GAE_FORM_GROUPS = 1 };
long long gae_lds_bytes(int form, int obs_dim, const PolicySpec& critic);
void launch_advantages(int form, const PolicySpec& critic, const float* params, int obs_dim, float gamma, float gl, int T, int B,
                       const rsx_adv_in& in, const rsx_adv_out& out, hipStream_t s);
// rsx_ppo.hip: gradients of the PPO loss with respect to an MLP actor, its log_std and an MLP critic (rsx_task_ppo_gradient).  actor /
// critic: rsx_policy_mlp, checked (the actor's out_act plays no part); n_params_*: the floats of each; in / cfg / out: the call's
// structs, checked.  Three launches: the row kernel for the actor, the same for the critic, the reduce.  ppo_grid: workgroups of a row
// launch (min(ceil(n_rows / 64), max_workgroups or the build's default)); ppo_workspace_bytes: one partial per workgroup and network;
// ppo_lds_bytes: LDS of one workgroup of a row launch (the host refuses more than 64 KB)
int ppo_grid(long long n_rows, int max_workgroups);
long long ppo_lds_bytes(int obs_dim, int act_dim, const PolicySpec& net);
long long ppo_workspace_bytes(long long n_params_actor, long long n_params_critic, int act_dim, long long n_rows, int max_workgroups);
void launch_ppo_gradient(const PolicySpec& actor, long long n_params_actor, const float* actor_params, const float* log_std,
                         const PolicySpec& critic, long long n_params_critic, const float* critic_params, int obs_dim, int act_dim,
                         const rsx_ppo_in& in, const rsx_ppo_cfg& cfg, const rsx_ppo_out& out, hipStream_t s);
// rsx_ppo_update.hip: the update phase around launch_ppo_gradient (rsx_ppo_normalize, rsx_ppo_permutation, rsx_adam_step, rsx_adam_mark,
// rsx_task_ppo_update); every argument checked by the caller.  Two launches each for the normalisation and the Adam step, one for the
// permutation and the mark.  ppo_update_workspace_bytes: launch_ppo_update's workspace (rows_offset: where the int32 rows lie in it);
// launch_ppo_update enqueues the whole phase and calls launch_ppo_gradient per minibatch
void launch_ppo_normalize(const float* adv, long long n, float eps, float* out, float* mean_std, void* workspace, hipStream_t s);
void launch_ppo_permutation(int32_t* rows, long long n, uint64_t seed, uint32_t update, const long long* update_dev, uint32_t epoch,
                            hipStream_t s);
void launch_adam_step(const rsx_adam_cfg& c, const rsx_adam_state& st, const rsx_adam_io& io, hipStream_t s);
void launch_update_mark(int64_t* counters, int op, hipStream_t s);
long long ppo_update_chunk(long long n_batch_rows, int minibatches);
long long ppo_update_workspace_bytes(long long n_params_actor, long long n_params_critic, int act_dim, long long n_batch_rows,
                                     int minibatches, int max_workgroups, long long* rows_offset);
void launch_ppo_update(const PolicySpec& actor, long long n_params_actor, float* actor_params, float* log_std, const PolicySpec& critic,
                       long long n_params_critic, float* critic_params, int obs_dim, int act_dim, const rsx_ppo_in& in,
                       const rsx_ppo_cfg& cfg, const rsx_ppo_update_cfg& u, const rsx_adam_cfg& adam, const rsx_adam_state& st, float* stats,
                       void* workspace, hipStream_t s);
// rsx_dpg.hip: gradients of the TD3 / DDPG losses with respect to an MLP actor and n_critics critics on [obs | action]
// (rsx_task_dpg_gradient).  actor / critic: rsx_policy_mlp, checked; n_params_*: the floats of one network; *_params: the live and the
// target parameters (critics: [n_critics][n_params_critic]); in / cfg / out: the call's structs, checked.  Four launches: the targets,
// the critics (grid.y = critic), the actor through critic 0 (skipped without out.grad_actor), the reduce.  dpg_grid: workgroups of a row
// launch (min(ceil(n_rows / 64), max_workgroups or the build's default)); dpg_workspace_bytes: the targets and one partial per workgroup
// and network; dpg_lds_bytes: LDS of one workgroup of row launch `launch` (the host refuses more than a CU's 160 KB; beyond 64 KB the
// launch raises the kernel's limit itself)
enum : int { DPG_LAUNCH_TARGET = 0, DPG_LAUNCH_CRITIC = 1, DPG_LAUNCH_ACTOR = 2 };
int dpg_grid(long long n_rows, int max_workgroups);
long long dpg_lds_bytes(int launch, int obs_dim, int act_dim, const PolicySpec& actor, const PolicySpec& critic, int n_critics);
long long dpg_workspace_bytes(long long n_params_actor, long long n_params_critic, int n_critics, long long n_rows, int max_workgroups);
void launch_dpg_gradient(const PolicySpec& actor, long long n_params_actor, const float* actor_params, const float* target_actor_params,
                         const PolicySpec& critic, long long n_params_critic, const float* critic_params, const float* target_critic_params,
                         int obs_dim, int act_dim, const rsx_dpg_in& in, const rsx_dpg_cfg& cfg, const rsx_dpg_out& out, hipStream_t s,
                         const rsx_grad_per* per = nullptr);
// rsx_sac.hip: gradients of the soft actor-critic losses with respect to an MLP actor with a squashed Gaussian head (an output layer of
// 2 * act_dim units), n_critics critics on [obs | action] and the log-temperature (rsx_task_sac_gradient).  The arguments as for
// launch_dpg_gradient (no target actor; log_alpha: [1] on the device); in / cfg / out checked.  Six launches: the targets, the critics
// (grid.y = critic), the actor's sample, each critic on (obs, sample) with its dQ/da (grid.y = critic), the actor's backward pass, the
// reduce.  sac_grid / sac_workspace_bytes / sac_lds_bytes: as dpg_*
enum : int { SAC_LAUNCH_TARGET = 0, SAC_LAUNCH_CRITIC = 1, SAC_LAUNCH_SAMPLE = 2, SAC_LAUNCH_QA = 3, SAC_LAUNCH_ACTOR = 4 };
int sac_grid(long long n_rows, int max_workgroups);
long long sac_lds_bytes(int launch, int obs_dim, int act_dim, const PolicySpec& actor, const PolicySpec& critic, int n_critics);
long long sac_workspace_bytes(long long n_params_actor, long long n_params_critic, int n_critics, long long n_rows, int max_workgroups);
void launch_sac_gradient(const PolicySpec& actor, long long n_params_actor, const float* actor_params, const PolicySpec& critic,
                         long long n_params_critic, const float* critic_params, const float* target_critic_params, const float* log_alpha,
                         int obs_dim, int act_dim, const rsx_dpg_in& in, const rsx_sac_cfg& cfg, const rsx_sac_out& out, hipStream_t s,
                         const rsx_grad_per* per = nullptr);
// rsx_dpg_update.hip: the update phase around launch_dpg_gradient (rsx_replay_sample_rows, rsx_dpg_adam_step, rsx_task_dpg_update); every
// argument checked by the caller.  One launch for the rows, two for the optimiser step (the norms of both groups, then Adam with the
// Polyak step).  dpg_update_workspace_bytes: launch_dpg_update's workspace (rows_offset: where the int32 rows lie in it);
// launch_dpg_update enqueues the whole phase and calls launch_dpg_gradient per gradient step
void launch_replay_sample_rows(int32_t* rows, long long m, long long n_batch_rows, long long fill, const long long* fill_dev, uint64_t seed,
                               long long step, const long long* step_dev, hipStream_t s);
void launch_dpg_adam_step(const rsx_dpg_adam_cfg& c, const rsx_dpg_adam_state& st, const rsx_dpg_adam_io& io, hipStream_t s);
long long dpg_update_workspace_bytes(long long n_params_actor, long long n_params_critic, int n_critics, long long n_rows,
                                     int max_workgroups, long long* rows_offset);
void launch_dpg_update(const PolicySpec& actor, long long n_params_actor, float* actor_params, float* target_actor_params,
                       const PolicySpec& critic, long long n_params_critic, float* critic_params, float* target_critic_params, int obs_dim,
                       int act_dim, const rsx_dpg_in& in, const rsx_dpg_cfg& cfg, const rsx_dpg_update_cfg& u, const rsx_dpg_adam_cfg& adam,
                       const rsx_dpg_adam_state& st, float* stats, void* workspace, hipStream_t s);
// rsx_sac_update.hip: the update phase around launch_sac_gradient (rsx_sac_adam_step, rsx_task_sac_update); every argument checked by the
// caller.  Two launches for the optimiser step (the norms of the critics and the actor, then Adam on three groups — log_alpha in one
// thread — with the Polyak step of the target critics).  sac_update_workspace_bytes: launch_sac_update's workspace (rows_offset: where
// the int32 rows lie in it); launch_sac_update enqueues the whole phase and calls launch_replay_sample_rows and launch_sac_gradient per
// gradient step
void launch_sac_adam_step(const rsx_sac_adam_cfg& c, const rsx_sac_adam_state& st, const rsx_sac_adam_io& io, hipStream_t s);
long long sac_update_workspace_bytes(long long n_params_actor, long long n_params_critic, int n_critics, long long n_rows,
                                     int max_workgroups, long long* rows_offset);
void launch_sac_update(const PolicySpec& actor, long long n_params_actor, float* actor_params, const PolicySpec& critic,
                       long long n_params_critic, float* critic_params, float* target_critic_params, float* log_alpha, int obs_dim,
                       int act_dim, const rsx_dpg_in& in, const rsx_sac_cfg& cfg, const rsx_sac_update_cfg& u, const rsx_sac_adam_cfg& adam,
                       const rsx_sac_adam_state& st, float* stats, void* workspace, hipStream_t s);
// rsx_replay.hip: prioritised and n-step replay (rsx_replay_add_nstep, rsx_replay_tree_geometry, rsx_replay_set_priorities,
// rsx_replay_sample_prioritized) and the TD error of the weighted gradient calls; every argument checked by the caller.  One launch for
// the add; 2 + levels for the priorities (the leaves cleared, raised, then each level's touched nodes); a memset node and two launches
// for the draw; one for the TD error (q: [n_critics][m]).  launch_replay_sample_prioritized returns the memset's status.  per (the two
// gradient launches above): the rows' discounts and the entries' weights, or nullptr; its td_error is the caller's to fill
void replay_tree_geometry(long long capacity, long long* floats, int* levels, long long* offsets);
void launch_replay_add_nstep(const rsx_replay_batch& b, const rsx_replay_ring& r, int n_step, float gamma, hipStream_t s);
void launch_replay_set_priorities(float* tree, void* state, long long capacity, const int32_t* rows, const float* td_error,
                                  const long long* head_dev, long long m, float alpha, float eps, hipStream_t s);
hipError_t launch_replay_sample_prioritized(const float* tree, void* state, long long capacity, long long fill, const long long* fill_dev,
                                            int32_t* rows, float* weights, long long m, float beta, const float* beta_dev, uint64_t seed,
                                            long long step, const long long* step_dev, hipStream_t s);
void launch_replay_td_error(const float* q, const float* target, int n_critics, long long m, float* td_error, hipStream_t s);
// rsx_render.hip: batched rgb frames (rsx_render_*).  render_check_view: nullptr when the view is valid (and the frame size), else the
// message; render_field_host: the static field image [H][W][3]; RenderGeom: what the kernel needs of a view, in float32
struct RenderGeom { int W, H; float s, cx, cy, r, rb; int square; };
const char* render_check_view(const rsx_render_view* v, int* W, int* H);
void render_field_host(const rsx_render_view& v, int W, int H, uint8_t* out_hwc);
RenderGeom render_geom(const rsx_render_view& v, int W, int H);
void launch_render(const RenderGeom& g, const float* state, int num_envs, int row_stride, int kind, int n_blue, int n_yellow,
                   const uint8_t* tpl, uint32_t* err, const int32_t* env_ids, int n, int channels_first, uint8_t* out, hipStream_t s);
// rsx_xfer.hip: transfer of running episodes between envs and handles (rsx_task_transfer).  XferSide: the per-env arrays of a handle,
// or of a staging buffer of the same shape (phys: the parameter rows, the coefficient rows behind them; flags: terminated bytes,
// truncated bytes flag_pitch further).  mode: XFER_DIRECT handle -> handle; XFER_GATHER handle -> staging (record i = pair i),
// XFER_SCATTER staging -> handle.  dst_envs / src_envs: envs of the two handles (pairs with an id outside are skipped, and counted in
// *err by the DIRECT and GATHER launches); pot_row: VSS-v0's previous-potential row, recomputed from the source handle's ball, or -1
struct XferSide { float *state, *aux, *phys, *obs, *final_obs; uint8_t* flags; int stride, flag_pitch; };
enum : int { XFER_DIRECT = 0, XFER_GATHER = 1, XFER_SCATTER = 2 };
void launch_transfer(int mode, const XferSide& dst, const XferSide& src, int dst_envs, int src_envs, const int32_t* dst_ids,
                     const int32_t* src_ids, int n, uint32_t* err, int state_rows, int aux_rows, int phys_rows, int obs_dim, int pot_row,
                     float hl_goal, float inv_len_cm, hipStream_t s);

}  // namespace rsx
