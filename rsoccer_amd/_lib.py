"""ctypes binding of librsx_hip.so — the C-ABI declared in include/rsx.h.

This is the binding the reference would hold in place of ``import robosim``
(rsoccer_gym/Simulators/rsim.py:2).  It fails loudly when the HIP library is missing or no
GPU is visible: the product has no CPU path.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RSX_LIB") or os.path.join(_HERE, "librsx_hip.so")  # RSX_LIB: development builds

KIND_VSS, KIND_SSL = 0, 1
TASK_NONE, TASK_VSS_V0, TASK_SSL_STATIC_DEFENDERS = 0, 1, 2
TASK_SSL_DRIBBLING, TASK_SSL_CONTESTED, TASK_SSL_PASS_ENDURANCE = 3, 4, 5
TASK_SSL_SCRIMMAGE, TASK_SSL_SCRIMMAGE_CROWDED = 6, 7
FIELD_KEYS = (
    "length", "width", "penalty_length", "penalty_width", "goal_width", "goal_depth",
    "ball_radius", "rbt_distance_center_kicker", "rbt_kicker_thickness", "rbt_kicker_width",
    "rbt_wheel0_angle", "rbt_wheel1_angle", "rbt_wheel2_angle", "rbt_wheel3_angle",
    "rbt_radius", "rbt_wheel_radius", "rbt_motor_max_rpm",
)  # Entities/Field.py:5-21
N_METRICS = 8
X_ROWS = 2   # internal state rows behind get_state(): ball vertical velocity, ball spin (RSX_STATE_EXTRA_ROWS)
# per-env physics parameters (include/rsx.h: RSX_PHYS_*), in row order; "a_lat" is a VSS parameter (SSL: 0)
PHYSICS_PARAMS = ("m_robot", "m_ball", "e_rr", "e_rb", "e_wb", "e_wr", "mu_rr", "mu_rb", "mu_wb", "mu_g", "spin_dec",
                  "a_lin", "a_ang", "a_lat")
PHYSICS_COEFS = ("w_rb_r", "w_rb_b", "kt_rb_r", "kt_rb_b", "ope_rr", "ope_rb", "ope_wb", "e_wb", "e_wr", "mu_rr", "mu_rb", "mu_wb",
                 "a_lin_h", "a_lin_h2", "a_lat_h", "a_ang_h", "mu_g_dt", "spin_dec_dt")
PHYS_RAW, PHYS_COEF = 0, 1
# trace evaluation (include/rsx.h: RSX_TRACE_TERMS), in row order of the loss
TRACE_TERMS = ("ball_xy", "ball_v", "robot_xy", "robot_heading", "robot_v", "robot_omega")
METRIC_NAMES = ("env_steps", "episodes", "goals_for", "goals_against", "return_sum_q20",
                "episode_len_sum", "truncated_episodes", "reserved")

# every symbol include/rsx.h declares (tests check the library exports each one)
SYMBOLS = (
    "rsx_abi_version", "rsx_last_error", "rsx_device_count", "rsx_create", "rsx_destroy",
    "rsx_get_field_params", "rsx_reset", "rsx_step", "rsx_get_state", "rsx_step_state", "rsx_wire_buffers", "rsx_step_wire", "rsx_set_state",
    "rsx_get_state_full", "rsx_dev_view_get", "rsx_step_dev", "rsx_step_dev_random", "rsx_step_dev_flip", "rsx_state_buffers",
    "rsx_reset_dev", "rsx_task_attach",
    "rsx_task_view_get", "rsx_task_reseed", "rsx_task_layout", "rsx_task_service_wave", "rsx_task_placement_cache_stats", "rsx_task_reset", "rsx_task_reset_to", "rsx_task_step",
    "rsx_task_step_n", "rsx_task_rollout", "rsx_read_metrics", "rsx_metrics_fold", "rsx_check_finite",
    "rsx_task_checkpoint_size", "rsx_task_checkpoint_save", "rsx_task_checkpoint_load",
    "rsx_task_enable_capture", "rsx_task_tick", "rsx_drop_pending_hip_error", "rsx_task_lookahead",
    "rsx_physics_defaults", "rsx_physics_derive", "rsx_physics_enable", "rsx_physics_set", "rsx_physics_get",
    "rsx_physics_randomize", "rsx_physics_errors",
    "rsx_trace_load", "rsx_trace_eval",
    "rsx_render_view_reference", "rsx_render_size", "rsx_render_field", "rsx_render_open", "rsx_render", "rsx_render_errors",
    "rsx_task_transfer", "rsx_task_transfer_errors",
    "rsx_task_lookahead_sampled", "rsx_plan_candidates", "rsx_plan_update",
    "rsx_policy_num_params", "rsx_task_lookahead_policy", "rsx_task_lookahead_match",
    "rsx_task_collect_policy", "rsx_task_collect_selfplay", "rsx_task_collect_team", "rsx_task_collect_gaussian",
    "rsx_critic_num_params", "rsx_task_advantages",
    "rsx_ppo_gradient_workspace", "rsx_task_ppo_gradient",
    "rsx_ppo_normalize", "rsx_ppo_permutation", "rsx_adam_step", "rsx_adam_mark", "rsx_ppo_update_workspace", "rsx_task_ppo_update",
    "rsx_dpg_gradient_workspace", "rsx_task_dpg_gradient",
    "rsx_sac_gradient_workspace", "rsx_task_sac_gradient",
    "rsx_replay_sample_rows", "rsx_dpg_adam_step", "rsx_dpg_update_workspace", "rsx_task_dpg_update",
    "rsx_sac_adam_step", "rsx_sac_update_workspace", "rsx_task_sac_update",
    "rsx_replay_add_nstep", "rsx_replay_tree_geometry", "rsx_replay_set_priorities", "rsx_replay_sample_prioritized",
    "rsx_task_dpg_gradient_w", "rsx_task_sac_gradient_w",
)
# activations of rsx_policy_mlp (include/rsx.h: RSX_ACT_*)
ACT_RELU, ACT_TANH, ACT_CLIP = 0, 1, 2
ACT_NONE = 3   # identity: the output of a critic (rsx_task_advantages only)


class RsxError(RuntimeError):
    pass


class PlanSampler(C.Structure):
    """rsx_plan_sampler (include/rsx.h): the noise of sampled planning candidates"""
    _fields_ = [("sample_seed", C.c_uint64), ("sigma", C.c_float), ("hold", C.c_int32)]


class PolicyMLP(C.Structure):
    """rsx_policy_mlp (include/rsx.h): the shape of the policies of rsx_task_lookahead_policy"""
    _fields_ = [("n_hidden_layers", C.c_int32), ("hidden", C.c_int32), ("hidden_act", C.c_int32), ("out_act", C.c_int32)]


class CollectOut(C.Structure):
    """rsx_collect_out (include/rsx.h): the [T][B] record of rsx_task_collect_policy; device addresses, the last three may be None"""
    _fields_ = [("obs", C.c_void_p), ("actions", C.c_void_p), ("rewards", C.c_void_p), ("flags", C.c_void_p),
                ("final_obs", C.c_void_p), ("mean", C.c_void_p), ("sample", C.c_void_p)]


class CollectGaussianCfg(C.Structure):
    """rsx_collect_gaussian_cfg (include/rsx.h): the squashed Gaussian head of rsx_task_collect_gaussian"""
    _fields_ = [("noise_seed", C.c_uint64), ("log_std_min", C.c_float), ("log_std_max", C.c_float), ("deterministic", C.c_int32),
                ("reserved", C.c_int32)]


class SelfplayOut(C.Structure):
    """rsx_selfplay_out (include/rsx.h): the opponent's [T][B] record of rsx_task_collect_selfplay; device addresses, each may be None"""
    _fields_ = [("opp_obs", C.c_void_p), ("opp_actions", C.c_void_p), ("opp_mean", C.c_void_p), ("opp_sample", C.c_void_p)]


class TeamSideOut(C.Structure):
    """rsx_team_side_out (include/rsx.h): one side's [T][B][S] record of rsx_task_collect_team; device addresses.  The actor's obs and
    actions are required, everything else may be None"""
    _fields_ = [("obs", C.c_void_p), ("actions", C.c_void_p), ("mean", C.c_void_p), ("sample", C.c_void_p), ("final_obs", C.c_void_p),
                ("next_obs", C.c_void_p)]


class TeamOut(C.Structure):
    """rsx_team_out (include/rsx.h): the record of rsx_task_collect_team: rewards and flags [T][B] and a TeamSideOut per side"""
    _fields_ = [("rewards", C.c_void_p), ("flags", C.c_void_p), ("actor", TeamSideOut), ("opponent", TeamSideOut)]


class MatchOut(C.Structure):
    """rsx_match_out (include/rsx.h): the [B][K][M] results and records of rsx_task_lookahead_match; device addresses, everything
    behind flags may be None"""
    _fields_ = [("returns", C.c_void_p), ("steps", C.c_void_p), ("flags", C.c_void_p), ("result", C.c_void_p), ("last_obs", C.c_void_p),
                ("actions", C.c_void_p), ("obs", C.c_void_p), ("opp_actions", C.c_void_p), ("opp_obs", C.c_void_p)]


class AdvIn(C.Structure):
    """rsx_adv_in (include/rsx.h): the [T][B] batch rsx_task_advantages reads; device addresses, final_obs may be None"""
    _fields_ = [("obs", C.c_void_p), ("rewards", C.c_void_p), ("terminated", C.c_void_p), ("truncated", C.c_void_p),
                ("final_obs", C.c_void_p), ("last_obs", C.c_void_p)]


class AdvOut(C.Structure):
    """rsx_adv_out (include/rsx.h): the [T][B] results of rsx_task_advantages; device addresses, next_values may be None"""
    _fields_ = [("values", C.c_void_p), ("advantages", C.c_void_p), ("returns", C.c_void_p), ("next_values", C.c_void_p)]


class PpoIn(C.Structure):
    """rsx_ppo_in (include/rsx.h): the flattened [N] batch rsx_task_ppo_gradient reads and the minibatch's rows; device addresses,
    rows may be None (rows 0 .. M - 1)"""
    _fields_ = [("obs", C.c_void_p), ("sample", C.c_void_p), ("old_log_prob", C.c_void_p), ("advantage", C.c_void_p), ("ret", C.c_void_p),
                ("rows", C.c_void_p), ("n_batch_rows", C.c_int64), ("n_rows", C.c_int64)]


class PpoCfg(C.Structure):
    """rsx_ppo_cfg (include/rsx.h): the scalars of the PPO loss and the cap of the grid (0 = the build's default)"""
    _fields_ = [("clip", C.c_float), ("vf_coef", C.c_float), ("ent_coef", C.c_float), ("max_workgroups", C.c_int32)]


class PpoOut(C.Structure):
    """rsx_ppo_out (include/rsx.h): the gradients, the stats [8], the optional forward outputs and the workspace; device addresses"""
    _fields_ = [("grad_actor", C.c_void_p), ("grad_log_std", C.c_void_p), ("grad_critic", C.c_void_p), ("stats", C.c_void_p),
                ("mean", C.c_void_p), ("value", C.c_void_p), ("workspace", C.c_void_p)]


# the slots of rsx_ppo_out.stats, in order
PPO_STATS = ("loss_pi", "loss_v", "entropy", "approx_kl", "clip_fraction", "ratio", "rows_used", "rows_skipped")


class DpgIn(C.Structure):
    """rsx_dpg_in (include/rsx.h): the N flat transition rows rsx_task_dpg_gradient reads and the minibatch's rows; device addresses,
    rows may be None (rows 0 .. M - 1)"""
    _fields_ = [("obs", C.c_void_p), ("action", C.c_void_p), ("reward", C.c_void_p), ("next_obs", C.c_void_p), ("terminated", C.c_void_p),
                ("rows", C.c_void_p), ("n_batch_rows", C.c_int64), ("n_rows", C.c_int64)]


class DpgCfg(C.Structure):
    """rsx_dpg_cfg (include/rsx.h): the smoothing noise's step (by value or as a device address), seed, sigma and clip, gamma, the number
    of critics and the cap of the grid (0 = the build's default)"""
    _fields_ = [("noise_step_dev", C.c_void_p), ("noise_seed", C.c_uint64), ("noise_step", C.c_int64), ("gamma", C.c_float),
                ("sigma", C.c_float), ("noise_clip", C.c_float), ("n_critics", C.c_int32), ("max_workgroups", C.c_int32)]


class DpgOut(C.Structure):
    """rsx_dpg_out (include/rsx.h): the gradients (grad_actor None: no actor launch), the stats [9], the optional per-entry outputs and
    the workspace; device addresses"""
    _fields_ = [("grad_actor", C.c_void_p), ("grad_critics", C.c_void_p), ("stats", C.c_void_p), ("target", C.c_void_p), ("q", C.c_void_p),
                ("action", C.c_void_p), ("target_noise", C.c_void_p), ("workspace", C.c_void_p)]


# the slots of rsx_dpg_out.stats, in order
DPG_STATS = ("loss_q0", "loss_q1", "q0", "q1", "loss_pi", "target", "abs_next_action", "rows_used", "rows_skipped")


class SacCfg(C.Structure):
    """rsx_sac_cfg (include/rsx.h): the draws' step (by value or as a device address) and seed, gamma, the target entropy, the log-std
    bounds, the number of critics and the cap of the grid (0 = the build's default)"""
    _fields_ = [("noise_step_dev", C.c_void_p), ("noise_seed", C.c_uint64), ("noise_step", C.c_int64), ("gamma", C.c_float),
                ("target_entropy", C.c_float), ("log_std_min", C.c_float), ("log_std_max", C.c_float), ("n_critics", C.c_int32),
                ("max_workgroups", C.c_int32)]


class SacOut(C.Structure):
    """rsx_sac_out (include/rsx.h): the three gradients, the stats [12], the optional per-entry outputs and the workspace; device addresses"""
    _fields_ = [("grad_actor", C.c_void_p), ("grad_critics", C.c_void_p), ("grad_log_alpha", C.c_void_p), ("stats", C.c_void_p),
                ("target", C.c_void_p), ("q", C.c_void_p), ("action", C.c_void_p), ("log_prob", C.c_void_p), ("next_log_prob", C.c_void_p),
                ("eps", C.c_void_p), ("next_eps", C.c_void_p), ("mean", C.c_void_p), ("log_std", C.c_void_p), ("workspace", C.c_void_p)]


# the slots of rsx_sac_out.stats, in order
SAC_STATS = ("loss_q0", "loss_q1", "q0", "q1", "loss_pi", "loss_alpha", "target", "log_prob", "next_log_prob", "alpha", "rows_used",
             "rows_skipped")


# the update phase (include/rsx.h: rsx_ppo_normalize, rsx_adam_step, rsx_task_ppo_update)
PPO_NORMALIZE_WORKSPACE_BYTES, ADAM_WORKSPACE_BYTES = 2048, 1024
# the slots of rsx_adam_state.counters (RSX_ADAM_*), and of one row of rsx_task_ppo_update's stats: PPO_STATS and two more
ADAM_COUNTERS = ("t", "updates", "applied", "stopped")
PPO_UPDATE_STATS = PPO_STATS + ("grad_norm", "applied")


class AdamCfg(C.Structure):
    """rsx_adam_cfg (include/rsx.h): the betas as doubles, lr by value or as a device address (lr_dev, None = lr), eps, the clip's
    max_grad_norm (<= 0: none) and the KL stop's target_kl (0: none)"""
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("lr_dev", C.c_void_p), ("lr", C.c_float), ("eps", C.c_float),
                ("max_grad_norm", C.c_float), ("target_kl", C.c_float)]


class AdamState(C.Structure):
    """rsx_adam_state (include/rsx.h): m and v of the three flat tensors, the int64 counters [4] and the three sizes; device addresses"""
    _fields_ = [("m_actor", C.c_void_p), ("v_actor", C.c_void_p), ("m_log_std", C.c_void_p), ("v_log_std", C.c_void_p),
                ("m_critic", C.c_void_p), ("v_critic", C.c_void_p), ("counters", C.c_void_p),
                ("n_actor", C.c_int64), ("n_log_std", C.c_int64), ("n_critic", C.c_int64)]


class AdamIo(C.Structure):
    """rsx_adam_io (include/rsx.h): the three parameter tensors (updated in place), their gradients, the optional approx_kl [1] and
    stats [2], and the workspace; device addresses"""
    _fields_ = [("actor_params", C.c_void_p), ("log_std", C.c_void_p), ("critic_params", C.c_void_p), ("grad_actor", C.c_void_p),
                ("grad_log_std", C.c_void_p), ("grad_critic", C.c_void_p), ("approx_kl", C.c_void_p), ("stats", C.c_void_p),
                ("workspace", C.c_void_p)]


class PpoUpdateCfg(C.Structure):
    """rsx_ppo_update_cfg (include/rsx.h): the permutations' seed, epochs, minibatches, whether and with which eps advantages are normalised"""
    _fields_ = [("seed", C.c_uint64), ("epochs", C.c_int32), ("minibatches", C.c_int32), ("normalize_advantage", C.c_int32),
                ("norm_eps", C.c_float)]


# the off-policy update phase (include/rsx.h: rsx_replay_sample_rows, rsx_dpg_adam_step, rsx_task_dpg_update)
DPG_ADAM_WORKSPACE_BYTES = 2048
# the slots of rsx_dpg_adam_state.counters (RSX_DPG_*), of rsx_dpg_adam_io.stats, and of one row of rsx_task_dpg_update's stats
DPG_COUNTERS = ("t_critic", "t_actor", "steps", "spare")
DPG_ADAM_STATS = ("grad_norm_critic", "grad_norm_actor", "targets_moved")
DPG_UPDATE_STATS = DPG_STATS + DPG_ADAM_STATS


class DpgAdamCfg(C.Structure):
    """rsx_dpg_adam_cfg (include/rsx.h): the betas as doubles, each group's lr by value or as a device address (None = by value), eps,
    the bound of each group's own gradient norm (<= 0: none) and the Polyak step's tau"""
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("lr_actor_dev", C.c_void_p), ("lr_critic_dev", C.c_void_p),
                ("lr_actor", C.c_float), ("lr_critic", C.c_float), ("eps", C.c_float), ("max_grad_norm", C.c_float), ("tau", C.c_float)]


class DpgAdamState(C.Structure):
    """rsx_dpg_adam_state (include/rsx.h): m and v of the actor's and the critics' flat tensors, the int64 counters [4] and the two
    sizes; device addresses"""
    _fields_ = [("m_actor", C.c_void_p), ("v_actor", C.c_void_p), ("m_critic", C.c_void_p), ("v_critic", C.c_void_p),
                ("counters", C.c_void_p), ("n_actor", C.c_int64), ("n_critic", C.c_int64)]


class DpgAdamIo(C.Structure):
    """rsx_dpg_adam_io (include/rsx.h): the live and target tensors of both groups (updated in place), the gradients (grad_actor None:
    no actor step), the optional stats [3], the workspace and whether the targets move; device addresses"""
    _fields_ = [("actor_params", C.c_void_p), ("target_actor_params", C.c_void_p), ("critic_params", C.c_void_p),
                ("target_critic_params", C.c_void_p), ("grad_actor", C.c_void_p), ("grad_critic", C.c_void_p), ("stats", C.c_void_p),
                ("workspace", C.c_void_p), ("update_targets", C.c_int32)]


class DpgUpdateCfg(C.Structure):
    """rsx_dpg_update_cfg (include/rsx.h): the ring's fill count (by device address, or None and by value), the row draws' seed, the
    gradient steps of the call and the actor's delay"""
    _fields_ = [("fill_dev", C.c_void_p), ("seed", C.c_uint64), ("fill", C.c_int64), ("grad_steps", C.c_int32), ("policy_delay", C.c_int32)]


# prioritised and n-step replay (include/rsx.h: rsx_replay_add_nstep, rsx_replay_set_priorities, rsx_replay_sample_prioritized)
# the 32-bit words of a state block (RSX_REPLAY_STATE_*)
REPLAY_STATE = ("max", "wmax", "skipped", "ticket")


class ReplayBatch(C.Structure):
    """rsx_replay_batch (include/rsx.h): the arrays of a collected [T][B] batch with final_obs; device addresses"""
    _fields_ = [("obs", C.c_void_p), ("actions", C.c_void_p), ("reward", C.c_void_p), ("terminated", C.c_void_p), ("truncated", C.c_void_p),
                ("final_obs", C.c_void_p), ("next_obs", C.c_void_p), ("T", C.c_int32), ("B", C.c_int32)]


class ReplayRing(C.Structure):
    """rsx_replay_ring (include/rsx.h): the ring's arrays, its head and fill counts and the add's ticket on the device, and its shape"""
    _fields_ = [("obs", C.c_void_p), ("actions", C.c_void_p), ("reward", C.c_void_p), ("next_obs", C.c_void_p), ("terminated", C.c_void_p),
                ("discount", C.c_void_p), ("head_dev", C.c_void_p), ("fill_dev", C.c_void_p), ("ticket_dev", C.c_void_p),
                ("capacity", C.c_int64), ("obs_dim", C.c_int32), ("act_dim", C.c_int32)]


class GradPer(C.Structure):
    """rsx_grad_per (include/rsx.h): the rows' discounts [N], the entries' weights [M] and the TD error [M] (out) of the weighted
    gradient calls; device addresses, each may be None"""
    _fields_ = [("discount", C.c_void_p), ("weight", C.c_void_p), ("td_error", C.c_void_p)]


# the soft actor-critic update phase (include/rsx.h: rsx_sac_adam_step, rsx_task_sac_update)
SAC_ADAM_WORKSPACE_BYTES = 2048
# the slots of rsx_sac_adam_state.counters (RSX_SAC_*), of rsx_sac_adam_io.stats, and of one row of rsx_task_sac_update's stats
SAC_COUNTERS = ("t_critic", "t_actor", "t_alpha", "steps")
SAC_ADAM_STATS = ("grad_norm_critic", "grad_norm_actor", "log_alpha", "targets_moved")
SAC_UPDATE_STATS = SAC_STATS + SAC_ADAM_STATS


class SacAdamCfg(C.Structure):
    """rsx_sac_adam_cfg (include/rsx.h): the betas as doubles, each group's lr (actor, critics, log_alpha) by value or as a device
    address (None = by value), eps, the bound of the critics' and of the actor's own gradient norm (<= 0: none) and the Polyak step's tau"""
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("lr_actor_dev", C.c_void_p), ("lr_critic_dev", C.c_void_p),
                ("lr_alpha_dev", C.c_void_p), ("lr_actor", C.c_float), ("lr_critic", C.c_float), ("lr_alpha", C.c_float), ("eps", C.c_float),
                ("max_grad_norm", C.c_float), ("tau", C.c_float)]


class SacAdamState(C.Structure):
    """rsx_sac_adam_state (include/rsx.h): m and v of the actor's and the critics' flat tensors and of log_alpha, the int64 counters [4]
    and the two sizes; device addresses"""
    _fields_ = [("m_actor", C.c_void_p), ("v_actor", C.c_void_p), ("m_critic", C.c_void_p), ("v_critic", C.c_void_p),
                ("m_alpha", C.c_void_p), ("v_alpha", C.c_void_p), ("counters", C.c_void_p), ("n_actor", C.c_int64), ("n_critic", C.c_int64)]


class SacAdamIo(C.Structure):
    """rsx_sac_adam_io (include/rsx.h): the actor, the critics, the target critics and log_alpha (updated in place), the gradients
    (grad_actor None: no actor step; grad_log_alpha None: a fixed temperature), the optional stats [4], the workspace and whether the
    targets move; device addresses"""
    _fields_ = [("actor_params", C.c_void_p), ("critic_params", C.c_void_p), ("target_critic_params", C.c_void_p), ("log_alpha", C.c_void_p),
                ("grad_actor", C.c_void_p), ("grad_critic", C.c_void_p), ("grad_log_alpha", C.c_void_p), ("stats", C.c_void_p),
                ("workspace", C.c_void_p), ("update_targets", C.c_int32)]


class SacUpdateCfg(C.Structure):
    """rsx_sac_update_cfg (include/rsx.h): the ring's fill count (by device address, or None and by value), the row draws' seed, the
    gradient steps of the call and whether log_alpha is stepped"""
    _fields_ = [("fill_dev", C.c_void_p), ("seed", C.c_uint64), ("fill", C.c_int64), ("grad_steps", C.c_int32), ("learn_alpha", C.c_int32)]


class DevView(C.Structure):
    _fields_ = [("num_envs", C.c_int32), ("n_robots", C.c_int32), ("state_dim", C.c_int32),
                ("cmd_dim", C.c_int32), ("state", C.c_void_p), ("cmds", C.c_void_p), ("row_stride", C.c_int32)]


class TaskView(C.Structure):
    _fields_ = [("task", C.c_int32), ("obs_dim", C.c_int32), ("act_dim", C.c_int32),
                ("info_dim", C.c_int32), ("max_episode_steps", C.c_int32),
                ("obs", C.c_void_p), ("reward", C.c_void_p), ("terminated", C.c_void_p),
                ("truncated", C.c_void_p), ("info", C.c_void_p), ("final_obs", C.c_void_p),
                ("steps", C.c_void_p), ("actions", C.c_void_p), ("metrics", C.c_void_p), ("row_stride", C.c_int32)]


# the keys of Render/raster.py's view dicts, in the order of rsx_render_view
RENDER_VIEW_KEYS = ("length", "width", "margin", "circle", "pen_len", "pen_wid", "goal_wid", "goal_dep", "scale", "robot", "ball", "square")


class RenderView(C.Structure):
    _fields_ = [(k, C.c_double) for k in RENDER_VIEW_KEYS[:-1]] + [("square", C.c_int32)]

    @classmethod
    def from_dict(cls, view):
        """a view dict in raster.py's format (VSS_VIEW / SSL_VIEW) as the C struct"""
        missing = [k for k in RENDER_VIEW_KEYS if k not in view]
        if missing:
            raise ValueError(f"render view lacks {missing}")
        return cls(*[float(view[k]) for k in RENDER_VIEW_KEYS[:-1]], 1 if view["square"] else 0)

    def to_dict(self):
        d = {k: float(getattr(self, k)) for k in RENDER_VIEW_KEYS[:-1]}
        d["square"] = bool(self.square)
        return d


_lib = None


def load():
    """Load librsx_hip.so (once).  torch is imported first so that the HIP runtime already in
    the process (torch ships its own libamdhip64.so.7) is the one the library binds to —
    device pointers and streams are then shared with torch tensors."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RsxError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). rsoccer_amd has no CPU fallback.")
    try:
        import torch  # noqa: F401  (loads libamdhip64 with the right SONAME first)
    except Exception:
        pass
    lib = C.CDLL(LIB_PATH)
    lib.rsx_last_error.restype = C.c_char_p
    vp, ip, dp = C.c_void_p, C.c_int, C.POINTER(C.c_double)
    lib.rsx_create.argtypes = [C.POINTER(vp), ip, ip, ip, ip, ip, ip, ip]
    lib.rsx_destroy.argtypes = [vp]
    lib.rsx_get_field_params.argtypes = [vp, dp]
    lib.rsx_reset.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.rsx_step.argtypes = [vp, vp, vp]
    lib.rsx_get_state.argtypes = [vp, vp, vp]
    lib.rsx_step_state.argtypes = [vp, vp, vp, vp]
    lib.rsx_task_layout.argtypes = [vp, C.c_char_p, C.c_size_t]
    lib.rsx_task_service_wave.argtypes = [vp, C.POINTER(C.c_int)]
    lib.rsx_task_placement_cache_stats.argtypes = [vp, C.POINTER(C.c_int64), vp]
    lib.rsx_set_state.argtypes = [vp, vp, vp]
    lib.rsx_wire_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    lib.rsx_step_wire.argtypes = [vp, vp]
    lib.rsx_get_state_full.argtypes = [vp, vp, vp]
    lib.rsx_dev_view_get.argtypes = [vp, C.POINTER(DevView)]
    lib.rsx_step_dev.argtypes = [vp, vp]
    lib.rsx_step_dev_random.argtypes = [vp, ip, C.c_uint64, C.c_uint32, vp]
    lib.rsx_step_dev_flip.argtypes = [vp, vp]
    lib.rsx_state_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    lib.rsx_reset_dev.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.rsx_task_attach.argtypes = [vp, ip, C.c_uint64, C.c_uint64, ip]
    lib.rsx_task_view_get.argtypes = [vp, C.POINTER(TaskView)]
    lib.rsx_task_reseed.argtypes = [vp, C.c_uint64, vp]
    lib.rsx_task_reset.argtypes = [vp, vp]
    lib.rsx_task_reset_to.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.rsx_task_step.argtypes = [vp, vp, vp]
    lib.rsx_task_step_n.argtypes = [vp, ip, vp]
    lib.rsx_task_rollout.argtypes = [vp, ip, vp]
    lib.rsx_read_metrics.argtypes = [vp, vp, vp]
    lib.rsx_metrics_fold.argtypes = [vp, vp]
    lib.rsx_task_checkpoint_size.argtypes = [vp, C.POINTER(C.c_size_t)]
    lib.rsx_task_checkpoint_save.argtypes = [vp, vp, C.c_size_t, vp]
    lib.rsx_task_checkpoint_load.argtypes = [vp, vp, C.c_size_t, vp]
    lib.rsx_check_finite.argtypes = [vp, C.POINTER(C.c_int64), vp]
    lib.rsx_task_enable_capture.argtypes = [vp, vp]
    lib.rsx_task_tick.argtypes = [vp, C.POINTER(C.c_uint32), vp]
    lib.rsx_drop_pending_hip_error.argtypes = []
    lib.rsx_task_lookahead.argtypes = [vp, vp, ip, ip, C.c_float, vp, vp, vp, vp, vp]
    lib.rsx_task_lookahead_sampled.argtypes = [vp, vp, C.POINTER(PlanSampler), ip, ip, C.c_float, vp, vp, vp, vp, vp]
    lib.rsx_plan_candidates.argtypes = [vp, vp, C.POINTER(PlanSampler), ip, ip, vp, vp]
    lib.rsx_plan_update.argtypes = [vp, vp, C.POINTER(PlanSampler), ip, ip, vp, C.c_float, vp, vp, vp]
    lib.rsx_policy_num_params.argtypes = [vp, C.POINTER(PolicyMLP), C.POINTER(C.c_int64)]
    lib.rsx_task_lookahead_policy.argtypes = [vp, C.POINTER(PolicyMLP), vp, ip, ip, C.c_float, vp, vp, vp, vp, vp, vp, vp]
    lib.rsx_task_collect_policy.argtypes = [vp, C.POINTER(PolicyMLP), vp, vp, C.c_uint64, ip, C.POINTER(CollectOut), vp]
    lib.rsx_task_collect_gaussian.argtypes = [vp, C.POINTER(PolicyMLP), vp, C.POINTER(CollectGaussianCfg), ip, C.POINTER(CollectOut), vp, vp]
    lib.rsx_task_collect_selfplay.argtypes = [vp, C.POINTER(PolicyMLP), vp, vp, C.POINTER(PolicyMLP), vp, vp, C.c_uint64, ip,
                                              C.POINTER(CollectOut), C.POINTER(SelfplayOut), vp]
    lib.rsx_task_lookahead_match.argtypes = [vp, C.POINTER(PolicyMLP), vp, ip, ip, C.POINTER(PolicyMLP), vp, ip, ip, ip, C.c_float,
                                             C.POINTER(MatchOut), vp]
    lib.rsx_task_collect_team.argtypes = [vp, C.POINTER(PolicyMLP), vp, vp, ip, C.POINTER(PolicyMLP), vp, vp, ip, C.c_uint64, ip,
                                          C.POINTER(TeamOut), vp]
    lib.rsx_critic_num_params.argtypes = [vp, C.POINTER(PolicyMLP), C.POINTER(C.c_int64)]
    lib.rsx_task_advantages.argtypes = [vp, C.POINTER(PolicyMLP), vp, C.c_float, C.c_float, ip, ip, C.POINTER(AdvIn), C.POINTER(AdvOut), vp]
    lib.rsx_ppo_gradient_workspace.argtypes = [vp, C.POINTER(PolicyMLP), C.POINTER(PolicyMLP), C.c_int64, ip, C.POINTER(C.c_int64)]
    lib.rsx_task_ppo_gradient.argtypes = [vp, C.POINTER(PolicyMLP), vp, vp, C.POINTER(PolicyMLP), vp, C.POINTER(PpoIn), C.POINTER(PpoCfg),
                                          C.POINTER(PpoOut), vp]
    lib.rsx_ppo_normalize.argtypes = [vp, C.c_int64, C.c_float, vp, vp, vp, vp]
    lib.rsx_ppo_permutation.argtypes = [vp, C.c_int64, C.c_uint64, C.c_uint64, vp, C.c_int64, vp]
    lib.rsx_adam_step.argtypes = [C.POINTER(AdamCfg), C.POINTER(AdamState), C.POINTER(AdamIo), vp]
    lib.rsx_adam_mark.argtypes = [C.POINTER(AdamState), ip, vp]
    lib.rsx_ppo_update_workspace.argtypes = [vp, C.POINTER(PolicyMLP), C.POINTER(PolicyMLP), C.c_int64, ip, ip, C.POINTER(C.c_int64),
                                             C.POINTER(C.c_int64)]
    lib.rsx_task_ppo_update.argtypes = [vp, C.POINTER(PolicyMLP), vp, vp, C.POINTER(PolicyMLP), vp, C.POINTER(PpoIn), C.POINTER(PpoCfg),
                                        C.POINTER(PpoUpdateCfg), C.POINTER(AdamCfg), C.POINTER(AdamState), vp, vp, vp]
    lib.rsx_dpg_gradient_workspace.argtypes = [vp, C.POINTER(PolicyMLP), C.POINTER(PolicyMLP), ip, C.c_int64, ip, C.POINTER(C.c_int64)]
    lib.rsx_sac_gradient_workspace.argtypes = [vp, C.POINTER(PolicyMLP), C.POINTER(PolicyMLP), ip, C.c_int64, ip, C.POINTER(C.c_int64)]
    lib.rsx_task_sac_gradient.argtypes = [vp, C.POINTER(PolicyMLP), vp, C.POINTER(PolicyMLP), vp, vp, vp, C.POINTER(DpgIn), C.POINTER(SacCfg),
                                          C.POINTER(SacOut), vp]
    lib.rsx_task_dpg_gradient.argtypes = [vp, C.POINTER(PolicyMLP), vp, vp, C.POINTER(PolicyMLP), vp, vp, C.POINTER(DpgIn), C.POINTER(DpgCfg),
                                          C.POINTER(DpgOut), vp]
    lib.rsx_replay_sample_rows.argtypes = [vp, C.c_int64, C.c_int64, C.c_int64, vp, C.c_uint64, C.c_int64, vp, vp]
    lib.rsx_dpg_adam_step.argtypes = [C.POINTER(DpgAdamCfg), C.POINTER(DpgAdamState), C.POINTER(DpgAdamIo), vp]
    lib.rsx_dpg_update_workspace.argtypes = [vp, C.POINTER(PolicyMLP), C.POINTER(PolicyMLP), ip, C.c_int64, ip, C.POINTER(C.c_int64),
                                             C.POINTER(C.c_int64)]
    lib.rsx_task_dpg_update.argtypes = [vp, C.POINTER(PolicyMLP), vp, vp, C.POINTER(PolicyMLP), vp, vp, C.POINTER(DpgIn), C.POINTER(DpgCfg),
                                        C.POINTER(DpgUpdateCfg), C.POINTER(DpgAdamCfg), C.POINTER(DpgAdamState), vp, vp, vp]
    lib.rsx_sac_adam_step.argtypes = [C.POINTER(SacAdamCfg), C.POINTER(SacAdamState), C.POINTER(SacAdamIo), vp]
    lib.rsx_sac_update_workspace.argtypes = [vp, C.POINTER(PolicyMLP), C.POINTER(PolicyMLP), ip, C.c_int64, ip, C.POINTER(C.c_int64),
                                             C.POINTER(C.c_int64)]
    lib.rsx_task_sac_update.argtypes = [vp, C.POINTER(PolicyMLP), vp, C.POINTER(PolicyMLP), vp, vp, vp, C.POINTER(DpgIn), C.POINTER(SacCfg),
                                        C.POINTER(SacUpdateCfg), C.POINTER(SacAdamCfg), C.POINTER(SacAdamState), vp, vp, vp]
    lib.rsx_replay_add_nstep.argtypes = [C.POINTER(ReplayBatch), C.POINTER(ReplayRing), ip, C.c_float, vp]
    lib.rsx_replay_tree_geometry.argtypes = [C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    lib.rsx_replay_set_priorities.argtypes = [vp, vp, C.c_int64, vp, vp, vp, C.c_int64, C.c_float, C.c_float, vp]
    lib.rsx_replay_sample_prioritized.argtypes = [vp, vp, C.c_int64, C.c_int64, vp, vp, vp, C.c_int64, C.c_float, vp, C.c_uint64, C.c_int64,
                                                  vp, vp]
    lib.rsx_task_dpg_gradient_w.argtypes = [vp, C.POINTER(PolicyMLP), vp, vp, C.POINTER(PolicyMLP), vp, vp, C.POINTER(DpgIn), C.POINTER(DpgCfg),
                                            C.POINTER(DpgOut), C.POINTER(GradPer), vp]
    lib.rsx_task_sac_gradient_w.argtypes = [vp, C.POINTER(PolicyMLP), vp, C.POINTER(PolicyMLP), vp, vp, vp, C.POINTER(DpgIn), C.POINTER(SacCfg),
                                            C.POINTER(SacOut), C.POINTER(GradPer), vp]
    lib.rsx_physics_defaults.argtypes = [ip, vp]
    lib.rsx_physics_derive.argtypes = [ip, ip, vp, vp]
    lib.rsx_physics_enable.argtypes = [vp, vp]
    lib.rsx_physics_set.argtypes = [vp, vp, ip, vp, vp]
    lib.rsx_physics_get.argtypes = [vp, ip, vp, vp]
    lib.rsx_physics_randomize.argtypes = [vp, vp, vp, C.c_uint32, vp]
    lib.rsx_physics_errors.argtypes = [vp, C.POINTER(C.c_int64), vp]
    lib.rsx_trace_load.argtypes = [vp, vp, vp, ip, vp, ip, vp]
    lib.rsx_trace_eval.argtypes = [vp, ip, vp, vp]
    lib.rsx_render_view_reference.argtypes = [ip, C.POINTER(RenderView)]
    lib.rsx_render_size.argtypes = [C.POINTER(RenderView), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.rsx_render_field.argtypes = [C.POINTER(RenderView), vp]
    lib.rsx_render_open.argtypes = [vp, C.POINTER(RenderView), vp]
    lib.rsx_render.argtypes = [vp, vp, ip, ip, vp, vp]
    lib.rsx_render_errors.argtypes = [vp, C.POINTER(C.c_int64), vp]
    lib.rsx_task_transfer.argtypes = [vp, vp, vp, vp, ip, vp]
    lib.rsx_task_transfer_errors.argtypes = [vp, C.POINTER(C.c_int64), vp]
    if lib.rsx_abi_version() != 6:
        raise RsxError("librsx_hip.so ABI version mismatch")
    _lib = lib
    return lib


def drop_pending_hip_error():
    """reads and clears the thread's pending HIP error (rsx_drop_pending_hip_error): what an aborted stream capture leaves behind"""
    return int(load().rsx_drop_pending_hip_error())


def _chk(rc):
    if rc != 0:
        raise RsxError(f"librsx_hip error {rc}: {load().rsx_last_error().decode()}")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the handle-free calls of the update phase: they run on the thread's current device (the callers make theirs current) ----
def ppo_normalize(adv_ptr, n, eps, out_ptr, mean_std_ptr, workspace_ptr, stream=None):
    """rsx_ppo_normalize: out = (adv - mean) / (std + eps) over n float32 entries, in two launches"""
    rc = load().rsx_ppo_normalize(adv_ptr, int(n), float(eps), out_ptr, mean_std_ptr, workspace_ptr, stream)
    if rc:
        _chk(rc)


def ppo_permutation(rows_ptr, n, seed, update, update_ptr, epoch, stream=None):
    """rsx_ppo_permutation: rows [n] int32 := the permutation of 0 .. n - 1 keyed by (seed, update or the int64 at update_ptr, epoch)"""
    rc = load().rsx_ppo_permutation(rows_ptr, int(n), int(seed) & ((1 << 64) - 1), int(update) & ((1 << 64) - 1), update_ptr, int(epoch), stream)
    if rc:
        _chk(rc)


def adam_step(cfg, state, io, stream=None):
    """rsx_adam_step: the global-norm clip and one Adam step on the three flat tensors, in two launches"""
    rc = load().rsx_adam_step(None if cfg is None else C.byref(cfg), None if state is None else C.byref(state),
                              None if io is None else C.byref(io), stream)
    if rc:
        _chk(rc)


def adam_mark(state, end, stream=None):
    """rsx_adam_mark: an update begins (end = False: applied and stopped are cleared) or ends (the update count advances)"""
    rc = load().rsx_adam_mark(None if state is None else C.byref(state), 1 if end else 0, stream)
    if rc:
        _chk(rc)


def replay_sample_rows(rows_ptr, m, n_batch_rows, fill, fill_ptr, seed, step, step_ptr, stream=None):
    """rsx_replay_sample_rows: rows [m] int32 := indices uniform over the first fill rows (fill, or the int64 at fill_ptr), keyed by
    (seed, step or the int64 at step_ptr); -1 everywhere on an empty ring"""
    rc = load().rsx_replay_sample_rows(rows_ptr, int(m), int(n_batch_rows), int(fill), fill_ptr, int(seed) & ((1 << 64) - 1), int(step),
                                       step_ptr, stream)
    if rc:
        _chk(rc)


def replay_add_nstep(batch, ring, n_step, gamma, stream=None):
    """rsx_replay_add_nstep: the [T][B] batch (a ReplayBatch) folded into n-step transitions and written into the ring (a ReplayRing)
    at the device's write head, in one launch; head and fill advance on the device"""
    rc = load().rsx_replay_add_nstep(None if batch is None else C.byref(batch), None if ring is None else C.byref(ring), int(n_step),
                                     float(gamma), stream)
    if rc:
        _chk(rc)


def replay_tree_geometry(capacity):
    """rsx_replay_tree_geometry: (floats of the priority tree's array, the root's level, each level's first float)"""
    floats, levels, off = C.c_int64(0), C.c_int32(0), (C.c_int64 * 8)()
    _chk(load().rsx_replay_tree_geometry(int(capacity), C.byref(floats), C.byref(levels), off))
    return int(floats.value), int(levels.value), [int(o) for o in off[:levels.value + 1]]


def replay_set_priorities(tree_ptr, state_ptr, capacity, rows_ptr, td_error_ptr, head_ptr, m, alpha, eps, stream=None):
    """rsx_replay_set_priorities: leaf[rows[t]] := (|td_error[t]| + eps)^alpha (td_error_ptr None: the running maximum; rows_ptr None:
    the m rows behind the write head at head_ptr), the largest value where rows repeat, and the touched ancestors recomputed"""
    rc = load().rsx_replay_set_priorities(tree_ptr, state_ptr, int(capacity), rows_ptr, td_error_ptr, head_ptr, int(m), float(alpha),
                                          float(eps), stream)
    if rc:
        _chk(rc)


def replay_sample_prioritized(tree_ptr, state_ptr, capacity, fill, fill_ptr, rows_ptr, weights_ptr, m, beta, beta_ptr, seed, step, step_ptr,
                              stream=None):
    """rsx_replay_sample_prioritized: rows [m] int32 and weights [m] float32 := stratified draws in proportion to the tree's leaves and
    their importance weights over the largest; -1 and 0 everywhere on an empty ring"""
    rc = load().rsx_replay_sample_prioritized(tree_ptr, state_ptr, int(capacity), int(fill), fill_ptr, rows_ptr, weights_ptr, int(m),
                                              float(beta), beta_ptr, int(seed) & ((1 << 64) - 1), int(step), step_ptr, stream)
    if rc:
        _chk(rc)


def dpg_adam_step(cfg, state, io, stream=None):
    """rsx_dpg_adam_step: clip + Adam on the critics and (with a grad_actor) the actor, each group on its own, and the Polyak step"""
    rc = load().rsx_dpg_adam_step(None if cfg is None else C.byref(cfg), None if state is None else C.byref(state),
                                  None if io is None else C.byref(io), stream)
    if rc:
        _chk(rc)


def sac_adam_step(cfg, state, io, stream=None):
    """rsx_sac_adam_step: clip + Adam on the critics, (with a grad_actor) the actor and (with a grad_log_alpha) log_alpha, each group on
    its own, and the Polyak step of the target critics"""
    rc = load().rsx_sac_adam_step(None if cfg is None else C.byref(cfg), None if state is None else C.byref(state),
                                  None if io is None else C.byref(io), stream)
    if rc:
        _chk(rc)


def _f64(a, shape):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.size != int(np.prod(shape)):
        raise ValueError(f"expected {shape} values, got {a.shape}")
    return a.reshape(shape)


class _DevArray:
    """Minimal __cuda_array_interface__ carrier so torch can wrap library-owned memory."""

    def __init__(self, ptr, shape, typestr, owner, strides=None):
        self.__cuda_array_interface__ = {
            "shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2,
            "strides": None if strides is None else tuple(int(x) for x in strides),   # bytes
        }
        self._owner = owner  # keeps the handle alive while a tensor views its memory


class Sim:
    """A batch of ``num_envs`` simulator instances on one GPU (C handle ``rsx_sim``)."""

    def __init__(self, kind, field_type, n_blue, n_yellow, time_step_ms=25, num_envs=1,
                 device_id=0):
        self._lib = load()
        h = C.c_void_p()
        _chk(self._lib.rsx_create(C.byref(h), kind, field_type, n_blue, n_yellow,
                                  int(time_step_ms), int(num_envs), int(device_id)))
        self._h = h
        self.kind, self.field_type = kind, field_type
        self.n_blue, self.n_yellow = n_blue, n_yellow
        self.num_envs, self.device_id = int(num_envs), int(device_id)
        self.n_robots = n_blue + n_yellow
        self.cmd_dim = 2 if kind == KIND_VSS else 8              # rsim.py:92-101 / :137-153
        self.state_dim = 5 + (6 if kind == KIND_VSS else 11) * self.n_robots   # Entities/Frame.py:20-47,55-92
        self._view_cache = None   # raw device pointers are fetched on first use (see _view)
        self._tview = None
        self.task = TASK_NONE

    @property
    def _view(self):
        # asking for the raw pointers tells the library that the state can change behind its back
        # (it then stops serving rsx_get_state from the copy rsx_step brought home), so the
        # single-env robosim classes, which never touch device memory, do not ask
        if self._view_cache is None:
            v = DevView()
            _chk(self._lib.rsx_dev_view_get(self._h, C.byref(v)))
            assert (v.n_robots, v.state_dim, v.cmd_dim) == (self.n_robots, self.state_dim, self.cmd_dim)
            self._view_cache = v
        return self._view_cache

    # ---- lifetime ----
    def close(self):
        if getattr(self, "_h", None):
            self._lib.rsx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _stream(stream):
        if stream is None:
            return None
        return C.c_void_p(int(stream))

    # ---- robosim surface (host f64 wire format) ----
    def get_field_params(self):
        out = (C.c_double * 17)()
        _chk(self._lib.rsx_get_field_params(self._h, out))
        return dict(zip(FIELD_KEYS, [float(x) for x in out]))

    def reset(self, ball, blue, yellow, env_mask=None, stream=None):
        B = self.num_envs
        ball = _f64(ball, (B, 4))
        blue = _f64(blue, (B, self.n_blue, 3)) if self.n_blue else None
        yellow = _f64(yellow, (B, self.n_yellow, 3)) if self.n_yellow else None
        m = None if env_mask is None else np.ascontiguousarray(env_mask, dtype=np.uint8)
        _chk(self._lib.rsx_reset(self._h, _ptr(ball), _ptr(blue), _ptr(yellow), _ptr(m),
                                 self._stream(stream)))

    def step(self, cmds, stream=None):
        cmds = _f64(cmds, (self.num_envs, self.n_robots, self.cmd_dim))
        _chk(self._lib.rsx_step(self._h, _ptr(cmds), self._stream(stream)))

    def step_state(self, cmds, copy=True):
        """step(cmds) + get_state() in one crossing (rsx_step_state, null stream): returns the [B, state_dim] float64
        state.  ``cmds`` must be a C-contiguous float64 array of B * n_robots * cmd_dim values — the lean path of the
        robosim-shaped single-env objects (no conversions, no per-call stream object).  ``copy=False`` on a handle with
        wire buffers (more than 64 envs): the commands are copied into the pinned command buffer, the step runs through
        ``rsx_step_wire`` and the result is a VIEW of the pinned state buffer — valid until the next step, no pass over
        the 8 * B * state_dim bytes on the host."""
        if not copy:
            wire = self.wire_buffers()
            if wire is not None:
                np.copyto(wire[0], np.asarray(cmds).reshape(wire[0].shape))
                rc = self._lib.rsx_step_wire(self._h, None)
                if rc:
                    _chk(rc)
                return wire[1][:, :self.state_dim]
        out = np.empty((self.num_envs, self.state_dim), dtype=np.float64)
        rc = self._lib.rsx_step_state(self._h, cmds.ctypes.data, out.ctypes.data, None)
        if rc:
            _chk(rc)
        return out

    def wire_buffers(self):
        """(cmds, state): numpy views of the handle's pinned wire-format buffers (rsx_wire_buffers; batches of more than 64 envs) —
        cmds [B, n_robots, cmd_dim] float64 to be filled before ``step_wire()``, state [B, state_dim + 2] float64 (the
        ``get_state()`` vector + the two internal rows) valid after it.  None for handles without them."""
        if getattr(self, "_wire", None) is None:
            c, st = C.c_void_p(), C.c_void_p()
            if self._lib.rsx_wire_buffers(self._h, C.byref(c), C.byref(st)) != 0:
                self._wire = False
            else:
                nc, ns = self.num_envs * self.n_robots * self.cmd_dim, self.num_envs * (self.state_dim + X_ROWS)
                cm = np.ctypeslib.as_array(C.cast(c, C.POINTER(C.c_double)), shape=(nc,)).reshape(self.num_envs, self.n_robots, self.cmd_dim)
                sv = np.ctypeslib.as_array(C.cast(st, C.POINTER(C.c_double)), shape=(ns,)).reshape(self.num_envs, self.state_dim + X_ROWS)
                self._wire = (cm, sv)
        return self._wire or None

    def step_wire(self, stream=None):
        """one step with the commands of ``wire_buffers()[0]``; the new state (all rows) lands in ``wire_buffers()[1]`` (rsx_step_wire)"""
        _chk(self._lib.rsx_step_wire(self._h, self._stream(stream)))

    def get_state(self, stream=None):
        out = np.empty((self.num_envs, self.state_dim), dtype=np.float64)
        _chk(self._lib.rsx_get_state(self._h, _ptr(out), self._stream(stream)))
        return out

    def get_state_full(self, stream=None):
        out = np.empty((self.num_envs, self.state_dim + X_ROWS), dtype=np.float64)
        _chk(self._lib.rsx_get_state_full(self._h, _ptr(out), self._stream(stream)))
        return out

    def set_state(self, state, stream=None):
        s = _f64(state, (self.num_envs, self.state_dim + X_ROWS))
        _chk(self._lib.rsx_set_state(self._h, _ptr(s), self._stream(stream)))

    # ---- device-resident path ----
    def step_dev(self, stream=None):
        _chk(self._lib.rsx_step_dev(self._h, self._stream(stream)))

    def step_dev_random(self, n=1, seed=0, first_tick=0, stream=None):
        """n steps with commands drawn on the device (Philox keyed by seed; ticks first_tick...)."""
        _chk(self._lib.rsx_step_dev_random(self._h, int(n), int(seed), int(first_tick), self._stream(stream)))

    def step_dev_flip(self, stream=None):
        """Double-buffered step_dev(): the two tensors of state_buffers() trade roles."""
        _chk(self._lib.rsx_step_dev_flip(self._h, self._stream(stream)))

    def state_buffers(self):
        """(current, other): two [state_dim+2, B] float32 views; after each step_dev_flip() the one
        that was current holds the previous frame."""
        cur, oth = C.c_void_p(), C.c_void_p()
        _chk(self._lib.rsx_state_buffers(self._h, C.byref(cur), C.byref(oth)))
        return self._rows(cur.value, self.state_dim + X_ROWS), self._rows(oth.value, self.state_dim + X_ROWS)

    def reset_dev(self, ball, blue, yellow, env_mask=None, stream=None):
        """reset() from device tensors: ball [B,4], blue [B,nb,3], yellow [B,ny,3] float32 CUDA,
        env_mask [B] uint8/bool CUDA or None.  Stream-ordered, no host copy."""
        import torch
        def prep(t, shape):
            if t is None:
                return None
            t = t.to(dtype=torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"expected {shape}, got {tuple(t.shape)}")
            return t
        B = self.num_envs
        ball = prep(ball, (B, 4))
        blue = prep(blue, (B, self.n_blue, 3)) if self.n_blue else None
        yellow = prep(yellow, (B, self.n_yellow, 3)) if self.n_yellow else None
        m = None
        if env_mask is not None:
            m = env_mask.to(dtype=torch.uint8).contiguous()
            if tuple(m.shape) != (B,):
                raise ValueError(f"env_mask must be [{B}]")
        ptr = lambda t: None if t is None else t.data_ptr()
        self._keep_reset = (ball, blue, yellow, m)   # alive until the launch has consumed them
        _chk(self._lib.rsx_reset_dev(self._h, ptr(ball), ptr(blue), ptr(yellow), ptr(m), self._stream(stream)))

    def _tensor(self, ptr, shape, typestr, strides=None):
        import torch
        return torch.as_tensor(_DevArray(ptr, shape, typestr, self, strides),
                               device=torch.device("cuda", self.device_id))

    def _rows(self, ptr, n_rows, rs=None):
        """[n_rows, B] float32 view of an SoA array whose rows are row_stride floats apart (dense unless the handle pads its rows:
        rsx.h, rsx_dev_view)"""
        rs = int(self._view.row_stride if rs is None else rs)
        return self._tensor(ptr, (n_rows, self.num_envs), "<f4", None if rs == self.num_envs else (4 * rs, 4))

    def state_tensor(self):
        """[state_dim+2, B] float32, zero-copy view of the SoA state."""
        return self._rows(self._view.state, self.state_dim + X_ROWS)

    def cmds_tensor(self):
        """[N*C, B] float32, zero-copy view of the SoA command buffer read by step_dev()."""
        return self._rows(self._view.cmds, self.n_robots * self.cmd_dim)

    # ---- fused tasks ----
    def task_attach(self, task, seed=0, env_id_base=0, max_episode_steps=0):
        _chk(self._lib.rsx_task_attach(self._h, task, seed, env_id_base, max_episode_steps))
        t = TaskView()
        _chk(self._lib.rsx_task_view_get(self._h, C.byref(t)))
        self._tview = t
        self.task = task
        self.obs_dim, self.act_dim, self.info_dim = t.obs_dim, t.act_dim, t.info_dim
        self.max_episode_steps = t.max_episode_steps

    def task_layout(self):
        """which tile layout steps this handle (rsx_task_layout): '8-lanes-per-env', 'one-lane-per-env', ..."""
        buf = C.create_string_buffer(64)
        _chk(self._lib.rsx_task_layout(self._h, buf, 64))
        return buf.value.decode()

    def task_service_wave(self):
        """whether single steps run in the paired form, a service wave next to each physics wave (rsx_task_service_wave)"""
        out = C.c_int(0)
        _chk(self._lib.rsx_task_service_wave(self._h, C.byref(out)))
        return bool(out.value)

    def placement_cache_stats(self, stream=None):
        """(resets served from the placement cache, resets placed inline), or (-1, -1) — rsx_task_placement_cache_stats"""
        out = (C.c_int64 * 2)()
        _chk(self._lib.rsx_task_placement_cache_stats(self._h, out, self._stream(stream)))
        return int(out[0]), int(out[1])

    def task_tensors(self):
        t, B = self._tview, self.num_envs
        return dict(
            obs=self._tensor(t.obs, (B, t.obs_dim), "<f4"),
            reward=self._tensor(t.reward, (B,), "<f4"),
            terminated=self._tensor(t.terminated, (B,), "|u1"),
            truncated=self._tensor(t.truncated, (B,), "|u1"),
            info=self._rows(t.info, t.info_dim, t.row_stride),
            final_obs=self._tensor(t.final_obs, (B, t.obs_dim), "<f4"),
            steps=self._tensor(t.steps, (B,), "<i4"),
            actions=self._tensor(t.actions, (B, t.act_dim), "<f4"),
            metrics=self._tensor(t.metrics, (N_METRICS,), "<i8"),
        )

    def task_reseed(self, seed, stream=None):
        """start over with another seed (rsx_task_reseed): the handle becomes what a fresh attach with that seed would be; reset next"""
        _chk(self._lib.rsx_task_reseed(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, self._stream(stream)))

    def task_reset(self, stream=None):
        _chk(self._lib.rsx_task_reset(self._h, self._stream(stream)))

    def task_reset_to(self, ball, blue, yellow, env_mask=None, stream=None):
        B = self.num_envs
        ball = _f64(ball, (B, 4))
        blue = _f64(blue, (B, self.n_blue, 3)) if self.n_blue else None
        yellow = _f64(yellow, (B, self.n_yellow, 3)) if self.n_yellow else None
        m = None if env_mask is None else np.ascontiguousarray(env_mask, dtype=np.uint8)
        _chk(self._lib.rsx_task_reset_to(self._h, _ptr(ball), _ptr(blue), _ptr(yellow), _ptr(m),
                                         self._stream(stream)))

    def task_step(self, actions_ptr=None, stream=None):
        """actions_ptr: device address of a [B][act_dim] float32 array, or None = random.
        Hot path of the Python API: plain ints go straight to ctypes (argtypes are c_void_p)."""
        rc = self._lib.rsx_task_step(self._h, actions_ptr, stream)
        if rc:
            _chk(rc)

    def task_step_n(self, n, stream=None):
        _chk(self._lib.rsx_task_step_n(self._h, int(n), self._stream(stream)))

    def task_rollout(self, n, stream=None):
        _chk(self._lib.rsx_task_rollout(self._h, int(n), self._stream(stream)))

    def task_lookahead(self, actions_ptr, n_candidates, horizon, gamma, returns_ptr, steps_ptr, flags_ptr, last_obs_ptr=None, stream=None):
        """rsx_task_lookahead: one launch that scores ``n_candidates`` action sequences of ``horizon`` steps per env from the current
        state and leaves the handle exactly as it was.  Device addresses: actions [B][K][H][act_dim] f32, returns [B][K] f32, steps
        [B][K] i32, flags [B][K] u8 (bit 0 terminated, bit 1 truncated), last_obs [B][K][obs_dim] f32 or None.  Plain ints go
        straight to ctypes."""
        rc = self._lib.rsx_task_lookahead(self._h, actions_ptr, int(n_candidates), int(horizon), float(gamma), returns_ptr, steps_ptr,
                                          flags_ptr, last_obs_ptr, stream)
        if rc:
            _chk(rc)

    def task_lookahead_sampled(self, mean_ptr, sampler, n_candidates, horizon, gamma, returns_ptr, steps_ptr, flags_ptr, last_obs_ptr=None,
                               stream=None):
        """rsx_task_lookahead_sampled: rsx_task_lookahead with the candidates drawn on the device around the plan ``mean``
        ([B][H][act_dim] f32 device address or None = zeros) by ``sampler`` (a PlanSampler, or None to pass NULL)."""
        rc = self._lib.rsx_task_lookahead_sampled(self._h, mean_ptr, None if sampler is None else C.byref(sampler), int(n_candidates),
                                                  int(horizon), float(gamma), returns_ptr, steps_ptr, flags_ptr, last_obs_ptr, stream)
        if rc:
            _chk(rc)

    def policy_num_params(self, spec):
        """rsx_policy_num_params: floats of one policy of shape ``spec`` (a PolicyMLP) on this handle's task"""
        n = C.c_int64(0)
        _chk(self._lib.rsx_policy_num_params(self._h, None if spec is None else C.byref(spec), C.byref(n)))
        return int(n.value)

    def task_lookahead_policy(self, spec, params_ptr, n_policies, horizon, gamma, returns_ptr, steps_ptr, flags_ptr, last_obs_ptr=None,
                              actions_out_ptr=None, obs_out_ptr=None, stream=None):
        """rsx_task_lookahead_policy: rsx_task_lookahead with each step's action computed by MLP policy k (``spec``: a PolicyMLP, or
        None to pass NULL; params [K][P] f32) from the observation the pair just produced.  Optional records: actions_out
        [B][K][H][act_dim], obs_out [B][K][H][obs_dim] (entries of steps a pair did not simulate are not written)."""
        rc = self._lib.rsx_task_lookahead_policy(self._h, None if spec is None else C.byref(spec), params_ptr, int(n_policies), int(horizon),
                                                 float(gamma), returns_ptr, steps_ptr, flags_ptr, last_obs_ptr, actions_out_ptr, obs_out_ptr,
                                                 stream)
        if rc:
            _chk(rc)

    def task_lookahead_match(self, spec, params_ptr, n_actors, seats, opp_spec, opp_params_ptr, n_opponents, opp_seats, horizon, gamma, out,
                             stream=None):
        """rsx_task_lookahead_match: ``task_lookahead_policy`` on a VSS-v0 handle against an opponent: pair (env, k, m) is actor k of
        ``spec`` (params [K][P] f32, ``seats`` = 1 or n_blue robots seated) against opponent m of ``opp_spec`` (params [M][P2] f32,
        ``opp_seats`` = 1 or n_yellow); ``out``: a MatchOut of device addresses, or None to pass NULL."""
        ref = lambda v: None if v is None else C.byref(v)   # noqa: E731
        rc = self._lib.rsx_task_lookahead_match(self._h, ref(spec), params_ptr, int(n_actors), int(seats), ref(opp_spec), opp_params_ptr,
                                                int(n_opponents), int(opp_seats), int(horizon), float(gamma), ref(out), stream)
        if rc:
            _chk(rc)

    def task_collect_policy(self, spec, params_ptr, sigma_ptr, noise_seed, n_steps, out, stream=None):
        """rsx_task_collect_policy: ``n_steps`` steps of the handle's envs under MLP policy ``spec`` (a PolicyMLP, or None to pass
        NULL; params [P] f32) in one launch, with auto-reset; ``out``: a CollectOut of device addresses ([T][B] records), or None to
        pass NULL.  ``sigma_ptr``: [act_dim] f32 device address of the Gaussian head's standard deviations, or None = deterministic."""
        rc = self._lib.rsx_task_collect_policy(self._h, None if spec is None else C.byref(spec), params_ptr, sigma_ptr,
                                               int(noise_seed) & 0xFFFFFFFFFFFFFFFF, int(n_steps), None if out is None else C.byref(out), stream)
        if rc:
            _chk(rc)

    def task_collect_gaussian(self, spec, params_ptr, cfg, n_steps, out, log_std_ptr=None, stream=None):
        """rsx_task_collect_gaussian: ``task_collect_policy`` under a state-dependent tanh-squashed Gaussian head: ``spec`` a PolicyMLP
        with out_act = ACT_NONE whose output layer is 2 * act_dim wide (params [P] f32), ``cfg`` a CollectGaussianCfg, ``out`` a
        CollectOut; each may be None to pass NULL.  ``log_std_ptr``: [T][B][act_dim] f32 device address for the clamped log-std, or None."""
        ref = lambda v: None if v is None else C.byref(v)   # noqa: E731
        rc = self._lib.rsx_task_collect_gaussian(self._h, ref(spec), params_ptr, ref(cfg), int(n_steps), ref(out), log_std_ptr, stream)
        if rc:
            _chk(rc)

    def task_collect_selfplay(self, spec, params_ptr, sigma_ptr, opp_spec, opp_params_ptr, opp_sigma_ptr, noise_seed, n_steps, out, sp,
                              stream=None):
        """rsx_task_collect_selfplay: ``task_collect_policy`` on a VSS-v0 handle with yellow robot 0 driven by a second MLP policy
        (``opp_spec``, params [P2] f32, ``opp_sigma_ptr`` [2] or None) from the mirrored observation; ``sp``: a SelfplayOut of device
        addresses (the opponent's records), or None to pass NULL."""
        ref = lambda v: None if v is None else C.byref(v)   # noqa: E731
        rc = self._lib.rsx_task_collect_selfplay(self._h, ref(spec), params_ptr, sigma_ptr, ref(opp_spec), opp_params_ptr, opp_sigma_ptr,
                                                 int(noise_seed) & 0xFFFFFFFFFFFFFFFF, int(n_steps), ref(out), ref(sp), stream)
        if rc:
            _chk(rc)

    def task_collect_team(self, spec, params_ptr, sigma_ptr, seats, opp_spec, opp_params_ptr, opp_sigma_ptr, opp_seats, noise_seed, n_steps,
                          out, stream=None):
        """rsx_task_collect_team: ``task_collect_selfplay`` with ``seats`` (1 or n_blue) blue robots driven by ``spec`` and ``opp_seats``
        (0 with ``opp_spec`` None, 1 or n_yellow) yellow robots by ``opp_spec``, each seat from its own row; ``out``: a TeamOut of device
        addresses (records with a seat axis behind B), or None to pass NULL."""
        ref = lambda v: None if v is None else C.byref(v)   # noqa: E731
        rc = self._lib.rsx_task_collect_team(self._h, ref(spec), params_ptr, sigma_ptr, int(seats), ref(opp_spec), opp_params_ptr,
                                             opp_sigma_ptr, int(opp_seats), int(noise_seed) & 0xFFFFFFFFFFFFFFFF, int(n_steps), ref(out),
                                             stream)
        if rc:
            _chk(rc)

    def critic_num_params(self, spec):
        """rsx_critic_num_params: floats of one critic of shape ``spec`` (a PolicyMLP with out_act = ACT_NONE) on this handle's task"""
        n = C.c_int64(0)
        _chk(self._lib.rsx_critic_num_params(self._h, None if spec is None else C.byref(spec), C.byref(n)))
        return int(n.value)

    def task_advantages(self, spec, params_ptr, gamma, lam, n_steps, n_envs, inp, out, stream=None):
        """rsx_task_advantages: values of critic ``spec`` (a PolicyMLP with out_act = ACT_NONE, or None to pass NULL; params [P] f32
        with act_dim = 1) on a [T][B] batch and its GAE advantages and returns, in two launches.  ``inp``: an AdvIn, ``out``: an AdvOut
        of device addresses (None passes NULL).  Reads and writes nothing of the envs."""
        rc = self._lib.rsx_task_advantages(self._h, None if spec is None else C.byref(spec), params_ptr, float(gamma), float(lam),
                                           int(n_steps), int(n_envs), None if inp is None else C.byref(inp),
                                           None if out is None else C.byref(out), stream)
        if rc:
            _chk(rc)

    def ppo_gradient_workspace(self, actor, critic, n_rows, max_workgroups=0):
        """rsx_ppo_gradient_workspace: bytes of scratch rsx_task_ppo_gradient needs for a minibatch of ``n_rows`` rows"""
        n = C.c_int64(0)
        _chk(self._lib.rsx_ppo_gradient_workspace(self._h, None if actor is None else C.byref(actor), None if critic is None else C.byref(critic),
                                                  int(n_rows), int(max_workgroups), C.byref(n)))
        return int(n.value)

    def task_ppo_gradient(self, actor, actor_params_ptr, log_std_ptr, critic, critic_params_ptr, inp, cfg, out, stream=None):
        """rsx_task_ppo_gradient: gradients of the PPO loss with respect to the actor's parameters, log_std and the critic's parameters on
        a minibatch, in three launches.  ``actor`` / ``critic``: PolicyMLP specs, ``inp``: a PpoIn, ``cfg``: a PpoCfg, ``out``: a PpoOut
        of device addresses (None passes NULL).  Reads and writes nothing of the envs."""
        rc = self._lib.rsx_task_ppo_gradient(self._h, None if actor is None else C.byref(actor), actor_params_ptr, log_std_ptr,
                                             None if critic is None else C.byref(critic), critic_params_ptr,
                                             None if inp is None else C.byref(inp), None if cfg is None else C.byref(cfg),
                                             None if out is None else C.byref(out), stream)
        if rc:
            _chk(rc)

    def ppo_update_workspace(self, actor, critic, n_batch_rows, minibatches, max_workgroups=0):
        """rsx_ppo_update_workspace: (bytes of scratch rsx_task_ppo_update needs, the offset of its int32 rows in it)"""
        n, off = C.c_int64(0), C.c_int64(0)
        _chk(self._lib.rsx_ppo_update_workspace(self._h, None if actor is None else C.byref(actor), None if critic is None else C.byref(critic),
                                                int(n_batch_rows), int(minibatches), int(max_workgroups), C.byref(n), C.byref(off)))
        return int(n.value), int(off.value)

    def task_ppo_update(self, actor, actor_params_ptr, log_std_ptr, critic, critic_params_ptr, inp, cfg, ucfg, adam, state, stats_ptr,
                        workspace_ptr, stream=None):
        """rsx_task_ppo_update: the whole update phase of PPO enqueued by one call — normalisation, per epoch a permutation, per minibatch
        the gradients and the clip + Adam step; the parameters are updated in place.  Reads and writes nothing of the envs."""
        b = lambda x: None if x is None else C.byref(x)   # noqa: E731
        rc = self._lib.rsx_task_ppo_update(self._h, b(actor), actor_params_ptr, log_std_ptr, b(critic), critic_params_ptr, b(inp), b(cfg),
                                           b(ucfg), b(adam), b(state), stats_ptr, workspace_ptr, stream)
        if rc:
            _chk(rc)

    def dpg_gradient_workspace(self, actor, critic, n_critics, n_rows, max_workgroups=0):
        """rsx_dpg_gradient_workspace: bytes of scratch rsx_task_dpg_gradient needs for a minibatch of ``n_rows`` rows"""
        n = C.c_int64(0)
        _chk(self._lib.rsx_dpg_gradient_workspace(self._h, None if actor is None else C.byref(actor), None if critic is None else C.byref(critic),
                                                  int(n_critics), int(n_rows), int(max_workgroups), C.byref(n)))
        return int(n.value)

    def task_dpg_gradient(self, actor, actor_params_ptr, target_actor_params_ptr, critic, critic_params_ptr, target_critic_params_ptr, inp,
                          cfg, out, stream=None):
        """rsx_task_dpg_gradient: gradients of the TD3 / DDPG losses with respect to the actor's and the critics' parameters on a
        minibatch of replayed transitions, in four launches.  ``actor`` / ``critic``: PolicyMLP specs, ``inp``: a DpgIn, ``cfg``: a
        DpgCfg, ``out``: a DpgOut of device addresses (None passes NULL).  Reads and writes nothing of the envs."""
        b = lambda x: None if x is None else C.byref(x)   # noqa: E731
        rc = self._lib.rsx_task_dpg_gradient(self._h, b(actor), actor_params_ptr, target_actor_params_ptr, b(critic), critic_params_ptr,
                                             target_critic_params_ptr, b(inp), b(cfg), b(out), stream)
        if rc:
            _chk(rc)

    def task_dpg_gradient_w(self, actor, actor_params_ptr, target_actor_params_ptr, critic, critic_params_ptr, target_critic_params_ptr, inp,
                            cfg, out, per, stream=None):
        """rsx_task_dpg_gradient_w: task_dpg_gradient with ``per``, a GradPer: per-row discounts in the target, per-entry weights on the
        critic loss and the per-entry TD error (one more launch)"""
        b = lambda x: None if x is None else C.byref(x)   # noqa: E731
        rc = self._lib.rsx_task_dpg_gradient_w(self._h, b(actor), actor_params_ptr, target_actor_params_ptr, b(critic), critic_params_ptr,
                                               target_critic_params_ptr, b(inp), b(cfg), b(out), b(per), stream)
        if rc:
            _chk(rc)

    def sac_gradient_workspace(self, actor, critic, n_critics, n_rows, max_workgroups=0):
        """rsx_sac_gradient_workspace: bytes of scratch rsx_task_sac_gradient needs for a minibatch of ``n_rows`` rows"""
        n = C.c_int64(0)
        _chk(self._lib.rsx_sac_gradient_workspace(self._h, None if actor is None else C.byref(actor), None if critic is None else C.byref(critic),
                                                  int(n_critics), int(n_rows), int(max_workgroups), C.byref(n)))
        return int(n.value)

    def task_sac_gradient(self, actor, actor_params_ptr, critic, critic_params_ptr, target_critic_params_ptr, log_alpha_ptr, inp, cfg, out,
                          stream=None):
        """rsx_task_sac_gradient: gradients of the soft actor-critic losses with respect to the actor's and the critics' parameters and
        the log-temperature on a minibatch of replayed transitions, in six launches.  ``actor`` / ``critic``: PolicyMLP specs (the actor's
        output layer 2 * act_dim wide, out_act = ACT_NONE), ``inp``: a DpgIn, ``cfg``: a SacCfg, ``out``: a SacOut of device addresses
        (None passes NULL).  Reads and writes nothing of the envs."""
        b = lambda x: None if x is None else C.byref(x)   # noqa: E731
        rc = self._lib.rsx_task_sac_gradient(self._h, b(actor), actor_params_ptr, b(critic), critic_params_ptr, target_critic_params_ptr,
                                             log_alpha_ptr, b(inp), b(cfg), b(out), stream)
        if rc:
            _chk(rc)

    def task_sac_gradient_w(self, actor, actor_params_ptr, critic, critic_params_ptr, target_critic_params_ptr, log_alpha_ptr, inp, cfg, out,
                            per, stream=None):
        """rsx_task_sac_gradient_w: task_sac_gradient with ``per``, a GradPer: per-row discounts in the target, per-entry weights on the
        critic loss and the per-entry TD error (one more launch)"""
        b = lambda x: None if x is None else C.byref(x)   # noqa: E731
        rc = self._lib.rsx_task_sac_gradient_w(self._h, b(actor), actor_params_ptr, b(critic), critic_params_ptr, target_critic_params_ptr,
                                               log_alpha_ptr, b(inp), b(cfg), b(out), b(per), stream)
        if rc:
            _chk(rc)

    def dpg_update_workspace(self, actor, critic, n_critics, n_rows, max_workgroups=0):
        """rsx_dpg_update_workspace: (bytes of scratch rsx_task_dpg_update needs, the offset of its int32 rows in it)"""
        n, off = C.c_int64(0), C.c_int64(0)
        _chk(self._lib.rsx_dpg_update_workspace(self._h, None if actor is None else C.byref(actor), None if critic is None else C.byref(critic),
                                                int(n_critics), int(n_rows), int(max_workgroups), C.byref(n), C.byref(off)))
        return int(n.value), int(off.value)

    def task_dpg_update(self, actor, actor_params_ptr, target_actor_params_ptr, critic, critic_params_ptr, target_critic_params_ptr, inp,
                        cfg, ucfg, adam, state, stats_ptr, workspace_ptr, stream=None):
        """rsx_task_dpg_update: the whole update phase of TD3 / DDPG enqueued by one call — per gradient step the row draw, the
        gradients and the clip + Adam + Polyak step; the four parameter tensors are updated in place.  Reads and writes nothing of
        the envs."""
        b = lambda x: None if x is None else C.byref(x)   # noqa: E731
        rc = self._lib.rsx_task_dpg_update(self._h, b(actor), actor_params_ptr, target_actor_params_ptr, b(critic), critic_params_ptr,
                                           target_critic_params_ptr, b(inp), b(cfg), b(ucfg), b(adam), b(state), stats_ptr, workspace_ptr,
                                           stream)
        if rc:
            _chk(rc)

    def sac_update_workspace(self, actor, critic, n_critics, n_rows, max_workgroups=0):
        """rsx_sac_update_workspace: (bytes of scratch rsx_task_sac_update needs, the offset of its int32 rows in it)"""
        n, off = C.c_int64(0), C.c_int64(0)
        _chk(self._lib.rsx_sac_update_workspace(self._h, None if actor is None else C.byref(actor), None if critic is None else C.byref(critic),
                                                int(n_critics), int(n_rows), int(max_workgroups), C.byref(n), C.byref(off)))
        return int(n.value), int(off.value)

    def task_sac_update(self, actor, actor_params_ptr, critic, critic_params_ptr, target_critic_params_ptr, log_alpha_ptr, inp, cfg, ucfg,
                        adam, state, stats_ptr, workspace_ptr, stream=None):
        """rsx_task_sac_update: the whole update phase of soft actor-critic enqueued by one call — per gradient step the row draw, the
        gradients and the three-group clip + Adam + Polyak step; the actor, the critics, the target critics and log_alpha are updated
        in place.  Reads and writes nothing of the envs."""
        b = lambda x: None if x is None else C.byref(x)   # noqa: E731
        rc = self._lib.rsx_task_sac_update(self._h, b(actor), actor_params_ptr, b(critic), critic_params_ptr, target_critic_params_ptr,
                                           log_alpha_ptr, b(inp), b(cfg), b(ucfg), b(adam), b(state), stats_ptr, workspace_ptr, stream)
        if rc:
            _chk(rc)

    def plan_candidates(self, mean_ptr, sampler, n_candidates, horizon, out_ptr, stream=None):
        """rsx_plan_candidates: the actions rsx_task_lookahead_sampled uses, written to out [B][K][H][act_dim] f32"""
        rc = self._lib.rsx_plan_candidates(self._h, mean_ptr, None if sampler is None else C.byref(sampler), int(n_candidates), int(horizon),
                                           out_ptr, stream)
        if rc:
            _chk(rc)

    def plan_update(self, mean_ptr, sampler, n_candidates, horizon, returns_ptr, temperature, new_mean_ptr, best_ptr=None, stream=None):
        """rsx_plan_update: fold returns [B][K] into new_mean [B][H][act_dim] (temperature 0: the best candidate; > 0: the
        softmax-weighted mean) by drawing the candidates again; best [B] i32 or None"""
        rc = self._lib.rsx_plan_update(self._h, mean_ptr, None if sampler is None else C.byref(sampler), int(n_candidates), int(horizon),
                                       returns_ptr, float(temperature), new_mean_ptr, best_ptr, stream)
        if rc:
            _chk(rc)

    def task_enable_capture(self, stream=None):
        """rsx_task_enable_capture: move the step counter to device memory so that stepping calls can be captured into a
        hipGraph (torch.cuda.CUDAGraph) and replayed.  Call once, outside any capture."""
        _chk(self._lib.rsx_task_enable_capture(self._h, self._stream(stream)))

    def task_tick(self, stream=None):
        """fused steps taken since attach (rsx_task_tick)"""
        n = C.c_uint32(0)
        _chk(self._lib.rsx_task_tick(self._h, C.byref(n), self._stream(stream)))
        return int(n.value)

    def check_finite(self, stream=None):
        """Number of non-finite floats in state / obs / reward / info (debugging aid; synchronises)."""
        n = C.c_int64(0)
        _chk(self._lib.rsx_check_finite(self._h, C.byref(n), self._stream(stream)))
        return int(n.value)

    def task_checkpoint(self, stream=None):
        """bytes of a checkpoint of the fused run (rsx_task_checkpoint_save): state, episode bookkeeping, noise
        state, step counter, metrics — see include/rsx.h"""
        n = C.c_size_t(0)
        _chk(self._lib.rsx_task_checkpoint_size(self._h, C.byref(n)))
        blob = np.empty(n.value, dtype=np.uint8)
        _chk(self._lib.rsx_task_checkpoint_save(self._h, blob.ctypes.data_as(C.c_void_p), n.value, self._stream(stream)))
        return blob

    def task_restore(self, blob, stream=None):
        """continue from ``task_checkpoint()`` (same simulator, batch, task, seed and env_id_base)"""
        blob = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else blob, dtype=np.uint8)
        _chk(self._lib.rsx_task_checkpoint_load(self._h, blob.ctypes.data_as(C.c_void_p), blob.size, self._stream(stream)))

    # ---- per-env physics (include/rsx.h: rsx_physics_*) ----
    def physics_enable(self, stream=None):
        """every env gets its own physics parameters, all at the defaults (the lane-group kernels step the handle from now on)"""
        _chk(self._lib.rsx_physics_enable(self._h, self._stream(stream)))
        self.physics_on = True

    def physics_set(self, values, env_mask=None, stream=None):
        """``values``: [len(PHYSICS_PARAMS), num_envs] float32, NaN = keep.  A numpy array is checked on the host (RsxError for an
        out-of-range value, nothing changed); a device tensor (anything with ``data_ptr``) is read on the device, where an env
        with an invalid value keeps its values and is counted by ``physics_errors()``.  ``env_mask``: [num_envs] bytes in the
        same memory, or None."""
        want = (len(PHYSICS_PARAMS), self.num_envs)
        if hasattr(values, "data_ptr"):
            if tuple(values.shape) != want or not values.is_contiguous() or str(values.dtype) != "torch.float32":
                raise ValueError(f"values must be a contiguous float32 tensor of shape {want}")
            m = None
            if env_mask is not None:
                if tuple(env_mask.shape) != (self.num_envs,) or env_mask.element_size() != 1 or not env_mask.is_contiguous():
                    raise ValueError("env_mask must be a contiguous 1-byte tensor of shape (num_envs,)")
                m = C.c_void_p(env_mask.data_ptr())
            _chk(self._lib.rsx_physics_set(self._h, C.c_void_p(values.data_ptr()), 1, m, self._stream(stream)))
            return
        v = np.ascontiguousarray(values, dtype=np.float32)
        if v.shape != want:
            raise ValueError(f"values must have shape {want}, got {v.shape}")
        m = None if env_mask is None else np.ascontiguousarray(env_mask, dtype=np.uint8)
        _chk(self._lib.rsx_physics_set(self._h, _ptr(v), 0, _ptr(m), self._stream(stream)))

    def physics_get(self, which=PHYS_RAW, stream=None):
        """[len(PHYSICS_PARAMS) | len(PHYSICS_COEFS), num_envs] float32 on the host (synchronises)"""
        out = np.zeros((len(PHYSICS_PARAMS) if which == PHYS_RAW else len(PHYSICS_COEFS), self.num_envs), dtype=np.float32)
        _chk(self._lib.rsx_physics_get(self._h, int(which), _ptr(out), self._stream(stream)))
        return out

    def physics_randomize(self, lo, hi, param_mask, stream=None):
        """redraw the parameters of ``param_mask`` (bit p = PHYSICS_PARAMS[p]) in [lo[p], hi[p]) at every episode start"""
        lo = np.ascontiguousarray(lo, dtype=np.float32).reshape(len(PHYSICS_PARAMS))
        hi = np.ascontiguousarray(hi, dtype=np.float32).reshape(len(PHYSICS_PARAMS))
        _chk(self._lib.rsx_physics_randomize(self._h, _ptr(lo), _ptr(hi), C.c_uint32(int(param_mask)), self._stream(stream)))

    def physics_errors(self, stream=None):
        """envs refused by device-side ``physics_set`` calls since the last call"""
        n = C.c_int64(0)
        _chk(self._lib.rsx_physics_errors(self._h, C.byref(n), self._stream(stream)))
        return int(n.value)

    # ---- trace evaluation (include/rsx.h: rsx_trace_*; rsoccer_amd/sysid.py) ----
    def trace_load(self, frames, cmds, anchors, stream=None):
        """``frames``: [n_frames, state_dim + 2] float64 (the ``get_state_full()`` layout), ``cmds``: [n_frames - 1, n_robots,
        cmd_dim] float64, ``anchors``: frame indices, ``num_envs`` a multiple of their count (env e: candidate e // n_anchors
        from anchor e % n_anchors).  Needs ``physics_enable()`` and no task; synchronises."""
        f = np.ascontiguousarray(frames, dtype=np.float64)
        if f.ndim != 2 or f.shape[1] != self.state_dim + X_ROWS or f.shape[0] < 2:
            raise ValueError(f"frames must have shape (n_frames >= 2, {self.state_dim + X_ROWS}), got {f.shape}")
        c = _f64(cmds, (f.shape[0] - 1, self.n_robots, self.cmd_dim))
        a = np.ascontiguousarray(anchors, dtype=np.int32).reshape(-1)
        _chk(self._lib.rsx_trace_load(self._h, _ptr(f), _ptr(c), int(f.shape[0]), _ptr(a), int(a.size), self._stream(stream)))

    def trace_eval(self, horizon, loss, stream=None):
        """one launch: ``loss`` (a contiguous float32 device tensor [len(TRACE_TERMS), num_envs]) receives every env's summed
        squared deviation from the loaded trace over ``horizon`` steps; the final states stay in the state buffer.  No
        synchronisation."""
        if tuple(loss.shape) != (len(TRACE_TERMS), self.num_envs) or not loss.is_contiguous() or str(loss.dtype) != "torch.float32":
            raise ValueError(f"loss must be a contiguous float32 tensor of shape {(len(TRACE_TERMS), self.num_envs)}")
        _chk(self._lib.rsx_trace_eval(self._h, int(horizon), C.c_void_p(loss.data_ptr()), self._stream(stream)))

    # ---- batched rgb frames (include/rsx.h: rsx_render_*; rsoccer_amd/vec/render.py) ----
    _render_key = None   # the view rsx_render draws (the values of RENDER_VIEW_KEYS), and its frame size
    _render_hw = None

    def render_open(self, view, stream=None, key=None):
        """make ``view`` (a dict in ``Render/raster.py``'s format or a ``RenderView``) the one ``render`` draws; returns the frame size
        (H, W).  A view the handle has not seen is drawn on the host and uploaded (synchronises; not inside a capture); one it has
        seen is only selected, and the view already current costs no FFI crossing.  Views stay allocated until ``close()`` — a
        captured ``render`` keeps drawing the view it was captured with — so a handle takes at most 16 different ones.
        ``key``: the view's values as a tuple, for callers that keep it (``vec/render.py``)."""
        v = view if isinstance(view, RenderView) else RenderView.from_dict(view)
        if key is None:
            key = tuple(getattr(v, k) for k in RENDER_VIEW_KEYS)
        if key != self._render_key:
            _chk(self._lib.rsx_render_open(self._h, C.byref(v), self._stream(stream)))
            self._render_key, self._render_hw = key, render_size(v)
        return self._render_hw

    def render(self, env_ids_ptr, n, channels_first, out_ptr, stream=None):
        """one launch: ``n`` frames of the current state into the device buffer at ``out_ptr`` ([n, H, W, 3] uint8, or [n, 3, H, W]);
        ``env_ids_ptr``: device address of ``n`` int32 env ids, or None = envs 0..n-1.  Plain ints go straight to ctypes."""
        rc = self._lib.rsx_render(self._h, env_ids_ptr, n, 1 if channels_first else 0, out_ptr, stream)
        if rc:
            _chk(rc)

    def render_errors(self, stream=None):
        """frames whose env id was out of range since the last call (they show the bare field)"""
        n = C.c_int64(0)
        _chk(self._lib.rsx_render_errors(self._h, C.byref(n), self._stream(stream)))
        return int(n.value)

    # ---- transfer of running episodes (include/rsx.h: rsx_task_transfer) ----
    def task_transfer(self, src, dst_ids_ptr=None, src_ids_ptr=None, n=0, stream=None):
        """one launch (two when ``src is self``): env ``src_ids[i]`` of ``src`` is copied into env ``dst_ids[i]`` of this handle for
        ``i < n`` — state, episode bookkeeping, noise state, observations, flags, per-env physics; metrics, step counter and random
        keys stay this handle's.  ``*_ids_ptr``: device addresses of ``n`` int32 ids, or None = envs 0..n-1.  Destination ids must
        be distinct; pairs with an id out of range are skipped and counted (``task_transfer_errors``).  Plain ints go straight to
        ctypes."""
        rc = self._lib.rsx_task_transfer(self._h, src._h, dst_ids_ptr, src_ids_ptr, int(n), stream)
        if rc:
            _chk(rc)

    def task_transfer_errors(self, stream=None):
        """pairs skipped by transfers into this handle since the last call (an id out of range); synchronises"""
        n = C.c_int64(0)
        _chk(self._lib.rsx_task_transfer_errors(self._h, C.byref(n), self._stream(stream)))
        return int(n.value)

    def metrics_fold(self, stream=None):
        """make the device copy of the episode counters (``task_tensors()["metrics"]``) exact, on ``stream``"""
        _chk(self._lib.rsx_metrics_fold(self._h, self._stream(stream)))

    def read_metrics(self, stream=None):
        out = np.zeros(N_METRICS, dtype=np.int64)
        _chk(self._lib.rsx_read_metrics(self._h, _ptr(out), self._stream(stream)))
        return out


def device_count():
    return int(load().rsx_device_count())


def physics_defaults(kind):
    """the per-env physics parameters' defaults of a robot class (rsx_physics_defaults): float32 [len(PHYSICS_PARAMS)]"""
    out = np.zeros(len(PHYSICS_PARAMS), dtype=np.float32)
    _chk(load().rsx_physics_defaults(int(kind), _ptr(out)))
    return out


def physics_derive(kind, time_step_ms, raw):
    """the coefficients the kernels derive from one parameter set (rsx_physics_derive): float32 [len(PHYSICS_COEFS)]"""
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    if raw.shape != (len(PHYSICS_PARAMS),):
        raise ValueError(f"expected {len(PHYSICS_PARAMS)} parameters, got {raw.shape}")
    out = np.zeros(len(PHYSICS_COEFS), dtype=np.float32)
    _chk(load().rsx_physics_derive(int(kind), int(time_step_ms), _ptr(raw), _ptr(out)))
    return out


def render_view_reference(kind):
    """the reference's fixed window of a robot class as a view dict (rsx_render_view_reference): raster.py's VSS_VIEW / SSL_VIEW"""
    v = RenderView()
    _chk(load().rsx_render_view_reference(int(kind), C.byref(v)))
    return v.to_dict()


def render_size(view):
    """(H, W) of the frames of a view (rsx_render_size); RsxError for an invalid view.  No device needed."""
    v = view if isinstance(view, RenderView) else RenderView.from_dict(view)
    w, h = C.c_int(0), C.c_int(0)
    _chk(load().rsx_render_size(C.byref(v), C.byref(w), C.byref(h)))
    return int(h.value), int(w.value)


def render_field(view):
    """the static field image of a view, uint8 [H, W, 3] (rsx_render_field): equals ``FieldRaster(view)._field``.  No device needed."""
    v = view if isinstance(view, RenderView) else RenderView.from_dict(view)
    h, w = render_size(v)
    out = np.empty((h, w, 3), dtype=np.uint8)
    _chk(load().rsx_render_field(C.byref(v), _ptr(out)))
    return out
