"""Fused batched tasks (one kernel launch per ``step()``)."""
import functools
import inspect

import numpy as np

from rsoccer_amd import _lib
from rsoccer_amd import gymshim as gym
from rsoccer_amd.vec.render import RenderMixin

_VSS_INFO = ("goal_score", "move", "ball_grad", "energy", "goals_blue", "goals_yellow")
_SD_INFO = ("goal", "rbt_in_gk_area", "done_ball_out", "done_ball_out_right", "done_rbt_out",
            "ball_dist", "ball_grad", "energy")


def batched_space(single, n):
    """the space of ``n`` copies of ``single`` (a Box), as ``gymnasium.vector`` describes a vector env: shape ``(n,) + single.shape``"""
    low = np.broadcast_to(single.low, (n,) + tuple(single.shape)).copy()
    high = np.broadcast_to(single.high, (n,) + tuple(single.shape)).copy()
    return gym.spaces.Box(low=low, high=high, shape=(n,) + tuple(single.shape), dtype=single.dtype)


def _records_ctor_kwargs(init):
    """wraps an ``__init__`` so that the OUTERMOST constructor call leaves its arguments, by name, in ``self._ctor_kw`` — what
    ``fork()`` builds its sibling from, whatever keywords a subclass adds"""
    sig = inspect.signature(init)

    @functools.wraps(init)
    def wrapped(self, *args, **kw):
        if "_ctor_kw" not in self.__dict__:
            bound = sig.bind(self, *args, **kw)
            rec = {}
            for name, val in list(bound.arguments.items())[1:]:
                if sig.parameters[name].kind is inspect.Parameter.VAR_KEYWORD:
                    rec.update(val)
                else:
                    rec[name] = val
            self._ctor_kw = rec
        return init(self, *args, **kw)
    return wrapped


class VecFusedEnv(RenderMixin):
    """``num_envs`` copies of a fused task on one GPU.

    ``reset()`` -> ``(obs, info)``; ``step(actions)`` -> ``(obs, reward, terminated, truncated,
    info)`` like ``gymnasium.vector`` with same-step auto-reset: when an env's episode ends
    (task ``done`` or the registry's TimeLimit) it is re-placed inside the same call, ``obs``
    already holds the first observation of its next episode and ``info["final_obs"]`` the
    terminal one.  All returned arrays are torch tensors on the env's device that VIEW the
    engine's buffers (no copies): they are overwritten by the next ``step()``.

    Every random draw (placement, OU noise, random actions) is keyed by
    ``(seed, env_id_base + env index, episode, step)``, so results do not depend on
    ``num_envs`` or on how a population of envs is split over GPUs.
    """

    KIND = None
    TASK = None
    FIELD_TYPE = 0
    N_BLUE = N_YELLOW = 0
    INFO_KEYS = ()
    TIME_STEP = 0.025

    @_records_ctor_kwargs
    def __init__(self, num_envs, device=0, seed=0, env_id_base=0, max_episode_steps=None,
                 field_type=None, physics=None, physics_ranges=None):
        import torch
        self._torch = torch
        self.num_envs = int(num_envs)
        self.device = torch.device("cuda", int(device))
        ft = self.FIELD_TYPE if field_type is None else field_type
        self.sim = _lib.Sim(self.KIND, ft, self.N_BLUE, self.N_YELLOW, int(self.TIME_STEP * 1000),
                            self.num_envs, int(device))
        self.sim.task_attach(self.TASK, int(seed), int(env_id_base), int(max_episode_steps or 0))
        self._seed = int(seed)   # (what plan() derives its default noise key from; follows reset(seed=...))
        # per-env physics: only when asked for (an env built without these keywords steps with the compiled-in constants)
        self._physics = physics is not None or physics_ranges is not None
        if self._physics:
            self.sim.physics_enable(self._stream())
            if physics:
                self.set_physics(**physics)
            if physics_ranges:
                self.set_physics_randomization(**physics_ranges)
        self.max_episode_steps = self.sim.max_episode_steps
        self._t = self.sim.task_tensors()
        self._info_views = None
        self._pending = None
        self.field = self.sim.get_field_params()
        self.single_action_space = gym.spaces.Box(low=-1, high=1, shape=(self.sim.act_dim,), dtype=np.float32)
        self.single_observation_space = gym.spaces.Box(low=-1.2, high=1.2, shape=(self.sim.obs_dim,), dtype=np.float32)
        # gymnasium.vector convention: action_space / observation_space describe the batch, single_* one env
        self.action_space = batched_space(self.single_action_space, self.num_envs)
        self.observation_space = batched_space(self.single_observation_space, self.num_envs)

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        if "__init__" in cls.__dict__:
            cls.__init__ = _records_ctor_kwargs(cls.__dict__["__init__"])

    # ---- gym-like surface ----
    def _stream(self):
        # raw handle of torch's current stream on the env's device (the private getter skips the
        # Stream object; the public API is the fallback)
        try:
            return self._torch._C._cuda_getCurrentRawStream(self.device.index)
        except AttributeError:
            return self._torch.cuda.current_stream(self.device).cuda_stream

    def _info(self):
        """The info dict of step(): tensor VIEWS of the engine's buffers, so one dict serves every
        step (a fresh shallow copy is returned: callers may add keys)."""
        if self._info_views is None:
            t = self._t
            info = {k: t["info"][i] for i, k in enumerate(self.INFO_KEYS)}
            info["final_obs"] = t["final_obs"]
            info["episode_steps"] = t["steps"]
            self._info_views = info
        return dict(self._info_views)

    def reset(self, *, seed=None, options=None):
        """New random placement for every env.  ``seed=None`` (the usual call): the random streams chosen at construction go on
        (episode counters advance).  ``seed=<int>``: start over — every random stream (placements, OU noise, random actions) is
        re-keyed and all counters cleared, exactly as if the env had just been constructed with that seed
        (``rsx_task_reseed``; env ``i`` keeps its global id ``env_id_base + i``, which distinguishes the envs' streams)."""
        if seed is not None:
            self.sim.task_reseed(int(seed), self._stream())
            self._seed = int(seed)
        self.sim.task_reset(self._stream())
        return self._t["obs"], {}

    def reset_to(self, ball, blue, yellow, env_mask=None):
        """Start new episodes on explicit placements (arrays as ``robosim.reset``: ball [B,4],
        blue [B,nb,3], yellow [B,ny,3]); ``env_mask`` selects the envs to touch."""
        self.sim.task_reset_to(ball, blue, yellow, env_mask, self._stream())
        return self._t["obs"], {}

    def step(self, actions=None):
        """actions: ``[num_envs, act_dim]`` float32 (torch CUDA tensor = zero-copy; numpy is
        staged through a device buffer) or None for uniform random actions drawn on device."""
        torch = self._torch
        ptr = None
        if actions is not None:
            want = (self.num_envs, self.sim.act_dim)
            if tuple(np.shape(actions)) != want:   # checked on the INPUT: copy_ below would broadcast
                raise ValueError(f"actions must be [{want[0]}, {want[1]}], got {tuple(np.shape(actions))}")
            if isinstance(actions, torch.Tensor):
                a = actions
                if a.device != self.device or a.dtype != torch.float32 or not a.is_contiguous():
                    a = a.to(device=self.device, dtype=torch.float32).contiguous()
            else:
                a = self._t["actions"]
                # pageable host memory: a blocking copy (non_blocking would read a temporary)
                a.copy_(torch.from_numpy(np.ascontiguousarray(actions, dtype=np.float32)))
            self._keep = a  # keep the tensor alive until the launch has consumed it
            ptr = a.data_ptr()
        self.sim.task_step(ptr, self._stream())
        t = self._t
        return t["obs"], t["reward"], t["terminated"], t["truncated"], self._info()

    def lookahead(self, actions, gamma=1.0, return_obs=False):
        """Score candidate action sequences from where every env stands now, without touching the env (``rsx_task_lookahead``).

        ``actions``: ``[num_envs, K, H, act_dim]`` float32 — for each env ``K`` candidate sequences of ``H`` actions (a CUDA float32
        contiguous torch tensor is zero-copy; anything else is converted the way ``step()`` converts).  One launch simulates every
        (env, candidate) pair for up to ``H`` steps with the candidate's actions and the env's REAL future draws (the OU noise of the
        other robots), so the result is exact: bit for bit what ``H`` calls of ``step()`` with those actions would return.  A pair
        stops at its env's first episode end; nothing behind it (placement, auto-reset) is simulated.

        Returns a dict of fresh device tensors (caller-owned: not views of engine buffers, not overwritten by the next call):
        ``return`` ``[num_envs, K]`` float32 — ``sum_t gamma^t reward_t`` up to the pair's end, ``steps`` int32 — steps simulated
        (``< H`` exactly when the episode ended inside the horizon), ``terminated`` / ``truncated`` bool — at the last simulated
        step, and with ``return_obs=True`` ``last_obs`` ``[num_envs, K, obs_dim]`` — the observation after the last simulated step
        (the terminal one if the pair ended).  The env is left exactly as it was: the next ``step()`` does what it would have done.
        Capturable into a ``torch.cuda.CUDAGraph`` after ``enable_graph_capture()``."""
        torch = self._torch
        shape = tuple(np.shape(actions))
        if len(shape) != 4 or shape[0] != self.num_envs or shape[3] != self.sim.act_dim:   # checked on the INPUT
            raise ValueError(f"actions must be [{self.num_envs}, K, H, {self.sim.act_dim}], got {shape}")
        K, H = int(shape[1]), int(shape[2])
        if K < 1 or H < 1:
            raise ValueError(f"actions must hold at least one candidate and one step, got K={K}, H={H}")
        gamma = float(gamma)
        if not np.isfinite(gamma):
            raise ValueError("gamma must be finite")
        if isinstance(actions, torch.Tensor):
            a = actions
            if a.device != self.device or a.dtype != torch.float32 or not a.is_contiguous():
                a = a.to(device=self.device, dtype=torch.float32).contiguous()
        else:
            a = torch.from_numpy(np.ascontiguousarray(actions, dtype=np.float32)).to(self.device)
        B = self.num_envs
        ret = torch.empty((B, K), dtype=torch.float32, device=self.device)
        steps = torch.empty((B, K), dtype=torch.int32, device=self.device)
        flags = torch.empty((B, K), dtype=torch.uint8, device=self.device)
        obs = torch.empty((B, K, self.sim.obs_dim), dtype=torch.float32, device=self.device) if return_obs else None
        self.sim.task_lookahead(a.data_ptr(), K, H, gamma, ret.data_ptr(), steps.data_ptr(), flags.data_ptr(),
                                obs.data_ptr() if return_obs else None, self._stream())
        self._keep_plan = a   # alive until the launch has consumed it
        out = {"return": ret, "steps": steps, "terminated": (flags & 1).bool(), "truncated": (flags & 2).bool()}
        if return_obs:
            out["last_obs"] = obs
        return out

    def lookahead_policy(self, policy, params, horizon, gamma=1.0, return_obs=False, return_actions=False, return_policy_obs=False):
        """``lookahead()`` closed-loop: ``K`` MLP policies instead of ``K`` action sequences (``rsx_task_lookahead_policy``).

        ``policy``: an ``rsoccer_amd.vec.policy.MLPPolicy`` for this env's ``obs_dim`` / ``act_dim``; ``params``: ``[K, P]`` float32,
        one flat parameter vector per policy (``MLPPolicy.pack`` / ``from_module``), shared by all envs.  Pair (env, k) starts from where
        the env stands now; the action of each simulated step is policy ``k``'s answer to the observation the pair just produced — at
        step 0 the env's current ``obs`` row — evaluated inside the launch.  Everything else is ``lookahead()``'s: the env's real
        future draws, a pair stops at its env's first episode end, the env is left exactly as it was.  ``horizon=max_episode_steps``
        straight after ``reset()`` scores whole episodes.

        Returns the dict of ``lookahead()`` (``return``, ``steps``, ``terminated``, ``truncated``, ``last_obs`` with
        ``return_obs=True``) plus, on request, ``actions`` ``[num_envs, K, H, act_dim]`` — the action taken at every simulated step —
        and ``policy_obs`` ``[num_envs, K, H, obs_dim]`` — the observation it was computed from; entries behind a pair's end stay zero.
        ``lookahead(out["actions"])`` from the same state returns the same bits.  Capturable after ``enable_graph_capture()``."""
        torch = self._torch
        from rsoccer_amd.vec.policy import MLPPolicy
        if not isinstance(policy, MLPPolicy):
            raise ValueError("policy must be an rsoccer_amd.vec.policy.MLPPolicy")
        H, gamma = int(horizon), float(gamma)
        if H < 1:
            raise ValueError(f"horizon must be >= 1, got {horizon}")
        if not np.isfinite(gamma):
            raise ValueError("gamma must be finite")
        if self.sim.act_dim != policy.act_dim or self.sim.obs_dim != policy.obs_dim:
            raise ValueError(f"the policy maps {policy.obs_dim} -> {policy.act_dim}, the env {self.sim.obs_dim} -> {self.sim.act_dim}")
        shape = tuple(np.shape(params))   # checked on the INPUT, as lookahead() checks its actions
        if len(shape) != 2 or shape[0] < 1 or shape[1] != policy.num_params:
            raise ValueError(f"params must be [K >= 1, {policy.num_params}], got {shape}")
        K = int(shape[0])
        if isinstance(params, torch.Tensor):
            p = params
            if p.device != self.device or p.dtype != torch.float32 or not p.is_contiguous():
                p = p.to(device=self.device, dtype=torch.float32).contiguous()
        else:
            p = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float32)).to(self.device)
        B, dev = self.num_envs, self.device
        ret = torch.empty((B, K), dtype=torch.float32, device=dev)
        steps = torch.empty((B, K), dtype=torch.int32, device=dev)
        flags = torch.empty((B, K), dtype=torch.uint8, device=dev)
        obs = torch.empty((B, K, self.sim.obs_dim), dtype=torch.float32, device=dev) if return_obs else None
        acts = torch.zeros((B, K, H, self.sim.act_dim), dtype=torch.float32, device=dev) if return_actions else None
        pobs = torch.zeros((B, K, H, self.sim.obs_dim), dtype=torch.float32, device=dev) if return_policy_obs else None
        self.sim.task_lookahead_policy(policy.spec(), p.data_ptr(), K, H, gamma, ret.data_ptr(), steps.data_ptr(), flags.data_ptr(),
                                       obs.data_ptr() if return_obs else None, acts.data_ptr() if return_actions else None,
                                       pobs.data_ptr() if return_policy_obs else None, self._stream())
        self._keep_plan = p   # alive until the launch has consumed it
        out = {"return": ret, "steps": steps, "terminated": (flags & 1).bool(), "truncated": (flags & 2).bool()}
        if return_obs:
            out["last_obs"] = obs
        if return_actions:
            out["actions"] = acts
        if return_policy_obs:
            out["policy_obs"] = pobs
        return out

    def lookahead_match(self, policy, params, opponent, opponent_params, horizon, gamma=1.0, team=False, opponent_team=False,
                        return_obs=False, return_actions=False, return_policy_obs=False):
        """``lookahead_policy()`` against an opponent (VSS-v0 with equal teams, ``rsx_task_lookahead_match``): ``K`` actors against ``M``
        opponents from every env's current state, in ONE launch.

        ``policy`` / ``params`` ``[K, P]``: the actors (blue), as ``lookahead_policy()`` takes them; ``opponent`` / ``opponent_params``
        ``[M, P2]``: the opponents (yellow), an ``MLPPolicy`` of this env's dims whose layers and hidden may differ.  Triple
        (env, k, m) starts from where the env stands now and runs to the env's first episode end or ``horizon`` steps.  A step is
        ``collect(opponent=...)``'s step with deterministic heads: the opponent answers the mirrored observation of the same instant;
        ``team=True`` seats every blue robot under actor ``k`` and ``opponent_team=True`` every yellow robot under opponent ``m``, each
        from its seat's row, as ``collect(team=..., opponent_team=...)`` does.  The draws are the env's real future ones and the env is
        left exactly as it was.  ``horizon=max_episode_steps`` straight after ``reset()`` plays whole episodes: all ``K x M`` pairs
        from the same ``B`` start states.

        Returns a dict of fresh device tensors: ``return`` ``[B, K, M]`` (blue's), ``steps``, ``terminated``, ``truncated`` and
        ``result`` (int8: +1 the pair ended on a goal for blue, -1 on one for yellow, 0 otherwise); with ``return_obs`` ``last_obs``
        ``[B, K, M, obs_dim]``; with ``return_actions`` ``actions`` ``[B, K, M, H, 2]`` and ``opponent_actions``; with
        ``return_policy_obs`` ``policy_obs`` ``[B, K, M, H, obs_dim]`` and ``opponent_obs``.  A side's recordings gain a seat axis
        behind ``H`` when that side's flag is set (``[B, K, M, H, S, 2]``); entries behind a pair's end stay zero.
        ``rsoccer_amd.vec.policy.match_table(out)`` folds the envs into ``[K, M]`` wins, draws, losses and mean return.
        Capturable after ``enable_graph_capture()``."""
        torch = self._torch
        from rsoccer_amd.vec.policy import MLPPolicy
        if not isinstance(policy, MLPPolicy):
            raise ValueError("policy must be an rsoccer_amd.vec.policy.MLPPolicy")
        if not isinstance(opponent, MLPPolicy):
            raise ValueError("opponent must be an rsoccer_amd.vec.policy.MLPPolicy")
        if self.TASK != _lib.TASK_VSS_V0 or self.N_BLUE != self.N_YELLOW:
            raise ValueError(f"lookahead_match: a match is played on VSS-v0 with equal teams, this env is {type(self).__name__}")
        H, gamma = int(horizon), float(gamma)
        if H < 1:
            raise ValueError(f"horizon must be >= 1, got {horizon}")
        if not np.isfinite(gamma):
            raise ValueError("gamma must be finite")
        if self.sim.act_dim != policy.act_dim or self.sim.obs_dim != policy.obs_dim:
            raise ValueError(f"the policy maps {policy.obs_dim} -> {policy.act_dim}, the env {self.sim.obs_dim} -> {self.sim.act_dim}")
        if self.sim.act_dim != opponent.act_dim or self.sim.obs_dim != opponent.obs_dim:
            raise ValueError(f"the opponent maps {opponent.obs_dim} -> {opponent.act_dim}, the env {self.sim.obs_dim} -> {self.sim.act_dim}")
        if params is None or opponent_params is None:
            raise ValueError("params and opponent_params must not be None")
        shape, oshape = tuple(np.shape(params)), tuple(np.shape(opponent_params))   # checked on the INPUT: a 1-D vector is not promoted
        if len(shape) != 2 or shape[0] < 1 or shape[1] != policy.num_params:
            raise ValueError(f"params must be [K >= 1, {policy.num_params}], got {shape}")
        if len(oshape) != 2 or oshape[0] < 1 or oshape[1] != opponent.num_params:
            raise ValueError(f"opponent_params must be [M >= 1, {opponent.num_params}], got {oshape}")
        K, M = int(shape[0]), int(oshape[0])
        B, dev, OD, AD = self.num_envs, self.device, self.sim.obs_dim, self.sim.act_dim

        def device_params(v):
            if isinstance(v, torch.Tensor):
                t = v.detach()
                if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                    t = t.to(device=dev, dtype=torch.float32).contiguous()
                return t
            return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)

        p, op = device_params(params), device_params(opponent_params)
        S, S2 = (self.N_BLUE if team else 1), (self.N_YELLOW if opponent_team else 1)
        f32 = dict(dtype=torch.float32, device=dev)
        ret = torch.empty((B, K, M), **f32)
        steps = torch.empty((B, K, M), dtype=torch.int32, device=dev)
        flags = torch.empty((B, K, M), dtype=torch.uint8, device=dev)
        result = torch.empty((B, K, M), dtype=torch.int8, device=dev)
        last = torch.empty((B, K, M, OD), **f32) if return_obs else None
        acts = torch.zeros((B, K, M, H, S, AD), **f32) if return_actions else None
        oacts = torch.zeros((B, K, M, H, S2, AD), **f32) if return_actions else None
        pobs = torch.zeros((B, K, M, H, S, OD), **f32) if return_policy_obs else None
        oobs = torch.zeros((B, K, M, H, S2, OD), **f32) if return_policy_obs else None
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        rec = _lib.MatchOut(ptr(ret), ptr(steps), ptr(flags), ptr(result), ptr(last), ptr(acts), ptr(pobs), ptr(oacts), ptr(oobs))
        self.sim.task_lookahead_match(policy.spec(), p.data_ptr(), K, S, opponent.spec(), op.data_ptr(), M, S2, H, gamma, rec, self._stream())
        self._keep_plan = (p, op)   # alive until the launch has consumed them
        out = {"return": ret, "steps": steps, "terminated": (flags & 1).bool(), "truncated": (flags & 2).bool(), "result": result}
        if return_obs:
            out["last_obs"] = last
        seat = lambda t, flag: t if flag else t[:, :, :, :, 0]   # noqa: E731  (the seat axis only where that side's flag is set)
        if return_actions:
            out["actions"], out["opponent_actions"] = seat(acts, team), seat(oacts, opponent_team)
        if return_policy_obs:
            out["policy_obs"], out["opponent_obs"] = seat(pobs, team), seat(oobs, opponent_team)
        return out

    def collect(self, policy, params, steps, log_std=None, noise_seed=None, iteration=0, return_final_obs=False,
                critic=None, critic_params=None, gamma=0.99, lam=0.95, opponent=None, opponent_params=None, opponent_log_std=None,
                team=False, opponent_team=False, deterministic=False):
        """Advance the envs ``steps`` steps under an MLP policy in ONE launch and return the on-policy batch
        (``rsx_task_collect_policy``): what a PPO / A2C loop calls between two updates.

        ``policy``: an ``rsoccer_amd.vec.policy.MLPPolicy`` for this env's ``obs_dim`` / ``act_dim``; ``params``: ``[P]`` float32, its
        flat parameters (``MLPPolicy.pack`` / ``from_module``).  Step 0 answers the env's current ``obs``; episode ends are handled
        inside the launch (same-step auto-reset), and row ``t + 1`` of ``obs`` for an env that ended at ``t`` is the first
        observation of its next episode.  The env ends up exactly where ``steps`` calls of ``step(out["actions"][t])`` leave it —
        state, counters, metrics and checkpoint, bit for bit.

        ``log_std``: ``[act_dim]`` (or a scalar) — the log standard deviations of a Gaussian head: ``sample = mean + exp(log_std) * eps``
        and ``action = out_act(sample)``, where ``mean`` is the output layer BEFORE ``out_act``.  ``None``: deterministic
        (``sample = mean``).  ``eps`` is keyed by ``noise_seed``, the global env id and the step counter; ``noise_seed`` defaults to a
        64-bit mix (splitmix64) of the env's seed and ``iteration``, the way ``plan()`` derives its sample seed — pass the update's
        index as ``iteration``.  A ``log_std`` given as host data (float, list, numpy) must be finite; a device tensor is not
        checked (that would synchronise).

        Returns a dict of fresh caller-owned device tensors (``T = steps``, ``B = num_envs``): ``obs`` ``[T, B, obs_dim]`` — the
        observation each action answered, ``actions`` ``[T, B, act_dim]``, ``reward`` ``[T, B]``, ``terminated`` / ``truncated``
        ``[T, B]`` bool, and ``next_obs`` — the env's ``obs`` VIEW after the call, for the bootstrap value.  With
        ``return_final_obs=True`` also ``final_obs`` ``[T, B, obs_dim]``: zeros, except at ended rows the terminal observation.  With
        ``log_std`` also ``mean``, ``sample`` ``[T, B, act_dim]`` and ``log_prob`` ``[T, B]``: the density of ``sample`` under
        ``N(mean, exp(log_std))`` summed over the components, computed in torch — the PRE-``out_act`` density (no tanh / clip
        correction; it cancels in PPO's ratio as long as the trainer evaluates the same pre-activation density).
        With ``critic`` (an ``MLPCritic``) and ``critic_params`` the batch also carries ``value``, ``advantage`` and ``return``
        ``[T, B]``: ``advantages(batch, critic, critic_params, gamma, lam)`` on the batch just collected (``final_obs`` is then always
        recorded and returned).  Without a critic the returned dict and the launches are what they were.

        Self-play (VSS-v0 only, ``rsx_task_collect_selfplay``): with ``opponent`` (an ``MLPPolicy`` of this env's dims; its layers and
        hidden may differ from the agent's) and ``opponent_params`` ``[P2]``, yellow robot 0 is driven by that policy inside the same
        launch instead of by its Ornstein-Uhlenbeck noise.  The opponent sees the mirrored observation — team colours swapped, the
        field turned by 180 degrees, the agent's layout — and answers the same instant as the agent; ``opponent_log_std`` gives it a
        Gaussian head of its own (the agent's noise key under another domain word: the heads never share a draw).  Rewards, flags,
        ``final_obs``, ``next_obs`` and the metrics stay the agent's.  The dict gains ``opponent_obs`` ``[T, B, obs_dim]``,
        ``opponent_actions`` ``[T, B, 2]`` and, with a head, ``opponent_mean``, ``opponent_sample`` and ``opponent_log_prob``.  The env
        can be handed back to ``step()`` or a plain ``collect()`` at any time: yellow 0's noise state kept advancing, unused.  A typical
        loop copies the learner's parameters into ``opponent_params`` every few updates (``examples/selfplay_vss.py``).  With
        ``opponent=None`` the call, its launches and its outputs are exactly what they are without these keywords.

        Team play (VSS-v0 with equal teams, ``rsx_task_collect_team``): ``team=True`` seats ALL blue robots under ``policy`` /
        ``params`` / ``log_std`` — blue seat ``i`` is blue robot ``i`` and sees the env's row with "own" slots 0 and ``i`` exchanged —
        and ``opponent_team=True`` (needs ``opponent``) seats all yellow robots under the opponent's, each from the mirrored row under
        the same exchange.  The flags combine freely: ``team=True`` alone, with the one-robot opponent, or with the opponent's team.
        Each seat's head draws noise of its own (the seat index is part of the counter; seat 0 draws what it draws without the flags).
        The reward stays VSS-v0's one reward per env.  When either flag is set, ``obs``, ``actions``, ``mean``, ``sample``,
        ``log_prob`` and ``final_obs`` (with a critic also ``value``, ``advantage``, ``return``) and the ``opponent_*`` tensors gain a
        seat axis behind ``B`` — ``obs`` ``[T, B, S, obs_dim]``, ``log_prob`` ``[T, B, S]`` — while ``reward``, ``terminated`` and
        ``truncated`` stay ``[T, B]``; ``next_obs`` is a fresh ``[B, S, obs_dim]`` tensor (the env's own ``obs`` view still holds seat 0's) and the
        dict also carries ``opponent_next_obs`` and, with ``return_final_obs``, ``opponent_final_obs``.  ``critic=`` evaluates the
        critic on every seat's rows and runs GAE per (env, seat) with the shared reward and flags.
        ``rsoccer_amd.vec.policy.seat_rows(batch)`` turns such a batch into the ``[T, B * S, ...]`` mapping ``advantages()``,
        ``ppo_gradient()`` and ``ppo_update()`` take.  With both flags false nothing changes.

        Soft actor-critic's actor (``rsx_task_collect_gaussian``): with ``policy`` an ``MLPGaussianPolicy`` — the output layer gives mean
        and log-std per state — the head is ``log_std = clamp(raw, policy.log_std_min, policy.log_std_max)``, ``sample = mean +
        exp(log_std) * eps`` (the same ``eps`` as above) and ``action = tanh(sample)``; ``deterministic=True`` takes ``action =
        tanh(mean)`` without a draw.  The dict is the one above (``obs``, ``actions``, ``reward``, ``terminated``, ``truncated``,
        ``next_obs``, ``final_obs`` on request) plus ``mean``, ``log_std``, ``sample`` ``[T, B, act_dim]`` and ``log_prob`` ``[T, B]``: the
        density of the ACTION, tanh correction included (``rsoccer_amd.vec.policy.squashed_log_prob``, computed in torch).  ``ReplayBuffer.add()`` takes
        it as it is.  ``log_std=``, ``critic=``, ``opponent=``, ``team=`` and ``opponent_team=`` are refused with this policy (a squashed
        head for self-play seats is a different feature); ``deterministic`` is refused with every other policy unless it is ``False``.
        Capturable into a ``torch.cuda.CUDAGraph`` after ``enable_graph_capture()``: every replay draws fresh noise."""
        torch = self._torch
        from rsoccer_amd.vec.policy import MLPGaussianPolicy, MLPPolicy
        if not isinstance(policy, MLPPolicy):
            raise ValueError("policy must be an rsoccer_amd.vec.policy.MLPPolicy")
        T = int(steps)
        if T < 1:
            raise ValueError(f"steps must be >= 1, got {steps}")
        if self.sim.act_dim != policy.act_dim or self.sim.obs_dim != policy.obs_dim:
            raise ValueError(f"the policy maps {policy.obs_dim} -> {policy.act_dim}, the env {self.sim.obs_dim} -> {self.sim.act_dim}")
        if isinstance(policy, MLPGaussianPolicy):
            for name, v in (("log_std", log_std), ("critic", critic), ("critic_params", critic_params), ("opponent", opponent),
                            ("opponent_params", opponent_params), ("opponent_log_std", opponent_log_std)):
                if v is not None:
                    raise ValueError(f"{name} cannot be combined with an MLPGaussianPolicy (its head is its own)")
            for name, v in (("team", team), ("opponent_team", opponent_team)):
                if v:
                    raise ValueError(f"{name} cannot be combined with an MLPGaussianPolicy (a squashed head for seats is a different feature)")
            return self._collect_gaussian(policy, params, T, noise_seed, iteration, return_final_obs, bool(deterministic))
        if deterministic is not False:
            raise ValueError("deterministic is an MLPGaussianPolicy's keyword: a plain MLPPolicy is deterministic without log_std")
        if critic is not None:
            cp = self._critic_args(critic, critic_params, gamma, lam)   # (refused before anything is enqueued)
            return_final_obs = True
        elif critic_params is not None:
            raise ValueError("critic_params given without a critic")
        shape = tuple(np.shape(params))   # checked on the INPUT, as lookahead_policy() checks its parameters
        if shape != (policy.num_params,):
            raise ValueError(f"params must be [{policy.num_params}] (one policy), got {shape}")
        if opponent is None:
            for name, v in (("opponent_params", opponent_params), ("opponent_log_std", opponent_log_std)):
                if v is not None:
                    raise ValueError(f"{name} given without an opponent")
        else:   # (refused before anything is enqueued)
            if not isinstance(opponent, MLPPolicy):
                raise ValueError("opponent must be an rsoccer_amd.vec.policy.MLPPolicy")
            if self.TASK != _lib.TASK_VSS_V0 or self.N_BLUE != self.N_YELLOW:
                raise ValueError(f"opponent: self-play drives yellow robot 0 of VSS-v0 with equal teams, this env is {type(self).__name__}")
            if self.sim.act_dim != opponent.act_dim or self.sim.obs_dim != opponent.obs_dim:
                raise ValueError(f"the opponent maps {opponent.obs_dim} -> {opponent.act_dim}, the env {self.sim.obs_dim} -> {self.sim.act_dim}")
            if opponent_params is None:
                raise ValueError("opponent_params must not be None")
            oshape = tuple(np.shape(opponent_params))
            if oshape != (opponent.num_params,):
                raise ValueError(f"opponent_params must be [{opponent.num_params}] (one policy), got {oshape}")
        team, opponent_team = bool(team), bool(opponent_team)
        if opponent_team and opponent is None:
            raise ValueError("opponent_team given without an opponent")
        if (team or opponent_team) and (self.TASK != _lib.TASK_VSS_V0 or self.N_BLUE != self.N_YELLOW):
            raise ValueError(f"{'team' if team else 'opponent_team'}: team play seats the robots of VSS-v0 with equal teams, "
                             f"this env is {type(self).__name__}")
        dev, B, OD, AD = self.device, self.num_envs, self.sim.obs_dim, self.sim.act_dim

        def device_params(v):
            if isinstance(v, torch.Tensor):
                t = v.detach()
                if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                    t = t.to(device=dev, dtype=torch.float32).contiguous()
                return t
            return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)

        def head(v, name):
            """(log_std [AD] on the device, sigma = exp(log_std)) of a Gaussian head, or (None, None)"""
            if v is None:
                return None, None
            if isinstance(v, torch.Tensor):
                t = v.detach().to(device=dev, dtype=torch.float32)
            else:
                host = np.asarray(v, dtype=np.float32)
                if not np.all(np.isfinite(host)):
                    raise ValueError(f"{name} must be finite")
                t = torch.from_numpy(np.array(host, dtype=np.float32, copy=True)).to(dev)   # (keeps a scalar 0-dimensional)
            if t.dim() == 0:
                t = t.expand(AD)
            if tuple(t.shape) != (AD,):
                raise ValueError(f"{name} must be a scalar or [{AD}], got {tuple(t.shape)}")
            return t, t.exp().contiguous()

        p = device_params(params)
        ls, sigma = head(log_std, "log_std")
        ols, osigma = head(opponent_log_std, "opponent_log_std")
        if noise_seed is None:
            noise_seed = self._collect_noise_seed(iteration)
        f32 = dict(dtype=torch.float32, device=dev)
        if team or opponent_team:
            op = None if opponent is None else device_params(opponent_params)
            out = self._collect_team(policy, p, ls, sigma, self.N_BLUE if team else 1, opponent, op, ols, osigma,
                                     0 if opponent is None else self.N_YELLOW if opponent_team else 1, noise_seed, T, return_final_obs)
            if critic is not None:
                from rsoccer_amd.vec.policy import seat_rows
                S = out["obs"].shape[2]
                adv = self._advantages(seat_rows(out), critic, cp, float(gamma), float(lam), False)
                out.update({k: v.view(T, B, S) for k, v in adv.items()})
            return out
        obs = torch.empty((T, B, OD), **f32)
        acts = torch.empty((T, B, AD), **f32)
        rew = torch.empty((T, B), **f32)
        flags = torch.empty((T, B), dtype=torch.uint8, device=dev)
        fobs = torch.zeros((T, B, OD), **f32) if return_final_obs else None
        mean = torch.empty((T, B, AD), **f32) if sigma is not None else None
        smp = torch.empty((T, B, AD), **f32) if sigma is not None else None
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        rec = _lib.CollectOut(ptr(obs), ptr(acts), ptr(rew), ptr(flags), ptr(fobs), ptr(mean), ptr(smp))
        if opponent is None:
            self.sim.task_collect_policy(policy.spec(), p.data_ptr(), ptr(sigma), noise_seed, T, rec, self._stream())
            self._keep_plan = (p, sigma)   # alive until the launch has consumed them
        else:
            op = device_params(opponent_params)
            oobs = torch.empty((T, B, OD), **f32)
            oacts = torch.empty((T, B, AD), **f32)
            omean = torch.empty((T, B, AD), **f32) if osigma is not None else None
            osmp = torch.empty((T, B, AD), **f32) if osigma is not None else None
            sp = _lib.SelfplayOut(ptr(oobs), ptr(oacts), ptr(omean), ptr(osmp))
            self.sim.task_collect_selfplay(policy.spec(), p.data_ptr(), ptr(sigma), opponent.spec(), op.data_ptr(), ptr(osigma), noise_seed,
                                           T, rec, sp, self._stream())
            self._keep_plan = (p, sigma, op, osigma)
        out = {"obs": obs, "actions": acts, "reward": rew, "terminated": (flags & 1).bool(), "truncated": (flags & 2).bool(),
               "next_obs": self._t["obs"]}
        if opponent is not None:
            out["opponent_obs"], out["opponent_actions"] = oobs, oacts
            if osigma is not None:
                out["opponent_mean"], out["opponent_sample"] = omean, osmp
                z = (osmp - omean) / osigma
                out["opponent_log_prob"] = (-0.5 * z * z - ols - 0.9189385332046727).sum(-1)
        if return_final_obs:
            out["final_obs"] = fobs
        if sigma is not None:
            out["mean"], out["sample"] = mean, smp
            z = (smp - mean) / sigma
            out["log_prob"] = (-0.5 * z * z - ls - 0.9189385332046727).sum(-1)   # 0.5 * log(2 pi)
        if critic is not None:
            out.update(self._advantages(out, critic, cp, float(gamma), float(lam), False))
        return out

    def _collect_noise_seed(self, iteration):
        """collect()'s default noise seed: splitmix64 of (seed, iteration), as _plan_sampler"""
        m = (1 << 64) - 1
        z = (self._seed + 0x9E3779B97F4A7C15 * (int(iteration) + 1)) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return z ^ (z >> 31)

    def _collect_gaussian(self, policy, params, T, noise_seed, iteration, return_final_obs, deterministic):
        """collect()'s launch and batch under an MLPGaussianPolicy (rsx_task_collect_gaussian); policy, T and the keywords checked"""
        torch = self._torch
        from rsoccer_amd.vec.policy import squashed_log_prob
        shape = tuple(np.shape(params))
        if shape != (policy.num_params,):
            raise ValueError(f"params must be [{policy.num_params}] (one policy, the output layer 2 * act_dim wide), got {shape}")
        dev, B, OD, AD = self.device, self.num_envs, self.sim.obs_dim, self.sim.act_dim
        if isinstance(params, torch.Tensor):
            p = params.detach()
            if p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
                p = p.to(device=dev, dtype=torch.float32).contiguous()
        else:
            p = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float32)).to(dev)
        if noise_seed is None:
            noise_seed = self._collect_noise_seed(iteration)
        f32 = dict(dtype=torch.float32, device=dev)
        obs = torch.empty((T, B, OD), **f32)
        acts, mean, smp, ls = (torch.empty((T, B, AD), **f32) for _ in range(4))
        rew = torch.empty((T, B), **f32)
        flags = torch.empty((T, B), dtype=torch.uint8, device=dev)
        fobs = torch.zeros((T, B, OD), **f32) if return_final_obs else None
        rec = _lib.CollectOut(obs.data_ptr(), acts.data_ptr(), rew.data_ptr(), flags.data_ptr(), None if fobs is None else fobs.data_ptr(),
                              mean.data_ptr(), smp.data_ptr())
        cfg = _lib.CollectGaussianCfg(int(noise_seed) & 0xFFFFFFFFFFFFFFFF, policy.log_std_min, policy.log_std_max, int(deterministic), 0)
        self.sim.task_collect_gaussian(policy.spec(), p.data_ptr(), cfg, T, rec, ls.data_ptr(), self._stream())
        self._keep_plan = (p,)   # alive until the launch has consumed it
        out = {"obs": obs, "actions": acts, "reward": rew, "terminated": (flags & 1).bool(), "truncated": (flags & 2).bool(),
               "next_obs": self._t["obs"]}
        if return_final_obs:
            out["final_obs"] = fobs
        out["mean"], out["log_std"], out["sample"] = mean, ls, smp
        eps = (smp - mean) / ls.exp()   # (deterministic: 0, the density at the mode)
        out["log_prob"] = squashed_log_prob(eps, ls, smp)
        return out

    def _collect_team(self, policy, p, ls, sigma, seats, opponent, op, ols, osigma, opp_seats, noise_seed, T, return_final_obs):
        """collect()'s launch and batch with seats (rsx_task_collect_team); every argument checked and on the device already"""
        torch = self._torch
        dev, B, OD, AD = self.device, self.num_envs, self.sim.obs_dim, self.sim.act_dim
        f32 = dict(dtype=torch.float32, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731

        def side(S, sig):
            """one side's record: (tensors by name, the TeamSideOut of their addresses)"""
            if S == 0:
                return {}, _lib.TeamSideOut()
            t = {"obs": torch.empty((T, B, S, OD), **f32), "actions": torch.empty((T, B, S, AD), **f32),
                 "mean": torch.empty((T, B, S, AD), **f32) if sig is not None else None,
                 "sample": torch.empty((T, B, S, AD), **f32) if sig is not None else None,
                 "final_obs": torch.zeros((T, B, S, OD), **f32) if return_final_obs else None,
                 "next_obs": torch.empty((B, S, OD), **f32)}
            return t, _lib.TeamSideOut(*(ptr(t[k]) for k in ("obs", "actions", "mean", "sample", "final_obs", "next_obs")))

        rew = torch.empty((T, B), **f32)
        flags = torch.empty((T, B), dtype=torch.uint8, device=dev)
        a, a_out = side(seats, sigma)
        o, o_out = side(opp_seats, osigma)
        rec = _lib.TeamOut(ptr(rew), ptr(flags), a_out, o_out)
        self.sim.task_collect_team(policy.spec(), p.data_ptr(), ptr(sigma), seats, None if opponent is None else opponent.spec(), ptr(op),
                                   ptr(osigma), opp_seats, noise_seed, T, rec, self._stream())
        self._keep_plan = (p, sigma, op, osigma)   # alive until the launch has consumed them
        out = {"obs": a["obs"], "actions": a["actions"], "reward": rew, "terminated": (flags & 1).bool(), "truncated": (flags & 2).bool(),
               "next_obs": a["next_obs"]}
        for pre, t, lsd, sig in (("", a, ls, sigma), ("opponent_", o, ols, osigma)):
            if not t:
                continue
            out[pre + "obs"], out[pre + "actions"], out[pre + "next_obs"] = t["obs"], t["actions"], t["next_obs"]
            if return_final_obs:
                out[pre + "final_obs"] = t["final_obs"]
            if sig is not None:
                out[pre + "mean"], out[pre + "sample"] = t["mean"], t["sample"]
                z = (t["sample"] - t["mean"]) / sig
                out[pre + "log_prob"] = (-0.5 * z * z - lsd - 0.9189385332046727).sum(-1)   # 0.5 * log(2 pi)
        return out

    def _critic_args(self, critic, params, gamma, lam):
        """what advantages() checks of its critic and scalars; returns the parameters as a device tensor"""
        torch = self._torch
        from rsoccer_amd.vec.policy import MLPCritic
        if not isinstance(critic, MLPCritic):
            raise ValueError("critic must be an rsoccer_amd.vec.policy.MLPCritic")
        if critic.obs_dim != self.sim.obs_dim:
            raise ValueError(f"the critic reads {critic.obs_dim} floats, the env's observation has {self.sim.obs_dim}")
        for name, v in (("gamma", gamma), ("lam", lam)):
            if not (np.isfinite(float(v)) and 0.0 <= float(v) <= 1.0):
                raise ValueError(f"{name} must be in [0, 1], got {v}")
        if params is None:
            raise ValueError("critic_params must not be None")
        shape = tuple(np.shape(params))
        if shape != (critic.num_params,):
            raise ValueError(f"critic params must be [{critic.num_params}], got {shape}")
        if isinstance(params, torch.Tensor):
            p = params.detach()
            if p.device != self.device or p.dtype != torch.float32 or not p.is_contiguous():
                p = p.to(device=self.device, dtype=torch.float32).contiguous()
        else:
            p = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float32)).to(self.device)
        return p

    def advantages(self, batch, critic, params, gamma=0.99, lam=0.95, return_next_values=False):
        """Values of an MLP critic on a collected batch and its GAE advantages and returns, in two launches
        (``rsx_task_advantages``): what a PPO / A2C loop does between ``collect()`` and its gradient step.

        ``batch``: a mapping with ``obs`` ``[T, B, obs_dim]`` float32, ``reward`` ``[T, B]`` float32, ``terminated`` / ``truncated``
        ``[T, B]`` bool or uint8, ``next_obs`` ``[B, obs_dim]`` float32 — the observation after the last step — and optionally
        ``final_obs`` ``[T, B, obs_dim]``: what ``collect(..., return_final_obs=True)`` returns; the tensors of a ``step()`` loop,
        stacked, serve as well.  All CUDA tensors on the env's device, contiguous; anything else is a ``ValueError`` naming the
        offender.  ``T`` and ``B`` come from ``obs`` (``B`` need not be ``num_envs``).  ``critic``: an
        ``rsoccer_amd.vec.policy.MLPCritic`` for this env's ``obs_dim``; ``params``: its flat ``[P]`` float32 parameters.

        A terminated row bootstraps from 0, a row that was only truncated from ``V(final_obs[t])`` (0 without ``final_obs``), any
        other from the next row's value, the last one from ``V(next_obs)``; the float32 recurrence is written out in
        ``include/rsx.h``.  ``value[t, e]`` is bit for bit ``collect()``'s ``mean[t, e, 0]`` of an actor that shares the critic's
        hidden layers and whose output row 0 is the critic's.

        Returns fresh device tensors ``value``, ``advantage``, ``return`` ``[T, B]`` (and ``next_value`` with
        ``return_next_values=True``).  Touches nothing of the env, never synchronises, capturable into a ``torch.cuda.CUDAGraph``."""
        p = self._critic_args(critic, params, gamma, lam)
        return self._advantages(batch, critic, p, float(gamma), float(lam), bool(return_next_values))

    def _advantages(self, batch, critic, p, gamma, lam, return_next_values):
        torch = self._torch
        for key in ("obs", "reward", "terminated", "truncated", "next_obs"):
            if key not in batch:
                raise ValueError(f"batch lacks {key!r}")
        obs = batch["obs"]
        OD = self.sim.obs_dim
        if not isinstance(obs, torch.Tensor) or obs.dim() != 3 or obs.shape[0] < 1 or obs.shape[1] < 1 or obs.shape[2] != OD:
            raise ValueError(f"batch['obs'] must be a [T >= 1, B >= 1, {OD}] tensor, got {tuple(np.shape(obs))}")
        T, B = int(obs.shape[0]), int(obs.shape[1])
        fobs = batch.get("final_obs")
        want = {"obs": ((T, B, OD), (torch.float32,)), "reward": ((T, B), (torch.float32,)),
                "terminated": ((T, B), (torch.bool, torch.uint8)), "truncated": ((T, B), (torch.bool, torch.uint8)),
                "next_obs": ((B, OD), (torch.float32,))}
        if fobs is not None:
            want["final_obs"] = ((T, B, OD), (torch.float32,))
        for key, (shape, dtypes) in want.items():
            t = batch[key]
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"batch[{key!r}] must be a torch tensor, got {type(t).__name__}")
            if tuple(t.shape) != shape:
                raise ValueError(f"batch[{key!r}] must be {list(shape)}, got {list(t.shape)}")
            if t.dtype not in dtypes:
                raise ValueError(f"batch[{key!r}] must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
            if t.device != self.device:
                raise ValueError(f"batch[{key!r}] is on {t.device}, the env on {self.device}")
            if not t.is_contiguous():
                raise ValueError(f"batch[{key!r}] must be contiguous")
        f32 = dict(dtype=torch.float32, device=self.device)
        val, adv, ret = (torch.empty((T, B), **f32) for _ in range(3))
        nxt = torch.empty((T, B), **f32) if return_next_values else None
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731  (a bool tensor is one byte per element, 0 or 1)
        inp = _lib.AdvIn(ptr(obs), ptr(batch["reward"]), ptr(batch["terminated"]), ptr(batch["truncated"]), ptr(fobs), ptr(batch["next_obs"]))
        self.sim.task_advantages(critic.spec(), p.data_ptr(), gamma, lam, T, B, inp, _lib.AdvOut(ptr(val), ptr(adv), ptr(ret), ptr(nxt)),
                                 self._stream())
        self._keep_adv = p   # alive until the launches have consumed it
        out = {"value": val, "advantage": adv, "return": ret}
        if return_next_values:
            out["next_value"] = nxt
        return out

    def _ppo_args(self, batch, policy, params, log_std, critic, critic_params, advantage, clip, vf_coef, ent_coef, max_workgroups):
        """what ppo_gradient() and ppo_update() check alike of the two networks, the loss's scalars, the batch and the parameter
        tensors; returns the (detached) tensors, (T, B, N) and the scalars as the C structs take them"""
        torch = self._torch
        from rsoccer_amd.vec.policy import MLPCritic, MLPPolicy
        if not isinstance(policy, MLPPolicy) or isinstance(policy, MLPCritic):
            raise ValueError("policy must be an rsoccer_amd.vec.policy.MLPPolicy")
        if not isinstance(critic, MLPCritic):
            raise ValueError("critic must be an rsoccer_amd.vec.policy.MLPCritic")
        OD, AD, dev = self.sim.obs_dim, self.sim.act_dim, self.device
        if policy.obs_dim != OD or policy.act_dim != AD:
            raise ValueError(f"the policy maps {policy.obs_dim} -> {policy.act_dim}, the env {OD} -> {AD}")
        if critic.obs_dim != OD:
            raise ValueError(f"the critic reads {critic.obs_dim} floats, the env's observation has {OD}")
        clip, vf_coef, ent_coef = float(clip), float(vf_coef), float(ent_coef)
        if not (np.isfinite(clip) and 0.0 < clip < 1.0):
            raise ValueError(f"clip must be in (0, 1), got {clip}")
        for name, v in (("vf_coef", vf_coef), ("ent_coef", ent_coef)):
            if not np.isfinite(v):
                raise ValueError(f"{name} must be finite, got {v}")
        mw = 0 if max_workgroups is None else int(max_workgroups)
        if mw < 0 or (max_workgroups is not None and mw < 1):
            raise ValueError(f"max_workgroups must be >= 1 or None, got {max_workgroups}")

        def need(name, t, shape, dtypes=(torch.float32,)):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
            if t.dtype not in dtypes:
                raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
            if t.device != dev:
                raise ValueError(f"{name} is on {t.device}, the env on {dev}")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            return t.detach()

        keys = ("obs", "sample", "log_prob", "return") + (("advantage",) if advantage is None else ())
        for key in keys:
            if key not in batch:
                raise ValueError(f"batch lacks {key!r}")
        obs = batch["obs"]
        if not isinstance(obs, torch.Tensor) or obs.dim() != 3 or obs.shape[0] < 1 or obs.shape[1] < 1 or obs.shape[2] != OD:
            raise ValueError(f"batch['obs'] must be a [T >= 1, B >= 1, {OD}] tensor, got {tuple(np.shape(obs))}")
        T, B = int(obs.shape[0]), int(obs.shape[1])
        N = T * B
        obs = need("batch['obs']", obs, (T, B, OD))
        smp = need("batch['sample']", batch["sample"], (T, B, AD))
        olp = need("batch['log_prob']", batch["log_prob"], (T, B))
        ret = need("batch['return']", batch["return"], (T, B))
        adv = need("batch['advantage']", batch["advantage"], (T, B)) if advantage is None else need("advantage", advantage, (T, B))
        p = need("params", params, (policy.num_params,))
        ls = need("log_std", log_std, (AD,))
        cp = need("critic_params", critic_params, (critic.num_params,))
        return (obs, smp, olp, ret, adv, p, ls, cp), (T, B, N), (clip, vf_coef, ent_coef, mw)

    def ppo_gradient(self, batch, policy, params, log_std, critic, critic_params, rows=None, advantage=None, clip=0.2, vf_coef=0.5,
                     ent_coef=0.0, max_workgroups=None, return_forward=False):
        """Gradients of the PPO loss with respect to an MLP actor, its ``log_std`` and an MLP critic on a minibatch of a collected
        batch, in three launches (``rsx_task_ppo_gradient``): what a PPO loop does per minibatch before ``opt.step()``.

        ``batch``: ``collect(..., critic=...)``'s dict; ``obs`` ``[T, B, obs_dim]``, ``sample`` ``[T, B, act_dim]``, ``log_prob``,
        ``advantage`` and ``return`` ``[T, B]`` are used, all float32 CUDA tensors on the env's device, contiguous (anything else is a
        ``ValueError`` naming the offender).  ``advantage=`` overrides the batch's with a ``[T, B]`` tensor (a normalised one, say).
        ``policy`` / ``params`` ``[P]`` / ``log_std`` ``[act_dim]`` and ``critic`` / ``critic_params`` ``[Pc]``: as for ``collect``, float32
        device tensors.  ``rows``: the minibatch as a 1-D int32 / int64 tensor of flat indices into the ``T * B`` rows, repeats allowed
        (int64 is converted by one torch op); ``None``: the whole batch.  Host-side ``rows`` (list, numpy, CPU tensor) are range-checked;
        a device tensor is not — an index outside ``[0, T * B)`` contributes nothing and is counted in ``stats["rows_skipped"]``.

        The loss is ``L_pi + vf_coef * L_v - ent_coef * entropy`` with the clipped surrogate of ``clip`` and means over the minibatch,
        written out in ``include/rsx.h`` with its float32 arithmetic.  ``max_workgroups`` caps the grid of the row launches (``None``:
        the build's default); the result bits depend on the inputs and that number only.

        Returns fresh device tensors ``grad_params`` ``[P]``, ``grad_log_std`` ``[act_dim]``, ``grad_critic_params`` ``[Pc]`` and
        ``stats``: a dict of 0-d views (``loss_pi``, ``loss_v``, ``entropy``, ``approx_kl``, ``clip_fraction``, ``ratio``, ``rows_used``,
        ``rows_skipped``; no synchronisation); with ``return_forward=True`` also ``mean`` ``[M, act_dim]`` and ``value`` ``[M]``, bit for
        bit ``batch["mean"]`` / ``batch["value"]`` at the rows.  Touches nothing of the env, never synchronises, capturable."""
        torch = self._torch
        dev, AD = self.device, self.sim.act_dim
        (obs, smp, olp, ret, adv, p, ls, cp), (T, B, N), (clip, vf_coef, ent_coef, mw) = self._ppo_args(
            batch, policy, params, log_std, critic, critic_params, advantage, clip, vf_coef, ent_coef, max_workgroups)
        if rows is None:
            r, M = None, N
        else:
            if not isinstance(rows, torch.Tensor) or not rows.is_cuda:   # host data: checked, then uploaded
                host = np.asarray(rows.numpy() if isinstance(rows, torch.Tensor) else rows)
                if host.ndim != 1 or host.size < 1 or host.dtype.kind not in "iu":
                    raise ValueError(f"rows must be a 1-D integer array with at least one entry, got shape {host.shape} dtype {host.dtype}")
                if int(host.min()) < 0 or int(host.max()) >= N:
                    raise ValueError(f"rows must lie in [0, {N}), got {int(host.min())} .. {int(host.max())}")
                rows = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).to(dev)
            if rows.dim() != 1 or rows.shape[0] < 1:
                raise ValueError(f"rows must be 1-D with at least one entry, got {list(rows.shape)}")
            if rows.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"rows must be torch.int32 or torch.int64, got {rows.dtype}")
            if rows.device != dev:
                raise ValueError(f"rows is on {rows.device}, the env on {dev}")
            r = rows.to(torch.int32) if rows.dtype == torch.int64 else rows
            if not r.is_contiguous():
                raise ValueError("rows must be contiguous")
            M = int(r.shape[0])
        aspec, cspec = policy.spec(), critic.spec()
        nbytes = self.sim.ppo_gradient_workspace(aspec, cspec, M, mw)
        f32 = dict(dtype=torch.float32, device=dev)
        ws = torch.empty(((nbytes + 3) // 4,), **f32)
        ga, gl, gc = torch.empty((policy.num_params,), **f32), torch.empty((AD,), **f32), torch.empty((critic.num_params,), **f32)
        stats = torch.empty((8,), **f32)
        mean = torch.empty((M, AD), **f32) if return_forward else None
        val = torch.empty((M,), **f32) if return_forward else None
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        inp = _lib.PpoIn(ptr(obs), ptr(smp), ptr(olp), ptr(adv), ptr(ret), ptr(r), N, M)
        out = _lib.PpoOut(ptr(ga), ptr(gl), ptr(gc), ptr(stats), ptr(mean), ptr(val), ptr(ws))
        self.sim.task_ppo_gradient(aspec, ptr(p), ptr(ls), cspec, ptr(cp), inp, _lib.PpoCfg(clip, vf_coef, ent_coef, mw), out, self._stream())
        self._keep_ppo = (ws, r)   # the call's own tensors: alive until the launches have consumed them
        res = {"grad_params": ga, "grad_log_std": gl, "grad_critic_params": gc,
               "stats": {name: stats[k] for k, name in enumerate(_lib.PPO_STATS)}}
        if return_forward:
            res["mean"], res["value"] = mean, val
        return res

    # ---- off-policy updates (include/rsx.h: rsx_task_dpg_gradient) ----
    def dpg_gradient(self, data, policy, params, target_params, critic, critic_params, target_critic_params, rows=None, gamma=0.99,
                     target_noise=0.0, noise_clip=0.5, noise_seed=0, noise_step=0, actor=True, max_workgroups=None, return_rows=False,
                     weights=None, return_td_error=False):
        """Gradients of the TD3 / DDPG losses with respect to an MLP actor and its one or two Q critics on a minibatch of replayed
        transitions, in four launches (``rsx_task_dpg_gradient``): what an off-policy loop does per gradient step before
        ``opt.step()`` and the Polyak update.

        ``data``: a mapping of flat transition rows — ``ReplayBuffer.data()`` or any tensors ``obs`` ``[N, obs_dim]``, ``actions``
        ``[N, act_dim]``, ``reward`` ``[N]``, ``next_obs`` ``[N, obs_dim]`` (float32) and ``terminated`` ``[N]`` (bool / uint8) on the
        env's device, contiguous (anything else is a ``ValueError`` naming the offender).  ``policy`` / ``params`` ``[P]`` /
        ``target_params`` ``[P]``: an ``MLPPolicy`` and its live and target parameters.  ``critic``: an ``MLPQCritic``;
        ``critic_params`` and ``target_critic_params`` ``[C, Pc]`` with ``C`` in (1, 2).  ``rows``: as for ``ppo_gradient``.

        ``target_noise`` (sigma) and ``noise_clip``: TD3's target policy smoothing; 0 draws nothing (DDPG).  The draw of minibatch
        position ``t`` depends on ``(noise_seed, noise_step, t)`` only; ``noise_step`` may be an int64 device tensor ``[1]``, read when
        the launch runs, so a replayed graph draws fresh noise once the tensor was advanced.  ``actor=False`` skips the actor launch
        (TD3's delayed policy update); every other output keeps its bits.  The losses and their float32 arithmetic are written out in
        ``include/rsx.h``; the result bits depend on the inputs and ``max_workgroups`` only.

        Returns fresh device tensors ``grad_params`` ``[P]`` (absent with ``actor=False``), ``grad_critic_params`` ``[C, Pc]`` and
        ``stats``: a dict of 0-d views (``_lib.DPG_STATS``; ``loss_pi`` absent with ``actor=False``; no synchronisation); with
        ``return_rows=True`` also ``target`` ``[M]``, ``q`` ``[C, M]``, ``target_noise`` ``[M, act_dim]`` and, with the actor,
        ``action`` ``[M, act_dim]``.  Touches nothing of the env, never synchronises, capturable.

        Prioritised and n-step replay (``rsx_task_dpg_gradient_w``): a ``data`` mapping that carries ``"discount"`` ``[N]`` (float32;
        ``PrioritizedReplayBuffer.data()``) uses it per row in place of ``gamma`` in the target; ``gamma`` then only validates.
        ``weights`` ``[M]`` (float32, by position in the minibatch: ``PrioritizedReplayBuffer.sample``'s) scale the critic loss only —
        the actor's loss stays unweighted; a weight of exactly 1 leaves every bit alone.  ``return_td_error=True`` adds ``td_error``
        ``[M]``, ``max_c |Q_c - y|`` per entry (0 for a skipped one), in one more launch: what ``update_priorities`` takes.  Without
        these two arguments and without that key the call is the plain entry point's, as before."""
        torch = self._torch
        from rsoccer_amd.vec.policy import MLPCritic, MLPPolicy, MLPQCritic
        if not isinstance(policy, MLPPolicy) or isinstance(policy, (MLPCritic, MLPQCritic)):
            raise ValueError("policy must be an rsoccer_amd.vec.policy.MLPPolicy")
        if not isinstance(critic, MLPQCritic):
            raise ValueError("critic must be an rsoccer_amd.vec.policy.MLPQCritic")
        OD, AD, dev = self.sim.obs_dim, self.sim.act_dim, self.device
        if policy.obs_dim != OD or policy.act_dim != AD:
            raise ValueError(f"the policy maps {policy.obs_dim} -> {policy.act_dim}, the env {OD} -> {AD}")
        if critic.state_dim != OD or critic.action_dim != AD:
            raise ValueError(f"the critic reads ({critic.state_dim}, {critic.action_dim}) floats, the env has ({OD}, {AD})")
        gamma, sigma, noise_clip = float(gamma), float(target_noise), float(noise_clip)
        if not (np.isfinite(gamma) and 0.0 <= gamma <= 1.0):
            raise ValueError(f"gamma must be in [0, 1], got {gamma}")
        for name, v in (("target_noise", sigma), ("noise_clip", noise_clip)):
            if not (np.isfinite(v) and v >= 0.0):
                raise ValueError(f"{name} must be finite and >= 0, got {v}")
        mw = 0 if max_workgroups is None else int(max_workgroups)
        if mw < 0 or (max_workgroups is not None and mw < 1):
            raise ValueError(f"max_workgroups must be >= 1 or None, got {max_workgroups}")

        def need(name, t, shape, dtypes=(torch.float32,)):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
            if t.dtype not in dtypes:
                raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
            if t.device != dev:
                raise ValueError(f"{name} is on {t.device}, the env on {dev}")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            return t.detach()

        for key in ("obs", "actions", "reward", "next_obs", "terminated"):
            if key not in data:
                raise ValueError(f"data lacks {key!r}")
        obs = data["obs"]
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2 or obs.shape[0] < 1 or obs.shape[1] != OD:
            raise ValueError(f"data['obs'] must be a [N >= 1, {OD}] tensor, got {tuple(np.shape(obs))}")
        N = int(obs.shape[0])
        obs = need("data['obs']", obs, (N, OD))
        act = need("data['actions']", data["actions"], (N, AD))
        rew = need("data['reward']", data["reward"], (N,))
        nxt = need("data['next_obs']", data["next_obs"], (N, OD))
        term = need("data['terminated']", data["terminated"], (N,), (torch.bool, torch.uint8))
        p = need("params", params, (policy.num_params,))
        tp = need("target_params", target_params, (policy.num_params,))
        if not isinstance(critic_params, torch.Tensor) or critic_params.dim() != 2 or critic_params.shape[0] not in (1, 2):
            raise ValueError(f"critic_params must be a [C, {critic.num_params}] tensor with C in (1, 2), got {tuple(np.shape(critic_params))}")
        C = int(critic_params.shape[0])
        cp = need("critic_params", critic_params, (C, critic.num_params))
        tcp = need("target_critic_params", target_critic_params, (C, critic.num_params))
        step_ptr, step = None, 0
        if isinstance(noise_step, torch.Tensor):
            step_t = need("noise_step", noise_step, (1,), (torch.int64,))
            step_ptr = step_t.data_ptr()
        else:
            step_t, step = None, int(noise_step)
        if rows is None:
            r, M = None, N
        else:
            if not isinstance(rows, torch.Tensor) or not rows.is_cuda:   # host data: checked, then uploaded
                host = np.asarray(rows.numpy() if isinstance(rows, torch.Tensor) else rows)
                if host.ndim != 1 or host.size < 1 or host.dtype.kind not in "iu":
                    raise ValueError(f"rows must be a 1-D integer array with at least one entry, got shape {host.shape} dtype {host.dtype}")
                if int(host.min()) < 0 or int(host.max()) >= N:
                    raise ValueError(f"rows must lie in [0, {N}), got {int(host.min())} .. {int(host.max())}")
                rows = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).to(dev)
            if rows.dim() != 1 or rows.shape[0] < 1:
                raise ValueError(f"rows must be 1-D with at least one entry, got {list(rows.shape)}")
            if rows.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"rows must be torch.int32 or torch.int64, got {rows.dtype}")
            if rows.device != dev:
                raise ValueError(f"rows is on {rows.device}, the env on {dev}")
            r = rows.to(torch.int32) if rows.dtype == torch.int64 else rows
            if not r.is_contiguous():
                raise ValueError("rows must be contiguous")
            M = int(r.shape[0])
        disc = need("data['discount']", data["discount"], (N,)) if "discount" in data else None
        wts = need("weights", weights, (M,)) if weights is not None else None
        with_per = disc is not None or wts is not None or bool(return_td_error)
        aspec, cspec = policy.spec(), critic.spec()
        f32 = dict(dtype=torch.float32, device=dev)
        # the workspace, cached per (shape, C, M, max_workgroups): calls on one stream are ordered, so they may share it
        key = (policy.layers, policy.hidden, critic.layers, critic.hidden, C, M, mw)
        cache = self.__dict__.setdefault("_dpg_ws", {})
        ws = cache.get(key)
        if ws is None:
            ws = cache[key] = torch.empty(((self.sim.dpg_gradient_workspace(aspec, cspec, C, M, mw) + 3) // 4,), **f32)
        ga = torch.empty((policy.num_params,), **f32) if actor else None
        gc = torch.empty((C, critic.num_params), **f32)
        stats = torch.empty((len(_lib.DPG_STATS),), **f32)
        tgt = torch.empty((M,), **f32) if return_rows or return_td_error else None   # (the TD error is computed from these two)
        q = torch.empty((C, M), **f32) if return_rows or return_td_error else None
        td = torch.empty((M,), **f32) if return_td_error else None
        pi = torch.empty((M, AD), **f32) if return_rows and actor else None
        nz = torch.empty((M, AD), **f32) if return_rows else None
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731  (a bool tensor is one byte per element, 0 or 1)
        inp = _lib.DpgIn(ptr(obs), ptr(act), ptr(rew), ptr(nxt), ptr(term), ptr(r), N, M)
        cfg = _lib.DpgCfg(step_ptr, int(noise_seed) & 0xFFFFFFFFFFFFFFFF, step, gamma, sigma, noise_clip, C, mw)
        out = _lib.DpgOut(ptr(ga), ptr(gc), ptr(stats), ptr(tgt), ptr(q), ptr(pi), ptr(nz), ptr(ws))
        if with_per:
            self.sim.task_dpg_gradient_w(aspec, ptr(p), ptr(tp), cspec, ptr(cp), ptr(tcp), inp, cfg, out,
                                         _lib.GradPer(ptr(disc), ptr(wts), ptr(td)), self._stream())
        else:
            self.sim.task_dpg_gradient(aspec, ptr(p), ptr(tp), cspec, ptr(cp), ptr(tcp), inp, cfg, out, self._stream())
        self._keep_dpg = (r, step_t, term, disc, wts, tgt, q)   # the call's own tensors: alive until the launches have consumed them
        res = {"grad_critic_params": gc,
               "stats": {name: stats[k] for k, name in enumerate(_lib.DPG_STATS) if actor or name != "loss_pi"}}
        if actor:
            res["grad_params"] = ga
        if return_rows:
            res["target"], res["q"], res["target_noise"] = tgt, q, nz
            if actor:
                res["action"] = pi
        if return_td_error:
            res["td_error"] = td
        return res

    def sac_gradient(self, data, policy, params, critic, critic_params, target_critic_params, log_alpha, rows=None, gamma=0.99,
                     target_entropy=None, noise_seed=0, noise_step=0, max_workgroups=None, return_rows=False, weights=None,
                     return_td_error=False):
        """Gradients of the soft actor-critic losses with respect to an ``MLPGaussianPolicy`` actor, its one or two Q critics and the
        log-temperature on a minibatch of replayed transitions, in six launches (``rsx_task_sac_gradient``): what a SAC loop does per
        gradient step before its three optimiser steps and the Polyak update of the target critics.

        ``data``, ``rows``, ``critic`` / ``critic_params`` / ``target_critic_params`` ``[C, Pc]``, ``gamma``, ``noise_seed``,
        ``noise_step`` (an int or an int64 device tensor ``[1]``) and ``max_workgroups`` are ``dpg_gradient``'s.  ``policy`` / ``params``
        ``[P]``: the actor (there is no target actor; the log-std bounds are the policy's).  ``log_alpha``: ``[1]`` float32 on the
        device, ``alpha = exp(log_alpha)`` read when the launches run.  ``target_entropy=None`` means ``-act_dim``.  The draws of
        minibatch position ``t`` depend on ``(noise_seed, noise_step, t)`` only.  The losses and their float32 arithmetic are written out
        in ``include/rsx.h``; the result bits depend on the inputs and ``max_workgroups`` only.

        Returns fresh device tensors ``grad_params`` ``[P]``, ``grad_critic_params`` ``[C, Pc]``, ``grad_log_alpha`` ``[1]`` and
        ``stats``: a dict of 0-d views (``_lib.SAC_STATS``; no synchronisation); with ``return_rows=True`` also ``target`` ``[M]``, ``q``
        ``[C, M]``, ``action`` ``[M, act_dim]`` (the sample on ``obs``), ``log_prob`` ``[M]``, ``next_log_prob`` ``[M]``, ``eps``,
        ``next_eps``, ``mean`` and ``log_std`` ``[M, act_dim]`` — zero for a skipped entry.  Touches nothing of the env, never
        synchronises, capturable.

        Prioritised and n-step replay (``rsx_task_sac_gradient_w``): ``data["discount"]`` ``[N]``, ``weights`` ``[M]`` and
        ``return_td_error`` are ``dpg_gradient``'s: a per-row discount in place of ``gamma`` in the target (``gamma`` then only
        validates), a per-entry weight on the critic loss only (the actor's and the temperature's losses stay unweighted) and
        ``td_error`` ``[M]``.  Without them the call is the plain entry point's, as before."""
        torch = self._torch
        from rsoccer_amd.vec.policy import MLPGaussianPolicy, MLPQCritic
        if not isinstance(policy, MLPGaussianPolicy):
            raise ValueError("policy must be an rsoccer_amd.vec.policy.MLPGaussianPolicy")
        if not isinstance(critic, MLPQCritic):
            raise ValueError("critic must be an rsoccer_amd.vec.policy.MLPQCritic")
        OD, AD, dev = self.sim.obs_dim, self.sim.act_dim, self.device
        if policy.obs_dim != OD or policy.act_dim != AD:
            raise ValueError(f"the policy maps {policy.obs_dim} -> {policy.act_dim}, the env {OD} -> {AD}")
        if critic.state_dim != OD or critic.action_dim != AD:
            raise ValueError(f"the critic reads ({critic.state_dim}, {critic.action_dim}) floats, the env has ({OD}, {AD})")
        gamma = float(gamma)
        if not (np.isfinite(gamma) and 0.0 <= gamma <= 1.0):
            raise ValueError(f"gamma must be in [0, 1], got {gamma}")
        te = -float(AD) if target_entropy is None else float(target_entropy)
        if not np.isfinite(te):
            raise ValueError(f"target_entropy must be finite, got {target_entropy}")
        mw = 0 if max_workgroups is None else int(max_workgroups)
        if mw < 0 or (max_workgroups is not None and mw < 1):
            raise ValueError(f"max_workgroups must be >= 1 or None, got {max_workgroups}")

        def need(name, t, shape, dtypes=(torch.float32,)):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
            if t.dtype not in dtypes:
                raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
            if t.device != dev:
                raise ValueError(f"{name} is on {t.device}, the env on {dev}")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            return t.detach()

        for key in ("obs", "actions", "reward", "next_obs", "terminated"):
            if key not in data:
                raise ValueError(f"data lacks {key!r}")
        obs = data["obs"]
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2 or obs.shape[0] < 1 or obs.shape[1] != OD:
            raise ValueError(f"data['obs'] must be a [N >= 1, {OD}] tensor, got {tuple(np.shape(obs))}")
        N = int(obs.shape[0])
        obs = need("data['obs']", obs, (N, OD))
        act = need("data['actions']", data["actions"], (N, AD))
        rew = need("data['reward']", data["reward"], (N,))
        nxt = need("data['next_obs']", data["next_obs"], (N, OD))
        term = need("data['terminated']", data["terminated"], (N,), (torch.bool, torch.uint8))
        p = need("params", params, (policy.num_params,))
        if not isinstance(critic_params, torch.Tensor) or critic_params.dim() != 2 or critic_params.shape[0] not in (1, 2):
            raise ValueError(f"critic_params must be a [C, {critic.num_params}] tensor with C in (1, 2), got {tuple(np.shape(critic_params))}")
        C = int(critic_params.shape[0])
        cp = need("critic_params", critic_params, (C, critic.num_params))
        tcp = need("target_critic_params", target_critic_params, (C, critic.num_params))
        la = need("log_alpha", log_alpha, (1,))
        step_ptr, step = None, 0
        if isinstance(noise_step, torch.Tensor):
            step_t = need("noise_step", noise_step, (1,), (torch.int64,))
            step_ptr = step_t.data_ptr()
        else:
            step_t, step = None, int(noise_step)
        if rows is None:
            r, M = None, N
        else:
            if not isinstance(rows, torch.Tensor) or not rows.is_cuda:   # host data: checked, then uploaded
                host = np.asarray(rows.numpy() if isinstance(rows, torch.Tensor) else rows)
                if host.ndim != 1 or host.size < 1 or host.dtype.kind not in "iu":
                    raise ValueError(f"rows must be a 1-D integer array with at least one entry, got shape {host.shape} dtype {host.dtype}")
                if int(host.min()) < 0 or int(host.max()) >= N:
                    raise ValueError(f"rows must lie in [0, {N}), got {int(host.min())} .. {int(host.max())}")
                rows = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32)).to(dev)
            if rows.dim() != 1 or rows.shape[0] < 1:
                raise ValueError(f"rows must be 1-D with at least one entry, got {list(rows.shape)}")
            if rows.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"rows must be torch.int32 or torch.int64, got {rows.dtype}")
            if rows.device != dev:
                raise ValueError(f"rows is on {rows.device}, the env on {dev}")
            r = rows.to(torch.int32) if rows.dtype == torch.int64 else rows
            if not r.is_contiguous():
                raise ValueError("rows must be contiguous")
            M = int(r.shape[0])
        disc = need("data['discount']", data["discount"], (N,)) if "discount" in data else None
        wts = need("weights", weights, (M,)) if weights is not None else None
        with_per = disc is not None or wts is not None or bool(return_td_error)
        aspec, cspec = policy.spec(), critic.spec()
        f32 = dict(dtype=torch.float32, device=dev)
        # the workspace, cached per (shape, C, M, max_workgroups): calls on one stream are ordered, so they may share it
        key = (policy.layers, policy.hidden, critic.layers, critic.hidden, C, M, mw)
        cache = self.__dict__.setdefault("_sac_ws", {})
        ws = cache.get(key)
        if ws is None:
            ws = cache[key] = torch.empty(((self.sim.sac_gradient_workspace(aspec, cspec, C, M, mw) + 3) // 4,), **f32)
        ga = torch.empty((policy.num_params,), **f32)
        gc = torch.empty((C, critic.num_params), **f32)
        gl = torch.empty((1,), **f32)
        stats = torch.empty((len(_lib.SAC_STATS),), **f32)
        per = {}
        if return_rows:
            per = {"target": (M,), "q": (C, M), "action": (M, AD), "log_prob": (M,), "next_log_prob": (M,), "eps": (M, AD),
                   "next_eps": (M, AD), "mean": (M, AD), "log_std": (M, AD)}
            per = {k: torch.empty(shape, **f32) for k, shape in per.items()}
        td = torch.empty((M,), **f32) if return_td_error else None
        own = per if return_rows or not return_td_error else {"target": torch.empty((M,), **f32), "q": torch.empty((C, M), **f32)}
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731  (a bool tensor is one byte per element, 0 or 1)
        inp = _lib.DpgIn(ptr(obs), ptr(act), ptr(rew), ptr(nxt), ptr(term), ptr(r), N, M)
        cfg = _lib.SacCfg(step_ptr, int(noise_seed) & 0xFFFFFFFFFFFFFFFF, step, gamma, te, policy.log_std_min, policy.log_std_max, C, mw)
        out = _lib.SacOut(ptr(ga), ptr(gc), ptr(gl), ptr(stats),
                          *(ptr(own.get(k)) for k in ("target", "q", "action", "log_prob", "next_log_prob", "eps", "next_eps", "mean", "log_std")),
                          ptr(ws))
        if with_per:
            self.sim.task_sac_gradient_w(aspec, ptr(p), cspec, ptr(cp), ptr(tcp), ptr(la), inp, cfg, out,
                                         _lib.GradPer(ptr(disc), ptr(wts), ptr(td)), self._stream())
        else:
            self.sim.task_sac_gradient(aspec, ptr(p), cspec, ptr(cp), ptr(tcp), ptr(la), inp, cfg, out, self._stream())
        self._keep_sac = (r, step_t, term, disc, wts, own)   # the call's own tensors: alive until the launches have consumed them
        res = {"grad_params": ga, "grad_critic_params": gc, "grad_log_alpha": gl,
               "stats": {name: stats[k] for k, name in enumerate(_lib.SAC_STATS)}}
        res.update(per)
        if return_td_error:
            res["td_error"] = td
        return res

    def dpg_update(self, buf, policy, params, target_params, critic, critic_params, target_critic_params, opt, grad_steps=8,
                   batch_size=256, policy_delay=2, gamma=0.99, target_noise=0.2, noise_clip=0.5, seed=0, max_workgroups=None):
        """The whole update phase of TD3 / DDPG enqueued by ONE call (``rsx_task_dpg_update``): per gradient step
        ``buf.sample_rows_device(batch_size, seed, opt.steps)``, ``dpg_gradient(rows=those, noise_seed=seed, noise_step=opt.steps,
        actor=<actor step>)`` and ``opt.step`` — bit for bit that sequence of calls, without the interpreter between them.  Step
        ``j`` of the call is an actor step (the actor is stepped and both targets move) when ``(j + 1) % policy_delay == 0``;
        ``grad_steps`` must be a multiple of ``policy_delay``.  ``policy_delay=1``, one critic and ``target_noise=0`` is DDPG.

        ``buf``: a ``ReplayBuffer``, or a ``data()`` mapping with a ``fill`` entry (int64 ``[1]`` on the env's device: the rows that
        hold a transition, read when the launches run).  ``policy`` / ``critic`` and the four parameter tensors: as for
        ``dpg_gradient``; the four are UPDATED IN PLACE, the transitions are not written.  ``opt``: a
        ``rsoccer_amd.vec.optim.DPGOptimizer`` of these networks on the env's device; its count of finished gradient steps (on the
        device) keys the row draws and the smoothing noise and advances by ``grad_steps``.  On an empty buffer every row is skipped,
        every gradient is 0 and no parameter moves; the counters advance.

        Returns ``{"stats": [grad_steps, 12], "rows": [batch_size] int32}``: per step ``dpg_gradient``'s nine values, the two gradient
        norms before the clip and whether the targets moved (``_lib.DPG_UPDATE_STATS``); ``rows`` is a view of the call's workspace
        holding the last step's rows.  Touches nothing of the env, never synchronises, capturable into a ``torch.cuda.CUDAGraph``:
        with ``collect()`` on a device-keyed env and ``buf.add`` in the same graph, one replay is one off-policy iteration."""
        torch = self._torch
        from rsoccer_amd.vec.optim import DPGOptimizer
        from rsoccer_amd.vec.policy import MLPCritic, MLPPolicy, MLPQCritic
        from rsoccer_amd.vec.replay import ReplayBuffer
        if not isinstance(opt, DPGOptimizer):
            raise ValueError("opt must be an rsoccer_amd.vec.optim.DPGOptimizer")
        if not isinstance(policy, MLPPolicy) or isinstance(policy, (MLPCritic, MLPQCritic)):
            raise ValueError("policy must be an rsoccer_amd.vec.policy.MLPPolicy")
        if not isinstance(critic, MLPQCritic):
            raise ValueError("critic must be an rsoccer_amd.vec.policy.MLPQCritic")
        OD, AD, dev = self.sim.obs_dim, self.sim.act_dim, self.device
        if policy.obs_dim != OD or policy.act_dim != AD:
            raise ValueError(f"the policy maps {policy.obs_dim} -> {policy.act_dim}, the env {OD} -> {AD}")
        if critic.state_dim != OD or critic.action_dim != AD:
            raise ValueError(f"the critic reads ({critic.state_dim}, {critic.action_dim}) floats, the env has ({OD}, {AD})")
        grad_steps, policy_delay, M = int(grad_steps), int(policy_delay), int(batch_size)
        if grad_steps < 1:
            raise ValueError(f"grad_steps must be >= 1, got {grad_steps}")
        if policy_delay < 1:
            raise ValueError(f"policy_delay must be >= 1, got {policy_delay}")
        if grad_steps % policy_delay != 0:
            raise ValueError(f"grad_steps must be a multiple of policy_delay, got {grad_steps} and {policy_delay}")
        if not 1 <= M <= 2 ** 31 - 1:
            raise ValueError(f"batch_size must be in 1 .. 2^31 - 1, got {batch_size}")
        gamma, sigma, noise_clip = float(gamma), float(target_noise), float(noise_clip)
        if not (np.isfinite(gamma) and 0.0 <= gamma <= 1.0):
            raise ValueError(f"gamma must be in [0, 1], got {gamma}")
        for name, v in (("target_noise", sigma), ("noise_clip", noise_clip)):
            if not (np.isfinite(v) and v >= 0.0):
                raise ValueError(f"{name} must be finite and >= 0, got {v}")
        if not 0.0 <= opt.tau <= 1.0:
            raise ValueError(f"tau must be in [0, 1], got {opt.tau}")
        mw = 0 if max_workgroups is None else int(max_workgroups)
        if mw < 0 or (max_workgroups is not None and mw < 1):
            raise ValueError(f"max_workgroups must be >= 1 or None, got {max_workgroups}")

        def need(name, t, shape, dtypes=(torch.float32,)):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
            if t.dtype not in dtypes:
                raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
            if t.device != dev:
                raise ValueError(f"{name} is on {t.device}, the env on {dev}")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            return t.detach()

        if isinstance(buf, ReplayBuffer):
            data = dict(buf.data(), fill=buf.fill)
        else:
            data = buf
            for key in ("obs", "actions", "reward", "next_obs", "terminated", "fill"):
                if key not in data:
                    raise ValueError(f"buf lacks {key!r}")
        obs = data["obs"]
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2 or obs.shape[0] < 1 or obs.shape[1] != OD:
            raise ValueError(f"buf['obs'] must be a [N >= 1, {OD}] tensor, got {tuple(np.shape(obs))}")
        N = int(obs.shape[0])
        obs = need("buf['obs']", obs, (N, OD))
        act = need("buf['actions']", data["actions"], (N, AD))
        rew = need("buf['reward']", data["reward"], (N,))
        nxt = need("buf['next_obs']", data["next_obs"], (N, OD))
        term = need("buf['terminated']", data["terminated"], (N,), (torch.bool, torch.uint8))
        fill = need("buf['fill']", data["fill"], (1,), (torch.int64,))
        p = need("params", params, (policy.num_params,))
        tp = need("target_params", target_params, (policy.num_params,))
        if not isinstance(critic_params, torch.Tensor) or critic_params.dim() != 2 or critic_params.shape[0] not in (1, 2):
            raise ValueError(f"critic_params must be a [C, {critic.num_params}] tensor with C in (1, 2), got {tuple(np.shape(critic_params))}")
        C = int(critic_params.shape[0])
        cp = need("critic_params", critic_params, (C, critic.num_params))
        tcp = need("target_critic_params", target_critic_params, (C, critic.num_params))
        if opt.device != dev:
            raise ValueError(f"the optimiser is on {opt.device}, the env on {dev}")
        if opt.sizes != (policy.num_params, C * critic.num_params):
            raise ValueError(f"the optimiser's state tensors have sizes {opt.sizes}, the networks "
                             f"{(policy.num_params, C * critic.num_params)}")
        aspec, cspec = policy.spec(), critic.spec()
        nbytes, rows_off = self.sim.dpg_update_workspace(aspec, cspec, C, M, mw)
        ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=dev)
        stats = torch.empty((grad_steps, len(_lib.DPG_UPDATE_STATS)), dtype=torch.float32, device=dev)
        ptr = lambda t: t.data_ptr()   # noqa: E731  (a bool tensor is one byte per element, 0 or 1)
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        inp = _lib.DpgIn(ptr(obs), ptr(act), ptr(rew), ptr(nxt), ptr(term), None, N, M)
        cfg = _lib.DpgCfg(None, seed, 0, gamma, sigma, noise_clip, C, mw)
        ucfg = _lib.DpgUpdateCfg(ptr(fill), seed, 0, grad_steps, policy_delay)
        self.sim.task_dpg_update(aspec, ptr(p), ptr(tp), cspec, ptr(cp), ptr(tcp), inp, cfg, ucfg, opt.cfg(), opt.state(), ptr(stats),
                                 ptr(ws), self._stream())
        self._keep_dpg_update = (ws, term, fill)   # the call's own tensors: alive until the launches have consumed them
        return {"stats": stats, "rows": ws[rows_off // 4: rows_off // 4 + M].view(torch.int32)}

    def sac_update(self, buf, policy, params, critic, critic_params, target_critic_params, log_alpha, opt, grad_steps=8, batch_size=256,
                   gamma=0.99, target_entropy=None, learn_alpha=True, seed=0, max_workgroups=None):
        """The whole update phase of soft actor-critic enqueued by ONE call (``rsx_task_sac_update``): per gradient step
        ``buf.sample_rows_device(batch_size, seed, opt.steps)``, ``sac_gradient(rows=those, noise_seed=seed, noise_step=opt.steps)``
        and ``opt.step(..., update_targets=True)`` — bit for bit that sequence of calls, without the interpreter between them.  Every
        step steps the critics and the actor and moves the target critics; ``learn_alpha=False`` keeps the temperature fixed
        (``log_alpha``, its moments and its step count keep their bytes).

        ``buf``: a ``ReplayBuffer``, or a ``data()`` mapping with a ``fill`` entry (int64 ``[1]`` on the env's device: the rows that
        hold a transition, read when the launches run).  ``policy`` / ``critic``, the three parameter tensors, ``log_alpha`` ``[1]``,
        ``gamma`` and ``target_entropy``: as for ``sac_gradient``; the four tensors are UPDATED IN PLACE, the transitions are not
        written.  ``opt``: a ``rsoccer_amd.vec.optim.SACOptimizer`` of these networks on the env's device; its count of finished
        gradient steps (on the device) keys the row draws and the sampling noise and advances by ``grad_steps``.  On an empty buffer
        every row is skipped, no parameter moves (``log_alpha`` neither), the counters advance and the targets take their steps.

        Returns ``{"stats": {name: [grad_steps]}, "table": [grad_steps, 16], "rows": [batch_size] int32}``: per step ``sac_gradient``'s
        twelve values, the two gradient norms before the clip, ``log_alpha`` after the step and whether the targets moved
        (``_lib.SAC_UPDATE_STATS``; ``stats`` holds the columns of ``table`` by name); ``rows`` is a view of the call's workspace holding
        the last step's rows.  Touches nothing of the env, never synchronises, capturable into a ``torch.cuda.CUDAGraph``: with
        ``collect()`` on a device-keyed env and ``buf.add`` in the same graph, one replay is one off-policy iteration."""
        torch = self._torch
        from rsoccer_amd.vec.optim import SACOptimizer
        from rsoccer_amd.vec.policy import MLPGaussianPolicy, MLPQCritic
        from rsoccer_amd.vec.replay import ReplayBuffer
        if not isinstance(opt, SACOptimizer):
            raise ValueError("opt must be an rsoccer_amd.vec.optim.SACOptimizer")
        if not isinstance(policy, MLPGaussianPolicy):
            raise ValueError("policy must be an rsoccer_amd.vec.policy.MLPGaussianPolicy")
        if not isinstance(critic, MLPQCritic):
            raise ValueError("critic must be an rsoccer_amd.vec.policy.MLPQCritic")
        OD, AD, dev = self.sim.obs_dim, self.sim.act_dim, self.device
        if policy.obs_dim != OD or policy.act_dim != AD:
            raise ValueError(f"the policy maps {policy.obs_dim} -> {policy.act_dim}, the env {OD} -> {AD}")
        if critic.state_dim != OD or critic.action_dim != AD:
            raise ValueError(f"the critic reads ({critic.state_dim}, {critic.action_dim}) floats, the env has ({OD}, {AD})")
        grad_steps, M = int(grad_steps), int(batch_size)
        if grad_steps < 1:
            raise ValueError(f"grad_steps must be >= 1, got {grad_steps}")
        if not 1 <= M <= 2 ** 31 - 1:
            raise ValueError(f"batch_size must be in 1 .. 2^31 - 1, got {batch_size}")
        gamma = float(gamma)
        if not (np.isfinite(gamma) and 0.0 <= gamma <= 1.0):
            raise ValueError(f"gamma must be in [0, 1], got {gamma}")
        te = -float(AD) if target_entropy is None else float(target_entropy)
        if not np.isfinite(te):
            raise ValueError(f"target_entropy must be finite, got {target_entropy}")
        if not 0.0 <= opt.tau <= 1.0:
            raise ValueError(f"tau must be in [0, 1], got {opt.tau}")
        mw = 0 if max_workgroups is None else int(max_workgroups)
        if mw < 0 or (max_workgroups is not None and mw < 1):
            raise ValueError(f"max_workgroups must be >= 1 or None, got {max_workgroups}")

        def need(name, t, shape, dtypes=(torch.float32,)):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
            if t.dtype not in dtypes:
                raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
            if t.device != dev:
                raise ValueError(f"{name} is on {t.device}, the env on {dev}")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
            return t.detach()

        if isinstance(buf, ReplayBuffer):
            data = dict(buf.data(), fill=buf.fill)
        else:
            data = buf
            for key in ("obs", "actions", "reward", "next_obs", "terminated", "fill"):
                if key not in data:
                    raise ValueError(f"buf lacks {key!r}")
        obs = data["obs"]
        if not isinstance(obs, torch.Tensor) or obs.dim() != 2 or obs.shape[0] < 1 or obs.shape[1] != OD:
            raise ValueError(f"buf['obs'] must be a [N >= 1, {OD}] tensor, got {tuple(np.shape(obs))}")
        N = int(obs.shape[0])
        obs = need("buf['obs']", obs, (N, OD))
        act = need("buf['actions']", data["actions"], (N, AD))
        rew = need("buf['reward']", data["reward"], (N,))
        nxt = need("buf['next_obs']", data["next_obs"], (N, OD))
        term = need("buf['terminated']", data["terminated"], (N,), (torch.bool, torch.uint8))
        fill = need("buf['fill']", data["fill"], (1,), (torch.int64,))
        p = need("params", params, (policy.num_params,))
        if not isinstance(critic_params, torch.Tensor) or critic_params.dim() != 2 or critic_params.shape[0] not in (1, 2):
            raise ValueError(f"critic_params must be a [C, {critic.num_params}] tensor with C in (1, 2), got {tuple(np.shape(critic_params))}")
        C = int(critic_params.shape[0])
        cp = need("critic_params", critic_params, (C, critic.num_params))
        tcp = need("target_critic_params", target_critic_params, (C, critic.num_params))
        la = need("log_alpha", log_alpha, (1,))
        if opt.device != dev:
            raise ValueError(f"the optimiser is on {opt.device}, the env on {dev}")
        if opt.sizes != (policy.num_params, C * critic.num_params):
            raise ValueError(f"the optimiser's state tensors have sizes {opt.sizes}, the networks "
                             f"{(policy.num_params, C * critic.num_params)}")
        aspec, cspec = policy.spec(), critic.spec()
        nbytes, rows_off = self.sim.sac_update_workspace(aspec, cspec, C, M, mw)
        ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=dev)
        stats = torch.empty((grad_steps, len(_lib.SAC_UPDATE_STATS)), dtype=torch.float32, device=dev)
        ptr = lambda t: t.data_ptr()   # noqa: E731  (a bool tensor is one byte per element, 0 or 1)
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        inp = _lib.DpgIn(ptr(obs), ptr(act), ptr(rew), ptr(nxt), ptr(term), None, N, M)
        cfg = _lib.SacCfg(None, seed, 0, gamma, te, policy.log_std_min, policy.log_std_max, C, mw)
        ucfg = _lib.SacUpdateCfg(ptr(fill), seed, 0, grad_steps, 1 if learn_alpha else 0)
        self.sim.task_sac_update(aspec, ptr(p), cspec, ptr(cp), ptr(tcp), ptr(la), inp, cfg, ucfg, opt.cfg(), opt.state(), ptr(stats),
                                 ptr(ws), self._stream())
        self._keep_sac_update = (ws, term, fill)   # the call's own tensors: alive until the launches have consumed them
        return {"stats": {name: stats[:, k] for k, name in enumerate(_lib.SAC_UPDATE_STATS)}, "table": stats,
                "rows": ws[rows_off // 4: rows_off // 4 + M].view(torch.int32)}

    # ---- the update phase around ppo_gradient (include/rsx.h: rsx_ppo_normalize, rsx_ppo_permutation, rsx_task_ppo_update) ----
    def normalize_advantages(self, adv, eps=1e-8, return_moments=False):
        """``(adv - adv.mean()) / (adv.std() + eps)`` over all entries of a float32 device tensor (any shape, at least two entries,
        contiguous), in two launches with a fixed reduction order (``rsx_ppo_normalize``; ``std`` carries Bessel's correction like
        ``torch.Tensor.std``; the sums are taken in float64, mean and std rounded to float32 once).  Returns a fresh tensor of
        ``adv``'s shape, with ``return_moments=True`` also a ``[2]`` tensor ``(mean, std)``.  Never synchronises, capturable."""
        torch = self._torch
        eps = float(eps)
        if not (np.isfinite(eps) and eps >= 0.0):
            raise ValueError(f"eps must be finite and >= 0, got {eps}")
        if not isinstance(adv, torch.Tensor):
            raise ValueError(f"adv must be a torch tensor, got {type(adv).__name__}")
        if adv.dtype != torch.float32:
            raise ValueError(f"adv must be torch.float32, got {adv.dtype}")
        if adv.numel() < 2:
            raise ValueError(f"adv must have at least 2 entries (one has no standard deviation), got {adv.numel()}")
        if adv.device != self.device:
            raise ValueError(f"adv is on {adv.device}, the env on {self.device}")
        if not adv.is_contiguous():
            raise ValueError("adv must be contiguous")
        adv = adv.detach()
        out = torch.empty_like(adv)
        ms = torch.empty((2,), dtype=torch.float32, device=self.device)
        ws = torch.empty((_lib.PPO_NORMALIZE_WORKSPACE_BYTES // 8,), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.ppo_normalize(adv.data_ptr(), adv.numel(), eps, out.data_ptr(), ms.data_ptr(), ws.data_ptr(), self._stream())
        self._keep_norm = ws   # alive until the launches have consumed it
        return (out, ms) if return_moments else out

    @staticmethod
    def minibatch_chunks(n, minibatches):
        """the ``(lo, hi)`` bounds of the ``minibatches`` chunks of ``n`` rows: ``c = ceil(n / minibatches)`` rows each, the last one
        what is left — ``torch.chunk``'s sizes.  A ``minibatches`` for which the last chunk would be empty is a ``ValueError``."""
        n, mb = int(n), int(minibatches)
        if n < 1:
            raise ValueError(f"n must be >= 1, got {n}")
        if mb < 1:
            raise ValueError(f"minibatches must be >= 1, got {minibatches}")
        c = -(-n // mb)
        if (mb - 1) * c >= n:
            raise ValueError(f"minibatches = {mb} leaves the last chunk of ceil({n} / {mb}) = {c} rows empty")
        return [(k * c, min((k + 1) * c, n)) for k in range(mb)]

    def minibatch_rows(self, n, seed, update, epoch, minibatches=None):
        """A fresh permutation of ``0 .. n - 1`` as an int32 device tensor, every entry computed independently from ``(seed, update,
        epoch, i)`` — no sort, no generator state (``rsx_ppo_permutation``: a keyed Feistel network with cycle walking, integer
        arithmetic written out in ``include/rsx.h``).  ``update``: an integer, or a ``PPOOptimizer`` — then the key is the update count
        in its device counters, read when the launch runs, so a replayed graph draws a new permutation on every replay.  With
        ``minibatches`` the list of that many chunk views (``minibatch_chunks``) is returned instead.  Never synchronises."""
        torch = self._torch
        from rsoccer_amd.vec.optim import PPOOptimizer
        n, epoch = int(n), int(epoch)
        if not 1 <= n <= 2 ** 31 - 1:
            raise ValueError(f"n must be in 1 .. 2^31 - 1, got {n}")
        if not 0 <= epoch < 2 ** 32:
            raise ValueError(f"epoch must be in 0 .. 2^32 - 1, got {epoch}")
        chunks = None if minibatches is None else self.minibatch_chunks(n, minibatches)
        upd_ptr, upd = None, 0
        if isinstance(update, PPOOptimizer):
            if update.device != self.device:
                raise ValueError(f"the optimiser is on {update.device}, the env on {self.device}")
            upd_ptr = update.counters.data_ptr() + 8 * _lib.ADAM_COUNTERS.index("updates")
        else:
            upd = int(update)
            if upd < 0:
                raise ValueError(f"update must be >= 0, got {update}")
        rows = torch.empty((n,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.ppo_permutation(rows.data_ptr(), n, int(seed), upd, upd_ptr, epoch, self._stream())
        return rows if chunks is None else [rows[lo:hi] for lo, hi in chunks]

    def ppo_update(self, batch, policy, params, log_std, critic, critic_params, opt, epochs=4, minibatches=4, clip=0.2, vf_coef=0.5,
                   ent_coef=0.0, normalize_advantage=True, target_kl=None, seed=0, max_workgroups=None):
        """The whole update phase of PPO enqueued by ONE call (``rsx_task_ppo_update``): ``normalize_advantages`` once per batch, per
        epoch one ``minibatch_rows(T * B, seed, opt, epoch)``, and per minibatch ``ppo_gradient(rows=chunk, advantage=normalised)``
        followed by ``opt.step`` — bit for bit that sequence of calls, without the interpreter between them.

        ``batch``, ``policy`` / ``params`` / ``log_std``, ``critic`` / ``critic_params``, ``clip``, ``vf_coef``, ``ent_coef``,
        ``max_workgroups``: as for ``ppo_gradient``.  ``params``, ``log_std`` and ``critic_params`` are UPDATED IN PLACE; ``batch`` is
        not written.  ``opt``: a ``rsoccer_amd.vec.optim.PPOOptimizer`` of these two networks on the env's device; its update count
        (on the device) keys the permutations and advances by one.  ``minibatches``: chunks of ``ceil(T * B / minibatches)`` rows,
        ``torch.chunk``'s sizes; a count for which the last chunk would be empty is refused.

        ``target_kl``: ``None`` or > 0.  The stopped flag is cleared when the call starts; a minibatch whose ``approx_kl`` exceeds
        ``target_kl`` sets it before its own step, and from then on no step of this call changes a parameter, a moment or ``t``.
        The remaining launches STILL RUN and their work is wasted: that is the price of not asking the host, which is what keeps the
        call free of synchronisation and capturable.

        Returns ``{"stats": [epochs, minibatches, 10], "rows": [T * B] int32}``: per minibatch ``ppo_gradient``'s eight values, the
        gradient norm before the clip and whether the step was applied (``_lib.PPO_UPDATE_STATS``); ``rows`` is a view of the call's
        workspace holding the last epoch's permutation.  Touches nothing of the env, never synchronises, capturable into a
        ``torch.cuda.CUDAGraph``: with ``collect()`` on a device-keyed env in the same graph, one replay is one PPO iteration."""
        torch = self._torch
        from rsoccer_amd.vec.optim import PPOOptimizer, check_target_kl
        if not isinstance(opt, PPOOptimizer):
            raise ValueError("opt must be an rsoccer_amd.vec.optim.PPOOptimizer")
        epochs = int(epochs)
        if epochs < 1:
            raise ValueError(f"epochs must be >= 1, got {epochs}")
        if int(minibatches) < 1:
            raise ValueError(f"minibatches must be >= 1, got {minibatches}")
        kl = check_target_kl(target_kl)
        (obs, smp, olp, ret, adv, p, ls, cp), (T, B, N), (clip, vf_coef, ent_coef, mw) = self._ppo_args(
            batch, policy, params, log_std, critic, critic_params, None, clip, vf_coef, ent_coef, max_workgroups)
        mb = len(self.minibatch_chunks(N, minibatches))
        if normalize_advantage and N < 2:
            raise ValueError("normalize_advantage needs at least 2 rows")
        if opt.device != self.device:
            raise ValueError(f"the optimiser is on {opt.device}, the env on {self.device}")
        if opt.sizes != (policy.num_params, self.sim.act_dim, critic.num_params):
            raise ValueError(f"the optimiser's state tensors have sizes {opt.sizes}, the networks "
                             f"{(policy.num_params, self.sim.act_dim, critic.num_params)}")
        aspec, cspec = policy.spec(), critic.spec()
        nbytes, rows_off = self.sim.ppo_update_workspace(aspec, cspec, N, mb, mw)
        ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=self.device)
        stats = torch.empty((epochs, mb, len(_lib.PPO_UPDATE_STATS)), dtype=torch.float32, device=self.device)
        ptr = lambda t: t.data_ptr()   # noqa: E731
        inp = _lib.PpoIn(ptr(obs), ptr(smp), ptr(olp), ptr(adv), ptr(ret), None, N, N)
        ucfg = _lib.PpoUpdateCfg(int(seed) & ((1 << 64) - 1), epochs, mb, 1 if normalize_advantage else 0, 1e-8)
        self.sim.task_ppo_update(aspec, ptr(p), ptr(ls), cspec, ptr(cp), inp, _lib.PpoCfg(clip, vf_coef, ent_coef, mw), ucfg,
                                 opt.cfg(None, kl if kl > 0.0 else None), opt.state(), ptr(stats), ptr(ws), self._stream())
        self._keep_update = ws   # the call's own tensor: alive until the launches have consumed it
        return {"stats": stats, "rows": ws[rows_off // 4: rows_off // 4 + N].view(torch.int32)}

    # ---- planning with candidates drawn on the device (include/rsx.h: rsx_plan_sampler) ----
    def _plan_sampler(self, sigma, hold, seed, iteration):
        """the rsx_plan_sampler of a call: ``sample_seed`` is a 64-bit mix (splitmix64) of ``seed`` (default: the env's) and
        ``iteration``, so refinement passes at one step use different noise and two envs built alike use the same"""
        sigma, hold = float(sigma), int(hold)
        if not np.isfinite(sigma) or sigma < 0:
            raise ValueError("sigma must be finite and >= 0")
        if hold < 1:
            raise ValueError("hold must be >= 1")
        m = (1 << 64) - 1
        z = ((self._seed if seed is None else int(seed)) + 0x9E3779B97F4A7C15 * (int(iteration) + 1)) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return _lib.PlanSampler(z ^ (z >> 31), sigma, hold)

    def _plan_mean(self, mean, horizon):
        """(device tensor or None, H) of a ``mean=`` / ``horizon=`` argument pair, shapes checked on the INPUT as lookahead() does"""
        torch = self._torch
        if mean is None:
            if horizon is None or int(horizon) < 1:
                raise ValueError("without a mean, horizon= must be given and >= 1")
            return None, int(horizon)
        shape = tuple(np.shape(mean))
        if len(shape) != 3 or shape[0] != self.num_envs or shape[2] != self.sim.act_dim or shape[1] < 1:
            raise ValueError(f"mean must be [{self.num_envs}, H >= 1, {self.sim.act_dim}], got {shape}")
        if horizon is not None and int(horizon) != shape[1]:
            raise ValueError(f"horizon={horizon} does not match mean's {shape[1]} steps")
        if isinstance(mean, torch.Tensor):
            m = mean
            if m.device != self.device or m.dtype != torch.float32 or not m.is_contiguous():
                m = m.to(device=self.device, dtype=torch.float32).contiguous()
        else:
            m = torch.from_numpy(np.ascontiguousarray(mean, dtype=np.float32)).to(self.device)
        return m, int(shape[1])

    def plan(self, mean=None, horizon=None, K=64, sigma=0.5, hold=1, temperature=0.0, gamma=1.0, seed=None, iteration=0,
             return_obs=False):
        """One iteration of random shooting / MPPI from where every env stands now, in two launches and without a candidate tensor
        (``rsx_task_lookahead_sampled``, ``rsx_plan_update``).

        ``K`` candidate sequences per env are drawn ON THE DEVICE around the plan ``mean`` ``[num_envs, H, act_dim]`` (``None``: zeros,
        with ``horizon=H``): candidate 0 is ``clamp(mean)``, candidate ``k >= 1`` is ``clamp(mean + sigma * noise)`` with one normal draw
        held for ``hold`` steps.  The noise is keyed by (``seed`` — default: the env's —, ``iteration``, global env id, candidate, the
        env's step counter): two calls between the same two steps see the same candidates unless ``iteration`` differs (refinement
        passes), after a ``step()`` they are fresh, and a captured call draws new noise on every replay.  The candidates are scored
        exactly as ``lookahead()`` scores them, then folded into the new plan: ``temperature == 0`` takes the best candidate,
        ``temperature > 0`` the mean weighted by ``exp((return - best return) / temperature)``.

        Returns a dict of fresh device tensors: ``action`` ``[num_envs, act_dim]`` (step 0 of the new plan: what to execute), ``mean``
        ``[num_envs, H, act_dim]`` (the new plan; shift it by one step for a warm start), ``return`` / ``steps`` / ``terminated`` /
        ``truncated`` ``[num_envs, K]`` as ``lookahead()``, ``best`` ``[num_envs]`` int32 (first index of the largest return), and with
        ``return_obs=True`` ``last_obs``.  The env is left exactly as it was.  Capturable after ``enable_graph_capture()``."""
        torch = self._torch
        m, H = self._plan_mean(mean, horizon)
        K, gamma, temperature = int(K), float(gamma), float(temperature)
        if K < 1:
            raise ValueError("K must be >= 1")
        if not np.isfinite(gamma):
            raise ValueError("gamma must be finite")
        if not np.isfinite(temperature) or temperature < 0:
            raise ValueError("temperature must be finite and >= 0")
        smp = self._plan_sampler(sigma, hold, seed, iteration)
        B, dev = self.num_envs, self.device
        ret = torch.empty((B, K), dtype=torch.float32, device=dev)
        steps = torch.empty((B, K), dtype=torch.int32, device=dev)
        flags = torch.empty((B, K), dtype=torch.uint8, device=dev)
        obs = torch.empty((B, K, self.sim.obs_dim), dtype=torch.float32, device=dev) if return_obs else None
        new = torch.empty((B, H, self.sim.act_dim), dtype=torch.float32, device=dev)
        best = torch.empty((B,), dtype=torch.int32, device=dev)
        mp = None if m is None else m.data_ptr()
        st = self._stream()
        self.sim.task_lookahead_sampled(mp, smp, K, H, gamma, ret.data_ptr(), steps.data_ptr(), flags.data_ptr(),
                                        obs.data_ptr() if return_obs else None, st)
        self.sim.plan_update(mp, smp, K, H, ret.data_ptr(), temperature, new.data_ptr(), best.data_ptr(), st)
        self._keep_plan = m   # alive until the launches have consumed it
        out = {"action": new[:, 0], "mean": new, "return": ret, "steps": steps, "terminated": (flags & 1).bool(),
               "truncated": (flags & 2).bool(), "best": best}
        if return_obs:
            out["last_obs"] = obs
        return out

    def plan_candidates(self, mean=None, horizon=None, K=64, sigma=0.5, hold=1, seed=None, iteration=0):
        """The candidates ``plan()`` with the same arguments scores at this step, written out: ``[num_envs, K, H, act_dim]`` float32
        (``rsx_plan_candidates``; for tests, debugging and callers who want a sequence's neighbours)."""
        torch = self._torch
        m, H = self._plan_mean(mean, horizon)
        K = int(K)
        if K < 1:
            raise ValueError("K must be >= 1")
        smp = self._plan_sampler(sigma, hold, seed, iteration)
        out = torch.empty((self.num_envs, K, H, self.sim.act_dim), dtype=torch.float32, device=self.device)
        self.sim.plan_candidates(None if m is None else m.data_ptr(), smp, K, H, out.data_ptr(), self._stream())
        self._keep_plan = m
        return out

    # ---- per-env physics / domain randomisation (include/rsx.h: rsx_physics_*; docs/PHYSICS.md section 3) ----
    def _physics_names(self):
        names = _lib.PHYSICS_PARAMS
        return names if self.KIND == _lib.KIND_VSS else tuple(n for n in names if n != "a_lat")

    def _need_physics(self):
        if not self._physics:
            raise RuntimeError("this env was built without per-env physics: pass physics=... or physics_ranges=... "
                               "(e.g. physics={}) to the constructor / make_vec")

    def set_physics(self, env_ids=None, **values):
        """Set physics parameters of the envs ``env_ids`` (None = all), e.g. ``set_physics(m_ball=0.05, mu_g=v)``.  A value is a
        scalar, a numpy array of ``len(env_ids)`` (or ``num_envs``) values, or a device tensor of that length (read on the device,
        no host copy).  Takes effect from the next step; out-of-range values raise (numpy / scalars) or are refused per env on
        the device (``sim.physics_errors()``)."""
        self._need_physics()
        torch = self._torch
        names = _lib.PHYSICS_PARAMS
        for k in values:
            if k not in self._physics_names():
                raise KeyError(f"unknown physics parameter {k!r}; known: {self._physics_names()}")
        B = self.num_envs
        if env_ids is None:
            mask = None
        else:
            ids = env_ids.cpu().numpy() if isinstance(env_ids, torch.Tensor) else np.asarray(env_ids)
            ids = np.nonzero(ids)[0] if ids.dtype == bool else ids.astype(np.int64).reshape(-1)
            mask = np.zeros(B, dtype=np.uint8)
            mask[ids] = 1
        on_dev = any(isinstance(v, torch.Tensor) and v.is_cuda for v in values.values())
        if on_dev:
            rows = torch.full((len(names), B), float("nan"), dtype=torch.float32, device=self.device)
            for k, v in values.items():
                v = torch.as_tensor(v, dtype=torch.float32, device=self.device)
                if env_ids is None:
                    rows[names.index(k)] = v.expand(B) if v.dim() == 0 else v
                else:
                    rows[names.index(k), torch.as_tensor(ids, device=self.device)] = v
            m = None if mask is None else torch.from_numpy(mask).to(self.device)
            self.sim.physics_set(rows, m, self._stream())
            self._keep_phys = (rows, m)   # alive until the launch has read them
            return
        rows = np.full((len(names), B), np.nan, dtype=np.float32)
        for k, v in values.items():
            v = np.asarray(v, dtype=np.float32)
            if env_ids is None:
                rows[names.index(k)] = v
            else:
                rows[names.index(k), ids] = v
        self.sim.physics_set(rows, mask, self._stream())

    def physics(self):
        """the current parameters: ``{name: (num_envs,) float32 tensor}`` on the env's device"""
        self._need_physics()
        raw = self.sim.physics_get(_lib.PHYS_RAW, self._stream())
        t = self._torch.from_numpy(raw).to(self.device)
        return {n: t[i] for i, n in enumerate(_lib.PHYSICS_PARAMS) if n in self._physics_names()}

    def set_physics_randomization(self, **ranges):
        """Domain randomisation: ``set_physics_randomization(m_ball=(0.04, 0.05), mu_g=None)`` — a parameter with a ``(lo, hi)``
        range is redrawn per env, on the device, at every episode start (reset() and the same-step auto-reset), keyed by
        ``(seed, env_id_base + env, episode)``; ``None`` removes its range (it then keeps its current values)."""
        self._need_physics()
        names = _lib.PHYSICS_PARAMS
        cur = getattr(self, "_ranges", {})
        for k, r in ranges.items():
            if k not in self._physics_names():
                raise KeyError(f"unknown physics parameter {k!r}; known: {self._physics_names()}")
            if r is None:
                cur.pop(k, None)
            else:
                lo, hi = r
                cur[k] = (float(lo), float(hi))
        lo = np.zeros(len(names), dtype=np.float32)
        hi = np.zeros(len(names), dtype=np.float32)
        mask = 0
        for k, (a, b) in cur.items():
            i = names.index(k)
            lo[i], hi[i] = a, b
            mask |= 1 << i
        self.sim.physics_randomize(lo, hi, mask, self._stream())
        self._ranges = cur

    def enable_graph_capture(self):
        """Make ``step()`` / ``step_random()`` capturable into a ``torch.cuda.CUDAGraph`` (hipGraph) and replayable.

        The engine's step counter — the key of the per-step random draws — moves to device memory
        (``rsx_task_enable_capture``), so every replay advances it exactly as an eager call would: a run is
        bit-identical whether its steps are issued eagerly, replayed from a graph, or both.  Call once, outside any
        capture; without it a captured ``step()`` raises instead of silently replaying one random stream.  Typical use
        (the loop of the reference's README.md:116-133 with the policy on the GPU)::

            env.enable_graph_capture()
            actions = torch.zeros(env.num_envs, env.sim.act_dim, device=env.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                actions.copy_(policy(obs))
                env.step(actions)
            for _ in range(n): g.replay()      # obs / reward / flags are the same tensor views as ever
        """
        self.sim.task_enable_capture(self._stream())
        return self

    def step_async(self, actions=None):
        """``gymnasium.vector``-style split call: enqueue the step (host-asynchronous, stream-ordered,
        exactly what ``step`` does)."""
        self._pending = self.step(actions)

    def step_wait(self, synchronize=False):
        """Results of the last ``step_async``: device tensors that are valid in stream order;
        ``synchronize=True`` also blocks the host until the launch has finished."""
        out, self._pending = self._pending, None
        if out is None:
            raise RuntimeError("step_wait() without step_async()")
        if synchronize:
            self._torch.cuda.current_stream(self.device).synchronize()
        return out

    def step_random(self, n=1, fused=False):
        """``n`` steps with device-side random actions: ``n`` launches issued from C, or
        (``fused=True``) one launch that keeps the state in registers between steps."""
        (self.sim.task_rollout if fused else self.sim.task_step_n)(int(n), self._stream())
        t = self._t
        return t["obs"], t["reward"], t["terminated"], t["truncated"], self._info()

    def checkpoint(self):
        """Everything needed to continue this run bit-identically (numpy uint8 blob, ``rsx_task_checkpoint_save``):
        simulator state, episode bookkeeping, noise state, the random streams' step counter, metrics.  Restore
        with ``restore()`` on an env of the same class, size, seed and ``env_id_base`` — in another process or on
        another GPU."""
        return self.sim.task_checkpoint(self._stream())

    def restore(self, blob):
        self.sim.task_restore(blob, self._stream())
        t = self._t
        return t["obs"], self._info()

    # ---- branching: episodes copied between envs and between handles (include/rsx.h: rsx_task_transfer) ----
    def _env_ids(self, ids, num_envs, what, is_dst):
        """ids of one side as an int32 device tensor (None = the identity map).  Device int tensors are used as they are; host
        values (numpy, lists, bool masks) are checked: range on both sides, duplicates on the destination side"""
        torch = self._torch
        if ids is None:
            return None
        if isinstance(ids, torch.Tensor) and ids.is_cuda and ids.dtype != torch.bool:
            if ids.dtype.is_floating_point or ids.dim() != 1:
                raise ValueError(f"{what} must be a 1-d integer tensor")
            if ids.device != self.device or ids.dtype != torch.int32 or not ids.is_contiguous():
                ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
            return ids
        a = ids.cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
        if a.dtype == bool:
            if a.shape != (num_envs,):
                raise ValueError(f"a bool mask for {what} must have shape ({num_envs},), got {a.shape}")
            a = np.nonzero(a)[0]
        elif a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{what} must hold integers or a bool mask")
        a = a.astype(np.int64).reshape(-1)
        if a.size and (a.min() < 0 or a.max() >= num_envs):
            raise ValueError(f"{what} holds an env id outside [0, {num_envs})")
        if is_dst and np.unique(a).size != a.size:
            raise ValueError(f"{what} names an env twice: destination ids must be distinct")
        return torch.from_numpy(a.astype(np.int32)).to(self.device)

    def copy_envs_from(self, src, src_ids=None, dst_ids=None):
        """Copy running episodes on the device: env ``src_ids[i]`` of ``src`` (another env of the same class and configuration, or
        ``self``) becomes env ``dst_ids[i]`` of ``self`` — simulator state, episode bookkeeping (step count, episode id, cumulative
        info terms, OU noise), ``obs`` / ``final_obs``, flags and per-env physics values; ``None`` on a side = envs ``0..n-1``.  Stream-
        ordered, no host copy (``rsx_task_transfer``).  Metrics, the step counter and the random keys stay ``self``'s: the copied
        episode continues under ``self``'s noise streams.

        Ids: int tensors on the device are used as they are (out-of-range pairs are skipped and counted by
        ``sim.task_transfer_errors()``; destination ids must be distinct, which is NOT checked there — a duplicated destination
        receives an unspecified mixture); numpy arrays, lists and bool masks are converted, and checked: ``ValueError`` for an id
        out of range or a duplicated destination.  Source ids may repeat (broadcast).  With ``src is self`` any map works (swaps,
        permutations, resampling), as if every read happened before every write.  Returns ``self``'s ``obs`` view."""
        if not isinstance(src, VecFusedEnv):
            raise TypeError("src must be a fused vector env (hook-written envs keep their task state in Python)")
        s_ids = self._env_ids(src_ids, src.num_envs, "src_ids", False)
        d_ids = self._env_ids(dst_ids, self.num_envs, "dst_ids", True)
        if s_ids is not None and d_ids is not None:
            if s_ids.numel() != d_ids.numel():
                raise ValueError(f"src_ids and dst_ids differ in length ({s_ids.numel()} and {d_ids.numel()})")
            n = s_ids.numel()
        elif s_ids is not None or d_ids is not None:
            n = (s_ids if s_ids is not None else d_ids).numel()
            other = self.num_envs if d_ids is None else src.num_envs
            if n > other:
                raise ValueError(f"{n} ids against the identity map of a side with {other} envs")
        else:
            if src.num_envs != self.num_envs:
                raise ValueError("give src_ids or dst_ids to copy between envs of different num_envs")
            n = self.num_envs
        self._keep_xfer = (s_ids, d_ids)   # alive until the launch has consumed them
        self.sim.task_transfer(src.sim, None if d_ids is None else d_ids.data_ptr(), None if s_ids is None else s_ids.data_ptr(),
                               n, self._stream())
        return self._t["obs"]

    def fork(self, num_envs=None, seed=None):
        """A new env of ``self``'s class and constructor configuration (device, ``env_id_base``, ``max_episode_steps``, field, team
        sizes, per-env physics on or off with ``self``'s randomisation ranges) with ``num_envs`` envs (default: as many) and ``seed``
        (default: the same), already reset: ready to receive ``copy_envs_from`` — a device-resident bank of states when it is never
        stepped (``lookahead`` works on it), or a second population."""
        kw = dict(self._ctor_kw)
        kw["num_envs"] = self.num_envs if num_envs is None else int(num_envs)
        if seed is not None:
            kw["seed"] = int(seed)
        kw.pop("physics", None)          # per-env values belong to the envs; they travel with copy_envs_from
        kw.pop("physics_ranges", None)
        if self._physics:
            kw["physics"] = {}
            ranges = dict(getattr(self, "_ranges", {}))
            if ranges:
                kw["physics_ranges"] = ranges
        env = type(self)(**kw)
        env.reset()
        return env

    def metrics(self):
        """Counters accumulated on device since construction (synchronises the stream)."""
        m = self.sim.read_metrics(self._stream())
        out = dict(zip(_lib.METRIC_NAMES, (int(v) for v in m)))
        out["return_sum"] = out.pop("return_sum_q20") / float(1 << 20)
        return out

    @property
    def state(self):
        """[state_dim + 2, num_envs] float32 view of the SoA simulator state — for READING (logging, analysis; pictures of the envs
        come from ``render()``, on the device).
        Writing it moves bodies behind the task's back: observations and per-episode task scalars are not refreshed (include/rsx.h:
        rsx_set_state); to re-place envs use ``reset_to``."""
        return self.sim.state_tensor()

    def close(self):
        self.sim.close()


_CONT_INFO = _SD_INFO + ("collision",)


class VecVSSEnv(VecFusedEnv):
    """VSS-v0 (rsoccer_gym/vss/env_vss/vss_gym.py:13): obs 40, action 2, TimeLimit 1200."""
    KIND, TASK, FIELD_TYPE, N_BLUE, N_YELLOW = _lib.KIND_VSS, _lib.TASK_VSS_V0, 0, 3, 3
    INFO_KEYS = _VSS_INFO


class VecSSLStaticDefendersEnv(VecFusedEnv):
    """SSLStaticDefenders-v0 (ssl/ssl_hw_challenge/static_defenders.py:12): obs 24, action 5,
    TimeLimit 1000, hardware-challenge field (field_type 2)."""
    KIND, TASK, FIELD_TYPE, N_BLUE, N_YELLOW = _lib.KIND_SSL, _lib.TASK_SSL_STATIC_DEFENDERS, 2, 1, 6
    INFO_KEYS = _SD_INFO


class VecSSLDribblingEnv(VecFusedEnv):
    """SSLDribbling-v0 (ssl/ssl_hw_challenge/dribbling.py:11): obs 21, action 4, TimeLimit 4800.
    info: the checkpoint counter (the reference task returns an empty info dict)."""
    KIND, TASK, FIELD_TYPE, N_BLUE, N_YELLOW = _lib.KIND_SSL, _lib.TASK_SSL_DRIBBLING, 2, 1, 4
    INFO_KEYS = ("checkpoints",)


class VecSSLContestedPossessionEnv(VecFusedEnv):
    """SSLContestedPossession-v0 (ssl/ssl_hw_challenge/contested_possession.py:11): obs 14,
    action 5, TimeLimit 1200."""
    KIND, TASK, FIELD_TYPE, N_BLUE, N_YELLOW = _lib.KIND_SSL, _lib.TASK_SSL_CONTESTED, 2, 1, 1
    INFO_KEYS = _CONT_INFO


class VecSSLPassEnduranceEnv(VecFusedEnv):
    """SSLPassEndurance-v0 (ssl/ssl_hw_challenge/pass_endurance.py:11): obs 16, action 3,
    TimeLimit 1200."""
    KIND, TASK, FIELD_TYPE, N_BLUE, N_YELLOW = _lib.KIND_SSL, _lib.TASK_SSL_PASS_ENDURANCE, 2, 2, 0
    INFO_KEYS = ("reversed_dist", "ball_grad")


class VecSSLScrimmageEnv(VecFusedEnv):
    """Synthetic SSL task in the style of the reference's example env (README.md:78-110) for team sizes
    no registered id covers — BASELINE.json configs[3]: 11v11 on the division-A field.  EVERY robot
    is commanded: action ``[B, 4 N]`` = per robot (v_x, v_y robot-local x 2.5 m/s, v_theta x 10 rad/s,
    kick 5 m/s when > 0.9); obs ``[B, 2 + 2 N]`` = normalised ball and robot positions; reward +1 / -1
    and done on a goal for blue / yellow; TimeLimit 1200.  ``crowded=True`` packs the line-up around
    the ball (worst-case all-pairs contacts)."""
    KIND = _lib.KIND_SSL
    INFO_KEYS = ("goals_blue", "goals_yellow")
    RENDER_VIEW = "field"   # division A / B: the reference's fixed 9 x 6 m window does not contain the field

    def __init__(self, num_envs, n_blue=11, n_yellow=11, field_type=1, crowded=False, **kw):
        self.N_BLUE, self.N_YELLOW, self.FIELD_TYPE = int(n_blue), int(n_yellow), int(field_type)
        self.TASK = _lib.TASK_SSL_SCRIMMAGE_CROWDED if crowded else _lib.TASK_SSL_SCRIMMAGE
        super().__init__(num_envs, **kw)
