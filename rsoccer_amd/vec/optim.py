"""The optimiser of the on-device PPO update (include/rsx.h: rsx_adam_step): ``torch.nn.utils.clip_grad_norm_`` followed by
``torch.optim.Adam`` on the three flat tensors ``VecFusedEnv.ppo_gradient`` differentiates — the actor's parameters, ``log_std`` and the
critic's parameters — with its whole state on the device, the step count included, so that a step is stream-ordered and capturable.
``DPGOptimizer`` is its off-policy twin (rsx_dpg_adam_step): the critics and the actor of TD3 / DDPG as two groups with step counts of
their own, and the Polyak step of the targets in the same two launches.  ``SACOptimizer`` is soft actor-critic's (rsx_sac_adam_step): a
third group for the scalar log-temperature, target critics only."""
import math

import numpy as np

from rsoccer_amd import _lib


def _finite(name, v, lo=None, lo_open=False):
    v = float(v)
    if not math.isfinite(v) or (lo is not None and (v <= lo if lo_open else v < lo)):
        raise ValueError(f"{name} must be finite" + ("" if lo is None else f" and {'>' if lo_open else '>='} {lo}") + f", got {v}")
    return v


def check_target_kl(target_kl):
    """``None`` (no KL stop) or a finite value > 0; returns the float the C structs take (0.0 = none)"""
    if target_kl is None:
        return 0.0
    return _finite("target_kl", target_kl, 0.0, lo_open=True)


class PPOOptimizer:
    """Global-norm clip + Adam (no amsgrad, no weight decay) for an ``MLPPolicy`` actor, its ``log_std`` ``[act_dim]`` and an
    ``MLPCritic``, in two launches per step.

    State, all on ``device``: ``m`` and ``v`` for the three flat tensors and ``counters``, int64 ``[4]`` — Adam's step count ``t``,
    the updates finished, the steps applied since the current update began, and the stopped flag of the KL stop
    (``_lib.ADAM_COUNTERS``).  The bias corrections ``1 - beta ** t`` are computed on the device from the device's ``t`` in float64,
    the betas being passed as doubles, as torch keeps them in Python floats.

    ``lr``: a float, or a float32 CUDA tensor ``[1]`` that is read on the device at every step (a schedule under graph replay: write
    the tensor, replay the graph).  ``max_grad_norm``: ``None`` or ``<= 0`` for no clipping.  Invalid values are a ``ValueError``
    naming the offender."""

    def __init__(self, policy, critic, device=0, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.5):
        import torch
        from rsoccer_amd.vec.policy import MLPCritic, MLPPolicy
        if not isinstance(policy, MLPPolicy) or isinstance(policy, MLPCritic):
            raise ValueError("policy must be an rsoccer_amd.vec.policy.MLPPolicy")
        if not isinstance(critic, MLPCritic):
            raise ValueError("critic must be an rsoccer_amd.vec.policy.MLPCritic")
        self._torch = torch
        self.device = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
        self.sizes = (policy.num_params, policy.act_dim, critic.num_params)
        self.lr = self._check_lr(lr)
        if len(tuple(betas)) != 2:
            raise ValueError(f"betas must be a pair, got {betas!r}")
        self.betas = tuple(float(b) for b in betas)
        for k, b in enumerate(self.betas):
            if not (0.0 <= b < 1.0):   # (a NaN fails both comparisons)
                raise ValueError(f"betas[{k}] must be in [0, 1), got {b}")
        self.eps = _finite("eps", eps, 0.0)
        self.max_grad_norm = 0.0 if max_grad_norm is None else _finite("max_grad_norm", max_grad_norm)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.m = [torch.zeros((n,), **f32) for n in self.sizes]
        self.v = [torch.zeros((n,), **f32) for n in self.sizes]
        self.counters = torch.zeros((4,), dtype=torch.int64, device=self.device)
        self._ws = torch.zeros((_lib.ADAM_WORKSPACE_BYTES // 8,), dtype=torch.float64, device=self.device)

    def _check_lr(self, lr):
        torch = self._torch
        if isinstance(lr, torch.Tensor):
            if lr.dtype != torch.float32 or lr.numel() != 1 or lr.device != self.device:
                raise ValueError(f"lr as a tensor must be one float32 on {self.device}, got {lr.dtype} {list(lr.shape)} on {lr.device}")
            return lr
        return _finite("lr", lr, 0.0)

    def _stream(self):
        try:
            return self._torch._C._cuda_getCurrentRawStream(self.device.index)
        except AttributeError:
            return self._torch.cuda.current_stream(self.device).cuda_stream

    # ---- the C structs ----
    def cfg(self, lr=None, target_kl=None):
        """the ``rsx_adam_cfg`` of this optimiser (``lr``: an override for this call)"""
        lr = self.lr if lr is None else self._check_lr(lr)
        by_ptr = isinstance(lr, self._torch.Tensor)
        return _lib.AdamCfg(self.betas[0], self.betas[1], lr.data_ptr() if by_ptr else None, 0.0 if by_ptr else lr, self.eps,
                            self.max_grad_norm, check_target_kl(target_kl))

    def state(self):
        """the ``rsx_adam_state`` of this optimiser"""
        (ma, ml, mc), (va, vl, vc) = self.m, self.v
        return _lib.AdamState(ma.data_ptr(), va.data_ptr(), ml.data_ptr(), vl.data_ptr(), mc.data_ptr(), vc.data_ptr(),
                              self.counters.data_ptr(), *self.sizes)

    def _need(self, name, t, n):
        torch = self._torch
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if tuple(t.shape) != (n,):
            raise ValueError(f"{name} must be [{n}], got {list(t.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be torch.float32, got {t.dtype}")
        if t.device != self.device:
            raise ValueError(f"{name} is on {t.device}, the optimiser on {self.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        return t.detach()

    # ---- steps ----
    def step(self, params, log_std, critic_params, grad_params, grad_log_std, grad_critic_params, approx_kl=None, target_kl=None,
             lr=None):
        """Clip the three gradients by their global norm and take one Adam step on ``params`` ``[P]``, ``log_std`` ``[act_dim]`` and
        ``critic_params`` ``[Pc]`` IN PLACE (``rsx_adam_step``; the arithmetic is written out in ``include/rsx.h``).  The gradients
        are ``ppo_gradient()``'s outputs and are not changed.

        With ``target_kl`` and ``approx_kl`` (a 0-d or ``[1]`` float32 device tensor: ``ppo_gradient``'s ``stats["approx_kl"]``) a
        step whose ``approx_kl`` exceeds ``target_kl`` sets the stopped flag before its own step, and a step that finds the flag set
        changes nothing — no parameter, no moment, not ``t``; its launches still run.  ``begin_update()`` clears the flag.

        Returns 0-d device views ``grad_norm`` (before the clip) and ``applied`` (1.0 or 0.0).  Never synchronises, capturable."""
        torch = self._torch
        names = ("params", "log_std", "critic_params")
        ps = [self._need(k, t, n) for k, t, n in zip(names, (params, log_std, critic_params), self.sizes)]
        gs = [self._need("grad_" + k, t, n) for k, t, n in zip(names, (grad_params, grad_log_std, grad_critic_params), self.sizes)]
        cfg = self.cfg(lr, target_kl)
        kl = None
        if approx_kl is not None:
            if not isinstance(approx_kl, torch.Tensor) or approx_kl.numel() != 1 or approx_kl.dtype != torch.float32 or approx_kl.device != self.device:
                raise ValueError(f"approx_kl must be one float32 on {self.device}")
            kl = approx_kl
        stats = torch.empty((2,), dtype=torch.float32, device=self.device)
        io = _lib.AdamIo(ps[0].data_ptr(), ps[1].data_ptr(), ps[2].data_ptr(), gs[0].data_ptr(), gs[1].data_ptr(), gs[2].data_ptr(),
                         None if kl is None else kl.data_ptr(), stats.data_ptr(), self._ws.data_ptr())
        with torch.cuda.device(self.device):
            _lib.adam_step(cfg, self.state(), io, self._stream())
        return {"grad_norm": stats[0], "applied": stats[1]}

    def begin_update(self):
        """an update begins: the steps-applied count and the stopped flag are cleared (what ``ppo_update()`` does first)"""
        with self._torch.cuda.device(self.device):
            _lib.adam_mark(self.state(), False, self._stream())

    def end_update(self):
        """an update ends: the update count, which keys ``minibatch_rows``, advances (what ``ppo_update()`` does last)"""
        with self._torch.cuda.device(self.device):
            _lib.adam_mark(self.state(), True, self._stream())

    # ---- checkpoints ----
    def state_dict(self):
        """clones of ``m``, ``v`` (three tensors each) and ``counters``, and the hyper-parameters: a training checkpoint round-trips"""
        lr = self.lr
        return {"m": [t.clone() for t in self.m], "v": [t.clone() for t in self.v], "counters": self.counters.clone(),
                "lr": lr.clone() if isinstance(lr, self._torch.Tensor) else lr, "betas": self.betas, "eps": self.eps,
                "max_grad_norm": self.max_grad_norm}

    def load_state_dict(self, sd):
        """copies a ``state_dict()`` into this optimiser's own tensors (their addresses stay: a captured graph keeps working);
        tensors of another size are a ``ValueError``"""
        torch = self._torch
        for key in ("m", "v", "counters"):
            if key not in sd:
                raise ValueError(f"state dict lacks {key!r}")
        for key, mine in (("m", self.m), ("v", self.v)):
            theirs = list(sd[key])
            if len(theirs) != 3:
                raise ValueError(f"state dict's {key!r} must hold three tensors, got {len(theirs)}")
            for k, (a, b) in enumerate(zip(mine, theirs)):
                if tuple(np.shape(b)) != tuple(a.shape):
                    raise ValueError(f"state dict's {key}[{k}] must be {list(a.shape)}, got {list(np.shape(b))}")
        if tuple(np.shape(sd["counters"])) != (4,):
            raise ValueError(f"state dict's counters must be [4], got {list(np.shape(sd['counters']))}")
        for key, mine in (("m", self.m), ("v", self.v)):
            for a, b in zip(mine, sd[key]):
                a.copy_(torch.as_tensor(b).to(device=self.device, dtype=torch.float32))
        self.counters.copy_(torch.as_tensor(sd["counters"]).to(device=self.device, dtype=torch.int64))
        if "lr" in sd:
            lr = sd["lr"]
            if isinstance(lr, torch.Tensor) and isinstance(self.lr, torch.Tensor):
                self.lr.copy_(lr.to(self.device))
            else:
                self.lr = self._check_lr(lr.to(self.device) if isinstance(lr, torch.Tensor) else lr)
        if "betas" in sd:
            self.betas = tuple(float(b) for b in sd["betas"])
        if "eps" in sd:
            self.eps = _finite("eps", sd["eps"], 0.0)
        if "max_grad_norm" in sd:
            self.max_grad_norm = _finite("max_grad_norm", sd["max_grad_norm"])


class DPGOptimizer:
    """The optimiser step of TD3 / DDPG for an ``MLPPolicy`` actor and ``n_critics`` ``MLPQCritic`` networks, in two launches
    (include/rsx.h: rsx_dpg_adam_step): two parameter groups — the critics' ``[C, Pc]`` tensor and the actor's ``[P]`` — each with its
    own global-norm clip, its own Adam (no amsgrad, no weight decay), its own ``lr`` and its own step count, as two torch optimisers
    behind two ``clip_grad_norm_`` calls; and the Polyak step of both targets behind it, on the new parameters.

    State, all on ``device``: ``m`` and ``v`` for the two flat tensors (actor, critics) and ``counters``, int64 ``[4]``
    (``_lib.DPG_COUNTERS``): the critics' ``t``, the actor's ``t`` (it advances on actor steps only), the gradient steps finished, one
    spare.  ``steps`` is a ``[1]`` view of the third: pass it as ``noise_step=`` to ``dpg_gradient`` and as ``step=`` to
    ``ReplayBuffer.sample_rows_device`` and a replayed graph draws new noise and new rows after every step.

    ``lr_actor`` / ``lr_critic``: a float, or a float32 CUDA tensor ``[1]`` read on the device at every step.  ``max_grad_norm``:
    ``None`` or ``<= 0`` for no clipping, else the bound of each group's own norm.  ``tau`` in ``[0, 1]``.  Invalid values are a
    ``ValueError`` naming the offender."""

    def __init__(self, policy, critic, n_critics, device=0, lr_actor=3e-4, lr_critic=3e-4, betas=(0.9, 0.999), eps=1e-8,
                 max_grad_norm=None, tau=0.005):
        import torch
        from rsoccer_amd.vec.policy import MLPCritic, MLPPolicy, MLPQCritic
        if not isinstance(policy, MLPPolicy) or isinstance(policy, (MLPCritic, MLPQCritic)):
            raise ValueError("policy must be an rsoccer_amd.vec.policy.MLPPolicy")
        if not isinstance(critic, MLPQCritic):
            raise ValueError("critic must be an rsoccer_amd.vec.policy.MLPQCritic")
        if n_critics not in (1, 2):
            raise ValueError(f"n_critics must be 1 or 2, got {n_critics!r}")
        self._torch = torch
        self.device = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
        self.n_critics = int(n_critics)
        self.sizes = (policy.num_params, self.n_critics * critic.num_params)
        self.lr_actor = self._check_lr("lr_actor", lr_actor)
        self.lr_critic = self._check_lr("lr_critic", lr_critic)
        if len(tuple(betas)) != 2:
            raise ValueError(f"betas must be a pair, got {betas!r}")
        self.betas = tuple(float(b) for b in betas)
        for k, b in enumerate(self.betas):
            if not (0.0 <= b < 1.0):   # (a NaN fails both comparisons)
                raise ValueError(f"betas[{k}] must be in [0, 1), got {b}")
        self.eps = _finite("eps", eps, 0.0)
        self.max_grad_norm = 0.0 if max_grad_norm is None else _finite("max_grad_norm", max_grad_norm)
        self.tau = self._check_tau(tau)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.m = [torch.zeros((n,), **f32) for n in self.sizes]
        self.v = [torch.zeros((n,), **f32) for n in self.sizes]
        self.counters = torch.zeros((4,), dtype=torch.int64, device=self.device)
        self._ws = torch.zeros((_lib.DPG_ADAM_WORKSPACE_BYTES // 8,), dtype=torch.float64, device=self.device)

    @staticmethod
    def _check_tau(tau):
        tau = float(tau)
        if not (0.0 <= tau <= 1.0):   # (a NaN fails both comparisons)
            raise ValueError(f"tau must be in [0, 1], got {tau}")
        return tau

    def _check_lr(self, name, lr):
        torch = self._torch
        if isinstance(lr, torch.Tensor):
            if lr.dtype != torch.float32 or lr.numel() != 1 or lr.device != self.device:
                raise ValueError(f"{name} as a tensor must be one float32 on {self.device}, got {lr.dtype} {list(lr.shape)} on {lr.device}")
            return lr
        return _finite(name, lr, 0.0)

    _stream = PPOOptimizer._stream

    @property
    def steps(self):
        """the gradient steps finished: an int64 ``[1]`` view of the device counter (the key of the row draws and the smoothing noise)"""
        k = _lib.DPG_COUNTERS.index("steps")
        return self.counters[k:k + 1]

    # ---- the C structs ----
    def cfg(self):
        """the ``rsx_dpg_adam_cfg`` of this optimiser"""
        is_t = lambda x: isinstance(x, self._torch.Tensor)   # noqa: E731
        la, lc = self.lr_actor, self.lr_critic
        return _lib.DpgAdamCfg(self.betas[0], self.betas[1], la.data_ptr() if is_t(la) else None, lc.data_ptr() if is_t(lc) else None,
                               0.0 if is_t(la) else la, 0.0 if is_t(lc) else lc, self.eps, self.max_grad_norm, self.tau)

    def state(self):
        """the ``rsx_dpg_adam_state`` of this optimiser"""
        (ma, mc), (va, vc) = self.m, self.v
        return _lib.DpgAdamState(ma.data_ptr(), va.data_ptr(), mc.data_ptr(), vc.data_ptr(), self.counters.data_ptr(), *self.sizes)

    def _need(self, name, t, n):
        torch = self._torch
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if t.numel() != n or t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[0] != self.n_critics):
            raise ValueError(f"{name} must hold {n} floats ([{n}] or [{self.n_critics}, {n // self.n_critics}]), got {list(t.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be torch.float32, got {t.dtype}")
        if t.device != self.device:
            raise ValueError(f"{name} is on {t.device}, the optimiser on {self.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        return t.detach()

    # ---- steps ----
    def step(self, params, target_params, critic_params, target_critic_params, grad_params, grad_critic_params, update_targets=None):
        """One optimiser step IN PLACE (``rsx_dpg_adam_step``; the arithmetic is written out in ``include/rsx.h``): clip + Adam on
        ``critic_params`` ``[C, Pc]`` with ``grad_critic_params``; with ``grad_params`` not ``None`` also on ``params`` ``[P]`` (an
        actor step — without it the actor's parameters, moments and step count stay exactly as they were); with ``update_targets``
        the Polyak step ``target += tau * (live - target)`` of both targets on the new parameters.  ``update_targets=None``: iff the
        actor stepped (TD3).  The gradients are ``dpg_gradient()``'s outputs and are not changed.

        Returns 0-d device views ``grad_norm_critic``, ``grad_norm_actor`` (before the clip; 0 without an actor step) and
        ``targets_moved`` (1.0 or 0.0).  Never synchronises, capturable."""
        torch = self._torch
        na, nc = self.sizes
        p, tp = self._need("params", params, na), self._need("target_params", target_params, na)
        cp, tcp = self._need("critic_params", critic_params, nc), self._need("target_critic_params", target_critic_params, nc)
        ga = None if grad_params is None else self._need("grad_params", grad_params, na)
        gc = self._need("grad_critic_params", grad_critic_params, nc)
        move = (ga is not None) if update_targets is None else bool(update_targets)
        stats = torch.empty((3,), dtype=torch.float32, device=self.device)
        io = _lib.DpgAdamIo(p.data_ptr(), tp.data_ptr(), cp.data_ptr(), tcp.data_ptr(), None if ga is None else ga.data_ptr(), gc.data_ptr(),
                            stats.data_ptr(), self._ws.data_ptr(), 1 if move else 0)
        with torch.cuda.device(self.device):
            _lib.dpg_adam_step(self.cfg(), self.state(), io, self._stream())
        return {name: stats[k] for k, name in enumerate(_lib.DPG_ADAM_STATS)}

    # ---- checkpoints ----
    def state_dict(self):
        """clones of ``m``, ``v`` (two tensors each: actor, critics) and ``counters``, and the hyper-parameters"""
        clone = lambda x: x.clone() if isinstance(x, self._torch.Tensor) else x   # noqa: E731
        return {"m": [t.clone() for t in self.m], "v": [t.clone() for t in self.v], "counters": self.counters.clone(),
                "lr_actor": clone(self.lr_actor), "lr_critic": clone(self.lr_critic), "betas": self.betas, "eps": self.eps,
                "max_grad_norm": self.max_grad_norm, "tau": self.tau}

    def load_state_dict(self, sd):
        """copies a ``state_dict()`` into this optimiser's own tensors (their addresses stay: a captured graph keeps working);
        tensors of another size are a ``ValueError``"""
        torch = self._torch
        for key in ("m", "v", "counters"):
            if key not in sd:
                raise ValueError(f"state dict lacks {key!r}")
        for key, mine in (("m", self.m), ("v", self.v)):
            theirs = list(sd[key])
            if len(theirs) != 2:
                raise ValueError(f"state dict's {key!r} must hold two tensors, got {len(theirs)}")
            for k, (a, b) in enumerate(zip(mine, theirs)):
                if tuple(np.shape(b)) != tuple(a.shape):
                    raise ValueError(f"state dict's {key}[{k}] must be {list(a.shape)}, got {list(np.shape(b))}")
        if tuple(np.shape(sd["counters"])) != (4,):
            raise ValueError(f"state dict's counters must be [4], got {list(np.shape(sd['counters']))}")
        for key, mine in (("m", self.m), ("v", self.v)):
            for a, b in zip(mine, sd[key]):
                a.copy_(torch.as_tensor(b).to(device=self.device, dtype=torch.float32))
        self.counters.copy_(torch.as_tensor(sd["counters"]).to(device=self.device, dtype=torch.int64))
        for name in ("lr_actor", "lr_critic"):
            if name in sd:
                lr, mine = sd[name], getattr(self, name)
                if isinstance(lr, torch.Tensor) and isinstance(mine, torch.Tensor):
                    mine.copy_(lr.to(self.device))
                else:
                    setattr(self, name, self._check_lr(name, lr.to(self.device) if isinstance(lr, torch.Tensor) else lr))
        if "betas" in sd:
            self.betas = tuple(float(b) for b in sd["betas"])
        if "eps" in sd:
            self.eps = _finite("eps", sd["eps"], 0.0)
        if "max_grad_norm" in sd:
            self.max_grad_norm = _finite("max_grad_norm", sd["max_grad_norm"])
        if "tau" in sd:
            self.tau = self._check_tau(sd["tau"])


class SACOptimizer:
    """The optimiser step of soft actor-critic for an ``MLPGaussianPolicy`` actor, ``n_critics`` ``MLPQCritic`` networks and the
    log-temperature, in two launches (include/rsx.h: rsx_sac_adam_step): three parameter groups — the critics' ``[C, Pc]`` tensor, the
    actor's ``[P]`` and ``log_alpha`` ``[1]`` — each with its own Adam (no amsgrad, no weight decay), its own ``lr`` and its own step
    count, as three torch optimisers; the critics and the actor each behind a ``clip_grad_norm_`` of their own, ``log_alpha`` never
    clipped; and the Polyak step of the target critics behind it, on the new parameters.  There is no target actor.

    State, all on ``device``: ``m`` and ``v`` for the three tensors (actor, critics, log_alpha) and ``counters``, int64 ``[4]``
    (``_lib.SAC_COUNTERS``): the critics' ``t``, the actor's, ``log_alpha``'s (a group's ``t`` advances only when the group steps) and
    the gradient steps finished.  ``steps`` is a ``[1]`` view of the fourth: pass it as ``noise_step=`` to ``sac_gradient`` and as
    ``step=`` to ``ReplayBuffer.sample_rows_device`` and a replayed graph draws new noise and new rows after every step.

    ``lr_actor`` / ``lr_critic`` / ``lr_alpha``: a float, or a float32 CUDA tensor ``[1]`` read on the device at every step.
    ``max_grad_norm``: ``None`` or ``<= 0`` for no clipping, else the bound of the critics' norm and of the actor's, each on its own.
    ``tau`` in ``[0, 1]``.  Invalid values are a ``ValueError`` naming the offender, raised before anything is allocated."""

    def __init__(self, policy, critic, n_critics, device=0, lr_actor=3e-4, lr_critic=3e-4, lr_alpha=3e-4, betas=(0.9, 0.999), eps=1e-8,
                 max_grad_norm=None, tau=0.005):
        import torch
        from rsoccer_amd.vec.policy import MLPGaussianPolicy, MLPQCritic
        if not isinstance(policy, MLPGaussianPolicy):
            raise ValueError("policy must be an rsoccer_amd.vec.policy.MLPGaussianPolicy")
        if not isinstance(critic, MLPQCritic):
            raise ValueError("critic must be an rsoccer_amd.vec.policy.MLPQCritic")
        if n_critics not in (1, 2):
            raise ValueError(f"n_critics must be 1 or 2, got {n_critics!r}")
        self._torch = torch
        self.device = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
        self.n_critics = int(n_critics)
        self.sizes = (policy.num_params, self.n_critics * critic.num_params)
        self.lr_actor = self._check_lr("lr_actor", lr_actor)
        self.lr_critic = self._check_lr("lr_critic", lr_critic)
        self.lr_alpha = self._check_lr("lr_alpha", lr_alpha)
        if len(tuple(betas)) != 2:
            raise ValueError(f"betas must be a pair, got {betas!r}")
        self.betas = tuple(float(b) for b in betas)
        for k, b in enumerate(self.betas):
            if not (0.0 <= b < 1.0):   # (a NaN fails both comparisons)
                raise ValueError(f"betas[{k}] must be in [0, 1), got {b}")
        self.eps = _finite("eps", eps, 0.0)
        self.max_grad_norm = 0.0 if max_grad_norm is None else _finite("max_grad_norm", max_grad_norm)
        self.tau = DPGOptimizer._check_tau(tau)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.m = [torch.zeros((n,), **f32) for n in self.sizes + (1,)]
        self.v = [torch.zeros((n,), **f32) for n in self.sizes + (1,)]
        self.counters = torch.zeros((4,), dtype=torch.int64, device=self.device)
        self._ws = torch.zeros((_lib.SAC_ADAM_WORKSPACE_BYTES // 8,), dtype=torch.float64, device=self.device)

    _check_lr = DPGOptimizer._check_lr
    _stream = PPOOptimizer._stream
    _need = DPGOptimizer._need

    @property
    def steps(self):
        """the gradient steps finished: an int64 ``[1]`` view of the device counter (the key of the row draws and the sampling noise)"""
        k = _lib.SAC_COUNTERS.index("steps")
        return self.counters[k:k + 1]

    # ---- the C structs ----
    def cfg(self):
        """the ``rsx_sac_adam_cfg`` of this optimiser"""
        is_t = lambda x: isinstance(x, self._torch.Tensor)   # noqa: E731
        lrs = (self.lr_actor, self.lr_critic, self.lr_alpha)
        return _lib.SacAdamCfg(self.betas[0], self.betas[1], *(x.data_ptr() if is_t(x) else None for x in lrs),
                               *(0.0 if is_t(x) else x for x in lrs), self.eps, self.max_grad_norm, self.tau)

    def state(self):
        """the ``rsx_sac_adam_state`` of this optimiser"""
        (ma, mc, ml), (va, vc, vl) = self.m, self.v
        return _lib.SacAdamState(ma.data_ptr(), va.data_ptr(), mc.data_ptr(), vc.data_ptr(), ml.data_ptr(), vl.data_ptr(),
                                 self.counters.data_ptr(), *self.sizes)

    def _need_scalar(self, name, t):
        torch = self._torch
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if tuple(t.shape) != (1,):
            raise ValueError(f"{name} must be [1], got {list(t.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be torch.float32, got {t.dtype}")
        if t.device != self.device:
            raise ValueError(f"{name} is on {t.device}, the optimiser on {self.device}")
        return t.detach()

    # ---- steps ----
    def step(self, params, critic_params, target_critic_params, log_alpha, grad_params, grad_critic_params, grad_log_alpha,
             update_targets=True):
        """One optimiser step IN PLACE (``rsx_sac_adam_step``; the arithmetic is written out in ``include/rsx.h``): clip + Adam on
        ``critic_params`` ``[C, Pc]`` with ``grad_critic_params``; with ``grad_params`` not ``None`` also on ``params`` ``[P]``; with
        ``grad_log_alpha`` not ``None`` Adam (no clip) on ``log_alpha`` ``[1]``; a group whose gradient is ``None`` keeps its
        parameters, moments and step count exactly as they were.  With ``update_targets`` the Polyak step
        ``target += tau * (live - target)`` of the target critics on the new parameters.  The gradients are ``sac_gradient()``'s
        outputs and are not changed.

        Returns 0-d device views ``grad_norm_critic``, ``grad_norm_actor`` (before the clip; 0 without an actor step), ``log_alpha``
        (after the step) and ``targets_moved`` (1.0 or 0.0).  Never synchronises, capturable."""
        torch = self._torch
        na, nc = self.sizes
        p = self._need("params", params, na)
        cp, tcp = self._need("critic_params", critic_params, nc), self._need("target_critic_params", target_critic_params, nc)
        la = self._need_scalar("log_alpha", log_alpha)
        ga = None if grad_params is None else self._need("grad_params", grad_params, na)
        gc = self._need("grad_critic_params", grad_critic_params, nc)
        gl = None if grad_log_alpha is None else self._need_scalar("grad_log_alpha", grad_log_alpha)
        stats = torch.empty((len(_lib.SAC_ADAM_STATS),), dtype=torch.float32, device=self.device)
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        io = _lib.SacAdamIo(ptr(p), ptr(cp), ptr(tcp), ptr(la), ptr(ga), ptr(gc), ptr(gl), ptr(stats), ptr(self._ws),
                            1 if update_targets else 0)
        with torch.cuda.device(self.device):
            _lib.sac_adam_step(self.cfg(), self.state(), io, self._stream())
        return {name: stats[k] for k, name in enumerate(_lib.SAC_ADAM_STATS)}

    # ---- checkpoints ----
    def state_dict(self):
        """clones of ``m``, ``v`` (three tensors each: actor, critics, log_alpha) and ``counters``, and the hyper-parameters"""
        clone = lambda x: x.clone() if isinstance(x, self._torch.Tensor) else x   # noqa: E731
        return {"m": [t.clone() for t in self.m], "v": [t.clone() for t in self.v], "counters": self.counters.clone(),
                "lr_actor": clone(self.lr_actor), "lr_critic": clone(self.lr_critic), "lr_alpha": clone(self.lr_alpha),
                "betas": self.betas, "eps": self.eps, "max_grad_norm": self.max_grad_norm, "tau": self.tau}

    def load_state_dict(self, sd):
        """copies a ``state_dict()`` into this optimiser's own tensors (their addresses stay: a captured graph keeps working);
        tensors of another size are a ``ValueError``"""
        torch = self._torch
        for key in ("m", "v", "counters"):
            if key not in sd:
                raise ValueError(f"state dict lacks {key!r}")
        for key, mine in (("m", self.m), ("v", self.v)):
            theirs = list(sd[key])
            if len(theirs) != 3:
                raise ValueError(f"state dict's {key!r} must hold three tensors, got {len(theirs)}")
            for k, (a, b) in enumerate(zip(mine, theirs)):
                if tuple(np.shape(b)) != tuple(a.shape):
                    raise ValueError(f"state dict's {key}[{k}] must be {list(a.shape)}, got {list(np.shape(b))}")
        if tuple(np.shape(sd["counters"])) != (4,):
            raise ValueError(f"state dict's counters must be [4], got {list(np.shape(sd['counters']))}")
        for key, mine in (("m", self.m), ("v", self.v)):
            for a, b in zip(mine, sd[key]):
                a.copy_(torch.as_tensor(b).to(device=self.device, dtype=torch.float32))
        self.counters.copy_(torch.as_tensor(sd["counters"]).to(device=self.device, dtype=torch.int64))
        for name in ("lr_actor", "lr_critic", "lr_alpha"):
            if name in sd:
                lr, mine = sd[name], getattr(self, name)
                if isinstance(lr, torch.Tensor) and isinstance(mine, torch.Tensor):
                    mine.copy_(lr.to(self.device))
                else:
                    setattr(self, name, self._check_lr(name, lr.to(self.device) if isinstance(lr, torch.Tensor) else lr))
        if "betas" in sd:
            self.betas = tuple(float(b) for b in sd["betas"])
        if "eps" in sd:
            self.eps = _finite("eps", sd["eps"], 0.0)
        if "max_grad_norm" in sd:
            self.max_grad_norm = _finite("max_grad_norm", sd["max_grad_norm"])
        if "tau" in sd:
            self.tau = DPGOptimizer._check_tau(sd["tau"])
