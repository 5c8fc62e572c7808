"""A ring buffer of transitions for off-policy training (DDPG, TD3): ``VecFusedEnv.collect`` fills it, ``VecFusedEnv.dpg_gradient``
reads it through ``rows``.  Plain torch on whatever device it is given; the write head and the fill count live on that device, so no
call synchronises or has a data-dependent shape, and all of them can be captured into a ``torch.cuda.CUDAGraph``."""


class ReplayBuffer:
    """``capacity`` flat transition rows ``(obs, action, reward, next_obs, terminated)``.

    ``next_obs`` of a row is its TRUE successor: the terminal observation where the episode ended at that step (the env has reset
    itself by then), else the next step's observation.  A row that ended on a time limit only is stored with ``terminated = 0`` and
    its terminal observation, so a target computed from it bootstraps through the limit, as ``advantages()`` does."""

    def __init__(self, capacity, obs_dim, act_dim, device):
        import torch
        self.capacity, self.obs_dim, self.act_dim = int(capacity), int(obs_dim), int(act_dim)
        if self.capacity < 1 or self.obs_dim < 1 or self.act_dim < 1:
            raise ValueError(f"capacity, obs_dim and act_dim must be >= 1, got {capacity}, {obs_dim}, {act_dim}")
        self.device = torch.device(device)
        f32 = dict(dtype=torch.float32, device=self.device)
        n = self.capacity
        self.obs = torch.zeros((n, self.obs_dim), **f32)
        self.actions = torch.zeros((n, self.act_dim), **f32)
        self.reward = torch.zeros((n,), **f32)
        self.next_obs = torch.zeros((n, self.obs_dim), **f32)
        self.terminated = torch.zeros((n,), dtype=torch.bool, device=self.device)
        self.head = torch.zeros((1,), dtype=torch.int64, device=self.device)   # the next row to write
        self.fill = torch.zeros((1,), dtype=torch.int64, device=self.device)   # rows that hold a transition

    def add(self, batch):
        """Append the ``T * B`` transitions of a ``collect(..., return_final_obs=True)`` batch ``[T, B, ...]`` (or of ``seat_rows()`` of a
        team batch) at the write head, step-major, wrapping around the end.  Refused: a batch without ``final_obs`` (the successor of an
        ended row would be the next episode's first observation) and a batch of more rows than the capacity."""
        import torch
        for key in ("obs", "actions", "reward", "terminated", "truncated", "next_obs"):
            if key not in batch:
                raise ValueError(f"batch lacks {key!r}")
        if batch.get("final_obs") is None:
            raise ValueError("batch lacks 'final_obs': collect it with return_final_obs=True")
        obs = batch["obs"]
        if obs.dim() != 3 or obs.shape[2] != self.obs_dim:
            raise ValueError(f"batch['obs'] must be [T, B, {self.obs_dim}], got {list(obs.shape)}")
        T, B = int(obs.shape[0]), int(obs.shape[1])
        n = T * B
        if n > self.capacity:
            raise ValueError(f"the batch has {n} rows, the buffer holds {self.capacity}")
        want = {"actions": (T, B, self.act_dim), "reward": (T, B), "terminated": (T, B), "truncated": (T, B),
                "final_obs": (T, B, self.obs_dim), "next_obs": (B, self.obs_dim)}
        for key, shape in want.items():
            if tuple(batch[key].shape) != shape:
                raise ValueError(f"batch[{key!r}] must be {list(shape)}, got {list(batch[key].shape)}")
        term, trunc = batch["terminated"].bool(), batch["truncated"].bool()
        following = torch.cat([obs[1:], batch["next_obs"].unsqueeze(0)], dim=0)
        succ = torch.where((term | trunc).unsqueeze(-1), batch["final_obs"], following)
        at = (self.head + torch.arange(n, device=self.device)) % self.capacity
        to = lambda t: t.to(self.device)   # noqa: E731
        self.obs.index_copy_(0, at, to(obs.reshape(n, self.obs_dim)))
        self.actions.index_copy_(0, at, to(batch["actions"].reshape(n, self.act_dim)))
        self.reward.index_copy_(0, at, to(batch["reward"].reshape(n)))
        self.next_obs.index_copy_(0, at, to(succ.reshape(n, self.obs_dim)))
        self.terminated.index_copy_(0, at, to(term.reshape(n)))
        self.head.copy_((self.head + n) % self.capacity)
        self.fill.copy_(torch.clamp(self.fill + n, max=self.capacity))
        return n

    def sample_rows(self, m, generator=None):
        """``m`` int32 row indices, uniform over the filled part with repeats, computed on the device from the device's fill count
        (``floor(u * fill)``): what ``dpg_gradient(rows=...)`` takes.  On an empty buffer every index is -1, which ``dpg_gradient``
        skips and counts."""
        import torch
        m = int(m)
        if m < 1:
            raise ValueError(f"m must be >= 1, got {m}")
        u = torch.rand((m,), dtype=torch.float64, device=self.device, generator=generator)
        return torch.minimum((u * self.fill).to(torch.int64), self.fill - 1).to(torch.int32)

    def sample_rows_device(self, m, seed=0, step=0):
        """``m`` int32 row indices, uniform over the filled part with repeats, drawn by the engine's own counter-based generator in
        one launch (``rsx_replay_sample_rows``; the integer arithmetic is written out in ``include/rsx.h``): entry ``t`` depends on
        ``(seed, step, t)`` and the device's fill count only.  ``step``: an int, or an int64 device tensor ``[1]`` read when the launch
        runs — ``DPGOptimizer.steps``, so that a replayed graph draws new rows after every gradient step.  On an empty buffer every
        index is -1.  Needs the buffer on a GPU; never synchronises, capturable."""
        import torch
        from rsoccer_amd import _lib
        m = int(m)
        if m < 1 or m > 2 ** 31 - 1:
            raise ValueError(f"m must be in 1 .. 2^31 - 1, got {m}")
        if self.capacity > 2 ** 31 - 1:
            raise ValueError(f"capacity must be at most 2^31 - 1, got {self.capacity}")
        if self.device.type != "cuda":
            raise ValueError(f"the buffer is on {self.device}: sample_rows_device needs it on a GPU (sample_rows works anywhere)")
        step_ptr, step_v = None, 0
        if isinstance(step, torch.Tensor):
            if step.dtype != torch.int64 or tuple(step.shape) != (1,) or step.device != self.fill.device:
                raise ValueError(f"step as a tensor must be int64 [1] on {self.fill.device}, got {step.dtype} {list(step.shape)} on {step.device}")
            step_ptr = step.data_ptr()
        else:
            step_v = int(step)
            if not -2 ** 63 <= step_v < 2 ** 63:
                raise ValueError(f"step must fit 64 bits, got {step}")
        rows = torch.empty((m,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            try:
                stream = torch._C._cuda_getCurrentRawStream(self.fill.device.index)
            except AttributeError:
                stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.replay_sample_rows(rows.data_ptr(), m, self.capacity, 0, self.fill.data_ptr(), int(seed), step_v, step_ptr, stream)
        self._keep_step = step   # alive until the launch has consumed it
        return rows

    def data(self):
        """the mapping ``VecFusedEnv.dpg_gradient`` takes: views of the whole ring (``N = capacity``); rows behind the fill count
        hold zeros and are never drawn by ``sample_rows``"""
        return {"obs": self.obs, "actions": self.actions, "reward": self.reward, "next_obs": self.next_obs, "terminated": self.terminated}


class PrioritizedReplayBuffer(ReplayBuffer):
    """A ``ReplayBuffer`` on a GPU with n-step transitions and proportional prioritised sampling, all on the device
    (``rsx_replay_add_nstep``, ``rsx_replay_set_priorities``, ``rsx_replay_sample_prioritized``; the arithmetic is written out in
    ``include/rsx.h``).  Rows gain a ``discount`` (``gamma^m`` of the row's own window of ``m <= n_step`` steps) that
    ``dpg_gradient`` / ``sac_gradient`` use per row when ``data()`` is passed to them.  Priorities live in a sum tree of fan-out 64
    whose leaves hold ``(|td_error| + eps)^alpha``; a new row gets the largest leaf value written so far (1 at the start).  No call
    synchronises or allocates a data-dependent shape; all can be captured into a ``torch.cuda.CUDAGraph``.  ``sample_rows`` and
    ``sample_rows_device`` stay available for uniform draws."""

    def __init__(self, capacity, obs_dim, act_dim, device, alpha=0.6, n_step=1, gamma=0.99, eps=1e-6):
        import math
        import torch
        from rsoccer_amd import _lib
        alpha, gamma, eps = float(alpha), float(gamma), float(eps)
        if not (math.isfinite(alpha) and alpha >= 0.0):
            raise ValueError(f"alpha must be finite and >= 0, got {alpha}")
        if int(n_step) != n_step or not 1 <= int(n_step) <= 16:
            raise ValueError(f"n_step must be an integer in 1 .. 16, got {n_step}")
        if not (math.isfinite(gamma) and 0.0 <= gamma <= 1.0):
            raise ValueError(f"gamma must be in [0, 1], got {gamma}")
        if not (math.isfinite(eps) and eps >= 0.0):
            raise ValueError(f"eps must be finite and >= 0, got {eps}")
        if int(capacity) > 2 ** 31 - 1:
            raise ValueError(f"capacity must be at most 2^31 - 1, got {capacity}")
        if torch.device(device).type != "cuda":
            raise ValueError(f"device must be a GPU, got {torch.device(device)}: the prioritised ring's kernels run there (ReplayBuffer works anywhere)")
        super().__init__(capacity, obs_dim, act_dim, device)
        self.alpha, self.n_step, self.gamma, self.eps = alpha, int(n_step), gamma, eps
        self.discount = torch.zeros((self.capacity,), dtype=torch.float32, device=self.device)
        floats, self.tree_levels, self.tree_offsets = _lib.replay_tree_geometry(self.capacity)
        self.tree = torch.zeros((floats,), dtype=torch.float32, device=self.device)
        # RSX_REPLAY_STATE_*: the running maximum (1.0f), the last draw's largest weight, skipped indices, the add's ticket
        self.state = torch.tensor([0x3F800000, 0, 0, 0], dtype=torch.int32, device=self.device)

    def _stream(self):
        import torch
        try:
            return torch._C._cuda_getCurrentRawStream(self.fill.device.index)
        except AttributeError:
            return torch.cuda.current_stream(self.device).cuda_stream

    def add(self, batch):
        """``ReplayBuffer.add`` with each row folded over its next ``n_step`` steps (never across an episode end or the end of the
        batch), in one launch, followed by the write of the running maximum priority to the new rows.  The batch's arrays must be
        on the buffer's device: float32, the flags bool or uint8 (others are converted by one torch op each)."""
        import torch
        from rsoccer_amd import _lib
        for key in ("obs", "actions", "reward", "terminated", "truncated", "next_obs"):
            if key not in batch:
                raise ValueError(f"batch lacks {key!r}")
        if batch.get("final_obs") is None:
            raise ValueError("batch lacks 'final_obs': collect it with return_final_obs=True")
        obs = batch["obs"]
        if obs.dim() != 3 or obs.shape[2] != self.obs_dim:
            raise ValueError(f"batch['obs'] must be [T, B, {self.obs_dim}], got {list(obs.shape)}")
        T, B = int(obs.shape[0]), int(obs.shape[1])
        n = T * B
        if n < 1:
            raise ValueError(f"the batch is empty: {list(obs.shape)}")
        if n > self.capacity:
            raise ValueError(f"the batch has {n} rows, the buffer holds {self.capacity}")
        want = {"obs": (T, B, self.obs_dim), "actions": (T, B, self.act_dim), "reward": (T, B), "terminated": (T, B), "truncated": (T, B),
                "final_obs": (T, B, self.obs_dim), "next_obs": (B, self.obs_dim)}
        arr = {}
        for key, shape in want.items():
            t = batch[key]
            if tuple(t.shape) != shape:
                raise ValueError(f"batch[{key!r}] must be {list(shape)}, got {list(t.shape)}")
            if t.device != self.fill.device:
                raise ValueError(f"batch[{key!r}] is on {t.device}, the buffer on {self.fill.device}")
            if key in ("terminated", "truncated"):
                t = t if t.dtype in (torch.bool, torch.uint8) else t.bool()
            elif t.dtype != torch.float32:
                raise ValueError(f"batch[{key!r}] must be torch.float32, got {t.dtype}")
            arr[key] = t.detach().contiguous()
        ptr = lambda t: t.data_ptr()   # noqa: E731  (a bool tensor is one byte per element, 0 or 1)
        b = _lib.ReplayBatch(*(ptr(arr[k]) for k in ("obs", "actions", "reward", "terminated", "truncated", "final_obs", "next_obs")), T, B)
        ring = _lib.ReplayRing(ptr(self.obs), ptr(self.actions), ptr(self.reward), ptr(self.next_obs), ptr(self.terminated), ptr(self.discount),
                               ptr(self.head), ptr(self.fill), self.state.data_ptr() + 4 * _lib.REPLAY_STATE.index("ticket"), self.capacity,
                               self.obs_dim, self.act_dim)
        with torch.cuda.device(self.device):
            stream = self._stream()
            _lib.replay_add_nstep(b, ring, self.n_step, self.gamma, stream)
            _lib.replay_set_priorities(ptr(self.tree), ptr(self.state), self.capacity, None, None, ptr(self.head), n, self.alpha, self.eps, stream)
        self._keep_add = arr   # alive until the launch has consumed them
        return n

    def sample(self, m, beta=0.4, seed=0, step=0):
        """``(rows, weights)``: ``m`` int32 row indices drawn in proportion to the priorities, one per stratum of the total, and
        their float32 importance weights ``(fill * p / total)^(-beta)`` over the largest of the minibatch: what ``dpg_gradient(rows=,
        weights=)`` takes.  Entry ``t`` depends on ``(seed, step, t)`` and the tree only.  ``step``: an int or an int64 device tensor
        ``[1]``; ``beta``: a float or a float32 device tensor ``[1]``; a tensor is read when the launch runs, so a replayed graph
        anneals ``beta`` and draws anew.  On an empty ring every index is -1 and every weight 0."""
        import math
        import torch
        from rsoccer_amd import _lib
        m = int(m)
        if m < 1 or m > 2 ** 31 - 1:
            raise ValueError(f"m must be in 1 .. 2^31 - 1, got {m}")
        step_ptr, step_v, beta_ptr, beta_v = None, 0, None, 0.0
        if isinstance(step, torch.Tensor):
            if step.dtype != torch.int64 or tuple(step.shape) != (1,) or step.device != self.fill.device:
                raise ValueError(f"step as a tensor must be int64 [1] on {self.fill.device}, got {step.dtype} {list(step.shape)} on {step.device}")
            step_ptr = step.data_ptr()
        else:
            step_v = int(step)
            if not -2 ** 63 <= step_v < 2 ** 63:
                raise ValueError(f"step must fit 64 bits, got {step}")
        if isinstance(beta, torch.Tensor):
            if beta.dtype != torch.float32 or tuple(beta.shape) != (1,) or beta.device != self.fill.device:
                raise ValueError(f"beta as a tensor must be float32 [1] on {self.fill.device}, got {beta.dtype} {list(beta.shape)} on {beta.device}")
            beta_ptr = beta.data_ptr()
        else:
            beta_v = float(beta)
            if not (math.isfinite(beta_v) and beta_v >= 0.0):
                raise ValueError(f"beta must be finite and >= 0, got {beta}")
        rows = torch.empty((m,), dtype=torch.int32, device=self.device)
        weights = torch.empty((m,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.replay_sample_prioritized(self.tree.data_ptr(), self.state.data_ptr(), self.capacity, 0, self.fill.data_ptr(), rows.data_ptr(),
                                           weights.data_ptr(), m, beta_v, beta_ptr, int(seed), step_v, step_ptr, self._stream())
        self._keep_sample = (step, beta)   # alive until the launches have consumed them
        return rows, weights

    def update_priorities(self, rows, td_error):
        """the priorities of ``rows`` ``[m]`` (int32, ``sample``'s) become ``(|td_error| + eps)^alpha`` (``td_error`` ``[m]`` float32:
        ``dpg_gradient(return_td_error=True)["td_error"]``).  An index outside the ring (-1 included) is skipped and counted in
        ``skipped()``; where a row occurs more than once its largest value wins."""
        import torch
        from rsoccer_amd import _lib
        for name, t, dtype in (("rows", rows, torch.int32), ("td_error", td_error, torch.float32)):
            if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.shape[0] < 1:
                raise ValueError(f"{name} must be a 1-D tensor with at least one entry, got {type(t).__name__} {tuple(getattr(t, 'shape', ()))}")
            if t.dtype != dtype:
                raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
            if t.device != self.fill.device:
                raise ValueError(f"{name} is on {t.device}, the buffer on {self.fill.device}")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
        if rows.shape != td_error.shape:
            raise ValueError(f"rows and td_error must have one shape, got {list(rows.shape)} and {list(td_error.shape)}")
        with torch.cuda.device(self.device):
            _lib.replay_set_priorities(self.tree.data_ptr(), self.state.data_ptr(), self.capacity, rows.data_ptr(), td_error.data_ptr(), None,
                                       int(rows.shape[0]), self.alpha, self.eps, self._stream())
        self._keep_update = (rows, td_error)

    def data(self):
        """``ReplayBuffer.data()`` and ``"discount"`` ``[capacity]``: with that key ``dpg_gradient`` / ``sac_gradient`` discount each
        row's bootstrap by the row's own ``gamma^m``"""
        return {**super().data(), "discount": self.discount}

    def priorities(self):
        """the leaves ``[capacity]``, ``priority^alpha`` per row (0 behind the fill count): a view, for inspection"""
        return self.tree[:self.capacity]

    def max_priority(self):
        """the running maximum leaf value as a 0-d float32 view"""
        import torch
        return self.state.view(torch.float32)[0]

    def skipped(self):
        """how many entries ``update_priorities`` skipped for their index so far, as a 0-d int32 view"""
        return self.state[2]
