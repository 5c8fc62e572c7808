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
