"""The MLP policies ``VecFusedEnv.lookahead_policy`` and ``collect`` evaluate inside their launches, and the critic of the same family
``VecFusedEnv.advantages`` evaluates on a collected batch (include/rsx.h: rsx_policy_mlp).

:class:`MLPPolicy` describes the SHAPE of a policy; its parameters are a flat float32 vector laid out like
``torch.nn.utils.parameters_to_vector`` of ``Sequential(Linear(obs_dim, hidden), act, [Linear(hidden, hidden), act,]
Linear(hidden, act_dim))``: ``W1 [hidden, obs_dim]`` row-major, ``b1``, (``W2``, ``b2``,) ``Wo [act_dim, hidden]``, ``bo``.  Many
parameter vectors of one shape — a population — form the ``[K, P]`` tensor the env call takes."""
import math

from rsoccer_amd import _lib

_HALF_LOG_2PI, _LOG_2 = 0.5 * math.log(2.0 * math.pi), math.log(2.0)
_HIDDEN_ACTS = {"relu": _lib.ACT_RELU, "tanh": _lib.ACT_TANH}
_OUT_ACTS = {"clip": _lib.ACT_CLIP, "tanh": _lib.ACT_TANH}


class MLPPolicy:
    """``obs_dim -> hidden [-> hidden] -> act_dim`` with ``layers`` in (1, 2) hidden layers of ``hidden`` in (32, 64) units,
    ``hidden_act`` in ("relu", "tanh") and ``out_act`` in ("clip", "tanh") — "clip" clamps to [-1, 1].  Anything else: ValueError."""

    def __init__(self, obs_dim, act_dim, hidden=64, layers=2, hidden_act="tanh", out_act="tanh"):
        self.obs_dim, self.act_dim, self.hidden, self.layers = int(obs_dim), int(act_dim), int(hidden), int(layers)
        if self.obs_dim < 1 or self.act_dim < 1:
            raise ValueError(f"obs_dim and act_dim must be >= 1, got {obs_dim}, {act_dim}")
        if self.hidden not in (32, 64):
            raise ValueError(f"hidden must be 32 or 64, got {hidden}")
        if self.layers not in (1, 2):
            raise ValueError(f"layers must be 1 or 2, got {layers}")
        if hidden_act not in _HIDDEN_ACTS:
            raise ValueError(f"hidden_act must be one of {sorted(_HIDDEN_ACTS)}, got {hidden_act!r}")
        if out_act not in _OUT_ACTS:
            raise ValueError(f"out_act must be one of {sorted(_OUT_ACTS)}, got {out_act!r}")
        self.hidden_act, self.out_act = hidden_act, out_act

    # ---- layout ----
    @property
    def shapes(self):
        """the tensors of one policy in layout order: [(out, in), (out,), ...]"""
        h = self.hidden
        dims = [(h, self.obs_dim)] + [(h, h)] * (self.layers - 1) + [(self.act_dim, h)]
        out = []
        for o, i in dims:
            out += [(o, i), (o,)]
        return out

    @property
    def num_params(self):
        n = 0
        for s in self.shapes:
            n += s[0] * (s[1] if len(s) == 2 else 1)
        return n

    def spec(self):
        """the rsx_policy_mlp of this shape"""
        return _lib.PolicyMLP(self.layers, self.hidden, _HIDDEN_ACTS[self.hidden_act], _OUT_ACTS[self.out_act])

    def pack(self, weights_and_biases):
        """``[W1, b1, (W2, b2,) Wo, bo]`` (tensors or arrays of the shapes above) -> the flat float32 vector ``[P]``"""
        import torch
        ts = [torch.as_tensor(t) for t in weights_and_biases]
        if [tuple(t.shape) for t in ts] != self.shapes:
            raise ValueError(f"expected tensors of shapes {self.shapes}, got {[tuple(t.shape) for t in ts]}")
        return torch.cat([t.detach().to(torch.float32).reshape(-1) for t in ts])

    def unpack(self, flat):
        """``[..., P]`` -> ``[W1, b1, (W2, b2,) Wo, bo]`` as views, leading dimensions kept (``[K, P]`` gives ``[K, out, in]`` ...)"""
        import torch
        flat = torch.as_tensor(flat)
        if flat.shape[-1] != self.num_params:
            raise ValueError(f"expected {self.num_params} parameters per policy, got {flat.shape[-1]}")
        out, at = [], 0
        for s in self.shapes:
            n = s[0] * (s[1] if len(s) == 2 else 1)
            out.append(flat[..., at:at + n].reshape(tuple(flat.shape[:-1]) + s))
            at += n
        return out

    def _torch_acts(self):
        import torch
        hid = torch.relu if self.hidden_act == "relu" else torch.tanh
        out = torch.tanh if self.out_act == "tanh" else (lambda v: v.clamp(-1.0, 1.0))
        return hid, out

    def from_module(self, module):
        """the flat parameters of a ``torch.nn.Sequential(Linear, act, Linear, ...)`` of this shape (its Linear layers in order)"""
        import torch
        lin = [m for m in module if isinstance(m, torch.nn.Linear)]
        ps = []
        for m in lin:
            if m.bias is None:
                raise ValueError("every Linear layer needs a bias")
            ps += [m.weight, m.bias]
        return self.pack(ps)

    def forward(self, obs, params, dtype=None):
        """The reference forward pass in torch: ``obs [..., obs_dim]``, ``params [P]`` (or ``[..., P]`` with leading dimensions that
        broadcast against obs's) -> actions ``[..., act_dim]`` in ``dtype`` (default float64).  For tests and for callers who run
        the same policy through ``step()``; the engine's own arithmetic is float32 in a fixed order (include/rsx.h)."""
        import torch
        dtype = torch.float64 if dtype is None else dtype
        x = torch.as_tensor(obs).to(dtype)
        ts = [t.to(dtype) for t in self.unpack(torch.as_tensor(params).to(x.device))]
        hid, out = self._torch_acts()
        n = len(ts) // 2
        for li in range(n):
            w, b = ts[2 * li], ts[2 * li + 1]
            x = (w @ x.unsqueeze(-1)).squeeze(-1) + b
            x = hid(x) if li + 1 < n else out(x)
        return x


class MLPCritic(MLPPolicy):
    """``obs_dim -> hidden [-> hidden] -> 1`` with a linear output: the critic ``VecFusedEnv.advantages`` evaluates
    (``rsx_task_advantages``).  ``MLPPolicy``'s layout with ``act_dim = 1``: the flat parameters equal
    ``parameters_to_vector`` of ``Sequential(Linear(obs_dim, hidden), act, [Linear(hidden, hidden), act,] Linear(hidden, 1))``.
    ``forward`` returns ``[..., 1]``, like the module."""

    def __init__(self, obs_dim, hidden=64, layers=2, hidden_act="tanh"):
        super().__init__(obs_dim, 1, hidden=hidden, layers=layers, hidden_act=hidden_act, out_act="tanh")   # (checks the shape)
        self.out_act = "none"

    def spec(self):
        """the rsx_policy_mlp of this shape, with out_act = RSX_ACT_NONE"""
        return _lib.PolicyMLP(self.layers, self.hidden, _HIDDEN_ACTS[self.hidden_act], _lib.ACT_NONE)

    def _torch_acts(self):
        hid, _ = super()._torch_acts()
        return hid, (lambda v: v)


class MLPQCritic(MLPPolicy):
    """``obs_dim + act_dim -> hidden [-> hidden] -> 1`` with a linear output: the action-value critic ``VecFusedEnv.dpg_gradient``
    differentiates (``rsx_task_dpg_gradient``).  ``MLPCritic``'s layout with input width ``obs_dim + act_dim``, the observation
    columns first: the flat parameters equal ``parameters_to_vector`` of ``Sequential(Linear(obs_dim + act_dim, hidden), act,
    [Linear(hidden, hidden), act,] Linear(hidden, 1))``.  Several critics of one shape (TD3's twins) form a ``[C, P]`` tensor."""

    def __init__(self, obs_dim, act_dim, hidden=64, layers=2, hidden_act="tanh"):
        if int(obs_dim) < 1 or int(act_dim) < 1:
            raise ValueError(f"obs_dim and act_dim must be >= 1, got {obs_dim}, {act_dim}")
        super().__init__(int(obs_dim) + int(act_dim), 1, hidden=hidden, layers=layers, hidden_act=hidden_act, out_act="tanh")
        self.out_act = "none"
        self.state_dim, self.action_dim = int(obs_dim), int(act_dim)   # (obs_dim is the input width, as the layout has it)

    def spec(self):
        """the rsx_policy_mlp of this shape, with out_act = RSX_ACT_NONE"""
        return _lib.PolicyMLP(self.layers, self.hidden, _HIDDEN_ACTS[self.hidden_act], _lib.ACT_NONE)

    def _torch_acts(self):
        hid, _ = super()._torch_acts()
        return hid, (lambda v: v)

    def forward(self, obs, action, params, dtype=None):
        """``Q(obs, action)``: ``obs [..., obs_dim]`` and ``action [..., act_dim]`` are concatenated along the last axis; returns
        ``[..., 1]``, like the module.  ``params [P]`` or ``[..., P]`` as for ``MLPPolicy.forward``."""
        import torch
        dtype = torch.float64 if dtype is None else dtype
        obs, action = torch.as_tensor(obs).to(dtype), torch.as_tensor(action).to(dtype)
        if obs.shape[-1] != self.state_dim or action.shape[-1] != self.action_dim:
            raise ValueError(f"expected obs [..., {self.state_dim}] and action [..., {self.action_dim}], got {list(obs.shape)} and {list(action.shape)}")
        return super().forward(torch.cat([obs, action.to(obs.device)], dim=-1), params, dtype=dtype)


class MLPGaussianPolicy(MLPPolicy):
    """``obs_dim -> hidden [-> hidden] -> 2 * act_dim``: soft actor-critic's actor, a state-dependent Gaussian squashed by tanh
    (``rsx_task_collect_gaussian``; include/rsx.h states the head).  ``MLPPolicy``'s layout with an output layer of ``2 * act_dim``
    units: rows ``[0, act_dim)`` of ``Wo`` / ``bo`` are the mean ``mu``, rows ``[act_dim, 2 * act_dim)`` the raw log-std, so the flat
    parameters equal ``parameters_to_vector`` of ``Sequential(Linear(obs_dim, hidden), act, [Linear(hidden, hidden), act,]
    Linear(hidden, 2 * act_dim))`` with ``mu, raw = out.chunk(2, -1)``.  ``log_std = clamp(raw, log_std_min, log_std_max)``,
    ``u = mu + exp(log_std) * eps``, ``action = tanh(u)``.  ``act_dim <= 8`` and finite bounds with ``log_std_min < log_std_max``;
    anything else: ValueError."""

    def __init__(self, obs_dim, act_dim, hidden=64, layers=2, hidden_act="tanh", log_std_min=-20.0, log_std_max=2.0):
        super().__init__(obs_dim, act_dim, hidden=hidden, layers=layers, hidden_act=hidden_act, out_act="tanh")   # (checks the shape)
        self.out_act = "none"
        if self.act_dim > 8:
            raise ValueError(f"act_dim must be <= 8, got {act_dim}")
        lo, hi = float(log_std_min), float(log_std_max)
        if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
            raise ValueError(f"log_std_min and log_std_max must be finite with log_std_min < log_std_max, got {log_std_min}, {log_std_max}")
        self.log_std_min, self.log_std_max = lo, hi

    @property
    def shapes(self):
        out = super().shapes
        out[-2:] = [(2 * self.act_dim, self.hidden), (2 * self.act_dim,)]
        return out

    def spec(self):
        """the rsx_policy_mlp of this shape, with out_act = RSX_ACT_NONE"""
        return _lib.PolicyMLP(self.layers, self.hidden, _HIDDEN_ACTS[self.hidden_act], _lib.ACT_NONE)

    def _torch_acts(self):
        hid, _ = super()._torch_acts()
        return hid, (lambda v: v)

    def forward(self, obs, params, dtype=None):
        """The reference forward pass in torch: ``(mu, log_std)``, each ``[..., act_dim]`` in ``dtype`` (default float64), the
        log-std clamped (``torch.clamp``: its gradient is 1 inside and at the bounds, 0 outside).  For tests."""
        mu, raw = super().forward(obs, params, dtype=dtype).chunk(2, -1)
        return mu, raw.clamp(self.log_std_min, self.log_std_max)

    def sample(self, obs, params, eps, dtype=None):
        """``(action, log_prob, u)`` for the standard normals ``eps [..., act_dim]`` by include/rsx.h's formulas, in torch:
        ``u = mu + exp(log_std) * eps``, ``action = tanh(u)`` and ``log_prob [...]`` with the tanh correction in its stable form
        ``2 (ln 2 - u - softplus(-2 u))``."""
        mu, ls = self.forward(obs, params, dtype=dtype)
        eps = eps.to(device=mu.device, dtype=mu.dtype)
        u = mu + ls.exp() * eps
        return u.tanh(), squashed_log_prob(eps, ls, u), u


def squashed_log_prob(eps, log_std, u):
    """``sum_k [-0.5 eps_k^2 - log_std_k - 0.5 ln(2 pi) - 2 (ln 2 - u_k - softplus(-2 u_k))]`` over the last axis, with
    ``softplus(z) = max(z, 0) + log1p(exp(-|z|))`` written out: the log-density of ``tanh(u)`` for ``u = mu + exp(log_std) * eps``."""
    z = -2.0 * u
    softplus = z.clamp(min=0.0) + (-z.abs()).exp().log1p()
    return (-0.5 * eps * eps - log_std - _HALF_LOG_2PI - 2.0 * (_LOG_2 - u - softplus)).sum(-1)


_SEAT_KEYS = ("obs", "actions", "mean", "sample", "log_prob", "final_obs", "value", "advantage", "return")


def seat_rows(batch, opponent=False):
    """A team batch of ``VecFusedEnv.collect(..., team=True)`` (or ``opponent_team=True``) as the ``[T, B * S, ...]`` mapping
    ``advantages()``, ``ppo_gradient()`` and ``ppo_update()`` accept: every (env, seat) pair becomes a column of its own, column
    ``e * S + s``.  The seat tensors ``[T, B, S, ...]`` (``obs``, ``actions``, ``mean``, ``sample``, ``log_prob``, ``final_obs`` and, if
    present, ``value``, ``advantage``, ``return``) are viewed as ``[T, B * S, ...]`` and ``next_obs`` ``[B, S, obs_dim]`` as
    ``[B * S, obs_dim]``; ``reward``, ``terminated`` and ``truncated`` ``[T, B]`` are expanded to ``[T, B * S]`` — the seats of an env
    share its reward and its episode ends.  Everything returned is contiguous.  ``opponent=True`` takes the ``opponent_*`` tensors
    instead (with the same shared reward and flags: negate the reward for a zero-sum learner)."""
    pre = "opponent_" if opponent else ""
    for key in (pre + "obs", pre + "next_obs", "reward", "terminated", "truncated"):
        if key not in batch:
            raise ValueError(f"batch lacks {key!r}")
    obs = batch[pre + "obs"]
    if obs.dim() != 4:
        raise ValueError(f"batch[{pre + 'obs'!r}] must be [T, B, S, obs_dim] (a team batch), got {list(obs.shape)}")
    T, B, S = int(obs.shape[0]), int(obs.shape[1]), int(obs.shape[2])
    out = {}
    for key in _SEAT_KEYS:
        t = batch.get(pre + key)
        if t is None:
            continue
        if tuple(t.shape[:3]) != (T, B, S):
            raise ValueError(f"batch[{pre + key!r}] must start with [{T}, {B}, {S}], got {list(t.shape)}")
        out[key] = t.reshape(T, B * S, *t.shape[3:]).contiguous()
    nxt = batch[pre + "next_obs"]
    if tuple(nxt.shape[:2]) != (B, S):
        raise ValueError(f"batch[{pre + 'next_obs'!r}] must start with [{B}, {S}], got {list(nxt.shape)}")
    out["next_obs"] = nxt.reshape(B * S, *nxt.shape[2:]).contiguous()
    for key in ("reward", "terminated", "truncated"):
        t = batch[key]
        if tuple(t.shape) != (T, B):
            raise ValueError(f"batch[{key!r}] must be [{T}, {B}], got {list(t.shape)}")
        out[key] = t.unsqueeze(-1).expand(T, B, S).reshape(T, B * S).contiguous()
    return out


def match_table(out):
    """The ``[K, M]`` table of a ``VecFusedEnv.lookahead_match()`` result, folded over the envs: ``wins`` (pairs that ended on a goal
    for the actor, ``result == 1``), ``losses`` (``result == -1``) and ``draws`` (everything else: time limit, horizon) as int64 counts
    that sum to ``B`` per cell, and ``mean_return`` float32.  Pure torch on the tensors' device; does not synchronise."""
    for key in ("result", "return"):
        if key not in out:
            raise ValueError(f"out lacks {key!r}")
    res, ret = out["result"], out["return"]
    if res.dim() != 3 or tuple(ret.shape) != tuple(res.shape):
        raise ValueError(f"out['result'] and out['return'] must be [B, K, M], got {list(res.shape)} and {list(ret.shape)}")
    wins, losses = (res > 0).sum(0), (res < 0).sum(0)
    return {"wins": wins, "draws": res.shape[0] - wins - losses, "losses": losses, "mean_return": ret.float().mean(0)}
