#!/usr/bin/env python
"""Time of the PPO loss gradients of a minibatch in three launches (env.ppo_gradient -> rsx_task_ppo_gradient,
rsoccer_amd/csrc/rsx_ppo.hip) next to the torch path it replaces.

Needs a GPU and fails without one.  VSS-v0, `--envs` envs, T = `--steps` steps per batch, a 40-64-64-2 tanh actor and a 40-64-64-1 tanh
critic, one batch collected (with advantages) up front and reused by every leg; the minibatch is `--rows` rows of a fixed permutation.
In one run:
  (a) ppo_gradient:      env.ppo_gradient on the minibatch;
  (b) torch, eager:      examples/ppo_vss.py's loss on torch modules and backward(), the gather of the rows included;
  (c) torch, graph:      the same replayed from one graph — the fair opponent, launch overhead removed;
  (d) collect + advantages of such a batch, for scale.
Device events around each window, a warm-up first, `--rounds` interleaved rounds of at least `--window` seconds; medians and spread.
(a) is set against its floor: 6 FLOP per weight and row (forward, back-propagation, weight gradient; the first layer has no
back-propagation) at the fp32 vector peak (157.3 TFLOP/s).

    python tools/bench_ppo_grad.py [--out profiles/r15_ppo_grad.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_policy_lookahead import _reps, _window  # noqa: E402

PEAK_FP32 = 157.3e12
CLIP, VF = 0.2, 0.5


def _log_prob(mean, log_std, sample):
    z = (sample - mean) / log_std.exp()
    return (-0.5 * z * z - log_std - 0.9189385332046727).sum(-1)


def _torch_path(torch, actor, critic, log_std, flat, idx):
    """the minibatch loss of examples/ppo_vss.py and its backward(); the gradients land in the modules' .grad"""
    for p in list(actor.parameters()) + list(critic.parameters()) + [log_std]:
        p.grad = None
    obs = flat["obs"][idx]
    lp = _log_prob(actor(obs), log_std, flat["sample"][idx])
    ratio = (lp - flat["old_lp"][idx]).exp()
    adv = flat["adv"][idx]
    loss_pi = -torch.min(ratio * adv, ratio.clamp(1 - CLIP, 1 + CLIP) * adv).mean()
    loss_v = 0.5 * (critic(obs).squeeze(-1) - flat["ret"][idx]).pow(2).mean()
    (loss_pi + VF * loss_v).backward()
    return loss_pi, loss_v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--rows", type=int, default=131072, help="rows of the minibatch")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ppo_grad.py needs a GPU")
    from rsoccer_amd.vec import VecVSSEnv
    from rsoccer_amd.vec.policy import MLPCritic, MLPPolicy
    n, T, M = args.envs, args.steps, args.rows
    head = (f"# tools/bench_ppo_grad.py: {torch.cuda.get_device_name(0)}, VSS-v0, num_envs {n}, T = {T}, minibatch {M} rows, 40-64-64-2 / -1 tanh, "
            f"{args.rounds} interleaved rounds of >= {args.window} s, device events; unit: us per minibatch")
    env = VecVSSEnv(n, device=0, seed=1)
    env.reset()
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    pol, val = MLPPolicy(OD, AD, out_act="clip"), MLPCritic(OD)
    torch.manual_seed(0)
    mk = lambda out: torch.nn.Sequential(torch.nn.Linear(OD, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),  # noqa: E731
                                         torch.nn.Linear(64, out)).to(dev)
    actor, critic = mk(AD), mk(1)
    log_std = torch.nn.Parameter(torch.full((AD,), -0.5, device=dev))
    params, cparams = pol.from_module(actor).to(dev), val.from_module(critic).to(dev)
    with torch.no_grad():
        batch = env.collect(pol, params, T, log_std=log_std, critic=val, critic_params=cparams)
        # the update the gradient is taken at: a small step away from the collecting policy, so that some rows clip
        for p in list(actor.parameters()) + list(critic.parameters()):
            p.add_(0.02 * torch.randn_like(p))
        params, cparams = pol.from_module(actor).to(dev), val.from_module(critic).to(dev)
    idx = torch.randperm(T * n, device=dev)[:M]
    idx32 = idx.to(torch.int32)
    flat = {"obs": batch["obs"].reshape(T * n, OD), "sample": batch["sample"].reshape(T * n, AD), "old_lp": batch["log_prob"].reshape(-1),
            "adv": batch["advantage"].reshape(-1), "ret": batch["return"].reshape(-1)}
    ls = log_std.detach()
    fused = lambda: env.ppo_gradient(batch, pol, params, ls, val, cparams, rows=idx32, clip=CLIP, vf_coef=VF)  # noqa: E731
    torch.cuda.synchronize()

    # agreement first: the engine's gradients against torch's float32 autograd of the same loss
    out = fused()
    _torch_path(torch, actor, critic, log_std, flat, idx)
    want_a = torch.nn.utils.parameters_to_vector([p.grad for p in actor.parameters()])
    want_c = torch.nn.utils.parameters_to_vector([p.grad for p in critic.parameters()])
    dev_a = float((out["grad_params"] - want_a).abs().max() / want_a.abs().max())
    dev_c = float((out["grad_critic_params"] - want_c).abs().max() / want_c.abs().max())
    dev_l = float((out["grad_log_std"] - log_std.grad).abs().max() / log_std.grad.abs().max())
    clip_fraction = float(out["stats"]["clip_fraction"])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            _torch_path(torch, actor, critic, log_std, flat, idx)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = _torch_path(torch, actor, critic, log_std, flat, idx)
    graph.keep = keep

    def collect():
        with torch.no_grad():
            return env.collect(pol, params, T, log_std=ls, critic=val, critic_params=cparams)

    legs = [("(a) ppo_gradient", fused),
            ("(b) torch loss + backward(), eager", lambda: _torch_path(torch, actor, critic, log_std, flat, idx)),
            ("(c) the same, graph replay", graph.replay),
            ("(d) collect + advantages of the batch", collect)]
    reps = [_reps(torch, fn, args.window) for _, fn in legs]
    times = [[] for _ in legs]
    for _ in range(args.rounds):
        for i, (_, fn) in enumerate(legs):
            times[i].append(_window(torch, fn, reps[i]))
    lines = [head, "%-42s | %12s | %16s | %s" % ("leg", "us / minibatch", "spread (min-max)", "rounds (us)")]
    rows = {}
    for (name, _), ts in zip(legs, times):
        m = statistics.median(ts)
        rows[name.strip()] = dict(us=m * 1e6, rounds_us=[x * 1e6 for x in ts])
        lines.append("%-42s | %14.1f | %7.1f - %6.1f | %s" % (name, m * 1e6, min(ts) * 1e6, max(ts) * 1e6, " ".join("%.1f" % (x * 1e6) for x in ts)))
    flop_row = sum(2 * (OD * 64) * 2 + 2 * (64 * 64) * 3 + 2 * (64 * o) * 3 for o in (AD, 1))
    t = rows["(a) ppo_gradient"]["us"] * 1e-6
    floor = M * flop_row / PEAK_FP32
    lines.append("(a): %d rows x %d FLOP = %.2f GFLOP, floor %.1f us at the fp32 vector peak, measured %.1f us = %.1f %% of peak" %
                 (M, flop_row, M * flop_row * 1e-9, floor * 1e6, t * 1e6, 100.0 * floor / t))
    a_us, c_us, b_us = rows["(a) ppo_gradient"], rows["(c) the same, graph replay"], rows["(b) torch loss + backward(), eager"]
    lines.append("ppo_gradient against the graph replay of the torch path: %.2f x, against the eager path: %.2f x (medians); rounds overlap: %s" %
                 (c_us["us"] / a_us["us"], b_us["us"] / a_us["us"], "yes" if max(a_us["rounds_us"]) >= min(c_us["rounds_us"]) else "no"))
    lines.append("largest relative deviation from torch's float32 autograd: actor %.3g, critic %.3g, log_std %.3g; clip_fraction %.4f" %
                 (dev_a, dev_c, dev_l, clip_fraction))
    print("\n".join(lines), flush=True)
    env.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"ppo_grad_bench": rows}))


if __name__ == "__main__":
    main()
