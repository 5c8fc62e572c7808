#!/usr/bin/env python
"""Time of one PPO update phase — advantage normalisation, `--epochs` x `--minibatches` minibatches of gradients, clip and Adam — as
ONE call (env.ppo_update -> rsx_task_ppo_update, rsoccer_amd/csrc/rsx_ppo_update.hip) next to the loops it replaces.

Needs a GPU and fails without one.  VSS-v0, T = `--steps` steps per batch, a 40-64-64-2 tanh actor and a 40-64-64-1 tanh critic, at each
of `--envs` batch sizes one batch collected (with advantages) up front and reused by every leg.  In one run per size:
  (a) env.ppo_update:       the whole phase enqueued by one call (global-norm clip at 0.5 included, which (c) and (d) do not do);
  (b) the same, graph:      that call captured once and replayed;
  (c) --fused-update loop:  examples/ppo_vss.py --fused-update as it was before ppo_update existed — adv.mean() / adv.std(),
                            torch.randperm(T * B).chunk(minibatches), env.ppo_gradient, three .grad assignments, torch.optim.Adam.step();
  (d) the all-torch loop:   the same example without --fused-update (torch modules, loss, backward(), Adam).
Device events around each window, a warm-up first, `--rounds` interleaved rounds of at least `--window` seconds; medians and spread.
The opponent of (a) is (c).

    python tools/bench_ppo_update.py [--out profiles/r18_ppo_update.txt]
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
from bench_ppo_grad import _log_prob  # noqa: E402

CLIP, VF, LR = 0.2, 0.5, 3e-4


def _size(torch, n, args):
    from rsoccer_amd.vec import VecVSSEnv
    from rsoccer_amd.vec.optim import PPOOptimizer
    from rsoccer_amd.vec.policy import MLPCritic, MLPPolicy
    T, E, MB = args.steps, args.epochs, args.minibatches
    env = VecVSSEnv(n, device=0, seed=1)
    env.reset()
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    pol, val = MLPPolicy(OD, AD, out_act="clip"), MLPCritic(OD)
    torch.manual_seed(0)
    mk = lambda out: torch.nn.Sequential(torch.nn.Linear(OD, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),  # noqa: E731
                                         torch.nn.Linear(64, out)).to(dev)
    actor, critic = mk(AD), mk(1)
    log_std = torch.nn.Parameter(torch.full((AD,), -0.5, device=dev))
    p0, c0 = pol.from_module(actor).to(dev), val.from_module(critic).to(dev)
    with torch.no_grad():
        batch = env.collect(pol, p0, T, log_std=log_std, critic=val, critic_params=c0)
    N = T * n

    # (a), (b): plain tensors updated in place
    pa, la, ca = p0.clone(), log_std.detach().clone(), c0.clone()
    opt_a = PPOOptimizer(pol, val, device=dev, lr=LR, max_grad_norm=0.5)
    leg_a = lambda: env.ppo_update(batch, pol, pa, la, val, ca, opt_a, epochs=E, minibatches=MB, clip=CLIP, vf_coef=VF, seed=1)  # noqa: E731
    pb, lb, cb = p0.clone(), log_std.detach().clone(), c0.clone()
    opt_b = PPOOptimizer(pol, val, device=dev, lr=LR, max_grad_norm=0.5)
    leg_b_eager = lambda: env.ppo_update(batch, pol, pb, lb, val, cb, opt_b, epochs=E, minibatches=MB, clip=CLIP, vf_coef=VF, seed=1)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        leg_b_eager()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graph.keep = leg_b_eager()

    # (c): the flat vectors are the leaves, as in examples/ppo_vss.py --fused-update
    pc, cc, lc = torch.nn.Parameter(p0.clone()), torch.nn.Parameter(c0.clone()), torch.nn.Parameter(log_std.detach().clone())
    opt_c = torch.optim.Adam([pc, cc, lc], lr=LR)

    def leg_c():
        adv = batch["advantage"]
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        for _ in range(E):
            for idx in torch.randperm(N, device=dev).chunk(MB):
                out = env.ppo_gradient(batch, pol, pc, lc, val, cc, rows=idx, advantage=adv, clip=CLIP, vf_coef=VF)
                pc.grad, cc.grad, lc.grad = out["grad_params"], out["grad_critic_params"], out["grad_log_std"]
                opt_c.step()

    # (d): torch modules
    opt_d = torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()) + [log_std], lr=LR)
    flat = {"obs": batch["obs"].reshape(N, OD), "sample": batch["sample"].reshape(N, AD)}
    old_lp, ret_f = batch["log_prob"].reshape(-1), batch["return"].reshape(-1)

    def leg_d():
        adv = batch["advantage"]
        adv_f = ((adv - adv.mean()) / (adv.std() + 1e-8)).reshape(-1)
        for _ in range(E):
            for idx in torch.randperm(N, device=dev).chunk(MB):
                lp = _log_prob(actor(flat["obs"][idx]), log_std, flat["sample"][idx])
                ratio = (lp - old_lp[idx]).exp()
                loss_pi = -torch.min(ratio * adv_f[idx], ratio.clamp(1 - CLIP, 1 + CLIP) * adv_f[idx]).mean()
                loss_v = 0.5 * (critic(flat["obs"][idx]).squeeze(-1) - ret_f[idx]).pow(2).mean()
                opt_d.zero_grad(set_to_none=True)
                (loss_pi + VF * loss_v).backward()
                opt_d.step()

    legs = [("(a) env.ppo_update", leg_a), ("(b) the same, graph replay", graph.replay), ("(c) --fused-update loop (parent)", leg_c),
            ("(d) all-torch loop", leg_d)]
    reps = [_reps(torch, fn, args.window) for _, fn in legs]
    times = [[] for _ in legs]
    for _ in range(args.rounds):
        for i, (_, fn) in enumerate(legs):
            times[i].append(_window(torch, fn, reps[i]))
    torch.cuda.synchronize()
    finite = all(bool(torch.isfinite(t).all()) for t in (pa, la, ca, pb, lb, cb))
    env.close()
    return legs, times, finite


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ppo_update.py needs a GPU")
    lines = [f"# tools/bench_ppo_update.py: {torch.cuda.get_device_name(0)}, VSS-v0, T = {args.steps}, {args.epochs} epochs x {args.minibatches} "
             f"minibatches, 40-64-64-2 / -1 tanh, {args.rounds} interleaved rounds of >= {args.window} s, device events; unit: ms per update"]
    result = {}
    for n in args.envs:
        legs, times, finite = _size(torch, n, args)
        lines.append(f"## num_envs {n}: {args.steps * n} rows per batch, {-(-args.steps * n // args.minibatches)} per minibatch")
        lines.append("%-36s | %11s | %17s | %s" % ("leg", "ms / update", "spread (min-max)", "rounds (ms)"))
        rows = {}
        for (name, _), ts in zip(legs, times):
            m = statistics.median(ts)
            rows[name[:3]] = dict(ms=m * 1e3, rounds_ms=[x * 1e3 for x in ts])
            lines.append("%-36s | %11.3f | %7.3f - %7.3f | %s" % (name, m * 1e3, min(ts) * 1e3, max(ts) * 1e3, " ".join("%.3f" % (x * 1e3) for x in ts)))
        a, b, c, d = (rows[k] for k in ("(a)", "(b)", "(c)", "(d)"))
        overlap = lambda x, y: "yes" if max(x["rounds_ms"]) >= min(y["rounds_ms"]) else "no"   # noqa: E731
        lines.append("(c) / (a) = %.2f x (rounds overlap: %s), (c) / (b) = %.2f x (rounds overlap: %s), (d) / (a) = %.2f x; parameters finite "
                     "after the run: %s" % (c["ms"] / a["ms"], overlap(a, c), c["ms"] / b["ms"], overlap(b, c), d["ms"] / a["ms"], finite))
        result[str(n)] = rows
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"ppo_update_bench": result}))


if __name__ == "__main__":
    main()
