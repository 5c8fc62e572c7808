#!/usr/bin/env python
"""Random-shooting model-predictive control on VecVSSEnv with the engine's exact lookahead, next to the random-action policy.

Every step the planner samples K action sequences of H steps per env, scores them from the envs' CURRENT state with
env.lookahead (one launch: the candidates meet the env's real future, OU noise of the other robots included), and executes the
first action of the best one.  No policy network, no learning: what it shows is that the task is playable on this physics.

    python examples/mppi_vss.py [--envs 256] [--steps 1200] [--K 64] [--H 10]

With --sampled the same loop goes through env.plan: the candidates are drawn on the device around a warm-started plan (normal noise
of --sigma, held for --hold steps), scored and folded into the next plan in two launches; no candidate tensor exists.  --temperature 0
keeps the best candidate (random shooting), > 0 takes the return-weighted mean (MPPI).

    python examples/mppi_vss.py --sampled [--sigma 0.5] [--temperature 0]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(torch, vec, args, plan):
    env = vec.VecVSSEnv(args.envs, device=0, seed=args.seed)
    env.reset()
    B, AD, dev = env.num_envs, env.sim.act_dim, env.device
    rows = torch.arange(B, device=dev)
    g = torch.Generator(device=dev).manual_seed(args.seed)
    mean = torch.zeros(B, args.H, AD, device=dev)
    for _ in range(args.steps):
        if plan and args.sampled:
            out = env.plan(mean=mean, K=args.K, sigma=args.sigma, hold=args.hold, temperature=args.temperature, gamma=args.gamma)
            action = out["action"]
            # warm start: the new plan shifted by the step about to be executed, its last step repeated
            mean = torch.cat([out["mean"][:, 1:], out["mean"][:, -1:]], dim=1)
        elif plan:
            cand = torch.rand(B, args.K, args.H, AD, device=dev, generator=g) * 2 - 1
            # hold each drawn action for `--hold` steps: smoother sequences reach further than white noise
            cand = cand[:, :, ::args.hold].repeat_interleave(args.hold, dim=2)[:, :, :args.H].contiguous()
            best = env.lookahead(cand, gamma=args.gamma)["return"].argmax(dim=1)
            action = cand[rows, best, 0]
        else:
            action = torch.rand(B, AD, device=dev, generator=g) * 2 - 1
        env.step(action)
    m = env.metrics()
    env.close()
    n = max(m["episodes"], 1)
    return dict(episodes=m["episodes"], mean_return=m["return_sum"] / n, goals_for=m["goals_for"] / n, goals_against=m["goals_against"] / n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--H", type=int, default=10)
    ap.add_argument("--hold", type=int, default=5)
    ap.add_argument("--gamma", type=float, default=0.98)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sampled", action="store_true", help="plan through env.plan: candidates drawn on the device, warm-started mean")
    ap.add_argument("--sigma", type=float, default=0.5, help="--sampled: standard deviation of the noise around the plan")
    ap.add_argument("--temperature", type=float, default=0.0, help="--sampled: 0 = keep the best candidate, > 0 = MPPI weights")
    args = ap.parse_args()
    import torch
    from rsoccer_amd import vec
    for name, plan in (("random actions", False), (f"{'sampled planning' if args.sampled else 'random shooting'} K={args.K} H={args.H}", True)):
        r = run(torch, vec, args, plan)
        print(f"{name:32s} episodes {r['episodes']:5d}  mean episode return {r['mean_return']:8.3f}  "
              f"goals for / episode {r['goals_for']:.3f}  against {r['goals_against']:.3f}")


if __name__ == "__main__":
    main()
