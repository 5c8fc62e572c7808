"""Evolution strategies on VSS-v0 with whole episodes scored in one launch per generation.

    python examples/es_vss.py [--envs 256] [--pairs 32] [--generations 5] [--sigma 0.05] [--lr 0.01] [--horizon N] [--opponent]

One generation: reset() gives every env a fresh start state; lookahead_policy(..., horizon=max_episode_steps) then runs the 2 * pairs
perturbed policies theta +- sigma * eps closed-loop from exactly those states against exactly the same future draws (the other robots'
OU noise is keyed by env and step, not by who asks): common random numbers for free, so the antithetic difference of two returns is
the policy's doing.  Fitness = mean return over the envs; the update is the plain antithetic ES estimator on rank-centred fitness.
The env is never stepped: a generation is two engine launches (reset, lookahead_policy) and a handful of torch ops.  With --opponent
the population is scored against a frozen opponent instead of Ornstein-Uhlenbeck noise: yellow robot 0 plays the initial theta from the
mirrored observation, in the same single launch (lookahead_match with K = population, M = 1)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rsoccer_amd.vec import VecVSSEnv
from rsoccer_amd.vec.policy import MLPPolicy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--pairs", type=int, default=32, help="antithetic pairs per generation (population = 2 * pairs)")
    ap.add_argument("--generations", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--horizon", type=int, default=None, help="steps per evaluation (default: max_episode_steps, whole episodes)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--opponent", action="store_true", help="score the population against a frozen opponent (the initial theta on yellow 0)")
    args = ap.parse_args()

    env = VecVSSEnv(args.envs, device=0, seed=args.seed)
    pol = MLPPolicy(env.sim.obs_dim, env.sim.act_dim, hidden=64, layers=2)
    H = args.horizon or env.max_episode_steps
    gen = torch.Generator(device=env.device).manual_seed(args.seed)
    theta = torch.nn.utils.parameters_to_vector(torch.nn.Sequential(
        torch.nn.Linear(pol.obs_dim, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
        torch.nn.Linear(64, pol.act_dim), torch.nn.Tanh()).parameters()).detach().to(env.device)   # torch's own layout
    frozen = theta.clone().unsqueeze(0)   # [1, P]: the opponent of --opponent
    n = args.pairs
    for g in range(args.generations):
        t0 = time.perf_counter()
        eps = torch.randn(n, pol.num_params, device=env.device, generator=gen)
        params = torch.cat([theta + args.sigma * eps, theta - args.sigma * eps, theta[None]])   # the last row: theta itself
        env.reset()
        if args.opponent:   # the same launch shape with yellow 0 under the frozen policy: [B, 2 n + 1, 1]
            out = env.lookahead_match(pol, params, pol, frozen, H)
            wins = int((out["result"][:, -1, 0] > 0).sum())
        else:
            out = env.lookahead_policy(pol, params, H)
        fitness = out["return"].reshape(args.envs, -1).mean(dim=0)   # [2 n + 1]: mean return over the envs
        ranks = fitness[:2 * n].argsort().argsort().float() / (2 * n - 1) - 0.5
        theta = theta + args.lr / (n * args.sigma) * ((ranks[:n] - ranks[n:]) @ eps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        steps = int(out["steps"].sum())
        versus = f" ({wins} of {args.envs} episodes won against the frozen opponent)" if args.opponent else ""
        print(f"generation {g}: fitness of theta {float(fitness[-1]):+.3f}{versus}, population mean {float(fitness[:2 * n].mean()):+.3f} "
              f"best {float(fitness[:2 * n].max()):+.3f}; {steps} env-steps in {dt * 1e3:.1f} ms ({steps / dt / 1e6:.1f} M env-steps/s)")
    env.close()


if __name__ == "__main__":
    main()
