"""Evolution strategies on VSS-v0 with whole episodes scored in one launch per generation.

    python examples/es_vss.py [--envs 256] [--pairs 32] [--generations 5] [--sigma 0.05] [--lr 0.01] [--horizon N]

One generation: reset() gives every env a fresh start state; lookahead_policy(..., horizon=max_episode_steps) then runs the 2 * pairs
perturbed policies theta +- sigma * eps closed-loop from exactly those states against exactly the same future draws (the other robots'
OU noise is keyed by env and step, not by who asks): common random numbers for free, so the antithetic difference of two returns is
the policy's doing.  Fitness = mean return over the envs; the update is the plain antithetic ES estimator on rank-centred fitness.
The env is never stepped: a generation is two engine launches (reset, lookahead_policy) and a handful of torch ops."""
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
    args = ap.parse_args()

    env = VecVSSEnv(args.envs, device=0, seed=args.seed)
    pol = MLPPolicy(env.sim.obs_dim, env.sim.act_dim, hidden=64, layers=2)
    H = args.horizon or env.max_episode_steps
    gen = torch.Generator(device=env.device).manual_seed(args.seed)
    theta = torch.nn.utils.parameters_to_vector(torch.nn.Sequential(
        torch.nn.Linear(pol.obs_dim, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
        torch.nn.Linear(64, pol.act_dim), torch.nn.Tanh()).parameters()).detach().to(env.device)   # torch's own layout
    n = args.pairs
    for g in range(args.generations):
        t0 = time.perf_counter()
        eps = torch.randn(n, pol.num_params, device=env.device, generator=gen)
        params = torch.cat([theta + args.sigma * eps, theta - args.sigma * eps, theta[None]])   # the last row: theta itself
        env.reset()
        out = env.lookahead_policy(pol, params, H)
        fitness = out["return"].mean(dim=0)   # [2 n + 1]: mean return over the envs
        ranks = fitness[:2 * n].argsort().argsort().float() / (2 * n - 1) - 0.5
        theta = theta + args.lr / (n * args.sigma) * ((ranks[:n] - ranks[n:]) @ eps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        steps = int(out["steps"].sum())
        print(f"generation {g}: fitness of theta {float(fitness[-1]):+.3f}, population mean {float(fitness[:2 * n].mean()):+.3f} "
              f"best {float(fitness[:2 * n].max()):+.3f}; {steps} env-steps in {dt * 1e3:.1f} ms ({steps / dt / 1e6:.1f} M env-steps/s)")
    env.close()


if __name__ == "__main__":
    main()
