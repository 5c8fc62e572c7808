"""Self-play PPO on VSS-v0: the learner (blue 0) against a frozen earlier copy of itself (yellow 0), both evaluated inside one launch.

    python examples/selfplay_vss.py [--envs 1024] [--steps 128] [--updates 20] [--snapshot 5] [--graph] [--team]

The --device-update loop of examples/ppo_vss.py with one change: env.collect(..., opponent=pol, opponent_params=p_opponent) drives
yellow robot 0 by a second copy of the policy, which sees the mirrored observation (team colours swapped, the field turned by 180
degrees) and acts deterministically.  Every --snapshot N updates the learner's parameters are copied into the opponent's: ONE copy_
between two device tensors, stream-ordered like everything else in the loop.  p_opponent keeps its address, so with --graph the copy
needs no re-capture: the captured collect + ppo_update reads whatever the tensor holds when it is replayed.  The other four robots keep
their Ornstein-Uhlenbeck noise.  With --team the whole team learns against a snapshot team: collect(..., team=True, opponent_team=True)
seats all three robots of each side (every seat sees its side's row with "own" slots 0 and i exchanged and shares its side's
parameters), and rsoccer_amd.vec.policy.seat_rows turns the [T, B, S, ...] batch into the [T, B * S, ...] rows ppo_update takes: three
samples per env step, one shared reward.  A demonstration of the call pattern, not a tuned trainer."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rsoccer_amd.vec import VecVSSEnv
from rsoccer_amd.vec.optim import PPOOptimizer
from rsoccer_amd.vec.policy import MLPCritic, MLPPolicy, seat_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=128, help="T: steps per env and update")
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--snapshot", type=int, default=5, help="copy the learner into the opponent every N updates")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.95)
    ap.add_argument("--clip", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--graph", action="store_true", help="capture collect + ppo_update once, replay it per iteration")
    ap.add_argument("--max-grad-norm", type=float, default=0.5, help="the global-norm clip (<= 0: none)")
    ap.add_argument("--target-kl", type=float, default=None, help="stop an update's steps once approx_kl exceeds this")
    ap.add_argument("--team", action="store_true", help="seat every robot of both sides: the team learns against a snapshot team")
    args = ap.parse_args()
    if args.snapshot < 1:
        ap.error("--snapshot must be >= 1")

    torch.manual_seed(args.seed)
    env = VecVSSEnv(args.envs, device=0, seed=args.seed)
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    pol = MLPPolicy(OD, AD, hidden=64, layers=2, hidden_act="tanh", out_act="clip")
    val = MLPCritic(OD, hidden=64, layers=2, hidden_act="tanh")
    actor = torch.nn.Sequential(torch.nn.Linear(OD, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, AD))
    critic = torch.nn.Sequential(torch.nn.Linear(OD, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1))
    p_actor, p_critic = pol.from_module(actor).to(dev), val.from_module(critic).to(dev)
    p_opponent = p_actor.clone()   # the frozen copy: the same shape here, though the engine lets the two differ
    log_std = torch.full((AD,), -0.5, device=dev)
    opt = PPOOptimizer(pol, val, device=dev, lr=args.lr, max_grad_norm=args.max_grad_norm)
    env.reset()
    if args.graph:
        env.enable_graph_capture()

    def iteration():
        batch = env.collect(pol, p_actor, args.steps, log_std=log_std, noise_seed=args.seed + 1, critic=val, critic_params=p_critic,
                            gamma=args.gamma, lam=args.lam, opponent=pol, opponent_params=p_opponent, team=args.team,
                            opponent_team=args.team)
        if args.team:   # every (env, seat) pair becomes a column: [T, B * S, ...], reward and flags shared by an env's seats
            batch = seat_rows(batch)
        out = env.ppo_update(batch, pol, p_actor, log_std, val, p_critic, opt, epochs=args.epochs, minibatches=args.minibatches,
                             clip=args.clip, vf_coef=0.5, target_kl=args.target_kl, seed=args.seed)
        return batch["reward"].mean(), out["stats"]

    graph = None
    for update in range(args.updates):
        t0 = time.perf_counter()
        if update and update % args.snapshot == 0:
            p_opponent.copy_(p_actor)   # one device copy; the captured graph reads the tensor it was captured with
        if args.graph and update == 1:   # (iteration 0 ran eagerly: torch's warm-up before a capture)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                reward, stats = iteration()
        if graph is not None:
            graph.replay()
        else:
            reward, stats = iteration()
        torch.cuda.synchronize()
        m = env.metrics()
        print(f"update {update}: mean reward / step {float(reward):+.5f}, episodes {m['episodes']}, goals for / against "
              f"{m['goals_for']} / {m['goals_against']}, sigma {log_std.exp().mean().item():.3f}, learner - opponent "
              f"{(p_actor - p_opponent).norm().item():.4f}, steps applied {int(stats[:, :, 9].sum())} / {stats.shape[0] * stats.shape[1]}; "
              f"{(time.perf_counter() - t0) * 1e3:.1f} ms{' (one graph replay)' if graph is not None else ''}")
    env.close()


if __name__ == "__main__":
    main()
