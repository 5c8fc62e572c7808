"""Self-play PPO on VSS-v0: the learner (blue 0) against a frozen earlier copy of itself (yellow 0), both evaluated inside one launch.

    python examples/selfplay_vss.py [--envs 1024] [--steps 128] [--updates 20] [--snapshot 5] [--graph] [--team] [--league M]

The --device-update loop of examples/ppo_vss.py with one change: env.collect(..., opponent=pol, opponent_params=p_opponent) drives
yellow robot 0 by a second copy of the policy, which sees the mirrored observation (team colours swapped, the field turned by 180
degrees) and acts deterministically.  Every --snapshot N updates the learner's parameters are copied into the opponent's: ONE copy_
between two device tensors, stream-ordered like everything else in the loop.  p_opponent keeps its address, so with --graph the copy
needs no re-capture: the captured collect + ppo_update reads whatever the tensor holds when it is replayed.  The other four robots keep
their Ornstein-Uhlenbeck noise.  With --team the whole team learns against a snapshot team: collect(..., team=True, opponent_team=True)
seats all three robots of each side (every seat sees its side's row with "own" slots 0 and i exchanged and shares its side's
parameters), and rsoccer_amd.vec.policy.seat_rows turns the [T, B, S, ...] batch into the [T, B * S, ...] rows ppo_update takes: three
samples per env step, one shared reward.  With --league M the last M snapshots are kept in ONE [M, P] device tensor, a ring written by
copy_.  At every snapshot the learner plays whole episodes against all of them in one env.lookahead_match on a forked evaluation env
straight after its reset() — the same start states and the same draws for every opponent, nothing committed — the win / draw / loss row
is printed (rsoccer_amd.vec.policy.match_table), and the next opponent is drawn from that row: the more the learner loses or draws against
a snapshot, the likelier it trains against it.  A demonstration of the call pattern, not a tuned trainer."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rsoccer_amd.vec import VecVSSEnv
from rsoccer_amd.vec.optim import PPOOptimizer
from rsoccer_amd.vec.policy import MLPCritic, MLPPolicy, match_table, seat_rows


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
    ap.add_argument("--league", type=int, default=0, metavar="M", help="keep the last M snapshots, score the learner against all of them "
                    "at every snapshot (one lookahead_match) and draw the next opponent from the result")
    ap.add_argument("--eval-envs", type=int, default=256, help="envs of the forked evaluation env (--league)")
    args = ap.parse_args()
    if args.snapshot < 1:
        ap.error("--snapshot must be >= 1")
    if args.league < 0 or args.eval_envs < 1:
        ap.error("--league must be >= 0 and --eval-envs >= 1")

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
    if args.league:
        ring = p_actor.clone().unsqueeze(0).repeat(args.league, 1)   # [M, P]: the last M snapshots, slot `snapshots % M` is written next
        snapshots = 1                                                # (slot 0 holds the initial copy)
        evaluation = env.fork(args.eval_envs, seed=args.seed + 1000)
        pick = torch.Generator().manual_seed(args.seed)
    if args.graph:
        env.enable_graph_capture()

    def league_round():
        """the learner against every kept snapshot from the same start states -> the slot of the next opponent"""
        evaluation.reset()
        kept = min(snapshots, args.league)
        out = evaluation.lookahead_match(pol, p_actor.unsqueeze(0), pol, ring[:kept], evaluation.max_episode_steps, team=args.team,
                                         opponent_team=args.team)
        table = {k: v[0].cpu() for k, v in match_table(out).items()}   # the learner's row: [kept]
        print("  league: " + ", ".join(f"slot {m}: {int(table['wins'][m])} / {int(table['draws'][m])} / {int(table['losses'][m])} "
                                        f"(mean return {float(table['mean_return'][m]):+.2f})" for m in range(kept)) + "  (win / draw / loss)")
        weight = (table["losses"] + 0.5 * table["draws"] + 1.0).double()   # never zero: every snapshot keeps a chance
        return int(torch.multinomial(weight / weight.sum(), 1, generator=pick))

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
            if args.league:
                ring[snapshots % args.league].copy_(p_actor)
                snapshots += 1
                p_opponent.copy_(ring[league_round()])
            else:
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
    if args.league:
        evaluation.close()
    env.close()


if __name__ == "__main__":
    main()
