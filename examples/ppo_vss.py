"""PPO on VSS-v0 with every rollout collected in one launch.

    python examples/ppo_vss.py [--envs 1024] [--steps 128] [--updates 10] [--epochs 4] [--minibatches 4] [--lr 3e-4]
                               [--fused-update | --device-update [--graph]] [--target-kl 0.02]

One update: env.collect(...) advances the envs `steps` steps under the current actor — the MLP evaluated inside the engine's launch, a
Gaussian head on top, episode ends handled in the launch — and, given the critic, evaluates it on the recorded observations and runs
the GAE recurrence in two more launches (env.advantages: a terminated row bootstraps from 0, a truncated one from the value of its
terminal observation), returning the [T, B] batch with `value`, `advantage` and `return`; a few epochs of clipped PPO follow in torch.
The actor's and the critic's weights reach the engine as flat vectors (MLPPolicy / MLPCritic.from_module: torch's own layout).  The
density PPO compares is the pre-activation one: log N(sample; mean, exp(log_std)), where the action fed to the env is clip(sample) —
the trainer evaluates the same expression on the recorded `sample`, so the ratio is exact.  With --fused-update the loss and its
gradients come from the engine as well (env.ppo_gradient: three launches per minibatch): the leaves are the flat parameter vectors, the
call's outputs become their .grad, and Adam steps on three tensors.  With --device-update the whole inner loop is ONE call
(env.ppo_update: advantage normalisation, a keyed permutation per epoch, the gradients, the global-norm clip and Adam per minibatch, all
stream-ordered with the optimiser's state and counters on the device); --graph captures collect + ppo_update once on a device-keyed
env and replays it: one replay is one PPO iteration.  A demonstration of the call pattern, not a tuned trainer."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rsoccer_amd.vec import VecVSSEnv
from rsoccer_amd.vec.policy import MLPCritic, MLPPolicy


def log_prob(mean, log_std, sample):
    z = (sample - mean) / log_std.exp()
    return (-0.5 * z * z - log_std - 0.9189385332046727).sum(-1)


def device_update(args):
    """the loop with the update phase on the device; with --graph one replay per iteration"""
    from rsoccer_amd.vec.optim import PPOOptimizer
    torch.manual_seed(args.seed)
    env = VecVSSEnv(args.envs, device=0, seed=args.seed)
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    pol = MLPPolicy(OD, AD, hidden=64, layers=2, hidden_act="tanh", out_act="clip")
    val = MLPCritic(OD, hidden=64, layers=2, hidden_act="tanh")
    actor = torch.nn.Sequential(torch.nn.Linear(OD, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, AD))
    critic = torch.nn.Sequential(torch.nn.Linear(OD, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1))
    # plain tensors, updated in place by the engine: no autograd anywhere in this loop
    p_actor, p_critic = pol.from_module(actor).to(dev), val.from_module(critic).to(dev)
    log_std = torch.full((AD,), -0.5, device=dev)
    opt = PPOOptimizer(pol, val, device=dev, lr=args.lr, max_grad_norm=args.max_grad_norm)
    env.reset()
    if args.graph:
        env.enable_graph_capture()   # the step counter moves to the device: collect() draws fresh noise on every replay

    def iteration():
        # (noise_seed fixed: the draws are keyed by the step counter, which advances; the permutations by opt's update count)
        batch = env.collect(pol, p_actor, args.steps, log_std=log_std, noise_seed=args.seed + 1, critic=val, critic_params=p_critic,
                            gamma=args.gamma, lam=args.lam)
        out = env.ppo_update(batch, pol, p_actor, log_std, val, p_critic, opt, epochs=args.epochs, minibatches=args.minibatches,
                             clip=args.clip, vf_coef=0.5, target_kl=args.target_kl, seed=args.seed)
        return batch["reward"].mean(), out["stats"]

    graph = None
    for update in range(args.updates):
        t0 = time.perf_counter()
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
        last = stats[-1, -1]
        print(f"update {update}: mean reward / step {float(reward):+.5f}, episodes {m['episodes']}, goals for / against "
              f"{m['goals_for']} / {m['goals_against']}, sigma {log_std.exp().mean().item():.3f}, loss_pi {float(last[0]):+.5f}, "
              f"loss_v {float(last[1]):.5f}, steps applied {int(stats[:, :, 9].sum())} / {stats.shape[0] * stats.shape[1]}; "
              f"collect + advantages + update {(time.perf_counter() - t0) * 1e3:.1f} ms{' (one graph replay)' if graph is not None else ''}")
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=128, help="T: steps per env and update")
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.95)
    ap.add_argument("--clip", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fused-update", action="store_true", help="loss and gradients of a minibatch from env.ppo_gradient instead of torch")
    ap.add_argument("--device-update", action="store_true", help="the whole update phase in one call: env.ppo_update with a PPOOptimizer")
    ap.add_argument("--graph", action="store_true", help="with --device-update: capture collect + ppo_update once, replay it per iteration")
    ap.add_argument("--max-grad-norm", type=float, default=0.5, help="--device-update: the global-norm clip (<= 0: none)")
    ap.add_argument("--target-kl", type=float, default=None, help="--device-update: stop an update's steps once approx_kl exceeds this")
    args = ap.parse_args()
    if args.graph and not args.device_update:
        ap.error("--graph needs --device-update")
    if args.device_update:
        return device_update(args)

    torch.manual_seed(args.seed)
    env = VecVSSEnv(args.envs, device=0, seed=args.seed)
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    pol = MLPPolicy(OD, AD, hidden=64, layers=2, hidden_act="tanh", out_act="clip")
    val = MLPCritic(OD, hidden=64, layers=2, hidden_act="tanh")
    # the actor WITHOUT its output activation: the engine applies the clip to the noisy sample, the trainer needs the mean
    actor = torch.nn.Sequential(torch.nn.Linear(OD, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, AD)).to(dev)
    critic = torch.nn.Sequential(torch.nn.Linear(OD, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1)).to(dev)
    log_std = torch.nn.Parameter(torch.full((AD,), -0.5, device=dev))
    if args.fused_update:   # the flat vectors are the leaves: the engine reads and differentiates them as they are
        p_actor = torch.nn.Parameter(pol.from_module(actor).to(dev))
        p_critic = torch.nn.Parameter(val.from_module(critic).to(dev))
        opt = torch.optim.Adam([p_actor, p_critic, log_std], lr=args.lr)
    else:
        opt = torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()) + [log_std], lr=args.lr)
    T, B = args.steps, args.envs
    env.reset()
    for update in range(args.updates):
        t0 = time.perf_counter()
        batch = env.collect(pol, p_actor if args.fused_update else pol.from_module(actor), T, log_std=log_std, iteration=update,
                            critic=val, critic_params=p_critic if args.fused_update else val.from_module(critic),
                            gamma=args.gamma, lam=args.lam)
        ret, adv = batch["return"], batch["advantage"]
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        torch.cuda.synchronize()
        t_collect = time.perf_counter() - t0
        flat = {k: batch[k].reshape(T * B, -1) for k in ("obs", "sample")}
        old_lp, adv_f, ret_f = batch["log_prob"].reshape(-1), adv.reshape(-1), ret.reshape(-1)
        for _ in range(args.epochs):
            for idx in torch.randperm(T * B, device=dev).chunk(args.minibatches):
                if args.fused_update:
                    out = env.ppo_gradient(batch, pol, p_actor, log_std, val, p_critic, rows=idx, advantage=adv, clip=args.clip, vf_coef=0.5)
                    p_actor.grad, p_critic.grad, log_std.grad = out["grad_params"], out["grad_critic_params"], out["grad_log_std"]
                    opt.step()
                    loss_pi, loss_v = out["stats"]["loss_pi"], out["stats"]["loss_v"]
                    continue
                lp = log_prob(actor(flat["obs"][idx]), log_std, flat["sample"][idx])
                ratio = (lp - old_lp[idx]).exp()
                loss_pi = -torch.min(ratio * adv_f[idx], ratio.clamp(1 - args.clip, 1 + args.clip) * adv_f[idx]).mean()
                loss_v = 0.5 * (critic(flat["obs"][idx]).squeeze(-1) - ret_f[idx]).pow(2).mean()
                opt.zero_grad(set_to_none=True)
                (loss_pi + 0.5 * loss_v).backward()
                opt.step()
        torch.cuda.synchronize()
        m = env.metrics()
        print(f"update {update}: mean reward / step {float(batch['reward'].mean()):+.5f}, episodes {m['episodes']}, goals for / against "
              f"{m['goals_for']} / {m['goals_against']}, sigma {log_std.exp().mean().item():.3f}, loss_pi {float(loss_pi):+.5f}, "
              f"loss_v {float(loss_v):.5f}; collect + advantages "
              f"{t_collect * 1e3:.1f} ms, update {((time.perf_counter() - t0) - t_collect) * 1e3:.1f} ms")
    env.close()


if __name__ == "__main__":
    main()
