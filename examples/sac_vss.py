"""Soft actor-critic on VSS-v0 with the rollouts collected in one launch under the actor itself.

    python examples/sac_vss.py [--envs 256] [--steps 16] [--updates 10] [--grad-steps 8] [--batch 256] [--torch]
                               [--device-update] [--graph] [--per [--alpha A --beta B]] [--n-step N]

One update: env.collect(MLPGaussianPolicy, ...) advances the envs `steps` steps under the current actor — mean and log-std per state,
the sample squashed by tanh, all inside the launch (rsx_task_collect_gaussian) — ReplayBuffer.add() stores the T * B transitions with
their true successors, and `grad-steps` gradient steps follow.  A gradient step: ReplayBuffer.sample_rows() draws the minibatch on the
device, env.sac_gradient(...) returns the gradients of the critic loss, the actor loss and the temperature loss in six launches
(rsx_task_sac_gradient), three torch Adam optimisers step on the flat tensors (the leaves), and lerp_ moves the target critics.
--torch runs the same losses in torch autograd instead (sac_losses below, on the same flat vectors: MLPGaussianPolicy.sample and
MLPQCritic.forward are plain torch; what tools/bench_sac_grad.py times the engine against).  --device-update replaces the whole
gradient-step loop by ONE call, env.sac_update with a SACOptimizer (rows from the engine's generator, the three Adam steps and the Polyak
step on the device); --graph captures collect + add + sac_update once and replays them (device_update below).  --per and --n-step N keep
the transitions in a PrioritizedReplayBuffer and run the piecewise loop on the device (per_loop below): buf.sample,
env.sac_gradient(weights=..., return_td_error=True), opt.step, buf.update_priorities; with --graph that loop is captured once, with
collect and buf.add.  The fused phase (--device-update) does not take priorities or per-row discounts yet.  A demonstration of the
call pattern, not a tuned trainer."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rsoccer_amd.vec import VecVSSEnv
from rsoccer_amd.vec.policy import MLPGaussianPolicy, MLPQCritic
from rsoccer_amd.vec.replay import PrioritizedReplayBuffer, ReplayBuffer


def mlp(n_in, n_out):
    return torch.nn.Sequential(torch.nn.Linear(n_in, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, n_out))


def sac_losses(pol, p_actor, qnet, p_critics, t_critics, log_alpha, data, idx, gamma, target_entropy):
    """(loss_q, loss_pi, loss_alpha, mean log_prob) on the flat parameters, float32; eps drawn by torch"""
    f32 = torch.float32
    obs, act, nxt = data["obs"][idx], data["actions"][idx], data["next_obs"][idx]
    alpha = log_alpha.detach().exp()
    q_all = lambda params, o, a: torch.stack([qnet.forward(o, a, p, dtype=f32).squeeze(-1) for p in params])   # noqa: E731  [C, M]
    with torch.no_grad():
        a2, logp2, _ = pol.sample(nxt, p_actor, torch.randn_like(act), dtype=f32)
        r = data["reward"][idx]
        y = torch.where(data["terminated"][idx], r, r + gamma * (q_all(t_critics, nxt, a2).min(0).values - alpha * logp2))
    loss_q = (0.5 * (q_all(p_critics, obs, act) - y).pow(2).mean(-1)).sum()
    a, logp, _ = pol.sample(obs, p_actor, torch.randn_like(act), dtype=f32)
    loss_pi = (alpha * logp - q_all(p_critics.detach(), obs, a).min(0).values).mean()
    loss_alpha = -(log_alpha * (logp.detach() + target_entropy).mean()).sum()
    return loss_q, loss_pi, loss_alpha, logp.detach().mean()


def device_update(args):
    """--device-update: the loop body is collect, buf.add, env.sac_update — rows drawn by the engine's generator, Adam on the three
    groups and the Polyak step on the device, no interpreter between the gradient steps.  --graph: those three calls captured once on a
    device-keyed env and replayed; the optimiser's step count on the device keys every replay's rows and noise."""
    from rsoccer_amd.vec.optim import SACOptimizer
    torch.manual_seed(args.seed)
    env = VecVSSEnv(args.envs, device=0, seed=args.seed)
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    pol = MLPGaussianPolicy(OD, AD, hidden=64, layers=2, hidden_act="tanh")
    qnet = MLPQCritic(OD, AD, hidden=64, layers=2, hidden_act="tanh")
    p_actor = pol.from_module(mlp(OD, 2 * AD)).to(dev)   # plain tensors: nothing here is differentiated by autograd
    p_critics = torch.stack([qnet.from_module(mlp(OD + AD, 1)) for _ in range(2)]).to(dev)
    t_critics, log_alpha = p_critics.clone(), torch.zeros(1, device=dev)
    opt = SACOptimizer(pol, qnet, 2, device=dev, lr_actor=args.lr, lr_critic=args.lr, lr_alpha=args.lr, tau=args.tau)
    buf = ReplayBuffer(args.capacity, OD, AD, dev)
    env.reset()
    if args.graph:
        env.enable_graph_capture()

    def iteration():
        batch = env.collect(pol, p_actor, args.steps, noise_seed=args.seed + 2, return_final_obs=True)
        buf.add(batch)
        out = env.sac_update(buf, pol, p_actor, qnet, p_critics, t_critics, log_alpha, opt, grad_steps=args.grad_steps, batch_size=args.batch,
                             gamma=args.gamma, seed=args.seed + 1)
        return batch["reward"].mean(), out["stats"]

    graph = None
    for update in range(args.updates):
        t0 = time.perf_counter()
        if graph is not None:
            graph.replay()
        else:
            reward, stats = iteration()   # (eager; with --graph also the warm-up before the capture)
        torch.cuda.synchronize()
        m = env.metrics()
        print(f"update {update}: mean reward / step {float(reward):+.5f}, episodes {m['episodes']}, goals for / against "
              f"{m['goals_for']} / {m['goals_against']}, buffer {int(buf.fill)} rows, gradient steps {int(opt.steps)}, loss_q "
              f"{float(stats['loss_q0'][-1] + stats['loss_q1'][-1]):.5f}, loss_pi {float(stats['loss_pi'][-1]):+.5f}, alpha "
              f"{float(log_alpha.exp()):.4f}, log_prob {float(stats['log_prob'][-1]):+.3f}; collect + add + {args.grad_steps} gradient steps "
              f"{(time.perf_counter() - t0) * 1e3:.1f} ms")
        if args.graph and graph is None:   # captured once (a capture records, it runs nothing): every further update is one replay
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                reward, stats = iteration()
    env.close()


def per_loop(args):
    """--per / --n-step: prioritised and n-step replay, every piece on the device.  Without --per the priorities play no part
    (alpha = 0 makes every leaf 1, beta = 0 every weight 1) and only the n-step fold and its per-row discounts remain.  --graph: one
    whole update captured once on a device-keyed env and replayed; the optimiser's step count on the device keys every draw."""
    from rsoccer_amd.vec.optim import SACOptimizer
    torch.manual_seed(args.seed)
    env = VecVSSEnv(args.envs, device=0, seed=args.seed)
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    pol = MLPGaussianPolicy(OD, AD, hidden=64, layers=2, hidden_act="tanh")
    qnet = MLPQCritic(OD, AD, hidden=64, layers=2, hidden_act="tanh")
    p_actor = pol.from_module(mlp(OD, 2 * AD)).to(dev)
    p_critics = torch.stack([qnet.from_module(mlp(OD + AD, 1)) for _ in range(2)]).to(dev)
    t_critics, log_alpha = p_critics.clone(), torch.zeros(1, device=dev)
    opt = SACOptimizer(pol, qnet, 2, device=dev, lr_actor=args.lr, lr_critic=args.lr, lr_alpha=args.lr, tau=args.tau)
    buf = PrioritizedReplayBuffer(args.capacity, OD, AD, dev, alpha=args.alpha if args.per else 0.0, n_step=args.n_step, gamma=args.gamma)
    beta = args.beta if args.per else 0.0
    env.reset()
    if args.graph:
        env.enable_graph_capture()

    def iteration():
        batch = env.collect(pol, p_actor, args.steps, noise_seed=args.seed + 2, return_final_obs=True)
        buf.add(batch)
        data = buf.data()   # carries "discount": the targets use each row's own gamma^m
        for _ in range(args.grad_steps):
            rows, weights = buf.sample(args.batch, beta=beta, seed=args.seed + 1, step=opt.steps)
            out = env.sac_gradient(data, pol, p_actor, qnet, p_critics, t_critics, log_alpha, rows=rows, gamma=args.gamma,
                                   noise_seed=args.seed + 1, noise_step=opt.steps, weights=weights, return_td_error=True)
            opt.step(p_actor, p_critics, t_critics, log_alpha, out["grad_params"], out["grad_critic_params"], out["grad_log_alpha"])
            buf.update_priorities(rows, out["td_error"])
        return batch["reward"].mean(), out["stats"], weights

    graph = None
    for update in range(args.updates):
        t0 = time.perf_counter()
        if graph is not None:
            graph.replay()
        else:
            reward, stats, weights = iteration()   # (eager; with --graph also the warm-up before the capture)
        torch.cuda.synchronize()
        m = env.metrics()
        print(f"update {update}: mean reward / step {float(reward):+.5f}, episodes {m['episodes']}, goals for / against "
              f"{m['goals_for']} / {m['goals_against']}, buffer {int(buf.fill)} rows, gradient steps {int(opt.steps)}, loss_q "
              f"{float(stats['loss_q0'] + stats['loss_q1']):.5f}, alpha {float(log_alpha.exp()):.4f}, largest priority "
              f"{float(buf.max_priority()):.4f}, smallest weight {float(weights.min()):.4f}; collect + add + {args.grad_steps} gradient steps "
              f"{(time.perf_counter() - t0) * 1e3:.1f} ms")
        if args.graph and graph is None:   # captured once (a capture records, it runs nothing): every further update is one replay
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                reward, stats, weights = iteration()
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=16, help="T: steps per env and update")
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--grad-steps", type=int, default=8, help="gradient steps per update")
    ap.add_argument("--batch", type=int, default=256, help="rows of a minibatch")
    ap.add_argument("--capacity", type=int, default=1 << 18)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--tau", type=float, default=0.005)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--torch", action="store_true", help="the same losses in torch autograd")
    ap.add_argument("--device-update", action="store_true", help="the whole update phase in one call: env.sac_update with a SACOptimizer")
    ap.add_argument("--graph", action="store_true", help="--device-update with collect + add + sac_update captured once and replayed")
    ap.add_argument("--per", action="store_true", help="prioritised replay: the piecewise loop on the device (per_loop)")
    ap.add_argument("--alpha", type=float, default=0.6, help="--per: the priorities' exponent")
    ap.add_argument("--beta", type=float, default=0.4, help="--per: the importance weights' exponent")
    ap.add_argument("--n-step", type=int, default=1, help="n-step transitions (1 .. 16); above 1 the piecewise loop on the device")
    args = ap.parse_args()
    if args.per or args.n_step != 1:
        if args.device_update:
            ap.error("--per and --n-step are not available with --device-update: the fused update phase does not take priorities or per-row "
                     "discounts yet; leave --device-update out (--graph still captures the whole piecewise iteration)")
        if args.torch:
            ap.error("--per / --n-step and --torch exclude each other")
        return per_loop(args)
    if args.device_update or args.graph:
        if args.torch:
            ap.error("--device-update / --graph and --torch exclude each other")
        return device_update(args)

    torch.manual_seed(args.seed)
    env = VecVSSEnv(args.envs, device=0, seed=args.seed)
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    pol = MLPGaussianPolicy(OD, AD, hidden=64, layers=2, hidden_act="tanh")
    qnet = MLPQCritic(OD, AD, hidden=64, layers=2, hidden_act="tanh")
    # the flat vectors are the leaves: the engine reads them as they are, autograd differentiates them as they are
    p_actor = torch.nn.Parameter(pol.from_module(mlp(OD, 2 * AD)).to(dev))
    p_critics = torch.nn.Parameter(torch.stack([qnet.from_module(mlp(OD + AD, 1)) for _ in range(2)]).to(dev))
    log_alpha = torch.nn.Parameter(torch.zeros(1, device=dev))
    t_critics = p_critics.detach().clone()
    opt_a, opt_c, opt_t = (torch.optim.Adam([p], lr=args.lr) for p in (p_actor, p_critics, log_alpha))
    buf = ReplayBuffer(args.capacity, OD, AD, dev)
    env.reset()
    step = 0
    for update in range(args.updates):
        t0 = time.perf_counter()
        with torch.no_grad():
            batch = env.collect(pol, p_actor.detach(), args.steps, iteration=update, return_final_obs=True)
            buf.add(batch)
        data = buf.data()
        torch.cuda.synchronize()
        t_collect = time.perf_counter() - t0
        for _ in range(args.grad_steps):
            rows = buf.sample_rows(args.batch)
            if args.torch:
                loss_q, loss_pi, loss_alpha, logp = sac_losses(pol, p_actor, qnet, p_critics, t_critics, log_alpha, data, rows.long(), args.gamma,
                                                               -float(AD))
                for opt in (opt_c, opt_a, opt_t):
                    opt.zero_grad(set_to_none=True)
                for loss in (loss_q, loss_pi, loss_alpha):   # (every backward() before the first step: loss_pi reads the critics' values)
                    loss.backward()
                for opt in (opt_c, opt_a, opt_t):
                    opt.step()
            else:
                out = env.sac_gradient(data, pol, p_actor, qnet, p_critics, t_critics, log_alpha, rows=rows, gamma=args.gamma,
                                       noise_seed=args.seed + 1, noise_step=step)
                p_actor.grad, p_critics.grad, log_alpha.grad = out["grad_params"], out["grad_critic_params"], out["grad_log_alpha"]
                for opt in (opt_c, opt_a, opt_t):
                    opt.step()
                st = out["stats"]
                loss_q, loss_pi, loss_alpha, logp = st["loss_q0"] + st["loss_q1"], st["loss_pi"], st["loss_alpha"], st["log_prob"]
            with torch.no_grad():
                t_critics.lerp_(p_critics, args.tau)
            step += 1
        torch.cuda.synchronize()
        m = env.metrics()
        print(f"update {update}: mean reward / step {float(batch['reward'].mean()):+.5f}, collected log_prob {float(batch['log_prob'].mean()):+.3f}, "
              f"mean log_std {float(batch['log_std'].mean()):+.3f}, episodes {m['episodes']}, goals for / against {m['goals_for']} / "
              f"{m['goals_against']}, buffer {int(buf.fill)} rows, loss_q {float(loss_q.detach()):.5f}, loss_pi {float(loss_pi.detach()):+.5f}, alpha "
              f"{float(log_alpha.detach().exp()):.4f}, log_prob {float(logp):+.3f}; collect + add {t_collect * 1e3:.1f} ms, {args.grad_steps} gradient "
              f"steps {((time.perf_counter() - t0) - t_collect) * 1e3:.1f} ms")
    env.close()


if __name__ == "__main__":
    main()
