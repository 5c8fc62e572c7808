"""TD3 / DDPG on VSS-v0 with the rollouts collected in one launch and the gradients of a replayed minibatch computed by the engine.

    python examples/td3_vss.py [--envs 256] [--steps 16] [--updates 10] [--grad-steps 8] [--batch 256] [--ddpg] [--torch]
                               [--device-update] [--graph] [--per [--alpha A --beta B]] [--n-step N]

One update: env.collect(...) advances the envs `steps` steps under the current actor with Gaussian exploration noise of standard
deviation --exploration (the engine clips the noisy sample: that is the executed action), ReplayBuffer.add() stores the T * B transitions
with their true successors, and `grad-steps` gradient steps follow.  A gradient step: ReplayBuffer.sample_rows() draws the minibatch on
the device, env.dpg_gradient(...) returns the gradients of the critic loss and — every --policy-delay-th step — of the actor loss in
four launches, torch's Adam steps on the flat parameter vectors (the leaves), and lerp_ moves the targets.  --ddpg: one critic, no
target smoothing, no delay.  --torch runs the same update with torch modules and autograd instead (torch_losses below: what
tools/bench_dpg_grad.py times the engine against).  --device-update replaces the whole gradient-step loop by ONE call, env.dpg_update
with a DPGOptimizer (rows from the engine's generator, Adam and the Polyak step on the device); --graph captures collect + add +
dpg_update once and replays them (device_update below).  --per and --n-step N keep the transitions in a PrioritizedReplayBuffer and
run the piecewise loop on the device (per_loop below): buf.sample, env.dpg_gradient(weights=..., return_td_error=True), opt.step,
buf.update_priorities; with --graph that loop is captured once, with collect and buf.add.  The fused phase (--device-update) does not
take priorities or per-row discounts yet.  A demonstration of the call pattern, not a tuned trainer."""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rsoccer_amd.vec import VecVSSEnv
from rsoccer_amd.vec.policy import MLPPolicy, MLPQCritic
from rsoccer_amd.vec.replay import PrioritizedReplayBuffer, ReplayBuffer


def mlp(n_in, n_out, out_tanh):
    mods = [torch.nn.Linear(n_in, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, n_out)]
    return torch.nn.Sequential(*(mods + [torch.nn.Tanh()] if out_tanh else mods))


def torch_losses(actor, critics, target_actor, target_critics, data, idx, gamma, sigma, noise_clip, with_actor):
    """the update's two losses on torch modules and their two backward() calls; the gradients land in the modules' .grad"""
    obs, act, nxt = data["obs"][idx], data["actions"][idx], data["next_obs"][idx]
    with torch.no_grad():
        a = target_actor(nxt)
        if sigma > 0.0:
            a = (a + (sigma * torch.randn_like(a)).clamp(-noise_clip, noise_clip)).clamp(-1.0, 1.0)
        xa = torch.cat([nxt, a], -1)
        q = target_critics[0](xa).squeeze(-1)
        for c in target_critics[1:]:
            q = torch.minimum(q, c(xa).squeeze(-1))
        r = data["reward"][idx]
        y = torch.where(data["terminated"][idx], r, r + gamma * q)
    xa = torch.cat([obs, act], -1)
    loss_q = sum(0.5 * (c(xa).squeeze(-1) - y).pow(2).mean() for c in critics)
    for c in critics:
        for p in c.parameters():
            p.grad = None
    loss_q.backward()
    loss_pi = None
    if with_actor:
        for p in actor.parameters():
            p.grad = None
        loss_pi = -critics[0](torch.cat([obs, actor(obs)], -1)).mean()
        loss_pi.backward(inputs=list(actor.parameters()))
    return loss_q, loss_pi


def device_update(args, C, sigma, delay):
    """--device-update: the loop body is collect, buf.add, env.dpg_update — rows drawn by the engine's generator, Adam and the Polyak
    step on the device, no interpreter between the gradient steps.  --graph: those three calls captured once on a device-keyed env
    and replayed; the optimiser's step count on the device keys every replay's rows and noise."""
    from rsoccer_amd.vec.optim import DPGOptimizer
    if args.grad_steps % delay:
        raise SystemExit(f"--grad-steps ({args.grad_steps}) must be a multiple of --policy-delay ({delay})")
    torch.manual_seed(args.seed)
    env = VecVSSEnv(args.envs, device=0, seed=args.seed)
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    pol = MLPPolicy(OD, AD, hidden=64, layers=2, hidden_act="tanh", out_act="tanh")
    qnet = MLPQCritic(OD, AD, hidden=64, layers=2, hidden_act="tanh")
    p_actor = pol.from_module(mlp(OD, AD, True)).to(dev)
    p_critics = torch.stack([qnet.from_module(mlp(OD + AD, 1, False)) for _ in range(C)]).to(dev)
    t_actor, t_critics = p_actor.clone(), p_critics.clone()
    opt = DPGOptimizer(pol, qnet, C, device=dev, lr_actor=args.lr, lr_critic=args.lr, tau=args.tau)
    buf = ReplayBuffer(args.capacity, OD, AD, dev)
    log_std = torch.full((AD,), math.log(args.exploration), device=dev)
    env.reset()
    if args.graph:
        env.enable_graph_capture()

    def iteration():
        batch = env.collect(pol, p_actor, args.steps, log_std=log_std, noise_seed=args.seed + 2, return_final_obs=True)
        buf.add(batch)
        out = env.dpg_update(buf, pol, p_actor, t_actor, qnet, p_critics, t_critics, opt, grad_steps=args.grad_steps, batch_size=args.batch,
                             policy_delay=delay, gamma=args.gamma, target_noise=sigma, noise_clip=args.noise_clip, seed=args.seed + 1)
        return batch["reward"].mean(), out["stats"]

    graph = None
    for update in range(args.updates):
        t0 = time.perf_counter()
        if graph is not None:
            graph.replay()
        else:
            reward, stats = iteration()   # (eager; with --graph also the warm-up before the capture)
        torch.cuda.synchronize()
        m, last = env.metrics(), stats[-1]
        print(f"update {update}: mean reward / step {float(reward):+.5f}, episodes {m['episodes']}, goals for / against "
              f"{m['goals_for']} / {m['goals_against']}, buffer {int(buf.fill)} rows, gradient steps {int(opt.steps)}, loss_q "
              f"{float(last[0] + last[1]):.5f}, loss_pi {float(last[4]):+.5f}; collect + add + {args.grad_steps} gradient steps "
              f"{(time.perf_counter() - t0) * 1e3:.1f} ms")
        if args.graph and graph is None:   # captured once (a capture records, it runs nothing): every further update is one replay
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                reward, stats = iteration()
    env.close()


def per_loop(args, C, sigma, delay):
    """--per / --n-step: prioritised and n-step replay, every piece on the device.  Without --per the priorities play no part
    (alpha = 0 makes every leaf 1, beta = 0 every weight 1) and only the n-step fold and its per-row discounts remain.  --graph: one
    whole update captured once on a device-keyed env and replayed; the optimiser's step count on the device keys every draw."""
    from rsoccer_amd.vec.optim import DPGOptimizer
    if args.grad_steps % delay:
        raise SystemExit(f"--grad-steps ({args.grad_steps}) must be a multiple of --policy-delay ({delay})")
    torch.manual_seed(args.seed)
    env = VecVSSEnv(args.envs, device=0, seed=args.seed)
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    pol = MLPPolicy(OD, AD, hidden=64, layers=2, hidden_act="tanh", out_act="tanh")
    qnet = MLPQCritic(OD, AD, hidden=64, layers=2, hidden_act="tanh")
    p_actor = pol.from_module(mlp(OD, AD, True)).to(dev)
    p_critics = torch.stack([qnet.from_module(mlp(OD + AD, 1, False)) for _ in range(C)]).to(dev)
    t_actor, t_critics = p_actor.clone(), p_critics.clone()
    opt = DPGOptimizer(pol, qnet, C, device=dev, lr_actor=args.lr, lr_critic=args.lr, tau=args.tau)
    buf = PrioritizedReplayBuffer(args.capacity, OD, AD, dev, alpha=args.alpha if args.per else 0.0, n_step=args.n_step, gamma=args.gamma)
    beta = args.beta if args.per else 0.0
    log_std = torch.full((AD,), math.log(args.exploration), device=dev)
    env.reset()
    if args.graph:
        env.enable_graph_capture()

    def iteration():
        batch = env.collect(pol, p_actor, args.steps, log_std=log_std, noise_seed=args.seed + 2, return_final_obs=True)
        buf.add(batch)
        data = buf.data()   # carries "discount": the targets use each row's own gamma^m
        for j in range(args.grad_steps):
            with_actor = (j + 1) % delay == 0
            rows, weights = buf.sample(args.batch, beta=beta, seed=args.seed + 1, step=opt.steps)
            out = env.dpg_gradient(data, pol, p_actor, t_actor, qnet, p_critics, t_critics, rows=rows, gamma=args.gamma, target_noise=sigma,
                                   noise_clip=args.noise_clip, noise_seed=args.seed + 1, noise_step=opt.steps, actor=with_actor,
                                   weights=weights, return_td_error=True)
            opt.step(p_actor, t_actor, p_critics, t_critics, out["grad_params"] if with_actor else None, out["grad_critic_params"])
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
              f"{float(stats['loss_q0'] + stats['loss_q1']):.5f}, largest priority {float(buf.max_priority()):.4f}, smallest weight "
              f"{float(weights.min()):.4f}; collect + add + {args.grad_steps} gradient steps {(time.perf_counter() - t0) * 1e3:.1f} ms")
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
    ap.add_argument("--exploration", type=float, default=0.1, help="standard deviation of the collector's noise")
    ap.add_argument("--target-noise", type=float, default=0.2)
    ap.add_argument("--noise-clip", type=float, default=0.5)
    ap.add_argument("--policy-delay", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ddpg", action="store_true", help="one critic, no target smoothing, no delay")
    ap.add_argument("--torch", action="store_true", help="the same update in torch autograd")
    ap.add_argument("--device-update", action="store_true", help="the whole update phase in one call: env.dpg_update with a DPGOptimizer")
    ap.add_argument("--graph", action="store_true", help="--device-update with collect + add + dpg_update captured once and replayed")
    ap.add_argument("--per", action="store_true", help="prioritised replay: the piecewise loop on the device (per_loop)")
    ap.add_argument("--alpha", type=float, default=0.6, help="--per: the priorities' exponent")
    ap.add_argument("--beta", type=float, default=0.4, help="--per: the importance weights' exponent")
    ap.add_argument("--n-step", type=int, default=1, help="n-step transitions (1 .. 16); above 1 the piecewise loop on the device")
    args = ap.parse_args()
    C, sigma, delay = (1, 0.0, 1) if args.ddpg else (2, args.target_noise, args.policy_delay)
    if args.per or args.n_step != 1:
        if args.device_update:
            ap.error("--per and --n-step are not available with --device-update: the fused update phase does not take priorities or per-row "
                     "discounts yet; leave --device-update out (--graph still captures the whole piecewise iteration)")
        if args.torch:
            ap.error("--per / --n-step and --torch exclude each other")
        return per_loop(args, C, sigma, delay)
    if args.device_update or args.graph:
        if args.torch:
            ap.error("--device-update / --graph and --torch exclude each other")
        return device_update(args, C, sigma, delay)

    torch.manual_seed(args.seed)
    env = VecVSSEnv(args.envs, device=0, seed=args.seed)
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    pol = MLPPolicy(OD, AD, hidden=64, layers=2, hidden_act="tanh", out_act="tanh")
    qnet = MLPQCritic(OD, AD, hidden=64, layers=2, hidden_act="tanh")
    actor = mlp(OD, AD, True).to(dev)
    critics = [mlp(OD + AD, 1, False).to(dev) for _ in range(C)]
    if args.torch:
        target_actor, target_critics = mlp(OD, AD, True).to(dev), [mlp(OD + AD, 1, False).to(dev) for _ in range(C)]
        for t, m in zip([target_actor] + target_critics, [actor] + critics):
            t.load_state_dict(m.state_dict())
        opt_a = torch.optim.Adam(actor.parameters(), lr=args.lr)
        opt_c = torch.optim.Adam([p for c in critics for p in c.parameters()], lr=args.lr)
    else:   # the flat vectors are the leaves: the engine reads and differentiates them as they are
        p_actor = torch.nn.Parameter(pol.from_module(actor).to(dev))
        p_critics = torch.nn.Parameter(torch.stack([qnet.from_module(c) for c in critics]).to(dev))
        t_actor, t_critics = p_actor.detach().clone(), p_critics.detach().clone()
        opt_a, opt_c = torch.optim.Adam([p_actor], lr=args.lr), torch.optim.Adam([p_critics], lr=args.lr)
    buf = ReplayBuffer(args.capacity, OD, AD, dev)
    log_std = torch.full((AD,), math.log(args.exploration), device=dev)
    env.reset()
    step = 0
    for update in range(args.updates):
        t0 = time.perf_counter()
        with torch.no_grad():
            batch = env.collect(pol, pol.from_module(actor).to(dev) if args.torch else p_actor.detach(), args.steps, log_std=log_std,
                                iteration=update, return_final_obs=True)
            buf.add(batch)
        data = buf.data()
        torch.cuda.synchronize()
        t_collect = time.perf_counter() - t0
        for _ in range(args.grad_steps):
            rows = buf.sample_rows(args.batch)
            with_actor = step % delay == 0
            if args.torch:
                loss_q, l_pi = torch_losses(actor, critics, target_actor, target_critics, data, rows.long(), args.gamma, sigma,
                                            args.noise_clip, with_actor)
                loss_q = loss_q.detach()
                opt_c.step()
                if with_actor:
                    loss_pi = l_pi.detach()
                    opt_a.step()
                    with torch.no_grad():
                        for t, m in zip([target_actor] + target_critics, [actor] + critics):
                            for pt, pm in zip(t.parameters(), m.parameters()):
                                pt.lerp_(pm, args.tau)
            else:
                out = env.dpg_gradient(data, pol, p_actor, t_actor, qnet, p_critics, t_critics, rows=rows, gamma=args.gamma,
                                       target_noise=sigma, noise_clip=args.noise_clip, noise_seed=args.seed + 1, noise_step=step,
                                       actor=with_actor)
                p_critics.grad = out["grad_critic_params"]
                opt_c.step()
                loss_q = out["stats"]["loss_q0"] + out["stats"]["loss_q1"]
                if with_actor:
                    p_actor.grad, loss_pi = out["grad_params"], out["stats"]["loss_pi"]
                    opt_a.step()
                    with torch.no_grad():
                        t_actor.lerp_(p_actor, args.tau)
                        t_critics.lerp_(p_critics, args.tau)
            step += 1
        torch.cuda.synchronize()
        m = env.metrics()
        print(f"update {update}: mean reward / step {float(batch['reward'].mean()):+.5f}, episodes {m['episodes']}, goals for / against "
              f"{m['goals_for']} / {m['goals_against']}, buffer {int(buf.fill)} rows, loss_q {float(loss_q):.5f}, loss_pi {float(loss_pi):+.5f}; "
              f"collect + add {t_collect * 1e3:.1f} ms, {args.grad_steps} gradient steps {((time.perf_counter() - t0) - t_collect) * 1e3:.1f} ms")
    env.close()


if __name__ == "__main__":
    main()
