#!/usr/bin/env python
"""Time per gradient step of the TD3 update phase in one call (env.dpg_update -> rsx_task_dpg_update,
rsoccer_amd/csrc/rsx_dpg_update.hip) next to the loops it replaces.

Needs a GPU and fails without one.  VSS-v0 shapes: a 40-64-64-2 tanh actor and twin 42-64-64-1 tanh critics, their targets 0.02 away;
a ReplayBuffer of `--envs` x `--steps` rows filled by one collect(); an update of `--grad-steps` gradient steps with `--policy-delay`.
In one run, per minibatch size in `--rows`:
  (a) dpg_update:                 env.dpg_update, eager;
  (b) dpg_update, graph:          the same replayed from one graph;
  (c) example loop, eager:        examples/td3_vss.py's loop — ReplayBuffer.sample_rows, env.dpg_gradient, torch.optim.Adam on the flat
                                  vectors, lerp_ — with the interpreter deciding the actor steps;
  (d) example loop, graph:        that loop replayed from one graph with torch.optim.Adam(capturable=True);
  (e) all torch, graph:           sample_rows, the example's torch_losses (the gather, six forwards, two backward()), Adam
                                  (capturable=True) on the modules and lerp_, replayed from one graph.
Every leg trains its own copy of the networks.  Device events around each window, a warm-up first, `--rounds` interleaved rounds of at
least `--window` seconds; medians and spread; a window's time is divided by its calls and by the gradient steps of a call.

    python tools/bench_dpg_update.py [--out profiles/r23_dpg_update.txt]
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from bench_policy_lookahead import _reps, _window  # noqa: E402

GAMMA, SIGMA, NOISE_CLIP, TAU, LR = 0.99, 0.2, 0.5, 0.005, 3e-4


def _graph(torch, fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g.keep = fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 4096], help="rows of the minibatches")
    ap.add_argument("--grad-steps", type=int, default=8)
    ap.add_argument("--policy-delay", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_dpg_update.py needs a GPU")
    import td3_vss as example
    from rsoccer_amd.vec import VecVSSEnv
    from rsoccer_amd.vec.optim import DPGOptimizer
    from rsoccer_amd.vec.policy import MLPPolicy, MLPQCritic
    from rsoccer_amd.vec.replay import ReplayBuffer
    n, T, K, delay = args.envs, args.steps, args.grad_steps, args.policy_delay
    env = VecVSSEnv(n, device=0, seed=1)
    env.reset()
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    head = (f"# tools/bench_dpg_update.py: {torch.cuda.get_device_name(0)}, VSS-v0, a {n * T}-row replay buffer, {OD}-64-64-{AD} actor, twin "
            f"{OD + AD}-64-64-1 critics, tanh, updates of {K} gradient steps with policy_delay {delay}, {args.rounds} interleaved rounds of "
            f">= {args.window} s, device events; unit: us per gradient step")
    pol, qnet = MLPPolicy(OD, AD, out_act="tanh"), MLPQCritic(OD, AD)
    torch.manual_seed(0)
    actor0, critics0 = example.mlp(OD, AD, True).to(dev), [example.mlp(OD + AD, 1, False).to(dev) for _ in range(2)]
    t_actor0, t_critics0 = copy.deepcopy(actor0), copy.deepcopy(critics0)
    with torch.no_grad():
        for m in [actor0] + critics0:
            for p in m.parameters():
                p.add_(0.02 * torch.randn_like(p))
        buf = ReplayBuffer(n * T, OD, AD, dev)
        buf.add(env.collect(pol, pol.from_module(actor0).to(dev), T, log_std=torch.full((AD,), -2.3, device=dev), return_final_obs=True))
    data = buf.data()
    torch.cuda.synchronize()

    def flat():
        """a leg's own flat parameter vectors: (actor, its target, critics, their target)"""
        return [pol.from_module(actor0).to(dev), pol.from_module(t_actor0).to(dev),
                torch.stack([qnet.from_module(c) for c in critics0]).to(dev), torch.stack([qnet.from_module(c) for c in t_critics0]).to(dev)]

    def fused_leg(M):
        P, opt = flat(), DPGOptimizer(pol, qnet, 2, device=dev, lr_actor=LR, lr_critic=LR, tau=TAU)
        return lambda: env.dpg_update(buf, pol, P[0], P[1], qnet, P[2], P[3], opt, grad_steps=K, batch_size=M, policy_delay=delay, gamma=GAMMA,
                                      target_noise=SIGMA, noise_clip=NOISE_CLIP, seed=1)

    def example_leg(M, capturable):
        P = flat()
        pa, pc = torch.nn.Parameter(P[0]), torch.nn.Parameter(P[2])
        oa, oc = torch.optim.Adam([pa], lr=LR, capturable=capturable), torch.optim.Adam([pc], lr=LR, capturable=capturable)

        def update():
            for j in range(K):
                with_actor = (j + 1) % delay == 0
                rows = buf.sample_rows(M)
                out = env.dpg_gradient(data, pol, pa, P[1], qnet, pc, P[3], rows=rows, gamma=GAMMA, target_noise=SIGMA, noise_clip=NOISE_CLIP,
                                       noise_seed=1, noise_step=j, actor=with_actor)
                pc.grad = out["grad_critic_params"]
                oc.step()
                if with_actor:
                    pa.grad = out["grad_params"]
                    oa.step()
                    with torch.no_grad():
                        P[1].lerp_(pa, TAU)
                        P[3].lerp_(pc, TAU)
        return update

    def torch_leg(M):
        actor, critics = copy.deepcopy(actor0), copy.deepcopy(critics0)
        t_actor, t_critics = copy.deepcopy(t_actor0), copy.deepcopy(t_critics0)
        oa = torch.optim.Adam(actor.parameters(), lr=LR, capturable=True)
        oc = torch.optim.Adam([p for c in critics for p in c.parameters()], lr=LR, capturable=True)

        def update():
            for j in range(K):
                with_actor = (j + 1) % delay == 0
                idx = buf.sample_rows(M).long()
                example.torch_losses(actor, critics, t_actor, t_critics, data, idx, GAMMA, SIGMA, NOISE_CLIP, with_actor)
                oc.step()
                if with_actor:
                    oa.step()
                    with torch.no_grad():
                        for t, m in zip([t_actor] + t_critics, [actor] + critics):
                            for pt, pm in zip(t.parameters(), m.parameters()):
                                pt.lerp_(pm, TAU)
        return update

    lines, result = [head], {}
    for M in args.rows:
        legs = [("(a) dpg_update, eager", fused_leg(M)), ("(b) dpg_update, graph replay", _graph(torch, fused_leg(M)).replay),
                ("(c) sample_rows + dpg_gradient + Adam + lerp_, eager", example_leg(M, False)),
                ("(d) the same, graph replay (capturable Adam)", _graph(torch, example_leg(M, True)).replay),
                ("(e) all torch, graph replay (capturable Adam)", _graph(torch, torch_leg(M)).replay)]
        reps = [_reps(torch, fn, args.window) for _, fn in legs]
        times = [[] for _ in legs]
        for _ in range(args.rounds):
            for i, (_, fn) in enumerate(legs):
                times[i].append(_window(torch, fn, reps[i]) / K)
        lines.append("")
        lines.append("minibatch of %d rows" % M)
        lines.append("%-54s | %12s | %16s | %s" % ("leg", "us / step", "spread (min-max)", "rounds (us)"))
        med = {}
        for (name, _), ts in zip(legs, times):
            med[name[:3]] = statistics.median(ts) * 1e6
            result["%d %s" % (M, name)] = dict(us=med[name[:3]], rounds_us=[x * 1e6 for x in ts])
            lines.append("%-54s | %12.1f | %7.1f - %6.1f | %s" % (name, med[name[:3]], min(ts) * 1e6, max(ts) * 1e6, " ".join("%.1f" % (x * 1e6) for x in ts)))
        lines.append("dpg_update eager against the example's eager loop: %.2f x; its graph replay against the example loop's: %.2f x, against all torch's: %.2f x"
                     % (med["(c)"] / med["(a)"], med["(d)"] / med["(b)"], med["(e)"] / med["(b)"]))
    print("\n".join(lines), flush=True)
    env.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"dpg_update_bench": result}))


if __name__ == "__main__":
    main()
