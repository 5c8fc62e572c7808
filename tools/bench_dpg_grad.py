#!/usr/bin/env python
"""Time of the TD3 gradients of a replayed minibatch in four launches (env.dpg_gradient -> rsx_task_dpg_gradient,
rsoccer_amd/csrc/rsx_dpg.hip) next to the torch path it replaces.

Needs a GPU and fails without one.  VSS-v0 shapes: a 40-64-64-2 tanh actor and twin 42-64-64-1 tanh critics, their targets 0.02 away;
a ReplayBuffer of `--envs` x `--steps` rows (4096 x 128 = 524 288) filled by one collect(); per minibatch size in `--rows` a fixed
draw of sample_rows.  In one run, per size:
  (a) dpg_gradient:              env.dpg_gradient with the actor launch;
  (b) dpg_gradient, no actor:    the same with actor=False (TD3's delayed steps);
  (c) torch, eager:              examples/td3_vss.py's torch_losses (the gather, six forwards, two backward()) with the actor;
  (d) torch, graph:              the same replayed from one graph — the fair opponent, launch overhead removed.
Device events around each window, a warm-up first, `--rounds` interleaved rounds of at least `--window` seconds; medians and spread.
(a) is set against its floor at the fp32 vector peak (157.3 TFLOP/s): 2 FLOP per weight and row for a forward, 2 more for a
back-propagation through the layer and 2 more for its weight gradient.

    python tools/bench_dpg_grad.py [--out profiles/r22_dpg_grad.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from bench_policy_lookahead import _reps, _window  # noqa: E402

PEAK_FP32 = 157.3e12
GAMMA, SIGMA, NOISE_CLIP = 0.99, 0.2, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 4096, 131072], help="rows of the minibatches")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_dpg_grad.py needs a GPU")
    import td3_vss as example
    from rsoccer_amd.vec import VecVSSEnv
    from rsoccer_amd.vec.policy import MLPPolicy, MLPQCritic
    from rsoccer_amd.vec.replay import ReplayBuffer
    n, T = args.envs, args.steps
    env = VecVSSEnv(n, device=0, seed=1)
    env.reset()
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    head = (f"# tools/bench_dpg_grad.py: {torch.cuda.get_device_name(0)}, VSS-v0, a {n * T}-row replay buffer, {OD}-64-64-{AD} actor, twin "
            f"{OD + AD}-64-64-1 critics, tanh, {args.rounds} interleaved rounds of >= {args.window} s, device events; unit: us per call")
    pol, qnet = MLPPolicy(OD, AD, out_act="tanh"), MLPQCritic(OD, AD)
    torch.manual_seed(0)
    actor, t_actor = example.mlp(OD, AD, True).to(dev), example.mlp(OD, AD, True).to(dev)
    critics = [example.mlp(OD + AD, 1, False).to(dev) for _ in range(2)]
    t_critics = [example.mlp(OD + AD, 1, False).to(dev) for _ in range(2)]
    with torch.no_grad():
        for t, m in zip([t_actor] + t_critics, [actor] + critics):
            t.load_state_dict(m.state_dict())
            for p in m.parameters():
                p.add_(0.02 * torch.randn_like(p))
        p_actor, pt_actor = pol.from_module(actor).to(dev), pol.from_module(t_actor).to(dev)
        p_critics = torch.stack([qnet.from_module(c) for c in critics]).to(dev)
        pt_critics = torch.stack([qnet.from_module(c) for c in t_critics]).to(dev)
        buf = ReplayBuffer(n * T, OD, AD, dev)
        buf.add(env.collect(pol, p_actor, T, log_std=torch.full((AD,), -2.3, device=dev), return_final_obs=True))
    data = buf.data()
    torch.cuda.synchronize()

    w1a, w2, woa, w1c, woc = OD * 64, 64 * 64, 64 * AD, (OD + AD) * 64, 64
    flop_row = (2 * (w1a + w2 + woa) + 2 * 2 * (w1c + w2 + woc)        # the targets: three forwards
                + 2 * (4 * w1c + 6 * w2 + 6 * woc)                     # the critics: forward, back-propagation, weight gradients
                + (4 * w1a + 6 * w2 + 6 * woa)                         # the actor
                + (2 * w1c + 4 * w2 + 4 * woc + 2 * AD * 64))          # critic 0 under the actor: forward and back to its action inputs
    lines, result = [head], {}
    for M in args.rows:
        rows = buf.sample_rows(M, generator=torch.Generator(device=dev).manual_seed(M))
        idx = rows.long()
        fused = lambda actor_too=True: env.dpg_gradient(data, pol, p_actor, pt_actor, qnet, p_critics, pt_critics, rows=rows, gamma=GAMMA,  # noqa: E731
                                                        target_noise=SIGMA, noise_clip=NOISE_CLIP, noise_seed=1, noise_step=0, actor=actor_too)
        torch_path = lambda: example.torch_losses(actor, critics, t_actor, t_critics, data, idx, GAMMA, SIGMA, NOISE_CLIP, True)  # noqa: E731
        # agreement first, without the smoothing noise (the two paths draw it differently): the engine against torch's float32 autograd
        out = env.dpg_gradient(data, pol, p_actor, pt_actor, qnet, p_critics, pt_critics, rows=rows, gamma=GAMMA)
        example.torch_losses(actor, critics, t_actor, t_critics, data, idx, GAMMA, 0.0, NOISE_CLIP, True)
        want_a = torch.nn.utils.parameters_to_vector([p.grad for p in actor.parameters()])
        want_c = torch.stack([torch.nn.utils.parameters_to_vector([p.grad for p in c.parameters()]) for c in critics])
        dev_a = float((out["grad_params"] - want_a).abs().max() / want_a.abs().max())
        dev_c = float((out["grad_critic_params"] - want_c).abs().max() / want_c.abs().max())

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                torch_path()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            graph.keep = torch_path()
        legs = [("(a) dpg_gradient", fused), ("(b) dpg_gradient, actor=False", lambda: fused(False)),
                ("(c) torch losses + 2 backward(), eager", torch_path), ("(d) the same, graph replay", graph.replay)]
        reps = [_reps(torch, fn, args.window) for _, fn in legs]
        times = [[] for _ in legs]
        for _ in range(args.rounds):
            for i, (_, fn) in enumerate(legs):
                times[i].append(_window(torch, fn, reps[i]))
        lines.append("")
        lines.append("minibatch of %d rows" % M)
        lines.append("%-42s | %12s | %16s | %s" % ("leg", "us / call", "spread (min-max)", "rounds (us)"))
        med = {}
        for (name, _), ts in zip(legs, times):
            med[name[:3]] = statistics.median(ts) * 1e6
            result["%d %s" % (M, name)] = dict(us=med[name[:3]], rounds_us=[x * 1e6 for x in ts])
            lines.append("%-42s | %12.1f | %7.1f - %6.1f | %s" % (name, med[name[:3]], min(ts) * 1e6, max(ts) * 1e6, " ".join("%.1f" % (x * 1e6) for x in ts)))
        floor = M * flop_row / PEAK_FP32 * 1e6
        lines.append("(a): %d rows x %d FLOP = %.3f GFLOP, floor %.2f us at the fp32 vector peak, measured %.1f us = %.2f %% of peak" %
                     (M, flop_row, M * flop_row * 1e-9, floor, med["(a)"], 100.0 * floor / med["(a)"]))
        lines.append("dpg_gradient against the graph replay of the torch path: %.2f x, against the eager path: %.2f x; without the actor %.2f x of the full call's time" %
                     (med["(d)"] / med["(a)"], med["(c)"] / med["(a)"], med["(b)"] / med["(a)"]))
        lines.append("largest relative deviation from torch's float32 autograd (no smoothing noise): actor %.3g, critics %.3g" % (dev_a, dev_c))
    print("\n".join(lines), flush=True)
    env.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"dpg_grad_bench": result}))


if __name__ == "__main__":
    main()
