#!/usr/bin/env python
"""Time per gradient step of the soft actor-critic update phase in one call (env.sac_update -> rsx_task_sac_update,
rsoccer_amd/csrc/rsx_sac_update.hip) next to the loop it replaces.

Needs a GPU and fails without one.  VSS-v0 shapes: a 40-64-64-4 tanh actor with a squashed Gaussian head and twin 42-64-64-1 tanh
critics, their targets 0.02 away; a ReplayBuffer of `--envs` x `--steps` rows filled by one collect(); an update of `--grad-steps`
gradient steps.  In one run, per minibatch size in `--rows`:
  (a) sac_update:                 env.sac_update, eager;
  (b) sac_update, graph:          the same replayed from one graph;
  (c) example loop, eager:        examples/sac_vss.py's loop — ReplayBuffer.sample_rows, env.sac_gradient, three torch.optim.Adam on the
                                  flat tensors, lerp_;
  (d) example loop, graph:        that loop replayed from one graph with torch.optim.Adam(capturable=True).
Every leg trains its own copy of the networks.  Device events around each window, a warm-up first, `--rounds` interleaved rounds of at
least `--window` seconds; medians and spread; a window's time is divided by its calls and by the gradient steps of a call.

    python tools/bench_sac_update.py [--out profiles/r25_sac_update.txt]
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

from bench_dpg_update import _graph  # noqa: E402
from bench_policy_lookahead import _reps, _window  # noqa: E402

GAMMA, TAU, LR = 0.99, 0.005, 3e-4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 4096], help="rows of the minibatches")
    ap.add_argument("--grad-steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sac_update.py needs a GPU")
    import sac_vss as example
    from rsoccer_amd.vec import VecVSSEnv
    from rsoccer_amd.vec.optim import SACOptimizer
    from rsoccer_amd.vec.policy import MLPGaussianPolicy, MLPQCritic
    from rsoccer_amd.vec.replay import ReplayBuffer
    n, T, K = args.envs, args.steps, args.grad_steps
    env = VecVSSEnv(n, device=0, seed=1)
    env.reset()
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    head = (f"# tools/bench_sac_update.py: {torch.cuda.get_device_name(0)}, VSS-v0, a {n * T}-row replay buffer, {OD}-64-64-{2 * AD} actor "
            f"(squashed Gaussian head), twin {OD + AD}-64-64-1 critics, tanh, a learned temperature, updates of {K} gradient steps, "
            f"{args.rounds} interleaved rounds of >= {args.window} s, device events; unit: us per gradient step")
    pol, qnet = MLPGaussianPolicy(OD, AD, hidden=64, layers=2, hidden_act="tanh"), MLPQCritic(OD, AD, hidden=64, layers=2, hidden_act="tanh")
    torch.manual_seed(0)
    actor0 = pol.from_module(example.mlp(OD, 2 * AD)).to(dev)
    t_critics0 = torch.stack([qnet.from_module(example.mlp(OD + AD, 1)) for _ in range(2)]).to(dev)
    critics0 = t_critics0 + 0.02 * torch.randn_like(t_critics0)
    buf = ReplayBuffer(n * T, OD, AD, dev)
    buf.add(env.collect(pol, actor0, T, noise_seed=3, return_final_obs=True))
    data = buf.data()
    torch.cuda.synchronize()

    def flat():
        """a leg's own tensors: (actor, critics, their target, log_alpha)"""
        return [actor0.clone(), critics0.clone(), t_critics0.clone(), torch.zeros(1, device=dev)]

    def fused_leg(M):
        P, opt = flat(), SACOptimizer(pol, qnet, 2, device=dev, lr_actor=LR, lr_critic=LR, lr_alpha=LR, tau=TAU)
        return lambda: env.sac_update(buf, pol, P[0], qnet, P[1], P[2], P[3], opt, grad_steps=K, batch_size=M, gamma=GAMMA, seed=1)

    def example_leg(M, capturable):
        P = flat()
        leaves = [torch.nn.Parameter(P[k]) for k in (1, 0, 3)]   # critics, actor, log_alpha: the example's order of steps
        opts = [torch.optim.Adam([p], lr=LR, capturable=capturable) for p in leaves]
        pc, pa, la = leaves

        def update():
            for j in range(K):
                rows = buf.sample_rows(M)
                out = env.sac_gradient(data, pol, pa, qnet, pc, P[2], la, rows=rows, gamma=GAMMA, noise_seed=1, noise_step=j)
                pa.grad, pc.grad, la.grad = out["grad_params"], out["grad_critic_params"], out["grad_log_alpha"]
                for o in opts:
                    o.step()
                with torch.no_grad():
                    P[2].lerp_(pc, TAU)
        return update

    lines, result = [head], {}
    for M in args.rows:
        legs = [("(a) sac_update, eager", fused_leg(M)), ("(b) sac_update, graph replay", _graph(torch, fused_leg(M)).replay),
                ("(c) sample_rows + sac_gradient + 3 Adam + lerp_, eager", example_leg(M, False)),
                ("(d) the same, graph replay (capturable Adam)", _graph(torch, example_leg(M, True)).replay)]
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
        lines.append("sac_update eager against the example's eager loop: %.2f x; its graph replay against the example loop's: %.2f x"
                     % (med["(c)"] / med["(a)"], med["(d)"] / med["(b)"]))
    print("\n".join(lines), flush=True)
    env.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"sac_update_bench": result}))


if __name__ == "__main__":
    main()
