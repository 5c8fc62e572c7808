#!/usr/bin/env python
"""Time of the soft actor-critic gradients of a replayed minibatch in six launches (env.sac_gradient -> rsx_task_sac_gradient,
rsoccer_amd/csrc/rsx_sac.hip) next to the torch path it replaces, and the rate of collection under SAC's actor
(env.collect(MLPGaussianPolicy) -> rsx_task_collect_gaussian) next to the plain collector's Gaussian head on the same handle.

Needs a GPU and fails without one.  VSS-v0 shapes: a 40-64-64-4 tanh actor (mean and log-std) and twin 42-64-64-1 tanh critics, the
target critics 0.02 away; a ReplayBuffer of `--envs` x `--steps` rows (4096 x 128 = 524 288) filled by one collect(MLPGaussianPolicy);
per minibatch size in `--rows` a fixed draw of sample_rows.  In one run, per size:
  (a) sac_gradient:     env.sac_gradient;
  (b) torch, eager:     examples/sac_vss.py's sac_losses (the gather, seven forwards) and its three backward();
  (c) torch, graph:     the same replayed from one graph — the fair opponent, launch overhead removed.
Then, on the same handle: collect(MLPGaussianPolicy), collect(MLPPolicy, log_std=...) and collect(MLPGaussianPolicy, deterministic=True),
T = `--steps`, each leg with what collect() does in torch behind the launch (flags, log_prob).
Device events around each window, a warm-up first, `--rounds` interleaved rounds of at least `--window` seconds; medians and spread.

    python tools/bench_sac_grad.py [--out profiles/r24_sac_grad.txt]
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

GAMMA = 0.99


def _timed(torch, legs, rounds, window):
    reps = [_reps(torch, fn, window) for _, fn in legs]
    times = [[] for _ in legs]
    for _ in range(rounds):
        for i, (_, fn) in enumerate(legs):
            times[i].append(_window(torch, fn, reps[i]))
    return times


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
        raise SystemExit("bench_sac_grad.py needs a GPU")
    import sac_vss as example
    from rsoccer_amd.vec import VecVSSEnv
    from rsoccer_amd.vec.policy import MLPGaussianPolicy, MLPPolicy, MLPQCritic
    from rsoccer_amd.vec.replay import ReplayBuffer
    n, T = args.envs, args.steps
    env = VecVSSEnv(n, device=0, seed=1)
    env.reset()
    dev, OD, AD = env.device, env.sim.obs_dim, env.sim.act_dim
    head = (f"# tools/bench_sac_grad.py: {torch.cuda.get_device_name(0)}, VSS-v0, a {n * T}-row replay buffer, {OD}-64-64-{2 * AD} actor, twin "
            f"{OD + AD}-64-64-1 critics, tanh, {args.rounds} interleaved rounds of >= {args.window} s, device events")
    pol, plain, qnet = MLPGaussianPolicy(OD, AD), MLPPolicy(OD, AD), MLPQCritic(OD, AD)
    torch.manual_seed(0)
    with torch.no_grad():
        p_actor = pol.from_module(example.mlp(OD, 2 * AD)).to(dev)
        p_plain = plain.from_module(example.mlp(OD, AD)).to(dev)
        pt_critics = torch.stack([qnet.from_module(example.mlp(OD + AD, 1)) for _ in range(2)]).to(dev)
        p_critics = pt_critics + 0.02 * torch.randn_like(pt_critics)
        log_alpha = torch.full((1,), -1.0, device=dev)
        buf = ReplayBuffer(n * T, OD, AD, dev)
        buf.add(env.collect(pol, p_actor, T, return_final_obs=True))
    data = buf.data()
    torch.cuda.synchronize()
    leaves = [torch.nn.Parameter(t.clone()) for t in (p_actor, p_critics, log_alpha)]

    def torch_path(idx):
        for leaf in leaves:
            leaf.grad = None
        loss_q, loss_pi, loss_alpha, _ = example.sac_losses(pol, leaves[0], qnet, leaves[1], pt_critics, leaves[2], data, idx, GAMMA, -float(AD))
        loss_q.backward()
        loss_pi.backward()
        loss_alpha.backward()
        return loss_q.detach(), loss_pi.detach(), loss_alpha.detach()   # (no autograd graph outlives the call)

    def agreement(rows, idx):
        """the call against torch's float32 autograd fed the call's own eps / next_eps: the largest relative deviation of the actor's and
        of the critics' gradients.  Leaves and graph of its own, all dropped on return: nothing of it is alive when torch_path is captured
        (an autograd graph kept alive from another stream breaks the capture of a later backward())"""
        f32 = torch.float32
        out = env.sac_gradient(data, pol, p_actor, qnet, p_critics, pt_critics, log_alpha, rows=rows, gamma=GAMMA, noise_seed=1, noise_step=0,
                               return_rows=True)
        la, lc = torch.nn.Parameter(p_actor.clone()), torch.nn.Parameter(p_critics.clone())
        with torch.no_grad():
            a2, logp2, _ = pol.sample(data["next_obs"][idx], p_actor, out["next_eps"], dtype=f32)
            q2 = torch.stack([qnet.forward(data["next_obs"][idx], a2, p, dtype=f32).squeeze(-1) for p in pt_critics]).min(0).values
            y = torch.where(data["terminated"][idx], data["reward"][idx], data["reward"][idx] + GAMMA * (q2 - log_alpha.exp() * logp2))
        q = torch.stack([qnet.forward(data["obs"][idx], data["actions"][idx], p, dtype=f32).squeeze(-1) for p in lc])
        g_c, = torch.autograd.grad((0.5 * (q - y).pow(2).mean(-1)).sum(), [lc])
        a1, logp1, _ = pol.sample(data["obs"][idx], la, out["eps"], dtype=f32)
        qa = torch.stack([qnet.forward(data["obs"][idx], a1, p, dtype=f32).squeeze(-1) for p in p_critics]).min(0).values
        g_a, = torch.autograd.grad((log_alpha.exp() * logp1 - qa).mean(), [la])
        return (float((out["grad_params"] - g_a).abs().max() / g_a.abs().max()),
                float((out["grad_critic_params"] - g_c).abs().max() / g_c.abs().max()))

    lines, result = [head, "", "unit: us per call"], {}
    for M in args.rows:
        rows = buf.sample_rows(M, generator=torch.Generator(device=dev).manual_seed(M))
        idx = rows.long()
        fused = lambda: env.sac_gradient(data, pol, p_actor, qnet, p_critics, pt_critics, log_alpha, rows=rows, gamma=GAMMA,  # noqa: E731
                                         noise_seed=1, noise_step=0)
        dev_a, dev_c = agreement(rows, idx)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                torch_path(idx)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            graph.keep = torch_path(idx)
        legs = [("(a) sac_gradient", fused), ("(b) torch losses + 3 backward(), eager", lambda: torch_path(idx)),
                ("(c) the same, graph replay", graph.replay)]
        times = _timed(torch, legs, args.rounds, args.window)
        lines.append("")
        lines.append("minibatch of %d rows" % M)
        lines.append("%-42s | %12s | %16s | %s" % ("leg", "us / call", "spread (min-max)", "rounds (us)"))
        med = {}
        for (name, _), ts in zip(legs, times):
            med[name[:3]] = statistics.median(ts) * 1e6
            result["%d %s" % (M, name)] = dict(us=med[name[:3]], rounds_us=[x * 1e6 for x in ts])
            lines.append("%-42s | %12.1f | %7.1f - %6.1f | %s" % (name, med[name[:3]], min(ts) * 1e6, max(ts) * 1e6, " ".join("%.1f" % (x * 1e6) for x in ts)))
        lines.append("sac_gradient against the graph replay of the torch path: %.2f x, against the eager path: %.2f x" %
                     (med["(c)"] / med["(a)"], med["(b)"] / med["(a)"]))
        lines.append("largest relative deviation from torch's float32 autograd on the call's own draws: actor %.3g, critics %.3g" % (dev_a, dev_c))

    # ---- collection under the squashed head next to the plain head, one handle ----
    with torch.no_grad():
        log_std = torch.full((AD,), -0.5, device=dev)
        it = [0]

        def collect(policy, params, **kw):
            it[0] += 1
            return env.collect(policy, params, T, iteration=it[0], **kw)

        legs = [("collect(MLPPolicy, log_std=...)", lambda: collect(plain, p_plain, log_std=log_std)),
                ("collect(MLPGaussianPolicy)", lambda: collect(pol, p_actor)),
                ("collect(MLPGaussianPolicy, deterministic=True)", lambda: collect(pol, p_actor, deterministic=True))]
        times = _timed(torch, legs, args.rounds, max(args.window, 0.25))
    lines += ["", "collection, num_envs %d, T = %d; unit: env-steps/s" % (n, T),
              "%-48s | %12s | %11s | %s" % ("leg", "env-steps/s", "us / batch", "rounds (us / batch)")]
    rate = {}
    for (name, _), ts in zip(legs, times):
        m = statistics.median(ts)
        rate[name] = n * T / m
        result[name] = dict(steps_per_s=rate[name], us_per_batch=m * 1e6, rounds_us=[x * 1e6 for x in ts])
        lines.append("%-48s | %12.4g | %11.1f | %s" % (name, rate[name], m * 1e6, " ".join("%.1f" % (x * 1e6) for x in ts)))
    lines.append("squashed head / plain head: %.3f" % (rate["collect(MLPGaussianPolicy)"] / rate["collect(MLPPolicy, log_std=...)"]))
    print("\n".join(lines), flush=True)
    env.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"sac_grad_bench": result}))


if __name__ == "__main__":
    main()
