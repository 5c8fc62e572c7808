#!/usr/bin/env python
"""Throughput of on-policy collection in one launch (env.collect -> rsx_task_collect_policy, rsoccer_amd/csrc/rsx_collect.hip) next to
the ways the same [T, B] batch can be produced without it.

Needs a GPU and fails without one.  VSS-v0, `--envs` envs, T = `--steps` steps per batch, a 40-64-64-2 tanh policy.  In one run:
  - collect:          one launch per batch, deterministic head; and the same with the Gaussian head (mean, sample recorded too);
  - fused loop:       T x (policy as one hand-written kernel -> step), each iteration copying obs, reward and the two flags into the
                      batch and writing its action straight into it, replayed from one graph.  The kernel is examples/fused_policy.hip's
                      40-64-2 policy (one hidden layer: less arithmetic than the collector's policy, in the loop's favour);
  - graph loop:       the same with the torch policy of examples/vec_policy_loop.py (four library kernels);
  - lookahead_policy: one policy (K = 1), horizon T, both recordings — the closed-loop lookahead records the same rows but leaves the
                      env where it was and stops a pair at its first episode end.
Device events around each window, a warm-up first, `--rounds` interleaved rounds of at least `--window` seconds; medians.

    python tools/bench_collect.py [--out profiles/r12_collect.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_policy_lookahead import _reps, _window  # noqa: E402


def _loop_graph(torch, env, policy, T):
    """one graph of T x (record obs -> policy -> step -> record reward and flags) into [T, B] tensors, as a trainer would keep them"""
    n, dev = env.num_envs, env.device
    t = env._t
    obs = torch.empty(T, n, env.sim.obs_dim, device=dev)
    acts = torch.zeros(T, n, env.sim.act_dim, device=dev)
    rew = torch.empty(T, n, device=dev)
    term = torch.empty(T, n, dtype=torch.uint8, device=dev)
    trunc = torch.empty(T, n, dtype=torch.uint8, device=dev)

    def batch():
        for i in range(T):
            obs[i].copy_(t["obs"])
            env.step(policy(t["obs"], acts[i]))
            rew[i].copy_(t["reward"])
            term[i].copy_(t["terminated"])
            trunc[i].copy_(t["truncated"])

    env.enable_graph_capture()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # torch's warm-up convention (real steps)
        batch()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        batch()
    g.keep = (obs, acts, rew, term, trunc)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of work per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_collect.py needs a GPU")
    import vec_policy_loop as loop
    from rsoccer_amd.vec import VecVSSEnv
    from rsoccer_amd.vec.policy import MLPPolicy
    n, T = args.envs, args.steps
    head = (f"# tools/bench_collect.py: {torch.cuda.get_device_name(0)}, VSS-v0, num_envs {n}, T = {T} steps per batch, 40-64-64-2 tanh policy, "
            f"{args.rounds} interleaved rounds of >= {args.window} s, device events; unit: env-steps/s")
    with torch.no_grad():
        envs = [VecVSSEnv(n, device=0, seed=s) for s in (1, 1, 2, 3, 4)]
        for e in envs:
            e.reset()
        e_det, e_noise, e_fused, e_torch, e_look = envs
        pol = MLPPolicy(e_det.sim.obs_dim, e_det.sim.act_dim)
        gen = torch.Generator().manual_seed(0)
        params = ((torch.rand(pol.num_params, generator=gen) * 2 - 1) / 8.0).to(e_det.device)   # scaled like torch's default Linear initialisation
        log_std = torch.full((e_det.sim.act_dim,), -0.5, device=e_det.device)
        it = [0]

        def noisy():
            it[0] += 1
            return e_noise.collect(pol, params, T, log_std=log_std, iteration=it[0])

        g_fused = _loop_graph(torch, e_fused, loop.make_fused_policy(e_fused.sim.obs_dim, e_fused.sim.act_dim, e_fused.device), T)
        g_torch = _loop_graph(torch, e_torch, loop.make_policy(e_torch.sim.obs_dim, e_torch.sim.act_dim, e_torch.device), T)
        legs = [("collect, deterministic", lambda: e_det.collect(pol, params, T), n * T),
                ("collect, Gaussian head (+ mean, sample, log_prob)", noisy, n * T),
                ("fused policy kernel -> step, recorded, graph replay", g_fused.replay, n * T),
                ("torch policy -> step, recorded, graph replay", g_torch.replay, n * T)]
        rec = e_look.lookahead_policy(pol, params[None], T, gamma=0.99, return_actions=True, return_policy_obs=True)
        torch.cuda.synchronize()
        legs.append(("lookahead_policy, K = 1, both recordings", lambda: e_look.lookahead_policy(pol, params[None], T, gamma=0.99,
                                                                                              return_actions=True, return_policy_obs=True),
                     int(rec["steps"].sum())))
        reps = [_reps(torch, fn, args.window) for _, fn, _ in legs]
        times = [[] for _ in legs]
        for _ in range(args.rounds):
            for i, (_, fn, _) in enumerate(legs):
                times[i].append(_window(torch, fn, reps[i]))
    med = [statistics.median(t) for t in times]
    lines = [head, "%-52s | %12s | %11s | %s" % ("leg", "env-steps/s", "us / batch", "rounds (us / batch)")]
    rows = {}
    for (name, _, steps), m, ts in zip(legs, med, times):
        rows[name] = dict(steps_per_s=steps / m, us_per_batch=m * 1e6, steps=steps, rounds_us=[x * 1e6 for x in ts])
        lines.append("%-52s | %12.4g | %11.1f | %s" % (name, steps / m, m * 1e6, " ".join("%.1f" % (x * 1e6) for x in ts)))
    base = rows["fused policy kernel -> step, recorded, graph replay"]["steps_per_s"]
    lines.append("collect / fused loop: %.2f (deterministic), %.2f (Gaussian head)" %
                 (rows["collect, deterministic"]["steps_per_s"] / base, rows["collect, Gaussian head (+ mean, sample, log_prob)"]["steps_per_s"] / base))
    print("\n".join(lines), flush=True)
    for e in envs:
        e.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"collect_bench": rows}))


if __name__ == "__main__":
    main()
