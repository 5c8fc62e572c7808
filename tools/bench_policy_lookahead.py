#!/usr/bin/env python
"""Throughput of the closed-loop lookahead (env.lookahead_policy -> rsx_task_lookahead_policy, rsoccer_amd/csrc/rsx_policy.hip)
next to what a user with a policy in the loop could run before it existed.

Needs a GPU and fails without one.  VSS-v0, `--envs` envs, a 40-64-64-2 tanh policy.  Per row (K policies, H steps):
  - policy:     one launch, num_envs * K pairs, each step's action computed inside it; env-steps/s over the steps really simulated
                (the sum of `steps`: a pair stops at its env's first episode end);
  - open loop:  `lookahead` on the actions that launch recorded — the same steps without the policy, i.e. the policy's cost alone.
Once per run, on a handle of num_envs envs (what examples/vec_policy_loop.py measures, with its own policy functions):
  - fused loop: policy as one hand-written kernel (examples/fused_policy.hip) -> step, replayed from a graph;
  - graph loop: the torch policy (four library kernels) -> step, replayed from a graph.
Device events around each window, a warm-up first, `--rounds` interleaved rounds of at least `--window` seconds; medians.

    python tools/bench_policy_lookahead.py [--out profiles/r11_policy_lookahead.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def _window(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def _reps(torch, fn, window):
    for _ in range(2):   # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    t = _window(torch, fn, 2)
    return max(2, int(window / max(t, 1e-6)) + 1)


def _loop_rate(torch, envs, fused, iters, rounds, window):
    """env-steps/s of policy -> step replayed from a graph (examples/vec_policy_loop.py's loop and policies)"""
    import vec_policy_loop as loop
    from rsoccer_amd.vec import VecVSSEnv
    env = VecVSSEnv(envs, device=0, seed=0)
    make = loop.make_fused_policy if fused else loop.make_policy
    policy = make(env.sim.obs_dim, env.sim.act_dim, env.device)
    actions = torch.zeros(envs, env.sim.act_dim, device=env.device)
    env.reset()
    with torch.no_grad():
        loop.run_eager(env, policy, actions, 20)
        g = loop.build_graph(env, policy, actions, iters)
        reps = _reps(torch, g.replay, window)
        t = statistics.median(_window(torch, g.replay, reps) for _ in range(rounds))
    env.close()
    return envs * iters / t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--K", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--H", type=int, nargs="+", default=[20, 1200])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of work per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_lookahead.py needs a GPU")
    from rsoccer_amd.vec import VecVSSEnv
    from rsoccer_amd.vec.policy import MLPPolicy
    lines = [f"# tools/bench_policy_lookahead.py: {torch.cuda.get_device_name(0)}, VSS-v0, num_envs {args.envs}, 40-64-64-2 tanh policy, "
             f"{args.rounds} interleaved rounds of >= {args.window} s, device events; unit: env-steps/s over the steps simulated",
             "%4s %5s | %12s %11s | %12s %11s | %9s | %s" % ("K", "H", "policy", "us/launch", "open loop", "us/launch", "policy/open", "steps simulated / nominal")]
    print("\n".join(lines), flush=True)
    env = VecVSSEnv(args.envs, device=0, seed=1)
    env.reset()   # straight after reset(): H = max_episode_steps scores whole episodes
    pol = MLPPolicy(env.sim.obs_dim, env.sim.act_dim)
    gen = torch.Generator().manual_seed(0)
    rows = []
    for K in args.K:
        # a population around zero, scaled like torch's default Linear initialisation
        params = ((torch.rand(K, pol.num_params, generator=gen) * 2 - 1) / 8.0).to(env.device)
        for H in args.H:
            rec = env.lookahead_policy(pol, params, H, gamma=0.99, return_actions=True)
            torch.cuda.synchronize()
            acts, sim = rec["actions"], int(rec["steps"].sum())
            closed = lambda: env.lookahead_policy(pol, params, H, gamma=0.99)
            opened = lambda: env.lookahead(acts, gamma=0.99)
            rc, ro = _reps(torch, closed, args.window), _reps(torch, opened, args.window)
            tc, to = [], []
            for _ in range(args.rounds):
                tc.append(_window(torch, closed, rc))
                to.append(_window(torch, opened, ro))
            c, o = statistics.median(tc), statistics.median(to)
            rows.append(dict(K=K, H=H, num_envs=args.envs, policy_steps_per_s=sim / c, policy_us=c * 1e6, open_loop_steps_per_s=sim / o,
                             open_loop_us=o * 1e6, steps_simulated=sim, steps_nominal=args.envs * K * H,
                             policy_rounds_us=[x * 1e6 for x in tc], open_loop_rounds_us=[x * 1e6 for x in to]))
            line = "%4d %5d | %12.4g %11.1f | %12.4g %11.1f | %9.2f | %d / %d" % (K, H, sim / c, c * 1e6, sim / o, o * 1e6, o / c, sim, args.envs * K * H)
            lines.append(line)
            print(line, flush=True)
            del rec, acts
            torch.cuda.empty_cache()
    env.close()
    loops = {}
    for name, fused in (("fused policy kernel -> step, graph replay", True), ("torch policy -> step, graph replay", False)):
        loops[name] = _loop_rate(torch, args.envs, fused, 8, args.rounds, args.window)
        line = "%-44s %12.4g env-steps/s" % (name, loops[name])
        lines.append(line)
        print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"policy_lookahead_bench": rows, "loops": loops}))


if __name__ == "__main__":
    main()
