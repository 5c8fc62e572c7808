#!/usr/bin/env python
"""Throughput of self-play collection (env.collect(..., opponent=...) -> rsx_task_collect_selfplay, rsoccer_amd/csrc/rsx_selfplay.hip)
next to plain collection (rsx_task_collect_policy, rsoccer_amd/csrc/rsx_collect.hip: the path without an opponent, unchanged) in the
same run.

Needs a GPU and fails without one.  VSS-v0, `--envs` envs, T = `--steps` steps per batch, a 40-64-64-2 tanh policy on both sides.
What the self-play launch adds per env step is a second forward pass and the mirrored row; what it loses is occupancy: both images
share a workgroup's LDS (79 040 B at 8 lanes per env: two workgroups per CU instead of three).  Legs, each on an env of its own:
  - collect, deterministic, and the same with the Gaussian head;
  - self-play, both sides deterministic, and the same with a Gaussian head on both sides.
Device events around each window, a warm-up first, `--rounds` rounds of at least `--window` seconds in which the legs ALTERNATE
(a round runs every leg once, in order); medians.  No ratio is asserted: the file records what was measured.

    python tools/bench_selfplay.py [--out profiles/r19_selfplay.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_policy_lookahead import _reps, _window  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of work per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_selfplay.py needs a GPU")
    from rsoccer_amd.vec import VecVSSEnv
    from rsoccer_amd.vec.policy import MLPPolicy
    n, T = args.envs, args.steps
    head = (f"# tools/bench_selfplay.py: {torch.cuda.get_device_name(0)}, VSS-v0, num_envs {n}, T = {T} steps per batch, 40-64-64-2 tanh policy "
            f"on both sides, {args.rounds} rounds of >= {args.window} s with the legs alternating, device events; unit: env-steps/s")
    with torch.no_grad():
        envs = [VecVSSEnv(n, device=0, seed=s) for s in (1, 1, 1, 1)]
        for e in envs:
            e.reset()
        e_det, e_noise, s_det, s_noise = envs
        pol = MLPPolicy(e_det.sim.obs_dim, e_det.sim.act_dim)
        gen = torch.Generator().manual_seed(0)
        draw = lambda: ((torch.rand(pol.num_params, generator=gen) * 2 - 1) / 8.0).to(e_det.device)   # noqa: E731  (torch's default Linear scale)
        params, opp = draw(), draw()
        log_std = torch.full((e_det.sim.act_dim,), -0.5, device=e_det.device)
        it = [0, 0]

        def noisy():
            it[0] += 1
            return e_noise.collect(pol, params, T, log_std=log_std, iteration=it[0])

        def selfplay_noisy():
            it[1] += 1
            return s_noise.collect(pol, params, T, log_std=log_std, iteration=it[1], opponent=pol, opponent_params=opp, opponent_log_std=log_std)

        legs = [("collect, deterministic", lambda: e_det.collect(pol, params, T)),
                ("self-play, deterministic", lambda: s_det.collect(pol, params, T, opponent=pol, opponent_params=opp)),
                ("collect, Gaussian head", noisy),
                ("self-play, Gaussian heads", selfplay_noisy)]
        reps = [_reps(torch, fn, args.window) for _, fn in legs]
        times = [[] for _ in legs]
        for _ in range(args.rounds):
            for i, (_, fn) in enumerate(legs):
                times[i].append(_window(torch, fn, reps[i]))
    med = [statistics.median(t) for t in times]
    lines = [head, "%-28s | %12s | %11s | %s" % ("leg", "env-steps/s", "us / batch", "rounds (us / batch)")]
    rows = {}
    for (name, _), m, ts in zip(legs, med, times):
        rows[name] = dict(steps_per_s=n * T / m, us_per_batch=m * 1e6, rounds_us=[x * 1e6 for x in ts])
        lines.append("%-28s | %12.4g | %11.1f | %s" % (name, n * T / m, m * 1e6, " ".join("%.1f" % (x * 1e6) for x in ts)))
    lines.append("self-play / collect: %.3f (deterministic), %.3f (Gaussian heads)" %
                 (rows["self-play, deterministic"]["steps_per_s"] / rows["collect, deterministic"]["steps_per_s"],
                  rows["self-play, Gaussian heads"]["steps_per_s"] / rows["collect, Gaussian head"]["steps_per_s"]))
    print("\n".join(lines), flush=True)
    for e in envs:
        e.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"selfplay_bench": rows}))


if __name__ == "__main__":
    main()
