#!/usr/bin/env python
"""Throughput of policy-vs-policy matches (env.lookahead_match -> rsx_task_lookahead_match, rsoccer_amd/csrc/rsx_match.hip) next to
its two neighbours in the same run: the committed self-play collect() of the same batch (rsx_task_collect_selfplay) and
lookahead_policy with K policies and no opponent (rsx_task_lookahead_policy).

Needs a GPU and fails without one.  VSS-v0, `--envs` envs, H = `--steps` steps, a 40-64-64-2 tanh policy on both sides, one seat a
side, straight after reset().  Legs:
  - lookahead_match with (K, M) = (1, 1), (4, 4) and (16, 1);
  - self-play collect, deterministic heads, T = H (it commits: every call continues where the last one stopped);
  - lookahead_policy with K = 1, 4 and 16.
Unit: pair-steps/s — simulated steps of (env, k, m) triples, counted from the call's own `steps` output (a pair stops at its env's first
episode end; the lookahead calls leave the env untouched, so every repetition simulates the same steps); for collect env-steps/s.
Device events around each window, a warm-up first, `--rounds` rounds of at least `--window` seconds in which the legs ALTERNATE (a
round runs every leg once, in order); medians.  No ratio is asserted: the file records what was measured.

    python tools/bench_match.py [--out profiles/r21_match.txt]
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

PAIRS = [(1, 1), (4, 4), (16, 1)]
POLICIES = [1, 4, 16]


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
        raise SystemExit("bench_match.py needs a GPU")
    from rsoccer_amd.vec import VecVSSEnv
    from rsoccer_amd.vec.policy import MLPPolicy
    n, H = args.envs, args.steps
    head = (f"# tools/bench_match.py: {torch.cuda.get_device_name(0)}, VSS-v0, num_envs {n}, H = {H}, 40-64-64-2 tanh policy on both sides, "
            f"one seat a side, {args.rounds} rounds of >= {args.window} s with the legs alternating, device events; unit: pair-steps/s")
    with torch.no_grad():
        ev, sp = VecVSSEnv(n, device=0, seed=1), VecVSSEnv(n, device=0, seed=1)
        ev.reset(); sp.reset()
        pol = MLPPolicy(ev.sim.obs_dim, ev.sim.act_dim)
        gen = torch.Generator().manual_seed(0)
        draw = lambda k: ((torch.rand(k, pol.num_params, generator=gen) * 2 - 1) / 8.0).to(ev.device)   # noqa: E731  (torch's default Linear scale)
        actors, opps = draw(16), draw(4)
        legs, work = [], []
        for K, M in PAIRS:
            fn = lambda K=K, M=M: ev.lookahead_match(pol, actors[:K], pol, opps[:M], H)   # noqa: E731
            legs.append((f"match K={K} M={M}", fn))
            work.append(int(fn()["steps"].sum()))
        legs.append(("self-play collect", lambda: sp.collect(pol, actors[0], H, opponent=pol, opponent_params=opps[0])))
        work.append(n * H)
        for K in POLICIES:
            fn = lambda K=K: ev.lookahead_policy(pol, actors[:K], H)   # noqa: E731
            legs.append((f"lookahead_policy K={K}", fn))
            work.append(int(fn()["steps"].sum()))
        reps = [_reps(torch, fn, args.window) for _, fn in legs]
        times = [[] for _ in legs]
        for _ in range(args.rounds):
            for i, (_, fn) in enumerate(legs):
                times[i].append(_window(torch, fn, reps[i]))
    med = [statistics.median(t) for t in times]
    lines = [head, "%-24s | %12s | %12s | %11s | %s" % ("leg", "pair-steps", "pair-steps/s", "us / call", "rounds (us / call)")]
    rows = {}
    for (name, _), w, m, ts in zip(legs, work, med, times):
        rows[name] = dict(pair_steps=w, steps_per_s=w / m, us_per_call=m * 1e6, rounds_us=[x * 1e6 for x in ts])
        lines.append("%-24s | %12d | %12.4g | %11.1f | %s" % (name, w, w / m, m * 1e6, " ".join("%.1f" % (x * 1e6) for x in ts)))
    rate = lambda name: rows[name]["steps_per_s"]   # noqa: E731
    lines.append("match / self-play collect: " + ", ".join("%.3f (K=%d M=%d)" % (rate(f"match K={K} M={M}") / rate("self-play collect"), K, M)
                                                           for K, M in PAIRS))
    lines.append("match / lookahead_policy with K * M policies: " +
                 ", ".join("%.3f (K=%d M=%d)" % (rate(f"match K={K} M={M}") / rate(f"lookahead_policy K={K * M}"), K, M) for K, M in PAIRS))
    print("\n".join(lines), flush=True)
    ev.close(); sp.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"match_bench": rows}))


if __name__ == "__main__":
    main()
