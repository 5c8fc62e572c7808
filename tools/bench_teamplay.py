#!/usr/bin/env python
"""Throughput of team-play collection (env.collect(..., team=True / opponent_team=True) -> rsx_task_collect_team,
rsoccer_amd/csrc/rsx_teamplay.hip) next to plain collection (rsx_collect.hip) and self-play (rsx_selfplay.hip), both unchanged, in the
same run.

Needs a GPU and fails without one.  VSS-v0, `--envs` envs, T = `--steps` steps per batch, a 40-64-64-2 tanh policy on both sides.
A seat is one more forward pass on a row made in place; LDS and occupancy are self-play's (79 040 B at 8 lanes per env, two workgroups
per CU).  Legs, each on an env of its own, each deterministic and with Gaussian heads:
  - collect (one seat), self-play (two seats);
  - team (3, 0): three seats, no opponent; team (3, 1): four seats; team (3, 3): six seats.
Device events around each window, a warm-up first, `--rounds` rounds of at least `--window` seconds in which the legs ALTERNATE
(a round runs every leg once, in order); medians: tools/bench_selfplay.py's method.  The file also states the expectation a seat was
designed to: with k seats in total,  t_team(k) <= 1.10 * (t_collect + (k - 1) * (t_selfplay - t_collect)),  all three times from this
run.  Nothing is asserted: the file records what was measured and whether the expectation held.

    python tools/bench_teamplay.py [--out profiles/r20_teamplay.txt]
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

# (name, seats in total, with an opponent, collect()'s seat keywords)
LEGS = [("collect", 1, False, {}), ("self-play", 2, True, {}), ("team (3, 0)", 3, False, dict(team=True)),
        ("team (3, 1)", 4, True, dict(team=True)), ("team (3, 3)", 6, True, dict(team=True, opponent_team=True))]


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
        raise SystemExit("bench_teamplay.py needs a GPU")
    from rsoccer_amd.vec import VecVSSEnv
    from rsoccer_amd.vec.policy import MLPPolicy
    n, T = args.envs, args.steps
    head = (f"# tools/bench_teamplay.py: {torch.cuda.get_device_name(0)}, VSS-v0, num_envs {n}, T = {T} steps per batch, 40-64-64-2 tanh policy "
            f"on both sides, {args.rounds} rounds of >= {args.window} s with the legs alternating, device events; unit: env-steps/s")
    with torch.no_grad():
        probe = VecVSSEnv(1, device=0, seed=1)
        pol = MLPPolicy(probe.sim.obs_dim, probe.sim.act_dim)
        dev = probe.device
        probe.close()
        gen = torch.Generator().manual_seed(0)
        draw = lambda: ((torch.rand(pol.num_params, generator=gen) * 2 - 1) / 8.0).to(dev)   # noqa: E731  (torch's default Linear scale)
        params, opp = draw(), draw()
        log_std = torch.full((pol.act_dim,), -0.5, device=dev)
        envs, legs = [], []

        def leg(has_opp, kw, noisy):
            env = VecVSSEnv(n, device=0, seed=1)
            env.reset()
            envs.append(env)
            more = dict(opponent=pol, opponent_params=opp, **kw) if has_opp else dict(kw)
            count = [0]

            def run():
                if not noisy:
                    return env.collect(pol, params, T, **more)
                count[0] += 1
                heads = dict(opponent_log_std=log_std) if has_opp else {}
                return env.collect(pol, params, T, log_std=log_std, iteration=count[0], **heads, **more)
            return run

        for noisy in (False, True):
            for name, k, has_opp, kw in LEGS:
                legs.append((name + (", Gaussian heads" if noisy else ", deterministic"), k, noisy, leg(has_opp, kw, noisy)))
        reps = [_reps(torch, fn, args.window) for *_, fn in legs]
        times = [[] for _ in legs]
        for _ in range(args.rounds):
            for i, (*_, fn) in enumerate(legs):
                times[i].append(_window(torch, fn, reps[i]))
    med = [statistics.median(t) for t in times]
    lines = [head, "%-30s | %5s | %12s | %11s | %s" % ("leg", "seats", "env-steps/s", "us / batch", "rounds (us / batch)")]
    rows = {}
    for (name, k, _, _), m, ts in zip(legs, med, times):
        rows[name] = dict(seats=k, steps_per_s=n * T / m, us_per_batch=m * 1e6, rounds_us=[x * 1e6 for x in ts])
        lines.append("%-30s | %5d | %12.4g | %11.1f | %s" % (name, k, n * T / m, m * 1e6, " ".join("%.1f" % (x * 1e6) for x in ts)))
    for tag in (", deterministic", ", Gaussian heads"):
        tc, ts = rows["collect" + tag]["us_per_batch"], rows["self-play" + tag]["us_per_batch"]
        lines.append("%s: one more seat costs t_selfplay - t_collect = %.1f us / batch; self-play / collect %.3f" % (tag[2:], ts - tc, tc / ts))
        for name, k, *_ in LEGS[2:]:
            t = rows[name + tag]["us_per_batch"]
            model = tc + (k - 1) * (ts - tc)
            rows[name + tag].update(model_us=model, ratio_to_model=t / model, within_bound=bool(t <= 1.10 * model))
            lines.append("  %-12s k = %d: %.1f us against t_collect + (k - 1) * (t_selfplay - t_collect) = %.1f us: ratio %.3f (expected <= 1.10: %s); "
                         "throughput / collect %.3f" % (name, k, t, model, t / model, "held" if t <= 1.10 * model else "MISSED", tc / t))
    print("\n".join(lines), flush=True)
    for e in envs:
        e.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"teamplay_bench": rows}))


if __name__ == "__main__":
    main()
