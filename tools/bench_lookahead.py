#!/usr/bin/env python
"""Throughput of the lookahead (env.lookahead -> rsx_task_lookahead, rsoccer_amd/csrc/rsx_plan.hip) against what a user could run
before it existed.

Needs a GPU and fails without one.  Per row (task, K candidates, H steps; num_envs envs):
  - lookahead: one launch that scores num_envs * K pairs over H steps from the envs' current state;
  - baseline:  the same number of env-steps as H fed `step(actions)` launches on a handle of num_envs * K envs — the cheapest
    way to buy that arithmetic with the stepping API (it does not answer the question: it cannot start K copies from one state).
Both are timed between device events, after a warm-up, in `--rounds` interleaved rounds (lookahead, baseline, lookahead, ...) of
at least `--window` seconds each; the row reports the median round of each side in candidate-env-steps/s = num_envs * K * H / time.
A pair whose episode ends inside the horizon idles from there on, so the row also gives the lookahead's rate over the steps it
really simulated (the sum of `steps`); `ratio` compares THAT rate with the baseline's, `nominal` the rate over num_envs * K * H.

    python tools/bench_lookahead.py [--out profiles/r07_lookahead.txt]
    python tools/bench_lookahead.py --tasks VecVSSEnv --K 64 --H 32 --profile-target   # launches alone, for rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _window(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def _reps(torch, fn, window):
    for _ in range(3):   # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    t = _window(torch, fn, 3)
    return max(3, int(window / max(t, 1e-6)) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", nargs="+", default=["VecVSSEnv", "VecSSLStaticDefendersEnv"])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--K", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--H", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of work per timed window")
    ap.add_argument("--warm-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-target", action="store_true", help="20 launches of each side per row, no timing")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lookahead.py needs a GPU")
    from rsoccer_amd import vec
    dev = torch.device("cuda", 0)
    lines = [f"# tools/bench_lookahead.py: {torch.cuda.get_device_name(0)}, num_envs {args.envs}, {args.rounds} interleaved rounds of >= {args.window} s, "
             "device events; unit: candidate-env-steps/s (num_envs * K * H / time)",
             "%-26s %4s %3s | %12s %12s %11s | %12s %11s | %6s %7s | %s" % ("task", "K", "H", "lookahead", "(simulated)", "us/launch", "baseline", "us/H steps",
                                                                               "ratio", "nominal", "pairs ended inside H")]
    print("\n".join(lines), flush=True)
    rows = []
    for name in args.tasks:
        env = getattr(vec, name)(args.envs, device=0, seed=1)
        env.reset()
        env.step_random(args.warm_steps)
        AD = env.sim.act_dim
        for K in args.K:
            base = getattr(vec, name)(args.envs * K, device=0, seed=2)
            base.reset()
            base.step_random(args.warm_steps)
            for H in args.H:
                g = torch.Generator(device=dev).manual_seed(K * 1000 + H)
                acts = torch.rand(args.envs, K, H, AD, device=dev, generator=g) * 2 - 1
                bacts = [torch.rand(args.envs * K, AD, device=dev, generator=g) * 2 - 1 for _ in range(min(H, 8))]
                look = lambda: env.lookahead(acts, gamma=0.99)

                def steps():
                    for t in range(H):
                        base.step(bacts[t % len(bacts)])

                if args.profile_target:
                    for _ in range(20):
                        look(); steps()
                    torch.cuda.synchronize()
                    continue
                rl, rb = _reps(torch, look, args.window), _reps(torch, steps, args.window)
                tl, tb = [], []
                for _ in range(args.rounds):
                    tl.append(_window(torch, look, rl))
                    tb.append(_window(torch, steps, rb))
                out = look()
                torch.cuda.synchronize()
                ended = float((out["steps"] < H).float().mean())
                n, sim = args.envs * K * H, int(out["steps"].sum())
                l, b = statistics.median(tl), statistics.median(tb)
                row = dict(task=name, num_envs=args.envs, K=K, H=H, lookahead_steps_per_s=n / l, lookahead_simulated_steps_per_s=sim / l, lookahead_us=l * 1e6,
                           baseline_steps_per_s=n / b, baseline_us=b * 1e6, ratio_simulated=(sim / l) / (n / b), ratio_nominal=b / l, ended_share=ended,
                           lookahead_rounds_us=[x * 1e6 for x in tl], baseline_rounds_us=[x * 1e6 for x in tb])
                rows.append(row)
                line = "%-26s %4d %3d | %12.4g %12.4g %11.1f | %12.4g %11.1f | %6.2f %7.2f | %.1f %%" % (
                    name, K, H, n / l, sim / l, l * 1e6, n / b, b * 1e6, (sim / l) / (n / b), b / l, 100 * ended)
                lines.append(line)
                print(line, flush=True)
            base.close()
            del base
            torch.cuda.empty_cache()
        env.close()
    if args.out and rows:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"lookahead_bench": rows}))


if __name__ == "__main__":
    main()
