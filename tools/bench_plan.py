#!/usr/bin/env python
"""One planning iteration two ways: candidates materialised by torch and scored by env.lookahead (what the engine offered before),
against env.plan (rsx_task_lookahead_sampled + rsx_plan_update, rsoccer_amd/csrc/rsx_plan_sampled.hip: candidates drawn in registers).

Needs a GPU and fails without one.  Per row (task, K candidates, H steps, hold; num_envs envs), four things are timed between device
events, after a warm-up, in `--rounds` interleaved rounds (a, b, c, d, a, b, ...) of at least `--window` seconds each; the row reports
the median round of each in microseconds per call:
  (a) materialised iteration: torch.randn [num_envs, K, ceil(H / hold), act_dim] held for `hold` steps, mean + sigma * noise, clamp,
      env.lookahead, then the update in torch — softmax((R - max R) / temperature)-weighted mean over the candidate tensor (or, with
      --temperature 0, argmax and a gather of the best row);
  (b) sampled iteration: env.plan with the same K, H, hold, sigma, temperature — two launches, no candidate tensor;
  (c) env.lookahead alone on pre-materialised actions;
  (d) rsx_task_lookahead_sampled alone (the first launch of (b)).
`b/a` and `d/c` are time ratios (below 1: the sampled side is faster); `cand MB` is the size of the tensor path (a) writes and reads.
The two paths draw different noise (torch's generator against the engine's Philox), so their returns are equal in distribution, not
in value; what (b) computes is pinned by tests/test_gpu_plan.py.

    python tools/bench_plan.py [--out profiles/r09_plan.txt]
    python tools/bench_plan.py --tasks VecVSSEnv --K 64 --hold 1 --profile-target   # launches alone, for rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_lookahead import _reps, _window   # noqa: E402  (the same timing windows as the lookahead's bench)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", nargs="+", default=["VecVSSEnv", "VecSSLStaticDefendersEnv"])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--K", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--H", type=int, default=20)
    ap.add_argument("--hold", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--temperature", type=float, default=0.5)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of work per timed window")
    ap.add_argument("--warm-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-target", action="store_true", help="20 calls of each side per row, no timing")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_plan.py needs a GPU")
    from rsoccer_amd import vec
    dev = torch.device("cuda", 0)
    H, sigma, temp, gamma = args.H, args.sigma, args.temperature, args.gamma
    lines = [f"# tools/bench_plan.py: {torch.cuda.get_device_name(0)}, num_envs {args.envs}, H {H}, sigma {sigma}, temperature {temp}, "
             f"{args.rounds} interleaved rounds of >= {args.window} s, device events; unit: us per call (median round)",
             "%-26s %5s %4s %8s | %13s %11s %6s | %13s %11s %6s" % ("task", "K", "hold", "cand MB", "(a) torch+look", "(b) plan", "b/a",
                                                                     "(c) lookahead", "(d) sampled", "d/c")]
    print("\n".join(lines), flush=True)
    rows = []
    for name in args.tasks:
        env = getattr(vec, name)(args.envs, device=0, seed=1)
        env.reset()
        env.step_random(args.warm_steps)
        B, AD = env.num_envs, env.sim.act_dim
        mean = torch.zeros(B, H, AD, device=dev)
        idx = torch.arange(B, device=dev)
        g = torch.Generator(device=dev).manual_seed(7)
        for K in args.K:
            for hold in args.hold:
                segs = (H + hold - 1) // hold

                def materialise():
                    eps = torch.randn(B, K, segs, AD, device=dev, generator=g)
                    if hold > 1:
                        eps = eps.repeat_interleave(hold, dim=2)[:, :, :H]
                    cand = (mean[:, None] + sigma * eps).clamp_(-1.0, 1.0)
                    cand[:, 0] = mean.clamp(-1.0, 1.0)
                    return cand

                def torch_iteration():
                    cand = materialise()
                    ret = env.lookahead(cand, gamma=gamma)["return"]
                    if temp > 0:
                        w = torch.softmax((ret - ret.max(dim=1, keepdim=True).values) / temp, dim=1)
                        return (w[:, :, None, None] * cand).sum(dim=1)
                    return cand[idx, ret.argmax(dim=1)]

                def plan_iteration():
                    return env.plan(mean=mean, K=K, sigma=sigma, hold=hold, temperature=temp, gamma=gamma)["mean"]

                fixed = materialise()
                smp = env._plan_sampler(sigma, hold, None, 0)
                ret = torch.empty(B, K, device=dev)
                steps = torch.empty(B, K, dtype=torch.int32, device=dev)
                flags = torch.empty(B, K, dtype=torch.uint8, device=dev)
                look_alone = lambda: env.lookahead(fixed, gamma=gamma)
                sampled_alone = lambda: env.sim.task_lookahead_sampled(mean.data_ptr(), smp, K, H, gamma, ret.data_ptr(), steps.data_ptr(),
                                                                       flags.data_ptr(), None, env._stream())
                sides = (torch_iteration, plan_iteration, look_alone, sampled_alone)
                if args.profile_target:
                    for _ in range(20):
                        for fn in sides:
                            fn()
                    torch.cuda.synchronize()
                    continue
                reps = [_reps(torch, fn, args.window) for fn in sides]
                times = [[] for _ in sides]
                for _ in range(args.rounds):
                    for t, fn, r in zip(times, sides, reps):
                        t.append(_window(torch, fn, r))
                a, b, c, d = (statistics.median(t) * 1e6 for t in times)
                mb = B * K * H * AD * 4 / 1e6
                row = dict(task=name, num_envs=B, K=K, H=H, hold=hold, sigma=sigma, temperature=temp, candidate_tensor_mb=mb,
                           torch_iteration_us=a, plan_iteration_us=b, lookahead_alone_us=c, sampled_alone_us=d,
                           rounds_us=[[x * 1e6 for x in t] for t in times])
                rows.append(row)
                line = "%-26s %5d %4d %8.1f | %13.1f %11.1f %6.2f | %13.1f %11.1f %6.2f" % (name, K, hold, mb, a, b, b / a, c, d, d / c)
                lines.append(line)
                print(line, flush=True)
                del fixed
                torch.cuda.empty_cache()
        env.close()
    if args.out and rows:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"plan_bench": rows}))


if __name__ == "__main__":
    main()
