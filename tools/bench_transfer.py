#!/usr/bin/env python
"""Time per call of the episode transfer (env.copy_envs_from -> rsx_task_transfer, rsoccer_amd/csrc/rsx_xfer.hip) next to the two
things it can be compared with.

Needs a GPU and fails without one.  Per (task, num_envs):
  - identity:    every env of one handle into the same env of another (one launch, consecutive ids on both sides);
  - permutation: a random permutation on ONE handle (gather launch into the staging buffer + scatter launch);
  - resample:    a multinomial resample (source ids drawn with replacement) on one handle, identity destination;
  - checkpoint:  checkpoint() + restore() of one handle — the only route before the transfer existed (through the host, synchronous);
  - d2d copy:    one plain device-to-device copy (torch `copy_`) of as many bytes as the identity transfer reads.
All sides are timed between device events after a warm-up, in `--rounds` interleaved rounds of at least `--window` seconds each
(the checkpoint route: at least 2 calls); a row gives the median round and the spread (min - max).  `TB/s` counts the bytes read
plus the bytes written (2 x bytes per env x envs, from the row counts: kept here, next to the timing) over the call time — the
unit of the 6.29 TB/s a float4 streaming copy reaches on this chip (MI355X_MICROARCH: HBM3E measured).  Call times include the
launch overhead: at 4096 envs they measure that, not bandwidth.

    python tools/bench_transfer.py [--out profiles/r08_transfer.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_TBS = 6.29


def _window(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def _reps(torch, fn, window, least=3):
    for _ in range(2):   # warm-up: code objects, allocator, the staging buffer
        fn()
    torch.cuda.synchronize()
    t = _window(torch, fn, 2)
    return max(least, int(window / max(t, 1e-7)) + 1)


def bytes_per_env(env):
    """what one transferred env reads (and writes): state rows, scalar arena, obs and final_obs rows, two flag bytes, physics rows"""
    sim = env.sim
    rows = (sim.state_dim + 2) + (15 + 2 * sim.n_robots) + (32 if env._physics else 0)   # rsx_params.hpp: aux_rows
    return 4 * rows + 2 * 4 * sim.obs_dim + 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", nargs="+", default=["VecVSSEnv", "VecSSLStaticDefendersEnv"])
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 1 << 20])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of work per timed window")
    ap.add_argument("--warm-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_transfer.py needs a GPU")
    from rsoccer_amd import vec
    dev = torch.device("cuda", 0)
    lines = [f"# tools/bench_transfer.py: {torch.cuda.get_device_name(0)}, {args.rounds} interleaved rounds of >= {args.window} s, device events; "
             f"us per call, median (min - max); TB/s = (bytes read + bytes written) / median; streaming copy on this chip: {STREAM_TBS} TB/s",
             "%-26s %8s %6s | %-12s %28s %8s %9s" % ("task", "envs", "B/env", "case", "us per call", "TB/s", "x d2d")]
    print("\n".join(lines), flush=True)
    rows = []
    for name in args.tasks:
        for B in args.envs:
            env = getattr(vec, name)(B, device=0, seed=1)
            env.reset()
            env.step_random(args.warm_steps)
            other = env.fork(seed=2)
            bpe = bytes_per_env(env)
            moved = 2 * bpe * B
            g = torch.Generator(device=dev).manual_seed(B)
            perm = torch.randperm(B, device=dev, generator=g).to(torch.int32)
            draw = torch.randint(0, B, (B,), device=dev, generator=g).to(torch.int32)
            x = torch.empty(bpe * B // 4, dtype=torch.float32, device=dev).normal_()
            y = torch.empty_like(x)
            blob = [None]

            def ckpt():
                blob[0] = env.checkpoint()
                env.restore(blob[0])

            cases = [
                ("identity", lambda: other.copy_envs_from(env), 3),
                ("permutation", lambda: env.copy_envs_from(env, src_ids=perm), 3),
                ("resample", lambda: env.copy_envs_from(env, src_ids=draw), 3),
                ("d2d copy", lambda: y.copy_(x), 3),
                ("checkpoint", ckpt, 2),
            ]
            reps = {c: _reps(torch, fn, args.window, least) for c, fn, least in cases}
            times = {c: [] for c, _, _ in cases}
            for _ in range(args.rounds):
                for c, fn, _ in cases:
                    times[c].append(_window(torch, fn, reps[c]))
            assert env.sim.task_transfer_errors() == 0 and other.sim.task_transfer_errors() == 0
            med = {c: statistics.median(t) for c, t in times.items()}
            for c, _, _ in cases:
                t = times[c]
                tbs = moved / med[c] * 1e-12
                line = "%-26s %8d %6d | %-12s %10.1f (%8.1f - %8.1f) %8.3f %9.2f" % (
                    name, B, bpe, c, med[c] * 1e6, min(t) * 1e6, max(t) * 1e6, tbs, med[c] / med["d2d copy"])
                lines.append(line)
                print(line, flush=True)
                rows.append(dict(task=name, num_envs=B, bytes_per_env=bpe, case=c, us_median=med[c] * 1e6, us_rounds=[v * 1e6 for v in t],
                                 reps=reps[c], tb_per_s=tbs, share_of_streaming_copy=tbs / STREAM_TBS, times_d2d=med[c] / med["d2d copy"]))
            env.close(); other.close()
            del env, other, x, y, perm, draw
            torch.cuda.empty_cache()
    if args.out and rows:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"transfer_bench": rows}))


if __name__ == "__main__":
    main()
