#!/usr/bin/env python
"""Throughput of the batched renderer (env.render -> rsx_render, rsoccer_amd/csrc/rsx_render.hip).

Needs a GPU and fails without one.  Per shape: bytes written (n * H * W * 3, from the shapes), time per launch between device events
over `--launches` launches after a warm-up, bytes per second, and three yardsticks measured in the same run:
  - torch `fill_` of the same output tensor (a store stream without arithmetic: the floor for this kernel on the box at hand);
  - the 6.29 TB/s a float4 copy streams on an MI355X, as the share of achievable bandwidth;
  - what a user did before: `env.state` to the host + one `FieldRaster.draw` per env on one CPU core (timed on 32 envs, per frame).

    python tools/bench_render.py [--launches 200] [--out profiles/render_throughput.md]
    python tools/bench_render.py --profile-target          # the launches alone, for rocprofv3 --kernel-trace --stats -- python ...
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_BW = 6.29e12   # bytes/s, measured float4 copy on an MI355X (79 % of the 8 TB/s HBM3E peak)

# (env class, envs, scale)
SHAPES = (("VecVSSEnv", 4096, 64), ("VecVSSEnv", 4096, 128), ("VecVSSEnv", 256, 500), ("VecSSLStaticDefendersEnv", 2048, 20))


def _time(torch, fn, warmup, launches, rounds=3):
    """median over `rounds` of the mean time of `launches` calls between two device events, seconds"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / launches)
    return sorted(out)[len(out) // 2], min(out), max(out)


def _cpu_per_frame(env, scale, vss):
    """env.state -> host + FieldRaster.draw per env, on 32 envs: seconds per frame"""
    from types import SimpleNamespace as NS
    from rsoccer_amd.Render import SSL_VIEW, VSS_VIEW, FieldRaster
    rs, nb, ny = (6 if vss else 11), env.sim.n_blue, env.sim.n_yellow

    def frame(st, e):
        rb = [NS(x=float(st[5 + rs * k, e]), y=float(st[6 + rs * k, e]), theta=float(st[7 + rs * k, e])) for k in range(nb + ny)]
        return NS(ball=NS(x=float(st[0, e]), y=float(st[1, e])), robots_blue=dict(enumerate(rb[:nb])), robots_yellow=dict(enumerate(rb[nb:])))
    fr = FieldRaster(dict(VSS_VIEW if vss else SSL_VIEW, scale=scale))
    t0 = time.perf_counter()
    st = env.state[:, :32].cpu().numpy()
    for e in range(32):
        fr.draw(frame(st, e))
    return (time.perf_counter() - t0) / 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="write the table (markdown) here")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU rasteriser yardstick (A/B legs of layout variants: RSX_LIB=...)")
    ap.add_argument("--profile-target", action="store_true", help="only launch every shape (to be run under rocprofv3)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_render.py needs a GPU: there is nothing to measure without one")
    if args.launches < 200 and not args.profile_target:
        sys.exit("--launches must be at least 200")
    from rsoccer_amd import vec
    rows = []
    for cls, n, scale in SHAPES:
        env = getattr(vec, cls)(n, seed=1)
        env.reset()
        env.step_random(50)
        vss = cls == "VecVSSEnv"
        H, W = env.render_shape(scale=scale)
        nbytes = n * H * W * 3
        cpu = float('nan') if args.profile_target or args.no_cpu else _cpu_per_frame(env, scale, vss)
        for cf in (False, True):
            out = torch.empty((n, 3, H, W) if cf else (n, H, W, 3), dtype=torch.uint8, device=env.device)
            fn = lambda: env.render(scale=scale, channels_first=cf, out=out)   # noqa: E731
            if args.profile_target:
                for _ in range(50):
                    fn()
                torch.cuda.synchronize()
                continue
            t, lo, hi = _time(torch, fn, args.warmup, args.launches)
            tf, _, _ = _time(torch, lambda: out.fill_(0), args.warmup, args.launches)
            rows.append(dict(env=cls, envs=n, scale=scale, H=H, W=W, layout="CHW" if cf else "HWC", bytes=nbytes,
                             us=t * 1e6, us_min=lo * 1e6, us_max=hi * 1e6, tb_s=nbytes / t / 1e12, fill_us=tf * 1e6,
                             vs_fill=t / tf, share_of_stream=nbytes / t / STREAM_BW, cpu_ms_per_frame=cpu * 1e3,
                             frames_per_s=n / t, speedup_vs_cpu=cpu / (t / n)))
            print(json.dumps(rows[-1]), flush=True)
        env.close()
    if args.profile_target or not rows:
        return
    lines = ["| env | envs | scale | H x W | layout | MB written | us / launch (min - max) | TB/s | fill_ us | render / fill_ | share of 6.29 TB/s | CPU raster ms / frame | frames / s | vs CPU |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['env']} | {r['envs']} | {r['scale']} | {r['H']} x {r['W']} | {r['layout']} | {r['bytes'] / 1e6:.1f} | "
                     f"{r['us']:.1f} ({r['us_min']:.1f} - {r['us_max']:.1f}) | {r['tb_s']:.2f} | {r['fill_us']:.1f} | {r['vs_fill']:.2f} | "
                     f"{100 * r['share_of_stream']:.0f} % | {r['cpu_ms_per_frame']:.2f} | {r['frames_per_s']:.3g} | {r['speedup_vs_cpu']:.3g} x |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
