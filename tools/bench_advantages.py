#!/usr/bin/env python
"""Time of values + GAE advantages of a collected batch in two launches (env.advantages -> rsx_task_advantages,
rsoccer_amd/csrc/rsx_gae.hip) next to the torch path it replaces.

Needs a GPU and fails without one.  VSS-v0, `--envs` envs, T = `--steps` steps per batch, a 40-64-64-1 tanh critic, one batch collected
up front and reused by every leg.  In one run:
  (a) advantages:        env.advantages on the batch, the default form of the values kernel (one row per lane); the same with
                         RSX_GAE_FORM=groups (eight lanes per row, the collector's policy_forward); and the values launch nearly alone
                         (the same rows presented as T = 1, B = T * B: the scan is one row per lane then), per form;
  (b) torch, eager:      the critic as a torch module on [T, B, obs_dim] and the Python loop over T of examples/ppo_vss.py before this call
                         existed (an ended row bootstraps nothing there: less work, in its favour);
  (c) torch, graph:      the same replayed from one graph — the fair opponent, launch overhead removed;
  (d) collect:           env.collect of such a batch, for scale.
Device events around each window, a warm-up first, `--rounds` interleaved rounds of at least `--window` seconds; medians and spread.
The values launch is set against its floor: 2 (OD H + H H + H) FLOP per row at the fp32 vector peak (157.3 TFLOP/s).

    python tools/bench_advantages.py [--out profiles/r13_advantages.txt]
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

PEAK_FP32 = 157.3e12


def _torch_path(torch, critic, batch, gamma, lam):
    """values, advantages and returns the way examples/ppo_vss.py computed them in torch"""
    T, B = batch["reward"].shape
    done = batch["terminated"] | batch["truncated"]
    values = critic(batch["obs"]).squeeze(-1)
    nxt = torch.cat([values[1:], critic(batch["next_obs"]).squeeze(-1)[None]])
    delta = batch["reward"] + gamma * nxt * (~done) - values
    adv = torch.zeros_like(delta)
    run = torch.zeros(B, device=delta.device)
    for t in reversed(range(T)):
        run = delta[t] + gamma * lam * (~done[t]) * run
        adv[t] = run
    return values, adv, adv + values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_advantages.py needs a GPU")
    from rsoccer_amd.vec import VecVSSEnv
    from rsoccer_amd.vec.policy import MLPCritic, MLPPolicy
    n, T, gamma, lam = args.envs, args.steps, 0.99, 0.95
    head = (f"# tools/bench_advantages.py: {torch.cuda.get_device_name(0)}, VSS-v0, num_envs {n}, T = {T}, 40-64-64-1 tanh critic, "
            f"{args.rounds} interleaved rounds of >= {args.window} s, device events; unit: us per batch")
    with torch.no_grad():
        env = VecVSSEnv(n, device=0, seed=1)
        env.reset()
        dev, OD = env.device, env.sim.obs_dim
        pol, critic = MLPPolicy(OD, env.sim.act_dim), MLPCritic(OD)
        gen = torch.Generator().manual_seed(0)
        params = ((torch.rand(pol.num_params, generator=gen) * 2 - 1) / 8.0).to(dev)   # scaled like torch's default Linear initialisation
        cparams = ((torch.rand(critic.num_params, generator=gen) * 2 - 1) / 8.0).to(dev)
        module = torch.nn.Sequential(torch.nn.Linear(OD, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1)).to(dev)
        torch.nn.utils.vector_to_parameters(cparams.clone(), module.parameters())
        log_std = torch.full((env.sim.act_dim,), -0.5, device=dev)
        batch = env.collect(pol, params, T, log_std=log_std, return_final_obs=True)
        batch["next_obs"] = batch["next_obs"].clone()   # (the legs below go on collecting: the batch keeps its own last observation)
        flat = {"obs": batch["obs"].reshape(1, T * n, OD), "reward": batch["reward"].reshape(1, T * n),
                "terminated": torch.zeros(1, T * n, dtype=torch.bool, device=dev), "truncated": torch.zeros(1, T * n, dtype=torch.bool, device=dev),
                "next_obs": batch["obs"].reshape(T * n, OD)}
        rows_flat = 2 * T * n   # (rows of that call: T * B of obs and as many of last_obs)
        torch.cuda.synchronize()

        def form(name, fn):
            def run():
                if name:
                    os.environ["RSX_GAE_FORM"] = name
                else:
                    os.environ.pop("RSX_GAE_FORM", None)
                return fn()
            return run

        # agreement first: the two forms give the same bits, torch's path the same numbers up to float32 and its missing bootstrap
        a = form(None, lambda: env.advantages(batch, critic, cparams, gamma, lam))()
        g = form("groups", lambda: env.advantages(batch, critic, cparams, gamma, lam))()
        tv, _, _ = _torch_path(torch, module, batch, gamma, lam)
        same = all(torch.equal(a[k].view(torch.int32), g[k].view(torch.int32)) for k in a)
        dev_v = float((a["value"] - tv).abs().max())

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _torch_path(torch, module, batch, gamma, lam)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            keep = _torch_path(torch, module, batch, gamma, lam)
        graph.keep = keep

        legs = [("(a) advantages, one row per lane", form(None, lambda: env.advantages(batch, critic, cparams, gamma, lam))),
                ("(a) advantages, eight lanes per row", form("groups", lambda: env.advantages(batch, critic, cparams, gamma, lam))),
                ("    values launch, one row per lane (2 T B rows)", form(None, lambda: env.advantages(flat, critic, cparams, gamma, lam))),
                ("    values launch, eight lanes per row (2 T B rows)", form("groups", lambda: env.advantages(flat, critic, cparams, gamma, lam))),
                ("(b) torch critic + Python GAE loop, eager", lambda: _torch_path(torch, module, batch, gamma, lam)),
                ("(c) the same, graph replay", graph.replay),
                ("(d) collect, Gaussian head, final_obs", lambda: env.collect(pol, params, T, log_std=log_std, return_final_obs=True))]
        reps = [_reps(torch, fn, args.window) for _, fn in legs]
        times = [[] for _ in legs]
        for _ in range(args.rounds):
            for i, (_, fn) in enumerate(legs):
                times[i].append(_window(torch, fn, reps[i]))
        os.environ.pop("RSX_GAE_FORM", None)
    lines = [head, "%-54s | %10s | %16s | %s" % ("leg", "us / batch", "spread (min-max)", "rounds (us / batch)")]
    rows = {}
    for (name, _), ts in zip(legs, times):
        m = statistics.median(ts)
        rows[name.strip()] = dict(us_per_batch=m * 1e6, rounds_us=[x * 1e6 for x in ts])
        lines.append("%-54s | %10.1f | %7.1f - %6.1f | %s" % (name, m * 1e6, min(ts) * 1e6, max(ts) * 1e6, " ".join("%.1f" % (x * 1e6) for x in ts)))
    flop_row = 2 * (OD * 64 + 64 * 64 + 64)
    for key in ("values launch, one row per lane (2 T B rows)", "values launch, eight lanes per row (2 T B rows)"):
        t = rows[key]["us_per_batch"] * 1e-6
        floor = rows_flat * flop_row / PEAK_FP32
        lines.append("%s: %d rows x %d FLOP = %.2f GFLOP, floor %.1f us at the fp32 vector peak, measured %.1f us = %.1f %% of peak "
                     "(instruction-bound: the activations, the LDS reads and the scan's launch are on top of the fmaf)" %
                     (key, rows_flat, flop_row, rows_flat * flop_row * 1e-9, floor * 1e6, t * 1e6, 100.0 * floor / t))
    a_us, c_us = rows["(a) advantages, one row per lane"], rows["(c) the same, graph replay"]
    lines.append("advantages against the graph replay of the torch path: %.2f x (medians); rounds overlap: %s" %
                 (c_us["us_per_batch"] / a_us["us_per_batch"], "yes" if max(a_us["rounds_us"]) >= min(c_us["rounds_us"]) else "no"))
    lines.append("the two forms agree bit for bit: %s; largest |value - torch's value|: %.3g" % (same, dev_v))
    print("\n".join(lines), flush=True)
    env.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"advantages_bench": rows}))


if __name__ == "__main__":
    main()
