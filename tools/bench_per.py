#!/usr/bin/env python
"""Time of prioritised and n-step replay on the device (rsoccer_amd/csrc/rsx_replay.hip through PrioritizedReplayBuffer) next to what it
replaces and what it is added to.

Needs a GPU and fails without one.  VSS-v0 shapes (obs 40, action 2), rings of `--capacities` rows filled with synthetic transitions
(the calls' cost does not depend on the values), minibatches of `--rows` rows.  In one run:
  1  sample + update_priorities against ReplayBuffer.sample_rows_device alone (the uniform draw it replaces);
  2  the same against the torch restatement a user would write — priorities in a tensor, cumsum + searchsorted over stratified targets,
     pow for the weights and the new priorities, indexed assignment — eager and replayed from a graph;
  3  add() with n_step = 3 on a [T, 4096] batch (T = capacity / 4096, at most 128) against ReplayBuffer.add and against a torch n-step
     fold (masked shifts, then the same index_copy_ calls);
  4  one whole piecewise gradient step — draw, gradients, optimiser step — with and without prioritisation, for TD3 and SAC, replayed
     from a graph: what share of the step the bookkeeping costs.
Device events around each window, a warm-up first, `--rounds` interleaved rounds of at least `--window` seconds; medians and spread
(min - max over the rounds; two legs' rounds overlap when their spreads do, which each comparison states).

    python tools/bench_per.py [--out profiles/r26_per.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_dpg_update import _graph  # noqa: E402
from bench_policy_lookahead import _reps, _window  # noqa: E402

GAMMA, ALPHA, BETA, EPS, LR, TAU, OD, AD = 0.99, 0.6, 0.4, 1e-6, 3e-4, 0.005, 40, 2


def synthetic_batch(torch, T, B, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)   # noqa: E731
    return {"obs": r(T, B, OD), "actions": r(T, B, AD).tanh(), "reward": r(T, B), "final_obs": r(T, B, OD), "next_obs": r(B, OD),
            "terminated": torch.rand(T, B, generator=g, device=dev) < 0.01, "truncated": torch.rand(T, B, generator=g, device=dev) < 0.01}


def torch_fold(torch, batch, n_step, gamma):
    """the n-step transitions of a [T, B] batch in torch: n_step - 1 masked shifts, then two gathers for the successor"""
    r, term = batch["reward"], batch["terminated"]
    done = term | batch["truncated"]
    T, B = r.shape
    R, g = r.clone(), torch.full_like(r, gamma)
    last = torch.arange(T, device=r.device)[:, None].expand(T, B).clone()
    alive = ~done
    for k in range(1, n_step):
        ext = alive.clone()
        ext[T - k:] = False
        R = torch.where(ext, R + g * torch.roll(r, -k, 0), R)
        g = torch.where(ext, g * gamma, g)
        last = last + ext
        alive = ext & ~torch.roll(done, -k, 0)
    ended = done.gather(0, last)
    following = torch.cat([batch["obs"][1:], batch["next_obs"][None]], 0)
    at = last[..., None].expand(T, B, OD)
    succ = torch.where(ended[..., None], batch["final_obs"].gather(0, at), following.gather(0, at))
    return R, g, term.gather(0, last), succ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacities", type=int, nargs="+", default=[65536, 524288])
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 4096], help="rows of the minibatches")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1, help="seconds of work per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_per.py needs a GPU")
    from rsoccer_amd.vec import VecVSSEnv
    from rsoccer_amd.vec.optim import DPGOptimizer, SACOptimizer
    from rsoccer_amd.vec.policy import MLPGaussianPolicy, MLPPolicy, MLPQCritic
    from rsoccer_amd.vec.replay import PrioritizedReplayBuffer, ReplayBuffer
    env = VecVSSEnv(64, device=0, seed=1)   # the gradient calls need its handle only
    dev = env.device
    assert (env.sim.obs_dim, env.sim.act_dim) == (OD, AD)
    lines = [f"# tools/bench_per.py: {torch.cuda.get_device_name(0)}, VSS-v0 shapes (obs {OD}, action {AD}), alpha {ALPHA}, beta {BETA}, "
             f"{args.rounds} interleaved rounds of >= {args.window} s, device events; unit: us per call of the leg"]
    result = {}

    def run(title, legs):
        """legs: [(name, fn)]; every round visits every leg; returns {name: median us}"""
        reps = [_reps(torch, fn, args.window) for _, fn in legs]
        times = [[] for _ in legs]
        for _ in range(args.rounds):
            for i, (_, fn) in enumerate(legs):
                times[i].append(_window(torch, fn, reps[i]) * 1e6)
        lines.append("")
        lines.append(title)
        lines.append("%-64s | %10s | %19s | %s" % ("leg", "us", "spread (min - max)", "rounds (us)"))
        med = {}
        for (name, _), ts in zip(legs, times):
            med[name] = statistics.median(ts)
            result[title + " / " + name] = dict(us=med[name], rounds_us=ts)
            lines.append("%-64s | %10.1f | %8.1f - %8.1f | %s" % (name, med[name], min(ts), max(ts), " ".join("%.1f" % x for x in ts)))
        spread = {name: (min(ts), max(ts)) for (name, _), ts in zip(legs, times)}
        return med, spread

    def versus(med, spread, a, b):
        over = spread[a][0] <= spread[b][1] and spread[b][0] <= spread[a][1]
        lines.append("%s against %s: %.2f x (%+.1f us); rounds %s" % (a, b, med[a] / med[b], med[a] - med[b], "overlap" if over else "do not overlap"))

    for cap in args.capacities:
        T = min(cap // 4096, 128)
        batch = synthetic_batch(torch, T, 4096, dev, cap)
        per = PrioritizedReplayBuffer(cap, OD, AD, dev, alpha=ALPHA, n_step=3, gamma=GAMMA, eps=EPS)
        for _ in range(cap // (T * 4096)):
            per.add(batch)
        torch.cuda.synchronize()
        assert int(per.fill) == cap
        for M in args.rows:
            g = torch.Generator(device=dev).manual_seed(M)
            td = torch.randn(M, generator=g, device=dev)
            per.update_priorities(torch.randint(0, cap, (cap // 4,), generator=g, device=dev, dtype=torch.int32),
                                  torch.randn(cap // 4, generator=g, device=dev))   # a spread of priorities
            prio = per.priorities().clone()
            ar = torch.arange(M, device=dev, dtype=torch.float32)

            def ours():
                rows, w = per.sample(M, beta=BETA, seed=1, step=0)
                per.update_priorities(rows, td)
                return rows, w

            def restated():
                cs = torch.cumsum(prio, 0)
                total = cs[-1]
                u = (ar + torch.rand(M, device=dev)) * (total / M)
                rows = torch.searchsorted(cs, u).clamp_(max=cap - 1)
                w = (cap * prio[rows] / total).pow(-BETA)
                w = w / w.max()
                prio[rows] = (td.abs() + EPS).pow(ALPHA)
                return rows, w

            legs = [("uniform: sample_rows_device", lambda: per.sample_rows_device(M, seed=1, step=0)),
                    ("sample + update_priorities, eager", ours),
                    ("sample + update_priorities, graph replay", _graph(torch, ours).replay),
                    ("torch cumsum + searchsorted + pow + assignment, eager", restated),
                    ("torch cumsum + searchsorted + pow + assignment, graph replay", _graph(torch, restated).replay)]
            med, spread = run(f"1-2  ring of {cap} rows ({per.tree_levels} tree levels), minibatch of {M} rows", legs)
            versus(med, spread, legs[1][0], legs[0][0])
            versus(med, spread, legs[1][0], legs[3][0])
            versus(med, spread, legs[2][0], legs[4][0])
        # 3: the add
        plain = ReplayBuffer(cap, OD, AD, dev)
        ring = ReplayBuffer(cap, OD, AD, dev)
        disc = torch.zeros(cap, device=dev)
        n = T * 4096

        def torch_add():
            R, gk, term, succ = torch_fold(torch, batch, 3, GAMMA)
            at = (ring.head + torch.arange(n, device=dev)) % cap
            ring.obs.index_copy_(0, at, batch["obs"].reshape(n, OD))
            ring.actions.index_copy_(0, at, batch["actions"].reshape(n, AD))
            ring.reward.index_copy_(0, at, R.reshape(n))
            disc.index_copy_(0, at, gk.reshape(n))
            ring.next_obs.index_copy_(0, at, succ.reshape(n, OD))
            ring.terminated.index_copy_(0, at, term.reshape(n))
            ring.head.copy_((ring.head + n) % cap)
            ring.fill.copy_(torch.clamp(ring.fill + n, max=cap))

        legs = [("PrioritizedReplayBuffer.add, n_step = 3 (fold + max-priority write)", lambda: per.add(batch)),
                ("ReplayBuffer.add (one step, torch)", lambda: plain.add(batch)),
                ("torch n-step fold + index_copy_", torch_add)]
        med, spread = run(f"3  add of a [{T}, 4096] batch ({n} rows) into a ring of {cap} rows", legs)
        versus(med, spread, legs[0][0], legs[1][0])
        versus(med, spread, legs[0][0], legs[2][0])
        # 4: one whole piecewise gradient step with and without prioritisation
        data = per.data()
        data_plain = {k: v for k, v in data.items() if k != "discount"}
        torch.manual_seed(0)
        for algo in ("TD3", "SAC"):
            for M in args.rows:
                def step_leg(with_per, algo=algo, M=M):
                    qnet = MLPQCritic(OD, AD)
                    pc = (0.1 * torch.randn(2, qnet.num_params)).to(dev)
                    tc = pc.clone()
                    if algo == "TD3":
                        pol = MLPPolicy(OD, AD, out_act="tanh")
                        pa = (0.1 * torch.randn(pol.num_params)).to(dev)
                        ta = pa.clone()
                        opt = DPGOptimizer(pol, qnet, 2, device=dev, lr_actor=LR, lr_critic=LR, tau=TAU)
                    else:
                        pol = MLPGaussianPolicy(OD, AD, hidden=64, layers=2, hidden_act="tanh")
                        pa = (0.1 * torch.randn(pol.num_params)).to(dev)
                        la = torch.zeros(1, device=dev)
                        opt = SACOptimizer(pol, qnet, 2, device=dev, lr_actor=LR, lr_critic=LR, lr_alpha=LR, tau=TAU)

                    def fn():
                        if with_per:
                            rows, w = per.sample(M, beta=BETA, seed=1, step=opt.steps)
                            kw = dict(rows=rows, weights=w, return_td_error=True)
                        else:
                            kw = dict(rows=per.sample_rows_device(M, seed=1, step=opt.steps))
                        d = data if with_per else data_plain
                        if algo == "TD3":
                            out = env.dpg_gradient(d, pol, pa, ta, qnet, pc, tc, gamma=GAMMA, target_noise=0.2, noise_clip=0.5, noise_seed=1,
                                                   noise_step=opt.steps, **kw)
                            opt.step(pa, ta, pc, tc, out["grad_params"], out["grad_critic_params"])
                        else:
                            out = env.sac_gradient(d, pol, pa, qnet, pc, tc, la, gamma=GAMMA, noise_seed=1, noise_step=opt.steps, **kw)
                            opt.step(pa, pc, tc, la, out["grad_params"], out["grad_critic_params"], out["grad_log_alpha"])
                        if with_per:
                            per.update_priorities(kw["rows"], out["td_error"])
                        return out
                    return fn
                legs = [("uniform rows + gradients + optimiser step, graph replay", _graph(torch, step_leg(False)).replay),
                        ("prioritised: sample + weighted gradients + step + update, replay", _graph(torch, step_leg(True)).replay)]
                med, spread = run(f"4  {algo}, one piecewise gradient step, ring of {cap} rows, minibatch of {M} rows", legs)
                versus(med, spread, legs[1][0], legs[0][0])
    print("\n".join(lines), flush=True)
    env.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"per_bench": result}))


if __name__ == "__main__":
    main()
