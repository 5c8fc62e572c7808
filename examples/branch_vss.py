#!/usr/bin/env python
"""A branching search on VecVSSEnv: step, score, resample the envs by score, archive the best — all on the device.

The population is one VecVSSEnv.  Every step each env picks the first action of its best of K random candidate sequences
(env.lookahead, as in examples/mppi_vss.py).  Every `--resample` steps the envs are scored by that best return and RESAMPLED:
env i continues the episode of an env drawn with probability softmax(score / temperature) — env.copy_envs_from(env, src_ids=...),
one gather and one scatter launch, no host copy; the copies diverge at once because each keeps its own noise streams.  The best
env of each round is archived into a BANK, a sibling env made by env.fork() that is never stepped: it holds whole running
episodes (state, step count, noise state) on the device, can be scored with lookahead like any env, and at the end seeds a
fresh population (Go-Explore's "return, then explore").

    python examples/branch_vss.py [--envs 256] [--steps 400] [--K 32] [--H 10] [--resample 20] [--bank 16]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--H", type=int, default=10)
    ap.add_argument("--resample", type=int, default=20)
    ap.add_argument("--bank", type=int, default=16)
    ap.add_argument("--temperature", type=float, default=0.5)
    ap.add_argument("--gamma", type=float, default=0.98)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    from rsoccer_amd import vec

    env = vec.VecVSSEnv(args.envs, device=0, seed=args.seed)
    env.reset()
    bank = env.fork(num_envs=args.bank, seed=args.seed + 1)   # already reset; never stepped
    B, AD, dev = env.num_envs, env.sim.act_dim, env.device
    rows = torch.arange(B, device=dev)
    g = torch.Generator(device=dev).manual_seed(args.seed)
    banked, bank_score = 0, torch.full((args.bank,), float("-inf"), device=dev)
    for t in range(1, args.steps + 1):
        cand = torch.rand(B, args.K, args.H, AD, device=dev, generator=g) * 2 - 1
        ret = env.lookahead(cand, gamma=args.gamma)["return"]
        score, best = ret.max(dim=1)
        env.step(cand[rows, best, 0])
        if t % args.resample == 0:
            # archive the round's best env: one pair, env -> slot of the bank (round robin)
            top = score.argmax().to(torch.int32).reshape(1)
            slot = torch.tensor([banked % args.bank], dtype=torch.int32, device=dev)
            bank.copy_envs_from(env, src_ids=top, dst_ids=slot)
            bank_score[banked % args.bank] = score[top.long()].squeeze()
            banked += 1
            # resample the population by score: sources drawn with replacement, identity destination
            p = torch.softmax((score - score.max()) / args.temperature, dim=0)
            src = torch.multinomial(p, B, replacement=True, generator=g).to(torch.int32)
            env.copy_envs_from(env, src_ids=src)
            print(f"step {t:5d}  best {float(score.max()):7.3f}  mean {float(score.mean()):7.3f}  distinct sources {int(src.unique().numel()):4d} of {B}")
    m = env.metrics()
    n = max(m["episodes"], 1)
    print(f"population: {m['episodes']} episodes, goals for / episode {m['goals_for'] / n:.3f}, against {m['goals_against'] / n:.3f}")
    # the bank is an env like any other: score its states with a fresh set of candidates, then restart everything from the best one
    k = min(banked, args.bank)
    if k:
        cand = torch.rand(args.bank, args.K, args.H, AD, device=dev, generator=g) * 2 - 1
        again = bank.lookahead(cand, gamma=args.gamma)["return"].max(dim=1).values[:k]
        best = int(again.argmax())
        print(f"bank: {k} archived states, episode steps {bank._t['steps'][:k].tolist()}, scores when archived "
              f"{[round(float(v), 3) for v in bank_score[:k]]}, rescored {[round(float(v), 3) for v in again]}")
        env.copy_envs_from(bank, src_ids=[best] * B)          # broadcast: every env plays that state under its own noise stream
        env.step_random(args.H)
        print(f"restarted {B} envs from bank slot {best}; {args.H} random steps later they hold "
              f"{int(torch.unique(env.state[:2].T, dim=0).shape[0])} distinct ball positions")
    assert env.sim.task_transfer_errors() == 0 and bank.sim.task_transfer_errors() == 0
    env.close(); bank.close()


if __name__ == "__main__":
    main()
