#!/usr/bin/env python3
"""Times the two-piece lookahead in one kernel (VecTetris.lookahead on tetris_hip_policy_two_ply) against the path that
existed before it: VecTetris.two_ply_values -- one expand_from into a child batch of B * a_max envs and one
greedy_actions per piece of the set, plus torch glue -- followed by the bag-weighted mean and the argmax in torch.
10x20 and 10x40, the default pair and the standard seven, B = 32,768 parents (the yardstick's child batch is then about
1 Mi envs).

Yardstick and subject run interleaved, call by call, in one process on one start state; HIP events around every call,
median (min - max) of the repeats.  The ratio is quoted beside the yardstick's own spread.  The subject is also timed
alone at 1 Mi parents, where the yardstick cannot run at all: it would need a child batch of 36 Mi envs.
One JSON document.
usage: bench_two_ply.py [--envs N] [--big N] [--repeats N] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tetris_amd import VecTetris, _lib  # noqa: E402

STANDARD7 = ["Straight", "RCorner", "LCorner", "Square", "SnakeR", "SnakeL", "T"]
W = list(VecTetris.BCTS_WEIGHTS)


def stats(evs):
    ts = sorted(s.elapsed_time(e) for s, e in evs)
    return dict(ms=ts[len(ts) // 2], ms_min=ts[0], ms_max=ts[-1])


def timed(fn, evs):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    evs.append((s, e))
    return out


def yardstick(env):
    """the parent commit's path: the table through the child batch, then the mean over the bag and the pick in torch"""
    v = env.two_ply_values(W)
    P = v.shape[2]
    every = (1 << P) - 1
    bag = (env.meta >> 52) & every
    bag = torch.where(bag == 0, torch.full_like(bag, every), bag)
    inbag = ((bag[:, None] >> torch.arange(P, device=v.device)[None, :]) & 1).bool()
    total = torch.where(inbag[:, None, :], v, torch.zeros_like(v)).sum(dim=2)
    mean = total / inbag.sum(dim=1)[:, None]
    return torch.nan_to_num(mean, nan=-float("inf")).argmax(dim=1)


def played(rows, pieces, B):
    env = VecTetris(10, rows, B, device="cuda", pieces=pieces, auto_reset=True, seed=0)
    for _ in range(100):
        env.step()
    return env


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1 << 15)
    ap.add_argument("--big", type=int, default=1 << 20, help="parents of the subject-only run (0: skip it)")
    ap.add_argument("--repeats", type=int, default=51)
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_two_ply.py measures on the GPU: no device found")
    lib = _lib.load()
    rows_out = []
    for rows in (20, 40):
        for set_name, pieces in (("default", "default"), ("standard7", STANDARD7)):
            B = args.envs
            env = played(rows, pieces, B)
            subject = lambda: env.lookahead(W)
            for _ in range(3):
                ya = yardstick(env)
                sa, _ = subject()
            # the two paths pick the same action wherever the yardstick's float32 mean (torch's summation order) has
            # one maximum; the bit-exact comparison is the test-suite's
            alive = env.n_valid > 0
            agree = float((ya[alive] == sa[alive].long()).float().mean())
            ev_y, ev_s = [], []
            for _ in range(args.repeats):
                timed(lambda: yardstick(env), ev_y)
                timed(subject, ev_s)
            torch.cuda.synchronize()
            y, s = stats(ev_y), stats(ev_s)
            row = dict(board="10x%d" % rows, pieces=set_name, n_pieces=len(env.piece_names), a_max=env.a_max, parents=B,
                       child_envs_of_the_yardstick=B * env.a_max, launches_of_the_yardstick=2 * len(env.piece_names),
                       yardstick_two_ply_values_mean_argmax=y, subject_lookahead=s, speedup=y["ms"] / s["ms"],
                       speedup_over_the_yardsticks_fastest=y["ms_min"] / s["ms"],
                       yardstick_spread=(y["ms_max"] - y["ms_min"]) / y["ms"], actions_agree=agree)
            rows_out.append(row)
            print(json.dumps(row), flush=True)
            del env
            torch.cuda.empty_cache()
            if args.big:
                env = played(rows, pieces, args.big)
                for _ in range(3):
                    env.lookahead(W)
                ev = []
                for _ in range(args.repeats):
                    timed(lambda: env.lookahead(W), ev)
                torch.cuda.synchronize()
                s = stats(ev)
                row = dict(board="10x%d" % rows, pieces=set_name, n_pieces=len(env.piece_names), a_max=env.a_max,
                           parents=args.big, subject_lookahead=s, us_per_1k_parents=1e3 * s["ms"] / (args.big / 1e3),
                           yardstick="cannot run: its child batch would hold %d envs" % (args.big * env.a_max))
                rows_out.append(row)
                print(json.dumps(row), flush=True)
                del env
                torch.cuda.empty_cache()
    doc = dict(tool="tools/bench_two_ply.py", library_source_hash=lib.source_hash(), device=torch.cuda.get_device_name(0),
               repeats=args.repeats, rows=rows_out)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
