#!/usr/bin/env python3
"""Times tetris_hip_play_linear (VecTetris.play's launch: K greedy steps of every env on its own weight row, totals
only) against tetris_hip_step_many(policy = 1) of the same library, at 1 Mi envs on 10x20 and 10x40, K = 20 steps per
launch.  Four cases, interleaved launch by launch in one process, each on its own copy of one start state:
  play_one_row        every env on row 0 of a [1, 8] matrix (the BCTS weights)
  play_1024_rows      P = 1024 rows (BCTS, each perturbed by 1 %), 1024 consecutive envs per row
  step_many_no_obs    step_many greedy on the BCTS weights, obs = NULL   <- the yardstick
  step_many_obs       the same with the [K][B][8] observation written
HIP events around windows of one launch, warm-up, median (min, max) of the repeats; ms per STEP.  The games run on
from launch to launch (no resets in play; step_many runs without auto-reset too): the share of envs still alive at
the end is reported, since a frozen env costs play nothing.  One JSON line per case.
usage: bench_play.py [--envs N] [--steps K] [--repeats N] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tetris_amd import VecTetris, _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_play.py measures on the GPU: no device found")
    B, K, dev = args.envs, args.steps, "cuda"
    lib = _lib.load()
    lines = []
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    for rows_, pieces in ((20, "default"), (40, "default")):
        start = VecTetris(10, rows_, B, device=dev, pieces=pieces, auto_reset=True, seed=0)
        for _ in range(30):
            start.step()
        start.auto_reset = False
        bcts = torch.tensor([VecTetris.BCTS_WEIGHTS], dtype=torch.float32, device=dev)
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        many = (bcts * (1 + 0.01 * torch.randn((1024, 8), device=dev, generator=g))).contiguous()
        block = torch.arange(B, dtype=torch.int32, device=dev) // 1024 % 1024
        zeros = torch.zeros(B, dtype=torch.int32, device=dev)

        def play_case(weights, index):
            env = start.fork(torch.arange(B, device=dev))
            tot = torch.zeros((2, B), dtype=torch.int32, device=dev)

            def launch():
                rc = lib.play_linear(ctypes.byref(env.desc), p(env.cols), p(env.meta), K, p(weights), weights.shape[0], p(index),
                                     p(tot[0]), p(tot[1]), p(env.n_valid), p(env.piece), p(env.status), env.seed, env.step_idx,
                                     env.env_offset, B, env._hip_stream())
                assert rc == 0, rc
                env.step_idx += K
            return env, launch

        def step_many_case(obs):
            env = start.fork(torch.arange(B, device=dev))
            env.compute_obs = obs
            box = [None]

            def launch():
                box[0] = env.step_many(K, policy="greedy", out=box[0])
            return env, launch

        cases = {"play_one_row": play_case(bcts, zeros), "play_1024_rows": play_case(many, block),
                 "step_many_no_obs": step_many_case(False), "step_many_obs": step_many_case(True)}
        for _ in range(args.warmup):
            for _, launch in cases.values():
                launch()
        evs = {name: [] for name in cases}
        for _ in range(args.repeats):
            for name, (_, launch) in cases.items():  # interleaved: every case sees the same drift of the device
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                launch()
                e.record()
                evs[name].append((s, e))
        torch.cuda.synchronize()
        yard = None
        out = {}
        for name in ("step_many_no_obs", "step_many_obs", "play_one_row", "play_1024_rows"):
            ts = sorted(s.elapsed_time(e) / K for s, e in evs[name])
            out[name] = (ts[len(ts) // 2], ts[0], ts[-1])
            yard = out[name] if name == "step_many_no_obs" else yard
        for name, (ms, lo, hi) in out.items():
            env = cases[name][0]
            row = dict(case=name, board="10x%d" % rows_, envs=B, steps_per_launch=K, launches=args.repeats, ms_per_step=ms,
                       ms_per_step_min=lo, ms_per_step_max=hi, over_step_many_no_obs=ms / yard[0],
                       step_many_no_obs_spread=(yard[2] - yard[1]) / yard[0], alive_share_at_end=float((env.n_valid > 0).float().mean()),
                       invalid=env.stats()["invalid"], library_source_hash=lib.source_hash())
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
        del cases, start
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
