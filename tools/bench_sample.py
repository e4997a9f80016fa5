#!/usr/bin/env python3
"""Times the softmax linear policy's kernels against their yardsticks of the same library, at 1 Mi envs on 10x20 and
10x40.  Five cases, interleaved launch by launch in one process, on copies of one start state, every env on row 0
of a [1, 8] matrix (the BCTS weights), temperature 1:
  policy_greedy_rows     one greedy decision per env                                  <- yardstick of the next
  policy_softmax_rows    one sampled decision per env with logp and score
  composed               what the kernel replaces: get_after_states(), then softmax, multinomial, the gather of the
                         picked row and the einsum of the expectation in torch, on the [B, a_max, 8] matrix
  play_linear            K greedy steps per launch, totals only                       <- yardstick of the next
  play_softmax           K sampled steps per launch, totals, logp_total and score_total
HIP events around windows of one launch, warm-up, median (min, max) of the repeats; ms per decision / per STEP.  The
games of the two play cases run on from launch to launch without resets: the share of envs still alive at the end is
reported, since a frozen env costs nothing.  One JSON line per case.
usage: bench_sample.py [--envs N] [--steps K] [--repeats N] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tetris_amd import VecTetris, _lib  # noqa: E402

YARDSTICK = {"policy_softmax_rows": "policy_greedy_rows", "composed": "policy_greedy_rows", "play_softmax": "play_linear"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sample.py measures on the GPU: no device found")
    B, K, T, dev = args.envs, args.steps, args.temperature, "cuda"
    lib = _lib.load()
    lines = []
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    for rows_ in (20, 40):
        start = VecTetris(10, rows_, B, device=dev, auto_reset=True, seed=0)
        for _ in range(30):
            start.step()
        start.auto_reset = False
        bcts = torch.tensor([VecTetris.BCTS_WEIGHTS], dtype=torch.float32, device=dev)
        zeros = torch.zeros(B, dtype=torch.int32, device=dev)
        i32 = lambda: torch.zeros(B, dtype=torch.int32, device=dev)
        f32 = lambda *shape: torch.zeros((B,) + shape, dtype=torch.float32, device=dev)

        def greedy_rows_case():
            env = start.fork(torch.arange(B, device=dev))
            ba, bv = i32(), f32()

            def launch():
                rc = lib.policy_greedy_rows(ctypes.byref(env.desc), p(env.cols), p(env.meta), p(bcts), 1, p(zeros), p(ba), p(bv),
                                            p(env.status), B, env._hip_stream())
                assert rc == 0, rc
            return env, launch, 1

        def softmax_rows_case():
            env = start.fork(torch.arange(B, device=dev))
            action, logp, score = i32(), f32(), f32(8)

            def launch():
                rc = lib.policy_softmax_rows(ctypes.byref(env.desc), p(env.cols), p(env.meta), p(bcts), 1, p(zeros), T, p(action),
                                             p(logp), p(score), None, None, p(env.status), env.seed, env.step_idx,
                                             env.env_offset, B, env._hip_stream())
                assert rc == 0, rc
            return env, launch, 1

        def composed_case():
            env = start.fork(torch.arange(B, device=dev))
            w = bcts[0]
            ar = torch.arange(B, device=dev)
            k = torch.arange(env.a_max, device=dev)[None, :]

            def launch():
                feats, nv = env.get_after_states()
                u = torch.matmul(feats, w) / T
                u = u.masked_fill(k >= nv[:, None], float("-inf"))
                prob = torch.softmax(u, dim=1)
                a = torch.multinomial(prob, 1)[:, 0]
                logp = torch.log(prob[ar, a])
                score = feats[ar, a] - torch.einsum("ba,baq->bq", prob, feats)
                return a, logp, score
            return env, launch, 1

        def play_case(softmax):
            env = start.fork(torch.arange(B, device=dev))
            tot, logp, score = torch.zeros((2, B), dtype=torch.int32, device=dev), f32(), f32(8)

            def launch():
                if softmax:
                    rc = lib.play_softmax(ctypes.byref(env.desc), p(env.cols), p(env.meta), K, p(bcts), 1, p(zeros), T, p(tot[0]),
                                          p(tot[1]), p(logp), p(score), p(env.n_valid), p(env.piece), p(env.status), env.seed,
                                          env.step_idx, env.env_offset, B, env._hip_stream())
                else:
                    rc = lib.play_linear(ctypes.byref(env.desc), p(env.cols), p(env.meta), K, p(bcts), 1, p(zeros), p(tot[0]),
                                         p(tot[1]), p(env.n_valid), p(env.piece), p(env.status), env.seed, env.step_idx,
                                         env.env_offset, B, env._hip_stream())
                assert rc == 0, rc
                env.step_idx += K
            return env, launch, K

        cases = {"policy_greedy_rows": greedy_rows_case(), "policy_softmax_rows": softmax_rows_case(),
                 "composed": composed_case(), "play_linear": play_case(False), "play_softmax": play_case(True)}
        for _ in range(args.warmup):
            for _, launch, _ in cases.values():
                launch()
        evs = {name: [] for name in cases}
        for _ in range(args.repeats):
            for name, (_, launch, _) in cases.items():  # interleaved: every case sees the same drift of the device
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                launch()
                e.record()
                evs[name].append((s, e))
        torch.cuda.synchronize()
        out = {}
        for name, (_, _, per) in cases.items():
            ts = sorted(s.elapsed_time(e) / per for s, e in evs[name])
            out[name] = (ts[len(ts) // 2], ts[0], ts[-1])
        for name, (ms, lo, hi) in out.items():
            env, _, per = cases[name]
            row = dict(case=name, board="10x%d" % rows_, envs=B, steps_per_launch=per, launches=args.repeats, temperature=T,
                       ms_per_step=ms, ms_per_step_min=lo, ms_per_step_max=hi,
                       alive_share_at_end=float((env.n_valid > 0).float().mean()), invalid=env.stats()["invalid"],
                       library_source_hash=lib.source_hash())
            if name in YARDSTICK:
                yard = out[YARDSTICK[name]]
                row.update(yardstick=YARDSTICK[name], over_yardstick=ms / yard[0], yardstick_spread=(yard[2] - yard[1]) / yard[0])
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
        del cases, start
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
