#!/usr/bin/env python3
"""Times tetris_hip_expand_envs (VecTetris.expand_from: dst[j] := src[parent[j]] after placement action[j]) at 1 Mi dst
envs, 10x20 and 10x40, against the composed pair that existed before the call -- copy_envs_from(src, parent) followed by
step(action) on dst, two launches with the children's parents written to HBM and read back in between -- for three
parent patterns: identity; each of B / 36 parents 36 times, sorted (the dense expansion); a random permutation.

Yardstick and subject run interleaved, launch by launch, in one process on two copies of one start state, with the same
parent and action tensors; HIP events around every launch (the pair: around both), median (min - max) of the repeats.
The ratio is quoted beside the yardstick's own spread.  One JSON document.
usage: bench_expand.py [--envs N] [--repeats N] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tetris_amd import VecTetris, _lib  # noqa: E402
from tetris_amd.vec_env import _ptr  # noqa: E402


def stats(evs):
    ts = sorted(s.elapsed_time(e) for s, e in evs)
    return dict(ms=ts[len(ts) // 2], ms_min=ts[0], ms_max=ts[-1])


def timed(fn, evs):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    evs.append((s, e))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=51)
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_expand.py measures on the GPU: no device found")
    B, dev = args.envs, "cuda"
    lib = _lib.load()
    rows_out = []
    for rows in (20, 40):
        src = VecTetris(10, rows, B, device=dev, auto_reset=True, seed=0)
        for _ in range(100):
            src.step()
        # two copies of one start state: the pair runs on `a`, the fused call on `b`
        a, b = (VecTetris(10, rows, B, device=dev, auto_reset=False, seed=1) for _ in range(2))
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        own = torch.arange(B, dtype=torch.int32, device=dev)
        patterns = {
            "identity": own,
            "each_of_B/36_36_times_sorted": own // 36,
            "random_permutation": torch.randperm(B, device=dev, generator=g).to(torch.int32),
        }
        per_child = src.n_planes * src.desc.word_bytes + 8  # board and meta of one child: written and read back by the pair
        for name, parent in patterns.items():
            u = torch.rand(B, device=dev, generator=g)
            action = (u * src.n_valid[parent.long()].to(torch.float32)).to(torch.int32).contiguous()

            def pair():
                a._gather_call(src.cols, src.meta, B, a.cols, a.meta, parent, a.status)
                a.step(action)

            def fused():  # (the call expand_from makes, without its argument checks: the window should hold the kernel)
                lib.expand_envs(ctypes.byref(b.desc), _ptr(src.cols), _ptr(src.meta), B, _ptr(b.cols), _ptr(b.meta),
                                _ptr(parent), _ptr(action), None, _ptr(b._obs_buf), _ptr(b._reward_buf), _ptr(b._done_buf),
                                _ptr(b._lines_buf), _ptr(b.n_valid), _ptr(b.piece), _ptr(b.status), src.seed, src.step_idx,
                                src.env_offset, B, b._hip_stream())

            for _ in range(5):
                pair()
                fused()
            ev_pair, ev_fused = [], []
            for _ in range(args.repeats):
                timed(pair, ev_pair)
                timed(fused, ev_fused)
            torch.cuda.synchronize()
            a.check()
            b.check()
            assert torch.equal(a.boards(), b.boards()) and torch.equal(a.lines, b.lines)  # the same children
            y, s = stats(ev_pair), stats(ev_fused)
            row = dict(board="10x%d" % rows, envs=B, pattern=name, yardstick_gather_then_step=y, subject_expand_envs=s,
                       speedup=y["ms"] / s["ms"], yardstick_spread=(y["ms_max"] - y["ms_min"]) / y["ms"],
                       round_trip_bytes_saved_per_child=2 * per_child)
            rows_out.append(row)
            print(json.dumps(row), flush=True)
        del src, a, b
        torch.cuda.empty_cache()
    doc = dict(tool="tools/bench_expand.py", library_source_hash=lib.source_hash(), device=torch.cuda.get_device_name(0),
               repeats=args.repeats, rows=rows_out)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
