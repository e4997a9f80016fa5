#!/usr/bin/env python3
"""Times tetris_hip_gather_envs (VecTetris.copy_envs_from: dst[j] := src[index[j]]) at 1 Mi dst envs, 10x20 and
10x40, for four index patterns, and prices it against HBM: algorithmic bytes per copied env =
2 * n_planes * W (board read + written) + 16 (meta) + 4 (index) + 2 (n_valid, piece); an entry of -1 costs its
4 index bytes.  Beside it, in the same process: the composed path that existed before the call (boards() ->
index_select -> set_boards(cells, piece), which does not carry the bag) and what the box gives a plain
torch copy_.  HIP events around each call, warm-up, median of the repeats.  One JSON line per case.
usage: bench_gather.py [--envs N] [--repeats N] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tetris_amd import VecTetris, _lib  # noqa: E402


def median_ms(fn, repeats, warmup=5, n_per=1):
    """ms per call: median (min, max) over `repeats` windows of `n_per` back-to-back calls between two events"""
    for _ in range(warmup):
        fn()
    evs = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n_per):
            fn()
        e.record()
        evs.append((s, e))
    torch.cuda.synchronize()
    ts = sorted(s.elapsed_time(e) / n_per for s, e in evs)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=31)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gather.py measures on the GPU: no device found")
    B, dev = args.envs, "cuda"
    lines = []

    def emit(**row):
        row["library_source_hash"] = _lib.load().source_hash()
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    # what this box's HBM gives a plain copy (as bench.py --full: read + written bytes of a 1 GiB copy_ / time)
    a = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    a.fill_(1.0)
    ms, lo, hi = median_ms(lambda: b.copy_(a), 11, warmup=3)
    copy_gbs = 2.0 * a.numel() * 4 / ms / 1e6
    emit(case="torch_copy_1GiB", ms=ms, ms_min=lo, ms_max=hi, GBps=copy_gbs)
    del a, b
    torch.cuda.empty_cache()

    for rows, pieces in ((20, "default"), (40, "default")):
        src = VecTetris(10, rows, B, device=dev, pieces=pieces, auto_reset=True, seed=0)
        for _ in range(100):
            src.step()
        dst = VecTetris(10, rows, B, device=dev, pieces=pieces, auto_reset=True, seed=1)
        per_env = 2 * src.n_planes * src.desc.word_bytes + 16 + 4 + 2
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        own = torch.arange(B, dtype=torch.int32, device=dev)
        draws = torch.randint(B, (B,), device=dev, generator=g).to(torch.int32)
        patterns = {
            "identity": own,
            "each_of_B/4_four_times_sorted": own // 4,
            "random_permutation": torch.randperm(B, device=dev, generator=g).to(torch.int32),
            "bank_25pct_rest_keep": torch.where(torch.rand(B, device=dev, generator=g) < 0.25, draws, torch.full_like(own, -1)),
        }
        base = None
        for name, index in patterns.items():
            copied = int((index >= 0).sum())
            nbytes = copied * per_env + (B - copied) * 4
            # (the call copy_envs_from makes, without its argument checks: the window should hold kernels, not Python)
            ms, lo, hi = median_ms(lambda: dst._gather_call(src.cols, src.meta, B, dst.cols, dst.meta, index, dst.status),
                                   args.repeats, n_per=20)
            base = ms if name == "identity" else base
            emit(case="gather_envs", board="10x%d" % rows, envs=B, pattern=name, copied=copied, bytes_per_copied_env=per_env,
                 ms=ms, ms_min=lo, ms_max=hi, GBps=nbytes / ms / 1e6, frac_of_copy=nbytes / ms / 1e6 / copy_gbs,
                 ms_over_identity=ms / base)
            dst.check()
        # the path a user had before: decode, reorder the cells, encode + refresh (the bag stays behind)
        for name in ("identity", "random_permutation"):
            index = patterns[name].long()

            def composed():
                dst.set_boards(src.boards().index_select(0, index), src.piece.index_select(0, index))
            ms, lo, hi = median_ms(composed, 11, warmup=3)
            emit(case="composed_boards_index_select_set_boards", board="10x%d" % rows, envs=B, pattern=name, ms=ms, ms_min=lo,
                 ms_max=hi, carries_bag=False)
        del src, dst
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
