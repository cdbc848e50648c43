#!/usr/bin/env python3
"""Time the fused ensemble_merge kernel against the eager torch chain it
replaces (flip-merge, bicubic x-stride upsample, crop, bicubic resize, scale,
accumulate) at the workload shape of a 512^2 image: a 160x160 stride-4 network
output, upsampled to 640x640 and resized to 512x512, 50 channels.

Both paths run interleaved in one process on the same random bf16
channels_last input; times come from device events around `--iters` calls.

    python scripts/ensemble_merge_perf.py [--n 8] [--iters 50] [--rounds 5]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from improved_body_parts_amd.ops.ensemble import (  # noqa: E402
    ensemble_merge, merge_chain)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1, 8],
                    help="images per call (each contributes two views)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_merge_perf.py needs a GPU")

    C, h4, w4, stride, sh, sw, H, W = 50, 160, 160, 4, 640, 640, 512, 512
    perm = np.random.RandomState(0).permutation(C)
    print(f"shape (h4,w4,sh,sw,H,W)=({h4},{w4},{sh},{sw},{H},{W}) C={C} "
          f"bf16 channels_last, {torch.cuda.get_device_name(0)}")

    for n in args.n:
        src = torch.rand(2 * n, C, h4, w4, device="cuda").bfloat16() \
            .contiguous(memory_format=torch.channels_last)
        acc_k = torch.zeros(n, C, H, W, device="cuda")
        acc_t = torch.zeros(n, C, H, W, device="cuda")

        def timed(fn):
            start = torch.cuda.Event(enable_timing=True)
            stop = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.iters):
                fn()
            stop.record()
            torch.cuda.synchronize()
            return start.elapsed_time(stop) / args.iters * 1e3   # us per call

        # accumulate=False is the first (or only) run of an ensemble: a pure
        # write; accumulate=True also reads the planar maps back
        for accumulate in (False, True):
            def kernel():
                ensemble_merge(src, perm, stride, (sh, sw), (H, W), scale=0.5,
                               out=acc_k, accumulate=accumulate)

            def chain():
                res = merge_chain(src, perm, stride, (sh, sw), (H, W), 0.5)
                if accumulate:
                    acc_t.add_(res)
                else:
                    acc_t.copy_(res)

            for fn in (kernel, chain):
                for _ in range(3):
                    fn()
            acc_k.zero_()
            acc_t.zero_()
            kernel()
            chain()
            err = float((acc_k - acc_t).abs().max())

            tk, tt = [], []
            for _ in range(args.rounds):
                tk.append(timed(kernel))
                tt.append(timed(chain))
            # bytes the fused pass has to move: both views in, the planar maps
            # written (and read first when accumulating)
            moved = src.numel() * 2 + (2 if accumulate else 1) * acc_k.numel() * 4
            mk, mt = float(np.median(tk)), float(np.median(tt))
            print(f"n={n} accumulate={accumulate}: kernel median {mk:.1f} us "
                  f"(min {min(tk):.1f}), torch chain median {mt:.1f} us "
                  f"(min {min(tt):.1f}), speedup {mt / mk:.2f}x, kernel "
                  f"{moved / mk / 1e6:.2f} TB/s of {moved / 1e6:.1f} MB, "
                  f"max abs diff {err:.2e}", flush=True)


if __name__ == "__main__":
    main()
