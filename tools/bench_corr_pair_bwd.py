"""The correlation backward of a frame pair's two flow networks (PWC-Net's configuration: pad 4, kernel 1, max displacement
4, strides 1; float32) at every level of the 1080p pyramid (B = 1) and of the Vimeo training pyramid (B = 3, 256x448 frames);
device events, the variants alternating inside one process after a warm-up, each number the median of --reps repetitions
of --iters calls with the spread (min-max) beside it:

  (a) two cabi.correlation_backward calls: four launches (the yardstick);
  (b) one cabi.correlation_backward_pair call with all four gradients: one launch;
  (c) one cabi.correlation_backward_pair call with only the two gradinput2 (the first features are frozen).

Then the sum over the five levels of each pyramid, and a JSON summary line.

    python tools/bench_corr_pair_bwd.py [--reps 7] [--iters 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vfidkr_amd  # noqa: E402,F401
from vfidkr_amd import cabi  # noqa: E402
from tools.bench_corr_bwd import LEVELS  # noqa: E402

PYRAMIDS = (("1080p_b1", 1, LEVELS), ("vimeo_b3", 3, ((32, 64, 112), (64, 32, 56), (96, 16, 28), (128, 8, 14), (196, 4, 7))))
CFG = (4, 1, 4, 1, 1)


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def impls(B, C, H, W):
    gen = torch.Generator().manual_seed(3)
    a1, a2, b1, b2 = (torch.randn((B, C, H, W), generator=gen).cuda() for _ in range(4))
    ga, gb = (torch.randn((B, 81, H, W), generator=gen).cuda() for _ in range(2))

    def two_calls():
        cabi.correlation_backward(a1, a2, ga, *CFG)
        cabi.correlation_backward(b1, b2, gb, *CFG)

    def pair_all():
        cabi.correlation_backward_pair(a1, a2, ga, b1, b2, gb, *CFG)

    def pair_second():
        cabi.correlation_backward_pair(a1, a2, ga, b1, b2, gb, *CFG, want=(False, True, False, True))

    return {"a_two_calls": two_calls, "b_pair_all": pair_all, "c_pair_gradinput2": pair_second}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_corr_pair_bwd.py needs a GPU")
    summary = {}
    for name, B, levels in PYRAMIDS:
        rows, sums = [], {}
        for (C, H, W) in levels:
            fns = impls(B, C, H, W)
            for fn in fns.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in fns}
            for _ in range(args.reps):
                for k, fn in fns.items():                   # alternating
                    times[k].append(timed(fn, args.iters))
            row = {"C": C, "H": H, "W": W}
            for k, ts in times.items():
                ts.sort()
                row[k] = {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}
                sums[k] = sums.get(k, 0.0) + ts[len(ts) // 2]
                print("%-9s C=%3d %3dx%3d  %-18s %.4f ms  (%.4f - %.4f)" % (name, C, H, W, k, ts[len(ts) // 2], ts[0], ts[-1]),
                      flush=True)
            rows.append(row)
        for k, s in sums.items():
            print("%-9s sum of the five levels  %-18s %.4f ms" % (name, k, s), flush=True)
        summary[name] = {"levels": rows, "sum_ms": {k: round(s, 4) for k, s in sums.items()}}
    print(json.dumps({"bench_corr_pair_bwd": summary, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
