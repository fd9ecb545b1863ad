"""What a PWC level spends on its cost volume, with and without the LeakyReLU fused into the correlation (PWC-Net's
configuration: pad 4, kernel 1, max displacement 4, strides 1; float32), at every level of the 1080p pyramid (B = 1) and of
the Vimeo training pyramid (B = 3, 256x448 frames), single (one network) and paired (both networks of a frame pair);
device events, the variants alternating inside one process after a warm-up, each number the median of --reps repetitions
of --iters calls with the spread (min-max) beside it.

  forward (inference, no grad):
    fwd_a  the correlation call + F.leaky_relu + torch.cat((corr, tail), 1) with a 32-channel tail;
    fwd_b  the fused call writing into buf[:, :81] of the preallocated (B, 113, H, W) buffer + the tail's copy into
           buf[:, 81:] (what torch.cat would still have to move).
  forward + backward under autograd (the loss reaches the cost volume through torch.cat; its gradient is a dense
  (B, 113, H, W) tensor that exists before the timed region):
    fb_a   fused.corr_pair / fused._Corr + F.leaky_relu + torch.cat, backward with today's .contiguous() of cat's gradient;
    fb_b   fused.corr_pair_lrelu / fused.corr_lrelu + torch.cat, backward reading cat's gradient where it lies.

Then the sum over the five levels of each pyramid, and a JSON summary line.

    python tools/bench_corr_lrelu.py [--reps 7] [--iters 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vfidkr_amd  # noqa: E402,F401
from vfidkr_amd import cabi, fused  # noqa: E402
from tools.bench_corr_pair_bwd import PYRAMIDS, timed  # noqa: E402

CFG = (4, 1, 4, 1, 1)
TAIL = 32
SLOPE = 0.1


def impls(B, C, H, W, paired):
    gen = torch.Generator().manual_seed(3)
    n = 2 if paired else 1
    xs = [torch.randn((B, C, H, W), generator=gen).cuda() for _ in range(2 * n)]
    tails = [torch.randn((B, TAIL, H, W), generator=gen).cuda() for _ in range(n)]
    gcat = [torch.randn((B, 81 + TAIL, H, W), generator=gen).cuda() for _ in range(n)]
    bufs = [torch.empty((B, 81 + TAIL, H, W), device="cuda") for _ in range(n)]
    leaves = [x.clone().requires_grad_(True) for x in xs]

    def fwd_a():
        with torch.no_grad():
            corrs = cabi.correlation_forward_pair(*xs, *CFG) if paired else (cabi.correlation_forward(*xs, *CFG),)
            return [torch.cat((F.leaky_relu(c, SLOPE), t), 1) for c, t in zip(corrs, tails)]

    def fwd_b():
        with torch.no_grad():
            if paired:
                fused.corr_pair_lrelu(*xs, negative_slope=SLOPE, out=(bufs[0][:, :81], bufs[1][:, :81]))
            else:
                fused.corr_lrelu(*xs, negative_slope=SLOPE, out=bufs[0][:, :81])
            for b, t in zip(bufs, tails):
                b[:, 81:].copy_(t)
            return bufs

    def backward(cats):
        torch.autograd.backward(cats, gcat, inputs=leaves)
        for x in leaves:
            x.grad = None

    def fb_a():
        corrs = fused.corr_pair(*leaves) if paired else (fused._Corr.apply(*leaves),)
        backward([torch.cat((F.leaky_relu(c, SLOPE), t), 1) for c, t in zip(corrs, tails)])

    def fb_b():
        corrs = fused.corr_pair_lrelu(*leaves, negative_slope=SLOPE) if paired else (fused.corr_lrelu(*leaves, negative_slope=SLOPE),)
        backward([torch.cat((c, t), 1) for c, t in zip(corrs, tails)])

    return {"fwd_a": fwd_a, "fwd_b": fwd_b, "fb_a": fb_a, "fb_b": fb_b}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_corr_lrelu.py needs a GPU")
    summary = {}
    for name, B, levels in PYRAMIDS:
        for paired in (False, True):
            tag = "%s_%s" % (name, "pair" if paired else "single")
            rows, sums = [], {}
            for (C, H, W) in levels:
                fns = impls(B, C, H, W, paired)
                for fn in fns.values():
                    for _ in range(args.warmup):
                        fn()
                torch.cuda.synchronize()
                times = {k: [] for k in fns}
                for _ in range(args.reps):
                    for k, fn in fns.items():               # alternating
                        times[k].append(timed(fn, args.iters))
                row = {"C": C, "H": H, "W": W}
                for k, ts in times.items():
                    ts.sort()
                    row[k] = {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}
                    sums[k] = sums.get(k, 0.0) + ts[len(ts) // 2]
                    print("%-16s C=%3d %3dx%3d  %-6s %.4f ms  (%.4f - %.4f)" % (tag, C, H, W, k, ts[len(ts) // 2], ts[0], ts[-1]),
                          flush=True)
                rows.append(row)
                del fns
                torch.cuda.empty_cache()
            for k, s in sums.items():
                print("%-16s sum of the five levels  %-6s %.4f ms" % (tag, k, s), flush=True)
            summary[tag] = {"levels": rows, "sum_ms": {k: round(s, 4) for k, s in sums.items()}}
    print(json.dumps({"bench_corr_lrelu": summary, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
