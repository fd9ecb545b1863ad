"""The context warp's backward (C = 196, fs = 4) at DAIN's training shape (B = 3, 256x448, one time offset) and at padded
1080p (B = 1, 1152x1984, the three time offsets of a x4 slow-motion step), on a smooth flow; device events, the variants
alternating inside one process after a warm-up, each number the median of --reps repetitions of --iters calls with the
spread (min-max) beside it:

  (a) what the reference-named module runs per time offset: zero-filled gradinput1 / 2 / 3 and
      vfi_filterinterp_backward_ori (all three gradients; the caller drops the flow's and the filter's), then torch adds the
      offsets' image gradients;
  (b) vfi_filterinterp_backward_ori_image_multi: the image gradient of every offset in one call, written once.

The fixed-point sums take 8 bytes per element of the gradient in the library's per-stream workspace: about 3.6 GB at the
1080p shape (printed).  Run under `rocprofv3 --kernel-trace --stats` (e.g. --reps 1 --iters 3) for the per-kernel split.

    python tools/bench_ctx_bwd.py [--reps 7] [--iters 10] [--warmup 3]
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

C = 196


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def smooth_flow(B, H, W, phase, t):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    f = torch.stack([6.0 * torch.sin(xx / 97.0 + yy / 131.0 + phase) + 1.3, 5.0 * torch.cos(xx / 113.0 - yy / 71.0) - 0.7])
    return (f * t)[None].repeat(B, 1, 1, 1).contiguous().cuda()


def impls(B, H, W, offsets):
    gen = torch.Generator().manual_seed(5)
    ctx = torch.rand((B, C, H, W), generator=gen).cuda()
    flows = [smooth_flow(B, H, W, 0.0, 2.0 * t) for t in offsets]          # (the projected flow of time offset t)
    filt = torch.softmax(torch.randn((B, 16, H, W), generator=gen), 1).cuda()
    gouts = [torch.randn((B, C, H, W), generator=gen).cuda() for _ in offsets]
    gimg = torch.empty_like(ctx)

    def per_offset():
        total = None
        for fl, g in zip(flows, gouts):
            g1, g2, g3 = torch.zeros_like(ctx), torch.zeros_like(fl), torch.zeros_like(filt)
            if cabi.filterinterp_backward_ori(ctx, fl, filt, g, g1, g2, g3) != 0:
                raise RuntimeError("filterinterp_backward_ori failed")
            total = g1 if total is None else total + g1
        return total

    def image_multi():
        if cabi.filterinterp_backward_ori_image_multi(flows, filt, gouts, gimg) != 0:
            raise RuntimeError("filterinterp_backward_ori_image_multi failed")
        return gimg

    return {"a_per_offset_full_backward": per_offset, "b_image_multi": image_multi}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ctx_bwd.py needs a GPU")
    summary = {}
    for name, (B, H, W), offsets in (("vimeo_b3_256x448_1offset", (3, 256, 448), (0.5,)),
                                     ("1080p_1152x1984_3offsets", (1, 1152, 1984), (0.25, 0.5, 0.75))):
        print("%s: %.2f GB of fixed-point sums in the library's workspace" % (name, 8.0 * B * C * H * W / 1e9))
        fns = impls(B, H, W, offsets)
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        a, b = fns["a_per_offset_full_backward"](), fns["b_image_multi"]()
        agree = float((a - b).abs().max())                  # (equal bits for one offset; for three the scales differ)
        times = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, fn in fns.items():                       # alternating
                times[k].append(timed(fn, args.iters))
        row = {"max_abs_difference": agree}
        for k, ts in times.items():
            ts.sort()
            row[k] = {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}
            print("%-26s %-28s %.4f ms  (%.4f - %.4f)" % (name, k, ts[len(ts) // 2], ts[0], ts[-1]))
        summary[name] = row
        del fns, a, b
        torch.cuda.empty_cache()
    print(json.dumps({"bench_ctx_bwd": summary, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
