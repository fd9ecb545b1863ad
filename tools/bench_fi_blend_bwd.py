"""The FilterInterpolate blend backward at DAIN's training shape (B = 3, 3x256x448) and at padded 1080p (1152x1984, C = 3),
fs = 4, on a smooth flow; device events, the variants alternating inside one process after a warm-up, each number the
median of --reps repetitions of --iters calls with the spread (min-max) beside it:

  (a) the composition the reference-named modules run: torch forms g_d = grad_blend * w_d + grad_out_d, then per direction
      zero-filled gradients and vfi_filterinterp_backward_ori (all three gradients);
  (b) vfi_filterinterp_blend_backward with all six gradients;
  (c) vfi_filterinterp_blend_backward without the frame gradients (DAIN training: the frames need none).

Run under `rocprofv3 --kernel-trace --stats` (e.g. --reps 1 --iters 5) for the per-kernel split.

    python tools/bench_fi_blend_bwd.py [--reps 7] [--iters 20] [--warmup 5]
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


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def smooth_flow(B, H, W, phase):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    f = torch.stack([6.0 * torch.sin(xx / 97.0 + yy / 131.0 + phase) + 1.3, 5.0 * torch.cos(xx / 113.0 - yy / 71.0) - 0.7])
    return f[None].repeat(B, 1, 1, 1).contiguous().cuda()


def impls(B, H, W, C=3, w0=0.5, w2=0.5):
    gen = torch.Generator().manual_seed(5)
    refs = [torch.rand((B, C, H, W), generator=gen).cuda() for _ in range(2)]
    flows = [smooth_flow(B, H, W, 0.0), smooth_flow(B, H, W, 1.7)]
    filts = [torch.softmax(torch.randn((B, 16, H, W), generator=gen), 1).cuda() for _ in range(2)]
    gb, g0, g2 = [torch.randn((B, C, H, W), generator=gen).cuda() for _ in range(3)]
    outs = [torch.empty_like(t) for t in (refs[0], refs[1], flows[0], flows[1], filts[0], filts[1])]

    def composed():
        for d, (go, wd) in enumerate(((g0, w0), (g2, w2))):
            g = gb * wd + go
            gr, gf, gk = torch.zeros_like(refs[d]), torch.zeros_like(flows[d]), torch.zeros_like(filts[d])
            if cabi.filterinterp_backward_ori(refs[d], flows[d], filts[d], g, gr, gf, gk) != 0:
                raise RuntimeError("filterinterp_backward_ori failed")

    def blend_all():
        if cabi.filterinterp_blend_backward(*refs, *flows, *filts, gb, g0, g2, w0, w2, *outs) != 0:
            raise RuntimeError("filterinterp_blend_backward failed")

    def blend_noref():
        if cabi.filterinterp_blend_backward(*refs, *flows, *filts, gb, g0, g2, w0, w2, None, None, *outs[2:]) != 0:
            raise RuntimeError("filterinterp_blend_backward failed")

    return {"a_composed_all": composed, "b_blend_all": blend_all, "c_blend_no_ref": blend_noref}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fi_blend_bwd.py needs a GPU")
    summary = {}
    for name, (B, H, W) in (("vimeo_b3_256x448", (3, 256, 448)), ("1080p_1152x1984", (1, 1152, 1984))):
        fns = impls(B, H, W)
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, fn in fns.items():                       # alternating
                times[k].append(timed(fn, args.iters))
        row = {}
        for k, ts in times.items():
            ts.sort()
            row[k] = {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}
            print("%-18s %-16s %.4f ms  (%.4f - %.4f)" % (name, k, ts[len(ts) // 2], ts[0], ts[-1]))
        summary[name] = row
    print(json.dumps({"bench_fi_blend_bwd": summary, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
