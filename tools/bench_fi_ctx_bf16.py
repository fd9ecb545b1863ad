"""The context warp (FilterInterpolate_ctx, C = 196, fs = 4) on bfloat16 tensors beside what a bfloat16 network had to do before,
in one process: one direction at padded 1080p (B = 1, 1152x1984, the three time offsets of a x4 slow-motion step) and at DAIN's
training shape (B = 3, 256x448, one offset), forward and forward + backward, on a smooth flow:

  bf16        the fused call on the bfloat16 context (vfi_filterinterp_forward_ori_multi_to_bf16; training: plus
              vfi_filterinterp_backward_ori_image_multi_bf16 on bfloat16 gradients)
  cast        the yardstick: .float() of the context, the float32 fused call, .bfloat16() of each output; training: autograd
              through the same casts, so the incoming gradients are widened and the context gradient is rounded by torch
  fp32        the float32 fused call alone, on float32 tensors (no requirement)
  f16         vfi_filterinterp_forward_ori_f16 once per offset, forward only (no requirement)

The variants alternate inside every repetition after a warm-up; a sample is --iters calls between two device events; each
figure is the median of --reps samples with their range [min - max], in milliseconds per call.  `of 8 TB/s`: the algorithmic
bytes of the bfloat16 forward (the context read once per offset and each output written once at 2 bytes, flow and filter at
4) over the median time.  Prints one block per shape, then a JSON line; `bf16_faster` says whether the bfloat16 path beat the
composition at that shape.

    python tools/bench_fi_ctx_bf16.py [--reps 7] [--iters 5] [--warmup 2] [--lib <pkg>/lib_vX/libvfi_hip.so]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vfidkr_amd  # noqa: E402,F401
if "--lib" in sys.argv:         # a variant build of the library (tools/mkvariant.sh)
    vfidkr_amd.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
from vfidkr_amd import cabi, fused  # noqa: E402

C = 196
SHAPES = (("1080p", 1, 1152, 1984, (0.25, 0.5, 0.75)), ("vimeo", 3, 256, 448, (0.5,)))
HBM_BYTES_PER_S = 8e12


def smooth_flow(B, H, W, t):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    f = torch.stack([6.0 * torch.sin(xx / 97.0 + yy / 131.0) + 1.3, 5.0 * torch.cos(xx / 113.0 - yy / 71.0) - 0.7])
    return (f * t)[None].repeat(B, 1, 1, 1).contiguous().cuda()


def variants(B, H, W, offsets):
    gen = torch.Generator().manual_seed(5)
    ctx32 = torch.rand((B, C, H, W), generator=gen).cuda()
    ctx_bf, ctx16 = ctx32.bfloat16(), ctx32.half()
    flows = [smooth_flow(B, H, W, 2.0 * t) for t in offsets]               # (the projected flow of time offset t)
    filt = torch.softmax(torch.randn((B, 16, H, W), generator=gen), 1).cuda()
    g32 = [torch.randn((B, C, H, W), generator=gen).cuda() for _ in offsets]
    g_bf = [g.bfloat16() for g in g32]
    out16 = torch.empty_like(ctx16)

    def fwd(ctx, cast):
        def run():
            with torch.no_grad():
                if cast:
                    return [o.bfloat16() for o in fused._ctx_warp(ctx.float(), flows, filt)]
                return fused._ctx_warp(ctx, flows, filt)
        return run

    def train(ctx, gouts, cast):
        leaf = ctx.clone().requires_grad_()

        def run():
            leaf.grad = None
            outs = [o.bfloat16() for o in fused._ctx_warp(leaf.float(), flows, filt)] if cast else fused._ctx_warp(leaf, flows, filt)
            torch.autograd.backward(outs, gouts)
            return leaf.grad
        return run

    def f16():
        for fl in flows:
            if cabi.filterinterp_forward_ori_f16(ctx16, fl, filt, out16) != 0:
                raise RuntimeError("filterinterp_forward_ori_f16 failed")

    return {"fwd": {"bf16": fwd(ctx_bf, False), "cast": fwd(ctx_bf, True), "fp32": fwd(ctx32, False), "f16": f16},
            "fwd+bwd": {"bf16": train(ctx_bf, g_bf, False), "cast": train(ctx_bf, g_bf, True), "fp32": train(ctx32, g32, False)}}


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fi_ctx_bf16.py needs a GPU")
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters, "shapes": []}
    for name, B, H, W, offsets in SHAPES:
        row = {"shape": name, "B": B, "C": C, "H": H, "W": W, "offsets": len(offsets)}
        algo = len(offsets) * (2 * B * C * H * W * 2 + B * 18 * H * W * 4)
        print("%s  B=%d C=%d %dx%d, %d time offset(s), one direction" % (name, B, C, H, W, len(offsets)), flush=True)
        for what, fns in variants(B, H, W, offsets).items():
            for fn in fns.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            samples = {k: [] for k in fns}
            for _ in range(args.reps):
                for k, fn in fns.items():
                    samples[k].append(timed(fn, args.iters))
            for k, v in samples.items():
                v.sort()
                row["%s %s" % (what, k)] = (round(v[len(v) // 2], 3), round(v[0], 3), round(v[-1], 3))
                print("    %-8s %-5s %8.3f ms  [%.3f - %.3f]" % ((what, k) + row["%s %s" % (what, k)]), flush=True)
            row["%s bf16_faster" % what] = row["%s bf16" % what][0] < row["%s cast" % what][0]
            print("    %-8s bf16 / cast = %.2f   bf16 faster than the composition: %s" % (
                what, row["%s bf16" % what][0] / row["%s cast" % what][0], row["%s bf16_faster" % what]), flush=True)
        row["fwd algorithmic GB"] = round(algo / 1e9, 3)
        row["fwd fraction of 8 TB/s"] = round(algo / (row["fwd bf16"][0] * 1e-3) / HBM_BYTES_PER_S, 3)
        print("    forward: %.3f GB algorithmic, %.1f %% of 8 TB/s" % (row["fwd algorithmic GB"], 100 * row["fwd fraction of 8 TB/s"]),
              flush=True)
        result["shapes"].append(row)
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
