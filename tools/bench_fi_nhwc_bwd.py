"""The image gradient of the context warp (FilterInterpolate_ctx, C = 196, fs = 4) on channels_last tensors beside what a
channels_last network had to do before, in one process: one direction at padded 1080p (B = 1, 1152x1984, the three time offsets
of a x4 slow-motion step) and at DAIN's training shape (B = 3, 256x448, one offset), smooth flow, float32 and bfloat16:

  (a) nhwc      the new call: channels_last gradients in, a channels_last context gradient out
                (vfi_filterinterp_backward_ori_nhwc_image_multi[_bf16])
  (a') direct   the same call with every tile on the per-addend kernel (the internal _direct entry): the staged kernel ships
                only while (a) beats this at the 1080p shape
  (b) copies    the composition (a) replaces: .contiguous() of each gradient, the NCHW backward, a channels_last copy of the result
  (c) nchw      the NCHW backward alone on NCHW tensors (reported, no requirement)
  (d) fwd+bwd   forward + backward through fused.FilterInterpolate_ctx_all: `train` with train_channels_last=True on a
                channels_last context, `train_copies` with the keyword's composition (a .contiguous() context into the NCHW
                Function, channels_last copies of the outputs; autograd then copies the gradients back the other way)

The variants alternate inside every repetition after a warm-up (run hot); a sample is --iters calls between two device events;
each figure is the median of --reps samples with their range [min - max], in milliseconds per call.  `apart`: the two ranges do
not overlap.  Prints one block per shape and dtype, then a JSON line.

    python tools/bench_fi_nhwc_bwd.py [--reps 7] [--iters 5] [--warmup 2] [--out profiles/fi_nhwc_bwd_bench.txt]
                                    [--shapes 1080p,vimeo] [--skip direct]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vfidkr_amd  # noqa: E402,F401
from vfidkr_amd import cabi, cabi_nhwc, fused  # noqa: E402

C = 196
SHAPES = (("1080p", 1, 1152, 1984, (0.25, 0.5, 0.75)), ("vimeo", 3, 256, 448, (0.5,)))
CL = torch.channels_last


def smooth_flow(B, H, W, t):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    f = torch.stack([6.0 * torch.sin(xx / 97.0 + yy / 131.0) + 1.3, 5.0 * torch.cos(xx / 113.0 - yy / 71.0) - 0.7])
    return (f * t)[None].repeat(B, 1, 1, 1).contiguous().cuda()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _check(err, what):
    if err != 0:
        raise RuntimeError("%s returned %d" % (what, err))


def variants(B, H, W, offsets, dtype, skip):
    gen = torch.Generator().manual_seed(5)
    flows = [smooth_flow(B, H, W, 2.0 * t) for t in offsets]               # (the projected flow of time offset t)
    filt = torch.softmax(torch.randn((B, 16, H, W), generator=gen), 1).cuda()
    gs = [torch.randn((B, C, H, W), generator=gen).cuda().to(dtype) for _ in offsets]
    gs_cl = [g.contiguous(memory_format=CL) for g in gs]
    out_cl = torch.empty((B, C, H, W), dtype=dtype, device="cuda").contiguous(memory_format=CL)
    out = torch.empty((B, C, H, W), dtype=dtype, device="cuda")
    ctx_cl = torch.rand((B, C, H, W), generator=gen).cuda().to(dtype).contiguous(memory_format=CL).requires_grad_()

    def nhwc():
        _check(cabi_nhwc.filterinterp_backward_nhwc_image_multi(flows, filt, gs_cl, out_cl), "nhwc")
        return out_cl

    def direct():
        _check(cabi_nhwc.filterinterp_backward_nhwc_image_multi(flows, filt, gs_cl, out_cl, direct=True), "direct")
        return out_cl

    def copies():
        _check(cabi.filterinterp_backward_ori_image_multi(flows, filt, [g.contiguous() for g in gs_cl], out), "copies")
        return out.contiguous(memory_format=CL)

    def nchw():
        _check(cabi.filterinterp_backward_ori_image_multi(flows, filt, gs, out), "nchw")
        return out

    def train():
        outs = fused._ctx_warp(ctx_cl, flows, filt, True)
        return torch.autograd.grad(outs, [ctx_cl], gs_cl)[0]

    def train_copies():
        outs = [o.contiguous(memory_format=CL) for o in fused._ctx_warp(ctx_cl.contiguous(), flows, filt)]
        return torch.autograd.grad(outs, [ctx_cl], gs_cl)[0]

    # (what is timed computes the same thing: checked once, outside the timed window)
    want = _bits(copies()).clone()
    assert torch.equal(_bits(nhwc()), want), "nhwc and copies differ"
    assert torch.equal(_bits(train()), want) and torch.equal(_bits(train_copies()), want), "the trained gradients differ"
    fns = {"nhwc": nhwc, "direct": direct, "copies": copies, "nchw": nchw, "train": train, "train_copies": train_copies}
    if "direct" not in skip:
        assert torch.equal(_bits(direct()), want), "direct and copies differ"
    return {k: f for k, f in fns.items() if k not in skip}


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def apart(a, b):
    return a[2] < b[1] or b[2] < a[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--shapes", default="1080p,vimeo")
    ap.add_argument("--skip", default="", help="variants to leave out, e.g. direct")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fi_nhwc_bwd.py needs a GPU")
    skip = set(filter(None, args.skip.split(",")))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters, "rows": []}
    say("device: %s; median of %d x %d calls [min - max], ms per call (one direction, all time offsets)" % (
        result["device"], args.reps, args.iters))
    for name, B, H, W, offsets in (s for s in SHAPES if s[0] in args.shapes.split(",")):
        for dtype in (torch.float32, torch.bfloat16):
            dn = str(dtype).replace("torch.", "")
            row = {"shape": name, "B": B, "C": C, "H": H, "W": W, "offsets": len(offsets), "dtype": dn, "flow": "smooth"}
            say("%s  B=%d C=%d %dx%d, %d time offset(s), %s, smooth flow" % (name, B, C, H, W, len(offsets), dn))
            fns = variants(B, H, W, offsets, dtype, skip)
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
                row[k] = (round(v[len(v) // 2], 3), round(v[0], 3), round(v[-1], 3))
                say("    %-13s %8.3f ms  [%.3f - %.3f]" % ((k,) + row[k]))
            row["nhwc_faster_than_copies"] = row["nhwc"][0] < row["copies"][0]
            row["ranges_apart"] = apart(row["nhwc"], row["copies"])
            say("    nhwc / copies = %.2f (ranges apart: %s)   nhwc / nchw = %.2f   train / train_copies = %.2f (ranges apart: %s)" % (
                row["nhwc"][0] / row["copies"][0], row["ranges_apart"], row["nhwc"][0] / row["nchw"][0],
                row["train"][0] / row["train_copies"][0], apart(row["train"], row["train_copies"])))
            if "direct" in row:
                say("    staged / direct = %.2f (ranges apart: %s)" % (row["nhwc"][0] / row["direct"][0], apart(row["nhwc"], row["direct"])))
            result["rows"].append(row)
            flush()
            del fns
            torch.cuda.empty_cache()
    flush()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
