"""The context warp (FilterInterpolate_ctx, C = 196, fs = 4) on channels_last tensors beside what a channels_last network had to do
before, in one process: one direction at padded 1080p (B = 1, 1152x1984, the three time offsets of a x4 slow-motion step) and
at DAIN's training shape (B = 3, 256x448, one offset), float32 and bfloat16, forward only:

  (a) nhwc    the new call: channels_last context in, channels_last outputs (vfi_filterinterp_forward_ori_nhwc_multi_to[_bf16])
  (b) copies  today's composition: .contiguous() of the context, the NCHW entry, .contiguous(memory_format=channels_last)
              of every output
  (c) nchw    the NCHW entry alone on NCHW tensors (reported, no requirement)
There is no (d) any more: the LDS-staged kernel was timed against the direct one with this tool, lost and
is not in the library, which ships one NHWC kernel per filter-size class.

Flows: the smooth field of the other FilterInterpolation tools, and -- for information -- the literal quarter-resolution field
(vfidkr_amd.synthetic.flow(..., "quarter"), an independent draw per 4x4 block).  The variants alternate inside every
repetition after a warm-up (run hot); a sample is --iters calls between two device events; each figure is the median of
--reps samples with their range [min - max], in milliseconds per call.  `apart`: the two ranges do not overlap.  Prints one
block per shape, dtype and flow, then a JSON line.

    python tools/bench_fi_nhwc.py [--reps 7] [--iters 5] [--warmup 2] [--out profiles/fi_nhwc_bench.txt]
                                [--shapes 1080p,vimeo] [--flows smooth,quarter] [--lib <pkg>/lib_vX/libvfi_hip.so]
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
from vfidkr_amd import fused, synthetic  # noqa: E402

C = 196
SHAPES = (("1080p", 1, 1152, 1984, (0.25, 0.5, 0.75)), ("vimeo", 3, 256, 448, (0.5,)))
CL = torch.channels_last


def smooth_flow(B, H, W, t):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    f = torch.stack([6.0 * torch.sin(xx / 97.0 + yy / 131.0) + 1.3, 5.0 * torch.cos(xx / 113.0 - yy / 71.0) - 0.7])
    return (f * t)[None].repeat(B, 1, 1, 1).contiguous().cuda()


def quarter_flow(B, H, W, t, name):
    sigma = synthetic.FLOW_SIGMA.get(name, 2.0)
    return (synthetic.flow(B, H, W, sigma, synthetic.generator(), "quarter") * (2.0 * t)).contiguous().cuda()


def variants(name, B, H, W, offsets, dtype, flow_kind):
    gen = torch.Generator().manual_seed(5)
    ctx = torch.rand((B, C, H, W), generator=gen).cuda().to(dtype)
    ctx_cl = ctx.contiguous(memory_format=CL)
    if flow_kind == "smooth":
        flows = [smooth_flow(B, H, W, 2.0 * t) for t in offsets]           # (the projected flow of time offset t)
    else:
        flows = [quarter_flow(B, H, W, t, name) for t in offsets]
    filt = torch.softmax(torch.randn((B, 16, H, W), generator=gen), 1).cuda()

    def nhwc():
        with torch.no_grad():
            return fused._ctx_warp(ctx_cl, flows, filt)

    def copies():
        with torch.no_grad():
            return [o.contiguous(memory_format=CL) for o in fused._ctx_warp(ctx_cl.contiguous(), flows, filt)]

    def nchw():
        with torch.no_grad():
            return fused._ctx_warp(ctx, flows, filt)

    # (what is timed computes the same thing: checked once, outside the timed window)
    a, b = nhwc(), copies()
    for x, y in zip(a, b):
        assert x.stride() == y.stride() and x.stride(1) == 1
        assert torch.equal(x.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                           y.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), "nhwc and copies differ"
    return {"nhwc": nhwc, "copies": copies, "nchw": nchw}


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
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--shapes", default="1080p,vimeo")
    ap.add_argument("--flows", default="smooth,quarter")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fi_nhwc.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters, "rows": []}
    say("device: %s; median of %d x %d calls [min - max], ms per call (one direction, all time offsets)" % (
        result["device"], args.reps, args.iters))
    for name, B, H, W, offsets in (s for s in SHAPES if s[0] in args.shapes.split(",")):
        for dtype in (torch.float32, torch.bfloat16):
            for flow_kind in args.flows.split(","):
                dn = str(dtype).replace("torch.", "")
                row = {"shape": name, "B": B, "C": C, "H": H, "W": W, "offsets": len(offsets), "dtype": dn, "flow": flow_kind}
                say("%s  B=%d C=%d %dx%d, %d time offset(s), %s, %s flow" % (name, B, C, H, W, len(offsets), dn, flow_kind))
                fns = variants(name, B, H, W, offsets, dtype, flow_kind)
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
                    say("    %-7s %8.3f ms  [%.3f - %.3f]" % ((k,) + row[k]))
                row["nhwc_faster_than_copies"] = row["nhwc"][0] < row["copies"][0]
                row["ranges_apart"] = row["nhwc"][2] < row["copies"][1] or row["copies"][2] < row["nhwc"][1]
                say("    nhwc / copies = %.2f (ranges apart: %s)   nhwc / nchw = %.2f   per offset: nhwc %.3f ms, nchw %.3f ms" % (
                    row["nhwc"][0] / row["copies"][0], row["ranges_apart"], row["nhwc"][0] / row["nchw"][0],
                    row["nhwc"][0] / len(offsets), row["nchw"][0] / len(offsets)))
                result["rows"].append(row)
                del fns
                torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
