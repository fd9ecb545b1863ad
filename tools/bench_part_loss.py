"""The fused training losses (fused.part_loss: vfi_part_loss_forward / vfi_part_loss_backward) against the same formulas
written in plain torch -- what a trainer runs today (loss_function.part_loss is torch eager), on the same GPU in the same process.
Legs, each for both sides:
  fwd        the three lists of losses, no grad;
  fwd_pixel  forward, then backward of pixel_loss[1] alone (train.py's total loss with alpha = [0, 1]);
  fwd_all    forward, then backward of the sum of every loss.
Shapes: the Vimeo batch (B = 3, 256 x 448) and one 1080p frame; two diffs, one flow pair, 3-channel images.  Device events
around --iters calls, every window ended in a synchronise; the sides alternate inside one process after a warm-up; --reps
repetitions, median and min-max of each.  The 1080p forward also reports its algorithmic bytes / time against 8 TB/s; at the
Vimeo size the call is bound by its launches, not by bytes, and no fraction is quoted.

    python tools/bench_part_loss.py [--reps 5] [--iters 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vfidkr_amd  # noqa: E402,F401
from vfidkr_amd import fused  # noqa: E402

EPS = 1e-6
SHAPES = [("vimeo_b3", 3, 256, 448), ("1080p", 1, 1080, 1920)]
HBM_BYTES_PER_S = 8.0e12


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def torch_part_loss(diffs, offsets, images, eps):
    """the losses in plain torch operations, as a trainer writes them today"""
    e2 = eps * eps

    def charbonnier(x):
        return torch.mean(torch.sqrt(x * x + e2))

    def tv(flow, image):
        centre_i, centre_f = image[:, :, :-1, :-1], flow[:, :, :-1, :-1]
        edges = torch.abs(centre_i - image[:, :, 1:, :-1]) + torch.abs(centre_i - image[:, :, :-1, 1:])
        weight = torch.exp(-torch.sum(edges, dim=1))
        t = torch.sqrt((centre_f - flow[:, :, 1:, :-1]) ** 2 + (centre_f - flow[:, :, :-1, 1:]) ** 2 + e2)
        return torch.mean(weight * torch.sum(t, dim=1))

    pixel = [charbonnier(d) for d in diffs]
    offset = [tv(o[0], images[0]) + tv(o[1], images[1]) for o in offsets]
    sym = [charbonnier(o[0] + o[1]) for o in offsets]
    return pixel, offset, sym


def shape_impls(B, H, W, gen, dev):
    images = [torch.rand((B, 3, H, W), generator=gen).to(dev) for _ in range(2)]
    diffs0 = [(torch.randn((B, 3, H, W), generator=gen) * 0.1).to(dev) for _ in range(2)]
    flows0 = [(torch.randn((B, 2, H, W), generator=gen) * 3.0).to(dev) for _ in range(2)]
    sides = {"fused": lambda d, o: fused.part_loss(d, o, [None], images, EPS),
             "torch": lambda d, o: torch_part_loss(d, o, images, EPS)}
    impls, leaves = {}, {}
    for side, fn in sides.items():
        d = [t.clone().requires_grad_(True) for t in diffs0]
        f = [t.clone().requires_grad_(True) for t in flows0]
        leaves[side] = d + f

        def fwd(fn=fn, d=d, f=f):
            with torch.no_grad():
                return fn(d, [f])

        def fwd_pixel(fn=fn, d=d, f=f):
            for t in d + f:
                t.grad = None
            fn(d, [f])[0][1].backward()

        def fwd_all(fn=fn, d=d, f=f):
            for t in d + f:
                t.grad = None
            pixel, offset, sym = fn(d, [f])
            (pixel[0] + pixel[1] + offset[0] + sym[0]).backward()

        impls[side + "_fwd"], impls[side + "_fwd_pixel"], impls[side + "_fwd_all"] = fwd, fwd_pixel, fwd_all
    # the sides agree before they are timed (to float32 rounding of sums taken in different orders)
    a, b = impls["fused_fwd"](), impls["torch_fwd"]()
    for x, y in zip(a[0] + a[1] + a[2], b[0] + b[1] + b[2]):
        assert abs(float(x) - float(y)) <= 1e-4 * abs(float(y)), "the fused losses and the torch composition differ"
    impls["fused_fwd_all"](), impls["torch_fwd_all"]()
    for x, y in zip(leaves["fused"], leaves["torch"]):
        assert float((x.grad - y.grad).abs().max()) <= 1e-4 * float(y.grad.abs().max()), "the gradients differ"
    return impls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_part_loss needs a GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1234)
    summary = {}
    for name, B, H, W in SHAPES:
        impls = shape_impls(B, H, W, gen, dev)
        for fn in impls.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in impls}
        for _ in range(args.reps):
            for k, fn in impls.items():                     # alternate the sides
                ms[k].append(timed(fn, args.iters))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        print("%-9s B%d %dx%d  " % (name, B, H, W) +
              "  ".join("%s %.4f ms [%.4f-%.4f]" % (k, med[k], min(ms[k]), max(ms[k])) for k in impls), flush=True)
        summary[name] = {k: {"median": round(med[k], 4), "min": round(min(ms[k]), 4), "max": round(max(ms[k]), 4)} for k in impls}
        legs = ("fwd", "fwd_pixel", "fwd_all")
        summary[name]["fused_slowest_below_torch_fastest"] = {leg: max(ms["fused_" + leg]) < min(ms["torch_" + leg]) for leg in legs}
        summary[name]["speedup_vs_torch"] = {leg: round(med["torch_" + leg] / med["fused_" + leg], 2) for leg in legs}
        if name == "1080p":
            # every input read once: two diffs and two images of 3 channels, two flows of 2 -- 16 floats per pixel
            nbytes = 16 * 4 * B * H * W
            summary[name]["fwd_algorithmic_bytes"] = nbytes
            summary[name]["fwd_fraction_of_8TBps"] = round(nbytes / (med["fused_fwd"] * 1e-3) / HBM_BYTES_PER_S, 3)
        else:
            summary[name]["fwd_fraction_of_8TBps"] = "not quoted: launch-bound at this size"
    ok = all(all(s["fused_slowest_below_torch_fastest"].values()) for s in summary.values())
    print(json.dumps({"bench": "part_loss", "ms": summary, "fused_slowest_below_torch_fastest": ok,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
