"""PWC-Net warp backward: vfi_pwc_warp_backward (both gradients) and fused.warp forward + backward against torch autograd of
the reference's warp() formula (PWCNet/PWCNet.py:159-199, written out below) on the GPU, at the four warped levels of the
padded 1080p pyramid (synthetic.correlation_features: 32@288x496 ... 128@36x62) and of the Vimeo training shape (B = 3,
256x448: 64x112 ... 8x14).  Device events; the implementations alternate inside one process, after a warm-up, and every
number is the median of --reps repetitions of --iters calls with the spread (min-max) beside it.  Algorithmic bytes per
pixel: (3C + 4) x 4 (read x and grad_output, write grad_x; read the flow, write its gradient).

    python tools/bench_warp_bwd.py [--reps 7] [--iters 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vfidkr_amd  # noqa: E402,F401
from vfidkr_amd import cabi, fused  # noqa: E402
from vfidkr_amd import synthetic as S  # noqa: E402

PEAK = 8.0e12                                               # HBM bytes/s of the MI355X


def torch_warp(x, flo):
    """the reference's warp(), align_corners=True (the grid_sample of torch <= 1.2 it was written for)"""
    B, C, H, W = x.size()
    xx = torch.arange(0, W, device=x.device).view(1, -1).repeat(H, 1).view(1, 1, H, W).repeat(B, 1, 1, 1)
    yy = torch.arange(0, H, device=x.device).view(-1, 1).repeat(1, W).view(1, 1, H, W).repeat(B, 1, 1, 1)
    vgrid = torch.cat((xx, yy), 1).float() + flo
    vgrid[:, 0, :, :] = 2.0 * vgrid[:, 0, :, :].clone() / max(W - 1, 1) - 1.0
    vgrid[:, 1, :, :] = 2.0 * vgrid[:, 1, :, :].clone() / max(H - 1, 1) - 1.0
    vgrid = vgrid.permute(0, 2, 3, 1)
    output = torch.nn.functional.grid_sample(x, vgrid, align_corners=True)
    mask = torch.ones(x.size(), device=x.device)
    mask = torch.nn.functional.grid_sample(mask, vgrid, align_corners=True)
    mask[mask < 0.9999] = 0
    mask[mask > 0] = 1
    return output * mask


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def level_impls(x, flo, g):
    gx, gf = torch.zeros_like(x), torch.empty_like(flo)

    def new_bwd():
        gx.zero_()                                          # (grad_x is added into)
        if cabi.pwc_warp_backward(x, flo, g, gx, gf, True) != 0:
            raise RuntimeError("pwc_warp_backward failed")

    xr, fr = x.clone().requires_grad_(True), flo.clone().requires_grad_(True)

    def new_fwd_bwd():
        xr.grad = fr.grad = None
        fused.warp(xr, fr).backward(g)

    xt, ft = x.clone().requires_grad_(True), flo.clone().requires_grad_(True)
    out_t = torch_warp(xt, ft)

    def torch_bwd():
        xt.grad = ft.grad = None
        out_t.backward(g, retain_graph=True)

    def torch_fwd_bwd():
        xt.grad = ft.grad = None
        torch_warp(xt, ft).backward(g)

    return {"new_bwd": new_bwd, "torch_bwd": torch_bwd, "new_fwd_bwd": new_fwd_bwd, "torch_fwd_bwd": torch_fwd_bwd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_warp_bwd needs a GPU"
    dev = torch.device("cuda:0")
    gen = S.generator()
    pyramids = {"1080p": (1, 1152, 1984), "vimeo_b3": (3, 256, 448)}
    summary = {}
    for name, (B, H, W) in pyramids.items():
        tot = {}
        for f1, f2 in S.correlation_features(B, H, W, gen)[1:]:      # the warped levels (not the 196-channel one)
            b, c, h, w = f2.shape
            x = f2.to(dev)
            flo = (torch.randn((b, 2, h, w), generator=gen) * 2.0).to(dev)
            g = torch.randn((b, c, h, w), generator=gen).to(dev)
            impls = level_impls(x, flo, g)
            for fn in impls.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in impls}
            for _ in range(args.reps):
                for k, fn in impls.items():                 # alternate the implementations
                    ms[k].append(timed(fn, args.iters))
            med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
            byt = (3 * c + 4) * 4 * b * h * w
            gbs = byt / (med["new_bwd"] * 1e-3) / 1e9
            print("%-9s %3d@%dx%d B%d  " % (name, c, h, w, b) +
                  "  ".join("%s %.4f ms [%.4f-%.4f]" % (k, med[k], min(ms[k]), max(ms[k])) for k in impls) +
                  "  new_bwd %.0f GB/s (%.1f%% of 8 TB/s)" % (gbs, 100.0 * gbs * 1e9 / PEAK), flush=True)
            for k in impls:
                t = tot.setdefault(k, [0.0, 0.0, 0.0])
                t[0] += med[k]
                t[1] += min(ms[k])
                t[2] += max(ms[k])
        print("%-9s sum of levels: " % name + "  ".join("%s %.4f ms [%.4f-%.4f]" % (k, v[0], v[1], v[2]) for k, v in tot.items()),
              flush=True)
        summary[name] = {k: round(v[0], 4) for k, v in tot.items()}
        summary[name]["bwd_speedup_vs_torch"] = round(tot["torch_bwd"][0] / tot["new_bwd"][0], 2)
    print(json.dumps({"bench": "warp_bwd", "ms": summary, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
