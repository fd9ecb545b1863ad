"""Times one PWC-Net level's block -- warp, correlation, LeakyReLU, concatenation -- on bfloat16 tensors beside what a
bfloat16 user had to write before, in one process, at the pyramid levels of a 1080p pair (batch 1) and of a Vimeo batch (B = 3)
that have a warp (the finest four of each; the coarsest level correlates without one), forward and forward + backward:

  a     fused.warp_corr_lrelu(c1, c2, flo, out=buf[:, :81]) on bfloat16 tensors: two launches on bfloat16 storage, the
        activated cost volume written into its slice of the concatenation buffer.  Under autograd (out= is for inference):
        torch.cat((fused.warp_corr_lrelu(c1, c2, flo), c1, flo), 1) and its backward.
  a+cp  forward only: leg a plus the copy_ of c1 and of the flow into the rest of the buffer, so that it ends with the
        same tensor as leg b (a network whose layers write into the buffer themselves does not pay these)
  b     the same tensor as a bfloat16 user wrote it before the warp and the fused LeakyReLU took bfloat16:
        torch.cat((F.leaky_relu(_Corr.apply(c1, warp(c2.float(), flo.float()).to(c1.dtype)), 0.1), c1, flo), 1)
  c     leg a on float32 copies of the tensors, for orientation

on random data, hot (the same tensors again and again).  The method of bench_corr_bf16.py's `choice` lines: a block is CALLS
calls of one leg between two device events with nothing in between, the legs' blocks alternate ROUNDS times in one go so
that all see the same machine; a figure is the median of the rounds with [min-max], microseconds per call.  The flow is
bfloat16 in legs a and b (what a flow head gives under autocast).  Prints one line per level and mode, then a JSON summary
line."""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vfidkr_amd  # noqa: E402,F401
from vfidkr_amd import fused  # noqa: E402

LEVELS = {"1080p": (1, ((32, 288, 496), (64, 144, 248), (96, 72, 124), (128, 36, 62))),
          "vimeo": (3, ((32, 64, 112), (64, 32, 56), (96, 16, 28), (128, 8, 14)))}
WARMUP, ROUNDS, CALLS = 5, 9, 20
SLOPE = 0.1


def unfused(c1, c2, flo):
    return F.leaky_relu(fused._Corr.apply(c1, fused.warp(c2.float(), flo.float()).to(c1.dtype)), SLOPE)


def forward_legs(c1, c2, flo):
    B, C, H, W = c1.shape
    buf = torch.empty((B, 81 + C + 2, H, W), dtype=c1.dtype, device=c1.device)
    f1, f2, ff = c1.float(), c2.float(), flo.float()
    buf32 = torch.empty((B, 81 + C + 2, H, W), dtype=torch.float32, device=c1.device)

    def a():
        fused.warp_corr_lrelu(c1, c2, flo, negative_slope=SLOPE, out=buf[:, :81])

    def a_cp():
        a()
        buf[:, 81:81 + C].copy_(c1)
        buf[:, 81 + C:].copy_(flo)

    def b():
        torch.cat((unfused(c1, c2, flo), c1, flo), 1)

    def c():
        fused.warp_corr_lrelu(f1, f2, ff, negative_slope=SLOPE, out=buf32[:, :81])

    return {"a": a, "a+cp": a_cp, "b": b, "c": c}


def training_legs(c1, c2, flo):
    B, C, H, W = c1.shape
    gy = torch.randn((B, 81 + C + 2, H, W), device=c1.device).to(c1.dtype)
    gy32 = gy.float()

    def leg(block, tensors, g):
        leaves = [t.clone().requires_grad_(True) for t in tensors]

        def run():
            for t in leaves:
                t.grad = None                               # (no accumulation launch)
            x1, x2, fl = leaves
            torch.cat((block(x1, x2, fl), x1, fl), 1).backward(g)
        return run

    new = lambda x1, x2, fl: fused.warp_corr_lrelu(x1, x2, fl, negative_slope=SLOPE)      # noqa: E731
    return {"a": leg(new, (c1, c2, flo), gy), "b": leg(unfused, (c1, c2, flo), gy),
            "c": leg(new, (c1.float(), c2.float(), flo.float()), gy32)}


def alternate(legs):
    """{leg: (median, min, max)} in microseconds per call over ROUNDS alternating blocks of CALLS calls"""
    t = {k: [] for k in legs}
    for fn in legs.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t[k].append(e0.elapsed_time(e1) * 1e3 / CALLS)
    out = {}
    for k, v in t.items():
        v.sort()
        out[k] = (round(v[len(v) // 2], 1), round(v[0], 1), round(v[-1], 1))
    return out


def main():
    gen = torch.Generator().manual_seed(5)
    result = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "calls": CALLS, "levels": []}
    for pyramid, (B, levels) in LEVELS.items():
        for (C, H, W) in levels:
            c1 = torch.randn((B, C, H, W), generator=gen).bfloat16().cuda()
            c2 = torch.randn((B, C, H, W), generator=gen).bfloat16().cuda()
            flo = (torch.randn((B, 2, H, W), generator=gen) * 3).bfloat16().cuda()
            row = {"pyramid": pyramid, "B": B, "C": C, "H": H, "W": W}
            with torch.no_grad():
                row["fwd"] = alternate(forward_legs(c1, c2, flo))
            row["fwd+bwd"] = alternate(training_legs(c1, c2, flo))
            for mode in ("fwd", "fwd+bwd"):
                r = row[mode]
                row[mode + " a below b's minimum"] = r["a"][0] < r["b"][1]
                print("%-7s %s B=%d C=%3d %3dx%3d  " % (mode, pyramid, B, C, H, W) +
                      "  ".join("%s %7.1f [%.1f-%.1f]" % ((k,) + v) for k, v in r.items()) +
                      "   a/b %.2f%s" % (r["a"][0] / r["b"][0], "" if row[mode + " a below b's minimum"] else "   (a NOT below b's minimum)"),
                      flush=True)
            result["levels"].append(row)
            del c1, c2, flo
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
