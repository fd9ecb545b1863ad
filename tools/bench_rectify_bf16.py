"""rectifyNet's input for a network under bfloat16 autocast: fused.rectify_inputs(dtype=torch.bfloat16) -- one head launch per
time offset, the context warps written as bfloat16 straight into the buffer -- against the two ways such a network could
build the same bfloat16 tensor before:

  cat    fused.FilterInterpolate per time offset + fused.FilterInterpolate_ctx_all on the bfloat16 contexts + torch.cat (which
         promotes to float32) + .to(torch.bfloat16)
  f32    .float() of the contexts + fused.rectify_inputs (float32) + .to(torch.bfloat16)

on the GPU, forward and forward + backward (frames, flows, filters and contexts train; the gradients arriving at the buffers
are bfloat16, those at cur_output float32):

  slowmo1080  padded 1080p (1152 x 1984), B = 1, three time offsets, 196 context channels (437-channel buffers)
  vimeo       B = 3, 256 x 448, one time offset, 196 context channels
  ... nocontext: the same two without context tensors (45 channels)
  head        the head launch alone (vfi_rectify_head_forward_bf16 into preallocated tensors) against
              vfi_filterinterp_blend_forward + four copy_ into a float32 45-channel buffer + .to(torch.bfloat16)

Device events; the variants alternate inside one process, after a warm-up, and every number is the median of --reps samples of
--iters calls with the range (min-max) beside it.

    python tools/bench_rectify_bf16.py [--reps 7] [--iters 5] [--warmup 2] [--only NAME]
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

BF = torch.bfloat16


def build_bf16(ref0, ref2, offsets, filt, times, ctx0, ctx2):
    return fused.rectify_inputs(ref0, ref2, offsets, filt, 16, times, ctx0, ctx2, dtype=BF)


def build_cat(ref0, ref2, offsets, filt, times, ctx0, ctx2):
    warped = fused.FilterInterpolate_ctx_all(ctx0, ctx2, offsets, filt) if ctx0 is not None else None
    out = []
    for i, t in enumerate(times):
        off = [offsets[0][i], offsets[1][i]]
        cur, r0, r2 = fused.FilterInterpolate(ref0, ref2, off, filt, 16, t)
        parts = [cur, r0, r2, off[0], off[1], filt[0], filt[1]] + (list(warped[i]) if warped is not None else [])
        out.append((torch.cat(parts, dim=1).to(BF), cur))
    return out


def build_f32(ref0, ref2, offsets, filt, times, ctx0, ctx2):
    wide = lambda t: None if t is None else t.float()      # noqa: E731
    return [(buf.to(BF), cur) for buf, cur in fused.rectify_inputs(ref0, ref2, offsets, filt, 16, times, wide(ctx0), wide(ctx2))]


BUILDERS = {"bf16": build_bf16, "cat": build_cat, "f32": build_f32}


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def inputs(B, H, W, times, cctx, gen, dev):
    ref0, ref2 = S.frames(B, H, W, gen).to(dev), S.frames(B, H, W, gen).to(dev)
    offsets = [[S.flow(B, H, W, 2.0 * (t if d == 0 else 1.0 - t) + 0.5, gen, "smooth").to(dev) for t in times] for d in (0, 1)]
    filt = [S.filters(B, H, W, gen).to(dev) for _ in (0, 1)]
    ctx = [torch.randn((B, cctx, H, W), generator=gen).to(dev).to(BF) for _ in (0, 1)] if cctx else [None, None]
    return ref0, ref2, offsets, filt, ctx


def case_impls(B, H, W, times, cctx, train, gen, dev):
    ref0, ref2, offsets, filt, ctx = inputs(B, H, W, times, cctx, gen, dev)
    leaves = [ref0, ref2, *offsets[0], *offsets[1], *filt] + [c for c in ctx if c is not None]
    total = 45 + 2 * (cctx or 0)
    if train:
        for t in leaves:
            t.requires_grad_()
        gb = [torch.randn((B, total, H, W), generator=gen).to(dev).to(BF) for _ in times]
        gc = [torch.randn((B, 3, H, W), generator=gen).to(dev) for _ in times]

    def run(build):
        def fn():
            pairs = build(ref0, ref2, offsets, filt, times, ctx[0], ctx[1])
            if train:
                for t in leaves:
                    t.grad = None
                torch.autograd.backward([x for pair in pairs for x in pair], [g for pair in zip(gb, gc) for g in pair])
        return fn
    return {k: run(b) for k, b in BUILDERS.items()}


def head_impls(B, H, W, gen, dev):
    ref0, ref2, offsets, filt, _ = inputs(B, H, W, [0.5], None, gen, dev)
    f0, f2 = offsets[0][0], offsets[1][0]
    buf, cur = torch.empty((B, 45, H, W), device=dev, dtype=BF), torch.empty((B, 3, H, W), device=dev)
    wide = torch.empty((B, 45, H, W), device=dev)

    def head():
        assert cabi.rectify_head_forward_bf16(ref0, ref2, f0, f2, filt[0], filt[1], buf, cur, 0.5, 0.5) == 0

    def blend_copies_cast():
        assert cabi.filterinterp_blend_forward(ref0, ref2, f0, f2, filt[0], filt[1], wide[:, 0:3], wide[:, 3:6], wide[:, 6:9], 0.5, 0.5) == 0
        wide[:, 9:11].copy_(f0), wide[:, 11:13].copy_(f2), wide[:, 13:29].copy_(filt[0]), wide[:, 29:45].copy_(filt[1])
        return wide.to(BF)
    return {"head": head, "blend+4 copy_+cast": blend_copies_cast}


P1080, VIMEO = (1, 1152, 1984), (3, 256, 448)
CASES = {
    "slowmo1080 fwd": (*P1080, [0.25, 0.5, 0.75], 196, False),
    "slowmo1080 fwd+bwd": (*P1080, [0.25, 0.5, 0.75], 196, True),
    "vimeo fwd": (*VIMEO, [0.5], 196, False),
    "vimeo fwd+bwd": (*VIMEO, [0.5], 196, True),
    "slowmo1080 nocontext fwd": (*P1080, [0.25, 0.5, 0.75], None, False),
    "slowmo1080 nocontext fwd+bwd": (*P1080, [0.25, 0.5, 0.75], None, True),
    "vimeo nocontext fwd": (*VIMEO, [0.5], None, False),
    "vimeo nocontext fwd+bwd": (*VIMEO, [0.5], None, True),
    "head 1080": (*P1080, None, None, False),
    "head vimeo": (*VIMEO, None, None, False),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, help="run the cases whose name contains this")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rectify_bf16 needs a GPU"
    dev = torch.device("cuda:0")
    gen = S.generator()
    summary = {}
    for name, (B, H, W, times, cctx, train) in CASES.items():
        if args.only and args.only not in name:
            continue
        impls = head_impls(B, H, W, gen, dev) if times is None else case_impls(B, H, W, times, cctx, train, gen, dev)
        for fn in impls.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in impls}
        for _ in range(args.reps):
            for k, fn in impls.items():                     # alternate the variants
                ms[k].append(timed(fn, args.iters))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        shape = "B%d %dx%d" % (B, H, W) + ("" if times is None else " T=%d Cctx=%s" % (len(times), cctx))
        print("%-29s %-28s " % (name, shape) + "  ".join("%s %.4f ms [%.4f-%.4f]" % (k, med[k], min(ms[k]), max(ms[k])) for k in impls),
              flush=True)
        summary[name] = {k: {"median": round(med[k], 4), "min": round(min(ms[k]), 4), "max": round(max(ms[k]), 4)} for k in impls}
        del impls
        torch.cuda.empty_cache()
    print(json.dumps({"bench": "rectify_bf16", "ms": summary, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
