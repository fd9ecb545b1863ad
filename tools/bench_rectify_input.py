"""rectifyNet's input: fused.rectify_inputs (the warps written straight into the concatenated tensor) against the composition
it replaces -- fused.FilterInterpolate per time offset + fused.FilterInterpolate_ctx_all + torch.cat
(networks/DAIN_slowmotion.py:167-181) -- on the GPU:

  slowmo1080  padded 1080p (1152 x 1984), B = 1, three time offsets, 196 context channels (437-channel inputs), forward
  dain1080    the same frames without context tensors (networks/DAIN.py:264-268: 45 channels), one time offset, forward
  vimeo       B = 3, 256 x 448, one time offset, 196 context channels, forward and forward + backward (every input trains;
              the loss uses the buffer and cur_output)

Device events; the two implementations alternate inside one process, after a warm-up, and every number is the median of
--reps repetitions of --iters calls with the spread (min-max) beside it.  `cat_bytes` is what the composition's torch.cat
moves (read + write of every channel) and rectify_inputs' copy_ still moves (the 36 flow and filter channels).

    python tools/bench_rectify_input.py [--reps 7] [--iters 10] [--warmup 3] [--only NAME]
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
from vfidkr_amd import synthetic as S  # noqa: E402


def composition(ref0, ref2, offsets, filt, times, ctx0, ctx2):
    warped = fused.FilterInterpolate_ctx_all(ctx0, ctx2, offsets, filt) if ctx0 is not None else None
    out = []
    for i, t in enumerate(times):
        off = [offsets[0][i], offsets[1][i]]
        cur, r0, r2 = fused.FilterInterpolate(ref0, ref2, off, filt, 16, t)
        parts = [cur, r0, r2, off[0], off[1], filt[0], filt[1]] + (list(warped[i]) if warped is not None else [])
        out.append((torch.cat(parts, dim=1), cur))
    return out


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def case_impls(B, H, W, times, cctx, train, gen, dev):
    ref0, ref2 = S.frames(B, H, W, gen).to(dev), S.frames(B, H, W, gen).to(dev)
    offsets = [[S.flow(B, H, W, 2.0 * (t if d == 0 else 1.0 - t) + 0.5, gen, "smooth").to(dev) for t in times] for d in (0, 1)]
    filt = [S.filters(B, H, W, gen).to(dev) for _ in (0, 1)]
    ctx = [torch.randn((B, cctx, H, W), generator=gen).to(dev) for _ in (0, 1)] if cctx else [None, None]
    leaves = [ref0, ref2, *offsets[0], *offsets[1], *filt] + [c for c in ctx if c is not None]
    total = 45 + 2 * (cctx or 0)
    if train:
        for t in leaves:
            t.requires_grad_()
        wb = [torch.randn((B, total, H, W), generator=gen).to(dev) for _ in times]
        wc = [torch.randn((B, 3, H, W), generator=gen).to(dev) for _ in times]

    def run(build):
        def fn():
            pairs = build(ref0, ref2, offsets, filt, times, ctx[0], ctx[1])
            if train:
                for t in leaves:
                    t.grad = None
                loss = 0
                for (buf, cur), b, c in zip(pairs, wb, wc):
                    loss = loss + (buf * b).sum() + (cur * c).sum()
                loss.backward()
        return fn

    new = lambda r0, r2, o, f, ts, c0, c2: fused.rectify_inputs(r0, r2, o, f, 16, ts, c0, c2)      # noqa: E731
    px = B * H * W * len(times)
    return {"rectify_inputs": run(new), "composition": run(composition)}, {"cat_bytes": 8 * total * px, "copy_bytes": 8 * 36 * px}


CASES = {
    "slowmo1080 fwd": (1, 1152, 1984, [0.25, 0.5, 0.75], 196, False),
    "dain1080 fwd": (1, 1152, 1984, [0.5], None, False),
    "vimeo fwd": (3, 256, 448, [0.5], 196, False),
    "vimeo fwd+bwd": (3, 256, 448, [0.5], 196, True),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="run the cases whose name contains this")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rectify_input needs a GPU"
    dev = torch.device("cuda:0")
    gen = S.generator()
    summary = {}
    for name, (B, H, W, times, cctx, train) in CASES.items():
        if args.only and args.only not in name:
            continue
        impls, info = case_impls(B, H, W, times, cctx, train, gen, dev)
        for fn in impls.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in impls}
        for _ in range(args.reps):
            for k, fn in impls.items():                     # alternate the implementations
                ms[k].append(timed(fn, args.iters))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        print("%-15s B%d %dx%d T=%d Cctx=%s  " % (name, B, H, W, len(times), cctx) +
              "  ".join("%s %.4f ms [%.4f-%.4f]" % (k, med[k], min(ms[k]), max(ms[k])) for k in impls) +
              "  saved %.4f ms  (cat moves %.2f GB, copy_ %.2f GB)" % (med["composition"] - med["rectify_inputs"],
                                                                      info["cat_bytes"] / 1e9, info["copy_bytes"] / 1e9), flush=True)
        summary[name] = {k: {"median": round(med[k], 4), "min": round(min(ms[k]), 4), "max": round(max(ms[k]), 4)} for k in impls}
        summary[name]["speedup"] = round(med["composition"] / med["rectify_inputs"], 3)
        del impls
        torch.cuda.empty_cache()
    print(json.dumps({"bench": "rectify_input", "ms": summary, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
