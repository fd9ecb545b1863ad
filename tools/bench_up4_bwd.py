"""Backward through the quarter-resolution flow: vfi_[depth]flowprojection_backward_up4 (one fused call for all time offsets)
and fused.FlowProject_from_quarter forward + backward, against
  * the composition a trainer had before them: torch.nn.Upsample(scale_factor=4, mode='bilinear')(div_flow * flow_q * t), then
    fused.FlowProject, under torch autograd (zero fill, proj_backward, upsample_bilinear2d_backward with atomics and the two
    scalar-multiply backwards, per time offset);
  * the library's own two-call backward: vfi_[depth]flowprojection_backward into zeros per time offset, then ONE
    vfi_flow_upsample4_backward (the full-resolution flows are formed before the clock starts).
Shapes: padded 1080p (quarter 288 x 496, B = 1, the three time offsets of the x4 slow-motion step, without and with depth) and the
Vimeo batch (B = 3, quarter 64 x 112, one time offset, no depth).  Device events around --iters calls, every window ended in a
synchronise; the sides alternate inside one process after a warm-up; --reps repetitions, median and min-max of each.

    python tools/bench_up4_bwd.py [--reps 5] [--iters 20] [--warmup 5]
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

DIV_FLOW = 20.0
SHAPES = [("1080p", 1, 288, 496, [0.25, 0.5, 0.75], False), ("1080p_depth", 1, 288, 496, [0.25, 0.5, 0.75], True),
          ("vimeo_b3", 3, 64, 112, [0.5], False)]


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def check(err):
    if err != 0:
        raise RuntimeError("the binding returned %d" % err)


def torch_composition(flow_q, ts, depth):
    up = torch.nn.Upsample(scale_factor=4, mode="bilinear")
    return fused.FlowProject([up(DIV_FLOW * flow_q * t) for t in ts], depth, fillhole=False)


def shape_impls(B, hq, wq, ts, with_depth, gen, dev):
    n, H, W = len(ts), 4 * hq, 4 * wq
    flow_q = (torch.randn((B, 2, hq, wq), generator=gen) * 0.1).to(dev)
    depth = (torch.rand((B, 1, H, W), generator=gen) * 0.9 + 0.1).to(dev) if with_depth else None
    gs = [torch.randn((B, 2, H, W), generator=gen).to(dev) for _ in ts]
    full, counts, outs = [], [], []
    for t in ts:
        F, count, out = torch.empty((B, 2, H, W), device=dev), torch.empty((B, 1, H, W), device=dev), torch.empty((B, 2, H, W), device=dev)
        check(cabi.flow_upsample4(flow_q, F, DIV_FLOW, t))
        check(cabi.flowprojection_forward(F, count, out, 0) if depth is None else
              cabi.depthflowprojection_forward(F, depth, count, out, 0))
        full.append(F), counts.append(count), outs.append(out)
    gq = torch.empty_like(flow_q)
    gds = [torch.empty_like(depth) for _ in ts] if with_depth else None
    Gs = [torch.empty_like(F) for F in full]

    def fused_bwd():
        check(cabi.flowprojection_backward_up4(flow_q, counts, gs, DIV_FLOW, ts, gq, depth, outs if with_depth else None, gds))

    def two_call_bwd():
        for i in range(n):
            Gs[i].zero_()
            if with_depth:
                gds[i].zero_()
                check(cabi.depthflowprojection_backward(full[i], depth, counts[i], outs[i], gs[i], Gs[i], gds[i]))
            else:
                check(cabi.flowprojection_backward(full[i], counts[i], gs[i], Gs[i]))
        check(cabi.flow_upsample4_backward(Gs, DIV_FLOW, ts, gq))

    qt = flow_q.clone().requires_grad_(True)
    dt = depth.clone().requires_grad_(True) if with_depth else None
    graph_t = torch_composition(qt, ts, dt)

    def clear(*tensors):
        for t in tensors:
            if t is not None:
                t.grad = None

    def torch_bwd():
        clear(qt, dt)
        torch.autograd.backward(graph_t, gs, retain_graph=True)

    def torch_fwd_bwd():
        clear(qt, dt)
        torch.autograd.backward(torch_composition(qt, ts, dt), gs)

    qn = flow_q.clone().requires_grad_(True)
    dn = depth.clone().requires_grad_(True) if with_depth else None

    def new_fwd_bwd():
        clear(qn, dn)
        torch.autograd.backward(fused.FlowProject_from_quarter(qn, DIV_FLOW, ts, dn, fillhole=False), gs)

    # the sides agree before they are timed (torch's composition to rounding: its upsample backward sums in another order)
    fused_bwd()
    a = gq.clone()
    two_call_bwd()
    assert torch.equal(a, gq), "fused and two-call backward differ"
    torch_bwd()
    scale = float(a.abs().max())
    assert float((qt.grad - a).abs().max()) <= 1e-3 * max(scale, 1.0), "torch composition and fused backward differ"
    return {"fused_bwd": fused_bwd, "two_call_bwd": two_call_bwd, "torch_bwd": torch_bwd, "new_fwd_bwd": new_fwd_bwd,
            "torch_fwd_bwd": torch_fwd_bwd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_up4_bwd needs a GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1234)
    summary = {}
    for name, B, hq, wq, ts, with_depth in SHAPES:
        impls = shape_impls(B, hq, wq, ts, with_depth, gen, dev)
        for fn in impls.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in impls}
        for _ in range(args.reps):
            for k, fn in impls.items():                     # alternate the sides
                ms[k].append(timed(fn, args.iters))
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        print("%-12s quarter %dx%d B%d x%d  " % (name, hq, wq, B, len(ts)) +
              "  ".join("%s %.4f ms [%.4f-%.4f]" % (k, med[k], min(ms[k]), max(ms[k])) for k in impls), flush=True)
        summary[name] = {k: {"median": round(med[k], 4), "min": round(min(ms[k]), 4), "max": round(max(ms[k]), 4)} for k in impls}
        summary[name]["fused_slowest_below_two_call_fastest"] = max(ms["fused_bwd"]) < min(ms["two_call_bwd"])
        summary[name]["bwd_speedup_vs_torch"] = round(med["torch_bwd"] / med["fused_bwd"], 2)
        summary[name]["fwd_bwd_speedup_vs_torch"] = round(med["torch_fwd_bwd"] / med["new_fwd_bwd"], 2)
    print(json.dumps({"bench": "up4_bwd", "ms": summary, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
