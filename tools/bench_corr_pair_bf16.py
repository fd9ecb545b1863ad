"""Times the paired correlation on bfloat16 tensors (PWC-Net's configuration: pad 4, kernel 1, max displacement 4, strides 1)
beside what it replaces, in one process, at the five PWC pyramid levels of a 1080p pair (batch 1) and of a Vimeo batch
(B = 3) -- the ten levels of tools/bench_corr_bf16.py -- for four operations of a level of a frame pair's two flow networks:

  fwd         both cost volumes                      lrelu fwd   the same with the LeakyReLU (slope 0.1)
  bwd 4       all four gradients                     bwd 2       only the two gradInput2 (the first features frozen)

and three columns:

  pair        ONE call of the bfloat16 pair entry (cabi.correlation_[lrelu_]forward_pair / _backward_pair on bfloat16 tensors):
              one launch
  singles     the single bfloat16 entries it replaces, the yardstick: two forward calls (two launches); two backward calls
              (four launches -- the single entry always computes both gradients, so `bwd 2` has the same yardstick as `bwd 4`)
  f32 pair    the float32 pair entry on the same values, for information

Method: a block is --iters calls of one column between two device events with nothing in between (no per-call event: the
figure is the steady per-call time of a stream of launches); the blocks of the three columns alternate --reps times after a
warm-up, so all see the same machine.  Each figure is the median of the --reps blocks with their range (min .. max),
microseconds per call.  hot: the same tensors every call (they stay in the caches).  cold: every call takes the next set of
a ring of tensor sets of at least 320 MB of bfloat16 (larger than the 256 MB Infinity Cache) where 256 sets reach that -- the
four finest 1080p levels and the three finest Vimeo levels; the three coarsest levels' rings stay below it (`cold_ring_mb`
in the summary), so their cold figure only means other addresses every call.  Outputs are allocated by the wrappers (the caching allocator), the same in every column.
Prints one line per level, operation and temperature, the five-level sums of the medians, then a JSON summary line.

    python tools/bench_corr_pair_bf16.py [--reps 7] [--iters 20] [--warmup 5]
    python tools/bench_corr_pair_bf16.py --launches     # every pair operation once per level and nothing else: run under a
                                                        # kernel trace to count launches (one per operation and level)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vfidkr_amd  # noqa: E402,F401
from vfidkr_amd import cabi  # noqa: E402
from tools.bench_corr_bf16 import LEVELS  # noqa: E402

PWC = (4, 1, 4, 1, 1)
SLOPE = 0.1
COLD_BYTES = 320 << 20
MAX_SETS = 256
SECOND = (False, True, False, True)


def tensor_set(B, C, H, W, dtype, gen):
    """(a1, a2, b1, b2, ga, gb, ya, yb): item b is item a swapped, as at the top level of the two flow networks"""
    a1, a2 = (torch.randn((B, C, H, W), generator=gen, device="cuda").to(dtype) for _ in range(2))
    ga, gb = (torch.randn((B, 81, H, W), generator=gen, device="cuda").to(dtype) for _ in range(2))
    ya, yb = cabi.correlation_lrelu_forward_pair(a1, a2, a2, a1, *PWC, SLOPE)
    return a1, a2, a2, a1, ga, gb, ya, yb


def operations():
    """name -> {column -> fn(tensor set)}"""
    def fwd_pair(s):
        cabi.correlation_forward_pair(*s[:4], *PWC)

    def fwd_singles(s):
        cabi.correlation_forward(s[0], s[1], *PWC)
        cabi.correlation_forward(s[2], s[3], *PWC)

    def lrelu_pair(s):
        cabi.correlation_lrelu_forward_pair(*s[:4], *PWC, SLOPE)

    def lrelu_singles(s):
        cabi.correlation_lrelu_forward(s[0], s[1], *PWC, SLOPE)
        cabi.correlation_lrelu_forward(s[2], s[3], *PWC, SLOPE)

    def bwd_pair(want):
        return lambda s: cabi.correlation_backward_pair(s[0], s[1], s[4], s[2], s[3], s[5], *PWC, want=want)

    def bwd_singles(s):
        cabi.correlation_backward(s[0], s[1], s[4], *PWC)
        cabi.correlation_backward(s[2], s[3], s[5], *PWC)

    return {"fwd": {"pair": fwd_pair, "singles": fwd_singles, "f32 pair": fwd_pair},
            "lrelu fwd": {"pair": lrelu_pair, "singles": lrelu_singles, "f32 pair": lrelu_pair},
            "bwd 4": {"pair": bwd_pair((True,) * 4), "singles": bwd_singles, "f32 pair": bwd_pair((True,) * 4)},
            "bwd 2": {"pair": bwd_pair(SECOND), "singles": bwd_singles, "f32 pair": bwd_pair(SECOND)}}


def block(fn, sets, first, iters):
    """iters calls between two device events: microseconds per call"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(sets[(first + i) % len(sets)])
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def measure(columns, sets, args):
    """{column: (median, min, max)} of args.reps alternating blocks; sets: {column: its ring of tensor sets}"""
    for name, fn in columns.items():
        for i in range(args.warmup):
            fn(sets[name][i % len(sets[name])])
    torch.cuda.synchronize()
    times, at = {name: [] for name in columns}, 0
    for _ in range(args.reps):
        for name, fn in columns.items():
            times[name].append(block(fn, sets[name], at, args.iters))
        at += args.iters
    out = {}
    for name, t in times.items():
        t.sort()
        out[name] = (round(t[len(t) // 2], 1), round(t[0], 1), round(t[-1], 1))
    return out


def launches():
    gen = torch.Generator(device="cuda").manual_seed(3)
    for pyramid, (B, levels) in LEVELS.items():
        for (C, H, W) in levels:
            a1, a2 = (torch.randn((B, C, H, W), generator=gen, device="cuda").bfloat16() for _ in range(2))
            ga, gb = (torch.randn((B, 81, H, W), generator=gen, device="cuda").bfloat16() for _ in range(2))
            cabi.correlation_forward_pair(a1, a2, a2, a1, *PWC)
            ya, yb = cabi.correlation_lrelu_forward_pair(a1, a2, a2, a1, *PWC, SLOPE)
            cabi.correlation_backward_pair(a1, a2, ga, a2, a1, gb, *PWC)
            cabi.correlation_lrelu_backward_pair(a1, a2, ya, ga, a2, a1, yb, gb, *PWC, SLOPE, want=SECOND)
    torch.cuda.synchronize()
    print("launches: 10 levels x (forward pair, lrelu forward pair, backward pair with four gradients, lrelu backward pair "
          "with two): 20 forward and 20 backward calls")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_corr_pair_bf16.py needs a GPU")
    if args.launches:
        return launches()
    gen = torch.Generator(device="cuda").manual_seed(3)
    ops = operations()
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters, "levels": [], "sums": {}}
    for pyramid, (B, levels) in LEVELS.items():
        sums = {}
        for (C, H, W) in levels:
            per_set = (2 * B * C * H * W + 4 * B * 81 * H * W) * 2                 # bytes of a bfloat16 set, its outputs aside
            nsets = min(max(2, -(-COLD_BYTES // per_set)), MAX_SETS)
            rings = {}
            for dtype in (torch.bfloat16, torch.float32):
                rings[dtype] = [tensor_set(B, C, H, W, dtype, gen) for _ in range(nsets)]
            by_column = {"pair": rings[torch.bfloat16], "singles": rings[torch.bfloat16], "f32 pair": rings[torch.float32]}
            row = {"pyramid": pyramid, "B": B, "C": C, "H": H, "W": W, "cold_sets": nsets, "cold_ring_mb": round(nsets * per_set / 2 ** 20)}
            for op, columns in ops.items():
                for temp in ("hot", "cold"):
                    sets = by_column if temp == "cold" else {k: v[:1] for k, v in by_column.items()}
                    got = measure(columns, sets, args)
                    row["%s %s" % (op, temp)] = got
                    for name, v in got.items():
                        sums[(op, temp, name)] = sums.get((op, temp, name), 0.0) + v[0]
                    print("%s B=%d C=%3d %3dx%3d  %-9s %-4s  " % (pyramid, B, C, H, W, op, temp) +
                          "   ".join("%s %7.1f (%.1f .. %.1f)" % ((name,) + v) for name, v in got.items()), flush=True)
            result["levels"].append(row)
            del rings, by_column
            torch.cuda.empty_cache()
        for op in ops:
            for temp in ("hot", "cold"):
                print("%s five-level sum  %-9s %-4s  " % (pyramid, op, temp) +
                      "   ".join("%s %7.1f" % (name, sums[(op, temp, name)]) for name in ("pair", "singles", "f32 pair")), flush=True)
        result["sums"][pyramid] = {"%s %s %s" % k: round(v, 1) for k, v in sums.items()}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
