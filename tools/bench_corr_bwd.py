"""Times correlation backward (both gradients, PWC-Net's configuration: pad 4, kernel 1, max displacement 4, strides 1) in
float32 and in half at the five levels of the PWC pyramid at 1080p, with device events after a warm-up, in one run.
Prints one line per level and dtype, then a JSON summary line."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vfidkr_amd  # noqa: E402,F401
from vfidkr_amd import cabi  # noqa: E402

LEVELS = ((32, 288, 496), (64, 144, 248), (96, 72, 124), (128, 36, 62), (196, 18, 31))
WARMUP, REPS = 5, 50


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS


def main():
    gen = torch.Generator().manual_seed(3)
    rows = []
    for (C, H, W) in LEVELS:
        f1 = torch.randn((1, C, H, W), generator=gen).cuda()
        f2 = torch.randn((1, C, H, W), generator=gen).cuda()
        go = torch.randn((1, 81, H, W), generator=gen).cuda()
        row = {"C": C, "H": H, "W": W}
        for name, dt in (("fp32", torch.float32), ("half", torch.float16)):
            a, b, g = f1.to(dt), f2.to(dt), go.to(dt)
            row[name + "_ms"] = round(timed(lambda: cabi.correlation_backward(a, b, g, 4, 1, 4, 1, 1)), 4)
        print("corr bwd C=%3d %3dx%3d   fp32 %8.4f ms   half %8.4f ms" % (C, H, W, row["fp32_ms"], row["half_ms"]), flush=True)
        rows.append(row)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "levels": rows}))


if __name__ == "__main__":
    main()
