"""Times the bfloat16 correlation (PWC-Net's configuration: pad 4, kernel 1, max displacement 4, strides 1) beside what it
replaces, in one process: at the five PWC pyramid levels of a 1080p pair (batch 1) and of a Vimeo batch (B = 3), forward,
backward and both, for

  bf16        vfi_correlation_forward_bf16 / _backward_bf16 (the dispatch's choice of kernel)
  bf16 mfma   the MFMA forward kernel, whatever the tile count      bf16 gen    the one-thread-per-output forward kernel
  fp32        vfi_correlation_forward / _backward                   f16         the _f16 entries
  cast        what a bfloat16 caller had to do before: cast up, run float32, cast down

on random data.  hot: the same tensors again and again (they stay in the caches); cold: a different set of tensors each call,
from a ring larger than the 256 MB Infinity Cache (a small level: one set per call, none used twice).  Each figure is the median of REPS samples of one call between two
device events, with the spread (10th..90th percentile); event timing adds a few microseconds per sample, the same for
every column.  Before that: the two forward kernels back to back at every level (`choice` lines: alternating blocks of
launches without per-call events -- the measurement behind corr_bf16_mfma_threshold), and a probe of what the MFMA does
with a bfloat16 subnormal input.  Prints one line per level, then a JSON
summary line."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vfidkr_amd  # noqa: E402,F401
from vfidkr_amd import cabi  # noqa: E402

LEVELS = {"1080p": (1, ((32, 288, 496), (64, 144, 248), (96, 72, 124), (128, 36, 62), (196, 18, 31))),
          "vimeo": (3, ((32, 64, 112), (64, 32, 56), (96, 16, 28), (128, 8, 14), (196, 4, 7)))}
PWC = (4, 1, 4, 1, 1)
WARMUP, REPS = 10, 100
COLD_BYTES = 320 << 20


def timed(fn, sets):
    """fn(*sets[i % len(sets)]) REPS times: median, 10th and 90th percentile in microseconds"""
    for i in range(WARMUP):
        fn(*sets[i % len(sets)])
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(*sets[(i + WARMUP) % len(sets)])
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return round(t[len(t) // 2], 1), round(t[len(t) // 10], 1), round(t[(9 * len(t)) // 10], 1)


def variants():
    fwd = lambda a, b, g: cabi.correlation_forward(a, b, *PWC)
    bwd = lambda a, b, g: cabi.correlation_backward(a, b, g, *PWC)

    def cast_fwd(a, b, g):
        return cabi.correlation_forward(a.float(), b.float(), *PWC).bfloat16()

    def cast_bwd(a, b, g):
        g1, g2 = cabi.correlation_backward(a.float(), b.float(), g.float(), *PWC)
        return g1.bfloat16(), g2.bfloat16()

    both = lambda f, r: (lambda a, b, g: (f(a, b, g), r(a, b, g)))
    bf, fl, hf = torch.bfloat16, torch.float32, torch.float16
    return [("bf16", bf, fwd, bwd), ("fp32", fl, fwd, bwd), ("f16", hf, fwd, bwd), ("cast", bf, cast_fwd, cast_bwd)], \
        [("bf16 mfma", bf, lambda a, b, g: cabi.correlation_forward_bf16_kernel("mfma", a, b, *PWC)),
         ("bf16 gen", bf, lambda a, b, g: cabi.correlation_forward_bf16_kernel("generic", a, b, *PWC))], both


def subnormal_probe():
    """One product of a bfloat16 subnormal (2^-130) with 2^100 in a 32-channel MFMA step: 2^-30 if the input is kept,
    0 if it is flushed."""
    a = torch.zeros((1, 32, 4, 16), dtype=torch.bfloat16, device="cuda")
    b = torch.zeros_like(a)
    a[0, 0] = 2.0 ** -130
    b[0, 0] = 2.0 ** 100
    assert float(a[0, 0, 0, 0]) != 0.0
    out = cabi.correlation_forward_bf16_kernel("mfma", a, b, *PWC)
    got = float(out[0, 40, 1, 1]) * 32
    return {"product_of_subnormal": got, "kept": got == 2.0 ** -30}


def kernel_choice(gen, rounds=9, calls=40):
    """The measurement behind corr_bf16_mfma_threshold: the two forward kernels back to back at every level, hot.  A block
    is `calls` launches of one kernel between two device events with nothing in between (no per-call event, so the figure
    is the steady per-call time of a stream of launches); blocks of the MFMA and of the generic kernel alternate `rounds`
    times in one go, so both see the same machine.  Median and range of the rounds, microseconds per call; tiles: the
    64 x 2-pixel tiles the dispatch counts."""
    rows = []
    for pyramid, (B, levels) in LEVELS.items():
        for (C, H, W) in levels:
            a = torch.randn((B, C, H, W), generator=gen).bfloat16().cuda()
            b = torch.randn((B, C, H, W), generator=gen).bfloat16().cuda()
            out = torch.empty((B, 81, H, W), dtype=torch.bfloat16, device="cuda")
            t = {"mfma": [], "generic": []}
            for which in t:
                for _ in range(WARMUP):
                    cabi.correlation_forward_bf16_kernel(which, a, b, *PWC, out=out)
            torch.cuda.synchronize()
            for _ in range(rounds):
                for which in t:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(calls):
                        cabi.correlation_forward_bf16_kernel(which, a, b, *PWC, out=out)
                    e1.record()
                    torch.cuda.synchronize()
                    t[which].append(e0.elapsed_time(e1) * 1e3 / calls)
            row = {"pyramid": pyramid, "B": B, "C": C, "H": H, "W": W, "tiles": -(-W // 64) * -(-H // 2) * B}
            for which, v in t.items():
                v.sort()
                row[which] = (round(v[len(v) // 2], 1), round(v[0], 1), round(v[-1], 1))
            row["faster"] = "mfma" if row["mfma"][0] < row["generic"][0] else "generic"
            print("choice %s B=%d C=%3d %3dx%3d  %5d tiles   mfma %6.1f (%.1f .. %.1f)   generic %6.1f (%.1f .. %.1f)   -> %s" % (
                (pyramid, B, C, H, W, row["tiles"]) + row["mfma"] + row["generic"] + (row["faster"],)), flush=True)
            rows.append(row)
    return rows


def main():
    gen = torch.Generator().manual_seed(3)
    full, kernels, both = variants()
    result = {"device": torch.cuda.get_device_name(0), "levels": [], "subnormal_probe": subnormal_probe()}
    print("bfloat16 subnormal input through the MFMA:", result["subnormal_probe"], flush=True)
    result["kernel_choice"] = kernel_choice(gen)
    for pyramid, (B, levels) in LEVELS.items():
        for (C, H, W) in levels:
            per_set = (2 * B * C * H * W + B * 81 * H * W) * 4
            nsets = min(max(2, -(-COLD_BYTES // per_set)), WARMUP + REPS)      # (a small level: a set per call, none used twice)
            host = [(torch.randn((B, C, H, W), generator=gen), torch.randn((B, C, H, W), generator=gen),
                     torch.randn((B, 81, H, W), generator=gen)) for _ in range(min(nsets, 8))]
            row = {"pyramid": pyramid, "B": B, "C": C, "H": H, "W": W, "cold_sets": nsets}
            for name, dt, f, r in full:
                sets = [tuple(t.to(dt).cuda() for t in host[i % len(host)]) for i in range(nsets)]
                for what, fn in (("fwd", f), ("bwd", r), ("fwd+bwd", both(f, r))):
                    row["%s %s hot" % (name, what)] = timed(fn, sets[:1])
                    row["%s %s cold" % (name, what)] = timed(fn, sets)
                del sets
            sets = [tuple(t.bfloat16().cuda() for t in host[i % len(host)]) for i in range(nsets)]
            for name, dt, f in kernels:
                row["%s fwd hot" % name] = timed(f, sets[:1])
                row["%s fwd cold" % name] = timed(f, sets)
            del sets
            torch.cuda.empty_cache()
            print("%s B=%d C=%3d %3dx%3d" % (pyramid, B, C, H, W), flush=True)
            for k, v in row.items():
                if isinstance(v, tuple):
                    print("    %-22s %8.1f us  (%.1f .. %.1f)" % ((k,) + v), flush=True)
            result["levels"].append(row)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
