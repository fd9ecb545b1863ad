#!/usr/bin/env python3
"""Development: the FilterInterpolation forward outputs of a variant build of the library against the product build's, bit for
bit (two processes: a process loads one library): the float32 entry on four flow models at three shapes, and the 16-bit
kernels -- fp16 staged and direct, bfloat16 multi_to staged and direct into channel slices -- on the all-class field of
tests/fi_windows.py (every ring class, interior and EDGE tiles, a ragged last tile column) and on an odd frame width.
    python tools/fi_lib_compare.py --save /tmp/ref.pt                    (product library)
    python tools/fi_lib_compare.py --lib <pkg>/lib_vX/libvfi_hip.so --check /tmp/ref.pt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import vfidkr_amd  # noqa: E402,F401
if "--lib" in sys.argv:
    vfidkr_amd.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
import numpy as np  # noqa: E402
from tests import fi_windows as fw  # noqa: E402
from vfidkr_amd import cabi, synthetic as S  # noqa: E402


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def sixteen_bit_cases(dev, gen, outs):
    """fp16: the staged and the direct entry; bfloat16: two flows into slices of a wider buffer, staged and direct"""
    B, C = 2, 7
    fh, fw_ = fw.field_shape("f16")
    field = torch.from_numpy(fw.build_field("f16", np.random.default_rng(16), B, fh, fw_)["flow"])
    for tag, h, w, flow in (("field", fh, fw_, field), ("odd", 50, 131, S.flow(B, 50, 131, 3.0, gen, "wild"))):
        ctx = S.context(B, C, h, w, gen).to(dev)
        filt = S.filters(B, h, w, gen).to(dev)
        flows = [flow.to(dev), (0.5 * flow).to(dev)]
        for direct in (False, True):
            name = "%s_%dx%d_%s" % (tag, h, w, "direct" if direct else "staged")
            half = ctx.half()
            out = torch.full_like(half, float("nan"))
            assert cabi.filterinterp_forward_ori_f16(half, flows[0], filt, out, direct=direct) == 0
            outs["f16_" + name] = out.cpu()
            wide = [torch.full((B, C + 4, h, w), float("nan"), dtype=torch.bfloat16, device=dev) for _ in flows]
            assert cabi.filterinterp_forward_ori_multi_to(ctx.bfloat16(), flows, filt, [b[:, 2:2 + C] for b in wide], direct=direct) == 0
            for t, b in enumerate(wide):
                outs["bf16_%s_t%d" % (name, t)] = b.cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--save", default=None)
    ap.add_argument("--check", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = S.generator()
    outs = {}
    for (hh, ww, C) in ((1080, 1920, 24), (270, 333, 5), (64, 70, 3)):
        h, w = (S.padded_size(hh, ww) if hh == 1080 else (hh, ww))
        ctx = S.context(1, C, h, w, gen).to(dev)
        filt = S.filters(1, h, w, gen).to(dev)
        for model in ("smooth", "quarter", "uniform1", "wild"):
            flow = S.flow(1, h, w, 8.0 * w / 1984.0, gen, model).to(dev)
            out = torch.full_like(ctx, float("nan"))
            assert cabi.filterinterp_forward_ori(ctx, flow, filt, out) == 0
            outs["%dx%d_%d_%s" % (h, w, C, model)] = out.cpu()
    sixteen_bit_cases(dev, gen, outs)
    if args.save:
        torch.save(outs, args.save)
        print("saved", len(outs), "outputs")
    if args.check:
        ref = torch.load(args.check)
        bad = [k for k in outs if k not in ref or not torch.equal(bits(outs[k]), bits(ref[k]))]
        print("same bits on all %d cases" % len(outs) if not bad else "DIFFERENT: %s" % bad)
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
