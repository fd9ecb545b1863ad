"""Helpers of the channels_last FilterInterpolation image-gradient tests
(vfi_filterinterp_backward_ori_nhwc_image_multi[_bf16], csrc/filterinterp_nhwc_bwd.hip).  No test functions, nothing of the
product imported.

  constants()                          the new unit's tile #defines, read from its source
  call_class(...)                      the per-call decision: "staged" or the reason every tile takes the per-addend kernel
                                       ("filter_size", "fp32", "scale2")
  tiles(flows) / tile_classes(...)     the per-tile decision for the flows of ONE launch: "empty", "staged", "staged_split",
                                       "direct_window"
  launches(flows)                      the flows launch by launch (FNB_NT per launch)
  vector_width(...)                    the launcher's choice of the gradient access width (fnb_vector_width), in elements
  expectation(flows, gouts, filt, bf)  tests/fi_ctx_backward.predict on the logical NCHW arrays (layout-free); bfloat16: to_bf16
                                       of it for widened bfloat16 gradients
  cl_buffer, guarded, guard_intact, same_raw_bits, ...   tests/fi_nhwc's buffers and raw-bit comparison
"""
import numpy as np

from oracle.np_oracle import _fi_geometry
from tests import bwd_tiles as bt
from tests import fi_ctx_backward as fc
from tests import fi_windows as fw
from tests.fi_nhwc import (FLOWS, cl_buffer, cl_fill, cl_tensor, from_bits, guard_intact, guarded, raw_bits,  # noqa: F401
                           same_raw_bits, tensor_layout, tensor_raw_bits, to_bf16)

SRC = "filterinterp_nhwc_bwd.hip"
f32 = np.float32
NAMES = ("FNB_TW", "FNB_TH", "FNB_PIXELS", "FNB_THREADS", "FNB_SLAB", "FNB_CELLS", "FNB_NT")


def constants():
    d = fw.defines(SRC)
    return {k: d[k] for k in NAMES}


# ------------------------------------------------------------------ decisions (as written in the source)

def call_class(gouts, filt, h, w, direct=False):
    """const bool staged = !DIRECT && fs == 4 && filter_channels == 16;  then, on the device, gradacc_staged_ok"""
    fcn = filt.shape[1]
    if direct or int(np.sqrt(f32(fcn))) != 4 or fcn != 16:
        return "filter_size"
    _, fp32, _, scale2 = fc.call_scale(gouts, filt, h, w)
    if fp32:
        return "fp32"
    return "scale2" if scale2 != 1 else "staged"


def window_fits(bw, bh):
    """(int64_t)bw * bh * FNB_SLAB <= FNB_CELLS"""
    c = constants()
    return bw * bh * c["FNB_SLAB"] <= c["FNB_CELLS"]


def launches(flows):
    nt = constants()["FNB_NT"]
    return [flows[i:i + nt] for i in range(0, len(flows), nt)]


def tiles(flows):
    """{(b, ty, tx): (class, box or None)} for the flows [B, 2, h, w] of ONE launch: the union box of the clamped taps of every
    valid pixel of every flow.  "empty" without one; "staged" when the union window fits the slab; otherwise the flows go one
    by one, each on its own window: "staged_split" when every one of them fits, "direct_window" when one does not (that flow
    is flagged for the per-addend kernel, the others are staged)"""
    c = constants()
    assert 1 <= len(flows) <= c["FNB_NT"]
    B, _, h, w = flows[0].shape
    per_flow = []
    for flow in flows:
        valid, _, _, _, _, _, _, L, T = _fi_geometry(flow.astype(f32), h, w, 4)
        per_flow.append([bt._boxes(valid[b], np.clip(L[b], 0, w - 1), np.clip(T[b], 0, h - 1), np.clip(L[b] + 3, 0, w - 1),
                                   np.clip(T[b] + 3, 0, h - 1), c["FNB_TH"], c["FNB_TW"]) for b in range(B)])
    out = {}
    for b in range(B):
        for key in per_flow[0][b]:
            live = [pf[b][key] for pf in per_flow if pf[b][key] is not None]
            if not live:
                out[(b,) + key] = ("empty", None)
                continue
            box = (min(x[0] for x in live), min(x[1] for x in live), max(x[2] for x in live), max(x[3] for x in live))
            if window_fits(box[2] - box[0] + 1, box[3] - box[1] + 1):
                out[(b,) + key] = ("staged", box)
            elif len(flows) > 1 and all(window_fits(x[2] - x[0] + 1, x[3] - x[1] + 1) for x in live):
                out[(b,) + key] = ("staged_split", box)
            else:
                out[(b,) + key] = ("direct_window", box)
    return out


def tile_classes(flows, gouts, filt):
    """the set of tile classes a call reaches, over all its launches: the per-tile classes when the call is staged, else
    {"direct_" + the call's reason} (and "empty": an empty tile is left before the call's class is looked at)"""
    h, w = flows[0].shape[2:]
    cls = call_class(gouts, filt, h, w)
    got = set()
    for group in launches(flows):
        if filt.shape[1] == 16 and int(np.sqrt(f32(filt.shape[1]))) == 4:
            for k, _ in tiles(group).values():
                got.add(k if cls == "staged" or k == "empty" else "direct_" + cls)
        else:
            got.add("direct_" + cls)
    return got


def vector_width(esize, shape, grads):
    """fnb_vector_width: grads are (data_ptr, (stride b, stride h, stride w)), one layout; the widest of 16, 8, 4 bytes (in
    elements) that divides every gradient's address and every stride the shape uses"""
    B, _, h, w = shape
    sb, sh, sw = grads[0][1]
    v = 16 // esize
    while v > 1:
        if (B == 1 or sb % v == 0) and (h == 1 or sh % v == 0) and (w == 1 or sw % v == 0) and \
                all(ptr % (v * esize) == 0 for ptr, _ in grads):
            return v
        v //= 2
    return 1


# ------------------------------------------------------------------ the inputs of the GPU tests

FRAME = (19, 37)
CHANNELS = (2, 3, 7, 8, 9, 196, 199)
FRAMES = ((3, 3), (5, 6), (1, 9), (9, 1), FRAME)
FILTER_CHANNELS = (16, 4, 25, 36, 1, 10, 18)
WINDOW_FRAME = (43, 200)


def _grads(rng, shape, n):
    return [np.clip(rng.standard_normal(shape), -3, 3).astype(f32) for _ in range(n)]


def case_channels(C):
    h, w = FRAME
    rng = np.random.default_rng(2100 + C)
    return dict(flows=[FLOWS[k](rng, 2, h, w) for k in ("subpixel", "borders")], filt=rng.random((2, 16, h, w), dtype=f32),
                gouts=_grads(rng, (2, C, h, w), 2))


def case_frames(h, w, B):
    rng = np.random.default_rng(2200 + 10 * h + w + B)
    return dict(flows=[FLOWS[k](rng, B, h, w) for k in ("borders", "leaving", "zero")], filt=rng.random((B, 16, h, w), dtype=f32),
                gouts=_grads(rng, (B, 9, h, w), 3))


def case_flows(kind, n):
    h, w = FRAME
    rng = np.random.default_rng(2300 + n)
    return dict(flows=[FLOWS[kind](rng, 1, h, w) for _ in range(n)], filt=rng.random((1, 16, h, w), dtype=f32) - f32(0.3),
                gouts=_grads(rng, (1, 8, h, w), n))


def case_window(nflows=3, B=2, C=5):
    """tests/fi_ctx_backward.build_field at 43 x 200: sub-pixel tiles (staged), windows stretched until they do not fit
    (direct), an empty tile"""
    h, w = WINDOW_FRAME
    rng = np.random.default_rng(2400 + nflows)
    flows = fc.build_field(rng, B, h, w, nflows)
    # rows 40.. of columns 64..95 (a tile no recipe of the builder uses): flow 0 alone points twelve rows up, so the union
    # window does not fit while every flow's own window does
    flows[0][:, 1, 40:, 64:96] -= f32(12)
    return dict(flows=flows, filt=rng.random((B, 16, h, w), dtype=f32), gouts=_grads(rng, (B, C, h, w), nflows))


def case_filter(fcn, B=2, C=7):
    h, w = FRAME
    rng = np.random.default_rng(2500 + fcn)
    return dict(flows=[FLOWS[k](rng, B, h, w) for k in ("borders", "leaving")], filt=rng.random((B, fcn, h, w), dtype=f32),
                gouts=_grads(rng, (B, C, h, w), 2))


def case_slices(C=196):
    h, w = FRAME
    rng = np.random.default_rng(2600)
    return dict(flows=[FLOWS[k](rng, 2, h, w) for k in ("borders", "leaving")], filt=rng.random((2, 16, h, w), dtype=f32),
                gouts=_grads(rng, (2, C, h, w), 2))


def case_tiny():
    c = case_channels(9)
    return dict(c, gouts=[(g * f32(2.0 ** -100)).astype(f32) for g in c["gouts"]])


def case_nonfinite():
    """dyadic inputs (every addend and partial sum exact in fp32 and in bfloat16 products), a +inf and a NaN in flow 1's
    gradient: the whole call scatters with fp32 atomics"""
    h, w = FRAME
    rng = np.random.default_rng(2700)
    flows = [(np.round(FLOWS[k](rng, 2, h, w) * 4) / 4).astype(f32) for k in ("subpixel", "borders", "subpixel")]
    filt = (np.round(rng.random((2, 16, h, w), dtype=f32) * 8) / 8).astype(f32)
    gouts = [(np.round(g * 4) / 4).astype(f32) for g in _grads(rng, (2, 7, h, w), 3)]
    gouts[1][0, 1, 2, 10] = np.inf
    gouts[1][1, 2, 17, 30] = np.nan
    return dict(flows=flows, filt=filt, gouts=gouts)


def all_cases():
    """(name, case) of every kernel-level GPU test input"""
    for C in CHANNELS:
        yield "channels %d" % C, case_channels(C)
    for h, w in FRAMES:
        for B in (1, 2):
            yield "frame %dx%d B=%d" % (h, w, B), case_frames(h, w, B)
    for kind in sorted(FLOWS):
        for n in (1, 2, 3, 4):
            yield "flows %s x%d" % (kind, n), case_flows(kind, n)
    yield "window", case_window()
    for fcn in FILTER_CHANNELS:
        yield "filter %d" % fcn, case_filter(fcn)
    yield "slices", case_slices()
    yield "tiny", case_tiny()
    yield "nonfinite", case_nonfinite()


# ------------------------------------------------------------------ expectation

def expectation(flows, gouts, filt, bf16):
    """(logical NCHW gradient as float32 -- of bfloat16 values where bf16 --, k, fp32 path); None on the fp32 path.  gouts are
    the gradients the kernels see: float32, or already bfloat16 values (widened exactly)"""
    want, k, fp32 = fc.predict(flows, gouts, filt)
    if want is not None and bf16:
        want = to_bf16(want)
    return want, k, fp32
