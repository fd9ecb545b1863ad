"""Helpers of the channels_last FilterInterpolation tests (vfi_filterinterp_forward_ori_nhwc_multi_to[_bf16],
csrc/filterinterp_nhwc.hip).  No test functions, nothing of the product imported.

  constants()                      the kernel's tile #defines, read from the source
  vector_width(...)                the launcher's choice of the access width (fn_vector_width), in elements
  expected(oracle, ...)            the logical NCHW result: oracle.filterinterp_ori_fwd(fmad=1) in float32; for bfloat16
                                   widen -> float32 -> round once (tests/fi_ctx_bf16.forward_reference)
  raw_bits / same_raw_bits         uint32 or uint16 patterns, compared NaN-aware
  FLOWS                            the flow generators: zero, sub-pixel, crossing each border and corner, leaving the frame
  cl_buffer / cl_slice             pattern-filled channels_last buffers and channel slices of them

The library ships ONE path per filter-size class (a direct gather; the LDS-staged window kernel lost its measurement and is
not shipped), so there is no per-tile choice to mirror: what varies per launch is the access width,
mirrored here and pinned to the library's own answer (vfi_filterinterp_nhwc_access_width).
"""
import numpy as np

from tests import fi_windows as fw
from tests.corr_bf16 import from_bits, to_bf16  # noqa: F401  (re-exported)
from tests.fi_ctx_bf16 import forward_reference
from tests.pwc_bf16 import guard_intact, guarded  # noqa: F401  (re-exported)

SRC = "filterinterp_nhwc.hip"
f32 = np.float32


def constants():
    d = fw.defines(SRC)
    return {k: d[k] for k in ("FN_TW", "FN_TH", "FN_PIXELS", "FN_THREADS")}


def vector_width(esize, shape, image, outs, fs=4):
    """fn_vector_width: image and outs are (data_ptr, (stride b, stride h, stride w)); the widest of 16, 8, 4 bytes (in
    elements) that divides every base address and every stride the shape uses; 1 for every filter size but 4"""
    B, _, h, w = shape
    if fs != 4:
        return 1
    v = 16 // esize
    while v > 1:
        ok = True
        for ptr, (sb, sh, sw) in [image] + list(outs):
            ok = ok and ptr % (v * esize) == 0 and (B == 1 or sb % v == 0) and (h == 1 or sh % v == 0) and (w == 1 or sw % v == 0)
        if ok:
            return v
        v //= 2
    return 1


def tensor_layout(t):
    """(data_ptr, (stride b, stride h, stride w)) of a torch tensor"""
    return t.data_ptr(), (t.stride(0), t.stride(2), t.stride(3))


# ------------------------------------------------------------------ expectation and comparison

def expected(oracle, img, flow, filt, bf16):
    """the logical [B, C, h, w] result as a float32 array (of bfloat16 values where bf16)"""
    if bf16:
        return forward_reference(oracle, img, flow, filt)
    with np.errstate(all="ignore"):
        return oracle.filterinterp_ori_fwd(np.ascontiguousarray(img, dtype=f32), flow, filt, fmad=1, nthreads=8)


def raw_bits(values, bf16):
    """values (float32; bfloat16 values where bf16) as uint16 / uint32 patterns"""
    a = np.ascontiguousarray(values, dtype=f32).view(np.uint32)
    if bf16:
        assert not (a & 0xffff).any(), "bfloat16 values"
        return (a >> 16).astype(np.uint16)
    return a


def tensor_raw_bits(torch, t):
    """the patterns of a float32 or bfloat16 tensor of any strides, in logical NCHW order"""
    c = t.contiguous().cpu()
    if t.dtype == torch.bfloat16:
        return c.view(torch.int16).numpy().view(np.uint16)
    return c.view(torch.int32).numpy().view(np.uint32)


def _as_float(b):
    return from_bits(b) if b.dtype == np.uint16 else b.view(f32)


def same_raw_bits(got, want):
    """NaN at the same places (payload and sign are not compared), every other element bit for bit; a message or ''"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "shapes / types %s %s / %s %s" % (got.shape, got.dtype, want.shape, want.dtype)
    g, w = _as_float(got), _as_float(want)
    ng, nw = np.isnan(g), np.isnan(w)
    bad = (ng != nw) | (~ng & ~nw & (got != want))
    if not bad.any():
        return ""
    idx = np.argwhere(bad)
    return "%d of %d differ; first (index, got, want): %s" % (len(idx), bad.size,
                                                              [(tuple(i), g[tuple(i)], w[tuple(i)]) for i in idx[:6]])


# ------------------------------------------------------------------ flows

def _zero(rng, B, h, w):
    return np.zeros((B, 2, h, w), f32)


def _subpixel(rng, B, h, w):
    return (rng.random((B, 2, h, w), dtype=f32) - f32(0.5)) * f32(0.9)


def _borders(rng, B, h, w):
    """every border and corner pixel's window reaches past the frame; the flow of the border pixels points outwards by
    less than a pixel where that keeps them valid (x2 in [0, w - 1]), inwards elsewhere, by up to two pixels"""
    fl = (rng.random((B, 2, h, w), dtype=f32) - f32(0.5)) * f32(4.0)
    x = np.arange(w, dtype=f32)[None, None, :]
    y = np.arange(h, dtype=f32)[None, :, None]
    fl[:, 0] = np.clip(x + fl[:, 0], 0, w - 1) - x              # every pixel lands inside the frame, many ON its border
    fl[:, 1] = np.clip(y + fl[:, 1], 0, h - 1) - y
    return fl.astype(f32)


def _leaving(rng, B, h, w):
    """a third of the pixels leave the frame or exceed half its size: they copy the input through"""
    fl = (rng.random((B, 2, h, w), dtype=f32) - f32(0.5)) * f32(3.0)
    out = rng.random((B, h, w)) < 0.34
    big = (rng.random((B, 2, h, w), dtype=f32) - f32(0.5)) * f32(2.5 * max(h, w))
    return np.where(out[:, None], big, fl).astype(f32)


FLOWS = {"zero": _zero, "subpixel": _subpixel, "borders": _borders, "leaving": _leaving}


def flow_features(flow, h, w, fs=4):
    """what a field exercises: 'valid', 'invalid', and a clamped tap on each side of the frame"""
    valid, ix, iy, _, _ = fw.samples(flow, h, w)
    L, T = ix + 1 - fs // 2, iy + 1 - fs // 2
    got = set()
    for name, m in (("valid", valid), ("invalid", ~valid), ("left", valid & (L < 0)), ("right", valid & (L + fs > w)),
                    ("top", valid & (T < 0)), ("bottom", valid & (T + fs > h))):
        if m.any():
            got.add(name)
    return got


# ------------------------------------------------------------------ channels_last buffers

def cl_buffer(torch, B, ctot, h, w, dtype, batch_pad=0, offset=64):
    """(raw pattern buffer, a [B, ctot, h, w] `dtype` view of it with channels_last strides): pixels ctot apart, batch
    items h * w * ctot + batch_pad apart, the first element `offset` elements into the buffer"""
    stride = (h * w * ctot + batch_pad, 1, w * ctot, ctot)
    return guarded(torch, (B, ctot, h, w), dtype, stride, offset)


def cl_fill(torch, view, values):
    """logical NCHW values (float32 numpy) into a view of any layout, converted to its dtype"""
    view.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=f32)).to(view.dtype).cuda())
    return view


def cl_tensor(torch, values, dtype):
    """a dense channels_last GPU tensor of the logical NCHW values"""
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=f32)).to(dtype).cuda()
    return t.contiguous(memory_format=torch.channels_last)
