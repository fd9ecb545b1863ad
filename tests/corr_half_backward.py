"""Numpy restatement of the reference's at::Half correlation backward (correlation_cuda_kernel.cu:151-334, dispatched
with AT_DISPATCH_FLOATING_TYPES_AND_HALF at :495-541), written literally from its arithmetic.

at::Half operators widen to float, compute, and round back to half after every operation:
  p   = half(float(gradOutput) * float(val))                        one term
  s_l = half(float(s_l) + float(p))                                 32 partials, `__shared__ scalar_t prod_sum[32]`
  r   = half(float(r) + float(s_l)), l = 0..31                      the sequential reduction of the partials
  out = half(float(r) / float(half(k*k*C)))                         `scalar_t nelems` is itself rounded to half
The terms, windows and skips are those of the float32 path (oracle.correlation_bwd): partial l takes tc = l, l+32, ...,
and for each tc the window rows outer, columns inner.  Positions the reference never visits keep the binding's zero fill.

`correlation_bwd_half(..., dtype=np.float64)` evaluates the same sums without rounding (for the error bound).
Vectorised over (n, c, y, x), looped over l, tc, j, i.
"""
import math

import numpy as np


def out_dims(h, w, pad, k, md, s1, s2):
    """correlation_cuda.cc:23-36 (ceil of a float quotient)."""
    kr = (k - 1) // 2
    border = kr + md
    dr = md // s2
    oh = int(math.ceil(np.float32(h + 2 * pad - 2 * border) / np.float32(s1)))
    ow = int(math.ceil(np.float32(w + 2 * pad - 2 * border) / np.float32(s1)))
    return (2 * dr + 1) ** 2, oh, ow


def _gather(a, yy, xx):
    """a[n, c, yy, xx] for per-pixel coordinates yy, xx of shape (H, W); zero outside the map (the padding)."""
    H, W = a.shape[2:]
    ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    v = a[:, :, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
    return np.where(ok[None, None], v, np.zeros((), a.dtype))


def correlation_bwd_half(f1, f2, gout, pad=4, k=1, md=4, s1=1, s2=1, dtype=np.float16):
    """(gradInput1, gradInput2) of the half backward; stride1 must be 1 (the only defined case)."""
    assert s1 == 1
    if dtype == np.float16:
        rnd = lambda v: v.astype(np.float16)                                            # noqa: E731
        mul = lambda a, b: rnd(a.astype(np.float32) * b.astype(np.float32))             # noqa: E731
        add = lambda a, b: rnd(a.astype(np.float32) + b.astype(np.float32))             # noqa: E731
        div = lambda a, b: rnd(a.astype(np.float32) / np.float32(b))                    # noqa: E731
        nelems = np.float16(k * k * f1.shape[1])
    else:
        mul = lambda a, b: a * b                                                        # noqa: E731
        add = lambda a, b: a + b                                                        # noqa: E731
        div = lambda a, b: a / b                                                        # noqa: E731
        nelems = dtype(k * k * f1.shape[1])
    f1, f2, gout = (np.asarray(a, np.float16).astype(dtype) for a in (f1, f2, gout))
    B, C, H, W = f1.shape
    oc, oh, ow = out_dims(H, W, pad, k, md, s1, s2)
    assert gout.shape == (B, oc, oh, ow)
    kr, dr = (k - 1) // 2, md // s2
    dsz = 2 * dr + 1
    y, x = np.meshgrid(np.arange(H) + pad, np.arange(W) + pad, indexing="ij")           # padded coordinates
    zero = np.zeros((B, C, H, W), dtype)
    grads = []
    for second in (False, True):
        other = f1 if second else f2
        r = zero.copy()
        for l in range(32):
            s = zero.copy()
            for tc in range(l, oc, 32):
                i2, j2 = (tc % dsz - dr) * s2, (tc // dsz - dr) * s2
                if second:
                    xmin, ymin = x - kr - md - i2, y - kr - md - j2
                    xmax, ymax = x + kr - md - i2, y + kr - md - j2
                    val = _gather(other, y - j2 - pad, x - i2 - pad)
                else:
                    xmin, ymin = x - kr - md, y - kr - md
                    xmax, ymax = x + kr - md, y + kr - md
                    val = _gather(other, y + j2 - pad, x + i2 - pad)
                # the reference's `continue` (gradInput2) / early return (gradInput1): no term at all
                visit = ~((xmax < 0) | (ymax < 0) | (xmin >= ow) | (ymin >= oh) | (xmin > xmax) | (ymin > ymax))
                for dj in range(k):                                     # window rows outer ...
                    j = ymin + dj
                    for di in range(k):                                 # ... columns inner
                        i = xmin + di
                        ok = visit & (j >= 0) & (j < oh) & (i >= 0) & (i < ow)
                        g = gout[:, tc][:, None][:, :, np.clip(j, 0, oh - 1), np.clip(i, 0, ow - 1)]
                        s = np.where(ok[None, None], add(s, mul(g, val)), s)
            r = add(r, s)
        out = div(r, nelems)
        if not second:
            any_ = ~((x + kr - md < 0) | (y + kr - md < 0) | (x - kr - md >= ow) | (y - kr - md >= oh))
            out = np.where(any_[None, None], out, zero)     # never visited: the binding's zero fill (+0)
        grads.append(out)
    return tuple(grads)
