"""Helpers of the bfloat16 PWC-Net block tests (vfi_pwc_warp_*_bf16, vfi_correlation_lrelu_*_bf16): the warp, the correlation
with LeakyReLU and the concatenation slice on bfloat16 storage.  No test functions, and nothing of the product is imported.

  lrelu_two_roundings(mean, slope)    the forward's contract in numpy: the mean rounded to bfloat16 FIRST, a value that is not
                                      positive multiplied by the slope in float32 and rounded AGAIN (float32 array of bfloat16 values)
  masked_gradient(g, y, slope)        the backward's g' = y > 0 ? g : bf16_rne(float(g) * slope)
  warp_forward_f64(x, flo, ac)        the warp in float64 after the float32 decisions, with the sum of |weight x value|
  guarded(...) / guard_intact(...)    a tensor of any strides inside a pattern-filled buffer, and whether everything the
                                      tensor does not address still holds the pattern
  half_ulp(v)                         half a unit in the last place of bfloat16 at v: what one rounding to nearest may cost
  bf16_within(...)                    the float32 warp backward test's tolerances plus half a bfloat16 ulp
"""
import numpy as np

from tests.corr_bf16 import bits, from_bits, same_bits, to_bf16  # noqa: F401  (re-exported for the tests)
from tests.pwc_warp_backward import flow_family, pwc_warp_bwd  # noqa: F401

GUARD16, GUARD32 = 0x5A5A, 0x5A5A5A5A


def half_ulp(v):
    """Half a bfloat16 unit in the last place at |v|: bfloat16 keeps 8 significand bits, so for 2^k <= |v| < 2^(k+1) the
    spacing is 2^(k-7) and rounding to nearest is off by at most 2^(k-8) = 2^-9 x 2^(k+1) -- "2^-9 relative" to the power of
    two ABOVE |v|.  Relative to |v| itself that is between 2^-9 (just below a power of two) and 2^-8 (just above one): no
    correctly rounded result, the rounded float32 entry included, stays within 2^-9 |v| everywhere.  Below the smallest
    normal number the spacing is 2^-133."""
    _, e = np.frexp(np.abs(np.asarray(v, np.float64)))          # |v| = m 2^e, 0.5 <= m < 1: k = e - 1
    return np.maximum(np.ldexp(1.0, e - 9), 2.0 ** -134)


# ------------------------------------------------------------------ LeakyReLU on bfloat16 storage

def lrelu_two_roundings(mean, slope):
    m = to_bf16(mean)
    with np.errstate(all="ignore"):
        return np.where(m > 0, m, to_bf16(m * np.float32(slope)))


def masked_gradient(g, y, slope):
    g = np.asarray(g, np.float32)
    with np.errstate(all="ignore"):
        return np.where(np.asarray(y) > 0, g, to_bf16(g * np.float32(slope)))


def edge_grid():
    """bfloat16 values that exercise the two roundings: both zeros, the smallest subnormals, normals either side of 1, the
    largest finite values, both infinities, NaN"""
    pats = [0x0000, 0x8000, 0x0001, 0x8001, 0x0002, 0x8003, 0x007F, 0x807F, 0x0080, 0x8080, 0x0081, 0x3F80, 0xBF80, 0x3F81, 0xBF81,
            0x3DCD, 0xBDCD, 0x4049, 0xC049, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0]
    rng = np.random.default_rng(3)
    rand = rng.integers(0, 1 << 16, 4096).astype(np.uint16)
    return from_bits(np.concatenate([np.array(pats, np.uint16), rand]))


# ------------------------------------------------------------------ cases

def dense_strides(shape):
    s, out = 1, []
    for n in reversed(shape):
        out.append(s)
        s *= n
    return tuple(reversed(out))


# ------------------------------------------------------------------ guards

def guarded(torch, shape, dtype, stride=None, offset=64, tail=64):
    """(buffer of raw words holding the pattern, a `dtype` tensor of `shape` / `stride` that starts `offset` elements into it)"""
    shape = tuple(shape)
    stride = dense_strides(shape) if stride is None else tuple(stride)
    span = 1 + sum((n - 1) * s for n, s in zip(shape, stride))
    raw, pattern = (torch.int16, GUARD16) if dtype == torch.bfloat16 else (torch.int32, GUARD32)
    buf = torch.full((offset + span + tail,), pattern, dtype=raw, device="cuda")
    return buf, buf.view(dtype).as_strided(shape, stride, offset)


def guard_intact(torch, buf, view):
    """every word of buf that `view` does not address still holds the pattern"""
    mask = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    mask.as_strided(tuple(view.shape), tuple(view.stride()), view.storage_offset()).fill_(True)
    pattern = GUARD16 if buf.dtype == torch.int16 else GUARD32
    return bool((buf[~mask] == pattern).all())


def fill(torch, view, values):
    """values (a float32 numpy array) into the guarded view, converted to its dtype"""
    view.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(view.dtype).cuda())
    return view


def tensor_bits(torch, t):
    """the uint16 patterns of a bfloat16 tensor (any strides)"""
    assert t.dtype == torch.bfloat16
    return t.contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


# ------------------------------------------------------------------ the warp in float64

def warp_forward_f64(x, flo, align_corners=True):
    """(W, A): the warped tensor and the sum of |weight * value| per output, float64 after the float32 decisions of `geometry`"""
    from tests.pwc_warp_backward import geometry
    B, C, h, w = x.shape
    ix, iy, fx0, fy0, inb, corners, mask = geometry(flo, h, w, align_corners)
    d = np.float64
    ix, iy, fx0, fy0 = ix.astype(d), iy.astype(d), fx0.astype(d), fy0.astype(d)
    dx1, dx0, dy1, dy0 = fx0 + 1 - ix, ix - fx0, fy0 + 1 - iy, iy - fy0
    wts = (dx1 * dy1, dx0 * dy1, dx1 * dy0, dx0 * dy0)
    W, A = np.zeros((B, C, h, w), d), np.zeros((B, C, h, w), d)
    flat = x.astype(d).reshape(B, C, h * w)
    for k in range(4):
        cy, cx = corners[k]
        idx = np.where(inb[k], np.clip(cy, 0, h - 1) * w + np.clip(cx, 0, w - 1), 0).reshape(B, 1, h * w)
        v = np.take_along_axis(flat, np.broadcast_to(idx, (B, C, h * w)), axis=2).reshape(B, C, h, w)
        term = np.where(inb[k], wts[k], 0.0)[:, None] * v * mask.astype(d)[:, None]
        W += term
        A += np.abs(term)
    return W, A


# ------------------------------------------------------------------ the backward's tolerance against float64

def bf16_within(got_x, got_f, ref, g, flow_bf16=True):
    """got_x / got_f: float64 arrays of the bfloat16 (or float32) results, or None; ref = pwc_warp_bwd(...) in float64.
    The float32 test's bounds (4e-7 A + 2^-40 max|g| for grad_x, 1e-5 S + 1e-7 for grad_flow) plus half a bfloat16 ulp at the
    reference value for the one rounding to bfloat16 (grad_flow: only where the flow, and so its gradient, is bfloat16).
    Returns the worst error in units of 2^-9 |reference| (the figure a bound of "2^-9 of the value" would have to pass)."""
    gx, gf, A, S, mask = ref
    worst = 0.0
    if got_x is not None:
        tol = 4e-7 * A + 2.0 ** -40 * float(np.abs(g).max()) + half_ulp(gx)
        bad = ~(np.abs(got_x - gx) <= tol)
        assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(np.abs(got_x - gx).max()))
        big = np.abs(gx) > 1e-3
        worst = max(worst, float((np.abs(got_x - gx)[big] / (2.0 ** -9 * np.abs(gx)[big])).max())) if big.any() else worst
    if got_f is not None:
        tol = 1e-5 * S + 1e-7 + (half_ulp(gf) if flow_bf16 else 0.0)
        bad = ~(np.abs(got_f - gf) <= tol)
        assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(np.nanmax(np.abs(got_f - gf))))
        off = np.broadcast_to((mask == 0)[:, None], got_f.shape)
        assert (got_f[off] == 0).all()
    return worst
