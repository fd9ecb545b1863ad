"""Numpy restatement of the gradient torch autograd gives for the reference's `PWCDCNet.warp` (PWCNet/PWCNet.py:159-199):
output = grid_sample(x, vgrid) * mask, where the mask is a constant (its two index assignments overwrite every element) and
grid_sample is ATen's bilinear grid_sampler_2d with zero padding, whose backward skips a corner outside the map.

The discrete decisions -- the sample coordinate, its floor corners, the in-bounds tests and the mask -- are evaluated in
`decide` precision (float32 by default, with the forward kernel's operation order: in float64 a pixel can cross the 0.9999
threshold or an integer boundary and change its gradient completely).  Everything after them is float64.

pwc_warp_bwd(x, flo, g, align_corners) -> (grad_x, grad_flow, A, S, mask):
  grad_x[b,c,y,x]   sum of gm * w_corner over the in-bounds corners that land on (y, x), gm = g * mask
  grad_flow[b,k]    sum_c gm * d(sample)/d(ix or iy) times grid_sampler_unnormalize's factor and 2 / max(W-1, 1)
  A                 per grad_x cell the sum of |addends|, S per grad_flow element the sum of |terms| (for tolerances)
"""
import numpy as np


def geometry(flo, h, w, align_corners, decide=np.float32):
    """The forward kernel's pwc_sample (csrc/pwc_warp.h) in `decide` precision, elementwise over [B, h, w]."""
    t = decide
    one, two = t(1), t(2)
    vx = np.arange(w, dtype=t)[None, None, :] + flo[:, 0].astype(t)
    vy = np.arange(h, dtype=t)[None, :, None] + flo[:, 1].astype(t)
    gx = two * vx / t(max(w - 1, 1)) - one
    gy = two * vy / t(max(h - 1, 1)) - one
    if align_corners:
        ix = ((gx + one) / two) * t(w - 1)
        iy = ((gy + one) / two) * t(h - 1)
    else:
        ix = ((gx + one) * t(w) - one) / two
        iy = ((gy + one) * t(h) - one) / two
    fx0, fy0 = np.floor(ix), np.floor(iy)
    wts = ((fx0 + one - ix) * (fy0 + one - iy), (ix - fx0) * (fy0 + one - iy),
           (fx0 + one - ix) * (iy - fy0), (ix - fx0) * (iy - fy0))
    finite = (np.abs(ix) < 1e9) & (np.abs(iy) < 1e9)
    with np.errstate(invalid="ignore"):
        x0 = np.where(finite, fx0, -2).astype(np.int64)
        y0 = np.where(finite, fy0, -2).astype(np.int64)
    inx0, inx1 = (x0 >= 0) & (x0 < w), (x0 + 1 >= 0) & (x0 + 1 < w)
    iny0, iny1 = (y0 >= 0) & (y0 < h), (y0 + 1 >= 0) & (y0 + 1 < h)
    inb = (iny0 & inx0, iny0 & inx1, iny1 & inx0, iny1 & inx1)           # nw, ne, sw, se
    m = np.zeros(ix.shape, t)
    for k in range(4):
        m = np.where(inb[k], m + wts[k], m)
    mask = np.where(m < t(0.9999), t(0), np.where(m > 0, t(1), m))
    corners = ((y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1))
    return ix, iy, fx0, fy0, inb, corners, mask


def coordinate_factors(h, w, align_corners):
    """d(ix)/d(flow x), d(iy)/d(flow y): grid_sampler_unnormalize's factor times the normalisation 2 / max(W-1, 1)."""
    fx = ((w - 1) / 2.0 if align_corners else w / 2.0) * 2.0 / max(w - 1, 1)
    fy = ((h - 1) / 2.0 if align_corners else h / 2.0) * 2.0 / max(h - 1, 1)
    return fx, fy


def pwc_warp_bwd(x, flo, g, align_corners=True, decide=np.float32):
    B, C, h, w = x.shape
    ix, iy, fx0, fy0, inb, corners, mask = geometry(flo, h, w, align_corners, decide)
    d = np.float64
    ix, iy, fx0, fy0 = ix.astype(d), iy.astype(d), fx0.astype(d), fy0.astype(d)
    dx1, dx0, dy1, dy0 = fx0 + 1 - ix, ix - fx0, fy0 + 1 - iy, iy - fy0
    wts = (dx1 * dy1, dx0 * dy1, dx1 * dy0, dx0 * dy0)
    x64, g64 = x.astype(d), g.astype(d)
    gm = g64 * mask.astype(d)[:, None]                                   # [B, C, h, w]
    gx = np.zeros((B, C, h * w), d)
    A = np.zeros((B, C, h * w), d)
    vals = []
    for k in range(4):
        cy, cx = corners[k]
        ok = inb[k]
        idx = np.where(ok, np.clip(cy, 0, h - 1) * w + np.clip(cx, 0, w - 1), 0)
        v = np.take_along_axis(x64.reshape(B, C, h * w), np.broadcast_to(idx.reshape(B, 1, h * w), (B, C, h * w)), axis=2)
        vals.append(np.where(ok[:, None], v.reshape(B, C, h, w), 0.0))
        add = gm * np.where(ok, wts[k], 0.0)[:, None]
        for b in range(B):
            sel = ok[b].reshape(-1)
            np.add.at(gx[b], (slice(None), idx[b].reshape(-1)[sel]), add[b].reshape(C, -1)[:, sel])
            np.add.at(A[b], (slice(None), idx[b].reshape(-1)[sel]), np.abs(add[b].reshape(C, -1)[:, sel]))
    pnw, pne, psw, pse = vals
    fx, fy = coordinate_factors(h, w, align_corners)
    gf = np.empty((B, 2, h, w), d)
    S = np.empty((B, 2, h, w), d)
    gf[:, 0] = (gm * ((pne - pnw) * dy1[:, None] + (pse - psw) * dy0[:, None])).sum(1) * fx
    gf[:, 1] = (gm * ((psw - pnw) * dx1[:, None] + (pse - pne) * dx0[:, None])).sum(1) * fy
    ag = np.abs(gm)
    S[:, 0] = (ag * ((np.abs(pne) + np.abs(pnw)) * dy1[:, None] + (np.abs(pse) + np.abs(psw)) * dy0[:, None])).sum(1) * abs(fx)
    S[:, 1] = (ag * ((np.abs(psw) + np.abs(pnw)) * dx1[:, None] + (np.abs(pse) + np.abs(pne)) * dx0[:, None])).sum(1) * abs(fy)
    return gx.reshape(B, C, h, w), gf, A.reshape(B, C, h, w), S, mask


def decisions(flo, h, w, align_corners, decide):
    """per pixel the discrete decisions (floor corners, in-bounds tests, mask) as one comparable array"""
    _, _, fx0, fy0, inb, _, mask = geometry(flo, h, w, align_corners, decide)
    with np.errstate(invalid="ignore"):
        return np.stack([fx0.astype(np.float64), fy0.astype(np.float64), mask.astype(np.float64)] +
                        [b.astype(np.float64) for b in inb])


def flow_family(rng, kind, B, h, w):
    """the flow families of the tests: zero, integer, N(0, sigma), across the border"""
    if kind == "zero":
        return np.zeros((B, 2, h, w), np.float32)
    if kind == "int":
        return rng.integers(-3, 4, (B, 2, h, w)).astype(np.float32)
    if kind == "dyadic":
        return (rng.integers(-48, 49, (B, 2, h, w)) / 16.0).astype(np.float32)
    if kind == "border":                       # pushes samples across every edge of the map
        f = rng.normal(0.0, 1.0, (B, 2, h, w)).astype(np.float32)
        f[:, 0] += np.where(np.arange(w) < w / 2, -0.6 * w, 0.6 * w)[None, None].astype(np.float32)
        f[:, 1] += np.where(np.arange(h) < h / 2, -0.6 * h, 0.6 * h)[None, :, None].astype(np.float32)
        return f
    sigma = float(kind)
    return (rng.normal(0.0, sigma, (B, 2, h, w))).astype(np.float32)


FLOW_KINDS = ("zero", "int", "dyadic", "0.5", "3", "20", "border")
