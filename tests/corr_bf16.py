"""Host helpers of the bfloat16 correlation tests (vfi_correlation_forward_bf16 / _backward_bf16).  No GPU, and nothing of
the product is imported.

  to_bf16(x) / bits(x) / from_bits(b)     round-to-nearest-even through torch's CPU conversion; the uint16 patterns
  reference(f1, f2, cfg)                  float64 over explicitly zero-padded maps: R, the mean of the products, and A, the
                                          same mean over |x1 * x2| (inf * 0 = NaN in both, as in the reference's padded buffers)
  tolerance(R, A, n)                      the MFMA forward's bound, derived below
  simulate_fp32(f1, f2, cfg, order)       a CPU float32 accumulation in 32-channel chunks, channels in a chosen order
  selected_kernel(B, C, H, W, cfg)        which forward kernel a call reaches (constants read from correlation_bf16.hip)

The bound.  n = k*k*C products per output, each exact in float32 (two 8-bit significands: 16 bits).  Every float32 addition
is off by at most one float32 unit in the last place of its result, whether the adder rounds to nearest or truncates and in
whatever order the hardware adds: |S - sum p| <= n 2^-23 sum |p|.  The division adds one float32 rounding, (1 + 2^-23), and
the conversion to bfloat16 (8 significand bits, round to nearest even) 2^-9 relative, bounded here by 2^-8:

    |got - R| <= 2^-8 |R| + (1 + 2^-8) (n + 2) 2^-23 A
"""
import functools
import re

import numpy as np
import torch

from tests.corr_edges import out_dims
from tests.fi_windows import _eval, source, source_expr

SRC = "correlation_bf16.hip"
PWC = (4, 1, 4, 1, 1)                       # pad, kernel_size, max_displacement, stride1, stride2
INT_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------ bfloat16 through torch's CPU conversion

def to_bf16(x):
    """x rounded to bfloat16 (nearest even), as a float32 array holding bfloat16 values"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16)
    return t.to(torch.float32).numpy()


def bits(x):
    """the uint16 patterns of x rounded to bfloat16"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16)


def from_bits(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def same_bits(got_bits, want_bits):
    """NaN at the same places (payload and sign are not compared), every other element bit for bit; returns a message or ''"""
    got_bits, want_bits = np.asarray(got_bits), np.asarray(want_bits)
    if got_bits.shape != want_bits.shape:
        return "shapes %s / %s" % (got_bits.shape, want_bits.shape)
    g, w = from_bits(got_bits), from_bits(want_bits)
    ng, nw = np.isnan(g), np.isnan(w)
    bad = (ng != nw) | (~ng & ~nw & (got_bits != want_bits))
    if not bad.any():
        return ""
    idx = np.argwhere(bad)
    return "%d of %d differ; first (index, got, want): %s" % (len(idx), bad.size, [(tuple(i), g[tuple(i)], w[tuple(i)]) for i in idx[:6]])


# ------------------------------------------------------------------ the float64 reference and the bound

def _padded(f, pad):
    B, C, H, W = f.shape
    p = np.zeros((B, C, H + 2 * pad, W + 2 * pad), np.float64)
    p[:, :, pad:pad + H, pad:pad + W] = f
    return p


def _taps(shape, cfg):
    """(output channel, [(rows, cols) of the first map's tap and of the second's, in the padded arrays, per kernel tap])"""
    pad, k, md, s1, s2 = cfg
    oc, oh, ow = out_dims(shape[2], shape[3], *cfg)
    kr, dr = (k - 1) // 2, md // s2
    ys, xs = np.arange(oh) * s1 + md, np.arange(ow) * s1 + md
    for tj in range(-dr, dr + 1):
        for ti in range(-dr, dr + 1):
            yield (tj + dr) * (2 * dr + 1) + (ti + dr), [
                ((ys + j)[:, None], (xs + i)[None, :], (ys + tj * s2 + j)[:, None], (xs + ti * s2 + i)[None, :])
                for j in range(-kr, kr + 1) for i in range(-kr, kr + 1)]


def reference(f1, f2, cfg=PWC):
    """(R, A): float64 means of x1 * x2 and of |x1 * x2| over the k x k window and the channels, both maps zero-padded
    explicitly and every tap multiplied."""
    pad, k = cfg[0], cfg[1]
    B, C = f1.shape[:2]
    oc, oh, ow = out_dims(f1.shape[2], f1.shape[3], *cfg)
    p1, p2 = _padded(f1, pad), _padded(f2, pad)
    R, A = np.zeros((B, oc, oh, ow)), np.zeros((B, oc, oh, ow))
    with np.errstate(all="ignore"):
        for tc, taps in _taps(f1.shape, cfg):
            for ya, xa, yb, xb in taps:
                prod = p1[:, :, ya, xa] * p2[:, :, yb, xb]
                R[:, tc] += prod.sum(axis=1)
                A[:, tc] += np.abs(prod).sum(axis=1)
        n = k * k * C
        return R / n, A / n


def tolerance(R, A, n):
    return 2.0 ** -8 * np.abs(R) + (1 + 2.0 ** -8) * (n + 2) * 2.0 ** -23 * A


def check_mfma_result(got_bits, f1, f2, cfg=PWC, min_exact=0.99):
    """The checks every MFMA result gets: NaN exactly where the reference has NaN, +-inf equal, every finite output within
    the bound, and at least `min_exact` of the outputs equal to bf16_rne(R) bit for bit.  Returns the exact fraction."""
    R, A = reference(f1, f2, cfg)
    n = cfg[1] * cfg[1] * f1.shape[1]
    got = from_bits(got_bits).astype(np.float64)
    assert got.shape == R.shape, (got.shape, R.shape)
    nan = np.isnan(R)
    assert np.array_equal(np.isnan(got), nan), "NaN positions: %d got, %d wanted" % (np.isnan(got).sum(), nan.sum())
    inf = np.isinf(R)
    assert np.array_equal(got[inf], R[inf]), "infinite outputs"
    fin = ~nan & ~inf
    with np.errstate(all="ignore"):
        err, tol = np.abs(got - R), tolerance(R, A, n)
    # (an output whose bfloat16 rounding overflows is compared as a pattern below; none of the cases has one)
    over = fin & (err > tol)
    assert not over.any(), "%d outputs outside the bound; worst ratio %.3f at %s" % (
        over.sum(), (err[fin] / np.maximum(tol[fin], 1e-300)).max(), np.argwhere(over)[:4].tolist())
    exact = float((got_bits[fin] == bits(R)[fin]).mean()) if fin.any() else 1.0
    print("n %d: worst error / bound %.3f, bit-exact %.5f of %d" % (
        n, float((err[fin] / np.maximum(tol[fin], 1e-300)).max()) if fin.any() else 0.0, exact, fin.sum()))
    assert exact >= min_exact, "only %.4f of the outputs equal bf16_rne(R)" % exact
    return exact


# ------------------------------------------------------------------ a CPU float32 accumulation

def simulate_fp32(f1, f2, cfg=PWC, order=None, chunk=32):
    """The forward with float32 sums on the CPU, PWC-Net's kernel size (1): per chunk of `chunk` channels (zero-filled tail)
    the products -- exact -- are added one after the other in float32 in the order `order` (a permutation of range(chunk);
    None: ascending), the chunks' sums into the running sum in sequence; the mean by a float32 division, rounded to bfloat16.
    Returns the uint16 patterns."""
    pad, k = cfg[0], cfg[1]
    assert k == 1
    B, C = f1.shape[:2]
    oc, oh, ow = out_dims(f1.shape[2], f1.shape[3], *cfg)
    p1, p2 = _padded(f1, pad).astype(np.float32), _padded(f2, pad).astype(np.float32)
    order = list(range(chunk)) if order is None else list(order)
    out = np.zeros((B, oc, oh, ow), np.float32)
    with np.errstate(all="ignore"):
        for tc, taps in _taps(f1.shape, cfg):
            (ya, xa, yb, xb), = taps
            prod = p1[:, :, ya, xa] * p2[:, :, yb, xb]                      # exact: 16 significand bits
            acc = np.zeros((B, oh, ow), np.float32)
            for c0 in range(0, C, chunk):
                part = np.zeros((B, oh, ow), np.float32)
                for c in order:
                    if c0 + c < C:
                        part = part + prod[:, c0 + c]
                acc = acc + part
            out[:, tc] = acc / np.float32(C)
    return bits(out)


# ------------------------------------------------------------------ which kernel a forward call reaches

@functools.lru_cache(maxsize=None)
def constants():
    mt, th = re.search(r"typedef CorrMfmaTile<\s*(\d+)\s*,\s*(\d+)\s*>\s*CorrMfma;", source(SRC)).groups()
    return {"corr_bf16_mfma_threshold": _eval(source_expr(SRC, r"static constexpr long long corr_bf16_mfma_threshold = ([^;]*);"), {}),
            "TW": 16 * int(mt), "TH": int(th), "KC": _eval(source_expr(SRC, r"\bKC = (\d+)"), {})}


def selected_kernel(B, C, H, W, cfg=PWC):
    """'mfma' or 'generic': the dispatch of vfi_correlation_forward_bf16"""
    c = constants()
    pad, k, md, s1, s2 = cfg
    _, oh, ow = out_dims(H, W, *cfg)
    pwc = k == 1 and s1 == 1 and s2 == 1 and md == 4
    fits = H * W * 2 * c["KC"] < INT_MAX and B <= 65535 and (oh + c["TH"] - 1) // c["TH"] <= 65535
    tiles = ((ow + c["TW"] - 1) // c["TW"]) * ((oh + c["TH"] - 1) // c["TH"]) * B
    return "mfma" if pwc and fits and tiles >= c["corr_bf16_mfma_threshold"] else "generic"
