"""Host helpers of the correlation forward edge tests: which kernel a call reaches, feature maps with non-finite and
extreme values planted next to the zero padding, plain references, and the NaN-aware bit comparison.

The reference repacks both maps into zero-padded buffers and multiplies every tap (correlation_cuda_kernel.cu:66-69,
:124), so an infinite or NaN feature that meets a padding zero gives inf * 0 = NaN.  Every forward kernel has to return
that NaN whichever way it treats the padding (staged zeros, a bounds test, a descriptor's range), and which kernel a
call reaches depends on tile counts and pointer alignment:

  selected_kernel(B, C, H, W, pad, ...)   the choice of correlation_forward_items / vfi_correlation_forward_f16
  plant(rng, B, C, H, W, dtype)           f1, f2, [what was planted where]
  reference(f1, f2, cfg)                  float64 products over zero-padded arrays, the sum rounded as the kernels round
  padding_sites(f1, f2, cfg)              outputs whose only non-finite operand meets a padding tap
  same_bits_nan_aware(got, want)          equal NaN masks, every other element bit for bit

The thresholds and CORR_CC_ROWS are read from the sources (as tests/fi_windows.py reads its constants);
tests/test_corr_edges_host.py pins the mirror's branches to the source text.
"""
import functools
import re

import numpy as np

from tests.fi_windows import _eval, source, source_expr

SRC, DEV, BWD, SRC_BF16 = "correlation.hip", "correlation_dev.h", "correlation_bwd.h", "correlation_bf16.hip"
INT_MAX = 2 ** 31 - 1
PWC = (4, 1, 4, 1, 1)                       # pad, kernel_size, max_displacement, stride1, stride2


# ------------------------------------------------------------------ the sources

@functools.lru_cache(maxsize=None)
def constants():
    c = {n: _eval(source_expr(SRC, r"static constexpr long long %s = ([^;]*);" % n), {})
         for n in ("corr_flat_threshold", "corr_big_threshold", "corr_quad_threshold")}
    c["CORR_CC_ROWS"] = _eval(source_expr(DEV, r"#define\s+CORR_CC_ROWS\s+(\d+)"), {})
    return c


def function_body(name, src=SRC):
    """The text of function `name` of `src` (correlation.hip) from its signature to the next function at column 0."""
    text = source(src)
    m = re.search(r"^[^\n]*\b%s\([^;{]*\{" % name, text, flags=re.M | re.S)
    if not m:
        raise AssertionError("no function %s" % name)
    end = re.search(r"^\}", text[m.end():], flags=re.M)
    return text[m.start():m.end() + end.start()]


def struct_body(name, src=SRC):
    """The text of `struct name {` of `src` up to its closing brace at column 0."""
    text = source(src)
    m = re.search(r"^struct %s \{" % name, text, flags=re.M)
    if not m:
        raise AssertionError("no struct %s" % name)
    end = re.search(r"^\};", text[m.end():], flags=re.M)
    return text[m.start():m.end() + end.start()]


def source_branches(func):
    """The kernel launches of `func` in source order as (condition, kernel): the condition of the innermost `if` that
    opens between the previous launch and this one, whitespace collapsed; None for a plain `else`; "" where no branch
    opens (the function's fall-through).  A text scan, not a parser.  It assumes the layout the dispatch is written in:
    a branch that holds a launch is braced, its condition ends in `) {` and contains neither `) {` nor `;`, a plain
    else is written `else {`, and an unbraced `if (...) statement;` never holds a launch.  A dispatch reformatted
    away from that fails tests/test_corr_edges_host.py until this scan or the layout follows."""
    body = function_body(func)
    out, pos = [], 0
    for m in re.finditer(r"hipLaunchKernelGGL\(\(?(\w+)", body):
        seg = body[pos:m.start()]
        # the `if (...) {` blocks opened since the previous launch (an `if (...) return ...;` opens none)
        ifs = [(i.start(), seg[i.end():seg.find(") {", i.end())]) for i in re.finditer(r"\bif \(", seg) if seg.find(") {", i.end()) >= 0]
        ifs = [(at, c) for at, c in ifs if ";" not in c]
        e = seg.rfind("else {")
        if not ifs and e < 0:
            cond = ""                                        # no branch of its own: the function's fall-through
        elif not ifs or e > ifs[-1][0]:
            cond = None
        else:
            cond = " ".join(ifs[-1][1].split())
        out.append((cond, m.group(1)))
        pos = m.end()
    return out


# the mirror's own statement of the two dispatch chains: (condition as the source writes it, kernel)
PWC_COND = "kernel_size == 1 && stride1 == 1 && stride2 == 1 && max_displacement == 4"
BRANCHES = {
    "correlation_forward_items": [
        ("small_tiles < corr_flat_threshold * nitems", "corr_forward_k1_flat"),
        ("aligned && (out_bits & 15) == 0 && (int64_t)((ow + 63) / 64) * ((oh + 3) / 4) * batch >= corr_quad_threshold * nitems",
         "corr_forward_k1_quad"),
        ("aligned", "corr_forward_k1_rows2"),
        ("big_tiles >= corr_big_threshold * nitems", "corr_forward_k1"),
        (None, "corr_forward_k1_rows"),
        ("", "corr_forward_generic")],
    "vfi_correlation_forward_f16": [
        ("aligned && small_tiles >= 4 * corr_flat_threshold", "corr_forward_k1_rows2_f16"),
        ("", "corr_forward_generic_f16")],
}
EXPRS = {
    "correlation_forward_items": {
        "big_tiles": "(int64_t)((ow + 31) / 32) * ((oh + 7) / 8) * batch",
        "small_tiles": "(int64_t)((ow + 15) / 16) * ((oh + 3) / 4) * batch",
        "batch": "nitems * per",
        "aligned": "(w & 3) == 0 && ((max_displacement - pad_size) & 3) == 0 && (in_bits & 15) == 0 && (out_bits & 7) == 0 && "
                   "(int64_t)h * w * 4 * (CORR_CC_ROWS + 1) < INT_MAX"},
    "vfi_correlation_forward_f16": {
        "small_tiles": "(int64_t)((ow + 15) / 16) * ((oh + 3) / 4) * batch",
        "aligned": "(w & 3) == 0 && ((max_displacement - pad_size) & 3) == 0 && ((reinterpret_cast<uintptr_t>(input1) | "
                   "reinterpret_cast<uintptr_t>(input2)) & 7) == 0 && (int64_t)h * w * 2 * (CORR_CC_ROWS + 1) < INT_MAX"},
}


def out_dims(H, W, pad, k, md, s1, s2):
    border = (k - 1) // 2 + md
    dr = md // s2
    f32 = np.float32
    return ((2 * dr + 1) ** 2, int(np.ceil(f32(H + 2 * pad - 2 * border) / f32(s1))),
            int(np.ceil(f32(W + 2 * pad - 2 * border) / f32(s1))))


def selected_kernel(B, C, H, W, pad, nitems=1, aligned=True, half=False, k=1, md=4, s1=1, s2=1):
    """The kernel a forward call reaches.  `aligned`: the input tensors start on a 16-byte boundary (8 bytes for
    half); outputs are fresh allocations.  nitems = 2: vfi_correlation_forward_pair."""
    c = constants()
    _, oh, ow = out_dims(H, W, pad, k, md, s1, s2)
    pwc = k == 1 and s1 == 1 and s2 == 1 and md == 4
    batch = nitems * B
    small_tiles = ((ow + 15) // 16) * ((oh + 3) // 4) * batch
    al = W % 4 == 0 and ((md - pad) & 3) == 0 and aligned and H * W * (2 if half else 4) * (c["CORR_CC_ROWS"] + 1) < INT_MAX
    if half:
        assert nitems == 1
        if pwc and al and small_tiles >= 4 * c["corr_flat_threshold"]:
            return "corr_forward_k1_rows2_f16"
        return "corr_forward_generic_f16"
    if not pwc:
        return "corr_forward_generic"
    big_tiles = ((ow + 31) // 32) * ((oh + 7) // 8) * batch
    if small_tiles < c["corr_flat_threshold"] * nitems:
        return "corr_forward_k1_flat"
    if al and ((ow + 63) // 64) * ((oh + 3) // 4) * batch >= c["corr_quad_threshold"] * nitems:
        return "corr_forward_k1_quad"
    if al:
        return "corr_forward_k1_rows2"
    if big_tiles >= c["corr_big_threshold"] * nitems:
        return "corr_forward_k1"
    return "corr_forward_k1_rows"


# ------------------------------------------------------------------ the cases both test files run

# name -> (dtype, (B, C, H, W), (pad, k, md, s1, s2), the kernel the dense call reaches, ... at a one-element storage offset)
FLAT, ROWS2, ROWS, K1, QUAD = ("corr_forward_k1_flat", "corr_forward_k1_rows2", "corr_forward_k1_rows", "corr_forward_k1",
                                "corr_forward_k1_quad")
F32_CASES = {
    # one per float kernel: the shapes of test_correlation_forward
    "flat": ((2, 7, 8, 33), PWC, FLAT, FLAT),
    "rows2": ((2, 6, 32, 128), PWC, ROWS2, ROWS),
    "rows": ((2, 5, 33, 130), PWC, ROWS, ROWS),
    "k1": ((2, 3, 136, 514), PWC, K1, K1),
    "quad": ((2, 5, 130, 1000), PWC, QUAD, K1),
    "generic": ((2, 5, 12, 14), (3, 3, 4, 1, 2), "corr_forward_generic", "corr_forward_generic"),
    # output origin outside the frame (pad > md: the first map's taps leave it too) and inside it
    "rows2_pad8": ((2, 6, 32, 128), (8, 1, 4, 1, 1), ROWS2, ROWS),
    "quad_pad8": ((2, 5, 130, 1000), (8, 1, 4, 1, 1), QUAD, K1),
    "rows_pad5": ((2, 5, 33, 130), (5, 1, 4, 1, 1), ROWS, ROWS),
    "k1_pad3": ((2, 3, 136, 514), (3, 1, 4, 1, 1), K1, K1),
    "flat_pad2": ((2, 7, 8, 33), (2, 1, 4, 1, 1), FLAT, FLAT),
    # the flat kernel with the FIRST map's tap outside the frame: the only way into its `!ok1 && ok2` lanes
    "flat_pad8": ((2, 7, 8, 33), (8, 1, 4, 1, 1), FLAT, FLAT),
}
ORIGIN_CASES = ("rows2_pad8", "quad_pad8", "rows_pad5", "k1_pad3", "flat_pad2", "flat_pad8")
F16_CASES = {
    "generic_f16": ((2, 19, 18, 31), PWC, "corr_forward_generic_f16", "corr_forward_generic_f16"),
    "generic_f16_k3": ((2, 5, 12, 14), (3, 3, 2, 1, 2), "corr_forward_generic_f16", "corr_forward_generic_f16"),
    "rows2_f16": ((2, 19, 68, 132), PWC, "corr_forward_k1_rows2_f16", "corr_forward_generic_f16"),
    # unpadded, the 60 x 124 outputs of this shape are 240 tiles, below the tiled kernel's 256; four more rows reach it
    "generic_f16_pad0": ((2, 19, 68, 132), (0, 1, 4, 1, 1), "corr_forward_generic_f16", "corr_forward_generic_f16"),
    "rows2_f16_pad0": ((2, 19, 72, 132), (0, 1, 4, 1, 1), "corr_forward_k1_rows2_f16", "corr_forward_generic_f16"),
}
SPARSE = ("generic", "generic_f16_k3")      # kernel_size 3 on small frames: one non-finite value per place (plant)
CASES = dict([(n, (np.float32,) + v) for n, v in F32_CASES.items()] + [(n, (np.float16,) + v) for n, v in F16_CASES.items()])
SEED = 20261019


def case_inputs(name, planted=True):
    """f1, f2, planted list, cfg of a case; planted=False: the same normal values with nothing planted."""
    dtype, shape, cfg = CASES[name][:3]
    rng = np.random.default_rng([SEED, sorted(CASES).index(name)])
    if planted:
        return plant(rng, *shape, dtype, every=name not in SPARSE, kr=(cfg[1] - 1) // 2) + (cfg,)
    f1, f2 = (rng.standard_normal(shape).astype(dtype) for _ in range(2))
    return f1, f2, [], cfg


# ------------------------------------------------------------------ planted inputs

def _positions(H, W):
    """Corner, edge and interior pixels, spread over the frame (interior: off the border, and as far from it as the
    frame allows)."""
    corners = [(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0)]
    edges = [(0, W // 3), (H // 2, W - 1), (H - 1, (2 * W) // 3), (H // 3, 0), (0, (5 * W) // 6), (H - 1, W // 6)]
    ys = sorted({max(1, min(H - 2, y)) for y in (H // 2, H // 4, (3 * H) // 4)})
    interior = [(ys[n % len(ys)], max(1, min(W - 2, (W * (2 * n + 1)) // 24))) for n in range(12)]
    return corners, edges, interior


def plant(rng, B, C, H, W, dtype, every=True, kr=0):
    """Normal feature maps with the edge values of the forward kernels planted, and the list of
    (what, map, image, channel, y, x).  Every item has a pixel of its image to itself, and the images and channels
    take turns (the last channel -- the partial chunk of every kernel -- first), so what a non-finite value poisons
    stays local: 81 outputs each at kernel_size 1.  every=False plants one value per place instead of all three (+inf
    at the corner, -inf at the edge, NaN inside for f1, turned by one for f2): with kernel_size 3 a value poisons 225
    outputs, and eighteen of them would leave nothing finite on a frame of 8 x 10 outputs.  kr: the kernel radius the
    maps are meant for (the subnormal product needs every other product of its output to vanish)."""
    cc = constants()["CORR_CC_ROWS"]
    assert C % 4 and C % cc and C >= 3 and B >= 1 and H >= 3 and W >= 12, "a partial last chunk in every kernel"
    half = np.dtype(dtype) == np.float16
    f1 = rng.standard_normal((B, C, H, W)).astype(dtype)
    f2 = rng.standard_normal((B, C, H, W)).astype(dtype)
    maps = {"f1": f1, "f2": f2}
    planted = []
    corners, edges, interior = _positions(H, W)
    taken = set()

    def take(pool, b):
        for y, x in pool:
            if (b, y, x) not in taken:
                taken.add((b, y, x))
                return y, x
        raise AssertionError("frame too small for the planted set")

    def put(what, m, b, c, y, x, v):
        maps[m][b, c, y, x] = v
        planted.append((what, m, b, c, y, x))

    # +inf, -inf and NaN in each map at a corner, an edge and an interior pixel
    turn = 0
    for mi, m in enumerate(("f1", "f2")):
        for wi, (where, pool) in enumerate((("corner", corners), ("edge", edges), ("interior", interior))):
            for vi, (what, v) in enumerate((("+inf", np.inf), ("-inf", -np.inf), ("nan", np.nan))):
                if not every and vi != (wi + mi) % 3:
                    continue
                b, c = turn % B, (C - 1 - turn // B) % C
                y, x = take(pool, b)
                put("%s %s" % (what, where), m, b, c, y, x, v)
                turn += 1
    # one more within max_displacement of the corner, not on the border: with a padding smaller than the displacement the
    # border pixels are no output centres, this one is, and its taps still leave the frame
    y, x = take([(3, 3), (2, 3), (1, 3)], B - 1)
    put("+inf near border", "f1", B - 1, 0, min(y, H - 2), x, np.inf)
    big, sub = (300.0, (1e-3, 1e-3)) if half else (3e38, (1e-30, 1e-10))
    # a product that overflows; two of opposite sign in one channel column: the sequential sum passes through inf - inf.
    # (On the border: a value of 3e38 overflows against every third normal value it meets, and from an interior pixel of
    # the small frames with kernel_size 3 it meets nine times as many.)
    y, x = take(edges, 0)
    put("overflow", "f1", 0, 0, y, x, big), put("overflow", "f2", 0, 0, y, x, big)
    y, x = take(corners, B - 1)
    for c, sign in ((0, 1.0), (C - 1, -1.0)):
        put("inf - inf", "f1", B - 1, c, y, x, sign * big), put("inf - inf", "f2", B - 1, c, y, x, big)
    # a subnormal product alone in its output (the first map is zero in every other channel and kernel tap around it), so
    # the mean is subnormal too; in half a second product of one unit in the last place (6e-8 * 1) beside it
    for pool in (interior, edges):
        free = [(y, x) for y, x in pool if not any((B - 1, y + j, x + i) in taken for j in range(-kr, kr + 1) for i in range(-kr, kr + 1))]
        y, x = take(free, B - 1)
        f1[B - 1, :, max(y - kr, 0):y + kr + 1, max(x - kr, 0):x + kr + 1] = 0
        put("subnormal", "f1", B - 1, 1, y, x, sub[0]), put("subnormal", "f2", B - 1, 1, y, x, sub[1])
        if half:
            put("subnormal", "f1", B - 1, 2, y, x, 6.0e-8), put("subnormal", "f2", B - 1, 2, y, x, 1.0)
    # -0.0, next to the border and inside
    for m, pool in (("f1", edges), ("f2", interior)):
        y, x = take(pool, 0)
        put("-0.0", m, 0, C // 2, y, x, -0.0)
    return f1, f2, planted


# ------------------------------------------------------------------ plain references

def _padded(f, pad, dtype=np.float64, fill=0):
    B, C, H, W = f.shape
    p = np.full((B, C, H + 2 * pad, W + 2 * pad), fill, dtype)
    p[:, :, pad:pad + H, pad:pad + W] = f
    return p


def _taps(shape, cfg):
    """(output channel, [(rows, cols of the first map's tap, of the second's) in the padded arrays per kernel tap])"""
    pad, k, md, s1, s2 = cfg
    oc, oh, ow = out_dims(shape[2], shape[3], *cfg)
    kr, dr = (k - 1) // 2, md // s2
    ys, xs = np.arange(oh) * s1 + md, np.arange(ow) * s1 + md
    for tj in range(-dr, dr + 1):
        for ti in range(-dr, dr + 1):
            yield (tj + dr) * (2 * dr + 1) + (ti + dr), [
                ((ys + j)[:, None], (xs + i)[None, :], (ys + tj * s2 + j)[:, None], (xs + ti * s2 + i)[None, :])
                for j in range(-kr, kr + 1) for i in range(-kr, kr + 1)]


def reference(f1, f2, cfg):
    """The forward in plain numpy over zero-padded float64 arrays: every product exact in float64; the running sum is
    kept in the kernels' format (float32: one rounding per term for float maps; for half maps the product is rounded
    to half first), because whether a sum overflows to infinity is a property of that format."""
    half = f1.dtype == np.float16
    pad, k = cfg[0], cfg[1]
    B, C = f1.shape[:2]
    oc, oh, ow = out_dims(f1.shape[2], f1.shape[3], *cfg)
    p1, p2 = _padded(f1, pad), _padded(f2, pad)
    out = np.zeros((B, oc, oh, ow), f1.dtype)
    with np.errstate(all="ignore"):
        for tc, taps in _taps(f1.shape, cfg):
            acc = np.zeros((B, oh, ow), np.float32)
            for ya, xa, yb, xb in taps:
                for c in range(C):
                    prod = p1[:, c][:, ya, xa] * p2[:, c][:, yb, xb]
                    if half:
                        prod = prod.astype(np.float16)
                    acc = (acc.astype(np.float64) + prod.astype(np.float64)).astype(np.float32)
            out[:, tc] = (acc.astype(np.float64) / (k * k * C)).astype(f1.dtype)
    return out


def padding_sites(f1, f2, cfg):
    """Two boolean masks over the output: elements where a non-finite value of f1 (of f2) meets a tap of the other map
    that lies in the zero padding, and no tap of the element has a non-finite operand with both sides in the frame:
    the reference's NaN there comes from inf * 0 (NaN * 0) alone."""
    pad = cfg[0]
    B = f1.shape[0]
    oc, oh, ow = out_dims(f1.shape[2], f1.shape[3], *cfg)
    nf1, nf2 = (_padded((~np.isfinite(f)).any(axis=1, keepdims=True), pad, bool, False)[:, 0] for f in (f1, f2))
    inside = _padded(np.ones((1, 1) + f1.shape[2:], bool), pad, bool, False)[0, 0]
    s1, s2, mixed = (np.zeros((B, oc, oh, ow), bool) for _ in range(3))
    for tc, taps in _taps(f1.shape, cfg):
        for ya, xa, yb, xb in taps:
            s1[:, tc] |= nf1[:, ya, xa] & ~inside[yb, xb]
            s2[:, tc] |= nf2[:, yb, xb] & ~inside[ya, xa]
            mixed[:, tc] |= (nf1[:, ya, xa] | nf2[:, yb, xb]) & inside[ya, xa] & inside[yb, xb]
    return s1 & ~mixed, s2 & ~mixed


# ------------------------------------------------------------------ comparison

def same_bits_nan_aware(got, want):
    """NaN at the same places (payload and sign are not compared), every other element bit for bit."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    bits = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    ng, nw = np.isnan(got), np.isnan(want)
    g, w = np.ascontiguousarray(got).view(bits), np.ascontiguousarray(want).view(bits)
    return bool(np.array_equal(ng, nw) and np.array_equal(g[~ng], w[~nw]))


def describe_difference(got, want, limit=6):
    """Where two results differ under same_bits_nan_aware, for an assertion message."""
    ng, nw = np.isnan(got), np.isnan(want)
    bits = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    bad = (ng != nw) | (~ng & ~nw & (np.ascontiguousarray(got).view(bits) != np.ascontiguousarray(want).view(bits)))
    idx = np.argwhere(bad)
    return "%d of %d differ; first (index, got, want): %s" % (
        len(idx), got.size, [(tuple(i), got[tuple(i)], want[tuple(i)]) for i in idx[:limit]])


# ------------------------------------------------------------------ PWC-Net's warp in front of the correlation

def warp_geometry(flo, align_corners):
    """pwc_warp.h's sampling geometry in float32: per pixel the four corner weights, whether each corner lies in the
    map, its row and column, and the mask (1 where the in-map weights reach 0.9999)."""
    f32 = np.float32
    B, _, H, W = flo.shape
    xx, yy = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
    vx, vy = xx[None] + flo[:, 0], yy[None] + flo[:, 1]
    gx = f32(2.0) * vx / f32(max(W - 1, 1)) - f32(1.0)
    gy = f32(2.0) * vy / f32(max(H - 1, 1)) - f32(1.0)
    if align_corners:
        ix, iy = ((gx + f32(1.0)) / f32(2.0)) * f32(W - 1), ((gy + f32(1.0)) / f32(2.0)) * f32(H - 1)
    else:
        ix, iy = ((gx + f32(1.0)) * f32(W) - f32(1.0)) / f32(2.0), ((gy + f32(1.0)) * f32(H) - f32(1.0)) / f32(2.0)
    fx0, fy0 = np.floor(ix), np.floor(iy)
    assert np.all(np.abs(ix) < 1e9) and np.all(np.abs(iy) < 1e9), "finite flows only"
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    wx = (fx0 + f32(1.0) - ix, ix - fx0)
    wy = (fy0 + f32(1.0) - iy, iy - fy0)
    corners = []
    m = np.zeros(ix.shape, f32)
    for dy in (0, 1):
        for dx in (0, 1):
            wgt = (wx[dx] * wy[dy]).astype(f32)
            inmap = (x0 + dx >= 0) & (x0 + dx < W) & (y0 + dy >= 0) & (y0 + dy < H)
            m = np.where(inmap, m + wgt, m).astype(f32)
            corners.append((wgt, inmap, y0 + dy, x0 + dx))
    return corners, np.where(m < f32(0.9999), f32(0), f32(1))


def warp_zero_weight_sites(feat, flo, align_corners):
    """Pixels (boolean [B, H, W]) that read a non-finite value of `feat` through an in-map corner of weight exactly 0
    while the pixel is masked in, and pixels that are masked out although a corner they read holds one."""
    B, C, H, W = feat.shape
    nf = (~np.isfinite(feat)).any(axis=1)
    corners, mask = warp_geometry(flo, align_corners)
    bi = np.arange(B)[:, None, None]
    zero_w, touched = np.zeros((B, H, W), bool), np.zeros((B, H, W), bool)
    for wgt, inmap, y, x in corners:
        hit = inmap & nf[bi, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]
        zero_w |= hit & (wgt == 0)
        touched |= hit
    return zero_w & (mask == 1), touched & (mask == 0)


WARP_SHAPE = (2, 7, 9, 35)                  # 2 x 3 tiles of 32 x 4 with ragged right and bottom tiles, a partial chunk


def warp_inputs(align_corners):
    """f1, f2 (planted) and a finite flow for PWC-Net's warp in front of the correlation: a smooth fractional flow,
    zero -- an integer -- at the pixel to the left of every non-finite value of f2 (its east corner is in the map
    with weight 0), half a pixel outwards at a non-finite value on the right border (the pixel is masked out), and a
    block that points far outside the map."""
    B, C, H, W = WARP_SHAPE
    rng = np.random.default_rng([SEED, 99, int(align_corners)])
    f1, f2, planted = plant(rng, B, C, H, W, np.float32)
    flo = (rng.standard_normal((B, 2, H, W)) * 0.7).astype(np.float32)
    flo[:, :, :2, 20:26] = np.float32(-40.0)
    for what, m, b, c, y, x in planted:
        if m == "f2" and not np.isfinite(f2[b, c, y, x]):
            if x >= 1:
                flo[b, :, y, x - 1] = 0
            if x == W - 1:
                flo[b, :, y, x] = (0.5, 0)
    return f1, f2, flo
