"""Host helpers of the side-op tests: planted inputs, class censuses and expected values for Interpolation /
InterpolationCh, SeparableConv, SeparableConvFlow (csrc/warp_sepconv.hip) and MinDepthFlowProjection
(csrc/mindepth.hip), in the manner of tests/forward_edges.py.  numpy and the oracle only.

Each of these ops is made of comparisons whose two sides random, finite, well-scaled inputs almost never separate; the
inputs here sit exactly on them:

  interp_border()                 flows that fail or pass Interpolation's validity test by a subnormal, -0.0, x2 == w
  sep_shapes() / sep_dyadic()     SeparableConv's channel tail (C % 3 != 0) against its eight-tap block (fs = 7 ... 17)
  sep_planted(fs)                 non-finite, huge, subnormal and -0.0 values in the image, in v and in h
  sepflow_planted()               tap vectors whose sum is +0, -0, subnormal, inf, NaN, inf - inf, overflowing
  pattern(shape, salt)            the non-zero dyadic starting gradients of the accumulation tests
  md_zero_tie(name)               signed-zero weights tied over a negative floor (MinDepthFlowProjection's tie rule)
  md_holes()                      a 200 x 300 incoming count that drives the hole filler's bitmap walks exactly
  md_walks(count)                 numpy: per cell and direction, the position of the nearest cell with count != 0
  md_backward()                   sources on the last column / row / corner, +-0, NaN, inf against the count

Everything finite that is planted is dyadic, so the sums are exact in any order: the GPU tests compare bit for bit.
"""
import numpy as np

from tests.forward_edges import FLT_MAX, describe_difference, same_bits_nan_aware  # noqa: F401  (re-exported)

f32 = np.float32
SUB = 2.0 ** -149                                           # "1e-45": the smallest subnormal
SEED = 20261021
INVALID = f32(1000.0)                                       # a flow that leaves every frame used here


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def pattern(shape, salt=0):
    """Non-zero dyadic starting gradients: odd multiples of 1/4 in [-7.75, 7.75], different in every element's neighbourhood."""
    n = int(np.prod(shape))
    k = (np.arange(n, dtype=np.int64) * 7 + 3 * salt) % 31 - 15
    return ((2 * k + 1) / 4.0).astype(f32).reshape(shape)


# ------------------------------------------------------------------ Interpolation

BORDER_SHAPE = (2, 2, 12, 20)


def interp_border(shape=BORDER_SHAPE):
    """(img, flow, expect): integer-valued image cells (every cell a different value, exact in float), zero flow, and the
    border decisions of interp_forward's validity test `x2 >= 0 && y2 >= 0 && x2 < w && y2 < h` planted in both items.
    expect: [(what, y, x, cell)] with cell the (y, x) of the image cell the output must equal, None for an invalid pixel
    (0 in every channel)."""
    B, C, H, W = shape
    img = (1 + np.arange(B * C * H * W, dtype=np.int64)).astype(f32).reshape(shape)
    flow = np.zeros((B, 2, H, W), f32)
    expect = []

    def put(what, y, x, comp, v, cell):
        flow[:, comp, y, x] = v
        expect.append((what, y, x, cell))

    for k, (name, v, valid) in enumerate((("-2^-149", -SUB, False), ("+2^-149", SUB, True), ("-0.0", -0.0, True))):
        put("x:col0:" + name, 3 + k, 0, 0, v, (3 + k, 0) if valid else None)
        put("y:row0:" + name, 0, 3 + k, 1, v, (0, 3 + k) if valid else None)
    put("x:interior:-2^-149", 6, 7, 0, -SUB, (6, 7))        # x + fx == x
    put("y:interior:-2^-149", 6, 9, 1, -SUB, (6, 9))
    put("x2==w", 7, W - 5, 0, 5.0, None)
    put("x2==w-0.5", 8, W - 5, 0, 4.5, (8, W - 1))          # L = R = w - 1: both halves read the last column
    put("y2==h", H - 4, 3, 1, 4.0, None)
    put("y2==h-0.5", H - 4, 4, 1, 3.5, (H - 1, 4))
    return img, flow, expect


def interp_border_expected(img, expect):
    """The output the plants name: img itself (zero flow) except at the planted pixels."""
    out = img.copy()
    for what, y, x, cell in expect:
        out[:, :, y, x] = 0.0 if cell is None else img[:, :, cell[0], cell[1]]
    return out


# ------------------------------------------------------------------ SeparableConv

SEP_CHANNELS = (1, 2, 4, 5, 7)                              # sepconv_forward<3>: every remainder, one and two full groups
SEP_SIZES = (7, 8, 9, 16, 17)                               # tail only, one eight-tap block, block + 1, two blocks, two + 1
_SEP_OUT = ((20, 66), (17, 65), (9, 63), (5, 37), (3, 5))   # out frames: no width a multiple of 64, one and two blocks wide


def sep_shapes():
    """[(C, fs, oh, ow)]: every channel count with every filter size, the out frame taking turns."""
    return [(C, fs) + _SEP_OUT[(i + j) % len(_SEP_OUT)] for i, C in enumerate(SEP_CHANNELS) for j, fs in enumerate(SEP_SIZES)]


def sep_dyadic(C, fs, oh, ow, B=2):
    """dict(img, v, h, gout, gflow): eighths in the image, quarters in the taps, halves in the gradients.  A product is a
    multiple of 2^-7 below 8 and a sum has at most 17 * 17 * 7 of them: below 2^24 units, exact in any order."""
    rng = np.random.default_rng([SEED, 2, C, fs, oh, ow])
    H, W = oh + fs - 1, ow + fs - 1
    return dict(img=(rng.integers(-16, 17, (B, C, H, W)) / 8).astype(f32),
                v=(rng.integers(-8, 9, (B, fs, oh, ow)) / 4).astype(f32),
                h=(rng.integers(-8, 9, (B, fs, oh, ow)) / 4).astype(f32),
                gout=(rng.integers(-8, 9, (B, C, oh, ow)) / 2).astype(f32),
                gflow=(rng.integers(-8, 9, (B, 2, oh, ow)) / 2).astype(f32))


SEP_PLANT_SET = (("+inf", np.inf), ("-inf", -np.inf), ("nan", np.nan), ("+FLT_MAX", FLT_MAX), ("-FLT_MAX", -FLT_MAX),
                 ("+2^-149", SUB), ("-2^-149", -SUB), ("-0.0", -0.0))
SEP_PLANT_SIZES = (5, 9)                                    # the tail loop alone, and the eight-tap block + tail
SEP_PLANT_FRAME = (2, 3, 24, 70)


def sep_planted(fs, frame=SEP_PLANT_FRAME):
    """sep_dyadic's kind of inputs on `frame` with SEP_PLANT_SET planted once each in the image (channels and items taking
    turns), in v and in h -- three sets of pixels apart from each other.  Returns the dict with planted: [(where, name, index)]."""
    B, C, H, W = frame
    oh, ow = H - fs + 1, W - fs + 1
    d = sep_dyadic(C, fs, oh, ow, B)
    planted = []
    n = len(SEP_PLANT_SET)
    for k, (name, val) in enumerate(SEP_PLANT_SET):
        at = (k % B, (C - 1 - k) % C, 1 + (k * (H - 3)) // (n - 1), 2 + (k * 5 * (W - 5) // (n - 1)) % (W - 4))
        d["img"][at] = val
        planted.append(("img", name, at))
        at = ((k + 1) % B, (3 * k) % fs, 1 + (k * 3) % (oh - 2), 3 + k * (ow - 6) // n)
        d["v"][at] = val
        planted.append(("v", name, at))
        at = (k % B, (2 * k + 1) % fs, oh - 2 - (k * 3) % (oh - 2), 5 + k * (ow - 8) // n)
        d["h"][at] = val
        planted.append(("h", name, at))
    d["planted"] = planted
    return d


def nonfinite_census(a):
    """(share of non-finite elements, has NaN, has +inf, has -inf)"""
    return float((~np.isfinite(a)).mean()), bool(np.isnan(a).any()), bool((a == np.inf).any()), bool((a == -np.inf).any())


# ------------------------------------------------------------------ SeparableConvFlow

SEPFLOW_FS = 5
# (name, the five taps, the flow the oracle gives: (mom / sum) - 2, or -2000 where |sum| > 0 is false)
SEPFLOW_VECTORS = (("cancel", (1.0, -1.0, 1.0, -1.0, 0.0), -2000.0),
                   ("all -0.0", (-0.0, -0.0, -0.0, -0.0, -0.0), -2000.0),
                   ("2^-149 first", (SUB, 0.0, 0.0, 0.0, 0.0), -2.0),       # a kernel that flushes denormals: -2000
                   ("2^-149 last", (0.0, 0.0, 0.0, 0.0, SUB), 2.0),
                   ("inf", (np.inf, 1.0, 1.0, 1.0, 1.0), np.nan),           # mom = 0 * inf
                   ("nan", (np.nan, 1.0, 1.0, 1.0, 1.0), -2000.0),          # |NaN| > 0 is false
                   ("overflow", (FLT_MAX, FLT_MAX, 0.0, 0.0, 0.0), -2.0),   # sum = inf, mom = FLT_MAX: 0 - 2
                   ("inf - inf", (np.inf, -np.inf, 0.0, 0.0, 0.0), -2000.0),
                   ("1e-30", (1e-30, 0.0, 0.0, 0.0, 1e-30), 0.0))
SEPFLOW_ROW_V, SEPFLOW_ROW_H = 3, 7                         # out rows that carry the vectors in v / in h
SEPFLOW_BOTH = 4                                            # the vector index whose v pixel carries an h vector too


def sepflow_x(k, step=3):
    return 2 + step * k


def sepflow_planted(frame=(2, 3, 24, 70), step=3):
    """sep_dyadic inputs at fs = 5 with SEPFLOW_VECTORS in v along out row SEPFLOW_ROW_V and in h along SEPFLOW_ROW_H, both
    items (the y and x decisions are independent), every `step` columns; the pixel of v's vector SEPFLOW_BOTH carries h's
    vector 2 as well."""
    B, C, H, W = frame
    fs = SEPFLOW_FS
    d = sep_dyadic(C, fs, H - fs + 1, W - fs + 1, B)
    # the dyadic background must decide too: no tap sum of exactly zero outside the plants
    for key in ("v", "h"):
        zero = d[key].sum(1) == 0
        d[key][:, 0][zero] += f32(0.25)
    for k, (name, taps, _) in enumerate(SEPFLOW_VECTORS):
        d["v"][:, :, SEPFLOW_ROW_V, sepflow_x(k, step)] = np.array(taps, f32)
        d["h"][:, :, SEPFLOW_ROW_H, sepflow_x(k, step)] = np.array(taps, f32)
    d["h"][:, :, SEPFLOW_ROW_V, sepflow_x(SEPFLOW_BOTH, step)] = np.array(SEPFLOW_VECTORS[2][1], f32)
    return d


SMALL_FRAME = (2, 3, 12, 20)                                # the versions the reference's own code runs on the CPU


def sepflow_expected(step=3):
    """[(x, flow)] along the planted rows: the flow the oracle gives for SEPFLOW_VECTORS (NaN: a NaN)."""
    return [(sepflow_x(k, step), want) for k, (_, _, want) in enumerate(SEPFLOW_VECTORS)]


def sepflow_finite(fs, oh=20, ow=66, B=2):
    """Finite dyadic taps for the other filter sizes, with tap sums of exactly +0 at a few pixels (all-zero taps; fs >= 2:
    a cancelling pair as well)."""
    d = sep_dyadic(3, fs, oh, ow, B)
    d["v"][0, :, 2, 3] = 0
    d["h"][1, :, oh - 1, ow - 1] = 0
    if fs >= 2:
        d["v"][1, :, 5, 65] = 0
        d["v"][1, :2, 5, 65] = (1.5, -1.5)
    return d


# ------------------------------------------------------------------ MinDepthFlowProjection: signed-zero ties

MD_TIE_NAMES = ("-0,+0", "+0,-0", "-0,+0,-0", "far block", "item 1")
MD_FLOOR = f32(-1.0)


def md_zero_tie(name):
    """(flow, weight, count0, expect): every flow invalid but those of two or three sources that land on one target, whose
    weights are zeros of the given signs in raster order; the incoming count is MD_FLOOR < 0 everywhere, so every zero beats
    it and the zeros tie with each other -- `+0 > -0` is false: the first source in raster order keeps the target.
    expect: (b, ty, tx, the first source's (y, x)).  "far block": the raster-earlier source lies in a later 64 x 4 block
    of the launch than the other (flows of 30 px).  "item 1": B = 2, the -0 then +0 tie in item 1, +0 then -0 in item 0."""
    signs = {"-0,+0": (-0.0, 0.0), "+0,-0": (0.0, -0.0), "-0,+0,-0": (-0.0, 0.0, -0.0), "far block": (-0.0, 0.0), "item 1": (-0.0, 0.0)}[name]
    B, H, W = (2, 12, 20) if name == "item 1" else (1, 8, 100) if name == "far block" else (1, 12, 20)
    flow = np.full((B, 2, H, W), INVALID, f32)
    wgt = np.full((B, 1, H, W), f32(0.5), f32)
    count0 = np.full((B, 1, H, W), MD_FLOOR, f32)
    if name == "far block":
        target, srcs = (2, 40), [(1, 70), (2, 10)]          # (1, 70): block (1, 0); (2, 10): block (0, 0)
    else:
        target, srcs = (5, 9), [(4, 8), (4, 11), (6, 9)][:len(signs)]
    items = [(B - 1, signs)] + ([(0, signs[::-1])] if name == "item 1" else [])
    expect = []
    for b, sg in items:
        for (y, x), s in zip(srcs, sg):
            flow[b, :, y, x] = (target[1] - x, target[0] - y)
            wgt[b, 0, y, x] = s
        expect.append((b, target[0], target[1], srcs[0]))
    return flow, wgt, count0, expect


# ------------------------------------------------------------------ MinDepthFlowProjection: designed holes

MD_HOLE_SHAPE = (2, 200, 300)
MD_DISTANCES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 161)
MD_ROW_ONLY = (257,)
# (y, x, count) of item 0; item 1 is item 0 mirrored left to right.  Positive cells on bit 0, on bit 31 and in the last,
# partial word of a row (w = 300: word 9 holds 12 bits) and of a column (h = 200: word 6 holds 8 bits): their whole row
# and column are holes that walk to them, from every distance.  The four cells at the end are found cells that are not
# plain positive counts; their own rows and columns hold nothing else (md_hole_rule).
MD_CELLS = ((10, 0, 0.25), (12, 299, 2.0), (14, 31, 0.5), (14, 288, 1.0), (16, 64, 0.125), (16, 191, 4.0),
            (0, 5, 0.5), (199, 9, 2.0), (31, 13, 0.25), (192, 13, 1.0), (64, 17, 8.0), (159, 17, 0.125),
            (110, 150, -0.5), (130, 170, -np.inf), (150, 190, np.inf), (170, 210, np.nan))


def md_holes():
    """(flow, weight, count0, out0): every flow invalid, so the forward writes nothing -- count stays the incoming count and
    output what the caller put there -- and the filler runs on exactly these arrays.  out0: distinct quarters."""
    B, H, W = MD_HOLE_SHAPE
    flow = np.full((B, 2, H, W), INVALID, f32)
    wgt = np.full((B, 1, H, W), f32(0.5), f32)
    count0 = np.zeros((B, 1, H, W), f32)
    for y, x, c in MD_CELLS:
        count0[0, 0, y, x] = c
        count0[1, 0, y, W - 1 - x] = c
    out0 = ((1 + np.arange(B * 2 * H * W, dtype=np.int64)) / 4.0).astype(f32).reshape(B, 2, H, W)
    return flow, wgt, count0, out0


def md_walks(count):
    """count [B, 1, H, W] -> dict(left, right, up, down): int arrays [B, H, W], the x (left, right) or y (up, down) of the
    nearest cell strictly beyond each cell with count != 0 (NaN counts: != 0), -1 where there is none -- what
    proj_bit_walk returns on the bitmaps of mindepth_award."""
    nz = count[:, 0] != 0
    B, H, W = nz.shape

    def before(nz, n, axis):
        shape = [1, 1, 1]
        shape[axis] = n
        idx = np.where(nz, np.arange(n).reshape(shape), -1)
        run = np.maximum.accumulate(idx, axis=axis)
        out = np.full_like(run, -1)
        sl_to, sl_from = [slice(None)] * 3, [slice(None)] * 3
        sl_to[axis], sl_from[axis] = slice(1, None), slice(0, -1)
        out[tuple(sl_to)] = run[tuple(sl_from)]
        return out

    def after(nz, n, axis):
        r = before(np.flip(nz, axis), n, axis)
        r = np.flip(r, axis)
        return np.where(r < 0, -1, n - 1 - r)

    return dict(left=before(nz, W, 2), right=after(nz, W, 2), up=before(nz, H, 1), down=after(nz, H, 1))


def md_found_counts(count, walks):
    """Per direction, the count at the found cell (0 where the walk found none)."""
    B, _, H, W = count.shape
    c = count[:, 0]
    bi, yi, xi = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    out = {}
    for k, pos in walks.items():
        p = np.maximum(pos, 0)
        got = c[bi, yi, p] if k in ("left", "right") else c[bi, p, xi]
        out[k] = np.where(pos < 0, f32(0), got)
    return out


def md_hole_census(count):
    """dict: distances per direction over the holes (count <= 0), the numbers of sides on which a hole's walk found nothing,
    the bit positions and words of the found cells per axis, the kinds of found counts."""
    B, _, H, W = count.shape
    walks = md_walks(count)
    hole = count[:, 0] <= 0
    pos = {"left": np.arange(W)[None, None, :], "right": np.arange(W)[None, None, :], "up": np.arange(H)[None, :, None],
           "down": np.arange(H)[None, :, None]}
    dist, nothing = {}, np.zeros(hole.shape, int)
    cells = {"x": set(), "y": set()}
    for k, found in walks.items():
        ok = hole & (found >= 0)
        dist[k] = set(np.abs(found - pos[k])[ok].tolist())
        nothing += (found < 0)
        cells["x" if k in ("left", "right") else "y"] |= set(found[ok].tolist())
    fc = md_found_counts(count, walks)
    kinds = set()
    for k, v in fc.items():
        v = v[hole & (walks[k] >= 0)]
        kinds |= {name for name, m in (("positive", (v > 0) & np.isfinite(v)), ("negative", (v < 0) & np.isfinite(v)),
                                       ("-inf", v == -np.inf), ("+inf", v == np.inf), ("nan", np.isnan(v))) if m.any()}
    return dict(dist=dist, nothing=set(nothing[hole].tolist()), cells=cells, kinds=kinds)


def md_hole_rule(count):
    """The plants' constraint: a cell with count <= 0 that some walk finds (count != 0) must be left unchanged by the
    filler -- its own four walks meet no positive count and no NaN (a NaN gets past the filler's `sum <= 0` test).  Then
    no filled value depends on the order the holes are visited in.  Returns the offending cells."""
    walks = md_walks(count)
    fc = md_found_counts(count, walks)
    c = count[:, 0]
    found_hole = (c <= 0) & (c != 0)
    bad = np.zeros(c.shape, bool)
    for v in fc.values():
        bad |= found_hole & ((v > 0) | np.isnan(v))
    return np.argwhere(bad)


# ------------------------------------------------------------------ MinDepthFlowProjection backward

MD_BWD_SHAPE = (2, 12, 20)


def md_backward(shape=MD_BWD_SHAPE):
    """(flow, weight, count, gout, expect): a background of random integer flows with weights in eighths against the
    forward's own count (many equalities), then planted sources whose four comparisons `weight == count[T / Bm, L / R]`
    are set by hand.  expect: [(what, b, y, x, [(ty, tx, times)])] -- the gradient of that source is the sum of
    -gout[b, :, ty, tx] * times (R == L on the last column and Bm == T on the last row name one target twice)."""
    from oracle import cpu_oracle
    B, H, W = shape
    rng = np.random.default_rng([SEED, 5])
    flow = rng.integers(-2, 3, (B, 2, H, W)).astype(f32)
    wgt = (rng.integers(1, 9, (B, 1, H, W)) / 8).astype(f32)
    _, count = cpu_oracle.mindepthflowproj_fwd(flow, wgt, 0)
    gout = (rng.integers(-8, 9, (B, 2, H, W)) / 2).astype(f32)
    gout[gout == 0] = f32(0.5)                              # every target's gradient tells
    expect = []
    b = B - 1                                               # the plants: item B - 1; no two of them share a target cell

    def plant(what, y, x, ty, tx, w, cells):
        """source (y, x) -> top-left target (ty, tx) with weight w; cells: {(cy, cx): count} for its up to four targets"""
        flow[b, :, y, x] = (tx - x, ty - y)
        wgt[b, 0, y, x] = w
        R, Bm = min(tx + 1, W - 1), min(ty + 1, H - 1)
        four = [(ty, tx), (ty, R), (Bm, tx), (Bm, R)]
        for cell in set(four):
            count[b, 0, cell[0], cell[1]] = cells.get(cell, f32(99.0))       # 99: no weight equals it
        hits = {}
        for cell in four:
            cv = count[b, 0, cell[0], cell[1]]
            if f32(w) == cv:
                hits[cell] = hits.get(cell, 0) + 1
        expect.append((what, b, y, x, [(cy, cx, n) for (cy, cx), n in sorted(hits.items())]))

    plant("last column", 1, W - 3, 1, W - 1, 0.375, {(1, W - 1): f32(0.375)})                     # R == L: twice
    plant("last column, both rows", 4, W - 2, 3, W - 1, 0.625, {(3, W - 1): f32(0.625), (4, W - 1): f32(0.625)})
    plant("last row", H - 3, 3, H - 1, 3, 0.375, {(H - 1, 3): f32(0.375)})                         # Bm == T: twice
    plant("corner", H - 2, W - 4, H - 1, W - 1, 0.875, {(H - 1, W - 1): f32(0.875)})               # four times
    plant("+0 weight, -0 count", 6, 2, 6, 3, 0.0, {(6, 3): f32(-0.0)})
    plant("-0 weight, +0 count", 6, 6, 6, 7, -0.0, {(6, 7): f32(0.0)})
    plant("nan, nan", 6, 10, 6, 11, np.nan, {(6, 11): f32(np.nan), (7, 11): f32(np.nan)})         # never equal
    plant("+inf, +inf", 8, 2, 8, 3, np.inf, {(8, 3): f32(np.inf)})
    plant("-inf, -inf", 8, 6, 8, 7, -np.inf, {(9, 8): f32(-np.inf)})                              # at the far corner only
    plant("neighbour only", 8, 10, 8, 11, 0.75, {(8, 12): f32(0.75), (9, 11): f32(0.75)})         # not its own top-left
    return flow, wgt, count, gout, expect


def md_backward_expected(gout, expect, start):
    """start + the planted sources' hand-computed gradients, at the planted sources only: {(b, y, x): [gx, gy]}"""
    out = {}
    for what, b, y, x, hits in expect:
        g = start[b, :, y, x].astype(np.float64)
        for ty, tx, n in hits:
            g = g - n * gout[b, :, ty, tx].astype(np.float64)
        out[(b, y, x)] = g.astype(f32)
    return out
