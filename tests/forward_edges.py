"""Host helpers of the forward edge tests: non-finite and extreme values planted into the inputs of FilterInterpolation,
the projections, the PWC-Net warp and MinDepthFlowProjection, in the manner of tests/corr_edges.py (whose NaN-aware bit
comparison they use).

FilterInterpolation multiplies every tap of a valid pixel's window, replicated border taps included, and copies an
invalid pixel's input through (oracle/vfi_oracle.c: fi_valid, fi_quadrants), so an infinity inside a window gives
+-inf, or NaN where it meets a zero weight or an infinity of the other sign, and a value outside every window of a
pixel must not reach that pixel.

  plant_fi(kernel, field, img, filt, rng, classify)   planted image, flow and filters on a field of fi_windows.build_field
  fi_case(kernel, C, aligned, fs)                     the planted inputs both test files run, per kernel and channel count
  class_caps / differing_by_class / clamped_windows   per-class summaries of an oracle result and of a comparison
  small_proj_inputs / small_fi_inputs / small_interp_inputs   small planted frames for the reference's own code on the CPU

The reference adds every source's weight and weighted flow to four cells with fp32 atomics and multiplies a hole's
neighbours by 0 / 1 weights (oracle/vfi_oracle.c: project, fillhole_pass), so a NaN or infinite weight gives a NaN or
infinite count and a NaN flow in exactly those four cells, and a hole whose nearest neighbour is such a cell becomes NaN
through 0 * NaN.  The library has to return the same cells, bit for bit, whichever K0 / K1 pair a call reaches.

  FLOW_SET, WEIGHT_SET                      the planted values
  plant_proj(kind, field, rng)              flow, depth, [(what, b, y, x)] on a field of proj_tiles.build_field
  proj_regions(planted, flow, h, w)         {what: boolean [h, w] mask of the four target cells of its sources}
  clean_field(kind, rng, B, h, w)           a small dyadic field with nothing planted
  up4_inputs(kind, rng)                     quarter-resolution flow with NaN and Inf, full-resolution planted depth
  warp_inputs(shape, align_corners)         features and a finite flow for pwc_warp_forward
  mindepth_inputs(shape, rng)               flow, weights, incoming count for MinDepthFlowProjection's order edges
  same_bits_nan_aware / same_nonfinite_mask comparisons

Everything finite that is planted is dyadic and kept apart from every other planted value, so that a finite cell's sum
is exact in any order of the atomics and a non-finite cell is non-finite in any order.
"""
import numpy as np

from tests import proj_tiles as pt
from tests.corr_edges import describe_difference, same_bits_nan_aware  # noqa: F401  (re-exported)

f32 = np.float32
FLT_MAX = float(np.finfo(f32).max)
NEG_NAN = np.array([0xffc00000], np.uint32).view(f32)[0]
POS_NAN = np.array([0x7fc00000], np.uint32).view(f32)[0]

# flows: NaN of both signs, +-inf, +-3e38, -0.0 and the largest negative subnormal (at column / row 0 it is the smallest
# step out of the frame: x2 = 0 + -2^-149 < 0, while 0 + -0.0 = +0 stays valid)
FLOW_SET = (("nan", POS_NAN), ("-nan", NEG_NAN), ("+inf", np.inf), ("-inf", -np.inf), ("+3e38", 3e38), ("-3e38", -3e38),
            ("-0.0", -0.0), ("-2^-149", -2.0 ** -149))
WEIGHT_SET = (("+inf", np.inf), ("-inf", -np.inf), ("nan", np.nan))
HUGE_WEIGHTS = (("2^100", 2.0 ** 100), ("2^120", 2.0 ** 120), ("FLT_MAX", FLT_MAX))
FEATURE_SET = (("+inf", np.inf), ("-inf", -np.inf), ("nan", np.nan), ("-0.0", -0.0), ("+FLT_MAX", FLT_MAX), ("-FLT_MAX", -FLT_MAX),
               ("FLT_MIN", float(np.finfo(f32).tiny)), ("2^-149", 2.0 ** -149), ("2^-127", 2.0 ** -127))

DEPTH_REGIMES = ("plain", "classes", "edge", "wide_cell")    # the tile regimes that get non-finite weights
TINY_ROWS, TINY_COLS = (64, 96), (384, 464)                  # whole 16x16 blocks: every weight in [2^-149, 2^-80]
HUGE_BLOCK = (48, 480)                                       # a block far from every site: 2^100, 2^120, FLT_MAX
HOLE_SOURCE = (5, pt.TW)                                     # the first source right of the empty tile (0, 0), whose cells are
#                                                              the nearest neighbours of that tile's holes in rows 5 and 6


def same_nonfinite_mask(got, want):
    """The looser comparison: non-finite (NaN or infinite) at the same places; which of the two is not compared."""
    got, want = np.asarray(got), np.asarray(want)
    return bool(got.shape == want.shape and np.array_equal(~np.isfinite(got), ~np.isfinite(want)))


# ------------------------------------------------------------------ FilterInterpolation

FILTER_SET = (("+0.0", 0.0), ("-0.0", -0.0), ("+inf", np.inf), ("-inf", -np.inf), ("nan", np.nan), ("+FLT_MAX", FLT_MAX),
              ("-FLT_MAX", -FLT_MAX), ("2^-149", 2.0 ** -149))
# fp16 storage: nothing planted overflows half (65504), in the image or -- times a filter tap below 1/4, sixteen of them --
# in a sum; a half subnormal and the smallest normal stand in for the float ones
FEATURE_SET_F16 = (("+inf", np.inf), ("-inf", -np.inf), ("nan", np.nan), ("-0.0", -0.0), ("+1000", 1000.0), ("-1000", -1000.0),
                   ("2^-14", 2.0 ** -14), ("2^-24", 2.0 ** -24), ("2^-20", 2.0 ** -20))
FILTER_SET_F16 = (("+0.0", 0.0), ("-0.0", -0.0), ("+inf", np.inf), ("-inf", -np.inf), ("nan", np.nan), ("2^-149", 2.0 ** -149))


def plant_fi(kernel, field, img, filt, rng, classify, fs=4):
    """(img, flow, filt, planted) -- planted copies of an image, of the flow of a field of fi_windows.build_field and of
    the filters.  classify(flow) -> the class label per (item, tile row, tile column), as fi_windows.classes gives it for
    the kernel and layout under test.

    Image and filter values go into one tile of EVERY class present (the gather and the no-valid-pixel tiles included):
    an image value at the sample position (int)y2, (int)x2 of one of the tile's pixels -- inside that pixel's window,
    so it reaches the tile's outputs wherever the flow points -- or, where the pixel is invalid, at the pixel itself
    (it is copied through); a filter value in one tap of another pixel of the tile.  The four frame corners and a pixel
    on each border get image values too (a replicated tap multiplies the same value several times), with taps of +0.0
    and -0.0 in the pixels around each corner.  Flow values (FLOW_SET, +-w/2 and +-h/2 exactly, and the flow that makes
    x2 == w - 1) go to pixels of tiles of two different classes; the classes are computed again afterwards -- a
    non-finite flow is an invalid pixel that adds nothing to its tile's box -- and every class must still be there."""
    from tests import fi_windows as fw
    flow = field["flow"].copy()
    img, filt = img.copy(), filt.copy()
    half = img.dtype == np.float16
    feats, taps = (FEATURE_SET_F16, FILTER_SET_F16) if half else (FEATURE_SET, FILTER_SET)
    feats = feats + feats[:3]                               # the non-finite ones twice: a later plant may take a pixel or its flow
    B, C, h, w = img.shape
    th, tw = fw.geometry(kernel, fs)[:2]
    lab = classify(flow)
    before = set(lab.ravel())
    valid, ix, iy, _, _ = fw.samples(flow, h, w)
    planted = []
    turn = 0

    def lattice(ty, tx):
        for sy, sx in ((2, 3), (1, 2), (1, 1)):             # (a ragged last tile is smaller)
            p = [(y, x) for y in range(ty * th, min(h, ty * th + th), sy) for x in range(tx * tw, min(w, tx * tw + tw), sx)]
            if len(p) >= len(feats) + len(taps):
                break
        return [p[i] for i in rng.permutation(len(p))]

    chosen = {}
    for label in sorted(before):
        tiles = np.argwhere(lab == label)
        b, ty, tx = (int(v) for v in tiles[int(rng.integers(len(tiles)))])
        chosen[label] = (b, ty, tx)
        pix = lattice(ty, tx)
        assert len(pix) >= len(feats) + len(taps), (label, len(pix))
        for (name, v), (y, x) in zip(feats, pix):
            py, px = (int(iy[b, y, x]), int(ix[b, y, x])) if valid[b, y, x] else (y, x)
            img[b, (C - 1 - turn) % C, py, px] = v
            planted.append(("img:" + name, label, b, py, px))
            turn += 1
        for (name, v), (y, x) in zip(taps, pix[len(feats):]):
            filt[b, int(rng.integers(filt.shape[1])), y, x] = v
            planted.append(("filt:" + name, label, b, y, x))
    # corners and borders
    spots = [(0, 0), (h - 1, w - 1), (0, w - 1), (h - 1, 0), (0, w // 2), (h // 2, 0), (h - 1, w // 3), (h // 3, w - 1)]
    for k, (y, x) in enumerate(spots):
        name, v = feats[k % 3] if k < 6 else feats[4 + k % 2]
        img[k % B, (C - 1 - k) % C, y, x] = v
        planted.append(("img:" + name, "border", k % B, y, x))
    for (y, x) in spots[:4]:
        ys, xs = slice(max(y - 1, 0), y + 2), slice(max(x - 1, 0), x + 2)
        filt[:, 0, ys, xs], filt[:, filt.shape[1] - 1, ys, xs] = 0.0, -0.0
    # flows, in tiles of two classes that have valid pixels
    fl_set = list(FLOW_SET) + [("+w/2", w / 2.0), ("-w/2", -w / 2.0), ("+h/2", h / 2.0), ("-h/2", -h / 2.0), ("x2=w-1", None)]
    two = [lb for lb in sorted(before) if lb not in ("none", "gather")]
    two = [two[0], two[-1]]
    for n, label in enumerate(two):
        # (another tile of the class than the one that holds its image and filter values, where there is one: an invalid
        #  pixel adds nothing to its tile's box, which may move that tile to another class)
        others = [t for t in map(tuple, np.argwhere(lab == label)) if t != chosen[label]]
        b, ty, tx = (int(v) for v in others[0]) if others else chosen[label]
        pix = lattice(ty, tx)[-len(fl_set):]
        for k, ((name, v), (y, x)) in enumerate(zip(fl_set, pix)):
            comp = (k + n) % 2 if not name.endswith("w/2") and not name.endswith("h/2") and v is not None else int("h/2" in name)
            flow[b, comp, y, x] = f32(w - 1 - x) if v is None else v
            planted.append(("flow:%s:%s" % (name, "xy"[comp]), label, b, y, x))
    after = set(classify(flow).ravel())
    assert before <= after, before - after
    return img, flow, filt, planted


def clamped_windows(flow, h, w, o=-1, span=4):
    """[B, h, w]: pixels whose window reaches past the frame (its taps are clamped, columns or rows replicated)."""
    from tests import fi_windows as fw
    valid, ix, iy, _, _ = fw.samples(flow, h, w)
    L, T = ix + o, iy + o
    return valid & ((L < 0) | (T < 0) | (L + span - 1 > w - 1) | (T + span - 1 > h - 1))


# ------------------------------------------------------------------ projections

def _tile_of(labels, want, taken):
    """The first tile of image 0 (raster order) that carries a label of `want` and is not taken yet."""
    for (b, ty, tx) in sorted(labels):
        if b == 0 and (ty, tx) not in taken and labels[(b, ty, tx)] & set(want) and "neg_weight" not in labels[(b, ty, tx)]:
            return ty, tx
    raise AssertionError("no free tile with a label of %s" % (want,))


def _sources_into(flow0, h, w, ty, tx):
    """Valid sources (y, x, T, L) of image `flow0` whose top-left target lies inside tile (ty, tx) and whose four cells do too."""
    valid, L, T = pt.targets(flow0[0], flow0[1], h, w)
    y0, x0 = ty * pt.TH, tx * pt.TW
    y1, x1 = min(y0 + pt.TH, h) - 1, min(x0 + pt.TW, w) - 1
    ok = valid & (T >= y0) & (T <= y1) & (L >= x0) & (L <= x1)
    ys, xs = np.nonzero(ok)
    return [(int(y), int(x), int(T[y, x]), int(L[y, x])) for y, x in zip(ys, xs)]


def _apart(cells, T, L, gap=4):
    return all(abs(T - t) >= gap or abs(L - l) >= gap for t, l in cells)


def plant_proj(kind, field, rng):
    """(flow, depth or None, planted): the planted copy of a field of proj_tiles.build_field(kind, ..., dyadic=True).
    planted: [(what, b, y, x)] with what = "<regime>:<value>" for weights, "flow:<value>:<component>" for flows.

    Depth (kind == "depth"), image 0: +inf, -inf and NaN at three valid sources each of a plain tile, a tile with two or
    more weight classes, a tile on the frame's last row or column and a wide-cell tile (there +inf sits on one of the
    converging sources); NaN at HOLE_SOURCE; 2^100, 2^120 and FLT_MAX in the block at HUGE_BLOCK; and four bands of tiny
    weights -- subnormal multiples of 2^-149, of 2^-131, multiples of 2^-104 and of 2^-84, every band within 24 bits so
    that its sums are exact, the bands separated by rows of weight zero -- over TINY_ROWS x TINY_COLS.
    Flow (both kinds): FLOW_SET at sources of two tiles on the frame's first column and first row, x and y component
    alternating; every value but -0.0 fails the reference's validity test there."""
    flow, depth = field
    flow = flow.copy()
    depth = None if depth is None else depth.copy()
    B, _, h, w = flow.shape
    planted, cells = [], []
    labels = pt.mirror(flow[:1], None if depth is None else depth[:1], "lean").labels()

    def put_weight(what, y, x, v):
        depth[0, 0, y, x] = v
        planted.append((what, 0, y, x))

    if kind == "depth":
        taken = {(2, 0), (0, 3)}                            # the tiles of the planted flows (below): their sources go invalid
        # keep clear of the tiny bands, the huge block and the hole source: their cells must stay what they are planted for
        reserved = [(t, l) for t in range(TINY_ROWS[0] - 4, TINY_ROWS[1] + 4, 2) for l in range(TINY_COLS[0] - 4, TINY_COLS[1] + 4, 2)]
        reserved += [(HUGE_BLOCK[0] + j, HUGE_BLOCK[1] + i) for j in range(0, 20, 2) for i in range(0, 20, 2)]
        reserved += [(HOLE_SOURCE[0] + j, HOLE_SOURCE[1] + i) for j in range(0, 3) for i in range(0, 3)]
        cells.extend(reserved)
        for regime, want in (("plain", ("plain",)), ("classes", ("classes_2", "classes_3", "classes_4")), ("edge", ("edge_x", "edge_y")),
                             ("wide_cell", ("wide_cell",))):
            ty, tx = _tile_of(labels, want, taken)
            taken.add((ty, tx))
            src = _sources_into(flow[0], h, w, ty, tx)
            if regime == "wide_cell":
                # the busiest cell first: one of the sources that converge on it takes the first value
                tl = [(s[2], s[3]) for s in src]
                busiest = max(set(tl), key=tl.count)
                src.sort(key=lambda s: (s[2], s[3]) != busiest)
            else:
                order = rng.permutation(len(src))
                src = [src[i] for i in order]
            if regime == "edge":
                # a source whose cells lie on the frame's last row / column (added twice there) first
                src.sort(key=lambda s: not (s[3] == w - 1 or s[2] == h - 1))
            todo = list(WEIGHT_SET)
            for (y, x, T, L) in src:
                if not todo:
                    break
                if _apart(cells, T, L) and np.isfinite(depth[0, 0, y, x]) and depth[0, 0, y, x] > 0:
                    name, v = todo.pop(0)
                    put_weight("%s:%s" % (regime, name), y, x, v)
                    cells.append((T, L))
            assert not todo, "tile (%d, %d) has no room for %s" % (ty, tx, todo)
        put_weight("hole:nan", HOLE_SOURCE[0], HOLE_SOURCE[1], np.nan)
        by, bx = HUGE_BLOCK
        for k, (name, v) in enumerate(HUGE_WEIGHTS):
            put_weight("huge:%s" % name, by + 2 + 5 * k, bx + 2 + 5 * k, v)
        flow[0, 0, by + 12, bx + 12] = 1.5                  # FLT_MAX * 1.5: the product overflows, the weight does not
        (r0, r1), (c0, c1) = TINY_ROWS, TINY_COLS
        depth[0, 0, r0:r1, c0:c1] = 0.0
        n = (r1 - r0) // 4
        for band, quantum in enumerate((2.0 ** -149, 2.0 ** -131, 2.0 ** -104, 2.0 ** -84)):
            rows = slice(r0 + band * n, r0 + (band + 1) * n - 4)          # four rows of weight zero below every band
            depth[0, 0, rows, c0:c1] = (rng.integers(1, 17, (n - 4, c1 - c0)) * quantum).astype(f32)
        planted.append(("tiny", 0, r0, c0))

    # flows: column 0 of tile (2, 0) and row 0 of tile (0, 3); rows / columns four apart
    for k, (name, v) in enumerate(FLOW_SET):
        for comp, (y, x) in ((0, (2 * pt.TH + 1 + (k % 4) * 4, 0 if k >= 6 else 2 + k)), (1, (0 if k >= 6 else 1 + k, 3 * pt.TW + 3 + 4 * k))):
            for b in range(B):
                flow[b, comp, y, x] = v
            planted.append(("flow:%s:%s" % (name, "xy"[comp]), 0, y, x))
    return flow, depth, planted


def proj_regions(planted, flow, h, w):
    """{what: [h, w] boolean mask of the (up to four) target cells of the planted weight `what`}, image 0; sources the flow
    sends out of the frame have none."""
    valid, L, T = pt.targets(flow[0, 0], flow[0, 1], h, w)
    out = {}
    for what, b, y, x in planted:
        if what.startswith("flow") or what == "tiny" or b != 0 or not valid[y, x]:
            continue
        m = np.zeros((h, w), bool)
        for ty in (T[y, x], min(T[y, x] + 1, h - 1)):
            for tx in (L[y, x], min(L[y, x] + 1, w - 1)):
                m[ty, tx] = True
        out[what] = m
    return out


def clean_field(kind, rng, B=1, h=40, w=132):
    """A small dyadic field (flows in eighths, weights in sixteenths) with nothing planted: the call after a poisoned one.
    (w is a multiple of four: dense rows are 16-byte aligned, as the 16-byte-lane kernels need.)"""
    flow = (rng.integers(-16, 17, (B, 2, h, w)) / 8).astype(f32)
    depth = (rng.integers(2, 17, (B, 1, h, w)) / 16).astype(f32) if kind == "depth" else None
    return flow, depth


def small_proj_inputs(rng, B=1, H=20, W=40):
    """(flow, depth): the planted sets on a frame small enough for the reference's own kernels run on the CPU
    (tests/reference_cases.py: x_flowproj_planted, x_depthproj_planted).  Dyadic like the large fields; a block of sources
    that leave the frame (holes) with a NaN weight at its right edge; +inf, -inf, 2^100 and FLT_MAX apart from each other;
    subnormal weights over rows H - 4 .. H - 1 of the first eight columns; FLOW_SET on column 0 and on row 0 -- every
    planted flow but -0.0 fails the reference's validity test, which comes before its (int) conversion."""
    flow = (rng.integers(-8, 9, (B, 2, H, W)) / 8).astype(f32)
    depth = (rng.integers(2, 17, (B, 1, H, W)) / 16).astype(f32)
    flow[:, 0, 4:10, 4:12] = 1000.0
    flow[:, :, 4:10, 12] = 0.0
    depth[0, 0, 6, 12] = np.nan
    depth[0, 0, 12, 20], depth[0, 0, 15, 30], depth[0, 0, 3, 30], depth[0, 0, 12, 35] = np.inf, -np.inf, 2.0 ** 100, FLT_MAX
    flow[0, :, 12, 35] = (1.5, 0.5)
    depth[0, 0, H - 4:, :8] = (rng.integers(1, 17, (4, 8)) * 2.0 ** -149).astype(f32)
    for k, (name, v) in enumerate(FLOW_SET):
        flow[:, 0, 1 + k, 0] = v
        flow[:, 1, 0, 14 + 3 * k] = v
    return flow, depth


def small_fi_inputs(rng, B=1, C=2, H=12, W=20, fs=4):
    """(img, flow, filt) for the reference's FilterInterpolation on the CPU (x_fi_ori_planted): FEATURE_SET in the image at
    the corners, on the borders and inside, FILTER_SET in single taps, and flows of FLOW_SET, +-w/2 and +-h/2 exactly (the
    strict |f| < w/2) and the value that makes x2 == w - 1 exactly.  Every planted flow either fails the reference's
    validity test (the pixel copies its input through) or gives an exactly representable x2 >= 0: no conversion of an
    out-of-range value to int."""
    img = rng.standard_normal((B, C, H, W)).astype(f32)
    filt = rng.standard_normal((B, fs * fs, H, W)).astype(f32)
    flow = (rng.standard_normal((B, 2, H, W)) * 1.5).astype(f32)
    spots = [(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0), (0, W // 2), (H // 2, 0), (H - 1, W // 3), (H // 3, W - 1), (H // 2, W // 2)]
    for k, (name, v) in enumerate(FEATURE_SET):
        y, x = spots[k % len(spots)]
        img[k % B, (C - 1 - k) % C, y, x] = v
    for k, (name, v) in enumerate(FILTER_SET):
        filt[k % B, (5 * k) % (fs * fs), 2 + k, 3 + k] = v
    for k, (name, v) in enumerate(FLOW_SET):
        flow[:, 0, 1 + k, 0] = v
        flow[:, 1, 0, 2 + 2 * k] = v
    y = H // 2
    flow[:, 0, y, 4], flow[:, 0, y, 5] = W / 2.0, -W / 2.0
    flow[:, 1, y, 6], flow[:, 1, y, 7] = H / 2.0, -H / 2.0
    flow[:, :, y + 1, W - 4] = (3.0, 0.0)                   # x2 == w - 1 exactly: the window's right taps are clamped
    return img, flow, filt


def small_interp_inputs(rng, B=1, C=2, H=12, W=20):
    """(img, flow) for the reference's Interpolation on the CPU (x_interp_planted): FEATURE_SET in the image, the flows of
    FLOW_SET that are NaN, infinite or +-3e38 (they fail its validity test) and zero flows beside the planted features."""
    img, flow, _ = small_fi_inputs(rng, B, C, H, W)
    flow = np.clip(flow, -3, 3)
    flow[np.isnan(flow)] = 0
    for b, c, y, x in np.argwhere(~np.isfinite(img)):
        flow[b, :, y, max(x - 1, 0):x + 1] = 0              # the pixel reads the value itself, its left neighbour with weight 0
    for k, (name, v) in enumerate(FLOW_SET[:6]):
        flow[:, 0, 1 + k, 0] = v
        flow[:, 1, 0, 2 + 2 * k] = v
    return img, flow


UP4_QUARTER = (40, 96)
UP4_MULS = (4.0, 1.0)


def up4_inputs(kind, rng):
    """(quarter-resolution flow, full-resolution depth or None): halves at quarter resolution, so that the x4 bilinear
    upsample (weights in eighths per axis) times 4 gives multiples of 1/32 -- exact sums; NaN, +inf and -inf planted in
    the quarter flow (each poisons the 8 x 8 full-resolution pixels whose taps read it: invalid sources), and with depth
    +inf, -inf and NaN weights at full-resolution sources far from those."""
    hq, wq = UP4_QUARTER
    fq = (rng.integers(-2, 3, (1, 2, hq, wq)) / 2).astype(f32)
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        fq[0, k % 2, 6 + 9 * k, 10 + 25 * k] = v
    fq[0, :, 0, 0] = (np.inf, np.nan)                       # the corner: replicated taps
    depth = None
    if kind == "depth":
        depth = (rng.integers(2, 17, (1, 1, 4 * hq, 4 * wq)) / 16).astype(f32)
        for k, (name, v) in enumerate(WEIGHT_SET):
            depth[0, 0, 100 + 13 * k, 60 + 90 * k] = v
        depth[0, 0, 140, 200] = 2.0 ** 100
    return fq, depth


# ------------------------------------------------------------------ PWC-Net warp

WARP_SHAPES = ((2, 9, 9, 13), (1, 196, 18, 31))


def warp_inputs(shape, align_corners):
    """(features, flow): FEATURE_SET planted over normal features, one value per pixel, channels taking turns (the last
    channel first); the flows of test_pwc_warp_bit_exact's kind (smooth, fractional, finite) except: zero -- an integer --
    at the pixel left of every non-finite feature (its east corner reads the value with weight exactly 0), half a pixel
    outwards at the non-finite features planted on the right border (that pixel is masked out: value * mask 0), and a
    block that points far out of the map."""
    B, C, H, W = shape
    rng = np.random.default_rng([20261020, C, int(align_corners)])
    x = rng.standard_normal(shape).astype(f32)
    flo = (rng.standard_normal((B, 2, H, W)) * 0.7).astype(f32)
    flo[:, :, :2, 5:8] = f32(-40.0)
    sites = [(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0), (H // 2, W - 1), (H // 2, W // 2), (H // 3, W // 4), (2 * H // 3, 3 * W // 4),
             (H // 4, 2 * W // 3)]
    planted = []
    for k, (name, v) in enumerate(FEATURE_SET):
        b, c = k % B, (C - 1 - k) % C
        y, xx = sites[k % len(sites)]
        x[b, c, y, xx] = v
        planted.append((name, b, c, y, xx))
        if not np.isfinite(v):
            # the pixel itself: a quarter pixel towards the inside (it reads the value with weight 9/16) ...
            flo[b, :, y, xx] = (0.25, 0.25 if y < H - 1 else -0.25)
            if xx >= 1:
                flo[b, :, y, xx - 1] = 0
            if xx == W - 1:                                 # ... or, on the right border, half a pixel out of the map
                flo[b, :, y, xx] = (0.5, 0)
    return x, flo, planted


# ------------------------------------------------------------------ MinDepthFlowProjection

MINDEPTH_SHAPES = ((1, 20, 30), (1, 33, 70))


def mindepth_inputs(shape, rng):
    """(flow, weight, count0): integer flows that send several sources to one cell, an incoming count that is negative
    over the left half (so that a NEGATIVE weight can win: the ~u branch of md_order_bits and its inverse), +inf and
    -inf weights, weights equal to the incoming count (the comparison is strict: they lose), and +0.0 / -0.0 against
    each other in both roles."""
    B, H, W = shape
    # (no zero flow: a filled hole's value would be a zero whose sign depends on the order the holes are visited in)
    flow = rng.choice(np.array([-2, -1, 1, 2], f32), (B, 2, H, W))
    wgt =(rng.integers(-12, 13, (B, 1, H, W)) / 8).astype(f32)
    count0 = (rng.integers(0, 5, (B, 1, H, W)) / 8).astype(f32)
    count0[..., : W // 2] = (rng.integers(-16, -7, (B, 1, H, W // 2)) / 8).astype(f32)
    # left half: every weight negative, some above the floor, some below, some equal to it
    wgt[..., : W // 2] = -np.abs(wgt[..., : W // 2]) - f32(0.125)
    valid, L, T = pt.targets(flow[0, 0], flow[0, 1], H, W)
    ys, xs = np.nonzero(valid)
    pick = rng.permutation(len(ys))
    k = 0
    for name, v in (("+inf", np.inf), ("-inf", -np.inf), ("+inf", np.inf), ("-inf", -np.inf)):
        y, x = ys[pick[k]], xs[pick[k]]
        wgt[0, 0, y, x] = v
        k += 1
    for _ in range(12):                                     # weight == incoming count at its own target
        y, x = ys[pick[k]], xs[pick[k]]
        wgt[0, 0, y, x] = count0[0, 0, T[y, x], L[y, x]]
        k += 1
    for sign_w, sign_c in ((0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (-0.0, -0.0)):
        for _ in range(3):
            y, x = ys[pick[k]], xs[pick[k]]
            wgt[0, 0, y, x] = sign_w
            count0[0, 0, T[y, x], L[y, x]] = sign_c
            k += 1
    count0[0, 0, 0, 0] = -np.inf                            # any weight beats it
    count0[0, 0, H - 1, W - 1] = np.inf                     # none does
    return flow, wgt, count0


# ------------------------------------------------------------------ FilterInterpolation: the cases both test files run

FI_SEED = 20261020
# another draw where the first one misses a cap of tests/test_forward_edges_host.py (a class without a NaN output)
FI_SALT = {("defor", 9, 4): 1, ("defor", 3, 6): 2}


def fi_case(kernel, C, aligned=True, fs=4, which=0):
    """The planted inputs of one FilterInterpolation test: a field of fi_windows.build_field for `kernel` (B = 2, the frame
    of fi_windows.field_shape), image values from rng.random (float16 for "f16", with taps below 1/4 as in
    test_gpu_fi_windows.py), planted by plant_fi; which: another draw of the same case (the blend's other direction).  A dict: img, flow, filt, flow2 / off where the kernel has them (not
    planted), classify, labels (after planting), pix (the labels per pixel), h, w, fs."""
    from tests import fi_windows as fw
    h, w = fw.field_shape(kernel, aligned)
    rng = np.random.default_rng([FI_SEED, sum(map(ord, kernel)), C, int(aligned), fs, FI_SALT.get((kernel, C, fs), 0)] + ([which] if which else []))
    f = fw.build_field(kernel, rng, 2, h, w, aligned, fs=fs)
    img = rng.random((2, C, h, w), dtype=f32)
    filt = rng.random((2, fs * fs, h, w), dtype=f32)
    if kernel == "f16":
        img, filt = img.astype(np.float16), (filt * f32(0.25)).astype(f32)
    if kernel in ("lds", "n"):
        classify = lambda fl: fw.classes(kernel, fl, h, w, aligned, fs=fs)                     # noqa: E731
    elif kernel == "multi":
        classify = lambda fl: fw.classes(kernel, fl, h, w, flow2=f["flow2"])                   # noqa: E731
    elif kernel == "defor":
        classify = lambda fl: fw.classes(kernel, fl, h, w, fs=fs, off=f["off"])                # noqa: E731
    else:
        classify = lambda fl: fw.classes(kernel, fl, h, w)                                     # noqa: E731
    img, flow, filt, planted = plant_fi(kernel, f, img, filt, rng, classify, fs)
    labels = classify(flow)
    case = dict(img=img, flow=flow, filt=filt, planted=planted, classify=classify, labels=labels, h=h, w=w, fs=fs,
                pix=fw.pixel_labels(kernel, labels, h, w, fs), all_classes=set(fw.all_classes(kernel, aligned)))
    for k in ("flow2", "off"):
        if k in f:
            case[k] = f[k]
    return case


def class_caps(ref, pix):
    """Per class of `pix`: (has a NaN output, has an infinite output, share of finite outputs) of the oracle result."""
    out = {}
    for label in sorted(set(pix.ravel())):
        r = ref[np.broadcast_to((pix == label)[:, None], ref.shape)]
        out[label] = (bool(np.isnan(r).any()), bool(np.isinf(r).any()), float(np.isfinite(r).mean()))
    return out


def differing_by_class(got, want, pix):
    """{label: pixels that differ in any channel} under same_bits_nan_aware's rule; empty when the results agree."""
    bits = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    ng, nw = np.isnan(got), np.isnan(want)
    bad = (ng != nw) | (~ng & ~nw & (np.ascontiguousarray(got).view(bits) != np.ascontiguousarray(want).view(bits)))
    bad_px = bad.any(1)
    return {label: int((bad_px & (pix == label)).sum()) for label in sorted(set(pix.ravel())) if (bad_px & (pix == label)).any()}
