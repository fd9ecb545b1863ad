"""Host mirror of the per-tile decisions of the LDS-staged backward kernels, an exact restatement of their image gradient,
and field builders that send every decision through at least one tile.

Each staged backward kernel takes the bounding box of its tile's taps, picks from it how many channels a pass sums (pc),
adds the image-gradient addends as 64-bit integers in LDS cells, and raises a per-tile flag when the box does not fit, so
that a per-tap kernel (launched with a different block shape) redoes the tile.  Kernels (instances):

  "ori"        fi_backward_ori4_lds (filterinterp.hip), 64x8 tiles
  "blend"      fi_blend_backward4_lds<true>: the same body, one channel per pass, z = direction * B + b
  "blend_nox"  fi_blend_backward4_lds<false>: no image gradient, channels per pass from the window slots only
  "defor"      fi_backward_defor_lds<0/1/2> (filterinterp_defor_bwd_lds.hip), 64x4 tiles, two boxes
  "interp"     interp_backward_lds (warp_sepconv.hip), 64x8 tiles
  "warp"       pwc_warp_backward_tile (pwc_warp_backward.hip), 64x8 tiles x channel groups

  tiles(kernel, flow, ...)        -> per (z, tile row, tile column) a record: boxes, channels per pass, labels
  predict_image_grad(kernel, ...) -> the image gradient bit for bit: the exact integer sums of rint(fp32 addend x 2^k)
                                     per cell, converted once as gradacc_convert does (gradacc.h "Deterministic image
                                     gradients"); the staged and the per-tap paths add the same integers, so one
                                     restatement holds for every class
  build_field(kernel, rng, B, h, w) -> inputs in which every reachable label owns a tile in every batch item (and direction)

Every constant is read from the kernels' #defines, so an edited constant moves the mirror with it.

Unreachable labels (stated, not silently absent):
  * "short_pass" of "blend" (and "pc1" short passes anywhere): one channel per pass leaves no shorter last pass.
  * "pc3" / "pc2" of "blend": the instance holds one channel per pass (CH = 1).
"""
import functools
import math
import re

import numpy as np

from oracle.np_oracle import _fi_geometry
from tests.fi_windows import _eval, source

f32 = np.float32

SOURCES = {"ori": "filterinterp.hip", "blend": "filterinterp.hip", "blend_nox": "filterinterp.hip",
           "defor": "filterinterp_defor_bwd_lds.hip", "interp": "warp_sepconv.hip", "warp": "pwc_warp_backward.hip"}
KERNELS = tuple(SOURCES)
CU_COUNT = 256                      # MI355X compute units (the warp launcher sizes its channel groups by them)


@functools.lru_cache(maxsize=None)
def constants(name):
    """The object-like integer #defines of a translation unit, each evaluated in terms of the ones before it."""
    env = {}
    for k, v in re.findall(r"^\s*#define\s+(\w+)[ \t]+([^\n]+)$", source(name), flags=re.M):
        try:
            env[k] = _eval(v, env)
        except (ValueError, SyntaxError, NameError, TypeError):
            pass
    return env


def _c(name, src):
    return constants(src)[name]


FB_TW, FB_TH = _c("FB_TW", "filterinterp.hip"), _c("FB_TH", "filterinterp.hip")
FB_THREADS, FB_CH, FB_CELLS = _c("FB_THREADS", "filterinterp.hip"), _c("FB_CH", "filterinterp.hip"), _c("FB_CELLS", "filterinterp.hip")
IB_TW, IB_TH, IB_CH, IB_CELLS = (_c(n, "warp_sepconv.hip") for n in ("IB_TW", "IB_TH", "IB_CH", "IB_CELLS"))
DB_TW, DB_TH, DB_CH = (_c(n, "filterinterp_defor_bwd_lds.hip") for n in ("DB_TW", "DB_TH", "DB_CH"))
DB_WIN_FLOATS, DB_CELLS = (_c(n, "filterinterp_defor_bwd_lds.hip") for n in ("DB_WIN_FLOATS", "DB_CELLS"))
PB_TW, PB_TH, PB_CH, PB_CELLS = (_c(n, "pwc_warp_backward.hip") for n in ("PB_TW", "PB_TH", "PB_CH", "PB_CELLS"))
FAR = 1e9                           # defor: |tap position| >= FAR (or not finite) flags the block

TILE = {"ori": (FB_TW, FB_TH), "blend": (FB_TW, FB_TH), "blend_nox": (FB_TW, FB_TH), "defor": (DB_TW, DB_TH),
        "interp": (IB_TW, IB_TH), "warp": (PB_TW, PB_TH)}
EDGE_LABELS = ("edge_left", "edge_right", "edge_top", "edge_bottom", "ragged_right", "ragged_bottom")


# ------------------------------------------------------------------ per-tile decisions (as written in the sources)

def ori_channels(n, ch):
    """fi_backward_ori4_tile: slot_floats = (n + FB_THREADS - 1) & ~(FB_THREADS - 1), pc = min(CH, FB_CELLS / slot_floats)"""
    slot = (n + FB_THREADS - 1) & ~(FB_THREADS - 1)
    return min(ch, FB_CELLS // slot)


def blend_ch(want_x):
    """CH = (BLEND && WANT_X) ? 1 : FB_CH"""
    return 1 if want_x else FB_CH


def interp_channels(n):
    return min(IB_CH, IB_CELLS // n)


def defor_channels(ncell):
    return min(DB_CH, DB_CELLS // max(ncell, 1))


def defor_window(bw, bh):
    """(pitch, pitch * bh): the window fits iff the second is at most DB_WIN_FLOATS"""
    pitch = (bw + 31) & ~31
    return pitch, pitch * bh


def warp_step(n):
    """None: the tile adds per corner (n > PB_CELLS); else the channels per pass"""
    return None if n > PB_CELLS else min(PB_CH, PB_CELLS // n)


def warp_groups(B, C, h, w, cu=CU_COUNT):
    """(cgroup, groups) as vfi_pwc_warp_backward computes them"""
    ntiles = -(-w // PB_TW) * -(-h // PB_TH) * B
    c8 = -(-C // PB_CH)
    groups = min(c8, max(1, -(-cu // ntiles)))
    groups = min(groups, 65535 // B)
    cgroup = PB_CH * (-(-c8 // groups))
    return cgroup, -(-C // cgroup)


def pass_label(pc, prefix="pc"):
    return "%s%d" % (prefix, pc)


def all_labels(kernel):
    """The labels a field of `kernel` must cover (reachable ones only; see the module docstring)."""
    if kernel == "blend":
        core = ("empty", "pc1", "flag_window")
    elif kernel == "defor":
        core = ("empty", "pc3", "pc2", "pc1", "short_pass", "flag_window", "flag_cells", "flag_position")
    elif kernel == "warp":
        core = ("empty", "step8", "step_mid", "step1", "short_pass", "flag_window")
    else:
        core = ("empty", "pc3", "pc2", "pc1", "short_pass", "flag_window")
    return core + EDGE_LABELS


def _edge_labels(box, h, w, ty, tx, th, tw):
    x0, y0, x1, y1 = box
    out = set()
    if x0 == 0:
        out.add("edge_left")
    if x1 == w - 1:
        out.add("edge_right")
    if y0 == 0:
        out.add("edge_top")
    if y1 == h - 1:
        out.add("edge_bottom")
    if (tx + 1) * tw > w:
        out.add("ragged_right")
    if (ty + 1) * th > h and (th != 8 or h % 8 <= 4):
        out.add("ragged_bottom")
    return out


def _boxes(mask, x0s, y0s, x1s, y1s, th, tw):
    """per tile of [h, w] the box (min x0, min y0, max x1, max y1) over the masked pixels, or None"""
    h, w = mask.shape
    out = {}
    for ty in range(-(-h // th)):
        for tx in range(-(-w // tw)):
            sl = (slice(ty * th, (ty + 1) * th), slice(tx * tw, (tx + 1) * tw))
            m = mask[sl]
            out[ty, tx] = None if not m.any() else (int(x0s[sl][m].min()), int(y0s[sl][m].min()),
                                                   int(x1s[sl][m].max()), int(y1s[sl][m].max()))
    return out


def _short(channel, pc, groups=None):
    """a pass with fewer channels than pc: channel % pc != 0 (per channel group for the warp kernel)"""
    if groups is None:
        return channel % pc != 0
    cgroup, ng = groups
    return any(min(cgroup, channel - g * cgroup) % pc != 0 for g in range(ng))


def tiles(kernel, flow, channel, off=None, align_corners=True, finite_call=True, scale2_one=True):
    """Per (z, ty, tx) {'box', 'pc', 'labels', ...} for one direction's flow [B, 2, h, w] (defor: with off [B, 32, h, w]).
    finite_call / scale2_one: the call-level state (gradacc_staged_ok); when it fails every non-empty tile is flagged."""
    B, _, h, w = flow.shape
    tw, th = TILE[kernel]
    out = {}
    staged_ok = finite_call and scale2_one
    if kernel in ("ori", "blend", "blend_nox", "defor"):
        valid, x2, y2, ix, iy, alpha, beta, L, T = _fi_geometry(flow.astype(f32), h, w, 4)
    for b in range(B):
        if kernel in ("ori", "blend", "blend_nox"):
            co0, co3 = np.clip(L[b], 0, w - 1), np.clip(L[b] + 3, 0, w - 1)
            ro0, ro3 = np.clip(T[b], 0, h - 1), np.clip(T[b] + 3, 0, h - 1)
            boxes = _boxes(valid[b], co0, ro0, co3, ro3, th, tw)
            ch = FB_CH if kernel == "ori" else blend_ch(kernel == "blend")
            for key, box in boxes.items():
                rec = {"box": box}
                if box is None:
                    rec["labels"] = {"empty"}
                else:
                    n = (box[2] - box[0] + 1) * (box[3] - box[1] + 1)
                    pc = ori_channels(n, ch)
                    rec["n"], rec["pc"] = n, pc
                    gate = staged_ok or kernel == "blend_nox"
                    if pc == 0 or not gate:
                        rec["labels"] = {"flag_window" if pc == 0 else "flag_call"}
                    else:
                        rec["labels"] = {pass_label(pc)} | ({"short_pass"} if _short(channel, pc) else set())
                    rec["labels"] |= _edge_labels(box, h, w, key[0], key[1], th, tw)
                out[(b,) + key] = rec
        elif kernel == "interp":
            fx, fy = flow[b, 0].astype(f32), flow[b, 1].astype(f32)
            xs, ys = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
            X2, Y2 = xs + fx, ys + fy
            with np.errstate(invalid="ignore"):
                v = (X2 >= 0) & (Y2 >= 0) & (X2 < f32(w)) & (Y2 < f32(h))
            Lb = np.where(v, np.trunc(np.where(v, X2, 0)), 0).astype(np.int64)
            Tb = np.where(v, np.trunc(np.where(v, Y2, 0)), 0).astype(np.int64)
            boxes = _boxes(v, Lb, Tb, np.minimum(Lb + 1, w - 1), np.minimum(Tb + 1, h - 1), th, tw)
            for key, box in boxes.items():
                rec = {"box": box}
                if box is None:
                    rec["labels"] = {"empty"}
                else:
                    n = (box[2] - box[0] + 1) * (box[3] - box[1] + 1)
                    pc = interp_channels(n)
                    rec["n"], rec["pc"] = n, pc
                    if pc == 0 or not staged_ok:
                        rec["labels"] = {"flag_window" if pc == 0 else "flag_call"}
                    else:
                        rec["labels"] = {pass_label(pc)} | ({"short_pass"} if _short(channel, pc) else set())
                    rec["labels"] |= _edge_labels(box, h, w, key[0], key[1], th, tw)
                out[(b,) + key] = rec
        elif kernel == "defor":
            vb = valid[b]
            co = [np.clip(L[b] + k, 0, w - 1) for k in range(4)]
            ro = [np.clip(T[b] + k, 0, h - 1) for k in range(4)]
            tcx_lo = np.full((h, w), np.iinfo(np.int64).max)
            tcy_lo = tcx_lo.copy()
            tcx_hi = np.full((h, w), np.iinfo(np.int64).min)
            tcy_hi = tcx_hi.copy()
            finite = np.ones((h, w), bool)
            for k in range(16):
                fracY = ro[k // 4].astype(f32) + off[b, k].astype(f32)
                fracX = co[k % 4].astype(f32) + off[b, 16 + k].astype(f32)
                with np.errstate(invalid="ignore"):
                    ok = (np.abs(fracY) < f32(FAR)) & (np.abs(fracX) < f32(FAR))
                finite &= ok
                top = np.clip(np.trunc(np.where(ok, fracY, 0)), -1, h - 1).astype(np.int64)
                left = np.clip(np.trunc(np.where(ok, fracX, 0)), -1, w - 1).astype(np.int64)
                tcx_lo, tcy_lo = np.minimum(tcx_lo, left), np.minimum(tcy_lo, top)
                tcx_hi, tcy_hi = np.maximum(tcx_hi, left + 1), np.maximum(tcy_hi, top + 1)
            wins = _boxes(vb, tcx_lo, tcy_lo, tcx_hi, tcy_hi, th, tw)
            cells = _boxes(vb, co[0], ro[0], co[3], ro[3], th, tw)
            bad = _boxes(vb & ~finite, co[0], ro[0], co[0], ro[0], th, tw)
            for key, cbox in cells.items():
                rec = {"box": cbox}
                if cbox is None:
                    rec["labels"] = {"empty"}
                else:
                    wbox = wins[key]
                    ncell = (cbox[2] - cbox[0] + 1) * (cbox[3] - cbox[1] + 1)
                    pc = defor_channels(ncell)
                    rec["ncell"], rec["pc"], rec["window"] = ncell, pc, wbox
                    if bad[key] is not None:
                        lab = "flag_position"
                    else:
                        _, nwin = defor_window(wbox[2] - wbox[0] + 1, wbox[3] - wbox[1] + 1)
                        rec["nwin"] = nwin
                        lab = "flag_window" if nwin > DB_WIN_FLOATS else "flag_cells" if pc == 0 else None
                    if not staged_ok and lab is None:
                        lab = "flag_call"
                    if lab is not None:
                        rec["labels"] = {lab}
                    else:
                        rec["labels"] = {pass_label(pc)} | ({"short_pass"} if _short(channel, pc) else set())
                    rec["labels"] |= _edge_labels(cbox, h, w, key[0], key[1], th, tw)
                out[(b,) + key] = rec
        elif kernel == "warp":
            from tests.pwc_warp_backward import geometry
            ix, iy, fx0, fy0, inb, corners, mask = geometry(flow[b:b + 1], h, w, align_corners)
            (y0, x0) = corners[0]
            scat = mask[0] != 0
            cx0, cx1 = np.clip(x0[0], 0, w - 1), np.clip(x0[0] + 1, 0, w - 1)
            cy0, cy1 = np.clip(y0[0], 0, h - 1), np.clip(y0[0] + 1, 0, h - 1)
            boxes = _boxes(scat, cx0, cy0, cx1, cy1, th, tw)
            groups = warp_groups(B, channel, h, w)
            for key, box in boxes.items():
                rec = {"box": box, "groups": groups}
                if box is None:
                    rec["labels"] = {"empty"}
                else:
                    n = (box[2] - box[0] + 1) * (box[3] - box[1] + 1)
                    step = warp_step(n)
                    rec["n"], rec["pc"] = n, step
                    if step is None or not staged_ok:
                        rec["labels"] = {"flag_window" if step is None else "flag_call"}
                    else:
                        lab = "step%d" % step if step in (1, PB_CH) else "step_mid"
                        rec["labels"] = {lab} | ({"short_pass"} if _short(channel, step, groups) else set())
                    rec["labels"] |= _edge_labels(box, h, w, key[0], key[1], th, tw)
                out[(b,) + key] = rec
        else:
            raise KeyError(kernel)
    return out


def label_counts(recs, z=None):
    """{label: tile count} over the records (of image / plane z only when given)"""
    out = {}
    for key, rec in recs.items():
        if z is not None and key[0] != z:
            continue
        for lab in rec["labels"]:
            out[lab] = out.get(lab, 0) + 1
    return out


def cell_labels(recs):
    """per (b, y, x) the set of labels of the tiles whose cell box covers the cell (to name a failing class)"""
    out = {}
    for key, rec in recs.items():
        if rec["box"] is None:
            continue
        x0, y0, x1, y1 = rec["box"]
        out.setdefault(key[0], []).append((x0, y0, x1, y1, rec["labels"], key[1:]))
    return out


def name_cells(recs, kernel, bad, h, w, limit=4):
    """a message naming the classes of the tiles that scatter into the first few mismatching cells bad = [(b, c, y, x)]"""
    idx = cell_labels(recs)
    lines, classes = [], set()
    for b, c, y, x in bad:
        labs = [(sorted(l), t) for x0, y0, x1, y1, l, t in idx.get(b, []) if x0 <= x <= x1 and y0 <= y <= y1]
        for l, _ in labs:
            classes.update(l)
        if len(lines) < limit:
            lines.append("cell b%d c%d (%d, %d): tiles %s" % (b, c, y, x, labs[:3]))
    return "%d cells differ; classes of the tiles reaching them: %s\n  %s" % (len(bad), sorted(classes), "\n  ".join(lines))


# ------------------------------------------------------------------ the scale (gradacc_scan / gradacc_ctx)

def _frexp_exp(v):
    return math.frexp(float(v))[1] if v != 0 else 0


def cells_log2(h, w, taps):
    """hdr[3]: the smallest L with 2^L >= h w max(taps, 4)"""
    n, L = h * w * max(taps, 4), 0
    while (1 << L) < n:
        L += 1
    return L


def grad_scale(gout, weights, h, w, taps):
    """(k, fp32 path, scale, scale2) of a call: gradacc_magnitude / gradacc_exponent / gradacc_fp32 / gradacc_ctx.
    The maxima skip non-finite elements (which raise hdr[1])."""
    a = np.abs(np.asarray(gout, f32))
    fin = np.isfinite(a)
    nonfinite = not fin.all()
    eg = _frexp_exp(a[fin].max() if fin.any() else 0.0)
    ew = 1
    if weights is not None:
        aw = np.abs(np.asarray(weights, f32))
        finw = np.isfinite(aw)
        nonfinite = nonfinite or not finw.all()
        mw = aw[finw].max() if finw.any() else 0.0
        if mw != 0:
            ew = _frexp_exp(mw)
    mag = eg + max(ew, 1)
    k = 62 - cells_log2(h, w, taps) - mag
    k1 = max(-126, min(126, k))
    scale, scale2 = 2.0 ** k1, 2.0 ** max(-126, min(126, k - k1))
    return k, nonfinite or mag > 128, f32(scale), f32(scale2)


# ------------------------------------------------------------------ the restatement

def _round(v, scale, scale2):
    """__float2ll_rn(v * scale [* scale2]) in fp32: round half to even to int64"""
    s = v.astype(f32) * scale
    if scale2 != 1:
        s = s * scale2
    return np.rint(s.astype(np.float64)).astype(np.int64)


def _scatter(sums, b, c, cy, cx, vals, m, w):
    np.add.at(sums[b, c], (cy[m] * w + cx[m]), vals[m])


def convert(sums, k, g0=None, overwrite=False):
    """gradacc_convert: (float)ldexp((double)sum, -k); added into g0 where sum != 0, or written (0 where sum == 0)"""
    v = np.ldexp(sums.astype(np.float64), -k).astype(f32)
    if overwrite:
        return np.where(sums != 0, v, f32(0))
    return np.where(sums != 0, (g0.astype(f32) + v).astype(f32), g0.astype(f32))


def integer_sums(kernel, flow, gout, k_scale, filt=None, off=None, variant=1, align_corners=True):
    """[B, C, h*w] int64 sums of the rounded addends of every cell (kernel != 'blend_nox'), each addend formed in fp32 in the
    kernel's operation order; k_scale = (scale, scale2) of grad_scale."""
    B, C, h, w = gout.shape
    scale, scale2 = k_scale
    sums = np.zeros((B, C, h * w), np.int64)
    one = f32(1)
    gout = gout.astype(f32)
    if kernel in ("ori", "blend", "defor"):
        valid, x2, y2, ix, iy, alpha, beta, L, T = _fi_geometry(flow.astype(f32), h, w, 4)
        for b in range(B):
            m = valid[b]
            for c in range(C):
                g = gout[b, c]
                qg = ((g * (one - alpha[b])) * (one - beta[b]), (g * alpha[b]) * (one - beta[b]),
                      (g * (one - alpha[b])) * beta[b], (g * alpha[b]) * beta[b])
                for dj in range(4):
                    cy = np.clip(T[b] + dj, 0, h - 1).astype(np.int64)
                    for di in range(4):
                        kk = dj * 4 + di
                        cx = np.clip(L[b] + di, 0, w - 1).astype(np.int64)
                        if kernel != "defor" or variant == 0:
                            quad = np.full((h, w), (dj >= 2) * 2 + (di >= 2))
                        else:
                            fracY = cy.astype(f32) + off[b, kk].astype(f32)
                            fracX = cx.astype(f32) + off[b, 16 + kk].astype(f32)
                            quad = (fracX > x2[b]).astype(int) | ((fracY > y2[b]).astype(int) << 1)
                        q = np.choose(quad, qg).astype(f32)
                        v = q if kernel == "defor" and variant == 2 else q * filt[b, kk].astype(f32)
                        _scatter(sums, b, c, cy, cx, _round(v, scale, scale2), m, w)
    elif kernel == "interp":
        xs, ys = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
        for b in range(B):
            X2, Y2 = xs + flow[b, 0].astype(f32), ys + flow[b, 1].astype(f32)
            with np.errstate(invalid="ignore"):
                m = (X2 >= 0) & (Y2 >= 0) & (X2 < f32(w)) & (Y2 < f32(h))
            X2, Y2 = np.where(m, X2, f32(0)), np.where(m, Y2, f32(0))
            Lb, Tb = np.trunc(X2).astype(np.int64), np.trunc(Y2).astype(np.int64)
            R, Bm = np.minimum(Lb + 1, w - 1), np.minimum(Tb + 1, h - 1)
            a, be = X2 - Lb.astype(f32), Y2 - Tb.astype(f32)
            for c in range(C):
                g = gout[b, c]
                for cy, cx, v in ((Tb, Lb, (g * (one - a)) * (one - be)), (Tb, R, (g * a) * (one - be)),
                                  (Bm, Lb, (g * (one - a)) * be), (Bm, R, (g * a) * be)):
                    _scatter(sums, b, c, cy, cx, _round(v, scale, scale2), m, w)
    elif kernel == "warp":
        from tests.pwc_warp_backward import geometry
        ix, iy, fx0, fy0, inb, corners, mask = geometry(flow, h, w, align_corners)
        wts = ((fx0 + one - ix) * (fy0 + one - iy), (ix - fx0) * (fy0 + one - iy),
               (fx0 + one - ix) * (iy - fy0), (ix - fx0) * (iy - fy0))
        for b in range(B):
            scat = mask[b] != 0
            for c in range(C):
                gm = gout[b, c] * mask[b]
                for kq in range(4):
                    cy, cx = corners[kq]
                    m = scat & inb[kq][b]
                    e = np.where(inb[kq][b], wts[kq][b], f32(0)).astype(f32)
                    _scatter(sums, b, c, np.clip(cy[b], 0, h - 1), np.clip(cx[b], 0, w - 1),
                             _round(e * gm, scale, scale2), m, w)
    else:
        raise KeyError(kernel)
    return sums.reshape(B, C, h, w)


def taps_of(kernel):
    return 16 if kernel in ("ori", "blend", "blend_nox", "defor") else 4


def predict_image_grad(kernel, flow, gout, g0=None, filt=None, off=None, variant=1, align_corners=True):
    """The image gradient bit for bit (g0: the starting value the kernels add into; the blend overwrites).
    Returns (grad, k, fp32_path); grad is None on the fp32 path (not restated: the atomic order is free)."""
    B, C, h, w = gout.shape
    weights = filt if kernel in ("ori", "blend") or (kernel == "defor" and variant != 2) else None
    k, fp32, scale, scale2 = grad_scale(gout, weights, h, w, taps_of(kernel))
    if fp32:
        return None, k, True
    sums = integer_sums(kernel, flow, gout, (scale, scale2), filt, off, variant, align_corners)
    return convert(sums, k, g0, overwrite=kernel == "blend"), k, False


def blend_grad(gb, go, wgt):
    """g = gb * w + go, the product and the sum rounded separately (GradTerms)"""
    if gb is None:
        return go.astype(f32)
    v = gb.astype(f32) * f32(wgt)
    return v if go is None else (v + go.astype(f32)).astype(f32)


# ------------------------------------------------------------------ field builders

def _recipes(kernel):
    """(label, recipe) pairs placed one per tile; recipe = (kind, parameter)"""
    if kernel in ("ori", "blend", "blend_nox"):     # (one blend field serves both instances: pc3 / pc2 / pc1 boxes are pc1 with CH = 1)
        return [("empty", ("empty", 0)), ("pc3", ("shear", 12)), ("pc2", ("shear", 30)), ("pc1", ("shear", 60)),
                ("flag_window", ("shear", 100)), ("partial", ("partial", 0))]
    if kernel == "interp":
        return [("empty", ("empty", 0)), ("pc3", ("shear", 12)), ("pc2", ("shear", 32)), ("pc1", ("shear", 66)),
                ("flag_window", ("shear", 110)), ("partial", ("partial", 0))]
    if kernel == "warp":
        return [("empty", ("empty", 0)), ("step8", ("shear", 2)), ("step_mid", ("shear", 20)), ("step1", ("shear", 66)),
                ("flag_window", ("shear", 110)), ("partial", ("partial", 0))]
    if kernel == "defor":
        return [("empty", ("empty", 0)), ("pc3", ("shear", 8)), ("pc2", ("squeeze", (14, 100))),
                ("pc1", ("squeeze", (26, 100))), ("flag_window", ("shear", 44)), ("flag_cells", ("collapse", 64)),
                ("flag_position", ("far", 0)), ("partial", ("partial", 0))]
    raise KeyError(kernel)


def build_field(kernel, rng, B, h=123, w=360, dirs=1):
    """flow [B, 2, h, w] (a list of dirs of them for dirs > 1) and, for "defor", offsets [B, 32, h, w] (likewise).

    Every tile starts from a small sub-pixel flow (and, for defor, small offsets); one tile per recipe of _recipes(kernel)
    then gets its recipe.  The recipe tiles sit on the interior tile rows, shifted by one tile column per batch item and
    per direction so that an item's or a direction's tiles take different classes.  Edge labels come from the frame's
    border tiles; h % 8 <= 4 and w % 64 != 0 make the last tile row and column ragged."""
    tw, th = TILE[kernel]
    flows, offs = [], []
    recipes = _recipes(kernel)
    tx_n, ty_n = -(-w // tw), -(-h // th)
    for d in range(dirs):
        flow = rng.uniform(-0.45, 0.45, (B, 2, h, w)).astype(f32)
        flow = (np.round(flow * 16) / 16).astype(f32)
        off = (np.round(rng.uniform(-1.5, 1.5, (B, 32, h, w)) * 8) / 8).astype(f32) if kernel == "defor" else None
        for b in range(B):
            # recipes on tile rows around the frame's middle (the shear recipes need room above and below)
            slots = [(ty_n // 2 + (i % 2) * (1 if th == 8 else 2), 1 + (i // 2 + b + 2 * d) % (tx_n - 2))
                     for i in range(len(recipes))]
            for (_, (kind, p)), (ty, tx) in zip(recipes, slots):
                y0, x0 = ty * th, tx * tw
                sl = (slice(y0, min(y0 + th, h)), slice(x0, min(x0 + tw, w)))
                xs = np.arange(x0, min(x0 + tw, w), dtype=f32)[None, :] - f32(x0)
                if kind == "empty":
                    flow[b, 0][sl] = f32(10 * w)
                elif kind == "partial":
                    flow[b, 0][sl] = np.where((xs.astype(int) // 4) % 2 == 1, f32(10 * w), flow[b, 0][sl])
                elif kind == "shear":
                    fy = (xs / f32(tw - 1) - f32(0.5)) * f32(p)
                    flow[b, 1][sl] = np.round(fy * 4) / 4
                elif kind == "squeeze":          # defor: x compressed to about gw columns, y sheared by p rows
                    gw, rng_y = p
                    flow[b, 0][sl] = np.round(-xs * (1 - (gw - 4) / (tw - 1)) * 4) / 4
                    flow[b, 1][sl] = np.round((xs / f32(tw - 1) - f32(0.5)) * f32(rng_y) * 4) / 4
                    off[b][:, sl[0], sl[1]] = 0
                elif kind == "collapse":         # defor: cells spread by a y shear, every tap moved onto one point
                    flow[b, 1][sl] = np.round((xs / f32(tw - 1) - f32(0.5)) * f32(p) * 4) / 4
                    valid, _, _, _, _, _, _, L, T = _fi_geometry(flow[b:b + 1], h, w, 4)
                    yc, xc = f32(y0 + 1.5), f32(x0 + 20.5)
                    for kk in range(16):
                        ro = np.clip(T[0][sl] + kk // 4, 0, h - 1).astype(f32)
                        co = np.clip(L[0][sl] + kk % 4, 0, w - 1).astype(f32)
                        off[b, kk][sl] = yc - ro
                        off[b, 16 + kk][sl] = xc - co
                elif kind == "far":
                    off[b, 5, y0 + 1, x0 + 7] = f32(1.5e9)
        flows.append(flow)
        offs.append(off)
    if dirs == 1:
        return flows[0], offs[0]
    return flows, offs
