"""Host mirror of the per-tile window choice of the LDS-staged FilterInterpolation forward kernels, and a field builder
that sends every choice through at least one tile.

Each staged kernel measures, per workgroup, the bounding box of its tile's taps, and from it picks one of several
compiled ring geometries (a template instance per staged-elements-per-thread K), or gathers from global memory when
the window does not fit.  A wrong count, pitch or parity in one instance corrupts only the tiles that land in it, so
the GPU tests compare per class, and the classes come from this module:

  classes(kernel, flow, h, w, ...)  -> one label per (batch item, tile row, tile column)
  build_field(kernel, rng, B, h, w, ...) -> flow (flow2 for the shared-window kernel, off for the deformable one)
                                       in which every class of all_classes(...) owns at least one tile

kernels: "lds" (filterinterp_lds.hip, lean loop, fs 4), "blend" (the same kernel with the blend epilogue), "n"
(filterinterp_lds_n.hip, fs 2 / 5 / 6), "f16" (filterinterp_f16.hip; its tile, ring and ladder are filterinterp_16.h's, which
filterinterp_bf16.hip shares), "multi" (filterinterp_multi.hip, two flows), "defor" (filterinterp_defor_lds.hip, fs 4 / 6).

Every constant (tile size, threads, ring and ladder limits, thresholds, pitch skew) is read from the #defines of the
kernel's translation unit and of the headers it includes, so an edited constant moves the mirror with it.  The rung ladders below are the mirror's own
statement of each dispatch chain; tests/test_fi_windows_host.py compares them with the chains in the sources.
"""
import functools
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "video-frame-interpolation-based-on-deformable-kernel-region_amd", "csrc")

SOURCES = {"lds": "filterinterp_lds.hip", "blend": "filterinterp_lds.hip", "n": "filterinterp_lds_n.hip",
           "f16": "filterinterp_f16.hip", "multi": "filterinterp_multi.hip", "defor": "filterinterp_defor_lds.hip"}

# the header of the 16-bit staged kernels: constants, tile prologue, channel loop, ladder, launch plan
FAMILY16 = "filterinterp_16.h"

f32 = np.float32


# ------------------------------------------------------------------ the sources

def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


@functools.lru_cache(maxsize=None)
def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return _strip_comments(f.read())


def _eval(expr, env):
    expr = expr.strip()
    if not re.fullmatch(r"[\w\s()+\-*/]+", expr):
        raise ValueError(expr)
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(env)))


_DEFINE = r"^\s*#define\s+(\w+)[ \t]+([^\n]+)$"


def includes(name):
    """the project headers a file includes itself (`#include "..."`), in source order"""
    return re.findall(r'^\s*#include\s+"([^"]+)"', source(name), flags=re.M)


@functools.lru_cache(maxsize=None)
def defines(name):
    """The object-like integer #defines of a translation unit: filterinterp_dev.h's (its FI_PITCH_SKEW only where the
    unit, or a header the unit includes, does not define one first), then those of the unit's own headers (one level of
    #include "..."), then the unit's own, each evaluated in terms of the ones before it."""
    env = {}
    files = [h for h in includes(name) if h != "filterinterp_dev.h" and os.path.exists(os.path.join(CSRC, h))] + [name]
    own_names = {k for f in files for k, _ in re.findall(_DEFINE, source(f), flags=re.M)}
    for fname in ["filterinterp_dev.h"] + files:
        for k, v in re.findall(_DEFINE, source(fname), flags=re.M):
            if fname == "filterinterp_dev.h" and k in own_names:
                continue
            try:
                env[k] = _eval(v, env)
            except (ValueError, SyntaxError, NameError, TypeError):
                pass
    return env


def macro_body(name, macro):
    """(parameter, body) of the one-parameter function-like macro `macro` of a file, continuation lines joined; None
    where the file defines no such macro"""
    m = re.search(r"^\s*#define\s+" + macro + r"\((\w+)\)((?:[^\n]*\\\n)*[^\n]*)$", source(name), flags=re.M)
    return (m.group(1), m.group(2).replace("\\\n", "\n")) if m else None


def _dispatch_text(name):
    """The source without preprocessor lines (a macro's own definition is not one of its uses)."""
    out, cont = [], False
    for line in source(name).split("\n"):
        if cont or line.lstrip().startswith("#"):
            cont = line.rstrip().endswith("\\")
            continue
        out.append(line)
    return "\n".join(out)


def source_chain(name, macro):
    """The uses of `macro` in source order as (variable, op, bound, args): `if (kmax <= 2 * FI_KS) FI_RUN(2 * FI_KS)`
    -> ("kmax", "<=", 2, (2,)); an `else` without a condition -> (None, None, None, args).  Values evaluated.  Where the
    file defines `macro` itself as a ladder over its parameter (`#define FI16_LADDER(RUN) if (kmax <= 2) RUN(2); ...`),
    the chain is that definition's."""
    env = defines(name)
    text = _dispatch_text(name)
    ladder = macro_body(name, macro)
    if ladder and re.search(r"\bif\s*\(", ladder[1]) and re.search(r"\b%s\(" % ladder[0], ladder[1]):
        macro, text = ladder
    pat = r"(?:if\s*\(\s*(\w+)\s*(<=|==)\s*([^()]*?)\s*\)\s*)?\b" + macro + r"\(([^()]*)\)"
    out = []
    for var, op, bound, args in re.findall(pat, text):
        vals = tuple(_eval(a, env) for a in args.split(","))
        out.append((var or None, op or None, _eval(bound, env) if bound else None, vals))
    return out


def source_expr(name, pattern):
    """group 1 of the first match of `pattern` in the (comment-free) source, whitespace collapsed"""
    m = re.search(pattern, source(name))
    if not m:
        raise AssertionError("%s: no match for %r" % (name, pattern))
    return " ".join(m.group(1).split())


# ------------------------------------------------------------------ the mirror's ladders

def rungs(kernel):
    """The mirror's dispatch chain of a kernel: [(op, bound, K)], op None = the final else."""
    if kernel in ("lds", "blend"):
        ks = defines(SOURCES[kernel])["FI_KS"]
        return [("<=", m * ks, m * ks) for m in (2, 3, 4, 5, 6, 7, 8, 10, 12)] + [(None, None, 15 * ks)]
    if kernel in ("n", "defor"):
        return [("<=", 3, 3), ("==", 4, 4), ("==", 5, 5), ("==", 6, 6), ("<=", 8, 8), ("<=", 10, 10), ("<=", 12, 12),
                (None, None, 15)]
    if kernel == "f16":
        return [("<=", 2, 2), ("==", 3, 3), ("==", 4, 4), ("<=", 6, 6), (None, None, 8)]
    if kernel == "multi":
        return [("<=", 8, 8), ("<=", 10, 10), ("<=", 12, 12), (None, None, 15)]
    raise KeyError(kernel)


# 16-byte staging of the lean fs = 4 loop: gate k16 <= 3, then units per thread
RUNGS16 = [("<=", 1, 1), ("==", 2, 2), (None, None, 3)]
D16_MAX = 3
B64_KMAX_MUL = 10           # FI_RUN: 8-byte reads compiled for K <= 10 * FI_KS; fits64: pitch * bh <= 10 * FI_KS * threads
# shared-window kernel: paired classes (segs, rows8 condition) -> (S, KR)
PAIRED = [(3, ("==", 3), (3, 3)), (3, ("==", 4), (3, 4)), (3, ("==", 5), (3, 5)), (3, (None, None), (3, 6)),
          (4, ("==", 3), (4, 3)), (4, (None, None), (4, 4))]
PAIRED_COND = "segs <= 4 && segs * rows8 <= FM_KPAIR"
# fi_channel_split's prologue argument per launcher (in channels' worth)
SPLIT_PROLOGUE = {"lds": "4.3", "n": "4.3 * (2 + fs * fs) / 18.0", "f16": "4.3",
                  "multi": "4.3 * (1.0 + 0.3 * (nflows - 1)) / nflows",
                  "defor": "variant == VFI_DEFOR_NOFILTER ? 2.0 : 3.0"}


def split_prologue(kernel, fs=4, variant=0, nflows=2):
    if kernel == "blend":
        return None                                  # the blend epilogue keeps a pixel's channels in one workgroup
    return {"lds": 4.3, "f16": 4.3, "n": 4.3 * (2 + fs * fs) / 18.0, "multi": 4.3 * (1.0 + 0.3 * (nflows - 1)) / nflows,
            "defor": 2.0 if variant == 2 else 3.0}[kernel]


def fi_channel_split(ntiles, channel, prologue, cu_count):
    """filterinterp.hip fi_channel_split: (ch_per_group, groups)"""
    if prologue is None:
        return channel, 1
    slots = cu_count * 2
    best, best_cost = 1, 0.0
    for g in range(1, min(8, channel) + 1):
        r = ntiles * g / slots
        cost = (channel + prologue * g) * ((r + 0.5) / r) * (1.0 + 0.25 / r)
        if g == 1 or cost < best_cost:
            best_cost, best = cost, g
    cpg = (channel + best - 1) // best
    return cpg, (channel + cpg - 1) // cpg


def xcd_grid(ntiles, round_=None):
    """filterinterp_dev.h fi_xcd_grid<ROUND>"""
    d = defines("filterinterp_lds.hip")
    xcds, run = d["FI_XCDS"], d["FI_XCD_RUN"]
    r = run if round_ is None else round_
    return ((ntiles + xcds - 1) // xcds + r - 1) // r * r * xcds


# ------------------------------------------------------------------ geometry per kernel

def geometry(kernel, fs=4):
    """(tile rows, tile columns, threads, first tap column relative to the sample's integer column, taps per row)"""
    d = defines(SOURCES[kernel])
    if kernel in ("lds", "blend"):
        return d["FI_TH"], d["FI_TW"], d["FI_THREADS"], -1, 4
    if kernel == "n":
        return d["FN_TH"], d["FN_TW"], d["FN_THREADS"], 1 - fs // 2, fs
    if kernel == "f16":
        return d["FI16_TH"], d["FI16_TW"], d["FI16_THREADS"], -1, 4
    if kernel == "multi":
        return d["FM_TH"], d["FM_TW"], d["FM_THREADS"], -1, 4
    if kernel == "defor":
        return d["DF_TH"], d["DF_TW"], d["DF_THREADS"], 1 - fs // 2, fs
    raise KeyError(kernel)


def _pick(chain, v):
    out = np.zeros(v.shape, np.int64)
    done = np.zeros(v.shape, bool)
    for op, b, k in chain:
        m = ~done & (np.ones(v.shape, bool) if op is None else (v <= b if op == "<=" else v == b))
        out[m] = k
        done |= m
    return out


def _ceil(a, b):
    return -(-a // b)


@functools.lru_cache(maxsize=None)
def _lut(fmt):
    return np.array([fmt % k for k in range(64)], object)


def pitch_for(bw, skew):
    """filterinterp_dev.h fi_pitch_for"""
    if skew:
        return ((np.maximum(bw - skew, 0) + 31) & ~31) + skew
    return (bw + 31) & ~31


def decide(kernel, x0, y0, x1, y1, anyv, h, w, aligned=True, detail=None):
    """The tile-uniform choice from the tap bounding box {x0, y0, x1, y1} (inclusive; for "f16" the box of the clamped
    window columns, for "defor" of the clamped corners).  Arrays in, (labels, staged elements n) out; "lds" / "blend"
    also fill `detail` (a dict) with the intermediate quantities of the kernel's decision."""
    x0, y0, x1, y1 = (np.asarray(a, np.int64) for a in (x0, y0, x1, y1))
    anyv = np.asarray(anyv, bool)
    x0, y0 = np.where(anyv, x0, 0), np.where(anyv, y0, 0)
    x1, y1 = np.where(anyv, x1, -1), np.where(anyv, y1, -1)
    d = defines(SOURCES[kernel])
    bh = np.where(anyv, y1 - y0 + 1, 0)
    if kernel in ("lds", "blend"):
        ks, thr = d["FI_KS"], d["FI_THREADS"]
        lean = kernel == "lds"
        raw_bw = np.where(anyv, x1 - x0 + 1, 0)
        can16 = lean & bool(aligned) & anyv & (x0 >= 0) & (x1 < w)
        lo = np.where(can16, x0 & ~3, x0)
        bw64 = np.where(anyv, x1 - (lo & ~1) + 1, 0)
        fits64 = ((((bw64 + 31) >> 6) << 6) + d["FI_B64_PITCH_SKEW"]) * bh <= B64_KMAX_MUL * ks * thr
        use64 = lean & fits64 & ((bh >= d["FI_B64_MIN_BH"]) | (raw_bw >= d["FI_B64_MIN_BW"]))
        bx0 = np.where(use64 & anyv, lo & ~1, lo)
        bw = np.where(anyv, x1 - bx0 + 1, 0)
        pitch = np.where(use64, (((bw + 31) >> 6) << 6) + d["FI_B64_PITCH_SKEW"], pitch_for(bw, d["FI_PITCH_SKEW"]))
        n = pitch * bh
        kmax = _ceil(n, thr)
        gather = kmax > d["FI_KTOP"]
        k16 = _ceil(n, 4 * thr)
        d16 = can16 & (k16 <= D16_MAX) & ~gather
        K16, K = _pick(RUNGS16, k16), _pick(rungs(kernel), kmax)
        ring = np.where(use64, np.where(K > B64_KMAX_MUL * ks, _lut("K=%d b64 UNCOMPILED")[K], _lut("K=%d b64")[K]),
                        _lut("K=%d")[K])
        d16n = np.where(use64, _lut("d16 k16=%d b64")[K16], _lut("d16 k16=%d")[K16])
        names = np.where(~anyv, "none", np.where(gather, "gather", np.where(d16, d16n, ring))).astype(object)
        if detail is not None:
            detail.update(raw_bw=raw_bw, raw_bh=bh, can16=can16, lo=lo, bw64=bw64, fits64=fits64, use64=use64, bx0=bx0,
                          bw=bw, pitch=pitch, n=n, kmax=kmax, k16=k16)
        return names, n
    if kernel == "multi":
        bw = np.where(anyv, x1 - x0 + 1, 0)
        bwp = np.where(anyv, bw - 2, 0)
        segs = np.maximum(3, (bwp + 31) >> 5)
        rows8 = np.maximum(3, (bh + 7) >> 3)
        paired = (segs <= 4) & (segs * rows8 <= d["FM_KPAIR"])
        pitch = np.where(paired, 32 * segs, (bw + 31) & ~31)
        n = np.where(paired, 0, pitch * bh)
        kmax = _ceil(n, d["FM_THREADS"])
        K = _pick(rungs(kernel), kmax)
        pn = np.full(x0.shape, "", object)
        for s_, (op, b), c in reversed(PAIRED):
            pn = np.where((segs == s_) & (np.ones(x0.shape, bool) if op is None else rows8 == b), "paired S=%d KR=%d" % c, pn)
        names = np.where(~anyv, "none", np.where(paired, pn, np.where(kmax > d["FM_KTOP"], "gather",
                                                                       _lut("plain K=%d")[K]))).astype(object)
        return names, np.where(paired, bw * bh, n)
    if kernel == "f16":
        bx0 = np.where(anyv, x0 & ~1, 0)
        bw = np.where(anyv, (x1 - bx0 + 2) >> 1, 0)
        pitch = pitch_for(bw, d["FI_PITCH_SKEW"])
        n = pitch * bh
        kmax, ktop = _ceil(n, d["FI16_THREADS"]), d["FI16_KTOP"]
    elif kernel == "n":
        bw = np.where(anyv, x1 - x0 + 1, 0)
        n = ((bw + 31) & ~31) * bh
        kmax, ktop = _ceil(n, d["FN_THREADS"]), d["FN_KTOP"]
    elif kernel == "defor":
        bw = np.where(anyv, x1 - x0 + 1, 0)
        n = ((bw + 31) & ~31) * bh
        kmax, ktop = np.minimum(_ceil(n, d["DF_THREADS"]), d["DF_KTOP"] + 1), d["DF_KTOP"]
    else:
        raise KeyError(kernel)
    K = _pick(rungs(kernel), kmax)
    names = np.where(~anyv, "none", np.where(kmax > ktop, "gather", _lut("K=%d")[K])).astype(object)
    return names, n


def all_classes(kernel, aligned=True):
    """Every class the table of the kernel lists (the 16-byte classes need an aligned layout)."""
    if kernel == "lds":
        ks = defines(SOURCES[kernel])["FI_KS"]
        out = ["d16 k16=%d%s" % (k, b) for _, _, k in RUNGS16 for b in ("", " b64")] if aligned else []
        for _, _, k in rungs(kernel):
            out.append("K=%d" % k)
            if k <= B64_KMAX_MUL * ks:
                out.append("K=%d b64" % k)
        return out + ["gather", "none"]
    if kernel == "multi":
        return (["paired S=%d KR=%d" % c for _, _, c in PAIRED] + ["plain K=%d" % k for _, _, k in rungs(kernel)] +
                ["gather", "none"])
    return ["K=%d" % k for _, _, k in rungs(kernel)] + ["gather", "none"]


# ------------------------------------------------------------------ per-pixel samples and per-tile boxes

def samples(flow, h, w):
    """fi_valid and the integer sample position (int)x2, (int)y2 in fp32, as the kernels compute them"""
    fx, fy = flow[:, 0].astype(f32), flow[:, 1].astype(f32)
    x2 = np.arange(w, dtype=f32)[None, None, :] + fx
    y2 = np.arange(h, dtype=f32)[None, :, None] + fy
    with np.errstate(invalid="ignore"):
        valid = ((x2 >= 0) & (y2 >= 0) & (x2 <= f32(w - 1)) & (y2 <= f32(h - 1)) &
                 (np.abs(fx) < f32(w) / f32(2)) & (np.abs(fy) < f32(h) / f32(2)))
    ix = np.where(valid, x2, 0).astype(np.int64)
    iy = np.where(valid, y2, 0).astype(np.int64)
    return valid, ix, iy, x2, y2


def to_tiles(a, th, tw, fill):
    """[B, h, w] -> [B, tiles_y, tiles_x, th * tw]"""
    B, h, w = a.shape
    ty, tx = _ceil(h, th), _ceil(w, tw)
    p = np.full((B, ty * th, tx * tw), fill, a.dtype)
    p[:, :h, :w] = a
    return p.reshape(B, ty, th, tx, tw).transpose(0, 1, 3, 2, 4).reshape(B, ty, tx, th * tw)


def _fold(parts, th, tw):
    """bounding box over (valid, lo_x, lo_y, hi_x, hi_y) pixel arrays [B, h, w] -> per-tile x0, y0, x1, y1, any"""
    big = np.iinfo(np.int64).max
    x0 = y0 = x1 = y1 = anyv = None
    for valid, lx, ly, hx, hy in parts:
        v = to_tiles(valid, th, tw, False)
        a = [to_tiles(np.where(valid, t, fill), th, tw, fill).min(-1) if fill == big else
             to_tiles(np.where(valid, t, fill), th, tw, fill).max(-1)
             for t, fill in ((lx, big), (ly, big), (hx, -big), (hy, -big))]
        if x0 is None:
            x0, y0, x1, y1, anyv = a[0], a[1], a[2], a[3], v.any(-1)
        else:
            x0, y0 = np.minimum(x0, a[0]), np.minimum(y0, a[1])
            x1, y1 = np.maximum(x1, a[2]), np.maximum(y1, a[3])
            anyv = anyv | v.any(-1)
    return x0, y0, x1, y1, anyv


def tile_boxes(kernel, flow, h, w, fs=4, flow2=None, off=None):
    """per-tile tap bounding boxes (x0, y0, x1, y1, any_valid), each [B, tiles_y, tiles_x]"""
    th, tw, _, o, span = geometry(kernel, fs)
    valid, ix, iy, _, _ = samples(flow, h, w)
    if kernel == "defor":
        nt = fs * fs
        off = off.astype(f32)
        lx, ly, hx, hy = (np.full(valid.shape, v, np.int64) for v in (2 ** 40, 2 ** 40, -2 ** 40, -2 ** 40))
        L, T = ix + o, iy + o
        for k in range(nt):
            cj = np.clip(T + k // fs, 0, h - 1)
            ci = np.clip(L + k % fs, 0, w - 1)
            fy = cj.astype(f32) + off[:, k]
            fx = ci.astype(f32) + off[:, nt + k]
            tt = np.clip(np.trunc(np.where(valid, fy, 0)).astype(np.int64), -1, h - 1)
            tl = np.clip(np.trunc(np.where(valid, fx, 0)).astype(np.int64), -1, w - 1)
            lx, ly = np.minimum(lx, tl), np.minimum(ly, tt)
            hx, hy = np.maximum(hx, tl + 1), np.maximum(hy, tt + 1)
        return _fold([(valid, lx, ly, hx, hy)], th, tw)
    parts = []
    for fl in ((flow,) if flow2 is None else (flow, flow2)):
        valid, ix, iy, _, _ = samples(fl, h, w)
        L, T = ix + o, iy + o
        if kernel == "f16":
            L = np.clip(L, 0, w - 4)
        parts.append((valid, L, T, L + span - 1, T + span - 1))
    return _fold(parts, th, tw)


def classes(kernel, flow, h, w, aligned=True, fs=4, flow2=None, off=None):
    """class label per (batch item, tile row, tile column)"""
    x0, y0, x1, y1, anyv = tile_boxes(kernel, flow, h, w, fs, flow2, off)
    return decide(kernel, x0, y0, x1, y1, anyv, h, w, aligned)[0]


def pixel_labels(kernel, labels, h, w, fs=4):
    """the tile labels spread over the tiles' pixels: [B, h, w]"""
    th, tw = geometry(kernel, fs)[:2]
    return np.repeat(np.repeat(labels, th, axis=1), tw, axis=2)[:, :h, :w]


def aligned16(t):
    """the host's aligned16 for a float32 input1 (filterinterp_lds.hip forward_ori_lds)"""
    _, _, h, w = t.shape
    sb, sc, sh, _ = t.stride()
    return (w % 4 == 0 and sh % 4 == 0 and sc % 4 == 0 and sb % 4 == 0 and t.data_ptr() % 16 == 0 and sc > 0 and
            4 * sc + 4 * ((h - 1) * sh + w) < 0x7fffffff)


# ------------------------------------------------------------------ the field builder

EDGES = ("in", "left", "right", "top", "bottom")

# frame (h, w) of each kernel's all-class field, B = 2: enough tiles for every class twice (fullest and smallest box)
# plus the edge boxes, tile counts off the XCD rounding of fi_xcd_grid (the surplus workgroups leave), ragged last tiles
# where w is not a multiple of the tile width
FIELDS = {("lds", True): (240, 384), ("lds", False): (240, 382), ("blend", True): (120, 510), ("n", True): (124, 446),
          ("f16", True): (112, 445), ("multi", True): (112, 512), ("defor", True): (94, 250)}


def field_shape(kernel, aligned=True):
    return FIELDS[(kernel, aligned if kernel == "lds" else True)]


def _box_range(kernel, h, w, fs):
    """smallest x0 / y0 and largest x1 / y1 a box can have"""
    o, span = geometry(kernel, fs)[3:]
    if kernel == "defor":
        return -1, -1, w, h
    if kernel == "f16":
        return 0, o, w - 1, h - 1 + o + span - 1
    return o, o, w - 1 + o + span - 1, h - 1 + o + span - 1


def _place(kernel, edge, bw, bh, cx, cy, r, h, w, fs):
    """box (x0, y0) of a bw x bh box for a tile centred at (cx, cy): inside the frame ("in", "top", "bottom" in x;
    x0 = r mod 4), or on the frame's smallest / largest reachable column or row"""
    xlo, ylo, xhi, yhi = _box_range(kernel, h, w, fs)
    if edge == "left":
        x0 = xlo
    elif edge == "right":
        x0 = xhi - bw + 1
    else:
        x0 = min(max(cx - bw // 2, 0), w - bw)
        x0 -= (x0 - r) % 4
        if x0 < 0:
            x0 += 4
    if edge == "top":
        y0 = ylo
    elif edge == "bottom":
        y0 = yhi - bh + 1
    else:
        y0 = min(max(cy - bh // 2, 0), h - bh)
    return x0, y0


def _edge_ok(kernel, edge, h, w, fs):
    xlo, ylo, xhi, yhi = _box_range(kernel, h, w, fs)
    return {"in": True, "left": xlo < 0, "right": xhi > w - 1, "top": ylo < 0, "bottom": yhi > h - 1}[edge]


def _search(kernel, label, edge, r, h, w, aligned, fs, bwmax, bhmax):
    """(bw, bh) of the box with the most and of the box with the fewest staged elements that lands in `label`
    (None when no box does)"""
    span = geometry(kernel, fs)[4]
    bmin = 2 if kernel == "defor" else span
    bw, bh = np.meshgrid(np.arange(bmin, bwmax + 1), np.arange(bmin, bhmax + 1), indexing="ij")
    bw, bh = bw.ravel(), bh.ravel()
    xlo, ylo, xhi, yhi = _box_range(kernel, h, w, fs)
    if edge == "left":
        x0 = np.full(bw.shape, xlo)
    elif edge == "right":
        x0 = xhi - bw + 1
    else:
        x0 = np.clip(w // 2 - bw // 2, 0, w - bw)
        x0 = x0 - (x0 - r) % 4
        x0 = np.where(x0 < 0, x0 + 4, x0)
    y0 = np.clip(h // 2 - bh // 2, 0, h - bh)
    if edge == "in":
        ok = (x0 >= 0) & (x0 + bw - 1 <= w - 1)
    else:
        ok = (x0 >= xlo) & (x0 + bw - 1 <= xhi)
    names, n = decide(kernel, x0, y0, x0 + bw - 1, y0 + bh - 1, np.ones(bw.shape, bool), h, w, aligned)
    hit = np.flatnonzero((names == label) & ok)
    if hit.size == 0:
        return None
    size = bw[hit] + bh[hit]
    big = hit[np.lexsort((size, -n[hit]))[0]]
    small = hit[np.lexsort((size, n[hit]))[0]]
    return (int(bw[big]), int(bh[big])), (int(bw[small]), int(bh[small]))


def targets(kernel, h, w, aligned=True, fs=4, rng=None):
    """[(label, edge, r, bw, bh)]: per class the fullest box and the smallest one, inside the frame where the class
    allows it, else on its left / right edge; one box on every reachable edge; one tile without a valid pixel"""
    rng = np.random.default_rng(0) if rng is None else rng
    th, tw = geometry(kernel, fs)[:2]
    # (a box no farther from its tile's pixels than half the frame: fi_valid bounds |flow| by w / 2 and h / 2)
    bwmax = min(w // 2 + tw - 4, 240) if kernel != "defor" else min(w, 240)
    bhmax = min(h // 2 - 4, 100) if kernel != "defor" else h
    out = []
    for label in all_classes(kernel, aligned):
        if label == "none":
            out.append(("none", "in", 0, 0, 0))
            continue
        got = None
        for edge in ("in", "left", "right"):
            if not _edge_ok(kernel, edge, h, w, fs):
                continue
            r = int(rng.integers(0, 4))
            got = _search(kernel, label, edge, r, h, w, aligned, fs, bwmax, bhmax)
            if got is not None:
                break
        if got is None:
            raise AssertionError("%s: no box lands in %r" % (kernel, label))
        for bw, bh in dict.fromkeys(got):
            out.append((label, edge, r, bw, bh))
    boxes = [t for t in out if t[0] != "none"]
    for edge in EDGES[1:]:
        if _edge_ok(kernel, edge, h, w, fs):
            _, _, r, bw, bh = boxes[int(rng.integers(0, len(boxes)))]
            out.append((None, edge, r, bw, bh))
    return out


def _realise_fi(kernel, rng, fl, valid_mask, box, tile, h, w, fs, half=None, anchors=(True, True)):
    """write into fl ([2, h, w], this batch item) the flow of one tile's pixels: anchors on the box's corners, a share
    of the rest on random dyadic positions inside it, everything else invalid (far outside the frame)"""
    th, tw, _, o, span = geometry(kernel, fs)
    x0, y0, x1, y1 = box
    ty, tx = tile
    ys, xs = np.meshgrid(np.arange(ty * th, min(h, ty * th + th)), np.arange(tx * tw, min(w, tx * tw + tw)), indexing="ij")
    ys, xs = ys.ravel(), xs.ravel()
    if kernel == "f16":     # columns of the clamped window: Lc = clamp(ix - 1, 0, w - 4)
        lc_lo, lc_hi = x0, x1 - 3
    else:
        lc_lo, lc_hi = x0, x1 - span + 1
    if half is not None:
        lc_hi = max(lc_lo, min(lc_hi, lc_lo + half))
    lt_lo, lt_hi = y0, y1 - span + 1
    n = xs.size
    Lc = rng.integers(lc_lo, lc_hi + 1, n)
    Tt = rng.integers(lt_lo, lt_hi + 1, n)
    use = rng.random(n) < 0.6
    pts = []
    if anchors[0]:
        pts.append((lc_lo, lt_lo))
    if anchors[1]:
        pts.append((lc_hi, lt_hi))
    for ax, ay in pts:          # the pixel nearest its target
        ix_t, iy_t = ax - o, ay - o
        k = int(np.argmin(np.abs(xs - ix_t) + np.abs(ys - iy_t)))
        Lc[k], Tt[k], use[k] = ax, ay, True
    if kernel == "f16":
        ix = Lc + 1
        ix = np.where(Lc == 0, rng.integers(0, 2, n), ix)
        ix = np.where(Lc == w - 4, rng.integers(w - 3, w, n), ix)
    else:
        ix = Lc - o
    iy = Tt - o
    fxr = rng.integers(0, 64, n) / 64.0
    fyr = rng.integers(0, 64, n) / 64.0
    fxr = np.where(ix >= w - 1, 0.0, fxr)
    fyr = np.where(iy >= h - 1, 0.0, fyr)
    fx = (ix + fxr - xs).astype(f32)
    fy = (iy + fyr - ys).astype(f32)
    ok = use & (np.abs(fx) < w / 2) & (np.abs(fy) < h / 2) & (ix >= 0) & (ix <= w - 1) & (iy >= 0) & (iy <= h - 1)
    fl[0, ys, xs] = np.where(ok, fx, f32(4 * w))
    fl[1, ys, xs] = np.where(ok, fy, f32(0))
    valid_mask[ys, xs] = ok


def _realise_defor(rng, fl, off, box, tile, h, w, fs):
    """deformable: small valid sampling flows, and per tap an offset that puts its top-left corner on a random cell of
    the box (corners before the clamp to [-1, h-1] / [-1, w-1]: some land beyond the frame and are clamped); two taps
    on the box's corners"""
    th, tw, _, o, _ = geometry("defor", fs)
    nt = fs * fs
    x0, y0, x1, y1 = box
    ty, tx = tile
    ys, xs = np.meshgrid(np.arange(ty * th, min(h, ty * th + th)), np.arange(tx * tw, min(w, tx * tw + tw)), indexing="ij")
    ys, xs = ys.ravel(), xs.ravel()
    n = xs.size
    fx = (rng.integers(-64, 65, n) / 64.0).astype(f32)
    fy = (rng.integers(-64, 65, n) / 64.0).astype(f32)
    x2, y2 = xs + fx, ys + fy
    inside = (x2 >= 0) & (x2 <= w - 1) & (y2 >= 0) & (y2 <= h - 1)
    fx, fy = np.where(inside, fx, f32(0)), np.where(inside, fy, f32(0))
    use = rng.random(n) < 0.7
    use[0] = use[n - 1] = True
    fl[0, ys, xs] = np.where(use, fx, f32(4 * w))
    fl[1, ys, xs] = np.where(use, fy, f32(0))
    ix, iy = (xs + fx).astype(np.int64), (ys + fy).astype(np.int64)
    Lft = rng.integers(x0, x1, (nt, n))             # corner columns x0 .. x1 - 1
    Top = rng.integers(y0, y1, (nt, n))
    Lft[0, 0], Top[0, 0] = x0, y0
    Lft[1, n - 1], Top[1, n - 1] = x1 - 1, y1 - 1
    for k in range(nt):
        cj = np.clip(iy + o + k // fs, 0, h - 1)
        ci = np.clip(ix + o + k % fs, 0, w - 1)
        fr_x, fr_y = rng.integers(0, 64, n) / 64.0, rng.integers(0, 64, n) / 64.0
        beyond_x, beyond_y = rng.integers(0, 3, n), rng.integers(0, 3, n)
        # a corner column -1 comes from any position below 0 (truncated: (-2, -1] is -1, beyond is clamped);
        # w - 1 from any position at or past it
        fxk = np.where(Lft[k] == -1, -1.0 - fr_x - beyond_x, np.where(Lft[k] == w - 1, w - 1 + fr_x + beyond_x, Lft[k] + fr_x))
        fyk = np.where(Top[k] == -1, -1.0 - fr_y - beyond_y, np.where(Top[k] == h - 1, h - 1 + fr_y + beyond_y, Top[k] + fr_y))
        off[k, ys, xs] = np.where(use, fyk - cj, rng.uniform(-1, 1, n)).astype(f32)
        off[nt + k, ys, xs] = np.where(use, fxk - ci, rng.uniform(-1, 1, n)).astype(f32)


def build_field(kernel, rng, B, h, w, aligned=True, fs=4, split=None):
    """Flow field(s) in which every class of all_classes(kernel, aligned) owns at least one tile of every batch item,
    each item with its own layout.  Returns a dict: "flow" [B, 2, h, w]; "flow2" (multi: the second flow; the first flow
    covers the left part of each box only, so its own box is narrower than the union); "off" (defor: [B, 2 fs^2, h, w]);
    "plan": per item the {(tile row, tile column): (label, edge, column residue, bw, bh)} that was aimed at (label None:
    an extra box on an edge, whatever class it lands in)."""
    th, tw = geometry(kernel, fs)[:2]
    tiles_y, tiles_x = _ceil(h, th), _ceil(w, tw)
    tlist = targets(kernel, h, w, aligned, fs, rng)
    flow = np.zeros((B, 2, h, w), f32)
    flow2 = np.zeros((B, 2, h, w), f32) if kernel == "multi" else None
    off = np.zeros((B, 2 * fs * fs, h, w), f32) if kernel == "defor" else None
    plans = []
    for b in range(B):
        free = {(ty, tx) for ty in range(tiles_y) for tx in range(tiles_x)}
        order = [tlist[i] for i in rng.permutation(len(tlist))]
        # edge targets first, each to the free tile nearest its edge
        order.sort(key=lambda t: t[1] == "in")
        plan = {}
        for label, edge, r, bw, bh in order:
            if not free:
                raise AssertionError("%s: %d targets, %d tiles" % (kernel, len(tlist), tiles_x * tiles_y))
            if edge == "left":
                key = lambda t: (t[1], rng.random())
            elif edge == "right":
                key = lambda t: (-t[1], rng.random())
            elif edge == "top":
                key = lambda t: (t[0], rng.random())
            elif edge == "bottom":
                key = lambda t: (-t[0], rng.random())
            else:
                key = lambda t: rng.random()
            tile = min(free, key=key)
            free.discard(tile)
            plan[tile] = (label, edge, r, bw, bh)
        inner = [t for t in tlist if t[1] == "in" and t[0] is not None]
        for tile in sorted(free):                 # the rest: any target inside the frame again
            plan[tile] = inner[int(rng.integers(0, len(inner)))]
        vm = np.zeros((h, w), bool)
        for (ty, tx), (label, edge, r, bw, bh) in sorted(plan.items()):
            ys = slice(ty * th, min(h, ty * th + th))
            xs = slice(tx * tw, min(w, tx * tw + tw))
            if label == "none":
                flow[b, 0, ys, xs] = 4 * w
                if flow2 is not None:
                    flow2[b, 0, ys, xs] = -4 * w
                continue
            cx, cy = (tx * tw + min(w, tx * tw + tw)) // 2, (ty * th + min(h, ty * th + th)) // 2   # (ragged last tiles)
            x0, y0 = _place(kernel, edge, bw, bh, cx, cy, r, h, w, fs)
            box = (x0, y0, x0 + bw - 1, y0 + bh - 1)
            if kernel == "defor":
                _realise_defor(rng, flow[b], off[b], box, (ty, tx), h, w, fs)
            elif kernel == "multi":
                _realise_fi(kernel, rng, flow[b], vm, box, (ty, tx), h, w, fs, half=max(0, bw // 2 - 3), anchors=(True, False))
                _realise_fi(kernel, rng, flow2[b], vm.copy(), box, (ty, tx), h, w, fs, anchors=(False, True))
            else:
                _realise_fi(kernel, rng, flow[b], vm, box, (ty, tx), h, w, fs)
        plans.append(plan)
    out = {"flow": flow, "plan": plans}
    if flow2 is not None:
        out["flow2"] = flow2
    if off is not None:
        out["off"] = off
    return out
