"""Host mirror of the per-tile decisions of the FlowProjection / DepthFlowProjection forward kernels (csrc/projection.hip),
and a field builder that sends every decision through at least one tile.

K0 (proj_scan / proj_scan4) merges, per 64x16 output tile, a record: the source rectangle that can reach the tile, the
largest |fx|, |fy|, |weight| and the smallest weight of the 16x16 source blocks that reach it.  K1 (proj_pull_lean,
proj_pull<DEPTH, true>, proj_pull<DEPTH, false>) picks from that record, per tile, a fixed-point scale per flow component
and for the weight, 1-4 weight classes (depth), and a coarser second pass when a cell takes more than PROJ_ADD_CELL
addends.  A block that reaches more than PROJ_BLOCK_CAP tiles sends the whole call to the atomic fallback.

  records(flow, depth, h, w)          -> K0's merged records, [B, tiles_y, tiles_x, 8] as stored, and the fallback flag
  dispatch(...)                       -> the K0 / K1 instantiation project_forward_list picks for a call
  regimes(flow, depth, k1)            -> per (image, tile) the set of labels of all_regimes() the tile runs through
  scales(flow, depth, k1)             -> per (image, tile, class) kvx, kvy, kc after the retry shift, and the shift
  predict_flowprojection(flow, k1)    -> count and output of FlowProjection before hole filling, bit for bit
  predict_depthflowprojection(...)    -> the same for DepthFlowProjection, in the kernels' class order
  build_field(kind, rng, B, h, w)     -> flow (and depth) in which every label of all_regimes(kind) owns a tile

Every constant is read from the #defines of projection.hip, so an edited constant moves the mirror with it.  The
exact sums are int64 (every sum the kernels keep in 32-bit halves is far below 2^62).
"""
import functools
import math
import re

import numpy as np

from tests.fi_windows import _eval, source

SOURCE = "projection.hip"
f32 = np.float32


@functools.lru_cache(maxsize=None)
def constants():
    """The object-like integer #defines of projection.hip, each evaluated in terms of the ones before it."""
    env = {}
    for k, v in re.findall(r"^\s*#define\s+(\w+)[ \t]+([^\n]+)$", source(SOURCE), flags=re.M):
        try:
            env[k] = _eval(v, env)
        except (ValueError, SyntaxError, NameError, TypeError):
            pass
    return env


def _c(name):
    return constants()[name]


def function_body(name):
    """The body of the function or kernel `name` of projection.hip, found by matching braces from the `{` that ends its
    signature (comment-free text, whitespace collapsed).  `name` is followed by `(` at its definition: a call inside
    another body ends in `;`, not in `{`, before the next `{`."""
    text = source(SOURCE)
    m = re.search(r"\b%s\s*\([^;{}]*\)\s*\{" % re.escape(name), text)
    if not m:
        raise AssertionError("no function %s" % name)
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return " ".join(text[m.end():i - 1].split())


TW, TH, BLK = _c("PROJ_TW"), _c("PROJ_TH"), _c("PROJ_BLK")
ADD_BITS, ADD_CELL, CLS_BITS = _c("PROJ_ADD_BITS"), _c("PROJ_ADD_CELL"), _c("PROJ_CLS_BITS")
BLOCK_CAP, NMAX, INV_BITS = _c("PROJ_BLOCK_CAP"), _c("PROJ_NMAX"), _c("PROJ_INV_BITS")
GH, GW = TH + 1, TW + 1                                     # K1's grid: one row above, one column left of the tile
MAX_CLS = 4                                                 # min(4, ...) in both K1 variants
K_CLAMP = 100                                               # max(-100, min(100, ...)) of the scales
W_LO_BITS, W_HI_BITS = _c("PROJ_W_LO_BITS"), _c("PROJ_W_HI_BITS")   # a block's largest |weight| outside: fallback

K1_VARIANTS = ("lean", "pull_vec", "pull_scalar")
BASE_LABELS = ("empty", "plain", "retry_1", "retry_2", "retry_3+", "wide_cell", "edge_x", "edge_y", "lopsided")
DEPTH_LABELS = ("classes_2", "classes_3", "classes_4", "neg_weight")
WIDE_CELL = 128                                             # addends per top-left grid cell from which a 2^25 bias carried


def all_regimes(kind):
    """The labels a field of `kind` ("flow" or "depth") must cover."""
    return BASE_LABELS + (DEPTH_LABELS if kind == "depth" else ())


# ------------------------------------------------------------------ dispatch (project_forward_list)

def dispatch(depth, sf, sc, s2=None, ptr_mod16=(0, 0, 0, 0), images=1, tiles_y=1):
    """(K0, K1) of project_forward_list.  sf: (b, c, h) element strides of the flow, which the outputs share; sc: (b, h)
    of count; s2: (b, h) of depth; ptr_mod16: byte addresses mod 16 of flow, depth, count, output."""
    pf, pd, pc, po = ptr_mod16
    vec_in = sf[0] % 4 == 0 and sf[1] % 4 == 0 and sf[2] % 4 == 0 and pf == 0
    if depth:
        vec_in = vec_in and s2[0] % 4 == 0 and s2[1] % 4 == 0 and pd == 0
    vec_out = sf[0] % 4 == 0 and sf[1] % 4 == 0 and sf[2] % 4 == 0 and sc[0] % 4 == 0 and sc[1] % 4 == 0 and po == 0 and pc == 0
    k0 = "scan4" if vec_in else "scan"
    if vec_in and vec_out and tiles_y <= 65535 and images <= 65535:
        return k0, "lean"
    return k0, ("pull_vec" if vec_in else "pull_scalar")


def dispatch_of(flow_t, count_t, out_t, depth_t=None):
    """dispatch() for torch tensors as the reference bindings pass them (the output takes the flow's strides)."""
    f, c = flow_t, count_t
    mods = (f.data_ptr() % 16, 0 if depth_t is None else depth_t.data_ptr() % 16, c.data_ptr() % 16, out_t.data_ptr() % 16)
    s2 = None if depth_t is None else (depth_t.stride(0), depth_t.stride(2))
    return dispatch(depth_t is not None, (f.stride(0), f.stride(1), f.stride(2)), (c.stride(0), c.stride(2)), s2, mods,
                    f.shape[0], -(-f.shape[2] // TH))


# ------------------------------------------------------------------ K0

def _bits(a):
    return np.abs(a.astype(f32)).view(np.int32).astype(np.int64)


def weight_unfit(cbits):
    """proj_weight_unfit: the bits of a block's largest |weight| over its valid sources that the fixed-point path cannot
    hold -- NaN, infinite, 2^64 and more, or non-zero below 2^-56.  Such a block sends the call to the fallback."""
    cbits = int(cbits)
    return cbits != 0 and not W_LO_BITS <= cbits < W_HI_BITS


def targets(fx, fy, h, w):
    """The reference's top-left target: x2 = x + fx in fp32, valid when 0 <= x2 <= w - 1 (NaN fails), L = trunc(x2)."""
    ys, xs = np.meshgrid(np.arange(h, dtype=f32), np.arange(w, dtype=f32), indexing="ij")
    x2, y2 = xs + fx.astype(f32), ys + fy.astype(f32)
    with np.errstate(invalid="ignore"):
        valid = (x2 >= 0) & (x2 <= f32(w - 1)) & (y2 >= 0) & (y2 <= f32(h - 1))
    L = np.where(valid, np.trunc(np.where(valid, x2, 0)), 0).astype(np.int64)
    T = np.where(valid, np.trunc(np.where(valid, y2, 0)), 0).astype(np.int64)
    return valid, L, T


def _image_records(fx, fy, d, h, w):
    tx_n, ty_n = -(-w // TW), -(-h // TH)
    rec = np.zeros((ty_n, tx_n, 8), np.int64)
    valid, L, T = targets(fx, fy, h, w)
    xs, ys = np.arange(w)[None, :], np.arange(h)[:, None]
    vb, fb = _bits(fx), _bits(fy)
    db = _bits(d) if d is not None else None
    wild = False
    for by in range(-(-h // BLK)):
        for bx in range(-(-w // BLK)):
            y0, bx0 = by * BLK, bx * BLK
            sl = (slice(y0, min(y0 + BLK, h)), slice(bx0, min(bx0 + BLK, w)))
            m = valid[sl]
            if not m.any():
                continue
            dl = (L[sl] - xs[:, sl[1]])[m]
            dt = (T[sl] - ys[sl[0], :])[m]
            dlmin, dlmax, dtmin, dtmax = dl.min(), dl.max(), dt.min(), dt.max()
            f4, f7 = vb[sl][m].max(), fb[sl][m].max()
            f5 = f6 = 0
            if db is not None:
                dd = db[sl][m]
                f5 = dd.max()
                nz = dd[dd != 0]
                f6 = (INV_BITS - nz).max() if nz.size else 0
            bx1, by1 = min(bx0 + BLK - 1, w - 1), min(y0 + BLK - 1, h - 1)
            X0, X1 = max(bx0 + dlmin, 0), min(bx1 + dlmax, w - 1)
            Y0, Y1 = max(y0 + dtmin, 0), min(by1 + dtmax, h - 1)
            a0, a1 = X0 // TW, min(X1 + 1, w - 1) // TW
            c0, c1 = Y0 // TH, min(Y1 + 1, h - 1) // TH
            if (a1 - a0 + 1) * (c1 - c0 + 1) > BLOCK_CAP or weight_unfit(f5):
                wild = True
                continue
            for ty in range(c0, c1 + 1):
                for tx in range(a0, a1 + 1):
                    ox0, oy0 = tx * TW, ty * TH
                    tx1, ty1 = min(ox0 + TW - 1, w - 1), min(oy0 + TH - 1, h - 1)
                    sx0, sx1 = max(bx0, ox0 - 1 - dlmax), min(bx1, tx1 - dlmin)
                    sy0, sy1 = max(y0, oy0 - 1 - dtmax), min(by1, ty1 - dtmin)
                    if sx0 > sx1 or sy0 > sy1:
                        continue
                    f = (32767 - sx0, 32767 - sy0, sx1 + 1, sy1 + 1, f4, f5, f6, f7)
                    rec[ty, tx] = np.maximum(rec[ty, tx], f)
    return rec, wild


def records(flow, depth, h, w):
    """K0: ([B, tiles_y, tiles_x, 8] records as stored -- 0 = nothing -- , does any block send the call to the fallback)."""
    recs, wild = [], False
    for b in range(flow.shape[0]):
        r, wl = _image_records(flow[b, 0], flow[b, 1], None if depth is None else depth[b, 0], h, w)
        recs.append(r)
        wild = wild or wl
    return np.stack(recs), wild


def rectangle(rec):
    """K1's reading of a record: (ux0, uy0, uw, uh); uh == 0: nothing lands."""
    ux0, uy0 = 32767 - rec[..., 0], 32767 - rec[..., 1]
    uw = rec[..., 2] - ux0
    uh = np.where(rec[..., 2] > 0, rec[..., 3] - uy0, 0)
    return ux0, uy0, uw, uh


# ------------------------------------------------------------------ K1

def _frexp_e(bits):
    return np.frexp(bits.astype(np.int32).view(f32).astype(np.float64))[1].astype(np.int64)


def base_scales(rec, depth):
    """Per tile and class, before the retry: kvx, kvy, kc [..., MAX_CLS] and ncls, emax."""
    efx, efy = _frexp_e(rec[..., 4]), _frexp_e(rec[..., 7])
    ec = _frexp_e(rec[..., 5]) if depth else np.zeros_like(efx)
    emax = (rec[..., 5] >> 23) & 0xFF
    emin = np.where(rec[..., 6] != 0, ((INV_BITS - rec[..., 6]) >> 23) & 0xFF, emax)
    ncls = np.minimum(MAX_CLS, np.maximum(0, emax - emin) // CLS_BITS + 1) if depth else np.ones_like(emax)
    cls = CLS_BITS * np.arange(MAX_CLS)
    clamp = lambda k: np.clip(k, -K_CLAMP, K_CLAMP)     # noqa: E731
    kc = clamp(ADD_BITS - (ec[..., None] - cls))
    kvx = clamp(ADD_BITS - (efx[..., None] + ec[..., None] - cls))
    kvy = clamp(ADD_BITS - (efy[..., None] + ec[..., None] - cls))
    return kvx, kvy, kc, ncls, emax


def _rint_scaled(a, k):
    """__float2int_rn(a * 2^k) for fp32 a: the product is exact in float64, rint rounds half to even."""
    return np.rint(a.astype(np.float64) * np.exp2(k.astype(np.float64))).astype(np.int64)


def _shift_of(n):
    """ceil(log2(n)) - 5 for n > PROJ_ADD_CELL, else 0."""
    n = np.asarray(n, np.int64)
    bl = np.array([int(v - 1).bit_length() for v in n.ravel()], np.int64).reshape(n.shape)
    return np.where(n > ADD_CELL, bl - int(ADD_CELL - 1).bit_length(), 0)


class Mirror:
    """Everything K0 and K1 decide for one call, computed once: records, scales, labels, exact sums."""

    def __init__(self, flow, depth=None, k1="lean"):
        assert k1 in K1_VARIANTS
        flow = np.asarray(flow, f32)
        self.depth_op = depth is not None
        self._depth = depth
        self.k1 = k1
        B, _, h, w = flow.shape
        self.B, self.h, self.w = B, h, w
        self.txn, self.tyn = -(-w // TW), -(-h // TH)
        self.rec, self.fallback = records(flow, depth, h, w)
        kvx, kvy, kc, ncls, emax = base_scales(self.rec, self.depth_op)
        self.ncls = ncls
        nt = B * self.tyn * self.txn
        # every (source, tile grid it lands in): a top-left target (T, L) lies in the grid of tile (T // TH, L // TW) and,
        # on a tile's first row / column minus one, in the grid of the tile below / right as well
        cols = {k: [] for k in ("t", "gi", "gj", "b", "y", "x", "L", "T")}
        for b in range(B):
            valid, L, T = targets(flow[b, 0], flow[b, 1], h, w)
            ys, xs = np.nonzero(valid)
            Ls, Ts = L[ys, xs], T[ys, xs]
            for dy in (0, 1):
                for dx in (0, 1):
                    ty = Ts // TH + dy
                    tx = Ls // TW + dx
                    ok = (ty < self.tyn) & (tx < self.txn)
                    if dy:
                        ok &= Ts % TH == TH - 1
                    if dx:
                        ok &= Ls % TW == TW - 1
                    cols["t"].append(((b * self.tyn + ty) * self.txn + tx)[ok])
                    cols["gi"].append((Ts - (ty * TH - 1))[ok])
                    cols["gj"].append((Ls - (tx * TW - 1))[ok])
                    for k, v in (("b", np.full(ys.shape, b)), ("y", ys), ("x", xs), ("L", Ls), ("T", Ts)):
                        cols[k].append(v[ok])
        e = {k: np.concatenate(v).astype(np.int64) for k, v in cols.items()}
        self.e = e
        fx = flow[e["b"], 0, e["y"], e["x"]]
        fy = flow[e["b"], 1, e["y"], e["x"]]
        d = depth[e["b"], 0, e["y"], e["x"]].astype(f32) if self.depth_op else np.ones_like(fx)
        t = e["t"]
        if self.depth_op:
            delta = emax.reshape(-1)[t] - ((d.view(np.int32).astype(np.int64) >> 23) & 0xFF)
            cls = sum((delta >= CLS_BITS * j).astype(np.int64) for j in (1, 2, 3))
            cls = np.minimum(cls, ncls.reshape(-1)[t] - 1)
        else:
            cls = np.zeros_like(t)
        e["cls"] = cls
        ax = (d * fx).astype(f32) if self.depth_op else fx
        ay = (d * fy).astype(f32) if self.depth_op else fy
        gidx = t * (GH * GW) + e["gi"] * GW + e["gj"]
        kvx, kvy, kc = (k.reshape(nt, MAX_CLS) for k in (kvx, kvy, kc))

        # tile-cell sums of a grid quantity, with the frame's last row / column added twice (R == L, B == T)
        tyi = (np.arange(nt) // self.txn) % self.tyn
        txi = np.arange(nt) % self.txn
        wy = 1 + ((tyi[:, None] * TH + np.arange(TH)[None, :]) == h - 1).astype(np.int64)
        wx = 1 + ((txi[:, None] * TW + np.arange(TW)[None, :]) == w - 1).astype(np.int64)
        inside = (((tyi[:, None] * TH + np.arange(TH)[None, :]) < h)[:, :, None]
                  & ((txi[:, None] * TW + np.arange(TW)[None, :]) < w)[:, None, :])
        self.inside = inside

        def cells(vals, mask):
            G = np.zeros(nt * GH * GW, np.int64)
            np.add.at(G, gidx[mask], vals[mask] if vals is not None else 1)
            G = G.reshape(nt, GH, GW)
            return (G[:, :-1, :-1] + wx[:, None, :] * G[:, :-1, 1:] + wy[:, :, None] * G[:, 1:, :-1]
                    + wy[:, :, None] * wx[:, None, :] * G[:, 1:, 1:]), G

        ncl = int(ncls.max()) if ncls.size else 1
        # first pass (shift 0): the busiest cell, as the kernels count it
        busy = np.zeros((nt, MAX_CLS), np.int64)
        grid_n = np.zeros(nt * GH * GW, np.int64)
        np.add.at(grid_n, gidx, 1)
        self.grid_max = grid_n.reshape(nt, GH * GW).max(axis=1)
        for j in range(ncl):
            m = cls == j
            n_cell, n_grid = cells(None, m)
            if not self.depth_op:
                hi = n_cell
            else:
                wgt = _rint_scaled(d, kc[t, j])
                if k1 == "lean":
                    # each grid cell is one 64-bit word (addends << 32) + sum of (weight + 2^25): the low half carries
                    _, wsum = cells(wgt + (1 << ADD_BITS), m)
                    carry = wsum >> 32
                    g = n_grid + carry
                    hi = (g[:, :-1, :-1] + wx[:, None, :] * g[:, :-1, 1:] + wy[:, :, None] * g[:, 1:, :-1]
                          + wy[:, :, None] * wx[:, None, :] * g[:, 1:, 1:])
                else:
                    # pack2(1, weight) summed over the cell's grid cells: packed_hi = N + (W - sext32(W)) / 2^32
                    W, _ = cells(wgt, m)
                    lo = ((W + (1 << 31)) % (1 << 32)) - (1 << 31)
                    hi = n_cell + (W - lo) // (1 << 32)
            busy[:, j] = np.where(inside, hi, 0).reshape(nt, -1).max(axis=1)
        if k1 == "lean":
            shift = np.repeat(_shift_of(busy.max(axis=1))[:, None], MAX_CLS, axis=1)
        else:
            shift = _shift_of(busy)
        self.busy, self.shift = busy, shift
        self.kvx, self.kvy, self.kc = kvx - shift, kvy - shift, kc - shift

        # the kept pass: exact integer sums per class -> one fp32 rounding, ldexp, classes added in order
        resx = resy = resc = None
        self.n = np.zeros((nt, TH, TW), np.int64)
        self.cls_n = np.zeros((nt, MAX_CLS, TH, TW), np.int64)
        self.absx = np.zeros((nt, TH, TW))
        self.absy = np.zeros((nt, TH, TW))
        self.absc = np.zeros((nt, TH, TW))
        for j in range(ncl):
            m = cls == j
            X, _ = cells(_rint_scaled(-ax, self.kvx[t, j]), m)
            Y, _ = cells(_rint_scaled(-ay, self.kvy[t, j]), m)
            n_cell, _ = cells(None, m)
            self.n += n_cell
            self.cls_n[:, j] = n_cell
            px = np.ldexp(X.astype(f32), -self.kvx[:, j][:, None, None].astype(np.int32)).astype(f32)
            py = np.ldexp(Y.astype(f32), -self.kvy[:, j][:, None, None].astype(np.int32)).astype(f32)
            if self.depth_op:
                C, _ = cells(_rint_scaled(d, self.kc[t, j]), m)
                pc = np.ldexp(C.astype(f32), -self.kc[:, j][:, None, None].astype(np.int32)).astype(f32)
            else:
                pc = n_cell.astype(f32)
            if j == 0:
                resx, resy, resc = px, py, pc
            else:
                resx, resy, resc = (resx + px).astype(f32), (resy + py).astype(f32), (resc + pc).astype(f32)
        for arr, v in ((self.absx, np.abs(ax)), (self.absy, np.abs(ay)), (self.absc, np.abs(d))):
            G = np.zeros(nt * GH * GW)
            np.add.at(G, gidx, v.astype(np.float64))
            G = G.reshape(nt, GH, GW)
            arr += (G[:, :-1, :-1] + wx[:, None, :] * G[:, :-1, 1:] + wy[:, :, None] * G[:, 1:, :-1]
                    + wy[:, :, None] * wx[:, None, :] * G[:, 1:, 1:])
        self.resx, self.resy, self.resc = resx, resy, resc

    # ---- per-cell planes [B, 1 or 2, h, w] from per-tile [nt, TH, TW] arrays
    def plane(self, a):
        a = np.asarray(a).reshape(self.B, self.tyn, self.txn, TH, TW).transpose(0, 1, 3, 2, 4)
        return a.reshape(self.B, self.tyn * TH, self.txn * TW)[:, :self.h, :self.w]

    def tile_plane(self, per_tile):
        """a per-tile value broadcast to its cells"""
        return self.plane(np.broadcast_to(np.asarray(per_tile).reshape(-1, 1, 1), (per_tile.size, TH, TW)))

    def predict(self):
        """(out [B,2,h,w], count [B,1,h,w]) before hole filling, as K1 writes them."""
        c, vx, vy = self.resc, self.resx, self.resy
        if self.depth_op:
            pos = c > 0
            ox = np.where(pos, vx / np.where(pos, c, f32(1)), vx).astype(f32)
            oy = np.where(pos, vy / np.where(pos, c, f32(1)), vy).astype(f32)
        else:
            dd = np.maximum(c, f32(1))
            ox, oy = (vx / dd).astype(f32), (vy / dd).astype(f32)
        out = np.stack([self.plane(ox), self.plane(oy)], 1)
        return out, self.plane(c)[:, None]

    def labels(self):
        """{(b, ty, tx): set of labels}"""
        nt = self.B * self.tyn * self.txn
        e, t = self.e, self.e["t"]
        has = lambda mask: np.bincount(t[mask], minlength=nt) > 0      # noqa: E731
        landed = has(np.ones_like(t, bool))
        edge_x, edge_y = has(e["L"] == self.w - 1), has(e["T"] == self.h - 1)
        rec = self.rec.reshape(nt, 8)
        with np.errstate(over="ignore"):
            mfx = rec[:, 4].astype(np.int32).view(f32).astype(np.float64)
            mfy = rec[:, 7].astype(np.int32).view(f32).astype(np.float64)
        lop = mfy < 2.0 ** -10 * mfx
        neg = np.zeros(nt, bool)
        if self.depth_op:
            neg = has(self._d_of_entries() < 0)
        ncls = self.ncls.reshape(-1)
        smax = self.shift.max(axis=1)
        out = {}
        for i in range(nt):
            b, ty, tx = i // (self.tyn * self.txn), (i // self.txn) % self.tyn, i % self.txn
            s = set()
            if not landed[i]:
                s.add("empty")
            else:
                if smax[i] == 0 and (not self.depth_op or ncls[i] == 1):
                    s.add("plain")
                if smax[i] > 0:
                    s.add("retry_%d" % smax[i] if smax[i] < 3 else "retry_3+")
                if self.grid_max[i] >= WIDE_CELL:
                    s.add("wide_cell")
                if edge_x[i]:
                    s.add("edge_x")
                if edge_y[i]:
                    s.add("edge_y")
                if lop[i]:
                    s.add("lopsided")
                if self.depth_op and ncls[i] > 1:
                    s.add("classes_%d" % ncls[i])
                if neg[i]:
                    s.add("neg_weight")
            out[(b, ty, tx)] = s
        return out

    def _d_of_entries(self):
        return self._depth[self.e["b"], 0, self.e["y"], self.e["x"]]

    def contributors_inside(self):
        """Does every (source, tile) pair lie inside the tile's source rectangle?"""
        ux0, uy0, uw, uh = (a.reshape(-1) for a in rectangle(self.rec))
        t, x, y = self.e["t"], self.e["x"], self.e["y"]
        return (x >= ux0[t]) & (x < ux0[t] + uw[t]) & (y >= uy0[t]) & (y < uy0[t] + uh[t])


def mirror(flow, depth=None, k1="lean"):
    return Mirror(flow, depth, k1)


def regimes(flow, depth=None, k1="lean", k0=None):
    """{"k0", "k1", "fallback", "tiles": {(b, ty, tx): labels}}"""
    m = mirror(flow, depth, k1)
    return {"k0": k0, "k1": k1, "fallback": m.fallback, "tiles": m.labels()}


def scales(flow, depth=None, k1="lean"):
    """(kvx, kvy, kc, shift), each [B, tiles_y, tiles_x, MAX_CLS], after the retry; classes >= ncls unused."""
    m = mirror(flow, depth, k1)
    shp = (m.B, m.tyn, m.txn, MAX_CLS)
    return m.kvx.reshape(shp), m.kvy.reshape(shp), m.kc.reshape(shp), m.shift.reshape(shp)


def predict_flowprojection(flow, k1="lean"):
    """FlowProjection's (out, count) with fillhole = 0, bit for bit (not for a call that takes the fallback)."""
    return mirror(flow, None, k1).predict()


def predict_depthflowprojection(flow, depth, k1="lean"):
    return mirror(flow, depth, k1).predict()


def covered(labels):
    return set().union(*labels.values()) if labels else set()


# ------------------------------------------------------------------ fields

# converging sites: (sources per top-left cell, tile row, tile column) -- 48 -> retry 1, 100 -> 2, 128, 200 -> 3 (and a
# wide cell), 400 -> 4, 1100 -> 6.  The frame below has room for them side by side.
SITES = ((48, 1, 1), (100, 1, 3), (128, 1, 5), (200, 1, 7), (400, 4, 1), (1100, 4, 4))
FIELD_SHAPE = (170, 620)                                    # last tile row 10 high, last tile column 44 wide


def _site(rng, fl, n, cy, cx, dyadic, quarter=False):
    """n sources around (cy, cx) whose top-left target is (cy, cx)."""
    side = int(math.ceil(math.sqrt(n)))
    y0, x0 = cy - side // 2, cx - side // 2
    idx = [(y0 + i // side, x0 + i % side) for i in range(n)]
    for (y, x) in idx:
        frx = rng.integers(0, 8) / 8 if dyadic else rng.uniform(0, 0.999)
        fry = rng.integers(0, 8) / 8 if dyadic else rng.uniform(0, 0.999)
        fl[0, y, x] = cx - x + frx
        fl[1, y, x] = cy - y + fry


def build_field(kind, rng, B=1, h=None, w=None, dyadic=False):
    """(flow [B,2,h,w], depth [B,1,h,w] or None): every label of all_regimes(kind) owns at least one tile of image 0;
    later images are other draws of the same plan."""
    h, w = (h, w) if h else FIELD_SHAPE
    assert (h, w) == FIELD_SHAPE, "the plan below is laid out for FIELD_SHAPE"
    flow = np.zeros((B, 2, h, w), f32)
    depth = np.zeros((B, 1, h, w), f32) if kind == "depth" else None
    for b in range(B):
        fl = np.zeros((2, h, w), np.float64)
        # a small non-negative smooth flow: every source moves right / down by less than 1.5 px
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        ph = rng.uniform(0, 2 * np.pi, 4)
        fl[0] = 0.7 + 0.6 * np.sin(xx / 23.0 + ph[0]) * np.cos(yy / 17.0 + ph[1])
        fl[1] = 0.7 + 0.6 * np.cos(xx / 19.0 + ph[2]) * np.sin(yy / 29.0 + ph[3])
        # empty: the sources of tile (0, 0) leave the frame, nothing else moves left or up into it
        fl[0, 0:TH, 0:TW] = -500.0
        # lopsided: tile row 8 (rows 128..143) and the blocks above and below: large fx, |fy| below 2^-10 of it
        fl[0, 112:160, :] = 2.0 + rng.uniform(0, 1.5, (48, w))
        fl[1, 112:160, :] = rng.uniform(0, 1e-4, (48, w))
        for n, ty, tx in SITES:
            _site(rng, fl, n, ty * TH + 7, tx * TW + 30, dyadic)
        # the frame's last column and row: targets with L == w - 1 or T == h - 1 exactly (R == L / B == T add twice)
        for x in range(w - 4, w):
            fl[0, 40:60, x] = (w - 1) - x
        for y in range(h - 3, h):
            fl[1, y, 200:260] = (h - 1) - y
        if dyadic:
            fl = np.round(fl * 8) / 8
        flow[b] = fl.astype(f32)
        if kind == "depth":
            dp = rng.uniform(0.5, 1.0, (h, w))
            if dyadic:
                dp = np.round(dp * 16) / 16
            # weight classes (far from the sites): one block each with weights 2^-7, 2^-13 or 2^-19 of the largest (two,
            # three, four classes), every class populated, and the flows of the light pixels whole numbers so that the
            # dyadic field stays exact in fp32
            for (y0, x0, tiny) in ((32, 64 + 16, (7,)), (32, 192 + 16, (7, 13)), (96, 320 + 16, (7, 13, 19))):
                for i, k in enumerate(tiny):
                    ys, xs = slice(y0 + 3 * i, y0 + 3 * i + 2), slice(x0, x0 + 8)
                    dp[ys, xs] = 2.0 ** -k
                    flow[b, :, ys, xs] = np.round(flow[b, :, ys, xs])
            # negative weights (DepthFlowProjection takes the weight as given)
            dp[100:104, 520:530] = -0.25
            depth[b, 0] = dp.astype(f32)
    return flow, depth
