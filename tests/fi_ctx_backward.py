"""Host mirror, exact restatement and field builder for vfi_filterinterp_backward_ori_image_multi (filterinterp_ctx_bwd.h; the float32 unit filterinterp_ctx_bwd.hip):
the image gradient of FilterInterpolation `_ori` summed over several flows, the backward of the context warp.

  channels(n) / channel_groups(...)   the staged kernel's per-tile decision and the launcher's channel groups, as written in the source
  tiles(flows, channel)               per (b, tile row, tile column) the UNION box of the taps of all flows one launch carries, the
                                      channels per pass, and labels (below)
  predict(flows, gouts, filt)         the gradient bit for bit: one scale for the call (tests/bwd_tiles.grad_scale over every
                                      gradient, taps = filter channels x flows), the per-flow integer sums of tests/bwd_tiles added
                                      up, converted once and written (overwrite)
  build_field(rng, B, h, w, nflows)   flows in which every reachable label owns a tile in every batch item

Labels: "empty" (no valid pixel under any flow), "pc<k>" (k channels per pass, k = CB_CH .. 1), "short_pass" (a channel
group whose size is no multiple of the pass), "flag_window" (the union box does not fit one channel: the per-tap kernel
takes the tile), "flag_call" (the call scatters in fp32 or needs the second scale factor: every tile flagged),
"union_sides" (the union box's left side comes from one flow alone and its right side from another alone), "one_flow"
(several flows, exactly one with a valid pixel in the tile), and the six edge / ragged labels of bwd_tiles.EDGE_LABELS.
Unreachable with one flow: "union_sides", "one_flow".  Every constant is read from the source's #defines."""
import numpy as np

from oracle.np_oracle import _fi_geometry
from tests import bwd_tiles as bt

f32 = np.float32
SRC = "filterinterp_ctx_bwd.h"              # the kernels and the launcher, templates on the gradients' storage
UNIT = "filterinterp_ctx_bwd.hip"           # their float32 instances; restates the tile constants (read here, as ever)
CB_TW, CB_TH, CB_THREADS, CB_CH, CB_CELLS, CB_NT = (bt.constants(UNIT)[n] for n in
                                                     ("CB_TW", "CB_TH", "CB_THREADS", "CB_CH", "CB_CELLS", "CB_NT"))
FLOW_LABELS = ("union_sides", "one_flow")


# ------------------------------------------------------------------ decisions (as written in the source)

def channels(n):
    """const int pc = min(CB_CH, CB_CELLS / n);  0: the tile is flagged"""
    return min(CB_CH, CB_CELLS // n)


def channel_groups(B, C, h, w, cu=bt.CU_COUNT):
    """(ch_per_group, groups) of the staged launch"""
    ntiles = -(-w // CB_TW) * -(-h // CB_TH) * B
    slots = cu * 2
    groups = 1
    while groups < 8 and ntiles * groups < 2 * slots and C // (groups * 2) >= 4 * CB_CH and B * groups * 2 <= 65535:
        groups *= 2
    per = -(-(-(-C // groups)) // CB_CH) * CB_CH
    return per, -(-C // per)


def pass_labels():
    return tuple("pc%d" % k for k in range(CB_CH, 0, -1))


def all_labels(nflows):
    """the labels a field of nflows flows must cover"""
    return ("empty",) + pass_labels() + ("short_pass", "flag_window") + (FLOW_LABELS if nflows > 1 else ()) + bt.EDGE_LABELS


def tiles(flows, channel, finite_call=True, scale2_one=True):
    """Per (b, ty, tx) {'box', 'boxes', 'n', 'pc', 'labels'} for the flows [B, 2, h, w] of ONE launch (at most CB_NT)."""
    assert 1 <= len(flows) <= CB_NT
    B, _, h, w = flows[0].shape
    staged_ok = finite_call and scale2_one
    groups = channel_groups(B, channel, h, w)
    per_flow = []
    for flow in flows:
        valid, _, _, _, _, _, _, L, T = _fi_geometry(flow.astype(f32), h, w, 4)
        per_flow.append([bt._boxes(valid[b], np.clip(L[b], 0, w - 1), np.clip(T[b], 0, h - 1), np.clip(L[b] + 3, 0, w - 1),
                                   np.clip(T[b] + 3, 0, h - 1), CB_TH, CB_TW) for b in range(B)])
    out = {}
    for b in range(B):
        for key in per_flow[0][b]:
            boxes = [pf[b][key] for pf in per_flow]
            live = [bx for bx in boxes if bx is not None]
            rec = {"boxes": boxes, "groups": groups}
            if not live:
                rec["box"], rec["labels"] = None, {"empty"}
            else:
                box = (min(bx[0] for bx in live), min(bx[1] for bx in live), max(bx[2] for bx in live), max(bx[3] for bx in live))
                n = (box[2] - box[0] + 1) * (box[3] - box[1] + 1)
                pc = channels(n)
                rec["box"], rec["n"], rec["pc"] = box, n, pc
                if pc == 0 or not staged_ok:
                    rec["labels"] = {"flag_window" if pc == 0 else "flag_call"}
                else:
                    rec["labels"] = {"pc%d" % pc} | ({"short_pass"} if bt._short(channel, pc, groups) else set())
                if len(flows) > 1 and len(live) == 1:
                    rec["labels"].add("one_flow")
                left = [t for t, bx in enumerate(boxes) if bx is not None and bx[0] == box[0]]
                right = [t for t, bx in enumerate(boxes) if bx is not None and bx[2] == box[2]]
                if len(left) == 1 and len(right) == 1 and left != right:
                    rec["labels"].add("union_sides")
                rec["labels"] |= bt._edge_labels(box, h, w, key[0], key[1], CB_TH, CB_TW)
            out[(b,) + key] = rec
    return out


# ------------------------------------------------------------------ the restatement

def integer_sums(flow, gout, k_scale, filt):
    """[B, C, h, w] int64 sums of one flow's rounded addends; 16 filter channels: bwd_tiles.integer_sums("ori"); any other
    filter size: window_sums"""
    if filt.shape[1] == 16:
        return bt.integer_sums("ori", flow, gout, k_scale, filt)
    return window_sums(flow, gout, k_scale, filt, int(np.sqrt(f32(filt.shape[1]))))


def window_sums(flow, gout, k_scale, filt, fs):
    """the same addends over an fs x fs window (the quadrant of a tap as the forward picks it: below / right of (ix, iy))"""
    B, C, h, w = gout.shape
    scale, scale2 = k_scale
    one = f32(1)
    gout = gout.astype(f32)
    sums = np.zeros((B, C, h * w), np.int64)
    valid, _, _, ix, iy, alpha, beta, L, T = _fi_geometry(flow.astype(f32), h, w, fs)
    for b in range(B):
        for c in range(C):
            g = gout[b, c]
            qg = ((g * (one - alpha[b])) * (one - beta[b]), (g * alpha[b]) * (one - beta[b]),
                  (g * (one - alpha[b])) * beta[b], (g * alpha[b]) * beta[b])
            for dj in range(fs):
                cy = np.clip(T[b] + dj, 0, h - 1).astype(np.int64)
                for di in range(fs):
                    cx = np.clip(L[b] + di, 0, w - 1).astype(np.int64)
                    quad = (T[b] + dj > iy[b]).astype(int) * 2 + (L[b] + di > ix[b]).astype(int)
                    v = np.choose(quad, qg).astype(f32) * filt[b, dj * fs + di].astype(f32)
                    bt._scatter(sums, b, c, cy, cx, bt._round(v, scale, scale2), valid[b], w)
    return sums.reshape(B, C, h, w)


def call_scale(gouts, filt, h, w):
    """(k, fp32 path, scale, scale2) of a call: the maxima over every gradient and the filter, taps = filter channels x flows"""
    return bt.grad_scale(np.stack(gouts), filt, h, w, max(filt.shape[1], 4) * len(gouts))


def predict(flows, gouts, filt):
    """(gradinput1, k, fp32 path); the gradient is None on the fp32 path (the atomic order is free)"""
    B, C, h, w = gouts[0].shape
    k, fp32, scale, scale2 = call_scale(gouts, filt, h, w)
    if fp32:
        return None, k, True
    sums = np.zeros((B, C, h, w), np.int64)
    for flow, gout in zip(flows, gouts):
        sums += integer_sums(flow, gout, (scale, scale2), filt)
    return bt.convert(sums, k, overwrite=True), k, False


# ------------------------------------------------------------------ field builder

def _box_sizes():
    """per channels-per-pass value k (and 0: flagged) a box (bw, bh) whose cell count lies mid-way inside k's range"""
    cands = [(bw, bh) for bw in (70, 100, 170) for bh in range(12, 27)]
    out = {0: (164, 38)}
    assert channels(164 * 38) == 0, "the flagged recipe's box must not fit one channel"
    for k in range(CB_CH, 0, -1):
        lo, hi = CB_CELLS // (k + 1), CB_CELLS // k              # lo < n <= hi  <=>  channels(n) == k (k < CB_CH); k == CB_CH: n <= hi
        mid = (max(lo, 12 * 70) + hi) / 2.0
        fit = [c for c in cands if channels(c[0] * c[1]) == k]
        assert fit, "no candidate box for %d channels per pass" % k
        out[k] = min(fit, key=lambda c: abs(c[0] * c[1] - mid))
    return out


def _stretch(flows, b, ty, tx, bw, bh, h, w):
    """every flow sends the tile's pixels onto a box of exactly bw x bh cells around the tile: the column decides the
    position (x stretched, y sheared), so every row spans the box; flow t lands t/16 of a pixel further (the same cells)"""
    y0, x0 = ty * CB_TH, tx * CB_TW
    X0 = min(max(x0 + CB_TW // 2 - bw // 2, 0), w - bw)
    Y0 = min(max(y0 + CB_TH // 2 - bh // 2, 0), h - bh)
    ys, xs = np.mgrid[y0:min(y0 + CB_TH, h), x0:min(x0 + CB_TW, w)]
    u = (xs - x0) / float(CB_TW - 1)
    ixs = X0 + 1 + np.rint(u * (bw - 4)).astype(np.int64)
    iys = Y0 + 1 + np.rint(u * (bh - 4)).astype(np.int64)
    frac = ((xs + 2 * ys) % 4) / 4.0
    for t, flow in enumerate(flows):
        jit = (t % 4) / 16.0
        flow[b, 0, ys, xs] = (ixs + frac + jit - xs).astype(f32)
        flow[b, 1, ys, xs] = (iys + (0.75 - frac) + jit - ys).astype(f32)


def build_field(rng, B, h=43, w=200, nflows=1):
    """flows: nflows arrays [B, 2, h, w].  Every tile starts from a small sub-pixel flow (each flow its own); one tile per
    recipe then gets it: an empty tile, one box per channels-per-pass value and a flagged one (all flows on the same
    cells), a tile whose flows 0 and 1 move left and right (the union's sides), a tile valid in one flow only.  The recipes
    sit on interior tile columns and swap columns from one batch item to the next.  Edge labels come from the frame's border
    tiles; h % 8 <= 4 and w % 64 != 0 make the last tile row and column ragged."""
    assert CB_CH <= 6 and h >= 40 and w >= 200 and -(-h // CB_TH) >= 6, "the recipes' slots are laid out for these"
    flows = [(np.round(rng.uniform(-0.45, 0.45, (B, 2, h, w)) * 16) / 16).astype(f32) for _ in range(nflows)]
    sizes = _box_sizes()
    for b in range(B):
        s = b % 2
        slots = {0: (2, 1 + s), 1: (3, 2 - s), 2: (1, 1 + s), 3: (4, 2 - s), 4: (1, 2 - s), 5: (3, 1 + s), 6: (4, 1 + s)}
        for k, (bw, bh) in sizes.items():
            _stretch(flows, b, slots[k][0], slots[k][1], bw, bh, h, w)

        def tile(ty, tx):
            return slice(ty * CB_TH, min((ty + 1) * CB_TH, h)), slice(tx * CB_TW, min((tx + 1) * CB_TW, w))
        sl = tile(2 + s, 0)                                  # empty
        for flow in flows:
            flow[b, 0][sl] = f32(10 * w)
        sl = tile(0, 1 + s)                                  # union_sides: flow 0 to the left, flow 1 to the right
        for t, flow in enumerate(flows[:2]):
            flow[b, 0][sl] += f32(-6 if t == 0 else 6)
        sl = tile(0, 2 - s)                                  # one_flow
        for t, flow in enumerate(flows):
            if t != b % nflows:
                flow[b, 0][sl] = f32(10 * w)
    return flows
