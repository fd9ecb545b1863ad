"""Helpers of the bfloat16 context-warp tests (vfi_filterinterp_forward_ori_multi_to_bf16 and
vfi_filterinterp_backward_ori_image_multi_bf16, csrc/filterinterp_bf16.hip).  No test functions, nothing of the product imported.

  constants() / RUNGS                 the staged kernel's #defines (read from the source: the unit and filterinterp_16.h) and
                                      the mirror's own rung ladder
  takes_staged(...)                   the launcher's choice between the staged and the direct kernel, by layout
  decide(x0, y0, x1, y1, any)         the per-tile decision from the box of the moved windows: dwords per row, pitch, staged
                                      dwords, ring class ("K=2" .. "K=8", "gather", "none")
  tiles(flow, h, w)                   per (b, tile row, tile column): the ring class, and whether a valid pixel's window was moved
                                      inside the image from the left (by one column) or the right (by one, by two): the EDGE
                                      instance of the channel loop
  features(flow, h, w) / ALL_FEATURES what a field exercises: every ring class, the interior and the EDGE instance, each move,
                                      a ragged last tile column
  forward_reference(oracle, ...)      to_bf16(oracle.filterinterp_ori_fwd(widened image, flow, filter, fmad=1))
  forward_f64(...)                    the same sums in float64 after the float32 geometry, with sum |weight x tap x value|
  backward_reference(...)             to_bf16 of tests/fi_ctx_backward.predict on the widened gradients
  pipeline_spills(path)               tests/test_abi_and_host's criterion -- no scratch operation in an LDS-DMA pipeline -- applied
                                      to one assembly file

The tile geometry is the fp16 kernel's (one set of constants and one prologue, filterinterp_16.h), so fi_windows.build_field("f16", ...) builds
the all-class fields: its windows are moved inside the image exactly as this kernel's are.
"""
import re

import numpy as np

from tests import fi_ctx_backward as fc
from tests import fi_windows as fw
from tests.corr_bf16 import bits, from_bits, same_bits, to_bf16  # noqa: F401  (re-exported)
from tests.pwc_bf16 import edge_grid, guard_intact, guarded, half_ulp  # noqa: F401

SRC = "filterinterp_bf16.hip"
f32 = np.float32
# the mirror's own statement of the dispatch chain: (op, bound on kmax, K); op None = the final else
RUNGS = [("<=", 2, 2), ("==", 3, 3), ("==", 4, 4), ("<=", 6, 6), (None, None, 8)]
RING_CLASSES = ["K=%d" % k for _, _, k in RUNGS] + ["gather", "none"]
EDGE_FEATURES = ["interior", "edge left", "edge right 1", "edge right 2", "ragged last column"]
ALL_FEATURES = RING_CLASSES + EDGE_FEATURES
INT_MAX = 2 ** 31 - 1


def constants():
    d = fw.defines(SRC)
    return {k: d[k] for k in ("FI16_TW", "FI16_TH", "FI16_PX", "FI16_THREADS", "FI16_PASS_ROWS", "FI16_HDR", "FI16_RING_DWORDS",
                              "FI16_RMAX", "FI16_KTOP", "FI_PITCH_SKEW")}


def ring_geometry(K):
    """(slots R, windows in flight D) of the instance for K dwords per thread, as fi16_run_channels (filterinterp_16.h) computes them"""
    c = constants()
    R = min(c["FI16_RING_DWORDS"] // (K * c["FI16_THREADS"]), c["FI16_RMAX"])
    return R, R - 1


def takes_staged(shape, stride, data_ptr, filter_channels):
    """forward_bf16: dword staging needs fs == 4, w >= 4, even row / plane / batch strides, a 4-byte aligned base and
    in-plane byte offsets within 31 bits"""
    _, _, h, w = shape
    sb, sc, sh = stride[:3]
    return (filter_channels == 16 and w >= 4 and (sb | sc | sh) % 2 == 0 and data_ptr % 4 == 0 and h * sh * 2 < INT_MAX)


def decide(x0, y0, x1, y1, anyv):
    """arrays in; dict of arrays out: bx0 (even), bw (dwords), bh, pitch, n (staged dwords), kmax, label"""
    c = constants()
    x0, y0, x1, y1 = (np.asarray(a, np.int64) for a in (x0, y0, x1, y1))
    anyv = np.asarray(anyv, bool)
    bx0 = np.where(anyv, x0 & ~1, 0)
    bw = np.where(anyv, (x1 - bx0 + 2) >> 1, 0)
    bh = np.where(anyv, y1 - y0 + 1, 0)
    pitch = fw.pitch_for(bw, c["FI_PITCH_SKEW"])
    n = pitch * bh
    kmax = -(-n // c["FI16_THREADS"])
    K = fw._pick(RUNGS, kmax)
    label = np.where(~anyv, "none", np.where(kmax > c["FI16_KTOP"], "gather", fw._lut("K=%d")[K])).astype(object)
    return {"bx0": bx0, "bw": bw, "bh": bh, "pitch": pitch, "n": n, "kmax": kmax, "label": label}


def tiles(flow, h, w):
    """per (b, tile row, tile column): 'label' and the moves of the valid pixels' windows, 'left', 'right1', 'right2' (bool arrays)"""
    c = constants()
    th, tw = c["FI16_TH"], c["FI16_TW"]
    valid, ix, iy, _, _ = fw.samples(flow, h, w)
    L, T = ix - 1, iy - 1
    Lc = np.clip(L, 0, w - 4)
    out = decide(*fw._fold([(valid, Lc, T, Lc + 3, T + 3)], th, tw))
    shift = L - Lc
    for name, s in (("left", -1), ("right1", 1), ("right2", 2)):
        out[name] = fw.to_tiles(valid & (shift == s), th, tw, False).any(-1)
    assert not (valid & ((shift < -1) | (shift > 2))).any(), "validity bounds the move to one column left, two right"
    out["edge"] = out["left"] | out["right1"] | out["right2"]
    return out


def features(flow, h, w):
    """the members of ALL_FEATURES that at least one tile of the field exercises (the EDGE features in staged tiles only)"""
    t = tiles(flow, h, w)
    staged = np.array([str(s).startswith("K=") for s in t["label"].ravel()]).reshape(t["label"].shape)
    got = set(t["label"].ravel())
    for name, key in (("edge left", "left"), ("edge right 1", "right1"), ("edge right 2", "right2")):
        if (staged & t[key]).any():
            got.add(name)
    if (staged & ~t["edge"]).any():
        got.add("interior")
    if w % constants()["FI16_TW"] and staged[:, :, -1].any():
        got.add("ragged last column")
    return got


def pixel_labels(flow, h, w):
    """[B, h, w]: the tile's ring class, ' edge' appended where the tile runs the EDGE instance"""
    t = tiles(flow, h, w)
    c = constants()
    lab = np.where(t["edge"] & (t["label"] != "gather") & (t["label"] != "none"), t["label"] + " edge", t["label"]).astype(object)
    return np.repeat(np.repeat(lab, c["FI16_TH"], axis=1), c["FI16_TW"], axis=2)[:, :h, :w]


# ------------------------------------------------------------------ references

def forward_reference(oracle, img, flow, filt):
    """img: float32 array of bfloat16 values (the widened image).  float32 array of bfloat16 values."""
    assert np.array_equal(bits(img), bits(from_bits(bits(img)))), "the image holds bfloat16 values"
    with np.errstate(all="ignore"):
        return to_bf16(oracle.filterinterp_ori_fwd(np.ascontiguousarray(img, dtype=f32), flow, filt, fmad=1, nthreads=8))


def forward_f64(img, flow, filt):
    """(R, A): the layer in float64 after the float32 decisions (validity, cell, blend fractions), and the sum of
    |blend weight x filter tap x image value| per output; fs from the filter's channels; an invalid pixel copies (A = 0)"""
    B, C, h, w = img.shape
    fs = int(np.sqrt(f32(filt.shape[1])))
    valid, ix, iy, x2, y2 = fw.samples(flow, h, w)
    alpha = (x2 - ix.astype(f32)).astype(np.float64)
    beta = (y2 - iy.astype(f32)).astype(np.float64)
    L, T = ix + 1 - fs // 2, iy + 1 - fs // 2
    wq = [(1 - alpha) * (1 - beta), alpha * (1 - beta), (1 - alpha) * beta, alpha * beta]
    R, A = np.zeros(img.shape), np.zeros(img.shape)
    img64, filt64 = img.astype(np.float64), filt.astype(np.float64)
    bidx = np.arange(B)[:, None, None]
    for dj in range(fs):
        for di in range(fs):
            j, i = T + dj, L + di
            quad = (j > iy).astype(int) * 2 + (i > ix).astype(int)
            val = img64[bidx, :, np.clip(j, 0, h - 1), np.clip(i, 0, w - 1)].transpose(0, 3, 1, 2)
            term = (np.choose(quad, wq) * filt64[:, dj * fs + di])[:, None] * val
            R += term
            A += np.abs(term)
    v = valid[:, None]
    return np.where(v, R, img64), np.where(v, A, 0.0)


def backward_reference(flows, gouts, filt):
    """gouts: float32 arrays of bfloat16 values.  (float32 array of bfloat16 values or None on the fp32 path, k, fp32 path)"""
    want, k, fp32 = fc.predict(flows, [np.asarray(g, f32) for g in gouts], filt)
    return (None if want is None else to_bf16(want)), k, fp32


# ------------------------------------------------------------------ the assembly

def pipeline_spills(path):
    """(blocks checked, [(block label, scratch operations)]) -- the criterion of
    tests/test_abi_and_host.test_no_register_spills_inside_the_counted_vmcnt_pipelines: no scratch operation in a basic block that
    issues LDS-DMA loads (after its first such load, in straight-line code) nor in any block of a loop that does, unless every
    hand-written vmcnt wait of the loop is vmcnt(0)."""
    blocks, cur, func, in_asm = [], None, "", False
    for line in open(path):
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", line)
        if m:
            hdr = re.search(r"Header[:=]\s*(BB\d+_\d+)", m.group(2))
            cur = {"label": m.group(1)[2:], "loop": hdr.group(1) if hdr else None, "ins": [], "asm": [],
                   "is_header": "Loop Header" in m.group(2), "func": func}
            blocks.append(cur)
        elif re.match(r"^_Z\w+:", line):
            cur, func = None, line.split(":")[0]
        elif ";;#ASMSTART" in line:
            in_asm = True
        elif ";;#ASMEND" in line:
            in_asm = False
        elif cur is not None and re.match(r"^\s+[a-z]", line):
            cur["ins"].append(line.strip())
            if in_asm:
                cur["asm"].append(line.strip())
    for b in blocks:
        if b["is_header"]:
            b["loop"] = b["label"]
    for b in blocks:
        if b["loop"]:
            for k, i in enumerate(b["ins"]):
                if re.match(r"s_c?branch\w*\s+\.L" + re.escape(b["loop"]) + r"\b", i):
                    b["ins"] = b["ins"][:k + 1]
                    break
    is_dma = lambda i: i.startswith("buffer_load") and " lds" in i      # noqa: E731
    dma_loops = {b["loop"] for b in blocks if b["loop"] and any(is_dma(i) for i in b["ins"])}
    counted = set()
    for b in blocks:
        for i in b["asm"]:
            m = re.match(r"s_waitcnt vmcnt\((\d+)\)", i)
            if m and int(m.group(1)) > 0 and b["loop"]:
                counted.add(b["loop"])
    checked, bad = 0, []
    for b in blocks:
        pipelined = any(is_dma(i) for i in b["ins"]) or (b["loop"] in dma_loops)
        if not pipelined or (b["loop"] in dma_loops and b["loop"] not in counted):
            continue
        own = [re.match(r"s_waitcnt vmcnt\((\d+)\)", i) for i in b["asm"]]
        own = [int(m.group(1)) for m in own if m]
        if b["loop"] is None and own and max(own) == 0:
            continue
        checked += 1
        ins = b["ins"]
        if b["loop"] is None:
            ins = ins[next(k for k, i in enumerate(ins) if is_dma(i)):]
        spills = [i for i in ins if i.startswith("scratch_")]
        if spills:
            bad.append((b["label"], spills[:3]))
    return checked, bad, len(counted)
