"""The planted inputs of tests/side_ops.py against the oracle alone (no GPU): every plant still decides what it was planted
to decide, every class the GPU tests rely on occurs, and the kernels still have the structure the plants were designed
for (source pins, in the manner of tests/test_bwd_tiles_host.py).  tests/test_gpu_side_ops.py runs the same inputs through
the HIP kernels and compares with the same oracle calls, bit for bit.
"""
import os
import re

import numpy as np
import pytest

from tests import forward_edges as fe
from tests import side_ops as so

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "video-frame-interpolation-based-on-deformable-kernel-region_amd", "csrc")
NONFINITE_CAP = 0.10


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------ Interpolation

def test_interp_border_plants_decide(oracle):
    """The oracle gives 0 / the cell / the cell ... exactly as the plants list them, at fmad 0 and 1 (every product is exact)."""
    img, flow, expect = so.interp_border()
    want = so.interp_border_expected(img, expect)
    assert sum(cell is None for *_, cell in expect) == 4 and len(expect) == 12
    for fmad in (0, 1):
        out = oracle.interp_fwd(img, flow, fmad=fmad)
        assert so.same_bits_nan_aware(out, want), so.describe_difference(out, want)
    for what, y, x, cell in expect:                         # the result names the cell: no other cell holds that value
        if cell is not None:
            assert (img == img[0, 0, cell[0], cell[1]]).sum() == 1
    # a kernel that flushed the subnormal would call the invalid pixel valid: the two answers differ
    assert want[0, 0, 3, 0] == 0 and img[0, 0, 3, 0] != 0


@pytest.mark.parametrize("C", [2, 3])
def test_small_interp_inputs_reach_nonfinite_outputs(oracle, C):
    img, flow = fe.small_interp_inputs(np.random.default_rng([so.SEED, 1, C]), B=2, C=C)
    out = oracle.interp_fwd(img, flow, fmad=1)
    assert np.isnan(out).any() and np.isinf(out).any() and np.isfinite(out).mean() >= 0.9
    assert (~np.isfinite(flow)).any()


# ------------------------------------------------------------------ SeparableConv

def test_sep_shapes_cover_the_tail_and_the_block():
    shapes = so.sep_shapes()
    assert {s[0] for s in shapes} == {1, 2, 4, 5, 7} and {s[1] for s in shapes} == {7, 8, 9, 16, 17}
    assert len(shapes) == 25 and len(set(shapes)) == 25
    assert {C % 3 for C, *_ in shapes} == {1, 2} and any(3 < C < 6 for C, *_ in shapes) and any(C > 6 for C, *_ in shapes)
    assert {(fs // 8, fs % 8 > 0) for _, fs, _, _ in shapes} == {(0, True), (1, False), (1, True), (2, False), (2, True)}
    for C, fs, oh, ow in shapes:
        assert oh <= 20 and ow <= 66 and ow % 64 != 0
    assert any(ow > 64 for *_, ow in shapes) and any(oh > 4 for *_, oh, _ in shapes)       # more than one 64 x 4 block


def test_sep_dyadic_sums_are_exact(oracle):
    """The largest shape: the fp32 results equal the float64 sums of the same products (so any order gives the same bits)."""
    C, fs, oh, ow = 7, 17, 9, 63
    d = so.sep_dyadic(C, fs, oh, ow)
    out = oracle.sepconv_fwd(d["img"], d["v"], d["h"], fmad=1)
    img, v, h = (d[k].astype(np.float64) for k in ("img", "v", "h"))
    want = np.zeros(out.shape)
    for fy in range(fs):
        for fx in range(fs):
            want += img[:, :, fy:fy + oh, fx:fx + ow] * v[:, None, fy] * h[:, None, fx]
    assert np.array_equal(out.astype(np.float64), want)
    assert np.array_equal(out, oracle.sepconv_fwd(d["img"], d["v"], d["h"], fmad=0))


@pytest.mark.parametrize("fs", so.SEP_PLANT_SIZES)
def test_sep_planted_outputs(oracle, fs):
    """At most 10 % of every output tensor is non-finite and each of NaN, +inf and -inf occurs in it."""
    d = so.sep_planted(fs)
    assert len(d["planted"]) == 3 * len(so.SEP_PLANT_SET)
    for where, name, at in d["planted"]:                    # no plant overwrote another
        got, want = d[where][at], dict(so.SEP_PLANT_SET)[name]
        assert so.bits(np.array([got]))[0] == so.bits(np.array([want]))[0] or (np.isnan(got) and np.isnan(want)), (where, name)
    out = oracle.sepconv_fwd(d["img"], d["v"], d["h"], fmad=1)
    start = tuple(so.pattern(d[k].shape, n) for n, k in enumerate(("img", "v", "h")))
    grads = oracle.sepconv_bwd(d["img"], d["v"], d["h"], d["gout"], start=start)
    for key, a in zip(("out", "gimg", "gv", "gh"), (out,) + grads):
        share, nan, pinf, ninf = so.nonfinite_census(a)
        assert share <= NONFINITE_CAP and nan and pinf and ninf, (fs, key, share, nan, pinf, ninf)


def test_sep_backward_adds_into_what_the_gradients_hold(oracle):
    """The oracle's C function accumulates into the arrays it is handed: on dyadic inputs, start + the zero-start result."""
    d = so.sep_dyadic(4, 9, 5, 37)
    start = tuple(so.pattern(d[k].shape, n) for n, k in enumerate(("img", "v", "h")))
    zero = oracle.sepconv_bwd(d["img"], d["v"], d["h"], d["gout"])
    got = oracle.sepconv_bwd(d["img"], d["v"], d["h"], d["gout"], start=start)
    for s, z, g in zip(start, zero, got):
        assert (s != 0).all() and np.array_equal(g, s + z) and not np.array_equal(g, z)


# ------------------------------------------------------------------ SeparableConvFlow

def test_sepflow_vectors_give_the_listed_flows(oracle):
    d = so.sepflow_planted()
    H, W = d["img"].shape[2:]
    for fmad in (0, 1):
        fl = oracle.sepconvflow_fwd(d["v"], d["h"], H, W, fmad=fmad)
        for x, want in so.sepflow_expected():
            for got in (fl[:, 1, so.SEPFLOW_ROW_V, x], fl[:, 0, so.SEPFLOW_ROW_H, x]):
                assert np.isnan(got).all() if np.isnan(want) else (got == f32(want)).all(), (x, want, got)
        # the pixel that carries both: y from v's vector, x from h's
        xb = so.sepflow_x(so.SEPFLOW_BOTH)
        assert np.isnan(fl[:, 1, so.SEPFLOW_ROW_V, xb]).all() and (fl[:, 0, so.SEPFLOW_ROW_V, xb] == -2.0).all()
        for axis in (0, 1):                                 # {-2000, finite, NaN} on both axes
            a = fl[:, axis]
            assert (a == -2000.0).any() and np.isnan(a).any() and (np.isfinite(a) & (a != -2000.0)).any()
        # the undecided pixels are the planted ones alone
        assert (fl == -2000.0).sum() == 2 * 2 * sum(w == -2000.0 for *_, w in so.SEPFLOW_VECTORS)
    assert [w for *_, w in so.SEPFLOW_VECTORS][:4] == [-2000.0, -2000.0, -2.0, 2.0]


def test_sepflow_backward_situations(oracle):
    """gradinput2: the stored value where |sum_v| > 0, the pattern untouched elsewhere; gradinput3: pattern + term where
    |sum_h| > 0, the pattern elsewhere -- all four occur, and the rows of gradinput2 hold 0, NaN, -inf and mixtures."""
    d = so.sepflow_planted()
    H, W = d["img"].shape[2:]
    fl = oracle.sepconvflow_fwd(d["v"], d["h"], H, W, fmad=1)
    start = (so.pattern(d["v"].shape, 1), so.pattern(d["h"].shape, 2))
    gv, gh = oracle.sepconvflow_bwd(d["v"], d["h"], d["gflow"], H, W, fmad=1, start=start)
    zv, zh = oracle.sepconvflow_bwd(d["v"], d["h"], d["gflow"], H, W, fmad=1)
    dec_v = np.broadcast_to((fl[:, 1:2] != -2000.0), gv.shape)         # (a NaN flow is a decided one)
    dec_h = np.broadcast_to((fl[:, 0:1] != -2000.0), gh.shape)
    assert dec_v.any() and (~dec_v).any() and dec_h.any() and (~dec_h).any()
    assert np.array_equal(so.bits(gv)[~dec_v], so.bits(start[0])[~dec_v])                  # untouched
    assert so.same_bits_nan_aware(gv[dec_v], zv[dec_v]) and (gv[dec_v] != start[0][dec_v]).any()   # stored, whatever it held
    assert np.array_equal(so.bits(gh)[~dec_h], so.bits(start[1])[~dec_h])
    fin = dec_h & np.isfinite(gh) & np.isfinite(zh)
    assert fin.any() and (gh[fin] != zh[fin]).any() and (gh[fin] != start[1][fin]).any()  # added
    row = gv[:, :, so.SEPFLOW_ROW_V, [x for x, _ in so.sepflow_expected()]]
    assert np.isnan(row).any() and (row == 0).any() and np.isinf(row).any()


@pytest.mark.parametrize("fs", [1, 2, 5, 51])
def test_sepflow_finite_inputs_have_decided_and_undecided_pixels(oracle, fs):
    d = so.sepflow_finite(fs)
    oh, ow = d["v"].shape[2:]
    fl = oracle.sepconvflow_fwd(d["v"], d["h"], oh + fs - 1, ow + fs - 1, fmad=1)
    assert oh <= 20 and ow <= 66 and np.isfinite(fl).all()
    for axis in (0, 1):
        assert (fl[:, axis] == -2000.0).any() and (fl[:, axis] != -2000.0).any()


# ------------------------------------------------------------------ MinDepthFlowProjection forward

@pytest.mark.parametrize("name", so.MD_TIE_NAMES)
@pytest.mark.parametrize("fillhole", [0, 1])
def test_md_zero_tie_first_source_wins(oracle, name, fillhole):
    flow, wgt, count0, expect = so.md_zero_tie(name)
    out, count = oracle.mindepthflowproj_fwd(flow, wgt, fillhole, count0=count0)
    assert (count0 < 0).all() and len(expect) == (2 if name == "item 1" else 1)
    for b, ty, tx, (sy, sx) in expect:
        assert np.array_equal(out[b, :, ty, tx], -flow[b, :, sy, sx])
        assert so.bits(count)[b, 0, ty, tx] == so.bits(wgt)[b, 0, sy, sx]
        # the other sources of the target: other flows, and a zero of the other sign among them
        others = [(y, x) for y, x in np.argwhere(flow[b, 0] != so.INVALID) if (y, x) != (sy, sx)]
        assert others and all(not np.array_equal(flow[b, :, y, x], flow[b, :, sy, sx]) for y, x in others)
        assert {int(so.bits(wgt)[b, 0, y, x]) for y, x in others + [(sy, sx)]} == {0, 0x80000000}
    untouched = np.ones(count.shape, bool)
    for b, ty, tx, _ in expect:
        untouched[b, 0, ty, tx] = False
    assert (count[untouched] == so.MD_FLOOR).all() and not out[np.broadcast_to(untouched, out.shape)].any()


def test_md_zero_tie_key_arithmetic():
    """Why the parent's keys broke the rule, and what the fixed key does: -0.0 ordered below +0.0 lets a LATER +0.0 beat an
    earlier -0.0; with both zeros on one key the larger (0xffffffff - index), the earlier source, wins."""
    def key(w, index, fold):
        u = int(so.bits(np.array([w]))[0])
        if fold and w == 0:
            u = 0
        k = (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)
        return (k << 32) | (0xffffffff - index)
    assert key(-0.0, 5, False) < key(0.0, 9, False)                         # the later source won
    assert key(-0.0, 5, True) > key(0.0, 9, True) and key(0.0, 5, True) > key(-0.0, 9, True)
    w = np.array([-np.inf, -3.0, -so.SUB, -0.0, so.SUB, 0.5, np.inf], f32)
    keys = [key(float(v), 0, True) for v in w]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)             # still the order of `<` on the values


@pytest.fixture(scope="module")
def holes(oracle):
    flow, wgt, count0, out0 = so.md_holes()
    out, count = oracle.mindepthflowproj_fwd(flow, wgt, 1, count0=count0, out0=out0)
    return dict(count0=count0, out0=out0, out=out, count=count, census=so.md_hole_census(count0))


def test_md_holes_forward_writes_nothing_and_the_filler_fills(oracle, holes):
    flow, wgt, count0, out0 = so.md_holes()
    o0, c0 = oracle.mindepthflowproj_fwd(flow, wgt, 0, count0=count0, out0=out0)
    assert so.same_bits_nan_aware(c0, count0) and np.array_equal(o0, out0)            # fillhole 0: untouched
    assert so.same_bits_nan_aware(holes["count"], count0)
    changed = so.bits(holes["out"]) != so.bits(out0)
    assert changed.sum() > 10000 and np.isnan(holes["out"]).any()
    assert not changed[np.broadcast_to(~(count0 <= 0), changed.shape)].any()         # only holes are written
    assert np.array_equal(count0[1], count0[0][..., ::-1], equal_nan=True)            # the items are mirrored
    assert len(np.unique(out0)) == out0.size and np.array_equal(out0 * 4, np.round(out0 * 4))


def test_md_holes_census(holes):
    c = holes["census"]
    B, H, W = so.MD_HOLE_SHAPE
    for k in ("left", "right"):
        assert set(so.MD_DISTANCES + so.MD_ROW_ONLY) <= c["dist"][k], (k, set(so.MD_DISTANCES + so.MD_ROW_ONLY) - c["dist"][k])
    for k in ("up", "down"):
        assert set(so.MD_DISTANCES) <= c["dist"][k], (k, set(so.MD_DISTANCES) - c["dist"][k])
    assert c["nothing"] >= {1, 2, 3, 4}
    assert c["kinds"] == {"positive", "negative", "-inf", "+inf", "nan"}
    for axis, n in (("x", W), ("y", H)):
        cells = c["cells"][axis]
        assert any(p % 32 == 0 for p in cells) and any(p % 32 == 31 for p in cells), axis
        assert n % 32 != 0 and any(p // 32 == n // 32 for p in cells), (axis, "the last, partial word")
    assert W > 5 * 32 and H > 5 * 32                        # a walk longer than one four-word group, on both axes


def test_md_holes_rule_no_result_depends_on_the_visiting_order(holes):
    assert len(so.md_hole_rule(holes["count0"])) == 0
    bad = holes["count0"].copy()
    bad[0, 0, 110, 10] = 0.5                                # a positive count in the row of the negative cell: caught
    assert len(so.md_hole_rule(bad)) > 0
    # and in the oracle's result those cells did keep their values
    c = holes["count0"][:, 0]
    keep = np.broadcast_to(((c < 0) | np.isnan(c) | (c > 0))[:, None], holes["out"].shape)
    assert np.array_equal(holes["out"][keep], holes["out0"][keep])


def test_md_walks_agree_with_a_cell_by_cell_walk():
    rng = np.random.default_rng([so.SEED, 6])
    count = (rng.random((1, 1, 9, 70)) < 0.06).astype(f32)
    w = so.md_walks(count)
    nz = count[0, 0] != 0
    for y in range(9):
        for x in range(70):
            left = [i for i in range(x - 1, -1, -1) if nz[y, i]]
            down = [j for j in range(y + 1, 9) if nz[j, x]]
            assert w["left"][0, y, x] == (left[0] if left else -1) and w["down"][0, y, x] == (down[0] if down else -1)
    f = count[:, :, ::-1, ::-1]
    wf = so.md_walks(f)
    assert np.array_equal(np.where(wf["right"] < 0, -1, 69 - wf["right"])[:, ::-1, ::-1], w["left"])
    assert np.array_equal(np.where(wf["up"] < 0, -1, 8 - wf["up"])[:, ::-1, ::-1], w["down"])


# ------------------------------------------------------------------ MinDepthFlowProjection backward

def test_md_backward_plants(oracle):
    flow, wgt, count, gout, expect = so.md_backward()
    start = so.pattern(flow.shape, 3)
    zero = oracle.mindepthflowproj_bwd(flow, wgt, count, gout)
    got = oracle.mindepthflowproj_bwd(flow, wgt, count, gout, start=start)
    assert np.array_equal(got, start + zero) and (zero != 0).sum() > 100         # the sums are exact
    hits = {what: h for what, _, _, _, h in expect}
    assert [n for *_, n in hits["last column"]] == [2] and [n for *_, n in hits["last row"]] == [2]
    assert [n for *_, n in hits["last column, both rows"]] == [2, 2] and [n for *_, n in hits["corner"]] == [4]
    assert len(hits["+0 weight, -0 count"]) == 1 and len(hits["-0 weight, +0 count"]) == 1
    assert hits["nan, nan"] == [] and len(hits["+inf, +inf"]) == 1 and len(hits["-inf, -inf"]) == 1
    what, b, y, x, h = [e for e in expect if e[0] == "neighbour only"][0]
    T, L = int(y + flow[b, 1, y, x]), int(x + flow[b, 0, y, x])
    assert len(h) == 2 and (T, L) not in [(ty, tx) for ty, tx, _ in h]
    for (b, y, x), want in so.md_backward_expected(gout, expect, start).items():
        assert np.array_equal(got[b, :, y, x], want), (b, y, x, got[b, :, y, x], want)
    assert (gout != 0).all()


# ------------------------------------------------------------------ source pins

def test_the_kernels_still_have_the_structure_the_plants_aim_at():
    ws = _src("warp_sepconv.hip")
    assert len(re.findall(r"sepconv_forward<(\d+)>", ws)) == 1 and "hipLaunchKernelGGL(sepconv_forward<3>," in ws
    assert "for (; fx + 8 <= fs; fx += 8)" in ws and "float t3[8], pv[8][CH];" in ws      # the eight-tap block
    assert "(c0 + k < channel)" in ws                                                    # the channel tail
    assert ws.count("fabsf(sum) > 0.0f") == 4                                            # SeparableConvFlow's decisions
    assert "x2 >= 0.0f && y2 >= 0.0f && x2 < (float)w && y2 < (float)h" in ws            # Interpolation's strict upper bound
    md = _src("mindepth.hip")
    assert re.search(r"#define MD_ROWS 32\b", md) and "m.cmw = (h + MD_ROWS - 1) / MD_ROWS;" in md
    assert "weight == cn[" in md and "!(weight > count[" in md
    bw = _src("bitwalk.h")
    assert "wi >= 0; wi -= 4" in bw and "wi < nw; wi += 4" in bw and bw.count("unsigned q[4];") == 2
    vc = _src("vfi_common.h")
    assert re.search(r"#define VFI_TX 64\b", vc) and re.search(r"#define VFI_TY 4\b", vc)  # the 64 x 4 blocks of "far block"


def test_cabi_wrappers_keep_the_references_refusal_by_default():
    import inspect
    try:
        from vfidkr_amd import cabi
    except Exception as e:                                  # (torch for the GPU is imported by the package)
        pytest.fail("vfidkr_amd.cabi must import without a GPU: %r" % (e,))
    for fn in (cabi.separableconv_forward, cabi.separableconv_backward, cabi.separableconvflow_forward, cabi.separableconvflow_backward):
        assert inspect.signature(fn).parameters["require_c3"].default is True
    assert inspect.signature(cabi.interpolation_forward).parameters["require_c3"].default is False
