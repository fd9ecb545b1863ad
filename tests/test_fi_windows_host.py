"""CPU checks of tests/fi_windows.py, the host mirror of the staged FilterInterpolation kernels' per-tile window
choice: its ladders are the ones the sources instantiate, its hand-worked cases hold, and the fields it builds send
every class through at least one tile (the GPU file tests/test_gpu_fi_windows.py runs those fields)."""
import numpy as np
import pytest

from tests import fi_windows as fw

CHAINS = [("lds", "FI_RUN"), ("n", "FN_RUN"), ("f16", "FI16_LADDER"), ("multi", "FM_RUN_PLAIN"), ("defor", "DF_RUN")]
# where a kernel's ladder and launch plan live, when not in its own unit
SHARED = {"f16": fw.FAMILY16}


@pytest.mark.parametrize("kernel,macro", CHAINS)
def test_rung_lists_match_the_sources(kernel, macro):
    """Adding, removing or moving a rung in a kernel fails here until the mirror follows."""
    got = fw.source_chain(SHARED.get(kernel, fw.SOURCES[kernel]), macro)
    assert all(var in (None, "kmax") for var, _, _, _ in got), got
    assert [(op, b, args[0]) for _, op, b, args in got] == fw.rungs(kernel)
    assert got[-1][1] is None and all(op is not None for _, op, _, _ in got[:-1])


def test_lds_staging_and_read_width_conditions_match_the_source():
    name = fw.SOURCES["lds"]
    d = fw.defines(name)
    got = fw.source_chain(name, "FI_RUN16")
    assert all(var in (None, "k16") for var, _, _, _ in got)
    assert [(op, b, args[0]) for _, op, b, args in got] == fw.RUNGS16
    assert fw._eval(fw.source_expr(name, r"if \(can16 && k16 <= ([^)]*)\)"), d) == fw.D16_MAX
    # the 8-byte instances exist for K <= 10 FI_KS, and fits64 keeps use64 tiles inside them
    assert fw._eval(fw.source_expr(name, r"if constexpr \(\(K\) <= ([^)]*)\)"), d) == fw.B64_KMAX_MUL * d["FI_KS"]
    assert fw._eval(fw.source_expr(name, r"fits64 = [^;]*<= ([^;]*) \* FI_THREADS;"), d) == fw.B64_KMAX_MUL * d["FI_KS"]
    assert fw.source_expr(name, r"const bool can16 = ([^;]*);") == "lean && aligned16 && any_valid && box[0] >= 0 && box[2] < w"
    assert fw.source_expr(name, r"const int lo = ([^;]*);") == "can16 ? (box[0] & ~3) : box[0]"
    assert fw.source_expr(name, r"const bool use64 = ([^;]*);") == \
        "lean && fits64 && (raw_bh >= FI_B64_MIN_BH || raw_bw >= FI_B64_MIN_BW)"
    assert fw.source_expr(name, r"const int pitch = ([^;]*);") == \
        "use64 ? (((bw + 31) >> 6) << 6) + FI_B64_PITCH_SKEW : fi_pitch_for(bw)"


def test_shared_window_classes_match_the_source():
    name = fw.SOURCES["multi"]
    got = fw.source_chain(name, "FM_RUN")
    assert all(var in (None, "rows8") for var, _, _, _ in got)
    # the segs == 3 block first, then the segs == 4 one
    assert "if (segs == 3) {" in " ".join(fw._dispatch_text(name).split())
    assert [(op, b, args) for _, op, b, args in got] == [(op, b, c) for _, (op, b), c in fw.PAIRED]
    assert [s for s, _, _ in fw.PAIRED] == sorted(s for s, _, _ in fw.PAIRED)
    assert fw.source_expr(name, r"const bool paired = ([^;]*);") == fw.PAIRED_COND
    assert fw.source_expr(name, r"const int segs = ([^;]*);") == "max(3, (bwp + 31) >> 5)"
    assert fw.source_expr(name, r"const int rows8 = ([^;]*);") == "max(3, (bh + 7) >> 3)"


def test_channel_split_arguments_match_the_sources():
    for kernel, expr in fw.SPLIT_PROLOGUE.items():
        assert fw.source_expr(SHARED.get(kernel, fw.SOURCES[kernel]), r"fi_channel_split\(ntiles, channel, (.*?)\);") == expr, kernel
    # the blend epilogue keeps the channels in one workgroup
    assert "blend.out ? FiSplit{channel, 1}" in fw.source(fw.SOURCES["blend"])
    # a frame of the GPU file's channel-split case: more than one group, and a short last one
    cpg, groups = fw.fi_channel_split(2 * 8 * 6, 196, fw.split_prologue("lds"), 256)
    assert groups > 1 and 196 % cpg != 0


def test_constants_come_from_each_translation_unit():
    assert fw.defines(fw.SOURCES["f16"])["FI_PITCH_SKEW"] == 16 and fw.defines("filterinterp_bf16.hip")["FI_PITCH_SKEW"] == 16
    assert fw.FAMILY16 in fw.includes(fw.SOURCES["f16"]) and fw.FAMILY16 in fw.includes("filterinterp_bf16.hip")
    assert fw.defines(fw.SOURCES["lds"])["FI_PITCH_SKEW"] == 0
    d = fw.defines(fw.SOURCES["lds"])
    assert d["FI_THREADS"] == d["FI_TW"] * d["FI_TH"] // d["FI_PX"] and d["FI_KTOP"] == 15 * d["FI_KS"]
    assert fw.geometry("defor", 6)[3:] == (-2, 6) and fw.geometry("n", 2)[3:] == (0, 2)


def _lds_tile(flow, h, w, ty, tx, aligned=True):
    x0, y0, x1, y1, anyv = fw.tile_boxes("lds", flow, h, w)
    info = {}
    names, _ = fw.decide("lds", x0[0, ty, tx], y0[0, ty, tx], x1[0, ty, tx], y1[0, ty, tx], anyv[0, ty, tx], h, w, aligned,
                         detail=info)
    return str(names), {k: v.item() for k, v in info.items()}


def test_hand_worked_cases():
    h, w = 64, 256
    flow = np.zeros((1, 2, h, w), np.float32)
    # zero flow, interior tile (1, 1) of an aligned frame: taps of columns 63 .. 129, rows 15 .. 33
    label, t = _lds_tile(flow, h, w, 1, 1)
    assert (t["raw_bw"], t["raw_bh"]) == (67, 19)
    assert t["can16"] and t["bx0"] == 64 - 4 and t["bw"] == 70 and t["pitch"] == 96 and t["n"] == 1824
    assert t["kmax"] == 4 and t["k16"] == 1 and not t["use64"] and label == "d16 k16=1"
    # the same tile unaligned: 4-byte staging from column 63, pitch 96, kmax 4
    label, t = _lds_tile(flow, h, w, 1, 1, aligned=False)
    assert t["bx0"] == 63 and t["pitch"] == 96 and label == "K=4"
    # one pixel of the tile's last row (31) 15 rows down: rows 15 .. 48, raw_bh 34, the 8-byte reads switch on
    f = flow.copy()
    f[0, 1, 31, 100] = 15.0
    label, t = _lds_tile(f, h, w, 1, 1)
    assert t["raw_bh"] == 34 and t["fits64"] and t["use64"] and t["pitch"] == 96 and label == "d16 k16=2 b64"
    f[0, 1, 31, 100] = 14.0
    label, t = _lds_tile(f, h, w, 1, 1)
    assert t["raw_bh"] == 33 and not t["use64"]
    # right edge tile (1, 3): the pixel of column 255 taps up to 257; without it the box ends at 256, one column past
    # the frame: can16 off; without column 254 as well it ends at 255 and can16 holds
    f = flow.copy()
    f[0, 0, 16:32, 255] = 1000.0
    label, t = _lds_tile(f, h, w, 1, 3)
    assert not t["can16"] and label.startswith("K=")
    f[0, 0, 16:32, 254] = 1000.0
    label, t = _lds_tile(f, h, w, 1, 3)
    assert t["can16"] and label.startswith("d16")
    # no valid pixel
    f[0, 0, 16:32] = 1000.0
    assert _lds_tile(f, h, w, 1, 1)[0] == "none"


def _field_cases():
    out = [("lds", 4, True), ("lds", 4, False), ("blend", 4, True), ("f16", 4, True), ("multi", 4, True)]
    out += [("n", fs, True) for fs in (2, 5, 6)] + [("defor", fs, True) for fs in (4, 6)]
    return out


@pytest.mark.parametrize("kernel,fs,aligned", _field_cases())
def test_built_fields_cover_every_class(kernel, fs, aligned):
    """Every class of the kernel's table owns a tile of each batch item, every tile lands where the builder aimed it,
    and the two items lay the classes out differently.  (The deformable variants share one geometry: the box does not
    depend on the variant.)"""
    h, w = fw.field_shape(kernel, aligned)
    f = fw.build_field(kernel, np.random.default_rng(7), 2, h, w, aligned, fs)
    lab = fw.classes(kernel, f["flow"], h, w, aligned, fs, f.get("flow2"), f.get("off"))
    want = fw.all_classes(kernel, aligned)
    for b in range(2):
        missing = [c for c in want if c not in set(lab[b].ravel())]
        assert not missing, "%s fs=%d item %d misses %s" % (kernel, fs, b, missing)
        wrong = [(t, p[0], lab[b][t]) for t, p in f["plan"][b].items() if p[0] is not None and p[0] != lab[b][t]]
        assert not wrong, wrong
    assert not np.array_equal(lab[0], lab[1])
    assert set(lab.ravel()) <= set(want)
    # boxes across every edge a tap window can cross (clamped reads), in each batch item
    x0, y0, x1, y1, anyv = fw.tile_boxes(kernel, f["flow"], h, w, fs, f.get("flow2"), f.get("off"))
    xlo, ylo, xhi, yhi = fw._box_range(kernel, h, w, fs)
    for b in range(2):
        v = anyv[b]
        crossed = {"left": (x0[b][v] == xlo).any() and xlo < 0, "right": (x1[b][v] == xhi).any() and xhi > w - 1,
                   "top": (y0[b][v] == ylo).any() and ylo < 0, "bottom": (y1[b][v] == yhi).any() and yhi > h - 1}
        assert all(crossed[e] for e in fw.EDGES[1:] if fw._edge_ok(kernel, e, h, w, fs)), (b, crossed)
    if kernel == "lds":
        # 8-byte tiles see window origins of both parities (px.odd)
        valid, ix, _, _, _ = fw.samples(f["flow"], h, w)
        b64 = np.char.endswith(fw.pixel_labels(kernel, lab, h, w).astype(str), "b64") & valid
        assert b64.any() and set(np.unique((ix[b64] - 1) & 1)) == {0, 1}


def test_shared_window_union_can_be_plain_where_one_flow_is_paired():
    h, w = fw.field_shape("multi")
    f = fw.build_field("multi", np.random.default_rng(7), 2, h, w)
    union = fw.classes("multi", f["flow"], h, w, flow2=f["flow2"])
    alone = fw.classes("multi", f["flow"], h, w, flow2=f["flow"])
    both = np.char.startswith(union.astype(str), "plain") & np.char.startswith(alone.astype(str), "paired")
    assert both.any()


def test_random_boxes_never_reach_an_uncompiled_instance():
    """use64 with K > 10 FI_KS would run no channel loop at all: fits64 must exclude it for every box."""
    rng = np.random.default_rng(3)
    n = 200000
    x0 = rng.integers(-1, 2000, n)
    y0 = rng.integers(-1, 1000, n)
    bw, bh = rng.integers(4, 400, n), rng.integers(4, 200, n)
    for aligned in (True, False):
        names, _ = fw.decide("lds", x0, y0, x0 + bw - 1, y0 + bh - 1, np.ones(n, bool), 1080, 1920, aligned)
        assert not any("UNCOMPILED" in s for s in set(names))


def test_non_finite_flows_are_invalid_pixels_that_add_nothing_to_the_box():
    """A NaN, infinite or huge flow fails fi_valid (every comparison with NaN is false, |inf| < w/2 is false): the pixel is
    copied through and its tile's box is that of the other pixels -- the mirror's, as the kernels' (tests/forward_edges.py
    plants such flows)."""
    h, w = 16, 64
    flow = np.full((1, 2, h, w), 0.5, np.float32)
    base = fw.tile_boxes("lds", flow, h, w)
    f2 = flow.copy()
    for k, v in enumerate((np.nan, -np.nan, np.inf, -np.inf, 3e38, -3e38)):
        f2[0, k % 2, 3, 5 + 4 * k] = v
    valid0 = fw.samples(flow, h, w)[0]
    valid, ix, iy, _, _ = fw.samples(f2, h, w)
    assert (valid0 & ~valid).sum() == 6 and not (valid & ~valid0).any()
    assert (ix[~valid] == 0).all() and (iy[~valid] == 0).all()
    for a, b in zip(base, fw.tile_boxes("lds", f2, h, w)):
        assert np.array_equal(a, b)
    assert np.array_equal(fw.classes("lds", flow, h, w), fw.classes("lds", f2, h, w))
    # -0.0 stays valid everywhere; the largest negative subnormal only leaves the frame from column 0
    f3 = flow.copy()
    f3[0, 0, 2, 0], f3[0, 0, 2, 7], f3[0, 0, 4, 0] = -2.0 ** -149, -2.0 ** -149, -0.0
    v3 = fw.samples(f3, h, w)[0]
    assert not v3[0, 2, 0] and v3[0, 2, 7] and v3[0, 4, 0]
