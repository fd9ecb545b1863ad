"""Non-finite and extreme inputs through FilterInterpolation (staged, direct, blend, multi-flow, deformable and fp16
entries; at the end of the file), the forward projections, the PWC-Net warp and MinDepthFlowProjection
(tests/forward_edges.py plants them; tests/test_forward_edges_host.py checks the plants against the oracle alone).

What is asserted, everywhere: the result equals the oracle's NaN-aware and bit for bit -- NaN at the same elements
(payload and sign not compared), every other element, infinities and signed zeros included, with the same bits.  The
planted fields are dyadic and every planted value has its cells to itself, so the fp32 sums of the finite cells are exact
in any order and the non-finite ones are non-finite in any order: there is no tolerance to state.

Outputs are views into buffers filled with a finite sentinel, 16 floats of guard on both sides (a NaN prefill cannot
tell an unwritten element from a NaN result): every call runs with two different sentinels, the two results must be the
same, neither sentinel may survive inside the view and every guard element must still hold it.

Projections: FlowProjection and DepthFlowProjection, fillhole 0 and 1, through every (K0, K1) pair of
proj_tiles.dispatch -- proj_scan4 + proj_pull_lean (dense tensors), proj_scan4 + proj_pull<., true> (count at an odd
element offset), proj_scan + proj_pull<., false> (flow and output rows of w + 1 floats) --, the list entries with a
poisoned and a clean item, the `_up4` entries, and a clean smaller call right after each poisoned one (the fallback's
scratch planes get cleaned).  A planted DepthFlowProjection call must take the atomic fallback (proj_weight_unfit in
K0); FlowProjection has no weights and keeps its path.
"""
import numpy as np
import pytest

from tests import forward_edges as fe
from tests import proj_tiles as pt
from tests.test_gpu_parity import cpu, gpu, torch_mod, cabi  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

f32 = np.float32
SEED = 20261020
SENTINELS = (12345.678, -0.0009765)                         # finite, and no result of any planted input
GUARD = 16


# ------------------------------------------------------------------ sentinel-framed outputs

class Guarded:
    """A [shape] view `v` at float offset `off` of a flat buffer filled with `fill`; pad: extra floats per row (the view's
    rows are then w + pad apart).  ok(): no element of the view holds the sentinel, every element outside it does."""

    def __init__(self, torch, shape, fill, off=GUARD, pad=0):
        B, C, h, w = shape
        n = B * C * h * (w + pad)
        self.fill = fill
        self.flat = torch.full((n + 2 * GUARD + 1,), fill, device="cuda:0")
        self.v = self.flat[off:off + n].view(B, C, h, w + pad)[..., :w]
        self.inside = torch.zeros_like(self.flat, dtype=torch.bool)
        self.inside[off:off + n].view(B, C, h, w + pad)[..., :w] = True

    def ok(self, torch, what):
        sent = self.flat == self.fill
        assert not (sent & self.inside).any(), "%s: %d elements of the view left unwritten" % (what, int((sent & self.inside).sum()))
        assert sent[~self.inside].all(), "%s: %d elements written outside the view" % (what, int((~sent[~self.inside]).sum()))


def _same(what, got, want, m=None):
    if fe.same_bits_nan_aware(got, want):
        return
    msg = "%s: %s" % (what, fe.describe_difference(got, want))
    if m is not None:
        ng, nw = np.isnan(got), np.isnan(want)
        bad = (ng != nw) | (~ng & ~nw & (got.view(np.uint32) != want.view(np.uint32)))
        labels = m.labels()
        per = {}
        for (b, y, x) in np.argwhere(bad.any(1)):
            for lab in labels[(b, y // pt.TH, x // pt.TW)]:
                per[lab] = per.get(lab, 0) + 1
        msg += "; cells by tile label %s" % per
    pytest.fail(msg)


# ------------------------------------------------------------------ projections

@pytest.fixture(scope="module")
def planted(oracle):
    """{kind: field, planted copy, the unplanted field's mirror (for tile labels), oracle results per fillhole} -- once"""
    cache = {}

    def get(kind):
        if kind not in cache:
            rng = np.random.default_rng([SEED, kind == "depth"])
            field = pt.build_field(kind, rng, 1, dyadic=True)
            flow, depth, plist = fe.plant_proj(kind, field, rng)
            ref = {fh: (oracle.flowproj_fwd(flow, fh) if depth is None else oracle.depthflowproj_fwd(flow, depth, fh)) for fh in (0, 1)}
            rng2 = np.random.default_rng([SEED, 2, kind == "depth"])
            small = fe.clean_field(kind, rng2)
            sref = {fh: (oracle.flowproj_fwd(small[0], fh) if depth is None else oracle.depthflowproj_fwd(small[0], small[1], fh))
                    for fh in (0, 1)}
            for a in (flow, depth) + small:
                if a is not None:
                    a.setflags(write=False)
            cache[kind] = dict(field=field, flow=flow, depth=depth, planted=plist, mirror=pt.mirror(field[0], field[1], "lean"),
                               ref=ref, small=small, sref=sref)
        return cache[kind]
    return get


def _call(torch, cabi, variant, flow, depth, fillhole, fill):
    """One projection call in the layout that reaches `variant`; (out, count) as numpy."""
    B, _, h, w = flow.shape
    pad = 1 if variant == "pull_scalar" else 0
    fl = Guarded(torch, flow.shape, 0.0, pad=pad)
    fl.v.copy_(torch.from_numpy(np.ascontiguousarray(flow)))
    out = Guarded(torch, flow.shape, fill, pad=pad)
    count = Guarded(torch, (B, 1, h, w), fill, off=GUARD + (1 if variant == "pull_vec" else 0))
    dp = None if depth is None else gpu(torch, depth)
    assert pt.dispatch_of(fl.v, count.v, out.v, dp)[1] == variant
    if dp is None:
        assert cabi.flowprojection_forward(fl.v, count.v, out.v, fillhole) == 0
    else:
        assert cabi.depthflowprojection_forward(fl.v, dp, count.v, out.v, fillhole) == 0
    what = "%s fillhole %d sentinel %g" % (variant, fillhole, fill)
    out.ok(torch, what + " out")
    count.ok(torch, what + " count")
    return cpu(out.v), cpu(count.v)


@pytest.mark.parametrize("kind", ["flow", "depth"])
@pytest.mark.parametrize("variant", ["lean", "pull_vec", "pull_scalar"])
@pytest.mark.parametrize("fillhole", [0, 1])
def test_planted_projection_equals_the_oracle(torch_mod, cabi, planted, kind, variant, fillhole):
    torch = torch_mod
    p = planted(kind)
    flow, depth = p["flow"], p["depth"]
    assert pt.records(flow, depth, *flow.shape[2:])[1] == (kind == "depth"), "the planted weights send the call to the fallback"
    runs = [_call(torch, cabi, variant, flow, depth, fillhole, s) for s in SENTINELS]
    ref, rcount = p["ref"][fillhole]
    _same("count, planted %s" % kind, runs[0][1], rcount, p["mirror"])
    _same("out, planted %s" % kind, runs[0][0], ref, p["mirror"])
    _same("count, second sentinel", runs[1][1], runs[0][1])
    _same("out, second sentinel", runs[1][0], runs[0][0])
    # the next call on the stream, a clean smaller frame: bit for bit the oracle's (the fallback's scratch was cleaned)
    sflow, sdepth = p["small"]
    out, count = _call(torch, cabi, variant, sflow, sdepth, fillhole, SENTINELS[0])
    sref, scount = p["sref"][fillhole]
    assert np.isfinite(sref).all() and np.array_equal(count, scount) and np.array_equal(out, sref)


@pytest.mark.parametrize("kind", ["flow", "depth"])
@pytest.mark.parametrize("fillhole", [0, 1])
def test_batch_with_a_poisoned_and_a_clean_item(torch_mod, cabi, planted, kind, fillhole):
    """The list entries: item 0 planted, item 1 the same field with nothing planted.  The poisoned item equals the oracle,
    the clean one its own single call (and the oracle)."""
    torch = torch_mod
    p = planted(kind)
    flows = [p["flow"], p["field"][0]]
    depths = None if kind == "flow" else [p["depth"], p["field"][1]]
    B, _, h, w = flows[0].shape
    results = []
    for fill in SENTINELS:
        outs = [Guarded(torch, (B, 2, h, w), fill) for _ in flows]
        counts = [Guarded(torch, (B, 1, h, w), fill) for _ in flows]
        d = None if depths is None else [gpu(torch, a) for a in depths]
        assert cabi.flowprojection_forward_batch([gpu(torch, f) for f in flows], [c.v for c in counts], [o.v for o in outs],
                                                 fillhole, inputs2=d) == 0
        for i, (o, c) in enumerate(zip(outs, counts)):
            o.ok(torch, "item %d out" % i), c.ok(torch, "item %d count" % i)
        results.append([(cpu(o.v), cpu(c.v)) for o, c in zip(outs, counts)])
    ref, rcount = p["ref"][fillhole]
    _same("poisoned item count", results[0][0][1], rcount, p["mirror"])
    _same("poisoned item out", results[0][0][0], ref, p["mirror"])
    single = _call(torch, cabi, "lean", flows[1], None if depths is None else depths[1], fillhole, SENTINELS[0])
    assert np.isfinite(single[0]).all() and np.isfinite(single[1]).all()
    assert np.array_equal(results[0][1][1], single[1]) and np.array_equal(results[0][1][0], single[0]), "clean item != its single call"
    for i in range(2):
        _same("item %d, second sentinel" % i, results[1][i][0], results[0][i][0])
        _same("item %d count, second sentinel" % i, results[1][i][1], results[0][i][1])


@pytest.mark.parametrize("kind", ["flow", "depth"])
@pytest.mark.parametrize("fillhole", [0, 1])
def test_up4_with_planted_quarter_flow_and_depth(torch_mod, cabi, oracle, kind, fillhole):
    torch = torch_mod
    fq, depth = fe.up4_inputs(kind, np.random.default_rng([SEED, 4]))
    m0, m1 = fe.UP4_MULS
    hq, wq = fq.shape[2:]
    ref, rcount = oracle.flowproj_up4_fwd(fq, m0, m1, fillhole, depth=depth, fmad=1)
    runs = []
    for fill in SENTINELS:
        out = Guarded(torch, (1, 2, 4 * hq, 4 * wq), fill)
        count = Guarded(torch, (1, 1, 4 * hq, 4 * wq), fill)
        if depth is None:
            assert cabi.flowprojection_forward_up4(gpu(torch, fq), count.v, out.v, m0, m1, fillhole) == 0
        else:
            assert cabi.depthflowprojection_forward_up4(gpu(torch, fq), gpu(torch, depth), count.v, out.v, m0, m1, fillhole) == 0
        out.ok(torch, "up4 out"), count.ok(torch, "up4 count")
        runs.append((cpu(out.v), cpu(count.v)))
    _same("up4 count", runs[0][1], rcount)
    _same("up4 out", runs[0][0], ref)
    _same("up4 count, second sentinel", runs[1][1], runs[0][1])
    _same("up4 out, second sentinel", runs[1][0], runs[0][0])


# ------------------------------------------------------------------ PWC-Net warp

@pytest.mark.parametrize("shape", fe.WARP_SHAPES)
@pytest.mark.parametrize("align_corners", [True, False])
def test_pwc_warp_planted_features(torch_mod, cabi, oracle, shape, align_corners):
    torch = torch_mod
    x, flo, _ = fe.warp_inputs(shape, align_corners)
    ref = oracle.pwc_warp(x, flo, align_corners, fmad=1)
    assert np.isnan(ref).any()
    runs = []
    for fill in SENTINELS:
        out = Guarded(torch, shape, fill)
        assert cabi.pwc_warp_forward(gpu(torch, x), gpu(torch, flo), out.v, align_corners) == 0
        out.ok(torch, "pwc_warp_forward")
        runs.append(cpu(out.v))
    _same("pwc_warp_forward", runs[0], ref)
    _same("pwc_warp_forward, second sentinel", runs[1], runs[0])
    # the fused entry: warp the planted map, correlate with a finite one == the two launches
    f1 = np.random.default_rng([SEED, 5]).standard_normal(shape).astype(f32)
    fused = cabi.pwc_warp_correlation_forward(gpu(torch, f1), gpu(torch, x), gpu(torch, flo), align_corners)
    two = cabi.correlation_forward(gpu(torch, f1), gpu(torch, runs[0]), 4, 1, 4, 1, 1)
    assert np.isnan(cpu(two)).any() and np.isfinite(cpu(two)).any()
    _same("pwc_warp_correlation_forward against warp, then correlation", cpu(fused), cpu(two))


# ------------------------------------------------------------------ MinDepthFlowProjection

@pytest.mark.parametrize("shape", fe.MINDEPTH_SHAPES)
@pytest.mark.parametrize("fillhole", [0, 1])
def test_mindepth_order_edges(torch_mod, cabi, oracle, shape, fillhole):
    """Negative weights over a negative incoming count (the ~u branch of md_order_bits and its inverse), infinite weights,
    weights equal to the incoming count (strict >), +0.0 against -0.0: bit for bit the oracle's raster-order result."""
    torch = torch_mod
    flow, wgt, count0 = fe.mindepth_inputs(shape, np.random.default_rng([SEED, shape[2]]))
    B, H, W = shape
    ref, rcount = oracle.mindepthflowproj_fwd(flow, wgt, fillhole, count0=count0)
    count = gpu(torch, count0)
    out = torch.zeros((B, 2, H, W), device="cuda:0")
    assert cabi.mindepthflowprojection_forward(gpu(torch, flow), gpu(torch, wgt), count, out, fillhole) == 0
    _same("MinDepth count", cpu(count), rcount)
    _same("MinDepth out", cpu(out), ref)


# ------------------------------------------------------------------ FilterInterpolation

F16_TOL = 2e-3                              # tests/test_gpu_fi_windows.py's rule for the fp16 staged kernel


class FramedS:
    """tests/test_gpu_fi_windows.py's Framed with a finite sentinel instead of NaN: an interior view [:, :, 1:h+1, col:col+w]
    of a larger buffer.  ok(): no element of the view holds the sentinel, every element outside it does."""

    def __init__(self, torch, shape, col, dtype, fill, data=None):
        B, C, h, w = shape
        self.col, self.h, self.w, self.fill = col, h, w, fill
        self.big = torch.full((B, C, h + 3, w + 8 + (w % 2)), fill, dtype=dtype, device="cuda:0")
        self.v = self.big[:, :, 1:h + 1, col:col + w]
        if data is not None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(data)))

    def ok(self, torch, what):
        sent = self.big == torch.tensor(self.fill, dtype=self.big.dtype, device="cuda:0")
        inside = torch.zeros_like(sent)
        inside[:, :, 1:self.h + 1, self.col:self.col + self.w] = True
        assert not (sent & inside).any(), "%s: %d elements of the view left unwritten" % (what, int((sent & inside).sum()))
        assert sent[~inside].all(), "%s: %d elements written outside the view" % (what, int((~sent[~inside]).sum()))

    def np(self):
        return self.v.cpu().numpy()


def _fi_same(what, got, want, pix):
    d = fe.differing_by_class(got, want, pix)
    assert not d, "%s: pixels that differ, by class: %s; %s" % (what, d, fe.describe_difference(got, want))


def _twice(torch, shape, col, dtype, call, what):
    """`call(out view)` into two sentinel-framed outputs; the two results must be the same.  Returns the first."""
    res = []
    for fill in SENTINELS:
        out = FramedS(torch, shape, col, dtype, fill)
        assert call(out.v) == 0, what
        out.ok(torch, "%s, sentinel %g" % (what, fill))
        res.append(out.np())
    assert fe.same_bits_nan_aware(res[1], res[0]), "%s: the result depends on what the output held" % what
    return res[0]


@pytest.mark.parametrize("C", [3, 9])
@pytest.mark.parametrize("layout", ["aligned", "unaligned"])
def test_fi_ori_planted(torch_mod, cabi, oracle, layout, C):
    """filterinterp_forward_ori, fs = 4: the staged kernel and direct=True, every window class of the layout."""
    torch = torch_mod
    from tests import fi_windows as fw
    c = fe.fi_case("lds", C, layout == "aligned", 4)
    col = 4 if layout == "aligned" else 1
    gi = FramedS(torch, c["img"].shape, col, torch.float32, 0.0, c["img"])
    assert fw.aligned16(gi.v) == (layout == "aligned")
    flow, gk = gpu(torch, c["flow"]), gpu(torch, c["filt"])
    ref = oracle.filterinterp_ori_fwd(c["img"], c["flow"], c["filt"], fmad=1, nthreads=8)
    staged = _twice(torch, c["img"].shape, col, torch.float32, lambda o: cabi.filterinterp_forward_ori(gi.v, flow, gk, o), "staged")
    direct = _twice(torch, c["img"].shape, col, torch.float32,
                    lambda o: cabi.filterinterp_forward_ori(gi.v, flow, gk, o, direct=True), "direct")
    _fi_same("staged (C=%d, %s) vs oracle" % (C, layout), staged, ref, c["pix"])
    _fi_same("direct (C=%d, %s) vs oracle" % (C, layout), direct, ref, c["pix"])
    _fi_same("staged vs direct", staged, direct, c["pix"])


@pytest.mark.parametrize("C", [3, 9])
@pytest.mark.parametrize("fs", [2, 5, 6])
def test_fi_ori_planted_other_filter_sizes(torch_mod, cabi, oracle, fs, C):
    torch = torch_mod
    c = fe.fi_case("n", C, True, fs)
    gi = FramedS(torch, c["img"].shape, 3, torch.float32, 0.0, c["img"])
    flow, gk = gpu(torch, c["flow"]), gpu(torch, c["filt"])
    ref = oracle.filterinterp_ori_fwd(c["img"], c["flow"], c["filt"], fmad=1, nthreads=8)
    staged = _twice(torch, c["img"].shape, 3, torch.float32, lambda o: cabi.filterinterp_forward_ori(gi.v, flow, gk, o), "staged")
    direct = _twice(torch, c["img"].shape, 3, torch.float32,
                    lambda o: cabi.filterinterp_forward_ori(gi.v, flow, gk, o, direct=True), "direct")
    _fi_same("fs=%d staged (C=%d) vs oracle" % (fs, C), staged, ref, c["pix"])
    _fi_same("fs=%d direct (C=%d) vs oracle" % (fs, C), direct, ref, c["pix"])


@pytest.mark.parametrize("C", [3, 9])
def test_fi_blend_planted(torch_mod, cabi, oracle, C):
    """filterinterp_blend_forward: C <= 4 blends in the second direction's epilogue, C = 9 runs two launches and
    fi_blend_only.  Both directions planted; blend, out0 and out2 against the oracle."""
    torch = torch_mod
    from tests import fi_windows as fw
    c2, c0 = fe.fi_case("blend", C), fe.fi_case("blend", C, which=1)
    shape = c2["img"].shape
    w0, w2 = 0.75, 0.25
    g0 = FramedS(torch, shape, 4, torch.float32, 0.0, c0["img"])
    g2 = FramedS(torch, shape, 4, torch.float32, 0.0, c2["img"])
    args = (g0.v, g2.v, gpu(torch, c0["flow"]), gpu(torch, c2["flow"]), gpu(torch, c0["filt"]), gpu(torch, c2["filt"]))
    res = []
    for fill in SENTINELS:
        outs = [FramedS(torch, shape, 4, torch.float32, fill) for _ in range(3)]
        assert cabi.filterinterp_blend_forward(*args, outs[0].v, outs[1].v, outs[2].v, w0, w2) == 0
        for o, name in zip(outs, ("blend", "out0", "out2")):
            o.ok(torch, name)
        res.append([o.np() for o in outs])
    r_blend, r0, r2 = oracle.filterinterp_blend(c0["img"], c2["img"], c0["flow"], c2["flow"], c0["filt"], c2["filt"], w0, w2, fmad=1)
    assert np.isnan(r_blend).any() and np.isinf(r_blend).any()
    pix0 = fw.pixel_labels("lds", fw.classes("lds", c0["flow"], c0["h"], c0["w"], fw.aligned16(g0.v)), c0["h"], c0["w"])
    _fi_same("out2 (C=%d)" % C, res[0][2], r2, c2["pix"])
    _fi_same("out0 (C=%d)" % C, res[0][1], r0, pix0)
    _fi_same("blend (C=%d)" % C, res[0][0], r_blend, c2["pix"])
    for k, name in enumerate(("blend", "out0", "out2")):
        assert fe.same_bits_nan_aware(res[1][k], res[0][k]), name


@pytest.mark.parametrize("C", [3, 9])
def test_fi_multi_planted(torch_mod, cabi, oracle, C):
    """filterinterp_forward_ori_multi: both flows' outputs (the first flow planted) equal the oracle's."""
    torch = torch_mod
    c = fe.fi_case("multi", C)
    shape = c["img"].shape
    gi = FramedS(torch, shape, 4, torch.float32, 0.0, c["img"])
    flows = [gpu(torch, c["flow"]), gpu(torch, c["flow2"])]
    gk = gpu(torch, c["filt"])
    res = []
    for fill in SENTINELS:
        outs = [FramedS(torch, shape, 4, torch.float32, fill) for _ in range(2)]
        assert cabi.filterinterp_forward_ori_multi(gi.v, flows, gk, [o.v for o in outs]) == 0
        for t, o in enumerate(outs):
            o.ok(torch, "multi out %d" % t)
        res.append([o.np() for o in outs])
    for t, fl in enumerate((c["flow"], c["flow2"])):
        ref = oracle.filterinterp_ori_fwd(c["img"], fl, c["filt"], fmad=1, nthreads=8)
        assert np.isnan(ref).any() and np.isinf(ref).any()
        _fi_same("multi flow %d (C=%d)" % (t, C), res[0][t], ref, c["pix"])
        assert fe.same_bits_nan_aware(res[1][t], res[0][t])


@pytest.mark.parametrize("C", [3, 9])
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("fs", [4, 6])
def test_fi_defor_planted(torch_mod, cabi, oracle, fs, variant, C):
    """filterinterp_forward_defor, staged and general=True: image, filter and flow planted; the offsets stay finite (the
    reference converts them to int with no defined result for a non-finite one)."""
    torch = torch_mod
    c = fe.fi_case("defor", C, True, fs)
    shape = c["img"].shape
    gi = FramedS(torch, shape, 3, torch.float32, 0.0, c["img"])
    flow = gpu(torch, c["flow"])
    third, fourth = (gpu(torch, c["off"]), None) if variant == 2 else (gpu(torch, c["filt"]), gpu(torch, c["off"]))
    ref = oracle.filterinterp_defor_fwd(variant, c["img"], c["flow"], c["filt"], c["off"], fmad=1)
    staged = _twice(torch, shape, 3, torch.float32, lambda o: cabi.filterinterp_forward_defor(variant, gi.v, flow, third, fourth, o), "staged")
    general = _twice(torch, shape, 3, torch.float32,
                     lambda o: cabi.filterinterp_forward_defor(variant, gi.v, flow, third, fourth, o, general=True), "general")
    _fi_same("defor fs=%d v%d (C=%d) staged vs oracle" % (fs, variant, C), staged, ref, c["pix"])
    _fi_same("defor fs=%d v%d (C=%d) general vs oracle" % (fs, variant, C), general, ref, c["pix"])


@pytest.mark.parametrize("C", [3, 9])
def test_fi_f16_planted(torch_mod, cabi, oracle, C):
    """fp16 storage.  The direct kernel: bit for bit.  The staged kernel merges the weights of clamped columns (DESIGN.md
    4.3), so at a border it may return Inf where the oracle has NaN: finite outputs within F16_TOL, the non-finite mask
    the oracle's everywhere, NaN against Inf the oracle's at every pixel whose window is not clamped."""
    torch = torch_mod
    c = fe.fi_case("f16", C)
    shape = c["img"].shape
    gi = FramedS(torch, shape, 2, torch.float16, 0.0, c["img"])
    flow, gk = gpu(torch, c["flow"]), gpu(torch, c["filt"])
    ref = oracle.filterinterp_ori_fwd_f16(c["img"], c["flow"], c["filt"], fmad=1)
    staged = _twice(torch, shape, 2, torch.float16, lambda o: cabi.filterinterp_forward_ori_f16(gi.v, flow, gk, o), "f16 staged")
    direct = _twice(torch, shape, 2, torch.float16,
                    lambda o: cabi.filterinterp_forward_ori_f16(gi.v, flow, gk, o, direct=True), "f16 direct")
    _fi_same("f16 direct (C=%d) vs oracle" % C, direct, ref, c["pix"])
    assert fe.same_nonfinite_mask(staged, ref), "f16 staged: non-finite mask: %d elements differ" % int(
        (np.isfinite(staged) != np.isfinite(ref)).sum())
    fin = np.isfinite(ref)
    g, r = staged.astype(np.float64), ref.astype(np.float64)
    bad = fin & (np.abs(np.where(fin, g, 0) - np.where(fin, r, 0)) > F16_TOL * np.maximum(1.0, np.abs(np.where(fin, r, 0))))
    assert not bad.any(), "f16 staged: %d finite outputs beyond F16_TOL" % int(bad.sum())
    free = ~fe.clamped_windows(c["flow"], c["h"], c["w"])
    free = np.broadcast_to(free[:, None], ref.shape)
    assert np.array_equal(np.isnan(staged)[free], np.isnan(ref)[free]), "f16 staged: NaN against Inf where no window is clamped"
    assert np.array_equal(staged[free & np.isinf(ref)], ref[free & np.isinf(ref)]), "f16 staged: the sign of an infinity"
