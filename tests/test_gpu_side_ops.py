"""Interpolation / InterpolationCh, SeparableConv, SeparableConvFlow and MinDepthFlowProjection on the inputs that decide
their comparisons (tests/side_ops.py plants them; tests/test_side_ops_host.py checks the plants against the oracle alone).

What is asserted, everywhere: the result equals the oracle's (`fmad=1`) NaN-aware and bit for bit -- NaN at the same
elements, every other element, infinities and signed zeros included, with the same bits.  Every planted finite value is
dyadic, so there is no tolerance to state.

Outputs are views into sentinel-filled buffers with guard elements on both sides (Guarded, of test_gpu_forward_edges.py).
An op that writes its whole output runs with two sentinels: the two results are the same, no sentinel survives inside the
view, every guard element is intact.  An op that adds into its output, or leaves untouched targets alone, starts from a
non-zero dyadic pattern (or from the sentinel itself) that the oracle is handed too; the guard elements are checked alike.
"""
import numpy as np
import pytest

from tests import forward_edges as fe
from tests import side_ops as so
from tests.test_gpu_forward_edges import GUARD, SENTINELS, Guarded
from tests.test_gpu_parity import cpu, gpu, torch_mod, cabi  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

f32 = np.float32
OTHER = 777.0                                               # what the unused parts of an input buffer hold


class GuardedSlice(Guarded):
    """Channels c0 .. c0 + C of a Guarded tensor of `wide` channels: the batch stride is that of the wider tensor."""

    def __init__(self, torch, shape, fill, c0, wide, off=GUARD, pad=0):
        B, C, h, w = shape
        super().__init__(torch, (B, wide, h, w), fill, off=off, pad=pad)
        n = B * wide * h * (w + pad)
        self.v = self.v[:, c0:c0 + C]
        self.inside.zero_()
        self.inside[off:off + n].view(B, wide, h, w + pad)[:, c0:c0 + C, :, :w] = True


def _load(torch, g, data):
    g.v.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=f32)))
    return g


def _put(torch, data, pad=0, off=GUARD, fill=OTHER):
    """An input (or a starting value) in a guarded buffer."""
    return _load(torch, Guarded(torch, data.shape, fill, off=off, pad=pad), data)


def _guards_intact(g, what):
    sent = g.flat == g.fill
    assert sent[~g.inside].all(), "%s: %d elements written outside the view" % (what, int((~sent[~g.inside]).sum()))


def _same(what, got, want):
    assert so.same_bits_nan_aware(got, want), "%s: %s" % (what, so.describe_difference(got, want))


# ------------------------------------------------------------------ Interpolation / InterpolationCh

INTERP_CASES = ("planted C=2", "planted C=3", "border")


@pytest.fixture(scope="module")
def interp_cases(oracle):
    """{name: (img, flow, require_c3, the oracle's output)} -- once"""
    cache = {}
    for name in INTERP_CASES:
        if name == "border":
            img, flow, expect = so.interp_border()
            c3 = False
        else:
            C = int(name[-1])
            img, flow = fe.small_interp_inputs(np.random.default_rng([so.SEED, 1, C]), B=2, C=C)
            c3 = C == 3
        ref = oracle.interp_fwd(img, flow, fmad=1)
        if name == "border":
            assert so.same_bits_nan_aware(ref, so.interp_border_expected(img, expect))
        for a in (img, flow, ref):
            a.setflags(write=False)
        cache[name] = (img, flow, c3, ref)
    return cache


@pytest.mark.parametrize("layout", ["dense", "slice", "rows"])
@pytest.mark.parametrize("name", INTERP_CASES)
def test_interpolation_forward_planted(torch_mod, cabi, interp_cases, name, layout):
    """interp_forward on tests/forward_edges.small_interp_inputs (B = 2; NaN, infinities, +-3e38 flows, non-finite image
    values) and on the border decisions of side_ops.interp_border.  slice: image and output are channels 1 .. C of tensors
    of C + 2 channels; rows: image, flow and output rows are w + 1 floats apart."""
    torch = torch_mod
    img, flow, c3, ref = interp_cases[name]
    B, C, H, W = img.shape
    runs = []
    for fill in SENTINELS:
        if layout == "slice":
            gi = _load(torch, GuardedSlice(torch, img.shape, OTHER, 1, C + 2), img)
            out = GuardedSlice(torch, img.shape, fill, 1, C + 2)
            fl = _put(torch, flow)
        else:
            pad = int(layout == "rows")
            gi, fl = _put(torch, img, pad=pad), _put(torch, flow, pad=pad)
            out = Guarded(torch, img.shape, fill, pad=pad)
        assert cabi.interpolation_forward(gi.v, fl.v, out.v, require_c3=c3) == 0
        what = "%s, %s, sentinel %g" % (name, layout, fill)
        out.ok(torch, what)
        _guards_intact(gi, what + " image"), _guards_intact(fl, what + " flow")
        runs.append(cpu(out.v))
    _same("%s, %s" % (name, layout), runs[0], ref)
    _same("%s, %s, second sentinel" % (name, layout), runs[1], runs[0])


def test_interpolation_modules_planted(torch_mod, cabi, interp_cases):
    """The same inputs through the two reference-named modules (Interpolation takes three channels only)."""
    torch = torch_mod
    from vfidkr_amd.my_package.Interpolation import InterpolationModule
    from vfidkr_amd.my_package.InterpolationCh import InterpolationChModule
    with torch.no_grad():
        for name in INTERP_CASES:
            img, flow, c3, ref = interp_cases[name]
            _same("InterpolationCh, " + name, cpu(InterpolationChModule()(gpu(torch, img), gpu(torch, flow))), ref)
            if c3:
                _same("Interpolation, " + name, cpu(InterpolationModule()(gpu(torch, img), gpu(torch, flow))), ref)


# ------------------------------------------------------------------ SeparableConv

def _sep_run(torch, cabi, oracle, d, what, c3):
    """Forward (two sentinels) and the backward's three gradients, added into non-zero dyadic starting values."""
    img, v, h, gout = d["img"], d["v"], d["h"], d["gout"]
    gi, gv, gh = gpu(torch, img), gpu(torch, v), gpu(torch, h)
    kw = {} if c3 else dict(require_c3=False)
    ref = oracle.sepconv_fwd(img, v, h, fmad=1)
    runs = []
    for fill in SENTINELS:
        out = Guarded(torch, ref.shape, fill)
        assert cabi.separableconv_forward(gi, gv, gh, out.v, **kw) == 0
        out.ok(torch, "%s forward, sentinel %g" % (what, fill))
        runs.append(cpu(out.v))
    _same(what + " forward", runs[0], ref)
    _same(what + " forward, second sentinel", runs[1], runs[0])
    start = tuple(so.pattern(a.shape, n) for n, a in enumerate((img, v, h)))
    want = oracle.sepconv_bwd(img, v, h, gout, start=start)
    grads = [_put(torch, s, fill=SENTINELS[0]) for s in start]
    assert cabi.separableconv_backward(gi, gv, gh, gpu(torch, gout), grads[0].v, grads[1].v, grads[2].v, **kw) == 0
    for g, w, key in zip(grads, want, ("gradinput1", "gradinput2", "gradinput3")):
        g.ok(torch, "%s backward %s" % (what, key))
        _same("%s backward %s" % (what, key), cpu(g.v), w)


@pytest.mark.parametrize("C,fs,oh,ow", so.sep_shapes())
def test_separableconv_channel_tail_and_tap_block(torch_mod, cabi, oracle, C, fs, oh, ow):
    """sepconv_forward<3>'s channel tail (C % 3 != 0) with its eight-tap block alone, with a remainder, twice; the backward's
    gradients add into what they hold.  Finite dyadic inputs: every sum is exact."""
    assert cabi.separableconv_forward(*(gpu(torch_mod, np.zeros(s, f32)) for s in ((1, C, fs, fs), (1, fs, 1, 1), (1, fs, 1, 1), (1, C, 1, 1)))) == 1
    _sep_run(torch_mod, cabi, oracle, so.sep_dyadic(C, fs, oh, ow), "C=%d fs=%d %dx%d" % (C, fs, oh, ow), False)


@pytest.mark.parametrize("fs", so.SEP_PLANT_SIZES)
def test_separableconv_planted(torch_mod, cabi, oracle, fs):
    """+-inf, NaN, +-FLT_MAX, +-2^-149 and -0.0 in the image, in v and in h: the forward, sepconv_backward's v / h gradients
    and sepconv_backward_image's gather (the sequential order) agree with the oracle bit for bit."""
    _sep_run(torch_mod, cabi, oracle, so.sep_planted(fs), "planted fs=%d" % fs, True)


# ------------------------------------------------------------------ SeparableConvFlow

def _sepflow_run(torch, cabi, oracle, d, what):
    v, h, gflow = d["v"], d["h"], d["gflow"]
    H, W = d["img"].shape[2:]
    gi, gv, gh = gpu(torch, d["img"]), gpu(torch, v), gpu(torch, h)
    ref = oracle.sepconvflow_fwd(v, h, H, W, fmad=1)
    runs = []
    for fill in SENTINELS:
        out = Guarded(torch, ref.shape, fill)
        assert cabi.separableconvflow_forward(gi, gv, gh, out.v) == 0
        out.ok(torch, "%s forward, sentinel %g" % (what, fill))
        runs.append(cpu(out.v))
    _same(what + " forward", runs[0], ref)
    _same(what + " forward, second sentinel", runs[1], runs[0])
    # gradinput2 is stored, gradinput3 added to, each only where its tap sum decides: both start from a non-zero pattern
    start = (so.pattern(v.shape, 1), so.pattern(h.shape, 2))
    want = oracle.sepconvflow_bwd(v, h, gflow, H, W, fmad=1, start=start)
    grads = [_put(torch, s, fill=SENTINELS[0]) for s in start]
    assert cabi.separableconvflow_backward(gi, gv, gh, gpu(torch, gflow), grads[0].v, grads[1].v) == 0
    for g, w, key in zip(grads, want, ("gradinput2", "gradinput3")):
        g.ok(torch, "%s backward %s" % (what, key))
        _same("%s backward %s" % (what, key), cpu(g.v), w)
    return runs[0]


def test_separableconvflow_planted(torch_mod, cabi, oracle):
    """The tap vectors of side_ops.SEPFLOW_VECTORS in v along one row and in h along another: `fabsf(sum) > 0` on +0, -0,
    a subnormal (a kernel that flushes it answers -2000 instead of -2), inf, NaN, inf - inf and an overflowing sum."""
    fl = _sepflow_run(torch_mod, cabi, oracle, so.sepflow_planted(), "planted")
    for x, want in so.sepflow_expected():
        for got in (fl[:, 1, so.SEPFLOW_ROW_V, x], fl[:, 0, so.SEPFLOW_ROW_H, x]):
            assert np.isnan(got).all() if np.isnan(want) else (got == f32(want)).all(), (x, want, got)


@pytest.mark.parametrize("fs", [1, 2, 5, 51])
def test_separableconvflow_finite(torch_mod, cabi, oracle, fs):
    _sepflow_run(torch_mod, cabi, oracle, so.sepflow_finite(fs), "fs=%d" % fs)


# ------------------------------------------------------------------ MinDepthFlowProjection forward

def _md_call(torch, cabi, layout, flow, wgt, count0, out0, fillhole, fill):
    """One forward call; (out, count) as numpy.  rows: flow and output rows w + 1 floats apart; count_odd: count at an odd
    element offset; weight_slice: the weight is channel 1 of a three-channel tensor.  count and output start from count0
    and out0; whatever the call leaves alone must still hold them, and every guard element its sentinel."""
    pad = int(layout == "rows")
    fl = _put(torch, flow, pad=pad)
    out = _put(torch, out0, pad=pad, fill=fill)
    count = _put(torch, count0, off=GUARD + int(layout == "count_odd"), fill=fill)
    if layout == "weight_slice":
        w = _load(torch, GuardedSlice(torch, wgt.shape, OTHER, 1, 3), wgt)
    else:
        w = _put(torch, wgt)
    assert cabi.mindepthflowprojection_forward(fl.v, w.v, count.v, out.v, fillhole) == 0
    for g, name in ((fl, "flow"), (w, "weight"), (count, "count"), (out, "output")):
        _guards_intact(g, "%s, sentinel %g: %s" % (layout, fill, name))
    assert torch.equal(fl.v, torch.from_numpy(flow).cuda()), "the flow was written"
    return cpu(out.v), cpu(count.v)


@pytest.mark.parametrize("name", so.MD_TIE_NAMES)
@pytest.mark.parametrize("fillhole", [0, 1])
def test_mindepth_signed_zero_ties_keep_the_first_source(torch_mod, cabi, oracle, name, fillhole):
    """Two or three sources with weights -0.0 / +0.0 on one target over an incoming count of -1: `+0 > -0` is false, so the
    first source in raster order keeps the target -- its negated flow in the output, its own weight bits in count.  The
    output starts from the sentinel: untouched targets keep it."""
    torch = torch_mod
    flow, wgt, count0, expect = so.md_zero_tie(name)
    for fill in SENTINELS:
        out0 = np.full(flow.shape, fill, f32)
        ref, rcount = oracle.mindepthflowproj_fwd(flow, wgt, fillhole, count0=count0, out0=out0)
        out, count = _md_call(torch, cabi, "dense", flow, wgt, count0, out0, fillhole, fill)
        for b, ty, tx, (sy, sx) in expect:
            assert np.array_equal(out[b, :, ty, tx], -flow[b, :, sy, sx]), (
                "%s: target (%d, %d, %d) holds %s, the first source's negated flow is %s" % (name, b, ty, tx, out[b, :, ty, tx], -flow[b, :, sy, sx]))
            assert so.bits(count)[b, 0, ty, tx] == so.bits(wgt)[b, 0, sy, sx], (
                "%s: count bits %#x, the first source's weight bits %#x" % (name, so.bits(count)[b, 0, ty, tx], so.bits(wgt)[b, 0, sy, sx]))
        _same("%s count" % name, count, rcount)
        _same("%s out" % name, out, ref)


@pytest.fixture(scope="module")
def holes(oracle):
    flow, wgt, count0, out0 = so.md_holes()
    ref, rcount = oracle.mindepthflowproj_fwd(flow, wgt, 1, count0=count0, out0=out0)
    sflow, swgt, scount0 = fe.mindepth_inputs(fe.MINDEPTH_SHAPES[0], np.random.default_rng([so.SEED, 7]))
    sref = oracle.mindepthflowproj_fwd(sflow, swgt, 1, count0=scount0)
    for a in (flow, wgt, count0, out0, ref, rcount, sflow, swgt, scount0) + sref:
        a.setflags(write=False)
    return dict(big=(flow, wgt, count0, out0), ref=ref, rcount=rcount, small=(sflow, swgt, scount0), sref=sref)


@pytest.mark.parametrize("layout", ["dense", "rows", "count_odd", "weight_slice"])
def test_mindepth_designed_holes(torch_mod, cabi, holes, layout):
    """Every flow invalid: the forward writes nothing and mindepth_fillhole runs on the caller's count and output alone
    (side_ops.md_holes: 200 x 300, B = 2 mirrored) -- walks of every distance class up to 299 columns and 199 rows, found
    cells on bit 0, on bit 31 and in the last partial word, walks that find nothing, found counts that are negative,
    infinite or NaN."""
    torch = torch_mod
    flow, wgt, count0, out0 = holes["big"]
    runs = [_md_call(torch, cabi, layout, flow, wgt, count0, out0, 1, fill) for fill in SENTINELS]
    _same("count (%s)" % layout, runs[0][1], holes["rcount"])
    _same("out (%s)" % layout, runs[0][0], holes["ref"])
    _same("count, second sentinel", runs[1][1], runs[0][1])
    _same("out, second sentinel", runs[1][0], runs[0][0])
    if layout == "dense":                                   # fillhole 0: nothing at all is written
        out, count = _md_call(torch, cabi, layout, flow, wgt, count0, out0, 0, SENTINELS[0])
        _same("count, fillhole 0", count, count0)
        _same("out, fillhole 0", out, out0)


def test_mindepth_scratch_reuse_across_frame_sizes(torch_mod, cabi, holes):
    """The 200 x 300 call, a 20 x 30 call, the 200 x 300 call again on one stream: the keys and bitmaps of the per-stream
    scratch are rebuilt by every call."""
    torch = torch_mod
    flow, wgt, count0, out0 = holes["big"]
    sflow, swgt, scount0 = holes["small"]
    for step in range(3):
        if step == 1:
            out, count = _md_call(torch, cabi, "dense", sflow, swgt, scount0, np.zeros(sflow.shape, f32), 1, SENTINELS[0])
            _same("small call count", count, holes["sref"][1])
            _same("small call out", out, holes["sref"][0])
        else:
            out, count = _md_call(torch, cabi, "dense", flow, wgt, count0, out0, 1, SENTINELS[0])
            _same("large call %d count" % step, count, holes["rcount"])
            _same("large call %d out" % step, out, holes["ref"])


# ------------------------------------------------------------------ MinDepthFlowProjection backward

@pytest.mark.parametrize("layout", ["dense", "rows"])
def test_mindepth_backward_plants(torch_mod, cabi, oracle, layout):
    """Sources on the last column, the last row and the corner (R == L, Bm == T: the same target two or four times), +0.0
    against -0.0 (equal), NaN against NaN (never), inf against inf, a weight equal to a neighbour's count only; gradinput1
    starts from a non-zero dyadic pattern and the sums are exact."""
    torch = torch_mod
    flow, wgt, count, gout, expect = so.md_backward()
    start = so.pattern(flow.shape, 3)
    want = oracle.mindepthflowproj_bwd(flow, wgt, count, gout, start=start)
    pad = int(layout == "rows")
    fl, go = _put(torch, flow, pad=pad), _put(torch, gout, pad=pad)
    g1 = _put(torch, start, pad=pad, fill=SENTINELS[0])
    g2 = torch.zeros(wgt.shape, device="cuda:0")
    unused = torch.zeros(flow.shape, device="cuda:0")
    assert cabi.mindepthflowprojection_backward(fl.v, gpu(torch, wgt), gpu(torch, count), unused, go.v, g1.v, g2) == 0
    g1.ok(torch, "gradinput1 (%s)" % layout)
    got = cpu(g1.v)
    for (b, y, x), w in so.md_backward_expected(gout, expect, start).items():
        assert np.array_equal(got[b, :, y, x], w), ("source (%d, %d, %d)" % (b, y, x), got[b, :, y, x], w)
    _same("gradinput1 (%s)" % layout, got, want)
    assert not cpu(g2).any() and not cpu(unused).any()
