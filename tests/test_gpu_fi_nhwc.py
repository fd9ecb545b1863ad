"""GPU suite (`-m gpu`): the context warp on channels_last tensors, vfi_filterinterp_forward_ori_nhwc_multi_to[_bf16]
(csrc/filterinterp_nhwc.hip), and fused.FilterInterpolate_ctx_all on channels_last context tensors.

Every result is compared as raw BITS, NaN at equal positions (tests/fi_nhwc.same_raw_bits), with two yardsticks:
  the oracle    oracle.filterinterp_ori_fwd(fmad=1) on the logical NCHW tensors; bfloat16: widen -> float32 -> round once;
  the NCHW entry  cabi.filterinterp_forward_ori_multi on `.contiguous()` copies of the same tensors.
Image and destinations live in pattern-filled buffers (tests/pwc_bf16.guarded): nothing outside a view is written.

Tile: FN_TW x FN_TH = 32 x 4 pixels (tests/fi_nhwc.constants), so the 19 x 37 frame has 5 x 2 tiles with ragged last tiles
both ways.  The library ships one path per filter-size class: the LDS-staged window kernel was built, was bit-equal to this
one, measured slower and is not shipped, so there is no staged / direct pair and no tile whose window
exceeds an LDS budget; what differs between launches is the access width.  The width the library chooses is read back
(cabi.filterinterp_nhwc_access_width) and must be the mirror's, and every width is compared with the same yardsticks.
"""
import numpy as np
import pytest

from tests import fi_nhwc as fn
from tests import forward_edges as fe
from tests.test_gpu_parity import cabi, gpu, torch_mod  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

f32 = np.float32
DTYPES = ["float32", "bfloat16"]
FRAME = (19, 37)


@pytest.fixture(scope="module")
def fused(torch_mod):
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import fused as f
    return f


def _dtype(torch, name):
    return getattr(torch, name)


def _image(rng, shape, bf16):
    img = rng.random(shape, dtype=f32) * 2 - 1
    return fn.to_bf16(img) if bf16 else img


def _ff(torch, a, layout):
    """a float32 flow / filter on the GPU, NCHW or channels_last"""
    t = gpu(torch, a)
    return t.contiguous(memory_format=torch.channels_last) if layout == "cl" else t


def run_case(torch, cabi, oracle, dtype, img, flows, filt, dst=None, src=None, batch_pad=16, ff_layout="nchw", want_width=None):
    """img, flows, filt: logical NCHW numpy arrays.  src / dst: None for a dense channels_last tensor, else (total channels,
    first channel) of the wider channels_last buffer the image / every destination is a slice of.  Compares every output
    with the oracle and with the NCHW entry, checks the guards, returns the access width the launcher chose."""
    bf16 = dtype == "bfloat16"
    td = _dtype(torch, dtype)
    B, C, h, w = img.shape
    esize = 2 if bf16 else 4

    def view(spec):
        ctot, c0 = (C, 0) if spec is None else spec
        buf, wide = fn.cl_buffer(torch, B, ctot, h, w, td, batch_pad)
        return buf, wide[:, c0:c0 + C]

    ibuf, vin = view(src)
    fn.cl_fill(torch, vin, img)
    ibits = ibuf.clone()
    outs = [view(dst) for _ in flows]
    gflows = [_ff(torch, fl, ff_layout) for fl in flows]
    gfilt = _ff(torch, filt, ff_layout)
    fs = int(np.sqrt(f32(filt.shape[1])))
    width = fn.vector_width(esize, img.shape, fn.tensor_layout(vin), [fn.tensor_layout(o) for _, o in outs], fs)
    if want_width is not None:
        assert want_width(width), "access width %d" % width
    chosen = cabi.filterinterp_nhwc_access_width(vin, gfilt, [o for _, o in outs])
    assert chosen == width, "the library runs width %d, the mirror says %d" % (chosen, width)
    assert cabi.filterinterp_forward_nhwc_multi_to(vin, gflows, gfilt, [o for _, o in outs]) == 0
    # the NCHW entry on contiguous copies
    nin = vin.contiguous()
    nouts = [torch.empty_like(nin) for _ in flows]
    assert nin.stride(3) == 1 or w == 1
    assert cabi.filterinterp_forward_ori_multi(nin, [gpu(torch, fl) for fl in flows], gpu(torch, filt), nouts) == 0
    for t, fl in enumerate(flows):
        got = fn.tensor_raw_bits(torch, outs[t][1])
        msg = fn.same_raw_bits(got, fn.raw_bits(fn.expected(oracle, img, fl, filt, bf16), bf16))
        assert not msg, "flow %d vs the oracle (width %d): %s" % (t, width, msg)
        msg = fn.same_raw_bits(got, fn.tensor_raw_bits(torch, nouts[t]))
        assert not msg, "flow %d vs the NCHW entry (width %d): %s" % (t, width, msg)
        assert fn.guard_intact(torch, *outs[t]), "flow %d: written outside the destination" % t
    assert torch.equal(ibuf, ibits), "the image's buffer changed"
    return width


# ------------------------------------------------------------------ channel counts, frames, flows

@pytest.mark.parametrize("C", [2, 3, 7, 8, 9, 196, 199])
@pytest.mark.parametrize("dtype", DTYPES)
def test_channel_counts(torch_mod, cabi, oracle, dtype, C):
    """around the access widths (4 and 2 floats, 8, 4 and 2 bfloat16): dense channels_last, B = 2 with a batch stride larger
    than the image, two flows per call"""
    h, w = FRAME
    rng = np.random.default_rng(100 + C)
    img = _image(rng, (2, C, h, w), dtype == "bfloat16")
    filt = rng.random((2, 16, h, w), dtype=f32)
    flows = [fn.FLOWS[k](rng, 2, h, w) for k in ("subpixel", "borders")]
    width = run_case(torch_mod, cabi, oracle, dtype, img, flows, filt)
    top = 4 if dtype == "float32" else 8
    assert width == max(v for v in (1, 2, 4, 8) if v <= top and C % v == 0)


@pytest.mark.parametrize("h,w", [(3, 3), (5, 6), (1, 9), (9, 1), FRAME])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_frames(torch_mod, cabi, oracle, dtype, B, h, w):
    """frames smaller than a tile (every tap clamped), one row, one column, and 5 x 2 ragged tiles; three flows per call"""
    rng = np.random.default_rng(200 + 10 * h + w + B)
    img = _image(rng, (B, 9, h, w), dtype == "bfloat16")
    filt = rng.random((B, 16, h, w), dtype=f32)
    flows = [fn.FLOWS[k](rng, B, h, w) for k in ("borders", "leaving", "zero")]
    if (h, w) == FRAME:
        c = fn.constants()
        assert -(-h // c["FN_TH"]) >= 2 and -(-w // c["FN_TW"]) >= 2 and h % c["FN_TH"] and w % c["FN_TW"]
        got = set().union(*(fn.flow_features(fl, h, w) for fl in flows))
        assert got >= {"valid", "invalid", "left", "right", "top", "bottom"}, got
    run_case(torch_mod, cabi, oracle, dtype, img, flows, filt, batch_pad=24 if B == 2 else 0)


@pytest.mark.parametrize("kind", sorted(fn.FLOWS))
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_flows(torch_mod, cabi, oracle, dtype, n, kind):
    """each flow field alone and in calls of 1, 2 and 3 flows (different draws of the same kind)"""
    h, w = FRAME
    rng = np.random.default_rng(300 + n)
    img = _image(rng, (1, 8, h, w), dtype == "bfloat16")
    filt = rng.random((1, 16, h, w), dtype=f32) - f32(0.3)
    flows = [fn.FLOWS[kind](rng, 1, h, w) for _ in range(n)]
    run_case(torch_mod, cabi, oracle, dtype, img, flows, filt, batch_pad=0)


# ------------------------------------------------------------------ filter sizes, layouts of flow and filter

@pytest.mark.parametrize("fc", [4, 25, 36, 18, 1, 10])
@pytest.mark.parametrize("dtype", DTYPES)
def test_filter_sizes(torch_mod, cabi, oracle, dtype, fc):
    """fs = 2, 5, 6 (one element per item); 18 filter channels are fs = 4 on the first 16; 1 and 10 channels are fs = 1 and 3"""
    h, w = FRAME
    rng = np.random.default_rng(400 + fc)
    img = _image(rng, (2, 7, h, w), dtype == "bfloat16")
    filt = rng.random((2, fc, h, w), dtype=f32)
    flows = [fn.FLOWS[k](rng, 2, h, w) for k in ("borders", "leaving")]
    run_case(torch_mod, cabi, oracle, dtype, img, flows, filt)


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("fc", [16, 25])
@pytest.mark.parametrize("dtype", DTYPES)
def test_flow_and_filter_layouts(torch_mod, cabi, oracle, dtype, fc, layout):
    h, w = FRAME
    rng = np.random.default_rng(500 + fc)
    img = _image(rng, (2, 12, h, w), dtype == "bfloat16")
    filt = rng.random((2, fc, h, w), dtype=f32)
    flows = [fn.FLOWS[k](rng, 2, h, w) for k in ("subpixel", "borders")]
    run_case(torch_mod, cabi, oracle, dtype, img, flows, filt, ff_layout=layout)


# ------------------------------------------------------------------ destinations

@pytest.mark.parametrize("dst,want", [(None, lambda v: v == 4), ((437, 45), lambda v: v == 1), ((440, 48), lambda v: v == 4)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_destinations(torch_mod, cabi, oracle, dtype, dst, want):
    """C = 196 into a dense channels_last tensor, into channels 45.. of a 437-channel buffer (offset and pixel stride odd: the
    single-element instance) and into channels 48.. of a 440-channel one (vector accesses; the dense 196-channel image
    allows 4 elements: 16 bytes in float32, 8 in bfloat16)"""
    h, w = FRAME
    rng = np.random.default_rng(600)
    img = _image(rng, (2, 196, h, w), dtype == "bfloat16")
    filt = rng.random((2, 16, h, w), dtype=f32)
    flows = [fn.FLOWS[k](rng, 2, h, w) for k in ("borders", "leaving")]
    run_case(torch_mod, cabi, oracle, dtype, img, flows, filt, dst=dst, want_width=want)


@pytest.mark.parametrize("C", [196, 199, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_widest_access_with_a_channel_tail(torch_mod, cabi, oracle, dtype, C):
    """image = channels 8.. of a 216-channel buffer, destinations = channels 48.. of a 440-channel one: 16-byte accesses in
    both dtypes, and for C = 199 / 5 a last chunk of 7 / 5 bfloat16 or 3 / 1 floats handled element by element"""
    h, w = FRAME
    rng = np.random.default_rng(700 + C)
    img = _image(rng, (2, C, h, w), dtype == "bfloat16")
    filt = rng.random((2, 16, h, w), dtype=f32)
    flows = [fn.FLOWS[k](rng, 2, h, w) for k in ("borders", "leaving")]
    top = 4 if dtype == "float32" else 8
    run_case(torch_mod, cabi, oracle, dtype, img, flows, filt, src=(216, 8), dst=(440, 48), want_width=lambda v: v == top)


def test_a_misaligned_base_takes_a_narrower_access(torch_mod, cabi, oracle):
    """the same tensors one element further into their buffers: the base address, not a stride, narrows the access"""
    torch = torch_mod
    h, w = FRAME
    rng = np.random.default_rng(800)
    img = _image(rng, (1, 8, h, w), True)
    filt = rng.random((1, 16, h, w), dtype=f32)
    flow = fn.FLOWS["borders"](rng, 1, h, w)
    want = fn.raw_bits(fn.expected(oracle, img, flow, filt, True), True)
    for off, width in ((64, 8), (68, 4), (66, 2), (65, 1)):
        _, vin = fn.guarded(torch, img.shape, torch.bfloat16, (h * w * 8, 1, w * 8, 8), off)
        fn.cl_fill(torch, vin, img)
        obuf, out = fn.guarded(torch, img.shape, torch.bfloat16, (h * w * 8, 1, w * 8, 8), 64)
        assert fn.vector_width(2, img.shape, fn.tensor_layout(vin), [fn.tensor_layout(out)]) == width
        assert cabi.filterinterp_forward_nhwc_multi_to(vin, [gpu(torch, flow)], gpu(torch, filt), [out]) == 0
        msg = fn.same_raw_bits(fn.tensor_raw_bits(torch, out), want)
        assert not msg, "offset %d: %s" % (off, msg)
        assert fn.guard_intact(torch, obuf, out)


# ------------------------------------------------------------------ non-finite and extreme values

@pytest.mark.parametrize("fs", [4, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_nonfinite_and_extreme_values(torch_mod, cabi, oracle, dtype, fs):
    """+-inf, NaN, +-FLT_MAX, -0.0 and subnormals in the image, the filter taps and the flow (tests/forward_edges
    .small_fi_inputs): NaN stays at the same positions, everything else bit for bit; an invalid pixel copies its bits"""
    rng = np.random.default_rng(900 + fs)
    h, w = FRAME
    img, flow, filt = fe.small_fi_inputs(rng, B=2, C=9, H=h, W=w, fs=fs)
    if dtype == "bfloat16":
        with np.errstate(all="ignore"):
            img = fn.to_bf16(img)
    assert np.isnan(img).any() and np.isinf(img).any() and np.isnan(flow).any() and np.isnan(filt).any()
    run_case(torch_mod, cabi, oracle, dtype, img, [flow, fn.FLOWS["subpixel"](rng, 2, h, w)], filt)


# ------------------------------------------------------------------ fused.FilterInterpolate_ctx_all

def _ctx_case(torch, dtype, seed, B=2, C=12, T=2):
    h, w = FRAME
    rng = np.random.default_rng(seed)
    td = _dtype(torch, dtype)
    ctx = [gpu(torch, _image(rng, (B, C, h, w), dtype == "bfloat16")).to(td) for _ in range(2)]
    offsets = [[gpu(torch, fn.FLOWS[k](rng, B, h, w)) for k in ("borders", "leaving", "subpixel")[:T]] for _ in range(2)]
    filt = [gpu(torch, rng.random((B, 16, h, w), dtype=f32)) for _ in range(2)]
    return ctx, offsets, filt


def _assert_pairs(torch, got, want):
    assert len(got) == len(want)
    for t, (g, r) in enumerate(zip(got, want)):
        for d in range(2):
            assert g[d].dtype == r[d].dtype and g[d].shape == r[d].shape
            assert g[d].is_contiguous(memory_format=torch.channels_last) and g[d].stride(1) == 1, "t=%d d=%d is not channels_last" % (t, d)
            ref = r[d].contiguous(memory_format=torch.channels_last)
            msg = fn.same_raw_bits(fn.tensor_raw_bits(torch, g[d]), fn.tensor_raw_bits(torch, ref))
            assert not msg, "t=%d d=%d: %s" % (t, d, msg)


@pytest.mark.parametrize("ff_layout", ["nchw", "cl"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_ctx_all_on_channels_last(torch_mod, fused, dtype, ff_layout):
    """channels_last contexts in, channels_last tensors out, equal to the NCHW call's channels_last copy; and
    FilterInterpolate_ctx for one time offset"""
    torch = torch_mod
    ctx, offsets, filt = _ctx_case(torch, dtype, 1000)
    want = fused.FilterInterpolate_ctx_all(ctx[0], ctx[1], offsets, filt)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)      # noqa: E731
    if ff_layout == "cl":
        offsets, filt = [[cl(o) for o in d] for d in offsets], [cl(f) for f in filt]
    got = fused.FilterInterpolate_ctx_all(cl(ctx[0]), cl(ctx[1]), offsets, filt)
    _assert_pairs(torch, got, want)
    one = fused.FilterInterpolate_ctx(cl(ctx[0]), cl(ctx[1]), [offsets[0][1], offsets[1][1]], filt)
    _assert_pairs(torch, [one], [want[1]])
    with pytest.raises(RuntimeError, match="forward-only"):
        fused.FilterInterpolate_ctx_all(cl(ctx[0]).requires_grad_(), cl(ctx[1]), offsets, filt)


def test_fused_ctx_all_replays_from_a_graph(torch_mod, fused):
    """the channels_last call allocates and enqueues launches only: captured on one stream, it replays the eager bits"""
    torch = torch_mod
    ctx, offsets, filt = _ctx_case(torch, "bfloat16", 1100, T=3)
    want = fused.FilterInterpolate_ctx_all(ctx[0], ctx[1], offsets, filt)
    c0, c2 = (c.contiguous(memory_format=torch.channels_last) for c in ctx)
    call = lambda: fused.FilterInterpolate_ctx_all(c0, c2, offsets, filt)      # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = call()
    for _ in range(2):
        for pair in got:
            for t in pair:
                t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _assert_pairs(torch, got, want)
    del graph


def test_fused_ctx_all_under_autocast_behind_a_channels_last_convolution(torch_mod, fused):
    """a channels_last convolution under torch.autocast(dtype=torch.bfloat16) stands in for the context network: its output
    goes into the warp as it is -- no cast, no copy -- and the result equals the NCHW call on a .contiguous() copy"""
    torch = torch_mod
    F = torch.nn.functional
    h, w = FRAME
    rng = np.random.default_rng(1200)
    frames = [gpu(torch, rng.random((2, 3, h, w), dtype=f32)).contiguous(memory_format=torch.channels_last) for _ in range(2)]
    weight = gpu(torch, rng.standard_normal((12, 3, 3, 3)) * 0.3).contiguous(memory_format=torch.channels_last)
    _, offsets, filt = _ctx_case(torch, "bfloat16", 1201)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ctx = [F.conv2d(f, weight, padding=1) for f in frames]
        assert all(c.dtype == torch.bfloat16 for c in ctx)
        if not all(c.stride(1) == 1 and c.stride(3) != 1 for c in ctx):
            # (the convolution library chose NCHW for its output: put the stand-in's output into the layout under test)
            ctx = [c.contiguous(memory_format=torch.channels_last) for c in ctx]
        got = fused.FilterInterpolate_ctx_all(ctx[0], ctx[1], offsets, filt)
        want = fused.FilterInterpolate_ctx_all(ctx[0].contiguous(), ctx[1].contiguous(), offsets, filt)
    _assert_pairs(torch, got, want)
