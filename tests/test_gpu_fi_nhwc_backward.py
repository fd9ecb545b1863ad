"""GPU suite (`-m gpu`): the image gradient of the context warp on channels_last tensors,
vfi_filterinterp_backward_ori_nhwc_image_multi[_bf16] (csrc/filterinterp_nhwc_bwd.hip), and fused.FilterInterpolate_ctx_all with
train_channels_last=True.

Common to every kernel-level case (run_case), in float32 and bfloat16: the gradients live in pattern-filled buffers, gradinput1
arrives NaN-filled inside one; every element is written and nothing outside changes; the result is compared as raw BITS with
  the mirror      tests/fi_ctx_backward.predict on the logical NCHW arrays (to_bf16 of it for widened bfloat16 gradients), and
  the NCHW entry  cabi.filterinterp_backward_ori_image_multi on `.contiguous()` copies;
the bits are the same on a second run, with the flows in another order, and from the per-addend kernel alone (direct=True).
The inputs are tests/fi_nhwc_backward's cases: tests/test_fi_nhwc_backward_host.py checks on the CPU that they reach every
tile class (empty, staged on the union window, staged flow by flow, a flow left to the per-addend kernel) and every call class (filter size, fp32 path, second scale factor).
"""
import numpy as np
import pytest

from tests import fi_nhwc_backward as fb
from tests.test_gpu_backward import IMG_ROUNDINGS, U
from tests.test_gpu_parity import cabi, gpu, torch_mod  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

f32 = np.float32
DTYPES = ["float32", "bfloat16"]


@pytest.fixture(scope="module")
def cabi_nhwc(cabi):  # noqa: F811
    from vfidkr_amd import cabi_nhwc as c
    return c


@pytest.fixture(scope="module")
def fused(torch_mod):  # noqa: F811
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import fused as f
    return f


def _ff(torch, a, layout):
    t = gpu(torch, a)
    return t.contiguous(memory_format=torch.channels_last) if layout == "cl" else t


def run_case(torch, cabi, cabi_nhwc, dtype, case, gspec=None, ospec=None, batch_pad=16, ff_layout="nchw", want_width=None,  # noqa: F811
             goffset=64, finite=True):
    """case: logical NCHW numpy arrays (flows, filt, gouts).  gspec / ospec: None for dense channels_last tensors, else (total
    channels, first channel) of the wider channels_last buffer every gradient / gradinput1 is a slice of.  Returns (the
    result's logical NCHW float32 values, the NCHW entry's, the gradients the kernels saw)."""
    bf16 = dtype == "bfloat16"
    td = getattr(torch, dtype)
    flows, filt = case["flows"], case["filt"]
    with np.errstate(all="ignore"):
        gouts = [fb.to_bf16(g) for g in case["gouts"]] if bf16 else case["gouts"]
    B, C, h, w = gouts[0].shape
    n = len(flows)

    def view(spec, offset=64):
        ctot, c0 = (C, 0) if spec is None else spec
        buf, wide = fb.cl_buffer(torch, B, ctot, h, w, td, batch_pad, offset)
        return buf, wide[:, c0:c0 + C]

    gviews = [view(gspec, goffset) for _ in gouts]
    for (_, v), g in zip(gviews, gouts):
        fb.cl_fill(torch, v, g)
    gbits = [buf.clone() for buf, _ in gviews]
    gflows = [_ff(torch, fl, ff_layout) for fl in flows]
    gfilt = _ff(torch, filt, ff_layout)
    gs = [v for _, v in gviews]
    if filt.shape[1] == 16:
        width = fb.vector_width(2 if bf16 else 4, gouts[0].shape, [fb.tensor_layout(g) for g in gs])
        if want_width is not None:
            assert want_width(width), "access width %d" % width
        chosen = cabi_nhwc.filterinterp_nhwc_bwd_access_width(gfilt, gs)
        assert chosen == width, "the library runs width %d, the mirror says %d" % (chosen, width)

    def call(order=range(n), direct=False):
        obuf, out = view(ospec)
        out.fill_(float("nan"))
        assert cabi_nhwc.filterinterp_backward_nhwc_image_multi([gflows[t] for t in order], gfilt, [gs[t] for t in order], out,
                                                                direct=direct) == 0
        assert fb.guard_intact(torch, obuf, out), "written outside gradinput1"
        return fb.tensor_raw_bits(torch, out), out

    got, out = call()
    # the NCHW entry on contiguous copies
    ngs = [g.contiguous() for g in gs]
    nout = torch.full((B, C, h, w), float("nan"), dtype=td, device="cuda:0")
    assert cabi.filterinterp_backward_ori_image_multi([gpu(torch, fl) for fl in flows], gpu(torch, filt), ngs, nout) == 0
    ref = fb.tensor_raw_bits(torch, nout)
    if finite:
        want, _, fp32 = fb.expectation(flows, gouts, filt, bf16)
        assert not fp32
        msg = fb.same_raw_bits(got, fb.raw_bits(want, bf16))
        assert not msg, "against the mirror: %s" % msg
        msg = fb.same_raw_bits(got, ref)
        assert not msg, "against the NCHW entry: %s" % msg
        assert not np.isnan(out.float().cpu().numpy()).any(), "an element was not written"
        msg = fb.same_raw_bits(call()[0], got)
        assert not msg, "second run: %s" % msg
        if n > 1:
            msg = fb.same_raw_bits(call(list(range(n))[::-1])[0], got)
            assert not msg, "flows reversed: %s" % msg
        msg = fb.same_raw_bits(call(direct=True)[0], got)
        assert not msg, "the per-addend kernel alone: %s" % msg
    for (buf, _), bits in zip(gviews, gbits):
        assert torch.equal(buf, bits), "a gradient's buffer changed"
    return out.float().cpu().numpy(), nout.float().cpu().numpy(), gouts


# ------------------------------------------------------------------ channel counts, frames, flows

@pytest.mark.parametrize("C", fb.CHANNELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_channel_counts(torch_mod, cabi, cabi_nhwc, dtype, C):  # noqa: F811
    """slab tails (C no multiple of 16) and width tails (C no multiple of the access width)"""
    top = 4 if dtype == "float32" else 8
    run_case(torch_mod, cabi, cabi_nhwc, dtype, fb.case_channels(C),
             want_width=lambda v: v == max(k for k in (1, 2, 4, 8) if k <= top and C % k == 0))


@pytest.mark.parametrize("h,w", fb.FRAMES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_frames(torch_mod, cabi, cabi_nhwc, dtype, B, h, w):  # noqa: F811
    run_case(torch_mod, cabi, cabi_nhwc, dtype, fb.case_frames(h, w, B), batch_pad=24 if B == 2 else 0)


@pytest.mark.parametrize("kind", sorted(fb.FLOWS))
@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_flows(torch_mod, cabi, cabi_nhwc, dtype, n, kind):  # noqa: F811
    """1, 2 and 3 flows in one launch; four flows take two launches over the same accumulator"""
    run_case(torch_mod, cabi, cabi_nhwc, dtype, fb.case_flows(kind, n), batch_pad=0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_staged_and_direct_tiles_in_one_call(torch_mod, cabi, cabi_nhwc, dtype):  # noqa: F811
    """the builder's field at 43 x 200: windows stretched until they do not fit next to sub-pixel tiles, an empty one, and one
    whose union window does not fit while each flow's own does"""
    case = fb.case_window()
    kinds = {k for group in fb.launches(case["flows"]) for k, _ in fb.tiles(group).values()}
    assert kinds == {"empty", "staged", "staged_split", "direct_window"}
    run_case(torch_mod, cabi, cabi_nhwc, dtype, case)


# ------------------------------------------------------------------ filter sizes, layouts of flow and filter

@pytest.mark.parametrize("fcn", fb.FILTER_CHANNELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_filter_sizes(torch_mod, cabi, cabi_nhwc, dtype, fcn):  # noqa: F811
    run_case(torch_mod, cabi, cabi_nhwc, dtype, fb.case_filter(fcn))


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("fcn", [16, 25])
@pytest.mark.parametrize("dtype", DTYPES)
def test_flow_and_filter_layouts(torch_mod, cabi, cabi_nhwc, dtype, fcn, layout):  # noqa: F811
    run_case(torch_mod, cabi, cabi_nhwc, dtype, fb.case_filter(fcn, C=12), ff_layout=layout)


# ------------------------------------------------------------------ slices

@pytest.mark.parametrize("gspec,ospec,goffset,batch_pad,want", [
    ((437, 45), (437, 45), 64, 16, lambda v: v == 1),               # channels 45.. of 437: one element
    ((440, 48), (440, 48), 64, 16, lambda v: v in (4, 8)),          # channels 48.. of 440: full width
    ((440, 48), None, 65, 16, lambda v: v == 1),                    # one odd element offset
    (None, (437, 45), 64, 24, lambda v: v == 4),                    # dense gradients, a sliced result, a batch pad
    ((440, 48), None, 64, 3, lambda v: v == 1)])                    # an odd batch pad
@pytest.mark.parametrize("dtype", DTYPES)
def test_gradient_and_result_slices(torch_mod, cabi, cabi_nhwc, dtype, gspec, ospec, goffset, batch_pad, want):  # noqa: F811
    run_case(torch_mod, cabi, cabi_nhwc, dtype, fb.case_slices(), gspec=gspec, ospec=ospec, goffset=goffset, batch_pad=batch_pad,
             want_width=want)


# ------------------------------------------------------------------ tiny and non-finite gradients

@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_gradients_take_the_second_scale_factor(torch_mod, cabi, cabi_nhwc, dtype):  # noqa: F811
    case = fb.case_tiny()
    k, fp32, _, scale2 = fb.fc.call_scale(case["gouts"], case["filt"], *fb.FRAME)
    assert k > 126 and not fp32 and scale2 != 1
    run_case(torch_mod, cabi, cabi_nhwc, dtype, case)


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_gradient_lands_where_the_nchw_call_puts_it(torch_mod, cabi, cabi_nhwc, np_oracle, dtype):  # noqa: F811
    """fp32 atomics for the whole call.  Dyadic inputs: every addend and every partial sum is exact in fp32, so the finite cells
    do not depend on the order of the atomics, here or in the NCHW call."""
    case = fb.case_nonfinite()
    with np.errstate(all="ignore"):
        assert fb.fc.call_scale(case["gouts"], case["filt"], *fb.FRAME)[1]
    got, ref, gouts = run_case(torch_mod, cabi, cabi_nhwc, dtype, case, finite=False)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(got).any()
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.isposinf(got).any()
    assert not np.isneginf(got).any() and not np.isneginf(ref).any()
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        S = sum(np_oracle.filterinterp_ori_bwd_img(fl, case["filt"], g)[1] for fl, g in zip(case["flows"], gouts))
    # assert_image_grad's bound without its fixed-point term (no addend is rounded to the integer grid on this path)
    bound = IMG_ROUNDINGS["ori"] * U * S[fin] * (1 + 1e-6) + np.abs(np.spacing(ref[fin]))
    assert np.all(np.abs(got[fin].astype(np.float64) - ref[fin]) <= bound)


# ------------------------------------------------------------------ autograd through fused

def _ctx_case(torch, dtype, seed, B=2, C=12, T=3):
    h, w = fb.FRAME
    rng = np.random.default_rng(seed)
    td = getattr(torch, dtype)
    ctx = [gpu(torch, rng.random((B, C, h, w), dtype=f32) * 2 - 1).to(td) for _ in range(2)]
    offsets = [[gpu(torch, fb.FLOWS[k](rng, B, h, w)) for k in ("borders", "leaving", "subpixel")[:T]] for _ in range(2)]
    filt = [gpu(torch, rng.random((B, 16, h, w), dtype=f32)) for _ in range(2)]
    gs = [[gpu(torch, np.clip(rng.standard_normal((B, C, h, w)), -3, 3)).to(td) for _ in range(T)] for _ in range(2)]
    return ctx, offsets, filt, gs


def _loss(outs, gs, used):
    return sum((outs[t][d].float() * gs[d][t].float()).sum() for t in used for d in range(2))


def _same(torch, got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    msg = fb.same_raw_bits(fb.tensor_raw_bits(torch, got), fb.tensor_raw_bits(torch, want))
    assert not msg, "%s: %s" % (what, msg)


@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_through_fused(torch_mod, fused, dtype):  # noqa: F811
    """keyword set: the gradients of channels_last contexts are, bit for bit, the NCHW Function's on `.contiguous()` contexts --
    with an unused time offset, a channel-slice context, and one direction of each layout"""
    torch = torch_mod
    ctx, offsets, filt, gs = _ctx_case(torch, dtype, 3100)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)      # noqa: E731
    used = (0, 2)                                           # the middle offset arrives as a None gradient
    n0, n2 = (c.clone().requires_grad_() for c in ctx)
    nouts = fused.FilterInterpolate_ctx_all(n0, n2, offsets, filt)
    _loss(nouts, gs, used).backward()
    # dense channels_last contexts
    c0, c2 = (cl(c).requires_grad_() for c in ctx)
    with pytest.raises(RuntimeError, match="forward-only.*contiguous"):
        fused.FilterInterpolate_ctx_all(c0, c2, offsets, filt)
    outs = fused.FilterInterpolate_ctx_all(c0, c2, offsets, filt, train_channels_last=True)
    for (a, b), (na, nb) in zip(outs, nouts):
        assert a.grad_fn is not None and a.stride(1) == 1
        _same(torch, a, na, "forward 0")
        _same(torch, b, nb, "forward 2")
    _loss(outs, gs, used).backward()
    for c, nref, what in ((c0, n0, "ctx0"), (c2, n2, "ctx2")):
        assert c.grad.is_contiguous(memory_format=torch.channels_last) and c.grad.stride(1) == 1
        _same(torch, c.grad, nref.grad, what)
    assert all(o.grad is None for d in offsets for o in d) and all(f.grad is None for f in filt)
    # a channel-slice context, and one direction NCHW and one channels_last
    C = ctx[0].size(1)
    wide = cl(torch.zeros((2, C + 9, *fb.FRAME), dtype=ctx[0].dtype, device="cuda:0"))
    with torch.no_grad():
        wide[:, 5:5 + C].copy_(ctx[0])
    wide.requires_grad_()
    m2 = ctx[1].clone().requires_grad_()
    outs = fused.FilterInterpolate_ctx_all(wide[:, 5:5 + C], m2, offsets, filt, train_channels_last=True)
    assert outs[0][0].stride(1) == 1 and outs[0][1].stride(3) == 1
    _loss(outs, gs, used).backward()
    _same(torch, wide.grad[:, 5:5 + C], n0.grad, "slice context")
    assert not wide.grad[:, :5].any() and not wide.grad[:, 5 + C:].any()
    _same(torch, m2.grad, n2.grad, "NCHW direction next to a channels_last one")
    # the single-offset form
    c0.grad = None
    n0.grad = None
    o0, _ = fused.FilterInterpolate_ctx(c0, c2, [offsets[0][1], offsets[1][1]], filt, train_channels_last=True)
    (o0.float() * gs[0][1].float()).sum().backward()
    r0, _ = fused.FilterInterpolate_ctx(n0, n2, [offsets[0][1], offsets[1][1]], filt)
    (r0.float() * gs[0][1].float()).sum().backward()
    _same(torch, c0.grad, n0.grad, "FilterInterpolate_ctx")


def test_autograd_under_autocast_behind_a_channels_last_convolution(torch_mod, fused):  # noqa: F811
    """a channels_last convolution under torch.autocast(dtype=torch.bfloat16) stands in for the context network: it trains
    through the warp, its weight gradient equal to the one through the NCHW Function on `.contiguous()` contexts"""
    torch = torch_mod
    F = torch.nn.functional
    h, w = fb.FRAME
    rng = np.random.default_rng(3200)
    frames = [gpu(torch, rng.random((2, 3, h, w), dtype=f32)).contiguous(memory_format=torch.channels_last) for _ in range(2)]
    _, offsets, filt, gs = _ctx_case(torch, "bfloat16", 3201)
    grads = {}
    for mode in ("nhwc", "nchw"):
        weight = gpu(torch, np.random.default_rng(3202).standard_normal((12, 3, 3, 3)) * 0.3)
        weight = weight.contiguous(memory_format=torch.channels_last).requires_grad_()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ctx = [F.conv2d(f, weight, padding=1) for f in frames]
            assert all(c.dtype == torch.bfloat16 and c.requires_grad for c in ctx)
            ctx = [c.contiguous(memory_format=torch.channels_last) if mode == "nhwc" else c.contiguous() for c in ctx]
            assert all((c.stride(1) == 1 and c.stride(3) != 1) == (mode == "nhwc") for c in ctx)
            for c in ctx:
                c.retain_grad()
            outs = fused.FilterInterpolate_ctx_all(ctx[0], ctx[1], offsets, filt, train_channels_last=mode == "nhwc")
        _loss(outs, gs, (0, 1, 2)).backward()
        grads[mode] = [c.grad for c in ctx] + [weight.grad]
    for got, want, what in zip(grads["nhwc"][:2], grads["nchw"][:2], ("ctx0", "ctx2")):
        assert got.dtype == torch.bfloat16                   # (a retained gradient's layout is autograd's choice)
        _same(torch, got, want, what)
    assert torch.isfinite(grads["nhwc"][2]).all() and grads["nhwc"][2].abs().max() > 0
    # (the convolution's weight gradient goes through the convolution library in two layouts: close, not bit-equal)
    assert torch.allclose(grads["nhwc"][2], grads["nchw"][2], rtol=2e-2, atol=2e-2 * float(grads["nchw"][2].abs().max()))


def test_forward_and_backward_replay_from_a_graph(torch_mod, fused):  # noqa: F811
    """forward + backward captured in one torch.cuda.graph on a side stream after a warm-up there: every replay the eager bits"""
    torch = torch_mod
    ctx, offsets, filt, gs = _ctx_case(torch, "bfloat16", 3300)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)      # noqa: E731
    c0, c2 = (cl(c).requires_grad_() for c in ctx)

    def step():
        outs = fused.FilterInterpolate_ctx_all(c0, c2, offsets, filt, train_channels_last=True)
        _loss(outs, gs, (0, 1, 2)).backward()
    step()
    torch.cuda.synchronize()
    want = [c0.grad.clone(), c2.grad.clone()]
    c0.grad = c2.grad = None
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                                  # warm-up on the capture stream
            step()
            c0.grad = c2.grad = None
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    got = [c0.grad, c2.grad]
    for turn in range(3):
        for g in got:
            g.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for g, r, what in zip(got, want, ("ctx0", "ctx2")):
            _same(torch, g, r, "replay %d, %s" % (turn, what))
    del graph
