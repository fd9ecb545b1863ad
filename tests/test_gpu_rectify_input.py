"""GPU suite (`-m gpu`): the FilterInterpolation forward writing into a destination with a layout of its own
(vfi_filterinterp_forward_ori_multi_to, vfi_filterinterp_blend_forward with a strided s_out) and fused.rectify_inputs.

The kernels must write the bits of the dense call, into the slice and nowhere else: every destination is a channel slice
at a non-zero offset of a wider buffer pre-filled with a bit pattern, compared as integers.  Fields come from
tests/fi_windows.py, so that every window class of every staged kernel writes through the second set of strides.
fused.rectify_inputs is compared bit for bit with the composition it replaces (tests/rectify_input.py)."""
import ctypes

import numpy as np
import pytest

from tests import fi_windows as fw
from tests import rectify_input as ri

pytestmark = pytest.mark.gpu

f32 = np.float32
PATTERN = 0x7FC0BEEF          # a NaN no kernel produces


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("`-m gpu` tests need a GPU: torch.cuda.is_available() is False")
    return torch


@pytest.fixture(scope="module")
def cabi(torch_mod):
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi as c
    assert "gfx950" in c.version()
    return c


@pytest.fixture(scope="module")
def fused(cabi):
    from vfidkr_amd import fused as f
    return f


def gpu(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to("cuda:0")


class Wide:
    """A [B, Cw, h, w] buffer holding PATTERN; slices of it are the destinations.  every_other: the slice takes every
    second channel (its channel stride is two planes)."""

    def __init__(self, torch, B, Cw, h, w):
        self.torch = torch
        self.buf = torch.full((B, Cw, h, w), PATTERN, dtype=torch.int32, device="cuda:0").view(torch.float32)
        self.taken = torch.zeros(Cw, dtype=torch.bool)

    def slice(self, first, C, every_other=False):
        idx = slice(first, first + 2 * C, 2) if every_other else slice(first, first + C)
        assert not self.taken[idx].any()
        self.taken[idx] = True
        return self.buf[:, idx]

    def check_rest(self, what):
        torch = self.torch
        rest = self.buf[:, ~self.taken.to("cuda:0")]
        bad = int((rest.contiguous().view(torch.int32) != PATTERN).sum())
        assert bad == 0, "%s: %d elements written outside the destination slices" % (what, bad)


def same_bits(torch, what, got, ref, pix=None):
    g, r = got.contiguous().view(torch.int32), ref.contiguous().view(torch.int32)
    if torch.equal(g, r):
        return
    bad = (g != r).any(1).cpu().numpy()
    msg = "%s: %d pixels differ" % (what, int(bad.sum()))
    if pix is not None:
        msg += " in classes " + ", ".join("%s (%d)" % (k, int((bad & (pix == k)).sum())) for k in sorted(set(pix[bad].ravel())))
    raise AssertionError(msg)


def _inputs(rng, B, C, h, w, taps):
    return rng.random((B, C, h, w), dtype=f32), rng.random((B, taps, h, w), dtype=f32)


# ------------------------------------------------------------------ vfi_filterinterp_forward_ori_multi_to, per window class

@pytest.mark.parametrize("C", [1, 3, 9])
@pytest.mark.parametrize("kernel,fs", [("lds", 4), ("multi", 4), ("n", 2), ("n", 5), ("n", 6)])
def test_multi_to_every_window_class(torch_mod, cabi, kernel, fs, C):
    """Every window class of the fs = 4 kernel (one flow), of the shared-window kernel (two flows) and of the fs 2 / 5 / 6
    kernel, gather fallbacks and empty tiles included: the slice holds the dense call's bits, the rest of the buffer its
    pattern.  C = 9: several channel groups per tile."""
    torch = torch_mod
    h, w = fw.field_shape(kernel)
    rng = np.random.default_rng(7000 + 10 * fs + C + len(kernel))
    f = fw.build_field(kernel, rng, 2, h, w, fs=fs)
    if kernel == "multi":
        lab = fw.classes("multi", f["flow"], h, w, flow2=f["flow2"])
        flows_np = [f["flow"], f["flow2"]]
    else:
        lab = fw.classes(kernel, f["flow"], h, w, fs=fs)
        flows_np = [f["flow"]]
    assert set(fw.all_classes(kernel)) <= set(lab.ravel())
    pix = fw.pixel_labels(kernel, lab, h, w, fs)
    img, filt = _inputs(rng, 2, C, h, w, fs * fs)
    gi, gk, flows = gpu(torch, img), gpu(torch, filt), [gpu(torch, x) for x in flows_np]
    if kernel == "lds":
        assert fw.aligned16(gi)                                        # the 16-byte staging classes are in the field
    dense = [torch.empty_like(gi) for _ in flows]
    assert cabi.filterinterp_forward_ori_multi(gi, flows, gk, dense) == 0
    wides = [Wide(torch, 2, C + 5, h, w) for _ in flows]
    dst = [wd.slice(3, C) for wd in wides]
    assert dst[0].stride(1) == gi.stride(1) and dst[0].stride(0) != gi.stride(0) and dst[0].data_ptr() != wides[0].buf.data_ptr()
    assert cabi.filterinterp_forward_ori_multi_to(gi, flows, gk, dst) == 0
    for t, (wd, d, ref) in enumerate(zip(wides, dst, dense)):
        same_bits(torch, "%s fs=%d C=%d flow %d" % (kernel, fs, C, t), d, ref, pix)
        wd.check_rest("%s fs=%d C=%d flow %d" % (kernel, fs, C, t))


# ------------------------------------------------------------------ strides, alignment, flow counts

def _smooth(rng, B, h, w, amp=4.0):
    yy, xx = np.meshgrid(np.arange(h, dtype=f32), np.arange(w, dtype=f32), indexing="ij")
    ph = rng.uniform(0, 6.28, 4)
    fx = amp * np.sin(xx / 9.0 + ph[0]) * np.cos(yy / 7.0 + ph[1]) + rng.uniform(-0.5, 0.5, (B, h, w))
    fy = amp * np.cos(xx / 8.0 + ph[2]) * np.sin(yy / 11.0 + ph[3]) + rng.uniform(-0.5, 0.5, (B, h, w))
    return np.stack([fx, fy], axis=1).astype(f32)


@pytest.mark.parametrize("nflows", [1, 2, 3])
@pytest.mark.parametrize("layout", ["strided input", "strided destination", "odd width"])
@pytest.mark.parametrize("fcn", [16, 25])
def test_multi_to_strides_and_flow_counts(torch_mod, cabi, fcn, layout, nflows):
    """The two sets of strides differ in the channel AND the batch stride (with both tensors contiguous the channel strides
    coincide, and a kernel that stored with the input's would pass):
      strided input:       input1 is an every-other-channel view of a larger tensor, the destination a plain channel slice
      strided destination: input1 is contiguous, the destination takes every other channel of the buffer
      odd width:           h x w odd and a slice starting at channel 1: the destination is 4-byte aligned and no more
    for 1, 2 and 3 flows (3 = a two-flow launch and a single one), fs = 4 and fs = 5.  37 x 139: three tile columns, a ragged
    last tile."""
    torch = torch_mod
    B, C, h, w = 2, 5, 37, (139 if layout == "odd width" else 140)
    rng = np.random.default_rng(8000 + fcn + nflows + len(layout))
    img, filt = _inputs(rng, B, 2 * C, h, w, fcn)
    big = gpu(torch, img)
    gi = big[:, ::2] if layout == "strided input" else big[:, :C].contiguous()
    gk = gpu(torch, filt)
    flows = [gpu(torch, _smooth(rng, B, h, w)) for _ in range(nflows)]
    dense = [torch.empty_strided(gi.shape, gi.stride(), dtype=gi.dtype, device=gi.device) for _ in flows]
    assert cabi.filterinterp_forward_ori_multi(gi, flows, gk, dense) == 0
    wides = [Wide(torch, B, 2 * C + 3, h, w) for _ in flows]
    dst = [wd.slice(1, C, every_other=(layout == "strided destination")) for wd in wides]
    assert dst[0].stride(1) != gi.stride(1) or layout == "odd width"
    assert dst[0].stride(0) != gi.stride(0) and dst[0].stride(2) == gi.stride(2)
    if layout == "odd width":
        assert dst[0].data_ptr() % 8 == 4
    assert cabi.filterinterp_forward_ori_multi_to(gi, flows, gk, dst) == 0
    for t, (wd, d, ref) in enumerate(zip(wides, dst, dense)):
        same_bits(torch, "%s fcn=%d flow %d of %d" % (layout, fcn, t, nflows), d, ref)
        wd.check_rest("%s fcn=%d flow %d of %d" % (layout, fcn, t, nflows))


def test_other_row_stride_is_refused_not_rerouted(torch_mod, cabi):
    """a destination whose rows are farther apart than input1's: the binding and the library both say 1, nothing is written"""
    torch = torch_mod
    B, C, h, w = 1, 3, 16, 64
    gi = torch.rand(B, C, h, w, device="cuda:0")
    flow, gk = torch.zeros(B, 2, h, w, device="cuda:0"), torch.rand(B, 16, h, w, device="cuda:0")
    pad = torch.full((B, C + 2, h, w + 4), PATTERN, dtype=torch.int32, device="cuda:0").view(torch.float32)
    dst = pad[:, 1:1 + C, :, :w]
    assert cabi.filterinterp_forward_ori_multi_to(gi, [flow], gk, [dst]) == 1
    for n in (1, 2):
        tab = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])     # noqa: E731
        with torch.cuda.device(0):
            err = cabi.lib().vfi_filterinterp_forward_ori_multi_to(
                cabi._ptr(gi), tab([flow] * n), cabi._ptr(gk), tab([dst] * n), n, B, C, h, w, 16, cabi._st(gi), cabi._st(flow),
                cabi._st(gk), cabi._st(dst), cabi._stream(gi))
        assert err == cabi.VFI_ERR_SHAPE
    torch.cuda.synchronize()
    assert int((pad.view(torch.int32) != PATTERN).sum()) == 0


# ------------------------------------------------------------------ vfi_filterinterp_blend_forward with a strided s_out

@pytest.mark.parametrize("C", [1, 3, 4, 5])
@pytest.mark.parametrize("outs", ["all", "blend only"])
def test_blend_forward_into_slices(torch_mod, cabi, C, outs):
    """blend, out0 and out2 as three channel slices of ONE buffer (how rectify_inputs calls it), on a field that sends the
    blend epilogue through every window class; C = 5 is above the epilogue's channel limit (staged kernels + the blend
    launch); `blend only` (out0 / out2 NULL) is the per-pixel gather kernel.  Bit-equal to the call with dense outputs."""
    torch = torch_mod
    h, w = fw.field_shape("blend")
    rng = np.random.default_rng(9000 + C)
    f0, f2 = fw.build_field("blend", rng, 2, h, w), fw.build_field("blend", rng, 2, h, w)
    lab = fw.classes("blend", f2["flow"], h, w)
    assert set(fw.all_classes("blend")) <= set(lab.ravel())
    pix = fw.pixel_labels("blend", lab, h, w)
    ref0, filt0 = _inputs(rng, 2, C, h, w, 16)
    ref2, filt2 = _inputs(rng, 2, C, h, w, 16)
    args = tuple(gpu(torch, a) for a in (ref0, ref2, f0["flow"], f2["flow"], filt0, filt2))
    w0, w2 = 0.75, 0.25
    dense = [torch.empty_like(args[0]) for _ in range(3)]
    wide = Wide(torch, 2, 3 * C + 4, h, w)
    if outs == "all":
        dst = [wide.slice(2 + k * C, C) for k in range(3)]
        assert cabi.filterinterp_blend_forward(*args, *dense, w0, w2) == 0
        assert cabi.filterinterp_blend_forward(*args, *dst, w0, w2) == 0
    else:
        dst = [wide.slice(2, C), None, None]
        assert cabi.filterinterp_blend_forward(*args, dense[0], None, None, w0, w2) == 0
        assert cabi.filterinterp_blend_forward(*args, dst[0], None, None, w0, w2) == 0
    for name, d, ref in zip(("blend", "out0", "out2"), dst, dense):
        if d is not None:
            same_bits(torch, "C=%d %s %s" % (C, outs, name), d, ref, pix)
    wide.check_rest("C=%d %s" % (C, outs))


# ------------------------------------------------------------------ fused.rectify_inputs

SHAPE = (2, 40, 136)            # B, H, W: three tile columns and rows, ragged last tiles


@pytest.mark.parametrize("T,cctx", [(1, None), (1, 6), (3, 6)])
def test_rectify_inputs_forward(torch_mod, fused, T, cctx):
    torch = torch_mod
    B, H, W = SHAPE
    times = [0.5] if T == 1 else [0.25, 0.5, 0.75]
    ref0, ref2, offs, filt, ctx0, ctx2 = ri.smooth_inputs(torch, np.random.default_rng(100 + T), B, H, W, T, cctx)
    want = ri.composition(torch, fused, ref0, ref2, offs, filt, 16, times, ctx0, ctx2)
    got = fused.rectify_inputs(ref0, ref2, offs, filt, 16, times, ctx0, ctx2)
    m = ri.channel_map(16, cctx)
    assert len(got) == T
    for t, ((buf, cur), (rbuf, rcur)) in enumerate(zip(got, want)):
        assert buf.shape == (B, m["total"], H, W) and buf.is_contiguous() and buf.grad_fn is None
        assert cur.data_ptr() == buf.data_ptr() and cur.shape == (B, 3, H, W)           # the view rectify_input_t[:, :3]
        for name in (k for k in m if k != "total"):
            a, b = m[name]
            same_bits(torch, "T=%d t=%d %s" % (T, t, name), buf[:, a:b], rbuf[:, a:b])
        same_bits(torch, "T=%d t=%d cur_output" % (T, t), cur, rcur)


def _train(torch, tensors):
    for t in tensors:
        if t is not None:
            t.requires_grad_()


def _grads(tensors):
    return [None if t is None or t.grad is None else t.grad.clone() for t in tensors]


@pytest.mark.parametrize("variant", ["all", "cur_output unused", "context without grad", "no context"])
def test_rectify_inputs_backward_one_time_offset(torch_mod, fused, variant):
    """T = 1: every gradient equals autograd's through torch.cat over the existing fused functions, bit for bit"""
    torch = torch_mod
    B, H, W = SHAPE
    rng = np.random.default_rng(200)
    cctx = None if variant == "no context" else 6
    ref0, ref2, offs, filt, ctx0, ctx2 = ri.smooth_inputs(torch, rng, B, H, W, 1, cctx)
    leaves = [ref0, ref2, offs[0][0], offs[1][0], filt[0], filt[1]] + ([] if variant == "context without grad" else [ctx0, ctx2])
    _train(torch, leaves)
    everything = [ref0, ref2, offs[0][0], offs[1][0], filt[0], filt[1], ctx0, ctx2]
    m = ri.channel_map(16, cctx)
    wb = gpu(torch, rng.standard_normal((B, m["total"], H, W)))
    wc = gpu(torch, rng.standard_normal((B, 3, H, W)))

    def loss(pairs):
        buf, cur = pairs[0]
        total = (buf * wb).sum()
        return total if variant == "cur_output unused" else total + (cur * wc).sum()

    loss(ri.composition(torch, fused, ref0, ref2, offs, filt, 16, [0.5], ctx0, ctx2)).backward()
    want = _grads(everything)
    for t in everything:
        if t is not None:
            t.grad = None
    pairs = fused.rectify_inputs(ref0, ref2, offs, filt, 16, [0.5], ctx0, ctx2)
    assert pairs[0][0].grad_fn is not None and pairs[0][1].data_ptr() != pairs[0][0].data_ptr()
    loss(pairs).backward()
    got = _grads(everything)
    names = ("ref0", "ref2", "offset0", "offset1", "filter0", "filter1", "ctx0", "ctx2")
    for name, g, r in zip(names, got, want):
        assert (g is None) == (r is None), (variant, name)
        if g is not None:
            same_bits(torch, "%s: grad %s" % (variant, name), g, r)
    assert got[0] is not None and (got[6] is None) == (variant in ("context without grad", "no context"))


@pytest.mark.parametrize("variant", ["all", "buffer 1 unused", "cur_output unused"])
def test_rectify_inputs_backward_three_time_offsets(torch_mod, fused, variant):
    """T = 3: the documented order -- per flow kernel term + passed-through slice; per filter and frame the left-to-right
    sum over t ascending of (kernel term, slice); per context tensor one call over the live time offsets"""
    torch = torch_mod
    B, H, W = SHAPE
    rng = np.random.default_rng(300)
    times = [0.25, 0.5, 0.75]
    ref0, ref2, offs, filt, ctx0, ctx2 = ri.smooth_inputs(torch, rng, B, H, W, 3, 6)
    everything = [ref0, ref2, filt[0], filt[1], ctx0, ctx2] + offs[0] + offs[1]
    _train(torch, everything)
    m = ri.channel_map(16, 6)
    wb = [gpu(torch, rng.standard_normal((B, m["total"], H, W))) for _ in times]
    wc = [gpu(torch, rng.standard_normal((B, 3, H, W))) for _ in times]
    if variant == "buffer 1 unused":
        wb[1] = None
    if variant == "cur_output unused":
        wc = [None] * 3
    pairs = fused.rectify_inputs(ref0, ref2, offs, filt, 16, times, ctx0, ctx2)
    total = 0
    for (buf, cur), b, c in zip(pairs, wb, wc):
        total = total + (0 if b is None else (buf * b).sum()) + (0 if c is None else (cur * c).sum())
    total.backward()
    with torch.enable_grad():
        want = ri.expected_gradients(torch, fused, ref0.detach(), ref2.detach(), [[o.detach() for o in d] for d in offs],
                                     [k.detach() for k in filt], 16, times, ctx0.detach(), ctx2.detach(), wb, wc)
    for name, t in (("ref0", ref0), ("ref2", ref2), ("filter0", filt[0]), ("filter1", filt[1]), ("ctx0", ctx0), ("ctx2", ctx2)):
        same_bits(torch, "%s: grad %s" % (variant, name), t.grad, want[name])
    for d in (0, 1):
        for t in range(3):
            same_bits(torch, "%s: grad offset%d[%d]" % (variant, d, t), offs[d][t].grad, want["offset%d" % d][t])


def test_rectify_inputs_replays_from_a_graph(torch_mod, fused):
    """the forward allocates its buffers and enqueues launches and copies only: captured once, it replays the same bits"""
    torch = torch_mod
    B, H, W = SHAPE
    times = [0.25, 0.5, 0.75]
    ref0, ref2, offs, filt, ctx0, ctx2 = ri.smooth_inputs(torch, np.random.default_rng(400), B, H, W, 3, 6)
    want = [buf.clone() for buf, _ in fused.rectify_inputs(ref0, ref2, offs, filt, 16, times, ctx0, ctx2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused.rectify_inputs(ref0, ref2, offs, filt, 16, times, ctx0, ctx2)          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = fused.rectify_inputs(ref0, ref2, offs, filt, 16, times, ctx0, ctx2)
    for _ in range(2):
        for buf, _cur in got:
            buf.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for t, ((buf, cur), ref) in enumerate(zip(got, want)):
            same_bits(torch, "replay t=%d" % t, buf, ref)
            same_bits(torch, "replay t=%d cur_output" % t, cur, ref[:, 0:3])
    del graph
