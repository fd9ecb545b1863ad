"""CPU checks of the destination-layout forward (vfi_filterinterp_forward_ori_multi_to) and of fused.rectify_inputs:

  * the header declares the entry point, libvfi_hip.so exports it, cabi knows its 15 arguments, and argument errors -- a
    destination row stride unlike input1's among them -- return 1 before any launch;
  * cabi.filterinterp_forward_ori_multi_to refuses an h stride unlike input1's, a w stride other than 1, lists of unequal
    length and CPU tensors;
  * the channel map is the reference's for no context tensors, 1 and 196 context channels, and fused.rectify_channels agrees;
  * fused.rectify_inputs hands channel slices of one contiguous buffer per time offset to the frame kernel and to ONE
    multi-flow call per direction, copies flows and filters into their channels, returns a view of the buffer for
    cur_output in inference and a dense output of its own in training, saves neither buffers nor context tensors, and its
    backward sums in the documented order (launches stubbed).
"""
import ctypes
import os
import re

import pytest
import torch

from tests import rectify_input as ri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vfi_filterinterp_forward_ori_multi_to"


@pytest.fixture(scope="module")
def built():
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import build
    build.build_all()
    return build


def test_header_declares_and_library_exports_the_entry_point(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vfi_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, text)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    dense = re.search(r"\bint\s+vfi_filterinterp_forward_ori_multi\s*\(([^)]*)\)", text).group(1)
    dense = [" ".join(a.split()) for a in dense.split(",")]
    assert args == dense[:-1] + ["vfi_strides s_out", dense[-1]]          # the dense entry's arguments plus the destination's strides
    lib = ctypes.CDLL(built.LIB_PATH)
    assert hasattr(lib, NAME)
    from vfidkr_amd import cabi
    assert len(cabi.SIGNATURES[NAME]) == len(args) == 15
    assert cabi.SIGNATURES[NAME] == cabi.SIGNATURES["vfi_filterinterp_forward_ori_multi"][:-1] + [cabi.Strides, ctypes.c_void_p]
    assert callable(cabi.filterinterp_forward_ori_multi_to)


def test_argument_errors_return_1_without_a_gpu(built):
    from vfidkr_amd import cabi
    f = getattr(cabi.lib(), NAME)
    s = cabi.Strides(192, 64, 8)
    p = ctypes.c_void_p(16)                 # never dereferenced: every call below returns before any launch
    two = (ctypes.c_void_p * 2)(16, 16)
    hole = (ctypes.c_void_p * 2)(16, None)

    def call(flows=two, filt=p, outs=two, img=p, n=2, dims=(1, 3, 8, 8), fcn=16, so=cabi.Strides(640, 64, 9)):
        return f(img, flows, filt, outs, n, *dims, fcn, s, s, s, so, None)
    # a destination whose rows are not as far apart as input1's: refused, for every filter size and flow count
    for fcn in (16, 4, 25, 36, 7):
        for n in (1, 2):
            assert call(fcn=fcn, n=n) == 1
    assert call(so=cabi.Strides(192, 64, 0)) == 1 and call(so=cabi.Strides(192, 64, -8)) == 1
    ok = cabi.Strides(640, 64, 8)
    assert call(flows=None, so=ok) == 1 and call(outs=None, so=ok) == 1 and call(filt=None, so=ok) == 1 and call(img=None, so=ok) == 1
    assert call(flows=hole, so=ok) == 1 and call(outs=hole, so=ok) == 1
    assert call(n=0, so=ok) == 1 and call(n=-1, so=ok) == 1 and call(fcn=0, so=ok) == 1
    for dims in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1)):
        assert call(dims=dims, so=ok) == 1


def test_binding_refusals():
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi
    B, C, H, W = 2, 3, 6, 16
    img, filt = torch.rand(B, C, H, W), torch.rand(B, 16, H, W)
    flows = [torch.rand(B, 2, H, W) for _ in range(2)]
    wide = [torch.zeros(B, 9, H, W) for _ in range(2)]
    good = [b[:, 4:7] for b in wide]
    call = cabi.filterinterp_forward_ori_multi_to
    # rows of the destination farther apart than input1's
    padded = [torch.zeros(B, 9, H, W + 4)[:, 4:7, :, :W] for _ in range(2)]
    assert padded[0].shape == img.shape and call(img, flows, filt, padded) == 1
    # ... and the other way round: a padded image, a dense destination
    assert call(torch.rand(B, C, H, W + 4)[..., :W], flows, filt, good) == 1
    # w stride 2
    assert call(img, flows, filt, [torch.zeros(B, 9, H, 2 * W)[:, 4:7, :, ::2] for _ in range(2)]) == 1
    assert call(img[..., ::2], [f[..., ::2] for f in flows], filt[..., ::2], [g[..., ::2] for g in good]) == 1
    # list lengths, shapes, destinations of two layouts
    assert call(img, flows, filt, good[:1]) == 1 and call(img, flows[:1], filt, good) == 1 and call(img, [], filt, []) == 1
    assert call(img, flows, filt, [good[0], wide[1][:, 4:8]]) == 1
    assert call(img, flows, filt, [good[0], torch.zeros(B, 12, H, W)[:, 4:7]]) == 1
    assert call(img, [flows[0], torch.rand(B, 2, H, W + 1)], filt, good) == 1
    # CPU tensors that pass every layout check: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        call(img, flows, filt, good)


@pytest.mark.parametrize("cctx", [None, 1, 196])
def test_channel_map(cctx):
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import fused
    m = ri.channel_map(16, cctx)
    assert m == fused.rectify_channels(16, cctx)
    c = cctx or 0
    assert m["total"] == 45 + 2 * c == {None: 45, 1: 47, 196: 437}[cctx]
    assert (m["cur_output"], m["ref0"], m["ref2"]) == ((0, 3), (3, 6), (6, 9))
    assert (m["offset0"], m["offset1"], m["filter0"], m["filter1"]) == ((9, 11), (11, 13), (13, 29), (29, 45))
    if cctx:
        assert (m["ctx0"], m["ctx2"]) == ((45, 45 + c), (45 + c, 45 + 2 * c))
    else:
        assert "ctx0" not in m and "ctx2" not in m
    # the order of networks/DAIN_slowmotion.py:177-181: the map's ranges tile [0, total) in that order
    names = ["cur_output", "ref0", "ref2", "offset0", "offset1", "filter0", "filter1"] + (["ctx0", "ctx2"] if cctx else [])
    at = 0
    for n in names:
        assert m[n][0] == at
        at = m[n][1]
    assert at == m["total"]
    assert ri.channel_map(36)["total"] == 13 + 72


# ------------------------------------------------------------------ fused.rectify_inputs, launches stubbed

class _Stub:
    """Stands in for the four launches: fills what the kernels write with values that name the call."""

    def __init__(self):
        self.blend, self.ctx, self.blend_bwd, self.ctx_bwd = [], [], [], []

    def blend_forward(self, ref0, ref2, f0, f2, k0, k2, blend, out0, out2, w0, w2):
        self.blend.append((blend, out0, out2, w0, w2, f0, f2))
        blend.fill_(100.0 + len(self.blend)), out0.fill_(200.0 + len(self.blend)), out2.fill_(300.0 + len(self.blend))
        return 0

    def multi_to(self, image, flows, filt, outs):
        self.ctx.append((image, list(flows), filt, list(outs)))
        for t, o in enumerate(outs):
            o.fill_(1000.0 * len(self.ctx) + t)
        return 0

    def blend_backward(self, ref0, ref2, f0, f2, k0, k2, g_blend, g_out0, g_out2, w0, w2, gr0, gr2, gf0, gf2, gk0, gk2):
        n = len(self.blend_bwd) + 1
        self.blend_bwd.append((g_blend, g_out0, g_out2, w0, w2, f0, f2, (gr0, gr2, gf0, gf2, gk0, gk2)))
        for i, o in enumerate((gr0, gr2, gf0, gf2, gk0, gk2)):
            if o is not None:
                o.fill_(10.0 * n + i)
        return 0

    def image_multi(self, flows, filt, gouts, g1):
        self.ctx_bwd.append((list(flows), filt, list(gouts)))
        g1.fill_(7.0 * len(self.ctx_bwd))
        return 0


@pytest.fixture
def stubbed(monkeypatch):
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi, fused
    stub = _Stub()
    monkeypatch.setattr(cabi, "filterinterp_blend_forward", stub.blend_forward)
    monkeypatch.setattr(cabi, "filterinterp_forward_ori_multi_to", stub.multi_to)
    monkeypatch.setattr(cabi, "filterinterp_blend_backward", stub.blend_backward)
    monkeypatch.setattr(cabi, "filterinterp_backward_ori_image_multi", stub.image_multi)
    return fused, stub


def _inputs(T, cctx, B=2, H=5, W=6):
    ref0, ref2 = torch.rand(B, 3, H, W), torch.rand(B, 3, H, W)
    offs = [[torch.rand(B, 2, H, W) for _ in range(T)] for _ in range(2)]
    filts = [torch.rand(B, 16, H, W) for _ in range(2)]
    ctx = [torch.rand(B, cctx, H, W) for _ in range(2)] if cctx else [None, None]
    return ref0, ref2, offs, filts, ctx[0], ctx[1]


def _is_slice(view, buf, rng):
    ref = buf[:, rng[0]:rng[1]]
    return view.data_ptr() == ref.data_ptr() and view.shape == ref.shape and view.stride() == ref.stride()


@pytest.mark.parametrize("cctx", [None, 4])
def test_inference_writes_slices_of_one_buffer_per_time_offset(stubbed, monkeypatch, cctx):
    fused, stub = stubbed

    def refuse(*a, **k):
        raise AssertionError("the autograd Function was reached")
    monkeypatch.setattr(fused._RectifyInputs, "apply", refuse)
    times = [0.25, 0.5, 0.75]
    ref0, ref2, offs, filts, ctx0, ctx2 = _inputs(3, cctx)
    out = fused.rectify_inputs(ref0, ref2, offs, filts, 16, times, ctx0, ctx2)
    m = ri.channel_map(16, cctx)
    assert len(out) == 3 and len(stub.blend) == 3 and len(stub.ctx) == (2 if cctx else 0)
    for t, (buf, cur) in enumerate(out):
        assert buf.shape == (2, m["total"], 5, 6) and buf.is_contiguous() and buf.grad_fn is None
        assert _is_slice(cur, buf, m["cur_output"])                          # a view, not a copy
        blend, out0, out2, w0, w2, f0, f2 = stub.blend[t]
        assert _is_slice(blend, buf, m["cur_output"]) and _is_slice(out0, buf, m["ref0"]) and _is_slice(out2, buf, m["ref2"])
        assert (w0, w2) == (1.0 - times[t], times[t]) and f0 is offs[0][t] and f2 is offs[1][t]
        assert torch.equal(buf[:, 9:11], offs[0][t]) and torch.equal(buf[:, 11:13], offs[1][t])
        assert torch.equal(buf[:, 13:29], filts[0]) and torch.equal(buf[:, 29:45], filts[1])
        assert (buf[:, 0:3] == 101.0 + t).all() and (buf[:, 3:6] == 201.0 + t).all() and (buf[:, 6:9] == 301.0 + t).all()
    if cctx:
        for d, name in enumerate(("ctx0", "ctx2")):                           # one call per direction, every time offset in it
            image, flows, filt, outs = stub.ctx[d]
            assert image is (ctx0, ctx2)[d] and filt is filts[d] and all(a is b for a, b in zip(flows, offs[d]))
            assert len(outs) == 3 and all(_is_slice(o, out[t][0], m[name]) for t, o in enumerate(outs))
    with pytest.raises(RuntimeError):
        fused.rectify_inputs(ref0, ref2, offs, filts, 16, times, torch.rand(2, 4, 5, 6), None)


def test_training_returns_dense_cur_output_and_sums_in_the_documented_order(stubbed):
    fused, stub = stubbed
    times = [0.25, 0.5, 0.75]
    ref0, ref2, offs, filts, ctx0, ctx2 = _inputs(3, 4)
    for t in [ref0, filts[0], filts[1], ctx0] + offs[0] + offs[1]:
        t.requires_grad_()
    with torch.no_grad():                                                   # grad mode off: the plain launches
        assert all(b.grad_fn is None for b, _ in fused.rectify_inputs(ref0, ref2, offs, filts, 16, times, ctx0, ctx2))
    stub.__init__()
    out = fused.rectify_inputs(ref0, ref2, offs, filts, 16, times, ctx0, ctx2)
    m = ri.channel_map(16, 4)
    fn = out[0][0].grad_fn
    assert fn is not None and all(b.grad_fn is fn and c.grad_fn is fn for b, c in out)      # ONE Function over all time offsets
    for buf, cur in out:
        assert cur.shape == (2, 3, 5, 6) and cur.is_contiguous() and cur.data_ptr() != buf.data_ptr()
        assert torch.equal(cur, buf[:, 0:3])
    # saved: frames, filters, flows -- no buffer, no context tensor
    assert sorted(tuple(t.shape)[1] for t in fn.saved_tensors) == [2] * 6 + [3, 3, 16, 16]
    # gradients: buffers 0 and 2 and cur_output 0 and 1 are used; buffer 1 is not
    g0, g2 = torch.rand(2, m["total"], 5, 6), torch.rand(2, m["total"], 5, 6)
    c0, c1 = torch.rand(2, 3, 5, 6), torch.rand(2, 3, 5, 6)
    ((out[0][0] * g0).sum() + (out[2][0] * g2).sum() + (out[0][1] * c0).sum() + (out[1][1] * c1).sum()).backward()
    assert len(stub.blend_bwd) == 3
    for t, (gb, gc) in enumerate(((g0, c0), (None, c1), (g2, None))):
        g_blend, g_out0, g_out2, w0, w2, f0, f2, outs = stub.blend_bwd[t]
        want = gc if gb is None else (gb[:, 0:3] if gc is None else gb[:, 0:3] + gc)
        assert torch.equal(g_blend, want) and (w0, w2) == (1.0 - times[t], times[t])
        assert torch.equal(f0, offs[0][t]) and torch.equal(f2, offs[1][t])
        if gb is None:
            assert g_out0 is None and g_out2 is None
        else:
            assert torch.equal(g_out0, gb[:, 3:6]) and torch.equal(g_out2, gb[:, 6:9])
        assert g_out0 is None or g_blend.stride() == g_out0.stride() == g_out2.stride()
        assert [o is None for o in outs] == [False, True, False, False, False, False]      # ref2 does not require grad
    # the stub's kernel terms of call n: 10 n + (0 ref0, 2 flow0, 3 flow2, 4 filt0, 5 filt2)
    full = lambda v, like: torch.full_like(like, v)      # noqa: E731
    assert torch.equal(ref0.grad, (full(10.0, ref0) + 20.0) + 30.0) and ref2.grad is None
    assert torch.equal(offs[0][0].grad, full(12.0, offs[0][0]) + g0[:, 9:11])
    assert torch.equal(offs[1][0].grad, full(13.0, offs[1][0]) + g0[:, 11:13])
    assert torch.equal(offs[0][1].grad, full(22.0, offs[0][1])) and torch.equal(offs[1][1].grad, full(23.0, offs[1][1]))
    assert torch.equal(offs[0][2].grad, full(32.0, offs[0][2]) + g2[:, 9:11])
    assert torch.equal(filts[0].grad, (((full(14.0, filts[0]) + g0[:, 13:29]) + 24.0) + 34.0) + g2[:, 13:29])
    assert torch.equal(filts[1].grad, (((full(15.0, filts[1]) + g0[:, 29:45]) + 25.0) + 35.0) + g2[:, 29:45])
    # the context path: direction 0 only (ctx2 does not require grad), the two live buffers, their slices read in place
    assert len(stub.ctx_bwd) == 1
    flows, filt, gouts = stub.ctx_bwd[0]
    assert len(flows) == 2 and torch.equal(flows[0], offs[0][0]) and torch.equal(flows[1], offs[0][2]) and torch.equal(filt, filts[0])
    for g, src in zip(gouts, (g0, g2)):
        assert torch.equal(g, src[:, 45:49]) and g.stride() == src[:, 45:49].stride() and not g.is_contiguous()
    assert torch.equal(ctx0.grad, full(7.0, ctx0)) and ctx2.grad is None
