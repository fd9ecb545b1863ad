"""CPU tests (`-m "not gpu"`) of the bfloat16 rectify buffer (csrc/rectify_head_bf16.hip, cabi.rectify_head_forward_bf16,
fused.rectify_inputs(dtype=torch.bfloat16); tests/rectify_bf16.py):

  * the header declares vfi_rectify_head_forward_bf16 as the ctypes table has it, the library exports it, the unit is in the
    Makefile, and argument errors -- a head row stride unlike the frames' among them -- return before any launch;
  * with the library stubbed, cabi refuses a float32 head, bfloat16 frames, float16 and CPU tensors before any library call;
  * with the launches stubbed, fused.rectify_inputs refuses a float32 context for a bfloat16 buffer, a bfloat16 context for a
    float32 one, float16 anywhere and bfloat16 frames before any call; dtype=None issues exactly the calls it issued before;
    dtype=torch.bfloat16 issues one head call per time offset and one multi-flow call per direction, no copy_, no cat, and
    returns a float32 cur_output of its own; its backward widens the head channels, reads the context channels in place and
    allocates bfloat16 context gradients;
  * the expected-buffer helper, evaluated through the CPU oracle, equals numpy's concatenation rounded to nearest even;
  * every case of the GPU grid has invalid pixels, windows clamped at all four borders and interior pixels, and stays at
    least half valid.
"""
import contextlib
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import rectify_bf16 as rb
from tests import rectify_input as ri
from tests.test_abi_and_host import built  # noqa: F401  (fixture)
from tests.test_corr_bf16_host import _FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video-frame-interpolation-based-on-deformable-kernel-region_amd")
BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16
f32 = np.float32


# ------------------------------------------------------------------ 1. the entry: header, table, library, argument errors

def _params(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vfi_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "the header does not declare %s" % name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_library_and_ctypes_table_agree(built):  # noqa: F811
    from vfidkr_amd import cabi
    want = []
    for p in _params(rb.NAME):
        if "*" in p or p.startswith("vfi_stream_t"):
            want.append(ctypes.c_void_p)
        elif p.startswith("vfi_strides"):
            want.append(cabi.Strides)
        elif p.startswith("float "):
            want.append(ctypes.c_float)
        else:
            assert re.fullmatch(r"int \w+", p), p
            want.append(ctypes.c_int)
    assert cabi.SIGNATURES[rb.NAME] == want and len(want) == 21
    # the float32 entry's inputs, sizes and weights; one bfloat16 destination and the float32 blend for its three outputs
    blend = _params("vfi_filterinterp_blend_forward")
    assert _params(rb.NAME) == blend[:6] + ["void* head_bf16", "float* blend_f32"] + blend[9:19] + \
        ["vfi_strides s_head", "vfi_strides s_blend", blend[20]]
    assert hasattr(ctypes.CDLL(built.LIB_PATH), rb.NAME)
    fn = getattr(cabi.lib(), rb.NAME)
    assert fn.argtypes == want and fn.restype is ctypes.c_int
    text = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "rectify_head_bf16.hip" in re.search(r"^SRCS\s*:=\s*(.*)$", text, flags=re.M).group(1).split()


def test_argument_errors_return_before_any_launch(built):  # noqa: F811
    from vfidkr_amd import cabi
    f, E = getattr(cabi.lib(), rb.NAME), cabi.VFI_ERR_SHAPE
    p = ctypes.c_void_p(4096)               # never dereferenced: every call below returns before any launch
    s = cabi.Strides(384, 64, 8)

    def call(ptrs=(p,) * 7, blend=p, dims=(1, 3, 8, 8), fcn=16, sr=s, sh=cabi.Strides(2880, 64, 8)):
        return f(*ptrs, blend, *dims, fcn, 0.5, 0.5, sr, s, s, sh, s, None)
    for k in range(7):                      # every input and the head; blend_f32 alone may be NULL
        assert call(ptrs=(p,) * k + (None,) + (p,) * (6 - k)) == E
    for dims in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1), (65536, 3, 8, 8)):
        assert call(dims=dims) == E and call(dims=dims, blend=None) == E
    assert call(fcn=0) == E and call(fcn=-16) == E
    # the head's rows are the frames' rows, for every filter size and with or without the float32 blend
    for fcn in (16, 36, 4, 25, 7):
        for blend in (p, None):
            assert call(fcn=fcn, blend=blend, sh=cabi.Strides(2880, 64, 10)) == E
            assert call(fcn=fcn, blend=blend, sr=cabi.Strides(384, 64, 9)) == E
    assert call(sh=cabi.Strides(2880, 64, 0)) == E and call(sh=cabi.Strides(2880, 64, -8)) == E
    # ... asserted from the source's host check too: one test before the launch, for every kernel instance
    src = " ".join(open(os.path.join(PKG, "csrc", "rectify_head_bf16.hip")).read().split())
    entry = src.split('extern "C" int %s(' % rb.NAME, 1)[1]
    check, launch = entry.index("if (s_head.h != s_ref.h || batch > 65535) return VFI_ERR_SHAPE;"), entry.index("hipLaunchKernelGGL(")
    assert check < launch and entry.count("hipLaunchKernelGGL(") == 1
    # the arithmetic is the float32 kernel's, through its helpers: nothing restated
    assert all(t in src for t in ("fi_side(", "fi4_value(", "fi_side_value(", "bf16_pack_rne(")) and "fmaf(" not in src
    assert "struct FiSide" not in open(os.path.join(PKG, "csrc", "glue.hip")).read()


# ------------------------------------------------------------------ 2. cabi, library stubbed

class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


@pytest.fixture
def stubbed_lib(monkeypatch):
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi
    rec = _Recorder()
    monkeypatch.setattr(cabi, "lib", lambda: rec)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: types.SimpleNamespace(cuda_stream=0))
    return cabi, rec


def _t(dtype, *shape, cuda=True):
    return _FakeCuda(torch.zeros(*shape, dtype=dtype), cuda)


def _head_args(frames=F32, flows=F32, filts=F32, head=BF, blend=F32, fcn=16):
    B, H, W = 2, 6, 10
    return [_t(frames, B, 3, H, W), _t(frames, B, 3, H, W), _t(flows, B, 2, H, W), _t(flows, B, 2, H, W), _t(filts, B, fcn, H, W),
            _t(filts, B, fcn, H, W), _t(head, B, 13 + 2 * fcn, H, W), None if blend is None else _t(blend, B, 3, H, W)]


def test_cabi_passes_the_layouts_and_refuses_before_any_library_call(stubbed_lib):
    cabi, rec = stubbed_lib
    call = cabi.rectify_head_forward_bf16
    # the head as the first 45 channels of a 57-channel buffer; blend given and absent
    wide = torch.zeros(2, 57, 6, 10, dtype=BF)
    args = _head_args()
    args[6] = _FakeCuda(wide[:, :45])
    assert call(*args, 0.75, 0.25) == 0 and call(*args[:7], None, 0.75, 0.25) == 0
    assert [n for n, _ in rec.calls] == [rb.NAME] * 2
    for (_, a), null in zip(rec.calls, (False, True)):
        assert len(a) == len(cabi.SIGNATURES[rb.NAME]) and a[8:13] == (2, 3, 6, 10, 16) and a[13:15] == (0.75, 0.25)
        assert [(s.b, s.c, s.h) for s in a[15:20]] == [(180, 60, 10), (120, 60, 10), (960, 60, 10), (3420, 60, 10), (180, 60, 10)]
        assert (a[7].value is None) == null
    del rec.calls[:]
    for kw, want in ((dict(head=F32), "bfloat16"), (dict(frames=BF), "float32"), (dict(flows=BF), "float32"), (dict(filts=BF), "float32"),
                     (dict(blend=BF), "float32"), (dict(head=F16), "bfloat16"), (dict(frames=F16), "float32"), (dict(flows=F16), "float32"),
                     (dict(filts=F16), "float32"), (dict(blend=F16), "float32")):
        with pytest.raises(RuntimeError, match="tensors must be " + want):
            call(*_head_args(**kw), 0.5, 0.5)
    for k in (0, 3, 6, 7):
        args = _head_args()
        args[k] = _FakeCuda(args[k].t, False)
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call(*args, 0.5, 0.5)
    # layouts: another channel count, rows farther apart than the frames', a w stride of 2, a blend of another shape
    args = _head_args()
    assert call(*args[:6], _t(BF, 2, 44, 6, 10), args[7], 0.5, 0.5) == 1
    assert call(*args[:6], _FakeCuda(torch.zeros(2, 45, 6, 12, dtype=BF)[..., :10]), args[7], 0.5, 0.5) == 1
    assert call(*args[:6], _FakeCuda(torch.zeros(2, 45, 6, 20, dtype=BF)[..., ::2]), args[7], 0.5, 0.5) == 1
    assert call(*args[:7], _t(F32, 2, 4, 6, 10), 0.5, 0.5) == 1
    assert rec.calls == []


# ------------------------------------------------------------------ 3. fused, launches stubbed

class _Stub:
    """Stands in for the launches: logs each call and fills what the kernel writes with values that name the call."""

    def __init__(self):
        self.log, self.head_calls, self.ctx, self.blend_bwd, self.ctx_bwd = [], [], [], [], []

    def blend_forward(self, ref0, ref2, f0, f2, k0, k2, blend, out0, out2, w0, w2):
        self.log.append("blend_forward")
        blend.fill_(1.0), out0.fill_(2.0), out2.fill_(3.0)
        return 0

    def head(self, ref0, ref2, f0, f2, k0, k2, head, blend, w0, w2):
        self.log.append("head")
        self.head_calls.append((ref0, ref2, f0, f2, k0, k2, head, blend, w0, w2))
        head.fill_(100.0 + len(self.head_calls)), blend.fill_(200.0 + len(self.head_calls))
        return 0

    def multi_to(self, image, flows, filt, outs):
        self.log.append("multi_to")
        self.ctx.append((image, list(flows), filt, list(outs)))
        for t, o in enumerate(outs):
            o.fill_(8.0 * len(self.ctx) + t)
        return 0

    def blend_backward(self, ref0, ref2, f0, f2, k0, k2, g_blend, g_out0, g_out2, w0, w2, gr0, gr2, gf0, gf2, gk0, gk2):
        self.log.append("blend_backward")
        self.blend_bwd.append((g_blend, g_out0, g_out2, w0, w2))
        for i, o in enumerate((gr0, gr2, gf0, gf2, gk0, gk2)):
            if o is not None:
                o.fill_(10.0 * len(self.blend_bwd) + i)
        return 0

    def image_multi(self, flows, filt, gouts, g1):
        self.log.append("image_multi")
        self.ctx_bwd.append((list(flows), filt, list(gouts), g1))
        g1.fill_(7.0 * len(self.ctx_bwd))
        return 0


@pytest.fixture
def stubbed(monkeypatch):
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi, fused
    stub = _Stub()
    monkeypatch.setattr(cabi, "filterinterp_blend_forward", stub.blend_forward)
    monkeypatch.setattr(cabi, "rectify_head_forward_bf16", stub.head)
    monkeypatch.setattr(cabi, "filterinterp_forward_ori_multi_to", stub.multi_to)
    monkeypatch.setattr(cabi, "filterinterp_blend_backward", stub.blend_backward)
    monkeypatch.setattr(cabi, "filterinterp_backward_ori_image_multi", stub.image_multi)
    return fused, stub


def _inputs(T, cctx, ctx_dtype=BF, float_dtype=F32, frame_dtype=F32, B=2, H=5, W=6):
    ref0, ref2 = torch.rand(B, 3, H, W).to(frame_dtype), torch.rand(B, 3, H, W).to(frame_dtype)
    offs = [[torch.rand(B, 2, H, W).to(float_dtype) for _ in range(T)] for _ in range(2)]
    filts = [torch.rand(B, 16, H, W).to(float_dtype) for _ in range(2)]
    ctx = [torch.rand(B, cctx, H, W).to(ctx_dtype) for _ in range(2)] if cctx else [None, None]
    return ref0, ref2, offs, filts, ctx[0], ctx[1]


def _is_slice(view, buf, rng):
    ref = buf[:, rng[0]:rng[1]]
    return view.data_ptr() == ref.data_ptr() and view.shape == ref.shape and view.stride() == ref.stride()


TIMES = [0.25, 0.5, 0.75]


def test_refusals_happen_before_any_call(stubbed):
    fused, stub = stubbed

    def refused(dtype, **kw):
        ref0, ref2, offs, filts, c0, c2 = _inputs(3, 4, **kw)
        with pytest.raises(RuntimeError, match="tensors must be"):
            fused.rectify_inputs(ref0, ref2, offs, filts, 16, TIMES, c0, c2, dtype=dtype)
        assert stub.log == []
    refused(BF, ctx_dtype=F32)                                  # a float32 context into the bfloat16 buffer
    refused(None, ctx_dtype=BF)                                 # a bfloat16 context into the float32 buffer: as before
    refused(BF, frame_dtype=BF)                                 # frames are float32
    for dtype in (BF, None):
        for kw in (dict(ctx_dtype=F16), dict(float_dtype=F16), dict(frame_dtype=F16)):
            refused(dtype, **kw)
    refused(None, ctx_dtype=F32, float_dtype=BF)                # bfloat16 flows and filters belong to the bfloat16 buffer
    ref0, ref2, offs, filts, c0, c2 = _inputs(3, 4)
    for dtype in (F32, F16, torch.float64):
        with pytest.raises(RuntimeError, match="dtype is None"):
            fused.rectify_inputs(ref0, ref2, offs, filts, 16, TIMES, c0, c2, dtype=dtype)
    with pytest.raises(RuntimeError, match="together"):
        fused.rectify_inputs(ref0, ref2, offs, filts, 16, TIMES, c0, None, dtype=BF)
    assert stub.log == []


@pytest.mark.parametrize("cctx", [None, 4])
@pytest.mark.parametrize("train", [False, True])
def test_dtype_none_issues_the_calls_it_issued_before(stubbed, cctx, train):
    fused, stub = stubbed
    ref0, ref2, offs, filts, c0, c2 = _inputs(3, cctx, ctx_dtype=F32)
    if train:
        filts[0].requires_grad_()
    for kw in ({}, {"dtype": None}):
        del stub.log[:]
        out = fused.rectify_inputs(ref0, ref2, offs, filts, 16, TIMES, c0, c2, **kw)
        assert stub.log == ["blend_forward"] * 3 + ["multi_to"] * (2 if cctx else 0)
        m = ri.channel_map(16, cctx)
        for t, (buf, cur) in enumerate(out):
            assert buf.dtype == F32 and buf.shape == (2, m["total"], 5, 6) and cur.dtype == F32
            assert (cur.data_ptr() == buf.data_ptr()) == (not train) and (buf.grad_fn is not None) == train
            assert torch.equal(buf[:, 13:29].detach(), filts[0].detach()) and torch.equal(buf[:, 9:11].detach(), offs[0][t])
    assert not stub.head_calls


@pytest.mark.parametrize("cctx", [None, 4])
@pytest.mark.parametrize("float_dtype", [F32, BF])
def test_bfloat16_issues_one_head_call_per_time_offset_and_no_copy(stubbed, monkeypatch, cctx, float_dtype):
    fused, stub = stubbed
    ref0, ref2, offs, filts, c0, c2 = _inputs(3, cctx, float_dtype=float_dtype)

    def refuse(name):
        def fn(*a, **k):
            raise AssertionError("%s was reached" % name)
        return fn
    monkeypatch.setattr(fused._RectifyInputsBf16, "apply", refuse("the autograd Function"))
    monkeypatch.setattr(fused._RectifyInputs, "apply", refuse("the float32 Function"))
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "copy_", refuse("copy_"))
        mp.setattr(torch, "cat", refuse("torch.cat"))
        mp.setattr(torch.Tensor, "clone", refuse("clone"))
        out = fused.rectify_inputs(ref0, ref2, offs, filts, 16, TIMES, c0, c2, dtype=BF)
    assert stub.log == ["head"] * 3 + ["multi_to"] * (2 if cctx else 0)
    m = ri.channel_map(16, cctx)
    assert len(out) == 3
    for t, (buf, cur) in enumerate(out):
        assert buf.dtype == BF and buf.shape == (2, m["total"], 5, 6) and buf.is_contiguous() and buf.grad_fn is None
        # cur_output: float32, dense, a tensor of its own -- in inference too
        assert cur.dtype == F32 and cur.shape == (2, 3, 5, 6) and cur.is_contiguous() and cur.grad_fn is None
        ref0_, ref2_, f0, f2, k0, k2, head, blend, w0, w2 = stub.head_calls[t]
        assert ref0_ is ref0 and ref2_ is ref2 and _is_slice(head, buf, (0, 45)) and blend is cur
        assert (w0, w2) == (1.0 - TIMES[t], TIMES[t])
        # the kernel sees float32 flows and filters: passed through untouched, or widened once for all time offsets
        assert f0.dtype == F32 and k0.dtype == F32 and torch.equal(f0, offs[0][t].float()) and torch.equal(k2, filts[1].float())
        assert (f0 is offs[0][t]) == (float_dtype == F32) and k0 is stub.head_calls[0][4] and (k0 is filts[0]) == (float_dtype == F32)
        assert (buf[:, :45] == 101.0 + t).all() and (cur == 201.0 + t).all()
    if cctx:
        for d, name in enumerate(("ctx0", "ctx2")):
            image, flows, filt, outs = stub.ctx[d]
            assert image is (c0, c2)[d] and image.dtype == BF and filt is stub.head_calls[0][4 + d]
            assert all(a is b[2 + d] for a, b in zip(flows, stub.head_calls))
            assert len(outs) == 3 and all(o.dtype == BF and _is_slice(o, out[t][0], m[name]) for t, o in enumerate(outs))


def test_bfloat16_training_shares_the_float32_bookkeeping(stubbed):
    fused, stub = stubbed
    ref0, ref2, offs, filts, c0, c2 = _inputs(3, 4)
    bfilt = filts[1].to(BF).requires_grad_()                    # a bfloat16 leaf: its gradient comes back rounded
    for t in [ref0, filts[0], c0] + offs[0] + offs[1]:
        t.requires_grad_()
    with torch.no_grad():
        assert all(b.grad_fn is None for b, _ in fused.rectify_inputs(ref0, ref2, offs, [filts[0], bfilt], 16, TIMES, c0, c2, dtype=BF))
    stub.__init__()
    out = fused.rectify_inputs(ref0, ref2, offs, [filts[0], bfilt], 16, TIMES, c0, c2, dtype=BF)
    assert stub.log == ["head"] * 3 + ["multi_to"] * 2
    m = ri.channel_map(16, 4)
    fn = out[0][0].grad_fn
    assert fn is not None and all(b.grad_fn is fn and c.grad_fn is fn for b, c in out)       # ONE Function over all time offsets
    assert type(fn).__name__.startswith("_RectifyInputsBf16")
    assert all(b.dtype == BF and c.dtype == F32 and c.data_ptr() != b.data_ptr() for b, c in out)
    assert sorted((tuple(t.shape)[1], t.dtype) for t in fn.saved_tensors) == sorted([(2, F32)] * 6 + [(3, F32)] * 2 + [(16, F32)] * 2)
    g0, g2 = torch.rand(2, m["total"], 5, 6).to(BF), torch.rand(2, m["total"], 5, 6).to(BF)
    c_0, c_1 = torch.rand(2, 3, 5, 6), torch.rand(2, 3, 5, 6)
    del stub.log[:]
    torch.autograd.backward([out[0][0], out[2][0], out[0][1], out[1][1]], [g0, g2, c_0, c_1])
    assert stub.log == ["blend_backward"] * 3 + ["image_multi"]
    for t, (gb, gc) in enumerate(((g0, c_0), (None, c_1), (g2, None))):
        g_blend, g_out0, g_out2, w0, w2 = stub.blend_bwd[t]
        want = gc if gb is None else (gb[:, 0:3].float() if gc is None else gb[:, 0:3].float() + gc)
        assert g_blend.dtype == F32 and torch.equal(g_blend, want) and (w0, w2) == (1.0 - TIMES[t], TIMES[t])
        if gb is None:
            assert g_out0 is None and g_out2 is None
        else:
            assert g_out0.dtype == F32 and torch.equal(g_out0, gb[:, 3:6].float()) and torch.equal(g_out2, gb[:, 6:9].float())
            assert g_blend.stride() == g_out0.stride() == g_out2.stride()
    full = lambda v, like: torch.full_like(like, v)      # noqa: E731
    # the float32 path's sums, in its order, over the widened slices
    assert ref0.grad.dtype == F32 and torch.equal(ref0.grad, (full(10.0, ref0) + 20.0) + 30.0) and ref2.grad is None
    assert torch.equal(offs[0][0].grad, full(12.0, offs[0][0]) + g0[:, 9:11].float())
    assert torch.equal(offs[1][1].grad, full(23.0, offs[1][1]))
    assert torch.equal(offs[0][2].grad, full(32.0, offs[0][2]) + g2[:, 9:11].float())
    want0 = (((full(14.0, filts[0]) + g0[:, 13:29].float()) + 24.0) + 34.0) + g2[:, 13:29].float()
    assert filts[0].grad.dtype == F32 and torch.equal(filts[0].grad, want0)
    want1 = (((full(15.0, filts[1]) + g0[:, 29:45].float()) + 25.0) + 35.0) + g2[:, 29:45].float()
    assert bfilt.grad.dtype == BF and torch.equal(bfilt.grad, want1.to(BF))
    # the context path: direction 0 only, the two live buffers, their bfloat16 slices read in place, a bfloat16 gradient
    flows, filt, gouts, g1 = stub.ctx_bwd[0]
    assert len(flows) == 2 and torch.equal(flows[0], offs[0][0]) and torch.equal(flows[1], offs[0][2]) and filt.dtype == F32
    for g, src in zip(gouts, (g0, g2)):
        assert g.dtype == BF and g.data_ptr() == src[:, 45:49].data_ptr() and g.stride() == src[:, 45:49].stride()
    assert g1.dtype == BF and c0.grad.dtype == BF and torch.equal(c0.grad, full(7.0, c0)) and c2.grad is None


# ------------------------------------------------------------------ 4. the expected buffer, through the oracle

@pytest.mark.parametrize("shape,filter_channels,channel", [((2, 9, 21), 16, 3), ((1, 5, 7), 36, 1), ((2, 6, 21), 16, 3)])
def test_expected_head_through_the_oracle(oracle, shape, filter_channels, channel):
    """the helper on CPU tensors with the oracle as the float32 function: torch's CPU cat and conversion give numpy's
    concatenation rounded to nearest even (restated on the bits), in the reference's channel order"""
    case = rb.head_case(shape, filter_channels, channel)
    tensors = [torch.from_numpy(a) for a in case]
    head, blend = rb.expected_head(torch, rb.oracle_blend(torch, oracle), *tensors, 0.75, 0.25)
    assert head.dtype == BF and tuple(head.shape) == (shape[0], rb.head_channels(channel, filter_channels)) + shape[1:]
    b, o0, o2 = oracle.filterinterp_blend(*case, 0.75, 0.25, fmad=1)
    assert np.array_equal(blend.numpy(), b) and np.array_equal(b, o0 * f32(0.75) + o2 * f32(0.25))
    cat = np.concatenate((b, o0, o2) + case[2:], axis=1)
    u = np.ascontiguousarray(cat).view(np.uint32).astype(np.uint64)
    rne = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)           # (finite inputs: no NaN to keep quiet)
    assert np.isfinite(cat).all() and np.array_equal(rb.tensor_bits(torch, head), rne)
    assert not rb.same_bits(rb.tensor_bits(torch, head), rb.bits(cat))
    C = channel
    assert np.array_equal(rb.tensor_bits(torch, head[:, 3 * C:3 * C + 2]), rb.bits(case[2]))                 # flow0 after the frames
    assert np.array_equal(rb.tensor_bits(torch, head[:, 3 * C + 4 + filter_channels:]), rb.bits(case[5]))    # filt2 last
    # the comparison itself: NaN anywhere matches NaN, a changed bit or a NaN at another place does not
    a = torch.tensor([1.0, float("nan"), -0.0, 3.0]).to(BF)
    assert not rb.diff_bf16(torch, a, torch.tensor([1.0, -float("nan"), -0.0, 3.0]).to(BF))
    assert rb.diff_bf16(torch, a, torch.tensor([1.0, float("nan"), 0.0, 3.0]).to(BF))
    assert rb.diff_bf16(torch, a, torch.tensor([float("nan"), 1.0, -0.0, 3.0]).to(BF))
    assert rb.diff_f32(torch, torch.tensor([0.0]), torch.tensor([-0.0])) and not rb.diff_f32(torch, torch.tensor([float("nan")]), torch.tensor([float("nan")]))


# ------------------------------------------------------------------ 5. the census of the GPU cases, and their layouts

@pytest.mark.parametrize("shape,filter_channels,channel", rb.all_head_cases())
def test_census_of_every_gpu_case(shape, filter_channels, channel):
    B, H, W = shape
    case = rb.head_case(shape, filter_channels, channel)
    for flow in case[2:4]:
        c = rb.census(flow, H, W)
        assert c["invalid"] + c["clamped"] + c["interior"] == c["total"] == B * H * W
        assert rb.census_ok(c), c


def test_census_counts_by_hand():
    flow = np.zeros((1, 2, 6, 8), f32)
    c = rb.census(flow, 6, 8)
    # zero flow: ix = x, the window spans x - 1 .. x + 2: clamped in column 0 and columns 6, 7; rows 0, 4, 5
    assert (c["invalid"], c["left"], c["right"], c["top"], c["bottom"]) == (0, 6, 12, 8, 16)
    assert c["interior"] == 5 * 3 and c["clamped"] == 48 - 15 and not rb.census_ok(c)
    flow[0, 0, 2, 3] = 4.0                                     # |fx| reaches w / 2: invalid
    flow[0, 1, 3, 3] = -2.5                                    # lands in row 0: clamped at the top
    c2 = rb.census(flow, 6, 8)
    assert (c2["invalid"], c2["interior"], c2["top"]) == (1, 13, 9) and rb.census_ok(c2)


def test_guarded_slice_layout():
    for shape in rb.HEAD_SHAPES + rb.PADDED_SHAPES:
        for C in (rb.head_channels(c, fc) for c in rb.HEAD_CHANNELS for fc in rb.HEAD_FILTERS):
            (sb, sc, sh, sw), offset = rb.slice_layout((shape[0], C, shape[1], shape[2]))
            assert sb % 2 == 1 and offset % 2 == 1 and sh == shape[2] and sw == 1      # odd per-image count, odd offset, the frames' rows
            assert sc != shape[1] * shape[2] and sb != C * sc and sb >= C * sc         # batch and channel strides of its own
