"""CPU tests (`-m "not gpu"`) of the channels_last image gradient of FilterInterpolation
(csrc/filterinterp_nhwc_bwd.hip, vfidkr_amd/cabi_nhwc.py, fused's train_channels_last; tests/fi_nhwc_backward.py):

  * the header declares both entries with the layouts' own structs, the Makefile lists the unit, the library exports them, the
    ctypes table carries them, and every refusal of the entries returns VFI_ERR_SHAPE before any launch;
  * the mirror's constants are the source's, and the width mirror gives the library's own answer;
  * with the library stubbed, cabi_nhwc.filterinterp_backward_nhwc_image_multi passes element strides of dense and sliced
    channels_last tensors, dispatches on dtype, and refuses every one-argument-wrong call before a library call;
  * with the wrappers stubbed, fused keeps its default refusal, and with train_channels_last=True reaches the new Function:
    the backward gets exactly the live gradients with their flows, channels_last, flows widened; and every other case goes
    where it went;
  * a census through the mirror: the GPU tests' inputs reach every tile class and every call class.
"""
import contextlib
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import fi_nhwc_backward as fb
from tests.test_abi_and_host import built, header_functions  # noqa: F401  (fixture)
from tests.test_corr_bf16_host import _FakeCuda
from tests.test_fi_nhwc_host import _params, _Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video-frame-interpolation-based-on-deformable-kernel-region_amd")
F32N, BF16N = "vfi_filterinterp_backward_ori_nhwc_image_multi", "vfi_filterinterp_backward_ori_nhwc_image_multi_bf16"
BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16
f32 = np.float32


# ------------------------------------------------------------------ 1. header, Makefile, library, table

@pytest.mark.parametrize("name", [F32N, BF16N])
def test_header_makefile_library_and_ctypes_table_agree(built, name):  # noqa: F811
    from vfidkr_amd import cabi
    assert name in header_functions()
    want = []
    for p in _params(name):
        if "*" in p or p.startswith("vfi_stream_t"):
            want.append(ctypes.c_void_p)
        elif p.startswith("vfi_strides_nhwc "):
            want.append(cabi.StridesNhwc)
        elif p.startswith("vfi_strides4 "):
            want.append(cabi.Strides4)
        else:
            assert re.fullmatch(r"int \w+", p), p
            want.append(ctypes.c_int)
    assert cabi.SIGNATURES[name] == want and len(want) == 15
    ps = _params(name)
    assert [p.split()[0] for p in ps[10:14]] == ["vfi_strides_nhwc", "vfi_strides4", "vfi_strides4", "vfi_strides_nhwc"]
    assert [p.split()[-1] for p in ps[10:15]] == ["s1", "s2", "s3", "sg", "stream"]
    assert [re.search(r"(\w+)$", p).group(1) for p in ps[:10]] == \
        ["flows", "input3", "gradoutputs" + ("_bf16" if name == BF16N else ""), "gradinput1" + ("_bf16" if name == BF16N else ""),
         "nflows", "batch", "channel", "h", "w", "filter_channels"]
    assert hasattr(ctypes.CDLL(built.LIB_PATH), name)
    fn_ = getattr(cabi.lib(), name)
    assert fn_.argtypes == want and fn_.restype is ctypes.c_int
    assert cabi.INTERNAL_SIGNATURES[name + "_direct"] == want and hasattr(ctypes.CDLL(built.LIB_PATH), name + "_direct")
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert fb.SRC in re.search(r"^SRCS\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()


def test_argument_errors_return_before_any_launch(built):  # noqa: F811
    from vfidkr_amd import cabi
    lib, E = cabi.lib(), cabi.VFI_ERR_SHAPE
    p = ctypes.c_void_p(4096)               # never dereferenced
    two, hole = (ctypes.c_void_p * 2)(4096, 4096), (ctypes.c_void_p * 2)(4096, None)
    s1, s4 = cabi.StridesNhwc(192, 24, 3), cabi.Strides4(128, 64, 8, 1)
    for name in (F32N, BF16N, F32N + "_direct", BF16N + "_direct"):
        f = getattr(lib, name)

        def bwd(flows=two, filt=p, gouts=two, g1=p, n=2, dims=(1, 3, 8, 8), fcn=16):
            return f(flows, filt, gouts, g1, n, *dims, fcn, s1, s4, s4, s1, None)
        assert bwd(flows=None) == E and bwd(filt=None) == E and bwd(gouts=None) == E and bwd(g1=None) == E
        assert bwd(flows=hole) == E and bwd(gouts=hole) == E and bwd(n=0) == E and bwd(n=-1) == E and bwd(fcn=0) == E
        for dims in ((0, 3, 8, 8), (1, 0, 8, 8), (1, -2, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1), (65536, 3, 8, 8),
                     (65535, 3, 4 * 64, 32 * 65)):            # batch beyond the limit; more than 2^28 tiles
            assert bwd(dims=dims) == E, (name, dims)


# ------------------------------------------------------------------ 2. the mirror's constants and the width mirror

def test_constants_and_the_width_mirror(built):  # noqa: F811
    c = fb.constants()
    assert c == {"FNB_TW": 32, "FNB_TH": 4, "FNB_PIXELS": 128, "FNB_THREADS": 256, "FNB_SLAB": 16, "FNB_CELLS": 7168, "FNB_NT": 3}
    assert c["FNB_PIXELS"] == c["FNB_TW"] * c["FNB_TH"]
    assert c["FNB_SLAB"] * 8 >= 128                          # a cell's slab spans at least 128 bytes of the scratch
    # a 35 x 7 window (a 32 x 4 tile on a smooth flow) is staged, and so is a tile whose flows reach two pixels every way
    # (39 x 11); the first that does not fit has more than 448 cells
    assert fb.window_fits(35, 7) and fb.window_fits(39, 11) and fb.window_fits(448, 1) and not fb.window_fits(449, 1) and \
        not fb.window_fits(64, 8)
    # the launcher's source states the decision the mirror restates
    src = fb.fw.source(fb.SRC)
    assert "(int64_t)bw * bh * FNB_SLAB <= FNB_CELLS" in src and "!DIRECT && fs == 4 && filter_channels == 16" in src
    from vfidkr_amd import cabi
    lib = cabi.lib()

    def both(esize, shape, grads):
        gp = (ctypes.c_void_p * len(grads))(*[p for p, _ in grads])
        got = lib.vfi_filterinterp_nhwc_bwd_access_width(esize, gp, len(grads), shape[0], shape[2], shape[3], 16,
                                                         cabi.StridesNhwc(*grads[0][1]))
        assert got == fb.vector_width(esize, shape, grads), (got, esize, shape, grads)
        return got
    shape = (2, 196, 19, 37)
    dense = lambda c_: (19 * 37 * c_, 37 * c_, c_)      # noqa: E731
    assert both(4, shape, [(256, dense(196)), (512, dense(196))]) == 4
    assert both(2, shape, [(256, dense(196)), (512, dense(196))]) == 4
    assert both(2, shape, [(256 + 96, dense(440))]) == 8 and both(4, shape, [(256 + 96, dense(440))]) == 4
    assert both(2, shape, [(256 + 96, dense(440)), (256 + 90, dense(440))]) == 1
    assert both(2, shape, [(256 + 90, dense(437))]) == 1 and both(4, shape, [(256 + 180, dense(437))]) == 1
    assert both(2, shape, [(256 + 8, dense(440))]) == 4 and both(4, shape, [(256 + 8, dense(440))]) == 2
    odd = (19 * 37 * 8 + 1, 37 * 8, 8)
    assert both(2, (1, 8, 19, 37), [(256, odd)]) == 8 and both(2, (2, 8, 19, 37), [(256, odd)]) == 1
    assert lib.vfi_filterinterp_nhwc_bwd_access_width(4, (ctypes.c_void_p * 1)(256), 1, 2, 19, 37, 25, cabi.StridesNhwc(*dense(8))) == -1


# ------------------------------------------------------------------ 3. cabi_nhwc, library stubbed

@pytest.fixture
def stubbed(monkeypatch):
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi, cabi_nhwc
    rec = _Recorder()
    monkeypatch.setattr(cabi, "lib", lambda: rec)
    monkeypatch.setattr(cabi_nhwc, "lib", lambda: rec)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: types.SimpleNamespace(cuda_stream=0))
    return cabi_nhwc, rec


def _t(dtype, *shape, cuda=True, cl=False):
    t = torch.zeros(*shape, dtype=dtype)
    return _FakeCuda(t.contiguous(memory_format=torch.channels_last) if cl else t, cuda)


class _Elsewhere(_FakeCuda):
    """... and says it lives on a second GPU"""
    device = torch.device("cuda", 1)


def test_cabi_nhwc_passes_channels_last_layouts_in_elements(stubbed):
    from vfidkr_amd import cabi
    cabi_nhwc, rec = stubbed
    for dt, name in ((F32, F32N), (BF, BF16N)):
        del rec.calls[:]
        wide = _t(dt, 2, 9, 6, 10, cl=True)
        gs = [_FakeCuda(wide.t[:, 1:6]), _FakeCuda(torch.zeros_like(wide.t)[:, 1:6])]
        g1 = _t(dt, 2, 5, 6, 10, cl=True)
        flows = [_t(F32, 2, 2, 6, 10), _t(F32, 2, 2, 6, 10)]
        filt = _t(F32, 2, 16, 6, 10, cl=True)
        assert cabi_nhwc.filterinterp_backward_nhwc_image_multi(flows, filt, gs, g1) == 0
        (got, a), = rec.calls
        assert got == name and len(a) == len(cabi.SIGNATURES[name])
        assert a[4:10] == (2, 2, 5, 6, 10, 16)
        s1, s2, s3, sg = a[10:14]
        assert (s1.b, s1.h, s1.w) == (300, 50, 5) and (sg.b, sg.h, sg.w) == (540, 90, 9)
        assert (s2.b, s2.c, s2.h, s2.w) == (120, 60, 10, 1) and (s3.b, s3.c, s3.h, s3.w) == (960, 1, 160, 16)
        # a sliced result and dense gradients; the internal switch takes the _direct entry
        del rec.calls[:]
        dense = [_t(dt, 2, 5, 6, 10, cl=True)]
        assert cabi_nhwc.filterinterp_backward_nhwc_image_multi(flows[:1], filt, dense, gs[0], direct=True) == 0
        (got, a), = rec.calls
        assert got == name + "_direct" and (a[10].b, a[10].h, a[10].w) == (540, 90, 9) and (a[13].b, a[13].h, a[13].w) == (300, 50, 5)
        # a one-channel tensor is channels_last whatever its channel stride says
        assert cabi_nhwc.filterinterp_backward_nhwc_image_multi(flows[:1], filt, [_t(dt, 2, 1, 6, 10)], _t(dt, 2, 1, 6, 10)) == 0


def test_cabi_nhwc_refuses_every_one_argument_wrong_call_before_the_library(stubbed):
    cabi_nhwc, rec = stubbed
    call = cabi_nhwc.filterinterp_backward_nhwc_image_multi
    for dt, other in ((F32, BF), (BF, F32)):
        g, g1 = _t(dt, 2, 5, 6, 10, cl=True), _t(dt, 2, 5, 6, 10, cl=True)
        flow, filt = _t(F32, 2, 2, 6, 10), _t(F32, 2, 16, 6, 10)
        wide = _t(dt, 2, 9, 6, 10, cl=True)
        assert call([flow], filt, [g], g1) == 0 and len(rec.calls) == 1     # the base call is legal
        del rec.calls[:]
        shapes = {
            "rank of gradinput1": lambda: call([flow], filt, [g], _FakeCuda(g1.t[0])),
            "rank of a gradient": lambda: call([flow], filt, [_FakeCuda(g.t[0])], g1),
            "rank of a flow": lambda: call([_FakeCuda(flow.t[0])], filt, [g], g1),
            "rank of the filter": lambda: call([flow], _FakeCuda(filt.t[0]), [g], g1),
            "gradient channels": lambda: call([flow], filt, [_t(dt, 2, 4, 6, 10, cl=True)], g1),
            "gradient frame": lambda: call([flow], filt, [_t(dt, 2, 5, 6, 11, cl=True)], g1),
            "flow channels": lambda: call([_t(F32, 2, 3, 6, 10)], filt, [g], g1),
            "flow frame": lambda: call([_t(F32, 2, 2, 7, 10)], filt, [g], g1),
            "an NCHW gradient": lambda: call([flow], filt, [_t(dt, 2, 5, 6, 10)], g1),
            "an NCHW gradinput1": lambda: call([flow], filt, [g], _t(dt, 2, 5, 6, 10)),
            "two gradient layouts": lambda: call([flow, flow], filt, [g, _FakeCuda(wide.t[:, :5])], g1),
            "two flow layouts": lambda: call([flow, _t(F32, 2, 2, 6, 10, cl=True)], filt, [g, g], g1),
            "a None flow": lambda: call([flow, None], filt, [g, g], g1),
            "a None gradient": lambda: call([flow, flow], filt, [g, None], g1),
            "empty lists": lambda: call([], filt, [], g1),
            "lists of two lengths": lambda: call([flow, flow], filt, [g], g1),
            "a zero dimension": lambda: call([_t(F32, 2, 2, 0, 10)], _t(F32, 2, 16, 0, 10), [_t(dt, 2, 5, 0, 10)], _t(dt, 2, 5, 0, 10)),
            "a filter of another frame": lambda: call([flow], _t(F32, 2, 16, 7, 10), [g], g1),
            "a filter of another batch": lambda: call([flow], _t(F32, 1, 16, 6, 10), [g], g1),
        }
        for what, bad in shapes.items():
            assert bad() == 1, "%s (%s) was not refused with 1" % (what, dt)
        raises = {
            "a float16 gradient": (lambda: call([flow], filt, [_t(F16, 2, 5, 6, 10, cl=True)], g1), "tensors must be"),
            "float16 everywhere": (lambda: call([flow], filt, [_t(F16, 2, 5, 6, 10, cl=True)], _t(F16, 2, 5, 6, 10, cl=True)),
                                   "tensors must be float32"),
            "a gradient of the other dtype": (lambda: call([flow], filt, [_t(other, 2, 5, 6, 10, cl=True)], g1), "tensors must be"),
            "gradinput1 of the other dtype": (lambda: call([flow], filt, [g], _t(other, 2, 5, 6, 10, cl=True)), "tensors must be"),
            "a bfloat16 flow": (lambda: call([_t(BF, 2, 2, 6, 10)], filt, [g], g1), "tensors must be float32"),
            "a bfloat16 filter": (lambda: call([flow], _t(BF, 2, 16, 6, 10), [g], g1), "tensors must be float32"),
            "a CPU gradient": (lambda: call([flow], filt, [_t(dt, 2, 5, 6, 10, cl=True, cuda=False)], g1), "must live on the GPU"),
            "a CPU gradinput1": (lambda: call([flow], filt, [g], _t(dt, 2, 5, 6, 10, cl=True, cuda=False)), "must live on the GPU"),
            "a CPU flow": (lambda: call([_t(F32, 2, 2, 6, 10, cuda=False)], filt, [g], g1), "must live on the GPU"),
            "a gradient on a second device": (lambda: call([flow], filt, [_Elsewhere(g.t)], g1), "one device"),
            "a filter on a second device": (lambda: call([flow], _Elsewhere(filt.t), [g], g1), "one device"),
        }
        for what, (bad, text) in raises.items():
            with pytest.raises(RuntimeError, match=text):
                bad()
                pytest.fail("%s (%s) was not refused" % (what, dt))
        assert rec.calls == [], rec.calls


# ------------------------------------------------------------------ 4. fused, wrappers stubbed

def test_fused_train_channels_last(monkeypatch):
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi, cabi_nhwc, fused
    log = []

    def forward(tag):
        def fn_(image, flows, filt, outs):
            log.append((tag, tuple(image.stride())))
            for o in outs:
                o.zero_()
            return 0
        return fn_

    def backward(tag):
        def fn_(flows, filt, gouts, gimg):
            log.append((tag, [int(f.flatten()[0]) for f in flows], [f.dtype for f in flows], filt.dtype,
                        [(g.dtype, tuple(g.stride()), float(g.flatten()[0])) for g in gouts], gimg.dtype, tuple(gimg.stride())))
            gimg.fill_(1.0)
            return 0
        return fn_
    monkeypatch.setattr(cabi, "filterinterp_forward_ori_multi", forward("nchw"))
    monkeypatch.setattr(cabi, "filterinterp_forward_nhwc_multi_to", forward("nhwc"))
    monkeypatch.setattr(cabi, "filterinterp_backward_ori_image_multi", backward("bwd_nchw"))
    monkeypatch.setattr(cabi_nhwc, "filterinterp_backward_nhwc_image_multi", backward("bwd_nhwc"))
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)      # noqa: E731
    nchw, nhwc = (240, 60, 10, 1), (240, 1, 40, 4)
    for dt in (F32, BF):
        for fdt in ((F32, BF) if dt == BF else (F32,)):
            # flow t of direction d holds 10 d + t, so the backward's flows can be told apart
            offs = [[torch.full((2, 2, 6, 10), 10.0 * d + t, dtype=fdt) for t in range(3)] for d in range(2)]
            filts = [torch.zeros(2, 16, 6, 10, dtype=fdt), cl(torch.zeros(2, 16, 6, 10, dtype=fdt))]
            c0, c2 = torch.zeros(2, 4, 6, 10, dtype=dt), torch.zeros(2, 4, 6, 10, dtype=dt)
            # the default still raises, with nothing called
            del log[:]
            with pytest.raises(RuntimeError, match="forward-only.*contiguous"):
                fused.FilterInterpolate_ctx_all(cl(c0).requires_grad_(), cl(c2), offs, filts)
            with pytest.raises(RuntimeError, match="forward-only.*contiguous"):
                fused.FilterInterpolate_ctx(cl(c0), cl(c2).requires_grad_(), [offs[0][0], offs[1][0]], filts)
            assert log == []
            # the keyword reaches the Function: one NHWC launch per direction, outputs with a grad_fn where the context trains
            a0, a2 = cl(c0).requires_grad_(), cl(c2)
            outs = fused.FilterInterpolate_ctx_all(a0, a2, offs, filts, train_channels_last=True)
            assert log == [("nhwc", nhwc)] * 2
            assert all(o0.grad_fn is not None and o2.grad_fn is None and tuple(o0.stride()) == nhwc for o0, o2 in outs)
            # the backward receives exactly the live gradients with their flows: offsets 0 and 2 were used, 1 was not
            del log[:]
            (outs[0][0] * 2.0).sum().backward(retain_graph=True)
            a0.grad = None
            del log[:]
            ((outs[0][0] * 3.0).sum() + (outs[2][0] * 5.0).sum()).backward(retain_graph=True)
            (tag, flows_seen, fdts, filt_dt, gs, gdt, gst), = log
            assert tag == "bwd_nhwc" and flows_seen == [0, 2] and fdts == [F32, F32] and filt_dt == F32      # (bfloat16 flows widened)
            assert [g[0] for g in gs] == [dt, dt] and [g[2] for g in gs] == [3.0, 5.0]
            assert all(g[1][1] == 1 for g in gs), "the gradients arrive with channel stride 1"
            assert gdt == dt and gst == nhwc and a0.grad.dtype == dt and tuple(a0.grad.stride()) == nhwc and bool((a0.grad == 1).all())
            assert all(f.grad is None for f in offs[0]) and filts[0].grad is None
            # an NCHW-laid-out incoming gradient arrives channels_last
            del log[:]
            a0.grad = None
            outs[1][0].backward(torch.full((2, 4, 6, 10), 7.0, dtype=dt), retain_graph=True)
            assert log[0][0] == "bwd_nhwc" and log[0][1] == [1] and log[0][4] == [(dt, nhwc, 7.0)]
            # ... and so does an expanded one (zero strides)
            del log[:]
            outs[1][0].backward(torch.full((1, 1, 1, 1), 7.0, dtype=dt).expand(2, 4, 6, 10), retain_graph=True)
            assert log[0][4] == [(dt, nhwc, 7.0)]
            # every output unused (autograd runs such a node below a function that used none of them), or a context that
            # needs no gradient: no call, None
            del log[:]
            node = types.SimpleNamespace(saved_tensors=(filts[0].float(), *[o.float() for o in offs[0]]),
                                         needs_input_grad=(True, False, False, False, False), image_layout=((2, 4, 6, 10), dt))
            assert fused._FilterInterpolateCtxNhwc.backward(node, None, None, None) == (None,) * 5
            node.needs_input_grad = (False,) * 5
            assert fused._FilterInterpolateCtxNhwc.backward(node, torch.ones(2, 4, 6, 10, dtype=dt), None, None) == (None,) * 5
            assert log == []
            # a channel-slice context: the gradient is dense channels_last, not laid out with the slice's strides
            del log[:]
            wide = cl(torch.zeros(2, 9, 6, 10, dtype=dt)).requires_grad_()
            o0, _ = fused.FilterInterpolate_ctx(wide[:, 1:5], a2, [offs[0][0], offs[1][0]], filts, train_channels_last=True)
            o0.sum().backward()
            assert [e[0] for e in log] == ["nhwc", "nhwc", "bwd_nhwc"] and log[0][1] == (540, 1, 90, 9) and log[2][6] == nhwc
            assert bool((wide.grad[:, 1:5] == 1).all()) and bool((wide.grad[:, :1] == 0).all())
            # no_grad takes the plain launch
            del log[:]
            with torch.no_grad():
                outs = fused.FilterInterpolate_ctx_all(a0, a2, offs, filts, train_channels_last=True)
            assert log == [("nhwc", nhwc)] * 2 and all(o.grad_fn is None for pair in outs for o in pair)
            # a channels_last context that needs no gradient: the plain launch too
            del log[:]
            outs = fused.FilterInterpolate_ctx_all(cl(c0), cl(c2), offs, filts, train_channels_last=True)
            assert log == [("nhwc", nhwc)] * 2 and all(o.grad_fn is None for pair in outs for o in pair)
            # an NCHW context with the keyword set takes today's Function; the directions may differ in layout
            del log[:]
            n0 = c0.clone().requires_grad_()
            b2 = cl(c2).requires_grad_()
            outs = fused.FilterInterpolate_ctx_all(n0, b2, offs, filts, train_channels_last=True)
            assert log == [("nchw", nchw), ("nhwc", nhwc)]
            del log[:]
            (outs[1][0].sum() + outs[1][1].sum()).backward()
            assert sorted(e[0] for e in log) == ["bwd_nchw", "bwd_nhwc"]
            assert tuple(n0.grad.stride()) == nchw and tuple(b2.grad.stride()) == nhwc
            assert [e[1] for e in log if e[0] == "bwd_nhwc"] == [[11]] and [e[1] for e in log if e[0] == "bwd_nchw"] == [[1]]
            # [B, 1, H, W] is both layouts at once: the old path, keyword or not
            del log[:]
            one = torch.zeros(2, 1, 6, 10, dtype=dt, requires_grad=True)
            fused.FilterInterpolate_ctx_all(one, one, offs, filts, train_channels_last=True)
            assert log == [("nchw", (60, 60, 10, 1))] * 2


# ------------------------------------------------------------------ 5. census of the GPU tests' inputs

def test_the_gpu_inputs_reach_every_tile_class_and_every_call_class():
    want = {"empty", "staged", "staged_split", "direct_window", "direct_filter_size", "direct_fp32", "direct_scale2"}
    got, by_case = set(), {}
    for name, c in fb.all_cases():
        for bf16 in (False, True):
            gouts = [fb.to_bf16(g) for g in c["gouts"]] if bf16 else c["gouts"]
            with np.errstate(all="ignore"):
                k = fb.tile_classes(c["flows"], gouts, c["filt"])
            by_case[name, bf16] = k
            got |= k
    assert got == want, (want - got, got - want)
    for bf16 in (False, True):
        # the fields that are there for one class reach it, in both dtypes
        assert by_case["window", bf16] == {"staged", "staged_split", "direct_window", "empty"}, by_case["window", bf16]
        assert by_case["tiny", bf16] == {"direct_scale2"} and by_case["nonfinite", bf16] == {"direct_fp32"}
        for fcn in fb.FILTER_CHANNELS:
            k = by_case["filter %d" % fcn, bf16]
            assert ("staged" in k and "direct_filter_size" not in k) if fcn == 16 else k == {"direct_filter_size"}, (fcn, k)
        # sub-pixel and border flows reach at most two pixels, a window of at most 39 x 11 cells: every tile staged; a
        # "leaving" flow also holds long valid vectors, so some of its tiles are not
        assert by_case["channels 196", bf16] == {"staged"} and "staged" in by_case["slices", bf16]
    # four flows take two launches
    assert [len(g) for g in fb.launches(fb.case_flows("zero", 4)["flows"])] == [3, 1]
    # the tiny case needs the second scale factor, the non-finite case the fp32 path, by the call's own scale
    c = fb.case_tiny()
    k, fp32, _, scale2 = fb.fc.call_scale(c["gouts"], c["filt"], *fb.FRAME)
    assert k > 126 and not fp32 and scale2 != 1
    c = fb.case_nonfinite()
    with np.errstate(all="ignore"):
        assert fb.fc.call_scale(c["gouts"], c["filt"], *fb.FRAME)[1]
