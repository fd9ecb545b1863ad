"""CPU tests (`-m "not gpu"`) of the bfloat16 context warp (csrc/filterinterp_bf16.hip, tests/fi_ctx_bf16.py):

  * the mirror's ladder and constants equal the dispatch chain and the expressions in the source -- the unit and the header it
    shares with the fp16 kernel, each shared expression in the header alone -- and the tile geometry is the fp16 kernel's (so
    its field builder builds this kernel's fields);
  * the new symbols are declared, exported and in the ctypes table; argument errors return before any launch;
  * the counted-vmcnt pipelines of the new unit hold no scratch operation (the existing spill test's criterion);
  * with the library stubbed, cabi dispatches on the image / gradient dtype and refuses mixes, float16, a bfloat16 flow and a
    row-stride mismatch before any library call;
  * with the launches stubbed, fused widens a bfloat16 flow and filter once, allocates the gradient in the image's dtype, skips
    absent outputs, and sends float32 calls to exactly the entries they reach today;
  * the forward reference agrees with a float64 evaluation within half a bfloat16 ulp plus the float32 evaluation's own error.
"""
import contextlib
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import fi_ctx_bf16 as fb
from tests import fi_windows as fw
from tests.test_abi_and_host import built  # noqa: F401  (fixture)
from tests.test_corr_bf16_host import _FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video-frame-interpolation-based-on-deformable-kernel-region_amd")
FWD, BWD = "vfi_filterinterp_forward_ori_multi_to_bf16", "vfi_filterinterp_backward_ori_image_multi_bf16"
BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16
f32 = np.float32


# ------------------------------------------------------------------ 1. the mirror and the source

def test_ladder_and_constants_match_the_source():
    # one ladder for both 16-bit kernels, in the family header; each unit runs it once
    chain = fw.source_chain(fw.FAMILY16, "FI16_LADDER")
    assert chain == [("kmax" if op else None, op, b, (k,)) for op, b, k in fb.RUNGS]
    units = {name: " ".join(fw.source(name).split()) for name in (fb.SRC, fw.SOURCES["f16"])}
    assert all(u.count("FI16_LADDER(") == 1 for u in units.values())
    c = fb.constants()
    assert c == {"FI16_TW": 64, "FI16_TH": 16, "FI16_PX": 2, "FI16_THREADS": 512, "FI16_PASS_ROWS": 8, "FI16_HDR": 16,
                 "FI16_RING_DWORDS": 15984, "FI16_RMAX": 5, "FI16_KTOP": 8, "FI_PITCH_SKEW": 16}
    # the fp16 kernel's tile geometry, ring and ladder: one set of constants, so fi_windows.build_field("f16", ...) serves both
    d16 = fw.defines(fw.SOURCES["f16"])
    assert all(c[k] == d16[k] for k in c)
    assert not [k for name in units for k in re.findall(r"#define\s+((?:F16|BF|FI16)_\w+)[ \t]+\d", fw.source(name))]
    assert fb.RUNGS == fw.rungs("f16")
    assert [fb.ring_geometry(k) for _, _, k in fb.RUNGS] == [(5, 4), (5, 4), (5, 4), (5, 4), (3, 2)]
    assert all(r * k * c["FI16_THREADS"] <= c["FI16_RING_DWORDS"] and (r - 2) * k <= 63 for k in (2, 3, 4, 6, 8) for r in [fb.ring_geometry(k)[0]])
    src = units[fb.SRC]
    family = " ".join(fw.source(fw.FAMILY16).split())
    # what both kernels share stands in the family header exactly once, and in neither unit
    for expr in ("t.Lc = clampi(t.L, 0, w - 4);",
                 "fi_box_add4(g.valid, t.Lc, t.T, box.bx_lo, box.by_lo, box.bx_hi, box.by_hi);",
                 "const int bx0 = any_valid ? box[0] & ~1 : 0, by0 = box[1];",
                 "const int bw = any_valid ? (box[2] - bx0 + 2) >> 1 : 0;",
                 "const int bh = any_valid ? box[3] - by0 + 1 : 0;",
                 "const int pitch = fi_pitch_for(bw);",
                 "const bool staged = filter_channels == 16 && w >= 4 && ((s1.h | s1.c | s1.b) & 1) == 0 && "
                 "(reinterpret_cast<uintptr_t>(input1) & 3) == 0 && (int64_t)h * s1.h * 2 < INT_MAX;",
                 "const FiSplit split = fi_channel_split(ntiles, channel, 4.3);"):
        assert family.count(expr) == 1 and not any(expr in u for u in units.values()), expr
    # what changes a kernel's code when a helper forms it stays written out, the same in both units
    for expr in ("const int n = win.pitch * win.bh;",
                 "const int kmax = (n + FI16_THREADS - 1) / FI16_THREADS;",
                 "if (kmax > FI16_KTOP) {"):
        assert all(u.count(expr) == 1 for u in units.values()) and expr not in family, expr
    # this kernel's own
    for expr in ("const int shift = L[p] - Lc[p];",
                 "moved = moved || (g.valid && shift != 0);",
                 "if (so.h != s1.h || batch > 65535) return VFI_ERR_SHAPE;"):
        assert expr in src, expr
    # the arithmetic is the float32 kernels': fi4_pixel on widened taps, no folded weights; the family header knows no format
    assert src.count("fi4_pixel(v, px[p].f, px[p].alpha, px[p].beta)") == 2 and "v_fma_mix" not in src and "__half" not in src
    assert not [t for t in ("__half", "v_fma_mix", "bf16_", "fi4_pixel") if t in family]
    # the backward instantiates the float32 call's templates
    assert "backward_image_multi<bf16_t>(" in src and '#include "filterinterp_ctx_bwd.h"' in fw.source(fb.SRC)
    assert "backward_image_multi<float>(" in fw.source("filterinterp_ctx_bwd.hip") and "FI_CTX_BWD" not in fw.source("filterinterp_ctx_bwd.h")


def test_hand_worked_tiles():
    h, w = 32, 130
    zero = np.zeros((1, 2, h, w), f32)
    t = fb.tiles(zero, h, w)
    # tile (0, 0): windows of columns -1 .. 65 moved to 0 .. 65, rows -1 .. 17: 33 dwords x 19 rows at pitch 48
    assert (t["bx0"][0, 0, 0], t["bw"][0, 0, 0], t["bh"][0, 0, 0], t["pitch"][0, 0, 0]) == (0, 33, 19, 48)
    assert t["label"][0, 0, 0] == "K=2" and t["left"][0, 0, 0] and not t["right1"][0, 0, 0]
    # tile (0, 1): columns 63 .. 129: bx0 = 62, 34 dwords; no window moved
    assert (t["bx0"][0, 0, 1], t["bw"][0, 0, 1]) == (62, 34) and not t["edge"][0, 0, 1]
    # the ragged last tile column (x = 128, 129): windows 127 .. 131 moved to 126 .. 129, by one and by two columns
    assert t["right1"][0, 0, 2] and t["right2"][0, 0, 2] and not t["left"][0, 0, 2]
    assert fb.features(zero, h, w) >= {"K=2", "interior", "edge left", "edge right 1", "edge right 2", "ragged last column"}
    gone = zero.copy()
    gone[0, 0, :16, 64:128] = 1000
    assert fb.tiles(gone, h, w)["label"][0, 0, 1] == "none"
    # staged or direct, by layout
    assert fb.takes_staged((1, 3, 8, 16), (384, 128, 16, 1), 256, 16)
    for shape, stride, ptr, fcn in (((1, 3, 8, 16), (384, 128, 16, 1), 258, 16), ((1, 3, 8, 15), (360, 120, 15, 1), 256, 16),
                                    ((1, 3, 8, 16), (384, 128, 16, 1), 256, 25), ((1, 3, 8, 3), (96, 32, 4, 1), 256, 16),
                                    ((1, 3, 8, 16), (385, 128, 16, 1), 256, 16)):
        assert not fb.takes_staged(shape, stride, ptr, fcn)


def test_the_all_class_field_exercises_every_feature():
    h, w = fw.field_shape("f16")
    flow = fw.build_field("f16", np.random.default_rng(3000), 2, h, w)["flow"]
    assert not [x for x in fb.ALL_FEATURES if x not in fb.features(flow, h, w)]
    assert (fw.classes("f16", flow, h, w) == fb.tiles(flow, h, w)["label"]).all()


# ------------------------------------------------------------------ 2. symbols, table, argument errors, assembly

def _params(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vfi_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "the header does not declare %s" % name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", [FWD, BWD])
def test_header_library_and_ctypes_table_agree(built, name):  # noqa: F811
    from vfidkr_amd import cabi
    want = []
    for p in _params(name):
        if "*" in p or p.startswith("vfi_stream_t"):
            want.append(ctypes.c_void_p)
        elif p.startswith("vfi_strides"):
            want.append(cabi.Strides)
        else:
            assert re.fullmatch(r"int \w+", p), p
            want.append(ctypes.c_int)
    assert cabi.SIGNATURES[name] == want and len(want) == 15
    assert hasattr(ctypes.CDLL(built.LIB_PATH), name)
    fn = getattr(cabi.lib(), name)
    assert fn.argtypes == want and fn.restype is ctypes.c_int
    # the float32 twins' parameter lists with the image-side pointers typeless
    drop = lambda ps: [re.sub(r"\b(const )?(float|void)\* ?(const\*)? ?(\w+?)(_bf16)?$", r"ptr \4", p) for p in ps]      # noqa: E731
    assert drop(_params(name)) == drop(_params(name[:-len("_bf16")]))
    assert cabi.INTERNAL_SIGNATURES[FWD + "_direct"] == cabi.SIGNATURES[FWD] and hasattr(ctypes.CDLL(built.LIB_PATH), FWD + "_direct")
    text = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "filterinterp_bf16.hip" in re.search(r"^SRCS\s*:=\s*(.*)$", text, flags=re.M).group(1).split()
    assert "filterinterp_bf16" in re.search(r"^STAGED\s*:=\s*(.*)$", text, flags=re.M).group(1).split()


def test_argument_errors_return_before_any_launch(built):  # noqa: F811
    from vfidkr_amd import cabi
    lib, E = cabi.lib(), cabi.VFI_ERR_SHAPE
    p = ctypes.c_void_p(4096)               # never dereferenced
    two, hole = (ctypes.c_void_p * 2)(4096, 4096), (ctypes.c_void_p * 2)(4096, None)
    s = cabi.Strides(384, 64, 8)
    for name in (FWD, FWD + "_direct"):
        f = getattr(lib, name)

        def fwd(img=p, flows=two, filt=p, outs=two, n=2, dims=(1, 3, 8, 8), fcn=16, so=s):
            return f(img, flows, filt, outs, n, *dims, fcn, s, s, s, so, None)
        assert fwd(img=None) == E and fwd(flows=None) == E and fwd(filt=None) == E and fwd(outs=None) == E
        assert fwd(flows=hole) == E and fwd(outs=hole) == E and fwd(n=0) == E and fwd(n=-1) == E and fwd(fcn=0) == E
        for dims in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1), (65536, 3, 8, 8)):
            assert fwd(dims=dims) == E
        assert fwd(so=cabi.Strides(384, 64, 10)) == E                                   # s_out.h != s1.h
    b = getattr(lib, BWD)

    def bwd(flows=two, filt=p, gouts=two, g1=p, n=2, dims=(1, 3, 8, 8), fcn=16):
        return b(flows, filt, gouts, g1, n, *dims, fcn, s, s, s, s, None)
    assert bwd(flows=None) == E and bwd(gouts=None) == E and bwd(filt=None) == E and bwd(g1=None) == E
    assert bwd(flows=hole) == E and bwd(gouts=hole) == E and bwd(n=0) == E and bwd(fcn=0) == E
    for dims in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1)):
        assert bwd(dims=dims) == E


def test_no_register_spills_inside_the_counted_vmcnt_pipelines(built):  # noqa: F811
    """tests/test_abi_and_host's criterion on the new unit: ten instances of the channel loop (five rungs, interior and EDGE),
    each a steady-state loop with a counted wait, none with a scratch operation"""
    path = os.path.join(PKG, "lib", "filterinterp_bf16.s")
    assert os.path.exists(path), path
    checked, bad, counted = fb.pipeline_spills(path)
    assert not bad, "scratch operations inside an LDS-DMA pipeline: %s" % bad[:4]
    # (the K = 8 ring holds two windows in flight at most: its one counted wait is vmcnt(8) as well)
    assert checked >= 20 and counted >= 10, (checked, counted)
    text = open(path).read()
    # the backward's bfloat16 instances live in this unit, and hold no scratch either (tests/test_fi_ctx_backward_host's rule)
    names = re.findall(r"^(_Z\S*fi_ctx_\S*):", text, flags=re.M)
    assert len(names) == 3, names
    for name in names:
        body = text.split(name + ":", 1)[1].split(".Lfunc_end", 1)[0]
        assert not re.search(r"^\s*scratch_", body, flags=re.M), name


# ------------------------------------------------------------------ 3. cabi's dispatch, library stubbed

class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


@pytest.fixture
def stubbed(monkeypatch):
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi
    rec = _Recorder()
    monkeypatch.setattr(cabi, "lib", lambda: rec)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: types.SimpleNamespace(cuda_stream=0))
    return cabi, rec


def _t(dtype, *shape, cuda=True):
    return _FakeCuda(torch.zeros(*shape, dtype=dtype), cuda)


def test_cabi_sends_each_dtype_to_its_entries(stubbed):
    cabi, rec = stubbed
    for dt, suffix in ((BF, "_bf16"), (F32, "")):
        del rec.calls[:]
        img, outs = _t(dt, 2, 5, 6, 10), [_t(dt, 2, 5, 6, 10) for _ in range(2)]
        flows, filt = [_t(F32, 2, 2, 6, 10) for _ in range(2)], _t(F32, 2, 16, 6, 10)
        wide = _t(dt, 2, 9, 6, 10)
        slices = [_FakeCuda(wide.t[:, 1:6]), _FakeCuda(wide.t[:, 3:8])]
        assert cabi.filterinterp_forward_ori_multi(img, flows, filt, outs) == 0
        assert cabi.filterinterp_forward_ori_multi_to(img, flows, filt, slices) == 0
        assert cabi.filterinterp_backward_ori_image_multi(flows, filt, outs, img) == 0
        names = [n for n, _ in rec.calls]
        if suffix:
            assert names == [FWD, FWD, BWD]
            assert cabi.filterinterp_forward_ori_multi_to(img, flows, filt, slices, direct=True) == 0
            assert rec.calls[-1][0] == FWD + "_direct"
        else:
            assert names == ["vfi_filterinterp_forward_ori_multi", "vfi_filterinterp_forward_ori_multi_to",
                             "vfi_filterinterp_backward_ori_image_multi"]
            with pytest.raises(RuntimeError, match="direct=True"):
                cabi.filterinterp_forward_ori_multi_to(img, flows, filt, slices, direct=True)
        # the destination's strides travel as s_out, in elements: the dense call passes the image's, the slice its own
        so = [a[13] for n, a in rec.calls if n.startswith("vfi_filterinterp_forward_ori_multi_to")]
        assert [(s.b, s.c, s.h) for s in so[:2]] == ([(300, 60, 10), (540, 60, 10)] if suffix else [(540, 60, 10)])
        assert all(len(a) == len(cabi.SIGNATURES.get(n) or cabi.INTERNAL_SIGNATURES[n]) for n, a in rec.calls)


def test_cabi_refusals_launch_nothing(stubbed):
    cabi, rec = stubbed
    img, out, g = _t(BF, 2, 5, 6, 10), _t(BF, 2, 5, 6, 10), _t(BF, 2, 5, 6, 10)
    fimg, fout = _t(F32, 2, 5, 6, 10), _t(F32, 2, 5, 6, 10)
    flow, filt = _t(F32, 2, 2, 6, 10), _t(F32, 2, 16, 6, 10)
    bflow, bfilt = _t(BF, 2, 2, 6, 10), _t(BF, 2, 16, 6, 10)
    himg, hout = _t(F16, 2, 5, 6, 10), _t(F16, 2, 5, 6, 10)
    fwd, to, bwd = cabi.filterinterp_forward_ori_multi, cabi.filterinterp_forward_ori_multi_to, cabi.filterinterp_backward_ori_image_multi
    for call in (lambda: fwd(img, [flow], filt, [fout]), lambda: to(img, [flow], filt, [fout]),           # image-side mixes
                 lambda: fwd(img, [flow, flow], filt, [out, fout]), lambda: bwd([flow], filt, [fout], img),
                 lambda: bwd([flow, flow], filt, [g, fout], img), lambda: fwd(img, [flow], filt, [hout])):
        with pytest.raises(RuntimeError, match="tensors must be bfloat16"):
            call()
    for call in (lambda: fwd(fimg, [flow], filt, [out]), lambda: to(fimg, [flow], filt, [out]), lambda: bwd([flow], filt, [g], fimg),
                 lambda: fwd(himg, [flow], filt, [hout]), lambda: to(himg, [flow], filt, [hout]), lambda: bwd([flow], filt, [hout], himg),
                 # flows and filter are float32 whatever the image is
                 lambda: fwd(img, [bflow], filt, [out]), lambda: fwd(img, [flow], bfilt, [out]), lambda: to(img, [flow, bflow], filt, [out, out]),
                 lambda: bwd([bflow], filt, [g], img), lambda: bwd([flow], bfilt, [g], img), lambda: fwd(fimg, [bflow], filt, [fout]),
                 lambda: fwd(img, [_t(F16, 2, 2, 6, 10)], filt, [out])):
        with pytest.raises(RuntimeError, match="tensors must be float32"):
            call()
    cpu_img = _t(BF, 2, 5, 6, 10, cuda=False)
    for call in (lambda: fwd(cpu_img, [flow], filt, [out]), lambda: to(img, [flow], filt, [cpu_img]), lambda: bwd([flow], filt, [cpu_img], img),
                 lambda: fwd(img, [_t(F32, 2, 2, 6, 10, cuda=False)], filt, [out])):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call()
    # a destination whose rows are not the image's rows, other shapes, a missing output: refused (1), nothing launched
    wide = _t(BF, 2, 5, 6, 12)
    assert to(img, [flow], filt, [_FakeCuda(wide.t[:, :, :, :10])]) == 1
    assert to(img, [flow], filt, [_t(BF, 2, 4, 6, 10)]) == 1 and to(img, [flow, flow], filt, [out]) == 1 and fwd(img, [], filt, []) == 1
    assert fwd(img, [flow], filt, [_FakeCuda(wide.t[:, :, :, :10])]) == 1
    assert bwd([flow], filt, [_t(BF, 2, 5, 6, 11)], img) == 1 and bwd([flow], _t(F32, 2, 16, 6, 11), [g], img) == 1
    assert rec.calls == []


# ------------------------------------------------------------------ 4. fused, launches stubbed

def test_fused_plumbing(monkeypatch):
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi, fused
    log = []

    def fwd(image, flows, filt, outs):
        log.append(("fwd", image.dtype, [f.dtype for f in flows], filt.dtype, [o.dtype for o in outs], [id(f) for f in flows], id(filt)))
        for t, o in enumerate(outs):
            o.fill_(t + 1)
        return 0

    def bwd(flows, filt, gouts, gimg):
        log.append(("bwd", gimg.dtype, [f.dtype for f in flows], filt.dtype, [g.dtype for g in gouts], len(flows)))
        gimg.fill_(len(flows))
        return 0
    monkeypatch.setattr(cabi, "filterinterp_forward_ori_multi", fwd)
    monkeypatch.setattr(cabi, "filterinterp_backward_ori_image_multi", bwd)
    monkeypatch.setattr(cabi, "filterinterp_forward_ori_multi_to", lambda *a, **k: pytest.fail("the context warp writes dense outputs"))
    for dt in (BF, F32):
        for fdt in ((BF, F32) if dt == BF else (F32,)):
            del log[:]
            c0 = torch.zeros(1, 4, 6, 10, dtype=dt, requires_grad=True)
            c2 = torch.zeros(1, 4, 6, 10, dtype=dt)
            offs = [[torch.zeros(1, 2, 6, 10, dtype=fdt, requires_grad=True) for _ in range(3)],
                    [torch.zeros(1, 2, 6, 10, dtype=fdt) for _ in range(3)]]
            filts = [torch.zeros(1, 16, 6, 10, dtype=fdt, requires_grad=True), torch.zeros(1, 16, 6, 10, dtype=fdt)]
            outs = fused.FilterInterpolate_ctx_all(c0, c2, offs, filts)
            # one launch per direction; the kernels see float32 flows and filter, widened once per direction
            assert [e[:5] for e in log] == [("fwd", dt, [F32] * 3, F32, [dt] * 3)] * 2
            if fdt == F32:                                       # float32 tensors pass through untouched
                assert log[0][5] == [id(o) for o in offs[0]] and log[0][6] == id(filts[0])
            assert all(a.dtype == dt and b.dtype == dt and a.grad_fn is not None and b.grad_fn is None for a, b in outs)
            (outs[0][0].float().sum() + outs[2][0].float().sum()).backward()            # the middle offset: an absent gradient
            assert log[2] == ("bwd", dt, [F32] * 2, F32, [dt] * 2, 2)
            assert c0.grad.dtype == dt and float(c0.grad.float().min()) == 2.0
            assert all(o.grad is None for o in offs[0]) and filts[0].grad is None
            # the single-offset form, no gradient wanted: the plain launch
            del log[:]
            with torch.no_grad():
                o0, o2 = fused.FilterInterpolate_ctx(c0, c2, [offs[0][1], offs[1][1]], filts)
            assert [e[:5] for e in log] == [("fwd", dt, [F32], F32, [dt])] * 2 and o0.grad_fn is None and o0.dtype == dt


def test_fused_rectify_inputs_stays_float32(stubbed):
    """a bfloat16 context tensor into the float32 rectify buffer is a dtype mix: refused before any launch"""
    cabi, rec = stubbed
    with pytest.raises(RuntimeError, match="tensors must be"):
        cabi.filterinterp_forward_ori_multi_to(_t(BF, 1, 4, 6, 10), [_t(F32, 1, 2, 6, 10)], _t(F32, 1, 16, 6, 10),
                                               [_FakeCuda(torch.zeros(1, 9, 6, 10)[:, 2:6])])
    assert rec.calls == []


# ------------------------------------------------------------------ 5. the forward reference against float64

@pytest.mark.parametrize("filter_channels", [16, 25])
def test_forward_reference_agrees_with_float64(oracle, filter_channels):
    """|to_bf16(float32 evaluation) - float64| <= half a bfloat16 ulp + the float32 evaluation's own error.  The float32
    evaluation rounds each tap product into its chain (at most fs^2 / 4 + fs roundings per quadrant), the four blend weights
    (two roundings each) and the three blend additions: every term's relative error stays below (1 + u)^(fs^2 / 4 + 8) - 1,
    u = 2^-24, so its error is below (fs^2 / 4 + 9) u A with A = sum |weight x tap x value|.  The half ulp is taken at the
    float32 value's magnitude, |R| + that error at most."""
    rng = np.random.default_rng(5 + filter_channels)
    B, C, h, w = 2, 3, 40, 150
    img = fb.to_bf16(rng.standard_normal((B, C, h, w)).astype(f32))
    flow = (rng.uniform(-4, 4, (B, 2, h, w))).astype(f32)
    flow[:, :, :3, :5] = 1000                                   # some invalid pixels: copied through
    filt = (rng.random((B, filter_channels, h, w), dtype=f32) - f32(0.3)).astype(f32)
    want = fb.forward_reference(oracle, img, flow, filt)
    R, A = fb.forward_f64(img, flow, filt)
    fs = int(np.sqrt(filter_channels))
    err32 = (fs * fs / 4 + 9) * 2.0 ** -24 * A
    tol = fb.half_ulp(np.abs(R) + err32) + err32
    bad = ~(np.abs(want.astype(np.float64) - R) <= tol)
    assert not bad.any(), (int(bad.sum()), float(np.abs(want - R).max()))
    valid = fw.samples(flow, h, w)[0]
    assert (~valid).any() and np.array_equal(want[np.broadcast_to(~valid[:, None], img.shape)], img[np.broadcast_to(~valid[:, None], img.shape)])
