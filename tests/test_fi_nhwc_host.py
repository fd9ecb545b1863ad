"""CPU tests (`-m "not gpu"`) of the channels_last context warp (csrc/filterinterp_nhwc.hip, tests/fi_nhwc.py):

  * the header declares both entries with the layouts' own structs, the library exports them, the ctypes table carries them;
  * every refusal of the entries returns VFI_ERR_SHAPE before any launch (no GPU is touched);
  * with the library stubbed, cabi.filterinterp_forward_nhwc_multi_to passes channels_last strides in elements, and refuses
    layouts (1) and dtypes / devices (RuntimeError) before a library call; the NCHW wrappers keep refusing stride(3) != 1;
  * with the launches stubbed, fused sends a contiguous context where it always went, a channels_last one to the new wrapper
    once per direction with channels_last outputs, refuses one that requires grad with nothing called, and keeps a
    [B, 1, H, W] tensor (both layouts at once) on the old path;
  * the mirror's constants are the source's, and the width mirror gives the library's own answer (a host-only internal entry);
  * the expected-value helper agrees with a planted case worked by hand.
"""
import contextlib
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import fi_nhwc as fn
from tests.test_abi_and_host import built, header_functions  # noqa: F401  (fixture)
from tests.test_corr_bf16_host import _FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video-frame-interpolation-based-on-deformable-kernel-region_amd")
F32N, BF16N = "vfi_filterinterp_forward_ori_nhwc_multi_to", "vfi_filterinterp_forward_ori_nhwc_multi_to_bf16"
BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16
f32 = np.float32


# ------------------------------------------------------------------ 1. header, library, table

def _params(name):
    text = open(os.path.join(ROOT, "include", "vfi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
    assert m, "the header does not declare %s" % name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", [F32N, BF16N])
def test_header_library_and_ctypes_table_agree(built, name):  # noqa: F811
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
    assert [p.split()[0] for p in _params(name)[10:14]] == ["vfi_strides_nhwc", "vfi_strides4", "vfi_strides4", "vfi_strides_nhwc"]
    assert hasattr(ctypes.CDLL(built.LIB_PATH), name)
    fn_ = getattr(cabi.lib(), name)
    assert fn_.argtypes == want and fn_.restype is ctypes.c_int
    # the structs are the header's: three and four int64 fields in its order
    text = open(os.path.join(ROOT, "include", "vfi_hip.h")).read()
    for struct, cls in (("vfi_strides_nhwc", cabi.StridesNhwc), ("vfi_strides4", cabi.Strides4)):
        m = re.search(r"typedef struct " + struct + r" \{\s*int64_t ([\w, ]+);", text)
        assert m and [f.strip() for f in m.group(1).split(",")] == [f for f, _ in cls._fields_]
        assert all(t is ctypes.c_int64 for _, t in cls._fields_)
    # the float32 and the bfloat16 entry differ in the image-side pointers only
    drop = lambda ps: [re.sub(r"\b(const )?(float|void)\* ?(const\*)? ?(\w+?)(_bf16)?$", r"ptr \4", p) for p in ps]      # noqa: E731
    assert drop(_params(F32N)) == drop(_params(BF16N))
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "filterinterp_nhwc.hip" in re.search(r"^SRCS\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()


def test_argument_errors_return_before_any_launch(built):  # noqa: F811
    from vfidkr_amd import cabi
    lib, E = cabi.lib(), cabi.VFI_ERR_SHAPE
    p = ctypes.c_void_p(4096)               # never dereferenced
    two, hole = (ctypes.c_void_p * 2)(4096, 4096), (ctypes.c_void_p * 2)(4096, None)
    s1, s4 = cabi.StridesNhwc(192, 24, 3), cabi.Strides4(128, 64, 8, 1)
    for name in (F32N, BF16N):
        f = getattr(lib, name)

        def fwd(img=p, flows=two, filt=p, outs=two, n=2, dims=(1, 3, 8, 8), fcn=16):
            return f(img, flows, filt, outs, n, *dims, fcn, s1, s4, s4, s1, None)
        assert fwd(img=None) == E and fwd(flows=None) == E and fwd(filt=None) == E and fwd(outs=None) == E
        assert fwd(flows=hole) == E and fwd(outs=hole) == E and fwd(n=0) == E and fwd(n=-1) == E and fwd(fcn=0) == E
        for dims in ((0, 3, 8, 8), (1, 0, 8, 8), (1, -2, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1), (65536, 3, 8, 8),
                     (65535, 3, 4 * 64, 32 * 65)):            # batch beyond the limit; more than 2^28 tiles
            assert fwd(dims=dims) == E, dims


# ------------------------------------------------------------------ 2. cabi, library stubbed

class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn_(*args):
            self.calls.append((name, args))
            return 0
        return fn_


@pytest.fixture
def stubbed(monkeypatch):
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi
    rec = _Recorder()
    monkeypatch.setattr(cabi, "lib", lambda: rec)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: types.SimpleNamespace(cuda_stream=0))
    return cabi, rec


def _t(dtype, *shape, cuda=True, cl=False):
    t = torch.zeros(*shape, dtype=dtype)
    return _FakeCuda(t.contiguous(memory_format=torch.channels_last) if cl else t, cuda)


def test_cabi_passes_channels_last_layouts_in_elements(stubbed):
    cabi, rec = stubbed
    for dt, name in ((F32, F32N), (BF, BF16N)):
        del rec.calls[:]
        img = _t(dt, 2, 5, 6, 10, cl=True)
        wide = _t(dt, 2, 9, 6, 10, cl=True)
        outs = [_FakeCuda(wide.t[:, 1:6]), _FakeCuda(torch.zeros_like(wide.t)[:, 1:6])]
        flows = [_t(F32, 2, 2, 6, 10), _t(F32, 2, 2, 6, 10)]
        filt = _t(F32, 2, 16, 6, 10, cl=True)
        assert cabi.filterinterp_forward_nhwc_multi_to(img, flows, filt, outs) == 0
        (got, a), = rec.calls
        assert got == name and len(a) == len(cabi.SIGNATURES[name])
        assert a[4:10] == (2, 2, 5, 6, 10, 16)
        s1, s2, s3, so = a[10:14]
        assert (s1.b, s1.h, s1.w) == (300, 50, 5) and (so.b, so.h, so.w) == (540, 90, 9)
        assert (s2.b, s2.c, s2.h, s2.w) == (120, 60, 10, 1) and (s3.b, s3.c, s3.h, s3.w) == (960, 1, 160, 16)
        # a one-channel image is channels_last whatever its channel stride says
        assert cabi.filterinterp_forward_nhwc_multi_to(_t(dt, 2, 1, 6, 10), flows[:1], filt, [_t(dt, 2, 1, 6, 10)]) == 0


def test_cabi_refusals_call_nothing(stubbed):
    cabi, rec = stubbed
    call = cabi.filterinterp_forward_nhwc_multi_to
    img, out = _t(BF, 2, 5, 6, 10, cl=True), _t(BF, 2, 5, 6, 10, cl=True)
    fimg, fout = _t(F32, 2, 5, 6, 10, cl=True), _t(F32, 2, 5, 6, 10, cl=True)
    flow, filt = _t(F32, 2, 2, 6, 10), _t(F32, 2, 16, 6, 10)
    # layouts and shapes: 1, silently, as the bindings do
    assert call(_t(BF, 2, 5, 6, 10), [flow], filt, [out]) == 1                  # an NCHW image
    assert call(img, [flow], filt, [_t(BF, 2, 5, 6, 10)]) == 1                  # an NCHW destination
    assert call(img, [flow, flow], filt, [out]) == 1 and call(img, [], filt, []) == 1
    assert call(img, [flow], filt, [_t(BF, 2, 4, 6, 10, cl=True)]) == 1
    assert call(img, [_t(F32, 2, 2, 6, 11)], filt, [out]) == 1 and call(img, [_t(F32, 2, 3, 6, 10)], filt, [out]) == 1
    assert call(img, [flow], _t(F32, 2, 16, 7, 10), [out]) == 1 and call(img, [flow], _t(F32, 1, 16, 6, 10), [out]) == 1
    assert call(img, [flow, _t(F32, 2, 2, 6, 10, cl=True)], filt, [out, out]) == 1            # two flow layouts in one call
    wide = _t(BF, 2, 9, 6, 10, cl=True)
    assert call(img, [flow, flow], filt, [out, _FakeCuda(wide.t[:, :5])]) == 1                # two destination layouts
    # dtypes and devices: raised
    for bad in (lambda: call(img, [flow], filt, [fout]), lambda: call(img, [flow, flow], filt, [out, fout])):
        with pytest.raises(RuntimeError, match="tensors must be bfloat16"):
            bad()
    for bad in (lambda: call(fimg, [flow], filt, [out]), lambda: call(_t(F16, 2, 5, 6, 10, cl=True), [flow], filt, [_t(F16, 2, 5, 6, 10, cl=True)]),
                lambda: call(img, [_t(BF, 2, 2, 6, 10)], filt, [out]), lambda: call(img, [flow], _t(BF, 2, 16, 6, 10), [out]),
                lambda: call(fimg, [flow], _t(F16, 2, 16, 6, 10), [fout])):
        with pytest.raises(RuntimeError, match="tensors must be float32"):
            bad()
    for bad in (lambda: call(_t(BF, 2, 5, 6, 10, cl=True, cuda=False), [flow], filt, [out]),
                lambda: call(img, [_t(F32, 2, 2, 6, 10, cuda=False)], filt, [out])):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            bad()
    # the NCHW wrappers refuse a channels_last image as before
    assert cabi.filterinterp_forward_ori_multi(img, [flow], filt, [out]) == 1
    assert cabi.filterinterp_forward_ori_multi_to(img, [flow], filt, [out]) == 1
    assert cabi.filterinterp_forward_ori(fimg, flow, filt, fout) == 1
    assert rec.calls == []


# ------------------------------------------------------------------ 3. fused, launches stubbed

def test_fused_dispatch(monkeypatch):
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi, fused
    log = []

    def record(tag):
        def fn_(image, flows, filt, outs):
            log.append((tag, image.dtype, tuple(image.stride()), [f.dtype for f in flows], filt.dtype,
                        [(o.dtype, tuple(o.stride())) for o in outs]))
            for o in outs:
                o.zero_()
            return 0
        return fn_
    monkeypatch.setattr(cabi, "filterinterp_forward_ori_multi", record("nchw"))
    monkeypatch.setattr(cabi, "filterinterp_forward_nhwc_multi_to", record("nhwc"))
    monkeypatch.setattr(cabi, "filterinterp_backward_ori_image_multi", lambda *a: pytest.fail("no backward here"))
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)      # noqa: E731
    for dt in (F32, BF):
        for fdt in ((F32, BF) if dt == BF else (F32,)):
            offs = [[torch.zeros(2, 2, 6, 10, dtype=fdt) for _ in range(3)] for _ in range(2)]
            filts = [torch.zeros(2, 16, 6, 10, dtype=fdt), cl(torch.zeros(2, 16, 6, 10, dtype=fdt))]
            c0, c2 = torch.zeros(2, 4, 6, 10, dtype=dt), torch.zeros(2, 4, 6, 10, dtype=dt)
            nchw, nhwc = (240, 60, 10, 1), (240, 1, 40, 4)
            # contiguous contexts: the entry they always reached
            del log[:]
            fused.FilterInterpolate_ctx_all(c0, c2, offs, filts)
            assert log == [("nchw", dt, nchw, [F32] * 3, F32, [(dt, nchw)] * 3)] * 2
            # channels_last contexts: the new wrapper, once per direction, outputs laid out as the input
            del log[:]
            outs = fused.FilterInterpolate_ctx_all(cl(c0), cl(c2), offs, filts)
            assert log == [("nhwc", dt, nhwc, [F32] * 3, F32, [(dt, nhwc)] * 3)] * 2
            assert len(outs) == 3 and all(tuple(o.stride()) == nhwc and o.grad_fn is None for pair in outs for o in pair)
            # a channel slice of a wider channels_last tensor is one too
            del log[:]
            wide = cl(torch.zeros(2, 9, 6, 10, dtype=dt))
            fused.FilterInterpolate_ctx(wide[:, 1:5], wide[:, 5:9], [offs[0][0], offs[1][0]], filts)
            assert [e[0] for e in log] == ["nhwc"] * 2 and log[0][2] == (540, 1, 90, 9) and log[0][5] == [(dt, (540, 1, 90, 9))]
            # one direction of each layout
            del log[:]
            fused.FilterInterpolate_ctx_all(cl(c0), c2, offs, filts)
            assert [e[0] for e in log] == ["nhwc", "nchw"]
            # requires grad: the NCHW tensor trains (not stubbed here: only checked to be untouched by the new branch) ...
            del log[:]
            with pytest.raises(RuntimeError, match="forward-only.*contiguous"):
                fused.FilterInterpolate_ctx_all(cl(c0).requires_grad_(), cl(c2), offs, filts)
            with pytest.raises(RuntimeError, match="forward-only"):
                fused.FilterInterpolate_ctx_all(cl(c0), cl(c2).requires_grad_(), offs, filts)
            assert log == []                                     # (both contexts are looked at before the first launch)
            # ... and with grad mode off the same tensors are warped
            del log[:]
            with torch.no_grad():
                fused.FilterInterpolate_ctx_all(cl(c0).requires_grad_(), cl(c2), offs, filts)
            assert [e[0] for e in log] == ["nhwc"] * 2
            # [B, 1, H, W] is both layouts at once: the old path
            del log[:]
            one = torch.zeros(2, 1, 6, 10, dtype=dt)
            assert one.is_contiguous() and one.is_contiguous(memory_format=torch.channels_last)
            fused.FilterInterpolate_ctx_all(one, cl(one), offs, filts)
            assert [e[0] for e in log] == ["nchw"] * 2


# ------------------------------------------------------------------ 4. the mirrors

def test_constants_and_the_width_mirror():
    c = fn.constants()
    assert c == {"FN_TW": 32, "FN_TH": 4, "FN_PIXELS": 128, "FN_THREADS": 512}
    assert c["FN_PIXELS"] == c["FN_TW"] * c["FN_TH"] and c["FN_THREADS"] == 4 * c["FN_PIXELS"]
    # the library's own choice (a host-only internal entry) is the mirror's, layout by layout
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi
    lib = cabi.lib()

    def chosen(esize, shape_, image, outs, fs=4):
        op = (ctypes.c_void_p * len(outs))(*[p for p, _ in outs])
        return lib.vfi_filterinterp_nhwc_access_width(esize, ctypes.c_void_p(image[0]), op, len(outs), shape_[0], shape_[2], shape_[3],
                                                      fs * fs, cabi.StridesNhwc(*image[1]), cabi.StridesNhwc(*outs[0][1]))
    mirror = fn.vector_width

    def both(esize, shape_, image, outs, fs=4):
        got = chosen(esize, shape_, image, outs, fs)
        assert got == mirror(esize, shape_, image, outs, fs), (got, esize, shape_, image, outs, fs)
        return got
    fn_vector_width = both
    shape = (2, 196, 19, 37)
    dense = lambda c_: (19 * 37 * c_, 37 * c_, c_)      # noqa: E731
    for esize, want in ((4, 4), (2, 4)):
        assert fn_vector_width(esize, shape, (256, dense(196)), [(512, dense(196))]) == want
    assert fn_vector_width(2, shape, (256, dense(440)), [(256 + 96, dense(440))]) == 8
    assert fn_vector_width(2, shape, (256, dense(440)), [(256 + 96, dense(440)), (256 + 90, dense(437))]) == 1
    assert fn_vector_width(2, shape, (256, dense(440)), [(256 + 8, dense(440))]) == 4
    assert fn_vector_width(4, shape, (256, dense(440)), [(256 + 8, dense(440))]) == 2
    assert fn_vector_width(4, shape, (256, dense(440)), [(256 + 16, dense(440))], fs=5) == 1
    # an odd batch stride matters only with more than one batch item
    odd = (19 * 37 * 8 + 1, 37 * 8, 8)
    assert fn_vector_width(2, (1, 8, 19, 37), (256, odd), [(512, odd)]) == 8
    assert fn_vector_width(2, (2, 8, 19, 37), (256, odd), [(512, odd)]) == 1


# ------------------------------------------------------------------ 5. the expectation, by hand

@pytest.mark.parametrize("bf16", [False, True])
def test_expected_agrees_with_a_case_worked_by_hand(oracle, bf16):
    """6 x 7 frame, 2 channels of small integers (exact in bfloat16 and in every sum), taps that are powers of two, and three
    planted pixels: (y 2, x 3) with flow (0.5, 0.25) -- cell (3, 2), window rows 1..4, columns 2..5 --; the corner (0, 0) with
    flow (0.25, 0.5) -- rows -1..2 and columns -1..2, clamped: row 0 and column 0 are read twice --; and (y 4, x 1) with a
    flow that leaves the frame, which copies the input through.  Every product and sum is exact, so the order does not matter."""
    h, w = 6, 7
    img = np.arange(2 * h * w, dtype=f32).reshape(1, 2, h, w) % 13 - 6
    filt = np.zeros((1, 16, h, w), f32)
    taps = (2.0 ** -np.arange(16) * np.where(np.arange(16) % 3 == 0, -1, 1)).astype(f32)
    filt[0, :, 2, 3] = taps
    filt[0, :, 0, 0] = taps[::-1]
    flow = np.zeros((1, 2, h, w), f32)
    flow[0, :, 2, 3] = (0.5, 0.25)
    flow[0, :, 0, 0] = (0.25, 0.5)
    flow[0, :, 4, 1] = (-1.5, 0.0)
    got = fn.expected(oracle, img, flow, filt, bf16)

    def by_hand(c, y, x, t):
        fx, fy = (float(v) for v in flow[0, :, y, x])
        ix, iy = int(x + fx), int(y + fy)
        a, b = x + fx - ix, y + fy - iy
        q = [0.0] * 4
        for r in range(4):
            for k in range(4):
                v = float(img[0, c, min(max(iy - 1 + r, 0), h - 1), min(max(ix - 1 + k, 0), w - 1)])
                q[2 * (r >= 2) + (k >= 2)] += v * float(t[4 * r + k])
        return (1 - a) * (1 - b) * q[0] + a * (1 - b) * q[1] + (1 - a) * b * q[2] + a * b * q[3]
    for c in range(2):
        for (y, x, t) in ((2, 3, taps), (0, 0, taps[::-1])):
            want = by_hand(c, y, x, t)
            want = float(fn.to_bf16(np.array([want], f32))[0]) if bf16 else want
            assert float(got[0, c, y, x]) == want, (c, y, x, float(got[0, c, y, x]), want)
        assert got[0, c, 4, 1] == img[0, c, 4, 1]               # x2 = -0.5 < 0: copied through
    # every other pixel has zero flow and zero taps: a valid pixel whose sums are +0
    rest = np.ones((h, w), bool)
    rest[2, 3] = rest[0, 0] = rest[4, 1] = False
    assert not got[0][:, rest].any()
    bits = fn.raw_bits(got, bf16)
    assert bits.dtype == (np.uint16 if bf16 else np.uint32) and not fn.same_raw_bits(bits, bits.copy())
    other = bits.copy()
    other[0, 0, 0, 0] ^= 1
    assert "1 of" in fn.same_raw_bits(other, bits)
