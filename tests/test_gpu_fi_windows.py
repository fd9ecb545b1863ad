"""GPU suite (`-m gpu`): every per-tile window class of the LDS-staged FilterInterpolation forward kernels, on fields
built by tests/fi_windows.py so that each class owns tiles of both batch items (the host mirror says which tile took
which class).  Results are compared with the CPU oracle at fmad=1 and with the kernels' own direct / general paths, per
class as well as on the whole frame, so a failure names the ring geometry it happened in.  Outputs go into interior
views of NaN-filled buffers: every element of the view is written, nothing outside it changes."""
import numpy as np
import pytest

from tests import fi_windows as fw

pytestmark = pytest.mark.gpu

f32 = np.float32
CHANNELS = [1, 2, 3, 4, 5, 6, 9]            # on and around each rung's in-flight depth D, ring slots R and R + 1
F16_TOL = 2e-3                              # test_filterinterp_f16_storage's rule


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


def gpu(torch, a):
    t = torch.empty(a.shape, dtype=torch.float32, device="cuda:0")
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


class Framed:
    """An interior view [:, :, 1:h+1, col:col+w] of a larger buffer, the rest NaN."""

    def __init__(self, torch, shape, col, dtype, data=None):
        B, C, h, w = shape
        self.col, self.h, self.w = col, h, w
        self.big = torch.full((B, C, h + 3, w + 8 + (w % 2)), float("nan"), dtype=dtype, device="cuda:0")
        self.v = self.big[:, :, 1:h + 1, col:col + w]
        if data is not None:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(data)))

    def check(self, torch, what):
        assert not torch.isnan(self.v).any(), "%s: elements of the output view left unwritten" % what
        m = torch.isnan(self.big)
        m[:, :, 1:self.h + 1, self.col:self.col + self.w] = True
        assert m.all(), "%s: %d elements written outside the output view" % (what, int((~m).sum()))

    def np(self):
        return self.v.cpu().numpy()


def compare(what, got, ref, pix, tol=None):
    """per class: how many of its pixels differ in any channel (bit for bit, or beyond tol * max(1, |ref|))"""
    g, r = got.astype(np.float64), ref.astype(np.float64)
    d = np.abs(g - r)
    bad = (d > tol * np.maximum(1.0, np.abs(r))) if tol else (got != ref)
    bad_px, d_px = bad.any(1), d.max(1)
    msgs = []
    for label in sorted(set(pix.ravel())):
        m = pix == label
        nb = int((bad_px & m).sum())
        if nb:
            msgs.append("%s %s: %d of %d pixels differ, max %.3g" % (what, label, nb, int(m.sum()), d_px[m].max()))
    assert not msgs, "\n".join(msgs)
    assert not bad.any()


def _inputs(rng, B, C, h, w, taps):
    return rng.random((B, C, h, w), dtype=f32), rng.random((B, taps, h, w), dtype=f32)


@pytest.mark.parametrize("C", CHANNELS + [196])
@pytest.mark.parametrize("layout", ["aligned", "unaligned", "aligned field, 1-column view"])
def test_lds_every_window_class(torch_mod, cabi, oracle, layout, C):
    """filterinterp_lds.hip, lean loop: 16-byte staging k16 1-3 and the 4-byte ladder, each with and without the 8-byte
    tap reads, the gather fallback and tiles without a valid pixel.  B = 2, 2 x 90 tiles (not a multiple of the XCD
    rounding: surplus workgroups leave)."""
    torch = torch_mod
    aligned_field = layout != "unaligned"
    h, w = fw.field_shape("lds", aligned_field)
    rng = np.random.default_rng(1000 + C + 7 * len(layout))
    f = fw.build_field("lds", rng, 2, h, w, aligned_field)
    img, filt = _inputs(rng, 2, C, h, w, 16)
    col = 4 if layout == "aligned" else 1
    gi = Framed(torch, img.shape, col, torch.float32, img)
    aligned = fw.aligned16(gi.v)
    assert aligned == (layout == "aligned")
    lab = fw.classes("lds", f["flow"], h, w, aligned)
    assert fw.xcd_grid(lab.size, 8) > lab.size                     # (forward_ori_lds: fi_xcd_grid<8>)
    if layout != "aligned field, 1-column view":
        assert set(fw.all_classes("lds", aligned)) <= set(lab.ravel())
    if C in (9, 196):
        cu = torch.cuda.get_device_properties(0).multi_processor_count
        cpg, groups = fw.fi_channel_split(lab.size, C, fw.split_prologue("lds"), cu)
        assert groups > 1, (cpg, groups)                             # several channel groups ...
        assert C == 9 or C % cpg != 0, (cpg, groups)                # ... at C = 196 a short last one
    flow, gk = gpu(torch, f["flow"]), gpu(torch, filt)
    out = Framed(torch, img.shape, col, torch.float32)
    assert cabi.filterinterp_forward_ori(gi.v, flow, gk, out.v) == 0
    direct = Framed(torch, img.shape, col, torch.float32)
    assert cabi.filterinterp_forward_ori(gi.v, flow, gk, direct.v, direct=True) == 0
    out.check(torch, "lds")
    direct.check(torch, "direct")
    pix = fw.pixel_labels("lds", lab, h, w)
    ref = oracle.filterinterp_ori_fwd(img, f["flow"], filt, fmad=1, nthreads=8)
    got = out.np()
    compare("lds (C=%d, %s) vs oracle" % (C, layout), got, ref, pix)
    compare("lds (C=%d, %s) vs direct" % (C, layout), got, direct.np(), pix)


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_blend_epilogue_every_window_class(torch_mod, cabi, oracle, C):
    """fi_forward_ori_lds<true>: the plain channel loop at every K, gather with blend, tiles without a valid pixel; the
    first direction goes through the lean kernel."""
    torch = torch_mod
    h, w = fw.field_shape("blend")
    rng = np.random.default_rng(2000 + C)
    f2 = fw.build_field("blend", rng, 2, h, w)
    f0 = fw.build_field("blend", rng, 2, h, w)
    lab = fw.classes("blend", f2["flow"], h, w)
    assert set(fw.all_classes("blend")) <= set(lab.ravel())
    ref0, filt0 = _inputs(rng, 2, C, h, w, 16)
    ref2, filt2 = _inputs(rng, 2, C, h, w, 16)
    w0, w2 = 0.75, 0.25
    g0 = Framed(torch, ref0.shape, 4, torch.float32, ref0)
    g2 = Framed(torch, ref2.shape, 4, torch.float32, ref2)
    outs = [Framed(torch, ref0.shape, 4, torch.float32) for _ in range(3)]
    args = (g0.v, g2.v, gpu(torch, f0["flow"]), gpu(torch, f2["flow"]), gpu(torch, filt0), gpu(torch, filt2))
    assert cabi.filterinterp_blend_forward(*args, outs[0].v, outs[1].v, outs[2].v, w0, w2) == 0
    for o, name in zip(outs, ("blend", "out0", "out2")):
        o.check(torch, name)
    r_blend, r0, r2 = oracle.filterinterp_blend(ref0, ref2, f0["flow"], f2["flow"], filt0, filt2, w0, w2, fmad=1)
    pix = fw.pixel_labels("blend", lab, h, w)
    compare("blend (C=%d) out2" % C, outs[2].np(), r2, pix)
    compare("blend (C=%d) blend" % C, outs[0].np(), r_blend, pix)
    lab0 = fw.classes("lds", f0["flow"], h, w, fw.aligned16(g0.v))
    compare("blend (C=%d) out0" % C, outs[1].np(), r0, fw.pixel_labels("lds", lab0, h, w))
    direct = Framed(torch, ref2.shape, 4, torch.float32)
    assert cabi.filterinterp_forward_ori(g2.v, args[3], args[5], direct.v, direct=True) == 0
    compare("blend (C=%d) out2 vs direct" % C, outs[2].np(), direct.np(), pix)


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("fs", [2, 5, 6])
def test_lds_n_every_window_class(torch_mod, cabi, oracle, fs, C):
    torch = torch_mod
    h, w = fw.field_shape("n")
    rng = np.random.default_rng(3000 + 10 * fs + C)
    f = fw.build_field("n", rng, 2, h, w, fs=fs)
    lab = fw.classes("n", f["flow"], h, w, fs=fs)
    assert set(fw.all_classes("n")) <= set(lab.ravel())
    img, filt = _inputs(rng, 2, C, h, w, fs * fs)
    gi = Framed(torch, img.shape, 3, torch.float32, img)
    flow, gk = gpu(torch, f["flow"]), gpu(torch, filt)
    out, direct = Framed(torch, img.shape, 3, torch.float32), Framed(torch, img.shape, 3, torch.float32)
    assert cabi.filterinterp_forward_ori(gi.v, flow, gk, out.v) == 0
    assert cabi.filterinterp_forward_ori(gi.v, flow, gk, direct.v, direct=True) == 0
    out.check(torch, "lds_n")
    pix = fw.pixel_labels("n", lab, h, w, fs)
    compare("lds_n fs=%d (C=%d) vs oracle" % (fs, C), out.np(), oracle.filterinterp_ori_fwd(img, f["flow"], filt, fmad=1), pix)
    compare("lds_n fs=%d (C=%d) vs direct" % (fs, C), out.np(), direct.np(), pix)


@pytest.mark.parametrize("C", CHANNELS)
def test_f16_every_window_class(torch_mod, cabi, oracle, C):
    """fp16 storage: the staged kernel within F16_TOL of the oracle, the direct kernel bit for bit; an odd frame width
    inside rows of even stride (the last dword of a window row reaches one column past the frame)."""
    torch = torch_mod
    h, w = fw.field_shape("f16")
    rng = np.random.default_rng(4000 + C)
    f = fw.build_field("f16", rng, 2, h, w)
    lab = fw.classes("f16", f["flow"], h, w)
    assert fw.xcd_grid(lab.size) > lab.size
    assert set(fw.all_classes("f16")) <= set(lab.ravel())
    img = rng.random((2, C, h, w), dtype=f32).astype(np.float16)
    filt = (rng.random((2, 16, h, w), dtype=f32) * f32(0.25)).astype(f32)
    gi = Framed(torch, img.shape, 2, torch.float16, img)
    assert gi.v.stride(2) % 2 == 0 and gi.v.data_ptr() % 4 == 0          # the staged kernel's dword layout
    flow, gk = gpu(torch, f["flow"]), gpu(torch, filt)
    out, direct = Framed(torch, img.shape, 2, torch.float16), Framed(torch, img.shape, 2, torch.float16)
    assert cabi.filterinterp_forward_ori_f16(gi.v, flow, gk, out.v) == 0
    assert cabi.filterinterp_forward_ori_f16(gi.v, flow, gk, direct.v, direct=True) == 0
    out.check(torch, "f16")
    direct.check(torch, "f16 direct")
    ref = oracle.filterinterp_ori_fwd_f16(img, f["flow"], filt, fmad=1)
    pix = fw.pixel_labels("f16", lab, h, w)
    compare("f16 (C=%d) vs oracle" % C, out.np(), ref, pix, tol=F16_TOL)
    compare("f16 direct (C=%d) vs oracle" % C, direct.np(), ref, pix)


@pytest.mark.parametrize("C", CHANNELS + [196])
def test_multi_every_window_class(torch_mod, cabi, oracle, C):
    """filterinterp_multi.hip: the union box of two flows lands in every paired class (S, KR) and every plain K; tiles
    where one flow alone would be paired but the union is plain.  Both outputs equal the single-flow op and the oracle."""
    torch = torch_mod
    h, w = fw.field_shape("multi")
    rng = np.random.default_rng(5000 + C)
    f = fw.build_field("multi", rng, 2, h, w)
    lab = fw.classes("multi", f["flow"], h, w, flow2=f["flow2"])
    assert fw.xcd_grid(lab.size) > lab.size
    assert set(fw.all_classes("multi")) <= set(lab.ravel())
    alone = fw.classes("multi", f["flow"], h, w, flow2=f["flow"])
    assert (np.char.startswith(lab.astype(str), "plain") & np.char.startswith(alone.astype(str), "paired")).any()
    img, filt = _inputs(rng, 2, C, h, w, 16)
    gi = Framed(torch, img.shape, 4, torch.float32, img)
    flows = [gpu(torch, f["flow"]), gpu(torch, f["flow2"])]
    gk = gpu(torch, filt)
    outs = [Framed(torch, img.shape, 4, torch.float32) for _ in range(2)]
    assert cabi.filterinterp_forward_ori_multi(gi.v, flows, gk, [o.v for o in outs]) == 0
    pix = fw.pixel_labels("multi", lab, h, w)
    for t, (o, fl) in enumerate(zip(outs, (f["flow"], f["flow2"]))):
        o.check(torch, "multi out %d" % t)
        single = Framed(torch, img.shape, 4, torch.float32)
        assert cabi.filterinterp_forward_ori(gi.v, flows[t], gk, single.v) == 0
        compare("multi flow %d (C=%d) vs oracle" % (t, C), o.np(), oracle.filterinterp_ori_fwd(img, fl, filt, fmad=1, nthreads=8), pix)
        compare("multi flow %d (C=%d) vs single-flow op" % (t, C), o.np(), single.np(), pix)


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("fs", [4, 6])
def test_defor_every_window_class(torch_mod, cabi, oracle, fs, variant, C):
    """filterinterp_defor_lds.hip: learned offsets stretch the corner box into every rung and past it; corners clamped
    at -1 and at h - 1 / w - 1 on all four sides."""
    torch = torch_mod
    h, w = fw.field_shape("defor")
    rng = np.random.default_rng(6000 + 100 * fs + 10 * variant + C)
    f = fw.build_field("defor", rng, 2, h, w, fs=fs)
    lab = fw.classes("defor", f["flow"], h, w, fs=fs, off=f["off"])
    assert set(fw.all_classes("defor")) <= set(lab.ravel())
    x0, y0, x1, y1, anyv = fw.tile_boxes("defor", f["flow"], h, w, fs, off=f["off"])
    assert (x0[anyv] == -1).any() and (y0[anyv] == -1).any() and (x1[anyv] == w).any() and (y1[anyv] == h).any()
    img, filt = _inputs(rng, 2, C, h, w, fs * fs)
    off = f["off"]
    gi = Framed(torch, img.shape, 3, torch.float32, img)
    flow = gpu(torch, f["flow"])
    third, fourth = (gpu(torch, off), None) if variant == 2 else (gpu(torch, filt), gpu(torch, off))
    out, general = Framed(torch, img.shape, 3, torch.float32), Framed(torch, img.shape, 3, torch.float32)
    assert cabi.filterinterp_forward_defor(variant, gi.v, flow, third, fourth, out.v) == 0
    assert cabi.filterinterp_forward_defor(variant, gi.v, flow, third, fourth, general.v, general=True) == 0
    out.check(torch, "defor")
    pix = fw.pixel_labels("defor", lab, h, w, fs)
    ref = oracle.filterinterp_defor_fwd(variant, img, f["flow"], filt, off, fmad=1)
    compare("defor fs=%d v%d (C=%d) vs oracle" % (fs, variant, C), out.np(), ref, pix)
    compare("defor fs=%d v%d (C=%d) vs general" % (fs, variant, C), out.np(), general.np(), pix)
