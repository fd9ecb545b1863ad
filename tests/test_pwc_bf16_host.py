"""CPU checks of the bfloat16 PWC-Net block (vfi_pwc_warp_forward_bf16 / _backward_bf16, vfi_correlation_lrelu_forward_bf16 /
_backward_bf16; cabi's dtype dispatch; fused.warp_corr / warp_corr_lrelu / _Warp / _CorrLrelu on bfloat16):

  * the header declares the four entries, the library exports them, cabi's table matches the header; argument errors
    return before any launch;
  * with the library stubbed, cabi sends bfloat16 tensors to the `_bf16` entries and float32 ones to the old entries, takes
    both flow dtypes, keeps today's message for float16, and refuses a bfloat16 / float32 mix and CPU tensors before any call;
  * with the launches stubbed, fused._Warp and fused._CorrLrelu allocate and return the right dtypes, and out= is refused in
    grad mode for bfloat16 too; fused.warp and fused.corr_lrelu keep refusing bfloat16, as the existing suite requires
    (tests/test_gpu_corr_bf16.py), before any launch;
  * the helper's statement of the two-rounding LeakyReLU and of the masked gradient equals torch's CPU bfloat16 leaky_relu,
    forward and autograd, bit for bit;
  * the new kernels' gfx950 assembly has no scratch and rounds with the convert instruction.
"""
import contextlib
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from tests import pwc_bf16 as pb
from tests.test_abi_and_host import built  # noqa: F401  (fixture)
from tests.test_corr_bf16_host import _FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video-frame-interpolation-based-on-deformable-kernel-region_amd")
ENTRIES = ("vfi_pwc_warp_forward_bf16", "vfi_pwc_warp_backward_bf16", "vfi_correlation_lrelu_forward_bf16",
           "vfi_correlation_lrelu_backward_bf16")
PWC = (4, 1, 4, 1, 1)


# ------------------------------------------------------------------ 1. symbols and table

def _params(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vfi_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "the header does not declare %s" % name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", ENTRIES)
def test_header_library_and_ctypes_table_agree(built, name):  # noqa: F811
    from vfidkr_amd import cabi
    want = []
    for p in _params(name):
        if "*" in p or p.startswith("vfi_stream_t"):
            want.append(ctypes.c_void_p)
        elif p.startswith("vfi_strides"):
            want.append(cabi.Strides)
        elif p.startswith("int64_t"):
            want.append(ctypes.c_int64)
        elif p.startswith("float"):
            want.append(ctypes.c_float)
        else:
            assert re.fullmatch(r"int \w+", p), p
            want.append(ctypes.c_int)
    assert cabi.SIGNATURES[name] == want
    assert hasattr(ctypes.CDLL(built.LIB_PATH), name)
    fn = getattr(cabi.lib(), name)
    assert fn.argtypes == want and fn.restype is ctypes.c_int


def test_the_bf16_entries_are_the_float32_entries_plus_the_flow_flag():
    drop = lambda ps: [re.sub(r"\b(const )?(float|void)\*", "ptr", p) for p in ps]      # noqa: E731
    for which in ("forward", "backward"):
        f32, bf = _params("vfi_pwc_warp_%s" % which), _params("vfi_pwc_warp_%s_bf16" % which)
        assert bf[2] == "int flow_is_bf16" and drop(bf[:2] + bf[3:]) == drop(f32)
        assert drop(_params("vfi_correlation_lrelu_%s_bf16" % which)) == drop(_params("vfi_correlation_lrelu_%s" % which))
    text = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "pwc_warp_bf16.hip" in re.search(r"^SRCS\s*:=\s*(.*)$", text, flags=re.M).group(1).split()


def test_argument_errors_return_before_any_launch(built):  # noqa: F811
    from vfidkr_amd import cabi
    lib, E = cabi.lib(), cabi.VFI_ERR_SHAPE
    p = ctypes.c_void_p(4096)           # never dereferenced
    st = cabi.Strides(64, 64, 8)
    wf = lambda x=p, f=p, o=p, b=1, c=1, h=8, w=8: lib.vfi_pwc_warp_forward_bf16(x, f, 1, o, b, c, h, w, 1, st, st, st, None)      # noqa: E731
    wb = lambda x=p, f=p, g=p, gx=p, gf=p, b=1, w=8: lib.vfi_pwc_warp_backward_bf16(x, f, 0, g, gx, gf, b, 1, 8, w, 1, st, st, st, st, st, None)  # noqa: E731
    assert wf(x=None) == E and wf(f=None) == E and wf(o=None) == E and wf(b=0) == E and wf(c=0) == E and wf(h=0) == E and wf(w=0) == E
    assert wf(b=65536) == E                                                             # batch x channel chunks beyond a grid's z
    assert wb(x=None) == E and wb(f=None) == E and wb(g=None) == E and wb(b=0) == E and wb(w=0) == E and wb(b=65536) == E
    assert wb(gx=None, gf=None) == cabi.VFI_OK                                          # nothing requested
    img = 81 * 8 * 8
    cf = lambda slope=0.1, stride=img, out=p, b=1: lib.vfi_correlation_lrelu_forward_bf16(p, p, out, stride, b, 2, 8, 8, 4, 1, 4, 1, 1, slope, None)  # noqa: E731
    cbw = lambda slope=0.1, ys=img, gs=img, y=p, g1=p, s1=1: lib.vfi_correlation_lrelu_backward_bf16(  # noqa: E731
        p, p, y, ys, p, gs, g1, p, 1, 2, 8, 8, 4, 1, 4, s1, 1, slope, None)
    for bad in (0.0, -0.1, float("inf"), float("-inf"), float("nan")):
        assert cf(slope=bad) == E and cbw(slope=bad) == E, bad
    assert cf(stride=img - 1) == E and cf(stride=0) == E and cbw(ys=img - 1) == E and cbw(gs=-img) == E
    assert cf(out=None) == E and cf(b=0) == E and cbw(y=None) == E and cbw(g1=None) == E and cbw(s1=2) == E


# ------------------------------------------------------------------ 2. cabi's dispatch, library stubbed

class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "vfi_correlation_output_dims":
                args[7]._obj.value, args[8]._obj.value, args[9]._obj.value = 81, args[0], args[1]
            return 0
        return fn


@pytest.fixture
def stubbed(monkeypatch):
    """cabi with the library, the device context and the stream stubbed; tensors are CPU tensors that say they are on the GPU"""
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi
    rec = _Recorder()
    monkeypatch.setattr(cabi, "lib", lambda: rec)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(torch, "empty", lambda *a, **k: _FakeCuda(torch.zeros(*a, dtype=k.get("dtype"))))
    monkeypatch.setattr(torch, "empty_like", lambda t, **k: _FakeCuda(torch.zeros(t.shape, dtype=t.dtype)))
    monkeypatch.setattr(torch, "zeros_like", lambda t, **k: _FakeCuda(torch.zeros(t.shape, dtype=t.dtype)))
    launches = lambda: [n for n, _ in rec.calls if n != "vfi_correlation_output_dims"]      # noqa: E731
    return cabi, rec, launches


def _t(dtype, *shape, cuda=True):
    return _FakeCuda(torch.zeros(*shape, dtype=dtype), cuda)


BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16


def test_cabi_sends_each_dtype_to_its_entries(stubbed):
    cabi, rec, launches = stubbed
    for dt, suffix in ((BF, "_bf16"), (F32, "")):
        for fdt in ((BF, F32) if dt == BF else (F32,)):
            del rec.calls[:]
            x, g, gx, out = (_t(dt, 2, 3, 6, 10) for _ in range(4))
            flo, gf = _t(fdt, 2, 2, 6, 10), _t(fdt, 2, 2, 6, 10)
            assert cabi.pwc_warp_forward(x, flo, out) == 0
            assert cabi.pwc_warp_backward(x, flo, g, gx, gf) == 0
            assert cabi.pwc_warp_backward(x, flo, g, None, gf) == 0 and cabi.pwc_warp_backward(x, flo, g, gx, None) == 0
            assert launches() == ["vfi_pwc_warp_forward" + suffix] + ["vfi_pwc_warp_backward" + suffix] * 3
            if suffix:                                                                  # the flow's dtype travels as the flag
                assert [a[2] for n, a in rec.calls] == [int(fdt == BF)] * 4
        del rec.calls[:]
        a, b = _t(dt, 2, 4, 6, 10), _t(dt, 2, 4, 6, 10)
        y = cabi.correlation_lrelu_forward(a, b, *PWC, 0.1)
        assert y.dtype == dt and tuple(y.shape) == (2, 81, 6, 10)
        wide = _t(dt, 2, 90, 6, 10)
        dst = _FakeCuda(wide.t[:, 3:84])
        assert cabi.correlation_lrelu_forward(a, b, *PWC, 0.1, out=dst) is dst
        g1, g2 = cabi.correlation_lrelu_backward(a, b, y, _t(dt, 2, 81, 6, 10), *PWC, 0.1)
        assert g1.dtype == dt and g2.dtype == dt
        assert launches() == ["vfi_correlation_lrelu_forward" + suffix] * 2 + ["vfi_correlation_lrelu_backward" + suffix]
        strides = [a[3] for n, a in rec.calls if n.startswith("vfi_correlation_lrelu_forward")]
        assert strides == [81 * 60, 90 * 60]                                            # the slice's batch stride, in elements


def test_cabi_refusals_launch_nothing(stubbed):
    cabi, rec, launches = stubbed
    x, g, flo = _t(BF, 2, 3, 6, 10), _t(BF, 2, 3, 6, 10), _t(F32, 2, 2, 6, 10)
    bfl = _t(BF, 2, 2, 6, 10)
    mixed = (lambda: cabi.pwc_warp_forward(x, flo, _t(F32, 2, 3, 6, 10)),
             lambda: cabi.pwc_warp_backward(x, flo, _t(F32, 2, 3, 6, 10), g, None),       # bfloat16 x, float32 grad_output
             lambda: cabi.pwc_warp_backward(x, flo, g, _t(F32, 2, 3, 6, 10), None),
             lambda: cabi.pwc_warp_backward(x, flo, g, g, bfl),                           # grad_flow has the flow's dtype
             lambda: cabi.correlation_lrelu_forward(x, _t(F32, 2, 3, 6, 10), *PWC, 0.1),
             lambda: cabi.correlation_lrelu_forward(x, x, *PWC, 0.1, out=_t(F32, 2, 81, 6, 10)),
             lambda: cabi.correlation_lrelu_backward(x, x, _t(BF, 2, 81, 6, 10), _t(F32, 2, 81, 6, 10), *PWC, 0.1),
             lambda: cabi.correlation_lrelu_backward(x, x, _t(F32, 2, 81, 6, 10), _t(BF, 2, 81, 6, 10), *PWC, 0.1))
    for call in mixed:
        with pytest.raises(RuntimeError, match="tensors must be (bfloat16|float32)"):
            call()
    # float16 anywhere, a bfloat16 tensor behind a float32 first one, a bfloat16 flow with float32 features: today's message
    h = _t(F16, 2, 3, 6, 10)
    f = _t(F32, 2, 3, 6, 10)
    for call in (lambda: cabi.pwc_warp_forward(h, flo, h), lambda: cabi.pwc_warp_backward(h, flo, h, h, None),
                 lambda: cabi.pwc_warp_forward(x, _t(F16, 2, 2, 6, 10), g), lambda: cabi.pwc_warp_forward(f, bfl, f),
                 lambda: cabi.pwc_warp_forward(f, flo, x), lambda: cabi.pwc_warp_backward(f, flo, g, f, None),
                 lambda: cabi.correlation_lrelu_forward(h, h, *PWC, 0.1), lambda: cabi.correlation_lrelu_forward(f, x, *PWC, 0.1),
                 lambda: cabi.correlation_lrelu_backward(h, h, _t(F16, 2, 81, 6, 10), _t(F16, 2, 81, 6, 10), *PWC, 0.1)):
        with pytest.raises(RuntimeError, match="tensors must be float32"):
            call()
    cx, cf = _t(BF, 2, 3, 6, 10, cuda=False), _t(F32, 2, 2, 6, 10, cuda=False)
    for call in (lambda: cabi.pwc_warp_forward(cx, flo, g), lambda: cabi.pwc_warp_forward(x, cf, g), lambda: cabi.pwc_warp_forward(x, flo, cx),
                 lambda: cabi.pwc_warp_backward(x, flo, cx, g, None), lambda: cabi.correlation_lrelu_forward(cx, cx, *PWC, 0.1),
                 lambda: cabi.correlation_lrelu_backward(x, x, _t(BF, 2, 81, 6, 10), _t(BF, 2, 81, 6, 10, cuda=False), *PWC, 0.1)):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call()
    assert launches() == []


# ------------------------------------------------------------------ 3. the autograd Functions, launches stubbed

def test_fused_functions_allocate_and_return_the_right_dtypes(monkeypatch):
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi, fused
    seen = []

    def warp_fwd(x, flo, out, ac):
        seen.append(("wf", x.dtype, flo.dtype, out.dtype))
        return 0

    def warp_bwd(x, flo, g, gx, gf, ac):
        seen.append(("wb", g.dtype, None if gx is None else (gx.dtype, bool(torch.isnan(gx).all()) if gx.dtype == BF else float(gx.abs().sum())),
                     None if gf is None else gf.dtype))
        for t in (gx, gf):
            if t is not None:
                t.zero_()
        return 0

    def lrelu_fwd(c1, c2, *cfg, out=None):
        seen.append(("cf", c1.dtype, c2.dtype, None if out is None else out.dtype))
        return torch.ones(c1.size(0), 81, c1.size(2), c1.size(3), dtype=c1.dtype) if out is None else out

    def lrelu_bwd(c1, c2, y, g, *cfg):
        seen.append(("cb", y.dtype, g.dtype))
        return torch.zeros_like(c1), torch.zeros_like(c2)

    monkeypatch.setattr(cabi, "pwc_warp_forward", warp_fwd)
    monkeypatch.setattr(cabi, "pwc_warp_backward", warp_bwd)
    monkeypatch.setattr(cabi, "correlation_lrelu_forward", lrelu_fwd)
    monkeypatch.setattr(cabi, "correlation_lrelu_backward", lrelu_bwd)
    # (empty_like hands the bfloat16 grad_x over unwritten: NaN-fill it so the stub can tell empty_like from zeros_like)
    real_empty_like = torch.empty_like
    monkeypatch.setattr(torch, "empty_like", lambda t, **k: real_empty_like(t, **k).fill_(float("nan")) if t.dtype == BF else real_empty_like(t, **k))
    for dt in (BF, F32):
        for fdt in ((BF, F32) if dt == BF else (F32,)):
            del seen[:]
            c1 = torch.randn(2, 4, 6, 10).to(dt).requires_grad_(True)
            c2 = torch.randn(2, 4, 6, 10).to(dt).requires_grad_(True)
            flo = torch.randn(2, 2, 6, 10).to(fdt).requires_grad_(True)
            out = fused.warp_corr_lrelu(c1, c2, flo)
            assert out.dtype == dt and out.grad_fn is not None
            out.sum().backward()
            assert c1.grad.dtype == dt and c2.grad.dtype == dt and flo.grad.dtype == fdt
            # bfloat16: grad_x comes from empty_like (written by the kernel); float32: from zeros_like (added into)
            assert seen == [("wf", dt, fdt, dt), ("cf", dt, dt, None), ("cb", dt, dt), ("wb", dt, (dt, True if dt == BF else 0.0), fdt)]
            with pytest.raises(RuntimeError, match="out= is for inference"):
                fused.warp_corr_lrelu(c1, c2, flo, out=torch.zeros(2, 81, 6, 10, dtype=dt))
            # the two functions the existing suite pins to float32 stay there; the Functions behind them take bfloat16
            del seen[:]
            if dt == BF:
                for call in (lambda: fused.warp(c2, flo), lambda: fused.warp(c2.detach(), flo.detach()),
                             lambda: fused.corr_lrelu(c1, c2), lambda: fused.corr_lrelu(c1.detach(), c2.detach())):
                    with pytest.raises(RuntimeError, match="must be float32"):
                        call()
                assert seen == []
            else:
                w = fused.warp(c2.detach(), flo.detach())
                assert w.dtype == dt and w.grad_fn is None
                with pytest.raises(RuntimeError, match="out= is for inference"):
                    fused.corr_lrelu(c1, c2, out=torch.zeros(2, 81, 6, 10, dtype=dt))
            w = fused._Warp.apply(c2, flo, True)
            y = fused._CorrLrelu.apply(c1, c2, 0.1)
            assert w.dtype == dt and w.grad_fn is not None and y.dtype == dt and y.grad_fn is not None
            with torch.no_grad():
                dst = torch.zeros(2, 90, 6, 10, dtype=dt)[:, 2:83]
                assert fused.warp_corr_lrelu(c1, c2, flo, out=dst) is dst
    # warp_corr(one_launch=True) on bfloat16: the two-launch path
    monkeypatch.setattr(cabi, "pwc_warp_correlation_forward", lambda *a: pytest.fail("the one-launch kernel is float32 only"))
    monkeypatch.setattr(cabi, "correlation_forward", lambda a, b, *cfg: ("corr", a.dtype, b.dtype))
    with torch.no_grad():
        assert fused.warp_corr(torch.zeros(1, 4, 6, 10, dtype=BF), torch.zeros(1, 4, 6, 10, dtype=BF), torch.zeros(1, 2, 6, 10),
                               one_launch=True) == ("corr", BF, BF)


# ------------------------------------------------------------------ 4. the helper's LeakyReLU is torch's, bit for bit

@pytest.mark.parametrize("slope", [0.1, 0.5, 0.01, 3.0])
def test_two_rounding_lrelu_and_masked_gradient_equal_torch_cpu_bf16(slope):
    grid = pb.edge_grid()
    assert np.isnan(grid).any() and np.isinf(grid).any() and (grid == 0).sum() >= 2 and (np.abs(grid[np.isfinite(grid) & (grid != 0)]).min() < 1e-40)
    # forward: the stored cost volume is bfloat16 already (the first rounding), torch activates and rounds again
    t = torch.from_numpy(grid).to(BF)
    want = torch.nn.functional.leaky_relu(t, slope)
    msg = pb.same_bits(pb.bits(pb.lrelu_two_roundings(grid, slope)), want.view(torch.int16).numpy().view(np.uint16))
    assert not msg, msg
    # from a float32 mean: the first rounding is the helper's own
    rng = np.random.default_rng(5)
    mean = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 1e-3, np.array([1e-41, -1e-41, 2.0 ** -134, -2.0 ** -134], np.float32)])
    want = torch.nn.functional.leaky_relu(torch.from_numpy(mean).to(BF), slope)
    msg = pb.same_bits(pb.bits(pb.lrelu_two_roundings(mean, slope)), want.view(torch.int16).numpy().view(np.uint16))
    assert not msg, msg
    # backward: torch autograd through leaky_relu on bfloat16, with the mask read off the saved OUTPUT's sign
    x = t.clone().requires_grad_(True)
    y = torch.nn.functional.leaky_relu(x, slope)
    g = torch.from_numpy(np.roll(grid, 7)).to(BF)
    y.backward(g)
    got = pb.masked_gradient(g.float().numpy(), y.detach().float().numpy(), slope)
    msg = pb.same_bits(pb.bits(got), x.grad.view(torch.int16).numpy().view(np.uint16))
    assert not msg, msg
    # and torch.where(y > 0, g, g * slope) in bfloat16, the form the GPU test feeds the unactivated backward
    alt = torch.where(y.detach() > 0, g, g * slope)
    msg = pb.same_bits(pb.bits(got), alt.view(torch.int16).numpy().view(np.uint16))
    assert not msg, msg


# ------------------------------------------------------------------ 5. the assembly

def test_new_kernels_have_no_scratch_and_round_with_the_convert(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    text = open(os.path.join(PKG, "csrc", "Makefile")).read()
    flags = re.search(r"^HIPFLAGS\s*\?=\s*(.*)$", text, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    wanted = {"pwc_warp_bf16": ("pwc_warp_forward_bf16", "pwc_warp_backward_tile_bf16", "pwc_warp_flow_combine_bf16ILb1"),
              "gradacc": ("gradacc_convert_bf16",),
              "correlation_bf16": ("CorrBf16Lrelu", "CorrBf16GradLrelu")}
    for src, names in wanted.items():
        out = tmp_path / (src + ".s")
        subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(PKG, "csrc", src + ".hip"), "-o", str(out)],
                       check=True, cwd=os.path.join(PKG, "csrc"))
        kernels = re.findall(r"^(_ZN3vfi\w+):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", out.read_text(), flags=re.M | re.S)
        for name in names:
            mine = [(n, body) for n, body in kernels if name in n]
            assert mine, (name, [n for n, _ in kernels])
            for n, body in mine:
                assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), n          # no scratch, no spills
                if "pwc_warp_backward_tile_bf16ILb0" not in n:                                # (float32 flow gradient: it rounds nothing)
                    assert "v_cvt_pk_bf16_f32" in body, n                                     # round to nearest even, never a shift
