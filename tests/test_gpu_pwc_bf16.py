"""GPU: PWC-Net's warp and correlation + LeakyReLU on bfloat16 storage (vfi_pwc_warp_forward_bf16 / _backward_bf16,
vfi_correlation_lrelu_forward_bf16 / _backward_bf16, and fused.warp_corr / warp_corr_lrelu / _Warp / _CorrLrelu on top).

Every result is compared bit for bit with the composition it replaces, run on the same GPU: the float32 warp entries on
the widened tensors rounded once, F.leaky_relu on the bfloat16 cost volume, the unactivated bfloat16 correlation backward fed
a materialised masked gradient.  The warp is also compared with the CPU oracle (forward, bit for bit after the rounding) and
with the float64 restatement of torch autograd (backward: the float32 test's tolerances plus half a bfloat16 ulp for the
one rounding -- 2^-9 of the power of two above the value, tests/pwc_bf16.py: half_ulp; 2^-9 of the value itself is not
attainable by a correctly rounded result, measured worst 1.99 x 2^-9 |value| for the rounded float32 entry).  Every output lives inside a pattern-filled buffer that is checked for writes outside the tensor and
between the images and planes of a strided destination."""
import numpy as np
import pytest

from tests import pwc_bf16 as pb
from tests.corr_edges import out_dims
from tests.test_gpu_corr_bf16 import MFMA_SHAPES, backward_reference, dev
from tests.test_gpu_correlation_f16_backward import SHAPES as BACKWARD_SHAPES
from tests import corr_bf16 as cb

pytestmark = pytest.mark.gpu

PWC = cb.PWC
KINDS = ("zero", "int", "3", "border")


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


def bf(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).cuda()


def f32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def same(torch, got, want):
    """two bfloat16 (or float32) tensors: equal patterns"""
    assert got.dtype == want.dtype and got.shape == want.shape
    raw = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    return torch.equal(got.contiguous().view(raw), want.contiguous().view(raw))


# ------------------------------------------------------------------ the warp's cases

# (B, C, h, w), layout.  "odd": every tensor starts at an odd element offset of its buffer (bfloat16: 2-byte aligned only);
# "slice": x is a channel slice of a wider buffer whose rows are longer than w, and the outputs have strides of their own
WARP_CASES = [((1, 1, 1, 1), "dense"), ((3, 5, 8, 64), "dense"), ((2, 3, 9, 67), "dense"), ((1, 35, 5, 130), "dense"),
              ((2, 196, 4, 7), "dense"),           # C large on a small frame: the channels are split over workgroups, the flow combine runs
              ((2, 9, 7, 67), "odd"), ((2, 6, 9, 34), "slice")]


def layout(shape, how, what):
    """(stride or None, offset) of tensor `what` ('x', 'flow', 'out') in layout `how`"""
    B, C, h, w = shape
    if how == "odd":
        return None, 63
    if how == "slice":
        if what == "x":                                     # channels 2 .. 2 + C of a (C + 5)-channel buffer with rows of w + 3
            row, plane = w + 3, h * (w + 3) + 1
            return (plane * (C + 5), plane, row, 1), 64 + 2 * plane
        if what == "out":                                   # planes and images apart, an odd image stride
            row, plane = w + 1, h * (w + 1) + 3
            return (plane * C + 5, plane, row, 1), 64
    return None, 64


def place(torch, values, dtype, shape, how, what):
    stride, offset = layout(shape, how, what)
    buf, view = pb.guarded(torch, values.shape, dtype, stride, offset)
    pb.fill(torch, view, values)
    return buf, view


def warp_inputs(rng, shape, kind):
    B, C, h, w = shape
    x = pb.to_bf16(rng.normal(size=shape))
    g = pb.to_bf16(rng.normal(size=shape))
    flo = pb.flow_family(rng, kind, B, h, w)
    return x, flo, g


@pytest.mark.parametrize("shape,how", WARP_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_warp_forward_bits(torch_mod, cabi, oracle, shape, how):
    torch = torch_mod
    B, C, h, w = shape
    rng = np.random.default_rng([1] + list(shape))
    for kind in KINDS:
        x_np, flo32, _ = warp_inputs(rng, shape, kind)
        _, x = place(torch, x_np, torch.bfloat16, shape, how, "x")
        for fdt in (torch.float32, torch.bfloat16):
            flo_np = flo32 if fdt == torch.float32 else pb.to_bf16(flo32)
            _, flo = place(torch, flo_np, fdt, shape, how, "flow")
            if how == "odd":
                assert x.data_ptr() % 4 == 2 and (fdt == torch.float32 or flo.data_ptr() % 4 == 2)
            for ac in (True, False):
                stride, offset = layout(shape, how, "out")
                buf, out = pb.guarded(torch, shape, torch.bfloat16, stride, offset)
                assert cabi.pwc_warp_forward(x, flo, out, ac) == 0
                torch.cuda.synchronize()
                assert pb.guard_intact(torch, buf, out), (kind, fdt, ac)
                ref = torch.empty(shape, device="cuda")
                assert cabi.pwc_warp_forward(x.float().contiguous(), flo.float().contiguous(), ref, ac) == 0
                assert same(torch, out, ref.to(torch.bfloat16)), (kind, fdt, ac)
                want = pb.bits(oracle.pwc_warp(x_np, flo_np, ac, fmad=1))
                msg = pb.same_bits(pb.tensor_bits(torch, out), want)
                assert not msg, (kind, fdt, ac, msg)


def run_backward(torch, cabi, shape, how, x, flo, g, ac, want_x, want_f):
    """the bfloat16 entry into NaN-prefilled guarded gradients; returns (grad_x, grad_flow) after the guard check"""
    stride, offset = layout(shape, how, "out")
    gx = gf = bx = bfl = None
    if want_x:
        bx, gx = pb.guarded(torch, shape, torch.bfloat16, stride, offset)
        gx.fill_(float("nan"))                              # written in full: no NaN survives
    if want_f:
        bfl, gf = pb.guarded(torch, flo.shape, flo.dtype, None, 63 if how == "odd" else 64)
        gf.fill_(float("nan"))
    assert cabi.pwc_warp_backward(x, flo, g, gx, gf, ac) == 0
    torch.cuda.synchronize()
    assert (bx is None or pb.guard_intact(torch, bx, gx)) and (bfl is None or pb.guard_intact(torch, bfl, gf))
    return gx, gf


def reference_backward(torch, cabi, x, flo, g, ac):
    """the float32 entry on the widened tensors: (grad_x, grad_flow), float32"""
    xf, ff, gf32 = x.float().contiguous(), flo.float().contiguous(), g.float().contiguous()
    rx, rf = torch.zeros_like(xf), torch.empty_like(ff)
    assert cabi.pwc_warp_backward(xf, ff, gf32, rx, rf, ac) == 0
    return rx, rf


@pytest.mark.parametrize("shape,how", WARP_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_warp_backward_bits_tolerance_and_repeat(torch_mod, cabi, shape, how):
    torch = torch_mod
    rng = np.random.default_rng([2] + list(shape))
    worst = 0.0
    for kind in KINDS:
        x_np, flo32, g_np = warp_inputs(rng, shape, kind)
        _, x = place(torch, x_np, torch.bfloat16, shape, how, "x")
        _, g = place(torch, g_np, torch.bfloat16, shape, how, "x")
        for fdt in (torch.float32, torch.bfloat16):
            flo_np = flo32 if fdt == torch.float32 else pb.to_bf16(flo32)
            _, flo = place(torch, flo_np, fdt, shape, how, "flow")
            for ac in (True, False):
                rx, rf = reference_backward(torch, cabi, x, flo, g, ac)
                want_x, want_f = rx.to(torch.bfloat16), rf.to(fdt)
                gx, gf = run_backward(torch, cabi, shape, how, x, flo, g, ac, True, True)
                assert same(torch, gx, want_x) and same(torch, gf, want_f), (kind, fdt, ac)
                gx2, gf2 = run_backward(torch, cabi, shape, how, x, flo, g, ac, True, True)
                assert same(torch, gx, gx2) and same(torch, gf, gf2), "two runs differ"
                only_x, none = run_backward(torch, cabi, shape, how, x, flo, g, ac, True, False)
                none2, only_f = run_backward(torch, cabi, shape, how, x, flo, g, ac, False, True)
                assert none is None and none2 is None and same(torch, only_x, want_x) and same(torch, only_f, want_f)
                ref = pb.pwc_warp_bwd(x_np, flo_np, g_np, ac)
                worst = max(worst, pb.bf16_within(gx.float().cpu().numpy().astype(np.float64), gf.float().cpu().numpy().astype(np.float64),
                                                  ref, g_np, flow_bf16=fdt == torch.bfloat16))
    print("grad_x: worst error in units of 2^-9 |reference|: %.3f" % worst)


def test_the_channel_split_case_splits(cabi):
    """(2, 196, 4, 7) above has one tile per image: the float32 entry's group rule gives it more than one channel group on any
    device with more than two compute units, so the partial sums and the combine kernel run there."""
    tiles, c8 = 1 * 1 * 2, (196 + 7) // 8
    for cus in (64, 256, 304):
        assert min(c8, max(1, (cus + tiles - 1) // tiles)) > 1


# the four warped levels of the 1080p pyramid and of the Vimeo training shape (tests/test_gpu_pwc_warp_backward.py)
LEVELS = [(1, 32, 288, 496), (1, 64, 144, 248), (1, 96, 72, 124), (1, 128, 36, 62),
          (3, 32, 64, 112), (3, 64, 32, 56), (3, 96, 16, 28), (3, 128, 8, 14)]


@pytest.mark.parametrize("lv", LEVELS, ids=lambda v: "B%dC%d_%dx%d" % v)
def test_pyramid_levels_equal_the_rounded_float32_entries(torch_mod, cabi, lv):
    torch = torch_mod
    gen = torch.Generator(device="cuda").manual_seed(lv[1] * lv[2])
    x = torch.randn(lv, device="cuda", generator=gen).bfloat16()
    g = torch.randn(lv, device="cuda", generator=gen).bfloat16()
    flo = (torch.randn((lv[0], 2, lv[2], lv[3]), device="cuda", generator=gen) * 3).bfloat16()
    out = torch.empty_like(x)
    assert cabi.pwc_warp_forward(x, flo, out, True) == 0
    ref = torch.empty(lv, device="cuda")
    assert cabi.pwc_warp_forward(x.float(), flo.float(), ref, True) == 0
    assert same(torch, out, ref.bfloat16())
    gx, gf = torch.full_like(x, float("nan")), torch.full_like(flo, float("nan"))
    assert cabi.pwc_warp_backward(x, flo, g, gx, gf, True) == 0
    rx, rf = reference_backward(torch, cabi, x, flo, g, True)
    assert same(torch, gx, rx.bfloat16()) and same(torch, gf, rf.bfloat16())


def test_inf_gradient_poisons_the_float32_entrys_cells(torch_mod, cabi):
    """A call the accumulator sends to fp32 atomics: NaN / Inf exactly where the float32 entry has them; the finite cells
    against float64 within the float32 test's tolerance for that path (4e-7 A + 1e-6) plus half a bfloat16 ulp."""
    torch = torch_mod
    rng = np.random.default_rng(10)
    shape = (1, 3, 17, 33)
    x_np = pb.to_bf16(rng.normal(size=shape))
    g_np = pb.to_bf16(rng.normal(size=shape))
    flo_np = pb.flow_family(rng, "dyadic", 1, 17, 33)                      # (exact in bfloat16 too: sixteenths below 4)
    g_np[0, 1, 5, 7] = np.inf
    x, g = bf(torch, x_np), bf(torch, g_np)
    for fdt in (torch.float32, torch.bfloat16):
        flo = f32(torch, flo_np).to(fdt)
        gx, gf = run_backward(torch, cabi, shape, "dense", x, flo, g, True, True, True)
        rx, rf = reference_backward(torch, cabi, x, flo, g, True)
        gxn, rxn = gx.float().cpu().numpy(), rx.cpu().numpy()
        assert np.array_equal(~np.isfinite(gxn), ~np.isfinite(rxn)) and (~np.isfinite(gxn)).sum() >= 1
        assert np.array_equal(~np.isfinite(gf.float().cpu().numpy()), ~np.isfinite(rf.cpu().numpy()))
        fin = np.isfinite(rxn)
        g64, _, A, _, _ = pb.pwc_warp_bwd(x_np, flo_np, np.where(np.isfinite(g_np), g_np, 0).astype(np.float32), True)
        assert (np.abs(gxn[fin] - g64[fin]) <= 4e-7 * A[fin] + 1e-6 + pb.half_ulp(g64[fin])).all()


# ------------------------------------------------------------------ correlation + LeakyReLU, forward

def lrelu_reference(torch, cabi, a, b, cfg, slope):
    return torch.nn.functional.leaky_relu(cabi.correlation_forward(a, b, *cfg), slope)


def both_signs(rng, shape):
    f1, f2 = pb.to_bf16(rng.standard_normal(shape) + 0.25), pb.to_bf16(rng.standard_normal(shape))
    return f1, f2


def slice_destination(torch, B, oc, oh, ow, k):
    """buf[:, k:k + oc] of a wider bfloat16 buffer whose per-image element count is ODD (consecutive images alternate between
    4-byte and 2-byte alignment), at an element offset with k's parity"""
    image = (oc + 5) * oh * ow
    image += 1 - image % 2
    off = 64 + k * oh * ow
    off += (off % 2) != (k % 2)
    return pb.guarded(torch, (B, oc, oh, ow), torch.bfloat16, (image, oh * ow, ow, 1), off, tail=64 + 5 * oh * ow)


@pytest.mark.parametrize("shape,pad,offset,guard", MFMA_SHAPES)
@pytest.mark.parametrize("slope", [0.1, 0.5])
def test_lrelu_forward_is_the_composition_dense_and_in_a_slice(torch_mod, cabi, shape, pad, offset, guard, slope):
    torch = torch_mod
    cfg = (pad, 1, 4, 1, 1)
    rng = np.random.default_rng([4] + list(shape) + [pad])
    f1, f2 = both_signs(rng, shape)
    a, b = dev(torch, f1, offset), dev(torch, f2, offset)
    want = lrelu_reference(torch, cabi, a, b, cfg, slope)
    assert (want > 0).any() and (want < 0).any() or shape[2] * shape[3] == 1
    B, (oc, oh, ow) = shape[0], out_dims(shape[2], shape[3], *cfg)
    buf, dense = pb.guarded(torch, (B, oc, oh, ow), torch.bfloat16, None, guard)
    assert cabi.correlation_lrelu_forward(a, b, *cfg, slope, out=dense) is dense
    torch.cuda.synchronize()
    assert pb.guard_intact(torch, buf, dense) and same(torch, dense, want)
    assert same(torch, cabi.correlation_lrelu_forward(a, b, *cfg, slope), want)
    for k in (2, 3):
        buf, dst = slice_destination(torch, B, oc, oh, ow, k)
        assert dst.data_ptr() % 4 == 2 * (k % 2) and (B == 1 or dst.stride(0) % 2 == 1)
        cabi.correlation_lrelu_forward(a, b, *cfg, slope, out=dst)
        torch.cuda.synchronize()
        assert pb.guard_intact(torch, buf, dst), "the rest of the buffer changed"
        assert same(torch, dst, want), k


def test_lrelu_forward_reaches_both_kernels():
    reached = {cb.selected_kernel(*s, (pad, 1, 4, 1, 1)) for s, pad, _, _ in MFMA_SHAPES}
    assert reached == {"mfma", "generic"}


def test_lrelu_forward_generic_configuration(torch_mod, cabi):
    torch = torch_mod
    shape, cfg = (2, 3, 8, 8), (4, 3, 4, 1, 2)
    rng = np.random.default_rng(6)
    f1, f2 = both_signs(rng, shape)
    a, b = bf(torch, f1), bf(torch, f2)
    want = lrelu_reference(torch, cabi, a, b, cfg, 0.1)
    oc, oh, ow = out_dims(8, 8, *cfg)
    for k in (2, 3):
        buf, dst = slice_destination(torch, 2, oc, oh, ow, k)
        cabi.correlation_lrelu_forward(a, b, *cfg, 0.1, out=dst)
        torch.cuda.synchronize()
        assert pb.guard_intact(torch, buf, dst) and same(torch, dst, want)


@pytest.mark.parametrize("shape", [(1, 5, 11, 20), (1, 5, 66, 64)])
def test_lrelu_forward_non_finite_inputs_both_kernels(torch_mod, cabi, shape):
    """+inf inside x1, -inf in x2, a NaN, and an inf of x1 at the border whose padding taps give inf * 0 = NaN: NaN where the
    composition has NaN, every other element its bits."""
    torch = torch_mod
    rng = np.random.default_rng(5)
    f1, f2 = both_signs(rng, shape)
    f1[0, 2, 5, 10] = np.inf
    f2[0, 1, 6, 14] = -np.inf
    f1[0, 0, 3, 16] = np.nan
    f1[0, 4, 0, 0] = np.inf
    assert cb.selected_kernel(*shape) == ("generic" if shape[2] == 11 else "mfma")
    a, b = bf(torch, f1), bf(torch, f2)
    want = lrelu_reference(torch, cabi, a, b, PWC, 0.1)
    got = cabi.correlation_lrelu_forward(a, b, *PWC, 0.1)
    assert torch.isnan(want).any() and torch.isinf(want).any() and not torch.isnan(want).all()
    msg = pb.same_bits(pb.tensor_bits(torch, got), pb.tensor_bits(torch, want))
    assert not msg, msg


# ------------------------------------------------------------------ correlation + LeakyReLU, backward

def lrelu_backward_check(torch, cabi, a, b, y, g, cfg, slope):
    gp = torch.where(y > 0, g, g * slope)
    assert gp.dtype == torch.bfloat16
    want = cabi.correlation_backward(a, b, gp.contiguous(), *cfg)
    got = cabi.correlation_lrelu_backward(a, b, y, g, *cfg, slope)
    for u, v in zip(got, want):
        msg = pb.same_bits(pb.tensor_bits(torch, u), pb.tensor_bits(torch, v))
        assert not msg, msg
    return want


BWD_CASES = [((B, C, H, W), PWC) for B, C, H, W in [(1, 7, 13, 65), (3, 5, 9, 31), (2, 3, 5, 1), (1, 9, 21, 127), (3, 4, 6, 66)]] + \
            [((2, s[0], s[1], s[2]), (s[3], s[4], s[5], 1, s[6])) for s in (BACKWARD_SHAPES[1], BACKWARD_SHAPES[5])]


@pytest.mark.parametrize("shape,cfg", BWD_CASES)
def test_lrelu_backward_is_the_unactivated_backward_of_the_masked_gradient(torch_mod, cabi, shape, cfg):
    torch = torch_mod
    assert cfg == PWC or cfg[:3] != PWC[:3]
    rng = np.random.default_rng([7] + list(shape))
    f1, f2 = both_signs(rng, shape)
    a, b = bf(torch, f1), bf(torch, f2)
    B, (oc, oh, ow) = shape[0], out_dims(shape[2], shape[3], *cfg)
    y = cabi.correlation_lrelu_forward(a, b, *cfg, 0.1)
    g = bf(torch, pb.to_bf16(rng.standard_normal((B, oc, oh, ow))))
    for slope in (0.1, 0.5):
        lrelu_backward_check(torch, cabi, a, b, y, g, cfg, slope)
    # both branches: an all-negative and an all-positive y
    mag = bf(torch, pb.to_bf16(np.abs(rng.standard_normal((B, oc, oh, ow))) + 0.01))
    neg = lrelu_backward_check(torch, cabi, a, b, -mag, g, cfg, 0.1)
    pos = lrelu_backward_check(torch, cabi, a, b, mag, g, cfg, 0.1)
    plain = cabi.correlation_backward(a, b, g, *cfg)
    assert same(torch, pos[0], plain[0]) and same(torch, pos[1], plain[1]) and not same(torch, neg[0], plain[0])


@pytest.mark.parametrize("shape,cfg", [BWD_CASES[1], BWD_CASES[4], BWD_CASES[5]])
def test_lrelu_backward_reads_strided_gradient_and_y_where_they_lie(torch_mod, cabi, shape, cfg):
    torch = torch_mod
    rng = np.random.default_rng([8] + list(shape))
    f1, f2 = both_signs(rng, shape)
    a, b = bf(torch, f1), bf(torch, f2)
    B, (oc, oh, ow) = shape[0], out_dims(shape[2], shape[3], *cfg)
    y = cabi.correlation_lrelu_forward(a, b, *cfg, 0.1)
    g = bf(torch, pb.to_bf16(rng.standard_normal((B, oc, oh, ow))))
    want = lrelu_backward_check(torch, cabi, a, b, y, g, cfg, 0.1)
    # gradoutput: the narrow() view of a wider gradient (what torch.cat's backward hands down), at an odd per-image offset
    ystride = oc * oh * ow + 3
    ystride += 1 - ystride % 2                              # an odd image stride for y
    wide = torch.zeros((B, oc + 4, oh, ow), dtype=torch.bfloat16, device="cuda")
    gview = wide.narrow(1, 3, oc)
    gview.copy_(g)
    _, ys = pb.guarded(torch, (B, oc, oh, ow), torch.bfloat16, (ystride, oh * ow, ow, 1), 65)
    ys.copy_(y)
    assert not gview.is_contiguous() and not ys.is_contiguous() or B == 1
    for gg, yy in ((gview, y), (g, ys), (gview, ys)):
        got = cabi.correlation_lrelu_backward(a, b, yy, gg, *cfg, 0.1)
        assert same(torch, got[0], want[0]) and same(torch, got[1], want[1])


# ------------------------------------------------------------------ autograd

@pytest.mark.parametrize("flow_bf16", [False, True])
def test_fused_functions_give_the_cabi_gradients(torch_mod, cabi, fused, flow_bf16):
    torch = torch_mod
    gen = torch.Generator(device="cpu").manual_seed(19)
    shape = (2, 12, 20, 37)
    c1_0, c2_0 = (torch.randn(shape, generator=gen).bfloat16().cuda() for _ in range(2))
    flo_0 = (torch.randn(2, 2, 20, 37, generator=gen) * 2).cuda()
    flo_0 = flo_0.bfloat16() if flow_bf16 else flo_0
    gw = torch.randn(shape, generator=gen).bfloat16().cuda()
    go = torch.randn(2, 81, 20, 37, generator=gen).bfloat16().cuda()
    leaves = lambda: (c1_0.clone().requires_grad_(True), c2_0.clone().requires_grad_(True), flo_0.clone().requires_grad_(True))  # noqa: E731

    def warp_bwd(g):
        gx, gf = torch.empty_like(c2_0), torch.empty_like(flo_0)
        assert cabi.pwc_warp_backward(c2_0, flo_0, g, gx, gf, True) == 0
        return gx, gf

    warped = torch.empty_like(c2_0)
    assert cabi.pwc_warp_forward(c2_0, flo_0, warped, True) == 0
    # the warp alone: fused.warp stays float32 only (the existing suite pins that), the Function behind it takes bfloat16
    _, c2, flo = leaves()
    with pytest.raises(RuntimeError, match="must be float32"):
        fused.warp(c2, flo)
    with pytest.raises(RuntimeError, match="must be float32"):
        fused.corr_lrelu(c1_0, c2_0)
    out = fused._Warp.apply(c2, flo, True)
    assert out.dtype == torch.bfloat16 and out.grad_fn is not None and same(torch, out.detach(), warped)
    out.backward(gw)
    gx, gf = warp_bwd(gw)
    assert c2.grad.dtype == torch.bfloat16 and flo.grad.dtype == flo_0.dtype and same(torch, c2.grad, gx) and same(torch, flo.grad, gf)
    # warp_corr (one_launch is ignored on bfloat16, with and without autograd)
    for one_launch in (False, True):
        c1, c2, flo = leaves()
        out = fused.warp_corr(c1, c2, flo, one_launch=one_launch)
        with torch.no_grad():
            assert same(torch, fused.warp_corr(c1, c2, flo, one_launch=one_launch), out.detach())
        assert same(torch, out.detach(), cabi.correlation_forward(c1_0, warped, *PWC))
        out.backward(go)
        g1, gwarp = cabi.correlation_backward(c1_0, warped, go, *PWC)
        gx, gf = warp_bwd(gwarp)
        assert same(torch, c1.grad, g1) and same(torch, c2.grad, gx) and same(torch, flo.grad, gf)
    # the correlation + LeakyReLU alone (fused._CorrLrelu) and warp_corr_lrelu
    for second, fn in ((c2_0, lambda a, b, f: fused._CorrLrelu.apply(a, b, 0.1)), (warped, lambda a, b, f: fused.warp_corr_lrelu(a, b, f, True, 0.1))):
        c1, c2, flo = leaves()
        out = fn(c1, c2, flo)
        y = cabi.correlation_lrelu_forward(c1_0, second, *PWC, 0.1)
        assert out.dtype == torch.bfloat16 and same(torch, out.detach(), y)
        out.backward(go)
        g1, g2 = cabi.correlation_lrelu_backward(c1_0, second, y, go, *PWC, 0.1)
        if second is warped:
            g2, gf = warp_bwd(g2)
            assert same(torch, flo.grad, gf)
        assert same(torch, c1.grad, g1) and same(torch, c2.grad, g2)
    # inference: out= a channel slice of the concatenation buffer, no grad_fn
    with torch.no_grad():
        cat = torch.zeros((2, 81 + 12 + 2, 20, 37), dtype=torch.bfloat16, device="cuda")
        res = fused.warp_corr_lrelu(c1_0, c2_0, flo_0, out=cat[:, :81])
        assert res.grad_fn is None and same(torch, cat[:, :81], cabi.correlation_lrelu_forward(c1_0, warped, *PWC, 0.1))
        assert (cat[:, 81:] == 0).all()


@pytest.mark.parametrize("flow_bf16", [False, True])
def test_concatenated_use_equals_the_unfused_bfloat16_composition(torch_mod, fused, flow_bf16):
    """torch.cat((warp_corr_lrelu(c1, c2, flo), c1, flo), 1) under a weighted sum: the bits, forward and backward, of what a
    bfloat16 user wrote before -- casts around the float32 warp, the bfloat16 correlation, torch's leaky_relu."""
    torch = torch_mod
    F = torch.nn.functional
    gen = torch.Generator(device="cpu").manual_seed(29)
    shape = (2, 16, 24, 40)
    c1_0, c2_0 = (torch.randn(shape, generator=gen).bfloat16().cuda() for _ in range(2))
    flo_0 = (torch.randn(2, 2, 24, 40, generator=gen) * 2).cuda()
    flo_0 = flo_0.bfloat16() if flow_bf16 else flo_0
    wgt = torch.randn(2, 81 + 16 + 2, 24, 40, generator=gen).bfloat16().cuda()

    def run(block):
        c1, c2, flo = (t.clone().requires_grad_(True) for t in (c1_0, c2_0, flo_0))
        cost = block(c1, c2, flo)
        total = (torch.cat((cost, c1, flo.to(cost.dtype)), 1) * wgt).float().sum()
        total.backward()
        return cost.detach(), total.detach(), c1.grad, c2.grad, flo.grad

    new = run(lambda c1, c2, flo: fused.warp_corr_lrelu(c1, c2, flo))
    old = run(lambda c1, c2, flo: F.leaky_relu(fused._Corr.apply(c1, fused.warp(c2.float(), flo.float()).to(c1.dtype)), 0.1))
    for a, b in zip(new, old):
        assert same(torch, a, b)
    assert new[2].dtype == torch.bfloat16 and new[4].dtype == flo_0.dtype


# ------------------------------------------------------------------ under autocast

def test_pwc_level_trains_under_bf16_autocast(torch_mod, fused, cabi):
    """One PWC-Net-like level under torch.autocast(dtype=torch.bfloat16) with no cast written anywhere: conv features, conv
    flow (from the images, so that a feature tensor's gradient is the fused block's alone), warp_corr_lrelu, conv head, loss;
    8 channels, 12 x 20, B = 2.  Judged as test_network_trains_under_bf16_autocast judges the plain correlation: float64 on
    the CPU from the bfloat16 tensors autocast retains (features a and b, the flow, the block's output and its gradient, the
    head's output gradient), the tolerances formed the same way.

      * the warped features w (recomputed from the retained b and flow by the warp's C-ABI call: the same deterministic launch):
        2^-8 |W| + 1e-5 A, A the sum of |weight x value| -- one rounding to bfloat16 plus float32 arithmetic on four terms;
      * the block's output against lrelu(R), R the float64 mean over (a, w): 2 tol(R) + 2^-8 |lrelu(R)| with tol the
        correlation's bound -- the stored mean is within tol of R, so where the two differ in sign both are within tol of
        zero, and the activation's own rounding is 2^-9 relative;
      * a's gradient and the warped tensor's gradient (recomputed by the C-ABI call on the retained tensors; a's must equal
        autograd's bit for bit) against float64 over the masked gradient g' (formed from the retained bfloat16 tensors, which
        is exact): tolerance(G, A, 81 + 32) as in that test;
      * b's and the flow's gradients against the float64 restatement of the warp backward fed that bfloat16 gradient: the
        float32 test's bounds plus half a bfloat16 ulp;
      * the head's weight and bias gradients: that test's check, with the block's output bound pushed through the convolution.
    The other parameter gradients are float32, finite and non-zero.  A second run gives the same bits everywhere."""
    torch = torch_mod
    slope = 0.1

    def run():
        torch.manual_seed(31)
        feat = torch.nn.Conv2d(3, 8, 3, padding=1).cuda()
        flow = torch.nn.Conv2d(6, 2, 3, padding=1).cuda()
        head = torch.nn.Conv2d(81, 2, 3, padding=1).cuda()
        x0, x1 = torch.randn(2, 3, 12, 20, device="cuda"), torch.randn(2, 3, 12, 20, device="cuda")
        with torch.autocast("cuda", dtype=torch.bfloat16):
            a, b = feat(x0), feat(x1)
            flo = flow(torch.cat((x0, x1), 1))
            cost = fused.warp_corr_lrelu(a, b, flo, negative_slope=slope)
            y = head(cost)
            loss = y.float().pow(2).mean()
        for t in (a, b, flo, cost, y):
            t.retain_grad()
        loss.backward()
        params = list(feat.parameters()) + list(flow.parameters()) + list(head.parameters())
        return a, b, flo, cost, y, head, params

    a, b, flo, cost, y, head, params = run()
    for t in (a, b, flo, cost, y):
        assert t.dtype == torch.bfloat16 and t.grad is not None and t.grad.dtype == torch.bfloat16
    for p in params:
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0
    again = run()
    for t, u in zip((a, b, flo, cost, y), again[:5]):
        assert same(torch, t.detach(), u.detach()) and same(torch, t.grad, u.grad)
    for p, q in zip(params, again[6]):
        assert same(torch, p.grad, q.grad)

    np64 = lambda t: t.detach().float().cpu().numpy().astype(np.float64)       # noqa: E731
    np32 = lambda t: t.detach().float().cpu().numpy()                            # noqa: E731
    # the warp
    w = torch.empty_like(b)
    assert cabi.pwc_warp_forward(b.detach(), flo.detach(), w, True) == 0
    W, WA = pb.warp_forward_f64(np32(b), np32(flo), True)
    assert (np.abs(np64(w) - W) <= 2.0 ** -8 * np.abs(W) + 1e-5 * WA).all()
    # the block's output
    f1, f2 = np32(a), np32(w)
    R, RA = cb.reference(f1, f2)
    Y = np.where(R > 0, R, R * slope)
    tol_y = 2 * cb.tolerance(R, RA, 8) + 2.0 ** -8 * np.abs(Y)
    err = np.abs(np64(cost) - Y)
    print("output: worst error / bound %.3f" % float((err / np.maximum(tol_y, 1e-300)).max()))
    assert (err <= tol_y).all()
    # the correlation's gradients over the masked gradient
    g1, gw = cabi.correlation_lrelu_backward(a.detach(), w, cost.detach(), cost.grad, *PWC, slope)
    assert same(torch, a.grad, g1)
    gp = pb.masked_gradient(np32(cost.grad), np32(cost), slope)
    G1, G2, A1, A2 = backward_reference(f1, f2, gp)
    for got, G, A in ((g1, G1, A1), (gw, G2, A2)):
        err, tol = np.abs(np64(got) - G), cb.tolerance(G, A, 81 + 32)
        print("gradient: worst error / bound %.3f" % float((err / np.maximum(tol, 1e-300)).max()))
        assert (err <= tol).all()
    # the warp's gradients
    ref = pb.pwc_warp_bwd(np32(b), np32(flo), np32(gw), True)
    pb.bf16_within(np64(b.grad), np64(flo.grad), ref, np32(gw), flow_bf16=True)
    # the head's parameter gradients
    t64 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))      # noqa: E731
    cw = lambda x, gr, shape: torch.nn.grad.conv2d_weight(t64(x), shape, t64(gr), padding=1).numpy()      # noqa: E731
    n = 2 * 12 * 20
    gy, ws = np64(y.grad), tuple(head.weight.shape)
    for name, got, refv, push, S in (
            ("head.weight", head.weight.grad, cw(Y, gy, ws), cw(tol_y, np.abs(gy), ws), cw(np.abs(Y), np.abs(gy), ws)),
            ("head.bias", head.bias.grad, gy.sum(axis=(0, 2, 3)), np.zeros(2), np.abs(gy).sum(axis=(0, 2, 3)))):
        tol = (1 + 2.0 ** -6) * push + 2.0 ** -8 * np.abs(refv) + (n + 2) * 2.0 ** -23 * S
        err = np.abs(np64(got) - refv)
        print("%s: worst error / bound %.3f" % (name, float((err / tol).max())))
        assert (err <= tol).all(), name
        if refv.size >= 100:
            assert (np.abs(refv) > 4 * tol).mean() > 0.5, name
