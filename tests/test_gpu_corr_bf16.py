"""GPU: the bfloat16 correlation (vfi_correlation_forward_bf16 / _backward_bf16).

Forward, the MFMA kernel (run directly through cabi.correlation_forward_bf16_kernel, so every shape reaches it whatever the
dispatch's tile threshold): the derived bound of tests/corr_bf16.py against the float64 reference, at least 99 % of the
outputs bit-equal to bf16_rne(R), two runs with equal bits, untouched guards either side of the output; integer inputs bit
for bit.  Forward, the generic kernel, and the backward: bit for bit bf16_rne of the CPU oracle's float32 result on the
widened inputs.  The public entry must give the bits of the kernel the dispatch mirror names.  Then the reference-named
module, the autograd layers and a small network under torch.autocast(dtype=torch.bfloat16)."""
import numpy as np
import pytest

from tests import corr_bf16 as cb
from tests.corr_edges import out_dims
from tests.test_gpu_correlation_f16_backward import SHAPES as BACKWARD_SHAPES

pytestmark = pytest.mark.gpu

PWC = cb.PWC


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


def dev(torch, x, offset=0):
    """x (float32 holding bfloat16 values) as a bfloat16 tensor on the GPU; offset: a dense view that starts `offset`
    elements into its storage"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16)
    if not offset:
        return t.cuda()
    buf = torch.empty(t.numel() + offset, dtype=torch.bfloat16, device="cuda")
    view = buf[offset:].view(t.shape)
    view.copy_(t)
    return view


def rand(rng, shape, scale=1.0):
    return cb.to_bf16(rng.standard_normal(shape) * scale)


GUARD_PATTERN = 0x5A5A


def run_guarded(torch, cabi, which, a, b, cfg, guard):
    """One forward kernel into a view `guard` elements into a pattern-filled buffer: the output's bits, after checking that
    the `guard` elements either side still hold the pattern."""
    B, C, H, W = a.shape
    oc, oh, ow = out_dims(H, W, *cfg)
    n = B * oc * oh * ow
    buf = torch.full((n + 2 * guard,), GUARD_PATTERN, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    out = buf[guard:guard + n].view(B, oc, oh, ow)
    cabi.correlation_forward_bf16_kernel(which, a, b, *cfg, out=out)
    torch.cuda.synchronize()
    raw = buf.view(torch.int16).cpu().numpy().view(np.uint16)
    assert (raw[:guard] == GUARD_PATTERN).all() and (raw[guard + n:] == GUARD_PATTERN).all(), "a guard element was written"
    return raw[guard:guard + n].reshape(B, oc, oh, ow).copy()


# (B, C, H, W), pad, storage offset of the inputs and guard width (an odd guard puts the output on a 2-byte boundary only)
MFMA_SHAPES = [
    ((1, 1, 1, 1), 4, 0, 64),            # everything but the centre tap is padding
    ((2, 33, 5, 5), 4, 0, 64),           # narrower than the band; K tail of one channel
    ((1, 32, 4, 16), 4, 0, 64),          # exactly one 16-pixel block and one K step
    ((2, 196, 7, 21), 4, 0, 64),         # ragged both ways; tail of 4
    ((3, 8, 9, 47), 4, 0, 64),           # width 16 * 3 - 1; batch 3; C below one K step
    ((1, 196, 18, 31), 4, 0, 64),        # the coarsest 1080p level
    ((1, 32, 64, 256), 4, 0, 64),        # past any plausible tile threshold
    ((1, 16, 12, 20), 3, 0, 64),         # pad != max displacement
    ((2, 33, 7, 21), 4, 1, 33),          # 2-byte-aligned pointers only, inputs and output
    ((1, 5, 3, 130), 4, 0, 64),          # three 64-pixel tiles, the last 2 pixels wide; one output row of a two-row tile
]


@pytest.mark.parametrize("shape,pad,offset,guard", MFMA_SHAPES)
def test_mfma_forward_bound_exact_fraction_repeat_guards(torch_mod, cabi, oracle, shape, pad, offset, guard):
    torch = torch_mod
    cfg = (pad, 1, 4, 1, 1)
    rng = np.random.default_rng([20261020] + list(shape) + [pad])
    f1, f2 = rand(rng, shape), rand(rng, shape)
    a, b = dev(torch, f1, offset), dev(torch, f2, offset)
    assert a.data_ptr() % 4 == 2 * (offset % 2)
    got = run_guarded(torch, cabi, "mfma", a, b, cfg, guard)
    cb.check_mfma_result(got, f1, f2, cfg)
    again = run_guarded(torch, cabi, "mfma", a, b, cfg, guard)
    assert np.array_equal(got, again), "two runs differ"
    # the generic kernel on the same frame, and the public entry: the kernel the dispatch mirror names
    want = cb.bits(oracle.correlation_fwd(f1, f2, *cfg, order=1, fmad=1))
    gen = run_guarded(torch, cabi, "generic", a, b, cfg, guard)
    assert not cb.same_bits(gen, want), cb.same_bits(gen, want)
    pub = cabi.correlation_forward(a, b, *cfg)
    assert pub.dtype == torch.bfloat16
    pub = pub.cpu().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(pub, got if cb.selected_kernel(*shape, cfg) == "mfma" else gen)


def test_dispatch_reaches_both_kernels_at_these_shapes():
    """The shapes above lie on both sides of the threshold (the mirror is pinned to the source by the host test)."""
    reached = {cb.selected_kernel(*s, (pad, 1, 4, 1, 1)) for s, pad, _, _ in MFMA_SHAPES}
    assert reached == {"mfma", "generic"}


@pytest.mark.parametrize("shape", [(2, 33, 5, 5), (2, 196, 7, 21), (3, 8, 9, 47)])
def test_mfma_ragged_classes_at_the_smallest_frame_past_the_threshold(torch_mod, cabi, shape):
    """The ragged classes once more through the PUBLIC entry, on the MFMA side of the threshold: the same channel counts on
    frames grown (odd sizes kept) until the dispatch takes the MFMA kernel."""
    torch = torch_mod
    B, C, H, W = shape
    while cb.selected_kernel(B, C, H, W) != "mfma":
        H += 4
        if cb.selected_kernel(B, C, H, W) != "mfma":
            W += 16
    assert cb.selected_kernel(B, C, H - 4, W - 16) == "generic" and H * W * C < 4e6, (H, W)
    rng = np.random.default_rng([7, B, C, H, W])
    f1, f2 = rand(rng, (B, C, H, W)), rand(rng, (B, C, H, W))
    a, b = dev(torch, f1), dev(torch, f2)
    got = cabi.correlation_forward(a, b, *PWC).cpu().view(torch.int16).numpy().view(np.uint16)
    cb.check_mfma_result(got, f1, f2)
    assert np.array_equal(got, run_guarded(torch, cabi, "mfma", a, b, PWC, 64))


@pytest.mark.parametrize("C", [16, 32, 64])
def test_mfma_forward_integer_inputs_bit_for_bit(torch_mod, cabi, C):
    """Integers in [-4, 4]: every partial sum is exact in float32 in any order, and so is the division by a power of two."""
    torch = torch_mod
    rng = np.random.default_rng(C)
    f1, f2 = (rng.integers(-4, 5, (2, C, 7, 21)).astype(np.float32) for _ in range(2))
    R, _ = cb.reference(f1, f2)
    got = run_guarded(torch, cabi, "mfma", dev(torch, f1), dev(torch, f2), PWC, 64)
    assert np.array_equal(got, cb.bits(R))
    assert np.array_equal(run_guarded(torch, cabi, "generic", dev(torch, f1), dev(torch, f2), PWC, 64), cb.bits(R))


@pytest.mark.parametrize("shape,cfg", [((2, 3, 8, 8), (4, 3, 4, 1, 2)), ((2, 4, 12, 20), (3, 1, 3, 1, 1)), ((2, 33, 7, 21), PWC)])
def test_generic_forward_bit_for_bit(torch_mod, cabi, oracle, shape, cfg):
    torch = torch_mod
    rng = np.random.default_rng([3] + list(shape))
    f1, f2 = rand(rng, shape), rand(rng, shape)
    want = cb.bits(oracle.correlation_fwd(f1, f2, *cfg, order=1, fmad=1))
    a, b = dev(torch, f1), dev(torch, f2)
    if cfg != PWC:
        assert cb.selected_kernel(*shape, cfg) == "generic"
        got = cabi.correlation_forward(a, b, *cfg).cpu().view(torch.int16).numpy().view(np.uint16)
        assert not cb.same_bits(got, want), cb.same_bits(got, want)
    gen = run_guarded(torch, cabi, "generic", a, b, cfg, 33)
    assert not cb.same_bits(gen, want), cb.same_bits(gen, want)


def test_forward_non_finite_inputs_both_kernels(torch_mod, cabi, oracle):
    """+inf inside x1, -inf in x2, a NaN, and an inf of x1 at the border whose padding taps give inf * 0 = NaN."""
    torch = torch_mod
    rng = np.random.default_rng(5)
    shape = (1, 5, 11, 20)
    f1, f2 = rand(rng, shape), rand(rng, shape)
    f1[0, 2, 5, 10] = np.inf
    f2[0, 1, 6, 14] = -np.inf
    f1[0, 0, 3, 16] = np.nan
    f1[0, 4, 0, 0] = np.inf
    R, _ = cb.reference(f1, f2)
    assert np.isnan(R[0, 0, 0, 0]) and np.isinf(R).any() and np.isnan(R).sum() < R.size // 2     # a padding tap; inf kept
    a, b = dev(torch, f1), dev(torch, f2)
    cb.check_mfma_result(run_guarded(torch, cabi, "mfma", a, b, PWC, 64), f1, f2)
    want = cb.bits(oracle.correlation_fwd(f1, f2, *PWC, order=1, fmad=1))
    gen = run_guarded(torch, cabi, "generic", a, b, PWC, 64)
    assert not cb.same_bits(gen, want), cb.same_bits(gen, want)
    g = cb.from_bits(gen)
    assert np.array_equal(np.isnan(g), np.isnan(R)) and np.array_equal(g[np.isinf(R)], R[np.isinf(R)])


# ------------------------------------------------------------------ backward

def backward_check(torch, cabi, oracle, f1, f2, g, pad, k, md, s2):
    want = oracle.correlation_bwd(f1, f2, g, pad, k, md, 1, s2)
    got = cabi.correlation_backward(dev(torch, f1), dev(torch, f2), dev(torch, g), pad, k, md, 1, s2)
    for a, w in zip(got, want):
        assert a.dtype == torch.bfloat16
        msg = cb.same_bits(a.cpu().view(torch.int16).numpy().view(np.uint16), cb.bits(w))
        assert not msg, msg
    return want


@pytest.mark.parametrize("shape", BACKWARD_SHAPES)
def test_backward_bit_for_bit(torch_mod, cabi, oracle, shape):
    C, H, W, pad, k, md, s2 = shape
    rng = np.random.default_rng(sum(shape))
    oc, oh, ow = out_dims(H, W, pad, k, md, 1, s2)
    backward_check(torch_mod, cabi, oracle, rand(rng, (2, C, H, W)), rand(rng, (2, C, H, W)), rand(rng, (2, oc, oh, ow)), pad, k, md, s2)


@pytest.mark.parametrize("B,C,H,W", [(1, 7, 13, 65), (3, 5, 9, 31), (2, 3, 5, 1), (1, 9, 21, 127), (3, 4, 6, 66)])
def test_backward_tiled_odd_widths_channels_batch(torch_mod, cabi, oracle, B, C, H, W):
    rng = np.random.default_rng(B * 1000 + C * 100 + W)
    backward_check(torch_mod, cabi, oracle, rand(rng, (B, C, H, W)), rand(rng, (B, C, H, W)), rand(rng, (B, 81, H, W)), 4, 1, 4, 1)


@pytest.mark.parametrize("C,H,W", [(196, 18, 31), (32, 288, 496)])
def test_backward_1080p_pwc_levels(torch_mod, cabi, oracle, C, H, W):
    rng = np.random.default_rng(C)
    backward_check(torch_mod, cabi, oracle, rand(rng, (1, C, H, W)), rand(rng, (1, C, H, W)), rand(rng, (1, 81, H, W)), 4, 1, 4, 1)


@pytest.mark.parametrize("shape", [(5, 11, 20, 4, 1, 4, 1), (3, 10, 12, 3, 3, 3, 2)])
def test_backward_inf_in_gradoutput_at_the_border(torch_mod, cabi, oracle, shape):
    """An inf in gradOutput at the border meets padding taps: inf * 0 = NaN, on both kernels."""
    C, H, W, pad, k, md, s2 = shape
    rng = np.random.default_rng(11)
    oc, oh, ow = out_dims(H, W, pad, k, md, 1, s2)
    f1, f2, g = rand(rng, (1, C, H, W)), rand(rng, (1, C, H, W)), rand(rng, (1, oc, oh, ow))
    g[0, 7, 0, 0] = np.inf
    want = backward_check(torch_mod, cabi, oracle, f1, f2, g, pad, k, md, s2)
    assert any(np.isnan(w).any() for w in want) and not all(np.isnan(w).all() for w in want)


@pytest.mark.parametrize("shape", [(6, 9, 33, 4, 1, 4, 1), (3, 8, 8, 4, 3, 4, 2), (4, 12, 20, 3, 1, 4, 1)])
def test_backward_writes_every_element_through_the_module(torch_mod, cabi, oracle, shape):
    """NaN-prefilled gradients through correlation_cuda.backward: nothing survives, result as through cabi."""
    torch = torch_mod
    import correlation_cuda
    C, H, W, pad, k, md, s2 = shape
    rng = np.random.default_rng(17)
    oc, oh, ow = out_dims(H, W, pad, k, md, 1, s2)
    f1, f2, g = rand(rng, (2, C, H, W)), rand(rng, (2, C, H, W)), rand(rng, (2, oc, oh, ow))
    a, b, go = dev(torch, f1), dev(torch, f2), dev(torch, g)
    g1 = torch.full((2, C, H, W), float("nan"), dtype=torch.bfloat16, device="cuda")
    g2 = torch.full_like(g1, float("nan"))
    assert correlation_cuda.backward(a, b, a.new_empty(0), a.new_empty(0), go, g1, g2, pad, k, md, 1, s2, 1) == 1
    assert not torch.isnan(g1).any() and not torch.isnan(g2).any()
    c1, c2 = cabi.correlation_backward(a, b, go, pad, k, md, 1, s2)
    assert torch.equal(g1.view(torch.int16), c1.view(torch.int16)) and torch.equal(g2.view(torch.int16), c2.view(torch.int16))
    want = oracle.correlation_bwd(f1, f2, g, pad, k, md, 1, s2)
    assert np.array_equal(g1.cpu().view(torch.int16).numpy().view(np.uint16), cb.bits(want[0]))
    assert np.array_equal(g2.cpu().view(torch.int16).numpy().view(np.uint16), cb.bits(want[1]))


# ------------------------------------------------------------------ module and autograd

def test_module_forward_equals_cabi(torch_mod, cabi):
    torch = torch_mod
    import correlation_cuda
    rng = np.random.default_rng(23)
    for shape in ((2, 33, 7, 21), (1, 32, 64, 256)):
        a, b = dev(torch, rand(rng, shape)), dev(torch, rand(rng, shape))
        out = a.new_empty(0)
        assert correlation_cuda.forward(a, b, a.new_empty(0), a.new_empty(0), out, 4, 1, 4, 1, 1, 1) == 1
        assert out.dtype == torch.bfloat16 and tuple(out.shape) == (shape[0], 81, shape[2], shape[3])
        assert torch.equal(out.view(torch.int16), cabi.correlation_forward(a, b, *PWC).view(torch.int16))


def test_mixed_dtypes_raise(torch_mod, cabi):
    torch = torch_mod
    import correlation_cuda
    a = torch.randn(1, 4, 8, 10, device="cuda").bfloat16()
    b = torch.randn(1, 4, 8, 10, device="cuda").bfloat16()
    go = torch.randn(1, 81, 8, 10, device="cuda").bfloat16()
    e = a.new_empty(0)
    for bad in (b.float(), b.half()):
        with pytest.raises(RuntimeError):
            correlation_cuda.forward(a, bad, e, e, a.new_empty(0), 4, 1, 4, 1, 1, 1)
        with pytest.raises(RuntimeError):
            correlation_cuda.backward(a, bad, e, e, go, a.new_empty(0), a.new_empty(0), 4, 1, 4, 1, 1, 1)
        with pytest.raises(RuntimeError, match="tensors must be bfloat16"):
            cabi.correlation_forward(a, bad, *PWC)
        with pytest.raises(RuntimeError, match="tensors must be bfloat16"):
            cabi.correlation_backward(a, bad, go, *PWC)
    with pytest.raises(RuntimeError):
        correlation_cuda.backward(a, b, e, e, go.float(), a.new_empty(0), a.new_empty(0), 4, 1, 4, 1, 1, 1)
    with pytest.raises(RuntimeError, match="tensors must be bfloat16"):
        cabi.correlation_backward(a, b, go.float(), *PWC)
    with pytest.raises(RuntimeError, match="GPU"):
        cabi.correlation_backward(a.cpu(), b.cpu(), go.cpu(), *PWC)


def test_autograd_layers_give_the_cabi_gradients(torch_mod, cabi):
    """Correlation(4, 1, 4, 1, 1) and fused._Corr on bfloat16 leaves; fused.warp_corr's correlation half on a warped map
    cast back to the features' dtype (grid_sample and fused.warp are float32)."""
    torch = torch_mod
    from vfidkr_amd import fused
    from vfidkr_amd.PWCNet.correlation_package_pytorch1_0.correlation import Correlation
    gen = torch.Generator(device="cpu").manual_seed(19)
    c1 = torch.randn(2, 12, 20, 37, generator=gen).bfloat16().cuda()
    c2 = torch.randn(2, 12, 20, 37, generator=gen).bfloat16().cuda()
    go = torch.randn(2, 81, 20, 37, generator=gen).bfloat16().cuda()
    want_out = cabi.correlation_forward(c1, c2, *PWC)
    w1, w2 = cabi.correlation_backward(c1, c2, go, *PWC)
    for layer in (Correlation(4, 1, 4, 1, 1, 1), fused._Corr.apply):
        a, b = c1.clone().requires_grad_(True), c2.clone().requires_grad_(True)
        out = layer(a, b)
        assert out.dtype == torch.bfloat16 and torch.equal(out.view(torch.int16), want_out.view(torch.int16))
        out.backward(go)
        assert a.grad.dtype == torch.bfloat16 and b.grad.dtype == torch.bfloat16
        assert torch.equal(a.grad.view(torch.int16), w1.view(torch.int16)) and torch.equal(b.grad.view(torch.int16), w2.view(torch.int16))
    flo = torch.randn(2, 2, 20, 37, generator=gen).cuda()
    with pytest.raises(RuntimeError):
        fused.warp(c2, flo)                                                     # float32 only, and says so
    warped = fused.warp(c2.float(), flo).to(c1.dtype)
    assert torch.equal(fused._Corr.apply(c1, warped).view(torch.int16), cabi.correlation_forward(c1, warped, *PWC).view(torch.int16))
    with pytest.raises(RuntimeError):
        fused.corr_pair(c1, c2, c2, c1)
    with pytest.raises(RuntimeError):
        fused.corr_lrelu(c1, c2)


def backward_reference(f1, f2, g):
    """float64 gradients of PWC-Net's configuration and the same sums over |g * v| (both over the 81 displacements)."""
    B, C, H, W = f1.shape
    p1, p2 = np.pad(f1.astype(np.float64), ((0, 0), (0, 0), (4, 4), (4, 4))), np.pad(f2.astype(np.float64), ((0, 0), (0, 0), (4, 4), (4, 4)))
    g = g.astype(np.float64)
    G1, G2, A1, A2 = (np.zeros((B, C, H + 8, W + 8)) for _ in range(4))
    for tj in range(9):
        for ti in range(9):
            gt = g[:, tj * 9 + ti][:, None]                                     # out[y, x] = f1[y, x] * f2[y + tj - 4, x + ti - 4]
            v2 = p2[:, :, tj:tj + H, ti:ti + W]
            G1[:, :, 4:4 + H, 4:4 + W] += gt * v2
            A1[:, :, 4:4 + H, 4:4 + W] += np.abs(gt * v2)
            G2[:, :, tj:tj + H, ti:ti + W] += gt * f1
            A2[:, :, tj:tj + H, ti:ti + W] += np.abs(gt * f1)
    crop = lambda t: t[:, :, 4:4 + H, 4:4 + W] / C
    return crop(G1), crop(G2), crop(A1), crop(A2)


def test_network_trains_under_bf16_autocast(torch_mod):
    """conv -> Correlation(4, 1, 4, 1, 1) -> conv under torch.autocast(dtype=torch.bfloat16), 8 channels, 12 x 20: no cast
    around the correlation.  Everything is compared with float64 computed on the CPU from the bfloat16 tensors autocast
    retains (the correlation's inputs a and b, the gradient of its output, the gradient gy of the head's output, the
    bfloat16-rounded images):

      * the correlation's output: the forward's derived bound (tests/corr_bf16.py);
      * the gradients it hands back: the same kind of bound -- exact products, 81 fused multiply-adds and 32 partial
        additions in float32, one division, the rounding to bfloat16: tolerance(G, A, 81 + 32) on the sum of |g * v|;
      * every PARAMETER gradient against torch.nn.grad.conv2d_weight in float64 fed the float64 correlation results (R for
        the head, G1 and G2 for the first convolution), within
            push + 2^-8 (sum of |each convolution's gradient| + |their sum|) + (n + 2) 2^-23 S.
        push: the correlation's bound above pushed through the convolution (the convolution of the absolute values of its
        other operand with the bound, widened by 2^-6 for the roundings that act on it).  The rest is the allowance for
        torch's bfloat16 convolution backward, taken to be: exact bfloat16 products, n = B H W = 480 terms added in float32
        in any order (S: the sum of their absolute values), the result rounded to bfloat16 once per convolution, and the
        first convolution's two weight gradients (it is called twice) added in bfloat16 -- one more rounding."""
    torch = torch_mod
    from vfidkr_amd.PWCNet.correlation_package_pytorch1_0.correlation import Correlation
    torch.manual_seed(23)
    feat = torch.nn.Conv2d(3, 8, 3, padding=1).cuda()
    head = torch.nn.Conv2d(81, 2, 3, padding=1).cuda()
    corr = Correlation(4, 1, 4, 1, 1, 1)
    x0, x1 = torch.randn(2, 3, 12, 20, device="cuda"), torch.randn(2, 3, 12, 20, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        a, b = feat(x0), feat(x1)
        a.retain_grad(), b.retain_grad()
        cost = corr(a, b)
        cost.retain_grad()
        y = head(cost)
        y.retain_grad()
        loss = y.float().pow(2).mean()
    assert a.dtype == torch.bfloat16 and cost.dtype == torch.bfloat16 and y.dtype == torch.bfloat16
    loss.backward()
    for p in list(feat.parameters()) + list(head.parameters()):
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0
    assert a.grad.dtype == torch.bfloat16 and cost.grad.dtype == torch.bfloat16 and y.grad.dtype == torch.bfloat16
    f1, f2, g = (t.detach().float().cpu().numpy() for t in (a, b, cost.grad))

    # the correlation, forward and backward
    cb.check_mfma_result(cost.detach().cpu().view(torch.int16).numpy().view(np.uint16), f1, f2, min_exact=0.99)
    R, RA = cb.reference(f1, f2)
    tol_fwd = cb.tolerance(R, RA, 8)
    G1, G2, A1, A2 = backward_reference(f1, f2, g)
    tols = [cb.tolerance(G, A, 81 + 32) for G, A in ((G1, A1), (G2, A2))]
    for got, G, tol in ((a.grad, G1, tols[0]), (b.grad, G2, tols[1])):
        err = np.abs(got.float().cpu().numpy().astype(np.float64) - G)
        print("gradient: worst error / bound %.3f" % float((err / np.maximum(tol, 1e-300)).max()))
        assert (err <= tol).all()

    # the parameter gradients
    f64 = lambda t: (t if isinstance(t, np.ndarray) else t.detach().float().cpu().numpy()).astype(np.float64)
    t64 = lambda x: torch.from_numpy(np.ascontiguousarray(f64(x)))
    cw = lambda x, gr, shape: torch.nn.grad.conv2d_weight(t64(x), shape, t64(gr), padding=1).numpy()
    n = 2 * 12 * 20
    u8, u23 = 2.0 ** -8, (n + 2) * 2.0 ** -23

    def check(name, got, parts):
        """parts: per convolution (gradient, push, sum of absolute terms); got: the parameter's float32 gradient"""
        ref = sum(p[0] for p in parts)
        tol = (1 + 2.0 ** -6) * sum(p[1] for p in parts) + u8 * (sum(np.abs(p[0]) for p in parts) + (len(parts) > 1) * np.abs(ref)) \
            + u23 * sum(p[2] for p in parts)
        err = np.abs(f64(got) - ref)
        print("%s: worst error / bound %.3f, largest |gradient| / bound %.1f" % (
            name, float((err / tol).max()), float((np.abs(ref) / tol).max())))
        assert (err <= tol).all(), name
        if ref.size >= 100:                                         # (the weights: the bound would not pass a wrong sign or a factor of two)
            assert (np.abs(ref) > 4 * tol).mean() > 0.5, name

    gy = f64(y.grad)
    ws, wf = tuple(head.weight.shape), tuple(feat.weight.shape)
    check("head.weight", head.weight.grad, [(cw(R, gy, ws), cw(tol_fwd, np.abs(gy), ws), cw(np.abs(R), np.abs(gy), ws))])
    check("head.bias", head.bias.grad, [(gy.sum(axis=(0, 2, 3)), np.zeros(2), np.abs(gy).sum(axis=(0, 2, 3)))])
    xs = [cb.to_bf16(f64(x)) for x in (x0, x1)]                                  # autocast rounds the images for the convolution
    check("feat.weight", feat.weight.grad,
          [(cw(x, G, wf), cw(np.abs(x), tol, wf), cw(np.abs(x), np.abs(G) + tol, wf)) for x, G, tol in zip(xs, (G1, G2), tols)])
    check("feat.bias", feat.bias.grad,
          [(G.sum(axis=(0, 2, 3)), tol.sum(axis=(0, 2, 3)), (np.abs(G) + tol).sum(axis=(0, 2, 3))) for G, tol in zip((G1, G2), tols)])


