"""GPU: the half-precision correlation backward (vfi_correlation_backward_f16: corr_backward_f16 and, for PWC-Net's
configuration, corr_backward_k1_f16) against the numpy restatement of the reference's at::Half arithmetic
(tests/corr_half_backward.py), bit for bit as uint16 (NaN positions included), through the C ABI, the reference-named
module and the autograd layer."""
import numpy as np
import pytest

from tests.corr_half_backward import correlation_bwd_half, out_dims

pytestmark = pytest.mark.gpu

f16 = np.float16


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


def h2d(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f16)).cuda()


def same_bits(got, want):
    g = got.detach().cpu().numpy() if hasattr(got, "detach") else got
    assert g.dtype == f16 and g.shape == want.shape
    gb, wb = g.view(np.uint16), want.view(np.uint16)
    nan_g, nan_w = np.isnan(g), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), int((nan_g != nan_w).sum())
    bad = (gb != wb) & ~nan_w
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist())


def check(torch, cabi, f1, f2, g, pad, k, md, s2):
    want = correlation_bwd_half(f1, f2, g, pad, k, md, 1, s2)
    got = cabi.correlation_backward(h2d(torch, f1), h2d(torch, f2), h2d(torch, g), pad, k, md, 1, s2)
    for a, b in zip(got, want):
        assert a.dtype == torch.float16
        same_bits(a, b)
    return want


def rand(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(f16)


# the float32 test's six shapes (test_gpu_parity.py: ragged tiles, several channel groups, 2x3 frames, pad != md, k 3 / s2 2)
SHAPES = ((6, 9, 33, 4, 1, 4, 1), (3, 8, 8, 4, 3, 4, 2), (32, 36, 62, 4, 1, 4, 1), (5, 70, 130, 4, 1, 4, 1),
          (2, 3, 2, 4, 1, 4, 1), (4, 12, 20, 3, 1, 4, 1))


@pytest.mark.parametrize("shape", SHAPES)
def test_half_backward_matches_restatement(torch_mod, cabi, shape):
    C, H, W, pad, k, md, s2 = shape
    rng = np.random.default_rng(sum(shape))
    oc, oh, ow = out_dims(H, W, pad, k, md, 1, s2)
    check(torch_mod, cabi, rand(rng, (2, C, H, W)), rand(rng, (2, C, H, W)), rand(rng, (2, oc, oh, ow)), pad, k, md, s2)


@pytest.mark.parametrize("B,C,H,W", [(1, 7, 13, 65), (3, 5, 9, 31), (2, 3, 5, 1), (1, 9, 21, 127), (3, 4, 6, 66)])
def test_half_backward_tiled_odd_widths_channels_batch(torch_mod, cabi, B, C, H, W):
    """The tiled kernel's odd pixel pair (odd widths), odd channel counts, batch 3."""
    rng = np.random.default_rng(B * 1000 + C * 100 + W)
    check(torch_mod, cabi, rand(rng, (B, C, H, W)), rand(rng, (B, C, H, W)), rand(rng, (B, 81, H, W)), 4, 1, 4, 1)


@pytest.mark.parametrize("C,H,W", [(196, 18, 31), (32, 288, 496)])
def test_half_backward_1080p_pwc_levels(torch_mod, cabi, C, H, W):
    """The coarsest and the finest level of the PWC pyramid at 1080p."""
    rng = np.random.default_rng(C)
    check(torch_mod, cabi, rand(rng, (1, C, H, W)), rand(rng, (1, C, H, W)), rand(rng, (1, 81, H, W)), 4, 1, 4, 1)


@pytest.mark.parametrize("shape", [(5, 11, 20, 4, 1, 4, 1), (3, 10, 12, 3, 3, 3, 2)])
def test_half_backward_magnitude_edges(torch_mod, cabi, shape):
    """Subnormal products, partials that overflow to inf, inf - inf = NaN, an inf in gradOutput at the border (a padding
    tap: inf * 0 = NaN), on both kernels."""
    C, H, W, pad, k, md, s2 = shape
    rng = np.random.default_rng(11)
    oc, oh, ow = out_dims(H, W, pad, k, md, 1, s2)
    f1, f2, g = rand(rng, (1, C, H, W)), rand(rng, (1, C, H, W)), rand(rng, (1, oc, oh, ow))
    f1[0, 0] = f16(1e-3) * np.sign(f1[0, 0] + f16(0.5))                  # products around 1e-6: half subnormals
    f2[0, 0] = f16(1e-3)
    g[0, :, 1:3, 2:5] = f16(1e-3)
    f2[0, 1, 2:4, 2:6] = f16(60000.0)                                    # 60000 * 40 overflows; partials to inf
    g[0, :, 3, 3:5] = f16(40.0)
    f2[0, 2, 4:7, 4:7] = f16(30000.0)                                    # +inf and -inf terms in one sum: NaN
    g[0, : oc // 2, 5, 5] = f16(50.0)
    g[0, oc // 2:, 5, 5] = f16(-50.0)
    g[0, 7, 0, 0] = f16(np.inf)                                          # inf at the border: its padding taps give NaN
    want = check(torch_mod, cabi, f1, f2, g, pad, k, md, s2)
    assert any(np.isnan(w).any() for w in want) and any(np.isinf(w).any() for w in want)
    tiny = np.abs(want[0][0, 0]).astype(np.float32)
    assert ((tiny > 0) & (tiny < 6.1e-5)).any()                          # subnormal results survived


def test_half_backward_nelems_rounds_above_2048(torch_mod, cabi):
    """k*k*C = 2049 > 2048: nelems is half(2049) = 2048."""
    rng = np.random.default_rng(13)
    check(torch_mod, cabi, rand(rng, (1, 2049, 4, 5)), rand(rng, (1, 2049, 4, 5)), rand(rng, (1, 81, 4, 5)), 4, 1, 4, 1)
    check(torch_mod, cabi, rand(rng, (1, 229, 4, 5)), rand(rng, (1, 229, 4, 5)), rand(rng, (1, 81, 2, 3), 4.0), 4, 3, 4, 1)


@pytest.mark.parametrize("shape", [(6, 9, 33, 4, 1, 4, 1), (3, 8, 8, 4, 3, 4, 2), (4, 12, 20, 3, 1, 4, 1)])
def test_half_backward_writes_every_element_through_the_module(torch_mod, cabi, shape):
    """NaN-prefilled gradients through correlation_cuda.backward: nothing survives, result as through cabi."""
    torch = torch_mod
    import correlation_cuda
    C, H, W, pad, k, md, s2 = shape
    rng = np.random.default_rng(17)
    oc, oh, ow = out_dims(H, W, pad, k, md, 1, s2)
    f1, f2, g = rand(rng, (2, C, H, W)), rand(rng, (2, C, H, W)), rand(rng, (2, oc, oh, ow))
    a, b, go = h2d(torch, f1), h2d(torch, f2), h2d(torch, g)
    g1 = torch.full((2, C, H, W), float("nan"), dtype=torch.float16, device="cuda")
    g2 = torch.full_like(g1, float("nan"))
    assert correlation_cuda.backward(a, b, a.new_empty(0), a.new_empty(0), go, g1, g2, pad, k, md, 1, s2, 1) == 1
    assert not torch.isnan(g1).any() and not torch.isnan(g2).any()
    c1, c2 = cabi.correlation_backward(a, b, go, pad, k, md, 1, s2)
    assert torch.equal(g1.view(torch.int16), c1.view(torch.int16)) and torch.equal(g2.view(torch.int16), c2.view(torch.int16))
    want = correlation_bwd_half(f1, f2, g, pad, k, md, 1, s2)
    same_bits(g1, want[0]), same_bits(g2, want[1])


def test_half_backward_module_cabi_autograd_agree_and_views(torch_mod, cabi):
    """correlation_cuda.backward, cabi and Correlation(...) autograd on half leaves give the same bits; channel-slice views
    (non-contiguous) give what contiguous copies give."""
    torch = torch_mod
    import correlation_cuda
    from vfidkr_amd.PWCNet.correlation_package_pytorch1_0.correlation import Correlation
    gen = torch.Generator(device="cpu").manual_seed(19)
    big1 = torch.randn(2, 12, 20, 37, generator=gen).half().cuda()
    big2 = torch.randn(2, 12, 20, 37, generator=gen).half().cuda()
    go = torch.randn(2, 81, 20, 37, generator=gen).half().cuda()
    v1, v2 = big1[:, 2:9], big2[:, 3:10]                                      # channel slices: not contiguous
    assert not v1.is_contiguous()
    c1, c2 = cabi.correlation_backward(v1, v2, go, 4, 1, 4, 1, 1)
    d1, d2 = cabi.correlation_backward(v1.contiguous(), v2.contiguous(), go, 4, 1, 4, 1, 1)
    assert torch.equal(c1.view(torch.int16), d1.view(torch.int16)) and torch.equal(c2.view(torch.int16), d2.view(torch.int16))
    m1, m2 = v1.new_empty(0), v1.new_empty(0)
    assert correlation_cuda.backward(v1, v2, v1.new_empty(0), v1.new_empty(0), go, m1, m2, 4, 1, 4, 1, 1, 1) == 1
    assert torch.equal(m1.view(torch.int16), c1.view(torch.int16)) and torch.equal(m2.view(torch.int16), c2.view(torch.int16))
    a = v1.detach().clone().requires_grad_(True)
    b = v2.detach().clone().requires_grad_(True)
    out = Correlation(4, 1, 4, 1, 1, 1)(a, b)
    assert out.dtype == torch.float16
    out.backward(go)
    assert a.grad.dtype == torch.float16 and b.grad.dtype == torch.float16
    assert torch.equal(a.grad.view(torch.int16), c1.view(torch.int16)) and torch.equal(b.grad.view(torch.int16), c2.view(torch.int16))
    same_bits(c1, correlation_bwd_half(v1.cpu().numpy(), v2.cpu().numpy(), go.cpu().numpy())[0])


def test_half_toy_network_trains(torch_mod):
    """A .half() network, conv -> Correlation(4, 1, 4, 1, 1, 1) -> conv -> loss: loss.backward() runs and the conv weights
    get finite gradients."""
    torch = torch_mod
    from vfidkr_amd.PWCNet.correlation_package_pytorch1_0.correlation import Correlation
    torch.manual_seed(23)
    feat = torch.nn.Conv2d(3, 16, 3, padding=1).cuda().half()
    head = torch.nn.Conv2d(81, 2, 3, padding=1).cuda().half()
    corr = Correlation(4, 1, 4, 1, 1, 1)
    x0 = torch.randn(2, 3, 24, 40, device="cuda").half()
    x1 = torch.randn(2, 3, 24, 40, device="cuda").half()
    loss = head(corr(feat(x0), feat(x1))).float().pow(2).mean()
    loss.backward()
    for p in list(feat.parameters()) + list(head.parameters()):
        assert p.grad is not None and p.grad.dtype == torch.float16 and torch.isfinite(p.grad).all()
    assert feat.weight.grad.abs().sum() > 0


def test_half_backward_mixed_dtypes_raise(torch_mod, cabi):
    torch = torch_mod
    import correlation_cuda
    a = torch.randn(1, 4, 8, 10, device="cuda").half()
    b = torch.randn(1, 4, 8, 10, device="cuda").half()
    go = torch.randn(1, 81, 8, 10, device="cuda").half()
    e = a.new_empty(0)
    with pytest.raises(RuntimeError):
        correlation_cuda.backward(a, b.float(), e, e, go, a.new_empty(0), a.new_empty(0), 4, 1, 4, 1, 1, 1)
    with pytest.raises(RuntimeError):
        correlation_cuda.backward(a, b, e, e, go.float(), a.new_empty(0), a.new_empty(0), 4, 1, 4, 1, 1, 1)
    with pytest.raises(RuntimeError):
        correlation_cuda.backward(a, b, e, e, go, a.new_empty(0).float(), a.new_empty(0), 4, 1, 4, 1, 1, 1)
    with pytest.raises(RuntimeError):
        cabi.correlation_backward(a, b.float(), go, 4, 1, 4, 1, 1)
    with pytest.raises(RuntimeError):
        cabi.correlation_backward(a, b, go.float(), 4, 1, 4, 1, 1)
    with pytest.raises(RuntimeError):
        cabi.correlation_backward(a.cpu(), b.cpu(), go.cpu(), 4, 1, 4, 1, 1)


def test_half_backward_graph_capture_replays_bit_identically(torch_mod, cabi):
    """One capture of the half backward on a single stream (no parallel branches); the replay equals the eager call."""
    torch = torch_mod
    gen = torch.Generator(device="cpu").manual_seed(29)
    a = torch.randn(1, 16, 36, 62, generator=gen).half().cuda()
    b = torch.randn(1, 16, 36, 62, generator=gen).half().cuda()
    go = torch.randn(1, 81, 36, 62, generator=gen).half().cuda()
    e1, e2 = cabi.correlation_backward(a, b, go, 4, 1, 4, 1, 1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cabi.correlation_backward(a, b, go, 4, 1, 4, 1, 1)             # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r1, r2 = cabi.correlation_backward(a, b, go, 4, 1, 4, 1, 1)
    r1.fill_(0), r2.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(r1.view(torch.int16), e1.view(torch.int16)) and torch.equal(r2.view(torch.int16), e2.view(torch.int16))
