"""GPU: the PWC-Net warp backward (vfi_pwc_warp_backward) against the numpy restatement of torch autograd of the reference's
warp() (tests/pwc_warp_backward.py) and against torch autograd itself on the GPU, through the C ABI and fused.warp /
fused.warp_corr.  Bounds: grad_x <= 4e-7 A + 2^-40 max|g| (A: the cell's sum of |addends|), grad_flow <= 1e-5 S + 1e-7
(S: the pixel's sum of |terms|)."""
import numpy as np
import pytest

from tests.pwc_warp_backward import FLOW_KINDS, flow_family, pwc_warp_bwd
from tests.test_pwc_warp_backward_host import torch_warp

pytestmark = pytest.mark.gpu

f32 = np.float32


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


def gpu(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).cuda()


def run(torch, cabi, x, flo, g, ac, want_x=True, want_f=True):
    gx = torch.zeros_like(x) if want_x else None
    gf = torch.full_like(flo, float("nan")) if want_f else None           # written: NaN prefill shows a missed pixel
    assert cabi.pwc_warp_backward(x, flo, g, gx, gf, ac) == 0
    torch.cuda.synchronize()
    return gx, gf


def within(got_x, got_f, ref, g):
    gx, gf, A, S, mask = ref
    gx_, gf_ = got_x.cpu().numpy().astype(np.float64), got_f.cpu().numpy().astype(np.float64)
    tol_x = 4e-7 * A + 2.0 ** -40 * float(np.abs(g).max())
    bad = ~(np.abs(gx_ - gx) <= tol_x)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(np.abs(gx_ - gx).max()))
    bad = ~(np.abs(gf_ - gf) <= 1e-5 * S + 1e-7)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(np.nanmax(np.abs(gf_ - gf))))
    off = np.broadcast_to((mask == 0)[:, None], gf_.shape)
    assert (gf_[off] == 0).all()


def case(rng, B, C, h, w, kind, scale=1.0):
    x = rng.normal(size=(B, C, h, w)).astype(f32)
    flo = flow_family(rng, kind, B, h, w)
    g = (rng.normal(size=(B, C, h, w)) * scale).astype(f32)
    return x, flo, g


def _random_cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        out.append((int(rng.integers(1, 4)), (1, 3, 8, 9, 32, 196)[i % 6], int(rng.integers(1, 101)),
                    int(rng.integers(1, 101)), FLOW_KINDS[i % len(FLOW_KINDS)], bool(i % 2), int(rng.integers(1 << 30))))
    return out


RANDOM = _random_cases(24, 715)


@pytest.mark.parametrize("c", RANDOM, ids=lambda c: "B%dC%d_%dx%d_%s_ac%d" % (c[:5] + (int(c[5]),)))
def test_cabi_against_restatement(torch_mod, cabi, c):
    torch = torch_mod
    B, C, h, w, kind, ac, seed = c
    x, flo, g = case(np.random.default_rng(seed), B, C, h, w, kind)
    gx, gf = run(torch, cabi, gpu(torch, x), gpu(torch, flo), gpu(torch, g), ac)
    within(gx, gf, pwc_warp_bwd(x, flo, g, ac), g)


# the four warped levels of the 1080p pyramid (padded 1152 x 1984: synthetic.correlation_features) and the Vimeo
# training shape (B = 3, 256 x 448: levels 64 x 112 ... 8 x 14)
LEVELS = [(1, 32, 288, 496), (1, 64, 144, 248), (1, 96, 72, 124), (1, 128, 36, 62),
          (3, 32, 64, 112), (3, 64, 32, 56), (3, 96, 16, 28), (3, 128, 8, 14)]


@pytest.mark.parametrize("lv", LEVELS, ids=lambda v: "B%dC%d_%dx%d" % v)
def test_pyramid_levels(torch_mod, cabi, lv):
    torch = torch_mod
    B, C, h, w = lv
    rng = np.random.default_rng(C * h)
    x, flo, g = case(rng, B, C, h, w, "3")
    for ac in (True, False):
        gx, gf = run(torch, cabi, gpu(torch, x), gpu(torch, flo), gpu(torch, g), ac)
        within(gx, gf, pwc_warp_bwd(x, flo, g, ac), g)


def torch_gpu_grads(torch, x, flo, g, ac):
    xt = gpu(torch, x).requires_grad_(True)
    ft = gpu(torch, flo).requires_grad_(True)
    torch_warp(xt, ft, ac).backward(gpu(torch, g))
    return xt.grad, ft.grad


# torch's float32 coordinates are not ours operation for operation (a division by a scalar runs as a multiply by its
# reciprocal): an ulp of ix at x ~ 200 moves a weight by 1.5e-5.  So the shapes here have h - 1, w - 1 powers of two and
# the flows are dyadic: every float32 coordinate is exact in both, and only the summation order differs.
TORCH = [(2, 8, 33, 65, "dyadic", True), (1, 32, 129, 257, "dyadic", True), (3, 64, 33, 65, "int", True),
         (2, 9, 17, 33, "border", True), (2, 8, 33, 65, "dyadic", False), (1, 32, 129, 257, "dyadic", False),
         (3, 9, 9, 17, "int", False), (2, 196, 17, 33, "border", False)]


@pytest.mark.parametrize("c", TORCH, ids=lambda c: "B%dC%d_%dx%d_%s_ac%d" % (c[:5] + (int(c[5]),)))
def test_against_torch_autograd_on_the_gpu(torch_mod, cabi, c):
    torch = torch_mod
    B, C, h, w, kind, ac = c
    rng = np.random.default_rng(B * C * h)
    x, flo, g = case(rng, B, C, h, w, kind)
    if kind == "border":
        flo = (np.round(flo * 16) / 16).astype(f32)
    tx, tf = torch_gpu_grads(torch, x, flo, g, ac)
    gx, gf = run(torch, cabi, gpu(torch, x), gpu(torch, flo), gpu(torch, g), ac)
    _, _, A, S, _ = pwc_warp_bwd(x, flo, g, ac)
    d = np.abs(gx.cpu().numpy().astype(np.float64) - tx.cpu().numpy())
    assert (d <= 4e-7 * A + 2.0 ** -40 * np.abs(g).max() + 2.0 ** -40).all(), float(d.max())
    d = np.abs(gf.cpu().numpy().astype(np.float64) - tf.cpu().numpy())
    assert (d <= 1e-5 * S + 1e-7).all(), float(d.max())


def test_strided_views(torch_mod, cabi):
    torch = torch_mod
    rng = np.random.default_rng(5)
    B, C, h, w = 2, 9, 37, 70
    big = rng.normal(size=(B, C + 5, h, w)).astype(f32)
    x_np = big[:, 2:2 + C]
    flo = flow_family(rng, "3", B, h, w)
    g_np = rng.normal(size=(B, C, h, w)).astype(f32)
    x = gpu(torch, big)[:, 2:2 + C]                                        # channel slice
    g = gpu(torch, np.ascontiguousarray(g_np.transpose(1, 0, 2, 3))).permute(1, 0, 2, 3)   # non-contiguous
    gxb = torch.zeros((B, C + 3, h, w + 8), device="cuda")
    gx = gxb[:, 1:1 + C, :, 3:3 + w]                                     # strides of its own
    gfb = torch.zeros((2, B, h, w + 4), device="cuda")
    gf = gfb.permute(1, 0, 2, 3)[:, :, :, :w]
    fl = gpu(torch, flo)
    assert cabi.pwc_warp_backward(x, fl, g, gx, gf, True) == 0
    torch.cuda.synchronize()
    within(gx, gf, pwc_warp_bwd(x_np, flo, g_np, True), g_np)
    gx2, gf2 = run(torch, cabi, gpu(torch, x_np), fl, gpu(torch, g_np), True)
    assert torch.equal(gx, gx2) and torch.equal(gf, gf2)
    assert gxb[:, 0].abs().sum() == 0 and gxb[:, 1 + C:].abs().sum() == 0 and gxb[..., :3].abs().sum() == 0


def test_determinism(torch_mod, cabi):
    torch = torch_mod
    rng = np.random.default_rng(8)
    for B, C, h, w, kind in ((1, 32, 136, 248, "3"), (3, 128, 8, 14, "0.5"), (2, 196, 18, 31, "20")):
        x, flo, g = (gpu(torch, a) for a in case(rng, B, C, h, w, kind))
        a = run(torch, cabi, x, flo, g, True)
        b = run(torch, cabi, x, flo, g, True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            c = run(torch, cabi, x, flo, g, True)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
        only_x, _ = run(torch, cabi, x, flo, g, True, want_f=False)
        _, only_f = run(torch, cabi, x, flo, g, True, want_x=False)
        assert torch.equal(a[0], only_x) and torch.equal(a[1], only_f)


def test_far_flows_give_zero_gradients(torch_mod, cabi):
    torch = torch_mod
    rng = np.random.default_rng(9)
    x, _, g = case(rng, 2, 8, 20, 30, "zero")
    flo = np.full((2, 2, 20, 30), 1e4, f32)
    gx, gf = run(torch, cabi, gpu(torch, x), gpu(torch, flo), gpu(torch, g), True)
    assert (gx == 0).all() and (gf == 0).all()


def test_inf_gradient_takes_the_fp32_path(torch_mod, cabi):
    torch = torch_mod
    rng = np.random.default_rng(10)
    B, C, h, w = 1, 3, 17, 33                              # exact coordinates (see TORCH)
    x, flo, g = case(rng, B, C, h, w, "dyadic")
    g[0, 1, 5, 7] = np.inf
    gx, gf = run(torch, cabi, gpu(torch, x), gpu(torch, flo), gpu(torch, g), True)
    tx, tf = torch_gpu_grads(torch, x, flo, g, True)
    gxn, txn = gx.cpu().numpy(), tx.cpu().numpy()
    assert np.array_equal(~np.isfinite(gxn), ~np.isfinite(txn))
    assert np.array_equal(~np.isfinite(gf.cpu().numpy()), ~np.isfinite(tf.cpu().numpy()))
    assert (~np.isfinite(gxn)).sum() >= 1
    fin = np.isfinite(txn)
    _, _, A, _, _ = pwc_warp_bwd(x, flo, np.where(np.isfinite(g), g, 0).astype(f32), True)
    assert (np.abs(gxn[fin] - txn[fin]) <= 4e-7 * A[fin] + 1e-6).all()


def test_bad_shapes(torch_mod, cabi):
    torch = torch_mod
    x = torch.zeros((1, 3, 8, 8), device="cuda")
    fl = torch.zeros((1, 2, 8, 8), device="cuda")
    g = torch.zeros_like(x)
    assert cabi.pwc_warp_backward(x, torch.zeros((1, 3, 8, 8), device="cuda"), g, torch.zeros_like(x), None) == 1
    assert cabi.pwc_warp_backward(x, fl, torch.zeros((1, 3, 8, 9), device="cuda"), torch.zeros_like(x), None) == 1
    assert cabi.pwc_warp_backward(x, fl, g, torch.zeros((1, 3, 8, 9), device="cuda"), None) == 1
    assert cabi.pwc_warp_backward(x, fl, g, None, torch.zeros((1, 2, 8, 9), device="cuda")) == 1
    assert cabi.pwc_warp_backward(x, fl, g.transpose(2, 3), torch.zeros_like(x), None) == 1         # w stride != 1


# ------------------------------------------------------------------ autograd

def test_fused_warp_autograd(torch_mod, cabi, fused):
    torch = torch_mod
    rng = np.random.default_rng(11)
    x_np, flo_np, g_np = case(rng, 2, 32, 40, 60, "3")
    for ac in (True, False):
        x = gpu(torch, x_np).requires_grad_(True)
        fl = gpu(torch, flo_np).requires_grad_(True)
        out = fused.warp(x, fl, ac)
        assert out.grad_fn is not None
        out.backward(gpu(torch, g_np))
        gx, gf = run(torch, cabi, gpu(torch, x_np), gpu(torch, flo_np), gpu(torch, g_np), ac)
        assert torch.equal(x.grad, gx) and torch.equal(fl.grad, gf)
        with torch.no_grad():
            plain = fused.warp(x, fl, ac)
        assert plain.grad_fn is None
        ref = torch.empty_like(plain)
        assert cabi.pwc_warp_forward(gpu(torch, x_np), gpu(torch, flo_np), ref, ac) == 0
        assert torch.equal(plain, ref) and torch.equal(out.detach(), ref)
    # only the flow requires grad: x's gradient is not computed
    fl = gpu(torch, flo_np).requires_grad_(True)
    fused.warp(gpu(torch, x_np), fl).sum().backward()
    _, gf = run(torch, cabi, gpu(torch, x_np), gpu(torch, flo_np), torch.ones((2, 32, 40, 60), device="cuda"), True,
                want_x=False)
    assert torch.equal(fl.grad, gf)


def test_fused_warp_corr_autograd(torch_mod, cabi, fused):
    torch = torch_mod
    rng = np.random.default_rng(12)
    B, C, h, w = 2, 32, 36, 62
    c1_np, c2_np = (rng.normal(size=(B, C, h, w)).astype(f32) for _ in range(2))
    flo_np = flow_family(rng, "3", B, h, w)
    g = gpu(torch, rng.normal(size=(B, 81, h, w)).astype(f32))
    warped = torch.empty((B, C, h, w), device="cuda")
    assert cabi.pwc_warp_forward(gpu(torch, c2_np), gpu(torch, flo_np), warped, True) == 0
    g1, gw = cabi.correlation_backward(gpu(torch, c1_np), warped, g, 4, 1, 4, 1, 1)
    g2, gf = run(torch, cabi, gpu(torch, c2_np), gpu(torch, flo_np), gw, True)
    for one_launch in (False, True):
        c1, c2, fl = (gpu(torch, a).requires_grad_(True) for a in (c1_np, c2_np, flo_np))
        out = fused.warp_corr(c1, c2, fl, True, one_launch=one_launch)
        with torch.no_grad():
            plain = fused.warp_corr(c1, c2, fl, True, one_launch=one_launch)
        assert torch.equal(out.detach(), plain)
        out.backward(g)
        assert torch.equal(c1.grad, g1) and torch.equal(c2.grad, g2) and torch.equal(fl.grad, gf)


def test_training_loop_is_reproducible(torch_mod, fused):
    torch = torch_mod
    rng = np.random.default_rng(13)
    c1_np, c2_np = (rng.normal(size=(2, 64, 32, 56)).astype(f32) for _ in range(2))
    flo_np = flow_family(rng, "3", 2, 32, 56)
    results = []
    for _ in range(3):                                  # forward, loss, backward: the same bits every time
        wgt = torch.linspace(0.5, 1.5, 64, device="cuda").view(1, 64, 1, 1).requires_grad_(True)
        c1, c2, fl = (gpu(torch, a).requires_grad_(True) for a in (c1_np, c2_np, flo_np))
        corr = torch.nn.functional.leaky_relu(fused.warp_corr(c1, c2 * wgt, fl), 0.1)
        loss = (corr ** 2).mean() + fused.warp(c1, fl).abs().mean()
        loss.backward()
        results.append([t.detach().clone() for t in (loss, c1.grad, c2.grad, fl.grad, wgt.grad)])
    for r in results[1:]:
        for a, b in zip(results[0], r):
            assert torch.equal(a, b)
