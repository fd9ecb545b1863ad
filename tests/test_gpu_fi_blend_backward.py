"""GPU: the FilterInterpolate blend backward (vfi_filterinterp_blend_backward, fused.FilterInterpolate) and the FlowProject
autograd Function (fused.FlowProject / FlowProject_directions).

The blend backward must equal, bit for bit, torch forming g_d = grad_blend * w_d + grad_out_d followed by
vfi_filterinterp_backward_ori per direction on zero-filled outputs; against the CPU oracle the flow and filter gradients
are exact and the image gradient is within the existing backward tolerance (tests/test_gpu_backward.py)."""
import itertools

import numpy as np
import pytest

from tests.test_gpu_backward import assert_image_grad, grad_exponent, make_flow

pytestmark = pytest.mark.gpu

f32 = np.float32
WEIGHTS = [(0.5, 0.5), (0.75, 0.25), (1.0, 0.0)]


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


def make_case(torch, seed, B, C, H, W, fc, model="mixed"):
    rng = np.random.default_rng(seed)
    refs = [gpu(torch, rng.standard_normal((B, C, H, W))) for _ in range(2)]
    flows = [gpu(torch, make_flow(rng, model if d == 0 else "invalid", B, H, W)) for d in range(2)]
    filts = [gpu(torch, rng.random((B, fc, H, W), dtype=f32)) for _ in range(2)]
    grads = [gpu(torch, rng.standard_normal((B, C, H, W))) for _ in range(3)]
    return refs, flows, filts, grads


def composed(torch, cabi, refs, flows, filts, gb, g0, g2, w0, w2):
    """torch forms g_d, then vfi_filterinterp_backward_ori per direction on zero-filled outputs"""
    out = []
    for d, (go, wd) in enumerate(((g0, w0), (g2, w2))):
        terms = ([gb * wd] if gb is not None else []) + ([go] if go is not None else [])
        r, f, k = refs[d], flows[d], filts[d]
        if not terms:
            out.append([torch.zeros_like(r), torch.zeros_like(f), torch.zeros_like(k)])
            continue
        g = terms[0] + terms[1] if len(terms) == 2 else terms[0].contiguous()
        gr, gf, gk = torch.zeros_like(r), torch.zeros_like(f), torch.zeros_like(k)
        assert cabi.filterinterp_backward_ori(r, f, k, g, gr, gf, gk) == 0
        out.append([gr, gf, gk])
    torch.cuda.synchronize()
    return out


def fused_bwd(torch, cabi, refs, flows, filts, gb, g0, g2, w0, w2, want=(True,) * 6, prefill=float("nan")):
    like = [refs[0], refs[1], flows[0], flows[1], filts[0], filts[1]]
    outs = [torch.empty_strided(t.shape, t.stride(), device=t.device).fill_(prefill) if wt else None
            for t, wt in zip(like, want)]
    assert cabi.filterinterp_blend_backward(refs[0], refs[1], flows[0], flows[1], filts[0], filts[1], gb, g0, g2, w0, w2,
                                            *outs) == 0
    torch.cuda.synchronize()
    return outs


def assert_same(a, b, what=""):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(a, b, equal_nan=True), "%s: %d cells differ, max %g" % (
        what, int((a != b).sum()), float(np.nanmax(np.abs(a - b))))


def check_parity(torch, cabi, refs, flows, filts, gb, g0, g2, w0, w2, want=(True,) * 6):
    got = fused_bwd(torch, cabi, refs, flows, filts, gb, g0, g2, w0, w2, want)
    ref = composed(torch, cabi, refs, flows, filts, gb, g0, g2, w0, w2)
    order = [ref[0][0], ref[1][0], ref[0][1], ref[1][1], ref[0][2], ref[1][2]]
    names = ["grad_ref0", "grad_ref2", "grad_flow0", "grad_flow2", "grad_filt0", "grad_filt2"]
    for g, r, n, wt in zip(got, order, names, want):
        if wt:
            assert_same(g, r, n)
        else:
            assert g is None
    return got


# ------------------------------------------------------------------ 1. bit parity with the composition

def test_parity_random_shapes(torch_mod, cabi):
    torch = torch_mod
    rng = np.random.default_rng(2024)
    for i in range(24):
        B = int(rng.integers(1, 4))
        C = int(rng.choice([1, 3, 4, 17]))
        H = int(rng.choice([1, 5, 8, 17, 33]))
        W = int(rng.choice([1, 7, 64, 65, 130]))
        fc = int(rng.choice([4, 16, 36]))
        model = str(rng.choice(["smooth", "mixed", "invalid", "border", "subpixel"]))
        w0, w2 = WEIGHTS[i % 3]
        refs, flows, filts, (gb, g0, g2) = make_case(torch, 100 + i, B, C, H, W, fc, model)
        check_parity(torch, cabi, refs, flows, filts, gb, g0, g2, w0, w2)


def test_parity_every_null_pattern(torch_mod, cabi):
    torch = torch_mod
    refs, flows, filts, (gb, g0, g2) = make_case(torch, 5, 2, 3, 19, 70, 16)
    for k, present in enumerate(itertools.product([True, False], repeat=3)):
        terms = [t if p else None for t, p in zip((gb, g0, g2), present)]
        w0, w2 = WEIGHTS[k % 3]
        check_parity(torch, cabi, refs, flows, filts, *terms, w0, w2)
    for want in itertools.product([True, False], repeat=6):
        if any(want):
            check_parity(torch, cabi, refs, flows, filts, gb, g0, g2, 0.75, 0.25, want)
    # a filter size off the staged path, with the image gradient in one direction only
    refs, flows, filts, (gb, g0, g2) = make_case(torch, 6, 1, 4, 9, 66, 36)
    check_parity(torch, cabi, refs, flows, filts, gb, g0, None, 0.5, 0.5, (False, True, True, False, True, True))
    # a filter count that is not a square (fs = 4, 20 channels): every channel of the filter gradients is written
    refs, flows, filts, (gb, g0, g2) = make_case(torch, 7, 2, 3, 17, 65, 20)
    check_parity(torch, cabi, refs, flows, filts, gb, g0, g2, 0.75, 0.25)


# ------------------------------------------------------------------ 2. oracle

@pytest.mark.parametrize("fc,model", [(16, "mixed"), (16, "border"), (36, "smooth"), (4, "invalid")])
def test_against_the_oracle(torch_mod, cabi, oracle, np_oracle, fc, model):
    torch = torch_mod
    B, C, H, W = 2, 3, 21, 77
    refs, flows, filts, (gb, g0, g2) = make_case(torch, 11, B, C, H, W, fc, model)
    w0, w2 = 0.75, 0.25
    got = fused_bwd(torch, cabi, refs, flows, filts, gb, g0, g2, w0, w2)
    for d, (go, wd) in enumerate(((g0, w0), (g2, w2))):
        g = (gb * wd + go).cpu().numpy()
        img, flow, filt = refs[d].cpu().numpy(), flows[d].cpu().numpy(), filts[d].cpu().numpy()
        r_img, r_flow, r_filt = oracle.filterinterp_ori_bwd(img, flow, filt, g, fmad=1)
        assert np.array_equal(got[2 + d].cpu().numpy(), r_flow)
        assert np.array_equal(got[4 + d].cpu().numpy(), r_filt)
        stats = np_oracle.filterinterp_ori_bwd_img(flow, filt, g)
        assert_image_grad(got[d].cpu().numpy(), np.zeros_like(img), stats, grad_exponent(g, filt, H, W, fc), "ori")


# ------------------------------------------------------------------ 3-6. target shapes, strided views, determinism, non-finite

@pytest.mark.parametrize("B,H,W", [(3, 256, 448), (1, 1152, 1984)])
def test_target_shapes(torch_mod, cabi, B, H, W):
    torch = torch_mod
    refs, flows, filts, (gb, g0, g2) = make_case(torch, 21, B, 3, H, W, 16, "smooth")
    check_parity(torch, cabi, refs, flows, filts, gb, g0, g2, 0.5, 0.5)
    check_parity(torch, cabi, refs, flows, filts, gb, g0, g2, 0.5, 0.5, (False, False, True, True, True, True))


def test_strided_views_equal_contiguous_copies(torch_mod, cabi):
    torch = torch_mod
    refs, flows, filts, (gb, g0, g2) = make_case(torch, 31, 2, 3, 24, 70, 16)
    big = [torch.randn((2, 7, 24, 70), device="cuda") for _ in range(5)]
    for t in big:
        t[:, 2:5] = 0
    views = [b[:, 2:5] for b in big]
    for v, src in zip(views, (refs[0], refs[1], gb, g0, g2)):
        v.copy_(src)
    vrefs, (vgb, vg0, vg2) = views[:2], views[2:]
    got = fused_bwd(torch, cabi, vrefs, flows, filts, vgb, vg0, vg2, 0.75, 0.25)
    want = fused_bwd(torch, cabi, refs, flows, filts, gb, g0, g2, 0.75, 0.25)
    for a, b in zip(got, want):
        assert_same(a, b, "strided")


def test_deterministic_and_overwrites(torch_mod, cabi):
    torch = torch_mod
    refs, flows, filts, (gb, g0, g2) = make_case(torch, 41, 3, 4, 40, 130, 16, "mixed")
    a = fused_bwd(torch, cabi, refs, flows, filts, gb, g0, g2, 0.5, 0.5, prefill=float("nan"))
    b = fused_bwd(torch, cabi, refs, flows, filts, gb, g0, g2, 0.5, 0.5, prefill=123.0)
    for x, y in zip(a, b):
        assert not torch.isnan(x).any()
        assert_same(x, y, "run to run")


def test_shared_scratch_between_layouts(torch_mod, cabi):
    """Calls that lay the shared gradient scratch out differently, back to back on one stream, each give the bits of the
    same call made alone on fresh workspaces: two directions + flags (two tiles across, the second ragged), one smaller
    direction (interpolation_backward), flags only, then the first again."""
    torch = torch_mod
    refs, flows, filts, (gb, g0, g2) = make_case(torch, 81, 1, 2, 9, 65, 16)
    rng = np.random.default_rng(82)
    img, gout = (gpu(torch, rng.standard_normal((1, 1, 5, 64))) for _ in range(2))
    flow = gpu(torch, make_flow(rng, "subpixel", 1, 5, 64))

    def blend(want):
        return [o for o in fused_bwd(torch, cabi, refs, flows, filts, gb, g0, g2, 0.75, 0.25, want) if o is not None]

    def interp():
        g1, g2_ = torch.zeros_like(img), torch.zeros_like(flow)
        assert cabi.interpolation_backward(img, flow, gout, g1, g2_) == 0
        torch.cuda.synchronize()
        return [g1, g2_]

    calls = [lambda: blend((True,) * 6), interp, lambda: blend((False, False, True, True, True, True)),
             lambda: blend((True,) * 6)]
    alone = []
    for call in calls:
        assert cabi.release_workspaces() == 0
        alone.append(call())
    assert cabi.release_workspaces() == 0
    for i, (call, want) in enumerate(zip(calls, alone)):
        for a, b in zip(call(), want):
            assert_same(a, b, "call %d after the others" % i)


def test_non_finite_grad_blend(torch_mod, cabi):
    torch = torch_mod
    refs, flows, filts, (gb, g0, g2) = make_case(torch, 51, 1, 3, 30, 70, 16, "smooth")
    gb = gb.clone()
    gb[0, 0, 3, 5] = float("inf")
    gb[0, 1, 20, 40] = float("nan")
    gb[0, 2, 11, 11] = -float("inf")
    got = fused_bwd(torch, cabi, refs, flows, filts, gb, g0, g2, 0.75, 0.25)
    ref = composed(torch, cabi, refs, flows, filts, gb, g0, g2, 0.75, 0.25)
    order = [ref[0][0], ref[1][0], ref[0][1], ref[1][1], ref[0][2], ref[1][2]]
    for g, r in zip(got, order):
        g, r = g.cpu().numpy(), r.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(np.isinf(g), np.isinf(r))
        assert np.array_equal(np.sign(g[np.isinf(r)]), np.sign(r[np.isinf(r)]))
        fin = np.isfinite(r)
        assert np.abs(g[fin] - r[fin]).max() <= 1e-5 * max(1.0, np.abs(r[fin]).max())


# ------------------------------------------------------------------ 7. fused.FilterInterpolate autograd

def _module_graph(torch, refs, offs, filts, t):
    from vfidkr_amd.my_package.FilterInterpolation import FilterInterpolationModule
    o0 = FilterInterpolationModule()(refs[0], offs[0], filts[0])
    o2 = FilterInterpolationModule()(refs[1], offs[1], filts[1])
    return o0 * (1.0 - t) + o2 * t, o0, o2


@pytest.mark.parametrize("ref_grad", [False, True])
def test_filter_interpolate_autograd(torch_mod, fused, ref_grad):
    torch = torch_mod
    t = 0.5
    refs, flows, filts, (ga, gb_, gc) = make_case(torch, 61, 3, 3, 64, 96, 16, "smooth")
    with torch.no_grad():
        plain = fused.FilterInterpolate(refs[0], refs[1], flows, filts, 16, t)
    assert all(x.grad_fn is None for x in plain)
    results = []
    for path in ("fused", "module"):
        leaves = [x.clone().requires_grad_() for x in flows + filts] + [x.clone().requires_grad_(ref_grad) for x in refs]
        offs, fl, rf = leaves[:2], leaves[2:4], leaves[4:]
        if path == "fused":
            blend, o0, o2 = fused.FilterInterpolate(rf[0], rf[1], offs, fl, 16, t)
            assert blend.grad_fn is not None and o0.grad_fn is not None
            for a, b in zip((blend, o0, o2), plain):
                assert_same(a.detach(), b, "forward")
        else:
            blend, o0, o2 = _module_graph(torch, rf, offs, fl, t)
        loss = (blend * ga).sum() + (o0 * gb_).sum() + (o2 * gc).abs().sum()
        loss.backward()
        results.append([x.grad for x in leaves if x.requires_grad])
    for a, b in zip(*results):
        assert_same(a, b, "autograd")
    # an output left out of the loss is an absent term
    leaves = [x.clone().requires_grad_() for x in flows + filts]
    fused.FilterInterpolate(refs[0], refs[1], leaves[:2], leaves[2:], 16, 0.25)[0].sum().backward()
    lm = [x.clone().requires_grad_() for x in flows + filts]
    _module_graph(torch, refs, lm[:2], lm[2:], 0.25)[0].sum().backward()
    for a, b in zip(leaves, lm):
        assert_same(a.grad, b.grad, "blend only")


# ------------------------------------------------------------------ 8. fused.FlowProject autograd

@pytest.mark.parametrize("depth_mode", [None, "per_item", "shared"])
def test_flow_project_autograd(torch_mod, fused, depth_mode):
    torch = torch_mod
    from vfidkr_amd.my_package.FlowProjection import FlowProjectionModule
    from vfidkr_amd.my_package.DepthFlowProjection import DepthFlowProjectionModule
    rng = np.random.default_rng(71)
    B, H, W = 2, 48, 80
    flows = [gpu(torch, make_flow(rng, "smooth", B, H, W) * 3.0) for _ in range(2)]
    depths = [gpu(torch, rng.uniform(0.1, 1.0, (B, 1, H, W))) for _ in range(2)]
    gouts = [gpu(torch, rng.standard_normal((B, 2, H, W))) for _ in range(2)]
    results = []
    for path in ("fused", "module"):
        fl = [f.clone().requires_grad_() for f in flows]
        dp = None
        if depth_mode == "per_item":
            dp = [d.clone().requires_grad_() for d in depths]
        elif depth_mode == "shared":
            shared = depths[0].clone().requires_grad_()
            dp = [shared, shared]
        if path == "fused":
            outs = fused.FlowProject(fl, dp, fillhole=False)
            assert all(o.grad_fn is not None for o in outs)
        elif dp is None:
            outs = [FlowProjectionModule(True)(f) for f in fl]
        else:
            outs = [DepthFlowProjectionModule(True)(f, d) for f, d in zip(fl, dp)]
        sum((o * g).sum() for o, g in zip(outs, gouts)).backward()
        leaves = fl + ([] if dp is None else ([dp[0]] if depth_mode == "shared" else dp))
        results.append([x.grad for x in leaves])
    for a, b in zip(*results):
        assert_same(a, b, "FlowProject")
    # FlowProject_directions inherits it (direction 0's depth shared by its items)
    fl = [f.clone().requires_grad_() for f in flows]
    dinv = None if depth_mode is None else [dp_ for dp_ in (depths[0].clone().requires_grad_(), depths[1])]
    outs = fused.FlowProject_directions([[fl[0]], [fl[1]]], dinv, fillhole=False)
    assert outs[0][0].grad_fn is not None
    (outs[0][0] * gouts[0]).sum().backward()
    assert fl[1].grad is None
    fm = flows[0].clone().requires_grad_()
    dm = None if dinv is None else depths[0].clone().requires_grad_()
    om = FlowProjectionModule(True)(fm) if dm is None else DepthFlowProjectionModule(True)(fm, dm)
    (om * gouts[0]).sum().backward()
    assert_same(fl[0].grad, fm.grad, "directions")
    if dm is not None:
        assert_same(dinv[0].grad, dm.grad, "directions depth")


# ------------------------------------------------------------------ 9. training

def _train(torch, fused, use_fused, steps=30):
    from vfidkr_amd.my_package.FilterInterpolation import FilterInterpolationModule
    from vfidkr_amd.my_package.FlowProjection import FlowProjectionModule
    torch.manual_seed(0)
    B, H, W = 2, 32, 48
    g = torch.Generator().manual_seed(3)
    base = torch.rand((B, 3, H, W + 4), generator=g)
    frame0, frame2 = base[..., :W].cuda(), base[..., 4:].cuda()       # a pair translated by four pixels
    target = base[..., 2:W + 2].cuda()
    # 3x3 convolutions written as unfold + matmul: a library convolution's backward may pick its algorithm per call and
    # sum with atomics, which would make two identical loops drift apart for reasons outside the synthesis
    params = []
    for cout in (4, 32):
        wgt = (torch.randn((cout, 6 * 9), generator=g) * 0.01).cuda().requires_grad_()
        bias = torch.zeros((cout, 1), device="cuda", requires_grad=True)
        params += [wgt, bias]

    def conv(x, wgt, bias):
        return (wgt @ torch.nn.functional.unfold(x, 3, padding=1) + bias).view(B, -1, H, W)

    opt = torch.optim.SGD(params, lr=0.5)
    losses = []
    x = torch.cat([frame0, frame2], 1)
    for _ in range(steps):
        opt.zero_grad()
        fl = conv(x, *params[:2]) * 4.0
        kf = torch.softmax(conv(x, *params[2:]).view(B, 2, 16, H, W), 2)
        f0, f2 = fl[:, :2].contiguous(), fl[:, 2:].contiguous()
        k0, k2 = kf[:, 0].contiguous(), kf[:, 1].contiguous()
        if use_fused:
            p0, p2 = fused.FlowProject([f0, f2], None, fillhole=False)
            blend, o0, o2 = fused.FilterInterpolate(frame0, frame2, [p0, p2], [k0, k2], 16, 0.5)
        else:
            p0, p2 = FlowProjectionModule(True)(f0), FlowProjectionModule(True)(f2)
            o0 = FilterInterpolationModule()(frame0, p0, k0)
            o2 = FilterInterpolationModule()(frame2, p2, k2)
            blend = o0 / 2.0 + o2 / 2.0
        loss = (blend - target).abs().mean() + 0.1 * ((o0 - target).abs().mean() + (o2 - target).abs().mean())
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses


def test_training_through_the_fused_synthesis(torch_mod, fused):
    torch = torch_mod
    a = _train(torch, fused, True)
    b = _train(torch, fused, False)
    assert b == _train(torch, fused, False)                 # (the loop itself is reproducible)
    assert a == b, (a[:5], b[:5])
    assert a[-1] < a[0]
