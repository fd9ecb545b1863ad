"""The LDS-staged backward kernels through every tile class of tests/bwd_tiles.py (empty tiles, three / two / one channel
per pass and a short last pass, windows that do not fit, deformable tap positions that are far, cell boxes over budget
while the window fits, boxes at each frame edge, ragged right and bottom tiles), at C in {1, 2, 3, 4, 5, 7} (16 for the
warp kernel's channel groups), each from a non-zero starting image gradient where the kernels add into it.

  * image gradient: bit-equal to bwd_tiles.predict_image_grad (exact integer sums of the rounded fp32 addends, converted
    once); a mismatch names the classes of the tiles that scatter into the failing cells.  Independently within the
    float64 bound of tests/test_gpu_backward.assert_image_grad;
  * flow, filter and offset gradients: bit-equal to the C oracle at fmad=1 (the warp kernel's flow gradient: within the
    float64 restatement's tolerance, as tests/test_gpu_pwc_warp_backward.py checks it);
  * blend outputs are written into interior views of NaN-filled buffers: every pixel of the view written, nothing outside;
  * a second call gives the same bits;
  * call-level classes: tiny gradients (k > 126: the second scale factor, every tile to the per-tap path) bit-equal to the
    restatement; a non-finite gradient puts NaN / Inf where the oracle does.
"""
import functools

import numpy as np
import pytest

from tests import bwd_tiles as bt
from tests.test_gpu_backward import assert_image_grad
from tests.test_gpu_parity import GRAD_TOL, cpu, gpu, torch_mod, cabi  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

f32 = np.float32
B, H, W = 2, 123, 360
CS = (1, 2, 3, 4, 5, 7)
CMAX = 7


@functools.lru_cache(maxsize=None)
def case(kernel, variant=0, cmax=CMAX):
    """(flow, off, img, filt, gout, g0) of a kernel's field; gout's largest |element| is pinned in channel 0 so that every
    C <= cmax shares one scale exponent (the integer sums of the first C channels are then those of the full call)"""
    rng = np.random.default_rng(500 + 10 * bt.KERNELS.index(kernel) + variant)
    flow, off = bt.build_field(kernel, rng, B, H, W)
    img = rng.random((B, cmax, H, W), dtype=f32)
    filt = rng.random((B, 16, H, W), dtype=f32)
    gout = np.clip(rng.standard_normal((B, cmax, H, W)), -3, 3).astype(f32)
    gout[:, 0, 0, 0] = f32(3.5)
    g0 = rng.standard_normal((B, cmax, H, W)).astype(f32)
    return flow, off, img, filt, gout, g0


@functools.lru_cache(maxsize=None)
def predicted_sums(kernel, variant=0, cmax=CMAX):
    flow, off, img, filt, gout, g0 = case(kernel, variant, cmax)
    weights = filt if kernel == "ori" or (kernel == "defor" and variant != 2) else None
    k, fp32, scale, scale2 = bt.grad_scale(gout, weights, H, W, bt.taps_of(kernel))
    assert not fp32
    return bt.integer_sums(kernel, flow, gout, (scale, scale2), filt, off, variant), k


def assert_bits(got, want, recs, kernel, what="image gradient"):
    if np.array_equal(got, want, equal_nan=True):
        return
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    raise AssertionError("%s %s: %s" % (kernel, what, bt.name_cells(recs, kernel, [tuple(i) for i in bad], H, W)))


def run(torch, cabi, kernel, variant, img, flow, filt, off, gout, g0):
    """one call; the image gradient from g0, the others from zero.  numpy (gimg, gflow, gfilt or None, goff or None)"""
    g1 = gpu(torch, g0)
    g2 = torch.zeros((B, 2, H, W), device="cuda:0")
    if kernel == "interp":
        assert cabi.interpolation_backward(gpu(torch, img), gpu(torch, flow), gpu(torch, gout), g1, g2) == 0
        return cpu(g1), cpu(g2), None, None
    if kernel == "ori":
        g3 = torch.zeros(filt.shape, device="cuda:0")
        assert cabi.filterinterp_backward_ori(gpu(torch, img), gpu(torch, flow), gpu(torch, filt), gpu(torch, gout),
                                              g1, g2, g3) == 0
        return cpu(g1), cpu(g2), cpu(g3), None
    go = torch.zeros(off.shape, device="cuda:0")
    if variant == 2:
        assert cabi.filterinterp_backward_defor(2, gpu(torch, img), gpu(torch, flow), gpu(torch, off), None,
                                                gpu(torch, gout), g1, g2, go, None) == 0
        return cpu(g1), cpu(g2), None, cpu(go)
    gf = torch.zeros(filt.shape, device="cuda:0")
    assert cabi.filterinterp_backward_defor(variant, gpu(torch, img), gpu(torch, flow), gpu(torch, filt), gpu(torch, off),
                                            gpu(torch, gout), g1, g2, gf, go) == 0
    return cpu(g1), cpu(g2), cpu(gf), cpu(go)


def oracle_bwd(oracle, kernel, variant, img, flow, filt, off, gout):
    if kernel == "interp":
        r1, r2 = oracle.interp_bwd(img, flow, gout, fmad=1)
        return r1, r2, None, None
    if kernel == "ori":
        return oracle.filterinterp_ori_bwd(img, flow, filt, gout, fmad=1) + (None,)
    return oracle.filterinterp_defor_bwd(variant, img, flow, filt, off, gout, fmad=1)


def stats(np_oracle, kernel, variant, img, flow, filt, off, gout):
    if kernel == "interp":
        return np_oracle.interp_bwd_img(flow, gout)
    if kernel == "ori":
        return np_oracle.filterinterp_ori_bwd_img(flow, filt, gout)
    return np_oracle.filterinterp_defor_bwd(variant, img, flow, filt, off, gout, img_stats=True)[0]


WARPS = [("ori", 0), ("interp", 0), ("defor", 0), ("defor", 1), ("defor", 2)]


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("kernel,variant", WARPS, ids=lambda v: str(v))
def test_warping_backward_every_tile_class(torch_mod, cabi, oracle, np_oracle, kernel, variant, C):
    torch = torch_mod
    flow, off, img, filt, gout, g0 = case(kernel, variant)
    img, gout, g0 = img[:, :C], gout[:, :C], g0[:, :C]
    sums, k = predicted_sums(kernel, variant)
    want = bt.convert(sums[:, :C], k, g0)
    recs = bt.tiles(kernel, flow, C, off=off)
    got = run(torch, cabi, kernel, variant, img, flow, filt, off, gout, g0)
    assert_bits(got[0], want, recs, kernel)
    ref = oracle_bwd(oracle, kernel, variant, img, flow, filt, off, gout)
    for name, a, r in zip(("flow", "filter", "offset"), got[1:], ref[1:]):
        if r is not None:
            assert np.array_equal(a, r), "%s %s gradient: %d elements differ" % (kernel, name, int((a != r).sum()))
    if C == CMAX:
        assert_image_grad(got[0], g0, stats(np_oracle, kernel, variant, img, flow, filt, off, gout), k,
                          "defor" if kernel == "defor" else kernel)
        again = run(torch, cabi, kernel, variant, img, flow, filt, off, gout, g0)
        assert all(np.array_equal(a, b) for a, b in zip(got, again) if a is not None)


@pytest.mark.parametrize("C", CS + (16,))
def test_warp_backward_every_tile_class(torch_mod, cabi, C):
    from tests.pwc_warp_backward import pwc_warp_bwd
    torch = torch_mod
    cmax = 16 if C == 16 else CMAX
    flow, _, img, _, gout, g0 = case("warp", 0, cmax)
    img, gout, g0 = img[:, :C], gout[:, :C], g0[:, :C]
    sums, k = predicted_sums("warp", 0, cmax)
    recs = bt.tiles("warp", flow, C)
    if C == 16:
        assert recs[0, 0, 0]["groups"] == (8, 2)
    gx, gf = gpu(torch, g0), torch.full((B, 2, H, W), float("nan"), device="cuda:0")
    assert cabi.pwc_warp_backward(gpu(torch, img), gpu(torch, flow), gpu(torch, gout), gx, gf, True) == 0
    assert_bits(cpu(gx), bt.convert(sums[:, :C], k, g0), recs, "warp")
    ref_x, ref_f, A, S, mask = pwc_warp_bwd(img, flow, gout, True)
    got_f = cpu(gf).astype(np.float64)
    assert np.all(np.abs(got_f - ref_f) <= 1e-5 * S + 1e-7)
    assert np.all(np.abs(cpu(gx) - g0 - ref_x) <= 4e-7 * A + 2.0 ** -(k - 2) + np.abs(np.spacing(g0 + ref_x.astype(f32))))
    hx, hf = gpu(torch, g0), torch.zeros_like(gf)
    assert cabi.pwc_warp_backward(gpu(torch, img), gpu(torch, flow), gpu(torch, gout), hx, hf, True) == 0
    assert torch.equal(gx, hx) and torch.equal(gf, hf)


def _view(torch, a, fill):
    """a [b, c, h, w] as the interior view of a (h + 2) x (w + 5) buffer filled with `fill`"""
    b, c, h, w = a.shape
    buf = torch.full((b, c, h + 2, w + 5), fill, device="cuda:0")
    v = buf[:, :, 1:h + 1, 2:w + 2]
    if a is not None:
        v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return buf, v


@pytest.mark.parametrize("C", CS)
def test_blend_backward_every_tile_class(torch_mod, cabi, oracle, C):
    torch = torch_mod
    rng = np.random.default_rng(600 + C)
    flows, _ = bt.build_field("blend", np.random.default_rng(600), B, H, W, dirs=2)
    refs = [rng.random((B, C, H, W), dtype=f32) for _ in range(2)]
    filts = [rng.random((B, 16, H, W), dtype=f32) for _ in range(2)]
    gb, go0, go2 = (rng.standard_normal((B, C, H, W)).astype(f32) for _ in range(3))
    w0, w2 = 0.75, 0.25
    ins = [_view(torch, a, 0.0)[1] for a in refs + flows + filts + [gb, go0, go2]]
    outs = [_view(torch, np.zeros(a.shape, f32), float("nan")) for a in refs + flows + filts]
    for buf, v in outs:
        v.fill_(float("nan"))
    assert cabi.filterinterp_blend_backward(*ins[:6], *ins[6:], w0, w2, *[v for _, v in outs]) == 0
    torch.cuda.synchronize()
    for buf, v in outs:                                     # nothing outside the views changed
        m = torch.ones_like(buf, dtype=torch.bool)
        m[:, :, 1:H + 1, 2:W + 2] = False
        assert torch.isnan(buf[m]).all()
    for d, (go, wd) in enumerate(((go0, w0), (go2, w2))):
        g = bt.blend_grad(gb, go, wd)
        recs = bt.tiles("blend", flows[d], C)
        want, k, fp32 = bt.predict_image_grad("blend", flows[d], g, filt=filts[d])
        assert not fp32
        assert_bits(cpu(outs[d][1]), want, recs, "blend direction %d" % d)
        r1, r2, r3 = oracle.filterinterp_ori_bwd(refs[d], flows[d], filts[d], g, fmad=1)
        assert np.array_equal(cpu(outs[2 + d][1]), r2), "blend direction %d flow gradient" % d
        assert np.array_equal(cpu(outs[4 + d][1]), r3), "blend direction %d filter gradient" % d
    # without the image gradients: fi_blend_backward4_lds<false>, whose passes take up to three channels
    nox = [_view(torch, np.zeros(a.shape, f32), float("nan"))[1] for a in flows + filts]
    assert cabi.filterinterp_blend_backward(*ins[:6], *ins[6:], w0, w2, None, None, *nox) == 0
    for d in range(2):
        assert {"pc3", "pc2", "pc1", "flag_window"} <= set(bt.label_counts(bt.tiles("blend_nox", flows[d], C)))
        assert torch.equal(nox[d], outs[2 + d][1]) and torch.equal(nox[2 + d], outs[4 + d][1])


@pytest.mark.parametrize("kernel,variant", WARPS + [("warp", 0)], ids=lambda v: str(v))
def test_tiny_gradients_take_the_second_scale_factor(torch_mod, cabi, kernel, variant):
    """gradients near 1e-30: k > 126, gradacc_staged_ok is false, every tile goes to the per-tap path, whose addends are
    v * scale * scale2"""
    torch = torch_mod
    flow, off, img, filt, gout, g0 = case(kernel, variant)
    C = 4
    img, gout, g0 = img[:, :C], (gout[:, :C] * f32(1e-30)).astype(f32), g0[:, :C] * f32(1e-30)
    want, k, fp32 = bt.predict_image_grad(kernel, flow, gout, g0, filt, off, variant)
    assert k > 126 and not fp32
    recs = bt.tiles(kernel, flow, C, off=off, scale2_one=False)
    if kernel == "warp":
        gx = gpu(torch, g0)
        assert cabi.pwc_warp_backward(gpu(torch, img), gpu(torch, flow), gpu(torch, gout), gx, None, True) == 0
        got = cpu(gx)
    else:
        got = run(torch, cabi, kernel, variant, img, flow, filt, off, gout, g0)[0]
    assert_bits(got, want, recs, kernel)


@pytest.mark.parametrize("kernel,variant", WARPS, ids=lambda v: str(v))
def test_non_finite_gradient_lands_where_the_oracle_puts_it(torch_mod, cabi, oracle, kernel, variant):
    torch = torch_mod
    flow, off, img, filt, gout, g0 = case(kernel, variant)
    C = 3
    img, gout = img[:, :C], gout[:, :C].copy()
    gout[0, 1, 2, 10] = np.inf                              # (in the first tile: three channels per pass in every field)
    gout[1, 2, 30, 200] = np.nan
    zero = np.zeros_like(img)
    got = run(torch, cabi, kernel, variant, img, flow, filt, off, gout, zero)[0]
    ref = oracle_bwd(oracle, kernel, variant, img, flow, filt, off, gout)[0]
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
    assert np.isnan(got).any() and np.isinf(got).any()
    fin = np.isfinite(ref)
    assert np.abs(got[fin] - ref[fin]).max() <= GRAD_TOL * max(1.0, np.abs(ref[fin]).max())
