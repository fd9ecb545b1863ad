"""`-m gpu` backward passes: every backward entry point on hypothesis-drawn shapes around the kernels' tiles, on strided views,
and at the magnitude edges of the fixed-point image-gradient scatter (gradacc.h: gradacc_*).

  * per-pixel gradients (flow, filter, offsets, SeparableConv v / h, projections, correlation): bit-exact against the C
    oracle in fmad=1 mode;
  * image gradients of the warping layers, per cell:  |g - (g0 + e)| <= c u S + n 2^-(k+1) + ulp(g0 + e), with e, S, n the
    float64 sum, absolute sum and count of the cell's addends (oracle/np_oracle.py), g0 the tensor's starting value, k the
    scale exponent restated from gradacc.h, u = 2^-24 and c the fp32 roundings of one addend plus one for the conversion
    of the integer sum to float (IMG_ROUNDINGS); bit-exact on dyadic inputs; a second call gives the same bits.
"""
import numpy as np
import pytest

from tests.bwd_tiles import grad_scale
from tests.test_gpu_parity import cpu, gpu, smooth_flow, f32, torch_mod, cabi  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# fp32 roundings per image-gradient addend: 1 - alpha, 1 - beta and the products g x bilinear weights (x filter tap); one more
# for the float conversion of the cell's integer sum
IMG_ROUNDINGS = {"ori": 5 + 1, "defor": 5 + 1, "interp": 4 + 1}
# tiles: fi_backward_ori4_lds 64x8, fi_backward_defor_lds 64x4, interp_backward_lds 64x8, the pixel grid 64x4, corr_backward_k1 64x4
HS = [1, 3, 4, 5, 8, 9, 16, 17]
WS = [1, 2, 63, 64, 65, 129]


def _settings(n):
    from hypothesis import settings, HealthCheck
    return settings(max_examples=n, deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)


def grad_exponent(gout, weights, h, w, taps):
    """the scale exponent k of a call (gradacc.h gradacc_exponent, gradacc_scan): 62 - ceil(log2(h w max(taps, 4))) - eg - ew"""
    return grad_scale(gout, weights, h, w, taps)[0]


def assert_image_grad(got, g0, stats, k, kind):
    e, S, n = stats
    want = g0.astype(np.float64) + e
    ulp = np.abs(np.spacing(want.astype(f32))).astype(np.float64)
    bound = IMG_ROUNDINGS[kind] * U * S * (1 + 1e-6) + n * 2.0 ** -(k + 1) + ulp
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= bound), "worst cell %s: err %g bound %g" % (np.unravel_index(np.argmax(err - bound), err.shape),
                                                                    err.max(), bound.flat[np.argmax(err - bound)])


def make_flow(rng, model, B, H, W):
    if model == "zero":
        return np.zeros((B, 2, H, W), f32)
    if model == "subpixel":
        return rng.uniform(-0.9, 0.9, (B, 2, H, W)).astype(f32)
    if model == "smooth":
        return smooth_flow(rng, B, H, W, 2.0)
    if model == "mixed":            # staged tiles on the left, flagged (+-80 px) on the right
        f = smooth_flow(rng, B, H, W, 2.0)
        f[:, :, :, W // 2:] = rng.uniform(-80, 80, (B, 2, H, W - W // 2)).astype(f32)
        return f
    if model == "border":           # many taps clamped onto the border cells
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        f = np.stack([(W - 1 - xs) * 0.49, -ys * 0.49]).astype(f32)[None].repeat(B, 0)
        f[:, :, ::2] *= -1.0
        return f
    f = smooth_flow(rng, B, H, W, 2.0)   # "invalid": a quarter of the pixels leave the frame
    f[:, 0][rng.random((B, H, W)) < 0.25] = 1.0e4
    return f


FLOWS = ["zero", "subpixel", "smooth", "mixed", "border", "invalid"]


def dyadic(a, q):
    return (np.round(a * q) / q).astype(f32)


def run_warp_bwd(torch, cabi, kind, variant, img, flow, filt, off, gout, g0):
    """one backward call; image gradient from g0, the others from zero.  Returns numpy (gimg, gflow, gfilt or None, goff or None)."""
    B, C, H, W = img.shape
    g1 = gpu(torch, g0)
    g2 = torch.zeros((B, 2, H, W), device="cuda:0")
    if kind == "interp":
        assert cabi.interpolation_backward(gpu(torch, img), gpu(torch, flow), gpu(torch, gout), g1, g2) == 0
        return cpu(g1), cpu(g2), None, None
    if kind == "ori":
        g3 = torch.zeros(filt.shape, device="cuda:0")
        assert cabi.filterinterp_backward_ori(gpu(torch, img), gpu(torch, flow), gpu(torch, filt), gpu(torch, gout), g1, g2, g3) == 0
        return cpu(g1), cpu(g2), cpu(g3), None
    go = torch.zeros(off.shape, device="cuda:0")
    if variant == 2:
        assert cabi.filterinterp_backward_defor(2, gpu(torch, img), gpu(torch, flow), gpu(torch, off), None, gpu(torch, gout),
                                                g1, g2, go, None) == 0
        return cpu(g1), cpu(g2), None, cpu(go)
    gf = torch.zeros(filt.shape, device="cuda:0")
    assert cabi.filterinterp_backward_defor(variant, gpu(torch, img), gpu(torch, flow), gpu(torch, filt), gpu(torch, off),
                                            gpu(torch, gout), g1, g2, gf, go) == 0
    return cpu(g1), cpu(g2), cpu(gf), cpu(go)


def oracle_warp_bwd(oracle, np_oracle, kind, variant, img, flow, filt, off, gout):
    """(C oracle fmad=1 gradients, float64 image-gradient stats)"""
    if kind == "interp":
        r1, r2 = oracle.interp_bwd(img, flow, gout, fmad=1)
        return (r1, r2, None, None), np_oracle.interp_bwd_img(flow, gout)
    if kind == "ori":
        r1, r2, r3 = oracle.filterinterp_ori_bwd(img, flow, filt, gout, fmad=1)
        return (r1, r2, r3, None), np_oracle.filterinterp_ori_bwd_img(flow, filt, gout)
    r = oracle.filterinterp_defor_bwd(variant, img, flow, filt, off, gout, fmad=1)
    return r, np_oracle.filterinterp_defor_bwd(variant, img, flow, filt, off, gout, img_stats=True)[0]


def check_warp_example(torch, cabi, oracle, np_oracle, kind, variant, B, C, H, W, fs, model, seed):
    rng = np.random.default_rng(seed)
    taps = fs * fs if kind != "interp" else 4
    img = rng.standard_normal((B, C, H, W)).astype(f32)
    flow = make_flow(rng, model, B, H, W)
    filt = rng.random((B, taps, H, W), dtype=f32)
    off = rng.uniform(-1.5, 1.5, (B, 2 * taps, H, W)).astype(f32)
    gout = rng.standard_normal((B, C, H, W)).astype(f32)
    g0 = rng.standard_normal((B, C, H, W)).astype(f32)              # the reference adds into gradinput1
    weights = None if kind == "interp" or variant == 2 else filt
    got = run_warp_bwd(torch, cabi, kind, variant, img, flow, filt, off, gout, g0)
    ref, stats = oracle_warp_bwd(oracle, np_oracle, kind, variant, img, flow, filt, off, gout)
    assert_image_grad(got[0], g0, stats, grad_exponent(gout, weights, H, W, taps), kind)
    for a, r in zip(got[1:], ref[1:]):
        if r is not None:
            assert np.array_equal(a, r), "per-pixel gradient: max diff %g" % np.abs(a - r).max()
    again = run_warp_bwd(torch, cabi, kind, variant, img, flow, filt, off, gout, g0)
    assert all(np.array_equal(a, b) for a, b in zip(got, again) if a is not None)      # order-free: same bits
    # dyadic inputs: every addend and every partial sum exact, so the result IS the oracle's (from a zero start)
    fq, gq, filtq, offq = dyadic(flow, 4), dyadic(gout, 16), dyadic(filt, 16), dyadic(off, 4)
    got = run_warp_bwd(torch, cabi, kind, variant, img, fq, filtq, offq, gq, np.zeros_like(g0))
    ref, _ = oracle_warp_bwd(oracle, np_oracle, kind, variant, img, fq, filtq, offq, gq)
    assert np.array_equal(got[0], ref[0]), "dyadic image gradient: max diff %g" % np.abs(got[0] - ref[0]).max()


# ------------------------------------------------------------------ 2. sweeps

@pytest.mark.parametrize("kind,variant", [("ori", None), ("defor", 0), ("defor", 1), ("defor", 2), ("interp", None)])
def test_warp_backward_random_shapes(torch_mod, cabi, oracle, np_oracle, kind, variant):
    """B up to 3, C in {1, 2, 3, 4, 7} (the three-channel passes and a remainder), H / W around every backward tile and 1,
    fs 2..6 (4: the staged kernels), six flow models including staged and flagged tiles in one call."""
    from hypothesis import example, given, strategies as st

    @_settings(60)
    @given(st.sampled_from([1, 2, 3]), st.sampled_from([1, 2, 3, 4, 7]), st.sampled_from(HS), st.sampled_from(WS),
           st.sampled_from([2, 3, 4, 4, 5, 6]), st.sampled_from(FLOWS), st.integers(0, 2 ** 31 - 1))
    # staged and flagged tiles in one call, at the staged filter size and beside it, ragged in both directions
    @example(3, 7, 17, 129, 4, "mixed", 1)
    @example(2, 4, 9, 65, 4, "border", 2)
    @example(1, 3, 16, 129, 4, "smooth", 3)
    @example(3, 2, 8, 64, 6, "mixed", 4)
    @example(2, 7, 5, 63, 4, "invalid", 5)
    def run(B, C, H, W, fs, model, seed):
        check_warp_example(torch_mod, cabi, oracle, np_oracle, kind, variant, B, C, H, W, fs, model, seed)

    run()


def test_projection_backward_random_shapes(torch_mod, cabi, oracle):
    torch = torch_mod
    from hypothesis import given, strategies as st

    @_settings(25)
    @given(st.sampled_from([1, 2, 3]), st.sampled_from(HS), st.sampled_from(WS), st.sampled_from(FLOWS), st.integers(0, 2 ** 31 - 1))
    def run(B, H, W, model, seed):
        rng = np.random.default_rng(seed)
        flow = make_flow(rng, model, B, H, W)
        depth = rng.uniform(0.1, 1.0, (B, 1, H, W)).astype(f32)
        gout = rng.standard_normal((B, 2, H, W)).astype(f32)
        out, count = oracle.depthflowproj_fwd(flow, depth, 0)
        cnt = np.where(count > 0, count, 1).astype(f32)
        g1 = torch.zeros((B, 2, H, W), device="cuda:0")
        assert cabi.flowprojection_backward(gpu(torch, flow), gpu(torch, cnt), gpu(torch, gout), g1) == 0
        assert np.array_equal(cpu(g1), oracle.flowproj_bwd(flow, cnt, gout))
        g1.zero_()
        g2 = torch.zeros((B, 1, H, W), device="cuda:0")
        assert cabi.depthflowprojection_backward(gpu(torch, flow), gpu(torch, depth), gpu(torch, cnt), gpu(torch, out),
                                                 gpu(torch, gout), g1, g2) == 0
        rf, rd = oracle.depthflowproj_bwd(flow, depth, cnt, out, gout)
        assert np.array_equal(cpu(g1), rf) and np.array_equal(cpu(g2), rd)
        _, mcount = oracle.mindepthflowproj_fwd(flow, depth, 0)
        g1.zero_(), g2.zero_()
        assert cabi.mindepthflowprojection_backward(gpu(torch, flow), gpu(torch, depth), gpu(torch, mcount), gpu(torch, out),
                                                    gpu(torch, gout), g1, g2) == 0
        assert np.array_equal(cpu(g1), oracle.mindepthflowproj_bwd(flow, depth, mcount, gout)) and not cpu(g2).any()

    run()


def test_separableconv_backward_random_shapes(torch_mod, cabi, oracle):
    torch = torch_mod
    from hypothesis import given, strategies as st

    @_settings(20)
    @given(st.sampled_from([1, 2, 3]), st.sampled_from([1, 2, 3, 5, 6]), st.sampled_from(HS), st.sampled_from(WS),
           st.integers(0, 2 ** 31 - 1))
    def run(B, fs, H, W, seed):
        H, W = H + fs - 1, W + fs - 1
        rng = np.random.default_rng(seed)
        oh, ow = H - fs + 1, W - fs + 1
        img = rng.standard_normal((B, 3, H, W)).astype(f32)
        v = rng.random((B, fs, oh, ow), dtype=f32)
        h = rng.random((B, fs, oh, ow), dtype=f32)
        gi, gv, gh = gpu(torch, img), gpu(torch, v), gpu(torch, h)
        gout = rng.standard_normal((B, 3, oh, ow)).astype(f32)
        g1, g2, g3 = torch.zeros_like(gi), torch.zeros_like(gv), torch.zeros_like(gh)
        assert cabi.separableconv_backward(gi, gv, gh, gpu(torch, gout), g1, g2, g3) == 0
        r1, r2, r3 = oracle.sepconv_bwd(img, v, h, gout)
        assert np.array_equal(cpu(g1), r1) and np.array_equal(cpu(g2), r2) and np.array_equal(cpu(g3), r3)
        gflow = rng.standard_normal((B, 2, oh, ow)).astype(f32)
        g2.zero_(), g3.zero_()
        assert cabi.separableconvflow_backward(gi, gv, gh, gpu(torch, gflow), g2, g3) == 0
        r2, r3 = oracle.sepconvflow_bwd(v, h, gflow, H, W, fmad=1)
        assert np.array_equal(cpu(g2), r2) and np.array_equal(cpu(g3), r3)

    run()


def test_correlation_backward_random_shapes(torch_mod, cabi, oracle):
    """PWC-Net's configuration (pad 4, k 1, md 4: the pixel-owns-its-gradOutput kernel, channel groups split with a
    remainder up to C ~ 200) and the generic kernel (other pads, k = 3, stride2 = 2)."""
    torch = torch_mod
    from hypothesis import given, strategies as st

    @_settings(25)
    @given(st.sampled_from([1, 2, 3]), st.sampled_from([1, 3, 7, 33, 64, 65, 130, 197]), st.sampled_from(HS),
           st.sampled_from(WS), st.sampled_from([(4, 1, 4, 1), (4, 1, 4, 1), (3, 3, 4, 2), (2, 1, 4, 1), (4, 1, 2, 2)]),
           st.integers(0, 2 ** 31 - 1))
    def run(B, C, H, W, cfg, seed):
        pad, k, md, s2 = cfg
        if C > 64 and H * W > 2000:
            C = 64
        rng = np.random.default_rng(seed)
        try:
            oc, oh, ow = oracle.correlation_out_dims(H, W, pad, k, md, 1, s2)
        except Exception:
            return
        if oh <= 0 or ow <= 0:
            return
        f1 = rng.standard_normal((B, C, H, W)).astype(f32)
        f2 = rng.standard_normal((B, C, H, W)).astype(f32)
        g = rng.standard_normal((B, oc, oh, ow)).astype(f32)
        g1, g2 = cabi.correlation_backward(gpu(torch, f1), gpu(torch, f2), gpu(torch, g), pad, k, md, 1, s2)
        r1, r2 = oracle.correlation_bwd(f1, f2, g, pad, k, md, 1, s2)
        assert np.array_equal(cpu(g1), r1) and np.array_equal(cpu(g2), r2)

    run()


def test_correlation_backward_refuses_stride1(torch_mod, cabi):
    torch = torch_mod
    f = torch.zeros((1, 4, 16, 16), device="cuda:0")
    with pytest.raises(Exception):
        cabi.correlation_backward(f, f, torch.zeros((1, 81, 8, 8), device="cuda:0"), 4, 1, 4, 2, 1)


# ------------------------------------------------------------------ 3. views

def strided(torch, a, mode, fill=7.0):
    """a as a channel slice ("chan") or a width crop ("crop", stride(3) == 1) of a larger tensor filled with `fill`"""
    a = np.asarray(a, f32)
    B, C, H, W = a.shape
    if mode == "chan":
        big = torch.full((B, C + 3, H, W), fill, device="cuda:0")
        v = big[:, 2:2 + C]
    else:
        big = torch.full((B, C, H, W + 5), fill, device="cuda:0")
        v = big[:, :, :, 3:3 + W]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return v


def prefix_view(torch, a, span):
    """a contiguous tensor holding `a`, allocated as the prefix of a buffer of `span` elements (reads past a with another
    tensor's strides stay inside the allocation)"""
    a = np.asarray(a, f32)
    buf = torch.full((max(span, a.size),), 5.0, device="cuda:0")
    t = buf[:a.size].view(a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def _span(t):
    return t.storage_offset() + sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1 + 64


def _bwd_calls(oracle, rng, B, C, H, W, fs):
    """(name, arrays, call(torch, cabi, T) -> tuple of result tensors) for every backward entry point; T maps a name to a
    tensor (inputs and zero / non-zero starting gradients alike)"""
    taps = fs * fs
    a = dict(img=rng.standard_normal((B, C, H, W)).astype(f32), flow=smooth_flow(rng, B, H, W, 2.0),
             filt=rng.random((B, taps, H, W), dtype=f32), off=rng.uniform(-1.5, 1.5, (B, 2 * taps, H, W)).astype(f32),
             gout=rng.standard_normal((B, C, H, W)).astype(f32), g1=rng.standard_normal((B, C, H, W)).astype(f32),
             g2=np.zeros((B, 2, H, W), f32), gf=np.zeros((B, taps, H, W), f32), go=np.zeros((B, 2 * taps, H, W), f32),
             depth=rng.uniform(0.1, 1.0, (B, 1, H, W)).astype(f32), gout2=rng.standard_normal((B, 2, H, W)).astype(f32),
             gd=np.zeros((B, 1, H, W), f32))
    out, count = oracle.depthflowproj_fwd(a["flow"], a["depth"], 0)
    a["out"], a["count"] = out, np.where(count > 0, count, 1).astype(f32)
    calls = [
        ("ori", lambda c, T: (c.filterinterp_backward_ori(T["img"], T["flow"], T["filt"], T["gout"], T["g1"], T["g2"], T["gf"]),
                              T["g1"], T["g2"], T["gf"])),
        ("interp", lambda c, T: (c.interpolation_backward(T["img"], T["flow"], T["gout"], T["g1"], T["g2"]), T["g1"], T["g2"])),
        ("flowproj", lambda c, T: (c.flowprojection_backward(T["flow"], T["count"], T["gout2"], T["g2"]), T["g2"])),
        ("depthproj", lambda c, T: (c.depthflowprojection_backward(T["flow"], T["depth"], T["count"], T["out"], T["gout2"],
                                                                   T["g2"], T["gd"]), T["g2"], T["gd"])),
        ("mindepthproj", lambda c, T: (c.mindepthflowprojection_backward(T["flow"], T["depth"], T["count"], T["out"], T["gout2"],
                                                                         T["g2"], T["gd"]), T["g2"])),
    ]
    for v in (0, 1):
        calls.append(("defor%d" % v, lambda c, T, v=v: (c.filterinterp_backward_defor(
            v, T["img"], T["flow"], T["filt"], T["off"], T["gout"], T["g1"], T["g2"], T["gf"], T["go"]), T["g1"], T["g2"], T["gf"], T["go"])))
    calls.append(("defor2", lambda c, T: (c.filterinterp_backward_defor(2, T["img"], T["flow"], T["off"], None, T["gout"], T["g1"],
                                                                          T["g2"], T["go"], None), T["g1"], T["g2"], T["go"])))
    return a, calls


@pytest.mark.parametrize("mode", ["chan", "crop"])
@pytest.mark.parametrize("fs", [4, 3])
def test_backward_on_views_equals_contiguous(torch_mod, cabi, oracle, mode, fs):
    """Inputs that are channel slices or width crops, gradients as matching views: every result equals the call on
    contiguous copies bit for bit, and nothing outside the views is written."""
    torch = torch_mod
    rng = np.random.default_rng(900 + fs)
    B, C, H, W = 2, 4, 12, 70
    arrays, calls = _bwd_calls(oracle, rng, B, C, H, W, fs)
    for name, call in calls:
        dense = {k: gpu(torch, v) for k, v in arrays.items()}
        views = {k: strided(torch, v, mode) for k, v in arrays.items()}
        rd, rv = call(cabi, dense), call(cabi, views)
        assert rd[0] == 0 and rv[0] == 0, name
        for x, y in zip(rd[1:], rv[1:]):
            assert torch.equal(x, y), name
            assert torch.all(y._base.flatten()[~torch.isin(torch.arange(y._base.numel(), device="cuda:0"),
                                                           _view_indices(torch, y))] == 7.0), name

    # SeparableConv / SeparableConvFlow (three channels, outputs smaller than the image)
    oh, ow = H - fs + 1, W - fs + 1
    img = rng.standard_normal((B, 3, H, W)).astype(f32)
    v, h = rng.random((B, fs, oh, ow), dtype=f32), rng.random((B, fs, oh, ow), dtype=f32)
    gout, gfl = rng.standard_normal((B, 3, oh, ow)).astype(f32), rng.standard_normal((B, 2, oh, ow)).astype(f32)
    res = []
    for mk in (gpu, lambda t, x: strided(t, x, mode)):
        T = dict(img=mk(torch, img), v=mk(torch, v), h=mk(torch, h), gout=mk(torch, gout), gfl=mk(torch, gfl),
                 g1=mk(torch, np.zeros_like(img)), g2=mk(torch, np.zeros_like(v)), g3=mk(torch, np.zeros_like(h)),
                 f2=mk(torch, np.zeros_like(v)), f3=mk(torch, np.zeros_like(h)))
        assert cabi.separableconv_backward(T["img"], T["v"], T["h"], T["gout"], T["g1"], T["g2"], T["g3"]) == 0
        assert cabi.separableconvflow_backward(T["img"], T["v"], T["h"], T["gfl"], T["f2"], T["f3"]) == 0
        res.append([cpu(T[k]) for k in ("g1", "g2", "g3", "f2", "f3")])
    assert all(np.array_equal(x, y) for x, y in zip(*res))
    # correlation (the binding makes its inputs contiguous)
    f1, f2 = rng.standard_normal((B, 5, H, W)).astype(f32), rng.standard_normal((B, 5, H, W)).astype(f32)
    g = rng.standard_normal((B, 81, H, W)).astype(f32)
    a = cabi.correlation_backward(gpu(torch, f1), gpu(torch, f2), gpu(torch, g), 4, 1, 4, 1, 1)
    b = cabi.correlation_backward(strided(torch, f1, mode), strided(torch, f2, mode), strided(torch, g, mode), 4, 1, 4, 1, 1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _view_indices(torch, t):
    """flat indices into t._base of t's elements"""
    idx = torch.zeros((), dtype=torch.int64, device="cuda:0") + t.storage_offset() - t._base.storage_offset()
    for n, s in zip(t.shape, t.stride()):
        idx = idx[..., None] + torch.arange(n, device="cuda:0") * s
    return idx.flatten()


@pytest.mark.parametrize("name", ["ori", "defor0", "defor1", "defor2", "interp", "flowproj", "depthproj", "mindepthproj"])
def test_backward_gradoutput_layout_mismatch(torch_mod, cabi, oracle, name):
    """A gradoutput (or output, or a gradient) whose shape or strides differ from those of the tensor whose strides the
    library addresses it with: refused (return 1) or computed correctly -- never read with the other tensor's strides.
    Every such tensor is the prefix of an allocation that the other tensor's strides stay inside."""
    torch = torch_mod
    rng = np.random.default_rng(950)
    B, C, H, W, fs = 2, 3, 10, 40, 4
    arrays, calls = _bwd_calls(oracle, rng, B, C, H, W, fs)
    call = dict(calls)[name]
    want = call(cabi, {k: gpu(torch, v) for k, v in arrays.items()})
    assert want[0] == 0
    proj = name.endswith("proj")
    keys = ["gout2", "g2"] + (["out", "gd"] if name == "depthproj" else []) if proj else ["gout", "g1"]
    for key in keys:
        for kind in ("strides", "shape"):
            T = {k: strided(torch, v, "crop") for k, v in arrays.items()}
            ref = T["flow"] if key in ("gout2", "g2", "out") else T["depth"] if key == "gd" else T["img"]
            a = arrays[key] if kind == "strides" else arrays[key][:, :, :-1]
            T[key] = prefix_view(torch, a, _span(ref))
            got = call(cabi, T)
            if kind == "shape":
                assert got[0] == 1, (name, key, kind)
            else:
                assert got[0] in (0, 1), (name, key, kind)
                if got[0] == 0:
                    assert all(torch.equal(x, y) for x, y in zip(want[1:], got[1:])), (name, key, kind)


# ------------------------------------------------------------------ 4. magnitude edges of the fixed-point scatter

@pytest.mark.parametrize("kind,variant", [("ori", None), ("defor", 0), ("defor", 1), ("defor", 2), ("interp", None)])
def test_image_gradient_power_of_two_scaling(torch_mod, cabi, kind, variant):
    """g(2^s gout) == 2^s g(gout) bit for bit for s from -110 to +100: every addend stays a normal fp32 number (gradoutput in
    [0.5, 1], flow fractions in [1/8, 7/8], filters in [1/4, 1]: addends in [2^-9, 1]) and is not dyadic, so a scale that
    stopped at 2^126 would round the small ones onto a coarse grid."""
    torch = torch_mod
    rng = np.random.default_rng(77 + (variant or 0))
    B, C, H, W, fs = 1, 3, 20, 70, 4
    taps = 16 if kind != "interp" else 4
    img = rng.standard_normal((B, C, H, W)).astype(f32)
    flow = (rng.integers(-2, 3, (B, 2, H, W)) + rng.uniform(1 / 8, 7 / 8, (B, 2, H, W))).astype(f32)
    filt = rng.uniform(0.25, 1.0, (B, taps, H, W)).astype(f32)
    off = rng.uniform(-1.5, 1.5, (B, 2 * taps, H, W)).astype(f32)
    gout = rng.uniform(0.5, 1.0, (B, C, H, W)).astype(f32)
    zero = np.zeros((B, C, H, W), f32)
    base = run_warp_bwd(torch, cabi, kind, variant, img, flow, filt, off, gout, zero)[0]
    assert base.min() >= 0 and (base > 0).sum() > 0.5 * base.size
    for s in (-110, -100, -90, -84, -80, -60, -20, 1, 40, 80, 100):
        got = run_warp_bwd(torch, cabi, kind, variant, img, flow, filt, off, np.ldexp(gout, s).astype(f32), zero)[0]
        assert np.array_equal(got, np.ldexp(base, s).astype(f32)), (s, np.abs(got / np.ldexp(base, s) - 1)[base > 0].max())


@pytest.mark.parametrize("kind,variant", [("ori", None), ("defor", 0), ("defor", 1)])
def test_image_gradient_overflowing_products(torch_mod, cabi, oracle, kind, variant):
    """Finite gradoutput up to 1e30 and filters up to 1e10: some products overflow to infinities, others do not.  The
    inf / NaN cells and the signs of the infinities are the sequential oracle's, the finite cells agree within 1e-5."""
    torch = torch_mod
    rng = np.random.default_rng(88 + (variant or 0))
    B, C, H, W, fs = 1, 2, 24, 70, 4
    img = rng.random((B, C, H, W), dtype=f32)
    flow = smooth_flow(rng, B, H, W, 2.0)
    filt = rng.random((B, 16, H, W), dtype=f32)
    off = rng.uniform(-1.5, 1.5, (B, 32, H, W)).astype(f32)
    gout = rng.standard_normal((B, C, H, W)).astype(f32)
    big_g = rng.random((B, C, H, W)) < 0.05
    gout[big_g] = np.sign(gout[big_g]) * 1e30
    big_f = rng.random((B, 16, H, W)) < 0.05
    filt[big_f] = 1e10
    got = run_warp_bwd(torch, cabi, kind, variant, img, flow, filt, off, gout, np.zeros((B, C, H, W), f32))[0]
    if kind == "ori":
        ref = oracle.filterinterp_ori_bwd(img, flow, filt, gout, fmad=1)[0]
    else:
        ref = oracle.filterinterp_defor_bwd(variant, img, flow, filt, off, gout, fmad=1)[0]
    assert np.isinf(ref).sum() >= 4 and np.isfinite(ref).sum() > 0.5 * ref.size
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
    assert np.array_equal(np.sign(got[np.isinf(ref)]), np.sign(ref[np.isinf(ref)]))
    fin = np.isfinite(ref)
    assert np.abs(got[fin] - ref[fin]).max() <= 1e-5 * max(1.0, np.abs(ref[fin]).max())
