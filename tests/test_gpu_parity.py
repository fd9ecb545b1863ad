"""GPU suite (`-m gpu`): the HIP kernels, called through the C ABI (ctypes) and through the
reference-named extension modules / wrapper mirrors, against the CPU oracle and the
committed golden fixtures.

Tolerances (float32):
  * deterministic ops (FilterInterpolation fwd incl. deformable variants, Interpolation fwd,
    SeparableConv fwd, SeparableConvFlow, correlation fwd, the per-pixel parts of the
    backwards): BIT-EXACT against the oracle in fmad=1 mode (same operations, same order,
    same fused multiply-adds), and <= 1e-5 * max(1, |ref|) against the oracle's strict
    C-semantics mode and the golden fixtures (the only difference is FMA contraction);
  * scatter ops (projections fwd, image gradients): `count` bit-exact for FlowProjection,
    values <= 1e-4 abs (fp32 atomic order); bit-exact on dyadic inputs whose sums are exact
    in any order; identical hole mask;
  * correlation against the reference's 32-lane tree order: <= 1e-5 rel.
"""
import os

import numpy as np
import pytest

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


def gpu(torch, a):
    # copy into a freshly allocated tensor: canonical dense strides whatever numpy's layout was
    # (from_numpy / torch.tensor keep a transposed layout or the arbitrary stride of a size-1
    # axis, which the bindings' stride checks rightly reject)
    a = np.asarray(a)
    t = torch.empty(a.shape, dtype=torch.float32, device="cuda:0")
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def cpu(t):
    return t.detach().cpu().numpy()


def smooth_flow(rng, b, h, w, sigma):
    from tests.golden.make_golden import smooth_flow as sf
    return sf(rng, b, h, w, sigma)


# image gradients of the warping layers: exact integer (fixed-point) sums rounded to fp32 once, against the oracle's
# sequential fp32 sums (one rounding per addend); the reference's own atomics differ from run to run by as much
GRAD_TOL = 2e-6


def close(a, ref, tol=1e-5):
    return np.all(np.abs(a - ref) <= tol * np.maximum(1.0, np.abs(ref)))


# ------------------------------------------------------------------ FilterInterpolation forward

FI_SHAPES = [(1, 3, 32, 48), (2, 5, 40, 72), (1, 3, 17, 130), (1, 1, 1, 1), (1, 2, 3, 5), (3, 4, 16, 64),
             (1, 196, 20, 70)]


def run_fi(torch, cabi, img, flow, filt, direct=False):
    out = torch.full_like(img, float("nan"))         # every element must be written
    assert cabi.filterinterp_forward_ori(img, flow, filt, out, direct=direct) == 0
    return out


@pytest.mark.parametrize("B,C,H,W", FI_SHAPES)
@pytest.mark.parametrize("flow_kind", ["smooth", "uniform1", "wild", "zero", "border"])
def test_filterinterp_forward_bit_exact(torch_mod, cabi, oracle, B, C, H, W, flow_kind):
    torch = torch_mod
    rng = np.random.default_rng(B * 7 + C * 3 + H + W)
    img = rng.random((B, C, H, W), dtype=f32)
    filt = rng.random((B, 16, H, W), dtype=f32)
    if flow_kind == "smooth":
        flow = smooth_flow(rng, B, H, W, 3.0)
    elif flow_kind == "uniform1":
        flow = rng.uniform(-1, 1, (B, 2, H, W)).astype(f32)
    elif flow_kind == "wild":
        flow = rng.uniform(-W / 2, W / 2, (B, 2, H, W)).astype(f32)
    elif flow_kind == "zero":
        flow = np.zeros((B, 2, H, W), f32)
    else:   # every pixel lands exactly on the last row / column or on (0,0): closed bounds, clamped windows
        flow = np.zeros((B, 2, H, W), f32)
        flow[:, 0] = (W - 1) - np.arange(W)[None, None, :]
        flow[:, 1] = (H - 1) - np.arange(H)[None, :, None]
        flow[:, :, ::2, ::2] *= -0.0
        flow[:, 0, 1::2] = -np.arange(W)[None, None, :]
    ref = oracle.filterinterp_ori_fwd(img, flow, filt, fmad=1)
    strict = oracle.filterinterp_ori_fwd(img, flow, filt, fmad=0)
    for direct in (False, True):
        out = cpu(run_fi(torch, cabi, gpu(torch, img), gpu(torch, flow), gpu(torch, filt), direct))
        assert np.array_equal(out, ref), "max diff %g" % np.abs(out - ref).max()
        assert close(out, strict)


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 9, 23])
def test_filterinterp_forward_mixed_tiles_and_short_channel_ranges(torch_mod, cabi, oracle, C):
    """One frame whose 64x16 tiles take different paths of the staged kernel: smooth tiles (4-byte tap reads), rough tiles
    whose bounding box is tall / wide (aligned 8-byte tap reads, odd and even window origins, negative window corners at
    the frame border), tiles too rough for the 8-byte pitch, and a band that leaves the frame (copy-through).  Channel
    counts below, at and above the ring depth: the steady-state loop, the tail loop and both together.  Bit-exact."""
    torch = torch_mod
    rng = np.random.default_rng(100 + C)
    B, H, W = 1, 96, 448
    img = rng.random((B, C, H, W), dtype=f32)
    filt = rng.random((B, 16, H, W), dtype=f32)
    flow = smooth_flow(rng, B, H, W, 3.0)
    flow[:, :, :, 128:256] += rng.uniform(-9, 9, (B, 2, H, 128)).astype(f32)         # rough: boxes ~ 16 + 21 rows
    flow[:, :, :, 256:320] += rng.uniform(-30, 30, (B, 2, H, 64)).astype(f32)        # too rough for the wide pitch
    flow[:, 0, 40:56, 330:400] = 1000.0                                              # invalid: copy-through
    flow[:, :, :16, :64] = rng.uniform(-9, 0, (B, 2, 16, 64)).astype(f32)            # rough at the top-left corner
    ref = oracle.filterinterp_ori_fwd(img, flow, filt, fmad=1)
    out = cpu(run_fi(torch, cabi, gpu(torch, img), gpu(torch, flow), gpu(torch, filt)))
    assert np.array_equal(out, ref), "max diff %g" % np.abs(out - ref).max()


@pytest.mark.parametrize("fs", [2, 3, 5, 6])
def test_filterinterp_forward_other_filter_sizes(torch_mod, cabi, oracle, fs):
    torch = torch_mod
    rng = np.random.default_rng(fs)
    B, C, H, W = 2, 3, 24, 70
    img = rng.random((B, C, H, W), dtype=f32)
    filt = rng.random((B, fs * fs, H, W), dtype=f32)
    flow = smooth_flow(rng, B, H, W, 3.0)
    out = cpu(run_fi(torch, cabi, gpu(torch, img), gpu(torch, flow), gpu(torch, filt)))
    assert np.array_equal(out, oracle.filterinterp_ori_fwd(img, flow, filt, fmad=1))


@pytest.mark.parametrize("fs", [2, 5, 6])
def test_filterinterp_lds_other_filter_sizes(torch_mod, cabi, oracle, fs):
    """fs = 2, 5, 6 (the reference's other --filter_size choices) run the LDS-staged kernel of filterinterp_lds_n.hip:
    same bits as the direct kernel and the oracle, on ragged frames, with windows that fit and that do not."""
    torch = torch_mod
    rng = np.random.default_rng(50 + fs)
    for (B, C, H, W, kind, sig) in ((2, 3, 37, 70, "smooth", 3.0), (1, 7, 64, 200, "smooth", 9.0), (1, 2, 9, 5, "rand", 2.0),
                                    (1, 3, 40, 130, "rand", 60.0), (1, 4, 130, 131, "smooth", 0.0)):
        img = rng.standard_normal((B, C, H, W)).astype(f32)
        filt = rng.random((B, fs * fs, H, W), dtype=f32)
        flow = smooth_flow(rng, B, H, W, sig) if kind == "smooth" else (rng.standard_normal((B, 2, H, W)) * sig).astype(f32)
        gi, gf, gk = gpu(torch, img), gpu(torch, flow), gpu(torch, filt)
        a = run_fi(torch, cabi, gi, gf, gk, direct=False)
        b = run_fi(torch, cabi, gi, gf, gk, direct=True)
        assert torch.equal(a, b), (fs, B, C, H, W, kind)
        assert np.array_equal(cpu(a), oracle.filterinterp_ori_fwd(img, flow, filt, fmad=1))


def test_filterinterp_forward_strided_views(torch_mod, cabi, oracle):
    """batch / channel / row strides other than dense (the bindings allow any with w stride 1)."""
    torch = torch_mod
    rng = np.random.default_rng(9)
    B, C, H, W = 2, 3, 20, 66
    big = gpu(torch, rng.random((B, C + 2, H + 3, W + 5), dtype=f32))
    img = big[:, 1:C + 1, 2:H + 2, 3:W + 3]
    outbuf = torch.zeros_like(big)
    out = outbuf[:, 1:C + 1, 2:H + 2, 3:W + 3]
    fbig = gpu(torch, rng.random((B, 18, H, W + 1), dtype=f32))
    filt = fbig[:, 1:17, :, :W]
    flow_np = smooth_flow(rng, B, H, W, 3.0)
    flow = gpu(torch, flow_np)
    assert not img.is_contiguous() and not filt.is_contiguous()
    assert cabi.filterinterp_forward_ori(img, flow, filt, out) == 0
    ref = oracle.filterinterp_ori_fwd(cpu(img), flow_np, cpu(filt), fmad=1)
    assert np.array_equal(cpu(out), ref)
    outbuf[:, 1:C + 1, 2:H + 2, 3:W + 3] = 0
    assert not outbuf.any()                              # nothing written outside the view


def test_filterinterp_binding_checks(torch_mod, cabi):
    torch = torch_mod
    img = torch.zeros((1, 3, 8, 8), device="cuda:0")
    filt = torch.zeros((1, 16, 8, 8), device="cuda:0")
    out = torch.zeros_like(img)
    assert cabi.filterinterp_forward_ori(img, torch.zeros((1, 3, 8, 8), device="cuda:0"), filt, out) == 1
    assert cabi.filterinterp_forward_ori(img, torch.zeros((1, 2, 8, 9), device="cuda:0"), filt, out) == 1
    assert cabi.filterinterp_forward_ori(img, torch.zeros((2, 2, 8, 8), device="cuda:0"), filt, out) == 1
    import filterinterpolation_cuda as m
    assert m.FilterInterpolationLayer_gpu_forward_ori(img, torch.zeros((1, 3, 8, 8), device="cuda:0"), filt, out) == 1
    with pytest.raises(RuntimeError):
        cabi.filterinterp_forward_ori(img.cpu(), torch.zeros((1, 2, 8, 8)), filt.cpu(), out.cpu())


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("fs", [4, 6, 3])
def test_deformable_forward_bit_exact(torch_mod, cabi, oracle, variant, fs):
    torch = torch_mod
    rng = np.random.default_rng(40 + variant + fs)
    B, C, H, W = 2, 3, 24, 70
    img = rng.random((B, C, H, W), dtype=f32)
    flow = smooth_flow(rng, B, H, W, 2.0)
    filt = rng.random((B, fs * fs, H, W), dtype=f32)
    for scale in (0.5, 3.0):
        off = rng.uniform(-scale, scale, (B, 2 * fs * fs, H, W)).astype(f32)
        out = torch.zeros((B, C, H, W), device="cuda:0")
        if variant == 2:
            err = cabi.filterinterp_forward_defor(variant, gpu(torch, img), gpu(torch, flow), gpu(torch, off), None, out)
        else:
            err = cabi.filterinterp_forward_defor(variant, gpu(torch, img), gpu(torch, flow), gpu(torch, filt),
                                                  gpu(torch, off), out)
        assert err == 0
        ref = oracle.filterinterp_defor_fwd(variant, img, flow, filt, off, fmad=1)
        assert np.array_equal(cpu(out), ref)


@pytest.mark.parametrize("fs", [4, 6])
def test_deformable_fast_kernel_equals_general(torch_mod, cabi, oracle, fs):
    """fs == 4 and fs == 6 (the sizes the reference's 4-input kernel has bodies for) run the LDS-staged kernel; the general
    one-thread-per-pixel kernel is kept for other sizes.  Same bits, on frames with taps leaving the image on every side and
    large learned offsets (the last case: windows that do not fit the LDS, the staged kernel's own gather fallback)."""
    torch = torch_mod
    rng = np.random.default_rng(41 + fs)
    for (B, C, H, W, sig, osig) in ((2, 5, 37, 70, 3.0, 0.7), (1, 9, 64, 130, 8.0, 3.0), (1, 3, 8, 9, 1.0, 6.0), (1, 2, 40, 200, 2.0, 40.0)):
        img = rng.standard_normal((B, C, H, W)).astype(f32)
        flow = smooth_flow(rng, B, H, W, sig) if min(H, W) >= 16 else (rng.standard_normal((B, 2, H, W)) * sig).astype(f32)
        filt = rng.random((B, fs * fs, H, W), dtype=f32)
        off = (rng.standard_normal((B, 2 * fs * fs, H, W)) * osig).astype(f32)
        for variant in (0, 1, 2):
            third = off if variant == 2 else filt
            outs = []
            for general in (False, True):
                out = torch.full((B, C, H, W), float("nan"), device="cuda:0")
                assert cabi.filterinterp_forward_defor(variant, gpu(torch, img), gpu(torch, flow), gpu(torch, third),
                                                       None if variant == 2 else gpu(torch, off), out, general=general) == 0
                outs.append(out)
            assert torch.equal(outs[0], outs[1]), (variant, B, C, H, W)
            assert np.array_equal(cpu(outs[0]), oracle.filterinterp_defor_fwd(variant, img, flow, filt, off, fmad=1))


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("fs", [4, 6, 3])
def test_deformable_backward(torch_mod, cabi, oracle, variant, fs):
    """gflow / gfilt / goff cells belong to one pixel: bit-exact.  gimg: order-free fixed-point scatter."""
    torch = torch_mod
    rng = np.random.default_rng(70 + variant + fs)
    B, C, H, W = 2, 3, 20, 70
    img = rng.random((B, C, H, W), dtype=f32)
    flow = smooth_flow(rng, B, H, W, 2.0)
    flow[0, 0, 3, 3] = W                                       # invalid pixel: no gradient at all
    filt = rng.random((B, fs * fs, H, W), dtype=f32)
    gout = rng.normal(size=(B, C, H, W)).astype(f32)
    for scale in (0.5, 3.0):
        off = rng.uniform(-scale, scale, (B, 2 * fs * fs, H, W)).astype(f32)
        g1 = torch.zeros((B, C, H, W), device="cuda:0")
        g2 = torch.zeros((B, 2, H, W), device="cuda:0")
        go = torch.zeros((B, 2 * fs * fs, H, W), device="cuda:0")
        if variant == 2:
            err = cabi.filterinterp_backward_defor(variant, gpu(torch, img), gpu(torch, flow), gpu(torch, off), None,
                                                   gpu(torch, gout), g1, g2, go, None)
        else:
            gf = torch.zeros((B, fs * fs, H, W), device="cuda:0")
            err = cabi.filterinterp_backward_defor(variant, gpu(torch, img), gpu(torch, flow), gpu(torch, filt),
                                                   gpu(torch, off), gpu(torch, gout), g1, g2, gf, go)
        assert err == 0
        r1, r2, r3, r4 = oracle.filterinterp_defor_bwd(variant, img, flow, filt, off, gout, fmad=1)
        assert np.abs(cpu(g1) - r1).max() <= GRAD_TOL * max(1.0, np.abs(r1).max())
        assert np.array_equal(cpu(g2), r2)
        assert np.array_equal(cpu(go), r4)
        if variant != 2:
            assert np.array_equal(cpu(gf), r3)
        assert not cpu(go)[0, :, 3, 3].any() and not cpu(g2)[0, :, 3, 3].any()


@pytest.mark.parametrize("variant,fs", [(0, 4), (1, 4), (2, 4), (1, 2)])
def test_deformable_backward_staged_and_flagged_blocks(torch_mod, cabi, oracle, variant, fs):
    """The deformable backward sums a 64x4 block's image-gradient addends in LDS when the block's window fits and leaves the
    block to the per-tap instance when it does not: smooth flow on the left (staged), flows up to +-80 px on the right
    (flagged); C = 4 = one three-channel pass and a remainder; every gradient adds into what its tensor holds (fs = 4 keeps
    the filter / offset sums in registers across channels: same order, same bits)."""
    torch = torch_mod
    rng = np.random.default_rng(170 + 10 * variant + fs)
    B, C, H, W = 1, 4, 24, 200
    img = rng.random((B, C, H, W), dtype=f32)
    flow = smooth_flow(rng, B, H, W, 2.0)
    flow[:, :, :, W // 2:] = rng.uniform(-80, 80, size=(B, 2, H, W - W // 2)).astype(f32)
    filt = rng.random((B, fs * fs, H, W), dtype=f32)
    off = rng.uniform(-1.5, 1.5, (B, 2 * fs * fs, H, W)).astype(f32)
    gout = rng.normal(size=(B, C, H, W)).astype(f32)
    s1 = rng.normal(size=(B, C, H, W)).astype(f32)
    g1, g2 = gpu(torch, s1), torch.zeros((B, 2, H, W), device="cuda:0")
    go = torch.zeros((B, 2 * fs * fs, H, W), device="cuda:0")
    if variant == 2:
        err = cabi.filterinterp_backward_defor(variant, gpu(torch, img), gpu(torch, flow), gpu(torch, off), None,
                                               gpu(torch, gout), g1, g2, go, None)
    else:
        gf = torch.zeros((B, fs * fs, H, W), device="cuda:0")
        err = cabi.filterinterp_backward_defor(variant, gpu(torch, img), gpu(torch, flow), gpu(torch, filt),
                                               gpu(torch, off), gpu(torch, gout), g1, g2, gf, go)
    assert err == 0
    r1, r2, r3, r4 = oracle.filterinterp_defor_bwd(variant, img, flow, filt, off, gout, fmad=1)
    assert np.abs(cpu(g1) - (s1 + r1)).max() <= GRAD_TOL * max(1.0, np.abs(r1).max())
    if fs == 4:     # ... and bit for bit the exact integer sums (tests/bwd_tiles.py), added into s1
        from tests import bwd_tiles
        assert np.array_equal(cpu(g1), bwd_tiles.predict_image_grad("defor", flow, gout, s1, filt, off, variant)[0])
    assert np.array_equal(cpu(g2), r2)
    assert np.array_equal(cpu(go), r4)
    if variant != 2:
        assert np.array_equal(cpu(gf), r3)


def test_two_streams_same_bits_as_one(torch_mod, cabi):
    """`bench.py --streams 2` / INTEGRATION.md: projections on two streams at once (each stream has its own workspace and
    count plane), their consumers ordered by events on the other stream.  Same bits as the same calls on one stream,
    repeated so that the streams really overlap."""
    torch = torch_mod
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(77)
    H, W, C = 192, 320, 8
    flows = [gpu(torch, smooth_flow(rng, 1, H, W, 6.0)) for _ in range(4)]
    depth = gpu(torch, (1e-6 + np.exp(-rng.normal(size=(1, 1, H, W)))).astype(f32))
    ctx = gpu(torch, rng.random((1, C, H, W), dtype=f32))
    filt = gpu(torch, rng.random((1, 16, H, W), dtype=f32))

    def run(two):
        main = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(dev) if two else main
        projs = [torch.zeros((1, 2, H, W), device=dev) for _ in flows]
        outs = [torch.empty_like(ctx) for _ in flows]
        counts = [torch.zeros((1, 1, H, W), device=dev) for _ in range(2)]
        side.wait_stream(main)
        done = []
        for k, fl in enumerate(flows):
            st = side if (k % 2) else main
            with torch.cuda.stream(st):
                assert cabi.depthflowprojection_forward(fl, depth, counts[k % 2], projs[k], 1) == 0
                done.append(st.record_event())
        for k in range(len(flows)):                          # every warp on the stream that did NOT project its flow
            st = main if (k % 2) else side
            with torch.cuda.stream(st):
                st.wait_event(done[k])
                assert cabi.filterinterp_forward_ori(ctx, projs[k], filt, outs[k]) == 0
        main.wait_stream(side)
        torch.cuda.synchronize(dev)
        return [cpu(t) for t in projs + outs]

    ref = run(False)
    for _ in range(5):
        got = run(True)
        assert all(np.array_equal(a, b) for a, b in zip(ref, got))


def test_direction_streams_helper(torch_mod, cabi):
    """fused.DirectionStreams: one stream per flow direction (projection, then two warps that read it), joined at the end;
    the same bits as the calls in a row, over several repetitions."""
    torch = torch_mod
    from vfidkr_amd import fused
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(78)
    H, W, C = 160, 256, 12
    flows = [gpu(torch, smooth_flow(rng, 1, H, W, 5.0)) for _ in range(2)]
    depth = [gpu(torch, (1e-6 + np.exp(-rng.normal(size=(1, 1, H, W)))).astype(f32)) for _ in range(2)]
    ctx = [gpu(torch, rng.random((1, C, H, W), dtype=f32)) for _ in range(2)]
    frame = [gpu(torch, rng.random((1, 3, H, W), dtype=f32)) for _ in range(2)]
    filt = [gpu(torch, rng.random((1, 16, H, W), dtype=f32)) for _ in range(2)]

    def chain(d, res):
        count, proj = torch.zeros((1, 1, H, W), device=dev), torch.zeros((1, 2, H, W), device=dev)
        oc, oi = torch.empty_like(ctx[d]), torch.empty_like(frame[d])
        assert cabi.depthflowprojection_forward(flows[d], depth[d], count, proj, 1) == 0
        assert cabi.filterinterp_forward_ori(ctx[d], proj, filt[d], oc) == 0
        assert cabi.filterinterp_forward_ori(frame[d], proj, filt[d], oi) == 0
        res[d] = (proj, oc, oi)

    ref = {}
    for d in (0, 1):
        chain(d, ref)
    torch.cuda.synchronize(dev)
    lanes = fused.DirectionStreams(dev)
    for _ in range(5):
        got = {}
        lanes.fork()
        for d in (0, 1):
            with lanes.direction(d):
                chain(d, got)
        lanes.join()
        torch.cuda.synchronize(dev)
        for d in (0, 1):
            assert all(torch.equal(a, b) for a, b in zip(ref[d], got[d]))


# ------------------------------------------------------------------ fp16 storage (BASELINE configs[2])

def gpu16(torch, a):
    t = torch.empty(a.shape, dtype=torch.float16, device="cuda:0")
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


# the staged kernel sums the 16 products in one chain: equal to the reference order to fp16 rounding
F16_TOL = 2e-3


@pytest.mark.parametrize("B,C,H,W,fs", [(1, 3, 32, 48, 4), (2, 5, 40, 72, 4), (1, 3, 17, 130, 4), (1, 1, 1, 1, 4),
                                         (1, 2, 3, 5, 4), (1, 196, 20, 70, 4), (1, 3, 24, 40, 5), (1, 2, 9, 7, 2)])
@pytest.mark.parametrize("flow_kind", ["smooth", "uniform1", "wild", "zero", "border"])
def test_filterinterp_f16_storage(torch_mod, cabi, oracle, B, C, H, W, fs, flow_kind):
    torch = torch_mod
    rng = np.random.default_rng(B * 7 + C * 3 + H + W + fs)
    img = rng.random((B, C, H, W), dtype=f32).astype(np.float16)
    filt = (rng.random((B, fs * fs, H, W), dtype=f32) * f32(4.0 / (fs * fs))).astype(f32)      # results stay near [0, 1]
    if flow_kind == "smooth":
        flow = smooth_flow(rng, B, H, W, 3.0) if H > 1 else np.zeros((B, 2, H, W), f32)
    elif flow_kind == "uniform1":
        flow = rng.uniform(-1, 1, (B, 2, H, W)).astype(f32)
    elif flow_kind == "wild":
        flow = rng.uniform(-W / 2, W / 2, (B, 2, H, W)).astype(f32)
    elif flow_kind == "zero":
        flow = np.zeros((B, 2, H, W), f32)
    else:
        flow = np.zeros((B, 2, H, W), f32)
        flow[:, 0] = (W - 1) - np.arange(W)[None, None, :]
        flow[:, 1] = (H - 1) - np.arange(H)[None, :, None]
        flow[:, 0, 1::2] = -np.arange(W)[None, None, :]
    ref = oracle.filterinterp_ori_fwd_f16(img, flow, filt, fmad=1)
    for direct in (True, False):
        out = torch.full((B, C, H, W), float("nan"), dtype=torch.float16, device="cuda:0")
        assert cabi.filterinterp_forward_ori_f16(gpu16(torch, img), gpu(torch, flow), gpu(torch, filt), out, direct=direct) == 0
        got = out.cpu().numpy()
        if direct:
            assert np.array_equal(got, ref), "max diff %g" % np.abs(got.astype(f32) - ref.astype(f32)).max()
        else:
            d = np.abs(got.astype(f32) - ref.astype(f32))
            assert np.all(d <= F16_TOL * np.maximum(1.0, np.abs(ref.astype(f32)))), "max diff %g" % d.max()
    # float32 tensors are refused (no silent conversion)
    with pytest.raises(RuntimeError):
        cabi.filterinterp_forward_ori_f16(gpu(torch, img.astype(f32)), gpu(torch, flow), gpu(torch, filt), out)


def test_filterinterp_f16_views_and_alignment(torch_mod, cabi, oracle):
    """odd row strides / odd offsets cannot be moved as dwords: those calls take the direct kernel."""
    torch = torch_mod
    rng = np.random.default_rng(77)
    B, C, H, W = 1, 3, 20, 66
    big = gpu16(torch, rng.random((B, C + 1, H + 2, W + 3), dtype=f32).astype(np.float16))
    flow_np, filt_np = smooth_flow(rng, B, H, W, 3.0), (rng.random((B, 16, H, W), dtype=f32) * f32(0.25)).astype(f32)
    for x0 in (0, 1, 2):
        img = big[:, 1:, 1:H + 1, x0:x0 + W]
        outbuf = torch.zeros_like(big)
        out = outbuf[:, 1:, 1:H + 1, x0:x0 + W]
        assert cabi.filterinterp_forward_ori_f16(img, gpu(torch, flow_np), gpu(torch, filt_np), out) == 0
        ref = oracle.filterinterp_ori_fwd_f16(img.cpu().numpy(), flow_np, filt_np, fmad=1)
        d = np.abs(out.cpu().numpy().astype(f32) - ref.astype(f32))
        assert np.all(d <= F16_TOL * np.maximum(1.0, np.abs(ref.astype(f32))))
        outbuf[:, 1:, 1:H + 1, x0:x0 + W] = 0
        assert not outbuf.any()


# ------------------------------------------------------------------ projections

@pytest.mark.parametrize("B,H,W", [(1, 32, 48), (2, 17, 70), (1, 1, 1), (1, 40, 200)])
@pytest.mark.parametrize("fillhole", [0, 1])
def test_flowprojection_forward(torch_mod, cabi, oracle, B, H, W, fillhole):
    torch = torch_mod
    rng = np.random.default_rng(H * W)
    flow = smooth_flow(rng, B, H, W, 3.0) if H > 1 else np.zeros((B, 2, H, W), f32)
    for fl, exact in ((flow, False), ((np.round(flow * 8) / 8).astype(f32), True)):
        count = torch.zeros((B, 1, H, W), device="cuda:0")
        out = torch.zeros((B, 2, H, W), device="cuda:0")
        assert cabi.flowprojection_forward(gpu(torch, fl), count, out, fillhole) == 0
        ref, rcount = oracle.flowproj_fwd(fl, fillhole)
        assert np.array_equal(cpu(count), rcount)                    # exact small integers
        if exact:
            assert np.array_equal(cpu(out), ref)                     # dyadic sums: order-free
        else:
            assert np.abs(cpu(out) - ref).max() <= 1e-4
        assert np.array_equal(cpu(out) == 0, ref == 0) or not exact  # identical hole pattern


@pytest.mark.parametrize("fillhole", [0, 1])
def test_depthflowprojection_forward(torch_mod, cabi, oracle, fillhole):
    torch = torch_mod
    rng = np.random.default_rng(3)
    B, H, W = 2, 33, 70
    flow = smooth_flow(rng, B, H, W, 3.0)
    depth = rng.uniform(0.1, 1.0, (B, 1, H, W)).astype(f32)
    count = torch.zeros((B, 1, H, W), device="cuda:0")
    out = torch.zeros((B, 2, H, W), device="cuda:0")
    assert cabi.depthflowprojection_forward(gpu(torch, flow), gpu(torch, depth), count, out, fillhole) == 0
    ref, rcount = oracle.depthflowproj_fwd(flow, depth, fillhole)
    assert np.array_equal(cpu(count) > 0, rcount > 0)
    assert close(cpu(count), rcount, 1e-4) and close(cpu(out), ref, 1e-4)
    # dyadic flow and depth: exact sums -> bit-identical
    fq = (np.round(flow * 8) / 8).astype(f32)
    dq = (np.round(depth * 16) / 16 + 1 / 16).astype(f32)
    count.zero_(), out.zero_()
    assert cabi.depthflowprojection_forward(gpu(torch, fq), gpu(torch, dq), count, out, fillhole) == 0
    ref, rcount = oracle.depthflowproj_fwd(fq, dq, fillhole)
    assert np.array_equal(cpu(count), rcount) and np.array_equal(cpu(out), ref)


@pytest.mark.parametrize("fillhole", [0, 1])
def test_mindepthflowprojection(torch_mod, cabi, oracle, golden_dir, fillhole):
    """Defined result = the reference statements in raster order (largest weight, first source on ties): bit-exact."""
    torch = torch_mod
    rng = np.random.default_rng(17)
    cases = [(2, 33, 70, 3.0, 8), (1, 64, 200, 6.0, 2), (1, 1, 37, 1.0, 4), (1, 41, 1, 1.0, 4), (1, 130, 260, 0.4, 1000)]
    for (B, H, W, sig, levels) in cases:
        flow = smooth_flow(rng, B, H, W, sig) if min(H, W) >= 4 else (rng.standard_normal((B, 2, H, W)) * sig).astype(f32)
        wgt = (np.round(rng.uniform(0.1, 1.0, (B, 1, H, W)) * levels) / levels).astype(f32)   # few levels: many ties
        count = torch.zeros((B, 1, H, W), device="cuda:0")
        out = torch.zeros((B, 2, H, W), device="cuda:0")
        assert cabi.mindepthflowprojection_forward(gpu(torch, flow), gpu(torch, wgt), count, out, fillhole) == 0
        ref, rcount = oracle.mindepthflowproj_fwd(flow, wgt, fillhole)
        assert np.array_equal(cpu(count), rcount) and np.array_equal(cpu(out), ref)
        # backward on the forward's count
        gout = rng.standard_normal((B, 2, H, W)).astype(f32)
        g1 = torch.zeros((B, 2, H, W), device="cuda:0")
        g2 = torch.zeros((B, 1, H, W), device="cuda:0")
        assert cabi.mindepthflowprojection_backward(gpu(torch, flow), gpu(torch, wgt), count, out, gpu(torch, gout), g1, g2) == 0
        assert np.array_equal(cpu(g1), oracle.mindepthflowproj_bwd(flow, wgt, rcount, gout)) and not cpu(g2).any()
    # an incoming count is a floor; negative, zero and NaN weights never register
    B, H, W = 1, 20, 30
    flow = smooth_flow(rng, B, H, W, 2.0)
    wgt = rng.uniform(-0.5, 1.0, (B, 1, H, W)).astype(f32)
    wgt[0, 0, 3, 4] = np.nan
    wgt[0, 0, 5, 6] = 0.0
    count0 = rng.uniform(0.0, 0.6, (B, 1, H, W)).astype(f32)
    count = gpu(torch, count0)
    out = torch.zeros((B, 2, H, W), device="cuda:0")
    assert cabi.mindepthflowprojection_forward(gpu(torch, flow), gpu(torch, wgt), count, out, fillhole) == 0
    ref, rcount = oracle.mindepthflowproj_fwd(flow, wgt, fillhole, count0=count0)
    assert np.array_equal(cpu(count), rcount) and np.array_equal(cpu(out), ref)
    # committed fixture
    g = np.load(os.path.join(golden_dir, "mindepth.npz"))
    count = torch.zeros((2, 1, 19, 27), device="cuda:0")
    out = torch.zeros((2, 2, 19, 27), device="cuda:0")
    assert cabi.mindepthflowprojection_forward(gpu(torch, g["flow"]), gpu(torch, g["weight"]), count, out, fillhole) == 0
    assert np.array_equal(cpu(out), g["out_fh%d" % fillhole]) and np.array_equal(cpu(count), g["count_fh%d" % fillhole])


def test_mindepth_wrapper_mirror(torch_mod, cabi, oracle):
    torch = torch_mod
    from vfidkr_amd.my_package.MinDepthFlowProjection import minDepthFlowProjectionModule
    rng = np.random.default_rng(19)
    B, H, W = 2, 24, 40
    flow_np = smooth_flow(rng, B, H, W, 2.0)
    wgt_np = rng.uniform(0.1, 1.0, (B, 1, H, W)).astype(f32)
    for rg in (False, True):
        o = minDepthFlowProjectionModule(rg)(gpu(torch, flow_np), gpu(torch, wgt_np))
        assert np.array_equal(cpu(o), oracle.mindepthflowproj_fwd(flow_np, wgt_np, 0 if rg else 1)[0])
    fl = gpu(torch, flow_np).requires_grad_(True)
    wg = gpu(torch, wgt_np).requires_grad_(True)
    o = minDepthFlowProjectionModule(True)(fl, wg)
    gout = rng.standard_normal((B, 2, H, W)).astype(f32)
    o.backward(gpu(torch, gout))
    _, rcount = oracle.mindepthflowproj_fwd(flow_np, wgt_np, 0)
    assert np.array_equal(cpu(fl.grad), oracle.mindepthflowproj_bwd(flow_np, wgt_np, rcount, gout))
    assert not cpu(wg.grad).any()


def test_projection_edge_cases(torch_mod, cabi, oracle):
    torch = torch_mod
    H, W = 12, 70
    for fl in (np.full((1, 2, H, W), 100.0, f32),                        # everything leaves the frame
               np.stack([np.full((H, W), 2.0, f32), np.full((H, W), 1.0, f32)])[None]):   # SURVEY case 5
        for fh in (0, 1):
            count = torch.zeros((1, 1, H, W), device="cuda:0")
            out = torch.zeros((1, 2, H, W), device="cuda:0")
            assert cabi.flowprojection_forward(gpu(torch, fl), count, out, fh) == 0
            ref, rcount = oracle.flowproj_fwd(fl, fh)
            assert np.array_equal(cpu(out), ref) and np.array_equal(cpu(count), rcount)


def test_projection_fallback_and_workspace_reuse(torch_mod, cabi, oracle):
    """Fields whose sources reach many tiles overflow the per-tile lists and take the atomic
    fallback; normal and fallback calls alternate on one stream and frame sizes change (the
    workspace is per stream, grown on demand, and its lists must be empty again after each call)."""
    torch = torch_mod
    rng = np.random.default_rng(77)
    for (B, H, W, kind) in ((1, 64, 200, "smooth"), (2, 96, 520, "wild"), (2, 96, 520, "smooth"), (1, 40, 130, "wild"),
                            (1, 200, 700, "smooth"), (1, 64, 200, "rows")):
        if kind == "smooth":
            flow = smooth_flow(rng, B, H, W, 3.0)
        elif kind == "wild":
            flow = rng.uniform(-W / 2, W / 2, (B, 2, H, W)).astype(f32)
        else:       # every source lands in one row of the frame: a few tiles collect everything
            flow = np.zeros((B, 2, H, W), f32)
            flow[:, 1] = 5.0 - np.arange(H)[None, :, None]
        fq = (np.round(flow * 8) / 8).astype(f32)
        depth = (np.round(rng.uniform(0.1, 1.0, (B, 1, H, W)) * 16) / 16 + 1 / 16).astype(f32)
        for fh in (1, 0):
            # NaN-filled, not zero-filled: the library must write (or zero) every element itself
            count = torch.full((B, 1, H, W), float("nan"), device="cuda:0")
            out = torch.full((B, 2, H, W), float("nan"), device="cuda:0")
            assert cabi.flowprojection_forward(gpu(torch, fq), count, out, fh) == 0
            ref, rcount = oracle.flowproj_fwd(fq, fh)
            assert np.array_equal(cpu(count), rcount) and np.array_equal(cpu(out), ref), (B, H, W, kind, fh)
            count.fill_(float("nan")), out.fill_(float("nan"))
            assert cabi.depthflowprojection_forward(gpu(torch, fq), gpu(torch, depth), count, out, fh) == 0
            ref, rcount = oracle.depthflowproj_fwd(fq, depth, fh)
            assert np.array_equal(cpu(count), rcount) and np.array_equal(cpu(out), ref), (B, H, W, kind, fh)


def test_projection_backward(torch_mod, cabi, oracle):
    torch = torch_mod
    rng = np.random.default_rng(21)
    B, H, W = 2, 20, 70
    flow = smooth_flow(rng, B, H, W, 3.0)
    depth = rng.uniform(0.1, 1.0, (B, 1, H, W)).astype(f32)
    gout = rng.normal(size=(B, 2, H, W)).astype(f32)
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


# ------------------------------------------------------------------ FilterInterpolation backward

def test_filterinterp_backward(torch_mod, cabi, oracle):
    torch = torch_mod
    rng = np.random.default_rng(31)
    for (B, C, H, W, fs) in ((2, 3, 20, 70, 4), (1, 2, 12, 20, 5)):
        img = rng.random((B, C, H, W), dtype=f32)
        flow = smooth_flow(rng, B, H, W, 3.0)
        filt = rng.random((B, fs * fs, H, W), dtype=f32)
        gout = rng.normal(size=(B, C, H, W)).astype(f32)
        g1 = torch.zeros((B, C, H, W), device="cuda:0")
        g2 = torch.zeros((B, 2, H, W), device="cuda:0")
        g3 = torch.zeros((B, fs * fs, H, W), device="cuda:0")
        assert cabi.filterinterp_backward_ori(gpu(torch, img), gpu(torch, flow), gpu(torch, filt), gpu(torch, gout),
                                              g1, g2, g3) == 0
        r1, r2, r3 = oracle.filterinterp_ori_bwd(img, flow, filt, gout, fmad=1)
        # image gradient: exact fixed-point sums rounded once (order-free) vs the oracle's sequential fp32 sums
        assert np.abs(cpu(g1) - r1).max() <= GRAD_TOL * max(1.0, np.abs(r1).max())
        assert np.array_equal(cpu(g2), r2)                          # per-pixel, deterministic
        assert np.array_equal(cpu(g3), r3)
        h1 = torch.zeros_like(g1)                                   # ... and reproducible bit for bit
        assert cabi.filterinterp_backward_ori(gpu(torch, img), gpu(torch, flow), gpu(torch, filt), gpu(torch, gout),
                                              h1, torch.zeros_like(g2), torch.zeros_like(g3)) == 0
        assert torch.equal(g1, h1)


def test_filterinterp_backward_staged_and_flagged_tiles(torch_mod, cabi, oracle):
    """The fs=4 backward sums a tile's image-gradient addends in LDS when the tile's window fits and leaves the tile to the
    per-tap kernel when it does not.  Left half of the image: smooth flow (staged tiles); right half: flows up to +-70 px
    (windows far larger than the LDS budget, flagged tiles); C = 7 exercises the three-channel passes with a remainder,
    non-zero starting gradients exercise the accumulate semantics (the reference adds into gradinput1 / gradinput3)."""
    torch = torch_mod
    rng = np.random.default_rng(35)
    B, C, H, W, fs = 2, 7, 40, 200, 4
    img = rng.random((B, C, H, W), dtype=f32)
    flow = smooth_flow(rng, B, H, W, 3.0)
    flow[:, :, :, W // 2:] = rng.uniform(-70, 70, size=(B, 2, H, W - W // 2)).astype(f32)
    filt = rng.random((B, fs * fs, H, W), dtype=f32)
    gout = rng.normal(size=(B, C, H, W)).astype(f32)
    s1 = rng.normal(size=(B, C, H, W)).astype(f32)
    s3 = rng.normal(size=(B, fs * fs, H, W)).astype(f32)
    g1, g2, g3 = gpu(torch, s1), torch.zeros((B, 2, H, W), device="cuda:0"), gpu(torch, s3)
    assert cabi.filterinterp_backward_ori(gpu(torch, img), gpu(torch, flow), gpu(torch, filt), gpu(torch, gout), g1, g2, g3) == 0
    r1, r2, r3 = oracle.filterinterp_ori_bwd(img, flow, filt, gout, fmad=1)
    assert np.abs(cpu(g1) - (s1 + r1)).max() <= GRAD_TOL * max(1.0, np.abs(r1).max())
    from tests import bwd_tiles     # ... and bit for bit the exact integer sums, added into s1
    assert np.array_equal(cpu(g1), bwd_tiles.predict_image_grad("ori", flow, gout, s1, filt)[0])
    assert np.array_equal(cpu(g2), r2)
    # filter gradient: the kernel sums the channels in order starting from the cell's value, as the reference's += does
    want3 = s3.copy()
    for c in range(C):
        want3 = want3 + oracle.filterinterp_ori_bwd(img[:, c:c + 1], flow, filt, gout[:, c:c + 1], fmad=1)[2]
    assert np.array_equal(cpu(g3), want3)
    h1 = gpu(torch, s1)
    assert cabi.filterinterp_backward_ori(gpu(torch, img), gpu(torch, flow), gpu(torch, filt), gpu(torch, gout),
                                          h1, torch.zeros_like(g2), gpu(torch, s3)) == 0
    assert torch.equal(g1, h1)


def test_image_gradient_nonfinite_and_large_inputs(torch_mod, cabi, oracle):
    """The fixed-point image gradient must not turn a NaN / Inf gradoutput into finite numbers (the reference's fp32
    atomics propagate it: divergence checks rely on that) and must not wrap on large filter values or many addends per
    cell.  A non-finite gradoutput or filter switches the call to fp32 atomics: NaN / Inf land in exactly the cells the
    sequential oracle poisons, the finite cells agree; filters of 1e6 and a flow that sends every pixel to one cell stay
    within the usual tolerance."""
    torch = torch_mod
    rng = np.random.default_rng(32)
    B, C, H, W, fs = 1, 2, 24, 40, 4
    img = rng.random((B, C, H, W), dtype=f32)
    flow = smooth_flow(rng, B, H, W, 2.0)
    filt = rng.random((B, fs * fs, H, W), dtype=f32)
    gout = rng.normal(size=(B, C, H, W)).astype(f32)

    def run(img_, flow_, filt_, gout_):
        g1 = torch.zeros((B, C, H, W), device="cuda:0")
        g2 = torch.zeros((B, 2, H, W), device="cuda:0")
        g3 = torch.zeros((B, fs * fs, H, W), device="cuda:0")
        assert cabi.filterinterp_backward_ori(gpu(torch, img_), gpu(torch, flow_), gpu(torch, filt_), gpu(torch, gout_), g1, g2, g3) == 0
        return cpu(g1)

    for bad in (np.nan, np.inf, -np.inf):
        g = gout.copy()
        g[0, 1, 7, 9] = bad
        got = run(img, flow, filt, g)
        ref = oracle.filterinterp_ori_bwd(img, flow, filt, g, fmad=1)[0]
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
        assert np.array_equal(np.sign(got[np.isinf(ref)]), np.sign(ref[np.isinf(ref)]))
        fin = np.isfinite(ref)
        assert fin.sum() > 0.9 * fin.size and (~fin).sum() >= 16          # the poisoned cells are the pixel's own window
        assert np.abs(got[fin] - ref[fin]).max() <= 1e-5 * max(1.0, np.abs(ref[fin]).max())     # fp32 atomics: order-dependent rounding
    f2 = filt.copy()
    f2[0, 3, 5, 5] = np.nan                                                # a non-finite weight poisons its cell too
    got, ref = run(img, flow, f2, gout), oracle.filterinterp_ori_bwd(img, flow, f2, gout, fmad=1)[0]
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref).sum() >= 1
    # large weights: 1e6 x the usual, well past the old 2^10 headroom
    big = (filt * 1.0e6).astype(f32)
    got, ref = run(img, flow, big, gout), oracle.filterinterp_ori_bwd(img, flow, big, gout, fmad=1)[0]
    assert np.abs(got - ref).max() <= GRAD_TOL * max(1.0, np.abs(ref).max())
    # every pixel's window on one spot: H * W * 16 addends in a handful of cells
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    conv = np.stack([(W // 2 - xs).astype(f32), (H // 2 - ys).astype(f32)])[None]
    conv = np.where(np.abs(conv) < np.array([W / 2.0, H / 2.0], f32)[None, :, None, None], conv, 0.0).astype(f32)
    got, ref = run(img, conv, filt, gout), oracle.filterinterp_ori_bwd(img, conv, filt, gout, fmad=1)[0]
    assert np.abs(got - ref).max() <= 5e-5 * max(1.0, np.abs(ref).max())          # ~900 addends per cell: the ORACLE's sequential fp32 sum carries n * 2^-24 of rounding
    # Interpolation's image gradient shares the scheme
    g = gout.copy()
    g[0, 0, 3, 4] = np.nan
    g1 = torch.zeros((B, C, H, W), device="cuda:0")
    g2 = torch.zeros((B, 2, H, W), device="cuda:0")
    assert cabi.interpolation_backward(gpu(torch, img), gpu(torch, flow), gpu(torch, g), g1, g2) == 0
    ref = oracle.interp_bwd(img, flow, g)[0]
    assert np.array_equal(np.isnan(cpu(g1)), np.isnan(ref)) and 1 <= np.isnan(ref).sum() <= 4


# ------------------------------------------------------------------ Interpolation / SeparableConv / SeparableConvFlow

def test_interpolation_forward_backward(torch_mod, cabi, oracle):
    torch = torch_mod
    rng = np.random.default_rng(41)
    B, C, H, W = 2, 5, 20, 70
    img = rng.random((B, C, H, W), dtype=f32)
    flow = smooth_flow(rng, B, H, W, 3.0)
    flow[0, 0, 0, :] = (W - 0.5) - np.arange(W)                     # x2 in (W-1, W): valid for this op only
    gout = rng.normal(size=(B, C, H, W)).astype(f32)
    out = torch.full((B, C, H, W), float("nan"), device="cuda:0")
    assert cabi.interpolation_forward(gpu(torch, img), gpu(torch, flow), out) == 0
    assert np.array_equal(cpu(out), oracle.interp_fwd(img, flow, fmad=1))
    assert cabi.interpolation_forward(gpu(torch, img), gpu(torch, flow), out, require_c3=True) == 1
    g1 = torch.zeros((B, C, H, W), device="cuda:0")
    g2 = torch.zeros((B, 2, H, W), device="cuda:0")
    assert cabi.interpolation_backward(gpu(torch, img), gpu(torch, flow), gpu(torch, gout), g1, g2) == 0
    r1, r2 = oracle.interp_bwd(img, flow, gout, fmad=1)
    assert np.abs(cpu(g1) - r1).max() <= GRAD_TOL * max(1.0, np.abs(r1).max())
    assert np.array_equal(cpu(g2), r2)
    h1 = torch.zeros_like(g1)
    assert cabi.interpolation_backward(gpu(torch, img), gpu(torch, flow), gpu(torch, gout), h1, torch.zeros_like(g2)) == 0
    assert torch.equal(g1, h1)                                      # order-free sums: reproducible bit for bit
    # dyadic inputs: every sum is exact in any order, so the fixed-point result IS the oracle's
    gq = (np.round(gout * 16) / 16).astype(f32)
    fq = np.round(flow * 4) / 4
    fq[0, 0, 0, :] = flow[0, 0, 0, :]
    fq = fq.astype(f32)
    g1.zero_(), g2.zero_()
    assert cabi.interpolation_backward(gpu(torch, img), gpu(torch, fq), gpu(torch, gq), g1, g2) == 0
    assert np.array_equal(cpu(g1), oracle.interp_bwd(img, fq, gq, fmad=1)[0])


def test_interpolation_backward_staged_and_flagged_tiles(torch_mod, cabi, oracle):
    """Interpolation's backward sums a tile's image-gradient addends in LDS when the tile's window fits and leaves the tile
    to the per-tap kernel when it does not: smooth flow on the left half (staged tiles), flows up to +-90 px on the right
    (flagged tiles); C = 4 = one three-channel pass and a remainder; the image gradient adds into what gradinput1 holds."""
    torch = torch_mod
    rng = np.random.default_rng(43)
    B, C, H, W = 2, 4, 36, 200
    img = rng.random((B, C, H, W), dtype=f32)
    flow = smooth_flow(rng, B, H, W, 3.0)
    flow[:, :, :, W // 2:] = rng.uniform(-90, 90, size=(B, 2, H, W - W // 2)).astype(f32)
    gout = rng.normal(size=(B, C, H, W)).astype(f32)
    s1 = rng.normal(size=(B, C, H, W)).astype(f32)
    g1, g2 = gpu(torch, s1), torch.zeros((B, 2, H, W), device="cuda:0")
    assert cabi.interpolation_backward(gpu(torch, img), gpu(torch, flow), gpu(torch, gout), g1, g2) == 0
    r1, r2 = oracle.interp_bwd(img, flow, gout, fmad=1)
    assert np.abs(cpu(g1) - (s1 + r1)).max() <= GRAD_TOL * max(1.0, np.abs(r1).max())
    from tests import bwd_tiles     # ... and bit for bit the exact integer sums, added into s1
    assert np.array_equal(cpu(g1), bwd_tiles.predict_image_grad("interp", flow, gout, s1)[0])
    assert np.array_equal(cpu(g2), r2)
    h1 = gpu(torch, s1)
    assert cabi.interpolation_backward(gpu(torch, img), gpu(torch, flow), gpu(torch, gout), h1, torch.zeros_like(g2)) == 0
    assert torch.equal(g1, h1)


@pytest.mark.parametrize("fs", [1, 5, 13])
def test_separableconv_and_flow(torch_mod, cabi, oracle, fs):
    torch = torch_mod
    rng = np.random.default_rng(50 + fs)
    B, C, H, W = 2, 3, 30, 80
    oh, ow = H - fs + 1, W - fs + 1
    img = rng.random((B, C, H, W), dtype=f32)
    v = rng.random((B, fs, oh, ow), dtype=f32)
    h = rng.random((B, fs, oh, ow), dtype=f32)
    v[0, :, 2, 3] = 0
    gi, gv, gh = gpu(torch, img), gpu(torch, v), gpu(torch, h)
    out = torch.full((B, C, oh, ow), float("nan"), device="cuda:0")
    assert cabi.separableconv_forward(gi, gv, gh, out) == 0
    assert np.array_equal(cpu(out), oracle.sepconv_fwd(img, v, h, fmad=1))
    fo = torch.full((B, 2, oh, ow), float("nan"), device="cuda:0")
    assert cabi.separableconvflow_forward(gi, gv, gh, fo) == 0
    assert np.array_equal(cpu(fo), oracle.sepconvflow_fwd(v, h, H, W, fmad=1))
    assert cpu(fo)[0, 1, 2, 3] == -2000.0
    gout = rng.normal(size=(B, C, oh, ow)).astype(f32)
    g1, g2, g3 = torch.zeros_like(gi), torch.zeros_like(gv), torch.zeros_like(gh)
    assert cabi.separableconv_backward(gi, gv, gh, gpu(torch, gout), g1, g2, g3) == 0
    r1, r2, r3 = oracle.sepconv_bwd(img, v, h, gout)
    assert np.array_equal(cpu(g1), r1)                              # gathered in the sequential loop's order: bit-exact
    assert np.array_equal(cpu(g2), r2) and np.array_equal(cpu(g3), r3)
    gflow = rng.normal(size=(B, 2, oh, ow)).astype(f32)
    g2.zero_(), g3.zero_()
    assert cabi.separableconvflow_backward(gi, gv, gh, gpu(torch, gflow), g2, g3) == 0
    r2, r3 = oracle.sepconvflow_bwd(v, h, gflow, H, W, fmad=1)
    assert np.array_equal(cpu(g2), r2) and np.array_equal(cpu(g3), r3)


# ------------------------------------------------------------------ correlation

@pytest.mark.parametrize("C,H,W,pad,k,md,s1,s2", [(32, 20, 40, 4, 1, 4, 1, 1), (196, 9, 13, 4, 1, 4, 1, 1),
                                                   (7, 8, 33, 4, 1, 4, 1, 1), (5, 12, 14, 3, 3, 4, 1, 2),
                                                   (8, 16, 18, 20, 1, 20, 2, 2), (3, 10, 10, 2, 1, 4, 1, 1),
                                                   # one shape per PWC-configuration kernel: two-pixel 16-byte-staged
                                                   # (aligned rows, >= 64 tiles), one-pixel tiled (unaligned rows),
                                                   # big tiles (unaligned, >= 256 of them); the small ones above are flat
                                                   (6, 32, 128, 4, 1, 4, 1, 1), (19, 41, 256, 4, 1, 4, 1, 1),
                                                   (5, 33, 130, 4, 1, 4, 1, 1), (3, 136, 514, 4, 1, 4, 1, 1),
                                                   # four pixels per lane, three displacement rows per workgroup (aligned
                                                   # rows, >= 512 tiles of 64x4): ragged tiles and a ragged channel chunk; an
                                                   # unpadded call (output origin 4 pixels inside the input)
                                                   (5, 130, 1000, 4, 1, 4, 1, 1), (6, 140, 968, 0, 1, 4, 1, 1)])
def test_correlation_forward(torch_mod, cabi, oracle, C, H, W, pad, k, md, s1, s2):
    torch = torch_mod
    rng = np.random.default_rng(C + H)
    f1 = rng.normal(size=(2, C, H, W)).astype(f32)
    f2 = rng.normal(size=(2, C, H, W)).astype(f32)
    out = cpu(cabi.correlation_forward(gpu(torch, f1), gpu(torch, f2), pad, k, md, s1, s2))
    seq = oracle.correlation_fwd(f1, f2, pad, k, md, s1, s2, order=1, fmad=1)
    assert out.shape == seq.shape
    assert np.array_equal(out, seq)                                 # same sequential channel order
    tree = oracle.correlation_fwd(f1, f2, pad, k, md, s1, s2, order=0, fmad=0)
    assert close(out, tree, 1e-5)                                   # reference's lane/tree order


def test_correlation_backward(torch_mod, cabi, oracle):
    torch = torch_mod
    rng = np.random.default_rng(61)
    # (pad 4, k 1, md 4, strides 1 = PWC-Net's configuration: the pixel-owns-its-gradOutput kernel, incl. ragged tiles, several
    #  channel groups and frames smaller than the halo; anything else: the one-thread-per-element kernel)
    for (C, H, W, pad, k, md, s2) in ((6, 9, 33, 4, 1, 4, 1), (3, 8, 8, 4, 3, 4, 2), (32, 36, 62, 4, 1, 4, 1), (5, 70, 130, 4, 1, 4, 1),
                                      (2, 3, 2, 4, 1, 4, 1), (4, 12, 20, 3, 1, 4, 1)):
        f1 = rng.normal(size=(2, C, H, W)).astype(f32)
        f2 = rng.normal(size=(2, C, H, W)).astype(f32)
        oc, oh, ow = oracle.correlation_out_dims(H, W, pad, k, md, 1, s2)
        g = rng.normal(size=(2, oc, oh, ow)).astype(f32)
        g1, g2 = cabi.correlation_backward(gpu(torch, f1), gpu(torch, f2), gpu(torch, g), pad, k, md, 1, s2)
        r1, r2 = oracle.correlation_bwd(f1, f2, g, pad, k, md, 1, s2)
        assert np.array_equal(cpu(g1), r1) and np.array_equal(cpu(g2), r2)


# ------------------------------------------------------------------ glue either side of the ops

@pytest.mark.parametrize("shape", [(1, 2, 8, 11), (2, 2, 5, 7), (1, 3, 1, 1), (1, 2, 18, 31)])
def test_flow_upsample4_bit_exact(torch_mod, cabi, oracle, shape):
    torch = torch_mod
    rng = np.random.default_rng(sum(shape))
    x = rng.normal(size=shape).astype(f32)
    B, C, hq, wq = shape
    for m0, m1 in ((20.0, 0.5), (20.0, 0.25)):
        out = torch.full((B, C, 4 * hq, 4 * wq), float("nan"), device="cuda:0")
        assert cabi.flow_upsample4(gpu(torch, x), out, m0, m1) == 0
        assert np.array_equal(cpu(out), oracle.flow_upsample4(x, m0, m1, fmad=1))
    # into a channel slice of a larger tensor (zero-copy concat); nothing written outside it
    big = torch.zeros((B, C + 3, 4 * hq, 4 * wq), device="cuda:0")
    assert cabi.flow_upsample4(gpu(torch, x), big[:, 2:2 + C], 20.0, 0.5) == 0
    assert np.array_equal(cpu(big[:, 2:2 + C]), oracle.flow_upsample4(x, 20.0, 0.5, fmad=1))
    big[:, 2:2 + C] = 0
    assert not big.any()
    assert cabi.flow_upsample4(gpu(torch, x), torch.zeros((B, C, 4 * hq, 4 * wq + 1), device="cuda:0"), 1.0, 1.0) == 1


@pytest.mark.parametrize("B,hq,wq", [(1, 8, 12), (2, 5, 18), (1, 1, 1), (1, 10, 50)])
@pytest.mark.parametrize("fillhole", [0, 1])
@pytest.mark.parametrize("depth", [False, True])
def test_projection_from_quarter_flow(torch_mod, cabi, oracle, B, hq, wq, fillhole, depth):
    """fused x4 upsample + splat == the unfused pair bit for bit; the pair agrees with the oracle as before."""
    torch = torch_mod
    rng = np.random.default_rng(hq * wq + B)
    H, W = 4 * hq, 4 * wq
    flow_q = gpu(torch, (rng.normal(size=(B, 2, hq, wq)) * 0.2).astype(f32))
    dep_np = rng.uniform(0.1, 1.0, (B, 1, H, W)).astype(f32)
    dep = gpu(torch, dep_np)
    for m1 in (0.25, 0.5):
        full = torch.empty((B, 2, H, W), device="cuda:0")
        assert cabi.flow_upsample4(flow_q, full, 20.0, m1) == 0
        c_ref = torch.full((B, 1, H, W), float("nan"), device="cuda:0")
        o_ref = torch.full((B, 2, H, W), float("nan"), device="cuda:0")
        c_fus, o_fus = torch.full_like(c_ref, float("nan")), torch.full_like(o_ref, float("nan"))
        if depth:
            assert cabi.depthflowprojection_forward(full, dep, c_ref, o_ref, fillhole) == 0
            assert cabi.depthflowprojection_forward_up4(flow_q, dep, c_fus, o_fus, 20.0, m1, fillhole) == 0
        else:
            assert cabi.flowprojection_forward(full, c_ref, o_ref, fillhole) == 0
            assert cabi.flowprojection_forward_up4(flow_q, c_fus, o_fus, 20.0, m1, fillhole) == 0
        assert torch.equal(c_fus, c_ref) and torch.equal(o_fus, o_ref)
        r_out, r_count = oracle.flowproj_up4_fwd(cpu(flow_q), 20.0, m1, fillhole, dep_np if depth else None, fmad=1)
        if depth:
            assert close(cpu(c_fus), r_count, 1e-4) and close(cpu(o_fus), r_out, 1e-4)
        else:
            assert np.array_equal(cpu(c_fus), r_count) and np.abs(cpu(o_fus) - r_out).max() <= 1e-4


@pytest.mark.parametrize("B,C,H,W,fs", [(1, 3, 32, 48, 4), (2, 3, 17, 70, 4), (1, 2, 12, 20, 5), (1, 1, 1, 1, 4)])
def test_filterinterp_blend(torch_mod, cabi, oracle, B, C, H, W, fs):
    torch = torch_mod
    rng = np.random.default_rng(B + C + H + W + fs)
    ref0, ref2 = rng.random((B, C, H, W), dtype=f32), rng.random((B, C, H, W), dtype=f32)
    flow0 = smooth_flow(rng, B, H, W, 2.0) if H > 1 else np.zeros((B, 2, H, W), f32)
    flow2 = -flow0 + rng.uniform(-0.5, 0.5, flow0.shape).astype(f32)
    flow0[0, 0, 0, 0] = W                                   # one copy-through pixel
    filt0, filt2 = rng.random((B, fs * fs, H, W), dtype=f32), rng.random((B, fs * fs, H, W), dtype=f32)
    for t in (0.5, 0.25, 0.125):
        w0, w2 = float(1.0 - t), float(t)
        blend = torch.full((B, C, H, W), float("nan"), device="cuda:0")
        out0, out2 = torch.full_like(blend, float("nan")), torch.full_like(blend, float("nan"))
        args = [gpu(torch, a) for a in (ref0, ref2, flow0, flow2, filt0, filt2)]
        assert cabi.filterinterp_blend_forward(*args, blend, out0, out2, w0, w2) == 0
        r_blend, r0, r2 = oracle.filterinterp_blend(ref0, ref2, flow0, flow2, filt0, filt2, w0, w2, fmad=1)
        assert np.array_equal(cpu(out0), r0) and np.array_equal(cpu(out2), r2)
        assert np.array_equal(cpu(blend), r_blend)
        only = torch.full_like(blend, float("nan"))
        assert cabi.filterinterp_blend_forward(*args, only, None, None, w0, w2) == 0
        assert torch.equal(only, blend)
    assert cabi.filterinterp_blend_forward(args[0], args[1][:, :, :, :-1] if W > 1 else args[1][:, :0], *args[2:], blend,
                                           out0, out2, 0.5, 0.5) == 1


@pytest.mark.parametrize("align_corners", [True, False])
@pytest.mark.parametrize("shape", [(1, 3, 9, 13), (2, 4, 16, 22), (1, 1, 1, 1), (1, 196, 18, 31)])
def test_pwc_warp_bit_exact(torch_mod, cabi, oracle, shape, align_corners):
    torch = torch_mod
    rng = np.random.default_rng(sum(shape) + int(align_corners))
    B, C, H, W = shape
    feat = rng.normal(size=shape).astype(f32)
    for scale in (0.7, 3.0, 40.0, 1e12):
        flo = (rng.normal(size=(B, 2, H, W)) * scale).astype(f32)
        out = torch.full(shape, float("nan"), device="cuda:0")
        assert cabi.pwc_warp_forward(gpu(torch, feat), gpu(torch, flo), out, align_corners) == 0
        assert np.array_equal(cpu(out), oracle.pwc_warp(feat, flo, align_corners, fmad=1))
    assert cabi.pwc_warp_forward(gpu(torch, feat), gpu(torch, np.zeros((B, 3, H, W), f32)), out, True) == 1


def test_frame_boundary(torch_mod, cabi, oracle):
    torch = torch_mod
    from vfidkr_amd import fused
    rng = np.random.default_rng(11)
    for (b, h, w) in ((2, 9, 14), (1, 37, 130), (1, 1, 1)):
        u8 = rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)
        for pad in ((3, 2, 4, 1), (0, 0, 0, 0), (32, 32, 16, 16)):
            left, right, top, bottom = pad
            dst = torch.full((b, 3, h + top + bottom, w + left + right), float("nan"), device="cuda:0")
            assert cabi.frame_u8_to_planar(torch.from_numpy(u8).cuda(), dst, *pad) == 0
            ref = oracle.frame_to_padded(u8, *pad)
            assert np.array_equal(cpu(dst), ref)
            # back: values below 0, above 1 and exact ties included
            y = (ref * f32(1.3) - f32(0.1)).astype(f32)
            y[..., 0, 0] = f32(0.5) / f32(255.0)
            back = torch.zeros((b, h, w, 3), dtype=torch.uint8, device="cuda:0")
            assert cabi.planar_to_frame_u8(gpu(torch, y), back, top, left) == 0
            assert np.array_equal(back.cpu().numpy(), oracle.padded_to_frame(y, h, w, left, top))
    ties = np.array([-0.2, 0.0, 0.5 / 255, 1.5 / 255, 2.5 / 255, 0.999, 1.0, 7.0], f32).reshape(1, 1, 1, 8).repeat(3, 1)
    back = torch.zeros((1, 1, 8, 3), dtype=torch.uint8, device="cuda:0")
    assert cabi.planar_to_frame_u8(gpu(torch, ties), back, 0, 0) == 0
    assert back.cpu().numpy()[0, 0, :, 0].tolist() == [0, 0, 0, 2, 2, 255, 255, 255]
    # error sums are exact integers; PSNR / interpolation error as demo_MiddleBury.py computes them
    a = rng.integers(0, 256, (2, 33, 65, 3), dtype=np.uint8)
    bb = rng.integers(0, 256, (2, 33, 65, 3), dtype=np.uint8)
    sums = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    assert cabi.frame_error_sums(torch.from_numpy(a).cuda(), torch.from_numpy(bb).cuda(), sums) == 0
    d = a.astype(np.int64) - bb.astype(np.int64)
    assert sums.cpu().tolist() == [int(np.abs(d).sum()), int((d * d).sum())]
    err, psnr = fused.interpolation_error_and_psnr(torch.from_numpy(a).cuda(), torch.from_numpy(bb).cuda())
    r_err, r_psnr = oracle.frame_error(a, bb)
    assert abs(err - r_err) <= 1e-12 and abs(psnr - r_psnr) <= 1e-9
    # the whole boundary through the host mirror: pad, crop back, identical frame, infinite PSNR
    frames = torch.from_numpy(rng.integers(0, 256, (1, 40, 72, 3), dtype=np.uint8)).cuda()
    x, padding = fused.frames_to_padded(frames)
    assert tuple(x.shape) == (1, 3, 128, 128) and padding == (28, 28, 44, 44)
    assert torch.equal(fused.padded_to_frames(x, 40, 72, padding), frames)
    assert fused.interpolation_error_and_psnr(fused.padded_to_frames(x, 40, 72, padding), frames) == (0.0, float("inf"))


def test_correlation_half(torch_mod, cabi, oracle):
    """The reference's at::Half dispatch of correlation forward: bit-exact with the half restatement."""
    torch = torch_mod
    import correlation_cuda
    rng = np.random.default_rng(37)
    for (B, C, H, W, pad, k, md, s1, s2) in ((2, 8, 9, 11, 4, 1, 4, 1, 1), (1, 19, 18, 31, 4, 1, 4, 1, 1),
                                              (1, 5, 12, 14, 3, 3, 2, 1, 2), (1, 3, 10, 10, 4, 1, 4, 2, 2)):
        f1 = rng.standard_normal((B, C, H, W)).astype(np.float16)
        f2 = rng.standard_normal((B, C, H, W)).astype(np.float16)
        a, b = torch.from_numpy(f1).cuda(), torch.from_numpy(f2).cuda()
        want = oracle.correlation_fwd_f16(f1, f2, pad, k, md, s1, s2)
        got = cabi.correlation_forward(a, b, pad, k, md, s1, s2)
        assert got.dtype == torch.float16 and np.array_equal(got.cpu().numpy(), want)
        # through the reference-named module: empty half tensors in, resized by the binding (correlation.py:23-25)
        r1, r2, out = a.new_empty(0), a.new_empty(0), a.new_empty(0)
        assert correlation_cuda.forward(a, b, r1, r2, out, pad, k, md, s1, s2, 1) == 1
        assert out.dtype == torch.float16 and np.array_equal(out.cpu().numpy(), want)
    with pytest.raises(RuntimeError):
        correlation_cuda.forward(a, b.float(), a.new_empty(0), a.new_empty(0), a.new_empty(0), 4, 1, 4, 1, 1, 1)


def test_correlation_half_tiled_kernel(torch_mod, cabi, oracle):
    """PWC-Net's configuration on 8-byte aligned rows takes the tiled half kernel (corr_forward_k1_rows2_f16: packed half
    products, mixed-precision float adds): bit-exact with the half restatement, including half subnormals, products
    that overflow to inf, ragged right / bottom tiles and a channel count that is not a multiple of the LDS chunk."""
    torch = torch_mod
    rng = np.random.default_rng(41)
    for (B, C, H, W) in ((1, 16, 64, 256), (2, 19, 68, 132), (1, 5, 70, 260)):   # 256, 306, 306 16x4 tiles: the tiled kernel
        f1 = rng.standard_normal((B, C, H, W)).astype(np.float16)
        f2 = rng.standard_normal((B, C, H, W)).astype(np.float16)
        f1[:, 0, ::3, ::5] = np.float16(6.0e-8)              # smallest subnormals
        f2[:, 0, 1::3, ::7] = np.float16(3.0e-6)
        f1[:, 1, ::9, 1::4] = np.float16(300.0)              # 300 * 300 > 65504: the rounded product is inf
        f2[:, 1, ::9, 1::4] = np.float16(300.0)
        f2[:, 2, 5::11, 2::6] = np.float16(-0.0)
        want = oracle.correlation_fwd_f16(f1, f2, 4, 1, 4, 1, 1)
        got = cabi.correlation_forward(torch.from_numpy(f1).cuda(), torch.from_numpy(f2).cuda(), 4, 1, 4, 1, 1)
        assert got.dtype == torch.float16
        g = got.cpu().numpy()
        assert np.array_equal(g.view(np.uint16), want.view(np.uint16)), (B, C, H, W)
        assert np.isinf(g).any()


def test_correlation_half_1080p_tiled_equals_one_thread_per_output(torch_mod, cabi):
    """At the PWC pyramid's 1080p level sizes the tiled half kernel and the one-thread-per-output half kernel (taken when
    the maps are not 8-byte aligned: here a view that starts one half into its buffer) return the same bits."""
    torch = torch_mod
    gen = torch.Generator(device="cpu").manual_seed(43)
    for (C, H, W) in ((32, 272, 480), (64, 136, 240), (96, 68, 120)):
        f1 = torch.randn(1, C, H, W, generator=gen).half().cuda()
        f2 = torch.randn(1, C, H, W, generator=gen).half().cuda()
        tiled = cabi.correlation_forward(f1, f2, 4, 1, 4, 1, 1)
        n = f1.numel()
        b1, b2 = torch.empty(n + 1, dtype=torch.float16, device="cuda"), torch.empty(n + 1, dtype=torch.float16, device="cuda")
        u1, u2 = b1[1:].view(1, C, H, W), b2[1:].view(1, C, H, W)
        u1.copy_(f1), u2.copy_(f2)
        assert u1.data_ptr() % 8 != 0
        plain = cabi.correlation_forward(u1, u2, 4, 1, 4, 1, 1)
        assert torch.equal(tiled.view(torch.int16), plain.view(torch.int16))


def test_projection_fallback_scratch_is_cleaned_across_frame_sizes(torch_mod, cabi, oracle):
    """The atomic fallback (a field that scatters a block over more than 64 tiles) leaves sums in the workspace's scratch
    planes, which the NEXT call cleans.  That call may be on a smaller frame: it has to clean what was dirtied, not what
    it would dirty itself -- a large wild field, a small smooth one, a large wild one again, each against the oracle
    (found by tests/soak_projection.py: the third call used to add onto the first one's leftovers)."""
    torch = torch_mod
    rng = np.random.default_rng(77)
    big = (np.round(rng.uniform(-300, 300, (1, 2, 211, 700)) * 8) / 8).astype(f32)
    small = (np.round(rng.uniform(-2, 2, (1, 2, 40, 130)) * 8) / 8).astype(f32)
    big2 = (np.round(rng.uniform(-300, 300, (1, 2, 211, 700)) * 8) / 8).astype(f32)
    for flow in (big, small, big2, small, big):
        B, _, H, W = flow.shape
        for fh in (0, 1):
            count = torch.full((B, 1, H, W), float("nan"), device="cuda:0")
            out = torch.full((B, 2, H, W), float("nan"), device="cuda:0")
            assert cabi.flowprojection_forward(gpu(torch, flow), count, out, fh) == 0
            r, rc = oracle.flowproj_fwd(flow, fh)
            assert np.array_equal(cpu(count), rc)
            assert np.abs(cpu(out) - r).max() <= 1e-4 * max(1.0, np.abs(r).max())


def test_frame_ssim(torch_mod, cabi, oracle):
    """SSIM as demo_MiddleBury.py:382-388 reports it; float32 on the GPU against the float64 oracle."""
    torch = torch_mod
    from vfidkr_amd import fused
    rng = np.random.default_rng(29)
    for (B, h, w, noise) in ((1, 24, 31, 12), (2, 50, 97, 40), (1, 11, 11, 5), (1, 9, 30, 12), (1, 16, 7, 12),
                             (1, 3, 5, 12), (1, 270, 480, 6)):
        gt = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
        if h >= 64:                                          # a smooth frame: flat regions stress the variance terms
            yy, xx = np.mgrid[0:h, 0:w]
            gt = np.stack([(127 + 100 * np.sin(xx / 37.0 + c) * np.cos(yy / 23.0)) for c in range(3)], -1)[None].astype(np.uint8)
        rec = np.clip(gt.astype(np.int32) + rng.integers(-noise, noise + 1, gt.shape), 0, 255).astype(np.uint8)
        got = fused.ssim(torch.from_numpy(rec).cuda(), torch.from_numpy(gt).cuda())
        want = oracle.frame_ssim(rec, gt)
        assert abs(got - want) <= 2e-5, (B, h, w, got, want)
        assert abs(fused.ssim(torch.from_numpy(gt).cuda(), torch.from_numpy(gt).cuda()) - 1.0) <= 1e-6
    # the sum is an order-free integer: two runs agree bit for bit
    a, b = torch.from_numpy(rec).cuda(), torch.from_numpy(gt).cuda()
    s1 = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    s2 = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    assert cabi.frame_ssim_sums(a, b, s1) == 0 and cabi.frame_ssim_sums(a, b, s2) == 0
    assert int(s1.cpu()[0]) == int(s2.cpu()[0]) != 0
    assert cabi.frame_ssim_sums(a[..., :2].contiguous(), b[..., :2].contiguous(), s1) == 1      # not 3 colour planes


def test_fused_host_mirror(torch_mod, cabi, oracle):
    """`fused.py`: the reference helpers' names on the fused entry points."""
    torch = torch_mod
    from vfidkr_amd import fused
    rng = np.random.default_rng(5)
    flow_q = (rng.normal(size=(1, 2, 8, 12)) * 0.2).astype(f32)
    ups = fused.forward_flownets_upsample(gpu(torch, flow_q), 20.0, [0.25, 0.5])
    assert np.array_equal(cpu(ups[1]), oracle.flow_upsample4(flow_q, 20.0, 0.5, fmad=1))
    depth = rng.uniform(0.1, 1.0, (1, 1, 32, 48)).astype(f32)
    proj = fused.FlowProject_from_quarter(gpu(torch, flow_q), 20.0, [0.25, 0.5], gpu(torch, depth))
    r_out, _ = oracle.flowproj_up4_fwd(flow_q, 20.0, 0.5, 1, depth, fmad=1)
    assert close(cpu(proj[1]), r_out, 1e-4)
    ref0, ref2 = rng.random((1, 3, 32, 48), dtype=f32), rng.random((1, 3, 32, 48), dtype=f32)
    filt = rng.random((1, 16, 32, 48), dtype=f32)
    off = [proj[0], proj[1]]
    blend, o0, o2 = fused.FilterInterpolate(gpu(torch, ref0), gpu(torch, ref2), off, [gpu(torch, filt)] * 2, 16, 0.25)
    rb, r0, r2 = oracle.filterinterp_blend(ref0, ref2, cpu(off[0]), cpu(off[1]), filt, filt, 0.75, 0.25, fmad=1)
    assert np.array_equal(cpu(blend), rb) and np.array_equal(cpu(o0), r0) and np.array_equal(cpu(o2), r2)
    feat = rng.normal(size=(1, 8, 32, 48)).astype(f32)
    assert np.array_equal(cpu(fused.warp(gpu(torch, feat), off[0])), oracle.pwc_warp(feat, cpu(off[0]), True, fmad=1))


# ------------------------------------------------------------------ golden fixtures (no oracle involved)

def test_against_golden_fixtures(torch_mod, cabi, golden_dir):
    torch = torch_mod
    g = np.load(os.path.join(golden_dir, "filterinterp.npz"))
    img, flow, filt, off = (gpu(torch, g[k]) for k in ("fi_img", "fi_flow", "fi_filt", "fi_off"))
    out = torch.zeros_like(img)
    assert cabi.filterinterp_forward_ori(img, flow, filt, out) == 0
    assert close(cpu(out), g["fi_out"])
    for v, name in ((0, "offset"), (1, "region"), (2, "nofilter")):
        out.zero_()
        a3, a4 = (off, None) if v == 2 else (filt, off)
        assert cabi.filterinterp_forward_defor(v, img, flow, a3, a4, out) == 0
        assert close(cpu(out), g["fi_out_" + name])
        grads = [torch.zeros_like(t) for t in ((img, flow, off) if v == 2 else (img, flow, filt, off))]
        if v == 2:
            assert cabi.filterinterp_backward_defor(v, img, flow, off, None, gpu(torch, g["fi_gout"]),
                                                    grads[0], grads[1], grads[2], None) == 0
            names = ("gimg", "gflow", "goff")
        else:
            assert cabi.filterinterp_backward_defor(v, img, flow, filt, off, gpu(torch, g["fi_gout"]), *grads) == 0
            names = ("gimg", "gflow", "gfilt", "goff")
        for t, n in zip(grads, names):
            assert close(cpu(t), g["fi_%s_%s" % (n, name)], 1e-4), (name, n)
    out5 = torch.zeros_like(img[:1])
    assert cabi.filterinterp_forward_ori(img[:1].contiguous(), flow[:1].contiguous(), gpu(torch, g["fi5_filt"]), out5) == 0
    assert close(cpu(out5), g["fi5_out"])
    gl = np.load(os.path.join(golden_dir, "glue.npz"))
    up = torch.empty((2, 2, 24, 36), device="cuda:0")
    assert cabi.flow_upsample4(gpu(torch, gl["flow_q"]), up, 20.0, 0.25) == 0
    assert close(cpu(up), gl["up4"])
    for fh in (0, 1):
        cnt, po = torch.empty((2, 1, 24, 36), device="cuda:0"), torch.empty((2, 2, 24, 36), device="cuda:0")
        assert cabi.flowprojection_forward_up4(gpu(torch, gl["flow_q"]), cnt, po, 20.0, 0.25, fh) == 0
        assert np.array_equal(cpu(cnt), gl["proj_up4_count_fh%d" % fh]) and close(cpu(po), gl["proj_up4_fh%d" % fh], 1e-4)
    for ac in (0, 1):
        wo = torch.empty((2, 4, 12, 17), device="cuda:0")
        assert cabi.pwc_warp_forward(gpu(torch, gl["feat"]), gpu(torch, gl["flo"]), wo, bool(ac)) == 0
        assert close(cpu(wo), gl["warp_ac%d" % ac])
    bl = torch.empty((1, 3, 32, 48), device="cuda:0")
    assert cabi.filterinterp_blend_forward(*(gpu(torch, gl[k]) for k in ("ref0", "ref2", "flow0", "flow2", "filt0", "filt2")),
                                           bl, None, None, 0.75, 0.25) == 0
    assert close(cpu(bl), gl["blend"])
    fp = torch.empty((2, 3, 14, 19), device="cuda:0")
    assert cabi.frame_u8_to_planar(torch.from_numpy(gl["frame_u8"]).cuda(), fp, 3, 2, 4, 1) == 0
    assert np.array_equal(cpu(fp), gl["frame_padded"])
    fb = torch.zeros((2, 9, 14, 3), dtype=torch.uint8, device="cuda:0")
    assert cabi.planar_to_frame_u8(gpu(torch, gl["frame_y"]), fb, 4, 3) == 0
    assert np.array_equal(fb.cpu().numpy(), gl["frame_back"])
    g1, g2, g3 = torch.zeros_like(img), torch.zeros_like(flow), torch.zeros_like(filt)
    assert cabi.filterinterp_backward_ori(img, flow, filt, gpu(torch, g["fi_gout"]), g1, g2, g3) == 0
    assert close(cpu(g1), g["fi_gimg"], 1e-4) and close(cpu(g2), g["fi_gflow"], 1e-4) and close(cpu(g3), g["fi_gfilt"], 1e-4)

    g = np.load(os.path.join(golden_dir, "projection.npz"))
    B, _, H, W = g["flow"].shape
    for fh in (0, 1):
        count = torch.zeros((B, 1, H, W), device="cuda:0")
        out = torch.zeros((B, 2, H, W), device="cuda:0")
        assert cabi.flowprojection_forward(gpu(torch, g["flow_q"]), count, out, fh) == 0
        assert np.array_equal(cpu(out), g["outq_fh%d" % fh]) and np.array_equal(cpu(count), g["countq_fh%d" % fh])
        count.zero_(), out.zero_()
        assert cabi.flowprojection_forward(gpu(torch, g["flow"]), count, out, fh) == 0
        assert np.array_equal(cpu(count), g["count_fh%d" % fh]) and np.abs(cpu(out) - g["out_fh%d" % fh]).max() <= 1e-4
        count.zero_(), out.zero_()
        assert cabi.depthflowprojection_forward(gpu(torch, g["flow"]), gpu(torch, g["depth"]), count, out, fh) == 0
        assert close(cpu(out), g["dout_fh%d" % fh], 1e-4) and close(cpu(count), g["dcount_fh%d" % fh], 1e-4)

    g = np.load(os.path.join(golden_dir, "warp_sepconv.npz"))
    img, flow = gpu(torch, g["img"]), gpu(torch, g["flow"])
    out = torch.zeros_like(img)
    assert cabi.interpolation_forward(img, flow, out) == 0
    assert close(cpu(out), g["out"])
    v, h = gpu(torch, g["sep_v"]), gpu(torch, g["sep_h"])
    so = torch.zeros(g["sep_out"].shape, device="cuda:0")
    assert cabi.separableconv_forward(img, v, h, so) == 0
    assert close(cpu(so), g["sep_out"])
    fo = torch.zeros(g["sepflow_out"].shape, device="cuda:0")
    assert cabi.separableconvflow_forward(img, v, h, fo) == 0
    assert close(cpu(fo), g["sepflow_out"])

    g = np.load(os.path.join(golden_dir, "correlation.npz"))
    f1, f2 = gpu(torch, g["f1"]), gpu(torch, g["f2"])
    assert close(cpu(cabi.correlation_forward(f1, f2, 4, 1, 4, 1, 1)), g["out_pwc"])
    assert close(cpu(cabi.correlation_forward(f1, f2, 3, 3, 4, 1, 2)), g["out_k3s2"])
    assert close(cpu(cabi.correlation_forward(f1[:, :8], f2[:, :8], 20, 1, 20, 2, 2)), g["out_flownet"])
    g1, g2 = cabi.correlation_backward(f1, f2, gpu(torch, g["gout_pwc"]), 4, 1, 4, 1, 1)
    assert close(cpu(g1), g["g1_pwc"], 1e-4) and close(cpu(g2), g["g2_pwc"], 1e-4)


# ------------------------------------------------------------------ extension modules + wrapper mirrors (drop-in path)

def test_wrapper_mirrors_match_cabi(torch_mod, cabi, oracle):
    torch = torch_mod
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd.my_package.FilterInterpolation import FilterInterpolationModule, FilterInterpolationDeformableModule
    from vfidkr_amd.my_package.FlowProjection import FlowProjectionModule
    from vfidkr_amd.my_package.DepthFlowProjection import DepthFlowProjectionModule
    from vfidkr_amd.my_package.Interpolation import InterpolationModule
    from vfidkr_amd.my_package.InterpolationCh import InterpolationChModule
    from vfidkr_amd.my_package.SeparableConv import SeparableConvModule
    from vfidkr_amd.my_package.SeparableConvFlow import SeparableConvFlowModule
    from vfidkr_amd.PWCNet.correlation_package_pytorch1_0.correlation import Correlation

    rng = np.random.default_rng(71)
    B, C, H, W = 2, 3, 24, 70
    img_np = rng.random((B, C, H, W), dtype=f32)
    flow_np = smooth_flow(rng, B, H, W, 3.0)
    filt_np = rng.random((B, 16, H, W), dtype=f32)
    off_np = rng.uniform(-1, 1, (B, 32, H, W)).astype(f32)
    depth_np = rng.uniform(0.1, 1.0, (B, 1, H, W)).astype(f32)
    img = gpu(torch, img_np).requires_grad_(True)
    flow = gpu(torch, flow_np).requires_grad_(True)
    filt = gpu(torch, filt_np).requires_grad_(True)

    out = FilterInterpolationModule()(img, flow, filt)
    assert np.array_equal(cpu(out), oracle.filterinterp_ori_fwd(img_np, flow_np, filt_np, fmad=1))
    gout_np = rng.normal(size=(B, C, H, W)).astype(f32)
    out.backward(gpu(torch, gout_np))
    r1, r2, r3 = oracle.filterinterp_ori_bwd(img_np, flow_np, filt_np, gout_np, fmad=1)
    assert np.abs(cpu(img.grad) - r1).max() <= 1e-4
    assert np.array_equal(cpu(flow.grad), r2) and np.array_equal(cpu(filt.grad), r3)

    for mode, variant in (("offset", 0), ("deforconv", 1), ("nofilter", 2)):
        m = FilterInterpolationDeformableModule(mode)
        i2, f2, w2 = (gpu(torch, a).requires_grad_(True) for a in (img_np, flow_np, filt_np))
        o2 = gpu(torch, off_np).requires_grad_(True)
        o = m(i2, f2, o2) if variant == 2 else m(i2, f2, w2, o2)
        assert np.array_equal(cpu(o), oracle.filterinterp_defor_fwd(variant, img_np, flow_np, filt_np, off_np, fmad=1))
        o.backward(gpu(torch, gout_np))
        d1, d2, d3, d4 = oracle.filterinterp_defor_bwd(variant, img_np, flow_np, filt_np, off_np, gout_np, fmad=1)
        assert np.abs(cpu(i2.grad) - d1).max() <= 1e-4
        assert np.array_equal(cpu(f2.grad), d2) and np.array_equal(cpu(o2.grad), d4)
        if variant != 2:
            assert np.array_equal(cpu(w2.grad), d3)

    fq = (np.round(flow_np * 8) / 8).astype(f32)
    # requires_grad=False -> fillhole (inference); True -> no fillhole (FlowProjectionLayer.py:23)
    for rg, fh in ((False, 1), (True, 0)):
        o = FlowProjectionModule(rg)(gpu(torch, fq))
        assert np.array_equal(cpu(o), oracle.flowproj_fwd(fq, fh)[0])
        o = DepthFlowProjectionModule(rg)(gpu(torch, flow_np), gpu(torch, depth_np))
        assert close(cpu(o), oracle.depthflowproj_fwd(flow_np, depth_np, fh)[0], 1e-4)
    fl = gpu(torch, flow_np).requires_grad_(True)
    o = FlowProjectionModule(True)(fl)
    o.backward(torch.ones_like(o))
    assert fl.grad is not None and torch.isfinite(fl.grad).all()     # a source's own targets have count >= 1

    with torch.no_grad():
        assert np.array_equal(cpu(InterpolationModule()(img, flow)), oracle.interp_fwd(img_np, flow_np, fmad=1))
        img5 = gpu(torch, np.concatenate([img_np, img_np[:, :2]], 1))
        assert np.array_equal(cpu(InterpolationChModule()(img5, flow))[:, :3], oracle.interp_fwd(img_np, flow_np, fmad=1))
        fs = 5
        v_np = rng.random((B, fs, H - fs + 1, W - fs + 1), dtype=f32)
        h_np = rng.random((B, fs, H - fs + 1, W - fs + 1), dtype=f32)
        o = SeparableConvModule(fs)(img, gpu(torch, v_np), gpu(torch, h_np))
        assert np.array_equal(cpu(o), oracle.sepconv_fwd(img_np, v_np, h_np, fmad=1))
        o = SeparableConvFlowModule(fs)(img, gpu(torch, v_np), gpu(torch, h_np))
        assert np.array_equal(cpu(o), oracle.sepconvflow_fwd(v_np, h_np, H, W, fmad=1))
        f1 = rng.normal(size=(B, 32, 12, 20)).astype(f32)
        f2 = rng.normal(size=(B, 32, 12, 20)).astype(f32)
        o = Correlation(pad_size=4, kernel_size=1, max_displacement=4, stride1=1, stride2=1, corr_multiply=1)(
            gpu(torch, f1), gpu(torch, f2))
        assert np.array_equal(cpu(o), oracle.correlation_fwd(f1, f2, 4, 1, 4, 1, 1, order=1, fmad=1))
    a = gpu(torch, f1).requires_grad_(True)
    b = gpu(torch, f2).requires_grad_(True)
    o = Correlation(4, 1, 4, 1, 1, 1)(a, b)
    g = rng.normal(size=tuple(o.shape)).astype(f32)
    o.backward(gpu(torch, g))
    r1, r2 = oracle.correlation_bwd(f1, f2, g, 4, 1, 4, 1, 1)
    assert np.array_equal(cpu(a.grad), r1) and np.array_equal(cpu(b.grad), r2)


def test_hip_graph_capture_and_two_streams(torch_mod, cabi, oracle):
    """The entry points only enqueue work on the caller's stream: a sequence of them can be captured into a HIP
    graph after one warm-up call on the capture stream (the projection's per-stream workspace is allocated by that
    call, as include/vfi_hip.h says) and replayed; two streams with their own workspaces run concurrently."""
    torch = torch_mod
    rng = np.random.default_rng(43)
    B, C, H, W = 1, 6, 96, 160
    img = gpu(torch, rng.standard_normal((B, C, H, W)).astype(f32))
    filt = gpu(torch, rng.random((B, 16, H, W), dtype=f32))
    flow_np = smooth_flow(rng, B, H, W, 3.0)
    flow = gpu(torch, flow_np)
    depth = gpu(torch, rng.uniform(0.1, 1.0, (B, 1, H, W)).astype(f32))
    f1 = gpu(torch, rng.standard_normal((B, 16, 24, 40)).astype(f32))
    f2 = gpu(torch, rng.standard_normal((B, 16, 24, 40)).astype(f32))
    count, proj, out = torch.empty((B, 1, H, W), device="cuda:0"), torch.empty_like(flow), torch.empty_like(img)

    def sequence():
        assert cabi.depthflowprojection_forward(flow, depth, count, proj, 1) == 0
        assert cabi.filterinterp_forward_ori(img, proj, filt, out) == 0
        return cabi.correlation_forward(f1, f2, 4, 1, 4, 1, 1)

    corr_eager = sequence()
    torch.cuda.synchronize()
    want_proj, want_out, want_corr = proj.clone(), out.clone(), corr_eager.clone()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sequence()                                           # warm-up on the capture stream: workspace allocation
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        corr_graph = sequence()
    for t in (count, proj, out, corr_graph):
        t.fill_(float("nan"))
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(proj, want_proj) and torch.equal(out, want_out) and torch.equal(corr_graph, want_corr)

    # new inputs in the same buffers: the graph recomputes from what the buffers hold at replay time
    flow.copy_(gpu(torch, smooth_flow(rng, B, H, W, 5.0)))
    graph.replay()
    torch.cuda.synchronize()
    got_proj = proj.clone()
    sequence()
    torch.cuda.synchronize()
    assert torch.equal(proj, got_proj)

    # two streams, each with its own projection workspace, interleaved: same results as alone
    flows = [gpu(torch, smooth_flow(rng, B, H, W, s)) for s in (2.0, 6.0)]
    alone = []
    for fl in flows:
        c, p = torch.empty_like(count), torch.empty_like(proj)
        assert cabi.flowprojection_forward(fl, c, p, 1) == 0
        alone.append((c, p))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    res = [(torch.empty_like(count), torch.empty_like(proj)) for _ in range(2)]
    for rep in range(4):
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                assert cabi.flowprojection_forward(flows[k], res[k][0], res[k][1], 1) == 0
    torch.cuda.synchronize()
    for k in range(2):
        assert torch.equal(res[k][0], alone[k][0]) and torch.equal(res[k][1], alone[k][1])


def test_random_shapes_against_oracle(torch_mod, cabi, oracle):
    """Shapes, batch sizes and flow scales drawn by hypothesis (ragged sizes around the 64-pixel tile edges, 1-pixel
    dimensions, flows from sub-pixel to beyond the frame): every forward of the hot path against the oracle."""
    torch = torch_mod
    from hypothesis import given, settings, strategies as st, HealthCheck

    @settings(max_examples=80, deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)
    @given(st.integers(1, 2), st.integers(1, 5), st.sampled_from([1, 3, 15, 16, 17, 33, 40]),
           st.sampled_from([1, 2, 63, 64, 65, 100, 129]), st.sampled_from([0.0, 0.4, 3.0, 50.0]), st.integers(0, 2 ** 31 - 1))
    def run(B, C, H, W, scale, seed):
        rng = np.random.default_rng(seed)
        img = rng.standard_normal((B, C, H, W)).astype(f32)
        filt = rng.random((B, 16, H, W), dtype=f32)
        flow = (rng.standard_normal((B, 2, H, W)) * scale).astype(f32)
        gi, gf, gk = gpu(torch, img), gpu(torch, flow), gpu(torch, filt)
        ref = oracle.filterinterp_ori_fwd(img, flow, filt, fmad=1)
        for direct in (False, True):
            assert np.array_equal(cpu(run_fi(torch, cabi, gi, gf, gk, direct=direct)), ref)
        off = (rng.standard_normal((B, 32, H, W)) * 0.7).astype(f32)
        go = gpu(torch, off)
        for variant in (0, 1, 2):
            out = torch.full((B, C, H, W), float("nan"), device="cuda:0")
            assert cabi.filterinterp_forward_defor(variant, gi, gf, go if variant == 2 else gk,
                                                   None if variant == 2 else go, out) == 0
            assert np.array_equal(cpu(out), oracle.filterinterp_defor_fwd(variant, img, flow, filt, off, fmad=1))
        fq = (np.round(flow * 8) / 8).astype(f32)                      # dyadic: every sum exact
        wgt = (np.round(rng.uniform(0.1, 1.0, (B, 1, H, W)) * 16) / 16 + 1 / 16).astype(f32)
        for fh in (0, 1):
            count = torch.full((B, 1, H, W), float("nan"), device="cuda:0")
            out = torch.full((B, 2, H, W), float("nan"), device="cuda:0")
            assert cabi.flowprojection_forward(gpu(torch, fq), count, out, fh) == 0
            r, rc = oracle.flowproj_fwd(fq, fh)
            assert np.array_equal(cpu(count), rc) and np.array_equal(cpu(out), r)
            assert cabi.depthflowprojection_forward(gpu(torch, fq), gpu(torch, wgt), count, out, fh) == 0
            r, rc = oracle.depthflowproj_fwd(fq, wgt, fh)
            assert np.array_equal(cpu(count), rc) and np.array_equal(cpu(out), r)
            count.zero_(), out.zero_()
            assert cabi.mindepthflowprojection_forward(gpu(torch, fq), gpu(torch, wgt), count, out, fh) == 0
            r, rc = oracle.mindepthflowproj_fwd(fq, wgt, fh)
            assert np.array_equal(cpu(count), rc) and np.array_equal(cpu(out), r)
        warped = torch.empty_like(gi)
        assert cabi.pwc_warp_forward(gi, gf, warped, True) == 0
        assert np.array_equal(cpu(warped), oracle.pwc_warp(img, flow, True, fmad=1))
        if H >= 1 and W >= 1:
            f2 = rng.standard_normal((B, C, H, W)).astype(f32)
            got = cabi.correlation_forward(gi, gpu(torch, f2), 4, 1, 4, 1, 1)
            assert np.array_equal(cpu(got), oracle.correlation_fwd(img, f2, 4, 1, 4, 1, 1, order=1, fmad=1))

    run()


def test_random_shapes_glue_against_oracle(torch_mod, cabi, oracle):
    """The glue entry points on hypothesis-drawn shapes: x4 upsample, the splat fused with it, both warps +
    blend, the uint8 frame boundary, SSIM, the half correlation."""
    torch = torch_mod
    from vfidkr_amd import fused
    from hypothesis import given, settings, strategies as st, HealthCheck

    @settings(max_examples=40, deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)
    @given(st.integers(1, 2), st.sampled_from([1, 2, 4, 5, 9]), st.sampled_from([1, 3, 16, 17, 33]),
           st.sampled_from([0.25, 0.5, 0.75]), st.integers(0, 2 ** 31 - 1))
    def run(B, hq, wq, t, seed):
        rng = np.random.default_rng(seed)
        H, W = 4 * hq, 4 * wq
        flow_q = (np.round(rng.standard_normal((B, 2, hq, wq)) * 8) / 64).astype(f32)        # dyadic: exact sums
        gq = gpu(torch, flow_q)
        up = torch.empty((B, 2, H, W), device="cuda:0")
        assert cabi.flow_upsample4(gq, up, 16.0, t) == 0
        assert np.array_equal(cpu(up), oracle.flow_upsample4(flow_q, 16.0, t, fmad=1))
        depth = (np.round(rng.uniform(0.1, 1.0, (B, 1, H, W)) * 16) / 16 + 1 / 16).astype(f32)
        for fh in (0, 1):
            for dep in (None, depth):
                count = torch.full((B, 1, H, W), float("nan"), device="cuda:0")
                out = torch.full((B, 2, H, W), float("nan"), device="cuda:0")
                if dep is None:
                    assert cabi.flowprojection_forward_up4(gq, count, out, 16.0, t, fh) == 0
                else:
                    assert cabi.depthflowprojection_forward_up4(gq, gpu(torch, dep), count, out, 16.0, t, fh) == 0
                r, rc = oracle.flowproj_up4_fwd(flow_q, 16.0, t, fh, depth=dep, fmad=1)
                assert np.array_equal(cpu(count), rc) and np.array_equal(cpu(out), r)
        C = 3
        ref0, ref2 = (rng.standard_normal((B, C, H, W)).astype(f32) for _ in range(2))
        fl0, fl2 = ((rng.standard_normal((B, 2, H, W)) * 2).astype(f32) for _ in range(2))
        k0, k2 = (rng.random((B, 16, H, W), dtype=f32) for _ in range(2))
        blend, o0, o2 = (torch.empty((B, C, H, W), device="cuda:0") for _ in range(3))
        assert cabi.filterinterp_blend_forward(gpu(torch, ref0), gpu(torch, ref2), gpu(torch, fl0), gpu(torch, fl2),
                                               gpu(torch, k0), gpu(torch, k2), blend, o0, o2, 1.0 - t, t) == 0
        rb, r0, r2 = oracle.filterinterp_blend(ref0, ref2, fl0, fl2, k0, k2, 1.0 - t, t, fmad=1)
        assert np.array_equal(cpu(blend), rb) and np.array_equal(cpu(o0), r0) and np.array_equal(cpu(o2), r2)
        # frames: pad, back, error sums, SSIM
        u8 = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        pl, pr, pt, pb = (int(v) for v in rng.integers(0, 9, 4))
        padded = torch.empty((B, 3, H + pt + pb, W + pl + pr), device="cuda:0")
        assert cabi.frame_u8_to_planar(torch.from_numpy(u8).cuda(), padded, pl, pr, pt, pb) == 0
        assert np.array_equal(cpu(padded), oracle.frame_to_padded(u8, pl, pr, pt, pb))
        back = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda:0")
        assert cabi.planar_to_frame_u8(padded, back, pt, pl) == 0
        assert np.array_equal(back.cpu().numpy(), u8)
        noisy = np.clip(u8.astype(np.int32) + rng.integers(-9, 10, u8.shape), 0, 255).astype(np.uint8)
        got = fused.ssim(torch.from_numpy(noisy).cuda(), torch.from_numpy(u8).cuda())
        assert abs(got - oracle.frame_ssim(noisy, u8)) <= 3e-5
        h1, h2 = (rng.standard_normal((B, 5, hq + 3, wq + 2)).astype(np.float16) for _ in range(2))
        got = cabi.correlation_forward(torch.from_numpy(h1).cuda(), torch.from_numpy(h2).cuda(), 4, 1, 4, 1, 1)
        assert np.array_equal(got.cpu().numpy(), oracle.correlation_fwd_f16(h1, h2, 4, 1, 4, 1, 1))

    run()


def test_no_cpu_fallback(torch_mod):
    torch = torch_mod
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd.my_package.FilterInterpolation import FilterInterpolationModule
    with pytest.raises(RuntimeError):
        FilterInterpolationModule()(torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8, 8), torch.zeros(1, 16, 8, 8))


# ------------------------------------------------------------------ BASELINE sizes: properties + sampled oracle checks

def test_full_size_1080p(torch_mod, cabi, oracle):
    """cfg3 padded 1152x1984: LDS path == direct path bit for bit on the whole frame (two
    independent code paths), oracle on C=3 and on sampled channels of C=196, identity and
    projection invariants."""
    torch = torch_mod
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import synthetic as S
    H, W = S.padded_size(1080, 1920)
    gen = S.generator()
    frame = S.frames(1, H, W, gen)
    filt = S.filters(1, H, W, gen)
    for model in ("smooth", "quarter"):
        flow = S.flow(1, H, W, 8.0, gen, model)
        gi, gf, gk = frame.cuda(), flow.cuda(), filt.cuda()
        a = run_fi(torch, cabi, gi, gf, gk, direct=False)
        b = run_fi(torch, cabi, gi, gf, gk, direct=True)
        assert torch.equal(a, b)
        ref = oracle.filterinterp_ori_fwd(frame.numpy(), flow.numpy(), filt.numpy(), fmad=1, nthreads=8)
        assert np.array_equal(cpu(a), ref)
        # projection: count is exact; every valid source adds 4
        count = torch.zeros((1, 1, H, W), device="cuda:0")
        out = torch.zeros((1, 2, H, W), device="cuda:0")
        assert cabi.flowprojection_forward(gf, count, out, 1) == 0
        rout, rcount = oracle.flowproj_fwd(flow.numpy(), 1)
        assert np.array_equal(cpu(count), rcount)
        assert np.abs(cpu(out) - rout).max() <= 1e-4
        xs = torch.arange(W)[None, :] + flow[0, 0]
        ys = torch.arange(H)[:, None] + flow[0, 1]
        nvalid = int(((xs >= 0) & (ys >= 0) & (xs <= W - 1) & (ys <= H - 1)).sum())
        assert float(count.double().sum()) == 4.0 * nvalid
    # 196-channel context tensor (DAIN_slowmotion): LDS == direct, oracle on sampled channels
    ctx = S.context(1, 196, H, W, gen)
    gc = ctx.cuda()
    a = run_fi(torch, cabi, gc, gf, gk, direct=False)
    b = run_fi(torch, cabi, gc, gf, gk, direct=True)
    assert torch.equal(a, b)
    sel = [0, 1, 97, 98, 195]
    ref = oracle.filterinterp_ori_fwd(ctx[:, sel].numpy(), flow.numpy(), filt.numpy(), fmad=1, nthreads=8)
    assert np.array_equal(cpu(a[:, sel]), ref)
    # identity: zero flow + one-hot tap (1,1) returns the input exactly
    onehot = torch.zeros_like(gk)
    onehot[:, 5] = 1
    assert torch.equal(run_fi(torch, cabi, gc, torch.zeros_like(gf), onehot), gc)


@pytest.mark.parametrize("raw", [(256, 448), (480, 640), (2160, 3840)])
def test_other_baseline_sizes(torch_mod, cabi, oracle, raw):
    """cfg1/cfg4 (256x448 -> 320x512), cfg2 (480x640 -> 512x704), cfg5 (4K -> 2176x3904): the frame-level ops
    on the whole padded frame; LDS == direct, oracle on the frame, projection count exact, the fused
    quarter-flow projection == the unfused pair."""
    torch = torch_mod
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import fused, synthetic as S
    H, W = S.padded_size(*raw)
    left, right, top, bottom = fused.padding_for(*raw)
    assert (H, W) == (raw[0] + top + bottom, raw[1] + left + right)
    gen = S.generator()
    frame, filt = S.frames(1, H, W, gen), S.filters(1, H, W, gen)
    flow = S.flow(1, H, W, 8.0 * W / 1984.0, gen, "smooth")
    gi, gf, gk = frame.cuda(), flow.cuda(), filt.cuda()
    a = run_fi(torch, cabi, gi, gf, gk, direct=False)
    assert torch.equal(a, run_fi(torch, cabi, gi, gf, gk, direct=True))
    assert np.array_equal(cpu(a), oracle.filterinterp_ori_fwd(frame.numpy(), flow.numpy(), filt.numpy(), fmad=1, nthreads=8))
    count = torch.full((1, 1, H, W), float("nan"), device="cuda:0")
    out = torch.full((1, 2, H, W), float("nan"), device="cuda:0")
    assert cabi.flowprojection_forward(gf, count, out, 1) == 0
    rout, rcount = oracle.flowproj_fwd(flow.numpy(), 1)
    assert np.array_equal(cpu(count), rcount) and np.abs(cpu(out) - rout).max() <= 1e-4
    flow_q = (torch.randn((1, 2, H // 4, W // 4), generator=gen) * 0.3).cuda()
    full = torch.empty((1, 2, H, W), device="cuda:0")
    assert cabi.flow_upsample4(flow_q, full, 20.0, 0.5) == 0
    c2, o2 = torch.empty_like(count), torch.empty_like(out)
    assert cabi.flowprojection_forward(full, count, out, 1) == 0
    assert cabi.flowprojection_forward_up4(flow_q, c2, o2, 20.0, 0.5, 1) == 0
    assert torch.equal(c2, count) and torch.equal(o2, out)
    if raw[0] >= 2160:
        # a 64-channel slice of the 4K context tensor (6.7 GB at C = 196): 64-bit plane offsets
        ctx = S.context(1, 64, H, W, gen).cuda()
        a = run_fi(torch, cabi, ctx, gf, gk, direct=False)
        assert torch.equal(a, run_fi(torch, cabi, ctx, gf, gk, direct=True))
        ref = oracle.filterinterp_ori_fwd(ctx[:, [0, 63]].cpu().numpy(), flow.numpy(), filt.numpy(), fmad=1, nthreads=8)
        assert np.array_equal(cpu(a[:, [0, 63]]), ref)


def test_full_size_1080p_deformable(torch_mod, cabi, oracle):
    """cfg3 frame size, the deformable forwards: the LDS-staged kernel == the general gather kernel bit for bit, with
    small learned offsets (every tile staged) and with huge ones (most tiles take the in-kernel fallback), and the
    oracle on a full-width 160-row band of the same tensors."""
    torch = torch_mod
    import ctypes
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import synthetic as S
    H, W = S.padded_size(1080, 1920)
    gen = S.generator()
    img = S.context(1, 5, H, W, gen).cuda()
    filt = S.filters(1, H, W, gen).cuda()
    flow = S.flow(1, H, W, 8.0, gen, "smooth").cuda()
    for osig in (0.5, 40.0):
        off = (torch.randn((1, 32, H, W), generator=gen) * osig).cuda()
        for variant in (0, 1, 2):
            outs = []
            for general in (False, True):
                out = torch.full_like(img, float("nan"))
                assert cabi.filterinterp_forward_defor(variant, img, flow, off if variant == 2 else filt,
                                                       None if variant == 2 else off, out, general=general) == 0
                outs.append(out)
            assert torch.equal(outs[0], outs[1]), (osig, variant)
            # the oracle on a crop: rows [y0, y1) of the frame depend on rows within the flow + offset reach only when
            # the crop is taken as a frame of its own, so compare on a band whose taps stay inside it: run the op on the
            # band alone (a 160-row frame) and check it against the oracle there
            band = slice(496, 656)
            bi, bf = img[:, :, band].contiguous(), flow[:, :, band].contiguous()
            bk, bo = filt[:, :, band].contiguous(), off[:, :, band].contiguous()
            bout = torch.full_like(bi, float("nan"))
            assert cabi.filterinterp_forward_defor(variant, bi, bf, bo if variant == 2 else bk, None if variant == 2 else bo, bout) == 0
            ref = oracle.filterinterp_defor_fwd(variant, bi.cpu().numpy(), bf.cpu().numpy(), bk.cpu().numpy(), bo.cpu().numpy(), fmad=1)
            assert np.array_equal(cpu(bout), ref), (osig, variant)


def test_full_size_1080p_f16_storage(torch_mod, cabi, oracle):
    """cfg3 with fp16 storage: staged == direct to fp16 rounding on the whole 196-channel tensor,
    the direct kernel == the oracle on sampled channels."""
    torch = torch_mod
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import synthetic as S
    H, W = S.padded_size(1080, 1920)
    gen = S.generator()
    filt = S.filters(1, H, W, gen)
    flow = S.flow(1, H, W, 8.0, gen, "smooth")
    ctx = S.context(1, 196, H, W, gen).to(torch.float16)
    gc, gf, gk = ctx.cuda(), flow.cuda(), filt.cuda()
    a, b = torch.empty_like(gc), torch.empty_like(gc)
    assert cabi.filterinterp_forward_ori_f16(gc, gf, gk, a) == 0
    assert cabi.filterinterp_forward_ori_f16(gc, gf, gk, b, direct=True) == 0
    d = (a.float() - b.float()).abs()
    assert bool((d <= F16_TOL * torch.clamp(b.float().abs(), min=1.0)).all())
    sel = [0, 97, 195]
    ref = oracle.filterinterp_ori_fwd_f16(ctx[:, sel].numpy(), flow.numpy(), filt.numpy(), fmad=1, nthreads=8)
    assert np.array_equal(b[:, sel].cpu().numpy(), ref)


# ------------------------------------------------------------------ BASELINE sizes: the remaining ops (VERDICT r01 gaps)

def test_depthflowprojection_1080p(torch_mod, cabi, oracle):
    """cfg3 (1152x1984), the projection the slow-motion step actually calls: count / flow against the oracle within
    1e-4 (fp32 sum order), identical hole mask; bit-exact on dyadic flow and depth (exact sums in any order)."""
    torch = torch_mod
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import synthetic as S
    H, W = S.padded_size(1080, 1920)
    gen = S.generator()
    for model in ("smooth", "quarter"):
        flow = S.flow(1, H, W, 8.0, gen, model).numpy()
        depth = S.depth_weight(1, H, W, gen).numpy()
        for fl, dp, exact in ((flow, depth, False),
                              ((np.round(flow * 8) / 8).astype(f32), (np.round(depth * 16) / 16 + 1 / 16).astype(f32), True)):
            count = torch.full((1, 1, H, W), float("nan"), device="cuda:0")
            out = torch.full((1, 2, H, W), float("nan"), device="cuda:0")
            assert cabi.depthflowprojection_forward(gpu(torch, fl), gpu(torch, dp), count, out, 1) == 0
            ref, rcount = oracle.depthflowproj_fwd(fl, dp, 1)
            if exact:
                assert np.array_equal(cpu(count), rcount) and np.array_equal(cpu(out), ref), model
            else:
                assert np.array_equal(cpu(count) > 0, rcount > 0)
                assert close(cpu(count), rcount, 1e-4) and close(cpu(out), ref, 1e-4), model


def test_depthflowprojection_wide_weight_range(torch_mod, cabi, oracle):
    """Inverse-depth weights spanning 2^24 inside one tile (depth_inv = 1e-6 + exp(-d), DAIN_slowmotion.py:143): a cell
    that receives only tiny weights keeps its value (normalised by its own tiny count), it does not turn into a hole.
    The fixed-point scale is per output tile, set by the largest weight that reaches the tile: a weight more than
    2^25 below it rounds to nothing -- documented in DESIGN.md; here the range stays inside that."""
    torch = torch_mod
    rng = np.random.default_rng(123)
    B, H, W = 1, 48, 160
    flow = smooth_flow(rng, B, H, W, 2.0)
    depth = np.exp2(-rng.integers(0, 21, (B, 1, H, W)).astype(f32)).astype(f32)          # 2^0 .. 2^-20, dyadic
    depth[:, :, :, 40:90] = np.float32(2.0 ** -20)                                         # a region of only-tiny weights
    fq = (np.round(flow * 8) / 8).astype(f32)
    count = torch.full((B, 1, H, W), float("nan"), device="cuda:0")
    out = torch.full((B, 2, H, W), float("nan"), device="cuda:0")
    assert cabi.depthflowprojection_forward(gpu(torch, fq), gpu(torch, depth), count, out, 1) == 0
    ref, rcount = oracle.depthflowproj_fwd(fq, depth, 1)
    assert np.array_equal(cpu(count) > 0, rcount > 0)                  # no cell lost to the quantisation
    assert close(cpu(count), rcount, 1e-5) and np.abs(cpu(out) - ref).max() <= 1e-4


@pytest.mark.parametrize("raw", [(1080, 1920), (480, 640)])
def test_correlation_pyramid_shapes(torch_mod, cabi, oracle, raw):
    """The five PWC-Net pyramid levels of cfg3 (32@288x496 ... 196@18x31) and cfg2 (32@128x176 ... 196@8x11), both
    directions: the kernels the bench dispatches (rows2 at real tile counts, flat for the coarse levels) against the
    sequential-order oracle bit for bit and the reference's tree order within 1e-5."""
    torch = torch_mod
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import synthetic as S
    H, W = S.padded_size(*raw)
    gen = S.generator()
    oracle.set_num_threads(8)
    for f1, f2 in S.correlation_features(1, H, W, gen):
        for a, b in ((f1, f2), (f2, f1)):
            out = cpu(cabi.correlation_forward(a.cuda(), b.cuda(), 4, 1, 4, 1, 1))
            seq = oracle.correlation_fwd(a.numpy(), b.numpy(), 4, 1, 4, 1, 1, order=1, fmad=1)
            assert np.array_equal(out, seq), tuple(a.shape)
        tree = oracle.correlation_fwd(f2.numpy(), f1.numpy(), 4, 1, 4, 1, 1, order=0, fmad=0)
        assert close(out, tree, 1e-5), tuple(f1.shape)


def test_vimeo64_batch_shapes(torch_mod, cabi, oracle):
    """The batch `bench.py --workload vimeo64` runs (BASELINE configs[3]): B = 3 triplets at 256x448 padded to 320x512, built
    exactly as the bench's VimeoPair builds them -- FilterInterpolation C=3 (staged == direct == oracle, bit for bit),
    FlowProjection with hole filling (count exact, flow <= 1e-4, same hole mask, run-to-run identical) and the 320x512
    correlation pyramid (32@80x128 ... 196@5x8, B = 3: the tiled kernel on the two finest levels, corr_forward_k1_flat on
    the coarse ones) against the sequential-order oracle bit for bit and the reference's tree order within 1e-5."""
    torch = torch_mod
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import synthetic as S
    B = 3
    H, W = S.padded_size(256, 448)
    assert (H, W) == (320, 512)
    gen = S.generator(S.SEED + 1000)
    frames = [S.frames(B, H, W, gen) for _ in range(2)]
    filters = [S.filters(B, H, W, gen) for _ in range(2)]
    flows = [(S.flow(B, H, W, 2.0, gen, "smooth") * 0.5).contiguous() for _ in range(2)]
    feats = S.correlation_features(B, H, W, gen)
    assert [tuple(a.shape[1:]) for a, _ in feats] == [(196, 5, 8), (128, 10, 16), (96, 20, 32), (64, 40, 64), (32, 80, 128)]
    oracle.set_num_threads(8)
    for d in range(2):
        gflow = flows[d].cuda()
        count = torch.full((B, 1, H, W), float("nan"), device="cuda:0")
        proj = torch.full((B, 2, H, W), float("nan"), device="cuda:0")
        assert cabi.flowprojection_forward(gflow, count, proj, 1) == 0
        rproj, rcount = oracle.flowproj_fwd(flows[d].numpy(), 1)
        assert np.array_equal(cpu(count), rcount)
        assert np.abs(cpu(proj) - rproj).max() <= 1e-4
        assert np.array_equal(cpu(count) > 0, rcount > 0)
        c2, p2 = torch.empty_like(count), torch.empty_like(proj)
        assert cabi.flowprojection_forward(gflow, c2, p2, 1) == 0
        assert torch.equal(c2, count) and torch.equal(p2, proj)
        # the warp consumes the projected flow: feed the oracle the GPU's, so that the comparison is exact
        gi, gk = frames[d].cuda(), filters[d].cuda()
        a = run_fi(torch, cabi, gi, proj, gk, direct=False)
        assert torch.equal(a, run_fi(torch, cabi, gi, proj, gk, direct=True))
        assert np.array_equal(cpu(a), oracle.filterinterp_ori_fwd(frames[d].numpy(), cpu(proj), filters[d].numpy(), fmad=1, nthreads=8))
    for f1, f2 in feats:
        for a, b in ((f1, f2), (f2, f1)):
            out = cpu(cabi.correlation_forward(a.cuda(), b.cuda(), 4, 1, 4, 1, 1))
            assert out.shape == (B, 81) + tuple(a.shape[2:])
            seq = oracle.correlation_fwd(a.numpy(), b.numpy(), 4, 1, 4, 1, 1, order=1, fmad=1)
            assert np.array_equal(out, seq), tuple(a.shape)
        tree = oracle.correlation_fwd(f2.numpy(), f1.numpy(), 4, 1, 4, 1, 1, order=0, fmad=0)
        assert close(out, tree, 1e-5), tuple(f1.shape)


def test_f16_storage_staged_kernel_within_one_half_ulp(torch_mod, cabi, oracle):
    """The staged fp16-storage kernel against its DEFINITION (the fp32 op on the widened image, rounded to half once = the
    direct kernel, which is bit-exact with the oracle: test_full_size_1080p_f16_storage) on a 1080p channel set.  The
    staged kernel sums the same 16 products as one folded dot product, so its fp32 value differs from the definition's
    by a few fp32 roundings (< 1e-6 absolute for these inputs) and the two half results differ only where that fp32
    value sits that close to a half rounding boundary: by at most one half ulp of the result (2^-10 |ref|) beyond those
    1e-6, and in well under 0.2 % of the elements (measured: 2.3e-7, 0.047 %) -- three orders of magnitude tighter than
    the 2e-3 relative bound of SURVEY 8(d) that the other fp16 tests use."""
    torch = torch_mod
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import synthetic as S
    H, W = S.padded_size(1080, 1920)
    gen = S.generator()
    filt = S.filters(1, H, W, gen)
    flow = S.flow(1, H, W, 8.0, gen, "smooth")
    ctx = S.context(1, 12, H, W, gen).to(torch.float16)
    gc, gf, gk = ctx.cuda(), flow.cuda(), filt.cuda()
    a, b = torch.empty_like(gc), torch.empty_like(gc)
    assert cabi.filterinterp_forward_ori_f16(gc, gf, gk, a) == 0                   # staged
    assert cabi.filterinterp_forward_ori_f16(gc, gf, gk, b, direct=True) == 0      # the definition
    ref = oracle.filterinterp_ori_fwd_f16(ctx[:, [0, 11]].numpy(), flow.numpy(), filt.numpy(), fmad=1, nthreads=8)
    assert np.array_equal(b[:, [0, 11]].cpu().numpy(), ref)
    d = (a.float() - b.float()).abs()
    excess = float((d - b.float().abs() * 2.0 ** -10).max())
    assert excess <= 1e-6, excess
    frac = float((d != 0).float().mean())
    assert frac <= 2e-3, frac


def test_separableconv_fs51(torch_mod, cabi, oracle):
    """The reference's own SeparableConv size (filter_size 51, my_args.py:35 / test_module.py:904) at its test shape."""
    torch = torch_mod
    rng = np.random.default_rng(51)
    B, C, H, W, fs = 1, 3, 128, 160, 51
    oh, ow = H - fs + 1, W - fs + 1
    img = rng.random((B, C, H, W), dtype=f32)
    v = rng.random((B, fs, oh, ow), dtype=f32)
    h = rng.random((B, fs, oh, ow), dtype=f32)
    gi, gv, gh = gpu(torch, img), gpu(torch, v), gpu(torch, h)
    out = torch.full((B, C, oh, ow), float("nan"), device="cuda:0")
    assert cabi.separableconv_forward(gi, gv, gh, out) == 0
    assert np.array_equal(cpu(out), oracle.sepconv_fwd(img, v, h, fmad=1))
    fo = torch.full((B, 2, oh, ow), float("nan"), device="cuda:0")
    assert cabi.separableconvflow_forward(gi, gv, gh, fo) == 0
    assert np.array_equal(cpu(fo), oracle.sepconvflow_fwd(v, h, H, W, fmad=1))
    gout = rng.normal(size=(B, C, oh, ow)).astype(f32)
    g1, g2, g3 = torch.zeros_like(gi), torch.zeros_like(gv), torch.zeros_like(gh)
    assert cabi.separableconv_backward(gi, gv, gh, gpu(torch, gout), g1, g2, g3) == 0
    r1, r2, r3 = oracle.sepconv_bwd(img, v, h, gout)
    assert np.array_equal(cpu(g1), r1) and np.array_equal(cpu(g2), r2) and np.array_equal(cpu(g3), r3)


def test_projection_workspace_api_and_graph_replay_after_growth(torch_mod, cabi, oracle):
    """vfi_projection_reserve sizes the workspace outside a capture; a graph captured on a small frame stays valid
    after a larger frame has made the library move to a bigger workspace (the old one is retired, not freed), and
    a replay after a call that took the fallback still takes the normal path (no call state lives in kernel
    arguments); vfi_release_workspaces frees everything and the next call allocates afresh."""
    torch = torch_mod
    rng = np.random.default_rng(9)
    B, H, W = 1, 64, 200
    fq = (np.round(smooth_flow(rng, B, H, W, 3.0) * 8) / 8).astype(f32)
    gflow = gpu(torch, fq)
    count = torch.full((B, 1, H, W), float("nan"), device="cuda:0")
    out = torch.full((B, 2, H, W), float("nan"), device="cuda:0")
    ref, rcount = oracle.flowproj_fwd(fq, 1)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert cabi.projection_reserve(B, H, W) == 0
        assert cabi.flowprojection_forward(gflow, count, out, 1) == 0          # warm-up on this stream
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            assert cabi.flowprojection_forward(gflow, count, out, 1) == 0
        # a larger frame on the same stream: the workspace is replaced; then a wild field: the fallback path
        big = (np.round(smooth_flow(rng, 1, 200, 700, 3.0) * 8) / 8).astype(f32)
        bc = torch.empty((1, 1, 200, 700), device="cuda:0")
        bo = torch.empty((1, 2, 200, 700), device="cuda:0")
        assert cabi.flowprojection_forward(gpu(torch, big), bc, bo, 1) == 0
        rb, rbc = oracle.flowproj_fwd(big, 1)
        wild = (np.round(rng.uniform(-350, 350, (1, 2, 200, 700)) * 8) / 8).astype(f32)
        assert cabi.flowprojection_forward(gpu(torch, wild), bc, bo, 1) == 0
        rw, rwc = oracle.flowproj_fwd(wild, 1)
        s.synchronize()
        assert np.array_equal(cpu(bc), rwc) and np.array_equal(cpu(bo), rw)
        for _ in range(2):
            count.fill_(float("nan")), out.fill_(float("nan"))
            g.replay()
            s.synchronize()
            assert np.array_equal(cpu(count), rcount) and np.array_equal(cpu(out), ref)
        del g
    torch.cuda.synchronize()
    assert cabi.release_workspaces() == 0
    assert cabi.flowprojection_forward(gflow, count, out, 1) == 0
    torch.cuda.synchronize()
    assert np.array_equal(cpu(count), rcount) and np.array_equal(cpu(out), ref)


@pytest.mark.parametrize("B,C,H,W,nt", [(1, 5, 40, 200, 3), (2, 3, 33, 70, 2), (1, 7, 64, 130, 4), (1, 4, 20, 66, 5), (1, 3, 17, 64, 1)])
def test_filterinterp_multi_flow(torch_mod, cabi, oracle, B, C, H, W, nt):
    """vfi_filterinterp_forward_ori_multi: one image, one filter, nt flows -> nt outputs, each bit for bit the single-flow
    op (and the oracle): scaled copies of one field as in a slow-motion step, an unrelated field, invalid regions."""
    torch = torch_mod
    rng = np.random.default_rng(B * 1000 + W)
    img = rng.standard_normal((B, C, H, W)).astype(f32)
    filt = rng.random((B, 16, H, W), dtype=f32)
    base = smooth_flow(rng, B, H, W, 6.0)
    flows = [(base * f32((t + 1) / (nt + 1))).astype(f32) for t in range(nt)]
    if nt >= 3:
        flows[-1] = (rng.standard_normal((B, 2, H, W)) * 9.0).astype(f32)           # unrelated, rough
        flows[0][:, :, : H // 2, : W // 3] = 1000.0                                  # copy-through region
    gi, gk = gpu(torch, img), gpu(torch, filt)
    gf = [gpu(torch, f) for f in flows]
    outs = [torch.full((B, C, H, W), float("nan"), device="cuda:0") for _ in range(nt)]
    assert cabi.filterinterp_forward_ori_multi(gi, gf, gk, outs) == 0
    for t in range(nt):
        single = torch.empty_like(gi)
        assert cabi.filterinterp_forward_ori(gi, gf[t], gk, single) == 0
        assert torch.equal(outs[t], single), t
        assert np.array_equal(cpu(outs[t]), oracle.filterinterp_ori_fwd(img, flows[t], filt, fmad=1)), t
    # other filter sizes go through the single-flow kernels
    filt5 = rng.random((B, 25, H, W), dtype=f32)
    outs5 = [torch.full((B, C, H, W), float("nan"), device="cuda:0") for _ in range(min(nt, 2))]
    assert cabi.filterinterp_forward_ori_multi(gi, gf[:len(outs5)], gpu(torch, filt5), outs5) == 0
    for t in range(len(outs5)):
        assert np.array_equal(cpu(outs5[t]), oracle.filterinterp_ori_fwd(img, flows[t], filt5, fmad=1))


def test_filterinterp_multi_flow_1080p(torch_mod, cabi, oracle):
    """The slow-motion shape: 1152x1984, three time offsets of one projected flow, 196 channels (== three single
    launches) and the fused.FilterInterpolate_ctx_all mirror."""
    torch = torch_mod
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import fused, synthetic as S
    H, W = S.padded_size(1080, 1920)
    gen = S.generator()
    ctx = [S.context(1, 196, H, W, gen).cuda() for _ in range(2)]
    filt = [S.filters(1, H, W, gen).cuda() for _ in range(2)]
    base = [S.flow(1, H, W, 8.0, gen, "smooth") for _ in range(2)]
    offs = [[(base[d] * (2.0 * t)).contiguous().cuda() for t in (0.25, 0.5, 0.75)] for d in range(2)]
    pairs = fused.FilterInterpolate_ctx_all(ctx[0], ctx[1], offs, filt)
    single = torch.empty_like(ctx[0])
    for t in range(3):
        for d in range(2):
            assert cabi.filterinterp_forward_ori(ctx[d], offs[d][t], filt[d], single) == 0
            assert torch.equal(pairs[t][d], single), (t, d)
    sel = [0, 97, 195]
    ref = oracle.filterinterp_ori_fwd(ctx[0][:, sel].cpu().numpy(), offs[0][2].cpu().numpy(), filt[0].cpu().numpy(), fmad=1, nthreads=8)
    assert np.array_equal(cpu(pairs[2][0][:, sel]), ref)


@pytest.mark.parametrize("B", [1, 2])
def test_filterinterp_ctx_all_on_channel_slices(torch_mod, cabi, oracle, B):
    """fused.FilterInterpolate_ctx_all on channel slices of a larger tensor -- views with the parent's batch stride (for B = 1
    the stride of a size-1 dimension, which torch leaves arbitrary) whose outputs must keep the view's layout: the three time
    offsets from one launch per direction == three single calls == the oracle."""
    torch = torch_mod
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import fused
    rng = np.random.default_rng(77 + B)
    H, W = 40, 72
    parent = gpu(torch, rng.standard_normal((B, 12, H, W)).astype(f32))
    ctx0, ctx2 = parent[:, 2:7], parent[:, 5:10]
    assert ctx0.stride(0) == 12 * H * W
    filt = [gpu(torch, rng.random((B, 16, H, W), dtype=f32)) for _ in range(2)]
    base = [smooth_flow(rng, B, H, W, 4.0) for _ in range(2)]
    offs = [[gpu(torch, (base[d] * f32(2.0 * t)).astype(f32)) for t in (0.25, 0.5, 0.75)] for d in range(2)]
    pairs = fused.FilterInterpolate_ctx_all(ctx0, ctx2, offs, filt)
    for t in range(3):
        for d, ctx in enumerate((ctx0, ctx2)):
            assert pairs[t][d].stride() == ctx.stride()
            single = torch.empty_strided(ctx.shape, ctx.stride(), dtype=ctx.dtype, device=ctx.device)
            assert cabi.filterinterp_forward_ori(ctx, offs[d][t], filt[d], single) == 0
            assert torch.equal(pairs[t][d], single), (t, d)
            assert np.array_equal(cpu(pairs[t][d]), oracle.filterinterp_ori_fwd(cpu(ctx.contiguous()), cpu(offs[d][t]), cpu(filt[d]), fmad=1)), (t, d)


@pytest.mark.parametrize("shape", [(1, 32, 36, 62), (2, 19, 18, 31), (1, 8, 72, 124), (1, 3, 5, 7), (1, 196, 9, 13)])
@pytest.mark.parametrize("align_corners", [True, False])
def test_pwc_warp_correlation_fused(torch_mod, cabi, oracle, shape, align_corners):
    """warp -> correlation of PWC-Net in one launch == the two launches == the oracle's two functions, bit for bit;
    flows that leave the map (mask 0), land on its edge, and NaN-free rough fields."""
    torch = torch_mod
    B, C, H, W = shape
    rng = np.random.default_rng(C * 100 + W)
    f1 = rng.standard_normal(shape).astype(f32)
    f2 = rng.standard_normal(shape).astype(f32)
    flo = (rng.standard_normal((B, 2, H, W)) * 2.5).astype(f32)
    flo[:, :, 0, :] = 50.0                                            # a row of samples far outside
    flo[:, 0, :, 0] = 0.0                                             # integer positions on the edge
    fused_out = cabi.pwc_warp_correlation_forward(gpu(torch, f1), gpu(torch, f2), gpu(torch, flo), align_corners)
    warped = torch.empty((B, C, H, W), device="cuda:0")
    assert cabi.pwc_warp_forward(gpu(torch, f2), gpu(torch, flo), warped, align_corners) == 0
    two = cabi.correlation_forward(gpu(torch, f1), warped, 4, 1, 4, 1, 1)
    assert torch.equal(fused_out, two)
    ref = oracle.correlation_fwd(f1, oracle.pwc_warp(f2, flo, align_corners, fmad=1), 4, 1, 4, 1, 1, order=1, fmad=1)
    assert np.array_equal(cpu(fused_out), ref)


def test_pwc_warp_correlation_pyramid_1080p(torch_mod, cabi, oracle):
    """the four warped levels of a 1080p pyramid (32@288x496 ... 128@36x62), fused == two launches"""
    torch = torch_mod
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import fused, synthetic as S
    H, W = S.padded_size(1080, 1920)
    gen = S.generator()
    for f1, f2 in S.correlation_features(1, H, W, gen)[1:]:
        h, w = f1.shape[2:]
        flo = (torch.randn((1, 2, h, w), generator=gen) * 1.5).cuda()
        a = fused.warp_corr(f1.cuda(), f2.cuda(), flo, one_launch=True)
        b = fused.warp_corr(f1.cuda(), f2.cuda(), flo)
        assert torch.equal(a, b), tuple(f1.shape)
