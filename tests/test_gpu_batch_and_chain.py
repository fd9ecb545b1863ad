"""`-m gpu` parity tests (round 4): the list form of the projections (`FlowProject(inputs, depth)` in one launch triple),
and the chained harness-level check -- FlowProject -> FilterInterpolate -> blend -> uint8 frame on the GPU only against the
same chain on the oracle only, PSNR as demo_MiddleBury.py:370-378 with SURVEY 8(d)'s thresholds."""
import numpy as np
import pytest

from tests.test_gpu_parity import close, cpu, gpu, smooth_flow, f32, torch_mod, cabi  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _nan(torch, *shape):
    return torch.full(shape, float("nan"), device="cuda:0")


@pytest.mark.parametrize("n,B,H,W", [(2, 1, 32, 48), (3, 2, 17, 70), (6, 1, 40, 200), (9, 1, 33, 130), (1, 1, 1, 1)])
@pytest.mark.parametrize("fillhole", [0, 1])
@pytest.mark.parametrize("depth_mode", ["none", "shared", "per_item"])
def test_projection_batch_equals_single_calls(torch_mod, cabi, oracle, n, B, H, W, fillhole, depth_mode):
    """Every item of a batched call == the single call on that item, bit for bit (same kernels, same tile work), and
    == the oracle within the single call's tolerances.  n = 9 goes as 8 + 1 items; depth shared by all items or one
    per item (DAIN_slowmotion: one per direction)."""
    torch = torch_mod
    rng = np.random.default_rng(n * 1000 + H * W)
    flows = [(smooth_flow(rng, B, H, W, 3.0) * f32(0.5 + 0.25 * i)).astype(f32) if H > 1 else np.zeros((B, 2, H, W), f32)
             for i in range(n)]
    depths = None
    if depth_mode == "shared":
        d = rng.uniform(0.1, 1.0, (B, 1, H, W)).astype(f32)
        depths = [d] * n
    elif depth_mode == "per_item":
        depths = [rng.uniform(0.1, 1.0, (B, 1, H, W)).astype(f32) for _ in range(n)]
    gflows = [gpu(torch, f) for f in flows]
    gdepths = None
    if depths is not None:
        shared = gpu(torch, depths[0])
        gdepths = shared if depth_mode == "shared" else [gpu(torch, d) for d in depths]
    counts = [_nan(torch, B, 1, H, W) for _ in range(n)]
    outs = [_nan(torch, B, 2, H, W) for _ in range(n)]
    assert cabi.flowprojection_forward_batch(gflows, counts, outs, fillhole, gdepths) == 0
    for i in range(n):
        c1, o1 = _nan(torch, B, 1, H, W), _nan(torch, B, 2, H, W)
        if depths is None:
            assert cabi.flowprojection_forward(gflows[i], c1, o1, fillhole) == 0
            ref, rcount = oracle.flowproj_fwd(flows[i], fillhole)
            assert np.array_equal(cpu(counts[i]), rcount)
            assert np.abs(cpu(outs[i]) - ref).max() <= 1e-4
        else:
            gd = gdepths if depth_mode == "shared" else gdepths[i]
            assert cabi.depthflowprojection_forward(gflows[i], gd, c1, o1, fillhole) == 0
            ref, rcount = oracle.depthflowproj_fwd(flows[i], depths[i], fillhole)
            assert np.array_equal(cpu(counts[i]) > 0, rcount > 0)
            assert close(cpu(counts[i]), rcount, 1e-4) and close(cpu(outs[i]), ref, 1e-4)
        assert torch.equal(counts[i], c1) and torch.equal(outs[i], o1), i


def test_projection_batch_mixed_fields_and_fallback(torch_mod, cabi, oracle):
    """Items of one call on very different fields: zero, smooth, uniform(-1,1), all-out-of-frame and a +-W/2 field that
    sends the WHOLE call down the atomic fallback; dyadic values, so every sum is exact in any order: bit-exact with the
    oracle on both paths.  Then a normal call on the same stream: the fallback's scratch planes were cleaned."""
    torch = torch_mod
    rng = np.random.default_rng(77)
    B, H, W = 1, 48, 200
    q = lambda a: (np.round(a * 8) / 8).astype(f32)     # noqa: E731
    fields = [np.zeros((B, 2, H, W), f32), q(smooth_flow(rng, B, H, W, 4.0)), q(rng.uniform(-1, 1, (B, 2, H, W))),
              np.full((B, 2, H, W), 1000.0, f32)]
    wild = q(rng.uniform(-W / 2, W / 2, (B, 2, H, W)))
    for fl in (fields, fields + [wild], fields):
        n = len(fl)
        counts = [_nan(torch, B, 1, H, W) for _ in range(n)]
        outs = [_nan(torch, B, 2, H, W) for _ in range(n)]
        assert cabi.flowprojection_forward_batch([gpu(torch, f) for f in fl], counts, outs, 1) == 0
        for i in range(n):
            ref, rcount = oracle.flowproj_fwd(fl[i], 1)
            assert np.array_equal(cpu(counts[i]), rcount) and np.array_equal(cpu(outs[i]), ref), (n, i)


def test_projection_batch_binding_checks(torch_mod, cabi):
    torch = torch_mod
    B, H, W = 1, 16, 64
    fl = [torch.zeros((B, 2, H, W), device="cuda:0") for _ in range(2)]
    cn = [torch.zeros((B, 1, H, W), device="cuda:0") for _ in range(2)]
    out = [torch.zeros((B, 2, H, W), device="cuda:0") for _ in range(2)]
    assert cabi.flowprojection_forward_batch(fl, cn, out, 1) == 0
    assert cabi.flowprojection_forward_batch(fl, [cn[0], cn[0]], out, 1) == 1          # shared count plane
    assert cabi.flowprojection_forward_batch(fl, cn, [out[0], out[0]], 1) == 1          # shared output
    assert cabi.flowprojection_forward_batch(fl, cn[:1], out, 1) == 1                   # list lengths
    assert cabi.flowprojection_forward_batch([fl[0], torch.zeros((B, 2, H, W + 4), device="cuda:0")], cn, out, 1) == 1
    assert cabi.flowprojection_forward_batch([], [], [], 1) == 1
    with pytest.raises(RuntimeError):
        cabi.flowprojection_forward_batch([f.cpu() for f in fl], cn, out, 1)


def test_projection_batch_1080p_and_graph_replay(torch_mod, cabi, oracle):
    """The slow-motion step's six DepthFlowProjection calls (2 directions x 3 time offsets, each direction its own depth)
    as ONE call at 1152x1984: bit-identical with the six single calls, run-to-run bitwise, replayable from a HIP graph
    (pointer tables are kernel arguments), one item against the oracle."""
    torch = torch_mod
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import synthetic as S, fused
    H, W = S.padded_size(1080, 1920)
    gen = S.generator()
    base = [S.flow(1, H, W, 8.0, gen, "smooth") for _ in range(2)]
    depth = [S.depth_weight(1, H, W, gen) for _ in range(2)]
    times = (0.25, 0.5, 0.75)
    flows = [[(base[d] * (2.0 * t)).contiguous().cuda() for t in times] for d in range(2)]
    gdepth = [d.cuda() for d in depth]
    flat = flows[0] + flows[1]
    dlist = [gdepth[0]] * 3 + [gdepth[1]] * 3
    single = []
    for f, d in zip(flat, dlist):
        c, o = _nan(torch, 1, 1, H, W), _nan(torch, 1, 2, H, W)
        assert cabi.depthflowprojection_forward(f, d, c, o, 1) == 0
        single.append((c, o))
    counts = [_nan(torch, 1, 1, H, W) for _ in flat]
    outs = [_nan(torch, 1, 2, H, W) for _ in flat]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert cabi.projection_reserve(len(flat), H, W) == 0
        assert cabi.flowprojection_forward_batch(flat, counts, outs, 1, dlist) == 0
        s.synchronize()
        for i, (c, o) in enumerate(single):
            assert torch.equal(counts[i], c) and torch.equal(outs[i], o), i
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            assert cabi.flowprojection_forward_batch(flat, counts, outs, 1, dlist) == 0
        for _ in range(2):
            for c, o in zip(counts, outs):
                c.fill_(float("nan")), o.fill_(float("nan"))
            g.replay()
            s.synchronize()
            for i, (c, o) in enumerate(single):
                assert torch.equal(counts[i], c) and torch.equal(outs[i], o), i
        del g
    torch.cuda.synchronize()
    ref, rcount = oracle.depthflowproj_fwd(flat[4].cpu().numpy(), depth[1].numpy(), 1)
    assert np.array_equal(cpu(counts[4]) > 0, rcount > 0)
    assert close(cpu(counts[4]), rcount, 1e-4) and close(cpu(outs[4]), ref, 1e-4)
    # the host mirror of the networks' two FlowProject calls
    both = fused.FlowProject_directions(flows, gdepth)
    torch.cuda.synchronize()
    for d in range(2):
        for ti in range(3):
            assert torch.equal(both[d][ti], single[3 * d + ti][1])
    # FlowProjection (no depth), both directions of DAIN x2 in one call == two calls
    two = fused.FlowProject_directions([[flows[0][1]], [flows[1][1]]])
    for d in range(2):
        c, o = _nan(torch, 1, 1, H, W), _nan(torch, 1, 2, H, W)
        assert cabi.flowprojection_forward(flows[d][1], c, o, 1) == 0
        assert torch.equal(two[d][0], o)


@pytest.mark.parametrize("model", ["smooth", "quarter"])
def test_chain_psnr_1080p(torch_mod, cabi, oracle, model):
    """SURVEY 8(d) harness-level parity at 1152x1984: one interpolated frame of DAIN_slowmotion made by the GPU chain only
    (FlowProject of both directions -> FilterInterpolate -> blend -> uint8 frame) against the oracle chain only
    (oracle/chain.py), same inputs.  The projected flows differ in the last bits (sum order), and a difference that
    straddles an integer moves a warp window by a whole pixel: PSNR of the uint8 frames (demo_MiddleBury.py:370-378) is the
    measure.  fp32 >= 60 dB; fp16 storage (frames and warped frames stored as half, BASELINE configs[2]) >= 45 dB."""
    torch = torch_mod
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import synthetic as S, fused
    from oracle import chain
    h, w = 1080, 1920
    H, W = S.padded_size(h, w)
    left, right, top, bottom = fused.padding_for(h, w)
    assert (H, W) == (h + top + bottom, w + left + right)
    gen = S.generator(4242)
    t = 0.25
    frames = [S.frames(1, H, W, gen) for _ in range(2)]
    filters = [S.filters(1, H, W, gen) for _ in range(2)]
    depths = [S.depth_weight(1, H, W, gen) for _ in range(2)]
    base = [S.flow(1, H, W, 8.0, gen, model) for _ in range(2)]
    flows = [(base[0] * (2.0 * t)).contiguous(), (base[1] * (2.0 * (1.0 - t))).contiguous()]
    ctx = [S.context(1, 6, H, W, gen) for _ in range(2)]
    ref = chain.unit([f.numpy() for f in frames], [f.numpy() for f in flows], [d.numpy() for d in depths],
                     [k.numpy() for k in filters], t, h, w, left, top, nthreads=8, ctx=[c.numpy() for c in ctx])

    gfr, gfl, gd, gk = ([x.cuda() for x in v] for v in (frames, flows, depths, filters))
    proj = fused.FlowProject_directions([[gfl[0]], [gfl[1]]], gd)
    p0, p2 = proj[0][0], proj[1][0]
    blend, _, _ = fused.FilterInterpolate(gfr[0], gfr[1], [p0, p2], gk, 16, t)
    u8 = fused.padded_to_frames(blend, h, w, (left, right, top, bottom))
    gctx = fused.FilterInterpolate_ctx_all(ctx[0].cuda(), ctx[1].cuda(), [[p0], [p2]], gk)[0]
    torch.cuda.synchronize()

    # the projections: within the op's tolerance; how many window origins a last-bit difference moves
    flips, dmax = 0, 0.0
    for d, p in enumerate((p0, p2)):
        assert close(cpu(p), ref["proj"][d], 1e-4)
        flips += chain.int_flips(cpu(p), ref["proj"][d])
        dmax = max(dmax, float(np.abs(cpu(p) - ref["proj"][d]).max()))
    psnr = chain.psnr_u8(cpu(u8), ref["u8"])
    differing = int(np.count_nonzero(cpu(u8) != ref["u8"]))
    print("chain parity (%s): PSNR %.2f dB, %d of %d uint8 values differ, %d window origins moved"
          % (model, psnr, differing, ref["u8"].size, flips))
    assert psnr >= 60.0
    # a moved window origin changes that pixel only; everywhere else the bilinear fractions differ in their last bits,
    # which can move a value across a rounding boundary by one level at most
    big = np.abs(cpu(u8).astype(np.int32) - ref["u8"].astype(np.int32)) > 1
    assert np.count_nonzero(np.any(big, axis=3)) <= flips
    # the context warps likewise: a difference d of the projected flow moves a bilinear fraction by d, i.e. the value by at
    # most d x (the four quadrant sums' spread: 16 taps of weight < 1 on N(0, 1) values)
    for d in range(2):
        bad = np.any(np.abs(cpu(gctx[d]) - ref["ctx"][d]) > (1e-5 + 100.0 * dmax) * np.maximum(1.0, np.abs(ref["ctx"][d])), axis=1)
        assert np.count_nonzero(bad) <= flips

    # fp16 storage: frames in, warped frames out as half; flows, filters, depth and all arithmetic fp32
    o0 = torch.empty((1, 3, H, W), device="cuda:0", dtype=torch.float16)
    o2 = torch.empty_like(o0)
    assert cabi.filterinterp_forward_ori_f16(gfr[0].half(), p0, gk[0], o0) == 0
    assert cabi.filterinterp_forward_ori_f16(gfr[1].half(), p2, gk[1], o2) == 0
    blend16 = (o0.float() * (1.0 - t) + o2.float() * t).half().float()
    u16 = fused.padded_to_frames(blend16.contiguous(), h, w, (left, right, top, bottom))
    torch.cuda.synchronize()
    psnr16 = chain.psnr_u8(cpu(u16), ref["u8"])
    print("chain parity (%s), fp16 storage: PSNR %.2f dB" % (model, psnr16))
    assert psnr16 >= 45.0


def _dfp_report(torch, cabi, oracle, flow, depth, label):
    H, W = flow.shape[2:]
    count = _nan(torch, 1, 1, H, W)
    out = _nan(torch, 1, 2, H, W)
    assert cabi.depthflowprojection_forward(gpu(torch, flow), gpu(torch, depth), count, out, 1) == 0
    ref, rcount = oracle.depthflowproj_fwd(flow, depth, 1)
    o, c = cpu(out), cpu(count)
    err = np.abs(o - ref) / np.maximum(1.0, np.abs(ref))
    cerr = np.abs(c - rcount) / np.maximum(1.0, np.abs(rcount))
    print("%s: |flow| max %.1f px; output max err (rel to max(1,|ref|)) %.3g, count %.3g, cells over 1e-4: %d of %d"
          % (label, float(np.abs(flow).max()), float(err.max()), float(cerr.max()), int(np.count_nonzero(err > 1e-4)), err.size))
    assert np.array_equal(c > 0, rcount > 0)
    return float(err.max()), float(cerr.max())


def test_depthflowprojection_4k_and_large_flows(torch_mod, cabi, oracle):
    """SURVEY 8(d)'s tolerance for DepthFlowProjection is 1e-4 relative.  BASELINE configs[4]: 2176x3904 with sigma = 16 px
    scaled by 2t = 1.5 (the largest time offset of a slow-motion step), smooth and quarter fields: met (1.4e-5 / 1.9e-5).
    Beyond the networks' range -- a field with flows up to 256 px at 1080p, a quarter of the frame at 1/64 of that -- the
    fixed-point sums bound a cell's error by 2^(e - 20) px, 2^e > the largest |fx| (|fy|) that reaches the cell's tile: the
    handful of cells where +250 px and -250 px addends cancel to a value below 1 px come out 1.6e-4 off (the reference's fp32
    sums keep ~1e-5 there).  Asserted: the documented bound, and that such cells are fewer than one in 10^5."""
    torch = torch_mod
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import synthetic as S
    gen = S.generator(99)
    H, W = S.padded_size(2160, 3840)
    flow = (S.flow(1, H, W, 16.0, gen, "smooth") * 1.5).contiguous().numpy()
    depth = S.depth_weight(1, H, W, gen).numpy()
    e4k, c4k = _dfp_report(torch, cabi, oracle, flow, depth, "4K smooth x 1.5")
    flowq = (S.flow(1, H, W, 16.0, gen, "quarter") * 1.5).contiguous().numpy()
    eq, cq = _dfp_report(torch, cabi, oracle, flowq, depth, "4K quarter x 1.5")
    assert max(e4k, eq) <= 1e-4 and max(c4k, cq) <= 1e-4
    H, W = S.padded_size(1080, 1920)
    big = S.flow(1, H, W, 8.0, gen, "smooth").numpy()
    big = (big * (256.0 / np.abs(big).max())).astype(f32)           # flows up to 256 px, slowly varying
    # (a quarter of the frame keeps small flows: small values beside large ones inside the tiles along the seam)
    big[:, :, :, : W // 4] *= f32(1.0 / 64.0)
    depth2 = S.depth_weight(1, H, W, gen).numpy()
    eb, cb = _dfp_report(torch, cabi, oracle, big, depth2, "1080p, flows to 256 px")
    assert eb <= 2.0 ** (9 - 20) and cb <= 1e-4
    count = _nan(torch, 1, 1, H, W)
    out = _nan(torch, 1, 2, H, W)
    assert cabi.depthflowprojection_forward(gpu(torch, big), gpu(torch, depth2), count, out, 1) == 0
    ref, _ = oracle.depthflowproj_fwd(big, depth2, 1)
    over = np.count_nonzero(np.abs(cpu(out) - ref) > 1e-4 * np.maximum(1.0, np.abs(ref)))
    assert over <= ref.size // 100000


@pytest.mark.parametrize("shape", [(1, 196, 18, 31), (1, 128, 36, 62), (2, 96, 72, 124), (1, 64, 144, 248), (1, 32, 288, 496),
                                   (1, 7, 9, 13), (3, 16, 20, 44), (2, 5, 33, 130), (1, 3, 136, 514)])
def test_correlation_pair_equals_two_calls(torch_mod, cabi, oracle, shape):
    """Both directions of a pyramid level in one launch == the two single calls bit for bit (all five 1080p level shapes, a
    batch, unaligned widths), and == the oracle on the smallest.  The last two shapes are unaligned and take the pair through
    the two kernels the others do not reach: corr_forward_k1_rows (324 tiles of 16x4, 100 of 32x8) and corr_forward_k1<4,32,8>
    (578 tiles of 32x8); test_correlation_forward pins their single calls to the oracle."""
    torch = torch_mod
    from vfidkr_amd import fused
    B, C, H, W = shape
    rng = np.random.default_rng(C * H)
    t = [gpu(torch, rng.standard_normal((B, C, H, W)).astype(f32)) for _ in range(4)]
    oa, ob = fused.corr_pair(t[0], t[1], t[2], t[3])
    ra = cabi.correlation_forward(t[0], t[1], 4, 1, 4, 1, 1)
    rb = cabi.correlation_forward(t[2], t[3], 4, 1, 4, 1, 1)
    assert torch.equal(oa, ra) and torch.equal(ob, rb)
    if H * W <= 600:
        ref = oracle.correlation_fwd(cpu(t[2]), cpu(t[3]), 4, 1, 4, 1, 1, order=1, fmad=1)      # sequential channel order
        assert np.array_equal(cpu(ob), ref)
    # a view at an odd element offset of its storage (the tiled kernel's 8-byte stores need an aligned output)
    if W % 4 == 0:
        assert torch.equal(cabi.correlation_forward(t[0], t[1], 4, 1, 4, 1, 1), ra)


def test_image_gradient_headroom_when_every_tap_lands_on_one_cell(torch_mod, cabi, oracle):
    """border clamping folds several of the fs x fs taps of a pixel onto one cell, so a corner cell can receive
    more addends than the frame has pixels -- the 64-bit fixed-point scale leaves room for (frame pixels x taps).  Deformable
    region variant, fs = 6, the top-left quarter of the frame flowing onto pixel (0, 0) -- the largest convergence the
    validity test |f| < w / 2 allows: nine of its 36 clamped taps per pixel on cell (0, 0) -- with gradoutput and weights
    uniformly at their maxima: the sums must come out as the oracle's, not wrapped."""
    torch = torch_mod
    B, C, H, W, fs = 1, 1, 24, 40, 6
    xs, ys = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
    flow = np.stack([np.where(xs < W // 2, -xs, 0.0), np.where(ys < H // 2, -ys, 0.0)])[None].astype(f32)
    img = np.ones((B, C, H, W), f32)
    filt = np.full((B, fs * fs, H, W), 4.0, f32)
    off = np.zeros((B, 2 * fs * fs, H, W), f32)
    gout = np.full((B, C, H, W), 8.0, f32)
    g = [torch.zeros(s, device="cuda:0") for s in (img.shape, flow.shape, filt.shape, off.shape)]
    assert cabi.filterinterp_backward_defor(cabi.DEFOR_REGION, gpu(torch, img), gpu(torch, flow), gpu(torch, filt), gpu(torch, off),
                                            gpu(torch, gout), g[0], g[1], g[2], g[3]) == 0
    ref = oracle.filterinterp_defor_bwd(cabi.DEFOR_REGION, img, flow, filt, off, gout, fmad=1)
    assert np.all(np.isfinite(cpu(g[0])))
    assert close(cpu(g[0]), ref[0], 1e-5)


def test_double_tensors_are_refused_like_the_reference_wrappers_would(torch_mod, cabi):
    """The reference's launchers are instantiated for double as well (AT_DISPATCH_FLOATING_TYPES), but its Layer wrappers hand them
    `torch.cuda.FloatTensor` outputs (FilterInterpolationLayer.py:34, FlowProjectionLayer.py:35-36), so a double input cannot get
    through the reference's own call path either (`output.data<double>()` on a float tensor throws).  Decision (VERDICT r03
    item 8): float32 only; a double tensor is an immediate, loud error -- from the pybind modules and from the ctypes layer --
    never a silent float computation."""
    torch = torch_mod
    import filterinterpolation_cuda
    import flowprojection_cuda
    img = torch.zeros((1, 3, 16, 64), device="cuda:0", dtype=torch.float64)
    flow = torch.zeros((1, 2, 16, 64), device="cuda:0", dtype=torch.float64)
    filt = torch.zeros((1, 16, 16, 64), device="cuda:0", dtype=torch.float64)
    out = torch.zeros_like(img)
    with pytest.raises(RuntimeError, match="float32"):
        filterinterpolation_cuda.FilterInterpolationLayer_gpu_forward_ori(img, flow, filt, out)
    with pytest.raises(RuntimeError, match="float32"):
        flowprojection_cuda.FlowProjectionLayer_gpu_forward(flow, torch.zeros((1, 1, 16, 64), device="cuda:0", dtype=torch.float64),
                                                           torch.zeros_like(flow), 1)
    with pytest.raises(RuntimeError, match="float32"):
        cabi.filterinterp_forward_ori(img, flow, filt, out)
    with pytest.raises(RuntimeError, match="float32"):
        cabi.flowprojection_forward_batch([flow], [torch.zeros((1, 1, 16, 64), device="cuda:0")], [torch.zeros_like(flow)], 1)


@pytest.mark.parametrize("model", ["smooth", "zero", "wild"])
def test_filterinterp_channel_planes_farther_apart_than_a_descriptor_spans(torch_mod, cabi, oracle, model):
    """The 16-byte-staging loop addresses all planes of a tensor through ONE buffer descriptor and a scalar offset per plane; a
    descriptor spans 2^31 - 1 bytes, so on tensors larger than that (4K x 196 channels: 6.9 GB) the base moves up every few
    planes.  Small planes 600 MB apart (a view with a huge channel stride) cross that boundary twice in nine channels without
    a 4K-sized oracle run: bit-exact with the oracle, nothing written between the planes' neighbours."""
    torch = torch_mod
    rng = np.random.default_rng(77)
    C, H, W = 9, 96, 256
    cs = 150_000_000                                      # floats: 600 MB between planes (a multiple of four: rows stay 16-byte aligned)
    img = rng.standard_normal((1, C, H, W)).astype(f32)
    filt = rng.random((1, 16, H, W), dtype=f32)
    flow = {"smooth": smooth_flow(rng, 1, H, W, 3.0), "zero": np.zeros((1, 2, H, W), f32),
            "wild": (rng.standard_normal((1, 2, H, W)) * 40.0).astype(f32)}[model]
    n = (C - 1) * cs + H * W
    src = torch.empty(n + 3 * W, device="cuda:0")
    dst = torch.empty(n + 3 * W, device="cuda:0")
    gin = torch.as_strided(src, (1, C, H, W), (n, cs, W, 1), 2 * W)
    gout = torch.as_strided(dst, (1, C, H, W), (n, cs, W, 1), 2 * W)
    guard = torch.as_strided(dst, (C, 2, W), (cs, H * W + W, 1), W)          # the row just before and the row just after every plane
    gin.copy_(gpu(torch, img))
    gout.fill_(float("nan"))
    guard.fill_(-7.0)
    assert cabi.filterinterp_forward_ori(gin, gpu(torch, flow), gpu(torch, filt), gout) == 0
    ref = oracle.filterinterp_ori_fwd(img, flow, filt, fmad=1)
    assert np.array_equal(cpu(gout.contiguous()), ref)
    g = cpu(guard.contiguous())
    assert np.all(g == -7.0)
    del src, dst
    torch.cuda.empty_cache()


def test_correlation_kernels_agree_on_random_shapes(torch_mod, cabi):
    """PWC-Net's configuration on random shapes: the aligned path (the four-pixel kernel for large levels, the two-pixel one below)
    and the kernels that take over when the inputs sit at an odd element offset of their storage sum the channels in the same
    order -- same bits; the pair entry equals two single calls.  (tools/corr_soak.py runs more of these.)"""
    torch = torch_mod
    g = torch.Generator().manual_seed(5)
    for case in range(14):
        b = int(torch.randint(1, 3, (1,), generator=g))
        c = int(torch.randint(1, 70, (1,), generator=g))
        h = int(torch.randint(9, 300, (1,), generator=g))
        w = 4 * int(torch.randint(4, 260, (1,), generator=g))
        pad = 4 if case % 5 else 0
        n = b * c * h * w
        s1, s2 = torch.randn(n + 1, generator=g).to("cuda:0"), torch.randn(n + 1, generator=g).to("cuda:0")
        u1, u2 = s1[1:].view(b, c, h, w), s2[1:].view(b, c, h, w)                  # 4 bytes off a 16-byte boundary
        a1, a2 = u1.clone(), u2.clone()                                             # the same values, aligned
        ref = cabi.correlation_forward(u1, u2, pad, 1, 4, 1, 1)
        out = cabi.correlation_forward(a1, a2, pad, 1, 4, 1, 1)
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), (b, c, h, w, pad)
        pa, pb = cabi.correlation_forward_pair(a1, a2, a2, a1, pad, 1, 4, 1, 1)
        assert torch.equal(pa, out) and torch.equal(pb, cabi.correlation_forward(a2, a1, pad, 1, 4, 1, 1)), (b, c, h, w, pad)
