"""Shared by the reference-pinning tests: the edge inputs, how a case is run on the CPU execution of the reference
(`oracle/refexec/ref_exec.py`) and on the oracle, and the rules by which the two are compared.

A case is (op, params, inputs).  `run_ref` returns the executor's outputs as a flat dict of arrays -- what
`tests/golden/reference.npz` records, in raster order; `run_oracle` returns the oracle's (`fmad=0`) under the same
keys; `check` asserts the rules:

  per-pixel results      bit for bit, in both thread orders (the executor's two orders must first agree)
  scatters / atomic sums raster order: bit for bit (the oracle sums in raster order);
                         block order: counts exact, projected flow <= 1e-4 abs, image gradients
                         <= 2e-6 * max(1, |ref|), every other sum <= 1e-5 * max(1, |ref|); dyadic inputs bit for bit
  MinDepthFlowProjection tie-free weights: bit for bit in both orders; tied weights: bit for bit in raster order
                         and the executor's two orders differ on the same input
  deformable variants    compared where the executor's mask is clear; the mask covers <= 25 % and leaves pixels
                         in all four border bands of width fs
  correlation            bit for bit against order=0, fmad=0, where the executor's mask is clear
"""
import numpy as np

f32 = np.float32

PROJ_TOL = 1e-4       # projected flow, absolute
GRAD_TOL = 2e-6       # image gradients, * max(1, |ref|)
SUM_TOL = 1e-5        # any other reordered sum, * max(1, |ref|)
MASK_CAP = 0.25


class Case:
    def __init__(self, op, inputs, **params):
        self.op, self.inputs, self.params = op, inputs, params


# ---------------------------------------------------------------- inputs

def edge_flow(rng, B, H, W, sigma=2.0):
    """Random flow with the truncation / border / range edges planted in the top-left pixels of item 0."""
    flow = (rng.standard_normal((B, 2, H, W)) * sigma).astype(f32)
    plant = [
        (1.0, 0.0), (-2.0, 1.0),                        # exactly integer
        (-0.5, -0.5), (-1e-7, -1e-7),                   # (int) truncates towards zero, floor does not
        ("x0", "y0"), ("xw", "yh"),                     # lands exactly on 0 / on w-1, h-1
        ("xw+", "yh+"), ("x0-", "y0-"),                 # just past them
        ("half", 0.0), (0.0, "half"), ("-half", "-half"),   # |f| >= w/2, h/2
    ]
    k = 0
    for fx, fy in plant:
        y, x = divmod(k, W)
        if y >= H:
            break
        k += 1

        def val(v, pos, n):
            if not isinstance(v, str):
                return f32(v)
            if v in ("x0", "y0"):
                return f32(-pos)
            if v in ("xw", "yh"):
                return f32(n - 1 - pos)
            if v in ("xw+", "yh+"):
                return np.nextafter(f32(n - 1 - pos), f32(np.inf)) + f32(1e-3)
            if v in ("x0-", "y0-"):
                return f32(-pos) - f32(1e-3)
            return f32(n) / f32(2) * (f32(-1) if v[0] == "-" else f32(1))
        flow[0, 0, y, x], flow[0, 1, y, x] = val(fx, x, W), val(fy, y, H)
    return flow


def _fi_case(rng, B, C, H, W, fs, sigma=2.0):
    return Case("fi_ori", dict(img=rng.standard_normal((B, C, H, W)).astype(f32), flow=edge_flow(rng, B, H, W, sigma),
                               filt=rng.standard_normal((B, fs * fs, H, W)).astype(f32),
                               gout=rng.standard_normal((B, C, H, W)).astype(f32)))


def _defor_inputs(rng, B, C, H, W, fs, sigma=2.0):
    return dict(img=rng.standard_normal((B, C, H, W)).astype(f32), flow=edge_flow(rng, B, H, W, sigma),
                filt=rng.standard_normal((B, fs * fs, H, W)).astype(f32),
                off=rng.uniform(-1, 1, (B, 2 * fs * fs, H, W)).astype(f32),
                gout=rng.standard_normal((B, C, H, W)).astype(f32))


def _proj_inputs(rng, B, H, W, kind):
    if kind == "dyadic":
        flow = (np.round(rng.standard_normal((B, 2, H, W)) * 2.0 * 4) / 4).astype(f32)
        depth = f32(2.0) ** rng.integers(-2, 2, (B, 1, H, W)).astype(f32)
        gout = (np.round(rng.standard_normal((B, 2, H, W)) * 8) / 8).astype(f32)
        return flow, depth, gout
    if kind == "nothing":                               # nothing lands: the hole filler finds no neighbour
        flow = np.full((B, 2, H, W), f32(W + H), f32)
    elif kind == "gaps":
        # near identity (every source lands within its own pixel), but source rows 1, 2 and source columns 2, 3
        # land nowhere.  The summed projections splat every
        # source onto (x, x+1) x (y, y+1) (flowprojection_cuda_kernel.cu:70-88), so target row 2 and target column 3
        # stay empty -- a hole whose left / right (up / down) search runs off the frame while the other pair
        # succeeds; MinDepthFlowProjection writes the top-left target only: rows 1, 2 and columns 2, 3 stay empty
        flow = np.empty((B, 2, H, W), f32)              # a small dyadic flow: the filled holes are not zero
        flow[:, 0] = 0.25 + 0.125 * (np.arange(W) % 2)
        flow[:, 1] = (0.5 - 0.125 * (np.arange(H) % 3))[:, None]
        flow[:, 1, 1:3, :] = 1000.0
        flow[:, 0, :, 2:4] = 1000.0
    else:
        flow = edge_flow(rng, B, H, W)
    depth = rng.uniform(0.1, 1.0, (B, 1, H, W)).astype(f32)
    gout = rng.standard_normal((B, 2, H, W)).astype(f32)
    return flow, depth, gout


def _weights(rng, B, H, W, tied):
    if tied:
        return (rng.integers(1, 9, (B, 1, H, W)) / 8.0).astype(f32)
    w = rng.permutation(B * H * W).astype(f32) / f32(B * H * W) + f32(0.25)      # all distinct
    return w.reshape(B, 1, H, W)


def _sep_inputs(rng, B, C, H, W, fs):
    oh, ow = H - fs + 1, W - fs + 1
    v = rng.standard_normal((B, fs, oh, ow)).astype(f32)
    h = rng.standard_normal((B, fs, oh, ow)).astype(f32)
    v[0, :, 0, 0] = 0.0                                 # weight sums of exactly zero (SeparableConvFlow's -2000)
    h[0, :, 0, 1] = 0.0
    v[0, :, 1, 0] = np.resize(np.array([1.0, -1.0], f32), fs) * (np.arange(fs) < fs - fs % 2)
    return dict(img=rng.standard_normal((B, C, H, W)).astype(f32), v=v, h=h,
                gout=rng.standard_normal((B, C, oh, ow)).astype(f32),
                gflow=rng.standard_normal((B, 2, oh, ow)).astype(f32))


def _corr_case(rng, cfg, B, C, H, W):
    f1 = rng.standard_normal((B, C, H, W)).astype(f32)
    f2 = rng.standard_normal((B, C, H, W)).astype(f32)
    pad, k, md, s1, s2 = cfg
    border = (k - 1) // 2 + md
    oc = (md // s2 * 2 + 1) ** 2
    oh = int(np.ceil(f32(H + 2 * pad - 2 * border) / f32(s1)))
    ow = int(np.ceil(f32(W + 2 * pad - 2 * border) / f32(s1)))
    return Case("corr", dict(f1=f1, f2=f2, gout=rng.standard_normal((B, oc, oh, ow)).astype(f32)), cfg=cfg)


def cases(extra=False):
    """The recorded set (small: it has to fit tests/golden/reference.npz).  extra=True adds the larger live-only
    cases: two blocks in both directions with B = 2, and the frames of the deformable measurements."""
    rng = np.random.default_rng(20241018)
    c = {}
    # FilterInterpolation `_ori`: every filter size on a frame wider than one 32-thread block row, and the
    # degenerate frames
    c["fi_ori_fs4"] = _fi_case(rng, 1, 2, 18, 36, 4)
    for fs in (2, 5, 6):
        c["fi_ori_fs%d" % fs] = _fi_case(rng, 1, 2, 5, 34, fs)
    c["fi_ori_w1"] = _fi_case(rng, 1, 2, 5, 1, 4, 0.7)
    c["fi_ori_h1"] = _fi_case(rng, 1, 2, 1, 7, 4, 0.7)
    c["fi_ori_1x1"] = _fi_case(rng, 1, 1, 1, 1, 4, 0.3)
    # deformable variants share one input set per filter size
    d4 = _defor_inputs(rng, 1, 2, 12, 34, 4)
    for v in (0, 1, 2):
        c["fi_defor%d_fs4" % v] = Case("fi_defor", d4, variant=v)
    # projections
    for kind, (B, H, W) in (("edge", (1, 18, 36)), ("dyadic", (1, 18, 36)), ("nothing", (1, 4, 5)),
                            ("gaps", (1, 6, 7)), ("w1", (1, 5, 1)), ("h1", (1, 1, 6)), ("1x1", (1, 1, 1))):
        flow, depth, gout = _proj_inputs(rng, B, H, W, kind)
        c["flowproj_" + kind] = Case("flowproj", dict(flow=flow, gout=gout), dyadic=kind == "dyadic", gaps=kind == "gaps")
        c["depthproj_" + kind] = Case("depthproj", dict(flow=flow, depth=depth, gout=gout), dyadic=kind == "dyadic",
                                      gaps=kind == "gaps")
        if kind in ("edge", "gaps", "1x1"):
            c["mindepth_" + kind] = Case("mindepth", dict(flow=flow, weight=_weights(rng, B, H, W, False), gout=gout),
                                         tied=False, gaps=kind == "gaps")
    flow, _, gout = _proj_inputs(rng, 1, 18, 36, "edge")
    c["mindepth_tied"] = Case("mindepth", dict(flow=flow, weight=_weights(rng, 1, 18, 36, True), gout=gout), tied=True)
    # Interpolation / InterpolationCh
    for name, (C, H, W, s) in (("", (2, 18, 36, 2.0)), ("_w1", (1, 4, 1, 0.7)), ("_h1", (1, 1, 5, 0.7)), ("_1x1", (1, 1, 1, 0.3))):
        i = dict(img=rng.standard_normal((1, C, H, W)).astype(f32), flow=edge_flow(rng, 1, H, W, s),
                 gout=rng.standard_normal((1, C, H, W)).astype(f32))
        c["interp" + name] = Case("interp", i)
        c["interpch" + name] = Case("interpch", i)
    # SeparableConv / SeparableConvFlow (three channels: the reference's wrappers accept nothing else)
    s5 = _sep_inputs(rng, 1, 3, 10, 38, 5)
    c["sepconv_fs5"] = Case("sepconv", s5)
    c["sepconvflow_fs5"] = Case("sepconvflow", s5)
    s2 = _sep_inputs(rng, 1, 3, 3, 4, 2)
    c["sepconv_fs2"] = Case("sepconv", s2)
    c["sepconvflow_fs2"] = Case("sepconvflow", s2)
    # correlation: PWC's configuration with 0, 1 or 2 channels per lane, the two others, a 3x2 frame
    pwc = (4, 1, 4, 1, 1)
    c["corr_pwc_c5"] = _corr_case(rng, pwc, 2, 5, 5, 6)
    c["corr_pwc_c32"] = _corr_case(rng, pwc, 1, 32, 5, 6)
    c["corr_pwc_c40"] = _corr_case(rng, pwc, 1, 40, 5, 6)
    c["corr_k3s2"] = _corr_case(rng, (3, 3, 4, 1, 2), 2, 5, 7, 8)
    c["corr_flownet"] = _corr_case(rng, (20, 1, 20, 2, 2), 1, 5, 6, 7)
    c["corr_pwc_3x2"] = _corr_case(rng, pwc, 2, 5, 3, 2)
    # MinDepthFlowProjection's tie rule on signed zeros (tests/side_ops.py): two sources whose weights are -0.0 and +0.0, in
    # both raster orders (item 1, item 0), over an incoming count of -1 -- the first source keeps the target
    from tests import side_ops as so
    flow, weight, count0, _ = so.md_zero_tie("item 1")
    c["mindepth_zero_tie"] = Case("planted", dict(flow=flow, weight=weight, count0=count0), what="mindepth_floor")
    if extra:
        rng = np.random.default_rng(7)
        for fs in (2, 4, 5, 6):
            c["x_fi_ori_fs%d" % fs] = _fi_case(rng, 2, 3, 20, 40, fs, 3.0)
        for v, (fs, H, W) in ((0, (4, 32, 48)), (1, (4, 20, 40)), (2, (4, 24, 24)), (0, (5, 24, 40)), (1, (6, 24, 40)),
                              (2, (2, 20, 40)), (1, (5, 20, 40)), (2, (6, 24, 24))):
            c["x_fi_defor%d_fs%d_%dx%d" % (v, fs, H, W)] = Case("fi_defor", _defor_inputs(rng, 2, 3, H, W, fs, 3.0), variant=v)
        for kind in ("edge", "dyadic", "gaps"):
            flow, depth, gout = _proj_inputs(rng, 2, 20, 40, kind)
            c["x_flowproj_" + kind] = Case("flowproj", dict(flow=flow, gout=gout), dyadic=kind == "dyadic",
                                           gaps=kind == "gaps")
            c["x_depthproj_" + kind] = Case("depthproj", dict(flow=flow, depth=depth, gout=gout), dyadic=kind == "dyadic",
                                            gaps=kind == "gaps")
            for tied in (False, True):
                c["x_mindepth_%s_%s" % (kind, "tied" if tied else "free")] = Case(
                    "mindepth", dict(flow=flow, weight=_weights(rng, 2, 20, 40, tied), gout=gout), tied=tied,
                    gaps=kind == "gaps")
        i = dict(img=rng.standard_normal((2, 3, 20, 40)).astype(f32), flow=edge_flow(rng, 2, 20, 40, 3.0),
                 gout=rng.standard_normal((2, 3, 20, 40)).astype(f32))
        c["x_interp"], c["x_interpch"] = Case("interp", i), Case("interpch", i)
        s = _sep_inputs(rng, 2, 3, 20, 40, 5)
        c["x_sepconv"], c["x_sepconvflow"] = Case("sepconv", s), Case("sepconvflow", s)
        # the correlation forward on non-finite, overflowing and subnormal features (tests/corr_edges.py): what the
        # reference's zero-padded buffers make of an infinity next to the frame edge
        from tests import corr_edges
        f1, f2, _ = corr_edges.plant(rng, 2, 5, 6, 13, f32)
        c["x_corr_planted"] = Case("corr_planted", dict(f1=f1, f2=f2), cfg=pwc)
        # pad 8: the output origin lies outside the frame, so the FIRST map's tap meets the padding too (0 * inf)
        c["x_corr_planted_pad8"] = Case("corr_planted", dict(f1=f1, f2=f2), cfg=(8, 1, 4, 1, 1))
        # the forward warps and projections on planted inputs (tests/forward_edges.py): forward only, NaN and infinity are
        # results.  Every planted flow fails the reference's validity test or gives an exactly representable position
        # inside the frame, so no case depends on the conversion of an out-of-range float to int
        from tests import forward_edges as fe
        rng = np.random.default_rng(20261020)
        flow, depth = fe.small_proj_inputs(rng)
        c["x_flowproj_planted"] = Case("planted", dict(flow=flow), what="flowproj")
        c["x_depthproj_planted"] = Case("planted", dict(flow=flow, depth=depth), what="depthproj")
        img, flow, filt = fe.small_fi_inputs(rng)
        c["x_fi_ori_planted"] = Case("planted", dict(img=img, flow=flow, filt=filt), what="fi_ori")
        img, flow = fe.small_interp_inputs(rng)
        c["x_interp_planted"] = Case("planted", dict(img=img, flow=flow), what="interp")
        # the side ops on planted inputs (tests/side_ops.py), small versions: Interpolation's border decisions, SeparableConv
        # and SeparableConvFlow with non-finite, huge, subnormal and signed-zero values, MinDepthFlowProjection's ties of
        # signed zeros over a negative floor.  Every planted flow fails the validity test or is exactly representable
        # inside the frame, as above
        img, flow, _ = so.interp_border()
        c["x_interp_border"] = Case("planted", dict(img=img, flow=flow), what="interp_border")
        d = so.sep_planted(5, so.SMALL_FRAME)
        c["x_sepconv_planted"] = Case("planted", {k: d[k] for k in ("img", "v", "h", "gout")}, what="sepconv")
        d = so.sepflow_planted(so.SMALL_FRAME, step=1)
        c["x_sepconvflow_planted"] = Case("planted", {k: d[k] for k in ("img", "v", "h", "gflow")}, what="sepconvflow")
        for name in so.MD_TIE_NAMES:
            flow, weight, count0, _ = so.md_zero_tie(name)
            if flow.shape[2:] == so.SMALL_FRAME[2:]:
                c["x_mindepth_zero_tie_" + name.replace(",", "").replace(" ", "_")] = Case(
                    "planted", dict(flow=flow, weight=weight, count0=count0), what="mindepth_floor")
    return c


# ---------------------------------------------------------------- running a case

def ones(count):
    """Counts of zero replaced by one, as callers of the projections' backward do before dividing by them (and
    tests/golden/make_golden.py did).  The reference's wrappers replace nothing and its backward kernels read the
    count only at cells something landed on: the `*_ones` gradients must equal the plain ones, which `check` asserts."""
    return np.where(count > 0, count, 1).astype(f32)


def run_ref(R, case, given=None):
    """The executor's outputs in its current thread order, always under canvas=True: the masks of the deformable
    variants and the correlation are outputs; every other op's must be empty, asserted here.  `given`: outputs of
    an earlier run whose forward results (count, out0) the projections' backward is handed instead of this run's,
    so that two thread orders can be compared on the same backward inputs."""
    i, op = case.inputs, case.op
    p = dict(case.params)
    if given is not None:
        p.update({k: given[k] for k in ("count", "out0") if k in given})
    o = {}

    def clean(*masks):
        assert R.last_margin_writes == 0, (op, "wrote outside a frame")
        for m in masks:
            for k in (m if isinstance(m, tuple) else (m,)):
                assert not k.any(), (op, "read outside a frame")

    if op == "fi_ori":
        o["out"], m = R.filterinterp_ori_fwd(i["img"], i["flow"], i["filt"], canvas=True)
        clean(m)
        o["gimg"], o["gflow"], o["gfilt"], m = R.filterinterp_ori_bwd(i["img"], i["flow"], i["filt"], i["gout"], canvas=True)
        clean(m)
    elif op == "fi_defor":
        v = p["variant"]
        o["out"], o["mask"] = R.filterinterp_defor_fwd(v, i["img"], i["flow"], i["filt"], i["off"], canvas=True)
        assert R.last_margin_writes == 0
        px = R.filterinterp_defor_bwd(v, i["img"], i["flow"], i["filt"], i["off"], i["gout"], canvas=True)[-1]
        # a second pass with the gradient zeroed on those pixels: their threads then add zeros to the image gradient,
        # which makes it comparable everywhere
        r = R.filterinterp_defor_bwd(v, i["img"], i["flow"], i["filt"], i["off"], i["gout"] * ~px, canvas=True)
        assert R.last_margin_writes == 0
        assert np.array_equal(r[-1], px)
        o["pxmask"] = px
        o["gimg"], o["gflow"], o["goff"] = r[0], r[1], r[3]
        if v != 2:
            o["gfilt"] = r[2]
    elif op == "flowproj":
        o["out0"], o["count"], m = R.flowproj_fwd(i["flow"], 0, canvas=True)
        clean(m)
        o["out1"], _, m = R.flowproj_fwd(i["flow"], 1, canvas=True)
        clean(m)
        o["gflow"], m = R.flowproj_bwd(i["flow"], p.get("count", o["count"]), i["gout"], canvas=True)
        clean(m)
        o["gflow_ones"], m = R.flowproj_bwd(i["flow"], ones(p.get("count", o["count"])), i["gout"], canvas=True)
        clean(m)
    elif op == "depthproj":
        o["out0"], o["count"], m = R.depthflowproj_fwd(i["flow"], i["depth"], 0, canvas=True)
        clean(m)
        o["out1"], _, m = R.depthflowproj_fwd(i["flow"], i["depth"], 1, canvas=True)
        clean(m)
        o["gflow"], o["gdepth"], m = R.depthflowproj_bwd(i["flow"], i["depth"], p.get("count", o["count"]),
                                                         p.get("out0", o["out0"]), i["gout"], canvas=True)
        clean(m)
        o["gflow_ones"], o["gdepth_ones"], m = R.depthflowproj_bwd(i["flow"], i["depth"], ones(p.get("count", o["count"])),
                                                                   p.get("out0", o["out0"]), i["gout"], canvas=True)
        clean(m)
    elif op == "mindepth":
        o["out0"], o["count"], m = R.mindepthflowproj_fwd(i["flow"], i["weight"], 0, canvas=True)
        clean(m)
        o["out1"], _, m = R.mindepthflowproj_fwd(i["flow"], i["weight"], 1, canvas=True)
        clean(m)
        o["gflow"], m = R.mindepthflowproj_bwd(i["flow"], i["weight"], p.get("count", o["count"]), i["gout"],
                                               p.get("out0", o["out0"]), canvas=True)
        clean(m)
    elif op in ("interp", "interpch"):
        fwd, bwd = (R.interp_fwd, R.interp_bwd) if op == "interp" else (R.interpch_fwd, R.interpch_bwd)
        o["out"], m = fwd(i["img"], i["flow"], canvas=True)
        clean(m)
        o["gimg"], o["gflow"], m = bwd(i["img"], i["flow"], i["gout"], canvas=True)
        clean(m)
    elif op == "sepconv":
        o["out"], m = R.sepconv_fwd(i["img"], i["v"], i["h"], canvas=True)
        clean(m)
        o["gimg"], o["gv"], o["gh"], m = R.sepconv_bwd(i["img"], i["v"], i["h"], i["gout"], canvas=True)
        clean(m)
    elif op == "sepconvflow":
        H, W = i["img"].shape[2:]
        o["out"], m = R.sepconvflow_fwd(i["v"], i["h"], H, W, canvas=True)
        clean(m)
        o["gv"], o["gh"], m = R.sepconvflow_bwd(i["v"], i["h"], i["gflow"], H, W, canvas=True)
        clean(m)
    elif op == "corr":
        cfg = p["cfg"]
        o["out"], o["mask"] = R.correlation_fwd(i["f1"], i["f2"], *cfg, canvas=True)
        if cfg[3] == 1:     # stride1 > 1: the reference's backward writes outside gradInput (not run)
            o["g1"], o["g2"], (o["mask1"], o["mask2"]) = R.correlation_bwd(i["f1"], i["f2"], i["gout"], *cfg, canvas=True)
    elif op == "corr_planted":
        o["out"] = R.correlation_fwd(i["f1"], i["f2"], *p["cfg"])      # (NaN is a result here: no canvas mask)
    elif op == "planted":                                              # (likewise)
        what = p["what"]
        if what == "flowproj":
            (o["out0"], o["count"]), (o["out1"], _) = R.flowproj_fwd(i["flow"], 0), R.flowproj_fwd(i["flow"], 1)
        elif what == "depthproj":
            (o["out0"], o["count"]), (o["out1"], _) = (R.depthflowproj_fwd(i["flow"], i["depth"], fh) for fh in (0, 1))
        elif what == "fi_ori":
            o["out"] = R.filterinterp_ori_fwd(i["img"], i["flow"], i["filt"])
        elif what == "sepconv":
            o["out"] = R.sepconv_fwd(i["img"], i["v"], i["h"])
            o["gimg"], o["gv"], o["gh"] = R.sepconv_bwd(i["img"], i["v"], i["h"], i["gout"])
        elif what == "sepconvflow":
            H, W = i["img"].shape[2:]
            o["out"] = R.sepconvflow_fwd(i["v"], i["h"], H, W)
            o["gv"], o["gh"] = R.sepconvflow_bwd(i["v"], i["h"], i["gflow"], H, W)
        elif what == "mindepth_floor":
            (o["out0"], o["count"]), (o["out1"], _) = (R.mindepthflowproj_fwd(i["flow"], i["weight"], fh, count0=i["count0"])
                                                       for fh in (0, 1))
        else:                                                          # "interp", "interp_border"
            o["out"] = R.interp_fwd(i["img"], i["flow"])
    else:
        raise KeyError(op)
    return o


def run_oracle(O, case, ref):
    """The oracle at fmad=0 under run_ref's keys.  `ref` supplies what the executor alone defines: the deformable
    pixel mask (for the second backward pass) and the forward results the projections' backward is given."""
    i, p, op = case.inputs, case.params, case.op
    o = {}
    if op == "fi_ori":
        o["out"] = O.filterinterp_ori_fwd(i["img"], i["flow"], i["filt"], fmad=0)
        o["gimg"], o["gflow"], o["gfilt"] = O.filterinterp_ori_bwd(i["img"], i["flow"], i["filt"], i["gout"], fmad=0)
    elif op == "fi_defor":
        v = p["variant"]
        o["out"] = O.filterinterp_defor_fwd(v, i["img"], i["flow"], i["filt"], i["off"], fmad=0)
        r = O.filterinterp_defor_bwd(v, i["img"], i["flow"], i["filt"], i["off"], i["gout"] * ~ref["pxmask"], fmad=0)
        o["gimg"], o["gflow"], o["goff"] = r[0], r[1], r[3]
        if v != 2:
            o["gfilt"] = r[2]
    elif op == "flowproj":
        o["out0"], o["count"] = O.flowproj_fwd(i["flow"], 0)
        o["out1"], _ = O.flowproj_fwd(i["flow"], 1)
        o["gflow"] = O.flowproj_bwd(i["flow"], ref["count"], i["gout"])
        o["gflow_ones"] = O.flowproj_bwd(i["flow"], ones(ref["count"]), i["gout"])
    elif op == "depthproj":
        o["out0"], o["count"] = O.depthflowproj_fwd(i["flow"], i["depth"], 0)
        o["out1"], _ = O.depthflowproj_fwd(i["flow"], i["depth"], 1)
        o["gflow"], o["gdepth"] = O.depthflowproj_bwd(i["flow"], i["depth"], ref["count"], ref["out0"], i["gout"])
        o["gflow_ones"], o["gdepth_ones"] = O.depthflowproj_bwd(i["flow"], i["depth"], ones(ref["count"]), ref["out0"],
                                                                i["gout"])
    elif op == "mindepth":
        o["out0"], o["count"] = O.mindepthflowproj_fwd(i["flow"], i["weight"], 0)
        o["out1"], _ = O.mindepthflowproj_fwd(i["flow"], i["weight"], 1)
        o["gflow"] = O.mindepthflowproj_bwd(i["flow"], i["weight"], ref["count"], i["gout"])
    elif op in ("interp", "interpch"):
        o["out"] = O.interp_fwd(i["img"], i["flow"], fmad=0)
        o["gimg"], o["gflow"] = O.interp_bwd(i["img"], i["flow"], i["gout"], fmad=0)
    elif op == "sepconv":
        o["out"] = O.sepconv_fwd(i["img"], i["v"], i["h"], fmad=0)
        o["gimg"], o["gv"], o["gh"] = O.sepconv_bwd(i["img"], i["v"], i["h"], i["gout"])
    elif op == "sepconvflow":
        H, W = i["img"].shape[2:]
        o["out"] = O.sepconvflow_fwd(i["v"], i["h"], H, W, fmad=0)
        o["gv"], o["gh"] = O.sepconvflow_bwd(i["v"], i["h"], i["gflow"], H, W, fmad=0)
    elif op == "corr":
        cfg = p["cfg"]
        o["out"] = O.correlation_fwd(i["f1"], i["f2"], *cfg, order=0, fmad=0)
        if cfg[3] == 1:
            o["g1"], o["g2"] = O.correlation_bwd(i["f1"], i["f2"], i["gout"], *cfg, fmad=0)
    elif op == "corr_planted":
        o["out"] = O.correlation_fwd(i["f1"], i["f2"], *p["cfg"], order=0, fmad=0)
    elif op == "planted":
        what = p["what"]
        if what == "flowproj":
            (o["out0"], o["count"]), (o["out1"], _) = O.flowproj_fwd(i["flow"], 0), O.flowproj_fwd(i["flow"], 1)
        elif what == "depthproj":
            (o["out0"], o["count"]), (o["out1"], _) = (O.depthflowproj_fwd(i["flow"], i["depth"], fh) for fh in (0, 1))
        elif what == "fi_ori":
            o["out"] = O.filterinterp_ori_fwd(i["img"], i["flow"], i["filt"], fmad=0)
        elif what == "sepconv":
            o["out"] = O.sepconv_fwd(i["img"], i["v"], i["h"], fmad=0)
            o["gimg"], o["gv"], o["gh"] = O.sepconv_bwd(i["img"], i["v"], i["h"], i["gout"])
        elif what == "sepconvflow":
            H, W = i["img"].shape[2:]
            o["out"] = O.sepconvflow_fwd(i["v"], i["h"], H, W, fmad=0)
            o["gv"], o["gh"] = O.sepconvflow_bwd(i["v"], i["h"], i["gflow"], H, W, fmad=0)
        elif what == "mindepth_floor":
            (o["out0"], o["count"]), (o["out1"], _) = (O.mindepthflowproj_fwd(i["flow"], i["weight"], fh, count0=i["count0"])
                                                       for fh in (0, 1))
        else:
            o["out"] = O.interp_fwd(i["img"], i["flow"], fmad=0)
    else:
        raise KeyError(op)
    return o


# ---------------------------------------------------------------- the rules

# which outputs are sums over threads (atomicAdd scatters); everything else is computed by one thread alone
SCATTER = {"fi_ori": {"gimg": GRAD_TOL}, "fi_defor": {"gimg": GRAD_TOL}, "interp": {"gimg": GRAD_TOL},
           "interpch": {"gimg": GRAD_TOL}, "sepconv": {"gimg": GRAD_TOL},
           "flowproj": {"out0": PROJ_TOL, "out1": PROJ_TOL, "count": 0.0},
           "depthproj": {"out0": PROJ_TOL, "out1": PROJ_TOL, "count": SUM_TOL},
           "mindepth": {"out0": None, "out1": None, "count": None}}
MASK_KEYS = ("mask", "pxmask", "mask1", "mask2")


def mask_for(case, ref, key):
    """The elements of `key` the executor calls undefined (None: all defined)."""
    if case.op == "fi_defor":
        if key == "out":
            return ref["mask"]
        if key in ("gflow", "gfilt", "goff"):
            return np.broadcast_to(ref["pxmask"], ref[key].shape)
    if case.op == "corr":
        return {"out": ref["mask"], "g1": ref.get("mask1"), "g2": ref.get("mask2")}[key]
    return None


def same(a, b, mask=None):
    if mask is not None:
        a, b = np.where(mask, f32(0), a), np.where(mask, f32(0), b)
    return np.array_equal(a, b)


def within(a, ref, tol, absolute=False):
    bound = tol if absolute else tol * np.maximum(1.0, np.abs(ref))
    return bool(np.all(np.abs(a.astype(np.float64) - ref) <= bound))


def check_masks(case, ref):
    """Every mask of out-of-buffer reads: at most 25 % of the elements.  The deformable ones leave clear pixels in all
    four border bands of width fs; the correlation's are empty at kernel_size 1 (its kernels stay inside the padded
    scratch) and, at kernel_size 3, confined to where its window start is short by the kernel radius."""
    if case.op == "corr":
        k = case.params["cfg"][1]
        for key in ("mask", "mask1", "mask2"):
            if key in ref:
                assert ref[key].mean() <= MASK_CAP, (key, ref[key].mean())
                assert k > 1 or not ref[key].any(), (key, "kernel_size 1 must not read outside its scratch")
        if k > 1:       # forward: only batch item 0 reads in front of the scratch: its top output row (window row -1)
            assert not ref["mask"][1:].any() and not ref["mask"][0, :, 2:].any()     # and (row 0, column -1) below it
        return
    if case.op != "fi_defor":
        return
    fs = int(np.sqrt(f32(case.inputs["off"].shape[1] // 2)))
    for m in (ref["mask"], ref["pxmask"]):
        assert m.mean() <= MASK_CAP, m.mean()
        clear = ~m.any(axis=1)
        assert clear[:, :fs].any() and clear[:, -fs:].any() and clear[:, :, :fs].any() and clear[:, :, -fs:].any()


def check_gaps(name, case, ref):
    """The 'gaps' frames: the count has a whole empty row and a whole empty column next to non-empty ones, so the
    hole filler meets holes whose search runs off the frame in one direction; and it did fill something."""
    if not case.params.get("gaps"):
        return
    zero = ref["count"][:, 0] == 0
    rows, cols = zero.all(axis=2), zero.all(axis=1)                  # [B, H], [B, W]
    for b in range(zero.shape[0]):
        r, c = np.flatnonzero(rows[b]), np.flatnonzero(cols[b])
        assert r.size and c.size, (name, "no empty row / column")
        assert any(0 < y < rows.shape[1] - 1 and not rows[b, y - 1] or not rows[b, min(y + 1, rows.shape[1] - 1)]
                   for y in r), name
        assert any(0 < x < cols.shape[1] - 1 and not cols[b, x - 1] or not cols[b, min(x + 1, cols.shape[1] - 1)]
                   for x in c), name
    assert not np.array_equal(ref["out0"], ref["out1"]), (name, "fillhole changed nothing")


def check(name, case, ref_raster, got, ref_blocks=None):
    """`got` (the oracle) against the executor's raster-order outputs and, when given, its block-order outputs."""
    if case.op == "corr_planted":
        # NaN and infinity are the expected results: NaN masks equal, everything else bit for bit, in both thread orders;
        # and the reference does turn a non-finite value that meets its padding into NaN
        from tests import corr_edges
        want = ref_raster["out"]
        cfg = case.params["cfg"]
        sites1, sites2 = corr_edges.padding_sites(case.inputs["f1"], case.inputs["f2"], cfg)
        assert sites1.any() and np.isnan(want[sites1]).all(), (name, "inf * 0 of the padding")
        # (a first-map tap in the padding needs an output origin outside the frame: pad > max_displacement)
        assert sites2.any() == (cfg[0] > cfg[2]) and np.isnan(want[sites2]).all(), (name, "0 * inf of the padding")
        assert np.isinf(want).any() and np.isfinite(want).mean() >= 0.75, name
        if ref_blocks is not None:
            assert corr_edges.same_bits_nan_aware(ref_blocks["out"], want), (name, "the executor's two orders differ")
        assert corr_edges.same_bits_nan_aware(got["out"], want), (name, "oracle != reference",
                                                                  corr_edges.describe_difference(got["out"], want))
        return
    if case.op == "planted":
        # as above: NaN masks equal and everything else bit for bit, in both thread orders (the planted values sit apart and
        # the rest is dyadic, so the projections' sums do not depend on the order); and the plants did reach the outputs
        from tests import corr_edges
        what = case.params["what"]
        for key, want in ref_raster.items():
            if ref_blocks is not None:
                assert corr_edges.same_bits_nan_aware(ref_blocks[key], want), (name, key, "the executor's two orders differ")
            assert corr_edges.same_bits_nan_aware(got[key], want), (name, key, "oracle != reference",
                                                                    corr_edges.describe_difference(got[key], want))
            assert np.isfinite(want).mean() >= 0.5, (name, key)
        if what in ("interp_border", "sepconv", "sepconvflow", "mindepth_floor"):
            check_side_op(name, case, ref_raster)
        elif what == "flowproj":
            assert all(np.isfinite(v).all() for v in ref_raster.values()), (name, "no planted flow is a valid source")
        elif what == "depthproj":
            cnt = ref_raster["count"]
            assert np.isnan(cnt).any() and (cnt == np.inf).any() and (cnt == -np.inf).any(), name
            assert ((cnt > 0) & (cnt < 2.0 ** -140)).any(), (name, "subnormal counts")
            hole = cnt <= 0
            assert (hole & np.isfinite(ref_raster["out0"][:, :1]) & np.isnan(ref_raster["out1"][:, :1])).any(), (
                name, "a hole filled with NaN from a poisoned neighbour")
        else:
            assert np.isnan(ref_raster["out"]).any() and np.isinf(ref_raster["out"]).any(), name
        return
    scatter = SCATTER.get(case.op, {})
    check_masks(case, ref_raster)
    check_gaps(name, case, ref_raster)
    for key in ("gflow", "gdepth"):
        if key + "_ones" in ref_raster:
            assert same(ref_raster[key + "_ones"], ref_raster[key]), (name, key, "the backward read an empty count")
    for key, want in ref_raster.items():
        if key in MASK_KEYS:
            if ref_blocks is not None:
                assert np.array_equal(want, ref_blocks[key]), (name, key, "mask depends on the thread order")
            continue
        mask = mask_for(case, ref_raster, key)
        if mask is not None:
            assert not np.isnan(want[~mask]).any(), (name, key)
        else:
            assert not np.isnan(want).any(), (name, key)
        tied = case.op == "mindepth" and case.params["tied"]
        if key not in scatter:
            # one thread per element: order-free, proven from the executor alone before the oracle is looked at
            if ref_blocks is not None:
                assert same(want, ref_blocks[key], mask), (name, key, "the executor's two orders differ")
            assert same(got[key], want, mask), (name, key, "oracle != reference")
            continue
        assert same(got[key], want, mask), (name, key, "oracle != reference in raster order")
        if ref_blocks is None:
            continue
        blk, tol = ref_blocks[key], scatter[key]
        if case.op == "mindepth":
            if not tied:
                assert same(blk, want), (name, key, "tie-free weights must not depend on the order")
            continue                                     # tied: see check_tied_orders_differ
        if case.params.get("dyadic") or tol == 0.0:
            assert same(blk, want, mask), (name, key, "exact sums must not depend on the order")
        else:
            assert within(blk, want, tol, absolute=tol == PROJ_TOL), (name, key, np.abs(blk - want).max())
            assert within(got[key], blk, tol, absolute=tol == PROJ_TOL), (name, key)


def check_side_op(name, case, ref):
    """The planted side-op cases (tests/side_ops.py): the plants did decide, in the reference's own results."""
    from tests import side_ops as so
    what, i = case.params["what"], case.inputs
    if what == "interp_border":
        img, flow, expect = so.interp_border()
        assert so.same_bits_nan_aware(ref["out"], so.interp_border_expected(img, expect)), name
    elif what == "sepconv":
        for key in ("out", "gimg", "gv", "gh"):
            _, nan, pinf, ninf = so.nonfinite_census(ref[key])
            assert nan and (pinf or ninf), (name, key)
    elif what == "sepconvflow":
        for x, want in so.sepflow_expected(step=1):
            for got in (ref["out"][:, 1, so.SEPFLOW_ROW_V, x], ref["out"][:, 0, so.SEPFLOW_ROW_H, x]):
                assert np.isnan(got).all() if np.isnan(want) else (got == f32(want)).all(), (name, x, want, got)
    else:
        bits = lambda a: np.ascontiguousarray(a).view(np.uint32)      # noqa: E731
        for b in range(i["flow"].shape[0]):              # per item: every valid source lands on one target; the first wins
            srcs = np.argwhere(i["flow"][b, 0] != so.INVALID)
            if not len(srcs):
                continue
            sy, sx = (int(v) for v in srcs[0])
            ty, tx = int(sy + i["flow"][b, 1, sy, sx]), int(sx + i["flow"][b, 0, sy, sx])
            assert len(srcs) >= 2 and {int(v) for v in bits(i["weight"])[b, 0][tuple(srcs.T)]} == {0, 0x80000000}, name
            for key in ("out0", "out1"):
                assert np.array_equal(ref[key][b, :, ty, tx], -i["flow"][b, :, sy, sx]), (name, key, "the first source's flow")
            assert bits(ref["count"])[b, 0, ty, tx] == bits(i["weight"])[b, 0, sy, sx], (name, "the first source's weight bits")


def flatten(name, case, ref, seen):
    """npz entries of one case: inputs as `<name>/in/<key>`, the executor's outputs as `<name>/ref/<key>`.  An input
    array that an earlier case already stored (cases share input sets) becomes a reference to that entry; `seen`
    is the caller's {id(array): entry} across cases."""
    d = {}
    for k, v in case.inputs.items():
        key = "%s/in/%s" % (name, k)
        d[key] = np.array("@" + seen[id(v)]) if id(v) in seen else v
        seen.setdefault(id(v), key)
    d.update({"%s/ref/%s" % (name, k): v for k, v in ref.items()})
    return d


def load(npz):
    """{name: (Case, recorded outputs)} from tests/golden/reference.npz; ops and params come from cases()."""
    def entry(key):
        v = npz[key]
        return npz[str(v)[1:]] if v.dtype.kind == "U" else v

    out = {}
    for name, c in cases().items():
        ins = {k: entry("%s/in/%s" % (name, k)) for k in c.inputs}
        ref = {key.split("/")[2]: npz[key] for key in npz.files if key.startswith(name + "/ref/")}
        out[name] = (Case(c.op, ins, **c.params), ref)
    return out
