"""CPU checks of tests/forward_edges.py: the planted inputs, sent through the oracle alone, do produce what the GPU tests
(tests/test_gpu_forward_edges.py) are there to compare -- NaN and infinite cells in every planted regime, a hole that the
oracle fills with NaN from a poisoned neighbour, and a frame that stays mostly finite -- and the mirror sends every
planted DepthFlowProjection call to the fallback while FlowProjection keeps its path."""
import numpy as np
import pytest

from tests import forward_edges as fe
from tests import proj_tiles as pt

f32 = np.float32
SEED = 20261020


@pytest.fixture(scope="module")
def planted_proj():
    cache = {}

    def get(kind):
        if kind not in cache:
            rng = np.random.default_rng([SEED, kind == "depth"])
            field = pt.build_field(kind, rng, 1, dyadic=True)
            cache[kind] = (field,) + fe.plant_proj(kind, field, rng)
        return cache[kind]
    return get


def test_comparisons():
    a = np.array([1.0, np.nan, np.inf, -np.inf, -0.0], f32)
    assert fe.same_bits_nan_aware(a, a.copy()) and fe.same_nonfinite_mask(a, a.copy())
    b = a.copy()
    b[1] = fe.NEG_NAN                                        # another NaN: the same
    assert fe.same_bits_nan_aware(a, b)
    b[2] = np.nan                                            # NaN for Inf: only the looser comparison accepts it
    assert not fe.same_bits_nan_aware(a, b) and fe.same_nonfinite_mask(a, b)
    b = a.copy()
    b[4] = 0.0
    assert not fe.same_bits_nan_aware(a, b) and fe.same_nonfinite_mask(a, b)
    b[0] = np.inf
    assert not fe.same_nonfinite_mask(a, b)


def test_planted_depth_projection_caps(oracle, planted_proj):
    (flow0, depth0), flow, depth, planted = planted_proj("depth")
    B, _, h, w = flow.shape
    out0, count = oracle.depthflowproj_fwd(flow, depth, 0)
    out1, count1 = oracle.depthflowproj_fwd(flow, depth, 1)
    assert fe.same_bits_nan_aware(count, count1)
    regions = fe.proj_regions(planted, flow, h, w)
    # every planted regime: a NaN count cell and an infinite one, and the flow of both is NaN (inf / inf, or NaN sums)
    for regime in fe.DEPTH_REGIMES:
        cells = {v: regions["%s:%s" % (regime, v)] for v in ("+inf", "-inf", "nan")}
        assert np.isnan(count[0, 0][cells["nan"]]).all() and cells["nan"].any(), regime
        assert (count[0, 0][cells["+inf"]] == np.inf).all() and (count[0, 0][cells["-inf"]] == -np.inf).all(), regime
        assert np.isnan(out0[0, 0][cells["+inf"]]).all() and np.isnan(out0[0, 0][cells["nan"]]).all(), regime
        # a cell of count -inf is a hole: it keeps its sums, +-inf or NaN
        assert not np.isfinite(out0[0, 0][cells["-inf"]]).any(), regime
    # the huge weights stay finite in the count (2^100, 2^120) or overflow to +inf (FLT_MAX twice on the last row: not here)
    assert (count[0, 0][regions["huge:2^100"]] == f32(2.0 ** 100)).all()
    assert np.isfinite(count[0, 0][regions["huge:FLT_MAX"]]).all() and np.isinf(out0[0][:, regions["huge:FLT_MAX"]]).any()
    # the tiny region: its counts are tiny, non-zero and exact -- the cells are no holes
    (r0, r1), (c0, c1) = fe.TINY_ROWS, fe.TINY_COLS
    inner = count[0, 0, r0 + 2:r0 + 4, c0 + 4:c1 - 4]
    assert (inner > 0).all() and (inner < 2.0 ** -140).all()
    tiny = count[0, 0, r0:r1, c0 + 4:c1 - 4]
    assert ((tiny > 0) & (tiny < 2.0 ** -79)).mean() > 0.5
    # over the frame: mostly finite, and at least one hole that the oracle fills with NaN from a poisoned neighbour
    for a in (count, out0, out1):
        assert np.isfinite(a).mean() >= 0.5
    assert np.isfinite(count).mean() >= 0.99
    hole = count[0, 0] <= 0
    poisoned_fill = hole & np.isfinite(out0[0, 0]) & np.isnan(out1[0, 0])
    assert poisoned_fill.any()
    y, x = fe.HOLE_SOURCE
    assert poisoned_fill[y:y + 3, :x].any(), "the holes left of the NaN cell at HOLE_SOURCE"
    # ... and holes that a finite neighbour fills stay finite
    assert (hole & np.isfinite(out1[0, 0]) & (out1[0, 0] != out0[0, 0])).any()
    # the mirror: the call takes the fallback for its weights; the unplanted field does not
    assert pt.records(flow, depth, h, w)[1] and not pt.records(flow0, depth0, h, w)[1]
    # each reason on its own sends the call away
    for what in ("plain:+inf", "plain:nan", "huge:2^100"):
        d = depth0.copy()
        _, b, yy, xx = next(p for p in planted if p[0] == what)
        d[b, 0, yy, xx] = depth[b, 0, yy, xx]
        assert pt.records(flow0, d, h, w)[1], what
    d = depth0.copy()
    d[0, 0, r0:r1, c0:c1] = depth[0, 0, r0:r1, c0:c1]
    assert pt.records(flow0, d, h, w)[1], "tiny"


def test_planted_flows_fail_the_validity_test_except_minus_zero(oracle, planted_proj):
    for kind in ("flow", "depth"):
        (flow0, depth0), flow, depth, planted = planted_proj(kind)
        B, _, h, w = flow.shape
        valid, _, _ = pt.targets(flow[0, 0], flow[0, 1], h, w)
        valid0, _, _ = pt.targets(flow0[0, 0], flow0[0, 1], h, w)
        seen = set()
        for what, b, y, x in planted:
            if what.startswith("flow:"):
                name = what.split(":")[1]
                seen.add(name)
                assert valid0[y, x], (what, "planted on a source that was invalid already")
                assert valid[y, x] == (name == "-0.0"), what
        assert seen == {n for n, _ in fe.FLOW_SET}
        if kind == "flow":
            # FlowProjection has no weights: no planted flow sends it to the fallback, and the result stays finite
            assert not pt.records(flow, None, h, w)[1]
            out, count = oracle.flowproj_fwd(flow, 1)
            assert np.isfinite(out).all() and np.isfinite(count).all()
            ref, rcount = oracle.flowproj_fwd(flow0, 1)
            assert not np.array_equal(count, rcount)


@pytest.mark.parametrize("kind", ["flow", "depth"])
def test_up4_inputs(oracle, kind):
    fq, depth = fe.up4_inputs(kind, np.random.default_rng([SEED, 4]))
    m0, m1 = fe.UP4_MULS
    full = oracle.flow_upsample4(fq, m0, m1, fmad=1)
    bad = ~np.isfinite(full).all(axis=1)
    assert 0.001 < bad.mean() < 0.1
    fin = full[np.isfinite(full)]
    assert np.array_equal(fin * 32, np.round(fin * 32)), "multiples of 1/32: exact sums"
    out, count = oracle.flowproj_up4_fwd(fq, m0, m1, 1, depth=depth, fmad=1)
    assert np.isfinite(out).mean() >= 0.5
    if kind == "depth":
        assert np.isnan(count).any() and np.isinf(count).any() and np.isnan(out).any()
        assert pt.records(np.nan_to_num(full, nan=1e9, posinf=1e9, neginf=-1e9), depth, *full.shape[2:])[1]
    else:
        assert np.isfinite(out).all() and np.isfinite(count).all()


@pytest.mark.parametrize("shape", fe.WARP_SHAPES)
@pytest.mark.parametrize("align_corners", [True, False])
def test_warp_inputs(oracle, shape, align_corners):
    from tests import corr_edges
    x, flo, planted = fe.warp_inputs(shape, align_corners)
    assert {p[0] for p in planted} == {n for n, _ in fe.FEATURE_SET} and np.isfinite(flo).all()
    zero_w, masked = corr_edges.warp_zero_weight_sites(x, flo, align_corners)
    out = oracle.pwc_warp(x, flo, align_corners, fmad=1)
    if align_corners:
        # (without align_corners a whole-pixel flow does not land on a whole sample position: no weight is exactly 0)
        assert zero_w.any(), "an in-map corner of weight exactly 0 reads a non-finite value"
        bi, yi, xi = np.nonzero(zero_w)
        assert np.isnan(out[bi, :, yi, xi]).any()
        assert np.isinf(out).any(), "a non-finite value read with a positive weight"
    assert masked.any(), "a masked-out pixel reads a non-finite value"
    bi, yi, xi = np.nonzero(masked)
    assert np.isnan(out[bi, :, yi, xi]).any(), "inf * mask 0"
    assert np.isfinite(out).mean() >= 0.5


@pytest.mark.parametrize("shape", fe.MINDEPTH_SHAPES)
def test_mindepth_inputs(oracle, shape):
    flow, wgt, count0 = fe.mindepth_inputs(shape, np.random.default_rng([SEED, shape[2]]))
    B, H, W = shape
    out, count = oracle.mindepthflowproj_fwd(flow, wgt, 0, count0=count0)
    changed = count != count0
    # a negative weight won over a negative floor; an infinite weight registered; equal weights and zeros of either sign lost
    assert (changed & (count < 0)).any() and (count[changed] == np.inf).any()
    valid, L, T = pt.targets(flow[0, 0], flow[0, 1], H, W)
    eq = valid & (wgt[0, 0] == count0[0, 0][T, L])
    assert eq.sum() >= 12
    zeros = valid & (wgt[0, 0] == 0) & (count0[0, 0][T, L] == 0)
    assert zeros.sum() >= 8 and (np.signbit(wgt[0, 0][zeros]) != np.signbit(count0[0, 0][T, L][zeros])).any()
    assert not (flow == 0).any(), "a zero flow would make the sign of a filled zero depend on the order"
    out1, _ = oracle.mindepthflowproj_fwd(flow, wgt, 1, count0=count0)
    assert not np.array_equal(out1, out) and np.isfinite(out1).all()


# ------------------------------------------------------------------ FilterInterpolation

FI_KERNELS = [("lds", True, 4), ("lds", False, 4), ("n", True, 2), ("n", True, 5), ("n", True, 6), ("blend", True, 4),
              ("multi", True, 4), ("f16", True, 4), ("defor", True, 4), ("defor", True, 6)]


def _fi_refs(oracle, kernel, c):
    if kernel == "f16":
        return [oracle.filterinterp_ori_fwd_f16(c["img"], c["flow"], c["filt"], fmad=1)]
    if kernel == "defor":
        return [oracle.filterinterp_defor_fwd(v, c["img"], c["flow"], c["filt"], c["off"], fmad=1) for v in (0, 1, 2)]
    return [oracle.filterinterp_ori_fwd(c["img"], c["flow"], c["filt"], fmad=1, nthreads=8)]


@pytest.mark.parametrize("kernel,aligned,fs", FI_KERNELS)
@pytest.mark.parametrize("C", [3, 9])
def test_planted_filterinterp_caps(oracle, kernel, aligned, fs, C):
    """Per kernel and window class, through the oracle: a NaN output, an infinite output, at least half finite; every
    class of the kernel's table still owns a tile after the flows were planted; invalid pixels copy their input."""
    from tests import fi_windows as fw
    c = fe.fi_case(kernel, C, aligned, fs)
    assert c["all_classes"] <= set(c["labels"].ravel()), c["all_classes"] - set(c["labels"].ravel())
    kinds = {p[0].split(":")[0] for p in c["planted"]}
    assert kinds == {"img", "filt", "flow"}
    assert len({p[1] for p in c["planted"] if p[0].startswith("flow")}) == 2, "flows in tiles of two classes"
    valid = fw.samples(c["flow"], c["h"], c["w"])[0]
    planted_flow = np.zeros(valid.shape, bool)
    for what, _, b, y, x in c["planted"]:
        if what.startswith("flow"):
            planted_flow[b, y, x] = True
    assert (planted_flow & ~valid).sum() >= 10 and (planted_flow & valid).any()
    for ref in _fi_refs(oracle, kernel, c):
        for label, (has_nan, has_inf, finite) in fe.class_caps(ref, c["pix"]).items():
            assert has_nan and has_inf and finite >= 0.5, (label, has_nan, has_inf, finite)
        inv = np.broadcast_to(~valid[:, None], ref.shape)
        assert fe.same_bits_nan_aware(ref[inv], c["img"][inv]), "invalid pixels copy the input through"
        if kernel == "f16":
            fin = np.abs(ref[np.isfinite(ref)].astype(np.float64))
            assert fin.max() < 0.99 * 65504, "no finite result within 1 % of the largest half"
            assert fe.clamped_windows(c["flow"], c["h"], c["w"]).any()
