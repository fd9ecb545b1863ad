"""FlowProjection / DepthFlowProjection forward through every K1 instantiation and every per-tile regime of
tests/proj_tiles.py (empty tiles, retries with shift 1 / 2 / >= 3, wide cells, 2-4 weight classes, the frame's last
row and column, negative weights, lopsided flows), each cell checked against float64 sums of the fp32 addends.

K1 instantiations, all reached through the public ABI: proj_pull_lean (contiguous tensors), proj_pull<., true> (a count
view at an odd element offset: no 16-byte stores) and proj_pull<., false> (flow and output rows of w + 1 floats).

Bounds, from csrc/projection.hip.  A tile adds every addend a (-fx, or -d*fx formed in fp32) as round(a * 2^k) with k
the tile's scale for that component and weight class after the retry shift (proj_tiles.scales): an error of at most
2^-(k+1) per addend, summed exactly; the class sum is converted to float once (one rounding, u = 2^-24 relative) and
the classes are added in fp32 (one rounding each).
  * FlowProjection: count exact; out bit-equal to proj_tiles.predict_flowprojection; independently
    |out - (-sum fx / n)| <= 2^-(k+1) + 2^-23 |want| (the n addends' errors over n, the conversion and the division).
  * DepthFlowProjection, per component: dN <= sum_j n_j 2^-(kv_j+1) + 2 ncls u S_N, dD likewise with kc and S_D (S =
    float64 sum of |addends|), and |out - N/D| <= (dN + |N/D| dD) / (D - dD) + ulp/2 where D > dD; count within dD of D.
    Where D <= dD (weights that cancel to within the classes' rounding) the cell may come out as a hole or not
    (DESIGN.md 4.2): count is still within dD of D.  out and count are also bit-equal to the mirror's restatement.
  * the hole mask is the oracle's; fillhole = 1 equals the oracle's pass 3 applied to this library's own fillhole = 0
    result, bit for bit; a second call gives the same bits; dyadic fields equal the oracle bit for bit.
A failure names the regime labels of the worst tile, the tile and the cell.
"""
import numpy as np
import pytest

from tests import proj_tiles as pt
from tests.test_gpu_parity import cpu, gpu, torch_mod, cabi  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

f32 = np.float32
U = 2.0 ** -24


@pytest.fixture(scope="module")
def fields():
    cache = {}

    def get(kind, dyadic, B=1):
        key = (kind, dyadic, B)
        if key not in cache:
            cache[key] = pt.build_field(kind, np.random.default_rng(100 + 10 * dyadic + (kind == "depth")), B, dyadic=dyadic)
        return cache[key]
    return get


def _tensors(torch, variant, flow, depth):
    """(flow, depth, count, out) views that make project_forward_list pick `variant`; outputs NaN-filled."""
    B, _, h, w = flow.shape
    nan = float("nan")
    dev = "cuda:0"
    if variant == "pull_scalar":
        fb = torch.zeros((B, 2, h, w + 1), device=dev)
        fb[..., :w] = gpu(torch, flow)
        fl = fb[..., :w]
        out = torch.full((B, 2, h, w + 1), nan, device=dev)[..., :w]
    else:
        fl = gpu(torch, flow)
        out = torch.full((B, 2, h, w), nan, device=dev)
    if variant == "pull_vec":
        count = torch.full((B * h * w + 1,), nan, device=dev)[1:].view(B, 1, h, w)
    else:
        count = torch.full((B, 1, h, w), nan, device=dev)
    dp = None if depth is None else gpu(torch, depth)
    assert pt.dispatch_of(fl, count, out, dp)[1] == variant
    return fl, dp, count, out


def _run(cabi, fl, dp, count, out, fillhole):
    if dp is None:
        assert cabi.flowprojection_forward(fl, count, out, fillhole) == 0
    else:
        assert cabi.depthflowprojection_forward(fl, dp, count, out, fillhole) == 0
    return cpu(out), cpu(count)


def _report(m, bad, what):
    """Assert no cell is bad; otherwise name the labels, tile and cell of the worst one."""
    if not bad.any():
        return
    labels = m.labels()
    per_label = {}
    cells = np.argwhere(bad.any(1))                         # [B, C, h, w] -> (b, y, x)
    b, y, x = cells[0]
    for (bb, yy, xx) in cells:
        for lab in labels[(bb, yy // pt.TH, xx // pt.TW)]:
            per_label[lab] = per_label.get(lab, 0) + 1
    tile = (b, y // pt.TH, x // pt.TW)
    pytest.fail("%s: %d bad cells, by label %s; first at cell %s of tile %s %s" % (
        what, len(cells), per_label, (b, y, x), tile, sorted(labels[tile])))


def _float64_sums(flow, depth):
    """per cell: N (2 components), D, n, each as float64 sums over the reference's four targets"""
    B, _, h, w = flow.shape
    N = np.zeros((B, 2, h * w))
    D = np.zeros((B, h * w))
    for b in range(B):
        valid, L, T = pt.targets(flow[b, 0], flow[b, 1], h, w)
        R, Bm = np.minimum(L + 1, w - 1), np.minimum(T + 1, h - 1)
        d = np.ones((h, w), f32) if depth is None else depth[b, 0]
        for ty, tx in ((T, L), (T, R), (Bm, L), (Bm, R)):
            idx = (ty * w + tx)[valid]
            for c in range(2):
                a = (-d * flow[b, c]).astype(f32) if depth is not None else -flow[b, c]
                np.add.at(N[b, c], idx, a[valid].astype(np.float64))
            np.add.at(D[b], idx, d[valid].astype(np.float64))
    return N.reshape(B, 2, h, w), D.reshape(B, 1, h, w)


def _check_bounds(m, flow, depth, out, count):
    N, D = _float64_sums(flow, depth)
    if depth is None:
        n = m.plane(m.n)[:, None]
        assert np.array_equal(count, n.astype(f32)), "count"
        want = np.where(n > 0, N / np.maximum(n, 1), 0)
        kx = np.stack([m.tile_plane(m.kvx[:, 0]), m.tile_plane(m.kvy[:, 0])], 1)
        bound = np.exp2(-(kx + 1.0)) + 2.0 ** -23 * np.abs(want)
        _report(m, np.abs(out - want) > bound, "FlowProjection out against float64")
        return
    ncl = m.ncls.reshape(-1)
    rnd = 2 * m.tile_plane(ncl)[:, None]
    dN = [sum(m.plane(m.cls_n[:, j]) * np.exp2(-(m.tile_plane(k[:, j]) + 1.0)) for j in range(pt.MAX_CLS))
          for k in (m.kvx, m.kvy)]
    dN = np.stack(dN, 1) + rnd * U * np.stack([m.plane(m.absx), m.plane(m.absy)], 1)
    dD = (sum(m.plane(m.cls_n[:, j]) * np.exp2(-(m.tile_plane(m.kc[:, j]) + 1.0)) for j in range(pt.MAX_CLS))[:, None]
          + rnd * U * m.plane(m.absc)[:, None])
    _report(m, np.abs(count - D) > dD, "DepthFlowProjection count against float64")
    ok = D > dD
    want = np.where(ok, N / np.where(ok, D, 1), 0)
    ulp = np.abs(np.spacing(want.astype(f32))).astype(np.float64)
    bound = (dN + np.abs(want) * dD) / np.where(ok, D - dD, 1) + ulp / 2
    _report(m, ok & (np.abs(out - want) > bound), "DepthFlowProjection out against float64")


@pytest.mark.parametrize("kind", ["flow", "depth"])
@pytest.mark.parametrize("variant", ["lean", "pull_vec", "pull_scalar"])
def test_regimes_random_fields(torch_mod, cabi, oracle, fields, kind, variant):
    torch = torch_mod
    flow, depth = fields(kind, False)
    m = pt.mirror(flow, depth, variant)
    assert not m.fallback and pt.covered(m.labels()) >= set(pt.all_regimes(kind))
    T = _tensors(torch, variant, flow, depth)
    out0, count0 = _run(cabi, *T, 0)
    pout, pcount = m.predict()
    _report(m, pcount != count0, "count against the mirror")
    _report(m, pout != out0, "out against the mirror")
    _check_bounds(m, flow, depth, out0.astype(np.float64), count0.astype(np.float64))
    # the hole mask: the oracle's (DepthFlowProjection: where the weight sum is clear of the rounding)
    ref, rcount = (oracle.flowproj_fwd(flow, 0) if depth is None else oracle.depthflowproj_fwd(flow, depth, 0))
    same = (count0 > 0) == (rcount > 0)
    if depth is not None:
        _, D = _float64_sums(flow, depth)
        same |= np.abs(D) <= 1e-3 * np.maximum(m.plane(m.absc)[:, None], 1e-30)
    _report(m, ~same, "hole mask against the oracle")
    # the same bits again
    out1, count1 = _run(cabi, *_tensors(torch, variant, flow, depth), 0)
    assert np.array_equal(out1, out0, equal_nan=True) and np.array_equal(count1, count0)
    # hole filling on its own: the oracle's pass 3 on this library's fillhole = 0 result
    outf, countf = _run(cabi, *_tensors(torch, variant, flow, depth), 1)
    assert np.array_equal(countf, count0)
    _report(m, outf != oracle.proj_fillhole(count0, out0), "fillhole = 1 against the oracle's fill of fillhole = 0")


@pytest.mark.parametrize("kind", ["flow", "depth"])
@pytest.mark.parametrize("variant", ["lean", "pull_vec", "pull_scalar"])
@pytest.mark.parametrize("fillhole", [0, 1])
def test_regimes_dyadic_fields_equal_the_oracle(torch_mod, cabi, oracle, fields, kind, variant, fillhole):
    torch = torch_mod
    flow, depth = fields(kind, True)
    m = pt.mirror(flow, depth, variant)
    assert pt.covered(m.labels()) >= set(pt.all_regimes(kind))
    out, count = _run(cabi, *_tensors(torch, variant, flow, depth), fillhole)
    ref, rcount = oracle.flowproj_fwd(flow, fillhole) if depth is None else oracle.depthflowproj_fwd(flow, depth, fillhole)
    _report(m, count != rcount, "count against the oracle (dyadic)")
    _report(m, out != ref, "out against the oracle (dyadic)")


def test_list_form_over_the_regimes(torch_mod, cabi, fields):
    """flowprojection_forward_batch, 3 items of 2 images: every item equals the mirror (which sees 6 images)."""
    torch = torch_mod
    items = [fields("flow", False, 2)[0]] + [fields("flow", True, 2)[0], fields("flow", False, 2)[0][::-1].copy()]
    B, _, h, w = items[0].shape
    counts = [torch.full((B, 1, h, w), float("nan"), device="cuda:0") for _ in items]
    outs = [torch.full((B, 2, h, w), float("nan"), device="cuda:0") for _ in items]
    assert cabi.flowprojection_forward_batch([gpu(torch, f) for f in items], counts, outs, 0) == 0
    for f, c, o in zip(items, counts, outs):
        m = pt.mirror(f, None, "lean")
        pout, pcount = m.predict()
        _report(m, cpu(c) != pcount, "list form count")
        _report(m, cpu(o) != pout, "list form out")


@pytest.mark.parametrize("kind", ["flow", "depth"])
def test_up4_over_converging_fields(torch_mod, cabi, fields, kind):
    """*_forward_up4: the x4 upsample inside the call, then the projection -- equal to the mirror of the upsampled
    flow that flow_upsample4 gives; the quarter field converges on a few cells (retries, a wide cell)."""
    torch = torch_mod
    rng = np.random.default_rng(9)
    hq, wq = 40, 96
    fq = rng.uniform(-0.2, 0.2, (1, 2, hq, wq)).astype(f32)
    ys, xs = np.meshgrid(np.arange(hq), np.arange(wq), indexing="ij")
    for (cy, cx, r) in ((10, 20, 4), (25, 60, 7)):
        near = (np.abs(ys - cy) <= r) & (np.abs(xs - cx) <= r)
        fq[0, 0][near] = (cx - xs[near]) + 0.1
        fq[0, 1][near] = (cy - ys[near]) + 0.1
    m0, m1 = 4.0, 1.0                                      # quarter-resolution pixels -> full-resolution ones
    h, w = 4 * hq, 4 * wq
    full = torch.zeros((1, 2, h, w), device="cuda:0")
    assert cabi.flow_upsample4(gpu(torch, fq), full, m0, m1) == 0
    flow = cpu(full)
    depth = rng.uniform(0.25, 1.0, (1, 1, h, w)).astype(f32) if kind == "depth" else None
    m = pt.mirror(flow, depth, "lean")
    lab = pt.covered(m.labels())
    assert not m.fallback and "wide_cell" in lab and "retry_3+" in lab, lab
    count = torch.full((1, 1, h, w), float("nan"), device="cuda:0")
    out = torch.full((1, 2, h, w), float("nan"), device="cuda:0")
    if depth is None:
        assert cabi.flowprojection_forward_up4(gpu(torch, fq), count, out, m0, m1, 0) == 0
    else:
        assert cabi.depthflowprojection_forward_up4(gpu(torch, fq), gpu(torch, depth), count, out, m0, m1, 0) == 0
    pout, pcount = m.predict()
    _report(m, cpu(count) != pcount, "up4 count")
    _report(m, cpu(out) != pout, "up4 out")
