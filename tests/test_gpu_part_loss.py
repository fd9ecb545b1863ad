"""`-m gpu`: the fused training losses -- vfi_part_loss_forward / vfi_part_loss_backward and fused.part_loss.

  1. values against float64: |v - ref| <= K 2^-24 |ref| (every term is positive, so the bound is relative), K counted along
     one term in tests/part_loss.py: K = 6 for the pixel and symmetry losses (subtraction 1, square 1/2, add 1/2, sqrt 1,
     double sum < 1, final rounding 1, one of slack for second-order terms), K = 11 + 2 ci amax for the total variation
     (T 3.5, T_0 + T_1 1, product 1, expf 1 ulp = 2, the exponent's 2 ci roundings of a sum <= amax = 2 ci max|dI|, double
     sum < 1, mean 1, the add of the two means 1); images are drawn from [0, 1], so amax <= 2 ci.  With neg_psnr the value
     log(l_b) / 100 is not a sum of positive terms: the bound is the absolute one of part_loss.value_bounds (the error of
     l_b passes through the logarithm at its full size).  No measured constant goes in and no element is left out;
  2. the pixel and symmetry gradients: bit for bit the float32 mirror (elementwise, correctly rounded divide and sqrt);
  3. the flow gradient of the total variation, alone and with the symmetry term: within the absolute bound of
     part_loss.flow_grad_bound against float64 (the sum of the bounds of at most four terms, which can cancel);
  4. shapes: the smallest legal one, H = 2 with a row tail, one 16-byte unit per row, one unit plus a tail, a batch of 3,
     and BIG, which has more partials per sample than one pass of the finish workgroup takes; nd in {1, 2, 4}, with and
     without flows, target and neg_psnr; H = 1 and W = 1 without flows (legal) and with (shape error);
  5. views (misaligned base, channel slice, row- and batch-strided): the same bits as their dense copies;
  6. two runs give identical bits;
  7. requested gradients are fully written, what lies around them and what is not requested is untouched;
  8. autograd = the C-ABI call bit for bit; `pixel_loss[1]` alone gives gradients to that diff only;
  9. FlowProject_from_quarter -> FilterInterpolate -> part_loss backpropagates to flow_q, reproducibly;
 10. the target shapes run and meet bound 1.
"""
import itertools

import numpy as np
import pytest

from tests import part_loss as M
from tests.test_gpu_parity import cpu, gpu, f32, torch_mod, cabi  # noqa: F401  (fixtures)
from tests.test_part_loss_host import make_inputs

pytestmark = pytest.mark.gpu

f64 = np.float64
EPS = 1e-6
SMALL = [(1, 1, 2, 2), (1, 3, 2, 5), (2, 3, 3, 4), (1, 3, 5, 9), (3, 3, 17, 67)]
# ceil(C H ceil(W / 4) / DIFF_BLOCK_UNITS) = 259 diff partials and 1035 flow partials per sample, both above FINISH_THREADS
BIG = (1, 1, 1030, 1028)
assert min(M.partial_counts(*BIG)) > M.FINISH_THREADS and M.partial_counts(*BIG)[0] < 2 * M.FINISH_THREADS
CONFIGS = list(itertools.product([1, 2, 4], [False, True], [False, True], [False, True]))    # nd, flows, target, neg_psnr
CASES = [(s, c) for s in SMALL for c in CONFIGS] + [(BIG, (1, True, False, False)), (BIG, (2, True, True, True)),
                                                    (BIG, (4, False, False, True))]


@pytest.fixture(scope="module")
def fused(cabi):  # noqa: F811
    from vfidkr_amd import fused as f
    return f


class Case:
    def __init__(self, torch, shape, nd, with_flows, with_target, neg, seed=0):
        B, C, H, W = shape
        rng = np.random.default_rng(seed + B + 10 * C + 100 * H + 1000 * W + nd)
        self.np = make_inputs(rng, B, C, H, W, nd, with_target)
        self.shape, self.nd, self.neg, self.with_flows = shape, nd, neg, with_flows
        diffs, target, flows, images = self.np
        if not with_flows:
            self.np = (diffs, target, None, None)
        self.diffs = [gpu(torch, d) for d in diffs]
        self.target = gpu(torch, target) if with_target else None
        self.flows = [gpu(torch, f) for f in flows] if with_flows else [None, None]
        self.images = [gpu(torch, i) for i in images] if with_flows else [None, None]
        self.gv_np = rng.uniform(0.5, 2.0, nd + 2).astype(f32) * rng.choice([-1.0, 1.0], nd + 2).astype(f32)
        self.gv = gpu(torch, self.gv_np)

    def forward(self, torch, cabi, tensors=None):  # noqa: F811
        diffs, target, flows, images = tensors or (self.diffs, self.target, self.flows, self.images)
        values = torch.full((self.nd + 2,), float("nan"), device="cuda:0")
        means = torch.full((self.nd * self.shape[0],), float("nan"), device="cuda:0")
        assert cabi.part_loss_forward(diffs, target, *flows, *images, EPS, self.neg, values, means) == 0
        return values, means

    def backward(self, torch, cabi, means, mask, want_diffs=None, want_flows=(True, True), tensors=None, outs=None):  # noqa: F811
        diffs, target, flows, images = tensors or (self.diffs, self.target, self.flows, self.images)
        want_diffs = [True] * self.nd if want_diffs is None else want_diffs
        nan = lambda t: torch.full_like(t, float("nan"), memory_format=torch.contiguous_format)    # noqa: E731
        if outs is None:
            gds = [nan(d) if w else None for d, w in zip(diffs, want_diffs)]
            gfs = [nan(f) if (w and self.with_flows) else None for f, w in zip(flows, want_flows)]
        else:
            gds, gfs = outs
        assert cabi.part_loss_backward(diffs, target, *flows, *images, EPS, self.neg, self.gv, means, mask, gds, *gfs) == 0
        return gds, gfs


def check_pixel_grads(c, gds, means):
    diffs, target, _, _ = c.np
    m = cpu(means).reshape(c.nd, -1)
    for i, g in enumerate(gds):
        want = M.pixel_grad(diffs[i], target, c.gv_np[i], EPS, c.neg, m[i])
        assert np.array_equal(cpu(g), want), "pixel gradient %d differs from the mirror" % i


@pytest.mark.parametrize("shape,config", CASES, ids=lambda v: "x".join(str(int(x)) for x in v))
def test_values_and_gradients(torch_mod, cabi, shape, config):  # noqa: F811
    torch = torch_mod
    nd, with_flows, with_target, neg = config
    c = Case(torch, shape, nd, with_flows, with_target, neg)
    diffs, target, flows, images = c.np
    values, means = c.forward(torch, cabi)
    got = cpu(values).astype(f64)
    ref = M.reference64(diffs, target, flows, images, EPS, neg)
    bound = M.value_bounds(ref, diffs, target, flows, images, EPS, neg)
    print("values", got, "ref", ref, "err/bound", np.abs(got - ref) / np.maximum(bound, 1e-300))
    assert not np.isnan(got).any()
    assert np.all(np.abs(got - ref) <= bound)
    if not with_flows:
        assert got[nd] == 0 and got[nd + 1] == 0
    # the per-sample means: K_PIXEL roundings
    for i in range(nd):
        x = M.diff_of(diffs[i].astype(f64), None if target is None else target.astype(f64))
        l64 = M.charbonnier(x, M.e2_of(EPS, f64)).reshape(shape[0], -1).mean(1)
        assert np.all(np.abs(cpu(means).reshape(nd, -1)[i].astype(f64) - l64) <= M.K_PIXEL * M.U * l64)
    # gradients: everything at once, then each flow loss alone
    full = (1 << (nd + 2)) - 1
    gds, gfs = c.backward(torch, cabi, means, full)
    check_pixel_grads(c, gds, means)
    if not with_flows:
        return
    g_tv, g_sym = c.gv_np[nd], c.gv_np[nd + 1]
    _, sym_only = c.backward(torch, cabi, means, 2 << nd, want_diffs=[False] * nd)
    _, tv_only = c.backward(torch, cabi, means, 1 << nd, want_diffs=[False] * nd)
    for s in range(2):
        f, other, img = flows[s], flows[1 - s], images[s]
        assert np.array_equal(cpu(sym_only[s]), M.sym_grad(f, other, g_sym, EPS)), "symmetry gradient differs from the mirror"
        for got_g, gs in ((tv_only[s], None), (gfs[s], g_sym)):
            ref_g = M.flow_grad(f, other, img, g_tv, gs, EPS, dtype=f64)
            b = M.flow_grad_bound(f, other, img, g_tv, gs, EPS)
            err = np.abs(cpu(got_g).astype(f64) - ref_g)
            print("flow %d grad (sym %s): max err %.3g, max err/bound %.3g" % (s, gs is not None, err.max(),
                                                                               (err / np.maximum(b, 1e-300)).max()))
            assert not np.isnan(cpu(got_g)).any() and np.all(err <= b)


@pytest.mark.parametrize("shape", [(2, 3, 1, 7), (2, 3, 5, 1), (1, 1, 1, 1)], ids=str)
def test_single_row_and_single_column(torch_mod, cabi, shape):  # noqa: F811
    torch = torch_mod
    c = Case(torch, shape, 2, False, True, False)
    diffs, target, _, _ = c.np
    values, means = c.forward(torch, cabi)
    ref = M.reference64(diffs, target, None, None, EPS, False)
    assert np.all(np.abs(cpu(values).astype(f64) - ref) <= M.value_bounds(ref, diffs, target, None, None, EPS, False))
    gds, _ = c.backward(torch, cabi, means, 0x3)
    check_pixel_grads(c, gds, means)
    # with flows the total variation's mean would be over nothing
    z = lambda ch: torch.zeros((shape[0], ch) + shape[2:], device="cuda:0")     # noqa: E731
    assert cabi.part_loss_forward(c.diffs, c.target, z(2), z(2), z(3), z(3), EPS, False, values, means) == 1
    assert cabi.part_loss_backward(c.diffs, c.target, z(2), z(2), z(3), z(3), EPS, False, c.gv, means, 0xF, None, z(2), None) == 1


VIEWS = ["misaligned", "channel", "rows", "batch"]


def as_view(torch, t, kind, fill=None):
    """a view of kind `kind` holding t's values inside a wider tensor (filled with `fill`, default zeros)"""
    if t is None:
        return None
    B, C, H, W = t.shape
    wide = {"misaligned": (B, C, H, W + 1), "channel": (B, C + 2, H, W), "rows": (B, C, 2 * H, W), "batch": (2 * B, C, H, W)}[kind]
    base = torch.full(wide, 0.0 if fill is None else fill, device=t.device)
    view = {"misaligned": base[..., 1:], "channel": base[:, 1:1 + C], "rows": base[:, :, ::2], "batch": base[::2]}[kind]
    view.copy_(t)
    view.base_tensor = base
    return view


@pytest.mark.parametrize("kind", VIEWS)
@pytest.mark.parametrize("shape,neg", [((2, 3, 5, 8), False), ((2, 3, 5, 9), True), ((3, 2, 4, 12), False)], ids=str)
def test_views_give_the_bits_of_their_dense_copies_and_writes_stay_inside(torch_mod, cabi, shape, neg, kind):  # noqa: F811
    torch = torch_mod
    c = Case(torch, shape, 2, True, True, neg, seed=5)
    values, means = c.forward(torch, cabi)
    full = 0xF
    gds, gfs = c.backward(torch, cabi, means, full)
    # 6. a second run: identical bits
    values2, means2 = c.forward(torch, cabi)
    gds2, gfs2 = c.backward(torch, cabi, means2, full)
    assert torch.equal(values, values2) and torch.equal(means, means2)
    assert all(torch.equal(a, b) for a, b in zip(gds + gfs, gds2 + gfs2))
    v = lambda t: as_view(torch, t, kind)                                # noqa: E731
    tensors = ([v(d) for d in c.diffs], v(c.target), [v(f) for f in c.flows], [v(i) for i in c.images])
    vvalues, vmeans = c.forward(torch, cabi, tensors)
    assert torch.equal(values, vvalues) and torch.equal(means, vmeans)
    nan = float("nan")
    outs = ([as_view(torch, d, kind, nan) for d in c.diffs], [as_view(torch, f, kind, nan) for f in c.flows])
    for o in outs[0] + outs[1]:
        o.fill_(nan)
    vgds, vgfs = c.backward(torch, cabi, vmeans, full, tensors=tensors, outs=outs)
    for a, b in zip(gds + gfs, vgds + vgfs):
        assert not torch.isnan(b).any() and torch.equal(a, b)
        # 7. around the view nothing was written: as many NaNs in the wide tensor as it has cells outside the view
        assert int(torch.isnan(b.base_tensor).sum()) == b.base_tensor.numel() - b.numel()


def test_only_what_is_asked_for_is_written(torch_mod, cabi):  # noqa: F811
    torch = torch_mod
    c = Case(torch, (2, 3, 6, 10), 2, True, False, False, seed=9)
    _, means = c.forward(torch, cabi)
    ref_gds, ref_gfs = c.backward(torch, cabi, means, 0xF)
    # one diff and one flow asked for: the same bits as in the full call
    gds, gfs = c.backward(torch, cabi, means, 0xF, want_diffs=[False, True], want_flows=(False, True))
    assert gds[0] is None and gfs[0] is None
    assert torch.equal(gds[1], ref_gds[1]) and torch.equal(gfs[1], ref_gfs[1])
    # a requested gradient whose losses are all masked out is written with zeros
    gds, gfs = c.backward(torch, cabi, means, 0x2)
    assert torch.equal(gds[1], ref_gds[1]) and not gds[0].any() and not gfs[0].any() and not gfs[1].any()
    # the pixel losses alone with no flow gradient: flows and images are not read (a call without them gives the same bits)
    gds2 = [torch.full_like(d, float("nan")) for d in c.diffs]
    assert cabi.part_loss_backward(c.diffs, None, None, None, None, None, EPS, False, c.gv, means, 0x3, gds2) == 0
    assert torch.equal(gds2[0], ref_gds[0]) and torch.equal(gds2[1], ref_gds[1])


def test_autograd_equals_the_c_abi_call(torch_mod, cabi, fused):  # noqa: F811
    torch = torch_mod
    c = Case(torch, (3, 3, 17, 67), 2, True, True, False, seed=11)
    values, means = c.forward(torch, cabi)
    d = [t.clone().requires_grad_(True) for t in c.diffs]
    fl = [t.clone().requires_grad_(True) for t in c.flows]
    pixel, offset, sym = fused.part_loss(d, [fl], [None], c.images, EPS, target=c.target)
    assert len(pixel) == 2 and len(offset) == 1 and len(sym) == 1 and all(v.dim() == 0 for v in pixel + offset + sym)
    assert torch.equal(torch.stack(pixel + offset + sym).detach(), values)
    # train.py: the enhanced output's loss alone -- one diff gets a gradient, nothing else is computed
    w = [float(x) for x in c.gv_np]
    (w[1] * pixel[1]).backward(retain_graph=True)
    ref_gds, ref_gfs = c.backward(torch, cabi, means, 0xF)
    assert d[0].grad is None and fl[0].grad is None and fl[1].grad is None
    assert torch.equal(d[1].grad, ref_gds[1])
    d[1].grad = None
    # every loss
    (w[0] * pixel[0] + w[1] * pixel[1] + w[2] * offset[0] + w[3] * sym[0]).backward()
    for got, want in zip([t.grad for t in d + fl], ref_gds + ref_gfs):
        assert torch.equal(got, want)
    # without grad mode, or with nothing that requires grad: the plain forward
    with torch.no_grad():
        p2, o2, s2 = fused.part_loss(d, [fl], [None], c.images, EPS, target=c.target)
    p3, o3, s3 = fused.part_loss(c.diffs, [c.flows], [None], c.images, EPS, target=c.target)
    for vals in (p2 + o2 + s2, p3 + o3 + s3):
        assert all(v.grad_fn is None and not v.requires_grad for v in vals)
        assert torch.equal(torch.stack(vals), values)
    # no flows: a zero offset loss, as in the reference; neg_psnr goes through
    p4, o4, s4 = fused.part_loss(d, [[None, None]], [None], c.images, EPS, use_negPSNR=True)
    assert len(p4) == 2 and float(o4[0]) == 0.0 and s4 == []
    p4[0].backward()
    assert d[1].grad is not None and torch.isfinite(d[0].grad).all()


def test_chain_from_the_quarter_resolution_flow_to_the_losses(torch_mod, cabi, fused):  # noqa: F811
    torch = torch_mod
    B, H, W = 2, 32, 48
    g = torch.Generator().manual_seed(3)
    base = torch.rand((B, 3, H, W + 4), generator=g)
    frame0, frame2, target = base[..., :W].cuda(), base[..., 4:].cuda(), base[..., 2:W + 2].cuda()
    q = [(torch.randn((B, 2, H // 4, W // 4), generator=g) * 0.05).cuda() for _ in range(2)]
    k = [torch.softmax(torch.randn((B, 16, H, W), generator=g), 1).cuda() for _ in range(2)]

    def run():
        q0, q2 = (t.clone().requires_grad_(True) for t in q)
        p0 = fused.FlowProject_from_quarter(q0, 20.0, [0.5], fillhole=False)[0]
        p2 = fused.FlowProject_from_quarter(q2, 20.0, [0.5], fillhole=False)[0]
        blend, o0, o2 = fused.FilterInterpolate(frame0, frame2, [p0, p2], k, 16, 0.5)
        pixel, offset, sym = fused.part_loss([o0, blend], [[p0, p2]], [None], [frame0, frame2], EPS, target=target)
        total = pixel[1] + 0.01 * offset[0] + 0.01 * sym[0]
        total.backward()
        return total.detach(), q0.grad, q2.grad

    a, b = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.isfinite(a[1]).all() and torch.isfinite(a[2]).all() and bool(a[1].abs().sum() > 0) and bool(a[2].abs().sum() > 0)


@pytest.mark.parametrize("shape", [(3, 3, 256, 448), (1, 3, 1080, 1920)], ids=["vimeo", "1080p"])
def test_target_shapes_run_and_meet_the_value_bound(torch_mod, cabi, shape):  # noqa: F811
    torch = torch_mod
    c = Case(torch, shape, 2, True, True, False, seed=21)
    diffs, target, flows, images = c.np
    values, means = c.forward(torch, cabi)
    got = cpu(values).astype(f64)
    ref = M.reference64(diffs, target, flows, images, EPS, False)
    bound = M.value_bounds(ref, diffs, target, flows, images, EPS, False)
    print("values", got, "ref", ref, "err/bound", np.abs(got - ref) / bound)
    assert np.all(np.abs(got - ref) <= bound)
    gds, gfs = c.backward(torch, cabi, means, 0xF)
    assert all(bool(torch.isfinite(t).all()) for t in gds + gfs)
    check_pixel_grads(c, gds[:1], means)
