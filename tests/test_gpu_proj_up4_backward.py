"""`-m gpu`: training through the quarter-resolution flow -- vfi_flow_upsample4_backward, vfi_[depth]flowprojection_backward_up4
and the autograd Functions of fused.forward_flownets_upsample / fused.FlowProject_from_quarter.

  1. bit for bit: the fused backward = vfi_flow_upsample4 -> forward (count, out) -> vfi_[depth]flowprojection_backward into
     zeros -> vfi_flow_upsample4_backward; grad_depth_i = the oracle's; vfi_flow_upsample4_backward = the float32 mirror
     (tests/proj_up4_backward.py);
  2. against float64: |grad_q - ref64| <= (n + 12) 2^-24 S per element -- the forward error bound of an ordered fp32 sum of n
     terms (n additions, plus at most 12 roundings along one term: the divide and four adds inside G, two weight products,
     two multipliers, slack for fmaf); no element is left out, no measured constant goes in;
  3. reproducible, fully written, null grad_depth, strided views;
  4. autograd = the C-ABI call, bit for bit; no grad_fn and unchanged bits without grad;
  5. the chain flow_q -> FlowProject_from_quarter -> FilterInterpolate trains, reproducibly;
  6. the target shapes run.
"""
import numpy as np
import pytest

from tests import proj_up4_backward as M
from tests.test_gpu_parity import cpu, gpu, smooth_flow, f32, torch_mod, cabi  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

MUL0 = 20.0
MUL1 = [0.25, 0.5, 0.75, 0.125, 0.375, 0.625, 0.875, 1.0]
KINDS = ["smooth", "leave", "converge", "zero", "rough"]


@pytest.fixture(scope="module")
def fused(cabi):  # noqa: F811
    from vfidkr_amd import fused as f
    return f


def cases():
    """20 seeded shapes: hq, wq in 1..70 -- 1 x 1, below one 8 x 16 tile, no multiple of it, several tiles --, B in 1..3,
    nitems in 1..8; every flow kind several times"""
    fixed = [(1, 1, 1, 1), (2, 1, 9, 3), (1, 7, 1, 8), (1, 8, 16, 2), (3, 9, 17, 1), (1, 70, 70, 3), (2, 5, 33, 8), (1, 24, 48, 4)]
    rng = np.random.default_rng(2024)
    out = []
    for k in range(20):
        if k < len(fixed):
            B, hq, wq, n = fixed[k]
        else:
            B, hq, wq, n = int(rng.integers(1, 4)), int(rng.integers(1, 71)), int(rng.integers(1, 71)), int(rng.integers(1, 9))
        out.append((B, hq, wq, n, KINDS[k % len(KINDS)], 100 + k))
    return out


def make_flow_q(rng, kind, B, hq, wq, m1=0.5):
    """quarter-resolution flows whose upsampled MUL0 * MUL1 multiples are a few pixels (smooth, rough), leave the frame in
    places (leave: the invalid branch), pile onto a few cells (converge) or are zero"""
    if kind == "zero":
        return np.zeros((B, 2, hq, wq), f32)
    if kind == "converge":
        # F(x) ~ c - x for the item with multiplier m1: whole neighbourhoods land on a few target cells
        ys, xs = np.meshgrid(np.arange(hq, dtype=np.float64), np.arange(wq, dtype=np.float64), indexing="ij")
        cy, cx = rng.uniform(0, 4 * hq - 1), rng.uniform(0, 4 * wq - 1)
        q = np.stack([(cx - (4 * xs + 1.5)), (cy - (4 * ys + 1.5))]) / (MUL0 * m1)
        q = np.repeat(q[None], B, 0) + rng.uniform(-0.02, 0.02, (B, 2, hq, wq))
        return q.astype(f32)
    q = smooth_flow(rng, B, hq, wq, 0.4) if kind != "rough" else rng.uniform(-0.6, 0.6, (B, 2, hq, wq)).astype(f32)
    if kind == "leave":
        q[:, 0][rng.random((B, hq, wq)) < 0.25] = 1.0e3
        q[:, 1][rng.random((B, hq, wq)) < 0.1] = -1.0e3
    return q.astype(f32)


class Case:
    """the tensors of one call, the forward's count / out computed by the library itself (fillhole = 0, as in training)"""

    def __init__(self, torch, cabi, B, hq, wq, n, kind, seed, depth=False, shared_depth=False):  # noqa: F811
        rng = np.random.default_rng(seed)
        self.B, self.hq, self.wq, self.n, self.has_depth = B, hq, wq, n, depth
        H, W = 4 * hq, 4 * wq
        self.mul1 = [MUL1[(seed + i) % len(MUL1)] for i in range(n)]
        self.flow_q = gpu(torch, make_flow_q(rng, kind, B, hq, wq, self.mul1[0]))
        self.gouts = [gpu(torch, rng.standard_normal((B, 2, H, W)).astype(f32)) for _ in range(n)]
        d0 = gpu(torch, rng.uniform(0.1, 1.0, (B, 1, H, W)).astype(f32))
        self.depths = None if not depth else [d0 if shared_depth or i == 0 else
                                              gpu(torch, rng.uniform(0.1, 1.0, (B, 1, H, W)).astype(f32)) for i in range(n)]
        self.full, self.counts, self.outs = [], [], []
        for i in range(n):
            F = torch.empty((B, 2, H, W), device="cuda:0")
            assert cabi.flow_upsample4(self.flow_q, F, MUL0, self.mul1[i]) == 0
            count, out = torch.empty((B, 1, H, W), device="cuda:0"), torch.empty((B, 2, H, W), device="cuda:0")
            if depth:
                assert cabi.depthflowprojection_forward(F, self.depths[i], count, out, 0) == 0
            else:
                assert cabi.flowprojection_forward(F, count, out, 0) == 0
            self.full.append(F), self.counts.append(count), self.outs.append(out)

    def composition(self, torch, cabi):  # noqa: F811
        """the library's own two-call backward: (grad_q, [G_i], [grad_depth_i])"""
        Gs, gds = [], []
        for i in range(self.n):
            G = torch.zeros_like(self.full[i])
            if self.has_depth:
                gd = torch.zeros_like(self.depths[i])
                assert cabi.depthflowprojection_backward(self.full[i], self.depths[i], self.counts[i], self.outs[i], self.gouts[i],
                                                         G, gd) == 0
                gds.append(gd)
            else:
                assert cabi.flowprojection_backward(self.full[i], self.counts[i], self.gouts[i], G) == 0
            Gs.append(G)
        gq = torch.full_like(self.flow_q, float("nan"))
        assert cabi.flow_upsample4_backward(Gs, MUL0, self.mul1, gq) == 0
        return gq, Gs, gds

    def fused_call(self, torch, cabi, want_depth=True, flow_q=None, gouts=None, grad_q=None, outs=None):  # noqa: F811
        flow_q = self.flow_q if flow_q is None else flow_q
        gq = torch.full_like(self.flow_q, float("nan")) if grad_q is None else grad_q
        gds = None
        if self.has_depth and want_depth:
            gds = [torch.full_like(self.depths[i], float("nan")) for i in range(self.n)]
        assert cabi.flowprojection_backward_up4(flow_q, self.counts, self.gouts if gouts is None else gouts, MUL0, self.mul1, gq,
                                                self.depths, (outs or self.outs) if self.has_depth else None, gds) == 0
        return gq, gds


@pytest.mark.parametrize("depth", [False, True], ids=["flow", "depth"])
@pytest.mark.parametrize("B,hq,wq,n,kind,seed", cases())
def test_bit_for_bit_against_the_composition_and_float64(torch_mod, cabi, oracle, B, hq, wq, n, kind, seed, depth):  # noqa: F811
    torch = torch_mod
    c = Case(torch, cabi, B, hq, wq, n, kind, seed, depth=depth, shared_depth=seed % 2 == 0)
    ref_q, Gs, ref_gd = c.composition(torch, cabi)
    gq, gds = c.fused_call(torch, cabi)
    got = cpu(gq)
    assert not np.isnan(got).any()
    assert np.array_equal(got, cpu(ref_q))
    # vfi_flow_upsample4_backward = the mirror, bit for bit
    mirror32, _, _, _ = M.up4_backward([cpu(G) for G in Gs], MUL0, c.mul1)
    assert np.array_equal(cpu(ref_q), mirror32)
    # against float64, G_i from the oracle
    counts, gouts = [cpu(t) for t in c.counts], [cpu(t) for t in c.gouts]
    depths = [cpu(t) for t in c.depths] if depth else None
    outs = [cpu(t) for t in c.outs] if depth else None
    o32, ref64, S, nadd, oGs, ogds = M.proj_up4_backward(oracle, cpu(c.flow_q), MUL0, c.mul1, counts, gouts, depths, outs)
    err = np.abs(got.astype(np.float64) - ref64)
    bound = (nadd + 12) * 2.0 ** -24 * S
    print("case B=%d hq=%d wq=%d n=%d %s depth=%s: max err %.3g, max err/bound %.3g" %
          (B, hq, wq, n, kind, depth, err.max(), (err / np.maximum(bound, 1e-300)).max() if S.max() > 0 else 0.0))
    assert np.all(err <= bound)
    if depth:
        for i in range(n):
            assert np.array_equal(cpu(gds[i]), cpu(ref_gd[i])), i
            assert np.array_equal(cpu(gds[i]), ogds[i]), i
    if kind == "leave":
        valid = [np.abs(cpu(F)).max(1) < 500 for F in c.full]
        assert not all(v.all() for v in valid)              # (the invalid branch ran)
    if kind == "converge" and hq * wq > 16:
        assert max(float(cpu(t).max()) for t in c.counts) > (2.0 if depth else 8.0)      # (many sources per target cell)


def test_reproducible_and_self_contained(torch_mod, cabi):  # noqa: F811
    torch = torch_mod
    for depth in (False, True):
        c = Case(torch, cabi, 2, 21, 37, 3, "smooth", 7, depth=depth, shared_depth=True)
        gq, gds = c.fused_call(torch, cabi)
        gq2, gds2 = c.fused_call(torch, cabi)
        assert not torch.isnan(gq).any() and torch.equal(gq, gq2)
        if depth:
            for a, b in zip(gds, gds2):
                assert not torch.isnan(a).any() and torch.equal(a, b)
            gq3, none = c.fused_call(torch, cabi, want_depth=False)
            assert none is None and torch.equal(gq, gq3)
            # one wanted, the others not
            only = [None, torch.full_like(c.depths[1], float("nan")), None]
            gq4 = torch.full_like(gq, float("nan"))
            assert cabi.flowprojection_backward_up4(c.flow_q, c.counts, c.gouts, MUL0, c.mul1, gq4, c.depths, c.outs, only) == 0
            assert torch.equal(gq, gq4) and torch.equal(only[1], gds[1])
        # strided views: a channel slice of a wider tensor for flow_q, gout and grad_q
        wide_q = torch.randn((2, 5, 21, 37), device="cuda:0")
        wide_q[:, 2:4] = c.flow_q
        wide_g = [torch.randn((2, 4, 84, 148 + 3), device="cuda:0") for _ in range(3)]
        wide_o = [torch.randn((2, 4, 84, 148 + 3), device="cuda:0") for _ in range(3)]
        views, out_views = [], []
        for w_, o_, g, o in zip(wide_g, wide_o, c.gouts, c.outs):
            w_[:, 1:3, :, 2:150] = g
            o_[:, 1:3, :, 2:150] = o
            views.append(w_[:, 1:3, :, 2:150])
            out_views.append(o_[:, 1:3, :, 2:150])              # (the depth form addresses out like gout)
        wide_out = torch.full((2, 6, 21, 40), float("nan"), device="cuda:0")
        gq5, _ = c.fused_call(torch, cabi, want_depth=False, flow_q=wide_q[:, 2:4], gouts=views, grad_q=wide_out[:, 3:5, :, 1:38],
                               outs=out_views)
        assert torch.equal(gq5, gq)
        assert torch.isnan(wide_out[:, :3]).all() and torch.isnan(wide_out[:, 5:]).all() and torch.isnan(wide_out[..., 0]).all()
        # the standalone adjoint on the same kind of views
        ref = torch.full_like(gq, float("nan"))
        assert cabi.flow_upsample4_backward(c.gouts, MUL0, c.mul1, ref) == 0
        wide_out.fill_(float("nan"))
        assert cabi.flow_upsample4_backward(views, MUL0, c.mul1, wide_out[:, 3:5, :, 1:38]) == 0
        assert torch.equal(wide_out[:, 3:5, :, 1:38], ref) and torch.isnan(wide_out[:, :3]).all()
        again = torch.full_like(gq, float("nan"))
        assert cabi.flow_upsample4_backward(c.gouts, MUL0, c.mul1, again) == 0 and torch.equal(again, ref)


def test_upsample_backward_any_channel_count(torch_mod, cabi):  # noqa: F811
    torch = torch_mod
    rng = np.random.default_rng(5)
    for (B, C, hq, wq, n) in ((1, 1, 1, 1, 1), (2, 3, 5, 66, 2), (1, 5, 70, 3, 8), (3, 2, 4, 64, 3)):
        Gs = [rng.standard_normal((B, C, 4 * hq, 4 * wq)).astype(f32) for _ in range(n)]
        gq = torch.full((B, C, hq, wq), float("nan"), device="cuda:0")
        assert cabi.flow_upsample4_backward([gpu(torch, G) for G in Gs], MUL0, MUL1[:n], gq) == 0
        m32, ref64, S, nadd = M.up4_backward(Gs, MUL0, MUL1[:n])
        assert np.array_equal(cpu(gq), m32)
        assert np.all(np.abs(cpu(gq).astype(np.float64) - ref64) <= (nadd + 12) * 2.0 ** -24 * S)


# ------------------------------------------------------------------ 4. autograd

@pytest.mark.parametrize("mode", ["flow", "shared_depth", "unused_output", "nine_offsets"])
def test_from_quarter_autograd_equals_the_c_abi(torch_mod, cabi, fused, mode):  # noqa: F811
    torch = torch_mod
    rng = np.random.default_rng(11)
    B, hq, wq = 2, 13, 22
    ts = [0.25, 0.5, 0.75] if mode != "nine_offsets" else [0.1 * k for k in range(1, 10)]
    depth = mode in ("shared_depth", "nine_offsets")
    fq = gpu(torch, make_flow_q(rng, "smooth", B, hq, wq))
    d = gpu(torch, rng.uniform(0.1, 1.0, (B, 1, 4 * hq, 4 * wq)).astype(f32)) if depth else None
    gs = [gpu(torch, rng.standard_normal((B, 2, 4 * hq, 4 * wq)).astype(f32)) for _ in ts]
    with torch.no_grad():
        plain = fused.FlowProject_from_quarter(fq, MUL0, ts, d, fillhole=False)
    assert all(o.grad_fn is None and not o.requires_grad for o in plain)
    idle = fused.FlowProject_from_quarter(fq, MUL0, ts, d, fillhole=False)          # grad mode on, nothing requires grad
    assert all(o.grad_fn is None for o in idle) and all(torch.equal(a, b) for a, b in zip(plain, idle))

    q = fq.clone().requires_grad_()
    dd = d.clone().requires_grad_() if depth else None
    outs = fused.FlowProject_from_quarter(q, MUL0, ts, dd, fillhole=False)
    assert all(o.grad_fn is not None for o in outs) and all(torch.equal(a, b.detach()) for a, b in zip(plain, outs))
    used = [i for i in range(len(ts)) if not (mode == "unused_output" and i == 1)]
    sum((outs[i] * gs[i]).sum() for i in used).backward()

    # the same through the C ABI: count / out of the forward recomputed with the same calls
    q_parts, d_parts = [], []
    for k in range(0, len(used), 8):
        idx = used[k:k + 8]
        counts, fo = [], []
        for i in idx:
            count, out = torch.empty((B, 1, 4 * hq, 4 * wq), device="cuda:0"), torch.empty((B, 2, 4 * hq, 4 * wq), device="cuda:0")
            if depth:
                assert cabi.depthflowprojection_forward_up4(fq, d, count, out, MUL0, ts[i], 0) == 0
            else:
                assert cabi.flowprojection_forward_up4(fq, count, out, MUL0, ts[i], 0) == 0
            counts.append(count), fo.append(out)
        gq = torch.full_like(fq, float("nan"))
        gds = [torch.full_like(d, float("nan")) for _ in idx] if depth else None
        assert cabi.flowprojection_backward_up4(fq, counts, [gs[i] for i in idx], MUL0, [ts[i] for i in idx], gq,
                                                d, fo if depth else None, gds) == 0
        q_parts.append(gq)
        d_parts += gds or []
    want_q = q_parts[0]
    for p in q_parts[1:]:
        want_q = want_q + p
    assert torch.equal(q.grad, want_q)
    if depth:
        want_d = d_parts[0]
        for p in d_parts[1:]:
            want_d = want_d + p
        assert torch.equal(dd.grad, want_d)
    if mode == "nine_offsets":
        assert len(q_parts) == 2

    # fillhole keeps its meaning in the forward and plays no part in the backward
    q2 = fq.clone().requires_grad_()
    filled = fused.FlowProject_from_quarter(q2, MUL0, ts, d, fillhole=True)
    with torch.no_grad():
        assert all(torch.equal(a.detach(), b) for a, b in zip(filled, fused.FlowProject_from_quarter(fq, MUL0, ts, d, fillhole=True)))
    sum((filled[i] * gs[i]).sum() for i in used).backward()
    assert torch.equal(q2.grad, q.grad)


@pytest.mark.parametrize("mode", ["all", "unused_output", "nine_offsets"])
def test_upsample_autograd_equals_the_c_abi(torch_mod, cabi, fused, mode):  # noqa: F811
    torch = torch_mod
    rng = np.random.default_rng(12)
    B, C, hq, wq = 2, 2, 9, 31
    ts = [0.25, 0.5, 0.75] if mode != "nine_offsets" else [0.1 * k for k in range(1, 10)]
    fq = gpu(torch, rng.standard_normal((B, C, hq, wq)).astype(f32))
    gs = [gpu(torch, rng.standard_normal((B, C, 4 * hq, 4 * wq)).astype(f32)) for _ in ts]
    with torch.no_grad():
        plain = fused.forward_flownets_upsample(fq, MUL0, ts)
    idle = fused.forward_flownets_upsample(fq, MUL0, ts)
    assert all(o.grad_fn is None for o in plain + idle) and all(torch.equal(a, b) for a, b in zip(plain, idle))
    q = fq.clone().requires_grad_()
    outs = fused.forward_flownets_upsample(q, MUL0, ts)
    assert all(o.grad_fn is not None for o in outs) and all(torch.equal(a, b.detach()) for a, b in zip(plain, outs))
    used = [i for i in range(len(ts)) if not (mode == "unused_output" and i == 1)]
    sum((outs[i] * gs[i]).sum() for i in used).backward()
    parts = []
    for k in range(0, len(used), 8):
        idx = used[k:k + 8]
        gq = torch.full_like(fq, float("nan"))
        assert cabi.flow_upsample4_backward([gs[i] for i in idx], MUL0, [ts[i] for i in idx], gq) == 0
        parts.append(gq)
    want = parts[0]
    for p in parts[1:]:
        want = want + p
    assert torch.equal(q.grad, want)
    # and the float64 gradient of torch's own upsample, to the bound of test 2
    _, ref64, S, nadd = M.up4_backward([cpu(gs[i]) for i in used], MUL0, [ts[i] for i in used])
    assert np.all(np.abs(cpu(q.grad).astype(np.float64) - ref64) <= (nadd + 12 + len(parts)) * 2.0 ** -24 * S)


# ------------------------------------------------------------------ 5. the chain trains

def _train(torch, fused, from_quarter, steps=30):
    torch.manual_seed(0)
    B, H, W = 2, 32, 48
    g = torch.Generator().manual_seed(3)
    base = torch.rand((B, 3, H, W + 4), generator=g)
    frame0, frame2 = base[..., :W].cuda(), base[..., 4:].cuda()       # a pair translated by four pixels
    target = base[..., 2:W + 2].cuda()
    # convolutions written as unfold + matmul: a library convolution's backward may pick its algorithm per call and
    # sum with atomics, which would make two identical loops drift apart for reasons outside the chain under test
    params = []
    for cout in (4, 32):
        wgt = (torch.randn((cout, 6 * 9), generator=g) * 0.01).cuda().requires_grad_()
        bias = torch.zeros((cout, 1), device="cuda", requires_grad=True)
        params += [wgt, bias]

    def conv(x, wgt, bias):
        return (wgt @ torch.nn.functional.unfold(x, 3, padding=1) + bias).view(x.size(0), -1, x.size(2), x.size(3))

    opt = torch.optim.SGD(params, lr=0.5)
    losses = []
    x = torch.cat([frame0, frame2], 1)
    xq = torch.nn.functional.avg_pool2d(x, 4)
    div_flow, t = 20.0, 0.5
    for _ in range(steps):
        opt.zero_grad()
        fq = conv(xq, *params[:2]) * 0.1                              # the flow network: quarter resolution, both directions
        kf = torch.softmax(conv(x, *params[2:]).view(B, 2, 16, H, W), 2)
        q0, q2 = fq[:, :2].contiguous(), fq[:, 2:].contiguous()
        k0, k2 = kf[:, 0].contiguous(), kf[:, 1].contiguous()
        if from_quarter:
            p0 = fused.FlowProject_from_quarter(q0, div_flow, [t], fillhole=False)[0]
            p2 = fused.FlowProject_from_quarter(q2, div_flow, [1.0 - t], fillhole=False)[0]
        else:
            p0 = fused.FlowProject(fused.forward_flownets_upsample(q0, div_flow, [t]), None, fillhole=False)[0]
            p2 = fused.FlowProject(fused.forward_flownets_upsample(q2, div_flow, [1.0 - t]), None, fillhole=False)[0]
        blend, o0, o2 = fused.FilterInterpolate(frame0, frame2, [p0, p2], [k0, k2], 16, t)
        loss = (blend - target).abs().mean()
        loss.backward()
        assert params[0].grad is not None and bool(params[0].grad.abs().sum() > 0)   # (the loss reaches the flow network)
        opt.step()
        losses.append(loss.item())
    return losses


def test_training_through_the_quarter_resolution_flow(torch_mod, fused):  # noqa: F811
    torch = torch_mod
    a = _train(torch, fused, True)
    assert a == _train(torch, fused, True)                  # (reproducible run to run)
    b = _train(torch, fused, False)
    print("losses: first %.6f last %.6f" % (a[0], a[-1]))
    assert a == b, (a[:5], b[:5])
    assert a[-1] < a[0]


# ------------------------------------------------------------------ 6. the target shapes

@pytest.mark.parametrize("B,hq,wq,n,depth", [(1, 288, 496, 3, True), (3, 64, 112, 1, False), (1, 540, 960, 1, False)],
                         ids=["1080p", "vimeo", "4k"])
def test_target_shapes_run(torch_mod, cabi, B, hq, wq, n, depth):  # noqa: F811
    torch = torch_mod
    c = Case(torch, cabi, B, hq, wq, n, "smooth", 31, depth=depth, shared_depth=True)
    gq, gds = c.fused_call(torch, cabi)
    ref_q, _, ref_gd = c.composition(torch, cabi)
    assert not torch.isnan(gq).any() and torch.equal(gq, ref_q)
    if depth:
        assert all(torch.equal(a, b) for a, b in zip(gds, ref_gd))
