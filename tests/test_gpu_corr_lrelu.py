"""`-m gpu`: the correlation with PWC-Net's LeakyReLU fused in, bit for bit against tests/corr_lrelu.py (torch's
leaky_relu of the oracle's forward; the oracle's backward fed torch.where(y > 0, g, g * slope)).  NaN at the same places,
every other element the same bits: no tolerance anywhere.

  1. forward, every float kernel (the cases of tests/corr_edges.py, normal and planted values), single and paired;
  2. slopes 0.2 and 1.0 (slope 1: the unactivated entry's bits);
  3. a destination inside a concatenation buffer, at batch strides that keep and that break 8- and 16-byte alignment;
  4. backward: one and several channels per group with ragged tiles, the generic configuration; the single entry, the pair
     entry with four, two and (one item's gradient None) two gradients; planted gradients; the narrow() view of a wider
     gradient;
  5. autograd through torch.cat against F.leaky_relu of the unfused functions, with no dense copy of cat's gradient;
  6. the unfused entries keep their bits after the fused ones ran.
"""
import numpy as np
import pytest

from tests import corr_edges as ce
from tests import corr_lrelu as cl
from tests.test_gpu_corr_edges import assert_same, dev
from tests.test_gpu_parity import cpu, gpu, f32, torch_mod, cabi  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
SLOPE = cl.SLOPE


def _bits(t):
    return cpu(t).view(np.uint32)


# ------------------------------------------------------------------ 1. forward: every kernel, single and paired

@pytest.mark.parametrize("planted", [False, True], ids=["normal", "planted"])
@pytest.mark.parametrize("name", cl.FORWARD_CASES)
def test_forward_every_kernel_single_and_paired(torch_mod, cabi, name, planted):  # noqa: F811
    torch = torch_mod
    shape, cfg, dense, _ = ce.F32_CASES[name]
    kw = dict(k=cfg[1], md=cfg[2], s1=cfg[3], s2=cfg[4])
    _, oh, ow = ce.out_dims(shape[2], shape[3], *cfg)
    for nitems in (1, 2):
        assert cl.selected_kernel_out(*shape, cfg[0], nitems=nitems, out_bits=81 * oh * ow * 4, **kw) == dense
    f1, f2, _ = cl.forward_inputs(name, planted)
    want, want_swapped = cl.forward_expected(name, planted), cl.forward_expected(name, planted, swapped=True)
    if not planted and name != "flat_pad8":                # (flat_pad8: 73 % padding zeros -- tests/test_corr_lrelu_host.py)
        assert (want < 0).mean() >= 0.25 and (want > 0).mean() >= 0.25
    a1, a2 = dev(torch, f1), dev(torch, f2)
    single = cabi.correlation_lrelu_forward(a1, a2, *cfg, SLOPE)
    assert_same(single, want, (dense, "single"))
    pa, pb = cabi.correlation_lrelu_forward_pair(a1, a2, a2, a1, *cfg, SLOPE)      # two different input pairs
    assert_same(pa, want, (dense, "pair, first item"))
    assert_same(pb, want_swapped, (dense, "pair, second item"))
    if not planted:
        got = cpu(single)
        zero = got == 0
        assert zero.any() and not np.signbit(got[zero]).any()


# ------------------------------------------------------------------ 2. slopes

def test_other_slopes(torch_mod, cabi):  # noqa: F811
    torch = torch_mod
    name = "rows2"
    cfg = ce.F32_CASES[name][1]
    for planted in (False, True):
        f1, f2, _ = cl.forward_inputs(name, planted)
        a1, a2 = dev(torch, f1), dev(torch, f2)
        assert_same(cabi.correlation_lrelu_forward(a1, a2, *cfg, 0.2), cl.forward_expected(name, planted, 0.2), "slope 0.2")
        # slope 1: v * 1 is v, -0 and NaN included -- the unactivated entry's bits
        plain = cabi.correlation_forward(a1, a2, *cfg)
        one = cabi.correlation_lrelu_forward(a1, a2, *cfg, 1.0)
        assert_same(one, cpu(plain), "slope 1.0")
        pa, pb = cabi.correlation_lrelu_forward_pair(a1, a2, a2, a1, *cfg, 1.0)
        qa, qb = cabi.correlation_forward_pair(a1, a2, a2, a1, *cfg)
        assert_same(pa, cpu(qa), "slope 1.0, pair")
        assert_same(pb, cpu(qb), "slope 1.0, pair")
    assert not np.array_equal(cl.forward_expected(name, False, 0.2), cl.forward_expected(name, False))


# ------------------------------------------------------------------ 3. a destination inside a concatenation buffer

SENTINEL = -7.25


def _cat_buffer(torch, B, oh, ow, extra):
    """(the (B, 90, oh, ow) view, its whole storage): images 90 * oh * ow + extra elements apart, filled with the sentinel"""
    n = cl.CAT * oh * ow
    store = torch.full((B, n + extra), SENTINEL, device="cuda:0")
    assert store.data_ptr() % 16 == 0
    return store[:, :n].view(B, cl.CAT, oh, ow), store


@pytest.mark.parametrize("name,extra", [("rows2", 0), ("rows2", 1), ("rows2", 2), ("quad", 0), ("quad", 1), ("quad", 2),
                                        ("flat", 0), ("flat", 1)])
def test_strided_destination(torch_mod, cabi, name, extra):  # noqa: F811
    torch = torch_mod
    shape, cfg = ce.F32_CASES[name][:2]
    B = shape[0]
    _, oh, ow = ce.out_dims(shape[2], shape[3], *cfg)
    f1, f2, _ = cl.forward_inputs(name, False)
    a1, a2 = dev(torch, f1), dev(torch, f2)
    dense = cabi.correlation_lrelu_forward(a1, a2, *cfg, SLOPE)
    assert_same(dense, cl.forward_expected(name, False), name)
    buf, store = _cat_buffer(torch, B, oh, ow, extra)
    dst = buf[:, 3:84]
    bits = dst.data_ptr() | (dst.stride(0) * 4)
    assert bits % 16 == (0, 4, 8)[extra]                    # keeps 16-byte alignment; breaks 8 and 16; breaks 16 only
    got = cabi.correlation_lrelu_forward(a1, a2, *cfg, SLOPE, out=dst)
    assert got is dst
    assert np.array_equal(_bits(dst), _bits(dense)), (name, extra, cl.selected_kernel_out(*shape, cfg[0], out_bits=bits % 16))
    rest = cpu(store).copy()
    rest.reshape(B, -1)[:, 3 * oh * ow:84 * oh * ow] = SENTINEL
    assert (rest == SENTINEL).all(), "an element outside the 81 channels was written"
    # the pair: both destinations in ONE buffer (channels 3..83 and a second buffer's 9..89), one stride each
    buf2, store2 = _cat_buffer(torch, B, oh, ow, 0)
    pa, pb = cabi.correlation_lrelu_forward_pair(a1, a2, a2, a1, *cfg, SLOPE, out=(dst, buf2[:, 9:]))
    assert np.array_equal(_bits(pa), _bits(dense))
    assert_same(pb, cl.forward_expected(name, False, swapped=True), (name, "pair, second destination"))
    assert (cpu(buf2[:, :9]) == SENTINEL).all() and (cpu(buf[:, :3]) == SENTINEL).all() and (cpu(buf[:, 84:]) == SENTINEL).all()


# ------------------------------------------------------------------ 4. backward

def _dev_items(torch, name, planted):
    host = cl.backward_inputs(name, planted)
    return [gpu(torch, x) for x in host[:8]], host[8]


@pytest.mark.parametrize("planted", [False, True], ids=["normal", "planted"])
@pytest.mark.parametrize("name", sorted(cl.BACKWARD_CASES))
def test_backward_single_and_pair(torch_mod, cabi, name, planted):  # noqa: F811
    torch = torch_mod
    (a1, a2, ya, ga, b1, b2, yb, gb), cfg = _dev_items(torch, name, planted)
    want = cl.backward_expected(name, planted)
    if planted:
        assert all(np.isnan(w).any() and np.isfinite(w).any() for w in want)
    single = cabi.correlation_lrelu_backward(a1, a2, ya, ga, *cfg, SLOPE) + cabi.correlation_lrelu_backward(b1, b2, yb, gb, *cfg, SLOPE)
    for i, (s, w) in enumerate(zip(single, want)):
        assert_same(s, w, (name, "single", i))
    # all four gradients from one call
    four = cabi.correlation_lrelu_backward_pair(a1, a2, ya, ga, b1, b2, yb, gb, *cfg, SLOPE)
    for i in range(4):
        assert_same(four[i], want[i], (name, "pair of four", i))
        assert_same(four[i], cpu(single[i]), (name, "pair of four against single", i))
    # only the two second gradients
    two = cabi.correlation_lrelu_backward_pair(a1, a2, ya, ga, b1, b2, yb, gb, *cfg, SLOPE, want=(False, True, False, True))
    assert two[0] is None and two[2] is None
    for i in (1, 3):
        assert_same(two[i], want[i], (name, "second gradients", i))
    # one item's gradient None
    half = cabi.correlation_lrelu_backward_pair(a1, a2, ya, None, b1, b2, yb, gb, *cfg, SLOPE)
    assert half[0] is None and half[1] is None
    for i in (2, 3):
        assert_same(half[i], want[i], (name, "item a unused", i))
    assert cabi.correlation_lrelu_backward_pair(a1, a2, ya, None, b1, b2, None, None, *cfg, SLOPE) == (None,) * 4


@pytest.mark.parametrize("name", sorted(cl.BACKWARD_CASES))
def test_backward_reads_a_narrowed_gradient_where_it_lies(torch_mod, cabi, name, monkeypatch):  # noqa: F811
    torch = torch_mod
    (a1, a2, ya, ga, b1, b2, yb, gb), cfg = _dev_items(torch, name, True)
    oc, wide = ga.size(1), ga.size(1) + 9                   # (81 of 90 channels; the generic configuration: 25 of 34)
    wide_a = torch.full((ga.size(0), wide) + tuple(ga.shape[2:]), float("nan"), device="cuda:0")
    wide_b = torch.full_like(wide_a, float("nan"))
    wide_a[:, :oc] = ga
    wide_b[:, 9:] = gb
    va, vb = wide_a.narrow(1, 0, oc), wide_b.narrow(1, 9, oc)
    assert not va.is_contiguous() and not vb.is_contiguous()
    # y too may live inside a buffer: the forward's strided destination
    ybuf = torch.zeros_like(wide_a)
    ybuf[:, 5:5 + oc] = yb
    yv = ybuf[:, 5:5 + oc]
    seen = []
    planes = cabi._planes
    monkeypatch.setattr(cabi, "_planes", lambda t: (seen.append((t, planes(t))), seen[-1][1])[1])
    dense = cabi.correlation_lrelu_backward(a1, a2, ya, ga, *cfg, SLOPE) + cabi.correlation_lrelu_backward(b1, b2, yb, gb, *cfg, SLOPE)
    del seen[:]
    got = cabi.correlation_lrelu_backward(a1, a2, ya, va, *cfg, SLOPE) + cabi.correlation_lrelu_backward(b1, b2, yv, vb, *cfg, SLOPE)
    pair = cabi.correlation_lrelu_backward_pair(a1, a2, ya, va, b1, b2, yv, vb, *cfg, SLOPE)
    assert len(seen) == 8 and all(out[0] is t for t, out in seen), "a strided tensor was copied"
    assert {out[1] for t, out in seen} == {oc * ga.size(2) * ga.size(3), wide * ga.size(2) * ga.size(3)}
    for i in range(4):
        assert np.array_equal(_bits(got[i]), _bits(dense[i])), (name, "single, strided", i)
        assert np.array_equal(_bits(pair[i]), _bits(dense[i])), (name, "pair, strided", i)
        assert_same(pair[i], cl.backward_expected(name, True)[i], (name, "pair, strided, against the helper", i))


# ------------------------------------------------------------------ 5. autograd through torch.cat

def _cat_loss(torch, corrs, tails, weights):
    return sum((torch.cat((c, t), 1) * w).sum() for c, t, w in zip(corrs, tails, weights))


def test_autograd_pair_equals_the_composition_and_copies_no_gradient(torch_mod, cabi, monkeypatch):  # noqa: F811
    torch = torch_mod
    F = torch.nn.functional
    from vfidkr_amd import fused
    host = cl.backward_inputs("one_channel_per_group")
    B, C, H, W = host[0].shape
    rng = np.random.default_rng(77)
    tails = [gpu(torch, rng.standard_normal((B, cl.CAT - 81, H, W)).astype(f32)) for _ in range(2)]
    weights = [gpu(torch, rng.standard_normal((B, cl.CAT, H, W)).astype(f32)) for _ in range(2)]

    def leaves(pattern=(True,) * 4):
        return [gpu(torch, host[i]).requires_grad_(r) for i, r in zip((0, 1, 4, 5), pattern)]

    seen = []
    planes = cabi._planes
    monkeypatch.setattr(cabi, "_planes", lambda t: (seen.append((t, planes(t))), seen[-1][1])[1])

    def fused_grads(pattern=(True,) * 4, use_b=True):
        xs = leaves(pattern)
        ya, yb = fused.corr_pair_lrelu(*xs, negative_slope=SLOPE)
        assert ya.grad_fn is not None and yb.grad_fn is ya.grad_fn
        loss = _cat_loss(torch, (ya, yb) if use_b else (ya,), tails, weights)
        return (ya, yb), torch.autograd.grad(loss, [x for x in xs if x.requires_grad], allow_unused=True)

    def composed_grads(pattern=(True,) * 4, use_b=True):
        xs = leaves(pattern)
        ya, yb = (F.leaky_relu(c, SLOPE) for c in fused.corr_pair(*xs))
        loss = _cat_loss(torch, (ya, yb) if use_b else (ya,), tails, weights)
        return (ya, yb), torch.autograd.grad(loss, [x for x in xs if x.requires_grad], allow_unused=True)

    (ya, yb), got = fused_grads()
    cat_stride = cl.CAT * H * W
    grads_seen = [(t, out) for t, out in seen if t.stride(0) == cat_stride]
    assert len(grads_seen) == 2 and all(out[0] is t and out[1] == cat_stride for t, out in grads_seen), "cat's gradient was copied"
    (za, zb), want = composed_grads()
    assert np.array_equal(_bits(ya), _bits(za)) and np.array_equal(_bits(yb), _bits(zb))
    assert_same(cpu(ya), cl.expected_forward(host[0], host[1], ce.PWC), "the activated output")
    assert len(got) == 4 and all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))
    # two backward runs: the same bits
    _, again = fused_grads()
    assert all(np.array_equal(_bits(g), _bits(a)) for g, a in zip(got, again))
    # the helper, on the gradient cat's backward hands down
    ref = cl.expected_backward(host[0], host[1], cpu(ya), cpu(weights[0])[:, :81], ce.PWC) + \
        cl.expected_backward(host[4], host[5], cpu(yb), cpu(weights[1])[:, :81], ce.PWC)
    assert all(np.array_equal(cpu(g), r) for g, r in zip(got, ref))
    # only the second inputs require grad; an unused cost volume
    _, got = fused_grads((False, True, False, True))
    _, want = composed_grads((False, True, False, True))
    assert len(got) == 2 and all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))
    _, got = fused_grads(use_b=False)
    _, want = composed_grads(use_b=False)
    assert got[2] is None and got[3] is None and want[2] is None
    assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got[:2], want[:2]))
    # grad mode off, or nothing requires grad: no grad_fn, the same bits, and out= is accepted
    with torch.no_grad():
        outs = fused.corr_pair_lrelu(*leaves(), negative_slope=SLOPE)
    assert all(o.grad_fn is None and not o.requires_grad for o in outs) and np.array_equal(_bits(outs[0]), _bits(ya))
    outs = fused.corr_pair_lrelu(*leaves((False,) * 4))
    assert all(o.grad_fn is None for o in outs) and np.array_equal(_bits(outs[1]), _bits(yb))
    buf = torch.zeros(B, cl.CAT, H, W, device="cuda:0")
    outs = fused.corr_pair_lrelu(*leaves((False,) * 4), out=(buf[:, :81], None))
    assert outs[0].data_ptr() == buf.data_ptr() and np.array_equal(_bits(buf[:, :81]), _bits(ya))
    single = fused.corr_lrelu(*leaves((False,) * 4)[:2], out=buf[:, 9:])
    assert np.array_equal(_bits(single), _bits(ya)) and single.grad_fn is None


@pytest.mark.parametrize("align_corners", [True, False])
def test_autograd_warp_corr_lrelu_equals_the_composition(torch_mod, cabi, align_corners):  # noqa: F811
    torch = torch_mod
    F = torch.nn.functional
    from vfidkr_amd import fused
    host = cl.backward_inputs("one_channel_per_group")
    B, C, H, W = host[0].shape
    rng = np.random.default_rng(78)
    flo_h = (rng.standard_normal((B, 2, H, W)) * 0.7).astype(f32)
    tail = gpu(torch, rng.standard_normal((B, cl.CAT - 81, H, W)).astype(f32))
    weight = gpu(torch, rng.standard_normal((B, cl.CAT, H, W)).astype(f32))

    def run(fn):
        c1, c2, flo = (gpu(torch, x).requires_grad_(True) for x in (host[0], host[1], flo_h))
        y = fn(c1, c2, flo)
        assert y.grad_fn is not None
        return y, torch.autograd.grad((torch.cat((y, tail), 1) * weight).sum(), (c1, c2, flo))

    y, got = run(lambda c1, c2, flo: fused.warp_corr_lrelu(c1, c2, flo, align_corners, SLOPE))
    z, want = run(lambda c1, c2, flo: F.leaky_relu(fused.warp_corr(c1, c2, flo, align_corners), SLOPE))
    assert np.array_equal(_bits(y), _bits(z))
    assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))
    _, again = run(lambda c1, c2, flo: fused.warp_corr_lrelu(c1, c2, flo, align_corners, SLOPE))
    assert all(np.array_equal(_bits(g), _bits(a)) for g, a in zip(got, again))
    c1, c2, flo = (gpu(torch, x).requires_grad_(True) for x in (host[0], host[1], flo_h))
    with torch.no_grad():
        plain = fused.warp_corr_lrelu(c1, c2, flo, align_corners, SLOPE)
    assert plain.grad_fn is None and np.array_equal(_bits(plain), _bits(y))
    one = fused.corr_lrelu(c1.detach().requires_grad_(True), c2.detach())
    assert one.grad_fn is not None and fused.corr_lrelu(c1.detach(), c2.detach()).grad_fn is None


# ------------------------------------------------------------------ 6. the unfused entries are what they were

def test_existing_entries_keep_their_bits_after_the_fused_ones_ran(torch_mod, cabi):  # noqa: F811
    torch = torch_mod
    from vfidkr_amd import fused
    f1, f2, cfg = cl.forward_inputs("rows2", False)
    a1, a2 = dev(torch, f1), dev(torch, f2)
    before = [cpu(t) for t in fused.corr_pair(a1, a2, a2, a1)]
    g = torch.ones_like(fused.corr_pair(a1, a2, a2, a1)[0])
    before_grads = [cpu(t) for t in cabi.correlation_backward_pair(a1, a2, g, a2, a1, g, *cfg)]
    ya, yb = fused.corr_pair_lrelu(a1, a2, a2, a1)
    cabi.correlation_lrelu_backward_pair(a1, a2, ya, g, a2, a1, yb, g, *cfg, SLOPE)
    after = [cpu(t) for t in fused.corr_pair(a1, a2, a2, a1)]
    after_grads = [cpu(t) for t in cabi.correlation_backward_pair(a1, a2, g, a2, a1, g, *cfg)]
    assert all(np.array_equal(b.view(np.uint32), a.view(np.uint32)) for b, a in zip(before + before_grads, after + after_grads))
    assert np.array_equal(after[0], cl._oracle().correlation_fwd(f1, f2, *cfg, order=1, fmad=1))
