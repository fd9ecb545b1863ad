"""GPU: the paired correlation on bfloat16 tensors (vfi_correlation_[lrelu_]forward_pair_bf16 / _backward_pair_bf16, the
bfloat16 side of cabi.correlation_*_pair, fused._CorrPair / corr_pair_lrelu on bfloat16 leaves).

Every comparison is on raw bits (view(torch.int16)) against the single bfloat16 entries on each item -- NaN positions
included, no tolerance anywhere: the pair entries run the single entries' kernels' code, chosen as the single entry
chooses it, and the backward's channel groups only partition the channels."""
import ctypes
import itertools

import pytest

from tests import corr_bf16 as cb
from tests import corr_lrelu as cl
from tests.test_gpu_corr_bf16 import torch_mod, cabi  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

PWC = cb.PWC
OTHER = (3, 3, 4, 1, 2)                     # pad, kernel 3, max displacement 4, stride1 1, stride2 2: the generic kernels
PATTERN = 0x5A5A
SLOPE = 0.1


def rnd(torch, gen, *shape):
    """standard-normal bfloat16 values with a full significand (integer-free: the two forward kernels round differently)"""
    return torch.randn(*shape, generator=gen).to(torch.bfloat16).cuda()


def same(torch, a, b):
    return a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and tuple(a.shape) == tuple(b.shape) and \
        torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def four(torch, gen, shape, swapped=False):
    a1, a2 = rnd(torch, gen, *shape), rnd(torch, gen, *shape)
    return (a1, a2, a2, a1) if swapped else (a1, a2, rnd(torch, gen, *shape), rnd(torch, gen, *shape))


def gen_of(torch, seed):
    return torch.Generator(device="cpu").manual_seed(seed)


# ------------------------------------------------------------------ forward

@pytest.mark.parametrize("batch", [1, 2])
def test_forward_mfma_class(torch_mod, cabi, batch):
    """33 tiles of 64 x 2 per image: at or above the threshold for one item, so both items take the matrix cores.  C = 33 leaves
    a K tail of one channel, and 130 = 2 * 64 + 2 an edge tile in x that holds a single pixel pair.  batch 1: item b is item
    a swapped (the same tensor objects); batch 2: four different tensors."""
    torch = torch_mod
    shape = (batch, 33, 22, 130)
    assert cb.selected_kernel(*shape) == "mfma" and cb.selected_kernel(1, 33, 22, 130) == "mfma"
    a1, a2, b1, b2 = four(torch, gen_of(torch, 3 + batch), shape, swapped=(batch == 1))
    outa, outb = cabi.correlation_forward_pair(a1, a2, b1, b2, *PWC)
    assert same(torch, outa, cabi.correlation_forward(a1, a2, *PWC)) and same(torch, outb, cabi.correlation_forward(b1, b2, *PWC))
    assert same(torch, outa, cabi.correlation_forward_bf16_kernel("mfma", a1, a2, *PWC))
    assert outa.float().abs().max() > 0 and not same(torch, outa, outb)


def test_forward_kernel_is_chosen_per_item(torch_mod, cabi):
    """18 tiles per item (generic), 36 for the pair (a pair-count choice would take the MFMA kernel, whose bits differ)"""
    torch = torch_mod
    shape = (1, 12, 12, 130)
    assert cb.selected_kernel(*shape) == "generic" and cb.selected_kernel(2, *shape[1:]) == "mfma"
    gen = gen_of(torch, 7)
    a1, a2, b1, b2 = four(torch, gen, shape)
    # Standard-normal channels alone leave the two kernels equal here: twelve exact products summed in float32 in another
    # order differ by about 2^-23 of the terms, and that crosses a bfloat16 rounding boundary (2^-9 of the result) once in
    # some 10^5 outputs.  So the second half of the channels nearly cancels the first: the first map's channel c + 6 is
    # minus its channel c times (1 + 2^-8 n), n standard normal, rounded to bfloat16, and the second map's channel c + 6 is
    # its channel c.  The mean is then about 2^-8 of the terms and the float32 error about 2^-15 of it: on the CPU
    # (tests/corr_bf16.py simulate_fp32) two addition orders of these inputs differ in some 200 to 300 of the 126360 outputs.
    for first, second in ((a1, a2), (b1, b2)):
        noise = torch.randn(1, 6, 12, 130, generator=gen).cuda()
        first[:, 6:] = (-first[:, :6].float() * (1.0 + noise / 256)).to(torch.bfloat16)
        second[:, 6:] = second[:, :6]
    gen_a, gen_b = (cabi.correlation_forward_bf16_kernel("generic", x, y, *PWC) for x, y in ((a1, a2), (b1, b2)))
    mfma_a, mfma_b = (cabi.correlation_forward_bf16_kernel("mfma", x, y, *PWC) for x, y in ((a1, a2), (b1, b2)))
    assert not same(torch, gen_a, mfma_a) and not same(torch, gen_b, mfma_b)      # the two kernels do differ on this input
    outa, outb = cabi.correlation_forward_pair(a1, a2, b1, b2, *PWC)
    assert same(torch, outa, gen_a) and same(torch, outb, gen_b)
    ya, yb = cabi.correlation_lrelu_forward_pair(a1, a2, b1, b2, *PWC, 1.0)
    assert same(torch, ya, gen_a) and same(torch, yb, gen_b)


def test_forward_other_configuration(torch_mod, cabi):
    torch = torch_mod
    a1, a2, b1, b2 = four(torch, gen_of(torch, 11), (2, 5, 9, 14))
    outa, outb = cabi.correlation_forward_pair(a1, a2, b1, b2, *OTHER)
    assert same(torch, outa, cabi.correlation_forward(a1, a2, *OTHER)) and same(torch, outb, cabi.correlation_forward(b1, b2, *OTHER))
    ya, yb = cabi.correlation_lrelu_forward_pair(a1, a2, b1, b2, *OTHER, SLOPE)
    assert same(torch, ya, cabi.correlation_lrelu_forward(a1, a2, *OTHER, SLOPE))
    assert same(torch, yb, cabi.correlation_lrelu_forward(b1, b2, *OTHER, SLOPE))
    assert outa.float().abs().max() > 0


def _pattern(torch, n):
    return torch.full((n,), PATTERN, dtype=torch.int16, device="cuda").view(torch.bfloat16)


@pytest.mark.parametrize("shape", [(2, 5, 7, 70), (2, 33, 22, 70)])       # the generic kernel (16 tiles per item); the MFMA kernel (44)
def test_lrelu_forward_into_channel_slices(torch_mod, cabi, shape):
    """Item a into buf[:, 3:84] of a (B, 90, H, W) buffer, item b into 81 planes of a buffer whose images lie an ODD number of
    elements apart (every other image on a 2-byte boundary); both buffers pattern-filled, and whole buffers are compared."""
    torch = torch_mod
    B, C, H, W = shape
    assert cb.selected_kernel(*shape) == ("generic" if C == 5 else "mfma")
    a1, a2, b1, b2 = four(torch, gen_of(torch, 13 + C), shape)
    stride = 90 * H * W + 1
    assert stride % 2 == 1

    def buffers():
        buf_a = _pattern(torch, B * 90 * H * W).view(B, 90, H, W)
        flat_b = _pattern(torch, B * stride + 7)
        return buf_a, buf_a[:, 3:84], flat_b, flat_b.as_strided((B, 81, H, W), (stride, H * W, W, 1), 5 * H * W + 3)

    for slope in (SLOPE, 1.0):
        want_a, want_b = cabi.correlation_lrelu_forward(a1, a2, *PWC, slope), cabi.correlation_lrelu_forward(b1, b2, *PWC, slope)
        assert (want_a.float() < 0).any() and (want_a.float() > 0).any()
        buf_a, out_a, flat_b, out_b = buffers()
        exp_a, exp_out_a, exp_b, exp_out_b = buffers()
        exp_out_a.copy_(want_a)
        exp_out_b.copy_(want_b)
        got = cabi.correlation_lrelu_forward_pair(a1, a2, b1, b2, *PWC, slope, out=(out_a, out_b))
        assert got[0] is out_a and got[1] is out_b
        assert torch.equal(buf_a.view(torch.int16), exp_a.view(torch.int16)), "item a, or an element outside its slice"
        assert torch.equal(flat_b.view(torch.int16), exp_b.view(torch.int16)), "item b, or an element outside its slice"
        # one destination is None: a fresh dense tensor for that item, the other buffer as before
        buf_a, out_a, flat_b, out_b = buffers()
        ya, yb = cabi.correlation_lrelu_forward_pair(a1, a2, b1, b2, *PWC, slope, out=(None, out_b))
        assert yb is out_b and same(torch, ya, want_a) and ya.is_contiguous()
        assert torch.equal(flat_b.view(torch.int16), exp_b.view(torch.int16)) and (buf_a.view(torch.int16) == PATTERN).all()
        ya, yb = cabi.correlation_lrelu_forward_pair(a1, a2, b1, b2, *PWC, slope, out=(out_a, None))
        assert ya is out_a and same(torch, yb, want_b) and torch.equal(buf_a.view(torch.int16), exp_a.view(torch.int16))
        if slope == 1.0:                                    # the activation with slope 1 is the identity: the plain pair's bits
            pa, pb = cabi.correlation_forward_pair(a1, a2, b1, b2, *PWC)
            assert same(torch, pa, want_a) and same(torch, pb, want_b)


# ------------------------------------------------------------------ backward

def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def test_backward_every_subset_through_the_c_abi(torch_mod, cabi):
    """The 15 non-empty subsets of the four gradients and the empty one on (2, 5, 7, 70): two tiles each way, both ragged.
    Item b is item a swapped (the same tensor objects).  Unrequested outputs keep their sentinel."""
    torch = torch_mod
    B, C, H, W = shape = (2, 5, 7, 70)
    assert W % 64 and H % 4 and cl.tiles_of(shape) == 4
    gen = gen_of(torch, 5)
    a1, a2, b1, b2 = four(torch, gen, shape, swapped=True)
    ga, gb = rnd(torch, gen, B, 81, H, W), rnd(torch, gen, B, 81, H, W)
    single = cabi.correlation_backward(a1, a2, ga, *PWC) + cabi.correlation_backward(b1, b2, gb, *PWC)
    assert all(s.float().abs().max() > 0 for s in single)
    fn = cabi.lib().vfi_correlation_backward_pair_bf16
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    subsets = [s for n in range(0, 5) for s in itertools.combinations(range(4), n)]
    assert len(subsets) == 16
    for subset in subsets:
        outs = [_pattern(torch, a1.numel()).view(shape) for _ in range(4)]
        o = [outs[i] if i in subset else None for i in range(4)]
        # an item nothing is asked of passes NULL inputs and a NULL gradoutput
        ia = (a1, a2, ga) if (0 in subset or 1 in subset) else (None, None, None)
        ib = (b1, b2, gb) if (2 in subset or 3 in subset) else (None, None, None)
        err = fn(_p(ia[0]), _p(ia[1]), _p(ia[2]), _p(o[0]), _p(o[1]), _p(ib[0]), _p(ib[1]), _p(ib[2]), _p(o[2]), _p(o[3]),
                 B, C, H, W, *PWC, stream)
        assert err == 0, subset
        for i in range(4):
            if i in subset:
                assert same(torch, outs[i], single[i]), (subset, i)
            else:
                assert (outs[i].view(torch.int16) == PATTERN).all(), (subset, i)


def test_backward_channel_groups_differ_from_the_single_calls(torch_mod, cabi):
    """(2, 3, 64, 520): 9 x 16 = 144 tiles.  corr_backward_groups(tiles, batch, channel): groups = min(C, max(1, ceil(2048 /
    (tiles * batch)))), evened out.  A single call (batch 2): ceil(2048 / 288) = 8 -> 3 groups of one channel.  The four-role
    launch counts batch * roles = 8 images: ceil(2048 / 1152) = 2 groups -> two channels in the first group, so its
    double-buffered channel loop runs more than one step; the bits must not depend on it."""
    torch = torch_mod
    B, C, H, W = shape = (2, 3, 64, 520)
    tiles = cl.tiles_of(shape)
    assert cl.backward_groups(tiles, B, C)[1] == 1 and cl.backward_groups(tiles, B * 4, C)[1] == 2
    gen = gen_of(torch, 17)
    a1, a2, b1, b2 = four(torch, gen, shape)
    ga, gb = rnd(torch, gen, B, 81, H, W), rnd(torch, gen, B, 81, H, W)
    got = cabi.correlation_backward_pair(a1, a2, ga, b1, b2, gb, *PWC)
    single = cabi.correlation_backward(a1, a2, ga, *PWC) + cabi.correlation_backward(b1, b2, gb, *PWC)
    assert all(same(torch, g, s) for g, s in zip(got, single))
    ya, yb = cabi.correlation_lrelu_forward_pair(a1, a2, b1, b2, *PWC, SLOPE)
    got = cabi.correlation_lrelu_backward_pair(a1, a2, ya, ga, b1, b2, yb, gb, *PWC, SLOPE)
    single = cabi.correlation_lrelu_backward(a1, a2, ya, ga, *PWC, SLOPE) + cabi.correlation_lrelu_backward(b1, b2, yb, gb, *PWC, SLOPE)
    assert all(same(torch, g, s) for g, s in zip(got, single))


def test_backward_other_configuration_is_one_launch_per_gradient(torch_mod, cabi):
    torch = torch_mod
    shape = (2, 5, 9, 14)
    gen = gen_of(torch, 19)
    a1, a2, b1, b2 = four(torch, gen, shape)
    gshape = (2,) + cabi.correlation_output_dims(9, 14, *OTHER)
    ga, gb = rnd(torch, gen, *gshape), rnd(torch, gen, *gshape)
    single = cabi.correlation_backward(a1, a2, ga, *OTHER) + cabi.correlation_backward(b1, b2, gb, *OTHER)
    for want in ((True,) * 4, (False, True, True, False)):
        got = cabi.correlation_backward_pair(a1, a2, ga, b1, b2, gb, *OTHER, want=want)
        assert all((g is None) if not w else same(torch, g, s) for g, s, w in zip(got, single, want))
    ya, yb = cabi.correlation_lrelu_forward_pair(a1, a2, b1, b2, *OTHER, SLOPE)
    got = cabi.correlation_lrelu_backward_pair(a1, a2, ya, ga, b1, b2, yb, gb, *OTHER, SLOPE)
    single = cabi.correlation_lrelu_backward(a1, a2, ya, ga, *OTHER, SLOPE) + cabi.correlation_lrelu_backward(b1, b2, yb, gb, *OTHER, SLOPE)
    assert all(same(torch, g, s) for g, s in zip(got, single)) and single[0].float().abs().max() > 0


@pytest.mark.parametrize("cfg", [PWC, OTHER])
def test_lrelu_backward_reads_strided_gradients_and_saved_outputs(torch_mod, cabi, cfg):
    """gradoutput of item a is the narrow() view torch.cat's backward hands down, of item b one of another width (the two
    items' strides differ); y of item a is a channel slice of a concatenation buffer, of item b dense."""
    torch = torch_mod
    B, C, H, W = shape = (2, 5, 7, 70)
    gen = gen_of(torch, 23)
    a1, a2, b1, b2 = four(torch, gen, shape, swapped=True)
    oc, oh, ow = cabi.correlation_output_dims(H, W, *cfg)
    ga = rnd(torch, gen, B, oc + 9, oh, ow).narrow(1, 0, oc)
    gb = rnd(torch, gen, B, oc + 4, oh, ow).narrow(1, 4, oc)
    cat = rnd(torch, gen, B, oc + 19, oh, ow)
    ya, yb = cabi.correlation_lrelu_forward_pair(a1, a2, b1, b2, *cfg, SLOPE, out=(cat[:, 7:7 + oc], None))
    assert not ga.is_contiguous() and not ya.is_contiguous() and ga.stride(0) != gb.stride(0) and ya.stride(0) != yb.stride(0)
    assert cabi._planes(ga)[0] is ga and cabi._planes(ya)[0] is ya                 # read where they lie
    single = cabi.correlation_lrelu_backward(a1, a2, ya.contiguous(), ga.contiguous(), *cfg, SLOPE) + \
        cabi.correlation_lrelu_backward(b1, b2, yb, gb.contiguous(), *cfg, SLOPE)
    got = cabi.correlation_lrelu_backward_pair(a1, a2, ya, ga, b1, b2, yb, gb, *cfg, SLOPE)
    assert all(same(torch, g, s) for g, s in zip(got, single))
    got = cabi.correlation_lrelu_backward_pair(a1, a2, ya, ga, b1, b2, yb, gb, *cfg, SLOPE, want=(False, True, False, True))
    assert got[0] is None and got[2] is None and same(torch, got[1], single[1]) and same(torch, got[3], single[3])
    # the mask does something: the unmasked gradients differ
    plain = cabi.correlation_backward_pair(a1, a2, ga, b1, b2, gb, *cfg)
    assert not same(torch, plain[0], single[0])


# ------------------------------------------------------------------ planted values

def _plant(torch, t, values):
    """values at the frame's corners, on its edges and one pixel inside them (the taps next to the zero padding), in the
    first and last plane of the first and last image"""
    H, W = t.shape[2:]
    spots = [(0, 0), (0, 1), (1, 1), (H - 1, W - 1), (H - 2, W - 2), (H - 1, 0), (H // 2, W - 1), (1, W - 2), (0, W // 2)]
    for i, (y, x) in enumerate(spots):
        t[0 if i % 2 else -1, 0 if i % 3 else -1, y, x] = values[i % len(values)]
    return t


@pytest.mark.parametrize("shape", [(2, 5, 7, 70), (1, 33, 22, 130)])       # the generic forward kernel; the MFMA kernel
def test_non_finite_values_at_the_padding_border(torch_mod, cabi, shape):
    """+-inf, NaN, and a zero next to an infinity (inf * 0 at the border is NaN: the padding is multiplied, not skipped), in
    the inputs and in the gradient: NaN positions and every other bit are the single entries'."""
    torch = torch_mod
    inf, nan = float("inf"), float("nan")
    gen = gen_of(torch, 29)
    a1, a2, b1, b2 = four(torch, gen, shape)
    a1, b2 = _plant(torch, a1, (inf, 0.0, -inf, nan)), _plant(torch, b2, (0.0, inf, nan, -inf))
    a2, b1 = _plant(torch, a2, (0.0, -inf, inf, 0.0)), _plant(torch, b1, (nan, 0.0, inf, 0.0))
    B, _, H, W = shape
    ga, gb = _plant(torch, rnd(torch, gen, B, 81, H, W), (inf, nan, 0.0, -inf)), _plant(torch, rnd(torch, gen, B, 81, H, W), (-inf, 0.0, nan))
    outa, outb = cabi.correlation_forward_pair(a1, a2, b1, b2, *PWC)
    assert outa.isnan().any() and outa.isinf().any() and outb.isnan().any()
    assert same(torch, outa, cabi.correlation_forward(a1, a2, *PWC)) and same(torch, outb, cabi.correlation_forward(b1, b2, *PWC))
    ya, yb = cabi.correlation_lrelu_forward_pair(a1, a2, b1, b2, *PWC, SLOPE)
    assert same(torch, ya, cabi.correlation_lrelu_forward(a1, a2, *PWC, SLOPE)) and same(torch, yb, cabi.correlation_lrelu_forward(b1, b2, *PWC, SLOPE))
    got = cabi.correlation_backward_pair(a1, a2, ga, b1, b2, gb, *PWC)
    single = cabi.correlation_backward(a1, a2, ga, *PWC) + cabi.correlation_backward(b1, b2, gb, *PWC)
    assert all(g.isnan().any() for g in got) and all(same(torch, g, s) for g, s in zip(got, single))
    got = cabi.correlation_lrelu_backward_pair(a1, a2, ya, ga, b1, b2, yb, gb, *PWC, SLOPE)
    single = cabi.correlation_lrelu_backward(a1, a2, ya, ga, *PWC, SLOPE) + cabi.correlation_lrelu_backward(b1, b2, yb, gb, *PWC, SLOPE)
    assert all(same(torch, g, s) for g, s in zip(got, single))


# ------------------------------------------------------------------ autograd

def _grads(torch, outs, gouts, leaves):
    for x in leaves:
        x.grad = None
    torch.autograd.backward([o for o, g in zip(outs, gouts) if g is not None], [g for g in gouts if g is not None])
    return [x.grad for x in leaves]


@pytest.mark.parametrize("lrelu", [False, True])
def test_autograd_on_bfloat16_leaves_equals_the_single_functions(torch_mod, cabi, lrelu):
    torch = torch_mod
    from vfidkr_amd import fused
    shape = (2, 6, 9, 70)
    gen = gen_of(torch, 31)
    leaves = [t.requires_grad_(True) for t in four(torch, gen, shape)]
    ga, gb = rnd(torch, gen, 2, 81, 9, 70), rnd(torch, gen, 2, 81, 9, 70)
    if lrelu:
        pair = lambda: fused.corr_pair_lrelu(*leaves, negative_slope=SLOPE)                          # noqa: E731
        one = lambda x, y: fused._CorrLrelu.apply(x, y, SLOPE)                                      # noqa: E731
    else:
        pair = lambda: fused._CorrPair.apply(*leaves)                                               # noqa: E731
        one = fused._Corr.apply
    want_outs = [one(leaves[0], leaves[1]), one(leaves[2], leaves[3])]
    want = _grads(torch, want_outs[:1], [ga], leaves)[:2] + _grads(torch, want_outs[1:], [gb], leaves)[2:]
    outs = pair()
    assert all(o.dtype == torch.bfloat16 and o.grad_fn is not None for o in outs)
    assert same(torch, outs[0], want_outs[0]) and same(torch, outs[1], want_outs[1])
    got = _grads(torch, outs, [ga, gb], leaves)
    assert all(g.dtype == torch.bfloat16 and same(torch, g, w) for g, w in zip(got, want))
    # a cost volume the loss does not use: None for its item
    got = _grads(torch, pair(), [None, gb], leaves)
    assert got[0] is None and got[1] is None and same(torch, got[2], want[2]) and same(torch, got[3], want[3])
    # leaves that need no gradient get none
    leaves[0].requires_grad_(False)
    leaves[3].requires_grad_(False)
    got = _grads(torch, pair(), [ga, gb], leaves)
    assert got[0] is None and got[3] is None and same(torch, got[1], want[1]) and same(torch, got[2], want[2])


def test_under_autocast_a_two_conv_stand_in_feeds_corr_pair_lrelu(torch_mod, cabi):
    """Two convolutions under torch.autocast(dtype=torch.bfloat16) stand in for the feature pyramid: their bfloat16 outputs go
    into corr_pair_lrelu as (f0, f1) and (f1, f0) with no cast, and the loss reaches the convolutions.  Cost volumes and
    feature gradients are those of two _CorrLrelu calls, bit for bit (a feature's two gradients are added once, in either
    order)."""
    torch = torch_mod
    from vfidkr_amd import fused
    gen = gen_of(torch, 37)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.LeakyReLU(0.1), torch.nn.Conv2d(8, 6, 3, padding=1)).cuda()
    img0, img1 = torch.randn(1, 3, 12, 70, generator=gen).cuda(), torch.randn(1, 3, 12, 70, generator=gen).cuda()
    wa, wb = rnd(torch, gen, 1, 81, 12, 70), rnd(torch, gen, 1, 81, 12, 70)

    def run(paired):
        net.zero_grad(set_to_none=True)
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            f0, f1 = net(img0), net(img1)
            assert f0.dtype == torch.bfloat16 and f0.requires_grad
            f0.retain_grad()
            f1.retain_grad()
            if paired:
                ya, yb = fused.corr_pair_lrelu(f0, f1, f1, f0, negative_slope=SLOPE)
            else:
                ya, yb = fused._CorrLrelu.apply(f0, f1, SLOPE), fused._CorrLrelu.apply(f1, f0, SLOPE)
            assert ya.dtype == torch.bfloat16 and yb.dtype == torch.bfloat16
        torch.autograd.backward([ya, yb], [wa, wb])
        grad = net[0].weight.grad
        assert grad is not None and torch.isfinite(grad).all() and grad.abs().max() > 0
        return ya.detach(), yb.detach(), f0.grad, f1.grad

    run(False)                                              # (the convolutions have chosen their algorithms)
    want, got = run(False), run(True)
    assert all(same(torch, g, w) for g, w in zip(got, want))
    assert got[2].float().abs().max() > 0


# ------------------------------------------------------------------ graph capture

def test_forward_and_backward_pair_replay_from_one_single_stream_graph(torch_mod, cabi):
    torch = torch_mod
    shape = (2, 6, 9, 70)
    gen = gen_of(torch, 41)
    static = list(four(torch, gen, shape)) + [rnd(torch, gen, 2, 81, 9, 70), rnd(torch, gen, 2, 81, 9, 70)]

    def step(a1, a2, b1, b2, ga, gb):
        ya, yb = cabi.correlation_lrelu_forward_pair(a1, a2, b1, b2, *PWC, SLOPE)
        return (ya, yb) + cabi.correlation_lrelu_backward_pair(a1, a2, ya, ga, b1, b2, yb, gb, *PWC, SLOPE) + \
            cabi.correlation_backward_pair(a1, a2, ga, b1, b2, gb, *PWC, want=(False, True, False, True))[1::2]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(*static)
    for seed in (43, 47):
        fresh = list(four(torch, gen_of(torch, seed), shape)) + [rnd(torch, gen, 2, 81, 9, 70), rnd(torch, gen, 2, 81, 9, 70)]
        for s, f in zip(static, fresh):
            s.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(*fresh)
        assert len(eager) == 8 and all(same(torch, c, e) for c, e in zip(captured, eager)), seed
        assert captured[2].float().abs().max() > 0
