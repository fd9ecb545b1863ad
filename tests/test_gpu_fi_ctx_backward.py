"""vfi_filterinterp_backward_ori_image_multi on the GPU: the image gradient of FilterInterpolation `_ori` summed over
several flows (the backward of the context warp), through every tile class of tests/fi_ctx_backward.py.

  * one flow: bit-equal to gradinput1 of vfi_filterinterp_backward_ori on zero-filled outputs;
  * 1, 2 and 3 flows on the builder's fields, and one flow more than a launch carries: bit-equal to the restatement (exact
    integer sums of the rounded fp32 addends of every flow at the call's one scale, converted once), the same bits on a second
    run and with the flows in another order; a mismatch names the classes of the tiles that reach the failing cells;
  * the output arrives filled with NaN: every element is written;
  * channel-slice views with the parent's batch stride: nothing outside the slice changes;
  * 25 filter channels and tiny gradients (the per-tap kernel takes the call) bit-equal to the restatement;
  * a +inf and a NaN in one flow's gradient (fp32 atomics): NaN and +inf where the per-flow calls summed by torch put them,
    finite cells within the float64 bound;
  * autograd through fused.FilterInterpolate_ctx_all / FilterInterpolate_ctx.
"""
import functools

import numpy as np
import pytest

from tests import bwd_tiles as bt
from tests import fi_ctx_backward as fc
from tests.test_gpu_backward import IMG_ROUNDINGS, U, assert_image_grad
from tests.test_gpu_parity import cpu, gpu, torch_mod, cabi  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

f32 = np.float32
B, C, H, W = 2, 7, 43, 200


@functools.lru_cache(maxsize=None)
def case(nflows, filter_channels=16, dyadic=False):
    """(flows, filt, gouts) on the builder's field of nflows flows"""
    rng = np.random.default_rng(700 + nflows + filter_channels)
    flows = fc.build_field(rng, B, H, W, nflows)
    filt = rng.random((B, filter_channels, H, W), dtype=f32)
    gouts = [np.clip(rng.standard_normal((B, C, H, W)), -3, 3).astype(f32) for _ in range(nflows)]
    if dyadic:
        filt = (np.round(filt * 16) / 16).astype(f32)
        gouts = [(np.round(g * 16) / 16).astype(f32) for g in gouts]
    return flows, filt, gouts


@functools.lru_cache(maxsize=None)
def predicted(nflows, filter_channels=16):
    flows, filt, gouts = case(nflows, filter_channels)
    want, k, fp32 = fc.predict(flows, gouts, filt)
    assert not fp32
    return want, k


def run(torch, cabi, flows, filt, gouts, order=None):
    """one call into a NaN-filled gradient; numpy"""
    order = range(len(flows)) if order is None else order
    g1 = torch.full(gouts[0].shape, float("nan"), device="cuda:0")
    assert cabi.filterinterp_backward_ori_image_multi([gpu(torch, flows[t]) for t in order], gpu(torch, filt),
                                                      [gpu(torch, gouts[t]) for t in order], g1) == 0
    return cpu(g1)


def assert_bits(got, want, recs, what):
    if np.array_equal(got, want, equal_nan=True):
        return
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    raise AssertionError("%s: %s" % (what, bt.name_cells(recs, "ctx", [tuple(i) for i in bad], got.shape[2], got.shape[3])))


def test_one_flow_equals_the_full_backward(torch_mod, cabi):
    torch = torch_mod
    flows, filt, gouts = case(1)
    img = np.random.default_rng(3).random((B, C, H, W), dtype=f32)
    g1, g2, g3 = (torch.zeros(s, device="cuda:0") for s in ((B, C, H, W), (B, 2, H, W), (B, 16, H, W)))
    assert cabi.filterinterp_backward_ori(gpu(torch, img), gpu(torch, flows[0]), gpu(torch, filt), gpu(torch, gouts[0]),
                                          g1, g2, g3) == 0
    got = run(torch, cabi, flows, filt, gouts)
    assert_bits(got, cpu(g1), fc.tiles(flows, C), "against vfi_filterinterp_backward_ori")


@pytest.mark.parametrize("nflows", [1, 2, 3])
def test_every_tile_class(torch_mod, cabi, np_oracle, nflows):
    torch = torch_mod
    flows, filt, gouts = case(nflows)
    want, k = predicted(nflows)
    recs = fc.tiles(flows, C)
    assert not [lab for lab in fc.all_labels(nflows) if lab not in bt.label_counts(recs)]
    got = run(torch, cabi, flows, filt, gouts)
    assert_bits(got, want, recs, "%d flows against the restatement" % nflows)
    again = run(torch, cabi, flows, filt, gouts)
    assert_bits(again, got, recs, "%d flows, second run" % nflows)
    order = list(range(nflows))[::-1] if nflows > 1 else [0]
    assert_bits(run(torch, cabi, flows, filt, gouts, order), got, recs, "%d flows, reversed" % nflows)
    if nflows == 3:
        assert_bits(run(torch, cabi, flows, filt, gouts, [1, 2, 0]), got, recs, "3 flows, rotated")
        # independently of the restatement: within the float64 bound
        stats = [np_oracle.filterinterp_ori_bwd_img(fl, filt, g) for fl, g in zip(flows, gouts)]
        assert_image_grad(got, np.zeros_like(got), tuple(sum(s[i] for s in stats) for i in range(3)), k, "ori")


def test_more_flows_than_one_launch_carries(torch_mod, cabi):
    torch = torch_mod
    n = fc.CB_NT + 1
    flows, filt, gouts = case(n)
    want, _ = predicted(n)
    got = run(torch, cabi, flows, filt, gouts)
    assert_bits(got, want, fc.tiles(flows[:fc.CB_NT], C), "%d flows against the restatement" % n)


def test_long_channel_loop(torch_mod, cabi):
    """C = 196 on a 24 x 72 frame, three flows: channel groups, and 196 = 6 x 32 + 4 channels of passes"""
    torch = torch_mod
    rng = np.random.default_rng(77)
    b, c, h, w = 1, 196, 24, 72
    assert fc.channel_groups(b, c, h, w)[1] > 1
    flows = [(np.round(rng.uniform(-2.5, 2.5, (b, 2, h, w)) * 16) / 16).astype(f32) for _ in range(3)]
    filt = rng.random((b, 16, h, w), dtype=f32)
    gouts = [rng.standard_normal((b, c, h, w)).astype(f32) for _ in range(3)]
    want, k, fp32 = fc.predict(flows, gouts, filt)
    assert not fp32
    assert_bits(run(torch, cabi, flows, filt, gouts), want, fc.tiles(flows, c), "C = 196")


def test_channel_slice_views(torch_mod, cabi):
    torch = torch_mod
    flows, filt, gouts = case(2)
    want, _ = predicted(2)
    wide_out = torch.full((B, C + 5, H, W), float("nan"), device="cuda:0")
    g1 = wide_out[:, 2:2 + C]
    wide_g = [torch.full((B, C + 3, H, W), 7.0, device="cuda:0") for _ in gouts]
    gs = [wg[:, 1:1 + C] for wg in wide_g]
    for v, g in zip(gs, gouts):
        v.copy_(torch.from_numpy(g))
    assert g1.stride(0) == (C + 5) * H * W and gs[0].stride(0) == (C + 3) * H * W
    assert cabi.filterinterp_backward_ori_image_multi([gpu(torch, f) for f in flows], gpu(torch, filt), gs, g1) == 0
    assert_bits(cpu(g1), want, fc.tiles(flows, C), "channel-slice views")
    assert torch.isnan(wide_out[:, :2]).all() and torch.isnan(wide_out[:, 2 + C:]).all()
    for wg in wide_g:
        assert (wg[:, :1] == 7.0).all() and (wg[:, 1 + C:] == 7.0).all()


def test_25_filter_channels_take_the_per_tap_kernel(torch_mod, cabi):
    torch = torch_mod
    flows, filt, gouts = case(2, 25)
    want, k = predicted(2, 25)
    assert k == bt.grad_scale(np.stack(gouts), filt, H, W, 25 * 2)[0]
    assert_bits(run(torch, cabi, flows, filt, gouts), want, fc.tiles(flows, C), "25 filter channels")


def test_tiny_gradients_take_the_second_scale_factor(torch_mod, cabi):
    torch = torch_mod
    flows, filt, gouts = case(2)
    gouts = [(g * f32(2.0 ** -100)).astype(f32) for g in gouts]
    want, k, fp32 = fc.predict(flows, gouts, filt)
    assert k > 126 and not fp32 and fc.call_scale(gouts, filt, H, W)[3] != 1
    assert_bits(run(torch, cabi, flows, filt, gouts), want, fc.tiles(flows, C, scale2_one=False), "tiny gradients")


def test_non_finite_gradient_lands_where_the_per_flow_calls_put_it(torch_mod, cabi, np_oracle):
    """fp32 atomics for the whole call.  Dyadic inputs: every addend and every partial sum is exact in fp32, so the finite
    cells do not depend on the order of the atomics, here or in the per-flow calls."""
    torch = torch_mod
    flows, filt, gouts = case(3, 16, True)
    gouts = [g.copy() for g in gouts]
    gouts[1][0, 1, 2, 10] = np.inf
    gouts[1][1, 2, 30, 150] = np.nan
    assert fc.call_scale(gouts, filt, H, W)[1]
    got = run(torch, cabi, flows, filt, gouts)
    img = gpu(torch, np.zeros((B, C, H, W), f32))
    total = torch.zeros((B, C, H, W), device="cuda:0")
    for fl, g in zip(flows, gouts):
        g1, g2, g3 = (torch.zeros(s, device="cuda:0") for s in ((B, C, H, W), (B, 2, H, W), (B, 16, H, W)))
        assert cabi.filterinterp_backward_ori(img, gpu(torch, fl), gpu(torch, filt), gpu(torch, g), g1, g2, g3) == 0
        total = total + g1
    ref = cpu(total)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(got).any()
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.isposinf(got).any()
    assert not np.isneginf(got).any() and not np.isneginf(ref).any()
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        S = sum(np_oracle.filterinterp_ori_bwd_img(fl, filt, g)[1] for fl, g in zip(flows, gouts))
    # assert_image_grad's bound without its fixed-point term (no addend is rounded to the integer grid on this path)
    bound = IMG_ROUNDINGS["ori"] * U * S[fin] * (1 + 1e-6) + np.abs(np.spacing(ref[fin]))
    assert np.all(np.abs(got[fin].astype(np.float64) - ref[fin]) <= bound)


def test_autograd_through_the_fused_calls(torch_mod, cabi):
    torch = torch_mod
    from vfidkr_amd import fused
    flows, filt, gouts = case(3)
    rng = np.random.default_rng(9)
    ctx0 = gpu(torch, rng.random((B, C, H, W), dtype=f32)).requires_grad_()
    ctx2 = gpu(torch, rng.random((B, C, H, W), dtype=f32))
    offs = [[gpu(torch, f).requires_grad_() for f in flows], [gpu(torch, f) for f in flows[::-1]]]
    filts = [gpu(torch, filt).requires_grad_(), gpu(torch, filt)]
    with torch.no_grad():
        plain = fused.FilterInterpolate_ctx_all(ctx0, ctx2, offs, filts)
    assert all(o.grad_fn is None for pair in plain for o in pair)
    outs = fused.FilterInterpolate_ctx_all(ctx0, ctx2, offs, filts)
    assert all(a.grad_fn is not None and b.grad_fn is None for a, b in outs)
    for (a, b), (pa, pb) in zip(outs, plain):
        assert torch.equal(a, pa) and torch.equal(b, pb)
    ga, gb = gpu(torch, gouts[0]), gpu(torch, gouts[2])
    ((outs[0][0] * ga).sum() + (outs[2][0] * gb).sum()).backward()         # the middle offset arrives as a None gradient
    want = torch.full((B, C, H, W), float("nan"), device="cuda:0")
    assert cabi.filterinterp_backward_ori_image_multi([offs[0][0].detach(), offs[0][2].detach()], filts[0].detach(),
                                                      [ga, gb], want) == 0
    assert torch.equal(ctx0.grad, want)
    assert all(f.grad is None for f in offs[0]) and filts[0].grad is None
    # the single-offset form
    ctx0.grad = None
    o0, o2 = fused.FilterInterpolate_ctx(ctx0, ctx2, [offs[0][1], offs[1][1]], filts)
    assert torch.equal(o0, plain[1][0]) and torch.equal(o2, plain[1][1]) and o2.grad_fn is None
    (o0 * ga).sum().backward()
    assert cabi.filterinterp_backward_ori_image_multi([offs[0][1].detach()], filts[0].detach(), [ga], want) == 0
    assert torch.equal(ctx0.grad, want)
