"""CPU suite: the fused training losses (vfi_part_loss_forward / _backward, fused.part_loss) without a GPU -- the float32
mirror of the kernel's arithmetic against float64 within the bounds the GPU tests use, the closed-form gradients against
torch autograd, and the entry points' refusals."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import part_loss as M
from tests.test_abi_and_host import PKG, built  # noqa: F401  (fixture)

f32, f64 = np.float32, np.float64
EPS = 1e-6
SHAPES = [(1, 1, 2, 2), (1, 3, 2, 5), (2, 3, 3, 4), (1, 3, 5, 9), (3, 3, 17, 67)]


def make_inputs(rng, B, C, H, W, nd=2, with_target=False):
    """images in [0, 1] (the exponent of w is then bounded by 2 C), outputs near them, flows of a few pixels"""
    images = [rng.random((B, C, H, W)).astype(f32) for _ in range(2)]
    target = rng.random((B, C, H, W)).astype(f32) if with_target else None
    diffs = [(rng.standard_normal((B, C, H, W)) * 0.1).astype(f32) + (target if with_target else 0) for _ in range(nd)]
    flows = [(rng.standard_normal((B, 2, H, W)) * 3.0).astype(f32) for _ in range(2)]
    return diffs, target, flows, images


@pytest.mark.parametrize("neg", [False, True], ids=["charbonnier", "negpsnr"])
@pytest.mark.parametrize("with_target", [False, True], ids=["diffs", "target"])
@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_mirror_values_within_the_derived_bounds(B, C, H, W, with_target, neg):
    rng = np.random.default_rng(B + 10 * C + 100 * H + 1000 * W)
    diffs, target, flows, images = make_inputs(rng, B, C, H, W, 2, with_target)
    got, means = M.values(diffs, target, flows, images, EPS, neg)
    ref = M.reference64(diffs, target, flows, images, EPS, neg)
    bound = M.value_bounds(ref, diffs, target, flows, images, EPS, neg)
    assert got.dtype == f32 and means.shape == (2, B)
    assert np.all(np.abs(got.astype(f64) - ref) <= bound), (got, ref, bound)
    # the float64 evaluation of the same functions agrees with torch's to float64 rounding
    got64, _ = M.values(diffs, target, flows, images, EPS, neg, dtype=f64)
    assert np.all(np.abs(got64 - ref) <= 1e-12 * np.abs(ref) + 1e-15)
    # without flows the last two values are zeros
    none, _ = M.values(diffs, target, None, None, EPS, neg)
    assert none[2] == 0 and none[3] == 0 and np.array_equal(none[:2], got[:2])


@pytest.mark.parametrize("neg", [False, True], ids=["charbonnier", "negpsnr"])
@pytest.mark.parametrize("B,C,H,W", SHAPES)
def test_closed_form_gradients_equal_autograd_and_the_mirror_obeys_the_bound(B, C, H, W, neg):
    rng = np.random.default_rng(7 + B + 10 * C + 100 * H + 1000 * W)
    diffs, target, flows, images = make_inputs(rng, B, C, H, W, 2, True)
    gv = np.array([0.7, -1.3, 0.9, 1.1], f32)
    _, gd64, gf64 = M.reference64(diffs, target, flows, images, EPS, neg, gv)
    _, means32 = M.values(diffs, target, flows, images, EPS, neg)
    for i in range(2):
        x64 = M.diff_of(diffs[i].astype(f64), target.astype(f64))
        means64 = M.charbonnier(x64, M.e2_of(EPS, f64)).reshape(B, -1).mean(1)
        closed = M.pixel_grad(diffs[i], target, gv[i], EPS, neg, means64, dtype=f64)
        scale = np.abs(gd64[i]).max()
        assert np.all(np.abs(closed - gd64[i]) <= 1e-12 * scale)
        got = M.pixel_grad(diffs[i], target, gv[i], EPS, neg, means32[i])
        assert got.dtype == f32
        # out - target, the ratio's three roundings and divide, the coefficient's divides (and the sample mean's own
        # K_PIXEL with neg_psnr), the product: 16 u covers them
        assert np.all(np.abs(got.astype(f64) - gd64[i]) <= 16 * M.U * np.abs(gd64[i]))
    for s in range(2):
        f, other, img = flows[s], flows[1 - s], images[s]
        closed = M.flow_grad(f, other, img, gv[2], gv[3], EPS, dtype=f64)
        assert np.all(np.abs(closed - gf64[s]) <= 1e-12 * np.abs(gf64[s]).max())
        got = M.flow_grad(f, other, img, gv[2], gv[3], EPS)
        bound = M.flow_grad_bound(f, other, img, gv[2], gv[3], EPS)
        assert got.dtype == f32 and np.all(np.abs(got.astype(f64) - gf64[s]) <= bound)
        # an unused loss is an absent term
        tv_only = M.flow_grad(f, other, img, gv[2], None, EPS, dtype=f64)
        sym_only = M.flow_grad(f, other, img, None, gv[3], EPS, dtype=f64)
        assert np.all(np.abs(tv_only + sym_only - closed) <= 1e-12 * np.abs(closed).max())


def test_constants_match_the_kernel_source():
    text = open(os.path.join(PKG, "csrc", "losses.hip")).read()
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))    # noqa: E731
    assert define("LOSS_THREADS") == M.THREADS and define("LOSS_FINISH_THREADS") == M.FINISH_THREADS
    assert define("LOSS_DIFF_UNITS_PER_THREAD") * M.THREADS == M.DIFF_BLOCK_UNITS
    assert re.search(r"#define LOSS_FLOW_BLOCK_UNITS LOSS_THREADS\b", text) and M.FLOW_BLOCK_UNITS == M.THREADS
    assert M.partial_counts(3, 3, 256, 448) == (84, 112)
    assert "losses.hip" in open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "WS_LOSS" in open(os.path.join(PKG, "csrc", "workspace.h")).read()


def test_entry_points_refuse_bad_arguments_without_a_gpu(built):  # noqa: F811
    from vfidkr_amd import cabi
    lib = cabi.lib()
    S = cabi.Strides
    fake = ctypes.c_void_p(4096)                            # never dereferenced: every call below returns before a launch
    table = (ctypes.c_void_p * 8)(*[4096] * 8)
    null_entry = (ctypes.c_void_p * 8)(4096, None, 4096, 4096, 4096, 4096, 4096, 4096)
    sd, sf = S(3 * 8 * 12, 8 * 12, 12), S(2 * 8 * 12, 8 * 12, 12)

    def fwd(d=table, nd=2, t=None, f0=fake, f1=fake, i0=fake, i1=fake, b=1, cd=3, ci=3, h=8, w=12, v=fake, m=fake):
        return lib.vfi_part_loss_forward(d, nd, t, f0, f1, i0, i1, b, cd, ci, h, w, 1e-6, 0, v, m, sd, sf, sd, None)

    def bwd(d=table, nd=2, t=None, f0=fake, f1=fake, i0=fake, i1=fake, b=1, cd=3, ci=3, h=8, w=12, gv=fake, m=fake, neg=0,
            gd=table, g0=fake, g1=fake):
        return lib.vfi_part_loss_backward(d, nd, t, f0, f1, i0, i1, b, cd, ci, h, w, 1e-6, neg, gv, m, 0xF, gd, g0, g1, sd, sf,
                                          sd, sd, sf, None)

    E = cabi.VFI_ERR_SHAPE
    assert E == 1
    for call in (fwd, bwd):
        assert call(d=None) == E and call(d=null_entry) == E
        assert call(nd=0) == E and call(nd=9) == E and call(nd=-1) == E
        assert call(b=0) == E and call(cd=0) == E and call(h=0) == E and call(w=-2) == E
        assert call(f1=None) == E and call(f0=None) == E                # one flow of the pair
        assert call(i0=None) == E and call(i1=None) == E and call(ci=0) == E
        assert call(h=1) == E and call(w=1) == E                       # with flows: the total variation's mean over nothing
    assert fwd(v=None) == E and fwd(m=None) == E
    assert bwd(gv=None) == E and bwd(neg=1, m=None) == E
    assert bwd(f0=None, f1=None, i0=None, i1=None) == E                 # flow gradients asked for without flows
    # nothing asked for: success without a launch
    assert bwd(gd=None, g0=None, g1=None) == 0
    assert bwd(f0=None, f1=None, i0=None, i1=None, gd=None, g0=None, g1=None, h=1, w=1) == 0


def test_part_loss_signature_and_refusals(built):  # noqa: F811
    import torch
    from vfidkr_amd import cabi, fused
    assert list(inspect.signature(fused.part_loss).parameters) == ["diffs", "offsets", "occlusions", "images", "epsilon",
                                                                   "use_negPSNR", "target"]
    assert inspect.signature(fused.part_loss).parameters["use_negPSNR"].default is False
    assert inspect.signature(fused.part_loss).parameters["target"].default is None
    z = torch.zeros
    diffs = [z(1, 3, 8, 12), z(1, 3, 8, 12)]
    flows, images = [z(1, 2, 8, 12), z(1, 2, 8, 12)], [z(1, 3, 8, 12), z(1, 3, 8, 12)]
    for wants_grad in (False, True):
        d = [t.clone().requires_grad_(wants_grad) for t in diffs]
        with pytest.raises(RuntimeError, match="no CPU path"):
            fused.part_loss(d, [flows], [None], images, 1e-6)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fused.part_loss(d, [[None, None]], [None], images, 1e-6, use_negPSNR=True, target=z(1, 3, 8, 12))
    # images and target are data
    with pytest.raises(RuntimeError, match="requires grad"):
        fused.part_loss(diffs, [flows], [None], [images[0], images[1].clone().requires_grad_(True)], 1e-6)
    with pytest.raises(RuntimeError, match="requires grad"):
        fused.part_loss(diffs, [flows], [None], images, 1e-6, target=z(1, 3, 8, 12, requires_grad=True))
    # mismatched sizes: the binding's silent `return 1`, before anything touches a device
    v, m = z(4), z(2)
    assert cabi.part_loss_forward(diffs, None, flows[0], z(1, 2, 8, 10), *images, 1e-6, False, v, m) == 1
    assert cabi.part_loss_forward(diffs, None, flows[0], None, *images, 1e-6, False, v, m) == 1
    assert cabi.part_loss_forward([diffs[0], z(1, 3, 8, 16)], None, *flows, *images, 1e-6, False, v, m) == 1
    assert cabi.part_loss_forward(diffs, z(1, 3, 4, 12), *flows, *images, 1e-6, False, v, m) == 1
    assert cabi.part_loss_forward(diffs, None, *flows, images[0], z(1, 1, 8, 12), 1e-6, False, v, m) == 1
    assert cabi.part_loss_forward([], None, *flows, *images, 1e-6, False, v, m) == 1
    assert cabi.part_loss_forward(diffs * 5, None, *flows, *images, 1e-6, False, z(12), z(10)) == 1
    with pytest.raises(RuntimeError, match="no CPU path"):
        cabi.part_loss_forward(diffs, None, *flows, *images, 1e-6, False, v, m)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cabi.part_loss_backward(diffs, None, *flows, *images, 1e-6, False, v, m, 0xF, [z(1, 3, 8, 12), None], z(1, 2, 8, 12), None)
    assert cabi.part_loss_backward(diffs, None, *flows, *images, 1e-6, False, v, m, 0xF, [z(1, 3, 8, 10), None]) == 1
    assert cabi.part_loss_backward(diffs, None, None, None, None, None, 1e-6, False, v, m, 0x3, None, z(1, 2, 8, 12)) == 1
