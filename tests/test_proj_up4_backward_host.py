"""CPU suite: the quarter-resolution backwards (vfi_flow_upsample4_backward, vfi_[depth]flowprojection_backward_up4) without
a GPU -- the numpy mirror of up4_adjoint against torch autograd, its analytic case, and the entry points' refusals."""
import ctypes

import numpy as np
import pytest

from tests import proj_up4_backward as M
from tests.test_abi_and_host import built  # noqa: F401  (fixture)

f32 = np.float32
# hq or wq of 1, 2 and 3: the taps of a pixel are clamped on both sides at once
SHAPES = [(1, 2, 1, 1), (1, 2, 1, 5), (2, 2, 5, 1), (1, 1, 2, 2), (1, 2, 2, 7), (2, 3, 3, 3), (1, 2, 3, 9), (1, 2, 4, 6), (2, 2, 9, 17)]


@pytest.mark.parametrize("B,C,hq,wq", SHAPES)
@pytest.mark.parametrize("nitems", [1, 3])
def test_mirror_equals_torch_autograd(B, C, hq, wq, nitems):
    """ref64 of the mirror = d/dq sum_i <G_i, interpolate(m0 * q * m1_i, x4, bilinear)> of torch in float64, to 1e-12 of S"""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(B + 10 * C + 100 * hq + 1000 * wq + nitems)
    m0, m1s = 20.0, [0.25, 0.5, 0.75][:nitems]
    Gs = [rng.standard_normal((B, C, 4 * hq, 4 * wq)).astype(f32) for _ in m1s]
    q = torch.zeros((B, C, hq, wq), dtype=torch.float64, requires_grad=True)
    loss = sum((F.interpolate(float(f32(m0) * f32(m1)) * q, scale_factor=4, mode="bilinear", align_corners=False)
                * torch.from_numpy(G.astype(np.float64))).sum() for G, m1 in zip(Gs, m1s))
    loss.backward()
    got32, ref, S, n = M.up4_backward(Gs, m0, m1s)
    want = q.grad.numpy()
    assert np.all(np.abs(ref - want) <= 1e-12 * S), np.abs(ref - want).max()
    # the float32 result obeys the bound the GPU test uses
    assert np.all(np.abs(got32.astype(np.float64) - ref) <= (n + 12) * 2.0 ** -24 * S)
    assert n.max() <= 64 * nitems and n.min() >= min(4 * hq, 6) * min(4 * wq, 6) * nitems


def test_footprint_is_the_set_of_pixels_with_a_tap_on_q():
    for size in (1, 2, 3, 4, 9):
        d, w, valid = M.footprint(size)
        i0, i1, l0, l1 = M.up4_tap(np.arange(4 * size), size)
        for q in range(size):
            full = np.where(i0 == q, l0, 0) + np.where(i1 == q, l1, 0)          # weight of q in every pixel of the axis
            inside = np.zeros(4 * size)
            inside[d[q][valid[q]]] = w[q][valid[q]]
            assert np.array_equal(full.astype(f32), inside.astype(f32))
        assert np.allclose(w.sum(0).sum(), 4 * size)        # every pixel's two taps sum to 1


@pytest.mark.parametrize("B,C,hq,wq", [(1, 2, 1, 1), (1, 2, 3, 2), (2, 2, 6, 11)])
def test_constant_gradient_sums_to_the_multiplier(B, C, hq, wq):
    m0, m1 = 20.0, 0.25
    G = np.full((B, C, 4 * hq, 4 * wq), 0.5, f32)
    got32, ref, S, n = M.up4_backward([G], m0, [m1])
    want = m0 * m1 * float(G.astype(np.float64).sum())
    assert abs(ref.sum() - want) <= 1e-12 * abs(want)
    assert abs(float(got32.astype(np.float64).sum()) - want) <= 1e-5 * abs(want)


def test_fma32_rounds_once():
    a = f32(1 + 2.0 ** -12)
    assert f32(a * a) - f32(1) == f32(2.0 ** -11)           # the product alone rounds its 2^-24 away
    assert M.fma32(a, a, f32(-1.0)) == f32(2.0 ** -11 + 2.0 ** -24)
    # 64 (1 - 2^-46) + (2^30 + 128) lies just below a float32 tie; float64 rounds it ONTO the tie, and a second rounding
    # would then go up to the even neighbour
    x, y, c = f32(8 + 2.0 ** -20), f32(8 - 2.0 ** -20), f32(2.0 ** 30 + 128)
    assert f32(np.float64(x) * np.float64(y) + np.float64(c)) == f32(2.0 ** 30 + 256)
    assert M.fma32(x, y, c) == f32(2.0 ** 30 + 128)


def test_entry_points_refuse_bad_arguments_without_a_gpu(built):  # noqa: F811
    from vfidkr_amd import cabi
    lib = cabi.lib()
    S = cabi.Strides
    fake = ctypes.c_void_p(4096)                            # never dereferenced: every call below returns before a launch
    table = (ctypes.c_void_p * 9)(*[4096] * 9)
    null_entry = (ctypes.c_void_p * 9)(4096, None, 4096, 4096, 4096, 4096, 4096, 4096, 4096)
    mul = (ctypes.c_float * 9)(*[0.5] * 9)
    sq, sf = S(2 * 6 * 10, 6 * 10, 10), S(2 * 24 * 40, 24 * 40, 40)
    sc = S(24 * 40, 24 * 40, 40)

    def up(g=table, m=mul, n=3, gq=fake, b=1, c=2, hq=6, wq=10, sg=sf, s=sq):
        return lib.vfi_flow_upsample4_backward(g, m, n, gq, b, c, hq, wq, 20.0, sg, s, None)

    def fp(fq=fake, cn=table, go=table, m=mul, n=3, gq=fake, b=1, hq=6, wq=10, s=sq, c=sc, o=sf, gs=sq):
        return lib.vfi_flowprojection_backward_up4(fq, cn, go, m, n, gq, b, hq, wq, 20.0, s, c, o, gs, None)

    def dp(fq=fake, d=table, cn=table, out=table, go=table, m=mul, n=3, gq=fake, gd=None, b=1, hq=6, wq=10, s=sq, s2=sc, c=sc,
           o=sf, gs=sq):
        return lib.vfi_depthflowprojection_backward_up4(fq, d, cn, out, go, m, n, gq, gd, b, hq, wq, 20.0, s, s2, c, o, gs, None)

    E = cabi.VFI_ERR_SHAPE
    for call in (up, fp, dp):
        assert call(n=0) == E and call(n=9) == E and call(n=-1) == E
        assert call(gq=None) == E and call(m=None) == E
        assert call(b=0) == E and call(hq=0) == E and call(wq=-3) == E and call(hq=2 ** 29) == E
        assert call(s=S(0, 0, 2 ** 31)) == E                # a row stride beyond 32-bit in-plane offsets
    assert up(g=None) == E and up(g=null_entry) == E and up(c=0) == E and up(sg=S(0, 0, 2 ** 30)) == E
    assert fp(fq=None) == E and fp(cn=None) == E and fp(go=None) == E and fp(cn=null_entry) == E and fp(go=null_entry) == E
    assert fp(c=S(0, 0, 2 ** 30)) == E and fp(o=S(0, 0, 2 ** 30)) == E and fp(gs=S(0, 0, 2 ** 31)) == E
    assert dp(fq=None) == E and dp(d=None) == E and dp(cn=None) == E and dp(out=None) == E and dp(go=None) == E
    assert dp(d=null_entry) == E and dp(out=null_entry) == E and dp(s2=S(0, 0, 2 ** 30)) == E


def test_wrappers_refuse_mismatched_sizes_and_cpu_tensors(built):  # noqa: F811
    import torch
    from vfidkr_amd import cabi, fused
    z = torch.zeros
    q, gq = z(1, 2, 6, 10), z(1, 2, 6, 10)
    full2, full1 = z(1, 2, 24, 40), z(1, 1, 24, 40)
    # mismatched sizes: the binding's silent `return 1`, before anything touches a device
    assert cabi.flow_upsample4_backward([z(1, 2, 24, 44)], 20.0, [0.5], gq) == 1
    assert cabi.flow_upsample4_backward([full2, z(1, 2, 24, 36)], 20.0, [0.5, 0.25], gq) == 1
    assert cabi.flow_upsample4_backward([full2], 20.0, [0.5, 0.25], gq) == 1
    assert cabi.flow_upsample4_backward([], 20.0, [], gq) == 1
    assert cabi.flowprojection_backward_up4(q, [z(1, 1, 24, 36)], [full2], 20.0, [0.5], gq) == 1
    assert cabi.flowprojection_backward_up4(q, [full1], [z(1, 2, 20, 40)], 20.0, [0.5], gq) == 1
    assert cabi.flowprojection_backward_up4(q, [full1], [full2], 20.0, [0.5], z(1, 2, 6, 9)) == 1
    assert cabi.flowprojection_backward_up4(q, [full1], [full2, full2], 20.0, [0.5, 0.25], gq) == 1
    assert cabi.flowprojection_backward_up4(q, [full1], [full2], 20.0, [0.5], gq, depths=z(1, 1, 24, 36), outputs=[full2]) == 1
    assert cabi.flowprojection_backward_up4(q, [full1], [full2], 20.0, [0.5], gq, depths=full1) == 1          # no outputs
    # right sizes on the CPU: refused as the other wrappers refuse them
    with pytest.raises(RuntimeError, match="no CPU path"):
        cabi.flow_upsample4_backward([full2], 20.0, [0.5], gq)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cabi.flowprojection_backward_up4(q, [full1], [full2], 20.0, [0.5], gq)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cabi.flowprojection_backward_up4(q, [full1], [full2], 20.0, [0.5], gq, depths=full1, outputs=[full2], grad_depths=[None])
    for wants_grad in (False, True):
        fq = z(1, 2, 6, 10, requires_grad=wants_grad)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fused.forward_flownets_upsample(fq, 20.0, [0.25, 0.5])
        with pytest.raises(RuntimeError, match="no CPU path"):
            fused.FlowProject_from_quarter(fq, 20.0, [0.25, 0.5])
        with pytest.raises(RuntimeError, match="no CPU path"):
            fused.FlowProject_from_quarter(fq, 20.0, [0.5], depth=full1, fillhole=False)
