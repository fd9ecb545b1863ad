"""`-m gpu`: the correlation forward kernels on non-finite and extreme values -- every kernel, bit for bit.

The reference multiplies every tap of its zero-padded buffers, so an infinity or a NaN that meets the padding gives NaN
(tests/corr_edges.py).  Each case plants +-inf, NaN, overflowing and subnormal products and -0.0 at corner, edge and
interior pixels and in the last, partial channel chunk, and asserts with the host mirror that it reaches the kernel it
is meant for.  No tolerance anywhere: NaN at the same places, every other element the same bits.

  1. every float kernel against the oracle (sequential channel order, fused multiply-add);
  2. the same values one element off a 16-byte boundary: the kernels that take over give the same bits;
  3. the pair entry equals the two single calls (it selects the kernel the single call selects: the host file searches);
  4. output origins other than pad 4 / pad 0: 4 pixels outside the frame on the 16-byte-staged kernels, 1 outside and 1
     inside on the one-float-staged ones, 2 inside and 4 outside on the flat one (outside: the only way to a first-map
     tap in the padding, 0 * v) -- finite and planted;
  5. the half kernels against the half restatement, and against each other through an odd-offset view;
  6. PWC-Net's warp and the fused warp + correlation with non-finite features and a finite flow, with a source pixel
     sampled at weight exactly 0 and a masked-out pixel.
"""
import functools

import numpy as np
import pytest

from tests import corr_edges as ce
from tests.test_gpu_parity import cpu, gpu, f32, torch_mod, cabi  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def inputs(name, planted=True):
    return ce.case_inputs(name, planted)


@functools.lru_cache(maxsize=None)
def oracle_result(name, planted=True):
    """The oracle's result of a case, computed once and shared (callers do not write to it)."""
    from oracle import cpu_oracle
    cpu_oracle.build()
    f1, f2, _, cfg = inputs(name, planted)
    with np.errstate(all="ignore"):
        if f1.dtype == np.float16:
            out = cpu_oracle.correlation_fwd_f16(f1, f2, *cfg)
        else:
            out = cpu_oracle.correlation_fwd(f1, f2, *cfg, order=1, fmad=1)
    out.setflags(write=False)
    return out


def dev(torch, a):
    """A dense device copy that starts on an allocation boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    assert t.data_ptr() % 16 == 0
    return t


def shifted(torch, t):
    """The same values in a view that starts one element into its storage: 4 bytes off for float, 2 for half."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % (8 if t.element_size() == 2 else 16) != 0 and v.is_contiguous()
    return v


def reaches(name, aligned=True, nitems=1):
    dtype, shape, cfg = ce.CASES[name][:3]
    return ce.selected_kernel(*shape, cfg[0], nitems=nitems, aligned=aligned, half=dtype == np.float16,
                              k=cfg[1], md=cfg[2], s1=cfg[3], s2=cfg[4])


def assert_same(got, want, what):
    got = got if isinstance(got, np.ndarray) else got.cpu().numpy()
    assert ce.same_bits_nan_aware(got, want), (what, ce.describe_difference(got, want))


# ------------------------------------------------------------------ 1, 2: every float kernel, dense and shifted

@pytest.mark.parametrize("name", ["flat", "rows2", "rows", "k1", "quad", "generic"])
def test_float_kernel_on_planted_values(torch_mod, cabi, name):  # noqa: F811
    torch = torch_mod
    _, shape, cfg, dense, offset = ce.CASES[name]
    assert reaches(name) == dense and reaches(name, aligned=False) == offset
    f1, f2, _, _ = inputs(name)
    want = oracle_result(name)
    assert np.isnan(want).any() and np.isinf(want).any()
    a1, a2 = dev(torch, f1), dev(torch, f2)
    out = cabi.correlation_forward(a1, a2, *cfg)
    assert_same(out, want, dense)
    # one element off the boundary: the kernels without 16-byte staging, the same bits as the aligned ones
    got = cabi.correlation_forward(shifted(torch, a1), shifted(torch, a2), *cfg)
    assert_same(got, want, offset)
    assert_same(got, out.cpu().numpy(), (offset, "against", dense))


# ------------------------------------------------------------------ 3: the pair entry

@pytest.mark.parametrize("name", ["flat", "rows2", "rows", "quad_pad8", "flat_pad2", "flat_pad8"])
def test_pair_entry_on_planted_values(torch_mod, cabi, name):  # noqa: F811
    torch = torch_mod
    _, shape, cfg, dense, _ = ce.CASES[name]
    assert reaches(name, nitems=2) == dense          # (no shape selects differently as a pair: test_corr_edges_host.py)
    f1, f2, _, _ = inputs(name)
    a1, a2 = dev(torch, f1), dev(torch, f2)
    pa, pb = cabi.correlation_forward_pair(a1, a2, a2, a1, *cfg)
    assert_same(pa, oracle_result(name), (dense, "pair, first item"))
    assert_same(pa, cabi.correlation_forward(a1, a2, *cfg).cpu().numpy(), (dense, "pair against single"))
    assert_same(pb, cabi.correlation_forward(a2, a1, *cfg).cpu().numpy(), (dense, "pair against single, swapped"))
    with np.errstate(all="ignore"):
        from oracle import cpu_oracle
        swapped = cpu_oracle.correlation_fwd(f2, f1, *cfg, order=1, fmad=1)
    assert_same(pb, swapped, (dense, "pair, second item"))


# ------------------------------------------------------------------ 4: other output origins

@pytest.mark.parametrize("planted", [False, True], ids=["finite", "planted"])
@pytest.mark.parametrize("name", ce.ORIGIN_CASES)
def test_output_origin(torch_mod, cabi, name, planted):  # noqa: F811
    torch = torch_mod
    _, shape, cfg, dense, offset = ce.CASES[name]
    assert reaches(name) == dense and reaches(name, aligned=False) == offset
    f1, f2, _, _ = inputs(name, planted)
    want = oracle_result(name, planted)
    assert np.isnan(want).any() == planted
    a1, a2 = dev(torch, f1), dev(torch, f2)
    out = cabi.correlation_forward(a1, a2, *cfg)
    if planted:
        assert_same(out, want, dense)
    else:
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), dense
    if dense != offset:
        assert_same(cabi.correlation_forward(shifted(torch, a1), shifted(torch, a2), *cfg), want, offset)


# ------------------------------------------------------------------ 5: the half kernels

@pytest.mark.parametrize("name", sorted(ce.F16_CASES))
def test_half_kernel_on_planted_values(torch_mod, cabi, name):  # noqa: F811
    torch = torch_mod
    _, shape, cfg, dense, offset = ce.CASES[name]
    assert reaches(name) == dense and reaches(name, aligned=False) == offset
    f1, f2, _, _ = inputs(name)
    want = oracle_result(name)
    assert want.dtype == np.float16 and np.isnan(want).any() and np.isinf(want).any()
    a1, a2 = dev(torch, f1), dev(torch, f2)
    out = cabi.correlation_forward(a1, a2, *cfg)
    assert out.dtype == torch.float16
    assert_same(out, want, dense)
    if dense != offset:
        # the tiled kernel against the one-thread-per-output kernel, which the odd-offset view reaches
        got = cabi.correlation_forward(shifted(torch, a1), shifted(torch, a2), *cfg)
        assert_same(got, want, offset)
        assert_same(got, out.cpu().numpy(), (offset, "against", dense))


# ------------------------------------------------------------------ 6: the warp in front of the correlation

@pytest.mark.parametrize("align_corners", [True, False])
def test_warp_and_fused_warp_correlation_on_planted_values(torch_mod, cabi, oracle, align_corners):  # noqa: F811
    """The in-map corner of weight exactly 0 exists with align_corners=True only: there an integer flow lands on a pixel
    centre.  With align_corners=False the source coordinate of pixel x is (x + flow) W / (W - 1) - 0.5, which no
    integer flow makes an integer, so that run has the masked-out pixel and the non-finite corners of non-zero weight,
    and the weight-0 site is required of the align_corners=True run alone."""
    torch = torch_mod
    f1, f2, flo = ce.warp_inputs(align_corners)
    zero_w, masked = ce.warp_zero_weight_sites(f2, flo, align_corners)
    assert masked.any() and (zero_w.any() or not align_corners)
    with np.errstate(all="ignore"):
        want_warp = oracle.pwc_warp(f2, flo, align_corners, fmad=1)
        want = oracle.correlation_fwd(f1, want_warp, *ce.PWC, order=1, fmad=1)
    assert np.isnan(want_warp).any(axis=1)[zero_w | masked].all()
    a1, a2, fl = dev(torch, f1), dev(torch, f2), dev(torch, flo)
    warped = torch.full(f2.shape, 7.0, device="cuda:0")
    assert cabi.pwc_warp_forward(a2, fl, warped, align_corners) == 0
    assert_same(warped, want_warp, "pwc_warp_forward")
    fused = cabi.pwc_warp_correlation_forward(a1, a2, fl, align_corners)
    assert_same(fused, want, "pwc_warp_correlation_forward")
    two = cabi.correlation_forward(a1, warped, *ce.PWC)
    assert ce.selected_kernel(*ce.WARP_SHAPE, 4) == ce.FLAT
    assert_same(fused, two.cpu().numpy(), "fused against warp, then correlation")
