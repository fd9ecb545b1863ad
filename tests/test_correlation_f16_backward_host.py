"""CPU checks of the half-precision correlation backward (the reference's at::Half instantiation).

  * the numpy restatement (tests/corr_half_backward.py) agrees with the float32 oracle where every half operation is
    exact, stays within a stated bound of a float64 evaluation, and accumulates in half (a hand-worked case);
  * libvfi_hip.so declares and exports vfi_correlation_backward_f16; argument errors return 1 before any launch;
  * the new kernels' gfx950 assembly has no fused or mixed-precision f16 instruction and no scratch.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.corr_half_backward import correlation_bwd_half, out_dims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video-frame-interpolation-based-on-deformable-kernel-region_amd")

# (C, H, W, pad, k, md, s2): k 1 with PWC-Net's pad = md = 4 (incl. frames smaller than the halo), pad != md, k 3 / s2 2
SHAPES = ((4, 9, 11, 4, 1, 4, 1), (8, 3, 2, 4, 1, 4, 1), (4, 12, 20, 3, 1, 4, 1), (4, 8, 8, 4, 3, 4, 2), (2, 10, 9, 3, 3, 3, 2))


def _small_ints(rng, shape):
    return rng.integers(-3, 4, shape).astype(np.float16)


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_equals_float_oracle_when_every_half_operation_is_exact(oracle, shape):
    """Small integers: every product and partial sum is an integer below 2048, so half arithmetic is exact and the
    result is the float32 path's rounded to half once; with C*k*k a power of two the mean is exact too."""
    C, H, W, pad, k, md, s2 = shape
    rng = np.random.default_rng(sum(shape))
    f1, f2 = _small_ints(rng, (2, C, H, W)), _small_ints(rng, (2, C, H, W))
    oc, oh, ow = out_dims(H, W, pad, k, md, 1, s2)
    g = _small_ints(rng, (2, oc, oh, ow))
    got = correlation_bwd_half(f1, f2, g, pad, k, md, 1, s2)
    want = oracle.correlation_bwd(f1.astype(np.float32), f2.astype(np.float32), g.astype(np.float32), pad, k, md, 1, s2)
    for a, b in zip(got, want):
        assert a.dtype == np.float16 and a.shape == b.shape
        assert np.array_equal(a.view(np.uint16), b.astype(np.float16).view(np.uint16))
        if (k * k * C) & (k * k * C - 1) == 0:
            assert np.array_equal(a.astype(np.float32), b)
    assert any(np.abs(a).max() > 0 for a in got)


@pytest.mark.parametrize("shape", [(32, 12, 14, 4, 1, 4, 1), (6, 9, 10, 4, 3, 4, 2)])
def test_restatement_within_bound_of_float64(shape):
    """Random data: |half - exact| <= (n + 2) * u * sum|terms| / nelems + (n + 2) * 2^-25, u = 2^-11, n = the roundings
    one gradient element goes through (terms per partial, plus the 32 partial sums); the second term covers the
    subnormal range.  The difference is not zero: the half path rounds."""
    C, H, W, pad, k, md, s2 = shape
    rng = np.random.default_rng(7)
    f1 = rng.standard_normal((1, C, H, W)).astype(np.float16)
    f2 = rng.standard_normal((1, C, H, W)).astype(np.float16)
    oc, oh, ow = out_dims(H, W, pad, k, md, 1, s2)
    g = rng.standard_normal((1, oc, oh, ow)).astype(np.float16)
    half = correlation_bwd_half(f1, f2, g, pad, k, md, 1, s2)
    exact = correlation_bwd_half(f1, f2, g, pad, k, md, 1, s2, dtype=np.float64)
    mag = correlation_bwd_half(np.abs(f1), np.abs(f2), np.abs(g), pad, k, md, 1, s2, dtype=np.float64)
    n = -(-oc // 32) * k * k + 32
    u = 2.0 ** -11
    for h_, e, m in zip(half, exact, mag):
        err = np.abs(h_.astype(np.float64) - e)
        bound = (n + 2) * u * m + (n + 2) * 2.0 ** -25
        assert (err <= bound).all(), float((err / bound).max())
        assert err.max() > 0


def test_restatement_accumulates_in_half():
    """Partial 0 of gradInput1 at pixel (4, 4) receives tc = 0 (2048 * 1), tc = 32 (1 * 1) and tc = 64 (1 * 1).  In half,
    2048 + 1 = 2049 is not representable and rounds to even, 2048, twice: the result is 2048.  A float accumulator would
    reach 2050, which is a half."""
    H = W = 9
    f1 = np.zeros((1, 1, H, W), np.float16)
    f2 = np.zeros((1, 1, H, W), np.float16)
    g = np.zeros((1, 81, H, W), np.float16)
    # pad = md = 4, k 1: gradInput1[y, x] = sum_tc g[tc, y, x] * f2[y + tc // 9 - 4, x + tc % 9 - 4]
    f2[0, 0, 0, 0] = 2048.0           # tc = 0 at (4, 4)
    f2[0, 0, 3, 5] = 1.0              # tc = 32: (3, 5)
    f2[0, 0, 7, 1] = 1.0              # tc = 64: (7, 1)
    g[0, [0, 32, 64], 4, 4] = 1.0
    g1, _ = correlation_bwd_half(f1, f2, g, 4, 1, 4, 1, 1)
    assert g1[0, 0, 4, 4] == np.float16(2048.0)
    exact = correlation_bwd_half(f1, f2, g, 4, 1, 4, 1, 1, dtype=np.float64)[0]
    assert exact[0, 0, 4, 4] == 2050.0 and np.float16(2050.0) == 2050.0


def test_restatement_rounds_nelems_to_half():
    """k*k*C = 2049 is not a half: nelems = half(2049) = 2048, so a sum of 2048 gives exactly 1."""
    C = 2049
    f1 = np.zeros((1, C, 1, 1), np.float16)
    f2 = np.ones((1, C, 1, 1), np.float16)
    g = np.zeros((1, 81, 1, 1), np.float16)
    g[0, 40] = 2048.0                 # tc = 40: zero displacement
    g1, g2 = correlation_bwd_half(f1, f2, g, 4, 1, 4, 1, 1)
    assert (g1 == np.float16(1.0)).all() and (g2 == 0).all()
    assert np.float16(2049) == np.float16(2048)


# ------------------------------------------------------------------ the C ABI

@pytest.fixture(scope="module")
def built():
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import build
    build.build_all()
    return build


def test_header_declares_and_library_exports_backward_f16(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vfi_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+vfi_correlation_backward_f16\s*\(", text)
    lib = ctypes.CDLL(built.LIB_PATH)
    assert hasattr(lib, "vfi_correlation_backward_f16")
    from vfidkr_amd import cabi
    assert "vfi_correlation_backward_f16" in cabi.SIGNATURES


def test_backward_f16_argument_errors_return_1_without_a_gpu(built):
    from vfidkr_amd import cabi
    f = cabi.lib().vfi_correlation_backward_f16
    p = ctypes.c_void_p(16)           # never dereferenced: every call below fails validation first
    assert f(None, None, None, None, None, 1, 1, 8, 8, 4, 1, 4, 1, 1, None) == 1
    assert f(p, p, p, p, None, 1, 1, 8, 8, 4, 1, 4, 1, 1, None) == 1
    assert f(p, p, p, p, p, 1, 1, 8, 8, 4, 1, 4, 2, 1, None) == 1           # stride1 = 2 is undefined in the reference
    assert f(p, p, p, p, p, 0, 1, 8, 8, 4, 1, 4, 1, 1, None) == 1           # empty batch
    assert f(p, p, p, p, p, 1, 1, 2, 2, 0, 1, 4, 1, 1, None) == 1           # no output pixel
    assert f(p, p, p, p, p, 1, 1, 8, 8, 4, 0, 4, 1, 1, None) == 1           # kernel_size 0


# ------------------------------------------------------------------ the device code

FORBIDDEN = ("v_fma_f16", "v_pk_fma_f16", "v_fmac_f16", "v_fma_mix", "v_mad_mix", "scratch_")


def _makefile_flags():
    text = open(os.path.join(PKG, "csrc", "Makefile")).read()
    flags = re.search(r"^HIPFLAGS\s*\?=\s*(.*)$", text, flags=re.M).group(1)
    return flags.replace("$(ARCH)", "gfx950").split()


def test_half_backward_kernels_are_unfused_and_spill_free(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "correlation.s"
    subprocess.run([hipcc] + _makefile_flags() + ["-S", "--cuda-device-only", os.path.join(PKG, "csrc", "correlation.hip"),
                                                  "-o", str(out)], check=True, cwd=os.path.join(PKG, "csrc"))
    asm = out.read_text()
    bodies = re.findall(r"^(_Z\w*corr_backward(?:_k1)?_f16\w*):[^\n]*\n(.*?)^\.Lfunc_end", asm, flags=re.S | re.M)
    names = sorted(n for n, _ in bodies)
    assert len(names) == 4, names                   # corr_backward_f16<false/true>, corr_backward_k1_f16<false/true>
    for name, body in bodies:
        for op in FORBIDDEN:
            assert op not in body, (name, op)
        assert "v_mul_f16" in body or "v_pk_mul_f16" in body, name
        assert "v_add_f16" in body or "v_pk_add_f16" in body, name
    tiled = [b for n, b in bodies if "k1_f16" in n]
    assert all("v_pk_mul_f16" in b and "v_pk_add_f16" in b for b in tiled)
