"""CPU checks of the bfloat16 correlation (vfi_correlation_forward_bf16 / _backward_bf16):

  * the header declares both entries with the `_f16` argument lists, the library exports them, cabi's table holds them;
  * argument errors return 1 before any launch; the shim source admits kBFloat16 in forward and backward;
  * the helper's bound and exactness claims (tests/corr_bf16.py) hold for a CPU float32 simulation;
  * the dispatch mirror is pinned to the source text;
  * cabi refuses a bfloat16 / float32 mix and CPU tensors before any library call (library stubbed);
  * the MFMA kernel's gfx950 assembly: the matrix-core and the rounding-convert instruction, no scratch.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import corr_bf16 as cb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video-frame-interpolation-based-on-deformable-kernel-region_amd")


@pytest.fixture(scope="module")
def built():
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import build
    build.build_all()
    return build


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vfi_hip.h")).read(), flags=re.S)


def _args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, _header())
    assert m, name
    # the types, names dropped: `const void* input1_half` and `const void* input1` are the same argument
    return [re.sub(r"\s*\w+$", "", " ".join(a.split())) for a in m.group(1).split(",")]


def test_header_declares_both_entries_with_the_f16_argument_lists(built):
    assert _args("vfi_correlation_forward_bf16") == _args("vfi_correlation_forward_f16")
    assert _args("vfi_correlation_backward_bf16") == _args("vfi_correlation_backward_f16")
    lib = ctypes.CDLL(built.LIB_PATH)
    assert hasattr(lib, "vfi_correlation_forward_bf16") and hasattr(lib, "vfi_correlation_backward_bf16")
    text = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "correlation_bf16.hip" in re.search(r"^SRCS\s*:=\s*(.*)$", text, flags=re.M).group(1).split()


def test_cabi_table_matches_the_header(built):
    from vfidkr_amd import cabi
    for dt in ("forward", "backward"):
        assert cabi.SIGNATURES["vfi_correlation_%s_bf16" % dt] == cabi.SIGNATURES["vfi_correlation_%s_f16" % dt]
        assert len(cabi.SIGNATURES["vfi_correlation_%s_bf16" % dt]) == len(_args("vfi_correlation_%s_bf16" % dt))
    assert "vfi_correlation_forward_bf16_kernel" in cabi.INTERNAL_SIGNATURES
    assert "vfi_correlation_forward_bf16_kernel" not in _header()


def test_argument_errors_return_1_without_a_gpu(built):
    from vfidkr_amd import cabi
    fwd, bwd, one = (cabi.lib().vfi_correlation_forward_bf16, cabi.lib().vfi_correlation_backward_bf16,
                     cabi.lib().vfi_correlation_forward_bf16_kernel)
    p = ctypes.c_void_p(16)           # never dereferenced: every call below fails validation first
    E = 1
    assert fwd(None, p, p, 1, 4, 8, 8, 4, 1, 4, 1, 1, None) == E and fwd(p, p, None, 1, 4, 8, 8, 4, 1, 4, 1, 1, None) == E
    assert fwd(p, p, p, 0, 4, 8, 8, 4, 1, 4, 1, 1, None) == E and fwd(p, p, p, 1, 0, 8, 8, 4, 1, 4, 1, 1, None) == E
    assert fwd(p, p, p, 1, 4, 8, 8, 4, 0, 4, 1, 1, None) == E and fwd(p, p, p, 1, 4, 2, 2, 0, 1, 4, 1, 1, None) == E
    assert bwd(p, p, p, p, None, 1, 4, 8, 8, 4, 1, 4, 1, 1, None) == E
    assert bwd(p, p, p, p, p, 1, 4, 8, 8, 4, 1, 4, 2, 1, None) == E                      # stride1 != 1
    assert bwd(p, p, p, p, p, 1, 4, 8, 8, 4, 1, 4, 1, 0, None) == E
    assert one(0, p, p, p, 1, 4, 8, 8, 4, 3, 4, 1, 1, None) == E                         # the MFMA kernel: PWC-Net's configuration only
    assert one(0, p, p, p, 1, 4, 8, 8, 4, 1, 4, 1, 2, None) == E
    assert one(7, p, p, p, 1, 4, 8, 8, 4, 1, 4, 1, 1, None) == E and one(1, None, p, p, 1, 4, 8, 8, 4, 1, 4, 1, 1, None) == E


def test_shim_source_admits_bfloat16_in_forward_and_backward():
    text = open(os.path.join(PKG, "csrc", "shim", "vfi_torch_shim.cpp")).read()
    for fn, entry in (("correlation_forward", "vfi_correlation_forward_bf16"), ("correlation_backward", "vfi_correlation_backward_bf16")):
        body = text[text.index("int %s(at::Tensor& input1" % fn):]
        body = body[:body.index("\n}\n")]
        assert "at::kBFloat16" in body and entry in body and entry.replace("_bf16", "_f16") in body
        assert "scalar_type() == dt" in body                                             # every tensor has the first one's dtype
    assert re.search(r"allow_half && \(t\.scalar_type\(\) == at::kHalf \|\| t\.scalar_type\(\) == at::kBFloat16\)", text)


# ------------------------------------------------------------------ the helper's claims

def test_bf16_rounding_is_nearest_even():
    f32 = lambda b: np.array([b], np.uint32).view(np.float32)
    assert cb.bits(f32(0x3F808000))[0] == 0x3F80                # a tie: to the even pattern below ...
    assert cb.bits(f32(0x3F818000))[0] == 0x3F82                # ... and above
    assert cb.bits(f32(0x3F808001))[0] == 0x3F81 and cb.bits(f32(0x3F807FFF))[0] == 0x3F80
    x = np.array([1.0, -2.5, 3.0e38, np.inf], np.float32)
    assert np.array_equal(cb.from_bits(cb.bits(x))[[0, 1, 3]], x[[0, 1, 3]])


@pytest.mark.parametrize("C", [1, 33, 196])
def test_bound_holds_for_a_float32_accumulation_in_chunks_of_32(C):
    """N(0, 1) data: a float32 accumulation in 32-channel chunks stays inside the bound, and nearly every output is
    bf16_rne(R) bit for bit (the reference alone: all of them)."""
    rng = np.random.default_rng(C)
    shape = (1, C, 6, 19)
    f1, f2 = cb.to_bf16(rng.standard_normal(shape)), cb.to_bf16(rng.standard_normal(shape))
    for order in (None, list(range(31, -1, -1)), [(5 * i + 3) % 32 for i in range(32)]):
        assert cb.check_mfma_result(cb.simulate_fp32(f1, f2, order=order), f1, f2) >= 0.999
    R, _ = cb.reference(f1, f2)
    assert cb.check_mfma_result(cb.bits(R), f1, f2) == 1.0


def test_a_truncating_convert_and_a_slipped_diagonal_fail_the_checks():
    rng = np.random.default_rng(2)
    shape = (1, 32, 6, 19)
    f1, f2 = cb.to_bf16(rng.standard_normal(shape)), cb.to_bf16(rng.standard_normal(shape))
    R, _ = cb.reference(f1, f2)
    trunc = (R.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    assert 0.3 < (trunc == cb.bits(R)).mean() < 0.9                                   # far below the 99 % the check asks for
    with pytest.raises(AssertionError):
        cb.check_mfma_result(trunc, f1, f2)
    slipped = cb.bits(np.roll(R.reshape(1, 9, 9, 6, 19), 1, axis=2).reshape(R.shape))
    with pytest.raises(AssertionError):
        cb.check_mfma_result(slipped, f1, f2)


@pytest.mark.parametrize("C", [16, 32, 64])
def test_integer_inputs_are_exact_in_any_order(C):
    rng = np.random.default_rng(C)
    f1, f2 = (rng.integers(-4, 5, (2, C, 7, 21)).astype(np.float32) for _ in range(2))
    R, _ = cb.reference(f1, f2)
    for order in (None, list(range(31, -1, -1))):
        assert np.array_equal(cb.simulate_fp32(f1, f2, order=order), cb.bits(R))


def test_reference_multiplies_the_padding():
    f1, f2 = np.ones((1, 2, 3, 3), np.float32), np.ones((1, 2, 3, 3), np.float32)
    f1[0, 0, 0, 0] = np.inf
    R, A = cb.reference(f1, f2)
    assert np.isnan(R[0, 0, 0, 0]) and np.isnan(A[0, 0, 0, 0])          # tap (-4, -4) of the second map: inf * 0
    assert R[0, 40, 0, 0] == np.inf and R[0, 40, 1, 1] == 1.0


# ------------------------------------------------------------------ the dispatch mirror

def test_dispatch_mirror_is_pinned_to_the_source():
    text = " ".join(cb.source(cb.SRC).split())
    assert "static bool corr_bf16_is_pwc(int kernel_size, int max_displacement, int stride1, int stride2) { " \
           "return kernel_size == 1 && stride1 == 1 && stride2 == 1 && max_displacement == 4; }" in text
    assert "return (int64_t)h * w * 2 * CorrMfma::KC < INT_MAX && batch <= 65535 && (oh + CorrMfma::TH - 1) / CorrMfma::TH <= 65535;" in text
    assert ("if (corr_bf16_is_pwc(kernel_size, max_displacement, stride1, stride2) && corr_bf16_mfma_fits(batch, h, w, oh)) { "
            "const int64_t mfma_tiles = (int64_t)((ow + CorrMfma::TW - 1) / CorrMfma::TW) * ((oh + CorrMfma::TH - 1) / CorrMfma::TH) * batch; "
            "if (mfma_tiles >= corr_bf16_mfma_threshold) { return corr_bf16_launch_mfma<CorrMfma>(") in text
    assert "MT = MT_, TW = 16 * MT, TH = TH_" in text
    c = cb.constants()
    assert c["KC"] == 32 and c["TW"] % 16 == 0 and c["corr_bf16_mfma_threshold"] >= 1
    # either side of the threshold, and what never reaches the MFMA kernel
    t, TW, TH = c["corr_bf16_mfma_threshold"], c["TW"], c["TH"]
    assert cb.selected_kernel(1, 8, TH * t, TW) == "mfma" and cb.selected_kernel(1, 8, TH * t, TW + 1) == "mfma"
    if t > 1:
        assert cb.selected_kernel(1, 8, TH * (t - 1), TW) == "generic"
        assert cb.selected_kernel(t, 8, 1, 1) == "mfma" and cb.selected_kernel(t - 1, 8, TH, TW) == "generic"
    assert cb.selected_kernel(1, 8, 512, 512, (4, 3, 4, 1, 1)) == "generic" and cb.selected_kernel(1, 8, 512, 512, (4, 1, 4, 1, 2)) == "generic"
    assert cb.selected_kernel(1, 8, 512, 512, (3, 1, 3, 1, 1)) == "generic" and cb.selected_kernel(1, 8, 512, 512, (0, 1, 4, 1, 1)) == "mfma"


# ------------------------------------------------------------------ cabi, library stubbed

class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            if name == "vfi_correlation_output_dims":
                args[7]._obj.value, args[8]._obj.value, args[9]._obj.value = 81, args[0], args[1]
            return 0
        return fn


class _FakeCuda:
    """A bfloat16 / float32 CPU tensor that says it lives on the GPU: cabi's dtype and device checks run before any call."""

    def __init__(self, t, is_cuda=True):
        self.t, self.is_cuda = t, is_cuda

    def __getattr__(self, name):
        return getattr(self.t, name)

    def contiguous(self):
        return self


def test_cabi_refuses_mixed_dtypes_and_cpu_tensors_before_any_library_call(monkeypatch):
    import torch
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi
    rec = _Recorder()
    monkeypatch.setattr(cabi, "lib", lambda: rec)
    monkeypatch.setattr(torch, "empty", lambda *a, **k: _FakeCuda(torch.zeros(*a, dtype=k.get("dtype"))))
    monkeypatch.setattr(torch, "empty_like", lambda t, **k: _FakeCuda(torch.zeros(t.shape, dtype=t.dtype)))
    bf = lambda *s: _FakeCuda(torch.zeros(*s, dtype=torch.bfloat16))
    f32 = lambda *s: _FakeCuda(torch.zeros(*s, dtype=torch.float32))
    a, b, g = bf(1, 4, 8, 10), bf(1, 4, 8, 10), bf(1, 81, 8, 10)
    launches = lambda: [c for c in rec.calls if c != "vfi_correlation_output_dims"]
    for call in (lambda: cabi.correlation_forward(a, f32(1, 4, 8, 10), *cb.PWC),
                 lambda: cabi.correlation_backward(a, f32(1, 4, 8, 10), g, *cb.PWC),
                 lambda: cabi.correlation_backward(a, b, f32(1, 81, 8, 10), *cb.PWC),
                 lambda: cabi.correlation_forward(a, _FakeCuda(torch.zeros(1, 4, 8, 10, dtype=torch.float16)), *cb.PWC)):
        with pytest.raises(RuntimeError, match="tensors must be bfloat16"):
            call()
    # a float32 first tensor with a bfloat16 one behind it: the float32 kernel would read past the 2-byte buffer's end
    for call in (lambda: cabi.correlation_forward(f32(1, 4, 8, 10), b, *cb.PWC),
                 lambda: cabi.correlation_backward(f32(1, 4, 8, 10), b, f32(1, 81, 8, 10), *cb.PWC),
                 lambda: cabi.correlation_backward(f32(1, 4, 8, 10), f32(1, 4, 8, 10), g, *cb.PWC)):
        with pytest.raises(RuntimeError, match="tensors must be float32"):
            call()
    for call in (lambda: cabi.correlation_forward(_FakeCuda(a.t, False), _FakeCuda(b.t, False), *cb.PWC),
                 lambda: cabi.correlation_backward(a, b, _FakeCuda(g.t, False), *cb.PWC)):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call()
    assert launches() == []


# ------------------------------------------------------------------ the assembly

def test_mfma_kernel_uses_the_matrix_cores_rounds_with_the_convert_and_has_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    text = open(os.path.join(PKG, "csrc", "Makefile")).read()
    flags = re.search(r"^HIPFLAGS\s*\?=\s*(.*)$", text, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    out = tmp_path / "correlation_bf16.s"
    subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(PKG, "csrc", "correlation_bf16.hip"), "-o", str(out)],
                   check=True, cwd=os.path.join(PKG, "csrc"))
    asm = out.read_text()
    kernels = re.findall(r"^(_ZN3vfi\w+):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", asm, flags=re.M | re.S)
    mfma = [body for name, body in kernels if "corr_forward_k1_mfma_bf16" in name]
    assert mfma and len(kernels) > len(mfma), [n for n, _ in kernels]
    for name, body in kernels:
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), name              # no scratch, no spills
    for body in mfma:
        assert "v_mfma_f32_16x16x32_bf16" in body and "v_cvt_pk_bf16_f32" in body            # round to nearest even, never a shift
