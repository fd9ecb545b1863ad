"""CPU checks of the FilterInterpolate blend backward (vfi_filterinterp_blend_backward).

  * the header declares it, libvfi_hip.so exports it, cabi knows its 27 arguments;
  * NULL inputs and bad sizes return 1 without a GPU; all six outputs NULL returns 0 and launches nothing;
  * the rounding rule of the incoming gradient, g_d = grad_blend * w_d + grad_out_d with the product and the sum rounded
    separately, is what torch float32 autograd accumulates for blend = out0 * w0 + out2 * w2 when out0 / out2 have another
    use (DAIN's `/ 2.0` included);
  * the new kernel instances use no scratch memory.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC_LIB = os.path.join(ROOT, "video-frame-interpolation-based-on-deformable-kernel-region_amd", "lib")


@pytest.fixture(scope="module")
def built():
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import build
    build.build_all()
    return build


def test_header_declares_and_library_exports_blend_backward(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vfi_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+vfi_filterinterp_blend_backward\s*\(([^)]*)\)", text)
    assert m
    lib = ctypes.CDLL(built.LIB_PATH)
    assert hasattr(lib, "vfi_filterinterp_blend_backward")
    from vfidkr_amd import cabi
    assert len(cabi.SIGNATURES["vfi_filterinterp_blend_backward"]) == len(m.group(1).split(",")) == 27


def _call(f, ptrs, dims, outs=None):
    from vfidkr_amd import cabi
    s = cabi.Strides(0, 0, 0)
    p = ctypes.c_void_p(16)           # never dereferenced: every call below returns before any launch
    outs = [p] * 6 if outs is None else outs
    return f(*ptrs, p, p, p, *outs, *dims, 16, 0.5, 0.5, s, s, s, s, None)


def test_blend_backward_argument_errors_return_1_without_a_gpu(built):
    from vfidkr_amd import cabi
    f = cabi.lib().vfi_filterinterp_blend_backward
    p = ctypes.c_void_p(16)
    for i in range(6):                # each of the six inputs NULL
        ptrs = [p] * 6
        ptrs[i] = None
        assert _call(f, ptrs, (1, 3, 8, 8)) == 1
    for dims in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1)):
        assert _call(f, [p] * 6, dims) == 1
    s = cabi.Strides(0, 0, 0)
    assert f(p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, 1, 3, 8, 8, 0, 0.5, 0.5, s, s, s, s, None) == 1
    # all six outputs NULL: nothing to compute, nothing launched (no GPU needed)
    assert _call(f, [p] * 6, (1, 3, 8, 8), outs=[None] * 6) == 0


@pytest.mark.parametrize("w0,w2", [(0.5, 0.5), (0.75, 0.25), (1.0, 0.0), (1.0 - 0.3, 0.3), ("half", "half")])
def test_gradient_rounding_matches_torch_autograd(w0, w2):
    """torch CPU float32: blend = out0 * w0 + out2 * w2 (or DAIN's out0 / 2.0 + out2 / 2.0) with out0 / out2 also used by
    the loss; the gradient reaching out_d equals float32(float32(grad_blend * w_d) + grad_out_d)."""
    gen = torch.Generator().manual_seed(7)
    for trial in range(4):
        shape = (2, 3, 5, 7)
        out0 = (torch.randn(shape, generator=gen) * 10.0 ** (trial - 1)).requires_grad_()
        out2 = torch.randn(shape, generator=gen).requires_grad_()
        gb = torch.randn(shape, generator=gen) * 3.0
        g0 = torch.randn(shape, generator=gen) * 10.0 ** (1 - trial)
        g2 = torch.randn(shape, generator=gen)
        if w0 == "half":
            blend, fw0, fw2 = out0 / 2.0 + out2 / 2.0, 0.5, 0.5
        else:
            blend, fw0, fw2 = out0 * w0 + out2 * w2, w0, w2
        loss = (blend * gb).sum() + (out0 * g0).sum() + (out2 * g2).sum()
        loss.backward()
        f = np.float32
        want0 = (gb.numpy() * f(fw0)).astype(f) + g0.numpy()
        want2 = (gb.numpy() * f(fw2)).astype(f) + g2.numpy()
        assert want0.dtype == f and want2.dtype == f
        assert np.array_equal(out0.grad.numpy(), want0)
        assert np.array_equal(out2.grad.numpy(), want2)


def test_blend_backward_kernels_use_no_scratch(built):
    """the new instances of the blend backward (the staged tile kernel with and without the image gradient, the per-pixel
    kernel) reserve no scratch memory and hold no scratch instruction"""
    text = open(os.path.join(CSRC_LIB, "filterinterp.s")).read()
    names = re.findall(r"^(_Z\S*blend_backward\S*):", text, flags=re.M)
    assert len(names) == 4, names
    for name in names:
        body = text.split(name + ":", 1)[1].split(".Lfunc_end", 1)[0]
        assert not re.search(r"^\s*scratch_", body, flags=re.M), name
        meta = text.split(".amdhsa_kernel " + name, 1)[1].split(".end_amdhsa_kernel", 1)[0]
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", meta), name
