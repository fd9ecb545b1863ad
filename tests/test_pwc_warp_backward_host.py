"""CPU checks of the PWC-Net warp backward.

  * the numpy restatement (tests/pwc_warp_backward.py) agrees with torch autograd of the reference's warp() formula in
    float64 on CPU, both align_corners, over seeded random shapes and the flow families;
  * on flows whose float32 coordinates are exact, its float32 decisions give the float64 (and torch) gradients;
  * libvfi_hip.so declares and exports vfi_pwc_warp_backward, cabi knows its 16 arguments, argument errors return 1.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.pwc_warp_backward import FLOW_KINDS, decisions, flow_family, pwc_warp_bwd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_warp(x, flo, align_corners):
    """the reference's PWCDCNet.warp written out (PWCNet/PWCNet.py:167-199), in x's dtype"""
    B, C, H, W = x.size()
    xx = torch.arange(0, W).view(1, -1).repeat(H, 1)
    yy = torch.arange(0, H).view(-1, 1).repeat(1, W)
    xx = xx.view(1, 1, H, W).repeat(B, 1, 1, 1)
    yy = yy.view(1, 1, H, W).repeat(B, 1, 1, 1)
    grid = torch.cat((xx, yy), 1).to(x.dtype).to(x.device)
    vgrid = grid + flo
    vgrid[:, 0, :, :] = 2.0 * vgrid[:, 0, :, :].clone() / max(W - 1, 1) - 1.0
    vgrid[:, 1, :, :] = 2.0 * vgrid[:, 1, :, :].clone() / max(H - 1, 1) - 1.0
    vgrid = vgrid.permute(0, 2, 3, 1)
    output = torch.nn.functional.grid_sample(x, vgrid, align_corners=align_corners)
    mask = torch.ones(x.size(), dtype=x.dtype, device=x.device)
    mask = torch.nn.functional.grid_sample(mask, vgrid, align_corners=align_corners)
    mask[mask < 0.9999] = 0
    mask[mask > 0] = 1
    return output * mask


def torch_grads(x, flo, g, align_corners, dtype=torch.float64, device="cpu"):
    xt = torch.tensor(x, dtype=dtype, device=device, requires_grad=True)
    ft = torch.tensor(flo, dtype=dtype, device=device, requires_grad=True)
    torch_warp(xt, ft, align_corners).backward(torch.tensor(g, dtype=dtype, device=device))
    return xt.grad.cpu().numpy(), ft.grad.cpu().numpy()


def _cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        B, C = int(rng.integers(1, 3)), int(rng.integers(1, 6))
        h, w = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        if i % 10 == 3:
            h = 1
        if i % 10 == 7:
            w = 1
        out.append((B, C, h, w, FLOW_KINDS[i % len(FLOW_KINDS)], bool(i % 2), int(rng.integers(1 << 30))))
    return out


CASES = _cases(30, 20261015)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%dC%d_%dx%d_%s_ac%d" % (c[:5] + (int(c[5]),)))
def test_restatement_equals_torch_autograd_in_float64(case):
    B, C, h, w, kind, ac, seed = case
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, C, h, w))
    flo = flow_family(rng, kind, B, h, w).astype(np.float64)
    g = rng.normal(size=(B, C, h, w))
    gx, gf, A, S, _ = pwc_warp_bwd(x, flo, g, ac, decide=np.float64)
    tx, tf = torch_grads(x, flo, g, ac)
    assert np.all(np.abs(gx - tx) <= 1e-12 * A + 1e-300), np.abs(gx - tx).max()
    assert np.all(np.abs(gf - tf) <= 1e-12 * S + 1e-300), np.abs(gf - tf).max()


# h - 1 and w - 1 powers of two (or 0) and dyadic flows: every float32 coordinate is exact, so the float32 decisions
# and weights are the float64 ones
EXACT = [(h, w, kind, ac) for (h, w) in ((1, 1), (2, 3), (5, 9), (3, 17), (9, 5), (17, 2))
         for kind in ("zero", "int", "dyadic", "border") for ac in (True, False)]


@pytest.mark.parametrize("case", EXACT, ids=lambda c: "%dx%d_%s_ac%d" % (c[0], c[1], c[2], int(c[3])))
def test_float32_decisions_equal_float64_on_exact_coordinates(case):
    h, w, kind, ac = case
    rng = np.random.default_rng(h * 100 + w)
    B, C = 2, 3
    x = rng.normal(size=(B, C, h, w)).astype(np.float32)
    flo = flow_family(rng, kind, B, h, w)
    if kind == "border":
        flo = np.round(flo * 16) / 16
    flo = flo.astype(np.float32)
    assert (decisions(flo, h, w, ac, np.float32) == decisions(flo, h, w, ac, np.float64)).all()
    g = rng.normal(size=(B, C, h, w)).astype(np.float32)
    a = pwc_warp_bwd(x, flo, g, ac, decide=np.float32)
    b = pwc_warp_bwd(x, flo, g, ac, decide=np.float64)
    assert np.all(np.abs(a[0] - b[0]) <= 1e-12 * a[2] + 1e-300)
    assert np.all(np.abs(a[1] - b[1]) <= 1e-12 * a[3] + 1e-300)
    tx, tf = torch_grads(x.astype(np.float64), flo.astype(np.float64), g.astype(np.float64), ac)
    assert np.all(np.abs(a[0] - tx) <= 1e-12 * a[2] + 1e-300)
    assert np.all(np.abs(a[1] - tf) <= 1e-12 * a[3] + 1e-300)


def test_zero_flow_one_sided_derivative_at_the_last_column():
    """a sample exactly on the last column: its ne corner is outside the map and reads 0 (ATen)"""
    x = np.arange(12, dtype=np.float32).reshape(1, 1, 3, 4)
    g = np.ones_like(x)
    _, gf, _, _, mask = pwc_warp_bwd(x, np.zeros((1, 2, 3, 4), np.float32), g, True)
    assert (mask == 1).all()
    assert np.allclose(gf[0, 0, :, :3], 1.0) and np.allclose(gf[0, 0, :, 3], -x[0, 0, :, 3])
    tx, tf = torch_grads(x.astype(np.float64), np.zeros((1, 2, 3, 4)), g.astype(np.float64), True)
    assert np.allclose(tf, gf)


# ------------------------------------------------------------------ the C ABI

@pytest.fixture(scope="module")
def built():
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import build
    build.build_all()
    return build


def test_header_declares_and_library_exports_pwc_warp_backward(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vfi_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+vfi_pwc_warp_backward\s*\(", text)
    lib = ctypes.CDLL(built.LIB_PATH)
    assert hasattr(lib, "vfi_pwc_warp_backward")
    from vfidkr_amd import cabi
    assert len(cabi.SIGNATURES["vfi_pwc_warp_backward"]) == 16


def test_pwc_warp_backward_argument_errors_return_1_without_a_gpu(built):
    from vfidkr_amd import cabi
    f = cabi.lib().vfi_pwc_warp_backward
    p = ctypes.c_void_p(16)           # never dereferenced: every call below fails validation first
    s = cabi.Strides(0, 0, 0)
    assert f(None, p, p, p, p, 1, 1, 8, 8, 1, s, s, s, s, s, None) == 1
    assert f(p, None, p, p, p, 1, 1, 8, 8, 1, s, s, s, s, s, None) == 1
    assert f(p, p, None, p, p, 1, 1, 8, 8, 1, s, s, s, s, s, None) == 1
    assert f(p, p, p, p, p, 0, 1, 8, 8, 1, s, s, s, s, s, None) == 1
    assert f(p, p, p, p, p, 1, 0, 8, 8, 1, s, s, s, s, s, None) == 1
    assert f(p, p, p, p, p, 1, 1, 0, 8, 1, s, s, s, s, s, None) == 1
    assert f(p, p, p, p, p, 1, 1, 8, -1, 1, s, s, s, s, s, None) == 1
