"""Host helpers of the fused correlation + LeakyReLU tests (tests/test_corr_lrelu_host.py, tests/test_gpu_corr_lrelu.py):

  expected_forward(f1, f2, cfg, slope)          torch's leaky_relu, on the CPU, of the oracle's correlation forward
  masked(y, g, slope)                           torch.where(y > 0, g, g * slope): what the backward feeds the correlation
  expected_backward(f1, f2, y, g, cfg, slope)   the oracle's correlation backward fed masked(y, g, slope)
  forward_inputs(name, planted)                 a case of tests/corr_edges.py; the normal ones with an all-zero pixel
  selected_kernel_out(..., out_bits)            tests.corr_edges.selected_kernel for an output pointer / batch stride
  backward_groups(tiles, batch, channel)        the host's split of the channels into groups (corr_backward_groups)
  corr64(x1, x2)                                PWC-Net's correlation restated in torch, float64, differentiable

Comparison is bit for bit with equal NaN positions (tests.corr_edges.same_bits_nan_aware)."""
import functools

import numpy as np
import torch

from tests import corr_edges as ce

SLOPE = 0.1
CAT = 90                                    # channels of the concatenation buffers the tests write into / slice gradients from


def _oracle():
    from oracle import cpu_oracle
    cpu_oracle.build()
    return cpu_oracle


def leaky(x, slope):
    return torch.nn.functional.leaky_relu(torch.from_numpy(np.ascontiguousarray(x)), slope).numpy()


def expected_forward(f1, f2, cfg, slope=SLOPE):
    with np.errstate(all="ignore"):
        return leaky(_oracle().correlation_fwd(f1, f2, *cfg, order=1, fmad=1), slope)


def masked(y, g, slope=SLOPE):
    y, g = torch.from_numpy(np.ascontiguousarray(y)), torch.from_numpy(np.ascontiguousarray(g))
    return torch.where(y > 0, g, g * torch.tensor(slope, dtype=torch.float32)).numpy()


def expected_backward(f1, f2, y, g, cfg, slope=SLOPE):
    with np.errstate(all="ignore"):
        return _oracle().correlation_bwd(f1, f2, masked(y, g, slope), *cfg)


# ------------------------------------------------------------------ forward cases

FORWARD_CASES = tuple(ce.F32_CASES)


@functools.lru_cache(maxsize=None)
def forward_inputs(name, planted):
    """f1, f2, cfg of a float case.  Normal values: one pixel (one kernel patch) of the first map is zero in every channel, so its outputs
    are exact zeros (+0) and go through the `> 0` test."""
    f1, f2, _, cfg = ce.case_inputs(name, planted)
    if not planted:
        f1 = f1.copy()
        kr, y, x = (cfg[1] - 1) // 2, f1.shape[2] // 2, f1.shape[3] // 2
        f1[0, :, y - kr:y + kr + 1, x - kr:x + kr + 1] = 0     # (kernel_size 3: the 3 x 3 patch of one output pixel)
    for a in (f1, f2):
        a.setflags(write=False)
    return f1, f2, cfg


@functools.lru_cache(maxsize=None)
def forward_expected(name, planted, slope=SLOPE, swapped=False):
    """computed once and shared; read-only"""
    f1, f2, cfg = forward_inputs(name, planted)
    out = expected_forward(f2, f1, cfg, slope) if swapped else expected_forward(f1, f2, cfg, slope)
    out.setflags(write=False)
    return out


def selected_kernel_out(B, C, H, W, pad, nitems=1, out_bits=0, **kw):
    """The forward kernel a float call reaches when its inputs are 16-byte aligned and `out_bits` is the OR of the output
    pointers and, for the fused entries, the outputs' batch strides in bytes -- correlation_forward_items counts a stride
    that breaks a store's alignment exactly as it counts a misaligned pointer.  8-byte stores (two pixels per lane) need
    out_bits & 7 == 0, 16-byte stores (four per lane) out_bits & 15 == 0."""
    if out_bits & 7:
        return ce.selected_kernel(B, C, H, W, pad, nitems=nitems, aligned=False, **kw)
    k = ce.selected_kernel(B, C, H, W, pad, nitems=nitems, aligned=True, **kw)
    return ce.ROWS2 if k == ce.QUAD and out_bits & 15 else k


def slice_bits(shape, cfg, first_channel, channels=CAT):
    """out_bits of the view buf[:, first_channel:first_channel + oc] of a 16-byte-aligned (B, channels, oh, ow) buffer"""
    _, oh, ow = ce.out_dims(shape[2], shape[3], *cfg)
    return (first_channel * oh * ow * 4) | (channels * oh * ow * 4)


# ------------------------------------------------------------------ backward cases

def backward_groups(tiles, batch, channel):
    """(groups, channels per group) of corr_backward_groups in correlation.hip"""
    groups = min(channel, max(1, (2048 + tiles * batch - 1) // (tiles * batch)))
    per = (channel + groups - 1) // groups
    return (channel + per - 1) // per, per


def tiles_of(shape):
    return ((shape[3] + 63) // 64) * ((shape[2] + 3) // 4)


# name -> ((B, C, H, W), (pad, k, md, s1, s2)): 64 x 4 tiles, ragged on the right and at the bottom in both tiled shapes
BACKWARD_CASES = {
    "one_channel_per_group": ((2, 7, 5, 65), ce.PWC),
    "several_channels_per_group": ((2, 53, 30, 130), ce.PWC),
    "generic": ((2, 5, 9, 20), (3, 3, 4, 1, 2)),
}


@functools.lru_cache(maxsize=None)
def backward_inputs(name, planted=False):
    """(a1, a2, ya, ga, b1, b2, yb, gb, cfg): two items; y is the activated forward of its item, g normal values -- with
    planted: +-inf and NaN at a few positions on and next to the border."""
    shape, cfg = BACKWARD_CASES[name]
    rng = np.random.default_rng([ce.SEED, 7, sorted(BACKWARD_CASES).index(name)])
    a1, a2, b1, b2 = (rng.standard_normal(shape).astype(np.float32) for _ in range(4))
    ya, yb = expected_forward(a1, a2, cfg), expected_forward(b1, b2, cfg)
    ga, gb = (rng.standard_normal(ya.shape).astype(np.float32) for _ in range(2))
    if planted:
        oh, ow = ya.shape[2:]
        spots = [(0, 0), (0, 1), (1, 1), (oh - 1, ow - 1), (oh - 2, ow - 2), (oh - 1, 0), (oh // 2, ow - 1), (1, ow - 2)]
        for k, g in enumerate((ga, gb)):
            for j, (y, x) in enumerate(spots):
                g[j % 2, (7 * j + 3 * k) % g.shape[1], y, x] = (np.inf, -np.inf, np.nan)[(j + k) % 3]
    out = (a1, a2, ya, ga, b1, b2, yb, gb)
    for a in out:
        a.setflags(write=False)
    return out + (cfg,)


@functools.lru_cache(maxsize=None)
def backward_expected(name, planted=False):
    a1, a2, ya, ga, b1, b2, yb, gb, cfg = backward_inputs(name, planted)
    out = expected_backward(a1, a2, ya, ga, cfg) + expected_backward(b1, b2, yb, gb, cfg)
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------ float64 restatement

def corr64(x1, x2, pad=4, md=4):
    """PWC-Net's correlation (kernel 1, strides 1) in torch, float64: mean over the channels of x1 * shifted x2."""
    B, C, H, W = x1.shape
    p2 = torch.nn.functional.pad(x2.double(), (pad, pad, pad, pad))
    x1 = x1.double()
    org = md - pad
    oh, ow = H + 2 * pad - 2 * md, W + 2 * pad - 2 * md
    p1 = torch.nn.functional.pad(x1, (pad, pad, pad, pad))
    c1 = p1[:, :, md:md + oh, md:md + ow]
    assert org + pad == md
    planes = []
    for tj in range(-md, md + 1):
        for ti in range(-md, md + 1):
            planes.append((c1 * p2[:, :, md + tj:md + tj + oh, md + ti:md + ti + ow]).sum(1) / C)
    return torch.stack(planes, 1)
