"""ctypes caller of the channels_last (NHWC) image gradient of FilterInterpolation:
vfi_filterinterp_backward_ori_nhwc_image_multi[_bf16] (include/vfi_hip.h, csrc/filterinterp_nhwc_bwd.hip).

The contract is cabi's: a shape, rank or layout the library does not take returns 1, silently; a dtype or device it does not
take raises RuntimeError; both before any library call.  The checks and the stride structures are cabi's own helpers."""
import ctypes

import torch

from . import cabi
from .cabi import (_channels_innermost, _fi_filter_ok, _fi_image_dtype, _finish, _ptr, _same_strides, _st4, _st_nhwc, _stream,
                   lib)


def _checked(flows, filt, gradoutputs, gradinput1):
    """(dtype, suffix) of a legal call, None for a shape or layout the library does not take; raises for dtype / device"""
    n = len(flows)
    if n == 0 or len(gradoutputs) != n or gradinput1 is None or filt is None or \
            any(t is None for t in flows) or any(t is None for t in gradoutputs):
        return None
    if gradinput1.dim() != 4 or filt.dim() != 4 or 0 in gradinput1.shape:
        return None
    b, c, h, w = gradinput1.shape
    if not _channels_innermost(gradinput1) or not _fi_filter_ok(gradinput1, filt) or filt.size(1) < 1:
        return None
    for fl, g in zip(flows, gradoutputs):
        if fl.dim() != 4 or tuple(fl.shape) != (b, 2, h, w) or not _same_strides(fl, flows[0]):
            return None
        if g.dim() != 4 or g.shape != gradinput1.shape or not _channels_innermost(g) or not _same_strides(g, gradoutputs[0]):
            return None
    return _fi_image_dtype((gradinput1, *gradoutputs), (filt, *flows))


def filterinterp_backward_nhwc_image_multi(flows, filt, gradoutputs, gradinput1, direct=False):
    """gradinput1 = the sum over t of the image gradient of FilterInterpolation(., flows[t], filt) for gradoutputs[t], for
    channels_last tensors: cabi.filterinterp_backward_ori_image_multi's result for the same logical tensors, bit for bit.
    Every gradient and gradinput1 have channel stride 1 -- dense channels_last tensors or channel slices of wider ones; the
    gradients share one layout, gradinput1 has its own.  gradinput1 is written in full (no zero fill needed).  The gradients
    and gradinput1 float32, or all bfloat16; flows (one layout) and filter float32, in NCHW or channels_last.
    direct=True: every tile on the per-addend kernel, an internal entry point the tests and tools compare the staged kernel
    with."""
    ok = _checked(flows, filt, gradoutputs, gradinput1)
    if ok is None:
        return 1
    dtype, suffix = ok
    n = len(flows)
    b, c, h, w = gradinput1.shape
    fp = (ctypes.c_void_p * n)(*[fl.data_ptr() for fl in flows])
    gp = (ctypes.c_void_p * n)(*[g.data_ptr() for g in gradoutputs])
    with torch.cuda.device(gradinput1.device):
        fn = getattr(lib(), "vfi_filterinterp_backward_ori_nhwc_image_multi" + suffix + ("_direct" if direct else ""))
        return _finish(fn(fp, _ptr(filt), gp, _ptr(gradinput1), n, b, c, h, w, filt.size(1), _st_nhwc(gradinput1),
                          _st4(flows[0]), _st4(filt), _st_nhwc(gradoutputs[0]), _stream(gradinput1, dtype)))


def filterinterp_nhwc_bwd_access_width(filt, gradoutputs):
    """the width, in elements, of the staged kernel's gradient loads for these gradients (host code, no launch)"""
    if len(gradoutputs) == 0 or any(g is None for g in gradoutputs) or filt.dim() != 4 or \
            not all(g.dim() == 4 and _channels_innermost(g) and _same_strides(g, gradoutputs[0]) for g in gradoutputs):
        raise RuntimeError("filterinterp_nhwc_bwd_access_width: not the gradients of a filterinterp_backward_nhwc_image_multi call")
    cabi._bf16_or_f32(*gradoutputs)
    g0 = gradoutputs[0]
    gp = (ctypes.c_void_p * len(gradoutputs))(*[g.data_ptr() for g in gradoutputs])
    b, _, h, w = g0.shape
    return lib().vfi_filterinterp_nhwc_bwd_access_width(g0.element_size(), gp, len(gradoutputs), b, h, w, filt.size(1), _st_nhwc(g0))
