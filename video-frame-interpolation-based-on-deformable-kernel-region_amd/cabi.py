"""ctypes caller of libvfi_hip.so (include/vfi_hip.h) for torch GPU tensors.

Each function is the ctypes twin of one reference binding: it checks its
tensors, then passes raw device pointers, sizes, element strides and torch's
current HIP stream to the C ABI.  No arithmetic happens on this side.  torch is
used for memory and streams only.

The contract of every wrapper (tests/binding_cases.py states it as a table):
a shape, rank or layout the library does not take returns 1, silently, like
`filterinterpolation_cuda.cc:543-583` (a wrapper that allocates and returns
tensors raises RuntimeError); a dtype or device it does not take raises
RuntimeError; both before any library call.  The reference bindings check the
flow's shape and a few strides; the checks here follow what the C entry
addresses: every tensor's shape (`_shaped`, `_is4`), the layout of a tensor the
entry reads or writes with another's strides (`_addressed_as`), and the dtype
and device of all of them (`_on_gpu`).
"""
import ctypes
import math

import torch  # must be imported before libvfi_hip.so so both bind the same libamdhip64.so.7

from . import LIB_PATH

_i = ctypes.c_int
_f = ctypes.c_float
_p = ctypes.c_void_p
_l = ctypes.c_int64


class Strides(ctypes.Structure):
    _fields_ = [("b", ctypes.c_int64), ("c", ctypes.c_int64), ("h", ctypes.c_int64)]


class StridesNhwc(ctypes.Structure):
    """vfi_strides_nhwc: batch, row and pixel strides of a tensor whose channel stride is 1"""
    _fields_ = [("b", ctypes.c_int64), ("h", ctypes.c_int64), ("w", ctypes.c_int64)]


class Strides4(ctypes.Structure):
    """vfi_strides4: all four element strides"""
    _fields_ = [("b", ctypes.c_int64), ("c", ctypes.c_int64), ("h", ctypes.c_int64), ("w", ctypes.c_int64)]


VFI_OK, VFI_ERR_SHAPE, VFI_ERR_LAUNCH = 0, 1, -2
DEFOR_OFFSET, DEFOR_REGION, DEFOR_NOFILTER = 0, 1, 2

# name -> argtypes, exactly the declarations of include/vfi_hip.h
SIGNATURES = {
    "vfi_filterinterp_forward_ori": [_p, _p, _p, _p, _i, _i, _i, _i, _i, Strides, Strides, Strides, _p],
    "vfi_filterinterp_backward_ori": [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, Strides, Strides, Strides, _p],
    "vfi_filterinterp_forward_ori_f16": [_p, _p, _p, _p, _i, _i, _i, _i, _i, Strides, Strides, Strides, _p],
    "vfi_filterinterp_forward_ori_multi": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, Strides, Strides, Strides, _p],
    "vfi_filterinterp_forward_ori_multi_to": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, Strides, Strides, Strides, Strides, _p],
    "vfi_filterinterp_backward_ori_image_multi": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, Strides, Strides, Strides, Strides, _p],
    "vfi_filterinterp_forward_ori_multi_to_bf16": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, Strides, Strides, Strides, Strides, _p],
    "vfi_filterinterp_forward_ori_nhwc_multi_to": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, StridesNhwc, Strides4, Strides4,
                                                   StridesNhwc, _p],
    "vfi_filterinterp_forward_ori_nhwc_multi_to_bf16": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, StridesNhwc, Strides4, Strides4,
                                                        StridesNhwc, _p],
    "vfi_filterinterp_backward_ori_image_multi_bf16": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, Strides, Strides, Strides, Strides,
                                                       _p],
    "vfi_filterinterp_backward_ori_nhwc_image_multi": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, StridesNhwc, Strides4, Strides4,
                                                       StridesNhwc, _p],
    "vfi_filterinterp_backward_ori_nhwc_image_multi_bf16": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, StridesNhwc, Strides4,
                                                            Strides4, StridesNhwc, _p],
    "vfi_filterinterp_forward_defor": [_i, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, Strides, Strides, Strides,
                                       Strides, _p],
    "vfi_filterinterp_backward_defor": [_i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, Strides, Strides,
                                        Strides, Strides, _p],
    "vfi_flowprojection_forward": [_p, _p, _p, _i, _i, _i, _i, Strides, Strides, _p],
    "vfi_flowprojection_forward_batch": [_p, _p, _p, _i, _i, _i, _i, _i, Strides, Strides, _p],
    "vfi_depthflowprojection_forward_batch": [_p, _p, _p, _p, _i, _i, _i, _i, _i, Strides, Strides, Strides, _p],
    "vfi_flowprojection_backward": [_p, _p, _p, _p, _i, _i, _i, Strides, Strides, _p],
    "vfi_projection_reserve": [_i, _i, _i, _p],
    "vfi_release_workspaces": [],
    "vfi_depthflowprojection_forward": [_p, _p, _p, _p, _i, _i, _i, _i, Strides, Strides, Strides, _p],
    "vfi_depthflowprojection_backward": [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, Strides, Strides, Strides, _p],
    "vfi_mindepthflowprojection_forward": [_p, _p, _p, _p, _i, _i, _i, _i, Strides, Strides, Strides, _p],
    "vfi_mindepthflowprojection_backward": [_p, _p, _p, _p, _p, _i, _i, _i, Strides, Strides, Strides, _p],
    "vfi_interpolation_forward": [_p, _p, _p, _i, _i, _i, _i, Strides, Strides, _p],
    "vfi_interpolation_backward": [_p, _p, _p, _p, _p, _i, _i, _i, _i, Strides, Strides, _p],
    "vfi_separableconv_forward": [_p, _p, _p, _p, _i, _i, _i, _i, _i, Strides, Strides, Strides, Strides, _p],
    "vfi_separableconv_backward": [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, Strides, Strides, Strides,
                                   Strides, _p],
    "vfi_separableconvflow_forward": [_p, _p, _p, _i, _i, _i, _i, Strides, Strides, Strides, _p],
    "vfi_separableconvflow_backward": [_p, _p, _p, _p, _p, _i, _i, _i, _i, Strides, Strides, Strides, _p],
    "vfi_correlation_output_dims": [_i, _i, _i, _i, _i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i),
                                    ctypes.POINTER(_i)],
    "vfi_correlation_forward": [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p],
    "vfi_correlation_forward_pair": [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p],
    "vfi_correlation_forward_f16": [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p],
    "vfi_correlation_backward": [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p],
    "vfi_correlation_backward_pair": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p],
    "vfi_correlation_backward_f16": [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p],
    "vfi_correlation_forward_bf16": [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p],
    "vfi_correlation_backward_bf16": [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p],
    "vfi_correlation_lrelu_forward_bf16": [_p, _p, _p, _l, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _p],
    "vfi_correlation_lrelu_backward_bf16": [_p, _p, _p, _l, _p, _l, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _p],
    "vfi_correlation_lrelu_forward": [_p, _p, _p, _l, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _p],
    "vfi_correlation_lrelu_forward_pair": [_p, _p, _p, _l, _p, _p, _p, _l, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _p],
    "vfi_correlation_lrelu_backward": [_p, _p, _p, _l, _p, _l, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _p],
    "vfi_correlation_lrelu_backward_pair": [_p, _p, _p, _l, _p, _l, _p, _p, _p, _p, _p, _l, _p, _l, _p, _p,
                                            _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _p],
    "vfi_correlation_forward_pair_bf16": [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p],
    "vfi_correlation_lrelu_forward_pair_bf16": [_p, _p, _p, _l, _p, _p, _p, _l, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _p],
    "vfi_correlation_backward_pair_bf16": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p],
    "vfi_correlation_lrelu_backward_pair_bf16": [_p, _p, _p, _l, _p, _l, _p, _p, _p, _p, _p, _l, _p, _l, _p, _p,
                                                 _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _p],
    # glue either side of the ops
    "vfi_flow_upsample4": [_p, _p, _i, _i, _i, _i, _f, _f, Strides, Strides, _p],
    "vfi_flowprojection_forward_up4": [_p, _p, _p, _i, _i, _i, _f, _f, _i, Strides, Strides, Strides, _p],
    "vfi_depthflowprojection_forward_up4": [_p, _p, _p, _p, _i, _i, _i, _f, _f, _i, Strides, Strides, Strides, Strides,
                                            _p],
    "vfi_flow_upsample4_backward": [_p, _p, _i, _p, _i, _i, _i, _i, _f, Strides, Strides, _p],
    "vfi_flowprojection_backward_up4": [_p, _p, _p, _p, _i, _p, _i, _i, _i, _f, Strides, Strides, Strides, Strides, _p],
    "vfi_depthflowprojection_backward_up4": [_p, _p, _p, _p, _p, _p, _i, _p, _p, _i, _i, _i, _f, Strides, Strides, Strides,
                                             Strides, Strides, _p],
    "vfi_filterinterp_blend_forward": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _f, Strides, Strides,
                                       Strides, Strides, _p],
    "vfi_filterinterp_blend_backward": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i,
                                        _f, _f, Strides, Strides, Strides, Strides, _p],
    "vfi_rectify_head_forward_bf16": [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _f, Strides, Strides, Strides,
                                      Strides, Strides, _p],
    "vfi_pwc_warp_forward": [_p, _p, _p, _i, _i, _i, _i, _i, Strides, Strides, Strides, _p],
    "vfi_pwc_warp_backward": [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, Strides, Strides, Strides, Strides, Strides, _p],
    "vfi_pwc_warp_forward_bf16": [_p, _p, _i, _p, _i, _i, _i, _i, _i, Strides, Strides, Strides, _p],
    "vfi_pwc_warp_backward_bf16": [_p, _p, _i, _p, _p, _p, _i, _i, _i, _i, _i, Strides, Strides, Strides, Strides, Strides, _p],
    "vfi_pwc_warp_correlation_forward": [_p, _p, _p, _p, _i, _i, _i, _i, _i, Strides, _p],
    "vfi_frame_u8_to_planar": [_p, _p, _i, _i, _i, _i, _i, _i, _i, Strides, _p],
    "vfi_planar_to_frame_u8": [_p, _p, _i, _i, _i, _i, _i, Strides, _p],
    "vfi_frame_error_sums": [_p, _p, ctypes.c_int64, _p, _p],
    "vfi_frame_ssim_sums": [_p, _p, _i, _i, _i, _p, _p],
    # training losses
    "vfi_part_loss_forward": [_p, _i, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, ctypes.c_double, _i, _p, _p, Strides, Strides,
                              Strides, _p],
    "vfi_part_loss_backward": [_p, _i, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, ctypes.c_double, _i, _p, _p, ctypes.c_uint, _p, _p,
                               _p, Strides, Strides, Strides, Strides, Strides, _p],
}
# internal entry points used by the bench / tests to time one code path in isolation
INTERNAL_SIGNATURES = {
    "vfi_filterinterp_forward_ori_direct": [_p, _p, _p, _p, _i, _i, _i, _i, _i, Strides, Strides, Strides, _p],
    "vfi_filterinterp_forward_ori_f16_direct": [_p, _p, _p, _p, _i, _i, _i, _i, _i, Strides, Strides, Strides, _p],
    "vfi_filterinterp_forward_ori_multi_to_bf16_direct": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, Strides, Strides, Strides, Strides,
                                                          _p],
    # (the access width, in elements, the NHWC entries choose for these layouts)
    "vfi_filterinterp_nhwc_access_width": [_i, _p, _p, _i, _i, _i, _i, _i, StridesNhwc, StridesNhwc],
    # (the NHWC image gradient with every tile on the per-addend kernel, and the width of its staged kernel's gradient loads)
    "vfi_filterinterp_backward_ori_nhwc_image_multi_direct": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, StridesNhwc, Strides4,
                                                              Strides4, StridesNhwc, _p],
    "vfi_filterinterp_backward_ori_nhwc_image_multi_bf16_direct": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, StridesNhwc, Strides4,
                                                                   Strides4, StridesNhwc, _p],
    "vfi_filterinterp_nhwc_bwd_access_width": [_i, _p, _i, _i, _i, _i, _i, StridesNhwc],
    "vfi_filterinterp_forward_defor_general": [_i, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, Strides, Strides, Strides,
                                               Strides, _p],
    # (which kernel: 0 the MFMA kernel, 1 the generic kernel)
    "vfi_correlation_forward_bf16_kernel": [_i, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p],
}

_lib = None


def lib():
    """Load libvfi_hip.so; raises OSError if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        l = ctypes.CDLL(LIB_PATH)
        l.vfi_version.restype = ctypes.c_char_p
        l.vfi_version.argtypes = []
        for table in (SIGNATURES, INTERNAL_SIGNATURES):
            for name, argtypes in table.items():
                fn = getattr(l, name)
                fn.restype = _i
                fn.argtypes = argtypes
        _lib = l
    return _lib


def version():
    return lib().vfi_version().decode()


def _st(t):
    return Strides(t.stride(0), t.stride(1), t.stride(2))


def _st_tuple(t):
    return (t.stride(0), t.stride(1), t.stride(2), t.stride(3))


def _st_nhwc(t):
    return StridesNhwc(t.stride(0), t.stride(2), t.stride(3))


def _st4(t):
    return Strides4(*t.stride())


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _dev(t, dtype=torch.float32):
    if not t.is_cuda:
        raise RuntimeError("vfidkr_amd.cabi: tensors must live on the GPU (there is no CPU path)")
    if t.dtype != dtype:
        raise RuntimeError("vfidkr_amd.cabi: tensors must be %s" % str(dtype).replace("torch.", ""))
    return t.device


def _on_gpu(dtype, *tensors):
    """same device and dtype, all of them (None entries: absent optional tensors); the device"""
    device = None
    for t in tensors:
        if t is None:
            continue
        d = _dev(t, dtype)
        if device is None:
            device = d
        elif d != device:
            raise RuntimeError("vfidkr_amd.cabi: tensors must live on one device (%s and %s)" % (device, d))
    return device


def _shaped(t, *shape):
    """shape equals: a tensor of exactly these sizes, none of them zero"""
    return t is not None and t.dim() == len(shape) and tuple(t.shape) == tuple(shape) and 0 not in shape


def _is4(*tensors):
    """NCHW tensors with something in them"""
    return all(t is not None and t.dim() == 4 and 0 not in t.shape for t in tensors)


def _stream(t, dtype=torch.float32):
    return ctypes.c_void_p(torch.cuda.current_stream(_dev(t, dtype)).cuda_stream)


def _finish(err):
    if err == VFI_ERR_LAUNCH:
        raise RuntimeError("CUDA call failed")      # the reference's AT_ERROR text
    return err


# ---------------------------------------------------------------- filterinterpolation_cuda

def _fi_checks(input1, input2, input3, out_like):
    """The reference binding's checks (filterinterpolation_cuda.cc:543-583) and what it leaves to the caller: the flow is
    [B, 2, H, W], the filter one plane of taps per pixel, and out_like -- addressed with input1's strides -- is laid out as
    input1."""
    if not _is4(input1, input2, input3):
        return None
    b, c, h, w = input1.shape
    if not _shaped(input2, b, 2, h, w) or not _fi_filter_ok(input1, input3):
        return None
    if input1.stride(3) != 1 or input2.stride(3) != 1 or input3.stride(3) != 1:
        return None
    if out_like is not None and not _addressed_as(input1, out_like):
        return None
    return b, c, h, w


def filterinterp_forward_ori(input1, input2, input3, output, direct=False):
    dims = _fi_checks(input1, input2, input3, output)
    if dims is None:
        return 1
    b, c, h, w = dims
    with torch.cuda.device(_on_gpu(torch.float32, input1, input2, input3, output)):
        fn = lib().vfi_filterinterp_forward_ori_direct if direct else lib().vfi_filterinterp_forward_ori
        return _finish(fn(_ptr(input1), _ptr(input2), _ptr(input3), _ptr(output), b, c, h, w, input3.size(1),
                          _st(input1), _st(input2), _st(input3), _stream(input1)))


def _fi_image_dtype(images, floats):
    """_bf16_or_f32 over the image-side tensors of a FilterInterpolation call (the image and the outputs, or the gradients):
    all bfloat16 -- the `_bf16` entries -- or all float32; the flows and the filter (`floats`) are float32 either way.
    float16 and every mix raise here, before any library call."""
    dtype, suffix = _bf16_or_f32(*images)
    _on_gpu(torch.float32, *floats)
    if _dev(floats[0]) != images[0].device:
        raise RuntimeError("vfidkr_amd.cabi: tensors must live on one device")
    return dtype, suffix


def filterinterp_forward_ori_multi(input1, flows, input3, outputs):
    """outputs[t] = FilterInterpolation(input1, flows[t], input3): the time offsets of a slow-motion step in one launch.
    input1 and the outputs float32, or all bfloat16 (vfi_filterinterp_forward_ori_multi_to_bf16 with the outputs laid out as
    input1: bf16_rne of the float32 call on the widened image, bit for bit); flows and filter float32 always."""
    n = len(flows)
    if n == 0 or len(outputs) != n or None in flows or None in outputs:
        return 1
    for fl, out in zip(flows, outputs):
        # (layouts compared as _same_strides does: the stride of a size-1 dimension is arbitrary, e.g. after slicing)
        if _fi_checks(input1, fl, input3, out) is None or not _same_strides(fl, flows[0]) or not _same_strides(out, input1):
            return 1
    dtype, suffix = _fi_image_dtype((input1, *outputs), (input3, *flows))
    b, c, h, w = input1.shape
    fp = (ctypes.c_void_p * n)(*[fl.data_ptr() for fl in flows])
    op = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outputs])
    if suffix:
        with torch.cuda.device(input1.device):
            return _finish(lib().vfi_filterinterp_forward_ori_multi_to_bf16(
                _ptr(input1), fp, _ptr(input3), op, n, b, c, h, w, input3.size(1), _st(input1), _st(flows[0]), _st(input3),
                _st(input1), _stream(input1, dtype)))
    with torch.cuda.device(_dev(input1)):
        return _finish(lib().vfi_filterinterp_forward_ori_multi(_ptr(input1), fp, _ptr(input3), op, n, b, c, h, w, input3.size(1),
                                                                _st(input1), _st(flows[0]), _st(input3), _stream(input1)))


def filterinterp_forward_ori_multi_to(input1, flows, input3, outputs, direct=False):
    """filterinterp_forward_ori_multi into destinations with a layout of their own: outputs[t] (input1's shape; typically
    buf_t[:, k:k + C] of a wider contiguous buffer) receives the same bits.  The destinations share one layout with w
    stride 1 and input1's row stride -- anything else is refused here, before the call; batch and channel strides are
    free.  They must not overlap input1 or each other (not checked).  float32, or input1 and every output bfloat16 (a
    bfloat16 destination slice needs 2-byte alignment only); direct=True (bfloat16 only): the one-thread-per-pixel kernel,
    an internal entry point the tests compare the staged kernel with."""
    n = len(flows)
    if n == 0 or len(outputs) != n or None in flows or None in outputs:
        return 1
    for fl, out in zip(flows, outputs):
        if _fi_checks(input1, fl, input3, None) is None or not _same_strides(fl, flows[0]):
            return 1
        if out.dim() != 4 or out.shape != input1.shape or out.stride(3) != 1 or not _same_strides(out, outputs[0]):
            return 1
        # (the row stride of a one-row tensor addresses nothing)
        if input1.size(2) != 1 and out.stride(2) != input1.stride(2):
            return 1
    dtype, suffix = _fi_image_dtype((input1, *outputs), (input3, *flows))
    if direct and not suffix:
        raise RuntimeError("filterinterp_forward_ori_multi_to: direct=True is the bfloat16 kernels' switch")
    b, c, h, w = input1.shape
    so = _st(outputs[0])
    so.h = input1.stride(2)
    fp = (ctypes.c_void_p * n)(*[fl.data_ptr() for fl in flows])
    op = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outputs])
    if suffix:
        with torch.cuda.device(input1.device):
            fn = lib().vfi_filterinterp_forward_ori_multi_to_bf16_direct if direct else lib().vfi_filterinterp_forward_ori_multi_to_bf16
            return _finish(fn(_ptr(input1), fp, _ptr(input3), op, n, b, c, h, w, input3.size(1), _st(input1), _st(flows[0]),
                              _st(input3), so, _stream(input1, dtype)))
    with torch.cuda.device(_dev(input1)):
        return _finish(lib().vfi_filterinterp_forward_ori_multi_to(_ptr(input1), fp, _ptr(input3), op, n, b, c, h, w, input3.size(1),
                                                                   _st(input1), _st(flows[0]), _st(input3), so, _stream(input1)))


def _channels_innermost(t):
    """channel stride 1 (the stride of a one-channel tensor addresses nothing)"""
    return t.size(1) == 1 or t.stride(1) == 1


def filterinterp_forward_nhwc_multi_to(image, flows, filt, outs):
    """filterinterp_forward_ori_multi_to for a channels_last image: outs[t] = FilterInterpolation(image, flows[t], filt), bit
    for bit what the NCHW call writes for the same logical tensors.  image and every output have channel stride 1: a dense
    channels_last tensor or a channel slice of a wider one; the outputs share one layout of their own, all strides free.
    image and outputs float32, or all bfloat16; flows (one layout) and filter float32, in NCHW or channels_last.  Forward only.
    A shape or layout the library does not take returns 1; a dtype or device it does not take raises, both before any
    library call.  The destinations must not overlap the inputs or each other (not checked)."""
    n = len(flows)
    if n == 0 or len(outs) != n or None in flows or None in outs or image.dim() != 4 or filt.dim() != 4:
        return 1
    b, c, h, w = image.shape
    if not _channels_innermost(image) or not _fi_filter_ok(image, filt) or filt.size(1) < 1 or 0 in image.shape:
        return 1
    for fl, out in zip(flows, outs):
        if fl.dim() != 4 or tuple(fl.shape) != (b, 2, h, w) or not _same_strides(fl, flows[0]):
            return 1
        if out.dim() != 4 or out.shape != image.shape or not _channels_innermost(out) or not _same_strides(out, outs[0]):
            return 1
    dtype, suffix = _fi_image_dtype((image, *outs), (filt, *flows))
    fp = (ctypes.c_void_p * n)(*[fl.data_ptr() for fl in flows])
    op = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    with torch.cuda.device(image.device):
        fn = getattr(lib(), "vfi_filterinterp_forward_ori_nhwc_multi_to" + suffix)
        return _finish(fn(_ptr(image), fp, _ptr(filt), op, n, b, c, h, w, filt.size(1), _st_nhwc(image), _st4(flows[0]),
                          _st4(filt), _st_nhwc(outs[0]), _stream(image, dtype)))


def filterinterp_nhwc_access_width(image, filt, outs):
    """the access width, in elements, filterinterp_forward_nhwc_multi_to runs these tensors with (host code, no launch)"""
    if len(outs) == 0 or None in outs or not _is4(image, filt, *outs) or not _fi_filter_ok(image, filt) or \
            not _channels_innermost(image) or \
            not all(o.shape == image.shape and _channels_innermost(o) and _same_strides(o, outs[0]) for o in outs):
        raise RuntimeError("filterinterp_nhwc_access_width: not the tensors of a filterinterp_forward_nhwc_multi_to call")
    _bf16_or_f32(image, *outs)
    if _dev(filt) != image.device:
        raise RuntimeError("vfidkr_amd.cabi: tensors must live on one device")
    op = (ctypes.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    b, _, h, w = image.shape
    return lib().vfi_filterinterp_nhwc_access_width(image.element_size(), _ptr(image), op, len(outs), b, h, w, filt.size(1),
                                                    _st_nhwc(image), _st_nhwc(outs[0]))


def filterinterp_forward_ori_f16(input1, input2, input3, output, direct=False):
    """fp16 storage: input1 / output are float16 tensors, flow and filter float32."""
    dims = _fi_checks(input1, input2, input3, output)
    if dims is None or output.stride(3) != 1:
        return 1
    b, c, h, w = dims
    if _on_gpu(torch.float32, input2, input3) != _on_gpu(torch.float16, input1, output):
        raise RuntimeError("vfidkr_amd.cabi: tensors must live on one device")
    with torch.cuda.device(input1.device):
        fn = lib().vfi_filterinterp_forward_ori_f16_direct if direct else lib().vfi_filterinterp_forward_ori_f16
        return _finish(fn(_ptr(input1), _ptr(input2), _ptr(input3), _ptr(output), b, c, h, w, input3.size(1),
                          _st(input1), _st(input2), _st(input3), _stream(input2)))


def filterinterp_backward_ori(input1, input2, input3, gradoutput, gradinput1, gradinput2, gradinput3):
    dims = _fi_checks(input1, input2, input3, gradinput1)
    if dims is None:
        return 1
    # the library addresses gradoutput / gradinput1 with input1's strides, gradinput2 with input2's, gradinput3 with input3's
    if not _addressed_as(input1, gradoutput, gradinput1) or not _addressed_as(input2, gradinput2) or \
            not _addressed_as(input3, gradinput3) or not _fi_filter_ok(input1, input3):
        return 1
    b, c, h, w = dims
    with torch.cuda.device(_on_gpu(torch.float32, input1, input2, input3, gradoutput, gradinput1, gradinput2, gradinput3)):
        return _finish(lib().vfi_filterinterp_backward_ori(
            _ptr(input1), _ptr(input2), _ptr(input3), _ptr(gradoutput), _ptr(gradinput1), _ptr(gradinput2),
            _ptr(gradinput3), b, c, h, w, input3.size(1), _st(input1), _st(input2), _st(input3), _stream(input1)))


def filterinterp_backward_ori_image_multi(flows, input3, gradoutputs, gradinput1):
    """gradinput1 = the sum over t of the image gradient of FilterInterpolation(., flows[t], input3) for gradoutputs[t]: the
    backward of filterinterp_forward_ori_multi towards the image alone.  gradinput1 is written in full (no zero fill needed).
    The gradients and gradinput1 float32, or all bfloat16 (vfi_filterinterp_backward_ori_image_multi_bf16: bf16_rne of the
    float32 call on the widened gradients, bit for bit); flows and filter float32 always."""
    n = len(flows)
    if n == 0 or len(gradoutputs) != n or None in flows or None in gradoutputs:
        return 1
    for fl, g in zip(flows, gradoutputs):
        # gradinput1 in the image's place: the binding's checks, then one layout per list and the gradients shaped like gradinput1
        if _fi_checks(gradinput1, fl, input3, None) is None or not _same_strides(fl, flows[0]) or g is None or \
                g.dim() != 4 or g.shape != gradinput1.shape or g.stride(3) != 1 or not _same_strides(g, gradoutputs[0]):
            return 1
    if not _fi_filter_ok(gradinput1, input3):
        return 1
    dtype, suffix = _fi_image_dtype((gradinput1, *gradoutputs), (input3, *flows))
    b, c, h, w = gradinput1.shape
    fp = (ctypes.c_void_p * n)(*[fl.data_ptr() for fl in flows])
    gp = (ctypes.c_void_p * n)(*[g.data_ptr() for g in gradoutputs])
    with torch.cuda.device(gradinput1.device):
        fn = getattr(lib(), "vfi_filterinterp_backward_ori_image_multi" + suffix)
        return _finish(fn(fp, _ptr(input3), gp, _ptr(gradinput1), n, b, c, h, w, input3.size(1), _st(gradinput1), _st(flows[0]),
                          _st(input3), _st(gradoutputs[0]), _stream(gradinput1, dtype)))


def filterinterp_forward_defor(variant, input1, input2, input3, input4, output, general=False):
    """variant: DEFOR_OFFSET (4-input forward), DEFOR_REGION (deforconv), DEFOR_NOFILTER (input4 = None).
    general=True: always the one-thread-per-pixel kernel (an internal entry point the tests compare the staged one with)."""
    # (the kernels address the output with input1's strides in every variant)
    dims = _fi_checks(input1, input2, input3, output)
    if dims is None:
        return 1
    b, c, h, w = dims
    if variant == DEFOR_NOFILTER:
        fs = int(math.sqrt(input3.size(1) // 2))
        p4, s4 = ctypes.c_void_p(0), _st(input3)
        if 2 * fs * fs > input3.size(1):
            return 1
        input4 = None
    else:
        fs = int(math.sqrt(input3.size(1)))
        # input4: the 2 * fs * fs offsets of every pixel
        if not _is4(input4) or input4.stride(3) != 1 or not _fi_filter_ok(input1, input4) or input4.size(1) < 2 * fs * fs:
            return 1
        p4, s4 = _ptr(input4), _st(input4)
    with torch.cuda.device(_on_gpu(torch.float32, input1, input2, input3, input4, output)):
        fn = lib().vfi_filterinterp_forward_defor_general if general else lib().vfi_filterinterp_forward_defor
        return _finish(fn(variant, _ptr(input1), _ptr(input2), _ptr(input3), p4, _ptr(output), b, c, h, w, fs, _st(input1),
                          _st(input2), _st(input3), s4, _stream(input1)))


def filterinterp_backward_defor(variant, input1, input2, input3, input4, gradoutput, gradinput1, gradinput2,
                                gradinput3, gradinput4):
    """Backward of the deformable variants; variant DEFOR_NOFILTER: input4 = gradinput4 = None."""
    dims = _fi_checks(input1, input2, input3, gradinput1)
    if dims is None:
        return 1
    if not _addressed_as(input1, gradoutput, gradinput1) or not _addressed_as(input2, gradinput2) or \
            not _addressed_as(input3, gradinput3) or not _fi_filter_ok(input1, input3):
        return 1
    b, c, h, w = dims
    if variant == DEFOR_NOFILTER:
        fs = int(math.sqrt(input3.size(1) // 2))
        p4, g4, s4 = ctypes.c_void_p(0), ctypes.c_void_p(0), _st(input3)
        input4 = gradinput4 = None
    else:
        fs = int(math.sqrt(input3.size(1)))
        if not _is4(input4) or input4.stride(3) != 1 or not _addressed_as(input4, gradinput4) or \
                not _fi_filter_ok(input1, input4) or input4.size(1) < 2 * fs * fs:
            return 1
        p4, g4, s4 = _ptr(input4), _ptr(gradinput4), _st(input4)
    with torch.cuda.device(_on_gpu(torch.float32, input1, input2, input3, input4, gradoutput, gradinput1, gradinput2, gradinput3,
                                   gradinput4)):
        return _finish(lib().vfi_filterinterp_backward_defor(
            variant, _ptr(input1), _ptr(input2), _ptr(input3), p4, _ptr(gradoutput), _ptr(gradinput1),
            _ptr(gradinput2), _ptr(gradinput3), g4, b, c, h, w, fs, _st(input1), _st(input2), _st(input3), s4,
            _stream(input1)))


# ---------------------------------------------------------------- flowprojection_cuda / depthflowprojection_cuda

def _proj_checks(input1, planes, like_input1):
    """(b, h, w) of a projection call: the flow [B, 2, H, W], `planes` (count, depth) [B, 1, H, W] with strides of their own,
    `like_input1` (the output, the gradients) addressed with the flow's strides; w stride 1 everywhere"""
    if not _is4(input1) or input1.size(1) != 2:
        return None
    b, _, h, w = input1.shape
    if not all(_shaped(t, b, 1, h, w) for t in planes) or not _addressed_as(input1, *like_input1) or \
            not _nchw_ok(input1, *planes):
        return None
    return b, h, w


def flowprojection_forward(input1, count, output, fillhole):
    dims = _proj_checks(input1, (count,), (output,))
    if dims is None:
        return 1
    b, h, w = dims
    with torch.cuda.device(_on_gpu(torch.float32, input1, count, output)):
        return _finish(lib().vfi_flowprojection_forward(_ptr(input1), _ptr(count), _ptr(output), b, h, w,
                                                        int(fillhole), _st(input1), _st(count), _stream(input1)))


def flowprojection_forward_batch(inputs1, counts, outputs, fillhole, inputs2=None):
    """The list form of flowprojection_forward / depthflowprojection_forward (inputs2: one depth tensor per item, or one
    tensor shared by all): every item in one launch triple.  Items share shape and strides."""
    n = len(inputs1)
    if n == 0 or len(counts) != n or len(outputs) != n or None in inputs1 or None in counts or None in outputs:
        return 1
    if inputs2 is not None and not isinstance(inputs2, (list, tuple)):
        inputs2 = [inputs2] * n
    if inputs2 is not None and (len(inputs2) != n or None in inputs2):
        return 1
    f0, c0 = inputs1[0], counts[0]
    if _proj_checks(f0, (c0,), (outputs[0],)) is None:
        return 1
    b, _, h, w = f0.shape
    for i in range(n):
        fl, cn, out = inputs1[i], counts[i], outputs[i]
        if fl.dim() != 4 or fl.size(1) != 2 or tuple(fl.shape) != tuple(f0.shape) or tuple(out.shape) != tuple(f0.shape) or tuple(cn.shape) != (b, 1, h, w):
            return 1
        if not _same_strides(fl, f0) or not _same_strides(out, f0) or not _same_strides(cn, c0):
            return 1
        _dev(fl), _dev(cn), _dev(out)
        if inputs2 is not None:
            d = inputs2[i]
            if not _shaped(d, b, 1, h, w) or d.stride(3) != 1 or not _same_strides(d, inputs2[0]):
                return 1
            _dev(d)
    _on_gpu(torch.float32, *inputs1, *counts, *outputs, *(inputs2 or ()))
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])     # noqa: E731
    with torch.cuda.device(_dev(f0)):
        if inputs2 is None:
            return _finish(lib().vfi_flowprojection_forward_batch(arr(inputs1), arr(counts), arr(outputs), n, b, h, w, int(fillhole),
                                                                  _st(f0), _st(c0), _stream(f0)))
        return _finish(lib().vfi_depthflowprojection_forward_batch(arr(inputs1), arr(inputs2), arr(counts), arr(outputs), n, b, h, w,
                                                                   int(fillhole), _st(f0), _st(inputs2[0]), _st(c0), _stream(f0)))


def projection_reserve(batch, h, w, device=None):
    """Size the projection workspace of the current stream for [batch, *, h, w] frames (call before graph capture)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        return _finish(lib().vfi_projection_reserve(int(batch), int(h), int(w),
                                                    ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))


def release_workspaces():
    """Free every workspace the library holds (synchronises).  Only when no launch or graph still needs them."""
    return _finish(lib().vfi_release_workspaces())


def flowprojection_backward(input1, count, gradoutput, gradinput1):
    dims = _proj_checks(input1, (count,), (gradoutput, gradinput1))
    if dims is None:
        return 1
    b, h, w = dims
    with torch.cuda.device(_on_gpu(torch.float32, input1, count, gradoutput, gradinput1)):
        return _finish(lib().vfi_flowprojection_backward(_ptr(input1), _ptr(count), _ptr(gradoutput),
                                                         _ptr(gradinput1), b, h, w, _st(input1), _st(count),
                                                         _stream(input1)))


def depthflowprojection_forward(input1, input2, count, output, fillhole):
    dims = _proj_checks(input1, (input2, count), (output,))
    if dims is None:
        return 1
    b, h, w = dims
    with torch.cuda.device(_on_gpu(torch.float32, input1, input2, count, output)):
        return _finish(lib().vfi_depthflowprojection_forward(
            _ptr(input1), _ptr(input2), _ptr(count), _ptr(output), b, h, w, int(fillhole), _st(input1), _st(input2),
            _st(count), _stream(input1)))


def depthflowprojection_backward(input1, input2, count, output, gradoutput, gradinput1, gradinput2):
    # output, gradoutput and gradinput1 are addressed with input1's strides, gradinput2 with input2's
    dims = _proj_checks(input1, (input2, count), (output, gradoutput, gradinput1))
    if dims is None or not _addressed_as(input2, gradinput2):
        return 1
    b, h, w = dims
    with torch.cuda.device(_on_gpu(torch.float32, input1, input2, count, output, gradoutput, gradinput1, gradinput2)):
        return _finish(lib().vfi_depthflowprojection_backward(
            _ptr(input1), _ptr(input2), _ptr(count), _ptr(output), _ptr(gradoutput), _ptr(gradinput1),
            _ptr(gradinput2), b, h, w, _st(input1), _st(input2), _st(count), _stream(input1)))


def mindepthflowprojection_forward(input1, input2, count, output, fillhole):
    """mindepthflowprojection_cuda.cc:12-66; count and output zero-filled by the caller."""
    dims = _proj_checks(input1, (input2, count), (output,))
    if dims is None:
        return 1
    b, h, w = dims
    with torch.cuda.device(_on_gpu(torch.float32, input1, input2, count, output)):
        return _finish(lib().vfi_mindepthflowprojection_forward(
            _ptr(input1), _ptr(input2), _ptr(count), _ptr(output), b, h, w, int(fillhole), _st(input1), _st(input2),
            _st(count), _stream(input1)))


def mindepthflowprojection_backward(input1, input2, count, output, gradoutput, gradinput1, gradinput2):
    """mindepthflowprojection_cuda.cc:68-139; `output` and `gradinput2` are accepted and unused, as in the reference."""
    dims = _proj_checks(input1, (input2, count), (gradoutput, gradinput1))
    if dims is None:
        return 1
    b, h, w = dims
    with torch.cuda.device(_on_gpu(torch.float32, input1, input2, count, gradoutput, gradinput1)):
        return _finish(lib().vfi_mindepthflowprojection_backward(
            _ptr(input1), _ptr(input2), _ptr(count), _ptr(gradoutput), _ptr(gradinput1), b, h, w, _st(input1),
            _st(input2), _st(count), _stream(input1)))


# ---------------------------------------------------------------- interpolation_cuda / interpolationch_cuda

def interpolation_forward(input1, input2, output, require_c3=False):
    if not _is4(input1):
        return 1
    b, c, h, w = input1.shape
    if require_c3 and c != 3:
        return 1
    if not _shaped(input2, b, 2, h, w) or not _nchw_ok(input1, input2):
        return 1
    if not _addressed_as(input1, output):
        return 1
    with torch.cuda.device(_on_gpu(torch.float32, input1, input2, output)):
        return _finish(lib().vfi_interpolation_forward(_ptr(input1), _ptr(input2), _ptr(output), b, c, h, w,
                                                       _st(input1), _st(input2), _stream(input1)))


def interpolation_backward(input1, input2, gradoutput, gradinput1, gradinput2, require_c3=False):
    if not _is4(input1):
        return 1
    b, c, h, w = input1.shape
    if require_c3 and c != 3:
        return 1
    if not _shaped(input2, b, 2, h, w) or input1.stride(3) != 1 or input2.stride(3) != 1:
        return 1
    if not _addressed_as(input1, gradoutput, gradinput1) or not _addressed_as(input2, gradinput2):
        return 1
    with torch.cuda.device(_on_gpu(torch.float32, input1, input2, gradoutput, gradinput1, gradinput2)):
        return _finish(lib().vfi_interpolation_backward(_ptr(input1), _ptr(input2), _ptr(gradoutput),
                                                        _ptr(gradinput1), _ptr(gradinput2), b, c, h, w, _st(input1),
                                                        _st(input2), _stream(input1)))


# ---------------------------------------------------------------- separableconv_cuda / separableconvflow_cuda

def _sep_checks(input1, input2, input3, require_c3=True):
    """require_c3: the reference's wrappers refuse any other channel count (separableconv_cuda.cc); the library takes any."""
    if not _is4(input1, input2, input3):
        return None
    b, c, h, w = input1.shape
    fs = input2.size(1)
    if (require_c3 and c != 3) or input2.size(0) != b or input2.size(1) != input3.size(1):
        return None
    if input2.size(2) != h - fs + 1 or input2.size(3) != w - fs + 1 or input3.shape != input2.shape:
        return None
    if input1.stride(3) != 1 or input2.stride(3) != 1 or input3.stride(3) != 1:
        return None
    if input2.stride(0) != input3.stride(0) or input2.stride(1) != input3.stride(1):
        return None
    return b, c, h, w, fs


def separableconv_forward(input1, input2, input3, output, require_c3=True):
    dims = _sep_checks(input1, input2, input3, require_c3)
    if dims is None:
        return 1
    b, c, h, w, fs = dims
    if not _shaped(output, b, c, h - fs + 1, w - fs + 1) or output.stride(3) != 1:
        return 1
    with torch.cuda.device(_on_gpu(torch.float32, input1, input2, input3, output)):
        return _finish(lib().vfi_separableconv_forward(_ptr(input1), _ptr(input2), _ptr(input3), _ptr(output), b, c,
                                                       h, w, fs, _st(input1), _st(input2), _st(input3), _st(output),
                                                       _stream(input1)))


def separableconv_backward(input1, input2, input3, gradoutput, gradinput1, gradinput2, gradinput3, require_c3=True):
    dims = _sep_checks(input1, input2, input3, require_c3)
    if dims is None or gradoutput is None or gradoutput.dim() != 4 or gradoutput.stride(3) != 1:
        return 1
    if not _addressed_as(input1, gradinput1) or not _addressed_as(input2, gradinput2) or not _addressed_as(input3, gradinput3):
        return 1
    b, c, h, w, fs = dims
    if tuple(gradoutput.shape) != (b, c, h - fs + 1, w - fs + 1):
        return 1
    with torch.cuda.device(_on_gpu(torch.float32, input1, input2, input3, gradoutput, gradinput1, gradinput2, gradinput3)):
        return _finish(lib().vfi_separableconv_backward(
            _ptr(input1), _ptr(input2), _ptr(input3), _ptr(gradoutput), _ptr(gradinput1), _ptr(gradinput2),
            _ptr(gradinput3), b, c, h, w, fs, _st(input1), _st(input2), _st(input3), _st(gradoutput),
            _stream(input1)))


def separableconvflow_forward(input1, input2, input3, flow_output, require_c3=True):
    dims = _sep_checks(input1, input2, input3, require_c3)
    if dims is None:
        return 1
    b, c, h, w, fs = dims
    if not _shaped(flow_output, b, 2, h - fs + 1, w - fs + 1) or flow_output.stride(3) != 1:
        return 1
    with torch.cuda.device(_on_gpu(torch.float32, input2, input1, input3, flow_output)):
        return _finish(lib().vfi_separableconvflow_forward(_ptr(input2), _ptr(input3), _ptr(flow_output), b, h, w,
                                                           fs, _st(input2), _st(input3), _st(flow_output),
                                                           _stream(input2)))


def separableconvflow_backward(input1, input2, input3, gradflow_output, gradinput2, gradinput3, require_c3=True):
    dims = _sep_checks(input1, input2, input3, require_c3)
    if dims is None or gradflow_output is None or gradflow_output.dim() != 4 or gradflow_output.stride(3) != 1:
        return 1
    if not _addressed_as(input2, gradinput2) or not _addressed_as(input3, gradinput3):
        return 1
    b, c, h, w, fs = dims
    if tuple(gradflow_output.shape) != (b, 2, h - fs + 1, w - fs + 1):
        return 1
    with torch.cuda.device(_on_gpu(torch.float32, input2, input1, input3, gradflow_output, gradinput2, gradinput3)):
        return _finish(lib().vfi_separableconvflow_backward(
            _ptr(input2), _ptr(input3), _ptr(gradflow_output), _ptr(gradinput2), _ptr(gradinput3), b, h, w, fs,
            _st(input2), _st(input3), _st(gradflow_output), _stream(input2)))


# ---------------------------------------------------------------- correlation_cuda

def correlation_output_dims(h, w, pad_size, kernel_size, max_displacement, stride1, stride2):
    oc, oh, ow = _i(), _i(), _i()
    err = lib().vfi_correlation_output_dims(h, w, pad_size, kernel_size, max_displacement, stride1, stride2,
                                            ctypes.byref(oc), ctypes.byref(oh), ctypes.byref(ow))
    if err != 0:
        raise RuntimeError("CUDA call failed")
    return oc.value, oh.value, ow.value


_CORR_SUFFIX = {torch.float16: "_f16", torch.bfloat16: "_bf16"}     # the 2-byte dtypes with entries of their own


def _corr_call(f32_name, tensors, *args):
    """The float entry; for float16 tensors the reference's at::Half instantiation and for bfloat16 tensors the `_bf16` entry
    (no conversion; every tensor is checked for dtype and device), on the tensors' stream."""
    suffix = _CORR_SUFFIX.get(tensors[0].dtype)
    # (a 2-byte tensor behind a float32 first one would be read past its end)
    device = _on_gpu(tensors[0].dtype if suffix else torch.float32, *tensors)
    with torch.cuda.device(device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        err = getattr(lib(), f32_name + (suffix or ""))(*[_ptr(t) for t in tensors], *args, stream)
    if err != 0:
        raise RuntimeError("CUDA call failed")


def _corr_inputs(what, first, *rest):
    """the feature maps of a correlation call: [B, C, H, W], all of one shape (any strides: they are made contiguous)"""
    if not _is4(first) or any(t is None or t.dim() != 4 or t.shape != first.shape for t in rest):
        raise RuntimeError("%s: the inputs must be [B, C, H, W] tensors of one shape, none of it zero" % what)


def correlation_forward(input1, input2, pad_size, kernel_size, max_displacement, stride1, stride2):
    """Allocates and returns the output, as the reference binding resizes its `output` argument.  float32, float16 (the
    reference's at::Half arithmetic) or bfloat16 (exact products, float32 sums, one rounding: include/vfi_hip.h) -- the
    output has the inputs' dtype."""
    _corr_inputs("correlation_forward", input1, input2)
    _on_gpu(input1.dtype if input1.dtype in _CORR_SUFFIX else torch.float32, input1, input2)
    input1, input2 = input1.contiguous(), input2.contiguous()
    b, c, h, w = input1.shape
    oc, oh, ow = correlation_output_dims(h, w, pad_size, kernel_size, max_displacement, stride1, stride2)
    dtype = input1.dtype if input1.dtype in _CORR_SUFFIX else torch.float32
    output = torch.empty((b, oc, oh, ow), dtype=dtype, device=input1.device)
    _corr_call("vfi_correlation_forward", (input1, input2, output), b, c, h, w, pad_size,
               kernel_size, max_displacement, stride1, stride2)
    return output


def correlation_forward_bf16_kernel(which, input1, input2, pad_size, kernel_size, max_displacement, stride1, stride2, out=None):
    """correlation_forward on bfloat16 tensors through ONE of its two kernels whatever the tile count (internal: tests and
    tools/bench_corr_bf16.py).  which: "mfma" (PWC-Net's configuration only) or "generic".  `out`: a dense bfloat16 tensor
    (or view) of the output's shape to write into."""
    _corr_inputs("correlation_forward_bf16_kernel", input1, input2)
    _on_gpu(torch.bfloat16, input1, input2, out)
    input1, input2 = input1.contiguous(), input2.contiguous()
    b, c, h, w = input1.shape
    oc, oh, ow = correlation_output_dims(h, w, pad_size, kernel_size, max_displacement, stride1, stride2)
    if out is None:
        out = torch.empty((b, oc, oh, ow), dtype=torch.bfloat16, device=input1.device)
    if out.dim() != 4 or tuple(out.shape) != (b, oc, oh, ow) or not out.is_contiguous():
        raise RuntimeError("correlation_forward_bf16_kernel: `out` must be a dense tensor of the output's shape")
    for t in (input1, input2, out):
        _dev(t, torch.bfloat16)
    with torch.cuda.device(input1.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(input1.device).cuda_stream)
        err = lib().vfi_correlation_forward_bf16_kernel({"mfma": 0, "generic": 1}[which], _ptr(input1), _ptr(input2),
                                                        _ptr(out), b, c, h, w, pad_size, kernel_size, max_displacement, stride1,
                                                        stride2, stream)
    if err != 0:
        raise RuntimeError("CUDA call failed")
    return out


def correlation_forward_pair(a1, a2, b1, b2, pad_size, kernel_size, max_displacement, stride1, stride2):
    """(correlation_forward(a1, a2, ...), correlation_forward(b1, b2, ...)) from one launch: equal shapes, all four float32
    or all four bfloat16 (vfi_correlation_forward_pair_bf16: each output bit-equal to correlation_forward's on its item);
    the outputs have the inputs' dtype."""
    _corr_inputs("correlation_forward_pair", a1, a2, b1, b2)
    dtype, suffix = _bf16_or_f32(a1, a2, b1, b2)
    a1, a2, b1, b2 = (t.contiguous() for t in (a1, a2, b1, b2))
    b, c, h, w = a1.shape
    oc, oh, ow = correlation_output_dims(h, w, pad_size, kernel_size, max_displacement, stride1, stride2)
    outa = torch.empty((b, oc, oh, ow), device=a1.device, dtype=dtype)
    outb = torch.empty_like(outa)
    with torch.cuda.device(a1.device):
        fn = getattr(lib(), "vfi_correlation_forward_pair" + suffix)
        err = fn(_ptr(a1), _ptr(a2), _ptr(outa), _ptr(b1), _ptr(b2), _ptr(outb), b, c, h, w,
                 pad_size, kernel_size, max_displacement, stride1, stride2, _stream(a1, dtype))
    if _finish(err) != 0:
        raise RuntimeError("correlation_forward_pair: the binding returned %d" % err)
    return outa, outb


def correlation_backward(input1, input2, gradoutput, pad_size, kernel_size, max_displacement, stride1, stride2):
    _corr_inputs("correlation_backward", input1, input2)
    _on_gpu(input1.dtype if input1.dtype in _CORR_SUFFIX else torch.float32, input1, input2, gradoutput)
    input1, input2, gradoutput = input1.contiguous(), input2.contiguous(), gradoutput.contiguous()
    b, c, h, w = input1.shape
    if input2.shape != input1.shape or \
            tuple(gradoutput.shape) != (b,) + correlation_output_dims(h, w, pad_size, kernel_size, max_displacement, stride1, stride2):
        raise RuntimeError("correlation_backward: input2 / gradoutput do not match input1's shape and the output dimensions")
    g1, g2 = torch.empty_like(input1), torch.empty_like(input2)
    _corr_call("vfi_correlation_backward", (input1, input2, gradoutput, g1, g2), b, c, h, w,
               pad_size, kernel_size, max_displacement, stride1, stride2)
    return g1, g2


def correlation_backward_pair(a1, a2, ga, b1, b2, gb, pad_size, kernel_size, max_displacement, stride1, stride2,
                              want=(True, True, True, True)):
    """(correlation_backward(a1, a2, ga, ...), correlation_backward(b1, b2, gb, ...)) from ONE vfi_correlation_backward_pair
    call: equal shapes, every tensor float32 or every tensor bfloat16 (vfi_correlation_backward_pair_bf16).  Returns
    (grad a1, grad a2, grad b1, grad b2), each written in full, of the inputs' dtype and bit-equal to the single call's;
    None where `want` says so or where that item's gradoutput is None (such a gradient costs nothing)."""
    inputs = (a1, a2, b1, b2)
    _corr_inputs("correlation_backward_pair", *inputs)
    b, c, h, w = a1.shape
    gshape = (b,) + correlation_output_dims(h, w, pad_size, kernel_size, max_displacement, stride1, stride2)
    if len(want) != 4 or any(tuple(t.shape) != tuple(a1.shape) for t in inputs) or \
            any(g is not None and tuple(g.shape) != gshape for g in (ga, gb)):
        raise RuntimeError("correlation_backward_pair: the four inputs must have one shape and the gradoutputs the output dimensions")
    dtype, suffix = _bf16_or_f32(*inputs, *(g for g in (ga, gb) if g is not None))
    a1, a2, b1, b2 = (t.contiguous() for t in inputs)
    ga, gb = (None if g is None else g.contiguous() for g in (ga, gb))
    grads = [torch.empty_like(t) if want[i] and (ga, gb)[i // 2] is not None else None for i, t in enumerate((a1, a2, b1, b2))]
    if all(g is None for g in grads):
        return tuple(grads)
    with torch.cuda.device(a1.device):
        fn = getattr(lib(), "vfi_correlation_backward_pair" + suffix)
        err = fn(_ptr(a1), _ptr(a2), _opt(ga), _opt(grads[0]), _opt(grads[1]),
                 _ptr(b1), _ptr(b2), _opt(gb), _opt(grads[2]), _opt(grads[3]), b, c, h, w,
                 pad_size, kernel_size, max_displacement, stride1, stride2, _stream(a1, dtype))
    if _finish(err) != 0:
        raise RuntimeError("correlation_backward_pair: the binding returned %d" % err)
    return tuple(grads)


# the correlation with PWC-Net's LeakyReLU fused in (vfi_correlation_lrelu_*): float32

def _dense_planes(t):
    """The planes of every image contiguous and the images at least an image apart: a contiguous NCHW tensor, or a
    channel slice buf[:, k:k + C] of a larger one (a dimension of size 1 has no stride to speak of)."""
    b, c, h, w = t.shape
    s = t.stride()
    return (w == 1 or s[3] == 1) and (h == 1 or s[2] == w) and (c == 1 or s[1] == h * w) and (b == 1 or s[0] >= c * h * w)


def _planes(t):
    """(t, its batch stride in elements), t made contiguous unless its layout is dense planes at any batch stride"""
    if not _dense_planes(t):
        t = t.contiguous()
    return t, (t.stride(0) if t.size(0) > 1 else t.size(1) * t.size(2) * t.size(3))


def _slope(negative_slope):
    s = ctypes.c_float(float(negative_slope)).value
    if not (s > 0.0 and math.isfinite(s)):
        raise RuntimeError("correlation_lrelu: negative_slope must be finite and > 0 (the backward reads the sign off the output)")
    return s


def _lrelu_out(out, shape, like, what, dtype=torch.float32):
    if out is None:
        return torch.empty(shape, device=like.device, dtype=dtype)
    if out.dim() != 4 or tuple(out.shape) != tuple(shape):
        raise RuntimeError("%s: out= must have the output dimensions %s" % (what, tuple(shape)))
    if not _dense_planes(out):
        raise RuntimeError("%s: out= must have dense planes (a channel slice of a contiguous NCHW buffer)" % what)
    if _dev(out, dtype) != like.device:
        raise RuntimeError("%s: out= must live on the inputs' device" % what)
    return out


def _bf16_or_f32(first, *rest):
    """The dtype a call with `_bf16` twins runs in -- bfloat16 when its first tensor is, float32 otherwise -- after checking
    every tensor for it and for the device (float16 and a bfloat16 / float32 mix raise here, before any library call)."""
    dtype = torch.bfloat16 if first.dtype == torch.bfloat16 else torch.float32
    _on_gpu(dtype, first, *rest)
    return dtype, ("_bf16" if dtype == torch.bfloat16 else "")


def correlation_lrelu_forward(input1, input2, pad_size, kernel_size, max_displacement, stride1, stride2, negative_slope, out=None):
    """leaky_relu(correlation_forward(input1, input2, ...), negative_slope) from the correlation's own launch, bit for bit.
    float32, or bfloat16 (every tensor, out= included: vfi_correlation_lrelu_forward_bf16 -- torch's bfloat16 leaky_relu on the
    bfloat16 cost volume, two roundings).
    out=: where to write it -- a tensor of the output's shape whose planes are dense, such as buf[:, k:k + 81] of a
    contiguous NCHW buffer; returned as it is."""
    slope = _slope(negative_slope)
    _corr_inputs("correlation_lrelu_forward", input1, input2)
    b, c, h, w = input1.shape
    oc, oh, ow = correlation_output_dims(h, w, pad_size, kernel_size, max_displacement, stride1, stride2)
    if out is not None:                                     # (its shape and layout first, then everybody's dtype and device)
        _lrelu_out(out, (b, oc, oh, ow), input1, "correlation_lrelu_forward",
                   torch.bfloat16 if input1.dtype == torch.bfloat16 else torch.float32)
    dtype, suffix = _bf16_or_f32(input1, input2)
    input1, input2 = input1.contiguous(), input2.contiguous()
    out = _lrelu_out(out, (b, oc, oh, ow), input1, "correlation_lrelu_forward", dtype)
    with torch.cuda.device(input1.device):
        fn = getattr(lib(), "vfi_correlation_lrelu_forward" + suffix)
        err = fn(_ptr(input1), _ptr(input2), _ptr(out), _planes(out)[1], b, c, h, w, pad_size,
                 kernel_size, max_displacement, stride1, stride2, slope, _stream(input1, dtype))
    if _finish(err) != 0:
        raise RuntimeError("correlation_lrelu_forward: the binding returned %d" % err)
    return out


def correlation_lrelu_forward_pair(a1, a2, b1, b2, pad_size, kernel_size, max_displacement, stride1, stride2, negative_slope,
                                   out=None):
    """(correlation_lrelu_forward(a1, a2, ...), correlation_lrelu_forward(b1, b2, ...)) from one launch: equal shapes.
    out=: a pair of destinations (either may be None), each as correlation_lrelu_forward's.  float32, or bfloat16 for every
    tensor, out= included (vfi_correlation_lrelu_forward_pair_bf16: each output bit-equal to correlation_lrelu_forward's)."""
    slope = _slope(negative_slope)
    _corr_inputs("correlation_lrelu_forward_pair", a1, a2, b1, b2)
    b, c, h, w = a1.shape
    oc, oh, ow = correlation_output_dims(h, w, pad_size, kernel_size, max_displacement, stride1, stride2)
    outs = tuple(out) if out is not None else (None, None)
    if len(outs) != 2 or (outs[0] is not None and outs[0] is outs[1]):
        raise RuntimeError("correlation_lrelu_forward_pair: out= is a pair of two different destinations")
    for o in outs:                                          # (their shape and layout first, then everybody's dtype and device)
        if o is not None:
            _lrelu_out(o, (b, oc, oh, ow), a1, "correlation_lrelu_forward_pair",
                       torch.bfloat16 if a1.dtype == torch.bfloat16 else torch.float32)
    dtype, suffix = _bf16_or_f32(a1, a2, b1, b2)
    a1, a2, b1, b2 = (t.contiguous() for t in (a1, a2, b1, b2))
    outa, outb = (_lrelu_out(o, (b, oc, oh, ow), a1, "correlation_lrelu_forward_pair", dtype) for o in outs)
    with torch.cuda.device(a1.device):
        fn = getattr(lib(), "vfi_correlation_lrelu_forward_pair" + suffix)
        err = fn(_ptr(a1), _ptr(a2), _ptr(outa), _planes(outa)[1], _ptr(b1), _ptr(b2),
                 _ptr(outb), _planes(outb)[1], b, c, h, w, pad_size, kernel_size,
                 max_displacement, stride1, stride2, slope, _stream(a1, dtype))
    if _finish(err) != 0:
        raise RuntimeError("correlation_lrelu_forward_pair: the binding returned %d" % err)
    return outa, outb


def correlation_lrelu_backward(input1, input2, y, gradoutput, pad_size, kernel_size, max_displacement, stride1, stride2,
                               negative_slope):
    """correlation_backward(input1, input2, where(y > 0, g, g * negative_slope), ...) from the correlation backward's own
    launches: y is the saved output of correlation_lrelu_forward.  y and gradoutput are read where they lie when their
    planes are dense, whatever their batch stride (the narrow() view of torch.cat's backward); otherwise copied.  float32, or
    bfloat16 for all four tensors (vfi_correlation_lrelu_backward_bf16: g * negative_slope is rounded to bfloat16, as a
    materialised masked gradient would be)."""
    slope = _slope(negative_slope)
    _corr_inputs("correlation_lrelu_backward", input1, input2)
    b, c, h, w = input1.shape
    gshape = (b,) + correlation_output_dims(h, w, pad_size, kernel_size, max_displacement, stride1, stride2)
    if input2.shape != input1.shape or tuple(gradoutput.shape) != gshape or tuple(y.shape) != gshape:
        raise RuntimeError("correlation_lrelu_backward: input2 / y / gradoutput do not match input1's shape and the output dimensions")
    dtype, suffix = _bf16_or_f32(input1, input2, y, gradoutput)
    input1, input2 = input1.contiguous(), input2.contiguous()
    (y, ys), (gradoutput, gs) = _planes(y), _planes(gradoutput)
    g1, g2 = torch.empty_like(input1), torch.empty_like(input2)
    with torch.cuda.device(input1.device):
        fn = getattr(lib(), "vfi_correlation_lrelu_backward" + suffix)
        err = fn(_ptr(input1), _ptr(input2), _ptr(y), ys, _ptr(gradoutput), gs, _ptr(g1), _ptr(g2),
                 b, c, h, w, pad_size, kernel_size, max_displacement, stride1, stride2, slope, _stream(input1, dtype))
    if _finish(err) != 0:
        raise RuntimeError("correlation_lrelu_backward: the binding returned %d" % err)
    return g1, g2


def correlation_lrelu_backward_pair(a1, a2, ya, ga, b1, b2, yb, gb, pad_size, kernel_size, max_displacement, stride1, stride2,
                                    negative_slope, want=(True, True, True, True)):
    """(correlation_lrelu_backward(a1, a2, ya, ga, ...), correlation_lrelu_backward(b1, b2, yb, gb, ...)) from ONE
    vfi_correlation_lrelu_backward_pair call.  Returns (grad a1, grad a2, grad b1, grad b2), each written in full and
    bit-equal to the single call's; None where `want` says so or where that item's gradoutput is None.  float32, or bfloat16
    for every tensor (vfi_correlation_lrelu_backward_pair_bf16)."""
    slope = _slope(negative_slope)
    inputs = (a1, a2, b1, b2)
    _corr_inputs("correlation_lrelu_backward_pair", *inputs)
    b, c, h, w = a1.shape
    gshape = (b,) + correlation_output_dims(h, w, pad_size, kernel_size, max_displacement, stride1, stride2)
    if len(want) != 4 or any(tuple(t.shape) != tuple(a1.shape) for t in inputs) or \
            any(g is not None and (tuple(g.shape) != gshape or y is None or tuple(y.shape) != gshape) for y, g in ((ya, ga), (yb, gb))):
        raise RuntimeError("correlation_lrelu_backward_pair: the four inputs must have one shape, and y and the gradoutputs "
                           "the output dimensions")
    dtype, suffix = _bf16_or_f32(*inputs, *(t for y, g in ((ya, ga), (yb, gb)) if g is not None for t in (y, g)))
    a1, a2, b1, b2 = (t.contiguous() for t in inputs)
    (ya, yas), (ga, gas) = ((None, 0), (None, 0)) if ga is None else (_planes(ya), _planes(ga))
    (yb, ybs), (gb, gbs) = ((None, 0), (None, 0)) if gb is None else (_planes(yb), _planes(gb))
    grads = [torch.empty_like(t) if want[i] and (ga, gb)[i // 2] is not None else None for i, t in enumerate((a1, a2, b1, b2))]
    if all(g is None for g in grads):
        return tuple(grads)
    with torch.cuda.device(a1.device):
        fn = getattr(lib(), "vfi_correlation_lrelu_backward_pair" + suffix)
        err = fn(_ptr(a1), _ptr(a2), _opt(ya), yas, _opt(ga), gas, _opt(grads[0]), _opt(grads[1]),
                 _ptr(b1), _ptr(b2), _opt(yb), ybs, _opt(gb), gbs, _opt(grads[2]), _opt(grads[3]),
                 b, c, h, w, pad_size, kernel_size, max_displacement, stride1, stride2, slope, _stream(a1, dtype))
    if _finish(err) != 0:
        raise RuntimeError("correlation_lrelu_backward_pair: the binding returned %d" % err)
    return tuple(grads)


# ---------------------------------------------------------------- glue either side of the ops

def _nchw_ok(*tensors):
    return all(t is not None and t.dim() == 4 and t.stride(3) == 1 for t in tensors)


def flow_upsample4(input, output, mul0, mul1):
    if not _is4(input) or not _nchw_ok(input, output) or not _shaped(output, input.size(0), input.size(1), 4 * input.size(2), 4 * input.size(3)):
        return 1
    b, c, hq, wq = input.shape
    with torch.cuda.device(_on_gpu(torch.float32, input, output)):
        return _finish(lib().vfi_flow_upsample4(_ptr(input), _ptr(output), b, c, hq, wq, mul0, mul1, _st(input),
                                                _st(output), _stream(input)))


def flowprojection_forward_up4(flow_q, count, output, mul0, mul1, fillhole):
    if not _is4(flow_q) or not _nchw_ok(flow_q, count, output):
        return 1
    b, c, hq, wq = flow_q.shape
    if c != 2 or tuple(output.shape) != (b, 2, 4 * hq, 4 * wq) or tuple(count.shape) != (b, 1, 4 * hq, 4 * wq):
        return 1
    with torch.cuda.device(_on_gpu(torch.float32, flow_q, count, output)):
        return _finish(lib().vfi_flowprojection_forward_up4(_ptr(flow_q), _ptr(count), _ptr(output), b, hq, wq, mul0,
                                                            mul1, int(fillhole), _st(flow_q), _st(count), _st(output),
                                                            _stream(flow_q)))


def depthflowprojection_forward_up4(flow_q, input2, count, output, mul0, mul1, fillhole):
    if not _is4(flow_q) or not _nchw_ok(flow_q, input2, count, output):
        return 1
    b, c, hq, wq = flow_q.shape
    full = (b, 1, 4 * hq, 4 * wq)
    if c != 2 or tuple(output.shape) != (b, 2, 4 * hq, 4 * wq) or tuple(count.shape) != full or tuple(input2.shape) != full:
        return 1
    with torch.cuda.device(_on_gpu(torch.float32, flow_q, input2, count, output)):
        return _finish(lib().vfi_depthflowprojection_forward_up4(
            _ptr(flow_q), _ptr(input2), _ptr(count), _ptr(output), b, hq, wq, mul0, mul1, int(fillhole), _st(flow_q),
            _st(input2), _st(count), _st(output), _stream(flow_q)))


def _ptr_table(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def flow_upsample4_backward(grads_full, mul0, mul1, grad_q):
    """grad_q = sum_i (mul0 * mul1[i]) U^T grads_full[i] (1..8 items of one shape and layout); grad_q is written."""
    n = len(grads_full)
    if n == 0 or len(mul1) != n or not _is4(grad_q) or not _nchw_ok(grad_q, *grads_full):
        return 1
    b, c, hq, wq = grad_q.shape
    g0 = grads_full[0]
    if tuple(g0.shape) != (b, c, 4 * hq, 4 * wq) or not _addressed_as(g0, *grads_full):
        return 1
    with torch.cuda.device(_on_gpu(torch.float32, grad_q, *grads_full)):
        return _finish(lib().vfi_flow_upsample4_backward(_ptr_table(grads_full), (_f * n)(*mul1), n, _ptr(grad_q), b, c, hq, wq,
                                                         mul0, _st(g0), _st(grad_q), _stream(grad_q)))


def flowprojection_backward_up4(flow_q, counts, gradoutputs, mul0, mul1, grad_q, depths=None, outputs=None, grad_depths=None):
    """The backward of [depth]flowprojection_forward_up4 for the items (mul0, mul1[i]) of one flow_q.  depths (one tensor
    per item, or one shared by all) and outputs select the depth form; grad_depths: None, or one tensor or None per item."""
    n = len(counts)
    if n == 0 or len(gradoutputs) != n or len(mul1) != n or not _is4(flow_q):
        return 1
    b, c, hq, wq = flow_q.shape
    full = (b, 1, 4 * hq, 4 * wq)
    if c != 2 or tuple(grad_q.shape) != tuple(flow_q.shape) or not _nchw_ok(flow_q, grad_q, *counts, *gradoutputs):
        return 1
    c0, g0 = counts[0], gradoutputs[0]
    if tuple(c0.shape) != full or tuple(g0.shape) != (b, 2, 4 * hq, 4 * wq):
        return 1
    if not _addressed_as(c0, *counts) or not _addressed_as(g0, *gradoutputs):
        return 1
    mul = (_f * n)(*mul1)
    if depths is None:
        with torch.cuda.device(_on_gpu(torch.float32, flow_q, grad_q, *counts, *gradoutputs)):
            return _finish(lib().vfi_flowprojection_backward_up4(
                _ptr(flow_q), _ptr_table(counts), _ptr_table(gradoutputs), mul, n, _ptr(grad_q), b, hq, wq, mul0, _st(flow_q),
                _st(c0), _st(g0), _st(grad_q), _stream(flow_q)))
    if not isinstance(depths, (list, tuple)):
        depths = [depths] * n
    if outputs is None or len(depths) != n or len(outputs) != n or (grad_depths is not None and len(grad_depths) != n):
        return 1
    d0 = depths[0]
    if not _nchw_ok(d0) or tuple(d0.shape) != full or not _addressed_as(d0, *depths) or not _addressed_as(g0, *outputs):
        return 1
    wanted = [t for t in (grad_depths or []) if t is not None]
    if not _addressed_as(d0, *wanted):
        return 1
    with torch.cuda.device(_on_gpu(torch.float32, flow_q, grad_q, *counts, *gradoutputs, *depths, *outputs, *wanted)):
        return _finish(lib().vfi_depthflowprojection_backward_up4(
            _ptr(flow_q), _ptr_table(depths), _ptr_table(counts), _ptr_table(outputs), _ptr_table(gradoutputs), mul, n,
            _ptr(grad_q), None if grad_depths is None else _ptr_table(grad_depths), b, hq, wq, mul0, _st(flow_q), _st(d0),
            _st(c0), _st(g0), _st(grad_q), _stream(flow_q)))


def _same_strides(a, b):
    """same layout: the stride of a dimension of size 1 is never used (torch leaves it arbitrary, e.g. after slicing)"""
    return a.shape == b.shape and all(sa == sb for n, sa, sb in zip(a.shape, a.stride(), b.stride()) if n != 1)


def _addressed_as(ref, *tensors):
    """tensors the library reads or writes with ref's strides: same shape and layout as ref, or the call would address
    other elements than the caller's"""
    return all(t is not None and t.dim() == 4 and _same_strides(t, ref) for t in tensors)


def _fi_filter_ok(input1, filt):
    """a per-pixel filter / offset tensor: one plane of taps per pixel of input1"""
    return filt.dim() == 4 and filt.size(0) == input1.size(0) and tuple(filt.shape[2:]) == tuple(input1.shape[2:])


def filterinterp_blend_forward(ref0, ref2, flow0, flow2, filt0, filt2, blend, out0, out2, w0, w2):
    """out0 / out2 may be None."""
    dims = _fi_checks(ref0, flow0, filt0, None)
    if dims is None or not (_same_strides(ref0, ref2) and _same_strides(flow0, flow2) and _same_strides(filt0, filt2)):
        return 1
    outs = [t for t in (out0, out2) if t is not None]
    if not _nchw_ok(blend) or blend.shape != ref0.shape or not _addressed_as(blend, *outs):
        return 1
    b, c, h, w = dims
    null = ctypes.c_void_p(0)
    with torch.cuda.device(_on_gpu(torch.float32, ref0, ref2, flow0, flow2, filt0, filt2, blend, *outs)):
        return _finish(lib().vfi_filterinterp_blend_forward(
            _ptr(ref0), _ptr(ref2), _ptr(flow0), _ptr(flow2), _ptr(filt0), _ptr(filt2), _ptr(blend),
            _ptr(out0) if out0 is not None else null, _ptr(out2) if out2 is not None else null, b, c, h, w,
            filt0.size(1), w0, w2, _st(ref0), _st(flow0), _st(filt0), _st(blend), _stream(ref0)))


def rectify_head_forward_bf16(ref0, ref2, flow0, flow2, filt0, filt2, head, blend, w0, w2):
    """The first 3 C + 4 + 2 filter channels of a bfloat16 rectify buffer in one launch (vfi_rectify_head_forward_bf16): head
    (bfloat16, [B, 3 C + 4 + 2 filter channels, H, W], typically buf[:, :45]) receives bf16_rne of blend, out0, out2 of
    filterinterp_blend_forward and of the flows and filters; blend (float32, [B, C, H, W], or None) the unrounded blend.
    The inputs are float32.  The head has w stride 1 and the frames' row stride -- anything else is refused here (1), before the
    call; its batch and channel strides are free, and it needs 2-byte alignment only."""
    dims = _fi_checks(ref0, flow0, filt0, None)
    if dims is None or not (_same_strides(ref0, ref2) and _same_strides(flow0, flow2) and _same_strides(filt0, filt2)):
        return 1
    b, c, h, w = dims
    if not _fi_filter_ok(ref0, filt0) or head.dim() != 4 or tuple(head.shape) != (b, 3 * c + 4 + 2 * filt0.size(1), h, w) or \
            head.stride(3) != 1 or (h != 1 and head.stride(2) != ref0.stride(2)):      # (a one-row tensor's row stride addresses nothing)
        return 1
    if blend is not None and (blend.dim() != 4 or blend.shape != ref0.shape or blend.stride(3) != 1):
        return 1
    if _on_gpu(torch.float32, ref0, ref2, flow0, flow2, filt0, filt2, blend) != _dev(head, torch.bfloat16):
        raise RuntimeError("vfidkr_amd.cabi: tensors must live on one device")
    sh = _st(head)
    sh.h = ref0.stride(2)
    with torch.cuda.device(ref0.device):
        return _finish(lib().vfi_rectify_head_forward_bf16(
            _ptr(ref0), _ptr(ref2), _ptr(flow0), _ptr(flow2), _ptr(filt0), _ptr(filt2), _ptr(head),
            _ptr(blend) if blend is not None else ctypes.c_void_p(0), b, c, h, w, filt0.size(1), w0, w2, _st(ref0), _st(flow0),
            _st(filt0), sh, _st(blend if blend is not None else ref0), _stream(ref0)))


def filterinterp_blend_backward(ref0, ref2, flow0, flow2, filt0, filt2, grad_blend, grad_out0, grad_out2, w0, w2,
                                grad_ref0=None, grad_ref2=None, grad_flow0=None, grad_flow2=None, grad_filt0=None,
                                grad_filt2=None):
    """Backward of filterinterp_blend_forward: direction d's gradient is grad_blend * w_d + grad_out_d (None = an absent term).
    Gradient outputs that are None are not computed; the others are written in full (no zero fill needed) and share
    their input's layout.  The incoming gradients share one layout."""
    dims = _fi_checks(ref0, flow0, filt0, None)
    if dims is None or not (_same_strides(ref0, ref2) and _same_strides(flow0, flow2) and _same_strides(filt0, filt2)):
        return 1
    if not _fi_filter_ok(ref0, filt0):
        return 1
    grads = [t for t in (grad_blend, grad_out0, grad_out2) if t is not None]
    if grads and (not _nchw_ok(grads[0]) or grads[0].shape != ref0.shape or not _addressed_as(grads[0], *grads)):
        return 1
    if not _addressed_as(ref0, *[t for t in (grad_ref0, grad_ref2) if t is not None]) or \
            not _addressed_as(flow0, *[t for t in (grad_flow0, grad_flow2) if t is not None]) or \
            not _addressed_as(filt0, *[t for t in (grad_filt0, grad_filt2) if t is not None]):
        return 1
    b, c, h, w = dims
    outs = (grad_ref0, grad_ref2, grad_flow0, grad_flow2, grad_filt0, grad_filt2)
    null = ctypes.c_void_p(0)
    opt = lambda t: _ptr(t) if t is not None else null      # noqa: E731
    with torch.cuda.device(_on_gpu(torch.float32, ref0, ref2, flow0, flow2, filt0, filt2, *grads, *outs)):
        return _finish(lib().vfi_filterinterp_blend_backward(
            _ptr(ref0), _ptr(ref2), _ptr(flow0), _ptr(flow2), _ptr(filt0), _ptr(filt2), opt(grad_blend), opt(grad_out0),
            opt(grad_out2), *[opt(t) for t in outs], b, c, h, w, filt0.size(1), w0, w2, _st(ref0), _st(flow0), _st(filt0),
            _st(grads[0]) if grads else _st(ref0), _stream(ref0)))


def _warp_flow_dtype(x, flow):
    """The flow's dtype in a warp call: float32 with a float32 x; float32 or bfloat16, independently, with a bfloat16 x."""
    if x.dtype == torch.bfloat16 and flow.dtype == torch.bfloat16:
        return torch.bfloat16
    return torch.float32


def pwc_warp_forward(x, flow, output, align_corners=True):
    """float32, or bfloat16 x / output (vfi_pwc_warp_forward_bf16) with a float32 or a bfloat16 flow."""
    if not _is4(x) or not _nchw_ok(x, flow, output) or tuple(flow.shape) != (x.size(0), 2, x.size(2), x.size(3)) or \
            output.shape != x.shape:
        return 1
    b, c, h, w = x.shape
    fdtype = _warp_flow_dtype(x, flow)
    dtype, suffix = _bf16_or_f32(x, output)
    if _dev(flow, fdtype) != x.device:
        raise RuntimeError("vfidkr_amd.cabi: tensors must live on one device")
    with torch.cuda.device(x.device):
        if suffix:
            return _finish(lib().vfi_pwc_warp_forward_bf16(_ptr(x), _ptr(flow), int(fdtype == torch.bfloat16), _ptr(output), b, c, h, w,
                                                           int(bool(align_corners)), _st(x), _st(flow), _st(output),
                                                           _stream(x, dtype)))
        return _finish(lib().vfi_pwc_warp_forward(_ptr(x), _ptr(flow), _ptr(output), b, c, h, w, int(bool(align_corners)),
                                                  _st(x), _st(flow), _st(output), _stream(x)))


def pwc_warp_backward(x, flow, grad_output, grad_x=None, grad_flow=None, align_corners=True):
    """grad_x and / or grad_flow (written) of pwc_warp_forward; None = not computed.  float32: grad_x is added into
    (zero-fill it).  bfloat16 x / grad_output / grad_x (vfi_pwc_warp_backward_bf16): grad_x is WRITTEN in full; the flow is
    float32 or bfloat16 and grad_flow has its dtype."""
    grads = [t for t in (grad_x, grad_flow) if t is not None]
    if not _is4(x) or not _nchw_ok(x, flow, grad_output, *grads) or tuple(flow.shape) != (x.size(0), 2, x.size(2), x.size(3)) or \
            grad_output.shape != x.shape:
        return 1
    b, c, h, w = x.shape
    if (grad_x is not None and grad_x.shape != x.shape) or (grad_flow is not None and grad_flow.shape != flow.shape):
        return 1
    fdtype = _warp_flow_dtype(x, flow)
    dtype, suffix = _bf16_or_f32(x, grad_output, *([grad_x] if grad_x is not None else []))
    if _on_gpu(fdtype, flow, grad_flow) != x.device:
        raise RuntimeError("vfidkr_amd.cabi: tensors must live on one device")
    null = ctypes.c_void_p(0)
    with torch.cuda.device(x.device):
        tail = (_ptr(grad_output), _ptr(grad_x) if grad_x is not None else null,
                _ptr(grad_flow) if grad_flow is not None else null, b, c, h, w, int(bool(align_corners)), _st(x), _st(flow),
                _st(grad_output), _st(grad_x) if grad_x is not None else _st(x),
                _st(grad_flow) if grad_flow is not None else _st(flow), _stream(x, dtype))
        if suffix:
            return _finish(lib().vfi_pwc_warp_backward_bf16(_ptr(x), _ptr(flow), int(fdtype == torch.bfloat16), *tail))
        return _finish(lib().vfi_pwc_warp_backward(_ptr(x), _ptr(flow), *tail))


def pwc_warp_correlation_forward(input1, input2, flow, align_corners=True):
    """correlation(input1, warp(input2, flow)) of PWC-Net (pad 4, k 1, md 4, strides 1) in one launch; returns [B,81,h,w]."""
    _corr_inputs("pwc_warp_correlation_forward", input1, input2)
    input1, input2 = input1.contiguous(), input2.contiguous()
    b, c, h, w = input1.shape
    if tuple(input2.shape) != (b, c, h, w) or not _shaped(flow, b, 2, h, w) or flow.stride(3) != 1:
        raise RuntimeError("pwc_warp_correlation_forward: shape mismatch")
    _on_gpu(torch.float32, input1, input2, flow)
    output = torch.empty((b, 81, h, w), dtype=torch.float32, device=input1.device)
    with torch.cuda.device(_dev(input1)):
        err = _finish(lib().vfi_pwc_warp_correlation_forward(_ptr(input1), _ptr(input2), _ptr(flow), _ptr(output), b, c, h, w,
                                                             int(bool(align_corners)), _st(flow), _stream(input1)))
    if err != 0:
        raise RuntimeError("CUDA call failed")
    return output


def frame_u8_to_planar(src_hwc, dst, pad_left, pad_right, pad_top, pad_bottom):
    """src_hwc: dense uint8 [B,h,w,3]; dst: float32 [B,3,h+pt+pb,w+pl+pr]."""
    if not _is4(src_hwc) or not _nchw_ok(dst) or min(pad_left, pad_right, pad_top, pad_bottom) < 0:
        return 1
    b, h, w, c = src_hwc.shape
    if c != 3 or not src_hwc.is_contiguous():
        return 1
    if tuple(dst.shape) != (b, 3, h + pad_top + pad_bottom, w + pad_left + pad_right):
        return 1
    if _dev(dst) != _dev(src_hwc, torch.uint8):
        raise RuntimeError("vfidkr_amd.cabi: tensors must live on one device")
    with torch.cuda.device(src_hwc.device):
        return _finish(lib().vfi_frame_u8_to_planar(_ptr(src_hwc), _ptr(dst), b, h, w, pad_left, pad_right, pad_top,
                                                    pad_bottom, _st(dst), _stream(dst)))


def planar_to_frame_u8(src, dst_hwc, top, left):
    """src: float32 [B,3,H,W]; dst_hwc: dense uint8 [B,h,w,3], the crop at (top, left)."""
    if not _is4(dst_hwc, src):
        return 1
    b, h, w, c = dst_hwc.shape
    if c != 3 or not dst_hwc.is_contiguous() or src.stride(3) != 1 or src.size(0) != b or src.size(1) != 3:
        return 1
    if top < 0 or left < 0 or top + h > src.size(2) or left + w > src.size(3):
        return 1
    if _dev(dst_hwc, torch.uint8) != _dev(src):
        raise RuntimeError("vfidkr_amd.cabi: tensors must live on one device")
    with torch.cuda.device(src.device):
        return _finish(lib().vfi_planar_to_frame_u8(_ptr(src), _ptr(dst_hwc), b, h, w, top, left, _st(src),
                                                    _stream(src)))


def frame_error_sums(a, b, sums):
    """a, b: dense uint8 tensors of one shape; sums: int64[2] on the GPU, zeroed by the caller."""
    if a.shape != b.shape or a.numel() == 0 or not a.is_contiguous() or not b.is_contiguous() or sums.numel() < 2 or \
            not sums.is_contiguous():
        return 1
    if _dev(sums, torch.int64) != _on_gpu(torch.uint8, a, b):
        raise RuntimeError("vfidkr_amd.cabi: tensors must live on one device")
    with torch.cuda.device(a.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)
        return _finish(lib().vfi_frame_error_sums(_ptr(a), _ptr(b), a.numel(), _ptr(sums), stream))


def frame_ssim_sums(a, b, sums):
    """a, b: dense uint8 [B,h,w,3]; sums: int64[1] on the GPU, zeroed by the caller (2^-32 fixed point)."""
    if a.shape != b.shape or a.dim() != 4 or a.size(3) != 3 or not a.is_contiguous() or not b.is_contiguous():
        return 1
    if sums.numel() < 1 or a.numel() == 0 or not sums.is_contiguous():
        return 1
    if _dev(sums, torch.int64) != _on_gpu(torch.uint8, a, b):
        raise RuntimeError("vfidkr_amd.cabi: tensors must live on one device")
    with torch.cuda.device(a.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)
        return _finish(lib().vfi_frame_ssim_sums(_ptr(a), _ptr(b), a.size(0), a.size(1), a.size(2), _ptr(sums), stream))


# ---------------------------------------------------------------- training losses (loss_function.py: part_loss)

PART_LOSS_ITEMS = 8     # diffs per call of the library (LOSS_NMAX)


def _part_loss_checks(diffs, target, flow0, flow1, img0, img1):
    """(b, cd, ci, h, w) when the tensors of a part_loss call fit together, else None"""
    n = len(diffs)
    if n == 0 or n > PART_LOSS_ITEMS or (flow0 is None) != (flow1 is None):
        return None
    d0 = diffs[0]
    if not _nchw_ok(*diffs) or not _is4(d0) or not _addressed_as(d0, *diffs) or (target is not None and not _addressed_as(d0, target)):
        return None
    b, cd, h, w = d0.shape
    ci = 0
    if flow0 is not None:
        if img0 is None or img1 is None or not _nchw_ok(flow0, flow1, img0, img1):
            return None
        ci = img0.size(1)
        if tuple(flow0.shape) != (b, 2, h, w) or tuple(img0.shape) != (b, ci, h, w):
            return None
        if not _addressed_as(flow0, flow1) or not _addressed_as(img0, img1):
            return None
    return b, cd, ci, h, w


def _part_loss_on_device(*tensors):
    _on_gpu(torch.float32, *tensors)


def _opt(t):
    return ctypes.c_void_p(0) if t is None else _ptr(t)


def _opt_st(t, like=None):
    return _st(t) if t is not None else (_st(like) if like is not None else Strides(0, 0, 0))


def part_loss_forward(diffs, target, flow0, flow1, img0, img1, epsilon, neg_psnr, values, sample_means):
    """values[nd + 2] = the pixel losses of diffs (of diffs[i] - target with a target), the offset loss and the symmetry loss of
    the flow pair (zeros when flow0 / flow1 are None); sample_means[nd * B] = the per-sample Charbonnier means."""
    dims = _part_loss_checks(diffs, target, flow0, flow1, img0, img1)
    if dims is None:
        return 1
    b, cd, ci, h, w = dims
    n = len(diffs)
    if values.numel() != n + 2 or sample_means.numel() != n * b or not values.is_contiguous() or not sample_means.is_contiguous():
        return 1
    _part_loss_on_device(*diffs, target, flow0, flow1, *((img0, img1) if flow0 is not None else ()), values, sample_means)
    with torch.cuda.device(_dev(diffs[0])):
        return _finish(lib().vfi_part_loss_forward(
            _ptr_table(diffs), n, _opt(target), _opt(flow0), _opt(flow1), _opt(img0 if flow0 is not None else None),
            _opt(img1 if flow0 is not None else None), b, cd, ci, h, w, float(epsilon), int(bool(neg_psnr)), _ptr(values),
            _ptr(sample_means), _st(diffs[0]), _opt_st(flow0), _opt_st(img0 if flow0 is not None else None), _stream(diffs[0])))


def part_loss_backward(diffs, target, flow0, flow1, img0, img1, epsilon, neg_psnr, grad_values, sample_means, loss_mask,
                       grad_diffs=None, grad_flow0=None, grad_flow1=None):
    """The gradients of sum_j grad_values[j] * values[j] over the losses whose bit of loss_mask is set, into the tensors that
    are given: grad_diffs (None, or one tensor or None per diff; they share one layout), grad_flow0 / grad_flow1.  Given
    tensors are written in full."""
    dims = _part_loss_checks(diffs, target, flow0, flow1, img0, img1)
    if dims is None:
        return 1
    b, cd, ci, h, w = dims
    n = len(diffs)
    if grad_values.numel() != n + 2 or not grad_values.is_contiguous():
        return 1
    if neg_psnr and (sample_means is None or sample_means.numel() != n * b or not sample_means.is_contiguous()):
        return 1
    gds = [t for t in (grad_diffs or []) if t is not None]
    gfs = [t for t in (grad_flow0, grad_flow1) if t is not None]
    if (grad_diffs is not None and len(grad_diffs) != n) or (gfs and flow0 is None):
        return 1
    if not _nchw_ok(*gds, *gfs) or any(t.shape != diffs[0].shape for t in gds) or any(t.shape != flow0.shape for t in gfs):
        return 1
    if (gds and not _addressed_as(gds[0], *gds)) or (gfs and not _addressed_as(gfs[0], *gfs)):
        return 1
    _part_loss_on_device(*diffs, target, flow0, flow1, *((img0, img1) if flow0 is not None else ()), grad_values, sample_means,
                         *gds, *gfs)
    with torch.cuda.device(_dev(diffs[0])):
        return _finish(lib().vfi_part_loss_backward(
            _ptr_table(diffs), n, _opt(target), _opt(flow0), _opt(flow1), _opt(img0 if flow0 is not None else None),
            _opt(img1 if flow0 is not None else None), b, cd, ci, h, w, float(epsilon), int(bool(neg_psnr)), _ptr(grad_values),
            _opt(sample_means), int(loss_mask), None if grad_diffs is None else _ptr_table(grad_diffs), _opt(grad_flow0),
            _opt(grad_flow1), _st(diffs[0]), _opt_st(flow0), _opt_st(img0 if flow0 is not None else None),
            _opt_st(gds[0] if gds else None, diffs[0]), _opt_st(gfs[0] if gfs else None, flow0), _stream(diffs[0])))
