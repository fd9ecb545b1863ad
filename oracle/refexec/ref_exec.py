"""ctypes caller of oracle/_ref/libvfi_ref.so: the reference's own kernels, executed on the CPU.

TEST INFRASTRUCTURE ONLY.  Same function names and argument order as oracle/cpu_oracle.py (no `fmad`: the
executor is strict C, compiled with -ffp-contract=off), so a test can call both with one argument list.

    available()                    the library exists (built by build_ref.py when the reference checkout is there)
    set_order("blocks" | "raster") CUDA's block-major thread numbering, or whole-frame raster order
    canvas=True                    every tensor of the call lives inside a larger canvas (inputs NaN-filled, outputs
                                   zero-filled) and is handed to the launcher as a strided view, so a read outside
                                   any frame -- also one that merely wraps into the neighbouring row -- turns the
                                   element that used it into NaN.  The call then also returns the boolean mask(s)
                                   of those elements; `last_margin_writes` counts the canvas elements outside the
                                   frames that the call wrote.

What the reference's `*_cuda.cc` / `*Layer.py` wrappers do around the launchers is done here: zero-filled outputs
and gradients (e.g. FlowProjectionLayer.py:35-36, :69), filter_size = (int)sqrt(channels)
(filterinterpolation_cuda.cc:33-34; channels / 2 for the filterless variant, :395-396), the correlation's output
dims, NHWC rInput buffers and zero fills (correlation_cuda.cc:23-40, :97-113).
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(os.path.dirname(_HERE), "_ref", "libvfi_ref.so")
_lib = None
_IP = ctypes.POINTER(ctypes.c_int)

MARGIN = 8                 # canvas margin in pixels, every side (and guard rows above and below)
last_margin_writes = 0
_record = None             # a list while `recording()`: _call appends one job per launcher call for dump_jobs()


def available():
    return os.path.exists(_SO)


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(_SO)
    return _lib


def set_order(order):
    lib().vfi_ref_set_order({"blocks": 0, "raster": 1}[order])


def get_order():
    return ("blocks", "raster")[lib().vfi_ref_get_order()]


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _strides(a):
    assert all(s % 4 == 0 for s in a.strides) and a.dtype == np.float32 and a.ndim == 4
    return [s // 4 for s in a.strides]


def _root(a):
    while a.base is not None:
        a = a.base
    return a


def _call(name, ia, tensors):
    job = None
    if _record is not None:     # buffers as they are before the call, for the stand-alone program
        job = {"name": name, "ia": [int(v) for v in ia], "pre": [_root(t).copy() for t in tensors],
               "offset": [(t.ctypes.data - _root(t).ctypes.data) // 4 for t in tensors],
               "strides": [_strides(t) for t in tensors]}
    fn = getattr(lib(), "vfi_ref_" + name)
    n = len(tensors)
    ints = (ctypes.c_int * len(ia))(*[int(v) for v in ia])
    ptrs = (ctypes.c_void_p * n)(*[t.ctypes.data for t in tensors])
    keep = [(ctypes.c_int * 4)(*_strides(t)) for t in tensors]
    strides = (_IP * n)(*[ctypes.cast(k, _IP) for k in keep])
    err = fn(ints, ptrs, strides)
    if err != 0:
        raise RuntimeError("reference launcher %s returned %d" % (name, err))
    if job is not None:
        job["post"] = [_root(t).copy() for t in tensors]
        _record.append(job)


class _Frames:
    """Places the tensors of one call: plain contiguous arrays, or views into canvases."""

    def __init__(self, canvas, margin):
        self.canvas, self.m = bool(canvas), int(MARGIN if margin is None else margin)
        self.outs = []

    def _new(self, shape, fill):
        if not self.canvas:
            return np.full(shape, fill, np.float32)
        B, C, H, W = shape
        m = self.m
        base = np.full((B, C, H + 2 * m, W + 2 * m), fill, np.float32)
        return base[:, :, m:m + H, m:m + W]

    def put(self, a):
        """An input: its values, surrounded by NaN under canvas=True."""
        v = self._new(a.shape, np.nan)
        v[...] = a
        return v

    def out(self, shape, init=None):
        """An output (zero-filled like the reference's wrappers do), or an in/out tensor starting at `init`."""
        v = self._new(tuple(shape), 0.0)
        if init is not None:
            v[...] = init
        self.outs.append(v)
        return v

    def finish(self, *views, pixel_mask=False):
        """Contiguous copies of the outputs; under canvas=True also their masks and the margin-write count."""
        global last_margin_writes
        res = [np.ascontiguousarray(v) for v in views]
        last_margin_writes = 0
        if not self.canvas:
            return res[0] if len(res) == 1 else tuple(res)
        for v in self.outs:
            base = v.base
            inside = np.zeros(base.shape, bool)
            m = self.m
            inside[:, :, m:m + v.shape[2], m:m + v.shape[3]] = True
            last_margin_writes += int(np.count_nonzero((base != 0) & ~inside))
        masks = [np.isnan(r) for r in res]
        if pixel_mask:                           # one thread per pixel: any NaN it produced marks the pixel
            px = np.zeros((res[0].shape[0], 1) + res[0].shape[2:], bool)
            for k in masks:
                if k.shape[2:] == px.shape[2:]:
                    px |= k.any(axis=1, keepdims=True)
            return tuple(res) + (px,)
        return tuple(res) + (masks[0] if len(masks) == 1 else tuple(masks),)


def _fs(channels):
    return int(np.sqrt(np.float32(channels)))


# ---------------------------------------------------------------- FilterInterpolation

def filterinterp_ori_fwd(img, flow, filt, canvas=False, margin=None):
    img, flow, filt = _f32(img), _f32(flow), _f32(filt)
    B, C, H, W = img.shape
    f = _Frames(canvas, margin)
    out = f.out(img.shape)
    _call("FilterInterpolationLayer_gpu_forward_kernel_ori", [W, H, C, B, _fs(filt.shape[1])],
          [f.put(img), f.put(flow), f.put(filt), out])
    return f.finish(out)


def filterinterp_ori_bwd(img, flow, filt, gout, canvas=False, margin=None):
    img, flow, filt, gout = _f32(img), _f32(flow), _f32(filt), _f32(gout)
    B, C, H, W = img.shape
    f = _Frames(canvas, margin)
    g1, g2, g3 = f.out(img.shape), f.out(flow.shape), f.out(filt.shape)
    _call("FilterInterpolationLayer_gpu_backward_kernel_ori", [W, H, C, B, _fs(filt.shape[1])],
          [f.put(img), f.put(flow), f.put(filt), f.put(gout), g1, g2, g3])
    return f.finish(g1, g2, g3, pixel_mask=True)


_DEFOR_FWD = ("FilterInterpolationLayer_gpu_forward_kernel", "FilterInterpolationLayer_gpu_forward_kernel_deforconv",
              "FilterInterpolationLayer_gpu_forward_kernel_nofilterwithdeforconv")
_DEFOR_BWD = ("FilterInterpolationLayer_gpu_backward_kernel", "FilterInterpolationLayer_gpu_backward_kernel_deforconv",
              "FilterInterpolationLayer_gpu_backward_kernel_nofilterwithdeforconv")


def filterinterp_defor_fwd(variant, img, flow, filt, off, canvas=False, margin=None):
    """variant 0: `_kernel` (image, flow, filter, offset); 1: `_deforconv`; 2: `_nofilterwithdeforconv` (filt ignored)."""
    img, flow, off = _f32(img), _f32(flow), _f32(off)
    B, C, H, W = img.shape
    f = _Frames(canvas, margin)
    out = f.out(img.shape)
    if variant != 2:
        filt = _f32(filt)
        _call(_DEFOR_FWD[variant], [W, H, C, B, _fs(filt.shape[1])],
              [f.put(img), f.put(flow), f.put(filt), f.put(off), out])
    else:
        _call(_DEFOR_FWD[2], [W, H, C, B, _fs(off.shape[1] // 2)], [f.put(img), f.put(flow), f.put(off), out])
    return f.finish(out)


def filterinterp_defor_bwd(variant, img, flow, filt, off, gout, canvas=False, margin=None):
    """Returns (gimg, gflow, gfilt or None, goff) and, under canvas=True, the per-pixel mask [B,1,H,W]."""
    img, flow, off, gout = _f32(img), _f32(flow), _f32(off), _f32(gout)
    B, C, H, W = img.shape
    f = _Frames(canvas, margin)
    g1, g2, g4 = f.out(img.shape), f.out(flow.shape), f.out(off.shape)
    if variant != 2:
        filt = _f32(filt)
        g3 = f.out(filt.shape)
        _call(_DEFOR_BWD[variant], [W, H, C, B, _fs(filt.shape[1])],
              [f.put(img), f.put(flow), f.put(filt), f.put(off), f.put(gout), g1, g2, g3, g4])
        r = f.finish(g1, g2, g3, g4, pixel_mask=True)
        return r
    _call(_DEFOR_BWD[2], [W, H, C, B, _fs(off.shape[1] // 2)],
          [f.put(img), f.put(flow), f.put(off), f.put(gout), g1, g2, g4])
    r = f.finish(g1, g2, g4, pixel_mask=True)
    return (r[0], r[1], None) + tuple(r[2:])


# ---------------------------------------------------------------- projections

def flowproj_fwd(flow, fillhole=1, canvas=False, margin=None):
    flow = _f32(flow)
    B, _, H, W = flow.shape
    f = _Frames(canvas, margin)
    count, out = f.out((B, 1, H, W)), f.out(flow.shape)
    _call("FlowProjection_gpu_forward_kernel", [W, H, 2, B, int(fillhole)], [f.put(flow), count, out])
    return f.finish(out, count)


def flowproj_bwd(flow, count, gout, canvas=False, margin=None):
    flow, count, gout = _f32(flow), _f32(count), _f32(gout)
    B, _, H, W = flow.shape
    f = _Frames(canvas, margin)
    g = f.out(flow.shape)
    _call("FlowProjection_gpu_backward_kernel", [W, H, 2, B], [f.put(flow), f.put(count), f.put(gout), g])
    return f.finish(g)


def _depth_fwd(name, flow, depth, fillhole, count0, canvas, margin):
    flow, depth = _f32(flow), _f32(depth)
    B, _, H, W = flow.shape
    f = _Frames(canvas, margin)
    count, out = f.out((B, 1, H, W), count0), f.out(flow.shape)
    _call(name, [W, H, 2, B, int(fillhole)], [f.put(flow), f.put(depth), count, out])
    return f.finish(out, count)


def _depth_bwd(name, flow, depth, count, out, gout, canvas, margin):
    flow, depth, count, out, gout = _f32(flow), _f32(depth), _f32(count), _f32(out), _f32(gout)
    B, _, H, W = flow.shape
    f = _Frames(canvas, margin)
    g1, g2 = f.out(flow.shape), f.out(depth.shape)
    _call(name, [W, H, 2, B], [f.put(flow), f.put(depth), f.put(count), f.put(out), f.put(gout), g1, g2])
    return f.finish(g1, g2)


def depthflowproj_fwd(flow, depth, fillhole=1, canvas=False, margin=None):
    return _depth_fwd("DepthFlowProjection_gpu_forward_kernel", flow, depth, fillhole, None, canvas, margin)


def depthflowproj_bwd(flow, depth, count, out, gout, canvas=False, margin=None):
    return _depth_bwd("DepthFlowProjection_gpu_backward_kernel", flow, depth, count, out, gout, canvas, margin)


def mindepthflowproj_fwd(flow, weight, fillhole=1, count0=None, canvas=False, margin=None):
    return _depth_fwd("minDepthFlowProjection_gpu_forward_kernel", flow, weight, fillhole, count0, canvas, margin)


def mindepthflowproj_bwd(flow, weight, count, gout, out=None, canvas=False, margin=None):
    """The launcher also takes the forward's output and returns a weight gradient (the oracle does neither):
    `out` defaults to zeros; returns gflow only, like the oracle."""
    out = np.zeros_like(_f32(flow)) if out is None else out
    r = _depth_bwd("minDepthFlowProjection_gpu_backward_kernel", flow, weight, count, out, gout, canvas, margin)
    return (r[0], r[2][0]) if canvas else r[0]


# ---------------------------------------------------------------- Interpolation, SeparableConv

def _interp(name, img, flow, canvas, margin):
    img, flow = _f32(img), _f32(flow)
    B, C, H, W = img.shape
    f = _Frames(canvas, margin)
    out = f.out(img.shape)
    _call(name, [W, H, C, B], [f.put(img), f.put(flow), out])
    return f.finish(out)


def _interp_bwd(name, img, flow, gout, canvas, margin):
    img, flow, gout = _f32(img), _f32(flow), _f32(gout)
    B, C, H, W = img.shape
    f = _Frames(canvas, margin)
    g1, g2 = f.out(img.shape), f.out(flow.shape)
    _call(name, [W, H, C, B], [f.put(img), f.put(flow), f.put(gout), g1, g2])
    return f.finish(g1, g2, pixel_mask=True)


def interp_fwd(img, flow, canvas=False, margin=None):
    return _interp("InterpolationLayer_gpu_forward_kernel", img, flow, canvas, margin)


def interp_bwd(img, flow, gout, canvas=False, margin=None):
    return _interp_bwd("InterpolationLayer_gpu_backward_kernel", img, flow, gout, canvas, margin)


def interpch_fwd(img, flow, canvas=False, margin=None):
    return _interp("InterpolationChLayer_gpu_forward_kernel", img, flow, canvas, margin)


def interpch_bwd(img, flow, gout, canvas=False, margin=None):
    return _interp_bwd("InterpolationChLayer_gpu_backward_kernel", img, flow, gout, canvas, margin)


def sepconv_fwd(img, v, h, canvas=False, margin=None):
    img, v, h = _f32(img), _f32(v), _f32(h)
    B, C, H, W = img.shape
    fs = v.shape[1]
    f = _Frames(canvas, margin)
    out = f.out((B, C, H - fs + 1, W - fs + 1))
    _call("SeparableConvLayer_gpu_forward_kernel", [W, H, C, B, fs], [f.put(img), f.put(v), f.put(h), out])
    return f.finish(out)


def sepconv_bwd(img, v, h, gout, canvas=False, margin=None):
    img, v, h, gout = _f32(img), _f32(v), _f32(h), _f32(gout)
    B, C, H, W = img.shape
    f = _Frames(canvas, margin)
    g1, g2, g3 = f.out(img.shape), f.out(v.shape), f.out(h.shape)
    _call("SeparableConvLayer_gpu_backward_kernel", [W, H, C, B, v.shape[1]],
          [f.put(img), f.put(v), f.put(h), f.put(gout), g1, g2, g3])
    return f.finish(g1, g2, g3)


def sepconvflow_fwd(v, h, H, W, canvas=False, margin=None):
    """input1 is used for its sizes only (SeparableConvFlowLayer.py): a one-channel image of zeros stands in."""
    v, h = _f32(v), _f32(h)
    B, fs = v.shape[0], v.shape[1]
    f = _Frames(canvas, margin)
    out = f.out((B, 2, H - fs + 1, W - fs + 1))
    _call("SeparableConvFlowLayer_gpu_forward_kernel", [W, H, 1, B, fs],
          [f.put(np.zeros((B, 1, H, W), np.float32)), f.put(v), f.put(h), out])
    return f.finish(out)


def sepconvflow_bwd(v, h, gflow, H, W, canvas=False, margin=None):
    v, h, gflow = _f32(v), _f32(h), _f32(gflow)
    B, fs = v.shape[0], v.shape[1]
    f = _Frames(canvas, margin)
    g1, g2, g3 = f.out((B, 1, H, W)), f.out(v.shape), f.out(h.shape)
    _call("SeparableConvFlowLayer_gpu_backward_kernel", [W, H, 1, B, fs],
          [f.put(np.zeros((B, 1, H, W), np.float32)), f.put(v), f.put(h), f.put(gflow), g1, g2, g3])
    r = f.finish(g1, g2, g3)
    return (r[1], r[2], r[3][1:]) if canvas else (r[1], r[2])


# ---------------------------------------------------------------- correlation (fp32; at::Half is out of scope)

def correlation_out_dims(H, W, pad, k, md, s1, s2):
    """correlation_cuda.cc:23-32."""
    border = (k - 1) // 2 + md
    oc = (md // s2 * 2 + 1) ** 2
    oh = int(np.ceil(np.float32(H + 2 * pad - 2 * border) / np.float32(s1)))
    ow = int(np.ceil(np.float32(W + 2 * pad - 2 * border) / np.float32(s1)))
    return oc, oh, ow


def _rinput(B, C, H, W, pad, k, md):
    """The NHWC scratch the launchers repack into (correlation_cuda.cc:34-39: resized, zero-filled), with NaN in
    front of it and behind it: the kernels compute positions in it from blockIdx alone, and for some
    configurations those leave it (see correlation_fwd)."""
    n = B * (H + 2 * pad) * (W + 2 * pad) * C
    guard = (md + (k - 1) // 2 + 2) * (W + 2 * pad) * C
    base = np.full(n + 2 * guard, np.nan, np.float32)
    base[guard:guard + n] = 0
    return base[guard:guard + n].reshape(B, H + 2 * pad, W + 2 * pad, C)


def correlation_fwd(f1, f2, pad=4, k=1, md=4, s1=1, s2=1, canvas=False):
    """The launcher takes strides and ignores them (every tensor is addressed as dense), so there is no canvas for
    the features.  Its scratch always has NaN guards: with kernel_size > 1 the kernel starts its window at
    max_displacement instead of max_displacement + kernel_radius (correlation_cuda_kernel.cu:90-91), so the top
    output row of batch item 0 reads the rows in front of the scratch.  canvas=True also returns that mask."""
    f1, f2 = _f32(f1), _f32(f2)
    B, C, H, W = f1.shape
    oc, oh, ow = correlation_out_dims(H, W, pad, k, md, s1, s2)
    out = np.zeros((B, oc, oh, ow), np.float32)
    r1, r2 = _rinput(B, C, H, W, pad, k, md), _rinput(B, C, H, W, pad, k, md)
    _call("correlation_forward_cuda_kernel", [B, C, H, W, oc, oh, ow, pad, k, md, s1, s2], [f1, f2, out, r1, r2])
    return (out, np.isnan(out)) if canvas else out


def correlation_bwd(f1, f2, gout, pad=4, k=1, md=4, s1=1, s2=1, canvas=False):
    """stride1 == 1 only: the kernels index gradInput by blockIdx * stride1 (correlation_cuda_kernel.cu:163-164,
    :237), which writes past the tensor for stride1 > 1 -- not run."""
    if s1 != 1:
        raise ValueError("the reference's correlation backward writes outside gradInput for stride1 > 1")
    f1, f2, gout = _f32(f1), _f32(f2), _f32(gout)
    B, C, H, W = f1.shape
    oc, oh, ow = gout.shape[1:]
    g1, g2 = np.zeros_like(f1), np.zeros_like(f2)
    r1, r2 = _rinput(B, C, H, W, pad, k, md), _rinput(B, C, H, W, pad, k, md)
    _call("correlation_backward_cuda_kernel", [B, C, H, W, oc, oh, ow, pad, k, md, s1, s2],
          [f1, f2, gout, g1, g2, r1, r2])
    return (g1, g2, (np.isnan(g1), np.isnan(g2))) if canvas else (g1, g2)


# ---------------------------------------------------------------- jobs for the sanitized stand-alone program

class recording:
    """with recording() as jobs: ... -- every launcher call in the block is also kept for dump_jobs()."""

    def __enter__(self):
        global _record
        _record = []
        return _record

    def __exit__(self, *exc):
        global _record
        _record = None


def dump_jobs(jobs, directory, order="blocks"):
    """Writes jobs.txt and, per job and tensor, the whole buffer as it was before the call (raw float32) for
    oracle/refexec/selfcheck.cpp, which writes each buffer back as `<file>.out` after the call.  Returns the
    path of jobs.txt; compare `<file>.out` with job["post"][i]."""
    lines = ["%d %d" % (len(jobs), {"blocks": 0, "raster": 1}[order])]
    for j, job in enumerate(jobs):
        lines.append("%s %d %s %d" % (job["name"], len(job["ia"]), " ".join(str(v) for v in job["ia"]),
                                      len(job["pre"])))
        for i, root in enumerate(job["pre"]):
            fn = "j%d_t%d.bin" % (j, i)
            np.ascontiguousarray(root).tofile(os.path.join(directory, fn))
            lines.append("%d %d %s %s" % (root.size, job["offset"][i], " ".join(str(v) for v in job["strides"][i]),
                                          fn))
    path = os.path.join(directory, "jobs.txt")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return path
