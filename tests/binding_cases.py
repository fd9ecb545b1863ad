"""The contract of the tensor bindings (vfidkr_amd.cabi), as one table, and the mismatched calls generated from it.

Every public wrapper of cabi.py (minus EXCLUDED) has at least one Case: how to make a valid call from fake tensors at a small,
unsymmetric shape; which library entries that call reaches, with which integer arguments and stride structs; and for every
tensor (or list-of-tensors) parameter its Role -- the dtype it must have, each of its sizes as an expression of the shape
constants ENV (or free), whether its innermost stride must be 1, whose strides the library addresses it with, and whether it
may be None.  The relations are those of what the C entry addresses (include/vfi_hip.h and the kernels' indexing), not of what
a wrapper happens to check.

mutations(case) turns each Role into one-argument-wrong calls: a dtype, a device, a rank, every fixed size +1 and -1 as a
narrowed / widened VIEW with the valid tensor's strides, a zero batch, the layout relations one stride at a time, and the
list forms.  The expected outcome depends on the kind alone:

  shape, rank, layout, list   a wrapper that returns a status returns 1; one that returns tensors or a value raises RuntimeError
  dtype, device               RuntimeError

and in every case no library entry is reached (the two pure host functions HOST_ONLY apart).

No test functions here, and the product is not imported when this module is: tests/test_binding_refusals_host.py (fakes, the
library stubbed) and tests/test_gpu_binding_refusals.py (real tensors) use it.
"""
import collections
import itertools

import torch

from tests.test_corr_bf16_host import _FakeCuda

EXCLUDED = ["lib", "version", "correlation_output_dims", "projection_reserve", "release_workspaces"]
HOST_ONLY = ("vfi_correlation_output_dims", "vfi_version")

# b, c, h, w are all different and the frame is not square, so that a swapped dimension shows.  fs / oh / ow: SeparableConv's
# filter size and its output (h - fs + 1, w - fs + 1); hq / wq: a quarter-resolution flow; oc: PWC's 81 displacements;
# hh / hw: a cropped uint8 frame; the pads of frame_u8_to_planar
ENV = dict(b=2, c=3, h=6, w=10, fc=16, n=4, fs=3, oh=4, ow=8, hq=3, wq=5, oc=81, ci=4, hh=4, hw=7,
           pl=1, pr=2, pt=3, pb=1, top=1, left=2)
PWC = (4, 1, 4, 1, 1)       # pad_size, kernel_size, max_displacement, stride1, stride2: [b, 81, h, w]
F32, F16, BF16, U8, I64 = "float32", "float16", "bfloat16", "uint8", "int64"
WRONG_DTYPES = {F32: ("float64", F16), F16: ("float64", F32), BF16: ("float64", F32), U8: ("float64",), I64: ("float64",)}


class Role:
    """One tensor parameter.  sizes: one token per dimension -- an expression of ENV (the size is fixed), `*expr` (free; expr is
    the valid call's size) or `>=expr` (at least; the valid call has exactly that).  inner: the dimension whose stride must be
    1 (3: the NCHW bindings' w; 1: a channels_last image; None: any), `dense`: contiguous in full.  as_: the parameter (or
    `name.0`, the first item of a list) with whose strides the library addresses this tensor; row_as: the same for the row
    stride alone.  opt: may be None.  used=False: accepted and never looked at (the reference passes it)."""

    def __init__(self, sizes, dtype=F32, inner=3, dense=False, as_=None, row_as=None, opt=False, used=True, present=True,
                 channels_last=False, wrong=None):
        self.sizes, self.dtype, self.inner, self.dense = sizes.split(), dtype, (None if dense else inner), dense
        self.as_, self.row_as, self.opt, self.used, self.present, self.channels_last = as_, row_as, opt, used, present, channels_last
        self.wrong = WRONG_DTYPES[dtype] if wrong is None else wrong
        assert present or opt

    def shape(self):
        return tuple(eval(s.lstrip("*>="), {}, ENV) for s in self.sizes)


class Items:
    """A list-of-tensors parameter: n items of one Role that share one layout (item.as_ = None: the first item's).
    none_items: an item may be None; opt: the whole list may be None."""

    def __init__(self, item, n=None, opt=False, none_items=False, present=True):
        self.item, self.n, self.opt, self.none_items, self.present = item, ENV["n"] if n is None else n, opt, none_items, present
        self.fixed_length = n is not None


T, L = Role, Items
Case = collections.namedtuple("Case", "wrapper name args calls returns")
Call = collections.namedtuple("Call", "entry ints strides")      # strides: parameter references, `name` or `name.k`
CASES = []


def case(wrapper, name, args, *calls, returns="status"):
    CASES.append(Case(wrapper, name, args, [Call(*c) for c in calls], returns))


def _img(**kw):
    return T("b c h w", **kw)


def _flow(**kw):
    return T("b 2 h w", **kw)


def _filt(**kw):
    return T("b *fc h w", **kw)


def _plane(**kw):
    return T("b 1 h w", **kw)


# ---------------------------------------------------------------- FilterInterpolation
case("filterinterp_forward_ori", "f32",
     dict(input1=_img(), input2=_flow(), input3=_filt(), output=_img(as_="input1"), direct=False),
     ("vfi_filterinterp_forward_ori", "b c h w fc", "input1 input2 input3"))
case("filterinterp_forward_ori", "direct",
     dict(input1=_img(), input2=_flow(), input3=_filt(), output=_img(as_="input1"), direct=True),
     ("vfi_filterinterp_forward_ori_direct", "b c h w fc", "input1 input2 input3"))
case("filterinterp_forward_ori_f16", "f16",
     dict(input1=_img(dtype=F16), input2=_flow(), input3=_filt(), output=_img(dtype=F16, as_="input1"), direct=False),
     ("vfi_filterinterp_forward_ori_f16", "b c h w fc", "input1 input2 input3"))
for _dt, _sfx in ((F32, ""), (BF16, "_bf16")):
    case("filterinterp_forward_ori_multi", _dt,
         dict(input1=_img(dtype=_dt), flows=L(_flow()), input3=_filt(), outputs=L(_img(dtype=_dt, as_="input1"))),
         ("vfi_filterinterp_forward_ori_multi" + ("_to_bf16" if _sfx else ""), "n b c h w fc",
          "input1 flows.0 input3" + (" input1" if _sfx else "")))
    case("filterinterp_forward_ori_multi_to", _dt,
         dict(input1=_img(dtype=_dt), flows=L(_flow()), input3=_filt(), outputs=L(_img(dtype=_dt, row_as="input1")), direct=False),
         ("vfi_filterinterp_forward_ori_multi_to" + _sfx, "n b c h w fc", "input1 flows.0 input3 outputs.0"))
    case("filterinterp_forward_nhwc_multi_to", _dt,
         dict(image=_img(dtype=_dt, inner=1, channels_last=True), flows=L(_flow(inner=None)), filt=_filt(inner=None),
              outs=L(_img(dtype=_dt, inner=1, channels_last=True))),
         ("vfi_filterinterp_forward_ori_nhwc_multi_to" + _sfx, "n b c h w fc", "image flows.0 filt outs.0"))
    case("filterinterp_backward_ori_image_multi", _dt,
         dict(flows=L(_flow()), input3=_filt(), gradoutputs=L(_img(dtype=_dt)), gradinput1=_img(dtype=_dt)),
         ("vfi_filterinterp_backward_ori_image_multi" + _sfx, "n b c h w fc", "gradinput1 flows.0 input3 gradoutputs.0"))
case("filterinterp_nhwc_access_width", "f32",
     dict(image=_img(inner=1, channels_last=True), filt=_filt(inner=None), outs=L(_img(inner=1, channels_last=True))),
     ("vfi_filterinterp_nhwc_access_width", "4 n b h w fc", "image outs.0"), returns="value")
case("filterinterp_backward_ori", "f32",
     dict(input1=_img(), input2=_flow(), input3=_filt(), gradoutput=_img(as_="input1"), gradinput1=_img(as_="input1"),
          gradinput2=_flow(as_="input2"), gradinput3=_filt(as_="input3")),
     ("vfi_filterinterp_backward_ori", "b c h w fc", "input1 input2 input3"))
# the deformable variants: input3 = the fs * fs taps and input4 = the 2 * fs * fs offsets; without a filter input3 = the offsets
# (filter_size = (int)sqrt(input3.size(1) [/ 2]), as the reference binding computes it: input3's channel count is free)
for _v, _vn in ((0, "offset"), (1, "region")):
    case("filterinterp_forward_defor", _vn,
         dict(variant=_v, input1=_img(), input2=_flow(), input3=_filt(), input4=T("b >=2*fc h w", opt=True),
              output=_img(as_="input1"), general=False),
         ("vfi_filterinterp_forward_defor", "%d b c h w 4" % _v, "input1 input2 input3 input4"))
    case("filterinterp_backward_defor", _vn,
         dict(variant=_v, input1=_img(), input2=_flow(), input3=_filt(), input4=T("b >=2*fc h w", opt=True),
              gradoutput=_img(as_="input1"), gradinput1=_img(as_="input1"), gradinput2=_flow(as_="input2"),
              gradinput3=_filt(as_="input3"), gradinput4=T("b >=2*fc h w", as_="input4", opt=True)),
         ("vfi_filterinterp_backward_defor", "%d b c h w 4" % _v, "input1 input2 input3 input4"))
case("filterinterp_forward_defor", "nofilter",
     dict(variant=2, input1=_img(), input2=_flow(), input3=T("b *2*fc h w"), input4=T("b >=2*fc h w", opt=True, present=False),
          output=_img(as_="input1"), general=True),
     ("vfi_filterinterp_forward_defor_general", "2 b c h w 4", "input1 input2 input3 input3"))
case("filterinterp_backward_defor", "nofilter",
     dict(variant=2, input1=_img(), input2=_flow(), input3=T("b *2*fc h w"), input4=T("b >=2*fc h w", opt=True, present=False),
          gradoutput=_img(as_="input1"), gradinput1=_img(as_="input1"), gradinput2=_flow(as_="input2"),
          gradinput3=T("b *2*fc h w", as_="input3"), gradinput4=T("b >=2*fc h w", as_="input4", opt=True, present=False)),
     ("vfi_filterinterp_backward_defor", "2 b c h w 4", "input1 input2 input3 input3"))

# ---------------------------------------------------------------- the projections
case("flowprojection_forward", "f32",
     dict(input1=_flow(), count=_plane(), output=_flow(as_="input1"), fillhole=1),
     ("vfi_flowprojection_forward", "b h w 1", "input1 count"))
case("flowprojection_forward_batch", "flow",
     dict(inputs1=L(_flow()), counts=L(_plane()), outputs=L(_flow(as_="inputs1.0")), fillhole=1,
          inputs2=L(_plane(), opt=True, present=False)),
     ("vfi_flowprojection_forward_batch", "n b h w 1", "inputs1.0 counts.0"))
case("flowprojection_forward_batch", "depth",
     dict(inputs1=L(_flow()), counts=L(_plane()), outputs=L(_flow(as_="inputs1.0")), fillhole=0, inputs2=L(_plane(), opt=True)),
     ("vfi_depthflowprojection_forward_batch", "n b h w 0", "inputs1.0 inputs2.0 counts.0"))
case("flowprojection_backward", "f32",
     dict(input1=_flow(), count=_plane(), gradoutput=_flow(as_="input1"), gradinput1=_flow(as_="input1")),
     ("vfi_flowprojection_backward", "b h w", "input1 count"))
for _w in ("depthflowprojection", "mindepthflowprojection"):
    case(_w + "_forward", "f32",
         dict(input1=_flow(), input2=_plane(), count=_plane(), output=_flow(as_="input1"), fillhole=1),
         ("vfi_%s_forward" % _w, "b h w 1", "input1 input2 count"))
case("depthflowprojection_backward", "f32",
     dict(input1=_flow(), input2=_plane(), count=_plane(), output=_flow(as_="input1"), gradoutput=_flow(as_="input1"),
          gradinput1=_flow(as_="input1"), gradinput2=_plane(as_="input2")),
     ("vfi_depthflowprojection_backward", "b h w", "input1 input2 count"))
case("mindepthflowprojection_backward", "f32",      # (output and gradinput2: passed by the reference's wrapper, never read or written)
     dict(input1=_flow(), input2=_plane(), count=_plane(), output=_flow(used=False), gradoutput=_flow(as_="input1"),
          gradinput1=_flow(as_="input1"), gradinput2=_plane(used=False)),
     ("vfi_mindepthflowprojection_backward", "b h w", "input1 input2 count"))

# ---------------------------------------------------------------- Interpolation, SeparableConv[Flow]
case("interpolation_forward", "f32",
     dict(input1=_img(), input2=_flow(), output=_img(as_="input1"), require_c3=True),
     ("vfi_interpolation_forward", "b c h w", "input1 input2"))
case("interpolation_backward", "f32",
     dict(input1=_img(), input2=_flow(), gradoutput=_img(as_="input1"), gradinput1=_img(as_="input1"),
          gradinput2=_flow(as_="input2"), require_c3=False),
     ("vfi_interpolation_backward", "b c h w", "input1 input2"))


def _taps(**kw):
    return T("b fs oh ow", **kw)


case("separableconv_forward", "f32",
     dict(input1=_img(), input2=_taps(), input3=_taps(), output=T("b c oh ow"), require_c3=True),
     ("vfi_separableconv_forward", "b c h w fs", "input1 input2 input3 output"))
case("separableconv_backward", "f32",
     dict(input1=_img(), input2=_taps(), input3=_taps(), gradoutput=T("b c oh ow"), gradinput1=_img(as_="input1"),
          gradinput2=_taps(as_="input2"), gradinput3=_taps(as_="input3"), require_c3=True),
     ("vfi_separableconv_backward", "b c h w fs", "input1 input2 input3 gradoutput"))
case("separableconvflow_forward", "f32",      # (input1 gives the frame's size alone: the image does not enter the flow)
     dict(input1=_img(), input2=_taps(), input3=_taps(), flow_output=T("b 2 oh ow"), require_c3=True),
     ("vfi_separableconvflow_forward", "b h w fs", "input2 input3 flow_output"))
case("separableconvflow_backward", "f32",
     dict(input1=_img(), input2=_taps(), input3=_taps(), gradflow_output=T("b 2 oh ow"), gradinput2=_taps(as_="input2"),
          gradinput3=_taps(as_="input3"), require_c3=True),
     ("vfi_separableconvflow_backward", "b h w fs", "input2 input3 gradflow_output"))

# ---------------------------------------------------------------- correlation (the wrappers make their inputs contiguous: any strides)


def _feat(dtype=F32, **kw):
    return T("b c h w", dtype=dtype, inner=None, **kw)


def _cost(dtype=F32, **kw):
    return T("b oc h w", dtype=dtype, inner=None, **kw)


_P = dict(zip(("pad_size", "kernel_size", "max_displacement", "stride1", "stride2"), PWC))
_PI = " 4 1 4 1 1"
for _dt, _sfx in ((F32, ""), (F16, "_f16"), (BF16, "_bf16")):
    case("correlation_forward", _dt, dict(input1=_feat(_dt), input2=_feat(_dt), **_P),
         ("vfi_correlation_forward" + _sfx, "b c h w" + _PI, ""), returns="value")
    case("correlation_backward", _dt, dict(input1=_feat(_dt), input2=_feat(_dt), gradoutput=_cost(_dt), **_P),
         ("vfi_correlation_backward" + _sfx, "b c h w" + _PI, ""), returns="value")
case("correlation_forward_bf16_kernel", "generic",
     dict(which="generic", input1=_feat(BF16), input2=_feat(BF16), **_P, out=T("b oc h w", dtype=BF16, dense=True, opt=True)),
     ("vfi_correlation_forward_bf16_kernel", "1 b c h w" + _PI, ""), returns="value")
for _dt, _sfx in ((F32, ""), (BF16, "_bf16")):
    case("correlation_forward_pair", _dt, dict(a1=_feat(_dt), a2=_feat(_dt), b1=_feat(_dt), b2=_feat(_dt), **_P),
         ("vfi_correlation_forward_pair" + _sfx, "b c h w" + _PI, ""), returns="value")
    case("correlation_backward_pair", _dt,
         dict(a1=_feat(_dt), a2=_feat(_dt), ga=_cost(_dt, opt=True), b1=_feat(_dt), b2=_feat(_dt), gb=_cost(_dt, opt=True), **_P,
              want=(True, True, True, True)),
         ("vfi_correlation_backward_pair" + _sfx, "b c h w" + _PI, ""), returns="value")
    # out=: planes dense, any batch stride (the fake's is the dense one)
    case("correlation_lrelu_forward", _dt,
         dict(input1=_feat(_dt), input2=_feat(_dt), **_P, negative_slope=0.1, out=T("b oc h w", dtype=_dt, opt=True)),
         ("vfi_correlation_lrelu_forward" + _sfx, "b c h w" + _PI, ""), returns="value")
    case("correlation_lrelu_forward_pair", _dt,
         dict(a1=_feat(_dt), a2=_feat(_dt), b1=_feat(_dt), b2=_feat(_dt), **_P, negative_slope=0.1,
              out=L(T("b oc h w", dtype=_dt, as_="-"), n=2, opt=True, none_items=True)),
         ("vfi_correlation_lrelu_forward_pair" + _sfx, "b c h w" + _PI, ""), returns="value")
    case("correlation_lrelu_backward", _dt,
         dict(input1=_feat(_dt), input2=_feat(_dt), y=_cost(_dt), gradoutput=_cost(_dt), **_P, negative_slope=0.1),
         ("vfi_correlation_lrelu_backward" + _sfx, "b c h w" + _PI, ""), returns="value")
    case("correlation_lrelu_backward_pair", _dt,
         dict(a1=_feat(_dt), a2=_feat(_dt), ya=_cost(_dt, opt=True), ga=_cost(_dt, opt=True), b1=_feat(_dt), b2=_feat(_dt),
              yb=_cost(_dt, opt=True), gb=_cost(_dt, opt=True), **_P, negative_slope=0.1, want=(True, True, True, True)),
         ("vfi_correlation_lrelu_backward_pair" + _sfx, "b c h w" + _PI, ""), returns="value")
case("pwc_warp_correlation_forward", "f32",
     dict(input1=_feat(), input2=_feat(), flow=_flow(), align_corners=True),
     ("vfi_pwc_warp_correlation_forward", "b c h w 1", "flow"), returns="value")

# ---------------------------------------------------------------- the glue: x4 upsampling, blend, warp, frames


def _q(ch, **kw):
    return T("b %s hq wq" % ch, **kw)


def _full(ch, **kw):
    return T("b %s 4*hq 4*wq" % ch, **kw)


case("flow_upsample4", "f32", dict(input=_q("c"), output=_full("c"), mul0=0.5, mul1=2.0),
     ("vfi_flow_upsample4", "b c hq wq", "input output"))
case("flowprojection_forward_up4", "f32",
     dict(flow_q=_q(2), count=_full(1), output=_full(2), mul0=0.5, mul1=2.0, fillhole=1),
     ("vfi_flowprojection_forward_up4", "b hq wq 1", "flow_q count output"))
case("depthflowprojection_forward_up4", "f32",
     dict(flow_q=_q(2), input2=_full(1), count=_full(1), output=_full(2), mul0=0.5, mul1=2.0, fillhole=1),
     ("vfi_depthflowprojection_forward_up4", "b hq wq 1", "flow_q input2 count output"))
case("flow_upsample4_backward", "f32",
     dict(grads_full=L(_full("c")), mul0=0.5, mul1=[1.0, 2.0, 3.0, 4.0], grad_q=_q("c")),
     ("vfi_flow_upsample4_backward", "n b c hq wq", "grads_full.0 grad_q"))
case("flowprojection_backward_up4", "flow",
     dict(flow_q=_q(2), counts=L(_full(1)), gradoutputs=L(_full(2)), mul0=0.5, mul1=[1.0, 2.0, 3.0, 4.0], grad_q=_q(2),
          depths=L(_full(1), opt=True, present=False), outputs=L(_full(2, as_="gradoutputs.0"), opt=True, present=False),
          grad_depths=L(_full(1, as_="depths.0"), opt=True, none_items=True, present=False)),
     ("vfi_flowprojection_backward_up4", "n b hq wq", "flow_q counts.0 gradoutputs.0 grad_q"))
case("flowprojection_backward_up4", "depth",
     dict(flow_q=_q(2), counts=L(_full(1)), gradoutputs=L(_full(2)), mul0=0.5, mul1=[1.0, 2.0, 3.0, 4.0], grad_q=_q(2),
          depths=L(_full(1), opt=True), outputs=L(_full(2, as_="gradoutputs.0"), opt=True),
          grad_depths=L(_full(1, as_="depths.0"), opt=True, none_items=True)),
     ("vfi_depthflowprojection_backward_up4", "n b hq wq", "flow_q depths.0 counts.0 gradoutputs.0 grad_q"))

_PAIR = dict(ref0=_img(), ref2=_img(as_="ref0"), flow0=_flow(), flow2=_flow(as_="flow0"), filt0=_filt(), filt2=_filt(as_="filt0"))
case("filterinterp_blend_forward", "f32",
     dict(_PAIR, blend=_img(), out0=_img(as_="blend", opt=True), out2=_img(as_="blend", opt=True), w0=0.25, w2=0.75),
     ("vfi_filterinterp_blend_forward", "b c h w fc", "ref0 flow0 filt0 blend"))
case("rectify_head_forward_bf16", "bf16",
     dict(_PAIR, head=T("b 3*c+4+2*fc h w", dtype=BF16, row_as="ref0"), blend=_img(opt=True), w0=0.25, w2=0.75),
     ("vfi_rectify_head_forward_bf16", "b c h w fc", "ref0 flow0 filt0 head blend"))
case("filterinterp_blend_backward", "f32",
     dict(_PAIR, grad_blend=_img(opt=True), grad_out0=_img(as_="grad_blend", opt=True), grad_out2=_img(as_="grad_blend", opt=True),
          w0=0.25, w2=0.75, grad_ref0=_img(as_="ref0", opt=True), grad_ref2=_img(as_="ref0", opt=True),
          grad_flow0=_flow(as_="flow0", opt=True), grad_flow2=_flow(as_="flow0", opt=True),
          grad_filt0=_filt(as_="filt0", opt=True), grad_filt2=_filt(as_="filt0", opt=True)),
     ("vfi_filterinterp_blend_backward", "b c h w fc", "ref0 flow0 filt0 grad_blend"))
for _dt, _fdt, _sfx, _flag in ((F32, F32, "", ""), (BF16, F32, "_bf16", "0 "), (BF16, BF16, "_bf16", "1 ")):
    _n = _dt + ("" if _fdt == _dt else "_flow_" + _fdt)
    _fw = ("float64", F16) if _fdt == BF16 else None       # (a float32 flow under a bfloat16 image is a valid call)
    case("pwc_warp_forward", _n,
         dict(x=_img(dtype=_dt), flow=_flow(dtype=_fdt, wrong=_fw), output=_img(dtype=_dt), align_corners=False),
         ("vfi_pwc_warp_forward" + _sfx, _flag + "b c h w 0", "x flow output"))
    case("pwc_warp_backward", _n,
         dict(x=_img(dtype=_dt), flow=_flow(dtype=_fdt, wrong=_fw), grad_output=_img(dtype=_dt), grad_x=_img(dtype=_dt, opt=True),
              grad_flow=_flow(dtype=_fdt, opt=True), align_corners=True),
         ("vfi_pwc_warp_backward" + _sfx, _flag + "b c h w 1", "x flow grad_output grad_x grad_flow"))
case("frame_u8_to_planar", "u8",
     dict(src_hwc=T("b h w 3", dtype=U8, dense=True), dst=T("b 3 h+pt+pb w+pl+pr"), pad_left=ENV["pl"], pad_right=ENV["pr"],
          pad_top=ENV["pt"], pad_bottom=ENV["pb"]),
     ("vfi_frame_u8_to_planar", "b h w pl pr pt pb", "dst"))
case("planar_to_frame_u8", "u8",
     dict(src=T("b 3 >=top+hh >=left+hw"), dst_hwc=T("b hh hw 3", dtype=U8, dense=True), top=ENV["top"], left=ENV["left"]),
     ("vfi_planar_to_frame_u8", "b hh hw top left", "src"))
case("frame_error_sums", "u8",
     dict(a=T("b h w 3", dtype=U8, dense=True), b=T("b h w 3", dtype=U8, dense=True), sums=T(">=2", dtype=I64, dense=True)),
     ("vfi_frame_error_sums", "", ""))
case("frame_ssim_sums", "u8",
     dict(a=T("b h w 3", dtype=U8, dense=True), b=T("b h w 3", dtype=U8, dense=True), sums=T(">=1", dtype=I64, dense=True)),
     ("vfi_frame_ssim_sums", "b h w", ""))

# ---------------------------------------------------------------- the training losses
_LOSS = dict(diffs=L(_img()), target=_img(as_="diffs.0", opt=True), flow0=_flow(opt=True), flow1=_flow(as_="flow0", opt=True),
             img0=T("b *ci h w", opt=True), img1=T("b *ci h w", as_="img0", opt=True), epsilon=1e-6, neg_psnr=True)
case("part_loss_forward", "f32",
     dict(_LOSS, values=T("n+2", dense=True), sample_means=T("n*b", dense=True)),
     ("vfi_part_loss_forward", "n b c ci h w 1", "diffs.0 flow0 img0"))
case("part_loss_backward", "f32",
     dict(_LOSS, grad_values=T("n+2", dense=True), sample_means=T("n*b", dense=True, opt=True), loss_mask=7,
          grad_diffs=L(_img(), opt=True, none_items=True), grad_flow0=_flow(opt=True), grad_flow1=_flow(as_="grad_flow0", opt=True)),
     ("vfi_part_loss_backward", "n b c ci h w 1", "diffs.0 flow0 img0 grad_diffs.0 grad_flow0"))


# ---------------------------------------------------------------- fake tensors

class FakeGpu(_FakeCuda):
    """_FakeCuda that also says WHICH device: cuda:index, or the CPU with is_cuda=False"""

    def __init__(self, t, is_cuda=True, index=0):
        super().__init__(t, is_cuda)
        self.device = torch.device("cuda", index) if is_cuda else torch.device("cpu")


def _dtype(name):
    return getattr(torch, name)


def _dense_strides(shape, channels_last=False):
    if channels_last:
        b, c, h, w = shape
        return (h * w * c, 1, w * c, c)
    return tuple(int(torch.tensor(shape[k + 1:]).prod()) for k in range(len(shape)))


def view(shape, strides, dtype, is_cuda=True, index=0):
    """a fake tensor of this shape and these strides inside an allocation of its own that covers every element"""
    extent = 1 + sum((n - 1) * s for n, s in zip(shape, strides) if n > 0)
    return FakeGpu(torch.zeros(extent + 8, dtype=_dtype(dtype)).as_strided(tuple(shape), tuple(strides)), is_cuda, index)


def valid_tensor(role, dtype=None):
    shape = role.shape()
    return view(shape, _dense_strides(shape, role.channels_last), dtype or role.dtype)


def valid_args(case_):
    """the keyword arguments of the case's valid call"""
    kw = {}
    for name, spec in case_.args.items():
        if isinstance(spec, Role):
            kw[name] = valid_tensor(spec) if spec.present else None
        elif isinstance(spec, Items):
            kw[name] = [valid_tensor(spec.item) for _ in range(spec.n)] if spec.present else None
        else:
            kw[name] = spec
    return kw


def resolve(kw, ref):
    """the tensor a strides reference (`name` or `name.k`) means"""
    name, _, k = ref.partition(".")
    return kw[name][int(k)] if k else kw[name]


# ---------------------------------------------------------------- mutations

Mutation = collections.namedtuple("Mutation", "param what kind apply")     # kind: shape | rank | layout | list | dtype | device


def _restride(t, shape=None, strides=None, **kw):
    return view(t.shape if shape is None else shape, t.stride() if strides is None else strides, str(t.dtype).replace("torch.", ""), **kw)


def tensor_mutations(role, layout_partner):
    """(what, kind, fn(valid fake) -> mutated fake) for one tensor of this Role; layout_partner: it shares its layout with
    another tensor (as_, or the first item of its list)"""
    if not role.used:
        return
    for wrong in role.wrong:
        yield "dtype_" + wrong, "dtype", lambda t, wrong=wrong: view(t.shape, t.stride(), wrong)
    yield "on_the_cpu", "device", lambda t: _restride(t, is_cuda=False)
    yield "on_gpu_1", "device", lambda t: _restride(t, index=1)
    if len(role.sizes) == 4:
        yield "rank_3", "rank", lambda t: _restride(t, t.shape[1:], t.stride()[1:])
    for d, token in enumerate(role.sizes):
        if token.startswith("*"):
            continue
        for delta in ((-1,) if token.startswith(">=") else (1, -1)):
            def resize(t, d=d, delta=delta):
                shape = list(t.shape)
                shape[d] += delta
                return _restride(t, shape)
            yield "size%d%+d" % (d, delta), "shape", resize
    yield "batch_0", "shape", lambda t: _restride(t, (0,) + tuple(t.shape[1:]))
    shape = role.shape()
    if role.dense and max(shape) > 1:                   # (a one-element tensor is dense whatever its strides say)
        yield "not_dense", "layout", lambda t: _restride(t, strides=(t.stride(0) + 1,) + tuple(t.stride()[1:]))
    elif role.inner is not None and shape[role.inner] != 1:
        def spread(t):
            s = [2 * v for v in t.stride()]
            return _restride(t, strides=s)
        yield "stride%d_2" % role.inner, "layout", spread
    if layout_partner or role.row_as:
        for d in ((2,) if not layout_partner else range(len(shape) - 1)):
            if shape[d] == 1 or d == role.inner:       # (the stride of a size-1 dimension is free)
                continue

            def shift(t, d=d):
                s = list(t.stride())
                s[d] += 4 if role.channels_last else 2       # (keeps the innermost stride and the alignment)
                return _restride(t, strides=s)
            yield "stride%d_differs" % d, "layout", shift


def mutations(case_):
    """every one-argument-wrong call of the case: Mutation.apply(kw) changes the valid keyword arguments in place"""
    for name, spec in case_.args.items():
        if isinstance(spec, Role) and spec.present:
            for what, kind, fn in tensor_mutations(spec, spec.as_ is not None):
                yield Mutation(name, what, kind, lambda kw, name=name, fn=fn: kw.__setitem__(name, fn(kw[name])))
        elif isinstance(spec, Items) and spec.present:
            last = spec.n - 1
            yield Mutation(name, "empty_list", "list", lambda kw, name=name: kw.__setitem__(name, []))
            # lengths that differ: from another list's (a list of factors included), or from the length the wrapper fixes
            if spec.fixed_length or sum(1 for v in case_.args.values() if isinstance(v, (Items, list)) and getattr(v, "present", True)) > 1:
                yield Mutation(name, "one_item_short", "list", lambda kw, name=name: kw.__setitem__(name, kw[name][:-1]))
                yield Mutation(name, "one_item_more", "list", lambda kw, name=name: kw.__setitem__(name, kw[name] + kw[name][-1:]))
            if not spec.none_items:
                yield Mutation(name, "item_none", "list", lambda kw, name=name: kw[name].__setitem__(last, None))
            for what, kind, fn in tensor_mutations(spec.item, spec.item.as_ != "-"):
                yield Mutation(name, "item%d_%s" % (last, what), kind,
                               lambda kw, name=name, fn=fn: kw[name].__setitem__(last, fn(kw[name][last])))


def expected(case_, kind):
    """"raises" (RuntimeError) or "returns 1": fixed per kind, never read from what a wrapper does"""
    return "raises" if kind in ("dtype", "device") or case_.returns == "value" else "returns 1"


def all_cases():
    return list(CASES)


def all_mutations():
    return [(c, m) for c in CASES for m in mutations(c)]


def case_id(c, m=None):
    return "%s[%s]" % (c.wrapper, c.name) + ("" if m is None else "-%s-%s" % (m.param, m.what))


assert len(set(itertools.starmap(lambda c, m: case_id(c, m), all_mutations()))) == len(all_mutations())
