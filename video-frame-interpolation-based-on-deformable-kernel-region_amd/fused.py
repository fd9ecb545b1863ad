"""Host-side mirrors of the glue either side of the hot-path ops, on the fused entry
points of libvfi_hip.so.  Same names and argument meaning as the reference's static helpers
(`networks/DAIN_slowmotion.py:204-216, 301-335`, `PWCNet/PWCNet.py:159-199`,
`demo_MiddleBury.py:280-318, 350-388`).  `warp`, `warp_corr` and `corr_pair` are differentiable (PWC-Net's glue, trained
with the flow network: the backward is vfi_pwc_warp_backward, for `warp_corr` also the correlation backward, and for
`corr_pair` one vfi_correlation_backward_pair call for both networks).  `corr_lrelu`, `warp_corr_lrelu` and
`corr_pair_lrelu` are their twins with PWC-Net's LeakyReLU inside the correlation's launch, forward and backward
(vfi_correlation_lrelu_*): in inference they can write into a channel slice of the concatenation buffer, in training the
backward masks the gradient as it loads it and reads torch.cat's strided gradient where it lies.
`FlowProject` / `FlowProject_directions` and `FilterInterpolate` are differentiable too, so DAIN's synthesis loss reaches
the flow and filter networks (networks/DAIN.py:215-238): the projection's backward is the reference's per-item kernel,
the blend's is vfi_filterinterp_blend_backward (both directions, the blend weights folded in, no image gradient unless
a frame requires grad).  Each takes its autograd Function only when grad mode is on and an input requires grad; otherwise
it is the plain forward launch, with no grad_fn.  `forward_flownets_upsample` and `FlowProject_from_quarter` are
differentiable in the same way, so the loss reaches the quarter-resolution flow of the flow network: one backward call of
the library for all time offsets (vfi_flow_upsample4_backward, vfi_[depth]flowprojection_backward_up4).
`rectify_inputs` is the end of the synthesis stage in one call: `FilterInterpolate`, `FilterInterpolate_ctx_all` and the `torch.cat`
that builds rectifyNet's input, with the warps written straight into that input (vfi_filterinterp_forward_ori_multi_to) and one
autograd Function over all time offsets.
With dtype=torch.bfloat16 that input is a bfloat16 tensor for a network under bfloat16 autocast: one vfi_rectify_head_forward_bf16
launch per time offset writes its first 45 channels and the float32 `cur_output`, the bfloat16 context warp the rest.
`FilterInterpolate_ctx_all` and `FilterInterpolate_ctx` train the context network: the context tensors get the image
gradient of every time offset from one call per direction (vfi_filterinterp_backward_ori_image_multi), and flows and
filter get none, because the reference detaches them on this path.  The rest (the frame glue) is inference only."""
import math

import torch
from torch.autograd.function import once_differentiable

from . import cabi, cabi_nhwc


def _check(err, what):
    if err != 0:
        raise RuntimeError("%s: the binding returned %d (shape / stride mismatch)" % (what, err))


class DirectionStreams:
    """One HIP stream per flow direction.  In `DAIN_slowmotion.forward` (networks/DAIN_slowmotion.py:147-183) direction d's
    chain -- its flow network with the correlations, `FlowProject` of its flow for every time offset, `FilterInterpolate_ctx` /
    `FilterInterpolate` on context / frame d -- needs nothing of the other direction's until the blend.  Run on two streams
    the chains overlap: the short launches of one hide under the 196-channel warps of the other (1080p pair: 6.5 instead of
    7.0 ms, same bits).  The library keeps its projection workspace per (device, stream); give each direction its own
    `count` plane and output tensors.

        ds = DirectionStreams(device)
        ds.fork()                       # the side stream starts after what the current stream holds NOW (the inputs)
        for d in (0, 1):
            with ds.direction(d):       # d = 0: the current stream; d = 1: the side stream
                ...                     # direction d's calls
        ds.join()                       # the current stream continues when both are done

    Memory across the two streams (torch's caching allocator keeps one pool per stream): a tensor allocated inside
    `with ds.direction(1)` belongs to the side stream's pool and is consumed on the current stream after `join()`; inputs
    allocated on the current stream are read on the side stream after `fork()`.  That is safe as long as such a tensor stays
    alive until the next `fork()` / `join()` has ordered the streams again -- a tensor freed earlier can be handed out again
    on the OTHER stream while launches that use it are still in flight.  Either pre-allocate what crosses the streams (what
    `bench.py` does), or call `tensor.record_stream(stream)` on it; `join(*tensors)` does the latter for the tensors it is given.
    """

    def __init__(self, device=None):
        self.device = device
        self.side = torch.cuda.Stream(device)
        self._forked = False

    def fork(self):
        self.side.wait_stream(torch.cuda.current_stream(self.device))
        self._forked = True

    def direction(self, d):
        if not self._forked:
            raise RuntimeError("DirectionStreams.fork() first: the side stream must be ordered after the inputs")
        return torch.cuda.stream(torch.cuda.current_stream(self.device) if d == 0 else self.side)

    def join(self, *tensors):
        """`tensors`: results of direction 1 that the current stream goes on to use (recorded on it for the allocator)"""
        if self._forked:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_stream(self.side)
            for t in tensors:
                t.record_stream(cur)
            self._forked = False


UP4_ITEMS = 8       # items per backward call of the library (PROJ_NMAX)


def _flow_upsample_launch(flow_q, div_flow, time_offsets):
    b, c, hq, wq = flow_q.shape
    outs = []
    for t in time_offsets:
        out = torch.empty((b, c, 4 * hq, 4 * wq), device=flow_q.device, dtype=torch.float32)
        _check(cabi.flow_upsample4(flow_q, out, float(div_flow), float(t)), "flow_upsample4")
        outs.append(out)
    return outs


def _add_in_order(parts):
    total = parts[0]
    for p in parts[1:]:
        total = total + p
    return total


class _FlowUpsample(torch.autograd.Function):
    """`forward_flownets`' upsample for the whole list of time offsets; the backward is ONE vfi_flow_upsample4_backward call
    over the outputs that received a gradient (per eight of them: the partial sums are added in group order)."""

    @staticmethod
    def forward(ctx, flow_q, div_flow, time_offsets):
        ctx.div_flow, ctx.time_offsets = div_flow, time_offsets
        ctx.q_shape = tuple(flow_q.shape)
        ctx.set_materialize_grads(False)                   # (an unused output is an absent item, not a tensor of zeros)
        return tuple(_flow_upsample_launch(flow_q, div_flow, time_offsets))

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        live = [i for i, g in enumerate(grads) if g is not None]
        if not live:
            return None, None, None
        gs = _grad_layout([grads[i] for i in live])
        parts = []
        for k in range(0, len(live), UP4_ITEMS):
            gq = torch.empty(ctx.q_shape, device=gs[0].device, dtype=torch.float32)
            _check(cabi.flow_upsample4_backward(gs[k:k + UP4_ITEMS], ctx.div_flow,
                                                [ctx.time_offsets[i] for i in live[k:k + UP4_ITEMS]], gq), "flow_upsample4_backward")
            parts.append(gq)
        return _add_in_order(parts), None, None


def forward_flownets_upsample(flow_q, div_flow, time_offsets):
    """`forward_flownets` after the flow network: [div_flow * flow * t upsampled x4 for t in time_offsets].
    Differentiable when grad mode is on and flow_q requires grad (div_flow and the time offsets are Python floats, with
    no gradient): flow_q's gradient is the adjoint of the upsample applied to every output's gradient, summed over the
    time offsets in list order inside one kernel -- reproducible bit for bit, where torch's `upsample_bilinear2d_backward`
    adds with atomics.  Otherwise the plain forward launches, with no grad_fn."""
    if _wants_grad(flow_q):
        return list(_FlowUpsample.apply(flow_q, float(div_flow), tuple(float(t) for t in time_offsets)))
    return _flow_upsample_launch(flow_q, div_flow, time_offsets)


def _flow_project_launch(inputs, depth, fillhole):
    counts = [torch.empty((f.size(0), 1, f.size(2), f.size(3)), device=f.device, dtype=torch.float32) for f in inputs]
    outs = [torch.empty_strided(f.shape, f.stride(), device=f.device, dtype=torch.float32) for f in inputs]
    _check(cabi.flowprojection_forward_batch(inputs, counts, outs, int(fillhole), depth), "flowprojection_forward_batch")
    return counts, outs


class _FlowProject(torch.autograd.Function):
    """The list form of FlowProjectionLayer / DepthFlowProjectionLayer: the forward is the one list call, the backward the
    reference's per-item kernel into zero-filled gradients (it ignores fillhole, as the reference's does).  A depth tensor
    shared by several items appears once per item among the inputs, and autograd sums its gradients."""

    @staticmethod
    def forward(ctx, fillhole, n, *tensors):
        flows, depths = list(tensors[:n]), (list(tensors[n:]) or None)
        counts, outs = _flow_project_launch(flows, depths, fillhole)
        ctx.n, ctx.has_depth = n, depths is not None
        ctx.save_for_backward(*flows, *counts, *(depths + outs if depths is not None else []))
        ctx.set_materialize_grads(False)                   # (an unused output gets no backward, as with one module per item)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        n, saved = ctx.n, ctx.saved_tensors
        flows, counts = saved[:n], saved[n:2 * n]
        gflows, gdepths = [None] * n, [None] * n
        for i in range(n):
            if grads[i] is None:
                continue
            f, g = flows[i].contiguous(), grads[i].contiguous()        # (the reference's layers take contiguous tensors)
            gf = torch.zeros_like(f)
            if not ctx.has_depth:
                _check(cabi.flowprojection_backward(f, counts[i], g, gf), "flowprojection_backward")
            else:
                d, out = saved[2 * n + i].contiguous(), saved[3 * n + i].contiguous()
                gd = torch.zeros_like(d)
                _check(cabi.depthflowprojection_backward(f, d, counts[i], out, g, gf, gd), "depthflowprojection_backward")
                gdepths[i] = gd if ctx.needs_input_grad[2 + n + i] else None
            gflows[i] = gf if ctx.needs_input_grad[2 + i] else None
        return (None, None, *gflows, *(gdepths if ctx.has_depth else []))


def FlowProject(inputs, depth=None, fillhole=True):
    """`DAIN.FlowProject` / `DAIN_slowmotion.FlowProject` (networks/DAIN.py:533-539, networks/DAIN_slowmotion.py:301-307):
    inputs = the list of full-resolution flows of `forward_flownets`, depth = the direction's inverse depth (or None);
    returns the list of projected flows.  The reference loops over the list, one module call per flow; here the list is
    ONE call of the library (one launch triple per eight flows), same results bit for bit.  depth may also be a list, one
    tensor per flow -- which is how both directions go through together: `FlowProject_directions`.
    Differentiable when grad mode is on and a flow or depth requires grad: the gradients are those of the reference's
    per-item `FlowProjectionModule` / `DepthFlowProjectionModule` graph, a shared depth getting the sum of its items'.  The
    reference trains with fillhole=0 (`FlowProjectionModule(input.requires_grad)`, networks/DAIN.py:218); fillhole keeps
    its meaning in the forward, and the backward ignores it, as the reference's does."""
    inputs = list(inputs)
    depths = None if depth is None else (list(depth) if isinstance(depth, (list, tuple)) else [depth] * len(inputs))
    if _wants_grad(*inputs, *(depths or [])):
        if depths is not None and len(depths) != len(inputs):
            _check(1, "flowprojection_forward_batch")
        return list(_FlowProject.apply(bool(fillhole), len(inputs), *inputs, *(depths or [])))
    return _flow_project_launch(inputs, depth, fillhole)[1]


def FlowProject_directions(cur_offset_outputs, depth_inv=None, fillhole=True):
    """The two `FlowProject` calls of `forward` back to back (networks/DAIN.py:215-220, networks/DAIN_slowmotion.py:156-159):
    `[FlowProject(cur_offset_outputs[0], depth_inv[0]), FlowProject(cur_offset_outputs[1], depth_inv[1])]` as one call."""
    n0 = len(cur_offset_outputs[0])
    flows = list(cur_offset_outputs[0]) + list(cur_offset_outputs[1])
    depth = None if depth_inv is None else [depth_inv[0]] * n0 + [depth_inv[1]] * len(cur_offset_outputs[1])
    outs = FlowProject(flows, depth, fillhole)
    return [outs[:n0], outs[n0:]]


def _from_quarter_launch(flow_q, div_flow, time_offsets, depth, fillhole):
    b, _, hq, wq = flow_q.shape
    counts, outs = [], []
    for t in time_offsets:
        count = torch.empty((b, 1, 4 * hq, 4 * wq), device=flow_q.device, dtype=torch.float32)
        out = torch.empty((b, 2, 4 * hq, 4 * wq), device=flow_q.device, dtype=torch.float32)
        if depth is None:
            err = cabi.flowprojection_forward_up4(flow_q, count, out, float(div_flow), float(t), int(fillhole))
        else:
            err = cabi.depthflowprojection_forward_up4(flow_q, depth, count, out, float(div_flow), float(t), int(fillhole))
        _check(err, "flowprojection_forward_up4")
        counts.append(count)
        outs.append(out)
    return counts, outs


class _FlowProjectFromQuarter(torch.autograd.Function):
    """`forward_flownets` + `FlowProject` on the quarter-resolution flow: the forward is the *_forward_up4 call per time
    offset, the backward ONE *_backward_up4 call (per eight time offsets) that never materialises the full-resolution
    flow or its gradient.  It ignores fillhole, as `_FlowProject`'s and the reference's do."""

    @staticmethod
    def forward(ctx, div_flow, time_offsets, fillhole, flow_q, depth):
        counts, outs = _from_quarter_launch(flow_q, div_flow, time_offsets, depth, fillhole)
        ctx.div_flow, ctx.time_offsets, ctx.has_depth = div_flow, time_offsets, depth is not None
        ctx.save_for_backward(flow_q, *counts, *([depth] + outs if depth is not None else []))
        ctx.set_materialize_grads(False)                   # (an unused output is an absent item, not a tensor of zeros)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        n, saved = len(ctx.time_offsets), ctx.saved_tensors
        flow_q, counts = saved[0], saved[1:1 + n]
        live = [i for i, g in enumerate(grads) if g is not None]
        if not live:
            return None, None, None, None, None
        gs = _grad_layout([grads[i] for i in live])
        depth = saved[1 + n] if ctx.has_depth else None
        if ctx.has_depth and not cabi._same_strides(gs[0], saved[2 + n]):      # (the depth form addresses gout like out)
            gs = [g.contiguous() for g in gs]
        want_depth = ctx.has_depth and ctx.needs_input_grad[4]
        q_parts, d_parts = [], []
        for k in range(0, len(live), UP4_ITEMS):
            idx = live[k:k + UP4_ITEMS]
            gq = torch.empty_like(flow_q)
            gds = [torch.empty_like(depth) for _ in idx] if want_depth else None
            _check(cabi.flowprojection_backward_up4(
                flow_q, [counts[i] for i in idx], gs[k:k + UP4_ITEMS], ctx.div_flow, [ctx.time_offsets[i] for i in idx], gq,
                depth, [saved[2 + n + i] for i in idx] if ctx.has_depth else None, gds), "flowprojection_backward_up4")
            q_parts.append(gq)
            d_parts += gds or []
        return (None, None, None, _add_in_order(q_parts) if ctx.needs_input_grad[3] else None,
                _add_in_order(d_parts) if want_depth else None)


def FlowProject_from_quarter(flow_q, div_flow, time_offsets, depth=None, fillhole=True):
    """`forward_flownets` + `FlowProject` in one call per time offset: the full-resolution flow lives in a scratch tensor of
    the library, not in a tensor of the caller.  depth: the direction's inverse depth, shared by the time offsets, or None.
    Differentiable when grad mode is on and flow_q or depth requires grad: flow_q's gradient is that of
    `FlowProject(forward_flownets_upsample(flow_q, ...), depth)` bit for bit, from one fused call of the library for the
    whole list (vfi_[depth]flowprojection_backward_up4: neither the full-resolution flow nor its gradient is stored), and
    depth gets the sum of the time offsets' depth gradients, added in list order.  Reproducible bit for bit.  The
    reference trains with fillhole=0 (networks/DAIN.py:218); fillhole keeps its meaning in the forward, and the backward
    ignores it, as the reference's does.  Otherwise (inference) the plain forward launches, with no grad_fn."""
    if _wants_grad(flow_q, *([] if depth is None else [depth])):
        return list(_FlowProjectFromQuarter.apply(float(div_flow), tuple(float(t) for t in time_offsets), bool(fillhole),
                                                  flow_q, depth))
    return _from_quarter_launch(flow_q, div_flow, time_offsets, depth, fillhole)[1]


def _filter_interpolate_launch(ref0, ref2, off0, off2, filt0, filt2, w0, w2):
    blend, out0, out2 = torch.empty_like(ref0), torch.empty_like(ref0), torch.empty_like(ref0)
    _check(cabi.filterinterp_blend_forward(ref0, ref2, off0, off2, filt0, filt2, blend, out0, out2, w0, w2),
           "filterinterp_blend_forward")
    return blend, out0, out2


def _grad_layout(grads):
    """The incoming gradients share one dense layout for the kernel (an expanded gradient of a sum(), or one laid out
    unlike the others, is made contiguous)."""
    live = [g for g in grads if g is not None]
    if not live:
        return grads
    ref = live[0]
    if ref.stride(3) != 1 or 0 in ref.stride() or not all(cabi._same_strides(ref, g) for g in live):
        return [g.contiguous() if g is not None else None for g in grads]
    return grads


class _FilterInterpolate(torch.autograd.Function):
    """`DAIN.FilterInterpolate` with the gradients of FilterInterpolationModule on both frames plus torch's blend: one
    forward launch, one backward call (vfi_filterinterp_blend_backward)."""

    @staticmethod
    def forward(ctx, ref0, ref2, off0, off2, filt0, filt2, w0, w2):
        blend, out0, out2 = _filter_interpolate_launch(ref0, ref2, off0, off2, filt0, filt2, w0, w2)
        ctx.save_for_backward(ref0, ref2, off0, off2, filt0, filt2)
        ctx.w = (w0, w2)
        ctx.set_materialize_grads(False)                   # (an unused output is an absent term, not a tensor of zeros)
        return blend, out0, out2

    @staticmethod
    @once_differentiable
    def backward(ctx, g_blend, g_out0, g_out2):
        if g_blend is None and g_out0 is None and g_out2 is None:
            # (autograd runs a node whose outputs all went unused, e.g. below a part_loss that used only its flow terms:
            # no launch, and None instead of a tensor of zeros, as in _rectify_backward)
            return (None,) * 8
        saved = ctx.saved_tensors
        g_blend, g_out0, g_out2 = _grad_layout([g_blend, g_out0, g_out2])
        outs = [torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device) if need else None
                for t, need in zip(saved, ctx.needs_input_grad[:6])]
        if any(o is not None for o in outs):
            gr0, gr2, gf0, gf2, gk0, gk2 = outs
            _check(cabi.filterinterp_blend_backward(*saved, g_blend, g_out0, g_out2, ctx.w[0], ctx.w[1], gr0, gr2, gf0, gf2,
                                                    gk0, gk2), "filterinterp_blend_backward")
        return (*outs, None, None)


def FilterInterpolate(ref0, ref2, offset, filter, filter_size2, time_offset):
    """`DAIN.FilterInterpolate`: returns (ref0_offset*(1-t) + ref2_offset*t, ref0_offset, ref2_offset).  Differentiable
    when grad mode is on and a frame, flow or filter requires grad (time_offset is a Python float, with no gradient):
    the gradients equal those of two `FilterInterpolationModule` calls plus torch's blend, bit for bit.  Otherwise the
    plain forward launch."""
    assert filter[0].size(1) == filter_size2
    w0, w2 = float(1.0 - time_offset), float(time_offset)
    if _wants_grad(ref0, ref2, *offset, *filter):
        return _FilterInterpolate.apply(ref0, ref2, offset[0], offset[1], filter[0], filter[1], w0, w2)
    return _filter_interpolate_launch(ref0, ref2, offset[0], offset[1], filter[0], filter[1], w0, w2)


def _ctx_warp_launch(ctx, offsets, filt):
    # (outputs share the input's layout, strided views included: empty_like would densify a channel slice)
    outs = [torch.empty_strided(ctx.shape, ctx.stride(), dtype=ctx.dtype, device=ctx.device) for _ in offsets]
    _check(cabi.filterinterp_forward_ori_multi(ctx, list(offsets), filt, outs), "filterinterp_forward_ori_multi")
    return outs


class _FilterInterpolateCtx(torch.autograd.Function):
    """One direction of `FilterInterpolate_ctx` for a list of time offsets: the forward is the one multi-flow launch, the
    backward ONE vfi_filterinterp_backward_ori_image_multi call over the outputs that received a gradient.  The context
    tensor's gradient does not depend on its values, so only the flows and the filter are saved.  Flows and filter get no
    gradient (the reference detaches them).  A bfloat16 image takes the bfloat16 entries: its outputs and its gradient are
    bfloat16, flows and filter arrive here as float32 (`_ctx_warp` widens them) and are saved as such."""

    @staticmethod
    def forward(ctx, image, filt, *offsets):
        outs = _ctx_warp_launch(image, offsets, filt)
        ctx.save_for_backward(filt, *offsets)
        ctx.image_layout = (image.shape, image.stride(), image.dtype)
        ctx.set_materialize_grads(False)                   # (an unused time offset is an absent flow, not a tensor of zeros)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        saved = ctx.saved_tensors                          # (read once: torch.utils.checkpoint refuses a second unpack)
        filt, offsets = saved[0], saved[1:]
        none = (None,) * (2 + len(offsets))
        live = [i for i, g in enumerate(grads) if g is not None]
        if not live or not ctx.needs_input_grad[0]:
            return none
        gs = _grad_layout([grads[i] for i in live])
        shape, stride, dtype = ctx.image_layout
        gimg = torch.empty_strided(shape, stride, dtype=dtype, device=gs[0].device)      # (written in full)
        _check(cabi.filterinterp_backward_ori_image_multi([offsets[i] for i in live], filt, gs, gimg),
               "filterinterp_backward_ori_image_multi")
        return (gimg,) + none[1:]


def _f32_once(t):
    """a bfloat16 flow or filter widened to float32 (exact); a float32 tensor as it is"""
    return t.float() if t.dtype == torch.bfloat16 else t


def _channels_last_only(t):
    """channel stride 1 and a pixel stride that is not: a channels_last tensor (or a channel slice of one) that the NCHW
    entries refuse.  A [B, 1, H, W] tensor is both layouts at once and stays on the NCHW path."""
    return t.dim() == 4 and t.stride(3) != 1 and t.stride(1) == 1


def _refuse_channels_last_grad(*images):
    for image in images:
        if _channels_last_only(image) and _wants_grad(image):
            raise RuntimeError("FilterInterpolate_ctx: the channels_last warp is forward-only by default; a .contiguous() "
                               "context tensor trains, and so does a channels_last one with train_channels_last=True")


def _ctx_warp_nhwc_launch(ctx, offsets, filt):
    # (the outputs get the input's strides, as in _ctx_warp_launch; flows and filter may be NCHW or channels_last)
    outs = [torch.empty_strided(ctx.shape, ctx.stride(), dtype=ctx.dtype, device=ctx.device) for _ in offsets]
    _check(cabi.filterinterp_forward_nhwc_multi_to(ctx, list(offsets), filt, outs), "filterinterp_forward_nhwc_multi_to")
    return outs


def _grad_layout_nhwc(grads):
    """The incoming gradients as the NHWC image gradient reads them: channel stride 1 and one shared layout without zero
    strides (an expanded gradient).  Gradients that are not all like that are each made dense channels_last."""
    ref = grads[0]
    if not cabi._channels_innermost(ref) or 0 in ref.stride() or not all(cabi._same_strides(ref, g) for g in grads):
        return [g.contiguous(memory_format=torch.channels_last) for g in grads]
    return grads


class _FilterInterpolateCtxNhwc(torch.autograd.Function):
    """`_FilterInterpolateCtx` for a channels_last context tensor: the forward is the NHWC launch, the backward ONE
    vfi_filterinterp_backward_ori_nhwc_image_multi[_bf16] call over the outputs that received a gradient, on the gradients
    where they are.  Only the flows and the filter are saved; they get no gradient.  The context gradient is a dense
    channels_last tensor of the context's dtype (not laid out with a slice's strides), written in full."""

    @staticmethod
    def forward(ctx, image, filt, *offsets):
        outs = _ctx_warp_nhwc_launch(image, offsets, filt)
        ctx.save_for_backward(filt, *offsets)
        ctx.image_layout = (image.shape, image.dtype)
        ctx.set_materialize_grads(False)                   # (an unused time offset is an absent flow, not a tensor of zeros)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        saved = ctx.saved_tensors                          # (read once: torch.utils.checkpoint refuses a second unpack)
        filt, offsets = saved[0], saved[1:]
        none = (None,) * (2 + len(offsets))
        live = [i for i, g in enumerate(grads) if g is not None]
        if not live or not ctx.needs_input_grad[0]:
            return none
        gs = _grad_layout_nhwc([grads[i] for i in live])
        shape, dtype = ctx.image_layout
        gimg = torch.empty(shape, dtype=dtype, device=gs[0].device, memory_format=torch.channels_last)      # (written in full)
        _check(cabi_nhwc.filterinterp_backward_nhwc_image_multi([offsets[i] for i in live], filt, gs, gimg),
               "filterinterp_backward_nhwc_image_multi")
        return (gimg,) + none[1:]


def _ctx_warp(image, offsets, filt, train_channels_last=False):
    """one direction: the Function when the context tensor can train, today's plain launch otherwise.  With a bfloat16
    context tensor a bfloat16 flow or filter is widened here, once per direction; float32 calls pass through untouched.
    A channels_last context tensor (stride(3) != 1, stride(1) == 1) is warped in place by the NHWC entry: one that requires
    grad in grad mode raises before any launch, or, with train_channels_last, takes the NHWC Function."""
    nhwc = _channels_last_only(image)
    if not train_channels_last:
        _refuse_channels_last_grad(image)
    if image.dtype == torch.bfloat16:
        offsets, filt = [_f32_once(o) for o in offsets], _f32_once(filt)
    if nhwc:
        if train_channels_last and _wants_grad(image):
            return list(_FilterInterpolateCtxNhwc.apply(image, filt, *offsets))
        return _ctx_warp_nhwc_launch(image, offsets, filt)
    if _wants_grad(image):
        return list(_FilterInterpolateCtx.apply(image, filt, *offsets))
    return _ctx_warp_launch(image, offsets, filt)


def FilterInterpolate_ctx_all(ctx0, ctx2, offsets, filter, train_channels_last=False):
    """`DAIN_slowmotion.FilterInterpolate_ctx` (networks/DAIN_slowmotion.py:311-317) for every time offset of a step at
    once (the loop at :167-183 calls it once per t with the same context tensors and filters): offsets[d][t] is the
    projected flow of direction d at time offset t.  Returns [(ctx0_offset_t, ctx2_offset_t) for t], each pair what
    the reference's call returns -- from one launch per direction that stages every image window once.
    Differentiable towards the context tensors when grad mode is on and ctx0 or ctx2 requires grad: a direction's context
    tensor gets the sum over the time offsets of FilterInterpolationModule's image gradient, from ONE call of the library
    over the outputs the loss used (reproducible bit for bit).  Offsets and filter get NO gradient, whether or not they
    require grad: the reference passes `offset[d].detach()` and `filter[d].detach()` on this path.  Otherwise (inference,
    or no context tensor requiring grad) the plain forward launches, with no grad_fn.
    bfloat16 context tensors (a context network under `torch.autocast(dtype=torch.bfloat16)`) are warped as they are: the
    outputs are bfloat16 -- bit for bit `.float()`, the float32 call, `.bfloat16()` -- and so is the context gradient,
    bf16_rne of the float32 backward on the widened incoming gradients.  Flow and filter stay float32 in the kernels: a
    bfloat16 flow or filter is widened once per direction with `.float()`, which is exact.  A float32 context tensor takes
    the launches it always took.
    channels_last context tensors (float32 or bfloat16; `stride(3) != 1` and `stride(1) == 1`, a channel slice of a wider
    channels_last tensor included) are warped where they are by vfi_filterinterp_forward_ori_nhwc_multi_to[_bf16]: the outputs
    have the input's strides and hold, bit for bit, the NCHW call's `.contiguous(memory_format=torch.channels_last)`; flows
    and filter may be in either layout.  "The input's strides" includes a slice's: the outputs of `wide[:, 45:241]` of a
    437-channel tensor each span the wide tensor's footprint (437 / 196 of the dense size) -- pass a dense context, or call
    `cabi.filterinterp_forward_nhwc_multi_to` with destinations of your own, where that matters.  By default the path is
    forward-only: if either context is such a tensor and requires grad in grad mode, the call raises a RuntimeError before any
    launch of either direction (`.contiguous()` trains).  Every tensor with `stride(3) == 1` goes where it always went.
    train_channels_last=True: such a context trains where it is.  In grad mode a channels_last context that requires grad
    takes the NHWC forward launch and, in the backward, ONE vfi_filterinterp_backward_ori_nhwc_image_multi[_bf16] call over
    the outputs the loss used: its gradient is, bit for bit, what the NCHW Function returns for the `.contiguous()` context,
    as a dense channels_last tensor of the context's dtype (also for a channel-slice context).  Incoming gradients are read
    where they are when they all have channel stride 1 and one layout without zero strides; otherwise each is made
    `.contiguous(memory_format=torch.channels_last)` first.  Everything else goes where it goes without the keyword: NCHW
    contexts, channels_last contexts that need no gradient, `[B, 1, H, W]` contexts, `no_grad` calls; the two directions may
    differ in layout."""
    if not train_channels_last:
        _refuse_channels_last_grad(ctx0, ctx2)              # (both directions, before the first launch)
    out0 = _ctx_warp(ctx0, list(offsets[0]), filter[0], train_channels_last)
    out2 = _ctx_warp(ctx2, list(offsets[1]), filter[1], train_channels_last)
    return list(zip(out0, out2))


def FilterInterpolate_ctx(ctx0, ctx2, offset, filter, train_channels_last=False):
    """`DAIN.FilterInterpolate_ctx` (networks/DAIN.py:544-552): (ctx0_offset, ctx2_offset) for one time offset,
    offset = [flow of direction 0, flow of direction 1].  Differentiable exactly as `FilterInterpolate_ctx_all` is:
    towards the context tensors only; `train_channels_last` as there."""
    return FilterInterpolate_ctx_all(ctx0, ctx2, [[offset[0]], [offset[1]]], filter, train_channels_last)[0]


# ---------------------------------------------------------------- the rectify network's input, written in place

def rectify_channels(filter_size2, ctx_channels=None):
    """Channel ranges of the tensor the reference concatenates for rectifyNet (networks/DAIN_slowmotion.py:177-181,
    networks/DAIN.py:264-268), in its order: name -> (first, one past last), plus 'total'.  `cur_output`, `ref0`, `ref2` are
    the blend and the two warped frames, `offset0/1` the projected flows, `filter0/1` the filters, `ctx0/2` the warped
    context tensors (absent for ctx_channels None: DAIN's 45-channel input at filter_size2 == 16, 437 with 196)."""
    m, at = {}, 0
    for name, n in (("cur_output", 3), ("ref0", 3), ("ref2", 3), ("offset0", 2), ("offset1", 2), ("filter0", filter_size2),
                    ("filter1", filter_size2)) + ((("ctx0", ctx_channels), ("ctx2", ctx_channels)) if ctx_channels else ()):
        m[name] = (at, at + n)
        at += n
    m["total"] = at
    return m


def _ch(t, rng):
    return t[:, rng[0]:rng[1]]


def _rectify_buffers(ref0, filt0, ctx0, ctx2, time_offsets, off0, off2, dtype):
    """the argument checks of both launches, then the T buffers (uninitialised) and the channel map"""
    if (ctx0 is None) != (ctx2 is None):
        raise RuntimeError("rectify_inputs: ctx0 and ctx2 are given together or not at all")
    b, c, h, w = ref0.shape
    if c != 3 or len(off0) != len(time_offsets) or len(off2) != len(time_offsets):
        raise RuntimeError("rectify_inputs: 3-channel frames and one flow per direction and time offset")
    m = rectify_channels(filt0.size(1), None if ctx0 is None else ctx0.size(1))
    return [torch.empty((b, m["total"], h, w), device=ref0.device, dtype=dtype) for _ in time_offsets], m


def _rectify_launch(ref0, ref2, filt0, filt2, ctx0, ctx2, time_offsets, off0, off2):
    """the T buffers, every channel written: the frames' kernel into 0-8, one multi-flow call per direction into the context
    slices of all T buffers, copy_ for the flows and filters"""
    bufs, m = _rectify_buffers(ref0, filt0, ctx0, ctx2, time_offsets, off0, off2, torch.float32)
    for buf, t, f0, f2 in zip(bufs, time_offsets, off0, off2):
        _check(cabi.filterinterp_blend_forward(ref0, ref2, f0, f2, filt0, filt2, _ch(buf, m["cur_output"]), _ch(buf, m["ref0"]),
                                               _ch(buf, m["ref2"]), float(1.0 - t), float(t)), "filterinterp_blend_forward")
        for name, src in (("offset0", f0), ("offset1", f2), ("filter0", filt0), ("filter1", filt2)):
            _ch(buf, m[name]).copy_(src)
    _rectify_ctx_launch(bufs, m, filt0, filt2, ctx0, ctx2, off0, off2)
    return bufs, m


def _rectify_ctx_launch(bufs, m, filt0, filt2, ctx0, ctx2, off0, off2):
    """one multi-flow call per direction into the context slices of all T buffers, in the buffers' dtype"""
    for name, image, flows, filt in (("ctx0", ctx0, off0, filt0), ("ctx2", ctx2, off2, filt2)):
        if image is not None:
            _check(cabi.filterinterp_forward_ori_multi_to(image, list(flows), filt, [_ch(buf, m[name]) for buf in bufs]),
                   "filterinterp_forward_ori_multi_to")


def _rectify_launch_bf16(ref0, ref2, filt0, filt2, ctx0, ctx2, time_offsets, off0, off2):
    """the T bfloat16 buffers and the T dense float32 blends, every element written by a kernel: ONE head launch per time
    offset (vfi_rectify_head_forward_bf16: channels 0-44 and the float32 blend), one multi-flow call per direction into the
    context slices of all T buffers.  No copy_, no cast."""
    bufs, m = _rectify_buffers(ref0, filt0, ctx0, ctx2, time_offsets, off0, off2, torch.bfloat16)
    curs = [torch.empty(ref0.shape, device=ref0.device, dtype=torch.float32) for _ in time_offsets]
    head = (0, m["filter1"][1])
    for buf, cur, t, f0, f2 in zip(bufs, curs, time_offsets, off0, off2):
        _check(cabi.rectify_head_forward_bf16(ref0, ref2, f0, f2, filt0, filt2, _ch(buf, head), cur, float(1.0 - t), float(t)),
               "rectify_head_forward_bf16")
    _rectify_ctx_launch(bufs, m, filt0, filt2, ctx0, ctx2, off0, off2)
    return bufs, curs, m


def _rectify_forward(ctx, bf16, ref0, ref2, filt0, filt2, ctx0, ctx2, time_offsets, *offsets):
    n = len(time_offsets)
    off0, off2 = offsets[:n], offsets[n:]
    if bf16:
        bufs, curs, m = _rectify_launch_bf16(ref0, ref2, filt0, filt2, ctx0, ctx2, time_offsets, off0, off2)
    else:
        bufs, m = _rectify_launch(ref0, ref2, filt0, filt2, ctx0, ctx2, time_offsets, off0, off2)
        curs = [_ch(buf, m["cur_output"]).clone() for buf in bufs]
    ctx.save_for_backward(ref0, ref2, filt0, filt2, *offsets)
    ctx.time_offsets, ctx.map = tuple(time_offsets), m
    ctx.ctx_layouts = [None if t is None else (t.shape, t.stride(), t.dtype) for t in (ctx0, ctx2)]
    ctx.set_materialize_grads(False)                   # (an unused output is an absent term, not a tensor of zeros)
    return (*bufs, *curs)


def _rectify_backward(ctx, bf16, *grads):
    """bf16: the buffers' gradients are bfloat16 (the cur_output gradients float32).  The nine frame channels and the slices
    that passed through are widened (exactly) where they are used; the context channels are read in place, as bfloat16."""
    saved = ctx.saved_tensors                              # (read once: torch.utils.checkpoint refuses a second unpack)
    ref0, ref2, filt0, filt2 = saved[:4]
    offsets = saved[4:]
    n, m = len(ctx.time_offsets), ctx.map
    off = (offsets[:n], offsets[n:])
    g_buf, g_cur = grads[:n], grads[n:]
    need = ctx.needs_input_grad
    like = lambda t: torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device)      # noqa: E731
    f32 = (lambda g, name: _ch(g, m[name]).float()) if bf16 else (lambda g, name: _ch(g, m[name]))
    # ---- frames, flows, filters: one blend backward per time offset that received a gradient; its flow and filter terms,
    # then the slice of the buffer's gradient that passed through.  Sums run over t ascending, the kernel's term first.
    terms = {"ref0": [], "ref2": [], "filt0": [], "filt2": []}
    g_off = [[None] * n, [None] * n]
    for t in range(n):
        gb, gc = g_buf[t], g_cur[t]
        if gb is None and gc is None:
            continue
        g_blend = gc if gb is None else (f32(gb, "cur_output") if gc is None else f32(gb, "cur_output") + gc)
        g_blend, g_out0, g_out2 = _grad_layout([g_blend, None if gb is None else f32(gb, "ref0"),
                                                None if gb is None else f32(gb, "ref2")])
        outs = [like(x) if nd else None for x, nd in
                ((ref0, need[0]), (ref2, need[1]), (off[0][t], need[7 + t]), (off[1][t], need[7 + n + t]), (filt0, need[2]),
                 (filt2, need[3]))]
        if any(o is not None for o in outs):
            w0, w2 = float(1.0 - ctx.time_offsets[t]), float(ctx.time_offsets[t])
            _check(cabi.filterinterp_blend_backward(ref0, ref2, off[0][t], off[1][t], filt0, filt2, g_blend, g_out0, g_out2,
                                                    w0, w2, *outs), "filterinterp_blend_backward")
        gr0, gr2, gf0, gf2, gk0, gk2 = outs
        for d, gf in ((0, gf0), (1, gf2)):
            if gf is not None:
                g_off[d][t] = gf if gb is None else gf + f32(gb, "offset%d" % d)
        for key, kernel, through in (("ref0", gr0, None), ("ref2", gr2, None), ("filt0", gk0, "filter0"), ("filt2", gk2, "filter1")):
            if kernel is not None:
                terms[key].append(kernel)
                if through is not None and gb is not None:
                    terms[key].append(f32(gb, through))
    total = {k: (_add_in_order(v) if v else None) for k, v in terms.items()}
    # ---- context tensors: one image-only call per direction over the buffers that received a gradient, which reads the
    # context channels of those gradients where they lie
    g_ctx = [None, None]
    live = [t for t in range(n) if g_buf[t] is not None]
    for d, name in ((0, "ctx0"), (1, "ctx2")):
        if ctx.ctx_layouts[d] is None or not need[4 + d] or not live:
            continue
        gs = _grad_layout([_ch(g_buf[t], m[name]) for t in live])
        shape, stride, dtype = ctx.ctx_layouts[d]
        g_ctx[d] = torch.empty_strided(shape, stride, dtype=dtype, device=gs[0].device)      # (written in full)
        _check(cabi.filterinterp_backward_ori_image_multi([off[d][t] for t in live], (filt0, filt2)[d], gs, g_ctx[d]),
               "filterinterp_backward_ori_image_multi")
    return (total["ref0"], total["ref2"], total["filt0"], total["filt2"], g_ctx[0], g_ctx[1], None, *g_off[0], *g_off[1])


class _RectifyInputs(torch.autograd.Function):
    """`rectify_inputs` over all time offsets: outputs are the T buffers, then T dense copies of their `cur_output` channels
    (the loss uses those directly; as slices of the buffers they would each cost autograd a full-size zero gradient).
    Saved: frames, flows and filters -- not the buffers, and not the context tensors (their gradient does not depend on
    their values)."""

    @staticmethod
    def forward(ctx, *args):
        return _rectify_forward(ctx, False, *args)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        return _rectify_backward(ctx, False, *grads)


class _RectifyInputsBf16(torch.autograd.Function):
    """`_RectifyInputs` with bfloat16 buffers (and bfloat16 context tensors): the same arguments, outputs, saved tensors and
    gradient bookkeeping; the T `cur_output` tensors stay float32, written by the head kernel beside the rounded channels.
    The buffers' gradients arrive as bfloat16, the context gradients leave as bfloat16, everything else is float32."""

    @staticmethod
    def forward(ctx, *args):
        return _rectify_forward(ctx, True, *args)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        return _rectify_backward(ctx, True, *grads)


def _rectify_dtypes(bf16, frames, floats, contexts):
    """the dtype rules of `rectify_inputs`, checked before any launch: float32 frames; float32 flows and filters, for a
    bfloat16 buffer bfloat16 ones too; context tensors of the buffer's dtype"""
    def must_be(t, *dtypes):
        if t.dtype not in dtypes:
            raise RuntimeError("rectify_inputs: tensors must be %s" % " or ".join(str(d).replace("torch.", "") for d in dtypes))
    for t in frames:
        must_be(t, torch.float32)
    for t in floats:
        must_be(t, *((torch.float32, torch.bfloat16) if bf16 else (torch.float32,)))
    for t in contexts:
        must_be(t, torch.bfloat16 if bf16 else torch.float32)


def rectify_inputs(ref0, ref2, offsets, filter, filter_size2, time_offsets, ctx0=None, ctx2=None, dtype=None):
    """The end of the synthesis stage for every time offset of a step (networks/DAIN_slowmotion.py:167-182; without context
    tensors networks/DAIN.py:255-269): `FilterInterpolate`, `FilterInterpolate_ctx` and the `torch.cat` that builds
    rectifyNet's input, with the warps written straight into that input.  offsets[d][t] is the projected flow of direction
    d at time offset t (as for `FilterInterpolate_ctx_all`), filter = [filter of direction 0, of direction 1].
    Returns [(rectify_input_t, cur_output_t) for t in time_offsets]: rectify_input_t is one freshly allocated contiguous
    [B, 13 + 2 filter_size2 (+ 2 Cctx), H, W] tensor in the reference's channel order (`rectify_channels`).  The blend and
    the two warped frames are written into channels 0-8 by vfi_filterinterp_blend_forward, each direction's context warps for
    all time offsets by one vfi_filterinterp_forward_ori_multi_to call; only the flows and filters (36 channels of 437) are
    copied.
    Bit-equal, forward: every channel equals `torch.cat` over `FilterInterpolate` and `FilterInterpolate_ctx_all`.
    Inference (grad mode off, or no input requires grad): cur_output_t is the view rectify_input_t[:, :3].
    Training: one autograd Function over all time offsets; cur_output_t is then a dense copy and an output of its own.
    Frames, flows and filters get the gradient of the blend backward (one vfi_filterinterp_blend_backward per time offset,
    fed grad_blend = grad(rectify_input_t)[:, 0:3] + grad(cur_output_t)) plus, for flows and filters, the channels of
    grad(rectify_input_t) that passed through; a context tensor gets one vfi_filterinterp_backward_ori_image_multi call over
    the context channels of the gradients, read in place.  As on the reference's path the context warps give flows and
    filters no gradient.  An output the loss did not use is an absent term.
    Bit-equal, backward: a flow's gradient is kernel term + passed-through slice; a filter's or frame's is the left-to-right
    sum over t ascending of (kernel term of t, passed-through slice of t).  For one time offset each sum has at most two
    terms, so every gradient equals autograd's through `torch.cat` over the functions above, bit for bit.
    dtype: None -- everything float32, as described above -- or torch.bfloat16, for a rectifyNet under
    `torch.autocast(dtype=torch.bfloat16)`: rectify_input_t is then a BFLOAT16 tensor, written in place and once.  Frames
    are float32; flows and filters float32 or bfloat16 (widened once, exactly, outside the autograd Function: autograd rounds
    their gradient back); context tensors bfloat16, or absent.  Every other dtype is refused before any launch.  Per time
    offset ONE vfi_rectify_head_forward_bf16 launch writes channels 0-44 and cur_output_t; one
    vfi_filterinterp_forward_ori_multi_to_bf16 call per direction writes the context channels of all buffers; there is no
    copy_, no cast and no torch.cat.  cur_output_t is float32 and a tensor of its own, in inference too: the reference adds
    it to rectifyNet's output and puts it into the loss, where a view of the rounded channels would have lost 16 bits.
    Bit-equal: rectify_input_t is the float32 call's (the contexts entering through `.float()`) `.to(torch.bfloat16)`,
    cur_output_t the float32 call's; every gradient is what autograd gives through that graph -- float32 for frames, flows
    and filters (the buffers' bfloat16 gradients widened where they are used), bfloat16 for the context tensors, from one
    vfi_filterinterp_backward_ori_image_multi_bf16 call per direction that reads the gradients' context channels in place."""
    assert filter[0].size(1) == filter_size2
    if dtype is not None and dtype != torch.bfloat16:
        raise RuntimeError("rectify_inputs: dtype is None (float32) or torch.bfloat16")
    bf16 = dtype is not None
    time_offsets = [float(t) for t in time_offsets]
    off0, off2, filt = list(offsets[0]), list(offsets[1]), list(filter[:2])
    _rectify_dtypes(bf16, (ref0, ref2), (*filt, *off0, *off2), [t for t in (ctx0, ctx2) if t is not None])
    if bf16:
        off0, off2, filt = [_f32_once(o) for o in off0], [_f32_once(o) for o in off2], [_f32_once(f) for f in filt]
    n = len(time_offsets)
    tensors = [ref0, ref2, *filt, *off0, *off2] + [t for t in (ctx0, ctx2) if t is not None]
    if _wants_grad(*tensors):
        fn = _RectifyInputsBf16 if bf16 else _RectifyInputs
        outs = fn.apply(ref0, ref2, filt[0], filt[1], ctx0, ctx2, tuple(time_offsets), *off0, *off2)
        return list(zip(outs[:n], outs[n:]))
    if bf16:
        bufs, curs, m = _rectify_launch_bf16(ref0, ref2, filt[0], filt[1], ctx0, ctx2, time_offsets, off0, off2)
        return list(zip(bufs, curs))
    bufs, m = _rectify_launch(ref0, ref2, filt[0], filt[1], ctx0, ctx2, time_offsets, off0, off2)
    return [(buf, _ch(buf, m["cur_output"])) for buf in bufs]


class _Warp(torch.autograd.Function):
    """`PWCDCNet.warp` with the gradients torch autograd gives for the reference's formula (vfi_pwc_warp_backward; for a
    bfloat16 x vfi_pwc_warp_backward_bf16, whose grad_x is bfloat16 and whose grad_flow has the flow's dtype)."""

    @staticmethod
    def forward(ctx, x, flo, align_corners):
        out = torch.empty_like(x)
        _check(cabi.pwc_warp_forward(x, flo, out, align_corners), "pwc_warp_forward")
        ctx.save_for_backward(x, flo)
        ctx.align_corners = align_corners
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, flo = ctx.saved_tensors
        if grad_out.stride(3) != 1:                         # (e.g. the expanded gradient of a sum())
            grad_out = grad_out.contiguous()
        if not ctx.needs_input_grad[0]:
            gx = None
        else:                                               # (float32: added into; bfloat16: written in full)
            gx = torch.empty_like(x) if x.dtype == torch.bfloat16 else torch.zeros_like(x)
        gf = torch.empty_like(flo) if ctx.needs_input_grad[1] else None        # (written)
        if gx is not None or gf is not None:
            _check(cabi.pwc_warp_backward(x, flo, grad_out, gx, gf, ctx.align_corners), "pwc_warp_backward")
        return gx, gf, None


class _Corr(torch.autograd.Function):
    """PWC-Net's correlation (pad 4, k 1, md 4, strides 1) on the C ABI, forward and backward.  float32, float16 or
    bfloat16 (all tensors of one dtype: `cabi.correlation_forward` / `correlation_backward` dispatch on it)."""

    @staticmethod
    def forward(ctx, c1, c2):
        ctx.save_for_backward(c1, c2)
        return cabi.correlation_forward(c1, c2, 4, 1, 4, 1, 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        c1, c2 = ctx.saved_tensors
        g1, g2 = cabi.correlation_backward(c1, c2, grad_out, 4, 1, 4, 1, 1)
        return (g1 if ctx.needs_input_grad[0] else None), (g2 if ctx.needs_input_grad[1] else None)


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def _float32_only(what, hint, *tensors):
    for t in tensors:
        if t.dtype != torch.float32:
            raise RuntimeError("%s: tensors must be float32 (%s)" % (what, hint))


def _warp(x, flo, align_corners):
    """`warp` for the dtypes the library warps: float32, or a bfloat16 x -- the dtype of a network under
    torch.autocast(dtype=torch.bfloat16) -- with a float32 or a bfloat16 flow.  On bfloat16 the result is bit for bit
    `warp(x.float(), flo.float()).to(x.dtype)` from one launch and without a cast; the gradients are that composition's too,
    each rounded once (grad_x bfloat16, grad_flow in the flow's dtype).  float16 raises."""
    if _wants_grad(x, flo):
        return _Warp.apply(x, flo, bool(align_corners))
    out = torch.empty_like(x)
    _check(cabi.pwc_warp_forward(x, flo, out, align_corners), "pwc_warp_forward")
    return out


def warp(x, flo, align_corners=True):
    """`PWCDCNet.warp`.  Differentiable when grad mode is on and x or flo requires grad; otherwise the plain forward
    launch (no grad_fn).  float32 only (anything else raises), as it has always been: a bfloat16 network warps inside
    `warp_corr` / `warp_corr_lrelu`, which take bfloat16 features and run the warp on bfloat16 storage without a cast; the
    warp alone on bfloat16 is `_Warp.apply(x, flo, align_corners)` (trainable) or `cabi.pwc_warp_forward`."""
    _float32_only("warp", "warp_corr, warp_corr_lrelu and _Warp.apply take bfloat16", x, flo)
    return _warp(x, flo, align_corners)


def warp_corr(c1, c2, flo, align_corners=True, one_launch=False):
    """`self.corr(c1, self.warp(c2, flo))` of PWCDCNet.forward (PWCNet/PWCNet.py:244-247 ...); the reference applies
    its LeakyReLU to the result afterwards.  Default: the warp kernel, then the correlation kernel.  one_launch=True:
    vfi_pwc_warp_correlation_forward, which never materialises the warped tensor -- same bits, but measured SLOWER on
    MI355X at PWC-Net's sizes (0.33 vs 0.15 ms for the five levels of a 1080p pair): every tile re-forms the bilinear
    samples of its 4-pixel halo (3.75 x the taps), which costs more than the 2 x 18 MB round trip it saves.
    Differentiable when grad mode is on and an input requires grad: then the two-launch path (one_launch is ignored;
    same bits), whose warped tensor the correlation backward needs.  float32, or bfloat16 features (with a float32 or a
    bfloat16 flow): two launches on bfloat16 storage, no cast; one_launch is ignored there too (the one-launch kernel is
    float32 only).  float16 raises."""
    if _wants_grad(c1, c2, flo):
        return _Corr.apply(c1, _warp(c2, flo, align_corners))
    if one_launch and c1.dtype != torch.bfloat16:
        return cabi.pwc_warp_correlation_forward(c1, c2, flo, align_corners)
    return cabi.correlation_forward(c1, _warp(c2, flo, align_corners), 4, 1, 4, 1, 1)


class _CorrPair(torch.autograd.Function):
    """`corr_pair` with its backward: the forward is the one vfi_correlation_forward_pair launch, the backward ONE
    vfi_correlation_backward_pair call for the gradients autograd needs -- each bit-equal to `_Corr`'s.  A cost volume
    the loss did not use arrives as None (not as zeros), and its item's gradients are None at no cost.  float32 or
    bfloat16 (all tensors of one dtype: `cabi.correlation_forward_pair` / `correlation_backward_pair` dispatch on it)."""

    @staticmethod
    def forward(ctx, c1_a, c2_a, c1_b, c2_b):
        ctx.save_for_backward(c1_a, c2_a, c1_b, c2_b)
        ctx.set_materialize_grads(False)
        return cabi.correlation_forward_pair(c1_a, c2_a, c1_b, c2_b, 4, 1, 4, 1, 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_a, grad_b):
        c1_a, c2_a, c1_b, c2_b = ctx.saved_tensors
        return cabi.correlation_backward_pair(c1_a, c2_a, grad_a, c1_b, c2_b, grad_b, 4, 1, 4, 1, 1,
                                              want=tuple(ctx.needs_input_grad))


def corr_pair(c1_a, c2_a, c1_b, c2_b):
    """`self.corr(c1, c2)` of the two flow networks of a frame pair at one pyramid level (PWCNet/PWCNet.py:230, 246, 267, 283,
    300 for the (I0, I1) network and again for (I1, I0): networks/DAIN.py:196-202) in one launch; returns both cost volumes.
    Differentiable when grad mode is on and one of the four inputs requires grad: the backward is then ONE call for the
    gradients that are needed (each bit-equal to the single correlation's; reproducible).  Otherwise the plain forward
    launch (no grad_fn).  float32 only, as it has always been: bfloat16 and float16 tensors raise.  On bfloat16 the pair is
    `corr_pair_lrelu` (what a PWC-Net level needs) or, without the activation, `_CorrPair.apply(c1_a, c2_a, c1_b, c2_b)`
    (trainable) / `cabi.correlation_forward_pair`: one launch each way, every tensor bit-equal to the single bfloat16
    correlation's."""
    _float32_only("corr_pair", "corr_pair_lrelu and _CorrPair.apply take bfloat16", c1_a, c2_a, c1_b, c2_b)
    if _wants_grad(c1_a, c2_a, c1_b, c2_b):
        return _CorrPair.apply(c1_a, c2_a, c1_b, c2_b)
    return cabi.correlation_forward_pair(c1_a, c2_a, c1_b, c2_b, 4, 1, 4, 1, 1)


class _CorrLrelu(torch.autograd.Function):
    """`_Corr` with PWC-Net's LeakyReLU in the correlation's own launch (float32 or bfloat16: `cabi.correlation_lrelu_forward` /
    `_backward` dispatch on the dtype).  The saved tensor is the activated output y; the
    backward is one vfi_correlation_lrelu_backward call that masks the gradient as it loads it and reads a strided
    gradient (the narrow() view of torch.cat's backward) where it lies."""

    @staticmethod
    def forward(ctx, c1, c2, slope):
        y = cabi.correlation_lrelu_forward(c1, c2, 4, 1, 4, 1, 1, slope)
        ctx.save_for_backward(c1, c2, y)
        ctx.slope = slope
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        c1, c2, y = ctx.saved_tensors
        g1, g2 = cabi.correlation_lrelu_backward(c1, c2, y, grad_out, 4, 1, 4, 1, 1, ctx.slope)
        return (g1 if ctx.needs_input_grad[0] else None), (g2 if ctx.needs_input_grad[1] else None), None


class _CorrPairLrelu(torch.autograd.Function):
    """`_CorrPair` with the LeakyReLU fused into both directions: one forward launch, ONE
    vfi_correlation_lrelu_backward_pair call for the gradients autograd needs.  A cost volume the loss did not use arrives
    as None, and its item's gradients are None at no cost.  float32 or bfloat16, as `_CorrLrelu`."""

    @staticmethod
    def forward(ctx, c1_a, c2_a, c1_b, c2_b, slope):
        y_a, y_b = cabi.correlation_lrelu_forward_pair(c1_a, c2_a, c1_b, c2_b, 4, 1, 4, 1, 1, slope)
        ctx.save_for_backward(c1_a, c2_a, c1_b, c2_b, y_a, y_b)
        ctx.slope = slope
        ctx.set_materialize_grads(False)
        return y_a, y_b

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_a, grad_b):
        c1_a, c2_a, c1_b, c2_b, y_a, y_b = ctx.saved_tensors
        return cabi.correlation_lrelu_backward_pair(c1_a, c2_a, y_a, grad_a, c1_b, c2_b, y_b, grad_b, 4, 1, 4, 1, 1, ctx.slope,
                                                    want=tuple(ctx.needs_input_grad[:4])) + (None,)


def _no_out_in_grad_mode(out, what):
    if out is not None:
        raise RuntimeError("%s: out= is for inference; under autograd the result is the tensor the backward saves" % what)


def corr_lrelu(c1, c2, negative_slope=0.1, out=None):
    """`self.leakyRELU(self.corr(c1, c2))` of PWCDCNet.forward (PWCNet/PWCNet.py:230-231) from the correlation's launch:
    the bits of F.leaky_relu on the correlation's output.  Differentiable when grad mode is on and an input requires grad
    (one backward call, which masks the gradient as it loads it and takes torch.cat's strided gradient without a copy).
    Otherwise the plain launch, and out= may name where to write: buf[:, k:k + 81] of the contiguous NCHW buffer the
    reference would get from `torch.cat((corr, ...), 1)`.  float32 only: bfloat16 and float16 tensors
    raise, as they always have.  On bfloat16 use `warp_corr_lrelu` (the warped levels), and for a level without a warp
    `_CorrLrelu.apply(c1, c2, slope)` (trainable) or `cabi.correlation_lrelu_forward(..., out=)`: the bits of F.leaky_relu on
    the bfloat16 cost volume -- the mean rounded first, the activation rounded again."""
    _float32_only("corr_lrelu", "warp_corr_lrelu and _CorrLrelu.apply take bfloat16", c1, c2)
    if _wants_grad(c1, c2):
        _no_out_in_grad_mode(out, "corr_lrelu")
        return _CorrLrelu.apply(c1, c2, float(negative_slope))
    return cabi.correlation_lrelu_forward(c1, c2, 4, 1, 4, 1, 1, negative_slope, out=out)


def warp_corr_lrelu(c1, c2, flo, align_corners=True, negative_slope=0.1, out=None):
    """`self.leakyRELU(self.corr(c1, self.warp(c2, flo)))` (PWCNet/PWCNet.py:244-248 ...): the warp, then the correlation
    with the LeakyReLU in its launch.  Differentiable as `warp_corr` is; in inference out= as `corr_lrelu`'s.  float32, or
    bfloat16 features (out= included) with a float32 or a bfloat16 flow: a PWC-Net level under
    torch.autocast(dtype=torch.bfloat16) is these two launches, with no cast and, with out=, no copy into the
    concatenation; the bits are those of F.leaky_relu on the bfloat16 cost volume, and the backward's those of autograd
    through it.  float16 raises."""
    if _wants_grad(c1, c2, flo):
        _no_out_in_grad_mode(out, "warp_corr_lrelu")
        return _CorrLrelu.apply(c1, _warp(c2, flo, align_corners), float(negative_slope))
    return cabi.correlation_lrelu_forward(c1, _warp(c2, flo, align_corners), 4, 1, 4, 1, 1, negative_slope, out=out)


def corr_pair_lrelu(c1_a, c2_a, c1_b, c2_b, negative_slope=0.1, out=None):
    """`corr_pair` followed by the reference's LeakyReLU on both cost volumes, from the one launch.  Differentiable when
    grad mode is on and one of the four inputs requires grad: ONE backward call for the gradients that are needed, each
    bit-equal to `F.leaky_relu(corr_pair(...))`'s.  Otherwise the plain launch; out= is then a pair of destinations
    (either may be None), each as `corr_lrelu`'s.  float32, or bfloat16 for all four features (and out=): the level of both
    flow networks under torch.autocast(dtype=torch.bfloat16) in one launch each way, every tensor bit-equal to
    `_CorrLrelu.apply`'s on its item -- F.leaky_relu on the bfloat16 cost volume, and autograd through it.  float16 raises."""
    if _wants_grad(c1_a, c2_a, c1_b, c2_b):
        _no_out_in_grad_mode(out, "corr_pair_lrelu")
        return _CorrPairLrelu.apply(c1_a, c2_a, c1_b, c2_b, float(negative_slope))
    return cabi.correlation_lrelu_forward_pair(c1_a, c2_a, c1_b, c2_b, 4, 1, 4, 1, 1, negative_slope, out=out)


class _PartLoss(torch.autograd.Function):
    """The losses of one `part_loss` call as ONE tensor of nd + 2 values (vfi_part_loss_forward); the backward is ONE launch
    (vfi_part_loss_backward) over the dense gradient vector autograd hands back.  `used` is the host-side set of loss
    indices whose element received a gradient in this backward pass (filled by the hooks `part_loss` puts on the elements
    it hands out): a loss outside it is an absent term, so `pixel_loss[1].backward()` is one elementwise pass over one
    tensor.  Nothing synchronises with the host."""

    @staticmethod
    def forward(ctx, epsilon, neg_psnr, used, target, flow0, flow1, img0, img1, *diffs):
        values, means = _part_loss_launch(diffs, target, flow0, flow1, img0, img1, epsilon, neg_psnr)
        ctx.epsilon, ctx.neg_psnr, ctx.used, ctx.nd = epsilon, neg_psnr, used, len(diffs)
        ctx.has_target, ctx.has_flows = target is not None, flow0 is not None
        ctx.save_for_backward(means, *diffs, *([target] if target is not None else []),
                              *([flow0, flow1, img0, img1] if flow0 is not None else []))
        return values

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_values):
        nd, saved = ctx.nd, ctx.saved_tensors
        means, diffs = saved[0], list(saved[1:1 + nd])
        rest = list(saved[1 + nd:])
        target = rest.pop(0) if ctx.has_target else None
        flow0, flow1, img0, img1 = rest if ctx.has_flows else (None, None, None, None)
        used = sorted(ctx.used) if ctx.used else list(range(nd + 2))      # (no hook ran: values was used whole)
        ctx.used.clear()
        mask = sum(1 << j for j in used)
        gds = [torch.empty_like(d) if ctx.needs_input_grad[8 + i] and (mask >> i) & 1 else None for i, d in enumerate(diffs)]
        flow_terms = ctx.has_flows and (mask >> nd) & 3
        gf0 = torch.empty_like(flow0) if flow_terms and ctx.needs_input_grad[4] else None
        gf1 = torch.empty_like(flow1) if flow_terms and ctx.needs_input_grad[5] else None
        if any(g is not None for g in (*gds, gf0, gf1)):
            gv = grad_values.to(torch.float32).contiguous()
            _check(cabi.part_loss_backward(diffs, target, flow0, flow1, img0, img1, ctx.epsilon, ctx.neg_psnr, gv, means, mask,
                                           gds, gf0, gf1), "part_loss_backward")
        return (None, None, None, None, gf0, gf1, None, None, *gds)


def _part_loss_launch(diffs, target, flow0, flow1, img0, img1, epsilon, neg_psnr):
    d0 = diffs[0]
    values = torch.empty(len(diffs) + 2, device=d0.device, dtype=torch.float32)
    means = torch.empty(len(diffs) * d0.size(0), device=d0.device, dtype=torch.float32)
    _check(cabi.part_loss_forward(list(diffs), target, flow0, flow1, img0, img1, epsilon, neg_psnr, values, means),
           "part_loss_forward")
    return values, means


def _part_loss_call(diffs, target, flow0, flow1, img0, img1, epsilon, neg_psnr):
    """values[nd + 2] of one library call, with the autograd Function when something can train"""
    diffs = list(diffs)
    d0 = diffs[0]
    if d0.dim() == 4 and not all(cabi._same_strides(d, d0) and d.stride(3) == 1 for d in diffs):
        diffs = [d.contiguous() for d in diffs]
    if target is not None and not cabi._same_strides(target, diffs[0]):     # (the library addresses target like the diffs)
        diffs, target = [d.contiguous() for d in diffs], target.contiguous()
    if flow0 is not None and not cabi._same_strides(flow0, flow1):
        flow0, flow1 = flow0.contiguous(), flow1.contiguous()
    if flow0 is not None and not cabi._same_strides(img0, img1):
        img0, img1 = img0.contiguous(), img1.contiguous()
    trainable = [t for t in (*diffs, flow0, flow1) if t is not None]
    if not _wants_grad(*trainable):
        return _part_loss_launch(diffs, target, flow0, flow1, img0, img1, epsilon, neg_psnr)[0], None
    used = set()
    return _PartLoss.apply(epsilon, neg_psnr, used, target, flow0, flow1, img0, img1, *diffs), used


def _hand_out(values, used, indices):
    """the elements of `values` as 0-dim tensors; each notes on the host that its loss received a gradient"""
    out = []
    for j in indices:
        v = values[j]
        if used is not None and v.requires_grad:
            v.register_hook(lambda g, j=j: used.add(j))
        out.append(v)
    return out


def part_loss(diffs, offsets, occlusions, images, epsilon, use_negPSNR=False, target=None):
    """`loss_function.part_loss` as `train.py` calls it: returns (pixel_loss, offset_loss, sym_loss), lists of 0-dim tensors.
      pixel_loss[i]  the Charbonnier loss of diffs[i] (the negative-PSNR form with use_negPSNR); with `target` the entries of
                     diffs are the network's outputs and diffs[i] - target is formed inside the kernel, never stored;
      offset_loss[k] the gradient-adaptive total variation of offsets[k] = [flow0, flow1] against images = [I0, I1]; one
                     zero when offsets[0][0] is None, as in the reference;
      sym_loss[k]    the motion-symmetry loss of offsets[k] (none when offsets[0][0] is None: the reference cannot form it).
    occlusions is accepted and ignored, as in the reference.  The diffs and the first flow pair are one call of the library
    (one forward launch plus a small finish launch); further pairs are calls of their own.  Differentiable when grad mode
    is on and a diff or flow requires grad: the backward is one launch that computes only what the losses actually used
    ask for, reproducible bit for bit.  Otherwise the plain forward, with no grad_fn.  Images and target are data: one
    that requires grad is refused, not given a silent zero gradient."""
    diffs = list(diffs)
    if not diffs:
        raise RuntimeError("part_loss: no diffs")
    pairs = [] if offsets[0][0] is None else [(o[0], o[1]) for o in offsets]
    for t in (*(images if pairs else ()), *([target] if target is not None else [])):
        if t.requires_grad:
            raise RuntimeError("part_loss: images and target are data; a tensor among them requires grad")
    epsilon, neg = float(epsilon), bool(use_negPSNR)
    nd = len(diffs)
    pixel_loss, offset_loss, sym_loss = [], [], []
    for k in range(0, nd, cabi.PART_LOSS_ITEMS):
        chunk = diffs[k:k + cabi.PART_LOSS_ITEMS]
        first = pairs[0] if pairs and k == 0 else (None, None)
        values, used = _part_loss_call(chunk, target, first[0], first[1], images[0] if pairs else None,
                                       images[1] if pairs else None, epsilon, neg)
        picked = _hand_out(values, used, range(len(chunk) + (2 if k == 0 and pairs else 0)))
        pixel_loss += picked[:len(chunk)]
        if k == 0 and pairs:
            offset_loss.append(picked[len(chunk)])
            sym_loss.append(picked[len(chunk) + 1])
    for f0, f1 in pairs[1:]:
        # (the library's call carries at least one diff: the first one rides along and its value is not handed out)
        values, used = _part_loss_call([diffs[0].detach()], None if target is None else target, f0, f1, images[0], images[1],
                                       epsilon, neg)
        picked = _hand_out(values, used, (1, 2))
        offset_loss.append(picked[0])
        sym_loss.append(picked[1])
    if not pairs:
        offset_loss = [torch.zeros(1, device=diffs[0].device)]
    return pixel_loss, offset_loss, sym_loss


def padding_for(height, width):
    """(left, right, top, bottom) of `demo_MiddleBury.py:294-310`: next multiple of 128, or 32 each side."""
    def one(n):
        if n != ((n >> 7) << 7):
            total = (((n >> 7) + 1) << 7) - n
            return int(total / 2), total - int(total / 2)
        return 32, 32
    left, right = one(width)
    top, bottom = one(height)
    return left, right, top, bottom


def frames_to_padded(frames_u8):
    """uint8 [B,h,w,3] on the GPU -> float32 [B,3,H,W] / 255 with replication padding; returns (tensor, padding)."""
    b, h, w, _ = frames_u8.shape
    left, right, top, bottom = padding_for(h, w)
    out = torch.empty((b, 3, h + top + bottom, w + left + right), device=frames_u8.device, dtype=torch.float32)
    _check(cabi.frame_u8_to_planar(frames_u8, out, left, right, top, bottom), "frame_u8_to_planar")
    return out, (left, right, top, bottom)


def padded_to_frames(y, height, width, padding):
    """float32 [B,3,H,W] -> uint8 [B,height,width,3]: clip, crop, x255, round (`demo_MiddleBury.py:350-364`)."""
    left, _, top, _ = padding
    out = torch.empty((y.size(0), height, width, 3), device=y.device, dtype=torch.uint8)
    _check(cabi.planar_to_frame_u8(y, out, top, left), "planar_to_frame_u8")
    return out


def interpolation_error_and_psnr(rec_u8, gt_u8):
    """(mean |rec - gt|, PSNR in dB) of `demo_MiddleBury.py:370-381`; the sums are exact integers."""
    sums = torch.zeros(2, device=rec_u8.device, dtype=torch.int64)
    _check(cabi.frame_error_sums(rec_u8, gt_u8, sums), "frame_error_sums")
    s_abs, s_sq = (int(v) for v in sums.cpu())
    n = rec_u8.numel()
    mse = s_sq / n
    psnr = float("inf") if mse == 0 else 20 * math.log10(255.0 / math.sqrt(mse))
    return s_abs / n, psnr


def ssim(rec_u8, gt_u8):
    """Mean SSIM of uint8 frames [B,h,w,3] as `demo_MiddleBury.py:382-388` computes it (`ssim()` :40-162 on the
    colour planes / 255: 11-tap sigma-1.5 Gaussian without padding, data_range 1)."""
    sums = torch.zeros(1, device=rec_u8.device, dtype=torch.int64)
    _check(cabi.frame_ssim_sums(rec_u8, gt_u8, sums), "frame_ssim_sums")
    b, h, w, _ = rec_u8.shape
    n = b * 3 * (h - 10 if h >= 11 else h) * (w - 10 if w >= 11 else w)
    return int(sums.cpu()[0]) / 4294967296.0 / n
