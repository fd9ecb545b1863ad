/*
 * vfi_hip.h -- C ABI of libvfi_hip.so, the MI355X (gfx950) implementation of the
 * DAIN / VFIDKR frame-synthesis hot path.
 *
 * One entry point per function the reference's pybind11 extension modules
 * export.  No torch types cross this boundary: device
 * pointers, sizes, element strides and a HIP stream.  The torch extension
 * modules in csrc/shim/ (same module and function names as the reference's)
 * and the ctypes loader in the package are both thin callers of this ABI.
 *
 * Conventions (kept from the reference bindings unless stated):
 *  - tensors are float32, NCHW, innermost (w) stride 1 (the one exception: the
 *    vfi_filterinterp_forward_ori_nhwc_* entries, which say so); `*_s` arguments are the
 *    batch / channel / row strides IN ELEMENTS (int64: a 196-channel 4K tensor
 *    overflows the reference's 32-bit offsets for batch >= 2);
 *  - all pointers are DEVICE pointers valid on the device `stream` belongs to;
 *  - calls are asynchronous: kernels are enqueued on `stream`, nothing syncs;
 *  - return value: 0 = success, 1 = shape/stride problem (the reference
 *    bindings' silent `return 1`), VFI_ERR_LAUNCH = a HIP launch failed (the
 *    reference bindings raise AT_ERROR("CUDA call failed") for it);
 *  - the reference's my_package ops expect the CALLER to zero-fill outputs /
 *    counts / grads (FilterInterpolationLayer.py:34, FlowProjectionLayer.py:35-36).
 *    Every FORWARD entry point here writes every element of its outputs
 *    (`count` and `output` of the projections included), so forward outputs need
 *    no zero fill; a zero-filled buffer is of course accepted.  Every grad*
 *    buffer of a BACKWARD must arrive zeroed exactly as in the reference.
 */
#ifndef VFI_HIP_H
#define VFI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VFI_OK          0
#define VFI_ERR_SHAPE   1
#define VFI_ERR_LAUNCH  (-2)

typedef void* vfi_stream_t;           /* hipStream_t */

/* strides of one NCHW tensor, in elements; w stride is 1 by contract */
typedef struct vfi_strides {
    int64_t b, c, h;
} vfi_strides;

/* library / build identification: "vfi_hip <version> gfx950" */
const char* vfi_version(void);

/* ---- filterinterpolation_cuda ------------------------------------------------
 * replaces FilterInterpolationLayer_gpu_forward_ori / _backward_ori
 * (filterinterpolation_cuda.cc:537-606, 608-687).  filter_channels = input3.size(1);
 * filter_size = (int)sqrt((float)filter_channels) as the binding computes it.
 * output uses input1's strides (the binding checks they are equal, cc:582-583). */
int vfi_filterinterp_forward_ori(const float* input1, const float* input2, const float* input3,
                                 float* output,
                                 int batch, int channel, int h, int w, int filter_channels,
                                 vfi_strides s1, vfi_strides s2, vfi_strides s3,
                                 vfi_stream_t stream);
int vfi_filterinterp_backward_ori(const float* input1, const float* input2, const float* input3,
                                  const float* gradoutput,
                                  float* gradinput1, float* gradinput2, float* gradinput3,
                                  int batch, int channel, int h, int w, int filter_channels,
                                  vfi_strides s1, vfi_strides s2, vfi_strides s3,
                                  vfi_stream_t stream);

/* The same forward for SEVERAL flows over one image and one filter: outputs[t] = the function above with
 * input2 = flows[t], t < nflows (bit for bit).  This is what DAIN_slowmotion does per direction: FilterInterpolate_ctx
 * (networks/DAIN_slowmotion.py:167-183, 311-317) warps the same context tensor with the same filter once per time
 * offset.  With filter_channels == 16 one launch stages ONE window per tile and channel for two flows (half the image
 * traffic per output; more flows go in pairs, a last odd one alone: the three time offsets of DAIN_slowmotion x4 = one
 * two-flow launch + one single-flow launch -- measured faster than a three-flow launch, whose union window outgrows the
 * LDS ring); other filter sizes are single launches.
 * flows / outputs: HOST arrays of nflows device pointers; every flow has strides s2, every output s1. */
int vfi_filterinterp_forward_ori_multi(const float* input1, const float* const* flows, const float* input3,
                                       float* const* outputs, int nflows,
                                       int batch, int channel, int h, int w, int filter_channels,
                                       vfi_strides s1, vfi_strides s2, vfi_strides s3,
                                       vfi_stream_t stream);

/* The same call with a destination layout of its own: outputs[t] holds, bit for bit, what
 * vfi_filterinterp_forward_ori_multi writes, addressed with s_out instead of s1.  For a caller that needs the warps inside a
 * wider tensor -- the input of the reference's rectifyNet is torch.cat((cur_output, ref0, ref2, offsets, filters, ctx0, ctx2),
 * dim=1), networks/DAIN_slowmotion.py:177-182 -- and would otherwise copy every one of them once more: outputs[t] is then
 * the first element of a channel slice of that buffer.
 * Contract of s_out: w stride 1; s_out.h == s1.h (a pixel's offset inside a plane is shared by the load and the store:
 * any other row stride returns VFI_ERR_SHAPE, it is not served by a slower kernel); s_out.b and s_out.c are free.  A
 * contiguous [B, C', h, w] buffer meets it whenever input1 is contiguous or itself a channel slice of such a tensor.
 * Every store is one float: outputs[t] needs 4-byte alignment only.  The kernel and the window class a tile takes depend on
 * the inputs alone (same kernels, same pairing of the flows, any nflows >= 1).  The destinations must not overlap input1,
 * the flows, input3 or each other: documented, not checked, as for the entry above.  s_out == s1 is that entry. */
int vfi_filterinterp_forward_ori_multi_to(const float* input1, const float* const* flows, const float* input3,
                                          float* const* outputs, int nflows,
                                          int batch, int channel, int h, int w, int filter_channels,
                                          vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides s_out,
                                          vfi_stream_t stream);

/* The backward of that call as the context path needs it (networks/DAIN.py:544-552, networks/DAIN_slowmotion.py:311-317
 * detach flow and filter): gradinput1 = the sum over t < nflows of the IMAGE gradient of
 * vfi_filterinterp_forward_ori(., flows[t], input3) for gradoutputs[t].  The image itself is not an argument: its gradient
 * depends on the flow, the filter and the incoming gradient only.  No flow or filter gradient is formed.
 * gradinput1 is WRITTEN, every element (+0 where no tap lands): it need not arrive zeroed.  An invalid pixel contributes
 * nothing (filterinterpolation_cuda_kernel.cu:2863-2864).  Deterministic (one fixed-point accumulation over all flows, one
 * scale from the largest |gradient| of all of them and the largest |filter tap|; a cell may take all filter_channels x nflows
 * taps of every pixel); for nflows == 1 bit for bit gradinput1 of vfi_filterinterp_backward_ori on a zero-filled buffer.
 * Non-finite inputs: the reference's fp32 atomics, as there.
 * flows / gradoutputs: HOST arrays of nflows device pointers, every entry non-null; every flow has strides s2, every
 * gradoutput sg, gradinput1 s1.  Scratch: 8 bytes per element of gradinput1 (the per-stream workspace). */
int vfi_filterinterp_backward_ori_image_multi(const float* const* flows, const float* input3,
                                              const float* const* gradoutputs, float* gradinput1, int nflows,
                                              int batch, int channel, int h, int w, int filter_channels,
                                              vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides sg,
                                              vfi_stream_t stream);

/* fp16 STORAGE, fp32 arithmetic (BASELINE.json configs[2]): input1 and output are IEEE
 * half tensors (strides in half elements), flow and filter stay float32.  The result is the fp32
 * result of the function above on the widened inputs, rounded to half once; the LDS-staged path
 * (filter_channels == 16) sums the 16 products in one chain and agrees with that to fp16 rounding. */
int vfi_filterinterp_forward_ori_f16(const void* input1_half, const float* input2, const float* input3,
                                     void* output_half,
                                     int batch, int channel, int h, int w, int filter_channels,
                                     vfi_strides s1, vfi_strides s2, vfi_strides s3,
                                     vfi_stream_t stream);

/* bfloat16 STORAGE of the image and the outputs, float32 arithmetic: vfi_filterinterp_forward_ori_multi_to for a network
 * that runs under bfloat16 autocast (the context warp, C = 196).  input1 and outputs[t] are bfloat16 tensors (strides in
 * bfloat16 elements), flows and filter stay float32 (2 and 16 channels against 196).  The 16-bit patterns are widened
 * exactly, the arithmetic is the float32 kernels' -- four quadrant chains and the blend, clamped taps read as replicated
 * values; nothing is folded as in the fp16 entry above -- and each result is rounded once, to nearest even: every output
 * element is, bit for bit, bf16_rne of what vfi_filterinterp_forward_ori writes for the widened image.  NaN stays NaN at the
 * same positions; an invalid pixel copies the input's bits through.
 * Contract of s_out as above: w stride 1, s_out.h == s1.h (else VFI_ERR_SHAPE), s_out.b and s_out.c free; every store is
 * one 2-byte element, so outputs[t] needs 2-byte alignment only.  filter_channels == 16 with even s1.h, s1.c, s1.b and a
 * 4-byte aligned input1 takes the LDS-staged kernel; everything else (any filter size, any strides, 2-byte alignment) the
 * one-thread-per-pixel kernel, with the same bits.  One launch per flow (no shared-window kernel).  batch <= 65535. */
int vfi_filterinterp_forward_ori_multi_to_bf16(const void* input1_bf16, const float* const* flows, const float* input3,
                                               void* const* outputs_bf16, int nflows,
                                               int batch, int channel, int h, int w, int filter_channels,
                                               vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides s_out,
                                               vfi_stream_t stream);

/* ---- channels_last (NHWC) images: the one exception to "NCHW, innermost stride 1" above ----
 * The context warp for a network that keeps its activations in torch.channels_last (the layout 16-bit convolutions are
 * usually run in): vfi_filterinterp_forward_ori_multi_to[_bf16] on an image and destinations whose CHANNEL stride is 1,
 * without a .contiguous() copy of the image on the way in and a channels_last copy of every output on the way out.
 * Forward only (the image gradient is vfi_filterinterp_backward_ori_nhwc_image_multi[_bf16], below).
 *   input1, outputs[t]   [batch, channel, h, w] with channel stride 1; batch, row and pixel strides in ELEMENTS in a
 *                        vfi_strides_nhwc.  input1 (s1) may be a dense channels_last tensor or a channel slice of a wider
 *                        one.  Every output has the layout s_out, which is its own: all three strides are free, so
 *                        buf[:, 45:45 + channel] of a channels_last [batch, 437, h, w] buffer is a legal destination.
 *   flows[t], input3     float32, four element strides each (s2 for every flow, s3): NCHW and channels_last are both
 *                        accepted.  Per pixel they are 2 + filter_channels scalar reads shared by all channels.
 * Values: every output element is, bit for bit, what the NCHW entry writes for the same logical tensors --
 * vfi_filterinterp_forward_ori_multi in float32, vfi_filterinterp_forward_ori_multi_to_bf16 in bfloat16 (bf16_rne of the
 * float32 result on the widened image).  NaN stays NaN at the same positions; an invalid pixel copies the input's bits
 * through; every filter_channels >= 1 is accepted (filter_size 4 reads the first 16 filter channels, as there).
 * Alignment: an access is 16, 8 or 4 bytes wide or one element, the widest that divides the address of input1, the address
 * of EVERY output and every stride of s1 and s_out that the shape uses (a dense bfloat16 tensor of 196 channels: 8 bytes;
 * an odd channel offset or an odd pixel stride: one element).  No misaligned vector access is issued, and every width
 * writes the same bits.  channel need not be a multiple of the width.
 * Refusals, all VFI_ERR_SHAPE before any launch: a null pointer (a null entry of flows or outputs included), nflows < 1,
 * batch, channel, h, w or filter_channels < 1, batch > 65535, more than 2^28 tiles of 32 x 4 pixels.  The destinations
 * must not overlap input1, the flows, input3 or each other: documented, not checked, as for the entries above.  One
 * launch per flow, no allocation, no synchronisation: legal inside a stream capture. */
typedef struct vfi_strides_nhwc {
    int64_t b, h, w;                  /* channel stride is 1 by contract */
} vfi_strides_nhwc;
typedef struct vfi_strides4 {
    int64_t b, c, h, w;
} vfi_strides4;
int vfi_filterinterp_forward_ori_nhwc_multi_to(const float* input1, const float* const* flows, const float* input3,
                                               float* const* outputs, int nflows,
                                               int batch, int channel, int h, int w, int filter_channels,
                                               vfi_strides_nhwc s1, vfi_strides4 s2, vfi_strides4 s3,
                                               vfi_strides_nhwc s_out, vfi_stream_t stream);
int vfi_filterinterp_forward_ori_nhwc_multi_to_bf16(const void* input1_bf16, const float* const* flows, const float* input3,
                                                    void* const* outputs_bf16, int nflows,
                                                    int batch, int channel, int h, int w, int filter_channels,
                                                    vfi_strides_nhwc s1, vfi_strides4 s2, vfi_strides4 s3,
                                                    vfi_strides_nhwc s_out, vfi_stream_t stream);

/* vfi_filterinterp_backward_ori_image_multi on bfloat16 gradients: gradoutputs[t] (strides sg) and gradinput1 (strides s1)
 * are bfloat16 tensors, flows and filter float32.  gradinput1 is, bit for bit, bf16_rne of what the float32 entry writes
 * for the widened gradients: the same kernels on widened gradient rows, one fixed-point accumulation over all flows at the
 * float32 call's scale, every element WRITTEN, reproducible bit for bit.  A call with a non-finite gradient or filter, or
 * magnitudes whose product can overflow, scatters FLOATS with fp32 atomics into the zeroed scratch cells and rounds each
 * once at the end: no atomic touches bfloat16 storage.  Scratch: 8 bytes per element of gradinput1. */
int vfi_filterinterp_backward_ori_image_multi_bf16(const float* const* flows, const float* input3,
                                                   const void* const* gradoutputs_bf16, void* gradinput1_bf16, int nflows,
                                                   int batch, int channel, int h, int w, int filter_channels,
                                                   vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides sg,
                                                   vfi_stream_t stream);

/* ---- channels_last (NHWC) gradients: the backward of the channels_last context warp ----
 * vfi_filterinterp_backward_ori_image_multi[_bf16] for gradients and a result whose CHANNEL stride is 1: gradinput1 = the
 * sum over t < nflows of the image gradient of FilterInterpolation `_ori` for gradoutputs[t], without a .contiguous() copy of
 * every incoming gradient and a channels_last copy of the result.
 *   gradoutputs[t]       [batch, channel, h, w] with channel stride 1, all of layout sg.
 *   gradinput1           the same shape with channel stride 1, layout s1.  Batch, row and pixel strides are free on both
 *                        sides: a channel slice of a wider channels_last buffer is legal as a gradient and as the result.
 *   flows[t], input3     float32, four element strides each (s2 for every flow, s3), NCHW or channels_last, as in the
 *                        forward entries above.
 * Values: every element of gradinput1 is, bit for bit, what vfi_filterinterp_backward_ori_image_multi writes for the same
 * logical tensors (the _bf16 entry: bf16_rne of the float32 entry's result on the widened gradients).  The fixed-point sums do
 * not depend on the order of the addends, every addend is formed as the NCHW kernels form it, and the scale is the NCHW
 * call's: the largest |gradient| over all flows, the largest |filter tap|, a cell taking max(filter_channels, 4) x nflows
 * taps of every pixel.  gradinput1 is WRITTEN, every element (+0 where no tap lands): it need not arrive zeroed.  An invalid
 * pixel contributes nothing.  Reproducible bit for bit.  A call with a non-finite gradient or filter, or magnitudes whose
 * product can overflow, scatters with fp32 atomics as the NCHW entries do: float32 into gradinput1, zeroed first; bfloat16
 * as floats into the low words of the zeroed scratch cells, rounded once at the end -- no atomic touches bfloat16 storage.
 * Kernels: filter_channels == 16 sums a tile's window slab by slab of 16 channels in LDS and flushes 128-byte runs of the
 * [b][y][x][c] scratch; any other filter size, a call on the fp32 path or with tiny gradients (a second scale factor), and
 * the tiles whose window does not fit, take the per-addend kernel: the same addends, the same bits.  The gradient loads are
 * 16, 8 or 4 bytes wide or one element, the widest that divides the address of EVERY gradient and every stride of sg that the
 * shape uses; no misaligned vector access is issued, and channel need not be a multiple of anything.
 * Refusals, all VFI_ERR_SHAPE before any launch: a null pointer (a null entry of flows or gradoutputs included), nflows < 1,
 * batch, channel, h, w or filter_channels < 1, batch > 65535, more than 2^28 tiles of 32 x 4 pixels (or tiles x launches of
 * three flows past INT_MAX); and, for gradients or a result whose pixels are NOT contiguous (pixel stride != channel: a
 * channel slice), batch x h x w > INT_MAX -- the conversion walks such a tensor pixel by pixel and counts them in an int
 * (a dense channels_last tensor is walked row by row: w x channel <= INT_MAX there).  Scratch: 8 bytes per element of gradinput1 (the per-stream workspace); no other allocation, no
 * synchronisation: legal inside a stream capture. */
int vfi_filterinterp_backward_ori_nhwc_image_multi(const float* const* flows, const float* input3,
                                                   const float* const* gradoutputs, float* gradinput1, int nflows,
                                                   int batch, int channel, int h, int w, int filter_channels,
                                                   vfi_strides_nhwc s1, vfi_strides4 s2, vfi_strides4 s3, vfi_strides_nhwc sg,
                                                   vfi_stream_t stream);
int vfi_filterinterp_backward_ori_nhwc_image_multi_bf16(const float* const* flows, const float* input3,
                                                        const void* const* gradoutputs_bf16, void* gradinput1_bf16, int nflows,
                                                        int batch, int channel, int h, int w, int filter_channels,
                                                        vfi_strides_nhwc s1, vfi_strides4 s2, vfi_strides4 s3,
                                                        vfi_strides_nhwc sg, vfi_stream_t stream);

/* deformable-kernel variants (filterinterpolation_cuda.cc:11-92, 191-272, 374-447).
 * variant: 0 = FilterInterpolationLayer_gpu_forward (4 inputs, fs in {4,6}),
 *          1 = ..._forward_deforconv, 2 = ..._forward_nofilterwithdeforconv
 *              (input3 is the 2*fs*fs offset field, input4 unused/NULL).
 * Documented divergence: the reference reads out of bounds when a displaced tap
 * leaves the image; here the four bilinear corners are clamped to the image. */
#define VFI_DEFOR_OFFSET   0
#define VFI_DEFOR_REGION   1
#define VFI_DEFOR_NOFILTER 2
int vfi_filterinterp_forward_defor(int variant,
                                   const float* input1, const float* input2, const float* input3,
                                   const float* input4, float* output,
                                   int batch, int channel, int h, int w, int filter_size,
                                   vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides s4,
                                   vfi_stream_t stream);

/* backward of the same three variants: FilterInterpolationLayer_gpu_backward (cc:93-187),
 * ..._backward_deforconv (cc:273-367), ..._backward_nofilterwithdeforconv (cc:448-533).
 * gradinput1..4 must arrive zeroed.  variant 2: input3 / gradinput3 are the offset field and its
 * gradient, input4 / gradinput4 unused (NULL).  gradoutput is addressed with input1's strides,
 * gradinput_k with input_k's, as in the reference. */
int vfi_filterinterp_backward_defor(int variant,
                                    const float* input1, const float* input2, const float* input3,
                                    const float* input4, const float* gradoutput,
                                    float* gradinput1, float* gradinput2, float* gradinput3, float* gradinput4,
                                    int batch, int channel, int h, int w, int filter_size,
                                    vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides s4,
                                    vfi_stream_t stream);

/* ---- flowprojection_cuda -----------------------------------------------------
 * replaces FlowProjectionLayer_gpu_forward / _backward (flowprojection_cuda.cc:9-57, 59-114).
 * count [B,1,H,W] and output [B,2,H,W] are fully written (no zero fill needed).
 * The forward keeps a per-(device, stream) workspace (block tables, bitmaps, three scratch planes: about
 * 13 bytes per pixel), allocated on the first call for a stream and replaced by a larger one when a larger
 * frame arrives.  hipMalloc is not legal inside a stream capture: call vfi_projection_reserve (or make one
 * warm-up call) before capturing into a HIP graph.  A buffer that has been outgrown is retired, never freed,
 * so a graph captured earlier stays replayable; vfi_release_workspaces() frees everything. */
int vfi_flowprojection_forward(const float* input1, float* count, float* output,
                               int batch, int h, int w, int fillhole,
                               vfi_strides s1, vfi_strides sc,
                               vfi_stream_t stream);
int vfi_flowprojection_backward(const float* input1, const float* count, const float* gradoutput,
                                float* gradinput1,
                                int batch, int h, int w,
                                vfi_strides s1, vfi_strides sc,
                                vfi_stream_t stream);

/* FlowProject(inputs, depth) of the networks (networks/DAIN.py:533-539, networks/DAIN_slowmotion.py:301-307 -- the reference
 * loops over the list, one FlowProjectionModule call per flow, and does so for both directions back to back,
 * DAIN.py:215-220 / DAIN_slowmotion.py:156-159): the whole list in ONE launch triple (per 8 items), so that the three
 * dependent launches of a projection are paid once per list, not once per flow.  inputs1 / counts / outputs: HOST arrays of
 * nitems device pointers, item i = [batch,2,h,w] flow -> [batch,1,h,w] count + [batch,2,h,w] output; all items share
 * shape and strides (s1: flows and outputs, sc: counts).  Every item needs its own count and output (they are written
 * concurrently: two equal pointers are refused with VFI_ERR_SHAPE).  Results per item: vfi_flowprojection_forward's, bit for
 * bit.  The workspace must cover nitems * batch frames: vfi_projection_reserve(nitems * batch, h, w, stream) before a capture. */
int vfi_flowprojection_forward_batch(const float* const* inputs1, float* const* counts, float* const* outputs,
                                     int nitems, int batch, int h, int w, int fillhole,
                                     vfi_strides s1, vfi_strides sc,
                                     vfi_stream_t stream);

/* Make the projection workspace of `stream` large enough for [batch, *, h, w] frames (both projections and
 * their _up4 forms; h, w are the full-resolution sizes).  Allocates, so call it outside a capture. */
int vfi_projection_reserve(int batch, int h, int w, vfi_stream_t stream);
/* Synchronises the devices involved and frees every workspace the library holds (live and retired) on every
 * stream.  Call only when no launch or captured graph of this library is still to run; later calls
 * allocate afresh. */
int vfi_release_workspaces(void);

/* ---- depthflowprojection_cuda ------------------------------------------------
 * replaces DepthFlowProjectionLayer_gpu_forward / _backward
 * (depthflowprojection_cuda.cc:10-68, 70-139). */
int vfi_depthflowprojection_forward(const float* input1, const float* input2,
                                    float* count, float* output,
                                    int batch, int h, int w, int fillhole,
                                    vfi_strides s1, vfi_strides s2, vfi_strides sc,
                                    vfi_stream_t stream);
/* the list form (see vfi_flowprojection_forward_batch); inputs2[i] is item i's depth weight [batch,1,h,w] with strides s2 --
 * items may share one (DAIN_slowmotion projects every time offset of a direction with that direction's depth) */
int vfi_depthflowprojection_forward_batch(const float* const* inputs1, const float* const* inputs2,
                                          float* const* counts, float* const* outputs,
                                          int nitems, int batch, int h, int w, int fillhole,
                                          vfi_strides s1, vfi_strides s2, vfi_strides sc,
                                          vfi_stream_t stream);
int vfi_depthflowprojection_backward(const float* input1, const float* input2,
                                     const float* count, const float* output,
                                     const float* gradoutput,
                                     float* gradinput1, float* gradinput2,
                                     int batch, int h, int w,
                                     vfi_strides s1, vfi_strides s2, vfi_strides sc,
                                     vfi_stream_t stream);

/* ---- mindepthflowprojection_cuda --------------------------------------------
 * replaces minDepthFlowProjectionLayer_gpu_forward / _backward
 * (mindepthflowprojection_cuda.cc:12-66, 68-139).  Each target keeps the (negated) flow of the
 * source with the largest weight `input2` that lands on it (top-left integer neighbour only) and
 * that weight in `count`.  The reference does this with an unguarded read-compare-write and is
 * scheduling dependent; this library returns what those statements give when the sources are
 * visited in raster order (largest weight above the incoming `count`, first source on ties;
 * -0.0 and +0.0 are one weight, and `count` receives the winner's own bits).  The reference's
 * wrapper zero-fills count and output.  A non-zero incoming `count` is a floor: only a weight
 * above it is recorded, and a target no source beats keeps its incoming count and output.
 * The forward keeps a per-stream scratch buffer of about 8.3 bytes per pixel (keys + two bitmaps).  The backward gives
 * gradinput1 only: the reference never writes gradinput2 (its code for it is commented out). */
int vfi_mindepthflowprojection_forward(const float* input1, const float* input2,
                                       float* count, float* output,
                                       int batch, int h, int w, int fillhole,
                                       vfi_strides s1, vfi_strides s2, vfi_strides sc,
                                       vfi_stream_t stream);
int vfi_mindepthflowprojection_backward(const float* input1, const float* input2,
                                        const float* count, const float* gradoutput,
                                        float* gradinput1,
                                        int batch, int h, int w,
                                        vfi_strides s1, vfi_strides s2, vfi_strides sc,
                                        vfi_stream_t stream);

/* ---- interpolation_cuda / interpolationch_cuda -------------------------------
 * replaces Interpolation[Ch]Layer_gpu_forward / _backward (interpolation_cuda.cc:10-60,
 * 63-121).  The C==3 restriction of `interpolation_cuda` lives in its shim. */
int vfi_interpolation_forward(const float* input1, const float* input2, float* output,
                              int batch, int channel, int h, int w,
                              vfi_strides s1, vfi_strides s2,
                              vfi_stream_t stream);
int vfi_interpolation_backward(const float* input1, const float* input2, const float* gradoutput,
                               float* gradinput1, float* gradinput2,
                               int batch, int channel, int h, int w,
                               vfi_strides s1, vfi_strides s2,
                               vfi_stream_t stream);

/* ---- separableconv_cuda ------------------------------------------------------
 * replaces SeparableConvLayer_gpu_forward / _backward (separableconv_cuda.cc:10-87, 88-174).
 * h, w are input1's; input2/input3/output are [B, fs | C, h-fs+1, w-fs+1]. */
int vfi_separableconv_forward(const float* input1, const float* input2, const float* input3,
                              float* output,
                              int batch, int channel, int h, int w, int filter_size,
                              vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides so,
                              vfi_stream_t stream);
int vfi_separableconv_backward(const float* input1, const float* input2, const float* input3,
                               const float* gradoutput,
                               float* gradinput1, float* gradinput2, float* gradinput3,
                               int batch, int channel, int h, int w, int filter_size,
                               vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides so,
                               vfi_stream_t stream);

/* ---- separableconvflow_cuda --------------------------------------------------
 * replaces SeparableConvFlowLayer_gpu_forward / _backward (separableconvflow_cuda.cc:9-102,
 * 103-199).  input1 is only shape-checked by the reference and is not passed. */
int vfi_separableconvflow_forward(const float* input2, const float* input3, float* flow_output,
                                  int batch, int h, int w, int filter_size,
                                  vfi_strides s2, vfi_strides s3, vfi_strides so,
                                  vfi_stream_t stream);
int vfi_separableconvflow_backward(const float* input2, const float* input3,
                                   const float* gradflow_output,
                                   float* gradinput2, float* gradinput3,
                                   int batch, int h, int w, int filter_size,
                                   vfi_strides s2, vfi_strides s3, vfi_strides so,
                                   vfi_stream_t stream);

/* ---- correlation_cuda --------------------------------------------------------
 * replaces correlation_cuda.forward / .backward (correlation_cuda.cc:8-85, 87-165).
 * Inputs and outputs are DENSE NCHW (the reference kernels ignore strides).
 * The padded NHWC repack buffers rInput1/rInput2 of the reference are not
 * needed by these kernels; the shim still resizes and zero-fills them so a
 * caller that inspects them sees the reference's shapes.
 * vfi_correlation_output_dims reproduces correlation_cuda.cc:23-36. */
int vfi_correlation_output_dims(int h, int w, int pad_size, int kernel_size, int max_displacement,
                                int stride1, int stride2,
                                int* out_channels, int* out_h, int* out_w);
int vfi_correlation_forward(const float* input1, const float* input2, float* output,
                            int batch, int channel, int h, int w,
                            int pad_size, int kernel_size, int max_displacement,
                            int stride1, int stride2,
                            vfi_stream_t stream);
/* Two forward calls of equal shape in ONE launch: the same pyramid level of the two flow networks a frame pair runs,
 * (I0, I1) and (I1, I0) (networks/DAIN.py:196-202; PWCNet/PWCNet.py:230-300 calls the layer once per level).  At the coarse
 * levels a launch is pure latency (13-18 us for 1 MB at 1080p) and two cost what one does.  Results: the two
 * vfi_correlation_forward calls', bit for bit.  (Callers that batch the two orders along dim 0 need nothing new: batch = 2.) */
int vfi_correlation_forward_pair(const float* input1_a, const float* input2_a, float* output_a,
                                 const float* input1_b, const float* input2_b, float* output_b,
                                 int batch, int channel, int h, int w,
                                 int pad_size, int kernel_size, int max_displacement,
                                 int stride1, int stride2,
                                 vfi_stream_t stream);
/* The reference's at::Half instantiation of the forward (correlation_cuda_kernel.cu:386, 403): inputs and output
 * IEEE half, each product rounded to half, float accumulation, mean rounded to half once. */
int vfi_correlation_forward_f16(const void* input1_half, const void* input2_half, void* output_half,
                                int batch, int channel, int h, int w,
                                int pad_size, int kernel_size, int max_displacement,
                                int stride1, int stride2,
                                vfi_stream_t stream);
int vfi_correlation_backward(const float* input1, const float* input2, const float* gradoutput,
                             float* gradinput1, float* gradinput2,
                             int batch, int channel, int h, int w,
                             int pad_size, int kernel_size, int max_displacement,
                             int stride1, int stride2,
                             vfi_stream_t stream);
/* The backward of vfi_correlation_forward_pair: two vfi_correlation_backward calls of equal shape -- items a and b, the
 * same pyramid level of a frame pair's two flow networks -- with any subset of their four gradients.
 *   Layout: contiguous NCHW float32, as the other correlation entries; `batch` is per item.
 *   Result: every requested gradient equals the same-named output of vfi_correlation_backward on that item bit for bit
 *     (the reference's order: 32 partial sums over tc = l, l+32, ..., then the partials added in sequence).
 *   Every requested gradient is WRITTEN in full; the caller does not zero it.
 *   Any of the four gradinput* may be NULL: it is not computed, and no workgroup is launched for it.  An item with both
 *     outputs NULL may have NULL gradoutput and NULL inputs; otherwise its input1, input2 and gradoutput must all be
 *     non-NULL.  All four outputs NULL (and a valid shape): VFI_OK, nothing launched.
 *   Inputs may alias each other (at the top level (input1_b, input2_b) is often (input2_a, input1_a)).  Two equal non-NULL
 *     output pointers return VFI_ERR_SHAPE, as vfi_correlation_forward_pair refuses output_a == output_b.
 *   stride1 != 1 returns VFI_ERR_SHAPE, and so does everything else vfi_correlation_backward refuses (a shape that is
 *     not positive, invalid parameters, no output pixel).  Every check runs before the first launch.
 *   PWC-Net's configuration (pad 4, kernel 1, max displacement 4, strides 1): ONE launch for all requested gradients,
 *     unless gradients x batch x channel groups exceeds a grid's z (65535).  Then, and for any other configuration, one
 *     launch per requested gradient -- the same bits.
 *   Nothing is allocated and no workspace is used: the call is legal inside a stream capture.  float32 (the bfloat16 twin:
 *     vfi_correlation_backward_pair_bf16, further down). */
int vfi_correlation_backward_pair(const float* input1_a, const float* input2_a, const float* gradoutput_a,
                                  float* gradinput1_a, float* gradinput2_a,
                                  const float* input1_b, const float* input2_b, const float* gradoutput_b,
                                  float* gradinput1_b, float* gradinput2_b,
                                  int batch, int channel, int h, int w,
                                  int pad_size, int kernel_size, int max_displacement,
                                  int stride1, int stride2,
                                  vfi_stream_t stream);
/* ---- the correlation with PWC-Net's LeakyReLU fused in (PWCNet/PWCNet.py:230-301: every `self.corr(...)` is followed by
 * `self.leakyRELU(corr)` and a `torch.cat((corr, ...), 1)`).  float32 (the bfloat16 twins of all four: further down).  Each entry is its unactivated twin with the
 * same argument checks, the same kernels and the same kernel choice, plus:
 *   forward:  y = v > 0 ? v : v * negative_slope applied to every mean v as it is stored -- one float multiplication, the
 *     bits of torch.nn.functional.leaky_relu on the twin's output (NaN stays NaN, -0 becomes -0 * negative_slope).
 *   backward: every gradOutput value g at output position p becomes g' = y[p] > 0 ? g : g * negative_slope as it is
 *     loaded, y the SAVED ACTIVATED OUTPUT (its sign is the pre-activation's for any slope > 0); g' is rounded to float
 *     before it is used, so each gradient equals the twin's fed g', bit for bit.
 *   negative_slope must be finite and > 0: anything else returns VFI_ERR_SHAPE, in all four entries.
 *   *_batch_stride: the distance in ELEMENTS between two images of that tensor.  The 81 (out_channels) planes of an image
 *     stay contiguous, so `output` may be the first channels of a preallocated concatenation buffer, and `gradoutput` the
 *     narrow() view that torch.cat's backward hands down.  A stride below out_channels * out_h * out_w returns
 *     VFI_ERR_SHAPE.  An output stride that breaks the 16- or 8-byte alignment of a kernel's stores selects the kernel a
 *     misaligned output pointer would select; the result does not depend on it.
 *   The pair entries are ONE launch for both items (forward) and for every requested gradient (backward: NULL gradients
 *     are skipped, an item with both gradients NULL may be all NULL), exactly as vfi_correlation_backward_pair. */
int vfi_correlation_lrelu_forward(const float* input1, const float* input2, float* output, int64_t output_batch_stride,
                                  int batch, int channel, int h, int w,
                                  int pad_size, int kernel_size, int max_displacement,
                                  int stride1, int stride2, float negative_slope,
                                  vfi_stream_t stream);
int vfi_correlation_lrelu_forward_pair(const float* input1_a, const float* input2_a, float* output_a, int64_t output_a_batch_stride,
                                       const float* input1_b, const float* input2_b, float* output_b, int64_t output_b_batch_stride,
                                       int batch, int channel, int h, int w,
                                       int pad_size, int kernel_size, int max_displacement,
                                       int stride1, int stride2, float negative_slope,
                                       vfi_stream_t stream);
int vfi_correlation_lrelu_backward(const float* input1, const float* input2, const float* y, int64_t y_batch_stride,
                                   const float* gradoutput, int64_t gradoutput_batch_stride,
                                   float* gradinput1, float* gradinput2,
                                   int batch, int channel, int h, int w,
                                   int pad_size, int kernel_size, int max_displacement,
                                   int stride1, int stride2, float negative_slope,
                                   vfi_stream_t stream);
int vfi_correlation_lrelu_backward_pair(const float* input1_a, const float* input2_a, const float* y_a, int64_t y_a_batch_stride,
                                        const float* gradoutput_a, int64_t gradoutput_a_batch_stride,
                                        float* gradinput1_a, float* gradinput2_a,
                                        const float* input1_b, const float* input2_b, const float* y_b, int64_t y_b_batch_stride,
                                        const float* gradoutput_b, int64_t gradoutput_b_batch_stride,
                                        float* gradinput1_b, float* gradinput2_b,
                                        int batch, int channel, int h, int w,
                                        int pad_size, int kernel_size, int max_displacement,
                                        int stride1, int stride2, float negative_slope,
                                        vfi_stream_t stream);
/* The reference's at::Half instantiation of the backward (correlation_cuda_kernel.cu:151-334, dispatched at :495-541):
 * all five tensors IEEE half, dense NCHW, stride1 == 1 as for vfi_correlation_backward (same terms, windows and skips).
 * at::Half arithmetic rounds to half after every operation: each term p = half(gradOutput * value); 32 partials
 * s_l (l = 0..31, over tc = l, l+32, ...; for k > 1 the window rows outer, columns inner) accumulate IN HALF,
 * s_l = half(s_l + p); then r = half(r + s_l) in order of l; gradInput = half(r / half(k*k*C)) -- the count itself
 * rounded to half.  A term whose other-map tap lies in the zero padding is not skipped (it adds half(g * 0)).  Every
 * element of both gradients is written (the positions the reference never visits as +0), so they need no zero fill;
 * nothing is allocated: the call can be captured in a graph. */
int vfi_correlation_backward_f16(const void* input1, const void* input2, const void* gradoutput,
                                 void* gradinput1, void* gradinput2,
                                 int batch, int channel, int h, int w,
                                 int pad_size, int kernel_size, int max_displacement,
                                 int stride1, int stride2,
                                 vfi_stream_t stream);

/* The cost volume on bfloat16 tensors -- the mixed-precision dtype of torch.autocast(dtype=torch.bfloat16).  All
 * tensors dense NCHW bfloat16 at any 2-byte-aligned address; the argument checks of the _f16 entries (the backward
 * refuses stride1 != 1).  Nothing is allocated, no workspace, no atomics: the calls are legal inside a stream capture,
 * every output element is written, nothing else is touched, and the same inputs give the same bits run after run.
 *
 * Forward:  out = bf16_rne( (sum over the k x k window and the C channels of x1 * x2) / (float)(k*k*C) ).
 * Every product is exact in float32 (two 8-bit significands); the sum is accumulated in float32; the mean is rounded to
 * bfloat16 once, to nearest even.  A tap of the second map that lies in the zero padding is a product with +0 and is
 * not skipped: inf * 0 is NaN there, as in the reference's physically padded rInput2.
 *   - PWC-Net's configuration (kernel 1, strides 1, max displacement 4, any pad) from a tile count on:
 *     the matrix cores, v_mfma_f32_16x16x32_bf16 over 32 channels per instruction.  The order of the float32 additions
 *     inside an instruction is the hardware's, so the result is within
 *         2^-8 |R| + (1 + 2^-8) (n + 2) 2^-23 A,   n = k*k*C, R the exact mean, A the same mean over |x1 * x2|,
 *     of R, not a fixed bit pattern of a float32 chain.  Channel positions the kernel pads up to its K step of 32 hold
 *     zero in BOTH operands.  bfloat16 SUBNORMAL inputs: the MFMA keeps them (measured on an MI355X, not taken from the
 *     instruction set document: tools/bench_corr_bf16.py); no test depends on it.
 *   - every other configuration, and PWC-Net levels below that tile count: one thread per output, bit for bit
 *     bf16_rne(vfi_correlation_forward(float(x1), float(x2))) -- the float32 kernel's arithmetic in the same order.
 *
 * Backward: storage bfloat16, arithmetic that of vfi_correlation_backward term by term on the widened values (float32
 * products, 32 partials over tc = l, l+32, ..., partials added in sequence, divided by (float)(k*k*C)), rounded to
 * bfloat16 once: bit for bit bf16_rne(vfi_correlation_backward(float(x1), float(x2), float(g))), NaN positions
 * included. */
int vfi_correlation_forward_bf16(const void* input1, const void* input2, void* output,
                                 int batch, int channel, int h, int w,
                                 int pad_size, int kernel_size, int max_displacement,
                                 int stride1, int stride2,
                                 vfi_stream_t stream);
int vfi_correlation_backward_bf16(const void* input1, const void* input2, const void* gradoutput,
                                  void* gradinput1, void* gradinput2,
                                  int batch, int channel, int h, int w,
                                  int pad_size, int kernel_size, int max_displacement,
                                  int stride1, int stride2,
                                  vfi_stream_t stream);

/* The bfloat16 cost volume with PWC-Net's LeakyReLU fused in: vfi_correlation_forward_bf16 / _backward_bf16 with the same
 * argument checks, the same kernels, the same kernel choice, plus the rules of the float32 lrelu entries above for
 * negative_slope (finite and > 0, else VFI_ERR_SHAPE) and the batch strides (in ELEMENTS, the 81 planes of an image
 * contiguous, a stride below out_channels * out_h * out_w is VFI_ERR_SHAPE).  No workspace, no atomics.
 *   forward:  the bits of the composition it replaces, torch's leaky_relu on the bfloat16 cost volume: the mean is rounded
 *     to bfloat16 FIRST; a value that is not positive is then multiplied by negative_slope in float32 and rounded again.
 *     (One rounding of lrelu(mean) would differ from the unfused network in the last bit, and where a tiny positive mean
 *     rounds to +0 the backward's mask -- the sign of the saved y -- would differ too.)  An output_batch_stride that is odd
 *     puts every other image on a 2-byte boundary: the stores test their alignment one by one.
 *   backward: every gradOutput value g becomes g' = y > 0 ? g : bf16_rne(float(g) * negative_slope) as it is loaded, in both
 *     kernels and for both gradients; the result is vfi_correlation_backward_bf16 fed a materialised bfloat16 g', bit for
 *     bit -- what torch autograd gives through leaky_relu on bfloat16.  y and gradoutput are read where they lie. */
int vfi_correlation_lrelu_forward_bf16(const void* input1, const void* input2, void* output, int64_t output_batch_stride,
                                       int batch, int channel, int h, int w,
                                       int pad_size, int kernel_size, int max_displacement,
                                       int stride1, int stride2, float negative_slope,
                                       vfi_stream_t stream);
int vfi_correlation_lrelu_backward_bf16(const void* input1, const void* input2, const void* y, int64_t y_batch_stride,
                                        const void* gradoutput, int64_t gradoutput_batch_stride,
                                        void* gradinput1, void* gradinput2,
                                        int batch, int channel, int h, int w,
                                        int pad_size, int kernel_size, int max_displacement,
                                        int stride1, int stride2, float negative_slope,
                                        vfi_stream_t stream);

/* The pair entries on bfloat16 tensors: two calls of equal shape -- items a and b, the same pyramid level of a frame pair's
 * two flow networks -- in ONE launch (forward), and any subset of their four gradients in ONE launch (backward).  The
 * contract is the union of the float32 pair entries' above and of the bfloat16 single entries':
 *   Layout: dense NCHW bfloat16 at any 2-byte-aligned address; `batch` is per item.  The lrelu entries take batch strides
 *     in ELEMENTS (the 81 planes of an image contiguous); an odd stride is legal, the stores test their alignment one by one.
 *   Result: every output equals the same-named output of the single bfloat16 entry on that item (vfi_correlation_forward_bf16,
 *     vfi_correlation_lrelu_forward_bf16, vfi_correlation_backward_bf16, vfi_correlation_lrelu_backward_bf16) bit for bit, NaN
 *     positions included, for every shape.  The forward kernel is therefore chosen as the single entry chooses it, on ONE
 *     item's batch, h and w -- not on the pair's tile count, as the float32 pair does: the matrix-core kernel's float32
 *     addition order is the hardware's and is not the one-thread-per-output kernel's chain.
 *   Every requested output is WRITTEN in full; nothing else is touched.  Nothing is allocated, no workspace, no atomics:
 *     the calls are legal inside a stream capture.
 *   Backward: any of the four gradinput* may be NULL: it is not computed and no workgroup is launched for it.  An item with
 *     both gradients NULL may be all NULL; otherwise its input1, input2, gradoutput (and y) must be non-NULL.  All four
 *     NULL with a valid shape: VFI_OK, nothing launched.
 *   Inputs may alias each other (at the top level item b is often item a swapped).  Two equal non-NULL outputs return
 *     VFI_ERR_SHAPE.  So do, all before the first launch: a negative_slope that is not finite and > 0, a batch stride below
 *     out_channels * out_h * out_w, stride1 != 1 in the backward, a shape that is not positive, a NULL tensor of an item
 *     that needs it (a missing y included), invalid parameters, no output pixel.
 *   Launches.  Forward: one, unless 2 * batch exceeds a grid's z (65535) where the matrix-core kernel is chosen; then one
 *     per item.  Backward, PWC-Net's configuration (pad 4, kernel 1, max displacement 4, strides 1): one, unless gradients x
 *     batch x channel groups exceeds 65535; then, and for any other configuration, one per requested gradient.  The bits
 *     do not depend on it. */
int vfi_correlation_forward_pair_bf16(const void* input1_a, const void* input2_a, void* output_a,
                                      const void* input1_b, const void* input2_b, void* output_b,
                                      int batch, int channel, int h, int w,
                                      int pad_size, int kernel_size, int max_displacement,
                                      int stride1, int stride2,
                                      vfi_stream_t stream);
int vfi_correlation_lrelu_forward_pair_bf16(const void* input1_a, const void* input2_a, void* output_a, int64_t output_a_batch_stride,
                                            const void* input1_b, const void* input2_b, void* output_b, int64_t output_b_batch_stride,
                                            int batch, int channel, int h, int w,
                                            int pad_size, int kernel_size, int max_displacement,
                                            int stride1, int stride2, float negative_slope,
                                            vfi_stream_t stream);
int vfi_correlation_backward_pair_bf16(const void* input1_a, const void* input2_a, const void* gradoutput_a,
                                       void* gradinput1_a, void* gradinput2_a,
                                       const void* input1_b, const void* input2_b, const void* gradoutput_b,
                                       void* gradinput1_b, void* gradinput2_b,
                                       int batch, int channel, int h, int w,
                                       int pad_size, int kernel_size, int max_displacement,
                                       int stride1, int stride2,
                                       vfi_stream_t stream);
int vfi_correlation_lrelu_backward_pair_bf16(const void* input1_a, const void* input2_a, const void* y_a, int64_t y_a_batch_stride,
                                             const void* gradoutput_a, int64_t gradoutput_a_batch_stride,
                                             void* gradinput1_a, void* gradinput2_a,
                                             const void* input1_b, const void* input2_b, const void* y_b, int64_t y_b_batch_stride,
                                             const void* gradoutput_b, int64_t gradoutput_b_batch_stride,
                                             void* gradinput1_b, void* gradinput2_b,
                                             int batch, int channel, int h, int w,
                                             int pad_size, int kernel_size, int max_displacement,
                                             int stride1, int stride2, float negative_slope,
                                             vfi_stream_t stream);

/* ==== glue either side of the ops above: the reference does these with torch
 * built-ins and Python; here each is one launch.  No reference binding exists for them: the
 * host-side mirrors are <pkg>/fused.py. ========================================================= */

/* forward_flownets (networks/DAIN_slowmotion.py:204-216, DAIN.py:296-311):
 * output[B,C,4hq,4wq] = nn.Upsample(scale_factor=4, mode='bilinear')((mul0 * input) * mul1),
 * torch's align_corners=False rule.  mul0 = div_flow, mul1 = the time offset. */
int vfi_flow_upsample4(const float* input, float* output,
                       int batch, int channels, int hq, int wq, float mul0, float mul1,
                       vfi_strides sq, vfi_strides so,
                       vfi_stream_t stream);

/* forward_flownets + FlowProject in one call: the quarter-resolution flow [B,2,hq,wq] is upsampled
 * into a per-stream scratch tensor of the library and projected; count [B,1,4hq,4wq] and output
 * [B,2,4hq,4wq] as vfi_flowprojection_forward.  Results equal vfi_flow_upsample4 followed by
 * vfi_[depth]flowprojection_forward bit for bit (it is those two steps without a caller-side
 * tensor). */
int vfi_flowprojection_forward_up4(const float* flow_q, float* count, float* output,
                                   int batch, int hq, int wq, float mul0, float mul1, int fillhole,
                                   vfi_strides sq, vfi_strides sc, vfi_strides so,
                                   vfi_stream_t stream);
int vfi_depthflowprojection_forward_up4(const float* flow_q, const float* input2,
                                        float* count, float* output,
                                        int batch, int hq, int wq, float mul0, float mul1, int fillhole,
                                        vfi_strides sq, vfi_strides s2, vfi_strides sc, vfi_strides so,
                                        vfi_stream_t stream);

/* ---- training through the quarter-resolution flow: the backwards of the three entry points above, each for a LIST
 * of 1 <= nitems <= 8 time offsets of ONE quarter-resolution tensor (the gradients of all of them land on it).
 * Table arguments (`[]` below) are HOST arrays of nitems device pointers, mul1 a HOST array of nitems floats; items
 * share shape and strides.  grad_q is WRITTEN, every element once: no zero fill, no accumulation, no atomics, so the
 * results are reproducible bit for bit.  Nothing is allocated: the calls can be captured in a graph (the tables travel
 * by value in the kernel arguments).  Null pointers, nitems outside 1..8, sizes or strides beyond 32-bit in-plane
 * offsets: VFI_ERR_SHAPE before any launch.
 *
 * vfi_flow_upsample4_backward: grad_q[B,C,hq,wq] = sum_i m_i * U^T grad_full[i], U the x4 bilinear upsample of
 * vfi_flow_upsample4, m_i = mul0 * mul1[i] (one fp32 product).  A quarter pixel q of an axis collects from the
 * full-resolution pixels d = 4q-2 .. 4q+5 cut to the image, with weight (i0 == q ? l0 : 0) + (i1 == q ? l1 : 0) of d's
 * two taps.  Per item: rows ascending, inside a row columns ascending, r = fmaf(wx, G, r), then s = fmaf(wy, r, s);
 * items in order, acc = fmaf(m_i, s_i, acc) (csrc/flow_up4.h: up4_adjoint).  grad_full[i]: [B,C,4hq,4wq], strides sg. */
int vfi_flow_upsample4_backward(const float* const* grad_full, const float* mul1, int nitems,
                                float* grad_q,
                                int batch, int channels, int hq, int wq, float mul0,
                                vfi_strides sg, vfi_strides sq,
                                vfi_stream_t stream);
/* Backward of vfi_flowprojection_forward_up4 for item i = (mul0, mul1[i]): counts[i] [B,1,4hq,4wq] is what that
 * forward wrote, gradoutputs[i] [B,2,4hq,4wq] the gradient of its output.  grad_q [B,2,hq,wq] equals, bit for bit,
 * vfi_flow_upsample4 -> vfi_flowprojection_backward into a zero-filled gradient (per item) ->
 * vfi_flow_upsample4_backward; the full-resolution flow and its gradient exist per tile in LDS only.  fillhole plays
 * no part, as in vfi_flowprojection_backward.  sq: flow_q, sc: counts, so: gradoutputs, sgq: grad_q. */
int vfi_flowprojection_backward_up4(const float* flow_q, const float* const* counts,
                                    const float* const* gradoutputs, const float* mul1, int nitems,
                                    float* grad_q,
                                    int batch, int hq, int wq, float mul0,
                                    vfi_strides sq, vfi_strides sc, vfi_strides so, vfi_strides sgq,
                                    vfi_stream_t stream);
/* The same for vfi_depthflowprojection_forward_up4: depths[i] (items may share one) and the forward's outputs[i] are
 * needed as in vfi_depthflowprojection_backward.  grad_depths (the table, or any entry) may be NULL = not wanted;
 * a given grad_depths[i] [B,1,4hq,4wq] is WRITTEN in full with item i's depth gradient, equal bit for bit to what
 * vfi_depthflowprojection_backward adds into zeros (a caller whose items share a depth sums them).  s2: depths and
 * grad_depths, so: outputs and gradoutputs. */
int vfi_depthflowprojection_backward_up4(const float* flow_q, const float* const* depths,
                                         const float* const* counts, const float* const* outputs,
                                         const float* const* gradoutputs, const float* mul1, int nitems,
                                         float* grad_q, float* const* grad_depths,
                                         int batch, int hq, int wq, float mul0,
                                         vfi_strides sq, vfi_strides s2, vfi_strides sc, vfi_strides so,
                                         vfi_strides sgq,
                                         vfi_stream_t stream);

/* FilterInterpolate (networks/DAIN_slowmotion.py:324-335, DAIN.py:560-573): out0 = A1(ref0, flow0,
 * filt0), out2 = A1(ref2, flow2, filt2), blend = out0 * w0 + out2 * w2 (products rounded
 * separately, as torch's three elementwise ops).  out0 / out2 may be NULL.  ref0/ref2, flow0/flow2
 * and filt0/filt2 share strides pairwise; blend/out0/out2 share s_out, which may be any layout with w
 * stride 1 (the three may be channel slices of one wider buffer).  filter_channels == 16 with both
 * out0 and out2 given and s_out.h == s_ref.h runs the LDS-staged kernels, anything else the per-pixel
 * gather: the same bits either way. */
int vfi_filterinterp_blend_forward(const float* ref0, const float* ref2,
                                   const float* flow0, const float* flow2,
                                   const float* filt0, const float* filt2,
                                   float* blend, float* out0, float* out2,
                                   int batch, int channel, int h, int w, int filter_channels,
                                   float w0, float w2,
                                   vfi_strides s_ref, vfi_strides s_flow, vfi_strides s_filt, vfi_strides s_out,
                                   vfi_stream_t stream);

/* Backward of vfi_filterinterp_blend_forward (training DAIN through the fused synthesis).
 * - Per direction d (0: ref0 / flow0 / filt0 / w0, 2: the same with 2) the incoming gradient is
 *   g_d = grad_blend * w_d + grad_out_d, the product and the sum rounded separately: what torch
 *   autograd accumulates for out_d when blend = out0 * w0 + out2 * w2 and out_d has another use.
 *   It is formed in registers, never stored.  A NULL grad_blend / grad_out_d is an absent term; a
 *   direction with both terms NULL has zero gradients.
 * - Every requested gradient equals, bit for bit, vfi_filterinterp_backward_ori(ref_d, flow_d,
 *   filt_d, g_d) run on zero-filled outputs with g_d materialised; the image gradient's fixed-point
 *   scale comes from a max-scan over g_d formed the same way.  Non-finite g_d or filters scatter
 *   the image gradient with fp32 atomics as that entry does (same NaN / Inf pattern).
 * - Any of the six gradient outputs may be NULL and is then not computed (with both grad_ref NULL
 *   there is no image-gradient work at all).  Requested outputs are written in full: the caller
 *   does not zero them.  All six NULL: VFI_OK, nothing launched.
 * - ref0/ref2 and grad_ref0/grad_ref2 use s_ref, flows and their gradients s_flow, filters and
 *   their gradients s_filt, grad_blend/grad_out0/grad_out2 s_grad.
 * - Any filter_channels the forward accepts; 16 (fs = 4) is the LDS-staged path.  Both directions
 *   run in the same launches; results are reproducible bit for bit. */
int vfi_filterinterp_blend_backward(const float* ref0, const float* ref2,
                                    const float* flow0, const float* flow2,
                                    const float* filt0, const float* filt2,
                                    const float* grad_blend, const float* grad_out0, const float* grad_out2,
                                    float* grad_ref0, float* grad_ref2,
                                    float* grad_flow0, float* grad_flow2,
                                    float* grad_filt0, float* grad_filt2,
                                    int batch, int channel, int h, int w, int filter_channels, float w0, float w2,
                                    vfi_strides s_ref, vfi_strides s_flow, vfi_strides s_filt, vfi_strides s_grad,
                                    vfi_stream_t stream);

/* The "head" of rectifyNet's input on bfloat16 storage, for a network under bfloat16 autocast: one launch writes the
 * 3 * channel + 4 + 2 * filter_channels consecutive channels blend, out0, out2, flow0, flow2, filt0, filt2 (the order of the
 * reference's torch.cat, networks/DAIN_slowmotion.py:177-181; 45 channels at channel = 3, filter_channels = 16) of head_bf16,
 * a bfloat16 tensor with strides s_head in bfloat16 elements -- typically the first channels of the network's wider input,
 * whose context channels vfi_filterinterp_forward_ori_multi_to_bf16 fills -- and, where blend_f32 is not NULL, the blend as
 * float32 with strides s_blend.  All inputs are float32, with the meaning and the pairwise shared strides of
 * vfi_filterinterp_blend_forward.
 * Bits: with blend, out0, out2 the float32 values vfi_filterinterp_blend_forward writes for the same inputs, blend_f32 is
 * that blend, and the head holds bf16_rne (round to nearest even, once) of blend, out0, out2 and of every flow and filter
 * value.  The blend is formed from the UNROUNDED out0 and out2, its two products rounded separately and not contracted:
 * both sides' values of a pixel are in registers when it is formed, nothing is read back.  So the head equals, bit for bit,
 * torch.cat((blend, out0, out2, flow0, flow2, filt0, filt2), 1).to(torch.bfloat16); NaN stays NaN at the same positions
 * (payloads are not specified); an invalid pixel copies the frame's value through, rounded.
 * Layouts: w stride 1 everywhere; s_head.h == s_ref.h (else VFI_ERR_SHAPE: the rule of the entry that fills the rest of the
 * buffer), s_head.b and s_head.c free; head_bf16 needs 2-byte alignment only.  A lane owns two horizontally adjacent pixels:
 * where every row of the flows, the filters and blend_f32 starts 8-byte aligned and every row of the head 4-byte aligned
 * (even strides, aligned bases) they are read and written as pairs, otherwise element by element, with the same bits.
 * Any filter_channels vfi_filterinterp_blend_forward accepts, any channel >= 1, batch <= 65535.  The destinations must not
 * overlap the inputs or each other (not checked).  Every argument is checked before the launch. */
int vfi_rectify_head_forward_bf16(const float* ref0, const float* ref2,
                                  const float* flow0, const float* flow2,
                                  const float* filt0, const float* filt2,
                                  void* head_bf16, float* blend_f32,
                                  int batch, int channel, int h, int w, int filter_channels,
                                  float w0, float w2,
                                  vfi_strides s_ref, vfi_strides s_flow, vfi_strides s_filt, vfi_strides s_head,
                                  vfi_strides s_blend,
                                  vfi_stream_t stream);

/* PWCDCNet.warp (PWCNet/PWCNet.py:159-199): output = grid_sample(x, grid(flow)) * mask, mask = 1
 * where grid_sample(ones, grid) >= 0.9999 else 0; bilinear, zeros padding.  align_corners: 1 = the
 * grid_sample of torch <= 1.2 the reference was written for, 0 = the default of torch >= 1.3. */
int vfi_pwc_warp_forward(const float* x, const float* flow, float* output,
                         int batch, int channel, int h, int w, int align_corners,
                         vfi_strides sx, vfi_strides sf, vfi_strides so,
                         vfi_stream_t stream);

/* Backward of PWCDCNet.warp: the gradients torch autograd gives for the reference's warp() in the same
 * align_corners mode.  The mask is a constant (its two index assignments overwrite every element); the
 * sample is ATen's bilinear grid_sampler_2d with zero padding, so a corner outside the map counts 0 in
 * both gradients (a sample on the last column / row gets a one-sided derivative).  With gm = grad_output
 * x mask: grad_x[c, corner] += gm x weight for the in-bounds corners, summed as 64-bit fixed-point
 * integers (DESIGN.md "Deterministic image gradients"; fp32 atomics where grad_output holds a NaN / Inf or
 * magnitudes that could overflow); grad_x is ADDED INTO, the caller zero-fills it, as for
 * vfi_interpolation_backward.  grad_flow is WRITTEN: per pixel the channel sum of gm x d(sample)/d(ix, iy)
 * in a fixed order, times grid_sample's un-normalisation ((W-1)/2 aligned, W/2 not) and the reference's
 * 2 / max(W-1, 1); a pixel with mask 0 gets 0 for finite inputs.  Either gradient may be NULL (not
 * computed; the other one is bit-identical).  Both are bit-reproducible.  Any batch / channel / row
 * strides, w stride 1 for every tensor.  May allocate library scratch on its first call per stream. */
int vfi_pwc_warp_backward(const float* x, const float* flow, const float* grad_output,
                          float* grad_x, float* grad_flow,
                          int batch, int channel, int h, int w, int align_corners,
                          vfi_strides sx, vfi_strides sf, vfi_strides sgo, vfi_strides sgx, vfi_strides sgf,
                          vfi_stream_t stream);

/* PWCDCNet.warp on bfloat16 storage.  x, output, grad_output and grad_x are bfloat16; flow is float32, or bfloat16 when
 * flow_is_bf16 != 0, and grad_flow has the flow's dtype.  Strides in elements with the float32 entries' rules (any batch /
 * channel / row stride, w stride 1); any 2-byte-aligned address.  Values are widened on load (exact), the arithmetic is the
 * float32 entries' in their order, and a result is rounded to bfloat16 once, to nearest even.
 *   forward:  bit for bit bf16_rne(vfi_pwc_warp_forward(float(x), float(flow))).
 *   backward: grad_x is WRITTEN in full, not added into (adding into bfloat16 would round twice): bf16_rne of what
 *     vfi_pwc_warp_backward leaves in a zero-filled grad_x for the widened tensors, from the same fixed-point accumulator
 *     (same scale, same addends, same integer sums, one conversion, one rounding).  grad_flow is WRITTEN: the float32
 *     entry's ordered channel sum, rounded once where the flow is bfloat16.  Either gradient may be NULL (the other one is
 *     bit-identical); both are bit-reproducible.  A call the accumulator sends to fp32 atomics (a NaN / Inf in grad_output,
 *     or magnitudes that could overflow) adds in float32 library scratch and rounds once at the end -- NaN / Inf land in the
 *     cells they poison in the float32 entry; no atomic touches bfloat16 storage.
 * May allocate library scratch on its first call per stream (the backward). */
int vfi_pwc_warp_forward_bf16(const void* x, const void* flow, int flow_is_bf16, void* output,
                              int batch, int channel, int h, int w, int align_corners,
                              vfi_strides sx, vfi_strides sf, vfi_strides so,
                              vfi_stream_t stream);
int vfi_pwc_warp_backward_bf16(const void* x, const void* flow, int flow_is_bf16, const void* grad_output,
                               void* grad_x, void* grad_flow,
                               int batch, int channel, int h, int w, int align_corners,
                               vfi_strides sx, vfi_strides sf, vfi_strides sgo, vfi_strides sgx, vfi_strides sgf,
                               vfi_stream_t stream);

/* PWCDCNet's warp feeding its correlation layer (PWCNet/PWCNet.py:244-247, 266-267, 282-283, 299-300):
 * output[B,81,h,w] = correlation(input1, warp(input2, flow)) with pad 4, kernel 1, max displacement 4, strides 1 --
 * vfi_pwc_warp_forward followed by vfi_correlation_forward, bit for bit, in one launch and without the warped
 * tensor.  input1 / input2 / output dense NCHW, flow [B,2,h,w] with strides sf. */
int vfi_pwc_warp_correlation_forward(const float* input1, const float* input2, const float* flow, float* output,
                                     int batch, int channel, int h, int w, int align_corners,
                                     vfi_strides sf, vfi_stream_t stream);

/* frame boundary (demo_MiddleBury.py:280-318, 350-364, 370-388).
 * u8 -> planar: dst[b,c,y,x] = src[b, clamp(y - pad_top), clamp(x - pad_left), c] / 255 for the padded
 * frame (h + pad_top + pad_bottom) x (w + pad_left + pad_right); src is dense [B,h,w,3] uint8.
 * planar -> u8: dst[b,y,x,c] = uint8(rint(255 * clip(src[b,c,top+y,left+x], 0, 1))), dst dense [B,h,w,3].
 * error sums: sums[0] += sum|a-b|, sums[1] += sum (a-b)^2 over n bytes (exact; caller zeroes sums).
 * ssim sums: sums[0] += sum of the SSIM map of every colour plane of every frame pair as the demo computes it
 *   (demo_MiddleBury.py:40-162, 382-388: planes / 255, 11-tap sigma-1.5 Gaussian along H then W without padding,
 *   data_range 1, K = (0.01, 0.03)), each value as a 2^-32 fixed-point integer (order-free; caller zeroes sums).
 *   mean SSIM = sums[0] / 2^32 / (batch * 3 * (h - 10) * (w - 10)); a dimension below 11 is not smoothed and
 *   contributes its full length instead of (length - 10), as in the reference.  a, b: dense [B,h,w,3] uint8. */
int vfi_frame_u8_to_planar(const unsigned char* src_hwc, float* dst,
                           int batch, int h, int w, int pad_left, int pad_right, int pad_top, int pad_bottom,
                           vfi_strides sd, vfi_stream_t stream);
int vfi_planar_to_frame_u8(const float* src, unsigned char* dst_hwc,
                           int batch, int h, int w, int top, int left,
                           vfi_strides ss, vfi_stream_t stream);
int vfi_frame_error_sums(const unsigned char* a, const unsigned char* b, int64_t n,
                         unsigned long long* sums, vfi_stream_t stream);
int vfi_frame_ssim_sums(const unsigned char* a, const unsigned char* b, int batch, int h, int w,
                        long long* sums, vfi_stream_t stream);

/* ==== training losses (loss_function.py: part_loss as train.py calls it) ========================================
 * The Charbonnier pixel loss of nd tensors, the gradient-adaptive total variation of a flow pair and the pair's
 * motion-symmetry loss, forward in one launch plus a small finish launch, backward in one launch.
 *
 *   x_i      = diffs[i]                       (target == NULL)
 *            = diffs[i] - target              (target given: diffs[i] is the network output; one fp32 rounding)
 *   e2       = (float)(epsilon * epsilon)     (the product in double)
 *   l_ib     = mean over [cd,h,w] of sqrt(x_i^2 + e2) of sample b          -> sample_means[i * batch + b]
 *   pixel_i  = mean over [batch,cd,h,w] of sqrt(x_i^2 + e2)                (neg_psnr == 0)
 *            = mean_b( -log(1 / l_ib) / 100 )                              (neg_psnr != 0)
 *   tv(f, I) = mean over b, y < h-1, x < w-1 of  w (T_0 + T_1),
 *              T_c = sqrt((f_c(y,x) - f_c(y+1,x))^2 + (f_c(y,x) - f_c(y,x+1))^2 + e2),
 *              w   = exp(-sum over the ci channels of (|I(y,x) - I(y+1,x)| + |I(y,x) - I(y,x+1)|))
 *   offset   = tv(flow0, img0) + tv(flow1, img1)                           (two fp32 means, one fp32 add)
 *   sym      = mean over [batch,2,h,w] of sqrt((flow0 + flow1)^2 + e2)
 *   values   = [pixel_0 .. pixel_{nd-1}, offset, sym]                      (nd + 2 floats on the device)
 *
 * Every term is formed in fp32, one rounding per operation (no contraction), and summed in double: per lane, then
 * per wave, then per workgroup; the workgroups' partial sums go to a per-stream scratch buffer of the library and the
 * finish launch adds them in a fixed order.  No floating-point atomics: results are reproducible bit for bit, and the
 * same for a strided view as for its dense copy (rows are read 16 bytes at a time where base, strides and w allow,
 * element by element otherwise; both give every lane the same elements in the same order).
 *
 * diffs: HOST array of 1 <= nd <= 8 device pointers, [batch,cd,h,w] each with strides sd; target (may be NULL) shares
 * sd.  flow0 / flow1: [batch,2,h,w], strides sf, both given or both NULL (then values[nd] = values[nd+1] = 0 and the
 * images are not read).  img0 / img1: [batch,ci,h,w], strides si, required with flows.  With flows h >= 2 and w >= 2
 * (the total variation's mean would be over nothing).  Null required pointers, nd outside 1..8, non-positive sizes:
 * VFI_ERR_SHAPE before any launch.  May allocate library scratch on its first call per stream. */
int vfi_part_loss_forward(const float* const* diffs, int nd, const float* target,
                          const float* flow0, const float* flow1,
                          const float* img0, const float* img1,
                          int batch, int cd, int ci, int h, int w,
                          double epsilon, int neg_psnr,
                          float* values, float* sample_means,
                          vfi_strides sd, vfi_strides sf, vfi_strides si,
                          vfi_stream_t stream);

/* Gradients of sum_j grad_values[j] * values[j] in ONE launch; grad_values is a DEVICE vector of nd + 2 floats (nothing
 * synchronises with the host).  loss_mask: bit j set = loss j takes part; a loss whose bit is clear is an absent term
 * (not a multiplication by zero).  grad_diffs: HOST array of nd device pointers, entries (or the table) may be NULL =
 * not wanted; grad_flow0 / grad_flow1 may be NULL.  Requested outputs are WRITTEN in full (zeros where every loss that
 * reaches them is masked out); nothing else is touched -- with only pixel bits set and the flow gradients NULL the
 * launch is one elementwise pass per requested diff and reads neither flows nor images.
 *   grad_diffs[i] = c * (x / sqrt(x^2 + e2)),  c = grad_values[i] / (float)(batch cd h w), or with neg_psnr
 *                   c_b = ((grad_values[i] / (float)(100 batch)) / sample_means[i * batch + b]) / (float)(cd h w);
 *                   with target it is the gradient of diffs[i], the network output (target gets none).
 *   grad_flow_s[c](y,x), terms added in this order into 0:
 *        + (k w(y,x))   * ((dy + dx) / T_c(y,x))                  own cell,        y < h-1 and x < w-1
 *        - (k w(y-1,x)) * (dy / T_c)  of the cell (y-1,x)         y >= 1 and x < w-1
 *        - (k w(y,x-1)) * (dx / T_c)  of the cell (y,x-1)         x >= 1 and y < h-1
 *        + ks * (u / sqrt(u^2 + e2)),  u = flow0 + flow1          symmetry
 *     k = grad_values[nd] / (float)(batch (h-1) (w-1)), ks = grad_values[nd+1] / (float)(batch 2 h w); divide and sqrt
 *     correctly rounded.  Images and target are data: no gradient.
 * sample_means: what the forward wrote (read with neg_psnr only).  sgd: strides of every grad_diffs[i], sgf: of the
 * flow gradients.  Nothing is allocated: the call can be captured in a graph. */
int vfi_part_loss_backward(const float* const* diffs, int nd, const float* target,
                           const float* flow0, const float* flow1,
                           const float* img0, const float* img1,
                           int batch, int cd, int ci, int h, int w,
                           double epsilon, int neg_psnr,
                           const float* grad_values, const float* sample_means, unsigned int loss_mask,
                           float* const* grad_diffs, float* grad_flow0, float* grad_flow1,
                           vfi_strides sd, vfi_strides sf, vfi_strides si, vfi_strides sgd, vfi_strides sgf,
                           vfi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VFI_HIP_H */
