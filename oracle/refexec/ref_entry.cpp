/* extern "C" entry points onto the reference's host launchers (`*_kernel` in `*_cuda_kernel.cu`), which are
 * called unchanged.  TEST INFRASTRUCTURE ONLY; CPU only.
 *
 * Every wrapper has one shape:   int vfi_ref_<launcher>(const int *ia, float *const *t, const int *const *s)
 *   ia  the launcher's integer arguments, in the launcher's order (listed per wrapper)
 *   t   the tensors' data pointers, in the launcher's order
 *   s   per tensor its four strides (batch, channel, height, width), in elements
 * The caller (ref_exec.py) passes the strides of its numpy arrays: for a contiguous NCHW array those are the
 * values `tensor.stride(0..3)` of the reference's `*_cuda.cc` wrappers (e.g. flowprojection_cuda.cc:26-34,
 * filterinterpolation_cuda.cc:39-57, separableconv_cuda.cc:32-50); for a view into a larger canvas they address
 * the frame inside the canvas.  What else the `.cc` wrappers do is done by the caller and cited there:
 * sizes and filter_size (filterinterpolation_cuda.cc:22-34, :395-396), nElement = 0 (flowprojection_cuda.cc:40),
 * zero-filled outputs and gradients (the `*Layer.py` files), the correlation's output dims, rInput buffers and
 * zero fills (correlation_cuda.cc:23-40, :97-113).
 */
#include "cuda_cpu_shim.h"

#include "filterinterpolation_cuda_kernel.cuh"
#include "flowprojection_cuda_kernel.cuh"
#include "depthflowprojection_cuda_kernel.cuh"
#include "mindepthflowprojection_cuda_kernel.cuh"
#include "interpolation_cuda_kernel.cuh"
#include "interpolationch_cuda_kernel.cuh"
#include "separableconv_cuda_kernel.cuh"
#include "separableconvflow_cuda_kernel.cuh"
#include "correlation_cuda_kernel.cuh"

#define S(k) s[k][0], s[k][1], s[k][2], s[k][3]
#define T(k) ten[k]
#define ENTRY(name, ntensors) \
    extern "C" int vfi_ref_##name(const int *ia, float *const *t, const int *const *s) { \
        at::Tensor ten[12]; \
        for (int i = 0; i < (ntensors); ++i) ten[i].ptr = t[i]; \
        const cudaStream_t stream = nullptr; \
        const int nElement = 0; /* "UNUSED" in every .cc wrapper */ \
        (void)s; (void)stream; (void)nElement;
#define END }

/* ---- FilterInterpolation.  ia = w, h, channel, batch, filter_size ---- */
/* tensors: input1 image, input2 flow, input3 filter, output (strides of input1, filterinterpolation_cuda.cc:67-68) */
ENTRY(FilterInterpolationLayer_gpu_forward_kernel_ori, 4)
    return FilterInterpolationLayer_gpu_forward_kernel_ori(stream, nElement, ia[0], ia[1], ia[2], ia[3], ia[4],
                                                           S(0), S(1), S(2), T(0), T(1), T(2), T(3));
END
/* image, flow, filter, gradoutput, gradinput1, gradinput2, gradinput3 */
ENTRY(FilterInterpolationLayer_gpu_backward_kernel_ori, 7)
    return FilterInterpolationLayer_gpu_backward_kernel_ori(stream, nElement, ia[0], ia[1], ia[2], ia[3], ia[4],
                                                            S(0), S(1), S(2), T(0), T(1), T(2), T(3), T(4), T(5), T(6));
END
/* image, flow, filter, offset, output */
ENTRY(FilterInterpolationLayer_gpu_forward_kernel, 5)
    return FilterInterpolationLayer_gpu_forward_kernel(stream, nElement, ia[0], ia[1], ia[2], ia[3], ia[4],
                                                       S(0), S(1), S(2), S(3), T(0), T(1), T(2), T(3), T(4));
END
/* image, flow, filter, offset, gradoutput, gradinput1..4 */
ENTRY(FilterInterpolationLayer_gpu_backward_kernel, 9)
    return FilterInterpolationLayer_gpu_backward_kernel(stream, nElement, ia[0], ia[1], ia[2], ia[3], ia[4],
                                                        S(0), S(1), S(2), S(3),
                                                        T(0), T(1), T(2), T(3), T(4), T(5), T(6), T(7), T(8));
END
ENTRY(FilterInterpolationLayer_gpu_forward_kernel_deforconv, 5)
    return FilterInterpolationLayer_gpu_forward_kernel_deforconv(stream, nElement, ia[0], ia[1], ia[2], ia[3], ia[4],
                                                                 S(0), S(1), S(2), S(3), T(0), T(1), T(2), T(3), T(4));
END
ENTRY(FilterInterpolationLayer_gpu_backward_kernel_deforconv, 9)
    return FilterInterpolationLayer_gpu_backward_kernel_deforconv(stream, nElement, ia[0], ia[1], ia[2], ia[3], ia[4],
                                                                  S(0), S(1), S(2), S(3),
                                                                  T(0), T(1), T(2), T(3), T(4), T(5), T(6), T(7), T(8));
END
/* image, flow, offset, output */
ENTRY(FilterInterpolationLayer_gpu_forward_kernel_nofilterwithdeforconv, 4)
    return FilterInterpolationLayer_gpu_forward_kernel_nofilterwithdeforconv(
        stream, nElement, ia[0], ia[1], ia[2], ia[3], ia[4], S(0), S(1), S(2), T(0), T(1), T(2), T(3));
END
/* image, flow, offset, gradoutput, gradinput1..3 */
ENTRY(FilterInterpolationLayer_gpu_backward_kernel_nofilterwithdeforconv, 7)
    return FilterInterpolationLayer_gpu_backward_kernel_nofilterwithdeforconv(
        stream, nElement, ia[0], ia[1], ia[2], ia[3], ia[4], S(0), S(1), S(2),
        T(0), T(1), T(2), T(3), T(4), T(5), T(6));
END

/* ---- projections.  forward ia = w, h, channel, batch, fillhole; backward ia = w, h, channel, batch ---- */
/* flow, count, output */
ENTRY(FlowProjection_gpu_forward_kernel, 3)
    return FlowProjection_gpu_forward_kernel(stream, nElement, ia[0], ia[1], ia[2], ia[3], ia[4], S(0), S(1),
                                             T(0), T(1), T(2));
END
/* flow, count, gradoutput, gradinput1 */
ENTRY(FlowProjection_gpu_backward_kernel, 4)
    return FlowProjection_gpu_backward_kernel(stream, nElement, ia[0], ia[1], ia[2], ia[3], S(0), S(1),
                                              T(0), T(1), T(2), T(3));
END
/* flow, depth, count, output */
ENTRY(DepthFlowProjection_gpu_forward_kernel, 4)
    return DepthFlowProjection_gpu_forward_kernel(stream, nElement, ia[0], ia[1], ia[2], ia[3], ia[4],
                                                  S(0), S(1), S(2), T(0), T(1), T(2), T(3));
END
/* flow, depth, count, output, gradoutput, gradinput1, gradinput2 */
ENTRY(DepthFlowProjection_gpu_backward_kernel, 7)
    return DepthFlowProjection_gpu_backward_kernel(stream, nElement, ia[0], ia[1], ia[2], ia[3], S(0), S(1), S(2),
                                                   T(0), T(1), T(2), T(3), T(4), T(5), T(6));
END
ENTRY(minDepthFlowProjection_gpu_forward_kernel, 4)
    return minDepthFlowProjection_gpu_forward_kernel(stream, nElement, ia[0], ia[1], ia[2], ia[3], ia[4],
                                                     S(0), S(1), S(2), T(0), T(1), T(2), T(3));
END
ENTRY(minDepthFlowProjection_gpu_backward_kernel, 7)
    return minDepthFlowProjection_gpu_backward_kernel(stream, nElement, ia[0], ia[1], ia[2], ia[3], S(0), S(1), S(2),
                                                      T(0), T(1), T(2), T(3), T(4), T(5), T(6));
END

/* ---- Interpolation, InterpolationCh.  ia = w, h, channel, batch ---- */
/* image, flow, output */
ENTRY(InterpolationLayer_gpu_forward_kernel, 3)
    return InterpolationLayer_gpu_forward_kernel(stream, nElement, ia[0], ia[1], ia[2], ia[3], S(0), S(1),
                                                 T(0), T(1), T(2));
END
/* image, flow, gradoutput, gradinput1, gradinput2 */
ENTRY(InterpolationLayer_gpu_backward_kernel, 5)
    return InterpolationLayer_gpu_backward_kernel(stream, nElement, ia[0], ia[1], ia[2], ia[3], S(0), S(1),
                                                  T(0), T(1), T(2), T(3), T(4));
END
ENTRY(InterpolationChLayer_gpu_forward_kernel, 3)
    return InterpolationChLayer_gpu_forward_kernel(stream, nElement, ia[0], ia[1], ia[2], ia[3], S(0), S(1),
                                                   T(0), T(1), T(2));
END
ENTRY(InterpolationChLayer_gpu_backward_kernel, 5)
    return InterpolationChLayer_gpu_backward_kernel(stream, nElement, ia[0], ia[1], ia[2], ia[3], S(0), S(1),
                                                    T(0), T(1), T(2), T(3), T(4));
END

/* ---- SeparableConv, SeparableConvFlow.  ia = w, h, channel, batch, filter_size (= input2.size(1),
 *      separableconv_cuda.cc:70, separableconvflow_cuda.cc:80) ---- */
/* image, vertical, horizontal, output */
ENTRY(SeparableConvLayer_gpu_forward_kernel, 4)
    return SeparableConvLayer_gpu_forward_kernel(stream, nElement, ia[0], ia[1], ia[2], ia[3], ia[4],
                                                 S(0), S(1), S(2), S(3), T(0), T(1), T(2), T(3));
END
/* image, vertical, horizontal, gradoutput (its strides are "output" strides, separableconv_cuda.cc:128-131),
 * gradinput1..3 */
ENTRY(SeparableConvLayer_gpu_backward_kernel, 7)
    return SeparableConvLayer_gpu_backward_kernel(stream, nElement, ia[0], ia[1], ia[2], ia[3], ia[4],
                                                  S(0), S(1), S(2), S(3), T(0), T(1), T(2), T(3), T(4), T(5), T(6));
END
/* image (sizes only), vertical, horizontal, flow_output */
ENTRY(SeparableConvFlowLayer_gpu_forward_kernel, 4)
    return SeparableConvFlowLayer_gpu_forward_kernel(stream, nElement, ia[0], ia[1], ia[2], ia[3], ia[4],
                                                     S(0), S(1), S(2), S(3), T(0), T(1), T(2), T(3));
END
/* image, vertical, horizontal, gradflow_output, gradinput1..3 */
ENTRY(SeparableConvFlowLayer_gpu_backward_kernel, 7)
    return SeparableConvFlowLayer_gpu_backward_kernel(stream, nElement, ia[0], ia[1], ia[2], ia[3], ia[4],
                                                      S(0), S(1), S(2), S(3),
                                                      T(0), T(1), T(2), T(3), T(4), T(5), T(6));
END

/* ---- correlation, fp32.  ia = batch, channels, height, width, out channels, out height, out width,
 *      pad_size, kernel_size, max_displacement, stride1, stride2.  The launchers return 1 on success
 *      (correlation_cuda_kernel.cu:426); the wrappers return 0 on success like the rest. ---- */
/* input1, input2, output, rInput1, rInput2: argument order of correlation_cuda.cc:42-76 */
ENTRY(correlation_forward_cuda_kernel, 5)
    return !correlation_forward_cuda_kernel(T(2), ia[0], ia[4], ia[5], ia[6], S(2),
                                            T(0), ia[1], ia[2], ia[3], S(0),
                                            T(1), ia[1], S(1),
                                            T(3), T(4), ia[7], ia[8], ia[9], ia[10], ia[11], 1, stream);
END
/* input1, input2, gradOutput, gradInput1, gradInput2, rInput1, rInput2: correlation_cuda.cc:115-158 */
ENTRY(correlation_backward_cuda_kernel, 7)
    return !correlation_backward_cuda_kernel(T(2), ia[0], ia[4], ia[5], ia[6], S(2),
                                             T(0), ia[1], ia[2], ia[3], S(0),
                                             T(1), S(1),
                                             T(3), S(3),
                                             T(4), ia[1], S(4),
                                             T(5), T(6), ia[7], ia[8], ia[9], ia[10], ia[11], 1, stream);
END
