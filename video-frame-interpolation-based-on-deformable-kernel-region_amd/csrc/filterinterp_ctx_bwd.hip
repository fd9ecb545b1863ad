// filterinterp_ctx_bwd.hip -- the backward of the context warp on float32 gradients: the float instances of the kernels
// and the launcher of filterinterp_ctx_bwd.h.
#include "filterinterp_ctx_bwd.h"

// The tile these instances are built for, restated.  tests/fi_ctx_backward.py, the host mirror of this call, takes its
// constants from this unit's #defines, so that a mirror written against the unit keeps reading them where it always has;
// a restatement that differs from the header's does not compile.
#pragma clang diagnostic error "-Wmacro-redefined"
#define CB_TW 64
#define CB_TH 8
#define CB_THREADS (CB_TW * CB_TH)
#define CB_CH 6
#define CB_CELLS 6144
#define CB_NT 3

using namespace vfi;

extern "C" int vfi_filterinterp_backward_ori_image_multi(const float* const* flows, const float* input3,
                                                          const float* const* gradoutputs, float* gradinput1, int nflows,
                                                          int batch, int channel, int h, int w, int filter_channels,
                                                          vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides sg,
                                                          vfi_stream_t stream) {
    return backward_image_multi<float>(flows, input3, gradoutputs, gradinput1, nflows, batch, channel, h, w, filter_channels, s1,
                                       s2, s3, sg, stream);
}
