// filterinterp_paths.h -- the per-path launchers the FilterInterpolation entry points of vfi_hip.h dispatch to.
//
// Internal to libvfi_hip.so, with C++ linkage: a definition and a call that disagree on the parameters fail to compile
// or link instead of passing the wrong arguments.  Each launcher returns VFI_OK or VFI_ERR_LAUNCH, or FI_DECLINED when
// its kernel does not take the shape; then it has launched nothing and the caller takes the next path.
#pragma once
#include "vfi_common.h"

namespace vfi {

constexpr int FI_DECLINED = -1;
static_assert(FI_DECLINED != VFI_OK && FI_DECLINED != VFI_ERR_SHAPE && FI_DECLINED != VFI_ERR_LAUNCH, "a distinct result");

// How the staged FilterInterpolation kernels split a tile's channel range over blockIdx.y: ch_per_group channels per
// workgroup, `groups` workgroups (gridDim.y).  The number of groups g minimises a cost, in channels: a workgroup pays
// `prologue` channels' worth before its first channel (flow, filter, bounding box, first window); a launch leaves half a
// round of its slots (2 workgroups per CU) idle at the end on average; and the more workgroups a slot runs, the better their
// unequal durations even out (they go to whichever slot frees first).  Fitted to launches timed in isolation (fs=4, 1080p,
// C=196: 1 group 1.12 ms, 2 1.00-1.03, 3 0.99, 4 1.00, 8 1.08).  Defined in filterinterp.hip.
struct FiSplit { int ch_per_group, groups; };
FiSplit fi_channel_split(int ntiles, int channel, double prologue);

// The _ori forward launchers address what they WRITE with `so`, a layout of its own: w stride 1, so.h == s1.h (a pixel's
// offset inside a plane is one register shared by the load and the store; anything else is VFI_ERR_SHAPE, not a slower
// kernel), batch and channel strides free -- a channel slice of a wider contiguous buffer.  What a launcher decides from
// the input (16-byte staging, the 31-bit range checks, the window classes) does not look at the destination, and every
// store is a single dword, so the destination needs a float's alignment only.  so = s1 is the dense call: it runs the
// instances that carry no second set of strides.

// filterinterp_lds.hip: _ori forward, fs == 4
int launch_fi_ori_lds(const float* input1, const float* input2, const float* input3, float* output, int batch, int channel,
                      int h, int w, vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides so, vfi_stream_t stream);
// filterinterp_lds.hip: the same kernel with the blend of DAIN.FilterInterpolate as its epilogue -- besides output it
// writes blend = other * w0 + output * w2; other / blend have output's strides; declines channel > FI_BLEND_MAXC
int launch_fi_ori_lds_blend(const float* input1, const float* input2, const float* input3, float* output, const float* other,
                            float* blend, float w0, float w2, int batch, int channel, int h, int w, vfi_strides s1,
                            vfi_strides s2, vfi_strides s3, vfi_strides so, vfi_stream_t stream);
// filterinterp_lds_n.hip: _ori forward, fs 2, 5 and 6
int launch_fi_ori_lds_n(const float* input1, const float* input2, const float* input3, float* output, int batch, int channel,
                        int h, int w, int fs, vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides so, vfi_stream_t stream);
// filterinterp.hip: the direct gather, any filter size
int launch_fi_ori_direct(const float* input1, const float* input2, const float* input3, float* output, int batch, int channel,
                         int h, int w, int filter_channels, vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides so,
                         vfi_stream_t stream);
// filterinterp.hip: vfi_filterinterp_forward_ori with a destination layout -- the staged kernel of the filter size, else the
// direct gather; checks its arguments as the entry point does
int fi_forward_ori_to(const float* input1, const float* input2, const float* input3, float* output, int batch, int channel,
                      int h, int w, int filter_channels, vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides so,
                      vfi_stream_t stream);
// filterinterp_defor_lds.hip: forward of the deformable variants, fs 4 and 6
int launch_fi_defor_lds(int variant, const float* input1, const float* input2, const float* input3, const float* input4,
                        float* output, int batch, int channel, int h, int w, int filter_size, vfi_strides s1, vfi_strides s2,
                        vfi_strides s3, vfi_strides s4, vfi_stream_t stream);
// filterinterp_defor_bwd_lds.hip: backward of the deformable variants, fs == 4, into the caller's gradacc scratch (acc,
// hdr); the blocks it flags are left to the caller's per-tap launch
int launch_fi_defor_bwd_lds(int variant, const float* input1, const float* input2, const float* input3, const float* input4,
                            const float* gradoutput, unsigned long long* acc, const int* hdr, int* flags, float* gradinput2,
                            float* gradinput3, float* gradinput4, int batch, int channel, int h, int w, vfi_strides s1,
                            vfi_strides s2, vfi_strides s3, vfi_strides s4, vfi_stream_t stream);

}  // namespace vfi
