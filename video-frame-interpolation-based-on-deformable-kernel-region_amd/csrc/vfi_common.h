// vfi_common.h -- shared device/host helpers for the gfx950 kernels of libvfi_hip.so.
//
// Numerics contract (DESIGN.md "numerics"): the library is compiled with
// -ffp-contract=off; every fused multiply-add is written explicitly with
// fmaf() at the positions where nvcc's default -fmad=true would fuse the
// reference's `acc += a*b` statements.  The CPU oracle's fmad=1 mode performs
// the same operations in the same order, so deterministic ops compare bit for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vfi_hip.h"

#define VFI_WAVE 64

// Pixel tile of the one-thread-per-pixel kernels: one wave = one 64-pixel row
// segment (256-B coalesced rows of every plane), four rows per workgroup.
#define VFI_TX 64
#define VFI_TY 4

namespace vfi {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// (1-a)(1-b)*TL + a(1-b)*TR + (1-a)b*BL + ab*BR, left to right, adds fused
// (filterinterpolation_cuda_kernel.cu:2789-2793; interpolation_cuda_kernel.cu:86-87)
__device__ __forceinline__ float blend4(float a, float b, float TL, float TR, float BL, float BR) {
    const float w00 = (1.0f - a) * (1.0f - b);
    const float w10 = a * (1.0f - b);
    const float w01 = (1.0f - a) * b;
    const float w11 = a * b;
    float t = w00 * TL;
    t = fmaf(w10, TR, t);
    t = fmaf(w01, BL, t);
    t = fmaf(w11, BR, t);
    return t;
}

// Wave-wide min / max as six DPP steps at VALU rate (prefix within each row of 16 lanes, then
// row_bcast:15 and row_bcast:31 carry the row results to lane 63), read back as a scalar.  The
// __shfl_xor butterfly compiles to six dependent ds_bpermute_b32, each an LDS round trip.
#define VFI_DPP_STEP(OP, CTRL, ROWMASK) v = OP(v, __builtin_amdgcn_update_dpp(v, v, CTRL, ROWMASK, 0xf, false))
__device__ __forceinline__ int wave_min_i32(int v) {
    VFI_DPP_STEP(min, 0x111, 0xf); VFI_DPP_STEP(min, 0x112, 0xf); VFI_DPP_STEP(min, 0x114, 0xf);
    VFI_DPP_STEP(min, 0x118, 0xf); VFI_DPP_STEP(min, 0x142, 0xa); VFI_DPP_STEP(min, 0x143, 0xc);
    return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ int wave_max_i32(int v) {
    VFI_DPP_STEP(max, 0x111, 0xf); VFI_DPP_STEP(max, 0x112, 0xf); VFI_DPP_STEP(max, 0x114, 0xf);
    VFI_DPP_STEP(max, 0x118, 0xf); VFI_DPP_STEP(max, 0x142, 0xa); VFI_DPP_STEP(max, 0x143, 0xc);
    return __builtin_amdgcn_readlane(v, 63);
}
#undef VFI_DPP_STEP

// Word 3 of a raw buffer descriptor: DATA_FORMAT (bits 15-18) = 32 bits, no swizzle, no index stride.  Offsets at or past
// num_records bytes load 0 and drop stores without touching memory.
constexpr int BUF_RAW_FLAGS = 0x00020000;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* base, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, BUF_RAW_FLAGS);
}
// LDS destination of an LDS-DMA load (__builtin_amdgcn_raw_ptr_buffer_load_lds)
typedef __attribute__((address_space(3))) void* lds_ptr_t;

inline dim3 pixel_grid(int w, int h, int batch) {
    return dim3((unsigned)((w + VFI_TX - 1) / VFI_TX), (unsigned)((h + VFI_TY - 1) / VFI_TY), (unsigned)batch);
}

// compute units of the CURRENT device (cached per device id)
int device_cu_count();
// The filter size of a FilterInterpolation filter tensor with filter_channels channels, as the reference's bindings compute it
inline int fi_filter_size(int filter_channels) { return (int)sqrtf((float)filter_channels); }
inline int launch_status() {
    return hipGetLastError() == hipSuccess ? VFI_OK : VFI_ERR_LAUNCH;
}

}  // namespace vfi
