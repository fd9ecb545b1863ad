// correlation_dev.h -- the pieces the correlation kernels share (correlation.hip, correlation_bf16.hip,
// warp_correlation.hip): which image of a launch a workgroup works on, the staging plan in aligned units, the 32x4 tile with
// two pixels per lane, the mean of the running sums, the forward epilogues and the checks of the entries.  (The backward:
// correlation_bwd.h.)  Internal to the library.
#pragma once
#include "vfi_common.h"

#include <cfloat>
#include <initializer_list>

namespace vfi {

#define CORR_CC_ROWS 8   // channels staged per LDS fill by the wave-per-displacement-row kernels (16 measured the same: their chunk loop is LDS-bound, one workgroup per CU)

// The tensors of a launch: one call, or two calls of equal shape in one launch (both flow directions of a pyramid level: at
// the coarse levels a launch is latency, 13-18 us for 1 MB, and two cost what one does).  Images 0 .. per - 1 are item 0's.
struct CorrItems { const float* in1[2]; const float* in2[2]; float* out[2]; int per; };

// Image `img` of a launch: the item it belongs to and its index `b` inside that item.  A kernel indexes its own `items`
// argument with `item` and binds the three pointers to __restrict__ locals: handing `items` to a helper takes the
// argument's address, and the compiler then loads all six pointers and selects, instead of the three at `item`.
struct CorrImage { int item, b; };
__device__ __forceinline__ CorrImage corr_image(int img, int per) {
    const int item = img >= per ? 1 : 0;                    // (two calls in one launch: vfi_correlation_forward_pair)
    return {item, img - item * per};
}

// Staging plan in aligned units of four elements of EB bytes: unit e = tid + k * NT of a chunk's [CC][ROWS][UW] block whose
// rows start at frame position (y0, x0), x0 and w multiples of 4 (so a unit lies wholly inside or wholly outside the frame),
// as a byte offset from the chunk's first plane.  The loads are buffer loads through a descriptor that spans exactly the
// chunk's planes: a unit outside the frame gets an offset out of any range, a channel past the last one falls out of the
// descriptor's, and both arrive as zeros.
template <unsigned EB, int CC, int ROWS, int UW, int NT, int N>
__device__ __forceinline__ void corr_unit_plan(unsigned (&off)[N], int tid, int y0, int x0, int h, int w, int plane) {
    static_assert(N == (CC * ROWS * UW + NT - 1) / NT, "units per thread");
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int e = tid + k * NT;
        const int c = e / (ROWS * UW), rem = e - c * (ROWS * UW);
        const int r = rem / UW, col = 4 * (rem - r * UW);
        const int gy = y0 + r, gx = x0 + col;
        const bool ok = e < CC * ROWS * UW && gy >= 0 && gy < h && gx >= 0 && gx < w;
        off[k] = ok ? EB * (unsigned)(c * plane + gy * w + gx) : 0x80000000u;
    }
}

// The 32x4 tile of output pixels with one wave per displacement row (threadIdx.y = tj) and TWO horizontally adjacent pixels
// per lane: per channel a lane reads the D + 1 window values its two D-wide displacement rows share as (D + 1) / 2 aligned
// pairs.
template <int MD_>
struct CorrTile2 {
    static constexpr int MD = MD_, D = 2 * MD + 1, TW = 32, TH = 4, LW = TW + 2 * MD, LH = TH + 2 * MD, NT = 64 * D, CC = CORR_CC_ROWS;
    static constexpr int UW = LW / 4, NU = CC * LH * UW, NPT = (NU + NT - 1) / NT;    // window units of four elements per chunk, per thread
    static constexpr int FU = CC * TH * (TW / 4), NF1 = (FU + NT - 1) / NT;           // ... of the first map
    static constexpr int PAIRS = (D + 1) / 2;
    static __device__ __forceinline__ int px(int lane) { return 2 * (lane & 15); }
    static __device__ __forceinline__ int py(int lane) { return lane >> 4; }
    // the pairs at window row `row` from column px on (P: float2-like or __half2)
    template <class P, class E>
    static __device__ __forceinline__ void read_row(const E* row, P (&r)[PAIRS]) {
#pragma unroll
        for (int k = 0; k < PAIRS; ++k) r[k] = reinterpret_cast<const P*>(row)[k];
    }
};

// The mean of the running sums, handed to `store` as a function of one sum: a product with the exact reciprocal for a
// power-of-two channel count (the same real number), a division otherwise.
template <class Store>
__device__ __forceinline__ void corr_store_mean(int channel, Store&& store) {
    const float nelems = (float)channel;
    const float inv = 1.0f / nelems;
    if ((channel & (channel - 1)) == 0) store([&](float v) { return v * inv; });
    else store([&](float v) { return v / nelems; });
}

// What a float forward kernel does with a mean as it stores it, and where plane k of image b begins in the output: a
// compile-time choice, so the plain instances are the kernels they were.  CorrPlain: the mean as it is, dense images.
// CorrLrelu: PWC-Net's LeakyReLU on the mean, y = v > 0 ? v : v * slope -- ONE multiplication of the value the plain kernel
// stores (NaN stays NaN, -0 becomes -0 * slope: torch's leaky_relu in float) -- into an output whose images lie
// stride[item] elements apart while the planes of an image stay contiguous (the first channels of a concatenation buffer).
struct CorrPlain {
    static constexpr bool DENSE = true;
    __device__ __forceinline__ float operator()(float v) const { return v; }
    __device__ __forceinline__ int64_t plane(int, int b, int oc, int k, int oh, int ow) const { return ((int64_t)b * oc + k) * oh * ow; }
};
struct CorrLrelu {
    static constexpr bool DENSE = false;
    int64_t stride[2];
    float slope;
    __device__ __forceinline__ float operator()(float v) const { return v > 0.0f ? v : v * slope; }
    __device__ __forceinline__ int64_t plane(int item, int b, int, int k, int oh, int ow) const {
        return (int64_t)b * stride[item] + (int64_t)k * oh * ow;
    }
};

// Host side, defined in correlation.hip and shared with correlation_bf16.hip: the checks every entry makes before it
// launches, and the tiled backward kernels' split of the channels into groups.
int corr_check(std::initializer_list<const void*> tensors, int batch, int channel, int h, int w, int pad_size, int kernel_size,
               int max_displacement, int stride1, int stride2, bool backward, int* oc, int* oh, int* ow);
int corr_backward_groups(int tiles, int batch, int channel, int* ch_per_group);
// LeakyReLU's slope as the fused entries take it, forward and backward: finite and positive (the backward reads the
// pre-activation's sign off y)
inline bool corr_slope_ok(float slope) { return slope > 0.0f && slope <= FLT_MAX; }

}  // namespace vfi
