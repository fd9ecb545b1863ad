// filterinterp_dev.h -- device code shared by the whole FilterInterpolation family: the direct and the LDS-staged
// kernels, _ori and deformable, forward and backward, fp32 and fp16, and the fused blend in glue.hip.
#pragma once
#include "vfi_common.h"

#include <limits.h>

#include <type_traits>

namespace vfi {

// ---- one pixel's geometry (filterinterpolation_cuda_kernel.cu:2731-2747): the one definition for every kernel of the family
// and for the host mirrors, oracle/np_oracle.py:_fi_geometry and tests/fi_windows.py:samples.  A kernel whose code a helper
// changes keeps that step written out and says so there: the validity test of the kernels that return on an invalid pixel,
// all of fi_backward_ori4_tile and fi_backward_defor.

// validity test of the adaptive-warping layer (:2735-2736)
__device__ __forceinline__ bool fi_valid(float fx, float fy, float x2, float y2, int w, int h) {
    return x2 >= 0.0f && y2 >= 0.0f && x2 <= (float)(w - 1) && y2 <= (float)(h - 1) &&
           fabsf(fx) < (float)w / 2.0f && fabsf(fy) < (float)h / 2.0f;
}

// the flow of pixel (x, y) of batch item b; 0 for a thread outside the image
struct FiFlow { float fx, fy; };
__device__ __forceinline__ FiFlow fi_flow_at(const float* __restrict__ in2, const vfi_strides& s2, int b, int x, int y,
                                             bool inimg = true) {
    FiFlow f{0.0f, 0.0f};
    if (inimg) {
        const float* flow = in2 + (int64_t)b * s2.b + (int64_t)y * s2.h + x;
        f.fx = flow[0];
        f.fy = flow[s2.c];
    }
    return f;
}

// FiPoint: where the flow sends the pixel, and whether the layer interpolates there.  FiGeom adds the cell: the integer
// position (ix, iy) and the blend weights.  (The window corner L, T = ix + 1 - fs / 2, iy + 1 - fs / 2 stays with the kernels:
// formed in here it changes their code.)
struct FiPoint { bool valid; float x2, y2; };
struct FiGeom : FiPoint { int ix, iy; float alpha, beta; };
__device__ __forceinline__ FiPoint fi_point(float fx, float fy, int x, int y, int w, int h, bool inimg = true) {
    FiPoint p;
    p.x2 = (float)x + fx;
    p.y2 = (float)y + fy;
    p.valid = inimg && fi_valid(fx, fy, p.x2, p.y2, w, h);
    return p;
}
// An invalid pixel that stays alive gets cell (ix_invalid, 0), and no conversion of an x2 that may be NaN or huge; nothing
// reads its results.  The fp16 staged kernel passes 1, so that L = ix - 1 = 0: a window its column clamp leaves where it is.
__device__ __forceinline__ FiGeom fi_cell(const FiPoint& p, int ix_invalid = 0) {
    FiGeom g;
    g.valid = p.valid; g.x2 = p.x2; g.y2 = p.y2;
    g.ix = p.valid ? (int)p.x2 : ix_invalid;
    g.iy = p.valid ? (int)p.y2 : 0;
    g.alpha = p.x2 - (float)g.ix;
    g.beta = p.y2 - (float)g.iy;
    return g;
}
__device__ __forceinline__ FiGeom fi_geom(float fx, float fy, int x, int y, int w, int h, bool inimg = true, int ix_invalid = 0) {
    return fi_cell(fi_point(fx, fy, x, y, w, h, inimg), ix_invalid);
}

// copy-through of an invalid pixel (:2814-2818), channels [c0, c1) in planes cs apart: from pointers to the pixel, or (the
// staged kernels) from plane pointers and the pixel's element offset.  Two spellings, because either changes the other's kernels.
template <typename E>
__device__ __forceinline__ void fi_copy_through(const E* src, E* dst, int c0, int c1, int64_t cs) {
    for (int c = c0; c < c1; ++c) dst[(int64_t)c * cs] = src[(int64_t)c * cs];
}
template <typename E>
__device__ __forceinline__ void fi_copy_through(const E* src, E* dst, unsigned pix, int c0, int c1, int64_t cs) {
    for (int c = c0; c < c1; ++c) dst[(int64_t)c * cs + pix] = src[(int64_t)c * cs + pix];
}
// ... and, TO, into a destination whose planes are cso_to apart (the *_to entry points: the output is a channel slice of a
// wider buffer; its rows are as far apart as the source's, so the pixel's offset inside a plane is the same on both sides).
// !TO: cso_to is not looked at and the function is the one above.  (TO is a template parameter of every helper that takes
// the two strides, not a second value that happens to be equal: a helper is optimised before it is inlined, and with two
// strides it comes out as other code even where its caller passes the same value twice.)
// FI_CSO, the destination's plane distance inside such a helper, is spelled as this expression wherever it is used: a local
// variable holding it, captured by the channel loops' lambdas, changed the dense blend instance and the multi-flow kernel.
#define FI_CSO (TO ? cso_to : cs)
template <bool TO, typename E>
__device__ __forceinline__ void fi_copy_through_to(const E* src, E* dst, int c0, int c1, int64_t cs, int64_t cso_to) {
    for (int c = c0; c < c1; ++c) dst[(int64_t)c * FI_CSO] = src[(int64_t)c * cs];
}
template <bool TO, typename E>
__device__ __forceinline__ void fi_copy_through_to(const E* src, E* dst, unsigned pix, int c0, int c1, int64_t cs, int64_t cso_to) {
    for (int c = c0; c < c1; ++c) dst[(int64_t)c * FI_CSO + pix] = src[(int64_t)c * cs + pix];
}

// Where a forward kernel of the _ori family writes.  Its last parameters are a pack `DST... so`: empty in the dense instances
// (the output is laid out as input1 -- their parameter lists and their code are what they were before a destination could
// have a layout of its own), one vfi_strides in the *_to instances.  Contract: so.h == s1.h, so that a pixel's offset
// inside a plane is one register shared by the load and the store; batch and channel strides are free.
__device__ __forceinline__ const vfi_strides& fi_dst(const vfi_strides& s1) { return s1; }
__device__ __forceinline__ const vfi_strides& fi_dst(const vfi_strides&, const vfi_strides& so) { return so; }

// One pixel's 4x4 window, fs == 4: every quadrant is 2x2.  v = the 16 image
// taps (row major), f = the 16 filter taps.  Accumulation order inside each
// quadrant is rows outer, columns inner (filterinterpolation_cuda_kernel.cu:2749-2787);
// `acc += a*b` fused as nvcc -fmad=true fuses it.
__device__ __forceinline__ float fi4_pixel(const float (&v)[16], const float (&f)[16], float alpha, float beta) {
    float TL = v[0] * f[0];   TL = fmaf(v[1], f[1], TL);   TL = fmaf(v[4], f[4], TL);   TL = fmaf(v[5], f[5], TL);
    float TR = v[2] * f[2];   TR = fmaf(v[3], f[3], TR);   TR = fmaf(v[6], f[6], TR);   TR = fmaf(v[7], f[7], TR);
    float BL = v[8] * f[8];   BL = fmaf(v[9], f[9], BL);   BL = fmaf(v[12], f[12], BL); BL = fmaf(v[13], f[13], BL);
    float BR = v[10] * f[10]; BR = fmaf(v[11], f[11], BR); BR = fmaf(v[14], f[14], BR); BR = fmaf(v[15], f[15], BR);
    return blend4(alpha, beta, TL, TR, BL, BR);
}

// Row of staged element e (e < 2^15) in a window of row pitch p: floor(e / p) through a float reciprocal -- (e + 0.5) / p never
// comes within 0.5 / p of an integer, while the two roundings are off by less than 2e-3 / p (the quotient is at most 2^15 / p)
// -- instead of a 32-bit integer division (~40 instructions, once per staged element and tile).
__device__ __forceinline__ int fi_row_of(int e, float inv_pitch) {
    return (int)(((float)e + 0.5f) * inv_pitch);
}

// LDS row pitch of a staged window bw elements (dwords) wide: a multiple of the 32 banks, plus FI_PITCH_SKEW.
// The LDS serves the 4-byte tap reads 32 lanes per clock on 32 banks (measured with rocprofv3's SQ_LDS_BANK_CONFLICT on
// controlled flow fields, tools/lds_conflicts.sh).  fp32 windows: 32 neighbouring lanes read 32 different columns, so with a
// pitch that is a multiple of 32 a tap's bank depends on its column only and lanes that sit on different window rows (a step
// in the flow's vertical part) cannot collide -- 0 conflict cycles on such fields, 50 % with a skew of 8 or 16; what is left
// on a smooth field are the lanes a stretching flow pushes onto a 33rd column.  fp16 windows: two neighbouring lanes share
// a dword -- a broadcast while they sit on one row, a two-way conflict when the step falls between them (50 % conflict
// cycles on a field with a step per 20 lanes, 45 % on the smooth field).  There the 32 lanes use 16-17 banks, and a skew of
// 16 dwords puts the next row's copy of a dword on a bank none of them uses: conflict cycles on the smooth field 138 M ->
// 63 M per C=196 launch (-4.5 % time), on the quarter field 637 M -> 412 M (-20 %).
#ifndef FI_PITCH_SKEW
#define FI_PITCH_SKEW 0
#endif
__device__ __forceinline__ int fi_pitch_for(int bw) {
    return FI_PITCH_SKEW ? (((max(bw - FI_PITCH_SKEW, 0) + 31) & ~31) + FI_PITCH_SKEW) : ((bw + 31) & ~31);
}

// A tile's staged window: bw x bh elements from column bx0 / row by0 of an h x w plane with row stride hs, at LDS row
// pitch `pitch`
struct FiWindow { int bx0, by0, bw, bh, pitch, h, w, hs; };

// ---- shared by the LDS-staged kernels

// compile-time loop: the body sees a constant index, so register arrays indexed by it stay in
// registers (a runtime-indexed array would be demoted to scratch)
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// s_waitcnt vmcnt(G*K): everything but the youngest G staged windows (K DMA loads each) has landed, G = younger_groups
// (at most 3).  The count is clamped to the 6-bit vmcnt field: a smaller count only makes the wait stricter.  The pixel
// stores of the compute phases sit in the same in-order counter; not counting them only makes the wait stricter too.
template <int K>
__device__ __forceinline__ void wait_windows(int younger_groups) {
    switch (younger_groups) {
    case 0:  asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1:  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(K < 63 ? K : 63) : "memory"); break;
    case 2:  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * K < 63 ? 2 * K : 63) : "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * K < 63 ? 3 * K : 63) : "memory"); break;
    }
}

// Bounding box of a tile in the 4 header words of its LDS array, box = {x0, y0, x1, y1}:
//     if (tid == 0) fi_box_clear(box);
//     __syncthreads();
//     const bool any_valid = fi_box_fold(box, tid, lo_x, lo_y, hi_x, hi_y);
// folds the smallest (lo_x, lo_y) and the largest (hi_x, hi_y) over the workgroup's threads into box, one lane per wave, and
// ends with a barrier.  A thread with nothing to add passes INT_MAX / INT_MIN; false: no thread added anything.  (The
// thread-0 branch stays in the kernel: moved into a helper, it changes the compiled kernels.)
__device__ __forceinline__ void fi_box_clear(int* box) { box[0] = INT_MAX; box[1] = INT_MAX; box[2] = INT_MIN; box[3] = INT_MIN; }
__device__ __forceinline__ bool fi_box_fold(int* box, int tid, int lo_x, int lo_y, int hi_x, int hi_y) {
    const int x0 = wave_min_i32(lo_x), y0 = wave_min_i32(lo_y);
    const int x1 = wave_max_i32(hi_x), y1 = wave_max_i32(hi_y);
    if ((tid & 63) == 0 && x0 != INT_MAX) {
        atomicMin(&box[0], x0); atomicMin(&box[1], y0);
        atomicMax(&box[2], x1); atomicMax(&box[3], y1);
    }
    __syncthreads();
    return box[0] != INT_MAX;
}
// a thread's own running box (lo_x, lo_y, hi_x, hi_y), widened by the 4x4 window at (L, T) of a valid pixel
__device__ __forceinline__ void fi_box_add4(bool valid, int L, int T, int& lo_x, int& lo_y, int& hi_x, int& hi_y) {
    if (valid) {
        lo_x = min(lo_x, L); lo_y = min(lo_y, T);
        hi_x = max(hi_x, L + 3); hi_y = max(hi_y, T + 3);
    }
}

// A tile of a launch over tiles_x x tiles_y tiles per batch item, tile index row-major within an item: batch item b, tile
// row ty, tile column tx, and the channel range [c_begin, c_end) of this workgroup (blockIdx.y of ch_per_group channels).
struct FiTile { int b, ty, tx, c_begin, c_end; };
__device__ __forceinline__ FiTile fi_tile_at(int tile, int tiles_x, int tiles_y, int channel, int ch_per_group) {
    FiTile t;
    t.b = tile / (tiles_x * tiles_y);
    const int trem = tile - t.b * (tiles_x * tiles_y);
    t.ty = trem / tiles_x;
    t.tx = trem - t.ty * tiles_x;
    t.c_begin = blockIdx.y * ch_per_group;
    t.c_end = min(channel, t.c_begin + ch_per_group);
    return t;
}

// XCD-grouped tile order.  Workgroups are dealt round-robin over the FI_XCDS XCDs, each with its own L2, and a tile's
// window rows share their first and last 128-byte line with the horizontal neighbours' windows.  FI_XCD_RUN horizontally
// consecutive tiles go to ONE XCD (workgroups b, b + 8, b + 16, b + 24 share an XCD and start together), so three of four
// shared lines are L2 hits: EA read requests per C=196 launch 39.1 M -> 31.2 M (5.0 -> 4.0 GB), 1-9 % less time depending
// on the box.  Larger departures from raster order lose more than they save: XCD-contiguous bands +12 % time, 4x2 / 2x2
// tile blocks per XCD -25 % reads but +15-30 % time.
// Contract: gridDim.x is a multiple of FI_XCDS x FI_XCD_RUN (fi_xcd_grid); workgroups whose tile is >= ntiles leave.
#define FI_XCDS 8
#define FI_XCD_RUN 4
// device: the tile of workgroup bid = blockIdx.x, computed in type I.  The fp32 kernels compute it as int, the fp16 kernel as
// unsigned: the same tiles, different instructions (one type for all would change some kernel's code).
template <typename I>
__device__ __forceinline__ int fi_xcd_tile(I bid) {
    const I xs = bid % FI_XCDS, k = bid / FI_XCDS;
    return ((k / FI_XCD_RUN) * FI_XCDS + xs) * FI_XCD_RUN + (k % FI_XCD_RUN);
}
// host: gridDim.x for ntiles tiles, each XCD's share rounded up to a multiple of ROUND
template <int ROUND = FI_XCD_RUN>
inline int fi_xcd_grid(int ntiles) {
    static_assert(ROUND % FI_XCD_RUN == 0, "whole runs of tiles per XCD");
    return ((ntiles + FI_XCDS - 1) / FI_XCDS + ROUND - 1) / ROUND * ROUND * FI_XCDS;
}

// one channel of one valid pixel, fs == 4, from precomputed clamped row / column offsets.  Row by row, so the register need
// is 4 taps + 4 sums (the compiler may still batch rows when it has registers to spare); the operation order per quadrant is
// that of fi4_pixel.
__device__ __forceinline__ float fi4_value(const float* __restrict__ p, const unsigned (&ro)[4], const unsigned (&co)[4],
                                           const float (&f)[16], float alpha, float beta) {
    float a0 = p[ro[0] + co[0]], a1 = p[ro[0] + co[1]], a2 = p[ro[0] + co[2]], a3 = p[ro[0] + co[3]];
    float TL = a0 * f[0];  TL = fmaf(a1, f[1], TL);
    float TR = a2 * f[2];  TR = fmaf(a3, f[3], TR);
    a0 = p[ro[1] + co[0]]; a1 = p[ro[1] + co[1]]; a2 = p[ro[1] + co[2]]; a3 = p[ro[1] + co[3]];
    TL = fmaf(a0, f[4], TL);  TL = fmaf(a1, f[5], TL);
    TR = fmaf(a2, f[6], TR);  TR = fmaf(a3, f[7], TR);
    a0 = p[ro[2] + co[0]]; a1 = p[ro[2] + co[1]]; a2 = p[ro[2] + co[2]]; a3 = p[ro[2] + co[3]];
    float BL = a0 * f[8];   BL = fmaf(a1, f[9], BL);
    float BR = a2 * f[10];  BR = fmaf(a3, f[11], BR);
    a0 = p[ro[3] + co[0]]; a1 = p[ro[3] + co[1]]; a2 = p[ro[3] + co[2]]; a3 = p[ro[3] + co[3]];
    BL = fmaf(a0, f[12], BL);  BL = fmaf(a1, f[13], BL);
    BR = fmaf(a2, f[14], BR);  BR = fmaf(a3, f[15], BR);
    return blend4(alpha, beta, TL, TR, BL, BR);
}

// channel loop of one valid pixel gathering straight from global memory; TO: the destination's planes are cso_to apart
template <bool TO>
__device__ __forceinline__ void fi4_channels_direct(const float* __restrict__ img, float* __restrict__ dst,
                                                    int c0, int c1, int64_t cs, int64_t cso_to, int hs, int h, int w,
                                                    int L, int T, const float (&f)[16], float alpha, float beta) {
    // unsigned 32-bit element offsets from a wave-uniform plane pointer: the loads take the
    // scalar-base + vector-offset form, one VGPR per address
    unsigned ro[4], co[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ro[k] = (unsigned)(clampi(T + k, 0, h - 1) * hs);
        co[k] = (unsigned)clampi(L + k, 0, w - 1);
    }
    for (int c = c0; c < c1; ++c) dst[(int64_t)c * FI_CSO] = fi4_value(img + (int64_t)c * cs, ro, co, f, alpha, beta);
}

// quadrant sums for a runtime filter size, rows outer / columns inner per quadrant
__device__ __forceinline__ void quadrants_generic(const float* __restrict__ plane, const float* __restrict__ fpx,
                                                  int64_t fcs, int hs, int h, int w, int fs,
                                                  int L, int T, int ix, int iy, float q[4]) {
    const int R = L + fs, Bm = T + fs;
    float TL = 0.0f, TR = 0.0f, BL = 0.0f, BR = 0.0f;
    for (int j = T; j <= iy; ++j) {
        const float* row = plane + (int64_t)clampi(j, 0, h - 1) * hs;
        for (int i = L; i <= ix; ++i)
            TL = fmaf(row[clampi(i, 0, w - 1)], fpx[(int64_t)((j - T) * fs + (i - L)) * fcs], TL);
    }
    for (int j = T; j <= iy; ++j) {
        const float* row = plane + (int64_t)clampi(j, 0, h - 1) * hs;
        for (int i = ix + 1; i < R; ++i)
            TR = fmaf(row[clampi(i, 0, w - 1)], fpx[(int64_t)((j - T) * fs + (i - L)) * fcs], TR);
    }
    for (int j = iy + 1; j < Bm; ++j) {
        const float* row = plane + (int64_t)clampi(j, 0, h - 1) * hs;
        for (int i = L; i <= ix; ++i)
            BL = fmaf(row[clampi(i, 0, w - 1)], fpx[(int64_t)((j - T) * fs + (i - L)) * fcs], BL);
    }
    for (int j = iy + 1; j < Bm; ++j) {
        const float* row = plane + (int64_t)clampi(j, 0, h - 1) * hs;
        for (int i = ix + 1; i < R; ++i)
            BR = fmaf(row[clampi(i, 0, w - 1)], fpx[(int64_t)((j - T) * fs + (i - L)) * fcs], BR);
    }
    q[0] = TL; q[1] = TR; q[2] = BL; q[3] = BR;
}

// ---- the fused FilterInterpolate of both frames (glue.hip, rectify_head_bf16.hip)

// one side's pixel geometry (fi_geom) and window corner, from the pixel's flow in registers or from memory
struct FiSide {
    bool valid;
    int L, T, ix, iy;
    float alpha, beta;
};
__device__ __forceinline__ FiSide fi_side(float fx, float fy, int x, int y, int w, int h, int fs, bool inimg = true) {
    const FiGeom g = fi_geom(fx, fy, x, y, w, h, inimg);
    return FiSide{g.valid, g.ix + 1 - fs / 2, g.iy + 1 - fs / 2, g.ix, g.iy, g.alpha, g.beta};
}
__device__ __forceinline__ FiSide fi_side(const float* __restrict__ flow, int64_t cstride, int x, int y, int w, int h, int fs) {
    return fi_side(flow[0], flow[cstride], x, y, w, h, fs);
}
__device__ __forceinline__ float fi_side_value(const FiSide& s, const float* __restrict__ plane, const float* __restrict__ fpx,
                                               int64_t fcs, int hs, int h, int w, int fs, int x, int y) {
    if (!s.valid) return plane[(int64_t)y * hs + x];       // copy-through (:2814-2818)
    float q[4];
    quadrants_generic(plane, fpx, fcs, hs, h, w, fs, s.L, s.T, s.ix, s.iy, q);
    return blend4(s.alpha, s.beta, q[0], q[1], q[2], q[3]);
}

}  // namespace vfi
