// filterinterp_ctx_bwd.h -- the image gradient of FilterInterpolation `_ori` alone, for several flows over one image:
// the backward of the context warp (FilterInterpolate_ctx, networks/DAIN.py:544-552, networks/DAIN_slowmotion.py:311-317).
//
// The reference detaches flow and filter on this path, so only gradinput1 of its backward
// (filterinterpolation_cuda_kernel.cu:2827-2942) is wanted.  That gradient never reads the image: a valid pixel adds
// gradoutput x blend weight x filter tap to the 16 cells of its window.  With several time offsets over one context tensor
// every flow's addends land in the same cells, so ONE accumulator plane, one header and one conversion serve the whole call
// (gradacc.h: every addend rounded to an integer at one scale per call, the sums order-free).  Each addend is formed as
// fi_backward_ori4_tile (filterinterp.hip) forms it, so for one flow the result is that kernel's gradinput1 bit for bit.
// The kernels and the launcher are templates on the gradients' storage E: filterinterp_ctx_bwd.hip instantiates them for float
// (vfi_filterinterp_backward_ori_image_multi), filterinterp_bf16.hip for bfloat16 bits
// (vfi_filterinterp_backward_ori_image_multi_bf16); each unit's instances live in its own object and assembly.
#pragma once
#include "bf16.h"
#include "filterinterp_dev.h"
#include "gradacc.h"

#include <limits.h>

namespace vfi {

// tile of fi_ctx_backward4_lds (below): 64 x 8 pixels like fi_backward_ori4_lds, but the whole LDS array is 64-bit cells
#define CB_TW 64
#define CB_TH 8
#define CB_WAVES 4                                  // (launch bound: waves per SIMD the kernel must fit -- two workgroups per CU)
#define CB_THREADS (CB_TW * CB_TH)
#define CB_CH 6                                     // channels summed per pass at most
#define CB_CELLS 6144                               // 64-bit gradient cells per pass (49,152 bytes)
#define CB_NT 3                                     // flows one launch carries (the time offsets of a x4 slow-motion step)
static_assert(CB_THREADS <= 1024 && CB_THREADS % 64 == 0, "workgroup size");
static_assert(((CB_WAVES * 256) / CB_THREADS) * (2 + CB_CELLS) * 8 <= 160 * 1024, "workgroups per CU x LDS per workgroup exceed the CU's LDS");
static_assert(CB_CELLS < (1 << 15), "fi_row_of takes cell indices below 2^15");

// the flows of one launch and their incoming gradients (t < nt); E: the gradients' storage, float or bfloat16 bits
template <typename E>
struct CbPtrs {
    const float* flow[CB_NT];
    const E* gout[CB_NT];
};
// an incoming gradient element as the arithmetic sees it: bfloat16 storage widened exactly (the addends, and so the integer
// sums, are those of the float32 call on the widened gradients)
__device__ __forceinline__ float cb_grad(const float* p, int64_t o) { return p[o]; }
__device__ __forceinline__ float cb_grad(const bf16_t* p, int64_t o) { return bf16_widen(p[o]); }

// one pixel under one flow: valid, the blend fractions, and its window's clamped rows and columns
struct CbPixel {
    bool valid;
    float alpha, beta;
    int ro[4], co[4];
};
__device__ __forceinline__ CbPixel cb_pixel(const float* __restrict__ flow, const vfi_strides& s2, int b, int x, int y, int h, int w,
                                            bool inimg) {
    CbPixel p;
    const FiFlow fl = fi_flow_at(flow, s2, b, x, y, inimg);
    const float x2 = (float)x + fl.fx;
    const float y2 = (float)y + fl.fy;
    p.valid = inimg && fi_valid(fl.fx, fl.fy, x2, y2, w, h);        // an invalid pixel has no gradient (:2863-2864)
    const int ix = p.valid ? (int)x2 : 0, iy = p.valid ? (int)y2 : 0;
    p.alpha = x2 - (float)ix;
    p.beta = y2 - (float)iy;
#pragma unroll
    for (int k = 0; k < 4; ++k) { p.ro[k] = clampi(iy - 1 + k, 0, h - 1); p.co[k] = clampi(ix - 1 + k, 0, w - 1); }
    return p;
}

// fs == 4, filter_channels == 16.  A workgroup owns a 64 x 8 tile (and the channel range of its group).  The bounding box of
// the (clamped) taps of ALL the launch's flows is the tile's window of gradient cells; as many channels as fit (at most CB_CH)
// are summed per pass in LDS, and each non-zero cell leaves with one global 64-bit atomic.  The 16 filter taps and, per
// flow, the blend fractions and the window's cell offsets stay in registers across the channel loop.  A tile whose window
// does not fit one channel, and every tile of a call that scatters in fp32 or needs the second scale factor, is flagged
// for fi_ctx_backward_px, launched after this kernel with the same flows.
template <typename E>
__global__ __launch_bounds__(CB_THREADS, CB_WAVES) void fi_ctx_backward4_lds(
    CbPtrs<E> ptr, int nt, const float* __restrict__ in3, unsigned long long* __restrict__ acc, const int* __restrict__ hdr,
    int* __restrict__ tileflag, int channel, int h, int w, vfi_strides s2, vfi_strides s3, vfi_strides sg, int groups,
    int ch_per_group) {
    __shared__ __attribute__((aligned(16))) unsigned long long lds64[2 + CB_CELLS];      // header (bounding box), cells
    int* box = reinterpret_cast<int*>(lds64);
    unsigned long long* cells = lds64 + 2;
    const int tid = threadIdx.x;
    const int x = blockIdx.x * CB_TW + (tid & (CB_TW - 1));
    const int y = blockIdx.y * CB_TH + (tid >> 6);
    const int b = blockIdx.z / groups, grp = blockIdx.z - b * groups;
    const int c_begin = grp * ch_per_group, c_end = min(channel, c_begin + ch_per_group);
    const GradAccCtx gctx = gradacc_ctx(hdr);
    const bool inimg = x < w && y < h;
    CbPixel px[CB_NT];
    int lo_x = INT_MAX, lo_y = INT_MAX, hi_x = INT_MIN, hi_y = INT_MIN;
    static_for<0, CB_NT>([&](auto t) {
        px[t] = cb_pixel(ptr.flow[t], s2, b, x, y, h, w, inimg && t < nt);
        if (px[t].valid) {
            lo_x = min(lo_x, px[t].co[0]); lo_y = min(lo_y, px[t].ro[0]);
            hi_x = max(hi_x, px[t].co[3]); hi_y = max(hi_y, px[t].ro[3]);
        }
    });
    // ---- bounding box of the tile's (clamped) taps, all flows
    if (tid == 0) fi_box_clear(box);
    __syncthreads();
    if (!fi_box_fold(box, tid, lo_x, lo_y, hi_x, hi_y)) return;        // (workgroup-uniform: nothing in this tile has a gradient)
    const int bx0 = box[0], by0 = box[1], bw = box[2] - box[0] + 1, bh = box[3] - box[1] + 1;
    const int n = bw * bh;
    const int pc = min(CB_CH, CB_CELLS / n);
    if (!gradacc_staged_ok(gctx) || pc == 0) {              // (workgroup-uniform) left to fi_ctx_backward_px
        if (tid == 0) tileflag[(b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = 1;
        return;
    }

    unsigned long long* gimg = acc + (int64_t)b * channel * h * w;       // dense [b][c][y][x] fixed-point sums
    const float* fpx = in3 + (int64_t)b * s3.b + (int64_t)y * s3.h + x;
    bool any = false;
    static_for<0, CB_NT>([&](auto t) { any = any || px[t].valid; });
    float fv[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) fv[k] = any ? fpx[(int64_t)k * s3.c] : 0.0f;
    // the window rows' first cells, less the box's first column (in place of the rows)
    static_for<0, CB_NT>([&](auto t) {
#pragma unroll
        for (int k = 0; k < 4; ++k) px[t].ro[k] = (px[t].ro[k] - by0) * bw - bx0;
    });
    const int64_t gpx = (int64_t)b * sg.b + (int64_t)y * sg.h + x;
    const float inv_bw = 1.0f / (float)bw;
    for (int e = tid; e < n * pc; e += CB_THREADS) cells[e] = 0ull;
    for (int c0 = c_begin; c0 < c_end; c0 += pc) {
        const int cn = min(pc, c_end - c0);
        // ---- the cells are zero (the barrier); flow by flow, channel by channel, the next channel's gradient in flight
        // behind the adds
        __syncthreads();
        static_for<0, CB_NT>([&](auto t) {
            if (px[t].valid) {
                const E* gp = ptr.gout[t] + gpx + (int64_t)c0 * sg.c;
                const float alpha = px[t].alpha, beta = px[t].beta;
                float g = cb_grad(gp, 0);
#pragma unroll 1
                for (int cc = 0; cc < cn; ++cc) {
                    const float gnext = cc + 1 < cn ? cb_grad(gp, (int64_t)(cc + 1) * sg.c) : 0.0f;
                    unsigned long long* plane = cells + cc * n;
                    const float qg[4] = { g * (1.0f - alpha) * (1.0f - beta), g * alpha * (1.0f - beta),
                                          g * (1.0f - alpha) * beta,          g * alpha * beta };
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const int j = k >> 2, i = k & 3, quad = (j >> 1) * 2 + (i >> 1);
                        atomicAdd(&plane[px[t].ro[j] + px[t].co[i]], (unsigned long long)__float2ll_rn(qg[quad] * fv[k] * gctx.scale));
                    }
                    g = gnext;
                }
            }
        });
        __syncthreads();
        // ---- flush: one global atomic per non-zero cell, and the cell is zero again for the next pass
        for (int cc = 0; cc < cn; ++cc) {
            unsigned long long* plane = gimg + (int64_t)(c0 + cc) * h * w;
            for (int e = tid; e < n; e += CB_THREADS) {
                const unsigned long long v = cells[cc * n + e];
                if (v != 0ull) {
                    const int cy = fi_row_of(e, inv_bw), cx = e - cy * bw;
                    atomicAdd(&plane[(int64_t)(by0 + cy) * w + bx0 + cx], v);
                    cells[cc * n + e] = 0ull;
                }
            }
        }
    }
}

// one thread per pixel, any filter size: every flow of the launch, every channel, each addend through gradacc_add (the
// integer sums, or the reference's fp32 atomics for a call with non-finite inputs).  After fi_ctx_backward4_lds: only the
// tiles that kernel flagged (VFI_TX x VFI_TY blocks nest in them).  A bfloat16 call that scatters in fp32 adds its floats
// into the low words of the zeroed 64-bit cells (gradacc.h), never into bfloat16 storage: g1 is not looked at.
template <typename E>
__global__ __launch_bounds__(VFI_TX * VFI_TY) void fi_ctx_backward_px(
    CbPtrs<E> ptr, int nt, const float* __restrict__ in3, unsigned long long* __restrict__ acc, const int* __restrict__ hdr,
    const int* __restrict__ tileflag, float* g1, int channel, int h, int w, int fs, vfi_strides s1, vfi_strides s2,
    vfi_strides s3, vfi_strides sg) {
    const int x = blockIdx.x * VFI_TX + threadIdx.x;
    const int y = blockIdx.y * VFI_TY + threadIdx.y;
    if (x >= w || y >= h) return;
    const int b = blockIdx.z;
    if (tileflag && !tileflag[(b * ((h + CB_TH - 1) / CB_TH) + y / CB_TH) * gridDim.x + blockIdx.x]) return;
    const GradAccCtx gctx = gradacc_ctx(hdr);
    unsigned long long* gimg = acc + (int64_t)b * channel * h * w;       // dense [b][c][y][x] fixed-point sums
    const float* fpx = in3 + (int64_t)b * s3.b + (int64_t)y * s3.h + x;
    for (int t = 0; t < nt; ++t) {
        const FiFlow fl = fi_flow_at(ptr.flow[t], s2, b, x, y);
        const FiGeom g = fi_geom(fl.fx, fl.fy, x, y, w, h);
        if (!g.valid) continue;                             // no gradient (:2863-2864)
        const int ix = g.ix, iy = g.iy;
        const int L = ix + 1 - fs / 2, T = iy + 1 - fs / 2;
        const float alpha = g.alpha, beta = g.beta;
        const E* gpx = ptr.gout[t] + (int64_t)b * sg.b + (int64_t)y * sg.h + x;
        for (int c = 0; c < channel; ++c) {
            unsigned long long* gp = gimg + (int64_t)c * h * w;
            // (the fp32 scatter of a call with non-finite inputs)
            float* gfp = std::is_same<E, float>::value ? g1 + (int64_t)b * s1.b + (int64_t)c * s1.c : reinterpret_cast<float*>(gp);
            const float gr = cb_grad(gpx, (int64_t)c * sg.c);
            const float qg[4] = { gr * (1.0f - alpha) * (1.0f - beta), gr * alpha * (1.0f - beta),
                                  gr * (1.0f - alpha) * beta,          gr * alpha * beta };
            for (int j = 0; j < fs; ++j) {
                const int cy = clampi(T + j, 0, h - 1);
                for (int i = 0; i < fs; ++i) {
                    const int cx = clampi(L + i, 0, w - 1);
                    const int quad = (T + j > iy ? 2 : 0) + (L + i > ix ? 1 : 0);
                    const float fv = fpx[(int64_t)(j * fs + i) * s3.c];
                    if constexpr (std::is_same<E, float>::value)
                        gradacc_add(gp, gfp, (int64_t)cy * w + cx, (int64_t)cy * s1.h + cx, qg[quad] * fv, gctx);
                    else                                    // (float index 2 x cell index: the cell's low word)
                        gradacc_add(gp, gfp, (int64_t)cy * w + cx, 2 * ((int64_t)cy * w + cx), qg[quad] * fv, gctx);
                }
            }
        }
    }
}

// hdr[3] of the call: gradacc_scan writes the value for one flow's taps; the call's cells receive every flow's
// (a template like the two above: each translation unit that instantiates the call carries its own copy)
template <typename E>
__global__ void fi_ctx_set_cells_log2(int* __restrict__ hdr, int cells_log2) { hdr[3] = cells_log2; }

// the call for gradients stored as E (float, or bfloat16 bits): gradoutputs[t] and gradinput1 are E tensors
template <typename E>
static int backward_image_multi(const float* const* flows, const float* input3, const E* const* gradoutputs, E* gradinput1,
                                int nflows, int batch, int channel, int h, int w, int filter_channels, vfi_strides s1,
                                vfi_strides s2, vfi_strides s3, vfi_strides sg, vfi_stream_t stream) {
    constexpr bool F32 = std::is_same<E, float>::value;
    using Scan = typename std::conditional<F32, GradPlain, GradBf16>::type;
    if (nflows <= 0 || !flows || !gradoutputs || batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || filter_channels <= 0)
        return VFI_ERR_SHAPE;
    if (!input3 || !gradinput1) return VFI_ERR_SHAPE;
    for (int t = 0; t < nflows; ++t)
        if (!flows[t] || !gradoutputs[t]) return VFI_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int fs = fi_filter_size(filter_channels);
    const bool staged = fs == 4 && filter_channels == 16;
    const int tiles_x = (w + CB_TW - 1) / CB_TW, tiles_y = (h + CB_TH - 1) / CB_TH;
    const int64_t ntiles64 = (int64_t)tiles_x * tiles_y * batch;
    const int launches = (nflows + CB_NT - 1) / CB_NT;
    if (batch > 65535 || ntiles64 * launches > INT_MAX) return VFI_ERR_SHAPE;
    const int ntiles = (int)ntiles64;
    // one plane of sums, one header; flags: one word per 64 x 8 tile and launch: "the staged kernel left it alone"
    GradAccScratch sc;
    int err = gradacc_reserve(st, 1, (int64_t)batch * channel * h * w, staged ? ntiles * launches : 0, &sc);
    if (err != VFI_OK) return err;
    // the maxima over every gradient and the filter (the scans raise them with atomicMax into the one header)
    for (int t = 0; t < nflows; ++t) {
        err = gradacc_scan(st, Scan{gradoutputs[t]}, batch, channel, h, w, sg, t == 0 ? input3 : nullptr, filter_channels, s3,
                           sc.dir[0].hdr);
        if (err != VFI_OK) return err;
    }
    // a cell can receive every tap of every pixel of every flow
    const int64_t taps = (int64_t)(filter_channels > 4 ? filter_channels : 4) * nflows;
    int cells_log2 = 0;
    while (cells_log2 < 62 && ((int64_t)1 << cells_log2) < (int64_t)h * w * taps) ++cells_log2;
    hipLaunchKernelGGL(fi_ctx_set_cells_log2<E>, dim3(1), dim3(1), 0, st, sc.dir[0].hdr, cells_log2);
    if (launch_status() != VFI_OK) return VFI_ERR_LAUNCH;
    if constexpr (F32) {                                    // (a bfloat16 call's fp32 scatter goes into the zeroed scratch)
        err = gradacc_zero_fp32(st, sc.dir[0].hdr, gradinput1, batch, channel, h, w, s1);
        if (err != VFI_OK) return err;
    }
    static_assert(VFI_TX == CB_TW && CB_TH % VFI_TY == 0, "fi_ctx_backward_px's blocks nest in the staged kernel's tiles");
    // channel groups: a workgroup repeats the tile's prologue (flows, filter, bounding box) per group
    int groups = 1, ch_per_group = channel;
    if (staged) {
        // fewer than two rounds of the chip's workgroup slots (2 per CU): split the channels, whole passes per group
        const int slots = device_cu_count() * 2;
        while (groups < 8 && (int64_t)ntiles * groups < 2 * slots && channel / (groups * 2) >= 4 * CB_CH &&
               (int64_t)batch * groups * 2 <= 65535)
            groups *= 2;
        ch_per_group = ((channel + groups - 1) / groups + CB_CH - 1) / CB_CH * CB_CH;
        groups = (channel + ch_per_group - 1) / ch_per_group;
    }
    for (int l = 0; l < launches; ++l) {
        CbPtrs<E> ptr;
        const int nt = nflows - l * CB_NT < CB_NT ? nflows - l * CB_NT : CB_NT;
        for (int t = 0; t < CB_NT; ++t) {
            ptr.flow[t] = flows[l * CB_NT + (t < nt ? t : 0)];
            ptr.gout[t] = gradoutputs[l * CB_NT + (t < nt ? t : 0)];
        }
        int* flags = staged ? sc.flags + (int64_t)l * ntiles : nullptr;
        if (staged)
            hipLaunchKernelGGL(fi_ctx_backward4_lds<E>, dim3(tiles_x, tiles_y, batch * groups), dim3(CB_THREADS), 0, st, ptr, nt,
                               input3, sc.dir[0].acc, sc.dir[0].hdr, flags, channel, h, w, s2, s3, sg, groups, ch_per_group);
        hipLaunchKernelGGL(fi_ctx_backward_px<E>, pixel_grid(w, h, batch), dim3(VFI_TX, VFI_TY, 1), 0, st, ptr, nt, input3,
                           sc.dir[0].acc, sc.dir[0].hdr, flags, F32 ? reinterpret_cast<float*>(gradinput1) : nullptr, channel, h, w,
                           fs, s1, s2, s3, sg);
    }
    if (launch_status() != VFI_OK) return VFI_ERR_LAUNCH;
    if constexpr (F32) return gradacc_finish(st, sc.dir[0], gradinput1, batch, channel, h, w, s1, true);
    else return gradacc_finish_bf16(st, sc.dir[0], gradinput1, batch, channel, h, w, s1);
}

}  // namespace vfi
