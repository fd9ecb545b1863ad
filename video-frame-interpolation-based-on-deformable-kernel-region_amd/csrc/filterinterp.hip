// filterinterp.hip -- adaptive-warping layer (FilterInterpolation) for gfx950.
//
// Semantics: filterinterpolation_cuda_kernel.cu:2692-2823 (_ori forward),
// :2827-3125 (_ori backward), :29-426 / :1353-1496 / :2070-2191 (deformable
// forwards) of the reference; entry points replace filterinterpolation_cuda.cc.
//
// This file holds the direct-gather kernels: one thread per output pixel, a
// wave covers 64 consecutive x so flow / filter / output planes move as full
// 256-B rows; flow, the blend weights and (fs == 4) all 16 filter taps live in
// registers across the channel loop (the reference re-fetches them per channel).
// The LDS-staged forward for fs == 4 lives in filterinterp_lds.hip and falls
// back to the kernel here when a tile's tap window does not fit its LDS budget.
#include "filterinterp_dev.h"
#include "filterinterp_paths.h"
#include "gradacc.h"

#include <limits.h>

namespace vfi {

FiSplit fi_channel_split(int ntiles, int channel, double prologue) {
    const int slots = device_cu_count() * 2;
    int best = 1;
    double best_cost = 0.0;
    for (int g = 1; g <= 8 && g <= channel; ++g) {
        const double r = (double)ntiles * g / slots;
        const double cost = (channel + prologue * g) * ((r + 0.5) / r) * (1.0 + 0.25 / r);
        if (g == 1 || cost < best_cost) { best_cost = cost; best = g; }
    }
    const int ch_per_group = (channel + best - 1) / best;
    return FiSplit{ch_per_group, (channel + ch_per_group - 1) / ch_per_group};
}

// ------------------------------------------------------------------ forward, _ori

// DST = vfi_strides (fi_dst, filterinterp_dev.h): out is addressed with so's batch and channel strides; no DST: with s1's
template <bool FS4, class... DST>
__global__ __launch_bounds__(VFI_TX * VFI_TY) void fi_forward_ori_direct(
    const float* __restrict__ in1, const float* __restrict__ in2, const float* __restrict__ in3,
    float* __restrict__ out, int channel, int h, int w, int fs,
    vfi_strides s1, vfi_strides s2, vfi_strides s3, DST... so) {
    constexpr bool TO = sizeof...(DST) != 0;
    const int64_t ob = fi_dst(s1, so...).b, oc = fi_dst(s1, so...).c;
    const int x = blockIdx.x * VFI_TX + threadIdx.x;
    const int y = blockIdx.y * VFI_TY + threadIdx.y;
    if (x >= w || y >= h) return;
    const int b = blockIdx.z;
    const FiFlow fl = fi_flow_at(in2, s2, b, x, y);
    const float fx = fl.fx, fy = fl.fy;
    const float x2 = (float)x + fx;
    const float y2 = (float)y + fy;
    const float* img = in1 + (int64_t)b * s1.b;
    float* dst = out + (int64_t)b * ob + (int64_t)y * s1.h + x;
    if (!fi_valid(fx, fy, x2, y2, w, h)) {                  // (fi_point changes this kernel's code)
        fi_copy_through_to<TO>(img + (int64_t)y * s1.h + x, dst, 0, channel, s1.c, oc);
        return;
    }
    const FiGeom g = fi_cell(FiPoint{true, x2, y2});
    const int ix = g.ix, iy = g.iy;
    const int L = ix + 1 - fs / 2, T = iy + 1 - fs / 2;
    const float alpha = g.alpha, beta = g.beta;
    const float* fpx = in3 + (int64_t)b * s3.b + (int64_t)y * s3.h + x;
    if constexpr (FS4) {
        // fs == 4: every quadrant is 2x2; taps, clamped rows and columns hoisted out of the channel loop
        float f[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) f[k] = fpx[(int64_t)k * s3.c];
        fi4_channels_direct<TO>(img, dst, 0, channel, s1.c, oc, (int)s1.h, h, w, L, T, f, alpha, beta);
    } else {
        for (int c = 0; c < channel; ++c) {
            float q[4];
            quadrants_generic(img + (int64_t)c * s1.c, fpx, s3.c, (int)s1.h, h, w, fs, L, T, ix, iy, q);
            dst[(int64_t)c * oc] = blend4(alpha, beta, q[0], q[1], q[2], q[3]);
        }
    }
}

// ------------------------------------------------------------------ backward, _ori

// tile of fi_backward_ori4_lds (below)
#define FB_TW 64
#ifndef FB_TH
#define FB_TH 8
#endif
#ifndef FB_WAVES
#define FB_WAVES 4                                  // (launch bound: waves per SIMD the kernel must fit -- two workgroups per CU)
#endif
#define FB_THREADS (FB_TW * FB_TH)
#define FB_CH 3                                     // channels summed per pass
#define FB_CELLS 6144                               // 64-bit gradient cells per pass (49,152 bytes); half as many bytes of image windows
// what the launch bound promises must also hold for the LDS array: FB_WAVES waves per SIMD = FB_WAVES * 256 / FB_THREADS
// workgroups per CU, each with (2 + 1.5 FB_CELLS) * 8 bytes of the CU's 160 KB (a build that overrides FB_TH or FB_WAVES
// would otherwise keep compiling and silently lose occupancy)
static_assert(FB_THREADS <= 1024 && FB_THREADS % 64 == 0, "workgroup size");
static_assert(((FB_WAVES * 256) / FB_THREADS) * (2 + FB_CELLS + FB_CELLS / 2) * 8 <= 160 * 1024, "workgroups per CU x LDS per workgroup exceed the CU's LDS");

// Where the two kernels below read their incoming gradient and which outputs they write.  vfi_filterinterp_backward_ori: one
// tensor (GradPlain), every output requested and zero-filled by the caller.  vfi_filterinterp_blend_backward (BLEND): the two
// terms of a direction's gradient (GradTerms: g = grad_blend * w + grad_out, formed where the tensor is read), any output
// may be NULL, and requested outputs are written in full -- zeros where a pixel has no gradient, filter-gradient sums that
// start from 0 instead of the caller's cells (the same bits: the caller's cells are +0).  WANT_X = false: no image
// gradient -- no LDS cells, no 64-bit atomics, no fixed-point header.

// one direction of the blend backward (grid z = direction * batch + b)
struct FiBwdSide {
    const float* ref;
    const float* flow;
    const float* filt;
    GradTerms g;
    unsigned long long* acc;                                // this direction's dense fixed-point sums and header
    const int* hdr;
    float* gref;
    float* gflow;
    float* gfilt;
};
struct FiBwdPair { FiBwdSide d[2]; };

// flow / filter gradient of a pixel with none (BLEND: outputs are written in full)
__device__ __forceinline__ void fi_bwd_zero_px(float* gf, int64_t s2c, float* gfpx, int64_t s3c, int fs2) {
    if (gf) { gf[0] = 0.0f; gf[s2c] = 0.0f; }
    if (gfpx) for (int k = 0; k < fs2; ++k) gfpx[(int64_t)k * s3c] = 0.0f;
}

// one thread per pixel, any filter size; b: the image, zb: blockIdx.z (the flags' plane); sg: the incoming gradient's strides
template <class G, bool BLEND, bool WANT_X>
__device__ __forceinline__ void fi_backward_ori_px(
    const float* __restrict__ in1, const float* __restrict__ in2, const float* __restrict__ in3, G gsrc,
    unsigned long long* __restrict__ acc, const int* __restrict__ hdr, float* g1, float* g2, float* g3,
    int channel, int h, int w, int fs, vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides sg,
    const int* __restrict__ tileflag, int b, int zb, int fc = 0) {
    const int x = blockIdx.x * VFI_TX + threadIdx.x;
    const int y = blockIdx.y * VFI_TY + threadIdx.y;
    if (x >= w || y >= h) return;
    // (after fi_backward_ori4_lds: only the tiles that kernel left alone; VFI_TX x VFI_TY blocks nest in them)
    if (tileflag && !tileflag[(zb * ((h + FB_TH - 1) / FB_TH) + y / FB_TH) * gridDim.x + blockIdx.x]) return;
    const bool wx = WANT_X && (!BLEND || g1 != nullptr);   // (uniform: this direction's image gradient is wanted)
    const GradAccCtx gctx = wx ? gradacc_ctx(hdr) : GradAccCtx{1.0f, 1.0f, false};
    const FiFlow fl = fi_flow_at(in2, s2, b, x, y);
    const float fx = fl.fx, fy = fl.fy;
    const float x2 = (float)x + fx;
    const float y2 = (float)y + fy;
    float* gfpx = (!BLEND || g3) ? g3 + (int64_t)b * s3.b + (int64_t)y * s3.h + x : nullptr;
    if constexpr (BLEND) {
        float* gf0 = g2 ? g2 + (int64_t)b * s2.b + (int64_t)y * s2.h + x : nullptr;
        if (!gsrc.any() || !fi_valid(fx, fy, x2, y2, w, h)) {       // (fi_point changes this kernel's code)
            fi_bwd_zero_px(gf0, s2.c, gfpx, s3.c, fc);
            return;
        }
        if (gfpx) for (int k = 0; k < fc; ++k) gfpx[(int64_t)k * s3.c] = 0.0f;     // (every filter channel, taps or not)
    }
    if (!fi_valid(fx, fy, x2, y2, w, h)) return;           // no gradient (:2863-2864)
    const FiGeom g = fi_cell(FiPoint{true, x2, y2});
    const int ix = g.ix, iy = g.iy;
    const int L = ix + 1 - fs / 2, T = iy + 1 - fs / 2;
    const int R = L + fs, Bm = T + fs;
    const float alpha = g.alpha, beta = g.beta;
    const float* img = in1 + (int64_t)b * s1.b;
    unsigned long long* gimg = acc + (int64_t)b * channel * h * w;       // dense [b][c][y][x] fixed-point sums
    const float* fpx = in3 + (int64_t)b * s3.b + (int64_t)y * s3.h + x;
    const auto gpx = gsrc.row((int64_t)b * sg.b + (int64_t)y * sg.h + x);
    float gx = 0.0f, gy = 0.0f;
    for (int c = 0; c < channel; ++c) {
        const float* p = img + (int64_t)c * s1.c;
        unsigned long long* gp = gimg + (int64_t)c * h * w;
        float* gfp = g1 + (int64_t)b * s1.b + (int64_t)c * s1.c;    // (the fp32 scatter of a call with non-finite inputs)
        const float g = gpx[(int64_t)c * sg.c];
        const float qg[4] = { g * (1.0f - alpha) * (1.0f - beta), g * alpha * (1.0f - beta),
                              g * (1.0f - alpha) * beta,          g * alpha * beta };
        float q[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        for (int quad = 0; quad < 4; ++quad) {
            const int j0 = (quad < 2) ? T : iy + 1, j1 = (quad < 2) ? iy : Bm - 1;
            const int i0 = (quad & 1) ? ix + 1 : L, i1 = (quad & 1) ? R - 1 : ix;
            float acc = 0.0f;
            for (int j = j0; j <= j1; ++j) {
                const int64_t ro = (int64_t)clampi(j, 0, h - 1) * s1.h;
                for (int i = i0; i <= i1; ++i) {
                    const int64_t o = ro + clampi(i, 0, w - 1);
                    const int64_t k = (int64_t)((j - T) * fs + (i - L)) * s3.c;
                    const float pv = p[o], fv = fpx[k];
                    // image gradient: other pixels hit the same cell -> order-free fixed-point atomic (gradacc.h).
                    // The filter gradient cell belongs to this thread alone (index is this pixel's own), so a plain
                    // read-modify-write is equivalent to the reference's atomicAdd.
                    if (wx) gradacc_add(gp, gfp, (int64_t)clampi(j, 0, h - 1) * w + clampi(i, 0, w - 1), o, qg[quad] * fv, gctx);
                    if (!BLEND || gfpx) gfpx[k] += qg[quad] * pv;
                    acc = fmaf(pv, fv, acc);
                }
            }
            q[quad] = acc;
        }
        {   // flow gradient by quadrant differences (:2965-3102)
            const float gamma = 1.0f - beta;
            float temp = gamma * (q[1] - q[0]);
            temp = fmaf(1.0f - gamma, q[3] - q[2], temp);
            gx = fmaf(g, temp, gx);
        }
        {
            const float gamma = 1.0f - alpha;
            float temp = gamma * (q[2] - q[0]);
            temp = fmaf(1.0f - gamma, q[3] - q[1], temp);
            gy = fmaf(g, temp, gy);
        }
    }
    if (!BLEND || g2) {
        float* gf = g2 + (int64_t)b * s2.b + (int64_t)y * s2.h + x;
        gf[0] = gx;
        gf[s2.c] = gy;
    }
}

__global__ __launch_bounds__(VFI_TX * VFI_TY) void fi_backward_ori(
    const float* __restrict__ in1, const float* __restrict__ in2, const float* __restrict__ in3,
    const float* __restrict__ gout, unsigned long long* __restrict__ acc, const int* __restrict__ hdr, float* g1, float* g2, float* g3,
    int channel, int h, int w, int fs, vfi_strides s1, vfi_strides s2, vfi_strides s3, const int* __restrict__ tileflag) {
    fi_backward_ori_px<GradPlain, false, true>(in1, in2, in3, GradPlain{gout}, acc, hdr, g1, g2, g3, channel, h, w, fs, s1, s2, s3,
                                               s1, tileflag, blockIdx.z, blockIdx.z);
}

// fs == 4, image values and image gradient through LDS (round 3).  The per-tap kernel above gathers 16 image values per
// pixel and channel from global memory and scatters 16 global 64-bit atomics (110 M of them at 1080p, C = 3).  Here a
// workgroup owns a 64x8 tile and works through the channels three at a time.  The taps of `_ori` are undisplaced, so the
// bounding box of the tile's (clamped) taps is both the window of image values it reads and the window of gradient cells
// it writes: the three planes' windows are staged by LDS-DMA, the addends -- exact integers, summable in any grouping --
// are added to 64-bit cells in LDS, and each non-zero cell leaves with ONE global atomic ((64 + 12) x (8 + 12) cells
// instead of 512 x 16 addends per tile and channel).  Taps outside, the pass's channels inside; the 16 filter taps and
// the 16 filter-gradient sums of the pixel live in registers (the per-tap kernel re-reads the taps and read-modify-writes
// the gradient cells in global memory once per channel and tap).  Every sum keeps the per-tap kernel's order and starting
// value: its bits.  A call with non-finite inputs (fp32 atomics: gradacc.h) and a tile whose window does not fit are
// flagged, and fi_backward_ori, launched after this kernel, does those tiles only.  A tile with a large window takes two
// channels, or one, per pass.  Without the image gradient (WANT_X = false) the LDS holds the windows only; the channels per
// pass stay those of the window budget (at C = 3 one pass covers every channel either way).
template <class G, bool BLEND, bool WANT_X>
__device__ __forceinline__ void fi_backward_ori4_tile(
    const float* __restrict__ in1, const float* __restrict__ in2, const float* __restrict__ in3, G gsrc,
    unsigned long long* __restrict__ acc, const int* __restrict__ hdr, int* __restrict__ tileflag, float* g1,
    float* g2, float* g3, int channel, int h, int w, vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides sg, int b) {
    constexpr int fs = 4;
    constexpr int NCELLS = WANT_X ? FB_CELLS : 0;
    // channels per pass at most: the blend's instance with the image gradient holds two more 64-bit row pointers per pixel and
    // spilled to scratch at the launch bound with three (72 B/lane) or two (20 B/lane); with one it needs 108 VGPRs and none.
    // Every sum runs channel by channel whatever the pass size: the same bits.
    constexpr int CH = (BLEND && WANT_X) ? 1 : FB_CH;
    // one array: header (bounding box), gradient cells, image windows -- FB_CELLS of each for a pass
    __shared__ __attribute__((aligned(16))) unsigned long long lds64[2 + NCELLS + FB_CELLS / 2];
    int* box = reinterpret_cast<int*>(lds64);
    unsigned long long* cells = lds64 + 2;
    float* wins = reinterpret_cast<float*>(lds64 + 2 + NCELLS);
    const int tid = threadIdx.x;
    const int x = blockIdx.x * FB_TW + (tid & (FB_TW - 1));
    const int y = blockIdx.y * FB_TH + (tid >> 6);
    const bool wx = WANT_X && (!BLEND || g1 != nullptr);   // (uniform: this direction's image gradient is wanted)
    const GradAccCtx gctx = wx ? gradacc_ctx(hdr) : GradAccCtx{1.0f, 1.0f, false};
    const bool inimg = x < w && y < h;
    const FiFlow fl = fi_flow_at(in2, s2, b, x, y, inimg);
    // (written out: fi_geom changes the blend instances of this kernel)
    const float fx = fl.fx, fy = fl.fy;
    const float x2 = (float)x + fx;
    const float y2 = (float)y + fy;
    const bool valid = inimg && gsrc.any() && fi_valid(fx, fy, x2, y2, w, h);     // an invalid pixel has no gradient (:2863-2864)
    if constexpr (BLEND) {
        if (inimg && !valid)
            fi_bwd_zero_px(g2 ? g2 + (int64_t)b * s2.b + (int64_t)y * s2.h + x : nullptr, s2.c,
                           g3 ? g3 + (int64_t)b * s3.b + (int64_t)y * s3.h + x : nullptr, s3.c, 16);
    }
    const int ix = valid ? (int)x2 : 0, iy = valid ? (int)y2 : 0;
    const int L = ix - 1, T = iy - 1;
    const float alpha = x2 - (float)ix;
    const float beta = y2 - (float)iy;
    int ro[4], co[4];                                       // clamped rows and columns of the pixel's window
#pragma unroll
    for (int k = 0; k < 4; ++k) { ro[k] = clampi(T + k, 0, h - 1); co[k] = clampi(L + k, 0, w - 1); }
    // ---- bounding box of the tile's (clamped) taps
    if (tid == 0) { box[0] = INT_MAX; box[1] = INT_MAX; box[2] = INT_MIN; box[3] = INT_MIN; }
    __syncthreads();
    {
        const int wx0 = wave_min_i32(valid ? co[0] : INT_MAX), wy0 = wave_min_i32(valid ? ro[0] : INT_MAX);
        const int wx1 = wave_max_i32(valid ? co[3] : INT_MIN), wy1 = wave_max_i32(valid ? ro[3] : INT_MIN);
        if ((tid & 63) == 0 && wx0 != INT_MAX) {
            atomicMin(&box[0], wx0); atomicMin(&box[1], wy0);
            atomicMax(&box[2], wx1); atomicMax(&box[3], wy1);
        }
    }
    __syncthreads();
    if (box[0] == INT_MAX) return;                          // (workgroup-uniform: nothing in this tile has a gradient)
    const int bx0 = box[0], by0 = box[1], bw = box[2] - box[0] + 1, bh = box[3] - box[1] + 1;
    const int n = bw * bh;
    const int hs = (int)s1.h;
    // channels per pass: as many (at most CH) as fit the cells and the window slots -- a slot is the window rounded up to
    // whole DMA instructions, so that a window's last instruction stays inside its slot
    const int slot_floats = (n + FB_THREADS - 1) & ~(FB_THREADS - 1);
    const int pc = min(CH, FB_CELLS / slot_floats);
    if ((wx && !gradacc_staged_ok(gctx)) || pc == 0 || (int64_t)h * hs * 4 > INT_MAX) {     // (workgroup-uniform) left to fi_backward_ori
        if (tid == 0) tileflag[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = 1;
        return;
    }

    const float* img = in1 + (int64_t)b * s1.b;
    unsigned long long* gimg = acc + (int64_t)b * channel * h * w;       // dense [b][c][y][x] fixed-point sums
    const float* fpx = in3 + (int64_t)b * s3.b + (int64_t)y * s3.h + x;
    float* gfpx = g3 + (int64_t)b * s3.b + (int64_t)y * s3.h + x;
    const auto gpx = gsrc.row((int64_t)b * sg.b + (int64_t)y * sg.h + x);
    float fv[16], gf16[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        fv[k] = valid ? fpx[(int64_t)k * s3.c] : 0.0f;
        gf16[k] = (valid && !BLEND) ? gfpx[(int64_t)k * s3.c] : 0.0f;
    }
    int lrow[4];                                            // the window rows' first cells, less the box's first column
#pragma unroll
    for (int k = 0; k < 4; ++k) lrow[k] = (ro[k] - by0) * bw - bx0;
    const int plane_bytes = 4 * ((h - 1) * hs + w);
    const float inv_bw = 1.0f / (float)bw;
    const int wave_first = __builtin_amdgcn_readfirstlane(tid >> 6) * 64;
    float gx = 0.0f, gy = 0.0f;
    for (int c0 = 0; c0 < channel; c0 += pc) {
        const int cn = min(pc, channel - c0);
        // ---- stage the pass's windows (element e of a window = cell e: row-major, bw per row, all inside the image), zero the
        // cells, fetch gradoutput
        for (int cc = 0; cc < cn; ++cc) {
            const auto plane = buffer_rsrc(img + (int64_t)(c0 + cc) * s1.c, plane_bytes);
            float* slot = wins + cc * slot_floats + wave_first;
            for (int e0 = 0; e0 < n; e0 += FB_THREADS) {
                const int e = e0 + tid;
                const int r = fi_row_of(e, inv_bw);
                const int col = e - r * bw;
                // (lanes past the window get an out-of-range offset: they write zeros, inside the window's own slot)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(plane, (lds_ptr_t)(slot + e0), 4, e < n ? 4u * (unsigned)((by0 + r) * hs + bx0 + col) : 0x80000000u, 0, 0, 0);
            }
        }
        if (wx) for (int e = tid; e < n * cn; e += FB_THREADS) cells[e] = 0ull;
        float gv[CH];
#pragma unroll
        for (int cc = 0; cc < CH; ++cc) gv[cc] = (valid && cc < cn) ? gpx[(int64_t)(c0 + cc) * sg.c] : 0.0f;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (valid) {
            float qg[CH][4], q[CH][4];
#pragma unroll
            for (int cc = 0; cc < CH; ++cc) {
                const float g = gv[cc];
                qg[cc][0] = g * (1.0f - alpha) * (1.0f - beta); qg[cc][1] = g * alpha * (1.0f - beta);
                qg[cc][2] = g * (1.0f - alpha) * beta;          qg[cc][3] = g * alpha * beta;
                q[cc][0] = q[cc][1] = q[cc][2] = q[cc][3] = 0.0f;
            }
            // taps in the per-tap kernel's order (quadrant by quadrant), the pass's channels inside
#pragma unroll
            for (int quad = 0; quad < 4; ++quad)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                    for (int ii = 0; ii < 2; ++ii) {
                        const int j = (quad >> 1) * 2 + jj, i = (quad & 1) * 2 + ii, k = j * fs + i;
                        const int cell = lrow[j] + co[i];
#pragma unroll
                        for (int cc = 0; cc < CH; ++cc) {
                            if (cc < cn) {                  // (workgroup-uniform)
                                const float pv = wins[cc * slot_floats + cell];
                                if (wx) atomicAdd(&cells[cc * n + cell], (unsigned long long)__float2ll_rn(qg[cc][quad] * fv[k] * gctx.scale));
                                gf16[k] += qg[cc][quad] * pv;
                                q[cc][quad] = fmaf(pv, fv[k], q[cc][quad]);
                            }
                        }
                    }
#pragma unroll
            for (int cc = 0; cc < CH; ++cc) {
                if (cc < cn) {
                    const float g = gv[cc];
                    {   // flow gradient by quadrant differences (:2965-3102)
                        const float gamma = 1.0f - beta;
                        float temp = gamma * (q[cc][1] - q[cc][0]);
                        temp = fmaf(1.0f - gamma, q[cc][3] - q[cc][2], temp);
                        gx = fmaf(g, temp, gx);
                    }
                    {
                        const float gamma = 1.0f - alpha;
                        float temp = gamma * (q[cc][2] - q[cc][0]);
                        temp = fmaf(1.0f - gamma, q[cc][3] - q[cc][1], temp);
                        gy = fmaf(g, temp, gy);
                    }
                }
            }
        }
        __syncthreads();
        if (wx) {
            for (int e = tid; e < n * cn; e += FB_THREADS) {
                const unsigned long long v = cells[e];
                if (v != 0ull) {
                    const int cc = e / n, r = e - cc * n;
                    const int cy = r / bw, cx = r - cy * bw;
                    atomicAdd(&gimg[(int64_t)(c0 + cc) * h * w + (int64_t)(by0 + cy) * w + bx0 + cx], v);
                }
            }
            __syncthreads();                                // (the next pass overwrites windows and cells)
        }
    }
    if (valid) {
        if (!BLEND || g3) {
#pragma unroll
            for (int k = 0; k < 16; ++k) gfpx[(int64_t)k * s3.c] = gf16[k];
        }
        if (!BLEND || g2) {
            float* gf = g2 + (int64_t)b * s2.b + (int64_t)y * s2.h + x;
            gf[0] = gx;
            gf[s2.c] = gy;
        }
    }
}

__global__ __launch_bounds__(FB_THREADS, FB_WAVES) void fi_backward_ori4_lds(
    const float* __restrict__ in1, const float* __restrict__ in2, const float* __restrict__ in3,
    const float* __restrict__ gout, unsigned long long* __restrict__ acc, const int* __restrict__ hdr, int* __restrict__ tileflag,
    float* g2, float* g3, int channel, int h, int w, vfi_strides s1, vfi_strides s2, vfi_strides s3) {
    fi_backward_ori4_tile<GradPlain, false, true>(in1, in2, in3, GradPlain{gout}, acc, hdr, tileflag, nullptr, g2, g3, channel, h,
                                                  w, s1, s2, s3, s1, blockIdx.z);
}

// vfi_filterinterp_blend_backward: both directions in one launch (grid z = direction * batch + b), on the bodies above.
// Refs and their gradients use s1, flows s2, filters s3, the gradient terms sg.
template <bool WANT_X>
__global__ __launch_bounds__(FB_THREADS, FB_WAVES) void fi_blend_backward4_lds(
    FiBwdPair pr, int* __restrict__ tileflag, int batch, int channel, int h, int w,
    vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides sg) {
    const int dir = (int)blockIdx.z >= batch;
    const FiBwdSide& d = dir ? pr.d[1] : pr.d[0];
    fi_backward_ori4_tile<GradTerms, true, WANT_X>(d.ref, d.flow, d.filt, d.g, d.acc, d.hdr, tileflag, d.gref, d.gflow, d.gfilt,
                                                   channel, h, w, s1, s2, s3, sg, (int)blockIdx.z - dir * batch);
}

template <bool WANT_X>
__global__ __launch_bounds__(VFI_TX * VFI_TY) void fi_blend_backward_general(
    FiBwdPair pr, const int* __restrict__ tileflag, int batch, int channel, int h, int w, int fs, int fc,
    vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides sg) {
    const int dir = (int)blockIdx.z >= batch;
    const FiBwdSide& d = dir ? pr.d[1] : pr.d[0];
    fi_backward_ori_px<GradTerms, true, WANT_X>(d.ref, d.flow, d.filt, d.g, d.acc, d.hdr, d.gref, d.gflow, d.gfilt, channel, h, w,
                                                fs, s1, s2, s3, sg, tileflag, (int)blockIdx.z - dir * batch, blockIdx.z, fc);
}

// ------------------------------------------------------------------ forward, deformable variants

// bilinear sample at (clamped tap + learned offset) (:98-111); the four corner
// indices are clamped to the image (the reference leaves them unclamped: UB there)
__device__ __forceinline__ float defor_tap(const float* __restrict__ p, int hs, int h, int w, float fracY, float fracX) {
    const int Top = (int)fracY, Left = (int)fracX;
    const float phiY = fracY - (float)Top;
    const float phiX = fracX - (float)Left;
    const float PTL = (1.0f - phiX) * (1.0f - phiY);
    const float PTR = phiX * (1.0f - phiY);
    const float PBL = (1.0f - phiX) * phiY;
    const float PBR = phiY * phiX;
    const int64_t t = (int64_t)clampi(Top, 0, h - 1) * hs, bo = (int64_t)clampi(Top + 1, 0, h - 1) * hs;
    const int l = clampi(Left, 0, w - 1), r = clampi(Left + 1, 0, w - 1);
    float s = PTL * p[t + l];
    s = fmaf(PTR, p[t + r], s);
    s = fmaf(PBL, p[bo + l], s);
    s = fmaf(PBR, p[bo + r], s);
    return s;
}

template <int VARIANT>
__global__ __launch_bounds__(VFI_TX * VFI_TY) void fi_forward_defor(
    const float* __restrict__ in1, const float* __restrict__ in2, const float* __restrict__ in3,
    const float* __restrict__ in4, float* __restrict__ out, int channel, int h, int w, int fs,
    vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides s4) {
    const int x = blockIdx.x * VFI_TX + threadIdx.x;
    const int y = blockIdx.y * VFI_TY + threadIdx.y;
    if (x >= w || y >= h) return;
    const int b = blockIdx.z;
    const FiFlow fl = fi_flow_at(in2, s2, b, x, y);
    const float fx = fl.fx, fy = fl.fy;
    const float x2 = (float)x + fx;
    const float y2 = (float)y + fy;
    const float* img = in1 + (int64_t)b * s1.b;
    float* dst = out + (int64_t)b * s1.b + (int64_t)y * s1.h + x;
    if (!fi_valid(fx, fy, x2, y2, w, h)) {                  // (fi_point changes this kernel's code)
        const float* src = img + (int64_t)y * s1.h + x;
        for (int c = 0; c < channel; ++c) dst[(int64_t)c * s1.c] = src[(int64_t)c * s1.c];
        return;
    }
    const int fs2 = fs * fs;
    const FiGeom g = fi_cell(FiPoint{true, x2, y2});
    const int ix = g.ix, iy = g.iy;
    const int L = ix + 1 - fs / 2, T = iy + 1 - fs / 2;
    const int R = L + fs, Bm = T + fs;
    const float alpha = g.alpha, beta = g.beta;
    // VARIANT 2: the third input IS the offset field, there are no filter weights
    const float* fpx = in3 + (int64_t)b * s3.b + (int64_t)y * s3.h + x;
    const float* opx = (VARIANT == VFI_DEFOR_NOFILTER) ? fpx : in4 + (int64_t)b * s4.b + (int64_t)y * s4.h + x;
    const int64_t ocs = (VARIANT == VFI_DEFOR_NOFILTER) ? s3.c : s4.c;
    for (int c = 0; c < channel; ++c) {
        const float* p = img + (int64_t)c * s1.c;
        float TL = 0.0f, TR = 0.0f, BL = 0.0f, BR = 0.0f;
        if constexpr (VARIANT == VFI_DEFOR_OFFSET) {
            for (int quad = 0; quad < 4; ++quad) {
                const int j0 = (quad < 2) ? T : iy + 1, j1 = (quad < 2) ? iy : Bm - 1;
                const int i0 = (quad & 1) ? ix + 1 : L, i1 = (quad & 1) ? R - 1 : ix;
                float acc = 0.0f;
                for (int j = j0; j <= j1; ++j) {
                    const int cj = clampi(j, 0, h - 1);
                    for (int i = i0; i <= i1; ++i) {
                        const int ci = clampi(i, 0, w - 1);
                        const int k = (j - T) * fs + (i - L);
                        const float fracY = (float)cj + opx[(int64_t)k * ocs];
                        const float fracX = (float)ci + opx[(int64_t)(fs2 + k) * ocs];
                        acc = fmaf(defor_tap(p, (int)s1.h, h, w, fracY, fracX), fpx[(int64_t)k * s3.c], acc);
                    }
                }
                if (quad == 0) TL = acc; else if (quad == 1) TR = acc; else if (quad == 2) BL = acc; else BR = acc;
            }
        } else {
            for (int j = T; j < Bm; ++j) {
                const int cj = clampi(j, 0, h - 1);
                for (int i = L; i < R; ++i) {
                    const int ci = clampi(i, 0, w - 1);
                    const int k = (j - T) * fs + (i - L);
                    const float fracY = (float)cj + opx[(int64_t)k * ocs];
                    const float fracX = (float)ci + opx[(int64_t)(fs2 + k) * ocs];
                    const float v = defor_tap(p, (int)s1.h, h, w, fracY, fracX);
                    if constexpr (VARIANT == VFI_DEFOR_NOFILTER) {
                        if (fracX <= x2 && fracY <= y2) TL = TL + v;
                        if (fracX >  x2 && fracY <= y2) TR = TR + v;
                        if (fracX <= x2 && fracY >  y2) BL = BL + v;
                        if (fracX >  x2 && fracY >  y2) BR = BR + v;
                    } else {
                        const float wgt = fpx[(int64_t)k * s3.c];
                        if (fracX <= x2 && fracY <= y2) TL = fmaf(v, wgt, TL);
                        if (fracX >  x2 && fracY <= y2) TR = fmaf(v, wgt, TR);
                        if (fracX <= x2 && fracY >  y2) BL = fmaf(v, wgt, BL);
                        if (fracX >  x2 && fracY >  y2) BR = fmaf(v, wgt, BR);
                    }
                }
            }
        }
        dst[(int64_t)c * s1.c] = blend4(alpha, beta, TL, TR, BL, BR);
    }
}

// ------------------------------------------------------------------ backward, deformable variants

// filterinterpolation_cuda_kernel.cu:430-1215 (VARIANT 0), :1500-1935 (1), :2195-2567 (2).  Per valid
// pixel and tap: quadrant weight by integer index (0) or displaced position (1, 2); image gradient
// scattered to the clamped UNDISPLACED tap (the reference's own approximation) with atomics; filter
// and offset-field gradients belong to this pixel alone (plain read-modify-write, the same values as
// the reference's atomicAdd); flow gradient from the forward's quadrant sums.
// STAGED (round 3): the image-gradient addends of a 64x4 block are summed in a window of 64-bit LDS cells over the bounding
// box of the block's clamped taps, three channels at a time, and leave with one global atomic per non-zero cell (exact
// integer sums: the same bits as the per-tap scatter; see fi_backward_ori4_lds).  A block whose window does not fit, and
// every block of a call with non-finite inputs, raises its flag and returns; the !STAGED instance, launched afterwards with
// the flags, does those blocks only.
#define FD_CH 3
#define FD_CELLS 4608                               // 64-bit cells of LDS (36,864 bytes)
// FS = 4: the filter size at compile time -- offsets, weights and the filter / offset gradient sums of the pixel live in
// registers across the channel loop (summed in the same order from the cells' starting values: the same bits); FS = 0: any
// filter size, the cells are read and written in global memory per channel and tap.
template <int VARIANT, bool STAGED, int FS>
__global__ __launch_bounds__(VFI_TX * VFI_TY) void fi_backward_defor(
    const float* __restrict__ in1, const float* __restrict__ in2, const float* __restrict__ in3,
    const float* __restrict__ in4, const float* __restrict__ gout, unsigned long long* __restrict__ acc,
    const int* __restrict__ hdr, int* __restrict__ tileflag, float* g1, float* g2, float* g3, float* g4,
    int channel, int h, int w, int fs_arg, vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides s4) {
    const int fs = FS ? FS : fs_arg;
    constexpr int NA = FS ? FS * FS : 1;
    __shared__ unsigned long long cells[STAGED ? FD_CELLS : 1];
    __shared__ int box[4];
    const int x = blockIdx.x * VFI_TX + threadIdx.x;
    const int y = blockIdx.y * VFI_TY + threadIdx.y;
    const int b = blockIdx.z;
    const int tile = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const int tid = threadIdx.y * VFI_TX + threadIdx.x;
    if constexpr (!STAGED) {
        if (tileflag && !tileflag[tile]) return;
        if (x >= w || y >= h) return;
    }
    const bool inimg = x < w && y < h;
    const GradAccCtx gctx = gradacc_ctx(hdr);
    // (written out: fi_geom changes every instance of this kernel)
    const FiFlow fl = fi_flow_at(in2, s2, b, x, y, inimg);
    const float fx = fl.fx, fy = fl.fy;
    const float x2 = (float)x + fx;
    const float y2 = (float)y + fy;
    const bool valid = inimg && fi_valid(fx, fy, x2, y2, w, h);
    if constexpr (!STAGED) { if (!valid) return; }
    const int fs2 = fs * fs;
    const int ix = valid ? (int)x2 : 0, iy = valid ? (int)y2 : 0;
    const int L = ix + 1 - fs / 2, T = iy + 1 - fs / 2;
    int bx0 = 0, by0 = 0, bw = 0, n = 0;
    if constexpr (STAGED) {
        if (tid == 0) { box[0] = INT_MAX; box[1] = INT_MAX; box[2] = INT_MIN; box[3] = INT_MIN; }
        __syncthreads();
        const int wx0 = wave_min_i32(valid ? clampi(L, 0, w - 1) : INT_MAX), wy0 = wave_min_i32(valid ? clampi(T, 0, h - 1) : INT_MAX);
        const int wx1 = wave_max_i32(valid ? clampi(L + fs - 1, 0, w - 1) : INT_MIN), wy1 = wave_max_i32(valid ? clampi(T + fs - 1, 0, h - 1) : INT_MIN);
        if ((tid & 63) == 0 && wx0 != INT_MAX) {
            atomicMin(&box[0], wx0); atomicMin(&box[1], wy0);
            atomicMax(&box[2], wx1); atomicMax(&box[3], wy1);
        }
        __syncthreads();
        if (box[0] == INT_MAX) return;                      // (block-uniform: no pixel of the block has a gradient)
        bx0 = box[0]; by0 = box[1]; bw = box[2] - box[0] + 1;
        n = bw * (box[3] - box[1] + 1);
        if (!gradacc_staged_ok(gctx) || n * min(FD_CH, channel) > FD_CELLS) {      // (block-uniform) left to the !STAGED instance
            if (tid == 0) tileflag[tile] = 1;
            return;
        }
    }
    const float alpha = x2 - (float)ix;
    const float beta = y2 - (float)iy;
    const float* img = in1 + (int64_t)b * s1.b;
    unsigned long long* gimg = acc + (int64_t)b * channel * h * w;       // dense [b][c][y][x] fixed-point sums
    const float* gpx = gout + (int64_t)b * s1.b + (int64_t)y * s1.h + x;
    // VARIANT 2: the third input IS the offset field and g3 its gradient; no filter
    const float* fpx = in3 + (int64_t)b * s3.b + (int64_t)y * s3.h + x;
    float* gfpx = g3 + (int64_t)b * s3.b + (int64_t)y * s3.h + x;
    const float* opx = (VARIANT == VFI_DEFOR_NOFILTER) ? fpx : in4 + (int64_t)b * s4.b + (int64_t)y * s4.h + x;
    float* gopx = (VARIANT == VFI_DEFOR_NOFILTER) ? gfpx : g4 + (int64_t)b * s4.b + (int64_t)y * s4.h + x;
    const int64_t ocs = (VARIANT == VFI_DEFOR_NOFILTER) ? s3.c : s4.c;
    const float kq[4] = { (1.0f - alpha) * (1.0f - beta), alpha * (1.0f - beta), (1.0f - alpha) * beta, alpha * beta };
    float offy[NA], offx[NA], wgts[NA], gfa[NA], goy[NA], gox[NA];
    if constexpr (FS != 0) {
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            offy[k] = valid ? opx[(int64_t)k * ocs] : 0.0f;
            offx[k] = valid ? opx[(int64_t)(fs2 + k) * ocs] : 0.0f;
            goy[k] = valid ? gopx[(int64_t)k * ocs] : 0.0f;
            gox[k] = valid ? gopx[(int64_t)(fs2 + k) * ocs] : 0.0f;
            if constexpr (VARIANT != VFI_DEFOR_NOFILTER) {
                wgts[k] = valid ? fpx[(int64_t)k * s3.c] : 0.0f;
                gfa[k] = valid ? gfpx[(int64_t)k * s3.c] : 0.0f;
            }
        }
    }
    float gx = 0.0f, gy = 0.0f;
    const int chunk = STAGED ? FD_CH : channel;
    for (int c0 = 0; c0 < channel; c0 += chunk) {
    const int cn = min(chunk, channel - c0);
    if constexpr (STAGED) {
        for (int e = tid; e < n * cn; e += VFI_TX * VFI_TY) cells[e] = 0ull;
        __syncthreads();
    }
    for (int c = c0; c < c0 + cn && valid; ++c) {
        const float* p = img + (int64_t)c * s1.c;
        unsigned long long* gp = gimg + (int64_t)c * h * w;
        unsigned long long* win = cells + (STAGED ? (c - c0) * n : 0);
        float* gfp = g1 + (int64_t)b * s1.b + (int64_t)c * s1.c;    // (the fp32 scatter of a call with non-finite inputs)
        const float g = gpx[(int64_t)c * s1.c];
        const float qg[4] = { g * (1.0f - alpha) * (1.0f - beta), g * alpha * (1.0f - beta),
                              g * (1.0f - alpha) * beta,          g * alpha * beta };
        float q[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int dj = 0; dj < fs; ++dj) {
            const int j = T + dj, cj = clampi(j, 0, h - 1);
#pragma unroll
            for (int di = 0; di < fs; ++di) {
                const int i = L + di, ci = clampi(i, 0, w - 1);
                const int k = dj * fs + di;
                const int ka = FS ? k : 0;
                const float fracY = (float)cj + (FS ? offy[ka] : opx[(int64_t)k * ocs]);
                const float fracX = (float)ci + (FS ? offx[ka] : opx[(int64_t)(fs2 + k) * ocs]);
                int quad;
                if constexpr (VARIANT == VFI_DEFOR_OFFSET) quad = (j > iy ? 2 : 0) + (i > ix ? 1 : 0);
                else if (fracX <= x2 && fracY <= y2) quad = 0;
                else if (fracX > x2 && fracY <= y2) quad = 1;
                else if (fracX <= x2 && fracY > y2) quad = 2;
                else if (fracX > x2 && fracY > y2) quad = 3;
                else continue;                                      // NaN position: no quadrant
                const int Top = (int)fracY, Left = (int)fracX;
                const float phiY = fracY - (float)Top, phiX = fracX - (float)Left;
                const int64_t t = (int64_t)clampi(Top, 0, h - 1) * s1.h, bo = (int64_t)clampi(Top + 1, 0, h - 1) * s1.h;
                const int l = clampi(Left, 0, w - 1), r = clampi(Left + 1, 0, w - 1);
                const float vTL = p[t + l], vTR = p[t + r], vBL = p[bo + l], vBR = p[bo + r];
                float v = ((1.0f - phiX) * (1.0f - phiY)) * vTL;
                v = fmaf(phiX * (1.0f - phiY), vTR, v);
                v = fmaf((1.0f - phiX) * phiY, vBL, v);
                v = fmaf(phiY * phiX, vBR, v);
                float dY = (-(1.0f - phiX)) * vTL;
                dY = fmaf(1.0f - phiX, vBL, dY);
                dY = fmaf(-phiX, vTR, dY);
                dY = fmaf(phiX, vBR, dY);
                float dX = (-(1.0f - phiY)) * vTL;
                dX = fmaf(1.0f - phiY, vTR, dX);
                dX = fmaf(-phiY, vBL, dX);
                dX = fmaf(phiY, vBR, dX);
                const int64_t o = (int64_t)cj * w + ci;
                if constexpr (VARIANT == VFI_DEFOR_NOFILTER) {
                    if constexpr (STAGED) atomicAdd(&win[(cj - by0) * bw + ci - bx0], (unsigned long long)__float2ll_rn(qg[quad] * gctx.scale));
                    else gradacc_add(gp, gfp, o, (int64_t)cj * s1.h + ci, qg[quad], gctx);
                    q[quad] = q[quad] + v;
                    if constexpr (FS != 0) {
                        goy[ka] += g * kq[quad] * dY;
                        gox[ka] += g * kq[quad] * dX;
                    } else {
                        gopx[(int64_t)k * ocs] += g * kq[quad] * dY;
                        gopx[(int64_t)(fs2 + k) * ocs] += g * kq[quad] * dX;
                    }
                } else {
                    const float wgt = FS ? wgts[ka] : fpx[(int64_t)k * s3.c];
                    if constexpr (STAGED) atomicAdd(&win[(cj - by0) * bw + ci - bx0], (unsigned long long)__float2ll_rn(qg[quad] * wgt * gctx.scale));
                    else gradacc_add(gp, gfp, o, (int64_t)cj * s1.h + ci, qg[quad] * wgt, gctx);
                    q[quad] = fmaf(v, wgt, q[quad]);
                    if constexpr (FS != 0) {
                        gfa[ka] += qg[quad] * v;
                        goy[ka] += g * kq[quad] * dY * wgt;
                        gox[ka] += g * kq[quad] * dX * wgt;
                    } else {
                        gfpx[(int64_t)k * s3.c] += qg[quad] * v;
                        gopx[(int64_t)k * ocs] += g * kq[quad] * dY * wgt;
                        gopx[(int64_t)(fs2 + k) * ocs] += g * kq[quad] * dX * wgt;
                    }
                }
            }
        }
        {
            const float gamma = 1.0f - beta;
            float temp = gamma * (q[1] - q[0]);
            temp = fmaf(1.0f - gamma, q[3] - q[2], temp);
            gx = fmaf(g, temp, gx);
        }
        {
            const float gamma = 1.0f - alpha;
            float temp = gamma * (q[2] - q[0]);
            temp = fmaf(1.0f - gamma, q[3] - q[1], temp);
            gy = fmaf(g, temp, gy);
        }
    }
    if constexpr (STAGED) {
        __syncthreads();
        for (int e = tid; e < n * cn; e += VFI_TX * VFI_TY) {
            const unsigned long long v = cells[e];
            if (v != 0ull) {
                const int cc = e / n, r = e - cc * n;
                const int cy = r / bw, cx = r - cy * bw;
                atomicAdd(&gimg[(int64_t)(c0 + cc) * h * w + (int64_t)(by0 + cy) * w + bx0 + cx], v);
            }
        }
        __syncthreads();                                    // (the next pass zeroes the cells)
    }
    }
    if (valid) {
        float* gf = g2 + (int64_t)b * s2.b + (int64_t)y * s2.h + x;
        gf[0] = gx;
        gf[s2.c] = gy;
        if constexpr (FS != 0) {
#pragma unroll
            for (int k = 0; k < NA; ++k) {
                gopx[(int64_t)k * ocs] = goy[k];
                gopx[(int64_t)(fs2 + k) * ocs] = gox[k];
                if constexpr (VARIANT != VFI_DEFOR_NOFILTER) gfpx[(int64_t)k * s3.c] = gfa[k];
            }
        }
    }
}

}  // namespace vfi

using namespace vfi;

int vfi::launch_fi_ori_direct(const float* input1, const float* input2, const float* input3, float* output, int batch,
                              int channel, int h, int w, int filter_channels, vfi_strides s1, vfi_strides s2, vfi_strides s3,
                              vfi_strides so, vfi_stream_t stream) {
    if (batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || filter_channels <= 0) return VFI_ERR_SHAPE;
    if (!input1 || !input2 || !input3 || !output) return VFI_ERR_SHAPE;
    if (so.h != s1.h) return VFI_ERR_SHAPE;                  // one in-plane offset per pixel for loads and stores
    const int fs = fi_filter_size(filter_channels);
    const dim3 grid = pixel_grid(w, h, batch), block(VFI_TX, VFI_TY, 1);
    hipStream_t st = (hipStream_t)stream;
    const bool to = so.b != s1.b || so.c != s1.c;           // (a destination laid out as input1: the instances without a second set of strides)
#define FI_LAUNCH(KERNEL, ...) hipLaunchKernelGGL(KERNEL, grid, block, 0, st, input1, input2, input3, output, \
        channel, h, w, fs, s1, s2, s3, ##__VA_ARGS__)
    if (fs == 4) { if (to) FI_LAUNCH((fi_forward_ori_direct<true, vfi_strides>), so); else FI_LAUNCH(fi_forward_ori_direct<true>); }
    else { if (to) FI_LAUNCH((fi_forward_ori_direct<false, vfi_strides>), so); else FI_LAUNCH(fi_forward_ori_direct<false>); }
#undef FI_LAUNCH
    return launch_status();
}

extern "C" int vfi_filterinterp_forward_ori_direct(const float* input1, const float* input2, const float* input3,
                                                    float* output, int batch, int channel, int h, int w,
                                                    int filter_channels, vfi_strides s1, vfi_strides s2,
                                                    vfi_strides s3, vfi_stream_t stream) {
    return launch_fi_ori_direct(input1, input2, input3, output, batch, channel, h, w, filter_channels, s1, s2, s3, s1, stream);
}

int vfi::fi_forward_ori_to(const float* input1, const float* input2, const float* input3, float* output, int batch, int channel,
                           int h, int w, int filter_channels, vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides so,
                           vfi_stream_t stream) {
    if (batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || filter_channels <= 0) return VFI_ERR_SHAPE;
    if (!input1 || !input2 || !input3 || !output) return VFI_ERR_SHAPE;
    if (so.h != s1.h) return VFI_ERR_SHAPE;
    const int fs = fi_filter_size(filter_channels);
    if (fs == 4) {
        const int r = launch_fi_ori_lds(input1, input2, input3, output, batch, channel, h, w, s1, s2, s3, so, stream);
        if (r != FI_DECLINED) return r;
    } else if (fs * fs == filter_channels) {
        const int r = launch_fi_ori_lds_n(input1, input2, input3, output, batch, channel, h, w, fs, s1, s2, s3, so, stream);
        if (r != FI_DECLINED) return r;
    }
    return launch_fi_ori_direct(input1, input2, input3, output, batch, channel, h, w, filter_channels, s1, s2, s3, so, stream);
}

extern "C" int vfi_filterinterp_forward_ori(const float* input1, const float* input2, const float* input3,
                                             float* output, int batch, int channel, int h, int w,
                                             int filter_channels, vfi_strides s1, vfi_strides s2, vfi_strides s3,
                                             vfi_stream_t stream) {
    return fi_forward_ori_to(input1, input2, input3, output, batch, channel, h, w, filter_channels, s1, s2, s3, s1, stream);
}

extern "C" int vfi_filterinterp_backward_ori(const float* input1, const float* input2, const float* input3,
                                              const float* gradoutput, float* gradinput1, float* gradinput2,
                                              float* gradinput3, int batch, int channel, int h, int w,
                                              int filter_channels, vfi_strides s1, vfi_strides s2, vfi_strides s3,
                                              vfi_stream_t stream) {
    if (batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || filter_channels <= 0) return VFI_ERR_SHAPE;
    if (!input1 || !input2 || !input3 || !gradoutput || !gradinput1 || !gradinput2 || !gradinput3)
        return VFI_ERR_SHAPE;
    const int fs = fi_filter_size(filter_channels);
    GradAccScratch sc;                                      // flags: one word per FB_TW x FB_TH (64 x 8) tile: "the staged kernel left it alone"
    const int ntiles = ((w + FB_TW - 1) / FB_TW) * ((h + FB_TH - 1) / FB_TH) * batch;
    int err = gradacc_begin((hipStream_t)stream, gradoutput, batch, channel, h, w, s1, input3, filter_channels, s3,
                            fs == 4 ? ntiles : 0, &sc);
    if (err != VFI_OK) return err;
    static_assert(VFI_TX == FB_TW && FB_TH % VFI_TY == 0, "fi_backward_ori's blocks nest in the staged kernel's tiles");
    if (fs == 4)
        hipLaunchKernelGGL(fi_backward_ori4_lds, dim3((w + FB_TW - 1) / FB_TW, (h + FB_TH - 1) / FB_TH, batch), dim3(FB_THREADS), 0,
                           (hipStream_t)stream, input1, input2, input3, gradoutput, sc.dir[0].acc, sc.dir[0].hdr, sc.flags,
                           gradinput2, gradinput3, channel, h, w, s1, s2, s3);
    hipLaunchKernelGGL(fi_backward_ori, pixel_grid(w, h, batch), dim3(VFI_TX, VFI_TY, 1), 0, (hipStream_t)stream,
                       input1, input2, input3, gradoutput, sc.dir[0].acc, sc.dir[0].hdr, gradinput1, gradinput2, gradinput3,
                       channel, h, w, fs, s1, s2, s3, sc.flags);
    if (launch_status() != VFI_OK) return VFI_ERR_LAUNCH;
    return gradacc_finish((hipStream_t)stream, sc.dir[0], gradinput1, batch, channel, h, w, s1);
}

extern "C" int vfi_filterinterp_blend_backward(const float* ref0, const float* ref2, const float* flow0, const float* flow2,
                                                const float* filt0, const float* filt2, const float* grad_blend,
                                                const float* grad_out0, const float* grad_out2, float* grad_ref0, float* grad_ref2,
                                                float* grad_flow0, float* grad_flow2, float* grad_filt0, float* grad_filt2,
                                                int batch, int channel, int h, int w, int filter_channels, float w0, float w2,
                                                vfi_strides s_ref, vfi_strides s_flow, vfi_strides s_filt, vfi_strides s_grad,
                                                vfi_stream_t stream) {
    if (batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || filter_channels <= 0) return VFI_ERR_SHAPE;
    if (!ref0 || !ref2 || !flow0 || !flow2 || !filt0 || !filt2) return VFI_ERR_SHAPE;
    if (!grad_ref0 && !grad_ref2 && !grad_flow0 && !grad_flow2 && !grad_filt0 && !grad_filt2) return VFI_OK;
    hipStream_t st = (hipStream_t)stream;
    const int fs = fi_filter_size(filter_channels);
    // the staged kernel for fs == 4 with exactly its 16 filter channels (it writes 16); any other count: per pixel, which
    // writes every channel of a requested filter gradient
    const bool staged = fs == 4 && filter_channels == 16;
    const bool want_x = grad_ref0 || grad_ref2;
    // both directions' sums when an image gradient is wanted, and one flag word per 64 x 8 tile of both directions (staged)
    const int ntiles = staged ? ((w + FB_TW - 1) / FB_TW) * ((h + FB_TH - 1) / FB_TH) * 2 * batch : 0;
    GradAccScratch sc;
    if (gradacc_reserve(st, want_x ? 2 : 0, (int64_t)batch * channel * h * w, ntiles, &sc) != VFI_OK) return VFI_ERR_LAUNCH;
    FiBwdPair pr;
    pr.d[0] = FiBwdSide{ref0, flow0, filt0, GradTerms{grad_blend, grad_out0, w0}, sc.dir[0].acc, sc.dir[0].hdr, grad_ref0, grad_flow0, grad_filt0};
    pr.d[1] = FiBwdSide{ref2, flow2, filt2, GradTerms{grad_blend, grad_out2, w2}, sc.dir[1].acc, sc.dir[1].hdr, grad_ref2, grad_flow2, grad_filt2};
    if (want_x)
        for (int d = 0; d < 2; ++d) {
            const FiBwdSide& sd = pr.d[d];
            if (!sd.gref) continue;
            // the fixed-point scale from the direction's own gradient as the kernels form it, and its filter
            if (sd.g.any() && gradacc_scan(st, sd.g, batch, channel, h, w, s_grad, sd.filt, filter_channels, s_filt,
                                           sc.dir[d].hdr) != VFI_OK)
                return VFI_ERR_LAUNCH;
            if (gradacc_zero_fp32(st, sd.hdr, sd.gref, batch, channel, h, w, s_ref) != VFI_OK) return VFI_ERR_LAUNCH;
        }
    const dim3 tiles((w + FB_TW - 1) / FB_TW, (h + FB_TH - 1) / FB_TH, 2 * batch);
    const dim3 px = pixel_grid(w, h, 2 * batch), pxb(VFI_TX, VFI_TY, 1);
    if (staged) {
        if (want_x) hipLaunchKernelGGL(fi_blend_backward4_lds<true>, tiles, dim3(FB_THREADS), 0, st, pr, sc.flags, batch, channel, h, w,
                                       s_ref, s_flow, s_filt, s_grad);
        else hipLaunchKernelGGL(fi_blend_backward4_lds<false>, tiles, dim3(FB_THREADS), 0, st, pr, sc.flags, batch, channel, h, w,
                                s_ref, s_flow, s_filt, s_grad);
    }
    if (want_x) hipLaunchKernelGGL(fi_blend_backward_general<true>, px, pxb, 0, st, pr, sc.flags, batch, channel, h, w, fs,
                                   filter_channels, s_ref, s_flow, s_filt, s_grad);
    else hipLaunchKernelGGL(fi_blend_backward_general<false>, px, pxb, 0, st, pr, sc.flags, batch, channel, h, w, fs, filter_channels,
                            s_ref, s_flow, s_filt, s_grad);
    if (launch_status() != VFI_OK) return VFI_ERR_LAUNCH;
    for (int d = 0; d < 2 && want_x; ++d)
        if (pr.d[d].gref && gradacc_finish(st, sc.dir[d], pr.d[d].gref, batch, channel, h, w, s_ref, true) != VFI_OK)
            return VFI_ERR_LAUNCH;
    return VFI_OK;
}

static int defor_forward(bool allow_staged, int variant, const float* input1, const float* input2,
                         const float* input3, const float* input4, float* output,
                         int batch, int channel, int h, int w, int filter_size,
                         vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides s4,
                         vfi_stream_t stream) {
    if (batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || filter_size <= 0) return VFI_ERR_SHAPE;
    if (!input1 || !input2 || !input3 || !output) return VFI_ERR_SHAPE;
    if (variant != VFI_DEFOR_NOFILTER && !input4) return VFI_ERR_SHAPE;
    const dim3 grid = pixel_grid(w, h, batch), block(VFI_TX, VFI_TY, 1);
    hipStream_t st = (hipStream_t)stream;
    if ((filter_size == 4 || filter_size == 6) && allow_staged && variant >= 0 && variant <= 2) {
        // the LDS-staged kernel; when it declines the shape, the general kernel below runs
        const int err = launch_fi_defor_lds(variant, input1, input2, input3, input4, output, batch, channel, h, w, filter_size,
                                            s1, s2, s3, s4, stream);
        if (err != FI_DECLINED) return err;
    }
    switch (variant) {
    case VFI_DEFOR_OFFSET:
        // the reference kernel has a body for fs 4 and 6 only; other sizes leave
        // the caller's (zero-filled) output untouched (:68)
        if (!(filter_size == 4 || filter_size == 6)) return VFI_OK;
        hipLaunchKernelGGL(fi_forward_defor<VFI_DEFOR_OFFSET>, grid, block, 0, st, input1, input2, input3, input4,
                           output, channel, h, w, filter_size, s1, s2, s3, s4);
        break;
    case VFI_DEFOR_REGION:
        hipLaunchKernelGGL(fi_forward_defor<VFI_DEFOR_REGION>, grid, block, 0, st, input1, input2, input3, input4,
                           output, channel, h, w, filter_size, s1, s2, s3, s4);
        break;
    case VFI_DEFOR_NOFILTER:
        hipLaunchKernelGGL(fi_forward_defor<VFI_DEFOR_NOFILTER>, grid, block, 0, st, input1, input2, input3,
                           input3, output, channel, h, w, filter_size, s1, s2, s3, s3);
        break;
    default:
        return VFI_ERR_SHAPE;
    }
    return launch_status();
}

extern "C" int vfi_filterinterp_forward_defor(int variant, const float* input1, const float* input2,
                                               const float* input3, const float* input4, float* output,
                                               int batch, int channel, int h, int w, int filter_size,
                                               vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides s4,
                                               vfi_stream_t stream) {
    return defor_forward(true, variant, input1, input2, input3, input4, output, batch, channel, h, w, filter_size, s1, s2, s3,
                         s4, stream);
}

// internal (not in vfi_hip.h): always the general one-thread-per-pixel kernel -- the tests compare the staged kernel with it
extern "C" int vfi_filterinterp_forward_defor_general(int variant, const float* input1, const float* input2,
                                                       const float* input3, const float* input4, float* output,
                                                       int batch, int channel, int h, int w, int filter_size,
                                                       vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides s4,
                                                       vfi_stream_t stream) {
    return defor_forward(false, variant, input1, input2, input3, input4, output, batch, channel, h, w, filter_size, s1, s2, s3,
                         s4, stream);
}

extern "C" int vfi_filterinterp_backward_defor(int variant, const float* input1, const float* input2,
                                                const float* input3, const float* input4, const float* gradoutput,
                                                float* gradinput1, float* gradinput2, float* gradinput3,
                                                float* gradinput4, int batch, int channel, int h, int w,
                                                int filter_size, vfi_strides s1, vfi_strides s2, vfi_strides s3,
                                                vfi_strides s4, vfi_stream_t stream) {
    if (batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || filter_size <= 0) return VFI_ERR_SHAPE;
    if (!input1 || !input2 || !input3 || !gradoutput || !gradinput1 || !gradinput2 || !gradinput3) return VFI_ERR_SHAPE;
    if (variant != VFI_DEFOR_NOFILTER && (!input4 || !gradinput4)) return VFI_ERR_SHAPE;
    if (variant < 0 || variant > 2) return VFI_ERR_SHAPE;
    const dim3 grid = pixel_grid(w, h, batch), block(VFI_TX, VFI_TY, 1);
    hipStream_t st = (hipStream_t)stream;
    // (the tap weights of the variant without a filter are 1)
    GradAccScratch sc;                                      // flags: one word per block: "the staged instance left it alone"
    const int err = gradacc_begin(st, gradoutput, batch, channel, h, w, s1, variant == VFI_DEFOR_NOFILTER ? nullptr : input3,
                                  filter_size * filter_size, s3, (int)(grid.x * grid.y * grid.z), &sc);
    if (err != VFI_OK) return err;
    unsigned long long* const acc = sc.dir[0].acc;
    const int* const hdr = sc.dir[0].hdr;
    // fs == 4: the LDS-staged kernel, then the per-tap fs == 4 instance for the blocks it flagged.  Otherwise, and when the
    // staged kernel declines the shape, the STAGED per-tap instance for any filter size, then its !STAGED one for the blocks
    // that one flagged.
    bool staged = false;
    if (filter_size == 4) {
        const int r = launch_fi_defor_bwd_lds(variant, input1, input2, input3, input4, gradoutput, acc, hdr, sc.flags, gradinput2,
                                              gradinput3, gradinput4, batch, channel, h, w, s1, s2, s3, s4, stream);
        if (r != VFI_OK && r != FI_DECLINED) return VFI_ERR_LAUNCH;
        staged = r == VFI_OK;
    }
    // (the variant without a filter has no input4: its kernel takes input3 / gradinput3 / s3 in those places)
    const bool nofilter = variant == VFI_DEFOR_NOFILTER;
    const float* in4 = nofilter ? input3 : input4;
    float* g4 = nofilter ? gradinput3 : gradinput4;
    const vfi_strides t4 = nofilter ? s3 : s4;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, st, input1, input2, input3, in4, gradoutput, acc, hdr, sc.flags, gradinput1,
                           gradinput2, gradinput3, g4, channel, h, w, filter_size, s1, s2, s3, t4);
    };
    switch (variant) {
    case VFI_DEFOR_OFFSET:
        if (staged) launch(fi_backward_defor<VFI_DEFOR_OFFSET, false, 4>);
        else { launch(fi_backward_defor<VFI_DEFOR_OFFSET, true, 0>); launch(fi_backward_defor<VFI_DEFOR_OFFSET, false, 0>); }
        break;
    case VFI_DEFOR_REGION:
        if (staged) launch(fi_backward_defor<VFI_DEFOR_REGION, false, 4>);
        else { launch(fi_backward_defor<VFI_DEFOR_REGION, true, 0>); launch(fi_backward_defor<VFI_DEFOR_REGION, false, 0>); }
        break;
    default:
        if (staged) launch(fi_backward_defor<VFI_DEFOR_NOFILTER, false, 4>);
        else { launch(fi_backward_defor<VFI_DEFOR_NOFILTER, true, 0>); launch(fi_backward_defor<VFI_DEFOR_NOFILTER, false, 0>); }
        break;
    }
    if (launch_status() != VFI_OK) return VFI_ERR_LAUNCH;
    return gradacc_finish(st, sc.dir[0], gradinput1, batch, channel, h, w, s1);
}
