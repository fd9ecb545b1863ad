// warp_correlation.hip -- PWC-Net's warp feeding its correlation layer, in one launch.
//
// PWCDCNet.forward (PWCNet/PWCNet.py:244-247, 266-267, 282-283, 299-300) does, at four of its five pyramid levels,
//     warp_k = self.warp(c2_k, up_flow * s)           # grid_sample + mask, PWCNet.py:159-199
//     corr_k = self.corr(c1_k, warp_k)                # correlation_cuda.forward, pad 4, k 1, md 4, strides 1
// and uses warp_k for nothing else.  Here the correlation kernel's staging loads of the second map ARE the warp: a
// window element (tile + 4 halo) is the bilinear sample of c2 at (x + flow) times the validity mask, formed exactly as
// vfi_pwc_warp_forward forms it (glue.hip) and written to LDS instead of HBM; the 81 products per pixel and channel are
// then those of vfi_correlation_forward, same sequential channel order.  The warped tensor never exists: per level one
// launch instead of two, and its write + read (2 x 18 MB at the finest 1080p level) are gone.  Results equal
// vfi_pwc_warp_forward followed by vfi_correlation_forward bit for bit.
//
// One kernel for every level size: 32 x 4 output pixels per workgroup, one wave per displacement row (9 waves), a
// lane owns two adjacent pixels; window 12 x 40 = 480 pixels, one per thread: a thread keeps its window pixel's
// four clamped tap offsets, four weights and mask in registers for all channels and fetches 8 channels x 4 taps
// per chunk, the next chunk's before the current one is multiplied.
#include "correlation_dev.h"
#include "pwc_warp.h"

namespace vfi {

typedef CorrTile2<4> WC;                                   // the tile of corr_forward_k1_rows2, md = 4

__global__ __launch_bounds__(WC::NT) void warp_corr_forward(
    const float* __restrict__ in1, const float* __restrict__ in2, const float* __restrict__ flo, float* __restrict__ out,
    int channel, int h, int w, int align_corners, vfi_strides sf) {
    typedef float v2f __attribute__((ext_vector_type(2)));
    constexpr int F1 = WC::CC * WC::TH * WC::TW, NF1 = (F1 + WC::NT - 1) / WC::NT;     // first-map values per chunk: 1024, 2 per thread
    __shared__ __attribute__((aligned(16))) float tile[WC::CC][WC::LH][WC::LW];
    __shared__ __attribute__((aligned(16))) float f1s[WC::CC][WC::TH * WC::TW];

    const int lane = threadIdx.x, tj = threadIdx.y;
    const int tid = tj * 64 + lane;
    const int px = WC::px(lane), py = WC::py(lane);
    const int ox = blockIdx.x * WC::TW + px, oy = blockIdx.y * WC::TH + py;
    const int b = blockIdx.z;
    const int64_t plane = (int64_t)h * w;
    const float* f1 = in1 + (int64_t)b * channel * plane;
    const float* f2 = in2 + (int64_t)b * channel * plane;
    const int wy0 = blockIdx.y * WC::TH - WC::MD, wx0 = blockIdx.x * WC::TW - WC::MD;   // window origin (pad == md: org = 0)

    // ---- this thread's window pixel: the warp's sampling geometry (pwc_warp.h, as glue.hip: pwc_warp_forward)
    const int wr = tid / WC::LW, wc = tid - wr * WC::LW;
    const int gy = wy0 + wr, gx = wx0 + wc;
    const bool wpix = tid < WC::LH * WC::LW;
    const bool inframe = wpix && gy >= 0 && gy < h && gx >= 0 && gx < w;        // else the correlation's zero padding
    int onw = 0, one = 0, osw = 0, ose = 0;
    PwcSample s = {};
    if (inframe) {
        const float* f = flo + (int64_t)b * sf.b + (int64_t)gy * sf.h + gx;
        s = pwc_sample(f[0], f[sf.c], gx, gy, h, w, align_corners);
        onw = s.cy0 * w + s.cx0; one = s.cy0 * w + s.cx1; osw = s.cy1 * w + s.cx0; ose = s.cy1 * w + s.cx1;
    }
    auto warped = [&](float pnw, float pne, float psw, float pse) { return pwc_warped(s, pnw, pne, psw, pse); };

    // ---- staging plan of the first map: value e = tid + k * NT of the chunk's [CC][TH][TW] block
    int foff[NF1], fch[NF1];
    bool fok[NF1];
#pragma unroll
    for (int k = 0; k < NF1; ++k) {
        const int e = tid + k * WC::NT;
        const int c = e / (WC::TH * WC::TW), rem = e - c * (WC::TH * WC::TW);
        const int y = blockIdx.y * WC::TH + rem / WC::TW, x = blockIdx.x * WC::TW + rem % WC::TW;
        fch[k] = c;
        fok[k] = e < F1 && y < h && x < w;
        foff[k] = fok[k] ? y * w + x : 0;
    }

    float acc[2][WC::D];
#pragma unroll
    for (int ti = 0; ti < WC::D; ++ti) { acc[0][ti] = 0.0f; acc[1][ti] = 0.0f; }

    float q[WC::CC][4], nf[NF1];
    auto fetch = [&](int c0) {
        const int cn = min(WC::CC, channel - c0);
#pragma unroll
        for (int c = 0; c < WC::CC; ++c) {
            // (a channel past the end re-reads the last one: its values are never used)
            const float* pl = f2 + (int64_t)(c0 + min(c, cn - 1)) * plane;
            q[c][0] = pl[onw]; q[c][1] = pl[one]; q[c][2] = pl[osw]; q[c][3] = pl[ose];
        }
#pragma unroll
        for (int k = 0; k < NF1; ++k) nf[k] = (fok[k] && fch[k] < cn) ? f1[(int64_t)(c0 + fch[k]) * plane + foff[k]] : 0.0f;
    };
    fetch(0);
    for (int c0 = 0; c0 < channel; c0 += WC::CC) {
        const int cn = min(WC::CC, channel - c0);
        __syncthreads();
        if (wpix) {
#pragma unroll
            for (int c = 0; c < WC::CC; ++c)
                tile[c][wr][wc] = (inframe && c < cn) ? warped(q[c][0], q[c][1], q[c][2], q[c][3]) : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < NF1; ++k) {
            const int e = tid + k * WC::NT;
            if (e < F1) (&f1s[0][0])[e] = nf[k];
        }
        __syncthreads();
        if (c0 + WC::CC < channel) fetch(c0 + WC::CC);
        for (int c = 0; c < cn; ++c) {
            const v2f a = *reinterpret_cast<const v2f*>(&f1s[c][py * WC::TW + px]);
            v2f t[WC::PAIRS];
            WC::read_row(&tile[c][py + tj][px], t);
#pragma unroll
            for (int ti = 0; ti < WC::D; ++ti) {
                acc[0][ti] = fmaf(a.x, t[ti / 2][ti & 1], acc[0][ti]);
                acc[1][ti] = fmaf(a.y, t[(ti + 1) / 2][(ti + 1) & 1], acc[1][ti]);
            }
        }
    }
    const float nelems = (float)channel;
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (ox + k < w && oy < h) {
            float* o = out + ((int64_t)b * (WC::D * WC::D) + tj * WC::D) * plane + (int64_t)oy * w + ox + k;
#pragma unroll
            for (int ti = 0; ti < WC::D; ++ti) o[(int64_t)ti * plane] = acc[k][ti] / nelems;
        }
}

}  // namespace vfi

using namespace vfi;

extern "C" int vfi_pwc_warp_correlation_forward(const float* input1, const float* input2, const float* flow, float* output,
                                                 int batch, int channel, int h, int w, int align_corners,
                                                 vfi_strides sf, vfi_stream_t stream) {
    if (batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || !input1 || !input2 || !flow || !output) return VFI_ERR_SHAPE;
    if ((int64_t)h * w > (1 << 30) || batch > 65535) return VFI_ERR_SHAPE;         // in-plane offsets are 32-bit
    const dim3 grid((w + WC::TW - 1) / WC::TW, (h + WC::TH - 1) / WC::TH, batch);
    hipLaunchKernelGGL(warp_corr_forward, grid, dim3(64, WC::D, 1), 0, (hipStream_t)stream, input1, input2, flow, output,
                       channel, h, w, align_corners ? 1 : 0, sf);
    return launch_status();
}
