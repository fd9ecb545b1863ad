// pwc_warp_backward.hip -- the backward of PWCDCNet.warp (PWCNet/PWCNet.py:159-199) for gfx950.
//
// What torch autograd gives for the reference's warp(): the mask is a constant (`mask[mask<0.9999]=0; mask[mask>0]=1`
// overwrites every element, so nothing reaches the mask's own grid_sample); the sample is ATen's bilinear
// grid_sampler_2d with zero padding, whose backward skips a corner outside the map in both gradients.  With
// gm = gradoutput * mask, per pixel (pwc_warp.h gives the coordinate, corners, weights and mask):
//   grad_x[c, corner] += gm[c] * w_corner                                          (the in-bounds corners)
//   gix = sum_c gm[c] * ((ne - nw) (y0 + 1 - iy) + (se - sw) (iy - y0))            (a corner outside the map reads 0)
//   giy = sum_c gm[c] * ((sw - nw) (x0 + 1 - ix) + (se - ne) (ix - x0))
//   grad_flow = (gix, giy) x grid_sampler_unnormalize's factor ((W-1)/2 aligned, W/2 not) x 2 / max(W-1, 1)
// The image gradient is summed by the 64-bit fixed-point accumulator (gradacc.h "Deterministic image gradients"): a
// 64x8 tile adds its integer addends in LDS over the bounding box of the corners its masked-in pixels touch and issues
// one global atomic per non-zero cell (as interp_backward_lds, warp_sepconv.hip).  A tile whose box does not fit, a
// call whose scale needs its second factor and a call on the fp32 path add per corner instead (gradacc_add).  The flow
// gradient is a per-thread sum over the channels in a fixed order; when a pixel's channels are split over workgroups
// (blockIdx.z = batch x channel groups, for parallelism at the coarse levels) the partial sums go to a scratch plane
// and pwc_warp_flow_combine adds them in group order.  No float atomics outside the fp32 path: bit-reproducible.
#include "gradacc.h"
#include "pwc_warp.h"
#include "workspace.h"

#include <algorithm>

namespace vfi {

#define PB_TW 64
#define PB_TH 8
#define PB_THREADS (PB_TW * PB_TH)
#define PB_CH 8                                     // channels whose 5 loads per thread are in flight together
#define PB_CELLS 6144                               // 64-bit cells of LDS (49,152 bytes)

__global__ __launch_bounds__(PB_THREADS) void pwc_warp_backward_tile(
    const float* __restrict__ xin, const float* __restrict__ flo, const float* __restrict__ gout,
    unsigned long long* __restrict__ acc, const int* __restrict__ hdr, float* gx, float* gflow, float* __restrict__ partial,
    int channel, int cgroup, int groups, int h, int w, int align_corners, float sfx, float sfy,
    vfi_strides sx, vfi_strides sf, vfi_strides sgo, vfi_strides sgx, vfi_strides sgf) {
    __shared__ unsigned long long cells[PB_CELLS];
    __shared__ int box[4];
    const int tid = threadIdx.x;
    const int x = blockIdx.x * PB_TW + (tid & (PB_TW - 1));
    const int y = blockIdx.y * PB_TH + (tid >> 6);
    const int b = blockIdx.z / groups, grp = blockIdx.z - b * groups;
    const int cb = grp * cgroup, ce = min(channel, cb + cgroup);
    const bool want_x = acc != nullptr, want_f = gflow != nullptr;
    const GradAccCtx gctx = want_x ? gradacc_ctx(hdr) : GradAccCtx{1.0f, 1.0f, false};
    const bool inimg = x < w && y < h;
    PwcSample s = {};
    if (inimg) {
        const float* f = flo + (int64_t)b * sf.b + (int64_t)y * sf.h + x;
        s = pwc_sample(f[0], f[sf.c], x, y, h, w, align_corners);
    }
    // scatter: a masked-in pixel; on the fp32 path every pixel, as the reference's atomics (Inf * mask 0 = NaN reaches them)
    const bool scat = want_x && inimg && (s.mask != 0.0f || gctx.nonfinite);
    // the coordinate gradient: ATen adds a term per in-bounds corner (a pixel with none adds nothing, not NaN x 0)
    const bool flowsum = want_f && (s.bnw || s.bne || s.bsw || s.bse);
    const bool load = scat || flowsum;

    // ---- the tile's window: bounding box of the clamped corners of its scattering pixels (workgroup-uniform decision)
    bool staged = false;
    int bx0 = 0, by0 = 0, bw = 0, n = 0, step = PB_CH;
    if (want_x && gradacc_staged_ok(gctx)) {
        if (tid == 0) { box[0] = INT_MAX; box[1] = INT_MAX; box[2] = INT_MIN; box[3] = INT_MIN; }
        __syncthreads();
        const int wx0 = wave_min_i32(scat ? s.cx0 : INT_MAX), wy0 = wave_min_i32(scat ? s.cy0 : INT_MAX);
        const int wx1 = wave_max_i32(scat ? s.cx1 : INT_MIN), wy1 = wave_max_i32(scat ? s.cy1 : INT_MIN);
        if ((tid & 63) == 0 && wx0 != INT_MAX) {
            atomicMin(&box[0], wx0); atomicMin(&box[1], wy0);
            atomicMax(&box[2], wx1); atomicMax(&box[3], wy1);
        }
        __syncthreads();
        if (box[0] != INT_MAX) {
            bx0 = box[0]; by0 = box[1]; bw = box[2] - box[0] + 1;
            const int64_t cells_per_channel = (int64_t)bw * (box[3] - box[1] + 1);
            if (cells_per_channel <= PB_CELLS) {
                n = (int)cells_per_channel;
                step = min(PB_CH, PB_CELLS / n);            // channels per pass: as many as the cells allow
                staged = true;
            }
        }
    }
    const float* xb = xin + (int64_t)b * sx.b;
    const float* gb = gout + (int64_t)b * sgo.b + (int64_t)y * sgo.h + x;
    const int64_t onw = (int64_t)s.cy0 * sx.h + s.cx0, one = (int64_t)s.cy0 * sx.h + s.cx1;
    const int64_t osw = (int64_t)s.cy1 * sx.h + s.cx0, ose = (int64_t)s.cy1 * sx.h + s.cx1;
    // the corners' cells: in the tile's window (staged), in the dense scratch and in the caller's gradient (per corner)
    const int wnw = (s.cy0 - by0) * bw + s.cx0 - bx0, wne = (s.cy0 - by0) * bw + s.cx1 - bx0;
    const int wsw = (s.cy1 - by0) * bw + s.cx0 - bx0, wse = (s.cy1 - by0) * bw + s.cx1 - bx0;
    const int64_t anw = (int64_t)s.cy0 * w + s.cx0, ane = (int64_t)s.cy0 * w + s.cx1;
    const int64_t asw = (int64_t)s.cy1 * w + s.cx0, ase = (int64_t)s.cy1 * w + s.cx1;
    const int64_t gnw = (int64_t)s.cy0 * sgx.h + s.cx0, gne = (int64_t)s.cy0 * sgx.h + s.cx1;
    const int64_t gsw = (int64_t)s.cy1 * sgx.h + s.cx0, gse = (int64_t)s.cy1 * sgx.h + s.cx1;
    const int64_t plane = (int64_t)h * w;
    unsigned long long* accb = want_x ? acc + (int64_t)b * channel * plane : nullptr;
    const float dx1 = s.fx0 + 1.0f - s.ix, dx0 = s.ix - s.fx0, dy1 = s.fy0 + 1.0f - s.iy, dy0 = s.iy - s.fy0;
    float gix = 0.0f, giy = 0.0f;
    for (int c0 = cb; c0 < ce; c0 += step) {               // (trip count workgroup-uniform)
        const int cn = min(step, ce - c0);
        if (staged) {
            for (int e = tid; e < n * cn; e += PB_THREADS) cells[e] = 0ull;
            __syncthreads();
        }
        if (load) {
            // every load of the pass in flight at once (a channel past the pass re-reads its last one, never used)
            float q[PB_CH][4], gv[PB_CH];
#pragma unroll
            for (int c = 0; c < PB_CH; ++c) {
                const int64_t cc = c0 + min(c, cn - 1);
                const float* pl = xb + cc * sx.c;
                q[c][0] = pl[onw]; q[c][1] = pl[one]; q[c][2] = pl[osw]; q[c][3] = pl[ose];
                gv[c] = gb[cc * sgo.c];
            }
#pragma unroll
            for (int c = 0; c < PB_CH; ++c) {
                if (c >= cn) break;
                const float gm = gv[c] * s.mask;            // MulBackward of output * mask
                if (scat) {
                    // ATen's addend nw * gOut, then the fixed-point integer (or the fp32 atomic of that call)
                    const float anw_v = s.enw * gm, ane_v = s.ene * gm, asw_v = s.esw * gm, ase_v = s.ese * gm;
                    if (staged) {
                        unsigned long long* win = cells + c * n;
                        if (s.bnw) atomicAdd(&win[wnw], (unsigned long long)__float2ll_rn(anw_v * gctx.scale));
                        if (s.bne) atomicAdd(&win[wne], (unsigned long long)__float2ll_rn(ane_v * gctx.scale));
                        if (s.bsw) atomicAdd(&win[wsw], (unsigned long long)__float2ll_rn(asw_v * gctx.scale));
                        if (s.bse) atomicAdd(&win[wse], (unsigned long long)__float2ll_rn(ase_v * gctx.scale));
                    } else {
                        unsigned long long* ap = accb + (int64_t)(c0 + c) * plane;
                        float* gp = gx + (int64_t)b * sgx.b + (int64_t)(c0 + c) * sgx.c;
                        if (s.bnw) gradacc_add(ap, gp, anw, gnw, anw_v, gctx);
                        if (s.bne) gradacc_add(ap, gp, ane, gne, ane_v, gctx);
                        if (s.bsw) gradacc_add(ap, gp, asw, gsw, asw_v, gctx);
                        if (s.bse) gradacc_add(ap, gp, ase, gse, ase_v, gctx);
                    }
                }
                if (flowsum) {
                    const float pnw = s.bnw ? q[c][0] : 0.0f, pne = s.bne ? q[c][1] : 0.0f;
                    const float psw = s.bsw ? q[c][2] : 0.0f, pse = s.bse ? q[c][3] : 0.0f;
                    float t = (pne - pnw) * dy1;
                    t = fmaf(pse - psw, dy0, t);
                    gix = fmaf(gm, t, gix);
                    t = (psw - pnw) * dx1;
                    t = fmaf(pse - pne, dx0, t);
                    giy = fmaf(gm, t, giy);
                }
            }
        }
        if (staged) {
            __syncthreads();
            for (int e = tid; e < n * cn; e += PB_THREADS) {
                const unsigned long long v = cells[e];
                if (v != 0ull) {
                    const int cc = e / n, r = e - cc * n;
                    const int cy = r / bw, cx = r - cy * bw;
                    atomicAdd(&accb[(int64_t)(c0 + cc) * plane + (int64_t)(by0 + cy) * w + bx0 + cx], v);
                }
            }
            __syncthreads();                                // (the next pass zeroes the cells)
        }
    }
    if (want_f && inimg) {
        if (groups == 1) {
            float* gf = gflow + (int64_t)b * sgf.b + (int64_t)y * sgf.h + x;
            gf[0] = gix * sfx;
            gf[sgf.c] = giy * sfy;
        } else {                                            // [b][group][2][h][w], summed by pwc_warp_flow_combine
            float* p = partial + (int64_t)blockIdx.z * 2 * plane + (int64_t)y * w + x;
            p[0] = gix;
            p[plane] = giy;
        }
    }
}

// grad_flow = (sum of the groups' partial sums, in group order) x the coordinate factor
__global__ __launch_bounds__(VFI_TX * VFI_TY) void pwc_warp_flow_combine(
    const float* __restrict__ partial, float* __restrict__ gflow, int groups, int h, int w, float sfx, float sfy,
    vfi_strides sgf) {
    const int x = blockIdx.x * VFI_TX + threadIdx.x;
    const int y = blockIdx.y * VFI_TY + threadIdx.y;
    if (x >= w || y >= h) return;
    const int b = blockIdx.z;
    const int64_t plane = (int64_t)h * w;
    const float* p = partial + (int64_t)b * groups * 2 * plane + (int64_t)y * w + x;
    float sx = 0.0f, sy = 0.0f;
    for (int g = 0; g < groups; ++g) {
        sx += p[(int64_t)g * 2 * plane];
        sy += p[(int64_t)g * 2 * plane + plane];
    }
    float* gf = gflow + (int64_t)b * sgf.b + (int64_t)y * sgf.h + x;
    gf[0] = sx * sfx;
    gf[sgf.c] = sy * sfy;
}

}  // namespace vfi

using namespace vfi;

extern "C" int vfi_pwc_warp_backward(const float* x, const float* flow, const float* grad_output, float* grad_x,
                                      float* grad_flow, int batch, int channel, int h, int w, int align_corners,
                                      vfi_strides sx, vfi_strides sf, vfi_strides sgo, vfi_strides sgx, vfi_strides sgf,
                                      vfi_stream_t stream) {
    if (batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || !x || !flow || !grad_output) return VFI_ERR_SHAPE;
    const dim3 tiles((unsigned)((w + PB_TW - 1) / PB_TW), (unsigned)((h + PB_TH - 1) / PB_TH), 1);
    if (batch > 65535 || tiles.y > 65535) return VFI_ERR_SHAPE;
    if (!grad_x && !grad_flow) return VFI_OK;
    const hipStream_t st = (hipStream_t)stream;
    // channel groups of 8k channels, enough of them for about one workgroup per CU (the coarse levels have few tiles)
    const int64_t ntiles = (int64_t)tiles.x * tiles.y * batch;
    const int c8 = (channel + PB_CH - 1) / PB_CH;
    int groups = (int)std::min<int64_t>(c8, std::max<int64_t>(1, (device_cu_count() + ntiles - 1) / ntiles));
    groups = std::min(groups, 65535 / batch);
    const int cgroup = PB_CH * ((c8 + groups - 1) / groups);
    groups = (channel + cgroup - 1) / cgroup;
    // d(ix)/d(flow x): grid_sampler_unnormalize's factor times the normalisation's 2 / max(W - 1, 1) (PWCNet.py:184-185)
    const float sfx = (float)((align_corners ? (w - 1) / 2.0 : w / 2.0) * 2.0 / std::max(w - 1, 1));
    const float sfy = (float)((align_corners ? (h - 1) / 2.0 : h / 2.0) * 2.0 / std::max(h - 1, 1));
    float* partial = nullptr;
    if (grad_flow && groups > 1) {
        partial = static_cast<float*>(ws_get(st, WS_PWC_FLOW, (size_t)batch * groups * 2 * h * w * sizeof(float), false, nullptr));
        if (!partial) return VFI_ERR_LAUNCH;
    }
    GradAccScratch sc{};
    if (grad_x) {                                           // (bilinear weights times the mask: at most 1; 4 taps per pixel)
        const int err = gradacc_begin(st, grad_output, batch, channel, h, w, sgo, nullptr, 4, sgo, 0, &sc);
        if (err != VFI_OK) return err;
    }
    hipLaunchKernelGGL(pwc_warp_backward_tile, dim3(tiles.x, tiles.y, (unsigned)(batch * groups)), dim3(PB_THREADS), 0, st,
                       x, flow, grad_output, sc.dir[0].acc, sc.dir[0].hdr, grad_x, grad_flow, partial, channel, cgroup, groups, h, w,
                       align_corners ? 1 : 0, sfx, sfy, sx, sf, sgo, sgx, sgf);
    if (launch_status() != VFI_OK) return VFI_ERR_LAUNCH;
    if (partial) {
        hipLaunchKernelGGL(pwc_warp_flow_combine, pixel_grid(w, h, batch), dim3(VFI_TX, VFI_TY, 1), 0, st, partial, grad_flow,
                           groups, h, w, sfx, sfy, sgf);
        if (launch_status() != VFI_OK) return VFI_ERR_LAUNCH;
    }
    return grad_x ? gradacc_finish(st, sc.dir[0], grad_x, batch, channel, h, w, sgx) : VFI_OK;
}
