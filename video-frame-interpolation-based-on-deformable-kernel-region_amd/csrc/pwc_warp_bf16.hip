// pwc_warp_bf16.hip -- PWCDCNet.warp (PWCNet/PWCNet.py:159-199) on bfloat16 storage, forward and backward, for gfx950.
//
// x, the warped output and their gradients are bfloat16; the flow (and its gradient) is float32 or bfloat16 (FB).  Every
// value is widened on load (exact), the arithmetic is the float32 entries' in their order (pwc_warp.h; glue.hip:
// pwc_warp_forward; pwc_warp_backward.hip), and a result is rounded to bfloat16 once, to nearest even:
//   forward   bf16_rne(vfi_pwc_warp_forward(float(x), float(flow)))                                      bit for bit
//   grad_x    bf16_rne of what vfi_pwc_warp_backward leaves in a zero-filled float32 grad_x: the same fixed-point
//             accumulator (gradacc.h) with the same scale (the max-scan sees the widened gradoutput), the same addends and
//             integer sums, one conversion, one rounding; WRITTEN, never added into (gradacc_finish_bf16)
//   grad_flow the float32 entry's ordered channel sum -- the same channel groups, the same combine -- rounded once where the
//             flow is bfloat16
// A call that gradacc_fp32 sends to fp32 atomics (a non-finite gradoutput, magnitudes that could overflow) adds floats into
// the accumulator's zeroed cells and rounds once at the end: no atomic ever touches bfloat16 storage.
//
// Memory instructions.  The warped output and gradoutput rows are regular: a lane owns TWO horizontally adjacent pixels and
// moves them with one 4-byte access where the pair is 4-byte aligned and inside the row, with 2-byte accesses otherwise
// (bf16.h).  The four gathered taps of a pixel stay 2-byte loads.
#include "bf16.h"
#include "gradacc.h"
#include "pwc_warp.h"
#include "workspace.h"

#include <algorithm>
#include <climits>

namespace vfi {

template <bool FB>
__device__ __forceinline__ float pwb_flow(const void* flo, int64_t at) {
    if constexpr (FB) return bf16_widen(static_cast<const bf16_t*>(flo)[at]);
    else return static_cast<const float*>(flo)[at];
}
// two adjacent flow-gradient elements (the second only where `pair`)
template <bool FB>
__device__ __forceinline__ void pwb_store_flow(void* gf, int64_t at, float lo, float hi, bool pair) {
    if constexpr (FB) {
        bf16_store_pair(static_cast<bf16_t*>(gf) + at, bf16_pack_rne(lo, hi), pair);
    } else {
        float* p = static_cast<float*>(gf) + at;
        p[0] = lo;
        if (pair) p[1] = hi;
    }
}

// ---------------------------------------------------------------------------------------------------------------- forward
//
// A workgroup: 64 x 8 pixels as 32 x 8 lanes of one pixel pair each (a wave stores two 128-byte row segments per plane);
// blockIdx.z = batch x chunks of PWB_CH channels, all of a chunk's 8 x PWB_CH tap loads in flight at once.
#define PWB_TX 32
#define PWB_TY 8
#define PWB_CH 8

template <bool FB>
__global__ __launch_bounds__(PWB_TX * PWB_TY) void pwc_warp_forward_bf16(
    const bf16_t* __restrict__ xin, const void* __restrict__ flo, bf16_t* __restrict__ out,
    int channel, int groups, int h, int w, int align_corners, vfi_strides sx, vfi_strides sf, vfi_strides so) {
    const int x = 2 * (blockIdx.x * PWB_TX + threadIdx.x);
    const int y = blockIdx.y * PWB_TY + threadIdx.y;
    if (x >= w || y >= h) return;
    const bool pair = x + 1 < w;
    const int b = blockIdx.z / groups;
    const int64_t fo = (int64_t)b * sf.b + (int64_t)y * sf.h + x;
    PwcSample s[2];
    int64_t o[2][4];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int d = pair ? p : 0;                         // (a lone pixel is formed twice; its copy is dropped by the store)
        s[p] = pwc_sample(pwb_flow<FB>(flo, fo + d), pwb_flow<FB>(flo, fo + sf.c + d), x + d, y, h, w, align_corners);
        o[p][0] = (int64_t)s[p].cy0 * sx.h + s[p].cx0; o[p][1] = (int64_t)s[p].cy0 * sx.h + s[p].cx1;
        o[p][2] = (int64_t)s[p].cy1 * sx.h + s[p].cx0; o[p][3] = (int64_t)s[p].cy1 * sx.h + s[p].cx1;
    }
    const int c0 = (int)(blockIdx.z % groups) * PWB_CH, cn = min(PWB_CH, channel - c0);
    const bf16_t* src = xin + (int64_t)b * sx.b;
    bf16_t* dst = out + (int64_t)b * so.b + (int64_t)y * so.h + x;
    // a corner outside the map is read at a clamped (valid) address and replaced by 0 with weight 0 (pwc_warped); a channel
    // past the chunk re-reads the chunk's last one and is not stored
    bf16_t q[PWB_CH][2][4];
#pragma unroll
    for (int c = 0; c < PWB_CH; ++c) {
        const bf16_t* pl = src + (int64_t)(c0 + min(c, cn - 1)) * sx.c;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int k = 0; k < 4; ++k) q[c][p][k] = pl[o[p][k]];
    }
#pragma unroll
    for (int c = 0; c < PWB_CH; ++c) {
        if (c >= cn) break;
        float v[2];
#pragma unroll
        for (int p = 0; p < 2; ++p)
            v[p] = pwc_warped(s[p], bf16_widen(q[c][p][0]), bf16_widen(q[c][p][1]), bf16_widen(q[c][p][2]), bf16_widen(q[c][p][3]));
        bf16_store_pair(dst + (int64_t)(c0 + c) * so.c, bf16_pack_rne(v[0], v[1]), pair);
    }
}

// ---------------------------------------------------------------------------------------------------------------- backward
//
// pwc_warp_backward_tile (pwc_warp_backward.hip) with two pixels per lane: the same 64 x 8 tile -- so the same tile count and
// the same channel groups as the float32 entry, on which the bits of grad_flow depend -- on 256 threads, the same LDS
// window of 64-bit cells over the bounding box of the corners the tile's masked-in pixels touch, one global integer atomic
// per non-zero cell.  PBB_CH channels per pass: 9 loads per lane and channel (8 taps, one gradoutput pair).
#define PBB_TW 64
#define PBB_TH 8
#define PBB_THREADS 256
#define PBB_GROUP_CH 8                              // the float32 entry's PB_CH: channel groups are multiples of it
#define PBB_CH 4
#define PBB_CELLS 6144                              // 64-bit cells of LDS (49,152 bytes)

template <bool FB>
__global__ __launch_bounds__(PBB_THREADS) void pwc_warp_backward_tile_bf16(
    const bf16_t* __restrict__ xin, const void* __restrict__ flo, const bf16_t* __restrict__ gout,
    unsigned long long* __restrict__ acc, const int* __restrict__ hdr, void* gflow, float* __restrict__ partial,
    int channel, int cgroup, int groups, int h, int w, int align_corners, float sfx, float sfy,
    vfi_strides sx, vfi_strides sf, vfi_strides sgo, vfi_strides sgf) {
    __shared__ unsigned long long cells[PBB_CELLS];
    __shared__ int box[4];
    const int tid = threadIdx.x;
    const int x = blockIdx.x * PBB_TW + 2 * (tid & 31);
    const int y = blockIdx.y * PBB_TH + (tid >> 5);
    const int b = blockIdx.z / groups, grp = blockIdx.z - b * groups;
    const int cb = grp * cgroup, ce = min(channel, cb + cgroup);
    const bool want_x = acc != nullptr, want_f = gflow != nullptr;
    const GradAccCtx gctx = want_x ? gradacc_ctx(hdr) : GradAccCtx{1.0f, 1.0f, false};
    const bool inimg[2] = {x < w && y < h, x + 1 < w && y < h};
    const bool pair = inimg[1];
    PwcSample s[2] = {};
    bool scat[2], flowsum[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (inimg[p]) {
            const int64_t fo = (int64_t)b * sf.b + (int64_t)y * sf.h + x + p;
            s[p] = pwc_sample(pwb_flow<FB>(flo, fo), pwb_flow<FB>(flo, fo + sf.c), x + p, y, h, w, align_corners);
        }
        // scatter: a masked-in pixel; on the fp32 path every pixel, as the reference's atomics (Inf * mask 0 = NaN reaches them)
        scat[p] = want_x && inimg[p] && (s[p].mask != 0.0f || gctx.nonfinite);
        // the coordinate gradient: ATen adds a term per in-bounds corner (a pixel with none adds nothing, not NaN x 0)
        flowsum[p] = want_f && (s[p].bnw || s[p].bne || s[p].bsw || s[p].bse);
    }
    const bool load = scat[0] || scat[1] || flowsum[0] || flowsum[1];

    // ---- the tile's window: bounding box of the clamped corners of its scattering pixels (workgroup-uniform decision)
    bool staged = false;
    int bx0 = 0, by0 = 0, bw = 0, n = 0, step = PBB_CH;
    if (want_x && gradacc_staged_ok(gctx)) {
        if (tid == 0) { box[0] = INT_MAX; box[1] = INT_MAX; box[2] = INT_MIN; box[3] = INT_MIN; }
        __syncthreads();
        const int tx0 = min(scat[0] ? s[0].cx0 : INT_MAX, scat[1] ? s[1].cx0 : INT_MAX);
        const int ty0 = min(scat[0] ? s[0].cy0 : INT_MAX, scat[1] ? s[1].cy0 : INT_MAX);
        const int tx1 = max(scat[0] ? s[0].cx1 : INT_MIN, scat[1] ? s[1].cx1 : INT_MIN);
        const int ty1 = max(scat[0] ? s[0].cy1 : INT_MIN, scat[1] ? s[1].cy1 : INT_MIN);
        const int wx0 = wave_min_i32(tx0), wy0 = wave_min_i32(ty0);
        const int wx1 = wave_max_i32(tx1), wy1 = wave_max_i32(ty1);
        if ((tid & 63) == 0 && wx0 != INT_MAX) {
            atomicMin(&box[0], wx0); atomicMin(&box[1], wy0);
            atomicMax(&box[2], wx1); atomicMax(&box[3], wy1);
        }
        __syncthreads();
        if (box[0] != INT_MAX) {
            bx0 = box[0]; by0 = box[1]; bw = box[2] - box[0] + 1;
            const int64_t cells_per_channel = (int64_t)bw * (box[3] - box[1] + 1);
            if (cells_per_channel <= PBB_CELLS) {
                n = (int)cells_per_channel;
                step = min(PBB_CH, PBB_CELLS / n);          // channels per pass: as many as the cells allow
                staged = true;
            }
        }
    }
    const bf16_t* xb = xin + (int64_t)b * sx.b;
    const bf16_t* gb = gout + (int64_t)b * sgo.b + (int64_t)y * sgo.h + x;
    // one 4-byte load per gradoutput pair where every channel's pair is 4-byte aligned (an even channel stride keeps the
    // alignment of the first one); the decision is per lane and around the whole batch of loads
    const bool galigned = pair && (sgo.c & 1) == 0 && bf16_pair_aligned(gb);
    int64_t o[2][4];                                        // the corners' elements of x
    int wo[2][4];                                           // ... and their cells in the tile's window
    float dx1[2], dx0[2], dy1[2], dy0[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        o[p][0] = (int64_t)s[p].cy0 * sx.h + s[p].cx0; o[p][1] = (int64_t)s[p].cy0 * sx.h + s[p].cx1;
        o[p][2] = (int64_t)s[p].cy1 * sx.h + s[p].cx0; o[p][3] = (int64_t)s[p].cy1 * sx.h + s[p].cx1;
        wo[p][0] = (s[p].cy0 - by0) * bw + s[p].cx0 - bx0; wo[p][1] = (s[p].cy0 - by0) * bw + s[p].cx1 - bx0;
        wo[p][2] = (s[p].cy1 - by0) * bw + s[p].cx0 - bx0; wo[p][3] = (s[p].cy1 - by0) * bw + s[p].cx1 - bx0;
        dx1[p] = s[p].fx0 + 1.0f - s[p].ix; dx0[p] = s[p].ix - s[p].fx0;
        dy1[p] = s[p].fy0 + 1.0f - s[p].iy; dy0[p] = s[p].iy - s[p].fy0;
    }
    const int64_t plane = (int64_t)h * w;
    unsigned long long* accb = want_x ? acc + (int64_t)b * channel * plane : nullptr;
    float gix[2] = {0.0f, 0.0f}, giy[2] = {0.0f, 0.0f};
    for (int c0 = cb; c0 < ce; c0 += step) {               // (trip count workgroup-uniform)
        const int cn = min(step, ce - c0);
        if (staged) {
            for (int e = tid; e < n * cn; e += PBB_THREADS) cells[e] = 0ull;
            __syncthreads();
        }
        if (load) {
            // every load of the pass in flight at once (a channel past the pass re-reads its last one, never used)
            bf16_t q[PBB_CH][2][4];
            unsigned gv[PBB_CH];
#pragma unroll
            for (int c = 0; c < PBB_CH; ++c) {
                const bf16_t* pl = xb + (int64_t)(c0 + min(c, cn - 1)) * sx.c;
#pragma unroll
                for (int p = 0; p < 2; ++p)
#pragma unroll
                    for (int k = 0; k < 4; ++k) q[c][p][k] = pl[o[p][k]];
            }
            if (galigned) {
#pragma unroll
                for (int c = 0; c < PBB_CH; ++c)
                    gv[c] = *reinterpret_cast<const unsigned*>(gb + (int64_t)(c0 + min(c, cn - 1)) * sgo.c);
            } else {
#pragma unroll
                for (int c = 0; c < PBB_CH; ++c) {
                    const bf16_t* g = gb + (int64_t)(c0 + min(c, cn - 1)) * sgo.c;
                    gv[c] = (unsigned)g[0] | ((unsigned)g[pair ? 1 : 0] << 16);
                }
            }
#pragma unroll
            for (int c = 0; c < PBB_CH; ++c) {
                if (c >= cn) break;
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const float gval = __uint_as_float(p ? gv[c] & 0xffff0000u : gv[c] << 16);
                    const float gm = gval * s[p].mask;      // MulBackward of output * mask
                    if (scat[p]) {
                        // ATen's addend nw * gOut, then the fixed-point integer (or the fp32 atomic of that call)
                        const float av[4] = {s[p].enw * gm, s[p].ene * gm, s[p].esw * gm, s[p].ese * gm};
                        const bool in[4] = {s[p].bnw, s[p].bne, s[p].bsw, s[p].bse};
                        if (staged) {
                            unsigned long long* win = cells + c * n;
#pragma unroll
                            for (int k = 0; k < 4; ++k)
                                if (in[k]) atomicAdd(&win[wo[p][k]], (unsigned long long)__float2ll_rn(av[k] * gctx.scale));
                        } else {
                            // per corner: the integer into the cell, or on the fp32 path a FLOAT into the cell's low word
                            // (float index 2 x cell index; the finish rounds it to bfloat16 once)
                            unsigned long long* ap = accb + (int64_t)(c0 + c) * plane;
                            const int cys[4] = {s[p].cy0, s[p].cy0, s[p].cy1, s[p].cy1};
                            const int cxs[4] = {s[p].cx0, s[p].cx1, s[p].cx0, s[p].cx1};
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                const int64_t at = (int64_t)cys[k] * w + cxs[k];
                                if (in[k]) gradacc_add(ap, reinterpret_cast<float*>(ap), at, 2 * at, av[k], gctx);
                            }
                        }
                    }
                    if (flowsum[p]) {
                        const float pnw = s[p].bnw ? bf16_widen(q[c][p][0]) : 0.0f, pne = s[p].bne ? bf16_widen(q[c][p][1]) : 0.0f;
                        const float psw = s[p].bsw ? bf16_widen(q[c][p][2]) : 0.0f, pse = s[p].bse ? bf16_widen(q[c][p][3]) : 0.0f;
                        float t = (pne - pnw) * dy1[p];
                        t = fmaf(pse - psw, dy0[p], t);
                        gix[p] = fmaf(gm, t, gix[p]);
                        t = (psw - pnw) * dx1[p];
                        t = fmaf(pse - pne, dx0[p], t);
                        giy[p] = fmaf(gm, t, giy[p]);
                    }
                }
            }
        }
        if (staged) {
            __syncthreads();
            for (int e = tid; e < n * cn; e += PBB_THREADS) {
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
    if (want_f && inimg[0]) {
        if (groups == 1) {
            const int64_t at = (int64_t)b * sgf.b + (int64_t)y * sgf.h + x;
            pwb_store_flow<FB>(gflow, at, gix[0] * sfx, gix[1] * sfx, pair);
            pwb_store_flow<FB>(gflow, at + sgf.c, giy[0] * sfy, giy[1] * sfy, pair);
        } else {                                            // [b][group][2][h][w], summed by pwc_warp_flow_combine_bf16
            float* pp = partial + (int64_t)blockIdx.z * 2 * plane + (int64_t)y * w + x;
            pp[0] = gix[0];
            pp[plane] = giy[0];
            if (pair) { pp[1] = gix[1]; pp[plane + 1] = giy[1]; }
        }
    }
}

// grad_flow = (sum of the groups' partial sums, in group order) x the coordinate factor; a lane owns two adjacent pixels
template <bool FB>
__global__ __launch_bounds__(PWB_TX * PWB_TY) void pwc_warp_flow_combine_bf16(
    const float* __restrict__ partial, void* __restrict__ gflow, int groups, int h, int w, float sfx, float sfy, vfi_strides sgf) {
    const int x = 2 * (blockIdx.x * PWB_TX + threadIdx.x);
    const int y = blockIdx.y * PWB_TY + threadIdx.y;
    if (x >= w || y >= h) return;
    const bool pair = x + 1 < w;
    const int b = blockIdx.z;
    const int64_t plane = (int64_t)h * w;
    const float* p = partial + (int64_t)b * groups * 2 * plane + (int64_t)y * w + x;
    const int d = pair ? 1 : 0;
    float sx[2] = {0.0f, 0.0f}, sy[2] = {0.0f, 0.0f};
    for (int g = 0; g < groups; ++g) {
        sx[0] += p[(int64_t)g * 2 * plane];
        sy[0] += p[(int64_t)g * 2 * plane + plane];
        sx[1] += p[(int64_t)g * 2 * plane + d];
        sy[1] += p[(int64_t)g * 2 * plane + plane + d];
    }
    const int64_t at = (int64_t)b * sgf.b + (int64_t)y * sgf.h + x;
    pwb_store_flow<FB>(gflow, at, sx[0] * sfx, sx[1] * sfx, pair);
    pwb_store_flow<FB>(gflow, at + sgf.c, sy[0] * sfy, sy[1] * sfy, pair);
}

}  // namespace vfi

using namespace vfi;

extern "C" int vfi_pwc_warp_forward_bf16(const void* x, const void* flow, int flow_is_bf16, void* output, int batch, int channel,
                                          int h, int w, int align_corners, vfi_strides sx, vfi_strides sf, vfi_strides so,
                                          vfi_stream_t stream) {
    if (batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || !x || !flow || !output) return VFI_ERR_SHAPE;
    const int groups = (channel + PWB_CH - 1) / PWB_CH;
    const dim3 grid((unsigned)((w + 2 * PWB_TX - 1) / (2 * PWB_TX)), (unsigned)((h + PWB_TY - 1) / PWB_TY), (unsigned)(batch * groups));
    if ((int64_t)batch * groups > 65535 || grid.y > 65535) return VFI_ERR_SHAPE;
    hipLaunchKernelGGL(flow_is_bf16 ? pwc_warp_forward_bf16<true> : pwc_warp_forward_bf16<false>, grid, dim3(PWB_TX, PWB_TY, 1), 0,
                       (hipStream_t)stream, (const bf16_t*)x, flow, (bf16_t*)output, channel, groups, h, w, align_corners ? 1 : 0,
                       sx, sf, so);
    return launch_status();
}

extern "C" int vfi_pwc_warp_backward_bf16(const void* x, const void* flow, int flow_is_bf16, const void* grad_output, void* grad_x,
                                           void* grad_flow, int batch, int channel, int h, int w, int align_corners,
                                           vfi_strides sx, vfi_strides sf, vfi_strides sgo, vfi_strides sgx, vfi_strides sgf,
                                           vfi_stream_t stream) {
    if (batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || !x || !flow || !grad_output) return VFI_ERR_SHAPE;
    const dim3 tiles((unsigned)((w + PBB_TW - 1) / PBB_TW), (unsigned)((h + PBB_TH - 1) / PBB_TH), 1);
    if (batch > 65535 || tiles.y > 65535) return VFI_ERR_SHAPE;
    if (!grad_x && !grad_flow) return VFI_OK;
    const hipStream_t st = (hipStream_t)stream;
    // the channel groups of vfi_pwc_warp_backward, exactly: grad_flow adds the groups' partial sums, so its bits depend on them
    const int64_t ntiles = (int64_t)tiles.x * tiles.y * batch;
    const int c8 = (channel + PBB_GROUP_CH - 1) / PBB_GROUP_CH;
    int groups = (int)std::min<int64_t>(c8, std::max<int64_t>(1, (device_cu_count() + ntiles - 1) / ntiles));
    groups = std::min(groups, 65535 / batch);
    const int cgroup = PBB_GROUP_CH * ((c8 + groups - 1) / groups);
    groups = (channel + cgroup - 1) / cgroup;
    const float sfx = (float)((align_corners ? (w - 1) / 2.0 : w / 2.0) * 2.0 / std::max(w - 1, 1));
    const float sfy = (float)((align_corners ? (h - 1) / 2.0 : h / 2.0) * 2.0 / std::max(h - 1, 1));
    float* partial = nullptr;
    if (grad_flow && groups > 1) {
        partial = static_cast<float*>(ws_get(st, WS_PWC_FLOW, (size_t)batch * groups * 2 * h * w * sizeof(float), false, nullptr));
        if (!partial) return VFI_ERR_LAUNCH;
    }
    GradAccScratch sc{};
    if (grad_x) {                                           // (bilinear weights times the mask: at most 1; 4 taps per pixel)
        const int err = gradacc_begin_bf16(st, (const bf16_t*)grad_output, batch, channel, h, w, sgo, 4, &sc);
        if (err != VFI_OK) return err;
    }
    hipLaunchKernelGGL(flow_is_bf16 ? pwc_warp_backward_tile_bf16<true> : pwc_warp_backward_tile_bf16<false>,
                       dim3(tiles.x, tiles.y, (unsigned)(batch * groups)), dim3(PBB_THREADS), 0, st, (const bf16_t*)x, flow,
                       (const bf16_t*)grad_output, sc.dir[0].acc, sc.dir[0].hdr, grad_flow, partial, channel, cgroup, groups, h, w,
                       align_corners ? 1 : 0, sfx, sfy, sx, sf, sgo, sgf);
    if (launch_status() != VFI_OK) return VFI_ERR_LAUNCH;
    if (partial) {
        const dim3 grid((unsigned)((w + 2 * PWB_TX - 1) / (2 * PWB_TX)), (unsigned)((h + PWB_TY - 1) / PWB_TY), (unsigned)batch);
        hipLaunchKernelGGL(flow_is_bf16 ? pwc_warp_flow_combine_bf16<true> : pwc_warp_flow_combine_bf16<false>, grid,
                           dim3(PWB_TX, PWB_TY, 1), 0, st, partial, grad_flow, groups, h, w, sfx, sfy, sgf);
        if (launch_status() != VFI_OK) return VFI_ERR_LAUNCH;
    }
    return grad_x ? gradacc_finish_bf16(st, sc.dir[0], (bf16_t*)grad_x, batch, channel, h, w, sgx) : VFI_OK;
}
