// projection_up4_backward.hip -- training through the quarter-resolution flow.
//
// The training chain is flow network -> x div_flow x t -> nn.Upsample(x4, bilinear) -> FlowProject
// (networks/DAIN.py:196-238, 296-311, 533-539).  Two backwards live here, both pure gathers with ordered sums, so both
// are reproducible bit for bit and neither needs a zero-filled or accumulated output:
//
//   flow_upsample4_backward   the adjoint of vfi_flow_upsample4 for a LIST of time offsets: grad_q = sum_i m_i U^T G_i
//                             with G_i the caller's full-resolution gradients (up4_adjoint of flow_up4.h);
//   proj_backward_up4<DEPTH>  the same with G_i = what vfi_[depth]flowprojection_backward writes for the upsampled flow
//                             F_i = U(flow_q) -- formed per tile in LDS: neither F_i nor G_i reaches global memory.
//
// proj_backward_up4: one workgroup of 256 threads owns UB_QY x UB_QX = 8 x 16 quarter pixels.  Per item:
//   phase 1  over the tile's full-resolution footprint (32 x 64 own pixels plus two halo pixels on either side:
//            36 x 68), thread p, p + 256, ...: F = up4_blend of the four flow_q taps (the forward's
//            expression, so target pixels and validity are the forward's, bit for bit), then proj_backward's gather
//            from count / gout (/ depth, out) in proj_backward's operation order; G -> LDS, two planes of 36 rows of
//            68 floats (19 KB: eight workgroups per CU fit the 160 KB); with DEPTH the own pixels' depth
//            gradient -> global memory;
//   phase 2  thread = (channel, qy, qx): up4_adjoint over its 8 x 8 block of the LDS planes (a row is two aligned
//            16-byte reads: the block starts at column 4 qx of the staged footprint), folded into the thread's sum.
// After the last item every thread stores its one grad_q element.
#include "vfi_common.h"
#include "flow_up4.h"

#include <limits.h>

namespace vfi {

#define UB_NMAX 8                       // items per call (PROJ_NMAX of projection.hip)
#define UB_QX 16
#define UB_QY 8
#define UB_THREADS (2 * UB_QX * UB_QY)
#define UB_FW (4 * UB_QX + 4)           // footprint columns 4 qx0 - 2 .. 4 (qx0 + UB_QX) + 1
#define UB_FH (4 * UB_QY + 4)
#define UB_PITCH UB_FW                  // 16-byte rows
static_assert(UB_THREADS == 256 && UB_PITCH % 4 == 0, "tile layout");

struct Up4BwdItems {
    const float* g[UB_NMAX];            // flow_upsample4_backward: grad_full; proj_backward_up4: gradoutput
    const float* count[UB_NMAX];
    const float* depth[UB_NMAX];
    const float* out[UB_NMAX];
    float* gdepth[UB_NMAX];             // may be null
    float m1[UB_NMAX];                  // mul1: the forward's second multiplier
    float m[UB_NMAX];                   // mul0 * mul1, rounded once
    int n;
};

// loads of one footprint row from a global plane: 4-byte lanes (the block starts two floats before a 16-byte boundary
// at best, and the tensors' strides are the caller's)
struct Up4RowsGlobal {
    const float* base;                  // element (4qy - 2, 4qx - 2) of the plane
    int hs;
    Up4Foot fx;
    __device__ __forceinline__ void operator()(int ky, float* v) const {
        const float* row = base + ky * hs;
#pragma unroll
        for (int kx = 0; kx < UP4_FOOT; ++kx) v[kx] = (kx >= fx.lo && kx < fx.hi) ? row[kx] : 0.0f;
    }
};

// grad_q[b, c, qy, qx] = sum_i m_i * up4_adjoint(G_i[b, c]);  blockIdx.x = (b * channels + c, tile row, tile column)
__global__ __launch_bounds__(VFI_TX * VFI_TY) void flow_upsample4_backward(
    Up4BwdItems it, float* __restrict__ grad_q, int channels, int hq, int wq, int tiles_x, int tiles_y,
    vfi_strides sg, vfi_strides sq) {
    int blk = blockIdx.x;
    const int tx = blk % tiles_x; blk /= tiles_x;
    const int ty = blk % tiles_y; blk /= tiles_y;
    const int c = blk % channels, b = blk / channels;
    const int qx = tx * VFI_TX + threadIdx.x, qy = ty * VFI_TY + threadIdx.y;
    if (qx >= wq || qy >= hq) return;
    const Up4Foot fy = up4_foot(qy, hq), fx = up4_foot(qx, wq);
    const int64_t plane = (int64_t)b * sg.b + (int64_t)c * sg.c;
    const int corner = (4 * qy - 2) * (int)sg.h + (4 * qx - 2);      // (may be negative: the rows / columns below lo are not read)
    float acc = 0.0f;
    for (int i = 0; i < it.n; ++i) {
        const Up4RowsGlobal rows{it.g[i] + plane + corner, (int)sg.h, fx};
        acc = fmaf(it.m[i], up4_adjoint(fy, fx, rows), acc);
    }
    grad_q[(int64_t)b * sq.b + (int64_t)c * sq.c + (int64_t)qy * sq.h + qx] = acc;
}

struct Up4RowsLds {
    const float* base;                  // the thread's block inside its channel's LDS plane (16-byte aligned)
    __device__ __forceinline__ void operator()(int ky, float* v) const {
        const float4 a = *reinterpret_cast<const float4*>(base + ky * UB_PITCH);
        const float4 c = *reinterpret_cast<const float4*>(base + ky * UB_PITCH + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = c.x; v[5] = c.y; v[6] = c.z; v[7] = c.w;
    }
};

struct Up4BwdGeom {
    int hq, wq, tiles_x, tiles_y;
    int64_t qb, qc;                     // flow_q batch / channel stride
    int qh;
    int64_t cb, db, ob, oc;             // count / depth / out + gout batch strides, out + gout channel stride
    int ch, dh, oh;
    int64_t gb, gc;                     // grad_q
    int gh;
};

template <bool DEPTH>
__global__ __launch_bounds__(UB_THREADS) void proj_backward_up4(
    const float* __restrict__ flow_q, Up4BwdItems it, float* __restrict__ grad_q, float m0, Up4BwdGeom g) {
    __shared__ __attribute__((aligned(16))) float G[2][UB_FH][UB_PITCH];
    int blk = blockIdx.x;
    const int tx = blk % g.tiles_x; blk /= g.tiles_x;
    const int ty = blk % g.tiles_y;
    const int b = blk / g.tiles_y;
    const int h = 4 * g.hq, w = 4 * g.wq;
    const int y0 = 4 * ty * UB_QY - 2, x0 = 4 * tx * UB_QX - 2;      // the footprint's corner
    const int tid = threadIdx.x;
    // phase 2's role
    const int pc = tid / (UB_QX * UB_QY), pqy = (tid / UB_QX) % UB_QY, pqx = tid % UB_QX;
    const int qy = ty * UB_QY + pqy, qx = tx * UB_QX + pqx;
    const bool owner = qy < g.hq && qx < g.wq;
    Up4Foot fy, fx;
    if (owner) { fy = up4_foot(qy, g.hq); fx = up4_foot(qx, g.wq); }
    const float* fq0 = flow_q + (int64_t)b * g.qb;
    const float* fq1 = fq0 + g.qc;
    float acc = 0.0f;
    for (int i = 0; i < it.n; ++i) {
        const float m1 = it.m1[i];
        const float* cn = it.count[i] + (int64_t)b * g.cb;
        const float* go0 = it.g[i] + (int64_t)b * g.ob;
        const float* go1 = go0 + g.oc;
        if (i > 0) __syncthreads();                         // phase 2 of the item before is done with the planes
        for (int p = tid; p < UB_FH * UB_FW; p += UB_THREADS) {
            const int r = p / UB_FW, cl = p - r * UB_FW;
            const int y = y0 + r, x = x0 + cl;
            if (y < 0 || y >= h || x < 0 || x >= w) continue;       // (phase 2 skips these cells)
            const UpTap uy = up4_tap(y, g.hq), ux = up4_tap(x, g.wq);
            const float fxv = up4_sample(fq0, g.qh, uy, ux, m0, m1);
            const float fyv = up4_sample(fq1, g.qh, uy, ux, m0, m1);
            // proj_backward (projection.hip) from here on, statement for statement, on a gradient that starts at 0
            const float x2 = (float)x + fxv;
            const float y2 = (float)y + fyv;
            float g0 = 0.0f, g1 = 0.0f, gd = 0.0f;
            if (x2 >= 0.0f && y2 >= 0.0f && x2 <= (float)(w - 1) && y2 <= (float)(h - 1)) {
                const int L = (int)x2, T = (int)y2;
                const int R = min(L + 1, w - 1), Bm = min(T + 1, h - 1);
                const int to[4] = { T * g.oh + L, T * g.oh + R, Bm * g.oh + L, Bm * g.oh + R };
                const int tc[4] = { T * g.ch + L, T * g.ch + R, Bm * g.ch + L, Bm * g.ch + R };
                float gv0[4], gv1[4], cv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) { gv0[k] = go0[to[k]]; gv1[k] = go1[to[k]]; cv[k] = cn[tc[k]]; }
                if constexpr (DEPTH) {
                    const float d = it.depth[i][(int64_t)b * g.db + y * g.dh + x];
#pragma unroll
                    for (int k = 0; k < 4; ++k) { g0 += -gv0[k] * d / cv[k]; g1 += -gv1[k] * d / cv[k]; }
                    const float* fo0 = it.out[i] + (int64_t)b * g.ob;
                    const float* fo1 = fo0 + g.oc;
#pragma unroll
                    for (int k = 0; k < 4; ++k) gd += -gv0[k] / cv[k] * (fxv - fo0[to[k]]);
#pragma unroll
                    for (int k = 0; k < 4; ++k) gd += -gv1[k] / cv[k] * (fyv - fo1[to[k]]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) { g0 += -gv0[k] / cv[k]; g1 += -gv1[k] / cv[k]; }
                }
            }
            G[0][r][cl] = g0;
            G[1][r][cl] = g1;
            if constexpr (DEPTH) {
                // the tile's own pixels: rows / columns 2 .. 4 UB_Q + 1 of the footprint
                if (it.gdepth[i] && r >= 2 && r < 4 * UB_QY + 2 && cl >= 2 && cl < 4 * UB_QX + 2)
                    it.gdepth[i][(int64_t)b * g.db + y * g.dh + x] = gd;
            }
        }
        __syncthreads();
        if (owner) {
            const Up4RowsLds rows{&G[pc][4 * pqy][4 * pqx]};
            acc = fmaf(it.m[i], up4_adjoint(fy, fx, rows), acc);
        }
    }
    if (owner) grad_q[(int64_t)b * g.gb + (int64_t)pc * g.gc + qy * g.gh + qx] = acc;
}

// every in-plane element offset of a [*, *, h, w] tensor with row stride sh fits 31 bits
static bool fits32(int64_t sh, int h, int w) { return sh >= 0 && sh * (int64_t)(h - 1) + w < ((int64_t)1 << 31); }

static bool quarter_ok(int batch, int hq, int wq) {
    return batch > 0 && hq > 0 && wq > 0 && hq <= INT_MAX / 4 && wq <= INT_MAX / 4;
}

template <bool DEPTH>
static int project_backward_up4(const float* flow_q, const float* const* depths, const float* const* counts,
                                const float* const* outs, const float* const* gouts, const float* mul1, int n, float* grad_q,
                                float* const* grad_depths, int batch, int hq, int wq, float mul0, vfi_strides sq, vfi_strides s2,
                                vfi_strides sc, vfi_strides so, vfi_strides sgq, hipStream_t st) {
    if (n < 1 || n > UB_NMAX || !quarter_ok(batch, hq, wq) || !flow_q || !counts || !gouts || !mul1 || !grad_q ||
        (DEPTH && (!depths || !outs)))
        return VFI_ERR_SHAPE;
    const int h = 4 * hq, w = 4 * wq;
    if (!fits32(sq.h, hq, wq) || !fits32(sgq.h, hq, wq) || !fits32(sc.h, h, w) || !fits32(so.h, h, w) ||
        (DEPTH && !fits32(s2.h, h, w)))
        return VFI_ERR_SHAPE;
    Up4BwdItems it;
    for (int i = 0; i < UB_NMAX; ++i) {
        const int k = i < n ? i : 0;                        // (unused slots repeat item 0)
        if (!counts[k] || !gouts[k] || (DEPTH && (!depths[k] || !outs[k]))) return VFI_ERR_SHAPE;
        it.g[i] = gouts[k]; it.count[i] = counts[k];
        it.depth[i] = DEPTH ? depths[k] : nullptr; it.out[i] = DEPTH ? outs[k] : nullptr;
        it.gdepth[i] = DEPTH && grad_depths ? grad_depths[k] : nullptr;
        it.m1[i] = mul1[k]; it.m[i] = mul0 * mul1[k];
    }
    it.n = n;
    Up4BwdGeom g;
    g.hq = hq; g.wq = wq;
    g.tiles_x = (wq + UB_QX - 1) / UB_QX; g.tiles_y = (hq + UB_QY - 1) / UB_QY;
    const int64_t blocks = (int64_t)g.tiles_x * g.tiles_y * batch;
    if (blocks > INT_MAX) return VFI_ERR_SHAPE;
    g.qb = sq.b; g.qc = sq.c; g.qh = (int)sq.h;
    g.cb = sc.b; g.ch = (int)sc.h;
    g.db = DEPTH ? s2.b : 0; g.dh = DEPTH ? (int)s2.h : 0;
    g.ob = so.b; g.oc = so.c; g.oh = (int)so.h;
    g.gb = sgq.b; g.gc = sgq.c; g.gh = (int)sgq.h;
    hipLaunchKernelGGL(proj_backward_up4<DEPTH>, dim3((unsigned)blocks), dim3(UB_THREADS), 0, st, flow_q, it, grad_q, mul0, g);
    return launch_status();
}

}  // namespace vfi

using namespace vfi;

extern "C" int vfi_flow_upsample4_backward(const float* const* grad_full, const float* mul1, int nitems, float* grad_q,
                                            int batch, int channels, int hq, int wq, float mul0, vfi_strides sg, vfi_strides sq,
                                            vfi_stream_t stream) {
    if (nitems < 1 || nitems > UB_NMAX || !quarter_ok(batch, hq, wq) || channels <= 0 || !grad_full || !mul1 || !grad_q)
        return VFI_ERR_SHAPE;
    if (!fits32(sg.h, 4 * hq, 4 * wq) || !fits32(sq.h, hq, wq)) return VFI_ERR_SHAPE;
    Up4BwdItems it = {};
    for (int i = 0; i < UB_NMAX; ++i) {
        const int k = i < nitems ? i : 0;
        if (!grad_full[k]) return VFI_ERR_SHAPE;
        it.g[i] = grad_full[k]; it.m1[i] = mul1[k]; it.m[i] = mul0 * mul1[k];
    }
    it.n = nitems;
    const int tiles_x = (wq + VFI_TX - 1) / VFI_TX, tiles_y = (hq + VFI_TY - 1) / VFI_TY;
    const int64_t blocks = (int64_t)tiles_x * tiles_y * batch * channels;
    if (blocks > INT_MAX) return VFI_ERR_SHAPE;
    hipLaunchKernelGGL(flow_upsample4_backward, dim3((unsigned)blocks), dim3(VFI_TX, VFI_TY, 1), 0, (hipStream_t)stream, it,
                       grad_q, channels, hq, wq, tiles_x, tiles_y, sg, sq);
    return launch_status();
}

extern "C" int vfi_flowprojection_backward_up4(const float* flow_q, const float* const* counts, const float* const* gradoutputs,
                                                const float* mul1, int nitems, float* grad_q, int batch, int hq, int wq,
                                                float mul0, vfi_strides sq, vfi_strides sc, vfi_strides so, vfi_strides sgq,
                                                vfi_stream_t stream) {
    return project_backward_up4<false>(flow_q, nullptr, counts, nullptr, gradoutputs, mul1, nitems, grad_q, nullptr, batch, hq, wq,
                                       mul0, sq, sc, sc, so, sgq, (hipStream_t)stream);
}

extern "C" int vfi_depthflowprojection_backward_up4(const float* flow_q, const float* const* depths, const float* const* counts,
                                                     const float* const* outputs, const float* const* gradoutputs,
                                                     const float* mul1, int nitems, float* grad_q, float* const* grad_depths,
                                                     int batch, int hq, int wq, float mul0, vfi_strides sq, vfi_strides s2,
                                                     vfi_strides sc, vfi_strides so, vfi_strides sgq, vfi_stream_t stream) {
    return project_backward_up4<true>(flow_q, depths, counts, outputs, gradoutputs, mul1, nitems, grad_q, grad_depths, batch, hq,
                                      wq, mul0, sq, s2, sc, so, sgq, (hipStream_t)stream);
}
