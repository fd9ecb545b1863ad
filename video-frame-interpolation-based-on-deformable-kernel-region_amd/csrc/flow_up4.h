// flow_up4.h -- the x4 bilinear upsample of the quarter-resolution flow (forward_flownets), shared by its forward
// (projection.hip: flow_upsample4) and its adjoint (projection_up4_backward.hip).
#pragma once

#include "vfi_common.h"

namespace vfi {

// torch's upsample_bilinear2d, align_corners=False, scale factor 4 (ATen UpSampleBilinear2d):
// source index 0.25 * (dst + 0.5) - 0.5 clamped at 0, second tap one further unless at the edge
struct UpTap { int i0, i1; float l0, l1; };
__device__ __forceinline__ UpTap up4_tap(int dst, int in_size) {
    float src = 0.25f * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.0f ? 0.0f : src;
    UpTap t;
    t.i0 = (int)src;
    t.i1 = t.i0 + (t.i0 < in_size - 1 ? 1 : 0);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}
// one channel of the upsampled (m0 * plane) * m1 from its four taps; fused as nvcc fuses ATen's expression
__device__ __forceinline__ float up4_blend(float q00, float q01, float q10, float q11, const UpTap& ty, const UpTap& tx,
                                           float m0, float m1) {
    const float p00 = (m0 * q00) * m1, p01 = (m0 * q01) * m1, p10 = (m0 * q10) * m1, p11 = (m0 * q11) * m1;
    const float t0 = fmaf(tx.l1, p01, tx.l0 * p00);
    const float t1 = fmaf(tx.l1, p11, tx.l0 * p10);
    return fmaf(ty.l1, t1, ty.l0 * t0);
}
__device__ __forceinline__ float up4_sample(const float* __restrict__ plane, int64_t hs, const UpTap& ty, const UpTap& tx,
                                            float m0, float m1) {
    return up4_blend(plane[(int64_t)ty.i0 * hs + tx.i0], plane[(int64_t)ty.i0 * hs + tx.i1],
                     plane[(int64_t)ty.i1 * hs + tx.i0], plane[(int64_t)ty.i1 * hs + tx.i1], ty, tx, m0, m1);
}

// ---- the adjoint.  A quarter pixel q of an axis of in_size quarter pixels is a tap of the full-resolution pixels
// d = 4q - 2 + k, k = 0..7, cut to the image (d = 4q - 3 has taps q - 2, q - 1; d = 4q + 6 has q + 1, q + 2).  Its weight
// in pixel d is w(d) = (i0 == q ? l0 : 0) + (i1 == q ? l1 : 0) of up4_tap(d): l1 on the low side, l0 on the high side,
// l0 + l1 (one fp32 add) where the far edge clamps both taps onto q.
#define UP4_FOOT 8
struct Up4Foot {
    int lo, hi;             // the k with 0 <= 4q - 2 + k < 4 in_size are lo <= k < hi
    float w[UP4_FOOT];      // w(4q - 2 + k) (0 outside lo..hi)
};
__device__ __forceinline__ Up4Foot up4_foot(int q, int in_size) {
    Up4Foot f;
    const int d0 = 4 * q - 2;
    f.lo = d0 < 0 ? -d0 : 0;
    f.hi = min(UP4_FOOT, 4 * in_size - d0);
#pragma unroll
    for (int k = 0; k < UP4_FOOT; ++k) {
        const UpTap t = up4_tap(max(d0 + k, 0), in_size);
        const float w = (t.i0 == q ? t.l0 : 0.0f) + (t.i1 == q ? t.l1 : 0.0f);
        f.w[k] = (k >= f.lo && k < f.hi) ? w : 0.0f;
    }
    return f;
}

// One item's part of the adjoint at quarter pixel (qy, qx): with G the item's full-resolution gradient plane,
//     s = 0;  for ky = fy.lo .. fy.hi - 1:  { r = 0;  for kx = fx.lo .. fx.hi - 1:  r = fmaf(fx.w[kx], G[ky][kx], r);
//                                             s = fmaf(fy.w[ky], r, s); }
// (rows ascending, columns ascending inside a row, every step one fused multiply-add; pixels outside the image are
// skipped, not added as zeros).  The caller folds the items in order: acc = fmaf(m_i, s_i, acc) from acc = 0, with
// m_i = mul0 * mul1[i] rounded once.  tests/proj_up4_backward.py restates this bit for bit.
// rows(ky, v): loads v[kx] = G[4qy - 2 + ky][4qx - 2 + kx] for fx.lo <= kx < fx.hi (the rest of v is not used).
template <class Rows>
__device__ __forceinline__ float up4_adjoint(const Up4Foot& fy, const Up4Foot& fx, const Rows& rows) {
    float s = 0.0f;
#pragma unroll
    for (int ky = 0; ky < UP4_FOOT; ++ky) {
        if (ky < fy.lo || ky >= fy.hi) continue;
        float v[UP4_FOOT];
        rows(ky, v);
        float r = 0.0f;
#pragma unroll
        for (int kx = 0; kx < UP4_FOOT; ++kx)
            if (kx >= fx.lo && kx < fx.hi) r = fmaf(fx.w[kx], v[kx], r);
        s = fmaf(fy.w[ky], r, s);
    }
    return s;
}

}  // namespace vfi
