// pwc_warp.h -- the sampling geometry of PWCDCNet.warp (PWCNet/PWCNet.py:159-199), shared by the forward kernels
// (glue.hip: pwc_warp_forward; warp_correlation.hip: warp_corr_forward) and the backward (pwc_warp_backward.hip), so the
// passes cannot disagree about a coordinate, a corner or which pixels are masked in.
#pragma once
#include "vfi_common.h"

namespace vfi {

struct PwcSample {
    float ix, iy, fx0, fy0;                 // the source coordinate and its floor (ATen's ix_nw, iy_nw)
    float enw, ene, esw, ese;               // bilinear weights of the corners inside the map, 0 for the others
    int cx0, cx1, cy0, cy1;                 // corner columns / rows clamped into the map (always valid addresses)
    bool bnw, bne, bsw, bse;                // corner inside the map
    float mask;                             // 1 where grid_sample(ones) >= 0.9999, else 0
};

// vgrid = pixel + flow; normalised as PWCNet.py:184-185; ATen's grid_sampler_unnormalize (align_corners: 1 = torch <= 1.2,
// 0 = the default of torch >= 1.3); the mask as grid_sample of a ones tensor, thresholded.
__device__ __forceinline__ PwcSample pwc_sample(float fx, float fy, int x, int y, int h, int w, int align_corners) {
    PwcSample s;
    const float vx = (float)x + fx, vy = (float)y + fy;
    const float gx = 2.0f * vx / (float)max(w - 1, 1) - 1.0f;
    const float gy = 2.0f * vy / (float)max(h - 1, 1) - 1.0f;
    s.ix = align_corners ? ((gx + 1.0f) / 2.0f) * (float)(w - 1) : ((gx + 1.0f) * (float)w - 1.0f) / 2.0f;
    s.iy = align_corners ? ((gy + 1.0f) / 2.0f) * (float)(h - 1) : ((gy + 1.0f) * (float)h - 1.0f) / 2.0f;
    s.fx0 = floorf(s.ix);
    s.fy0 = floorf(s.iy);
    // corners as ATen orders them: nw, ne, sw, se; weights from the opposite corner
    const float wnw = (s.fx0 + 1.0f - s.ix) * (s.fy0 + 1.0f - s.iy), wne = (s.ix - s.fx0) * (s.fy0 + 1.0f - s.iy);
    const float wsw = (s.fx0 + 1.0f - s.ix) * (s.iy - s.fy0), wse = (s.ix - s.fx0) * (s.iy - s.fy0);
    // float -> int of a huge or NaN coordinate is undefined in C; such a corner is out of bounds anyway
    const bool finite = fabsf(s.ix) < 1.0e9f && fabsf(s.iy) < 1.0e9f;
    const int x0 = finite ? (int)s.fx0 : -2, y0 = finite ? (int)s.fy0 : -2;
    const bool inx0 = x0 >= 0 && x0 < w, inx1 = x0 + 1 >= 0 && x0 + 1 < w;
    const bool iny0 = y0 >= 0 && y0 < h, iny1 = y0 + 1 >= 0 && y0 + 1 < h;
    float m = 0.0f;
    if (iny0 && inx0) m += wnw;
    if (iny0 && inx1) m += wne;
    if (iny1 && inx0) m += wsw;
    if (iny1 && inx1) m += wse;
    s.mask = (m < 0.9999f) ? 0.0f : (m > 0.0f ? 1.0f : m);   // mask[mask<0.9999]=0; mask[mask>0]=1 (NaN stays)
    s.cx0 = clampi(x0, 0, w - 1); s.cx1 = clampi(x0 + 1, 0, w - 1);
    s.cy0 = clampi(y0, 0, h - 1); s.cy1 = clampi(y0 + 1, 0, h - 1);
    s.bnw = iny0 && inx0; s.bne = iny0 && inx1; s.bsw = iny1 && inx0; s.bse = iny1 && inx1;
    s.enw = s.bnw ? wnw : 0.0f; s.ene = s.bne ? wne : 0.0f; s.esw = s.bsw ? wsw : 0.0f; s.ese = s.bse ? wse : 0.0f;
    return s;
}

// the warped value of one channel from its four (clamped) corner reads: a corner outside the map contributes value 0
// with weight 0, so v = fma(0, 0, v) = v -- the same result as ATen's skipped corner, from straight-line loads
__device__ __forceinline__ float pwc_warped(const PwcSample& s, float pnw, float pne, float psw, float pse) {
    float v = 0.0f;                                         // out_acc += value * weight, fused as nvcc fuses ATen's grid_sampler
    v = fmaf(s.bnw ? pnw : 0.0f, s.enw, v);
    v = fmaf(s.bne ? pne : 0.0f, s.ene, v);
    v = fmaf(s.bsw ? psw : 0.0f, s.esw, v);
    v = fmaf(s.bse ? pse : 0.0f, s.ese, v);
    return v * s.mask;
}

}  // namespace vfi
