// rectify_head_bf16.hip -- the "head" of rectifyNet's input on bfloat16 storage, one launch for gfx950: the blend, the two
// warped frames and the flows and filters that pass through (networks/DAIN_slowmotion.py:177-181, channels 0 .. 12 + 2 fs^2
// at three frame channels), written as bfloat16 into a channel range of the network's input; the blend also as float32.
//
// The float32 path (vfi_filterinterp_blend_forward) runs one side, then the other with a blend epilogue that reads the first
// side's result back from memory.  Read back as bfloat16 that result would be a rounded one, and the blend is formed from the
// unrounded values: here a lane holds both sides' values of its pixels in registers when it blends.  The arithmetic is that
// of fi_blend_forward (glue.hip) through the same helpers -- fi_side, fi4_value, fi_side_value -- and every value is rounded
// once, to nearest even, as it is stored.
//
// A lane owns two horizontally adjacent pixels (x0 even): the flows and the filters -- 36 of the 45 channels at fs = 4, read
// exactly once and stored exactly once -- move as 8-byte loads and 4-byte stores of bfloat16 pairs.  PAIRS is decided on the
// host from the bases and the strides (every row start of every tensor read or written pairwise is aligned); without it, or
// for the lone last pixel of an odd row, the accesses are single elements.  The bits are the same either way.
#include "bf16.h"
#include "filterinterp_dev.h"

namespace vfi {

constexpr int RH_PX = 2;                                     // pixels of a lane

// N = 1 or 2 elements of a row; VEC (N == 2 only): as one access of 2 N or 4 N bytes, the row start being aligned to it
template <bool VEC, int N>
__device__ __forceinline__ void rh_load(const float* __restrict__ p, float (&v)[N]) {
    if constexpr (VEC) {
        const f32x2 t = *reinterpret_cast<const f32x2*>(p);
        v[0] = t.x; v[1] = t.y;
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = p[i];
    }
}
// bf16_rne of v into a row of the head
template <bool VEC, int N>
__device__ __forceinline__ void rh_store(bf16_t* __restrict__ p, const float (&v)[N]) {
    if constexpr (VEC) {
        *reinterpret_cast<unsigned*>(p) = bf16_pack_rne(v[0], v[1]);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) p[i] = bf16_rne(v[i]);
    }
}
template <bool VEC, int N>
__device__ __forceinline__ void rh_store(float* __restrict__ p, const float (&v)[N]) {
    if constexpr (VEC) {
        *reinterpret_cast<f32x2*>(p) = f32x2{v[0], v[1]};
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) p[i] = v[i];
    }
}

// The N pixels (x0 .. x0 + N - 1, y) of batch item b.  Head channels, `channel` = C frame channels and fc filter channels:
// blend [0, C), out0 [C, 2C), out2 [2C, 3C), flow0 [3C, 3C + 2), flow2 [3C + 2, 3C + 4), filt0 [3C + 4, 3C + 4 + fc), filt2
// [3C + 4 + fc, 3C + 4 + 2 fc): the order of fused.rectify_channels.  blend32 (strides sb) may be null.
template <bool PAIRS, int N>
__device__ __forceinline__ void rh_pixels(
    const float* __restrict__ ref0, const float* __restrict__ ref2, const float* __restrict__ flow0,
    const float* __restrict__ flow2, const float* __restrict__ filt0, const float* __restrict__ filt2,
    bf16_t* __restrict__ head, float* __restrict__ blend32, int channel, int h, int w, int fs, int fc, float w0, float w2,
    const vfi_strides& sr, const vfi_strides& sf, const vfi_strides& sk, const vfi_strides& sh, const vfi_strides& sb,
    int b, int x0, int y) {
    constexpr bool VEC = PAIRS && N == RH_PX;
    const int64_t fo = (int64_t)b * sf.b + (int64_t)y * sf.h + x0, ko = (int64_t)b * sk.b + (int64_t)y * sk.h + x0;
    bf16_t* __restrict__ hp = head + (int64_t)b * sh.b + (int64_t)y * sh.h + x0;
    const float* flows[2] = {flow0 + fo, flow2 + fo};
    const float* filts[2] = {filt0 + ko, filt2 + ko};
    const float* refs[2] = {ref0 + (int64_t)b * sr.b, ref2 + (int64_t)b * sr.b};
    const float wgt[2] = {w0, w2};
    const int hs = (int)sr.h;

    // ---- the flows: through to the head, and each side's geometry per pixel
    FiSide side[2][N];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        float fx[N], fy[N];
        rh_load<VEC>(flows[s], fx);
        rh_load<VEC>(flows[s] + sf.c, fy);
        rh_store<VEC>(hp + (int64_t)(3 * channel + 2 * s) * sh.c, fx);
        rh_store<VEC>(hp + (int64_t)(3 * channel + 2 * s + 1) * sh.c, fy);
#pragma unroll
        for (int p = 0; p < N; ++p) side[s][p] = fi_side(fx[p], fy[p], x0 + p, y, w, h, fs);
    }
    bf16_t* __restrict__ hk[2] = {hp + (int64_t)(3 * channel + 4) * sh.c, hp + (int64_t)(3 * channel + 4 + fc) * sh.c};
    float* __restrict__ bp = blend32 ? blend32 + (int64_t)b * sb.b + (int64_t)y * sb.h + x0 : nullptr;

    // one frame channel: both sides' values of the lane's pixels, stored rounded; the blend from the unrounded values, its
    // two products rounded separately (fi_blend_forward)
    auto emit = [&](int c, const float (&v)[2][N]) {
        rh_store<VEC>(hp + (int64_t)(channel + c) * sh.c, v[0]);
        rh_store<VEC>(hp + (int64_t)(2 * channel + c) * sh.c, v[1]);
        float bl[N];
#pragma unroll
        for (int p = 0; p < N; ++p) {
            const float q0 = v[0][p] * wgt[0], q2 = v[1][p] * wgt[1];
            bl[p] = q0 + q2;
        }
        rh_store<VEC>(hp + (int64_t)c * sh.c, bl);
        if (bp) rh_store<VEC>(bp + (int64_t)c * sb.c, bl);
    };

    if (fs == 4) {
        // the 16 taps of both sides and pixels stay in registers: through to the head, then the channel loop's operands,
        // with the clamped rows and columns hoisted out of that loop as in fi_blend_forward
        float f[2][N][16];
        unsigned ro[2][N][4], co[2][N][4];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                float t[N];
                rh_load<VEC>(filts[s] + (int64_t)k * sk.c, t);
                rh_store<VEC>(hk[s] + (int64_t)k * sh.c, t);
#pragma unroll
                for (int p = 0; p < N; ++p) f[s][p][k] = t[p];
            }
#pragma unroll
            for (int p = 0; p < N; ++p)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    ro[s][p][k] = (unsigned)(clampi(side[s][p].T + k, 0, h - 1) * hs);
                    co[s][p][k] = (unsigned)clampi(side[s][p].L + k, 0, w - 1);
                }
        }
        const unsigned self = (unsigned)(y * hs + x0);
        for (int c = 0; c < channel; ++c) {
            float v[2][N];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const float* plane = refs[s] + (int64_t)c * sr.c;
#pragma unroll
                for (int p = 0; p < N; ++p)
                    v[s][p] = side[s][p].valid ? fi4_value(plane, ro[s][p], co[s][p], f[s][p], side[s][p].alpha, side[s][p].beta)
                                               : plane[self + p];
            }
            emit(c, v);
        }
    } else {
        for (int c = 0; c < channel; ++c) {
            float v[2][N];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const float* plane = refs[s] + (int64_t)c * sr.c;
#pragma unroll
                for (int p = 0; p < N; ++p)
                    v[s][p] = fi_side_value(side[s][p], plane, filts[s] + p, sk.c, hs, h, w, fs, x0 + p, y);
            }
            emit(c, v);
        }
    }
    // the filter channels no tap loop has stored: all of them, or those past the 16 taps of fs == 4 (fc = 17 .. 24)
    for (int k = fs == 4 ? 16 : 0; k < fc; ++k) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float t[N];
            rh_load<VEC>(filts[s] + (int64_t)k * sk.c, t);
            rh_store<VEC>(hk[s] + (int64_t)k * sh.c, t);
        }
    }
}

template <bool PAIRS>
__global__ __launch_bounds__(VFI_TX * VFI_TY) void rectify_head_bf16(
    const float* __restrict__ ref0, const float* __restrict__ ref2, const float* __restrict__ flow0,
    const float* __restrict__ flow2, const float* __restrict__ filt0, const float* __restrict__ filt2,
    bf16_t* __restrict__ head, float* __restrict__ blend32, int channel, int h, int w, int fs, int fc, float w0, float w2,
    vfi_strides sr, vfi_strides sf, vfi_strides sk, vfi_strides sh, vfi_strides sb) {
    const int x0 = (blockIdx.x * VFI_TX + threadIdx.x) * RH_PX;
    const int y = blockIdx.y * VFI_TY + threadIdx.y;
    if (x0 >= w || y >= h) return;
    // a lane's two pixels, or the lone last pixel of an odd row
    if (x0 + 1 < w)
        rh_pixels<PAIRS, RH_PX>(ref0, ref2, flow0, flow2, filt0, filt2, head, blend32, channel, h, w, fs, fc, w0, w2, sr, sf, sk, sh,
                                sb, blockIdx.z, x0, y);
    else
        rh_pixels<PAIRS, 1>(ref0, ref2, flow0, flow2, filt0, filt2, head, blend32, channel, h, w, fs, fc, w0, w2, sr, sf, sk, sh, sb,
                            blockIdx.z, x0, y);
}

// every row start of a tensor with strides s, from a base aligned to `bytes`, is aligned to `bytes` = two elements
static bool rh_rows_pairwise(const void* base, const vfi_strides& s, unsigned bytes) {
    return (reinterpret_cast<uintptr_t>(base) & (bytes - 1)) == 0 && ((s.b | s.c | s.h) & 1) == 0;
}

}  // namespace vfi

using namespace vfi;

extern "C" int vfi_rectify_head_forward_bf16(const float* ref0, const float* ref2, const float* flow0, const float* flow2,
                                              const float* filt0, const float* filt2, void* head_bf16, float* blend_f32,
                                              int batch, int channel, int h, int w, int filter_channels, float w0, float w2,
                                              vfi_strides s_ref, vfi_strides s_flow, vfi_strides s_filt, vfi_strides s_head,
                                              vfi_strides s_blend, vfi_stream_t stream) {
    if (batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || filter_channels <= 0) return VFI_ERR_SHAPE;
    if (!ref0 || !ref2 || !flow0 || !flow2 || !filt0 || !filt2 || !head_bf16) return VFI_ERR_SHAPE;
    if (s_head.h != s_ref.h || batch > 65535) return VFI_ERR_SHAPE;
    const int fs = fi_filter_size(filter_channels);
    const dim3 grid((unsigned)((w + RH_PX * VFI_TX - 1) / (RH_PX * VFI_TX)), (unsigned)((h + VFI_TY - 1) / VFI_TY), (unsigned)batch);
    if (grid.y > 65535) return VFI_ERR_SHAPE;
    const bool pairs = rh_rows_pairwise(flow0, s_flow, 8) && rh_rows_pairwise(flow2, s_flow, 8) &&
                       rh_rows_pairwise(filt0, s_filt, 8) && rh_rows_pairwise(filt2, s_filt, 8) &&
                       rh_rows_pairwise(head_bf16, s_head, 4) && (!blend_f32 || rh_rows_pairwise(blend_f32, s_blend, 8));
    const auto kernel = pairs ? rectify_head_bf16<true> : rectify_head_bf16<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(VFI_TX, VFI_TY, 1), 0,
                       (hipStream_t)stream, ref0, ref2, flow0, flow2, filt0, filt2, static_cast<bf16_t*>(head_bf16), blend_f32,
                       channel, h, w, fs, filter_channels, w0, w2, s_ref, s_flow, s_filt, s_head, s_blend);
    return launch_status();
}
