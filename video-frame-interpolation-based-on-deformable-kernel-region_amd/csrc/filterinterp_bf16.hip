// filterinterp_bf16.hip -- FilterInterpolation (_ori forward) on bfloat16 STORAGE of the image and the output: the context
// warp of a network that runs under bfloat16 autocast (FilterInterpolate_ctx, C = 196).
//
// Contract (bf16.h): the 16-bit patterns are widened exactly on load, the arithmetic is the float32 kernels' arithmetic --
// per pixel the four 2x2 quadrant chains of fi4_pixel and blend4, clamped taps read as replicated VALUES -- and the result
// is rounded once, to nearest even.  Every output element is, bit for bit, bf16_rne of what vfi_filterinterp_forward_ori
// writes for the widened image ("cast up, float32 warp, cast down" without the casts); NaN stays NaN; an invalid pixel
// copies the input's bits through.  Flow and filter stay float32.  Nothing is folded: the fp16 kernel's single 16-term dot
// product and its merged weights of clamped columns (filterinterp_f16.hip) would each break that equality.
//
//   fi_forward_ori_direct_16<Bf16Store, vfi_strides>   the fallback and the yardstick (filterinterp_16.h).
//   fi_forward_ori_lds_bf16     fs == 4: the tile prologue, channel loop, ladder and launch plan of filterinterp_16.h, with
//                               the widening a shift / a mask and the arithmetic fi4_pixel.
// A window that crosses the left or right border is moved inside the image (filterinterp_16.h); the pixel then picks, per
// tap, the moved window's column that the clamped tap names (validity bounds the move to one column on the left, two on
// the right).  That selection is compiled into a second instance of the channel loop (EDGE), taken by the tiles in which
// some valid pixel's window was moved; the interior tiles' loop does not contain it.
// Both kernels write through a layout of their own (so.h == s1.h; batch and channel strides free), one 2-byte store per
// element: the destination may be a channel slice of a wider buffer that is only 2-byte aligned.
#include "bf16.h"
#include "filterinterp_16.h"
// the image-only multi-flow backward's kernels and launcher, templates on the gradients' storage: instantiated below
#include "filterinterp_ctx_bwd.h"

namespace vfi {

// the direct kernel's storage policy (S of fi_forward_ori_direct_16, filterinterp_16.h): fs == 4 starts each quadrant chain with a product
// (fi4_pixel), every other size from 0 (quadrants_generic), as the float32 entry's kernels do
struct Bf16Store {
    typedef bf16_t E;
    static constexpr bool PRODUCT_FIRST = true;
    static constexpr bool POINT_THEN_CELL = false;
    static __device__ __forceinline__ float widen(bf16_t v) { return bf16_widen(v); }
    static __device__ __forceinline__ bf16_t store(float v) { return bf16_rne(v); }
};

// ------------------------------------------------------------------ LDS-staged kernel, fs == 4

struct BfPixel {
    bool valid, inimg;
    int lbase;              // element index of the (moved) window's origin inside a staged window (row pitch 2 * pitch)
    unsigned sel[2];        // EDGE: v_perm selectors that replicate the moved window's columns into the pixel's own taps
    unsigned pix;
    float alpha, beta;
    float f[16];            // the filter taps
};

// the two elements of a packed dword, widened: a shift, a mask
__device__ __forceinline__ float bf16_lo(unsigned d) { return __uint_as_float(d << 16); }
__device__ __forceinline__ float bf16_hi(unsigned d) { return __uint_as_float(d & 0xffff0000u); }

// The channel loop (filterinterp_16.h) with the pixel's arithmetic fi4_pixel on the widened taps.  EDGE, the instance of the
// tiles with a moved window: tap k of the pixel's own window is column clamp(k + shift, 0, 3) of the moved one -- the
// replicated value, picked out of the eight bytes {e1, e0} by the pixel's two selectors.
template <int K, bool EDGE>
__device__ __forceinline__ void bf16_run_channels(const bf16_t* __restrict__ img, bf16_t* __restrict__ out, int64_t cs, int64_t cso,
                                                  int c_begin, int c_end, int tid, const FiWindow& win,
                                                  const BfPixel (&px)[FI16_PX], unsigned* __restrict__ ring) {
    fi16_run_channels<K, true>(img, out, cs, cso, c_begin, c_end, tid, win, px, ring,
                               [&](int p, auto&& row) {
        float v[16];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            unsigned e0, e1;
            row(r, e0, e1);
            const unsigned o0 = EDGE ? __builtin_amdgcn_perm(e1, e0, px[p].sel[0]) : e0;
            const unsigned o1 = EDGE ? __builtin_amdgcn_perm(e1, e0, px[p].sel[1]) : e1;
            v[r * 4 + 0] = bf16_lo(o0); v[r * 4 + 1] = bf16_hi(o0);
            v[r * 4 + 2] = bf16_lo(o1); v[r * 4 + 3] = bf16_hi(o1);
        }
        return bf16_rne(fi4_pixel(v, px[p].f, px[p].alpha, px[p].beta));
    });
}

__global__ __launch_bounds__(FI16_THREADS, 4) void fi_forward_ori_lds_bf16(
    const bf16_t* __restrict__ in1, const float* __restrict__ in2, const float* __restrict__ in3,
    bf16_t* __restrict__ out, int channel, int h, int w,
    vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides so,
    int tiles_x, int tiles_y, int ntiles, int ch_per_group) {
    __shared__ unsigned lds[FI16_HDR + FI16_RING_DWORDS];
    int* box = reinterpret_cast<int*>(lds);                 // [0..3] the bounding box, [4] "a window of this tile was moved"

    const int tile = fi_xcd_tile<unsigned>(blockIdx.x);
    if (tile >= ntiles) return;
    const int tid = threadIdx.x;
    const Fi16Tile t = fi16_tile(tile, tid, tiles_x, tiles_y, channel, ch_per_group);
    const int b = t.b, c_begin = t.c_begin, c_end = t.c_end, x = t.x, y0 = t.y0;

    BfPixel px[FI16_PX];
    int L[FI16_PX], Lc[FI16_PX], T[FI16_PX];
    Fi16Box own;
    bool moved = false;
#pragma unroll
    for (int p = 0; p < FI16_PX; ++p) {
        const int y = y0 + p * FI16_PASS_ROWS;
        px[p].inimg = x < w && y < h;
        px[p].pix = (unsigned)(y * (int)s1.h + x);
        const FiFlow fl = fi_flow_at(in2, s2, b, x, y, px[p].inimg);
        const Fi16Tap g = fi16_tap(fl.fx, fl.fy, x, y, w, h, px[p].inimg, own);
        px[p].valid = g.valid;
        L[p] = g.L; Lc[p] = g.Lc; T[p] = g.T;
        // the window's own first column less the moved window's: -1 (left border), 0, 1 or 2 (right border); element q of
        // {e1, e0} is bytes 2q, 2q + 1
        const int shift = L[p] - Lc[p];
        unsigned q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const unsigned e = (unsigned)clampi(k + shift, 0, 3); q[k] = ((2u * e + 1u) << 8) | (2u * e); }
        px[p].sel[0] = q[0] | (q[1] << 16);
        px[p].sel[1] = q[2] | (q[3] << 16);
        moved = moved || (g.valid && shift != 0);
        px[p].alpha = g.alpha; px[p].beta = g.beta;
    }

    if (tid == 0) { fi_box_clear(box); box[4] = 0; }
    __syncthreads();
    if (moved) box[4] = 1;
    const FiWindow win = fi16_window(box, tid, own, h, w, (int)s1.h);
    const bool edge = box[4] != 0;

#pragma unroll
    for (int p = 0; p < FI16_PX; ++p) {
        px[p].lbase = fi16_lbase(px[p].valid, Lc[p], T[p], win);
        const float* fpx = in3 + (int64_t)b * s3.b + (int64_t)(y0 + p * FI16_PASS_ROWS) * s3.h + x;
#pragma unroll
        for (int k = 0; k < 16; ++k) px[p].f[k] = px[p].valid ? fpx[(int64_t)k * s3.c] : 0.0f;
    }

    const bf16_t* img = in1 + (int64_t)b * s1.b;
    bf16_t* dst = out + (int64_t)b * so.b;
    const int n = win.pitch * win.bh;
    const int kmax = (n + FI16_THREADS - 1) / FI16_THREADS;      // (formed in a helper it changes this kernel's code)
    if (kmax > FI16_KTOP) {
        // window too large for LDS: the same chains gathered from global memory, rows and columns clamped per tap
#pragma unroll
        for (int p = 0; p < FI16_PX; ++p) {
            if (px[p].valid) {
                unsigned ro[4], co[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    ro[k] = (unsigned)(clampi(T[p] + k, 0, h - 1) * (int)s1.h);
                    co[k] = (unsigned)clampi(L[p] + k, 0, w - 1);
                }
                for (int c = c_begin; c < c_end; ++c) {
                    const bf16_t* plane = img + (int64_t)c * s1.c;
                    float v[16];
#pragma unroll
                    for (int k = 0; k < 16; ++k) v[k] = bf16_widen(plane[ro[k >> 2] + co[k & 3]]);
                    dst[(int64_t)c * so.c + px[p].pix] = bf16_rne(fi4_pixel(v, px[p].f, px[p].alpha, px[p].beta));
                }
            } else if (px[p].inimg) {
                fi_copy_through_to<true>(img, dst, px[p].pix, c_begin, c_end, s1.c, so.c);
            }
        }
        return;
    }

    unsigned* ring = lds + FI16_HDR;
#define BF_RUN(K) (edge ? bf16_run_channels<K, true>(img, dst, s1.c, so.c, c_begin, c_end, tid, win, px, ring) \
                        : bf16_run_channels<K, false>(img, dst, s1.c, so.c, c_begin, c_end, tid, win, px, ring))
    FI16_LADDER(BF_RUN);
#undef BF_RUN
}

// one flow, direct kernel
static int forward_bf16_direct(const bf16_t* input1, const float* flow, const float* input3, bf16_t* output, int batch, int channel,
                               int h, int w, int filter_channels, vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides so,
                               hipStream_t st) {
    hipLaunchKernelGGL((fi_forward_ori_direct_16<Bf16Store, vfi_strides>), pixel_grid(w, h, batch), dim3(VFI_TX, VFI_TY, 1), 0, st,
                       input1, flow, input3, output, channel, h, w, fi_filter_size(filter_channels), s1, s2, s3, so);
    return launch_status();
}

// one flow: the staged kernel where the image's layout allows dword staging, else the direct kernel
static int forward_bf16(const bf16_t* input1, const float* flow, const float* input3, bf16_t* output, int batch, int channel, int h,
                        int w, int filter_channels, vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides so, hipStream_t st) {
    const Fi16Plan plan = fi16_launch_plan(input1, s1, h, w, batch, channel, filter_channels);
    if (!plan.staged)
        return forward_bf16_direct(input1, flow, input3, output, batch, channel, h, w, filter_channels, s1, s2, s3, so, st);
    hipLaunchKernelGGL(fi_forward_ori_lds_bf16, dim3((unsigned)fi_xcd_grid(plan.ntiles), (unsigned)plan.split.groups, 1),
                       dim3(FI16_THREADS, 1, 1), 0, st, input1, flow, input3, output, channel, h, w, s1, s2, s3, so, plan.tiles_x,
                       plan.tiles_y, plan.ntiles, plan.split.ch_per_group);
    return launch_status();
}

// the entry points' argument checks (those of vfi_filterinterp_forward_ori_multi_to), then one launch per flow
static int forward_bf16_multi(bool direct, const void* input1, const float* const* flows, const float* input3, void* const* outputs,
                              int nflows, int batch, int channel, int h, int w, int filter_channels, vfi_strides s1, vfi_strides s2,
                              vfi_strides s3, vfi_strides so, vfi_stream_t stream) {
    if (nflows <= 0 || !flows || !outputs || batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || filter_channels <= 0)
        return VFI_ERR_SHAPE;
    if (!input1 || !input3) return VFI_ERR_SHAPE;
    for (int t = 0; t < nflows; ++t)
        if (!flows[t] || !outputs[t]) return VFI_ERR_SHAPE;
    if (so.h != s1.h || batch > 65535) return VFI_ERR_SHAPE;
    for (int t = 0; t < nflows; ++t) {
        const int err = (direct ? forward_bf16_direct : forward_bf16)((const bf16_t*)input1, flows[t], input3, (bf16_t*)outputs[t], batch,
                                                                      channel, h, w, filter_channels, s1, s2, s3, so, (hipStream_t)stream);
        if (err != VFI_OK) return err;
    }
    return VFI_OK;
}

}  // namespace vfi

using namespace vfi;

extern "C" int vfi_filterinterp_forward_ori_multi_to_bf16_direct(const void* input1_bf16, const float* const* flows,
                                                                  const float* input3, void* const* outputs_bf16, int nflows,
                                                                  int batch, int channel, int h, int w, int filter_channels,
                                                                  vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides s_out,
                                                                  vfi_stream_t stream) {
    return forward_bf16_multi(true, input1_bf16, flows, input3, outputs_bf16, nflows, batch, channel, h, w, filter_channels, s1, s2,
                              s3, s_out, stream);
}

extern "C" int vfi_filterinterp_forward_ori_multi_to_bf16(const void* input1_bf16, const float* const* flows, const float* input3,
                                                           void* const* outputs_bf16, int nflows, int batch, int channel, int h,
                                                           int w, int filter_channels, vfi_strides s1, vfi_strides s2,
                                                           vfi_strides s3, vfi_strides s_out, vfi_stream_t stream) {
    return forward_bf16_multi(false, input1_bf16, flows, input3, outputs_bf16, nflows, batch, channel, h, w, filter_channels, s1, s2,
                              s3, s_out, stream);
}

// The backward of the context warp on bfloat16 gradients: fi_ctx_backward4_lds / fi_ctx_backward_px reading a bfloat16
// gradient row widened (GradBf16 in the max-scan, so the scale is the float32 call's), the same tile classes, channel
// groups, CB_NT carries and fallbacks, one fixed-point accumulation over all flows, and gradacc_finish_bf16 WRITING every
// cell: bf16_rne of what vfi_filterinterp_backward_ori_image_multi writes for the widened gradients, bit for bit.
extern "C" int vfi_filterinterp_backward_ori_image_multi_bf16(const float* const* flows, const float* input3,
                                                               const void* const* gradoutputs_bf16, void* gradinput1_bf16,
                                                               int nflows, int batch, int channel, int h, int w,
                                                               int filter_channels, vfi_strides s1, vfi_strides s2, vfi_strides s3,
                                                               vfi_strides sg, vfi_stream_t stream) {
    return backward_image_multi<bf16_t>(flows, input3, reinterpret_cast<const bf16_t* const*>(gradoutputs_bf16),
                                        static_cast<bf16_t*>(gradinput1_bf16), nflows, batch, channel, h, w, filter_channels, s1,
                                        s2, s3, sg, stream);
}
