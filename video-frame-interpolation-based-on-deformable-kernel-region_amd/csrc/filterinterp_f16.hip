// filterinterp_f16.hip -- FilterInterpolation (_ori forward) with fp16 STORAGE of the image and the
// output and fp32 arithmetic (BASELINE.json configs[2]: "fp16 storage / fp32 accum").
//
// Semantics: filterinterpolation_cuda_kernel.cu:2692-2823 applied to the fp16 values widened to
// fp32; flow and filter stay fp32; the fp32 result is rounded to fp16 (round to nearest even).
//
//   fi_forward_ori_direct_16<F16Store>   the reference's operation order: bit-exact with the fp32 oracle run on the
//                               widened inputs and rounded once.  Fallback of the staged kernel and its yardstick.
//   fi_forward_ori_lds_f16      fs == 4, the 196-channel case: the tile prologue, channel loop and ladder of
//                               filterinterp_16.h; the products are v_fma_mix_f32 straight from the packed halves.
// Two things differ from the fp32 staged kernel, both inside the stated fp16 tolerance (2e-3 for
// images in [0, 1], tests/test_gpu_parity.py):
//   * the pixel is one 16-term dot product with weights filter x bilinear weight folded once per
//     tile (same products as the reference, one accumulation chain instead of four + blend);
//   * a pixel whose taps leave the image left or right (its window is moved inside) gets the weights
//     of the clamped taps added onto the column they clamp to.
#include "filterinterp_16.h"

#include <hip/hip_fp16.h>

namespace vfi {

// fp32 -> fp16, round to nearest even, of a value that has first been rounded to fp32.  The empty asm
// keeps hipcc from folding the conversion into the last FMA (v_fma_mixlo_f16 rounds the exact FMA
// result to fp16 once; "the fp32 op, then .half()" rounds twice, and ties can fall the other way).
__device__ __forceinline__ __half f16_store_value(float v) {
    asm volatile("" : "+v"(v));
    return __float2half_rn(v);
}

// the direct kernel's storage policy (S of fi_forward_ori_direct_16, filterinterp_16.h): every quadrant chain starts from 0, whatever the
// filter size; the validity test comes before the cell (fi_point changes this instance's code)
struct F16Store {
    typedef __half E;
    static constexpr bool PRODUCT_FIRST = false;
    static constexpr bool POINT_THEN_CELL = true;
    static __device__ __forceinline__ float widen(__half v) { return __half2float(v); }
    static __device__ __forceinline__ __half store(float v) { return f16_store_value(v); }
};

// ------------------------------------------------------------------ LDS-staged kernel, fs == 4

struct F16Pixel {
    bool valid, inimg;
    int lbase;              // half index of the window origin inside a staged window (row pitch 2 * pitch)
    unsigned pix;
    float g[16];            // folded tap weights on the (possibly moved) 4x4 window
};

// the two halves of a packed dword, widened (v_fma_mix_f32 reads them in place)
__device__ __forceinline__ float f16_lo(unsigned d) { return __half2float(__ushort_as_half((unsigned short)(d & 0xffffu))); }
__device__ __forceinline__ float f16_hi(unsigned d) { return __half2float(__ushort_as_half((unsigned short)(d >> 16))); }

__global__ __launch_bounds__(FI16_THREADS, 4) void fi_forward_ori_lds_f16(
    const __half* __restrict__ in1, const float* __restrict__ in2, const float* __restrict__ in3,
    __half* __restrict__ out, int channel, int h, int w,
    vfi_strides s1, vfi_strides s2, vfi_strides s3,
    int tiles_x, int tiles_y, int ntiles, int ch_per_group) {
    __shared__ unsigned lds[FI16_HDR + FI16_RING_DWORDS];
    int* box = reinterpret_cast<int*>(lds);

    const int tile = fi_xcd_tile<unsigned>(blockIdx.x);
    if (tile >= ntiles) return;
    const int tid = threadIdx.x;
    const Fi16Tile t = fi16_tile(tile, tid, tiles_x, tiles_y, channel, ch_per_group);
    const int b = t.b, c_begin = t.c_begin, c_end = t.c_end, x = t.x, y0 = t.y0;

    F16Pixel px[FI16_PX];
    int L[FI16_PX], Lc[FI16_PX], T[FI16_PX];
    float alpha[FI16_PX], beta[FI16_PX];
    Fi16Box own;
#pragma unroll
    for (int p = 0; p < FI16_PX; ++p) {
        const int y = y0 + p * FI16_PASS_ROWS;
        px[p].inimg = x < w && y < h;
        px[p].pix = (unsigned)(y * (int)s1.h + x);
        float fx = 0.0f, fy = 0.0f;                         // (fi_flow_at changes this kernel's code)
        if (px[p].inimg) {
            const float* flow = in2 + (int64_t)b * s2.b + (int64_t)y * s2.h + x;
            fx = flow[0];
            fy = flow[s2.c];
        }
        const Fi16Tap g = fi16_tap(fx, fy, x, y, w, h, px[p].inimg, own);
        px[p].valid = g.valid;
        L[p] = g.L; Lc[p] = g.Lc; T[p] = g.T;
        alpha[p] = g.alpha; beta[p] = g.beta;
    }

    if (tid == 0) fi_box_clear(box);
    __syncthreads();
    const FiWindow win = fi16_window(box, tid, own, h, w, (int)s1.h);
    const int n = win.pitch * win.bh;
    const int kmax = (n + FI16_THREADS - 1) / FI16_THREADS;      // (as fi_forward_ori_lds_bf16 forms it)

    // ---- folded tap weights: filter tap x bilinear quadrant weight, clamped columns merged
#pragma unroll
    for (int p = 0; p < FI16_PX; ++p) {
        px[p].lbase = fi16_lbase(px[p].valid, Lc[p], T[p], win);
#pragma unroll
        for (int k = 0; k < 16; ++k) px[p].g[k] = 0.0f;
        if (px[p].valid) {
            const float* fpx = in3 + (int64_t)b * s3.b + (int64_t)(y0 + p * FI16_PASS_ROWS) * s3.h + x;
            const float wx[2] = { 1.0f - alpha[p], alpha[p] }, wy[2] = { 1.0f - beta[p], beta[p] };
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float wgt = fpx[(int64_t)(r * 4 + k) * s3.c] * (wx[k >> 1] * wy[r >> 1]);
                    const int kk = clampi(L[p] + k, 0, w - 1) - Lc[p];          // 0..3
#pragma unroll
                    for (int q = 0; q < 4; ++q) px[p].g[r * 4 + q] += (kk == q) ? wgt : 0.0f;
                }
        }
    }

    const __half* img = in1 + (int64_t)b * s1.b;
    __half* dst = out + (int64_t)b * s1.b;
    unsigned* ring = lds + FI16_HDR;
    // the pixel's value: one 16-term dot product on the moved window
    auto value = [&](int p, auto&& row) {
        float acc = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            unsigned e0, e1;
            row(r, e0, e1);
            acc = fmaf(f16_lo(e0), px[p].g[r * 4 + 0], acc);
            acc = fmaf(f16_hi(e0), px[p].g[r * 4 + 1], acc);
            acc = fmaf(f16_lo(e1), px[p].g[r * 4 + 2], acc);
            acc = fmaf(f16_hi(e1), px[p].g[r * 4 + 3], acc);
        }
        return __half_as_ushort(f16_store_value(acc));
    };
    if (kmax > FI16_KTOP) {
        // window too large for LDS: the same dot product gathered from global memory
#pragma unroll
        for (int p = 0; p < FI16_PX; ++p) {
            if (px[p].valid) {
                for (int c = c_begin; c < c_end; ++c) {
                    const __half* plane = img + (int64_t)c * s1.c;
                    float acc = 0.0f;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const __half* row = plane + (int64_t)clampi(T[p] + r, 0, h - 1) * s1.h + Lc[p];
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc = fmaf(__half2float(row[k]), px[p].g[r * 4 + k], acc);
                    }
                    dst[(int64_t)c * s1.c + px[p].pix] = f16_store_value(acc);
                }
            } else if (px[p].inimg) {
                fi_copy_through(img, dst, px[p].pix, c_begin, c_end, s1.c);
            }
        }
        return;
    }
#define F16_RUN(K) fi16_run_channels<K, false>(img, dst, s1.c, 0, c_begin, c_end, tid, win, px, ring, value)
    FI16_LADDER(F16_RUN);
#undef F16_RUN
}

}  // namespace vfi

using namespace vfi;

extern "C" int vfi_filterinterp_forward_ori_f16_direct(const void* input1, const float* input2, const float* input3,
                                                        void* output, int batch, int channel, int h, int w,
                                                        int filter_channels, vfi_strides s1, vfi_strides s2,
                                                        vfi_strides s3, vfi_stream_t stream) {
    if (batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || filter_channels <= 0) return VFI_ERR_SHAPE;
    if (!input1 || !input2 || !input3 || !output) return VFI_ERR_SHAPE;
    const int fs = fi_filter_size(filter_channels);
    hipLaunchKernelGGL(fi_forward_ori_direct_16<F16Store>, pixel_grid(w, h, batch), dim3(VFI_TX, VFI_TY, 1), 0, (hipStream_t)stream,
                       (const __half*)input1, input2, input3, (__half*)output, channel, h, w, fs, s1, s2, s3);
    return launch_status();
}

extern "C" int vfi_filterinterp_forward_ori_f16(const void* input1, const float* input2, const float* input3,
                                                 void* output, int batch, int channel, int h, int w,
                                                 int filter_channels, vfi_strides s1, vfi_strides s2, vfi_strides s3,
                                                 vfi_stream_t stream) {
    if (batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || filter_channels <= 0) return VFI_ERR_SHAPE;
    if (!input1 || !input2 || !input3 || !output) return VFI_ERR_SHAPE;
    const Fi16Plan plan = fi16_launch_plan(input1, s1, h, w, batch, channel, filter_channels);
    if (!plan.staged)
        return vfi_filterinterp_forward_ori_f16_direct(input1, input2, input3, output, batch, channel, h, w,
                                                       filter_channels, s1, s2, s3, stream);
    hipLaunchKernelGGL(fi_forward_ori_lds_f16, dim3((unsigned)fi_xcd_grid(plan.ntiles), (unsigned)plan.split.groups, 1),
                       dim3(FI16_THREADS, 1, 1), 0, (hipStream_t)stream, (const __half*)input1, input2, input3, (__half*)output,
                       channel, h, w, s1, s2, s3, plan.tiles_x, plan.tiles_y, plan.ntiles, plan.split.ch_per_group);
    return launch_status();
}
