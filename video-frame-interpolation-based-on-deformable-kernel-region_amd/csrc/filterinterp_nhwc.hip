// filterinterp_nhwc.hip -- FilterInterpolation (_ori forward) on channels_last (NHWC) images: the context warp of a network
// that keeps its activations in torch.channels_last, float32 or bfloat16 storage, without the two layout copies around
// the NCHW entries.  Forward only.
//
// Contract: every output element is, bit for bit, what the NCHW entry writes for the same logical tensors --
// vfi_filterinterp_forward_ori_multi in float32, vfi_filterinterp_forward_ori_multi_to_bf16 in bfloat16 (bf16_rne of the
// float32 result on the widened image).  The arithmetic is not restated: the pixel's geometry is fi_geom, fs == 4 is
// fi4_pixel (four quadrant chains that start with a product, then blend4), every other size accumulates quadrant by
// quadrant from 0 in the order of quadrants_generic and ends in blend4.  (quadrants_generic itself reads float planes with
// column stride 1; here a column is s1.w elements away and the element may be 16 bits wide, so the loop is written over a
// tap accessor, as fi_forward_ori_direct_16 writes it for 16-bit storage.)  NaN stays where it is; an invalid pixel copies
// the input's bits through.
//
// In NHWC a tap is one contiguous run of C elements, so lanes run along CHANNELS first: a work item is one pixel and one
// chunk of V channels, and the items of a tile of FN_TW x FN_TH pixels are dealt flat over the workgroup's threads (C = 196
// in chunks of 4 is 49 items per pixel: a wave holds one pixel and a piece of the next instead of idling 15 lanes).  What
// depends on the pixel alone -- flow, validity, cell, alpha / beta, the clamped tap rows and columns, the 16 filter taps --
// is formed once per pixel by four threads and shared through LDS; after one barrier the channel loop has none.  Border
// clamping is a per-tap address: there is no moved window.
//
//   fi_forward_nhwc4<S, V>     fs == 4; V elements per item: 16, 8, 4 bytes or one element, whatever the bases and the
//                              strides of the image and of EVERY destination allow (fn_vector_width).  A channel tail
//                              (C not a multiple of V) is the last chunk, element by element.  Every V gives the same bits.
//   fi_forward_nhwc_any<S>     every other filter size, one element per item.
// Flow and filter are float32 and addressed with four strides each (2 + filter_channels scalar reads per pixel, shared by
// all channels): NCHW and channels_last are both accepted.  One launch per flow.
#include "bf16.h"
#include "filterinterp_dev.h"

namespace vfi {

// Tile: measured at padded 1080p, C = 196, smooth flow, three offsets: 32 x 4 4.49 / 3.30 ms (float32 /
// bfloat16), 16 x 4 4.87 / 3.34, 8 x 8 4.97 / 3.39, 32 x 2 4.95 / 3.38, 64 x 1 5.11 / 3.38.
#define FN_TW 32
#define FN_TH 4
#define FN_PIXELS (FN_TW * FN_TH)
// (four threads form one pixel's record)
#define FN_THREADS (4 * FN_PIXELS)

// storage policies: the element, its exact widening and its one rounding
struct NhwcF32 {
    typedef float E;
    static __device__ __forceinline__ float widen(float v) { return v; }
    static __device__ __forceinline__ float store(float v) { return v; }
};
struct NhwcBf16 {
    typedef bf16_t E;
    static __device__ __forceinline__ float widen(bf16_t v) { return bf16_widen(v); }
    static __device__ __forceinline__ bf16_t store(float v) { return bf16_rne(v); }
};

enum { FN_OUTSIDE = 0, FN_COPY = 1, FN_WARP = 2 };

// what a pixel's items share.  Offsets are in elements from the batch item's first element.
struct alignas(16) FnPixel {
    int64_t src, dst;                               // the pixel itself in the image / in the destination
    int state, ix, iy, pad;                         // (ix, iy: fi_forward_nhwc_any)
    float alpha, beta;
    int64_t fpx;                                    // the pixel's first filter tap (fi_forward_nhwc_any)
};
struct alignas(16) FnPixel4 {
    FnPixel p;
    int64_t ro[4], co[4];                           // the clamped tap rows and columns
    float f[16];
};

// the tile and the pixel a thread of the prologue works on (four threads per pixel: q = tid & 3)
struct FnWhere { int b, x, y; bool inimg; };
__device__ __forceinline__ FnWhere fn_where(int tile, int tid, int tiles_x, int tiles_y, int channel, int h, int w) {
    const FiTile t = fi_tile_at(tile, tiles_x, tiles_y, channel, channel);
    const int p = tid >> 2;
    FnWhere o;
    o.b = t.b;
    o.x = t.tx * FN_TW + (p % FN_TW);
    o.y = t.ty * FN_TH + (p / FN_TW);
    o.inimg = o.x < w && o.y < h;
    return o;
}

// the flow of pixel (x, y), four strides (fi_flow_at's: 0 for a thread outside the image)
__device__ __forceinline__ FiFlow fn_flow_at(const float* __restrict__ in2, const vfi_strides4& s2, int b, int x, int y, bool inimg) {
    FiFlow f{0.0f, 0.0f};
    if (inimg) {
        const float* flow = in2 + (int64_t)b * s2.b + (int64_t)y * s2.h + (int64_t)x * s2.w;
        f.fx = flow[0];
        f.fy = flow[s2.c];
    }
    return f;
}

__device__ __forceinline__ void fn_record(FnPixel& r, const FnWhere& at, const FiGeom& g, const vfi_strides_nhwc& s1,
                                          const vfi_strides_nhwc& so, const vfi_strides4& s3) {
    r.src = (int64_t)at.y * s1.h + (int64_t)at.x * s1.w;
    r.dst = (int64_t)at.y * so.h + (int64_t)at.x * so.w;
    r.state = !at.inimg ? FN_OUTSIDE : g.valid ? FN_WARP : FN_COPY;
    r.ix = g.ix; r.iy = g.iy; r.pad = 0;
    r.alpha = g.alpha; r.beta = g.beta;
    r.fpx = (int64_t)at.y * s3.h + (int64_t)at.x * s3.w;
}

// Items of a tile, dealt flat: item i is pixel i / chunks, chunk i % chunks; a thread takes items tid, tid + FN_THREADS, ...
// and keeps (pixel, chunk) running, so the one integer division is per thread and tile.
struct FnItems {
    int pixel, chunk, dq, dr, chunks;
    __device__ __forceinline__ FnItems(int tid, int chunks_) : chunks(chunks_) {
        pixel = tid / chunks; chunk = tid - pixel * chunks;
        dq = FN_THREADS / chunks; dr = FN_THREADS - dq * chunks;
    }
    __device__ __forceinline__ bool live() const { return pixel < FN_PIXELS; }
    __device__ __forceinline__ void next() {
        chunk += dr; pixel += dq;
        if (chunk >= chunks) { chunk -= chunks; ++pixel; }
    }
};

// ------------------------------------------------------------------ fs == 4

template <typename S, int V>
__global__ __launch_bounds__(FN_THREADS) void fi_forward_nhwc4(
    const typename S::E* __restrict__ in1, const float* __restrict__ in2, const float* __restrict__ in3,
    typename S::E* __restrict__ out, int channel, int h, int w,
    vfi_strides_nhwc s1, vfi_strides4 s2, vfi_strides4 s3, vfi_strides_nhwc so,
    int tiles_x, int tiles_y, int ntiles) {
    typedef typename S::E E;
    typedef E VE __attribute__((ext_vector_type(V > 1 ? V : 2)));      // (V == 1 never touches it)
    __shared__ FnPixel4 px[FN_PIXELS];

    const int tile = fi_xcd_tile<int>(blockIdx.x);
    if (tile >= ntiles) return;
    const int tid = threadIdx.x;
    const FnWhere at = fn_where(tile, tid, tiles_x, tiles_y, channel, h, w);
    {
        const int q = tid & 3;
        FnPixel4& r = px[tid >> 2];
        const FiFlow fl = fn_flow_at(in2, s2, at.b, at.x, at.y, at.inimg);
        const FiGeom g = fi_geom(fl.fx, fl.fy, at.x, at.y, w, h, at.inimg);
        if (q == 0) fn_record(r.p, at, g, s1, so, s3);
        // tap row / column q of the window at (ix - 1, iy - 1), clamped to the image
        r.ro[q] = (int64_t)clampi(g.iy - 1 + q, 0, h - 1) * s1.h;
        r.co[q] = (int64_t)clampi(g.ix - 1 + q, 0, w - 1) * s1.w;
        if (g.valid) {
            const float* fpx = in3 + (int64_t)at.b * s3.b + (int64_t)at.y * s3.h + (int64_t)at.x * s3.w;
#pragma unroll
            for (int k = 0; k < 4; ++k) r.f[4 * q + k] = fpx[(int64_t)(4 * q + k) * s3.c];
        }
    }
    __syncthreads();

    const E* img = in1 + (int64_t)at.b * s1.b;
    E* dst = out + (int64_t)at.b * so.b;
    for (FnItems it(tid, (channel + V - 1) / V); it.live(); it.next()) {
        const FnPixel4& r = px[it.pixel];
        const int state = r.p.state;
        if (state == FN_OUTSIDE) continue;
        const int c0 = it.chunk * V;
        const E* src = img + r.p.src + c0;
        E* o = dst + r.p.dst + c0;
        const bool whole = V == 1 || c0 + V <= channel;
        if (state == FN_COPY) {
            if constexpr (V > 1) {
                if (whole) { *reinterpret_cast<VE*>(o) = *reinterpret_cast<const VE*>(src); continue; }
            }
            for (int e = 0; e < channel - c0 && e < V; ++e) o[e] = src[e];
            continue;
        }
        float f[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) f[k] = r.f[k];
        const float alpha = r.p.alpha, beta = r.p.beta;
        const E* row[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) row[k] = img + r.ro[k] + c0;
        if constexpr (V > 1) {
            if (whole) {
                VE t[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) t[k] = *reinterpret_cast<const VE*>(row[k >> 2] + r.co[k & 3]);
                VE res;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    float v[16];
#pragma unroll
                    for (int k = 0; k < 16; ++k) v[k] = S::widen(t[k][e]);
                    res[e] = S::store(fi4_pixel(v, f, alpha, beta));
                }
                *reinterpret_cast<VE*>(o) = res;
                continue;
            }
        }
        // one element at a time: the single-element instance, and the channel tail of the others
        for (int e = 0; e < channel - c0 && e < V; ++e) {
            float v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = S::widen(row[k >> 2][r.co[k & 3] + e]);
            o[e] = S::store(fi4_pixel(v, f, alpha, beta));
        }
    }
}

// ------------------------------------------------------------------ any other filter size

template <typename S>
__global__ __launch_bounds__(FN_THREADS) void fi_forward_nhwc_any(
    const typename S::E* __restrict__ in1, const float* __restrict__ in2, const float* __restrict__ in3,
    typename S::E* __restrict__ out, int channel, int h, int w, int fs,
    vfi_strides_nhwc s1, vfi_strides4 s2, vfi_strides4 s3, vfi_strides_nhwc so,
    int tiles_x, int tiles_y, int ntiles) {
    typedef typename S::E E;
    __shared__ FnPixel px[FN_PIXELS];

    const int tile = fi_xcd_tile<int>(blockIdx.x);
    if (tile >= ntiles) return;
    const int tid = threadIdx.x;
    const FnWhere at = fn_where(tile, tid, tiles_x, tiles_y, channel, h, w);
    if ((tid & 3) == 0) {
        const FiFlow fl = fn_flow_at(in2, s2, at.b, at.x, at.y, at.inimg);
        fn_record(px[tid >> 2], at, fi_geom(fl.fx, fl.fy, at.x, at.y, w, h, at.inimg), s1, so, s3);
    }
    __syncthreads();

    const E* img = in1 + (int64_t)at.b * s1.b;
    E* dst = out + (int64_t)at.b * so.b;
    const float* filt = in3 + (int64_t)at.b * s3.b;
    for (FnItems it(tid, channel); it.live(); it.next()) {
        const FnPixel& r = px[it.pixel];
        if (r.state == FN_OUTSIDE) continue;
        const int c = it.chunk;
        if (r.state == FN_COPY) { dst[r.dst + c] = img[r.src + c]; continue; }
        const int ix = r.ix, iy = r.iy;
        const int L = ix + 1 - fs / 2, T = iy + 1 - fs / 2;
        const int R = L + fs, Bm = T + fs;
        const float* fpx = filt + r.fpx;
        const E* plane = img + c;
        float q[4];
        // quadrant by quadrant, rows outer / columns inner, every chain from 0 (quadrants_generic)
        for (int quad = 0; quad < 4; ++quad) {
            const int j0 = (quad & 2) ? iy + 1 : T, j1 = (quad & 2) ? Bm : iy + 1;
            const int i0 = (quad & 1) ? ix + 1 : L, i1 = (quad & 1) ? R : ix + 1;
            float acc = 0.0f;
            for (int j = j0; j < j1; ++j) {
                const E* rowp = plane + (int64_t)clampi(j, 0, h - 1) * s1.h;
                for (int i = i0; i < i1; ++i)
                    acc = fmaf(S::widen(rowp[(int64_t)clampi(i, 0, w - 1) * s1.w]), fpx[(int64_t)((j - T) * fs + (i - L)) * s3.c], acc);
            }
            q[quad] = acc;
        }
        dst[r.dst + c] = S::store(blend4(r.alpha, r.beta, q[0], q[1], q[2], q[3]));
    }
}

// ------------------------------------------------------------------ host

// The widest item the layouts allow, in elements: every address an item touches is base + a sum of strides + a multiple of
// V, so V elements must divide the bases (in bytes) and every stride that is ever multiplied by a non-zero index.  Misaligned
// vector accesses are never issued.
template <typename E>
static int fn_vector_width(const void* input1, void* const* outputs, int nflows, int batch, int h, int w,
                           const vfi_strides_nhwc& s1, const vfi_strides_nhwc& so) {
    for (int v = 16 / (int)sizeof(E); v > 1; v >>= 1) {
        const auto ok_stride = [&](const vfi_strides_nhwc& s) {
            return (batch == 1 || s.b % v == 0) && (h == 1 || s.h % v == 0) && (w == 1 || s.w % v == 0);
        };
        bool ok = ok_stride(s1) && ok_stride(so) && reinterpret_cast<uintptr_t>(input1) % (v * sizeof(E)) == 0;
        for (int t = 0; ok && t < nflows; ++t) ok = reinterpret_cast<uintptr_t>(outputs[t]) % (v * sizeof(E)) == 0;
        if (ok) return v;
    }
    return 1;
}

template <typename S>
static int forward_nhwc_multi(const void* input1, const float* const* flows, const float* input3, void* const* outputs,
                              int nflows, int batch, int channel, int h, int w, int filter_channels, vfi_strides_nhwc s1,
                              vfi_strides4 s2, vfi_strides4 s3, vfi_strides_nhwc so, vfi_stream_t stream) {
    typedef typename S::E E;
    if (nflows <= 0 || !flows || !outputs || batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || filter_channels <= 0)
        return VFI_ERR_SHAPE;
    if (!input1 || !input3) return VFI_ERR_SHAPE;
    for (int t = 0; t < nflows; ++t)
        if (!flows[t] || !outputs[t]) return VFI_ERR_SHAPE;
    const int tiles_x = (w + FN_TW - 1) / FN_TW, tiles_y = (h + FN_TH - 1) / FN_TH;
    const int64_t nt = (int64_t)tiles_x * tiles_y * batch;
    if (batch > 65535 || nt > (1 << 28)) return VFI_ERR_SHAPE;
    const int ntiles = (int)nt;
    const int fs = fi_filter_size(filter_channels);
    const int v = fs == 4 ? fn_vector_width<E>(input1, outputs, nflows, batch, h, w, s1, so) : 1;
    const dim3 grid((unsigned)fi_xcd_grid(ntiles), 1, 1), block(FN_THREADS, 1, 1);
    hipStream_t st = (hipStream_t)stream;
    for (int t = 0; t < nflows; ++t) {
        const E* in = (const E*)input1;
        E* o = (E*)outputs[t];
#define FN_LAUNCH4(V) hipLaunchKernelGGL((fi_forward_nhwc4<S, V>), grid, block, 0, st, in, flows[t], input3, o, channel, h, w, \
                                         s1, s2, s3, so, tiles_x, tiles_y, ntiles)
        if (fs != 4)
            hipLaunchKernelGGL(fi_forward_nhwc_any<S>, grid, block, 0, st, in, flows[t], input3, o, channel, h, w, fs, s1, s2, s3,
                               so, tiles_x, tiles_y, ntiles);
        else if (v * sizeof(E) == 16) FN_LAUNCH4(16 / (int)sizeof(E));
        else if (v * sizeof(E) == 8) FN_LAUNCH4(8 / (int)sizeof(E));
        else if (v * sizeof(E) == 4 && sizeof(E) == 2) FN_LAUNCH4(2);
        else FN_LAUNCH4(1);
#undef FN_LAUNCH4
        const int err = launch_status();
        if (err != VFI_OK) return err;
    }
    return VFI_OK;
}

}  // namespace vfi

using namespace vfi;

extern "C" int vfi_filterinterp_forward_ori_nhwc_multi_to(const float* input1, const float* const* flows, const float* input3,
                                                           float* const* outputs, int nflows, int batch, int channel, int h,
                                                           int w, int filter_channels, vfi_strides_nhwc s1, vfi_strides4 s2,
                                                           vfi_strides4 s3, vfi_strides_nhwc s_out, vfi_stream_t stream) {
    return forward_nhwc_multi<NhwcF32>(input1, flows, input3, reinterpret_cast<void* const*>(outputs), nflows, batch, channel, h, w,
                                       filter_channels, s1, s2, s3, s_out, stream);
}

extern "C" int vfi_filterinterp_forward_ori_nhwc_multi_to_bf16(const void* input1_bf16, const float* const* flows,
                                                                const float* input3, void* const* outputs_bf16, int nflows,
                                                                int batch, int channel, int h, int w, int filter_channels,
                                                                vfi_strides_nhwc s1, vfi_strides4 s2, vfi_strides4 s3,
                                                                vfi_strides_nhwc s_out, vfi_stream_t stream) {
    return forward_nhwc_multi<NhwcBf16>(input1_bf16, flows, input3, outputs_bf16, nflows, batch, channel, h, w, filter_channels,
                                        s1, s2, s3, s_out, stream);
}

// internal: the access width, in elements, that the entries above choose for these layouts (element_bytes 4 or 2); -1 for
// arguments they would refuse.  Host code only: the tests pin the launcher's choice with it.
extern "C" int vfi_filterinterp_nhwc_access_width(int element_bytes, const void* input1, void* const* outputs, int nflows,
                                                   int batch, int h, int w, int filter_channels, vfi_strides_nhwc s1,
                                                   vfi_strides_nhwc s_out) {
    if ((element_bytes != 4 && element_bytes != 2) || !input1 || !outputs || nflows <= 0 || batch <= 0 || h <= 0 || w <= 0 ||
        filter_channels <= 0)
        return -1;
    if (fi_filter_size(filter_channels) != 4) return 1;
    return element_bytes == 4 ? fn_vector_width<float>(input1, outputs, nflows, batch, h, w, s1, s_out)
                              : fn_vector_width<bf16_t>(input1, outputs, nflows, batch, h, w, s1, s_out);
}
