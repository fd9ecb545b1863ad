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
//   fi_forward_ori_direct_bf16  one thread per pixel, any filter size, any strides, 2-byte alignment: the fallback and the
//                               yardstick.  fs == 4 starts each quadrant chain with a product (fi4_pixel), every other size
//                               from 0 (quadrants_generic), as the float32 entry's kernels do.
//   fi_forward_ori_lds_bf16     fs == 4: the tiling, LDS-DMA ring, counted vmcnt, per-tile bounding box, rung ladder, gather
//                               fallback and channel split of fi_forward_ori_lds_f16 -- a staged window element is one
//                               dword = two pixels, a tap row is three dword LDS reads shifted into place by v_alignbit --
//                               with the widening a shift / a mask and the arithmetic fi4_pixel.
// Image columns are never replicated in LDS (a dword holds two pixels), so a window that crosses the left or right border
// is moved inside the image, as in the fp16 kernel; the pixel then picks, per tap, the moved window's column that the
// clamped tap names (validity bounds the move to one column on the left, two on the right).  That selection is compiled
// into a second instance of the channel loop (EDGE), taken by the tiles in which some valid pixel's window was moved; the
// interior tiles' loop does not contain it.
// Both kernels write through a layout of their own (so.h == s1.h; batch and channel strides free), one 2-byte store per
// element: the destination may be a channel slice of a wider buffer that is only 2-byte aligned.
#define FI_PITCH_SKEW 16                            // (dwords; see fi_pitch_for)
#include "bf16.h"
#include "filterinterp_dev.h"
#include "filterinterp_paths.h"
// the image-only multi-flow backward's kernels and launcher, templates on the gradients' storage: instantiated below
#define FI_CTX_BWD_TEMPLATES_ONLY
#include "filterinterp_ctx_bwd.hip"

#include <limits.h>

namespace vfi {

#define BF_TW 64
#define BF_TH 16
#define BF_PX 2
#define BF_THREADS (BF_TW * BF_TH / BF_PX)
#define BF_PASS_ROWS (BF_TH / BF_PX)
#define BF_HDR 16
#define BF_RING_DWORDS 15984
#define BF_RMAX 5
#define BF_KTOP 8

// ------------------------------------------------------------------ direct kernel (reference order)

__global__ __launch_bounds__(VFI_TX * VFI_TY) void fi_forward_ori_direct_bf16(
    const bf16_t* __restrict__ in1, const float* __restrict__ in2, const float* __restrict__ in3,
    bf16_t* __restrict__ out, int channel, int h, int w, int fs,
    vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides so) {
    const int x = blockIdx.x * VFI_TX + threadIdx.x;
    const int y = blockIdx.y * VFI_TY + threadIdx.y;
    if (x >= w || y >= h) return;
    const int b = blockIdx.z;
    const FiFlow fl = fi_flow_at(in2, s2, b, x, y);
    const bf16_t* img = in1 + (int64_t)b * s1.b;
    bf16_t* dst = out + (int64_t)b * so.b + (int64_t)y * so.h + x;
    const FiGeom g = fi_geom(fl.fx, fl.fy, x, y, w, h);
    if (!g.valid) {
        fi_copy_through_to<true>(img + (int64_t)y * s1.h + x, dst, 0, channel, s1.c, so.c);
        return;
    }
    const int ix = g.ix, iy = g.iy;
    const int L = ix + 1 - fs / 2, T = iy + 1 - fs / 2;
    const int R = L + fs, Bm = T + fs;
    const float* fpx = in3 + (int64_t)b * s3.b + (int64_t)y * s3.h + x;
    for (int c = 0; c < channel; ++c) {
        const bf16_t* plane = img + (int64_t)c * s1.c;
        float q[4];
        // quadrant by quadrant, rows outer / columns inner (:2749-2787)
        for (int quad = 0; quad < 4; ++quad) {
            const int j0 = (quad & 2) ? iy + 1 : T, j1 = (quad & 2) ? Bm : iy + 1;
            const int i0 = (quad & 1) ? ix + 1 : L, i1 = (quad & 1) ? R : ix + 1;
            float acc = 0.0f;
            bool product = fs == 4;                             // (fi4_pixel: the chain's first term is a plain product)
            for (int j = j0; j < j1; ++j) {
                const bf16_t* row = plane + (int64_t)clampi(j, 0, h - 1) * s1.h;
                for (int i = i0; i < i1; ++i) {
                    const float v = bf16_widen(row[clampi(i, 0, w - 1)]);
                    const float f = fpx[(int64_t)((j - T) * fs + (i - L)) * s3.c];
                    acc = product ? v * f : fmaf(v, f, acc);
                    product = false;
                }
            }
            q[quad] = acc;
        }
        dst[(int64_t)c * so.c] = bf16_rne(blend4(g.alpha, g.beta, q[0], q[1], q[2], q[3]));
    }
}

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

// Channel loop of one workgroup: f16_run_channels (filterinterp_f16.hip) -- ring geometry a compile-time function of K, one
// constant s_waitcnt in the steady state, running plane descriptors, the pipeline skewed by one pixel across the barrier --
// with the pixel's arithmetic fi4_pixel on the widened taps.  EDGE: the instance of the tiles with a moved window.
template <int K, bool EDGE>
__device__ __forceinline__ void bf16_run_channels(const bf16_t* __restrict__ img, bf16_t* __restrict__ out, int64_t cs, int64_t cso,
                                                  int c_begin, int c_end, int tid, const FiWindow& win,
                                                  const BfPixel (&px)[BF_PX], unsigned* __restrict__ ring) {
    typedef unsigned v2u __attribute__((ext_vector_type(2)));
    static_assert(BF_PX == 2, "two pixels per thread");
    constexpr int NP = K * BF_THREADS;                      // dwords per ring slot
    constexpr int R = (BF_RING_DWORDS / NP) < BF_RMAX ? (BF_RING_DWORDS / NP) : BF_RMAX;
    constexpr int D = R - 1;
    static_assert(D >= 1 && (D - 1) * K <= 63, "ring geometry");
    static_assert(R * NP <= BF_RING_DWORDS, "the ring's slots fit the LDS array");
    if (c_begin >= c_end) return;
    // dword e = tid + k*BF_THREADS of the staged window, row-major, `pitch` dwords per row; rows clamped to the image,
    // columns never out of it; pad dwords get an out-of-range offset (the load returns 0 without touching memory)
    const float inv_pitch32 = 1.0f / (float)win.pitch;
    unsigned goff[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = tid + k * BF_THREADS;
        const int r = fi_row_of(e, inv_pitch32);
        const int col = e - r * win.pitch;
        const unsigned off = 2u * (unsigned)(clampi(win.by0 + r, 0, win.h - 1) * win.hs + win.bx0 + 2 * col);
        goff[k] = (col < win.bw && r < win.bh) ? off : 0x80000000u;
    }
    const int plane_bytes = (2 * ((win.h - 1) * win.hs + win.w) + 3) & ~3;
    const int wave_first = __builtin_amdgcn_readfirstlane(tid >> 6) * 64;
    const unsigned ring_lds = (unsigned)(uintptr_t)(lds_ptr_t)ring;
    const unsigned pitch4 = 4u * (unsigned)win.pitch;
    unsigned lb[BF_PX], sh[BF_PX], soff[BF_PX];
#pragma unroll
    for (int p = 0; p < BF_PX; ++p) {
        lb[p] = ring_lds + 4u * (unsigned)(px[p].lbase >> 1);
        sh[p] = (unsigned)(px[p].lbase & 1) * 16u;
        soff[p] = px[p].valid ? 2u * px[p].pix : 0x80000000u;   // (an invalid pixel's store is dropped by the range check)
    }
    const int last = c_end - 1;
    const bf16_t* pdma = img + (int64_t)c_begin * cs;
    bf16_t* pout = out + (int64_t)c_begin * cso;
    auto issue = [&](int slot) {
        const auto plane = buffer_rsrc(pdma, plane_bytes);
        unsigned* l = ring + slot * NP + wave_first;
#pragma unroll
        for (int k = 0; k < K; ++k)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(plane, (lds_ptr_t)(l + k * BF_THREADS), 4, goff[k], 0, 0, 0);
        pdma += cs;
    };
#define BF_READ2(dst, addr) asm volatile("ds_read2_b32 %0, %1 offset0:0 offset1:1" : "=v"(dst) : "v"(addr))
#define BF_READ1(dst, addr) asm volatile("ds_read_b32 %0, %1 offset:8" : "=v"(dst) : "v"(addr))
    v2u a01[2][4];          // dwords 0, 1 of the four tap rows, two pixels
    unsigned a2[2][4];      // dword 2
    auto reads = [&](int p, unsigned so) {
        unsigned a = lb[p] + so;
#pragma unroll
        for (int r = 0; r < 4; ++r) { BF_READ2(a01[p][r], a); BF_READ1(a2[p][r], a); a += pitch4; }
    };
    auto pixel = [&](int p, const bf16_t* plane_ptr) {
        float v[16];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            // ({d1,d0} >> sh) and ({d2,d1} >> sh): the moved window's four columns as two packed pairs
            const unsigned e0 = __builtin_amdgcn_alignbit(a01[p][r].y, a01[p][r].x, sh[p]);
            const unsigned e1 = __builtin_amdgcn_alignbit(a2[p][r], a01[p][r].y, sh[p]);
            // EDGE: tap k of the pixel's own window is column clamp(k + shift, 0, 3) of the moved one -- the replicated
            // value, picked out of the eight bytes {e1, e0} by the pixel's two selectors
            const unsigned o0 = EDGE ? __builtin_amdgcn_perm(e1, e0, px[p].sel[0]) : e0;
            const unsigned o1 = EDGE ? __builtin_amdgcn_perm(e1, e0, px[p].sel[1]) : e1;
            v[r * 4 + 0] = bf16_lo(o0); v[r * 4 + 1] = bf16_hi(o0);
            v[r * 4 + 2] = bf16_lo(o1); v[r * 4 + 3] = bf16_hi(o1);
        }
        const float val = fi4_pixel(v, px[p].f, px[p].alpha, px[p].beta);
        const auto oplane = buffer_rsrc(plane_ptr, plane_bytes);
        __builtin_amdgcn_raw_buffer_store_b16(bf16_rne(val), oplane, soff[p], 0, 0);
    };
    auto compute = [&](int slot, bool first) {
        const unsigned so = (unsigned)(slot * (NP * 4));
        reads(0, so);
        if (!first) pixel(1, pout - cso);                   // pixel 1 of the previous channel
        asm volatile("s_waitcnt lgkmcnt(7)" ::: "memory");  // (at most 15 LDS reads outstanding)
        reads(1, so);
        asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(a01[0][0]), "+v"(a01[0][1]), "+v"(a01[0][2]), "+v"(a01[0][3]),
                                               "+v"(a2[0][0]), "+v"(a2[0][1]), "+v"(a2[0][2]), "+v"(a2[0][3]));
        pixel(0, pout);
        // pixel 1's taps are in registers before the barrier: the slot may be overwritten after it
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a01[1][0]), "+v"(a01[1][1]), "+v"(a01[1][2]), "+v"(a01[1][3]),
                                               "+v"(a2[1][0]), "+v"(a2[1][1]), "+v"(a2[1][2]), "+v"(a2[1][3]));
        pout += cso;
    };
#undef BF_READ2
#undef BF_READ1
    const int n0 = min(D, c_end - c_begin);
    for (int j = 0; j < n0; ++j) issue(j);
    wait_windows<K>(n0 - 1);                                    // the first window has landed ...
    __builtin_amdgcn_s_barrier();                               // ... in every wave
    int c = c_begin, slot = 0;
    for (; c + D <= last; ++c) {                                // steady state: window c + D exists
        issue(slot == 0 ? R - 1 : slot - 1);                    // into the slot every wave finished reading before the last barrier
        compute(slot, c == c_begin);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((D - 1) * K) : "memory");      // all but the D - 1 youngest windows: c + 1 has landed
        __builtin_amdgcn_s_barrier();
        slot = (slot + 1 == R) ? 0 : slot + 1;
    }
    for (; c <= last; ++c) {                                    // the last D channels: nothing left to stage
        compute(slot, c == c_begin);
        if (c < last) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        slot = (slot + 1 == R) ? 0 : slot + 1;
    }
    pixel(1, pout - cso);                                       // pixel 1 of the last channel
#pragma unroll
    for (int p = 0; p < BF_PX; ++p)
        if (px[p].inimg && !px[p].valid) fi_copy_through_to<true>(img, out, px[p].pix, c_begin, c_end, cs, cso);
}

__global__ __launch_bounds__(BF_THREADS, 4) void fi_forward_ori_lds_bf16(
    const bf16_t* __restrict__ in1, const float* __restrict__ in2, const float* __restrict__ in3,
    bf16_t* __restrict__ out, int channel, int h, int w,
    vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides so,
    int tiles_x, int tiles_y, int ntiles, int ch_per_group) {
    __shared__ unsigned lds[BF_HDR + BF_RING_DWORDS];
    int* box = reinterpret_cast<int*>(lds);                 // [0..3] the bounding box, [4] "a window of this tile was moved"

    // four horizontally consecutive tiles per XCD (fi_xcd_tile)
    const int tile = fi_xcd_tile<unsigned>(blockIdx.x);
    if (tile >= ntiles) return;
    const FiTile tp = fi_tile_at(tile, tiles_x, tiles_y, channel, ch_per_group);
    const int b = tp.b, c_begin = tp.c_begin, c_end = tp.c_end;

    const int tid = threadIdx.x;
    const int x = tp.tx * BF_TW + (tid & (BF_TW - 1));
    const int y0 = tp.ty * BF_TH + (tid >> 6);

    BfPixel px[BF_PX];
    int L[BF_PX], Lc[BF_PX], T[BF_PX];
    int bx_lo = INT_MAX, by_lo = INT_MAX, bx_hi = INT_MIN, by_hi = INT_MIN;
    bool moved = false;
#pragma unroll
    for (int p = 0; p < BF_PX; ++p) {
        const int y = y0 + p * BF_PASS_ROWS;
        px[p].inimg = x < w && y < h;
        px[p].pix = (unsigned)(y * (int)s1.h + x);
        const FiFlow fl = fi_flow_at(in2, s2, b, x, y, px[p].inimg);
        const FiGeom g = fi_geom(fl.fx, fl.fy, x, y, w, h, px[p].inimg, 1);        // (an invalid pixel's window: L = 0)
        px[p].valid = g.valid;
        L[p] = g.ix - 1; T[p] = g.iy - 1;
        Lc[p] = clampi(L[p], 0, w - 4);                     // the window moved inside the image (w >= 4)
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
        fi_box_add4(g.valid, Lc[p], T[p], bx_lo, by_lo, bx_hi, by_hi);
    }

    if (tid == 0) { fi_box_clear(box); box[4] = 0; }
    __syncthreads();
    if (moved) box[4] = 1;
    const bool any_valid = fi_box_fold(box, tid, bx_lo, by_lo, bx_hi, by_hi);
    const bool edge = box[4] != 0;
    const int bx0 = any_valid ? box[0] & ~1 : 0, by0 = box[1];          // even: dword-aligned rows
    const int bw = any_valid ? (box[2] - bx0 + 2) >> 1 : 0;              // dwords per row
    const int bh = any_valid ? box[3] - by0 + 1 : 0;
    const int pitch = fi_pitch_for(bw);
    const int n = pitch * bh;

#pragma unroll
    for (int p = 0; p < BF_PX; ++p) {
        px[p].lbase = px[p].valid ? (T[p] - by0) * (2 * pitch) + (Lc[p] - bx0) : 0;
        const float* fpx = in3 + (int64_t)b * s3.b + (int64_t)(y0 + p * BF_PASS_ROWS) * s3.h + x;
#pragma unroll
        for (int k = 0; k < 16; ++k) px[p].f[k] = px[p].valid ? fpx[(int64_t)k * s3.c] : 0.0f;
    }

    const bf16_t* img = in1 + (int64_t)b * s1.b;
    bf16_t* dst = out + (int64_t)b * so.b;
    const int kmax = (n + BF_THREADS - 1) / BF_THREADS;
    if (kmax > BF_KTOP) {
        // window too large for LDS: the same chains gathered from global memory, rows and columns clamped per tap
#pragma unroll
        for (int p = 0; p < BF_PX; ++p) {
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

    const FiWindow win{bx0, by0, bw, bh, pitch, h, w, (int)s1.h};          // bx0 even; bw, pitch in dwords
    unsigned* ring = lds + BF_HDR;
#define BF_RUN(K) (edge ? bf16_run_channels<K, true>(img, dst, s1.c, so.c, c_begin, c_end, tid, win, px, ring) \
                        : bf16_run_channels<K, false>(img, dst, s1.c, so.c, c_begin, c_end, tid, win, px, ring))
    if (kmax <= 2) BF_RUN(2);
    else if (kmax == 3) BF_RUN(3);
    else if (kmax == 4) BF_RUN(4);
    else if (kmax <= 6) BF_RUN(6);
    else BF_RUN(8);
#undef BF_RUN
}

// one flow, direct kernel
static int forward_bf16_direct(const bf16_t* input1, const float* flow, const float* input3, bf16_t* output, int batch, int channel,
                               int h, int w, int filter_channels, vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides so,
                               hipStream_t st) {
    hipLaunchKernelGGL(fi_forward_ori_direct_bf16, pixel_grid(w, h, batch), dim3(VFI_TX, VFI_TY, 1), 0, st, input1, flow, input3,
                       output, channel, h, w, fi_filter_size(filter_channels), s1, s2, s3, so);
    return launch_status();
}

// one flow: the staged kernel where the image's layout allows dword staging, else the direct kernel
static int forward_bf16(const bf16_t* input1, const float* flow, const float* input3, bf16_t* output, int batch, int channel, int h,
                        int w, int filter_channels, vfi_strides s1, vfi_strides s2, vfi_strides s3, vfi_strides so, hipStream_t st) {
    // the staged kernel moves dwords: rows, planes and the base address must be 4-byte aligned
    const bool staged = filter_channels == 16 && w >= 4 &&
                        ((s1.h | s1.c | s1.b) & 1) == 0 && (reinterpret_cast<uintptr_t>(input1) & 3) == 0 &&
                        (int64_t)h * s1.h * 2 < INT_MAX;
    const int tiles_x = (w + BF_TW - 1) / BF_TW, tiles_y = (h + BF_TH - 1) / BF_TH;
    const int64_t nt = (int64_t)tiles_x * tiles_y * batch;
    if (!staged || nt > (1 << 28))
        return forward_bf16_direct(input1, flow, input3, output, batch, channel, h, w, filter_channels, s1, s2, s3, so, st);
    const int ntiles = (int)nt;
    // split the channel range over blockIdx.y when that shortens the tail (as the fp32 kernel)
    const FiSplit split = fi_channel_split(ntiles, channel, 4.3);
    hipLaunchKernelGGL(fi_forward_ori_lds_bf16, dim3((unsigned)fi_xcd_grid(ntiles), (unsigned)split.groups, 1), dim3(BF_THREADS, 1, 1), 0,
                       st, input1, flow, input3, output, channel, h, w, s1, s2, s3, so, tiles_x, tiles_y, ntiles, split.ch_per_group);
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
