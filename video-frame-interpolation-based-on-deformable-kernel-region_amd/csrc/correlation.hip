// correlation.hip -- PWC-Net / FlowNet cost volume for gfx950.
//
// Semantics: correlation_cuda_kernel.cu:47-147 (forward) and :151-334 (backward)
// of the reference, output-size math of correlation_cuda.cc:23-36; entry points
// replace correlation_cuda.cc.
//
//   out[b, (tj+dr)*dsz + (ti+dr), y, x] =
//       (1 / (k*k*C)) * sum_{j,i in kxk} sum_c P1[b,c,y1+j,x1+i] * P2[b,c,y1+tj*s2+j,x1+ti*s2+i]
//   with P = input zero-padded by pad_size, y1 = y*s1 + md, x1 likewise.
//
// The reference first repacks both inputs to zero-padded NHWC and then runs one
// 32-thread block per output pixel.  Here nothing is repacked: the padding is
// an index test, and for the configuration PWC-Net uses (k=1, s1=s2=1) a
// workgroup owns a 32x8 tile of output pixels, stages the matching window of
// the second feature map (tile + 2*md halo) in LDS one channel chunk at a
// time, and each lane keeps all (2*md+1)^2 running sums in registers.  The coarser pyramid
// levels (hundreds to a few thousand pixels, up to 196 channels) would leave most of the chip
// idle that way; they use 16x4-pixel tiles with one WAVE PER DISPLACEMENT ROW (9 waves per
// workgroup, 9 running sums per lane), which spreads the same work over 9x more waves.
//
// Backward: the bodies, the arithmetic and the launchers are correlation_bwd.h's, one definition for float32, half and
// bfloat16 (correlation_bf16.hip).  This file holds the float32 and half __global__ kernels around them, the packed-half
// tiled kernel, and the structs that name those kernels for the launchers.
#include "correlation_bwd.h"

#include <algorithm>
#include <initializer_list>

#include <hip/hip_fp16.h>

namespace vfi {

#define CORR_CC 8       // channels staged per LDS fill of the 32x8 kernel (the others: CORR_CC_ROWS, correlation_dev.h)

__device__ __forceinline__ float padded_at(const float* __restrict__ f, int h, int w, int y, int x) {
    return (y >= 0 && y < h && x >= 0 && x < w) ? f[(int64_t)y * w + x] : 0.0f;
}

// k == 1, stride1 == stride2 == 1.  `org` = md - pad: output pixel (oy, ox) is
// centred on input pixel (oy + org, ox + org).
template <int MD, int CORR_TW, int CORR_TH, class Epi>
__global__ __launch_bounds__(CORR_TW * CORR_TH) void corr_forward_k1(
    CorrItems items, int channel, int h, int w, int oh, int ow, int org, Epi epi) {
    constexpr int D = 2 * MD + 1;
    constexpr int LW = CORR_TW + 2 * MD, LH = CORR_TH + 2 * MD;
    constexpr int NI = (LH + CORR_TH - 1) / CORR_TH, NJ = (LW + CORR_TW - 1) / CORR_TW;
    __shared__ float tile[CORR_CC][LH][LW];

    const int tx = threadIdx.x, ty = threadIdx.y;
    const int ox = blockIdx.x * CORR_TW + tx, oy = blockIdx.y * CORR_TH + ty;
    const CorrImage im = corr_image((int)blockIdx.z, items.per);
    const int b = im.b;
    const float* __restrict__ in1 = items.in1[im.item];
    const float* __restrict__ in2 = items.in2[im.item];
    float* __restrict__ out = items.out[im.item];
    const int64_t plane = (int64_t)h * w;
    const float* f1 = in1 + (int64_t)b * channel * plane;
    const float* f2 = in2 + (int64_t)b * channel * plane;
    const int y1 = oy + org, x1 = ox + org;                 // centre in input coordinates
    const int wy0 = blockIdx.y * CORR_TH + org - MD;        // window origin in input coordinates
    const int wx0 = blockIdx.x * CORR_TW + org - MD;

    float acc[D * D];
#pragma unroll
    for (int k = 0; k < D * D; ++k) acc[k] = 0.0f;

    // staging plan of this thread, the same for every channel: window rows ty + i*TH, columns
    // tx + j*TW -- row segments, no index arithmetic per element; zero padding is the bounds test
    int soff[NI][NJ];
    bool sin[NI][NJ], sok[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int r = ty + i * CORR_TH, col = tx + j * CORR_TW;
            const int gy = wy0 + r, gx = wx0 + col;
            sin[i][j] = r < LH && col < LW;
            sok[i][j] = sin[i][j] && gy >= 0 && gy < h && gx >= 0 && gx < w;
            soff[i][j] = sok[i][j] ? gy * w + gx : 0;
        }
    const bool f1ok = y1 >= 0 && y1 < h && x1 >= 0 && x1 < w;
    const int f1off = f1ok ? y1 * w + x1 : 0;

    // the next chunk's values are fetched into registers before the current chunk is multiplied and
    // written to LDS after it: the finest level has ~2 workgroups per CU, too few to hide the
    // load -> LDS -> multiply chain otherwise
    float nv[CORR_CC][NI][NJ], na[CORR_CC];
    auto fetch = [&](int c0) {
        const int cn = min(CORR_CC, channel - c0);
#pragma unroll
        for (int c = 0; c < CORR_CC; ++c) {
            const float* p = f2 + (int64_t)(c0 + c) * plane;
            const bool cok = c < cn;
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) nv[c][i][j] = (cok && sok[i][j]) ? p[soff[i][j]] : 0.0f;
            na[c] = (cok && f1ok) ? f1[(int64_t)(c0 + c) * plane + f1off] : 0.0f;
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < channel; c0 += CORR_CC) {
        const int cn = min(CORR_CC, channel - c0);
        __syncthreads();
        float a[CORR_CC];
#pragma unroll
        for (int c = 0; c < CORR_CC; ++c) {
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    if (sin[i][j]) tile[c][ty + i * CORR_TH][tx + j * CORR_TW] = nv[c][i][j];
            a[c] = na[c];
        }
        __syncthreads();
        if (c0 + CORR_CC < channel) fetch(c0 + CORR_CC);
        for (int c = 0; c < cn; ++c) {
            const float av = a[c];
#pragma unroll
            for (int tj = 0; tj < D; ++tj)
#pragma unroll
                for (int ti = 0; ti < D; ++ti)
                    acc[tj * D + ti] = fmaf(av, tile[c][ty + tj][tx + ti], acc[tj * D + ti]);
        }
    }
    if (ox < ow && oy < oh) {
        const float nelems = (float)channel;
        float* o = out + epi.plane(im.item, b, D * D, 0, oh, ow) + (int64_t)oy * ow + ox;
#pragma unroll
        for (int k = 0; k < D * D; ++k) o[(int64_t)k * oh * ow] = epi(acc[k] / nelems);
    }
}

// k == 1, strides 1, small frames: tile of 16x4 output pixels, threadIdx.y = displacement row tj.
template <int MD, class Epi>
__global__ __launch_bounds__(64 * (2 * MD + 1)) void corr_forward_k1_rows(
    CorrItems items, int channel, int h, int w, int oh, int ow, int org, Epi epi) {
    constexpr int D = 2 * MD + 1;
    constexpr int TW = 16, TH = 4, LW = TW + 2 * MD, LH = TH + 2 * MD;
    constexpr int NT = 64 * D, NE = CORR_CC_ROWS * LH * LW;      // threads, staged elements per chunk
    constexpr int NPT = (NE + NT - 1) / NT;
    __shared__ float tile[CORR_CC_ROWS][LH][LW];
    __shared__ float f1s[CORR_CC_ROWS][TH * TW];

    const int lane = threadIdx.x, tj = threadIdx.y;          // lane = pixel inside the tile
    const int tid = tj * 64 + lane;
    const int px = lane & (TW - 1), py = lane >> 4;
    const int ox = blockIdx.x * TW + px, oy = blockIdx.y * TH + py;
    const CorrImage im = corr_image((int)blockIdx.z, items.per);
    const int b = im.b;
    const float* __restrict__ in1 = items.in1[im.item];
    const float* __restrict__ in2 = items.in2[im.item];
    float* __restrict__ out = items.out[im.item];
    const int64_t plane = (int64_t)h * w;
    const float* f1 = in1 + (int64_t)b * channel * plane;
    const float* f2 = in2 + (int64_t)b * channel * plane;
    const int y1 = oy + org, x1 = ox + org;
    const int wy0 = blockIdx.y * TH + org - MD, wx0 = blockIdx.x * TW + org - MD;

    // staging plan: flat element e = tid + k*NT of the chunk's [CC][LH][LW] block (constant divisors)
    int soff[NPT], sch[NPT];
    bool sok[NPT];
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        const int e = tid + k * NT;
        const int c = e / (LH * LW), rem = e - c * (LH * LW);
        const int r = rem / LW, col = rem - r * LW;
        const int gy = wy0 + r, gx = wx0 + col;
        sch[k] = c;
        sok[k] = e < NE && gy >= 0 && gy < h && gx >= 0 && gx < w;
        soff[k] = sok[k] ? gy * w + gx : 0;
    }
    const bool f1ok = y1 >= 0 && y1 < h && x1 >= 0 && x1 < w;
    const int f1off = f1ok ? y1 * w + x1 : 0;

    float acc[D];
#pragma unroll
    for (int ti = 0; ti < D; ++ti) acc[ti] = 0.0f;

    // The chunk loop is a dependent chain (global loads -> LDS -> products) and a small level has too
    // few workgroups to hide it: the next chunk's values are fetched into registers before the
    // current chunk is multiplied, and only written to LDS after it.
    constexpr int NF1 = (CORR_CC_ROWS + D - 1) / D;          // channels of the first map each wave stages
    float nv[NPT], nf1[NF1];
    auto fetch = [&](int c0) {
        const int cn = min(CORR_CC_ROWS, channel - c0);
#pragma unroll
        for (int k = 0; k < NPT; ++k)
            nv[k] = (sok[k] && sch[k] < cn) ? f2[(int64_t)(c0 + sch[k]) * plane + soff[k]] : 0.0f;
#pragma unroll
        for (int q = 0; q < NF1; ++q) {
            const int cc = tj + q * D;
            nf1[q] = (cc < cn && f1ok) ? f1[(int64_t)(c0 + cc) * plane + f1off] : 0.0f;
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < channel; c0 += CORR_CC_ROWS) {
        const int cn = min(CORR_CC_ROWS, channel - c0);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const int e = tid + k * NT;
            if (e < NE) (&tile[0][0][0])[e] = nv[k];
        }
#pragma unroll
        for (int q = 0; q < NF1; ++q)
            if (tj + q * D < CORR_CC_ROWS) f1s[tj + q * D][lane] = nf1[q];
        __syncthreads();
        if (c0 + CORR_CC_ROWS < channel) fetch(c0 + CORR_CC_ROWS);
        for (int c = 0; c < cn; ++c) {
            const float av = f1s[c][lane];
#pragma unroll
            for (int ti = 0; ti < D; ++ti) acc[ti] = fmaf(av, tile[c][py + tj][px + ti], acc[ti]);
        }
    }
    if (ox < ow && oy < oh) {
        const float nelems = (float)channel;
        float* o = out + epi.plane(im.item, b, D * D, tj * D, oh, ow) + (int64_t)oy * ow + ox;
#pragma unroll
        for (int ti = 0; ti < D; ++ti) o[(int64_t)ti * oh * ow] = epi(acc[ti] / nelems);
    }
}

// k == 1, strides 1, frames whose rows are 16-byte aligned: tile of 32x4 output pixels,
// threadIdx.y = displacement row tj, a lane owns TWO horizontally adjacent pixels.  The window and the
// first map are staged as 16-byte units (global_load_dwordx4 -> ds_write_b128: a quarter of the
// vector-memory and LDS-write instructions of the one-float staging, which is what bounds the other
// tiled kernels at one workgroup per CU); per channel a lane reads the 10 values its two 9-wide
// displacement rows share as five aligned ds_read_b64 for 18 multiply-adds.  Same sequential
// channel order.
template <int MD, class Epi>
__global__ __launch_bounds__(64 * (2 * MD + 1)) void corr_forward_k1_rows2(
    CorrItems items, int channel, int h, int w, int oh, int ow, int org, Epi epi) {
    typedef CorrTile2<MD> T;                                                    // LW = 40: 10 aligned 16-byte units
    constexpr int D = T::D, TW = T::TW, TH = T::TH;
    typedef float v2f __attribute__((ext_vector_type(2)));
    typedef float v4f __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) float tile[T::CC][T::LH][T::LW];
    __shared__ __attribute__((aligned(16))) float f1s[T::CC][TH * TW];

    const int lane = threadIdx.x, tj = threadIdx.y;
    const int tid = tj * 64 + lane;
    const int px = T::px(lane), py = T::py(lane);
    const int ox = blockIdx.x * TW + px, oy = blockIdx.y * TH + py;
    const CorrImage im = corr_image((int)blockIdx.z, items.per);
    const int b = im.b;
    const float* __restrict__ in1 = items.in1[im.item];
    const float* __restrict__ in2 = items.in2[im.item];
    float* __restrict__ out = items.out[im.item];
    const int64_t plane = (int64_t)h * w;
    const float* f1 = in1 + (int64_t)b * channel * plane;
    const float* f2 = in2 + (int64_t)b * channel * plane;

    // staging plans of the chunk's [CC][LH][UW] window block and of its [CC][TH][TW/4] first-map block (corr_unit_plan).  The
    // window origin is a multiple of 4 columns: the host checks org and MD
    unsigned soff[T::NPT], foff[T::NF1];
    corr_unit_plan<4u, T::CC, T::LH, T::UW, T::NT>(soff, tid, blockIdx.y * TH + org - MD, blockIdx.x * TW + org - MD, h, w, (int)plane);
    corr_unit_plan<4u, T::CC, TH, TW / 4, T::NT>(foff, tid, blockIdx.y * TH + org, blockIdx.x * TW + org, h, w, (int)plane);

    float acc[2][D];
#pragma unroll
    for (int ti = 0; ti < D; ++ti) { acc[0][ti] = 0.0f; acc[1][ti] = 0.0f; }

    // the next chunk's units are fetched into registers before the current chunk is multiplied
    v4f nv[T::NPT], nf[T::NF1];
    auto fetch = [&](int c0) {
        const int cn = min(T::CC, channel - c0);
        const int bytes = cn * (int)plane * 4;
        const auto d2 = buffer_rsrc(f2 + (int64_t)c0 * plane, bytes);
        const auto d1 = buffer_rsrc(f1 + (int64_t)c0 * plane, bytes);
#pragma unroll
        for (int k = 0; k < T::NPT; ++k) nv[k] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(d2, soff[k], 0, 0));
#pragma unroll
        for (int k = 0; k < T::NF1; ++k) nf[k] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(d1, foff[k], 0, 0));
    };
    fetch(0);
    for (int c0 = 0; c0 < channel; c0 += T::CC) {
        const int cn = min(T::CC, channel - c0);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < T::NPT; ++k) {
            const int e = tid + k * T::NT;
            if (e < T::NU) reinterpret_cast<v4f*>(&tile[0][0][0])[e] = nv[k];
        }
#pragma unroll
        for (int k = 0; k < T::NF1; ++k) {
            const int e = tid + k * T::NT;
            if (e < T::FU) reinterpret_cast<v4f*>(&f1s[0][0])[e] = nf[k];
        }
        __syncthreads();
        if (c0 + T::CC < channel) fetch(c0 + T::CC);
        for (int c = 0; c < cn; ++c) {
            const v2f a = *reinterpret_cast<const v2f*>(&f1s[c][py * TW + px]);
            v2f t[T::PAIRS];
            T::read_row(&tile[c][py + tj][px], t);
            // (one v_fmac per term: left to itself the compiler packs the two pixels' terms into v_pk_fma_f32 -- 1.6 x a plain
            //  multiply-add each on gfx950 -- and pays four v_pk_mov per channel to line up the odd operand pairs: no faster)
#pragma unroll
            for (int ti = 0; ti < D; ++ti) {
                asm("v_fmac_f32_e32 %0, %1, %2" : "+v"(acc[0][ti]) : "v"(a.x), "v"(t[ti / 2][ti & 1]));
                asm("v_fmac_f32_e32 %0, %1, %2" : "+v"(acc[1][ti]) : "v"(a.y), "v"(t[(ti + 1) / 2][(ti + 1) & 1]));
            }
        }
    }
    corr_store_mean(channel, [&](auto mean) {
        if (oy < oh && ox + 1 < ow && (ow & 1) == 0) {
            // the lane's two pixels as one 8-byte store: a wave writes whole 128-byte row segments
            float* o = out + epi.plane(im.item, b, D * D, tj * D, oh, ow) + (int64_t)oy * ow + ox;
#pragma unroll
            for (int ti = 0; ti < D; ++ti) *reinterpret_cast<v2f*>(o + (int64_t)ti * oh * ow) = v2f{epi(mean(acc[0][ti])), epi(mean(acc[1][ti]))};
        } else {
#pragma unroll
            for (int q = 0; q < 2; ++q)
                if (ox + q < ow && oy < oh) {
                    float* o = out + epi.plane(im.item, b, D * D, tj * D, oh, ow) + (int64_t)oy * ow + ox + q;
#pragma unroll
                    for (int ti = 0; ti < D; ++ti) o[(int64_t)ti * oh * ow] = epi(mean(acc[q][ti]));
                }
        }
    });
}

// k == 1, strides 1, 16-byte-aligned rows, the LARGE levels (the finest pyramid level at 1080p: 288 x 496).  With one wave per
// displacement row a workgroup is 9 waves, three fit a CU, and the finest level's 1,152 tiles of corr_forward_k1_rows2 run as
// one full round and one half-empty one (33.7 us; the pair of both directions, exactly three rounds: 62.7).  Here a workgroup
// is 3 waves and owns THREE displacement rows (tj = 3 g + wave) of a 64 x 4 tile, a lane owns FOUR horizontally adjacent
// pixels: 36 running sums per lane, and per channel one 16-byte read of the first map and three of the second map's row feed
// 36 multiply-adds (rows2: six 8-byte reads for 18).  The window a workgroup stages is the tile + 8 columns x 6 rows (the three
// displacement rows its waves need) -- the three workgroups of a tile run on one XCD back to back and find each other's
// lines in its L2.  ~7 workgroups per CU are resident: every tile of the finest level at once.  Channels in sequence, the same
// fmaf per term: the same bits as every other kernel here.
//
// Staging: four channels per chunk by LDS-DMA (`buffer_load_dwordx4 ... lds`) into TWO LDS buffers.  The window and first-map
// units are buffer loads through a descriptor that spans exactly the chunk's planes, with one constant byte offset per unit
// (a unit outside the frame has an offset out of any range, a channel past the last one falls out of the descriptor's: both
// arrive as zeros); a chunk's units go from memory straight into the buffer the previous chunk was read from, under the current
// chunk's multiply-adds -- no staging registers, no ds_write, no address arithmetic, one barrier per chunk.  (The round's first
// version fetched the units into registers and wrote them to LDS: 87 registers, two barriers per chunk, 24 us; this one 63
// registers, 20.7 us at 32 x 288 x 496.)  The tap reads are asm: hipcc
// drains vmcnt before an LDS read it can see next to an LDS-DMA target (filterinterp_lds.hip), which would wait for the chunk
// in flight.  Same tile, same lanes, same order of the multiply-adds: the same bits.
#define CORR_QUAD_LDS_FLOATS (2 * (4 * 6 * 18 + 4 * 4 * 16) * 4)          // two buffers of 432 window units + 256 first-map units
template <int MD, class Epi>
__device__ __forceinline__ void corr_quad_body(
    const CorrItems& items, int channel, int h, int w, int oh, int ow, int org, int tiles_x, int tiles_y, int ntiles, float* lds,
    const Epi& epi) {
    constexpr int D = 2 * MD + 1, G = 3;
    constexpr int CCQ = 4;
    constexpr int TW = 64, TH = 4, LW = TW + 2 * MD, LH = TH + G - 1;
    constexpr int NT = 64 * G;
    constexpr int UW = LW / 4, NU = CCQ * LH * UW;                                // 432 window units (16 bytes) per chunk
    constexpr int NPT = (NU + NT - 1) / NT;
    constexpr int FU = CCQ * TH * (TW / 4);                                       // 256 first-map units
    constexpr int NF1 = (FU + NT - 1) / NT;
    constexpr int BUF = (NU + FU) * 4;                                            // floats per buffer: [window units][first-map units]
    typedef float v4f __attribute__((ext_vector_type(4)));
    static_assert(2 * BUF == CORR_QUAD_LDS_FLOATS, "the kernel's LDS array");

    const int xcd = blockIdx.x % 8, kq = blockIdx.x / 8;
    const int g = kq % (D / G), t_ = (kq / (D / G)) * 8 + xcd;
    if (t_ >= ntiles) return;
    const int img_ = t_ / (tiles_x * tiles_y), trem = t_ - img_ * (tiles_x * tiles_y);
    const int tyi = trem / tiles_x, txi = trem - tyi * tiles_x;
    const int lane = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int tid = wv * 64 + lane;
    const int tj = G * g + wv;
    const int px = 4 * (lane & 15), py = lane >> 4;
    const int ox = txi * TW + px, oy = tyi * TH + py;
    const CorrImage im = corr_image(img_, items.per);
    const int b = im.b;
    const float* __restrict__ in1 = items.in1[im.item];
    const float* __restrict__ in2 = items.in2[im.item];
    float* __restrict__ out = items.out[im.item];
    const int64_t plane = (int64_t)h * w;
    const float* f1 = in1 + (int64_t)b * channel * plane;
    const float* f2 = in2 + (int64_t)b * channel * plane;
    const int wy0 = tyi * TH + org - MD + G * g, wx0 = txi * TW + org - MD;

    // byte offsets of this thread's units from the chunk's first plane (corr_unit_plan)
    unsigned soff[NPT], foff[NF1];
    corr_unit_plan<4u, CCQ, LH, UW, NT>(soff, tid, wy0, wx0, h, w, (int)plane);
    corr_unit_plan<4u, CCQ, TH, TW / 4, NT>(foff, tid, tyi * TH + org, txi * TW + org, h, w, (int)plane);
    // a wave's 64 lanes write 64 consecutive units: wave-uniform destination + lane * 16 bytes (M0).  A staging instruction whose
    // units lie past the block's end is skipped by the waves it has nothing for and runs with a partial exec mask in the last one.
    auto issue = [&](int c0, int buf) {
        const int cn = min(CCQ, channel - c0);
        const int bytes = cn * (int)plane * 4;
        const auto d2 = buffer_rsrc(f2 + (int64_t)c0 * plane, bytes);
        const auto d1 = buffer_rsrc(f1 + (int64_t)c0 * plane, bytes);
        float* base = lds + buf * BUF;
#pragma unroll
        for (int k = 0; k < NPT; ++k)
            if (tid + k * NT < NU)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(d2, (lds_ptr_t)(base + (k * NT + wv * 64) * 4), 16, soff[k], 0, 0, 0);
#pragma unroll
        for (int k = 0; k < NF1; ++k)
            if (tid + k * NT < FU)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(d1, (lds_ptr_t)(base + NU * 4 + (k * NT + wv * 64) * 4), 16, foff[k], 0, 0, 0);
    };

    float acc[4][D];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int ti = 0; ti < D; ++ti) acc[q][ti] = 0.0f;

    const unsigned lds0 = (unsigned)(uintptr_t)(lds_ptr_t)lds;
    const unsigned a_addr = lds0 + 4u * (unsigned)(NU * 4 + py * TW + px);                 // first map: [c][TH * TW]
    const unsigned t_addr = lds0 + 4u * (unsigned)((py + wv) * LW + px);                   // window: [c][LH][LW]
#define CORR_CHANNEL_TERMS(c, bo) do { \
        v4f a4, r0, r1, r2; \
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a4) : "v"(a_addr + (bo)), "n"((c) * TH * TW * 4)); \
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r0) : "v"(t_addr + (bo)), "n"((c) * LH * LW * 4)); \
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r1) : "v"(t_addr + (bo)), "n"((c) * LH * LW * 4 + 16)); \
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r2) : "v"(t_addr + (bo)), "n"((c) * LH * LW * 4 + 32)); \
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a4), "+v"(r0), "+v"(r1), "+v"(r2)); \
        const float a_[4] = { a4.x, a4.y, a4.z, a4.w }; \
        const float t_v[12] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w }; \
        _Pragma("unroll") for (int ti = 0; ti < D; ++ti) \
            _Pragma("unroll") for (int q = 0; q < 4; ++q) asm("v_fmac_f32_e32 %0, %1, %2" : "+v"(acc[q][ti]) : "v"(a_[q]), "v"(t_v[q + ti])); \
    } while (0)

    issue(0, 0);
    int buf = 0;
    for (int c0 = 0; c0 < channel; c0 += CCQ) {
        const int cn = min(CCQ, channel - c0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this thread's units of the chunk have landed ...
        __builtin_amdgcn_s_barrier();                           // ... everybody's have, and everybody is done with the other buffer
        if (c0 + CCQ < channel) issue(c0 + CCQ, buf ^ 1);
        const unsigned bo = (unsigned)(buf * BUF * 4);
        CORR_CHANNEL_TERMS(0, bo);
        if (cn > 1) CORR_CHANNEL_TERMS(1, bo);
        if (cn > 2) CORR_CHANNEL_TERMS(2, bo);
        if (cn > 3) CORR_CHANNEL_TERMS(3, bo);
        buf ^= 1;
    }
#undef CORR_CHANNEL_TERMS
    static_assert(CCQ == 4, "four channels per chunk");
    if (oy >= oh) return;
    float* o = out + epi.plane(im.item, b, D * D, tj * D, oh, ow) + (int64_t)oy * ow + ox;
    corr_store_mean(channel, [&](auto mean) {
        if (ox + 3 < ow && (ow & 3) == 0) {
#pragma unroll
            for (int ti = 0; ti < D; ++ti)
                *reinterpret_cast<v4f*>(o + (int64_t)ti * oh * ow) =
                    v4f{epi(mean(acc[0][ti])), epi(mean(acc[1][ti])), epi(mean(acc[2][ti])), epi(mean(acc[3][ti]))};
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (ox + q < ow) {
#pragma unroll
                    for (int ti = 0; ti < D; ++ti) o[(int64_t)ti * oh * ow + q] = epi(mean(acc[q][ti]));
                }
        }
    });
}

// (the body is a device function: its inline assembly must not be instantiated by the host pass)
template <int MD, class Epi>
__global__ __launch_bounds__(192, 5) void corr_forward_k1_quad(
    CorrItems items, int channel, int h, int w, int oh, int ow, int org, int tiles_x, int tiles_y, int ntiles, Epi epi) {
    __shared__ __attribute__((aligned(16))) float lds[CORR_QUAD_LDS_FLOATS];  // ONE array (see above)
    corr_quad_body<MD>(items, channel, h, w, oh, ow, org, tiles_x, tiles_y, ntiles, lds, epi);
}

// (explicit: hipcc 7.2 leaves the host stub of a kernel template undefined when its only launch sits in a branch it folds away)
template __global__ void corr_forward_k1_quad<4, CorrPlain>(CorrItems, int, int, int, int, int, int, int, int, int, CorrPlain);
template __global__ void corr_forward_k1_quad<4, CorrLrelu>(CorrItems, int, int, int, int, int, int, int, int, int, CorrLrelu);

// k == 1, strides 1, tiny frames (the coarsest pyramid levels: a few hundred pixels, up to 196
// channels): one thread per output element, x fastest, so a wave reads 64 consecutive pixels of each
// map; eight channels in flight per thread.  A tiled kernel leaves most of the chip idle here (10
// workgroups for 18x31).  Sequential channel order, as everywhere.
//
// A tap outside the frame is a zero of the reference's padded buffers, and the reference multiplies it
// (correlation_cuda_kernel.cu:66-69, :124): with one tap inside, a * 0 per channel -- +0 in the sum unless a is infinite or
// NaN, then NaN.  Such a lane runs the same loop: its outside tap is read at the inside tap's pixel (a valid address) and
// `keep` clears what was read.  (A loop of its own for these lanes would run in nearly every wave, after the other one; and
// reading the inside tap's own address twice instead doubled this kernel's time at 196 x 18 x 31.  Both measured: DESIGN.md 4.3.)
template <int MD, class Epi>
__global__ __launch_bounds__(256) void corr_forward_k1_flat(
    CorrItems items, int batch, int channel, int h, int w, int oh, int ow, int org, Epi epi) {
    constexpr int D = 2 * MD + 1;
    const int64_t total = (int64_t)batch * D * D * oh * ow;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int ox = (int)(gid % ow);
    const int oy = (int)((gid / ow) % oh);
    const int tc = (int)((gid / ((int64_t)ow * oh)) % (D * D));
    const int bz = (int)(gid / ((int64_t)ow * oh * D * D));
    const CorrImage im = corr_image(bz, items.per);
    const int b = im.b;
    const float* __restrict__ in1 = items.in1[im.item];
    const float* __restrict__ in2 = items.in2[im.item];
    float* __restrict__ out = items.out[im.item];
    const int y1 = oy + org, x1 = ox + org;
    const int y2 = y1 + tc / D - MD, x2 = x1 + tc % D - MD;
    const bool ok1 = y1 >= 0 && y1 < h && x1 >= 0 && x1 < w, ok2 = y2 >= 0 && y2 < h && x2 >= 0 && x2 < w;
    float acc = 0.0f;
    if (ok1 || ok2) {                                                                           // else zero padding on both sides: +0
        const int64_t plane = (int64_t)h * w;
        // pa: the tap inside the frame (the first map's where both are), pv: the other tap, where it is outside a valid
        // address whose value `keep` turns into the padding's zero (the product commutes)
        const int64_t at1 = (int64_t)y1 * w + x1, at2 = (int64_t)y2 * w + x2;
        const float* pa = (ok1 ? in1 : in2) + (int64_t)b * channel * plane + (ok1 ? at1 : at2);
        const float* pv = (ok1 ? in2 : in1) + (int64_t)b * channel * plane + (ok2 ? at2 : at1);
        const unsigned keep = (ok1 && ok2) ? ~0u : 0u;
        auto tap = [&](int c) { return __uint_as_float(__float_as_uint(pv[(int64_t)c * plane]) & keep); };
        int c = 0;
        for (; c + 8 <= channel; c += 8) {
            float a[8], v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { a[k] = pa[(int64_t)(c + k) * plane]; v[k] = tap(c + k); }
#pragma unroll
            for (int k = 0; k < 8; ++k) acc = fmaf(a[k], v[k], acc);
        }
        for (; c < channel; ++c) acc = fmaf(pa[(int64_t)c * plane], tap(c), acc);
    }
    if constexpr (Epi::DENSE) out[gid - (int64_t)im.item * items.per * D * D * oh * ow] = epi(acc / (float)channel);
    else out[epi.plane(im.item, b, D * D, tc, oh, ow) + (int64_t)oy * ow + ox] = epi(acc / (float)channel);
}

// any kernel size / strides: one thread per output element, sequential channel order (one item per launch: epi's item 0)
template <class Epi>
__global__ __launch_bounds__(256) void corr_forward_generic(
    const float* __restrict__ in1, const float* __restrict__ in2, float* __restrict__ out,
    int batch, int channel, int h, int w, int oc, int oh, int ow,
    int pad, int kr, int md, int s1, int s2, int dr, Epi epi) {
    const int64_t total = (int64_t)batch * oc * oh * ow;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int ox = (int)(gid % ow);
    const int oy = (int)((gid / ow) % oh);
    const int tc = (int)((gid / ((int64_t)ow * oh)) % oc);
    const int b = (int)(gid / ((int64_t)ow * oh * oc));
    const int dsz = 2 * dr + 1;
    const int ti = tc % dsz - dr, tj = tc / dsz - dr;
    const int y1 = oy * s1 + md - pad, x1 = ox * s1 + md - pad;     // padded -> input coordinates
    const int y2 = y1 + tj * s2, x2 = x1 + ti * s2;
    const int64_t plane = (int64_t)h * w;
    const float* f1 = in1 + (int64_t)b * channel * plane;
    const float* f2 = in2 + (int64_t)b * channel * plane;
    float acc = 0.0f;
    for (int j = -kr; j <= kr; ++j)
        for (int i = -kr; i <= kr; ++i)
            for (int c = 0; c < channel; ++c)
                acc = fmaf(padded_at(f1 + (int64_t)c * plane, h, w, y1 + j, x1 + i),
                           padded_at(f2 + (int64_t)c * plane, h, w, y2 + j, x2 + i), acc);
    const int k = 2 * kr + 1;
    if constexpr (Epi::DENSE) out[gid] = epi(acc / (float)(k * k * channel));
    else out[epi.plane(0, b, oc, tc, oh, ow) + (int64_t)oy * ow + ox] = epi(acc / (float)(k * k * channel));
}

// The at::Half instantiation for PWC-Net's configuration, tiled like corr_forward_k1_rows2: 32x4 output pixels per
// workgroup, one wave per displacement row, a lane owns two adjacent pixels.  Both maps are staged as halves
// (8-byte units); per channel and displacement ONE packed multiply forms the two pixels' products, each rounded to
// half exactly as the reference's `rInput1[i] * rInput2[i]` on two Half values (correlation_cuda_kernel.cu:124), and
// two mixed-precision adds accumulate them in float, channels in sequence.  Same bits as corr_forward_generic_f16.
template <int MD>
__global__ __launch_bounds__(64 * (2 * MD + 1)) void corr_forward_k1_rows2_f16(
    const __half* __restrict__ in1, const __half* __restrict__ in2, __half* __restrict__ out,
    int channel, int h, int w, int oh, int ow, int org) {
    typedef CorrTile2<MD> T;                                                    // LW = 40 halves: 10 aligned 8-byte units
    constexpr int D = T::D, TW = T::TW, TH = T::TH;
    __shared__ __attribute__((aligned(16))) __half tile[T::CC][T::LH][T::LW];
    __shared__ __attribute__((aligned(16))) __half f1s[T::CC][TH * TW];

    const int lane = threadIdx.x, tj = threadIdx.y;
    const int tid = tj * 64 + lane;
    const int px = T::px(lane), py = T::py(lane);
    const int ox = blockIdx.x * TW + px, oy = blockIdx.y * TH + py;
    const int b = blockIdx.z;
    const int64_t plane = (int64_t)h * w;
    const __half* f1 = in1 + (int64_t)b * channel * plane;
    const __half* f2 = in2 + (int64_t)b * channel * plane;

    // staging plans of the window block and the first-map block, in 8-byte units (corr_unit_plan)
    unsigned soff[T::NPT], foff[T::NF1];
    corr_unit_plan<2u, T::CC, T::LH, T::UW, T::NT>(soff, tid, blockIdx.y * TH + org - MD, blockIdx.x * TW + org - MD, h, w, (int)plane);
    corr_unit_plan<2u, T::CC, TH, TW / 4, T::NT>(foff, tid, blockIdx.y * TH + org, blockIdx.x * TW + org, h, w, (int)plane);

    float acc[2][D];
#pragma unroll
    for (int ti = 0; ti < D; ++ti) { acc[0][ti] = 0.0f; acc[1][ti] = 0.0f; }

    uint2 nv[T::NPT], nf[T::NF1];
    typedef unsigned v2u_ __attribute__((ext_vector_type(2)));
    auto fetch = [&](int c0) {
        const int cn = min(T::CC, channel - c0);
        const int bytes = cn * (int)plane * 2;
        const auto d2 = buffer_rsrc(f2 + (int64_t)c0 * plane, bytes);
        const auto d1 = buffer_rsrc(f1 + (int64_t)c0 * plane, bytes);
#pragma unroll
        for (int k = 0; k < T::NPT; ++k) { const v2u_ v = __builtin_amdgcn_raw_buffer_load_b64(d2, soff[k], 0, 0); nv[k] = make_uint2(v.x, v.y); }
#pragma unroll
        for (int k = 0; k < T::NF1; ++k) { const v2u_ v = __builtin_amdgcn_raw_buffer_load_b64(d1, foff[k], 0, 0); nf[k] = make_uint2(v.x, v.y); }
    };
    fetch(0);
    for (int c0 = 0; c0 < channel; c0 += T::CC) {
        const int cn = min(T::CC, channel - c0);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < T::NPT; ++k) {
            const int e = tid + k * T::NT;
            if (e < T::NU) reinterpret_cast<uint2*>(&tile[0][0][0])[e] = nv[k];
        }
#pragma unroll
        for (int k = 0; k < T::NF1; ++k) {
            const int e = tid + k * T::NT;
            if (e < T::FU) reinterpret_cast<uint2*>(&f1s[0][0])[e] = nf[k];
        }
        __syncthreads();
        if (c0 + T::CC < channel) fetch(c0 + T::CC);
        for (int c = 0; c < cn; ++c) {
            const __half2 a = *reinterpret_cast<const __half2*>(&f1s[c][py * TW + px]);
            __half2 r[T::PAIRS];
            T::read_row(&tile[c][py + tj][px], r);
#pragma unroll
            for (int ti = 0; ti < D; ++ti) {
                // (t[ti], t[ti + 1]): pixel 0 meets displacement column ti, pixel 1 the next one
                const __half2 pair = (ti & 1) ? __halves2half2(__high2half(r[ti / 2]), __low2half(r[ti / 2 + 1])) : r[ti / 2];
                const __half2 p = __hmul2(a, pair);                        // two products, each rounded to half
                // acc + (float)product in one mixed-precision instruction (fma(p, 1, acc): one rounding, the float add's)
                const unsigned pb = __builtin_bit_cast(unsigned, p);
                asm("v_fma_mix_f32 %0, %1, 1.0, %0 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "+v"(acc[0][ti]) : "v"(pb));
                asm("v_fma_mix_f32 %0, %1, 1.0, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(acc[1][ti]) : "v"(pb));
            }
        }
    }
    // (the mean of a power-of-two channel count as a product with the exact reciprocal: the same real number, rounded to half once)
    corr_store_mean(channel, [&](auto mean) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (ox + q < ow && oy < oh) {
                __half* o = out + ((int64_t)b * (D * D) + tj * D) * oh * ow + (int64_t)oy * ow + ox + q;
#pragma unroll
                for (int ti = 0; ti < D; ++ti) o[(int64_t)ti * oh * ow] = __float2half_rn(mean(acc[q][ti]));
            }
    });
}

// half inputs and output, the reference's `scalar_t = at::Half` instantiation (correlation_cuda_kernel.cu:386,403):
// each product is formed in half (`rInput1[i] * rInput2[i]` on two Half values: one rounding to half, :124),
// widened and accumulated in float; the mean is rounded to half once (:143).  One thread per output element,
// sequential channel order, eight channels of loads in flight.
__global__ __launch_bounds__(256) void corr_forward_generic_f16(
    const __half* __restrict__ in1, const __half* __restrict__ in2, __half* __restrict__ out,
    int batch, int channel, int h, int w, int oc, int oh, int ow,
    int pad, int kr, int md, int s1, int s2, int dr) {
    const int64_t total = (int64_t)batch * oc * oh * ow;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int ox = (int)(gid % ow);
    const int oy = (int)((gid / ow) % oh);
    const int tc = (int)((gid / ((int64_t)ow * oh)) % oc);
    const int b = (int)(gid / ((int64_t)ow * oh * oc));
    const int dsz = 2 * dr + 1;
    const int ti = tc % dsz - dr, tj = tc / dsz - dr;
    const int y1 = oy * s1 + md - pad, x1 = ox * s1 + md - pad;     // padded -> input coordinates
    const int y2 = y1 + tj * s2, x2 = x1 + ti * s2;
    const int64_t plane = (int64_t)h * w;
    const __half* f1 = in1 + (int64_t)b * channel * plane;
    const __half* f2 = in2 + (int64_t)b * channel * plane;
    float acc = 0.0f;
    for (int j = -kr; j <= kr; ++j)
        for (int i = -kr; i <= kr; ++i) {
            const int ya = y1 + j, xa = x1 + i, yb = y2 + j, xb = x2 + i;
            // a tap outside a map is a zero of the reference's padded buffer.  Outside both: +0 for every channel, skipped.
            // Inside one: half(a * 0) per channel, +-0 unless a is infinite or NaN -- then NaN; the lane runs the same loop, its
            // outside tap read at the inside tap's pixel (a valid address) and cleared by `keep` (the product commutes).  (A
            // loop of their own for these lanes, and a second pass of workgroups for them, were built and measured slower than
            // this at the 1080p pyramid's half levels -- nearly every wave holds such a lane: DESIGN.md 4.3, padding taps.)
            const bool oka = ya >= 0 && ya < h && xa >= 0 && xa < w, okb = yb >= 0 && yb < h && xb >= 0 && xb < w;
            if (!oka && !okb) continue;
            const int64_t ata = (int64_t)ya * w + xa, atb = (int64_t)yb * w + xb;
            const __half* pa = (oka ? f1 : f2) + (oka ? ata : atb);
            const __half* pb = (oka ? f2 : f1) + (okb ? atb : ata);
            const unsigned short keep = (oka && okb) ? 0xffffu : 0u;
            auto tap = [&](int c) { return __ushort_as_half((unsigned short)(__half_as_ushort(pb[(int64_t)c * plane]) & keep)); };
            int c = 0;
            for (; c + 8 <= channel; c += 8) {
                __half va[8], vb[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) { va[q] = pa[(int64_t)(c + q) * plane]; vb[q] = tap(c + q); }
#pragma unroll
                for (int q = 0; q < 8; ++q) acc += __half2float(__hmul(va[q], vb[q]));
            }
            for (; c < channel; ++c) acc += __half2float(__hmul(pa[(int64_t)c * plane], tap(c)));
        }
    const int k = 2 * kr + 1;
    out[gid] = __float2half_rn(acc / (float)(k * k * channel));
}

// The backward kernels.  The arithmetic (CorrF32, CorrF16), the mask (CorrNoMask, CorrGradLrelu) and both bodies are
// correlation_bwd.h's, shared with the bfloat16 kernels of correlation_bf16.hip; the kernels here bind them to float and half.
// One thread per gradient element, any configuration:
#define CORR_BACKWARD_ARGS(T) const T* __restrict__ other, const T* __restrict__ gout, T* __restrict__ gin, \
    int batch, int channel, int h, int w, int oc, int oh, int ow, int pad, int kr, int md, int s2, int dr
template <bool SECOND>
__global__ __launch_bounds__(256) void corr_backward(CORR_BACKWARD_ARGS(float)) {
    corr_backward_body<CorrF32, SECOND>(other, gout, gin, batch, channel, h, w, oc, oh, ow, pad, kr, md, s2, dr, CorrNoMask<CorrF32>{});
}
// the same through LeakyReLU's derivative (vfi_correlation_lrelu_backward*, any configuration)
template <bool SECOND>
__global__ __launch_bounds__(256) void corr_lrelu_backward(CORR_BACKWARD_ARGS(float), CorrGradLrelu act) {
    corr_backward_body<CorrF32, SECOND>(other, gout, gin, batch, channel, h, w, oc, oh, ow, pad, kr, md, s2, dr, act);
}
template <bool SECOND>
__global__ __launch_bounds__(256) void corr_backward_f16(CORR_BACKWARD_ARGS(__half)) {
    corr_backward_body<CorrF16, SECOND>(other, gout, gin, batch, channel, h, w, oc, oh, ow, pad, kr, md, s2, dr, CorrNoMask<CorrF16>{});
}
#undef CORR_BACKWARD_ARGS

// Backward for PWC-Net's configuration (k == 1, strides 1, pad == md == 4; round 3).  corr_backward above is one thread per
// gradient element: 81 loads of gradOutput + 81 of the other map + 81 multiply-adds each, and a gradOutput element is
// fetched again by every channel (1.1 ms for both gradients at 32 x 288 x 496).  corr_backward_k1_body (correlation_bwd.h)
// gives a thread one PIXEL and its 81 gradOutput values in registers for all channels, with the same sums in the same
// order, so the result is corr_backward's and the oracle's bit for bit.  corr_backward_k1 below is one gradient per launch,
// and corr_backward_k1_pair runs one instance or the other per workgroup.
template <bool SECOND>
__global__ __launch_bounds__(256) void corr_backward_k1(
    const float* __restrict__ other, const float* __restrict__ gout, float* __restrict__ gin,
    int channel, int h, int w, int groups, int ch_per_group) {
    __shared__ CorrBwdWindow win;
    const CorrBwdTile t(channel, groups, ch_per_group);
    corr_backward_k1_body<CorrF32, SECOND>(win, t, other, gout, gin, channel, h, w, CorrNoMask<CorrF32>{});
}

// Up to four gradients of two calls of equal shape in ONE launch (vfi_correlation_backward_pair: both gradients of the same
// pyramid level of a frame pair's two flow networks).  A workgroup's role -- which item, first or second gradient -- comes
// from blockIdx.z once (CorrBwdTile), so it is uniform: its three pointers are scalar loads from the argument block at the
// role's index, and one scalar branch picks the instance of the body.  Nothing inside the channel loop knows of roles, and a
// gradient's bits are those of its own corr_backward_k1 launch (channel groups only partition the channels).
__global__ __launch_bounds__(256) void corr_backward_k1_pair(CorrBwdRoles roles, int channel, int h, int w, int groups, int ch_per_group) {
    __shared__ CorrBwdWindow win;
    const CorrBwdTile t(channel, groups, ch_per_group, roles.per_role);
    const float* __restrict__ other = roles.r[t.role].other;
    const float* __restrict__ gout = roles.r[t.role].gout;
    float* __restrict__ gin = roles.r[t.role].gin;
    if (roles.r[t.role].second) corr_backward_k1_body<CorrF32, true>(win, t, other, gout, gin, channel, h, w, CorrNoMask<CorrF32>{});
    else corr_backward_k1_body<CorrF32, false>(win, t, other, gout, gin, channel, h, w, CorrNoMask<CorrF32>{});
}

// The two kernels above with the mask (vfi_correlation_lrelu_backward, ..._pair): kernels of their own, so the plain ones
// are what they were.  A role's y and strides are scalar loads at the role's index, like its pointers.
// (The mask is 81 more loads per pixel and channel group, outside the channel loop; the channel loop is the same code.)
template <bool SECOND>
__global__ __launch_bounds__(256) void corr_lrelu_backward_k1(
    const float* __restrict__ other, const float* __restrict__ gout, float* __restrict__ gin,
    int channel, int h, int w, int groups, int ch_per_group, CorrGradLrelu act) {
    __shared__ CorrBwdWindow win;
    const CorrBwdTile t(channel, groups, ch_per_group);
    corr_backward_k1_body<CorrF32, SECOND>(win, t, other, gout, gin, channel, h, w, act);
}

__global__ __launch_bounds__(256) void corr_lrelu_backward_k1_pair(CorrBwdRoles roles, CorrBwdMasks masks, int channel, int h, int w,
                                                                   int groups, int ch_per_group) {
    __shared__ CorrBwdWindow win;
    const CorrBwdTile t(channel, groups, ch_per_group, roles.per_role);
    const float* __restrict__ other = roles.r[t.role].other;
    const float* __restrict__ gout = roles.r[t.role].gout;
    float* __restrict__ gin = roles.r[t.role].gin;
    const CorrGradLrelu act = {masks.y[t.role], masks.ystride[t.role], masks.gstride[t.role], masks.slope};
    if (roles.r[t.role].second) corr_backward_k1_body<CorrF32, true>(win, t, other, gout, gin, channel, h, w, act);
    else corr_backward_k1_body<CorrF32, false>(win, t, other, gout, gin, channel, h, w, act);
}

// PWC-Net's configuration (k == 1, strides 1, pad == md == 4), modelled on corr_backward_k1: a workgroup owns 64x4 pixels and
// stages the other map's 12x72 window per channel in LDS (double-buffered, zero padded); a lane owns TWO horizontally adjacent
// pixels, whose 81 gradOutput values are 81 packed-half registers for all channels of the group.  Per channel a term is one
// v_pk_mul_f16 and one v_pk_add_f16 for both pixels: the rounding is per half, so the bits are corr_backward_f16's.  The
// partials run in the reference's order (tc = l, l + 32, l + 64, then r += s_l for l = 0..31).  A term the reference skips
// (gradInput2, displaced position outside the frame) has g = 0 here and meets the window's zero padding: it adds
// half(0 * 0) = +0, which changes at most the sign of a zero partial -- and r, which starts at +0 and so is never -0,
// absorbs either zero alike.
template <bool SECOND>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(4))) void corr_backward_k1_f16(
    const __half* __restrict__ other, const __half* __restrict__ gout, __half* __restrict__ gin,
    int channel, int h, int w, int groups, int ch_per_group) {
    typedef CorrBwdTile T;
    constexpr int MD = T::MD, D = T::D, OC = T::OC;
    __shared__ __attribute__((aligned(16))) __half win[2][T::LH][T::LW];
    const T t(channel, groups, ch_per_group);
    const int tid = threadIdx.x, px = 2 * (tid & 31), py = tid >> 5;
    const int bx = t.x0 + px, by = t.y0 + py;
    const int n = t.n, c_begin = t.c_begin, c_end = t.c_end;
    const bool in0 = bx < w && by < h, in1 = bx + 1 < w && by < h;
    const int64_t plane = (int64_t)h * w;
    const __half* go = gout + (int64_t)n * OC * plane;
    const __half zero = __float2half_rn(0.0f);
    if (c_begin >= c_end) return;

    // the pair's 81 gradOutput values (zero where the reference skips the term, and for a pixel outside the frame).  Buffer
    // loads through a descriptor that spans the image's gradOutput: one 32-bit offset per load, and an offset out of range
    // (an element outside the frame) returns the zero.  (Left to itself the compiler issues all 162 loads at once and needs
    // over 200 registers: the loads go out one displacement row at a time.)
    const auto gd = buffer_rsrc(go, (int)(OC * plane * 2));
    __half2 g[OC];
#pragma unroll
    for (int tc = 0; tc < OC; ++tc) {
        const int gy = SECOND ? by - (tc / D - MD) : by, gx = SECOND ? bx - (tc % D - MD) : bx;
        const bool rok = gy >= 0 && gy < h;
        const bool ok0 = in0 && rok && gx >= 0 && gx < w, ok1 = in1 && rok && gx + 1 >= 0 && gx + 1 < w;
        const unsigned off = 2u * (unsigned)(tc * (int)plane + gy * w + gx);
        const unsigned short lo = __builtin_amdgcn_raw_buffer_load_b16(gd, ok0 ? off : 0x80000000u, 0, 0);
        const unsigned short hi = __builtin_amdgcn_raw_buffer_load_b16(gd, ok1 ? off + 2u : 0x80000000u, 0, 0);
        g[tc] = __halves2half2(__ushort_as_half(lo), __ushort_as_half(hi));
        asm volatile("" : "+v"(g[tc]));                              // (packed here, not both halves kept to the end)
        if (tc % D == D - 1) __builtin_amdgcn_sched_barrier(0);     // one displacement row of loads in flight at a time
    }

    auto stage = [&](int c, int buf) {
        const auto od = buffer_rsrc(other + ((int64_t)n * channel + c) * plane, (int)(plane * 2));
        for (int e = tid; e < T::LH * T::LW; e += 128) {
            const T::Elem p = t.window(e);
            const bool ok = p.gy >= 0 && p.gy < h && p.gx >= 0 && p.gx < w;
            win[buf][p.r][p.col] = __ushort_as_half(__builtin_amdgcn_raw_buffer_load_b16(od, ok ? 2u * (unsigned)(p.gy * w + p.gx) : 0x80000000u, 0, 0));
        }
    };
    stage(c_begin, 0);
    const float nelems_h = __half2float(__float2half_rn((float)channel));
    for (int c = c_begin; c < c_end; ++c) {
        const int buf = (c - c_begin) & 1;
        __syncthreads();                                    // window c has been written; window c - 1 has been read
        if (c + 1 < c_end) stage(c + 1, buf ^ 1);
        // tc in ascending order, the product of tc going straight into partial tc % 32: partial l receives tc = l, l + 32,
        // l + 64 in that order, and only the 32 partials are live beside g.  (s_l starts at its first term, not at +0 + it:
        // that changes at most the sign of a zero partial, and r -- which starts at +0 and so is never -0 -- absorbs either
        // zero alike.)  Window row tj (gradInput1) or 2*MD - tj (gradInput2), columns px .. px + 9 as five aligned pairs; the
        // pair a displacement column needs is one of them (even offset) or straddles two (odd offset).
        __half2 s[32];
#pragma unroll
        for (int tj = 0; tj < D; ++tj) {
            const __half2* row = reinterpret_cast<const __half2*>(&win[buf][py + (SECOND ? 2 * MD - tj : tj)][px]);
            __half2 q[MD + 1];
#pragma unroll
            for (int k = 0; k <= MD; ++k) q[k] = row[k];
#pragma unroll
            for (int ti = 0; ti < D; ++ti) {
                const int tc = tj * D + ti, o = SECOND ? 2 * MD - ti : ti;
                const __half2 v = (o & 1) ? __halves2half2(__high2half(q[o / 2]), __low2half(q[o / 2 + 1])) : q[o / 2];
                const __half2 prod = __hmul2(g[tc], v);
                s[tc % 32] = tc < 32 ? prod : __hadd2(s[tc % 32], prod);
            }
            __builtin_amdgcn_sched_barrier(0);     // (a row's window reads at a time: g and the 32 partials hold 113 registers)
        }
        __half2 r = __halves2half2(zero, zero);
#pragma unroll
        for (int l = 0; l < 32; ++l) r = __hadd2(r, s[l]);
        __half* o = gin + ((int64_t)n * channel + c) * plane + (int64_t)by * w + bx;
        if (in0) o[0] = corr_mean_f16(__low2half(r), nelems_h);
        if (in1) o[1] = corr_mean_f16(__high2half(r), nelems_h);
    }
}

}  // namespace vfi

using namespace vfi;

// kernel selection thresholds: number of 32x8 tiles from which the one-lane-per-pixel kernel is used ...
static constexpr long long corr_big_threshold = 256;
// ... and number of 16x4 tiles below which the one-thread-per-output kernel is used
static constexpr long long corr_flat_threshold = 64;    // measured at 1080p: 36 tiles 12 us flat vs 29 us tiled; 144 tiles 40 vs 24
// number of 64x4 tiles from which the four-pixels-per-lane kernel (three displacement rows per workgroup) is used; below it,
// aligned levels take two pixels per lane
static constexpr long long corr_quad_threshold = 128;   // (1080p pyramid: 64 x 144 x 248 -- 144 tiles -- 19.4 us against 21.4 with two pixels per lane; 96 x 72 x 124 -- 36 tiles -- 23.6 against 17.3)

extern "C" int vfi_correlation_output_dims(int h, int w, int pad_size, int kernel_size, int max_displacement,
                                            int stride1, int stride2, int* out_channels, int* out_h, int* out_w) {
    if (kernel_size <= 0 || stride1 <= 0 || stride2 <= 0 || max_displacement < 0 || pad_size < 0) return VFI_ERR_SHAPE;
    const int kr = (kernel_size - 1) / 2;
    const int border = kr + max_displacement;
    const int dr = max_displacement / stride2;
    if (out_channels) *out_channels = (dr * 2 + 1) * (dr * 2 + 1);
    // ceil(float / float), as correlation_cuda.cc:31-32 computes it
    if (out_h) *out_h = (int)ceilf((float)(h + 2 * pad_size - 2 * border) / (float)stride1);
    if (out_w) *out_w = (int)ceilf((float)(w + 2 * pad_size - 2 * border) / (float)stride1);
    return VFI_OK;
}

// The checks every entry makes before it launches, in this order: a positive shape, no null tensor, valid parameters, and
// at least one output pixel; the output dimensions come back.  (The reference's backward indexes gradInput rows by
// blockIdx * stride1 and leaves the tensor for stride1 > 1: only stride1 == 1 is defined.)
int vfi::corr_check(std::initializer_list<const void*> tensors, int batch, int channel, int h, int w, int pad_size, int kernel_size,
                      int max_displacement, int stride1, int stride2, bool backward, int* oc, int* oh, int* ow) {
    if (batch <= 0 || channel <= 0 || h <= 0 || w <= 0) return VFI_ERR_SHAPE;
    for (const void* t : tensors)
        if (!t) return VFI_ERR_SHAPE;
    if (vfi_correlation_output_dims(h, w, pad_size, kernel_size, max_displacement, stride1, stride2, oc, oh, ow))
        return VFI_ERR_SHAPE;
    if ((backward && stride1 != 1) || *oh <= 0 || *ow <= 0) return VFI_ERR_SHAPE;
    return VFI_OK;
}

// The tiled backward kernels' split of the channels into groups over blockIdx.z, so that a small level fills the chip
// (about 2048 workgroups); the group count comes back, 0 where batch * groups does not fit a grid.
int vfi::corr_backward_groups(int tiles, int batch, int channel, int* ch_per_group) {
    int groups = (int)std::min<int64_t>(channel, std::max<int64_t>(1, (2048 + (int64_t)tiles * batch - 1) / ((int64_t)tiles * batch)));
    *ch_per_group = (channel + groups - 1) / groups;
    groups = (channel + *ch_per_group - 1) / *ch_per_group;
    return (int64_t)batch * groups <= 65535 ? groups : 0;
}

// What an epilogue adds to the bits the alignment tests look at: an image stride that breaks a kernel's store alignment
// counts exactly as a misaligned base pointer does.  Whether the strides are valid for an output of oc x oh x ow planes.
static uintptr_t corr_stride_bits(const CorrPlain&, int) { return 0; }
static uintptr_t corr_stride_bits(const CorrLrelu& e, int item) { return (uintptr_t)e.stride[item] * sizeof(float); }
static bool corr_epilogue_ok(const CorrPlain&, int, int64_t) { return true; }
static bool corr_epilogue_ok(const CorrLrelu& e, int nitems, int64_t image) {
    return corr_slope_ok(e.slope) && e.stride[0] >= image && e.stride[nitems - 1] >= image;
}

// one call, or two calls of equal shape (nitems == 2) in one launch
template <class Epi>
static int correlation_forward_items(const float* const* in1s, const float* const* in2s, float* const* outs, int nitems, int per,
                                     int channel, int h, int w, int pad_size, int kernel_size, int max_displacement,
                                     int stride1, int stride2, vfi_stream_t stream, const Epi& epi) {
    int oc, oh, ow;
    if (nitems < 1 || nitems > 2) return VFI_ERR_SHAPE;
    const int last = nitems - 1;
    if (corr_check({in1s[0], in2s[0], outs[0], in1s[last], in2s[last], outs[last]}, per, channel, h, w, pad_size, kernel_size,
                   max_displacement, stride1, stride2, false, &oc, &oh, &ow))
        return VFI_ERR_SHAPE;
    if (nitems == 2 && outs[0] == outs[1]) return VFI_ERR_SHAPE;
    if (!corr_epilogue_ok(epi, nitems, (int64_t)oc * oh * ow)) return VFI_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int batch = nitems * per;                          // images of the launch
    CorrItems items;
    uintptr_t in_bits = 0, out_bits = 0;
    for (int i = 0; i < 2; ++i) {
        const int k = i < nitems ? i : 0;
        items.in1[i] = in1s[k]; items.in2[i] = in2s[k]; items.out[i] = outs[k];
        in_bits |= reinterpret_cast<uintptr_t>(in1s[k]) | reinterpret_cast<uintptr_t>(in2s[k]);
        out_bits |= reinterpret_cast<uintptr_t>(outs[k]) | corr_stride_bits(epi, k);
    }
    items.per = per;
    const int kr = (kernel_size - 1) / 2, dr = max_displacement / stride2;
    if (kernel_size == 1 && stride1 == 1 && stride2 == 1 && max_displacement == 4) {
        const int64_t big_tiles = (int64_t)((ow + 31) / 32) * ((oh + 7) / 8) * batch;
        const int64_t small_tiles = (int64_t)((ow + 15) / 16) * ((oh + 3) / 4) * batch;
        // 16-byte staging needs rows, planes and bases aligned (plane = h * w floats); the tiled kernel writes a lane's two
        // pixels as one 8-byte store: an output view at an odd element offset of its storage takes the other kernels
        const bool aligned = (w & 3) == 0 && ((max_displacement - pad_size) & 3) == 0 && (in_bits & 15) == 0 && (out_bits & 7) == 0 &&
                             (int64_t)h * w * 4 * (CORR_CC_ROWS + 1) < INT_MAX;      // (a chunk of planes through one buffer descriptor)
        if (small_tiles < corr_flat_threshold * nitems) {
            const int64_t total = (int64_t)batch * oc * oh * ow;
            hipLaunchKernelGGL((corr_forward_k1_flat<4, Epi>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, items,
                               batch, channel, h, w, oh, ow, max_displacement - pad_size, epi);
        } else if (aligned && (out_bits & 15) == 0 &&
                   (int64_t)((ow + 63) / 64) * ((oh + 3) / 4) * batch >= corr_quad_threshold * nitems) {
            const int tiles_x = (ow + 63) / 64, tiles_y = (oh + 3) / 4;
            const int64_t nt = (int64_t)tiles_x * tiles_y * batch;
            if (nt > (1 << 26)) return VFI_ERR_SHAPE;
            const unsigned wgs = (unsigned)((nt + 7) / 8) * 8 * 3;                 // whole groups of 8 XCDs x 3 displacement-row groups
            hipLaunchKernelGGL((corr_forward_k1_quad<4, Epi>), dim3(wgs), dim3(64, 3, 1), 0, st, items,
                               channel, h, w, oh, ow, max_displacement - pad_size, tiles_x, tiles_y, (int)nt, epi);
        } else if (aligned) {
            const dim3 grid((ow + 31) / 32, (oh + 3) / 4, batch);
            hipLaunchKernelGGL((corr_forward_k1_rows2<4, Epi>), grid, dim3(64, 9, 1), 0, st, items,
                               channel, h, w, oh, ow, max_displacement - pad_size, epi);
        } else if (big_tiles >= corr_big_threshold * nitems) {
            const dim3 grid((ow + 31) / 32, (oh + 7) / 8, batch);
            hipLaunchKernelGGL((corr_forward_k1<4, 32, 8, Epi>), grid, dim3(32, 8, 1), 0, st, items,
                               channel, h, w, oh, ow, max_displacement - pad_size, epi);
        } else {
            const dim3 grid((ow + 15) / 16, (oh + 3) / 4, batch);
            hipLaunchKernelGGL((corr_forward_k1_rows<4, Epi>), grid, dim3(64, 9, 1), 0, st, items,
                               channel, h, w, oh, ow, max_displacement - pad_size, epi);
        }
        return launch_status();
    }
    // any other configuration: the generic kernel, one launch per item
    for (int i = 0; i < nitems; ++i) {
        const int64_t total = (int64_t)per * oc * oh * ow;
        Epi one = epi;
        if constexpr (!Epi::DENSE) one.stride[0] = epi.stride[i];      // (the generic kernel runs one item per launch)
        hipLaunchKernelGGL(corr_forward_generic<Epi>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, in1s[i],
                           in2s[i], outs[i], per, channel, h, w, oc, oh, ow, pad_size, kr, max_displacement, stride1,
                           stride2, dr, one);
        if (launch_status() != VFI_OK) return VFI_ERR_LAUNCH;
    }
    return VFI_OK;
}

extern "C" int vfi_correlation_forward(const float* input1, const float* input2, float* output, int batch, int channel,
                                        int h, int w, int pad_size, int kernel_size, int max_displacement,
                                        int stride1, int stride2, vfi_stream_t stream) {
    if (batch <= 0 || !input1 || !input2 || !output) return VFI_ERR_SHAPE;
    return correlation_forward_items(&input1, &input2, &output, 1, batch, channel, h, w, pad_size, kernel_size, max_displacement,
                                     stride1, stride2, stream, CorrPlain{});
}

// vfi_correlation_forward with PWC-Net's LeakyReLU applied to every mean as it is stored, into an output whose images lie
// output_batch_stride elements apart: the same kernels with the epilogue compiled in.
extern "C" int vfi_correlation_lrelu_forward(const float* input1, const float* input2, float* output, int64_t output_batch_stride,
                                              int batch, int channel, int h, int w, int pad_size, int kernel_size,
                                              int max_displacement, int stride1, int stride2, float negative_slope,
                                              vfi_stream_t stream) {
    if (batch <= 0 || !input1 || !input2 || !output) return VFI_ERR_SHAPE;
    return correlation_forward_items(&input1, &input2, &output, 1, batch, channel, h, w, pad_size, kernel_size, max_displacement,
                                     stride1, stride2, stream, CorrLrelu{{output_batch_stride, output_batch_stride}, negative_slope});
}

// Two correlation calls of equal shape in ONE launch -- the same pyramid level of the two flow networks PWCDCNet runs for a
// frame pair, (I0, I1) and (I1, I0) (networks/DAIN.py:196-202, PWCNet/PWCNet.py:230-300).  Results: the two single calls',
// bit for bit (the same kernels; which of them runs is decided on the pair's tile count, and every one of them sums the
// channels in the same order).
extern "C" int vfi_correlation_forward_pair(const float* input1_a, const float* input2_a, float* output_a,
                                             const float* input1_b, const float* input2_b, float* output_b,
                                             int batch, int channel, int h, int w, int pad_size, int kernel_size,
                                             int max_displacement, int stride1, int stride2, vfi_stream_t stream) {
    if (batch <= 0) return VFI_ERR_SHAPE;
    const float* in1s[2] = {input1_a, input1_b};
    const float* in2s[2] = {input2_a, input2_b};
    float* outs[2] = {output_a, output_b};
    return correlation_forward_items(in1s, in2s, outs, 2, batch, channel, h, w, pad_size, kernel_size, max_displacement,
                                     stride1, stride2, stream, CorrPlain{});
}

extern "C" int vfi_correlation_lrelu_forward_pair(const float* input1_a, const float* input2_a, float* output_a,
                                                   int64_t output_a_batch_stride,
                                                   const float* input1_b, const float* input2_b, float* output_b,
                                                   int64_t output_b_batch_stride,
                                                   int batch, int channel, int h, int w, int pad_size, int kernel_size,
                                                   int max_displacement, int stride1, int stride2, float negative_slope,
                                                   vfi_stream_t stream) {
    if (batch <= 0) return VFI_ERR_SHAPE;
    const float* in1s[2] = {input1_a, input1_b};
    const float* in2s[2] = {input2_a, input2_b};
    float* outs[2] = {output_a, output_b};
    return correlation_forward_items(in1s, in2s, outs, 2, batch, channel, h, w, pad_size, kernel_size, max_displacement,
                                     stride1, stride2, stream, CorrLrelu{{output_a_batch_stride, output_b_batch_stride}, negative_slope});
}

extern "C" int vfi_correlation_forward_f16(const void* input1, const void* input2, void* output, int batch, int channel,
                                            int h, int w, int pad_size, int kernel_size, int max_displacement,
                                            int stride1, int stride2, vfi_stream_t stream) {
    int oc, oh, ow;
    if (corr_check({input1, input2, output}, batch, channel, h, w, pad_size, kernel_size, max_displacement, stride1, stride2, false,
                   &oc, &oh, &ow))
        return VFI_ERR_SHAPE;
    const int kr = (kernel_size - 1) / 2, dr = max_displacement / stride2;
    const int64_t total = (int64_t)batch * oc * oh * ow;
    if ((total + 255) / 256 > INT_MAX) return VFI_ERR_SHAPE;
    if (kernel_size == 1 && stride1 == 1 && stride2 == 1 && max_displacement == 4) {
        // PWC-Net's configuration on frames whose rows are 8-byte aligned, enough tiles to fill the chip: the tiled kernel
        const int64_t small_tiles = (int64_t)((ow + 15) / 16) * ((oh + 3) / 4) * batch;
        const bool aligned = (w & 3) == 0 && ((max_displacement - pad_size) & 3) == 0 &&
                             ((reinterpret_cast<uintptr_t>(input1) | reinterpret_cast<uintptr_t>(input2)) & 7) == 0 &&
                             (int64_t)h * w * 2 * (CORR_CC_ROWS + 1) < INT_MAX;      // (a chunk of planes through one buffer descriptor)
        // (measured at the 1080p pyramid: 144 such tiles 27 us tiled vs 21 us one thread per output; 576 tiles 33 vs 101)
        if (aligned && small_tiles >= 4 * corr_flat_threshold) {
            const dim3 grid((ow + 31) / 32, (oh + 3) / 4, batch);
            hipLaunchKernelGGL(corr_forward_k1_rows2_f16<4>, grid, dim3(64, 9, 1), 0, (hipStream_t)stream, (const __half*)input1,
                               (const __half*)input2, (__half*)output, channel, h, w, oh, ow, max_displacement - pad_size);
            return launch_status();
        }
    }
    hipLaunchKernelGGL(corr_forward_generic_f16, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const __half*)input1, (const __half*)input2, (__half*)output, batch, channel, h, w, oc, oh, ow,
                       pad_size, kr, max_displacement, stride1, stride2, dr);
    return launch_status();
}

// The backward entries.  The checks and the launchers are correlation_bwd.h's, the same for every storage type; here the
// file names its kernels.  float32: every kernel.
struct CorrBwdF32 {
    typedef float T;
    typedef CorrGradLrelu Mask;
    static constexpr bool MASKED = true, PAIRED = true;
    static bool k1_fits(int, int) { return true; }
    template <class... Args>
    static void generic(bool second, const Mask* act, dim3 grid, hipStream_t st, Args... args) {
        if (act) hipLaunchKernelGGL(second ? corr_lrelu_backward<true> : corr_lrelu_backward<false>, grid, dim3(256), 0, st, args..., *act);
        else hipLaunchKernelGGL(second ? corr_backward<true> : corr_backward<false>, grid, dim3(256), 0, st, args...);
    }
    template <class... Args>
    static void k1(bool second, const Mask* act, dim3 grid, hipStream_t st, Args... args) {
        if (act) hipLaunchKernelGGL(second ? corr_lrelu_backward_k1<true> : corr_lrelu_backward_k1<false>, grid, dim3(256), 0, st, args..., *act);
        else hipLaunchKernelGGL(second ? corr_backward_k1<true> : corr_backward_k1<false>, grid, dim3(256), 0, st, args...);
    }
    template <class... Args>
    static void pair(const CorrBwdRoles& roles, const CorrBwdMasks* masks, dim3 grid, hipStream_t st, Args... args) {
        if (masks) hipLaunchKernelGGL(corr_lrelu_backward_k1_pair, grid, dim3(256), 0, st, roles, *masks, args...);
        else hipLaunchKernelGGL(corr_backward_k1_pair, grid, dim3(256), 0, st, roles, args...);
    }
};
// half (the reference's at::Half instantiation): no masked and no pair kernels.  The tiled kernel has 128 threads and
// reaches an image's gradOutput through one buffer descriptor: 81 planes of halves below 2 GB.
struct CorrBwdF16 {
    typedef __half T;
    typedef void Mask;
    static constexpr bool MASKED = false, PAIRED = false;
    static bool k1_fits(int h, int w) { return (int64_t)81 * h * w * 2 < INT_MAX; }
    template <class... Args>
    static void generic(bool second, const Mask*, dim3 grid, hipStream_t st, Args... args) {
        hipLaunchKernelGGL(second ? corr_backward_f16<true> : corr_backward_f16<false>, grid, dim3(256), 0, st, args...);
    }
    template <class... Args>
    static void k1(bool second, const Mask*, dim3 grid, hipStream_t st, Args... args) {
        hipLaunchKernelGGL(second ? corr_backward_k1_f16<true> : corr_backward_k1_f16<false>, grid, dim3(128), 0, st, args...);
    }
};

extern "C" int vfi_correlation_backward(const float* input1, const float* input2, const float* gradoutput,
                                         float* gradinput1, float* gradinput2, int batch, int channel, int h, int w,
                                         int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
                                         vfi_stream_t stream) {
    return corr_backward_both<CorrBwdF32>(input1, input2, gradoutput, gradinput1, gradinput2, batch, channel, h, w, pad_size, kernel_size,
                                          max_displacement, stride1, stride2, stream);
}

// vfi_correlation_backward of gradOutput masked by LeakyReLU's derivative: the same two launches of the masked kernels.
extern "C" int vfi_correlation_lrelu_backward(const float* input1, const float* input2, const float* y, int64_t y_batch_stride,
                                               const float* gradoutput, int64_t gradoutput_batch_stride, float* gradinput1,
                                               float* gradinput2, int batch, int channel, int h, int w, int pad_size,
                                               int kernel_size, int max_displacement, int stride1, int stride2,
                                               float negative_slope, vfi_stream_t stream) {
    const CorrGradLrelu act = {y, y_batch_stride, gradoutput_batch_stride, negative_slope};
    return corr_backward_both<CorrBwdF32>(input1, input2, gradoutput, gradinput1, gradinput2, batch, channel, h, w, pad_size, kernel_size,
                                          max_displacement, stride1, stride2, stream, &act);
}

extern "C" int vfi_correlation_backward_pair(
    const float* input1_a, const float* input2_a, const float* gradoutput_a, float* gradinput1_a, float* gradinput2_a,
    const float* input1_b, const float* input2_b, const float* gradoutput_b, float* gradinput1_b, float* gradinput2_b,
    int batch, int channel, int h, int w, int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
    vfi_stream_t stream) {
    return corr_backward_pair<CorrBwdF32>(corr_backward_items<float>(input1_a, input2_a, gradoutput_a, gradinput1_a, gradinput2_a, input1_b,
                                                                     input2_b, gradoutput_b, gradinput1_b, gradinput2_b),
                                          nullptr, batch, channel, h, w, pad_size, kernel_size, max_displacement, stride1, stride2, stream);
}

extern "C" int vfi_correlation_lrelu_backward_pair(
    const float* input1_a, const float* input2_a, const float* y_a, int64_t y_a_batch_stride, const float* gradoutput_a,
    int64_t gradoutput_a_batch_stride, float* gradinput1_a, float* gradinput2_a,
    const float* input1_b, const float* input2_b, const float* y_b, int64_t y_b_batch_stride, const float* gradoutput_b,
    int64_t gradoutput_b_batch_stride, float* gradinput1_b, float* gradinput2_b,
    int batch, int channel, int h, int w, int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
    float negative_slope, vfi_stream_t stream) {
    const CorrGradLrelu acts[2] = {{y_a, y_a_batch_stride, gradoutput_a_batch_stride, negative_slope},
                                   {y_b, y_b_batch_stride, gradoutput_b_batch_stride, negative_slope}};
    return corr_backward_pair<CorrBwdF32>(corr_backward_items<float>(input1_a, input2_a, gradoutput_a, gradinput1_a, gradinput2_a, input1_b,
                                                                     input2_b, gradoutput_b, gradinput1_b, gradinput2_b),
                                          acts, batch, channel, h, w, pad_size, kernel_size, max_displacement, stride1, stride2, stream);
}

extern "C" int vfi_correlation_backward_f16(const void* input1, const void* input2, const void* gradoutput,
                                             void* gradinput1, void* gradinput2, int batch, int channel, int h, int w,
                                             int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
                                             vfi_stream_t stream) {
    return corr_backward_both<CorrBwdF16>(input1, input2, gradoutput, gradinput1, gradinput2, batch, channel, h, w, pad_size, kernel_size,
                                          max_displacement, stride1, stride2, stream);
}

