// correlation_bf16.hip -- the cost volume on bfloat16 tensors (vfi_correlation_forward_bf16 / _backward_bf16).
//
// Storage is bfloat16, arithmetic float32.  A product of two bfloat16 values has 16 significand bits and is exact in
// float32; the sums are float32; a result is rounded to bfloat16 once, to nearest even (v_cvt_pk_bf16_f32).
//
// Forward, PWC-Net's configuration (k == 1, strides 1, max displacement 4): the matrix cores.  For one output row y and one
// displacement row tj the nine values of a pixel are the band x2 - x1 in [-4, 4] of
//     C[x1][x2] = sum_c f1[c][y][x1] * f2[c][y + tj - 4][x2],
// a 16-pixel block of x1 needs 24 columns x2, and two 16x16x32 MFMAs per 32 channels form them (9 of 32 products wanted).
// Forward, anything else, and small PWC-Net levels: one thread per output, the float32 generic kernel's arithmetic.
// Backward: the float32 kernels' arithmetic on widened values -- the bodies and the launchers of correlation_bwd.h, which
// correlation.hip's float32 and half kernels share, bound to bfloat16 by the kernels of this file.
//
// The same with PWC-Net's LeakyReLU (vfi_correlation_lrelu_forward_bf16 / _backward_bf16): the kernels below take an epilogue
// (forward: what is stored, and where an image begins) and a gradient mask (backward: what a gradOutput value becomes as it is
// loaded); the plain entries instantiate them with the types that do nothing.
//
// Two calls of equal shape in one launch (vfi_correlation_[lrelu_]forward_pair_bf16, ..._backward_pair_bf16: the same pyramid
// level of a frame pair's two flow networks): pair kernels that take a workgroup's item or role from blockIdx and run the same
// bodies, so every output is its single entry's bit for bit.
#include "correlation_bwd.h"

namespace vfi {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// What a forward kernel stores for a mean v, and where image b of the output begins.  CorrBf16Plain: bf16_rne(v), dense images.
// CorrBf16Lrelu: the bits of torch's bfloat16 leaky_relu on the STORED cost volume -- the mean is rounded to bfloat16 first; a
// value that is not positive is then multiplied by the slope in float32 and rounded again (NaN stays NaN, -0 becomes
// -0 * slope) -- into an output whose images lie `stride` elements apart, the 81 planes of an image contiguous.
struct CorrBf16Plain {
    __device__ __forceinline__ unsigned pack(float lo, float hi) const { return bf16_pack_rne(lo, hi); }
    __device__ __forceinline__ int64_t image(int b, int64_t dense) const { return (int64_t)b * dense; }
};
struct CorrBf16Lrelu {
    int64_t stride;
    float slope;
    __device__ __forceinline__ unsigned pack(float lo, float hi) const {
        const unsigned m = bf16_pack_rne(lo, hi);
        const float a = __uint_as_float(m << 16), b = __uint_as_float(m & 0xffff0000u);
        return bf16_pack_rne(a > 0.0f ? a : a * slope, b > 0.0f ? b : b * slope);     // (a positive value: its own bits again)
    }
    __device__ __forceinline__ int64_t image(int b, int64_t) const { return (int64_t)b * stride; }
};

// The tensors of a launch of two calls of equal shape (the pair entries), and the two items' epilogues: each item has its
// own output base and its own image stride, and the slope is shared.  A pair kernel indexes its own arguments with the
// workgroup's item -- scalar loads -- and hands the body an epilogue of the single kernels' type.
struct CorrBf16Items { const bf16_t* in1[2]; const bf16_t* in2[2]; bf16_t* out[2]; };
struct CorrBf16PlainPair { typedef CorrBf16Plain One; };
struct CorrBf16LreluPair { typedef CorrBf16Lrelu One; int64_t stride[2]; float slope; };
__host__ __device__ __forceinline__ CorrBf16Plain corr_bf16_epilogue(const CorrBf16PlainPair&, int) { return {}; }
__host__ __device__ __forceinline__ CorrBf16Lrelu corr_bf16_epilogue(const CorrBf16LreluPair& e, int item) { return {e.stride[item], e.slope}; }

// ---------------------------------------------------------------------------------------------------------------- forward, MFMA
//
// A workgroup owns TW = 64 output pixels of TH = 2 output rows of one image; wave tj (of 9) owns displacement row tj.  Per
// chunk of 32 channels the workgroup stages the first map's TH x 64 pixels and the second map's (TH + 8) x 80 window
// (origin 4 left and 4 above the tile's centre pixels) in LDS TRANSPOSED, [row][pixel][32 channels]: a thread fetches the 8
// channels of one pixel and one channel group with eight 2-byte buffer loads (a wave's lanes are 64 adjacent pixels of a
// plane: 128-byte segments) and writes them as one 16-byte unit, which is exactly what a lane of
// v_mfma_f32_16x16x32_bf16 holds: lane l has A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15],
// j = 0..7.  A pixel's four units are 64 bytes; the unit of channel group g of pixel p sits in slot g ^ ((p >> 2) & 3), so
// the 16 lanes of a quarter wave (16 adjacent pixels, one group) touch 16 different 16-byte bank groups in the staging
// writes and in the operand reads alike.
//
// The loads go through a buffer descriptor that spans exactly the chunk's planes of the image: a pixel outside the frame
// has an offset out of any range and a channel past the last one falls out of the descriptor's, and both arrive as +0 --
// the zero padding (multiplied, not skipped: inf * 0 = NaN) and the zero fill of the K tail in BOTH operands.
//
// Per row and chunk a wave reads 4 A and 5 B operands and issues 8 MFMAs: pixel block m (16 pixels) against window blocks m
// and m + 1.  Accumulator (lane l, register v) of block pair (m, m + s) is C[x1 = 16 m + 4 (l >> 4) + v][x2 = 16 (m + s) +
// (l & 15)], displacement column ti = x2 - x1 (the window starts 4 to the left): the values with 0 <= ti <= 8 go to a
// wave-private LDS array [row][ti][64 pixels] (laid over the window), and come back with a lane owning two adjacent
// pixels: divide, one v_cvt_pk_bf16_f32, one 4-byte store -- a wave writes whole 128-byte segments of an output row per
// plane (2-byte stores where a pair is not 4-byte aligned or is cut by the frame).
template <int MT_, int TH_>
struct CorrMfmaTile {
    static constexpr int MD = 4, D = 2 * MD + 1, MT = MT_, TW = 16 * MT, TH = TH_, NB = MT + 1, BW = 16 * NB, LH = TH + 2 * MD;
    static constexpr int KC = 32, KG = KC / 8, NT = 64 * D;                     // channels per chunk, 16-byte units per pixel, threads
    static constexpr int A_UNITS = TH * TW * KG, B_UNITS = LH * BW * KG;
    static constexpr int NPA = (A_UNITS + NT - 1) / NT, NPB = (B_UNITS + NT - 1) / NT;
    static constexpr int TP = TW + 2;                                           // pitch of a row of the epilogue array, floats
    static constexpr int LDS_BYTES = (A_UNITS + B_UNITS) * 16;
    static_assert(D * TH * D * TP * 4 <= LDS_BYTES, "the epilogue arrays fit over the staged chunk");
    static_assert(LDS_BYTES <= 64 * 1024, "static LDS");
    static_assert(128 % TW == 0, "a wave's lanes are whole rows of pixel pairs");
    // slot of pixel p's channel group g, in units
    static __device__ __forceinline__ int unit(int p, int g) { return p * KG + (g ^ ((p >> 2) & (KG - 1))); }
};

template <class T, class Epi>
__device__ __forceinline__ void corr_mfma_bf16_body(
    const bf16_t* __restrict__ in1, const bf16_t* __restrict__ in2, bf16_t* __restrict__ out,
    int z0, int channel, int h, int w, int oh, int ow, int org, u32x4* lds, const Epi& epi) {
    constexpr int D = T::D, TW = T::TW, TH = T::TH, MT = T::MT, NB = T::NB, BW = T::BW, LH = T::LH, KG = T::KG, NT = T::NT;
    constexpr unsigned OUTSIDE = 0x80000000u;
    const int lane = threadIdx.x, tj = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int tid = tj * 64 + lane;
    const int ox0 = blockIdx.x * TW, oy0 = blockIdx.y * TH, b = blockIdx.z - z0;
    const int plane = h * w;
    const unsigned plane2 = 2u * (unsigned)plane;
    const bf16_t* f1 = in1 + (int64_t)b * channel * plane;
    const bf16_t* f2 = in2 + (int64_t)b * channel * plane;
    u32x4* lds_a = lds;
    u32x4* lds_b = lds + T::A_UNITS;

    // staging plan, the same for every chunk: unit e = tid + k * NT of the [KG][rows][pixels] block -> the byte offset of
    // its first channel from the chunk's first plane, and its LDS slot
    unsigned aoff[T::NPA], boff[T::NPB];
    int aslot[T::NPA], bslot[T::NPB];
#pragma unroll
    for (int k = 0; k < T::NPA; ++k) {
        const int e = tid + k * NT;
        const int p = e % TW, r = (e / TW) % TH, g = e / (TW * TH);
        const int gy = oy0 + r + org, gx = ox0 + p + org;
        const bool ok = e < T::A_UNITS && gy >= 0 && gy < h && gx >= 0 && gx < w;
        aoff[k] = ok ? 2u * (unsigned)(8 * g * plane + gy * w + gx) : OUTSIDE;
        aslot[k] = e < T::A_UNITS ? r * TW * KG + T::unit(p, g) : -1;
    }
#pragma unroll
    for (int k = 0; k < T::NPB; ++k) {
        const int e = tid + k * NT;
        const int q = e % BW, r = (e / BW) % LH, g = e / (BW * LH);
        const int gy = oy0 + r + org - T::MD, gx = ox0 + q + org - T::MD;
        const bool ok = e < T::B_UNITS && gy >= 0 && gy < h && gx >= 0 && gx < w;
        boff[k] = ok ? 2u * (unsigned)(8 * g * plane + gy * w + gx) : OUTSIDE;
        bslot[k] = e < T::B_UNITS ? r * BW * KG + T::unit(q, g) : -1;
    }

    f32x4 acc[TH][MT][2];
#pragma unroll
    for (int r = 0; r < TH; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) { acc[r][m][0] = f32x4{0, 0, 0, 0}; acc[r][m][1] = f32x4{0, 0, 0, 0}; }

    // a unit: the 8 channels of one pixel
    auto fetch = [&](const __amdgpu_buffer_rsrc_t& d, unsigned off) {
        unsigned v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            v[j] = __builtin_amdgcn_raw_buffer_load_b16(d, off == OUTSIDE ? OUTSIDE : off + (unsigned)j * plane2, 0, 0);
        return u32x4{v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16)};
    };
    const int li = lane & 15, lg = lane >> 4;
    const int opslot = T::unit(li, lg);                                          // (16 m + li has li's swizzle bits)

    for (int c0 = 0; c0 < channel; c0 += T::KC) {
        const int cn = min(T::KC, channel - c0);
        const auto d1 = buffer_rsrc(f1 + (int64_t)c0 * plane, cn * (int)plane2);
        const auto d2 = buffer_rsrc(f2 + (int64_t)c0 * plane, cn * (int)plane2);
        // (SB units -- 8 SB loads -- in flight per thread at a time.  All of a chunk's at once was measured SLOWER, 47.6 us
        //  against 42.8 at 32 x 288 x 496: the 2-byte loads' instruction count bounds the kernel, not their latency -- DESIGN.md 4.3a-4)
        constexpr int SB = 2;
        if (c0) __syncthreads();                                                 // the previous chunk has been read
#pragma unroll
        for (int k0 = 0; k0 < T::NPB; k0 += SB) {
            u32x4 u[SB];
#pragma unroll
            for (int k = k0; k < k0 + SB && k < T::NPB; ++k) u[k - k0] = fetch(d2, boff[k]);
#pragma unroll
            for (int k = k0; k < k0 + SB && k < T::NPB; ++k)
                if (bslot[k] >= 0) lds_b[bslot[k]] = u[k - k0];
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int k = 0; k < T::NPA; ++k) {
            const u32x4 u = fetch(d1, aoff[k]);
            if (aslot[k] >= 0) lds_a[aslot[k]] = u;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < TH; ++r) {
            bf16x8 a[MT], bb[NB];
#pragma unroll
            for (int m = 0; m < MT; ++m) a[m] = __builtin_bit_cast(bf16x8, lds_a[(r * TW + 16 * m) * KG + opslot]);
#pragma unroll
            for (int n = 0; n < NB; ++n) bb[n] = __builtin_bit_cast(bf16x8, lds_b[((r + tj) * BW + 16 * n) * KG + opslot]);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                acc[r][m][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], bb[m], acc[r][m][0], 0, 0, 0);
                acc[r][m][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], bb[m + 1], acc[r][m][1], 0, 0, 0);
            }
        }
    }
    __syncthreads();                                                             // the window has been read: it becomes the epilogue arrays

    float* t = reinterpret_cast<float*>(lds) + tj * (TH * D * T::TP);
#pragma unroll
    for (int r = 0; r < TH; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int i = 4 * lg + v, ti = li - i + 16 * s;
                    if (ti >= 0 && ti < D) t[(r * D + ti) * T::TP + 16 * m + i] = acc[r][m][s][v];
                }
    __syncthreads();

    const float nelems = (float)channel;
    // a lane owns one pixel pair; the wave's lanes are 128 / TW row segments (row r, displacement column ti) at a time
    const int px = 2 * (lane % (TW / 2)), ox = ox0 + px;
    const bool pair = ox + 1 < ow;
    for (int u = lane / (TW / 2); u < TH * D; u += 128 / TW) {
        const int r = u / D, ti = u - r * D;
        const int oy = oy0 + r;
        if (oy >= oh || ox >= ow) continue;
        const f32x2 s = *reinterpret_cast<const f32x2*>(&t[u * T::TP + px]);
        const unsigned two = epi.pack(s.x / nelems, s.y / nelems);
        // (the alignment is tested per store: an image stride that is odd moves every other image onto a 2-byte boundary)
        bf16_t* op = out + epi.image(b, (int64_t)(D * D) * oh * ow) + ((int64_t)(tj * D + ti) * oh + oy) * ow + ox;
        if (pair && (reinterpret_cast<uintptr_t>(op) & 3) == 0) {
            *reinterpret_cast<unsigned*>(op) = two;
        } else {
            op[0] = (bf16_t)(two & 0xffffu);
            if (pair) op[1] = (bf16_t)(two >> 16);
        }
    }
}

// (the body is a device function: the matrix-core builtin must not be instantiated by the host pass)
template <class T, class Epi>
__global__ __launch_bounds__(T::NT) void corr_forward_k1_mfma_bf16(
    const bf16_t* __restrict__ in1, const bf16_t* __restrict__ in2, bf16_t* __restrict__ out,
    int channel, int h, int w, int oh, int ow, int org, Epi epi) {
    __shared__ __attribute__((aligned(16))) u32x4 lds[T::LDS_BYTES / 16];
    corr_mfma_bf16_body<T>(in1, in2, out, 0, channel, h, w, oh, ow, org, lds, epi);
}

// Two calls of equal shape in ONE launch (vfi_correlation_forward_pair_bf16: the same pyramid level of a frame pair's two flow
// networks).  blockIdx.z is item x image, so the item is workgroup-uniform: its three pointers and its epilogue are scalar
// loads from the argument block at the item's index, and the body knows nothing of items -- an item's bits are those of its
// own corr_forward_k1_mfma_bf16 launch.
template <class T, class Epis>
__global__ __launch_bounds__(T::NT) void corr_forward_k1_mfma_bf16_pair(
    CorrBf16Items items, Epis epis, int batch, int channel, int h, int w, int oh, int ow, int org) {
    __shared__ __attribute__((aligned(16))) u32x4 lds[T::LDS_BYTES / 16];
    const int item = blockIdx.z >= (unsigned)batch ? 1 : 0;                      // (blockIdx.z / batch, of two items)
    const bf16_t* __restrict__ in1 = items.in1[item];
    const bf16_t* __restrict__ in2 = items.in2[item];
    bf16_t* __restrict__ out = items.out[item];
    corr_mfma_bf16_body<T>(in1, in2, out, item * batch, channel, h, w, oh, ow, org, lds, corr_bf16_epilogue(epis, item));
}
typedef CorrMfmaTile<4, 2> CorrMfma;

// ---------------------------------------------------------------------------------------------------------------- forward, generic
//
// Any kernel size / strides: one thread per output element, the arithmetic of corr_forward_generic (correlation.hip) on the
// widened values -- window rows outer, columns inner, channels in sequence, acc = fmaf(a, b, acc), the mean by division --
// rounded to bfloat16 once: bit for bit bf16_rne of the float32 entry on the widened maps.  A tap outside a map is the
// padding's +0 and is multiplied; outside both maps the term is fmaf(0, 0, acc) = acc (acc starts at +0 and is never -0) and
// is skipped.  With one tap inside, the lane runs the same loop: its outside tap is read at the inside tap's pixel (a valid
// address) and cleared by `keep`; eight channels of loads in flight (corr_forward_k1_flat's way, which this kernel stands
// in for at the small PWC-Net levels).
template <class Epi>
__device__ __forceinline__ void corr_generic_bf16_body(
    const bf16_t* __restrict__ in1, const bf16_t* __restrict__ in2, bf16_t* __restrict__ out,
    int batch, int channel, int h, int w, int oc, int oh, int ow, int pad, int kr, int md, int s1, int s2, int dr, Epi epi) {
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
    const bf16_t* f1 = in1 + (int64_t)b * channel * plane;
    const bf16_t* f2 = in2 + (int64_t)b * channel * plane;
    float acc = 0.0f;
    for (int j = -kr; j <= kr; ++j)
        for (int i = -kr; i <= kr; ++i) {
            const int ya = y1 + j, xa = x1 + i, yb = y2 + j, xb = x2 + i;
            const bool oka = ya >= 0 && ya < h && xa >= 0 && xa < w, okb = yb >= 0 && yb < h && xb >= 0 && xb < w;
            if (!oka && !okb) continue;
            const int64_t ata = (int64_t)ya * w + xa, atb = (int64_t)yb * w + xb;
            const bf16_t* pa = (oka ? f1 : f2) + (oka ? ata : atb);
            const bf16_t* pb = (oka ? f2 : f1) + (okb ? atb : ata);
            const bf16_t keep = (oka && okb) ? 0xffffu : 0u;
            int c = 0;
            for (; c + 8 <= channel; c += 8) {
                bf16_t va[8], vb[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) { va[q] = pa[(int64_t)(c + q) * plane]; vb[q] = pb[(int64_t)(c + q) * plane] & keep; }
#pragma unroll
                for (int q = 0; q < 8; ++q) acc = fmaf(bf16_widen(va[q]), bf16_widen(vb[q]), acc);
            }
            for (; c < channel; ++c) acc = fmaf(bf16_widen(pa[(int64_t)c * plane]), bf16_widen(pb[(int64_t)c * plane] & keep), acc);
        }
    const int k = 2 * kr + 1;
    const int64_t image = (int64_t)oc * oh * ow;
    out[epi.image(b, image) + (gid - (int64_t)b * image)] = (bf16_t)(epi.pack(acc / (float)(k * k * channel), 0.0f) & 0xffffu);
}

template <class Epi>
__global__ __launch_bounds__(256) void corr_forward_generic_bf16(
    const bf16_t* __restrict__ in1, const bf16_t* __restrict__ in2, bf16_t* __restrict__ out,
    int batch, int channel, int h, int w, int oc, int oh, int ow, int pad, int kr, int md, int s1, int s2, int dr, Epi epi) {
    corr_generic_bf16_body(in1, in2, out, batch, channel, h, w, oc, oh, ow, pad, kr, md, s1, s2, dr, epi);
}

// Two calls in one launch: the item is blockIdx.y -- a grid dimension of its own, so that it is workgroup-uniform (a flat
// index over both items' outputs would put two items into the workgroup at the seam) -- and blockIdx.x runs over ONE
// item's outputs exactly as in the single launch.
template <class Epis>
__global__ __launch_bounds__(256) void corr_forward_generic_bf16_pair(
    CorrBf16Items items, Epis epis, int batch, int channel, int h, int w, int oc, int oh, int ow, int pad, int kr, int md, int s1,
    int s2, int dr) {
    const int item = blockIdx.y;
    const bf16_t* __restrict__ in1 = items.in1[item];
    const bf16_t* __restrict__ in2 = items.in2[item];
    bf16_t* __restrict__ out = items.out[item];
    corr_generic_bf16_body(in1, in2, out, batch, channel, h, w, oc, oh, ow, pad, kr, md, s1, s2, dr, corr_bf16_epilogue(epis, item));
}

// ---------------------------------------------------------------------------------------------------------------- backward
//
// The float32 backward on bfloat16 storage.  The arithmetic (CorrBf16: float32 terms on exactly widened values, the mean
// rounded to bfloat16 once), the masks (CorrNoMask, CorrBf16GradLrelu) and both bodies are correlation_bwd.h's, shared with
// the float32 and half kernels of correlation.hip; the kernels here bind them to bfloat16.
// One thread per gradient element, any configuration:
template <bool SECOND, class Act>
__global__ __launch_bounds__(256) void corr_backward_bf16(
    const bf16_t* __restrict__ other, const bf16_t* __restrict__ gout, bf16_t* __restrict__ gin,
    int batch, int channel, int h, int w, int oc, int oh, int ow, int pad, int kr, int md, int s2, int dr, Act act) {
    corr_backward_body<CorrBf16, SECOND>(other, gout, gin, batch, channel, h, w, oc, oh, ow, pad, kr, md, s2, dr, act);
}

// PWC-Net's configuration (k == 1, strides 1, pad == md == 4): the tiled body, the same float32 terms in the same order as
// corr_backward_bf16, so the same bits.  corr_backward_k1_bf16 is one gradient per launch and includes the body's statements
// themselves: called through corr_backward_k1_body it compiled to slower code (see correlation_bwd_k1.inc).
typedef CorrNoMask<CorrBf16> CorrBf16Grad;

template <bool SECOND, class Act>
__global__ __launch_bounds__(256) void corr_backward_k1_bf16(
    const bf16_t* __restrict__ other, const bf16_t* __restrict__ gout, bf16_t* __restrict__ gin,
    int channel, int h, int w, int groups, int ch_per_group, Act act) {
    typedef CorrBf16 A;
    __shared__ CorrBwdWindow win;
    const CorrBwdTile t(channel, groups, ch_per_group);
#include "correlation_bwd_k1.inc"
}

// Up to four gradients of two calls of equal shape in ONE launch (vfi_correlation_backward_pair_bf16), as corr_backward_k1_pair
// (correlation.hip): a workgroup's role comes from blockIdx.z once (CorrBwdTile), its pointers are scalar loads from the
// argument block at the role's index, and one scalar branch picks the instance of the body.  Channel groups only partition
// the channels, so a gradient's bits are those of its own corr_backward_k1_bf16 launch.
typedef CorrBwdRolesT<bf16_t> CorrBf16BwdRoles;
typedef CorrBwdMasksT<bf16_t> CorrBf16BwdMasks;

__global__ __launch_bounds__(256) void corr_backward_k1_pair_bf16(CorrBf16BwdRoles roles, int channel, int h, int w, int groups,
                                                                  int ch_per_group) {
    __shared__ CorrBwdWindow win;
    const CorrBwdTile t(channel, groups, ch_per_group, roles.per_role);
    const bf16_t* __restrict__ other = roles.r[t.role].other;
    const bf16_t* __restrict__ gout = roles.r[t.role].gout;
    bf16_t* __restrict__ gin = roles.r[t.role].gin;
    if (roles.r[t.role].second) corr_backward_k1_body<CorrBf16, true>(win, t, other, gout, gin, channel, h, w, CorrBf16Grad{});
    else corr_backward_k1_body<CorrBf16, false>(win, t, other, gout, gin, channel, h, w, CorrBf16Grad{});
}

// the masked twin (vfi_correlation_lrelu_backward_pair_bf16): a role's y and strides are scalar loads at the role's index too
__global__ __launch_bounds__(256) void corr_lrelu_backward_k1_pair_bf16(CorrBf16BwdRoles roles, CorrBf16BwdMasks masks, int channel,
                                                                        int h, int w, int groups, int ch_per_group) {
    __shared__ CorrBwdWindow win;
    const CorrBwdTile t(channel, groups, ch_per_group, roles.per_role);
    const bf16_t* __restrict__ other = roles.r[t.role].other;
    const bf16_t* __restrict__ gout = roles.r[t.role].gout;
    bf16_t* __restrict__ gin = roles.r[t.role].gin;
    const CorrBf16GradLrelu act = {masks.y[t.role], masks.ystride[t.role], masks.gstride[t.role], masks.slope};
    if (roles.r[t.role].second) corr_backward_k1_body<CorrBf16, true>(win, t, other, gout, gin, channel, h, w, act);
    else corr_backward_k1_body<CorrBf16, false>(win, t, other, gout, gin, channel, h, w, act);
}

}  // namespace vfi

using namespace vfi;

// Number of 64x2 tiles of the MFMA forward kernel from which PWC-Net's configuration uses it; below it the level takes the
// one-thread-per-output kernel.
// Measured back to back, hot, MFMA vs generic (tools/bench_corr_bf16.py `choice` lines, profiles/corr_bf16_bench.txt): the
// MFMA kernel is faster at the five levels of 48 tiles and more (48 tiles, B=3 64 x 32 x 56: 10.8 vs 12.6 us; 72 tiles,
// 96 x 72 x 124: 12.7 vs 23.5), the generic kernel at the five of 24 and fewer (24 tiles, B=3 96 x 16 x 28: 12.4 vs 10.8;
// 18 tiles, 128 x 36 x 62: 15.9 vs 12.0; 9 tiles, 196 x 18 x 31: 22.2 vs 10.9 -- its channel loop is long there, but a
// launch this small is latency either way, and the MFMA kernel's chunk loop is seven dependent round trips).  Nothing was
// measured between 24 and 48.
static constexpr long long corr_bf16_mfma_threshold = 32;

static bool corr_bf16_is_pwc(int kernel_size, int max_displacement, int stride1, int stride2) {
    return kernel_size == 1 && stride1 == 1 && stride2 == 1 && max_displacement == 4;
}

// whether the MFMA kernel can take the frame: a chunk of 32 planes through one buffer descriptor, the grid's limits
static bool corr_bf16_mfma_fits(int batch, int h, int w, int oh) {
    return (int64_t)h * w * 2 * CorrMfma::KC < INT_MAX && batch <= 65535 && (oh + CorrMfma::TH - 1) / CorrMfma::TH <= 65535;
}

// The launchers take one item or two (nitems; `batch` is one item's).  Two items are ONE launch of the pair kernel where the
// doubled blockIdx.z fits; otherwise, and for one item, the single kernel per item -- the same bits either way.
template <class T, class Epis>
static int corr_bf16_launch_mfma(const CorrBf16Items& t, int nitems, const Epis& epis, int batch, int channel, int h, int w, int oh,
                                 int ow, int org, hipStream_t st) {
    const unsigned tx = (ow + T::TW - 1) / T::TW, ty = (oh + T::TH - 1) / T::TH;
    if (nitems == 2 && corr_bf16_mfma_fits(2 * batch, h, w, oh)) {
        hipLaunchKernelGGL((corr_forward_k1_mfma_bf16_pair<T, Epis>), dim3(tx, ty, 2 * batch), dim3(64, T::D, 1), 0, st, t, epis, batch,
                           channel, h, w, oh, ow, org);
        return launch_status();
    }
    for (int i = 0; i < nitems; ++i) {
        hipLaunchKernelGGL((corr_forward_k1_mfma_bf16<T, typename Epis::One>), dim3(tx, ty, batch), dim3(64, T::D, 1), 0, st, t.in1[i],
                           t.in2[i], t.out[i], channel, h, w, oh, ow, org, corr_bf16_epilogue(epis, i));
        if (launch_status() != VFI_OK) return VFI_ERR_LAUNCH;
    }
    return VFI_OK;
}

template <class Epis>
static int corr_bf16_launch_generic(const CorrBf16Items& t, int nitems, const Epis& epis, int batch, int channel, int h, int w, int oc,
                                    int oh, int ow, int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
                                    hipStream_t st) {
    const int64_t total = (int64_t)batch * oc * oh * ow;                 // of one item: blockIdx.x
    if ((total + 255) / 256 > INT_MAX) return VFI_ERR_SHAPE;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    const int kr = (kernel_size - 1) / 2, dr = max_displacement / stride2;
    if (nitems == 2) {
        hipLaunchKernelGGL(corr_forward_generic_bf16_pair<Epis>, dim3(blocks, 2), dim3(256), 0, st, t, epis, batch, channel, h, w, oc, oh,
                           ow, pad_size, kr, max_displacement, stride1, stride2, dr);
        return launch_status();
    }
    hipLaunchKernelGGL(corr_forward_generic_bf16<typename Epis::One>, dim3(blocks), dim3(256), 0, st, t.in1[0], t.in2[0], t.out[0], batch,
                       channel, h, w, oc, oh, ow, pad_size, kr, max_displacement, stride1, stride2, dr, corr_bf16_epilogue(epis, 0));
    return launch_status();
}

static bool corr_bf16_epilogue_ok(const CorrBf16PlainPair&, int, int64_t) { return true; }
static bool corr_bf16_epilogue_ok(const CorrBf16LreluPair& e, int nitems, int64_t image) {
    return corr_slope_ok(e.slope) && e.stride[0] >= image && e.stride[nitems - 1] >= image;
}

// The forward of all four entries: the checks, the kernel choice, one launch.  `batch` is one item's, and the choice is made
// on ONE item's tile count, for a pair too: the MFMA kernel's float32 addition order is the hardware's and not the generic
// kernel's chain, so only the single entry's own choice gives each item of a pair the single entry's bits.  (The float32
// pair chooses on the pair's count: its kernels all give the same bits.)
template <class Epis>
static int corr_bf16_forward(const CorrBf16Items& t, int nitems, const Epis& epis, int batch, int channel, int h, int w, int pad_size,
                             int kernel_size, int max_displacement, int stride1, int stride2, vfi_stream_t stream) {
    int oc, oh, ow;
    const int last = nitems - 1;
    if (corr_check({t.in1[0], t.in2[0], t.out[0], t.in1[last], t.in2[last], t.out[last]}, batch, channel, h, w, pad_size, kernel_size,
                   max_displacement, stride1, stride2, false, &oc, &oh, &ow))
        return VFI_ERR_SHAPE;
    if (nitems == 2 && t.out[0] == t.out[1]) return VFI_ERR_SHAPE;
    if (!corr_bf16_epilogue_ok(epis, nitems, (int64_t)oc * oh * ow)) return VFI_ERR_SHAPE;
    if (corr_bf16_is_pwc(kernel_size, max_displacement, stride1, stride2) && corr_bf16_mfma_fits(batch, h, w, oh)) {
        const int64_t mfma_tiles = (int64_t)((ow + CorrMfma::TW - 1) / CorrMfma::TW) * ((oh + CorrMfma::TH - 1) / CorrMfma::TH) * batch;
        if (mfma_tiles >= corr_bf16_mfma_threshold) {
            return corr_bf16_launch_mfma<CorrMfma>(t, nitems, epis, batch, channel, h, w, oh, ow, max_displacement - pad_size,
                                                   (hipStream_t)stream);
        }
    }
    return corr_bf16_launch_generic(t, nitems, epis, batch, channel, h, w, oc, oh, ow, pad_size, kernel_size, max_displacement, stride1,
                                    stride2, (hipStream_t)stream);
}

static CorrBf16Items corr_bf16_items(const void* input1_a, const void* input2_a, void* output_a, const void* input1_b = nullptr,
                                     const void* input2_b = nullptr, void* output_b = nullptr) {
    return {{(const bf16_t*)input1_a, (const bf16_t*)input1_b}, {(const bf16_t*)input2_a, (const bf16_t*)input2_b},
            {(bf16_t*)output_a, (bf16_t*)output_b}};
}

extern "C" int vfi_correlation_forward_bf16(const void* input1, const void* input2, void* output, int batch, int channel,
                                             int h, int w, int pad_size, int kernel_size, int max_displacement,
                                             int stride1, int stride2, vfi_stream_t stream) {
    return corr_bf16_forward(corr_bf16_items(input1, input2, output), 1, CorrBf16PlainPair{}, batch, channel, h, w, pad_size, kernel_size,
                             max_displacement, stride1, stride2, stream);
}

// vfi_correlation_forward_bf16 with PWC-Net's LeakyReLU applied to every stored value, into an output whose images lie
// output_batch_stride elements apart: the same kernels and the same choice, with the epilogue compiled in.
extern "C" int vfi_correlation_lrelu_forward_bf16(const void* input1, const void* input2, void* output, int64_t output_batch_stride,
                                                   int batch, int channel, int h, int w, int pad_size, int kernel_size,
                                                   int max_displacement, int stride1, int stride2, float negative_slope,
                                                   vfi_stream_t stream) {
    return corr_bf16_forward(corr_bf16_items(input1, input2, output), 1,
                             CorrBf16LreluPair{{output_batch_stride, output_batch_stride}, negative_slope}, batch, channel, h, w, pad_size,
                             kernel_size, max_displacement, stride1, stride2, stream);
}

// Two forward calls of equal shape in ONE launch -- the same pyramid level of the two flow networks of a frame pair: each
// output is its single entry's, bit for bit, for every shape (the kernel is the one the single entry takes for ONE item).
extern "C" int vfi_correlation_forward_pair_bf16(const void* input1_a, const void* input2_a, void* output_a,
                                                  const void* input1_b, const void* input2_b, void* output_b,
                                                  int batch, int channel, int h, int w, int pad_size, int kernel_size,
                                                  int max_displacement, int stride1, int stride2, vfi_stream_t stream) {
    return corr_bf16_forward(corr_bf16_items(input1_a, input2_a, output_a, input1_b, input2_b, output_b), 2, CorrBf16PlainPair{}, batch,
                             channel, h, w, pad_size, kernel_size, max_displacement, stride1, stride2, stream);
}

extern "C" int vfi_correlation_lrelu_forward_pair_bf16(const void* input1_a, const void* input2_a, void* output_a,
                                                        int64_t output_a_batch_stride,
                                                        const void* input1_b, const void* input2_b, void* output_b,
                                                        int64_t output_b_batch_stride,
                                                        int batch, int channel, int h, int w, int pad_size, int kernel_size,
                                                        int max_displacement, int stride1, int stride2, float negative_slope,
                                                        vfi_stream_t stream) {
    return corr_bf16_forward(corr_bf16_items(input1_a, input2_a, output_a, input1_b, input2_b, output_b), 2,
                             CorrBf16LreluPair{{output_a_batch_stride, output_b_batch_stride}, negative_slope}, batch, channel, h, w,
                             pad_size, kernel_size, max_displacement, stride1, stride2, stream);
}

// One kernel of vfi_correlation_forward_bf16 whatever the tile count (internal: the tests and tools/bench_corr_bf16.py run
// both kernels on the same frames).  which: 0 the MFMA kernel (PWC-Net's configuration only), 1 the generic kernel.
extern "C" int vfi_correlation_forward_bf16_kernel(int which, const void* input1, const void* input2, void* output, int batch,
                                                    int channel, int h, int w, int pad_size, int kernel_size, int max_displacement,
                                                    int stride1, int stride2, vfi_stream_t stream) {
    int oc, oh, ow;
    if (corr_check({input1, input2, output}, batch, channel, h, w, pad_size, kernel_size, max_displacement, stride1, stride2, false,
                   &oc, &oh, &ow))
        return VFI_ERR_SHAPE;
    const CorrBf16Items t = corr_bf16_items(input1, input2, output);
    if (which == 0) {
        if (!corr_bf16_is_pwc(kernel_size, max_displacement, stride1, stride2) || !corr_bf16_mfma_fits(batch, h, w, oh)) return VFI_ERR_SHAPE;
        return corr_bf16_launch_mfma<CorrMfma>(t, 1, CorrBf16PlainPair{}, batch, channel, h, w, oh, ow, max_displacement - pad_size,
                                               (hipStream_t)stream);
    }
    if (which != 1) return VFI_ERR_SHAPE;
    return corr_bf16_launch_generic(t, 1, CorrBf16PlainPair{}, batch, channel, h, w, oc, oh, ow, pad_size, kernel_size, max_displacement,
                                    stride1, stride2, (hipStream_t)stream);
}

// The backward entries: correlation_bwd.h's checks and launchers (the float32 entries' own) with this file's kernels.
struct CorrBwdBf16 {
    typedef bf16_t T;
    typedef CorrBf16GradLrelu Mask;
    static constexpr bool MASKED = true, PAIRED = true;
    static bool k1_fits(int, int) { return true; }
    template <class... Args>
    static void generic(bool second, const Mask* act, dim3 grid, hipStream_t st, Args... args) {
        if (act) hipLaunchKernelGGL((second ? corr_backward_bf16<true, Mask> : corr_backward_bf16<false, Mask>), grid, dim3(256), 0, st, args..., *act);
        else hipLaunchKernelGGL((second ? corr_backward_bf16<true, CorrBf16Grad> : corr_backward_bf16<false, CorrBf16Grad>), grid, dim3(256), 0, st, args..., CorrBf16Grad{});
    }
    template <class... Args>
    static void k1(bool second, const Mask* act, dim3 grid, hipStream_t st, Args... args) {
        if (act) hipLaunchKernelGGL((second ? corr_backward_k1_bf16<true, Mask> : corr_backward_k1_bf16<false, Mask>), grid, dim3(256), 0, st, args..., *act);
        else hipLaunchKernelGGL((second ? corr_backward_k1_bf16<true, CorrBf16Grad> : corr_backward_k1_bf16<false, CorrBf16Grad>), grid, dim3(256), 0, st, args..., CorrBf16Grad{});
    }
    template <class... Args>
    static void pair(const CorrBf16BwdRoles& roles, const CorrBf16BwdMasks* masks, dim3 grid, hipStream_t st, Args... args) {
        if (masks) hipLaunchKernelGGL(corr_lrelu_backward_k1_pair_bf16, grid, dim3(256), 0, st, roles, *masks, args...);
        else hipLaunchKernelGGL(corr_backward_k1_pair_bf16, grid, dim3(256), 0, st, roles, args...);
    }
};

extern "C" int vfi_correlation_backward_bf16(const void* input1, const void* input2, const void* gradoutput,
                                              void* gradinput1, void* gradinput2, int batch, int channel, int h, int w,
                                              int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
                                              vfi_stream_t stream) {
    return corr_backward_both<CorrBwdBf16>(input1, input2, gradoutput, gradinput1, gradinput2, batch, channel, h, w, pad_size, kernel_size,
                                           max_displacement, stride1, stride2, stream);
}

// vfi_correlation_backward_bf16 of gradOutput masked by LeakyReLU's derivative: the same two launches of the masked kernels.
extern "C" int vfi_correlation_lrelu_backward_bf16(const void* input1, const void* input2, const void* y, int64_t y_batch_stride,
                                                    const void* gradoutput, int64_t gradoutput_batch_stride, void* gradinput1,
                                                    void* gradinput2, int batch, int channel, int h, int w, int pad_size,
                                                    int kernel_size, int max_displacement, int stride1, int stride2,
                                                    float negative_slope, vfi_stream_t stream) {
    const CorrBf16GradLrelu act = {(const bf16_t*)y, y_batch_stride, gradoutput_batch_stride, negative_slope};
    return corr_backward_both<CorrBwdBf16>(input1, input2, gradoutput, gradinput1, gradinput2, batch, channel, h, w, pad_size, kernel_size,
                                           max_displacement, stride1, stride2, stream, &act);
}

extern "C" int vfi_correlation_backward_pair_bf16(
    const void* input1_a, const void* input2_a, const void* gradoutput_a, void* gradinput1_a, void* gradinput2_a,
    const void* input1_b, const void* input2_b, const void* gradoutput_b, void* gradinput1_b, void* gradinput2_b,
    int batch, int channel, int h, int w, int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
    vfi_stream_t stream) {
    return corr_backward_pair<CorrBwdBf16>(corr_backward_items<bf16_t>(input1_a, input2_a, gradoutput_a, gradinput1_a, gradinput2_a, input1_b,
                                                                       input2_b, gradoutput_b, gradinput1_b, gradinput2_b),
                                           nullptr, batch, channel, h, w, pad_size, kernel_size, max_displacement, stride1, stride2, stream);
}

extern "C" int vfi_correlation_lrelu_backward_pair_bf16(
    const void* input1_a, const void* input2_a, const void* y_a, int64_t y_a_batch_stride, const void* gradoutput_a,
    int64_t gradoutput_a_batch_stride, void* gradinput1_a, void* gradinput2_a,
    const void* input1_b, const void* input2_b, const void* y_b, int64_t y_b_batch_stride, const void* gradoutput_b,
    int64_t gradoutput_b_batch_stride, void* gradinput1_b, void* gradinput2_b,
    int batch, int channel, int h, int w, int pad_size, int kernel_size, int max_displacement, int stride1, int stride2,
    float negative_slope, vfi_stream_t stream) {
    const CorrBf16GradLrelu acts[2] = {{(const bf16_t*)y_a, y_a_batch_stride, gradoutput_a_batch_stride, negative_slope},
                                       {(const bf16_t*)y_b, y_b_batch_stride, gradoutput_b_batch_stride, negative_slope}};
    return corr_backward_pair<CorrBwdBf16>(corr_backward_items<bf16_t>(input1_a, input2_a, gradoutput_a, gradinput1_a, gradinput2_a, input1_b,
                                                                       input2_b, gradoutput_b, gradinput1_b, gradinput2_b),
                                           acts, batch, channel, h, w, pad_size, kernel_size, max_displacement, stride1, stride2, stream);
}
