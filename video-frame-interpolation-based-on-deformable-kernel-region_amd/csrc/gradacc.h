// gradacc.h -- the deterministic fixed-point accumulator every image gradient of the library goes through (gradacc.hip).
#pragma once
#include "bf16.h"
#include "vfi_common.h"

namespace vfi {

// Deterministic image gradients.  The reference scatters the image gradient of its warping layers with fp32 atomics
// (filterinterpolation_cuda_kernel.cu:2890-2942, interpolation_cuda_kernel.cu:154-157): the sum depends on the order the
// atomics arrive in, so two runs differ in the last bits.  Here every addend is scaled by ONE power of two per call,
// rounded to an integer and added with a 64-bit INTEGER atomic into a scratch plane; a last pass converts the exact
// integer sums to float once and adds them to the caller's (zero-filled) gradient.  Order-free, hence reproducible bit
// for bit.  The scale is 2^(62 - ceil(log2(h w T)) - eg - ew) with 2^eg > max |gradoutput|, 2^ew > max |tap weight|
// (the filter tensor; 1 where the weights are bilinear fractions only) and T = the taps of a pixel (fs x fs; 4 for a
// bilinear sample): an addend is below 2^(62 - ceil(log2(h w T))) and even a cell that EVERY tap of EVERY pixel of the frame
// hits (border clamping folds a pixel's taps onto one cell) stays inside 63 bits -- no combination of finite inputs overflows.
// The scale is applied as two power-of-two factors (2^min(k, 126), then 2^(k - min(k, 126))): k exceeds 126 when the inputs
// are tiny, and one fp32 factor clamped at 2^126 would round those addends onto a coarse grid.  Where k <= 126 the second
// factor is 1 and the bits are those of a single multiply.
// fp32 atomics instead: the first pass raises a flag when gradoutput or the weights hold a NaN or an infinity, and the
// kernels scatter with the reference's own fp32 atomics for that call when the flag is up OR when 2^eg x 2^ew reaches
// 2^128, i.e. when finite inputs admit a product that overflows to an infinity (NaN / Inf propagate to exactly the cells
// the reference would poison; the integer path would turn them into finite garbage).  gradacc_fp32 is that one predicate.
//   host:   gradacc_begin (zeroes the scratch; largest |gradoutput|, largest |weight|, non-finite flag)  ->  the backward kernel
//           ->  gradacc_finish
//   device: gradacc_ctx(hdr) once per thread, gradacc_add(...) per addend; cells are indexed densely [b][c][y][x] whatever
//           the strides of the gradient tensor.
// hdr words: [0] bits of max |gradoutput|, [1] non-finite flag, [2] bits of max |weight| (0: none given), [3] ceil(log2(h w T))
struct GradAccCtx { float scale, scale2; bool nonfinite; };
// eg + ew: 2^eg > max |gradoutput|, 2^ew > max |tap weight|
__device__ __forceinline__ int gradacc_magnitude(const int* __restrict__ hdr) {
    int eg = 0, ew = 1;                                     // no weight tensor: |weight| <= 1 < 2^1
    (void)frexpf(__int_as_float(hdr[0]), &eg);
    if (hdr[2] != 0) (void)frexpf(__int_as_float(hdr[2]), &ew);
    return eg + max(ew, 1);
}
// the scale exponent k (not clamped: from 62 - L - 256 to 62 - L + 147; the integer path only sees k >= -66 - L)
__device__ __forceinline__ int gradacc_exponent(const int* __restrict__ hdr) {
    return 62 - hdr[3] - gradacc_magnitude(hdr);
}
// true: this call scatters with fp32 atomics (a non-finite input, or finite inputs whose product can reach 2^128)
__device__ __forceinline__ bool gradacc_fp32(const int* __restrict__ hdr) {
    return hdr[1] != 0 || gradacc_magnitude(hdr) > 128;
}
__device__ __forceinline__ GradAccCtx gradacc_ctx(const int* __restrict__ hdr) {
    GradAccCtx c;
    const int k = gradacc_exponent(hdr);
    const int k1 = max(-126, min(126, k));
    c.scale = ldexpf(1.0f, k1);
    c.scale2 = ldexpf(1.0f, max(-126, min(126, k - k1)));    // 1 unless k > 126 (k - k1 <= 81 then)
    c.nonfinite = gradacc_fp32(hdr);
    return c;
}
// v * 2^k: exact (a power-of-two scaling of an fp32 value that stays in range), bit-identical to v * scale when k <= 126
__device__ __forceinline__ float gradacc_scaled(float v, const GradAccCtx& cx) { return v * cx.scale * cx.scale2; }
// The LDS-staged kernels multiply by `scale` alone (one multiply per addend in their inner loops) and leave a call whose scale
// needs the second factor (k > 126: tiny gradients) to the per-tap kernels, as they do a call that scatters in fp32.
__device__ __forceinline__ bool gradacc_staged_ok(const GradAccCtx& cx) { return !cx.nonfinite && cx.scale2 == 1.0f; }
// acc_plane / g_plane: the channel's plane of the dense scratch and of the caller's gradient tensor; di / gi: the cell's
// index in each
__device__ __forceinline__ void gradacc_add(unsigned long long* acc_plane, float* g_plane, int64_t di, int64_t gi, float v,
                                            const GradAccCtx& cx) {
    if (cx.nonfinite) atomicAdd(&g_plane[gi], v);
    else atomicAdd(&acc_plane[di], (unsigned long long)__float2ll_rn(gradacc_scaled(v, cx)));
}

// The incoming gradient of one direction of the blend's backward (vfi_filterinterp_blend_backward), formed in registers where
// it is read: g = gb * wgt + go, the product and the sum rounded separately (torch autograd's accumulation for
// out * w + <another use of out>).  A NULL term is absent; with both NULL the direction has no gradient.
// row(o): the gradient from element o on, indexed like a pointer (a plain gradient's row is the pointer itself: GradPlain).
struct GradTerms {
    const float* gb;
    const float* go;
    float wgt;
    struct Row {
        const float* gb;
        const float* go;
        float wgt;
        __device__ __forceinline__ float operator[](int64_t o) const {
            if (!gb) return go[o];
            const float v = gb[o] * wgt;
            return go ? v + go[o] : v;
        }
    };
    __host__ __device__ bool any() const { return gb != nullptr || go != nullptr; }
    __device__ __forceinline__ Row row(int64_t o) const { return Row{gb ? gb + o : nullptr, go ? go + o : nullptr, wgt}; }
};
struct GradPlain {
    const float* __restrict__ g;
    __host__ __device__ bool any() const { return true; }
    __device__ __forceinline__ const float* row(int64_t o) const { return g + o; }
};

// a plain gradient in bfloat16 storage: its elements widened (exactly) as they are read, so the max-scan sees the values the
// float32 entry sees for the widened tensor, and the scale is the same
struct GradBf16 {
    const bf16_t* __restrict__ g;
    struct Row {
        const bf16_t* g;
        __device__ __forceinline__ float operator[](int64_t o) const { return bf16_widen(g[o]); }
    };
    __host__ __device__ bool any() const { return true; }
    __device__ __forceinline__ Row row(int64_t o) const { return Row{g + o}; }
};

// The WS_GRADACC scratch of a call: [ndirs headers of 256 B][ndirs x cells 64-bit sums][nflags 32-bit words], ndirs 0, 1 or 2
// (one header and one plane of sums per gradient the call accumulates; the flag words are the caller's kernels'): offsets
// from gradacc_layout alone.
struct GradAccDir { unsigned long long* acc; int* hdr; };
struct GradAccScratch { GradAccDir dir[2]; int* flags; };
struct GradAccLayout { size_t hdr[2], acc[2], flags, bytes; };
constexpr GradAccLayout gradacc_layout(size_t ndirs, size_t cells, size_t nflags) {       // (hdr[d] / acc[d]: for d < ndirs)
    const size_t sums = 256 * ndirs, flags = sums + 8 * cells * ndirs;
    return GradAccLayout{{0, 256}, {sums, sums + 8 * cells}, flags, flags + 4 * nflags};
}
constexpr GradAccLayout GA0 = gradacc_layout(0, 100, 7), GA1 = gradacc_layout(1, 100, 7), GA2 = gradacc_layout(2, 100, 7);
static_assert(GA0.flags == 0 && GA0.bytes == 4 * 7, "no direction: flags only");
static_assert(GA1.hdr[0] == 0 && GA1.acc[0] == 256 && GA1.flags == 256 + 8 * 100 && GA1.bytes == 256 + 8 * 100 + 4 * 7, "one direction");
static_assert(GA2.hdr[0] == 0 && GA2.hdr[1] == 256 && GA2.acc[0] == 512 && GA2.acc[1] == 512 + 8 * 100 &&
              GA2.flags == 512 + 16 * 100 && GA2.bytes == 512 + 16 * 100 + 4 * 7, "two directions");

// Takes the slot for ndirs directions of `cells` sums and nflags flag words, zero-fills exactly those bytes on the stream and
// fills *s (a direction not laid out, and flags when nflags is 0: null).  Nothing to lay out: touches nothing.
int gradacc_reserve(hipStream_t st, int ndirs, int64_t cells, int nflags, GradAccScratch* s);
// The max-scans of the gradient g (GradPlain or GradTerms) and of the weights into a zeroed header.
// weights (may be null): a [batch, wchannel, h, w] tensor whose largest |element| bounds the tap weights; wchannel = the taps
// of a pixel (also when weights is null; below 4: 4)
template <class G>
int gradacc_scan(hipStream_t st, G g, int batch, int channel, int h, int w, vfi_strides sg, const float* weights, int wchannel,
                 vfi_strides sw, int* hdr);
// one direction with nflags flag words: gradacc_reserve, then gradacc_scan of the plain gradient gout
int gradacc_begin(hipStream_t st, const float* gout, int batch, int channel, int h, int w, vfi_strides sg,
                  const float* weights, int wchannel, vfi_strides sw, int nflags, GradAccScratch* s);
// zero the caller's gradient when the call scatters with fp32 atomics (for a caller that does not zero it)
int gradacc_zero_fp32(hipStream_t st, const int* hdr, float* g1, int batch, int channel, int h, int w, vfi_strides s1);
// the sums to float, added into g1; overwrite: WRITTEN to every cell of g1 (0 where the sum is 0) instead
int gradacc_finish(hipStream_t st, const GradAccDir& d, float* g1, int batch, int channel, int h, int w, vfi_strides s1,
                   bool overwrite = false);


// bfloat16 gradients (vfi_pwc_warp_backward_bf16).  gradacc_begin_bf16: gradacc_begin for a bfloat16 gradoutput, no weights.
// A call that gradacc_fp32 sends to fp32 atomics never adds into bfloat16 storage: its kernel adds FLOATS into the low
// words of the zeroed 64-bit cells (gradacc_add with the scratch plane as the float plane, float index 2 x cell index).
// gradacc_finish_bf16 WRITES every cell of the bfloat16 gradient g1 -- bf16_rne of the float the float32 finish would leave
// in a zero-filled gradient (the converted integer sum, +0 where it is 0), or of the cell's float on the fp32 path: one
// rounding either way.
int gradacc_begin_bf16(hipStream_t st, const bf16_t* gout, int batch, int channel, int h, int w, vfi_strides sg, int taps,
                       GradAccScratch* s);
int gradacc_finish_bf16(hipStream_t st, const GradAccDir& d, bf16_t* g1, int batch, int channel, int h, int w, vfi_strides s1);

}  // namespace vfi
