// correlation_bwd.h -- the correlation backward, once for every storage type (correlation.hip: float32 and half;
// correlation_bf16.hip: bfloat16).  Device side: the arithmetic of a storage type (CorrF32, CorrF16, CorrBf16), what a
// gradOutput value becomes as it is loaded (CorrNoMask, CorrGradLrelu, CorrBf16GradLrelu), the one-thread-per-element body, and
// the tile, the roles and the body of the tiled kernels (the statements: correlation_bwd_k1.inc).  Host side: the checks and
// the three launchers every backward entry forwards to, written against a struct in which a file names its own kernels.
// The __global__ kernels stay in their files: a kernel's instructions depend on what else its translation unit holds
// (DESIGN.md 4.3a-6).  Internal to the library.
#pragma once
#include "bf16.h"
#include "correlation_dev.h"

#include <climits>

#include <hip/hip_fp16.h>

namespace vfi {

// ------------------------------------------------------------------------------------------------------------ arithmetic
//
// The arithmetic of a backward kernel: the storage type T and the type S the sums run in, zero, the count the mean divides
// by, a loaded value, the term s <- s (+) g (*) v, the sum of two partials, and the mean as it is stored.  CorrF32 is the
// reference's float instantiation, its `acc += a * b` fused as nvcc fuses it.
struct CorrF32 {
    typedef float T;
    typedef float S;
    static __device__ __forceinline__ S zero() { return 0.0f; }
    static __device__ __forceinline__ float count(int n) { return (float)n; }
    static __device__ __forceinline__ S load(T v) { return v; }
    static __device__ __forceinline__ S term(S s, S g, S v) { return fmaf(g, v, s); }
    static __device__ __forceinline__ S add(S r, S s) { return r + s; }
    static __device__ __forceinline__ T store(S r, float nelems) { return r / nelems; }
    static __device__ __forceinline__ T store_zero() { return 0.0f; }
};

// The reference's at::Half instantiation of the backward (correlation_cuda_kernel.cu:151-334, dispatched at :495-541).
// The terms, windows and skips are corr_backward's; the arithmetic is at::Half's, which goes through float and rounds back to
// half after every operation: p = half(g * v), the 32 partials `__shared__ scalar_t prod_sum[32]` accumulate IN HALF,
// r = half(r + s_l) for l = 0..31, gin = half(r / nelems_h) with nelems_h = half(k*k*C) (not the exact count above 2048).
// float32 has 24 >= 2*11 + 2 significand bits, so float-then-round is the correctly rounded half operation: the products and
// sums here are plain v_mul_f16 / v_add_f16 (never fused: -ffp-contract=off, no fma written), and the one division is done in
// float on the two widened halves and rounded once.  A term whose other-map tap lies in the zero padding is NOT skipped: it
// adds half(g * 0), which is NaN when g is inf or NaN.
__device__ __forceinline__ __half corr_mean_f16(__half r, float nelems_h) {
    float rf = __half2float(r);
    asm volatile("" : "+v"(rf));        // (keeps the widening a v_cvt: nothing mixed-precision may be folded into the division)
    return __float2half_rn(rf / nelems_h);
}

struct CorrF16 {
    typedef __half T;
    typedef __half S;
    static __device__ __forceinline__ S zero() { return __float2half_rn(0.0f); }
    static __device__ __forceinline__ float count(int n) { return __half2float(__float2half_rn((float)n)); }   // nelems_h
    static __device__ __forceinline__ S load(T v) { return v; }
    static __device__ __forceinline__ S term(S s, S g, S v) { return __hadd(s, __hmul(g, v)); }
    static __device__ __forceinline__ S add(S r, S s) { return __hadd(r, s); }
    static __device__ __forceinline__ T store(S r, float nelems_h) { return corr_mean_f16(r, nelems_h); }
    static __device__ __forceinline__ T store_zero() { return zero(); }
};

// bfloat16 storage: CorrF32's arithmetic on exactly widened values, the mean rounded to bfloat16 once, to nearest even.
struct CorrBf16 {
    typedef bf16_t T;
    typedef float S;
    static __device__ __forceinline__ S zero() { return 0.0f; }
    static __device__ __forceinline__ float count(int n) { return (float)n; }
    static __device__ __forceinline__ S load(T v) { return bf16_widen(v); }
    static __device__ __forceinline__ S term(S s, S g, S v) { return fmaf(g, v, s); }
    static __device__ __forceinline__ S add(S r, S s) { return r + s; }
    static __device__ __forceinline__ T store(S r, float nelems) { return bf16_rne(r / nelems); }
    static __device__ __forceinline__ T store_zero() { return 0; }             // +0: the binding zero-fills gradInput
};

// ------------------------------------------------------------------------------------------------------------ the mask
//
// What a backward kernel does with a gradOutput value g whose output position holds yv as it loads it, and where the images
// of gradOutput and y begin (workgroup-uniform scalars).  CorrNoMask: the loaded value, dense images.  The masked types:
// LeakyReLU's derivative through the saved ACTIVATED output y (its sign is the pre-activation's for any slope > 0), g' = yv >
// 0 ? g : g * slope in the storage type -- rounded before the term that uses it, so the gradient is the plain kernel's fed g'
// -- with images of y and of gradOutput ystride / gstride elements apart and the planes of an image contiguous (gradOutput:
// the narrow() view that torch.cat's backward hands down).
// SELECT_LOADS: how the tiled kernels drop the pair they load for a skipped term -- `act(ok ? g : 0, ok ? yv : 0)` or
// `ok ? act(g, yv) : 0`, equal values.  Each storage type keeps the form its kernels have been timed with: the other one
// compiles to a different kernel.
template <class A>
struct CorrNoMask {
    static constexpr bool MASK = false;
    __device__ __forceinline__ const typename A::T* y_image(int) const { return nullptr; }
    __device__ __forceinline__ int64_t g_image(int n, int64_t dense) const { return (int64_t)n * dense; }
    __device__ __forceinline__ typename A::S operator()(typename A::T g, typename A::T) const { return A::load(g); }
};
struct CorrGradLrelu {
    static constexpr bool MASK = true, SELECT_LOADS = true;
    const float* y;
    int64_t ystride, gstride;
    float slope;
    __device__ __forceinline__ const float* y_image(int n) const { return y + (int64_t)n * ystride; }
    __device__ __forceinline__ int64_t g_image(int n, int64_t) const { return (int64_t)n * gstride; }
    // (a skipped term: 0 * slope = +0, slope finite and positive)
    __device__ __forceinline__ float operator()(float g, float yv) const { return yv > 0.0f ? g : g * slope; }
};
// bfloat16: g' = yv > 0 ? g : bf16_rne(float(g) * slope) -- torch's bfloat16 leaky_relu backward, a materialised bfloat16 g'
struct CorrBf16GradLrelu {
    static constexpr bool MASK = true, SELECT_LOADS = false;
    const bf16_t* y;
    int64_t ystride, gstride;
    float slope;
    __device__ __forceinline__ const bf16_t* y_image(int n) const { return y + (int64_t)n * ystride; }
    __device__ __forceinline__ int64_t g_image(int n, int64_t) const { return (int64_t)n * gstride; }
    __device__ __forceinline__ float operator()(bf16_t g, bf16_t yv) const {
        const float gf = bf16_widen(g);
        return bf16_widen(yv) > 0.0f ? gf : bf16_widen(bf16_rne(gf * slope));
    }
};

// ------------------------------------------------------------------------------------------------------------ one thread per element
//
// backward, stride1 == 1, any pad / k / md / stride2 (correlation_cuda_kernel.cu:151-334).  One thread per gradient
// element; the reference's reduction order (32 partial sums over tc = l, l+32, ..., then a sequential sum of the
// partials) is kept.  A term whose other-map tap lies in the zero padding is not skipped: it adds g * 0 in A's arithmetic
// (NaN for an infinite g).
template <class A, bool SECOND, class Act>
__device__ __forceinline__ void corr_backward_body(
    const typename A::T* __restrict__ other, const typename A::T* __restrict__ gout, typename A::T* __restrict__ gin,
    int batch, int channel, int h, int w, int oc, int oh, int ow, int pad, int kr, int md, int s2, int dr, const Act& act) {
    typedef typename A::T T;
    typedef typename A::S S;
    const int64_t total = (int64_t)batch * channel * h * w;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int bx = (int)(gid % w);
    const int by = (int)((gid / w) % h);
    const int c = (int)((gid / ((int64_t)w * h)) % channel);
    const int n = (int)(gid / ((int64_t)w * h * channel));
    const int dsz = 2 * dr + 1;
    const int y = by + pad, x = bx + pad;                   // padded coordinates
    const T* of = other + ((int64_t)n * channel + c) * h * w;
    const T* go = gout + act.g_image(n, (int64_t)oc * oh * ow);
    const T* yo = act.y_image(n);
    const float nelems = A::count((2 * kr + 1) * (2 * kr + 1) * channel);
    bool any = SECOND;
    if constexpr (!SECOND) {
        const int xmin = x - kr - md, ymin = y - kr - md, xmax = x + kr - md, ymax = y + kr - md;
        any = !(xmax < 0 || ymax < 0 || xmin >= ow || ymin >= oh || xmin > xmax || ymin > ymax);
    }
    if (!any) {
        gin[gid] = A::store_zero();   // the binding zero-fills gradInput (correlation_cuda.cc:112-113)
        return;
    }
    S r = A::zero();
    for (int l = 0; l < 32; ++l) {
        S s = A::zero();
        for (int tc = l; tc < oc; tc += 32) {
            const int i2 = (tc % dsz - dr) * s2, j2 = (tc / dsz - dr) * s2;
            int xmin, ymin, xmax, ymax, vy, vx;
            if constexpr (SECOND) {
                xmin = x - kr - md - i2; ymin = y - kr - md - j2;
                xmax = x + kr - md - i2; ymax = y + kr - md - j2;
                if (xmax < 0 || ymax < 0 || xmin >= ow || ymin >= oh || xmin > xmax || ymin > ymax) continue;
                vy = y - j2 - pad; vx = x - i2 - pad;
            } else {
                xmin = x - kr - md; ymin = y - kr - md; xmax = x + kr - md; ymax = y + kr - md;
                vy = y + j2 - pad; vx = x + i2 - pad;
            }
            const S val = (vy >= 0 && vy < h && vx >= 0 && vx < w) ? A::load(of[(int64_t)vy * w + vx]) : A::zero();
            xmin = max(0, xmin); xmax = min(ow - 1, xmax);
            ymin = max(0, ymin); ymax = min(oh - 1, ymax);
            const T* g = go + (int64_t)tc * oh * ow;
            for (int j = ymin; j <= ymax; ++j)
                for (int i = xmin; i <= xmax; ++i) {
                    const int64_t at = (int64_t)j * ow + i;
                    const T yv = Act::MASK ? yo[(int64_t)tc * oh * ow + at] : A::store_zero();
                    s = A::term(s, act(g[at], yv), val);
                }
        }
        r = A::add(r, s);
    }
    gin[gid] = A::store(r, nelems);
}

// ------------------------------------------------------------------------------------------------------------ tiled
//
// The tile of the tiled backward kernels (PWC-Net's configuration: k == 1, strides 1, pad == md == 4): a workgroup owns 64x4
// pixels of one image and one channel group, and stages the other map's window (tile + 4 halo, zero padded) per channel.
// blockIdx.z is image x channel group, and in a launch of several roles (per_role = images x groups of one role; 0: the
// launch has one role) role x image x channel group.  All of it is workgroup-uniform.
struct CorrBwdTile {
    static constexpr int MD = 4, D = 2 * MD + 1, OC = D * D, TW = 64, TH = 4, LW = TW + 2 * MD, LH = TH + 2 * MD;
    int role, x0, y0, n, c_begin, c_end;
    __device__ __forceinline__ CorrBwdTile(int channel, int groups, int ch_per_group, int per_role = 0) {
        x0 = blockIdx.x * TW; y0 = blockIdx.y * TH;
        role = per_role ? blockIdx.z / per_role : 0;
        const unsigned z = blockIdx.z - role * per_role;
        n = z / groups;
        c_begin = (z - n * groups) * ch_per_group;
        c_end = min(channel, c_begin + ch_per_group);
    }
    // window element e: its row and column in the window and its position in the frame (outside it: the zero padding)
    struct Elem { int r, col, gy, gx; };
    __device__ __forceinline__ Elem window(int e) const {
        const int r = e / LW, col = e - r * LW;
        return {r, col, y0 - MD + r, x0 - MD + col};
    }
};
// the two staged windows of a workgroup, float for every storage type (bfloat16 is widened as it is staged)
typedef float CorrBwdWindow[2][CorrBwdTile::LH][CorrBwdTile::LW];

// The tiled body (A::S == float: CorrF32, CorrBf16; the half kernel has a packed design of its own, corr_backward_k1_f16).  A
// thread owns one PIXEL: its 81 gradOutput values (gradInput1: the 81 planes at the pixel; gradInput2: plane tc at the pixel
// moved back by displacement tc) live in registers for all channels of the group, through the mask as they are loaded, and
// per channel the workgroup stages the other map's window in LDS, double-buffered.  The sum runs in the reference's order
// -- 32 partial sums over tc = l, l + 32, l + 64, added in sequence (correlation_cuda_kernel.cu:162-239, 255-332) -- so the
// result is corr_backward_body's and the oracle's bit for bit.  The statements are correlation_bwd_k1.inc: this function
// for the kernels that pick an instance per workgroup (the pair kernels) and the float32 single kernels; the bfloat16
// single kernels include the statements themselves (called through the function they compiled to slower code).
template <class A, bool SECOND, class Act>
__device__ __forceinline__ void corr_backward_k1_body(
    CorrBwdWindow& win, const CorrBwdTile& t, const typename A::T* __restrict__ other, const typename A::T* __restrict__ gout,
    typename A::T* __restrict__ gin, int channel, int h, int w, const Act& act) {
#include "correlation_bwd_k1.inc"
}

// The gradients of one paired launch: a role is one requested gradient of one item -- the map its window is staged from,
// the item's gradOutput, where it goes, and which of the two gradients it is.  The host compacts the requested ones (at
// most four) to the front; role i owns blockIdx.z in [i * per_role, (i + 1) * per_role).  E: the storage type.
template <class E>
struct CorrBwdRoleT { const E* other; const E* gout; E* gin; int second; };
template <class E>
struct CorrBwdRolesT { CorrBwdRoleT<E> r[4]; int per_role; };
typedef CorrBwdRolesT<float> CorrBwdRoles;
// the masks of a masked paired launch, by role
template <class E>
struct CorrBwdMasksT { const E* y[4]; int64_t ystride[4], gstride[4]; float slope; };
typedef CorrBwdMasksT<float> CorrBwdMasks;

// ------------------------------------------------------------------------------------------------------------ host
//
// A file names its kernels in a struct K:
//   T, Mask               the storage type; the mask the masked entries build (y, ystride, gstride, slope)
//   MASKED, PAIRED        whether the file has masked kernels and pair kernels (half has neither)
//   k1_fits(h, w)         whether the tiled kernel can take the frame beyond what its grid needs
//   generic(second, act, grid, st, args...), k1(second, act, grid, st, args...)
//                         launch the one-thread-per-element / the tiled kernel of one gradient, masked where act != NULL
//   pair(roles, masks, grid, st, args...)
//                         launch the tiled pair kernel, masked where masks != NULL
// One rule for errors: the code of the step that failed.

// a mask the entries accept: y present, a valid slope, images at least their own planes apart
template <class Mask>
inline bool corr_grad_ok(const Mask& a, int64_t image) {
    return a.y && corr_slope_ok(a.slope) && a.ystride >= image && a.gstride >= image;
}

// One gradient, one launch: gradInput1 (second == false) from other = input2, gradInput2 from other = input1.  `act` (or
// NULL): gradOutput goes through LeakyReLU's derivative as it is loaded -- the same launches of the masked kernels.  The
// callers have run corr_check.
template <class K>
inline int corr_backward_one(bool second, const typename K::T* other, const typename K::T* gout, typename K::T* gin, int batch,
                             int channel, int h, int w, int oc, int oh, int ow, int pad_size, int kernel_size, int max_displacement,
                             int stride2, hipStream_t st, const typename K::Mask* act) {
    if (!K::MASKED && act) return VFI_ERR_SHAPE;
    if (kernel_size == 1 && stride2 == 1 && max_displacement == 4 && pad_size == 4) {
        // PWC-Net's configuration: the pixel-owns-its-gradOutput kernels; channel groups over blockIdx.z fill the chip
        int ch_per_group;
        const int groups = corr_backward_groups(((w + 63) / 64) * ((h + 3) / 4), batch, channel, &ch_per_group);
        if (groups && K::k1_fits(h, w)) {
            K::k1(second, act, dim3((w + 63) / 64, (h + 3) / 4, batch * groups), st, other, gout, gin, channel, h, w, groups, ch_per_group);
            return launch_status();
        }
    }
    const int64_t total = (int64_t)batch * channel * h * w;
    if ((total + 255) / 256 > INT_MAX) return VFI_ERR_SHAPE;
    K::generic(second, act, dim3((unsigned)((total + 255) / 256)), st, other, gout, gin, batch, channel, h, w, oc, oh, ow, pad_size,
               (kernel_size - 1) / 2, max_displacement, stride2, max_displacement / stride2);
    return launch_status();
}

// both gradients: gradInput1 from (input2, gradOutput), then gradInput2 from (input1, gradOutput)
template <class K>
inline int corr_backward_both(const void* input1, const void* input2, const void* gradoutput, void* gradinput1, void* gradinput2,
                              int batch, int channel, int h, int w, int pad_size, int kernel_size, int max_displacement, int stride1,
                              int stride2, vfi_stream_t stream, const typename K::Mask* act = nullptr) {
    typedef typename K::T T;
    int oc, oh, ow;
    if (corr_check({input1, input2, gradoutput, gradinput1, gradinput2}, batch, channel, h, w, pad_size, kernel_size, max_displacement,
                   stride1, stride2, true, &oc, &oh, &ow))
        return VFI_ERR_SHAPE;
    if constexpr (K::MASKED)
        if (act && !corr_grad_ok(*act, (int64_t)oc * oh * ow)) return VFI_ERR_SHAPE;
    const int err = corr_backward_one<K>(false, (const T*)input2, (const T*)gradoutput, (T*)gradinput1, batch, channel, h, w, oc, oh, ow,
                                         pad_size, kernel_size, max_displacement, stride2, (hipStream_t)stream, act);
    if (err != VFI_OK) return err;
    return corr_backward_one<K>(true, (const T*)input1, (const T*)gradoutput, (T*)gradinput2, batch, channel, h, w, oc, oh, ow, pad_size,
                                kernel_size, max_displacement, stride2, (hipStream_t)stream, act);
}

// The tensors of a paired backward entry: two calls of equal shape, item a and item b, each with its two gradients (NULL:
// not requested), from the entry's _a / _b arguments.
template <class E>
struct CorrBwdItems { const E* in1[2]; const E* in2[2]; const E* go[2]; E* gi[2][2]; };
template <class E>
inline CorrBwdItems<E> corr_backward_items(const void* input1_a, const void* input2_a, const void* gradoutput_a, void* gradinput1_a,
                                           void* gradinput2_a, const void* input1_b, const void* input2_b, const void* gradoutput_b,
                                           void* gradinput1_b, void* gradinput2_b) {
    return {{(const E*)input1_a, (const E*)input1_b}, {(const E*)input2_a, (const E*)input2_b},
            {(const E*)gradoutput_a, (const E*)gradoutput_b}, {{(E*)gradinput1_a, (E*)gradinput2_a}, {(E*)gradinput1_b, (E*)gradinput2_b}}};
}

// The host's compaction: the requested gradients of the two items become roles 0 .. n - 1, each with its item's mask
// (`acts`, or NULL for the unmasked entries).  An item with nothing requested is skipped and may be all NULL.  Returns n, or
// -1 for what the entries refuse: a requested gradient whose item lacks an input, its gradOutput or its y, a mask stride
// below `image` elements, two equal outputs.
template <class E, class Mask>
inline int corr_backward_roles(const CorrBwdItems<E>& t, const Mask* acts, int64_t image, CorrBwdRolesT<E>& roles, CorrBwdMasksT<E>& masks) {
    int nroles = 0;
    for (int i = 0; i < 2; ++i) {
        if (!t.gi[i][0] && !t.gi[i][1]) continue;           // (nothing asked of this item: its inputs may be NULL)
        if (!t.in1[i] || !t.in2[i] || !t.go[i]) return -1;
        if (acts && (!acts[i].y || acts[i].ystride < image || acts[i].gstride < image)) return -1;
        for (int s = 0; s < 2; ++s) {
            if (!t.gi[i][s]) continue;
            for (int k = 0; k < nroles; ++k)
                if (roles.r[k].gin == t.gi[i][s]) return -1;
            if (acts) { masks.y[nroles] = acts[i].y; masks.ystride[nroles] = acts[i].ystride; masks.gstride[nroles] = acts[i].gstride; }
            roles.r[nroles++] = {s ? t.in1[i] : t.in2[i], t.go[i], t.gi[i][s], s};      // gradInput1 reads input2, gradInput2 input1
        }
    }
    if (acts) masks.slope = acts[0].slope;                  // (both items carry the one slope)
    return nroles;
}

// The backward of two calls of equal shape -- the same pyramid level of the two flow networks of a frame pair, whose forward
// is the paired forward entry -- with any subset of the four gradients.  PWC-Net's configuration: the requested gradients
// are the roles of ONE launch of the pair kernel, and the channel groups are sized on the whole launch (tiles x batch x
// roles).  Any other configuration, or roles x batch x groups beyond a grid's z: one launch per requested gradient with the
// kernels the single entry uses.  Either way a gradient's bits are that entry's.  `acts` (or NULL): the two items' masks --
// the same compaction and launches with the masked kernels; a role carries its item's mask.
template <class K>
inline int corr_backward_pair(const CorrBwdItems<typename K::T>& t, const typename K::Mask* acts, int batch, int channel, int h, int w,
                              int pad_size, int kernel_size, int max_displacement, int stride1, int stride2, vfi_stream_t stream) {
    typedef typename K::T T;
    static_assert(K::PAIRED, "the file has no pair kernels");
    int oc, oh, ow;
    if (corr_check({}, batch, channel, h, w, pad_size, kernel_size, max_displacement, stride1, stride2, true, &oc, &oh, &ow))
        return VFI_ERR_SHAPE;
    if (acts && !corr_slope_ok(acts[0].slope)) return VFI_ERR_SHAPE;
    CorrBwdRolesT<T> roles = {};
    CorrBwdMasksT<T> masks = {};
    const int nroles = corr_backward_roles(t, acts, (int64_t)oc * oh * ow, roles, masks);
    if (nroles < 0) return VFI_ERR_SHAPE;
    if (nroles == 0) return VFI_OK;
    hipStream_t st = (hipStream_t)stream;
    if (kernel_size == 1 && stride2 == 1 && max_displacement == 4 && pad_size == 4 && batch <= 65535) {
        int ch_per_group;
        const int groups = corr_backward_groups(((w + 63) / 64) * ((h + 3) / 4), batch * nroles, channel, &ch_per_group);
        if (groups && K::k1_fits(h, w)) {
            roles.per_role = batch * groups;
            K::pair(roles, acts ? &masks : nullptr, dim3((w + 63) / 64, (h + 3) / 4, nroles * roles.per_role), st, channel, h, w, groups,
                    ch_per_group);
            return launch_status();
        }
    }
    for (int k = 0; k < nroles; ++k) {
        const CorrBwdRoleT<T>& r = roles.r[k];
        const typename K::Mask act = {masks.y[k], masks.ystride[k], masks.gstride[k], masks.slope};
        const int err = corr_backward_one<K>(r.second != 0, r.other, r.gout, r.gin, batch, channel, h, w, oc, oh, ow, pad_size, kernel_size,
                                             max_displacement, stride2, st, acts ? &act : nullptr);
        if (err != VFI_OK) return err;
    }
    return VFI_OK;
}

}  // namespace vfi
