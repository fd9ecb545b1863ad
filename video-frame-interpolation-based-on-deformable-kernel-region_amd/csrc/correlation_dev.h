// correlation_dev.h -- the pieces the correlation kernels share (correlation.hip, warp_correlation.hip): which image of a
// launch a workgroup works on, the staging plan in aligned units, the 32x4 tile with two pixels per lane, the mean of the
// running sums, and the tile and the roles of the tiled backward kernels.  Internal to the library.
#pragma once
#include "vfi_common.h"

#include <initializer_list>

namespace vfi {

#define CORR_CC_ROWS 8   // channels staged per LDS fill by the wave-per-displacement-row kernels (16 measured the same: their chunk loop is LDS-bound, one workgroup per CU)

// The tensors of a launch: one call, or two calls of equal shape in one launch (both flow directions of a pyramid level: at
// the coarse levels a launch is latency, 13-18 us for 1 MB, and two cost what one does).  Images 0 .. per - 1 are item 0's.
struct CorrItems { const float* in1[2]; const float* in2[2]; float* out[2]; int per; };

// Image `img` of a launch: the item it belongs to and its index `b` inside that item.  A kernel indexes its own `items`
// argument with `item` and binds the three pointers to __restrict__ locals: handing `items` to a helper takes the
// argument's address, and the compiler then loads all six pointers and selects, instead of the three at `item`.
struct CorrImage { int item, b; };
__device__ __forceinline__ CorrImage corr_image(int img, int per) {
    const int item = img >= per ? 1 : 0;                    // (two calls in one launch: vfi_correlation_forward_pair)
    return {item, img - item * per};
}

// Staging plan in aligned units of four elements of EB bytes: unit e = tid + k * NT of a chunk's [CC][ROWS][UW] block whose
// rows start at frame position (y0, x0), x0 and w multiples of 4 (so a unit lies wholly inside or wholly outside the frame),
// as a byte offset from the chunk's first plane.  The loads are buffer loads through a descriptor that spans exactly the
// chunk's planes: a unit outside the frame gets an offset out of any range, a channel past the last one falls out of the
// descriptor's, and both arrive as zeros.
template <unsigned EB, int CC, int ROWS, int UW, int NT, int N>
__device__ __forceinline__ void corr_unit_plan(unsigned (&off)[N], int tid, int y0, int x0, int h, int w, int plane) {
    static_assert(N == (CC * ROWS * UW + NT - 1) / NT, "units per thread");
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int e = tid + k * NT;
        const int c = e / (ROWS * UW), rem = e - c * (ROWS * UW);
        const int r = rem / UW, col = 4 * (rem - r * UW);
        const int gy = y0 + r, gx = x0 + col;
        const bool ok = e < CC * ROWS * UW && gy >= 0 && gy < h && gx >= 0 && gx < w;
        off[k] = ok ? EB * (unsigned)(c * plane + gy * w + gx) : 0x80000000u;
    }
}

// The 32x4 tile of output pixels with one wave per displacement row (threadIdx.y = tj) and TWO horizontally adjacent pixels
// per lane: per channel a lane reads the D + 1 window values its two D-wide displacement rows share as (D + 1) / 2 aligned
// pairs.
template <int MD_>
struct CorrTile2 {
    static constexpr int MD = MD_, D = 2 * MD + 1, TW = 32, TH = 4, LW = TW + 2 * MD, LH = TH + 2 * MD, NT = 64 * D, CC = CORR_CC_ROWS;
    static constexpr int UW = LW / 4, NU = CC * LH * UW, NPT = (NU + NT - 1) / NT;    // window units of four elements per chunk, per thread
    static constexpr int FU = CC * TH * (TW / 4), NF1 = (FU + NT - 1) / NT;           // ... of the first map
    static constexpr int PAIRS = (D + 1) / 2;
    static __device__ __forceinline__ int px(int lane) { return 2 * (lane & 15); }
    static __device__ __forceinline__ int py(int lane) { return lane >> 4; }
    // the pairs at window row `row` from column px on (P: float2-like or __half2)
    template <class P, class E>
    static __device__ __forceinline__ void read_row(const E* row, P (&r)[PAIRS]) {
#pragma unroll
        for (int k = 0; k < PAIRS; ++k) r[k] = reinterpret_cast<const P*>(row)[k];
    }
};

// The mean of the running sums, handed to `store` as a function of one sum: a product with the exact reciprocal for a
// power-of-two channel count (the same real number), a division otherwise.
template <class Store>
__device__ __forceinline__ void corr_store_mean(int channel, Store&& store) {
    const float nelems = (float)channel;
    const float inv = 1.0f / nelems;
    if ((channel & (channel - 1)) == 0) store([&](float v) { return v * inv; });
    else store([&](float v) { return v / nelems; });
}

// What a float forward kernel does with a mean as it stores it, and where plane k of image b begins in the output: a
// compile-time choice, so the plain instances are the kernels they were.  CorrPlain: the mean as it is, dense images.
// CorrLrelu: PWC-Net's LeakyReLU on the mean, y = v > 0 ? v : v * slope -- ONE multiplication of the value the plain kernel
// stores (NaN stays NaN, -0 becomes -0 * slope: torch's leaky_relu in float) -- into an output whose images lie
// stride[item] elements apart while the planes of an image stay contiguous (the first channels of a concatenation buffer).
struct CorrPlain {
    static constexpr bool DENSE = true;
    __device__ __forceinline__ float operator()(float v) const { return v; }
    __device__ __forceinline__ int64_t plane(int, int b, int oc, int k, int oh, int ow) const { return ((int64_t)b * oc + k) * oh * ow; }
};
struct CorrLrelu {
    static constexpr bool DENSE = false;
    int64_t stride[2];
    float slope;
    __device__ __forceinline__ float operator()(float v) const { return v > 0.0f ? v : v * slope; }
    __device__ __forceinline__ int64_t plane(int item, int b, int, int k, int oh, int ow) const {
        return (int64_t)b * stride[item] + (int64_t)k * oh * ow;
    }
};

// What a float backward kernel does with a gradOutput value as it loads it, for one gradient (workgroup-uniform scalars).
// MASK == false: nothing, dense gradOutput.  MASK == true: LeakyReLU's derivative through the saved ACTIVATED output y (its
// sign is the pre-activation's for any slope > 0): g' = y > 0 ? g : g * slope, rounded to float before the term that uses
// it, so the gradient is the plain kernel's fed g'.  Images of y and of gradOutput lie ystride / gstride elements apart,
// the planes of an image contiguous (gradOutput: the narrow() view that torch.cat's backward hands down).
template <bool MASK_>
struct CorrGrad {
    static constexpr bool MASK = MASK_;
    const float* y;
    int64_t ystride, gstride;
    float slope;
    // value g whose output position holds yv
    __device__ __forceinline__ float operator()(float g, float yv) const {
        if constexpr (MASK_) return yv > 0.0f ? g : g * slope;      // (a skipped term: 0 * slope = +0, slope finite and positive)
        else return g;
    }
};
// the masks of a vfi_correlation_lrelu_backward_pair launch, by role (CorrBwdRoles); E: the storage type (float, or the
// bfloat16 bits of vfi_correlation_lrelu_backward_pair_bf16)
template <class E>
struct CorrBwdMasksT { const E* y[4]; int64_t ystride[4], gstride[4]; float slope; };
typedef CorrBwdMasksT<float> CorrBwdMasks;

// The gradients of one vfi_correlation_backward_pair launch: a role is one requested gradient of one item -- the map its
// window is staged from, the item's gradOutput, where it goes, and which of the two gradients it is.  The host compacts the
// requested ones (at most four) to the front; role i owns blockIdx.z in [i * per_role, (i + 1) * per_role).
template <class E>
struct CorrBwdRoleT { const E* other; const E* gout; E* gin; int second; };
template <class E>
struct CorrBwdRolesT { CorrBwdRoleT<E> r[4]; int per_role; };
typedef CorrBwdRolesT<float> CorrBwdRoles;

// The host's compaction, for either storage type: the requested gradients of the two items become roles 0 .. n - 1, each
// with its item's mask (`acts`, or NULL for the unmasked entries: two structs with y, ystride, gstride and slope).  An item
// with nothing requested is skipped and may be all NULL.  Returns n, or -1 for what the entries refuse: a requested
// gradient whose item lacks an input, its gradOutput or its y, a mask stride below `image` elements, two equal outputs.
template <class E, class Act>
inline int corr_backward_roles(const E* const (&in1)[2], const E* const (&in2)[2], const E* const (&go)[2], E* const (&gi)[2][2],
                               const Act* acts, int64_t image, CorrBwdRolesT<E>& roles, CorrBwdMasksT<E>& masks) {
    int nroles = 0;
    for (int i = 0; i < 2; ++i) {
        if (!gi[i][0] && !gi[i][1]) continue;               // (nothing asked of this item: its inputs may be NULL)
        if (!in1[i] || !in2[i] || !go[i]) return -1;
        if (acts && (!acts[i].y || acts[i].ystride < image || acts[i].gstride < image)) return -1;
        for (int s = 0; s < 2; ++s) {
            if (!gi[i][s]) continue;
            for (int k = 0; k < nroles; ++k)
                if (roles.r[k].gin == gi[i][s]) return -1;
            if (acts) { masks.y[nroles] = acts[i].y; masks.ystride[nroles] = acts[i].ystride; masks.gstride[nroles] = acts[i].gstride; }
            roles.r[nroles++] = {s ? in1[i] : in2[i], go[i], gi[i][s], s};      // gradInput1 reads input2, gradInput2 input1
        }
    }
    if (acts) masks.slope = acts[0].slope;
    return nroles;
}

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

// Host side, defined in correlation.hip and shared with correlation_bf16.hip: the checks every entry makes before it
// launches, and the tiled backward kernels' split of the channels into groups.
int corr_check(std::initializer_list<const void*> tensors, int batch, int channel, int h, int w, int pad_size, int kernel_size,
               int max_displacement, int stride1, int stride2, bool backward, int* oc, int* oh, int* ow);
int corr_backward_groups(int tiles, int batch, int channel, int* ch_per_group);

}  // namespace vfi
