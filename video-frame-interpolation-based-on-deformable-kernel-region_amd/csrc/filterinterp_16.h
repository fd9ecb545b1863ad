// filterinterp_16.h -- what the two LDS-staged FilterInterpolation kernels on 16-bit STORAGE share, fs == 4:
// fi_forward_ori_lds_f16 (filterinterp_f16.hip) and fi_forward_ori_lds_bf16 (filterinterp_bf16.hip), and the direct kernel of
// both.  The tiling, LDS-DMA ring and channel loop are those of fi_forward_ori_lds (filterinterp_lds.hip) with half the bytes
// everywhere: a staged window element is one dword = two pixels, a tap row is three dword LDS reads (instead of four) shifted
// into place by v_alignbit with a per-lane amount.  Image columns are never replicated in LDS (a dword holds two pixels, so
// per-pixel clamping of a dword load is impossible): a window that crosses the left or right border is moved inside the image
// (Lc), and each format makes up for the move in its own arithmetic.
// Nothing in here knows a number format: what a pixel does with its eight packed tap dwords, and how the 16-bit result is
// formed, is the unit's VALUE callable (its storage S for the direct kernel).
#pragma once
#ifdef FI_PITCH_SKEW
#error "filterinterp_16.h sets FI_PITCH_SKEW: include it before anything that includes filterinterp_dev.h"
#endif
#define FI_PITCH_SKEW 16                            // (dwords; see fi_pitch_for)
#include "filterinterp_dev.h"
#include "filterinterp_paths.h"

#include <limits.h>

namespace vfi {

#define FI16_TW 64
#define FI16_TH 16
#define FI16_PX 2
#define FI16_THREADS (FI16_TW * FI16_TH / FI16_PX)
#define FI16_PASS_ROWS (FI16_TH / FI16_PX)
#define FI16_HDR 16
#define FI16_RING_DWORDS 15984
#define FI16_RMAX 5
#define FI16_KTOP 8

// ------------------------------------------------------------------ direct kernel (reference order)

// One thread per pixel, any filter size, any strides, 2-byte alignment: the fallback of the staged kernel and its yardstick.
// S, a unit's storage policy:
//   E                 the element
//   widen(E)          -> float, exactly
//   store(float)      -> E, rounding once to nearest even
//   PRODUCT_FIRST     an fs == 4 quadrant chain starts with a plain product (as fi4_pixel); else with fmaf(v, f, 0), like
//                     every other size.  The two differ in the sign of a zero product.
//   POINT_THEN_CELL   which spelling of the validity step the instance keeps (below).  No behaviour hangs on it: both
//                     spellings give the same values, and the flag is there only so that each instance compiles to the code
//                     it was.  (The flow read is not the cause: both instances read it through fi_flow_at.)
// `DST... so`: the destination's own layout (fi_dst), or none.
template <typename S, typename... DST>
__global__ __launch_bounds__(VFI_TX * VFI_TY) void fi_forward_ori_direct_16(
    const typename S::E* __restrict__ in1, const float* __restrict__ in2, const float* __restrict__ in3,
    typename S::E* __restrict__ out, int channel, int h, int w, int fs,
    vfi_strides s1, vfi_strides s2, vfi_strides s3, DST... so) {
    typedef typename S::E E;
    constexpr bool TO = sizeof...(DST) != 0;
    const int x = blockIdx.x * VFI_TX + threadIdx.x;
    const int y = blockIdx.y * VFI_TY + threadIdx.y;
    if (x >= w || y >= h) return;
    const int b = blockIdx.z;
    const FiFlow fl = fi_flow_at(in2, s2, b, x, y);
    const E* img = in1 + (int64_t)b * s1.b;
    E* dst = out + (int64_t)b * fi_dst(s1, so...).b + (int64_t)y * fi_dst(s1, so...).h + x;
    // POINT_THEN_CELL: the validity test on the point, the cell after it (fi_geom before the test changes that instance's
    // code, and this spelling the other's)
    FiGeom g;
    if constexpr (S::POINT_THEN_CELL) g.valid = fi_valid(fl.fx, fl.fy, (float)x + fl.fx, (float)y + fl.fy, w, h);
    else g = fi_geom(fl.fx, fl.fy, x, y, w, h);
    if (!g.valid) {
        fi_copy_through_to<TO>(img + (int64_t)y * s1.h + x, dst, 0, channel, s1.c, fi_dst(s1, so...).c);
        return;
    }
    if constexpr (S::POINT_THEN_CELL) g = fi_cell(FiPoint{true, (float)x + fl.fx, (float)y + fl.fy});
    const int ix = g.ix, iy = g.iy;
    const int L = ix + 1 - fs / 2, T = iy + 1 - fs / 2;
    const int R = L + fs, Bm = T + fs;
    const float* fpx = in3 + (int64_t)b * s3.b + (int64_t)y * s3.h + x;
    for (int c = 0; c < channel; ++c) {
        const E* plane = img + (int64_t)c * s1.c;
        float q[4];
        // quadrant by quadrant, rows outer / columns inner (:2749-2787)
        for (int quad = 0; quad < 4; ++quad) {
            const int j0 = (quad & 2) ? iy + 1 : T, j1 = (quad & 2) ? Bm : iy + 1;
            const int i0 = (quad & 1) ? ix + 1 : L, i1 = (quad & 1) ? R : ix + 1;
            float acc = 0.0f;
            bool product = S::PRODUCT_FIRST && fs == 4;
            for (int j = j0; j < j1; ++j) {
                const E* row = plane + (int64_t)clampi(j, 0, h - 1) * s1.h;
                for (int i = i0; i < i1; ++i) {
                    const float v = S::widen(row[clampi(i, 0, w - 1)]);
                    const float f = fpx[(int64_t)((j - T) * fs + (i - L)) * s3.c];
                    acc = product ? v * f : fmaf(v, f, acc);
                    product = false;
                }
            }
            q[quad] = acc;
        }
        dst[(int64_t)c * fi_dst(s1, so...).c] = S::store(blend4(g.alpha, g.beta, q[0], q[1], q[2], q[3]));
    }
}

// ------------------------------------------------------------------ LDS-staged kernels: the tile prologue

// The workgroup's tile (four horizontally consecutive tiles per XCD, fi_xcd_tile; the test against ntiles stays in the kernel,
// in a helper it changes the kernels' code) and this thread's place in it: column x, and rows y0 + p * FI16_PASS_ROWS for its
// FI16_PX pixels.
struct Fi16Tile { int b, c_begin, c_end, x, y0; };
__device__ __forceinline__ Fi16Tile fi16_tile(int tile, int tid, int tiles_x, int tiles_y, int channel, int ch_per_group) {
    const FiTile tp = fi_tile_at(tile, tiles_x, tiles_y, channel, ch_per_group);
    return Fi16Tile{tp.b, tp.c_begin, tp.c_end, tp.tx * FI16_TW + (tid & (FI16_TW - 1)), tp.ty * FI16_TH + (tid >> 6)};
}

// One pixel's window from its flow: L, T the corner, Lc the first column after the move inside the image (an invalid pixel's
// window: L = 0); a valid pixel's moved window is added to the thread's own box.  (The loop over the thread's pixels, inimg,
// pix and the flow read stay in the kernels: in a helper they add an address computation to fi_forward_ori_lds_bf16.)
struct Fi16Box { int bx_lo = INT_MAX, by_lo = INT_MAX, bx_hi = INT_MIN, by_hi = INT_MIN; };
struct Fi16Tap { bool valid; int L, Lc, T; float alpha, beta; };
__device__ __forceinline__ Fi16Tap fi16_tap(float fx, float fy, int x, int y, int w, int h, bool inimg, Fi16Box& box) {
    const FiGeom g = fi_geom(fx, fy, x, y, w, h, inimg, 1);
    Fi16Tap t;
    t.valid = g.valid;
    t.L = g.ix - 1; t.T = g.iy - 1;
    t.Lc = clampi(t.L, 0, w - 4);                           // the window moved inside the image (w >= 4)
    t.alpha = g.alpha; t.beta = g.beta;
    fi_box_add4(g.valid, t.Lc, t.T, box.bx_lo, box.by_lo, box.bx_hi, box.by_hi);
    return t;
}

// The tile's staged window (of an h x w plane with row stride hs) from the threads' boxes, after
//     if (tid == 0) fi_box_clear(box);
//     __syncthreads();
// in the kernel (fi_box_fold): bx0 even; bw, pitch in dwords.  (kmax, the staged dwords per thread, is formed where the
// kernel dispatches on it: formed in here it changes fi_forward_ori_lds_bf16's code.)
__device__ __forceinline__ FiWindow fi16_window(int* box, int tid, const Fi16Box& own, int h, int w, int hs) {
    const bool any_valid = fi_box_fold(box, tid, own.bx_lo, own.by_lo, own.bx_hi, own.by_hi);
    const int bx0 = any_valid ? box[0] & ~1 : 0, by0 = box[1];          // even: dword-aligned rows
    const int bw = any_valid ? (box[2] - bx0 + 2) >> 1 : 0;              // dwords per row
    const int bh = any_valid ? box[3] - by0 + 1 : 0;
    const int pitch = fi_pitch_for(bw);
    return FiWindow{bx0, by0, bw, bh, pitch, h, w, hs};
}
// element index of a valid pixel's moved window (first column Lc, first row T) inside the staged window (row pitch 2 * pitch)
__device__ __forceinline__ int fi16_lbase(bool valid, int Lc, int T, const FiWindow& win) {
    return valid ? (T - win.by0) * (2 * win.pitch) + (Lc - win.bx0) : 0;
}

// ------------------------------------------------------------------ LDS-staged kernels: the channel loop

// Channel loop of one workgroup, written like fi_run_channels_lean (filterinterp_lds.hip: what bounds this loop is the
// instruction count): ring geometry a compile-time function of K and one constant s_waitcnt in the steady state, running
// plane descriptors, M0 formed on the scalar unit, tap reads as asm with two lgkmcnt waits per channel and the second
// pixel's first rows in flight under the first pixel's arithmetic, range-checked buffer stores.
//   K      staged dwords per thread (the rung)
//   TO     the destination's planes are cso_to apart (else cso_to is not looked at: FI_CSO, filterinterp_dev.h)
//   E      the 16-bit storage element
//   PX     the unit's pixel state; read here: valid, inimg, lbase (element index of the moved window's origin inside a
//          staged window of row pitch 2 * pitch), pix
//   VALUE  value(p, row) -> the 16 bits to store for pixel p; row(r, e0, e1) hands out the moved window's four columns of tap
//          row r as two packed pairs.  (The rows are fetched by the callable, one at a time where it uses them: handed over
//          as two arrays formed up front, the same instructions come out in another order and the fp16 kernel is slower.)
template <int K, bool TO, typename E, typename PX, typename VALUE>
__device__ __forceinline__ void fi16_run_channels(const E* __restrict__ img, E* __restrict__ out, int64_t cs, int64_t cso_to,
                                                  int c_begin, int c_end, int tid, const FiWindow& win,
                                                  const PX (&px)[FI16_PX], unsigned* __restrict__ ring, VALUE&& value) {
    typedef unsigned v2u __attribute__((ext_vector_type(2)));
    static_assert(sizeof(E) == 2, "16-bit storage");
    static_assert(FI16_PX == 2, "two pixels per thread");
    constexpr int NP = K * FI16_THREADS;                    // dwords per ring slot
    constexpr int R = (FI16_RING_DWORDS / NP) < FI16_RMAX ? (FI16_RING_DWORDS / NP) : FI16_RMAX;
    constexpr int D = R - 1;
    static_assert(D >= 1 && (D - 1) * K <= 63, "ring geometry");
    static_assert(R * NP <= FI16_RING_DWORDS, "the ring's slots fit the LDS array");
    if (c_begin >= c_end) return;
    // dword e = tid + k*FI16_THREADS of the staged window, row-major, `pitch` dwords per row; rows clamped to the image,
    // columns never out of it; pad dwords get an out-of-range offset (the load returns 0 without touching memory)
    const float inv_pitch32 = 1.0f / (float)win.pitch;
    unsigned goff[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = tid + k * FI16_THREADS;
        const int r = fi_row_of(e, inv_pitch32);
        const int col = e - r * win.pitch;
        const unsigned off = 2u * (unsigned)(clampi(win.by0 + r, 0, win.h - 1) * win.hs + win.bx0 + 2 * col);
        goff[k] = (col < win.bw && r < win.bh) ? off : 0x80000000u;
    }
    const int plane_bytes = (2 * ((win.h - 1) * win.hs + win.w) + 3) & ~3;
    const int wave_first = __builtin_amdgcn_readfirstlane(tid >> 6) * 64;
    const unsigned ring_lds = (unsigned)(uintptr_t)(lds_ptr_t)ring;
    const unsigned pitch4 = 4u * (unsigned)win.pitch;
    unsigned lb[FI16_PX], sh[FI16_PX], soff[FI16_PX];
#pragma unroll
    for (int p = 0; p < FI16_PX; ++p) {
        lb[p] = ring_lds + 4u * (unsigned)(px[p].lbase >> 1);
        sh[p] = (unsigned)(px[p].lbase & 1) * 16u;
        soff[p] = px[p].valid ? 2u * px[p].pix : 0x80000000u;   // (an invalid pixel's store is dropped by the range check)
    }
    const int last = c_end - 1;
    const E* pdma = img + (int64_t)c_begin * cs;
    E* pout = out + (int64_t)c_begin * FI_CSO;
    auto issue = [&](int slot) {
        const auto plane = buffer_rsrc(pdma, plane_bytes);
        unsigned* l = ring + slot * NP + wave_first;
#pragma unroll
        for (int k = 0; k < K; ++k)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(plane, (lds_ptr_t)(l + k * FI16_THREADS), 4, goff[k], 0, 0, 0);
        pdma += cs;
    };
#define FI16_READ2(dst, addr) asm volatile("ds_read2_b32 %0, %1 offset0:0 offset1:1" : "=v"(dst) : "v"(addr))
#define FI16_READ1(dst, addr) asm volatile("ds_read_b32 %0, %1 offset:8" : "=v"(dst) : "v"(addr))
    // The pipeline is skewed by one pixel across the barrier (filterinterp_lds.hip): in channel c a wave issues pixel 0's
    // reads, does the arithmetic of pixel 1 of channel c - 1 (taps read before the barrier, waiting in registers), issues
    // pixel 1's reads, does pixel 0, and waits for pixel 1's taps -- every LDS read is in flight under the wave's own arithmetic.
    v2u a01[2][4];          // dwords 0, 1 of the four tap rows, two pixels
    unsigned a2[2][4];      // dword 2
    auto reads = [&](int p, unsigned so) {
        unsigned a = lb[p] + so;
#pragma unroll
        for (int r = 0; r < 4; ++r) { FI16_READ2(a01[p][r], a); FI16_READ1(a2[p][r], a); a += pitch4; }
    };
    auto pixel = [&](int p, const E* plane_ptr) {
        // ({d1,d0} >> sh) and ({d2,d1} >> sh): the moved window's four columns of tap row r as two packed pairs
        auto row = [&](int r, unsigned& e0, unsigned& e1) {
            e0 = __builtin_amdgcn_alignbit(a01[p][r].y, a01[p][r].x, sh[p]);
            e1 = __builtin_amdgcn_alignbit(a2[p][r], a01[p][r].y, sh[p]);
        };
        const unsigned short bits = value(p, row);
        const auto oplane = buffer_rsrc(plane_ptr, plane_bytes);
        __builtin_amdgcn_raw_buffer_store_b16(bits, oplane, soff[p], 0, 0);
    };
    auto compute = [&](int slot, bool first) {
        const unsigned so = (unsigned)(slot * (NP * 4));
        reads(0, so);
        if (!first) pixel(1, pout - FI_CSO);                // pixel 1 of the previous channel
        asm volatile("s_waitcnt lgkmcnt(7)" ::: "memory");  // (at most 15 LDS reads outstanding)
        reads(1, so);
        asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(a01[0][0]), "+v"(a01[0][1]), "+v"(a01[0][2]), "+v"(a01[0][3]),
                                               "+v"(a2[0][0]), "+v"(a2[0][1]), "+v"(a2[0][2]), "+v"(a2[0][3]));
        pixel(0, pout);
        // pixel 1's taps are in registers before the barrier: the slot may be overwritten after it
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a01[1][0]), "+v"(a01[1][1]), "+v"(a01[1][2]), "+v"(a01[1][3]),
                                               "+v"(a2[1][0]), "+v"(a2[1][1]), "+v"(a2[1][2]), "+v"(a2[1][3]));
        pout += FI_CSO;
    };
#undef FI16_READ2
#undef FI16_READ1
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
    pixel(1, pout - FI_CSO);                                    // pixel 1 of the last channel
#pragma unroll
    for (int p = 0; p < FI16_PX; ++p)
        if (px[p].inimg && !px[p].valid) fi_copy_through_to<TO>(img, out, px[p].pix, c_begin, c_end, cs, cso_to);
}

// The rung ladder on kmax, the staged dwords per thread, at most FI16_KTOP (a window too large for the ring is gathered from
// global memory by the kernel itself, in its own arithmetic): RUN(K) with K a literal.  (A macro: as a function template
// taking a callable it changes fi_forward_ori_lds_bf16's code.)
#define FI16_LADDER(RUN)        \
    if (kmax <= 2) RUN(2);      \
    else if (kmax == 3) RUN(3); \
    else if (kmax == 4) RUN(4); \
    else if (kmax <= 6) RUN(6); \
    else RUN(8)

// ------------------------------------------------------------------ the launch plan (host)

// staged: the image's layout allows dword staging and the tile count fits; then the grid: fi_xcd_grid(ntiles) x split.groups
// workgroups of FI16_THREADS.  Else the caller launches the direct kernel.
struct Fi16Plan {
    bool staged;
    int tiles_x, tiles_y, ntiles;
    FiSplit split;
};
inline Fi16Plan fi16_launch_plan(const void* input1, vfi_strides s1, int h, int w, int batch, int channel, int filter_channels) {
    Fi16Plan plan{};
    // the staged kernel moves dwords: rows, planes and the base address must be 4-byte aligned
    const bool staged = filter_channels == 16 && w >= 4 &&
                        ((s1.h | s1.c | s1.b) & 1) == 0 && (reinterpret_cast<uintptr_t>(input1) & 3) == 0 &&
                        (int64_t)h * s1.h * 2 < INT_MAX;
    plan.tiles_x = (w + FI16_TW - 1) / FI16_TW;
    plan.tiles_y = (h + FI16_TH - 1) / FI16_TH;
    const int64_t nt = (int64_t)plan.tiles_x * plan.tiles_y * batch;
    if (!staged || nt > (1 << 28)) return plan;
    const int ntiles = (int)nt;
    // split the channel range over blockIdx.y when that shortens the tail (as the fp32 kernel)
    const FiSplit split = fi_channel_split(ntiles, channel, 4.3);
    plan.staged = true;
    plan.ntiles = ntiles;
    plan.split = split;
    return plan;
}

}  // namespace vfi
