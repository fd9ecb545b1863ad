// filterinterp_nhwc_bwd.hip -- the image gradient of FilterInterpolation `_ori`, summed over several flows, for channels_last
// (NHWC) gradients and a channels_last result: the backward of the context warp of filterinterp_nhwc.hip, float32 or bfloat16
// storage, without the layout copies around vfi_filterinterp_backward_ori_image_multi[_bf16].
//
// Contract: every element of gradinput1 is, bit for bit, what that NCHW entry writes for the same logical tensors.  The
// accumulator is gradacc.h's: every addend is rounded to an integer at ONE scale per call and added with integer atomics, so
// the sums do not depend on the order or on the layout.  Each addend is formed as filterinterp_ctx_bwd.h forms it --
// qg[quad] * fv[k] with qg = g (1 - alpha) (1 - beta) and so on, then the call's power of two, then __float2ll_rn -- and the
// scale is the one the NCHW call derives: the largest |gradient| over all flows, the largest |filter tap|, cells_log2 from
// h w max(filter_channels, 4) nflows.  The 64-bit scratch is dense [b][y][x][c], so a tile's flush and the conversion run
// along channels; the scans, the zero fill and the conversion are gradacc's own kernels on the tensor re-read as rows of
// stride-1 elements (fnb_rows).
//
//   fi_nhwc_backward4_lds<E, V>   fs == 4, filter_channels == 16, integer path, one scale factor.  A workgroup owns a tile of
//                                 FNB_TW x FNB_TH pixels.  What depends on the pixel alone -- per flow the validity, alpha /
//                                 beta and the window's LDS cell offsets, and the 16 filter taps -- is formed once per tile
//                                 and kept in LDS.  The union bounding box of the clamped taps of all the launch's flows is
//                                 the tile's window: 64-bit LDS cells [cell][FNB_SLAB channels].  Per pass one slab of
//                                 channels is summed with LDS atomics (an item is one pixel, one flow and V channels read
//                                 with one load), then every non-zero cell leaves with one global 64-bit atomic; a cell's
//                                 slab is FNB_SLAB x 8 = 128 contiguous bytes of the scratch.  Where the union window does
//                                 not fit, the tile's flows go one after the other, each on its own window; a flow whose
//                                 own window does not fit, and every flow of a call on the fp32 path or with a second scale
//                                 factor, is flagged (one bit per flow in the tile's flag word) for the kernel below.
//   fi_nhwc_backward_any<E>       any filter size, lanes along channels, every addend through gradacc_add (the integer sums,
//                                 or the fp32 atomics of a call with non-finite inputs): the flagged tiles after the staged
//                                 kernel, or all of them.
// Flows and filter are float32 with four strides each, as in the forward unit.
#include "bf16.h"
#include "filterinterp_dev.h"
#include "gradacc.h"

namespace vfi {

#define FNB_TW 32
#define FNB_TH 4
#define FNB_PIXELS (FNB_TW * FNB_TH)
#define FNB_THREADS 256
// channels summed per pass: a cell's slab is FNB_SLAB x 8 = 128 contiguous bytes of the scratch
#define FNB_SLAB 16
// 64-bit LDS cells of the window (57,344 bytes): a window of n cells is staged when n * FNB_SLAB <= FNB_CELLS
#define FNB_CELLS 7168
// flows one launch carries
#define FNB_NT 3
static_assert(FNB_THREADS % 64 == 0 && FNB_THREADS >= FNB_PIXELS && 2 * FNB_THREADS >= FNB_NT * FNB_PIXELS, "prologue mapping");
static_assert((FNB_SLAB & (FNB_SLAB - 1)) == 0 && FNB_SLAB >= 16, "a slab spans at least 128 bytes of the scratch");
static_assert(FNB_CELLS / FNB_SLAB < (1 << 15), "fi_row_of takes cell indices below 2^15");
static_assert(FNB_CELLS <= (1 << 16), "FnbFlow packs cell indices into 16 bits");

template <typename E>
struct FnbPtrs {
    const float* flow[FNB_NT];
    const E* gout[FNB_NT];
};
__device__ __forceinline__ float fnb_grad(float v) { return v; }
__device__ __forceinline__ float fnb_grad(bf16_t v) { return bf16_widen(v); }

// one pixel under one flow, as the staged kernel keeps it: row j's and column i's parts of the LDS index of tap (j, i)'s
// cell, channel 0 -- both non-negative and below FNB_CELLS < 2^16, two to a word
struct alignas(16) FnbFlow {
    int valid;
    float alpha, beta;
    int pad;
    unsigned ro[2], co[2];
};
// ... and as the direct kernel keeps it
struct FnbGeom {
    int valid, ix, iy;
    float alpha, beta;
};

struct FnbTile { int b, x0, y0; };
__device__ __forceinline__ FnbTile fnb_tile_at(int tile, int tiles_x, int tiles_y) {
    FnbTile t;
    t.b = tile / (tiles_x * tiles_y);
    const int trem = tile - t.b * (tiles_x * tiles_y);
    const int ty = trem / tiles_x;
    t.x0 = (trem - ty * tiles_x) * FNB_TW;
    t.y0 = ty * FNB_TH;
    return t;
}

__device__ __forceinline__ FiFlow fnb_flow_at(const float* __restrict__ in2, const vfi_strides4& s2, int b, int x, int y, bool inimg) {
    FiFlow f{0.0f, 0.0f};
    if (inimg) {
        const float* flow = in2 + (int64_t)b * s2.b + (int64_t)y * s2.h + (int64_t)x * s2.w;
        f.fx = flow[0];
        f.fy = flow[s2.c];
    }
    return f;
}

// ------------------------------------------------------------------ fs == 4, staged

template <typename E, int V>
__global__ __launch_bounds__(FNB_THREADS, 2) void fi_nhwc_backward4_lds(
    FnbPtrs<E> ptr, int nt, const float* __restrict__ in3, unsigned long long* __restrict__ acc, const int* __restrict__ hdr,
    int* __restrict__ tileflag, int channel, int h, int w, vfi_strides4 s2, vfi_strides4 s3, vfi_strides_nhwc sg,
    int tiles_x, int tiles_y, int ntiles) {
    typedef E VE __attribute__((ext_vector_type(V > 1 ? V : 2)));      // (V == 1 never touches it)
    constexpr int CHUNKS = FNB_SLAB / V;                                // items per pixel, flow and pass
    static_assert(V >= 1 && FNB_SLAB % V == 0 && (CHUNKS & (CHUNKS - 1)) == 0, "a slab is whole chunks");
    __shared__ __attribute__((aligned(16))) unsigned long long lds64[2 + FNB_CELLS];      // header (bounding box), cells
    __shared__ FnbFlow rec[FNB_NT][FNB_PIXELS];
    __shared__ float taps[FNB_PIXELS][16];
    int* box = reinterpret_cast<int*>(lds64);
    unsigned long long* cells = lds64 + 2;

    const int tile = fi_xcd_tile<int>(blockIdx.x);
    if (tile >= ntiles) return;
    const int tid = threadIdx.x;
    const FnbTile at = fnb_tile_at(tile, tiles_x, tiles_y);
    const GradAccCtx gctx = gradacc_ctx(hdr);

    if (!gradacc_staged_ok(gctx)) {                         // (workgroup-uniform) the call is left to fi_nhwc_backward_any
        if (tid == 0) tileflag[tile] = (1 << nt) - 1;
        return;
    }
    // ---- records: thread tid forms (pixel, flow) pairs tid and tid + FNB_THREADS of the FNB_NT * FNB_PIXELS
    FiGeom geo[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int pair = tid + r * FNB_THREADS;
        const int p = pair % FNB_PIXELS, t = pair / FNB_PIXELS;
        const int x = at.x0 + (p % FNB_TW), y = at.y0 + (p / FNB_TW);
        const bool live = t < nt && x < w && y < h;
        const FiFlow fl = fnb_flow_at(ptr.flow[t < FNB_NT ? t : 0], s2, at.b, x, y, live);
        geo[r] = fi_geom(fl.fx, fl.fy, x, y, w, h, live);
        if (t < FNB_NT) {
            FnbFlow& o = rec[t][p];
            o.valid = geo[r].valid;
            o.alpha = geo[r].alpha; o.beta = geo[r].beta; o.pad = 0;
        }
    }
    {
        // the 16 filter taps of a pixel, eight per thread
        const int p = tid >> 1, half = tid & 1;
        const int x = at.x0 + (p % FNB_TW), y = at.y0 + (p / FNB_TW);
        if (p < FNB_PIXELS) {
            const bool inimg = x < w && y < h;
            const float* fpx = in3 + (int64_t)at.b * s3.b + (int64_t)y * s3.h + (int64_t)x * s3.w;
#pragma unroll
            for (int k = 0; k < 8; ++k) taps[p][8 * half + k] = inimg ? fpx[(int64_t)(8 * half + k) * s3.c] : 0.0f;
        }
    }

    unsigned long long* gimg = acc + (int64_t)at.b * h * w * channel;   // dense [b][y][x][c] fixed-point sums
    // Lanes of one 32-lane LDS group sit V cells apart; the group's banks wrap every 32 / V lanes.  Each lane walks its V
    // channels from another start, so the lanes that would share banks are on different cells of their slabs.
    const int rot = V > 1 ? ((tid & 31) / (32 / (V > 1 ? V : 2))) % V : 0;
    // ---- flow groups [t_lo, t_hi): all the launch's flows on their union window; where that does not fit, flow by flow, each
    // on its own window; a flow whose own window does not fit is flagged for fi_nhwc_backward_any.  Everything that decides
    // is workgroup-uniform.
    int flagged = 0, t_lo = 0, t_hi = nt;
    while (t_lo < nt) {
        __syncthreads();                                    // nobody reads the previous group's box or records any more
        if (tid == 0) fi_box_clear(box);
        __syncthreads();
        int lo_x = INT_MAX, lo_y = INT_MAX, hi_x = INT_MIN, hi_y = INT_MIN;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int t = (tid + r * FNB_THREADS) / FNB_PIXELS;
            if (geo[r].valid && t >= t_lo && t < t_hi) {
                lo_x = min(lo_x, clampi(geo[r].ix - 1, 0, w - 1)); lo_y = min(lo_y, clampi(geo[r].iy - 1, 0, h - 1));
                hi_x = max(hi_x, clampi(geo[r].ix + 2, 0, w - 1)); hi_y = max(hi_y, clampi(geo[r].iy + 2, 0, h - 1));
            }
        }
        const bool any = fi_box_fold(box, tid, lo_x, lo_y, hi_x, hi_y);        // (false: nothing in this group has a gradient)
        const int bx0 = box[0], by0 = box[1], bw = box[2] - box[0] + 1, bh = box[3] - box[1] + 1;
        const int n = any && (int64_t)bw * bh * FNB_SLAB <= FNB_CELLS ? bw * bh : 0;       // (0: nothing to do here)
        if (any && n == 0) {                                // the window does not fit
            if (t_hi - t_lo > 1) { t_hi = t_lo + 1; continue; }
            flagged |= 1 << t_lo;
        }
        const int g_lo = t_lo, g_n = t_hi - t_lo;
        t_lo = t_hi;
        t_hi = g_n == nt ? nt : min(nt, t_lo + 1);          // (after a split every group is one flow)
        if (n == 0) continue;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int pair = tid + r * FNB_THREADS;
            const int p = pair % FNB_PIXELS, t = pair / FNB_PIXELS;
            if (t < g_lo || t >= g_lo + g_n) continue;
            FnbFlow& o = rec[t][p];
            // (an invalid pixel's offsets are never read)
            unsigned ro[4], co[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ro[k] = (unsigned)((clampi(geo[r].iy - 1 + k, 0, h - 1) - by0) * bw * FNB_SLAB) & 0xffffu;
                co[k] = (unsigned)((clampi(geo[r].ix - 1 + k, 0, w - 1) - bx0) * FNB_SLAB) & 0xffffu;
            }
            o.ro[0] = ro[0] | (ro[1] << 16); o.ro[1] = ro[2] | (ro[3] << 16);
            o.co[0] = co[0] | (co[1] << 16); o.co[1] = co[2] | (co[3] << 16);
        }
        for (int e = tid; e < n * FNB_SLAB; e += FNB_THREADS) cells[e] = 0ull;
        const float inv_bw = 1.0f / (float)bw;
        const int items = g_n * FNB_PIXELS * CHUNKS;
        for (int c0 = 0; c0 < channel; c0 += FNB_SLAB) {
            const int cn = min(FNB_SLAB, channel - c0);
            __syncthreads();                                    // the records are written and the cells are zero
            for (int i = tid; i < items; i += FNB_THREADS) {
                const int chunk = i & (CHUNKS - 1);
                const int p = (i / CHUNKS) % FNB_PIXELS, t = g_lo + i / (CHUNKS * FNB_PIXELS);
                const int cc = chunk * V;
                if (cc >= cn) continue;
                const FnbFlow& r = rec[t][p];
                if (!r.valid) continue;
                const int x = at.x0 + (p % FNB_TW), y = at.y0 + (p / FNB_TW);
                const E* gp = ptr.gout[t] + (int64_t)at.b * sg.b + (int64_t)y * sg.h + (int64_t)x * sg.w + c0 + cc;
                float g[V];
                const int ne = min(V, cn - cc);
                bool whole = false;
                if constexpr (V > 1) {
                    whole = ne == V;
                    if (whole) {
                        const VE v = *reinterpret_cast<const VE*>(gp);
#pragma unroll
                        for (int e = 0; e < V; ++e) g[e] = fnb_grad(v[e]);
                    }
                }
                if (!whole) {
                    // one element at a time: the single-element instance, and the channel tail of the others
#pragma unroll
                    for (int e = 0; e < V; ++e) g[e] = e < ne ? fnb_grad(gp[e]) : 0.0f;
                }
                const float alpha = r.alpha, beta = r.beta;
                float fv[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) fv[k] = taps[p][k];
                int ro[4], co[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    ro[k] = (int)((r.ro[k >> 1] >> (16 * (k & 1))) & 0xffffu);
                    co[k] = (int)((r.co[k >> 1] >> (16 * (k & 1))) & 0xffffu) + cc;
                }
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const int ee = V > 1 ? (e + rot) % V : 0;
                    if (ee >= ne) continue;
                    float ge = g[0];
#pragma unroll
                    for (int s = 1; s < V; ++s) ge = ee == s ? g[s] : ge;
                    const float qg[4] = { ge * (1.0f - alpha) * (1.0f - beta), ge * alpha * (1.0f - beta),
                                          ge * (1.0f - alpha) * beta,          ge * alpha * beta };
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const int j = k >> 2, q = k & 3, quad = (j >> 1) * 2 + (q >> 1);
                        atomicAdd(&cells[ro[j] + co[q] + ee], (unsigned long long)__float2ll_rn(qg[quad] * fv[k] * gctx.scale));
                    }
                }
            }
            __syncthreads();
            // ---- flush: one global atomic per non-zero cell, and the cell is zero again for the next pass
            for (int e = tid; e < n * FNB_SLAB; e += FNB_THREADS) {
                const unsigned long long v = cells[e];
                if (v != 0ull) {
                    const int cell = e / FNB_SLAB, ch = e % FNB_SLAB;
                    const int cy = fi_row_of(cell, inv_bw), cx = cell - cy * bw;
                    atomicAdd(&gimg[((int64_t)(by0 + cy) * w + bx0 + cx) * channel + c0 + ch], v);
                    cells[e] = 0ull;
                }
            }
        }
    }
    if (flagged && tid == 0) tileflag[tile] = flagged;
}

// ------------------------------------------------------------------ any filter size, direct

// A bfloat16 call that scatters in fp32 adds its floats into the low words of the zeroed 64-bit cells (gradacc.h), never
// into bfloat16 storage: g1 is not looked at.
template <typename E>
__global__ __launch_bounds__(FNB_THREADS) void fi_nhwc_backward_any(
    FnbPtrs<E> ptr, int nt, const float* __restrict__ in3, unsigned long long* __restrict__ acc, const int* __restrict__ hdr,
    const int* __restrict__ tileflag, float* g1, int channel, int h, int w, int fs, vfi_strides_nhwc s1, vfi_strides4 s2,
    vfi_strides4 s3, vfi_strides_nhwc sg, int tiles_x, int tiles_y, int ntiles) {
    __shared__ FnbGeom rec[FNB_NT][FNB_PIXELS];
    const int tile = fi_xcd_tile<int>(blockIdx.x);
    if (tile >= ntiles) return;
    const int flows_left = tileflag ? tileflag[tile] : ~0;  // bit t: the staged kernel left flow t of this tile alone
    if (!flows_left) return;                                // (workgroup-uniform)
    const int tid = threadIdx.x;
    const FnbTile at = fnb_tile_at(tile, tiles_x, tiles_y);
    const GradAccCtx gctx = gradacc_ctx(hdr);
    for (int pair = tid; pair < FNB_NT * FNB_PIXELS; pair += FNB_THREADS) {
        const int p = pair % FNB_PIXELS, t = pair / FNB_PIXELS;
        const int x = at.x0 + (p % FNB_TW), y = at.y0 + (p / FNB_TW);
        const bool live = t < nt && x < w && y < h;
        const FiFlow fl = fnb_flow_at(ptr.flow[t], s2, at.b, x, y, live);
        const FiGeom g = fi_geom(fl.fx, fl.fy, x, y, w, h, live);
        rec[t][p] = FnbGeom{g.valid, g.ix, g.iy, g.alpha, g.beta};
    }
    __syncthreads();

    unsigned long long* gimg = acc + (int64_t)at.b * h * w * channel;   // dense [b][y][x][c] fixed-point sums
    // (the fp32 scatter of a call with non-finite inputs)
    float* gfp = std::is_same<E, float>::value ? g1 + (int64_t)at.b * s1.b : reinterpret_cast<float*>(gimg);
    const int64_t items = (int64_t)FNB_PIXELS * channel;
    for (int64_t i = tid; i < items; i += FNB_THREADS) {
        const int p = (int)(i / channel), c = (int)(i - (int64_t)p * channel);
        const int x = at.x0 + (p % FNB_TW), y = at.y0 + (p / FNB_TW);
        if (x >= w || y >= h) continue;
        const float* fpx = in3 + (int64_t)at.b * s3.b + (int64_t)y * s3.h + (int64_t)x * s3.w;
        for (int t = 0; t < nt; ++t) {
            const FnbGeom& r = rec[t][p];
            if (!r.valid || !((flows_left >> t) & 1)) continue;        // no gradient, or summed by the staged kernel
            const int ix = r.ix, iy = r.iy;
            const int L = ix + 1 - fs / 2, T = iy + 1 - fs / 2;
            const float alpha = r.alpha, beta = r.beta;
            const float gr = fnb_grad(ptr.gout[t][(int64_t)at.b * sg.b + (int64_t)y * sg.h + (int64_t)x * sg.w + c]);
            const float qg[4] = { gr * (1.0f - alpha) * (1.0f - beta), gr * alpha * (1.0f - beta),
                                  gr * (1.0f - alpha) * beta,          gr * alpha * beta };
            for (int j = 0; j < fs; ++j) {
                const int cy = clampi(T + j, 0, h - 1);
                for (int q = 0; q < fs; ++q) {
                    const int cx = clampi(L + q, 0, w - 1);
                    const int quad = (T + j > iy ? 2 : 0) + (L + q > ix ? 1 : 0);
                    const float fv = fpx[(int64_t)(j * fs + q) * s3.c];
                    const int64_t di = ((int64_t)cy * w + cx) * channel + c;
                    if constexpr (std::is_same<E, float>::value)
                        gradacc_add(gimg, gfp, di, (int64_t)cy * s1.h + (int64_t)cx * s1.w + c, qg[quad] * fv, gctx);
                    else                                    // (float index 2 x cell index: the cell's low word)
                        gradacc_add(gimg, gfp, di, 2 * di, qg[quad] * fv, gctx);
                }
            }
        }
    }
}

// ------------------------------------------------------------------ the header

// largest |filter tap| into hdr[2], a NaN or an infinity raises hdr[1]: gradacc_max's words for a filter with four strides
__global__ __launch_bounds__(256) void fnb_filter_max(const float* __restrict__ in3, int filter_channels, int h, int w,
                                                      vfi_strides4 s3, int64_t n, int* __restrict__ hdr) {
    int m = 0;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int x = (int)(i % w);
        const int64_t r = i / w;
        const int y = (int)(r % h);
        const int64_t bc = r / h;
        const int c = (int)(bc % filter_channels), b = (int)(bc / filter_channels);
        const int bits = __float_as_int(fabsf(in3[(int64_t)b * s3.b + (int64_t)c * s3.c + (int64_t)y * s3.h + (int64_t)x * s3.w]));
        bad = bad || bits >= 0x7f800000;
        m = max(m, bits >= 0x7f800000 ? 0 : bits);
    }
    // one atomic per block, and only from a block that raises the maximum (as gradacc_max: atomics on one word serialise)
    __shared__ int wm[4], wbad[4];
    m = wave_max_i32(m);
    const bool anybad = __builtin_amdgcn_ballot_w64(bad) != 0ull;       // (all lanes active here)
    if ((threadIdx.x & 63) == 0) {
        wm[threadIdx.x >> 6] = m;
        wbad[threadIdx.x >> 6] = anybad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(wm[0], wm[1]), max(wm[2], wm[3]));
        if (m > __atomic_load_n(&hdr[2], __ATOMIC_RELAXED)) atomicMax(&hdr[2], m);
        if ((wbad[0] | wbad[1] | wbad[2] | wbad[3]) && !__atomic_load_n(&hdr[1], __ATOMIC_RELAXED)) atomicOr(&hdr[1], 1);
    }
}

// hdr[3] of the call: gradacc_scan writes a value for the re-read rows; the call's cells receive every tap of every flow
__global__ void fnb_set_cells_log2(int* __restrict__ hdr, int cells_log2) { hdr[3] = cells_log2; }

// ------------------------------------------------------------------ host

// A [batch, channel, h, w] tensor with channel stride 1 as gradacc's row-walking kernels take it: rows of stride-1 elements
// of a [R.batch, R.channel, R.h, R.w] tensor with strides R.s, whose dense scratch rows are the NHWC-dense scratch.  A pixel
// is a row of `channel` elements; where the pixels of an image row are contiguous too, the image row is the row.
struct FnbRows { int batch, channel, h, w; vfi_strides s; };
static bool fnb_rows(int batch, int channel, int h, int w, const vfi_strides_nhwc& s, FnbRows* r) {
    if ((w == 1 || s.w == channel) && (int64_t)w * channel <= INT_MAX) {
        *r = FnbRows{batch, 1, h, w * channel, vfi_strides{s.b, 0, s.h}};
        return true;
    }
    *r = FnbRows{batch, h, w, channel, vfi_strides{s.b, s.h, s.w}};
    return (int64_t)batch * h * w <= INT_MAX;               // (gradacc's kernels count rows in an int)
}

// The widest gradient load the layout allows, in elements: every address is a gradient's base + a sum of strides + a
// multiple of V, so V elements must divide the bases (in bytes) and every stride that is ever multiplied by a non-zero
// index.  Misaligned vector accesses are never issued.
template <typename E>
static int fnb_vector_width(const void* const* gradoutputs, int nflows, int batch, int h, int w, const vfi_strides_nhwc& sg) {
    for (int v = 16 / (int)sizeof(E); v > 1; v >>= 1) {
        bool ok = (batch == 1 || sg.b % v == 0) && (h == 1 || sg.h % v == 0) && (w == 1 || sg.w % v == 0);
        for (int t = 0; ok && t < nflows; ++t) ok = reinterpret_cast<uintptr_t>(gradoutputs[t]) % (v * sizeof(E)) == 0;
        if (ok) return v;
    }
    return 1;
}

// DIRECT: every tile through fi_nhwc_backward_any (an internal switch: the tests and tools compare the staged kernel with it)
template <typename E, bool DIRECT>
static int backward_nhwc_image_multi(const float* const* flows, const float* input3, const void* const* gradoutputs,
                                     void* gradinput1, int nflows, int batch, int channel, int h, int w, int filter_channels,
                                     vfi_strides_nhwc s1, vfi_strides4 s2, vfi_strides4 s3, vfi_strides_nhwc sg,
                                     vfi_stream_t stream) {
    constexpr bool F32 = std::is_same<E, float>::value;
    using Scan = typename std::conditional<F32, GradPlain, GradBf16>::type;
    if (nflows <= 0 || !flows || !gradoutputs || batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || filter_channels <= 0)
        return VFI_ERR_SHAPE;
    if (!input3 || !gradinput1) return VFI_ERR_SHAPE;
    for (int t = 0; t < nflows; ++t)
        if (!flows[t] || !gradoutputs[t]) return VFI_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int fs = fi_filter_size(filter_channels);
    const bool staged = !DIRECT && fs == 4 && filter_channels == 16;
    const int tiles_x = (w + FNB_TW - 1) / FNB_TW, tiles_y = (h + FNB_TH - 1) / FNB_TH;
    const int64_t ntiles64 = (int64_t)tiles_x * tiles_y * batch;
    const int launches = (nflows + FNB_NT - 1) / FNB_NT;
    if (batch > 65535 || ntiles64 > (1 << 28) || ntiles64 * launches > INT_MAX) return VFI_ERR_SHAPE;
    FnbRows rg, r1;
    if (!fnb_rows(batch, channel, h, w, sg, &rg) || !fnb_rows(batch, channel, h, w, s1, &r1)) return VFI_ERR_SHAPE;
    const int ntiles = (int)ntiles64;
    // one plane of sums, one header; flags: one word per tile and launch, bit t: "the staged kernel left flow t alone"
    GradAccScratch sc;
    int err = gradacc_reserve(st, 1, (int64_t)batch * channel * h * w, staged ? ntiles * launches : 0, &sc);
    if (err != VFI_OK) return err;
    int* hdr = sc.dir[0].hdr;
    // the maxima over every gradient and the filter (raised with atomicMax into the one header)
    for (int t = 0; t < nflows; ++t) {
        err = gradacc_scan(st, Scan{static_cast<const E*>(gradoutputs[t])}, rg.batch, rg.channel, rg.h, rg.w, rg.s, nullptr,
                           filter_channels, rg.s, hdr);
        if (err != VFI_OK) return err;
    }
    const int64_t nfilt = (int64_t)batch * filter_channels * h * w;
    const int64_t fblocks = (nfilt + 255) / 256;
    hipLaunchKernelGGL(fnb_filter_max, dim3((unsigned)(fblocks < 2048 ? fblocks : 2048)), dim3(256), 0, st, input3,
                       filter_channels, h, w, s3, nfilt, hdr);
    // a cell can receive every tap of every pixel of every flow
    const int64_t taps = (int64_t)(filter_channels > 4 ? filter_channels : 4) * nflows;
    int cells_log2 = 0;
    while (cells_log2 < 62 && ((int64_t)1 << cells_log2) < (int64_t)h * w * taps) ++cells_log2;
    hipLaunchKernelGGL(fnb_set_cells_log2, dim3(1), dim3(1), 0, st, hdr, cells_log2);
    if (launch_status() != VFI_OK) return VFI_ERR_LAUNCH;
    if constexpr (F32) {                                    // (a bfloat16 call's fp32 scatter goes into the zeroed scratch)
        err = gradacc_zero_fp32(st, hdr, static_cast<float*>(gradinput1), r1.batch, r1.channel, r1.h, r1.w, r1.s);
        if (err != VFI_OK) return err;
    }
    const int v = staged ? fnb_vector_width<E>(gradoutputs, nflows, batch, h, w, sg) : 1;
    const dim3 grid((unsigned)fi_xcd_grid(ntiles), 1, 1), block(FNB_THREADS, 1, 1);
    for (int l = 0; l < launches; ++l) {
        FnbPtrs<E> ptr;
        const int nt = nflows - l * FNB_NT < FNB_NT ? nflows - l * FNB_NT : FNB_NT;
        for (int t = 0; t < FNB_NT; ++t) {
            ptr.flow[t] = flows[l * FNB_NT + (t < nt ? t : 0)];
            ptr.gout[t] = static_cast<const E*>(gradoutputs[l * FNB_NT + (t < nt ? t : 0)]);
        }
        int* flags = staged ? sc.flags + (int64_t)l * ntiles : nullptr;
#define FNB_LAUNCH4(V) hipLaunchKernelGGL((fi_nhwc_backward4_lds<E, V>), grid, block, 0, st, ptr, nt, input3, sc.dir[0].acc, hdr, \
                                          flags, channel, h, w, s2, s3, sg, tiles_x, tiles_y, ntiles)
        if (staged) {
            if (v * sizeof(E) == 16) FNB_LAUNCH4(16 / (int)sizeof(E));
            else if (v * sizeof(E) == 8) FNB_LAUNCH4(8 / (int)sizeof(E));
            else if (v * sizeof(E) == 4 && sizeof(E) == 2) FNB_LAUNCH4(2);
            else FNB_LAUNCH4(1);
        }
#undef FNB_LAUNCH4
        hipLaunchKernelGGL(fi_nhwc_backward_any<E>, grid, block, 0, st, ptr, nt, input3, sc.dir[0].acc, hdr, flags,
                           F32 ? static_cast<float*>(gradinput1) : nullptr, channel, h, w, fs, s1, s2, s3, sg, tiles_x, tiles_y,
                           ntiles);
    }
    if (launch_status() != VFI_OK) return VFI_ERR_LAUNCH;
    if constexpr (F32)
        return gradacc_finish(st, sc.dir[0], static_cast<float*>(gradinput1), r1.batch, r1.channel, r1.h, r1.w, r1.s, true);
    else
        return gradacc_finish_bf16(st, sc.dir[0], static_cast<bf16_t*>(gradinput1), r1.batch, r1.channel, r1.h, r1.w, r1.s);
}

}  // namespace vfi

using namespace vfi;

#define FNB_ARGS flows, input3, reinterpret_cast<const void* const*>(gradoutputs), gradinput1, nflows, batch, channel, h, w, \
                 filter_channels, s1, s2, s3, sg, stream

extern "C" int vfi_filterinterp_backward_ori_nhwc_image_multi(const float* const* flows, const float* input3,
                                                               const float* const* gradoutputs, float* gradinput1, int nflows,
                                                               int batch, int channel, int h, int w, int filter_channels,
                                                               vfi_strides_nhwc s1, vfi_strides4 s2, vfi_strides4 s3,
                                                               vfi_strides_nhwc sg, vfi_stream_t stream) {
    return backward_nhwc_image_multi<float, false>(FNB_ARGS);
}

extern "C" int vfi_filterinterp_backward_ori_nhwc_image_multi_bf16(const float* const* flows, const float* input3,
                                                                    const void* const* gradoutputs_bf16, void* gradinput1_bf16,
                                                                    int nflows, int batch, int channel, int h, int w,
                                                                    int filter_channels, vfi_strides_nhwc s1, vfi_strides4 s2,
                                                                    vfi_strides4 s3, vfi_strides_nhwc sg, vfi_stream_t stream) {
    const void* const* gradoutputs = gradoutputs_bf16;
    void* gradinput1 = gradinput1_bf16;
    return backward_nhwc_image_multi<bf16_t, false>(FNB_ARGS);
}

// internal: the same calls with every tile on fi_nhwc_backward_any (the tests and tools compare the staged kernel with it)
extern "C" int vfi_filterinterp_backward_ori_nhwc_image_multi_direct(const float* const* flows, const float* input3,
                                                                      const float* const* gradoutputs, float* gradinput1,
                                                                      int nflows, int batch, int channel, int h, int w,
                                                                      int filter_channels, vfi_strides_nhwc s1, vfi_strides4 s2,
                                                                      vfi_strides4 s3, vfi_strides_nhwc sg, vfi_stream_t stream) {
    return backward_nhwc_image_multi<float, true>(FNB_ARGS);
}

extern "C" int vfi_filterinterp_backward_ori_nhwc_image_multi_bf16_direct(const float* const* flows, const float* input3,
                                                                           const void* const* gradoutputs_bf16,
                                                                           void* gradinput1_bf16, int nflows, int batch,
                                                                           int channel, int h, int w, int filter_channels,
                                                                           vfi_strides_nhwc s1, vfi_strides4 s2, vfi_strides4 s3,
                                                                           vfi_strides_nhwc sg, vfi_stream_t stream) {
    const void* const* gradoutputs = gradoutputs_bf16;
    void* gradinput1 = gradinput1_bf16;
    return backward_nhwc_image_multi<bf16_t, true>(FNB_ARGS);
}
#undef FNB_ARGS

// internal: the gradient access width, in elements, that the entries above choose for these layouts (element_bytes 4 or 2);
// -1 for arguments they would refuse.  Host code only: the tests pin the launcher's choice with it.
extern "C" int vfi_filterinterp_nhwc_bwd_access_width(int element_bytes, const void* const* gradoutputs, int nflows, int batch,
                                                       int h, int w, int filter_channels, vfi_strides_nhwc sg) {
    if ((element_bytes != 4 && element_bytes != 2) || !gradoutputs || nflows <= 0 || batch <= 0 || h <= 0 || w <= 0 ||
        filter_channels != 16)
        return -1;
    return element_bytes == 4 ? fnb_vector_width<float>(gradoutputs, nflows, batch, h, w, sg)
                              : fnb_vector_width<bf16_t>(gradoutputs, nflows, batch, h, w, sg);
}
