// losses.hip -- the training losses of loss_function.py's part_loss (train.py:183) for gfx950: the Charbonnier pixel
// loss of up to eight tensors, the gradient-adaptive total variation of a flow pair and the pair's motion-symmetry loss.
//   forward : loss_forward (every input read once, one double partial per workgroup and quantity) + loss_finish;
//   backward: loss_backward, one launch for every requested gradient.
// Arithmetic (include/vfi_hip.h has the formulas): every term in fp32 with one rounding per operation (-ffp-contract=off:
// x * x + e2 is two roundings, as torch's elementwise ops), correctly rounded divide and sqrt, sums in double.
//
// A lane owns UNITS of four consecutive elements of one row (the last unit of a row is cut at w).  Where the base
// pointers, the strides and w are multiples of four elements a unit is one 16-byte load, otherwise up to four 4-byte
// loads: the lane sees the same elements in the same order either way, so the sums have the same bits for a strided view
// as for its dense copy.  Reduction order: a lane adds its terms in element order; the 64 lanes of a wave are added by
// an xor butterfly (every lane ends with the same bits: each step adds the same two numbers on both sides); lane 0 of
// the workgroup adds the four waves in order; loss_finish gives thread t the partials t, t + 256, ... in ascending
// order and reduces the 256 threads the same way.  No floating-point atomics anywhere.
#include "workspace.h"

namespace vfi {

#define LOSS_THREADS 256
#define LOSS_DIFF_UNITS_PER_THREAD 4                                    // a diff workgroup: 1024 units = 4096 elements
#define LOSS_DIFF_BLOCK_UNITS (LOSS_THREADS * LOSS_DIFF_UNITS_PER_THREAD)
#define LOSS_FLOW_BLOCK_UNITS LOSS_THREADS                              // a flow workgroup: 256 units = 1024 pixels
#define LOSS_FINISH_THREADS 256
#define LOSS_NMAX 8

struct LossDiffs { const float* p[LOSS_NMAX]; };
struct LossGrads { float* p[LOSS_NMAX]; };

// sqrt(x^2 + e2): square, add, sqrt, one rounding each
__device__ __forceinline__ float charbonnier(float x, float e2) {
    float t = x * x;
    t = t + e2;
    return sqrtf(t);
}
// T of one cell and channel from f(y,x), f(y+1,x), f(y,x+1); dy and dx are handed back for the backward
__device__ __forceinline__ float tv_term(float f, float fdown, float fright, float e2, float& dy, float& dx) {
    dy = f - fdown;
    dx = f - fright;
    const float a = dy * dy, b = dx * dx;
    float t = a + b;
    t = t + e2;
    return sqrtf(t);
}
// one channel's part of the exponent of w: |I(y,x) - I(y+1,x)| + |I(y,x) - I(y,x+1)|
__device__ __forceinline__ float tv_edge(float i, float idown, float iright) {
    return fabsf(i - idown) + fabsf(i - iright);
}

// v[k] = row[x0 - 1 + k], k = 0..5, zero outside [0, w) and for a null row.  VEC: x0 .. x0+3 as one 16-byte load
// (the caller guarantees alignment and w % 4 == 0, so the four are inside the row).
template <bool VEC>
__device__ __forceinline__ void load_window(const float* __restrict__ row, int x0, int w, float v[6]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = 0.0f;
    if (!row) return;
    if constexpr (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(row + x0);
        v[1] = q.x; v[2] = q.y; v[3] = q.z; v[4] = q.w;
        if (x0 > 0) v[0] = row[x0 - 1];
        if (x0 + 4 < w) v[5] = row[x0 + 4];
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int x = x0 - 1 + k;
            if (x >= 0 && x < w) v[k] = row[x];
        }
    }
}
// the four elements of a unit alone
template <bool VEC>
__device__ __forceinline__ void load_unit(const float* __restrict__ row, int x0, int w, float v[4]) {
    if constexpr (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(row + x0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = x0 + k < w ? row[x0 + k] : 0.0f;
    }
}
template <bool VEC>
__device__ __forceinline__ void store_unit(float* __restrict__ row, int x0, int w, const float v[4]) {
    if constexpr (VEC) {
        *reinterpret_cast<float4*>(row + x0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x0 + k < w) row[x0 + k] = v[k];
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the workgroup's sum, valid in thread 0 (waves added in order); `part` is reused: the trailing barrier frees it
__device__ __forceinline__ double block_sum(double v, double* part) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = part[0];
    for (int k = 1; k < LOSS_THREADS / 64; ++k) s += part[k];
    __syncthreads();
    return s;
}

struct LossShape {
    int nd, batch, cd, ci, h, w;
    int units;                  // units per row: ceil(w / 4)
    int diff_blocks;            // workgroups per (tensor, sample)
    int flow_blocks;            // workgroups per sample of the flow part (0: no flows)
    float e2;
};

// exponent sums of one unit: own[e] of the cell (y, x0+e), and -- for the backward -- up[e] of (y-1, x0+e) and left[e] of
// (y, x0+e-1).  Channels are added in order; a sum whose cell does not exist is formed from zero padding and never used.
template <bool VEC, bool BWD>
__device__ __forceinline__ void tv_exponents(const float* __restrict__ img, vfi_strides si, int ci, int y, int h, int x0, int w,
                                             float own[4], float up[4], float left[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) own[e] = up[e] = left[e] = 0.0f;
    for (int c = 0; c < ci; ++c) {
        const float* plane = img + (int64_t)c * si.c;
        float r0[6], r1[6], r2[6];
        load_window<VEC>(BWD && y > 0 ? plane + (int64_t)(y - 1) * si.h : nullptr, x0, w, r0);
        load_window<VEC>(plane + (int64_t)y * si.h, x0, w, r1);
        load_window<VEC>(y + 1 < h ? plane + (int64_t)(y + 1) * si.h : nullptr, x0, w, r2);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            own[e] = own[e] + tv_edge(r1[e + 1], r2[e + 1], r1[e + 2]);
            if constexpr (BWD) {
                up[e] = up[e] + tv_edge(r0[e + 1], r1[e + 1], r0[e + 2]);
                left[e] = left[e] + tv_edge(r1[e], r2[e], r1[e + 1]);
            }
        }
    }
}

// ------------------------------------------------------------------ forward
// blocks [0, nd * batch * diff_blocks): tensor i, sample b, chunk k -> partial[(i * batch + b) * diff_blocks + k];
// then batch * flow_blocks blocks: sample b, chunk k -> fpart[(b * flow_blocks + k) * 3 + {tv0, tv1, sym}]
template <bool VEC_D, bool VEC_F>
__global__ __launch_bounds__(LOSS_THREADS) void loss_forward(LossDiffs diffs, const float* __restrict__ target,
                                                              const float* __restrict__ flow0, const float* __restrict__ flow1,
                                                              const float* __restrict__ img0, const float* __restrict__ img1,
                                                              LossShape s, vfi_strides sd, vfi_strides sf, vfi_strides si,
                                                              double* __restrict__ partial) {
    __shared__ double part[LOSS_THREADS / 64];
    const int64_t ndiff = (int64_t)s.nd * s.batch * s.diff_blocks;
    const int64_t blk = blockIdx.x;
    if (blk < ndiff) {
        const int k = (int)(blk % s.diff_blocks);
        const int ib = (int)(blk / s.diff_blocks);
        const int b = ib % s.batch, i = ib / s.batch;
        const float* base = diffs.p[i] + (int64_t)b * sd.b;
        const float* tbase = target ? target + (int64_t)b * sd.b : nullptr;
        const int64_t total = (int64_t)s.cd * s.h * s.units;
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < LOSS_DIFF_UNITS_PER_THREAD; ++j) {
            const int64_t q = (int64_t)k * LOSS_DIFF_BLOCK_UNITS + j * LOSS_THREADS + threadIdx.x;
            if (q >= total) continue;
            const int u = (int)(q % s.units);
            const int64_t row = q / s.units;
            const int y = (int)(row % s.h), c = (int)(row / s.h);
            const int64_t off = (int64_t)c * sd.c + (int64_t)y * sd.h;
            float x[4], t[4];
            load_unit<VEC_D>(base + off, 4 * u, s.w, x);
            if (tbase) {
                load_unit<VEC_D>(tbase + off, 4 * u, s.w, t);
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = x[e] - t[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * u + e < s.w) acc += (double)charbonnier(x[e], s.e2);
        }
        const double sum = block_sum(acc, part);
        if (threadIdx.x == 0) partial[blk] = sum;
        return;
    }
    const int64_t fb = blk - ndiff;
    const int k = (int)(fb % s.flow_blocks), b = (int)(fb / s.flow_blocks);
    const int64_t q = (int64_t)k * LOSS_FLOW_BLOCK_UNITS + threadIdx.x;
    double tv[2] = {0.0, 0.0}, sym = 0.0;
    if (q < (int64_t)s.h * s.units) {
        const int u = (int)(q % s.units), y = (int)(q / s.units), x0 = 4 * u;
        const bool inner_row = y + 1 < s.h;
        float centre[2][2][4];                             // [side][channel][element]: f(y, x0 + e)
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const float* fl = (side == 0 ? flow0 : flow1) + (int64_t)b * sf.b;
            const float* im = (side == 0 ? img0 : img1) + (int64_t)b * si.b;
            float own[4], up[4], left[4];
            if (inner_row) tv_exponents<VEC_F, false>(im, si, s.ci, y, s.h, x0, s.w, own, up, left);
            float T[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float* plane = fl + (int64_t)c * sf.c;
                float r1[6], r2[6];
                load_window<VEC_F>(plane + (int64_t)y * sf.h, x0, s.w, r1);
                load_window<VEC_F>(inner_row ? plane + (int64_t)(y + 1) * sf.h : nullptr, x0, s.w, r2);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    centre[side][c][e] = r1[e + 1];
                    float dy, dx;
                    const float t = tv_term(r1[e + 1], r2[e + 1], r1[e + 2], s.e2, dy, dx);
                    T[e] = c == 0 ? t : T[e] + t;          // T_0 + T_1
                }
            }
            if (inner_row) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (x0 + e + 1 < s.w) tv[side] += (double)(expf(-own[e]) * T[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (x0 + e >= s.w) continue;
#pragma unroll
            for (int c = 0; c < 2; ++c) sym += (double)charbonnier(centre[0][c][e] + centre[1][c][e], s.e2);
        }
    }
    double* fpart = partial + ndiff + fb * 3;
    const double s0 = block_sum(tv[0], part), s1 = block_sum(tv[1], part), s2 = block_sum(sym, part);
    if (threadIdx.x == 0) { fpart[0] = s0; fpart[1] = s1; fpart[2] = s2; }
}

// the sum of n partials p[0], p[stride], ...: thread t takes t, t + 256, ... in ascending order; valid in thread 0
__device__ __forceinline__ double finish_sum(const double* __restrict__ p, int64_t n, int stride, double* part) {
    double acc = 0.0;
    for (int64_t k = threadIdx.x; k < n; k += LOSS_FINISH_THREADS) acc += p[k * stride];
    return block_sum(acc, part);
}

// block i < nd: the samples of tensor i in order -> sample_means[i * batch + b], values[i]; block nd: offset and sym
__global__ __launch_bounds__(LOSS_FINISH_THREADS) void loss_finish(const double* __restrict__ partial, LossShape s, int neg_psnr,
                                                                   float* __restrict__ values, float* __restrict__ sample_means) {
    __shared__ double part[LOSS_THREADS / 64];
    const int i = blockIdx.x;
    if (i < s.nd) {
        const double n = (double)s.cd * (double)s.h * (double)s.w;
        double total = 0.0;
        for (int b = 0; b < s.batch; ++b) {
            const double sum = finish_sum(partial + ((int64_t)i * s.batch + b) * s.diff_blocks, s.diff_blocks, 1, part);
            if (threadIdx.x != 0) continue;
            const float l = (float)(sum / n);
            sample_means[i * s.batch + b] = l;
            if (neg_psnr) {
                const float r = 1.0f / l;
                const float v = -logf(r);
                total += (double)(v / 100.0f);
            } else {
                total += sum;
            }
        }
        if (threadIdx.x == 0) values[i] = (float)(neg_psnr ? total / (double)s.batch : total / (n * (double)s.batch));
        return;
    }
    if (s.flow_blocks == 0) {
        if (threadIdx.x == 0) values[s.nd] = values[s.nd + 1] = 0.0f;
        return;
    }
    const double* fpart = partial + (int64_t)s.nd * s.batch * s.diff_blocks;
    const int64_t np = (int64_t)s.batch * s.flow_blocks;
    const double t0 = finish_sum(fpart, np, 3, part), t1 = finish_sum(fpart + 1, np, 3, part), sy = finish_sum(fpart + 2, np, 3, part);
    if (threadIdx.x == 0) {
        const double ntv = (double)s.batch * (double)(s.h - 1) * (double)(s.w - 1);
        const float v0 = (float)(t0 / ntv), v1 = (float)(t1 / ntv);
        values[s.nd] = v0 + v1;
        values[s.nd + 1] = (float)(sy / ((double)s.batch * 2.0 * (double)s.h * (double)s.w));
    }
}

// ------------------------------------------------------------------ backward
struct LossBwdJobs {
    int first[LOSS_NMAX + 2];   // first block of diff job j (job_tensor[j]); first[njobs] = the flow job's first block
    int tensor[LOSS_NMAX];
    int njobs;                  // diff jobs
    unsigned mask;              // loss_mask
};

template <bool VEC_D, bool VEC_F>
__global__ __launch_bounds__(LOSS_THREADS) void loss_backward(LossDiffs diffs, const float* __restrict__ target,
                                                               const float* __restrict__ flow0, const float* __restrict__ flow1,
                                                               const float* __restrict__ img0, const float* __restrict__ img1,
                                                               LossShape s, int neg_psnr, const float* __restrict__ gvalues,
                                                               const float* __restrict__ sample_means, LossBwdJobs jobs,
                                                               LossGrads gdiffs, float* __restrict__ gflow0, float* __restrict__ gflow1,
                                                               vfi_strides sd, vfi_strides sf, vfi_strides si, vfi_strides sgd,
                                                               vfi_strides sgf) {
    const int blk = blockIdx.x;
    if (blk < jobs.first[jobs.njobs]) {
        int j = 0;
        while (j + 1 < jobs.njobs && blk >= jobs.first[j + 1]) ++j;
        const int i = jobs.tensor[j];
        const bool live = (jobs.mask >> i) & 1u;
        const float g = live ? gvalues[i] : 0.0f;
        const int64_t per_sample = (int64_t)s.cd * s.h * s.units, total = per_sample * s.batch;
        const float nb = (float)((int64_t)s.cd * s.h * s.w);
        const float call = g / (float)((int64_t)s.batch * s.cd * s.h * s.w);
        const float cneg = g / (float)(100 * (int64_t)s.batch);
#pragma unroll
        for (int jj = 0; jj < LOSS_DIFF_UNITS_PER_THREAD; ++jj) {
            const int64_t q = (int64_t)(blk - jobs.first[j]) * LOSS_DIFF_BLOCK_UNITS + jj * LOSS_THREADS + threadIdx.x;
            if (q >= total) continue;
            const int b = (int)(q / per_sample);
            const int64_t r = q % per_sample;
            const int u = (int)(r % s.units);
            const int64_t row = r / s.units;
            const int y = (int)(row % s.h), c = (int)(row / s.h);
            float* out = gdiffs.p[i] + (int64_t)b * sgd.b + (int64_t)c * sgd.c + (int64_t)y * sgd.h;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (live) {
                const int64_t off = (int64_t)b * sd.b + (int64_t)c * sd.c + (int64_t)y * sd.h;
                float x[4], t[4];
                load_unit<VEC_D>(diffs.p[i] + off, 4 * u, s.w, x);
                if (target) {
                    load_unit<VEC_D>(target + off, 4 * u, s.w, t);
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[e] = x[e] - t[e];
                }
                float coef = call;
                if (neg_psnr) {
                    coef = cneg / sample_means[i * s.batch + b];
                    coef = coef / nb;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float ratio = x[e] / charbonnier(x[e], s.e2);
                    v[e] = coef * ratio;
                }
            }
            store_unit<VEC_D>(out, 4 * u, s.w, v);
        }
        return;
    }
    // the flow job: one unit of one row per thread, both sides
    const int64_t q = (int64_t)(blk - jobs.first[jobs.njobs]) * LOSS_FLOW_BLOCK_UNITS + threadIdx.x;
    const int64_t per_sample = (int64_t)s.h * s.units;
    if (q >= per_sample * s.batch) return;
    const int b = (int)(q / per_sample);
    const int64_t r = q % per_sample;
    const int u = (int)(r % s.units), y = (int)(r / s.units), x0 = 4 * u;
    const bool tv_on = (jobs.mask >> s.nd) & 1u, sym_on = (jobs.mask >> (s.nd + 1)) & 1u;
    float k = 0.0f, ks = 0.0f;
    if (tv_on) k = gvalues[s.nd] / (float)((int64_t)s.batch * (s.h - 1) * (s.w - 1));
    if (sym_on) ks = gvalues[s.nd + 1] / (float)((int64_t)s.batch * 2 * s.h * s.w);
    float symterm[2][4];
    if (sym_on) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float a[4], d[4];
            const int64_t off = (int64_t)b * sf.b + (int64_t)c * sf.c + (int64_t)y * sf.h;
            load_unit<VEC_F>(flow0 + off, x0, s.w, a);
            load_unit<VEC_F>(flow1 + off, x0, s.w, d);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float usum = a[e] + d[e];
                const float ratio = usum / charbonnier(usum, s.e2);
                symterm[c][e] = ks * ratio;
            }
        }
    }
    for (int side = 0; side < 2; ++side) {
        float* gout = side == 0 ? gflow0 : gflow1;
        if (!gout) continue;
        const float* fl = (side == 0 ? flow0 : flow1) + (int64_t)b * sf.b;
        float own[4], up[4], left[4];
        if (tv_on) {
            const float* im = (side == 0 ? img0 : img1) + (int64_t)b * si.b;
            tv_exponents<VEC_F, true>(im, si, s.ci, y, s.h, x0, s.w, own, up, left);
#pragma unroll
            for (int e = 0; e < 4; ++e) {                  // k w of the three cells
                own[e] = k * expf(-own[e]);
                up[e] = k * expf(-up[e]);
                left[e] = k * expf(-left[e]);
            }
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (tv_on) {
                const float* plane = fl + (int64_t)c * sf.c;
                float r0[6], r1[6], r2[6];
                load_window<VEC_F>(y > 0 ? plane + (int64_t)(y - 1) * sf.h : nullptr, x0, s.w, r0);
                load_window<VEC_F>(plane + (int64_t)y * sf.h, x0, s.w, r1);
                load_window<VEC_F>(y + 1 < s.h ? plane + (int64_t)(y + 1) * sf.h : nullptr, x0, s.w, r2);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int x = x0 + e;
                    float dy, dx;
                    if (y + 1 < s.h && x + 1 < s.w) {       // own cell (y, x)
                        const float T = tv_term(r1[e + 1], r2[e + 1], r1[e + 2], s.e2, dy, dx);
                        const float a = dy + dx;
                        v[e] = v[e] + own[e] * (a / T);
                    }
                    if (y > 0 && x + 1 < s.w) {             // cell (y-1, x): this pixel is its lower neighbour
                        const float T = tv_term(r0[e + 1], r1[e + 1], r0[e + 2], s.e2, dy, dx);
                        v[e] = v[e] - up[e] * (dy / T);
                    }
                    if (x > 0 && y + 1 < s.h && x < s.w) {  // cell (y, x-1): this pixel is its right neighbour
                        const float T = tv_term(r1[e], r2[e], r1[e + 1], s.e2, dy, dx);
                        v[e] = v[e] - left[e] * (dx / T);
                    }
                }
            }
            if (sym_on) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = v[e] + symterm[c][e];
            }
            store_unit<VEC_F>(gout + (int64_t)b * sgf.b + (int64_t)c * sgf.c + (int64_t)y * sgf.h, x0, s.w, v);
        }
    }
}

// 16-byte units are legal for a tensor when its base and every stride that is used are multiples of four elements
static bool vec_ok(const void* p, vfi_strides st, int batch, int channel, int h) {
    if (!p) return true;
    if ((uintptr_t)p & 15) return false;
    return (batch == 1 || st.b % 4 == 0) && (channel == 1 || st.c % 4 == 0) && (h == 1 || st.h % 4 == 0);
}

static bool loss_shape(int nd, int batch, int cd, int ci, int h, int w, bool flows, double epsilon, LossShape* s) {
    if (nd < 1 || nd > LOSS_NMAX || batch <= 0 || cd <= 0 || h <= 0 || w <= 0) return false;
    if (flows && (ci <= 0 || h < 2 || w < 2)) return false;
    s->nd = nd; s->batch = batch; s->cd = cd; s->ci = ci; s->h = h; s->w = w;
    s->units = (w + 3) / 4;
    const int64_t dunits = (int64_t)cd * h * s->units, funits = (int64_t)h * s->units;
    const int64_t db = (dunits + LOSS_DIFF_BLOCK_UNITS - 1) / LOSS_DIFF_BLOCK_UNITS;
    const int64_t fb = flows ? (funits + LOSS_FLOW_BLOCK_UNITS - 1) / LOSS_FLOW_BLOCK_UNITS : 0;
    if ((db * nd + fb) * batch >= ((int64_t)1 << 31)) return false;
    s->diff_blocks = (int)db;
    s->flow_blocks = (int)fb;
    s->e2 = (float)(epsilon * epsilon);
    return true;
}

}  // namespace vfi

using namespace vfi;

#define LOSS_LAUNCH(KERNEL, VD, VF, ...)                                                                                       \
    do {                                                                                                                        \
        if (VD && VF) hipLaunchKernelGGL((KERNEL<true, true>), __VA_ARGS__);                                                    \
        else if (VD) hipLaunchKernelGGL((KERNEL<true, false>), __VA_ARGS__);                                                    \
        else if (VF) hipLaunchKernelGGL((KERNEL<false, true>), __VA_ARGS__);                                                    \
        else hipLaunchKernelGGL((KERNEL<false, false>), __VA_ARGS__);                                                           \
    } while (0)

extern "C" int vfi_part_loss_forward(const float* const* diffs, int nd, const float* target, const float* flow0,
                                      const float* flow1, const float* img0, const float* img1, int batch, int cd, int ci, int h,
                                      int w, double epsilon, int neg_psnr, float* values, float* sample_means, vfi_strides sd,
                                      vfi_strides sf, vfi_strides si, vfi_stream_t stream) {
    const bool flows = flow0 != nullptr;
    LossShape s;
    if (!diffs || !values || !sample_means || (flow0 == nullptr) != (flow1 == nullptr)) return VFI_ERR_SHAPE;
    if (flows && (!img0 || !img1)) return VFI_ERR_SHAPE;
    if (!loss_shape(nd, batch, cd, ci, h, w, flows, epsilon, &s)) return VFI_ERR_SHAPE;
    LossDiffs d = {};
    bool vd = w % 4 == 0 && vec_ok(target, sd, batch, cd, h);
    for (int i = 0; i < nd; ++i) {
        if (!diffs[i]) return VFI_ERR_SHAPE;
        d.p[i] = diffs[i];
        vd = vd && vec_ok(diffs[i], sd, batch, cd, h);
    }
    const bool vf = w % 4 == 0 && vec_ok(flow0, sf, batch, 2, h) && vec_ok(flow1, sf, batch, 2, h) &&
                    vec_ok(img0, si, batch, ci, h) && vec_ok(img1, si, batch, ci, h);
    const int64_t ndiff = (int64_t)nd * batch * s.diff_blocks, nflow = (int64_t)batch * s.flow_blocks;
    hipStream_t st = (hipStream_t)stream;
    double* partial = static_cast<double*>(ws_get(st, WS_LOSS, (size_t)(ndiff + 3 * nflow) * sizeof(double), false, nullptr));
    if (!partial) return VFI_ERR_LAUNCH;
    LOSS_LAUNCH(loss_forward, vd, vf, dim3((unsigned)(ndiff + nflow)), dim3(LOSS_THREADS), 0, st, d, target, flow0, flow1, img0, img1,
                s, sd, sf, si, partial);
    hipLaunchKernelGGL(loss_finish, dim3((unsigned)(nd + 1)), dim3(LOSS_FINISH_THREADS), 0, st, partial, s, neg_psnr ? 1 : 0, values,
                       sample_means);
    return launch_status();
}

extern "C" int vfi_part_loss_backward(const float* const* diffs, int nd, const float* target, const float* flow0,
                                       const float* flow1, const float* img0, const float* img1, int batch, int cd, int ci, int h,
                                       int w, double epsilon, int neg_psnr, const float* grad_values, const float* sample_means,
                                       unsigned int loss_mask, float* const* grad_diffs, float* grad_flow0, float* grad_flow1,
                                       vfi_strides sd, vfi_strides sf, vfi_strides si, vfi_strides sgd, vfi_strides sgf,
                                       vfi_stream_t stream) {
    const bool flows = flow0 != nullptr;
    LossShape s;
    if (!diffs || !grad_values || (flow0 == nullptr) != (flow1 == nullptr)) return VFI_ERR_SHAPE;
    if (flows && (!img0 || !img1)) return VFI_ERR_SHAPE;
    if (!flows && (grad_flow0 || grad_flow1)) return VFI_ERR_SHAPE;
    if (neg_psnr && !sample_means) return VFI_ERR_SHAPE;
    if (!loss_shape(nd, batch, cd, ci, h, w, flows, epsilon, &s)) return VFI_ERR_SHAPE;
    LossDiffs d = {};
    LossGrads g = {};
    LossBwdJobs jobs = {};
    jobs.mask = loss_mask;
    bool vd = w % 4 == 0 && vec_ok(target, sd, batch, cd, h);
    const int64_t diff_job_blocks = ((int64_t)batch * cd * h * s.units + LOSS_DIFF_BLOCK_UNITS - 1) / LOSS_DIFF_BLOCK_UNITS;
    int64_t blocks = 0;
    for (int i = 0; i < nd; ++i) {
        if (!diffs[i]) return VFI_ERR_SHAPE;
        d.p[i] = diffs[i];
        if (!grad_diffs || !grad_diffs[i]) continue;
        g.p[i] = grad_diffs[i];
        vd = vd && vec_ok(diffs[i], sd, batch, cd, h) && vec_ok(grad_diffs[i], sgd, batch, cd, h);
        jobs.first[jobs.njobs] = (int)blocks;
        jobs.tensor[jobs.njobs++] = i;
        blocks += diff_job_blocks;
        if (blocks >= ((int64_t)1 << 31)) return VFI_ERR_SHAPE;
    }
    jobs.first[jobs.njobs] = (int)blocks;
    const bool flow_job = grad_flow0 || grad_flow1;
    bool vf = false;
    if (flow_job) {
        blocks += ((int64_t)batch * h * s.units + LOSS_FLOW_BLOCK_UNITS - 1) / LOSS_FLOW_BLOCK_UNITS;
        if (blocks >= ((int64_t)1 << 31)) return VFI_ERR_SHAPE;
        vf = w % 4 == 0 && vec_ok(flow0, sf, batch, 2, h) && vec_ok(flow1, sf, batch, 2, h) && vec_ok(img0, si, batch, ci, h) &&
             vec_ok(img1, si, batch, ci, h) && vec_ok(grad_flow0, sgf, batch, 2, h) && vec_ok(grad_flow1, sgf, batch, 2, h);
    }
    if (blocks == 0) return VFI_OK;                          // nothing asked for
    LOSS_LAUNCH(loss_backward, vd, vf, dim3((unsigned)blocks), dim3(LOSS_THREADS), 0, (hipStream_t)stream, d, target, flow0, flow1,
                img0, img1, s, neg_psnr ? 1 : 0, grad_values, sample_means, jobs, g, grad_flow0, grad_flow1, sd, sf, si, sgd, sgf);
    return launch_status();
}
