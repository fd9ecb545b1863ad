// gradacc.hip -- see gradacc.h.
#include "gradacc.h"
#include "workspace.h"

namespace vfi {

// largest |element| of a [batch, channel, h, w] tensor into hdr[slot] (non-negative floats order like their bits); a NaN or an
// infinity raises hdr[1]
// G: a plain tensor (GradPlain) or the two terms of the blend backward's gradient (GradTerms, formed as its kernels form it)
template <class G>
__global__ __launch_bounds__(256) void gradacc_max(G g, int channel, int h, int w, vfi_strides sg, int64_t n,
                                                   int* __restrict__ hdr, int slot, int cells_log2) {
    int m = 0;
    bool bad = false;
    // a block per image row at a time: one set of divisions per row, consecutive lanes on consecutive elements
    const int rows = (int)(n / w);
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const int y = row % h, bc = row / h;
        const int c = bc % channel, b = bc / channel;
        const auto p = g.row((int64_t)b * sg.b + (int64_t)c * sg.c + (int64_t)y * sg.h);
        for (int x = threadIdx.x; x < w; x += 256) {
            const int bits = __float_as_int(fabsf(p[x]));
            bad = bad || bits >= 0x7f800000;                // infinity or NaN
            m = max(m, bits >= 0x7f800000 ? 0 : bits);
        }
    }
    // one atomic per block, and only from a block that raises the maximum: thousands of atomics on one word serialise
    // in L2 (measured: 0.2 ms per pass when every wave issued its own)
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
        if (m > __atomic_load_n(&hdr[slot], __ATOMIC_RELAXED)) atomicMax(&hdr[slot], m);
        if ((wbad[0] | wbad[1] | wbad[2] | wbad[3]) && !__atomic_load_n(&hdr[1], __ATOMIC_RELAXED)) atomicOr(&hdr[1], 1);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && slot == 0) hdr[3] = cells_log2;
}

// OVERWRITE: every cell of g1 is written (the blend backward's caller does not zero its gradient); else added into
template <bool OVERWRITE>
__global__ __launch_bounds__(256) void gradacc_convert(const unsigned long long* __restrict__ acc, const int* __restrict__ hdr,
                                                       float* __restrict__ g1, int channel, int h, int w, vfi_strides s1, int64_t n) {
    if (gradacc_fp32(hdr)) return;                          // the call scattered with fp32 atomics: nothing in the scratch
    const int k = gradacc_exponent(hdr);
    const int rows = (int)(n / w);
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const int y = row % h, bc = row / h;
        const int c = bc % channel, b = bc / channel;
        const unsigned long long* a = acc + (int64_t)row * w;
        float* cells = g1 + (int64_t)b * s1.b + (int64_t)c * s1.c + (int64_t)y * s1.h;
        for (int x = threadIdx.x; x < w; x += 256) {
            const long long sum = (long long)a[x];
            if constexpr (OVERWRITE) cells[x] = sum != 0 ? (float)ldexp((double)sum, -k) : 0.0f;    // (0 + v: the bits of v)
            else if (sum != 0) cells[x] += (float)ldexp((double)sum, -k);    // exact integer sum -> float once
        }
    }
}

// The sums of a bfloat16 gradient (gradacc.h): every cell of g1 written; a lane owns two adjacent cells (one 16-byte load of
// the sums, one 4-byte store where the pair is 4-byte aligned and inside the row).
__global__ __launch_bounds__(256) void gradacc_convert_bf16(const unsigned long long* __restrict__ acc, const int* __restrict__ hdr,
                                                            bf16_t* __restrict__ g1, int channel, int h, int w, vfi_strides s1, int64_t n) {
    const bool fp32 = gradacc_fp32(hdr);
    const int k = gradacc_exponent(hdr);
    const int rows = (int)(n / w);
    auto value = [&](unsigned long long cell) {
        if (fp32) return __uint_as_float((unsigned)cell);                   // (the float the atomics left in the low word)
        const long long sum = (long long)cell;
        return sum != 0 ? (float)ldexp((double)sum, -k) : 0.0f;
    };
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const int y = row % h, bc = row / h;
        const int c = bc % channel, b = bc / channel;
        const unsigned long long* a = acc + (int64_t)row * w;
        bf16_t* cells = g1 + (int64_t)b * s1.b + (int64_t)c * s1.c + (int64_t)y * s1.h;
        for (int x = 2 * threadIdx.x; x < w; x += 512) {
            const bool pair = x + 1 < w;
            const float lo = value(a[x]), hi = pair ? value(a[x + 1]) : 0.0f;
            bf16_store_pair(cells + x, bf16_pack_rne(lo, hi), pair);
        }
    }
}

// before an fp32 scatter into a gradient the caller has not zeroed: zero it (nothing to do on the integer path)
__global__ __launch_bounds__(256) void gradacc_zero_fp32_k(const int* __restrict__ hdr, float* __restrict__ g1, int channel, int h,
                                                           int w, vfi_strides s1, int64_t n) {
    if (!gradacc_fp32(hdr)) return;
    const int rows = (int)(n / w);
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const int y = row % h, bc = row / h;
        const int c = bc % channel, b = bc / channel;
        float* cells = g1 + (int64_t)b * s1.b + (int64_t)c * s1.c + (int64_t)y * s1.h;
        for (int x = threadIdx.x; x < w; x += 256) cells[x] = 0.0f;
    }
}

// Zero-fills the scratch in 16-byte units.  A kernel, not hipMemsetAsync: captured into a HIP graph with a whole training
// step, the memset nodes of the step's three gradacc calls held on the first replay and not on the second (the image
// gradients of the blend backward and of the second warp backward came out scaled by a stale header); a kernel node is
// ordered like the kernels around it.  The slot holds a multiple of 256 bytes (ws_get), so rounding up to 16 stays inside it.
__global__ __launch_bounds__(256) void gradacc_clear(uint4* __restrict__ p, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

int gradacc_reserve(hipStream_t st, int ndirs, int64_t cells, int nflags, GradAccScratch* s) {
    *s = GradAccScratch{};
    const GradAccLayout l = gradacc_layout((size_t)ndirs, (size_t)cells, (size_t)nflags);
    if (!l.bytes) return VFI_OK;
    size_t capacity = 0;
    char* p = static_cast<char*>(ws_get(st, WS_GRADACC, l.bytes, false, nullptr, &capacity));
    if (!p) return VFI_ERR_LAUNCH;
    const size_t n16 = (l.bytes + 15) / 16;
    if (n16 * 16 > capacity) return VFI_ERR_LAUNCH;
    const size_t blocks = (n16 + 255) / 256;
    hipLaunchKernelGGL(gradacc_clear, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, reinterpret_cast<uint4*>(p), n16);
    if (launch_status() != VFI_OK) return VFI_ERR_LAUNCH;
    for (int d = 0; d < ndirs; ++d)
        s->dir[d] = GradAccDir{reinterpret_cast<unsigned long long*>(p + l.acc[d]), reinterpret_cast<int*>(p + l.hdr[d])};
    if (nflags) s->flags = reinterpret_cast<int*>(p + l.flags);
    return VFI_OK;
}

// blocks of a row-walking kernel over `rows` image rows
static dim3 row_blocks(int64_t rows, int most) { return dim3((unsigned)(rows < most ? rows : most)); }

template <class G>
int gradacc_scan(hipStream_t st, G g, int batch, int channel, int h, int w, vfi_strides sg, const float* weights, int wchannel,
                 vfi_strides sw, int* hdr) {
    const int64_t n = (int64_t)batch * channel * h * w;
    // addends one cell can receive: every pixel of the frame, with every one of its taps -- border clamping can put all fs x fs
    // taps of a pixel (the four corners of a bilinear sample) on one cell (h w alone left (9/4) h w addends of
    // nearly 2^(62 - L) possible on a corner cell at fs = 6)
    const int64_t taps = wchannel > 4 ? wchannel : 4;
    int cells_log2 = 0;
    while (((int64_t)1 << cells_log2) < (int64_t)h * w * taps) ++cells_log2;
    hipLaunchKernelGGL(gradacc_max<G>, row_blocks(n / w, 2048), dim3(256), 0, st, g, channel, h, w, sg, n, hdr, 0, cells_log2);
    if (weights) {
        const int64_t nw = (int64_t)batch * wchannel * h * w;
        hipLaunchKernelGGL(gradacc_max<GradPlain>, row_blocks(nw / w, 2048), dim3(256), 0, st, GradPlain{weights}, wchannel, h, w,
                           sw, nw, hdr, 2, cells_log2);
    }
    return launch_status();
}
template int gradacc_scan<GradPlain>(hipStream_t, GradPlain, int, int, int, int, vfi_strides, const float*, int, vfi_strides, int*);
template int gradacc_scan<GradBf16>(hipStream_t, GradBf16, int, int, int, int, vfi_strides, const float*, int, vfi_strides, int*);
template int gradacc_scan<GradTerms>(hipStream_t, GradTerms, int, int, int, int, vfi_strides, const float*, int, vfi_strides, int*);

int gradacc_begin(hipStream_t st, const float* gout, int batch, int channel, int h, int w, vfi_strides sg,
                  const float* weights, int wchannel, vfi_strides sw, int nflags, GradAccScratch* s) {
    const int err = gradacc_reserve(st, 1, (int64_t)batch * channel * h * w, nflags, s);
    if (err != VFI_OK) return err;
    return gradacc_scan(st, GradPlain{gout}, batch, channel, h, w, sg, weights, wchannel, sw, s->dir[0].hdr);
}

int gradacc_begin_bf16(hipStream_t st, const bf16_t* gout, int batch, int channel, int h, int w, vfi_strides sg, int taps,
                       GradAccScratch* s) {
    const int err = gradacc_reserve(st, 1, (int64_t)batch * channel * h * w, 0, s);
    if (err != VFI_OK) return err;
    return gradacc_scan(st, GradBf16{gout}, batch, channel, h, w, sg, nullptr, taps, sg, s->dir[0].hdr);
}

int gradacc_finish_bf16(hipStream_t st, const GradAccDir& d, bf16_t* g1, int batch, int channel, int h, int w, vfi_strides s1) {
    const int64_t n = (int64_t)batch * channel * h * w;
    hipLaunchKernelGGL(gradacc_convert_bf16, row_blocks(n / w, 8192), dim3(256), 0, st, d.acc, d.hdr, g1, channel, h, w, s1, n);
    return launch_status();
}

int gradacc_zero_fp32(hipStream_t st, const int* hdr, float* g1, int batch, int channel, int h, int w, vfi_strides s1) {
    const int64_t n = (int64_t)batch * channel * h * w;
    hipLaunchKernelGGL(gradacc_zero_fp32_k, row_blocks(n / w, 2048), dim3(256), 0, st, hdr, g1, channel, h, w, s1, n);
    return launch_status();
}

int gradacc_finish(hipStream_t st, const GradAccDir& d, float* g1, int batch, int channel, int h, int w, vfi_strides s1,
                   bool overwrite) {
    const int64_t n = (int64_t)batch * channel * h * w;
    const auto convert = !overwrite ? gradacc_convert<false> : gradacc_convert<true>;
    hipLaunchKernelGGL(convert, row_blocks(n / w, 8192), dim3(256), 0, st, d.acc, d.hdr, g1, channel, h, w, s1, n);
    return launch_status();
}

}  // namespace vfi
