// filterinterp_multi.hip -- FilterInterpolation (_ori, fs == 4) forward of ONE image with SEVERAL flows at once.
//
// DAIN_slowmotion warps the same 196-channel context tensor with the same filter once per time offset
// (networks/DAIN_slowmotion.py:167-183 calls FilterInterpolate_ctx, :311-317, for t = 0.25, 0.5, 0.75: three
// FilterInterpolationModule calls per direction that differ in the flow only).  Each of those calls streams the
// whole tensor: the single-flow kernel (filterinterp_lds.hip) sits on the HBM ceiling, because a tile's window
// rows drag in the 128-byte lines they share with the neighbouring tiles (profiles/README.md: 1.8 x the
// algorithmic bytes leave the memory side).  Here a tile stages ONE window per channel -- the bounding box of the
// taps of both flows; the flows of a slow-motion step are scaled copies of each other, so it is only a few
// pixels larger than each flow's own window -- and produces two outputs from it.  Per output: half the window
// traffic, the same LDS reads and arithmetic.  Semantics per output: filterinterpolation_cuda_kernel.cu:2692-2823,
// bit for bit the single-flow kernel's (same taps, same order).
//
// Tiling, LDS-DMA ring, counted vmcnt and tile -> XCD grouping: exactly filterinterp_lds.hip (see there and
// filterinterp_dev.h); a thread owns two pixels, each with two (validity, window address, blend weights) and one set of
// 16 filter taps.
//
// Round 4: the window is staged as PAIRS.  With two outputs per staged window the launch is bound by its consumer side --
// LDS tap reads and vector issue (profiles/: three times the single-flow kernel's LDS cycles for one window's staging) --
// not by memory.  A tap row of the single-flow kernel is two ds_read2_b32 (columns (0, 2) and (1, 3), so that one packed
// multiply-add advances the left and the right quadrant sum): 128 B/clk.  Here the slot holds P[r][c] = (A[r][c], A[r][c + 2])
// as one 8-byte element, so the same two register pairs are two ds_read_b64 at P[c], P[c + 1] -- 8-byte aligned for every
// c, 256 B/clk, 64 banks (a stretching flow has slack).  The LDS-DMA writes consecutive dwords, so lane 2i of a staging
// instruction fetches column i and lane 2i + 1 column i + 2: every window element is staged twice (from L2 the second
// time), which the two outputs per window pay for.  The four blend weights of an evaluation are formed once per tile
// (blend4's own products: same bits) instead of once per channel.
#include "filterinterp_dev.h"
#include "filterinterp_paths.h"

namespace vfi {

#define FM_TW 64
#define FM_TH 16
#define FM_PX 2
#define FM_THREADS (FM_TW * FM_TH / FM_PX)          // 512
#define FM_PASS_ROWS (FM_TH / FM_PX)
#define FM_HDR 16
#define FM_RING_FLOATS 20464                        // with the header: 81,920 B = half of a CU's 160 KB (two workgroups per CU)
#define FM_RMAX 5
#define FM_KTOP 15                                  // staged dwords per thread and channel, at most
#define FM_KPAIR 18                                 // ... of a window staged as pairs: classes 3 x 3 ... 3 x 6, 4 x 3, 4 x 4
#define FM_NT 2                                     // flows per launch (three flows go as 2 + 1: see the host)

struct FmPtrs { const float* flow[FM_NT]; float* out[FM_NT]; };

struct FmWindow { int bx0, by0, bwp, bh, pitch, h, w, hs; };    // bwp / pitch: staged columns (pairs: bw - 2) and row pitch, in pairs / dwords
struct FmPixel {
    bool inimg;
    unsigned pix;           // element offset of the pixel inside an image plane
    float f[16];
    bool valid[FM_NT];
    float alpha[FM_NT], beta[FM_NT];
    int lbase[FM_NT];       // pair index of the 4x4 window origin of flow t inside the staged window
};

// Channel loop of one workgroup on a window staged as pairs, written like fi_run_channels_lean (filterinterp_lds.hip): ring
// geometry a compile-time function of the window class and one constant s_waitcnt in the steady state, running plane pointers,
// tap reads as asm (8-byte pairs, see the head of the file) at immediate offsets from one address per evaluation, with one
// lgkmcnt wait per half evaluation and the next half's rows in flight under the current one's arithmetic, range-checked buffer
// stores.  An evaluation = one pixel under one flow: 2 x FM_NT per thread and channel, each 8 LDS reads, 8 packed multiply-adds
// and the 4 operations of the blend.
// Window class <S, KR>: row pitch = 32 S pairs = S segments of 64 dwords, at most 8 KR rows.  A staging instruction writes one
// segment (64 consecutive dwords: what an LDS-DMA writes); wave v stages rows v, v + 8, ... whole: its KR x S instructions
// share S per-lane column offsets (the lane's column inside segment s, clamped to the frame; out of range for pad pairs) and
// take the row from the scalar offset operand -- S registers of addressing instead of one per staged dword (K = S KR = 9 ...
// 18), which is what lets a window of 96 x 48 pairs live beside the evaluations' state in 128 registers.  Rows past the
// window are staged through a descriptor of zero records: no memory traffic, and no address is formed from their offsets.
// Destination: ooff = the element offset of this batch item inside every output tensor, FI_CSO (filterinterp_dev.h) = the distance of its planes;
// the dense call passes the image's own (b * s1.b, cs).
template <int S, int KR, bool TO>
__device__ __forceinline__ void fm_run_channels(const float* __restrict__ img, const FmPtrs& ptr, int64_t ooff, int64_t cs,
                                                int64_t cso_to, int c_begin, int c_end, int tid, const FmWindow& win,
                                                const FmPixel (&px)[FM_PX], float* __restrict__ ring) {
    typedef float v2f __attribute__((ext_vector_type(2)));
    constexpr int K = S * KR;                               // staging instructions per wave and channel
    constexpr int NP = K * FM_THREADS;                      // dwords per ring slot
    constexpr int R = (FM_RING_FLOATS / NP) < FM_RMAX ? (FM_RING_FLOATS / NP) : FM_RMAX;
    constexpr int D = R - 1;
    constexpr int NE = FM_PX * FM_NT;                           // evaluations per thread and channel, e = t * FM_PX + p
    constexpr int PITCH8 = 256 * S;                          // row pitch in bytes
    static_assert(D >= 1 && D <= 4 && (D - 1) * K <= 63, "ring geometry");
    static_assert(3 * PITCH8 + 8 < 65536, "tap rows at immediate offsets");
    // the ds_read_b64 tap reads: the LDS array is 16-byte aligned, and every byte offset added to it is a multiple of 8
    static_assert((FM_HDR * 4) % 8 == 0 && (NP * 4) % 8 == 0 && PITCH8 % 8 == 0, "8-byte tap reads stay 8-byte aligned");
    if (c_begin >= c_end) return;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // lane's dword inside segment s: half (lane & 1) of pair column 32 s + lane / 2
    unsigned voff[S];
#pragma unroll
    for (int s_ = 0; s_ < S; ++s_) {
        const int colp = 32 * s_ + (lane >> 1);
        voff[s_] = colp < win.bwp ? 4u * (unsigned)clampi(win.bx0 + colp + 2 * (lane & 1), 0, win.w - 1) : 0x80000000u;
    }
    const int plane_bytes = 4 * ((win.h - 1) * win.hs + win.w);
    const unsigned ring_lds = (unsigned)(uintptr_t)(lds_ptr_t)ring;
    unsigned lb[NE], pix4[FM_PX];
    float W[NE][4];                                          // blend4's weights of an evaluation: (1-a)(1-b), a(1-b), (1-a)b, ab
#pragma unroll
    for (int t = 0; t < FM_NT; ++t)
#pragma unroll
        for (int p = 0; p < FM_PX; ++p) {
            const int e = t * FM_PX + p;
            lb[e] = ring_lds + 8u * (unsigned)px[p].lbase[t];                   // (an invalid evaluation's reads land anywhere: discarded)
            pix4[p] = 4u * px[p].pix;
            const float al = px[p].alpha[t], be = px[p].beta[t];
            W[e][0] = (1.0f - al) * (1.0f - be); W[e][1] = al * (1.0f - be); W[e][2] = (1.0f - al) * be; W[e][3] = al * be;
        }
    // filter taps as (left quadrant, right quadrant) pairs: rows 0-1 feed the top sums, rows 2-3 the bottom ones
    v2f F[FM_PX][8];
#pragma unroll
    for (int p = 0; p < FM_PX; ++p)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            F[p][2 * r] = v2f{px[p].f[4 * r], px[p].f[4 * r + 2]};
            F[p][2 * r + 1] = v2f{px[p].f[4 * r + 1], px[p].f[4 * r + 3]};
        }
    const int last = c_end - 1;
    const float* pdma = img + (int64_t)c_begin * cs;
    int64_t oofs = ooff + (int64_t)c_begin * FI_CSO;           // element offset of the output plane inside every output tensor
    auto issue = [&](int slot) {
        float* l = ring + slot * NP + wave * (64 * S);
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            const int row = wave + 8 * k;                                       // (scalar)
            const bool live = row < win.bh;
            // (a row past the window: zero records -- every offset out of range)
            const auto plane = buffer_rsrc(pdma, live ? plane_bytes : 0);
            const int soff = live ? 4 * clampi(win.by0 + row, 0, win.h - 1) * win.hs : 0;
#pragma unroll
            for (int s_ = 0; s_ < S; ++s_)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(plane, (lds_ptr_t)(l + (8 * k * S + s_) * 64), 4, voff[s_], soff, 0, 0);
        }
        pdma += cs;
    };
#define FM_READ_ROW(d0, d1, addr, r) do { \
        asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(d0) : "v"(addr), "n"((r) * PITCH8)); \
        asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(d1) : "v"(addr), "n"((r) * PITCH8 + 8)); } while (0)
    auto compute = [&](int slot) {
        const unsigned so = (unsigned)(slot * (NP * 4));
        // Tap reads ping-pong between two register sets, half an evaluation per set: while the top sums of evaluation e are
        // formed from rows 0-1 (set 0), rows 2-3 (set 1) are in flight, and so on.  (A whole evaluation per set, 16 LDS reads
        // in flight, measured 3.5 % slower: 1.66 against 1.60 ms per two-flow launch at 1080p, C = 196.)
        using I0 = std::integral_constant<int, 0>;
        using I1 = std::integral_constant<int, 1>;
        using I4 = std::integral_constant<int, 4>;
        auto finish = [&](auto E, const v2f& top, const v2f& bot) {
            constexpr int e = decltype(E)::value, t = e / FM_PX, p = e % FM_PX;
            float val = W[e][0] * top.x;                    // (blend4, its weights formed above)
            val = fmaf(W[e][1], top.y, val);
            val = fmaf(W[e][2], bot.x, val);
            val = fmaf(W[e][3], bot.y, val);
            const auto oplane = buffer_rsrc(ptr.out[t] + oofs, plane_bytes);
            // an invalid evaluation's store is dropped by the range check.  (The select is formed here, from a validity mask
            // the compiler keeps in scalar registers: loop-invariant offsets per evaluation instead of per pixel cost registers.)
            unsigned po = pix4[p];
            asm volatile("" : "+v"(po));
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(val), oplane, px[p].valid[t] ? po : 0x80000000u, 0, 0);
        };
        v2f q[2][4];
        unsigned adr[2];
        auto reads = [&](auto E, auto H) {                   // rows 2h, 2h + 1 of evaluation e into set h
            constexpr int e = decltype(E)::value, h = decltype(H)::value;
            v2f (&d)[4] = q[h];
            if constexpr (h == 0) adr[e & 1] = lb[e] + so;
            const unsigned a = adr[e & 1];
            FM_READ_ROW(d[0], d[1], a, 2 * h);
            FM_READ_ROW(d[2], d[3], a, 2 * h + 1);
        };
        auto landed = [&](v2f (&d)[4], auto LATER) {         // all but the `later` youngest LDS reads are back
            asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]) : "n"(decltype(LATER)::value));
        };
        reads(I0{}, I0{}); reads(I0{}, I1{});
        static_for<0, NE>([&](auto E) {
            constexpr int e = decltype(E)::value, p = e % FM_PX;
            // d[2r] = columns (0, 2), d[2r + 1] = columns (1, 3) of row r: the sums of fi4_pixel, two quadrants per instruction
            landed(q[0], I4{});
            v2f top = q[0][0] * F[p][0];
            top = __builtin_elementwise_fma(q[0][1], F[p][1], top);
            top = __builtin_elementwise_fma(q[0][2], F[p][2], top);
            top = __builtin_elementwise_fma(q[0][3], F[p][3], top);
            if constexpr (e + 1 < NE) { reads(std::integral_constant<int, e + 1>{}, I0{}); landed(q[1], I4{}); }
            else landed(q[1], I0{});
            v2f bot = q[1][0] * F[p][4];
            bot = __builtin_elementwise_fma(q[1][1], F[p][5], bot);
            bot = __builtin_elementwise_fma(q[1][2], F[p][6], bot);
            bot = __builtin_elementwise_fma(q[1][3], F[p][7], bot);
            if constexpr (e + 1 < NE) reads(std::integral_constant<int, e + 1>{}, I1{});
            finish(E, top, bot);
        });
        oofs += FI_CSO;
    };
#undef FM_READ_ROW
    // The steady-state wait.  vmcnt counts the staging loads AND the NE result stores of every step, in issue order (one counter
    // on gfx9).  Behind the loads of window c + 1 the stream holds, at the end of step c: the stores of the step that issued
    // them, then D - 1 steps of K loads + NE stores.  Rounds 3-4 waited for vmcnt <= (D - 1) K -- with the stores in the counter
    // that asks for part of window c + 2 as well, and with two ring slots (D = 1) for every store of the step itself.  The
    // prologue puts NE stores whose offsets are out of range behind each of its windows, so that the first steps see the same
    // stream as the later ones.  (In-kernel stamps had a quarter of a step in this wait.)
    constexpr int NWAIT = (D - 1) * (K + NE) + NE;
    static_assert(NWAIT <= 63, "vmcnt is six bits");
    const int n0 = min(D, c_end - c_begin);
    {
        const auto nowhere = buffer_rsrc(img, 0);      // (zero records: every offset out of range)
        for (int j = 0; j < n0; ++j) {
            issue(j);
#pragma unroll
            for (int e = 0; e < NE; ++e) __builtin_amdgcn_raw_buffer_store_b32(0u, nowhere, 0x80000000u, 0, 0);
        }
    }
    wait_windows<K>(n0 - 1);                                    // the first window has landed ...
    __builtin_amdgcn_s_barrier();                               // ... in every wave
    int c = c_begin, slot = 0;
    for (; c + D <= last; ++c) {                                // steady state: window c + D exists
        issue(slot == 0 ? R - 1 : slot - 1);                    // into the slot every wave finished reading before the last barrier
        compute(slot);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NWAIT) : "memory");            // window c + 1 has landed
        __builtin_amdgcn_s_barrier();
        slot = (slot + 1 == R) ? 0 : slot + 1;
    }
    for (; c <= last; ++c) {                                    // the last D channels: nothing left to stage
        compute(slot);
        if (c < last) {
            // behind the loads of window c + 1: m windows (m = last - c - 1 <= D - 2) and the stores of D steps -- provided
            // window c + 1 was staged by a step of the loop above (a channel range shorter than the ring waits for everything)
            const int m = last - c - 1;
            if (c - c_begin < D - 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else if (m <= 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(D * NE < 63 ? D * NE : 63) : "memory");
            else if (m == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(K + D * NE < 63 ? K + D * NE : 63) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * K + D * NE < 63 ? 2 * K + D * NE : 63) : "memory");
            __builtin_amdgcn_s_barrier();
        }
        slot = (slot + 1 == R) ? 0 : slot + 1;
    }
    // copy-through of the invalid pixels (:2814-2818), outside the pipelined loop (written out: fi_copy_through changes this code)
#pragma unroll
    for (int t = 0; t < FM_NT; ++t)
#pragma unroll
        for (int p = 0; p < FM_PX; ++p)
            if (px[p].inimg && !px[p].valid[t])
                for (int cc = c_begin; cc < c_end; ++cc)
                    ptr.out[t][ooff + (int64_t)cc * FI_CSO + px[p].pix] = img[(int64_t)cc * cs + px[p].pix];
}

// The same loop on a PLAIN window (one dword per element, tap rows as two ds_read2_b32: rounds 2-3) -- for tiles whose window
// does not fit the ring as pairs (rough flow fields: a window of 98 x 50 elements is 12.5 dwords per thread plain, 25 as
// pairs).  Written like fi_run_channels_lean (filterinterp_lds.hip): ring geometry a compile-time function of K and one constant s_waitcnt in the steady state, running
// plane pointers, M0 formed on the scalar unit, tap reads as asm (columns (0, 2) / (1, 3) of a row, so that one packed
// multiply-add advances the left and the right quadrant sum) with one lgkmcnt wait per evaluation and the next evaluation's
// first rows in flight under the current one's arithmetic, range-checked buffer stores.  An evaluation = one pixel under
// one flow: 2 x FM_NT per thread and channel.
template <int K, bool TO>
__device__ __forceinline__ void fm_run_channels_plain(const float* __restrict__ img, const FmPtrs& ptr, int64_t ooff, int64_t cs,
                                                int64_t cso_to, int c_begin, int c_end, int tid, const FmWindow& win,
                                                const FmPixel (&px)[FM_PX], float* __restrict__ ring) {
    typedef float v2f __attribute__((ext_vector_type(2)));
    constexpr int NP = K * FM_THREADS;
    constexpr int R = (FM_RING_FLOATS / NP) < FM_RMAX ? (FM_RING_FLOATS / NP) : FM_RMAX;
    constexpr int D = R - 1;
    constexpr int NE = FM_PX * FM_NT;                           // evaluations per thread and channel, e = t * FM_PX + p
    static_assert(D >= 1 && D <= 4 && (D - 1) * K <= 63, "ring geometry");
    if (c_begin >= c_end) return;
    // staged element e = tid + k * FM_THREADS, row pitch a multiple of the 32 LDS banks, borders replicated while
    // staging, pad elements out of the buffer's range (they cost no memory traffic): filterinterp_lds.hip
    const float inv_pitch32 = 1.0f / (float)win.pitch;
    unsigned goff[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = tid + k * FM_THREADS;
        const int r = fi_row_of(e, inv_pitch32);
        const int col = e - r * win.pitch;
        const unsigned off = 4u * (unsigned)(clampi(win.by0 + r, 0, win.h - 1) * win.hs + clampi(win.bx0 + col, 0, win.w - 1));
        goff[k] = (col < win.bwp && r < win.bh) ? off : 0x80000000u;    // (bwp = the window width here)
    }
    const int plane_bytes = 4 * ((win.h - 1) * win.hs + win.w);
    const int wave_first = __builtin_amdgcn_readfirstlane(tid >> 6) * 64;
    const unsigned ring_lds = (unsigned)(uintptr_t)(lds_ptr_t)ring;
    const unsigned pitch4 = 4u * (unsigned)win.pitch;
    unsigned lb[NE], pix4[FM_PX];
#pragma unroll
    for (int t = 0; t < FM_NT; ++t)
#pragma unroll
        for (int p = 0; p < FM_PX; ++p) {
            lb[t * FM_PX + p] = ring_lds + 4u * (unsigned)px[p].lbase[t];       // (an invalid evaluation's reads land anywhere: discarded)
            pix4[p] = 4u * px[p].pix;
        }
    // filter taps as (left quadrant, right quadrant) pairs: rows 0-1 feed the top sums, rows 2-3 the bottom ones
    v2f F[FM_PX][8];
#pragma unroll
    for (int p = 0; p < FM_PX; ++p)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            F[p][2 * r] = v2f{px[p].f[4 * r], px[p].f[4 * r + 2]};
            F[p][2 * r + 1] = v2f{px[p].f[4 * r + 1], px[p].f[4 * r + 3]};
        }
    const int last = c_end - 1;
    const float* pdma = img + (int64_t)c_begin * cs;
    int64_t oofs = ooff + (int64_t)c_begin * FI_CSO;           // element offset of the output plane inside every output tensor
    auto issue = [&](int slot) {
        const auto plane = buffer_rsrc(pdma, plane_bytes);
        float* l = ring + slot * NP + wave_first;
#pragma unroll
        for (int k = 0; k < K; ++k)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(plane, (lds_ptr_t)(l + k * FM_THREADS), 4, goff[k], 0, 0, 0);
        pdma += cs;
    };
#define FM_READ2(dst, addr, o0, o1) asm volatile("ds_read2_b32 %0, %1 offset0:" #o0 " offset1:" #o1 : "=v"(dst) : "v"(addr))
    auto compute = [&](int slot) {
        const unsigned so = (unsigned)(slot * (NP * 4));
        constexpr bool OVERLAP = K <= 12;                   // (a second evaluation in flight costs 16 registers)
        v2f q[OVERLAP ? 2 : 1][8];
        auto reads = [&](auto E, auto H) {                   // rows 2h, 2h + 1 of evaluation e
            constexpr int e = decltype(E)::value, h = decltype(H)::value;
            v2f (&d)[8] = q[OVERLAP ? (e & 1) : 0];
            unsigned a = lb[e] + so + (h ? 2u * pitch4 : 0u);
            FM_READ2(d[4 * h], a, 0, 2); FM_READ2(d[4 * h + 1], a, 1, 3);
            a += pitch4;
            FM_READ2(d[4 * h + 2], a, 0, 2); FM_READ2(d[4 * h + 3], a, 1, 3);
        };
        using I0 = std::integral_constant<int, 0>;
        using I1 = std::integral_constant<int, 1>;
        reads(I0{}, I0{}); reads(I0{}, I1{});
        if constexpr (OVERLAP) reads(I1{}, I0{});
        static_for<0, NE>([&](auto E) {
            constexpr int e = decltype(E)::value, t = e / FM_PX, p = e % FM_PX;
            v2f (&d)[8] = q[OVERLAP ? (e & 1) : 0];
            asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]), "+v"(d[4]), "+v"(d[5]),
                                                    "+v"(d[6]), "+v"(d[7]) : "n"(OVERLAP && e + 1 < NE ? 4 : 0));
            v2f top = d[0] * F[p][0];                       // (same order per quadrant sum as fi4_pixel)
            top = __builtin_elementwise_fma(d[1], F[p][1], top);
            top = __builtin_elementwise_fma(d[2], F[p][2], top);
            top = __builtin_elementwise_fma(d[3], F[p][3], top);
            v2f bot = d[4] * F[p][4];
            bot = __builtin_elementwise_fma(d[5], F[p][5], bot);
            bot = __builtin_elementwise_fma(d[6], F[p][6], bot);
            bot = __builtin_elementwise_fma(d[7], F[p][7], bot);
            // (the four blend weights are formed here each time: kept across the loop for 2 x FM_NT evaluations they do not fit)
            float al = px[p].alpha[t], be = px[p].beta[t];
            asm volatile("" : "+v"(al), "+v"(be));
            const float val = blend4(al, be, top.x, top.y, bot.x, bot.y);
            const auto oplane = buffer_rsrc(ptr.out[t] + oofs, plane_bytes);
            unsigned po = pix4[p];                          // (an invalid evaluation's store is dropped by the range check)
            asm volatile("" : "+v"(po));
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(val), oplane, px[p].valid[t] ? po : 0x80000000u, 0, 0);
            if constexpr (OVERLAP) {
                if constexpr (e + 1 < NE) reads(std::integral_constant<int, e + 1>{}, I1{});
                if constexpr (e + 2 < NE) reads(std::integral_constant<int, e + 2>{}, I0{});
            } else if constexpr (e + 1 < NE) {
                reads(std::integral_constant<int, e + 1>{}, I0{}); reads(std::integral_constant<int, e + 1>{}, I1{});
            }
        });
        oofs += FI_CSO;
    };
#undef FM_READ2
    // (the steady-state wait counts the result stores in: see fm_run_channels)
    constexpr int NWAIT = (D - 1) * (K + NE) + NE;
    static_assert(NWAIT <= 63, "vmcnt is six bits");
    const int n0 = min(D, c_end - c_begin);
    {
        const auto nowhere = buffer_rsrc(img, 0);
        for (int j = 0; j < n0; ++j) {
            issue(j);
#pragma unroll
            for (int e = 0; e < NE; ++e) __builtin_amdgcn_raw_buffer_store_b32(0u, nowhere, 0x80000000u, 0, 0);
        }
    }
    wait_windows<K>(n0 - 1);                                    // the first window has landed ...
    __builtin_amdgcn_s_barrier();                               // ... in every wave
    int c = c_begin, slot = 0;
    for (; c + D <= last; ++c) {                                // steady state: window c + D exists
        issue(slot == 0 ? R - 1 : slot - 1);                    // into the slot every wave finished reading before the last barrier
        compute(slot);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NWAIT) : "memory");            // window c + 1 has landed
        __builtin_amdgcn_s_barrier();
        slot = (slot + 1 == R) ? 0 : slot + 1;
    }
    for (; c <= last; ++c) {                                    // the last D channels: nothing left to stage
        compute(slot);
        if (c < last) {
            // behind the loads of window c + 1: m windows (m = last - c - 1 <= D - 2) and the stores of D steps -- provided
            // window c + 1 was staged by a step of the loop above (a channel range shorter than the ring waits for everything)
            const int m = last - c - 1;
            if (c - c_begin < D - 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else if (m <= 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(D * NE < 63 ? D * NE : 63) : "memory");
            else if (m == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(K + D * NE < 63 ? K + D * NE : 63) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * K + D * NE < 63 ? 2 * K + D * NE : 63) : "memory");
            __builtin_amdgcn_s_barrier();
        }
        slot = (slot + 1 == R) ? 0 : slot + 1;
    }
    // copy-through of the invalid pixels (:2814-2818), outside the pipelined loop (written out: fi_copy_through changes this code)
#pragma unroll
    for (int t = 0; t < FM_NT; ++t)
#pragma unroll
        for (int p = 0; p < FM_PX; ++p)
            if (px[p].inimg && !px[p].valid[t])
                for (int cc = c_begin; cc < c_end; ++cc)
                    ptr.out[t][ooff + (int64_t)cc * FI_CSO + px[p].pix] = img[(int64_t)cc * cs + px[p].pix];
}

// DST = vfi_strides (fi_dst, filterinterp_dev.h): the outputs are addressed with so's batch and channel strides; no DST:
// with s1's
template <class... DST>
__global__ __launch_bounds__(FM_THREADS, 4) void fi_forward_ori_multi(
    const float* __restrict__ in1, FmPtrs ptr, const float* __restrict__ in3, int channel, int h, int w,
    vfi_strides s1, vfi_strides s2, vfi_strides s3, int tiles_x, int tiles_y, int ntiles, int ch_per_group, DST... so) {
    __shared__ __attribute__((aligned(16))) float lds[FM_HDR + FM_RING_FLOATS];
    int* box = reinterpret_cast<int*>(lds);

    // four horizontally consecutive tiles per XCD (fi_xcd_tile)
    const int tile = fi_xcd_tile<int>(blockIdx.x);
    if (tile >= ntiles) return;
    const FiTile tp = fi_tile_at(tile, tiles_x, tiles_y, channel, ch_per_group);
    const int b = tp.b, c_begin = tp.c_begin, c_end = tp.c_end;

    const int tid = threadIdx.x;
    const int x = tp.tx * FM_TW + (tid & (FM_TW - 1));
    const int y0 = tp.ty * FM_TH + (tid >> 6);

    const int flow_bytes = ((int)s2.c + (h - 1) * (int)s2.h + w) * 4;           // (the host checked that these fit 31 bits)
    const int filt_bytes = (15 * (int)s3.c + (h - 1) * (int)s3.h + w) * 4;
    FmPixel px[FM_PX];
    int L[FM_PX][FM_NT], T[FM_PX][FM_NT];
    float fxv[FM_PX][FM_NT], fyv[FM_PX][FM_NT];
    int bx_lo = INT_MAX, by_lo = INT_MAX, bx_hi = INT_MIN, by_hi = INT_MIN;
#pragma unroll
    for (int p = 0; p < FM_PX; ++p) {
        const int y = y0 + p * FM_PASS_ROWS;
        px[p].inimg = x < w && y < h;
        px[p].pix = (unsigned)(y * (int)s1.h + x);
#pragma unroll
        for (int k = 0; k < 16; ++k) px[p].f[k] = 0.0f;
#pragma unroll
        for (int t = 0; t < FM_NT; ++t) fxv[p][t] = fyv[p][t] = 0.0f;
        if (px[p].inimg) {
            // (buffer loads: a uniform descriptor per tensor, a 32-bit byte offset per pixel, the plane's offset scalar)
            const int fo = (y * (int)s2.h + x) * 4, ko = (y * (int)s3.h + x) * 4;
#pragma unroll
            for (int t = 0; t < FM_NT; ++t) {
                const auto fr = buffer_rsrc(ptr.flow[t] + (int64_t)b * s2.b, flow_bytes);
                fxv[p][t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(fr, fo, 0, 0));
                fyv[p][t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(fr, fo, (int)s2.c * 4, 0));
            }
            const auto kr = buffer_rsrc(in3 + (int64_t)b * s3.b, filt_bytes);
#pragma unroll
            for (int k = 0; k < 16; ++k) px[p].f[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(kr, ko, k * (int)s3.c * 4, 0));
        }
    }
#pragma unroll
    for (int p = 0; p < FM_PX; ++p) {
        const int y = y0 + p * FM_PASS_ROWS;
#pragma unroll
        for (int t = 0; t < FM_NT; ++t) {
            const FiGeom g = fi_geom(fxv[p][t], fyv[p][t], x, y, w, h, px[p].inimg);
            px[p].valid[t] = g.valid;
            L[p][t] = g.ix - 1; T[p][t] = g.iy - 1;         // ix + 1 - fs/2, fs == 4
            px[p].alpha[t] = g.alpha; px[p].beta[t] = g.beta;
            fi_box_add4(g.valid, L[p][t], T[p][t], bx_lo, by_lo, bx_hi, by_hi);
        }
    }

    // ---- bounding box of every tap of the tile, all flows
    if (tid == 0) fi_box_clear(box);
    __syncthreads();
    const bool any_valid = fi_box_fold(box, tid, bx_lo, by_lo, bx_hi, by_hi);
    const int bx0 = box[0], by0 = box[1];
    const int bw = any_valid ? box[2] - bx0 + 1 : 0;
    const int bh = any_valid ? box[3] - by0 + 1 : 0;
    // the slot holds pairs (column c, column c + 2): bw - 2 of them per row, pitch a multiple of 32 pairs; a window too large
    // for that is staged plain (pitch a multiple of 32 dwords)
    const int bwp = any_valid ? bw - 2 : 0;
    const int segs = max(3, (bwp + 31) >> 5);                // S: segments of 32 pairs per row (a narrow window takes the class of 3)
    const int rows8 = max(3, (bh + 7) >> 3);                 // KR: rows per staging wave
    const bool paired = segs <= 4 && segs * rows8 <= FM_KPAIR;
    const int pitch = paired ? 32 * segs : (bw + 31) & ~31;
    const int n = paired ? 0 : pitch * bh;                   // dwords of a plain window
#pragma unroll
    for (int p = 0; p < FM_PX; ++p)
#pragma unroll
        for (int t = 0; t < FM_NT; ++t) px[p].lbase[t] = (T[p][t] - by0) * pitch + (L[p][t] - bx0);

    const int64_t boff = (int64_t)b * s1.b;
    constexpr bool TO = sizeof...(DST) != 0;
    int64_t ooff = boff, oc = s1.c;
    if constexpr (TO) { ooff = (int64_t)b * fi_dst(s1, so...).b; oc = fi_dst(s1, so...).c; }
    const float* img = in1 + boff;
    const int kmax = (n + FM_THREADS - 1) / FM_THREADS;
    if (kmax > FM_KTOP) {
        // window too large for LDS: gather from global memory (workgroup-uniform branch)
#pragma unroll
        for (int t = 0; t < FM_NT; ++t)
#pragma unroll
            for (int p = 0; p < FM_PX; ++p) {
                float* dst = ptr.out[t] + ooff;
                if (px[p].valid[t]) {
                    fi4_channels_direct<TO>(img, dst + px[p].pix, c_begin, c_end, s1.c, oc, (int)s1.h, h, w, L[p][t], T[p][t], px[p].f,
                                        px[p].alpha[t], px[p].beta[t]);
                } else if (px[p].inimg) {
                    fi_copy_through_to<TO>(img, dst, px[p].pix, c_begin, c_end, s1.c, oc);
                }
            }
        return;
    }

    const FmWindow win{bx0, by0, paired ? bwp : bw, bh, pitch, h, w, (int)s1.h};
    float* ring = lds + FM_HDR;
#define FM_RUN(S, KR) fm_run_channels<S, KR, TO>(img, ptr, ooff, s1.c, oc, c_begin, c_end, tid, win, px, ring)
#define FM_RUN_PLAIN(K) fm_run_channels_plain<K, TO>(img, ptr, ooff, s1.c, oc, c_begin, c_end, tid, win, px, ring)
    if (paired) {
        if (segs == 3) {
            if (rows8 == 3) FM_RUN(3, 3);
            else if (rows8 == 4) FM_RUN(3, 4);
            else if (rows8 == 5) FM_RUN(3, 5);
            else FM_RUN(3, 6);
        } else {
            if (rows8 == 3) FM_RUN(4, 3);
            else FM_RUN(4, 4);
        }
    } else {
        if (kmax <= 8) FM_RUN_PLAIN(8);
        else if (kmax <= 10) FM_RUN_PLAIN(10);
        else if (kmax <= 12) FM_RUN_PLAIN(12);
        else FM_RUN_PLAIN(15);
    }
#undef FM_RUN_PLAIN
#undef FM_RUN
}

}  // namespace vfi

using namespace vfi;

static int forward_ori_multi_to(const float* input1, const float* const* flows, const float* input3, float* const* outputs,
                                int nflows, int batch, int channel, int h, int w, int filter_channels, vfi_strides s1,
                                vfi_strides s2, vfi_strides s3, vfi_strides so, vfi_stream_t stream) {
    if (nflows <= 0 || !flows || !outputs || batch <= 0 || channel <= 0 || h <= 0 || w <= 0 || filter_channels <= 0)
        return VFI_ERR_SHAPE;
    if (!input1 || !input3) return VFI_ERR_SHAPE;
    for (int t = 0; t < nflows; ++t)
        if (!flows[t] || !outputs[t]) return VFI_ERR_SHAPE;
    // the destinations' rows are input1's rows: one in-plane offset per pixel for loads and stores (never a slower kernel)
    if (so.h != s1.h) return VFI_ERR_SHAPE;
    // more flows than one launch takes: pairs, and an odd flow alone.  (Round 4: a three-flow launch was slower than 2 + 1 --
    // 3.01 against 2.78 ms at 1080p, C = 196: the union window of three time offsets cost it its ring depth.)
    if (nflows > FM_NT) {
        for (int t0 = 0; t0 < nflows; t0 += FM_NT) {
            const int n = nflows - t0 < FM_NT ? nflows - t0 : FM_NT;
            const int err = forward_ori_multi_to(input1, flows + t0, input3, outputs + t0, n, batch, channel, h, w,
                                                 filter_channels, s1, s2, s3, so, stream);
            if (err != VFI_OK) return err;
        }
        return VFI_OK;
    }
    // the shared-window kernel: fs == 4, two flows, in-plane byte offsets within 32 bits; anything else (one flow among
    // them) is the single-flow entry point once per flow (same results)
    const bool staged = filter_channels == 16 && nflows == FM_NT && (int64_t)h * s1.h * 4 <= INT_MAX &&
                        s2.c >= 0 && s3.c >= 0 && (s2.c + (int64_t)h * s2.h) * 4 <= INT_MAX && (15 * s3.c + (int64_t)h * s3.h) * 4 <= INT_MAX;
    if (!staged) {
        for (int t = 0; t < nflows; ++t) {
            const int err = fi_forward_ori_to(input1, flows[t], input3, outputs[t], batch, channel, h, w, filter_channels,
                                              s1, s2, s3, so, stream);
            if (err != VFI_OK) return err;
        }
        return VFI_OK;
    }
    const int tiles_x = (w + FM_TW - 1) / FM_TW, tiles_y = (h + FM_TH - 1) / FM_TH;
    const int64_t nt = (int64_t)tiles_x * tiles_y * batch;
    if (nt > (1 << 28)) return VFI_ERR_SHAPE;
    const int ntiles = (int)nt;
    // (one prologue for nflows outputs per channel)
    const FiSplit split = fi_channel_split(ntiles, channel, 4.3 * (1.0 + 0.3 * (nflows - 1)) / nflows);
    FmPtrs ptr;
    for (int t = 0; t < FM_NT; ++t) { ptr.flow[t] = flows[t]; ptr.out[t] = outputs[t]; }
    const dim3 grid((unsigned)fi_xcd_grid(ntiles), (unsigned)split.groups, 1), block(FM_THREADS, 1, 1);
    // (every store is a single dword: the destinations need a float's alignment and no more.  Destinations laid out as
    //  input1 take the instance without a second set of strides: the code it always was.)
    if (so.b != s1.b || so.c != s1.c)
        hipLaunchKernelGGL(fi_forward_ori_multi<vfi_strides>, grid, block, 0, (hipStream_t)stream, input1, ptr, input3, channel, h,
                           w, s1, s2, s3, tiles_x, tiles_y, ntiles, split.ch_per_group, so);
    else
        hipLaunchKernelGGL(fi_forward_ori_multi<>, grid, block, 0, (hipStream_t)stream, input1, ptr, input3, channel, h, w, s1,
                           s2, s3, tiles_x, tiles_y, ntiles, split.ch_per_group);
    return launch_status();
}

extern "C" int vfi_filterinterp_forward_ori_multi(const float* input1, const float* const* flows, const float* input3,
                                                   float* const* outputs, int nflows, int batch, int channel, int h, int w,
                                                   int filter_channels, vfi_strides s1, vfi_strides s2, vfi_strides s3,
                                                   vfi_stream_t stream) {
    return forward_ori_multi_to(input1, flows, input3, outputs, nflows, batch, channel, h, w, filter_channels, s1, s2, s3, s1,
                                stream);
}

extern "C" int vfi_filterinterp_forward_ori_multi_to(const float* input1, const float* const* flows, const float* input3,
                                                      float* const* outputs, int nflows, int batch, int channel, int h, int w,
                                                      int filter_channels, vfi_strides s1, vfi_strides s2, vfi_strides s3,
                                                      vfi_strides s_out, vfi_stream_t stream) {
    return forward_ori_multi_to(input1, flows, input3, outputs, nflows, batch, channel, h, w, filter_channels, s1, s2, s3, s_out,
                                stream);
}
