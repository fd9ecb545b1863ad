// correlation_bwd_k1.inc -- the statements of the tiled correlation backward for every storage type whose sums are float
// (correlation_bwd.h: corr_backward_k1_body), included where A (CorrF32, CorrBf16), SECOND, Act, win (CorrBwdWindow), t
// (CorrBwdTile), other, gout, gin, channel, h, w and act are in scope: in corr_backward_k1_body, which the pair kernels and
// the float32 single kernels call, and in the bfloat16 single-gradient kernel corr_backward_k1_bf16.  The text is shared
// as well as the function because the bfloat16 single-gradient kernels compiled through the function came out slower
// (another interleaving of the window reads with the multiply-adds, 130 instead of 124 registers in one instance:
// DESIGN.md 4.3a-6); included in the kernel they are the instructions they were.
    typedef CorrBwdTile T;
    constexpr int MD = T::MD, D = T::D, OC = T::OC;
    const int tid = threadIdx.x, px = tid & 63, py = tid >> 6;
    const int bx = t.x0 + px, by = t.y0 + py;
    const int n = t.n, c_begin = t.c_begin, c_end = t.c_end;
    const bool in = bx < w && by < h;
    const int64_t plane = (int64_t)h * w;
    const typename A::T* go = gout + act.g_image(n, OC * plane);
    const typename A::T* yo = act.y_image(n);

    // the pixel's 81 gradOutput values (zero where the reference skips the term: gradInput2 near the frame's border)
    float g[OC];
#pragma unroll
    for (int tc = 0; tc < OC; ++tc) {
        const int gy = SECOND ? by - (tc / D - MD) : by, gx = SECOND ? bx - (tc % D - MD) : bx;
        if constexpr (Act::MASK) {
            // (a skipped term loads element 0 of its image -- a valid address -- and drops it: loads under a branch go out one
            //  at a time, each waited for; these go out a displacement row of gradOutput and y together)
            const bool ok = in && gy >= 0 && gy < h && gx >= 0 && gx < w;
            const int64_t at = ok ? (int64_t)tc * plane + (int64_t)gy * w + gx : 0;
            const typename A::T gv = go[at], yv = yo[at];
            if constexpr (Act::SELECT_LOADS) g[tc] = act(ok ? gv : 0.0f, ok ? yv : 0.0f);
            else g[tc] = ok ? act(gv, yv) : 0.0f;
            if (tc % D == D - 1) __builtin_amdgcn_sched_barrier(0);
        } else {
            g[tc] = (in && gy >= 0 && gy < h && gx >= 0 && gx < w) ? A::load(go[(int64_t)tc * plane + (int64_t)gy * w + gx]) : 0.0f;
        }
    }
    // (a term the reference skips -- gradInput2, displaced position outside the frame -- reads the other map at that same
    //  position: the zero padding of the staged window, so the skipped term is fma(0, 0, s) = s)

    auto stage = [&](int c, int buf) {
        const typename A::T* of = other + ((int64_t)n * channel + c) * plane;
        for (int e = tid; e < T::LH * T::LW; e += 256) {
            const T::Elem p = t.window(e);
            win[buf][p.r][p.col] = (p.gy >= 0 && p.gy < h && p.gx >= 0 && p.gx < w) ? A::load(of[(int64_t)p.gy * w + p.gx]) : 0.0f;
        }
    };
    if (c_begin >= c_end) return;
    stage(c_begin, 0);
    const float nelems = A::count(channel);
    for (int c = c_begin; c < c_end; ++c) {
        const int buf = (c - c_begin) & 1;
        __syncthreads();                                    // window c has been written; window c - 1 has been read
        if (c + 1 < c_end) stage(c + 1, buf ^ 1);
        float r = 0.0f;
#pragma unroll
        for (int l = 0; l < 32; ++l) {
            float s = 0.0f;
#pragma unroll
            for (int tc = l; tc < OC; tc += 32) {
                const int tj = tc / D, ti = tc % D;
                const float v = SECOND ? win[buf][py + 2 * MD - tj][px + 2 * MD - ti] : win[buf][py + tj][px + ti];
                s = A::term(s, g[tc], v);
            }
            r = A::add(r, s);
        }
        if (in) gin[((int64_t)n * channel + c) * plane + (int64_t)by * w + bx] = A::store(r, nelems);
    }
