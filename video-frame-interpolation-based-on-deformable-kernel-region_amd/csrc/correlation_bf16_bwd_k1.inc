// correlation_bf16_bwd_k1.inc -- the statements of the tiled bfloat16 correlation backward (correlation_bf16.hip), included
// where SECOND, Act, win (CorrBwdWindow), t (CorrBwdTile), other, gout, gin, channel, h, w and act are in scope: once in the
// single-gradient kernel corr_backward_k1_bf16 and once in the device function the pair kernels call.  The text is shared
// instead of the function because the single-gradient kernels compiled through the function came out slower (another
// interleaving of the window reads with the multiply-adds, 130 instead of 124 registers in one instance: DESIGN.md
// 4.3a-6); included in the kernel they are the instructions they were.
    typedef CorrBwdTile T;
    constexpr int MD = T::MD, D = T::D, OC = T::OC;
    const int tid = threadIdx.x, px = tid & 63, py = tid >> 6;
    const int bx = t.x0 + px, by = t.y0 + py;
    const int n = t.n, c_begin = t.c_begin, c_end = t.c_end;
    const bool in = bx < w && by < h;
    const int64_t plane = (int64_t)h * w;
    const bf16_t* go = gout + act.g_image(n, OC * plane);
    const bf16_t* yo = act.y_image(n);

    float g[OC];
#pragma unroll
    for (int tc = 0; tc < OC; ++tc) {
        const int gy = SECOND ? by - (tc / D - MD) : by, gx = SECOND ? bx - (tc % D - MD) : bx;
        if constexpr (Act::MASK) {
            // (a skipped term loads element 0 of its image -- a valid address -- and drops it, so that the loads of a
            //  displacement row of gradOutput and y go out together: corr_backward_k1_body, correlation.hip)
            const bool ok = in && gy >= 0 && gy < h && gx >= 0 && gx < w;
            const int64_t at = ok ? (int64_t)tc * plane + (int64_t)gy * w + gx : 0;
            const bf16_t gv = go[at], yv = yo[at];
            g[tc] = ok ? act(gv, yv) : 0.0f;
            if (tc % D == D - 1) __builtin_amdgcn_sched_barrier(0);
        } else {
            g[tc] = (in && gy >= 0 && gy < h && gx >= 0 && gx < w) ? bf16_widen(go[(int64_t)tc * plane + (int64_t)gy * w + gx]) : 0.0f;
        }
    }

    auto stage = [&](int c, int buf) {
        const bf16_t* of = other + ((int64_t)n * channel + c) * plane;
        for (int e = tid; e < T::LH * T::LW; e += 256) {
            const T::Elem p = t.window(e);
            win[buf][p.r][p.col] = (p.gy >= 0 && p.gy < h && p.gx >= 0 && p.gx < w) ? bf16_widen(of[(int64_t)p.gy * w + p.gx]) : 0.0f;
        }
    };
    if (c_begin >= c_end) return;
    stage(c_begin, 0);
    const float nelems = (float)channel;
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
                s = fmaf(g[tc], v, s);
            }
            r += s;
        }
        if (in) gin[((int64_t)n * channel + c) * plane + (int64_t)by * w + bx] = bf16_rne(r / nelems);
    }
