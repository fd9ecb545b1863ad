"""numpy mirror of the quarter-resolution backwards (csrc/flow_up4.h: up4_foot, up4_adjoint; csrc/projection_up4_backward.hip).
Helper module: no tests of its own.

`up4_backward(grad_full_list, mul0, mul1_list)` restates up4_adjoint in float32, operation for operation:

    for item i (ascending):  s = 0
        for d_y in the row footprint (ascending):  r = 0
            for d_x in the column footprint (ascending):  r = fmaf(w(d_x), G_i[d_y, d_x], r)
            s = fmaf(w(d_y), r, s)
        acc = fmaf(m_i, s, acc)                         m_i = fp32(mul0 * mul1[i]),  acc starts at 0

The footprint of quarter pixel q along an axis is d = 4q-2 .. 4q+5 cut to the image; w(d) = (i0 == q ? l0 : 0) +
(i1 == q ? l1 : 0) of up4_tap(d).  It also returns, in float64, the same sum, the sum S of the absolute values of its
terms m_i w(d_y) w(d_x) G_i[d_y, d_x] and the number n of addends, per quarter pixel.
"""
import numpy as np

f32 = np.float32


def fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays: the exact product (48 bits: exact in float64) plus c, rounded ONCE to float32.
    The float64 sum is rounded to odd (TwoSum gives its error), which makes the second rounding to float32 innocuous."""
    a, b, c = np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32)
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    odd = (s.view(np.int64) & 1).astype(bool)
    fix = (e != 0) & ~odd & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def up4_tap(d, in_size):
    """up4_tap of flow_up4.h for an integer array d: (i0, i1, l0, l1)"""
    d = np.asarray(d)
    src = f32(0.25) * (d.astype(f32) + f32(0.5)) - f32(0.5)
    src = np.where(src < 0, f32(0), src).astype(f32)
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < in_size - 1)
    l1 = (src - i0.astype(f32)).astype(f32)
    l0 = (f32(1) - l1).astype(f32)
    return i0, i1, l0, l1


def footprint(in_size):
    """(d [in_size, 8], w [in_size, 8] float32, valid [in_size, 8]): pixel d[q, k] = 4q - 2 + k and its weight for q"""
    q = np.arange(in_size)[:, None]
    d = 4 * q - 2 + np.arange(8)[None, :]
    valid = (d >= 0) & (d < 4 * in_size)
    i0, i1, l0, l1 = up4_tap(np.clip(d, 0, 4 * in_size - 1), in_size)
    w = (np.where(i0 == q, l0, f32(0)).astype(f32) + np.where(i1 == q, l1, f32(0)).astype(f32)).astype(f32)
    return d, np.where(valid, w, f32(0)).astype(f32), valid


def up4_backward(grad_full_list, mul0, mul1_list):
    """-> (grad_q float32 [B,C,hq,wq] in the kernel's order, ref64, S, n)"""
    g0 = np.asarray(grad_full_list[0])
    B, C, H, W = g0.shape
    hq, wq = H // 4, W // 4
    assert H == 4 * hq and W == 4 * wq
    dy, wy, vy = footprint(hq)
    dx, wx, vx = footprint(wq)
    dyc, dxc = np.clip(dy, 0, H - 1), np.clip(dx, 0, W - 1)
    acc = np.zeros((B, C, hq, wq), f32)
    ref = np.zeros((B, C, hq, wq), np.float64)
    S = np.zeros((B, C, hq, wq), np.float64)
    n = np.zeros((hq, wq), np.int64)
    for G, m1 in zip(grad_full_list, mul1_list):
        G = np.asarray(G, f32)
        m = f32(f32(mul0) * f32(m1))
        s = np.zeros((B, C, hq, wq), f32)
        s64 = np.zeros((B, C, hq, wq), np.float64)
        a64 = np.zeros((B, C, hq, wq), np.float64)
        for ky in range(8):
            rows = G[:, :, dyc[:, ky], :]                                   # [B, C, hq, W]
            r = np.zeros((B, C, hq, wq), f32)
            r64 = np.zeros((B, C, hq, wq), np.float64)
            ra64 = np.zeros((B, C, hq, wq), np.float64)
            for kx in range(8):
                v = rows[:, :, :, dxc[:, kx]]                               # [B, C, hq, wq]
                use = vx[:, kx][None, None, None, :]
                r = np.where(use, fma32(wx[:, kx][None, None, None, :], v, r), r)
                t = wx[:, kx].astype(np.float64)[None, None, None, :] * v.astype(np.float64)
                r64 += np.where(use, t, 0.0)
                ra64 += np.where(use, np.abs(t), 0.0)
            use = vy[:, ky][None, None, :, None]
            wyk = wy[:, ky][None, None, :, None]
            s = np.where(use, fma32(wyk, r, s), s)
            s64 += np.where(use, wyk.astype(np.float64) * r64, 0.0)
            a64 += np.where(use, wyk.astype(np.float64) * ra64, 0.0)
        acc = fma32(m, s, acc)
        ref += float(m) * s64
        S += abs(float(m)) * a64
        n += vy.sum(1)[:, None] * vx.sum(1)[None, :]
    return acc, ref, S, np.broadcast_to(n, (B, C, hq, wq))


def proj_up4_backward(oracle, flow_q, mul0, mul1_list, counts, gouts, depths=None, outs=None):
    """The composition on the CPU: oracle.flow_upsample4(fmad=1) -> oracle.flowproj_bwd / depthflowproj_bwd -> up4_backward.
    -> (grad_q float32, ref64, S, n, [G_i], [grad_depth_i] or None)"""
    Gs, gds = [], []
    for i, m1 in enumerate(mul1_list):
        F = oracle.flow_upsample4(flow_q, mul0, m1, fmad=1)
        if depths is None:
            Gs.append(oracle.flowproj_bwd(F, counts[i], gouts[i]))
        else:
            gf, gd = oracle.depthflowproj_bwd(F, depths[i], counts[i], outs[i], gouts[i])
            Gs.append(gf)
            gds.append(gd)
    return (*up4_backward(Gs, mul0, mul1_list), Gs, gds if depths is not None else None)
