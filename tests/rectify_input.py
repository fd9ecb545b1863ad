"""What `fused.rectify_inputs` has to equal, stated on its own: the channel map of the tensor the reference concatenates
for rectifyNet (networks/DAIN_slowmotion.py:177-181, networks/DAIN.py:264-268), the reference composition -- `torch.cat`
over the library's existing `fused` functions -- and the order in which the gradients of several time offsets are summed.
Field generation for the kernel tests is tests/fi_windows.py's (`build_field`, `field_shape`), by import."""
import numpy as np

from tests.fi_windows import build_field, field_shape  # noqa: F401  (re-exported for the GPU tests)

f32 = np.float32


def channel_map(filter_size2, ctx_channels=None):
    """name -> (first channel, one past the last), in the reference's order; "total" -> the channel count"""
    order = [("cur_output", 3), ("ref0", 3), ("ref2", 3), ("offset0", 2), ("offset1", 2), ("filter0", filter_size2),
             ("filter1", filter_size2)]
    if ctx_channels:
        order += [("ctx0", ctx_channels), ("ctx2", ctx_channels)]
    m, at = {}, 0
    for name, n in order:
        m[name] = (at, at + n)
        at += n
    m["total"] = at
    return m


def composition(torch, fused, ref0, ref2, offsets, filt, filter_size2, time_offsets, ctx0=None, ctx2=None):
    """[(rectify_input_t, cur_output_t)] the way a caller builds them from the existing functions: FilterInterpolate per
    time offset, FilterInterpolate_ctx_all once, torch.cat (DAIN_slowmotion.py:167-181)."""
    warped = None
    if ctx0 is not None:
        warped = fused.FilterInterpolate_ctx_all(ctx0, ctx2, offsets, filt)
    out = []
    for i, t in enumerate(time_offsets):
        off = [offsets[0][i], offsets[1][i]]
        cur, r0, r2 = fused.FilterInterpolate(ref0, ref2, off, filt, filter_size2, t)
        parts = [cur, r0, r2, off[0], off[1], filt[0], filt[1]]
        if warped is not None:
            parts += list(warped[i])
        out.append((torch.cat(parts, dim=1), cur))
    return out


def sum_in_order(terms):
    """left to right; None = an absent term"""
    total = None
    for t in terms:
        if t is not None:
            total = t if total is None else total + t
    return total


def expected_gradients(torch, fused, ref0, ref2, offsets, filt, filter_size2, time_offsets, ctx0, ctx2, g_bufs, g_curs):
    """The gradients `fused.rectify_inputs` documents, for incoming gradients g_bufs[t] / g_curs[t] (None = unused output):
      flow (d, t):      kernel term of t + the slice of g_bufs[t] that passed through
      filter d, frame:  the left-to-right sum over t ascending of (kernel term of t, passed-through slice of t)
      context tensor d: one FilterInterpolate_ctx_all backward over the time offsets whose buffer has a gradient
    Every kernel term comes from the existing functions' own backward on leaves of its own, so that the terms stay apart.
    Returns a dict name -> tensor or None: ref0, ref2, filter0, filter1, ctx0, ctx2, offset0 / offset1 (lists over t)."""
    n = len(time_offsets)
    m = channel_map(filter_size2, None if ctx0 is None else ctx0.size(1))
    leaf = lambda x: x.detach().clone().requires_grad_(True)       # noqa: E731
    terms = {"ref0": [], "ref2": [], "filter0": [], "filter1": []}
    g_off = [[None] * n, [None] * n]
    for t in range(n):
        gb, gc = g_bufs[t], g_curs[t]
        if gb is None and gc is None:
            continue
        r0, r2, f0, f2, k0, k2 = (leaf(x) for x in (ref0, ref2, offsets[0][t], offsets[1][t], filt[0], filt[1]))
        cur, o0, o2 = fused.FilterInterpolate(r0, r2, [f0, f2], [k0, k2], filter_size2, time_offsets[t])
        outs, gs = [cur], [sum_in_order([None if gb is None else gb[:, 0:3], gc])]
        if gb is not None:
            outs += [o0, o2]
            gs += [gb[:, 3:6], gb[:, 6:9]]
        torch.autograd.backward(outs, gs)
        through = (lambda name: None) if gb is None else (lambda name: gb[:, m[name][0]:m[name][1]])
        g_off[0][t] = sum_in_order([f0.grad, through("offset0")])
        g_off[1][t] = sum_in_order([f2.grad, through("offset1")])
        terms["ref0"].append(r0.grad)
        terms["ref2"].append(r2.grad)
        terms["filter0"] += [k0.grad, through("filter0")]
        terms["filter1"] += [k2.grad, through("filter1")]
    out = {k: sum_in_order(v) for k, v in terms.items()}
    out["offset0"], out["offset1"] = g_off
    out["ctx0"] = out["ctx2"] = None
    live = [t for t in range(n) if g_bufs[t] is not None]
    if ctx0 is not None and live:
        c0, c2 = leaf(ctx0), leaf(ctx2)
        warped = fused.FilterInterpolate_ctx_all(c0, c2, [[offsets[d][t] for t in live] for d in (0, 1)], filt)
        outs, gs = [], []
        for (w0, w2), t in zip(warped, live):
            outs += [w0, w2]
            gs += [g_bufs[t][:, m["ctx0"][0]:m["ctx0"][1]], g_bufs[t][:, m["ctx2"][0]:m["ctx2"][1]]]
        torch.autograd.backward(outs, gs)
        out["ctx0"], out["ctx2"] = c0.grad, c2.grad
    return out


def smooth_inputs(torch, rng, B, H, W, T, ctx_channels, amplitude=3.0, device="cuda:0"):
    """frames, per direction and time offset a smooth flow (a few pixels, some leaving the frame at the borders), two
    positive filters, two context tensors (None without ctx_channels)"""
    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a.astype(f32))).to(device)

    yy, xx = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")

    def flow():
        ph = rng.uniform(0, 6.28, 4)
        fx = amplitude * np.sin(xx / 17.0 + ph[0]) * np.cos(yy / 13.0 + ph[1]) + rng.uniform(-0.4, 0.4, (B, H, W))
        fy = amplitude * np.cos(xx / 11.0 + ph[2]) * np.sin(yy / 19.0 + ph[3]) + rng.uniform(-0.4, 0.4, (B, H, W))
        return dev(np.stack([fx, fy], axis=1))

    ref0, ref2 = dev(rng.random((B, 3, H, W))), dev(rng.random((B, 3, H, W)))
    offsets = [[flow() for _ in range(T)] for _ in (0, 1)]
    filt = [dev(rng.random((B, 16, H, W)) * 0.25) for _ in (0, 1)]
    ctx = [dev(rng.standard_normal((B, ctx_channels, H, W))) for _ in (0, 1)] if ctx_channels else [None, None]
    return ref0, ref2, offsets, filt, ctx[0], ctx[1]
