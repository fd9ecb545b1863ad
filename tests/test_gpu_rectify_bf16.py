"""GPU suite (`-m gpu`): rectifyNet's input on bfloat16 storage -- the head entry (vfi_rectify_head_forward_bf16) and
fused.rectify_inputs(dtype=torch.bfloat16), forward, backward, graph replay and under autocast.

Every result is compared as BITS, NaN at equal positions (tests/rectify_bf16.diff_bf16 / diff_f32), with what the float32
functions give: `torch.cat(...)` over them, `.to(torch.bfloat16)`.  The head entry writes into pattern-filled allocations
(dense, and channel slices at an odd element offset with an odd per-image element count): nothing outside is written."""
import functools

import numpy as np
import pytest

from tests import fi_ctx_bf16 as fb
from tests import forward_edges as fe
from tests import rectify_bf16 as rb
from tests import rectify_input as ri
from tests.test_gpu_rectify_input import SHAPE, cabi, fused, gpu, torch_mod  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

f32 = np.float32
W0, W2 = 0.75, 0.25


# ------------------------------------------------------------------ 1. the head entry

@functools.lru_cache(maxsize=None)
def head_reference(shape, filter_channels, channel):
    """(inputs on the GPU, expected head, expected float32 blend): computed once per case, never written"""
    import torch
    from vfidkr_amd import cabi as c
    g = tuple(gpu(torch, a) for a in rb.head_case(shape, filter_channels, channel))
    head, blend = rb.expected_head(torch, rb.library_blend(torch, c), *g, W0, W2)
    return g, head, blend


def check_head(torch, what, head, hbuf, blend, bbuf, want_head, want_blend):
    torch.cuda.synchronize()
    msg = rb.diff_bf16(torch, head, want_head)
    assert not msg, "%s, head: %s" % (what, msg)
    assert rb.guard_intact(torch, hbuf, head), "%s: written outside the head" % what
    if blend is not None:
        msg = rb.diff_f32(torch, blend, want_blend)
        assert not msg, "%s, float32 blend: %s" % (what, msg)
        assert rb.guard_intact(torch, bbuf, blend), "%s: written outside the float32 blend" % what


@pytest.mark.parametrize("dest", ["dense", "slice"])
@pytest.mark.parametrize("with_blend", [True, False])
@pytest.mark.parametrize("channel", rb.HEAD_CHANNELS)
@pytest.mark.parametrize("filter_channels", rb.HEAD_FILTERS)
@pytest.mark.parametrize("shape", rb.HEAD_SHAPES)
def test_head_entry(torch_mod, cabi, shape, filter_channels, channel, with_blend, dest):
    """the grid: one-block and several-row frames, odd and even widths (element and pair accesses), filter sizes 4 and 6
    (register taps and the generic quadrant loops), 1 / 3 / 4 frame channels, the float32 blend given or NULL, a dense
    destination or a slice of a wider buffer that is 2-byte aligned and no more"""
    torch = torch_mod
    B, H, W = shape
    for flow in rb.head_case(shape, filter_channels, channel)[2:4]:
        assert rb.census_ok(rb.census(flow, H, W))
    g, want_head, want_blend = head_reference(shape, filter_channels, channel)
    make = rb.guarded_dense if dest == "dense" else rb.guarded_slice
    hbuf, head = make(torch, (B, rb.head_channels(channel, filter_channels), H, W), torch.bfloat16)
    bbuf, blend = make(torch, (B, channel, H, W), torch.float32) if with_blend else (None, None)
    if dest == "slice":
        assert head.data_ptr() % 4 == 2 and head.stride(0) % 2 == 1 and head.stride(1) != H * W
    # which kernel instance: pairs for an aligned destination over even rows, single elements otherwise
    assert rb.takes_pairs(g[2], g[4], head, blend) == (dest == "dense" and W % 2 == 0)
    assert cabi.rectify_head_forward_bf16(*g, head, blend, W0, W2) == 0
    check_head(torch, "%s fc=%d C=%d %s" % (shape, filter_channels, channel, dest), head, hbuf, blend, bbuf, want_head, want_blend)


@pytest.mark.parametrize("with_blend", [True, False])
@pytest.mark.parametrize("shape", rb.PADDED_SHAPES)
def test_head_entry_odd_width_in_even_rows(torch_mod, cabi, shape, with_blend):
    """the lane class the dense grid cannot reach: every tensor's rows one element longer than an ODD width -- pair accesses
    and a lone last pixel in every row -- and, at 131 pixels, a second workgroup per row"""
    torch = torch_mod
    B, H, W = shape
    case = rb.head_case(shape, 16, 3)
    for flow in case[2:4]:
        assert rb.census_ok(rb.census(flow, H, W))
    g, want_head, want_blend = head_reference(shape, 16, 3)

    def padded(t):
        wide = torch.full(tuple(t.shape[:3]) + (W + 1,), float("nan"), device=t.device)
        wide[..., :W] = t
        return wide[..., :W]
    gp = tuple(padded(t) for t in g)
    rows = lambda C: (C * (H + 1) * (W + 1), (H + 1) * (W + 1), W + 1, 1)      # noqa: E731
    hbuf, head = rb.guarded(torch, (B, 45, H, W), torch.bfloat16, rows(45), 64)
    bbuf, blend = rb.guarded(torch, (B, 3, H, W), torch.float32, rows(3), 64) if with_blend else (None, None)
    assert rb.takes_pairs(gp[2], gp[4], head, blend) and W % 2 == 1 and head.stride(2) == gp[0].stride(2)
    assert cabi.rectify_head_forward_bf16(*gp, head, blend, W0, W2) == 0
    check_head(torch, "%s in rows of %d" % (shape, W + 1), head, hbuf, blend, bbuf, want_head, want_blend)


def test_head_entry_refuses_other_rows(torch_mod, cabi):
    """a head whose rows are farther apart than the frames': the binding and the library both refuse, nothing is written"""
    torch = torch_mod
    g, _, _ = head_reference((2, 16, 64), 16, 3)
    B, H, W = 2, 16, 64
    hbuf, head = rb.guarded(torch, (B, 45, H, W), torch.bfloat16, (45 * H * (W + 2), H * (W + 2), W + 2, 1), 64)
    assert cabi.rectify_head_forward_bf16(*g, head, None, W0, W2) == 1
    with torch.cuda.device(0):
        err = cabi.lib().vfi_rectify_head_forward_bf16(*[cabi._ptr(t) for t in g], cabi._ptr(head), None, B, 3, H, W, 16, W0, W2,
                                                       cabi._st(g[0]), cabi._st(g[2]), cabi._st(g[4]), cabi._st(head), cabi._st(g[0]),
                                                       cabi._stream(g[0]))
    assert err == cabi.VFI_ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((hbuf == hbuf[0]).all())


# ------------------------------------------------------------------ 2. rounding

# float32 patterns and the bfloat16 pattern round-to-nearest-even gives: ties towards the even neighbour in both directions
# and just off the tie, the largest finite values (they round up to infinity), float32 and bfloat16 subnormals, the tie
# between the largest subnormal and the smallest normal, infinities, +0
ROUNDING = ((0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0xBF808000, 0xBF80), (0xBF818000, 0xBF82), (0x3F808001, 0x3F81),
            (0x3F817FFF, 0x3F81), (0x7F7FFFFF, 0x7F80), (0xFF7FFFFF, 0xFF80), (0x7F7F7FFF, 0x7F7F), (0x7F7F8000, 0x7F80),
            (0x00000001, 0x0000), (0x00008000, 0x0000), (0x00008001, 0x0001), (0x00018000, 0x0002), (0x00010000, 0x0001),
            (0x807F8000, 0x8080), (0x80000001, 0x8000), (0x7F800000, 0x7F80), (0xFF800000, 0xFF80), (0x00000000, 0x0000))


@pytest.mark.parametrize("side", [0, 2])
def test_rounding_of_planted_frame_values(torch_mod, cabi, side):
    """one-hot filters (the tap at the pixel itself) and zero flows, weight 1 on the planted side and 0 on the other: the
    planted side's output and the blend are the frame's own values, so each planted pattern must come out as the pattern
    round-to-nearest-even gives -- and the whole head as the composition's.  The plants stand four pixels apart: no window
    holds two of them (an infinity times a zero tap is NaN in the neighbours' windows, in both computations)."""
    torch = torch_mod
    B, C, H, W = 1, 3, 8, 16
    rng = np.random.default_rng(77 + side)
    refs = [rng.standard_normal((B, C, H, W)).astype(f32) for _ in range(2)]
    spots = [(c, y, x) for c in range(C) for y in (1, 5) for x in (1, 5, 9, 13)]
    assert len(spots) >= len(ROUNDING)
    planted = refs[side // 2].view(np.uint32)
    for (pat, _), (c, y, x) in zip(ROUNDING, spots):
        planted[0, c, y, x] = pat
    # -0.0 too: compared with the composition only (its sign does not survive the sums of the window's zero products)
    planted[0, 0, 3, 3] = 0x80000000
    flow = np.zeros((B, 2, H, W), f32)
    filt = np.zeros((B, 16, H, W), f32)
    filt[:, 5] = 1.0                                            # window row 1, column 1: the pixel (ix, iy) itself
    w0, w2 = (1.0, 0.0) if side == 0 else (0.0, 1.0)
    g = tuple(gpu(torch, a) for a in (refs[0], refs[1], flow, flow, filt, filt))
    assert np.array_equal(g[side // 2].cpu().numpy().view(np.uint32), planted)          # (the upload keeps the patterns)
    want_head, want_blend = rb.expected_head(torch, rb.library_blend(torch, cabi), *g, w0, w2)
    hbuf, head = rb.guarded_dense(torch, (B, 45, H, W), torch.bfloat16)
    bbuf, blend = rb.guarded_dense(torch, (B, C, H, W), torch.float32)
    assert cabi.rectify_head_forward_bf16(*g, head, blend, w0, w2) == 0
    check_head(torch, "planted side %d" % side, head, hbuf, blend, bbuf, want_head, want_blend)
    got, got32 = rb.tensor_bits(torch, head), blend.cpu().numpy().view(np.uint32)
    first = 3 + 3 * (side // 2)                                 # out0 in channels 3-5, out2 in 6-8
    for (pat, want), (c, y, x) in zip(ROUNDING, spots):
        assert got[0, first + c, y, x] == want, "out%d: %08x -> %04x, not %04x" % (side, pat, got[0, first + c, y, x], want)
        assert got[0, c, y, x] == want, "blend: %08x -> %04x, not %04x" % (pat, got[0, c, y, x], want)
        assert got32[0, c, y, x] == pat, "float32 blend: %08x -> %08x" % (pat, got32[0, c, y, x])


def test_nan_in_frames_flows_and_filters(torch_mod, cabi):
    """tests/forward_edges.small_fi_inputs on both sides: NaN, infinities, FLT_MAX, subnormals and -0.0 in the frames and in
    single filter taps, NaN / infinite / huge flows (invalid pixels, copied through) and the flows exactly at the validity
    limits.  NaN at the composition's positions -- in the warped channels and in the channels that pass through"""
    torch = torch_mod
    B, C, H, W = 2, 3, 12, 20
    s0 = fe.small_fi_inputs(np.random.default_rng(501), B, C, H, W)
    s2 = fe.small_fi_inputs(np.random.default_rng(502), B, C, H, W)
    assert all(np.isnan(a).any() for a in s0 + s2)
    g = tuple(gpu(torch, a) for a in (s0[0], s2[0], s0[1], s2[1], s0[2], s2[2]))
    want_head, want_blend = rb.expected_head(torch, rb.library_blend(torch, cabi), *g, W0, W2)
    wnan = np.isnan(rb.from_bits(rb.tensor_bits(torch, want_head)))
    assert wnan[:, 0:3].any() and wnan[:, 3:6].any() and wnan[:, 6:9].any() and wnan[:, 9:13].any() and wnan[:, 13:].any()
    for make in (rb.guarded_dense, rb.guarded_slice):
        hbuf, head = make(torch, (B, 45, H, W), torch.bfloat16)
        bbuf, blend = make(torch, (B, C, H, W), torch.float32)
        assert cabi.rectify_head_forward_bf16(*g, head, blend, W0, W2) == 0
        check_head(torch, "non-finite inputs, %s" % make.__name__, head, hbuf, blend, bbuf, want_head, want_blend)
        assert np.array_equal(np.isnan(rb.from_bits(rb.tensor_bits(torch, head))), wnan)


# ------------------------------------------------------------------ 3. fused.rectify_inputs(dtype=torch.bfloat16), forward

def times_of(T):
    return [0.5] if T == 1 else [0.25, 0.5, 0.75]


@functools.lru_cache(maxsize=None)
def smooth_case(T, cctx, W=SHAPE[2], kind="float32", seed=0):
    """inputs on the GPU (never written): float32 frames, flows and filters as `kind`, bfloat16 context tensors"""
    import torch
    B, H, _ = SHAPE
    ref0, ref2, offs, filt, ctx0, ctx2 = ri.smooth_inputs(torch, np.random.default_rng(600 + 10 * T + seed), B, H, W, T, cctx)
    if kind == "bfloat16":
        offs, filt = [[o.to(torch.bfloat16) for o in d] for d in offs], [k.to(torch.bfloat16) for k in filt]
    bf = lambda t: None if t is None else t.to(torch.bfloat16)      # noqa: E731
    return ref0, ref2, offs, filt, bf(ctx0), bf(ctx2)


@pytest.mark.parametrize("kind", ["float32", "bfloat16"])
@pytest.mark.parametrize("T,cctx,W", [(1, None, 136), (1, 6, 136), (3, None, 136), (3, 6, 136), (3, 6, 135)])
def test_rectify_inputs_forward(torch_mod, fused, T, cctx, W, kind):
    """buffers and cur_output bit-equal to the float32 composition, `.to(torch.bfloat16)`; W = 135: the context warp takes
    its one-thread-per-pixel kernel and the head single-element accesses"""
    torch = torch_mod
    B, H, _ = SHAPE
    ref0, ref2, offs, filt, ctx0, ctx2 = smooth_case(T, cctx, W, kind)
    if cctx:
        assert fb.takes_staged(ctx0.shape, ctx0.stride(), ctx0.data_ptr(), 16) == (W % 2 == 0)
    want = rb.expected_buffers(torch, fused, ref0, ref2, offs, filt, 16, times_of(T), ctx0, ctx2)
    got = fused.rectify_inputs(ref0, ref2, offs, filt, 16, times_of(T), ctx0, ctx2, dtype=torch.bfloat16)
    m = ri.channel_map(16, cctx)
    assert len(got) == T
    for t, ((buf, cur), (rbuf, rcur)) in enumerate(zip(got, want)):
        assert buf.dtype == torch.bfloat16 and buf.shape == (B, m["total"], H, W) and buf.is_contiguous() and buf.grad_fn is None
        assert cur.dtype == torch.float32 and cur.shape == (B, 3, H, W) and cur.is_contiguous()
        for name in (k for k in m if k != "total"):
            a, b = m[name]
            msg = rb.diff_bf16(torch, buf[:, a:b], rbuf[:, a:b])
            assert not msg, "T=%d t=%d W=%d %s %s: %s" % (T, t, W, kind, name, msg)
        msg = rb.diff_f32(torch, cur, rcur)
        assert not msg, "T=%d t=%d cur_output: %s" % (T, t, msg)
        # the float32 blend is not the rounded one read back
        assert not torch.equal(cur, buf[:, 0:3].float())


# ------------------------------------------------------------------ 4. backward

def _leaves(torch, case, context_grad=True):
    ref0, ref2, offs, filt, ctx0, ctx2 = case
    leaf = lambda t, on=True: t.detach().clone().requires_grad_(on)      # noqa: E731
    return (leaf(ref0), leaf(ref2), [[leaf(o) for o in d] for d in offs], [leaf(k) for k in filt], leaf(ctx0, context_grad),
            leaf(ctx2, context_grad))


def _flat(leaves):
    ref0, ref2, offs, filt, ctx0, ctx2 = leaves
    names = ["ref0", "ref2", "filter0", "filter1", "ctx0", "ctx2"] + ["offset%d[%d]" % (d, t) for d in (0, 1) for t in range(len(offs[d]))]
    return list(zip(names, [ref0, ref2, filt[0], filt[1], ctx0, ctx2] + offs[0] + offs[1]))


@functools.lru_cache(maxsize=None)
def incoming(T, total):
    """the gradients arriving at the T buffers (bfloat16) and at the T cur_output tensors (float32)"""
    import torch
    B, H, W = SHAPE
    rng = np.random.default_rng(700 + T)
    return ([gpu(torch, rng.standard_normal((B, total, H, W))).to(torch.bfloat16) for _ in range(T)],
            [gpu(torch, rng.standard_normal((B, 3, H, W))) for _ in range(T)])


def _backward(torch, pairs, T, variant):
    gb, gc = incoming(T, pairs[0][0].size(1))
    outs, grads = [], []
    for t, (buf, cur) in enumerate(pairs):
        if not (variant == "buffer 1 unused" and t == 1):
            outs.append(buf), grads.append(gb[t])
        if variant != "cur_output unused":
            outs.append(cur), grads.append(gc[t])
    torch.autograd.backward(outs, grads)


@pytest.mark.parametrize("kind", ["float32", "bfloat16"])
@pytest.mark.parametrize("T,variant", [(1, "all"), (1, "cur_output unused"), (1, "context without grad"), (3, "all"),
                                       (3, "cur_output unused"), (3, "buffer 1 unused"), (3, "context without grad")])
def test_rectify_inputs_backward(torch_mod, fused, T, variant, kind):
    """every gradient bit-equal to autograd's through the float32 rectify_inputs (contexts, flows and filters entering
    through `.float()`), its buffers `.to(torch.bfloat16)`, fed the same incoming gradients; frames, flows and filters get
    gradients of their own dtype (float32, or a bfloat16 leaf's rounded by autograd), the contexts bfloat16 ones"""
    torch = torch_mod
    case = smooth_case(T, 6, SHAPE[2], kind, seed=1)
    train_ctx = variant != "context without grad"

    def run(bf16):
        leaves = _leaves(torch, case, train_ctx)
        ref0, ref2, offs, filt, ctx0, ctx2 = leaves
        if bf16:
            pairs = fused.rectify_inputs(ref0, ref2, offs, filt, 16, times_of(T), ctx0, ctx2, dtype=torch.bfloat16)
            assert all(b.dtype == torch.bfloat16 and c.dtype == torch.float32 and b.grad_fn is c.grad_fn is not None for b, c in pairs)
        else:
            wide = [[o.float() for o in d] for d in offs], [k.float() for k in filt]
            pairs = fused.rectify_inputs(ref0, ref2, wide[0], wide[1], 16, times_of(T), ctx0.float(), ctx2.float())
            pairs = [(b.to(torch.bfloat16), c) for b, c in pairs]
        _backward(torch, pairs, T, variant)
        return _flat(leaves)
    want = run(False)
    got = run(True)
    for (name, g), (_, r) in zip(got, want):
        assert (g.grad is None) == (r.grad is None), (variant, name)
        if name.startswith("ctx"):
            assert (g.grad is None) == (not train_ctx)
        else:
            assert g.grad is not None
        if g.grad is None:
            continue
        assert g.grad.dtype == g.dtype == (torch.bfloat16 if name.startswith("ctx") or (kind == "bfloat16" and name[:3] in ("fil", "off"))
                                          else torch.float32), name
        msg = (rb.diff_bf16 if g.grad.dtype == torch.bfloat16 else rb.diff_f32)(torch, g.grad, r.grad)
        assert not msg, "T=%d %s %s: grad %s: %s" % (T, variant, kind, name, msg)
    if T == 3 and variant == "all":                             # reproducible: a second run gives the same bits, NaN or not
        again = run(True)
        for (name, g), (_, a) in zip(got, again):
            assert torch.equal(g.grad.view(torch.int16 if g.grad.dtype == torch.bfloat16 else torch.int32),
                               a.grad.view(torch.int16 if a.grad.dtype == torch.bfloat16 else torch.int32)), name


# ------------------------------------------------------------------ 5. graph capture

def test_rectify_inputs_replays_from_a_graph(torch_mod, fused):
    """the bfloat16 forward allocates and enqueues launches only: captured once on one stream, it replays the eager bits"""
    torch = torch_mod
    times = times_of(3)
    ref0, ref2, offs, filt, ctx0, ctx2 = smooth_case(3, 6, SHAPE[2], "bfloat16", seed=2)
    call = lambda: fused.rectify_inputs(ref0, ref2, offs, filt, 16, times, ctx0, ctx2, dtype=torch.bfloat16)      # noqa: E731
    want = [(buf.clone(), cur.clone()) for buf, cur in call()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = call()
    for _ in range(2):
        for buf, cur in got:
            buf.fill_(float("nan")), cur.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for t, ((buf, cur), (rbuf, rcur)) in enumerate(zip(got, want)):
            assert not rb.diff_bf16(torch, buf, rbuf) and not torch.isnan(buf.float()).any(), "replay t=%d" % t
            assert not rb.diff_f32(torch, cur, rcur) and not torch.isnan(cur).any(), "replay t=%d cur_output" % t
    del graph


# ------------------------------------------------------------------ 6. under autocast

def test_three_layer_stand_in_under_autocast(torch_mod, fused):
    """filter conv and context conv (bfloat16 out of autocast), rectify_inputs(dtype=torch.bfloat16), a rectify conv that
    takes the buffer as it is, and a loss on rectify + cur_output: buffer, loss and every leaf's gradient bit-equal to the
    same graph written with the float32 composition and `.to(torch.bfloat16)`"""
    torch = torch_mod
    F = torch.nn.functional
    B, H, W = 1, 24, 40
    rng = np.random.default_rng(800)
    base = ri.smooth_inputs(torch, rng, B, H, W, 1, None, amplitude=2.0)
    weights = [gpu(torch, rng.standard_normal(s) * k) for s, k in (((32, 6, 1, 1), 0.1), ((6, 3, 1, 1), 0.5), ((3, 57, 1, 1), 0.1))]
    target = gpu(torch, rng.random((B, 3, H, W)))

    def run(bf16):
        leaf = lambda t: t.detach().clone().requires_grad_()      # noqa: E731
        ref0, ref2, f0, f2 = leaf(base[0]), leaf(base[1]), leaf(base[2][0][0]), leaf(base[2][1][0])
        wf, wc, wr = (leaf(w) for w in weights)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            taps = F.conv2d(torch.cat((ref0, ref2), 1), wf)
            filt = [taps[:, :16], taps[:, 16:]]
            ctx0, ctx2 = F.conv2d(ref0, wc), F.conv2d(ref2, wc)
            assert taps.dtype == torch.bfloat16 and ctx0.dtype == torch.bfloat16
            if bf16:
                buf, cur = fused.rectify_inputs(ref0, ref2, [[f0], [f2]], filt, 16, [0.5], ctx0, ctx2, dtype=torch.bfloat16)[0]
            else:
                buf, cur = rb.expected_buffers(torch, fused, ref0, ref2, [[f0], [f2]], filt, 16, [0.5], ctx0, ctx2)[0]
            assert buf.dtype == torch.bfloat16 and cur.dtype == torch.float32 and buf.shape == (B, 57, H, W)
            rect = F.conv2d(buf, wr)
            assert rect.dtype == torch.bfloat16
            loss = ((rect.float() + cur - target) ** 2).mean()
        loss.backward()
        return buf.detach(), loss.detach(), [("ref0", ref0), ("ref2", ref2), ("flow0", f0), ("flow2", f2), ("filter conv", wf),
                                             ("context conv", wc), ("rectify conv", wr)]
    rbuf, rloss, want = run(False)
    buf, loss, got = run(True)
    msg = rb.diff_bf16(torch, buf, rbuf)
    assert not msg, "buffer: %s" % msg
    assert not rb.diff_f32(torch, loss.reshape(1), rloss.reshape(1))
    for (name, g), (_, r) in zip(got, want):
        assert g.grad is not None and g.grad.dtype == g.dtype == torch.float32 and bool(torch.isfinite(g.grad).all()), name
        assert float(g.grad.abs().max()) > 0, name
        msg = rb.diff_f32(torch, g.grad, r.grad)
        assert not msg, "grad %s: %s" % (name, msg)
