"""What the bfloat16 rectify buffer has to equal, stated on its own (no test in here, nothing of the product imported at
module level):

  expected_head / expected_buffers   the buffer as `torch.cat(...).to(torch.bfloat16)` over the existing float32 functions
                                     (`blend_fn`: the library's float32 entry on the GPU, the CPU oracle in the host test;
                                     tests/rectify_input.composition for whole buffers, the contexts entering as `.float()`)
  diff_bf16 / diff_f32               the NaN-aware bit comparison: NaN at the same places, everything else bit for bit
  guarded_dense / guarded_slice      a destination inside a pattern-filled allocation (tests/pwc_bf16.guarded): dense, or a
                                     channel slice of a wider buffer at an ODD element offset with an ODD per-image element
                                     count and planes one row longer than the frame's -- 2-byte aligned and no more
  takes_pairs                        which of the kernel's two instances a call reaches (the host's alignment test, restated)
  census                             from a flow alone: invalid pixels, valid pixels whose 4 x 4 window is clamped at a border
                                     (per border too), interior pixels
  head_case                          the inputs of one case of the head entry's grid, shared by the host and the GPU test
"""
import functools

import numpy as np

from tests import fi_windows as fw
from tests import rectify_input as ri
from tests.corr_bf16 import bits, from_bits, same_bits, to_bf16  # noqa: F401  (re-exported)
from tests.corr_edges import describe_difference, same_bits_nan_aware
from tests.pwc_bf16 import guard_intact, guarded  # noqa: F401

f32 = np.float32
NAME = "vfi_rectify_head_forward_bf16"

# the grid of the head entry's test: (B, H, W) x filter channels x frame channels
HEAD_SHAPES = ((1, 5, 7), (2, 9, 21), (2, 16, 64), (3, 6, 66))
HEAD_FILTERS = (16, 36)
HEAD_CHANNELS = (1, 3, 4)
# the lane classes of the kernel that the grid's dense inputs cannot reach: an ODD width inside EVEN row strides -- pairs
# everywhere and a lone last pixel per row -- on more than one workgroup per row (128 pixels each)
PADDED_SHAPES = ((2, 6, 21), (1, 5, 131))


# ------------------------------------------------------------------ the expected buffer

def head_channels(channel, filter_channels):
    return 3 * channel + 4 + 2 * filter_channels


def expected_head(torch, blend_fn, ref0, ref2, flow0, flow2, filt0, filt2, w0, w2):
    """(head, blend): blend_fn(ref0, ref2, flow0, flow2, filt0, filt2, w0, w2) -> float32 (blend, out0, out2); the head is
    torch.cat in the reference's order, rounded once by torch"""
    blend, out0, out2 = blend_fn(ref0, ref2, flow0, flow2, filt0, filt2, w0, w2)
    return torch.cat((blend, out0, out2, flow0, flow2, filt0, filt2), 1).to(torch.bfloat16), blend


def oracle_blend(torch, oracle):
    """blend_fn on CPU tensors: the CPU oracle with the kernels' fused multiply-adds"""
    def fn(*args):
        arrays = [a.numpy() for a in args[:6]]
        return tuple(torch.from_numpy(np.ascontiguousarray(o, dtype=f32)) for o in oracle.filterinterp_blend(*arrays, args[6], args[7], fmad=1))
    return fn


def library_blend(torch, cabi):
    """blend_fn on GPU tensors: vfi_filterinterp_blend_forward into dense outputs"""
    def fn(ref0, ref2, flow0, flow2, filt0, filt2, w0, w2):
        outs = [torch.empty_like(ref0) for _ in range(3)]
        assert cabi.filterinterp_blend_forward(ref0, ref2, flow0, flow2, filt0, filt2, *outs, w0, w2) == 0
        return tuple(outs)
    return fn


def expected_buffers(torch, fused, ref0, ref2, offsets, filt, filter_size2, time_offsets, ctx0=None, ctx2=None):
    """[(rectify_input_t as bfloat16, cur_output_t as float32)]: the float32 composition (FilterInterpolate per time offset,
    FilterInterpolate_ctx_all, torch.cat) on the widened flows, filters and contexts, each buffer rounded once"""
    wide = lambda t: None if t is None else t.float()       # noqa: E731
    pairs = ri.composition(torch, fused, ref0, ref2, [[wide(o) for o in d] for d in offsets], [wide(k) for k in filt],
                           filter_size2, time_offsets, wide(ctx0), wide(ctx2))
    return [(buf.to(torch.bfloat16), cur) for buf, cur in pairs]


# ------------------------------------------------------------------ comparison

def tensor_bits(torch, t):
    """the uint16 patterns of a bfloat16 tensor (any strides, any device)"""
    assert t.dtype == torch.bfloat16
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def diff_bf16(torch, got, want):
    """'' or a message: two bfloat16 tensors, NaN at the same places, every other element bit for bit"""
    return same_bits(tensor_bits(torch, got), tensor_bits(torch, want))


def diff_f32(torch, got, want):
    assert got.dtype == torch.float32 and want.dtype == torch.float32
    g, w = got.detach().contiguous().cpu().numpy(), want.detach().contiguous().cpu().numpy()
    return "" if same_bits_nan_aware(g, w) else (describe_difference(g, w) if g.shape == w.shape else "shapes %s / %s" % (g.shape, w.shape))


# ------------------------------------------------------------------ guarded destinations

def guarded_dense(torch, shape, dtype):
    return guarded(torch, shape, dtype)


def slice_layout(shape, extra_channels=3, first=1):
    """(strides, offset) of a [B, C, H, W] channel slice of a wider buffer: rows W apart (the frames' row stride), planes one
    row longer than the frame's, C + extra_channels planes per image plus one element where that makes the per-image count
    odd, the slice starting at channel `first`, one element further where that makes the offset odd"""
    B, C, H, W = shape
    sc = (H + 1) * W
    sb = (C + extra_channels) * sc
    sb += 1 - sb % 2
    offset = 64 + first * sc
    offset += 1 - offset % 2
    return (sb, sc, W, 1), offset


def guarded_slice(torch, shape, dtype, extra_channels=3, first=1):
    stride, offset = slice_layout(shape, extra_channels, first)
    return guarded(torch, shape, dtype, stride, offset)


def takes_pairs(flow, filt, head, blend=None):
    """the entry's host decision, restated: every row of the flows, the filters and the float32 blend starts 8-byte aligned
    and every row of the head 4-byte aligned (aligned bases, even batch, channel and row strides)"""
    def rows(t, nbytes):
        return t.data_ptr() % nbytes == 0 and all(s % 2 == 0 for s in t.stride()[:3])
    return rows(flow, 8) and rows(filt, 8) and rows(head, 4) and (blend is None or rows(blend, 8))


# ------------------------------------------------------------------ census

def census(flow, h, w):
    """counts over the pixels of a flow [B, 2, h, w], from the flow alone (the 4 x 4 window of filter size 4 at ix - 1,
    iy - 1): invalid; valid with the window clamped at a border (`clamped`, and per border); valid with the whole window
    inside the frame (`interior`)"""
    valid, ix, iy, _, _ = fw.samples(flow, h, w)
    L, T = ix - 1, iy - 1
    edge = {"left": valid & (L < 0), "top": valid & (T < 0), "right": valid & (L + 3 > w - 1), "bottom": valid & (T + 3 > h - 1)}
    clamped = edge["left"] | edge["top"] | edge["right"] | edge["bottom"]
    out = {k: int(v.sum()) for k, v in edge.items()}
    out.update(total=int(valid.size), invalid=int((~valid).sum()), clamped=int(clamped.sum()), interior=int((valid & ~clamped).sum()))
    return out


def census_ok(c):
    """every kind of pixel is there, windows are clamped at all four borders, and at least half of the pixels are valid"""
    return (min(c["invalid"], c["clamped"], c["interior"], c["left"], c["top"], c["right"], c["bottom"]) >= 1 and
            2 * c["invalid"] <= c["total"])


# ------------------------------------------------------------------ cases

def head_flow(rng, B, H, W):
    """steps of 1/8 within +-3/4 of a pixel (at a border half of them leave the frame), and for one pixel in six a flow
    anywhere within +-0.7 of the frame: beyond half the frame it is invalid, within it the window lands anywhere"""
    fl = rng.integers(-6, 7, (B, 2, H, W)) / 8.0
    far = rng.uniform(-0.7, 0.7, (B, 2, H, W)) * np.array([W, H], np.float64)[None, :, None, None]
    pick = rng.random((B, 1, H, W)) < 1.0 / 6.0
    return np.where(pick, np.round(far * 8) / 8, fl).astype(f32)


@functools.lru_cache(maxsize=None)
def head_case(shape, filter_channels, channel):
    """numpy inputs of one case: frames, flows (head_flow), filters with both signs"""
    B, H, W = shape
    rng = np.random.default_rng(1000 * filter_channels + 100 * channel + H * W + B)
    ref0, ref2 = (rng.standard_normal((B, channel, H, W)).astype(f32) for _ in range(2))
    flow0, flow2 = head_flow(rng, B, H, W), head_flow(rng, B, H, W)
    filt0, filt2 = ((rng.random((B, filter_channels, H, W), dtype=f32) - f32(0.25)).astype(f32) for _ in range(2))
    return ref0, ref2, flow0, flow2, filt0, filt2


def all_head_cases():
    return [(s, fc, c) for s in HEAD_SHAPES for fc in HEAD_FILTERS for c in HEAD_CHANNELS] + [(s, 16, 3) for s in PADDED_SHAPES]
