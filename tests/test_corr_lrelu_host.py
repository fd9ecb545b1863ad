"""CPU suite: the correlation with PWC-Net's LeakyReLU fused in (vfi_correlation_lrelu_*, cabi.correlation_lrelu_*,
fused.corr_lrelu / warp_corr_lrelu / corr_pair_lrelu) without a GPU -- the four symbols and their ctypes rows, the
refusals of the entries and of the wrappers, the helper's backward against torch autograd in float64, the forward
kernel-selection mirror for the new entries (dense and strided outputs) pinned to the source text, and the cases the GPU
file (tests/test_gpu_corr_lrelu.py) relies on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import corr_edges as ce
from tests import corr_lrelu as cl
from tests.test_abi_and_host import built  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = ["batch", "channel", "h", "w", "pad_size", "kernel_size", "max_displacement", "stride1", "stride2", "negative_slope", "stream"]
ENTRIES = {
    "vfi_correlation_lrelu_forward": ["input1", "input2", "output", "output_batch_stride"] + CFG,
    "vfi_correlation_lrelu_forward_pair": ["input1_a", "input2_a", "output_a", "output_a_batch_stride",
                                           "input1_b", "input2_b", "output_b", "output_b_batch_stride"] + CFG,
    "vfi_correlation_lrelu_backward": ["input1", "input2", "y", "y_batch_stride", "gradoutput", "gradoutput_batch_stride",
                                       "gradinput1", "gradinput2"] + CFG,
    "vfi_correlation_lrelu_backward_pair": [
        "input1_a", "input2_a", "y_a", "y_a_batch_stride", "gradoutput_a", "gradoutput_a_batch_stride", "gradinput1_a", "gradinput2_a",
        "input1_b", "input2_b", "y_b", "y_b_batch_stride", "gradoutput_b", "gradoutput_b_batch_stride", "gradinput1_b", "gradinput2_b"] + CFG,
}


# ------------------------------------------------------------------ 1. symbols and table

@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_header_library_and_ctypes_table_agree(built, name):  # noqa: F811
    from vfidkr_amd import cabi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vfi_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "the header does not declare %s" % name
    params = [p.strip() for p in m.group(1).split(",")]
    want = []
    for p in params:
        if "*" in p or p.startswith("vfi_stream_t"):
            want.append(ctypes.c_void_p)
        elif p.startswith("int64_t"):
            want.append(ctypes.c_int64)
        elif p.startswith("float"):
            want.append(ctypes.c_float)
        else:
            assert re.fullmatch(r"int\s+\w+", p), p
            want.append(ctypes.c_int)
    assert [re.search(r"(\w+)$", p).group(1) for p in params] == ENTRIES[name]
    assert cabi.SIGNATURES[name] == want
    assert hasattr(ctypes.CDLL(built.LIB_PATH), name)
    fn = getattr(cabi.lib(), name)
    assert fn.argtypes == want and fn.restype is ctypes.c_int


# ------------------------------------------------------------------ 2. refusals before any launch

P = [ctypes.c_void_p(4096 * (i + 1)) for i in range(12)]        # never dereferenced: every call below returns before a launch
IMG = 81 * 8 * 8


def test_entries_refuse_bad_slopes_strides_and_shapes_without_a_gpu(built):  # noqa: F811
    from vfidkr_amd import cabi
    lib, E = cabi.lib(), cabi.VFI_ERR_SHAPE

    def fwd(slope=0.1, stride=IMG, batch=1, h=8, out=P[2], s1=1):
        return lib.vfi_correlation_lrelu_forward(P[0], P[1], out, stride, batch, 2, h, 8, 4, 1, 4, s1, 1, slope, None)

    def fwd_pair(slope=0.1, sa=IMG, sb=IMG, outb=P[5], batch=1):
        return lib.vfi_correlation_lrelu_forward_pair(P[0], P[1], P[2], sa, P[3], P[4], outb, sb, batch, 2, 8, 8, 4, 1, 4, 1, 1, slope, None)

    def bwd(slope=0.1, ys=IMG, gs=IMG, y=P[2], g1=P[4], s1=1, batch=1):
        return lib.vfi_correlation_lrelu_backward(P[0], P[1], y, ys, P[3], gs, g1, P[5], batch, 2, 8, 8, 4, 1, 4, s1, 1, slope, None)

    def bwd_pair(slope=0.1, a=(P[0], P[1], P[2], IMG, P[3], IMG, P[4], P[5]), b=(P[6], P[7], P[8], IMG, P[9], IMG, P[10], P[11]),
                 batch=1, s1=1):
        return lib.vfi_correlation_lrelu_backward_pair(*a, *b, batch, 2, 8, 8, 4, 1, 4, s1, 1, slope, None)

    for bad in (0.0, -0.1, float("inf"), float("-inf"), float("nan")):
        assert fwd(slope=bad) == E and fwd_pair(slope=bad) == E and bwd(slope=bad) == E and bwd_pair(slope=bad) == E, bad
    # an image stride below the image's own planes
    assert fwd(stride=IMG - 1) == E and fwd_pair(sb=IMG - 1) == E and fwd_pair(sa=0) == E
    assert bwd(ys=IMG - 1) == E and bwd(gs=-IMG) == E
    assert bwd_pair(a=(P[0], P[1], P[2], IMG - 1, P[3], IMG, P[4], P[5])) == E
    assert bwd_pair(b=(P[6], P[7], P[8], IMG, P[9], 5, None, P[11])) == E
    # the twins' checks
    assert fwd(batch=0) == E and fwd(h=0) == E and fwd(out=None) == E and fwd_pair(outb=P[2]) == E and fwd_pair(batch=-1) == E
    assert bwd(batch=0) == E and bwd(s1=2) == E and bwd(y=None) == E and bwd(g1=None) == E
    assert bwd_pair(s1=2) == E and bwd_pair(batch=0) == E
    assert bwd_pair(a=(P[0], P[1], None, IMG, P[3], IMG, P[4], None)) == E             # a requested gradient without its y
    assert bwd_pair(a=(P[0], P[1], P[2], IMG, None, IMG, None, P[5])) == E
    assert bwd_pair(b=(P[6], P[7], P[8], IMG, P[9], IMG, P[4], P[11])) == E            # two equal output pointers
    none8 = (None, None, None, 0, None, 0, None, None)
    assert bwd_pair(a=none8, b=none8) == cabi.VFI_OK                                   # nothing requested
    assert bwd_pair(a=(P[0], P[1], P[2], IMG, P[3], IMG, None, None), b=none8) == cabi.VFI_OK
    assert bwd_pair(a=none8, b=none8, slope=0.0) == E


def test_wrappers_refuse_before_they_touch_a_device(built):  # noqa: F811
    from vfidkr_amd import cabi, fused
    z = torch.zeros
    x, g = z(2, 2, 6, 10), z(2, 81, 6, 10)
    for bad in (0.0, -0.5, float("inf"), float("nan"), 1e39):
        with pytest.raises(RuntimeError, match="negative_slope"):
            cabi.correlation_lrelu_forward(x, x, 4, 1, 4, 1, 1, bad)
        with pytest.raises(RuntimeError, match="negative_slope"):
            cabi.correlation_lrelu_forward_pair(x, x, x, x, 4, 1, 4, 1, 1, bad)
        with pytest.raises(RuntimeError, match="negative_slope"):
            cabi.correlation_lrelu_backward(x, x, g, g, 4, 1, 4, 1, 1, bad)
        with pytest.raises(RuntimeError, match="negative_slope"):
            cabi.correlation_lrelu_backward_pair(x, x, g, g, x, x, g, g, 4, 1, 4, 1, 1, bad)
        with pytest.raises(RuntimeError, match="negative_slope"):
            fused.corr_pair_lrelu(x, x, x, x, negative_slope=bad)
    with pytest.raises(RuntimeError, match="one shape"):
        cabi.correlation_lrelu_forward_pair(x, x, x, z(2, 2, 6, 9), 4, 1, 4, 1, 1, 0.1)
    with pytest.raises(RuntimeError, match="one shape"):
        cabi.correlation_lrelu_forward(x, z(1, 2, 6, 10), 4, 1, 4, 1, 1, 0.1)
    with pytest.raises(RuntimeError, match="one shape"):
        cabi.correlation_lrelu_backward_pair(x, x, g, g, x, z(2, 3, 6, 10), g, g, 4, 1, 4, 1, 1, 0.1)
    with pytest.raises(RuntimeError, match="output dimensions"):
        cabi.correlation_lrelu_backward_pair(x, x, g, z(2, 80, 6, 10), x, x, g, g, 4, 1, 4, 1, 1, 0.1)
    with pytest.raises(RuntimeError, match="output dimensions"):
        cabi.correlation_lrelu_backward(x, x, z(2, 81, 6, 9), g, 4, 1, 4, 1, 1, 0.1)
    # out=: the shape, then dense planes
    buf = z(2, 90, 6, 10)
    for bad_out in (buf[:, 3:84:1, :, ::1][:, :, :, :9], buf[:, 0:81, :5]):
        with pytest.raises(RuntimeError, match="output dimensions"):
            cabi.correlation_lrelu_forward(x, x, 4, 1, 4, 1, 1, 0.1, out=bad_out)
    wide = z(2, 162, 6, 10)
    for bad_out in (wide[:, ::2], z(2, 81, 6, 20)[:, :, :, ::2], z(2, 81, 12, 10)[:, :, ::2], z(2, 6, 10, 81).permute(0, 3, 1, 2)):
        assert tuple(bad_out.shape) == (2, 81, 6, 10)
        with pytest.raises(RuntimeError, match="dense planes"):
            cabi.correlation_lrelu_forward(x, x, 4, 1, 4, 1, 1, 0.1, out=bad_out)
        with pytest.raises(RuntimeError, match="dense planes"):
            cabi.correlation_lrelu_forward_pair(x, x, x, x, 4, 1, 4, 1, 1, 0.1, out=(None, bad_out))
    # a channel slice is dense planes: the refusal it meets is the device's
    assert cabi._dense_planes(buf[:, 3:84]) and cabi._planes(buf[:, 3:84])[1] == 90 * 60
    with pytest.raises(RuntimeError, match="no CPU path"):
        cabi.correlation_lrelu_forward(x, x, 4, 1, 4, 1, 1, 0.1, out=buf[:, 3:84])
    with pytest.raises(RuntimeError, match="no CPU path"):
        cabi.correlation_lrelu_backward(x, x, g, buf[:, :81], 4, 1, 4, 1, 1, 0.1)
    # under autograd out= is refused
    c = z(2, 2, 6, 10, requires_grad=True)
    for call in (lambda: fused.corr_lrelu(c, x, out=buf[:, :81]), lambda: fused.warp_corr_lrelu(c, x, z(2, 2, 6, 10), out=buf[:, :81]),
                 lambda: fused.corr_pair_lrelu(c, x, x, x, out=(buf[:, :81], None))):
        with pytest.raises(RuntimeError, match="out= is for inference"):
            call()


def test_planes_keeps_a_batch_strided_view_and_copies_the_rest():
    from vfidkr_amd import cabi
    big = torch.arange(2 * 90 * 3 * 5, dtype=torch.float32).view(2, 90, 3, 5)
    v = big.narrow(1, 0, 81)
    t, stride = cabi._planes(v)
    assert t is v and stride == 90 * 15
    t, stride = cabi._planes(big[:, ::2][:, :45])
    assert t.is_contiguous() and stride == 45 * 15
    t, stride = cabi._planes(torch.zeros(1, 81, 3, 5).expand(2, 81, 3, 5))                 # batch stride 0: images overlap
    assert t.is_contiguous() and stride == 81 * 15
    t, stride = cabi._planes(big[:1, 4:85])                                                # one image: no stride to speak of
    assert t.data_ptr() == big[:1, 4:85].data_ptr() and stride == 81 * 15


# ------------------------------------------------------------------ 3. the helper against torch autograd, float64

def test_helper_backward_equals_autograd_of_the_float64_restatement():
    rng = np.random.default_rng(5)
    shape = (1, 2, 6, 7)
    for _ in range(40):                                     # values kept away from 0: the mask is unambiguous
        f1, f2 = (rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape) for _ in range(2))
        f1, f2 = f1.astype(np.float32), f2.astype(np.float32)
        pre = cl.corr64(torch.from_numpy(f1), torch.from_numpy(f2))
        if (pre[pre != 0].abs() > 1e-3).all():
            break
    else:
        raise AssertionError("no input with every pre-activation away from zero")
    g = rng.standard_normal((1, 81, 6, 7)).astype(np.float32)
    x1, x2 = (torch.from_numpy(f).double().requires_grad_(True) for f in (f1, f2))
    y64 = torch.nn.functional.leaky_relu(cl.corr64(x1, x2), cl.SLOPE)
    want1, want2 = torch.autograd.grad(y64, (x1, x2), torch.from_numpy(g).double())
    y = cl.expected_forward(f1, f2, ce.PWC)
    assert np.allclose(y, y64.detach().numpy(), rtol=1e-6, atol=1e-7)
    assert (y < 0).any() and (y > 0).any() and np.array_equal(y > 0, y64.detach().numpy() > 0)
    got1, got2 = cl.expected_backward(f1, f2, y, g, ce.PWC)
    for got, want in ((got1, want1.numpy()), (got2, want2.numpy())):
        # float32 sums of 81 terms against float64: 1e-6 relative to the gradient's scale
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max(), np.abs(got - want).max() / np.abs(want).max()


def test_masked_is_torchs_leaky_relu_backward_bit_for_bit():
    rng = np.random.default_rng(6)
    x = rng.standard_normal(4000).astype(np.float32)
    x[:7] = (0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45)
    g = rng.standard_normal(4000).astype(np.float32)
    g[7:10] = (np.inf, -np.inf, np.nan)
    for slope in (0.1, 0.2, 1.0):
        xt = torch.from_numpy(x).requires_grad_(True)
        y = torch.nn.functional.leaky_relu(xt, slope)
        (want,) = torch.autograd.grad(y, xt, torch.from_numpy(g))
        # the mask through the OUTPUT's sign is the mask through the input's
        assert ce.same_bits_nan_aware(cl.masked(y.detach().numpy(), g, slope), want.numpy())
        assert ce.same_bits_nan_aware(cl.leaky(x, slope), y.detach().numpy())
    assert np.array_equal(cl.leaky(x, 1.0).view(np.uint32)[~np.isnan(x)], x.view(np.uint32)[~np.isnan(x)])


# ------------------------------------------------------------------ 4. the dispatch mirror for the new entries

def test_new_entries_share_the_dispatch_and_a_stride_counts_as_a_pointer():
    """The fused entries call correlation_forward_items (the chain tests/test_corr_edges_host.py pins) with their
    epilogue; the only thing an epilogue adds to the dispatch is its strides' bits in out_bits."""
    text = " ".join(ce.source(ce.SRC).split())
    body = " ".join(ce.function_body("correlation_forward_items").split())
    assert ce.source_branches("correlation_forward_items") == ce.BRANCHES["correlation_forward_items"]
    assert "out_bits |= reinterpret_cast<uintptr_t>(outs[k]) | corr_stride_bits(epi, k);" in body
    assert "static uintptr_t corr_stride_bits(const CorrPlain&, int) { return 0; }" in text
    assert "static uintptr_t corr_stride_bits(const CorrLrelu& e, int item) { return (uintptr_t)e.stride[item] * sizeof(float); }" in text
    assert body.count("out_bits") == 4                      # declared, gathered, and the two tests the mirror restates
    assert "(out_bits & 7) == 0" in ce.EXPRS["correlation_forward_items"]["aligned"]
    assert "aligned && (out_bits & 15) == 0 &&" in ce.BRANCHES["correlation_forward_items"][1][0]
    for entry in ("vfi_correlation_lrelu_forward", "vfi_correlation_lrelu_forward_pair"):
        b = " ".join(ce.function_body(entry).split())
        assert "return correlation_forward_items(" in b and "CorrLrelu{{" in b and "hipLaunchKernelGGL" not in b
    for entry in ("vfi_correlation_forward", "vfi_correlation_forward_pair"):
        assert "CorrPlain{});" in " ".join(ce.function_body(entry).split())
    # every launch of the chain passes the epilogue it was given
    assert body.count("hipLaunchKernelGGL(") == 6 and body.count(", epi);") == 5 and body.count(", one);") == 1
    # backward, float32 and bfloat16: the masked kernels are launched where the plain ones are -- each file names its
    # kernels once, masked beside plain, and the one launcher of every storage type launches each kind in one place
    f32 = " ".join(ce.struct_body("CorrBwdF32").split())
    assert f32.count("if (act) hipLaunchKernelGGL(second ? corr_lrelu_backward_k1<true> : corr_lrelu_backward_k1<false>,") == 1
    assert f32.count("else hipLaunchKernelGGL(second ? corr_backward_k1<true> : corr_backward_k1<false>,") == 1
    assert f32.count("if (act) hipLaunchKernelGGL(second ? corr_lrelu_backward<true> : corr_lrelu_backward<false>,") == 1
    assert f32.count("else hipLaunchKernelGGL(second ? corr_backward<true> : corr_backward<false>,") == 1
    assert "if (masks) hipLaunchKernelGGL(corr_lrelu_backward_k1_pair," in f32 and "else hipLaunchKernelGGL(corr_backward_k1_pair," in f32
    assert f32.count("hipLaunchKernelGGL(") == 6
    bf16 = " ".join(ce.struct_body("CorrBwdBf16", ce.SRC_BF16).split())
    assert bf16.count("if (act) hipLaunchKernelGGL((second ? corr_backward_k1_bf16<true, Mask> : corr_backward_k1_bf16<false, Mask>),") == 1
    assert bf16.count("else hipLaunchKernelGGL((second ? corr_backward_k1_bf16<true, CorrBf16Grad> : corr_backward_k1_bf16<false, CorrBf16Grad>),") == 1
    assert bf16.count("if (act) hipLaunchKernelGGL((second ? corr_backward_bf16<true, Mask> : corr_backward_bf16<false, Mask>),") == 1
    assert bf16.count("else hipLaunchKernelGGL((second ? corr_backward_bf16<true, CorrBf16Grad> : corr_backward_bf16<false, CorrBf16Grad>),") == 1
    assert "if (masks) hipLaunchKernelGGL(corr_lrelu_backward_k1_pair_bf16," in bf16 and "else hipLaunchKernelGGL(corr_backward_k1_pair_bf16," in bf16
    assert bf16.count("hipLaunchKernelGGL(") == 6
    one = " ".join(ce.function_body("corr_backward_one", ce.BWD).split())
    assert one.count("K::k1(second, act,") == 1 and one.count("K::generic(second, act,") == 1 and "hipLaunchKernelGGL" not in one
    pair = " ".join(ce.function_body("corr_backward_pair", ce.BWD).split())
    assert pair.count("K::pair(roles, acts ? &masks : nullptr,") == 1 and pair.count("corr_backward_one<K>(") == 1
    assert "acts ? &act : nullptr);" in pair and "hipLaunchKernelGGL" not in pair
    # the entries only forward
    for src, k, suffix in ((ce.SRC, "CorrBwdF32", ""), (ce.SRC_BF16, "CorrBwdBf16", "_bf16")):
        for entry in ("vfi_correlation_backward_pair", "vfi_correlation_lrelu_backward_pair"):
            b = " ".join(ce.function_body(entry + suffix, src).split())
            assert "return corr_backward_pair<%s>(" % k in b and "hipLaunchKernelGGL" not in b
        for entry in ("vfi_correlation_backward", "vfi_correlation_lrelu_backward"):
            b = " ".join(ce.function_body(entry + suffix, src).split())
            assert "return corr_backward_both<%s>(" % k in b and "hipLaunchKernelGGL" not in b


def test_mirror_on_dense_and_strided_outputs():
    k = cl.selected_kernel_out
    for name, (shape, cfg, dense, offset) in ce.F32_CASES.items():
        kw = dict(k=cfg[1], md=cfg[2], s1=cfg[3], s2=cfg[4])
        _, oh, ow = ce.out_dims(shape[2], shape[3], *cfg)
        for nitems in (1, 2):
            assert k(*shape, cfg[0], nitems=nitems, out_bits=81 * oh * ow * 4, **kw) == dense, name      # a dense image stride
            assert k(*shape, cfg[0], nitems=nitems, out_bits=4, **kw) == offset, name
    # buf[:, 3:84] of a (B, 90, oh, ow) buffer: whether the slice keeps 16-byte alignment depends on oh * ow
    flat, rows2, quad = (ce.F32_CASES[n][0] for n in ("flat", "rows2", "quad"))
    assert cl.slice_bits(rows2, ce.PWC, 3) % 16 == 0 and k(*rows2, 4, out_bits=cl.slice_bits(rows2, ce.PWC, 3)) == ce.ROWS2
    assert cl.slice_bits(quad, ce.PWC, 3) % 16 == 0 and k(*quad, 4, out_bits=cl.slice_bits(quad, ce.PWC, 3)) == ce.QUAD
    assert cl.slice_bits(flat, ce.PWC, 3) % 8 == 0 and k(*flat, 4, out_bits=cl.slice_bits(flat, ce.PWC, 3)) == ce.FLAT
    # 8-byte but not 16-byte alignment: four pixels per lane give way to two; 4-byte: to the one-float kernels
    assert k(*quad, 4, out_bits=8) == ce.ROWS2 and k(*quad, 4, nitems=2, out_bits=8) == ce.ROWS2
    assert k(*quad, 4, out_bits=4) == ce.K1 and k(*rows2, 4, out_bits=8) == ce.ROWS2 and k(*rows2, 4, out_bits=12) == ce.ROWS
    assert k(*flat, 4, out_bits=4) == ce.FLAT and k(2, 5, 12, 14, 3, out_bits=4, k=3, s2=2) == "corr_forward_generic"


def test_strided_gpu_cases_break_alignment_as_the_gpu_file_says():
    """tests/test_gpu_corr_lrelu.py writes into buf[:, 3:84] of a (B, 90, oh, ow) buffer whose images lie 90 * oh * ow
    elements apart (the slice keeps 16-byte alignment), then one element further apart (no store wider than 4 bytes is
    aligned in the second image), and two further apart (8 bytes are, 16 are not)."""
    for name, kept, by8, by4 in (("rows2", ce.ROWS2, ce.ROWS2, ce.ROWS), ("quad", ce.QUAD, ce.ROWS2, ce.K1), ("flat", ce.FLAT, ce.FLAT, ce.FLAT)):
        shape, cfg = ce.F32_CASES[name][:2]
        _, oh, ow = ce.out_dims(shape[2], shape[3], *cfg)
        first = 3 * oh * ow * 4
        for pad_elems, want in ((0, kept), (2, by8), (1, by4)):
            bits = first | ((cl.CAT * oh * ow + pad_elems) * 4)
            assert bits % 16 == (0, 4, 8)[pad_elems]
            assert cl.selected_kernel_out(*shape, cfg[0], out_bits=bits) == want, (name, pad_elems)


# ------------------------------------------------------------------ 5. the cases of the GPU file

def test_backward_cases_reach_their_channel_groups():
    text = " ".join(ce.source(ce.SRC).split())
    assert ("int groups = (int)std::min<int64_t>(channel, std::max<int64_t>(1, (2048 + (int64_t)tiles * batch - 1) / "
            "((int64_t)tiles * batch)));") in text
    assert "*ch_per_group = (channel + groups - 1) / groups; groups = (channel + *ch_per_group - 1) / *ch_per_group;" in text
    one, several = (cl.BACKWARD_CASES[n][0] for n in ("one_channel_per_group", "several_channels_per_group"))
    for roles in (1, 2, 3, 4):                              # the single entry; the pair with 2, 3 or 4 gradients
        assert cl.backward_groups(cl.tiles_of(one), one[0] * roles, one[1])[1] == 1
        groups, per = cl.backward_groups(cl.tiles_of(several), several[0] * roles, several[1])
        assert per > 1 and groups > 1 and several[1] % per, (roles, groups, per)       # a ragged last group too
    for shape in (one, several):
        assert shape[3] % 64 and shape[2] % 4 and cl.tiles_of(shape) > 1
    assert cl.BACKWARD_CASES["generic"][1] == (3, 3, 4, 1, 2)


def test_forward_cases_exercise_both_branches_of_the_activation():
    """Standard-normal inputs: about half the outputs whose two taps lie in the frame are negative and half positive.
    Outputs with a tap in the zero padding are exact zeros; in flat_pad8 (pad 8 on an 8 x 33 frame) they are 73 % of the
    outputs, so the quarter is asked of all outputs everywhere else and of the in-frame outputs everywhere."""
    for name in cl.FORWARD_CASES:
        f1, f2, cfg = cl.forward_inputs(name, False)
        y = cl.forward_expected(name, False)
        inside = cl.expected_forward(np.ones_like(f1), np.ones_like(f2), cfg) > 0
        assert (y[inside] < 0).mean() >= 0.4 and (y[inside] > 0).mean() >= 0.4, name
        if name != "flat_pad8":
            assert (y < 0).mean() >= 0.25 and (y > 0).mean() >= 0.25, name
        # the all-zero pixel: 81 exact zeros inside the frame
        zero = (y == 0) & inside
        assert zero.sum() >= (9 if cfg[1] == 3 else 50), (name, zero.sum())
        assert not np.signbit(y[zero]).any()
        want = cl.forward_expected(name, True)
        assert np.isnan(want).any() and np.isinf(want).any() and (want < 0).any()
