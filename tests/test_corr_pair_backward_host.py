"""CPU suite: the paired correlation backward (vfi_correlation_backward_pair, cabi.correlation_backward_pair,
fused.corr_pair's autograd Function) without a GPU -- the symbol and its ctypes row, the entry's refusals before any launch,
the wrappers' refusals, the autograd wiring on a stubbed cabi, and the compiled kernels' registers and scratch."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests.test_abi_and_host import built  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video-frame-interpolation-based-on-deformable-kernel-region_amd")
NAME = "vfi_correlation_backward_pair"


# ------------------------------------------------------------------ 1. symbol and table

def test_header_library_and_ctypes_table_agree(built):  # noqa: F811
    from vfidkr_amd import cabi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vfi_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, text)
    assert m, "the header does not declare %s" % NAME
    params = [p.strip() for p in m.group(1).split(",")]
    want = []
    for p in params:
        if "*" in p or p.startswith("vfi_stream_t"):
            want.append(ctypes.c_void_p)
        else:
            assert re.fullmatch(r"int\s+\w+", p), p
            want.append(ctypes.c_int)
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    assert names == ["input1_a", "input2_a", "gradoutput_a", "gradinput1_a", "gradinput2_a",
                     "input1_b", "input2_b", "gradoutput_b", "gradinput1_b", "gradinput2_b",
                     "batch", "channel", "h", "w", "pad_size", "kernel_size", "max_displacement", "stride1", "stride2", "stream"]
    assert NAME in cabi.SIGNATURES and cabi.SIGNATURES[NAME] == want
    assert hasattr(ctypes.CDLL(built.LIB_PATH), NAME)
    fn = getattr(cabi.lib(), NAME)
    assert fn.argtypes == want and fn.restype is ctypes.c_int


# ------------------------------------------------------------------ 2. refusals before any launch

def test_entry_refuses_bad_arguments_and_accepts_nothing_requested_without_a_gpu(built):  # noqa: F811
    from vfidkr_amd import cabi
    fn = getattr(cabi.lib(), NAME)
    E = cabi.VFI_ERR_SHAPE
    # never dereferenced: every call below returns before a launch
    i1a, i2a, ga, o1a, o2a, i1b, i2b, gb, o1b, o2b = (ctypes.c_void_p(4096 * (i + 1)) for i in range(10))

    def call(a=(i1a, i2a, ga, o1a, o2a), b=(i1b, i2b, gb, o1b, o2b), batch=1, channel=2, h=8, w=8, pad=4, k=1, md=4, s1=1, s2=1):
        return fn(*a, *b, batch, channel, h, w, pad, k, md, s1, s2, None)

    assert call(batch=0) == E and call(batch=-1) == E and call(channel=0) == E and call(h=0) == E and call(w=-2) == E
    assert call(s1=2) == E
    assert call(k=0) == E and call(h=2, w=2, pad=0) == E                     # what corr_check refuses elsewhere
    # a requested gradient whose item lacks an input or its gradoutput
    assert call(a=(None, i2a, ga, o1a, o2a)) == E and call(a=(i1a, None, ga, o1a, None)) == E
    assert call(a=(i1a, i2a, None, None, o2a)) == E
    assert call(b=(None, i2b, gb, o1b, None)) == E and call(b=(i1b, i2b, None, None, o2b)) == E
    assert call(a=(None, None, None, None, None), b=(i1b, None, gb, None, o2b)) == E
    # two equal output pointers, within an item and across the items
    assert call(a=(i1a, i2a, ga, o1a, o1a)) == E and call(b=(i1b, i2b, gb, o1a, o2b)) == E
    assert call(b=(i1b, i2b, gb, o1b, o2a)) == E and call(b=(i1b, i2b, gb, None, o2a)) == E
    # the refusals hold in a configuration that would take the per-gradient launches too
    assert call(pad=3, k=3, md=4, s2=2, s1=2) == E and call(pad=3, k=3, md=4, s2=2, a=(i1a, i2a, None, o1a, None)) == E
    # nothing requested: fine, with or without the inputs
    none5 = (None,) * 5
    assert call(a=(i1a, i2a, ga, None, None), b=(i1b, i2b, gb, None, None)) == cabi.VFI_OK
    assert call(a=none5, b=none5) == cabi.VFI_OK
    assert call(a=none5, b=none5, pad=3, k=3, md=4, s2=2) == cabi.VFI_OK


# ------------------------------------------------------------------ 3. wrapper refusals

def test_wrappers_refuse_cpu_tensors_and_mismatched_shapes(built):  # noqa: F811
    from vfidkr_amd import cabi, fused
    z = torch.zeros
    x, g = z(1, 2, 6, 10), z(1, 81, 6, 10)
    with pytest.raises(RuntimeError, match="one shape"):
        cabi.correlation_backward_pair(x, x, g, x, z(1, 2, 6, 9), g, 4, 1, 4, 1, 1)
    with pytest.raises(RuntimeError, match="one shape"):
        cabi.correlation_backward_pair(x, z(2, 2, 6, 10), g, x, x, g, 4, 1, 4, 1, 1)
    with pytest.raises(RuntimeError, match="output dimensions"):
        cabi.correlation_backward_pair(x, x, g, x, x, z(1, 80, 6, 10), 4, 1, 4, 1, 1)
    with pytest.raises(RuntimeError, match="output dimensions"):
        cabi.correlation_backward_pair(x, x, z(1, 81, 6, 9), x, x, None, 4, 1, 4, 1, 1, want=(True, False, False, False))
    with pytest.raises(RuntimeError, match="no CPU path"):
        cabi.correlation_backward_pair(x, x, g, x, x, g, 4, 1, 4, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        cabi.correlation_backward_pair(x, x, None, x, x, g, 4, 1, 4, 1, 1, want=(False, False, False, True))
    for wants_grad in (False, True):
        c = z(1, 2, 6, 10, requires_grad=wants_grad)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fused.corr_pair(c, x, x, c)
        with pytest.raises(RuntimeError):
            fused.corr_pair(c, x, x, z(1, 2, 6, 9))


# ------------------------------------------------------------------ 4. autograd wiring on a stubbed cabi

class _Stub:
    """correlation_forward_pair / correlation_backward_pair on CPU tensors: the forward returns two fresh cost volumes, the
    backward records its call and returns a constant per gradient (1, 2, 3, 4) where the real wrapper would return a tensor"""

    def __init__(self):
        self.forward, self.backward = 0, []

    def fwd(self, a1, a2, b1, b2, pad, k, md, s1, s2):
        assert (pad, k, md, s1, s2) == (4, 1, 4, 1, 1)
        self.forward += 1
        b, _, h, w = a1.shape
        return torch.full((b, 81, h, w), 1.0), torch.full((b, 81, h, w), 2.0)

    def bwd(self, a1, a2, ga, b1, b2, gb, pad, k, md, s1, s2, want=(True,) * 4):
        assert (pad, k, md, s1, s2) == (4, 1, 4, 1, 1)
        self.backward.append(((a1, a2, b1, b2), (ga, gb), tuple(want)))
        gs = (ga, ga, gb, gb)
        return tuple(torch.full_like(t, i + 1.0) if want[i] and gs[i] is not None else None for i, t in enumerate((a1, a2, b1, b2)))


@pytest.fixture
def stubbed(monkeypatch):
    from vfidkr_amd import cabi, fused
    stub = _Stub()
    monkeypatch.setattr(cabi, "correlation_forward_pair", stub.fwd)
    monkeypatch.setattr(cabi, "correlation_backward_pair", stub.bwd)
    return fused, stub


def _inputs(pattern):
    return [torch.rand(1, 3, 5, 6, requires_grad=r) for r in pattern]


@pytest.mark.parametrize("pattern", [(True, True, True, True), (False, True, False, True), (True, True, False, False),
                                     (False, False, True, False)])
def test_backward_is_one_call_whose_want_is_the_requires_grad_pattern(stubbed, pattern):
    fused, stub = stubbed
    xs = _inputs(pattern)
    out_a, out_b = fused.corr_pair(*xs)
    assert out_a.grad_fn is not None and out_b.grad_fn is out_a.grad_fn and stub.forward == 1
    wa, wb = torch.rand(1, 81, 5, 6), torch.rand(1, 81, 5, 6)
    ((out_a * wa).sum() + (out_b * wb).sum()).backward()
    assert len(stub.backward) == 1
    saved, (ga, gb), want = stub.backward[0]
    assert want == pattern and all(s is x or torch.equal(s, x) for s, x in zip(saved, xs))
    assert torch.equal(ga, wa) and torch.equal(gb, wb)
    for i, x in enumerate(xs):
        if pattern[i]:
            assert torch.equal(x.grad, torch.full_like(x, i + 1.0))
        else:
            assert x.grad is None


def test_an_unused_output_arrives_as_none_and_its_item_gets_no_gradient(stubbed):
    fused, stub = stubbed
    xs = _inputs((True, True, True, True))
    out_a, out_b = fused.corr_pair(*xs)
    out_a.sum().backward()
    assert len(stub.backward) == 1
    _, (ga, gb), want = stub.backward[0]
    assert ga is not None and gb is None and want == (True,) * 4
    assert xs[0].grad is not None and xs[1].grad is not None and xs[2].grad is None and xs[3].grad is None
    # the other output alone, in a second graph
    ys = _inputs((True, True, True, True))
    (fused.corr_pair(*ys)[1] * 3.0).sum().backward()
    assert len(stub.backward) == 2 and stub.backward[1][1][0] is None and stub.backward[1][1][1] is not None
    assert ys[0].grad is None and ys[1].grad is None and torch.equal(ys[3].grad, torch.full_like(ys[3], 4.0))


def test_inference_path_reaches_no_autograd_function(stubbed, monkeypatch):
    fused, stub = stubbed

    def refuse(*a, **k):
        raise AssertionError("the autograd Function was reached")
    monkeypatch.setattr(fused._CorrPair, "apply", refuse)
    xs = _inputs((False,) * 4)
    outs = fused.corr_pair(*xs)
    assert all(o.grad_fn is None and not o.requires_grad for o in outs)
    ys = _inputs((True,) * 4)
    with torch.no_grad():
        outs = fused.corr_pair(*ys)
    assert all(o.grad_fn is None and not o.requires_grad for o in outs)
    assert stub.forward == 2 and not stub.backward


# ------------------------------------------------------------------ 5. kernel metadata

def _makefile_flags():
    text = open(os.path.join(PKG, "csrc", "Makefile")).read()
    flags = re.search(r"^HIPFLAGS\s*\?=\s*(.*)$", text, flags=re.M).group(1)
    return flags.replace("$(ARCH)", "gfx950").split()


def _waves_per_simd(vgprs):
    """512 registers per lane and SIMD, allocated in granules of 8, at most 8 waves"""
    return min(8, 512 // (-(-vgprs // 8) * 8))


def test_pair_kernel_has_no_scratch_and_the_single_kernels_occupancy(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "correlation.s"
    subprocess.run([hipcc] + _makefile_flags() + ["-S", "--cuda-device-only", os.path.join(PKG, "csrc", "correlation.hip"),
                                                  "-o", str(out)], check=True, cwd=os.path.join(PKG, "csrc"))
    asm = out.read_text()
    meta = {}
    for block in re.split(r"^  - \.agpr_count:", asm, flags=re.M)[1:]:
        name = re.search(r"^    \.name:\s+(\S+)", block, flags=re.M).group(1)       # (four spaces: the kernel's keys, not an argument's)
        meta[name] = {k: int(re.search(r"^    \.%s:\s+(\d+)" % k, block, flags=re.M).group(1))
                      for k in ("private_segment_fixed_size", "vgpr_count", "sgpr_count", "group_segment_fixed_size")}
        meta[name]["agpr_count"] = int(block.split()[0])
    pair = [n for n in meta if re.search(r"corr_backward_k1_pair", n)]
    single = sorted(n for n in meta if re.search(r"corr_backward_k1ILb[01]E", n))
    assert len(pair) == 1 and len(single) == 2, (pair, single)          # both existing instances are still kernels
    assert not re.search(r"corr_backward(?:_k1)?_f16", pair[0])
    p = meta[pair[0]]
    print({n: meta[n] for n in pair + single})
    assert p["private_segment_fixed_size"] == 0
    assert all(meta[n]["private_segment_fixed_size"] == 0 for n in single)
    assert p["group_segment_fixed_size"] == meta[single[0]]["group_segment_fixed_size"] == 2 * 12 * 72 * 4     # one window pair
    waves = {n: _waves_per_simd(meta[n]["vgpr_count"] + meta[n]["agpr_count"]) for n in pair + single}
    assert waves[pair[0]] >= min(waves[n] for n in single), waves
    assert p["vgpr_count"] >= 81                                          # the 81 gradOutput values live in registers
