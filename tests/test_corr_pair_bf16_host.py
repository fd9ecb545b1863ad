"""CPU suite: the paired correlation on bfloat16 tensors (vfi_correlation_[lrelu_]forward_pair_bf16 / _backward_pair_bf16,
the dtype dispatch of cabi.correlation_*_pair, fused._CorrPair / _CorrPairLrelu / corr_pair_lrelu on bfloat16) without a GPU
-- the four symbols and their ctypes rows, the entries' refusals before any launch, the wrappers' dispatch on a recording
library, and the autograd wiring on a stubbed cabi."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_abi_and_host import built  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = ["batch", "channel", "h", "w", "pad_size", "kernel_size", "max_displacement", "stride1", "stride2"]
ENTRIES = {
    "vfi_correlation_forward_pair_bf16": ["input1_a", "input2_a", "output_a", "input1_b", "input2_b", "output_b"] + CFG + ["stream"],
    "vfi_correlation_lrelu_forward_pair_bf16": ["input1_a", "input2_a", "output_a", "output_a_batch_stride",
                                                "input1_b", "input2_b", "output_b", "output_b_batch_stride"] + CFG + ["negative_slope", "stream"],
    "vfi_correlation_backward_pair_bf16": ["input1_a", "input2_a", "gradoutput_a", "gradinput1_a", "gradinput2_a",
                                           "input1_b", "input2_b", "gradoutput_b", "gradinput1_b", "gradinput2_b"] + CFG + ["stream"],
    "vfi_correlation_lrelu_backward_pair_bf16": [
        "input1_a", "input2_a", "y_a", "y_a_batch_stride", "gradoutput_a", "gradoutput_a_batch_stride", "gradinput1_a", "gradinput2_a",
        "input1_b", "input2_b", "y_b", "y_b_batch_stride", "gradoutput_b", "gradoutput_b_batch_stride", "gradinput1_b", "gradinput2_b"]
    + CFG + ["negative_slope", "stream"],
}


# ------------------------------------------------------------------ 1. symbols and table

def _header_params(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vfi_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "the header does not declare %s" % name
    return [p.strip() for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_header_library_and_ctypes_table_agree(built, name):  # noqa: F811
    from vfidkr_amd import cabi
    params = _header_params(name)
    want = []
    for p in params:
        if "*" in p or p.startswith("vfi_stream_t"):
            assert not p.startswith(("float", "const float")), p      # void* tensors
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
    # the argument list of the float32 pair entry, tensor types aside
    f32 = _header_params(name[:-len("_bf16")])
    assert [re.search(r"(\w+)$", p).group(1) for p in f32] == ENTRIES[name]
    assert cabi.SIGNATURES[name[:-len("_bf16")]] == want
    assert hasattr(ctypes.CDLL(built.LIB_PATH), name)
    fn = getattr(cabi.lib(), name)
    assert fn.argtypes == want and fn.restype is ctypes.c_int


# ------------------------------------------------------------------ 2. refusals before any launch

P = [ctypes.c_void_p(4096 * (i + 1)) for i in range(12)]        # never dereferenced: every call below returns before a launch
IMG = 81 * 8 * 8
BAD_SLOPES = (0.0, -0.1, float("inf"), float("-inf"), float("nan"))


def test_forward_entries_refuse_before_any_launch(built):  # noqa: F811
    from vfidkr_amd import cabi
    lib, E = cabi.lib(), cabi.VFI_ERR_SHAPE

    def fwd(a=(P[0], P[1], P[2]), b=(P[3], P[4], P[5]), batch=1, channel=2, h=8, w=8, pad=4, k=1, md=4, s1=1, s2=1):
        return lib.vfi_correlation_forward_pair_bf16(*a, *b, batch, channel, h, w, pad, k, md, s1, s2, None)

    def lrelu(slope=0.1, sa=IMG, sb=IMG, a=(P[0], P[1], P[2]), b=(P[3], P[4], P[5]), batch=1, channel=2, h=8, w=8, pad=4, k=1, s2=1):
        return lib.vfi_correlation_lrelu_forward_pair_bf16(*a, sa, *b, sb, batch, channel, h, w, pad, k, 4, 1, s2, slope, None)

    for call in (fwd, lrelu):
        assert call(batch=0) == E and call(batch=-1) == E and call(channel=0) == E and call(h=0) == E and call(w=-2) == E
        assert call(k=0) == E and call(h=2, w=2, pad=0) == E                       # invalid parameters, no output pixel
        assert call(b=(P[3], P[4], P[2])) == E                                      # two equal outputs
        for i in range(3):                                                          # a NULL tensor, either item
            assert call(a=tuple(None if j == i else P[j] for j in range(3))) == E
            assert call(b=tuple(None if j == i else P[3 + j] for j in range(3))) == E
        assert call(pad=3, k=3, s2=2, b=(P[3], P[4], P[2])) == E                    # the same in the generic kernel's configuration
    for bad in BAD_SLOPES:
        assert lrelu(slope=bad) == E, bad
    assert lrelu(sa=IMG - 1) == E and lrelu(sb=IMG - 1) == E and lrelu(sa=0) == E and lrelu(sb=-IMG) == E


def test_backward_entries_refuse_before_any_launch_and_accept_nothing_requested(built):  # noqa: F811
    from vfidkr_amd import cabi
    lib, E = cabi.lib(), cabi.VFI_ERR_SHAPE
    A, B = (P[0], P[1], P[2], P[3], P[4]), (P[5], P[6], P[7], P[8], P[9])        # input1, input2, gradoutput, gradinput1, gradinput2

    def bwd(a=A, b=B, batch=1, channel=2, h=8, w=8, pad=4, k=1, md=4, s1=1, s2=1):
        return lib.vfi_correlation_backward_pair_bf16(*a, *b, batch, channel, h, w, pad, k, md, s1, s2, None)

    def lrelu(a=A, b=B, ya=(P[10], IMG), yb=(P[11], IMG), gsa=IMG, gsb=IMG, slope=0.1, batch=1, channel=2, h=8, w=8, pad=4, k=1,
              md=4, s1=1, s2=1):
        return lib.vfi_correlation_lrelu_backward_pair_bf16(a[0], a[1], *ya, a[2], gsa, a[3], a[4], b[0], b[1], *yb, b[2], gsb, b[3], b[4],
                                                            batch, channel, h, w, pad, k, md, s1, s2, slope, None)

    none5 = (None,) * 5
    for call in (bwd, lrelu):
        assert call(batch=0) == E and call(batch=-1) == E and call(channel=0) == E and call(h=0) == E and call(w=-2) == E
        assert call(s1=2) == E and call(k=0) == E and call(h=2, w=2, pad=0) == E
        # a requested gradient whose item lacks an input or its gradoutput
        assert call(a=(None, P[1], P[2], P[3], P[4])) == E and call(a=(P[0], None, P[2], P[3], None)) == E
        assert call(a=(P[0], P[1], None, None, P[4])) == E and call(b=(None, P[6], P[7], P[8], None)) == E
        assert call(a=none5, b=(P[5], None, P[7], None, P[9])) == E
        # two equal outputs, within an item and across the items
        assert call(a=(P[0], P[1], P[2], P[3], P[3])) == E and call(b=(P[5], P[6], P[7], P[3], P[9])) == E
        assert call(b=(P[5], P[6], P[7], None, P[4])) == E
        # the refusals hold where the launches would be one per gradient
        assert call(pad=3, k=3, s2=2, s1=2) == E and call(pad=3, k=3, s2=2, a=(P[0], P[1], None, P[3], None)) == E
        # nothing requested: fine, with or without the inputs
        assert call(a=(P[0], P[1], P[2], None, None), b=(P[5], P[6], P[7], None, None)) == cabi.VFI_OK
        assert call(a=none5, b=none5) == cabi.VFI_OK
        assert call(a=none5, b=none5, pad=3, k=3, s2=2) == cabi.VFI_OK
    for bad in BAD_SLOPES:
        assert lrelu(slope=bad) == E, bad
        assert lrelu(a=none5, b=none5, slope=bad) == E, bad
    assert lrelu(ya=(P[10], IMG - 1)) == E and lrelu(gsa=IMG - 1) == E and lrelu(yb=(P[11], 5)) == E and lrelu(gsb=-IMG) == E
    assert lrelu(ya=(None, IMG)) == E and lrelu(yb=(None, IMG), b=(P[5], P[6], P[7], None, P[9])) == E      # a missing y
    assert lrelu(ya=(None, 0), a=(P[0], P[1], P[2], None, None), b=(P[5], P[6], P[7], None, None)) == cabi.VFI_OK     # ... of an item nothing is asked of
    assert lrelu(a=none5, b=none5, ya=(None, 0), yb=(None, 0), gsa=0, gsb=0) == cabi.VFI_OK


# ------------------------------------------------------------------ 3. cabi's dispatch, library stubbed

class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            if name == "vfi_correlation_output_dims":
                args[7]._obj.value, args[8]._obj.value, args[9]._obj.value = 81, args[0], args[1]
            return 0
        return fn


class _FakeCuda:
    """A CPU tensor that says it lives on the GPU: cabi's dtype and device checks run before any call."""

    def __init__(self, t, is_cuda=True):
        self.t, self.is_cuda = t, is_cuda

    def __getattr__(self, name):
        return getattr(self.t, name)

    def contiguous(self):
        return self


@pytest.fixture
def recorded(monkeypatch):
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi
    rec = _Recorder()
    monkeypatch.setattr(cabi, "lib", lambda: rec)
    monkeypatch.setattr(cabi, "_stream", lambda t, dtype=torch.float32: (cabi._dev(t, dtype), None)[1])
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    monkeypatch.setattr(torch, "empty", lambda *a, **k: _FakeCuda(torch.zeros(*a, dtype=k.get("dtype"))))
    monkeypatch.setattr(torch, "empty_like", lambda t, **k: _FakeCuda(torch.zeros(t.shape, dtype=t.dtype)))
    return cabi, rec, (lambda: [c for c in rec.calls if c != "vfi_correlation_output_dims"])


def _fake(dtype, *shape, is_cuda=True):
    return _FakeCuda(torch.zeros(*shape, dtype=dtype), is_cuda)


def _wrapper_calls(cabi, x, g, y):
    """the four pair wrappers on inputs x (four of them), gradoutputs g (two) and saved outputs y (two)"""
    return {
        "vfi_correlation_forward_pair": lambda: cabi.correlation_forward_pair(*x, 4, 1, 4, 1, 1),
        "vfi_correlation_backward_pair": lambda: cabi.correlation_backward_pair(x[0], x[1], g[0], x[2], x[3], g[1], 4, 1, 4, 1, 1),
        "vfi_correlation_lrelu_forward_pair": lambda: cabi.correlation_lrelu_forward_pair(*x, 4, 1, 4, 1, 1, 0.1),
        "vfi_correlation_lrelu_backward_pair": lambda: cabi.correlation_lrelu_backward_pair(
            x[0], x[1], y[0], g[0], x[2], x[3], y[1], g[1], 4, 1, 4, 1, 1, 0.1),
    }


def test_wrappers_dispatch_on_the_dtype_and_give_fresh_outputs_that_dtype(recorded):
    cabi, rec, launches = recorded
    for dtype, suffix in ((torch.bfloat16, "_bf16"), (torch.float32, "")):
        x = [_fake(dtype, 1, 4, 8, 10) for _ in range(4)]
        g, y = [_fake(dtype, 1, 81, 8, 10) for _ in range(2)], [_fake(dtype, 1, 81, 8, 10) for _ in range(2)]
        for name, call in _wrapper_calls(cabi, x, g, y).items():
            del rec.calls[:]
            outs = call()
            assert launches() == [name + suffix], (name, dtype)
            assert all(o.dtype == dtype for o in outs)
    # out= pairs take the inputs' dtype too
    x = [_fake(torch.bfloat16, 1, 4, 8, 10) for _ in range(4)]
    del rec.calls[:]
    out = (_fake(torch.bfloat16, 1, 81, 8, 10), None)
    got = cabi.correlation_lrelu_forward_pair(*x, 4, 1, 4, 1, 1, 0.1, out=out)
    assert got[0] is out[0] and got[1].dtype == torch.bfloat16 and launches() == ["vfi_correlation_lrelu_forward_pair_bf16"]


def test_wrappers_refuse_other_dtypes_and_mixes_before_any_library_call(recorded):
    cabi, rec, launches = recorded
    bf, f32 = torch.bfloat16, torch.float32

    def tensors(dt, where, other):
        """all tensors of dtype dt except the one at `where` (0-3 inputs, 4-5 gradoutputs, 6-7 saved outputs)"""
        t = [_fake(dt, 1, 4, 8, 10) for _ in range(4)] + [_fake(dt, 1, 81, 8, 10) for _ in range(4)]
        if where is not None:
            t[where] = _fake(other, *t[where].shape)
        return t[:4], t[4:6], t[6:8]

    uses = {"vfi_correlation_forward_pair": range(4), "vfi_correlation_backward_pair": range(6),
            "vfi_correlation_lrelu_forward_pair": range(4), "vfi_correlation_lrelu_backward_pair": range(8)}
    for first, other, message in ((bf, f32, "tensors must be bfloat16"), (bf, torch.float16, "tensors must be bfloat16"),
                                  (f32, bf, "tensors must be float32"), (f32, torch.float64, "tensors must be float32")):
        for where in range(1, 8):
            for name, call in _wrapper_calls(cabi, *tensors(first, where, other)).items():
                if where in uses[name]:
                    with pytest.raises(RuntimeError, match=message):
                        call()
    for dt in (torch.float16, torch.float64):                                   # all of one unsupported dtype: today's message
        for name, call in _wrapper_calls(cabi, *tensors(dt, None, None)).items():
            with pytest.raises(RuntimeError, match="tensors must be float32"):
                call()
    # a bfloat16 first tensor decides: the others must follow, a float32 out= too
    x = [_fake(bf, 1, 4, 8, 10) for _ in range(4)]
    with pytest.raises(RuntimeError, match="tensors must be bfloat16"):
        cabi.correlation_lrelu_forward_pair(*x, 4, 1, 4, 1, 1, 0.1, out=(None, _fake(f32, 1, 81, 8, 10)))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        cabi.correlation_forward_pair(x[0], x[1], x[2], _fake(bf, 1, 4, 8, 10, is_cuda=False), 4, 1, 4, 1, 1)
    assert launches() == []


# ------------------------------------------------------------------ 4. autograd wiring on a stubbed cabi

class _Stub:
    """The four pair wrappers on CPU tensors.  A forward returns two fresh cost volumes of the inputs' dtype; a backward
    records its call and returns a constant per gradient (1, 2, 3, 4)."""

    def __init__(self):
        self.launches = []

    def _fwd(self, name, a1, extra=None):
        self.launches.append((name, a1.dtype, extra))
        b, _, h, w = a1.shape
        return torch.full((b, 81, h, w), 1.0, dtype=a1.dtype), torch.full((b, 81, h, w), -2.0, dtype=a1.dtype)

    def _bwd(self, name, xs, gs, want, extra=None):
        self.launches.append((name, xs, gs, tuple(want), extra))
        per = (gs[0], gs[0], gs[1], gs[1])
        return tuple(torch.full_like(t, i + 1.0) if want[i] and per[i] is not None else None for i, t in enumerate(xs))

    def forward_pair(self, a1, a2, b1, b2, *cfg):
        assert cfg == (4, 1, 4, 1, 1)
        return self._fwd("forward_pair", a1)

    def backward_pair(self, a1, a2, ga, b1, b2, gb, *cfg, want=(True,) * 4):
        assert cfg == (4, 1, 4, 1, 1)
        return self._bwd("backward_pair", (a1, a2, b1, b2), (ga, gb), want)

    def lrelu_forward_pair(self, a1, a2, b1, b2, pad, k, md, s1, s2, slope, out=None):
        assert (pad, k, md, s1, s2) == (4, 1, 4, 1, 1)
        outs = self._fwd("lrelu_forward_pair", a1, out)
        return outs if out is None else tuple(o if d is None else d for o, d in zip(outs, out))

    def lrelu_backward_pair(self, a1, a2, ya, ga, b1, b2, yb, gb, pad, k, md, s1, s2, slope, want=(True,) * 4):
        assert (pad, k, md, s1, s2) == (4, 1, 4, 1, 1)
        return self._bwd("lrelu_backward_pair", (a1, a2, b1, b2), (ga, gb), want, (ya, yb, slope))

    def single(self, *a, **k):
        self.launches.append(("a single-entry wrapper",))
        raise AssertionError("a single-entry wrapper was reached")


@pytest.fixture
def stubbed(monkeypatch):
    from vfidkr_amd import cabi, fused
    stub = _Stub()
    monkeypatch.setattr(cabi, "correlation_forward_pair", stub.forward_pair)
    monkeypatch.setattr(cabi, "correlation_backward_pair", stub.backward_pair)
    monkeypatch.setattr(cabi, "correlation_lrelu_forward_pair", stub.lrelu_forward_pair)
    monkeypatch.setattr(cabi, "correlation_lrelu_backward_pair", stub.lrelu_backward_pair)
    for name in ("correlation_forward", "correlation_backward", "correlation_lrelu_forward", "correlation_lrelu_backward",
                 "pwc_warp_forward", "pwc_warp_backward"):
        monkeypatch.setattr(cabi, name, stub.single)
    return fused, stub


def _leaves(pattern):
    return [torch.rand(1, 3, 5, 6).bfloat16().requires_grad_(r) for r in pattern]


PATTERNS = [(True, True, True, True), (False, True, False, True), (True, True, False, False), (False, False, True, False)]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("lrelu", [False, True])
def test_bfloat16_leaves_go_through_and_only_the_needed_gradients_are_asked_for(stubbed, pattern, lrelu):
    fused, stub = stubbed
    xs = _leaves(pattern)
    out_a, out_b = fused.corr_pair_lrelu(*xs, negative_slope=0.2) if lrelu else fused._CorrPair.apply(*xs)
    assert out_a.dtype == torch.bfloat16 and out_b.dtype == torch.bfloat16 and out_a.grad_fn is not None and out_b.grad_fn is out_a.grad_fn
    assert [c[:2] for c in stub.launches] == [("lrelu_forward_pair" if lrelu else "forward_pair", torch.bfloat16)]
    wa, wb = torch.rand(1, 81, 5, 6).bfloat16(), torch.rand(1, 81, 5, 6).bfloat16()
    ((out_a * wa).sum() + (out_b * wb).sum()).backward()
    assert len(stub.launches) == 2
    name, saved, (ga, gb), want, extra = stub.launches[1]
    assert name == ("lrelu_backward_pair" if lrelu else "backward_pair") and want == pattern
    assert all(s.dtype == torch.bfloat16 and torch.equal(s, x) for s, x in zip(saved, xs))
    assert ga.dtype == torch.bfloat16 and torch.equal(ga, wa) and torch.equal(gb, wb)
    if lrelu:                                               # the saved tensors are the activated outputs, and the slope arrives
        assert torch.equal(extra[0], out_a) and torch.equal(extra[1], out_b) and extra[2] == pytest.approx(0.2)
    for i, x in enumerate(xs):
        if pattern[i]:
            assert x.grad.dtype == torch.bfloat16 and torch.equal(x.grad, torch.full_like(x, i + 1.0))
        else:
            assert x.grad is None


@pytest.mark.parametrize("lrelu", [False, True])
def test_an_unused_cost_volume_arrives_as_none(stubbed, lrelu):
    fused, stub = stubbed
    xs = _leaves((True,) * 4)
    outs = fused.corr_pair_lrelu(*xs) if lrelu else fused._CorrPair.apply(*xs)
    (outs[1].float() * 3.0).sum().backward()
    _, _, (ga, gb), want, _ = stub.launches[1]
    assert ga is None and gb is not None and gb.dtype == torch.bfloat16 and want == (True,) * 4
    assert xs[0].grad is None and xs[1].grad is None and torch.equal(xs[3].grad, torch.full_like(xs[3], 4.0))


def test_corr_pair_lrelu_takes_bfloat16_in_inference_with_out_pairs(stubbed, monkeypatch):
    fused, stub = stubbed

    def refuse(*a, **k):
        raise AssertionError("the autograd Function was reached")
    monkeypatch.setattr(fused._CorrPairLrelu, "apply", refuse)
    xs = _leaves((False,) * 4)
    buf = torch.zeros(1, 90, 5, 6, dtype=torch.bfloat16)
    got = fused.corr_pair_lrelu(*xs, out=(buf[:, 3:84], None))
    assert got[0].data_ptr() == buf[:, 3:84].data_ptr() and got[1].dtype == torch.bfloat16 and got[1].grad_fn is None
    assert [c[:2] for c in stub.launches] == [("lrelu_forward_pair", torch.bfloat16)] and stub.launches[0][2][1] is None
    with torch.no_grad():
        got = fused.corr_pair_lrelu(*_leaves((True,) * 4))
    assert all(o.grad_fn is None and o.dtype == torch.bfloat16 for o in got) and len(stub.launches) == 2
    with pytest.raises(RuntimeError, match="out= is for inference"):
        fused.corr_pair_lrelu(*_leaves((True,) * 4), out=(buf[:, 3:84], None))


@pytest.mark.parametrize("wants_grad", [False, True])
def test_the_float32_only_helpers_still_refuse_bfloat16_without_a_launch(stubbed, wants_grad):
    fused, stub = stubbed
    c = torch.rand(1, 3, 5, 6).bfloat16().requires_grad_(wants_grad)
    x = torch.rand(1, 3, 5, 6).bfloat16()
    flo = torch.zeros(1, 2, 5, 6)
    for call in (lambda: fused.corr_pair(c, x, x, c), lambda: fused.corr_pair(x.float(), x.float(), x.float(), c),
                 lambda: fused.corr_lrelu(c, x), lambda: fused.warp(c, flo), lambda: fused.warp(c, flo.bfloat16())):
        with pytest.raises(RuntimeError, match="must be float32"):
            call()
    assert stub.launches == []
