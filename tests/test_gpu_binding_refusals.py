"""GPU tests (`-m gpu`) of the bindings' refusals with real tensors through the real library (tests/binding_cases.py holds the
contract; tests/test_binding_refusals_host.py runs all of it on fakes).  What fakes cannot show: torch.Size comparisons, the
strides of real views, and the pybind path.

Per family -- FilterInterpolation ori (forward and backward), deformable, blend, the three projections (and FlowProjection's
backward), Interpolation, SeparableConv, correlation, the PWC-Net warp, the frame boundary -- one shape, one layout and one
dtype mutation of the table goes through `cabi` and, where the reference has a module for it, through that module; a CPU
tensor goes into every position of the modules' functions.  Asserted: the return value or the exception; every buffer of the
call still holds its sentinel, bit for bit, margins included; and the valid call made before the refused ones gives the same
bits when it is made again after them.

Two rules make a missed check an assertion and never a fault:
  * every tensor of a refused call is a view into an allocation of its own (ALLOC elements, the view OFFSET elements in) far
    larger than anything a kernel could address from it with the valid call's sizes and strides, sentinel-filled;
  * the module's first test re-runs the source-text check of the shim and the host refusals of the device mutations; if
    either fails, every other test here is skipped: no CPU tensor is handed to a binding whose check is not known to be there.
"""
import contextlib
import importlib
import types

import pytest
import torch

from tests import binding_cases as bc
from tests.test_binding_refusals_host import _Library, check_shim_source

pytestmark = pytest.mark.gpu

ALLOC, OFFSET = 1 << 16, 1 << 14
REACH = 20000               # more than any kernel addresses from a view's first element at the valid sizes ([2, 81, 6, 10] = 9720)
SENTINEL = {"uint8": 0xA5, "int64": 0x5A5A5A5A}

# family -> (the table's case, the reference-named module and function or None, the scalars that function takes after the tensors)
FAMILIES = {
    "filterinterp_ori": ("filterinterp_forward_ori[f32]", ("filterinterpolation_cuda", "FilterInterpolationLayer_gpu_forward_ori"), ()),
    "filterinterp_ori_backward": ("filterinterp_backward_ori[f32]",
                                  ("filterinterpolation_cuda", "FilterInterpolationLayer_gpu_backward_ori"), ()),
    "deformable": ("filterinterp_forward_defor[offset]", ("filterinterpolation_cuda", "FilterInterpolationLayer_gpu_forward"), ()),
    "blend": ("filterinterp_blend_forward[f32]", None, ()),
    "flowprojection": ("flowprojection_forward[f32]", ("flowprojection_cuda", "FlowProjectionLayer_gpu_forward"), ("fillhole",)),
    "flowprojection_backward": ("flowprojection_backward[f32]", ("flowprojection_cuda", "FlowProjectionLayer_gpu_backward"), ()),
    "depthflowprojection": ("depthflowprojection_forward[f32]",
                            ("depthflowprojection_cuda", "DepthFlowProjectionLayer_gpu_forward"), ("fillhole",)),
    "mindepthflowprojection": ("mindepthflowprojection_forward[f32]",
                               ("mindepthflowprojection_cuda", "minDepthFlowProjectionLayer_gpu_forward"), ("fillhole",)),
    "interpolation": ("interpolation_forward[f32]", ("interpolation_cuda", "InterpolationLayer_gpu_forward"), ()),
    "separableconv": ("separableconv_forward[f32]", ("separableconv_cuda", "SeparableConvLayer_gpu_forward"), ()),
    "correlation": ("correlation_forward[float32]", None, ()),
    "warp": ("pwc_warp_forward[float32]", None, ()),
    "frame_boundary": ("frame_u8_to_planar[u8]", None, ()),
}
_CASES = {bc.case_id(c): c for c in bc.CASES}


class Arena:
    """bc.view for real tensors: every tensor a view into a sentinel-filled allocation of its own"""

    def __init__(self, device):
        self.device, self.buffers = device, []

    def view(self, shape, strides, dtype, is_cuda=True, index=0):
        assert index == 0
        extent = 1 + sum((n - 1) * s for n, s in zip(shape, strides) if n > 0)
        assert OFFSET + max(extent, REACH) + OFFSET <= ALLOC
        fill = SENTINEL.get(dtype, -7.25)
        buf = torch.full((ALLOC,), fill, dtype=getattr(torch, dtype), device=self.device if is_cuda else "cpu")
        self.buffers.append((buf, fill))
        return buf.as_strided(tuple(shape), tuple(strides), OFFSET)

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((buf == fill).all()) for buf, fill in self.buffers)

    def bits(self):
        torch.cuda.synchronize()
        return [buf.cpu().view(torch.uint8) for buf, _ in self.buffers]


@contextlib.contextmanager
def real_tensors(arena):
    old = bc.view
    bc.view = arena.view
    try:
        yield
    finally:
        bc.view = old


def _tensors(kw):
    return [t for v in kw.values() for t in (v if isinstance(v, list) else [v]) if isinstance(t, torch.Tensor)]


def _randomise(kw, seed):
    gen = torch.Generator().manual_seed(seed)
    for t in _tensors(kw):
        if t.dtype == torch.uint8:
            t.copy_(torch.randint(0, 256, t.shape, generator=gen, dtype=torch.uint8))
        elif t.dtype.is_floating_point:
            t.copy_(torch.randn(t.shape, generator=gen).to(t.dtype))


def _valid_run(cabi, case, device):
    """the case's valid call on seeded inputs; every buffer's bits afterwards (and the returned tensors')"""
    arena = Arena(device)
    with real_tensors(arena):
        kw = bc.valid_args(case)
    _randomise(kw, 7)
    got = getattr(cabi, case.wrapper)(**kw)
    if case.returns == "status":
        assert got == 0, bc.case_id(case)
        got = ()
    got = got if isinstance(got, tuple) else (got,)
    bits = arena.bits() + [t.cpu().contiguous().view(torch.uint8) for t in got if isinstance(t, torch.Tensor)]
    assert not arena.untouched()                # (the call wrote something)
    return bits


def _pick(case):
    """one shape, one layout and one dtype mutation of the case: a NARROWED tensor (the direction that reads past an end), a
    stride that differs where the table has one (else a w stride of 2), and a 2-byte (else an 8-byte) tensor"""
    muts = [m for m in bc.mutations(case) if "on_gpu_1" not in m.what]
    tail = [m for m in muts if m.param != next(iter(case.args))] or muts        # (not the first tensor, where there is another)
    shape = [m for m in tail if m.kind == "shape" and m.what.endswith("-1")][-1]
    # (the row stride first: the one stride of a shared layout the reference bindings never compared)
    layout = ([m for m in tail if m.what.endswith("stride2_differs")] or [m for m in tail if m.kind == "layout" and "differs" in m.what] or
              [m for m in tail if m.kind == "layout"])
    dtype = ([m for m in tail if m.what.endswith("dtype_float16")] or [m for m in tail if m.kind == "dtype"])[-1]
    return [shape] + layout[:1] + [dtype]


# ------------------------------------------------------------------ the gate

def _checks_in_place():
    """the shim's source hands every tensor to its helper first, and cabi refuses every device mutation on fakes"""
    check_shim_source()
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi
    with pytest.MonkeyPatch.context() as mp:
        rec = _Library()
        mp.setattr(cabi, "lib", lambda: rec)
        mp.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
        mp.setattr(torch.cuda, "current_stream", lambda d=None: types.SimpleNamespace(cuda_stream=0))
        zeros = torch.zeros
        mp.setattr(torch, "empty", lambda *a, device=None, **k: bc.FakeGpu(zeros(*a, **k), True, getattr(device, "index", 0) or 0))
        mp.setattr(torch, "empty_like", lambda t, **k: bc.FakeGpu(zeros(t.shape, dtype=t.dtype), t.is_cuda, t.device.index or 0))
        n = 0
        for case, m in bc.all_mutations():
            if m.kind != "device":
                continue
            kw = bc.valid_args(case)
            m.apply(kw)
            with pytest.raises(RuntimeError):
                getattr(cabi, case.wrapper)(**kw)
            assert [c for c in rec.calls if c[0] not in bc.HOST_ONLY] == [], bc.case_id(case, m)
            n += 1
        assert n > 500
    return True


_GATE = {}


@pytest.fixture
def gate():
    if "ok" not in _GATE:
        try:
            _GATE["ok"] = _checks_in_place()
        except BaseException as e:      # noqa: B036  (an assertion included)
            _GATE["ok"] = False
            _GATE["why"] = repr(e)
    if not _GATE["ok"]:
        pytest.skip("the bindings' checks are not known to be in place: %s" % _GATE.get("why"))
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi
    return cabi, torch.device("cuda", 0)


def test_the_checks_are_in_place_before_any_mismatched_tensor_reaches_a_binding():
    assert _checks_in_place()


# ------------------------------------------------------------------ through cabi

@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_cabi_refuses_and_leaves_everything_as_it_was(gate, family):
    cabi, device = gate
    case = _CASES[FAMILIES[family][0]]
    before = _valid_run(cabi, case, device)
    for m in _pick(case):
        arena = Arena(device)
        with real_tensors(arena):
            kw = bc.valid_args(case)
            m.apply(kw)
        if bc.expected(case, m.kind) == "raises":
            with pytest.raises(RuntimeError):
                getattr(cabi, case.wrapper)(**kw)
        else:
            assert getattr(cabi, case.wrapper)(**kw) == 1, bc.case_id(case, m)
        assert arena.untouched(), bc.case_id(case, m)
    after = _valid_run(cabi, case, device)
    assert len(after) == len(before) and all(torch.equal(a, b) for a, b in zip(after, before))


# ------------------------------------------------------------------ through the reference-named modules

def _module_call(family, kw):
    case_id, (module, name), scalars = FAMILIES[family]
    case = _CASES[case_id]
    fn = getattr(importlib.import_module(module), name)
    tensors = [kw[p] for p, spec in case.args.items() if isinstance(spec, bc.Role)]
    return fn(*tensors, *[int(kw[s]) for s in scalars])


_MODULE_FAMILIES = sorted(f for f, v in FAMILIES.items() if v[1] is not None)


@pytest.mark.parametrize("family", _MODULE_FAMILIES)
def test_the_reference_named_module_refuses_and_leaves_everything_as_it_was(gate, family):
    cabi, device = gate
    case = _CASES[FAMILIES[family][0]]

    def valid():
        arena = Arena(device)
        with real_tensors(arena):
            kw = bc.valid_args(case)
        _randomise(kw, 11)
        assert _module_call(family, kw) == 0
        return arena.bits()
    before = valid()
    for m in _pick(case):
        arena = Arena(device)
        with real_tensors(arena):
            kw = bc.valid_args(case)
            m.apply(kw)
        if m.kind == "dtype":
            with pytest.raises(RuntimeError):
                _module_call(family, kw)
        else:
            assert _module_call(family, kw) == 1, bc.case_id(case, m)       # the reference's silent `return 1`
        assert arena.untouched(), bc.case_id(case, m)
    # a CPU tensor in each position
    roles = [p for p, spec in case.args.items() if isinstance(spec, bc.Role)]
    for p in roles:
        arena = Arena(device)
        with real_tensors(arena):
            kw = bc.valid_args(case)
            kw[p] = bc._restride(kw[p], is_cuda=False)
        with pytest.raises(RuntimeError):
            _module_call(family, kw)
        assert arena.untouched(), (family, p)
    after = valid()
    assert len(after) == len(before) and all(torch.equal(a, b) for a, b in zip(after, before))


def test_correlation_cuda_refuses_and_leaves_everything_as_it_was(gate):
    """correlation_cuda.forward / backward resize their outputs: a mismatch raises, as every failure of that binding does"""
    cabi, device = gate
    import correlation_cuda
    b, c, h, w = (bc.ENV[k] for k in "bchw")

    def run(a, bb):
        out = a.new_empty(0)
        assert correlation_cuda.forward(a, bb, a.new_empty(0), a.new_empty(0), out, *bc.PWC, 1) == 1      # (the reference returns 1)
        torch.cuda.synchronize()
        return out
    gen = torch.Generator().manual_seed(3)
    f1, f2 = (torch.randn(b, c, h, w, generator=gen).to(device) for _ in range(2))
    before = run(f1, f2)
    assert tuple(before.shape) == (b, 81, h, w)
    arena = Arena(device)
    wide = arena.view((b, c, h, w), (c * h * w, h * w, w, 1), "float32")
    new = lambda: wide.new_empty(0)      # noqa: E731
    for bad in (arena.view((b, c, h - 1, w), (c * h * w, h * w, w, 1), "float32"),        # a row short, the valid strides
                arena.view((b, c, h, w), (c * h * w, h * w, w, 1), "float16"),
                arena.view((c, h, w), (h * w, w, 1), "float32"),
                arena.view((b, c, h, w), (c * h * w, h * w, w, 1), "float32", is_cuda=False)):
        for args in ((wide, bad), (bad, wide)):
            with pytest.raises(RuntimeError):
                correlation_cuda.forward(*args, new(), new(), new(), *bc.PWC, 1)
        g = arena.view((b, 81, h, w), (81 * h * w, h * w, w, 1), "float32")
        with pytest.raises(RuntimeError):
            correlation_cuda.backward(wide, bad, new(), new(), g, new(), new(), *bc.PWC, 1)
    # a gradOutput that is not the output's shape
    g = arena.view((b, 81, h - 1, w), (81 * h * w, h * w, w, 1), "float32")
    with pytest.raises(RuntimeError):
        correlation_cuda.backward(wide, wide, new(), new(), g, new(), new(), *bc.PWC, 1)
    assert arena.untouched()
    assert torch.equal(run(f1, f2), before)
