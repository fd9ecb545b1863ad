"""CPU tests (`-m "not gpu"`) of what the bindings refuse before any launch (tests/binding_cases.py holds the contract):

  * the table covers every public wrapper of cabi.py and classifies every parameter, so a new wrapper or parameter fails here
    until it is added;
  * every valid call of the table reaches exactly the library entries the table names, once, with the fakes' integer
    dimensions and stride structs -- a refusal therefore cannot pass because the call was malformed in some other way;
  * every generated mutation, one test per (wrapper, parameter), each failing mutation named: a shape, rank, layout or list
    mutation returns 1 (raises RuntimeError from a wrapper that returns tensors), a dtype or device mutation raises
    RuntimeError, and the library is not called;
  * the pybind shim passes every at::Tensor& of every exported function to its one checking helper before the first
    library call (pinned to the source text);
  * the C entries' own refusals, swept from cabi.SIGNATURES and the header's parameter names in a child process that sees no
    device.
"""
import contextlib
import ctypes
import inspect
import os
import re
import subprocess
import sys
import types

import pytest
import torch

from tests import binding_cases as bc
from tests.test_abi_and_host import built  # noqa: F401  (fixture)
from tests.test_fi_nhwc_host import _Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video-frame-interpolation-based-on-deformable-kernel-region_amd")
SHIM = os.path.join(PKG, "csrc", "shim", "vfi_torch_shim.cpp")


class _Library(_Recorder):
    """_Recorder whose vfi_correlation_output_dims answers (a pure host function: csrc/correlation.hip)"""

    def vfi_correlation_output_dims(self, h, w, pad, k, md, s1, s2, oc, oh, ow):
        border = (k - 1) // 2 + md
        oc._obj.value = (2 * (md // s2) + 1) ** 2
        oh._obj.value = -(-(h + 2 * pad - 2 * border) // s1)
        ow._obj.value = -(-(w + 2 * pad - 2 * border) // s1)
        return 0


@pytest.fixture
def stubbed(monkeypatch):
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi
    rec = _Library()
    monkeypatch.setattr(cabi, "lib", lambda: rec)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: types.SimpleNamespace(cuda_stream=0))
    # the wrappers that allocate their results: fakes "on" the device asked for
    zeros = torch.zeros
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **k: bc.FakeGpu(zeros(*a, **k), True, getattr(device, "index", 0) or 0))
    monkeypatch.setattr(torch, "empty_like", lambda t, **k: bc.FakeGpu(zeros(t.shape, dtype=t.dtype), t.is_cuda, t.device.index or 0))
    return cabi, rec


def _public_wrappers(cabi):
    return {n for n, f in vars(cabi).items()
            if inspect.isfunction(f) and f.__module__ == cabi.__name__ and not n.startswith("_")} - set(bc.EXCLUDED)


# ------------------------------------------------------------------ 1. completeness

def test_the_table_covers_every_public_wrapper_and_every_parameter():
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi
    assert set(bc.EXCLUDED) <= set(vars(cabi))
    assert {c.wrapper for c in bc.CASES} == _public_wrappers(cabi)
    for c in bc.CASES:
        params = list(inspect.signature(getattr(cabi, c.wrapper)).parameters)
        assert list(c.args) == params, (bc.case_id(c), params)      # every parameter: a Role, an Items or a scalar's value
        for name, spec in c.args.items():
            assert isinstance(spec, (bc.Role, bc.Items)) or not hasattr(spec, "sizes"), name
    # a parameter is of one kind in every case of its wrapper
    kinds = {}
    for c in bc.CASES:
        for name, spec in c.args.items():
            kind = "tensor" if isinstance(spec, bc.Role) else "tensor list" if isinstance(spec, bc.Items) else "scalar"
            assert kinds.setdefault((c.wrapper, name), kind) == kind, (c.wrapper, name)
    assert len(bc.all_mutations()) > 4000


def test_the_shape_is_unsymmetric():
    e = bc.ENV
    assert len({e["b"], e["c"], e["h"], e["w"], e["fc"], e["n"]}) == 6 and e["oh"] == e["h"] - e["fs"] + 1 and e["ow"] == e["w"] - e["fs"] + 1
    assert e["n"] + 2 != e["n"] * e["b"] and e["hq"] != e["wq"]


# ------------------------------------------------------------------ 2. the positive control

def _fields(s):
    return tuple(getattr(s, f) for f, _ in s._fields_)


def _want_strides(cabi, struct, t):
    s = t.stride()
    if isinstance(struct, cabi.StridesNhwc):
        return (s[0], s[2], s[3])
    return tuple(s) if isinstance(struct, cabi.Strides4) else tuple(s[:3])


@pytest.mark.parametrize("case", bc.all_cases(), ids=bc.case_id)
def test_a_valid_call_reaches_the_library_once_with_the_fakes_dimensions(stubbed, case):
    cabi, rec = stubbed
    kw = bc.valid_args(case)
    result = getattr(cabi, case.wrapper)(**kw)
    if case.returns == "status":
        assert result == 0
    calls = [c for c in rec.calls if c[0] not in bc.HOST_ONLY]
    assert [n for n, _ in calls] == [c.entry for c in case.calls]
    for (name, args), want in zip(calls, case.calls):
        argtypes = cabi.SIGNATURES.get(name) or cabi.INTERNAL_SIGNATURES[name]
        assert len(args) == len(argtypes), name
        ints = [a for a, t in zip(args, argtypes) if t is ctypes.c_int]
        assert ints == [eval(e, {}, bc.ENV) for e in want.ints.split()], (name, ints)
        structs = [a for a in args if isinstance(a, (cabi.Strides, cabi.Strides4, cabi.StridesNhwc))]
        refs = want.strides.split()
        assert len(structs) == len(refs), name
        for s, ref in zip(structs, refs):
            assert _fields(s) == _want_strides(cabi, s, bc.resolve(kw, ref)), (name, ref)


# ------------------------------------------------------------------ 3. every generated call, one test per (wrapper, parameter)

# One pytest item per (wrapper[case], parameter) runs every mutation of that parameter, one at a time, and reports each one
# that is not refused as wrapper[case]-parameter-mutation: the generated calls number in the thousands, and an item apiece
# makes the suite's report (every later pull request reads it) several times as long as all other tests' together.
_GROUPS = {}
for _c, _m in bc.all_mutations():
    _GROUPS.setdefault("%s-%s" % (bc.case_id(_c), _m.param), []).append((_c, _m))


def refusal_failure(cabi, rec, case, mutation):
    """None when the mutated call is refused as its kind demands and reaches no library entry, else what happened instead"""
    kw = bc.valid_args(case)
    mutation.apply(kw)
    del rec.calls[:]
    want = bc.expected(case, mutation.kind)
    try:
        got = "returns %r" % (getattr(cabi, case.wrapper)(**kw),)
    except RuntimeError:
        got = "raises"
    except Exception as e:      # noqa: BLE001  (an AttributeError on a None item is no refusal)
        got = "raises %r" % (e,)
    reached = [c[0] for c in rec.calls if c[0] not in bc.HOST_ONLY]
    if got != want or reached:
        return "%s: %s, wanted %s; library calls %s" % (bc.case_id(case, mutation), got, want, reached)
    return None


@pytest.mark.parametrize("group", list(_GROUPS))
def test_refused_before_any_library_call(stubbed, group):
    cabi, rec = stubbed
    failures = [f for f in (refusal_failure(cabi, rec, c, m) for c, m in _GROUPS[group]) if f]
    assert not failures, "%d of %d mutations:\n%s" % (len(failures), len(_GROUPS[group]), "\n".join(failures))


def test_every_generated_mutation_is_in_a_group_and_every_kind_occurs():
    every = bc.all_mutations()
    assert sum(len(g) for g in _GROUPS.values()) == len(every) >= 5000
    assert len({bc.case_id(c, m) for c, m in every}) == len(every)              # the ids tell wrapper, parameter and mutation apart
    assert {m.kind for _, m in every} == {"dtype", "device", "rank", "shape", "layout", "list"}
    assert {bc.expected(c, m.kind) for c, m in every} == {"raises", "returns 1"}


def test_a_missing_check_is_reported_by_name(stubbed, monkeypatch):
    """the grouped test is no weaker than one test per mutation: with one helper's check taken out, exactly the mutations
    that need it are reported, by wrapper, parameter and mutation"""
    cabi, rec = stubbed
    monkeypatch.setattr(cabi, "_fi_filter_ok", lambda input1, filt: True)
    group = _GROUPS["filterinterp_forward_ori[f32]-input3"]
    failures = [f for f in (refusal_failure(cabi, rec, c, m) for c, m in group) if f]
    assert failures and all(f.startswith("filterinterp_forward_ori[f32]-input3-") for f in failures)
    assert any("size2-1" in f and "vfi_filterinterp_forward_ori" in f for f in failures)      # the issue's [B,16,H-1,W] filter
    assert len(failures) < len(group)


# ------------------------------------------------------------------ 4. the pybind shim, pinned to its source text

def shim_exported_functions():
    """{C++ function name: (its at::Tensor& parameter names, its body)} for every m.def of the shim's modules"""
    text = re.sub(r"//[^\n]*", "", open(SHIM).read())
    exported = re.findall(r"m\.def\(\"\w+\",\s*&(\w+)", text)
    assert len(exported) == len(set(exported)) == 24, exported
    out = {}
    for fn in exported:
        m = re.search(r"\bint %s\(([^)]*)\)\s*\{" % fn, text)
        assert m, fn
        depth, i = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(text[i], 0)
            i += 1
        out[fn] = (re.findall(r"at::Tensor&\s*(\w+)", m.group(1)), text[m.end():i - 1])
    return out


def check_shim_source():
    """every exported function hands every at::Tensor& to the checking helper, as its first statement and before any vfi_ call"""
    for fn, (tensors, body) in shim_exported_functions().items():
        assert tensors, fn
        m = re.match(r"\s*check_tensors(?:_as)?\(([^;]*)\);", body)
        assert m, "%s: check_tensors(...) is not the first statement" % fn
        passed = [a.strip() for a in m.group(1).split(",")]
        passed = [a for a in passed if not a.startswith("/*")]
        assert passed[-len(tensors):] == tensors, (fn, passed, tensors)
        first_call = re.search(r"\bvfi_\w+\s*\(", body)
        assert first_call is None or first_call.start() > m.end(), fn
    text = open(SHIM).read()
    # the helper itself: defined, on the GPU, one device, the dtype
    helper = text[text.index("inline void check_tensors_as("):text.index("inline void check_tensors(")]
    for needle in ("defined()", "is_cuda()", "device() == first.device()", "scalar_type() == dt", "at::kFloat"):
        assert needle in helper, needle
    assert "check_tensors_as(false, first, rest...)" in text


def test_every_exported_shim_function_checks_every_tensor_first():
    check_shim_source()
    text = open(SHIM).read()
    assert "a call the reference would have run out of bounds" in text      # the decision, stated where the checks are
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "would have run out of bounds" in design and "tests/binding_cases.py" in design


# ------------------------------------------------------------------ 5. the C entries' own refusals, swept

OPTIONAL_POINTERS = {
    # the header documents these as optional (NULL = absent / not wanted)
    "vfi_filterinterp_forward_defor": {"input4"}, "vfi_filterinterp_backward_defor": {"input4", "gradinput4"},
    "vfi_filterinterp_blend_forward": {"out0", "out2"},
    "vfi_filterinterp_blend_backward": {"grad_blend", "grad_out0", "grad_out2", "grad_ref0", "grad_ref2", "grad_flow0", "grad_flow2",
                                        "grad_filt0", "grad_filt2"},
    "vfi_rectify_head_forward_bf16": {"blend_f32"},
    "vfi_pwc_warp_backward": {"grad_x", "grad_flow"}, "vfi_pwc_warp_backward_bf16": {"grad_x", "grad_flow"},
    "vfi_depthflowprojection_backward_up4": {"grad_depths"},
    "vfi_part_loss_forward": {"target", "flow0", "flow1", "img0", "img1"},
    "vfi_part_loss_backward": {"target", "flow0", "flow1", "img0", "img1", "sample_means", "grad_diffs", "grad_flow0", "grad_flow1"},
}
for _n in ("", "_bf16"):
    # (any gradient NULL: not computed; an item with both gradients NULL may be all NULL)
    _g = {"gradinput1_a", "gradinput2_a", "gradinput1_b", "gradinput2_b"}
    OPTIONAL_POINTERS["vfi_correlation_backward_pair" + _n] = _g
    OPTIONAL_POINTERS["vfi_correlation_lrelu_backward_pair" + _n] = _g
NOT_SWEPT = {"vfi_projection_reserve", "vfi_release_workspaces", "vfi_correlation_output_dims"}      # no tensor arguments
DIMENSIONS = {"batch", "channel", "h", "w", "hq", "wq", "nflows", "nitems", "filter_channels", "filter_size",
              "nd", "cd", "ci", "channels", "n"}


def header_parameters(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vfi_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_the_sweep_knows_every_entry():
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi
    for name, argtypes in cabi.SIGNATURES.items():
        if name in NOT_SWEPT:
            continue
        params = header_parameters(name)
        assert len(params) == len(argtypes), name
        names = {re.search(r"(\w+)$", p).group(1) for p in params}
        assert OPTIONAL_POINTERS.get(name, set()) <= names, (name, OPTIONAL_POINTERS.get(name, set()) - names)


def test_c_entries_refuse_null_pointers_and_empty_dimensions_in_a_process_without_a_device(built):  # noqa: F811
    """Every entry of cabi.SIGNATURES with dummy pointers that address nothing: each pointer NULL in turn (the optional ones
    apart), each NULL slot of a pointer table, each dimension 0 and -1 -> VFI_ERR_SHAPE.  The child sees no device and
    checks that before its first call: a missing check cannot start a kernel anywhere."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "abi_sweep_child.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert re.search(r"^swept \d+ entries, \d+ calls, 0 not refused$", out.stdout.strip().splitlines()[-1]), out.stdout[-2000:]
