"""`-m gpu`: the HIP kernels against tests/golden/reference.npz -- the outputs of the reference's own kernels,
executed on the CPU (raster order), on the edge inputs of tests/reference_cases.py.  Reads tests/golden/ only.

Rules, those of test_against_golden_fixtures: forwards within 1e-5 * max(1, |ref|), gradients and projected flow
within 1e-4 (the former relative to max(1, |ref|), the latter absolute), counts exact (the signed-zero tie of
MinDepthFlowProjection: every output bit for bit); the deformable variants and the
kernel_size-3 correlation only where the recorded mask is clear (there the reference read outside its buffers:
undefined; the library clamps).

The frames are small, so they reach the small-frame kernels.  The staged (LDS) kernels that large frames take are
pinned to the oracle bit for bit by the tile-class tests (test_gpu_fi_windows.py, test_gpu_bwd_tiles.py,
test_gpu_proj_tiles.py), and tests/test_reference_exec.py / test_reference_golden.py pin the oracle to the reference:
that chain covers them, so no large frame is recorded here.
"""
import os

import numpy as np
import pytest

from tests import reference_cases as rc
from tests.test_gpu_parity import close, cpu, gpu, torch_mod, cabi  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NAMES = sorted(rc.cases())
FWD, GRAD = 1e-5, 1e-4


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return rc.load(np.load(os.path.join(golden_dir, "reference.npz")))


def near(got, ref, tol, mask=None, absolute=False):
    if mask is not None:
        got, ref = np.where(mask, 0, got), np.where(mask, 0, ref)
    assert not np.isnan(ref).any()
    return np.all(np.abs(got - ref) <= tol) if absolute else close(got, ref, tol)


def run_gpu(torch, cabi, case, ref):
    i, p, op = case.inputs, case.params, case.op
    t = {k: gpu(torch, v) for k, v in i.items()}
    z = lambda a: torch.zeros(tuple(a.shape), device="cuda:0")     # noqa: E731
    o = {}
    if op == "fi_ori":
        out, g1, g2, g3 = z(i["img"]), z(i["img"]), z(i["flow"]), z(i["filt"])
        assert cabi.filterinterp_forward_ori(t["img"], t["flow"], t["filt"], out) == 0
        assert cabi.filterinterp_backward_ori(t["img"], t["flow"], t["filt"], t["gout"], g1, g2, g3) == 0
        o = dict(out=out, gimg=g1, gflow=g2, gfilt=g3)
    elif op == "fi_defor":
        v = p["variant"]
        gout = gpu(torch, i["gout"] * ~ref["pxmask"])             # as recorded: see reference_cases.run_ref
        out, g1, g2, g3, g4 = z(i["img"]), z(i["img"]), z(i["flow"]), z(i["filt"]), z(i["off"])
        if v == 2:
            assert cabi.filterinterp_forward_defor(v, t["img"], t["flow"], t["off"], None, out) == 0
            assert cabi.filterinterp_backward_defor(v, t["img"], t["flow"], t["off"], None, gout, g1, g2, g4, None) == 0
            o = dict(out=out, gimg=g1, gflow=g2, goff=g4)
        else:
            assert cabi.filterinterp_forward_defor(v, t["img"], t["flow"], t["filt"], t["off"], out) == 0
            assert cabi.filterinterp_backward_defor(v, t["img"], t["flow"], t["filt"], t["off"], gout, g1, g2, g3, g4) == 0
            o = dict(out=out, gimg=g1, gflow=g2, gfilt=g3, goff=g4)
    elif op in ("flowproj", "depthproj", "mindepth"):
        B, _, H, W = i["flow"].shape
        second = {"flowproj": (), "depthproj": (t.get("depth"),), "mindepth": (t.get("weight"),)}[op]
        fwd = {"flowproj": cabi.flowprojection_forward, "depthproj": cabi.depthflowprojection_forward,
               "mindepth": cabi.mindepthflowprojection_forward}[op]
        for fh in (0, 1):
            count, out = torch.zeros((B, 1, H, W), device="cuda:0"), z(i["flow"])
            assert fwd(t["flow"], *second, count, out, fh) == 0
            o["out%d" % fh] = out
            if fh == 0:
                o["count"] = count
        rout = gpu(torch, ref["out0"])
        # the backward given the recorded count, and given it with zeros replaced by one (the recording shows that
        # the reference reads no empty cell: both are the same arrays there)
        for suffix, cnt in (("", ref["count"]), ("_ones", rc.ones(ref["count"]))):
            if suffix and op == "mindepth":
                continue
            rcount, g1 = gpu(torch, cnt), z(i["flow"])
            if op == "flowproj":
                assert cabi.flowprojection_backward(t["flow"], rcount, t["gout"], g1) == 0
            else:
                g2 = z(i[("depth" if op == "depthproj" else "weight")])
                bwd = cabi.depthflowprojection_backward if op == "depthproj" else cabi.mindepthflowprojection_backward
                assert bwd(t["flow"], second[0], rcount, rout, t["gout"], g1, g2) == 0
                if op == "depthproj":
                    o["gdepth" + suffix] = g2
            o["gflow" + suffix] = g1
    elif op in ("interp", "interpch"):
        out, g1, g2 = z(i["img"]), z(i["img"]), z(i["flow"])
        assert cabi.interpolation_forward(t["img"], t["flow"], out) == 0
        assert cabi.interpolation_backward(t["img"], t["flow"], t["gout"], g1, g2) == 0
        o = dict(out=out, gimg=g1, gflow=g2)
    elif op == "sepconv":
        out, g1, g2, g3 = z(ref["out"]), z(i["img"]), z(i["v"]), z(i["h"])
        assert cabi.separableconv_forward(t["img"], t["v"], t["h"], out) == 0
        assert cabi.separableconv_backward(t["img"], t["v"], t["h"], t["gout"], g1, g2, g3) == 0
        o = dict(out=out, gimg=g1, gv=g2, gh=g3)
    elif op == "sepconvflow":
        out, g2, g3 = z(ref["out"]), z(i["v"]), z(i["h"])
        assert cabi.separableconvflow_forward(t["img"], t["v"], t["h"], out) == 0
        assert cabi.separableconvflow_backward(t["img"], t["v"], t["h"], t["gflow"], g2, g3) == 0
        o = dict(out=out, gv=g2, gh=g3)
    elif op == "planted":                                  # MinDepthFlowProjection over an incoming count (the signed-zero ties)
        assert p["what"] == "mindepth_floor"
        for fh in (0, 1):
            count, out = gpu(torch, i["count0"]), z(i["flow"])
            assert cabi.mindepthflowprojection_forward(t["flow"], t["weight"], count, out, fh) == 0
            o["out%d" % fh] = out
            if fh == 0:
                o["count"] = count
    elif op == "corr":
        cfg = p["cfg"]
        o["out"] = cabi.correlation_forward(t["f1"], t["f2"], *cfg)
        if "g1" in ref:
            o["g1"], o["g2"] = cabi.correlation_backward(t["f1"], t["f2"], t["gout"], *cfg)
    torch.cuda.synchronize()
    return {k: cpu(v) for k, v in o.items()}


@pytest.mark.parametrize("name", NAMES)
def test_kernels_match_recorded_reference(name, recorded, torch_mod, cabi):
    case, ref = recorded[name]
    rc.check_masks(case, ref)
    rc.check_gaps(name, case, ref)
    got = run_gpu(torch_mod, cabi, case, ref)
    assert sorted(got) == sorted(k for k in ref if k not in rc.MASK_KEYS), name
    for key, val in got.items():
        assert val.shape == ref[key].shape, (name, key)
        mask = rc.mask_for(case, ref, key)
        if case.op == "planted":                         # bit for bit, the sign of a zero count included
            assert val.view(np.uint32).tobytes() == ref[key].view(np.uint32).tobytes(), (name, key)
        elif key == "count" and case.op in ("flowproj", "mindepth"):
            assert np.array_equal(val, ref[key]), (name, key)
        elif key in ("out0", "out1"):
            assert near(val, ref[key], GRAD, mask, absolute=True), (name, key, np.abs(val - ref[key]).max())
        elif key == "out":
            assert near(val, ref[key], FWD, mask), (name, key)
        else:                                            # gradients, and DepthFlowProjection's summed depth
            assert near(val, ref[key], GRAD, mask), (name, key)
