"""CPU checks of the training-step chain (tests/train_chain.py), which the GPU module tests/test_gpu_train_chain.py rests on:

  * R is right: central finite differences of R's total (float64, the stop-gradients lifted: `exact=True`) at 24 seeded
    elements of every leaf agree with its autograd gradient to 1e-6 of the leaf's largest gradient; in `dain` the
    stop-gradients change the gradients of the frames only;
  * O against R: the measured max |O - R| / max |R| of every gradient is inside the table train_chain.MEASURED, from which
    the GPU bounds are formed, and the table names every gradient of the step;
  * census: O's forward tensors reach a target pixel with count == 0, projected flows leaving the frame on each side, a
    FilterInterpolation pixel failing its validity test, a PWC mask zero, both LeakyReLU signs, and flow terms of the loss
    on the frame's last row and column;
  * plumbing: wiring A with every launch of the library stubbed -- for each requires-grad subset and loss subset exactly
    the expected backward calls, with the expected live items and output patterns, and None gradients where the loss
    cannot reach or nothing was asked.
"""
import numpy as np
import pytest
import torch

from tests import train_chain as tc

FD_ELEMENTS = 24
FD_STEP = 2e-5


# ------------------------------------------------------------------ R is right

def _total(T, name):
    cfg = tc.CONFIGS[name]
    n = len(cfg["times"])
    w = dict(zip(tc.loss_names(cfg), tc.OUT_W[:n] + tc.CUR_W[:n] + (tc.OFFSET_W, tc.SYM_W)))
    return sum(float(T["loss_" + k]) * w[k] for k in tc.loss_names(cfg))


@pytest.mark.parametrize("name", ["dain", "slowmo"])
def test_reference_matches_finite_differences(name):
    """Every decision of R is a constant taken from O, so R is smooth and no element has to be skipped for a decision that
    changes inside the step (asserted: skipped == 0 < one in ten).  Step 2e-5: the second-order term is below 1e-7 of the
    gradient even where a Charbonnier argument is about eps, the float64 roundoff of total / step about 1e-7."""
    aux = tc.oracle_and_reference(name)[4]
    ops = tc.ReferenceOps(torch, aux, exact=True)
    L, _, _, _ = tc.run(torch, ops, name, dtype=torch.float64)
    base = {k: v.detach() for k, v in L.items()}
    rng = np.random.default_rng(5)
    checked = skipped = 0
    for leaf in tc.LEAVES:
        if leaf not in base:
            continue
        g = L[leaf].grad
        scale = float(g.abs().max())
        assert scale > 0, leaf
        h = FD_STEP / tc.DIV_FLOW if leaf == "flo" else FD_STEP     # (div_flow multiplies the flow's step into pixels)
        for idx in rng.choice(g.numel(), FD_ELEMENTS, replace=False):
            vals = []
            for delta in (h, -h):
                x = base[leaf].clone()
                x.view(-1)[int(idx)] += delta
                with torch.no_grad():
                    vals.append(_total(tc.step(torch, ops, {**base, leaf: x}, name)[0], name))
            fd = (vals[0] - vals[1]) / (2 * h)
            err = abs(fd - float(g.view(-1)[int(idx)])) / scale
            assert err <= 1e-6, "%s[%d]: finite difference %.9g, autograd %.9g (%.2g of the leaf's scale)" % (
                leaf, idx, fd, float(g.view(-1)[int(idx)]), err)
            checked += 1
    assert checked and skipped * 10 < checked


def test_stop_gradients_touch_only_the_frames_in_dain():
    """without depth and context tensors the stop-gradients left are the copied-through pixels and the loss's images: both
    act on the frames alone"""
    _, _, _, GR, aux = tc.oracle_and_reference("dain")
    _, _, _, GX = tc.run(torch, tc.ReferenceOps(torch, aux, exact=True), "dain", dtype=torch.float64)
    for leaf in ("f1", "f2", "flo", "filt0", "filt1"):
        assert tc.rel_err(GX[leaf], GR[leaf]) <= 1e-12, leaf
    for leaf in ("ref0", "ref2"):
        assert tc.rel_err(GX[leaf], GR[leaf]) > 1e-3, leaf


# ------------------------------------------------------------------ O against R: the table

def _key(name, subset):
    return name if subset is None else "%s/%s" % (name, subset)


TABLE_CASES = [("dain", None), ("slowmo", None)] + [("slowmo", s) for s in tc.LOSS_SUBSETS]


@pytest.mark.parametrize("name,subset", TABLE_CASES)
def test_oracle_is_inside_the_measured_table(name, subset):
    TO, GO, TR, GR, _ = tc.oracle_and_reference(name, None if subset is None else tc.LOSS_SUBSETS[subset])
    table = tc.MEASURED[_key(name, subset)]
    seen = set()
    for k in GO:                                            # the most downstream first
        assert (GO[k] is None) == (GR[k] is None), k
        if GO[k] is None:
            continue
        e = tc.rel_err(GO[k], GR[k])
        assert e <= table[k], "%s: grad %s: O is %.3g from R, the table says %.3g" % (_key(name, subset), k, e, table[k])
        assert e > 0.1 * table[k] or table[k] < tc.FLOOR, "%s: grad %s: the table's %.3g is stale (measured %.3g)" % (
            _key(name, subset), k, table[k], e)
        seen.add(k)
    if subset is None:
        for k in TO:
            if k.startswith(("loss_", "out")):
                e = tc.rel_err(TO[k], TR[k])
                assert e <= table["value_" + k], (k, e)
                seen.add("value_" + k)
    assert seen == set(table)


def test_forward_of_the_reference_follows_the_oracle():
    """R's forward, with O's decisions, is O's to float32 rounding at every tensor: R states the same graph"""
    for name in ("dain", "slowmo"):
        TO, _, TR, _, _ = tc.oracle_and_reference(name)
        for k in TO:
            assert tc.rel_err(TO[k], TR[k]) <= 4e-6, (name, k)


def test_bound_has_a_floor():
    assert tc.bound("dain", "f1") == pytest.approx(4 * tc.MEASURED["dain"]["f1"])
    assert tc.FLOOR == 8 * 2.0 ** -23 and all(tc.bound(c, k) >= tc.FLOOR for c in tc.MEASURED for k in tc.MEASURED[c])


# ------------------------------------------------------------------ census

@pytest.mark.parametrize("name", ["dain", "slowmo", "slowmo_big"])
def test_census(name):
    got = tc.census(name)
    assert set(got) == {"count == 0", "leaves left", "leaves right", "leaves top", "leaves bottom", "invalid", "mask zero",
                        "lrelu positive", "lrelu negative", "loss last row", "loss last column"}
    for case, n in got.items():
        assert n >= 1, "%s: no element takes the case %r" % (name, case)


# ------------------------------------------------------------------ plumbing, launches stubbed

class _Stub:
    """Stands in for every launch of wiring A; the backward ones note what they were asked for."""

    def __init__(self):
        self.calls = []

    def log(self, name, **info):
        self.calls.append((name, info))

    @staticmethod
    def fill(value, *tensors):
        for t in tensors:
            if t is not None:
                t.fill_(value)
        return 0

    def pwc_warp_forward(self, x, flo, out, align_corners=True):
        return self.fill(0.5, out)

    def correlation_lrelu_forward(self, c1, c2, *cfg, out=None):
        return torch.full((c1.size(0), 81, c1.size(2), c1.size(3)), 0.25)

    def flowprojection_forward_up4(self, fq, count, out, div, t, fillhole):
        assert fillhole == 0 and div == tc.DIV_FLOW
        return self.fill(1.0, count) or self.fill(t, out)

    def depthflowprojection_forward_up4(self, fq, depth, count, out, div, t, fillhole):
        assert fillhole == 0 and div == tc.DIV_FLOW
        return self.fill(1.0, count) or self.fill(t, out)

    def filterinterp_blend_forward(self, ref0, ref2, f0, f2, k0, k2, blend, out0, out2, w0, w2):
        return self.fill(0.125, blend, out0, out2)

    def filterinterp_forward_ori_multi_to(self, image, flows, filt, outs):
        return self.fill(0.375, *outs)

    def part_loss_forward(self, diffs, target, f0, f1, i0, i1, eps, neg, values, means):
        return self.fill(1.0, values, means)

    def part_loss_backward(self, diffs, target, f0, f1, i0, i1, eps, neg, gv, means, mask, gds, gf0, gf1):
        self.log("part_loss", mask=mask, diffs=tuple(g is not None for g in gds), flows=(gf0 is not None, gf1 is not None))
        return self.fill(1.0, *gds, gf0, gf1)

    def filterinterp_blend_backward(self, ref0, ref2, f0, f2, k0, k2, g_blend, g_out0, g_out2, w0, w2, *outs):
        self.log("blend", w=(w0, w2), warped=g_out0 is not None, outs=tuple(o is not None for o in outs))
        return self.fill(2.0, *outs)

    def filterinterp_backward_ori_image_multi(self, flows, filt, gouts, g1):
        self.log("image", items=len(flows))
        assert len(flows) == len(gouts)
        return self.fill(3.0, g1)

    def flowprojection_backward_up4(self, fq, counts, gs, mul0, mul1, gq, depths=None, outputs=None, grad_depths=None):
        self.log("up4", times=tuple(mul1), depth=depths is not None, grad_depths=grad_depths is not None)
        assert len(counts) == len(gs) == len(mul1) and (outputs is None or len(outputs) == len(gs))
        return self.fill(4.0, gq, *(grad_depths or []))

    def correlation_lrelu_backward(self, c1, c2, y, g, *cfg):
        self.log("corr")
        return torch.full_like(c1, 5.0), torch.full_like(c2, 5.0)

    def pwc_warp_backward(self, x, flo, g, gx=None, gf=None, align_corners=True):
        self.log("warp", outs=(gx is not None, gf is not None))
        return self.fill(6.0, gx, gf)


STUBBED = ("pwc_warp_forward", "correlation_lrelu_forward", "flowprojection_forward_up4", "depthflowprojection_forward_up4",
           "filterinterp_blend_forward", "filterinterp_forward_ori_multi_to", "part_loss_forward", "part_loss_backward",
           "filterinterp_blend_backward", "filterinterp_backward_ori_image_multi", "flowprojection_backward_up4",
           "correlation_lrelu_backward", "pwc_warp_backward")


@pytest.fixture
def stubbed(monkeypatch):
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi, fused
    stub = _Stub()
    for name in STUBBED:
        assert callable(getattr(cabi, name))
        monkeypatch.setattr(cabi, name, getattr(stub, name))
    return fused, stub


def expected(requires, losses, name="slowmo"):
    """(the backward calls, the leaves with a gradient) of wiring A, from the step's definition alone.  requires: the
    leaves that require grad; losses: the names in total."""
    cfg = tc.CONFIGS[name]
    times = cfg["times"]
    n, mid = len(times), len(times) // 2
    R = set(requires)
    flow_stage = bool(R & {"f1", "f2", "flo"})
    proj_req = [flow_stage or "depth%d" % d in R for d in (0, 1)]
    synth_req = bool(R & {"ref0", "ref2", "filt0", "filt1", "ctx0", "ctx2"}) or any(proj_req)
    names = tc.loss_names(cfg)
    # (the losses are elements of one tensor, which requires grad as soon as one diff or flow does: a projected flow that
    # requires grad makes the buffers require it, so that is `synth_req`)
    chosen = [k for k in names if k in losses and synth_req]
    calls = []
    if not chosen:
        return calls, set()
    mask = sum(1 << names.index(k) for k in chosen)
    flows_used = bool({"offset", "sym"} & set(chosen))
    asked = dict(mask=mask, diffs=tuple(k in chosen for k in names[:-2]), flows=tuple(flows_used and p for p in proj_req))
    if any(asked["diffs"]) or any(asked["flows"]):
        calls.append(("part_loss", asked))
    kernel_needs = ("ref0" in R, "ref2" in R, proj_req[0], proj_req[1], "filt0" in R, "filt1" in R)
    proj_grad = [set(), set()]                              # per direction the time offsets whose projected flow gets a gradient
    for t in range(n):
        g_buf, g_cur = "out%d" % t in chosen, "out%d" % t in chosen or "cur%d" % t in chosen
        if (g_buf or g_cur) and any(kernel_needs):
            calls.append(("blend", dict(w=(1.0 - times[t], times[t]), warped=g_buf, outs=kernel_needs)))
            for d in (0, 1):
                if proj_req[d]:
                    proj_grad[d].add(t)
    live = [t for t in range(n) if "out%d" % t in chosen]
    for d, c in enumerate(("ctx0", "ctx2")):
        if c in R and live:
            calls.append(("image", dict(items=len(live))))
    reached = set()
    for d in (0, 1):
        if flows_used and proj_req[d]:
            proj_grad[d].add(mid)
        if proj_grad[d]:
            depth = "depth%d" % d in R
            calls.append(("up4", dict(times=tuple(float(times[t]) for t in sorted(proj_grad[d])), depth=cfg["depth"],
                                      grad_depths=depth)))
            if depth:
                reached.add("depth%d" % d)
            if flow_stage:
                calls.append(("corr", {}))
                # direction d warps the other frame's features: its gradient, and the flow's
                outs = (("f1", "f2")[1 - d] in R, "flo" in R)
                if any(outs):
                    calls.append(("warp", dict(outs=outs)))
                reached |= R & {"f1", "f2", "flo"}
    if any(c[0] == "blend" for c in calls):
        reached |= R & {"ref0", "ref2", "filt0", "filt1"}
    if live:
        reached |= R & {"ctx0", "ctx2"}
    return calls, reached


ALL_LOSSES = tuple(tc.loss_names(tc.CONFIGS["slowmo"]))
PLUMBING = [(tc.GROUPS[g], ALL_LOSSES) for g in ("all", "flows", "filters", "contexts", "depths", "frames", "all but contexts")]
PLUMBING += [(("depth1",), ALL_LOSSES), (("flo",), ALL_LOSSES), (("f2", "ctx2"), ALL_LOSSES)]
PLUMBING += [(tc.GROUPS["all"], s) for s in tc.LOSS_SUBSETS.values()]
PLUMBING += [(("depth1",), tc.LOSS_SUBSETS["one pixel"]), (tc.GROUPS["contexts"], tc.LOSS_SUBSETS["cur only"])]


@pytest.mark.parametrize("requires,losses", PLUMBING, ids=lambda v: "+".join(v) if len(v) < 5 else "%d names" % len(v))
def test_plumbing_with_the_launches_stubbed(stubbed, requires, losses):
    fused, stub = stubbed
    ops = tc.FusedOps(torch, fused, "A")
    L, T, total, G = tc.run(torch, ops, "slowmo", requires=requires, loss_terms=losses)
    want_calls, reached = expected(requires, losses)
    key = lambda c: (c[0], sorted(c[1].items()))      # noqa: E731
    assert sorted(map(key, stub.calls)) == sorted(map(key, want_calls))
    assert (total is None) == (not want_calls)
    for leaf in tc.LEAVES:
        assert (L[leaf].grad is not None) == (leaf in reached), leaf
    # the same graph once more: part_loss's `used` set starts empty again
    stub.calls.clear()
    for v in L.values():
        v.grad = None
    T2, total2 = tc.step(torch, ops, L, "slowmo", losses)
    if total2 is not None:
        total2.backward()
    assert sorted(map(key, stub.calls)) == sorted(map(key, want_calls))


def test_two_backward_passes_ask_for_what_each_uses(stubbed):
    """part_loss's host-side `used` set across two backward passes through ONE graph: the first uses one pixel loss, the
    second the flow terms; each launch gets its own mask"""
    fused, stub = stubbed
    ops = tc.FusedOps(torch, fused, "A")
    L = tc.leaves(torch, "slowmo")
    T, _ = tc.step(torch, ops, L, "slowmo")
    T["loss_out1"].backward(retain_graph=True)
    first = [c for c in stub.calls if c[0] == "part_loss"]
    stub.calls.clear()
    (T["loss_offset"] + T["loss_sym"]).backward()
    second = [c for c in stub.calls if c[0] == "part_loss"]
    names = tc.loss_names(tc.CONFIGS["slowmo"])
    assert [c[1]["mask"] for c in first] == [1 << names.index("out1")]
    assert [c[1]["mask"] for c in second] == [(1 << names.index("offset")) | (1 << names.index("sym"))]
    assert first[0][1]["flows"] == (False, False) and second[0][1]["flows"] == (True, True)
    assert not any(c[0] in ("blend", "image") for c in stub.calls)


def test_filter_interpolate_with_every_output_unused_launches_nothing(stubbed):
    """Wiring B below a part_loss that used only its flow terms: autograd still runs the FilterInterpolate node, with three
    absent gradients.  It must launch nothing and hand back None, not a tensor of zeros (found by the chain: the flows'
    gradient came back as zeros where the fused entry and the oracle have none)."""
    fused, stub = stubbed

    class Unused(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            return None

    t = {k: torch.rand(1, c, 4, 6, requires_grad=True) for k, c in (("ref0", 3), ("ref2", 3), ("f0", 2), ("f2", 2), ("k0", 16), ("k2", 16))}
    blend, out0, out2 = fused.FilterInterpolate(t["ref0"], t["ref2"], [t["f0"], t["f2"]], [t["k0"], t["k2"]], 16, 0.25)
    (Unused.apply(blend).sum() + (t["f0"] * 2.0).sum()).backward()
    assert not stub.calls
    assert torch.equal(t["f0"].grad, torch.full_like(t["f0"], 2.0))
    assert all(t[k].grad is None for k in ("ref0", "ref2", "f2", "k0", "k2"))
    # one used output: the call is made
    blend, out0, out2 = fused.FilterInterpolate(t["ref0"], t["ref2"], [t["f0"], t["f2"]], [t["k0"], t["k2"]], 16, 0.25)
    (Unused.apply(blend).sum() + out2.sum()).backward()
    assert [c[0] for c in stub.calls] == ["blend"] and t["k2"].grad is not None


@pytest.mark.parametrize("losses", [ALL_LOSSES, tc.LOSS_SUBSETS["one pixel"]])
def test_checkpointed_step_makes_the_same_calls(stubbed, monkeypatch, losses):
    """torch.utils.checkpoint(use_reentrant=False) around projection and synthesis refuses a backward that unpacks its saved
    tensors twice (found by the chain in _rectify_backward and _FilterInterpolateCtx.backward): the checkpointed step runs,
    makes the plain step's backward calls and fills the same gradients"""
    fused, stub = stubbed
    ops = tc.FusedOps(torch, fused, "A")
    L, T, total, G = tc.run(torch, ops, "slowmo", loss_terms=losses, checkpoint=True)
    want_calls, reached = expected(tc.LEAVES, losses)
    key = lambda c: (c[0], sorted(c[1].items()))      # noqa: E731
    assert sorted(map(key, stub.calls)) == sorted(map(key, want_calls))
    assert {k for k in tc.LEAVES if L[k].grad is not None} == reached
    # the image-only Function of the unfused wiring, under a checkpoint of its own
    from torch.utils.checkpoint import checkpoint
    monkeypatch.setattr(cabi_of(fused), "filterinterp_forward_ori_multi", lambda image, offs, k, outs: stub.fill(0.5, *outs))
    c0 = torch.rand(1, 5, 4, 6, requires_grad=True)
    flows, filt = [torch.rand(1, 2, 4, 6) for _ in range(2)], torch.rand(1, 16, 4, 6)
    outs = checkpoint(lambda c: tuple(fused._FilterInterpolateCtx.apply(c, filt, *flows)), c0, use_reentrant=False)
    (outs[0].sum() + outs[1].sum()).backward()
    assert torch.equal(c0.grad, torch.full_like(c0, 3.0))


def cabi_of(fused):
    return fused.cabi
