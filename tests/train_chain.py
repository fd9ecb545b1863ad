"""One miniature DAIN / DAIN_slowmotion training step made only of the library's own trainable entries, in four wirings.
Helper module of tests/test_train_chain_host.py and tests/test_gpu_train_chain.py: no tests of its own.

The step (`step`).  The leaves are what the networks would output; there is no convolution anywhere.

  1. flow stage (one PWC level)   cost_a = lrelu(corr(f1, warp(f2, flo))), cost_b = lrelu(corr(f2, warp(f1, -flo)));
                                  flow_q_d = flo_d + mix(cost_d), mix a fixed 81 -> 2 map written as a left-to-right loop
                                  of elementwise multiply and add, so that CPU and GPU perform the same IEEE operations
  2. projection                   proj_d[t] = FlowProject(div_flow * t * upsample4(flow_q_d), depth_d), fillhole = 0
  3. synthesis                    (buf_t, cur_t) = rectify_inputs(ref0, ref2, proj, filters, 16, times, ctx0, ctx2)
  4. rectify stand-in             out_t = cur_t + (buf_t * wvec[None, :, None, None]).sum(1, keepdim=True)
  5. loss                         part_loss([out_t ..., cur_t ...], [[proj_0[mid], proj_1[mid]]], None, [ref0, ref2], eps,
                                  target=gt); total = a fixed weighted sum of the returned losses

Every stage comes from an `ops` object, the glue between the stages is the same plain torch for all wirings:

  A  FusedOps("A")       the fused entries: warp_corr_lrelu, FlowProject_from_quarter, rectify_inputs, part_loss
     FusedOps("A_pair")  as A with the pre-warped pair sent through corr_pair_lrelu
  B  FusedOps("B")       the compositions A is documented to equal: warp + corr_lrelu, forward_flownets_upsample +
                         FlowProject, tests.rectify_input.composition, the same part_loss
  O  OracleOps()         CPU, float32: one torch.autograd.Function per item, as the reference's layers are called; forward
                         and backward from oracle.cpu_oracle and the suite's restatements (tests/proj_tiles.py for the
                         fixed-point projection forward, tests/proj_up4_backward.py, tests/pwc_warp_backward.py,
                         tests/corr_lrelu.py), the loss from tests.part_loss.torch_losses under CPU autograd
  R  ReferenceOps(aux)   CPU, float64, plain torch (gather, index_add, elementwise) under torch autograd, no hand-written
                         backward.  Every discrete decision -- floor cell, validity test, border clamp, count > 0, the
                         PWC mask and the LeakyReLU sign -- is computed from O's float32 tensors at the same point (`aux`)
                         and enters as a constant, so R follows O's branch everywhere.

The reference's backward differs from the derivative of its forward in three places, and the library reproduces the
reference; a fourth stop-gradient is the step's own (the frames enter the loss as data).  R states each with `.detach()`;
ReferenceOps(aux, exact=True) is the same graph without them, which is what finite differences can check:
  * DepthFlowProjection gives the depth -g / count * (f - out) per target cell, where the quotient rule gives
    -g / count * (f + out) (out = -sum(d f) / sum(d)): R writes out = (num + (count - count.detach()) * out.detach()) /
    count.detach(), whose value is num / count and whose depth derivative is the reference's;
  * FilterInterpolation copies the image through where the validity test fails and gives that pixel no gradient;
  * FilterInterpolate_ctx passes flows and filters detached.
"""
import functools

import numpy as np

from tests import corr_edges as ce
from tests import corr_lrelu as cl
from tests import part_loss as pl
from tests import proj_tiles as pt
from tests import proj_up4_backward as pu
from tests import pwc_warp_backward as pwb
from tests import rectify_input as ri

f32 = np.float32
DIV_FLOW = 20.0
EPS = 1e-3
SLOPE = 0.1
FS2 = 16
FEATURES = 12

# quarter 9 x 20 -> 36 x 80: one full and one partial 64-wide tile per row, 36 = 4 x 8 + 4 = 9 x 4 rows; the quarter map has
# one partial 64 x 4 correlation tile per row and three tile rows.  The second size serves the workspace test only.
CONFIGS = {
    "dain": dict(B=2, hq=9, wq=20, times=(0.5,), depth=False, cctx=0, bf16=False, seed=1),
    "slowmo": dict(B=2, hq=9, wq=20, times=(0.25, 0.5, 0.75), depth=True, cctx=5, bf16=False, seed=2),
    "slowmo_bf16": dict(B=2, hq=9, wq=20, times=(0.25, 0.5, 0.75), depth=True, cctx=5, bf16=True, seed=2),
    "slowmo_big": dict(B=1, hq=17, wq=35, times=(0.25, 0.5, 0.75), depth=True, cctx=5, bf16=False, seed=3),
}

LEAVES = ("f1", "f2", "flo", "depth0", "depth1", "ref0", "ref2", "filt0", "filt1", "ctx0", "ctx2")
GROUPS = {
    "flows": ("f1", "f2", "flo"),
    "filters": ("filt0", "filt1"),
    "contexts": ("ctx0", "ctx2"),
    "depths": ("depth0", "depth1"),
    "frames": ("ref0", "ref2"),
}
GROUPS["all"] = LEAVES
GROUPS["all but contexts"] = tuple(n for n in LEAVES if n not in GROUPS["contexts"])

MIX = np.random.default_rng(7).normal(0.0, 0.02, (2, 81)).astype(f32)          # the fixed 81 -> 2 channel map
OUT_W, CUR_W = (1.0, 0.75, 0.5), (0.5, 0.25, 0.125)                             # loss weights: dyadic, so w * loss is exact
OFFSET_W, SYM_W = 0.25, 0.5


# totals made of part of the losses (slowmo): the other outputs are absent items all the way up
LOSS_SUBSETS = {"one pixel": ("out1",), "flow terms": ("offset", "sym"), "cur only": ("cur0", "cur1", "cur2")}


def wvec(channels):
    """the stand-in's fixed channel weights"""
    return np.random.default_rng(8).normal(0.0, 0.1, channels).astype(f32)


_WVEC = {}


def _wvec_on(torch, channels, device):
    """wvec on a device, copied there once (a captured step must not copy from the host)"""
    key = (channels, str(device))
    if key not in _WVEC:
        _WVEC[key] = torch.from_numpy(wvec(channels)).to(device)
    return _WVEC[key]


def frame(cfg):
    return 4 * cfg["hq"], 4 * cfg["wq"]


def loss_names(cfg):
    n = len(cfg["times"])
    return ["out%d" % t for t in range(n)] + ["cur%d" % t for t in range(n)] + ["offset", "sym"]


def pixel_names(cfg):
    return loss_names(cfg)[:-2]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """name -> {leaf or "gt": float32 numpy array}, read-only.  Flows of a few pixels, some leaving the frame."""
    import torch
    cfg = CONFIGS[name]
    B, hq, wq = cfg["B"], cfg["hq"], cfg["wq"]
    H, W = frame(cfg)
    rng = np.random.default_rng([2024, cfg["seed"]])
    a = {"f1": rng.standard_normal((B, FEATURES, hq, wq)).astype(f32),
         "f2": rng.standard_normal((B, FEATURES, hq, wq)).astype(f32),
         # quarter-resolution flow in units of div_flow: sigma 0.3 is 20 t 0.3 = 1.5 .. 4.5 pixels at full resolution
         "flo": (pwb.flow_family(rng, "3", B, hq, wq) * f32(0.1)).astype(f32)}
    ref0, ref2, _, filt, c0, c2 = ri.smooth_inputs(torch, rng, B, H, W, 1, cfg["cctx"] or None, device="cpu")
    a.update(ref0=ref0.numpy(), ref2=ref2.numpy(), filt0=filt[0].numpy(), filt1=filt[1].numpy())
    if cfg["cctx"]:
        a.update(ctx0=c0.numpy(), ctx2=c2.numpy())
    if cfg["depth"]:
        a.update(depth0=rng.uniform(0.1, 1.0, (B, 1, H, W)).astype(f32), depth1=rng.uniform(0.1, 1.0, (B, 1, H, W)).astype(f32))
    a["gt"] = rng.random((B, 3, H, W)).astype(f32)
    if cfg["bf16"]:                                        # the values a bfloat16 network would hand over
        for k in ("f1", "f2", "ctx0", "ctx2"):
            a[k] = torch.from_numpy(a[k]).to(torch.bfloat16).float().numpy()
    for v in a.values():
        v.setflags(write=False)
    return a


BF16_LEAVES = ("f1", "f2", "ctx0", "ctx2")


def leaves(torch, name, device="cpu", dtype=None, requires="all"):
    """fresh leaf tensors of a configuration (and "gt", never requiring grad); requires: a key of GROUPS or a tuple of names"""
    cfg = CONFIGS[name]
    want = GROUPS[requires] if isinstance(requires, str) else tuple(requires)
    out = {}
    for k, v in inputs(name).items():
        t = torch.from_numpy(np.array(v)).to(device)
        if dtype is not None:
            t = t.to(dtype)
        elif cfg["bf16"] and k in BF16_LEAVES:
            t = t.to(torch.bfloat16)
        out[k] = t.requires_grad_(k in want)
    return out


# ------------------------------------------------------------------ the step

def mix(torch, cost, d):
    """the fixed 81 -> 2 map of direction d: per output channel ((c_0 w_0 + c_1 w_1) + c_2 w_2) + ..., one torch op each"""
    planes = []
    for k in range(2):
        w = [float(MIX[(k + d) % 2, c]) for c in range(81)]
        acc = cost[:, 0:1] * w[0]
        for c in range(1, 81):
            acc = acc + cost[:, c:c + 1] * w[c]
        planes.append(acc)
    return torch.cat(planes, dim=1)


def stage23(torch, ops, cfg, fq0, fq1, dep0, dep1, ref0, ref2, k0, k2, c0, c2):
    """projection and synthesis as one function of tensors (what the checkpoint test wraps): a flat tuple of
    2T upsampled flows (or none), 2T projected flows, their 2T taps into the synthesis, T buffers, T cur_outputs"""
    times = cfg["times"]
    ups, proj, taps = [], [], []
    for d, (fq, dep) in enumerate(((fq0, dep0), (fq1, dep1))):
        up, pr = ops.project(fq, dep, times, d)
        ups += list(up or [])
        proj.append(list(pr))
        # the synthesis reads a copy: its gradient is the synthesis stage's alone, before the loss's term joins
        taps.append([p.clone() for p in pr])
    pairs = ops.synth(ref0, ref2, taps, [k0, k2], times, c0, c2)
    return (*ups, *proj[0], *proj[1], *taps[0], *taps[1], *[b for b, _ in pairs], *[c for _, c in pairs])


def step(torch, ops, L, name, loss_terms=None, checkpoint=False):
    """Runs the step on the leaves L.  Returns (tensors, total): `tensors` maps names to the intermediates in graph order
    (upstream first; every one that requires grad retains it), the loss values included; total is None when no chosen
    loss requires grad (or none is chosen).  loss_terms: the names of `loss_names` that enter total, None = all."""
    cfg = CONFIGS[name]
    n = len(cfg["times"])
    T = {}
    flos = (L["flo"], -L["flo"])
    costs = ops.costs(L["f1"], L["f2"], flos)
    fq = []
    for d in (0, 1):
        T["cost%d" % d] = costs[d]
        cost = costs[d].float() if costs[d].dtype == torch.bfloat16 else costs[d]
        fq.append(flos[d] + mix(torch, cost, d))
        T["flow_q%d" % d] = fq[d]
    args = (fq[0], fq[1], L.get("depth0"), L.get("depth1"), L["ref0"], L["ref2"], L["filt0"], L["filt1"], L.get("ctx0"), L.get("ctx2"))
    if checkpoint:
        from torch.utils.checkpoint import checkpoint as ckpt
        flat = ckpt(lambda *a: stage23(torch, ops, cfg, *a), *args, use_reentrant=False)
    else:
        flat = stage23(torch, ops, cfg, *args)
    flat = list(flat)
    if len(flat) == 8 * n:
        for d in (0, 1):
            for t in range(n):
                T["up%d_%d" % (d, t)] = flat.pop(0)
    for kind in ("proj", "tap"):
        for d in (0, 1):
            for t in range(n):
                T["%s%d_%d" % (kind, d, t)] = flat.pop(0)
    for kind in ("buf", "cur"):
        for t in range(n):
            T["%s%d" % (kind, t)] = flat.pop(0)
    assert not flat
    wv = _wvec_on(torch, T["buf0"].shape[1], T["buf0"].device)
    for t in range(n):
        buf = T["buf%d" % t]
        T["out%d" % t] = T["cur%d" % t] + (buf * wv.to(buf.dtype)[None, :, None, None]).sum(1, keepdim=True)
    mid = n // 2
    diffs = [T["out%d" % t] for t in range(n)] + [T["cur%d" % t] for t in range(n)]
    # (the frames enter the loss as data, as in the reference's train.py; ReferenceOps(exact=True) lets them through)
    images = (L["ref0"], L["ref2"]) if getattr(ops, "exact", False) else (L["ref0"].detach(), L["ref2"].detach())
    pixel, offset, sym = ops.loss(diffs, (T["proj0_%d" % mid], T["proj1_%d" % mid]), images, L["gt"])
    values = dict(zip(loss_names(cfg), list(pixel) + [offset, sym]))
    weights = dict(zip(loss_names(cfg), OUT_W[:n] + CUR_W[:n] + (OFFSET_W, SYM_W)))
    total = None
    for k in loss_names(cfg):
        T["loss_" + k] = values[k]
        if (loss_terms is None or k in loss_terms) and values[k].requires_grad:
            term = values[k] * weights[k]
            total = term if total is None else total + term
    for v in T.values():
        if v.requires_grad and not v.is_leaf:
            v.retain_grad()
    return T, total


def gradients(T, L):
    """name -> gradient or None, the most downstream tensor first and the leaves last"""
    out = {}
    for k in reversed(list(T)):
        if not k.startswith("loss_"):
            out[k] = T[k].grad if T[k].requires_grad else None
    for k in LEAVES:
        if k in L:
            out[k] = L[k].grad
    return out


# ------------------------------------------------------------------ A and B: the library on the GPU

class FusedOps:
    def __init__(self, torch, fused, wiring, bf16=False):
        assert wiring in ("A", "A_pair", "B")
        self.torch, self.fused, self.wiring, self.bf16 = torch, fused, wiring, bf16

    def costs(self, f1, f2, flos):
        fused, torch = self.fused, self.torch
        if self.wiring == "A":
            return fused.warp_corr_lrelu(f1, f2, flos[0]), fused.warp_corr_lrelu(f2, f1, flos[1])
        if self.wiring == "A_pair":
            return fused.corr_pair_lrelu(f1, fused.warp(f2, flos[0]), f2, fused.warp(f1, flos[1]))
        if self.bf16:
            # the documented composition of the bfloat16 warp: the float32 warp of the widened features, rounded once
            warp = lambda x, flo: fused.warp(x.float(), flo).to(torch.bfloat16)      # noqa: E731
            return (fused._CorrLrelu.apply(f1, warp(f2, flos[0]), SLOPE), fused._CorrLrelu.apply(f2, warp(f1, flos[1]), SLOPE))
        return fused.corr_lrelu(f1, fused.warp(f2, flos[0])), fused.corr_lrelu(f2, fused.warp(f1, flos[1]))

    def project(self, fq, depth, times, d):
        fused = self.fused
        if self.wiring != "B":
            return None, fused.FlowProject_from_quarter(fq, DIV_FLOW, list(times), depth, fillhole=0)
        ups = fused.forward_flownets_upsample(fq, DIV_FLOW, list(times))
        return ups, fused.FlowProject(ups, depth, fillhole=0)

    def synth(self, ref0, ref2, offs, filts, times, c0, c2):
        fused, torch = self.fused, self.torch
        if self.wiring != "B":
            return fused.rectify_inputs(ref0, ref2, offs, filts, FS2, list(times), c0, c2, dtype=torch.bfloat16 if self.bf16 else None)
        if self.bf16:
            # the float32 call (the contexts entering through .float()) .to(bfloat16); cur_output is the float32 call's
            wide = (None, None) if c0 is None else (c0.float(), c2.float())
            return [(buf.to(torch.bfloat16), cur) for buf, cur in ri.composition(torch, fused, ref0, ref2, offs, filts, FS2, list(times), *wide)]
        return ri.composition(torch, fused, ref0, ref2, offs, filts, FS2, list(times), c0, c2)

    def loss(self, diffs, flows, images, gt):
        pixel, offset, sym = self.fused.part_loss(diffs, [[flows[0], flows[1]]], None, list(images), EPS, target=gt)
        return pixel, offset[0], sym[0]


# ------------------------------------------------------------------ O: the oracle on the CPU, float32

def _np(t):
    return np.ascontiguousarray(t.detach().numpy(), dtype=f32)


def _oracle():
    from oracle import cpu_oracle
    cpu_oracle.build()
    return cpu_oracle


def _oracle_functions(torch):
    """the reference's layers as autograd Functions over the CPU oracle, one item each"""
    oracle = _oracle()
    th = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=f32))      # noqa: E731

    class Warp(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, flo):
            ctx.save_for_backward(x, flo)
            return th(oracle.pwc_warp(_np(x), _np(flo), True, fmad=1))

        @staticmethod
        def backward(ctx, g):
            x, flo = ctx.saved_tensors
            gx, gf = pwb.pwc_warp_bwd(_np(x), _np(flo), _np(g), True)[:2]
            return th(gx), th(gf)

    class CorrLrelu(torch.autograd.Function):
        @staticmethod
        def forward(ctx, c1, c2):
            y = th(cl.expected_forward(_np(c1), _np(c2), ce.PWC, SLOPE))
            ctx.save_for_backward(c1, c2, y)
            return y

        @staticmethod
        def backward(ctx, g):
            c1, c2, y = ctx.saved_tensors
            g1, g2 = cl.expected_backward(_np(c1), _np(c2), _np(y), _np(g), ce.PWC, SLOPE)
            return th(g1), th(g2)

    class Upsample(torch.autograd.Function):
        @staticmethod
        def forward(ctx, fq, t):
            ctx.t = t
            return th(oracle.flow_upsample4(_np(fq), DIV_FLOW, t, fmad=1))

        @staticmethod
        def backward(ctx, g):
            return th(pu.up4_backward([_np(g)], DIV_FLOW, [ctx.t])[0]), None

    class Project(torch.autograd.Function):
        """FlowProjectionModule / DepthFlowProjectionModule, fillhole = 0: the forward is the library's fixed-point sum
        (tests/proj_tiles.py), the backward the reference's"""
        @staticmethod
        def forward(ctx, flow, depth, box):
            if depth is None:
                out, count = pt.predict_flowprojection(_np(flow))
            else:
                out, count = pt.predict_depthflowprojection(_np(flow), _np(depth))
            out, count = th(out), th(count)
            box["count"] = count
            ctx.has_depth = depth is not None
            ctx.save_for_backward(flow, count, out, *([depth] if depth is not None else []))
            return out

        @staticmethod
        def backward(ctx, g):
            flow, count, out = ctx.saved_tensors[:3]
            if not ctx.has_depth:
                return th(oracle.flowproj_bwd(_np(flow), _np(count), _np(g))), None, None
            gf, gd = oracle.depthflowproj_bwd(_np(flow), _np(ctx.saved_tensors[3]), _np(count), _np(out), _np(g))
            return th(gf), th(gd), None

    class FilterInterp(torch.autograd.Function):
        @staticmethod
        def forward(ctx, img, flow, filt):
            ctx.save_for_backward(img, flow, filt)
            return th(oracle.filterinterp_ori_fwd(_np(img), _np(flow), _np(filt), fmad=1))

        @staticmethod
        def backward(ctx, g):
            img, flow, filt = ctx.saved_tensors
            return tuple(th(a) for a in oracle.filterinterp_ori_bwd(_np(img), _np(flow), _np(filt), _np(g), fmad=1))

    return Warp, CorrLrelu, Upsample, Project, FilterInterp


class OracleOps:
    """`aux` collects, as numpy float32 / bool arrays, what R takes its decisions from"""

    def __init__(self, torch):
        self.torch = torch
        self.Warp, self.CorrLrelu, self.Upsample, self.Project, self.FilterInterp = _oracle_functions(torch)
        self.aux = {}

    def costs(self, f1, f2, flos):
        out = []
        for d, (a, b) in enumerate(((f1, f2), (f2, f1))):
            y = self.CorrLrelu.apply(a, self.Warp.apply(b, flos[d]))
            self.aux["flo%d" % d], self.aux["positive%d" % d] = _np(flos[d]), _np(y) > 0
            out.append(y)
        return out

    def project(self, fq, depth, times, d):
        ups, proj = [], []
        for i, t in enumerate(times):
            up = self.Upsample.apply(fq, float(t))
            box = {}
            proj.append(self.Project.apply(up, depth, box))
            self.aux["up%d_%d" % (d, i)], self.aux["count%d_%d" % (d, i)] = _np(up), _np(box["count"])
            ups.append(up)
        return ups, proj

    def synth(self, ref0, ref2, offs, filts, times, c0, c2):
        torch, FI = self.torch, self.FilterInterp
        out = []
        for i, t in enumerate(times):
            p0, p2 = offs[0][i], offs[1][i]
            self.aux["tap0_%d" % i], self.aux["tap1_%d" % i] = _np(p0), _np(p2)
            o0, o2 = FI.apply(ref0, p0, filts[0]), FI.apply(ref2, p2, filts[1])
            cur = o0 * float(1.0 - t) + o2 * float(t)
            parts = [cur, o0, o2, p0, p2, filts[0], filts[1]]
            if c0 is not None:                             # (the reference detaches flow and filter on the context path)
                parts += [FI.apply(c0, p0.detach(), filts[0].detach()), FI.apply(c2, p2.detach(), filts[1].detach())]
            out.append((torch.cat(parts, dim=1), cur))
        return out

    def loss(self, diffs, flows, images, gt):
        return pl.torch_losses(list(diffs), gt, list(flows), list(images), EPS, False)


# ------------------------------------------------------------------ R: float64, plain torch, decisions from O

class ReferenceOps:
    def __init__(self, torch, aux, exact=False):
        self.torch, self.aux, self.exact = torch, aux, exact

    def _c(self, a, dtype=None):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(dtype or self.torch.float64)

    # ---- PWC-Net's warp: grid_sample with zero padding times the constant mask
    def warp(self, x, flo, flo32):
        torch = self.torch
        B, C, h, w = x.shape
        _, _, fx0, fy0, inb, corners, mask = pwb.geometry(flo32, h, w, True, f32)
        ix = torch.arange(w, dtype=torch.float64)[None, None, :] + flo[:, 0]       # (align_corners: the unnormalised grid)
        iy = torch.arange(h, dtype=torch.float64)[None, :, None] + flo[:, 1]
        fx0, fy0 = self._c(fx0), self._c(fy0)
        dx1, dx0, dy1, dy0 = fx0 + 1 - ix, ix - fx0, fy0 + 1 - iy, iy - fy0
        wts = (dx1 * dy1, dx0 * dy1, dx1 * dy0, dx0 * dy0)
        flat = x.reshape(B, C, h * w)
        out = 0
        for k in range(4):
            cy, cx = corners[k]
            idx = self._c(np.clip(cy, 0, h - 1) * w + np.clip(cx, 0, w - 1), torch.int64).reshape(B, 1, h * w).expand(B, C, h * w)
            v = torch.gather(flat, 2, idx).reshape(B, C, h, w)
            out = out + v * (wts[k] * self._c(inb[k]))[:, None]
        return out * self._c(mask)[:, None]

    def costs(self, f1, f2, flos):
        torch = self.torch
        out = []
        for d, (a, b) in enumerate(((f1, f2), (f2, f1))):
            c = cl.corr64(a, self.warp(b, flos[d], self.aux["flo%d" % d]))
            out.append(torch.where(self._c(self.aux["positive%d" % d], torch.bool), c, c * SLOPE))
        return out

    # ---- the x4 bilinear upsample (align_corners False) times div_flow * t
    def upsample(self, fq, t):
        hq, wq = fq.shape[2:]
        y0, y1, ly0, ly1 = pu.up4_tap(np.arange(4 * hq), hq)
        x0, x1, lx0, lx1 = pu.up4_tap(np.arange(4 * wq), wq)
        rows = fq[:, :, y0, :] * self._c(ly0)[None, None, :, None] + fq[:, :, y1, :] * self._c(ly1)[None, None, :, None]
        full = rows[:, :, :, x0] * self._c(lx0)[None, None, None, :] + rows[:, :, :, x1] * self._c(lx1)[None, None, None, :]
        return full * (DIV_FLOW * float(t))

    # ---- FlowProjection / DepthFlowProjection, fillhole = 0
    def projection(self, flow, depth, flow32, count32):
        torch = self.torch
        B, _, H, W = flow.shape
        idx, src = [], []
        for b in range(B):
            valid, L, T = pt.targets(flow32[b, 0], flow32[b, 1], H, W)
            ys, xs = np.nonzero(valid)
            Ls, Ts = L[ys, xs], T[ys, xs]
            Rs, Bs = np.minimum(Ls + 1, W - 1), np.minimum(Ts + 1, H - 1)
            for ty, tx in ((Ts, Ls), (Ts, Rs), (Bs, Ls), (Bs, Rs)):       # (at the far edges the same cell twice)
                idx.append((b * H + ty) * W + tx)
                src.append((b * H + ys) * W + xs)
        idx, src = self._c(np.concatenate(idx), torch.int64), self._c(np.concatenate(src), torch.int64)
        d = torch.ones(B * H * W, dtype=torch.float64) if depth is None else depth.reshape(-1)
        fx, fy = flow[:, 0].reshape(-1), flow[:, 1].reshape(-1)
        num = torch.zeros(B * H * W, 2, dtype=torch.float64).index_add(0, idx, torch.stack([-(d * fx), -(d * fy)], 1)[src])
        cnt = torch.zeros(B * H * W, dtype=torch.float64).index_add(0, idx, d[src])
        pos = self._c(count32.reshape(-1) > 0, torch.bool)
        safe = torch.where(pos, cnt, torch.ones_like(cnt))[:, None]
        out = num / safe
        if depth is not None and not self.exact:       # (the reference's depth gradient: see the module docstring)
            out = (num + (safe - safe.detach()) * out.detach()) / safe.detach()
        out = torch.where(pos[:, None], out, num)
        return out.reshape(B, H, W, 2).permute(0, 3, 1, 2)

    def project(self, fq, depth, times, d):
        ups = [self.upsample(fq, t) for t in times]
        return ups, [self.projection(up, depth, self.aux["up%d_%d" % (d, i)], self.aux["count%d_%d" % (d, i)])
                     for i, up in enumerate(ups)]

    # ---- FilterInterpolation, filter size 4
    def filterinterp(self, img, flow, filt, flow32, image_only=False):
        torch = self.torch
        B, C, H, W = img.shape
        if image_only and not self.exact:
            flow, filt = flow.detach(), filt.detach()
        ys, xs = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")
        fx, fy = flow32[:, 0], flow32[:, 1]
        x2, y2 = (xs + fx).astype(f32), (ys + fy).astype(f32)
        valid = ((x2 >= 0) & (y2 >= 0) & (x2 <= f32(W - 1)) & (y2 <= f32(H - 1))
                 & (np.abs(fx) < f32(W) / f32(2)) & (np.abs(fy) < f32(H) / f32(2)))
        ix = np.where(valid, x2, 0).astype(np.int64)
        iy = np.where(valid, y2, 0).astype(np.int64)
        alpha = (self._c(xs) + flow[:, 0] - self._c(ix))[:, None]
        beta = (self._c(ys) + flow[:, 1] - self._c(iy))[:, None]
        flat = img.reshape(B, C, H * W)
        quad = [0, 0, 0, 0]                                               # TL, TR, BL, BR
        for j in range(4):
            cj = np.clip(iy - 1 + j, 0, H - 1)
            for i in range(4):
                ci = np.clip(ix - 1 + i, 0, W - 1)
                idx = self._c(cj * W + ci, torch.int64).reshape(B, 1, H * W).expand(B, C, H * W)
                v = torch.gather(flat, 2, idx).reshape(B, C, H, W)
                q = 2 * (j >= 2) + (i >= 2)
                quad[q] = quad[q] + v * filt[:, j * 4 + i][:, None]
        out = ((1 - alpha) * (1 - beta) * quad[0] + alpha * (1 - beta) * quad[1] + (1 - alpha) * beta * quad[2]
               + alpha * beta * quad[3])
        through = img if self.exact else img.detach()                     # (copied through, and given no gradient)
        return torch.where(self._c(valid, torch.bool)[:, None], out, through)

    def synth(self, ref0, ref2, offs, filts, times, c0, c2):
        torch = self.torch
        out = []
        for i, t in enumerate(times):
            p0, p2 = offs[0][i], offs[1][i]
            a0, a2 = self.aux["tap0_%d" % i], self.aux["tap1_%d" % i]
            o0, o2 = self.filterinterp(ref0, p0, filts[0], a0), self.filterinterp(ref2, p2, filts[1], a2)
            cur = o0 * float(1.0 - t) + o2 * float(t)
            parts = [cur, o0, o2, p0, p2, filts[0], filts[1]]
            if c0 is not None:
                parts += [self.filterinterp(c0, p0, filts[0], a0, True), self.filterinterp(c2, p2, filts[1], a2, True)]
            out.append((torch.cat(parts, dim=1), cur))
        return out

    def loss(self, diffs, flows, images, gt):
        return pl.torch_losses(list(diffs), gt, list(flows), list(images), EPS, False)


# ------------------------------------------------------------------ running O and R, comparing

def run(torch, ops, name, device="cpu", dtype=None, requires="all", loss_terms=None, checkpoint=False, backward=True):
    """one step on fresh leaves: (leaves, tensors, total, gradients)"""
    L = leaves(torch, name, device, dtype, requires)
    T, total = step(torch, ops, L, name, loss_terms, checkpoint)
    if backward and total is not None:
        total.backward()
    return L, T, total, gradients(T, L)


@functools.lru_cache(maxsize=None)
def oracle_and_reference(name, loss_terms=None):
    """(O's tensors, O's gradients, R's tensors, R's gradients, aux) of a configuration, computed once; treat as read-only"""
    import torch
    ops = OracleOps(torch)
    _, TO, _, GO = run(torch, ops, name, loss_terms=loss_terms)
    _, TR, _, GR = run(torch, ReferenceOps(torch, ops.aux), name, dtype=torch.float64, loss_terms=loss_terms)
    return TO, GO, TR, GR, ops.aux


def rel_err(got, ref):
    """max |got - ref| / max |ref|, in float64, on the CPU"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    return err / scale if scale > 0 else err


FLOOR = 8 * 2.0 ** -23                  # eight float32 ulps: a tensor on which O meets R to the last bit keeps a real bound

# Measured max |O - R| / max |R| per configuration (and loss subset: "slowmo/<subset>") and gradient, rounded up to two
# digits; "value_*" are forward tensors behind a reduction (tests/test_train_chain_host.py asserts that O is inside the
# table, so it cannot go stale).  Most of an entry is the Charbonnier term's conditioning: the slope of x / sqrt(x^2 + eps^2)
# reaches 1 / eps = 1000, so the 1e-7 float32 carries in x = out - gt becomes 1e-4 of the gradient's scale wherever |x| is
# about eps.  The GPU bound of a tensor is max(4 e, FLOOR) max |R|: the
# GPU graphs add in other orders than the sequential oracle (torch's tree reductions, the fixed-point image gradients,
# part_loss's double sums), each at least as exact as a sequential float32 sum, and a small constant factor covers that.
MEASURED = {
    "dain": {
        "out0": 1.1e-04, "cur0": 7.3e-05, "buf0": 3.6e-05, "tap1_0": 1.5e-05, "tap0_0": 2.2e-05, "proj1_0": 5.2e-05,
        "proj0_0": 5.5e-05, "up1_0": 7.4e-06, "up0_0": 1.4e-05, "flow_q1": 2.4e-06, "cost1": 2.0e-06,
        "flow_q0": 3.5e-06, "cost0": 2.4e-06, "f1": 2.0e-06, "f2": 1.7e-06, "flo": 2.2e-06, "ref0": 1.4e-05,
        "ref2": 4.9e-06, "filt0": 3.0e-05, "filt1": 1.4e-05, "value_out0": 6.2e-07, "value_loss_out0": 2.8e-08,
        "value_loss_cur0": 6.6e-08, "value_loss_offset": 6.7e-08, "value_loss_sym": 2.7e-08,
    },
    "slowmo": {
        "out2": 4.3e-04, "out1": 2.6e-04, "out0": 2.9e-04, "cur2": 2.5e-04, "cur1": 1.5e-04, "cur0": 1.5e-04,
        "buf2": 1.5e-04, "buf1": 8.6e-05, "buf0": 9.7e-05, "tap1_2": 5.7e-05, "tap1_1": 2.6e-05, "tap1_0": 3.5e-05,
        "tap0_2": 6.8e-05, "tap0_1": 5.7e-05, "tap0_0": 7.2e-05, "proj1_2": 5.7e-05, "proj1_1": 2.9e-04,
        "proj1_0": 3.5e-05, "proj0_2": 6.8e-05, "proj0_1": 2.7e-04, "proj0_0": 7.2e-05, "up1_2": 7.4e-06,
        "up1_1": 9.6e-05, "up1_0": 2.1e-05, "up0_2": 2.1e-05, "up0_1": 1.1e-04, "up0_0": 1.3e-05, "flow_q1": 1.1e-05,
        "cost1": 8.8e-06, "flow_q0": 8.4e-06, "cost0": 5.7e-06, "f1": 7.6e-06, "f2": 6.6e-06, "flo": 8.8e-06,
        "depth0": 1.1e-05, "depth1": 2.3e-05, "ref0": 2.4e-05, "ref2": 9.9e-06, "filt0": 2.7e-05, "filt1": 2.4e-05,
        "ctx0": 7.2e-06, "ctx2": 3.4e-06, "value_out0": 1.2e-06, "value_out1": 1.3e-06, "value_out2": 8.5e-07,
        "value_loss_out0": 9.0e-08, "value_loss_out1": 3.6e-08, "value_loss_out2": 1.7e-08, "value_loss_cur0": 6.3e-08,
        "value_loss_cur1": 1.1e-08, "value_loss_cur2": 6.0e-08, "value_loss_offset": 7.9e-09,
        "value_loss_sym": 3.8e-08,
    },
    "slowmo/one pixel": {
        "out1": 2.6e-04, "cur1": 1.9e-04, "buf1": 8.6e-05, "tap1_1": 3.0e-05, "tap0_1": 6.3e-05, "proj1_1": 3.0e-05,
        "proj0_1": 6.3e-05, "up1_1": 1.1e-05, "up0_1": 1.8e-05, "flow_q1": 1.6e-06, "cost1": 1.7e-06,
        "flow_q0": 1.6e-06, "cost0": 1.7e-06, "f1": 1.1e-06, "f2": 9.3e-07, "flo": 1.7e-06, "depth0": 6.7e-06,
        "depth1": 7.6e-06, "ref0": 2.1e-05, "ref2": 8.5e-06, "filt0": 7.6e-05, "filt1": 5.2e-05, "ctx0": 7.6e-06,
        "ctx2": 3.5e-06,
    },
    "slowmo/flow terms": {
        "proj1_1": 2.9e-04, "proj0_1": 3.2e-04, "up1_1": 1.2e-04, "up0_1": 1.4e-04, "flow_q1": 1.4e-05,
        "cost1": 9.7e-06, "flow_q0": 1.4e-05, "cost0": 1.1e-05, "f1": 1.1e-05, "f2": 7.3e-06, "flo": 1.2e-05,
        "depth0": 1.5e-05, "depth1": 2.6e-05,
    },
    "slowmo/cur only": {
        "cur2": 5.7e-04, "cur1": 4.9e-04, "cur0": 3.3e-04, "tap1_2": 2.2e-04, "tap1_1": 9.8e-05, "tap1_0": 2.0e-05,
        "tap0_2": 3.8e-05, "tap0_1": 4.3e-05, "tap0_0": 4.5e-05, "proj1_2": 2.2e-04, "proj1_1": 9.8e-05,
        "proj1_0": 2.0e-05, "proj0_2": 3.8e-05, "proj0_1": 4.3e-05, "proj0_0": 4.5e-05, "up1_2": 4.9e-05,
        "up1_1": 2.9e-05, "up1_0": 1.2e-05, "up0_2": 2.3e-05, "up0_1": 1.9e-05, "up0_0": 2.4e-05, "flow_q1": 2.4e-05,
        "cost1": 2.1e-05, "flow_q0": 1.4e-05, "cost0": 1.6e-05, "f1": 1.2e-05, "f2": 9.9e-06, "flo": 1.9e-05,
        "depth0": 6.8e-06, "depth1": 1.1e-05, "ref0": 2.3e-05, "ref2": 1.2e-05, "filt0": 2.3e-05, "filt1": 4.0e-05,
    },
}


def bound(name, tensor):
    return max(4.0 * MEASURED[name][tensor], FLOOR)


def same_bits(torch, a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return bool(torch.equal(a.contiguous().view(view), b.contiguous().view(view)))


def first_mismatch(torch, got, want, names=None):
    """the first name -- the most downstream, in the order of `gradients` -- whose tensors differ in a bit, or None"""
    for k in (names if names is not None else got):
        if k in want and not same_bits(torch, got[k], want[k]):
            return k
    return None


def outside_bound(got, ref, name, names=None):
    """[(tensor, error, bound)] of the tensors of `got` outside their bound against R, the most downstream first"""
    bad = []
    for k in (names if names is not None else got):
        if k not in ref or ref[k] is None:
            continue
        if got[k] is None:
            bad.append((k, float("inf"), bound(name, k)))
            continue
        e = rel_err(got[k], ref[k])
        if not e <= bound(name, k):
            bad.append((k, e, bound(name, k)))
    return bad


# ------------------------------------------------------------------ census: the inputs reach the cases

def census(name):
    """name of a case -> how many elements of O's forward take it"""
    cfg = CONFIGS[name]
    TO, _, _, _, aux = oracle_and_reference(name)
    H, W = frame(cfg)
    n = len(cfg["times"])
    out = {"count == 0": 0, "leaves left": 0, "leaves right": 0, "leaves top": 0, "leaves bottom": 0, "invalid": 0}
    ys, xs = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")
    for d in (0, 1):
        for t in range(n):
            out["count == 0"] += int((aux["count%d_%d" % (d, t)] == 0).sum())
            p = _np(TO["proj%d_%d" % (d, t)])
            x2, y2 = xs + p[:, 0], ys + p[:, 1]
            out["leaves left"] += int((x2 < 0).sum())
            out["leaves right"] += int((x2 > W - 1).sum())
            out["leaves top"] += int((y2 < 0).sum())
            out["leaves bottom"] += int((y2 > H - 1).sum())
            valid = ((x2 >= 0) & (y2 >= 0) & (x2 <= f32(W - 1)) & (y2 <= f32(H - 1))
                     & (np.abs(p[:, 0]) < f32(W) / f32(2)) & (np.abs(p[:, 1]) < f32(H) / f32(2)))
            out["invalid"] += int((~valid).sum())
    hq, wq = cfg["hq"], cfg["wq"]
    out["mask zero"] = sum(int((pwb.geometry(aux["flo%d" % d], hq, wq, True)[6] == 0).sum()) for d in (0, 1))
    out["lrelu positive"] = sum(int(aux["positive%d" % d].sum()) for d in (0, 1))
    out["lrelu negative"] = sum(int((~aux["positive%d" % d]).sum()) for d in (0, 1))
    # a flow term of part_loss on the frame's last row and column: the symmetry term there is not the constant eps
    mid = n // 2
    s = _np(TO["proj0_%d" % mid]) + _np(TO["proj1_%d" % mid])
    out["loss last row"] = int((s[:, :, H - 1, :] != 0).sum())
    out["loss last column"] = int((s[:, :, :, W - 1] != 0).sum())
    return out
