"""CPU checks of tests/proj_tiles.py, the host mirror of the projection kernels' per-tile decisions: its constants and
dispatch chain are the sources', hand-worked records and regimes hold, the fields it builds send every label through a
tile, every contributor lies in its tile's rectangle, and its FlowProjection restatement equals the oracle bit for bit on
dyadic fields and stays within the stated bound on random ones (the GPU file is tests/test_gpu_proj_tiles.py)."""
import re

import numpy as np
import pytest

from tests import proj_tiles as pt
from tests.fi_windows import source

f32 = np.float32


def test_constants_match_the_source():
    text = source(pt.SOURCE)
    for name, value in (("PROJ_TW", pt.TW), ("PROJ_TH", pt.TH), ("PROJ_BLK", pt.BLK), ("PROJ_ADD_BITS", pt.ADD_BITS),
                        ("PROJ_ADD_CELL", pt.ADD_CELL), ("PROJ_CLS_BITS", pt.CLS_BITS), ("PROJ_BLOCK_CAP", pt.BLOCK_CAP),
                        ("PROJ_NMAX", pt.NMAX), ("PROJ_INV_BITS", pt.INV_BITS)):
        m = re.search(r"^\s*#define\s+%s\s+(\S+)" % name, text, flags=re.M)
        assert m and int(m.group(1), 0) == value, name
    # the constants the mirror states itself: each defined once, in a helper both K1 families call
    flat = " ".join(text.split())
    pull, lean = pt.function_body("proj_pull"), pt.function_body("proj_pull_lean")
    ncls = "min(4, max(0, p.emax - emin) / PROJ_CLS_BITS + 1)"
    assert flat.count("max(0, p.emax - emin) / PROJ_CLS_BITS") == flat.count("/ PROJ_CLS_BITS") == 1
    assert ncls in pt.function_body("proj_plan")
    clamp = "max(-100, min(100, PROJ_ADD_BITS - ("
    assert flat.count(clamp) == flat.count("max(-100,") == 3 and pt.function_body("proj_class_scales").count(clamp) == 3
    for body in (pull, lean):
        assert "proj_plan<DEPTH>(" in body and "proj_class_scales(plan, cls)" in body
    # a source's weight class: once, both K1 families through it (proj_pull inside pull_add)
    assert flat.count(">= 3 * PROJ_CLS_BITS") == 1 and ">= 3 * PROJ_CLS_BITS" in pt.function_body("proj_weight_class")
    assert "proj_weight_class(d, emax, ncls)" in pt.function_body("pull_add") and "pull_add<DEPTH>(" in pull
    assert "proj_weight_class(d, emax, ncls)" in lean
    assert text.count("(32 - __clz(nmax - 1)) - 5") == 1 and text.count("(32 - __clz(busiest - 1)) - 5") == 1
    assert 2 ** 5 == pt.ADD_CELL


def test_dispatch_chain_matches_project_forward_list():
    text = " ".join(source(pt.SOURCE).split())
    body = text[text.index("static int project_forward_list("):text.index("static int project_forward_items(")]
    assert "bool vec_in = sf.b % 4 == 0 && sf.c % 4 == 0 && sf.h % 4 == 0 && (!DEPTH || (s2.b % 4 == 0 && s2.h % 4 == 0));" in body
    assert "bool vec_out = s1.b % 4 == 0 && s1.c % 4 == 0 && s1.h % 4 == 0 && sc.b % 4 == 0 && sc.h % 4 == 0;" in body
    assert "vec_in = vec_in && (uintptr_t)flows[k] % 16 == 0 && (!DEPTH || (uintptr_t)depths[k] % 16 == 0);" in body
    assert "vec_out = vec_out && (uintptr_t)outs[k] % 16 == 0 && (uintptr_t)counts[k] % 16 == 0;" in body
    launches = re.findall(r"(if \(vec_in[^)]*\)|else if \(vec_in\)|else) hipLaunchKernelGGL\(\(?(\w+)(<[^>]*>)?", body)
    assert "if (vec_in) { const int groups_x = (g.tiles_x + 3) / 4; hipLaunchKernelGGL((proj_scan4<DEPTH>)" in body
    assert "} else { hipLaunchKernelGGL((proj_scan<DEPTH>)" in body
    assert launches == [("if (vec_in && vec_ok && g.tiles_y <= 65535 && images <= 65535)", "proj_pull_lean", "<DEPTH>"),
                        ("else if (vec_in)", "proj_pull", "<DEPTH, true>"), ("else", "proj_pull", "<DEPTH, false>")]
    # the bindings pass the flow's strides for the outputs
    assert "project_forward<false>(input1, s1, nullptr, count, output, batch, h, w, fillhole, s1, s1, sc," in text
    # the mirror's statement of the same chain
    D = pt.dispatch
    assert D(False, (2 * 64 * 80, 64 * 80, 80), (64 * 80, 80)) == ("scan4", "lean")
    assert D(False, (2 * 64 * 80, 64 * 80, 80), (64 * 80, 80), ptr_mod16=(0, 0, 4, 0)) == ("scan4", "pull_vec")
    assert D(False, (2 * 64 * 81, 64 * 81, 81), (64 * 80, 80)) == ("scan", "pull_scalar")
    assert D(True, (2 * 64 * 80, 64 * 80, 80), (64 * 80, 80), (64 * 81, 81)) == ("scan", "pull_scalar")
    assert D(False, (2 * 64 * 80, 64 * 80, 80), (64 * 80, 80), images=65536) == ("scan4", "pull_vec")


def test_k1_scale_and_retry_statements_match_the_sources():
    text = " ".join(source(pt.SOURCE).split())
    # proj_pull: per class, retried once; proj_pull_lean: one shift for all classes, bias scaled with it
    assert "kvx -= shift; kvy -= shift; kc -= shift;" in pt.function_body("proj_pull")
    assert "const int kc = k0.kc - shift, kvx = k0.kvx - shift, kvy = k0.kvy - shift;" in pt.function_body("proj_pull_lean")
    assert "max(-100, min(100, PROJ_ADD_BITS - (p.efx + p.ec - PROJ_CLS_BITS * cls)))," in pt.function_body("proj_class_scales")
    assert "const int bias_bits = max(PROJ_ADD_BITS - shift, 0);" in text
    assert "const int Y = (int)(vlo[j] - ((unsigned)n << bias_bits));" in text
    assert "PL_BIAS" not in text


def test_shared_helpers_are_defined_once_and_called_from_every_kernel():
    text = " ".join(source(pt.SOURCE).split())
    bodies = {k: pt.function_body(k) for k in ("proj_scan", "proj_scan4", "proj_pull", "proj_pull_lean", "proj_finish")}
    # workgroup -> tile: one chain of divisions
    assert text.count("tile / per_img") == 1 and "const int b = tile / per_img;" in pt.function_body("proj_tile")
    for k, body in bodies.items():
        assert "proj_tile(" in body and "band_item(blockIdx.x, gridDim.x)" in body, k
    assert "proj_tile(band_item(blockIdx.x, gridDim.x), groups_x, g.tiles_y)" in bodies["proj_scan4"]
    # proj_finish leaves before the divisions where a tile has nothing to do
    fin = bodies["proj_finish"]
    assert fin.index("if (!fallback && (!fillhole || tflag == 0)) return;") < fin.index("proj_tile(tile, g.tiles_x, g.tiles_y)")
    # the fallback's dirty planes: cleaned by K0, marked by K1
    assert text.count("planes[i] = 0.0f;") == 1 and text.count("ws[PROJ_WS_DIRTY] =") == 1
    assert "proj_clean_dirty<64>(ws, planes);" in bodies["proj_scan"] and "proj_clean_dirty<256>(ws, planes);" in bodies["proj_scan4"]
    # K1: strip walk, quad loads, output buffers, stores and bookkeeping
    for stmt, helper in (("(lr * src.fh + px) * 4", "proj_quad_strip"), ("buf_f32x4(pl.f1, s.vo, yu * src.fh * 4)", "proj_load_quad"),
                         ("buffer_rsrc(out + oc,", "proj_out"), ("o.ro1, vo, so0, PROJ_ST_AUX);", "proj_store_quad"),
                         ("o.rcn, voc, soc, 0);", "proj_store_cell"), ("ws[PROJ_WS_DIRTY + 1] =", "proj_mark_dirty")):
        assert text.count(stmt) == 1 and stmt in pt.function_body(helper), helper
        for k in ("proj_pull", "proj_pull_lean"):
            assert re.search(r"\b%s(<[^>]*>)?\(" % helper, bodies[k]), (helper, k)
    assert "PROJ_ST_AUX" not in bodies["proj_pull"] + bodies["proj_pull_lean"]
    assert not re.search(r"#\s*ifndef\s+(PROJ_|PL_)", source(pt.SOURCE))


def test_hand_worked_records():
    h, w = 64, 256
    # a constant shift of (+3, +2): every block reaches its own tiles and the ones 3 px right / 2 px down
    flow = np.zeros((1, 2, h, w), f32)
    flow[0, 0], flow[0, 1] = 3.0, 2.0
    rec, wild = pt.records(flow, None, h, w)
    assert not wild
    ux0, uy0, uw, uh = pt.rectangle(rec[0])
    # tile (1, 1): L in [63, 127], T in [15, 31] -> x in [60, 124], y in [13, 29]
    assert (ux0[1, 1], uy0[1, 1], uw[1, 1], uh[1, 1]) == (60, 13, 65, 17)
    assert (ux0[0, 0], uy0[0, 0], uw[0, 0], uh[0, 0]) == (0, 0, 61, 14)
    assert rec[0, 0, 0, 4] == np.float32(3.0).view(np.int32) and rec[0, 0, 0, 7] == np.float32(2.0).view(np.int32)
    # one block scattered over 65 tiles: the fallback
    flow = np.zeros((1, 2, 16 * 13, 64 * 5), f32)
    ys, xs = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    flow[0, 0, :16, :16] = (xs % 5) * 64 - xs
    flow[0, 1, :16, :16] = (ys % 13) * 16 - ys
    assert pt.records(flow, None, 16 * 13, 64 * 5)[1]
    flow[0, 1, :16, :16] = (ys % 12) * 16 - ys                  # 5 x 12 = 60 tiles: no fallback
    assert not pt.records(flow, None, 16 * 13, 64 * 5)[1]


def test_weight_predicate_matches_the_source_and_spares_ordinary_calls():
    """The second fallback reason: a block whose largest |weight| the fixed-point sums cannot hold (proj_weight_unfit)."""
    text = " ".join(source(pt.SOURCE).split())
    assert ("return cbits != 0 && (unsigned)(cbits - PROJ_W_LO_BITS) >= (unsigned)(PROJ_W_HI_BITS - PROJ_W_LO_BITS);") in text
    # both K0 kernels test it beside the PROJ_BLOCK_CAP reason, on the block's largest weight over its valid sources, and on
    # the tiles proj_block_reach gives (the test itself is written out in each: as a function it changes proj_scan4's code)
    scatter, scan4 = pt.function_body("scan_scatter"), pt.function_body("proj_scan4")
    assert "> PROJ_BLOCK_CAP || proj_weight_unfit(__builtin_amdgcn_readlane(cbits, sl));" in scatter
    assert "const bool wild = any && (nx * ny > PROJ_BLOCK_CAP || proj_weight_unfit(e[5]));" in scan4
    assert text.count("proj_weight_unfit(") == 3 and text.count("> PROJ_BLOCK_CAP") == 2
    # the span of a block's targets, the tiles it reaches and its part that reaches one tile: one definition each, both K0s
    flat = " ".join(text.split())
    for helper, stmt in (("proj_block_span", "max(bx0 + range.x0, 0)"), ("proj_block_reach", "min(span.x1 + 1, g.w - 1) / PROJ_TW"),
                         ("proj_block_part", "max(bx0, ox0 - 1 - range.x1)")):
        assert stmt in pt.function_body(helper) and flat.count(stmt) == 1, helper
        assert helper + "(" in scatter and helper + "(" in scan4, helper
    assert "scan_scatter(" in pt.function_body("proj_scan")
    bits = lambda v: int(np.abs(f32(v)).view(np.int32))     # noqa: E731
    assert pt.W_LO_BITS == bits(2.0 ** -56) and pt.W_HI_BITS == bits(2.0 ** 64)
    for v, unfit in ((0.0, False), (-0.0, False), (2.0 ** -40, False), (2.0 ** 40, False), (-2.0 ** 40, False), (2.0 ** -56, False),
                     (np.nextafter(f32(2.0 ** 64), f32(0)), False), (2.0 ** 64, True), (2.0 ** 100, True), (3.4e38, True),
                     (np.inf, True), (-np.inf, True), (np.nan, True), (np.nextafter(f32(2.0 ** -56), f32(0)), True),
                     (2.0 ** -80, True), (2.0 ** -149, True)):
        assert pt.weight_unfit(bits(v)) == unfit, v
    # inside the range no scale clamp bites on account of the weight: a valid |flow| is below 2^15 (frames are at most 32767
    # wide), the last class adds (MAX_CLS - 1) * CLS_BITS
    for ec in (-55, 64):                                     # frexp exponents of 2^-56 and of the float below 2^64
        for efx in (0, 15):
            for cls in range(pt.MAX_CLS):
                assert abs(pt.ADD_BITS - (ec - pt.CLS_BITS * cls)) <= pt.K_CLAMP
                assert abs(pt.ADD_BITS - (efx + ec - pt.CLS_BITS * cls)) <= pt.K_CLAMP
    # the largest product weight x flow stays finite in fp32
    assert np.isfinite(np.nextafter(f32(2.0 ** 64), f32(0)) * f32(32767))
    # weights in [2^-40, 2^40] with flows below 2^12 keep their path; one weight outside the range sends the call away --
    # but only at a VALID source
    rng = np.random.default_rng(8)
    h, w = 48, 160
    flow = np.round(rng.uniform(-3, 3, (1, 2, h, w)) * 8).astype(f32) / 8
    depth = np.exp2(rng.integers(-40, 41, (1, 1, h, w))).astype(f32)
    assert not pt.records(flow, depth, h, w)[1]
    assert not pt.records(flow, np.zeros_like(depth), h, w)[1]
    for v in (np.inf, -np.inf, np.nan, 2.0 ** 100, -2.0 ** 64):
        d2 = depth.copy()
        d2[0, 0, 20, 70] = v
        fl = flow.copy()
        fl[0, :, 20, 70] = 0
        assert pt.records(fl, d2, h, w)[1], v
        fl[0, 0, 20, 70] = 4000.0                            # the source leaves the frame: its weight is never read
        assert not pt.records(fl, d2, h, w)[1], v
    # a whole block of tiny weights (its largest is tiny): fallback; one tiny weight beside ordinary ones: not
    d2 = depth.copy()
    d2[0, 0, 16:32, 32:48] = 2.0 ** -90
    assert pt.records(flow, d2, h, w)[1]
    d2 = depth.copy()
    d2[0, 0, 20, 70] = 2.0 ** -149
    d2[0, 0, 20, 71] = 1.0
    assert not pt.records(flow, d2, h, w)[1]


def test_hand_worked_regimes():
    h, w = 32, 128
    flow = np.full((1, 2, h, w), 0.5, f32)
    depth = np.full((1, 1, h, w), 0.75, f32)
    depth[0, 0, 20, 70] = 0.75 * 2.0 ** -7                    # a weight 7 binary orders down: two classes
    m = pt.mirror(flow, depth, "lean")
    lab = m.labels()
    assert "classes_2" in lab[(0, 1, 1)] and "plain" not in lab[(0, 1, 1)]
    assert lab[(0, 0, 0)] == {"plain"}
    kvx, kvy, kc, shift = pt.scales(flow, depth, "lean")
    # max |fx| = 0.5 -> |fx| < 2^0; max weight 0.75 -> 2^0: kvx = 25 - 0 + 6 cls, kc = 25 + 6 cls
    assert list(kvx[0, 1, 1, :2]) == [25, 31] and list(kc[0, 1, 1, :2]) == [25, 31] and not shift.any()
    # 40 sources on one top-left cell (15, 50) beside the still field's own four per cell: 44 > 32 addends, once more
    # 1 bit coarser, in both tiles whose grids hold row 15
    flow2 = np.zeros((1, 2, h, w), f32)
    flow2[0, 0, 10, :40] = 50 - np.arange(40, dtype=f32)
    flow2[0, 1, 10, :40] = 5
    m = pt.mirror(flow2, None, "lean")
    assert list(m.busy[:, 0]) == [44, 6, 44, 9] and list(m.shift[:, 0]) == [1, 0, 1, 0]
    assert "retry_1" in m.labels()[(0, 0, 0)] and "retry_1" in m.labels()[(0, 1, 0)]
    out, cnt = m.predict()
    assert cnt[0, 0, 15, 50] == 44 and cnt[0, 0, 16, 51] == 44


@pytest.mark.parametrize("kind", ["flow", "depth"])
@pytest.mark.parametrize("k1", ["lean", "pull_vec"])
@pytest.mark.parametrize("dyadic", [False, True])
def test_fields_cover_every_label(kind, k1, dyadic):
    flow, depth = pt.build_field(kind, np.random.default_rng(5), 1, dyadic=dyadic)
    m = pt.mirror(flow, depth, k1)
    assert not m.fallback
    assert pt.covered(m.labels()) >= set(pt.all_regimes(kind)), set(pt.all_regimes(kind)) - pt.covered(m.labels())
    assert m.contributors_inside().all()
    # the converging sites reach the shifts they were placed for
    for n, ty, tx in pt.SITES:
        assert m.grid_max.reshape(m.tyn, m.txn)[ty, tx] >= n


def test_contributors_inside_rectangles_on_random_fields():
    rng = np.random.default_rng(11)
    for (h, w, amp) in ((40, 130, 3.0), (70, 200, 20.0), (33, 64, 0.5)):
        flow = rng.uniform(-amp, amp, (2, 2, h, w)).astype(f32)
        m = pt.mirror(flow, None, "lean")
        assert not m.fallback and m.contributors_inside().all()


@pytest.mark.parametrize("k1", ["lean", "pull_vec"])
def test_predict_flowprojection_equals_oracle_on_dyadic_fields(oracle, k1):
    flow, _ = pt.build_field("flow", np.random.default_rng(2), 2, dyadic=True)
    out, cnt = pt.predict_flowprojection(flow, k1)
    ref, rcount = oracle.flowproj_fwd(flow, 0)
    assert np.array_equal(cnt, rcount) and np.array_equal(out, ref)


@pytest.mark.parametrize("k1", ["lean", "pull_vec"])
def test_predict_depthflowprojection_equals_oracle_on_dyadic_fields(oracle, k1):
    flow, depth = pt.build_field("depth", np.random.default_rng(3), 1, dyadic=True)
    out, cnt = pt.predict_depthflowprojection(flow, depth, k1)
    ref, rcount = oracle.depthflowproj_fwd(flow, depth, 0)
    assert np.array_equal(cnt, rcount) and np.array_equal(out, ref)


def test_predict_flowprojection_within_bound_on_random_fields():
    flow, _ = pt.build_field("flow", np.random.default_rng(4), 1)
    m = pt.mirror(flow, None, "lean")
    out, cnt = m.predict()
    err, bound = flow_errors(m, flow, out)
    assert np.all(err <= bound), (err - bound).max()


def flow_errors(m, flow, out):
    """|out - (-sum fx / n)| and its bound 2^-(kx+1) + 2^-23 |want| per cell (float64 sums of the fp32 addends)."""
    B, _, h, w = flow.shape
    sums = np.zeros((B, 2, h * w))
    n = np.zeros((B, h * w))
    for b in range(B):
        valid, L, T = pt.targets(flow[b, 0], flow[b, 1], h, w)
        R, Bm = np.minimum(L + 1, w - 1), np.minimum(T + 1, h - 1)
        for ty, tx in ((T, L), (T, R), (Bm, L), (Bm, R)):
            idx = (ty * w + tx)[valid]
            for c in range(2):
                np.add.at(sums[b, c], idx, -flow[b, c][valid].astype(np.float64))
            np.add.at(n[b], idx, 1)
    n = n.reshape(B, 1, h, w)
    want = np.where(n > 0, sums.reshape(B, 2, h, w) / np.maximum(n, 1), 0)
    kx = np.stack([m.tile_plane(m.kvx[:, 0]), m.tile_plane(m.kvy[:, 0])], 1)
    bound = np.exp2(-(kx + 1.0)) + 2.0 ** -23 * np.abs(want)
    return np.abs(out.astype(np.float64) - want), bound
