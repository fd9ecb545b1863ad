"""CPU checks of tests/bwd_tiles.py, the host mirror of the LDS-staged backward kernels' per-tile decisions: its decision
expressions are the sources', hand-worked tiles sit on either side of every threshold, the fields it builds send every
reachable label through a tile of every batch item (and direction), and its image-gradient restatement equals the C
oracle bit for bit on dyadic inputs and stays within the float64 bound on random ones (the GPU file is
tests/test_gpu_bwd_tiles.py)."""
import numpy as np
import pytest

from tests import bwd_tiles as bt
from tests.fi_windows import source, source_expr

f32 = np.float32


def _flat(name):
    return " ".join(source(name).split())


def test_decision_expressions_match_the_sources():
    fi, de, ws, pw = (_flat(n) for n in ("filterinterp.hip", "filterinterp_defor_bwd_lds.hip", "warp_sepconv.hip",
                                          "pwc_warp_backward.hip"))
    assert "const int slot_floats = (n + FB_THREADS - 1) & ~(FB_THREADS - 1);" in fi
    assert "const int pc = min(CH, FB_CELLS / slot_floats);" in fi
    assert "constexpr int CH = (BLEND && WANT_X) ? 1 : FB_CH;" in fi
    assert "const int pc = min(DB_CH, DB_CELLS / max(ncell, 1));" in de
    assert "const int pitch = (bw + 31) & ~31;" in de
    assert "if (!gradacc_staged_ok(gctx) || box[8] || n64 > DB_WIN_FLOATS || pc == 0) {" in de
    assert "finite = finite && fabsf(fracY) < 1e9f && fabsf(fracX) < 1e9f;" in de
    assert "const int pc = min(IB_CH, IB_CELLS / n);" in ws
    assert "if (!gradacc_staged_ok(gctx) || pc == 0) {" in ws
    assert "if (cells_per_channel <= PB_CELLS) {" in pw and "step = min(PB_CH, PB_CELLS / n);" in pw
    # the launcher's channel groups
    assert "int groups = (int)std::min<int64_t>(c8, std::max<int64_t>(1, (device_cu_count() + ntiles - 1) / ntiles));" in pw
    assert "const int cgroup = PB_CH * ((c8 + groups - 1) / groups);" in pw
    assert "groups = (channel + cgroup - 1) / cgroup;" in pw
    # the per-tap kernels find the staged kernels' flags by recomputing the 64x8 tile from their 64x4 blocks
    assert source_expr("filterinterp.hip", r"if \(tileflag && (!tileflag\[[^;]*\])\) return;") == \
        "!tileflag[(zb * ((h + FB_TH - 1) / FB_TH) + y / FB_TH) * gridDim.x + blockIdx.x]"
    assert source_expr("warp_sepconv.hip", r"if \(tileflag && (!tileflag\[[^;]*\])\) return;") == \
        "!tileflag[(b * ((h + IB_TH - 1) / IB_TH) + y / IB_TH) * gridDim.x + blockIdx.x]"
    assert fi.count("tileflag[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = 1;") == 1
    # the blend's per-tap kernel passes the staged launch's z (direction * batch + b) as the flags' plane
    assert "tileflag, (int)blockIdx.z - dir * batch, blockIdx.z, fc);" in fi
    # the addends, as the restatement forms them
    assert "__float2ll_rn(qg[cc][quad] * fv[k] * gctx.scale)" in fi
    assert "__float2ll_rn(g * (1.0f - alpha) * (1.0f - beta) * gctx.scale)" in ws
    assert "__float2ll_rn(qgq * wg * gctx.scale)" in de and "__float2ll_rn(qgq * gctx.scale)" in de
    assert "__float2ll_rn(anw_v * gctx.scale)" in pw
    assert "return v * cx.scale * cx.scale2;" in _flat("gradacc.h")
    assert "cells[x] += (float)ldexp((double)sum, -k);" in _flat("gradacc.hip")


def test_constants_come_from_the_sources():
    assert (bt.FB_TW, bt.FB_TH, bt.FB_THREADS, bt.FB_CH, bt.FB_CELLS) == (64, 8, 512, 3, 6144)
    assert (bt.IB_TW, bt.IB_TH, bt.IB_CH, bt.IB_CELLS) == (64, 8, 3, 6144)
    assert (bt.DB_TW, bt.DB_TH, bt.DB_CH, bt.DB_WIN_FLOATS, bt.DB_CELLS) == (64, 4, 3, 3840, 4096)
    assert (bt.PB_TW, bt.PB_TH, bt.PB_CH, bt.PB_CELLS) == (64, 8, 8, 6144)


def _last(f, lo, hi, v):
    """the largest n in [lo, hi] with f(n) == v"""
    return max(n for n in range(lo, hi + 1) if f(n) == v)


def test_thresholds_on_either_side():
    ori = lambda n: bt.ori_channels(n, bt.FB_CH)
    assert [_last(ori, 1, 7000, pc) for pc in (3, 2, 1)] == [2048, 3072, 6144] and ori(6145) == 0
    assert [ori(n) for n in (2048, 2049, 3072, 3073, 6144, 6145)] == [3, 2, 2, 1, 1, 0]
    assert [bt.ori_channels(n, bt.blend_ch(True)) for n in (1, 6144, 6145)] == [1, 1, 0]
    assert [bt.interp_channels(n) for n in (2048, 2049, 3072, 3073, 6144, 6145)] == [3, 2, 2, 1, 1, 0]
    assert [bt.defor_channels(n) for n in (1365, 1366, 2048, 2049, 4096, 4097)] == [3, 2, 2, 1, 1, 0]
    assert bt.defor_window(32, 120) == (32, 3840) and bt.defor_window(33, 60)[1] == 3840
    assert bt.defor_window(33, 61)[1] > bt.DB_WIN_FLOATS
    assert [bt.warp_step(n) for n in (768, 769, 3072, 3073, 6144, 6145)] == [8, 7, 2, 1, 1, None]
    assert bt.warp_groups(1, 16, 123, 360) == (8, 2) and bt.warp_groups(1, 7, 123, 360) == (8, 1)


def test_hand_worked_tiles():
    h, w = 24, 200
    flow = np.zeros((1, 2, h, w), f32)
    rec = bt.tiles("ori", flow, 7)
    # an interior tile: taps x - 1 .. x + 2, y - 1 .. y + 2 -> 67 x 11 cells, three channels per pass, 7 = 3 + 3 + 1
    assert rec[0, 1, 1]["box"] == (63, 7, 129, 17) and rec[0, 1, 1]["n"] == 67 * 11
    assert rec[0, 1, 1]["labels"] == {"pc3", "short_pass"}
    assert rec[0, 0, 0]["labels"] == {"pc3", "short_pass", "edge_left", "edge_top"}
    assert rec[0, 2, 3]["labels"] == {"pc3", "short_pass", "edge_right", "edge_bottom", "ragged_right"}
    assert bt.tiles("ori", flow, 6)[0, 1, 1]["labels"] == {"pc3"}
    assert bt.tiles("interp", flow, 3)[0, 1, 1]["box"] == (64, 8, 128, 16)
    rec = bt.tiles("defor", flow, 3, off=np.zeros((1, 32, h, w), f32))
    assert rec[0, 1, 1]["box"] == (63, 3, 129, 9) and rec[0, 1, 1]["window"] == (63, 3, 130, 10)
    # a y shear that takes the box to 67 x 31 (n = 2077: two channels) and to 67 x 92 (6164: flagged)
    for rows, want in ((31, "pc2"), (46, "pc1"), (92, "flag_window")):
        f = np.zeros((1, 2, 128, 200), f32)
        f[0, 1, 64:72, 64:128] = np.arange(64, dtype=f32)[None, :] * f32((rows - 11) / 63.0) - f32((rows - 11) / 2.0)
        r = bt.tiles("ori", f, 4)[0, 8, 1]
        assert want in r["labels"], (rows, r)
    # an h % 8 <= 4 frame: the last tile row is ragged (the per-tap kernel's second 64x4 block lies outside)
    assert "ragged_bottom" in bt.tiles("ori", np.zeros((1, 2, 20, 64), f32), 1)[0, 2, 0]["labels"]
    assert "ragged_bottom" not in bt.tiles("ori", np.zeros((1, 2, 22, 64), f32), 1)[0, 2, 0]["labels"]


CASES = [("ori", None), ("blend", None), ("blend_nox", None), ("interp", None), ("warp", None), ("defor", 0), ("defor", 1),
         ("defor", 2)]


@pytest.mark.parametrize("kernel,variant", CASES)
def test_built_fields_cover_every_label(kernel, variant):
    dirs = 2 if kernel.startswith("blend") else 1
    flows, offs = bt.build_field(kernel, np.random.default_rng(7), 2, dirs=dirs)
    flows, offs = (flows, offs) if dirs == 2 else ([flows], [offs])
    seen = []
    for flow, off in zip(flows, offs):
        recs = bt.tiles(kernel, flow, 7, off=off)
        for b in range(2):
            counts = bt.label_counts(recs, b)
            missing = [lab for lab in bt.all_labels(kernel) if lab not in counts]
            assert not missing, (kernel, b, missing, counts)
            seen.append({k: frozenset(r["labels"]) for k, r in recs.items() if k[0] == b})
    if dirs == 2:       # the two directions put different classes on the same tiles
        assert seen[0] != seen[2] and seen[1] != seen[3]


def _dyadic(a, q):
    return (np.round(a * q) / q).astype(f32)


@pytest.mark.parametrize("kernel,variant", [("ori", None), ("interp", None), ("defor", 0), ("defor", 1), ("defor", 2)])
def test_restatement_equals_the_oracle_on_dyadic_inputs(oracle, kernel, variant):
    """dyadic flows, filters, offsets and gradients: every addend and every partial sum exact, so the oracle's sequential
    fp32 sums, the float64 sums and the restatement agree bit for bit (from a zero start, and added into a start)"""
    rng = np.random.default_rng(11)
    B, C, h, w = 2, 3, 21, 70
    flow = _dyadic(rng.uniform(-3, 3, (B, 2, h, w)), 4)
    flow[0, 0, :4] = f32(1000)                              # invalid pixels
    img = rng.random((B, C, h, w), dtype=f32)
    filt = _dyadic(rng.random((B, 16, h, w)), 16)
    off = _dyadic(rng.uniform(-1.5, 1.5, (B, 32, h, w)), 4)
    gout = _dyadic(rng.standard_normal((B, C, h, w)), 16)
    if kernel == "ori":
        ref = oracle.filterinterp_ori_bwd(img, flow, filt, gout, fmad=1)[0]
    elif kernel == "interp":
        ref = oracle.interp_bwd(img, flow, gout, fmad=1)[0]
    else:
        ref = oracle.filterinterp_defor_bwd(variant, img, flow, filt, off, gout, fmad=1)[0]
    zero = np.zeros_like(img)
    got, k, fp32 = bt.predict_image_grad(kernel, flow, gout, zero, filt, off, variant or 0)
    assert not fp32 and np.array_equal(got, ref)
    g0 = _dyadic(rng.standard_normal(img.shape), 8)
    got, _, _ = bt.predict_image_grad(kernel, flow, gout, g0, filt, off, variant or 0)
    assert np.array_equal(got, (g0 + ref).astype(f32))


@pytest.mark.parametrize("kernel,variant", [("ori", None), ("interp", None), ("defor", 1), ("defor", 2)])
def test_restatement_within_the_float64_bound(np_oracle, kernel, variant):
    from tests.test_gpu_backward import IMG_ROUNDINGS, U
    rng = np.random.default_rng(12)
    B, C, h, w = 1, 2, 19, 67
    flow = rng.uniform(-4, 4, (B, 2, h, w)).astype(f32)
    filt = rng.random((B, 16, h, w), dtype=f32)
    off = rng.uniform(-1.5, 1.5, (B, 32, h, w)).astype(f32)
    gout = rng.standard_normal((B, C, h, w)).astype(f32)
    if kernel == "ori":
        e, S, n = np_oracle.filterinterp_ori_bwd_img(flow, filt, gout)
    elif kernel == "interp":
        e, S, n = np_oracle.interp_bwd_img(flow, gout)
    else:
        e, S, n = np_oracle.filterinterp_defor_bwd(variant, np.zeros((B, C, h, w), f32), flow, filt, off, gout,
                                                   img_stats=True)[0]
    got, k, _ = bt.predict_image_grad(kernel, flow, gout, np.zeros((B, C, h, w), f32), filt, off, variant or 0)
    kind = "defor" if kernel == "defor" else kernel
    bound = IMG_ROUNDINGS[kind] * U * S * (1 + 1e-6) + n * 2.0 ** -(k + 1) + np.abs(np.spacing(e.astype(f32)))
    assert np.all(np.abs(got.astype(np.float64) - e) <= bound)


def test_warp_restatement_within_the_float64_bound():
    from tests.pwc_warp_backward import pwc_warp_bwd
    rng = np.random.default_rng(13)
    x = rng.standard_normal((2, 3, 20, 70)).astype(f32)
    flo = rng.uniform(-3, 3, (2, 2, 20, 70)).astype(f32)
    g = rng.standard_normal(x.shape).astype(f32)
    gx, _, A, _, _ = pwc_warp_bwd(x, flo, g, True)
    got, k, _ = bt.predict_image_grad("warp", flo, g, np.zeros_like(x))
    assert np.all(np.abs(got - gx) <= 4e-7 * A + 2.0 ** -(k - 2) + np.abs(np.spacing(gx.astype(f32))))


def test_scale_exponent_hand_worked():
    """k = 62 - L - eg - max(ew, 1), every term written out: 2^L >= h w max(taps, 4), 2^eg > max |g|, 2^ew > max |weight|"""
    cases = [  # gout, weights, h, w, taps, k, fp32 path (the maxima are all grad_scale takes from the tensors)
        ([0.25, -1.5], [0.5, 0.0], 9, 33, 16, 62 - 13 - 1 - 1, False),      # 9 * 33 * 16 = 4752 <= 2^13, 1.5 < 2^1, ew 0 -> 1
        ([0.25, -1.5], None, 9, 33, 4, 62 - 11 - 1 - 1, False),             # 9 * 33 * 4 = 1188 <= 2^11, no weights: ew = 1
        ([1.0], None, 1, 128, 4, 62 - 9 - 1 - 1, False),                    # h w taps = 512 = 2^9; 1.0 = 0.5 * 2^1
        ([1.0], None, 1, 129, 4, 62 - 10 - 1 - 1, False),                   # 516: one column above the power of two
        ([0.0, 4.0], None, 9, 33, 4, 62 - 11 - 3 - 1, False),               # max |g| a power of two: 4 = 0.5 * 2^3
        ([np.nextafter(f32(4), f32(0))], None, 9, 33, 4, 62 - 11 - 2 - 1, False),   # and just below: < 2^2
        ([1.5], [0.0, 0.75], 9, 33, 16, 62 - 13 - 1 - 1, False),            # weights below 1: ew clamps to 1
        ([1.5], [0.0, 3.0], 9, 33, 16, 62 - 13 - 1 - 2, False),             # weights above 1: 3 < 2^2
        ([0.0, 0.0], None, 9, 33, 4, 62 - 11 - 0 - 1, False),               # an all-zero gradient: eg = 0
        ([3e38], [3.0], 9, 33, 16, 62 - 13 - 128 - 2, True),                # 2^127 <= 3e38 < 2^128: eg + ew = 130 > 128
    ]
    assert [c[5] for c in cases] == [47, 49, 51, 50, 47, 48, 47, 46, 50, -81]
    for g, wt, h, w, taps, k, fp32 in cases:
        assert bt.grad_scale(g, wt, h, w, taps)[:2] == (k, fp32)
    k, fp32, scale, scale2 = bt.grad_scale(np.full((1, 1, 9, 33), 1e-30, f32), None, 9, 33, 4)
    assert k > 126 and not fp32 and scale2 != 1
    assert bt.grad_scale(np.array([[[[np.inf]]]], f32), None, 1, 1, 4)[1]
