"""CPU checks of tests/corr_edges.py: the kernel-selection mirror is the dispatch the sources write, the planted inputs
contain what the GPU file (tests/test_gpu_corr_edges.py) relies on, and the oracle it compares the kernels with agrees
on them with a plain float64 numpy restatement -- NaN for NaN, infinity for infinity."""
import functools

import numpy as np
import pytest

from tests import corr_edges as ce


# ------------------------------------------------------------------ the mirror against the source text

def test_constants_come_from_the_sources():
    c = ce.constants()
    assert set(c) == {"corr_flat_threshold", "corr_big_threshold", "corr_quad_threshold", "CORR_CC_ROWS"}
    assert all(isinstance(v, int) and v > 0 for v in c.values())
    # the tile a count is taken over, per kernel, as the launches write their grids
    body = ce.function_body("correlation_forward_items")
    for grid in ("dim3 grid((ow + 31) / 32, (oh + 3) / 4, batch)", "dim3 grid((ow + 31) / 32, (oh + 7) / 8, batch)",
                 "dim3 grid((ow + 15) / 16, (oh + 3) / 4, batch)"):
        assert grid in body, grid


@pytest.mark.parametrize("func", sorted(ce.BRANCHES))
def test_branch_order_matches_the_source(func):
    """Adding, removing, moving or re-conditioning a launch fails here until the mirror follows."""
    assert ce.source_branches(func) == ce.BRANCHES[func]
    body = " ".join(ce.function_body(func).split())
    assert body.count("if (" + ce.PWC_COND + ") {") == 1
    for name, expr in ce.EXPRS[func].items():
        assert "const %s %s = %s;" % ("bool" if name == "aligned" else "int" if name == "batch" else "int64_t", name, expr) in body, name


def test_mirror_follows_its_branches():
    """Hand-worked tile counts either side of every threshold (PWC-Net's configuration, pad 4: the output is the frame)."""
    c = ce.constants()
    flat, big, quad = c["corr_flat_threshold"], c["corr_big_threshold"], c["corr_quad_threshold"]
    assert (flat, big, quad) == (64, 256, 128)                      # the shapes below are worked out for these
    k = ce.selected_kernel
    assert k(1, 8, 28, 144, 4) == ce.FLAT and k(1, 8, 29, 128, 4) == ce.ROWS2          # 7 * 9 = 63 tiles, 8 * 8 = 64
    assert k(1, 8, 29, 128, 4, aligned=False) == ce.ROWS and k(1, 8, 29, 130, 4) == ce.ROWS
    assert k(1, 8, 128, 192, 4) == ce.ROWS2 and k(1, 8, 128, 256, 4) == ce.QUAD        # 3 * 32 = 96 tiles of 64 x 4, 4 * 32 = 128
    assert k(1, 8, 128, 256, 4, aligned=False) == ce.ROWS                              # 8 * 16 = 128 tiles of 32 x 8 ...
    assert k(2, 8, 128, 256, 4, aligned=False) == ce.K1                                # ... 256 with B = 2
    assert k(1, 8, 128, 250, 4) == ce.ROWS and k(2, 8, 128, 250, 4) == ce.K1           # rows that are no multiple of 4
    assert k(1, 8, 128, 256, 0) == ce.ROWS2 and k(2, 8, 128, 256, 0) == ce.QUAD        # pad 0: 120 x 248 outputs, 4 * 30 tiles per image
    assert k(2, 8, 128, 256, 3) == ce.K1 and k(2, 8, 128, 256, 8) == ce.QUAD           # origin: (md - pad) & 3 must be 0
    assert k(1, 8, 29, 128, 4, k=3) == "corr_forward_generic" and k(1, 8, 29, 128, 4, s2=2) == "corr_forward_generic"
    h = functools.partial(k, half=True)
    assert h(1, 8, 60, 256, 4) == "corr_forward_generic_f16" and h(1, 8, 61, 256, 4) == "corr_forward_k1_rows2_f16"   # 240, 256
    assert h(1, 8, 64, 256, 4, aligned=False) == h(1, 8, 64, 254, 4) == h(1, 8, 64, 256, 4, md=2) == "corr_forward_generic_f16"


def test_every_case_reaches_the_kernel_it_names():
    for name, (dtype, shape, cfg, dense, offset) in ce.CASES.items():
        kw = dict(half=dtype == np.float16, k=cfg[1], md=cfg[2], s1=cfg[3], s2=cfg[4])
        assert ce.selected_kernel(*shape, cfg[0], **kw) == dense, name
        assert ce.selected_kernel(*shape, cfg[0], aligned=False, **kw) == offset, name
    dense = {v[3] for v in ce.CASES.values()} | {v[4] for v in ce.CASES.values()}
    assert dense == {k for chain in ce.BRANCHES.values() for _, k in chain}, "a forward kernel without a case"


def test_pair_entry_selects_what_the_single_call_selects():
    """vfi_correlation_forward_pair decides on the pair's tile count, and every threshold it compares with is multiplied
    by the number of items: no shape takes one kernel as a pair and another alone.  (Searched, not assumed: a threshold
    that stops scaling with nitems shows here, and the GPU file's pair test would then need such a shape.)"""
    differ = [(B, H, W, pad, al) for B in (1, 2, 3) for H in range(9, 160, 3) for W in range(12, 300, 2) for pad in (0, 4, 8)
              for al in (True, False)
              if ce.selected_kernel(B, 8, H, W, pad, nitems=2, aligned=al) != ce.selected_kernel(B, 8, H, W, pad, aligned=al)]
    assert not differ, differ[:5]


# ------------------------------------------------------------------ the comparison

def test_same_bits_nan_aware():
    for dt in (np.float32, np.float16):
        a = np.array([1.0, -0.0, np.inf, np.nan, 6e-8], dt)
        assert ce.same_bits_nan_aware(a, a.copy())
        b = a.copy()
        b.view({2: np.uint16, 4: np.uint32}[a.itemsize])[3] ^= 0x8001          # another NaN: sign and payload differ
        assert np.isnan(b[3]) and ce.same_bits_nan_aware(a, b)
        for i, v in ((1, 0.0), (2, -np.inf), (3, np.inf), (0, np.nan), (4, 0.0)):
            b = a.copy()
            b[i] = v
            assert not ce.same_bits_nan_aware(a, b), (dt, i)
            assert "1 of 5 differ" in ce.describe_difference(a, b)
    assert not ce.same_bits_nan_aware(np.zeros(3, np.float32), np.zeros(3, np.float16))


# ------------------------------------------------------------------ the planted inputs and the oracle on them

@functools.lru_cache(maxsize=None)
def oracle_result(name):
    from oracle import cpu_oracle
    cpu_oracle.build()
    f1, f2, planted, cfg = ce.case_inputs(name)
    with np.errstate(all="ignore"):                     # (the half restatement is numpy: inf * 0 and overflow are the point)
        if f1.dtype == np.float16:
            return cpu_oracle.correlation_fwd_f16(f1, f2, *cfg)
        return cpu_oracle.correlation_fwd(f1, f2, *cfg, order=1, fmad=1)


def test_planted_set_is_complete():
    for name in ce.CASES:
        f1, f2, planted, cfg = ce.case_inputs(name)
        B, C, H, W = f1.shape
        kinds = {(what, m) for what, m, *_ in planted}
        for m in ("f1", "f2"):
            for wi, where in enumerate(("corner", "edge", "interior")):
                for vi, what in enumerate(("+inf", "-inf", "nan")):
                    if name not in ce.SPARSE or vi == (wi + (m == "f2")) % 3:
                        assert ("%s %s" % (what, where), m) in kinds, (name, m, what, where)
            assert {("overflow", m), ("inf - inf", m), ("subnormal", m), ("-0.0", m)} <= kinds
        maps = {"f1": f1, "f2": f2}
        for what, m, b, c, y, x in planted:
            v = maps[m][b, c, y, x]
            on_border = y in (0, H - 1) or x in (0, W - 1)
            if what.endswith("corner"):
                assert (y in (0, H - 1)) and (x in (0, W - 1))
            elif what.endswith("edge"):
                assert on_border and not ((y in (0, H - 1)) and (x in (0, W - 1)))
            elif what.endswith(("interior", "near border")):
                assert not on_border
            if what.startswith(("+inf", "-inf")):
                assert np.isinf(v) and (v > 0) == what.startswith("+")
            elif what.startswith("nan"):
                assert np.isnan(v)
            elif what == "-0.0":
                assert v == 0 and np.signbit(v)
        # a non-finite value in the last channel: the partial chunk of the 4- and the CORR_CC_ROWS-channel kernels
        assert C % 4 and C % ce.constants()["CORR_CC_ROWS"]
        assert any(c == C - 1 and not np.isfinite(maps[m][b, c, y, x]) for _, m, b, c, y, x in planted), name
        # no two items of an image share a pixel, except the two sides of a product
        seen = {}
        for what, m, b, c, y, x in planted:
            assert seen.setdefault((b, y, x), what) == what, (name, what, seen[(b, y, x)])
        # the products: overflow, two of opposite sign in one column, subnormal
        big = [(b, c, y, x) for what, m, b, c, y, x in planted if what == "inf - inf" and m == "f1"]
        assert len(big) == 2 and big[0][0] == big[1][0] and big[0][2:] == big[1][2:] and big[0][1] != big[1][1]
        with np.errstate(over="ignore"):
            for what, m, b, c, y, x in planted:
                if m != "f1":
                    continue
                p = (f1[b, c, y, x].astype(np.float64) * f2[b, c, y, x].astype(np.float64)).astype(f1.dtype)
                if what in ("overflow", "inf - inf"):
                    assert np.isinf(p), (name, what)
                elif what == "subnormal":
                    assert 0 < abs(p) < np.finfo(f1.dtype).tiny, (name, p)
            assert np.isinf(np.float32(3e38) * np.float32(3e38)) and np.isinf(np.float16(300) * np.float16(300))


@pytest.mark.parametrize("name", sorted(ce.CASES))
def test_oracle_equals_plain_float64_reference_on_planted_inputs(name):
    """The oracle the GPU file compares with, against products in float64 over zero-padded arrays: NaN at the same
    places, +inf and -inf at the same places; and (beyond what is asked) every finite value within the float format's
    rounding of the sequential sum."""
    f1, f2, planted, cfg = ce.case_inputs(name)
    got, want = oracle_result(name), ce.reference(f1, f2, cfg)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(np.isnan(got), np.isnan(want))
    for inf in (np.inf, -np.inf):
        assert np.array_equal(got == inf, want == inf)
    if f1.dtype == np.float16:
        assert ce.same_bits_nan_aware(got, want), ce.describe_difference(got, want)     # the same operations exactly
    else:
        # float: the reference rounds a * b + acc twice (to float64, then to float32), the oracle's fmaf once: they
        # differ by at most one unit in the last place of the sum per term where a double rounding falls on a tie
        fin = np.isfinite(want)
        C = f1.shape[1] * cfg[1] ** 2
        scale = np.maximum(np.abs(want[fin]), np.finfo(np.float32).tiny)
        assert np.all(np.abs(got[fin].astype(np.float64) - want[fin]) <= C * 2.0 ** -23 * np.maximum(scale, 1.0))


@pytest.mark.parametrize("name", sorted(ce.CASES))
def test_planted_cases_keep_the_gpu_test_honest(name):
    """On the oracle's result alone: the poison stays local, a NaN comes from a padding tap alone, an infinity and a
    subnormal survive."""
    f1, f2, planted, cfg = ce.case_inputs(name)
    want = oracle_result(name)
    pad, k, md = cfg[:3]
    assert (~np.isfinite(want)).mean() <= 0.25, (~np.isfinite(want)).mean()
    s1, s2 = ce.padding_sites(f1, f2, cfg)
    # a planted f1 pixel whose second-map tap lies outside the frame: wherever the output reaches past the frame
    if pad > 0:
        assert s1.any() and np.isnan(want[s1]).all(), name
    else:
        assert not s1.any()
    # the mirror case needs the first map's tap outside the frame: an output origin (less the kernel radius) outside it
    if pad > md - (k - 1) // 2:
        assert s2.any() and np.isnan(want[s2]).all(), name
    else:
        assert not s2.any()
    assert np.isposinf(want).any() and np.isneginf(want).any()
    tiny = np.finfo(want.dtype).tiny
    assert ((want != 0) & (np.abs(want) < tiny)).any(), "no subnormal result"
    assert np.isnan(want).any() and np.isfinite(want).any()


def test_padding_sites_hand_worked():
    """One +inf at f1's corner (0, 0) of a 6 x 13 frame, pad 4: output pixel (0, 0) meets the padding wherever the
    displacement points up or left -- rows tj < 4 (36 outputs) and columns ti < 4 of the other rows (20)."""
    f1 = np.ones((1, 3, 6, 13), np.float32)
    f2 = np.ones_like(f1)
    f1[0, 2, 0, 0] = np.inf
    s1, s2 = ce.padding_sites(f1, f2, ce.PWC)
    assert s1.sum() == 56 and not s2.any() and s1[0, :, 0, 0].sum() == 56
    assert s1[0, :, 0, 0].reshape(9, 9)[:4].all() and s1[0, :, 0, 0].reshape(9, 9)[4:, :4].all()
    ref = ce.reference(f1, f2, ce.PWC)
    assert np.isnan(ref[0, :, 0, 0]).sum() == 56 and np.isposinf(ref[0, :, 0, 0]).sum() == 25
    # pad 8: output pixel (0, 0) is centred on input (-4, -4); the second map's corner tap is reached by displacement
    # (+4, +4) of output (0, 0) alone among the outputs whose own centre is outside
    f2[0, 1, 0, 0] = -np.inf
    f1[0, 2, 0, 0] = 1.0
    s1, s2 = ce.padding_sites(f1, f2, (8, 1, 4, 1, 1))
    assert s2[0, 80, 0, 0] and not s1.any() and np.isnan(ce.reference(f1, f2, (8, 1, 4, 1, 1))[0, 80, 0, 0])


# ------------------------------------------------------------------ the warp's planted field

def test_warp_field_has_a_zero_weight_corner_and_a_masked_pixel():
    for ac in (True, False):
        f1, f2, flo = ce.warp_inputs(ac)
        zero_w, masked = ce.warp_zero_weight_sites(f2, flo, ac)
        assert masked.any(), ac
        assert np.isfinite(flo).all()
        if ac:
            # an integer flow lands on a pixel centre: the east / south neighbours are in the map with weight exactly 0
            assert zero_w.any()
            from oracle import cpu_oracle
            cpu_oracle.build()
            w = cpu_oracle.pwc_warp(f2, flo, ac, fmad=1)
            assert np.isnan(w).any(axis=1)[zero_w].all()
            assert np.isnan(w).any(axis=1)[masked].all()           # inf * 0 of the mask
            assert np.isfinite(w).mean() > 0.75
