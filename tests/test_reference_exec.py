"""The oracle against the reference's own kernels, executed on the CPU (oracle/refexec).

`oracle/vfi_oracle.c` is this project's restatement of the reference; these tests run the reference's text itself
-- every `*_cuda_kernel.cu`, compiled with g++ behind a CUDA-on-CPU shim -- and compare.  The rules are in
tests/reference_cases.py.  The whole module needs oracle/_ref/libvfi_ref.so, which `__graft_entry__.build()` makes
when the reference checkout is present; without it the module skips, and tests/test_reference_golden.py checks the
same rules against the executor's recorded outputs instead.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle.refexec import build_ref, ref_exec as R
from tests import reference_cases as rc

pytestmark = pytest.mark.skipif(not R.available(),
                                reason="oracle/_ref/libvfi_ref.so is absent (no reference checkout at build time); "
                                       "tests/test_reference_golden.py covers the recorded outputs")

CASES = rc.cases(extra=True) if R.available() else {}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True)
def _block_order_afterwards():
    yield
    R.set_order("blocks")


def both_orders(case):
    R.set_order("raster")
    raster = rc.run_ref(R, case)
    R.set_order("blocks")
    return raster, rc.run_ref(R, case, given=raster)


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_matches_reference(name, oracle):
    case = CASES[name]
    raster, blocks = both_orders(case)
    rc.check(name, case, raster, rc.run_oracle(oracle, case, raster), blocks)


def test_tied_mindepth_depends_on_the_thread_order():
    """With tied weights the reference's read-compare-write keeps whichever thread ran last among the best: its
    two thread orders give different flows on the same input, so the oracle's raster order is one of the
    reference's outcomes (the per-case test pins it to the raster-order run), not a deviation from it."""
    differ = 0
    for name, case in CASES.items():
        if case.op == "mindepth" and case.params["tied"] and name.startswith("x_"):
            raster, blocks = both_orders(case)
            differ += not np.array_equal(raster["out0"], blocks["out0"])
            assert np.array_equal(raster["count"], blocks["count"]), name     # the best weight itself is order-free
    assert differ > 0


def test_thread_orders_visit_every_thread_once():
    """Raster order and block order are the same set of threads: a kernel that only writes its own pixel gives the
    same frame in both, on a frame that is no multiple of the 32x16 block."""
    case = CASES["x_interp"]
    raster, blocks = both_orders(case)
    assert np.array_equal(raster["out"], blocks["out"]) and np.abs(raster["out"]).sum() > 0


@pytest.mark.parametrize("fixture", ["filterinterp", "projection", "mindepth", "warp_sepconv", "correlation"])
def test_existing_fixtures_are_the_references(fixture, oracle):
    """Every array of tests/golden/*.npz that the reference defines (all but glue.npz), re-derived by the executor
    from the stored inputs: the fixtures the GPU suite consumes are the reference's results, not only the oracle's.
    They were written by the oracle at fmad=0, so the rules of tests/reference_cases.py apply unchanged: bit for
    bit (scatters in raster order), the deformable variants and the kernel_size-3 correlation where the executor's
    mask is clear.  One exception: the correlation gradients were written with the contracted multiply-add the
    oracle had alone until now; they are within 1e-4 (the bound the GPU test applies to them), and the oracle's
    fmad=0 is bit for bit."""
    g = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    R.set_order("raster")
    same = rc.same
    if fixture == "filterinterp":
        img, flow, filt, off, gout = (g[k] for k in ("fi_img", "fi_flow", "fi_filt", "fi_off", "fi_gout"))
        assert same(R.filterinterp_ori_fwd(img, flow, filt), g["fi_out"])
        for got, key in zip(R.filterinterp_ori_bwd(img, flow, filt, gout), ("fi_gimg", "fi_gflow", "fi_gfilt")):
            assert same(got, g[key]), key
        assert same(R.filterinterp_ori_fwd(img[:1], flow[:1], g["fi5_filt"]), g["fi5_out"])
        for v, name in ((0, "offset"), (1, "region"), (2, "nofilter")):
            out, mask = R.filterinterp_defor_fwd(v, img, flow, filt, off, canvas=True)
            assert mask.mean() <= rc.MASK_CAP and same(out, g["fi_out_" + name], mask), name
            r = R.filterinterp_defor_bwd(v, img, flow, filt, off, gout, canvas=True)
            px = r[-1]
            assert px.mean() <= rc.MASK_CAP
            for got, key in zip(r[1:4], ("gflow", "gfilt", "goff")):
                if got is not None:
                    assert same(got, g["fi_%s_%s" % (key, name)], np.broadcast_to(px, got.shape)), (name, key)
            # the fixture's image gradient holds the masked threads' scatters too, which only the oracle defines
            # (clamped corners): compare the two sides with those threads silenced on both
            want = oracle.filterinterp_defor_bwd(v, img, flow, filt, off, gout * ~px, fmad=0)[0]
            assert same(R.filterinterp_defor_bwd(v, img, flow, filt, off, gout * ~px)[0], want), name
    elif fixture == "projection":
        for fh in (0, 1):
            for flow, o, c in ((g["flow"], "out_fh%d", "count_fh%d"), (g["flow_q"], "outq_fh%d", "countq_fh%d")):
                out, count = R.flowproj_fwd(flow, fh)
                assert same(count, g[c % fh]) and same(out, g[o % fh]), (o, fh)
            out, count = R.depthflowproj_fwd(g["flow"], g["depth"], fh)
            assert same(out, g["dout_fh%d" % fh]) and same(count, g["dcount_fh%d" % fh]), fh
        # the backward fixtures were given counts with zeros replaced by one; no launcher reads those cells
        ones = lambda c: np.where(c > 0, c, 1).astype(np.float32)     # noqa: E731
        assert same(R.flowproj_bwd(g["flow"], ones(g["count_fh0"]), g["gout"]), g["gflow"])
        gf, gd = R.depthflowproj_bwd(g["flow"], g["depth"], ones(g["dcount_fh0"]), g["dout_fh0"], g["gout"])
        assert same(gf, g["dgflow"]) and same(gd, g["dgdepth"])
    elif fixture == "mindepth":
        for fh in (0, 1):
            out, count = R.mindepthflowproj_fwd(g["flow"], g["weight"], fh)
            assert same(out, g["out_fh%d" % fh]) and same(count, g["count_fh%d" % fh]), fh
        assert same(R.mindepthflowproj_bwd(g["flow"], g["weight"], g["count_fh0"], g["gout"], g["out_fh0"]), g["gflow"])
    elif fixture == "warp_sepconv":
        img, flow, v, h = g["img"], g["flow"], g["sep_v"], g["sep_h"]
        assert same(R.interp_fwd(img, flow), g["out"]) and same(R.interpch_fwd(img, flow), g["out"])
        assert same(R.sepconv_fwd(img, v, h), g["sep_out"])
        assert same(R.sepconvflow_fwd(v, h, img.shape[2], img.shape[3]), g["sepflow_out"])
        for fn in (R.interp_bwd, R.interpch_bwd):
            gi, gf = fn(img, flow, g["gout"])
            assert same(gi, g["gimg"]) and same(gf, g["gflow"])
        for got, key in zip(R.sepconv_bwd(img, v, h, g["sep_gout"]), ("sep_gimg", "sep_gv", "sep_gh")):
            assert same(got, g[key]), key
        for got, key in zip(R.sepconvflow_bwd(v, h, g["sepflow_gout"], img.shape[2], img.shape[3]),
                            ("sepflow_gv", "sepflow_gh")):
            assert same(got, g[key]), key
    else:
        f1, f2 = g["f1"], g["f2"]
        assert same(R.correlation_fwd(f1, f2, 4, 1, 4, 1, 1), g["out_pwc"])
        out, mask = R.correlation_fwd(f1, f2, 3, 3, 4, 1, 2, canvas=True)
        assert mask.mean() <= 0.05 and same(out, g["out_k3s2"], mask)
        assert same(R.correlation_fwd(f1[:, :8], f2[:, :8], 20, 1, 20, 2, 2), g["out_flownet"])
        g1, g2 = R.correlation_bwd(f1, f2, g["gout_pwc"], 4, 1, 4, 1, 1)
        assert rc.within(g["g1_pwc"], g1, 1e-4) and rc.within(g["g2_pwc"], g2, 1e-4)
        o1, o2 = oracle.correlation_bwd(f1, f2, g["gout_pwc"], 4, 1, 4, 1, 1, fmad=0)
        assert same(g1, o1) and same(g2, o2)


def test_sanitized_standalone_run(tmp_path, oracle):
    """The wrappers under -fsanitize=address,undefined, in a stand-alone program (the sanitizer is never loaded
    into python): every buffer is allocated at exactly the canvas size, so a clean run proves that every read and
    write of the reference stays within the margin -- all of them are accounted for -- and its outputs are the
    unsanitized library's, byte for byte."""
    if build_ref.reference_present():
        exe = build_ref.build(sanitize=True)
    elif os.path.exists(build_ref.SELFCHECK):
        exe = build_ref.SELFCHECK                       # built earlier, where the checkout was
    else:
        pytest.skip("no reference checkout to compile the sanitized program from, and no oracle/_ref/selfcheck_san")
    assert exe and os.path.exists(exe)
    names = ["fi_ori_fs6", "fi_defor0_fs4", "fi_defor1_fs4", "fi_defor2_fs4", "flowproj_edge", "flowproj_nothing",
             "depthproj_gaps", "mindepth_tied", "interp", "interpch_w1", "sepconv_fs5", "sepconvflow_fs2",
             "corr_pwc_3x2", "corr_k3s2", "x_fi_defor1_fs6_24x40", "x_fi_defor2_fs6_24x24"]
    for order in ("blocks", "raster"):
        R.set_order(order)
        with R.recording() as jobs:
            for n in names:
                rc.run_ref(R, CASES[n])
        d = tmp_path / order
        d.mkdir()
        R.dump_jobs(jobs, str(d), order)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe, str(d)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0 and "%d jobs clean" % len(jobs) in p.stdout, p.stdout[-4000:]
        for j, job in enumerate(jobs):
            for t, post in enumerate(job["post"]):
                got = np.fromfile(str(d / ("j%d_t%d.bin.out" % (j, t))), np.float32)
                assert got.tobytes() == np.ascontiguousarray(post).tobytes(), (order, job["name"], t)
