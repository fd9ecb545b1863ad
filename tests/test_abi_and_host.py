"""CPU suite, part 2: the C-ABI library and the host-side logic (no GPU compute).

  * libvfi_hip.so loads and exports every symbol include/vfi_hip.h declares;
  * the ctypes table of the package matches the header;
  * the eight reference-named extension modules import and expose the reference's names;
  * the product never imports the oracle;
  * synthetic inputs are deterministic; padding rule; pair sharding incl. a 2-rank gloo run.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video-frame-interpolation-based-on-deformable-kernel-region_amd")


@pytest.fixture(scope="module")
def built():
    """Build the native artefacts in-tree if they are missing (hipcc cross-compiles without a GPU)."""
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import build
    build.build_all()
    return build


def header_functions():
    text = open(os.path.join(ROOT, "include", "vfi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.findall(r"\b(?:int|const char\*)\s+(vfi_\w+)\s*\(", text)


def test_library_exports_every_declared_symbol(built):
    names = header_functions()
    assert len(names) >= 17 and "vfi_filterinterp_forward_ori" in names and "vfi_correlation_forward" in names
    lib = ctypes.CDLL(built.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), "libvfi_hip.so does not export %s" % n
    lib.vfi_version.restype = ctypes.c_char_p
    assert b"gfx950" in lib.vfi_version()
    # pure helper: no GPU needed (correlation_cuda.cc:23-36)
    oc, oh, ow = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.vfi_correlation_output_dims(10, 12, 4, 1, 4, 1, 1, ctypes.byref(oc), ctypes.byref(oh), ctypes.byref(ow)) == 0
    assert (oc.value, oh.value, ow.value) == (81, 10, 12)
    assert lib.vfi_correlation_output_dims(10, 12, 20, 1, 20, 2, 2, ctypes.byref(oc), ctypes.byref(oh), ctypes.byref(ow)) == 0
    assert (oc.value, oh.value, ow.value) == (441, 5, 6)


def test_product_library_exports_no_development_knobs(built):
    """Kernel-selection thresholds are compile-time constants: the library exports the declared ABI, the internal
    single-path entry points the tests and tools time, and nothing that mutates process-global state."""
    out = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("vfi_")}
    from vfidkr_amd import cabi
    # the per-path launchers the public entry points dispatch to are C++ functions of csrc/filterinterp_paths.h, not exports
    expected = set(header_functions()) | set(cabi.INTERNAL_SIGNATURES)
    assert exported == expected, sorted(exported ^ expected)


def test_ctypes_table_matches_header(built):
    from vfidkr_amd import cabi
    declared = set(header_functions()) - {"vfi_version"}
    assert declared == set(cabi.SIGNATURES), declared ^ set(cabi.SIGNATURES)
    cabi.lib()      # sets argtypes on every entry: fails if a symbol is missing
    # null pointers / bad sizes are shape errors, not launches (safe without a GPU)
    s = cabi.Strides(0, 0, 0)
    assert cabi.lib().vfi_filterinterp_forward_ori(None, None, None, None, 1, 3, 8, 8, 16, s, s, s, None) == 1
    assert cabi.lib().vfi_flowprojection_forward(None, None, None, 0, 8, 8, 1, s, s, None) == 1
    assert cabi.lib().vfi_correlation_forward(None, None, None, 1, 1, 8, 8, 4, 1, 4, 1, 1, None) == 1


REFERENCE_EXPORTS = {
    "filterinterpolation_cuda": ["FilterInterpolationLayer_gpu_forward_ori", "FilterInterpolationLayer_gpu_backward_ori",
                                 "FilterInterpolationLayer_gpu_forward", "FilterInterpolationLayer_gpu_forward_deforconv",
                                 "FilterInterpolationLayer_gpu_forward_nofilterwithdeforconv",
                                 "FilterInterpolationLayer_gpu_backward", "FilterInterpolationLayer_gpu_backward_deforconv",
                                 "FilterInterpolationLayer_gpu_backward_nofilterwithdeforconv"],
    "flowprojection_cuda": ["FlowProjectionLayer_gpu_forward", "FlowProjectionLayer_gpu_backward"],
    "depthflowprojection_cuda": ["DepthFlowProjectionLayer_gpu_forward", "DepthFlowProjectionLayer_gpu_backward"],
    "mindepthflowprojection_cuda": ["minDepthFlowProjectionLayer_gpu_forward", "minDepthFlowProjectionLayer_gpu_backward"],
    "interpolation_cuda": ["InterpolationLayer_gpu_forward", "InterpolationLayer_gpu_backward"],
    "interpolationch_cuda": ["InterpolationChLayer_gpu_forward", "InterpolationChLayer_gpu_backward"],
    "separableconv_cuda": ["SeparableConvLayer_gpu_forward", "SeparableConvLayer_gpu_backward"],
    "separableconvflow_cuda": ["SeparableConvFlowLayer_gpu_forward", "SeparableConvFlowLayer_gpu_backward"],
    "correlation_cuda": ["forward", "backward"],
}


def test_extension_modules_have_reference_names(built):
    import importlib
    import vfidkr_amd  # noqa: F401  (puts ext/ on sys.path)
    for mod, funcs in REFERENCE_EXPORTS.items():
        m = importlib.import_module(mod)
        assert os.path.dirname(m.__file__) == os.path.join(PKG, "ext")      # in-tree, not site-packages
        for f in funcs:
            assert callable(getattr(m, f)), "%s.%s missing" % (mod, f)


def test_wrapper_mirrors_import_and_reject_cpu_tensors(built):
    import torch
    from vfidkr_amd.my_package.FilterInterpolation import FilterInterpolationModule
    from vfidkr_amd.my_package.FlowProjection import FlowProjectionModule
    from vfidkr_amd.my_package.DepthFlowProjection import DepthFlowProjectionModule
    from vfidkr_amd.PWCNet.correlation_package_pytorch1_0.correlation import Correlation
    assert FlowProjectionModule().requires_grad is True and DepthFlowProjectionModule(False).requires_grad is False
    with pytest.raises(RuntimeError, match="no CPU path"):
        FilterInterpolationModule()(torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8, 8), torch.zeros(1, 16, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        FlowProjectionModule(False)(torch.zeros(1, 2, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        Correlation(4, 1, 4, 1, 1, 1)(torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 8, 8))


def test_product_never_imports_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline may touch oracle/."""
    offenders = []
    for dirpath, _, files in os.walk(PKG):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                if re.search(r"^\s*(from|import)\s+oracle\b|vfi_oracle|libvfi_oracle", text, flags=re.M):
                    offenders.append(os.path.join(dirpath, f))
    assert not offenders, offenders


def test_synthetic_inputs_and_padding():
    import torch
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import synthetic as S
    assert S.padded_size(1080, 1920) == (1152, 1984)
    assert S.padded_size(480, 640) == (512, 704)
    assert S.padded_size(256, 448) == (320, 512)          # 256 is a multiple of 128 -> +64
    assert S.padded_size(2160, 3840) == (2176, 3904)
    a = S.flow(1, 64, 96, 4.0, S.generator(), "smooth")
    b = S.flow(1, 64, 96, 4.0, S.generator(), "smooth")
    assert torch.equal(a, b) and a.shape == (1, 2, 64, 96) and a.is_contiguous()
    q = S.flow(1, 64, 96, 4.0, S.generator(), "quarter")
    assert (q[:, :, :, 1:] - q[:, :, :, :-1]).abs().mean() > (a[:, :, :, 1:] - a[:, :, :, :-1]).abs().mean()
    d = S.depth_weight(1, 8, 8, S.generator())
    assert float(d.min()) >= 0.1 and float(d.max()) <= 1.0
    shapes = [tuple(f1.shape) for f1, _ in S.correlation_features(1, 512, 704, S.generator())]
    assert shapes == [(1, 196, 8, 11), (1, 128, 16, 22), (1, 96, 32, 44), (1, 64, 64, 88), (1, 32, 128, 176)]


def test_shard_pairs_partition():
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd.runner import shard_pairs
    for n in (0, 1, 7, 64, 65):
        for world in (1, 2, 3, 8):
            parts = [list(shard_pairs(n, r, world)) for r in range(world)]
            assert sorted(sum(parts, [])) == list(range(n))
            assert max(map(len, parts)) - min(map(len, parts)) <= 1
    with pytest.raises(ValueError):
        shard_pairs(4, 2, 2)


_WORKER = r'''
import os, sys, json
sys.path.insert(0, %(root)r)
import torch, torch.distributed as dist
import vfidkr_amd
from vfidkr_amd import runner
rank, local_rank, world = runner.init_distributed("gloo")
mine = list(runner.shard_pairs(13, rank, world))
import time
t = runner.timed_region(lambda i: time.sleep(0.01 * (rank + 1)), 3)
total = runner.total_units(len(mine))
gathered = [None] * world
dist.all_gather_object(gathered, mine)
if rank == 0:
    print(json.dumps({"t": t, "total": total, "parts": gathered}))
dist.destroy_process_group()
'''


def test_two_rank_gloo_sharding(tmp_path):
    """world_size 2 on CPU: the partition is complete and the timing join is MAX over ranks."""
    import json
    import socket
    script = tmp_path / "worker.py"
    script.write_text(_WORKER % {"root": ROOT})
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=240) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-2000:] for o in outs]
    res = json.loads(outs[0][0].strip().splitlines()[-1])
    assert res["total"] == 13.0
    assert sorted(res["parts"][0] + res["parts"][1]) == list(range(13))
    assert res["t"] >= 3 * 0.02 * 0.9            # rank 1 sleeps 0.02 s per step: MAX, not rank 0's 0.03 s


def test_same_strides_ignores_size_one_dimensions():
    """torch leaves the stride of a size-1 dimension arbitrary (a B = 1 channel slice keeps the wide tensor's batch stride
    and still counts as contiguous): the glue entry points compare layouts without it."""
    import torch
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi
    wide = torch.zeros(1, 7, 4, 6)
    sl, dense = wide[:, 2:5], torch.zeros(1, 3, 4, 6)
    assert sl.is_contiguous() and sl.stride(0) != dense.stride(0)
    assert cabi._same_strides(sl, dense)
    assert not cabi._same_strides(torch.zeros(2, 7, 4, 6)[:, 2:5], torch.zeros(2, 3, 4, 6))
    assert not cabi._same_strides(dense, torch.zeros(1, 3, 4, 5))


def test_bench_launcher_starts_its_own_ranks():
    """`bench.py --gpus 2` with no RANK in the environment starts two ranks itself (gloo timing join) and prints ONE
    JSON line whose n_gpus is the number of ranks that ran; --stub-step replaces the GPU step by a sleep."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "0",
                        "--stub-step", "0.02"], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["steps"] == 3 and res["data"] == "stub"
    assert res["ms_per_step"] >= 20.0 * 0.9


def test_bench_runs_as_ranks_under_torch_distributed_run():
    """the driver's N > 1 command: `python -m torch.distributed.run --nproc-per-node 2 ... bench.py --gpus 2` -- bench.py
    finds RANK / WORLD_SIZE in the environment, does not start ranks of its own, and rank 0 prints the one JSON line."""
    import json
    from vfidkr_amd import runner
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(runner.free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2",
                        "--steps", "3", "--warmup", "1", "--stub-step", "0.02"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] >= 20.0 * 0.9


def test_bench_launcher_fails_cleanly_without_gpus():
    """on a box with fewer GPUs than --gpus the parent says so and exits non-zero before starting anything;
    a rank that dies makes the parent exit non-zero too."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("this box has the GPUs")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode != 0 and "GPU(s) visible" in r.stderr and not r.stdout.strip()
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import runner
    rc = runner.spawn_ranks(["-c", "import os, sys; sys.exit(3 if os.environ['RANK'] == '1' else 0)"], 2, timeout=60)
    assert rc == 3


# ------------------------------------------------------------------ a compiler hazard of the LDS-DMA pipelines

def test_no_register_spills_inside_the_counted_vmcnt_pipelines(built):
    """The LDS-staged kernels wait for a staged window with a hand-counted `s_waitcnt vmcnt(N)`: N = the LDS-DMA
    loads issued after it.  A register spill or reload (scratch_store / scratch_load: vector-memory operations in the
    same in-order counter) inside such a pipeline makes every counted wait stricter than written and a reload drains
    the counter altogether -- the ring would silently run one window deep.  The committed build has its few spills in the direct-gather fallback loops only; this test
    reads the device assembly the Makefile leaves beside the objects and keeps it that way: no scratch operation in
    any basic block that issues LDS-DMA loads, nor in any block of a loop that does."""
    import re
    checked = 0
    for name in ("filterinterp_lds.s", "filterinterp_lds_n.s", "filterinterp_multi.s", "filterinterp_defor_lds.s", "filterinterp_f16.s"):
        path = os.path.join(PKG, "lib", name)
        assert os.path.exists(path), path
        blocks, cur, func, in_asm = [], None, "", False
        for line in open(path):
            m = re.match(r"^(\.LBB\d+_\d+):(.*)$", line)
            if m:
                hdr = re.search(r"Header[:=]\s*(BB\d+_\d+)", m.group(2))
                cur = {"label": m.group(1)[2:], "loop": hdr.group(1) if hdr else None, "ins": [], "asm": [],
                       "is_header": "Loop Header" in m.group(2), "func": func}
                blocks.append(cur)
            elif re.match(r"^_Z\w+:", line):
                cur = None                                   # a new function: forget the block
                func = line.split(":")[0]
            elif ";;#ASMSTART" in line:
                in_asm = True
            elif ";;#ASMEND" in line:
                in_asm = False
            elif cur is not None and re.match(r"^\s+[a-z]", line):
                cur["ins"].append(line.strip())
                if in_asm:
                    cur["asm"].append(line.strip())
        for b in blocks:
            if b["is_header"]:
                b["loop"] = b["label"]
        for b in blocks:
            # what follows the branch back to the loop's header in the same text block is the loop's exit path (an
            # unlabelled fall-through block), not the loop
            if b["loop"]:
                for k, i in enumerate(b["ins"]):
                    if re.match(r"s_c?branch\w*\s+\.L" + re.escape(b["loop"]) + r"\b", i):
                        b["ins"] = b["ins"][:k + 1]
                        break
        is_dma = lambda i: i.startswith("buffer_load") and " lds" in i      # noqa: E731
        dma_loops = {b["loop"] for b in blocks if b["loop"] and any(is_dma(i) for i in b["ins"])}
        # a loop whose every hand-written vmcnt wait (the asm statements of the pipeline; the compiler's own waits for the
        # prologue's loads do not pace the ring) is vmcnt(0) keeps nothing in flight across its waits (the two-slot rings of
        # the largest windows): a reload cannot make those waits any stricter
        counted = set()
        for b in blocks:
            for i in b["asm"]:
                m = re.match(r"s_waitcnt vmcnt\((\d+)\)", i)
                if m and int(m.group(1)) > 0 and b["loop"]:
                    counted.add(b["loop"])
        for b in blocks:
            # (the multi-flow kernel keeps 2 x 2 pixel states: its straight-line prologue, which also issues the first
            #  windows, spills a few registers once per tile; what must stay clean there is the channel loop)
            prologue_ok = name == "filterinterp_multi.s"
            if "fi_forward_ori_ldsILb1E" in b["func"]:
                continue            # the blend-epilogue instance runs 3-channel frames only: its ring is never deeper than that
            pipelined = (any(is_dma(i) for i in b["ins"]) and not prologue_ok) or (b["loop"] in dma_loops)
            if not pipelined or (b["loop"] in dma_loops and b["loop"] not in counted):
                continue
            # a straight-line block that stages windows and then waits for EVERYTHING (hand-written vmcnt(0) only: the prologue
            # of a two-slot ring) cannot be hurt by a spill either
            own = [re.match(r"s_waitcnt vmcnt\((\d+)\)", i) for i in b["asm"]]
            own = [int(m.group(1)) for m in own if m]
            if b["loop"] is None and own and max(own) == 0:
                continue
            checked += 1
            ins = b["ins"]
            if b["loop"] is None:
                # (straight-line code: a spill OLDER than the block's first staging load retires before it -- vector-memory
                #  operations complete in issue order -- and leaves every counted wait as written)
                first = next(k for k, i in enumerate(ins) if is_dma(i))
                ins = ins[first:]
            spills = [i for i in ins if i.startswith("scratch_")]
            assert not spills, "%s %s: %d scratch operations inside an LDS-DMA pipeline: %s" % (
                name, b["label"], len(spills), spills[:3])
    assert checked >= 60                    # every K instantiation of every staged kernel was looked at


def test_row_of_staged_element_division_is_exact():
    """csrc/filterinterp_dev.h: fi_row_of() finds the window row of a staged element as (int)((e + 0.5f) * (1.0f / pitch)) --
    the staged kernels' LDS layout and DMA addresses depend on it being floor(e / pitch) for every pitch they can choose
    (any positive value since the fp16 kernel's pitch is 32k + 16) and every element index below 2^15.  Checked
    exhaustively in IEEE float32, also with a reciprocal that is one ulp off in either direction."""
    import numpy as np
    e = np.arange(0, 1 << 15, dtype=np.int32)
    ef = e.astype(np.float32) + np.float32(0.5)
    for pitch in range(1, 8193):
        exact = np.float32(1.0) / np.float32(pitch)
        for inv in (exact, np.nextafter(exact, np.float32(0.0)), np.nextafter(exact, np.float32(2.0))):
            assert np.array_equal((ef * inv).astype(np.int32), e // pitch), pitch
