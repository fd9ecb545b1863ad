"""Build oracle/_ref/libvfi_ref.so: the reference's own kernel files, run on the CPU.

TEST INFRASTRUCTURE ONLY.  The reference checkout is found through the environment variable VFI_REFERENCE
(default /root/reference).  Each `*_cuda_kernel.cu` is read, its kernel launches

    name<<<grid, block, 0, stream>>>(args);          (also  name<scalar_t><<<...>>> (args);)

are rewritten into `VFI_LAUNCH(grid, block, 0, stream, name, args);` -- the only edit besides dropping the
`static` in front of `__shared__`, which the shim already spells `static` -- and the result is written to
oracle/_ref/src/ and compiled, one translation unit per file, against cuda_cpu_shim.h and the stub headers.
Everything this reads from the reference or makes from it stays under oracle/_ref/, which git ignores.

    python -m oracle.refexec.build_ref [--force] [--sanitize]
"""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF_OUT = os.path.join(os.path.dirname(HERE), "_ref")
SO = os.path.join(REF_OUT, "libvfi_ref.so")
SELFCHECK = os.path.join(REF_OUT, "selfcheck_san")

# (directory below the checkout, kernel file, needs lock-step blocks)
KERNEL_FILES = [
    ("my_package/FilterInterpolation", "filterinterpolation_cuda_kernel.cu", False),
    ("my_package/FlowProjection", "flowprojection_cuda_kernel.cu", False),
    ("my_package/DepthFlowProjection", "depthflowprojection_cuda_kernel.cu", False),
    ("my_package/MinDepthFlowProjection", "mindepthflowprojection_cuda_kernel.cu", False),
    ("my_package/Interpolation", "interpolation_cuda_kernel.cu", False),
    ("my_package/InterpolationCh", "interpolationch_cuda_kernel.cu", False),
    ("my_package/SeparableConv", "separableconv_cuda_kernel.cu", False),
    ("my_package/SeparableConvFlow", "separableconvflow_cuda_kernel.cu", False),
    ("PWCNet/correlation_package_pytorch1_0", "correlation_cuda_kernel.cu", True),
]

CXXFLAGS = ["-O2", "-fPIC", "-U_FORTIFY_SOURCE", "-ffp-contract=off", "-fno-fast-math", "-std=c++14", "-w"]
SANFLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
            "-ffp-contract=off", "-fno-fast-math", "-std=c++14", "-w"]

_LAUNCH = re.compile(r"([A-Za-z_]\w*(?:\s*<\s*\w+\s*>)?)\s*<<<([^<>]*?)>>>\s*\(")


def reference_root():
    return os.environ.get("VFI_REFERENCE", "/root/reference")


def reference_present():
    root = reference_root()
    return all(os.path.isfile(os.path.join(root, d, f)) for d, f, _ in KERNEL_FILES)


def rewrite_launches(text):
    """`k<<<cfg>>>(args)` -> `VFI_LAUNCH(cfg, k, args)`.  Commented-out launches are rewritten too; harmless."""
    out, pos, count = [], 0, 0
    for m in _LAUNCH.finditer(text):
        if m.start() < pos:
            continue
        depth, i = 1, m.end()
        while depth:
            c = text[i]
            depth += (c == "(") - (c == ")")
            i += 1
        cfg = [s.strip() for s in m.group(2).split(",")]
        if len(cfg) != 4:
            raise RuntimeError("launch configuration with %d entries: %r" % (len(cfg), m.group(0)))
        args = text[m.end():i - 1]
        out.append(text[pos:m.start()])
        out.append("VFI_LAUNCH(%s, %s, %s)" % (", ".join(cfg), re.sub(r"\s+", "", m.group(1)), args))
        pos = i
        count += 1
    out.append(text[pos:])
    return "".join(out).replace("static __shared__", "__shared__"), count


def _newer(target, sources):
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(s) <= t for s in sources)


def _own_sources():
    names = ["cuda_cpu_shim.h", "shim_runtime.cpp", "ref_entry.cpp", "selfcheck.cpp", "build_ref.py"]
    return [os.path.join(HERE, n) for n in names]


def build(force=False, sanitize=False, verbose=False):
    """Returns the path of the library (or of the sanitized stand-alone program), or None without a checkout."""
    if not reference_present():
        return None
    root = reference_root()
    target = SELFCHECK if sanitize else SO
    refs = [os.path.join(root, d, f) for d, f, _ in KERNEL_FILES]
    if not force and _newer(target, refs + _own_sources()):
        return target
    src = os.path.join(REF_OUT, "src")
    objdir = os.path.join(REF_OUT, "obj_san" if sanitize else "obj")
    os.makedirs(src, exist_ok=True)
    os.makedirs(objdir, exist_ok=True)
    flags = SANFLAGS if sanitize else CXXFLAGS
    inc = ["-I", HERE, "-I", os.path.join(HERE, "stubs"), "-include", os.path.join(HERE, "cuda_cpu_shim.h")]
    objs, jobs = [], []
    for d, f, lockstep in KERNEL_FILES:
        with open(os.path.join(root, d, f), errors="replace") as fh:
            text, n = rewrite_launches(fh.read())
        if n == 0:
            raise RuntimeError("no kernel launch found in " + f)
        cpp = os.path.join(src, f[:-3] + ".cpp")
        with open(cpp, "w") as fh:
            fh.write(text)
        obj = os.path.join(objdir, f[:-3] + ".o")
        cmd = ["g++"] + flags + inc + ["-I", os.path.join(root, d)] + (["-DVFI_SHIM_LOCKSTEP"] if lockstep else []) \
            + ["-c", cpp, "-o", obj]
        jobs.append((cmd, subprocess.Popen(cmd)))
        objs.append(obj)
    own = ["shim_runtime.cpp", "ref_entry.cpp"] + (["selfcheck.cpp"] if sanitize else [])
    for name in own:
        obj = os.path.join(objdir, name[:-4] + ".o")
        cmd = ["g++"] + flags + inc + sum((["-I", os.path.join(root, d)] for d, _, _ in KERNEL_FILES), []) \
            + ["-c", os.path.join(HERE, name), "-o", obj]
        jobs.append((cmd, subprocess.Popen(cmd)))
        objs.append(obj)
    for cmd, p in jobs:
        if p.wait() != 0:
            raise RuntimeError("failed: " + " ".join(cmd))
    link = ["g++"] + (["-fsanitize=address,undefined"] if sanitize else ["-shared"]) + objs + ["-o", target]
    if verbose:
        print(" ".join(link))
    subprocess.check_call(link)
    return target


if __name__ == "__main__":
    path = build(force="--force" in sys.argv, sanitize="--sanitize" in sys.argv, verbose=True)
    print(path if path else "no reference checkout at %s: nothing built" % reference_root())
