"""The child process of tests/test_binding_refusals_host.py's sweep of the C ABI's own refusals (not a test module).

For every entry of cabi.SIGNATURES with tensor arguments, a base argument list is made from the header's parameter names:
dummy pointers that address nothing, small positive dimensions, plausible strides.  The base call itself is never made.  One
argument is then changed per call -- each pointer NULL (those the header documents as optional apart), each slot of a pointer
table NULL, each dimension 0 and -1 -- and the entry has to answer VFI_ERR_SHAPE.

The dummy pointers must never reach a kernel, so before the first call the HIP runtime is asked for its device count (through
ctypes; the parent hides every device): if it is not 0 the child leaves with that message and makes no call.
"""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DUMMY = 1 << 20                 # never dereferenced on the device: no device is visible
BASE_INTS = dict(batch=1, channel=3, channels=3, h=8, w=8, hq=2, wq=2, nflows=2, nitems=2, nd=2, cd=3, ci=3, filter_channels=16,
                 filter_size=4, pad_size=4, kernel_size=1, max_displacement=4, stride1=1, stride2=1, fillhole=1, align_corners=1,
                 variant=0, flow_is_bf16=0, neg_psnr=1, pad_left=1, pad_right=1, pad_top=1, pad_bottom=1, top=0, left=0, n=64)
HOST_FLOAT_ARRAYS = {"mul1"}    # host arrays of factors, read by the entry itself


def device_count():
    import torch  # noqa: F401  (binds libamdhip64 as the library will)
    hip = None
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
        try:
            hip = ctypes.CDLL(name)
            break
        except OSError:
            continue
    if hip is None:
        return None
    count = ctypes.c_int(-1)
    hip.hipGetDeviceCount(ctypes.byref(count))
    return count.value


def main():
    count = device_count()
    if count != 0:
        print("the HIP runtime reports %r devices: no call made (dummy pointers must never reach a kernel)" % (count,))
        return 2
    import vfidkr_amd  # noqa: F401
    from vfidkr_amd import cabi
    from tests.test_binding_refusals_host import DIMENSIONS, NOT_SWEPT, OPTIONAL_POINTERS, header_parameters
    lib = cabi.lib()
    keep = []                   # the host arrays stay alive
    entries = calls = 0
    bad = []
    for name, argtypes in cabi.SIGNATURES.items():
        if name in NOT_SWEPT:
            continue
        entries += 1
        params = header_parameters(name)
        base, kinds = [], []
        for p, ty in zip(params, argtypes):
            pname = re.search(r"(\w+)$", p).group(1)
            ptype = p[:-len(pname)].strip()
            if "* const*" in ptype or "*const*" in ptype:
                table = (ctypes.c_void_p * 8)(*([DUMMY] * 8))
                keep.append(table)
                base.append(table), kinds.append(("table", pname))
            elif pname in HOST_FLOAT_ARRAYS and "*" in ptype:
                arr = (ctypes.c_float * 8)(*([1.0] * 8))
                keep.append(arr)
                base.append(ctypes.cast(arr, ctypes.c_void_p)), kinds.append(("pointer", pname))
            elif ptype == "vfi_stream_t":
                base.append(None), kinds.append(("stream", pname))
            elif "*" in ptype:
                base.append(ctypes.c_void_p(DUMMY)), kinds.append(("pointer", pname))
            elif ty is cabi.Strides:
                base.append(cabi.Strides(4096, 64, 8)), kinds.append(("strides", pname))
            elif ty is cabi.Strides4:
                base.append(cabi.Strides4(4096, 64, 8, 1)), kinds.append(("strides", pname))
            elif ty is cabi.StridesNhwc:
                base.append(cabi.StridesNhwc(4096, 64, 8)), kinds.append(("strides", pname))
            elif ty is ctypes.c_int or ty is ctypes.c_int64:
                base.append(BASE_INTS.get(pname, 8192)), kinds.append(("dimension" if pname in DIMENSIONS else "int", pname))
            elif ty is ctypes.c_uint:
                base.append(7), kinds.append(("int", pname))
            elif ty is ctypes.c_double:
                base.append(1e-6), kinds.append(("float", pname))
            else:
                assert ty is ctypes.c_float, (name, p)
                base.append(0.5), kinds.append(("float", pname))
        mutated = []
        for k, (kind, pname) in enumerate(kinds):
            if kind == "pointer" and pname not in OPTIONAL_POINTERS.get(name, ()):
                mutated.append(("%s NULL" % pname, k, None))
            elif kind == "table":
                if pname not in OPTIONAL_POINTERS.get(name, ()):
                    mutated.append(("%s NULL" % pname, k, None))
                    for slot in range(2):
                        hole = (ctypes.c_void_p * 8)(*([DUMMY] * 8))
                        hole[slot] = None
                        keep.append(hole)
                        mutated.append(("%s[%d] NULL" % (pname, slot), k, hole))
            elif kind == "dimension":
                if pname != "ci":           # (no image channels: a call without the flow pair)
                    mutated.append(("%s = 0" % pname, k, 0))
                mutated.append(("%s = -1" % pname, k, -1))
        fn = getattr(lib, name)
        for what, k, value in mutated:
            args = list(base)
            args[k] = value
            print("%s: %s" % (name, what), flush=True)
            calls += 1
            got = fn(*args)
            if got != cabi.VFI_ERR_SHAPE:
                bad.append("%s: %s -> %d" % (name, what, got))
                print("  NOT REFUSED: returned %d" % got, flush=True)
    for line in bad:
        print("not refused:", line)
    print("swept %d entries, %d calls, %d not refused" % (entries, calls, len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
