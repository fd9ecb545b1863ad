"""A few channels_last context warps at padded 1080p (C = 196, smooth flow, three offsets) and the NCHW call beside them, for a
profiler to look at (kernel names: fi_forward_nhwc4 against the NCHW kernels):  python tools/prof_fi_nhwc.py [bfloat16|float32]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vfidkr_amd  # noqa: E402,F401
from tools.bench_fi_nhwc import variants  # noqa: E402

dtype = getattr(torch, sys.argv[1] if len(sys.argv) > 1 else "bfloat16")
fns = variants("1080p", 1, 1152, 1984, (0.25, 0.5, 0.75), dtype, "smooth")
for _ in range(3):
    fns["nhwc"]()
    fns["nchw"]()
torch.cuda.synchronize()
