"""CPU oracle for the frame-synthesis hot path -- TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import
this package, and only as the checker.  See vfi_oracle.h for the parity status
(pinned to the reference's own kernels run on the CPU by oracle/refexec, and by
analytic cases + np_oracle).
"""
