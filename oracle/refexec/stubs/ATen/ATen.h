#include "cuda_cpu_shim.h" /* stub: everything the reference kernels need from this header is in the shim */
