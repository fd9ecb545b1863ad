/* CUDA-on-CPU shim: just enough of the CUDA and ATen surface for the reference's one-thread-per-pixel
 * kernel files (and its correlation file) to compile with plain g++ and run on the host.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing here is derived from the reference; the reference's own text is read at
 * build time by build_ref.py, which only rewrites `kernel<<<grid, block, 0, stream>>>(args);` into
 * `VFI_LAUNCH(grid, block, 0, stream, kernel, args);`.
 *
 * Standard headers come first: the reference files define `min` / `max` macros right after their includes.
 */
#ifndef VFI_CUDA_CPU_SHIM_H
#define VFI_CUDA_CPU_SHIM_H

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <math.h>
#include <stdio.h>

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
extern thread_local dim3 gridDim, blockIdx, blockDim, threadIdx;
static const int warpSize = 32;

/* internal linkage: the reference files reuse kernel names, and template instantiations with one mangled name
 * would otherwise be merged across translation units by the linker */
#define __global__ static
#define __device__ static
#define __forceinline__ inline
#define __shared__ static          /* one block runs at a time (see launch_lockstep) */
#define __restrict__

typedef void *cudaStream_t;
typedef int cudaError_t;
enum { cudaSuccess = 0 };
static inline cudaError_t cudaGetLastError() { return cudaSuccess; }
static inline const char *cudaGetErrorString(cudaError_t) { return "no error"; }

/* the host runs one thread at a time: a serial read-modify-write is the atomic */
static inline float atomicAdd(float *p, float v) { float old = *p; *p = old + v; return old; }
static inline int atomicAdd(int *p, int v) { int old = *p; *p = old + v; return old; }

/* CUDA's integer min / max builtins (the correlation file uses them; the other files define macros later) */
static inline int max(int a, int b) { return a > b ? a : b; }
static inline int min(int a, int b) { return a < b ? a : b; }

namespace at {
struct Half {};
struct Tensor {
    void *ptr;
    int type() const { return 0; }
    template <typename T> T *data() const { return static_cast<T *>(ptr); }
};
}  // namespace at

/* float only: the at::Half dispatch of the correlation file is out of scope */
#define AT_DISPATCH_FLOATING_TYPES(TYPE, NAME, ...) { using scalar_t = float; (void)(TYPE); __VA_ARGS__(); }
#define AT_DISPATCH_FLOATING_TYPES_AND_HALF(TYPE, NAME, ...) AT_DISPATCH_FLOATING_TYPES(TYPE, NAME, __VA_ARGS__)

namespace vfi_shim {
/* Runs `thread` once per CUDA thread of the launch, serially.  Order 0: CUDA's numbering, block-major
 * (blockIdx.z, .y, .x outermost, then threadIdx.z, .y, .x).  Order 1: raster order over the whole frame
 * (z = batch, then the global y, then the global x), the order a sequential CPU loop would take. */
void launch_serial(dim3 grid, dim3 block, const std::function<void()> &thread);
/* Runs the blocks one after another and each block's threads (blockDim.x <= 64, 1-D) as coroutines that switch
 * at every barrier(): all threads reach a barrier before any goes past it, as on the device. */
void launch_lockstep(dim3 grid, dim3 block, const std::function<void()> &thread);
void barrier();
float shfl_down(float v, unsigned delta);
}  // namespace vfi_shim

static inline void __syncthreads() { vfi_shim::barrier(); }
static inline void __syncwarp(unsigned = 0xffffffffu) { vfi_shim::barrier(); }
static inline float __shfl_down_sync(unsigned, float v, unsigned delta) { return vfi_shim::shfl_down(v, delta); }

#ifdef VFI_SHIM_LOCKSTEP
#define VFI_LAUNCH_FN vfi_shim::launch_lockstep
#else
#define VFI_LAUNCH_FN vfi_shim::launch_serial
#endif
#define VFI_LAUNCH(grid, block, shmem, stream, kernel, ...) \
    VFI_LAUNCH_FN((grid), (block), [&]() { kernel(__VA_ARGS__); })

#endif
