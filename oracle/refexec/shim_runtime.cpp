/* The shim's launch loops (see cuda_cpu_shim.h).  TEST INFRASTRUCTURE ONLY. */
#include "cuda_cpu_shim.h"

#include <ucontext.h>
#include <vector>

thread_local dim3 gridDim, blockIdx, blockDim, threadIdx;

static int g_order = 0;   /* 0: block-major, 1: whole-frame raster */

extern "C" void vfi_ref_set_order(int raster) { g_order = raster ? 1 : 0; }
extern "C" int vfi_ref_get_order() { return g_order; }

namespace vfi_shim {

void launch_serial(dim3 grid, dim3 block, const std::function<void()> &thread) {
    gridDim = grid;
    blockDim = block;
    if (g_order == 0) {
        for (unsigned bz = 0; bz < grid.z; ++bz)
            for (unsigned by = 0; by < grid.y; ++by)
                for (unsigned bx = 0; bx < grid.x; ++bx)
                    for (unsigned tz = 0; tz < block.z; ++tz)
                        for (unsigned ty = 0; ty < block.y; ++ty)
                            for (unsigned tx = 0; tx < block.x; ++tx) {
                                blockIdx = dim3(bx, by, bz);
                                threadIdx = dim3(tx, ty, tz);
                                thread();
                            }
    } else {
        for (unsigned z = 0; z < grid.z * block.z; ++z)
            for (unsigned y = 0; y < grid.y * block.y; ++y)
                for (unsigned x = 0; x < grid.x * block.x; ++x) {
                    blockIdx = dim3(x / block.x, y / block.y, z / block.z);
                    threadIdx = dim3(x % block.x, y % block.y, z % block.z);
                    thread();
                }
    }
}

/* ---- lock-step blocks: one coroutine per thread of the block, switched at every barrier ----
 * A lane starts on its own stack through makecontext / setcontext; later switches are _setjmp / _longjmp, which
 * make no system call (a block of the PWC configuration passes ~500 barriers with 32 lanes each).  A sanitized
 * build switches with swapcontext throughout, which AddressSanitizer follows. */
#if defined(__SANITIZE_ADDRESS__)
#define VFI_SHIM_JMP 0
#else
#define VFI_SHIM_JMP 1
#include <setjmp.h>
#endif

enum { MAX_LANES = 64, STACK_BYTES = 256 * 1024 };
static ucontext_t g_sched, g_ctx[MAX_LANES];
static bool g_done[MAX_LANES], g_started[MAX_LANES];
static int g_cur = -1;
static volatile int g_lane;                  /* scheduler state lives outside its frame: it is re-entered by longjmp */
static volatile bool g_live;
static unsigned g_round = 0;                 /* barriers passed so far in this block */
static float g_slot[2][MAX_LANES];
static const std::function<void()> *g_body = nullptr;
#if VFI_SHIM_JMP
static jmp_buf g_jsched, g_jctx[MAX_LANES];
#endif

static void to_scheduler() {
#if VFI_SHIM_JMP
    if (_setjmp(g_jctx[g_cur]) == 0) _longjmp(g_jsched, 1);
#else
    swapcontext(&g_ctx[g_cur], &g_sched);
#endif
}

static void lane_main() {
    (*g_body)();
    g_done[g_cur] = true;
    to_scheduler();
}

static void resume_lane(int i) {
#if VFI_SHIM_JMP
    if (_setjmp(g_jsched) == 0) {
        if (!g_started[i]) {
            g_started[i] = true;
            setcontext(&g_ctx[i]);
        }
        _longjmp(g_jctx[i], 1);
    }
#else
    g_started[i] = true;
    swapcontext(&g_sched, &g_ctx[i]);
#endif
}

void barrier() {
    if (g_cur < 0) return;                   /* serial launches have no barriers to honour */
    to_scheduler();
}

float shfl_down(float v, unsigned delta) {
    /* two buffers: a lane is at most one barrier ahead of the slowest one */
    const unsigned buf = g_round & 1u;
    const unsigned lane = threadIdx.x % warpSize, base = threadIdx.x - lane;
    g_slot[buf][threadIdx.x] = v;
    barrier();
    return lane + delta < (unsigned)warpSize ? g_slot[buf][base + lane + delta] : v;
}

void launch_lockstep(dim3 grid, dim3 block, const std::function<void()> &thread) {
    static int n;
    static unsigned bx, by, bz;
    n = (int)block.x;
    if (n > MAX_LANES || block.y != 1 || block.z != 1) {
        fprintf(stderr, "vfi_shim: lock-step blocks are 1-D with at most %d threads\n", (int)MAX_LANES);
        abort();
    }
    static std::vector<char> stacks;
    stacks.resize((size_t)n * STACK_BYTES);
    gridDim = grid;
    blockDim = block;
    g_body = &thread;
    for (bz = 0; bz < gridDim.z; ++bz)
        for (by = 0; by < gridDim.y; ++by)
            for (bx = 0; bx < gridDim.x; ++bx) {
                g_round = 0;
                for (int i = 0; i < n; ++i) {
                    getcontext(&g_ctx[i]);
                    g_ctx[i].uc_stack.ss_sp = stacks.data() + (size_t)i * STACK_BYTES;
                    g_ctx[i].uc_stack.ss_size = STACK_BYTES;
                    g_ctx[i].uc_link = nullptr;
                    makecontext(&g_ctx[i], lane_main, 0);
                    g_done[i] = g_started[i] = false;
                }
                for (g_live = true; g_live;) {
                    g_live = false;
                    for (g_lane = 0; g_lane < n; g_lane = g_lane + 1) {
                        if (g_done[g_lane]) continue;
                        g_cur = g_lane;
                        blockIdx = dim3(bx, by, bz);
                        threadIdx = dim3((unsigned)g_lane, 0, 0);
                        resume_lane(g_lane);
                        if (!g_done[g_lane]) g_live = true;
                    }
                    ++g_round;
                }
                g_cur = -1;
            }
    g_body = nullptr;
}

}  // namespace vfi_shim
