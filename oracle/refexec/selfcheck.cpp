/* Stand-alone runner of the reference wrappers, built with -fsanitize=address,undefined (build_ref.py --sanitize).
 * TEST INFRASTRUCTURE ONLY.
 *
 *     selfcheck_san DIR
 *
 * reads DIR/jobs.txt, written by ref_exec.dump_jobs():
 *     <number of jobs> <thread order: 0 blocks, 1 raster>
 *     per job:     <launcher name> <n ints> <ints...> <n tensors>
 *     per tensor:  <elements of the whole buffer> <offset of the tensor in it> <4 strides> <file name>
 * Every buffer is filled from its file, handed to the wrapper at its offset with its strides, and written back as
 * <file>.out.  It sits between two poisoned zones of 1 MiB (the allocator's own red zones are a few hundred bytes,
 * less than a row of a small frame), so a read or write of the reference outside a buffer -- that is, beyond the
 * canvas margin ref_exec.py chose -- ends the run with the sanitizer's report and a non-zero status.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#else
#define ASAN_POISON_MEMORY_REGION(p, n) ((void)(p), (void)(n))
#define ASAN_UNPOISON_MEMORY_REGION(p, n) ((void)(p), (void)(n))
#endif

static const size_t kZone = 1u << 20;   /* bytes, either side of every buffer */

typedef int (*entry_t)(const int *, float *const *, const int *const *);
extern "C" void vfi_ref_set_order(int raster);

#define LAUNCHERS(X) \
    X(FilterInterpolationLayer_gpu_forward_kernel_ori) X(FilterInterpolationLayer_gpu_backward_kernel_ori) \
    X(FilterInterpolationLayer_gpu_forward_kernel) X(FilterInterpolationLayer_gpu_backward_kernel) \
    X(FilterInterpolationLayer_gpu_forward_kernel_deforconv) X(FilterInterpolationLayer_gpu_backward_kernel_deforconv) \
    X(FilterInterpolationLayer_gpu_forward_kernel_nofilterwithdeforconv) \
    X(FilterInterpolationLayer_gpu_backward_kernel_nofilterwithdeforconv) \
    X(FlowProjection_gpu_forward_kernel) X(FlowProjection_gpu_backward_kernel) \
    X(DepthFlowProjection_gpu_forward_kernel) X(DepthFlowProjection_gpu_backward_kernel) \
    X(minDepthFlowProjection_gpu_forward_kernel) X(minDepthFlowProjection_gpu_backward_kernel) \
    X(InterpolationLayer_gpu_forward_kernel) X(InterpolationLayer_gpu_backward_kernel) \
    X(InterpolationChLayer_gpu_forward_kernel) X(InterpolationChLayer_gpu_backward_kernel) \
    X(SeparableConvLayer_gpu_forward_kernel) X(SeparableConvLayer_gpu_backward_kernel) \
    X(SeparableConvFlowLayer_gpu_forward_kernel) X(SeparableConvFlowLayer_gpu_backward_kernel) \
    X(correlation_forward_cuda_kernel) X(correlation_backward_cuda_kernel)

#define DECLARE(name) extern "C" int vfi_ref_##name(const int *, float *const *, const int *const *);
LAUNCHERS(DECLARE)
#define ROW(name) {#name, vfi_ref_##name},
static const struct { const char *name; entry_t fn; } kTable[] = {LAUNCHERS(ROW)};

static void die(const char *what, const std::string &arg) {
    fprintf(stderr, "selfcheck: %s %s\n", what, arg.c_str());
    exit(2);
}

int main(int argc, char **argv) {
    if (argc != 2) die("usage: selfcheck_san", "DIR");
    const std::string dir = argv[1];
    FILE *jf = fopen((dir + "/jobs.txt").c_str(), "r");
    if (!jf) die("cannot open", dir + "/jobs.txt");
    int njobs = 0, order = 0;
    if (fscanf(jf, "%d %d", &njobs, &order) != 2) die("bad header in", "jobs.txt");
    vfi_ref_set_order(order);
    for (int j = 0; j < njobs; ++j) {
        char name[128];
        int ni = 0, nt = 0;
        if (fscanf(jf, "%127s %d", name, &ni) != 2) die("bad job line in", "jobs.txt");
        std::vector<int> ia(ni);
        for (int i = 0; i < ni; ++i)
            if (fscanf(jf, "%d", &ia[i]) != 1) die("bad integer in job", name);
        if (fscanf(jf, "%d", &nt) != 1) die("bad tensor count in job", name);
        entry_t fn = nullptr;
        for (const auto &row : kTable)
            if (!strcmp(row.name, name)) fn = row.fn;
        if (!fn) die("unknown launcher", name);
        std::vector<float *> bufs(nt), ptrs(nt);
        std::vector<long> sizes(nt);
        std::vector<std::vector<int>> strides(nt, std::vector<int>(4));
        std::vector<const int *> sp(nt);
        std::vector<std::string> files(nt);
        for (int t = 0; t < nt; ++t) {
            long off = 0;
            char fnm[128];
            if (fscanf(jf, "%ld %ld %d %d %d %d %127s", &sizes[t], &off, &strides[t][0], &strides[t][1],
                       &strides[t][2], &strides[t][3], fnm) != 7)
                die("bad tensor line in job", name);
            files[t] = dir + "/" + fnm;
            const size_t bytes = sizeof(float) * (size_t)sizes[t];
            char *region = static_cast<char *>(malloc(bytes + 2 * kZone));
            if (!region) die("out of memory for", fnm);
            ASAN_POISON_MEMORY_REGION(region, kZone);
            ASAN_POISON_MEMORY_REGION(region + kZone + bytes, kZone);
            bufs[t] = reinterpret_cast<float *>(region + kZone);
            FILE *f = fopen(files[t].c_str(), "rb");
            if (!f || fread(bufs[t], sizeof(float), (size_t)sizes[t], f) != (size_t)sizes[t]) die("cannot read", files[t]);
            fclose(f);
            ptrs[t] = bufs[t] + off;
            sp[t] = strides[t].data();
        }
        const int err = fn(ia.data(), ptrs.data(), sp.data());
        if (err) die("launcher returned an error:", name);
        for (int t = 0; t < nt; ++t) {
            FILE *f = fopen((files[t] + ".out").c_str(), "wb");
            if (!f || fwrite(bufs[t], sizeof(float), (size_t)sizes[t], f) != (size_t)sizes[t]) die("cannot write", files[t]);
            fclose(f);
            char *region = reinterpret_cast<char *>(bufs[t]) - kZone;
            ASAN_UNPOISON_MEMORY_REGION(region, sizeof(float) * (size_t)sizes[t] + 2 * kZone);
            free(region);
        }
    }
    fclose(jf);
    printf("selfcheck: %d jobs clean\n", njobs);
    return 0;
}
