// Micro-benchmark: chip-wide rate of no-return 64-bit INTEGER atomic adds to global memory (what the mesh export's accumulation issues,
// csrc/mesh.hip), next to no-return f32 atomic adds measured by the same program on the same box.  One adder per address per pass,
// consecutive lanes on consecutive elements, several footprints.  Prints one JSON line.
// Build: hipcc -O2 --offload-arch=gfx950 -munsafe-fp-atomics atomic_u64_rate.hip -o atomic_u64_rate ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include <algorithm>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e)); return 1; } } while (0)

template <typename T>
__global__ void __launch_bounds__(256) add_kernel(T* p, size_t n, int passes)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (int k = 0; k < passes; k++)
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) atomicAdd(&p[i], (T)1);
}

template <typename T>
static int measure(size_t bytes, int passes, double* gbs)
{
    T* d; const size_t n = bytes / sizeof(T);
    CK(hipMalloc(&d, bytes)); CK(hipMemset(d, 0, bytes));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int blocks = 256 * 8;
    hipLaunchKernelGGL(add_kernel<T>, dim3(blocks), dim3(256), 0, 0, d, n, 1);   // warm-up
    CK(hipDeviceSynchronize());
    std::vector<double> r;
    for (int rep = 0; rep < 5; rep++) {
        CK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(add_kernel<T>, dim3(blocks), dim3(256), 0, 0, d, n, passes);
        CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
        float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
        r.push_back((double)bytes * passes / (ms * 1e-3) / 1e9);
    }
    std::sort(r.begin(), r.end());
    *gbs = r[2];
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1)); CK(hipFree(d));
    return 0;
}

int main()
{
    const size_t mib[3] = {64, 512, 2048};
    printf("{\"metric\": \"global_atomic_add_GBps\", \"adders_per_address\": 1, \"median_of\": 5");
    for (int k = 0; k < 3; k++) {
        double u64 = 0, f32 = 0;
        const int passes = k == 0 ? 32 : (k == 1 ? 8 : 2);
        if (measure<unsigned long long>(mib[k] << 20, passes, &u64)) return 1;
        if (measure<float>(mib[k] << 20, passes, &f32)) return 1;
        printf(", \"u64_%zuMiB\": %.1f, \"f32_%zuMiB\": %.1f", mib[k], u64, mib[k], f32);
    }
    printf("}\n");
    return 0;
}
