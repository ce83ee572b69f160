// Microbenchmark: SIMD cycles per FP64 VALU instruction on gfx950 with the SIMD saturated -- what v_add_f64 and
// v_max_f64 (the whole arithmetic of the f64 row sweep, dcp_f64.hip) cost per issue, beside v_add_f32 / v_max_f32
// measured the same way.  The f64 kernel's roofline is cells x (adds + maxes per cell) x this cost.
// Not part of the product.
//   hipcc --offload-arch=gfx950 -O3 -w f64_issue.hip -o f64_issue && ./f64_issue
// Method (valu_issue.hip's): every lane runs `iters` x 64 independent instructions (16 accumulators, each depending
// only on the result 16 instructions back); one block of 256 x W threads per CU = W wavefronts per SIMD.
// Cycles = the block's span in shader clocks (s_memtime), first wavefront's start to last one's end (the oldest
// wavefront is issued first and finishes early), / (iters x 64 x W): clocks per wavefront-instruction per SIMD.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>

#define BODY64(ASM)                                                                                          \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) _Pragma("unroll") for (int i = 0; i < 16; ++i)             \
        asm volatile(ASM : "+v"(a[i]) : "v"(b));

template <int OP> __global__ __launch_bounds__(1024) void f64_kernel(double *out, int iters, double s0, ulonglong2 *clk)
{
    double a[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
        a[i] = threadIdx.x * 1e-3 + i;
    double const b = s0 * (1.0 + (threadIdx.x & 63) * 1e-3);
    unsigned long long const t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it)
    {
        if constexpr (OP == 0) { BODY64("v_add_f64 %0, %0, %1") }
        else { BODY64("v_max_f64 %0, %0, %1") }
    }
    unsigned long long const t1 = __builtin_amdgcn_s_memtime();
    double acc = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        acc += a[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
    if ((threadIdx.x & 63) == 0) clk[blockIdx.x * 16 + (threadIdx.x >> 6)] = ulonglong2{t0, t1};
}

template <int OP> __global__ __launch_bounds__(1024) void f32_kernel(double *out, int iters, double s0, ulonglong2 *clk)
{
    float a[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
        a[i] = threadIdx.x * 1e-3f + i;
    float const b = (float)s0 * (1.0f + (threadIdx.x & 63) * 1e-3f);
    unsigned long long const t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it)
    {
        if constexpr (OP == 0) { BODY64("v_add_f32 %0, %0, %1") }
        else { BODY64("v_max_f32 %0, %0, %1") }
    }
    unsigned long long const t1 = __builtin_amdgcn_s_memtime();
    float acc = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        acc += a[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
    if ((threadIdx.x & 63) == 0) clk[blockIdx.x * 16 + (threadIdx.x >> 6)] = ulonglong2{t0, t1};
}

typedef void (*Kern)(double *, int, double, ulonglong2 *);

int main()
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 1;
    int const ncu = prop.multiProcessorCount, iters = 4096;
    double *out;
    ulonglong2 *clk;
    if (hipMalloc(&out, sizeof(double) * ncu * 1024) != hipSuccess || hipMalloc(&clk, sizeof(ulonglong2) * 16 * ncu) != hipSuccess)
        return 1;
    struct { char const *name; Kern k; } const ks[] = {{"v_add_f64", f64_kernel<0>}, {"v_max_f64", f64_kernel<1>},
                                                       {"v_add_f32", f32_kernel<0>}, {"v_max_f32", f32_kernel<1>}};
    for (auto const &k : ks)
        for (int W : {1, 2, 4})
        {
            hipLaunchKernelGGL(k.k, dim3(ncu), dim3(256 * W), 0, 0, out, iters, 1.0, clk); // warm-up
            hipLaunchKernelGGL(k.k, dim3(ncu), dim3(256 * W), 0, 0, out, iters, 1.0, clk);
            if (hipDeviceSynchronize() != hipSuccess) return 1;
            std::vector<ulonglong2> st((size_t)16 * ncu);
            if (hipMemcpy(st.data(), clk, sizeof(ulonglong2) * 16 * ncu, hipMemcpyDeviceToHost) != hipSuccess) return 1;
            std::vector<unsigned long long> c(ncu);
            for (int b = 0; b < ncu; ++b)
            {
                unsigned long long lo = ~0ull, hi = 0;
                for (int w = 0; w < 4 * W; ++w)
                    lo = std::min(lo, st[(size_t)b * 16 + w].x), hi = std::max(hi, st[(size_t)b * 16 + w].y);
                c[b] = hi - lo;
            }
            std::sort(c.begin(), c.end());
            // s_memtime counts the shader clock: clocks per wavefront-instruction per SIMD
            printf("%-10s W=%d  %.2f cycles / wavefront-instruction (median CU)\n", k.name, W,
                   (double)c[ncu / 2] / ((double)iters * 64.0 * W));
        }
    (void)hipFree(out);
    (void)hipFree(clk);
    return 0;
}
