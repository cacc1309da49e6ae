// Issue cost of v_pk_fma_f32 against two v_fma_f32 in a kernel without MFMAs: 16 independent
// f32 accumulators per lane, advanced `iters` times by either 16 scalar FMAs or 8 packed ones
// (the same IEEE operation per component), at 1, 2 and 4 waves per SIMD.  Prints cycles per
// wave-instruction on one SIMD from the shader clock (s_memtime), so the figure does not depend
// on the clock state.  hipcc --offload-arch=gfx950 -O3 tools/probe/pk_fma.hip -o tools/probe/pk_fma
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

typedef float v2f __attribute__((ext_vector_type(2)));

template <bool PACKED>
__global__ __launch_bounds__(256) void k(float* out, unsigned long long* cyc, int iters, float m, float c) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    v2f a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = v2f{(float)i + j, (float)i - j};
    const v2f mm = {m, m}, cc = {c, c};
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (PACKED) {
                asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(a[j]) : "v"(mm), "v"(cc));
            } else {
                asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[j].x) : "v"(m), "v"(c));
                asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[j].y) : "v"(m), "v"(c));
            }
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += a[j].x + a[j].y;
    out[i] = s;
    if ((threadIdx.x & 63) == 0) cyc[i >> 6] = t1 - t0;
}

int main() {
    int cus = 0;
    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
    const int iters = 20000;
    for (int wps = 1; wps <= 4; wps *= 2) {       // waves per SIMD: `wps` workgroups of 4 waves per CU
        const int blocks = cus * wps, n = blocks * 256;
        float* out;
        unsigned long long* cyc;
        hipMalloc(&out, n * sizeof(float));
        hipMalloc(&cyc, (n / 64) * sizeof(unsigned long long));
        std::vector<unsigned long long> h(n / 64);
        for (int packed = 0; packed < 2; ++packed) {
            for (int rep = 0; rep < 2; ++rep) {   // the second launch is the one reported
                if (packed) hipLaunchKernelGGL(k<true>, dim3(blocks), dim3(256), 0, 0, out, cyc, iters, 0.999f, 0.5f);
                else hipLaunchKernelGGL(k<false>, dim3(blocks), dim3(256), 0, 0, out, cyc, iters, 0.999f, 0.5f);
                if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
            }
            hipMemcpy(h.data(), cyc, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
            double sum = 0;
            for (auto v : h) sum += (double)v;
            const double per_wave = sum / h.size();               // s_memtime ticks of one wave's loop
            const double insts = (double)iters * (packed ? 8 : 16);
            printf("waves/SIMD %d  %s: %.0f ticks per wave, %.3f ticks per instruction per wave, "
                   "%.3f per 16 component-FMAs per SIMD-wave-slot\n",
                   wps, packed ? "v_pk_fma_f32 x 8" : "v_fma_f32 x 16  ", per_wave, per_wave / insts,
                   per_wave / iters / wps);
        }
        hipFree(out);
        hipFree(cyc);
    }
    return 0;
}
