// v_fma_f64 and v_cvt_f64_f32 on gfx950: issue time of a dependent and of an independent chain, in clock64() ticks per
// wave instruction, beside v_fma_f32 as the yardstick (one wave, nothing else on the CU; run on the GPU box).
//   hipcc -O3 --offload-arch=gfx950 valu_f64_rate.hip -o valu_f64_rate
#include <hip/hip_runtime.h>
#include <stdio.h>

#define REP16(x) x x x x x x x x x x x x x x x x
constexpr int ITERS = 256, PER_ITER = 16;

// WHICH 0: v_fma_f32, 1: v_fma_f64, 2: v_cvt_f64_f32.  DEP: every instruction reads the result of the one before it;
// otherwise eight chains in turn.  The dependent conversion feeds the low word of its result back as the next input.
template <int WHICH, bool DEP>
__global__ void timing(double *out, long long *cyc) {
    float f[8];
    double d[8];
    for (int i = 0; i < 8; ++i) {
        f[i] = 1.0f + threadIdx.x * 0.001f + i;
        d[i] = 1.0 + threadIdx.x * 0.001 + i;
    }
    const float af = 0.999f, bf = 1e-3f;
    const double ad = 0.999, bd = 1e-3;
    const long long t0 = clock64();
    for (int it = 0; it < ITERS; ++it) {
        if constexpr (WHICH == 0 && DEP) {
            REP16(asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(f[0]) : "v"(af), "v"(bf));)
        } else if constexpr (WHICH == 0) {
            REP16(asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(f[0]) : "v"(af), "v"(bf));
                  asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(f[1]) : "v"(af), "v"(bf));
                  asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(f[2]) : "v"(af), "v"(bf));
                  asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(f[3]) : "v"(af), "v"(bf));
                  asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(f[4]) : "v"(af), "v"(bf));
                  asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(f[5]) : "v"(af), "v"(bf));
                  asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(f[6]) : "v"(af), "v"(bf));
                  asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(f[7]) : "v"(af), "v"(bf));)
        } else if constexpr (WHICH == 1 && DEP) {
            REP16(asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(d[0]) : "v"(ad), "v"(bd));)
        } else if constexpr (WHICH == 1) {
            REP16(asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(d[0]) : "v"(ad), "v"(bd));
                  asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(d[1]) : "v"(ad), "v"(bd));
                  asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(d[2]) : "v"(ad), "v"(bd));
                  asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(d[3]) : "v"(ad), "v"(bd));
                  asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(d[4]) : "v"(ad), "v"(bd));
                  asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(d[5]) : "v"(ad), "v"(bd));
                  asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(d[6]) : "v"(ad), "v"(bd));
                  asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(d[7]) : "v"(ad), "v"(bd));)
        } else if constexpr (DEP) {
            REP16(asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d[0]) : "v"(f[0]));
                  f[0] = __int_as_float(__double2loint(d[0]));)
        } else {
            REP16(asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d[0]) : "v"(f[0]));
                  asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d[1]) : "v"(f[1]));
                  asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d[2]) : "v"(f[2]));
                  asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d[3]) : "v"(f[3]));
                  asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d[4]) : "v"(f[4]));
                  asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d[5]) : "v"(f[5]));
                  asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d[6]) : "v"(f[6]));
                  asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d[7]) : "v"(f[7]));)
        }
    }
    const long long t1 = clock64();
    double s = 0.0;
    for (int i = 0; i < 8; ++i) s += d[i] + (double)f[i];
    out[threadIdx.x] = s;
    if (threadIdx.x == 0) cyc[0] = t1 - t0;
}

template <int WHICH, bool DEP>
static void run(const char *name, double *d, long long *dc) {
    long long hc = 0;
    for (int rep = 0; rep < 3; ++rep) {   // the last of three launches is reported
        hipLaunchKernelGGL((timing<WHICH, DEP>), dim3(1), dim3(64), 0, 0, d, dc);
        if (hipMemcpy(&hc, dc, 8, hipMemcpyDeviceToHost) != hipSuccess) hc = -1;
    }
    const int n = ITERS * PER_ITER * (DEP ? 1 : 8);
    printf("%-34s %7.2f ticks per wave instruction (%d instructions)\n", name, (double)hc / n, n);
}

int main() {
    double *d;
    long long *dc;
    if (hipMalloc(&d, 64 * 8) != hipSuccess || hipMalloc(&dc, 8) != hipSuccess) return 1;
    run<0, true>("v_fma_f32 dependent", d, dc);
    run<0, false>("v_fma_f32 8 chains", d, dc);
    run<1, true>("v_fma_f64 dependent", d, dc);
    run<1, false>("v_fma_f64 8 chains", d, dc);
    run<2, true>("v_cvt_f64_f32 dependent", d, dc);
    run<2, false>("v_cvt_f64_f32 8 independent", d, dc);
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
