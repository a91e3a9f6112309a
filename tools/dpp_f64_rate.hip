// Micro-benchmark: issue rate of the fused fp64 multiply-add with a DPP row broadcast operand (v_fmac_f64_dpp row_newbcast:n) on gfx950,
// against the plain v_fmac_f64 and against plain FMAs whose row operands arrive as 16-byte LDS broadcasts (the pattern of rank2 in
// csrc/mvmc_tri_w1.h: two ds_read_b128 feed four FMAs).
//   hipcc --offload-arch=gfx950 -O3 -o tools/bin/dpp_f64_rate tools/dpp_f64_rate.hip && tools/bin/dpp_f64_rate
// Every wave runs ITERS iterations over NACC independent accumulators (the rate, not the latency of one chain, is measured).  Workgroups
// of 256 threads put one wave on each SIMD of a CU; W workgroups per CU give W waves per SIMD, all four SIMDs busy, so that (c) shows the
// LDS pipe the CU's waves share.  The "1 SIMD" rows launch 64-thread workgroups, one per CU: one wave alone on the CU.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

constexpr int ITERS = 8192, NACC = 16;

#define ACC16 "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]), "+v"(acc[7]),          \
              "+v"(acc[8]), "+v"(acc[9]), "+v"(acc[10]), "+v"(acc[11]), "+v"(acc[12]), "+v"(acc[13]), "+v"(acc[14]), "+v"(acc[15])

// (a) 64 plain v_fmac_f64 per iteration: accumulator c <- v * t + accumulator c
#define PL(A, S, T) "v_fmac_f64_e32 %" #A ", %" #S ", %" #T "\n\t"
#define PL16(S, T) PL(0, S, T) PL(1, S, T) PL(2, S, T) PL(3, S, T) PL(4, S, T) PL(5, S, T) PL(6, S, T) PL(7, S, T)                       \
                   PL(8, S, T) PL(9, S, T) PL(10, S, T) PL(11, S, T) PL(12, S, T) PL(13, S, T) PL(14, S, T) PL(15, S, T)
__global__ void __launch_bounds__(256) k_plain(double* out, double a0, double b0) {
    double acc[NACC];
    for (int c = 0; c < NACC; ++c) acc[c] = c * 1e-3;
    double v0 = a0 + threadIdx.x * 1e-9, v1 = a0 - threadIdx.x * 1e-9, t0 = b0, t1 = -b0;
    for (int it = 0; it < ITERS; ++it)
        asm volatile(PL16(16, 18) PL16(17, 19) PL16(16, 19) PL16(17, 18) : ACC16 : "v"(v0), "v"(v1), "v"(t0), "v"(t1));
    double s = 0.0;
    for (int c = 0; c < NACC; ++c) s += acc[c];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// (b) the same 64 multiply-adds, the first factor taken from lane n of the reading lane's row of 16, n rotating over 0 .. 15
#define DP(A, S, T, N) "v_fmac_f64_dpp %" #A ", %" #S ", %" #T " row_newbcast:" #N " row_mask:0xf bank_mask:0xf\n\t"
#define DP16(S, T) DP(0, S, T, 0) DP(1, S, T, 1) DP(2, S, T, 2) DP(3, S, T, 3) DP(4, S, T, 4) DP(5, S, T, 5) DP(6, S, T, 6)              \
                   DP(7, S, T, 7) DP(8, S, T, 8) DP(9, S, T, 9) DP(10, S, T, 10) DP(11, S, T, 11) DP(12, S, T, 12) DP(13, S, T, 13)     \
                   DP(14, S, T, 14) DP(15, S, T, 15)
// (b'): as (b) with the broadcast factor negated (the rank-2 update's form)
#define DN(A, S, T, N) "v_fmac_f64_dpp %" #A ", -%" #S ", %" #T " row_newbcast:" #N " row_mask:0xf bank_mask:0xf\n\t"
#define DN16(S, T) DN(0, S, T, 0) DN(1, S, T, 1) DN(2, S, T, 2) DN(3, S, T, 3) DN(4, S, T, 4) DN(5, S, T, 5) DN(6, S, T, 6)              \
                   DN(7, S, T, 7) DN(8, S, T, 8) DN(9, S, T, 9) DN(10, S, T, 10) DN(11, S, T, 11) DN(12, S, T, 12) DN(13, S, T, 13)     \
                   DN(14, S, T, 14) DN(15, S, T, 15)
template <bool NEG>
__global__ void __launch_bounds__(256) k_dpp(double* out, double a0, double b0) {
    double acc[NACC];
    for (int c = 0; c < NACC; ++c) acc[c] = c * 1e-3;
    double v0 = a0 + threadIdx.x * 1e-9, v1 = a0 - threadIdx.x * 1e-9, t0 = b0, t1 = -b0;
    for (int it = 0; it < ITERS; ++it) {
        if (NEG) asm volatile("s_nop 1\n\t" DN16(16, 18) DN16(17, 19) DN16(16, 19) DN16(17, 18) : ACC16 : "v"(v0), "v"(v1), "v"(t0), "v"(t1));
        else     asm volatile("s_nop 1\n\t" DP16(16, 18) DP16(17, 19) DP16(16, 19) DP16(17, 18) : ACC16 : "v"(v0), "v"(v1), "v"(t0), "v"(t1));
    }
    double s = 0.0;
    for (int c = 0; c < NACC; ++c) s += acc[c];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// (c) 64 plain FMAs per iteration in two chunks of the rank-2 update's shape: eight ds_read_b128 of v, eight of w (every lane the same
// address), then a[i] = fma(-w_i, vj, fma(-v_i, wj, a[i])) on sixteen rows
__global__ void __launch_bounds__(256) k_lds(double* out, double a0, double b0) {
    __shared__ __attribute__((aligned(16))) double vb[64], pb[64];
    if (threadIdx.x < 64) { vb[threadIdx.x] = b0 * threadIdx.x; pb[threadIdx.x] = -b0 * threadIdx.x; }
    __syncthreads();
    double acc[NACC];
    for (int c = 0; c < NACC; ++c) acc[c] = c * 1e-3;
    const double vj = a0 + threadIdx.x * 1e-9, wj = a0 - threadIdx.x * 1e-9;
    for (int it = 0; it < ITERS; ++it) {
#pragma unroll
        for (int c = 0; c < 32; c += 16) {
            double2 v2[8], w2[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                v2[u] = *reinterpret_cast<const double2*>(&vb[c + 2 * u]);
                w2[u] = *reinterpret_cast<const double2*>(&pb[c + 2 * u]);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                acc[2 * u] = fma(-w2[u].x, vj, fma(-v2[u].x, wj, acc[2 * u]));
                acc[2 * u + 1] = fma(-w2[u].y, vj, fma(-v2[u].y, wj, acc[2 * u + 1]));
            }
            asm volatile("" ::: "memory");   // the operands are read again every time
        }
    }
    double s = 0.0;
    for (int c = 0; c < NACC; ++c) s += acc[c];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <typename K>
static double run_ms(K kernel, int blocks, int threads, double* out) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, 0, out, 1.0000001, 1e-9);   // warm-up
    hipDeviceSynchronize();
    double best = 1e30;
    for (int rep = 0; rep < 3; ++rep) {
        hipEventRecord(e0);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, 0, out, 1.0000001, 1e-9);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        if (ms < best) best = ms;
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    return best;
}

int main() {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) { fprintf(stderr, "no device\n"); return 1; }
    const int cus = p.multiProcessorCount;
    double* out;
    if (hipMalloc(&out, sizeof(double) * 256 * cus * 4) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    printf("device %s, %d CUs, clock %d MHz; %d iterations of 64 fp64 multiply-adds per wave\n", p.gcnArchName, cus, p.clockRate / 1000, ITERS);
    printf("ns per wave-level multiply-add and SIMD (best of 3 launches); in brackets: ratio to (a)\n");
    printf("%-22s %12s %20s %20s %20s\n", "waves per SIMD", "(a) fmac", "(b) fmac_dpp", "(b') fmac_dpp -src", "(c) ds_read_b128+fma");
    const double fmas = (double)ITERS * 64.0;
    for (int mode = 0; mode < 4; ++mode) {
        // mode 0: one wave alone on each CU; modes 1 .. 3: 1, 2, 4 waves on each of the four SIMDs
        const int threads = mode == 0 ? 64 : 256, wps = mode == 0 ? 1 : 1 << (mode - 1), blocks = cus * wps;
        const double a = run_ms(k_plain, blocks, threads, out), b = run_ms(k_dpp<false>, blocks, threads, out),
                     bn = run_ms(k_dpp<true>, blocks, threads, out), c = run_ms(k_lds, blocks, threads, out);
        const double sc = 1e6 / (fmas * wps);
        char label[32];
        snprintf(label, sizeof label, mode == 0 ? "1 (1 SIMD per CU)" : "%d (4 SIMDs)", wps);
        printf("%-22s %9.3f ns %11.3f ns (%4.2f) %11.3f ns (%4.2f) %11.3f ns (%4.2f)\n", label, a * sc, b * sc, b / a, bn * sc, bn / a, c * sc, c / a);
    }
    if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "device error\n"); return 1; }
    hipFree(out);
    return 0;
}
