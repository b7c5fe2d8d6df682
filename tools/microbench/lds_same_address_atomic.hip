// GPU box: what a returning LDS atomic add costs when the 64 lanes of a wave hit 1, 2, 3 or 64 distinct addresses (the
// tails of path_pool's queues: a push by one atomic per lane puts 64 lanes on the 2-3 tails its batch feeds), and what
// that traffic does to the vector-ALU stream of the other waves on the same SIMDs.
//   hipcc --offload-arch=gfx950 -O3 tools/microbench/lds_same_address_atomic.hip -o /tmp/lds_atomic && /tmp/lds_atomic
// 8 waves per SIMD (4 workgroups of 8 waves per CU) in every run.
//   part 1: every wave issues ITER x 8 ds_add_rtn_u32 (8 in flight, then a wait); all waves of a workgroup share the addresses.
//           cycles per wave-instruction per CU: the LDS pipe is one per CU.
//   part 2: waves 0-3 of each workgroup (one per SIMD) run 16 independent v_fma_f32 chains, waves 4-7 either leave at once
//           ("alone") or keep issuing the atomics on 3 addresses until the kernel ends ("with LDS atomics"); the VALU
//           waves time themselves with the constant 100 MHz clock.  cycles per wave-instruction per SIMD.
// Cycles are priced at 2.4 GHz like the other microbenchmarks here; the clock the part ran at is lower under load.
#include <hip/hip_runtime.h>
#include <cstdio>
constexpr int ITER = 2048;
constexpr int VITER = 4096;

__device__ __forceinline__ unsigned atomics8(unsigned addr, unsigned one) {
    unsigned r0, r1, r2, r3, r4, r5, r6, r7;
    asm volatile("ds_add_rtn_u32 %0, %8, %9\n\tds_add_rtn_u32 %1, %8, %9\n\tds_add_rtn_u32 %2, %8, %9\n\tds_add_rtn_u32 %3, %8, %9\n\t"
                 "ds_add_rtn_u32 %4, %8, %9\n\tds_add_rtn_u32 %5, %8, %9\n\tds_add_rtn_u32 %6, %8, %9\n\tds_add_rtn_u32 %7, %8, %9\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7) : "v"(addr), "v"(one) : "memory");
    return r0 ^ r1 ^ r2 ^ r3 ^ r4 ^ r5 ^ r6 ^ r7;
}

__global__ __launch_bounds__(512) void lds_rate(unsigned *out, int n_addr) {
    __shared__ unsigned tails[64];
    if (threadIdx.x < 64) tails[threadIdx.x] = 0;
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u;
    const unsigned addr = (unsigned)(uintptr_t)tails + (lane % (unsigned)n_addr) * 4u;
    unsigned acc = 0;
    for (int i = 0; i < ITER; i++) acc ^= atomics8(addr, 1u);
    if (acc == 0xDEADBEEFu) out[0] = acc;
}

// out[0]: sum of the VALU waves' ticks (100 MHz), out[1]: their number, out[2]: the longest
__global__ __launch_bounds__(512) void mixed(unsigned long long *out, int lds_traffic, float seed) {
    __shared__ unsigned tails[64];
    __shared__ unsigned done;
    if (threadIdx.x < 64) tails[threadIdx.x] = 0;
    if (threadIdx.x == 0) done = 0;
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (wave < 4) {
        float a[16];
        for (int k = 0; k < 16; k++) a[k] = seed + k + threadIdx.x;
        const float m = 1.0000001f;
        const unsigned long long t0 = wall_clock64();
        for (int i = 0; i < VITER; i++) {
#pragma unroll
            for (int k = 0; k < 16; k++) asm volatile("v_fma_f32 %0, %0, %1, %1" : "+v"(a[k]) : "v"(m));
        }
        const unsigned long long dt = wall_clock64() - t0;
        float s = 0;
        for (int k = 0; k < 16; k++) s += a[k];
        if (s == 12345.678f) out[3] = 1;
        if (lane == 0) { atomicAdd(&out[0], dt); atomicAdd(&out[1], 1ull); atomicMax(&out[2], dt); atomicAdd(&done, 1u); }
    } else if (lds_traffic) {
        const unsigned addr = (unsigned)(uintptr_t)tails + (lane % 3u) * 4u;
        unsigned acc = 0;
        // until the four VALU waves of this workgroup are through (bounded: a logic error must not hang the GPU)
        for (int i = 0; i < 64 * ITER; i++) {
            acc ^= atomics8(addr, 1u);
            if (__hip_atomic_load(&done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= 4u) break;
        }
        if (acc == 0xDEADBEEFu) out[3] = acc;
    }
}

int main() {
    unsigned long long *d;
    if (hipMalloc(&d, 64) != hipSuccess) { printf("no device memory\n"); return 1; }
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    int cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) == hipSuccess) cus = prop.multiProcessorCount;
    const int blocks = cus * 4;              // 4 workgroups of 8 waves per CU = 8 waves per SIMD
    printf("# ds_add_rtn_u32, 64 lanes on N distinct addresses; %d CUs, 8 waves per SIMD, cycles at 2.4 GHz\n", cus);
    printf("# addresses        ms   cycles per wave-instruction per CU\n");
    const int n_addrs[4] = { 1, 2, 3, 64 };
    for (int a = 0; a < 4; a++) {
        lds_rate<<<blocks, 512>>>((unsigned *)d, n_addrs[a]);
        hipEventRecord(e0);
        for (int r = 0; r < 3; r++) lds_rate<<<blocks, 512>>>((unsigned *)d, n_addrs[a]);
        hipEventRecord(e1);
        if (hipEventSynchronize(e1) != hipSuccess) { printf("launch failed\n"); return 1; }
        float ms; hipEventElapsedTime(&ms, e0, e1); ms /= 3;
        const double per_cu = (double)blocks / cus * 8 * ITER * 8;
        printf("  %9d  %8.3f   %.2f\n", n_addrs[a], ms, ms * 1e-3 * 2.4e9 / per_cu);
    }
    printf("# v_fma_f32 stream of 4 waves per SIMD, next to 4 waves per SIMD that idle or issue the atomics (3 addresses)\n");
    printf("# neighbours            mean ms   longest ms   cycles per wave-instruction per SIMD\n");
    for (int traffic = 0; traffic < 2; traffic++) {
        unsigned long long h[4];
        for (int r = 0; r < 3; r++) {            // (the last of three runs counts)
            hipMemset(d, 0, 64);
            mixed<<<blocks, 512>>>(d, traffic, 1.0f);
            if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
        }
        hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);
        const double mean_ms = (double)h[0] / (double)(h[1] ? h[1] : 1) / 1e5, max_ms = (double)h[2] / 1e5;
        // one SIMD issues for its 4 VALU waves: 4 x VITER x 16 wave-instructions in that time
        printf("  %-18s  %8.3f     %8.3f   %.2f\n", traffic ? "with LDS atomics" : "alone", mean_ms, max_ms, mean_ms * 1e-3 * 2.4e9 / (4.0 * VITER * 16));
    }
    return 0;
}
