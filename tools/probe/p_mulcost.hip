// p_mulcost.hip -- issue cost of the integer multiplies on gfx950, by in-kernel s_memtime stamps
// (measurement harness, not part of the product):
//   make -C tools/probe NAME=p_mulcost SRC=p_mulcost.hip && tools/probe/p_mulcost
// Each instruction as a dependent chain (one register) and as an independent stream (eight
// registers, round-robin), at one wave per SIMD (one 256-thread workgroup on one CU) and at eight
// waves per SIMD (two 1024-thread workgroups per CU on every CU, held there by their LDS size).
// A wave stamps s_memtime before and after N instructions; the line gives the median over the
// waves of (stamp difference) / N, the same as nanoseconds by the 100 MHz wall clock, and -- for
// eight waves -- the cycles per instruction of one SIMD, (difference) / (8 N).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#define CHECK(x)                                                                 \
    do {                                                                         \
        hipError_t e_ = (x);                                                     \
        if (e_ != hipSuccess) {                                                  \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));         \
            return 1;                                                            \
        }                                                                        \
    } while (0)

constexpr int UNROLL = 64, LOOPS = 64, N = UNROLL * LOOPS;

enum Op { MUL_LO, MUL_HI, MAD64, MUL24, ADD, N_OPS };
static const char* OP_NAME[N_OPS] = {"v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32", "v_mul_u32_u24", "v_add_u32"};

template <int OP>
__device__ __forceinline__ void one(uint32_t& a, uint64_t& w, uint32_t b) {
    if constexpr (OP == MUL_LO) asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a) : "v"(b));
    if constexpr (OP == MUL_HI) asm volatile("v_mul_hi_u32 %0, %0, %1" : "+v"(a) : "v"(b));
    if constexpr (OP == MAD64) asm volatile("v_mad_u64_u32 %0, vcc, %1, %1, %0" : "+v"(w) : "v"(b) : "vcc");
    if constexpr (OP == MUL24) asm volatile("v_mul_u32_u24 %0, %0, %1" : "+v"(a) : "v"(b));
    if constexpr (OP == ADD) asm volatile("v_add_u32 %0, %0, %1" : "+v"(a) : "v"(b));
}

// out[wave]: {memtime ticks, wall-clock ticks}; sink keeps the registers alive
template <int OP, bool INDEP>
__global__ void k_cost(uint64_t* out, uint32_t* sink, uint32_t seed) {
    extern __shared__ uint8_t hold[];  // (only its size matters: workgroups per CU)
    constexpr int R = INDEP ? 8 : 1;
    uint32_t a[R];
    uint64_t w[R];
    const uint32_t b = seed | 1u;
#pragma unroll
    for (int i = 0; i < R; i++) {
        a[i] = threadIdx.x + seed + i;
        w[i] = a[i];
    }
    __syncthreads();
    const uint64_t t0 = __builtin_amdgcn_s_memtime(), c0 = wall_clock64();
    for (int l = 0; l < LOOPS; l++) {
#pragma unroll
        for (int u = 0; u < UNROLL; u++) one<OP>(a[u % R], w[u % R], b);
    }
    const uint64_t t1 = __builtin_amdgcn_s_memtime(), c1 = wall_clock64();
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < R; i++) s ^= a[i] ^ (uint32_t)w[i] ^ (uint32_t)(w[i] >> 32);
    if (s == 0x12345678u) sink[0] = s + hold[threadIdx.x];
    if ((threadIdx.x & 63) == 0) {
        const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
        out[2 * wave] = t1 - t0;
        out[2 * wave + 1] = c1 - c0;
    }
}

template <int OP, bool INDEP>
static int run(int waves_per_simd, int cus, uint64_t* d_out, uint32_t* d_sink) {
    const int threads = waves_per_simd == 1 ? 256 : 1024;
    const int blocks = waves_per_simd == 1 ? 1 : 2 * cus;
    // one workgroup per CU (one wave per SIMD) or exactly two (eight)
    const size_t lds = waves_per_simd == 1 ? 100 * 1024 : 72 * 1024;
    auto kern = k_cost<OP, INDEP>;
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int waves = blocks * threads / 64;
    for (int rep = 0; rep < 2; rep++) {  // (the first launch warms the instruction cache)
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), lds, 0, d_out, d_sink, 12345u + rep);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
    }
    std::vector<uint64_t> h(2 * (size_t)waves);
    CHECK(hipMemcpy(h.data(), d_out, h.size() * 8, hipMemcpyDeviceToHost));
    std::vector<double> t(waves), c(waves);
    for (int i = 0; i < waves; i++) t[i] = (double)h[2 * i] / N, c[i] = (double)h[2 * i + 1] * 10.0 / N;
    std::sort(t.begin(), t.end());
    std::sort(c.begin(), c.end());
    std::printf("{\"op\": \"%s\", \"form\": \"%s\", \"waves_per_simd\": %d, \"memtime_per_instr\": %.3f, "
                "\"memtime_per_instr_min\": %.3f, \"ns_per_instr\": %.3f, \"per_simd_memtime_per_instr\": %.3f}\n",
                OP_NAME[OP], INDEP ? "independent" : "dependent", waves_per_simd, t[waves / 2], t[0], c[waves / 2],
                t[waves / 2] / waves_per_simd);
    return 0;
}

template <int OP>
static int run_op(int cus, uint64_t* d_out, uint32_t* d_sink) {
    for (int wps : {1, 8}) {
        if (run<OP, false>(wps, cus, d_out, d_sink)) return 1;
        if (run<OP, true>(wps, cus, d_out, d_sink)) return 1;
    }
    return 0;
}

int main() {
    hipDeviceProp_t p;
    CHECK(hipGetDeviceProperties(&p, 0));
    const int cus = p.multiProcessorCount;
    std::printf("{\"device\": \"%s\", \"cus\": %d, \"clock_khz\": %d, \"n\": %d}\n", p.gcnArchName, cus, p.clockRate, N);
    uint64_t* d_out;
    uint32_t* d_sink;
    CHECK(hipMalloc(&d_out, (size_t)2 * cus * 16 * 2 * 8));
    CHECK(hipMalloc(&d_sink, 64));
    if (run_op<MUL_LO>(cus, d_out, d_sink) || run_op<MUL_HI>(cus, d_out, d_sink) || run_op<MAD64>(cus, d_out, d_sink) ||
        run_op<MUL24>(cus, d_out, d_sink) || run_op<ADD>(cus, d_out, d_sink))
        return 1;
    return 0;
}
