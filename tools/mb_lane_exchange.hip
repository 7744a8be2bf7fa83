// The all-reduce over the four K-slice lanes of a pixel (lanes l, l ^ 16, l ^ 32, l ^ 48) carried by the LDS pipe (ds_swizzle +
// ds_bpermute) and by the vector pipe (v_permlane16_swap + v_permlane32_swap): csrc/wave_util.hpp, quad_sum / quad_max.
//  1. Are the two the same bits?  Every set of 64 lane values -- random finite values; +0, -0, +inf, -inf and NaN in every lane
//     position among random values and among -inf (the softmax's masked planes); sets of specials only -- goes through both
//     forms of the sum and of the maximum in one test wave per SIMD of every CU; every lane compares the bits.
//  2. What does a step (transport + combine) cost a wave that waits for it?  A chain of dependent quad_sum, cycles by clock64().
// Both "alone" (the test waves are the only ones) and "loaded": the three other waves of every SIMD run
// v_mfma_f32_16x16x32_f16 and same-address LDS atomics meanwhile, as the other waves of the sweep kernel do (beside that
// instruction packed fp32 loses results on gfx950: wave_util.hpp -- hence the look at a new cross-lane vector instruction).
// Prints per setting `mismatches N` and the cycles per step of both forms; exit status 1 on any mismatch.
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -I probabilistic-depth_amd/csrc -o tools/mb_lane_exchange tools/mb_lane_exchange.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "wave_util.hpp"

using namespace pdepth::wv;
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

constexpr int WAVES = 16;     // per workgroup: waves 0..3 test (one per SIMD), waves 4..15 are the load
constexpr int CHAIN = 64;     // dependent quad_sum per timed stretch (two steps each)

// the load of a wave: multiplications and two LDS atomics on one address per round, like a sweep wave between its barriers
__device__ __forceinline__ float load_wave(int rounds, int* tab, int lane) {
    h8 a, b;
    for (int i = 0; i < 8; ++i) { a[i] = (_Float16)(0.001f * (lane + i)); b[i] = (_Float16)(0.002f * (lane - i)); }
    v4f acc = {0, 0, 0, 0};
    for (int r = 0; r < rounds; ++r) {
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
        atomicMin(&tab[(r & 7) * 2], lane - r);
        atomicMax(&tab[(r & 7) * 2 + 1], lane + r);
    }
    return acc.x + acc.y + acc.z + acc.w;
}

// in: nsets x 64 lane values.  Every test wave runs every set through both forms of both reductions; bad[0 .. 1]: lanes whose
// sum / maximum differ between the forms; first[0 .. 3]: set, lane, bits (LDS pipe), bits (swaps) of one of them.
// keep[]: per thread, so that nothing is optimised away; sums[set * 64 + lane], maxs[...]: the swaps' results of workgroup 0, wave 0
__global__ __launch_bounds__(WAVES * 64) void check_kernel(const unsigned* in, int nsets, int loaded, int load_rounds, unsigned* bad,
                                                           unsigned* first, float* keep, unsigned* sums, unsigned* maxs) {
    __shared__ int tab[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 16) tab[threadIdx.x] = threadIdx.x & 1 ? INT_MIN : INT_MAX;
    __syncthreads();
    const int a32 = (lane ^ 32) << 2;
    if (wave >= 4) {
        if (loaded) keep[blockIdx.x * (WAVES * 64) + threadIdx.x] = load_wave(load_rounds, tab, lane);
        return;
    }
    unsigned nbad_s = 0, nbad_m = 0, acc = 0;
    for (int s = 0; s < nsets; ++s) {
        const float x = __builtin_bit_cast(float, in[s * 64 + lane]);
        const unsigned s0 = __builtin_bit_cast(unsigned, quad_sum<0>(x, a32)), s1 = __builtin_bit_cast(unsigned, quad_sum<1>(x, a32));
        const unsigned m0 = __builtin_bit_cast(unsigned, quad_max<0>(x, a32)), m1 = __builtin_bit_cast(unsigned, quad_max<1>(x, a32));
        if (s0 != s1 || m0 != m1) {
            if (atomicAdd(&first[4], 1u) == 0) { first[0] = s; first[1] = lane; first[2] = s0 != s1 ? s0 : m0; first[3] = s0 != s1 ? s1 : m1; }
        }
        nbad_s += s0 != s1;
        nbad_m += m0 != m1;
        acc ^= s1 ^ m1;
        if (blockIdx.x == 0 && wave == 0) { sums[s * 64 + lane] = s1; maxs[s * 64 + lane] = m1; }
    }
    if (nbad_s) atomicAdd(&bad[0], nbad_s);
    if (nbad_m) atomicAdd(&bad[1], nbad_m);
    keep[blockIdx.x * (WAVES * 64) + threadIdx.x] = __builtin_bit_cast(float, acc & 0x3fffffffu);
}

// cycles of CHAIN dependent quad_sum<XCHG> (2 CHAIN steps), the least of `reps` stretches, per test wave: cyc[workgroup * 4 + wave]
template <int XCHG>
__global__ __launch_bounds__(WAVES * 64) void time_kernel(int reps, int loaded, int load_rounds, float* keep, unsigned* cyc) {
    __shared__ int tab[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 16) tab[threadIdx.x] = threadIdx.x & 1 ? INT_MIN : INT_MAX;
    __syncthreads();
    const int a32 = (lane ^ 32) << 2;
    if (wave >= 4) {
        if (loaded) keep[blockIdx.x * (WAVES * 64) + threadIdx.x] = load_wave(load_rounds, tab, lane);
        return;
    }
    float x = 1.0f + lane * 0.5f;
    unsigned long long sum = 0;
    unsigned best = 0xffffffffu;
    for (int r = 0; r < reps; ++r) {
        const unsigned long long t0 = clock64();
        asm volatile("" : "+v"(x));
#pragma unroll
        for (int i = 0; i < CHAIN; ++i) x = quad_sum<XCHG>(x, a32);   // (runs up to inf: the time does not depend on the value)
        asm volatile("" : "+v"(x));
        const unsigned long long t1 = clock64();
        best = min(best, (unsigned)(t1 - t0));
        sum += t1 - t0;
    }
    keep[blockIdx.x * (WAVES * 64) + threadIdx.x] = x;
    if (lane == 0) { cyc[(blockIdx.x * 4 + wave) * 2] = best; cyc[(blockIdx.x * 4 + wave) * 2 + 1] = (unsigned)(sum / reps); }
}

static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static float flt(unsigned u) { float f; memcpy(&f, &u, 4); return f; }

int main() {
    // ---- the sets ----
    std::vector<unsigned> in;
    std::vector<int> finite;   // sets the host can check (finite values: the host's float sums round alike)
    unsigned rng = 12345u;
    auto rnd = [&]() { rng = rng * 1664525u + 1013904223u; return (float)((int)(rng >> 8) - (1 << 23)) * (1000.0f / (1 << 23)); };
    const unsigned special[5] = {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u};   // +0, -0, +inf, -inf, NaN
    auto push_set = [&](auto f, bool fin) { if (fin) finite.push_back((int)in.size() / 64); for (int l = 0; l < 64; ++l) in.push_back(f(l)); };
    for (int i = 0; i < 64; ++i) push_set([&](int) { return bits(rnd()); }, true);
    for (int sp = 0; sp < 5; ++sp)
        for (int pos = 0; pos < 64; ++pos) {
            push_set([&](int l) { return l == pos ? special[sp] : bits(rnd()); }, false);        // among random values
            push_set([&](int l) { return l == pos ? special[sp] : 0xff800000u; }, false);        // among -inf (masked planes)
            push_set([&](int l) { return l == pos ? bits(rnd()) : special[sp]; }, false);        // one value among specials
        }
    for (int sp = 0; sp < 5; ++sp) push_set([&](int) { return special[sp]; }, false);
    for (int i = 0; i < 64; ++i)   // specials and values at random
        push_set([&](int) { rng = rng * 1664525u + 1013904223u; const unsigned k = (rng >> 20) % 10; return k < 5 ? special[k] : bits(rnd()); }, false);
    const int nsets = (int)in.size() / 64;

    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int blocks = prop.multiProcessorCount;   // a workgroup of 16 waves per CU
    const size_t nthreads = (size_t)blocks * WAVES * 64;
    unsigned *d_in, *d_bad, *d_first, *d_cyc, *d_sums, *d_maxs;
    float* d_keep;
    CHECK(hipMalloc(&d_in, in.size() * 4));
    CHECK(hipMalloc(&d_bad, 2 * 4));
    CHECK(hipMalloc(&d_first, 5 * 4));
    CHECK(hipMalloc(&d_cyc, (size_t)blocks * 4 * 2 * 4));
    CHECK(hipMalloc(&d_sums, in.size() * 4));
    CHECK(hipMalloc(&d_maxs, in.size() * 4));
    CHECK(hipMalloc(&d_keep, nthreads * 4));
    CHECK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    printf("%s, %d CUs; %d sets of 64 lane values, every set in %d test waves (one per SIMD)\n", prop.name, blocks, nsets, blocks * 4);

    // rounds of the load waves: long enough to outlast the test waves (8 multiplications + 2 atomics per round)
    const int check_load_rounds = 10 * nsets, reps = 50, time_load_rounds = 10 * reps * CHAIN;
    unsigned long long total_bad = 0;
    for (int loaded = 0; loaded < 2; ++loaded) {
        const char* name = loaded ? "loaded" : "alone";
        CHECK(hipMemset(d_bad, 0, 2 * 4));
        CHECK(hipMemset(d_first, 0, 5 * 4));
        hipLaunchKernelGGL(check_kernel, dim3(blocks), dim3(WAVES * 64), 0, 0, d_in, nsets, loaded, check_load_rounds, d_bad, d_first, d_keep, d_sums, d_maxs);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        unsigned bad[2], first[5];
        CHECK(hipMemcpy(bad, d_bad, sizeof bad, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(first, d_first, sizeof first, hipMemcpyDeviceToHost));
        // the swaps' results against the host on the finite sets (both forms agreeing on a wrong value would pass the comparison)
        std::vector<unsigned> sums(in.size()), maxs(in.size());
        CHECK(hipMemcpy(sums.data(), d_sums, in.size() * 4, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(maxs.data(), d_maxs, in.size() * 4, hipMemcpyDeviceToHost));
        unsigned host_bad = 0;
        for (int s : finite)
            for (int l = 0; l < 64; ++l) {
                const unsigned* v = &in[(size_t)s * 64];
                const volatile float p = flt(v[l]) + flt(v[l ^ 16]), q = flt(v[l ^ 32]) + flt(v[l ^ 48]);
                const volatile float sum = p + q;
                const float mx = std::max(std::max(flt(v[l]), flt(v[l ^ 16])), std::max(flt(v[l ^ 32]), flt(v[l ^ 48])));
                host_bad += bits(sum) != sums[(size_t)s * 64 + l];
                host_bad += bits(mx) != maxs[(size_t)s * 64 + l];
            }
        const unsigned long long n = (unsigned long long)bad[0] + bad[1] + host_bad;
        total_bad += n;
        printf("%-6s: mismatches %llu  (sum %u, max %u of %llu lane results each; against the host on the %d finite sets: %u)\n", name, n,
               bad[0], bad[1], (unsigned long long)blocks * 4 * nsets * 64, (int)finite.size(), host_bad);
        if (bad[0] + bad[1]) printf("        e.g. set %u lane %u: LDS pipe %08x, swaps %08x\n", first[0], first[1], first[2], first[3]);

        double med[2][2];
        for (int form = 0; form < 2; ++form) {
            if (form == 0) hipLaunchKernelGGL(time_kernel<0>, dim3(blocks), dim3(WAVES * 64), 0, 0, reps, loaded, time_load_rounds, d_keep, d_cyc);
            else hipLaunchKernelGGL(time_kernel<1>, dim3(blocks), dim3(WAVES * 64), 0, 0, reps, loaded, time_load_rounds, d_keep, d_cyc);
            CHECK(hipGetLastError());
            CHECK(hipDeviceSynchronize());
            std::vector<unsigned> cyc((size_t)blocks * 4 * 2);
            CHECK(hipMemcpy(cyc.data(), d_cyc, cyc.size() * 4, hipMemcpyDeviceToHost));
            for (int k = 0; k < 2; ++k) {
                std::vector<unsigned> v;
                for (size_t i = k; i < cyc.size(); i += 2) v.push_back(cyc[i]);
                std::sort(v.begin(), v.end());
                med[form][k] = (double)v[v.size() / 2] / (2 * CHAIN);
            }
        }
        printf("%-6s: cycles per step (transport + combine + wait, a dependent chain; median over the test waves of least / mean of %d stretches):"
               " LDS pipe %.1f / %.1f, swaps %.1f / %.1f\n", name, reps, med[0][0], med[0][1], med[1][0], med[1][1]);
    }
    printf("total mismatches %llu\n", total_bad);
    return total_bad ? 1 : 0;
}
