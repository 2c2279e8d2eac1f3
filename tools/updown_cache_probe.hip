// updown_cache_probe.hip -- does a second pass over a chunk of K, taken right after the first one in the opposite direction, come out of a
// cache?  (forward + adjoint sweep in one kernel.)  The K trajectory of the bench is 64 seeds x 500 slices x 16 KB = 524 MB;
// a (seed, chunk) item of S slices is S x 16 KB.  One wave per item streams its slices up (mode 0), up and back down (mode 1), or up twice
// (mode 2); a writer kernel fills the buffer first (as the exponential kernel does in the iteration).  Output: time and GB/s per mode for
// several chunk lengths and occupancies (dynamic LDS limits the workgroups per CU).
//
// `updown_cache_probe policy`: the cache-policy grid of the fused sweep (csrc/qoc_mfma_downup.h) on the same buffer -- a PAIR of waves per item as
// in k_mfma_downup (wave 0 up the first half, wave 1 down from the chunk's end, both storing 4 KB of X per 16 KB slice; then each goes back over
// its half reading K and X again), 4 pairs per workgroup, one workgroup per CU, with the knobs of the kernels: the writer's stores (plain / nt /
// write-through, QOC_EXPM_KSTORE), the K loads of pass A and pass B (QOC_DOWNUP_KA / KB), the X stores and loads (QOC_DOWNUP_XS / XL) and the
// late start of wave 0 (QOC_DOWNUP_LATE0).  No arithmetic beyond sums: it ranks what the memory system does with the streams, nothing else.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)
typedef double d2 __attribute__((ext_vector_type(2)));

// the writer: as the exponential kernel, one wave per item writes its S slices in time order, all items at once (so what was written LAST --
// what a write-back cache still holds -- is the late slices of every item, not the end of the buffer)
__global__ void __launch_bounds__(64) k_fill(d2* p, int S, int nt) {
    d2* base = p + (size_t)blockIdx.x * S * 1024;
    for (int s = 0; s < S; ++s) {
        if (nt == 2) {                                                  // write-through
#pragma unroll
            for (int q = 0; q < 16; ++q)
                asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" :: "v"(&base[(size_t)s * 1024 + q * 64 + threadIdx.x]), "v"((d2){(double)(s + q), 1.0}) : "memory");
        } else if (nt) {
#pragma unroll
            for (int q = 0; q < 16; ++q) __builtin_nontemporal_store((d2){(double)(s + q), 1.0}, &base[(size_t)s * 1024 + q * 64 + threadIdx.x]);
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) base[(size_t)s * 1024 + q * 64 + threadIdx.x] = (d2){(double)(s + q), 1.0};
        }
        __builtin_amdgcn_s_sleep(100);
    }
}

__device__ __forceinline__ void slice_sum(const d2* __restrict__ F, int lane, d2 (&acc)[4]) {
    d2 v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = F[q * 64 + lane];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q & 3] += v[q];
}

__global__ void __launch_bounds__(256) k_probe(const d2* __restrict__ K, double* out, int items, int S, int mode) {
    extern __shared__ char smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    d2 acc[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    for (int item = blockIdx.x * 4 + wv; item < items; item += gridDim.x * 4) {
        const d2* base = K + (size_t)item * S * 1024;
        if (mode == 5 || mode == 6) {                                   // up, the loads of DEPTH slices in flight (5: two, 6: three)
            d2 v0[16], v1[16], v2[16];
            auto ld = [&](d2 (&v)[16], int s) {
#pragma unroll
                for (int q = 0; q < 16; ++q) v[q] = base[(size_t)(s < S ? s : S - 1) * 1024 + q * 64 + lane];
                asm volatile("" ::: "memory");
            };
            auto use = [&](d2 (&v)[16]) {
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[q & 3] += v[q];
            };
            if (mode == 5) {
                ld(v0, 0);
                for (int s = 0; s < S; s += 2) { ld(v1, s + 1); use(v0); ld(v0, s + 2); use(v1); }
            } else {
                ld(v0, 0); ld(v1, 1);
                for (int s = 0; s < S; s += 3) { ld(v2, s + 2); use(v0); ld(v0, s + 3); use(v1); ld(v1, s + 4); use(v2); }
            }
            continue;
        }
        if (mode >= 3) {                                                // 3: down only, 4: down and back up
            for (int s = S - 1; s >= 0; --s) slice_sum(base + (size_t)s * 1024, lane, acc);
            if (mode == 4) for (int s = 0; s < S; ++s) slice_sum(base + (size_t)s * 1024, lane, acc);
            continue;
        }
        for (int s = 0; s < S; ++s) slice_sum(base + (size_t)s * 1024, lane, acc);
        if (mode == 1) for (int s = S - 1; s >= 0; --s) slice_sum(base + (size_t)s * 1024, lane, acc);
        if (mode == 2) for (int s = 0; s < S; ++s) slice_sum(base + (size_t)s * 1024, lane, acc);
    }
    const d2 t = acc[0] + acc[1] + acc[2] + acc[3];
    if (t.x == -1.0) out[threadIdx.x] = t.y;
    if (smem[0] == 77 && t.y == -2.0) out[0] = 1.0;
}

// ---- the policy grid ----------------------------------------------------------------------------------------------------------------------
template <bool NTL> __device__ __forceinline__ d2 ld(const d2* p) { if constexpr (NTL) return __builtin_nontemporal_load(p); else return *p; }
template <bool NTS> __device__ __forceinline__ void st(d2* p, d2 v) { if constexpr (NTS) __builtin_nontemporal_store(v, p); else *p = v; }

// items of S slices; X: [items * S][256] d2 (4 KB per slice)
template <bool KA, bool KB, bool XS, bool XL, bool LATE>
__global__ void __launch_bounds__(512) k_pair(const d2* __restrict__ K, d2* __restrict__ X, double* out, int items, int S) {
    extern __shared__ char smem[];
    volatile int* flag = (volatile int*)smem;                           // per pair: wave 1 is half way down
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, role = wv & 1, pr = wv >> 1;
    if (threadIdx.x < 4) flag[threadIdx.x] = 0;
    __syncthreads();
    const int item = blockIdx.x * 4 + pr;
    if (item >= items) return;
    const d2* base = K + (size_t)item * S * 1024;
    d2* xb = X + (size_t)item * S * 256;
    const int sm = (S + 1) / 2;
    d2 acc[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    auto slice = [&](int s, auto ntl, bool store, bool loadx) {
        d2 v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = ld<decltype(ntl)::value>(base + (size_t)s * 1024 + q * 64 + lane);
        if (loadx) {
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += ld<XL>(xb + (size_t)s * 256 + q * 64 + lane);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q & 3] += v[q];
        if (store) {
#pragma unroll
            for (int q = 0; q < 4; ++q) st<XS>(xb + (size_t)s * 256 + q * 64 + lane, acc[q]);
        }
    };
    std::integral_constant<bool, KA> ka; std::integral_constant<bool, KB> kb;
    if (role == 0) {
        if (LATE) while (flag[pr] == 0) __builtin_amdgcn_s_sleep(8);
        for (int s = 0; s < sm; ++s) slice(s, ka, true, false);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        for (int s = sm - 1; s >= 0; --s) slice(s, kb, false, true);
    } else {
        const int n = S - sm;
        if (LATE && n / 2 == 0 && lane == 0) flag[pr] = 1;
        for (int i = 0; i < n; ++i) {
            if (LATE && i > 0 && i == n / 2 && lane == 0) flag[pr] = 1;
            slice(S - 1 - i, ka, true, false);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        for (int s = sm; s < S; ++s) slice(s, kb, false, true);
    }
    const d2 t = acc[0] + acc[1] + acc[2] + acc[3];
    if (t.x == -1.0) out[threadIdx.x] = t.y;
}

template <int BITS>
static void pair_launch(int bits, const d2* K, d2* X, double* out, int items, int S, size_t lds) {
    if constexpr (BITS >= 0) {
        if (bits == BITS) {
            auto fn = k_pair<(BITS & 1) != 0, (BITS & 2) != 0, (BITS & 4) != 0, (BITS & 8) != 0, (BITS & 16) != 0>;
            CHECK(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(fn, dim3((items + 3) / 4), dim3(512), lds, 0, K, X, out, items, S);
        } else pair_launch<BITS - 1>(bits, K, X, out, items, S, lds);
    }
}

static int policy_grid() {
    const int S = 32, items = 64 * 500 / S;                             // the bench: 64 seeds x 500 slices, 16 chunks a seed
    const size_t n = (size_t)items * S * 1024;
    d2 *K, *X; double* out;
    CHECK(hipMalloc((void**)&K, n * sizeof(d2)));
    CHECK(hipMalloc((void**)&X, n / 4 * sizeof(d2)));
    CHECK(hipMalloc((void**)&out, 4096));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const size_t lds = 150 * 1024;                                      // one workgroup per CU, as k_mfma_downup
    printf("K = %.0f MB, X = %.0f MB; %d items of %d slices, a pair of waves per item, 4 pairs per workgroup, one workgroup per CU; best of 4, us\n",
           n * 16 / 1e6, n * 4 / 1e6, items, S);
    printf("%-8s %-4s %-4s %-4s %-4s %-5s | %9s\n", "writer", "KA", "KB", "XS", "XL", "late0", "pair");
    const char* wn[] = {"plain", "nt", "wt"};
    // the knobs one at a time, then the combinations the single rows suggest
    const int rows[] = {0, 1, 3, 4, 12, 16, 17, 19, 13, 29, 31};       // bit 0 KA, 1 KB, 2 XS, 3 XL, 4 LATE0
    for (int w = 0; w < 3; ++w)
        for (int bits : rows) {
            float best = 1e9f;
            for (int rep = 0; rep < 4; ++rep) {
                hipLaunchKernelGGL(k_fill, dim3(items), dim3(64), 0, 0, K, S, w);
                CHECK(hipEventRecord(e0));
                pair_launch<31>(bits, K, X, out, items, S, lds);
                CHECK(hipEventRecord(e1));
                CHECK(hipEventSynchronize(e1));
                float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (ms < best) best = ms;
            }
            printf("%-8s %-4s %-4s %-4s %-4s %-5d | %9.1f\n", wn[w], bits & 1 ? "nt" : "-", bits & 2 ? "nt" : "-", bits & 4 ? "nt" : "-", bits & 8 ? "nt" : "-", (bits >> 4) & 1, best * 1e3f);
        }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && argv[1][0] == 'p') return policy_grid();
    const size_t total_slices = 64 * 500, n = total_slices * 1024;
    d2* K; double* out;
    CHECK(hipMalloc((void**)&K, n * sizeof(d2)));
    CHECK(hipMalloc((void**)&out, 4096));
    CHECK(hipFuncSetAttribute((const void*)k_probe, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const int nt = argc > 1 ? atoi(argv[1]) : 0;                        // 1: the writer uses non-temporal stores, 2: write-through stores
    printf("writer stores: %s\n", nt == 2 ? "write-through" : nt ? "non-temporal" : "plain");
    const int Ss[] = {4, 8, 16, 32};
    const int ldss[] = {0, 40 * 1024, 80 * 1024, 160 * 1024};          // workgroups per CU: 8 (register limit of the probe), 4, 2, 1
    printf("K = %.0f MB; one wave per item, 4 waves per workgroup; persistent grid of 256 x (workgroups per CU)\n", n * 16 / 1e6);
    printf("%4s %6s %6s | %9s %9s %9s %9s %9s %9s %9s (us)\n", "S", "wg/CU", "items", "up", "updown", "upup", "down", "downup", "up 2 deep", "up 3 deep");
    for (int S : Ss)
        for (int li = 0; li < 4; ++li) {
            const int items = (int)(total_slices / S), per_cu = li == 0 ? 8 : (li == 1 ? 4 : (li == 2 ? 2 : 1));
            float us[7];
            for (int mode = 0; mode < 7; ++mode) {
                float best = 1e9f;
                for (int rep = 0; rep < 4; ++rep) {
                    hipLaunchKernelGGL(k_fill, dim3(items), dim3(64), 0, 0, K, S, nt);
                    CHECK(hipEventRecord(e0));
                    hipLaunchKernelGGL(k_probe, dim3(256 * per_cu), dim3(256), ldss[li], 0, K, out, items, S, mode);
                    CHECK(hipEventRecord(e1));
                    CHECK(hipEventSynchronize(e1));
                    float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
                    if (ms < best) best = ms;
                }
                us[mode] = best * 1e3f;
            }
            printf("%4d %6d %6d | %9.1f %9.1f %9.1f %9.1f %9.1f %9.1f %9.1f\n", S, per_cu, items, us[0], us[1], us[2], us[3], us[4], us[5], us[6]);
        }
    return 0;
}
