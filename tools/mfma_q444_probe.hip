// mfma_q444_probe.hip -- do v_mfma_f64_16x16x4 and v_mfma_f64_4x4x4_4b round alike?  The same A (16 x 8) and B (8 x 16) go through
//   two v_mfma_f64_16x16x4 (k = 0..3, then k = 4..7, accumulator from zero): D register r, lane 16 i + c = D[4 r + i][c], and
//   2 x 4 v_mfma_f64_4x4x4_4b, strip by strip: for the rows 4 rb .. 4 rb + 3 the A block A[4 rb + i][4 q + k] at lane 16 k + 4 b + i
//   (the same block for the four b) against the B register as it is (B[4 q + k][c] at lane 16 k + c), the same k grouping,
// and the D strips are compared BIT FOR BIT.  This is the premise of forming the gradient's Q = conj(Lambda) Psi^T of k_mfma_downup on the
// 4x4x4 form (csrc/qoc_mfma_downup.h, QOC_DOWNUP_Q444).  Operands: sign * (1 + u) * 2^e, e uniform in [-E, E], for E = 0, 2, 30, 300
// (narrow: the roundings of near-equal terms; wide: alignment shifts and cancellations), TRIALS tiles each.  Also reported: how far both
// are from a sequential fma chain on the host (the layout check: a wrong lane assignment would not be a rounding difference).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

typedef double d4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(64) k_probe(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ D16, double* __restrict__ D4) {
    const int lane = threadIdx.x, lk = lane >> 4, lc = lane & 15, li = lane & 3;
    const double* a = A + (size_t)blockIdx.x * 128;          // A[row][8]
    const double* b = B + (size_t)blockIdx.x * 128;          // B[k][16]
    d4 d = {0, 0, 0, 0};
    double s[4] = {0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const double bv = b[(4 * q + lk) * 16 + lc];
        d = __builtin_amdgcn_mfma_f64_16x16x4f64(a[lc * 8 + 4 * q + lk], bv, d, 0, 0, 0);
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) s[rb] = __builtin_amdgcn_mfma_f64_4x4x4f64(a[(4 * rb + li) * 8 + 4 * q + lk], bv, s[rb], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        D16[(size_t)blockIdx.x * 256 + (4 * r + lk) * 16 + lc] = d[r];
        D4[(size_t)blockIdx.x * 256 + (4 * r + lk) * 16 + lc] = s[r];
    }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 1; } } while (0)

int main() {
    const int TRIALS = 4096;
    const int spreads[4] = {0, 2, 30, 300};
    std::mt19937_64 rng(20240607);
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    std::vector<double> hA((size_t)TRIALS * 128), hB((size_t)TRIALS * 128), h16((size_t)TRIALS * 256), h4((size_t)TRIALS * 256);
    double *dA, *dB, *d16, *d4p;
    CK(hipMalloc(&dA, hA.size() * sizeof(double))); CK(hipMalloc(&dB, hB.size() * sizeof(double)));
    CK(hipMalloc(&d16, h16.size() * sizeof(double))); CK(hipMalloc(&d4p, h4.size() * sizeof(double)));
    long total_diff = 0;
    for (int E : spreads) {
        std::uniform_int_distribution<int> ue(-E, E);
        auto draw = [&]() { const double v = std::ldexp(1.0 + u01(rng), ue(rng)); return (rng() & 1) ? -v : v; };
        for (auto& v : hA) v = draw();
        for (auto& v : hB) v = draw();
        CK(hipMemcpy(dA, hA.data(), hA.size() * sizeof(double), hipMemcpyHostToDevice));
        CK(hipMemcpy(dB, hB.data(), hB.size() * sizeof(double), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_probe, dim3(TRIALS), dim3(64), 0, 0, dA, dB, d16, d4p);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(h16.data(), d16, h16.size() * sizeof(double), hipMemcpyDeviceToHost));
        CK(hipMemcpy(h4.data(), d4p, h4.size() * sizeof(double), hipMemcpyDeviceToHost));
        long diff = 0, not_chain = 0, nonfinite = 0;
        double worst = 0.0, worst_host = 0.0;
        for (int t = 0; t < TRIALS; ++t)
            for (int r = 0; r < 16; ++r)
                for (int c = 0; c < 16; ++c) {
                    const double x = h16[(size_t)t * 256 + r * 16 + c], y = h4[(size_t)t * 256 + r * 16 + c];
                    uint64_t bx, by;
                    std::memcpy(&bx, &x, 8); std::memcpy(&by, &y, 8);
                    double ref = 0.0, mag = 0.0;
                    for (int k = 0; k < 8; ++k) {
                        ref = std::fma(hA[(size_t)t * 128 + r * 8 + k], hB[(size_t)t * 128 + k * 16 + c], ref);
                        mag += std::fabs(hA[(size_t)t * 128 + r * 8 + k] * hB[(size_t)t * 128 + k * 16 + c]);
                    }
                    if (!std::isfinite(x) || !std::isfinite(y)) ++nonfinite;
                    if (bx != by) { ++diff; if (mag > 0.0) worst = std::fmax(worst, std::fabs(x - y) / mag); }
                    if (x != ref) ++not_chain;
                    if (mag > 0.0) worst_host = std::fmax(worst_host, std::fabs(x - ref) / mag);
                }
        printf("exponent spread +-%3d: %d tiles, %ld of %ld D entries differ between 16x16x4 and 4x4x4_4b (largest |diff| / sum|a b| %.3e); "
               "16x16x4 off a sequential host fma chain in %ld entries, at most %.3e of sum|a b|; non-finite %ld\n",
               E, TRIALS, diff, (long)TRIALS * 256, worst, not_chain, worst_host, nonfinite);
        total_diff += diff;
    }
    printf("%s\n", total_diff == 0 ? "RESULT: bit-identical" : "RESULT: the two shapes round differently");
    return 0;
}
