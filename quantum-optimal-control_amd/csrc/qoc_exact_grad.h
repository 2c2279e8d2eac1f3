// qoc_exact_grad.h -- the exact gradient (qoc_config.gradient = 1): dL/du_{k,t} = Re <Lambda_{t+1}, dK_t[E_k] Psi_t>, the derivative of the
// slice propagator the engine actually computes (truncated Taylor polynomial, squarings included), in place of the reference's first-order
// Re <Lambda_{t+1}, H_k' Psi_{t+1}>.  The reference has no counterpart (core/tensorflow_state.py:49-65, 100-133 register the first-order
// formula as the gradient of matexp_op / matvecexp_op).
//
// Two steps on the generic path ("Exact gradient"):
//   k_bwd_store / k_st_bwd_store : k_bwd_generic / k_st_bwd_generic with the contraction taken out -- one workgroup per trajectory, the same
//                                  recursion operation for operation, every costate Lambda_{t+1} written to Lam[b][t]
//   k_exact_grad                 : one workgroup per (trajectory, slice), nothing sequential in t.  With A = generator / 2^s,
//                                  P = sum_{j <= D} A^j / j! (D = T, or T - 1 without squarings in state transfer) and N = 2^s sub-steps:
//                                      psi_i = P^i Psi_t,  lambda_i = (P^dagger)^(N - i) Lambda_{t+1}
//                                      dL/du_k = Re sum_{rc} E_k[r][c] M[r][c],   E_k = H_k' / 2^s
//                                      M[r][c] = sum_i sum_{a + b <= D - 1} conj(y_{i,a}[r][:]) . x_{i,b}[c][:] / (a + b + 1)!
//                                      x_{i,b} = A^b psi_{i-1},  y_{i,a} = (A^dagger)^a lambda_i
//                                  Only n x m blocks and ONE n x n accumulator are formed, never a dK matrix per control; the y chain of
//                                  sub-step i also gives lambda_{i-1}.  Every sum runs in a fixed order: two evaluations are bit-identical.
#pragma once
#include "qoc_common.h"
#include "qoc_kernels_generic.h"

#define QOC_EXACT_MAX_T 60          // 1 / (a + b + 1)! table
#define QOC_EXACT_MAX_S 12          // 2^s sub-states of a slice are kept per workgroup
#define QOC_EXACT_MREG 16           // LDS variant: n <= 64, the accumulator M lives in 16 complex registers per thread

struct QocExact {
    int on = 0;
    cplx* Lam = nullptr;            // [B][steps][n][m]: Lambda_{t+1} of every slice
    cplx* scratch = nullptr;        // per workgroup: 2^s sub-states (+ generator, accumulator and vector blocks in the global variant)
    size_t per_wg = 0;              // complex numbers of scratch per workgroup
    int grid = 0;
    int lds = 0;                    // 1: generator and vector blocks in LDS (lds_bytes of dynamic shared memory)
    size_t lds_bytes = 0;
};

// Costate sweep, unitary mode: Lambda_{t-1} = K_t^dagger Lambda_t + S_{t-1} as in k_bwd_generic, stored
__global__ void __launch_bounds__(QOC_BLOCK) k_bwd_store(QocDev d, const cplx* __restrict__ Kin, cplx* __restrict__ Lam) {
    const int b = blockIdx.x, n = d.n, m = d.m, nn = n * n, nm = n * m;
    cplx* L = Lam + (size_t)b * d.steps * nm;
    const bool need_src = d.n_forb > 0 || d.has_speed;
    wg_terminal_costate(d, b, need_src, L + (size_t)(d.steps - 1) * nm);
    __syncthreads();
    for (int t = d.steps - 1; t >= 1; --t) {
        const cplx* Kt = Kin + ((size_t)b * d.steps + t) * nn;
        const cplx* la = L + (size_t)t * nm;
        cplx* lb = L + (size_t)(t - 1) * nm;
        wg_mm<true>(n, m, n, Kt, n, la, m, lb, m);
        __syncthreads();
        if (need_src) {
            for (int o = threadIdx.x; o < nm; o += blockDim.x) lb[o] = cadd(lb[o], source_at(d, b, t, o / m, o % m));
        }
        __syncthreads();
    }
}

// Costate sweep, state transfer: lambda_t = sum_{j<T} (-B_t)^j lambda_{t+1} / j! + S_t as in k_st_bwd_generic, stored.
// scratch per trajectory: n*n (B_t) + 2*n*m.
__global__ void __launch_bounds__(QOC_BLOCK) k_st_bwd_store(QocDev d, cplx* __restrict__ scratch, cplx* __restrict__ Lam) {
    const int b = blockIdx.x, n = d.n, m = d.m, nn = n * n, nm = n * m;
    cplx* Bt = scratch + (size_t)b * (nn + 3 * nm);
    cplx* pa = Bt + nn;
    cplx* pb = pa + nm;
    cplx* L = Lam + (size_t)b * d.steps * nm;
    const bool need_src = d.n_forb > 0 || d.has_speed;
    wg_terminal_costate(d, b, need_src, L + (size_t)(d.steps - 1) * nm);
    __syncthreads();
    for (int t = d.steps - 1; t >= 1; --t) {
        const cplx* prev = L + (size_t)t * nm;
        cplx* lam = L + (size_t)(t - 1) * nm;
        wg_assemble(d, b, t, 1.0, -1.0, Bt);
        for (int o = threadIdx.x; o < nm; o += blockDim.x) { pa[o] = prev[o]; lam[o] = prev[o]; }
        __syncthreads();
        double fact = 1.0;
        for (int ii = 1; ii < d.T; ++ii) {
            wg_mm<false>(n, m, n, Bt, n, pa, m, pb, m);
            __syncthreads();
            fact *= (double)ii;
            for (int o = threadIdx.x; o < nm; o += blockDim.x) {
                cplx v = lam[o];
                v.x += pb[o].x / fact; v.y += pb[o].y / fact;
                lam[o] = v;
            }
            cplx* tmp = pa; pa = pb; pb = tmp;
            __syncthreads();
        }
        if (need_src) {
            for (int o = threadIdx.x; o < nm; o += blockDim.x) lam[o] = cadd(lam[o], source_at(d, b, t, o / m, o % m));
            __syncthreads();
        }
    }
}

// out[n x m] = A v  or  A^dagger v; A is n x n row-major, the blocks n x m row-major.  No barrier inside.
template <bool ADJ>
__device__ __forceinline__ void xg_mv(int n, int m, const cplx* __restrict__ A, const cplx* __restrict__ v, cplx* __restrict__ out) {
    const int nm = n * m;
    for (int o = threadIdx.x; o < nm; o += QOC_BLOCK) {
        const int i = o / m, j = o - i * m;
        cplx acc = cmake(0.0, 0.0);
        if (ADJ) { for (int c = 0; c < n; ++c) cfma_conj(acc, A[c * n + i], v[c * m + j]); }
        else { for (int c = 0; c < n; ++c) cfma(acc, A[i * n + c], v[c * m + j]); }
        out[o] = acc;
    }
}

// LDS = true: generator and vector blocks in dynamic LDS, M in registers (n <= 64); false: everything in the workgroup's global scratch
template <bool LDS>
__global__ void __launch_bounds__(QOC_BLOCK) k_exact_grad(QocDev d, const cplx* __restrict__ Lam, cplx* __restrict__ scratch, size_t per_wg) {
    extern __shared__ __attribute__((aligned(16))) cplx xg_lds[];
    __shared__ double red[8];
    __shared__ double ifc[QOC_EXACT_MAX_T + 2];
    const int tid = threadIdx.x, n = d.n, m = d.m, nn = n * n, nm = n * m;
    const int D = d.state_transfer ? d.T - 1 : d.T;           // degree of the slice polynomial
    const int N = 1 << d.s;                                   // sub-steps of a slice (state transfer: d.s = 0)
    const double inv_scale = 1.0 / (double)N;
    cplx* PS = scratch + (size_t)blockIdx.x * per_wg;         // [N][n][m] sub-states psi_0 .. psi_{N-1}
    cplx* work = LDS ? xg_lds : PS + (size_t)N * nm;
    cplx* A = work;                                           // [n][n]
    cplx* X = A + nn;                                         // [D][n][m]  x_b = A^b psi_{i-1}
    cplx* ya = X + (size_t)(D > 0 ? D : 1) * nm;              // y chain, ping
    cplx* yb = ya + nm;                                       //            pong
    cplx* Z = yb + nm;                                        // z_a = sum_b x_b / (a + b + 1)!
    cplx* lacc = Z + nm;                                      // lambda_{i-1} = sum_j (A^dagger)^j lambda_i / j!
    cplx* Mg = lacc + nm;                                     // [n][n] accumulator of the global variant
    if (tid == 0) {
        double f = 1.0;
        ifc[0] = 1.0;
        for (int j = 1; j <= D + 1; ++j) { f *= (double)j; ifc[j] = 1.0 / f; }
    }
    for (int item = blockIdx.x; item < d.B * d.steps; item += gridDim.x) {
        const int b = item / d.steps, t = item - b * d.steps;
        __syncthreads();                                      // (the previous item's readers of A / the table's writer)
        if (D < 1) {                                          // K = I: no control reaches the slice
            for (int kk = tid; kk < d.k; kk += QOC_BLOCK) d.dLdu[((size_t)b * d.k + kk) * d.steps + t] = 0.0;
            continue;
        }
        wg_assemble(d, b, t, inv_scale, 1.0, A);
        const cplx* psi_in = t == 0 ? d.Psi0 : d.inter + ((size_t)b * (d.steps + 1) + t) * nm;
        const cplx* lam_in = Lam + ((size_t)b * d.steps + t) * nm;
        for (int o = tid; o < nm; o += QOC_BLOCK) { PS[o] = psi_in[o]; ya[o] = lam_in[o]; }
        cplx macc[QOC_EXACT_MREG];
        if (LDS) {
#pragma unroll
            for (int e = 0; e < QOC_EXACT_MREG; ++e) macc[e] = cmake(0.0, 0.0);
        } else {
            for (int o = tid; o < nn; o += QOC_BLOCK) Mg[o] = cmake(0.0, 0.0);
        }
        __syncthreads();
        // sub-states: psi_i = sum_{j <= D} A^j psi_{i-1} / j!   (X[0], Z as the chain's ping-pong)
        for (int i = 1; i < N; ++i) {
            const cplx* src = PS + (size_t)(i - 1) * nm;
            cplx* dst = PS + (size_t)i * nm;
            cplx* pa = X;
            cplx* pb = Z;
            for (int o = tid; o < nm; o += QOC_BLOCK) { pa[o] = src[o]; dst[o] = src[o]; }
            __syncthreads();
            for (int j = 1; j <= D; ++j) {
                xg_mv<false>(n, m, A, pa, pb);
                __syncthreads();
                const double c = ifc[j];
                for (int o = tid; o < nm; o += QOC_BLOCK) {
                    cplx v = dst[o];
                    v.x = fma(pb[o].x, c, v.x); v.y = fma(pb[o].y, c, v.y);
                    dst[o] = v;
                }
                cplx* tmp = pa; pa = pb; pb = tmp;
                __syncthreads();
            }
        }
        // sub-steps from the last to the first: ya = lambda_i
        for (int i = N; i >= 1; --i) {
            const cplx* src = PS + (size_t)(i - 1) * nm;
            for (int o = tid; o < nm; o += QOC_BLOCK) { X[o] = src[o]; if (i > 1) lacc[o] = ya[o]; }
            __syncthreads();
            for (int bb = 1; bb < D; ++bb) {
                xg_mv<false>(n, m, A, X + (size_t)(bb - 1) * nm, X + (size_t)bb * nm);
                __syncthreads();
            }
            cplx* yc = ya;
            cplx* yn = yb;
            for (int a = 0; a < D; ++a) {
                for (int o = tid; o < nm; o += QOC_BLOCK) {
                    cplx z = cmake(0.0, 0.0);
                    for (int bb = 0; bb <= D - 1 - a; ++bb) {
                        const cplx x = X[(size_t)bb * nm + o];
                        const double c = ifc[a + bb + 1];
                        z.x = fma(x.x, c, z.x); z.y = fma(x.y, c, z.y);
                    }
                    Z[o] = z;
                }
                __syncthreads();
                // M[r][c] += sum_j conj(y_a[r][j]) z_a[c][j]
                if (LDS) {
#pragma unroll
                    for (int e = 0; e < QOC_EXACT_MREG; ++e) {
                        const int o = tid + e * QOC_BLOCK;
                        if (o < nn) {
                            const int r = o / n, c = o - r * n;
                            cplx acc = macc[e];
                            for (int j = 0; j < m; ++j) cfma_conj(acc, yc[r * m + j], Z[c * m + j]);
                            macc[e] = acc;
                        }
                    }
                } else {
                    for (int o = tid; o < nn; o += QOC_BLOCK) {
                        const int r = o / n, c = o - r * n;
                        cplx acc = Mg[o];
                        for (int j = 0; j < m; ++j) cfma_conj(acc, yc[r * m + j], Z[c * m + j]);
                        Mg[o] = acc;
                    }
                }
                // y_{a+1} = A^dagger y_a: for the next term, and (i > 1) for lambda_{i-1}, which needs every power up to D
                if (a + 1 < D || i > 1) {
                    xg_mv<true>(n, m, A, yc, yn);
                    __syncthreads();
                    if (i > 1) {
                        const double c = ifc[a + 1];
                        for (int o = tid; o < nm; o += QOC_BLOCK) {
                            cplx v = lacc[o];
                            v.x = fma(yn[o].x, c, v.x); v.y = fma(yn[o].y, c, v.y);
                            lacc[o] = v;
                        }
                    }
                    cplx* tmp = yc; yc = yn; yn = tmp;
                }
                __syncthreads();
            }
            if (i > 1) {
                for (int o = tid; o < nm; o += QOC_BLOCK) ya[o] = lacc[o];
                __syncthreads();
            }
        }
        // dL/du_k = Re sum_rc E_k[r][c] M[r][c]
        for (int kk = 0; kk < d.k; ++kk) {
            const cplx* Hk = d.Hs + (size_t)(kk + 1) * nn;
            double part = 0.0;
            if (LDS) {
#pragma unroll
                for (int e = 0; e < QOC_EXACT_MREG; ++e) {
                    const int o = tid + e * QOC_BLOCK;
                    if (o < nn) { const cplx h = Hk[o]; part = fma(h.x, macc[e].x, part); part = fma(-h.y, macc[e].y, part); }
                }
            } else {
                for (int o = tid; o < nn; o += QOC_BLOCK) { const cplx h = Hk[o], mv = Mg[o]; part = fma(h.x, mv.x, part); part = fma(-h.y, mv.y, part); }
            }
            const double g = block_sum(part, red);
            if (tid == 0) d.dLdu[((size_t)b * d.k + kk) * d.steps + t] = g * inv_scale;
        }
    }
}

// complex numbers of vector blocks + generator (+ accumulator: global variant) behind the sub-states
static inline size_t qoc_exact_work(const QocDev& d, bool with_M) {
    const size_t nn = (size_t)d.n * d.n, nm = (size_t)d.n * d.m;
    const int D = d.state_transfer ? d.T - 1 : d.T;
    return nn + (size_t)((D > 0 ? D : 1) + 4) * nm + (with_M ? nn : 0);
}

// Sizes of an exact engine; the caller allocates Lam and scratch.  Returns a message on a shape the kernel does not take.
static inline const char* qoc_exact_plan(QocExact& x, const QocDev& d) {
    if (d.T > QOC_EXACT_MAX_T) return "the exact gradient needs taylor_terms <= 60";
    if (d.s > QOC_EXACT_MAX_S) return "the exact gradient needs scaling <= 12";
    const size_t nm = (size_t)d.n * d.m, N = (size_t)1 << d.s;
    const size_t lds_bytes = qoc_exact_work(d, false) * sizeof(cplx);
    // 160 KiB of LDS per compute unit; the static part (reduction slots, factorial table) stays below 1 KiB
    x.lds = d.n <= 64 && lds_bytes <= (size_t)159 * 1024 ? 1 : 0;
    x.lds_bytes = x.lds ? lds_bytes : 0;
    x.per_wg = N * nm + (x.lds ? 0 : qoc_exact_work(d, true));
    long long grid = (long long)d.B * d.steps;
    if (grid > 2048) grid = 2048;
    const size_t budget = (size_t)1 << 28;                   // of scratch, in bytes
    const size_t fit = budget / (x.per_wg * sizeof(cplx));
    if ((size_t)grid > fit) grid = fit < 1 ? 1 : (long long)fit;
    x.grid = (int)grid;
    x.on = 1;
    return nullptr;
}

static inline hipError_t qoc_exact_lds_opt_in(const QocExact& x) {
    if (!x.lds || x.lds_bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute((const void*)k_exact_grad<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)x.lds_bytes);
}

// the backward half of an exact engine's iteration: storing sweep, then the slice-parallel gradient
static inline void qoc_exact_backward(const QocExact& x, const QocDev& d, const cplx* K, cplx* seed_scratch, hipStream_t s) {
    if (!d.state_transfer) hipLaunchKernelGGL(k_bwd_store, dim3(d.B), dim3(QOC_BLOCK), 0, s, d, K, x.Lam);
    else hipLaunchKernelGGL(k_st_bwd_store, dim3(d.B), dim3(QOC_BLOCK), 0, s, d, seed_scratch, x.Lam);
    if (x.lds) hipLaunchKernelGGL(k_exact_grad<true>, dim3(x.grid), dim3(QOC_BLOCK), x.lds_bytes, s, d, x.Lam, x.scratch, x.per_wg);
    else hipLaunchKernelGGL(k_exact_grad<false>, dim3(x.grid), dim3(QOC_BLOCK), 0, s, d, x.Lam, x.scratch, x.per_wg);
}
