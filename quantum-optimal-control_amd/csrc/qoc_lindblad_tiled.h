// qoc_lindblad_tiled.h -- open-system GRAPE past the LDS rule of qoc_lindblad.h (QOC_PATH_LINDBLAD_TILED): 1 <= n <= 128, any c <= 8.
// The mathematics is that of qoc_lindblad.h, term for term (its header comment has the formulas): the slice map with its N = 2^s sub-steps and its
// ascending Taylor sum, A_t in lb_assemble's order, the dissipator sum scaled by 1 / N before A X + X A^dagger is added, pairs i <= j with weights 1
// and 2, Lambda(T), the first-order gradient, member rows and running costs.  What differs is where the operators live and what multiplies them.
//
// Layout.  NP = 16 ceil(n / 16).  A workgroup (one per (control set, pair), as there) owns QOC_LBT_MATS = 5 matrices of NP x NP complex numbers in
// global scratch, W.work[B R][5][NP][NP] -- 1.25 MiB at NP = 128, resident in L2: A_t / N, the operator, the running Taylor term, the next term and one
// temporary (X D^dagger).  The next term needs a home of its own here: the LDS kernels keep it in four registers per thread, and 16 tiles per wave at
// NP = 128 do not fit in registers.  The collapse operators come from a padded table W.Dp[rows][c][NP][NP], scaled per member row by sqrt(s_j) on the
// host (the product lb_setup forms on the way into LDS).  hist, partial, pop and expct keep the unpadded layouts, so k_lb_reduce, k_lb_populations
// and k_lb_expectations run on this path as they are.
//
// Pads.  The scratch comes uninitialised.  Every matrix is written in full -- pad rows and columns as zeros -- before it is first read: the operator
// and A_t by the elementwise loops below (which run over all NP x NP elements), the history's rho likewise, every product by its own tiles; the
// table of D_j is padded on the host.  A product of zero-padded operands has zero pads, so they stay zero.
//
// Products.  An NP x NP complex product is formed tile by tile with v_mfma_f64_16x16x4_f64: lane l holds A[row l & 15][k = l >> 4] and
// B[k = l >> 4][col l & 15], and of the result C[row (l >> 4) + 4 reg][col l & 15].  The NP^2 / 256 tiles are dealt over the four waves (tile tl to
// wave tl mod 4), one tile at a time: four real products in four independent accumulators (re re, im im, re im, im re), combined when the tile is
// done.  X A^dagger, X D^dagger, A^dagger Y and D^dagger Y read the same arrays with swapped indices and the sign of the imaginary part turned:
// there are no transposed copies.  Every elementwise step uses the result layout too, so a thread reads back what it wrote itself wherever the
// step before was elementwise or a product, and everything else is behind __syncthreads().  All accesses to the scratch are plain loads and stores.
//
// Gradient.  Once per slice G^dagger = Lambda rho^dagger + Lambda^dagger rho (two products, into the running term's place, which is free between
// slices), then dL/du_k = weight Re sum_ab conj(H_k'[a][b]) G^dagger[a][b] -- the sum Re <Lambda, H_k' rho + rho H_k'^dagger> of qoc_lindblad.h --
// as k block reductions over elements each thread wrote itself.
// Every sum runs in a fixed order and nothing is accumulated with atomics: two evaluations are bit-identical (with the LDS path they agree to rounding).
#pragma once
#include "qoc_lindblad.h"
#include "qoc_mfma_frag.h"

#define QOC_LBT_MAX_N 128
#define QOC_LBT_MATS 5
#define QOC_LBT_WAVES (QOC_BLOCK / 64)

struct QocLbt {
    int on, NP;
    size_t work_bytes;
    cplx* work;                     // [B R][QOC_LBT_MATS][NP][NP]
    const cplx* Dp;                 // [rows][c][NP][NP] sqrt(s_j) D_j, zero padded
};

static inline int qoc_lbt_np(int n) { return 16 * ((n + 15) / 16); }

struct LbtAcc { d4 rr, ii, ri, ir; };
__device__ __forceinline__ LbtAcc lbt_zero() {
    LbtAcc a;
    a.rr = a.ii = a.ri = a.ir = d4{0.0, 0.0, 0.0, 0.0};
    return a;
}

// acc += op(P)[tile row I][:] op(Q)[:][tile column J]; LH: op(P) = P^dagger, RH: op(Q) = Q^dagger
template <bool LH, bool RH>
__device__ __forceinline__ void lbt_mac(LbtAcc& acc, const cplx* P, const cplx* Q, int I, int J, int NP) {
    const int lr = threadIdx.x & 15, lq = (threadIdx.x & 63) >> 4;
    const cplx* pl = LH ? P + (size_t)lq * NP + 16 * I + lr : P + (size_t)(16 * I + lr) * NP + lq;
    const cplx* pr = RH ? Q + (size_t)(16 * J + lr) * NP + lq : Q + (size_t)lq * NP + 16 * J + lr;
    const int sl = LH ? 4 * NP : 4, sr = RH ? 4 : 4 * NP;
#pragma unroll 4
    for (int p = 0; p < NP; p += 4) {
        const cplx a = *pl, b = *pr;
        pl += sl; pr += sr;
        const double ai = LH ? -a.y : a.y, bi = RH ? -b.y : b.y;
        acc.rr = QMFMA(a.x, b.x, acc.rr);
        acc.ii = QMFMA(ai, bi, acc.ii);
        acc.ri = QMFMA(a.x, bi, acc.ri);
        acc.ir = QMFMA(ai, b.x, acc.ir);
    }
}

// f(I, J) for every tile of this wave
template <typename F>
__device__ __forceinline__ void lbt_tiles(int NP, F f) {
    const int nt = NP >> 4;
    for (int tl = threadIdx.x >> 6; tl < nt * nt; tl += QOC_LBT_WAVES) {
        const int I = tl / nt;
        f(I, tl - I * nt);
    }
}
// row, column of element reg of tile (I, J) in this lane (the result layout of the matrix instruction)
__device__ __forceinline__ int lbt_row(int I, int reg) { return 16 * I + ((threadIdx.x & 63) >> 4) + 4 * reg; }
__device__ __forceinline__ int lbt_col(int J) { return 16 * J + (threadIdx.x & 15); }
// f(row, column, offset row NP + column) for every element of this thread, pads included
template <typename F>
__device__ __forceinline__ void lbt_each(int NP, F f) {
    lbt_tiles(NP, [&](int I, int J) {
        const int col = lbt_col(J);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = lbt_row(I, reg);
            f(row, col, row * NP + col);
        }
    });
}

// A = (H0eff + sum_k u_k[t] H_k') / N, pads zero (lb_assemble's sum, in its order)
__device__ __forceinline__ void lbt_assemble(const QocDev& d, const cplx* __restrict__ H0, int b, int t, double inv_n, int NP, cplx* A) {
    const int n = d.n, nn = n * n;
    const double* ub = d.u + (size_t)b * d.k * d.steps + t;
    lbt_each(NP, [&](int row, int col, int at) {
        cplx acc = cmake(0.0, 0.0);
        if (row < n && col < n) {
            const int o = row * n + col;
            acc = cscale(H0[o], inv_n);
            for (int kk = 0; kk < d.k; ++kk) {
                const double c = ub[(size_t)kk * d.steps] * inv_n;
                const cplx h = d.Hs[(size_t)(kk + 1) * nn + o];
                acc.x = fma(c, h.x, acc.x);
                acc.y = fma(c, h.y, acc.y);
            }
        }
        A[at] = acc;
    });
}

// the five matrices of a workgroup
struct LbtMats { cplx *A, *X, *term, *next, *tmp; };
__device__ __forceinline__ LbtMats lbt_carve(const QocLbt& W) {
    const size_t mat = (size_t)W.NP * W.NP;
    LbtMats s;
    s.A = W.work + (size_t)blockIdx.x * QOC_LBT_MATS * mat;
    s.X = s.A + mat; s.term = s.X + mat; s.next = s.term + mat; s.tmp = s.next + mat;
    return s;
}
__device__ __forceinline__ void lbt_factorials(int T, double* ifc) {
    if (threadIdx.x == 0) {
        double f = 1.0;
        ifc[0] = 1.0;
        for (int j = 1; j <= T; ++j) { f *= (double)j; ifc[j] = 1.0 / f; }
    }
}

// One slice: N sub-steps X <- sum_{j <= T} (L / N)^j X / j! (ADJ: L^dagger), in place.  A holds A_t / N, D the (scaled, padded) D_j; s.term and
// s.next change places with every term.  Enters behind the writes of A and X without a barrier (the first one below orders them); leaves behind one.
template <bool ADJ>
__device__ __forceinline__ void lbt_slice(int NP, int c, int T, int N, double inv_n, const cplx* D, LbtMats& s, const double* ifc) {
    const size_t mat = (size_t)NP * NP;
    for (int sub = 0; sub < N; ++sub) {
        lbt_each(NP, [&](int, int, int at) { s.term[at] = s.X[at]; });
        __syncthreads();
        for (int jt = 1; jt <= T; ++jt) {
            const double cj = ifc[jt];
            // (1 / N) v + A X + X A^dagger (ADJ: A^dagger Y + Y A) into the next term, and its share into the operator
            auto finish = [&](int I, int J, d4 vr, d4 vi) {
                LbtAcc a = lbt_zero();
                if (ADJ) { lbt_mac<true, false>(a, s.A, s.term, I, J, NP); lbt_mac<false, false>(a, s.term, s.A, I, J, NP); }
                else { lbt_mac<false, false>(a, s.A, s.term, I, J, NP); lbt_mac<false, true>(a, s.term, s.A, I, J, NP); }
                const int col = lbt_col(J);
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int at = lbt_row(I, reg) * NP + col;
                    cplx v = cmake(vr[reg] * inv_n + (a.rr[reg] - a.ii[reg]), vi[reg] * inv_n + (a.ri[reg] + a.ir[reg]));
                    s.next[at] = v;
                    cplx x = s.X[at];
                    x.x = fma(v.x, cj, x.x); x.y = fma(v.y, cj, x.y);
                    s.X[at] = x;
                }
            };
            for (int q = 0; q < c; ++q) {
                const cplx* Dq = D + (size_t)q * mat;
                // tmp = X D_q^dagger (ADJ: Y D_q)
                lbt_tiles(NP, [&](int I, int J) {
                    LbtAcc a = lbt_zero();
                    lbt_mac<false, !ADJ>(a, s.term, Dq, I, J, NP);
                    const int col = lbt_col(J);
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) s.tmp[lbt_row(I, reg) * NP + col] = cmake(a.rr[reg] - a.ii[reg], a.ri[reg] + a.ir[reg]);
                });
                __syncthreads();
                // next += D_q tmp (ADJ: D_q^dagger tmp), q ascending; the last q goes on to A X + X A^dagger
                lbt_tiles(NP, [&](int I, int J) {
                    LbtAcc a = lbt_zero();
                    lbt_mac<ADJ, false>(a, Dq, s.tmp, I, J, NP);
                    const int col = lbt_col(J);
                    d4 vr = a.rr - a.ii, vi = a.ri + a.ir;
                    if (q > 0) {
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) {
                            const cplx o = s.next[lbt_row(I, reg) * NP + col];
                            vr[reg] = o.x + vr[reg]; vi[reg] = o.y + vi[reg];
                        }
                    }
                    if (q == c - 1) { finish(I, J, vr, vi); return; }
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) s.next[lbt_row(I, reg) * NP + col] = cmake(vr[reg], vi[reg]);
                });
                __syncthreads();
            }
            if (c == 0) {
                lbt_tiles(NP, [&](int I, int J) { finish(I, J, d4{0.0, 0.0, 0.0, 0.0}, d4{0.0, 0.0, 0.0, 0.0}); });
                __syncthreads();
            }
            cplx* sw = s.term; s.term = s.next; s.next = sw;
        }
    }
}

// ROWS: the engine has a row per member (qoc_create_open_fleet), as in k_lb_forward
template <bool ROWS>
__global__ void __launch_bounds__(QOC_BLOCK) k_lbt_forward(QocDev d, QocLb L, QocLbt W) {
    __shared__ double ifc[QOC_LB_MAX_T + 2];
    const int b = blockIdx.x / L.R, r = blockIdx.x - b * L.R;
    if (d.skip_done && d.done[b]) return;
    const int n = d.n, m = d.m, nn = n * n, N = 1 << d.s, NP = W.NP;
    const double inv_n = 1.0 / (double)N;
    const int row = ROWS ? lb_row(L, b) : 0;
    const cplx* H0 = L.H0 + (size_t)row * nn;
    const cplx* D = W.Dp + (size_t)row * L.c * NP * NP;
    LbtMats s = lbt_carve(W);
    lbt_factorials(d.T, ifc);
    int pi, pj;
    lb_pair(r, m, pi, pj);
    // rho_ij(0) = psi_i psi_j^dagger
    lbt_each(NP, [&](int a, int c, int at) {
        s.X[at] = a < n && c < n ? cmul(d.Psi0[a * m + pi], cconj(d.Psi0[c * m + pj])) : cmake(0.0, 0.0);
    });
    cplx* hist = L.hist + ((size_t)b * L.R + r) * d.steps * nn;
    for (int t = 0; t < d.steps; ++t) {
        lbt_assemble(d, H0, b, t, inv_n, NP, s.A);
        lbt_slice<false>(NP, L.c, d.T, N, inv_n, D, s, ifc);
        lbt_each(NP, [&](int a, int c, int at) {
            if (a < n && c < n) hist[(size_t)t * nn + a * n + c] = s.X[at];
        });
    }
}

// COSTS: the running costs of a diagonal pair, as in k_lb_backward
template <bool ROWS, bool COSTS = false>
__global__ void __launch_bounds__(QOC_BLOCK) k_lbt_backward(QocDev d, QocLb L, QocLbt W) {
    __shared__ double ifc[QOC_LB_MAX_T + 2];
    __shared__ double red[8];
    const int b = blockIdx.x / L.R, r = blockIdx.x - b * L.R;
    if (d.skip_done && d.done[b]) return;
    const int n = d.n, m = d.m, nn = n * n, N = 1 << d.s, NP = W.NP;
    const double inv_n = 1.0 / (double)N;
    const int row = ROWS ? lb_row(L, b) : 0;
    const cplx* H0 = L.H0 + (size_t)row * nn;
    const cplx* D = W.Dp + (size_t)row * L.c * NP * NP;
    LbtMats s = lbt_carve(W);
    lbt_factorials(d.T, ifc);
    int pi, pj;
    lb_pair(r, m, pi, pj);
    const double weight = pi == pj ? 1.0 : 2.0, c0 = -1.0 / ((double)m * (double)m);
    // Lambda_ij(T) = -w_i w_j^dagger / m^2
    lbt_each(NP, [&](int a, int c, int at) {
        s.X[at] = a < n && c < n ? cscale(cmul(d.W[a * m + pi], cconj(d.W[c * m + pj])), c0) : cmake(0.0, 0.0);
    });
    const cplx* hist = L.hist + ((size_t)b * L.R + r) * d.steps * nn;
    double* part_out = L.partial + ((size_t)b * L.R + r) * d.k * d.steps;
    double cost = 0.0;
    for (int t = d.steps - 1; t >= 0; --t) {
        cplx* rho = s.tmp;
        cplx* G = s.term;
        lbt_each(NP, [&](int a, int c, int at) {
            rho[at] = a < n && c < n ? hist[(size_t)t * nn + a * n + c] : cmake(0.0, 0.0);
        });
        if (COSTS && pi == pj) {
            // x = Re <O_l, rho_ii(t+1)>; Lambda_ii(t+1) += a_l x^(p_l - 1) O_l, both on the thread's own elements
            for (int l = 0; l < L.nc; ++l) {
                const cplx* O = L.cO + (size_t)l * nn;
                double part = 0.0;
                lbt_each(NP, [&](int a, int c, int at) {
                    if (a < n && c < n) { const cplx ov = O[a * n + c], rv = rho[at]; part += ov.x * rv.x + ov.y * rv.y; }
                });
                const double x = block_sum(part, red);
                const double ca = L.ca[l];
                const bool sq = L.cp[l] == 2;
                const double f = sq ? ca * x : ca;
                cost += sq ? 0.5 * (ca * x * x) : ca * x;
                lbt_each(NP, [&](int a, int c, int at) {
                    if (a < n && c < n) {
                        const cplx ov = O[a * n + c];
                        cplx lam = s.X[at];
                        lam.x = fma(f, ov.x, lam.x); lam.y = fma(f, ov.y, lam.y);
                        s.X[at] = lam;
                    }
                });
            }
        }
        __syncthreads();                                      // rho and Lambda are whole
        // G^dagger = Lambda rho^dagger + Lambda^dagger rho
        lbt_tiles(NP, [&](int I, int J) {
            LbtAcc a = lbt_zero();
            lbt_mac<false, true>(a, s.X, rho, I, J, NP);
            lbt_mac<true, false>(a, s.X, rho, I, J, NP);
            const int col = lbt_col(J);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) G[lbt_row(I, reg) * NP + col] = cmake(a.rr[reg] - a.ii[reg], a.ri[reg] + a.ir[reg]);
        });
        // weight Re sum_ab conj(H_k'[a][b]) G^dagger[a][b]
        for (int kk = 0; kk < d.k; ++kk) {
            const cplx* Hk = d.Hs + (size_t)(kk + 1) * nn;
            double part = 0.0;
            lbt_each(NP, [&](int a, int c, int at) {
                if (a < n && c < n) { const cplx h = Hk[a * n + c], g = G[at]; part += h.x * g.x + h.y * g.y; }
            });
            const double g = block_sum(part, red);
            if (threadIdx.x == 0) part_out[(size_t)kk * d.steps + t] = weight * g;
        }
        __syncthreads();                                      // (k = 0 never happens; kept for the readers of rho all the same)
        lbt_assemble(d, H0, b, t, inv_n, NP, s.A);
        lbt_slice<true>(NP, L.c, d.T, N, inv_n, D, s, ifc);
    }
    if (COSTS && pi == pj && threadIdx.x == 0) L.cost_partial[(size_t)b * L.R + r] = cost;
}

// the three launches of an open engine's evaluation on this path (the reduction is k_lb_reduce itself)
static inline void qoc_lbt_forward(const QocLb& L, const QocLbt& W, const QocDev& d, hipStream_t s) {
    if (qoc_lb_member_rows(L)) hipLaunchKernelGGL(k_lbt_forward<true>, dim3((unsigned)(d.B * L.R)), dim3(QOC_BLOCK), 0, s, d, L, W);
    else hipLaunchKernelGGL(k_lbt_forward<false>, dim3((unsigned)(d.B * L.R)), dim3(QOC_BLOCK), 0, s, d, L, W);
}
static inline void qoc_lbt_backward(const QocLb& L, const QocLbt& W, const QocDev& d, hipStream_t s) {
    if (L.nc > 0) {
        if (qoc_lb_member_rows(L)) hipLaunchKernelGGL((k_lbt_backward<true, true>), dim3((unsigned)(d.B * L.R)), dim3(QOC_BLOCK), 0, s, d, L, W);
        else hipLaunchKernelGGL((k_lbt_backward<false, true>), dim3((unsigned)(d.B * L.R)), dim3(QOC_BLOCK), 0, s, d, L, W);
        hipLaunchKernelGGL(k_lb_reduce<true>, dim3((unsigned)d.B), dim3(QOC_BLOCK), 0, s, d, L);
        return;
    }
    if (qoc_lb_member_rows(L)) hipLaunchKernelGGL(k_lbt_backward<true>, dim3((unsigned)(d.B * L.R)), dim3(QOC_BLOCK), 0, s, d, L, W);
    else hipLaunchKernelGGL(k_lbt_backward<false>, dim3((unsigned)(d.B * L.R)), dim3(QOC_BLOCK), 0, s, d, L, W);
    hipLaunchKernelGGL(k_lb_reduce<false>, dim3((unsigned)d.B), dim3(QOC_BLOCK), 0, s, d, L);
}
