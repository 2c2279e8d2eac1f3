// qoc_lindblad.h -- open-system GRAPE (qoc_create_open, QOC_PATH_LINDBLAD): the pulse is scored and optimised under a Lindblad master equation.
// The reference has no counterpart (its graph propagates state vectors: core/tensorflow_state.py:209-256).
//
// With H' = -i dt H as in d.Hs and collapse operators D_j = sqrt(dt) C_j (the square root of the rate inside C_j):
//     A_t      = H0' + sum_k u_k[t] H_k' - 1/2 sum_j D_j^dagger D_j
//     L_t(X)   = A_t X + X A_t^dagger + sum_j D_j X D_j^dagger               L_t^dagger(Y) = A_t^dagger Y + Y A_t + sum_j D_j^dagger Y D_j
// Slice map (both modes): N = 2^s sub-steps, each X <- sum_{j = 0 .. T} (L_t / N)^j X / j!, the terms formed as a chain X_j = (L_t / N) X_{j-1}
// and summed in ascending j.  The operators rho_ij(0) = psi_i psi_j^dagger of the m states of interest are propagated for the pairs i <= j only
// (R = m (m + 1) / 2: rho_ji = rho_ij^dagger) and scored against sigma_ij = w_i w_j^dagger:
//     loss          = 1 - (1 / m^2) sum_ij Re Tr(sigma_ij^dagger rho_ij(T))        (no collapse operator: the closed engine's 1 - |sum_i <w_i|psi_i>|^2 / m^2)
//     unitary_scale = (1 / m) sum_i Re Tr rho_ii(T)                                (1 for a trace-preserving map)
//     dL/du[k, t]   = sum_pairs weight Re <Lambda(t+1), H_k' rho(t+1) + rho(t+1) H_k'^dagger>,  Lambda_ij(T) = -sigma_ij / m^2, Lambda(t) the adjoint
//                     slice map (the same series in L_t^dagger) of Lambda(t+1); weight 1 on the diagonal pairs, 2 off it -- first order in dt, as
//                     the reference's gradient is
//
//   k_lb_forward  : one workgroup per (control set, pair), sequential in t; rho(t+1) of every slice to hist[B][R][steps][n][n]
//   k_lb_backward : the same layout, t descending: k block reductions per slice into partial[B][R][k][steps], then the adjoint slice map
//   k_lb_reduce   : one workgroup per control set: the partials summed over the pairs in ascending pair order into d.dLdu, loss, unitary_scale
//                   and a zero reg_state -- what k_loss and the backward sweep leave behind on the closed paths, so that the tail runs unchanged
// Every sum runs in a fixed order and nothing is accumulated with atomics: two evaluations are bit-identical.
//
// LDS (dynamic): A_t, the c matrices D_j, the operator, the running Taylor term and one temporary -- c + 4 matrices of n rows; a thread owns up
// to four elements of the next term and keeps them in registers until every thread has read the running one.  X A^dagger and X D^dagger read
// rows of BOTH operands, so the lanes of a 16-lane ds_read_b128 group (consecutive columns j of the result) read rows j of the right operand: with
// a row stride of n complex numbers these are n * 16 bytes apart, and at n = 32 (512 bytes = two bank rows) all sixteen fall on the same four
// banks.  The row stride is therefore S = n | 1 complex numbers: S odd makes 4 S mod 64 an odd multiple of 4, so sixteen consecutive rows start on
// sixteen different 16-byte slots of the 256-byte bank row.  (c + 4) n S 16 bytes <= 159 KiB with n <= 32, c <= 8, m <= n; no global-memory variant.
//
// Decay per member (qoc_create_open_fleet): the trajectories of an ensemble or fleet engine share the operators D_j and differ in their rates.  Member e of
// device f has the collapse operators sqrt(s[f][e][j]) D_j, so two tables of F E rows stand where one drift stood: H0[row] = H0' - 1/2 sum_j s_j D_j^dagger D_j
// (formed on the host) and rs[row][j] = sqrt(s_j), which lb_setup multiplies into D_j on its way into LDS.  Trajectory b reads row ((b / E) / Rs) E + b % E
// (E members, Rs control sets per device: the member block of qoc_ensemble.h).  An engine of qoc_create_open has one row and no rs: nothing is scaled.
//
// Running costs (qoc_create_open_costs): nc observables O_l with coefficients a_l (already divided by steps) and powers p_l in {1, 2} put
//     R = sum_l a_l sum_{tau = 0 .. steps} sum_{i < m} x_l,i(tau)^p_l / p_l,    x_l,i(tau) = Re sum_ac conj(O_l[a][c]) rho_ii(tau)[a][c]
// into reg_state.  Only the COSTS instances of k_lb_backward and k_lb_reduce know of them: the workgroup of a diagonal pair (i, i) forms x_l,i(t+1) from
// the operator it has just loaded (one block_sum per observable, O_l read from global memory: no LDS), adds a_l x^(p_l - 1) O_l to its own elements of
// Lambda_ii(t+1) BEFORE the slice's contraction -- once per slice, not per sub-step -- and leaves its share of R in cost_partial[B][R]; k_lb_reduce<true>
// adds the tau = 0 terms from Psi0 (value only: the start does not depend on the pulse) and the partials of the diagonal pairs in ascending pair order.
// Off-diagonal pairs run what they always ran.  The instances without COSTS are the kernels of every engine that has no costs.
#pragma once
#include "qoc_common.h"

#define QOC_LB_MAX_N 32
#define QOC_LB_MAX_C 8
#define QOC_LB_MAX_T 60             // 1 / j! table
#define QOC_LB_MAX_S 12
#define QOC_LB_MAX_COSTS 16
#define QOC_LB_E 4                  // elements of an n x n operator per thread: 32 * 32 / QOC_BLOCK
#define QOC_LB_LDS_LIMIT ((size_t)159 * 1024)     // of the 160 KiB per compute unit; the static part (reduction slots, 1 / j! table) stays below 1 KiB

struct QocLb {
    int on, c, R, S;                // collapse operators, pairs i <= j, LDS row stride in complex numbers
    size_t lds_bytes;
    const cplx* D;                  // [c][n][n] sqrt(dt) C_j at rate scale 1
    const cplx* H0;                 // [rows][n][n] the drift H0' - 1/2 sum_j s_j D_j^dagger D_j
    cplx* hist;                     // [B][R][steps][n][n] rho(t+1) of the last evaluation
    double* partial;                // [B][R][k][steps] a pair's share of dL/du
    double* pop;                    // [B][steps+1][n][m] populations (formed on read-back)
    // the member axis, behind what a one-row engine reads
    const double* rs;               // [rows][c] sqrt(s_j), or null: every scale is 1 and D_j is copied as it is
    int E, Rs, rows;                // members per control set, control sets per device, rows of H0 and rs (F E; 1: qoc_create_open)
    // running costs (qoc_create_open_costs), read by the COSTS instances only
    int nc;                         // observables, 0 .. QOC_LB_MAX_COSTS
    const cplx* cO;                 // [nc][n][n] row-major
    const double* ca;               // [nc] a_l / steps
    const int* cp;                  // [nc] 1 or 2
    double* cost_partial;           // [B][R] a pair's share of R over tau = 1 .. steps (diagonal pairs only)
    double* expct;                  // [B][steps+1][nc][m] x_l,i(tau) (formed on read-back)
};

static inline int qoc_lb_stride(int n) { return n | 1; }
static inline size_t qoc_lb_lds_bytes(int n, int c) { return (size_t)(c + 4) * n * qoc_lb_stride(n) * sizeof(cplx); }

// pair r of the list (0,0) (0,1) .. (0,m-1) (1,1) ..
__device__ __forceinline__ void lb_pair(int r, int m, int& i, int& j) {
    i = 0;
    while (r >= m - i) { r -= m - i; ++i; }
    j = i + r;
}

// the elements of an n x n operator this thread owns: o = tid + e * QOC_BLOCK, as LDS offsets row * S + column (-1: none)
struct LbOwn { int row[QOC_LB_E], col[QOC_LB_E], at[QOC_LB_E]; };
__device__ __forceinline__ LbOwn lb_own(int n, int S) {
    LbOwn w;
#pragma unroll
    for (int e = 0; e < QOC_LB_E; ++e) {
        const int o = threadIdx.x + e * QOC_BLOCK;
        const bool ok = o < n * n;
        w.row[e] = ok ? o / n : 0;
        w.col[e] = ok ? o - w.row[e] * n : 0;
        w.at[e] = ok ? w.row[e] * S + w.col[e] : -1;
    }
    return w;
}

// the row of L.H0 and L.rs that trajectory b reads
__device__ __forceinline__ int lb_row(const QocLb& L, int b) {
    const int g = b / L.E;
    return (g / L.Rs) * L.E + (b - g * L.E);
}

// A = (H0eff + sum_k u_k[t] H_k') / N into LDS rows of stride S (wg_assemble's sum, in its order)
__device__ __forceinline__ void lb_assemble(const QocDev& d, const QocLb& L, const cplx* __restrict__ H0, int b, int t, double inv_n, const LbOwn& w,
                                            cplx* __restrict__ A) {
    const int nn = d.n * d.n;
    const double* ub = d.u + (size_t)b * d.k * d.steps + t;
#pragma unroll
    for (int e = 0; e < QOC_LB_E; ++e) {
        if (w.at[e] < 0) continue;
        const int o = threadIdx.x + e * QOC_BLOCK;
        cplx acc = cscale(H0[o], inv_n);
        for (int kk = 0; kk < d.k; ++kk) {
            const double c = ub[(size_t)kk * d.steps] * inv_n;
            const cplx h = d.Hs[(size_t)(kk + 1) * nn + o];
            acc.x = fma(c, h.x, acc.x);
            acc.y = fma(c, h.y, acc.y);
        }
        A[w.at[e]] = acc;
    }
}

// One slice: N sub-steps X <- sum_{j <= T} (L / N)^j X / j! (ADJ: L^dagger), in place in LDS.  A holds A_t / N, D the unscaled D_j.
// Enters behind the writes of A and X without a barrier (the first one below orders them); leaves behind a barrier.
template <bool ADJ>
__device__ __forceinline__ void lb_slice(int n, int S, int c, int T, int N, double inv_n, const LbOwn& w, const cplx* __restrict__ A,
                                         const cplx* __restrict__ D, cplx* __restrict__ X, cplx* __restrict__ term, cplx* __restrict__ tmp,
                                         const double* __restrict__ ifc) {
    for (int sub = 0; sub < N; ++sub) {
#pragma unroll
        for (int e = 0; e < QOC_LB_E; ++e)
            if (w.at[e] >= 0) term[w.at[e]] = X[w.at[e]];
        __syncthreads();
        for (int jt = 1; jt <= T; ++jt) {
            cplx acc[QOC_LB_E];
#pragma unroll
            for (int e = 0; e < QOC_LB_E; ++e) acc[e] = cmake(0.0, 0.0);
            for (int q = 0; q < c; ++q) {
                const cplx* Dq = D + (size_t)q * n * S;
                // tmp = X D_q^dagger (ADJ: Y D_q)
#pragma unroll
                for (int e = 0; e < QOC_LB_E; ++e) {
                    if (w.at[e] < 0) continue;
                    const cplx* xr = term + w.row[e] * S;
                    cplx v = cmake(0.0, 0.0);
                    if (ADJ) { for (int p = 0; p < n; ++p) cfma(v, xr[p], Dq[p * S + w.col[e]]); }
                    else { const cplx* dr = Dq + w.col[e] * S; for (int p = 0; p < n; ++p) cfma_conj(v, dr[p], xr[p]); }
                    tmp[w.at[e]] = v;
                }
                __syncthreads();
                // acc += D_q tmp (ADJ: D_q^dagger tmp)
#pragma unroll
                for (int e = 0; e < QOC_LB_E; ++e) {
                    if (w.at[e] < 0) continue;
                    cplx v = acc[e];
                    if (ADJ) { for (int p = 0; p < n; ++p) cfma_conj(v, Dq[p * S + w.row[e]], tmp[p * S + w.col[e]]); }
                    else { const cplx* dr = Dq + w.row[e] * S; for (int p = 0; p < n; ++p) cfma(v, dr[p], tmp[p * S + w.col[e]]); }
                    acc[e] = v;
                }
                __syncthreads();
            }
            // (1 / N) sum_q ..., then A X + X A^dagger (ADJ: A^dagger Y + Y A) with A = A_t / N
#pragma unroll
            for (int e = 0; e < QOC_LB_E; ++e) {
                if (w.at[e] < 0) continue;
                cplx v = cscale(acc[e], inv_n);
                const cplx* xr = term + w.row[e] * S;
                if (ADJ) {
                    for (int p = 0; p < n; ++p) cfma_conj(v, A[p * S + w.row[e]], term[p * S + w.col[e]]);
                    for (int p = 0; p < n; ++p) cfma(v, xr[p], A[p * S + w.col[e]]);
                } else {
                    const cplx* ar = A + w.row[e] * S;
                    const cplx* ac = A + w.col[e] * S;
                    for (int p = 0; p < n; ++p) cfma(v, ar[p], term[p * S + w.col[e]]);
                    for (int p = 0; p < n; ++p) cfma_conj(v, ac[p], xr[p]);
                }
                acc[e] = v;
            }
            __syncthreads();                                  // every reader of the running term is done
            const double cj = ifc[jt];
#pragma unroll
            for (int e = 0; e < QOC_LB_E; ++e) {
                if (w.at[e] < 0) continue;
                term[w.at[e]] = acc[e];
                cplx x = X[w.at[e]];
                x.x = fma(acc[e].x, cj, x.x); x.y = fma(acc[e].y, cj, x.y);
                X[w.at[e]] = x;
            }
            __syncthreads();
        }
    }
}

// what both sweeps set up: the 1 / j! table, the LDS carve-up, D_j (times the row's sqrt(s_j) where there is a table) into LDS
struct LbLds { cplx *A, *D, *X, *term, *tmp; };
template <bool ROWS>
__device__ __forceinline__ LbLds lb_setup(const QocDev& d, const QocLb& L, int row, cplx* lds, double* ifc) {
    const int n = d.n, S = L.S, mat = n * S;
    LbLds s;
    s.A = lds; s.D = s.A + mat; s.X = s.D + (size_t)L.c * mat; s.term = s.X + mat; s.tmp = s.term + mat;
    if (threadIdx.x == 0) {
        double f = 1.0;
        ifc[0] = 1.0;
        for (int j = 1; j <= d.T; ++j) { f *= (double)j; ifc[j] = 1.0 / f; }
    }
    for (int o = threadIdx.x; o < L.c * n * n; o += QOC_BLOCK) {
        const int q = o / (n * n), rc = o - q * n * n, r = rc / n;
        cplx v = L.D[o];
        if (ROWS && L.rs) v = cscale(v, L.rs[(size_t)row * L.c + q]);
        s.D[(size_t)q * mat + r * S + (rc - r * n)] = v;
    }
    return s;
}

// ROWS: the engine has a row per member (qoc_create_open_fleet); false is the one-row engine of qoc_create_open, whose sweeps read L.H0 and
// L.D as they are -- the kernels it always ran
template <bool ROWS>
__global__ void __launch_bounds__(QOC_BLOCK) k_lb_forward(QocDev d, QocLb L) {
    extern __shared__ __attribute__((aligned(16))) cplx lb_lds[];
    __shared__ double ifc[QOC_LB_MAX_T + 2];
    const int b = blockIdx.x / L.R, r = blockIdx.x - b * L.R;
    if (d.skip_done && d.done[b]) return;
    const int n = d.n, m = d.m, nn = n * n, N = 1 << d.s;
    const double inv_n = 1.0 / (double)N;
    const LbOwn w = lb_own(n, L.S);
    const int row = ROWS ? lb_row(L, b) : 0;
    const cplx* H0 = ROWS ? L.H0 + (size_t)row * nn : L.H0;
    const LbLds s = lb_setup<ROWS>(d, L, row, lb_lds, ifc);
    int pi, pj;
    lb_pair(r, m, pi, pj);
    // rho_ij(0) = psi_i psi_j^dagger
#pragma unroll
    for (int e = 0; e < QOC_LB_E; ++e)
        if (w.at[e] >= 0) s.X[w.at[e]] = cmul(d.Psi0[w.row[e] * m + pi], cconj(d.Psi0[w.col[e] * m + pj]));
    cplx* hist = L.hist + ((size_t)b * L.R + r) * d.steps * nn;
    for (int t = 0; t < d.steps; ++t) {
        lb_assemble(d, L, H0, b, t, inv_n, w, s.A);
        lb_slice<false>(n, L.S, L.c, d.T, N, inv_n, w, s.A, s.D, s.X, s.term, s.tmp, ifc);
#pragma unroll
        for (int e = 0; e < QOC_LB_E; ++e)
            if (w.at[e] >= 0) hist[(size_t)t * nn + threadIdx.x + e * QOC_BLOCK] = s.X[w.at[e]];
    }
}

// COSTS: the running costs of a diagonal pair -- sources on Lambda_ii(t+1) and the pair's share of R
template <bool ROWS, bool COSTS = false>
__global__ void __launch_bounds__(QOC_BLOCK) k_lb_backward(QocDev d, QocLb L) {
    extern __shared__ __attribute__((aligned(16))) cplx lb_lds[];
    __shared__ double ifc[QOC_LB_MAX_T + 2];
    __shared__ double red[8];
    const int b = blockIdx.x / L.R, r = blockIdx.x - b * L.R;
    if (d.skip_done && d.done[b]) return;
    const int n = d.n, m = d.m, nn = n * n, N = 1 << d.s, S = L.S;
    const double inv_n = 1.0 / (double)N;
    const LbOwn w = lb_own(n, S);
    const int row = ROWS ? lb_row(L, b) : 0;
    const cplx* H0 = ROWS ? L.H0 + (size_t)row * nn : L.H0;
    const LbLds s = lb_setup<ROWS>(d, L, row, lb_lds, ifc);
    int pi, pj;
    lb_pair(r, m, pi, pj);
    const double weight = pi == pj ? 1.0 : 2.0, c0 = -1.0 / ((double)m * (double)m);
    // Lambda_ij(T) = -w_i w_j^dagger / m^2
#pragma unroll
    for (int e = 0; e < QOC_LB_E; ++e)
        if (w.at[e] >= 0) s.X[w.at[e]] = cscale(cmul(d.W[w.row[e] * m + pi], cconj(d.W[w.col[e] * m + pj])), c0);
    const cplx* hist = L.hist + ((size_t)b * L.R + r) * d.steps * nn;
    double* part_out = L.partial + ((size_t)b * L.R + r) * d.k * d.steps;
    cplx* rho = s.tmp;
    double cost = 0.0;
    for (int t = d.steps - 1; t >= 0; --t) {
#pragma unroll
        for (int e = 0; e < QOC_LB_E; ++e)
            if (w.at[e] >= 0) rho[w.at[e]] = hist[(size_t)t * nn + threadIdx.x + e * QOC_BLOCK];
        __syncthreads();
        if (COSTS && pi == pj) {
            // x = Re <O_l, rho_ii(t+1)>; Lambda_ii(t+1) += a_l x^(p_l - 1) O_l on the thread's own elements (the contraction below reads only those)
            for (int l = 0; l < L.nc; ++l) {
                const cplx* O = L.cO + (size_t)l * nn;
                double part = 0.0;
#pragma unroll
                for (int e = 0; e < QOC_LB_E; ++e) {
                    if (w.at[e] < 0) continue;
                    const cplx ov = O[threadIdx.x + e * QOC_BLOCK], rv = rho[w.at[e]];
                    part += ov.x * rv.x + ov.y * rv.y;
                }
                const double x = block_sum(part, red);
                const double a = L.ca[l];
                const bool sq = L.cp[l] == 2;
                const double f = sq ? a * x : a;
                cost += sq ? 0.5 * (a * x * x) : a * x;
#pragma unroll
                for (int e = 0; e < QOC_LB_E; ++e) {
                    if (w.at[e] < 0) continue;
                    const cplx ov = O[threadIdx.x + e * QOC_BLOCK];         // (read again, from L2: four registers per element are dearer)
                    cplx lam = s.X[w.at[e]];
                    lam.x = fma(f, ov.x, lam.x); lam.y = fma(f, ov.y, lam.y);
                    s.X[w.at[e]] = lam;
                }
            }
        }
        // weight Re <Lambda(t+1), H_k' rho(t+1) + rho(t+1) H_k'^dagger>
        for (int kk = 0; kk < d.k; ++kk) {
            const cplx* Hk = d.Hs + (size_t)(kk + 1) * nn;
            double part = 0.0;
#pragma unroll
            for (int e = 0; e < QOC_LB_E; ++e) {
                if (w.at[e] < 0) continue;
                const cplx* hr = Hk + w.row[e] * n;
                const cplx* hc = Hk + w.col[e] * n;
                const cplx* xr = rho + w.row[e] * S;
                cplx y = cmake(0.0, 0.0);
                for (int p = 0; p < n; ++p) cfma(y, hr[p], rho[p * S + w.col[e]]);
                for (int p = 0; p < n; ++p) cfma_conj(y, hc[p], xr[p]);
                const cplx lam = s.X[w.at[e]];
                part += lam.x * y.x + lam.y * y.y;
            }
            const double g = block_sum(part, red);
            if (threadIdx.x == 0) part_out[(size_t)kk * d.steps + t] = weight * g;
        }
        __syncthreads();                                      // (k = 0 never happens; the readers of rho are behind block_sum's barriers)
        lb_assemble(d, L, H0, b, t, inv_n, w, s.A);
        lb_slice<true>(n, S, L.c, d.T, N, inv_n, w, s.A, s.D, s.X, s.term, s.tmp, ifc);
    }
    if (COSTS && pi == pj && threadIdx.x == 0) L.cost_partial[(size_t)b * L.R + r] = cost;
}

// d.dLdu = sum over the pairs, ascending; loss, unitary_scale, reg_state = 0 from the final operators
// COSTS: reg_state = the tau = 0 terms of the running costs from Psi0 (l ascending, i ascending inside), then the diagonal pairs' partials, ascending
template <bool COSTS = false>
__global__ void __launch_bounds__(QOC_BLOCK) k_lb_reduce(QocDev d, QocLb L) {
    __shared__ double red[8];
    const int b = blockIdx.x;
    if (d.skip_done && d.done[b]) return;
    const int n = d.n, m = d.m, nn = n * n, ks = d.k * d.steps;
    for (int o = threadIdx.x; o < ks; o += QOC_BLOCK) {
        const double* p = L.partial + (size_t)b * L.R * ks + o;
        double acc = p[0];
        for (int r = 1; r < L.R; ++r) acc += p[(size_t)r * ks];
        d.dLdu[(size_t)b * ks + o] = acc;
    }
    double fid = 0.0, tr = 0.0;
    for (int idx = threadIdx.x; idx < L.R * nn; idx += QOC_BLOCK) {
        const int r = idx / nn, o = idx - r * nn, a = o / n, c = o - a * n;
        int pi, pj;
        lb_pair(r, m, pi, pj);
        const cplx rho = L.hist[(((size_t)b * L.R + r) * d.steps + (d.steps - 1)) * nn + o];
        // Re(conj(sigma_ac) rho_ac), sigma_ac = w_i[a] conj(w_j[c])
        const cplx sg = cmul(d.W[a * m + pi], cconj(d.W[c * m + pj]));
        fid += (pi == pj ? 1.0 : 2.0) * (sg.x * rho.x + sg.y * rho.y);
        if (pi == pj && a == c) tr += rho.x;
    }
    fid = block_sum(fid, red);
    tr = block_sum(tr, red);
    double reg = 0.0;
    if (COSTS) {
        for (int l = 0; l < L.nc; ++l) {
            const cplx* O = L.cO + (size_t)l * nn;
            const double a = L.ca[l];
            const bool sq = L.cp[l] == 2;
            for (int i = 0; i < m; ++i) {
                double part = 0.0;
                for (int o = threadIdx.x; o < nn; o += QOC_BLOCK) {
                    const int a_ = o / n, c = o - a_ * n;
                    const cplx rv = cmul(d.Psi0[a_ * m + i], cconj(d.Psi0[c * m + i]));
                    part += O[o].x * rv.x + O[o].y * rv.y;
                }
                const double x = block_sum(part, red);
                reg += sq ? 0.5 * (a * x * x) : a * x;
            }
        }
        for (int i = 0, r = 0; i < m; r += m - i, ++i) reg += L.cost_partial[(size_t)b * L.R + r];
    }
    if (threadIdx.x == 0) {
        d.loss[b] = 1.0 - fid / ((double)m * (double)m);
        d.uscale[b] = tr / (double)m;
        d.reg_state[b] = reg;
    }
}

// read-back: pop[b][tau][l][i] = Re rho_ii(tau)[l][l], tau = 0 the start
__global__ void __launch_bounds__(QOC_BLOCK) k_lb_populations(QocDev d, QocLb L) {
    const int n = d.n, m = d.m, nn = n * n;
    const size_t total = (size_t)d.B * (d.steps + 1) * n * m;
    for (size_t o = (size_t)blockIdx.x * QOC_BLOCK + threadIdx.x; o < total; o += (size_t)gridDim.x * QOC_BLOCK) {
        const int i = (int)(o % m), l = (int)((o / m) % n), tau = (int)((o / ((size_t)m * n)) % (d.steps + 1));
        const size_t b = o / ((size_t)m * n * (d.steps + 1));
        int r = 0;                                            // the diagonal pair (i, i)
        for (int q = 0; q < i; ++q) r += m - q;
        double v;
        if (tau == 0) { const cplx p = d.Psi0[l * m + i]; v = p.x * p.x + p.y * p.y; }
        else v = L.hist[((b * L.R + r) * d.steps + (tau - 1)) * nn + (size_t)l * n + l].x;
        L.pop[o] = v;
    }
}

// read-back: expct[b][tau][l][i] = Re <O_l, rho_ii(tau)>, tau = 0 the start; one workgroup per (b, tau), the elements summed in a fixed order
__global__ void __launch_bounds__(QOC_BLOCK) k_lb_expectations(QocDev d, QocLb L) {
    __shared__ double red[8];
    const int n = d.n, m = d.m, nn = n * n;
    const int tau = blockIdx.x % (d.steps + 1);
    const size_t b = blockIdx.x / (d.steps + 1);
    for (int l = 0; l < L.nc; ++l) {
        const cplx* O = L.cO + (size_t)l * nn;
        for (int i = 0, r = 0; i < m; r += m - i, ++i) {          // r: the diagonal pair (i, i)
            double part = 0.0;
            for (int o = threadIdx.x; o < nn; o += QOC_BLOCK) {
                cplx rv;
                if (tau == 0) { const int a = o / n, c = o - a * n; rv = cmul(d.Psi0[a * m + i], cconj(d.Psi0[c * m + i])); }
                else rv = L.hist[((b * L.R + r) * d.steps + (tau - 1)) * nn + o];
                part += O[o].x * rv.x + O[o].y * rv.y;
            }
            const double x = block_sum(part, red);
            if (threadIdx.x == 0) L.expct[((b * (d.steps + 1) + tau) * L.nc + l) * m + i] = x;
        }
    }
}

// whether the engine has member rows to pick and scale by (one row of scales counts: a single member whose rates are not the nominal ones)
static inline bool qoc_lb_member_rows(const QocLb& L) { return L.rows > 1 || L.rs != nullptr; }
// the three launches of an open engine's evaluation
static inline void qoc_lb_forward(const QocLb& L, const QocDev& d, hipStream_t s) {
    if (qoc_lb_member_rows(L)) hipLaunchKernelGGL(k_lb_forward<true>, dim3((unsigned)(d.B * L.R)), dim3(QOC_BLOCK), L.lds_bytes, s, d, L);
    else hipLaunchKernelGGL(k_lb_forward<false>, dim3((unsigned)(d.B * L.R)), dim3(QOC_BLOCK), L.lds_bytes, s, d, L);
}
static inline void qoc_lb_backward(const QocLb& L, const QocDev& d, hipStream_t s) {
    if (L.nc > 0) {                                           // running costs: the COSTS instances of the sweep and of the reduction
        if (qoc_lb_member_rows(L)) hipLaunchKernelGGL((k_lb_backward<true, true>), dim3((unsigned)(d.B * L.R)), dim3(QOC_BLOCK), L.lds_bytes, s, d, L);
        else hipLaunchKernelGGL((k_lb_backward<false, true>), dim3((unsigned)(d.B * L.R)), dim3(QOC_BLOCK), L.lds_bytes, s, d, L);
        hipLaunchKernelGGL(k_lb_reduce<true>, dim3((unsigned)d.B), dim3(QOC_BLOCK), 0, s, d, L);
        return;
    }
    if (qoc_lb_member_rows(L)) hipLaunchKernelGGL(k_lb_backward<true>, dim3((unsigned)(d.B * L.R)), dim3(QOC_BLOCK), L.lds_bytes, s, d, L);
    else hipLaunchKernelGGL(k_lb_backward<false>, dim3((unsigned)(d.B * L.R)), dim3(QOC_BLOCK), L.lds_bytes, s, d, L);
    hipLaunchKernelGGL(k_lb_reduce<false>, dim3((unsigned)d.B), dim3(QOC_BLOCK), 0, s, d, L);
}
// Above 64 KiB of dynamic LDS a kernel has to be opted in.  The attribute belongs to the kernel for the whole process, not to an engine, so it is
// set to the size rule's limit -- never to this engine's own footprint, which would lower it under a larger open engine that is still alive.
static inline hipError_t qoc_lb_lds_opt_in(const QocLb& L) {
    if (L.lds_bytes <= 64 * 1024) return hipSuccess;
    const void* kernels[] = {(const void*)k_lb_forward<false>, (const void*)k_lb_backward<false>, (const void*)k_lb_forward<true>, (const void*)k_lb_backward<true>,
                             (const void*)k_lb_backward<false, true>, (const void*)k_lb_backward<true, true>};
    for (const void* f : kernels) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)QOC_LB_LDS_LIMIT);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
