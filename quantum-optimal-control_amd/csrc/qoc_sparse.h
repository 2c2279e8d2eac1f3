// qoc_sparse.h -- sparse state transfer (qoc_create_sparse, QOC_PATH_SPARSE): the reference's matvecexp_op sweeps (core/tensorflow_state.py:77-133) on
// operators that are never dense.  The reference has sparse_H / sparse_U / sparse_K for systems built from Kronecker products and switches them off under
// use_gpu ("GPU Sparse Matmul is not supported yet", main_grape/grape.py:28-32); here they get kernels of their own.
//
// Storage: each of the k + 1 operators A_j = -i dt H_j in ELLPACK, slot-major (csrc/qoc_sparse_host.h): col[slot][r], val[slot][r], width W_j of its
// own; neighbouring threads own neighbouring rows, so the loads of a slot coalesce.  A product is y = sum_j c_j (A_j x) with c_0 = 1, c_j = u_j[t]
// (the costate sweep: all of them negated); no union pattern and no assembled generator exist anywhere.
//
//   k_sp_forward   one workgroup per (control set, state column), sequential in t: psi_{t+1} = sum_{j<T} B_t^j psi_t / j!.  The running Taylor term lives in
//                  one of two vectors (ping-pong: term j is read from one and term j + 1 written to the other, gathered as x[col]), the sum accumulates in
//                  place in d.inter[b][t+1] by the thread that owns the row, as k_st_fwd_generic does.  One barrier per term: with two vectors nobody can
//                  still read the vector that the next term overwrites once everybody has passed the barrier behind the previous term.
//   k_sp_backward  the same layout, t descending: lam_t = sum_{j<T} (-B_t)^j lam_{t+1} / j! + S_t, the terminal costate as wg_terminal_costate forms it.
//                  lam_{t+1} of every slice is stored to Lam[b][t]; the sum accumulates there in place.  No contraction inside the sequential sweep.
//   k_sp_grad      one workgroup per (control set, slice), grid-stride: dL/du[k, t] = Re sum_{r, column} conj(lam_{t+1}[r]) (A_k psi_{t+1})[r], A_k from its
//                  own ELL, psi gathered from d.inter.  Nothing sequential in t (the contractions cost more inside a sweep than a launch).
// Where the two vectors live (QocSparse::home): in LDS while 2 n 16 B <= 159 KiB (n <= 5088), above that in the workgroup's block of global scratch --
// the same code through a pointer, as k_exact_grad has its two variants.  Every sum runs in a fixed order, there is no atomic: two evaluations are
// bit-identical, and so are the two homes.
#pragma once
#include "qoc_common.h"
#include "qoc_state_source.h"

#define QOC_SP_MAX_T 60
#define QOC_SP_LDS_LIMIT ((size_t)159 * 1024)     // of the 160 KiB per compute unit; the sweeps have no static LDS
// A sweep's workgroup has 256 threads up to this many rows (one row per thread and term) and 1024 above.  Measured on XX chains of 200 slices, ms per
// iteration with 256 / 1024 threads (tools/sparse_bench.py threads, profiles/sparse_state_transfer.txt): n = 64 1.574 / 1.577, n = 256 3.118 / 3.121,
// n = 512 6.33 / 3.71, n = 1024 13.49 / 4.69, n = 4096 59.3 / 19.2, n = 16384 924 / 306 -- level while every row has a thread, 1024 ahead as soon as
// 256 threads would take a second pass over the rows.
#define QOC_SP_WIDE_FROM 256
// What row_layout = 0 (auto) of qoc_create_sparse_fleet resolves to for an engine of n levels and `operators` = kt + q + 1 operators: 1 = merged rows.
// Measured on XX chains of 200 slices, one control set, E = 1 / E = 8 members, ms per iteration per-operator -> merged (tools/sparse_bench.py ensemble,
// the two engines timed alternately, six windows each; the windows of one engine lie within 0.2 ms of each other; profiles/sparse_ensemble.txt):
//   n =   64   3 operators  1.585 -> 2.208 /  1.608 -> 2.282        8 operators   3.008 ->  3.423 /  3.066 ->  3.526
//   n =  256   3 operators  3.109 -> 4.797 /  3.239 -> 4.893       10 operators   6.489 ->  7.862 /  6.617 ->  8.107
//   n = 1024   3 operators  4.670 -> 6.145 /  4.773 -> 6.269       12 operators  10.787 -> 10.386 / 10.930 -> 10.609
//   n = 4096   3 operators 19.208 -> 24.79 / 19.509 -> 25.21       14 operators  49.143 -> 43.114 / 49.734 -> 44.053
// Merged is ahead by more than the spread on every measured row with n >= 1024 and 12 or more operators (3.7 % and 12 %), and behind on every other
// row: with few operators a row's walk is one dependent chain of decode, compare and FMA where the per-operator loops run under uniform trip counts,
// and below n = 1024 the sweeps are bound by the k + 1 passes' latency less than by that chain.  So auto is merged exactly in that class, per-operator
// everywhere else, and merged stays a switch (row_layout = 2) there.  Nothing between 3 and 12 operators was measured at n >= 1024.
#define QOC_SP_MERGED_AUTO_N 1024
#define QOC_SP_MERGED_AUTO_OPS 12
#define QOC_SP_MERGED_AUTO(n, operators) ((n) >= QOC_SP_MERGED_AUTO_N && (operators) >= QOC_SP_MERGED_AUTO_OPS)

struct QocSparse {
    int on;
    int home;                       // 1: the two vectors of a sweep in LDS, 2: in global scratch
    int threads;                    // of a sweep's workgroup: 256 or 1024
    int grad_grid;
    size_t lds_bytes;               // dynamic LDS of a sweep (0 with the vectors in global scratch)
    long long stored;               // entries of all operators (padding not counted)
    const int* W;                   // [k+1] width of operator j
    const long long* off;           // [k+1] where its [W_j][n] block starts in col / val
    const int* col;
    const cplx* val;
    cplx* Lam;                      // [B][steps][n][m]: lam_{t+1} of every slice
    cplx* scratch;                  // [B m][2][n] (home 2)
    int kgrad;                      // controls k_sp_grad forms a gradient for: d.k, or kt on an ensemble engine (the frozen perturbation rows have no reader)
    // the merged layout (qoc_create_sparse_fleet, row_layout = 2; csrc/qoc_sparse_host.h: qoc_ell_merge), else merged = 0 and the rest null
    int merged;
    int Wm;                         // longest merged row
    size_t tab_bytes;               // the coefficient table of a merged sweep in LDS: 8 B per operator, rounded up to 16 B
    const int* mlen;                // [n] slots of row r
    const int* midx;                // [Wm][n] col | op << 24
    const cplx* mval;               // [Wm][n]
};

// (A_j x)[r]: the slots in ascending order.  (Eight slots in flight per trip -- columns and values first, then the gathers, then the FMAs -- were measured
// and lost: 2.21 against 1.57 ms per iteration at n = 64, 10.4 against 4.7 at n = 1024, 37.1 against 19.2 at n = 4096; the widths here are 1 to 13, and a
// trip of eight re-reads the last slot for the ones an operator does not have.  profiles/sparse_state_transfer.txt, section 5)
__device__ __forceinline__ cplx sp_row(const QocSparse& sp, int j, int n, int r, const cplx* __restrict__ x) {
    const int W = sp.W[j];
    const int* __restrict__ c = sp.col + sp.off[j] + r;
    const cplx* __restrict__ v = sp.val + sp.off[j] + r;
    cplx acc = cmake(0.0, 0.0);
    for (int s = 0; s < W; ++s) cfma(acc, v[(size_t)s * n], x[c[(size_t)s * n]]);
    return acc;
}

// (sum_j c_j A_j x)[r] from the merged list of row r (QocSparse::midx): ONE walk over the row's stored entries of all operators, in the arithmetic
// order of the per-operator loop in sp_chain -- within an operator cfma over its slots in ascending column into a partial sum that starts at +0; when the
// operator index changes the partial sum joins y as that loop joins it (operator 0: cscale by the sign, the others: two explicit fma with the
// coefficient).  What the old layout adds and this one does not: a padding slot's 0 * x[r] on a sum that started at +0 (no change for finite x), and an
// absent operator's fma(c, 0, y) (at most -0 -> +0).  So the two layouts agree under == on every output.  ctab: c_0 = sign, c_j = sign u_j[t], in LDS.
__device__ __forceinline__ cplx sp_row_merged(const QocSparse& sp, int n, int r, const cplx* __restrict__ x, const double* __restrict__ ctab, double sign) {
    const int len = sp.mlen[r];
    const int* __restrict__ ix = sp.midx + r;
    const cplx* __restrict__ v = sp.mval + r;
    cplx y = cmake(0.0, 0.0), z = cmake(0.0, 0.0);
    int cur = 0;
    for (int s = 0; s < len; ++s) {
        const unsigned pk = (unsigned)ix[(size_t)s * n];
        const int op = (int)(pk >> 24);
        if (op != cur) {
            if (cur == 0) y = cscale(z, sign);
            else { const double c = ctab[cur]; y.x = fma(c, z.x, y.x); y.y = fma(c, z.y, y.y); }
            cur = op;
            z = cmake(0.0, 0.0);
        }
        cfma(z, v[(size_t)s * n], x[pk & 0xffffffu]);
    }
    if (cur == 0) y = cscale(z, sign);
    else { const double c = ctab[cur]; y.x = fma(c, z.x, y.x); y.y = fma(c, z.y, y.y); }
    return y;
}

// One Taylor chain on column j of a state block: `acc` (global, row stride m) holds the chain's start vector and receives sum_{ii < T} (sign B_t)^ii start / ii!
// MERGED: the rows from the merged list, the slice's coefficients staged once into ctab (LDS, d.k + 1 entries) in front of the barrier behind the load of
// xa -- nobody still reads the previous slice's table there: its last term ended at a barrier (T = 1: the table is never read)
template <bool MERGED>
__device__ __forceinline__ void sp_chain(const QocDev& d, const QocSparse& sp, const double* __restrict__ ut, double sign, cplx* __restrict__ acc,
                                         cplx*& xa, cplx*& xb, double* ctab) {
    const int n = d.n, m = d.m;
    for (int r = threadIdx.x; r < n; r += blockDim.x) xa[r] = acc[(size_t)r * m];
    if (MERGED)
        for (int j = threadIdx.x; j <= d.k; j += blockDim.x) ctab[j] = j == 0 ? sign : sign * ut[(size_t)(j - 1) * d.steps];
    __syncthreads();
    double fact = 1.0;
    for (int ii = 1; ii < d.T; ++ii) {
        fact *= (double)ii;
        for (int r = threadIdx.x; r < n; r += blockDim.x) {
            cplx y;
            if (MERGED) y = sp_row_merged(sp, n, r, xa, ctab, sign);
            else {
                y = cscale(sp_row(sp, 0, n, r, xa), sign);
                for (int kk = 0; kk < d.k; ++kk) {
                    const double c = sign * ut[(size_t)kk * d.steps];
                    const cplx z = sp_row(sp, kk + 1, n, r, xa);
                    y.x = fma(c, z.x, y.x);
                    y.y = fma(c, z.y, y.y);
                }
            }
            xb[r] = y;
            cplx v = acc[(size_t)r * m];
            v.x += y.x / fact; v.y += y.y / fact;
            acc[(size_t)r * m] = v;
        }
        __syncthreads();
        cplx* tmp = xa; xa = xb; xb = tmp;
    }
}

// (MERGED: the coefficient table stands behind the two vectors when they live in LDS, alone in LDS when they live in global scratch)
template <bool LDS, bool MERGED = false>
__global__ void __launch_bounds__(1024) k_sp_forward(QocDev d, QocSparse sp) {
    extern __shared__ __attribute__((aligned(16))) cplx sp_lds[];
    const int b = blockIdx.x / d.m, j = blockIdx.x - b * d.m, n = d.n, m = d.m;
    if (d.skip_done && d.done[b]) return;
    cplx* xa = LDS ? sp_lds : sp.scratch + (size_t)blockIdx.x * 2 * n;
    cplx* xb = xa + n;
    double* ctab = MERGED ? (double*)(sp_lds + (LDS ? 2 * (size_t)n : 0)) : nullptr;
    const size_t nm = (size_t)n * m;
    cplx* iv = d.inter + (size_t)b * (d.steps + 1) * nm + j;
    for (int r = threadIdx.x; r < n; r += blockDim.x) iv[(size_t)r * m] = d.V[(size_t)r * m + j];
    const double* ub = d.u + (size_t)b * d.k * d.steps;
    for (int t = 0; t < d.steps; ++t) {
        const cplx* psi = iv + (size_t)t * nm;
        cplx* out = iv + (size_t)(t + 1) * nm;
        for (int r = threadIdx.x; r < n; r += blockDim.x) out[(size_t)r * m] = psi[(size_t)r * m];      // (each thread: the rows it owns, here and in the chain)
        sp_chain<MERGED>(d, sp, ub + t, 1.0, out, xa, xb, ctab);
    }
}

template <bool LDS, bool MERGED = false>
__global__ void __launch_bounds__(1024) k_sp_backward(QocDev d, QocSparse sp) {
    extern __shared__ __attribute__((aligned(16))) cplx sp_lds[];
    const int b = blockIdx.x / d.m, j = blockIdx.x - b * d.m, n = d.n, m = d.m;
    if (d.skip_done && d.done[b]) return;
    cplx* xa = LDS ? sp_lds : sp.scratch + (size_t)blockIdx.x * 2 * n;
    cplx* xb = xa + n;
    double* ctab = MERGED ? (double*)(sp_lds + (LDS ? 2 * (size_t)n : 0)) : nullptr;
    const size_t nm = (size_t)n * m;
    cplx* L = sp.Lam + (size_t)b * d.steps * nm + j;
    const bool need_src = d.n_forb > 0 || d.has_speed;
    const double* ub = d.u + (size_t)b * d.k * d.steps;
    {   // lam_N = (-2 / m^2) z W + S_N                          (wg_terminal_costate, this column)
        const cplx z = d.zfin[b];
        const double c0 = -2.0 / ((double)m * (double)m);
        cplx* last = L + (size_t)(d.steps - 1) * nm;
        for (int r = threadIdx.x; r < n; r += blockDim.x) {
            cplx v = cscale(cmul(z, d.W[(size_t)r * m + j]), c0);
            if (need_src) v = cadd(v, source_at(d, b, d.steps, r, j));
            last[(size_t)r * m] = v;
        }
    }
    for (int t = d.steps - 1; t >= 1; --t) {
        const cplx* prev = L + (size_t)t * nm;
        cplx* lam = L + (size_t)(t - 1) * nm;
        for (int r = threadIdx.x; r < n; r += blockDim.x) lam[(size_t)r * m] = prev[(size_t)r * m];
        sp_chain<MERGED>(d, sp, ub + t, -1.0, lam, xa, xb, ctab);
        if (need_src)
            for (int r = threadIdx.x; r < n; r += blockDim.x) lam[(size_t)r * m] = cadd(lam[(size_t)r * m], source_at(d, b, t, r, j));
    }
}

__global__ void __launch_bounds__(QOC_BLOCK) k_sp_grad(QocDev d, QocSparse sp) {
    __shared__ double red[8];
    const int n = d.n, m = d.m, nm = n * m;
    for (int item = blockIdx.x; item < d.B * d.steps; item += gridDim.x) {
        const int b = item / d.steps, t = item - b * d.steps;
        if (d.skip_done && d.done[b]) continue;
        const cplx* lam = sp.Lam + ((size_t)b * d.steps + t) * nm;
        const cplx* psi = d.inter + ((size_t)b * (d.steps + 1) + t + 1) * nm;
        for (int kk = 0; kk < sp.kgrad; ++kk) {
            const int W = sp.W[kk + 1];
            const int* __restrict__ c = sp.col + sp.off[kk + 1];
            const cplx* __restrict__ v = sp.val + sp.off[kk + 1];
            double part = 0.0;
            for (int o = threadIdx.x; o < nm; o += QOC_BLOCK) {
                const int r = o / m, j = o - r * m;
                cplx y = cmake(0.0, 0.0);
                for (int s = 0; s < W; ++s) cfma(y, v[(size_t)s * n + r], psi[(size_t)c[(size_t)s * n + r] * m + j]);
                part += lam[o].x * y.x + lam[o].y * y.y;                  // Re(conj(lam) * y)
            }
            const double g = block_sum(part, red);
            if (threadIdx.x == 0) d.dLdu[((size_t)b * d.k + kk) * d.steps + t] = g;
        }
    }
}

// the coefficient table of a merged sweep: a double per operator, rounded up to the vectors' 16 B; the largest n whose two vectors fit LDS beside `tab` bytes
static inline size_t qoc_sp_tab_bytes(int operators) { return ((size_t)operators * sizeof(double) + 15) & ~(size_t)15; }
static inline int qoc_sp_lds_max_n(size_t tab) { return (int)((QOC_SP_LDS_LIMIT - tab) / (2 * sizeof(cplx))); }

// home and sizes of a sparse engine (vector_home: 0 auto, 1 LDS, 2 global scratch); a message when LDS is asked for and does not fit.  merged: the sweeps
// walk the merged list of `operators` operators, whose coefficient table lives in LDS in both homes and moves the boundary of the LDS home down from
// n = 5088 to qoc_sp_lds_max_n (5087 for up to 4 operators, 5024 for 255)
static inline const char* qoc_sp_plan(QocSparse& sp, const QocDev& d, int vector_home, int threads, bool merged = false, int operators = 0) {
    static thread_local char msg[160];
    sp.merged = merged ? 1 : 0;
    sp.tab_bytes = merged ? qoc_sp_tab_bytes(operators) : 0;
    const size_t need = 2 * (size_t)d.n * sizeof(cplx) + sp.tab_bytes;
    if (vector_home == 1 && need > QOC_SP_LDS_LIMIT) {
        if (!merged) return "vector_home = 1 (LDS) needs 2 n 16 bytes <= 159 KiB (n <= 5088)";
        snprintf(msg, sizeof msg, "vector_home = 1 (LDS) needs 2 n 16 bytes + %zu bytes of coefficients <= 159 KiB (n <= %d with %d merged operators)",
                 sp.tab_bytes, qoc_sp_lds_max_n(sp.tab_bytes), operators);
        return msg;
    }
    sp.home = vector_home ? vector_home : (need <= QOC_SP_LDS_LIMIT ? 1 : 2);
    sp.lds_bytes = sp.home == 1 ? need : sp.tab_bytes;
    sp.threads = threads ? threads : (d.n > QOC_SP_WIDE_FROM ? 1024 : 256);
    long long grid = (long long)d.B * d.steps;
    sp.grad_grid = (int)(grid > 2048 ? 2048 : grid);
    sp.kgrad = d.k;
    sp.on = 1;
    return nullptr;
}

// Above 64 KiB of dynamic LDS a kernel has to be opted in: to the size rule's limit, never to this engine's own footprint (qoc_lb_lds_opt_in: the attribute
// belongs to the kernel for the whole process, and a smaller value would lower it under a larger engine that is still alive)
static inline hipError_t qoc_sp_lds_opt_in(const QocSparse& sp) {
    if (sp.lds_bytes <= 64 * 1024) return hipSuccess;
    const void* fwd = sp.merged ? (const void*)k_sp_forward<true, true> : (const void*)k_sp_forward<true>;
    const void* bwd = sp.merged ? (const void*)k_sp_backward<true, true> : (const void*)k_sp_backward<true>;
    const hipError_t e = hipFuncSetAttribute(fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)QOC_SP_LDS_LIMIT);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)QOC_SP_LDS_LIMIT);
}

static inline void qoc_sp_forward(const QocSparse& sp, const QocDev& d, hipStream_t s) {
    const dim3 grid((unsigned)(d.B * d.m)), block((unsigned)sp.threads);
    if (sp.merged) {
        if (sp.home == 1) hipLaunchKernelGGL((k_sp_forward<true, true>), grid, block, sp.lds_bytes, s, d, sp);
        else hipLaunchKernelGGL((k_sp_forward<false, true>), grid, block, sp.lds_bytes, s, d, sp);
    } else if (sp.home == 1) hipLaunchKernelGGL(k_sp_forward<true>, grid, block, sp.lds_bytes, s, d, sp);
    else hipLaunchKernelGGL(k_sp_forward<false>, grid, block, 0, s, d, sp);
}
static inline void qoc_sp_backward(const QocSparse& sp, const QocDev& d, hipStream_t s) {
    const dim3 grid((unsigned)(d.B * d.m)), block((unsigned)sp.threads);
    if (sp.merged) {
        if (sp.home == 1) hipLaunchKernelGGL((k_sp_backward<true, true>), grid, block, sp.lds_bytes, s, d, sp);
        else hipLaunchKernelGGL((k_sp_backward<false, true>), grid, block, sp.lds_bytes, s, d, sp);
    } else if (sp.home == 1) hipLaunchKernelGGL(k_sp_backward<true>, grid, block, sp.lds_bytes, s, d, sp);
    else hipLaunchKernelGGL(k_sp_backward<false>, grid, block, 0, s, d, sp);
    hipLaunchKernelGGL(k_sp_grad, dim3((unsigned)sp.grad_grid), dim3(QOC_BLOCK), 0, s, d, sp);
}
