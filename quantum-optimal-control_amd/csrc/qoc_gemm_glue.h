// qoc_gemm_glue.h -- the small kernels between the products and chains of the GEMM path: assembly of the generators, Paterson-Stockmeyer top
// block, chain starts and chunk boundaries, padding and un-padding of the thin / wide layouts, sources and terminal costates, gradient reductions.
// Kernels only; the host side that launches them is qoc_gemm_setup.h / qoc_gemm_launch.h / qoc_gemm_routes.h.
// Reference semantics: core/tensorflow_state.py:25-46, 49-65, 77-133, 204-261.
#pragma once
#include "qoc_common.h"
#include "qoc_gemm_tiles.h"
#include "qoc_gemm_chains.h"
#include "qoc_state_source.h"

// A_t = (H0' + sum_k u_k H_k') / 2^s for every (seed, slice), padded N x N           tensorflow_state.py:30-33
// Slices are padded to SP = NC*S per seed; a padded slice gets A = 0, i.e. K = I exactly.
// (item_first, item_count): the (seed, slice) items this launch assembles -- all of them, or the slices of one rank of a time-sharded
// engine
__global__ void __launch_bounds__(256) k_gemm_assemble(QocDev d, const cplx* __restrict__ HsP, cplx* __restrict__ Aout, int N, int SP,
    int sq,
                                                        size_t item_first, size_t item_count, int nn = 0) {
    const size_t NN = nn > 0 ? (size_t)nn : (size_t)N * N;         // (nn: entries per matrix of a packed stack, as in k_gemm_assemble_rows)
    const size_t total = item_count * NN;
    const double inv = 1.0 / (double)(1 << sq);
    for (size_t o0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o0 < total; o0 += (size_t)gridDim.x * blockDim.x) {
        const size_t o = o0 + item_first * NN;
        const size_t item = o / NN, e = o - item * NN;
        const int b = (int)(item / SP), t = (int)(item - (size_t)b * SP);
        cplx acc = cmake(0.0, 0.0);
        if (t < d.steps) {
            acc = cscale(HsP[e], inv);
            for (int kk = 0; kk < d.k; ++kk) {
                const double c = d.u[((size_t)b * d.k + kk) * d.steps + t] * inv;
                const cplx h = HsP[(size_t)(kk + 1) * NN + e];
                acc.x = fma(c, h.x, acc.x); acc.y = fma(c, h.y, acc.y);
            }
        }
        Aout[o] = acc;
    }
}
// The same with the k + 1 Hamiltonian entries of a thread held in registers over a run of (seed, slice) items (k <= 8, N*N a multiple of
// 256): k_gemm_assemble re-reads them from L2 for every output entry -- (k + 1) x the written bytes through L2, 2.0 ms for the 4.2 GB of
// C3 x 64 -- this one is bound by the HBM writes alone.  blockIdx.x = 256-entry column of the matrix, blockIdx.y = run of items.
// (t0, tn): with tn > 0 the items are the slices t0 .. t0 + tn - 1 of EVERY seed (item = b * tn + t - t0), written to their usual place
// nn > 0: entries per matrix of the stack and of the output when that is not N * N (the packed anti-Hermitian image of
// qoc_gemm_chain_dpp.h: 2560)
__global__ void __launch_bounds__(256) k_gemm_assemble_rows(QocDev d, const cplx* __restrict__ HsP, cplx* __restrict__ Aout, int N, int SP,
    int sq, int per,
                                                             size_t item_first, size_t item_count, int t0 = 0, int tn = 0, int nn = 0) {
    const size_t NN = nn > 0 ? (size_t)nn : (size_t)N * N;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const double inv = 1.0 / (double)(1 << sq);
    cplx h[9];
#pragma unroll
    for (int kk = 0; kk < 9; ++kk) h[kk] = kk <= d.k ? cscale(HsP[(size_t)kk * NN + e], inv) : cmake(0.0, 0.0);
    const size_t items = item_first + item_count;
    const size_t i0 = item_first + (size_t)blockIdx.y * per, i1 = i0 + per < items ? i0 + per : items;
    for (size_t item = i0; item < i1; ++item) {
        int b, t;
        if (tn > 0) { b = (int)(item / tn); t = t0 + (int)(item - (size_t)b * tn); }
        else { b = (int)(item / SP); t = (int)(item - (size_t)b * SP); }
        cplx acc = cmake(0.0, 0.0);
        if (t < d.steps) {
            acc = h[0];
            const double* ub = d.u + (size_t)b * d.k * d.steps + t;
#pragma unroll
            for (int kk = 0; kk < 8; ++kk)
                if (kk < d.k) { const double c = ub[(size_t)kk * d.steps]; acc.x = fma(c, h[kk + 1].x, acc.x); acc.y = fma(c, h[kk + 1].y,
                    acc.y); }
        }
        Aout[((size_t)b * SP + t) * NN + e] = acc;
    }
}
// ---- squared-generator chain (qoc_gemm_chain_sq.h): B_t and B_t^2 of every (seed, slice), both in the packed anti-Hermitian / Hermitian
// image ---- coefficient row of item (b, t): [1, u_1 .. u_k, u_kk u_ll for kk <= ll (kk-major)] -- P = (k + 1)(k + 2) / 2 doubles, read as
// scalars by the assembly
__global__ void __launch_bounds__(256) k_gemm_sq_coefs(QocDev d, double* __restrict__ coef, int SP, int P) {
    const size_t total = (size_t)d.B * d.steps;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(o / d.steps), t = (int)(o - (size_t)b * d.steps);
        const double* ub = d.u + (size_t)b * d.k * d.steps + t;
        double* c = coef + ((size_t)b * SP + t) * P;
        double u[8];
        for (int kk = 0; kk < d.k; ++kk) u[kk] = ub[(size_t)kk * d.steps];
        c[0] = 1.0;
        int p = 1;
        for (int kk = 0; kk < d.k; ++kk) c[p++] = u[kk];
        for (int kk = 0; kk < d.k; ++kk)
            for (int ll = kk; ll < d.k; ++ll) c[p++] = u[kk] * u[ll];
    }
}
// B_t = h_0 + sum_k u_k h_k and B_t^2 = sum_p c_p q_p for the packed entry e of a thread (its k + 1 + P basis entries in registers over a
// run of items), written as [B | B^2] (2 x 2560 entries per item).  KK = number of controls.  (t0, tn) as in k_gemm_assemble_rows.
template <int KK>
__global__ void __launch_bounds__(256) k_gemm_assemble_sq(QocDev d, const cplx* __restrict__ HsPK, const cplx* __restrict__ HsSQ,
    const double* __restrict__ coef,
                                                           cplx* __restrict__ Aout, int SP, int per, size_t item_count, int t0, int tn) {
    constexpr int P = (KK + 1) * (KK + 2) / 2, GE = QOC_DPP_PK_ELEMS;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    cplx h[KK + 1], q[P];
#pragma unroll
    for (int kk = 0; kk <= KK; ++kk) h[kk] = HsPK[(size_t)kk * GE + e];
#pragma unroll
    for (int p = 0; p < P; ++p) q[p] = HsSQ[(size_t)p * GE + e];
    const size_t i0 = (size_t)blockIdx.y * per, i1 = i0 + per < item_count ? i0 + per : item_count;
    for (size_t item = i0; item < i1; ++item) {
        int b, t;
        if (tn > 0) { b = (int)(item / tn); t = t0 + (int)(item - (size_t)b * tn); }
        else { b = (int)(item / SP); t = (int)(item - (size_t)b * SP); }
        const double* c = coef + ((size_t)b * SP + t) * P;
        cplx accB = h[0], accS = q[0];
#pragma unroll
        for (int kk = 1; kk <= KK; ++kk) { const double u = c[kk]; accB.x = fma(u, h[kk].x, accB.x); accB.y = fma(u, h[kk].y, accB.y); }
#pragma unroll
        for (int p = 1; p < P; ++p) { const double u = c[p]; accS.x = fma(u, q[p].x, accS.x); accS.y = fma(u, q[p].y, accS.y); }
        cplx* out = Aout + ((size_t)b * SP + t) * (2 * GE);
        out[e] = accB;
        out[GE + e] = accS;
    }
}
// S = c0*I + c1*A (+ cT*A2): top block of the Paterson-Stockmeyer recursion
__global__ void __launch_bounds__(256) k_gemm_ps_init(const cplx* __restrict__ A, const cplx* __restrict__ A2, cplx* __restrict__ S,
                                                       size_t count, int N, double c0, double c1, double cT) {
    const size_t NN = (size_t)N * N;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < count; o += (size_t)gridDim.x * blockDim.x) {
        const size_t e = o % NN;
        const int row = (int)(e / N), col = (int)(e - (size_t)row * N);
        const cplx a = A[o];
        cplx v = cmake(c1 * a.x + (row == col ? c0 : 0.0), c1 * a.y);
        if (A2) { const cplx a2 = A2[o]; v.x = fma(cT, a2.x, v.x); v.y = fma(cT, a2.y, v.y); }
        S[o] = v;
    }
}
// Y[b] = [U0 | Psi0] padded (N x (xw+32), xw = N, or 0 in state transfer: no X chain); Psibnd[b][0] = Psi0 padded;
// inter[b][0] = V
__global__ void __launch_bounds__(256) k_gemm_chain_init(QocDev d, cplx* __restrict__ Y, cplx* __restrict__ Psibnd, int N, int NC, int xw) {
    const int ld = xw + QOC_TW;
    const size_t per = (size_t)N * ld;
    const size_t total = (size_t)d.B * per;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const size_t bb = o / per, e = o - bb * per;
        const int row = (int)(e / ld), col = (int)(e - (size_t)row * ld);
        cplx v = cmake(0.0, 0.0);
        if (row < d.n) {
            if (col < xw) { if (col < d.n) v = d.U0[row * d.n + col]; }
            else if (col - xw < d.m) v = d.Psi0[row * d.m + (col - xw)];
        }
        Y[o] = v;
        if (col >= xw) Psibnd[(bb * NC) * (size_t)N * QOC_TW + (size_t)row * QOC_TW + (col - xw)] = v;
    }
    const size_t nm = (size_t)d.n * d.m;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < (size_t)d.B * nm; o += (size_t)gridDim.x * blockDim.x) {
        const size_t bb = o / nm, e = o - bb * nm;
        d.inter[bb * (size_t)(d.steps + 1) * nm + e] = d.V[e];
    }
}
// chunk-start vectors Psibnd[b][c], c = 1 .. NC-1, from the thin blocks (columns N..N+31) of the per-step results: Ys holds one
// [B][N][ld] result per chunk step (slot c = the vectors at the START of chunk c), so the per-step products of N > 64 need no copy
// launch between them (31 launches of ~8 us with their gaps per iteration at n = 128)
__global__ void __launch_bounds__(256) k_gemm_take_bnd_all(QocDev d, const cplx* __restrict__ Ys, cplx* __restrict__ Psibnd, int N, int NC,
    int xw) {
    const int ld = xw + QOC_TW;
    const size_t per = (size_t)N * QOC_TW, slot = (size_t)d.B * N * ld;
    const size_t total = (size_t)d.B * (NC - 1) * per;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const size_t bc = o / per, e = o - bc * per;
        const size_t bb = bc / (NC - 1);
        const int c = 1 + (int)(bc - bb * (NC - 1));
        const int row = (int)(e / QOC_TW), col = (int)(e - (size_t)row * QOC_TW);
        Psibnd[(bb * NC + c) * per + e] = Ys[(size_t)c * slot + bb * (size_t)N * ld + (size_t)row * ld + xw + col];
    }
}
// inter[b][t+1] (API layout) from interP[b][t] (padded thin), t < steps
__global__ void __launch_bounds__(256) k_gemm_unpad_inter(QocDev d, const cplx* __restrict__ interP, int N, int SP) {
    const size_t nm = (size_t)d.n * d.m, per = (size_t)N * QOC_TW;
    const size_t total = (size_t)d.B * d.steps * nm;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const size_t bt = o / nm, e = o - bt * nm;
        const size_t bb = bt / d.steps, t = bt - bb * d.steps;
        const int row = (int)(e / d.m), col = (int)(e - (size_t)row * d.m);
        d.inter[(bb * (size_t)(d.steps + 1) + t + 1) * nm + e] = interP[(bb * SP + t) * per + (size_t)row * QOC_TW + col];
    }
}
// final_state, unitary_scale from the X block of Y                                     tensorflow_state.py:223-225
__global__ void __launch_bounds__(1024) k_gemm_take_final(QocDev d, const cplx* __restrict__ Y, int N) {
    __shared__ double red[32];
    const int b = blockIdx.x, ld = N + QOC_TW, n = d.n;
    const cplx* X = Y + (size_t)b * N * ld;
    double part = 0.0;
    // a wave per row, lanes along it (a thread per row walked the row alone, 64 rows apart from its neighbours: 0.46 ms at n = 512)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int c = wv; c < n; c += nw) {
        double sr = 0.0, si = 0.0;
        for (int a = lane; a < n; a += 64) { const cplx v = X[(size_t)c * ld + a]; sr += v.x; si += v.y; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { sr += __shfl_xor(sr, off, 64); si += __shfl_xor(si, off, 64); }
        if (lane == 0) part += sr * sr + si * si;
    }
    for (int o = threadIdx.x; o < n * n; o += blockDim.x) d.Xfinal[(size_t)b * n * n + o] = X[(size_t)(o / n) * ld + (o % n)];
    const double tot = block_sum(part, red);
    if (threadIdx.x == 0) d.uscale[b] = tot / (double)n;
}
// sources SrcP[b][tau] (padded thin, tau = 0..SP-1; zero for tau = 0 and tau > steps) and the costate at the END of the
// last chunk Ebnd[b][NC-1]: -(2/m^2) z W, plus S_steps when there is no padded slice to add it through the recursion
// `cols` = columns written per row: QOC_TW, or the MV vector slots in the direct route, whose Taylor chains read nothing else of a thin
// panel (C3 x 64: 2.1 GB of zero columns, 0.34 ms per iteration, no longer written)
// `compact` (DPP chain, one vector): SrcP[b][tau][row] contiguous -- a thin panel puts the rows of ONE column 512 bytes apart, every
// 16-byte store its own memory transaction (C3 x 64: 0.11 ms for 4 M entries)
__global__ void __launch_bounds__(256) k_gemm_sources(QocDev d, cplx* __restrict__ SrcP, cplx* __restrict__ Ebnd, int N, int SP, int NC,
    int cols, int compact = 0) {
    const size_t per = (size_t)N * QOC_TW, perw = (size_t)N * cols;
    const bool need_src = d.n_forb > 0 || d.has_speed;
    const size_t total = (size_t)d.B * (need_src ? SP : 1) * perw;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const size_t bt = o / perw, ew = o - bt * perw;
        const int per_seed = need_src ? SP : 1;
        const int b = (int)(bt / per_seed), tau = (int)(bt - (size_t)b * per_seed);
        const int row = (int)(ew / cols), col = (int)(ew - (size_t)row * cols);
        const size_t e = (size_t)row * QOC_TW + col;
        const bool valid = row < d.n && col < d.m;
        if (need_src) {
            cplx s = cmake(0.0, 0.0);
            if (valid && tau >= 1 && tau <= d.steps) s = source_at(d, b, tau, row, col);
            SrcP[compact ? bt * (size_t)N + row : bt * per + e] = s;
        }
        if (tau == 0) {
            cplx v = cmake(0.0, 0.0);
            if (valid) {
                const double c0 = -2.0 / ((double)d.m * (double)d.m);
                v = cscale(cmul(d.zfin[b], d.W[row * d.m + col]), c0);
                if (need_src && SP == d.steps) v = cadd(v, source_at(d, b, d.steps, row, col));
            }
            Ebnd[((size_t)b * NC + (NC - 1)) * per + e] = v;
        }
    }
}
// z-free costate at the end of the pulse, Ebnd[b][NC-1] = -(2/m^2) W: start of a backward chain that does not wait for the overlap
__global__ void __launch_bounds__(256) k_gemm_zfree_end(QocDev d, cplx* __restrict__ Ebnd, int N, int NC) {
    const size_t per = (size_t)N * QOC_TW;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < (size_t)d.B * per; o += (size_t)gridDim.x * blockDim.x) {
        const size_t b = o / per, e = o - b * per;
        const int row = (int)(e / QOC_TW), col = (int)(e - (size_t)row * QOC_TW);
        cplx v = cmake(0.0, 0.0);
        if (row < d.n && col < d.m) v = cscale(d.W[row * d.m + col], -2.0 / ((double)d.m * (double)d.m));
        Ebnd[(b * NC + (NC - 1)) * per + e] = v;
    }
}
// Lambda_t = z Lambda0_t for the time-major wide costates of a seed (LamP[b]: N rows x ldW), z = d.zfin[b]
__global__ void __launch_bounds__(256) k_gemm_scale_lam(QocDev d, cplx* __restrict__ LamP, int N, int ldW, int cols) {
    const size_t per = (size_t)N * cols;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < (size_t)d.B * per; o += (size_t)gridDim.x * blockDim.x) {
        const size_t b = o / per, e = o - b * per;
        const size_t row = e / cols, col = e - row * cols;
        cplx* p = LamP + (b * N + row) * (size_t)ldW + col;
        *p = cmul(d.zfin[b], *p);
    }
}
// LamP[b][(c+1)S-1] = (Ebnd ? Ebnd[b][c] : 0): costate at the end of every chunk
__global__ void __launch_bounds__(256) k_gemm_set_chunk_ends(QocDev d, cplx* __restrict__ LamP, const cplx* __restrict__ Ebnd, int N, int S,
    int NC) {
    const size_t per = (size_t)N * QOC_TW;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < (size_t)d.B * NC * per; o += (size_t)gridDim.x * blockDim.x) {
        const size_t bc = o / per, e = o - bc * per;
        LamP[(bc * S + (S - 1)) * per + e] = Ebnd ? Ebnd[o] : cmake(0.0, 0.0);
    }
}
// dst[b] = src[b] for B matrices of NN elements (odd element of a product-tree level moves up unchanged)
__global__ void __launch_bounds__(256) k_gemm_copy_mats(cplx* __restrict__ dst, long long sD, const cplx* __restrict__ src, long long sS,
    int B, int NN) {
    const size_t total = (size_t)B * NN;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const size_t bb = o / NN, e = o - bb * NN;
        dst[bb * sD + e] = src[bb * sS + e];
    }
}
// inter[b][t+1] (API layout) from the time-major wide layout W[b][row][t*MV + col]
__global__ void __launch_bounds__(256) k_gemm_unpad_wide(QocDev d, const cplx* __restrict__ W, int N, int ldW, int MV) {
    const size_t nm = (size_t)d.n * d.m;
    const size_t total = (size_t)d.B * d.steps * nm;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const size_t bt = o / nm, e = o - bt * nm;
        const size_t bb = bt / d.steps, t = bt - bb * d.steps;
        const int row = (int)(e / d.m), col = (int)(e - (size_t)row * d.m);
        d.inter[(bb * (size_t)(d.steps + 1) + t + 1) * nm + e] = W[(bb * N + row) * (size_t)ldW + t * MV + col];
    }
}
// dLdu[b][k][t] = sum over row tiles and vector slots of the per-column dots (wide layout)
__global__ void __launch_bounds__(256) k_gemm_grad_reduce_wide(QocDev d, const double* __restrict__ partial, int tiles_m, int ldW, int MV) {
    const size_t total = (size_t)d.B * d.k * d.steps;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const size_t bk = o / d.steps;
        const int t = (int)(o - bk * d.steps);
        const double* p = partial + bk * tiles_m * (size_t)ldW + (size_t)t * MV;
        double s = 0.0;
        for (int i = 0; i < tiles_m; ++i)
            for (int jv = 0; jv < MV; ++jv) s += p[(size_t)i * ldW + jv];
        d.dLdu[o] = s;
    }
}
// dLdu[b][k][t] = sum over row tiles of the partial dots
__global__ void __launch_bounds__(256) k_gemm_grad_reduce(QocDev d, const double* __restrict__ partial, int tiles_m) {
    const size_t total = (size_t)d.B * d.steps * d.k;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const size_t bt = o / d.k;
        const int kk = (int)(o - bt * d.k);
        const int b = (int)(bt / d.steps), t = (int)(bt - (size_t)b * d.steps);
        const double* p = partial + (bt * d.k + kk) * tiles_m;
        double s = 0.0;
        for (int i = 0; i < tiles_m; ++i) s += p[i];
        d.dLdu[((size_t)b * d.k + kk) * d.steps + t] = s;
    }
}

// ---- gradients of large problems (N > 64, m <= 8) as ONE wide product per seed ----------------------------------------------------------
// The per-slice thin tiles [t][N][32] of Psi_t / Lambda_t carry m <= 8 useful columns of 32: k batched launches of 2000 padded thin
// products with a dot epilogue ran at ~21 TFLOP/s of mostly padding (C5: 12.7 ms of 215).  Re-packed time-major -- wide[row][t * 8 + col],
// the layout the persistent chains of N <= 64 write directly -- the products of ALL controls are one batched N x N x (8 steps) GEMM on
// k_zgemm_wg, and dL/du_{k,t} = Re sum conj(Lambda_t) (H_k' Psi_t) (tensorflow_state.py:61-63) is a column-block dot of its result.
#define QOC_WIDE_MV 8
__global__ void __launch_bounds__(256) k_gemm_to_wide(QocDev d, const cplx* __restrict__ thinP, const cplx* __restrict__ thinL,
                                                      cplx* __restrict__ wideP, cplx* __restrict__ wideL, int N, int W, int count) {
    const size_t total = (size_t)count * N * QOC_WIDE_MV;                                     // `count` slices from thinP / thinL on
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
        const int col = (int)(o % QOC_WIDE_MV);
        const size_t tr = o / QOC_WIDE_MV;
        const int row = (int)(tr % N), t = (int)(tr / N);
        const size_t src = ((size_t)t * N + row) * QOC_TW + col, dst = (size_t)row * W + (size_t)t * QOC_WIDE_MV + col;
        wideP[dst] = thinP[src];
        wideL[dst] = thinL[src];
    }
}
// one wave per (control, slice): rows lane, lane + 64, ...; the 8 columns of a slice are one 128-byte line of a row
// (column block ti of the wide buffers is slice t_first + ti: the whole pulse, or the slices of one rank of a time-sharded engine)
__global__ void __launch_bounds__(256) k_gemm_dot_wide(QocDev d, int b, const cplx* __restrict__ wideC, const cplx* __restrict__ wideL,
    int N, int W,
                                                       int t_first, int count) {
    const int lane = threadIdx.x & 63;
    const size_t item = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (item >= (size_t)d.k * count) return;
    const int kk = (int)(item / count), t = (int)(item - (size_t)kk * count);
    const cplx* C = wideC + (size_t)kk * N * W + (size_t)t * QOC_WIDE_MV;
    const cplx* L = wideL + (size_t)t * QOC_WIDE_MV;
    double acc = 0.0;
    for (int row = lane; row < N; row += 64) {
#pragma unroll
        for (int col = 0; col < QOC_WIDE_MV; ++col) {
            const cplx c = C[(size_t)row * W + col], l = L[(size_t)row * W + col];
            acc = fma(l.x, c.x, acc); acc = fma(l.y, c.y, acc);                          // Re conj(l) c
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) d.dLdu[((size_t)b * d.k + kk) * d.steps + t_first + t] = acc;
}

// K[b][t] = I for the padded slices t = steps .. SP - 1 (set once: the launch-per-product route of ONE control set never computes them)
__global__ void __launch_bounds__(256) k_gemm_pad_identity(cplx* __restrict__ K, int B, int N, int steps, int SP) {
    const size_t NN = (size_t)N * N, per = (size_t)(SP - steps) * NN;
    for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < (size_t)B * per; o += (size_t)gridDim.x * blockDim.x) {
        const size_t b = o / per, r = o - b * per, t = steps + r / NN, e = r % NN;
        K[(b * SP + t) * NN + e] = cmake(e / N == e % N ? 1.0 : 0.0, 0.0);
    }
}
