// qoc_gemm_launch.h -- the launchers of the GEMM path's kernels (each template ladder one qoc_pick) and the makers of their argument structs.
#pragma once
#include "qoc_pick.h"
#include "qoc_gemm_setup.h"

template <class T> static inline T qoc_zeroed() { T v; memset(&v, 0, sizeof v); return v; }
static inline int gemm_grid(size_t total) { size_t g = (total + 255) / 256; return (int)(g > 65535 ? 65535 : (g < 1 ? 1 : g)); }
// 1 / j! for j < QOC_GEMM_MAXT
static inline ExpmCoef qoc_inverse_factorials() {
    ExpmCoef cf;
    double f = 1.0;
    for (int j = 0; j < QOC_GEMM_MAXT; ++j) { if (j > 0) f *= (double)j; cf.c[j] = 1.0 / f; }
    return cf;
}

// ---- GemmArgs of the shapes this path multiplies; operands and the strides a maker does not name are the caller's --------------------------
// `batch` square N x N products
static inline GemmArgs qoc_gemm_square_args(int N, int batch) {
    GemmArgs g = qoc_zeroed<GemmArgs>();
    g.lda = g.ldb = g.ldc = N; g.Kdim = N; g.tiles_m = g.tiles_n = N / 32; g.batch = batch; g.alpha = 1.0;
    return g;
}
// [X | Psi] <- M [X | Psi]: N x N times N x ld (ld = 32 or N + 32), operand strides sA and sY
static inline GemmArgs qoc_gemm_boundary_args(int N, int ld, int batch, long long sA, long long sY) {
    GemmArgs g = qoc_zeroed<GemmArgs>();
    g.lda = N; g.sA = sA; g.ldb = g.ldc = ld; g.sB = g.sC = sY;
    g.Kdim = N; g.tiles_m = N / 32; g.tiles_n = ld / 32; g.batch = batch; g.alpha = 1.0;
    return g;
}
// thin panels: N x N times N x 32, + the addend E when `addend`
static inline GemmArgs qoc_gemm_thin_args(int N, int batch, bool addend) {
    GemmArgs g = qoc_zeroed<GemmArgs>();
    g.lda = N; g.ldb = g.ldc = QOC_TW; g.Kdim = N; g.tiles_m = N / 32; g.tiles_n = 1; g.batch = batch; g.alpha = 1.0;
    if (addend) { g.lde = QOC_TW; g.beta = 1.0; }
    return g;
}
// gradient products with a dot epilogue against conj(L): H_k' times panels of row stride ld, tiles_n column tiles
static inline GemmArgs qoc_gemm_dot_args(int N, int ld, int tiles_n) {
    GemmArgs g = qoc_zeroed<GemmArgs>();
    g.lda = N; g.ldb = g.ldl = ld; g.Kdim = N; g.tiles_m = N / 32; g.tiles_n = tiles_n;
    return g;
}
// wideC[kk] = H'_{kk+1} wideP for every control: batch index = control, W columns
static inline GemmArgs qoc_gemm_controls_args(const QocGemm& gm, const QocDev& d, int W) {
    const int N = gm.N;
    GemmArgs g = qoc_zeroed<GemmArgs>();
    g.A = gm.HsP + (size_t)N * N; g.sA = (long long)N * N; g.lda = N;
    g.Bm = gm.wideP; g.sB = 0; g.ldb = W;
    g.C = gm.wideC; g.sC = (long long)N * W; g.ldc = W;
    g.Kdim = N; g.tiles_m = N / 32; g.tiles_n = W / 32; g.batch = d.k; g.alpha = 1.0;
    return g;
}

// ---- k_zgemm32 / k_zgemm_wg ----------------------------------------------------------------------------------------------------------------
template <bool CONJT, int EPI, int SK>
static inline void qoc_gemm_launch_sk(const GemmArgs& g, unsigned blocks, hipStream_t s) {
    const size_t lds = SK > 1 ? (size_t)(SK - 1) * 2048 * sizeof(double) : 0;
    hipLaunchKernelGGL((k_zgemm32<CONJT, EPI, SK>), dim3(blocks), dim3(64 * SK), lds, s, g);
}
// Kernels that use more than 64 KB of dynamic LDS must opt in, per device: called after qoc_gemm_setup (one engine = one device)
template <bool CONJT, int EPI>
static inline bool qoc_gemm_lds_opt_in_sk() {
    return hipFuncSetAttribute((const void*)k_zgemm32<CONJT, EPI, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, 7 * 2048 * (int)sizeof(double)) == hipSuccess;
}
static inline size_t qoc_scan_lds(int N) { return ((size_t)N * (N + 1) + 2 * (size_t)N * 8) * sizeof(cplx); }
static inline bool qoc_gemm_lds_opt_in() {
    return qoc_gemm_lds_opt_in_sk<false, 0>() && qoc_gemm_lds_opt_in_sk<false, 1>() && qoc_gemm_lds_opt_in_sk<false, 2>() && qoc_gemm_lds_opt_in_sk<true, 0>() &&
           hipFuncSetAttribute((const void*)k_gemm_expm_fused<64>, hipFuncAttributeMaxDynamicSharedMemorySize,
               2 * 64 * (64 + QOC_EXPM_LDPAD) * (int)sizeof(cplx)) == hipSuccess &&
           hipFuncSetAttribute((const void*)k_gemm_scan_nodes<64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)qoc_scan_lds(64)) == hipSuccess &&
           qoc_zgemm_wg_opt_in();
}
// The split-K factor follows the launch size: fill ~2 waves per SIMD (2048 waves) when the batch is small.  The split factor and the
// kernel family change the association of the sums, so they follow the PLANNED batch: QocGemm::plan_scale = planned / local batch
#ifndef QOC_SK_TARGET
#define QOC_SK_TARGET 2048     // waves a split-K launch aims at (~2 per SIMD)
#endif
// large plain products: workgroup tiles of 64 x 128 on the 4x4x4 MFMA form (k_zgemm_wg), for `tiles` planned 32 x 32 tiles
static inline bool qoc_gemm_wg_shape(const GemmArgs& g, size_t tiles) {
    return (g.tiles_m & 1) == 0 && (g.tiles_n & 3) == 0 && (g.Kdim % ZW_KC) == 0 && g.Kdim >= 128 && tiles >= 8 * 1024;
}
static inline int qoc_gemm_split_k(const GemmArgs& g, size_t tiles) {
    int sk = 1;
    if (tiles * 2 <= QOC_SK_TARGET && (g.Kdim / 2) % 8 == 0) sk = 2;
    if (tiles * 4 <= QOC_SK_TARGET && (g.Kdim / 4) % 8 == 0) sk = 4;
    if (tiles * 8 <= QOC_SK_TARGET && (g.Kdim / 8) % 8 == 0) sk = 8;
    return sk;
}
static inline size_t qoc_gemm_planned_tiles(const QocGemm& gm, size_t tiles) { return (size_t)((double)tiles * gm.plan_scale + 0.5); }
// will this plain product run on k_zgemm_wg?
static inline bool qoc_gemm_takes_wg(const QocGemm& gm, const GemmArgs& g) {
    const size_t tiles = qoc_gemm_planned_tiles(gm, (size_t)g.batch * g.tiles_m * g.tiles_n);
    return qoc_gemm_split_k(g, tiles) == 1 && qoc_gemm_wg_shape(g, tiles);
}
// epi: 0 = C = alpha op(A) B + beta E + gamma I (conjt: op = conjugate transpose), 1 = per-tile dots, 2 = per-column dots.
// sk_tiles: tile count the split-K factor is chosen for when the launch is one PART of a product (the parts must sum in the order of the
// whole)
static inline void qoc_gemm_launch(const QocGemm& gm, bool conjt, int epi, const GemmArgs& g, hipStream_t s, size_t sk_tiles = 0) {
    const size_t real_tiles = (size_t)g.batch * g.tiles_m * g.tiles_n;
    const size_t tiles = qoc_gemm_planned_tiles(gm, sk_tiles ? sk_tiles : real_tiles);
    const int sk = qoc_gemm_split_k(g, tiles);
    if (epi == 0 && !conjt && sk == 1 && qoc_gemm_wg_shape(g, tiles)) { qoc_zgemm_wg_launch(g, (unsigned)(real_tiles / 8), s); return; }
    const int kind = epi == 2 ? 2 : (epi == 1 ? 1 : (conjt ? 3 : 0));                   // (3: the plain epilogue on the conjugate transpose)
    qoc_pick([&](auto KIND, auto SK) { qoc_gemm_launch_sk<KIND == 3, KIND == 3 ? 0 : KIND, SK>(g, (unsigned)real_tiles, s); },
             QocOneOf<2, 1, 3, 0>{kind}, QocOneOf<8, 4, 2, 1>{sk});
}

// ---- assembly of the generators -------------------------------------------------------------------------------------------------------------
// grid of the kernels that keep their stack entries in registers over a run of items: x = 256-entry columns, y = runs of `per` items
static inline dim3 qoc_gemm_rows_grid(size_t entries, size_t items, int target_wgs, int& per) {
    const int gx = (int)(entries / 256);
    per = (int)((items * gx + target_wgs - 1) / target_wgs);
    if (per < 4) per = 4;
    return dim3(gx, (int)((items + per - 1) / per));
}
// the slices t0 .. t0 + tn - 1 of every seed (needs what k_gemm_assemble_rows needs: k <= 8, N*N a multiple of 256)
static inline void qoc_gemm_assemble_window(const QocDev& d, const cplx* HsP, cplx* Aout, int N, int SP, int t0, int tn, hipStream_t s,
                                            int target_wgs = 8192, int nn = 0) {
    const size_t NN = nn > 0 ? (size_t)nn : (size_t)N * N, items = (size_t)d.B * tn;
    int per;
    const dim3 grid = qoc_gemm_rows_grid(NN, items, target_wgs, per);
    hipLaunchKernelGGL(k_gemm_assemble_rows, grid, dim3(256), 0, s, d, HsP, Aout, N, SP, 0, per, (size_t)0, items, t0, tn, nn);
}
// [B | B^2] of the slices t0 .. t0 + tn - 1 of every seed (tn = 0: all items) for the squared-generator chain
static inline void qoc_gemm_assemble_sq(const QocDev& d, const cplx* HsPK, const cplx* HsSQ, const double* coef, cplx* Aout, int SP, int t0,
                                        int tn, hipStream_t s, int target_wgs = 8192) {
    const size_t items = (size_t)d.B * (tn > 0 ? tn : SP);
    int per;
    const dim3 grid = qoc_gemm_rows_grid(QOC_DPP_PK_ELEMS, items, target_wgs, per);
    qoc_pick([&](auto KK) { hipLaunchKernelGGL(k_gemm_assemble_sq<KK>, grid, dim3(256), 0, s, d, HsPK, HsSQ, coef, Aout, SP, per, items, t0, tn); },
             QocOneOf<1, 2, 3, 4, 5, 6, 7, 8>{d.k});
}
static inline void qoc_gemm_assemble_launch(const QocDev& d, const cplx* HsP, cplx* Aout, int N, int SP, int sq, hipStream_t s,
                                            size_t item_first = 0, size_t item_count = 0, int nn = 0) {
    if (item_count == 0) item_count = (size_t)d.B * SP;
    const size_t NN = nn > 0 ? (size_t)nn : (size_t)N * N, items = item_count;
    if (d.k <= 8 && NN % 256 == 0 && items >= 64) {
        int per;
        const dim3 grid = qoc_gemm_rows_grid(NN, items, 8192, per);                      // ~8192 workgroups
        if (grid.y <= 65535) {
            hipLaunchKernelGGL(k_gemm_assemble_rows, grid, dim3(256), 0, s, d, HsP, Aout, N, SP, sq, per, item_first, item_count, 0, 0, nn);
            return;
        }
    }
    hipLaunchKernelGGL(k_gemm_assemble, dim3(gemm_grid(items * NN)), dim3(256), 0, s, d, HsP, Aout, N, SP, sq, item_first, item_count, nn);
}
// The generators of a direct route with the assembly overlap: window 0 on this stream -- it has the memory system to itself (started
// together, head and tail both took as long as the whole) --, the later windows on the second stream beside the forward chain.
// assemble(t0, tn, stream, target_wgs) assembles the slices t0 .. t0 + tn - 1 of every seed
template <class Assemble>
static inline void qoc_gemm_assemble_windows(const QocGemm& gm, hipStream_t s, Assemble&& assemble) {
    const int nw = (int)gm.asm_win.size() - 1;
    assemble(0, gm.asm_win[1], s, 8192);
    hipEventRecord(gm.ev_ready, s);
    hipStreamWaitEvent(gm.aux, gm.ev_ready, 0);
    for (int w = 1; w < nw; ++w) {
        assemble(gm.asm_win[w], gm.asm_win[w + 1] - gm.asm_win[w], gm.aux, gm.asm_tail_wgs);
        hipEventRecord(gm.ev_win[w], gm.aux);
    }
}

// ---- chains ---------------------------------------------------------------------------------------------------------------------------------
// a chain without an addend reads the zero thin buffer with zero strides
static inline void qoc_chain_zero_addend(const QocGemm& gm, ChainArgs& a) { if (!a.E) { a.E = gm.zthin; a.sEb = a.sEc = a.sEs = 0; } }
// The Taylor chains of the direct route, `blocks` workgroups; with `pair` a second chain beside the first in the same launch (`blocks`
// workgroups each).  The kernel follows QocGemm::dpp_mode()
static inline void qoc_taylor_chain_launch(const QocGemm& gm, ChainArgs a0, const ChainArgs* pair, int blocks, hipStream_t s) {
    ChainArgs a1 = pair ? *pair : a0;
    qoc_chain_zero_addend(gm, a0);
    qoc_chain_zero_addend(gm, a1);
    const dim3 grid(pair ? 2 * blocks : blocks);
    const int mode = gm.dpp_mode();
    if (mode == 3) hipLaunchKernelGGL(k_gemm_taylor_chain_sq, grid, dim3(256), 0, s, a0, a1, blocks);
    else if (mode == 2) hipLaunchKernelGGL(k_gemm_taylor_chain_dpp<true>, grid, dim3(256), 0, s, a0, a1, blocks);
    else if (mode) qoc_pick([&](auto CW) { hipLaunchKernelGGL((k_gemm_taylor_chain_dpp<false, CW>), grid, dim3(256), 0, s, a0, a1, blocks); },
                            QocOneOf<10, 12, 14, 16>{mode});
    else qoc_pick([&](auto N, auto MV) {
        hipLaunchKernelGGL((k_gemm_taylor_chain<N, MV>), grid, dim3(TaylorMap<N, MV>::type::THREADS), 0, s, a0, a1, blocks);
    }, QocOneOf<32, 64>{gm.N}, QocOneOf<1, 2, 4, 8>{gm.MV});
}
// y <- M_j y + E_j along `blocks` chains.  conjt: y <- conj(M_j) y, used with M_j = K_j^T for the backward chains (K_j^H = conj(K_j^T): the
// rows of the transposed copy are read with the same coalesced pattern as the forward chains)
static inline void qoc_chain_launch(const QocGemm& gm, bool conjt, ChainArgs a, int blocks, hipStream_t s) {
    if (a.len <= 0 && !a.Fin && !a.store_initial) return;
    qoc_chain_zero_addend(gm, a);
    qoc_pick([&](auto N, auto MV, auto CONJ, auto HAS_OUT) {
        hipLaunchKernelGGL((k_gemm_chain_fwd<N, MV, CONJ != 0, HAS_OUT != 0>), dim3(blocks), dim3(256), 0, s, a);
    }, QocOneOf<32, 64>{gm.N}, QocOneOf<1, 2, 4, 8>{gm.MV}, QocOneOf<1, 0>{conjt}, QocOneOf<1, 0>{a.Out != nullptr});
}
static inline void qoc_scan_launch(const QocGemm& gm, const ScanArgs& a, int B, hipStream_t s) {
    if (a.nchains <= 0) return;
    qoc_pick([&](auto N) { hipLaunchKernelGGL(k_gemm_scan_nodes<N>, dim3(B * a.nchains), dim3(256), qoc_scan_lds(N), s, a); }, QocOneOf<32, 64>{gm.N});
}
