// qoc_gemm_setup.h -- state of the GEMM path (QocGemm) and its set-up: the route and every flag and size decided once by a pure function, then the
// arena, the host images of the Hamiltonian stack, the clears and set-up kernels, the streams and events of the assembly overlap.
#pragma once
#include <string>
#include <utility>
#include <vector>
#include "qoc_gemm_glue.h"
#include "qoc_gemm_expm.h"

// Which of the three algorithms an engine of this path runs; fixed by set-up.
enum QocGemmRoute {
    QOC_GEMM_STEPWISE,     // N > 64 or m > 8: one batched product launch per chunk boundary and per sweep step
    QOC_GEMM_PERSISTENT,   // N <= 64, m <= 8: thin chains as persistent VALU kernels (qoc_gemm_chains.h) instead of one launch per step
    QOC_GEMM_DIRECT,       // state transfer, N <= 64, m <= 8: Taylor mat-vec chains on the assembled generators (one chunk, no propagators)
};

// the experimental switches of this path (qoc_exp_env), as qoc_gemm_decide read them
struct QocGemmSwitches {
    bool no_chain_dpp = false;       // QOC_CHAIN_DPP=0: the butterfly kernel k_gemm_taylor_chain
    bool no_active_columns = false;  // QOC_DPP_ACTIVE_COLUMNS=0
    bool no_overlap = false;         // QOC_ASM_OVERLAP=0: one assembly launch in front of the chain
    bool no_cumask = false;          // QOC_ASM_CUMASK=0: plain second stream, chain on the engine's
    int chain_cus = 112;             // QOC_ASM_CUMASK=<count>: compute units of the chains' mask
    int tail_wgs = 0;                // QOC_ASM_TAIL_WGS (0: the default of the stream kind)
    bool has_split16 = false; int split16 = 0;   // QOC_ASM_SPLIT16: sixteenths of the pulse assembled in front of the chain
    int windows = 2;                 // QOC_ASM_WINDOWS, 2 .. 4
};

// Time is cut into NC chunks of S = 2^L slices (padded with identity slices to SP = NC*S).  A pairwise product tree over
// the K_t gives the chunk products at the batched-GEMM rate; the sequential part of each chain shrinks from `steps`
// launches to NC (chunk boundaries) + S (all chunks swept in parallel).
struct QocGemm {
    QocGemmRoute route = QOC_GEMM_STEPWISE;
    int N = 0, S = 1, L = 0, NC = 1, SP = 1;
    int MV = 0, ldW = 0;      // vector slots (m rounded up to 1/2/4/8) and row stride of the time-major wide buffers of the chain routes
    // planned / local batch (QocDev::Bplan / B): split-K factors and kernel families are chosen for the planned batch
    double plan_scale = 1.0;
    QocGemmSwitches sw;
    bool antiherm = false;    // in: every generator anti-Hermitian (set by the engine before qoc_gemm_setup)
    // in: qoc_config.variant of an explicit GEMM-path request: 1 = never the squared-generator chain, 2 = always where it applies
    int direct_variant = 0;

    // ---- direct and persistent routes
    // state transfer: Psibnd[b][0] = Psi0 and inter[b][0] = V never change -- k_gemm_chain_init ran at set-up, not per iteration
    bool init_once = false;

    // ---- direct route only
    bool dpp_chain = false;   // N = 64, one state vector: k_gemm_taylor_chain_dpp (qoc_gemm_chain_dpp.h)
    // dpp_chain on anti-Hermitian generators: only the blocks on and below the block diagonal are assembled, stored and read
    bool dpp_packed = false;
    // dpp_packed, few enough control sets for the chains to be latency-bound: [B | B^2] per slice and k_gemm_taylor_chain_sq
    // (qoc_gemm_chain_sq.h)
    bool sq_chain = false;
    // dpp_chain on a padded problem (n <= 56 levels in N = 64) that is latency-bound (<= 128 control sets) or cannot be packed: columns per
    // wave 10 / 12 / 14 instead of 16 -- only the first 4 dpp_cw columns of the full image are assembled, stored, read and multiplied.  16: off
    int dpp_cw = 16;
    // dpp_chain with a state regulariser (forward chain alone in its launch): the pulse is cut into asm_win.size() - 1 windows
    // [asm_win[w], asm_win[w + 1]).  Window 0 = [0, asm_split) is assembled in front of the chain, window w >= 1 on the second stream (64 of
    // 256 CUs, 1.4 TB/s) while the chain walks window w - 1: one chain launch per window, each continuing from the state the previous one
    // left in Aoff.  asm_split == 0: no overlap
    int asm_split = 0, asm_tail_wgs = 512;
    std::vector<int> asm_win; std::vector<hipEvent_t> ev_win;
    int mask_cus = 0;         // > 0: the chains run on a stream masked to the first mask_cus compute units, the assembly on the others
    hipStream_t aux = nullptr, chain_s = nullptr; hipEvent_t ev_ready = nullptr, ev_fwd = nullptr, ev_p1 = nullptr;
    cplx* HsPT = nullptr;     // dpp_chain: the stack transposed (k_gemm_assemble_rows then writes the generators column-major), truncated or packed
    cplx* HsSQ = nullptr;     // sq_chain: the (k + 1)(k + 2) / 2 packed basis matrices of B^2
    double* sqc = nullptr;    // sq_chain: [B][SP][P] coefficient rows (k_gemm_sq_coefs)
    // what qoc_taylor_chain_launch runs: 0 = k_gemm_taylor_chain, 1 = k_gemm_taylor_chain_dpp on full generators, 2 = on packed anti-Hermitian
    // generators, 3 = k_gemm_taylor_chain_sq on packed [B | B^2], 10 / 12 / 14 = k_gemm_taylor_chain_dpp on the first 4 x 10 / 12 / 14 columns
    int dpp_mode() const { return dpp_chain ? (sq_chain ? 3 : (dpp_packed ? 2 : (dpp_cw < 16 ? dpp_cw : 1))) : 0; }
    // entries of one assembled slice, and of one matrix of the stack it is assembled from when that is not N * N (else 0)
    size_t gen_elems() const {
        if (sq_chain) return (size_t)2 * QOC_DPP_PK_ELEMS;
        if (dpp_packed) return (size_t)QOC_DPP_PK_ELEMS;
        return dpp_chain && dpp_cw < 16 ? (size_t)256 * dpp_cw : (size_t)N * N;
    }
    int stack_elems() const { return dpp_packed ? QOC_DPP_PK_ELEMS : (dpp_chain && dpp_cw < 16 ? 256 * dpp_cw : 0); }

    // ---- persistent route only
    cplx* KT = nullptr;       // K_t^T  [B*SP][N][N] (rows of K^H for the backward chains)
    cplx* PcT = nullptr;      // P_c^T  [B][NC][N][N] (== KT when S = 1)
    cplx* root = nullptr;     // unitary mode: product tree above the chunk products, down to one matrix per seed
    ScanArgs scan;            // its levels (filled by the forward pass each iteration; pointers are stable)

    // ---- stepwise route only
    // > 0: gradients of an N > 64 problem through ONE wide product per seed (k_gemm_to_wide, k_zgemm_wg, k_gemm_dot_wide)
    int wideW = 0;
    cplx *wideP = nullptr, *wideL = nullptr, *wideC = nullptr;   // [N][wideW], [N][wideW], [k][N][wideW]
    // time-axis sharding of one trajectory (qoc_gemm_ts.h): G ranks own runs of chunks; ts_rank < 0 emulates all of them in this engine
    int ts_G = 0, ts_rank = -1;
    std::vector<int> ts_cb;                                       // chunk boundaries: rank r owns [ts_cb[r], ts_cb[r + 1])
    cplx *ts_Rall = nullptr, *ts_Rtmp = nullptr;                  // [G][N][N] rank products (all-gathered in place), [2][N][N]
    // [G + 1][N][N + 32]: [X | Psi] at the rank boundaries; [G + 1][N][32]: costates there
    cplx *ts_Yr = nullptr, *ts_Er = nullptr;
    struct qoc_comm* ts_comm = nullptr;

    // ---- buffers (one arena)
    cplx* HsP = nullptr;      // [k+1][N][N]
    cplx *A = nullptr, *P = nullptr, *K = nullptr, *A2 = nullptr;     // [B*SP][N][N]
    cplx* tree = nullptr;     // levels 1..L of the product tree: level l at tree_off[l], [B][SP >> l][N][N]
    size_t tree_off[8];
    cplx *Y0 = nullptr, *Y1 = nullptr;                               // [B][N][N+32]
    cplx* interP = nullptr;   // [B][SP][N][32]   Psi_t
    cplx* LamP = nullptr;     // [B][SP][N][32]   Lambda_t
    cplx* SrcP = nullptr;     // [B][SP][N][32]   S_tau (state regularisers only)
    cplx* zthin = nullptr;    // [N][32] zeros
    cplx *Psibnd = nullptr, *Ebnd = nullptr, *Aoff = nullptr;        // [B][NC][N][32] chunk-start Psi, chunk-end Lambda, affine offsets
    double* partial = nullptr; // [B*steps][k][N/32]
};

// Unitary mode: any n.  State transfer: psi <- P(B_t) psi is the same chain with K_t = sum_{j<T} B_t^j/j! (no squaring);
// the reference's backward step lambda <- P(-B_t) lambda (tensorflow_state.py:118-131) equals K_t^dagger lambda exactly
// when every generator is anti-Hermitian (-i dt H with H Hermitian), which `antiherm` certifies at create time.
// Any state-transfer problem with n <= 64, m <= 8 can instead run "direct" (k_gemm_taylor_chain: the reference's own
// mat-vec recursion, forward and backward, on pre-assembled generators; no time parallelism, so it is the large-batch mode).
static inline bool qoc_gemm_direct_supported(const QocDev& d) { return d.state_transfer && d.n <= 64 && d.m <= 8 && d.T >= 1; }
// the polynomial coefficient tables (ExpmCoef, qoc_inverse_factorials) hold 1/j! for j < QOC_GEMM_MAXT (the MFMA path stops at T = 22: this
// path takes over)
static inline bool qoc_gemm_supported(const QocDev& d, bool antiherm) {
    return d.m <= QOC_TW && d.T >= 1 && d.T <= QOC_GEMM_MAXT - 1 && (!d.state_transfer || antiherm || qoc_gemm_direct_supported(d));
}
// (qoc_all_antihermitian: qoc_common.h)

// this problem has state-regulariser sources S_tau in its costate recursion (forbidden levels, speed_up)
static inline bool qoc_has_state_sources(const QocDev& d) { return d.n_forb > 0 || d.has_speed; }
// the routes whose thin chains are kernels of their own (N <= 64, m <= 8): their gradient leaves per-tile partials of the wide layout
// (qoc_gemm_partials_gradient), which the engine's split tail can sum itself
static inline bool qoc_gemm_chain_routes(const QocGemm& gm) { return gm.route != QOC_GEMM_STEPWISE; }
// direct route without a state regulariser: backward chain beside the forward one (qoc_gemm_forward_direct)
static inline bool qoc_gemm_zfree_backward(const QocGemm& gm, const QocDev& d) {
    return gm.route == QOC_GEMM_DIRECT && !qoc_has_state_sources(d) && d.steps >= 2;
}
// stepwise route in unitary mode: final_state / unitary_scale are formed when they are read back (qoc_gemm_forward with_final) -- inside
// the iterations the boundary chain carries the m vectors only, not the N columns of X beside them (C5: 63 products of 512 x 544 columns
// per iteration)
static inline bool qoc_gemm_lazy_final(const QocGemm& gm, const QocDev& d) { return gm.route == QOC_GEMM_STEPWISE && !d.state_transfer; }

static inline QocGemmSwitches qoc_gemm_read_switches() {
    QocGemmSwitches sw;
    const char* e = qoc_exp_env("QOC_CHAIN_DPP");
    sw.no_chain_dpp = e && e[0] == '0';
    sw.no_active_columns = qoc_exp_is("QOC_DPP_ACTIVE_COLUMNS", 0);
    e = qoc_exp_env("QOC_ASM_OVERLAP");
    sw.no_overlap = e && e[0] == '0';
    e = qoc_exp_env("QOC_ASM_CUMASK");
    sw.no_cumask = e && e[0] == '0';
    if (e && atoi(e) > 0) sw.chain_cus = atoi(e);
    if (const char* t = qoc_exp_env("QOC_ASM_TAIL_WGS")) sw.tail_wgs = atoi(t) > 0 ? atoi(t) : 0;
    if (const char* t = qoc_exp_env("QOC_ASM_SPLIT16")) { sw.has_split16 = true; sw.split16 = atoi(t); }
    if (const char* t = qoc_exp_env("QOC_ASM_WINDOWS")) sw.windows = atoi(t) >= 2 ? (atoi(t) <= 4 ? atoi(t) : 4) : 2;
    return sw;
}

// The windows of the assembly overlap, with the chains on their own compute units (`masked`) or sharing them with the assembly.
// On shared CUs: 512 long-running workgroups from 5/16 of the pulse on -- the chain's prefetch shares the memory system with them (a slice
// costs it 4-5.6 us beside an unthrottled assembly against 2.9 alone); sweep of (workgroups, split) at C3 x 64, ms per iteration: (8192, 3/16)
// 6.81, (2048, 3/16) 6.79, (512, 5/16) 6.67, (512, 8/16) 6.77, (384, 6/16) 6.68, (256, 5/16) 7.35; one launch in front of the chain 7.03.
// On its own CUs the assembly runs unthrottled from 4/16 on (C3 x 64, ms per iteration: masks of 80 / 96 / 112 / 128 CUs for the chains
// 6.31 / 6.31 / 6.25 / 6.34; shared CUs 6.40; 2048 workgroups 6.27 - 6.31; 3/16: 6.35 - 6.50).
// [0, asm_split) in front, the rest in nw - 1 equal windows beside the chain.  More than two windows buy nothing (C3 x 64: 5.85 / 5.87 ms at
// nw = 2 / 4 with 4/16 in front, 5.83 with 2/16 and nw = 4: the chain part that runs beside an assembly launch loses what the shorter head
// saves) and nine or more chain launches waiting on events of the second stream did not finish at all on ROCm 7.2:
// profiles/r05_c3_windows.txt
static inline void qoc_gemm_overlap_windows(QocGemm& gm, const QocDev& d, bool masked) {
    gm.asm_split = ((masked ? 4 : 5) * d.steps) / 16;
    gm.asm_tail_wgs = gm.sw.tail_wgs > 0 ? gm.sw.tail_wgs : (masked ? 8192 : 512);
    if (gm.sw.has_split16) gm.asm_split = (gm.sw.split16 * d.steps) / 16;
    if (gm.asm_split < 1) gm.asm_split = 1;
    if (gm.asm_split > d.steps - 1) gm.asm_split = d.steps - 1;
    int nw = gm.sw.windows;
    if (nw - 1 > d.steps - gm.asm_split) nw = 1 + (d.steps - gm.asm_split);
    gm.asm_win.assign(1, 0);
    for (int w = 1; w <= nw; ++w)
        gm.asm_win.push_back(w == nw ? d.steps : gm.asm_split + (int)(((long long)(d.steps - gm.asm_split) * (w - 1)) / (nw - 1)));
}

// (a) The decision: route, flags and every size, from the problem, the engine's wishes (gm.antiherm, gm.direct_variant, gm.ts_G; `direct`:
// AUTO or the caller asked for the direct route), the experimental switches and the device's compute-unit count.  No HIP call, no allocation.
static inline void qoc_gemm_decide(QocGemm& gm, const QocDev& d, bool direct, int ncu) {
    const int N = ((d.n + 31) / 32) * 32;
    const bool chains = N <= 64 && d.m <= 8;
    gm.sw = qoc_gemm_read_switches();
    gm.N = N;
    gm.plan_scale = (double)d.Bplan / (double)d.B;
    gm.MV = d.m <= 1 ? 1 : (d.m <= 2 ? 2 : (d.m <= 4 ? 4 : 8));
    gm.route = !chains ? QOC_GEMM_STEPWISE : (direct && d.state_transfer ? QOC_GEMM_DIRECT : QOC_GEMM_PERSISTENT);
    gm.dpp_chain = gm.route == QOC_GEMM_DIRECT && N == 64 && gm.MV == 1 && !gm.sw.no_chain_dpp;
    gm.dpp_packed = gm.dpp_chain && gm.antiherm;
    // padded problems: the FMAs of a mat-vec shrink with the columns a wave owns (48 -> 30 / 36 / 42 DPP FMAs), the bytes of a slice to
    // 256 cw entries (cw = 10: the packed size); where 256 chains are bound by the generator bytes (> 128 control sets) the packed
    // image stays ahead for cw > 10
    gm.dpp_cw = 16;
    if (gm.dpp_chain && d.n <= 56 && d.k <= 8 && gm.direct_variant != 2 && !gm.sw.no_active_columns) {
        const int cw = d.n <= 40 ? 10 : (d.n <= 48 ? 12 : 14);
        if (!gm.dpp_packed || d.Bplan <= 128 || cw == 10) { gm.dpp_cw = cw; gm.dpp_packed = false; }
    }
    // opt-in only (qoc_config.variant = 2 with path = GEMM): measured SLOWER than the plain chain at C3 x 64 (7.98 against 5.83 ms per
    // iteration) -- see the header of qoc_gemm_chain_sq.h and profiles/EXPERIMENTS.md
    gm.sq_chain = gm.dpp_packed && qoc_sq_chain_terms_ok(d.T) && d.k >= 1 && d.k <= 8 && gm.direct_variant == 2;
    int L = 0;
    while (L < 6 && (1 << (2 * (L + 1))) <= d.steps) ++L;        // S = 2^L ~ sqrt(steps), at most 64
    // unitary chains get their chunk boundaries in log depth (k_gemm_scan_nodes), so a latency-bound launch (few (seed, chunk)
    // workgroups) prefers chunks half as long: C2 single trajectory 0.214 (S = 16) -> 0.198 ms (S = 8); 0.195 at S = 4
    if (chains && !d.state_transfer && !direct && L > 1 && (size_t)d.Bplan * ((d.steps + (1 << L) - 1) >> L) <= 64) --L;
    gm.L = L; gm.S = 1 << L;
    gm.NC = (d.steps + gm.S - 1) / gm.S;
    gm.SP = gm.NC * gm.S;
    if (gm.route == QOC_GEMM_DIRECT) { gm.L = 0; gm.S = d.steps; gm.NC = 1; gm.SP = d.steps; }   // one chunk, no padding, no tree
    gm.ldW = ((gm.SP * gm.MV + 31) / 32) * 32;
    size_t tree_elems = 0;
    for (int l = 1; l <= gm.L; ++l) { gm.tree_off[l] = tree_elems; tree_elems += (size_t)d.B * (gm.SP >> l) * N * N; }
    // wide gradient products: large matrices with few vectors (row tiles in pairs and column tiles in fours: what k_zgemm_wg takes)
    gm.wideW = (!chains && N >= 128 && (N / 32) % 2 == 0 && d.m <= QOC_WIDE_MV) ? (int)((((size_t)d.steps * QOC_WIDE_MV + 127) / 128) * 128) : 0;
    // the constant starts of the chains, once (one launch less per iteration)
    gm.init_once = chains && d.state_transfer && gm.ts_G <= 0;
    // the assembly overlap (256 chains fill the chip: 14.6 against 14.0 ms); disjoint CU sets for the two kernels that run beside each
    // other: the assembly's workgroups otherwise land on the chains' CUs as well and take issue slots from waves whose every instruction is
    // on the critical path
    gm.asm_split = 0; gm.mask_cus = 0;
    if (gm.dpp_chain && qoc_has_state_sources(d) && d.k <= 8 && d.steps >= 64 && d.B <= 128 && !gm.sw.no_overlap) {
        if (!gm.sw.no_cumask && ncu >= 128 && ncu <= 1024 && d.B + 16 <= gm.sw.chain_cus) gm.mask_cus = gm.sw.chain_cus;
        qoc_gemm_overlap_windows(gm, d, gm.mask_cus > 0);
    }
}

// (b) The arena.  Every work buffer is carved out of ONE allocation: with one hipMalloc per buffer the placement after earlier engines of
// the same process were freed decided the speed (n = 128 x 4: 8.6 or 17-20 ms per iteration for the same problem).  The order fixes every
// offset
static inline bool qoc_gemm_arena(QocGemm& gm, const QocDev& d, std::vector<void*>& allocs) {
    const int N = gm.N;
    const size_t NN = (size_t)N * N, BSP = (size_t)d.B * gm.SP, thin = (size_t)N * QOC_TW, C = sizeof(cplx);
    const size_t stack = (size_t)(d.k + 1) * NN * C, bnd = (size_t)d.B * gm.NC * thin * C, Y = (size_t)d.B * N * (N + QOC_TW) * C;
    const bool chains = qoc_gemm_chain_routes(gm), direct = gm.route == QOC_GEMM_DIRECT, persistent = gm.route == QOC_GEMM_PERSISTENT;
    const bool fused = N <= 64 && !direct;                       // k_gemm_expm_fused needs no A / A2 / ping-pong buffers
    const bool poly = N > 64;                                    // batched polynomial: A2 and ping-pong buffers
    size_t root_elems = 0, tree_elems = 0;
    for (int cnt = gm.NC; cnt > 1; cnt = (cnt + 1) / 2) root_elems += (size_t)d.B * ((cnt + 1) / 2) * NN;
    for (int l = 1; l <= gm.L; ++l) tree_elems += (size_t)d.B * (gm.SP >> l) * NN;
    const size_t sqP = (size_t)(d.k + 1) * (d.k + 2) / 2;
    struct Entry { void** p; size_t bytes; bool wanted; };
    const Entry entries[] = {
        {(void**)&gm.HsP, stack, true},
        {(void**)&gm.HsPT, gm.dpp_chain ? stack : 16, true},
        {(void**)&gm.A, BSP * (direct ? gm.gen_elems() : NN) * C, !fused},
        {(void**)&gm.P, BSP * NN * C, poly},
        {(void**)&gm.A2, BSP * NN * C, poly},
        {(void**)&gm.root, (persistent && !d.state_transfer) ? root_elems * C : 16, true},
        {(void**)&gm.K, direct ? 16 : BSP * NN * C, true},
        {(void**)&gm.tree, tree_elems * C, true},
        {(void**)&gm.KT, persistent ? BSP * NN * C : 16, true},
        {(void**)&gm.PcT, (persistent && gm.L > 0) ? (size_t)d.B * gm.NC * NN * C : 16, true},
        // (stepwise boundary products: one result slot per chunk step, read back by ONE k_gemm_take_bnd_all)
        {(void**)&gm.Y0, (chains ? 1 : gm.NC + 1) * Y, true},
        {(void**)&gm.Y1, chains ? Y : 16, true},
        {(void**)&gm.interP, BSP * thin * C, true},
        {(void**)&gm.LamP, BSP * thin * C, true},
        {(void**)&gm.Psibnd, bnd, true},
        {(void**)&gm.Ebnd, bnd, true},
        {(void**)&gm.Aoff, bnd, true},
        {(void**)&gm.zthin, thin * C, true},
        {(void**)&gm.partial, (size_t)d.B * d.k * (N / 32) * (chains ? (size_t)gm.ldW : (size_t)d.steps) * sizeof(double), true},
        {(void**)&gm.SrcP, BSP * thin * C, qoc_has_state_sources(d)},
        {(void**)&gm.HsSQ, sqP * QOC_DPP_PK_ELEMS * C, gm.sq_chain},
        {(void**)&gm.sqc, BSP * sqP * sizeof(double), gm.sq_chain},
        {(void**)&gm.wideP, (size_t)N * gm.wideW * C, gm.wideW > 0},
        {(void**)&gm.wideL, (size_t)N * gm.wideW * C, gm.wideW > 0},
        {(void**)&gm.wideC, (size_t)d.k * N * gm.wideW * C, gm.wideW > 0},
        {(void**)&gm.ts_Rall, (size_t)gm.ts_G * NN * C, gm.ts_G > 0},
        {(void**)&gm.ts_Rtmp, 2 * NN * C, gm.ts_G > 0},
        {(void**)&gm.ts_Yr, (size_t)(gm.ts_G + 1) * N * (N + QOC_TW) * C, gm.ts_G > 0},
        {(void**)&gm.ts_Er, (size_t)(gm.ts_G + 1) * thin * C, gm.ts_G > 0},
    };
    auto rounded = [](size_t bytes) { return ((bytes ? bytes : 16) + 4095) & ~(size_t)4095; };
    size_t total = 0;
    for (const Entry& e : entries) if (e.wanted) total += rounded(e.bytes);
    char* arena = nullptr;
    if (hipMalloc((void**)&arena, qoc_arena_bytes(total)) != hipSuccess) return false;
    allocs.push_back(arena);
    size_t off = 0;
    for (const Entry& e : entries) if (e.wanted) { *e.p = arena + off; off += rounded(e.bytes); }
    return true;
}

// (c) The host images of the Hamiltonian stack.
// entry (a, c) of an N x N matrix in the packed image: blocks of 16 x 16 on and below the block diagonal, column-major inside a block
static inline void qoc_gemm_pack_lower_blocks(cplx* packed, const cplx* M, int N) {
    for (int a = 0; a < N; ++a)
        for (int c = 0; c < N; ++c) {
            const int R = a >> 4, C = c >> 4;
            if (R >= C) packed[(size_t)(R * (R + 1) / 2 + C) * 256 + (size_t)(c & 15) * 16 + (a & 15)] = M[(size_t)a * N + c];
        }
}
// the stack zero-padded to N x N
static inline std::vector<cplx> qoc_gemm_padded_stack(const QocGemm& gm, const QocDev& d, const cplx* Hs_host) {
    const int N = gm.N;
    const size_t NN = (size_t)N * N;
    std::vector<cplx> hp((size_t)(d.k + 1) * NN);
    for (auto& v : hp) { v.x = 0; v.y = 0; }
    for (int kk = 0; kk <= d.k; ++kk)
        for (int a = 0; a < d.n; ++a)
            for (int c = 0; c < d.n; ++c) hp[(size_t)kk * NN + (size_t)a * N + c] = Hs_host[(size_t)kk * d.n * d.n + (size_t)a * d.n + c];
    return hp;
}
// dpp_chain: every matrix packed, or column-major -- the first 4 dpp_cw columns of it, or all of it
static inline std::vector<cplx> qoc_gemm_chain_stack(const QocGemm& gm, const QocDev& d, const std::vector<cplx>& hp) {
    const int N = gm.N;
    const size_t NN = (size_t)N * N, ge = gm.stack_elems() ? (size_t)gm.stack_elems() : NN;
    std::vector<cplx> ht((size_t)(d.k + 1) * ge);
    for (int kk = 0; kk <= d.k; ++kk) {
        if (gm.dpp_packed) { qoc_gemm_pack_lower_blocks(&ht[(size_t)kk * ge], &hp[(size_t)kk * NN], N); continue; }
        for (int a = 0; a < N; ++a)
            for (int c = 0; c < 4 * gm.dpp_cw; ++c) ht[(size_t)kk * ge + (size_t)c * N + a] = hp[(size_t)kk * NN + (size_t)a * N + c];
    }
    return ht;
}
// sq_chain: M_0 = A_0^2, M_k = A_0 A_k + A_k A_0, M_kl = A_k A_l + A_l A_k (k < l), M_kk = A_k^2 -- Hermitian, packed like the generators
static inline std::vector<cplx> qoc_gemm_squared_basis(const QocGemm& gm, const QocDev& d, const std::vector<cplx>& hp) {
    const int N = gm.N;
    const size_t NN = (size_t)N * N;
    std::vector<cplx> hq((size_t)(d.k + 1) * (d.k + 2) / 2 * QOC_DPP_PK_ELEMS);
    std::vector<cplx> prod(NN);
    auto accumulate = [&](int x, int y, bool clear) {                        // prod (+)= A_x A_y
        const cplx* X = &hp[(size_t)x * NN]; const cplx* Y = &hp[(size_t)y * NN];
        for (int a = 0; a < N; ++a)
            for (int c = 0; c < N; ++c) {
                double re = 0.0, im = 0.0;
                for (int j = 0; j < N; ++j) {
                    const cplx u = X[(size_t)a * N + j], v = Y[(size_t)j * N + c];
                    re += u.x * v.x - u.y * v.y; im += u.x * v.y + u.y * v.x;
                }
                cplx& o = prod[(size_t)a * N + c];
                if (clear) { o.x = re; o.y = im; } else { o.x += re; o.y += im; }
            }
    };
    int p = 0;
    auto pack = [&]() { qoc_gemm_pack_lower_blocks(&hq[(size_t)(p++) * QOC_DPP_PK_ELEMS], prod.data(), N); };
    accumulate(0, 0, true); pack();
    for (int kk = 1; kk <= d.k; ++kk) { accumulate(0, kk, true); accumulate(kk, 0, false); pack(); }
    for (int kk = 1; kk <= d.k; ++kk)
        for (int ll = kk; ll <= d.k; ++ll) { accumulate(kk, ll, true); if (ll != kk) accumulate(ll, kk, false); pack(); }
    return hq;
}
static inline bool qoc_gemm_upload_images(QocGemm& gm, const QocDev& d, const cplx* Hs_host) {
    const std::vector<cplx> hp = qoc_gemm_padded_stack(gm, d, Hs_host);
    if (hipMemcpy(gm.HsP, hp.data(), hp.size() * sizeof(cplx), hipMemcpyHostToDevice) != hipSuccess) return false;
    if (gm.dpp_chain) {
        const std::vector<cplx> ht = qoc_gemm_chain_stack(gm, d, hp);
        if (hipMemcpy(gm.HsPT, ht.data(), ht.size() * sizeof(cplx), hipMemcpyHostToDevice) != hipSuccess) return false;
    }
    if (gm.sq_chain) {
        const std::vector<cplx> hq = qoc_gemm_squared_basis(gm, d, hp);
        if (hipMemcpy(gm.HsSQ, hq.data(), hq.size() * sizeof(cplx), hipMemcpyHostToDevice) != hipSuccess) return false;
    }
    return true;
}

// (d) Clears and the two set-up kernels.
static inline int qoc_gemm_init_buffers(QocGemm& gm, const QocDev& d, std::string& msg) {
    const int N = gm.N;
    const size_t BSP = (size_t)d.B * gm.SP, thin = (size_t)N * QOC_TW, bnd = (size_t)d.B * gm.NC * thin;
    // the persistent chain kernels write only the first m (<= 8) of the 32 thin columns; the rest must read as zero
    bool zeroed = hipMemset(gm.zthin, 0, thin * sizeof(cplx)) == hipSuccess &&
                  hipMemset(gm.interP, 0, BSP * thin * sizeof(cplx)) == hipSuccess &&
                  hipMemset(gm.LamP, 0, BSP * thin * sizeof(cplx)) == hipSuccess &&
                  hipMemset(gm.Psibnd, 0, bnd * sizeof(cplx)) == hipSuccess &&
                  hipMemset(gm.Ebnd, 0, bnd * sizeof(cplx)) == hipSuccess &&
                  hipMemset(gm.Aoff, 0, bnd * sizeof(cplx)) == hipSuccess;
    // (wide buffers: the columns beyond 8 steps)
    if (gm.wideW > 0) zeroed = zeroed && hipMemset(gm.wideP, 0, (size_t)N * gm.wideW * sizeof(cplx)) == hipSuccess &&
                                         hipMemset(gm.wideL, 0, (size_t)N * gm.wideW * sizeof(cplx)) == hipSuccess;
    if (!zeroed) { msg = "GEMM path: clearing the work buffers failed"; return -2; }
    if (gm.init_once) {
        const size_t work = ((size_t)d.B * N * QOC_TW + 255) / 256;
        hipLaunchKernelGGL(k_gemm_chain_init, dim3((unsigned)(work > 65535 ? 65535 : work)), dim3(256), 0, 0, d, gm.Y0, gm.Psibnd, N, gm.NC, 0);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(0) != hipSuccess) {
            msg = "GEMM path: the chain starts could not be set";
            return -2;
        }
    }
    // the batched polynomial of ONE control set never computes the padded slices: K = I, once
    if (N > 64 && gm.SP > d.steps) {
        hipLaunchKernelGGL(k_gemm_pad_identity, dim3(4096), dim3(256), 0, 0, gm.K, d.B, N, d.steps, gm.SP);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(0) != hipSuccess) {
            msg = "GEMM path: the padded propagators could not be set";
            return -2;
        }
    }
    return 0;
}

// (e) Streams and events of the assembly overlap (asm_split > 0); qoc_gemm_teardown is its mirror.
static inline int qoc_gemm_overlap_streams(QocGemm& gm, const QocDev& d, int ncu, std::string& msg) {
    if (gm.asm_split <= 0) return 0;
    if (gm.mask_cus > 0) {
        std::vector<uint32_t> mc((ncu + 31) / 32, 0u), ma((ncu + 31) / 32, 0u);
        for (int c = 0; c < ncu; ++c) (c < gm.mask_cus ? mc : ma)[c / 32] |= 1u << (c % 32);
        if (hipExtStreamCreateWithCUMask(&gm.chain_s, (uint32_t)mc.size(), mc.data()) != hipSuccess) { gm.chain_s = nullptr; (void)hipGetLastError(); }
        else if (hipExtStreamCreateWithCUMask(&gm.aux, (uint32_t)ma.size(), ma.data()) != hipSuccess) {
            hipStreamDestroy(gm.chain_s);
            gm.chain_s = nullptr; gm.aux = nullptr;
            (void)hipGetLastError();
        }
        if (gm.chain_s && (hipEventCreateWithFlags(&gm.ev_fwd, hipEventDisableTiming) != hipSuccess ||
                           hipEventCreateWithFlags(&gm.ev_p1, hipEventDisableTiming) != hipSuccess)) {
            msg = "GEMM path: events could not be created";
            return -2;
        }
        if (!gm.chain_s) { gm.mask_cus = 0; qoc_gemm_overlap_windows(gm, d, false); }        // no masked streams: the windows of shared CUs
    }
    if ((!gm.aux && hipStreamCreateWithFlags(&gm.aux, hipStreamNonBlocking) != hipSuccess) ||
        hipEventCreateWithFlags(&gm.ev_ready, hipEventDisableTiming) != hipSuccess) {
        msg = "GEMM path: second stream / events could not be created";
        return -2;
    }
    const int nw = (int)gm.asm_win.size() - 1;
    gm.ev_win.assign(nw, nullptr);
    for (int w = 1; w < nw; ++w)
        if (hipEventCreateWithFlags(&gm.ev_win[w], hipEventDisableTiming) != hipSuccess) { msg = "GEMM path: events could not be created"; return -2; }
    return 0;
}
static inline void qoc_gemm_teardown(QocGemm& gm) {
    if (gm.aux) { hipStreamSynchronize(gm.aux); hipStreamDestroy(gm.aux); gm.aux = nullptr; }
    if (gm.chain_s) { hipStreamSynchronize(gm.chain_s); hipStreamDestroy(gm.chain_s); gm.chain_s = nullptr; }
    if (gm.ev_fwd) { hipEventDestroy(gm.ev_fwd); gm.ev_fwd = nullptr; }
    if (gm.ev_p1) { hipEventDestroy(gm.ev_p1); gm.ev_p1 = nullptr; }
    if (gm.ev_ready) { hipEventDestroy(gm.ev_ready); gm.ev_ready = nullptr; }
    for (auto& ev : gm.ev_win) if (ev) { hipEventDestroy(ev); ev = nullptr; }
}

static inline int qoc_gemm_setup(QocGemm& gm, const QocDev& d, const cplx* Hs_host, bool direct, std::vector<void*>& allocs, std::string& msg) {
    int ncu = 0, dv = 0;
    if (hipGetDevice(&dv) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dv) != hipSuccess) ncu = 0;
    qoc_gemm_decide(gm, d, direct, ncu);
    if (!qoc_gemm_arena(gm, d, allocs)) { msg = "GEMM path: out of device memory"; return -3; }
    if (!qoc_gemm_upload_images(gm, d, Hs_host)) { msg = "GEMM path: upload failed"; return -2; }
    if (const int rc = qoc_gemm_init_buffers(gm, d, msg)) return rc;
    return qoc_gemm_overlap_streams(gm, d, ncu, msg);
}
