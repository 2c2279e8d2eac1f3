// qoc_gemm_routes.h -- an iteration of the GEMM path: qoc_gemm_expm, qoc_gemm_forward and qoc_gemm_backward dispatch over QocGemm::route to one
// function per route and phase, each the launch sequence of that route from top to bottom; what several routes launch alike is a named function
// above them.  qoc_gemm_ts.h (time shards) runs the stepwise pieces on sub-ranges of the slices.
#pragma once
#include "qoc_gemm_launch.h"

// ---- exponentials and the product tree -----------------------------------------------------------------------------------------------------
// pairwise product tree: T_l[i] = T_{l-1}[2i+1] * T_{l-1}[2i]  (later slice on the left), T_0 = K
// (item_first, item_count): the chunk-aligned run of (seed, slice) items whose tree is built -- all of them by default
static inline void qoc_gemm_tree(QocGemm& gm, const QocDev& d, hipStream_t s, size_t item_first = 0, size_t item_count = 0) {
    const int N = gm.N;
    const size_t NN = (size_t)N * N;
    if (item_count == 0) item_count = (size_t)d.B * gm.SP;
    GemmArgs g = qoc_gemm_square_args(N, 0);
    g.sA = g.sB = 2 * (long long)NN; g.sC = g.sCT = (long long)NN; g.ldct = N;
    const cplx* prev = gm.K;
    for (int l = 1; l <= gm.L; ++l) {
        cplx* out = gm.tree + gm.tree_off[l];
        g.A = prev + ((item_first >> (l - 1)) + 1) * NN; g.Bm = prev + (item_first >> (l - 1)) * NN; g.C = out + (item_first >> l) * NN;
        g.batch = (int)(item_count >> l);
        // chunk products also transposed, for the backward boundary chain of the persistent route
        g.CT = gm.route == QOC_GEMM_PERSISTENT && l == gm.L ? gm.PcT : nullptr;
        qoc_gemm_launch(gm, false, 0, g, s);
        prev = out;
    }
}
static inline const cplx* qoc_gemm_chunk_products(const QocGemm& gm) { return gm.L > 0 ? gm.tree + gm.tree_off[gm.L] : gm.K; }
// matvecexp sums j < T (tensorflow_state.py:88-96): the polynomial degree and the squarings of K_t
static inline int qoc_gemm_degree(const QocDev& d) { return d.state_transfer ? d.T - 1 : d.T; }
static inline int qoc_gemm_squarings(const QocDev& d) { return d.state_transfer ? 0 : d.s; }

// N <= 64: K_t (and, KT != nullptr, its transpose) of every (seed, slice) by one LDS-resident kernel
static inline void qoc_gemm_expm_fused(QocGemm& gm, const QocDev& d, hipStream_t s, cplx* KT) {
    const size_t lds = 2 * (size_t)gm.N * (gm.N + QOC_EXPM_LDPAD) * sizeof(cplx);
    const ExpmCoef cf = qoc_inverse_factorials();
    qoc_pick([&](auto N) {
        hipLaunchKernelGGL(k_gemm_expm_fused<N>, dim3((unsigned)((size_t)d.B * gm.SP)), dim3(N == 32 ? 128 : 512), lds, s, d, gm.HsP, gm.K, KT, gm.SP,
                           qoc_gemm_degree(d), qoc_gemm_squarings(d), cf);
    }, QocOneOf<32, 64>{gm.N});
}
// N > 64: K_t of the items [item_first, item_first + item_count) by batched launches (all items, or the slices of one rank of a
// time-sharded engine).  Taylor polynomial sum_{j<=T} A^j/j! (tensorflow_state.py:37-41) in Paterson-Stockmeyer form over A2 = A*A:
// S = B_m ; S = B_i + A2*S with B_i = c_{2i} I + c_{2i+1} A  (T = 5: 3 products instead of 4); then s squarings.
static inline void qoc_gemm_expm_products(QocGemm& gm, const QocDev& d, hipStream_t s, size_t item_first, size_t item_count) {
    const int N = gm.N, deg = qoc_gemm_degree(d), nsq = qoc_gemm_squarings(d);
    const size_t NN = (size_t)N * N, BS = item_count, off = item_first * NN;
    qoc_gemm_assemble_launch(d, gm.HsP, gm.A, N, gm.SP, nsq, s, item_first, item_count);
    cplx* const bufA = gm.A + off; cplx* const bufA2 = gm.A2 + off; cplx* const bufK = gm.K + off; cplx* const bufP = gm.P + off;
    GemmArgs g = qoc_gemm_square_args(N, (int)BS);
    g.lde = N; g.sA = g.sB = g.sC = g.sE = (long long)NN;
    const ExpmCoef cf = qoc_inverse_factorials();
    const double* invf = cf.c;
    const int mm = deg >> 1;
    const bool even = (deg & 1) == 0;
    const int horner = deg >= 2 ? (even ? mm - 1 : mm) : 0;      // products after A2
    const int products = horner + nsq;                           // buffer flips until the result
    cplx* cur = (products % 2 == 0) ? bufK : bufP;               // buffers alternate cur -> other on every product: the last lands in K
    cplx* oth = (products % 2 == 0) ? bufP : bufK;
    auto product = [&](const cplx* A, const cplx* Bm, cplx* C, const cplx* E, double beta, double gamma) {
        g.A = A; g.Bm = Bm; g.C = C; g.E = E; g.alpha = 1.0; g.beta = beta; g.gamma = gamma;
        qoc_gemm_launch(gm, false, 0, g, s);
    };
    auto top_block = [&](const cplx* A2, double c0, double c1, double cT) {
        hipLaunchKernelGGL(k_gemm_ps_init, dim3(gemm_grid(BS * NN)), dim3(256), 0, s, bufA, A2, cur, BS * NN, N, c0, c1, cT);
    };
    if (deg >= 2) {
        product(bufA, bufA, bufA2, nullptr, 0.0, 0.0);               // A2 = A*A
        // odd order on the workgroup-tiled kernel: the top block S = c_{2m} I + c_{2m+1} A is formed from A while the first Horner product
        // stages its right operand (GemmArgs::btrans) -- no k_gemm_ps_init pass (C5: 3.2 ms of reading and writing 8.4 GB each)
        const bool top_in_flight = !even && mm >= 1 && qoc_gemm_takes_wg(gm, g);
        if (even) top_block(bufA2, invf[2 * mm - 2], invf[2 * mm - 1], invf[deg]);
        else if (!top_in_flight) top_block(nullptr, invf[2 * mm], invf[2 * mm + 1], 0.0);
        for (int i = (even ? mm - 2 : mm - 1); i >= 0; --i) {    // S <- c_{2i} I + c_{2i+1} A + A2*S
            const bool first_in_flight = top_in_flight && i == mm - 1;
            if (first_in_flight) { g.btrans = 1; g.bt_c0 = invf[2 * mm]; g.bt_c1 = invf[2 * mm + 1]; }
            product(bufA2, first_in_flight ? bufA : cur, oth, bufA, invf[2 * i + 1], invf[2 * i]);
            g.btrans = 0;
            cplx* t = cur; cur = oth; oth = t;
        }
    } else {
        top_block(nullptr, 1.0, deg >= 1 ? 1.0 : 0.0, 0.0);
    }
    for (int sq = 0; sq < nsq; ++sq) {                       // M <- M M                    tensorflow_state.py:43-44
        product(cur, cur, oth, nullptr, 0.0, 0.0);
        cplx* t = cur; cur = oth; oth = t;
    }
}

// direct route: the chains apply the Taylor series themselves -- this is the assembly of their generators
static inline void qoc_gemm_expm_direct(QocGemm& gm, const QocDev& d, hipStream_t s) {
    const int N = gm.N, nn = gm.stack_elems();
    if (gm.sq_chain) {
        hipLaunchKernelGGL(k_gemm_sq_coefs, dim3(gemm_grid((size_t)d.B * d.steps)), dim3(256), 0, s, d, gm.sqc, gm.SP, (d.k + 1) * (d.k + 2) / 2);
        auto assemble = [&](int t0, int tn, hipStream_t st, int wgs) { qoc_gemm_assemble_sq(d, gm.HsPT, gm.HsSQ, gm.sqc, gm.A, gm.SP, t0, tn, st, wgs); };
        if (gm.asm_split > 0) qoc_gemm_assemble_windows(gm, s, assemble);
        else assemble(0, 0, s, 8192);
    } else if (gm.asm_split > 0) {
        qoc_gemm_assemble_windows(gm, s, [&](int t0, int tn, hipStream_t st, int wgs) { qoc_gemm_assemble_window(d, gm.HsPT, gm.A, N, gm.SP, t0, tn, st, wgs, nn); });
    } else {
        qoc_gemm_assemble_launch(d, gm.dpp_chain ? gm.HsPT : gm.HsP, gm.A, N, gm.SP, 0, s, 0, 0, nn);      // (dpp_chain: generators column-major)
    }
}
static inline void qoc_gemm_expm_persistent(QocGemm& gm, const QocDev& d, hipStream_t s) {
    qoc_gemm_expm_fused(gm, d, s, gm.KT);
    qoc_gemm_tree(gm, d, s);
}
static inline void qoc_gemm_expm_stepwise(QocGemm& gm, const QocDev& d, hipStream_t s) {
    // one control set: the padded slices (K = I exactly, written once by set-up) are not computed -- C5: 16 of 2016 slices, 96 products
    if (gm.N <= 64) qoc_gemm_expm_fused(gm, d, s, nullptr);
    else qoc_gemm_expm_products(gm, d, s, 0, d.B == 1 ? (size_t)d.steps : (size_t)d.B * gm.SP);
    qoc_gemm_tree(gm, d, s);
}
// K_t for all (seed, slice): the dominant part of the path (bracketed by the profiling events of the engine)
static inline void qoc_gemm_expm(QocGemm& gm, const QocDev& d, hipStream_t s) {
    switch (gm.route) {
        case QOC_GEMM_DIRECT: qoc_gemm_expm_direct(gm, d, s); break;
        case QOC_GEMM_PERSISTENT: qoc_gemm_expm_persistent(gm, d, s); break;
        case QOC_GEMM_STEPWISE: qoc_gemm_expm_stepwise(gm, d, s); break;
    }
}

// ---- forward --------------------------------------------------------------------------------------------------------------------------------
// Y0 = [U0 | Psi0] (xw = N columns of X, or 0: the vectors alone), Psibnd[b][0], inter[b][0] -- unless set-up did it once and for all
static inline void qoc_gemm_chain_starts(QocGemm& gm, const QocDev& d, hipStream_t s, int xw) {
    if (gm.init_once) return;
    hipLaunchKernelGGL(k_gemm_chain_init, dim3(gemm_grid((size_t)d.B * gm.N * (xw + QOC_TW))), dim3(256), 0, s, d, gm.Y0, gm.Psibnd, gm.N, gm.NC, xw);
}
static inline void qoc_gemm_unpad_wide(QocGemm& gm, const QocDev& d, hipStream_t s) {
    hipLaunchKernelGGL(k_gemm_unpad_wide, dim3(gemm_grid((size_t)d.B * d.steps * d.n * d.m)), dim3(256), 0, s, d, gm.interP, gm.N, gm.ldW, gm.MV);
}
static inline void qoc_gemm_take_final(QocGemm& gm, const QocDev& d, hipStream_t s, const cplx* Y) {
    hipLaunchKernelGGL(k_gemm_take_final, dim3(d.B), dim3(gm.N > 64 ? 1024 : 256), 0, s, d, Y, gm.N);
}

// psi_t = P(B_t) psi_{t-1} along the whole pulse, one chain per seed                      tensorflow_state.py:88-96 (direct route)
static inline ChainArgs qoc_gemm_direct_forward_args(const QocGemm& gm, const QocDev& d) {
    const int N = gm.N;
    const size_t thin = (size_t)N * QOC_TW, GE = gm.gen_elems();
    ChainArgs a = qoc_zeroed<ChainArgs>();
    a.K = gm.A; a.sKb = (long long)GE * gm.SP; a.sKs = (long long)GE;
    a.X0 = gm.Psibnd; a.sXb = (long long)thin;
    a.Out = gm.interP; a.sOb = (long long)N * gm.ldW; a.sOs = gm.MV; a.ldO = gm.ldW;
    a.CI = 1; a.len = d.steps; a.m = d.m; a.nterms = d.T; a.sign = 1.0;
    // the DPP chain writes inter[b][t + 1] itself (one vector: n contiguous entries per step)
    if (gm.dpp_chain) { a.Out2 = d.inter + d.n; a.sO2b = (long long)(d.steps + 1) * d.n; a.sO2s = d.n; a.n2 = d.n; }
    return a;
}
// lambda_{t-1} = P(-B_t) lambda_t + S_t   tensorflow_state.py:118-131 (direct route)
static inline ChainArgs qoc_gemm_direct_backward_args(const QocGemm& gm, const QocDev& d, bool sources) {
    const int N = gm.N;
    const size_t thin = (size_t)N * QOC_TW, GE = gm.gen_elems();
    ChainArgs a = qoc_zeroed<ChainArgs>();
    a.K = gm.A + (size_t)(d.steps - 1) * GE; a.sKb = (long long)GE * gm.SP; a.sKs = -(long long)GE;
    a.X0 = gm.Ebnd; a.sXb = (long long)thin;
    // (the DPP chain reads compact sources: one vector per step)
    if (sources && gm.dpp_chain) { a.E = gm.SrcP + (size_t)(d.steps - 1) * N; a.sEb = (long long)N * gm.SP; a.sEs = -(long long)N; a.ldE = 1; }
    else if (sources) { a.E = gm.SrcP + (size_t)(d.steps - 1) * thin; a.sEb = (long long)thin * gm.SP; a.sEs = -(long long)thin; }
    a.Out = gm.LamP + (long long)(d.steps - 2) * gm.MV; a.sOb = (long long)N * gm.ldW; a.sOs = -gm.MV; a.ldO = gm.ldW;
    a.store_initial = 1; a.CI = 1; a.len = d.steps - 1; a.m = d.m; a.nterms = d.T; a.sign = -1.0;
    return a;
}
// The forward chain of a direct route with the assembly overlap: one launch per window, each from the state the previous one left in
// Aoff; with a CU mask the chains keep their own CUs (the assembly of the later windows runs on the others) and the engine's stream
// joins after the last window
static inline void qoc_gemm_forward_windows(QocGemm& gm, const QocDev& d, hipStream_t s, const ChainArgs& a) {
    const size_t thin = (size_t)gm.N * QOC_TW;
    const int nw = (int)gm.asm_win.size() - 1;
    hipStream_t cs = gm.chain_s ? gm.chain_s : s;
    if (gm.chain_s) { hipEventRecord(gm.ev_fwd, s); hipStreamWaitEvent(cs, gm.ev_fwd, 0); }
    for (int w = 0; w < nw; ++w) {
        ChainArgs p = a;
        const int t0 = gm.asm_win[w];
        p.len = gm.asm_win[w + 1] - t0;
        if (w > 0) { p.X0 = gm.Aoff; p.sXb = (long long)thin; hipStreamWaitEvent(cs, gm.ev_win[w], 0); }
        if (w + 1 < nw) { p.Fin = gm.Aoff; p.sFb = (long long)thin; }
        p.K = a.K + (long long)t0 * a.sKs; p.Out = a.Out + (long long)t0 * a.sOs; p.Out2 = a.Out2 + (long long)t0 * a.sO2s;
        qoc_taylor_chain_launch(gm, p, nullptr, d.B, cs);
    }
    if (gm.chain_s) { hipEventRecord(gm.ev_p1, cs); hipStreamWaitEvent(s, gm.ev_p1, 0); }
}
static inline void qoc_gemm_forward_direct(QocGemm& gm, const QocDev& d, hipStream_t s) {
    const ChainArgs a = qoc_gemm_direct_forward_args(gm, d);
    qoc_gemm_chain_starts(gm, d, s, 0);
    if (qoc_gemm_zfree_backward(gm, d)) {
        // no state regulariser: the costate is linear in the overlap z -- the backward chain starts from -(2/m^2) W and runs
        // beside the forward one; qoc_gemm_backward_direct multiplies by z (C3 x 64: 13.2 -> 8 ms per iteration)
        const ChainArgs back = qoc_gemm_direct_backward_args(gm, d, false);
        hipLaunchKernelGGL(k_gemm_zfree_end, dim3(gemm_grid((size_t)d.B * gm.N * QOC_TW)), dim3(256), 0, s, d, gm.Ebnd, gm.N, gm.NC);
        qoc_taylor_chain_launch(gm, a, &back, d.B, s);
    }
    else if (gm.asm_split > 0) qoc_gemm_forward_windows(gm, d, s, a);
    else qoc_taylor_chain_launch(gm, a, nullptr, d.B, s);
    if (!gm.dpp_chain) qoc_gemm_unpad_wide(gm, d, s);
}

// persistent route, state transfer: chunk-start vectors Psibnd[c+1] = P_c Psibnd[c], one persistent workgroup per seed.  State transfer
// has no use for the upper product tree, and building it only for the scan costs more than the chain (C3: 0.58 vs 0.50 ms)
static inline void qoc_gemm_boundary_chain(QocGemm& gm, const QocDev& d, hipStream_t s) {
    const int N = gm.N, NC = gm.NC;
    const size_t NN = (size_t)N * N, thin = (size_t)N * QOC_TW;
    ChainArgs a = qoc_zeroed<ChainArgs>();
    a.K = qoc_gemm_chunk_products(gm); a.sKb = (long long)NN * NC; a.sKs = (long long)NN;
    a.X0 = gm.Psibnd; a.sXb = (long long)thin * NC;
    a.Out = gm.Psibnd + thin; a.sOb = (long long)thin * NC; a.sOs = (long long)thin; a.ldO = QOC_TW;
    a.CI = 1; a.len = NC - 1; a.m = d.m;
    qoc_chain_launch(gm, false, a, d.B, s);
}
// persistent route, unitary mode: the product tree continues above the chunk products (log2(NC) launches) -- its root gives final_state =
// (P_{NC-1} ... P_0) U0, its nodes give every chunk-boundary vector in log depth (k_gemm_scan_nodes).  Fills gm.scan for the backward pass
static inline void qoc_gemm_root_and_scan(QocGemm& gm, const QocDev& d, hipStream_t s) {
    const int N = gm.N, NC = gm.NC, ld = N + QOC_TW;
    const size_t NN = (size_t)N * N, thin = (size_t)N * QOC_TW;
    const cplx* lvl = qoc_gemm_chunk_products(gm);
    cplx* out = gm.root;
    ScanArgs& sc = gm.scan;
    sc = qoc_zeroed<ScanArgs>();
    sc.lvl[0] = lvl; sc.sLb[0] = (long long)NC * NN; sc.cnt[0] = NC; sc.levels = 1;
    GemmArgs r = qoc_gemm_square_args(N, 0);
    r.sA = r.sB = 2 * (long long)NN; r.sC = (long long)NN;
    for (int cnt = NC; cnt > 1; cnt = (cnt + 1) / 2) {
        const int pairs = cnt / 2, nxt = (cnt + 1) / 2;
        r.A = lvl + NN; r.Bm = lvl; r.C = out;
        r.inner = pairs; r.sA2 = r.sB2 = (long long)cnt * NN; r.sC2 = (long long)nxt * NN; r.batch = d.B * pairs;
        qoc_gemm_launch(gm, false, 0, r, s);
        if (cnt & 1)                                             // (the odd element of a level moves up unchanged)
            hipLaunchKernelGGL(k_gemm_copy_mats, dim3(gemm_grid((size_t)d.B * NN)), dim3(256), 0, s, out + (size_t)pairs * NN,
                               (long long)nxt * NN, lvl + (size_t)(cnt - 1) * NN, (long long)cnt * NN, d.B, (int)NN);
        if (sc.levels < 10) { sc.lvl[sc.levels] = out; sc.sLb[sc.levels] = (long long)nxt * NN; sc.cnt[sc.levels] = nxt; ++sc.levels; }
        lvl = out;
        out += (size_t)d.B * nxt * NN;
    }
    sc.NC = NC;
    GemmArgs y = qoc_gemm_boundary_args(N, ld, d.B, (long long)NN, (long long)N * ld);
    y.A = lvl; y.Bm = gm.Y0; y.C = gm.Y1;
    qoc_gemm_launch(gm, false, 0, y, s);
    qoc_gemm_take_final(gm, d, s, gm.Y1);
    // chunk-start vectors Psibnd[c] = P_{c-1} ... P_0 Psi0, c = 1 .. NC-1: one workgroup per (seed, chunk), <= log2(NC) nodes
    ScanArgs a = sc;
    a.X0 = gm.Psibnd; a.sXb = (long long)thin * NC;
    a.Out = gm.Psibnd; a.sOb = (long long)thin * NC; a.sOc = (long long)thin;
    a.c0 = 1; a.nchains = NC - 1; a.suffix = 0;
    qoc_scan_launch(gm, a, d.B, s);
}
static inline void qoc_gemm_forward_persistent(QocGemm& gm, const QocDev& d, hipStream_t s) {
    const int N = gm.N, S = gm.S, NC = gm.NC;
    const size_t NN = (size_t)N * N, thin = (size_t)N * QOC_TW;
    qoc_gemm_chain_starts(gm, d, s, d.state_transfer ? 0 : N);
    if (d.state_transfer) qoc_gemm_boundary_chain(gm, d, s);
    else qoc_gemm_root_and_scan(gm, d, s);
    // every chunk swept by its own persistent workgroup: Psi_{cS+j} = K_{cS+j} Psi_{cS+j-1}, into the time-major wide layout
    ChainArgs a = qoc_zeroed<ChainArgs>();
    a.K = gm.K; a.sKb = (long long)NN * gm.SP; a.sKc = (long long)NN * S; a.sKs = (long long)NN;
    a.X0 = gm.Psibnd; a.sXb = (long long)thin * NC; a.sXc = (long long)thin;
    a.Out = gm.interP; a.sOb = (long long)N * gm.ldW; a.sOc = (long long)S * gm.MV; a.sOs = gm.MV; a.ldO = gm.ldW;
    a.CI = NC; a.len = S; a.m = d.m;
    qoc_chain_launch(gm, false, a, d.B * NC, s);
    qoc_gemm_unpad_wide(gm, d, s);
}

// stepwise route, chunk boundaries: [X | Psi] <- P_c [X | Psi], one product per chunk (xw = N columns of X for final_state, or 0: the
// vectors alone); the chunk starts Psibnd from the thin blocks of all results at once                  tensorflow_state.py:214-238
static inline void qoc_gemm_boundary_products(QocGemm& gm, const QocDev& d, hipStream_t s, int xw) {
    const int N = gm.N, NC = gm.NC, ld = xw + QOC_TW;
    const size_t NN = (size_t)N * N, thin = (size_t)N * QOC_TW, yslot = (size_t)d.B * N * ld;
    const cplx* Pc = qoc_gemm_chunk_products(gm);                // [B][NC]
    qoc_gemm_chain_starts(gm, d, s, xw);
    GemmArgs g = qoc_gemm_boundary_args(N, ld, d.B, (long long)NN * NC, (long long)N * ld);
    for (int c = 0; c < NC; ++c) {
        g.A = Pc + (size_t)c * NN; g.Bm = gm.Y0 + (size_t)c * yslot; g.C = gm.Y0 + (size_t)(c + 1) * yslot;
        qoc_gemm_launch(gm, false, 0, g, s);
    }
    if (NC > 1) hipLaunchKernelGGL(k_gemm_take_bnd_all, dim3(gemm_grid((size_t)d.B * (NC - 1) * thin)), dim3(256), 0, s, d, gm.Y0, gm.Psibnd, N, NC, xw);
    if (xw > 0) qoc_gemm_take_final(gm, d, s, gm.Y0 + (size_t)NC * yslot);
}
// stepwise route, all chunks swept together: Psi_{cS+j} = K_{cS+j} Psi_{cS+j-1}, one launch per j, batch = B*NC
static inline void qoc_gemm_sweep_products(QocGemm& gm, const QocDev& d, hipStream_t s) {
    const int N = gm.N, S = gm.S, NC = gm.NC;
    const size_t NN = (size_t)N * N, thin = (size_t)N * QOC_TW;
    GemmArgs h = qoc_gemm_thin_args(N, d.B * NC, false);
    h.sA = (long long)NN * S; h.sC = (long long)thin * S;
    for (int j = 0; j < S; ++j) {
        h.A = gm.K + (size_t)j * NN;
        if (j == 0) { h.Bm = gm.Psibnd; h.sB = (long long)thin; }
        else { h.Bm = gm.interP + (size_t)(j - 1) * thin; h.sB = (long long)thin * S; }
        h.C = gm.interP + (size_t)j * thin;
        qoc_gemm_launch(gm, false, 0, h, s);
    }
    hipLaunchKernelGGL(k_gemm_unpad_inter, dim3(gemm_grid((size_t)d.B * d.steps * d.n * d.m)), dim3(256), 0, s, d, gm.interP, N, gm.SP);
}
// with_final: the read-back of final_state -- the boundary chain with X beside the vectors is all that is asked for
static inline void qoc_gemm_forward_stepwise(QocGemm& gm, const QocDev& d, hipStream_t s, bool with_final) {
    if (with_final) qoc_gemm_boundary_products(gm, d, s, d.state_transfer ? 0 : gm.N);
    else { qoc_gemm_boundary_products(gm, d, s, 0); qoc_gemm_sweep_products(gm, d, s); }
}
// with_final (stepwise route in unitary mode only, qoc_gemm_lazy_final): form final_state / unitary_scale of the last evaluation
static inline void qoc_gemm_forward(QocGemm& gm, const QocDev& d, hipStream_t s, bool with_final = false) {
    switch (gm.route) {
        case QOC_GEMM_DIRECT: qoc_gemm_forward_direct(gm, d, s); break;
        case QOC_GEMM_PERSISTENT: qoc_gemm_forward_persistent(gm, d, s); break;
        case QOC_GEMM_STEPWISE: qoc_gemm_forward_stepwise(gm, d, s, with_final); break;
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------------------
// sources S_tau (if any) and the costate at the end of the pulse; `cols` columns of a thin panel are written, `compact`: one vector per step
static inline void qoc_gemm_sources(QocGemm& gm, const QocDev& d, hipStream_t s, int cols, int compact) {
    hipLaunchKernelGGL(k_gemm_sources, dim3(gemm_grid((size_t)d.B * (qoc_has_state_sources(d) ? gm.SP : 1) * gm.N * cols)), dim3(256), 0, s, d, gm.SrcP,
                       gm.Ebnd, gm.N, gm.SP, gm.NC, cols, compact);
}
// gradients from the time-major wide layout: one product H_k' [Psi_0 ... Psi_{SP-1}] per control (batch = seeds), contracted column by
// column with conj(Lambda) (tensorflow_state.py:61-63) -- the columns [c_first, c_end) (multiples of 32) of it
static inline void qoc_gemm_wide_gradient(QocGemm& gm, const QocDev& d, hipStream_t s, int c_first, int c_end) {
    const int N = gm.N, tm = N / 32;
    const size_t NN = (size_t)N * N;
    GemmArgs h = qoc_gemm_dot_args(N, gm.ldW, (c_end - c_first) / 32);
    h.Bm = gm.interP + c_first; h.L = gm.LamP + c_first;
    h.partial = gm.partial + c_first; h.ldp = gm.ldW; h.partial_stride = tm * gm.ldW;         // partial[b][k][tile_m][column]
    // one launch for all (seed, control) pairs: batch index bt = b*k + kk -> A = H'_{kk+1}, Bm / L = buffers of seed b
    h.A = gm.HsP + NN; h.inner = d.k; h.sA = (long long)NN; h.sA2 = 0;
    h.sB = h.sL = 0; h.sB2 = h.sL2 = (long long)N * gm.ldW;
    h.batch = d.B * d.k;
    qoc_gemm_launch(gm, false, 2, h, s, (size_t)h.batch * tm * (gm.ldW / 32));
}
// the gradient of the chain routes: per-tile partial dots of the wide layout, summed here -- or by the engine's split tail (tail_sums_partials)
static inline void qoc_gemm_partials_gradient(QocGemm& gm, const QocDev& d, hipStream_t s, bool tail_sums_partials) {
    qoc_gemm_wide_gradient(gm, d, s, 0, gm.ldW);
    if (!tail_sums_partials)
        hipLaunchKernelGGL(k_gemm_grad_reduce_wide, dim3(gemm_grid((size_t)d.B * d.steps * d.k)), dim3(256), 0, s, d, gm.partial, gm.N / 32, gm.ldW, gm.MV);
}
// (the gradient products of the slices the chain has already left, on the second stream beside the rest of the chain, were built and
// measured: 6.19 against 6.17 ms at C3 x 64 -- the products slow the chain's prefetch as much as they save; profiles/EXPERIMENTS.md)
static inline void qoc_gemm_backward_direct(QocGemm& gm, const QocDev& d, hipStream_t s, bool tail_sums_partials) {
    if (qoc_gemm_zfree_backward(gm, d)) {
        // the chain ran beside the forward one from -(2/m^2) W: Lambda_t = z Lambda0_t
        hipLaunchKernelGGL(k_gemm_scale_lam, dim3(gemm_grid((size_t)d.B * gm.N * d.steps * gm.MV)), dim3(256), 0, s, d, gm.LamP, gm.N, gm.ldW, d.steps * gm.MV);
    } else {
        // (the Taylor chains read nothing but the MV vector slots of a thin panel)
        qoc_gemm_sources(gm, d, s, gm.MV, gm.dpp_chain ? 1 : 0);
        qoc_taylor_chain_launch(gm, qoc_gemm_direct_backward_args(gm, d, qoc_has_state_sources(d)), nullptr, d.B, s);
    }
    qoc_gemm_partials_gradient(gm, d, s, tail_sums_partials);
}
static inline void qoc_gemm_backward_persistent(QocGemm& gm, const QocDev& d, hipStream_t s, bool tail_sums_partials) {
    const int N = gm.N, S = gm.S, NC = gm.NC;
    const size_t NN = (size_t)N * N, thin = (size_t)N * QOC_TW;
    const bool sources = qoc_has_state_sources(d);
    qoc_gemm_sources(gm, d, s, QOC_TW, 0);
    ChainArgs sw = qoc_zeroed<ChainArgs>();                  // one chunk, backwards: Lambda_{t-1} = K_t^dagger Lambda_t + S_t, conj(K^T) = K^H
    sw.K = gm.KT + (size_t)(S - 1) * NN; sw.sKb = (long long)NN * gm.SP; sw.sKc = (long long)NN * S; sw.sKs = -(long long)NN;
    if (sources) { sw.E = gm.SrcP + (size_t)(S - 1) * thin; sw.sEb = (long long)thin * gm.SP; sw.sEc = (long long)thin * S; sw.sEs = -(long long)thin; }
    sw.CI = NC; sw.m = d.m;
    if (sources && NC > 1) {                                 // affine offsets a_c: every chunk run from a zero costate
        ChainArgs a = sw;
        a.len = S; a.Fin = gm.Aoff; a.sFb = (long long)thin * NC; a.sFc = (long long)thin;
        qoc_chain_launch(gm, true, a, d.B * NC, s);
    }
    if (!sources && !d.state_transfer) {
        // chunk-end costates E_c = P_{c+1}^H ... P_{NC-1}^H E_{NC-1}, log depth (unitary mode: the tree exists)
        ScanArgs a = gm.scan;
        a.X0 = gm.Ebnd + (size_t)(NC - 1) * thin; a.sXb = (long long)thin * NC;
        a.Out = gm.Ebnd; a.sOb = (long long)thin * NC; a.sOc = (long long)thin;
        a.c0 = 0; a.nchains = NC - 1; a.suffix = 1;
        qoc_scan_launch(gm, a, d.B, s);
    } else {
        // with sources the recursion is affine: E_{c-1} = P_c^dagger E_c + a_c, sequential
        ChainArgs a = qoc_zeroed<ChainArgs>();
        const cplx* PcT = gm.L > 0 ? gm.PcT : gm.KT;
        a.K = PcT + (size_t)(NC - 1) * NN; a.sKb = (long long)NN * NC; a.sKs = -(long long)NN;
        a.X0 = gm.Ebnd + (size_t)(NC - 1) * thin; a.sXb = (long long)thin * NC;
        if (sources) { a.E = gm.Aoff + (size_t)(NC - 1) * thin; a.sEb = (long long)thin * NC; a.sEs = -(long long)thin; }
        a.Out = gm.Ebnd + (long long)(NC - 2) * (long long)thin; a.sOb = (long long)thin * NC; a.sOs = -(long long)thin; a.ldO = QOC_TW;
        a.CI = 1; a.len = NC - 1; a.m = d.m;
        qoc_chain_launch(gm, true, a, d.B, s);
    }
    sw.X0 = gm.Ebnd; sw.sXb = (long long)thin * NC; sw.sXc = (long long)thin;
    sw.Out = gm.LamP + (long long)(S - 2) * gm.MV; sw.sOb = (long long)N * gm.ldW; sw.sOc = (long long)S * gm.MV; sw.sOs = -gm.MV; sw.ldO = gm.ldW;
    sw.store_initial = 1; sw.len = S - 1;
    qoc_chain_launch(gm, true, sw, d.B * NC, s);
    qoc_gemm_partials_gradient(gm, d, s, tail_sums_partials);
}

// one backward pass over all chunks in parallel: Lambda_{cS+j-1} = K_{cS+j}^dagger Lambda_{cS+j} + S_{cS+j}, j = S-1 .. 1;
// the j = 0 product (result belongs to the previous chunk's end) goes to `first_out` [B][NC] when requested
static inline void qoc_gemm_bwd_sweep(QocGemm& gm, const QocDev& d, hipStream_t s, bool sources, cplx* first_out) {
    const int N = gm.N, S = gm.S, NC = gm.NC;
    const size_t NN = (size_t)N * N, thin = (size_t)N * QOC_TW;
    GemmArgs g = qoc_gemm_thin_args(N, d.B * NC, true);
    g.sA = (long long)NN * S; g.sB = g.sE = (long long)thin * S;
    for (int j = S - 1; j >= (first_out ? 0 : 1); --j) {
        g.A = gm.K + (size_t)j * NN; g.Bm = gm.LamP + (size_t)j * thin;
        g.E = sources ? gm.SrcP + (size_t)j * thin : nullptr;
        if (j > 0) { g.C = gm.LamP + (size_t)(j - 1) * thin; g.sC = (long long)thin * S; }
        else { g.C = first_out; g.sC = (long long)thin; }
        qoc_gemm_launch(gm, true, 0, g, s);
    }
}
static inline void qoc_gemm_set_chunk_ends(QocGemm& gm, const QocDev& d, hipStream_t s, const cplx* Ebnd) {
    hipLaunchKernelGGL(k_gemm_set_chunk_ends, dim3(gemm_grid((size_t)d.B * gm.NC * gm.N * QOC_TW)), dim3(256), 0, s, d, gm.LamP, Ebnd, gm.N, gm.S, gm.NC);
}
// gradients of large problems (wideW > 0): per seed, the slices re-packed time-major, ONE product for all controls, column-block dots
static inline void qoc_gemm_gradient_wide_per_seed(QocGemm& gm, const QocDev& d, hipStream_t s) {
    const int N = gm.N, W = gm.wideW;
    const size_t thin = (size_t)N * QOC_TW;
    const GemmArgs h = qoc_gemm_controls_args(gm, d, W);
    for (int b = 0; b < d.B; ++b) {
        hipLaunchKernelGGL(k_gemm_to_wide, dim3(gemm_grid((size_t)d.steps * N * QOC_WIDE_MV)), dim3(256), 0, s, d,
                           (const cplx*)(gm.interP + (size_t)b * gm.SP * thin), (const cplx*)(gm.LamP + (size_t)b * gm.SP * thin), gm.wideP, gm.wideL, N, W,
                           d.steps);
        qoc_gemm_launch(gm, false, 0, h, s);
        hipLaunchKernelGGL(k_gemm_dot_wide, dim3((unsigned)(((size_t)d.k * d.steps + 3) / 4)), dim3(256), 0, s, d, b, (const cplx*)gm.wideC,
                           (const cplx*)gm.wideL, N, W, 0, d.steps);
    }
}
// gradients from the thin panels: for each control one batched product H_k' Psi_t contracted with conj(Lambda_t)   tensorflow_state.py:61-63
static inline void qoc_gemm_gradient_thin(QocGemm& gm, const QocDev& d, hipStream_t s) {
    const int N = gm.N;
    const size_t NN = (size_t)N * N, thin = (size_t)N * QOC_TW;
    GemmArgs h = qoc_gemm_dot_args(N, QOC_TW, 1);
    h.partial_stride = d.k * (N / 32);
    for (int b = 0; b < d.B; ++b) {
        h.batch = d.steps;
        h.Bm = gm.interP + (size_t)b * gm.SP * thin; h.sB = (long long)thin;
        h.L = gm.LamP + (size_t)b * gm.SP * thin; h.sL = (long long)thin;
        for (int kk = 0; kk < d.k; ++kk) {
            h.A = gm.HsP + (size_t)(kk + 1) * NN;
            h.partial = gm.partial + (size_t)b * d.steps * h.partial_stride;
            h.partial_offset = kk * (N / 32);
            qoc_gemm_launch(gm, false, 1, h, s);
        }
    }
    hipLaunchKernelGGL(k_gemm_grad_reduce, dim3(gemm_grid((size_t)d.B * d.steps * d.k)), dim3(256), 0, s, d, gm.partial, N / 32);
}
static inline void qoc_gemm_backward_stepwise(QocGemm& gm, const QocDev& d, hipStream_t s) {
    const int N = gm.N, NC = gm.NC;
    const size_t NN = (size_t)N * N, thin = (size_t)N * QOC_TW;
    const bool sources = qoc_has_state_sources(d);
    const cplx* Pc = qoc_gemm_chunk_products(gm);
    qoc_gemm_sources(gm, d, s, QOC_TW, 0);
    if (sources && NC > 1) {                                 // affine offsets a_c: every chunk run from a zero costate
        qoc_gemm_set_chunk_ends(gm, d, s, nullptr);
        qoc_gemm_bwd_sweep(gm, d, s, true, gm.Aoff);
    }
    // chunk-end costates: E_{c-1} = P_c^dagger E_c + a_c
    GemmArgs g = qoc_gemm_thin_args(N, d.B, true);
    g.sA = (long long)NN * NC; g.sB = g.sC = g.sE = (long long)thin * NC;
    for (int c = NC - 1; c >= 1; --c) {
        g.A = Pc + (size_t)c * NN; g.Bm = gm.Ebnd + (size_t)c * thin; g.C = gm.Ebnd + (size_t)(c - 1) * thin;
        g.E = sources ? gm.Aoff + (size_t)c * thin : nullptr;
        qoc_gemm_launch(gm, true, 0, g, s);
    }
    qoc_gemm_set_chunk_ends(gm, d, s, gm.Ebnd);
    qoc_gemm_bwd_sweep(gm, d, s, sources, nullptr);
    if (gm.wideW > 0) qoc_gemm_gradient_wide_per_seed(gm, d, s);
    else qoc_gemm_gradient_thin(gm, d, s);
}
// tail_sums_partials: the tail of this iteration is the engine's split tail summing the chain routes' gradient partials itself
static inline void qoc_gemm_backward(QocGemm& gm, const QocDev& d, hipStream_t s, bool tail_sums_partials) {
    switch (gm.route) {
        case QOC_GEMM_DIRECT: qoc_gemm_backward_direct(gm, d, s, tail_sums_partials); break;
        case QOC_GEMM_PERSISTENT: qoc_gemm_backward_persistent(gm, d, s, tail_sums_partials); break;
        case QOC_GEMM_STEPWISE: qoc_gemm_backward_stepwise(gm, d, s); break;
    }
}
