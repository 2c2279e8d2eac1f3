// qoc_mfma_expm.hip -- translation unit of the MFMA-path exponential kernels (qoc_mfma_expm.h) and their launcher.
#include <cstdlib>
#include "qoc_kernels_mfma.h"
#include "qoc_mfma_expm.h"
#include "qoc_mfma_expm_stream.h"
#include "qoc_mfma_expm_pair.h"
#include "qoc_mfma_expm_rows.h"

// final_state = P_{C-1} ... P_0 U0 and unitary_scale (tensorflow_state.py:223-225) for the latency mode, where the sweeps do not
// form them: one chain over the group products and U0, then the unpack.  Called by the engine before a read-back.
__global__ void __launch_bounds__(64) k_mfma_unpack_final(QocDev d, QocMfma mf) {
    const int b = blockIdx.x, lane = threadIdx.x, n = d.n;
    const cplx* T = mf.TfD + (size_t)b * mf.FR;
    cplx* Xf = d.Xfinal + (size_t)b * n * n;
    const int QS = 4 * mf.NT;
    for (int f = 0; f < mf.NT * QS; ++f) {
        const int cb = f / QS, q = f - cb * QS, row = 4 * q + (lane >> 4), col = 16 * cb + (lane & 15);
        if (row < n && col < n) Xf[row * n + col] = T[f * 64 + lane];
    }
    __syncthreads();
    double part = 0.0;
    for (int c = lane; c < n; c += 64) {
        cplx rs = cmake(0.0, 0.0);
        for (int a = 0; a < n; ++a) rs = cadd(rs, Xf[c * n + a]);
        part += rs.x * rs.x + rs.y * rs.y;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
    if (lane == 0) d.uscale[b] = part / (double)n;
}
static const char* const qoc_expm_names[] = {"k_mfma_expm_chunk", "k_mfma_expm_chunk4", "k_mfma_expm_chunk4w", "k_mfma_expm_chunk4s",
    "k_mfma_expm_slice2 + k_mfma_chain_rows", "k_mfma_expm_pair", "k_mfma_expm_rows", "k_mfma_expm_inplace"};     // by variant 1 .. 8

// AUTO: NT = 2 with at least half of the 1024 SIMDs busy -> one wave per (seed, chunk) on v_mfma_f64_4x4x4 (0.92 vs 1.21 ms
// per launch at C2 x 64); NT = 1 and small launches keep the 16x16x4 kernel (C1: 0.072 vs 0.074 ms; one C2 trajectory:
// 0.67 vs 0.75 ms).  qoc_config.variant forces one of the kernels (parity tests, A/B runs): qoc_mfma_expm_variant.
template <int NT>
static void qoc_resolve_expm(QocMfmaPlan& p, const QocMfma& mf, const QocDev& d) {
    const int v = p.expm_variant;
    const unsigned items = d.B * mf.C, slices = d.B * d.steps;
    const QocOneOf<4, 8> kc{d.k <= 4 ? 4 : 8};                          // control images of the assembly
    if constexpr (NT >= 3) if (v == 5 || v == 7) {
        // n > 32: the row-block kernel, per chunk (7) or -- latency mode -- per slice (5; NT = 3: two workgroups per CU), on the active inner
        // strips ceil(n / 4) of the problem padded to 16 NT (4 NT - 3 .. 4 NT); QOC_ROWS_QA_FULL=1 (experimental switch): the padded problem in full
        const int qa = mf.exp_rows_qa_full ? 4 * NT : (d.n + 3) / 4;
        qoc_pick([&](auto KC, auto SLICE, auto QA) { p.expm.set(k_mfma_expm_rows<NT, KC, SLICE != 0, QA>, SLICE ? slices : items, 256, qoc_expm_rows_lds<NT>()); },
                 kc, QocOneOf<1, 0>{v == 5}, QocOneOf<4 * NT, 4 * NT - 1, 4 * NT - 2, 4 * NT - 3>{qa});
    }
    if constexpr (NT == 2) {
        // latency mode: K_t by two waves per slice (QOC_LAT_QA8=1, experimental: the padded problem in full)
        if (v == 5) qoc_pick([&](auto KC, auto QA) { p.expm.set(k_mfma_expm_slice2<KC, QA>, slices, 128); },
                             kc, QocOneOf<2, 4, 5, 6, 7, 8>{mf.exp_lat_qa8 ? 8 : qoc_active_strips_lat(d.n)});
        if (v == 6) qoc_pick([&](auto KC) { p.expm.set(k_mfma_expm_pair<KC>, items, 128); }, kc);
        if (v == 4) qoc_pick([&](auto KC) { p.expm.set(k_mfma_expm_chunk4s<2, KC>, items, 64); }, kc);
    }
    // (a run-time NT <= 2: never launched for NT = 3 / 4, but how the compiler inlines the helpers k_mfma_expm_chunk<NT> and k_mfma_expm_chunk4<NT>
    // share with it -- their registers and spills -- depends on k_mfma_expm_chunk4w<NT> being instantiated beside them)
    if (NT <= 2 && v == 3) p.expm.set(k_mfma_expm_chunk4w<NT>, items, 64);
    if (v == 2) p.expm.set(k_mfma_expm_chunk4<NT>, items, 64 * NT);
    if (!p.expm.fn && v != 8) p.expm.set(k_mfma_expm_chunk<NT>, items, 64 * NT);      // 1 (8: qoc_mfma_resolve_expm_inplace)
    if constexpr (NT >= 2) if (mf.latency) {
        // then the chunk products and the products of groups of G chunks (k_mfma_chain_rows2: the columns of the right operand split over the
        // waves of a workgroup -- 9.8 -> 8.5 us per launch at C2); final_state from the group products and U0 on read-back
        p.chain_chunks.set(k_mfma_chain_rows2<NT>, d.B * mf.C * 4 * NT, 64 * NT);
        p.chain_groups.set(k_mfma_chain_rows2<NT>, d.B * mf.NG * 4 * NT, 64 * NT);
        p.final_chain.set(k_mfma_chain_rows<NT>, d.B * 4 * NT, 64);
    }
}
const char* qoc_mfma_resolve_expm(QocMfmaPlan& p, const QocMfma& mf, const QocDev& d) {
    p.expm_variant = qoc_mfma_expm_variant(mf, d);
    p.expm_name = p.expm_variant == 5 && mf.NT == 3 ? "k_mfma_expm_rows (per slice) + k_mfma_chain_rows" : qoc_expm_names[p.expm_variant >= 2 && p.expm_variant <= 8 ? p.expm_variant - 1 : 0];
    qoc_pick([&](auto NT) { qoc_resolve_expm<NT>(p, mf, d); }, QocOneOf<1, 2, 3, 4>{mf.NT});
    if (mf.latency) p.final_unpack.set(k_mfma_unpack_final, d.B, 64);
    return p.expm.reserve() ? nullptr : "MFMA path: cannot reserve LDS for the row-block exponential kernel";
}
void qoc_mfma_launch_expm(const QocMfmaPlan& p, const QocMfma& mf, const QocDev& d, hipStream_t s) {
    p.expm.run(s, d, mf);
    p.chain_chunks.run(s, d, mf, mf.KfD, 1, d.steps, mf.L, mf.PfD, mf.C, nullptr, mf.PfT);
    p.chain_groups.run(s, d, mf, mf.PfD, 0, mf.C, mf.G, mf.GfD, mf.NG, nullptr, mf.GfT);
}

void qoc_mfma_final_state(const QocMfmaPlan& p, const QocMfma& mf, const QocDev& d, hipStream_t s) {
    QocDev dd = d;
    dd.skip_done = 0;                                                     // every seed's last evaluation is still in GfD
    p.final_chain.run(s, dd, mf, mf.GfD, 0, mf.NG, mf.NG, mf.TfD, 1, mf.U0fD, nullptr);
    p.final_unpack.run(s, dd, mf);
}
