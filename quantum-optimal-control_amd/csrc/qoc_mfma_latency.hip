// qoc_mfma_latency.hip -- translation unit of the latency-mode sweeps (qoc_mfma_latency.h), their resolver and their launchers.
#include <cstdlib>
#include "qoc_kernels_mfma.h"
#include "qoc_mfma_latency.h"

static size_t grad_lat_lds(int kc, int NT) { return (size_t)kc * 256 * NT * NT * sizeof(cplx) + (size_t)16 * 4 * 2 * kc * sizeof(double); }

const char* qoc_mfma_resolve_latency(QocMfmaPlan& p, const QocMfma& mf, const QocDev& d) {
    if (!mf.latency) return nullptr;
    const int NT = mf.NT;
    const unsigned gc = d.B * mf.C * mf.mq, gg = d.B * mf.NG * mf.mq;
    // the chunk offsets of the source recursion come out of the forward sweep itself when the sources need nothing but Psi (undressed forbidden
    // levels, no speed_up): its forward role leaves them
    p.sweep_offsets = mf.lat_src_fast && !mf.lat_dressed && !d.has_speed && d.n_forb > 0 && !mf.exp_lat_offsets_own;
    qoc_pick([&](auto NTc, auto DRESS) {
        // forward and z-free adjoint sweep side by side: 2 x (seed, chunk, group of 4 columns) workgroups of NT waves (one row tile each); with a
        // state regulariser on the batch kernels' recursion the forward half only (on the thin source sweeps both halves, Lambda0 is used)
        p.sweep_lat.set(k_mfma_sweep_lat<NTc>, (mf.lat_sources && !mf.lat_src_fast ? 1 : 2) * gc, 64 * NT);
        if (!mf.lat_src_fast) return;
        // fidelity + state-regulariser values straight from PsiL (instead of unpack + k_loss); then the source part of the costate: chunk offsets
        // (unless the sweep has left them), group offsets, the sweep that stores the total costate
        p.loss_lat.set(k_mfma_loss_lat<NTc, DRESS != 0>, d.B * ((d.steps + 1 + 15) / 16), 1024);
        if (!p.sweep_offsets) p.src_chunks.set(k_mfma_sweep_src<NTc, DRESS != 0>, gc, 64 * NT);
        p.src_groups.set(k_mfma_sweep_src<NTc, DRESS != 0>, gg, 64 * NT);
        p.src_total.set(k_mfma_sweep_src<NTc, DRESS != 0>, gc, 64 * NT);
    }, QocOneOf<2, 3, 4>{NT}, QocOneOf<1, 0>{mf.lat_dressed});
    if (!p.tail_fusable) return nullptr;                                // (the batch backward kernels: qoc_mfma_backward.hip)
    // the gradient: 16 / NT slices per workgroup, NT waves (row tiles) each; control images in LDS (16 KB each at NT = 2, 36 KB at NT = 3; NT = 4: two per pass)
    const int kc = d.k <= 4 ? 4 : (d.k == 5 ? 5 : 8), sl = 16 / NT;
    const unsigned g = d.B * ((d.steps + sl - 1) / sl), b = 64 * sl * NT;
    const QocOneOf<2, 4> mq{mf.mq <= 2 ? 2 : 4};
    if (NT == 4) qoc_pick([&](auto MQ) { p.grad_lat.set(k_mfma_grad_lat4<MQ>, g, b, grad_lat_lds(2, 4)); }, mq);
    else if (NT == 3) qoc_pick([&](auto MQ) { p.grad_lat.set(k_mfma_grad_lat<MQ, 4, 3>, g, b, grad_lat_lds(kc, 3)); }, mq);
    else qoc_pick([&](auto MQ, auto KC) { p.grad_lat.set(k_mfma_grad_lat<MQ, KC>, g, b, grad_lat_lds(kc, 2)); }, mq, QocOneOf<8, 5, 4>{kc});
    return p.grad_lat.reserve() ? nullptr : "MFMA path: cannot reserve LDS for the latency-mode gradient kernel";
}

void qoc_mfma_latency_sweeps(const QocMfmaPlan& p, const QocMfma& mf, const QocDev& d, hipStream_t s) {
    p.sweep_lat.run(s, d, mf, p.sweep_offsets);
    p.loss_lat.run(s, d, mf);
    p.sweep_unpack.run(s, d, mf, p.MQ);
}

// ap != nullptr: the tail of the iteration (k_finish_t<true>) runs inside, in the last workgroup of each seed
// (no bandpass regulariser: its DFT stays in the separate k_finish_t<false>)
void qoc_mfma_latency_gradient(const QocMfmaPlan& p, const QocMfma& mf, const QocDev& d, const QocAdamDev* ap, hipStream_t s) {
    p.src_chunks.run(s, d, mf, 0);                                      // (k_loss has run)
    p.src_groups.run(s, d, mf, 1);
    p.src_total.run(s, d, mf, 2);
    const bool local_regs = d.has_amp || d.has_env || d.has_dwdt || d.has_d2wdt2;
    const int fuse = (ap ? 1 : 0) | (mf.lat_src_fast ? 2 : 0) | (local_regs ? 4 : 0);
    p.grad_lat.run(s, d, mf, ap ? *ap : QocAdamDev{}, fuse);
}
