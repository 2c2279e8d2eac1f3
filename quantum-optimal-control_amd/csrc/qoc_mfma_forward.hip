// qoc_mfma_forward.hip -- translation unit of the MFMA-path forward sweeps (qoc_mfma_forward.h), their resolver and their launchers.
#include "qoc_kernels_mfma.h"
#include "qoc_mfma_forward.h"

void qoc_mfma_resolve_forward(QocMfmaPlan& p, const QocMfma& mf, const QocDev& d) {
    const unsigned sw = d.B * mf.C, g = (sw + d.B * mf.NT + 3) / 4, gs = (sw + 3) / 4;     // (gs: sweep items only, final_state comes from the scan)
    const QocOneOf<2, 4> mq{mf.mq <= 2 ? 2 : 4};
    const bool fast = mf.variant != 1;                                  // the 4x4x4 sweeps; variant 1 keeps the 16x16x4 kernel (A/B)
    p.MQ = mq.v;
    p.inter_unpack.set(k_mfma_unpack_inter, 512, 256);
    if (mf.latency) {                                                    // the sweeps: qoc_mfma_latency.hip
        if (mf.lat_sources && !mf.lat_src_fast) p.sweep_unpack = p.inter_unpack;     // k_loss, the sources and the batch backward kernels read d.inter
        return;
    }
    if (mf.BndF) {
        // chunk boundaries once per seed (forward, and the z-free adjoint ones when the backward sweep takes them), then the sweep on the active
        // column groups ceil(n / 4) of K (NT = 2: 5 .. 8; 33 <= n <= 48: 9 .. 12 of the K padded to 48)
        const bool no_final = mf.updown || d.state_transfer;            // (state transfer has no final_state: tensorflow_state.py:244-261)
        const int adj = mf.BndA ? 1 : 0, waves = d.B * ((adj + 1) * mq.v + (no_final ? 0 : 4 * mf.NT));     // + the column blocks of final_state
        p.scan.set(mf.NT == 2 ? k_mfma_bnd_scan<2> : k_mfma_bnd_scan<3>, (waves + 3) / 4, 256);
        p.scan_flags = adj | (mf.updown ? 2 : 0) | (no_final ? 8 : 0);
        if (mf.NT == 2) qoc_pick([&](auto MQ, auto QA) { p.forward.set(k_mfma_forward2<2, MQ, true, QA>, gs, 256); }, mq, QocOneOf<5, 6, 7, 8>{qoc_active_strips(d.n)});
        else qoc_pick([&](auto MQ, auto QA) { p.forward.set(k_mfma_forward2<3, MQ, true, QA>, gs, 256); }, mq, QocOneOf<9, 10, 11, 12>{(d.n + 3) / 4});
        if (mf.updown) {
            // the forward sweep runs inside k_mfma_downup (after the adjoint one), which keeps no Psi_t: Psi_N for the loss comes from the scan, the
            // sweep runs when inter_vecs are read back, final_state = P_{C-1} ... P_0 U0 and unitary_scale are formed when they are
            p.inter_forward = p.forward;
            p.forward = {};
            p.inter_unpack = {};
            p.final_scan.set(k_mfma_bnd_scan<2>, (d.B * 4 * mf.NT + 3) / 4, 256);
            p.final_scan_flags = adj | 4;
            p.final_uscale.set(k_mfma_uscale, d.B, 64);
        }
    }
    // 4x4x4 sweeps; like the backward choice this must not depend on the batch size (bit-identical seeds across shardings)
    else if (mf.NT == 2 && fast) qoc_pick([&](auto MQ) { p.forward.set(k_mfma_forward2<2, MQ>, g, 256); }, mq);
    else if (mf.NT == 3 && fast) qoc_pick([&](auto MQ) { p.forward.set(k_mfma_forward2<3, MQ>, g, 256); }, mq);
    else if (mf.NT <= 3) qoc_pick([&](auto NT) { p.forward.set(k_mfma_forward<NT>, g, 256); }, QocOneOf<1, 2, 3>{mf.NT});
    // NT = 4: the active column groups ceil(n / 4) = 13 .. 16 of the K padded to 64
    else qoc_pick([&](auto QA) { p.forward.set(k_mfma_forward<4, QA>, g, 256); }, QocOneOf<13, 14, 15, 16>{(d.n + 3) / 4});
    if (!mf.updown && !d.state_transfer) p.uscale.set(k_mfma_uscale, d.B, 64);
}

void qoc_mfma_launch_forward(const QocMfmaPlan& p, const QocMfma& mf, const QocDev& d, hipStream_t s) {
    p.scan.run(s, d, mf, p.MQ, p.scan_flags, mf.PfT, mf.PfD, mf.C);
    p.forward.run(s, d, mf);
    if (!d.uscale_in_loss) p.uscale.run(s, d);
    qoc_mfma_latency_sweeps(p, mf, d, s);                               // (final_state only when read back: qoc_mfma_final_state)
}

void qoc_mfma_final_state_batch(const QocMfmaPlan& p, const QocMfma& mf, const QocDev& d, hipStream_t s) {
    QocDev dd = d;
    dd.skip_done = 0;                                                     // every seed's last evaluation is still in PfT
    p.final_scan.run(s, dd, mf, p.MQ, p.final_scan_flags, mf.PfT, mf.PfD, mf.C);
    p.final_uscale.run(s, dd);
}

// state transfer: unitary_scale of the last evaluation from Psi_N = d.inter[steps] (the routes whose loss is formed inside a sweep kernel), on
// read-back; one fixed launch, also the workgroup-resident path's (which has no plan)
void qoc_mfma_uscale_state_transfer(const QocDev& d, hipStream_t s) {
    QocDev dd = d;
    dd.skip_done = 0;
    hipLaunchKernelGGL(k_mfma_uscale_st, dim3(d.B), dim3(64), 0, s, dd);
}

void qoc_mfma_unpack_inter(const QocMfmaPlan& p, const QocMfma& mf, const QocDev& d, hipStream_t s) {
    p.inter_forward.run(s, d, mf);
    p.inter_unpack.run(s, d, mf, p.MQ);
}
