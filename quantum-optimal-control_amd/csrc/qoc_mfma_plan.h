// qoc_mfma_plan.h -- host side of the MFMA path: which kernel every launch of an iteration and of a read-back is, with what grid, block and
// dynamic LDS.  qoc_mfma_setup resolves all of it once (one resolver per translation unit, next to the kernels it picks from) and opts the
// picked kernels in for their LDS; the launchers walk the records.  QocMfma stays the kernels' argument; the plan lives beside it in the engine.
#pragma once
#include "qoc_pick.h"                 // QocOneOf / qoc_pick: the one idiom for the template ladders
#include "qoc_mfma_frag.h"

// one launch, typed by the kernel's argument list.  fn == nullptr: this engine never makes the launch
template <class... A> struct QocLaunch {
    void (*fn)(A...) = nullptr;
    dim3 grid, block;
    size_t lds = 0;
    void set(void (*f)(A...), unsigned g, unsigned b, size_t l = 0) { fn = f; grid = dim3(g); block = dim3(b); lds = l; }
    void run(hipStream_t s, const A&... a) const { if (fn) hipLaunchKernelGGL(fn, grid, block, lds, s, a...); }
    bool reserve() const { return !fn || !lds || hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess; }
};

struct QocMfmaPlan {
    using K1 = QocLaunch<QocDev>;
    using K2 = QocLaunch<QocDev, QocMfma>;
    using K3 = QocLaunch<QocDev, QocMfma, int>;
    using KScan = QocLaunch<QocDev, QocMfma, int, int, const cplx*, const cplx*, int>;
    using KChain = QocLaunch<QocDev, QocMfma, const cplx*, int, int, int, cplx*, int, const cplx*, cplx*>;
    using KGradLat = QocLaunch<QocDev, QocMfma, QocAdamDev, int>;
    // an iteration, in launch order.  qoc_mfma_launch_expm: K_t (batch kernels: with the chunk products), latency mode: chunk and group products
    K2 expm;
    KChain chain_chunks, chain_groups;
    // qoc_mfma_launch_forward: chunk boundaries, the sweep (none: it runs inside k_mfma_downup), unitary_scale unless k_loss forms it
    KScan scan;
    K2 forward;
    K1 uscale;
    // ... in latency mode (qoc_mfma_latency_sweeps): both sweeps, then the loss from PsiL or (batch backward kernels) d.inter for k_loss
    K3 sweep_lat;
    K2 loss_lat;
    K3 sweep_unpack;
    // qoc_mfma_launch_backward: chunk offsets of the source recursion, costates for the gradient kernel, group sweep, the sweep (by its
    // signature: k_mfma_backward3 / k_mfma_downup or k_mfma_backward), the slice-parallel gradient and the sum of its row-tile partials
    K2 offsets, costates, sweep_groups, sweep;
    K3 sweep1;
    K2 grad;
    K3 grad_sum;
    // qoc_mfma_latency_gradient: chunk offsets, group offsets and total costate of the source recursion, then the gradient (+ the fused tail)
    K3 src_chunks, src_groups, src_total;
    KGradLat grad_lat;
    // read-backs: qoc_mfma_final_state (latency mode), qoc_mfma_final_state_batch (k_mfma_downup), qoc_mfma_unpack_inter
    KChain final_chain;
    K2 final_unpack;
    KScan final_scan;
    K1 final_uscale;
    K3 inter_unpack;
    K2 inter_forward;
    // fixed integer arguments of these launches
    int MQ = 4, scan_flags = 0, final_scan_flags = 0, sweep_offsets = 0;
    // what the engine needs to know, by name
    bool engine_loss = true;           // the engine launches k_loss between the sweeps (else a sweep kernel forms the loss)
    bool tail_fusable = false;         // the gradient kernel can run the tail of the iteration (qoc_mfma_latency_gradient with Adam parameters)
    bool own_controls = false;         // the slice kernel forms its own controls
    bool uscale_in_loss = false;       // QocDev::uscale_in_loss of an iteration
    bool final_on_readback = false;    // final_state / unitary_scale are formed when read back ...
    bool final_from_groups = false;    //   ... by qoc_mfma_final_state (else qoc_mfma_final_state_batch)
    bool inter_on_readback = false;    // inter_vecs too (qoc_mfma_unpack_inter)
    const char* sweeps = "";           // qoc_plan_describe: sweeps=<word> expm=<number>
    int expm_variant = 1;
    int expm_hermitian = 0;            // in: 0, or with every Hamiltonian image exactly anti-Hermitian (qoc_mfma_setup) 1 / 2 (QOC_EXPM_HERM=2); out: what
                                       // k_mfma_expm_inplace runs (qoc_mfma_resolve_expm_inplace) -- 1: S S with copied accumulators, bit-identical to 0;
                                       // 2: the even/odd chain of symmetric products; qoc_plan_describe: expm_hermitian=<0|1|2>
    int mem_policy = 0;                // in: 1, or 0 with QOC_EXPERIMENTAL=1 QOC_MEM_POLICY=0 (qoc_mfma_setup); out: 1 when a kernel of the iteration runs its POL = 1
                                       // instance (k_mfma_expm_inplace: QOC_EXPM_KSTORE, k_mfma_downup: QOC_DOWNUP_*; built for k <= 4 only), else 0 -- plain
                                       // accesses.  Same bits either way; qoc_plan_describe: mem_policy=<0|1>
    const char* expm_name = "";        // qoc_profile_read
};
