// qoc_mfma_expm_inplace.hip -- translation unit of k_mfma_expm_inplace (qoc_mfma_expm_inplace.h) and its resolver.
// Compiled with -mllvm -amdgpu-mfma-vgpr-form (__graft_entry__.UNIT_FLAGS): the accumulators of its products live in VGPRs.
#include "qoc_kernels_mfma.h"
#include "qoc_mfma_expm_inplace.h"

// variant 8 (after qoc_mfma_resolve_expm): 4 or 8 control images, even / odd Taylor degree, s = 0, active 4-row strips of the padded 32 x 32
// matrices: ceil(n / 4) (17 <= n <= 32: 5 .. 8)
// p.expm_hermitian on entry: 0, or what the set-up allows after it found every Hamiltonian image exactly anti-Hermitian -- 1: S S with copied
// accumulators (bit-identical results), 2 (QOC_EXPM_HERM=2): the even/odd chain of symmetric products.  Both are built for Taylor order 5 on all 8
// strips (29 <= n <= 32); every other problem keeps the plain Horner chain.  On return: what the engine runs.
void qoc_mfma_resolve_expm_inplace(QocMfmaPlan& p, const QocMfma& mf, const QocDev& d) {
    const int herm = (p.expm_variant == 8 && d.T == 5 && qoc_active_strips(d.n) == 8) ? p.expm_hermitian : 0;
    p.expm_hermitian = herm;
    // p.mem_policy on entry: the request; the POL = 1 instances (the K_t stores under QOC_EXPM_KSTORE) exist for KC = 4 and only when the knob is not PLAIN
    const int pol = (p.expm_variant == 8 && qoc_expm_has_policy && d.k <= 4) ? p.mem_policy : 0;
    p.mem_policy = pol;                                                   // (the sweep's resolver adds its own)
    if (p.expm_variant != 8) return;
    qoc_pick([&](auto KC, auto EVEN, auto S0, auto QA, auto HERM, auto POL) {
        if constexpr (HERM != 0 && (EVEN != 0 || QA != 8)) return;        // (never picked: herm implies order 5 and QA = 8)
        else if constexpr (POL != 0 && (!qoc_expm_has_policy || KC != 4)) return;      // (never picked)
        else p.expm.set(k_mfma_expm_inplace<KC, EVEN != 0, S0 != 0, QA, HERM, POL>, d.B * mf.C, 64);
    }, QocOneOf<4, 8>{d.k <= 4 ? 4 : 8}, QocOneOf<1, 0>{(d.T & 1) == 0}, QocOneOf<1, 0>{d.s == 0}, QocOneOf<8, 7, 6, 5>{qoc_active_strips(d.n)}, QocOneOf<1, 2, 0>{herm},
       QocOneOf<1, 0>{pol});
}
