// qoc_mfma_expm_inplace.hip -- translation unit of k_mfma_expm_inplace (qoc_mfma_expm_inplace.h) and its resolver.
// Compiled with -mllvm -amdgpu-mfma-vgpr-form (__graft_entry__.UNIT_FLAGS): the accumulators of its products live in VGPRs.
#include "qoc_kernels_mfma.h"
#include "qoc_mfma_expm_inplace.h"

// variant 8 (after qoc_mfma_resolve_expm): 4 or 8 control images, even / odd Taylor degree, s = 0, active 4-row strips of the padded 32 x 32
// matrices: ceil(n / 4) (17 <= n <= 32: 5 .. 8)
void qoc_mfma_resolve_expm_inplace(QocMfmaPlan& p, const QocMfma& mf, const QocDev& d) {
    if (p.expm_variant != 8) return;
    qoc_pick([&](auto KC, auto EVEN, auto S0, auto QA) { p.expm.set(k_mfma_expm_inplace<KC, EVEN != 0, S0 != 0, QA>, d.B * mf.C, 64); },
             QocOneOf<4, 8>{d.k <= 4 ? 4 : 8}, QocOneOf<1, 0>{(d.T & 1) == 0}, QocOneOf<1, 0>{d.s == 0}, QocOneOf<8, 7, 6, 5>{qoc_active_strips(d.n)});
}
