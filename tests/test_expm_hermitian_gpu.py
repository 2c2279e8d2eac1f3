"""What k_mfma_expm_inplace makes of exactly anti-Hermitian generators (csrc/qoc_mfma_expm_inplace.h, HERM), against the CPU oracle.

With Taylor order 5 on all eight 4-row strips (29 <= n <= 32) and Hamiltonian images that are anti-Hermitian entry for entry the kernel runs
  mode 1 (the default): the Horner chain whose first product S S copies the accumulators a = sum re re and b = sum im im of its lower left quarter from
          the upper right one -- the same products summed in the same order, so every result is BIT-IDENTICAL to the plain chain's;
  mode 2 (QOC_EXPERIMENTAL=1 QOC_EXPM_HERM=2): p(S) = E(S^2) + S O(S^2) as three products whose lower left quarter is mirrored instead of multiplied --
          the same polynomial with other roundings.
Every other problem, and every problem with one entry out of place, keeps the plain Horner chain (mode 0; QOC_EXPM_HERM=0 forces it).
qoc_plan_describe reports the mode (expm_hermitian=<0|1|2>).

All cases: MFMA path, variant 8, chunks pinned to 2, 2 control sets, 7 slices -- chunks of 4 and 3 slices: the slice assembled in the open, the steady
state and an odd tail.  Tolerances (tests/test_hip_parity.py): 1e-12 x max|entry| for loss, final unitary and inter_vecs, 1e-11 x max|g| for the gradient.
Reference semantics: core/tensorflow_state.py:25-46 (matexp), :204-242 (chain), :49-65 (gradient).
"""
import numpy as np
import pytest

from oracle import grape_oracle as go
from tests.golden import cases
from tests.helpers import oracle_system

pytestmark = pytest.mark.gpu

U_ATOL, G_RTOL, S_RTOL = 1e-12, 1e-11, 1e-12
MFMA, STEPS, SETS = 2, 7, 2


def case(n=32, k=4, m=8, taylor=(5, 3), seed=0):
    return cases.case_c2(n=n, k=k, steps=STEPS, m=m, taylor=taylor, seed=seed)


def make_engine(sp, Hs=None, ensemble=None):
    from quantum_optimal_control.core import hip_engine
    return hip_engine.HipEngine(sp.Hs if Hs is None else Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling,
                                reg_coeffs={}, n_seeds=SETS, path=MFMA, chunks=2, variant=8, ensemble=ensemble)


def bases_for(sp, seed=11):
    rng = np.random.default_rng(seed)
    return [sp.base0, 2.0 * rng.normal(size=sp.base0.shape) / np.sqrt(sp.steps) - 0.2]


@pytest.fixture(params=[1, 2], ids=['copied_accumulators', 'even_odd_chain'])
def mode(request, monkeypatch):
    """The mode an engine with anti-Hermitian images, order 5 and 29 <= n <= 32 runs: the default, or the even/odd chain behind its switch (read when the
    engine is created)."""
    if request.param == 2:
        monkeypatch.setenv('QOC_EXPERIMENTAL', '1')
        monkeypatch.setenv('QOC_EXPM_HERM', '2')
    return request.param


def assert_kernel(eng, mode):
    assert eng.path == MFMA and eng.chunks == 2 and eng.plan['expm'] == '8', eng.plan
    assert eng.plan['expm_hermitian'] == str(int(mode)), eng.plan


def check_against_oracle(eng, sp, bases):
    r = eng.evaluate()
    inter, Uf = eng.get_inter_vecs(), eng.get_final_unitary()
    for b, base in enumerate(bases):
        o = go.evaluate(sp, base, want_inter=True)
        gmax = np.max(np.abs(o['grad']))
        figures = (abs(r['loss'][b] - o['loss']), np.max(np.abs(r['grad'][b] - o['grad'])) / gmax, np.max(np.abs(Uf[b] - o['U_final'])),
                   np.max(np.abs(inter[b] - o['inter_vecs'])))
        print('  set %d: |loss - oracle| %.2e  gradient %.2e of max|g| = %.2e  U_final %.2e  inter_vecs %.2e' % ((b,) + figures[:2] + (gmax,) + figures[2:]))
        assert figures[0] <= S_RTOL * max(1.0, abs(o['loss'])), ('loss', b, r['loss'][b], o['loss'])
        assert figures[1] <= G_RTOL, ('grad', b, figures[1], gmax)
        assert figures[2] <= U_ATOL * max(1.0, np.max(np.abs(o['U_final']))), ('U_final', b, figures[2])
        assert figures[3] <= U_ATOL * max(1.0, np.max(np.abs(o['inter_vecs']))), ('inter_vecs', b, figures[3])
    return r, Uf


def run_case(c, hermitian):
    sp = oracle_system(c)
    bases = bases_for(sp)
    eng = make_engine(sp)
    try:
        assert_kernel(eng, hermitian)
        eng.set_base(np.stack(bases))
        check_against_oracle(eng, sp, bases)
    finally:
        eng.close()


# ---- the chain itself -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('taylor', [(5, 3), (5, 1), (5, 0)], ids=['s3', 's1', 's0'])
def test_symmetric_products_at_full_size(taylor, mode):
    """n = 32, k = 4, m = 8: the bench shape; squarings behind the polynomial (mode 2: read-back into SA), one squaring, and none (the last polynomial product stores K_t itself)."""
    run_case(case(taylor=taylor), mode)


def test_padding_inside_the_mirrored_quarter(mode):
    """n = 29: all eight strips are active, and rows and columns 29 .. 31 of the mirrored quarter are padding."""
    run_case(case(n=29, seed=3), mode)


@pytest.mark.parametrize('n', [20, 17])
def test_five_strip_problems_keep_the_horner_chain(n, mode):
    """QA = 5 (one half group): the symmetric products are instantiated for QA = 8 only, so these run the Horner chain -- parity either way."""
    run_case(case(n=n, seed=4), 0)


def test_six_controls_take_the_wide_assembly(mode):
    """k = 6: the KC = 8 instances."""
    run_case(case(k=6, seed=5), mode)


@pytest.mark.parametrize('T', [3, 4, 6, 7])
def test_other_taylor_orders_keep_the_horner_chain(T, mode):
    run_case(case(taylor=(T, 3), seed=6), 0)


def structured(kind):
    c = case(seed=7)
    n = len(c['H0'])
    rng = np.random.default_rng(70)
    sym = lambda: (lambda a: (a + a.T) / 2)(rng.normal(size=(n, n)))
    skew = lambda: (lambda a: a - a.T)(rng.normal(size=(n, n)) / 2)
    scale = lambda h: np.max(np.abs(h))
    if kind == 'real_symmetric':              # -i dt H has no real part at all
        c['H0'] = (scale(c['H0']) * sym()).astype(complex)
        c['Hops'] = [(scale(h) * sym()).astype(complex) for h in c['Hops']]
    elif kind == 'imaginary_offdiagonal':     # H = real diagonal + i (A - A^T): -i dt H is real antisymmetric off the diagonal
        c['H0'] = np.diag(rng.normal(size=n)).astype(complex) * scale(c['H0']) + 1j * scale(c['H0']) * skew()
        c['Hops'] = [np.diag(rng.normal(size=n)).astype(complex) * scale(h) + 1j * scale(h) * skew() for h in c['Hops']]
    else:                                     # diagonal drift, dense controls
        c['H0'] = np.diag(np.real(np.diag(c['H0']))).astype(complex)
    return c


@pytest.mark.parametrize('kind', ['real_symmetric', 'imaginary_offdiagonal', 'diagonal_drift'])
def test_structured_hamiltonians(kind, mode):
    """A wrong sign or a missing conjugate in one of the mirrors shows where one plane of S vanishes."""
    run_case(structured(kind), mode)


# ---- the guard ------------------------------------------------------------------------------------------------------------------------------

def test_non_hermitian_drift_keeps_the_horner_chain(mode):
    """H0 + 1e-3 i G with G Hermitian: accepted in unitary mode, run on the Horner chain, same oracle."""
    c = case(seed=8)
    rng = np.random.default_rng(80)
    g = rng.normal(size=c['H0'].shape) + 1j * rng.normal(size=c['H0'].shape)
    c['H0'] = c['H0'] + 1e-3j * (g + g.conj().T) / 2
    run_case(c, 0)


def test_one_ulp_of_asymmetry_keeps_the_horner_chain(mode):
    """ONE off-diagonal entry of one control image moved by one ulp: the guard is entry for entry, without a tolerance."""
    sp = oracle_system(case(seed=9))
    eng = make_engine(sp)
    assert_kernel(eng, mode)
    eng.close()
    for part in ('real', 'imag'):
        Hs = np.array(sp.Hs)
        v = Hs[2][3, 17]
        Hs[2][3, 17] = complex(np.nextafter(v.real, np.inf), v.imag) if part == 'real' else complex(v.real, np.nextafter(v.imag, np.inf))
        assert Hs[2][3, 17] != v
        eng = make_engine(sp, Hs=Hs)
        try:
            assert_kernel(eng, 0)
        finally:
            eng.close()


def test_non_hermitian_perturbation_of_an_ensemble_keeps_the_horner_chain(mode):
    """The perturbation images of a robust ensemble are among the images the kernel assembles from."""
    from quantum_optimal_control.helper_functions.synthetic_systems import herm
    sp = oracle_system(case(seed=10))
    rng = np.random.default_rng(100)
    p = 0.3 * herm(rng, sp.n)
    ens = dict(offsets=np.array([[0.1], [-0.1]]), amp_scales=np.ones((2, sp.k)), weights=np.array([0.5, 0.5]))
    for operator, hermitian in ((p, mode), (p + 1e-3j * herm(rng, sp.n), 0)):
        eng = make_engine(sp, ensemble=dict(ens, operators=[operator]))
        try:
            assert_kernel(eng, hermitian)
            assert eng.plan['members'] == '2' and eng.plan['perturbations'] == '1', eng.plan
        finally:
            eng.close()


# ---- both chains in one process, and the device loop ----------------------------------------------------------------------------------------

def test_modes_against_the_plain_chain(monkeypatch):
    """QOC_EXPERIMENTAL=1 QOC_EXPM_HERM=0 / 2 (read when the engine is created) against the default, same inputs, one process.  The default (copied
    accumulators) is bit-identical to the plain Horner chain in everything read back, also after three iterations of the device loop.  The even/odd chain
    agrees with it to 1e-13 relative in final unitary and gradient, and its final unitary is no further from unitary than ten times the plain chain's."""
    sp = oracle_system(case(seed=0))
    bases = bases_for(sp)
    conv = dict(rate=0.01, learning_rate_decay=2500, conv_target=1e-8, min_grad=1e-25, max_iterations=3)
    out = {}
    for m in (1, 0, 2):
        if m != 1:
            monkeypatch.setenv('QOC_EXPERIMENTAL', '1')
            monkeypatch.setenv('QOC_EXPM_HERM', str(m))
        eng = make_engine(sp)
        try:
            assert_kernel(eng, m)
            eng.set_base(np.stack(bases))
            r, Uf = check_against_oracle(eng, sp, bases)
            inter = eng.get_inter_vecs()
            eng.iterate(eng.adam_params(poll_every=3, **conv), 3)
            eng.sync()
            out[m] = (r, Uf, inter, eng.get_base(), eng.evaluate()['grad'])
        finally:
            eng.close()
    (r1, U1, i1, b1, g1), (r0, U0, i0, b0, g0), (r2, U2) = out[1], out[0], out[2][:2]
    for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale', 'grad'):
        assert np.array_equal(r1[key], r0[key]), key
    assert np.array_equal(U1, U0) and np.array_equal(i1, i0) and np.array_equal(b1, b0) and np.array_equal(g1, g0)
    gd, ud = np.max(np.abs(r2['grad'] - r0['grad'])) / np.max(np.abs(r0['grad'])), np.max(np.abs(U2 - U0)) / np.max(np.abs(U0))
    defect = lambda U: max(np.linalg.norm(u.conj().T @ u - np.eye(sp.n)) for u in U)
    print('  even/odd against plain: gradient %.2e  U_final %.2e  |U^dagger U - I| %.2e against %.2e' % (gd, ud, defect(U2), defect(U0)))
    assert gd <= 1e-13 and ud <= 1e-13, (gd, ud)
    assert defect(U2) <= 10 * defect(U0), (defect(U2), defect(U0))


def test_three_iterations_of_the_device_loop(mode):
    """qoc_iterate on the new kernels against the oracle's loop (core/run_session.py:47-69), as tests/test_bench_config_parity.py does at full size."""
    sp = oracle_system(case(seed=12))
    bases = bases_for(sp)
    conv = dict(rate=0.01, learning_rate_decay=2500, conv_target=1e-8, min_grad=1e-25, max_iterations=3)
    eng = make_engine(sp)
    try:
        assert_kernel(eng, mode)
        eng.set_base(np.stack(bases))
        eng.iterate(eng.adam_params(poll_every=3, **conv), 3)
        eng.sync()
        base = eng.get_base()
        r, Uf = eng.evaluate(), eng.get_final_unitary()
        for b in range(SETS):
            ref = go.run_adam(sp, conv, base=bases[b])
            assert ref['iterations'] == 3
            print('  set %d: base %.2e  loss %.2e  U_final %.2e' % (b, np.max(np.abs(base[b] - ref['base'])), abs(r['loss'][b] - ref['loss']),
                                                                  np.max(np.abs(Uf[b] - ref['U_final']))))
            np.testing.assert_allclose(base[b], ref['base'], rtol=0, atol=1e-10)
            assert abs(r['loss'][b] - ref['loss']) <= 1e-10
            np.testing.assert_allclose(Uf[b], ref['U_final'], rtol=0, atol=1e-10)
    finally:
        eng.close()
