"""Robust GRAPE on the GPU: an ensemble engine (hip_engine.HipEngine(ensemble=...), qoc_create_ensemble) against the ensemble composed from the
unchanged oracle -- one go.OracleSystem per member, with the engine's (T, s) -- on every path that can host it, the bit identity of a one-member
ensemble with the plain engine, the device Adam loop against a Python loop over the composed oracle, AUTO's exclusions, and the capability
itself through Grape(robust=...)."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import robust as rb
from quantum_optimal_control.helper_functions.synthetic_systems import herm
from tests.composed_reference import run_adam
from tests.golden import cases
from tests.robust_reference import composed, member_systems, nominal_system          # noqa: F401  (also imported from here by other tests)
from tests.test_adam_tail import _choose_target

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U_ATOL, G_RTOL, S_RTOL = 1e-12, 1e-11, 1e-12          # tests/test_hip_parity.py
P = hip_engine
PULSE_REGS = dict(amplitude=0.01, envelope=0.02, dwdt=0.001, d2wdt2=1e-5, bandpass=0.01, band=[0.5, 5.0])


# ---- problems ---------------------------------------------------------------------------------------------------------------------------

def problem(kind, regs, steps=40):
    """A case dict (tests/golden/cases.py style) with fixed (T, s)."""
    if kind == 'unitary':
        c = cases.case_c2(n=8, k=2, steps=steps, m=4, taylor=(6, 2), seed=21)
        c['total_time'] = 0.05 * steps
    elif kind == 'dressed':
        c = cases.case_dressed()
        c['Taylor_terms'] = [8, 2]
    else:
        c = cases.case_state_small()
        c['Taylor_terms'] = [10, 0]
        c['reg_coeffs'] = {}
    c = dict(c)
    if regs == 'pulse':
        c['reg_coeffs'] = dict(PULSE_REGS)
    elif regs == 'state':
        c['reg_coeffs'] = {'forbidden_coeff_list': [20.0], 'states_forbidden_list': [len(c['H0']) - 1], 'speed_up': 0.1}
    elif regs == 'none':
        c['reg_coeffs'] = {}
    return c


def ensemble(c, E, q, seed=5):
    rng = np.random.default_rng(seed)
    n, k = len(c['H0']), len(c['Hops'])
    ops = [0.3 * 2 * np.pi * herm(rng, n) for _ in range(q)]
    off = rng.uniform(-0.2, 0.2, size=(E, q))
    amp = rng.uniform(0.9, 1.1, size=(E, k))
    w = rng.uniform(0.5, 1.5, size=E)
    if E == 1:
        off, amp, w = np.zeros((1, q)), np.ones((1, k)), np.ones(1)
    return rb.validate(dict(operators=ops, offsets=off, amp_scales=amp, weights=w), n, k)


def make_engine(sp, G, ens, path=P.PATH_AUTO, variant=0, chunks=0, plan_seeds=0):
    return hip_engine.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling,
                                state_transfer=sp.state_transfer, reg_coeffs=sp.reg_coeffs, one_minus_gauss=sp.one_minus_gauss, Vs=sp.Vs,
                                n_seeds=G, path=path, variant=variant, chunks=chunks, plan_seeds=plan_seeds, ensemble=ens)


def bases_for(sp, G):
    return np.stack([sp.base0, 0.6 * sp.base0 + 0.1, -0.8 * sp.base0 + 0.05][:G])


def check_evaluation(c, ens, G, path, variant=0, chunks=0):
    nominal = nominal_system(c)
    eng = make_engine(nominal, G, ens, path, variant, chunks)
    try:
        if path != P.PATH_AUTO:
            assert eng.path == path, (eng.path, path)
        assert eng.path != P.PATH_SMALL and 'latency' not in eng.plan.get('sweeps', '')
        assert eng.plan['members'] == str(len(ens['weights'])) and eng.plan['perturbations'] == str(len(ens['operators']))
        taylor = (nominal.exp_terms, nominal.scaling)
        sps = member_systems(c, ens, taylor)
        bases = bases_for(nominal, G)
        eng.set_base(bases)
        r = eng.evaluate()
        ms = eng.member_scalars()
        Uf = None if nominal.state_transfer else eng.get_final_unitary()
        for g in range(G):
            o = composed(sps, ens['weights'], bases[g])
            for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale'):
                assert abs(r[key][g] - o[key]) <= S_RTOL * max(1.0, abs(o[key])), (key, g, r[key][g], o[key])
            gm = max(1.0, float(np.max(np.abs(o['grad']))))
            assert np.max(np.abs(r['grad'][g] - o['grad'])) <= G_RTOL * gm, (g, np.max(np.abs(r['grad'][g] - o['grad'])))
            assert np.max(np.abs(ms['loss'][g] - o['member_loss'])) <= S_RTOL * max(1.0, np.max(np.abs(o['member_loss'])))
            if Uf is not None:
                assert np.max(np.abs(Uf[g] - o['U0'])) <= U_ATOL
    finally:
        eng.close()


# ---- 1. single evaluation against the composed oracle -----------------------------------------------------------------------------------

ENSEMBLES = [(1, 0, 1), (3, 1, 3), (16, 2, 1)]          # (E, q, G)
UNITARY_PATHS = [('auto', P.PATH_AUTO, 0, 0), ('mfma', P.PATH_MFMA, 0, 0), ('gemm', P.PATH_GEMM, 0, 0), ('generic', P.PATH_GENERIC, 0, 0)]
STATE_PATHS = UNITARY_PATHS[:2] + [('gemm_direct', P.PATH_GEMM, 0, 1), ('gemm_propagator', P.PATH_GEMM, 0, 2),
                                   ('st_fused', P.PATH_ST_FUSED, 0, 0), ('generic', P.PATH_GENERIC, 0, 0)]
ROWS = []
for kind, regsets, paths in (('unitary', ('none', 'pulse', 'state'), UNITARY_PATHS), ('dressed', ('keep',), UNITARY_PATHS),
                             ('state', ('none', 'pulse', 'state'), STATE_PATHS)):
    for regs in regsets:
        for pname, path, variant, chunks in paths:
            for E, q, G in ENSEMBLES:
                ROWS.append(pytest.param(kind, regs, path, variant, chunks, E, q, G, id='%s-%s-%s-E%d-q%d-G%d' % (kind, regs, pname, E, q, G)))


@pytest.mark.parametrize('kind,regs,path,variant,chunks,E,q,G', ROWS)
def test_evaluation_matches_the_composed_oracle(kind, regs, path, variant, chunks, E, q, G):
    c = problem(kind, regs)
    check_evaluation(c, ensemble(c, E, q), G, path, variant, chunks)


@pytest.mark.parametrize('path', [P.PATH_AUTO, P.PATH_MFMA, P.PATH_GEMM])
def test_split_tail_on_the_group_view(path):
    """k steps = 2 x 2100 > 4096: the split tail runs on the group view (the trajectories have k + q = 3 rows)."""
    c = problem('unitary', 'pulse', steps=2100)
    c['total_time'] = 0.002 * 2100
    c = dict(c, H0=c['H0'][:4, :4], Hops=[h[:4, :4] for h in c['Hops']], U=np.eye(4), states_concerned_list=[0, 1])
    ens = ensemble(c, 3, 1)
    eng = make_engine(nominal_system(c), 1, ens, path)
    try:
        assert eng.plan['tail'].startswith('split') and not eng.plan['tail'].endswith('partials'), eng.plan
    finally:
        eng.close()
    check_evaluation(c, ens, 1, path)


# ---- 2. bit identity of a one-member nominal ensemble -----------------------------------------------------------------------------------

@pytest.mark.parametrize('path,variant', [(P.PATH_MFMA, 0), (P.PATH_GEMM, 0), (P.PATH_GENERIC, 0)])
@pytest.mark.parametrize('regs', ['none', 'pulse'])
def test_one_nominal_member_is_bit_identical_to_the_plain_engine(path, variant, regs):
    c = problem('unitary', regs)
    sp = nominal_system(c)
    ens = rb.validate(dict(operators=[], offsets=np.zeros((1, 0)), amp_scales=np.ones((1, 2)), weights=[1.0]), 8, 2)
    conv = dict(rate=0.02, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=25, poll_every=7)
    out = []
    for e in (None, ens):
        eng = make_engine(sp, 2, e, path, variant)
        try:
            eng.set_base(bases_for(sp, 2))
            its = eng.run_adam(eng.adam_params(**conv))
            out.append((its, eng.get_base(), eng.scalars(), eng.get_uks(), eng.get_final_unitary()))
        finally:
            eng.close()
    (i0, b0, s0, u0, f0), (i1, b1, s1, u1, f1) = out
    assert np.array_equal(i0, i1) and np.array_equal(b0, b1) and np.array_equal(u0, u1) and np.array_equal(f0, f1)
    for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale', 'iterations', 'done'):
        assert np.array_equal(s0[key], s1[key]), key


# ---- 3. the device Adam loop against a Python loop over the composed oracle -------------------------------------------------------------

def python_loop(sps, w, base, conv):
    """run_session.start_adam_optimizer over the composed ensemble: go.Adam, run_adam's stop rule and learning-rate schedule."""
    return run_adam(lambda b: composed(sps, w, b), base, conv)


@pytest.mark.parametrize('kind,regs,path', [('unitary', 'pulse', P.PATH_AUTO), ('unitary', 'state', P.PATH_GEMM),
                                            ('state', 'none', P.PATH_AUTO)])
def test_adam_loop_matches_the_composed_oracle(kind, regs, path):
    """G = 2, 30 iterations: conv_target is chosen so that one control set stops early and finishes beside one that runs on."""
    c = problem(kind, regs)
    ens = ensemble(c, 3, 1)
    sps = member_systems(c, ens, c['Taylor_terms'])
    bases = bases_for(sps[0], 2)
    conv = dict(rate=0.02, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=30)
    free = [python_loop(sps, ens['weights'], b, conv) for b in bases]
    target, stops = _choose_target([f['history'] for f in free], 30)
    conv['conv_target'] = target
    refs = [python_loop(sps, ens['weights'], b, conv) for b in bases]
    assert [r['iterations'] for r in refs] == stops
    eng = make_engine(nominal_system(c), 2, ens, path)
    try:
        eng.set_base(bases)
        its = eng.run_adam(eng.adam_params(poll_every=4, **conv))
        s = eng.scalars()
        base = eng.get_base()
        for g, ref in enumerate(refs):
            assert its[g] == ref['iterations'], (its, stops)
            assert np.max(np.abs(base[g] - ref['base'])) < 1e-9, np.max(np.abs(base[g] - ref['base']))
            assert abs(s['loss'][g] - ref['last']['loss']) < 1e-10 * max(1.0, abs(ref['last']['loss']))
            assert abs(s['reg_loss'][g] - ref['last']['reg_loss']) < 1e-10 * max(1.0, abs(ref['last']['reg_loss']))
    finally:
        eng.close()


# ---- 4. AUTO exclusions and planning ----------------------------------------------------------------------------------------------------

def _auto_case(name):
    if name == 'qubit':
        return cases.case_c1()
    if name == 'two_transmon':
        c = cases.case_c2(n=9, k=2, steps=300, m=9, taylor=(6, 2), seed=3)
        return dict(c, reg_coeffs={'forbidden_coeff_list': [10.0], 'states_forbidden_list': [8]})
    return cases.case_c2(n=32, k=4, steps=500, m=8, taylor=(5, 3), seed=0)


@pytest.mark.parametrize('name', ['qubit', 'two_transmon', 'c2'])
@pytest.mark.parametrize('G', [1, 4])
def test_auto_never_picks_an_excluded_path(name, G):
    c = _auto_case(name)
    if c['Taylor_terms'] is None:
        c['Taylor_terms'] = [12, 2]
    ens = ensemble(c, 9, 1)
    sp = nominal_system(c)
    eng = make_engine(sp, G, ens)
    try:
        assert eng.path != P.PATH_SMALL and 'latency' not in eng.plan.get('sweeps', ''), eng.plan
        assert eng.plan['members'] == '9' and eng.plan['perturbations'] == '1'
        assert not eng.plan['tail'].startswith(('in_launch', 'latency')) and not eng.plan['tail'].endswith('partials')
    finally:
        eng.close()
    plain = make_engine(sp, G, None)
    try:
        assert 'members' not in plain.plan
    finally:
        plain.close()


@pytest.mark.parametrize('kw,match', [(dict(path=P.PATH_SMALL), 'workgroup-resident'), (dict(path=P.PATH_MFMA, variant=5), 'latency'),
                                      (dict(variant=5), 'latency')])
def test_explicit_excluded_requests_fail(kw, match):
    c = cases.case_c1()
    c['Taylor_terms'] = [12, 2]
    ens = ensemble(c, 3, 1)
    sp = nominal_system(c)
    with pytest.raises(hip_engine.QocError, match=match):
        make_engine(sp, 1, ens, **kw)


# ---- 5. the capability itself, and 6. the example ---------------------------------------------------------------------------------------

def test_robust_pulse_beats_the_nominal_pulse_on_the_worst_member():
    """Qubit pi pulse, x and y drives (maxA 0.1 GHz, 40 ns, 100 slices), 300 Adam iterations each; ensemble +-5 MHz detuning x {0.95, 1,
    1.05} amplitude (9 members).  Both pulses re-simulated on every member with scipy.linalg.expm (examples/robust_qubit_pi_pulse.py).
    Measured on an MI355X: worst-member infidelity of the nominal pulse 1.69e-1, of the robust pulse 1.00e-2 (16.9 x); the bound asks for 5 x."""
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import robust_qubit_pi_pulse as ex
    with contextlib.redirect_stdout(io.StringIO()) as out:
        f_nominal, f_robust = ex.main(iterations=300, quiet=True)
    worst_nominal, worst_robust = 1 - f_nominal.min(), 1 - f_robust.min()
    print('worst-member infidelity: nominal %.3e robust %.3e' % (worst_nominal, worst_robust))
    assert worst_robust * 5 < worst_nominal, (worst_nominal, worst_robust)
    assert 'Robust ensemble: 9 members' in out.getvalue()
