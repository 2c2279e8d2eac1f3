"""Transfer-function GRAPE on the GPU: a shaped engine (hip_engine.HipEngine(transfer=...), qoc_create_shaped) against the unchanged oracle,
composed -- the quantum part is go.evaluate at arcsin(sin(theta) @ T.T) on a system that carries only the state regularisers (the sin o
arcsin round trip is exact to 4e-16), the pulse part go.pulse_regularisers on a view of P samples of total_time / P each, the gradient
cos(theta) (maxA (dL_du @ T) + dR) -- on every path that can host it, with and without an ensemble; the split tail on the sample view; the
bit identity of the identity response with the plain engine; the device Adam loop against a Python loop over the composed oracle; AUTO's
exclusions; Grape(transfer=...); and the capability itself (examples/filtered_qutrit_x_gate.py)."""
import contextlib
import functools
import importlib.util
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import transfer as tf
from tests.composed_reference import run_adam, split_regs
from tests.golden import cases
from tests.robust_reference import composed_shaped
from tests.test_adam_tail import _choose_target
from tests.test_robust_gpu import STATE_PATHS, UNITARY_PATHS, bases_for, ensemble, member_systems, nominal_system, problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U_ATOL, G_RTOL, S_RTOL = 1e-12, 1e-11, 1e-12          # tests/test_hip_parity.py
P = hip_engine
PULSE_REGS = dict(amplitude=0.01, dwdt=0.001, d2wdt2=1e-5, bandpass=0.01, band=[0.5, 5.0])     # (no envelope: it is defined per time slice)


# ---- problems, responses, the composed oracle -------------------------------------------------------------------------------------------

def shaped_problem(kind, regs, steps=40):
    c = problem(kind, 'none' if regs == 'pulse' else regs, steps)
    if regs == 'pulse':
        c['reg_coeffs'] = dict(PULSE_REGS)
    return c


def response(name, steps, total_time):
    """steps x P matrices with rows of l1 norm <= 1 (arcsin of the filtered pulse is defined)."""
    if name == 'hold7':                                  # uneven windows
        return tf.hold(steps, 7).matrix
    if name == 'identity':
        return np.eye(steps)
    if name == 'gauss13':                                # overlapping windows
        M = tf.gaussian_filter(steps, 13, total_time, 1.5 * total_time / steps).matrix
        return M / np.maximum(1.0, np.sum(np.abs(M), axis=1))[:, None]        # (a row sum of 1 + 1 ulp -> 1)
    if name == 'dense5':                                 # full windows, negative entries
        M = np.random.default_rng(11).uniform(-1.0, 1.0, size=(steps, 5))
        return 0.9 * M / np.sum(np.abs(M), axis=1)[:, None]
    raise KeyError(name)


RESPONSES = ('hold7', 'identity', 'gauss13', 'dense5')


def thetas(k, Pn, G):
    rng = np.random.default_rng(1000 + Pn)
    return rng.normal(0.0, 0.7, size=(3, k, Pn))[:G]


def systems(c, ens):
    """(nominal system as the engine gets it, member systems with the state regularisers only, weights)."""
    nominal = nominal_system(c)
    state_rc, _ = split_regs(c['reg_coeffs'])
    cq = dict(c, reg_coeffs=state_rc)
    if ens is None:
        return nominal, [nominal_system(cq)], np.ones(1)
    return nominal, member_systems(cq, ens, (nominal.exp_terms, nominal.scaling)), ens['weights']


@functools.lru_cache(maxsize=None)
def reference(kind, regs, resp, Eq):
    """The composed oracle of a row at its three variables: computed once, shared by every path and batch size."""
    c = shaped_problem(kind, regs)
    ens = ensemble(c, *Eq) if Eq else None
    nominal, sps, w = systems(c, ens)
    T = response(resp, nominal.steps, nominal.total_time)
    th = thetas(nominal.k, T.shape[1], 3)
    _, pulse_rc = split_regs(c['reg_coeffs'])
    return [composed_shaped(sps, w, T, th[g], pulse_rc, nominal.total_time) for g in range(3)]


def make_engine(sp, G, T, ens=None, path=P.PATH_AUTO, variant=0, chunks=0, reg_coeffs=None):
    return hip_engine.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling,
                                state_transfer=sp.state_transfer, reg_coeffs=sp.reg_coeffs if reg_coeffs is None else reg_coeffs, Vs=sp.Vs,
                                n_seeds=G, path=path, variant=variant, chunks=chunks, ensemble=ens, transfer=T)


def pulse_atol(T, maxA):
    """Bound on |maxA T sin(theta)| computed twice in fp64: each of the two sums carries at most one rounding per term of a row (the terms are
    bounded by the row's l1 norm <= 1), the device's sin may differ from NumPy's by an ulp or two, and maxA adds one rounding each."""
    return (2 * T.shape[1] + 6) * 1.2e-16 * float(np.max(maxA))


def assert_matches(eng, r, g, o, state_transfer):
    for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale'):
        print('%s[%d]: engine %.17g composed %.17g' % (key, g, r[key][g], o[key]))
        assert abs(r[key][g] - o[key]) <= S_RTOL * max(1.0, abs(o[key])), (key, g, r[key][g], o[key])
    gm = max(1.0, float(np.max(np.abs(o['grad']))))
    err = float(np.max(np.abs(r['grad'][g] - o['grad'])))
    print('grad[%d]: max error %.3e of max %.3e' % (g, err, gm))
    assert err <= G_RTOL * gm, (g, err)


def check_evaluation(c, refs, T, ens, G, path, variant=0, chunks=0):
    nominal = nominal_system(c)
    eng = make_engine(nominal, G, T, ens, path, variant, chunks)
    try:
        if path != P.PATH_AUTO:
            assert eng.path == path, (eng.path, path)
        assert eng.path != P.PATH_SMALL and 'latency' not in eng.plan.get('sweeps', '')
        band = max(int(np.flatnonzero(row)[-1] - np.flatnonzero(row)[0] + 1) if np.any(row) else 0 for row in T)
        assert eng.plan['samples'] == str(T.shape[1]) and eng.plan['band'] == str(band), eng.plan
        th = thetas(nominal.k, T.shape[1], G)
        eng.set_base(th)
        r = eng.evaluate()
        pulse = eng.get_pulse()
        Uf = None if nominal.state_transfer else eng.get_final_unitary()
        r2 = eng.evaluate()
        assert np.array_equal(r['grad'], r2['grad'])                              # fixed summation order: bit-reproducible
        assert r['grad'].shape == (G, nominal.k, T.shape[1]) and pulse.shape == (G, nominal.k, nominal.steps)
        for g in range(G):
            o = refs[g]
            assert_matches(eng, r, g, o, nominal.state_transfer)
            perr = float(np.max(np.abs(pulse[g] - o['pulse'])))
            print('pulse[%d]: max error %.3e' % (g, perr))
            assert perr <= pulse_atol(T, nominal.maxA), perr
            if Uf is not None:
                assert np.max(np.abs(Uf[g] - o['U0'])) <= U_ATOL
        assert np.allclose(eng.get_uks(evaluated=True), nominal.maxA[None, :, None] * np.sin(th), rtol=0, atol=4e-16 * float(np.max(nominal.maxA)))
    finally:
        eng.close()


# ---- 1. single evaluation against the composed oracle -----------------------------------------------------------------------------------

ROWS = []
for kind, regsets, paths in (('unitary', ('none', 'pulse', 'state'), UNITARY_PATHS), ('dressed', ('keep',), UNITARY_PATHS),
                             ('state', ('none', 'pulse', 'state'), STATE_PATHS)):
    for regs in regsets:
        for resp in RESPONSES:
            for pname, path, variant, chunks in paths:
                for G in (1, 3):
                    ROWS.append(pytest.param(kind, regs, resp, path, variant, chunks, None, G, id='%s-%s-%s-%s-G%d' % (kind, regs, resp, pname, G)))
            for pname, path, variant, chunks in paths:
                if pname in ('auto', 'mfma', 'gemm', 'gemm_direct'):
                    ROWS.append(pytest.param(kind, regs, resp, path, variant, chunks, (3, 1), 3,
                                             id='%s-%s-%s-%s-E3-q1' % (kind, regs, resp, pname)))


@pytest.mark.parametrize('kind,regs,resp,path,variant,chunks,Eq,G', ROWS)
def test_evaluation_matches_the_composed_oracle(kind, regs, resp, path, variant, chunks, Eq, G):
    c = shaped_problem(kind, regs)
    nominal = nominal_system(c)
    T = response(resp, nominal.steps, nominal.total_time)
    check_evaluation(c, reference(kind, regs, resp, Eq), T, ensemble(c, *Eq) if Eq else None, G, path, variant, chunks)


# ---- 2. the split tail on the sample view -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _split_case():
    c = shaped_problem('unitary', 'pulse', steps=2100)
    c['total_time'] = 0.002 * 2100
    c = dict(c, H0=c['H0'][:4, :4], Hops=[h[:4, :4] for h in c['Hops']], U=np.eye(4), states_concerned_list=[0, 1])
    nominal, sps, w = systems(c, None)
    T = tf.gaussian_filter(2100, 2100, c['total_time'], 1.5 * 0.002).matrix
    T = T / np.maximum(1.0, np.sum(np.abs(T), axis=1))[:, None]
    _, pulse_rc = split_regs(c['reg_coeffs'])
    th = thetas(nominal.k, 2100, 1)
    return c, T, [composed_shaped(sps, w, T, th[0], pulse_rc, nominal.total_time)]


@pytest.mark.parametrize('path', [P.PATH_AUTO, P.PATH_MFMA, P.PATH_GEMM])
def test_split_tail_on_the_sample_view(path):
    """k P = 2 x 2100 > 4096: the split tail runs on the sample view, behind a Gaussian response a few slices wide."""
    c, T, refs = _split_case()
    eng = make_engine(nominal_system(c), 1, T, None, path)
    try:
        assert eng.plan['tail'].startswith('split') and not eng.plan['tail'].endswith('partials'), eng.plan
    finally:
        eng.close()
    check_evaluation(c, refs, T, None, 1, path)


# ---- 3. bit identity of the identity response -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('path,variant', [(P.PATH_MFMA, 0), (P.PATH_GEMM, 0), (P.PATH_GENERIC, 0)])
@pytest.mark.parametrize('regs', ['none', 'pulse'])
def test_identity_response_is_bit_identical_to_the_plain_engine(path, variant, regs):
    c = shaped_problem('unitary', regs)
    sp = nominal_system(c)
    conv = dict(rate=0.02, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=25, poll_every=7)
    out = []
    for T in (None, np.eye(sp.steps)):
        eng = make_engine(sp, 2, T, None, path, variant)
        try:
            eng.set_base(bases_for(sp, 2))
            its = eng.run_adam(eng.adam_params(**conv))
            out.append((its, eng.get_base(), eng.scalars(), eng.get_uks(), eng.get_final_unitary(),
                        eng.get_uks(evaluated=True) if T is None else eng.get_pulse()))
        finally:
            eng.close()
    (i0, b0, s0, u0, f0, p0), (i1, b1, s1, u1, f1, p1) = out
    assert np.array_equal(i0, i1) and np.array_equal(b0, b1) and np.array_equal(u0, u1) and np.array_equal(f0, f1) and np.array_equal(p0, p1)
    for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale', 'iterations', 'done'):
        assert np.array_equal(s0[key], s1[key]), key


# ---- 4. the device Adam loop against a Python loop over the composed oracle -------------------------------------------------------------

def python_loop(sps, w, T, theta, pulse_rc, total_time, conv):
    """run_session.start_adam_optimizer over the composed oracle: go.Adam, run_adam's stop rule and learning-rate schedule."""
    return run_adam(lambda th: composed_shaped(sps, w, T, th, pulse_rc, total_time), theta, conv)


@pytest.mark.parametrize('kind,regs,resp,path', [('unitary', 'pulse', 'hold7', P.PATH_AUTO), ('state', 'none', 'gauss13', P.PATH_AUTO)])
def test_adam_loop_matches_the_composed_oracle(kind, regs, resp, path):
    """G = 2, 30 iterations: conv_target is chosen so that one control set stops early and finishes beside one that runs on."""
    c = shaped_problem(kind, regs)
    nominal, sps, w = systems(c, None)
    T = response(resp, nominal.steps, nominal.total_time)
    _, pulse_rc = split_regs(c['reg_coeffs'])
    th = thetas(nominal.k, T.shape[1], 2)
    conv = dict(rate=0.02, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=30)
    free = [python_loop(sps, w, T, b, pulse_rc, nominal.total_time, conv) for b in th]
    target, stops = _choose_target([f['history'] for f in free], 30)
    conv['conv_target'] = target
    refs = [python_loop(sps, w, T, b, pulse_rc, nominal.total_time, conv) for b in th]
    assert [r['iterations'] for r in refs] == stops
    eng = make_engine(nominal, 2, T, None, path)
    try:
        eng.set_base(th)
        its = eng.run_adam(eng.adam_params(poll_every=4, **conv))
        s = eng.scalars()
        base = eng.get_base()
        for g, ref in enumerate(refs):
            assert its[g] == ref['iterations'], (its, stops)
            print('set %d: base error %.3e' % (g, np.max(np.abs(base[g] - ref['base']))))
            assert np.max(np.abs(base[g] - ref['base'])) < 1e-9, np.max(np.abs(base[g] - ref['base']))
            assert abs(s['loss'][g] - ref['last']['loss']) < 1e-10 * max(1.0, abs(ref['last']['loss']))
            assert abs(s['reg_loss'][g] - ref['last']['reg_loss']) < 1e-10 * max(1.0, abs(ref['last']['reg_loss']))
    finally:
        eng.close()


# ---- 5. AUTO exclusions -----------------------------------------------------------------------------------------------------------------

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
    sp = nominal_system(c)
    Pn = max(1, sp.steps // 4)
    eng = make_engine(sp, G, tf.hold(sp.steps, Pn).matrix)
    try:
        assert eng.path != P.PATH_SMALL and 'latency' not in eng.plan.get('sweeps', ''), eng.plan
        assert eng.plan['samples'] == str(Pn) and eng.plan['band'] == '1' and eng.plan['members'] == '1'
        assert not eng.plan['tail'].startswith(('in_launch', 'latency')) and not eng.plan['tail'].endswith('partials')
    finally:
        eng.close()
    plain = make_engine(sp, G, None)
    try:
        assert 'samples' not in plain.plan
        with pytest.raises(hip_engine.QocError, match='not a shaped engine'):
            plain.get_pulse()
    finally:
        plain.close()


@pytest.mark.parametrize('kw,match', [(dict(path=P.PATH_SMALL), 'workgroup-resident'), (dict(path=P.PATH_MFMA, variant=5), 'latency'),
                                      (dict(variant=5), 'latency'), (dict(reg_coeffs={'envelope': 0.02}), 'envelope')])
def test_explicit_excluded_requests_fail(kw, match):
    c = cases.case_c1()
    c['Taylor_terms'] = [12, 2]
    sp = nominal_system(c)
    with pytest.raises(hip_engine.QocError, match=match):
        make_engine(sp, 1, tf.hold(sp.steps, 5).matrix, **kw)


# ---- 6. Grape(transfer=...) -------------------------------------------------------------------------------------------------------------

SZ = np.array([[1, 0], [0, -1]], dtype=complex)
SX = np.array([[0, 1], [1, 0]], dtype=complex)
SY = np.array([[0, -1j], [1j, 0]], dtype=complex)
QUBIT = (0.0 * SZ, [2 * np.pi * SX / 2, 2 * np.pi * SY / 2], ['x', 'y'], SX)
QUBIT_KW = dict(total_time=20.0, steps=40, states_concerned_list=[0, 1], maxA=[0.1, 0.1], reg_coeffs={}, show_plots=False)


def _quiet_grape(*args, **kw):
    from quantum_optimal_control.main_grape.grape import Grape
    with contextlib.redirect_stdout(io.StringIO()) as out:
        res = Grape(*args, **kw)
    return res, out.getvalue()


@pytest.mark.parametrize('restarts', [1, 3])
def test_grape_returns_the_pulse_and_fills_the_samples(restarts):
    line = tf.gaussian_filter(40, 8, 20.0, 0.6)
    conv = {'rate': 0.02, 'update_step': 10, 'max_iterations': 30, 'conv_target': 1e-10, 'learning_rate_decay': 1000}
    np.random.seed(3)
    (uks, Uf), _ = _quiet_grape(*QUBIT, transfer=line, method='Adam', save=False, convergence=conv, restarts=restarts, **QUBIT_KW)
    assert uks.shape == (2, 40) and Uf.shape == (2, 2) and line.samples.shape == (2, 8)
    assert np.max(np.abs(uks - tf.apply(line, line.samples))) <= 1e-14
    assert np.max(np.abs(line.samples)) <= 0.1
    # a guess in sample amplitudes: EVOLVE returns its response
    guess = np.array([[0.05, -0.02, 0.01, 0.0, 0.03, 0.08, -0.1, 0.02], [0.0] * 8])
    (uks, _), _ = _quiet_grape(*QUBIT, transfer=line, method='EVOLVE', save=False, initial_guess=guess, **QUBIT_KW)
    assert np.max(np.abs(line.samples - guess)) <= 1e-15 and np.max(np.abs(uks - tf.apply(line, guess))) <= 1e-14


def test_grape_lbfgs_runs_on_the_samples():
    line = tf.hold(40, 8)
    np.random.seed(3)
    conv = {'rate': 0.02, 'update_step': 1, 'max_iterations': 40, 'conv_target': 1e-12, 'learning_rate_decay': 1000}
    (uks, Uf), text = _quiet_grape(*QUBIT, transfer=line, method='L-BFGS-B', save=False, convergence=conv, **QUBIT_KW)
    errors = [float(l.split('Error = :')[1].split(';')[0]) for l in text.splitlines() if l.startswith('Error = :')]
    assert uks.shape == (2, 40) and np.max(np.abs(uks - tf.apply(line, line.samples))) <= 1e-14
    print('L-BFGS-B: first loss %.3e, last loss %.3e' % (errors[0], errors[-1]))
    assert errors[-1] < errors[0]


def test_grape_run_log_holds_the_transfer_matrix_and_the_samples(tmp_path):
    """tests/transfer_h5_script.py in an interpreter with h5py: this one, else the one tests/test_h5_log.py falls back to."""
    from tests import test_h5_log
    if importlib.util.find_spec('h5py') is not None:
        exe = sys.executable
    elif os.path.exists(test_h5_log.CONDA):
        exe = test_h5_log.CONDA
    else:
        pytest.skip('no interpreter with h5py available')
    env = dict(os.environ)
    sys_cxx = '/usr/lib/x86_64-linux-gnu/libstdc++.so.6'
    if exe == test_h5_log.CONDA and os.path.exists(sys_cxx):
        # (as tests/test_h5_log.py: conda's libstdc++ is older than the HIP runtime needs; whatever is preloaded already stays)
        env['LD_PRELOAD'] = ':'.join(x for x in (sys_cxx, env.get('LD_PRELOAD', '')) if x)
    r = subprocess.run([exe, '-W', 'ignore', os.path.join(ROOT, 'tests', 'transfer_h5_script.py'), str(tmp_path)], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0 and 'OK grape_transfer_save' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_sharded_and_time_sharded_grape_refuse_a_transfer():
    from quantum_optimal_control.main_grape.grape import Grape, GrapeSharded
    with pytest.raises(ValueError, match='GrapeSharded: transfer'):
        GrapeSharded(*QUBIT, transfer=tf.hold(40, 8), restarts=2, save=False, **QUBIT_KW)
    with pytest.raises(ValueError, match='time-sharded'):
        Grape(*QUBIT, transfer=tf.hold(40, 8), time_comm=object(), save=False, **QUBIT_KW)


# ---- 7. the capability itself -----------------------------------------------------------------------------------------------------------

def test_aware_pulse_beats_the_naive_pulse_through_the_filter():
    """Qutrit X gate (anharmonicity -0.2 GHz, x and y drives of maxA 0.15, 10 ns in 100 slices), 10 samples per line through a Gaussian line
    response of sigma = 0.5 ns, 300 Adam iterations each (examples/filtered_qutrit_x_gate.py); both sample sets sent through the filter and
    re-simulated with scipy.linalg.expm.  The bounds: the aware pulse at least 100 x below the naive one, and below 1e-6.
    Measured on an MI355X: naive 1.05e-2, aware 7.8e-13 (1.3e10 x below)."""
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import filtered_qutrit_x_gate as ex
    with contextlib.redirect_stdout(io.StringIO()):
        inf_naive, inf_aware = ex.main(iterations=300, quiet=True)
    print('infidelity through the filter: naive %.3e aware %.3e' % (inf_naive, inf_aware))
    assert inf_aware * 100 <= inf_naive, (inf_naive, inf_aware)
    assert inf_aware < 1e-6, inf_aware
