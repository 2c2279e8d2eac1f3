"""Open-system GRAPE without a GPU: the NumPy reference of tests/lindblad_reference.py against the closed-system oracle (no collapse operator),
against scipy's exponential of the dense Liouvillian, and against central differences of its own loss; the Taylor rule of
helper_functions/open_system.py; and every refusal of the Python layer that needs no library."""
import functools
import inspect
import math

import numpy as np
import pytest
from scipy.linalg import expm

from oracle import grape_oracle as go
from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import open_system
from quantum_optimal_control.helper_functions.synthetic_systems import herm, random_unitary
from quantum_optimal_control.main_grape.grape import Grape, GrapeSharded, GrapeTimeSharded
from tests import lindblad_reference as lr
from tests.lindblad_reference import collapse_list

G_RTOL = 1e-11          # the constants of tests/test_hip_parity.py (restated: that module needs nothing this file does)
S_RTOL = 1e-12


# ---- systems shared with tests/test_open_system_gpu.py ----------------------------------------------------------------------------------

def open_case(n, k, m, steps, taylor, c, seed, state_transfer=False, reg_coeffs=None, dt=0.4, **kw):
    """(OracleSystem, collapse operators): generators of norm 1 (drift) and 1/2 (controls), amplitudes up to 1 + k / 4."""
    rng = np.random.default_rng(seed)
    H0 = herm(rng, n)
    Hops = [0.5 * herm(rng, n) for _ in range(k)]
    if state_transfer:
        def unit():
            v = rng.normal(size=n) + 1j * rng.normal(size=n)
            return v / np.linalg.norm(v)
        states, U = [unit() for _ in range(m)], [unit() for _ in range(m)]
    else:
        states, U = list(range(m)), random_unitary(rng, n)
    np.random.seed(seed)
    sp = go.OracleSystem(H0, Hops, U, dt * steps, steps, states, U0=None if state_transfer else random_unitary(rng, n), reg_coeffs=reg_coeffs or {},
                         maxA=[1.0 + 0.25 * i for i in range(k)], state_transfer=state_transfer, Taylor_terms=list(taylor), **kw)
    sp.H0_in, sp.Hops_in = H0, Hops
    return sp, collapse_list(n, c, seed)


def bases_of(sp, seed=0):
    rng = np.random.default_rng(50 + seed)
    b1 = sp.base0 + 0.4 * rng.normal(size=sp.base0.shape)
    return [sp.base0, b1, -0.5 * b1 + 0.1]


# ---- (a) the closed limit ---------------------------------------------------------------------------------------------------------------

def _closed_check(sp, oracle_sp):
    for base in bases_of(sp)[:2]:
        r = lr.evaluate(sp, [], base)
        o = go.evaluate(oracle_sp, base)
        gmax = float(np.max(np.abs(o['dL_du'])))
        err = float(np.max(np.abs(r['dL_du'] - o['dL_du'])))
        print('closed limit: loss %.17g / %.17g, gradient error %.3e of %.3e' % (r['loss'], o['loss'], err, gmax))
        assert abs(r['loss'] - o['loss']) <= S_RTOL * max(1.0, abs(o['loss']))
        assert err <= G_RTOL * gmax
        assert abs(r['unitary_scale'] - 1.0) <= 1e-9                     # (Taylor truncation only)


def test_closed_limit_unitary_mode():
    sp, _ = open_case(4, 2, 3, 7, (14, 2), 0, seed=1)
    _closed_check(sp, sp)


def test_closed_limit_state_transfer():
    """Degree 16 here is the closed engine's Taylor_terms = 17 in state transfer (sum over j < T)."""
    sp, _ = open_case(4, 2, 2, 7, (16, 0), 0, seed=2, state_transfer=True)
    oracle_sp, _ = open_case(4, 2, 2, 7, (17, 0), 0, seed=2, state_transfer=True)
    _closed_check(sp, oracle_sp)


# ---- (b) two collapse operators against the dense Liouvillian ------------------------------------------------------------------------------

def test_propagation_against_the_dense_liouvillian():
    sp, ops = open_case(4, 2, 3, 7, (14, 2), 2, seed=1)
    base = bases_of(sp)[1]
    r = lr.evaluate(sp, ops, base, want_grad=False)
    Ds = lr.scaled_ops(sp, ops)
    n, m = sp.n, sp.m
    psi = lr.start_vectors(sp)
    worst = 0.0
    for i in range(m):
        for j in range(m):
            v = np.outer(psi[:, i], np.conj(psi[:, j])).reshape(-1)
            for t in range(sp.steps):
                v = expm(lr.liouvillian(lr.generator(sp, Ds, r['uks'][:, t]), Ds)) @ v
            worst = max(worst, float(np.max(np.abs(v.reshape(n, n) - r['rho_final'][i, j]))))
            assert np.max(np.abs(r['rho_final'][j, i] - r['rho_final'][i, j].conj().T)) <= 1e-14
        assert abs(np.trace(r['rho_final'][i, i]) - 1.0) <= 1e-12
    print('largest deviation from expm of the Liouvillian: %.3e' % worst)
    assert worst <= 1e-12
    assert r['loss'] > 1e-3                                               # (decay is visible: not the closed limit in disguise)


# ---- (c) the first-order gradient is first order in dt ------------------------------------------------------------------------------------

def _gradient_error(steps):
    n, total = 3, 4.0
    rng = np.random.default_rng(7)
    H0, Hop = herm(rng, n), 0.8 * herm(rng, n)
    e0, e2 = np.eye(n)[0].astype(complex), np.eye(n)[2].astype(complex)
    np.random.seed(0)
    sp = go.OracleSystem(H0, [Hop], [e2], total, steps, [e0], maxA=[1.5], state_transfer=True, Taylor_terms=[14, 1], reg_coeffs={})
    ops = collapse_list(n, 2, 3)
    t = (np.arange(steps) + 0.5) / steps
    base = (0.7 * np.sin(2 * np.pi * t) + 0.3)[None, :]
    g = lr.evaluate(sp, ops, base)['grad']
    fd = np.zeros_like(g)
    eps = 1e-6
    for s in range(steps):
        bp, bm = base.copy(), base.copy()
        bp[0, s] += eps
        bm[0, s] -= eps
        fd[0, s] = (lr.evaluate(sp, ops, bp, want_grad=False)['loss'] - lr.evaluate(sp, ops, bm, want_grad=False)['loss']) / (2 * eps)
    return float(np.linalg.norm(g - fd) / np.linalg.norm(fd))


def test_first_order_gradient_against_central_differences():
    errs = [_gradient_error(s) for s in (5, 10, 20, 40)]
    ratios = [errs[i] / errs[i + 1] for i in range(3)]
    print('relative gradient error at 5, 10, 20, 40 slices: %s; ratios %s' % (errs, ratios))
    assert all(q >= 1.7 for q in ratios), (errs, ratios)


def test_reference_finds_the_route_around_the_lossy_level():
    """The Lambda system of examples/lossy_lambda_transfer.py with the reference in place of the engine: Adam from the example's fixed start, once
    without and once with the collapse operator, both pulses scored under the master equation.  100 iterations at degree 10 with two sub-steps
    per slice keep the test to seconds: 0.7826 against 0.0382 (300 iterations with the rule-chosen T = 6, s = 3: 0.7825 against 0.0318)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))
    import lossy_lambda_transfer as ex
    H0, Hops, _, start, target, ops = ex.problem()
    sp = go.OracleSystem(H0, Hops, [target], ex.TOTAL_TIME, ex.STEPS, [start], maxA=ex.MAXA, initial_guess=ex.initial_guess(), state_transfer=True,
                         Taylor_terms=[10, 1], reg_coeffs={})
    score = {}
    for name, used in (('closed', []), ('aware', ops)):
        base = lr.run_adam(sp, used, dict(ex.CONVERGENCE, max_iterations=100), sp.base0)['base']
        score[name] = lr.evaluate(sp, ops, base, want_grad=False)['loss']
    print('infidelity under decay: closed-optimised %.4f, optimised under the master equation %.4f' % (score['closed'], score['aware']))
    assert 2.0 * score['aware'] <= score['closed']


# ---- (d) the Taylor rule ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('unitary_error', [1e-4, 1e-8])
def test_choose_taylor(unitary_error):
    sp, ops = open_case(4, 2, 2, 12, (3, 0), 2, seed=4, dt=0.9)
    T, s = open_system.choose_taylor(sp.H0_in, sp.Hops_in, sp.maxA, ops, sp.dt, sp.steps, unitary_error)
    x = 2 * sp.dt * (np.linalg.norm(sp.H0_in, 2) + sum(a * np.linalg.norm(h, 2) for a, h in zip(sp.maxA, sp.Hops_in))
                     + sum(np.linalg.norm(c, 2) ** 2 for c in ops))
    bound = lambda T_, s_: sp.steps * 2.0 ** s_ * 2.0 * (x / 2.0 ** s_) ** (T_ + 1) / math.factorial(T_ + 1)
    assert x / 2.0 ** s <= 0.5 and (s == 0 or x / 2.0 ** (s - 1) > 0.5)
    assert T >= 2 and bound(T, s) <= unitary_error and (T == 2 or bound(T - 1, s) > unitary_error)
    assert s >= 1                                                         # (the case is not trivial)
    base = bases_of(sp)[1]
    sp.exp_terms, sp.scaling = T, s
    a = lr.evaluate(sp, ops, base, want_grad=False)['rho_final']
    sp.exp_terms = T + 6
    b = lr.evaluate(sp, ops, base, want_grad=False)['rho_final']
    print('T = %d, s = %d: deviation from T + 6 %.3e (unitary_error %.0e)' % (T, s, np.max(np.abs(a - b)), unitary_error))
    assert np.max(np.abs(a - b)) <= unitary_error


def test_choose_taylor_gives_up_past_the_engine_limits():
    H = np.diag([0.0, 1.0]).astype(complex)
    with pytest.raises(ValueError, match='sub-steps'):
        open_system.choose_taylor(1e5 * H, [H], [1.0], [], 1.0, 10, 1e-4)
    with pytest.raises(ValueError, match='Taylor terms'):
        open_system.choose_taylor(H, [H], [1.0], [], 0.2, 10, 1e-300)


# ---- (e) refusals of the Python layer -----------------------------------------------------------------------------------------------------

def test_validate_and_builders():
    a3 = open_system.relaxation(3, 4.0)
    assert np.allclose(a3, 0.5 * np.diag([1.0, math.sqrt(2.0)], 1))
    assert np.allclose(open_system.dephasing(3, 8.0), 0.5 * np.diag([0.0, 1.0, 2.0]))
    assert len(open_system.validate([a3, open_system.dephasing(3, 8.0)], 3)) == 2 and open_system.validate([], 3) == []
    for bad, msg in ((a3, 'a list'), ([np.eye(2)], 'shape'), ([np.full((3, 3), np.nan)], 'not finite'), ([np.zeros((3, 3))], 'all zero')):
        with pytest.raises(ValueError, match=msg):
            open_system.validate(bad, 3)
    for f in (open_system.relaxation, open_system.dephasing):
        with pytest.raises(ValueError):
            f(3, 0.0)


@functools.lru_cache(maxsize=None)
def _qubit():
    sx = np.array([[0, 1], [1, 0]], dtype=complex)
    return np.zeros((2, 2), dtype=complex), [sx], ['x'], sx


@pytest.mark.parametrize('extra, msg', [
    (dict(robust={}), 'robust'), (dict(transfer=np.eye(4)), 'transfer'), (dict(exact_gradient=True), 'exact_gradient'),
    (dict(time_comm=object()), 'time_comm'), (dict(dressed_info={'is_dressed': False}), 'dressed_info'),
    (dict(reg_coeffs={'forbidden_coeff_list': [1.0], 'states_forbidden_list': [1]}), 'forbidden-level'),
    (dict(reg_coeffs={'speed_up': 1.0}), 'speed_up'), (dict(reg_coeffs={'forbid_dressed': True}), 'forbid_dressed'),
    (dict(plan_seeds=4), 'sharded'), (dict(_first_seed=2), 'sharded')])
def test_grape_refuses_what_does_not_combine(extra, msg):
    H0, Hops, names, U = _qubit()
    kw = dict(save=False, show_plots=False, collapse_ops=[open_system.relaxation(2, 10.0)], reg_coeffs={})
    kw.update(extra)
    with pytest.raises(ValueError, match=msg):
        Grape(H0, Hops, names, U, 1.0, 4, [0, 1], **kw)


def test_grape_validates_the_list_and_the_sharded_entry_points_refuse():
    H0, Hops, names, U = _qubit()
    with pytest.raises(ValueError, match='shape'):
        Grape(H0, Hops, names, U, 1.0, 4, [0, 1], save=False, show_plots=False, reg_coeffs={}, collapse_ops=[np.eye(3)])
    ops = [open_system.relaxation(2, 10.0)]
    with pytest.raises(ValueError, match='GrapeSharded'):
        GrapeSharded(H0, Hops, names, U, 1.0, 4, [0, 1], save=False, show_plots=False, reg_coeffs={}, collapse_ops=ops, restarts=2)
    with pytest.raises(ValueError, match='GrapeTimeSharded'):
        GrapeTimeSharded(H0, Hops, names, U, 1.0, 4, [0, 1], save=False, show_plots=False, reg_coeffs={}, collapse_ops=ops)
    assert inspect.signature(Grape).parameters['collapse_ops'].kind is inspect.Parameter.KEYWORD_ONLY


@pytest.mark.parametrize('extra, msg', [
    (dict(ensemble=dict(amp_scales=[[1.0]], weights=[1.0])), 'ensemble'), (dict(transfer=np.eye(4)), 'transfer'),
    (dict(exact_gradient=True), 'exact_gradient'), (dict(time_shards=2), 'time sharding'), (dict(time_comm=object()), 'time sharding')])
def test_engine_refuses_what_does_not_combine(extra, msg, monkeypatch):
    monkeypatch.setattr(hip_engine, 'load_library', lambda: pytest.fail('the library was called'))
    H0, Hops, _, U = _qubit()
    Hs = np.stack([H0, -0.25j * Hops[0]])
    with pytest.raises(ValueError, match=msg):
        hip_engine.HipEngine(Hs, np.eye(2), np.eye(2), U, [1.0], 0.25, 1.0, 4, 6, 0, reg_coeffs={}, collapse_ops=[open_system.relaxation(2, 10.0)], **extra)
    with pytest.raises(ValueError, match='shape'):
        hip_engine.HipEngine(Hs, np.eye(2), np.eye(2), U, [1.0], 0.25, 1.0, 4, 6, 0, reg_coeffs={}, collapse_ops=[np.eye(3)])


def test_binding_declares_the_new_entry_points():
    assert hip_engine.PATH_LINDBLAD == 6
    for name in ('qoc_create_open', 'qoc_get_final_density', 'qoc_get_populations'):
        assert name in hip_engine.EXPORTED_SYMBOLS
    assert [f[0] for f in hip_engine.QocOpen._fields_] == ['n_collapse', 'C']
