"""Open-system running costs without a GPU: the NumPy reference of tests/running_cost_reference.py against the closed-system oracle
with forbidden levels (no collapse operator), its costates against an exact directional derivative, its gradient against central differences of its
own reg_loss; the builders and validate_costs of helper_functions/open_system.py; and every refusal of the Python layer that needs no library."""
import inspect

import numpy as np
import pytest

from oracle import grape_oracle as go
from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import open_system
from quantum_optimal_control.helper_functions.synthetic_systems import herm, random_unitary
from quantum_optimal_control.main_grape.grape import Grape, GrapeSharded, GrapeTimeSharded
from tests import running_cost_reference as rc
from tests.test_open_system import G_RTOL, S_RTOL, _qubit, bases_of, collapse_list, open_case


def dense_observable(n, seed):
    """A dense complex Hermitian observable of spectral norm 1."""
    O = herm(np.random.default_rng(700 + seed), n)
    return O / np.linalg.norm(O, 2)


# ---- 1. the closed limit --------------------------------------------------------------------------------------------------------------------

FORBID = {'forbidden_coeff_list': [2.0, 0.7], 'states_forbidden_list': [3, 1]}


def _closed_check(sp, oracle_sp, costs, with_tau0):
    """Gradient and reg_loss against the oracle's forbidden levels; with_tau0 False: both values without their tau = 0 terms (the reference's
    closed regulariser takes V at tau = 0, the running cost U0 V: DESIGN.md 6l)."""
    steps = sp.steps
    for base in bases_of(sp)[:2]:
        r = rc.evaluate(sp, [], costs, base)
        o = go.evaluate(oracle_sp, base)
        plain = go.evaluate(sp, base)
        gmax = float(np.max(np.abs(o['grad'])))
        err = float(np.max(np.abs(r['grad'] - o['grad'])))
        seen = float(np.max(np.abs(o['grad'] - plain['grad'])))
        mine, theirs = r['reg_loss'], o['reg_loss']
        if not with_tau0:
            mine -= rc.cost_value(costs, r['expectations'][:1], steps)
            Vd = oracle_sp.V if oracle_sp.Vs is None else oracle_sp.Vs.conj().T @ oracle_sp.V
            theirs -= sum(a / steps * 0.5 * np.sum(np.abs(Vd[s, :]) ** 4) for a, s in zip(FORBID['forbidden_coeff_list'], FORBID['states_forbidden_list']))
        print('closed limit: reg_loss %.17g / %.17g, gradient error %.3e of %.3e (the term moves it by %.3e)' % (mine, theirs, err, gmax, seen))
        assert seen > 1e-4 and o['reg_loss'] - o['loss'] > 1e-4                    # (the term is visible)
        assert abs(r['loss'] - o['loss']) <= S_RTOL * max(1.0, abs(o['loss']))
        assert abs(mine - theirs) <= S_RTOL * max(1.0, abs(theirs))
        assert err <= G_RTOL * gmax


def _level_costs(n):
    return [open_system.level_cost(n, s, a) for a, s in zip(FORBID['forbidden_coeff_list'], FORBID['states_forbidden_list'])]


def test_closed_limit_unitary_mode():
    sp, _ = open_case(4, 2, 3, 7, (14, 2), 0, seed=1)
    oracle_sp, _ = open_case(4, 2, 3, 7, (14, 2), 0, seed=1, reg_coeffs=FORBID)
    assert np.max(np.abs(sp.U0 - np.eye(4))) > 0.1
    _closed_check(sp, oracle_sp, _level_costs(4), with_tau0=False)


def test_closed_limit_state_transfer():
    """Degree 16 here is the closed engine's Taylor_terms = 17 in state transfer (sum over j < T); the values agree with their tau = 0 terms."""
    sp, _ = open_case(4, 2, 2, 7, (16, 0), 0, seed=2, state_transfer=True)
    oracle_sp, _ = open_case(4, 2, 2, 7, (17, 0), 0, seed=2, state_transfer=True, reg_coeffs=FORBID)
    _closed_check(sp, oracle_sp, _level_costs(4), with_tau0=True)


@pytest.mark.parametrize('state_transfer', [False, True])
def test_closed_limit_dressed(state_transfer):
    """forbid_dressed: the oracle projects on the columns of Vs, the running cost takes O = v v^dagger."""
    m, taylor = (2, (16, 0)) if state_transfer else (3, (14, 2))
    sp, _ = open_case(4, 2, m, 7, taylor, 0, seed=3, state_transfer=state_transfer)
    oracle_sp, _ = open_case(4, 2, m, 7, (17, 0) if state_transfer else taylor, 0, seed=3, state_transfer=state_transfer, reg_coeffs=FORBID)
    Vs = random_unitary(np.random.default_rng(11), 4)
    oracle_sp.Vs = Vs
    costs = [open_system.dressed_level_cost(Vs[:, s], a) for a, s in zip(FORBID['forbidden_coeff_list'], FORBID['states_forbidden_list'])]
    _closed_check(sp, oracle_sp, costs, with_tau0=state_transfer)


# ---- 2. the costate identity ------------------------------------------------------------------------------------------------------------------

def mixed_costs(n, seed=0):
    """One dense complex Hermitian observable with power 2 and one projector with power 1."""
    return [open_system.observable_cost(dense_observable(n, seed), 1.5, 2), open_system.subspace_cost(n, [n - 1, n - 2], 0.8, 1)]


def test_costates_are_the_derivative_with_respect_to_the_operators():
    """Exact, with no O(dt) error: eps delta injected into rho_ii(tau) and propagated on changes loss + R by eps Re <Lambda_ii(tau), delta> plus a term
    quadratic in eps, so central differences are exact up to rounding, about 1e-16 / h; with h = 1e-4, agreement to 1e-8 relative."""
    sp, ops = open_case(4, 2, 2, 6, (10, 1), 2, seed=5)
    costs = mixed_costs(4)
    base = bases_of(sp)[1]
    r = rc.evaluate(sp, ops, costs, base)
    assert np.max(np.abs(np.imag(costs[0][0]))) > 0.05
    rng = np.random.default_rng(9)
    h = 1e-4
    for tau in (2, 4):
        for i in range(sp.m):
            delta = rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4))
            f = []
            for sign in (1.0, -1.0):
                hist = np.array(r['hist'])
                hist[tau, i, i] += sign * h * delta
                f.append(rc.continue_from(sp, ops, costs, r['uks'], hist, tau))
            fd = (f[0] - f[1]) / (2 * h)
            want = float(np.real(np.sum(np.conj(r['costates'][tau, i, i]) * delta)))
            plain = float(np.real(np.sum(np.conj(rc.evaluate(sp, ops, [], base)['costates'][tau, i, i]) * delta)))
            print('tau %d, state %d: central difference %.12e, Re <Lambda, delta> %.12e (without the sources %.12e)' % (tau, i, fd, want, plain))
            assert abs(fd - want) <= 1e-8 * abs(want)
            assert abs(plain - want) > 1e-4 * abs(want)                         # (the sources are visible)


# ---- 3. first order in dt --------------------------------------------------------------------------------------------------------------------

def _gradient_error(steps):
    n, total = 3, 4.0
    rng = np.random.default_rng(7)
    H0, Hop = herm(rng, n), 0.8 * herm(rng, n)
    e0, e2 = np.eye(n)[0].astype(complex), np.eye(n)[2].astype(complex)
    np.random.seed(0)
    sp = go.OracleSystem(H0, [Hop], [e2], total, steps, [e0], maxA=[1.5], state_transfer=True, Taylor_terms=[14, 1], reg_coeffs={})
    ops = collapse_list(n, 2, 3)
    costs = [open_system.level_cost(n, 1, 3.0), open_system.observable_cost(dense_observable(n, 1), 1.0, 1)]
    t = (np.arange(steps) + 0.5) / steps
    base = (0.7 * np.sin(2 * np.pi * t) + 0.3)[None, :]
    g = rc.evaluate(sp, ops, costs, base)['grad']
    fd = np.zeros_like(g)
    eps = 1e-6
    for s in range(steps):
        bp, bm = base.copy(), base.copy()
        bp[0, s] += eps
        bm[0, s] -= eps
        fd[0, s] = (rc.evaluate(sp, ops, costs, bp, want_grad=False)['reg_loss'] - rc.evaluate(sp, ops, costs, bm, want_grad=False)['reg_loss']) / (2 * eps)
    return float(np.linalg.norm(g - fd) / np.linalg.norm(fd))


def test_first_order_gradient_against_central_differences():
    e10, e40 = _gradient_error(10), _gradient_error(40)
    print('relative gradient error of reg_loss at 10 and 40 slices: %.3e, %.3e (ratio %.2f; first order predicts 4)' % (e10, e40, e10 / e40))
    assert e40 <= 0.5 * e10


# ---- 4. builders and refusals ------------------------------------------------------------------------------------------------------------------

def test_builders():
    O, a, p = open_system.level_cost(4, 3, 0.5)
    assert (a, p) == (0.5, 2) and O.dtype == np.complex128 and np.array_equal(O, np.diag([0, 0, 0, 1.0]))
    O, a, p = open_system.subspace_cost(4, [2, 3], 1.5, power=1)
    assert (a, p) == (1.5, 1) and np.array_equal(O, np.diag([0, 0, 1.0, 1.0]))
    v = np.array([1.0, 1j, 0.0]) / np.sqrt(2.0)
    O, a, p = open_system.dressed_level_cost(v, 2.0)
    assert np.allclose(O, np.outer(v, v.conj())) and abs(np.trace(O) - 1.0) < 1e-15 and (a, p) == (2.0, 2)
    H = dense_observable(3, 0)
    O, a, p = open_system.observable_cost(H, 0.25, 1)
    assert np.array_equal(O, H) and O is not H and (a, p) == (0.25, 1)
    with pytest.raises(ValueError, match='outside'):
        open_system.subspace_cost(4, [4], 1.0)


def test_validate_costs():
    n = 3
    good = [open_system.level_cost(n, 2, 1.0), open_system.observable_cost(dense_observable(n, 2), -0.5, 1)]
    out = open_system.validate_costs(good, n)
    assert len(out) == 2 and all(o[0].shape == (n, n) and o[0].dtype == np.complex128 and o[0].flags['C_CONTIGUOUS'] for o in out)
    assert [o[1:] for o in out] == [(1.0, 2), (-0.5, 1)] and open_system.validate_costs([], n) == []
    assert len(open_system.validate_costs([good[0]] * 16, n)) == 16
    skew = np.array(dense_observable(n, 2))
    skew[0, 1] += 1e-9
    for bad, msg in ((np.eye(n), 'a list'), (good[0], 'record'), ([good[0]] * 17, 'at most 16'), ([(np.eye(2), 1.0, 2)], 'shape'), ([(np.eye(n), 1.0)], 'record'),
                     ([(skew, 1.0, 2)], 'not Hermitian'), ([(1j * np.eye(n), 1.0, 2)], 'not Hermitian'), ([(np.eye(n), np.inf, 2)], 'not finite'),
                     ([(np.eye(n), np.nan, 1)], 'not finite'), ([(np.full((n, n), np.nan), 1.0, 2)], 'not finite'), ([(np.eye(n), 1.0, 3)], 'power'),
                     ([(np.eye(n), 1.0, 0)], 'power'), ([(np.eye(n), 1.0, 1.5)], 'power'), ([(np.eye(n), 'x', 1)], 'not numeric')):
        with pytest.raises(ValueError, match=msg):
            open_system.validate_costs(bad, n)
    within = np.array(dense_observable(n, 2))
    within[0, 1] += 1e-14
    open_system.validate_costs([(within, 1.0, 2)], n)


def _grape(**kw):
    H0, Hops, names, U = _qubit()
    args = dict(save=False, show_plots=False, reg_coeffs={})
    args.update(kw)
    return Grape(H0, Hops, names, U, 1.0, 4, [0, 1], **args)


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(hip_engine, 'load_library', lambda: pytest.fail('the library was called'))


def test_grape_refuses_running_costs_on_closed_engines(no_library):
    cost = [open_system.level_cost(2, 1, 1.0)]
    robust = dict(operators=[np.diag([0.0, 1.0])], offsets=[[0.0], [0.1]])
    for extra in ({}, dict(robust=robust), dict(transfer=np.eye(4)), dict(exact_gradient=True)):
        with pytest.raises(ValueError, match='forbidden_coeff_list'):
            _grape(running_costs=cost, **extra)
    from quantum_optimal_control.helper_functions import fleet as fl_mod
    fl = fl_mod.Fleet([np.diag([0.0, 1.0])], np.zeros((2, 1, 1)), np.ones((2, 1, 1)))
    with pytest.raises(ValueError, match='forbidden_coeff_list'):
        _grape(running_costs=cost, fleet=fl)


def test_grape_validates_the_costs_before_the_library(no_library):
    ops = [open_system.relaxation(2, 10.0)]
    for bad, msg in (([(np.eye(3), 1.0, 2)], 'shape'), ([(np.eye(2), 1.0, 4)], 'power'), ([open_system.level_cost(2, 1, 1.0)] * 17, 'at most 16'),
                     (open_system.level_cost(2, 1, 1.0), 'record'), ([(np.array([[0, 1], [0, 0]]), 1.0, 2)], 'not Hermitian')):
        with pytest.raises(ValueError, match=msg):
            _grape(collapse_ops=ops, running_costs=bad)
        with pytest.raises(ValueError, match=msg):
            _grape(robust=dict(weights=[0.5, 0.5], collapse_ops=ops, rate_scales=[[1.0], [2.0]]), running_costs=bad)
    # what an open call refuses stays refused beside the costs
    for extra, msg in ((dict(reg_coeffs={'forbidden_coeff_list': [1.0], 'states_forbidden_list': [1]}), 'forbidden-level'),
                       (dict(reg_coeffs={'speed_up': 1.0}), 'speed_up'), (dict(exact_gradient=True), 'exact_gradient'), (dict(transfer=np.eye(4)), 'transfer')):
        with pytest.raises(ValueError, match=msg):
            _grape(collapse_ops=ops, running_costs=[open_system.level_cost(2, 1, 1.0)], **extra)


def test_the_keyword_and_the_sharded_entry_points():
    params = list(inspect.signature(Grape).parameters)
    assert params[params.index('fleet') + 1] == 'running_costs' and params[params.index('running_costs') + 1] == '_first_seed'
    assert inspect.signature(Grape).parameters['running_costs'].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(Grape).parameters['running_costs'].default is None
    assert inspect.signature(hip_engine.HipEngine.__init__).parameters['running_costs'].default is None
    H0, Hops, names, U = _qubit()
    kw = dict(save=False, show_plots=False, reg_coeffs={}, collapse_ops=[], running_costs=[open_system.level_cost(2, 1, 1.0)])
    with pytest.raises(ValueError, match='GrapeSharded'):
        GrapeSharded(H0, Hops, names, U, 1.0, 4, [0, 1], restarts=2, **kw)
    with pytest.raises(ValueError, match='GrapeTimeSharded'):
        GrapeTimeSharded(H0, Hops, names, U, 1.0, 4, [0, 1], **kw)
    del kw['collapse_ops']
    with pytest.raises(ValueError, match='GrapeSharded: running_costs'):
        GrapeSharded(H0, Hops, names, U, 1.0, 4, [0, 1], restarts=2, **kw)
    with pytest.raises(ValueError, match='GrapeTimeSharded: running_costs'):
        GrapeTimeSharded(H0, Hops, names, U, 1.0, 4, [0, 1], **kw)


def test_engine_refuses_running_costs_without_an_open_engine(no_library):
    H0, Hops, _, U = _qubit()
    Hs = np.stack([H0, -0.25j * Hops[0]])
    cost = [open_system.level_cost(2, 1, 1.0)]
    make = lambda **kw: hip_engine.HipEngine(Hs, np.eye(2), np.eye(2), U, [1.0], 0.25, 1.0, 4, 6, 0, reg_coeffs={}, **kw)
    with pytest.raises(ValueError, match='forbidden_coeff_list'):
        make(running_costs=cost)
    with pytest.raises(ValueError, match='forbidden_coeff_list'):
        make(running_costs=cost, ensemble=dict(amp_scales=[[1.0]], weights=[1.0]))
    with pytest.raises(ValueError, match='power'):
        make(running_costs=[(np.eye(2), 1.0, 3)], collapse_ops=[])
    with pytest.raises(ValueError, match='shape'):
        make(running_costs=[(np.eye(3), 1.0, 2)], ensemble=dict(amp_scales=[[1.0]], weights=[1.0], collapse_ops=[open_system.relaxation(2, 10.0)]))


def test_binding_declares_the_new_entry_points():
    for name in ('qoc_create_open_costs', 'qoc_get_expectations'):
        assert name in hip_engine.EXPORTED_SYMBOLS
    assert [f[0] for f in hip_engine.QocRunningCosts._fields_] == ['n_obs', 'O', 'coeffs', 'powers']
    assert len(hip_engine._SIGNATURES['qoc_create_open_costs'][1]) == len(hip_engine._SIGNATURES['qoc_create_open_fleet'][1]) + 1


# ---- 5. the GPU rows, checked where no GPU is needed ----------------------------------------------------------------------------------------------

def test_the_gpu_rows_see_the_costs_and_the_start():
    """The parity rows of tests/test_running_costs_gpu.py: without the sources the gradient of a row is far from the reference's, and with U0 != I the
    tau = 0 expectation values are not those of V itself -- the rows cannot pass with the sources left out or with the start taken from V."""
    from tests import lindblad_reference as lr
    from tests import test_running_costs_gpu as rows
    for name in ('n3_m2', 'scaling2'):
        (sp, ops, costs), refs = rows.system(name), rows.reference(name)
        plain = lr.evaluate(sp, ops, bases_of(sp)[1])
        assert np.max(np.abs(plain['grad'] - refs[1]['grad'])) > 1e-3 * np.max(np.abs(refs[1]['grad']))
    (sp, ops, costs), refs = rows.system('unitary_u0'), rows.reference('unitary_u0')
    from_V = np.array([[np.real(np.conj(sp.V[:, i]) @ O @ sp.V[:, i]) for i in range(sp.m)] for O, _, _ in costs])
    assert np.max(np.abs(from_V - refs[0]['expectations'][0])) > 1e-2


# ---- 6. the run log ---------------------------------------------------------------------------------------------------------------------------------

class LibraryTouched(Exception):
    pass


class RecordingLog(object):
    """Stands in for the HDF5 run log (data_management.H5File): what a call adds, by key."""
    seen = {}

    def __init__(self, path, mode='a'):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def add(self, key, data=None, **kw):
        RecordingLog.seen[key] = np.array(data)

    append = add

    def create_group(self, name):
        return self

    def create_dataset(self, key, data=None):
        pass


def test_save_logs_the_running_costs(monkeypatch, tmp_path):
    """save=True writes the inputs before anything is built: the log holds the observables, coefficients and powers next to collapse_ops -- arrays of
    length 0 for an empty list, none of the three without the keyword."""
    from quantum_optimal_control.helper_functions import data_management

    def touched():
        raise LibraryTouched()
    monkeypatch.setattr(hip_engine, 'load_library', touched)
    monkeypatch.setattr(data_management, 'H5File', RecordingLog)
    keys = ['running_cost_observables', 'running_cost_coeffs', 'running_cost_powers']
    O = dense_observable(2, 4)
    given = [open_system.level_cost(2, 1, 3.0), open_system.observable_cost(O, -0.5, 1)]
    for costs in (None, [], given):
        RecordingLog.seen = {}
        with pytest.raises(LibraryTouched):
            _grape(save=True, file_name='costs', data_path=str(tmp_path), convergence={'max_iterations': 2}, collapse_ops=[open_system.relaxation(2, 10.0)],
                   running_costs=costs)
        seen = RecordingLog.seen
        assert 'collapse_ops' in seen and [key in seen for key in keys] == [costs is not None] * 3, sorted(seen)
        if costs is not None:
            obs, coeffs, powers = (seen[key] for key in keys)
            assert obs.shape == (len(costs), 2, 2) and obs.dtype == np.complex128 and coeffs.shape == powers.shape == (len(costs),)
            assert coeffs.dtype == np.float64 and powers.dtype == np.int32
    assert np.array_equal(obs[0], np.diag([0.0, 1.0])) and np.array_equal(obs[1], O) and list(coeffs) == [3.0, -0.5] and list(powers) == [2, 1]
