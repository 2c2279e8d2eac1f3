"""Control maps without a GPU: the builders and validate of helper_functions/control_map.py, the formula and its chain rule, the composed
reference of tests/control_map_reference.py against central differences, the identity map, the Taylor rule, and what Grape and HipEngine refuse
before the library is loaded."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sps

from oracle import grape_oracle as go
from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import control_map as cmap
from quantum_optimal_control.helper_functions import open_system
from quantum_optimal_control.main_grape.grape import Grape, GrapeSharded, GrapeTimeSharded
from tests import control_map_reference as ref


# ---- builders ---------------------------------------------------------------------------------------------------------------------------------

def test_linear_and_identity():
    X = np.array([[1.0, 0.1], [0.2, 1.0], [0.0, -0.5]])
    cm = cmap.linear(X)
    assert (cm.n_terms, cm.n_pulses, cm.degree) == (3, 2, 1) and cm.mix is None and cm.fixed is None and cm.steps is None
    v = np.random.default_rng(0).normal(size=(2, 7))
    assert np.allclose(cmap.apply(cm, v), X @ v, rtol=0, atol=1e-15)
    assert np.array_equal(cmap.identity(3).alpha[:, :, 0], np.eye(3))
    with pytest.raises(ValueError, match=r'control_map.linear: X has shape'):
        cmap.linear(np.ones(3))


def test_carriers_at_the_slice_midpoints():
    steps, total = 8, 4.0
    cm = cmap.carriers([0.5, 1.25], [0.0, 0.3], total, steps)
    assert (cm.n_terms, cm.n_pulses, cm.degree) == (4, 2, 1) and cm.steps == steps
    t = (np.arange(steps) + 0.5) * total / steps
    assert np.allclose(cm.mix[0, 0], np.cos(2 * np.pi * 0.5 * t), rtol=0, atol=1e-15)
    assert np.allclose(cm.mix[3, 1], np.sin(2 * np.pi * 1.25 * t + 0.3), rtol=0, atol=1e-15)
    assert not np.any(cm.mix[0, 1]) and not np.any(cm.mix[2, 0]) and not np.any(cm.alpha[0, 1]) and not np.any(cm.alpha[3, 0])
    v = np.random.default_rng(1).normal(size=(2, steps))
    c = cmap.apply(cm, v)
    assert np.allclose(c[2], v[1] * np.cos(2 * np.pi * 1.25 * t + 0.3), rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match='at least one carrier'):
        cmap.carriers([], [], 1.0, 4)


def test_polynomial_fixed_and_the_combinations():
    a = np.array([[1.0, 0.0, -0.1], [1.0, 0.0, -0.2]])
    p = cmap.polynomial(a)
    assert (p.n_terms, p.n_pulses, p.degree) == (2, 2, 3) and not np.any(p.alpha[0, 1]) and np.array_equal(p.alpha[1, 1], a[1])
    assert cmap.polynomial(np.ones((3, 2, 4))).alpha.shape == (3, 2, 4)
    with pytest.raises(ValueError, match=r'control_map.polynomial: alpha has shape'):
        cmap.polynomial(np.ones(4))
    X = np.array([[1.0, 0.1], [0.1, 1.0]])
    v = np.random.default_rng(2).normal(size=(2, 5))
    chain = cmap.compose(cmap.linear(X), p)
    pv = a[:, 0:1] * v + a[:, 2:3] * v ** 3
    assert np.allclose(cmap.apply(chain, v), X @ pv, rtol=0, atol=1e-14)
    F = np.random.default_rng(3).normal(size=(2, 5))
    with_drive = cmap.combine(chain, cmap.fixed(F))
    assert np.allclose(cmap.apply(with_drive, v), X @ pv + F, rtol=0, atol=1e-14)
    below = cmap.stack(chain, cmap.fixed(F[:1]))
    assert below.n_terms == 3 and np.allclose(cmap.apply(below, v), np.concatenate([X @ pv, F[:1]]), rtol=0, atol=1e-14)
    both = cmap.combine(cmap.linear(X), cmap.polynomial(np.array([[0.0, 0.5], [0.0, -0.5]])))
    assert np.allclose(cmap.apply(both, v), X @ v + np.array([[0.5], [-0.5]]) * v ** 2, rtol=0, atol=1e-14)
    with pytest.raises(ValueError, match=r'control_map.fixed: the waveforms have shape'):
        cmap.fixed(np.ones(4))
    with pytest.raises(ValueError, match='the inner map must give every line its own polynomial'):
        cmap.compose(cmap.linear(X), cmap.linear(X))
    with pytest.raises(ValueError, match='the outer map must be of degree 1'):
        cmap.compose(p, p)
    with pytest.raises(ValueError, match='the outer map takes 3 pulses, the inner one delivers 2'):
        cmap.compose(cmap.linear(np.ones((2, 3))), p)
    with pytest.raises(ValueError, match='nothing to combine'):
        cmap.combine()
    with pytest.raises(ValueError, match='nothing to stack'):
        cmap.stack()
    with pytest.raises(ValueError, match='maps of 2 and 3 operators'):
        cmap.combine(cmap.linear(X), cmap.linear(np.ones((3, 2))))
    with pytest.raises(ValueError, match=r'control_map.stack: the maps take different numbers of pulses'):
        cmap.stack(cmap.linear(X), cmap.linear(np.ones((2, 3))))
    with pytest.raises(ValueError, match='different numbers of time slices'):
        cmap.combine(cmap.carriers([1.0], [0.0], 1.0, 4), cmap.fixed(np.ones((2, 5))))
    with pytest.raises(ValueError, match='pulse 0 reaches operator 0 through two different mixes'):
        cmap.combine(cmap.carriers([1.0], [0.0], 1.0, 4), cmap.linear(np.ones((2, 1))))


VALIDATE_ERRORS = [
    (lambda: 3.0, {}, 'a helper_functions.control_map.ControlMap'),
    (lambda: dict(alpha=np.ones((1, 1, 1)), gain=1), {}, 'unknown keys'),
    (lambda: dict(mix=np.ones((1, 1, 4))), {}, r'alpha \(r x k x D\) is required'),
    (lambda: cmap.ControlMap(np.ones((2, 2))), {}, r'alpha has shape \(2, 2\), expected \(r, k, D\)'),
    (lambda: cmap.fixed(np.ones((2, 4))), {}, r'alpha has shape \(2, 0, 1\)'),
    (lambda: cmap.ControlMap(np.ones((65, 1, 1))), {}, '65 operators, at most 64'),
    (lambda: cmap.ControlMap(np.ones((1, 1, 9))), {}, 'degree 9, at most 8'),
    (lambda: cmap.identity(2), dict(k=3), 'the map takes 2 pulses, the problem has 3'),
    (lambda: cmap.identity(2), dict(r=3), 'the map feeds 2 operators, the problem has 3'),
    (lambda: cmap.ControlMap(np.ones((2, 2, 1)), mix=np.ones((2, 2, 5))), dict(steps=4), r'mix has shape \(2, 2, 5\), expected \(2, 2, 4\)'),
    (lambda: cmap.ControlMap(np.ones((2, 2, 1)), mix=np.ones((2, 3, 4))), {}, r'mix has shape \(2, 3, 4\), expected \(2, 2, steps\)'),
    (lambda: cmap.ControlMap(np.ones((2, 2, 1)), fixed=np.ones((3, 4))), {}, r'fixed has shape \(3, 4\), expected \(2, steps\)'),
    (lambda: cmap.ControlMap(np.ones((2, 2, 1)), fixed=np.ones((2, 5))), dict(steps=4), r'fixed has shape \(2, 5\), expected \(2, 4\)'),
    (lambda: cmap.ControlMap(np.ones((2, 2, 1)), mix=np.ones((2, 2, 4)), fixed=np.ones((2, 5))), {}, 'mix has 4 time slices, fixed 5'),
    (lambda: cmap.ControlMap(np.array([[[np.nan]]])), {}, 'alpha has a non-finite entry'),
    (lambda: cmap.ControlMap(np.ones((1, 1, 1)), mix=np.full((1, 1, 3), np.inf)), {}, 'mix has a non-finite entry'),
    (lambda: cmap.ControlMap(np.ones((1, 1, 1)), fixed=np.full((1, 3), np.nan)), {}, 'fixed has a non-finite entry'),
    (lambda: cmap.linear([[1.0, 0.0], [0.5, 0.0]]), {}, 'pulse 1 reaches no operator'),
]


@pytest.mark.parametrize('make, kw, msg', VALIDATE_ERRORS, ids=[row[2][:40] for row in VALIDATE_ERRORS])
def test_validate_names_the_cause(make, kw, msg):
    with pytest.raises(ValueError, match=msg):
        cmap.validate(make(), **kw)


def test_a_pulse_that_reaches_nothing_through_its_mix():
    alpha = np.ones((2, 2, 2))
    mix = np.ones((2, 2, 4))
    mix[:, 0] = 0.0                                         # pulse 0: every polynomial is there, every mix is zero
    with pytest.raises(ValueError, match='pulse 0 reaches no operator'):
        cmap.validate(cmap.ControlMap(alpha, mix=mix))
    mix[1, 0, 2] = -0.5                                     # one slice of one operator is enough
    out = cmap.validate(dict(alpha=alpha, mix=mix), k=2, r=2, steps=4)
    assert isinstance(out, cmap.ControlMap) and out.alpha.flags['C_CONTIGUOUS'] and out.mix.dtype == np.float64


# ---- the formula and its chain rule -------------------------------------------------------------------------------------------------------------

def test_apply_against_a_triple_loop():
    k, r, D, steps = 2, 3, 3, 6
    cm = ref.make_map(k, r, D, steps, mix=True, fixed=True)
    v = np.random.default_rng(4).normal(size=(k, steps))
    want = np.zeros((r, steps))
    for i in range(r):
        for t in range(steps):
            acc = cm.fixed[i, t]
            for j in range(k):
                acc += cm.mix[i, j, t] * sum(cm.alpha[i, j, d - 1] * v[j, t] ** d for d in range(1, D + 1))
            want[i, t] = acc
    assert np.allclose(cmap.apply(cm, v), want, rtol=0, atol=1e-14)
    bare = cmap.ControlMap(cm.alpha)
    assert np.allclose(cmap.apply(bare, v), cmap.apply(cmap.ControlMap(cm.alpha, np.ones((r, k, steps)), np.zeros((r, steps))), v), rtol=0, atol=1e-15)


def test_jacobian_against_central_differences():
    """r != k, D = 3.  h = 1e-5 on a cubic of coefficients <= 1 at |v| ~ 1: truncation h^2 |p'''| / 6 ~ 1e-10, rounding eps |c| / h ~ 1e-11."""
    k, r, D, steps = 2, 3, 3, 5
    cm = ref.make_map(k, r, D, steps, mix=True, fixed=True, seed=1)
    v = np.random.default_rng(5).normal(size=(k, steps))
    J = cmap.jacobian(cm, v)
    assert J.shape == (r, k, steps)
    h = 1e-5
    for j in range(k):
        for t in range(steps):
            vp, vm = v.copy(), v.copy()
            vp[j, t] += h
            vm[j, t] -= h
            col = (cmap.apply(cm, vp) - cmap.apply(cm, vm)) / (2 * h)
            assert np.max(np.abs(col[:, t] - J[:, j, t])) <= 1e-8
            col[:, t] = 0.0
            assert not np.any(col)                          # slice t of a pulse reaches slice t of the coefficients only
    g = np.random.default_rng(6).normal(size=(r, steps))
    assert np.allclose(cmap.pullback(cm, v, g), np.einsum('it,ijt->jt', g, J), rtol=0, atol=1e-15)


@pytest.mark.parametrize('state_transfer', [False, True], ids=['unitary', 'state'])
def test_composed_gradient_against_central_differences(state_transfer):
    """The whole composed gradient -- map, three members with a perturbation, a hold line, pulse and state regularisers, the exact reference of
    tests/exact_gradient_reference.py for dJ/dc -- against central differences of the composed reg_loss, with the step h = 1e-6 and the bound
    1e-7 of the gradient's largest entry that tests/test_exact_gradient.py uses for its own such check."""
    from quantum_optimal_control.helper_functions import transfer as tf
    regs = {'dwdt': 0.1, 'amplitude': 0.2, 'forbidden_coeff_list': [5.0], 'states_forbidden_list': [3], 'speed_up': 0.3}
    c = ref.problem(4, 3, 2, 6, 2, state_transfer=state_transfer, taylor=(6, 1), seed=3, total_time=2.0, regs=regs)
    cm = ref.make_map(2, 3, 3, 6, mix=True, fixed=True, seed=2)
    ens = ref.ensemble(c, 3, 1)
    T = tf.hold(6, 4).matrix
    x = ref.variables(2, 4, 1)[0]
    o = ref.evaluate(c, cm, ens, x, T=T, exact=True)
    fd = ref.central_differences(lambda y: ref.evaluate(c, cm, ens, y, T=T, want_grad=False)['reg_loss'], x, h=1e-6)
    gmax = float(np.max(np.abs(o['grad'])))
    err = float(np.max(np.abs(o['grad'] - fd)))
    print('composed exact gradient against central differences: max error %.3e of max %.3e' % (err, gmax))
    assert err <= 1e-7 * max(gmax, 1e-3), (err, gmax)


# ---- the identity map -------------------------------------------------------------------------------------------------------------------------

def test_identity_map_is_no_map():
    k, steps = 3, 7
    ident = cmap.validate(cmap.identity(k))
    v = np.random.default_rng(7).normal(size=(k, steps))
    g = np.random.default_rng(8).normal(size=(k, steps))
    assert np.array_equal(cmap.apply(ident, v), v) and np.array_equal(cmap.pullback(ident, v, g), g)
    # the composed reference with the identity map is the oracle on the problem itself
    regs = {'dwdt': 0.1, 'amplitude': 0.2, 'forbidden_coeff_list': [5.0], 'states_forbidden_list': [3], 'speed_up': 0.3}
    c = ref.problem(4, k, k, steps, 2, seed=4, regs=regs)
    np.random.seed(0)
    sp = go.OracleSystem(c['H0'], c['Hops'], c['U'], c['total_time'], steps, c['states_concerned_list'], U0=c['U0'], reg_coeffs=regs, maxA=c['maxA'],
                         Taylor_terms=c['Taylor_terms'])
    x = ref.variables(k, steps, 1)[0]
    o, want = ref.evaluate(c, ident, ref.ensemble(c, 1, 0), x), go.evaluate(sp, x)
    for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale'):
        assert abs(o[key] - want[key]) <= 1e-12 * max(1.0, abs(want[key])), key
    assert np.max(np.abs(o['grad'] - want['grad'])) <= 1e-11 * max(1.0, np.max(np.abs(want['grad'])))
    assert np.max(np.abs(o['coefficients'] - want['uks'])) <= 4e-16 * np.max(c['maxA'])


# ---- the Taylor rule --------------------------------------------------------------------------------------------------------------------------

def test_coefficient_bounds_and_the_taylor_rule():
    k, r, D, steps = 2, 3, 3, 6
    cm = ref.make_map(k, r, D, steps, mix=True, fixed=True, seed=3)
    bound = np.array([1.5, 0.7])
    want = np.zeros(r)
    for i in range(r):
        want[i] = np.max(np.abs(cm.fixed[i]))
        for j in range(k):
            want[i] += np.max(np.abs(cm.mix[i, j])) * sum(abs(cm.alpha[i, j, d - 1]) * bound[j] ** d for d in range(1, D + 1))
    assert np.allclose(cmap.coefficient_bounds(cm, bound), want, rtol=1e-14, atol=0)
    # no value of the pulses within the bound leaves it
    v = np.random.default_rng(9).uniform(-1, 1, size=(k, steps)) * bound[:, None]
    assert np.all(np.max(np.abs(cmap.apply(cm, v)), axis=1) <= want)
    assert np.array_equal(cmap.coefficient_bounds(cmap.identity(2), bound), bound)
    # the chooser on (H0, Hops, cmax): the oracle's restatement of it gives the same pair; an ensemble takes the maximum over its members
    c = ref.problem(6, r, k, steps, 3, seed=5, total_time=3.0)
    U0 = np.identity(6)
    got = cmap.choose_taylor(cm, c['H0'], c['Hops'], None, bound, U0, c['total_time'], steps, 1e-4, False, False)
    assert got == tuple(go.choose_taylor(c['H0'], c['Hops'], want, U0, c['total_time'] / steps, steps, 1e-4, False, False)[:2])
    ens = ref.ensemble(c, 3, 1)
    pairs = []
    for e in range(3):
        H0e = c['H0'] + ens['offsets'][e, 0] * ens['operators'][0]
        cmax = cmap.coefficient_bounds(cm, np.abs(ens['amp_scales'][e]) * bound)
        pairs.append(go.choose_taylor(H0e, c['Hops'], cmax, U0, c['total_time'] / steps, steps, 1e-4, False, False)[:2])
    assert cmap.choose_taylor(cm, c['H0'], c['Hops'], ens, bound, U0, c['total_time'], steps, 1e-4, False, False) == \
        (max(p[0] for p in pairs), max(p[1] for p in pairs))
    # a stronger map needs no fewer terms and squarings than a weaker one
    strong = cmap.linear(8.0 * np.eye(r, k) + 1.0)
    weak = cmap.linear(0.01 * (np.eye(r, k) + 1.0))
    ts, tw = (cmap.choose_taylor(m, c['H0'], c['Hops'], None, bound, U0, c['total_time'], steps, 1e-4, False, False) for m in (strong, weak))
    assert sum(ts) > sum(tw), (ts, tw)


# ---- signatures and refusals, before the library is loaded ------------------------------------------------------------------------------------

def _qubits():
    sx, sy, sz = np.array([[0, 1], [1, 0]], dtype=complex), np.array([[0, -1j], [1j, 0]]), np.diag([1.0, -1.0]).astype(complex)
    return 0.5 * sz, [sx, sy, sz], ['a', 'b'], sx


def test_signatures():
    for fn, name in ((Grape, 'control_map'), (hip_engine.HipEngine.__init__, 'control_map')):
        assert inspect.signature(fn).parameters[name].default is None
    params = list(inspect.signature(Grape).parameters)
    assert inspect.signature(Grape).parameters['control_map'].kind is inspect.Parameter.KEYWORD_ONLY
    assert params.index('control_map') > max(params.index(p) for p in ('transfer', 'exact_gradient', 'collapse_ops'))
    assert {'qoc_create_mapped', 'qoc_get_coefficients'} <= set(hip_engine.EXPORTED_SYMBOLS)
    fields = [f[0] for f in hip_engine.QocControlMap._fields_]
    assert fields == ['n_terms', 'degree', 'poly', 'mix', 'fixed']


def test_grape_refuses_before_the_library_loads(monkeypatch):
    monkeypatch.setattr(hip_engine, 'load_library', lambda: pytest.fail('the library was called'))
    H0, Hops, names, U = _qubits()
    cm = cmap.linear(np.array([[1.0, 0.0], [0.0, 1.0], [0.1, 0.1]]))
    kw = dict(save=False, show_plots=False, reg_coeffs={}, control_map=cm)
    with pytest.raises(ValueError, match=r'control_map does not combine with collapse_ops'):
        Grape(H0, Hops, names, U, 1.0, 4, [0, 1], collapse_ops=[open_system.relaxation(2, 10.0)], **kw)
    with pytest.raises(ValueError, match=r'control_map does not combine with scipy.sparse Hamiltonians'):
        Grape(sps.csr_matrix(H0), [sps.csr_matrix(h) for h in Hops], names, [np.array([0, 1.0])], 1.0, 4, [np.array([1.0, 0])], state_transfer=True, **kw)
    with pytest.raises(ValueError, match=r'control_map does not combine with time_comm'):
        Grape(H0, Hops, names, U, 1.0, 4, [0, 1], time_comm=object(), **kw)
    with pytest.raises(ValueError, match='GrapeSharded'):
        GrapeSharded(H0, Hops, names, U, 1.0, 4, [0, 1], restarts=2, **kw)
    with pytest.raises(ValueError, match='GrapeTimeSharded'):
        GrapeTimeSharded(H0, Hops, names, U, 1.0, 4, [0, 1], **kw)
    with pytest.raises(ValueError, match='does not run sharded'):
        Grape(H0, Hops, names, U, 1.0, 4, [0, 1], plan_seeds=4, **kw)
    # the map against the problem: r operators, k names / amplitudes / guesses
    with pytest.raises(ValueError, match='the map feeds 3 operators, the problem has 2'):
        Grape(H0, Hops[:2], names, U, 1.0, 4, [0, 1], **kw)
    with pytest.raises(ValueError, match=r'Hnames has one entry per pulse \(2\), got 3'):
        Grape(H0, Hops, ['a', 'b', 'c'], U, 1.0, 4, [0, 1], **kw)
    with pytest.raises(ValueError, match=r'maxA has one entry per pulse \(2\), got 3'):
        Grape(H0, Hops, names, U, 1.0, 4, [0, 1], maxA=[1.0, 1.0, 1.0], **kw)
    with pytest.raises(ValueError, match=r'initial_guess has one entry per pulse \(2\), got 3'):
        Grape(H0, Hops, names, U, 1.0, 4, [0, 1], initial_guess=np.zeros((3, 4)), **kw)
    with pytest.raises(ValueError, match='mix has shape'):
        Grape(H0, Hops[:2], names, U, 1.0, 4, [0, 1], **dict(kw, control_map=cmap.carriers([1.0], [0.0], 1.0, 5)))


@pytest.mark.parametrize('extra, msg', [
    (dict(collapse_ops=[open_system.relaxation(2, 10.0)]), 'collapse_ops'), (dict(sparse_ops=[sps.identity(2)] * 3), 'sparse_ops'),
    (dict(time_shards=2), 'time sharding'), (dict(time_comm=object()), 'time sharding')])
def test_engine_refuses_what_does_not_combine(extra, msg, monkeypatch):
    monkeypatch.setattr(hip_engine, 'load_library', lambda: pytest.fail('the library was called'))
    H0, Hops, _, U = _qubits()
    Hs = np.stack([-0.25j * H0] + [-0.25j * h for h in Hops[:2]])
    with pytest.raises(ValueError, match='control_map does not combine with ' + msg):
        hip_engine.HipEngine(Hs, np.eye(2), np.eye(2), U, [1.0, 1.0], 0.25, 1.0, 4, 6, 0, reg_coeffs={}, control_map=cmap.identity(2), **extra)


def test_engine_checks_the_map_against_its_arrays(monkeypatch):
    monkeypatch.setattr(hip_engine, 'load_library', lambda: pytest.fail('the library was called'))
    H0, Hops, _, U = _qubits()
    Hs = np.stack([-0.25j * H0] + [-0.25j * h for h in Hops])
    with pytest.raises(ValueError, match='the map takes 2 pulses, the problem has 3'):
        hip_engine.HipEngine(Hs, np.eye(2), np.eye(2), U, [1.0, 1.0, 1.0], 0.25, 1.0, 4, 6, 0, reg_coeffs={}, control_map=cmap.linear(np.ones((3, 2))))
    with pytest.raises(ValueError, match='the map feeds 2 operators, the problem has 3'):
        hip_engine.HipEngine(Hs, np.eye(2), np.eye(2), U, [1.0, 1.0], 0.25, 1.0, 4, 6, 0, reg_coeffs={}, control_map=cmap.identity(2))
    with pytest.raises(ValueError, match='pulse 1 reaches no operator'):
        hip_engine.HipEngine(Hs, np.eye(2), np.eye(2), U, [1.0, 1.0], 0.25, 1.0, 4, 6, 0, reg_coeffs={},
                             control_map=cmap.linear([[1.0, 0.0], [1.0, 0.0], [1.0, 0.0]]))


def test_dump_inputs_writes_the_map_only_when_given(monkeypatch):
    from quantum_optimal_control.helper_functions import data_management
    from quantum_optimal_control.main_grape.grape import _dump_inputs
    written = {}

    class Recorder(object):                                 # (h5py is optional: what _dump_inputs adds is recorded instead of written)
        def __init__(self, path):
            self.keys = written.setdefault(path, {})

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def add(self, key, data=None):
            self.keys[key] = data

        def create_group(self, name):
            return self

        def create_dataset(self, key, data=None):
            self.keys[key] = data

    monkeypatch.setattr(data_management, 'H5File', Recorder)
    H0, Hops, names, U = _qubits()
    conv = {'rate': 0.01, 'max_iterations': 1}
    args = (H0, Hops, names, U, 1.0, 4, [0, 1], True, False, False, False, [1.0, 1.0], None, 'Adam', conv, {}, None)
    _dump_inputs('plain', *args)
    cm = cmap.combine(cmap.linear(np.ones((3, 2))), cmap.fixed(np.ones((3, 4))))
    _dump_inputs('mapped', *args, control_map=cm)
    assert not [key for key in written['plain'] if key.startswith('control_map')]
    assert sorted(key for key in written['mapped'] if key.startswith('control_map')) == ['control_map_alpha', 'control_map_fixed']
    assert np.array_equal(written['mapped']['control_map_alpha'], cm.alpha) and np.array_equal(written['mapped']['control_map_fixed'], cm.fixed)
    assert set(written['mapped']) - set(written['plain']) == {'control_map_alpha', 'control_map_fixed'}
