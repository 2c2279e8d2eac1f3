"""Open-system ensembles and fleets without a GPU: the new keys and attributes of helper_functions/robust.py and fleet.py, the Taylor rule over the
members, the composed reference of tests/open_fleet_reference.py against tests/lindblad_reference.py, against scipy's exponential of a member's dense
Liouvillian and against central differences of its own loss, and every refusal of the Python layer before the library is loaded."""
import numpy as np
import pytest
from scipy.linalg import expm

from oracle import grape_oracle as go
from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import fleet as fl_mod
from quantum_optimal_control.helper_functions import open_system
from quantum_optimal_control.helper_functions import robust as rb
from quantum_optimal_control.helper_functions.synthetic_systems import herm
from quantum_optimal_control.main_grape import grape as grape_mod
from tests import lindblad_reference as lr
from tests import open_fleet_reference as ofr
from tests.test_open_system import G_RTOL, S_RTOL, collapse_list

SZ = np.diag([1.0, -1.0]).astype(complex)
SX = np.array([[0, 1], [1, 0]], dtype=complex)
OPS2 = [open_system.relaxation(2, 10.0), open_system.dephasing(2, 20.0)]


class LibraryTouched(Exception):
    pass


@pytest.fixture
def no_library(monkeypatch):
    def touched():
        raise LibraryTouched()
    monkeypatch.setattr(hip_engine, 'load_library', touched)


# ---- the robust dict ------------------------------------------------------------------------------------------------------------------------

def test_validate_keeps_todays_keys_without_decay():
    ens = rb.validate(dict(operators=[SZ], offsets=[[0.0], [0.1]]), 2, 1)
    assert sorted(ens) == ['amp_scales', 'offsets', 'operators', 'risk', 'weights']
    assert not rb.has_decay(ens) and rb.member_collapse_ops(ens, 1) == []
    grid = rb.ensemble_grid([SZ], offsets=[[-0.1], [0.0], [0.1]], amp_scales=[0.9, 1.0], k=1)
    assert sorted(grid) == ['amp_scales', 'offsets', 'operators', 'risk', 'weights'] and grid['amp_scales'].shape == (6, 1)


def test_validate_normalises_the_decay_keys():
    ens = rb.validate(dict(amp_scales=[[1.0], [0.9]], collapse_ops=OPS2), 2, 1)
    assert sorted(ens) == ['amp_scales', 'collapse_ops', 'offsets', 'operators', 'rate_scales', 'risk', 'weights']
    assert np.array_equal(ens['rate_scales'], np.ones((2, 2))) and ens['collapse_ops'][0].dtype == np.complex128
    ens = rb.validate(dict(collapse_ops=OPS2, rate_scales=[[1.0, 0.0], [4.0, 0.25]]), 2, 1)        # (the members from the scales alone)
    assert ens['amp_scales'].shape == (2, 1) and rb.has_decay(ens)
    got = rb.member_collapse_ops(ens, 1)
    assert len(got) == 2 and np.allclose(got[0], 2.0 * OPS2[0]) and np.allclose(got[1], 0.5 * OPS2[1])
    assert len(rb.member_collapse_ops(ens, 0)) == 1                                                   # a scale of 0 switches the channel off
    empty = rb.validate(dict(amp_scales=[[1.0]], collapse_ops=[]), 2, 1)                           # the closed limit, still an open problem
    assert rb.has_decay(empty) and empty['rate_scales'].shape == (1, 0)


@pytest.mark.parametrize('bad, msg', [
    (dict(amp_scales=[[1.0]], rate_scales=[[1.0]]), 'rate_scales given without collapse_ops'),
    (dict(amp_scales=[[1.0]], collapse_ops=OPS2, rate_scales=[[1.0]]), r'rate_scales have shape \(1, 1\), expected \(1, 2\)'),
    (dict(amp_scales=[[1.0], [1.0]], collapse_ops=OPS2, rate_scales=[[1.0, 1.0]]), 'amp_scales have shape'),
    (dict(amp_scales=[[1.0]], collapse_ops=OPS2, rate_scales=[[1.0, -0.5]]), 'finite and >= 0'),
    (dict(amp_scales=[[1.0]], collapse_ops=OPS2, rate_scales=[[1.0, np.inf]]), 'finite and >= 0'),
    (dict(amp_scales=[[1.0]], collapse_ops=[np.eye(3)]), 'shape'),
    (dict(amp_scales=[[1.0]], collapse_ops=np.eye(2)), 'a list'),
    (dict(amp_scales=[[1.0]], collapse_ops=[np.zeros((2, 2))]), 'all zero')])
def test_validate_refuses(bad, msg):
    with pytest.raises(ValueError, match=msg):
        rb.validate(bad, 2, 1)


def test_ensemble_grid_takes_rate_rows_as_a_third_axis():
    grid = rb.ensemble_grid([SZ], offsets=[[-0.1], [0.0]], amp_scales=[0.9, 1.0], k=1, collapse_ops=OPS2, rate_scales=[[0.5, 2.0], 1.0, [3.0, 0.0]])
    assert grid['offsets'].shape == (12, 1) and grid['amp_scales'].shape == (12, 1) and grid['rate_scales'].shape == (12, 2)
    assert grid['offsets'][0, 0] == 0.0 and grid['amp_scales'][0, 0] == 1.0 and np.array_equal(grid['rate_scales'][0], [1.0, 1.0])      # nominal first
    rows = {(o[0], a[0]) + tuple(r) for o, a, r in zip(grid['offsets'], grid['amp_scales'], grid['rate_scales'])}
    assert len(rows) == 12 and (-0.1, 0.9, 3.0, 0.0) in rows
    assert np.allclose(grid['weights'], 1.0 / 12)
    only = rb.ensemble_grid(k=1, collapse_ops=OPS2)
    assert only['rate_scales'].shape == (1, 2)
    with pytest.raises(ValueError, match='rate_scales given without collapse_ops'):
        rb.ensemble_grid(k=1, rate_scales=[1.0])
    with pytest.raises(ValueError, match='a row has 3 entries, expected 2'):
        rb.ensemble_grid(k=1, collapse_ops=OPS2, rate_scales=[[1.0, 2.0, 3.0]])


# ---- the fleet ------------------------------------------------------------------------------------------------------------------------------

def test_devices_and_around_carry_the_decay():
    fl = fl_mod.devices([SZ], offsets=[[0.0], [0.1], [0.2]], k=1, collapse_ops=OPS2, rate_scales=[[1.0, 1.0], [2.0, 0.5], [0.0, 3.0]])
    assert fl.has_decay and fl.rate_scales.shape == (3, 1, 2) and len(fl.collapse_ops) == 2
    dev = fl.device(2)
    assert np.array_equal(dev['rate_scales'], [[0.0, 3.0]]) and len(dev['collapse_ops']) == 2 and rb.has_decay(rb.validate(dev, 2, 1))
    plain = fl_mod.devices([SZ], offsets=[[0.0], [0.1]], k=1)
    assert not plain.has_decay and plain.rate_scales is None and sorted(plain.device(0)) == ['amp_scales', 'offsets', 'operators', 'risk', 'weights']
    ones = fl_mod.devices([SZ], offsets=[[0.0], [0.1]], k=1, collapse_ops=OPS2)
    assert np.array_equal(ones.rate_scales, np.ones((2, 1, 2)))
    ens = rb.ensemble_grid([SZ], offsets=[[0.0], [0.05]], k=1, collapse_ops=OPS2, rate_scales=[1.0, [2.0, 4.0]])
    ar = fl_mod.around([SZ], offsets=[[0.0], [0.1], [0.2]], robust=ens, k=1, collapse_ops=OPS2, rate_scales=[[1.0, 1.0], [2.0, 0.5], [0.0, 3.0]])
    assert ar.rate_scales.shape == (3, 4, 2) and ar.n_members == 4
    for f in range(3):
        for e in range(4):
            assert np.array_equal(ar.rate_scales[f, e], fl.rate_scales[f, 0] * ens['rate_scales'][e])
            assert ar.offsets[f, e, 0] == fl.offsets[f, 0, 0] + ens['offsets'][e, 0]
    from_ens = fl_mod.around([SZ], offsets=[[0.0], [0.1]], robust=ens, k=1)                          # the ensemble's decay alone
    assert from_ens.has_decay and np.array_equal(from_ens.rate_scales[1], ens['rate_scales'])
    closed_ens = rb.ensemble_grid([SZ], offsets=[[0.0], [0.05]], k=1)
    from_fleet = fl_mod.around([SZ], offsets=[[0.0], [0.1]], robust=closed_ens, k=1, collapse_ops=OPS2, rate_scales=[[1.0, 2.0], [3.0, 4.0]])
    assert np.array_equal(from_fleet.rate_scales[1], [[3.0, 4.0], [3.0, 4.0]])


@pytest.mark.parametrize('make, msg', [
    (lambda: fl_mod.devices([SZ], offsets=[[0.0], [0.1]], k=1, rate_scales=[[1.0], [1.0]]), 'rate_scales given without collapse_ops'),
    (lambda: fl_mod.devices([SZ], offsets=[[0.0], [0.1]], k=1, collapse_ops=OPS2, rate_scales=[[1.0, 1.0]]), r'rate_scales have shape \(1, 2\), expected \(2, 2\)'),
    (lambda: fl_mod.devices([SZ], offsets=[[0.0], [0.1]], k=1, collapse_ops=OPS2, rate_scales=[[1.0, 1.0], [1.0, -1.0]]), 'finite and >= 0'),
    (lambda: fl_mod.devices([SZ], offsets=[[0.0]], k=1, collapse_ops=[np.eye(3)]), 'shape'),
    (lambda: fl_mod.validate(fl_mod.Fleet([], np.zeros((2, 1, 0)), np.ones((2, 1, 1)), collapse_ops=OPS2, rate_scales=np.ones((2, 2, 2))), 2, 1),
     r'rate_scales have shape \(2, 2, 2\), expected \(2, 1, 2\)'),
    (lambda: fl_mod.Fleet([], np.zeros((2, 1, 0)), np.ones((2, 1, 1)), rate_scales=np.ones((2, 1, 2))), 'rate_scales given without collapse_ops'),
    (lambda: fl_mod.around([SZ], offsets=[[0.0]], k=1, collapse_ops=OPS2[:1], robust=rb.ensemble_grid([SZ], offsets=[[0.0]], k=1, collapse_ops=OPS2)),
     'the same collapse operators')])
def test_fleet_refuses(make, msg):
    with pytest.raises(ValueError, match=msg):
        make()


def test_decay_arrays_of_the_binding():
    ens = rb.validate(dict(amp_scales=[[1.0], [0.9]], collapse_ops=OPS2, rate_scales=[[1.0, 0.0], [4.0, 0.25]]), 2, 1)
    D, rates = hip_engine.decay_arrays(ens, None, 2, 2, 0.25)
    assert D.shape == (2, 2, 2) and np.allclose(D[0], 0.5 * OPS2[0]) and rates.shape == (1, 2, 2) and rates.flags.c_contiguous
    fl = fl_mod.devices([SZ], offsets=[[0.0], [0.1], [0.2]], k=1, collapse_ops=OPS2, rate_scales=[[1.0, 1.0], [2.0, 0.5], [0.0, 3.0]])
    D, rates = hip_engine.decay_arrays(fl.device(0), fl, 2, 1, 1.0)                                   # the fleet's table stands in front of device 0's
    assert rates.shape == (3, 1, 2) and np.array_equal(rates[2, 0], [0.0, 3.0])
    assert hip_engine.decay_arrays(rb.validate(dict(amp_scales=[[1.0]]), 2, 1), None, 2, 1, 1.0) is None
    with pytest.raises(ValueError, match='rate_scales have shape'):
        hip_engine.decay_arrays(dict(ens, rate_scales=np.ones((3, 2))), None, 2, 2, 1.0)
    with pytest.raises(ValueError, match='finite and >= 0'):
        hip_engine.decay_arrays(dict(ens, rate_scales=[[1.0, -1.0], [1.0, 1.0]]), None, 2, 2, 1.0)
    assert [f[0] for f in hip_engine.QocDecay._fields_] == ['n_collapse', 'C', 'rate_scales']
    assert [f[0] for f in hip_engine.QocOpen._fields_] == ['n_collapse', 'C']
    for name in ('qoc_create_open_fleet', 'qoc_get_member_final_density'):
        assert name in hip_engine.EXPORTED_SYMBOLS


# ---- the Taylor rule ------------------------------------------------------------------------------------------------------------------------

def test_taylor_rule_is_the_maximum_over_the_members():
    rng = np.random.default_rng(3)
    H0, Hops = herm(rng, 3), [0.5 * herm(rng, 3)]
    ops = collapse_list(3, 2, 1)
    ens = rb.validate(dict(operators=[herm(rng, 3)], offsets=[[0.0], [0.8]], amp_scales=[[1.0], [1.3]], collapse_ops=ops,
                           rate_scales=[[1.0, 1.0], [40.0, 0.0]]), 3, 1)
    each = []
    for e in range(2):
        H0e, Hopse = rb.member_hamiltonians(H0, Hops, ens, e)
        each.append(open_system.choose_taylor(H0e, Hopse, [1.0], rb.member_collapse_ops(ens, e), 0.3, 10, 1e-6))
    got = open_system.choose_taylor_members(H0, Hops, [1.0], [ens], 0.3, 10, 1e-6)
    assert got == (max(t for t, _ in each), max(s for _, s in each)) and each[0] != each[1]
    fl = fl_mod.validate(fl_mod.Fleet(ens['operators'], ens['offsets'][:, None, :], ens['amp_scales'][:, None, :], collapse_ops=ops,
                                      rate_scales=ens['rate_scales'][:, None, :]), 3, 1)
    assert open_system.choose_taylor_members(H0, Hops, [1.0], [fl.device(f) for f in range(2)], 0.3, 10, 1e-6) == got


# ---- the reference --------------------------------------------------------------------------------------------------------------------------

def _problem(**kw):
    return ofr.problem(3, 2, 6, 2, 2, **kw)


def test_reference_with_one_member_and_scales_of_one_is_the_lindblad_reference():
    p = _problem(regs={'dwdt': 0.05, 'amplitude': 0.1})
    ens = rb.validate(dict(amp_scales=np.ones((1, 2)), collapse_ops=p['collapse_ops']), 3, 2)
    np.random.seed(p['np_seed'])
    sp = go.OracleSystem(p['H0'], p['Hops'], p['U'], p['total_time'], p['steps'], p['states_concerned_list'], U0=p['U0'], reg_coeffs=p['reg_coeffs'],
                         maxA=p['maxA'], Taylor_terms=p['Taylor_terms'])
    x = ref_start(p)
    a, b = ofr.evaluate(p, None, ens, x), lr.evaluate(sp, p['collapse_ops'], x)
    for key in ('loss', 'reg_loss', 'unitary_scale', 'grad_squared'):
        print('%s: composed %.17g, lindblad_reference %.17g' % (key, a[key], b[key]))
        assert abs(a[key] - b[key]) <= S_RTOL * max(1.0, abs(b[key]))
    assert np.max(np.abs(a['grad'] - b['grad'])) <= G_RTOL * np.max(np.abs(b['grad']))
    assert np.max(np.abs(a['rho_final'] - b['rho_final'])) <= S_RTOL and np.max(np.abs(a['populations'] - b['populations'])) <= S_RTOL
    assert a['loss'] > 1e-3


def ref_start(p, seed=0):
    return np.random.default_rng(90 + seed).normal(0.0, 0.7, size=(len(p['maxA']), p['steps']))


def test_a_member_with_its_own_scales_against_the_dense_liouvillian():
    """Member 1 has the scales (2.5, 0): its propagation is expm of the Liouvillian built from sqrt(2.5) C_0 alone, with its own drift and amplitudes."""
    p = _problem(taylor=(14, 2))
    rng = np.random.default_rng(8)
    ens = rb.validate(dict(operators=[herm(rng, 3)], offsets=[[0.0], [0.3]], amp_scales=[[1.0, 1.0], [1.1, 0.9]], collapse_ops=p['collapse_ops'],
                           rate_scales=[[1.0, 1.0], [2.5, 0.0]]), 3, 2)
    x = ref_start(p)
    r = ofr.evaluate(p, None, ens, x, want_grad=False)
    H0e, _ = rb.member_hamiltonians(p['H0'], [], ens, 1)
    sp = ofr.member_system(p, H0e, np.ones(2))
    Ds = [np.sqrt(sp.dt) * np.sqrt(2.5) * np.asarray(p['collapse_ops'][0])]
    u = ens['amp_scales'][1][:, None] * r['pulse']
    psi = lr.start_vectors(sp)
    worst = 0.0
    for i in range(sp.m):
        for j in range(sp.m):
            v = np.outer(psi[:, i], np.conj(psi[:, j])).reshape(-1)
            for t in range(sp.steps):
                v = expm(lr.liouvillian(lr.generator(sp, Ds, u[:, t]), Ds)) @ v
            worst = max(worst, float(np.max(np.abs(v.reshape(sp.n, sp.n) - r['member_rho'][1, i, j]))))
    print('member 1: largest deviation from expm of its Liouvillian %.3e' % worst)
    assert worst <= 1e-12
    assert np.max(np.abs(r['member_rho'][0] - r['member_rho'][1])) > 1e-3 and abs(r['member_loss'][0] - r['member_loss'][1]) > 1e-3


def _gradient_error(steps, beta):
    p = ofr.problem(3, 1, steps, 1, 2, state_transfer=True, taylor=(14, 1), seed=2)
    p['total_time'] = 4.0
    rng = np.random.default_rng(11)
    ens = rb.validate(dict(operators=[herm(rng, 3)], offsets=[[0.0], [0.3]], amp_scales=[[1.0], [1.2]], weights=[0.4, 0.6], collapse_ops=p['collapse_ops'],
                           rate_scales=[[1.0, 1.0], [2.5, 0.0]], risk=beta), 3, 1)
    t = (np.arange(steps) + 0.5) / steps
    x = (0.7 * np.sin(2 * np.pi * t) + 0.3)[None, :]
    g = ofr.evaluate(p, None, ens, x)['grad']
    fd = ofr.ref.central_differences(lambda y: ofr.evaluate(p, None, ens, y, want_grad=False)['loss'], x)
    return float(np.linalg.norm(g - fd) / np.linalg.norm(fd))


@pytest.mark.parametrize('beta', [0.0, 20.0])
def test_gradient_against_central_differences_of_the_references_own_loss(beta):
    """The slope tests/test_open_system.py documents for one open problem holds for the weighted mean and the soft worst case of two: the first-order
    gradient's relative error against central differences falls by at least 1.7 for every halving of dt."""
    errs = [_gradient_error(s, beta) for s in (5, 10, 20, 40)]
    ratios = [errs[i] / errs[i + 1] for i in range(3)]
    print('relative gradient error at 5, 10, 20, 40 slices: %s; ratios %s' % (errs, ratios))
    assert all(q >= 1.7 for q in ratios), (errs, ratios)


def test_devices_of_the_reference_fleet_lie_apart():
    p = _problem()
    fl = ofr.make_fleet(p, 2, 3, 1)
    flat = np.concatenate([fl.rate_scales.reshape(-1), fl.amp_scales.reshape(-1), fl.offsets.reshape(-1)])
    assert len(set(flat)) == flat.size and np.count_nonzero(fl.rate_scales == 0.0) == 1
    x = ref_start(p)
    at = [ofr.evaluate_device(p, None, fl, f, x) for f in range(2)]
    assert ofr.swapped_apart([o['loss'] for o in at]) and ofr.swapped_apart([o['grad'] for o in at]) and ofr.swapped_apart([o['rho_final'].view(np.float64) for o in at])


# ---- refusals of the Python layer, before the library is loaded --------------------------------------------------------------------------------

def qubit_call(**kw):
    args = dict(H0=0.5 * SZ, Hops=[SX], Hnames=['x'], U=SX, total_time=4.0, steps=8, states_concerned_list=[0, 1], save=False, show_plots=False,
                reg_coeffs={}, maxA=[0.5])
    args.update(kw)
    return args


def decay_grid():
    return rb.ensemble_grid([SZ], offsets=[[0.0], [0.05]], k=1, collapse_ops=OPS2, rate_scales=[1.0, [2.0, 0.0]])


def decay_fleet():
    return fl_mod.devices([SZ], offsets=[[0.0], [0.1], [0.2]], k=1, collapse_ops=OPS2, rate_scales=[[1.0, 1.0], [2.0, 0.5], [0.0, 3.0]])


@pytest.mark.parametrize('kind', ['robust', 'fleet'])
def test_grape_refuses_before_the_library_loads(kind, no_library):
    import scipy.sparse as sps
    carrier = dict(robust=decay_grid()) if kind == 'robust' else dict(fleet=decay_fleet())
    refused = [(dict(exact_gradient=True), 'exact_gradient'), (dict(dressed_info={'is_dressed': False}), 'dressed_info'),
               (dict(reg_coeffs={'forbidden_coeff_list': [1.0], 'states_forbidden_list': [1]}), 'forbidden-level'),
               (dict(reg_coeffs={'speed_up': 1.0}), 'speed_up'), (dict(reg_coeffs={'forbid_dressed': True}), 'forbid_dressed'),
               (dict(time_comm=object()), 'time_comm'), (dict(plan_seeds=4), 'sharded'), (dict(_first_seed=1), 'sharded'),
               (dict(collapse_ops=[OPS2[0]]), 'collapse_ops')]
    for extra, msg in refused:
        with pytest.raises(ValueError, match=msg):
            grape_mod.Grape(**qubit_call(**dict(carrier, **extra)))
    with pytest.raises(ValueError):
        grape_mod.Grape(**qubit_call(H0=sps.csr_matrix(0.5 * SZ), state_transfer=True, U=[np.array([0, 1])], states_concerned_list=[np.array([1, 0])], **carrier))
    for entry, name in ((grape_mod.GrapeSharded, 'GrapeSharded'), (grape_mod.GrapeTimeSharded, 'GrapeTimeSharded')):
        with pytest.raises(ValueError, match=name):
            entry(**qubit_call(**carrier))
    if kind == 'fleet':
        with pytest.raises(ValueError, match="method='Adam', 'LBFGS' or 'EVOLVE'"):
            grape_mod.Grape(**qubit_call(method='L-BFGS-B', **carrier))
    for method in ('Adam', 'LBFGS', 'EVOLVE'):
        with pytest.raises(LibraryTouched):                                                        # ... and what is allowed reaches the library
            grape_mod.Grape(**qubit_call(method=method, **carrier))


def test_hip_engine_refuses_before_the_library_loads(no_library):
    def make(**kw):
        args = dict(Hs=np.zeros((2, 2, 2)), U0=np.eye(2), V=np.eye(2), W=np.eye(2), maxA=[0.1], dt=1.0, total_time=4.0, steps=4, taylor_terms=5, scaling=1,
                    reg_coeffs={}, n_seeds=3)
        args.update(kw)
        return hip_engine.HipEngine(**args)
    for carrier in (dict(ensemble=decay_grid()), dict(fleet=decay_fleet())):
        with pytest.raises(LibraryTouched):
            make(**carrier)
        for extra, msg in ((dict(collapse_ops=[OPS2[0]]), 'collapse_ops= keyword'), (dict(exact_gradient=True), 'exact_gradient'),
                           (dict(time_shards=2), 'time sharding'), (dict(time_comm=object()), 'time sharding')):
            with pytest.raises(ValueError, match='with decay does not combine with .*%s' % msg):
                make(**dict(carrier, **extra))
    with pytest.raises(ValueError, match='rate_scales have shape'):
        make(ensemble=dict(decay_grid(), rate_scales=np.ones((2, 3))))
    with pytest.raises(ValueError, match='rate_scales given without collapse_ops'):
        make(ensemble=dict(amp_scales=np.ones((1, 1)), weights=np.ones(1), rate_scales=np.ones((1, 1))))


def test_the_pinned_refusals_of_the_keyword_still_raise(no_library):
    plain = rb.ensemble_grid([SZ], offsets=[[0.0], [0.05]], k=1)
    ops = [open_system.relaxation(2, 10.0)]
    with pytest.raises(ValueError, match='collapse_ops \\(open-system GRAPE\\) does not combine with robust'):
        grape_mod.Grape(**qubit_call(robust=plain, collapse_ops=ops))
    with pytest.raises(ValueError, match='collapse_ops \\(open-system GRAPE\\) does not combine with transfer'):
        grape_mod.Grape(**qubit_call(transfer=np.eye(8), collapse_ops=ops))
    with pytest.raises(ValueError, match='fleet does not combine with collapse_ops'):
        grape_mod.Grape(**qubit_call(fleet=fl_mod.devices([SZ], offsets=[[0.0], [0.1]], k=1), collapse_ops=ops))
    from quantum_optimal_control.helper_functions import control_map as cmap
    with pytest.raises(ValueError, match='control_map does not combine with collapse_ops'):
        grape_mod.Grape(**qubit_call(control_map=cmap.identity(1), collapse_ops=ops))
    with pytest.raises(ValueError, match='collapse_ops \\(open-system GRAPE\\) does not combine with ensemble'):
        hip_engine.HipEngine(np.zeros((2, 2, 2)), np.eye(2), np.eye(2), np.eye(2), [1.0], 0.25, 1.0, 4, 6, 0, reg_coeffs={}, collapse_ops=ops,
                             ensemble=dict(amp_scales=[[1.0]], weights=[1.0]))


# ---- the run log -----------------------------------------------------------------------------------------------------------------------------

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


@pytest.mark.parametrize('kind', ['robust', 'fleet'])
def test_save_logs_the_decay_of_the_members(kind, no_library, monkeypatch, tmp_path):
    """save=True writes the inputs before anything is built: the log of a call with decay holds the collapse operators and the rate scales of the
    robust dict (a fleet call: of the fleet as well); the log of the same call without decay holds neither."""
    from quantum_optimal_control.helper_functions import data_management
    monkeypatch.setattr(data_management, 'H5File', RecordingLog)
    plain = rb.ensemble_grid([SZ], offsets=[[0.0], [0.05]], k=1) if kind == 'robust' else fl_mod.devices([SZ], offsets=[[0.0], [0.1], [0.2]], k=1)
    carrier = decay_grid() if kind == 'robust' else decay_fleet()
    keys = [kind + '_collapse_ops', kind + '_rate_scales']
    for given, has in ((plain, False), (carrier, True)):
        RecordingLog.seen = {}
        with pytest.raises(LibraryTouched):
            grape_mod.Grape(**qubit_call(save=True, file_name='decay', data_path=str(tmp_path), convergence={'max_iterations': 2}, **{kind: given}))
        assert kind + '_offsets' in RecordingLog.seen and [key in RecordingLog.seen for key in keys] == [has, has], sorted(RecordingLog.seen)
    ops, scales = RecordingLog.seen[keys[0]], RecordingLog.seen[keys[1]]
    assert ops.shape == (2, 2, 2) and ops.dtype == np.complex128 and np.array_equal(ops, np.array(OPS2))
    if kind == 'robust':
        assert scales.shape == (4, 2) and np.array_equal(scales, carrier['rate_scales']) and sorted(map(tuple, scales)) == [(1, 1), (1, 1), (2, 0), (2, 0)]
    else:
        assert scales.shape == (3, 1, 2) and np.array_equal(scales[:, 0], [[1.0, 1.0], [2.0, 0.5], [0.0, 3.0]])
