"""Sparse ensembles, fleets, lines and maps on the GPU (qoc_create_sparse_fleet): the merged rows against the per-operator kernels under
np.array_equal on the smallest shapes at which a row walk can go wrong; the nominal engine against qoc_create_sparse bit for bit; parity with the composed
sparse reference of tests/sparse_ensemble_reference.py; frozen rows; the device loops against a dense ensemble engine; determinism; what the C ABI
refuses; create / destroy cycles; the example.  (A line on sparse operators is reached through the C entry point alone: line_engine below.)"""
import contextlib
import ctypes as C
import functools
import io
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sps

from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import fleet as fl_mod
from quantum_optimal_control.helper_functions import robust as rb
from tests import control_map_reference as ref
from tests import sparse_ensemble_reference as ser
from tests import sparse_reference as sr
from tests.test_adam_tail import LOOP_ATOL, _choose_target
from tests.test_hip_parity import G_RTOL, S_RTOL, U_ATOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
P = hip_engine


def make_ensemble(p, E, q, seed=5, zero_weight=False, sparse=True):
    """E members over q random sparse Hermitian perturbations: offsets in +-0.2, scales in 0.9 .. 1.1, random weights (validated: they sum to 1)."""
    rng = np.random.default_rng(seed)
    ops = [0.5 * sr.random_sparse(rng, p.n, (1, 3)) for _ in range(q)]
    w = rng.uniform(0.5, 1.5, size=E)
    if zero_weight:
        w[1] = 0.0
    ens = dict(operators=ops if sparse else [o.toarray() for o in ops], offsets=rng.uniform(-0.2, 0.2, size=(E, q)),
               amp_scales=rng.uniform(0.9, 1.1, size=(E, p.k)), weights=w)
    return rb.validate(ens, p.n, p.k, sparse=sparse)


def line_engine(p, n_seeds, ensemble, T, control_map=None, row_layout=0):
    """A line on sparse operators is served by the C entry point alone (HipEngine keeps refusing transfer= beside sparse_ops): the engine is created
    through ctypes and handed to a HipEngine object for its read-backs.  Problems without regularisers only."""
    assert not p.reg_coeffs
    lib = P.load_library()
    ops = p.engine_ops() + P.sparse_perturbations(ensemble, p.dt)
    n, indptr, row, col, val = P.sparse_arrays(ops)
    cfg = P.QocConfig()
    cfg.n, cfg.k, cfg.steps, cfg.m, cfg.taylor_terms, cfg.scaling, cfg.state_transfer, cfg.n_seeds = p.n, p.k, p.steps, p.m, p.T, 0, 1, n_seeds
    cfg.dt, cfg.total_time = p.dt, p.total_time
    s = P.QocSparse()
    s.indptr, s.row, s.col = indptr.ctypes.data_as(C.POINTER(C.c_int64)), row.ctypes.data_as(P._IP), col.ctypes.data_as(P._IP)
    s.val, s.vector_home = P._dp(val.view(np.float64)), 0
    pl = P.QocSparsePlan()
    pl.row_layout = row_layout
    keep = [np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in (T, p.maxA)]
    e = None
    if ensemble is not None:
        _, off, amp, wt = P.ensemble_arrays(ensemble, n, p.k, p.dt, dense=False)
        keep += [off, amp, wt]
        e = P.QocEnsemble()
        e.members, e.n_perturb, e.P, e.offsets, e.amp_scales, e.weights = amp.shape[0], off.shape[1], None, (P._dp(off) if off.shape[1] else None), P._dp(amp), P._dp(wt)
    t = P.QocTransfer()
    t.n_samples, t.T = keep[0].shape[1], P._dp(keep[0])
    m = None
    if control_map is not None:
        m = P.QocControlMap()
        m.n_terms, m.degree = control_map.n_terms, control_map.degree
        m.poly, m.mix, m.fixed = P._dp(control_map.alpha), P._dp(control_map.mix), P._dp(control_map.fixed)
    Vc, Wc = np.ascontiguousarray(p.V), np.ascontiguousarray(p.W)
    eng = P.HipEngine.__new__(P.HipEngine)
    eng._lib, eng._h = lib, C.c_void_p()
    P._check(lib.qoc_create_sparse_fleet(C.byref(cfg), C.byref(s), C.byref(pl), None if e is None else C.byref(e), None, C.byref(t), None if m is None else C.byref(m),
                                         P._dp(Vc.view(np.float64)), P._dp(Wc.view(np.float64)), P._dp(keep[1]), None, None, None, C.byref(eng._h)))
    eng.n, eng.k, eng.m, eng.steps, eng.n_seeds, eng.samples = p.n, p.k, p.m, p.steps, n_seeds, int(t.n_samples)
    eng.terms = p.k if control_map is None else control_map.n_terms
    eng.members, eng.devices, eng.risk, eng.state_transfer = (1 if e is None else int(e.members)), 0, 0.0, True
    if ensemble is not None and float(ensemble.get('risk', 0.0)) > 0:
        eng.set_risk(ensemble['risk'])
    buf = C.create_string_buffer(1024)
    P._check(lib.qoc_plan_describe(eng._h, buf, 1024))
    eng.plan = dict(kv.split('=', 1) for kv in buf.value.decode().split())
    return eng


def make_engine(p, n_seeds=1, ensemble=None, **kw):
    if kw.get('transfer') is not None:
        return line_engine(p, n_seeds, ensemble, kw['transfer'], kw.get('control_map'), P.ROW_LAYOUT[kw.get('row_layout') or 0])
    omg = None
    if 'envelope' in p.reg_coeffs:
        grid = np.linspace(-2, 2, p.steps)
        shape = np.ones(p.steps) - np.exp(-np.power(grid, 2.) / 2.)
        omg = np.tile(shape * (shape > 0) + 0.01 * np.ones(p.steps), (p.k, 1))
    return P.HipEngine(None, None, p.V, p.W, p.maxA, p.dt, p.total_time, p.steps, p.T, 0, state_transfer=True, reg_coeffs=p.reg_coeffs, one_minus_gauss=omg,
                       n_seeds=n_seeds, sparse_ops=p.engine_ops(), ensemble=ensemble, **kw)


def make_dense_engine(p, n_seeds, ensemble):
    Hs = np.stack([o.toarray() for o in p.engine_ops()])
    dense = dict(ensemble, operators=[o.toarray() for o in ensemble['operators']])
    return P.HipEngine(Hs, None, p.V, p.W, p.maxA, p.dt, p.total_time, p.steps, p.T, 0, state_transfer=True, reg_coeffs=p.reg_coeffs, n_seeds=n_seeds,
                       ensemble=dense)


def bases(p, G, width=None, seed=0):
    return np.random.default_rng(900 + seed).normal(0.0, 0.6, size=(G, p.k, p.steps if width is None else width))


# ---- 1. merged rows against the per-operator kernels: equal, not close -------------------------------------------------------------------------------

def _custom(kind):
    """Problems whose rows differ in which operators they hold."""
    sp = sr.sparse_case(20, 4, k=3, m=1, T=8, seed=70)
    H0, Hops = sp.H0_in.tolil(), [h.tolil() for h in sp.Hops_in]
    if kind == 'absent':                                 # control 0 lives in the upper half of the rows only, control 2 in rows 3 .. 6
        Hops[0][10:, :] = 0
        Hops[2][:3, :] = 0
        Hops[2][7:, :] = 0
    else:                                                # rows 4 and 17 have no entry in any operator
        for op in [H0] + Hops:
            op[4, :] = 0
            op[17, :] = 0
    mats = [sps.csr_matrix(op) for op in [H0] + Hops]
    for a in mats:
        a.eliminate_zeros()
    return ser.Problem(mats[0], mats[1:], sp.V, sp.W, sp.total_time, sp.steps, sp.exp_terms, sp.maxA, {'dwdt': 0.02})


LAYOUT_ROWS = {
    'n1': dict(n=1, steps=3),
    'n5': dict(n=5, steps=4),
    'n33': dict(n=33, steps=5, forbidden=True, reg_coeffs={'speed_up': 0.4, 'dwdt': 0.02}),
    'n257': dict(n=257, steps=3),                        # more rows than a 256-thread workgroup
    'n1025': dict(n=1025, steps=2),                      # more rows than 1024 threads: a thread walks two rows per term
    'dense_n8': dict(n=8, steps=4, kind='dense'),
    'width_0': dict(n=20, steps=4, kind='zero_control'),
    'absent': 'absent',
    'empty_rows': 'empty_rows',
    'T1': dict(n=12, steps=4, T=1),
    'T20': dict(n=12, steps=3, T=20),
    'm3': dict(n=12, steps=5, m=3),
}


@functools.lru_cache(maxsize=None)
def layout_problem(name):
    row = LAYOUT_ROWS[name]
    if isinstance(row, str):
        return _custom(row)
    return ser.from_sparse_case(sr.sparse_case(seed=200 + list(LAYOUT_ROWS).index(name), **row))


def run_layout(p, ens, layout, G=2, x=None, **kw):
    """Everything a layout can change: an evaluation's outputs, the members' scalars, and the state after 5 device Adam iterations."""
    eng = make_engine(p, G, ensemble=ens, row_layout=layout, **kw)
    try:
        plan = dict(eng.plan)
        eng.set_base(bases(p, G) if x is None else x)
        r = eng.evaluate()
        out = dict(r, inter=eng.get_inter_vecs(), member=eng.member_scalars())
        eng.iterate(eng.adam_params(rate=0.05, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=100, poll_every=1), 5)
        out.update(base5=eng.get_base(), scalars5=eng.scalars(), inter5=eng.get_inter_vecs())
    finally:
        eng.close()
    return plan, out


def assert_layouts_equal(a, b):
    for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale', 'grad', 'inter', 'base5', 'inter5'):
        assert np.array_equal(a[key], b[key]), key
    for key in ('loss', 'reg_state'):
        assert np.array_equal(a['member'][key], b['member'][key]), key
    for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale', 'iterations'):
        assert np.array_equal(a['scalars5'][key], b['scalars5'][key]), key


@pytest.mark.parametrize('home', ['lds', 'global'])
@pytest.mark.parametrize('name', list(LAYOUT_ROWS))
def test_merged_rows_equal_the_per_operator_kernels(name, home):
    p = layout_problem(name)
    ens = make_ensemble(p, 2, 1, seed=list(LAYOUT_ROWS).index(name))
    plan1, per_op = run_layout(p, ens, 1, vector_home=home)
    plan2, merged = run_layout(p, ens, 2, vector_home=home)
    K = p.k + 1 + 1
    tab = (8 * K + 15) // 16 * 16
    assert (plan1['rows'], plan1['merged_width']) == ('per_operator', '0') and plan2['rows'] == 'merged', (plan1, plan2)
    assert plan1['vector_home'] == plan2['vector_home'] == home
    assert int(plan1['lds']) == (2 * p.n * 16 if home == 'lds' else 0) and int(plan2['lds']) == (2 * p.n * 16 if home == 'lds' else 0) + tab, (plan1, plan2)
    mats = p.engine_ops() + P.sparse_perturbations(ens, p.dt)
    assert int(plan2['merged_width']) == int(np.max(sum(np.diff(a.indptr) for a in mats)))
    assert (plan2['members'], plan2['perturbations']) == ('2', '1')
    assert np.all(np.isfinite(per_op['grad'])) and (name in ('n1', 'T1') or np.max(np.abs(per_op['grad'])) > 1e-6)
    assert_layouts_equal(per_op, merged)


def test_merged_rows_with_255_operators():
    """k' + 1 = 255: 252 controls, 2 perturbations and the drift -- the most the packed operator index holds."""
    rng = np.random.default_rng(31)
    n, k, steps = 12, 252, 2
    mk = lambda: 0.05 * sr.random_sparse(rng, n, (0, 2))
    V, W = sr.unit_columns(rng, n, 1), sr.unit_columns(rng, n, 1)
    p = ser.Problem(sr.random_sparse(rng, n), [mk() for _ in range(k)], V, W, 0.3, steps, 6, np.ones(k), {})
    ens = make_ensemble(p, 2, 2)
    plan1, per_op = run_layout(p, ens, 1, G=1)
    plan2, merged = run_layout(p, ens, 2, G=1)
    assert plan2['rows'] == 'merged' and int(plan2['lds']) == 2 * n * 16 + 2048 and plan2['perturbations'] == '2', plan2
    assert np.max(np.abs(per_op['grad'])) > 1e-6
    assert_layouts_equal(per_op, merged)
    want = ser.evaluate(p, ens, bases(p, 1)[0])
    assert abs(merged['loss'][0] - want['loss']) <= S_RTOL and np.max(np.abs(merged['grad'][0] - want['grad'])) <= G_RTOL * max(np.max(np.abs(want['grad'])), 1e-3)
    more = ser.Problem(p.H0, p.Hops + [mk()], V, W, 0.3, steps, 6, np.ones(k + 1), {})
    with pytest.raises(P.QocError, match='at most 255'):
        make_engine(more, 1, ensemble=make_ensemble(more, 2, 2), row_layout=2)


@functools.lru_cache(maxsize=None)
def boundary_problem(n):
    return ser.from_sparse_case(sr.sparse_case(n, 2, k=2, m=1, T=3, seed=50))


@pytest.mark.parametrize('n,home', [(5087, 'lds'), (5088, 'global')])
def test_the_boundary_of_the_merged_home_rule(n, home):
    """2 n 16 B + 32 B of coefficients (3 operators) <= 159 KiB: n = 5087 is the last merged size in LDS; a per-operator engine of n = 5088 still is."""
    p = boundary_problem(n)
    x = bases(p, 1)
    plan1, per_op = run_layout(p, None, 1, G=1, x=x)
    plan2, merged = run_layout(p, None, 2, G=1, x=x)
    assert plan1['vector_home'] == 'lds' and int(plan1['lds']) == 2 * n * 16, plan1
    assert plan2['vector_home'] == home and int(plan2['lds']) == (2 * n * 16 + 32 if home == 'lds' else 32), plan2
    assert_layouts_equal(per_op, merged)
    if home == 'global':
        with pytest.raises(P.QocError, match='n <= 5087|at most 5087'):
            make_engine(p, 1, row_layout=2, vector_home='lds')


def test_what_auto_resolves_to():
    """row_layout = 0: merged where profiles/sparse_ensemble.txt has it ahead (n >= 1024 with 12 or more operators), per-operator everywhere else."""
    rng = np.random.default_rng(12)

    def plan_of(n, q, layout):
        mk = lambda: sps.diags(rng.normal(size=n).astype(np.complex128), format='csr')
        p = ser.Problem(mk(), [mk(), mk()], sr.unit_columns(rng, n, 1), sr.unit_columns(rng, n, 1), 0.1, 1, 3, [1.0, 1.0], {})
        ens = rb.validate(dict(operators=[mk() for _ in range(q)], offsets=np.zeros((1, q)), amp_scales=np.ones((1, 2))), n, 2, sparse=True)
        eng = make_engine(p, 1, ensemble=ens, row_layout=layout)
        try:
            return eng.plan['rows']
        finally:
            eng.close()
    assert plan_of(1024, 9, 0) == 'merged' and plan_of(1024, 9, 'auto') == 'merged'
    assert plan_of(1024, 8, 0) == 'per_operator' and plan_of(1023, 9, 0) == 'per_operator' and plan_of(33, 12, 0) == 'per_operator'
    assert plan_of(1024, 9, 1) == 'per_operator' and plan_of(33, 0, 2) == 'merged'


# ---- 2. the nominal engine is the engine of qoc_create_sparse, bit for bit ----------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['n33', 'm3'])
def test_nominal_engine_is_the_plain_sparse_engine_bit_for_bit(name):
    p = layout_problem(name)
    x = bases(p, 3)
    out = {}
    for kind, kw in (('plain', {}), ('entry', dict(row_layout=1))):
        eng = make_engine(p, 3, **kw)
        try:
            assert ('rows' in eng.plan) == (kind == 'entry'), eng.plan
            if kind == 'entry':
                assert (eng.plan['members'], eng.plan['perturbations'], eng.plan['rows']) == ('1', '0', 'per_operator')
            eng.set_base(x)
            r = eng.evaluate()
            first = dict(r, inter=eng.get_inter_vecs(), uks=eng.get_uks(evaluated=True))
            its = eng.run_adam(eng.adam_params(rate=0.05, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=6, poll_every=4))
            out[kind] = dict(first, its=its, base=eng.get_base(), after=eng.scalars(), inter_after=eng.get_inter_vecs())
        finally:
            eng.close()
    a, b = out['plain'], out['entry']
    for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale', 'grad', 'inter', 'uks', 'its', 'base', 'inter_after'):
        assert np.array_equal(a[key], b[key]), key
    for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale', 'iterations', 'done'):
        assert np.array_equal(a['after'][key], b['after'][key]), key


# ---- 3. parity with the composed sparse reference -------------------------------------------------------------------------------------------------------

def parity_problem(reg=None, forbidden=False, n=16, steps=8, k=2, r=None, m=2):
    sp = sr.sparse_case(n, steps, k=k if r is None else r, m=m, T=8, seed=300 + n, reg_coeffs=reg, forbidden=forbidden)
    p = ser.from_sparse_case(sp)
    if r is not None:
        p = ser.Problem(p.H0, p.Hops, p.V, p.W, p.total_time, p.steps, p.T, [1.0 + 0.25 * i for i in range(k)], p.reg_coeffs)
    return p


def line(steps, samples, seed=4):
    """A response with a finite memory: every sample reaches a window of slices."""
    rng = np.random.default_rng(seed)
    T = np.zeros((steps, samples))
    for t in range(steps):
        s = min(samples - 1, t * samples // steps)
        T[t, s] = 0.7 + 0.2 * rng.uniform()
        if s > 0:
            T[t, s - 1] = 0.3 * rng.uniform()
    return T


PARITY = {
    'ensemble': dict(E=3, q=2),
    'zero_weight': dict(E=3, q=2, zero_weight=True),
    'risk': dict(E=3, q=2, beta=4.0),
    'line': dict(E=2, q=1, samples=4),
    'map': dict(E=1, q=0, map=dict(r=3, D=3)),
    'line_map_ensemble': dict(E=2, q=1, samples=4, map=dict(r=3, D=3)),
    'all_regularisers': dict(E=2, q=1, reg=sr.ALL_REGS, forbidden=True, n=24, steps=16),
}


def assert_parity(tag, eng, x, wants):
    r = eng.evaluate()
    inter, member = eng.get_inter_vecs(), eng.member_scalars()
    for g, o in enumerate(wants):
        for key in ('loss', 'reg_loss', 'unitary_scale', 'grad_squared'):
            print('%s %s[%d]: engine %.17g reference %.17g' % (tag, key, g, r[key][g], o[key]))
            assert abs(r[key][g] - o[key]) <= S_RTOL * max(1.0, abs(o[key])), (tag, key, g)
        gmax, err = float(np.max(np.abs(o['grad']))), float(np.max(np.abs(r['grad'][g] - o['grad'])))
        print('%s grad[%d]: max error %.3e, largest entry %.3e' % (tag, g, err, gmax))
        assert gmax > 1e-3 and err <= G_RTOL * max(gmax, 1e-3), (tag, g, err, gmax)
        assert np.max(np.abs(inter[g] - o['inter_vecs'])) <= U_ATOL * max(1.0, np.max(np.abs(o['inter_vecs'])))
        assert np.max(np.abs(member['loss'][g] - o['member_loss'])) <= S_RTOL and np.max(np.abs(member['reg_state'][g] - o['member_reg_state'])) <= S_RTOL
        assert np.max(np.abs(eng.member_weights()[g] - o['weights'])) <= S_RTOL
    return r


@pytest.mark.parametrize('layout', [1, 2])
@pytest.mark.parametrize('G', [1, 3])
@pytest.mark.parametrize('name', list(PARITY))
def test_parity_with_the_composed_reference(name, G, layout):
    c = PARITY[name]
    mp = c.get('map')
    p = parity_problem(c.get('reg'), c.get('forbidden', False), n=c.get('n', 16), steps=c.get('steps', 8), r=mp['r'] if mp else None)
    ens = make_ensemble(p, c['E'], c['q'], zero_weight=c.get('zero_weight', False)) if (c['E'] > 1 or c['q']) else None
    cm = ref.make_map(p.k, mp['r'], mp['D'], p.steps, mix=True, fixed=True) if mp else None
    T = line(p.steps, c['samples']) if 'samples' in c else None
    if T is not None:
        p.reg_coeffs.pop('envelope', None)
    x = bases(p, G, None if T is None else T.shape[1])
    beta = c.get('beta', 0.0)
    wants = [ser.evaluate(p, ens if ens is not None else ser.nominal(p.k), x[g], cm=cm, T=T, beta=beta) for g in range(G)]
    eng = make_engine(p, G, ensemble=None if ens is None else dict(ens, risk=beta), transfer=T, control_map=cm, row_layout=layout)
    try:
        plan = eng.plan
        assert (plan['path'], plan['rows'], plan['gradient']) == ('sparse', 'merged' if layout == 2 else 'per_operator', 'first_order'), plan
        assert (int(plan['members']), int(plan['perturbations'])) == (c['E'], c['q']), plan
        assert len(plan['ell'].split(',')) == (mp['r'] if mp else p.k) + 1 + c['q']
        if mp:
            assert (plan['terms'], plan['degree']) == (str(mp['r']), str(mp['D']))
        if T is not None:
            assert plan['samples'] == str(T.shape[1])
        eng.set_base(x)
        assert_parity(name, eng, x, wants)
        assert eng.get_uks().shape == (G, p.k, x.shape[2])
        np.testing.assert_allclose(eng.get_uks(evaluated=True), np.stack([o['uks'] for o in wants]), rtol=0, atol=4e-15)
        if mp:
            np.testing.assert_allclose(eng.get_coefficients(), np.stack([o['coefficients'] for o in wants]), rtol=0, atol=U_ATOL)
        if T is not None:
            np.testing.assert_allclose(eng.get_pulse(), np.stack([o['pulse'] for o in wants]), rtol=0, atol=U_ATOL)
        with pytest.raises(P.QocError, match='no final unitary'):
            eng.get_final_unitary()
        with pytest.raises(P.QocError, match='no final unitary'):
            eng.member_final_unitary()
    finally:
        eng.close()


@pytest.mark.parametrize('layout', [1, 2])
def test_fleet_parity_with_the_composed_reference(layout):
    """F = 3 devices, R = 2 control sets each, E = 2 members around every device (fleet.around): control set g is device g // 2's ensemble."""
    p = parity_problem(reg={'dwdt': 0.02, 'speed_up': 0.3}, forbidden=True)
    rng = np.random.default_rng(8)
    ops = [0.5 * sr.random_sparse(rng, p.n, (1, 3))]
    around = rb.validate(dict(operators=ops, offsets=[[0.0], [0.15]], amp_scales=[[1.0, 1.0], [0.95, 1.05]], weights=[0.6, 0.4]), p.n, p.k, sparse=True)
    fl = fl_mod.around(ops, offsets=[[-0.2], [0.0], [0.2]], amp_scales=[[0.9, 1.0], [1.0, 1.0], [1.1, 0.95]], robust=around, k=p.k)
    assert sps.issparse(fl.operators[0]) and fl.offsets.shape == (3, 2, 1)
    x = bases(p, 6)
    wants = [ser.evaluate_fleet(p, fl, g // 2, x[g]) for g in range(6)]
    assert np.max(np.abs(wants[0]['grad'] - ser.evaluate_fleet(p, fl, 1, x[0])['grad'])) > 1e-4      # (the devices differ: rows cannot be swapped)
    eng = make_engine(p, 6, fleet=fl, row_layout=layout)
    try:
        assert (eng.plan['devices'], eng.plan['members'], eng.plan['perturbations']) == ('3', '2', '1') and eng.devices == 3, eng.plan
        eng.set_base(x)
        assert_parity('fleet', eng, x, wants)
    finally:
        eng.close()


# ---- 4. frozen rows, determinism, lifecycle ----------------------------------------------------------------------------------------------------------------

def test_frozen_rows_stay_out_of_the_variable():
    """The perturbations are frozen control rows of the trajectories: the variable, the gradient and get_uks keep k rows, and an offset of zero leaves
    the ensemble's values at the plain problem's -- the frozen rows contribute nothing but their offsets."""
    p = layout_problem('n33')
    ens = make_ensemble(p, 2, 2)
    zero = dict(ens, offsets=np.zeros((2, 2)), amp_scales=np.ones((2, p.k)))
    x = bases(p, 2)
    want = [ser.evaluate(p, ser.nominal(p.k), x[g]) for g in range(2)]
    for layout in (1, 2):
        eng = make_engine(p, 2, ensemble=zero, row_layout=layout)
        try:
            eng.set_base(x)
            for _ in range(2):
                r = eng.evaluate()
            assert r['grad'].shape == (2, p.k, p.steps) and eng.get_uks().shape == (2, p.k, p.steps) and eng.get_base().shape == (2, p.k, p.steps)
            for g in range(2):
                assert abs(r['loss'][g] - want[g]['loss']) <= S_RTOL and np.max(np.abs(r['grad'][g] - want[g]['grad'])) <= G_RTOL * np.max(np.abs(want[g]['grad']))
            m = eng.member_scalars()['loss']
            assert np.array_equal(m[:, 0], m[:, 1])
        finally:
            eng.close()
    # the trajectories' own gradient array: k_sp_grad stops at the kt real rows, the q frozen rows were cleared at creation and are never written --
    # exact zeros after two evaluations, in both layouts and under a map (kt = r = 3 rows in front of them), while the real rows carry a gradient
    for layout in (1, 2):
        for cm in (None, ref.make_map(2, 3, 2, 8, mix=True)):
            pm = p if cm is None else parity_problem(r=3)
            em = ens if cm is None else make_ensemble(pm, 2, 2)
            eng = make_engine(pm, 2, ensemble=em, row_layout=layout, control_map=cm)
            try:
                eng.set_base(bases(pm, 2))
                for _ in range(2):
                    eng.evaluate()
                g = eng.trajectory_gradient()
                kt = pm.k if cm is None else 3
                assert g.shape == (2, 2, kt + 2, pm.steps)
                assert np.array_equal(g[:, :, kt:], np.zeros((2, 2, 2, pm.steps))) and np.min(np.max(np.abs(g[:, :, :kt]), axis=3)) > 1e-6
            finally:
                eng.close()
    plain = make_engine(p, 1)
    try:
        plain.set_base(x[:1])
        plain.evaluate()
        with pytest.raises(P.QocError, match='not an ensemble engine'):
            plain.trajectory_gradient()
    finally:
        plain.close()


@pytest.mark.parametrize('layout', [1, 2])
def test_two_evaluations_are_bit_identical(layout):
    p = layout_problem('n257')
    ens = make_ensemble(p, 3, 2)
    x = bases(p, 2)
    runs = []
    for _ in range(2):
        eng = make_engine(p, 2, ensemble=ens, row_layout=layout)
        try:
            eng.set_base(x)
            for _ in range(2):
                r = eng.evaluate()
                runs.append(dict(r, inter=eng.get_inter_vecs(), member=eng.member_scalars()['loss']))
        finally:
            eng.close()
    for other in runs[1:]:
        for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale', 'grad', 'inter', 'member'):
            assert np.array_equal(runs[0][key], other[key]), key


def test_create_destroy_cycles_beside_a_live_plain_engine():
    p = layout_problem('n33')
    ens = make_ensemble(p, 2, 1)
    x = bases(p, 1)
    want_plain, want_ens = ser.evaluate(p, ser.nominal(p.k), x[0]), ser.evaluate(p, ens, x[0])
    plain = make_engine(p, 1)
    try:
        for cycle in range(10):
            eng = make_engine(p, 1, ensemble=ens, row_layout=1 + cycle % 2, vector_home=('lds', 'global')[(cycle // 2) % 2])
            try:
                eng.set_base(x)
                assert abs(eng.evaluate()['loss'][0] - want_ens['loss']) <= S_RTOL
            finally:
                eng.close()
            plain.set_base(x)
            assert abs(plain.evaluate()['loss'][0] - want_plain['loss']) <= S_RTOL
        big = make_engine(boundary_problem(5087), 1, row_layout=2)              # the largest merged LDS footprint beside the small engines
        try:
            big.set_base(bases(boundary_problem(5087), 1))
            assert np.isfinite(big.evaluate()['loss'][0])
            plain.set_base(x)
            assert abs(plain.evaluate()['loss'][0] - want_plain['loss']) <= S_RTOL
        finally:
            big.close()
    finally:
        plain.close()


# ---- 5. the device loops against the same loops on a dense ensemble engine ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def loop_case():
    p = ser.from_sparse_case(sr.sparse_case(64, 12, k=3, m=1, T=9, seed=60, reg_coeffs={'dwdt': 0.02, 'amplitude': 0.1}))
    return p, make_ensemble(p, 2, 2, seed=9), bases(p, 3, seed=3)


def _free_history(eng, x, iterate, evaluations):
    eng.set_base(x)
    hist = []
    for _ in range(evaluations):
        iterate(1)
        hist.append(eng.scalars()['loss'].copy())
    hist = np.array(hist)
    return [hist[:, b:b + 1] for b in range(hist.shape[1])]


def _compare_loops(dense, sparse, its_d, its_s):
    assert list(its_d) == list(its_s) and len(set(its_d)) >= 2, (its_d, its_s)       # (a set finishes inside a burst while its neighbours go on)
    sd, ss = dense.scalars(), sparse.scalars()
    assert list(sd['done']) == list(ss['done']) == [1, 1, 1]
    np.testing.assert_allclose(sparse.get_base(), dense.get_base(), rtol=0, atol=LOOP_ATOL)
    np.testing.assert_allclose(sparse.get_uks(evaluated=True), dense.get_uks(evaluated=True), rtol=0, atol=LOOP_ATOL)
    for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale'):
        np.testing.assert_allclose(ss[key], sd[key], rtol=0, atol=LOOP_ATOL)
    np.testing.assert_allclose(sparse.member_scalars()['loss'], dense.member_scalars()['loss'], rtol=0, atol=LOOP_ATOL)
    np.testing.assert_allclose(sparse.get_inter_vecs(), dense.get_inter_vecs(), rtol=0, atol=LOOP_ATOL)


@pytest.mark.parametrize('layout', [1, 2])
def test_adam_loop_against_the_dense_ensemble_engine(layout):
    p, ens, x = loop_case()
    max_it = 11
    dense, sparse = make_dense_engine(p, 3, ens), make_engine(p, 3, ensemble=ens, row_layout=layout)
    try:
        assert dense.path != P.PATH_SPARSE and sparse.path == P.PATH_SPARSE
        conv = dict(rate=0.05, max_iterations=max_it, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0)
        free = dense.adam_params(poll_every=1, **conv)
        target, stops = _choose_target(_free_history(dense, x, lambda n: dense.iterate(free, n), max_it + 1), max_it)
        conv['conv_target'] = target
        dense.set_base(x)
        sparse.set_base(x)
        its_d, its_s = dense.run_adam(dense.adam_params(poll_every=5, **conv)), sparse.run_adam(sparse.adam_params(poll_every=5, **conv))
        assert list(its_d) == stops
        _compare_loops(dense, sparse, its_d, its_s)
    finally:
        dense.close()
        sparse.close()


@pytest.mark.parametrize('layout', [1, 2])
def test_lbfgs_loop_against_the_dense_ensemble_engine(layout):
    p, ens, x = loop_case()
    max_it = 11
    dense, sparse = make_dense_engine(p, 3, ens), make_engine(p, 3, ensemble=ens, row_layout=layout)
    try:
        kw = dict(conv_target=-1.0, min_grad=-1.0, max_iterations=max_it, history=4)
        free = dense.lbfgs_params(poll_every=1, **kw)
        target, stops = _choose_target(_free_history(dense, x, lambda n: dense.iterate_lbfgs(free, n), max_it + 1), max_it)
        kw['conv_target'] = target
        dense.set_base(x)
        sparse.set_base(x)
        its_d, its_s = dense.run_lbfgs(dense.lbfgs_params(poll_every=5, **kw)), sparse.run_lbfgs(sparse.lbfgs_params(poll_every=5, **kw))
        _compare_loops(dense, sparse, its_d, its_s)
    finally:
        dense.close()
        sparse.close()


# ---- 6. what the C ABI refuses ---------------------------------------------------------------------------------------------------------------------------

def _raw_create(p, layout=0, cfg_set=None, ens=None, fleet=None, transfer=None, cmap_=None, operators=None, vector_home=0, null_plan=False, k=None):
    """qoc_create_sparse_fleet through ctypes with arguments the Python layer would not build; returns (status, message)."""
    lib = P.load_library()
    cfg = P.QocConfig()
    cfg.n, cfg.k, cfg.steps, cfg.m, cfg.taylor_terms, cfg.scaling, cfg.state_transfer, cfg.n_seeds = p.n, p.k if k is None else k, p.steps, p.m, p.T, 0, 1, 1
    cfg.dt, cfg.total_time = p.dt, p.total_time
    for key, val in (cfg_set or {}).items():
        setattr(cfg, key, val)
    n, indptr, row, col, val = P.sparse_arrays(p.engine_ops()) if operators is None else operators
    s = P.QocSparse()
    s.indptr, s.row, s.col = indptr.ctypes.data_as(C.POINTER(C.c_int64)), row.ctypes.data_as(P._IP), col.ctypes.data_as(P._IP)
    s.val, s.vector_home = P._dp(val.view(np.float64)), vector_home
    pl = P.QocSparsePlan()
    pl.row_layout = layout
    keep = []

    def dp(a):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
        keep.append(a)
        return P._dp(a)
    e = f = t = m = None
    if ens is not None:
        e = P.QocEnsemble()
        e.members, e.n_perturb = ens['members'], ens.get('q', 0)
        e.P = dp(ens['P']) if 'P' in ens else None
        e.offsets = dp(ens['offsets']) if 'offsets' in ens else None
        e.amp_scales, e.weights = dp(ens.get('amp', np.ones((max(ens['members'], 1), cfg.k)))), dp(ens.get('weights', np.ones(max(ens['members'], 1))))
    if fleet is not None:
        f = P.QocFleet()
        f.devices, f.offsets, f.amp_scales = fleet['devices'], None, dp(fleet['amp'])
    if transfer is not None:
        t = P.QocTransfer()
        t.n_samples, t.T = transfer.shape[1], dp(transfer)
    if cmap_ is not None:
        m = P.QocControlMap()
        m.n_terms, m.degree, m.poly, m.mix, m.fixed = cmap_['r'], cmap_['D'], dp(cmap_['poly']), None, None
    Vc, Wc, maxA = np.ascontiguousarray(p.V), np.ascontiguousarray(p.W), np.ascontiguousarray(np.ones(cfg.k))
    omg = dp(np.ones((cfg.k, p.steps)))
    h = C.c_void_p()
    rc = lib.qoc_create_sparse_fleet(C.byref(cfg), C.byref(s), None if null_plan else C.byref(pl), None if e is None else C.byref(e), None if f is None else C.byref(f),
                                     None if t is None else C.byref(t), None if m is None else C.byref(m), P._dp(Vc.view(np.float64)), P._dp(Wc.view(np.float64)),
                                     P._dp(maxA), omg, None, None, C.byref(h))
    msg = lib.qoc_last_error().decode()
    if rc == 0:
        lib.qoc_destroy(h)
    return rc, msg


def _empty_operators(n, K):
    return n, np.zeros(K + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.complex128)


C_REFUSALS = {
    'row_layout_3': (dict(layout=3), 'row_layout = 3'),
    'row_layout_negative': (dict(layout=-1), 'row_layout = -1'),
    'ens_P': (dict(ens=dict(members=2, q=0, P=np.zeros(2))), 'ens->P must be NULL'),
    'members_0': (dict(ens=dict(members=0)), 'members = 0'),
    'negative_weight': (dict(ens=dict(members=2, weights=[1.0, -0.5])), 'weight 1'),
    'nan_weight': (dict(ens=dict(members=2, weights=[1.0, np.nan])), 'weight 1'),
    'offsets_missing': (dict(ens=dict(members=2, q=1), operators='one_more'), 'ensemble arrays missing'),
    'devices_0': (dict(fleet=dict(devices=0, amp=np.ones((1, 1, 2)))), 'devices = 0'),
    'seeds_no_multiple': (dict(fleet=dict(devices=2, amp=np.ones((2, 1, 2))), cfg_set=dict(n_seeds=3)), 'no multiple of devices'),
    'fleet_table_inf': (dict(fleet=dict(devices=1, amp=np.array([[[1.0, np.inf]]]))), 'not finite'),
    'envelope_with_a_line': (dict(transfer=np.eye(4), cfg_set=dict(has_envelope=1, c_envelope=0.1)), 'envelope'),
    'line_nan': (dict(transfer=np.full((4, 2), np.nan)), 'not finite'),
    'map_terms_0': (dict(cmap_=dict(r=0, D=1, poly=np.ones(4))), 'n_terms = 0'),
    'map_degree_9': (dict(cmap_=dict(r=2, D=9, poly=np.ones(36))), 'degree = 9'),
    'merged_256_operators': (dict(layout=2, k=255, operators=('empty', 256)), 'at most 255'),
    'merged_n_2_24': (dict(layout=2, cfg_set=dict(n=1 << 24), operators=('empty', 3)), '24 bits'),
    'unitary_mode': (dict(cfg_set=dict(state_transfer=0)), 'state-transfer mode only'),
    'exact_gradient': (dict(cfg_set=dict(gradient=1)), 'exact gradient'),
    'time_shards': (dict(cfg_set=dict(time_shards=2)), 'time-sharded'),
    'path_generic': (dict(cfg_set=dict(path=P.PATH_GENERIC)), 'not on path 1'),
    'taylor_61': (dict(cfg_set=dict(taylor_terms=61)), 'taylor_terms = 61'),
    'vector_home_3': (dict(vector_home=3), 'vector_home = 3'),
}


@pytest.mark.parametrize('name', list(C_REFUSALS))
def test_c_level_refusals(name):
    kw, needle = C_REFUSALS[name]
    kw = dict(kw)
    p = layout_problem('n5')
    ops = kw.pop('operators', None)
    if ops == 'one_more':
        kw['operators'] = P.sparse_arrays(p.engine_ops() + [p.engine_ops()[0]])
    elif ops is not None:
        kw['operators'] = _empty_operators(kw.get('cfg_set', {}).get('n', p.n), ops[1])
    rc, msg = _raw_create(p, **kw)
    assert rc == -1 and msg.startswith('qoc_create_sparse_fleet') and needle in msg, (rc, msg)


def test_c_level_entry_accepts_the_untouched_arguments_and_auto_falls_back():
    p = layout_problem('n5')
    assert _raw_create(p)[0] == 0 and _raw_create(p, null_plan=True)[0] == 0 and _raw_create(p, layout=2)[0] == 0
    assert _raw_create(p, layout=0, k=255, operators=_empty_operators(p.n, 256))[0] == 0          # auto with 256 operators: per-operator rows


# ---- 7. the example -----------------------------------------------------------------------------------------------------------------------------------------

def test_disordered_chain_example():
    """examples/disordered_chain_transfer.py at a reduced size: both pulses arrive on the nominal chain, and the ensemble's pulse is no worse over the
    members it was optimised for."""
    import disordered_chain_transfer
    with contextlib.redirect_stdout(io.StringIO()):
        nominal, robust = disordered_chain_transfer.main(spins=5, iterations=120, members=3, spread=0.05, steps=50, quiet=True)
    print('nominal pulse %r, robust pulse %r' % (nominal, robust))
    assert nominal.shape == robust.shape == (3,) and nominal[0] < 0.1 and robust.mean() < 0.1
    assert robust.mean() <= nominal.mean() + 1e-3
