"""Noise traces on the GPU (qoc_set_traces): with a table, frozen row q' of member e of device f runs offsets[f][e][q'] + traces[f][e][q'][t].

  1. evaluation against the reference composed from the unchanged oracle (tests/noise_reference.py) on every route that hosts a member table: dense
     closed on every kernel family, state regularisers, a line, a control map, a fleet, a risk, the exact gradient, open members, sparse operators;
  2. bit identity (==): an all-zero table against no table, constant traces against the same offsets, two evaluations;
  3. the setter: between evaluations, between two bursts of a running Adam loop, None, return codes and messages;
  4. the device Adam and L-BFGS loops against Python loops over the reference;
  5. Grape(robust=...) and Grape(fleet=...) with traces, the log, method='EVOLVE' over 64 members.

E = 3 members, q = 2 perturbations; n = 4, k = 2, steps = 8, m = 3 in unitary mode and n = 5, m = 2, steps = 7 in state transfer (tests/fleet_reference.py:
problem); the traces are random with one row zero except at a single slice (tests/noise_reference.py: make_traces), so that a transposed index cannot
pass.  Tolerances: S_RTOL, G_RTOL and U_ATOL of tests/test_robust_gpu.py (the open and sparse reference files use the same constants of
tests/test_hip_parity.py), LOOP_ATOL of tests/test_adam_tail.py for the loops."""
import contextlib
import functools
import io
import os

import numpy as np
import pytest

from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import fleet as fl_mod
from quantum_optimal_control.helper_functions import noise
from quantum_optimal_control.helper_functions import open_system
from quantum_optimal_control.helper_functions import robust as rb
from quantum_optimal_control.helper_functions import transfer as tf
from tests import control_map_reference as ref
from tests import fleet_reference as fr
from tests import lbfgs_reference as lb
from tests import noise_reference as nr
from tests import open_fleet_reference as ofr
from tests import sparse_ensemble_reference as ser
from tests import sparse_reference as sr
from tests import test_robust_gpu as rg
from tests.test_adam_tail import LOOP_ATOL, _choose_target
from tests.test_robust_gpu import G_RTOL, S_RTOL, U_ATOL

pytestmark = pytest.mark.gpu

P = hip_engine
E, Q = 3, 2
KEYS = ('loss', 'reg_loss', 'grad_squared', 'unitary_scale')
STATE_REGS = dict(fr.REGS_UNITARY, forbidden_coeff_list=[5.0], states_forbidden_list=[3], speed_up=0.3)


# ---- engines ------------------------------------------------------------------------------------------------------------------------------------

def dense_engine(c, n_sets, ens=None, fl=None, path=P.PATH_AUTO, variant=0, chunks=0, T=None, cm=None, exact=False):
    sp = ref.engine_system(c)
    return P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, c['maxA'], sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, state_transfer=sp.state_transfer,
                       reg_coeffs=c['reg_coeffs'], n_seeds=n_sets, path=path, variant=variant, chunks=chunks, ensemble=ens, transfer=T,
                       exact_gradient=exact, control_map=cm, fleet=fl)


def open_engine(p, n_sets, ens=None, fl=None, costs=None):
    sp = ofr.engine_system(p)
    return P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, p['maxA'], sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, state_transfer=sp.state_transfer,
                       reg_coeffs=p['reg_coeffs'], n_seeds=n_sets, ensemble=ens, fleet=fl, running_costs=costs)


def sparse_engine(p, n_sets, ens=None, fl=None, **kw):
    return P.HipEngine(None, None, p.V, p.W, p.maxA, p.dt, p.total_time, p.steps, p.T, 0, state_transfer=True, reg_coeffs=p.reg_coeffs, n_seeds=n_sets,
                       sparse_ops=p.engine_ops(), ensemble=ens, fleet=fl, **kw)


def assert_values(tag, r, g, o):
    for key in KEYS:
        print('%s %s[%d]: engine %.17g reference %.17g' % (tag, key, g, r[key][g], o[key]))
        assert abs(r[key][g] - o[key]) <= S_RTOL * max(1.0, abs(o[key])), (tag, key, g, r[key][g], o[key])
    gm = max(1.0, float(np.max(np.abs(o['grad']))))
    err = float(np.max(np.abs(r['grad'][g] - o['grad'])))
    print('%s grad[%d]: max error %.3e of max %.3e' % (tag, g, err, gm))
    assert err <= G_RTOL * gm, (tag, g, err, gm)


def assert_members(tag, ms, g, o):
    assert np.max(np.abs(ms['loss'][g] - o['member_loss'])) <= S_RTOL * max(1.0, np.max(np.abs(o['member_loss']))), (tag, g, ms['loss'][g], o['member_loss'])


def apart(wants, plain):
    """The precondition of every comparison, on the CPU: the members' expected losses lie pairwise more than 1e-6 apart, and so do the expectations
    with the table and without it -- an engine that reads another member's trace, or none, cannot pass."""
    for o, o0 in zip(wants, plain):
        assert fr.swapped_apart(list(o['member_loss'])), o['member_loss']
        assert fr.swapped_apart([o['member_loss'], o0['member_loss']]) and fr.swapped_apart([o['grad'], o0['grad']])


# ---- 1. evaluation against the reference ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def dense_case(kind, comp='plain'):
    """(problem, ensemble with traces, line, map, exact, start points, expectations): computed once per composition, shared by the kernel families."""
    k, r = 2, 3 if 'map' in comp else 2
    regs = STATE_REGS if comp == 'state_regs' else None
    c = fr.problem(kind, k=k, r=r, regs=regs)
    steps = c['steps']
    ens = rg.ensemble(c, E, Q) if r == k else ref.ensemble(c, E, Q)
    ens = nr.with_traces(dict(ens, risk=5.0 if comp == 'risk' else 0.0), nr.make_traces(E, Q, steps, seed=len(comp)))
    T = tf.hold(steps, 3).matrix if 'line' in comp else None
    cm = ref.make_map(k, r, 2, steps, mix=True, fixed=True) if 'map' in comp else None
    exact = comp == 'exact'
    xs = ref.variables(k, steps if T is None else 3, 2, seed=len(comp))
    wants = [nr.evaluate(c, ens, x, cm=cm, T=T, exact=exact) for x in xs]
    apart(wants, [nr.evaluate(c, nr.with_traces(ens, None), x, cm=cm, T=T, exact=exact) for x in xs])
    return c, ens, T, cm, exact, xs, wants


def check_dense(kind, comp, path, variant=0, chunks=0, plan=None):
    c, ens, T, cm, exact, xs, wants = dense_case(kind, comp)
    eng = dense_engine(c, len(xs), ens, path=path, variant=variant, chunks=chunks, T=T, cm=cm, exact=exact)
    try:
        assert eng.plan.get('traces') == '1', eng.plan                       # the table first
        for key, val in dict(plan or {}, members=str(E), perturbations=str(Q)).items():
            assert eng.plan.get(key) == val, (key, val, eng.plan)
        eng.set_base(xs)
        r = eng.evaluate()
        ms = eng.member_scalars()
        for g, o in enumerate(wants):
            tag = '%s/%s' % (kind, comp)
            assert_values(tag, r, g, o)
            assert_members(tag, ms, g, o)
        if c['state_transfer']:
            inter = eng.get_inter_vecs()
            for g, o in enumerate(wants):
                assert np.max(np.abs(inter[g] - o['inter_vecs'])) <= U_ATOL, g
        else:
            Uf, Um = eng.get_final_unitary(), eng.member_final_unitary()
            for g, o in enumerate(wants):
                assert np.max(np.abs(Uf[g] - o['U_final'])) <= U_ATOL and np.max(np.abs(Um[g] - o['member_U'])) <= U_ATOL, g
        if T is not None:
            np.testing.assert_allclose(eng.get_pulse(), np.stack([o['pulse'] for o in wants]), rtol=0, atol=U_ATOL)
        if cm is not None:
            np.testing.assert_allclose(eng.get_coefficients(), np.stack([o['coefficients'] for o in wants]), rtol=0, atol=U_ATOL)
    finally:
        eng.close()


FAMILIES = [
    ('unitary_auto', 'unitary', P.PATH_AUTO, 0, 0, {}),
    ('unitary_mfma', 'unitary', P.PATH_MFMA, 0, 0, dict(path='mfma')),
    ('unitary_gemm', 'unitary', P.PATH_GEMM, 0, 0, dict(path='gemm', route='unitary')),
    ('unitary_generic', 'unitary', P.PATH_GENERIC, 0, 0, dict(path='generic')),
    ('state_auto', 'state', P.PATH_AUTO, 0, 0, {}),
    ('state_mfma', 'state', P.PATH_MFMA, 0, 0, dict(path='mfma')),
    ('state_gemm_direct', 'state', P.PATH_GEMM, 0, 1, dict(path='gemm', route='direct')),
    ('state_gemm_propagator', 'state', P.PATH_GEMM, 0, 2, dict(path='gemm', route='propagator')),
    ('state_st_fused', 'state', P.PATH_ST_FUSED, 0, 0, dict(path='st_fused')),
    ('state_generic', 'state', P.PATH_GENERIC, 0, 0, dict(path='generic')),
]


@pytest.mark.parametrize('name,kind,path,variant,chunks,plan', FAMILIES, ids=[row[0] for row in FAMILIES])
def test_plain_ensembles_on_every_kernel_family(name, kind, path, variant, chunks, plan):
    check_dense(kind, 'plain', path, variant, chunks, plan)


COMPOSITIONS = [('unitary', 'state_regs'), ('state', 'plain_regs'), ('unitary', 'line'), ('state', 'line'), ('unitary', 'map'), ('state', 'map'),
                ('unitary', 'map_line'), ('unitary', 'risk'), ('state', 'risk'), ('unitary', 'exact'), ('state', 'exact')]


@pytest.mark.parametrize('kind,comp', COMPOSITIONS, ids=['%s-%s' % row for row in COMPOSITIONS])
def test_compositions(kind, comp):
    """State regularisers (unitary: a forbidden level and speed_up added; state transfer: tests/fleet_reference.py: REGS_STATE has them already), a
    hold line (k_shape_expand), a control map with and without a line (k_map_expand copies the frozen rows through), risk beta = 5, the exact gradient."""
    check_dense(kind, comp, P.PATH_AUTO, plan=dict(samples='3') if 'line' in comp else None)


F, R = 2, 2


@functools.lru_cache(maxsize=None)
def fleet_case(kind):
    c = fr.problem(kind)
    base = fr.make_fleet(c, F, E, Q)
    tr = nr.make_traces(E, Q, c['steps'], seed=11, F=F)
    fl = fl_mod.validate(fl_mod.Fleet(base.operators, base.offsets, base.amp_scales, weights=base.weights, traces=tr), len(c['H0']), 2, steps=c['steps'])
    xs = ref.variables(2, c['steps'], 2, seed=5)[[0, 1, 0, 1]]                # (devices 0 and 1 start from the same two points)
    wants = [nr.evaluate(c, fl.device(f), xs[g]) for g, (f, _) in enumerate(fr.control_sets(F, R))]
    apart(wants, [nr.evaluate(c, nr.with_traces(fl.device(f), None), xs[g]) for g, (f, _) in enumerate(fr.control_sets(F, R))])
    # the devices differ in their traces: device 0's rows with device 1's table lie apart from both
    crossed = nr.evaluate(c, nr.with_traces(fl.device(0), tr[1]), xs[0])
    assert fr.swapped_apart([wants[0]['loss'], wants[2]['loss'], crossed['loss']]) and fr.swapped_apart([wants[0]['grad'], wants[2]['grad'], crossed['grad']])
    return c, fl, xs, wants


@pytest.mark.parametrize('kind', ['unitary', 'state'])
def test_fleet_whose_devices_differ_in_their_traces(kind):
    c, fl, xs, wants = fleet_case(kind)
    eng = dense_engine(c, F * R, fl=fl)
    try:
        assert eng.plan.get('traces') == '1' and eng.plan['devices'] == str(F), eng.plan
        eng.set_base(xs)
        r, ms = eng.evaluate(), eng.member_scalars()
        for g, o in enumerate(wants):
            assert_values('fleet/' + kind, r, g, o)
            assert_members('fleet', ms, g, o)
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def open_case(name):
    """n = 3, c = 1 collapse operator, k = 2, 6 slices, m = 2: an open ensemble, the same with a running cost, an open fleet F = 2, R = 2."""
    p = ofr.problem(3, 2, 6, 2, 1, taylor=(6, 1), regs={'dwdt': 0.02})
    costs = open_system.validate_costs([open_system.level_cost(3, 2, 0.7)], 3) if name == 'costs' else None
    n_dev = F if name == 'fleet' else 1
    base = ofr.make_fleet(p, n_dev, E, Q, zero=False)
    tr = nr.make_traces(E, Q, 6, seed=21, F=n_dev)
    fl = fl_mod.validate(fl_mod.Fleet(base.operators, base.offsets, base.amp_scales, weights=base.weights, collapse_ops=base.collapse_ops,
                                      rate_scales=base.rate_scales, traces=tr), 3, 2, steps=6)
    sets = fr.control_sets(n_dev, R)
    xs = ref.variables(2, 6, 2, seed=7)[[r for _, r in sets]]
    wants = [nr.evaluate_open(p, fl.device(f), xs[g], costs=costs or ()) for g, (f, _) in enumerate(sets)]
    apart(wants, [nr.evaluate_open(p, nr.with_traces(fl.device(f), None), xs[g], costs=costs or ()) for g, (f, _) in enumerate(sets)])
    if name == 'fleet':
        assert fr.swapped_apart([wants[0]['loss'], wants[2]['loss']]) and fr.swapped_apart([wants[0]['grad'], wants[2]['grad']])
    return p, fl, costs, xs, wants


@pytest.mark.parametrize('name', ['ensemble', 'costs', 'fleet'])
def test_open_members(name):
    p, fl, costs, xs, wants = open_case(name)
    eng = open_engine(p, len(xs), fl=fl, costs=costs) if name == 'fleet' else open_engine(p, len(xs), ens=fl.device(0), costs=costs)
    try:
        assert eng.plan.get('traces') == '1' and eng.plan['path'] == 'lindblad' and eng.plan['collapse'] == '1', eng.plan
        assert (eng.plan.get('running_costs') == '1') == (name == 'costs')
        eng.set_base(xs)
        r, ms, rho0, rho_m = eng.evaluate(), eng.member_scalars(), eng.get_final_density(), eng.member_final_density()
        for g, o in enumerate(wants):
            assert_values('open/' + name, r, g, o)
            assert_members('open', ms, g, o)
            assert np.max(np.abs(ms['reg_state'][g] - o['member_reg_state'])) <= S_RTOL
            assert np.max(np.abs(rho0[g] - o['rho_final'])) <= S_RTOL and np.max(np.abs(rho_m[g] - o['member_rho'])) <= S_RTOL, g
        if name == 'costs':
            x = eng.get_expectations()
            assert all(np.max(np.abs(x[g] - o['expectations'])) <= S_RTOL for g, o in enumerate(wants))
            assert min(float(np.min(o['member_reg_state'])) for o in wants) > 1e-4
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def sparse_case():
    """A 4-spin XX chain (n = 16), k = 2, 8 slices, E = 3 members over q = 2 sparse perturbations, F = 2 devices of R = 2 control sets."""
    p = ser.from_sparse_case(sr.chain_problem(4, 8, 8, k=2))
    rng = np.random.default_rng(31)
    ops = [0.5 * sr.random_sparse(rng, p.n, (1, 3)) for _ in range(Q)]
    fl = fl_mod.validate(fl_mod.Fleet(ops, rng.uniform(-0.2, 0.2, size=(F, E, Q)), rng.uniform(0.9, 1.1, size=(F, E, 2)), weights=rng.uniform(0.5, 1.5, size=E),
                                      traces=nr.make_traces(E, Q, 8, seed=33, F=F)), p.n, 2, sparse=True, steps=8)
    sets = fr.control_sets(F, R)
    xs = np.random.default_rng(35).normal(0.0, 0.6, size=(2, 2, 8))[[r for _, r in sets]]
    wants = [nr.evaluate_sparse(p, fl.device(f), xs[g]) for g, (f, _) in enumerate(sets)]
    apart(wants, [nr.evaluate_sparse(p, nr.with_traces(fl.device(f), None), xs[g]) for g, (f, _) in enumerate(sets)])
    assert fr.swapped_apart([wants[0]['loss'], wants[2]['loss']]) and fr.swapped_apart([wants[0]['grad'], wants[2]['grad']])
    return p, fl, xs, wants


@pytest.mark.parametrize('home', ['lds', 'global'])
@pytest.mark.parametrize('layout', [1, 2], ids=['per_operator', 'merged'])
def test_sparse_fleet_in_both_row_layouts_and_vector_homes(layout, home):
    p, fl, xs, wants = sparse_case()
    eng = sparse_engine(p, F * R, fl=fl, row_layout=layout, vector_home=home)
    try:
        plan = eng.plan
        assert plan.get('traces') == '1' and (plan['path'], plan['rows'], plan['vector_home']) == ('sparse', 'merged' if layout == 2 else 'per_operator', home), plan
        eng.set_base(xs)
        r, ms, inter = eng.evaluate(), eng.member_scalars(), eng.get_inter_vecs()
        for g, o in enumerate(wants):
            assert_values('sparse', r, g, o)
            assert_members('sparse', ms, g, o)
            assert np.max(np.abs(inter[g] - o['inter_vecs'])) <= U_ATOL * max(1.0, np.max(np.abs(o['inter_vecs'])))
    finally:
        eng.close()


# ---- 2. bit identity ----------------------------------------------------------------------------------------------------------------------------------

def _dense_row(shaped):
    c, ens, _, _, _, _, _ = dense_case('unitary')
    T = tf.hold(c['steps'], 3).matrix if shaped else None
    xs = ref.variables(2, 3 if shaped else c['steps'], 2, seed=2)
    return ens, xs, lambda e: dense_engine(c, 2, e, T=T)


def _open_row():
    p, fl, _, xs, _ = open_case('ensemble')
    return fl.device(0), xs, lambda e: open_engine(p, 2, ens=e)


def _sparse_row():
    p, fl, xs, _ = sparse_case()
    return fl.device(0), xs[:2], lambda e: sparse_engine(p, 2, ens=e, row_layout=2)


BIT_ROWS = {'dense': lambda: _dense_row(False), 'shaped': lambda: _dense_row(True), 'open': _open_row, 'sparse': _sparse_row}


def everything(eng, xs):
    """Two evaluations at xs: what the second reports, after asserting that it reports what the first did."""
    eng.set_base(xs)
    out = []
    for _ in range(2):
        r, ms = eng.evaluate(), eng.member_scalars()
        out.append(dict(r, member_loss=ms['loss'], member_reg_state=ms['reg_state'], trajectory_gradient=eng.trajectory_gradient()))
    for key, val in out[0].items():
        np.testing.assert_array_equal(out[1][key], val, err_msg='second evaluation: ' + key)
    return out[1]


@pytest.mark.parametrize('row', list(BIT_ROWS))
def test_zero_and_constant_tables_are_bit_identical_to_no_table(row):
    ens, xs, build = BIT_ROWS[row]()
    steps = ens['traces'].shape[2]
    const = np.repeat(ens['offsets'][:, :, None], steps, axis=2)
    variants = dict(no_table=nr.with_traces(ens, None), zero_table=nr.with_traces(ens, np.zeros_like(ens['traces'])),
                    constant_table=nr.with_traces(dict(ens, offsets=np.zeros_like(ens['offsets'])), const), table=ens)
    got = {}
    for name, e in variants.items():
        eng = build(e)
        try:
            assert ('traces' in eng.plan) == (name != 'no_table'), (name, eng.plan)
            got[name] = everything(eng, xs)
        finally:
            eng.close()
    for name in ('zero_table', 'constant_table'):
        for key, val in got['no_table'].items():
            np.testing.assert_array_equal(got[name][key], val, err_msg='%s: %s' % (name, key))
    assert not np.array_equal(got['table']['loss'], got['no_table']['loss'])


# ---- 3. the setter ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('row', list(BIT_ROWS))
def test_setting_a_table_between_two_evaluations(row):
    ens, xs, build = BIT_ROWS[row]()
    bare = nr.with_traces(ens, None)
    eng, fresh = build(bare), build(ens)
    try:
        before_line = dict(eng.plan)
        before = everything(eng, xs)
        eng.set_traces(ens['traces'])
        assert eng.plan.get('traces') == '1' and {k: v for k, v in eng.plan.items() if k != 'traces'} == before_line
        with_table, want = everything(eng, xs), everything(fresh, xs)
        for key, val in want.items():
            np.testing.assert_array_equal(with_table[key], val, err_msg=key)
        assert not np.array_equal(with_table['loss'], before['loss'])
        other = ens['traces'][::-1].copy()                                  # a later call overwrites the table
        eng.set_traces(other)
        fresh.set_traces(other)
        a, b = everything(eng, xs), everything(fresh, xs)
        assert np.array_equal(a['loss'], b['loss']) and np.array_equal(a['grad'], b['grad']) and not np.array_equal(a['loss'], with_table['loss'])
        eng.set_traces(None)
        assert eng.plan == before_line
        after = everything(eng, xs)
        for key, val in before.items():
            np.testing.assert_array_equal(after[key], val, err_msg='after None: ' + key)
    finally:
        eng.close()
        fresh.close()


LOOP = dict(rate=0.05, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=100)


def test_setting_a_table_between_two_bursts_of_a_running_adam_loop():
    """Five iterations without a table, five with one, on one engine: the Adam moments and counters carry over (the setter resets nothing), so the
    variable follows the Python Adam loop whose evaluations switch to the table at the sixth; the evaluation at the point reached equals a fresh
    engine's that was created with the table."""
    c, ens, _, _, _, xs, _ = dense_case('unitary')
    bare = nr.with_traces(ens, None)
    eng, fresh = dense_engine(c, 2, bare), dense_engine(c, 2, ens)
    try:
        params = eng.adam_params(poll_every=100, **LOOP)
        eng.set_base(xs)
        eng.iterate(params, 5)
        eng.set_traces(ens['traces'])
        eng.iterate(params, 5)
        s, base = eng.scalars(), eng.get_base()
        assert list(s['iterations']) == [10, 10] and list(s['done']) == [0, 0]
        for g in range(2):
            x, opt = np.array(xs[g]), ref.go.Adam(xs[g].shape)
            for it in range(1, 11):
                r = nr.evaluate(c, bare if it <= 5 else ens, x)
                x = opt.step(x, r['grad'], LOOP['rate'] * np.exp(-float(it) / LOOP['learning_rate_decay']))
            print('set %d: max |base - reference| %.3e' % (g, np.max(np.abs(base[g] - x))))
            np.testing.assert_allclose(base[g], x, rtol=0, atol=LOOP_ATOL)
            stayed = nr.evaluate(c, bare, x, want_grad=False)['loss']
            assert abs(stayed - nr.evaluate(c, ens, x, want_grad=False)['loss']) > 1e-6
        got, want = everything(eng, base), everything(fresh, base)          # (both from set_base: the same variable, the same first launch)
        for key, val in want.items():
            np.testing.assert_array_equal(got[key], val, err_msg=key)
    finally:
        eng.close()
        fresh.close()


def test_return_codes_and_messages():
    c, ens, _, _, _, xs, _ = dense_case('unitary')
    table = np.zeros((E, Q, c['steps']))
    sp = ref.engine_system(c)
    plain = P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, c['maxA'], sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, reg_coeffs={}, n_seeds=1)
    p, _, _, _, _ = open_case('ensemble')
    osp = ofr.engine_system(p)
    opened = P.HipEngine(osp.Hs, osp.U0, osp.V, osp.W, p['maxA'], osp.dt, osp.total_time, osp.steps, osp.exp_terms, osp.scaling, reg_coeffs={}, n_seeds=1,
                         collapse_ops=p['collapse_ops'])
    q, _, _, _ = sparse_case()
    sparse = sparse_engine(q, 1)
    nominal = dense_engine(c, 1, rb.validate(dict(operators=[], offsets=np.zeros((E, 0)), amp_scales=np.ones((E, 2))), 4, 2))
    good = dense_engine(c, 2, nr.with_traces(ens, None))
    try:
        assert (plain.plan['path'], opened.plan['path'], sparse.plan['path']) != ('', '', '') and 'members' not in plain.plan and 'rows' not in sparse.plan
        for eng in (plain, opened, sparse):                                 # qoc_create, qoc_create_open, qoc_create_sparse
            with pytest.raises(P.QocError, match=r'status -4: qoc_set_traces: the engine has no member table'):
                eng.set_traces(table)
            with pytest.raises(P.QocError, match=r'status -4: qoc_set_traces: the engine has no member table'):
                eng.set_traces(None)
        with pytest.raises(P.QocError, match=r'status -4: qoc_set_traces: the members have no perturbation row to add a trace to \(q = 0\)'):
            nominal.set_traces(np.zeros((E, 0, c['steps'])))
        bad = table.copy()
        bad[1, 1, 3] = np.nan
        with pytest.raises(P.QocError, match=r'status -1: qoc_set_traces: entry %d of the table is not finite' % ((1 * Q + 1) * c['steps'] + 3)):
            good.set_traces(bad)
        bad[1, 1, 3] = np.inf
        with pytest.raises(P.QocError, match='status -1: qoc_set_traces: entry'):
            good.set_traces(bad)
        assert 'traces' not in good.plan                                    # a refused table is not set
        with pytest.raises(ValueError, match=r'traces have shape \(3, 8, 2\), expected \(3, 2, 8\)'):
            good.set_traces(np.zeros((E, c['steps'], Q)))
        good.set_base(xs)
        good.evaluate()
    finally:
        for eng in (plain, opened, sparse, nominal, good):
            eng.close()


# ---- 4. loops -----------------------------------------------------------------------------------------------------------------------------------------

def _loop_row(row):
    """(evaluate_at(g) -> x -> reference dict, start points, engine factory, iteration budget) of a row with a table."""
    if row == 'dense':
        c, ens, _, _, _, xs, _ = dense_case('unitary')
        return (lambda g: lambda x: nr.evaluate(c, ens, x)), xs, (lambda: dense_engine(c, 2, ens)), 30
    if row == 'open':
        p, fl, _, xs, _ = open_case('ensemble')
        return (lambda g: lambda x: nr.evaluate_open(p, fl.device(0), x)), xs, (lambda: open_engine(p, 2, ens=fl.device(0))), 12
    p, fl, xs, _ = sparse_case()
    return (lambda g: lambda x: nr.evaluate_sparse(p, fl.device(0), x)), xs[:2], (lambda: sparse_engine(p, 2, ens=fl.device(0), row_layout=2)), 12


@functools.lru_cache(maxsize=None)
def adam_reference(row):
    at, xs, build, budget = _loop_row(row)
    conv = dict(LOOP, max_iterations=budget)
    free = [ofr.run_adam(at(g), xs[g], conv) for g in range(2)]
    target, stops = _choose_target([run['history'] for run in free], budget)
    conv = dict(conv, conv_target=target)
    refs = [ofr.run_adam(at(g), xs[g], conv) for g in range(2)]
    assert [run['iterations'] for run in refs] == stops and len(set(stops)) == 2
    return xs, build, conv, refs, stops


@pytest.mark.parametrize('row', ['dense', 'open', 'sparse'])
def test_adam_loop_against_the_python_loop_over_the_reference(row):
    xs, build, conv, refs, stops = adam_reference(row)
    poll = next(q for q in (5, 4, 7, 3, 6, 9, 8, 13) if all(s % q for s in stops))
    eng = build()
    try:
        assert eng.plan.get('traces') == '1'
        eng.set_base(xs)
        its = eng.run_adam(eng.adam_params(poll_every=poll, **conv))
        s, base, ms = eng.scalars(), eng.get_base(), eng.member_scalars()
        print(eng.plan, 'stops', stops, 'poll', poll)
        assert list(its) == stops and list(s['iterations']) == stops and list(s['done']) == [1, 1], (its, stops)
        for g, run in enumerate(refs):
            print('set %d: %d iterations, max |base - reference| %.3e' % (g, stops[g], np.max(np.abs(base[g] - run['base']))))
            np.testing.assert_allclose(base[g], run['base'], rtol=0, atol=LOOP_ATOL)
            for key in KEYS:
                assert abs(s[key][g] - run['last'][key]) <= LOOP_ATOL * max(1.0, abs(run['last'][key])), (key, g)
            np.testing.assert_allclose(ms['loss'][g], run['last']['member_loss'], rtol=0, atol=LOOP_ATOL)
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def lbfgs_reference(row):
    at, xs, build, budget = _loop_row(row)
    budget = min(budget, 10)
    free = [lb.run(at(g), xs[g], dict(conv_target=-1.0, min_grad=-1.0, max_iterations=budget)) for g in range(2)]
    hists = [np.array(rec['loss'])[:budget, None] for rec in free]
    target, _ = _choose_target(hists, budget)
    params = dict(conv_target=target, min_grad=-1.0, max_iterations=budget)
    recs = [lb.run(at(g), xs[g], params) for g in range(2)]
    assert len({rec['state'].iters for rec in recs}) == 2, [rec['state'].iters for rec in recs]
    for rec in recs:                                     # no Armijo decision of the reference rests on the last bits
        assert all(mg is None or abs(mg) > 1e-9 for mg in rec['margin']), rec['margin']
    return at, xs, build, params, recs


@pytest.mark.parametrize('row', ['dense', 'open', 'sparse'])
def test_lbfgs_loop_against_the_reference_loop(row):
    at, xs, build, params, recs = lbfgs_reference(row)
    eng = build()
    try:
        eng.set_base(xs)
        its = eng.run_lbfgs(eng.lbfgs_params(poll_every=3, **params))
        s, base = eng.scalars(), eng.get_base()
        res = eng.evaluate()
        for g, rec in enumerate(recs):
            o = at(g)(rec['x'])
            print('set %d: %d iterations (reference %d, %s), max |base - reference| %.3e' % (g, its[g], rec['state'].iters, rec['branch'],
                                                                                           np.max(np.abs(base[g] - rec['x']))))
            assert int(its[g]) == int(s['iterations'][g]) == rec['state'].iters and int(s['done'][g]) == 1, (g, its, rec['state'].iters)
            np.testing.assert_allclose(base[g], rec['x'], rtol=0, atol=LOOP_ATOL)
            assert abs(res['reg_loss'][g] - o['reg_loss']) <= LOOP_ATOL * max(1.0, abs(o['reg_loss'])), (g, res['reg_loss'][g], o['reg_loss'])
    finally:
        eng.close()


# ---- 5. Grape end to end --------------------------------------------------------------------------------------------------------------------------------

SX = np.array([[0, 1], [1, 0]], dtype=np.complex128)
SY = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
SZ = np.diag([1.0, -1.0]).astype(np.complex128)
QUBIT = dict(H0=0.0 * SZ, Hops=[0.5 * SX, 0.5 * SY], Hnames=['x', 'y'], U=SX, total_time=10.0, steps=20, states_concerned_list=[0, 1])
CONV = {'rate': 0.05, 'update_step': 5, 'max_iterations': 15, 'conv_target': 1e-12, 'learning_rate_decay': 100}


def _grape(**kw):
    from quantum_optimal_control.main_grape.grape import Grape
    with contextlib.redirect_stdout(io.StringIO()):
        return Grape(QUBIT['H0'], QUBIT['Hops'], QUBIT['Hnames'], QUBIT['U'], QUBIT['total_time'], QUBIT['steps'], QUBIT['states_concerned_list'],
                     show_plots=False, maxA=[0.2, 0.2], Taylor_terms=[10, 1], reg_coeffs={}, **kw)


def _qubit_case():
    return dict(H0=QUBIT['H0'], Hops=QUBIT['Hops'], U=QUBIT['U'], total_time=10.0, steps=20, states_concerned_list=[0, 1], U0=np.eye(2), maxA=[0.2, 0.2],
                state_transfer=False, Taylor_terms=[10, 1], reg_coeffs={}, np_seed=0)


def _qubit_ensemble(members, seed=3):
    dt = QUBIT['total_time'] / QUBIT['steps']
    return noise.ensemble([2 * np.pi * 0.5 * SZ], [noise.ornstein_uhlenbeck(members, QUBIT['steps'], dt, 0.02, 3.0, seed)], k=2)


class RecordingLog(object):
    """What Grape writes to its run log, kept in memory: helper_functions.data_management.H5File's add / append / create_group behind the same
    context manager (h5py is an optional dependency; what is checked here is what Grape logs, not how HDF5 stores it)."""
    files = {}

    def __init__(self, path, mode='a'):
        self.data = RecordingLog.files.setdefault(str(path), {})

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def add(self, key, data):
        self.data[key] = np.array(data)

    def append(self, key, data, force_append=False):
        self.data.setdefault(key, []).append(np.array(data))

    def create_group(self, name):
        group = self.data.setdefault(name, {})
        return type('Group', (), {'create_dataset': staticmethod(lambda key, data=None: group.__setitem__(key, data))})


def test_grape_robust_call_with_traces_and_its_log(tmp_path, monkeypatch):
    """The documented shapes, run_session's member losses (the log's robust_member_loss: the reported control set at its last evaluation) against the
    reference at the returned pulse, the table in the log, and the slice count checked before anything is built."""
    from quantum_optimal_control.helper_functions import data_management
    from quantum_optimal_control.main_grape.grape import Grape
    monkeypatch.setattr(data_management, 'H5File', RecordingLog)
    np.random.seed(1)
    ens = _qubit_ensemble(4)
    uks, Uf = _grape(robust=ens, convergence=CONV, save=True, file_name='noise', data_path=str(tmp_path))
    assert np.shape(uks) == (2, 20) and np.shape(Uf) == (2, 2)
    log = RecordingLog.files[os.path.join(str(tmp_path), '00000_noise.h5')]
    assert np.array_equal(log['robust_traces'], ens['traces']) and log['robust_offsets'].shape == (4, 1)
    logged = np.asarray(log['robust_member_loss']).reshape(-1)
    o = nr.evaluate(_qubit_case(), ens, np.arcsin(np.asarray(uks) / 0.2), want_grad=False)
    print('member losses: logged %s reference %s' % (logged, o['member_loss']))
    assert logged.shape == (4,) and np.max(np.abs(logged - o['member_loss'])) <= S_RTOL and fr.swapped_apart(list(o['member_loss']), floor=1e-9)
    assert np.max(np.abs(np.asarray(Uf) - o['U_final'])) <= U_ATOL
    with pytest.raises(ValueError, match='robust: traces have 20 slices, the pulse has 10'):
        Grape(QUBIT['H0'], QUBIT['Hops'], QUBIT['Hnames'], QUBIT['U'], 10.0, 10, [0, 1], robust=ens, reg_coeffs={}, save=False, show_plots=False)


def test_grape_fleet_call_with_traces():
    np.random.seed(1)
    dt = QUBIT['total_time'] / QUBIT['steps']
    op = 2 * np.pi * 0.5 * SZ
    tr = np.stack([noise.ornstein_uhlenbeck(3, 20, dt, 0.02, 3.0, 5 + f) for f in range(2)])[:, :, None, :]
    fl = fl_mod.around([op], offsets=[[-0.01], [0.01]], robust=rb.validate(dict(operators=[op], offsets=np.zeros((3, 1))), 2, 2), k=2, traces=tr)
    uks, Uf = _grape(fleet=fl, convergence=CONV, save=False, restarts=2)
    assert np.shape(uks) == (2, 2, 20) and np.shape(Uf) == (2, 2, 2) and fl.member_losses.shape == (2, 3) and fl.losses.shape == (2,)
    for f in range(2):
        o = nr.evaluate(_qubit_case(), fl.device(f), np.arcsin(np.asarray(uks[f]) / 0.2), want_grad=False)
        print('device %d: member losses %s reference %s' % (f, fl.member_losses[f], o['member_loss']))
        assert np.max(np.abs(fl.member_losses[f] - o['member_loss'])) <= S_RTOL and abs(fl.losses[f] - o['loss']) <= S_RTOL
        assert np.max(np.abs(np.asarray(Uf[f]) - o['U_final'])) <= U_ATOL


def test_evolve_scores_a_pulse_on_64_members_in_one_call():
    """method='EVOLVE' with initial_guess=pulse: one call, one evaluation, every member's loss (Grape's _restart_info hook reads them off the engine)."""
    np.random.seed(2)
    ens = _qubit_ensemble(64, seed=9)
    pulse = 0.1 * np.sin(np.linspace(0.0, np.pi, 20))[None, :] * np.array([[1.0], [0.3]])
    info = {}
    uks, _ = _grape(robust=ens, method='EVOLVE', initial_guess=pulse, save=False, _restart_info=info)
    assert np.max(np.abs(np.asarray(uks) - pulse)) <= 1e-14
    o = nr.evaluate(_qubit_case(), ens, np.arcsin(pulse / 0.2), want_grad=False)
    assert info['member_losses'].shape == (1, 64) and np.max(np.abs(info['member_losses'][0] - o['member_loss'])) <= S_RTOL
    assert abs(info['loss'][0] - o['loss']) <= S_RTOL and abs(info['loss'][0] - np.mean(o['member_loss'])) <= S_RTOL
    assert fr.swapped_apart(list(o['member_loss'][:8]), floor=1e-9)
