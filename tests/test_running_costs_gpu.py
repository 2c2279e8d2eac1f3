"""Open-system running costs on the GPU (HipEngine(running_costs=...), qoc_create_open_costs, the COSTS instances of csrc/qoc_lindblad.h) against
tests/running_cost_reference.py, for one and three control sets: the evaluation scalars, the gradient, get_expectations(), the members' reg_state and
the final density operators on the smallest shapes at which each code path can go wrong; the closed limit against the oracle's forbidden levels;
bit identity (two evaluations; n_obs = 0 against the engines without the term); the device loops; every refusal of the library by its message; and
Grape(running_costs=...) end to end on examples/guarded_transmon_under_decay.py at a reduced size.

Tolerances: S_RTOL, G_RTOL and LOOP_ATOL as tests/test_open_system_gpu.py imports and uses them."""
import contextlib
import functools
import os
import sys
import types

import numpy as np
import pytest

from oracle import grape_oracle as go
from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import open_system
from quantum_optimal_control.helper_functions import transfer as tf
from tests import open_fleet_reference as ofr
from tests import running_cost_reference as rc
from tests.test_adam_tail import LOOP_ATOL, _choose_target
from tests.test_hip_parity import G_RTOL, S_RTOL
from tests.test_open_system import bases_of, open_case
from tests.test_running_costs import FORBID, dense_observable

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
P = hip_engine
KEYS = ('loss', 'reg_loss', 'unitary_scale', 'grad_squared')


def costs_of(kind, n):
    if kind == 'mixed':            # ONE dense complex Hermitian observable under both powers (the conjugation convention), and a projector
        O = dense_observable(n, n)
        return [open_system.observable_cost(O, 1.5, 2), open_system.observable_cost(O, -0.6, 1), open_system.subspace_cost(n, [n - 1], 0.8, 1)]
    if kind == 'dense1':
        return [open_system.observable_cost(dense_observable(n, n), 2.5, 2)]
    if kind == 'two':
        return [open_system.observable_cost(dense_observable(n, n), 3.0, 2), open_system.subspace_cost(n, range(n // 2, n), 1.2, 1)]
    if kind == 'sixteen':          # the limit on L: every level twice under different powers, then dense observables
        out = [open_system.level_cost(n, l % n, 0.5 + 0.1 * l, 1 + l % 2) for l in range(2 * n)]
        return out + [open_system.observable_cost(dense_observable(n, 40 + l), 0.3 * (l + 1), 2 - l % 2) for l in range(16 - 2 * n)]
    raise KeyError(kind)


# name: (n, k, m, steps, (T, s), c, state_transfer, costs) -- and what the row guards
ROWS = {
    'n3_m2': (3, 1, 2, 12, (4, 0), 1, False, 'mixed'),          # pairs (0,0), (0,1), (1,1): the diagonal test on the pair index, an untouched off-diagonal pair
    'n17': (17, 1, 1, 4, (4, 0), 2, False, 'dense1'),           # 289 elements: the second owned element of a thread is only partly populated
    'n32_c5': (32, 2, 2, 3, (5, 1), 5, False, 'two'),           # all four owned elements; dynamic LDS past 64 KiB in the new instances
    'n4_m4_L16': (4, 2, 4, 5, (6, 1), 2, False, 'sixteen'),     # ten pairs, and the limit on L
    'state': (5, 2, 2, 9, (8, 0), 1, True, 'mixed'),            # state-transfer mode
    'unitary_u0': (4, 2, 3, 7, (14, 1), 2, False, 'two'),       # U0 != I: the tau = 0 term from Psi0 = U0 V
    'scaling2': (4, 2, 2, 6, (6, 2), 2, False, 'mixed'),        # four sub-steps: one source per slice
}


@functools.lru_cache(maxsize=None)
def system(name):
    n, k, m, steps, taylor, c, st, kind = ROWS[name]
    sp, ops = open_case(n, k, m, steps, taylor, c, seed=60 + list(ROWS).index(name), state_transfer=st)
    return sp, ops, costs_of(kind, n)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference at the row's three bases: computed once, shared by every test that needs it."""
    sp, ops, costs = system(name)
    return [rc.evaluate(sp, ops, costs, b) for b in bases_of(sp)]


def make_engine(sp, ops, costs, n_seeds=1, **kw):
    return P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, state_transfer=sp.state_transfer,
                       reg_coeffs=sp.reg_coeffs, one_minus_gauss=sp.one_minus_gauss, n_seeds=n_seeds, collapse_ops=ops, running_costs=costs, **kw)


def assert_gradient(tag, got, ref):
    gmax, err = float(np.max(np.abs(ref))), float(np.max(np.abs(got - ref)))
    print('%s: max gradient error %.3e, largest entry %.3e' % (tag, err, gmax))
    assert err <= G_RTOL * max(gmax, 1e-3), (tag, err, gmax)


def assert_scalar(tag, got, want):
    print('%s: engine %.17g reference %.17g' % (tag, got, want))
    assert abs(got - want) <= S_RTOL * max(1.0, abs(want)), (tag, got, want)


# ---- 1. parity with the reference -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('G', [1, 3])
@pytest.mark.parametrize('name', list(ROWS))
def test_parity_with_the_reference(name, G):
    (sp, ops, costs), refs = system(name), reference(name)
    bases = np.stack(bases_of(sp)[:G] if G > 1 else bases_of(sp)[1:2])
    refs = refs[:G] if G > 1 else refs[1:2]
    n, k, m, steps, taylor, c, st, kind = ROWS[name]
    L = len(costs)
    eng = make_engine(sp, ops, costs, G)
    try:
        plan = eng.plan
        assert (plan['path'], plan['collapse'], plan['pairs'], plan['running_costs']) == ('lindblad', str(c), str(m * (m + 1) // 2), str(L)), plan
        assert list(plan)[-1] == 'running_costs'
        if name == 'n32_c5':
            assert int(plan['lds']) > 140 * 1024
        if name == 'n4_m4_L16':
            assert L == 16
        eng.set_base(bases)
        r = eng.evaluate()
        x, ms, rho = eng.get_expectations(), eng.member_scalars(), eng.get_final_density()
        assert x.shape == (G, steps + 1, L, m) and ms['reg_state'].shape == (G, 1) and rho.shape == (G, m, m, n, n)
        for g, o in enumerate(refs):
            for key in KEYS:
                assert_scalar('%s %s[%d]' % (name, key, g), r[key][g], o[key])
            assert_gradient('%s grad[%d]' % (name, g), r['grad'][g], o['grad'])
            assert_scalar('%s reg_state[%d]' % (name, g), ms['reg_state'][g, 0], o['reg_state'])
            assert_scalar('%s member loss[%d]' % (name, g), ms['loss'][g, 0], o['loss'])
            print('%s: max |x - reference| %.3e of %.3e' % (name, np.max(np.abs(x[g] - o['expectations'])), np.max(np.abs(o['expectations']))))
            assert np.max(np.abs(x[g] - o['expectations'])) <= S_RTOL * max(1.0, np.max(np.abs(o['expectations'])))
            assert np.max(np.abs(rho[g] - o['rho_final'])) <= S_RTOL
            assert abs(o['reg_state']) > 1e-3                                       # (the term is visible in reg_loss)
    finally:
        eng.close()


# ---- 2. the member rows: a fleet with rate scales, a line and a risk -------------------------------------------------------------------------------

F, R, E, Q, SAMPLES = 2, 2, 2, 1, 4


@functools.lru_cache(maxsize=None)
def fleet_case():
    p = ofr.problem(3, 2, 6, 2, 2, regs={'dwdt': 0.05, 'amplitude': 0.1})
    fl = ofr.make_fleet(p, F, E, Q, risk=20.0)
    T = tf.hold(6, SAMPLES).matrix
    costs = costs_of('mixed', 3)
    xs = np.random.default_rng(77).normal(0.0, 0.7, size=(F * R, 2, SAMPLES))
    want = [rc.evaluate_members(p, None, fl.device(f), costs, xs[g], T=T, beta=float(fl.risk)) for g, (f, _) in enumerate(ofr.control_sets(F, R))]
    return p, fl, T, costs, xs, want


def fleet_engine(p, fl, T, costs):
    sp = ofr.engine_system(p)
    return P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, p['maxA'], sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, state_transfer=sp.state_transfer,
                       reg_coeffs=p['reg_coeffs'], n_seeds=F * R, transfer=T, fleet=fl, running_costs=costs)


def test_fleet_with_rate_scales_a_line_and_a_risk():
    """The member-row instances, and the glue reading the members' reg_state: the tilt's costs c_e = loss_e + R_e, reg_state = sum_e pi_e R_e."""
    p, fl, T, costs, xs, want = fleet_case()
    eng = fleet_engine(p, fl, T, costs)
    try:
        plan = eng.plan
        assert (plan['path'], plan['devices'], plan['members'], plan['samples'], plan['running_costs']) == ('lindblad', str(F), str(E), str(SAMPLES), '3'), plan
        eng.set_base(xs)
        r = eng.evaluate()
        ms, pi, x, rho = eng.member_scalars(), eng.member_weights(), eng.get_expectations(), eng.get_final_density()
        for g, o in enumerate(want):
            for key in KEYS:
                assert_scalar('fleet %s[%d]' % (key, g), r[key][g], o[key])
            assert_gradient('fleet grad[%d]' % g, r['grad'][g], o['grad'])
            print('members of set %d: reg_state %s reference %s, weights %s reference %s' % (g, ms['reg_state'][g], o['member_reg_state'], pi[g], o['weights']))
            assert np.max(np.abs(ms['reg_state'][g] - o['member_reg_state'])) <= S_RTOL * max(1.0, np.max(np.abs(o['member_reg_state'])))
            assert np.max(np.abs(ms['loss'][g] - o['member_loss'])) <= S_RTOL and np.max(np.abs(pi[g] - o['weights'])) <= S_RTOL
            assert np.max(np.abs(x[g] - o['expectations'])) <= S_RTOL and np.max(np.abs(rho[g] - o['rho_final'])) <= S_RTOL
            assert abs(o['member_reg_state'][0] - o['member_reg_state'][1]) > 1e-6 and abs(o['weights'][0] - fl.weights[0]) > 1e-3
        again = eng.evaluate()
        for key in KEYS + ('grad',):
            np.testing.assert_array_equal(r[key], again[key], err_msg=key)
    finally:
        eng.close()


# ---- 3. the closed limit, determinism, n_obs = 0 --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('state_transfer', [False, True])
def test_closed_limit_against_the_oracle_with_forbidden_levels(state_transfer):
    """No collapse operator, O = |l><l|, power 2: the gradient in both modes, reg_loss in state transfer and, in unitary mode (U0 != I), without the
    tau = 0 terms of either side."""
    m, taylor, theirs = (2, (16, 0), (17, 0)) if state_transfer else (3, (14, 2), (14, 2))
    sp, _ = open_case(4, 2, m, 7, taylor, 0, seed=2, state_transfer=state_transfer)
    oracle_sp, _ = open_case(4, 2, m, 7, theirs, 0, seed=2, state_transfer=state_transfer, reg_coeffs=FORBID)
    pairs = list(zip(FORBID['forbidden_coeff_list'], FORBID['states_forbidden_list']))
    costs = [open_system.level_cost(4, s, a) for a, s in pairs]
    bases = bases_of(sp)
    eng = make_engine(sp, [], costs, 3)
    try:
        assert eng.plan['collapse'] == '0' and eng.plan['running_costs'] == '2', eng.plan
        eng.set_base(np.stack(bases))
        r, x = eng.evaluate(), eng.get_expectations()
        for g, b in enumerate(bases):
            o = go.evaluate(oracle_sp, b)
            assert_scalar('closed limit loss[%d]' % g, r['loss'][g], o['loss'])
            assert_gradient('closed limit grad[%d]' % g, r['grad'][g], o['grad'])
            mine, want = r['reg_loss'][g], o['reg_loss']
            if not state_transfer:
                mine -= rc.cost_value(costs, x[g, :1], sp.steps)
                want -= sum(a / sp.steps * 0.5 * np.sum(np.abs(oracle_sp.V[s, :]) ** 4) for a, s in pairs)
            assert_scalar('closed limit reg_loss[%d]' % g, mine, want)
            assert o['reg_loss'] - o['loss'] > 1e-4
    finally:
        eng.close()


@pytest.mark.parametrize('name', ['n32_c5', 'n4_m4_L16'])
def test_two_evaluations_are_bit_identical(name):
    sp, ops, costs = system(name)
    eng = make_engine(sp, ops, costs, 3)
    try:
        eng.set_base(np.stack(bases_of(sp)))
        a, xa, ma = eng.evaluate(), eng.get_expectations(), eng.member_scalars()
        b = eng.evaluate()
        for key in KEYS + ('grad',):
            assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(xa, eng.get_expectations()) and np.array_equal(ma['reg_state'], eng.member_scalars()['reg_state'])
    finally:
        eng.close()


def three_iterations(eng, bases):
    """Every read-back at the start, after three iterations of the device Adam loop, and of one evaluation where they ended."""
    eng.set_base(bases)
    first = eng.evaluate()
    out = {'first_' + key: first[key] for key in KEYS + ('grad',)}
    out.update(first_rho=eng.get_final_density(), first_pop=eng.get_populations())
    eng.iterate(eng.adam_params(rate=0.02, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=100, poll_every=100), 3)
    s = eng.scalars()
    out.update({'loop_' + key: s[key] for key in KEYS + ('iterations', 'done')})
    out.update(base=eng.get_base(), uks=eng.get_uks(evaluated=True))
    r = eng.evaluate()
    out.update({key: r[key] for key in KEYS + ('grad',)})
    out.update(rho=eng.get_final_density(), pop=eng.get_populations())
    return out


@pytest.mark.parametrize('kind', ['plain', 'ensemble'])
def test_no_observable_is_the_engine_without_the_term(kind):
    """qoc_create_open_costs with n_obs = 0 against the engine of qoc_create_open (plain: bit for bit that of qoc_create_open_fleet with every glue pointer
    NULL, tests/test_open_fleet_gpu.py) and of qoc_create_open_fleet (an ensemble with rate scales): every read-back, also after three Adam iterations."""
    if kind == 'plain':
        sp, ops, _ = system('unitary_u0')
        bases = np.stack(bases_of(sp))
        make = lambda costs: P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, reg_coeffs={}, n_seeds=3,
                                         collapse_ops=ops, running_costs=costs)
    else:
        p, fl, _, _, _, _ = fleet_case()
        sp = ofr.engine_system(p)
        bases = np.random.default_rng(78).normal(0.0, 0.7, size=(3, 2, 6))
        make = lambda costs: P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, p['maxA'], sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, reg_coeffs=p['reg_coeffs'],
                                         n_seeds=3, ensemble=fl.device(1), running_costs=costs)
    out = []
    for costs in (None, []):
        eng = make(costs)
        try:
            assert 'running_costs' not in eng.plan and eng.n_costs == 0
            out.append(three_iterations(eng, bases))
            if kind == 'ensemble':
                out[-1].update(member_loss=eng.member_scalars()['loss'], member_reg=eng.member_scalars()['reg_state'], member_rho=eng.member_final_density())
                assert np.all(out[-1]['member_reg'] == 0.0)
            with pytest.raises(P.QocError, match='status -4'):
                eng.get_expectations()
        finally:
            eng.close()
    assert list(out[0]['loop_iterations']) == [3, 3, 3]
    for key, val in out[0].items():
        np.testing.assert_array_equal(out[1][key], val, err_msg=key)


# ---- 4. the loops ---------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _loop_reference():
    sp, ops, costs = system('scaling2')
    bases = bases_of(sp)
    max_it = 11                                                              # (poll every 5: never a divisor)
    conv = dict(rate=0.02, max_iterations=max_it, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0)
    free = [rc.run_adam(sp, ops, costs, conv, b) for b in bases]
    target, stops = _choose_target([r['history'] for r in free], max_it)
    conv = dict(conv, conv_target=target)
    refs = [rc.run_adam(sp, ops, costs, conv, b) if s < max_it else r for b, r, s in zip(bases, free, stops)]
    assert [r['iterations'] for r in refs] == stops and len(set(stops)) >= 2
    return sp, ops, costs, bases, conv, refs, stops


def test_device_adam_loop_against_the_reference():
    """qoc_run_adam with control sets that stop at different iterations inside one polling burst: the steps follow the gradient of reg_loss, the stop
    rule reads the loss; a finished set's read-backs stay those of its last evaluation."""
    sp, ops, costs, bases, conv, refs, stops = _loop_reference()
    eng = make_engine(sp, ops, costs, 3)
    try:
        eng.set_base(np.stack(bases))
        its = eng.run_adam(eng.adam_params(poll_every=5, **conv))
        assert list(its) == stops
        s = eng.scalars()
        assert list(s['iterations']) == stops and list(s['done']) == [1, 1, 1]
        base, rho, x, ms = eng.get_base(), eng.get_final_density(), eng.get_expectations(), eng.member_scalars()
        for g, ref in enumerate(refs):
            print('set %d: %d iterations, max |base - reference| %.3e' % (g, stops[g], np.max(np.abs(base[g] - ref['base']))))
            np.testing.assert_allclose(base[g], ref['base'], rtol=0, atol=LOOP_ATOL)
            for key in KEYS:
                assert abs(s[key][g] - ref['last'][key]) <= LOOP_ATOL * max(1.0, abs(ref['last'][key])), (key, g)
            np.testing.assert_allclose(rho[g], ref['last']['rho_final'], rtol=0, atol=LOOP_ATOL)
            np.testing.assert_allclose(x[g], ref['last']['expectations'], rtol=0, atol=LOOP_ATOL)
            assert abs(ms['reg_state'][g, 0] - ref['last']['reg_state']) <= LOOP_ATOL
    finally:
        eng.close()


def test_lbfgs_iterations_lower_reg_loss():
    sp, ops, costs = system('scaling2')
    bases = np.stack(bases_of(sp))
    start = reference('scaling2')
    eng = make_engine(sp, ops, costs, 3)
    try:
        eng.set_base(bases)
        its = eng.run_lbfgs(eng.lbfgs_params(conv_target=-1.0, min_grad=-1.0, max_iterations=6, poll_every=4))
        end, r = eng.get_base(), eng.evaluate()
        for g in range(3):
            o = rc.evaluate(sp, ops, costs, end[g], want_grad=False)
            print('set %d: %d iterations, reg_loss %.17g from %.17g (reference at the end point %.17g)' % (g, its[g], r['reg_loss'][g], start[g]['reg_loss'], o['reg_loss']))
            assert int(its[g]) == 6 and r['reg_loss'][g] < start[g]['reg_loss']
            assert_scalar('lbfgs reg_loss[%d]' % g, r['reg_loss'][g], o['reg_loss'])
    finally:
        eng.close()


# ---- 5. refusals of the library -------------------------------------------------------------------------------------------------------------------

ARGS = ('cfg', 'dc', 'rc', 'ens', 'fl', 'tr', 'mp', 'Hs', 'U0', 'V', 'W', 'maxA', 'omg', 'out')
W = 'qoc_create_open_costs: '


@contextlib.contextmanager
def tampered(change):
    """Lets `change(a)` alter what HipEngine hands to qoc_create_open_costs, so that what the Python layer would refuse itself reaches the library
    (tests/test_open_fleet_gpu.py: tampered)."""
    lib = P.load_library()
    real = lib.qoc_create_open_costs

    def call(*args):
        a = types.SimpleNamespace(drop=(), **{name: getattr(arg, '_obj', arg) for name, arg in zip(ARGS, args)})
        change(a)
        return real(*[None if name in a.drop else arg for name, arg in zip(ARGS, args)])
    lib.qoc_create_open_costs = call
    try:
        yield
    finally:
        lib.qoc_create_open_costs = real


def _set(obj, **kw):
    for key, v in kw.items():
        setattr(obj, key, v)


def _poke(arr, idx, v):
    arr[int(idx)] = v


C_REFUSALS = [
    # what qoc_create_open_fleet refuses keeps its meaning
    ('forbidden', 'plain', lambda a: _set(a.cfg, n_forbidden=1), W + 'forbidden levels are not available under a master equation'),
    ('speed_up', 'plain', lambda a: _set(a.cfg, has_speed_up=1), W + 'the speed_up regulariser'),
    ('forbid_dressed', 'plain', lambda a: _set(a.cfg, forbid_dressed=1), W + 'forbid_dressed'),
    ('exact', 'plain', lambda a: _set(a.cfg, gradient=1), W + 'the exact gradient'),
    ('n33', 'plain', lambda a: _set(a.cfg, n=33), W + r'n = 33 \(1 .. 32 levels\)'),
    ('c9', 'plain', lambda a: _set(a.dc, n_collapse=9), W + r'n_collapse = 9 \(at most 8'),
    ('scale_negative', 'fleet', lambda a: _poke(a.dc.rate_scales, 3, -0.5), W + r'rate_scales\[0\]\[1\]\[1\] is -0.5 \(finite, >= 0\)'),
    ('uneven', 'fleet', lambda a: _set(a.cfg, n_seeds=5), W + 'n_seeds = 5 is no multiple of devices = 2'),
    ('bad_weight', 'fleet', lambda a: _poke(a.ens.weights, 1, -0.25), W + 'weight 1 is -0.25'),
    ('T_nan', 'fleet', lambda a: _poke(a.tr.T, 2 * SAMPLES + 1, float('nan')), W + r'T\[2\]\[1\] is not finite'),
    ('null_cfg', 'plain', lambda a: _set(a, drop=('cfg',)), W + 'null argument'),
    ('null_decay', 'plain', lambda a: _set(a, drop=('dc',)), W + 'null argument'),
    # the costs
    ('L17', 'plain', lambda a: _set(a.rc, n_obs=17), W + r'n_obs = 17 \(0 .. 16 running costs\)'),
    ('L_negative', 'plain', lambda a: _set(a.rc, n_obs=-1), W + r'n_obs = -1 \(0 .. 16 running costs\)'),
    ('null_O', 'plain', lambda a: _set(a.rc, O=None), W + r'n_obs = 3 with its observables, coefficients and powers \(a null array\)'),
    ('null_coeffs', 'fleet', lambda a: _set(a.rc, coeffs=None), W + r'n_obs = 3 with its observables, coefficients and powers \(a null array\)'),
    ('null_powers', 'plain', lambda a: _set(a.rc, powers=None), W + r'n_obs = 3 with its observables, coefficients and powers \(a null array\)'),
    ('power3', 'plain', lambda a: _poke(a.rc.powers, 1, 3), W + r'powers\[1\] = 3 \(1 or 2\)'),
    ('power0', 'fleet', lambda a: _poke(a.rc.powers, 2, 0), W + r'powers\[2\] = 0 \(1 or 2\)'),
    ('coeff_nan', 'plain', lambda a: _poke(a.rc.coeffs, 0, float('nan')), W + r'coeffs\[0\] is not finite'),
    ('coeff_inf', 'plain', lambda a: _poke(a.rc.coeffs, 2, float('inf')), W + r'coeffs\[2\] is not finite'),
    ('O_nan', 'plain', lambda a: _poke(a.rc.O, 2 * 9 + 5, float('nan')), W + 'observable 1 is not finite'),
    ('O_inf', 'fleet', lambda a: _poke(a.rc.O, 2 * 2 * 9 + 17, float('-inf')), W + 'observable 2 is not finite'),
]


def refusal_engine(kind):
    """The engine a row of C_REFUSALS is made with (n = 3, three costs), from fresh copies of every table the change may write into."""
    if kind == 'fleet':
        p, fl, T, _, _, _ = fleet_case()
        return fleet_engine(p, ofr.make_fleet(p, F, E, Q, risk=20.0), T.copy(), costs_of('mixed', 3))
    sp, ops, _ = system('n3_m2')
    return make_engine(sp, ops, costs_of('mixed', 3), 2)


@pytest.mark.parametrize('name,kind,change,msg', C_REFUSALS, ids=[row[0] for row in C_REFUSALS])
def test_the_library_refuses_by_message(name, kind, change, msg):
    with tampered(change):
        with pytest.raises(P.QocError, match=msg) as err:
            refusal_engine(kind).close()
    assert 'status -1' in str(err.value)


def test_a_null_costs_pointer_is_no_cost():
    with tampered(lambda a: _set(a, drop=('rc',))):
        eng = refusal_engine('plain')
    try:
        assert 'running_costs' not in eng.plan and eng.plan['path'] == 'lindblad'
    finally:
        eng.close()


def test_get_expectations_refuses_every_other_engine():
    sp, ops, costs = system('n3_m2')
    plain = P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, reg_coeffs={}, collapse_ops=ops)
    closed = P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, reg_coeffs={})
    with_costs = make_engine(sp, ops, costs, 1)
    try:
        for e in (plain, closed):
            e.n_costs = 1
            e.set_base(sp.base0[None])
            e.evaluate()
            with pytest.raises(P.QocError, match='status -4'):
                e.get_expectations()
        with pytest.raises(P.QocError, match='nothing evaluated yet'):
            with_costs.get_expectations()
    finally:
        plain.close()
        closed.close()
        with_costs.close()


# ---- 6. Grape, the example ------------------------------------------------------------------------------------------------------------------------

def test_grape_on_the_guarded_transmon_at_a_reduced_size():
    """examples/guarded_transmon_under_decay.py with 12 slices and 25 iterations: the guarded call runs the costs (its pulse is not the unguarded one),
    and what method='EVOLVE' reports of it -- the infidelity and the guard level's population at every slice boundary -- is the reference's at that
    pulse (1e-10, as tests/test_open_system_gpu.py: test_grape_evolve_agrees_with_the_reference bounds a scored pulse)."""
    import guarded_transmon_under_decay as ex
    steps = 12
    plain, guarded = ex.optimise(False, steps, 25), ex.optimise(True, steps, 25)
    assert plain.shape == guarded.shape == (2, steps) and np.max(np.abs(plain - guarded)) > 1e-6
    H0, Hops, _, U, ops = ex.problem()
    T, s = open_system.choose_taylor(H0, Hops, ex.MAXA, ops, ex.TOTAL_TIME / steps, steps, 1e-4)
    for uks in (plain, guarded):
        loss, x = ex.score(uks)
        assert x.shape == (steps + 1, 1, 2)
        np.random.seed(0)
        sp = go.OracleSystem(H0, Hops, U, ex.TOTAL_TIME, steps, [0, 1], maxA=ex.MAXA, initial_guess=uks, Taylor_terms=[T, s], reg_coeffs={})
        o = rc.evaluate(sp, ops, [open_system.level_cost(ex.LEVELS, ex.GUARD, 0.0)], sp.base0, want_grad=False)
        print('infidelity %.12g (reference %.12g), largest guard population %.6e (reference %.6e)' % (loss, o['loss'], np.max(x), np.max(o['expectations'])))
        assert abs(loss - o['loss']) <= 1e-10 and np.max(np.abs(x - o['expectations'])) <= 1e-10
        assert o['reg_state'] == 0.0 and np.all(x[0] == 0.0) and np.max(x) > 0.0
    out = ex.main(steps, 5, quiet=True)
    assert len(out) == 2 and all(np.isfinite(v) for row in out for v in row)
