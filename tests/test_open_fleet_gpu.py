"""Open-system ensembles and fleets on the GPU (qoc_create_open_fleet) against tests/open_fleet_reference.py: every member of every
device is an open problem with its own drift, amplitude scales and decay rates.

  1. parity at n = 3, m = 2 (3 pairs), k = 2, c = 2, 6 slices, (T, s) = (6, 1), F = 2, R = 2, E = 3, q = 1, every table entry distinct and one rate
     scale 0, in both modes and once with pulse regularisers and bandpass;
  2. ownership edges: n = 17 (a thread owns two elements), n = 32 with c = 5 (the LDS limit, with scaled D), c = 0 (the closed limit);
  3. bit identity: all-NULL glue with scales of 1 against qoc_create_open, F = 1 against the ensemble, a fleet against one ensemble engine per device,
     two evaluations of one engine;
  4. composition with a risk, a line (P < steps), a control map (r != k), and the three on a fleet;
  5. the loops: Adam with devices that stop at different iterations, L-BFGS, method='EVOLVE' as the scan of one pulse;
  6. refusals of the library by message; two such engines and a plain open engine alive at once;
  7. Grape(robust=...) and Grape(fleet=...) with decay against plain Grape(collapse_ops=...) calls, and the example.

Tolerances: S_RTOL, G_RTOL and LOOP_ATOL as tests/test_open_system_gpu.py imports and uses them."""
import contextlib
import ctypes as C
import functools
import io
import os
import sys
import types

import numpy as np
import pytest

from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import fleet as fl_mod
from quantum_optimal_control.helper_functions import robust as rb
from quantum_optimal_control.helper_functions import transfer as tf
from tests import control_map_reference as ref
from tests import lbfgs_reference as lb
from tests import open_fleet_reference as ofr
from tests.test_adam_tail import LOOP_ATOL, _choose_target
from tests.test_hip_parity import G_RTOL, S_RTOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = hip_engine
F, R, E, Q = 2, 2, 3, 1
KEYS = ('loss', 'reg_loss', 'grad_squared', 'unitary_scale')
REGS = {'amplitude': 0.3, 'dwdt': 0.02, 'd2wdt2': 0.001, 'bandpass': 0.1, 'band': [0.4, 1.0]}


# ---- engines, start points, comparisons ---------------------------------------------------------------------------------------------------------

def make_engine(p, n_sets, ens=None, fl=None, T=None, cm=None):
    """An open fleet engine (fl: a Fleet with decay) or, fl None, the open ensemble engine of `ens`."""
    sp = ofr.engine_system(p)
    assert [sp.exp_terms, sp.scaling] == list(p['Taylor_terms'])
    return P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, p['maxA'], sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, state_transfer=sp.state_transfer,
                       reg_coeffs=p['reg_coeffs'], n_seeds=n_sets, ensemble=ens, transfer=T, control_map=cm, fleet=fl)


def start_points(k, width, count, seed=0):
    return np.random.default_rng(6000 + width + seed).normal(0.0, 0.7, size=(count, k, width))


def assert_scalars(tag, r, g, o, keys=KEYS):
    for key in keys:
        print('%s %s[%d]: engine %.17g reference %.17g' % (tag, key, g, r[key][g], o[key]))
        assert abs(r[key][g] - o[key]) <= S_RTOL * max(1.0, abs(o[key])), (tag, key, g, r[key][g], o[key])


def assert_gradient(tag, got, want):
    gmax, err = float(np.max(np.abs(want))), float(np.max(np.abs(got - want)))
    print('%s: max gradient error %.3e, largest entry %.3e' % (tag, err, gmax))
    assert err <= G_RTOL * max(gmax, 1e-3), (tag, err, gmax)


def assert_set(tag, eng, r, ms, rho_m, rho0, pop, g, o):
    """Everything the engine reports of control set g against its expectation o."""
    assert_scalars(tag, r, g, o)
    assert_gradient('%s grad[%d]' % (tag, g), r['grad'][g], o['grad'])
    assert np.max(np.abs(ms['loss'][g] - o['member_loss'])) <= S_RTOL * max(1.0, np.max(np.abs(o['member_loss']))), (tag, g, ms['loss'][g], o['member_loss'])
    assert np.all(ms['reg_state'][g] == 0.0)
    assert np.max(np.abs(rho_m[g] - o['member_rho'])) <= S_RTOL, (tag, g)
    assert np.max(np.abs(rho0[g] - o['rho_final'])) <= S_RTOL and np.max(np.abs(pop[g] - o['populations'])) <= S_RTOL, (tag, g)


def read_all(eng):
    return eng.evaluate(), eng.member_scalars(), eng.member_final_density(), eng.get_final_density(), eng.get_populations()


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------------------

PARITY = {'unitary': (False, None), 'state': (True, None), 'regs': (False, REGS)}


@functools.lru_cache(maxsize=None)
def parity_reference(name):
    """(problem, fleet, start points, expectation of every control set): computed once, shared.  Checked here, on the CPU: every entry of the three
    tables is distinct, one rate scale is 0, and at ONE start point the devices' expected losses, gradients and member-0 densities lie more than 1e-6
    apart -- a kernel that reads another device's row of drifts or of rate scales cannot pass."""
    st, regs = PARITY[name]
    p = ofr.problem(3, 2, 6, 2, 2, state_transfer=st, taylor=(6, 1), regs=regs)
    fl = ofr.make_fleet(p, F, E, Q)
    flat = np.concatenate([fl.rate_scales.reshape(-1), fl.amp_scales.reshape(-1), fl.offsets.reshape(-1)])
    assert len(set(flat)) == flat.size and np.count_nonzero(fl.rate_scales == 0.0) == 1
    xs = start_points(2, 6, F * R)
    at_one = [ofr.evaluate_device(p, None, fl, f, xs[1]) for f in range(F)]
    assert ofr.swapped_apart([o['loss'] for o in at_one]) and ofr.swapped_apart([o['grad'] for o in at_one])
    assert ofr.swapped_apart([o['rho_final'].view(np.float64) for o in at_one]) and ofr.swapped_apart([o['member_loss'] for o in at_one])
    return p, fl, xs, [ofr.evaluate_device(p, None, fl, f, xs[g]) for g, (f, _) in enumerate(ofr.control_sets(F, R))]


@pytest.mark.parametrize('name', list(PARITY))
def test_every_member_runs_its_own_open_problem(name):
    p, fl, xs, want = parity_reference(name)
    eng = make_engine(p, F * R, fl=fl)
    try:
        plan = eng.plan
        assert (plan['path'], plan['collapse'], plan['pairs'], plan['devices'], plan['members'], plan['perturbations'], plan['gradient']) == \
            ('lindblad', '2', '3', str(F), str(E), str(Q), 'first_order'), plan
        assert eng.path == P.PATH_LINDBLAD and eng.open_system and eng.devices == F and eng.members == E
        eng.set_base(xs)
        r, ms, rho_m, rho0, pop = read_all(eng)
        assert rho_m.shape == (F * R, E, 2, 2, 3, 3) and rho0.shape == (F * R, 2, 2, 3, 3) and pop.shape == (F * R, 7, 3, 2)
        for g, o in enumerate(want):
            assert_set(name, eng, r, ms, rho_m, rho0, pop, g, o)
            assert np.array_equal(rho_m[g, :, 1, 0], np.conj(np.swapaxes(rho_m[g, :, 0, 1], -1, -2)))
        for call in (eng.get_final_unitary, eng.get_inter_vecs, eng.member_final_unitary):
            with pytest.raises(P.QocError, match='status -4'):
                call()
    finally:
        eng.close()


# ---- 2. ownership edges ---------------------------------------------------------------------------------------------------------------------------

EDGES = {                                                  # name: (n, k, m, steps, (T, s), c)
    'n17': (17, 1, 1, 2, (4, 0), 1),                       # 289 elements: a thread owns two
    'n32_c5': (32, 1, 1, 2, (4, 1), 5),                    # the largest LDS footprint the size rule allows, every D_j scaled on its way in
    'c0': (4, 2, 2, 5, (10, 1), 0),                        # no collapse operator: the closed limit, through the member tables
}


@pytest.mark.parametrize('name', list(EDGES))
def test_ownership_edges(name):
    n, k, m, steps, taylor, c = EDGES[name]
    p = ofr.problem(n, k, steps, m, c, taylor=taylor, seed=10 + list(EDGES).index(name))
    fl = ofr.make_fleet(p, 1, 2, 1, zero=False)
    ens = fl.device(0)
    xs = start_points(k, steps, 2, seed=n)
    eng = make_engine(p, 2, ens=ens)
    try:
        assert (eng.plan['path'], eng.plan['collapse'], eng.plan['members']) == ('lindblad', str(c), '2') and 'devices' not in eng.plan, eng.plan
        if name == 'n32_c5':
            assert int(eng.plan['lds']) > 140 * 1024
        eng.set_base(xs)
        r, ms, rho_m, rho0, pop = read_all(eng)
        for g in range(2):
            o = ofr.evaluate(p, None, ens, xs[g])
            assert_set(name, eng, r, ms, rho_m, rho0, pop, g, o)
            assert abs(o['member_loss'][0] - o['member_loss'][1]) > 1e-6
            if c == 0:
                assert abs(r['unitary_scale'][g] - 1.0) <= 1e-9
    finally:
        eng.close()


# ---- 3. bit for bit -------------------------------------------------------------------------------------------------------------------------------

LOOP = dict(rate=0.02, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=100, poll_every=100)


def ten_iterations(eng, bases, members=True):
    """Ten iterations of the device Adam loop, then one evaluation where they ended: everything the comparison reads."""
    eng.set_base(bases)
    eng.iterate(eng.adam_params(**LOOP), 10)
    s = eng.scalars()
    out = dict(base=eng.get_base(), uks=eng.get_uks(evaluated=True))
    out.update({'loop_' + key: s[key] for key in KEYS + ('iterations', 'done')})
    r = eng.evaluate()
    out.update({key: r[key] for key in KEYS + ('grad',)})
    out.update(rho=eng.get_final_density(), pop=eng.get_populations())
    if members:
        out.update(member_loss=eng.member_scalars()['loss'], member_rho=eng.member_final_density())
    return out


def raw_open_fleet(p, n_sets, ops, scales):
    """qoc_create_open_fleet through the bare C ABI with ens, fleet, transfer and map all NULL, wrapped as a HipEngine for its read-backs."""
    lib = P.load_library()
    sp = ofr.engine_system(p)
    n, k, m = sp.n, sp.k, sp.m
    cfg = P.QocConfig()
    cfg.n, cfg.k, cfg.steps, cfg.m, cfg.taylor_terms, cfg.scaling, cfg.n_seeds = n, k, sp.steps, m, sp.exp_terms, sp.scaling, n_sets
    cfg.dt, cfg.total_time, cfg.state_transfer = sp.dt, sp.total_time, int(sp.state_transfer)
    rcfg = P.reg_config(p['reg_coeffs'], sp.total_time)
    for name in ('amplitude', 'dwdt', 'd2wdt2', 'bandpass'):
        setattr(cfg, 'has_' + name, rcfg['has_' + name])
        setattr(cfg, 'c_' + name, rcfg['c_' + name])
    cfg.band_lo, cfg.band_hi = rcfg.get('band_lo', 0), rcfg.get('band_hi', 0)
    D = np.ascontiguousarray(np.sqrt(sp.dt) * np.array(ops, dtype=np.complex128))
    dc = P.QocDecay()
    dc.n_collapse, dc.C, dc.rate_scales = len(ops), P._dp(D.view(np.float64)), P._dp(scales)
    arrs = [np.ascontiguousarray(a, dtype=np.complex128) for a in (sp.Hs, sp.U0, sp.V, sp.W)]
    maxA = np.ascontiguousarray(p['maxA'], dtype=np.float64)
    eng = P.HipEngine.__new__(P.HipEngine)
    eng._lib, eng._h = lib, C.c_void_p()
    rc = lib.qoc_create_open_fleet(C.byref(cfg), C.byref(dc), None, None, None, None, *[P._dp(a.view(np.float64)) for a in arrs], P._dp(maxA), None,
                                   C.byref(eng._h))
    assert rc == 0, lib.qoc_last_error().decode()
    eng.n, eng.k, eng.m, eng.steps, eng.n_seeds, eng.samples, eng.members, eng.terms = n, k, m, sp.steps, n_sets, None, 1, k
    buf = C.create_string_buffer(512)
    assert lib.qoc_plan_describe(eng._h, buf, 512) == 0
    eng.plan = dict(kv.split('=', 1) for kv in buf.value.decode().split())
    return eng


@pytest.mark.parametrize('name', ['unitary', 'regs'])
def test_all_null_glue_with_scales_of_one_is_the_plain_open_engine(name):
    p, _, xs, _ = parity_reference(name)
    sp = ofr.engine_system(p)
    plain = P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, p['maxA'], sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, reg_coeffs=p['reg_coeffs'], n_seeds=3,
                        collapse_ops=p['collapse_ops'])
    try:
        want = ten_iterations(plain, xs[:3], members=False)
        line = plain.plan
    finally:
        plain.close()
    for scales in (None, np.ones((1, 1, 2))):
        eng = raw_open_fleet(p, 3, p['collapse_ops'], scales)
        try:
            assert eng.plan['members'] == '1' and {key: v for key, v in eng.plan.items() if key not in ('members', 'perturbations')} == line, (eng.plan, line)
            got = ten_iterations(eng, xs[:3], members=False)
        finally:
            eng.close()
        for key, val in want.items():
            np.testing.assert_array_equal(got[key], val, err_msg=key)


def test_one_device_is_the_open_ensemble_engine():
    p, fl, xs, _ = parity_reference('unitary')
    one = fl_mod.validate(fl_mod.Fleet(fl.operators, fl.offsets[1:2], fl.amp_scales[1:2], weights=fl.weights, collapse_ops=fl.collapse_ops,
                                       rate_scales=fl.rate_scales[1:2]), 3, 2)
    out = []
    for fleet, ens in ((one, None), (None, fl.device(1))):
        eng = make_engine(p, R, ens=ens, fl=fleet)
        try:
            assert ('devices' in eng.plan) == (fleet is not None) and eng.plan['path'] == 'lindblad'
            out.append(ten_iterations(eng, xs[:R]))
        finally:
            eng.close()
    for key, val in out[1].items():
        np.testing.assert_array_equal(out[0][key], val, err_msg=key)


def test_fleet_is_bit_identical_to_the_ensemble_engines_of_its_devices():
    p, fl, xs, _ = parity_reference('regs')
    eng = make_engine(p, F * R, fl=fl)
    try:
        got = ten_iterations(eng, xs)
    finally:
        eng.close()
    assert list(got['loop_iterations']) == [10] * (F * R)
    for f in range(F):
        one = make_engine(p, R, ens=fl.device(f))
        try:
            want = ten_iterations(one, xs[f * R:(f + 1) * R])
        finally:
            one.close()
        for key, val in want.items():
            np.testing.assert_array_equal(got[key][f * R:(f + 1) * R], val, err_msg='%s of device %d' % (key, f))


def test_two_evaluations_are_bit_identical():
    p, fl, xs, _ = parity_reference('regs')
    eng = make_engine(p, F * R, fl=fl)
    try:
        eng.set_base(xs)
        first, rho_a = eng.evaluate(), eng.member_final_density()
        eng.set_base(xs)
        second = eng.evaluate()
        for key in KEYS + ('grad',):
            np.testing.assert_array_equal(first[key], second[key], err_msg=key)
        np.testing.assert_array_equal(rho_a, eng.member_final_density())
    finally:
        eng.close()


# ---- 4. composition -------------------------------------------------------------------------------------------------------------------------------

SAMPLES = 4                                               # hold(6, 4): P < steps
COMPOSITIONS = {                                          # name: (risk, line, map, fleet)
    'risk': (50.0, False, False, False),
    'line': (0.0, True, False, False),
    'control_map': (0.0, False, True, False),
    'risk_line_map_fleet': (50.0, True, True, True),
}


@pytest.mark.parametrize('name', list(COMPOSITIONS))
def test_open_members_compose(name):
    beta, with_line, with_map, with_fleet = COMPOSITIONS[name]
    k, r, steps = 2, 3 if with_map else 2, 6
    p = ofr.problem(3, k, steps, 2, 2, r=r, regs={'dwdt': 0.05, 'amplitude': 0.1})
    fl = ofr.make_fleet(p, F, E, Q, risk=beta)
    cm = ref.make_map(k, r, 3, steps, mix=True, fixed=True) if with_map else None
    T = tf.hold(steps, SAMPLES).matrix if with_line else None
    devs = list(range(F)) if with_fleet else [1]
    sets = ofr.control_sets(len(devs), R)
    xs = start_points(k, SAMPLES if with_line else steps, len(sets), seed=1)
    eng = make_engine(p, len(sets), ens=None if with_fleet else fl.device(1), fl=fl if with_fleet else None, T=T, cm=cm)
    try:
        assert eng.plan['path'] == 'lindblad' and eng.risk == beta and ('terms' in eng.plan) == with_map and ('samples' in eng.plan) == with_line
        assert ('devices' in eng.plan) == with_fleet
        eng.set_base(xs)
        r_, ms, rho_m, rho0, pop = read_all(eng)
        pi = eng.member_weights()
        seen = []
        for g, (f, _) in enumerate(sets):
            o = ofr.evaluate_device(p, cm, fl, devs[f], xs[g], T=T)
            assert_set(name, eng, r_, ms, rho_m, rho0, pop, g, o)
            print('weights[%d]: engine %s reference %s' % (g, pi[g], o['weights']))
            assert np.max(np.abs(pi[g] - o['weights'])) <= S_RTOL, (g, pi[g], o['weights'])
            seen.append(o['weights'])
            if with_line:
                assert np.max(np.abs(eng.get_pulse()[g] - o['pulse'])) <= S_RTOL
            if with_map:
                assert np.max(np.abs(eng.get_coefficients()[g] - o['coefficients'])) <= S_RTOL * max(1.0, np.max(np.abs(o['coefficients'])))
        if beta > 0:
            assert ofr.swapped_apart(seen)
    finally:
        eng.close()


# ---- 5. loops -------------------------------------------------------------------------------------------------------------------------------------

LOOP_MAX = 11


@functools.lru_cache(maxsize=None)
def loop_reference():
    """Two devices of two members from ONE start point, Adam over each device's reference, and a conv_target at which they stop at different
    iterations (tests/test_adam_tail.py: _choose_target)."""
    p = ofr.problem(3, 2, 6, 2, 2, regs={'dwdt': 0.01}, seed=3)
    fl = ofr.make_fleet(p, F, 2, 1, seed=9)
    x0 = start_points(2, 6, 1, seed=3)[0]
    conv = dict(rate=0.1, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=LOOP_MAX)
    at = [lambda x, f=f: ofr.evaluate_device(p, None, fl, f, x) for f in range(F)]
    free = [ofr.run_adam(at[f], x0, conv) for f in range(F)]
    target, stops = _choose_target([run['history'] for run in free], LOOP_MAX, accept=lambda s: len(set(s)) == F and min(s) > 0)
    conv = dict(conv, conv_target=target)
    refs = [ofr.run_adam(at[f], x0, conv) for f in range(F)]
    assert [run['iterations'] for run in refs] == stops
    return p, fl, x0, conv, refs, stops


def test_adam_loop_with_devices_that_stop_at_different_iterations():
    p, fl, x0, conv, refs, stops = loop_reference()
    poll = next(q for q in (5, 4, 7, 3, 6, 9, 8, 13) if all(s % q for s in stops))
    eng = make_engine(p, F, fl=fl)
    try:
        eng.set_base(np.broadcast_to(x0[None], (F,) + x0.shape))
        its = eng.run_adam(eng.adam_params(poll_every=poll, **conv))
        s, base, ms, rho = eng.scalars(), eng.get_base(), eng.member_scalars(), eng.get_final_density()
        print(eng.plan, 'stops', stops, 'poll', poll)
        assert list(its) == stops and list(s['iterations']) == stops and list(s['done']) == [1] * F, (its, stops)
        for f, run in enumerate(refs):
            print('device %d: %d iterations, max |base - reference| %.3e' % (f, stops[f], np.max(np.abs(base[f] - run['base']))))
            np.testing.assert_allclose(base[f], run['base'], rtol=0, atol=LOOP_ATOL)
            for key in KEYS:
                assert abs(s[key][f] - run['last'][key]) <= LOOP_ATOL * max(1.0, abs(run['last'][key])), (key, f)
            # a finished device keeps the read-backs of its last evaluation while the other goes on
            np.testing.assert_allclose(ms['loss'][f], run['last']['member_loss'], rtol=0, atol=LOOP_ATOL)
            np.testing.assert_allclose(rho[f], run['last']['rho_final'], rtol=0, atol=LOOP_ATOL)
    finally:
        eng.close()


def test_lbfgs_loop_runs_every_control_set_on_its_device():
    """run_lbfgs on the whole fleet against tests/lbfgs_reference.py driven by each control set's own device (the reference's gradient is the
    engine's first-order one, so both loops decide on the same numbers): the iteration count, the point it ends at and its reg_loss, which lies below
    the start's.  Checked here, on the CPU: no Armijo decision of the reference is closer to its threshold than 1e-9, and every set accepts a step."""
    p, fl, xs, want = parity_reference('unitary')
    params = dict(conv_target=-1.0, min_grad=-1.0, max_iterations=6)
    eng = make_engine(p, F * R, fl=fl)
    try:
        eng.set_base(xs)
        its = eng.run_lbfgs(eng.lbfgs_params(poll_every=4, **params))
        s, base = eng.scalars(), eng.get_base()
        res = eng.evaluate()
        for g, (f, _) in enumerate(ofr.control_sets(F, R)):
            rec = lb.run(lambda x: ofr.evaluate_device(p, None, fl, f, x), xs[g], params)
            assert all(mg is None or abs(mg) > 1e-9 for mg in rec['margin']) and rec['branch'][1:].count(lb.ACCEPT) >= 1, (g, rec['branch'], rec['margin'])
            o = ofr.evaluate_device(p, None, fl, f, rec['x'], want_grad=False)
            print('set %d: %d iterations (reference %d, %s), reg_loss %.17g from %.17g (reference %.17g), max |base - reference| %.3e'
                  % (g, its[g], rec['state'].iters, rec['branch'], res['reg_loss'][g], want[g]['reg_loss'], o['reg_loss'], np.max(np.abs(base[g] - rec['x']))))
            assert o['reg_loss'] < want[g]['reg_loss']
            assert int(its[g]) == int(s['iterations'][g]) == rec['state'].iters == 6 and int(s['done'][g]) == 1, (g, its, s['iterations'], rec['state'].iters)
            np.testing.assert_allclose(base[g], rec['x'], rtol=0, atol=LOOP_ATOL)
            assert abs(res['reg_loss'][g] - o['reg_loss']) <= LOOP_ATOL * max(1.0, abs(o['reg_loss'])), (g, res['reg_loss'][g], o['reg_loss'])
            assert res['reg_loss'][g] < want[g]['reg_loss'], (g, res['reg_loss'][g], want[g]['reg_loss'])
    finally:
        eng.close()


def _grape(*args, **kw):
    from quantum_optimal_control.main_grape.grape import Grape
    with contextlib.redirect_stdout(io.StringIO()):
        return Grape(*args, save=False, show_plots=False, **kw)


def grape_args(p):
    return (p['H0'], p['Hops'], p['Hnames'], p['U'], p['total_time'], p['steps'], p['states_concerned_list'])


def test_evolve_scans_one_pulse_over_the_devices():
    p, fl, xs, _ = parity_reference('unitary')
    maxA = np.asarray(p['maxA'])
    pulse = maxA[:, None] * np.sin(xs[0])
    uks, rho = _grape(*grape_args(p), U0=p['U0'], reg_coeffs=p['reg_coeffs'], maxA=list(maxA), method='EVOLVE', initial_guess=pulse,
                      Taylor_terms=p['Taylor_terms'], fleet=fl)
    assert uks.shape == (F, 2, 6) and rho.shape == (F, 2, 2, 3, 3) and list(fl.best) == [0] * F and fl.member_losses.shape == (F, E)
    for f in range(F):
        o = ofr.evaluate_device(p, None, fl, f, np.arcsin(pulse / maxA[:, None]), want_grad=False)
        assert np.max(np.abs(uks[f] - pulse)) <= 1e-14
        assert abs(fl.losses[f] - o['loss']) <= S_RTOL * max(1.0, abs(o['loss'])), (f, fl.losses[f], o['loss'])
        assert np.max(np.abs(fl.member_losses[f] - o['member_loss'])) <= S_RTOL and np.max(np.abs(rho[f] - o['rho_final'])) <= S_RTOL


# ---- 6. refusals of the library, engines side by side ---------------------------------------------------------------------------------------------

ARGS = ('cfg', 'dc', 'ens', 'fl', 'tr', 'mp', 'Hs', 'U0', 'V', 'W', 'maxA', 'omg', 'out')


@contextlib.contextmanager
def tampered(change):
    """Lets `change(a)` alter what HipEngine hands to qoc_create_open_fleet, so that what the Python layer would refuse itself reaches the library:
    a.cfg, a.dc, a.ens, a.fl, a.tr and a.mp are the structures (None where the call passes NULL), a.drop names the arguments to pass as NULL."""
    lib = P.load_library()
    real = lib.qoc_create_open_fleet

    def call(*args):
        a = types.SimpleNamespace(drop=(), **{name: getattr(arg, '_obj', arg) for name, arg in zip(ARGS, args)})
        change(a)
        return real(*[None if name in a.drop else arg for name, arg in zip(ARGS, args)])
    lib.qoc_create_open_fleet = call
    try:
        yield
    finally:
        lib.qoc_create_open_fleet = real


def _set(obj, **kw):
    for key, v in kw.items():
        setattr(obj, key, v)


def _poke(arr, idx, v):
    for i in np.atleast_1d(idx):
        arr[int(i)] = v


W = 'qoc_create_open_fleet: '
STEPS, MAP_R, MAP_D = 6, 3, 2                              # the refusal engines: 6 slices; a map of 3 operators of degree 2 on the 2 pulses
# (name, what the engine is made with, the change, the message).  'fleet': the parity fleet (F, E, q, c = 2, 3, 1, 2; k = 2); 'ens': device 1 of it
# as an ensemble; 'line': the fleet behind hold(6, 4); 'map': the fleet behind a map with mix and fixed; 'ens_line': the ensemble behind the line.
C_REFUSALS = [
    # what qoc_create_open refuses
    ('forbidden', 'fleet', lambda a: _set(a.cfg, n_forbidden=1), W + 'forbidden levels'),
    ('speed_up', 'fleet', lambda a: _set(a.cfg, has_speed_up=1), W + 'the speed_up regulariser'),
    ('forbid_dressed', 'fleet', lambda a: _set(a.cfg, forbid_dressed=1), W + 'forbid_dressed'),
    ('exact', 'fleet', lambda a: _set(a.cfg, gradient=1), W + 'the exact gradient'),
    ('time_shards', 'fleet', lambda a: _set(a.cfg, time_shards=2), W + 'an open system cannot be time-sharded'),
    ('generic_path', 'fleet', lambda a: _set(a.cfg, path=P.PATH_GENERIC), W + r'an open system runs on QOC_PATH_LINDBLAD \(or AUTO\), not on path 1'),
    ('small_path', 'fleet', lambda a: _set(a.cfg, path=P.PATH_SMALL), W + r'an open system runs on QOC_PATH_LINDBLAD \(or AUTO\), not on path 5'),
    ('n33', 'fleet', lambda a: _set(a.cfg, n=33), W + r'n = 33 \(1 .. 32 levels\)'),
    ('n0', 'fleet', lambda a: _set(a.cfg, n=0), W + r'n = 0 \(1 .. 32 levels\)'),
    ('c9', 'fleet', lambda a: _set(a.dc, n_collapse=9), W + r'n_collapse = 9 \(at most 8'),
    ('c_negative', 'fleet', lambda a: _set(a.dc, n_collapse=-1), W + r'n_collapse = -1 \(>= 0\) with its operators'),
    ('null_ops', 'fleet', lambda a: _set(a.dc, C=None), W + r'n_collapse = 2 \(>= 0\) with its operators'),
    ('m_above_n', 'fleet', lambda a: _set(a.cfg, m=4), W + r'm = 4 states of interest'),
    ('m0', 'fleet', lambda a: _set(a.cfg, m=0), W + r'm = 0 states of interest'),
    # (the one rule that joins n with decay->n_collapse)
    ('lds', 'fleet', lambda a: (_set(a.cfg, n=32), _set(a.dc, n_collapse=6)), W + r'n = 32 with 6 collapse operators needs \d+ bytes of LDS \(limit 162816\)'),
    ('taylor61', 'fleet', lambda a: _set(a.cfg, taylor_terms=61), W + r'taylor_terms = 61 \(1 .. 60\)'),
    ('taylor0', 'fleet', lambda a: _set(a.cfg, taylor_terms=0), W + r'taylor_terms = 0 \(1 .. 60\)'),
    ('scaling13', 'fleet', lambda a: _set(a.cfg, scaling=13), W + r'scaling = 13 \(0 .. 12\)'),
    ('scaling_negative', 'fleet', lambda a: _set(a.cfg, scaling=-1), W + r'scaling = -1 \(0 .. 12\)'),
    ('op_nan', 'fleet', lambda a: _poke(a.dc.C, 5, float('nan')), W + 'a collapse operator is not finite'),
    # the rate scales
    ('scale_negative', 'fleet', lambda a: _poke(a.dc.rate_scales, 1 * 6 + 2 * 2 + 1, -0.5), W + r'rate_scales\[1\]\[2\]\[1\] is -0.5 \(finite, >= 0\)'),
    ('scale_nan', 'fleet', lambda a: _poke(a.dc.rate_scales, 0 * 6 + 1 * 2 + 0, float('nan')), W + r'rate_scales\[0\]\[1\]\[0\] is nan'),
    ('scale_inf', 'fleet', lambda a: _poke(a.dc.rate_scales, 3, float('inf')), W + r'rate_scales\[0\]\[1\]\[1\] is inf'),
    ('scale_negative_ens', 'ens', lambda a: _poke(a.dc.rate_scales, 2 * 2 + 0, -2.0), W + r'rate_scales\[0\]\[2\]\[0\] is -2 \(finite, >= 0\)'),
    # what qoc_create_fleet refuses about its tables
    ('null_amp_scales', 'fleet', lambda a: _set(a.fl, amp_scales=None), W + r"the fleet's amp_scales are missing"),
    ('null_offsets', 'fleet', lambda a: _set(a.fl, offsets=None), W + r"the fleet's offsets are missing \(n_perturb = 1\)"),
    ('no_devices', 'fleet', lambda a: _set(a.fl, devices=0), W + r'devices = 0 \(>= 1\)'),
    ('no_sets', 'fleet', lambda a: _set(a.cfg, n_seeds=0), W + r'k, n_seeds must be >= 1'),
    ('no_pulses', 'fleet', lambda a: _set(a.cfg, k=0), W + r'k, n_seeds must be >= 1'),
    ('uneven', 'fleet', lambda a: _set(a.cfg, n_seeds=5), W + 'n_seeds = 5 is no multiple of devices = 2'),
    ('amp_nan', 'fleet', lambda a: _poke(a.fl.amp_scales, 1 * 6 + 2 * 2 + 1, float('nan')), W + r'amp_scales\[1\]\[2\]\[1\] is not finite'),
    ('offset_inf', 'fleet', lambda a: _poke(a.fl.offsets, 1 * 3 + 0, float('inf')), W + r'offsets\[1\]\[0\]\[0\] is not finite'),
    ('no_members', 'fleet', lambda a: _set(a.ens, members=0), W + r'members = 0 \(>= 1\), n_perturb = 1 \(>= 0\)'),
    ('perturb_negative', 'fleet', lambda a: _set(a.ens, n_perturb=-1), W + r'members = 3 \(>= 1\), n_perturb = -1 \(>= 0\)'),
    # what qoc_create_ensemble refuses, behind a fleet and on its own
    ('bad_weight', 'fleet', lambda a: _poke(a.ens.weights, 1, -0.25), W + 'weight 1 is -0.25'),
    ('nan_weight_ens', 'ens', lambda a: _poke(a.ens.weights, 2, float('nan')), W + 'weight 2 is nan'),
    ('null_weights', 'fleet', lambda a: _set(a.ens, weights=None), W + 'ensemble arrays missing'),
    ('null_operators', 'fleet', lambda a: _set(a.ens, P=None), W + 'ensemble arrays missing'),
    ('null_amp_scales_ens', 'ens', lambda a: _set(a.ens, amp_scales=None), W + 'ensemble arrays missing'),
    ('null_offsets_ens', 'ens', lambda a: _set(a.ens, offsets=None), W + 'ensemble arrays missing'),
    ('no_members_ens', 'ens', lambda a: _set(a.ens, members=0), W + r'members = 0 \(>= 1\), n_perturb = 1 \(>= 0\)'),
    ('no_steps', 'fleet', lambda a: _set(a.cfg, steps=0), W + 'n, k, steps, n_seeds must be >= 1'),
    ('no_pulses_ens', 'ens', lambda a: _set(a.cfg, k=0), W + 'n, k, steps, n_seeds must be >= 1'),
    ('plan_seeds_negative', 'ens', lambda a: _set(a.cfg, plan_seeds=-1), W + 'n, k, steps, n_seeds must be >= 1'),
    ('trajectories', 'fleet', lambda a: _set(a.cfg, n_seeds=1 << 24), W + '16777216 x 3 trajectories'),
    ('envelope_constant', 'fleet', lambda a: _set(a.cfg, has_envelope=1), W + 'envelope constant missing'),
    ('d2wdt2_alone', 'fleet', lambda a: _set(a.cfg, has_d2wdt2=1), W + r'd2wdt2 needs dwdt'),
    # what qoc_create_shaped refuses about the line
    ('no_samples', 'line', lambda a: _set(a.tr, n_samples=0), W + r'n_samples = 0 \(>= 1\)'),
    ('null_T', 'line', lambda a: _set(a.tr, T=None), W + 'the response matrix is missing'),
    ('envelope_line', 'ens_line', lambda a: _set(a.cfg, has_envelope=1), W + 'the envelope regulariser is defined per time slice, not per sample'),
    ('T_nan', 'line', lambda a: _poke(a.tr.T, 2 * SAMPLES + 1, float('nan')), W + r'T\[2\]\[1\] is not finite'),
    ('T_dead_column', 'ens_line', lambda a: _poke(a.tr.T, np.arange(STEPS) * SAMPLES + 2, 0.0), W + r'column 2 of T is zero \(the sample never reaches the pulse\)'),
    ('no_steps_line', 'line', lambda a: _set(a.cfg, steps=0), W + 'k, steps must be >= 1'),
    # what qoc_create_mapped refuses about the map
    ('null_poly', 'map', lambda a: _set(a.mp, poly=None), W + r"the map's polynomial coefficients \(poly\) are missing"),
    ('no_steps_map', 'map', lambda a: _set(a.cfg, steps=0), W + 'k, steps must be >= 1'),
    ('no_terms', 'map', lambda a: _set(a.mp, n_terms=0), W + r'n_terms = 0 \(1 .. 64 operators\)'),
    ('terms65', 'map', lambda a: _set(a.mp, n_terms=65), W + r'n_terms = 65 \(1 .. 64 operators\)'),
    ('degree0', 'map', lambda a: _set(a.mp, degree=0), W + r'degree = 0 \(1 .. 8\)'),
    ('degree9', 'map', lambda a: _set(a.mp, degree=9), W + r'degree = 9 \(1 .. 8\)'),
    ('poly_nan', 'map', lambda a: _poke(a.mp.poly, (2 * 2 + 1) * MAP_D + 1, float('nan')), W + r'poly\[2\]\[1\]\[1\] is not finite'),
    ('mix_inf', 'map', lambda a: _poke(a.mp.mix, (1 * 2 + 0) * STEPS + 4, float('inf')), W + r'mix\[1\]\[0\]\[4\] is not finite'),
    ('fixed_nan', 'map', lambda a: _poke(a.mp.fixed, 2 * STEPS + 3, float('nan')), W + r'fixed\[2\]\[3\] is not finite'),
    ('pulse_unmapped', 'map', lambda a: _poke(a.mp.poly, [(i * 2 + 1) * MAP_D + d for i in range(MAP_R) for d in range(MAP_D)], 0.0),
     W + r'pulse 1 reaches no operator \(poly\[i\]\[1\] or mix\[i\]\[1\] is zero for every i\)'),
    ('pulse_mixed_out', 'map', lambda a: _poke(a.mp.mix, [(i * 2 + 0) * STEPS + t for i in range(MAP_R) for t in range(STEPS)], 0.0),
     W + r'pulse 0 reaches no operator'),
]
C_REFUSALS += [('null_' + name, 'fleet', lambda a, name=name: _set(a, drop=(name,)), W + 'null argument') for name in ('cfg', 'dc', 'Hs', 'V', 'W', 'maxA', 'out')]


def refusal_engine(kind):
    """The engine a row of C_REFUSALS is made with, from fresh copies of every table the change may write into."""
    with_map, with_line = kind == 'map', kind in ('line', 'ens_line')
    p = ofr.problem(3, 2, STEPS, 2, 2, r=MAP_R if with_map else 2)
    fl = ofr.make_fleet(p, F, E, Q)
    cm = ref.make_map(2, MAP_R, MAP_D, STEPS, mix=True, fixed=True) if with_map else None
    T = tf.hold(STEPS, SAMPLES).matrix.copy() if with_line else None
    if kind in ('ens', 'ens_line'):
        return make_engine(p, R, ens=fl.device(1), T=T)
    return make_engine(p, F * R, fl=fl, T=T, cm=cm)


@pytest.mark.parametrize('name,kind,change,msg', C_REFUSALS, ids=[row[0] for row in C_REFUSALS])
def test_the_library_refuses_by_message(name, kind, change, msg):
    """Every message that qoc_create_open_fleet can give through its own checks and through the funnel of the fleet, the ensemble, the line and the
    map.  (Not reachable through it, and so not here: the funnel's own null-argument and missing-fleet or missing-map messages -- a NULL fleet, line
    or map is a meaning, and the other arguments are checked first; the ensemble's refusals of time sharding and of QOC_PATH_SMALL, which the open
    engine's own refusals of both come before; the limit of 8 controls, which holds on the MFMA and fused paths only.)"""
    with tampered(change):
        with pytest.raises(P.QocError, match=msg):
            refusal_engine(kind).close()


def test_no_variant_of_another_path_is_refused():
    """qoc_config.variant selects among kernels of the MFMA and GEMM paths.  An open engine has none: the ensemble's refusal of variant 5 (the MFMA
    path's latency mode) is not for it, as qoc_create_open does not know it either."""
    with tampered(lambda a: _set(a.cfg, variant=5)):
        eng = refusal_engine('fleet')
    try:
        assert eng.plan['path'] == 'lindblad' and eng.plan['devices'] == str(F)
    finally:
        eng.close()


def test_two_open_fleets_and_a_plain_open_engine_alive_at_once():
    p, fl, xs, want = parity_reference('unitary')
    last = fl_mod.validate(fl_mod.Fleet(fl.operators, fl.offsets[1:], fl.amp_scales[1:], weights=fl.weights, collapse_ops=fl.collapse_ops,
                                        rate_scales=fl.rate_scales[1:]), 3, 2)
    big = ofr.problem(32, 1, 2, 1, 5, taylor=(4, 1), seed=11)                       # (its LDS opt-in must not disturb the small engines, nor theirs it)
    sp, spb = ofr.engine_system(p), ofr.engine_system(big)
    a, b = make_engine(p, F * R, fl=fl), make_engine(p, R, fl=last)
    plain = P.HipEngine(spb.Hs, spb.U0, spb.V, spb.W, big['maxA'], spb.dt, spb.total_time, spb.steps, spb.exp_terms, spb.scaling, reg_coeffs={}, n_seeds=1,
                        collapse_ops=big['collapse_ops'])
    try:
        assert a.plan['devices'] == '2' and b.plan['devices'] == '1' and 'members' not in plain.plan
        xb = start_points(1, 2, 1, seed=32)
        plain.set_base(xb)
        before = plain.evaluate()
        a.set_base(xs)
        b.set_base(xs[R:])
        ra, rb_ = a.evaluate(), b.evaluate()
        for key in KEYS + ('grad',):                              # device 1 of the one is device 0 of the other
            np.testing.assert_array_equal(ra[key][R:], rb_[key], err_msg=key)
        for g, o in enumerate(want):
            assert_scalars('side by side', ra, g, o)
            assert_gradient('side by side grad[%d]' % g, ra['grad'][g], o['grad'])
        after = plain.evaluate()
        for key in KEYS + ('grad',):
            np.testing.assert_array_equal(before[key], after[key], err_msg=key)
        with pytest.raises(P.QocError, match='status -4'):
            plain.member_final_density()
    finally:
        a.close()
        b.close()
        plain.close()


# ---- 7. Grape, the example ------------------------------------------------------------------------------------------------------------------------

GRAPE_CONV = {'rate': 0.02, 'update_step': 7, 'max_iterations': 20, 'conv_target': 1e-12, 'learning_rate_decay': 100}


def test_grape_with_decay_against_plain_open_calls():
    """A fleet of three single-member devices and a robust call on one of them, 20 Adam iterations from one guess at a fixed (T, s): every device's
    loss, pulse and final density operators against Grape(collapse_ops=...) on that member's own Hamiltonians and scaled operators.  The loss at
    S_RTOL; pulse and densities at LOOP_ATOL, as a base after a loop is bounded."""
    p = ofr.problem(3, 2, 8, 2, 2, regs={'dwdt': 0.01}, seed=5)
    fl = ofr.make_fleet(p, 3, 1, 1, seed=4)
    guess = 0.5 * np.asarray(p['maxA'])[:, None] * np.sin(start_points(2, 8, 1, seed=8)[0])
    kw = dict(convergence=dict(GRAPE_CONV), U0=p['U0'], reg_coeffs=p['reg_coeffs'], maxA=list(p['maxA']), method='Adam', Taylor_terms=[6, 1], initial_guess=guess)
    uks, rho = _grape(*grape_args(p), fleet=fl, **kw)
    assert uks.shape == (3, 2, 8) and rho.shape == (3, 2, 2, 3, 3) and fl.losses.shape == (3,) and fl.member_losses.shape == (3, 1)
    assert list(fl.iterations) == [20] * 3 and list(fl.best) == [0] * 3
    u_r, rho_r = _grape(*grape_args(p), robust=fl.device(1), **kw)
    assert rho_r.shape == (2, 2, 3, 3)
    np.testing.assert_allclose(u_r, uks[1], rtol=0, atol=LOOP_ATOL)
    np.testing.assert_allclose(rho_r, rho[1], rtol=0, atol=LOOP_ATOL)
    for f in range(3):
        dev = fl.device(f)
        H0e, Hopse = rb.member_hamiltonians(p['H0'], p['Hops'], dev, 0)
        # (the member's scale on the operators: the same products u H, so the same pulse)
        u1, rho1, l1 = _grape(H0e, Hopse, p['Hnames'], p['U'], p['total_time'], p['steps'], p['states_concerned_list'], collapse_ops=rb.member_collapse_ops(dev, 0),
                              _return_session=True, **kw)
        print('device %d: fleet loss %.17g, plain open loss %.17g, max pulse difference %.3e' % (f, fl.losses[f], l1, np.max(np.abs(uks[f] - u1))))
        assert abs(fl.losses[f] - l1) <= S_RTOL * max(1.0, abs(l1))
        np.testing.assert_allclose(uks[f], u1, rtol=0, atol=LOOP_ATOL)
        np.testing.assert_allclose(rho[f], rho1, rtol=0, atol=LOOP_ATOL)
    assert ofr.swapped_apart(list(fl.losses))


def test_a_scipy_method_drives_a_robust_call_with_decay():
    """method='L-BFGS-B' on three members with their own decay: scipy's search, fed the engine's loss and gradient, ends below the reference's loss at
    the guess, and what the call returns is the reference's at the returned pulse."""
    p = ofr.problem(3, 2, 8, 2, 2, seed=5)
    ens = ofr.make_fleet(p, 1, 3, 1, seed=4).device(0)
    maxA = np.asarray(p['maxA'])
    x0 = start_points(2, 8, 1, seed=8)[0]
    uks, rho = _grape(*grape_args(p), robust=ens, convergence={'max_iterations': 5, 'conv_target': 1e-12, 'update_step': 5}, U0=p['U0'], reg_coeffs={},
                      maxA=list(maxA), method='L-BFGS-B', Taylor_terms=[6, 1], initial_guess=maxA[:, None] * np.sin(x0))
    assert uks.shape == (2, 8) and rho.shape == (2, 2, 3, 3)
    start = ofr.evaluate(p, None, ens, x0, want_grad=False)
    end = ofr.evaluate(p, None, ens, np.arcsin(np.clip(uks / maxA[:, None], -1.0, 1.0)), want_grad=False)
    print('L-BFGS-B: reference loss %.17g at the guess, %.17g at the returned pulse' % (start['loss'], end['loss']))
    assert end['loss'] < start['loss']
    assert np.max(np.abs(rho - end['rho_final'])) <= S_RTOL


def test_example_runs_with_a_short_budget():
    """examples/fleet_qubits_under_decay.py, 30 iterations: the shapes, and what holds after any budget -- every infidelity under decay is finite and
    positive (no pulse undoes T1 within the gate), and the table has one row per qubit."""
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import fleet_qubits_under_decay as ex
    with contextlib.redirect_stdout(io.StringIO()) as out:
        closed, aware = ex.main(iterations=30, quiet=True)
    assert closed.shape == aware.shape == (ex.QUBITS,)
    assert np.all(np.isfinite(closed)) and np.all(np.isfinite(aware)) and np.all(closed > 0) and np.all(aware > 0)
    assert len([ln for ln in out.getvalue().splitlines() if ln[:5].strip().isdigit()]) == ex.QUBITS
