"""Device fleets on the GPU (qoc_create_fleet): control set g of an engine with F devices and R control sets per device must compute
exactly what an ensemble engine computes for device g // R's rows.

  1. parity with the reference composed per device (tests/fleet_reference.py: rows picked, nothing else) on every kernel family an ensemble runs on;
  2. bit identity with qoc_create_ensemble engines built from each device's rows (the same plan_seeds), and of F = 1 with the plain ensemble engine;
  3. composition with a risk, a line, a control map and the exact gradient;
  4. the loops: Adam with devices that finish at different iterations, L-BFGS, and method='EVOLVE' as the scan of one pulse;
  5. more items than one pass of k_ens_expand's capped grid;
  6. refusals of the library, lifetime, determinism, Grape(fleet=...) against F Grape(robust=...) calls, the example.

Tolerances: TIGHT of tests/test_robust_families.py (1e-12 scalars relative to max(1, |x|), 1e-11 max(1, max|grad|), 1e-12 unitaries), at 7 and 8 slices; the
600-slice grid-cap problem takes that file's FULL (its rule for more than 200 slices: round-off accumulates along the product chain)."""
import contextlib
import functools
import io
import os
import sys

import numpy as np
import pytest

from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import control_map as cmap
from quantum_optimal_control.helper_functions import fleet as fl_mod
from quantum_optimal_control.helper_functions import transfer as tf
from tests import control_map_reference as ref
from tests import fleet_reference as fr
from tests import test_robust_gpu as rg
from tests.test_adam_tail import _choose_target
from tests.test_lbfgs_gpu import BASE as LBFGS_BASE
from tests.test_lbfgs_gpu import compare_with_reference
from tests.test_robust_families import FULL, TIGHT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = hip_engine
F, R = 3, 2
KEYS = ('loss', 'reg_loss', 'grad_squared', 'unitary_scale')


# ---- engines and start points -------------------------------------------------------------------------------------------------------------------

def make_engine(c, fl, n_sets, path=P.PATH_AUTO, variant=0, chunks=0, T=None, cm=None, exact=False, ensemble=None, plan_seeds=0):
    """A fleet engine (fl: a Fleet) or, fl None, the ensemble engine of `ensemble`."""
    sp = ref.engine_system(c)
    return P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, c['maxA'], sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, state_transfer=sp.state_transfer,
                       reg_coeffs=c['reg_coeffs'], n_seeds=n_sets, path=path, variant=variant, chunks=chunks, plan_seeds=plan_seeds, ensemble=ensemble,
                       transfer=T, exact_gradient=exact, control_map=cm, fleet=fl)


def start_points(k, width, count, seed=0):
    return np.random.default_rng(4000 + width + seed).normal(0.0, 0.7, size=(count, k, width))


def assert_plan(eng, fl, plan):
    for key, want in dict(plan, devices=str(fl.n_devices), members=str(fl.n_members), perturbations=str(len(fl.operators))).items():
        assert eng.plan.get(key) == want, (key, want, eng.plan)
    assert eng.devices == fl.n_devices and eng.members == fl.n_members


def assert_matches(tol, r, g, o, keys=KEYS):
    for key in keys:
        print('%s[%d]: engine %.17g reference %.17g' % (key, g, r[key][g], o[key]))
        assert abs(r[key][g] - o[key]) <= tol['s'] * max(1.0, abs(o[key])), (key, g, r[key][g], o[key])
    gm = max(1.0, float(np.max(np.abs(o['grad']))))
    err = float(np.max(np.abs(r['grad'][g] - o['grad'])))
    print('grad[%d]: max error %.3e of max %.3e' % (g, err, gm))
    assert err <= tol['g'] * gm, (g, err, gm)


# ---- 1. parity with the composed reference, family by family ------------------------------------------------------------------------------------

FAMILIES = [
    ('unitary_generic', 'unitary', P.PATH_GENERIC, 0, 0, dict(path='generic')),
    ('unitary_mfma', 'unitary', P.PATH_MFMA, 0, 0, dict(path='mfma', nt='1')),
    ('unitary_gemm', 'unitary', P.PATH_GEMM, 0, 0, dict(path='gemm', route='unitary')),
    ('state_generic', 'state', P.PATH_GENERIC, 0, 0, dict(path='generic')),
    ('state_mfma', 'state', P.PATH_MFMA, 0, 0, dict(path='mfma', nt='1')),
    ('state_gemm_direct', 'state', P.PATH_GEMM, 0, 1, dict(path='gemm', route='direct')),
    ('state_gemm_propagator', 'state', P.PATH_GEMM, 0, 2, dict(path='gemm', route='propagator')),
    ('state_st_fused', 'state', P.PATH_ST_FUSED, 0, 0, dict(path='st_fused')),
]
MEMBERS = [(1, 0), (1, 2), (3, 0), (3, 2)]                # (E, q)


@functools.lru_cache(maxsize=None)
def parity_reference(kind, E, q):
    """(problem, fleet, start points, expectation of every control set): computed once, shared by the families.  Checked here, on the CPU: every
    device's rows differ from every other's, devices 1 and 2 in offsets and in scales, and at ONE start point the devices' expected losses and
    gradients lie more than 1e-6 apart -- a kernel that reads the rows of device g % F, or of device 0, misses by orders of magnitude."""
    c = fr.problem(kind)
    fl = fr.make_fleet(c, F, E, q)
    for a in range(F):
        for b in range(a + 1, F):
            assert np.all(fl.amp_scales[a] != fl.amp_scales[b]) and (q == 0 or np.all(fl.offsets[a] != fl.offsets[b]))
    xs = start_points(len(c['maxA']), c['steps'], F * R)
    at_one = [fr.composed(c, fl, f, xs[1]) for f in range(F)]
    assert fr.swapped_apart([o['loss'] for o in at_one]) and fr.swapped_apart([o['grad'] for o in at_one])
    return c, fl, xs, [fr.composed(c, fl, f, xs[g]) for g, (f, _) in enumerate(fr.control_sets(F, R))]


@pytest.mark.parametrize('E,q', MEMBERS, ids=['E%dq%d' % eq for eq in MEMBERS])
@pytest.mark.parametrize('name,kind,path,variant,chunks,plan', FAMILIES, ids=[row[0] for row in FAMILIES])
def test_every_control_set_runs_its_own_device(name, kind, path, variant, chunks, plan, E, q):
    c, fl, xs, want = parity_reference(kind, E, q)
    eng = make_engine(c, fl, F * R, path, variant, chunks)
    try:
        assert_plan(eng, fl, plan)                               # the family first
        eng.set_base(xs)
        r = eng.evaluate()
        ms = eng.member_scalars()
        Uf = None if c['state_transfer'] else eng.get_final_unitary()
        assert r['grad'].shape == xs.shape and ms['loss'].shape == (F * R, E)
        for g, o in enumerate(want):
            assert_matches(TIGHT, r, g, o)
            assert np.max(np.abs(ms['loss'][g] - o['member_loss'])) <= TIGHT['s'] * max(1.0, np.max(np.abs(o['member_loss']))), (g, ms['loss'][g])
            if Uf is not None:
                assert np.max(np.abs(Uf[g] - o['U0'])) <= TIGHT['u'], g
    finally:
        eng.close()


# ---- 2. bit for bit against the existing entry point --------------------------------------------------------------------------------------------

LOOP = dict(rate=0.02, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=100, poll_every=100)


def ten_iterations(eng, bases):
    """Ten iterations of the device Adam loop, then one evaluation where they ended: everything the comparison reads."""
    eng.set_base(bases)
    eng.iterate(eng.adam_params(**LOOP), 10)
    s, ms = eng.scalars(), eng.member_scalars()
    out = dict(base=eng.get_base(), uks=eng.get_uks(evaluated=True), member_loss=ms['loss'], member_reg_state=ms['reg_state'])
    out.update({'loop_' + key: s[key] for key in KEYS + ('iterations', 'done')})
    r = eng.evaluate()
    out.update({key: r[key] for key in KEYS + ('grad',)})
    return out


BIT_PATHS = [('generic', P.PATH_GENERIC, dict(path='generic')), ('mfma', P.PATH_MFMA, dict(path='mfma')), ('gemm', P.PATH_GEMM, dict(path='gemm'))]


@pytest.mark.parametrize('name,path,plan', BIT_PATHS, ids=[row[0] for row in BIT_PATHS])
def test_fleet_is_bit_identical_to_the_ensemble_engines_of_its_devices(name, path, plan):
    c, fl, xs, _ = parity_reference('unitary', 3, 2)
    eng = make_engine(c, fl, F * R, path)
    try:
        assert_plan(eng, fl, plan)
        got = ten_iterations(eng, xs)
    finally:
        eng.close()
    assert list(got['loop_iterations']) == [10] * (F * R)
    for f in range(F):
        one = make_engine(c, None, R, path, ensemble=fr.device(fl, f), plan_seeds=F * R)
        try:
            assert 'devices' not in one.plan and one.plan['path'] == plan['path']
            want = ten_iterations(one, xs[f * R:(f + 1) * R])
        finally:
            one.close()
        for key, val in want.items():
            np.testing.assert_array_equal(got[key][f * R:(f + 1) * R], val, err_msg='%s of device %d' % (key, f))


@pytest.mark.parametrize('name,path,plan', BIT_PATHS, ids=[row[0] for row in BIT_PATHS])
def test_one_device_is_the_plain_ensemble_engine(name, path, plan):
    c, fl, xs, _ = parity_reference('unitary', 3, 2)
    one = fl_mod.validate(fl_mod.Fleet(fl.operators, fl.offsets[1:2], fl.amp_scales[1:2], weights=fl.weights), 4, 2)
    out = []
    for fleet, ens in ((one, None), (None, fr.device(fl, 1))):
        eng = make_engine(c, fleet, R, path, ensemble=ens)
        try:
            assert ('devices' in eng.plan) == (fleet is not None)
            out.append(ten_iterations(eng, xs[:R]))
        finally:
            eng.close()
    for key, val in out[1].items():
        np.testing.assert_array_equal(out[0][key], val, err_msg=key)


# ---- 3. composition -----------------------------------------------------------------------------------------------------------------------------

STEPS, SAMPLES = 8, 3                                     # hold(8, 3): windows of 3, 3 and 2 slices
COMPOSITIONS = {                                          # name: (risk, line, map, exact gradient, path)
    'risk': (50.0, False, False, False, P.PATH_AUTO),
    'hold_line': (0.0, True, False, False, P.PATH_AUTO),
    'control_map': (0.0, False, True, False, P.PATH_AUTO),
    'exact_gradient': (0.0, False, False, True, P.PATH_AUTO),
    'risk_line_map': (50.0, True, True, False, P.PATH_GENERIC),
    'risk_line_map_exact': (50.0, True, True, True, P.PATH_GENERIC),
}


@pytest.mark.parametrize('name', list(COMPOSITIONS))
def test_fleet_composes(name):
    """The reference is tests/control_map_reference.py: evaluate with device f's rows; where the engine has no map the reference runs the identity map
    (which tests/test_control_map_gpu.py holds bit-identical to no map)."""
    beta, with_line, with_map, exact, path = COMPOSITIONS[name]
    k, r = 2, 3 if with_map else 2
    c = fr.problem('unitary', k=k, r=r, steps=STEPS, regs=dict(fr.REGS_UNITARY, forbidden_coeff_list=[5.0], states_forbidden_list=[3], speed_up=0.3))
    fl = fr.make_fleet(c, F, 3, 2, risk=beta)
    cm = ref.make_map(2, 3, 3, STEPS, mix=True, fixed=True) if with_map else None
    ref_map = cm if with_map else cmap.validate(cmap.identity(k), k=k, r=k, steps=STEPS)
    T = tf.hold(STEPS, SAMPLES).matrix if with_line else None
    xs = start_points(k, SAMPLES if with_line else STEPS, F * R, seed=1)
    eng = make_engine(c, fl, F * R, path, T=T, cm=cm, exact=exact)
    try:
        assert_plan(eng, fl, dict(gradient='exact' if exact else 'first_order'))
        assert eng.risk == beta and ('terms' in eng.plan) == with_map and ('samples' in eng.plan) == with_line
        if exact or path == P.PATH_GENERIC:
            assert eng.plan['path'] == 'generic', eng.plan
        eng.set_base(xs)
        res, pi, ms = eng.evaluate(), eng.member_weights(), eng.member_scalars()
        assert pi.shape == (F * R, 3)
        seen = []
        for g, (f, _) in enumerate(fr.control_sets(F, R)):
            o = fr.evaluate(c, ref_map, fl, f, xs[g], T=T, exact=exact)
            assert_matches(TIGHT, res, g, o)
            assert np.max(np.abs(ms['loss'][g] - o['member_loss'])) <= TIGHT['s'] * max(1.0, np.max(np.abs(o['member_loss'])))
            print('weights[%d]: engine %s reference %s' % (g, pi[g], o['weights']))
            assert np.max(np.abs(pi[g] - o['weights'])) <= TIGHT['s'], (g, pi[g], o['weights'])
            seen.append(o['weights'])
        if beta > 0:                                       # the tilt is per control set: no two rows of weights agree (1e-6: six decades above the bound)
            assert fr.swapped_apart(seen)
    finally:
        eng.close()


# ---- 4. loops -----------------------------------------------------------------------------------------------------------------------------------

LOOP_MAX = 11


@functools.lru_cache(maxsize=None)
def loop_reference():
    """Three devices from ONE start point, Adam by rg.python_loop over each device's composed reference, and a conv_target at which they stop at
    different iterations (tests/test_adam_tail.py: _choose_target)."""
    c = fr.problem('unitary', regs={'dwdt': 0.01})
    fl = fr.make_fleet(c, F, 2, 1, seed=9)
    x0 = start_points(2, c['steps'], 1, seed=3)[0]
    conv = dict(rate=0.1, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=LOOP_MAX)
    sps = [fr.member_systems(c, fl, f) for f in range(F)]
    free = [rg.python_loop(sps[f], fl.weights, x0, conv) for f in range(F)]
    target, stops = _choose_target([run['history'] for run in free], LOOP_MAX, accept=lambda s: len(set(s)) == F and min(s) > 0)
    conv = dict(conv, conv_target=target)
    refs = [rg.python_loop(sps[f], fl.weights, x0, conv) for f in range(F)]
    assert [run['iterations'] for run in refs] == stops
    return c, fl, x0, conv, refs, stops


def test_adam_loop_with_devices_that_finish_at_different_iterations():
    """Iterations, bases (1e-9) and final scalars (1e-10) as tests/test_robust_families.py's loop rows; then every control set's member scalars and
    final unitary against the reference AT ITS OWN final base, at TIGHT: a finished control set keeps the read-backs of its last evaluation while the
    others go on (one Adam step further they would be off by far more)."""
    c, fl, x0, conv, refs, stops = loop_reference()
    poll = next(p for p in (5, 4, 7, 3, 6, 9, 8, 13) if all(s % p for s in stops))
    eng = make_engine(c, fl, F)
    try:
        eng.set_base(np.broadcast_to(x0[None], (F,) + x0.shape))
        its = eng.run_adam(eng.adam_params(poll_every=poll, **conv))
        Uf, s, base, ms = eng.get_final_unitary(), eng.scalars(), eng.get_base(), eng.member_scalars()
        print(eng.plan, 'stops', stops, 'poll', poll)
        assert list(its) == stops and list(s['iterations']) == stops and list(s['done']) == [1] * F, (its, stops)
        for f, run in enumerate(refs):
            assert np.max(np.abs(base[f] - run['base'])) < 1e-9, (f, np.max(np.abs(base[f] - run['base'])))
            for key in KEYS:
                assert abs(s[key][f] - run['last'][key]) < 1e-10 * max(1.0, abs(run['last'][key])), (key, f, s[key][f], run['last'][key])
            o = fr.composed(c, fl, f, base[f])
            for key in KEYS:
                assert abs(s[key][f] - o[key]) <= TIGHT['s'] * max(1.0, abs(o[key])), (key, f, s[key][f], o[key])
            assert np.max(np.abs(ms['loss'][f] - o['member_loss'])) <= TIGHT['s'], (f, stops[f])
            assert np.max(np.abs(Uf[f] - o['U0'])) <= TIGHT['u'], (f, stops[f])
    finally:
        eng.close()


def test_lbfgs_run_follows_the_reference_on_the_last_device():
    """tests/lbfgs_reference.py driven by device 2's reference with the exact gradient (tests/test_control_map_gpu.py does the same for one ensemble);
    the comparison steps control set 0, so the fleet here is the one device -- with rows that are not device 0's of the three."""
    c, fl, xs, _ = parity_reference('unitary', 3, 2)
    last = fl_mod.validate(fl_mod.Fleet(fl.operators, fl.offsets[2:], fl.amp_scales[2:], weights=fl.weights), 4, 2)
    ident = cmap.validate(cmap.identity(2), k=2, r=2, steps=c['steps'])
    eng = make_engine(c, last, 1, P.PATH_GENERIC, exact=True)
    try:
        compare_with_reference(eng, lambda x: fr.evaluate(c, ident, fl, 2, x, exact=True), xs[0], dict(LBFGS_BASE, max_iterations=8), 8, name='fleet')
    finally:
        eng.close()


def test_lbfgs_loop_runs_every_control_set_on_its_device():
    """run_lbfgs on the whole fleet: every control set ends no higher than it started, at a point whose reg_loss is its device's reference value."""
    c, fl, xs, want = parity_reference('unitary', 3, 2)
    eng = make_engine(c, fl, F * R, P.PATH_GENERIC, exact=True)
    try:
        eng.set_base(xs)
        eng.run_lbfgs(eng.lbfgs_params(conv_target=-1.0, min_grad=-1.0, max_iterations=6, poll_every=4))
        s, base = eng.scalars(), eng.get_base()
        res = eng.evaluate()
        for g, (f, _) in enumerate(fr.control_sets(F, R)):
            o = fr.composed(c, fl, f, base[g])
            assert abs(res['reg_loss'][g] - o['reg_loss']) <= TIGHT['s'] * max(1.0, abs(o['reg_loss'])), (g, res['reg_loss'][g], o['reg_loss'])
            assert res['reg_loss'][g] <= want[g]['reg_loss'] and s['iterations'][g] > 0, (g, res['reg_loss'][g], want[g]['reg_loss'])
    finally:
        eng.close()


def _grape(*args, **kw):
    from quantum_optimal_control.main_grape.grape import Grape
    with contextlib.redirect_stdout(io.StringIO()):
        return Grape(*args, save=False, show_plots=False, **kw)


def grape_args(c):
    return (c['H0'], c['Hops'], c['Hnames'], c['U'], c['total_time'], c['steps'], c['states_concerned_list'])


def test_evolve_scans_one_pulse_over_the_devices():
    c, fl, xs, _ = parity_reference('unitary', 3, 2)
    maxA = np.asarray(c['maxA'])
    pulse = maxA[:, None] * np.sin(xs[0])
    uks, Uf = _grape(*grape_args(c), U0=c['U0'], reg_coeffs=c['reg_coeffs'], maxA=list(maxA), method='EVOLVE', initial_guess=pulse, Taylor_terms=c['Taylor_terms'],
                     fleet=fl)
    assert uks.shape == (F, 2, c['steps']) and Uf.shape == (F, 4, 4) and list(fl.best) == [0] * F
    for f in range(F):
        o = fr.composed(c, fl, f, np.arcsin(pulse / maxA[:, None]))
        assert np.max(np.abs(uks[f] - pulse)) <= 1e-14
        assert abs(fl.losses[f] - o['loss']) <= TIGHT['s'] * max(1.0, abs(o['loss'])), (f, fl.losses[f], o['loss'])
        assert np.max(np.abs(fl.member_losses[f] - o['member_loss'])) <= TIGHT['s'] and np.max(np.abs(Uf[f] - o['U0'])) <= TIGHT['u']
    own = np.stack([maxA[:, None] * np.sin(xs[f]) for f in range(F)])                # a pulse per device
    _grape(*grape_args(c), U0=c['U0'], reg_coeffs=c['reg_coeffs'], maxA=list(maxA), method='EVOLVE', initial_guess=own, Taylor_terms=c['Taylor_terms'], fleet=fl)
    for f in range(F):
        o = fr.composed(c, fl, f, np.arcsin(own[f] / maxA[:, None]))
        assert abs(fl.losses[f] - o['loss']) <= TIGHT['s'] * max(1.0, abs(o['loss'])), (f, fl.losses[f], o['loss'])


# ---- 5. more items than one pass of k_ens_expand's grid -----------------------------------------------------------------------------------------

BIG_F, BIG_R, BIG_STEPS = 64, 4, 600


def test_more_items_than_one_pass_of_the_expand_grid():
    """256 control sets x 4 rows x 600 slices = 614 400 items through a grid capped at 2048 x 256 = 524 288 threads: the control sets from 218 on are
    written in the second pass, where the device index must still be g // R.  The first and the last control set and the two around item 524 288."""
    from tests.test_robust_families import qubit
    c = dict(qubit(BIG_STEPS), maxA=np.array([0.3, 0.2]))
    fl = fr.make_fleet(c, BIG_F, 1, 2, seed=2)
    rows, G = len(c['Hops']) + 2, BIG_F * BIG_R
    assert G * rows * BIG_STEPS > 2048 * 256
    edge = (2048 * 256) // (rows * BIG_STEPS)
    assert edge == 218 and edge // BIG_R != (edge + 2) // BIG_R                        # ... and a device boundary lies right behind it
    sample = [0, edge, edge + 2, G - 1]
    xs = np.random.default_rng(6).normal(0.0, 1 / np.sqrt(BIG_STEPS), size=(G, 2, BIG_STEPS))
    sp = rg.nominal_system(c)
    eng = P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, reg_coeffs=sp.reg_coeffs, n_seeds=G, fleet=fl)
    try:
        assert_plan(eng, fl, {})
        eng.set_base(xs)
        r = eng.evaluate()
        for g in sample:
            assert_matches(FULL, r, g, fr.composed(c, fl, g // BIG_R, xs[g]))
        other = fr.composed(c, fl, (edge + 2) // BIG_R - 1, xs[edge + 2], )              # the neighbouring device's rows give another value
        assert abs(other['loss'] - r['loss'][edge + 2]) > 1e-6
    finally:
        eng.close()


# ---- 6. refusals, lifetime, determinism, Grape, the example -------------------------------------------------------------------------------------

@contextlib.contextmanager
def tampered(change):
    """Lets `change(cfg, ens, fleet)` alter what HipEngine hands to qoc_create_fleet (it may return 'null fleet'): what the Python layer would refuse
    itself reaches the library."""
    lib = P.load_library()
    real = lib.qoc_create_fleet

    def call(cfg, ens, fl, *rest):
        if change(cfg._obj, ens._obj, fl._obj) == 'null fleet':
            fl = None
        return real(cfg, ens, fl, *rest)
    lib.qoc_create_fleet = call
    try:
        yield
    finally:
        lib.qoc_create_fleet = real


def _set(obj, **kw):
    for key, v in kw.items():
        setattr(obj, key, v)


def _poke(arr, idx, v):
    arr[idx] = v


C_REFUSALS = [
    ('null_fleet', lambda cfg, ens, fl: 'null fleet', 'qoc_create_fleet: the fleet is missing'),
    ('null_amp_scales', lambda cfg, ens, fl: _set(fl, amp_scales=None), r"qoc_create_fleet: the fleet's amp_scales are missing"),
    ('null_offsets', lambda cfg, ens, fl: _set(fl, offsets=None), r"qoc_create_fleet: the fleet's offsets are missing \(n_perturb = 2\)"),
    ('no_devices', lambda cfg, ens, fl: _set(fl, devices=0), r'qoc_create_fleet: devices = 0 \(>= 1\)'),
    ('uneven', lambda cfg, ens, fl: _set(cfg, n_seeds=7), 'qoc_create_fleet: n_seeds = 7 is no multiple of devices = 3'),
    ('amp_nan', lambda cfg, ens, fl: _poke(fl.amp_scales, 1 * 6 + 2 * 2 + 1, float('nan')), r'qoc_create_fleet: amp_scales\[1\]\[2\]\[1\] is not finite'),
    ('offset_inf', lambda cfg, ens, fl: _poke(fl.offsets, 2 * 6 + 0 * 2 + 1, float('inf')), r'qoc_create_fleet: offsets\[2\]\[0\]\[1\] is not finite'),
    ('time_shards', lambda cfg, ens, fl: _set(cfg, time_shards=2), 'qoc_create_fleet: an ensemble cannot be time-sharded'),
    ('small_path', lambda cfg, ens, fl: _set(cfg, path=P.PATH_SMALL), 'qoc_create_fleet: the workgroup-resident path'),
    ('latency', lambda cfg, ens, fl: _set(cfg, variant=5), 'qoc_create_fleet: the latency mode of the MFMA path'),
    ('bad_weight', lambda cfg, ens, fl: _poke(ens.weights, 1, -0.25), 'qoc_create_fleet: weight 1 is'),
    ('nine_controls', lambda cfg, ens, fl: _set(cfg, path=P.PATH_MFMA), r'qoc_create_fleet: path 2 is limited to 8 controls; the ensemble\'s trajectories have k \+ q = 9'),
]


@pytest.mark.parametrize('name,change,msg', C_REFUSALS, ids=[row[0] for row in C_REFUSALS])
def test_the_library_refuses_by_message(name, change, msg):
    c, fl, xs, _ = parity_reference('unitary', 3, 2)
    if name == 'nine_controls':
        c = fr.problem('unitary', k=7, seed=3)
        fl = fr.make_fleet(c, F, 3, 2)
    fl = fl_mod.validate(fl, None, len(c['maxA']))            # (a copy: the tampering writes into its arrays)
    with tampered(change):
        with pytest.raises(P.QocError, match=msg):
            make_engine(c, fl, F * R)


def test_create_destroy_and_two_fleets_alive_at_once():
    c, fl, xs, want = parity_reference('unitary', 3, 2)
    for _ in range(3):
        eng = make_engine(c, fl, F * R)
        eng.set_base(xs)
        assert abs(eng.evaluate()['loss'][3] - want[3]['loss']) <= TIGHT['s']
        eng.close()
        eng.close()
    two = fl_mod.validate(fl_mod.Fleet(fl.operators, fl.offsets[1:], fl.amp_scales[1:], weights=fl.weights), 4, 2)
    a, b = make_engine(c, fl, F * R), make_engine(c, two, 2 * R)
    try:
        assert a.plan['devices'] == '3' and b.plan['devices'] == '2'
        a.set_base(xs)
        b.set_base(xs[R:])
        ra, rb_ = a.evaluate(), b.evaluate()
        for key in KEYS + ('grad',):                             # devices 1 and 2 of the one are devices 0 and 1 of the other
            np.testing.assert_array_equal(ra[key][R:], rb_[key], err_msg=key)
        for g, o in enumerate(want):
            assert_matches(TIGHT, ra, g, o)
        plain = make_engine(c, None, 1, ensemble=fr.device(fl, 0))
        try:
            assert 'devices' not in plain.plan and plain.devices == 0
        finally:
            plain.close()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize('name,path,plan', BIT_PATHS, ids=[row[0] for row in BIT_PATHS])
def test_two_evaluations_are_bit_identical(name, path, plan):
    c, fl, xs, _ = parity_reference('unitary', 3, 2)
    eng = make_engine(c, fl, F * R, path)
    try:
        eng.set_base(xs)
        first = eng.evaluate()
        eng.set_base(xs)
        second = eng.evaluate()
        for key in KEYS + ('grad',):
            np.testing.assert_array_equal(first[key], second[key], err_msg=key)
    finally:
        eng.close()


GRAPE_CONV = {'rate': 0.02, 'update_step': 7, 'max_iterations': 20, 'conv_target': 1e-12, 'learning_rate_decay': 100}


def test_grape_fleet_against_one_robust_call_per_device():
    """n = 3, F = 3 devices of 3 members, restarts = 2, 20 Adam iterations, a fixed Taylor order: every device's final loss and pulse against
    Grape(robust=device f, restarts=2) from the same NumPy seed.  The loss at TIGHT; the pulse, as tests/test_robust_families.py bounds a base after a
    loop, to 1e-9 max(maxA)."""
    c = fr.problem('unitary', n=3, m=3, steps=12, regs={'dwdt': 0.01}, seed=5)
    fl = fr.make_fleet(c, F, 3, 1, seed=4)
    kw = dict(convergence=dict(GRAPE_CONV), U0=c['U0'], reg_coeffs=c['reg_coeffs'], maxA=list(c['maxA']), method='Adam', Taylor_terms=[8, 1], restarts=2)
    np.random.seed(31)
    uks, Uf = _grape(*grape_args(c), fleet=fl, **kw)
    assert uks.shape == (F, 2, 12) and Uf.shape == (F, 3, 3) and fl.losses.shape == (F,) and fl.member_losses.shape == (F, 3)
    assert fl.best.shape == (F,) and list(fl.iterations) == [20] * F
    for f in range(F):
        info = {}
        np.random.seed(31)
        u1, U1 = _grape(*grape_args(c), robust=fr.device(fl, f), _restart_info=info, **kw)
        best = int(info['best'])
        print('device %d: fleet loss %.17g (restart %d), robust loss %.17g (restart %d)' % (f, fl.losses[f], fl.best[f], info['loss'][best], best))
        assert fl.best[f] == best
        assert abs(fl.losses[f] - info['loss'][best]) <= TIGHT['s'] * max(1.0, abs(info['loss'][best])), (f, fl.losses[f], info['loss'][best])
        assert np.max(np.abs(uks[f] - u1)) <= 1e-9 * np.max(c['maxA']) and np.max(np.abs(Uf[f] - U1)) <= 1e-9


class _Log(object):
    """Stands where data_management.H5File stands (h5py is optional): keeps what add() is given, by file."""
    files = {}

    def __init__(self, path):
        self.data = self.files.setdefault(path, {})

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def add(self, key, data=None):
        self.data[key] = np.array(data)

    def append(self, key, data, force_append=False):
        self.data.setdefault(key, [])

    def create_group(self, name):
        return self

    def create_dataset(self, key, data=None):
        pass


def test_grape_fleet_fills_the_line_the_map_and_the_run_log(tmp_path, monkeypatch):
    """transfer.samples (F, k, P), control_map.coefficients (F, r, steps), and the run log's fleet_* datasets."""
    from quantum_optimal_control.helper_functions import data_management
    from quantum_optimal_control.main_grape.grape import Grape
    monkeypatch.setattr(data_management, 'H5File', _Log)
    c = fr.problem('unitary', k=2, r=3, steps=12, regs={'dwdt': 0.01}, seed=6)
    fl = fr.make_fleet(c, F, 2, 1, seed=4)
    cm, hold = ref.make_map(2, 3, 2, 12, mix=True, fixed=True, seed=4), tf.hold(12, 5)
    conv = dict(GRAPE_CONV, max_iterations=4)
    np.random.seed(8)
    with contextlib.redirect_stdout(io.StringIO()):
        uks, Uf = Grape(*grape_args(c), convergence=conv, U0=c['U0'], reg_coeffs=c['reg_coeffs'], maxA=list(c['maxA']), fleet=fl, transfer=hold, control_map=cm,
                        restarts=2, show_plots=False, save=True, file_name='fleet', data_path=str(tmp_path), Taylor_terms=[8, 1])
    assert uks.shape == (F, 2, 12) and hold.samples.shape == (F, 2, 5) and cm.coefficients.shape == (F, 3, 12)
    for f in range(F):
        assert np.max(np.abs(uks[f] - hold.samples[f] @ hold.matrix.T)) <= 1e-14
        want = cmap.apply(cm, fl.amp_scales[f, 0][:, None] * uks[f])
        assert np.max(np.abs(cm.coefficients[f] - want)) <= 1e-13 * max(1.0, np.max(np.abs(want)))
    log = _Log.files[os.path.join(str(tmp_path), '00000_fleet.h5')]
    assert np.array_equal(log['fleet_offsets'], fl.offsets) and np.array_equal(log['fleet_amp_scales'], fl.amp_scales)
    assert np.array_equal(log['fleet_uks'], uks) and np.array_equal(log['fleet_losses'], fl.losses) and 'wall_clock_time' in log


def test_fleet_example_runs_with_a_short_budget():
    """examples/fleet_qubit_pi_pulses.py, 40 iterations: the shapes, and what must hold after any budget -- a qubit's own pulse is no worse on it than
    the nominal pulse is only once optimised, so that is NOT asserted here; the scan of the nominal pulse must be worst far from the nominal qubit."""
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import fleet_qubit_pi_pulses as ex
    with contextlib.redirect_stdout(io.StringIO()) as out:
        nominal, own, worst = ex.main(iterations=40, quiet=True)
    assert nominal.shape == own.shape == worst.shape == (ex.QUBITS,)
    assert np.all(np.isfinite(nominal)) and np.all(np.isfinite(own)) and np.all(np.isfinite(worst))
    assert np.all(worst >= 0) and np.all(own >= 0)
    assert len([ln for ln in out.getvalue().splitlines() if ln[:5].strip().isdigit()]) == ex.QUBITS
