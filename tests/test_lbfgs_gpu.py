"""The device-resident L-BFGS loop (qoc_iterate_lbfgs / qoc_run_lbfgs, csrc/qoc_lbfgs.h) against its NumPy specification
(tests/lbfgs_reference.py: plain two-loop recursion on explicit vectors), step by step.

1. engine vs the reference driven by a second engine's own evaluate(): the same function on both sides, so what is compared is the step kernel --
   Gram-form recursion, multi-value reduction, ring of pairs, flags -- at every element count at which its launch or the mode-0 tail changes
2. engine vs the reference driven by the CPU oracle  3. one short row per engine kind  4. three control sets that stop at different evaluations
5. determinism  6. refusals through the raw ABI  7. qoc_set_base, a changed history, Adam afterwards  8. Grape(method='LBFGS') end to end

In every row the reference's Armijo margin f - (f_acc + c1 alpha gp) and its curvature margin sy - 1e-10 yy stay away from zero by more than
1e-9 max(1, |f|) (asserted), so that rounding cannot flip a branch; the starting seeds were picked with the oracle as the evaluator."""
import contextlib
import ctypes
import functools
import io
import os
import sys

import numpy as np
import pytest

from oracle import grape_oracle as go
from quantum_optimal_control.core import hip_engine
from tests import lbfgs_reference as ref
from tests.golden import cases
from tests.helpers import oracle_system
from tests.test_adam_tail import LOOP_ATOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
P = hip_engine
MARGIN = 1e-9
BASE = dict(conv_target=1e-9, min_grad=1e-25, max_iterations=100)

# name: (k, steps, seed of the problem and its start, parameters, J); n = 3, m = 2, slices of 0.02
ROWS = {
    'ks3': (3, 1, 42, {}, 8),
    'ks255': (5, 51, 42, {}, 8),                 # accept, rejections, accept
    'ks256': (8, 32, 42, {}, 8),
    'ks257': (1, 257, 42, {}, 8),                # more elements than the 256 threads
    'ks1025': (5, 205, 41, {}, 8),
    'ks2048': (8, 256, 42, {}, 6),               # the 1024-thread launch
    'ks4100': (5, 820, 43, {}, 6),               # mode 0 through the split tail
    'ks8195': (5, 1639, 42, {}, 6),              # more than eight elements per thread
    'wrap': (2, 20, 42, dict(history=3), 12),    # the history wraps from the sixth evaluation on
    'c1': (2, 20, 42, dict(c1=0.9), 10),         # runs of rejections
    'max_ls1': (2, 20, 41, dict(c1=0.9, max_ls=1), 10),           # the direction is reset
    'max_it4': (2, 20, 42, dict(c1=0.9, max_iterations=4), 8),    # a refused trial at the limit: restore, then stop
    # more than QOC_LBFGS_COLS = 8 stored pairs: k_lbfgs_step forms its dots in further sub-passes, the Gram matrix grows to 33 x 33, the ring wraps at 16.
    # Seeds and J chosen on the oracle (CPU) so that the margins stay wide: 'ks2048' seeds 41 .. 48 fall below 1e-8 from the 12th evaluation on.
    # Measured on an MI355X against the reference driven by the twin engine: 3.8e-12 over the 40 steps of history16, 1.3e-13 (history9), 1.4e-16 (ks2048)
    'history16': (2, 20, 42, dict(history=16), 40),               # 37 accepted, 3 rejected; 16 live pairs from evaluation 19 on, 20 wraps; worst margin 1.9e-6
    'history9': (2, 20, 42, dict(history=9), 24),                 # the count crosses 8 with the last sub-pass partly filled; wraps from evaluation 11; 1.5e-5
    'history16_ks2048': (8, 256, 45, dict(history=16), 11),       # ten pairs on the 1024-thread launch; worst margin 4e-7
}
ORACLE_ROWS = [r for r in ROWS if ROWS[r][0] * ROWS[r][1] <= 1025]
EXPECT = {'wrap': 'wrapped', 'c1': ref.REJECT, 'max_ls1': ref.RESET, 'max_it4': ref.RESTORE, 'ks255': ref.REJECT, 'history16': 'wrapped', 'history9': 'wrapped'}
PAIRS = {'history16': 16, 'history9': 9, 'history16_ks2048': 10}          # the pairs alive after the row's last evaluation


@functools.lru_cache(maxsize=None)
def system(k, steps, seed, n=3, m=2):
    c = cases.case_c2(n=n, k=k, steps=steps, m=m, taylor=(4, 1), seed=seed)
    c['reg_coeffs'] = {}
    c['total_time'] = 0.02 * steps
    return oracle_system(c)


def row(name):
    k, steps, seed, extra, J = ROWS[name]
    return system(k, steps, seed), dict(BASE, **extra), J


def make_engine(sp, n_seeds=1, path=P.PATH_GENERIC, variant=0, **kw):
    return P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, state_transfer=sp.state_transfer,
                       reg_coeffs=sp.reg_coeffs, one_minus_gauss=sp.one_minus_gauss, Vs=sp.Vs, n_seeds=n_seeds, path=path, variant=variant, **kw)


def lbfgs_params(p, poll_every=5):
    return P.HipEngine.lbfgs_params(poll_every=poll_every, **p)


def engine_evaluator(eng):
    """x -> the engine's own evaluation of control set 0 at x (every set is given x)."""
    def evaluate(x):
        eng.set_base(np.broadcast_to(x, eng._seed_shape()))
        r = eng.evaluate()
        return dict(reg_loss=r['reg_loss'][0], grad=r['grad'][0], loss=r['loss'][0], grad_squared=r['grad_squared'][0])
    return evaluate


def oracle_evaluator(sp):
    return lambda x: go.evaluate(sp, x)


def step_engine(eng, params, bases, J):
    """J times one loop iteration from `bases` [n_seeds][...]: per step the evaluated points, the points after the step and the scalars."""
    eng.set_base(bases)
    out = dict(points=[], next=[], scalars=[])
    for _ in range(J):
        out['points'].append(eng.get_base())
        eng.iterate_lbfgs(params, 1)
        out['next'].append(eng.get_base())
        out['scalars'].append(eng.scalars())
    return out


def infer_branches(points, nexts, iters, dones, p):
    """What the engine did at every evaluation, from what it shows: its counters and how the variable moved."""
    p = dict(ref.DEFAULTS, **p)
    out, x_acc, it_prev = [], None, 0
    for x, nx, it, done in zip(points, nexts, iters, dones):
        if done:
            assert it == it_prev and np.array_equal(nx, x)
            out.append(ref.STOP)
            break
        if it == it_prev:                              # no trial counted: the variable went back to the accepted point
            assert x_acc is not None and np.array_equal(nx, x_acc)
            out.append(ref.RESTORE if it_prev >= p['max_iterations'] else ref.STALL)
            continue
        assert it == it_prev + 1
        it_prev = it
        if x_acc is None:
            out.append(ref.ACCEPT)
            x_acc = x
            continue
        d_prev, d_new = (x - x_acc).ravel(), (nx - x_acc).ravel()
        if np.allclose(d_new, p['shrink'] * d_prev, rtol=1e-9, atol=1e-14):
            out.append(ref.REJECT)                     # the same direction, the step shrunk
        elif abs(np.linalg.norm(d_new) - 1.0) < 1e-9:
            out.append(ref.RESET)                      # x_acc kept, a unit step along the steepest descent
        else:
            out.append(ref.ACCEPT)
            x_acc = x
    return out


def assert_margins(rec):
    for f, margin, curv in zip(rec['f'], rec['margin'], rec['curvature']):
        for v in (margin, curv):
            assert v is None or abs(v) > MARGIN * max(1.0, abs(f)), (f, margin, curv)


def compare_with_reference(eng, evaluate, x0, p, J, name='', with_f=False):
    """The engine's J steps from x0 (control set 0 of one) against the reference driven by `evaluate`; the largest |base - reference|."""
    rec = ref.run(evaluate, x0, p, J)
    assert_margins(rec)
    got = step_engine(eng, lbfgs_params(p), x0[None], J)
    n = len(rec['branch'])
    worst = max(float(np.max(np.abs(got['next'][j][0] - rec['next'][j]))) for j in range(n))
    print('%s: branches %s, worst |base - reference| %.3e' % (name, ' '.join(rec['branch']), worst))
    branches = infer_branches([q[0] for q in got['points']], [q[0] for q in got['next']], [int(s['iterations'][0]) for s in got['scalars']],
                              [int(s['done'][0]) for s in got['scalars']], p)
    assert branches == rec['branch'], (branches, rec['branch'])
    for j in range(n):
        np.testing.assert_allclose(got['next'][j][0], rec['next'][j], rtol=0, atol=LOOP_ATOL, err_msg='step %d (%s)' % (j, rec['branch'][j]))
        if with_f:
            assert abs(got['scalars'][j]['reg_loss'][0] - rec['f'][j]) <= LOOP_ATOL, (j, got['scalars'][j]['reg_loss'][0], rec['f'][j])
    for j in range(n, J):                              # a finished control set is evaluated where it stands
        assert np.array_equal(got['next'][j], got['next'][n - 1]) and int(got['scalars'][j]['done'][0]) == 1
    assert int(got['scalars'][-1]['iterations'][0]) == rec['state'].iters
    return rec, worst


# ---- 1. step by step against the reference on the engine's own evaluations ------------------------------------------------------------------

@pytest.mark.parametrize('name', list(ROWS))
def test_steps_follow_the_reference(name):
    sp, p, J = row(name)
    eng, twin = make_engine(sp), make_engine(sp)
    try:
        assert eng.path == P.PATH_GENERIC
        if name == 'ks4100':
            assert eng.plan['tail'].startswith('split'), eng.plan
        rec, _ = compare_with_reference(eng, engine_evaluator(twin), sp.base0, p, J, name)
        if name in EXPECT:
            assert rec['wrapped'] if EXPECT[name] == 'wrapped' else EXPECT[name] in rec['branch'], rec['branch']
        if name in PAIRS:
            assert len(rec['state'].S) == PAIRS[name] > 8, (len(rec['state'].S), rec['branch'])
            if name == 'history16_ks2048':
                assert sp.k * sp.steps >= 2048
    finally:
        eng.close()
        twin.close()


# ---- 2. against the oracle -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ORACLE_ROWS)
def test_steps_follow_the_reference_on_the_oracle(name):
    sp, p, J = row(name)
    eng = make_engine(sp)
    try:
        compare_with_reference(eng, oracle_evaluator(sp), sp.base0, p, min(J, 10), name, with_f=True)
    finally:
        eng.close()


# ---- 3. every engine kind --------------------------------------------------------------------------------------------------------------------

def _closed(path, variant=0, n=3, m=2, k=4, steps=40, **kw):
    sp = system(k, steps, 44, n, m)
    return (lambda: make_engine(sp, 1, path, variant, **kw)), sp.base0


def _state_transfer():
    c = cases.case_c3(n=4, k=2, steps=30, taylor=(6, 0), seed=43)
    c['reg_coeffs'] = {'forbidden_coeff_list': [50.0], 'states_forbidden_list': [3]}
    c['total_time'] = 0.02 * 30
    sp = oracle_system(c)
    return (lambda: make_engine(sp, 1, P.PATH_ST_FUSED)), sp.base0


def _ensemble():
    from tests import test_robust_gpu as rg
    c = rg.problem('unitary', 'none')
    ens, sp = rg.ensemble(c, 3, 1), rg.nominal_system(c)
    return (lambda: rg.make_engine(sp, 1, ens)), sp.base0


def _shaped():
    from quantum_optimal_control.helper_functions import transfer as tf
    sp = system(2, 40, 44)
    T = tf.hold(40, 10).matrix
    x0 = np.random.default_rng(3).normal(0, 1 / np.sqrt(10), (2, 10))
    return (lambda: make_engine(sp, 1, P.PATH_AUTO, transfer=T)), x0


def _open():
    from tests import test_open_system_gpu as og
    sp, ops = og.system('n3_c1')
    return (lambda: og.make_engine(sp, ops)), sp.base0


KINDS = {
    'generic': (lambda: _closed(P.PATH_GENERIC, n=5, m=3, k=2, steps=30), 'generic'),
    'mfma_batch8': (lambda: _closed(P.PATH_MFMA, 8, n=17, m=3, k=2, steps=24), 'mfma'),      # the in-place exponentials are a 16 < n <= 32 kernel
    'mfma_latency5': (lambda: _closed(P.PATH_MFMA, 5), 'mfma'),
    'gemm': (lambda: _closed(P.PATH_GEMM), 'gemm'),
    'st_fused': (_state_transfer, 'st_fused'),
    'small': (lambda: _closed(P.PATH_SMALL), 'small'),
    'ensemble_E3': (_ensemble, None),
    'shaped_P10': (_shaped, None),
    'exact_gradient': (lambda: _closed(P.PATH_AUTO, exact_gradient=True), 'generic'),
    'open_n3_c1': (_open, 'lindblad'),
}


@pytest.mark.parametrize('kind', list(KINDS))
def test_every_engine_kind_runs_the_loop(kind):
    build, path = KINDS[kind]
    make, x0 = build()
    eng, twin = make(), make()
    try:
        if path is not None:
            assert eng.plan['path'] == path, eng.plan
        if kind == 'mfma_batch8':                      # the kernel family asked for, not a fall-back: the in-place exponentials, batch sweeps
            assert int(eng.plan['expm']) == 8 and not eng.plan['sweeps'].startswith('latency'), eng.plan
        if kind == 'mfma_latency5':
            assert int(eng.plan['expm']) == 5 and eng.plan['sweeps'].startswith('latency') and eng.plan['tail'].startswith('latency_fused'), eng.plan
        compare_with_reference(eng, engine_evaluator(twin), np.array(x0), dict(BASE), 6, kind)
    finally:
        eng.close()
        twin.close()


# ---- 4. three control sets that stop at different evaluations -------------------------------------------------------------------------------------

def test_three_control_sets_stop_on_their_own():
    sp = system(5, 51, 41)
    bases = np.stack([sp.base0, 0.6 * sp.base0 + 0.1, -0.8 * sp.base0 + 0.05])
    J, max_it = 14, 10
    free = dict(BASE, conv_target=-1.0, max_iterations=max_it)
    hist = [ref.run(oracle_evaluator(sp), b, free, J) for b in bases]
    # a target that exactly one control set reaches, and well before the others run into max_iterations: between two neighbouring losses of all
    # evaluations (half way in the logarithm), the candidate that keeps every loss furthest away
    losses = np.sort(np.concatenate([h['loss'] for h in hist]))
    best = None
    for lo, hi in zip(losses[:-1], losses[1:]):
        t = float(np.sqrt(lo * hi))
        first = [next((j for j, l in enumerate(h['loss']) if l < t), None) for h in hist]
        margin = min(abs(l - t) / t for l in losses)
        if sum(f is not None for f in first) == 1 and max(f for f in first if f is not None) <= max_it - 3 and (best is None or margin > best[0]):
            best = (margin, t)
    assert best is not None and best[0] > 1e-3, best
    target = best[1]
    p = dict(free, conv_target=target)
    recs = [ref.run(oracle_evaluator(sp), b, p, J) for b in bases]
    for r in recs:
        assert_margins(r)
        assert r['state'].done and min(abs(l - target) for l in r['loss']) > 1e-6 * target
    stops = [len(r['branch']) for r in recs]
    assert len(set(stops)) >= 2 and sum(r['loss'][-1] < target for r in recs) == 1, stops
    eng = make_engine(sp, 3)
    try:
        got = step_engine(eng, lbfgs_params(p), bases, J)
    finally:
        eng.close()
    keys = ('loss', 'reg_loss', 'grad_squared', 'unitary_scale', 'iterations', 'done')
    for b in range(3):
        assert [int(s['done'][b]) for s in got['scalars']] == [0] * (stops[b] - 1) + [1] * (J - stops[b] + 1), (b, stops)
        for j in range(stops[b], J):                   # finished: nothing of the set changes any more, bit for bit
            assert np.array_equal(got['next'][j][b], got['next'][stops[b] - 1][b])
            for key in keys:
                assert got['scalars'][j][key][b] == got['scalars'][stops[b] - 1][key][b], (b, j, key)
        np.testing.assert_allclose(got['next'][-1][b], recs[b]['x'], rtol=0, atol=LOOP_ATOL)
        single = make_engine(sp, 1)
        try:
            alone = step_engine(single, lbfgs_params(p), bases[b][None], J)
        finally:
            single.close()
        for j in range(J):
            assert np.array_equal(alone['next'][j][0], got['next'][j][b]), (b, j)
            for key in keys:
                assert alone['scalars'][j][key][0] == got['scalars'][j][key][b], (b, j, key)


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------------------------

def _run(eng, bases, p, poll_every=5):
    eng.set_base(bases)
    its = eng.run_lbfgs(lbfgs_params(p, poll_every))
    s = eng.scalars()
    return dict(base=eng.get_base(), its=its, **{key: s[key] for key in ('loss', 'reg_loss', 'grad_squared', 'iterations', 'done')})


def _same(a, b):
    return all(np.array_equal(a[key], b[key]) for key in a)


def test_run_lbfgs_is_deterministic():
    sp = system(5, 205, 41)
    bases = np.stack([sp.base0, 0.6 * sp.base0 + 0.1])
    p = dict(BASE, max_iterations=12, history=3)
    runs = []
    for _ in range(2):
        eng = make_engine(sp, 2)
        try:
            runs.append(_run(eng, bases, p))
        finally:
            eng.close()
    assert _same(runs[0], runs[1])
    assert np.all(runs[0]['done'] == 1) and np.all(runs[0]['its'] == runs[0]['iterations']) and np.all(runs[0]['its'] <= 12)
    assert np.all(runs[0]['loss'] < 0.5 * go.evaluate(sp, bases[0])['loss'])


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------

def _raw(eng, call, params):
    lib = P.load_library()
    arg = None if params is None else ctypes.byref(params)
    rc = getattr(lib, call)(eng._h, arg, 1 if call == 'qoc_iterate_lbfgs' else None)
    return rc, lib.qoc_last_error().decode()


@pytest.mark.parametrize('call', ['qoc_iterate_lbfgs', 'qoc_run_lbfgs'])
def test_bad_parameters_are_refused_by_name(call):
    sp = system(2, 20, 42)
    eng = make_engine(sp)
    try:
        eng.set_base(sp.base0[None])
        for bad, word in ((None, 'null params'), (dict(history=0), 'history'), (dict(history=17), 'history'), (dict(c1=0.0), 'c1'), (dict(c1=1.0), 'c1'),
                          (dict(shrink=0.0), 'shrink'), (dict(shrink=1.0), 'shrink'), (dict(max_ls=0), 'max_ls'), (dict(c1=float('nan')), 'c1')):
            rc, msg = _raw(eng, call, None if bad is None else lbfgs_params(dict(BASE, **bad)))
            assert rc == -1 and msg.startswith(call + ':') and word in msg, (bad, rc, msg)
        assert np.array_equal(eng.get_base()[0], sp.base0) and int(eng.scalars()['iterations'][0]) == 0       # nothing ran
        rc, msg = _raw(eng, call, lbfgs_params(dict(BASE, max_iterations=3)))
        assert rc == 0, msg
    finally:
        eng.close()


def test_time_sharded_engines_refuse_the_loop():
    c = cases.case_c2(n=100, k=3, steps=48, m=4, taylor=(5, 2), seed=21)
    c['total_time'] = 2.0
    sp = oracle_system(c)
    eng = make_engine(sp, 1, P.PATH_AUTO, time_shards=2, time_rank=-1)
    try:
        eng.set_base(sp.base0[None])
        for call in ('qoc_iterate_lbfgs', 'qoc_run_lbfgs'):
            rc, msg = _raw(eng, call, lbfgs_params(BASE))
            assert rc == -1 and msg.startswith(call + ':') and 'time-sharded' in msg, (rc, msg)
        with pytest.raises(P.QocError, match='qoc_run_lbfgs: .*time-sharded'):
            eng.run_lbfgs(lbfgs_params(BASE))
    finally:
        eng.close()


# ---- 7. set_base, another history, Adam afterwards ----------------------------------------------------------------------------------------------

def test_set_base_resets_the_loop_and_adam_is_untouched():
    sp = system(5, 51, 42)
    bases = np.stack([sp.base0, 0.6 * sp.base0 + 0.1])
    p = dict(BASE, max_iterations=9, history=3)
    long = dict(BASE, history=3)                                      # (the counters are not part of what a changed history resets: keep the limit away)
    adam = P.HipEngine.adam_params(rate=0.02, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=50, poll_every=3)
    eng, fresh = make_engine(sp, 2), make_engine(sp, 2)
    try:
        first = _run(eng, bases, p)
        assert not np.array_equal(first['base'], bases)
        assert _same(first, _run(eng, bases, p))                       # set_base: history, direction, flags and counters start over
        # another history between calls: the state starts over from where the variable stands
        p, q = long, dict(long, history=5)
        eng.set_base(bases)
        eng.iterate_lbfgs(lbfgs_params(p), 4)
        mid = eng.get_base()
        eng.iterate_lbfgs(lbfgs_params(q), 4)
        fresh.set_base(mid)
        fresh.iterate_lbfgs(lbfgs_params(q), 4)
        assert np.array_equal(eng.get_base(), fresh.get_base()) and not np.array_equal(eng.get_base(), mid)
        eng.iterate_lbfgs(lbfgs_params(p), 3)                          # ... and back to a history the allocation already holds
        fresh.set_base(fresh.get_base())
        fresh.iterate_lbfgs(lbfgs_params(p), 3)
        assert np.array_equal(eng.get_base(), fresh.get_base())
        # an Adam burst after an L-BFGS burst: what a fresh engine gives from the same base
        start = eng.get_base()
        eng.set_base(start)
        eng.iterate(adam, 7)
        clean = make_engine(sp, 2)
        try:
            clean.set_base(start)
            clean.iterate(adam, 7)
            a, b = eng.scalars(), clean.scalars()
            assert np.array_equal(eng.get_base(), clean.get_base()) and not np.array_equal(eng.get_base(), start)
            assert all(np.array_equal(a[key], b[key]) for key in a)
            assert np.array_equal(eng.get_uks(), clean.get_uks())
        finally:
            clean.close()
    finally:
        eng.close()
        fresh.close()


# ---- 8. Grape(method='LBFGS') ---------------------------------------------------------------------------------------------------------------------

def test_grape_lbfgs_reaches_the_coarse_qutrit_gate_within_four_times_scipys_evaluations():
    """Ten slices of 1 ns, exact gradient, target 1e-10: scipy's L-BFGS-B (strong-Wolfe search with interpolation) sets the count; the device loop
    (backtracking without interpolation) gets four times that as its whole budget -- a guard against a wrong direction, not a performance claim."""
    import coarse_qutrit_x_gate as coarse
    from quantum_optimal_control.main_grape.grape import Grape
    conv = dict(coarse.CONVERGENCE, conv_target=1e-10)
    scipy_run = coarse.run(True, convergence=dict(conv))
    assert scipy_run['infidelity'] < 2e-10
    budget = 4 * scipy_run['evaluations']
    H0, Hops, names, U = coarse.problem()
    np.random.seed(4)
    with contextlib.redirect_stdout(io.StringIO()):
        uks, _, loss = Grape(H0, Hops, names, U, coarse.TOTAL_TIME, coarse.STEPS, [0, 1], maxA=coarse.MAXA, reg_coeffs={}, method='LBFGS', show_plots=False,
                             save=False, Taylor_terms=coarse.TAYLOR, convergence=dict(conv, max_iterations=budget - 2), exact_gradient=True,
                             _return_session=True)
    print('L-BFGS-B: %d evaluations; LBFGS: budget %d, loss %.3e, re-simulated %.3e' % (
        scipy_run['evaluations'], budget, loss, coarse.infidelity(H0, Hops, U, uks, coarse.TOTAL_TIME)))
    assert loss < 1e-10 and coarse.infidelity(H0, Hops, U, uks, coarse.TOTAL_TIME) < 2e-10


def test_grape_lbfgs_restarts_are_independent_runs():
    import lbfgs_restarts as ex
    r = ex.run(restarts=4, convergence=dict(ex.CONVERGENCE, max_iterations=60, conv_target=1e-10))
    assert r['base'].shape == (4, 2, 10) and r['loss'].shape == (4,)
    for a in range(4):
        for b in range(a + 1, 4):
            assert not np.array_equal(r['base'][a], r['base'][b])
    best = int(np.argmin(r['loss']))
    np.testing.assert_allclose(r['uks'], np.array(ex.coarse.MAXA)[:, None] * np.sin(r['base'][best]), rtol=0, atol=1e-15)
    others = [b for b in range(4) if b != best]
    assert all(np.max(np.abs(r['uks'] - np.array(ex.coarse.MAXA)[:, None] * np.sin(r['base'][b]))) > 1e-6 for b in others)
    assert abs(r['infidelity'] - r['loss'][best]) < 1e-9
