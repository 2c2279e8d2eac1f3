"""Randomised differential tests of the glue between the views of an ensemble engine: robust ensembles, risk, transfer lines, control maps, device
fleets, open-system members and sparse operators, drawn together by tests/glue_fuzz_cases.py (96 closed dense, 32 open, 32 sparse seeds) and held
to the references composed from the unchanged oracle.

The unmarked tests run on the CPU and keep the families honest: every draw is well conditioned as drawn, devices and members are far enough
apart that a kernel reading another one's rows cannot pass, and the draws reach the shapes the glue kernels change their path at.  The `gpu`
tests run every draw on every kernel family that takes it.

Bounds (the project's own: tests/test_robust_gpu.py, tests/test_control_map_gpu.py, tests/test_robust_families.py):
  scalars 1e-12 of max(1, |reference|); the gradient and every read-back 1e-11 of max(1, largest reference entry); after four Adam iterations
  bases and scalars 1e-10; L-BFGS steps as tests/test_lbfgs_gpu.py: compare_with_reference bounds them.
Every assertion message carries the family, the seed and the drawn dict."""
import collections

import numpy as np
import pytest

from tests import glue_fuzz_cases as gz
from tests.fleet_reference import swapped_apart

gpu = pytest.mark.gpu
S_RTOL, G_RTOL, LOOP_TOL = 1e-12, 1e-11, 1e-10
KEYS = ('loss', 'reg_loss', 'grad_squared', 'unitary_scale')
PATHS = ('auto', 'generic', 'mfma', 'gemm', 'st_fused')


def draws(family):
    fn, count = gz.FAMILIES[family]
    return [fn(seed) for seed in range(count)]


def lbfgs_seeds():
    """Every fourth of the closed seeds that drew the exact gradient."""
    return [d.seed for d in draws('closed') if d.exact][::4]


# ---- CPU: the families themselves -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('family', list(gz.FAMILIES))
def test_every_draw_is_well_conditioned_as_drawn(family):
    """Every expected value finite and every member's unitary_scale in [0.5, 2], for every committed seed: there is no re-draw rule to hide behind."""
    ds = draws(family)
    assert [d.seed for d in ds] == list(range(gz.FAMILIES[family][1])) and len(ds) == dict(closed=96, open=32, sparse=32)[family]
    for d in ds:
        want = d.expected()
        assert len(want) == d.G == d.xs.shape[0], d.tag()
        for g, o in enumerate(want):
            for key, v in o.items():
                if v is not None:
                    assert np.all(np.isfinite(np.asarray(v, dtype=np.complex128))), (d.tag(), g, key)
            us = o['member_unitary_scale']
            assert us.shape == (d.info['E'],) and np.all(us >= 0.5) and np.all(us <= 2.0), (d.tag(), g, us)


@pytest.mark.parametrize('family', list(gz.FAMILIES))
def test_devices_and_members_are_apart(family):
    """At ONE start point (control set 0's).  F > 1: the devices' expected losses and gradients lie more than 1e-6 apart, so a kernel that reads the
    rows of device 0 or of device g % F misses by decades.  E > 1: so do the members' losses.  (Six decades above the bounds; at the other start
    points a pair of members may come closer by chance, never the ensembles as a whole.)"""
    for d in draws(family):
        first = d.expected()[0]
        if d.F > 1:
            at_one = [first] + [d.evaluate_at(f * d.R, d.xs[0]) for f in range(1, d.F)]
            assert swapped_apart([o['loss'] for o in at_one]) and swapped_apart([o['grad'] for o in at_one]), d.tag()
        if d.info['E'] > 1:
            assert swapped_apart(list(first['member_loss'])), (d.tag(), first['member_loss'])


def size_class(n):
    return '<=12' if n <= 12 else '13-32' if n <= 32 else '33-48' if n <= 48 else '49-64' if n <= 64 else '>64'


def count(ds, what):
    return sum(1 for d in ds if what(d.info))


def test_closed_family_covers_the_glue_shapes():
    ds = draws('closed')
    need = {
        'a column window > 32': (6, lambda i: i['window'] > 32),
        'a column window > 64': (3, lambda i: i['window'] > 64),
        'beta > 0 with E > 1': (25, lambda i: i['beta'] > 0 and i['E'] > 1),
        'a map': (40, lambda i: bool(i['map'])),
        'r + q = 9': (2, lambda i: i['r'] + i['q'] == 9),
        'F > 1': (50, lambda i: i['F'] > 1),
        'R > 1': (40, lambda i: i['F'] > 0 and i['R'] > 1),
        'a nominal ensemble': (3, lambda i: i['E'] == 1 and i['q'] == 0),
        'a zero weight': (4, lambda i: i['zero_weight'] >= 0),
        'n <= 12': (4, lambda i: i['n'] <= 12),
        'the exact gradient': (15, lambda i: i['exact']),
        'unitary mode': (30, lambda i: i['mode'] == 'unitary'),
        'state transfer': (30, lambda i: i['mode'] == 'state'),
        'a lossy drift': (2, lambda i: i['lossy']),
    }
    need.update({'line ' + kind: (8, lambda i, kind=kind: i['line'] == kind) for kind in gz.LINES})
    need.update({'n ' + cls: (6, lambda i, cls=cls: size_class(i['n']) == cls) for cls in ('<=12', '13-32', '33-48', '49-64', '>64')})
    got = {name: count(ds, what) for name, (_, what) in need.items()}
    print(got)
    short = {name: (got[name], least) for name, (least, _) in need.items() if got[name] < least}
    assert not short, short
    # the shapes no hand-picked file draws, together: the second trip of the lane loop under a risk and a map; r + q = 9 on a fleet; a zero weight
    # under a tilt beyond device 0; and each of them where another kernel family runs the trajectories
    assert count(ds, lambda i: i['window'] > 64 and i['beta'] > 0 and i['E'] > 1 and bool(i['map'])) >= 1
    assert count(ds, lambda i: i['r'] + i['q'] == 9 and i['F'] > 0) >= 1
    assert count(ds, lambda i: i['zero_weight'] >= 0 and i['beta'] > 0 and i['F'] > 1) >= 1
    assert all(count(ds, lambda i, n=n: i['n'] == n) >= 1 for n in (33, 49, 65))
    assert len(lbfgs_seeds()) >= 3


def test_open_and_sparse_families_cover_their_shapes():
    od, sd = draws('open'), draws('sparse')
    need_open = {'c = 0': (1, lambda i: i['c'] == 0), 'c > 0': (12, lambda i: i['c'] > 0), 'F > 1': (10, lambda i: i['F'] > 1), 'a map': (10, lambda i: bool(i['map'])),
                 'a line': (12, lambda i: i['line'] != 'none'), 'beta > 0 with E > 1': (6, lambda i: i['beta'] > 0 and i['E'] > 1), 'unitary mode': (8, lambda i: i['mode'] == 'unitary'),
                 'state transfer': (8, lambda i: i['mode'] == 'state'), 'n > 16': (6, lambda i: i['n'] > 16), 'an ensemble without a fleet': (5, lambda i: i['F'] == 0)}
    need_sparse = {'merged rows': (8, lambda i: i['row_layout'] == 2), 'rows per operator': (8, lambda i: i['row_layout'] == 1), 'vectors in LDS': (8, lambda i: i['vector_home'] == 'lds'),
                   'vectors in global memory': (8, lambda i: i['vector_home'] == 'global'), 'a fleet': (10, lambda i: i['F'] > 0), 'F > 1': (8, lambda i: i['F'] > 1),
                   'a map': (10, lambda i: bool(i['map'])), 'a line': (6, lambda i: i['line'] != 'none'), 'q > 0': (12, lambda i: i['q'] > 0),
                   'beta > 0 with E > 1': (6, lambda i: i['beta'] > 0 and i['E'] > 1), 'n >= 100': (8, lambda i: i['n'] >= 100)}
    for ds, need in ((od, need_open), (sd, need_sparse)):
        got = {name: count(ds, what) for name, (_, what) in need.items()}
        print(got)
        short = {name: (got[name], least) for name, (least, _) in need.items() if got[name] < least}
        assert not short, short
    for d in od:                                                  # inside what qoc_create_open_fleet documents
        i = d.info
        assert i['n'] <= 32 and i['c'] <= 8 and i['m'] <= i['n'] and (i['c'] + 4) * i['n'] * (i['n'] | 1) * 16 <= 159 * 1024 and i['taylor'][0] <= 60, d.tag()
        assert not set(i['regs']) & {'forbidden_coeff_list', 'speed_up'}, d.tag()
    for d in sd:                                                  # a line on sparse operators: the ctypes helper takes no fleet and no regulariser
        assert d.T is None or (d.fleet is None and not d.c.reg_coeffs), d.tag()


def test_route_predicate_admits_every_family_often_enough():
    ds = draws('closed')
    got = {path: sum(1 for d in ds if gz.eligible(d, path)) for path in PATHS}
    print(got)
    assert got['auto'] == got['generic'] == 96 and got['mfma'] >= 40 and got['gemm'] >= 60 and got['st_fused'] >= 10, got


def test_lbfgs_draws_decide_their_line_searches_by_a_margin():
    """The L-BFGS rows compare branch by branch (tests/test_lbfgs_gpu.py: compare_with_reference): every Armijo and curvature decision of the
    reference on these draws is taken by more than that file's margin, so rounding cannot flip one."""
    from tests import lbfgs_reference
    from tests.test_lbfgs_gpu import BASE, assert_margins
    for seed in lbfgs_seeds():
        d = gz.closed(seed)
        rec = lbfgs_reference.run(lambda x: d.evaluate_at(d.G - 1, x), d.xs[d.G - 1], dict(BASE, max_iterations=3), 3)
        assert_margins(rec)


# ---- GPU: every draw on every kernel family that takes it -------------------------------------------------------------------------------------------

WORST = collections.defaultdict(float)                            # kind of figure -> the largest error / bound seen in this process (printed per test)


def close_to(what, got, want, rtol, tag):
    """|got - want| <= rtol max(1, largest |want|); the figure error / max(1, .) joins WORST under the kind `what` starts with."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, what, got.shape, want.shape)
    err = float(np.max(np.abs(got - want))) if want.size else 0.0
    top = max(1.0, float(np.max(np.abs(want)))) if want.size else 1.0
    kind = what.split(' ')[0]
    WORST[kind] = max(WORST[kind], err / top)
    assert err <= rtol * top, '%s: %s off by %.3e (bound %.1e of %.3e)' % (tag, what, err, rtol, top)


def report(tag):
    print('%s: worst error over bound base so far: %s' % (tag, {key: '%.2e' % v for key, v in sorted(WORST.items())}))


def plan_words(d):
    want = dict(members=str(d.info['E']), perturbations=str(d.info['q']))
    want['devices'] = str(d.F) if d.fleet is not None else None
    want['terms'] = str(d.cm.n_terms) if d.cm is not None else None
    want['degree'] = str(d.cm.degree) if d.cm is not None else None
    return want


def assert_plan(d, eng, tag):
    for key, want in plan_words(d).items():
        assert eng.plan.get(key) == want, (tag, key, want, eng.plan)


def read_backs(d, eng):
    """Everything the draw's engine can be asked for after an evaluation."""
    out = dict(member_loss=eng.member_scalars()['loss'], weights=eng.member_weights(), uks=eng.get_uks())
    if d.cm is not None:
        out['coefficients'] = eng.get_coefficients()
    if d.T is not None:
        out['pulse'] = eng.get_pulse()
    if d.family == 'open':
        out.update(rho=eng.get_final_density(), member_rho=eng.member_final_density(), populations=eng.get_populations())
    else:
        out['inter'] = eng.get_inter_vecs()
        if d.family == 'closed' and not d.c['state_transfer']:
            out.update(Uf=eng.get_final_unitary(), member_U=eng.member_final_unitary())
    return out


def check_evaluation(d, eng, tag):
    """Checks 1 to 4: the plan words, evaluate() and the read-backs of every control set against its device's reference, and a second evaluation
    bit for bit.  Returns (evaluation, read-backs)."""
    assert_plan(d, eng, tag)
    eng.set_base(d.xs)
    r = eng.evaluate()
    rb = read_backs(d, eng)
    assert r['grad'].shape == d.xs.shape, (tag, r['grad'].shape)
    e = d.info.get('member', 0)
    for g, o in enumerate(d.expected()):
        at = '%s set %d (device %d)' % (tag, g, d.device_of(g))
        for key in KEYS:
            close_to('scalar %s' % key, r[key][g], o[key], S_RTOL, at)
        close_to('gradient', r['grad'][g], o['grad'], G_RTOL, at)
        close_to('readback member_loss', rb['member_loss'][g], o['member_loss'], G_RTOL, at)
        close_to('readback weights', rb['weights'][g], o['weights'], G_RTOL, at)
        close_to('readback uks', rb['uks'][g], o['uks'], G_RTOL, at)
        if d.cm is not None:
            close_to('readback coefficients', rb['coefficients'][g], o['coefficients'], G_RTOL, at)
        if d.T is not None:
            close_to('readback pulse', rb['pulse'][g], o['pulse'], G_RTOL, at)
        if d.family == 'open':
            close_to('readback rho_final', rb['rho'][g], o['rho_final'], G_RTOL, at)
            close_to('readback populations', rb['populations'][g], o['populations'], G_RTOL, at)
            close_to('readback member_rho[%d]' % e, rb['member_rho'][g][e], o['member_rho'][e], G_RTOL, at)
        else:
            close_to('readback inter_vecs', rb['inter'][g], o['inter_vecs'], G_RTOL, at)
        if 'Uf' in rb:
            close_to('readback U_final', rb['Uf'][g], o['U_final'], G_RTOL, at)
            close_to('readback member_U[%d]' % e, rb['member_U'][g][e], o['member_U'][e], G_RTOL, at)
    r2 = eng.evaluate()
    rb2 = read_backs(d, eng)
    for key in KEYS + ('grad',):
        assert np.array_equal(r[key], r2[key]), '%s: %s of a second evaluation differs' % (tag, key)
    for key in rb:
        assert np.array_equal(rb[key], rb2[key]), '%s: %s read back after a second evaluation differs' % (tag, key)
    return r, rb


def check_adam(d, eng, tag):
    """Check 5: four Adam iterations in one iterate call against run_adam over the reference; then the scalars where the loop ended."""
    eng.set_base(d.xs)
    eng.iterate(eng.adam_params(poll_every=3, **gz.ADAM), 4)
    base = eng.get_base()
    its = eng.scalars()['iterations']
    assert list(its) == [4] * d.G, (tag, its)
    r = eng.evaluate()
    for g in range(d.G):
        o = d.adam_reference(g)
        assert o['iterations'] == 4
        at = '%s set %d after 4 Adam iterations' % (tag, g)
        close_to('loop_base', base[g], o['base'], LOOP_TOL, at)
        for key in ('loss', 'reg_loss'):
            close_to('loop_scalar %s' % key, r[key][g], o[key], LOOP_TOL, at)


def envelope_of(d):
    return gz.envelope_constant(d.info['k'], d.info['steps']) if 'envelope' in d.info['regs'] else None


def closed_engine(d, path, chunks=0, n_sets=None, fleet='own', ens='own', exact=None):
    from quantum_optimal_control.core import hip_engine as P
    from tests import control_map_reference as ref
    sp, c = ref.engine_system(d.c), d.c
    fleet = d.fleet if fleet == 'own' else fleet
    ens = (None if fleet is not None else d.ens) if ens == 'own' else ens
    return P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, c['maxA'], sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, state_transfer=sp.state_transfer,
                       reg_coeffs=c['reg_coeffs'], one_minus_gauss=envelope_of(d), n_seeds=d.G if n_sets is None else n_sets, path=path, chunks=chunks, ensemble=ens,
                       transfer=d.T, exact_gradient=d.exact if exact is None else exact, control_map=d.cm, fleet=fleet)


@gpu
@pytest.mark.parametrize('seed', range(gz.CLOSED_SEEDS))
def test_closed_draw_on_every_kernel_family(seed):
    """AUTO, the generic path and each of MFMA, GEMM and ST_FUSED: the library accepts a draw exactly where gz.eligible says so, and every accepted
    engine passes checks 1 to 4; the AUTO engine also runs the Adam loop."""
    from quantum_optimal_control.core import hip_engine as P
    d = gz.closed(seed)
    i = d.info
    routes = (('auto', P.PATH_AUTO, 0), ('generic', P.PATH_GENERIC, 0), ('mfma', P.PATH_MFMA, i['mfma_chunks']), ('gemm', P.PATH_GEMM, i['gemm_chunks']),
              ('st_fused', P.PATH_ST_FUSED, 0))
    for name, path, chunks in routes:
        tag = '%s path %s chunks %d' % (d.tag(), name, chunks)
        try:
            eng = closed_engine(d, path, chunks)
        except P.QocError as err:
            assert not gz.eligible(d, name), '%s: refused where the documented limits admit it: %s' % (tag, err)
            continue
        try:
            assert gz.eligible(d, name), '%s: accepted where the documented limits refuse it: %s' % (tag, eng.plan)
            got = eng.plan['path']
            if name == 'auto':
                assert got != 'small' and (i['r'] + i['q'] < 9 or got not in ('mfma', 'st_fused')) and (not d.exact or got == 'generic'), (tag, eng.plan)
            else:
                assert got == name, (tag, eng.plan)
            check_evaluation(d, eng, tag)
            if name == 'auto':
                check_adam(d, eng, tag)
        finally:
            eng.close()
    report(d.tag())


@gpu
@pytest.mark.parametrize('seed', lbfgs_seeds())
def test_closed_draw_lbfgs_steps(seed):
    """Check 6: three steps of the device L-BFGS on the draw's LAST control set (the comparison steps one control set, so a fleet is cut down to that
    set's device, whose rows are not device 0's), against tests/lbfgs_reference.py driven by the exact reference."""
    from quantum_optimal_control.core import hip_engine as P
    from quantum_optimal_control.helper_functions import fleet as fl_mod
    from tests.test_lbfgs_gpu import BASE, compare_with_reference
    d = gz.closed(seed)
    g = d.G - 1
    one = None
    if d.fleet is not None:
        f, fl = d.device_of(g), d.fleet
        one = fl_mod.validate(fl_mod.Fleet(fl.operators, fl.offsets[f:f + 1], fl.amp_scales[f:f + 1], weights=fl.weights, risk=fl.risk), d.info['n'], d.info['k'])
    eng = closed_engine(d, P.PATH_GENERIC, n_sets=1, fleet=one, ens=None if one is not None else d.ens, exact=True)
    try:
        rec, worst = compare_with_reference(eng, lambda x: d.evaluate_at(g, x), d.xs[g], dict(BASE, max_iterations=3), 3, name=d.tag())
        WORST['lbfgs_base'] = max(WORST['lbfgs_base'], worst)
    finally:
        eng.close()
    report(d.tag())


def open_engine(d):
    from quantum_optimal_control.core import hip_engine as P
    from tests import open_fleet_reference as ofr
    p = d.c
    sp = ofr.engine_system(p)
    return P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, p['maxA'], sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, state_transfer=sp.state_transfer,
                       reg_coeffs=p['reg_coeffs'], one_minus_gauss=envelope_of(d), n_seeds=d.G, ensemble=None if d.fleet is not None else d.ens, transfer=d.T,
                       control_map=d.cm, fleet=d.fleet)


@gpu
@pytest.mark.parametrize('seed', range(gz.OPEN_SEEDS))
def test_open_draw(seed):
    """Members that decay, every one with its own row of rate scales: checks 1 to 5 on the one path an open engine has."""
    d = gz.opened(seed)
    eng = open_engine(d)
    try:
        assert eng.plan['path'] == 'lindblad' and eng.plan['collapse'] == str(d.info['c']), (d.tag(), eng.plan)
        check_evaluation(d, eng, d.tag())
        check_adam(d, eng, d.tag())
    finally:
        eng.close()
    report(d.tag())


def sparse_engine(d, layout):
    from tests.test_sparse_ensemble_gpu import make_engine
    ens = None if d.fleet is not None else dict(d.ens, risk=d.beta)
    if d.T is not None:
        return make_engine(d.c, d.G, ens, transfer=d.T, control_map=d.cm, row_layout=layout)
    return make_engine(d.c, d.G, ens, control_map=d.cm, fleet=d.fleet, row_layout=layout, vector_home=d.info['vector_home'])


@gpu
@pytest.mark.parametrize('seed', range(gz.SPARSE_SEEDS))
def test_sparse_draw(seed):
    """Sparse operators through the same funnel: checks 1 to 4 on the drawn row layout and on the other one, whose every figure is EQUAL; check 5
    on the drawn layout."""
    d = gz.sparse(seed)
    seen = {}
    for layout in (d.info['row_layout'], 3 - d.info['row_layout']):
        tag = '%s layout %d' % (d.tag(), layout)
        eng = sparse_engine(d, layout)
        try:
            assert eng.plan['path'] == 'sparse' and eng.plan['rows'] == ('merged' if layout == 2 else 'per_operator'), (tag, eng.plan)
            if d.T is None:
                assert eng.plan['vector_home'] == d.info['vector_home'], (tag, eng.plan)
            r, rb = check_evaluation(d, eng, tag)
            seen[layout] = dict(rb, **{key: r[key] for key in KEYS + ('grad',)})
            if layout == d.info['row_layout']:
                check_adam(d, eng, tag)
        finally:
            eng.close()
    for key in seen[1]:
        assert np.array_equal(seen[1][key], seen[2][key]), '%s: %s differs between the row layouts' % (d.tag(), key)
    report(d.tag())
