"""Control maps on the GPU: a mapped engine (hip_engine.HipEngine(control_map=...), qoc_create_mapped) against the expected values composed from
the unchanged oracle (tests/control_map_reference.py) -- every map shape, with and without M and F, members and a line, on every kernel family an
ensemble can run on --, the bit identity of the identity map with the same engine without a map, determinism, the capped grid of the two glue
kernels, the edges of a map, the device loops, the C refusals, and the capability itself through Grape(control_map=...).

Tolerances are the project's own for ensemble parity (tests/test_robust_gpu.py): 1e-12 relative on scalars, 1e-11 of the largest entry on gradients
and vectors."""
import contextlib
import functools
import io
import os
import sys

import numpy as np
import pytest

from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import control_map as cmap
from quantum_optimal_control.helper_functions import robust as rb
from quantum_optimal_control.helper_functions import transfer as tf
from tests import control_map_reference as ref
from tests.test_adam_tail import _choose_target
from tests.test_lbfgs_gpu import BASE as LBFGS_BASE
from tests.test_lbfgs_gpu import compare_with_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G_RTOL, S_RTOL = 1e-11, 1e-12
P = hip_engine
REGS = {'dwdt': 0.1, 'amplitude': 0.2, 'forbidden_coeff_list': [5.0], 'states_forbidden_list': [3], 'speed_up': 0.3}
STEPS, SAMPLES = 10, 4                                   # hold(10, 4): windows of 3, 2, 3, 2 slices


# ---- problems and engines ---------------------------------------------------------------------------------------------------------------------

def problem(kind, r, k, regs=True, n=5, m=3, steps=STEPS):
    st = kind == 'state'
    return ref.problem(n, r, k, steps, 2 if st else m, state_transfer=st, taylor=(8, 0) if st else (6, 1), seed=7 + r + 10 * k, regs=REGS if regs else {})


def make_engine(c, cm, ens, G, T=None, path=P.PATH_AUTO, variant=0, chunks=0, exact=False):
    sp = ref.engine_system(c)
    return P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, c['maxA'], sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, state_transfer=sp.state_transfer,
                       reg_coeffs=c['reg_coeffs'], n_seeds=G, path=path, variant=variant, chunks=chunks, ensemble=ens, transfer=T, exact_gradient=exact,
                       control_map=cm)


def line(with_line, steps=STEPS):
    return tf.hold(steps, SAMPLES).matrix if with_line else None


@functools.lru_cache(maxsize=None)
def reference(kind, k, r, D, mf, Eq, with_line):
    """The composed expected values of a row at its three variables: computed once, shared by every path and batch size."""
    c = problem(kind, r, k)
    cm = ref.make_map(k, r, D, STEPS, mix=mf, fixed=mf)
    ens = ref.ensemble(c, *Eq)
    T = line(with_line)
    xs = ref.variables(k, SAMPLES if with_line else STEPS, 3)
    return c, cm, ens, T, xs, [ref.evaluate(c, cm, ens, x, T=T) for x in xs]


def assert_matches(r, g, o, what=('loss', 'reg_loss', 'grad_squared', 'unitary_scale')):
    for key in what:
        print('%s[%d]: engine %.17g composed %.17g' % (key, g, r[key][g], o[key]))
        assert abs(r[key][g] - o[key]) <= S_RTOL * max(1.0, abs(o[key])), (key, g, r[key][g], o[key])
    gm = max(1.0, float(np.max(np.abs(o['grad']))))
    err = float(np.max(np.abs(r['grad'][g] - o['grad'])))
    print('grad[%d]: max error %.3e of max %.3e' % (g, err, gm))
    assert err <= G_RTOL * gm, (g, err)


def check_evaluation(row, G, path=P.PATH_AUTO, variant=0, chunks=0, plan=None):
    c, cm, ens, T, xs, refs = row
    eng = make_engine(c, cm, ens, G, T, path, variant, chunks)
    try:
        for key, val in dict(plan or {}, terms=str(cm.n_terms), degree=str(cm.degree), members=str(len(ens['weights'])),
                             perturbations=str(len(ens['operators']))).items():
            assert eng.plan.get(key) == val, (key, val, eng.plan)       # the plan first
        assert eng.path != P.PATH_SMALL and 'latency' not in eng.plan.get('sweeps', '')
        eng.set_base(xs[:G])
        r = eng.evaluate()
        ms, coeff, inter, uks = eng.member_scalars(), eng.get_coefficients(), eng.get_inter_vecs(), eng.get_uks()
        assert r['grad'].shape == xs[:G].shape and coeff.shape == (G, cm.n_terms, c['steps'])
        for g in range(G):
            o = refs[g]
            assert_matches(r, g, o)
            assert np.max(np.abs(ms['loss'][g] - o['member_loss'])) <= S_RTOL * max(1.0, np.max(np.abs(o['member_loss'])))
            for name, got, want in (('inter_vecs', inter[g], o['inter_vecs']), ('coefficients', coeff[g], o['coefficients']), ('uks', uks[g], o['uks'])):
                err, top = float(np.max(np.abs(got - want))), max(1.0, float(np.max(np.abs(want))))
                print('%s[%d]: max error %.3e of max %.3e' % (name, g, err, top))
                assert err <= G_RTOL * top, (name, g, err)
            if T is not None:
                assert np.max(np.abs(eng.get_pulse()[g] - o['pulse'])) <= G_RTOL * max(1.0, np.max(np.abs(o['pulse'])))
    finally:
        eng.close()


# ---- 1. parity with the composed oracle ---------------------------------------------------------------------------------------------------------

MAPS = [(2, 3, 3), (3, 2, 1), (1, 1, 2)]                 # (k, r, D)
ROWS = [pytest.param(k, r, D, mf, Eq, wl, G, id='k%dr%dD%d-%s-E%dq%d-%s-G%d' % (k, r, D, 'MF' if mf else 'bare', Eq[0], Eq[1], 'hold' if wl else 'direct', G))
        for (k, r, D) in MAPS for mf in (False, True) for Eq in ((1, 0), (3, 1)) for wl in (False, True) for G in (1, 3)]


@pytest.mark.parametrize('k,r,D,mf,Eq,with_line,G', ROWS)
def test_evaluation_matches_the_composed_oracle(k, r, D, mf, Eq, with_line, G):
    """Every map shape, with and without M (signed, slice-dependent) and F, one nominal member and three members with a perturbation, with and
    without a hold line of uneven windows, one and three control sets: the generic path, unitary mode, pulse and state regularisers."""
    check_evaluation(reference('unitary', k, r, D, mf, Eq, with_line), G, P.PATH_GENERIC, plan=dict(path='generic'))


FAMILIES = [
    ('generic_state', 'state', P.PATH_GENERIC, 0, 0, dict(path='generic')),
    ('mfma_nt1', 'unitary', P.PATH_MFMA, 0, 0, dict(path='mfma', nt='1')),
    ('gemm_unitary', 'unitary', P.PATH_GEMM, 0, 0, dict(path='gemm', route='unitary')),
    ('gemm_direct', 'state', P.PATH_GEMM, 0, 1, dict(path='gemm', route='direct')),
    ('st_fused', 'state', P.PATH_ST_FUSED, 0, 0, dict(path='st_fused')),
]


@pytest.mark.parametrize('name,kind,path,variant,chunks,plan', FAMILIES, ids=[f[0] for f in FAMILIES])
@pytest.mark.parametrize('k,r,D', MAPS)
def test_every_kernel_family_runs_a_map(name, kind, path, variant, chunks, plan, k, r, D):
    """One row per family an ensemble can run on beside the generic unitary rows above (both modes of the generic path, MFMA nt = 1, the GEMM
    unitary route, the GEMM direct state-transfer route, ST_FUSED): M and F, three members with a perturbation, the hold line, three control sets."""
    check_evaluation(reference(kind, k, r, D, True, (3, 1), True), 3, path, variant, chunks, plan)


@functools.lru_cache(maxsize=None)
def wide_row(r):
    c = ref.problem(4, r, 2, 6, 2, taylor=(6, 1), seed=40 + r, regs=REGS)
    cm = ref.make_map(2, r, 2, 6, mix=True, fixed=True, seed=r)
    ens = ref.ensemble(c, 2, 1)
    xs = ref.variables(2, 6, 1)
    return c, cm, ens, None, xs, [ref.evaluate(c, cm, ens, xs[0])]


def test_eight_trajectory_controls_on_the_mfma_path():
    """r + q = 8: the most the MFMA path takes."""
    check_evaluation(wide_row(7), 1, P.PATH_MFMA, plan=dict(path='mfma'))


def test_nine_trajectory_controls_under_auto():
    """r + q = 9: AUTO plans for the trajectories' controls and leaves the paths limited to 8; asking for one by name is refused."""
    row = wide_row(8)
    check_evaluation(row, 1, P.PATH_AUTO)
    eng = make_engine(*row[:3], 1)
    try:
        assert eng.plan['path'] not in ('mfma', 'st_fused', 'small'), eng.plan
    finally:
        eng.close()
    with pytest.raises(P.QocError, match=r'qoc_create_mapped: path 2 is limited to 8 controls; the ensemble\'s trajectories have r \+ q = 9'):
        make_engine(*row[:3], 1, path=P.PATH_MFMA)


# ---- 2. the identity map, determinism ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('path', [P.PATH_GENERIC, P.PATH_MFMA, P.PATH_GEMM], ids=['generic', 'mfma', 'gemm'])
@pytest.mark.parametrize('with_line', [False, True], ids=['direct', 'hold'])
def test_identity_map_is_bit_identical_to_no_map(path, with_line):
    """r = k, D = 1, alpha = I, no M, no F: every product is by 1.0 or 0.0 and every added term a zero.  Ten Adam iterations of three members."""
    c = problem('unitary', 3, 3)
    ens, T = ref.ensemble(c, 3, 1), line(with_line)
    xs = ref.variables(3, SAMPLES if with_line else STEPS, 2)
    conv = dict(rate=0.02, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=10, poll_every=3)
    out = []
    for cm in (None, cmap.identity(3)):
        eng = make_engine(c, cm, ens, 2, T, path)
        try:
            assert ('terms' in eng.plan) == (cm is not None), eng.plan
            eng.set_base(xs)
            first = eng.evaluate()
            its = eng.run_adam(eng.adam_params(**conv))
            out.append(dict(first, its=its, base=eng.get_base(), uks=eng.get_uks(), inter=eng.get_inter_vecs(), Uf=eng.get_final_unitary(),
                            member_loss=eng.member_scalars()['loss'], **{'final_' + key: v for key, v in eng.scalars().items()}))
            if cm is not None:
                v = eng.get_pulse() if with_line else eng.get_uks(evaluated=True)
                assert np.array_equal(eng.get_coefficients(), ens['amp_scales'][0][None, :, None] * v)
        finally:
            eng.close()
    assert np.all(out[0]['its'] == 10)
    for key in out[0]:
        np.testing.assert_array_equal(out[0][key], out[1][key], err_msg=key)


@pytest.mark.parametrize('path', [P.PATH_GENERIC, P.PATH_MFMA], ids=['generic', 'mfma'])
def test_two_evaluations_are_bit_identical(path):
    c, cm, ens, T, xs, _ = reference('unitary', 2, 3, 3, True, (3, 1), True)
    eng = make_engine(c, cm, ens, 3, T, path)
    try:
        eng.set_base(xs)
        a, ca = eng.evaluate(), eng.get_coefficients()
        b, cb = eng.evaluate(), eng.get_coefficients()
        for key in a:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
        np.testing.assert_array_equal(ca, cb)
    finally:
        eng.close()


# ---- 3. the capped grid ---------------------------------------------------------------------------------------------------------------------

def test_more_items_than_the_capped_grid_has_threads():
    """n = 2, r = k = 8, 1000 slices, 66 control sets: 528000 items through k_map_expand and through k_map_reduce, more than the 2048 x 256
    threads of the capped grid, so that the last control sets are reached by the stride alone.  The sets cycle through three variables: sets 0, 1
    and 2 are checked against the composed oracle, every other set against the set that shares its variable."""
    steps, G = 1000, 66
    c = ref.problem(2, 8, 8, steps, 2, taylor=(5, 1), seed=50, total_time=8.0, regs={'amplitude': 0.2})
    cm = ref.make_map(8, 8, 2, steps, mix=True, fixed=True, seed=9)
    ens = ref.ensemble(c, 1, 0)
    xs = ref.variables(8, steps, 3)
    eng = make_engine(c, cm, ens, G)
    try:
        eng.set_base(xs[np.arange(G) % 3])
        r, coeff = eng.evaluate(), eng.get_coefficients()
    finally:
        eng.close()
    assert G * 8 * steps > 2048 * 256
    for g in range(3):
        o = ref.evaluate(c, cm, ens, xs[g])
        assert_matches(r, g, o)
        assert np.max(np.abs(coeff[g] - o['coefficients'])) <= G_RTOL * max(1.0, np.max(np.abs(o['coefficients'])))
    for g in range(3, G):
        np.testing.assert_array_equal(coeff[g], coeff[g % 3], err_msg='coefficients of set %d' % g)
        gm = max(1.0, float(np.max(np.abs(r['grad'][g % 3]))))
        assert np.max(np.abs(r['grad'][g] - r['grad'][g % 3])) <= G_RTOL * gm, g
        assert abs(r['loss'][g] - r['loss'][g % 3]) <= S_RTOL


# ---- 4. edges -------------------------------------------------------------------------------------------------------------------------------

def test_edges_of_a_map():
    """One map with: alpha that zeroes the pair (operator 0, pulse 1); pulse 0 feeding operators 0 and 1 with different polynomials; operator 2 fed
    by F alone.  Three members, the second with weight zero."""
    k, r, D, steps = 2, 3, 3, STEPS
    rng = np.random.default_rng(77)
    alpha = np.zeros((r, k, D))
    alpha[0, 0] = [1.0, 0.3, -0.2]
    alpha[1, 0] = [-0.4, 0.0, 0.5]
    alpha[1, 1] = [0.9, -0.1, 0.0]
    cm = cmap.validate(cmap.ControlMap(alpha, rng.uniform(-1, 1, size=(r, k, steps)), rng.uniform(-0.5, 0.5, size=(r, steps))), k=k, r=r, steps=steps)
    c = problem('unitary', r, k)
    ens = ref.ensemble(c, 3, 1)
    ens = rb.validate(dict(ens, weights=[0.5, 0.0, 0.5]), 5, k)
    xs = ref.variables(k, steps, 2)
    row = (c, cm, ens, None, xs, [ref.evaluate(c, cm, ens, x) for x in xs])
    for path in (P.PATH_GENERIC, P.PATH_MFMA):
        check_evaluation(row, 2, path)
    assert np.array_equal(row[5][0]['coefficients'][2], cm.fixed[2])          # the operator the pulses do not reach runs its fixed waveform


# ---- 5. device loops --------------------------------------------------------------------------------------------------------------------------

def loop_row():
    c, cm, ens, T, xs, _ = reference('unitary', 2, 3, 3, True, (3, 1), True)
    return c, cm, ens, T, xs[:2]


def test_adam_loop_matches_a_python_loop_over_the_reference():
    """G = 2, 10 iterations: conv_target is chosen so that one control set stops inside a burst of 4 and finishes beside one that runs on."""
    c, cm, ens, T, xs = loop_row()
    conv = dict(rate=0.05, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=10)

    def python_loop(x0, conv):
        return ref.run_adam(lambda x: ref.evaluate(c, cm, ens, x, T=T), x0, conv)

    free = [python_loop(x, conv) for x in xs]
    target, stops = _choose_target([f['history'] for f in free], 10)
    conv['conv_target'] = target
    refs = [python_loop(x, conv) for x in xs]
    assert [r['iterations'] for r in refs] == stops and any(0 < s < 10 and s % 4 != 0 for s in stops), stops
    eng = make_engine(c, cm, ens, 2, T, P.PATH_GENERIC)
    try:
        eng.set_base(xs)
        its = eng.run_adam(eng.adam_params(poll_every=4, **conv))
        s, base = eng.scalars(), eng.get_base()
        for g, o in enumerate(refs):
            assert its[g] == o['iterations'], (its, stops)
            assert np.max(np.abs(base[g] - o['base'])) < 1e-9, np.max(np.abs(base[g] - o['base']))
            assert abs(s['loss'][g] - o['loss']) < 1e-10 * max(1.0, abs(o['loss']))
            assert abs(s['reg_loss'][g] - o['reg_loss']) < 1e-10 * max(1.0, abs(o['reg_loss']))
    finally:
        eng.close()


def test_lbfgs_run_follows_the_reference():
    """tests/lbfgs_reference.py driven by the composed reference (the exact gradient, so that the Armijo test sees the derivative of the loss)."""
    c, cm, ens, T, xs = loop_row()
    eng = make_engine(c, cm, ens, 1, T, P.PATH_GENERIC, exact=True)
    try:
        compare_with_reference(eng, lambda x: ref.evaluate(c, cm, ens, x, T=T, exact=True), xs[0], dict(LBFGS_BASE, max_iterations=8), 8, name='mapped')
    finally:
        eng.close()


def test_risk_ensemble_through_a_map():
    c, cm, ens, T, xs, _ = reference('unitary', 2, 3, 3, True, (3, 1), True)
    eng = make_engine(c, cm, dict(ens, risk=5.0), 3, T, P.PATH_GENERIC)
    try:
        assert eng.risk == 5.0
        eng.set_base(xs)
        r, pi = eng.evaluate(), eng.member_weights()
        for g in range(3):
            o = ref.evaluate(c, cm, ens, xs[g], T=T, beta=5.0)
            assert_matches(r, g, o, what=('loss', 'reg_loss', 'grad_squared'))
            assert np.max(np.abs(pi[g] - o['weights'])) <= S_RTOL
    finally:
        eng.close()


@pytest.mark.parametrize('kind', ['unitary', 'state'])
def test_exact_gradient_through_a_map(kind):
    """gradient = 1 against the exact reference, and against central differences of the engine's own reg_loss with the step and the bound of
    tests/test_exact_gradient.py (h = 1e-6, 1e-7 of the gradient's largest entry)."""
    c, cm, ens, T, xs, _ = reference(kind, 2, 3, 3, True, (3, 1), True)
    eng = make_engine(c, cm, ens, 1, T, exact=True)
    try:
        assert eng.plan['path'] == 'generic' and eng.plan['gradient'] == 'exact', eng.plan
        x = xs[0]
        eng.set_base(x[None])
        r = eng.evaluate()
        assert_matches(r, 0, ref.evaluate(c, cm, ens, x, T=T, exact=True))

        def own(y):
            eng.set_base(y[None])
            return float(eng.evaluate(want_grad=False)['reg_loss'][0])
        fd = ref.central_differences(own, x, h=1e-6)
        gmax, err = float(np.max(np.abs(r['grad'][0]))), float(np.max(np.abs(r['grad'][0] - fd)))
        print('exact gradient against central differences of the engine: max error %.3e of max %.3e' % (err, gmax))
        assert err <= 1e-7 * max(gmax, 1e-3), (err, gmax)
    finally:
        eng.close()


# ---- 6. refusals, lifetime --------------------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def tampered(change):
    """Lets `change(cfg, map)` alter the structs HipEngine hands to qoc_create_mapped (it may return 'null map'): what the Python layer would
    refuse itself reaches the library."""
    lib = P.load_library()
    real = lib.qoc_create_mapped

    def call(cfg, ens, tr, mp, *rest):
        if change(cfg._obj, mp._obj) == 'null map':
            mp = None
        return real(cfg, ens, tr, mp, *rest)
    lib.qoc_create_mapped = call
    try:
        yield
    finally:
        lib.qoc_create_mapped = real


def _set(obj, **kw):
    for key, v in kw.items():
        setattr(obj, key, v)


def _poke(arr, idx, v):
    arr[idx] = v


C_REFUSALS = [
    ('null_map', lambda cfg, mp: 'null map', 'qoc_create_mapped: the control map is missing'),
    ('null_poly', lambda cfg, mp: _set(mp, poly=None), r'qoc_create_mapped: the map\'s polynomial coefficients \(poly\) are missing'),
    ('no_terms', lambda cfg, mp: _set(mp, n_terms=0), r'qoc_create_mapped: n_terms = 0 \(1 .. 64 operators\)'),
    ('many_terms', lambda cfg, mp: _set(mp, n_terms=65), r'qoc_create_mapped: n_terms = 65 \(1 .. 64 operators\)'),
    ('degree_0', lambda cfg, mp: _set(mp, degree=0), r'qoc_create_mapped: degree = 0 \(1 .. 8\)'),
    ('degree_9', lambda cfg, mp: _set(mp, degree=9), r'qoc_create_mapped: degree = 9 \(1 .. 8\)'),
    ('poly_nan', lambda cfg, mp: _poke(mp.poly, 7, float('nan')), r'qoc_create_mapped: poly\[1\]\[0\]\[1\] is not finite'),
    ('mix_inf', lambda cfg, mp: _poke(mp.mix, STEPS + 2, float('inf')), r'qoc_create_mapped: mix\[0\]\[1\]\[2\] is not finite'),
    ('fixed_nan', lambda cfg, mp: _poke(mp.fixed, STEPS + 3, float('nan')), r'qoc_create_mapped: fixed\[1\]\[3\] is not finite'),
    ('dead_pulse_poly', lambda cfg, mp: [_poke(mp.poly, (i * 2 + 1) * 3 + d, 0.0) for i in range(3) for d in range(3)],
     'qoc_create_mapped: pulse 1 reaches no operator'),
    ('dead_pulse_mix', lambda cfg, mp: [_poke(mp.mix, (i * 2 + 0) * STEPS + t, 0.0) for i in range(3) for t in range(STEPS)],
     'qoc_create_mapped: pulse 0 reaches no operator'),
    ('time_shards', lambda cfg, mp: _set(cfg, time_shards=2), 'qoc_create_mapped: an ensemble cannot be time-sharded'),
    ('small_path', lambda cfg, mp: _set(cfg, path=P.PATH_SMALL), 'qoc_create_mapped: the workgroup-resident path'),
    ('latency', lambda cfg, mp: _set(cfg, variant=5), 'qoc_create_mapped: the latency mode of the MFMA path'),
    ('envelope_on_samples', lambda cfg, mp: _set(cfg, has_envelope=1), 'qoc_create_mapped: the envelope regulariser is defined per time slice'),
    ('bad_weight', None, 'qoc_create_mapped: weight 1 is'),
    ('no_samples', None, r'qoc_create_mapped: n_samples = 0'),
]


@pytest.mark.parametrize('name,change,msg', C_REFUSALS, ids=[row[0] for row in C_REFUSALS])
def test_the_library_refuses_by_message(name, change, msg):
    c, cm, ens, T, xs, _ = reference('unitary', 2, 3, 3, True, (3, 1), True)
    cm = cmap.validate(cmap.ControlMap(cm.alpha.copy(), cm.mix.copy(), cm.fixed.copy()))     # (the tampering writes into these arrays)
    if name == 'bad_weight':
        ens = dict(ens, weights=np.array([0.5, -0.25, 0.75]))
    if name == 'no_samples':
        T = np.zeros((STEPS, 0))
    with tampered(change or (lambda cfg, mp: None)):
        with pytest.raises(P.QocError, match=msg):
            make_engine(c, cm, ens, 1, T)


def test_create_destroy_and_the_read_backs_of_other_engines():
    c, cm, ens, T, xs, _ = reference('unitary', 2, 3, 3, True, (3, 1), False)
    for _ in range(3):
        eng = make_engine(c, cm, ens, 2)
        with pytest.raises(P.QocError, match='qoc_get_coefficients: nothing evaluated yet'):
            eng.get_coefficients()
        eng.set_base(xs[:2])
        eng.evaluate()
        assert eng.get_coefficients().shape == (2, 3, STEPS)
        eng.close()
        eng.close()
    c3 = problem('unitary', 3, 3)
    plain = make_engine(c3, None, ref.ensemble(c3, 3, 1), 1)          # an ensemble engine without a map
    try:
        with pytest.raises(P.QocError, match=r'qoc_get_coefficients: not a mapped engine \(qoc_create_mapped\)'):
            plain.get_coefficients()
        assert 'terms' not in plain.plan and 'degree' not in plain.plan
    finally:
        plain.close()


# ---- 7. the capability itself -------------------------------------------------------------------------------------------------------------------

def _grape(*args, **kw):
    from quantum_optimal_control.main_grape.grape import Grape
    with contextlib.redirect_stdout(io.StringIO()):
        return Grape(*args, save=False, show_plots=False, **kw)


@pytest.mark.parametrize('method', ['Adam', 'LBFGS', 'L-BFGS-B'])
def test_grape_through_a_constant_linear_map_equals_grape_on_hand_mixed_operators(method):
    """c = X v with a constant 3 x 2 matrix X is the plain problem on the two operators H_j = sum_i X[i, j] G_i: the same pulse, to rounding."""
    c = ref.problem(4, 3, 2, 12, 4, taylor=(6, 1), seed=60, total_time=3.0)
    X = np.array([[1.0, 0.1], [-0.2, 1.0], [0.3, 0.4]])
    mixed = [sum(X[i, j] * c['Hops'][i] for i in range(3)) for j in range(2)]
    guess = 0.3 * np.sin(np.linspace(0.0, 3.0, 12))[None, :] * np.array([[1.0], [-0.5]])
    conv = {'rate': 0.02, 'update_step': 10, 'max_iterations': 12, 'conv_target': 1e-12, 'learning_rate_decay': 100}
    kw = dict(convergence=conv, U0=c['U0'], reg_coeffs={'dwdt': 0.01}, maxA=[1.0, 1.2], initial_guess=guess, method=method, Taylor_terms=[8, 2])
    cm = cmap.linear(X)
    uks_map, Uf_map = _grape(c['H0'], c['Hops'], ['a', 'b'], c['U'], c['total_time'], 12, [0, 1, 2, 3], control_map=cm, **kw)
    uks_mix, Uf_mix = _grape(c['H0'], mixed, ['a', 'b'], c['U'], c['total_time'], 12, [0, 1, 2, 3], **kw)
    assert uks_map.shape == (2, 12) and cm.coefficients.shape == (3, 12)
    assert np.max(np.abs(uks_map - uks_mix)) <= 1e-9, np.max(np.abs(uks_map - uks_mix))
    assert np.max(np.abs(Uf_map - Uf_mix)) <= 1e-9
    assert np.max(np.abs(cm.coefficients - X @ uks_map)) <= 1e-14


def test_grape_combines_a_map_with_robust_transfer_exact_gradient_and_restarts():
    c = ref.problem(4, 3, 2, 12, 4, taylor=(6, 1), seed=61, total_time=3.0)
    cm = ref.make_map(2, 3, 3, 12, mix=True, fixed=True, seed=4)
    ens = ref.ensemble(c, 3, 1)
    hold = tf.hold(12, 5)
    conv = {'rate': 0.02, 'update_step': 10, 'max_iterations': 8, 'conv_target': 1e-12, 'learning_rate_decay': 100}
    np.random.seed(8)
    uks, Uf = _grape(c['H0'], c['Hops'], ['a', 'b'], c['U'], c['total_time'], 12, [0, 1, 2, 3], convergence=conv, U0=c['U0'], reg_coeffs={'dwdt': 0.01},
                     maxA=list(c['maxA']), robust=ens, transfer=hold, exact_gradient=True, restarts=3, control_map=cm)
    assert uks.shape == (2, 12) and hold.samples.shape == (2, 5) and Uf.shape == (4, 4)
    assert np.max(np.abs(uks - hold.samples @ hold.matrix.T)) <= 1e-14
    want = cmap.apply(cm, ens['amp_scales'][0][:, None] * uks)
    assert np.max(np.abs(cm.coefficients - want)) <= 1e-13 * max(1.0, np.max(np.abs(want)))


def test_crosstalk_compressed_drive_example():
    """examples/crosstalk_compressed_drive.py in a short budget: the pulse optimised through the map beats, through the map, the pulse that was
    optimised as if there were none, by more than a factor of ten.  A tenth of the first line's pi rotation turns the second qubit by 0.3 rad
    too far, an infidelity of order 1e-2 that no optimisation blind to the map removes, while the always-on ZZ coupling limits either pulse to a
    few 1e-4.  Measured on an MI355X with 400 iterations: 3.97e-2 against 4.4e-4 (profiles/control_map.txt)."""
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import crosstalk_compressed_drive as ex
    with contextlib.redirect_stdout(io.StringIO()):
        inf_naive, inf_aware = ex.main(iterations=200, quiet=True)
    print('infidelity through the true map: naive %.3e aware %.3e' % (inf_naive, inf_aware))
    assert inf_aware * 10 < inf_naive and inf_aware < 1e-2, (inf_naive, inf_aware)
