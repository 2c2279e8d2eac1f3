"""Risk-sensitive robust GRAPE on the GPU (qoc_set_risk, k_ens_tilt, DESIGN.md 6b'): an ensemble engine with a risk against the soft worst case
composed from the unchanged oracle (tests/robust_reference.py) on every path that hosts ensembles, with the exact gradient and behind a response
matrix; bit identity of risk 0 with no risk, of two evaluations, of a one-member ensemble; the large-beta limit; beta changed on a live engine; the
device Adam and L-BFGS loops; the refusals of the two entry points; and the capability through Grape(robust=ensemble_grid(..., risk=...))."""
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
from quantum_optimal_control.helper_functions import robust as rb
from quantum_optimal_control.helper_functions import transfer as tf
from tests import exact_gradient_reference as xr
from tests import lbfgs_reference as ref
from tests.composed_reference import run_adam
from tests.robust_reference import composed, composed_shaped
from tests.test_hip_parity import G_RTOL, S_RTOL
from tests.test_robust_gpu import bases_for, ensemble, make_engine, member_systems, nominal_system, problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = hip_engine
BETA = 200.0            # beta x 1e-15 (a member loss's error) = 2e-13 relative on pi: two decades under G_RTOL
MIN_TILT = 0.02         # every parity row: some |pi_e - w_e| at least this, so a mean-weighted reduce cannot pass
KEYS = ('loss', 'reg_loss', 'grad_squared', 'unitary_scale')


def with_risk(ens, beta):
    return dict(ens, risk=float(beta))


@functools.lru_cache(maxsize=None)
def row(kind, regs, E, q):
    """(case, ensemble without a risk, nominal system, member systems) of a row: built once."""
    c = problem(kind, regs)
    ens = ensemble(c, E, q)
    nominal = nominal_system(c)
    return c, ens, nominal, member_systems(c, ens, (nominal.exp_terms, nominal.scaling))


@functools.lru_cache(maxsize=None)
def reference(kind, regs, E, q, beta=BETA, exact=False):
    """The composed oracle of a row at its three bases: computed once, shared by every path.  Asserts the row's condition here, before any engine."""
    _, ens, nominal, sps = row(kind, regs, E, q)
    out = [composed(sps, ens['weights'], b, beta=beta, evaluate=xr.evaluate if exact else go.evaluate) for b in bases_for(nominal, 3)]
    if beta == BETA:
        for o in out:
            tilt = float(np.max(np.abs(o['pi'] - ens['weights'])))
            gap = o['reg_loss'] - float(np.dot(ens['weights'], [m['reg_loss'] for m in o['members']]))
            print('%s-%s E%d: largest |pi - w| %.3f, J - mean %.3e' % (kind, regs, E, tilt, gap))
            assert tilt >= MIN_TILT, (kind, regs, E, tilt)
    return out


def assert_matches(r, g, o, pi=None):
    """tests/test_robust_gpu.py check_evaluation's comparison of scalars and gradient, and the tilted weights."""
    for key in KEYS:
        assert abs(r[key][g] - o[key]) <= S_RTOL * max(1.0, abs(o[key])), (key, g, r[key][g], o[key])
    gm = max(1.0, float(np.max(np.abs(o['grad']))))
    assert np.max(np.abs(r['grad'][g] - o['grad'])) <= G_RTOL * gm, (g, np.max(np.abs(r['grad'][g] - o['grad'])))
    if pi is not None:
        assert np.max(np.abs(pi[g] - o['pi'])) <= S_RTOL * max(1.0, float(np.max(np.abs(o['pi'])))), (g, pi[g], o['pi'])


# ---- 1. single evaluation against the composed oracle -----------------------------------------------------------------------------------

ENSEMBLES = [(3, 1, 3), (16, 2, 1)]          # (E, q, G)
UNITARY_PATHS = [('auto', P.PATH_AUTO, 0), ('mfma', P.PATH_MFMA, 0), ('gemm', P.PATH_GEMM, 0), ('generic', P.PATH_GENERIC, 0)]
STATE_PATHS = [('auto', P.PATH_AUTO, 0), ('mfma', P.PATH_MFMA, 0), ('gemm', P.PATH_GEMM, 1), ('generic', P.PATH_GENERIC, 0)]
ROWS = []
for kind, regs in (('unitary', 'none'), ('unitary', 'state'), ('state', 'pulse'), ('dressed', 'state')):
    for pname, path, chunks in (STATE_PATHS if kind == 'state' else UNITARY_PATHS):
        for E, q, G in ENSEMBLES:
            ROWS.append(pytest.param(kind, regs, path, chunks, E, q, G, False, id='%s-%s-%s-E%d-q%d-G%d' % (kind, regs, pname, E, q, G)))
ROWS.append(pytest.param('unitary', 'state', P.PATH_AUTO, 0, 3, 1, 3, True, id='unitary-state-exact_gradient-E3-q1-G3'))


@pytest.mark.parametrize('kind,regs,path,chunks,E,q,G,exact', ROWS)
def test_evaluation_matches_the_composed_oracle(kind, regs, path, chunks, E, q, G, exact):
    _, ens, nominal, _ = row(kind, regs, E, q)
    refs = reference(kind, regs, E, q, BETA, exact)
    kw = dict(exact_gradient=True) if exact else {}
    eng = hip_engine.HipEngine(nominal.Hs, nominal.U0, nominal.V, nominal.W, nominal.maxA, nominal.dt, nominal.total_time, nominal.steps,
                               nominal.exp_terms, nominal.scaling, state_transfer=nominal.state_transfer, reg_coeffs=nominal.reg_coeffs,
                               one_minus_gauss=nominal.one_minus_gauss, Vs=nominal.Vs, n_seeds=G, path=path, chunks=chunks,
                               ensemble=with_risk(ens, BETA), **kw)
    try:
        if path != P.PATH_AUTO:
            assert eng.path == path, (eng.path, path)
        if exact:
            assert eng.plan['path'] == 'generic', eng.plan
        assert eng.plan['members'] == str(E) and eng.risk == BETA
        eng.set_base(bases_for(nominal, G))
        r = eng.evaluate()
        pi, ms = eng.member_weights(), eng.member_scalars()
        assert pi.shape == (G, E)
        for g in range(G):
            assert_matches(r, g, refs[g], pi)
            assert np.max(np.abs(ms['loss'][g] - refs[g]['member_loss'])) <= S_RTOL * max(1.0, np.max(np.abs(refs[g]['member_loss'])))
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def shaped_reference(resp):
    """tests/test_transfer_gpu.py's composition (members with the state regularisers only, pulse regularisers on the samples) under a risk."""
    from tests import test_transfer_gpu as tg
    c = tg.shaped_problem('unitary', 'state')
    c['reg_coeffs'] = dict(c['reg_coeffs'], **{key: tg.PULSE_REGS[key] for key in ('amplitude', 'dwdt')})
    ens = ensemble(c, 3, 1)
    nominal, sps, w = tg.systems(c, ens)
    T = tf.hold(nominal.steps, 10).matrix if resp == 'hold10' else tg.response('dense5', nominal.steps, nominal.total_time)
    th = tg.thetas(nominal.k, T.shape[1], 3)
    _, pulse_rc = tg.split_regs(c['reg_coeffs'])
    out = [composed_shaped(sps, w, T, th[g], pulse_rc, nominal.total_time, beta=BETA) for g in range(3)]
    for o in out:
        tilt = float(np.max(np.abs(o['pi'] - w)))
        print('shaped %s: largest |pi - w| %.3f' % (resp, tilt))
        assert tilt >= MIN_TILT, (resp, tilt)
    return nominal, ens, T, th, out


@pytest.mark.parametrize('resp,lanes', [('hold10', 1), ('dense5', 64)])
def test_shaped_evaluation_matches_the_composed_oracle(resp, lanes):
    """A hold response with P = 10 (column windows of 4 slices: one thread per output) and a dense signed one (windows of 40 slices: one wave)."""
    from tests import test_transfer_gpu as tg
    nominal, ens, T, th, refs = shaped_reference(resp)
    col_band = max(int(np.flatnonzero(col)[-1] - np.flatnonzero(col)[0] + 1) for col in T.T)
    assert (col_band > 32) == (lanes == 64), col_band
    eng = tg.make_engine(nominal, 3, T, with_risk(ens, BETA))
    try:
        eng.set_base(th)
        r = eng.evaluate()
        pi = eng.member_weights()
        for g in range(3):
            assert_matches(r, g, refs[g], pi)
    finally:
        eng.close()


# ---- 2. bit identity and determinism ------------------------------------------------------------------------------------------------------

ADAM25 = dict(rate=0.02, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=25, poll_every=7)


def _eval_and_loop(eng, bases):
    eng.set_base(bases)
    r = eng.evaluate()
    eng.set_base(bases)
    its = eng.run_adam(eng.adam_params(**ADAM25))
    return dict(r, its=its, base=eng.get_base(), uks=eng.get_uks(), after=eng.scalars(), weights=eng.member_weights())


def _assert_same(a, b):
    for key in KEYS + ('grad', 'its', 'base', 'uks', 'weights'):
        assert np.array_equal(a[key], b[key]), key
    for key in KEYS + ('iterations', 'done'):
        assert np.array_equal(a['after'][key], b['after'][key]), key


@pytest.mark.parametrize('path', [P.PATH_MFMA, P.PATH_GEMM, P.PATH_GENERIC])
def test_risk_zero_is_bit_identical_to_no_risk(path):
    _, ens, nominal, _ = row('unitary', 'state', 3, 1)
    absent = {key: v for key, v in ens.items() if key != 'risk'}
    out = []
    for e in (absent, with_risk(ens, 0.0)):
        eng = make_engine(nominal, 2, e, path)
        try:
            out.append(_eval_and_loop(eng, bases_for(nominal, 2)))
            assert np.array_equal(out[-1]['weights'], np.tile(ens['weights'], (2, 1)))
        finally:
            eng.close()
    _assert_same(*out)


def test_two_evaluations_under_a_risk_are_bit_identical():
    _, ens, nominal, _ = row('unitary', 'state', 16, 2)
    eng = make_engine(nominal, 3, with_risk(ens, BETA))
    try:
        eng.set_base(bases_for(nominal, 3))
        a, wa = eng.evaluate(), eng.member_weights()
        b, wb = eng.evaluate(), eng.member_weights()
        for key in KEYS + ('grad',):
            assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(wa, wb)
    finally:
        eng.close()


# ---- 3. limits ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('regs', ['none', 'state'])
def test_a_huge_beta_is_the_worst_member(regs):
    """beta = 1e9: exp underflows on every member but the worst (the costs differ by far more than 1e-7), whose weight is 1.  Then S = w_worst - 1
    exactly and J = c_worst + log(w_worst) / beta: the worst member's value and the term tests/test_risk.py bounds the distance to the maximum by, -1e-9
    for a weight of a third.  The loss is held to S_RTOL against that limit value, not against c_worst alone, which the function misses by this 1e-9
    at any finite beta (measured: 0.9776107138721752 against a worst member's 0.9776107146777411)."""
    _, ens, nominal, _ = row('unitary', regs, 3, 1)
    refs = reference('unitary', regs, 3, 1, 0.0)                      # (the members' own evaluations are what is needed)
    eng = make_engine(nominal, 3, with_risk(ens, 1e9))
    try:
        eng.set_base(bases_for(nominal, 3))
        r = eng.evaluate()
        pi = eng.member_weights()
        assert all(np.all(np.isfinite(r[key])) for key in KEYS + ('grad',)) and np.all(np.isfinite(pi))
        for g in range(3):
            members = refs[g]['members']
            cost = refs[g]['member_cost']
            worst = int(np.argmax(cost))
            assert np.sort(cost)[-1] - np.sort(cost)[-2] > 1e-6
            onehot = np.zeros(3)
            onehot[worst] = 1.0
            assert np.max(np.abs(pi[g] - onehot)) <= 1e-12, pi[g]
            o = members[worst]
            shift = float(np.log(ens['weights'][worst])) / 1e9
            assert abs(r['loss'][g] - (o['loss'] + shift)) <= S_RTOL * max(1.0, abs(o['loss'])), (r['loss'][g], o['loss'], shift)
            assert abs(r['reg_loss'][g] - (o['reg_loss'] + shift)) <= S_RTOL * max(1.0, abs(o['reg_loss']))
            gm = max(1.0, float(np.max(np.abs(o['grad']))))
            assert np.max(np.abs(r['grad'][g] - o['grad'])) <= G_RTOL * gm
    finally:
        eng.close()


@pytest.mark.parametrize('beta', [BETA, 1e9])
def test_one_member_ignores_beta_bit_for_bit(beta):
    c = problem('unitary', 'state')
    ens = ensemble(c, 1, 0)
    nominal = nominal_system(c)
    out = []
    for b in (0.0, beta):
        eng = make_engine(nominal, 2, with_risk(ens, b))
        try:
            out.append(_eval_and_loop(eng, bases_for(nominal, 2)))
        finally:
            eng.close()
    _assert_same(*out)
    assert np.array_equal(out[1]['weights'], np.ones((2, 1)))


# ---- 4. beta changed on a live engine -------------------------------------------------------------------------------------------------------

def test_set_risk_between_evaluations():
    _, ens, nominal, _ = row('unitary', 'state', 3, 1)
    refs = reference('unitary', 'state', 3, 1)
    eng = make_engine(nominal, 3, ens)
    try:
        eng.set_base(bases_for(nominal, 3))
        first = eng.evaluate()
        eng.set_risk(BETA)
        assert np.array_equal(eng.member_weights(), np.tile(ens['weights'], (3, 1)))       # nothing evaluated under the risk yet
        second = eng.evaluate()
        pi = eng.member_weights()
        for g in range(3):
            assert_matches(second, g, refs[g], pi)
        eng.set_risk(0.0)
        third = eng.evaluate()
        for key in KEYS + ('grad',):
            assert np.array_equal(first[key], third[key]), key
        assert np.array_equal(eng.member_weights(), np.tile(ens['weights'], (3, 1)))
    finally:
        eng.close()


# ---- 5. loops ---------------------------------------------------------------------------------------------------------------------------------

def python_loop(sps, w, beta, base, conv):
    """tests/test_robust_gpu.py python_loop over the composed risk ensemble: go.Adam, run_adam's stop rule and learning-rate schedule."""
    return run_adam(lambda b: composed(sps, w, b, beta=beta), base, conv)


def choose_target(hists, max_it):
    """A conv_target at which the three control sets stop at three different iterations, two of them before max_it, with no loss of any history
    within 1e-8 relative of it: midpoints between neighbouring losses, the widest margin wins."""
    losses = np.sort(np.unique(np.concatenate([h[:, 0] for h in hists])))
    best = None
    for lo, hi in zip(losses[:-1], losses[1:]):
        t = 0.5 * (lo + hi)
        stops = [int(np.nonzero(h[:, 0] < t)[0][0]) if np.any(h[:, 0] < t) else max_it for h in hists]
        margin = min(float(np.min(np.abs(h[:, 0] - t))) / abs(t) for h in hists)
        if len(set(stops)) == 3 and sum(0 < s < max_it for s in stops) >= 2 and (best is None or margin > best[0]):
            best = (margin, t, stops)
    assert best is not None and best[0] > 1e-8, best
    return best[1], best[2]


@functools.lru_cache(maxsize=None)
def adam_reference():
    """The loop's reference, shared by the two tests below: a free run of 24 iterations per control set, the target, the runs that stop at it."""
    _, ens, nominal, sps = row('unitary', 'state', 3, 1)
    bases = bases_for(nominal, 3)
    conv = dict(rate=0.02, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=24)
    free = [python_loop(sps, ens['weights'], BETA, b, conv) for b in bases]
    target, stops = choose_target([f['history'] for f in free], 24)
    conv['conv_target'] = target
    refs = [python_loop(sps, ens['weights'], BETA, b, conv) for b in bases]
    assert [r['iterations'] for r in refs] == stops
    return conv, refs, stops


def test_adam_loop_matches_the_composed_oracle():
    """Three control sets that stop at three different iterations, two of them inside a burst of 16."""
    _, ens, nominal, _ = row('unitary', 'state', 3, 1)
    conv, refs, stops = adam_reference()
    eng = make_engine(nominal, 3, with_risk(ens, BETA))
    try:
        eng.set_base(bases_for(nominal, 3))
        its = eng.run_adam(eng.adam_params(poll_every=16, **conv))
        s, base, pi = eng.scalars(), eng.get_base(), eng.member_weights()
        for g, rf in enumerate(refs):
            assert its[g] == rf['iterations'], (its, stops)
            assert np.max(np.abs(base[g] - rf['base'])) < 1e-9, np.max(np.abs(base[g] - rf['base']))
            assert abs(s['loss'][g] - rf['last']['loss']) < 1e-10 * max(1.0, abs(rf['last']['loss']))
            assert abs(s['reg_loss'][g] - rf['last']['reg_loss']) < 1e-10 * max(1.0, abs(rf['last']['reg_loss']))
            assert np.max(np.abs(pi[g] - rf['last']['pi'])) < 1e-6            # (beta times the bases' 1e-9 times the members' gradients)
    finally:
        eng.close()


def test_a_finished_control_set_keeps_its_weights():
    """One iteration at a time: once a control set is done its scalars and weights stay, bit for bit, while the others' move."""
    _, ens, nominal, sps = row('unitary', 'state', 3, 1)
    conv, refs, stops = adam_reference()
    first = int(np.argmin(stops))
    eng = make_engine(nominal, 3, with_risk(ens, BETA))
    try:
        eng.set_base(bases_for(nominal, 3))
        params = eng.adam_params(poll_every=1, **conv)
        seen = []
        for _ in range(stops[first] + 4):
            eng.iterate(params, 1)
            s = eng.scalars()
            seen.append((s['done'].copy(), eng.member_weights(), s['loss'].copy()))
        done_at = next(i for i, (d, _, _) in enumerate(seen) if d[first])
        assert done_at == stops[first], (done_at, stops)
        o = composed(sps, ens['weights'], eng.get_base()[first], beta=BETA)        # (a stopped set is not moved: evaluated where it stands)
        assert np.max(np.abs(seen[done_at][1][first] - o['pi'])) <= S_RTOL
        for d, pi, loss in seen[done_at + 1:]:
            assert d[first] and np.array_equal(pi[first], seen[done_at][1][first]) and loss[first] == seen[done_at][2][first]
        running = [g for g in range(3) if not seen[-1][0][g]]
        assert running and all(not np.array_equal(seen[-1][1][g], seen[done_at][1][g]) for g in running)
    finally:
        eng.close()


def test_lbfgs_steps_follow_the_reference_on_the_composed_oracle():
    """tests/test_lbfgs_gpu.py's "oracle as evaluator" row with the composed risk ensemble as the evaluator: branches, points (LOOP_ATOL) and values."""
    from tests import test_lbfgs_gpu as lg
    c = problem('unitary', 'none')
    ens, nominal = ensemble(c, 3, 1), nominal_system(c)
    sps = member_systems(c, ens, (nominal.exp_terms, nominal.scaling))
    eng = make_engine(nominal, 1, with_risk(ens, BETA))
    try:
        lg.compare_with_reference(eng, lambda x: composed(sps, ens['weights'], x, beta=BETA), nominal.base0, dict(lg.BASE), 6, 'risk', with_f=True)
    finally:
        eng.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------

def _last_error(eng):
    return eng._lib.qoc_last_error().decode()


@pytest.mark.parametrize('kind', ['plain', 'exact', 'open'])
def test_other_engines_refuse_the_two_entry_points(kind):
    if kind == 'open':
        from tests import test_open_system_gpu as og
        sp, ops = og.system('n3_c1')
        eng = og.make_engine(sp, ops)
    else:
        nominal = nominal_system(problem('unitary', 'none'))
        kw = dict(exact_gradient=True) if kind == 'exact' else {}
        eng = hip_engine.HipEngine(nominal.Hs, nominal.U0, nominal.V, nominal.W, nominal.maxA, nominal.dt, nominal.total_time, nominal.steps,
                                   nominal.exp_terms, nominal.scaling, reg_coeffs=nominal.reg_coeffs, n_seeds=1, **kw)
    try:
        assert eng._lib.qoc_set_risk(eng._h, 1.0) == -4 and 'qoc_set_risk: not an ensemble engine' in _last_error(eng)      # QOC_ERR_STATE
        out = np.zeros(4)
        assert eng._lib.qoc_get_member_weights(eng._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == -4
        assert 'qoc_get_member_weights: not an ensemble engine' in _last_error(eng)
        with pytest.raises(hip_engine.QocError, match='not an ensemble engine'):
            eng.set_risk(1.0)
    finally:
        eng.close()


@pytest.mark.parametrize('beta,cause', [(-1.0, 'negative'), (float('nan'), 'NaN'), (float('inf'), 'infinite')])
def test_bad_risks_are_refused_with_their_cause(beta, cause):
    _, ens, nominal, _ = row('unitary', 'none', 3, 1)
    eng = make_engine(nominal, 1, ens)
    try:
        assert eng._lib.qoc_set_risk(eng._h, beta) == -1                       # QOC_ERR_INVALID
        assert 'qoc_set_risk' in _last_error(eng) and cause in _last_error(eng), _last_error(eng)
        assert eng._lib.qoc_set_risk(eng._h, BETA) == 0                        # and the engine is as it was
    finally:
        eng.close()


# ---- 7. the capability through Grape, and the example --------------------------------------------------------------------------------------

def _oracle_infidelities(ex, ens, uks):
    """The members' infidelities of a pulse from the oracle, one system per member, with a generous series (14 terms, 3 squarings)."""
    H0, Hops, _, _ = ex.problem()
    out = []
    for e in range(len(ens['weights'])):
        H0e, Hopse = rb.member_hamiltonians(H0, Hops, ens, e)
        np.random.seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            sp = go.OracleSystem(H0e, Hopse, ex.SX, ex.TOTAL_TIME, ex.STEPS, [0, 1], reg_coeffs={}, maxA=ex.MAXA, Taylor_terms=[14, 3])
        out.append(go.evaluate(sp, np.arcsin(np.clip(uks / np.array(ex.MAXA)[:, None], -1.0, 1.0)), want_grad=False)['loss'])
    return np.array(out)


def test_risk_pulse_is_no_worse_than_the_mean_pulse_on_the_worst_member():
    """examples/worst_case_qubit_pi_pulse.py at its own settings, restarts=2: Grape(robust=ensemble_grid(..., risk=...)) against the mean objective
    from the same seeds and iteration budget; both pulses re-scored per member with the oracle.  The ordering is asserted, no figure.
    Measured on an MI355X: worst-member infidelity 7.951e-03 for the mean objective, 7.779e-03 at risk 1000 (mean infidelity 2.772e-03 / 4.744e-03)."""
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import worst_case_qubit_pi_pulse as ex
    with contextlib.redirect_stdout(io.StringIO()) as out:
        res = ex.main(restarts=2, quiet=True)
    text = out.getvalue()
    assert 'soft worst-case (risk %g)' % ex.RISK in text and 'mean objective:' in text
    i_mean, i_risk = _oracle_infidelities(ex, res['ens'], res['uks_mean']), _oracle_infidelities(ex, res['ens'], res['uks_risk'])
    w = res['ens']['weights']
    print('worst-member infidelity: mean objective %.3e, risk %g objective %.3e; mean infidelity %.3e / %.3e' % (
        i_mean.max(), ex.RISK, i_risk.max(), float(np.dot(w, i_mean)), float(np.dot(w, i_risk))))
    assert np.max(np.abs(i_mean - res['infidelity_mean'])) < 1e-9 and np.max(np.abs(i_risk - res['infidelity_risk'])) < 1e-9
    assert i_risk.max() <= i_mean.max(), (i_mean.max(), i_risk.max())
