"""Risk-sensitive robust GRAPE without a GPU: the NumPy statement of the soft worst case (tests/composed_reference.py) against an extended-precision
restatement and against central differences, the composed ensemble's gradient against central differences of its own value, the `risk` key of
helper_functions/robust.py, and the routing of the risk through HipEngine and Grape with the library replaced by a recorder."""
import numpy as np
import pytest

from oracle import grape_oracle as go
from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import robust as rb
from tests.composed_reference import soft_worst_case
from tests.robust_reference import composed
from tests.test_robust_gpu import ensemble, member_systems, problem

BETAS = [1e-9, 1e-3, 1.0, 200.0, 1e6]


def _costs(E, spread, seed=3):
    rng = np.random.default_rng(seed + E)
    w = rng.uniform(0.5, 1.5, size=E)
    w = w / w.sum()
    c = np.full(E, 0.37) if not spread else rng.uniform(1e-3, 0.9, size=E)
    return c, w


def _longdouble(c, w, beta):
    """The value in np.longdouble.  The weights sum to 1 only within an ulp of double, and the definition's expm1 form is log((1 - sum w) + sum w exp(x))
    exactly: the restatement carries that (1 - sum w), without which it would differ by log(sum w) / beta (1e-13 at beta = 1e-3).  Naive --
    log of the sum of exponentials, shifted by the largest cost so that exp cannot overflow -- wherever longdouble's 64-bit mantissa resolves it to 1e-15:
    log(A) near A = 1 carries an absolute error of 2^-64, divided by beta; below beta (c_max - c_min) = 2^-11 that is no longer two decades under
    1e-15 of J, and the definition itself is evaluated in longdouble instead."""
    cl, wl, bl = c.astype(np.longdouble), w.astype(np.longdouble), np.longdouble(beta)
    x = bl * (cl - np.max(cl))
    if beta * float(np.max(c) - np.min(c)) >= 2.0 ** -11:
        return np.max(cl) + np.log((np.longdouble(1.0) - np.sum(wl)) + np.sum(wl * np.exp(x))) / bl
    return np.max(cl) + np.log1p(np.sum(wl * np.expm1(x))) / bl


@pytest.mark.parametrize('spread', [False, True], ids=['equal', 'spread'])
@pytest.mark.parametrize('E', [1, 3, 16])
@pytest.mark.parametrize('beta', BETAS)
def test_soft_worst_case_against_the_naive_form_in_extended_precision(beta, E, spread):
    """1e-15 relative, against _longdouble above."""
    c, w = _costs(E, spread)
    J, pi = soft_worst_case(c, w, beta)
    ref = _longdouble(c, w, beta)
    assert abs(np.longdouble(J) - ref) <= 1e-15 * abs(ref), (J, float(ref))
    assert abs(pi.sum() - 1.0) <= 4e-16 * E


@pytest.mark.parametrize('E', [1, 3, 16])
def test_soft_worst_case_lies_between_mean_and_max_and_reaches_both(E):
    c, w = _costs(E, True)
    mean, cmax = float(np.dot(w, c)), float(np.max(c))
    for beta in BETAS:
        J, _ = soft_worst_case(c, w, beta)
        assert mean - 1e-15 <= J <= cmax + 1e-15, (beta, mean, J, cmax)
    # J - mean <= beta (c_max - c_min)^2 / 8 (Hoeffding's lemma), beta Var / 2 to leading order: 1e-9 reaches the mean to 1e-12 for costs within a range
    # of 0.089, as infidelities of one pulse over an ensemble are; the costs above span 0.9 (2.5e-11 at E = 16), so this line narrows them to 0.072
    cn = 0.01 + 0.08 * c
    assert abs(soft_worst_case(cn, w, 1e-9)[0] - float(np.dot(w, cn))) <= 1e-12
    J, pi = soft_worst_case(c, w, 1e6)
    assert 0.0 <= cmax - J <= np.log(1.0 / w[int(np.argmax(c))]) / 1e6 + 1e-15
    assert soft_worst_case(c, w, 0.0)[0] == float(np.dot(w, c)) and np.array_equal(soft_worst_case(c, w, 0.0)[1], w)


def test_a_member_of_weight_zero_sets_neither_the_shift_nor_the_value():
    c, w = np.array([0.1, 0.9, 0.2]), np.array([0.5, 0.0, 0.5])
    J, pi = soft_worst_case(c, w, 1e6)
    assert np.isfinite(J) and abs(J - 0.2) < 1e-6 and pi[1] == 0.0 and abs(pi[2] - 1.0) < 1e-12


@pytest.mark.parametrize('beta', [1e-3, 1.0, 200.0])
@pytest.mark.parametrize('E', [3, 16])
def test_tilted_weights_are_the_derivative_of_the_value(beta, E):
    c, w = _costs(E, True)
    _, pi = soft_worst_case(c, w, beta)
    h = 1e-6
    for e in range(E):
        d = np.zeros(E)
        d[e] = h
        fd = (soft_worst_case(c + d, w, beta)[0] - soft_worst_case(c - d, w, beta)[0]) / (2 * h)
        assert abs(fd - pi[e]) <= 1e-7, (e, fd, pi[e])


def test_composed_gradient_is_the_derivative_of_the_composed_value():
    """problem('state', 'pulse'), E = 3, beta = 200, six elements of `base`, central differences of step h = 1e-6 of the composed ensemble's own reg_loss.

    The admissible error is derived, not fitted.  (1) grad = sum_e pi_e grad_e with sum pi = 1 is a convex combination, and sum_e pi_e dc_e is the exact
    derivative of J; so grad misses it by at most max_e err_e, where err_e = |grad_e - central difference of member e's own reg_loss| is the existing
    first-order error of this case, measured here with the same stencil on the unchanged go.evaluate (it contains the members' own truncation and
    rounding).  (2) The stencil's truncation on J beyond the members' own: h^2 / 6 times the parts of J''' that carry beta -- the third cumulant of the
    directional derivatives under pi, beta^2 (2 g)^3 at most, and the cross term 3 beta (2 g)(2 g2) -- with g and g2 the largest first and second
    differences of the members' reg_loss at that element.  (3) Rounding of J (a few ulp of a value below 1) over 2 h: 1e-9."""
    c = problem('state', 'pulse')
    ens = ensemble(c, 3, 1)
    sps = member_systems(c, ens, c['Taylor_terms'])
    w, beta, h = ens['weights'], 200.0, 1e-6
    base = sps[0].base0.copy()
    r0 = composed(sps, w, base, beta=beta)
    assert np.max(np.abs(r0['pi'] - w)) >= 0.02
    rng = np.random.default_rng(0)
    for _ in range(6):
        j, t = int(rng.integers(base.shape[0])), int(rng.integers(base.shape[1]))
        d = np.zeros_like(base)
        d[j, t] = h
        up, dn = composed(sps, w, base + d, beta=beta), composed(sps, w, base - d, beta=beta)
        fd = (up['reg_loss'] - dn['reg_loss']) / (2 * h)
        cu = np.array([m['reg_loss'] for m in up['members']])
        cd = np.array([m['reg_loss'] for m in dn['members']])
        c0 = np.array([m['reg_loss'] for m in r0['members']])
        g1 = (cu - cd) / (2 * h)
        err_members = float(np.max(np.abs(g1 - np.array([m['grad'][j, t] for m in r0['members']]))))
        g, g2 = float(np.max(np.abs(g1))), float(np.max(np.abs(cu - 2 * c0 + cd))) / h ** 2
        bound = err_members + h * h / 6 * (beta ** 2 * (2 * g) ** 3 + 3 * beta * (2 * g) * (2 * g2)) + 1e-9
        print('element (%d, %d): |grad - fd| %.3e, bound %.3e (members %.3e)' % (j, t, abs(r0['grad'][j, t] - fd), bound, err_members))
        assert abs(r0['grad'][j, t] - fd) <= bound, (j, t, r0['grad'][j, t], fd, bound)


# ---- the `risk` key ---------------------------------------------------------------------------------------------------------------------

def _dict(**kw):
    return dict(dict(operators=[np.diag([1.0, -1.0])], offsets=[[0.0], [0.1]], amp_scales=np.ones((2, 1)), weights=[1.0, 3.0]), **kw)


def test_validate_accepts_defaults_and_refuses_risk_values():
    assert rb.validate(_dict(), 2, 1)['risk'] == 0.0
    out = rb.validate(_dict(risk=200), 2, 1)
    assert out['risk'] == 200.0 and isinstance(out['risk'], float) and abs(out['weights'].sum() - 1.0) < 1e-15
    assert rb.validate(_dict(risk=0), 2, 1)['risk'] == 0.0
    for bad in (-1.0, float('nan'), float('inf'), 'high', None):
        with pytest.raises(ValueError, match='risk'):
            rb.validate(_dict(risk=bad), 2, 1)
    with pytest.raises(ValueError, match='unknown keys'):
        rb.validate(_dict(extra=1), 2, 1)
    with pytest.raises(ValueError, match='unknown keys'):
        rb.validate(_dict(beta=1.0), 2, 1)


def test_ensemble_grid_passes_the_risk_on():
    kw = dict(operators=[np.diag([1.0, -1.0])], offsets=[[-0.1], [0.0], [0.1]], amp_scales=[0.9, 1.0], k=2)
    assert rb.ensemble_grid(**kw)['risk'] == 0.0
    ens = rb.ensemble_grid(risk=50.0, **kw)
    assert ens['risk'] == 50.0 and ens['weights'].shape == (6,)
    assert rb.validate(ens, 2, 2)['risk'] == 50.0                # what Grape does with it
    with pytest.raises(ValueError, match='risk'):
        rb.ensemble_grid(risk=-0.5, **kw)


# ---- routing, with the library replaced by a recorder --------------------------------------------------------------------------------------

class Recorder(object):
    """Stands where the loaded library stands: every entry point succeeds and is written down."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call

    def named(self, name):
        return [a for n, a in self.calls if n == name]


def _engine(monkeypatch, ens):
    lib = Recorder()
    monkeypatch.setattr(hip_engine, 'load_library', lambda: lib)
    Hs = np.zeros((2, 2, 2), dtype=np.complex128)
    eng = hip_engine.HipEngine(Hs, np.eye(2), np.eye(2), np.eye(2), [1.0], 0.1, 0.4, 4, 3, 0, reg_coeffs={}, n_seeds=2, ensemble=ens)
    return lib, eng


def test_engine_sets_the_risk_only_when_there_is_one(monkeypatch):
    for risk, expect in ((None, []), (0.0, []), (200.0, [200.0])):
        ens = rb.validate(_dict() if risk is None else _dict(risk=risk), 2, 1)
        if risk is None:
            del ens['risk']                                      # a dict from before the key existed
        lib, eng = _engine(monkeypatch, ens)
        assert [a[1] for a in lib.named('qoc_set_risk')] == expect and len(lib.named('qoc_create_ensemble')) == 1
        assert eng.risk == (risk or 0.0)


def test_engine_methods_reach_the_two_entry_points(monkeypatch):
    lib, eng = _engine(monkeypatch, rb.validate(_dict(), 2, 1))
    eng.set_risk(30)
    assert [a[1] for a in lib.named('qoc_set_risk')] == [30.0] and eng.risk == 30.0
    out = eng.member_weights()
    assert out.shape == (2, 2) and len(lib.named('qoc_get_member_weights')) == 1


def test_grape_hands_the_risk_to_the_engine(monkeypatch):
    from quantum_optimal_control.main_grape.grape import Grape
    seen = {}

    class Stop(Exception):
        pass

    def fake_engine(*args, **kw):
        seen.update(kw)
        raise Stop()

    monkeypatch.setattr(hip_engine, 'HipEngine', fake_engine)
    sx = np.array([[0, 1], [1, 0]], dtype=complex)
    ens = rb.ensemble_grid(operators=[np.diag([1.0, -1.0])], offsets=[[-0.01], [0.0], [0.01]], k=1, risk=75.0)
    with pytest.raises(Stop):
        Grape(0.0 * sx, [sx], ['x'], sx, 1.0, 4, [0, 1], maxA=[1.0], reg_coeffs={}, save=False, show_plots=False, robust=ens, Taylor_terms=[6, 1])
    assert seen['ensemble']['risk'] == 75.0 and len(seen['ensemble']['weights']) == 3
    with pytest.raises(ValueError, match='risk'):
        Grape(0.0 * sx, [sx], ['x'], sx, 1.0, 4, [0, 1], maxA=[1.0], reg_coeffs={}, save=False, show_plots=False, robust=dict(ens, risk=-1.0))


class FakeLog(object):
    """Stands where data_management.H5File stands (h5py is optional): the datasets a Grape call adds to its run log, by name."""
    added = {}

    def __init__(self, path, mode='a'):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def add(self, key, data=None):
        FakeLog.added[key] = data

    def create_group(self, name):
        return self

    def create_dataset(self, key, data=None):
        pass


@pytest.mark.parametrize('risk', [0.0, 75.0])
def test_run_log_holds_the_risk_when_there_is_one(risk, monkeypatch, tmp_path):
    from quantum_optimal_control.helper_functions import data_management
    from quantum_optimal_control.main_grape.grape import Grape

    class Stop(Exception):
        pass

    def fake_engine(*args, **kw):
        raise Stop()

    monkeypatch.setattr(hip_engine, 'HipEngine', fake_engine)
    monkeypatch.setattr(data_management, 'H5File', FakeLog)
    FakeLog.added = {}
    sx = np.array([[0, 1], [1, 0]], dtype=complex)
    ens = rb.ensemble_grid(operators=[np.diag([1.0, -1.0])], offsets=[[-0.01], [0.0], [0.01]], k=1, risk=risk)
    with pytest.raises(Stop):
        Grape(0.0 * sx, [sx], ['x'], sx, 1.0, 4, [0, 1], maxA=[1.0], reg_coeffs={}, save=True, file_name='risk', data_path=str(tmp_path),
              convergence={'max_iterations': 1}, show_plots=False, robust=ens, Taylor_terms=[6, 1])
    assert np.array_equal(FakeLog.added['robust_weights'], ens['weights'])
    if risk > 0:
        assert np.array_equal(np.asarray(FakeLog.added['robust_risk']), [risk])
    else:
        assert 'robust_risk' not in FakeLog.added
