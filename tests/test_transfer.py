"""Transfer-function GRAPE, CPU side: the response builders of helper_functions/transfer.py, validate / apply, and the refusals of
Grape(transfer=...) and of the engine that come before any device is touched."""
import warnings

import numpy as np
import pytest

from quantum_optimal_control.helper_functions import transfer as tf

SZ = np.array([[1, 0], [0, -1]], dtype=complex)
SX = np.array([[0, 1], [1, 0]], dtype=complex)
SY = np.array([[0, -1j], [1j, 0]], dtype=complex)

BUILDERS = [('hold', lambda s, p: tf.hold(s, p)), ('linear_interp', lambda s, p: tf.linear_interp(s, p)),
            ('gaussian', lambda s, p: tf.gaussian_filter(s, p, 0.1 * s, 0.17)), ('gaussian_wide', lambda s, p: tf.gaussian_filter(s, p, 1.0 * s, 3.0))]
SIZES = [(40, 7), (30, 13), (100, 10), (12, 12), (9, 1), (101, 17)]


def _windows_contiguous(M):
    """True when the nonzero entries of every row and of every column form one run."""
    for A in (M, M.T):
        for row in A:
            nz = np.flatnonzero(row)
            if nz.size and not np.all(row[nz[0]:nz[-1] + 1] != 0.0):
                return False
    return True


@pytest.mark.parametrize('name,build', BUILDERS)
@pytest.mark.parametrize('steps,P', SIZES)
def test_builders_give_row_stochastic_banded_matrices(name, build, steps, P):
    tr = build(steps, P)
    M = tr.matrix
    assert isinstance(tr, tf.Transfer) and tr.samples is None and tr.n_samples == P
    assert M.shape == (steps, P) and M.dtype == np.float64 and M.flags['C_CONTIGUOUS']
    np.testing.assert_allclose(M.sum(axis=1), 1.0, rtol=0, atol=2.3e-16 * steps)     # one rounding per term of the row sums
    assert np.all(M >= 0.0) and np.all(np.any(M != 0.0, axis=0))               # an average of the samples; every sample is used
    assert _windows_contiguous(M)
    assert tf.validate(tr, steps) is tr


@pytest.mark.parametrize('steps,P', SIZES)
def test_hold_has_one_unit_entry_per_row_in_the_window_of_its_sample(steps, P):
    M = tf.hold(steps, P).matrix
    assert np.all((M == 0.0) | (M == 1.0)) and np.all(M.sum(axis=1) == 1.0)
    t = np.arange(steps)
    assert np.array_equal(np.argmax(M, axis=1), t * P // steps)
    counts = M.sum(axis=0)
    assert counts.min() >= steps // P and counts.max() <= -(-steps // P)      # steps % P != 0: windows of two lengths
    if steps % P:
        assert counts.min() < counts.max()


def test_linear_interp_reproduces_a_linear_ramp_between_the_outer_sample_centres():
    steps, P = 60, 6
    M = tf.linear_interp(steps, P).matrix
    ramp = np.arange(P, dtype=float)
    x = (np.arange(steps) + 0.5) * P / steps - 0.5
    np.testing.assert_allclose(M @ ramp, np.clip(x, 0, P - 1), atol=1e-14)
    assert np.max(np.count_nonzero(M, axis=1)) == 2


def test_gaussian_filter_is_the_smoothed_hold():
    steps, P, total_time, sigma = 50, 10, 10.0, 0.5
    M = tf.gaussian_filter(steps, P, total_time, sigma).matrix
    H = tf.hold(steps, P).matrix
    s = sigma / (total_time / steps)
    t = 23
    lo, hi = t - int(4 * s), t + int(4 * s) + 1
    g = np.exp(-0.5 * ((np.arange(lo, hi) - t) / s) ** 2)
    np.testing.assert_allclose(M[t], (g / g.sum()) @ H[lo:hi], atol=1e-15)
    assert np.count_nonzero(M[t]) > 1                                          # overlapping windows
    # a vanishing sigma leaves the hold
    np.testing.assert_array_equal(tf.gaussian_filter(steps, P, total_time, 1e-3).matrix, H)
    with pytest.raises(ValueError, match='sigma'):
        tf.gaussian_filter(steps, P, total_time, 0.0)


def test_builders_reject_impossible_sizes():
    for bad in ((10, 0), (10, 11)):
        with pytest.raises(ValueError, match='samples for'):
            tf.hold(*bad)
        with pytest.raises(ValueError, match='samples for'):
            tf.linear_interp(*bad)


@pytest.mark.parametrize('matrix,match', [
    (np.ones((5, 2)), 'expected \\(6, P\\)'),
    (np.ones(6), 'expected \\(steps, P\\)'),
    (np.ones((6, 0)), 'P >= 1'),
    (np.where(np.eye(6, 3) > 0, np.nan, 0.5), 'non-finite'),
    (np.where(np.eye(6, 3) > 0, np.inf, 0.5), 'non-finite'),
    (np.eye(6, 3)[:, [0, 1, 1]] * np.array([1.0, 1.0, 0.0]), 'column 2 .* is zero'),
])
def test_validate_errors(matrix, match):
    with pytest.raises(ValueError, match=match):
        tf.validate(matrix, 6)


def test_validate_warns_once_when_a_row_exceeds_unit_l1_norm():
    tf._warned_l1 = False
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        tr = tf.validate(np.full((4, 2), 0.6), 4)
        tf.validate(np.full((4, 2), -0.7), 4)
    assert isinstance(tr, tf.Transfer)
    assert len(w) == 1 and 'l1 norm' in str(w[0].message) and 'maxA' in str(w[0].message)
    tf._warned_l1 = False
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        tf.validate(np.full((4, 2), -0.5), 4)                                   # l1 = 1: the bound holds
    assert len(w) == 0


def test_apply_is_the_matrix_product_on_the_sample_axis():
    rng = np.random.default_rng(0)
    M = rng.normal(size=(9, 4))
    c = rng.normal(size=(3, 4))
    u = tf.apply(M, c)
    assert u.shape == (3, 9)
    np.testing.assert_allclose(u, np.einsum('tp,jp->jt', M, c), atol=1e-15)
    np.testing.assert_array_equal(tf.apply(tf.Transfer(M), c), u)
    np.testing.assert_array_equal(tf.apply(tf.hold(9, 3), np.array([[1.0, 2.0, 3.0]])), [[1, 1, 1, 2, 2, 2, 3, 3, 3]])
    with pytest.raises(ValueError, match='samples have shape'):
        tf.apply(M, rng.normal(size=(3, 5)))


def test_grape_rejects_bad_transfer_arguments_before_any_device_work():
    from quantum_optimal_control.main_grape.grape import Grape, GrapeSharded
    args = (0 * SZ, [SX / 2, SY / 2], ['x', 'y'], SX, 10.0, 20, [0, 1])
    kw = dict(save=False, show_plots=False)
    with pytest.raises(ValueError, match='expected \\(20, P\\)'):
        Grape(*args, transfer=tf.hold(10, 5), **kw)
    with pytest.raises(ValueError, match='is zero'):
        Grape(*args, transfer=np.eye(20)[:, :5] * np.array([1, 1, 0, 1, 1.0]), **kw)
    with pytest.raises(ValueError, match='time-sharded'):
        Grape(*args, transfer=tf.hold(20, 5), time_comm=object(), **kw)
    with pytest.raises(ValueError, match='envelope'):
        Grape(*args, transfer=tf.hold(20, 5), reg_coeffs={'envelope': 0.1}, **kw)
    with pytest.raises(ValueError, match='\\(2, 5\\) sample amplitudes'):
        Grape(*args, transfer=tf.hold(20, 5), initial_guess=np.zeros((2, 20)), maxA=[0.1, 0.1], reg_coeffs={}, **kw)
    with pytest.raises(ValueError, match='Initial guess has strength > max_amp for op 1'):
        Grape(*args, transfer=tf.hold(20, 5), initial_guess=np.array([[0.05] * 5, [0.2] * 5]), maxA=[0.1, 0.1], reg_coeffs={}, **kw)
    with pytest.raises(ValueError, match='GrapeSharded: transfer'):
        GrapeSharded(*args, restarts=2, transfer=tf.hold(20, 5), **kw)
    import inspect
    params = inspect.signature(Grape).parameters
    names = list(params)
    assert params['transfer'].kind is inspect.Parameter.KEYWORD_ONLY and params['transfer'].default is None
    assert names.index('transfer') == names.index('robust') + 1


def test_shaped_engine_refuses_bad_arguments_before_touching_a_device():
    from quantum_optimal_control.core import hip_engine
    n, k, m, steps = 2, 1, 2, 4
    Hs = np.zeros((k + 1, n, n), dtype=np.complex128)
    base = (Hs, np.eye(n), np.eye(n)[:, :m], np.eye(n)[:, :m], [1.0], 0.1, 0.4, steps, 3, 0)
    T = tf.hold(steps, 2).matrix
    bad_col = T.copy()
    bad_col[:, 1] = 0.0
    nan = T.copy()
    nan[1, 0] = np.nan
    for kw, match in ((dict(transfer=np.zeros((steps, 0))), 'n_samples = 0'), (dict(transfer=nan), 'not finite'),
                      (dict(transfer=bad_col), 'column 1 of T is zero'),
                      (dict(reg_coeffs={'envelope': 0.1}, one_minus_gauss=np.ones((k, steps))), 'envelope'),
                      (dict(path=hip_engine.PATH_SMALL), 'workgroup-resident'), (dict(variant=5), 'latency mode'),
                      (dict(time_shards=2, time_rank=-1), 'time-sharded')):
        kw = dict(dict(transfer=T, reg_coeffs={}), **kw)
        with pytest.raises(hip_engine.QocError, match=match):
            hip_engine.HipEngine(*base, **kw)
    with pytest.raises(ValueError, match='transfer matrix has shape'):
        hip_engine.HipEngine(*base, transfer=np.ones((steps + 1, 2)), reg_coeffs={})
