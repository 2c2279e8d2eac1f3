"""Noise traces on the CPU: the rules of robust.validate and fleet.validate for the key `traces`, the builders of
helper_functions/noise.py, the Taylor rule, the reference of tests/noise_reference.py pinned to the constant-offset composition it generalises and
to central differences, and the statistics of the generators."""
import numpy as np
import pytest

from quantum_optimal_control.helper_functions import fleet as fl_mod
from quantum_optimal_control.helper_functions import noise
from quantum_optimal_control.helper_functions import robust as rb
from tests import control_map_reference as ref
from tests import fleet_reference as fr
from tests import noise_reference as nr
from tests import test_robust_gpu as rg

SZ = np.diag([1.0, -1.0]).astype(np.complex128)
SX = np.array([[0, 1], [1, 0]], dtype=np.complex128)


def _dict(E=3, q=2, steps=5, k=2, **kw):
    rng = np.random.default_rng(1)
    d = dict(operators=[SZ, SX][:q], offsets=rng.normal(size=(E, q)), amp_scales=np.ones((E, k)), traces=rng.normal(size=(E, q, steps)))
    d.update(kw)
    return d


# ---- validate ---------------------------------------------------------------------------------------------------------------------------

def test_validate_accepts_traces_and_returns_them_only_when_given():
    out = rb.validate(_dict(), 2, 2, steps=5)
    assert out['traces'].shape == (3, 2, 5) and out['traces'].dtype == np.float64
    assert set(out) == {'operators', 'offsets', 'amp_scales', 'weights', 'risk', 'traces'}
    d = _dict()
    del d['traces']
    assert set(rb.validate(d, 2, 2)) == {'operators', 'offsets', 'amp_scales', 'weights', 'risk'}
    assert rb.validate(_dict(), 2, 2)['traces'].shape == (3, 2, 5)              # (steps unknown to the caller: the last axis is free)


def test_validate_allows_traces_with_sparse_and_with_decay():
    import scipy.sparse as sps
    out = rb.validate(_dict(operators=[sps.csr_matrix(SZ), SX]), 2, 2, sparse=True, steps=5)
    assert 'traces' in out and sps.issparse(out['operators'][0])
    out = rb.validate(_dict(collapse_ops=[0.1 * np.array([[0, 1], [0, 0]], dtype=complex)]), 2, 2, steps=5)
    assert 'traces' in out and out['rate_scales'].shape == (3, 1)


@pytest.mark.parametrize('change,match', [
    (dict(traces=np.zeros((3, 2))), r'traces have shape \(3, 2\), expected \(3, 2, steps\)'),
    (dict(traces=np.zeros((2, 2, 5))), r'traces have shape \(2, 2, 5\), expected \(3, 2, steps\)'),
    (dict(traces=np.zeros((3, 5, 2))), r'traces have shape \(3, 5, 2\), expected \(3, 2, steps\)'),
    (dict(traces=np.zeros((3, 2, 4))), 'traces have 4 slices, the pulse has 5'),
    (dict(traces=np.full((3, 2, 5), np.nan)), 'traces must be finite'),
    (dict(traces=np.full((3, 2, 5), np.inf)), 'traces must be finite'),
    (dict(operators=[], offsets=np.zeros((3, 0)), traces=np.zeros((3, 0, 5))), 'traces given without operators'),
])
def test_validate_refuses(change, match):
    with pytest.raises(ValueError, match=match):
        rb.validate(_dict(**change), 2, 2, steps=5)


def test_fleet_carries_traces_and_hands_each_device_its_slice():
    rng = np.random.default_rng(2)
    tr = rng.normal(size=(2, 3, 2, 5))
    fl = fl_mod.validate(fl_mod.Fleet([SZ, SX], rng.normal(size=(2, 3, 2)), np.ones((2, 3, 2)), traces=tr), 2, 2, steps=5)
    assert np.array_equal(fl.traces, tr)
    for f in range(2):
        dev = fl.device(f)
        assert np.array_equal(dev['traces'], tr[f]) and np.array_equal(dev['offsets'], fl.offsets[f])
        assert rb.validate(dev, 2, 2, steps=5)['traces'].shape == (3, 2, 5)
    assert 'traces' not in fl_mod.Fleet([SZ], np.zeros((2, 1, 1)), np.ones((2, 1, 2))).device(0)
    with pytest.raises(ValueError, match=r'fleet: traces have shape \(2, 3, 2\), expected \(2, 3, 2, steps\)'):
        fl_mod.validate(fl_mod.Fleet([SZ, SX], np.zeros((2, 3, 2)), np.ones((2, 3, 2)), traces=np.zeros((2, 3, 2))), 2, 2)
    with pytest.raises(ValueError, match='fleet: traces have 5 slices, the pulse has 6'):
        fl_mod.validate(fl_mod.Fleet([SZ, SX], np.zeros((2, 3, 2)), np.ones((2, 3, 2)), traces=tr), 2, 2, steps=6)
    with pytest.raises(ValueError, match='fleet: traces must be finite'):
        fl_mod.validate(fl_mod.Fleet([SZ, SX], np.zeros((2, 3, 2)), np.ones((2, 3, 2)), traces=np.full((2, 3, 2, 5), np.nan)), 2, 2)
    one = fl_mod.devices([SZ], offsets=[[0.1], [0.2]], k=2, traces=tr[:, 0, :1])
    assert one.traces.shape == (2, 1, 1, 5) and np.array_equal(one.device(1)['traces'][0], tr[1, 0, :1])
    ens = noise.ensemble([SZ], [tr[0, :, 0]], k=2)
    ar = fl_mod.around([SZ], offsets=[[0.1], [0.2]], robust=ens, k=2)
    assert ar.traces.shape == (2, 3, 1, 5) and np.array_equal(ar.traces[1, :, 0], tr[0, :, 0])


# ---- the builders -----------------------------------------------------------------------------------------------------------------------

def test_ensemble_stacks_one_array_per_operator():
    a, b = noise.white(4, 6, 0.1, 1), noise.quasi_static(4, 6, 0.2, 2)
    ens = noise.ensemble([SZ, SX], [a, b], k=3, risk=2.0)
    assert ens['traces'].shape == (4, 2, 6) and np.array_equal(ens['traces'][:, 0], a) and np.array_equal(ens['traces'][:, 1], b)
    assert ens['offsets'].shape == (4, 2) and not ens['offsets'].any() and ens['amp_scales'].shape == (4, 3) and ens['risk'] == 2.0
    assert np.allclose(ens['weights'], 0.25)
    assert np.all(b == b[:, :1]) and len(set(b[:, 0])) == 4
    with pytest.raises(ValueError, match='one .E, steps. array of traces per operator'):
        noise.ensemble([SZ, SX], [a], k=3)
    with pytest.raises(ValueError, match='every array of traces is'):
        noise.ensemble([SZ, SX], [a, b[:, :5]], k=3)
    dec = noise.ensemble([SZ], [a], k=1, collapse_ops=[0.1 * SX], rate_scales=np.ones((4, 1)))
    assert dec['rate_scales'].shape == (4, 1) and 'traces' in dec


@pytest.mark.parametrize('make', [
    lambda rng: noise.quasi_static(5, 9, 0.3, rng), lambda rng: noise.white(5, 9, 0.3, rng),
    lambda rng: noise.ornstein_uhlenbeck(5, 9, 0.5, 0.3, 2.0, rng), lambda rng: noise.colored(5, 9, 0.5, lambda f: 1.0 / (1.0 + f * f), rng),
    lambda rng: noise.one_over_f(5, 9, 0.5, 0.1, 1.0, 0.01, rng)])
def test_generators_are_determined_by_their_seed(make):
    a, b, c = make(7), make(7), make(8)
    assert a.shape == (5, 9) and a.dtype == np.float64 and np.all(np.isfinite(a))
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(make(np.random.default_rng(7)), a)                   # (a Generator and the int that seeds it: the same stream)


# ---- the Taylor rule --------------------------------------------------------------------------------------------------------------------

def test_taylor_rule_uses_the_largest_perturbation_over_the_slices():
    """offsets + traces[t] of largest MAGNITUDE per member and operator (sign kept): against a hand-built constant-offset ensemble, on a member whose
    lone slice is large enough to change the squaring count."""
    off = np.array([[0.1, -0.2], [0.0, 0.3]])
    tr = np.zeros((2, 2, 6))
    tr[0, 0] = [0.0, 0.2, -0.5, 0.1, 0.0, 0.0]                    # 0.1 + (..) -> -0.4 is the largest magnitude
    tr[0, 1, 4] = 0.1                                             # -0.2 + 0.1 = -0.1: the untouched slices (-0.2) win
    tr[1, 1, 3] = 40.0                                            # 40.3: a lone slice that asks for more squarings
    ens = rb.validate(dict(operators=[SZ, SX], offsets=off, traces=tr), 2, 1, steps=6)
    view = rb.taylor_view(ens)
    assert 'traces' not in view and np.allclose(view['offsets'], [[-0.4, -0.2], [0.0, 40.3]], rtol=0, atol=1e-15)
    args = (0.5 * SZ, [SX], )
    tail = (np.array([1.0]), np.eye(2), 3.0, 6, 1e-4, False, False)
    hand = rb.validate(dict(operators=[SZ, SX], offsets=[[-0.4, -0.2], [0.0, 40.3]]), 2, 1)
    plain = rb.validate(dict(operators=[SZ, SX], offsets=off), 2, 1)
    with_tr, by_hand, without = (rb.choose_taylor(*args, e, *tail) for e in (ens, hand, plain))
    assert with_tr == by_hand and with_tr != without and with_tr[1] > without[1], (with_tr, by_hand, without)
    assert rb.taylor_view(plain) is plain
    fl = fl_mod.validate(fl_mod.Fleet([SZ, SX], np.stack([off, off]), np.ones((2, 2, 1)), traces=np.stack([0 * tr, tr])), 2, 1, steps=6)
    # (device 0 has a zero table -- the plain ensemble --, device 1 the traces: the fleet takes the larger of each figure)
    assert fl_mod.choose_taylor(fl, *args, None, *tail) == (max(by_hand[0], without[0]), max(by_hand[1], without[1]))


# ---- the reference ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['unitary', 'state'])
def test_reference_with_constant_traces_is_the_constant_offset_composition(kind):
    """traces[e, q, :] = c[e, q] on offsets 0, and half of c in each: the composition of tests/test_robust_gpu.py at offsets c, to rounding (the
    perturbation enters as a coefficient row in one and folded into the drift in the other)."""
    c = fr.problem(kind)
    E, q = 3, 2
    ens = rg.ensemble(c, E, q)
    base = np.random.default_rng(3).normal(0.0, 0.7, size=(2, c['steps']))
    o = rg.composed(rg.member_systems(c, ens, c['Taylor_terms']), ens['weights'], base)
    const = np.repeat(ens['offsets'][:, :, None], c['steps'], axis=2)
    for off, tr in ((np.zeros((E, q)), const), (0.5 * ens['offsets'], 0.5 * const)):
        r = nr.evaluate(c, nr.with_traces(dict(ens, offsets=off), tr), base)
        for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale'):
            assert abs(r[key] - o[key]) <= rg.S_RTOL * max(1.0, abs(o[key])), (key, r[key], o[key])
        assert np.max(np.abs(r['grad'] - o['grad'])) <= rg.G_RTOL * max(1.0, float(np.max(np.abs(o['grad']))))
        assert np.max(np.abs(r['member_loss'] - o['member_loss'])) <= rg.S_RTOL
        if kind == 'unitary':
            assert np.max(np.abs(r['U_final'] - o['U0'])) <= rg.U_ATOL
    # ... and a table that varies along the pulse computes something else
    r = nr.evaluate(c, nr.with_traces(ens, nr.make_traces(E, q, c['steps'])), base)
    assert np.max(np.abs(r['member_loss'] - o['member_loss'])) > 1e-4


def test_reference_gradient_against_central_differences():
    """One row (three members with traces, a risk, pulse and state regularisers; dJ/dc from tests/exact_gradient_reference.py) against central
    differences of the reference's reg_loss: h = 1e-6 and the bound 1e-7 of the gradient's largest entry, as tests/test_control_map.py and
    tests/test_exact_gradient.py use for their own such checks."""
    c = fr.problem('state')
    ens = nr.with_traces(dict(rg.ensemble(c, 3, 2), risk=5.0), nr.make_traces(3, 2, c['steps']))
    x = ref.variables(2, c['steps'], 1)[0]
    o = nr.evaluate(c, ens, x, exact=True)
    fd = ref.central_differences(lambda y: nr.evaluate(c, ens, y, exact=True, want_grad=False)['reg_loss'], x, h=1e-6)
    gmax, err = float(np.max(np.abs(o['grad']))), float(np.max(np.abs(o['grad'] - fd)))
    print('noise reference, exact gradient against central differences: max error %.3e of max %.3e' % (err, gmax))
    assert err <= 1e-7 * max(gmax, 1e-3), (err, gmax)


# ---- generator statistics ---------------------------------------------------------------------------------------------------------------

E_STAT = 4096


def test_ornstein_uhlenbeck_variance_and_correlations():
    """E = 4096 independent traces, fixed seed, every figure within 5 standard errors (textbook formulas, from E):
      variance at a slice: a sample variance of E Gaussian values has the standard error sigma^2 sqrt(2 / (E - 1));
      correlation at lag l: the sample correlation of E independent Gaussian pairs with correlation rho has the standard error
      (1 - rho^2) / sqrt(E - 1) (the large-sample formula), rho = a^l."""
    dt, sigma, tau, steps = 0.5, 0.3, 4.0, 40
    x = noise.ornstein_uhlenbeck(E_STAT, steps, dt, sigma, tau, 12345)
    a = np.exp(-dt / tau)
    se_var = sigma ** 2 * np.sqrt(2.0 / (E_STAT - 1))
    for t in (0, 1, steps // 2, steps - 1):                      # (stationary from the first slice on)
        v = np.var(x[:, t], ddof=1)
        print('OU variance at slice %d: %.6f (sigma^2 %.6f, se %.6f)' % (t, v, sigma ** 2, se_var))
        assert abs(v - sigma ** 2) <= 5 * se_var, (t, v)
    for lag in (1, 8):
        rho = a ** lag
        se = (1 - rho ** 2) / np.sqrt(E_STAT - 1)
        for t in (0, steps - 1 - lag):
            r = np.corrcoef(x[:, t], x[:, t + lag])[0, 1]
            print('OU correlation lag %d from slice %d: %.5f (a^lag %.5f, se %.5f)' % (lag, t, r, rho, se))
            assert abs(r - rho) <= 5 * se, (lag, t, r, rho)
    assert abs(np.mean(x[:, 0])) <= 5 * sigma / np.sqrt(E_STAT)


def _expected_periodogram(psd, steps, dt):
    """The mean of the one-sided periodogram (2 dt / steps) |sum_s x[s] e^{-2 pi i j s / steps}|^2 of a `steps`-long window of noise.colored's
    record, from the PSD alone: the record is stationary with the autocovariance R(l) = sum_k psd(f_k) df cos(2 pi k l / N) (df = 1 / (N dt); the
    Nyquist bin, a real coefficient, counts half), and E|X_j|^2 = sum_l (steps - |l|) R(l) cos(2 pi j l / steps).  For a flat PSD this is the PSD
    itself; for any other it is the PSD seen through the window's leakage, which is what a finite trace shows."""
    N = 1 << int(np.ceil(np.log2(noise.RECORD_FACTOR * steps)))
    kk = np.arange(1, N // 2 + 1)
    S = psd(kk / (N * dt)) / (N * dt)
    S[-1] *= 0.5
    lags = np.arange(-(steps - 1), steps)
    R = np.array([np.sum(S * np.cos(2 * np.pi * kk * l / N)) for l in lags])
    j = np.arange(1, steps // 2)
    return j, np.array([(2 * dt / steps) * np.sum((steps - np.abs(lags)) * R * np.cos(2 * np.pi * jj * lags / steps)) for jj in j])


@pytest.mark.parametrize('name,psd', [('flat', lambda f: 0.02 + 0.0 * f), ('lorentzian', lambda f: 0.05 / (1.0 + (f / 0.2) ** 2))])
def test_colored_periodogram_follows_the_psd(name, psd):
    """The trace-averaged periodogram per bin against the PSD: a periodogram bin of Gaussian noise is exponentially distributed (its standard
    deviation equals its mean S), so the average over E traces has the standard error S / sqrt(E) per bin; 5 of them."""
    steps, dt = 64, 0.5
    x = noise.colored(E_STAT, steps, dt, psd, 2468)
    j, want = _expected_periodogram(psd, steps, dt)
    if name == 'flat':
        assert np.allclose(want, 0.02, rtol=1e-9)                 # (no leakage to speak of: the expectation IS the PSD)
    got = np.mean((2 * dt / steps) * np.abs(np.fft.rfft(x, axis=1)[:, j]) ** 2, axis=0)
    dev = np.abs(got - want) / (want / np.sqrt(E_STAT))
    print('%s: largest deviation %.2f standard errors over %d bins' % (name, dev.max(), len(j)))
    assert np.all(dev <= 5.0), (name, dev.max(), int(np.argmax(dev)))
    # the record is RECORD_FACTOR pulses long: the window's mean is not removed, and its variance holds the power below 1 / (steps dt)
    # (sum_k psd(f_k) df, the Nyquist bin counting half; N = 8 x 64 = 512; standard error of a sample variance: total sqrt(2 / (E - 1)))
    N = noise.RECORD_FACTOR * steps
    S = psd(np.arange(1, N // 2 + 1) / (N * dt)) / (N * dt)
    total = np.sum(S) - 0.5 * S[-1]
    assert abs(np.var(x[:, 5], ddof=1) - total) <= 5 * total * np.sqrt(2.0 / (E_STAT - 1))


def test_one_over_f_is_colored_with_its_spectrum():
    a = noise.one_over_f(6, 16, 0.5, 0.1, 1.0, 0.05, 3)
    b = noise.colored(6, 16, 0.5, lambda f: 0.1 ** 2 / np.maximum(f, 0.05) ** 1.0, 3)
    assert np.array_equal(a, b)
    with pytest.raises(ValueError, match='f_min'):
        noise.one_over_f(6, 16, 0.5, 0.1, 1.0, 0.0, 3)
