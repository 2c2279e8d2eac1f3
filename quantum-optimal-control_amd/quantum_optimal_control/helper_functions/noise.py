"""Noise traces: seeded generators of sampled noise trajectories for ``Grape(..., robust=...)`` and ``HipEngine.set_traces``.

A robust ensemble models an error that is constant over the pulse, a collapse operator models white (Markovian) noise.  What limits gates in
practice lies between the two: 1/f-like flux and charge noise, a detuning that drifts with a correlation time comparable to the gate, two-level
fluctuators that switch during the pulse.  The standard answer is to optimise one pulse over an ensemble of sampled noise trajectories: member e
of the ensemble has, at slice t, the drift H0 + sum_q (offsets[e, q] + traces[e, q, t]) P_q (include/qoc.h, qoc_set_traces).

Every generator returns an (E, steps) array -- one trace per member, in the units the perturbation offsets have (the factor in front of P_q) --
and takes ``rng`` as a numpy.random.Generator or an int seed: the same seed gives the same traces.  ``ensemble`` stacks one such array per
operator into the dict Grape(robust=...) takes.
"""
import numpy as np

from quantum_optimal_control.helper_functions import robust as _robust

# colored(): the synthesised record is this many times longer than the pulse (rounded up to a power of two), and a window of `steps` samples is
# cut out of it, so that a trace is not periodic in the pulse length and holds frequencies below 1 / (steps dt)
RECORD_FACTOR = 8


def _generator(rng):
    return rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)


def _sizes(E, steps):
    E, steps = int(E), int(steps)
    if E < 1 or steps < 1:
        raise ValueError('noise: E and steps must be >= 1, got %d and %d' % (E, steps))
    return E, steps


def quasi_static(E, steps, sigma, rng):
    """One N(0, sigma^2) value per trace, constant over the pulse: what a robust ensemble of offsets models."""
    E, steps = _sizes(E, steps)
    return np.repeat(float(sigma) * _generator(rng).standard_normal((E, 1)), steps, axis=1)


def white(E, steps, sigma, rng):
    """Independent N(0, sigma^2) values per slice."""
    E, steps = _sizes(E, steps)
    return float(sigma) * _generator(rng).standard_normal((E, steps))


def ornstein_uhlenbeck(E, steps, dt, sigma, tau, rng):
    """A stationary Ornstein-Uhlenbeck process of standard deviation sigma and correlation time tau, sampled every dt by its exact discretisation
    x[t+1] = a x[t] + sigma sqrt(1 - a^2) xi[t], a = exp(-dt / tau), xi ~ N(0, 1), from the stationary start x[0] ~ N(0, sigma^2): the
    autocorrelation is sigma^2 a^|lag| at every slice."""
    E, steps = _sizes(E, steps)
    if not (dt > 0 and tau > 0):
        raise ValueError('noise: dt and tau must be > 0')
    a = np.exp(-float(dt) / float(tau))
    xi = _generator(rng).standard_normal((E, steps))
    x = np.empty((E, steps))
    x[:, 0] = float(sigma) * xi[:, 0]
    kick = float(sigma) * np.sqrt(1.0 - a * a)
    for t in range(1, steps):
        x[:, t] = a * x[:, t - 1] + kick * xi[:, t]
    return x


def colored(E, steps, dt, psd, rng):
    """Gaussian noise with the one-sided power spectral density psd(f) (a callable of the frequency in 1 / the unit of dt, returning power per unit
    frequency; it is never called at f = 0, the record has no mean), by spectral synthesis: a record of N = RECORD_FACTOR (= 8) x steps samples,
    rounded up to a power of two, gets independent complex Gaussian Fourier coefficients of variance psd(f_k) N / (2 dt) at f_k = k / (N dt),
    k = 1 .. N/2 (the Nyquist coefficient real), so that the periodogram (2 dt / N) |X_k|^2 of the record has the mean psd(f_k); a window of `steps`
    samples at a random position is cut from it.  The record being 8 or more pulses long, a trace is not periodic in the pulse length and carries
    the frequencies below 1 / (steps dt) as a drift."""
    E, steps = _sizes(E, steps)
    if not dt > 0:
        raise ValueError('noise: dt must be > 0')
    g = _generator(rng)
    N = 1 << int(np.ceil(np.log2(RECORD_FACTOR * steps)))
    f = np.arange(1, N // 2 + 1) / (N * float(dt))
    S = np.asarray(psd(f), dtype=np.float64)
    if S.shape != f.shape or not np.all(np.isfinite(S)) or np.any(S < 0):
        raise ValueError('noise: psd must return one finite value >= 0 per frequency')
    amp = np.sqrt(S * N / (2.0 * float(dt)))
    re, im = g.standard_normal((E, N // 2)), g.standard_normal((E, N // 2))
    spec = np.zeros((E, N // 2 + 1), dtype=np.complex128)
    spec[:, 1:] = amp * (re + 1j * im) / np.sqrt(2.0)
    spec[:, -1] = amp[-1] * re[:, -1]                    # (Nyquist: real, the full variance in one component)
    record = np.fft.irfft(spec, n=N, axis=1)             # (irfft divides by N: x[s] = (1 / N) sum_k X_k e^{2 pi i k s / N})
    start = g.integers(0, N - steps + 1, size=E)
    return np.stack([record[e, start[e]:start[e] + steps] for e in range(E)])


def one_over_f(E, steps, dt, amplitude, alpha, f_min, rng):
    """colored() with the one-sided spectrum psd(f) = amplitude^2 / max(f, f_min)^alpha: 1/f^alpha noise, flat below the cut-off f_min > 0 (what
    bounds the power of the slow drift)."""
    if not f_min > 0:
        raise ValueError('noise: f_min must be > 0')
    return colored(E, steps, dt, lambda f: float(amplitude) ** 2 / np.maximum(f, float(f_min)) ** float(alpha), rng)


def ensemble(operators, traces, offsets=None, amp_scales=None, k=None, weights=None, risk=0.0, collapse_ops=None, rate_scales=None):
    """The dict Grape(robust=...) takes, from one (E, steps) array of traces per operator: traces (E, q, steps), offsets (E, q) (default zeros),
    amp_scales (E, k) (default ones: k is then required), weights (E,) (default uniform), risk, and the decay keys when collapse_ops is given."""
    operators = [_robust.as_operator(p) for p in operators]
    traces = [np.asarray(tr, dtype=np.float64) for tr in traces]
    if len(traces) != len(operators) or not operators:
        raise ValueError('noise.ensemble: one (E, steps) array of traces per operator (%d operators, %d arrays)' % (len(operators), len(traces)))
    if any(tr.ndim != 2 or tr.shape != traces[0].shape for tr in traces):
        raise ValueError('noise.ensemble: every array of traces is (E, steps), got %s' % ([tr.shape for tr in traces],))
    E, q = traces[0].shape[0], len(operators)
    if amp_scales is None and k is None:
        raise ValueError('noise.ensemble: k (the number of control Hamiltonians) is required without amp_scales')
    ens = dict(operators=operators, traces=np.stack(traces, axis=1), offsets=np.zeros((E, q)) if offsets is None else offsets,
               amp_scales=np.ones((E, int(k))) if amp_scales is None else amp_scales, weights=weights, risk=risk)
    if ens['weights'] is None:
        del ens['weights']
    if collapse_ops is not None:
        ens['collapse_ops'] = list(collapse_ops)
        if rate_scales is not None:
            ens['rate_scales'] = rate_scales
    elif rate_scales is not None:
        raise ValueError('noise.ensemble: rate_scales given without collapse_ops')
    return _robust.validate(ens, None, int(np.shape(ens['amp_scales'])[1]), sparse=None)
