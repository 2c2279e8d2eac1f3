"""Transfer-function GRAPE: the response of the control line for ``Grape(..., transfer=...)``.

An AWG plays P samples per line; they reach the system through a known linear response -- a zero-order hold, an interpolation, a filter,
a measured line response.  The response is a real ``steps x P`` matrix T: with the samples ``c`` (k x P), the pulse the Hamiltonian sees
is ``u = c @ T.T`` (k x steps).  Grape then optimises the samples through T (include/qoc.h, qoc_create_shaped): the fidelity terms are
those of the filtered pulse, the pulse regularisers act on the samples.
"""
import warnings

import numpy as np


class Transfer(object):
    """A response matrix and, once a run has filled them, the optimised samples.

    matrix   (steps, P) real
    samples  None until Grape(..., transfer=self) returns; then the (k, P) sample amplitudes whose response is the returned pulse"""

    def __init__(self, matrix):
        self.matrix = np.ascontiguousarray(np.asarray(matrix, dtype=np.float64))
        if self.matrix.ndim != 2:
            raise ValueError('transfer: the response matrix has shape %s, expected (steps, P)' % (self.matrix.shape,))
        self.samples = None

    @property
    def n_samples(self):
        return self.matrix.shape[1]


_warned_l1 = False


def validate(T, steps):
    """Checks a response (a Transfer or a steps x P array) against a problem of `steps` time slices and returns it as a Transfer.
    Raises ValueError; warns once per process when a row's l1 norm exceeds 1 (maxA then no longer bounds the pulse)."""
    global _warned_l1
    tr = T if isinstance(T, Transfer) else Transfer(T)
    M = tr.matrix
    if M.shape[0] != int(steps) or M.shape[1] < 1:
        raise ValueError('transfer: the response matrix has shape %s, expected (%d, P) with P >= 1' % (M.shape, int(steps)))
    if not np.all(np.isfinite(M)):
        raise ValueError('transfer: the response matrix has non-finite entries')
    dead = np.flatnonzero(~np.any(M != 0.0, axis=0))
    if dead.size:
        raise ValueError('transfer: column %d of the response matrix is zero (the sample never reaches the pulse)' % dead[0])
    l1 = np.max(np.sum(np.abs(M), axis=1))
    if l1 > 1.0 + 1e-12 and not _warned_l1:
        _warned_l1 = True
        warnings.warn('transfer: a row of the response matrix has l1 norm %.6g > 1: maxA no longer bounds the pulse amplitude' % l1)
    return tr


def apply(T, samples):
    """The pulse (k, steps) that the samples (k, P) produce through the response T (a Transfer or a steps x P array)."""
    M = T.matrix if isinstance(T, Transfer) else np.asarray(T, dtype=np.float64)
    samples = np.asarray(samples, dtype=np.float64)
    if samples.ndim != 2 or samples.shape[1] != M.shape[1]:
        raise ValueError('transfer: samples have shape %s, expected (k, %d)' % (samples.shape, M.shape[1]))
    return samples @ M.T


def _check_sizes(steps, P):
    steps, P = int(steps), int(P)
    if P < 1 or steps < P:
        raise ValueError('transfer: %d samples for %d time slices (1 <= P <= steps)' % (P, steps))
    return steps, P


def hold(steps, P):
    """Zero-order hold: sample p drives the slices t with t * P // steps == p (steps need not be a multiple of P)."""
    steps, P = _check_sizes(steps, P)
    M = np.zeros((steps, P))
    t = np.arange(steps)
    M[t, t * P // steps] = 1.0
    return Transfer(M)


def linear_interp(steps, P):
    """Linear interpolation between the samples, sample p sitting at the centre of its hold window; constant beyond the first and
    the last centre.  Every row sums to 1."""
    steps, P = _check_sizes(steps, P)
    M = np.zeros((steps, P))
    if P == 1:
        M[:, 0] = 1.0
        return Transfer(M)
    x = (np.arange(steps) + 0.5) * P / steps - 0.5        # slice centres in units of the sample index
    x = np.clip(x, 0.0, P - 1.0)
    lo = np.minimum(np.floor(x).astype(int), P - 2)
    f = x - lo
    t = np.arange(steps)
    M[t, lo] = 1.0 - f
    M[t, lo + 1] += f
    return Transfer(M)


def gaussian_filter(steps, P, total_time, sigma):
    """The hold, smoothed by a Gaussian line response of standard deviation `sigma` (in the unit of total_time): slice t sees the
    row-normalised Gaussian average, truncated at 4 sigma, of the held samples around it."""
    steps, P = _check_sizes(steps, P)
    dt = float(total_time) / steps
    s = float(sigma) / dt                                  # in slices
    if not s > 0.0:
        raise ValueError('transfer: sigma = %r (> 0)' % (sigma,))
    H = hold(steps, P).matrix
    half = int(np.floor(4.0 * s))
    G = np.zeros((steps, steps))
    for t in range(steps):
        lo, hi = max(0, t - half), min(steps, t + half + 1)
        g = np.exp(-0.5 * ((np.arange(lo, hi) - t) / s) ** 2)
        G[t, lo:hi] = g / g.sum()
    return Transfer(G @ H)
