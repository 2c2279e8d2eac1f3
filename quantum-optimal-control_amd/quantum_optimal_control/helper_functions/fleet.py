"""Device fleets: one pulse per device, for many devices that differ slightly, for ``Grape(..., fleet=...)``.

A fleet has F devices.  Device f is an ensemble of E members (E = 1: the plain case): member e has the drift
H0 + sum_q offsets[f, e, q] P_q and the control Hamiltonians amp_scales[f, e, j] H_j.  The devices share the operators P_q, the member
weights and the risk, the targets, the states of interest, maxA, the regularisers, the line and the control map; nothing else couples them.
One engine holds R control sets per device (``restarts=R``), device-major, and optimises every device's own pulse in the same launches
(include/qoc.h, qoc_create_fleet).
"""
import numpy as np

from quantum_optimal_control.helper_functions import robust as _robust


class Fleet(object):
    """offsets (F, E, q), amp_scales (F, E, k), operators (q Hermitian n x n matrices), weights (E,) and risk (beta >= 0).  After a
    Grape(fleet=...) run: losses (F,) of every device's best control set, best (F,) the restart that won, member_losses (F, E) of that
    control set and iterations (F,) it took."""

    def __init__(self, operators, offsets, amp_scales, weights=None, risk=0.0):
        self.operators = [np.asarray(p) for p in operators]
        self.offsets = np.asarray(offsets, dtype=np.float64)
        self.amp_scales = np.asarray(amp_scales, dtype=np.float64)
        self.weights = None if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        self.risk = risk
        self.losses = self.best = self.member_losses = self.iterations = None

    @property
    def n_devices(self):
        return int(self.amp_scales.shape[0])

    @property
    def n_members(self):
        return int(self.amp_scales.shape[1])

    def device(self, f):
        """Device f as the dict Grape(robust=...) takes: its member rows, the shared operators, weights and risk."""
        w = np.ones(self.n_members) if self.weights is None else self.weights
        return dict(operators=list(self.operators), offsets=np.array(self.offsets[f]), amp_scales=np.array(self.amp_scales[f]),
                    weights=np.array(w), risk=self.risk)


def _device_rows(values, F, width, name):
    a = np.asarray(values, dtype=np.float64)
    if a.ndim == 1 and width == 1:
        a = a.reshape(-1, 1)
    if a.ndim != 2 or a.shape[1] != width or (F is not None and a.shape[0] != F):
        raise ValueError('fleet: %s have shape %s, expected (%s, %d)' % (name, a.shape, 'F' if F is None else F, width))
    return a


def devices(operators=(), offsets=None, amp_scales=None, k=None):
    """A fleet of one member per device: offsets (F, q), one row of perturbation values per device, and amp_scales (F, k) or None (ones)."""
    if k is None:
        raise ValueError('fleet.devices: k (the number of pulses) is required')
    k = int(k)
    operators = [np.asarray(p) for p in operators]
    q = len(operators)
    F = None
    if offsets is not None and (q or np.size(offsets)):
        if q == 0:
            raise ValueError('fleet: offsets given without operators')
        offsets = _device_rows(offsets, None, q, 'offsets')
        F = offsets.shape[0]
    elif q:
        raise ValueError('fleet: offsets (F x q) are required with operators')
    if amp_scales is not None:
        amp_scales = _device_rows(amp_scales, F, k, 'amp_scales')
        F = amp_scales.shape[0]
    if F is None:
        raise ValueError('fleet: the fleet has no devices (give offsets or amp_scales)')
    off = np.zeros((F, 1, q)) if not q else offsets.reshape(F, 1, q)
    amp = np.ones((F, 1, k)) if amp_scales is None else amp_scales.reshape(F, 1, k)
    return validate(Fleet(operators, off, amp), None, k)


def around(operators=(), offsets=None, amp_scales=None, robust=None, k=None):
    """Every device gets the ensemble `robust` (a Grape(robust=...) dict over the same operators) centred on it: member e of device f has the
    offsets offsets[f] + robust offsets[e] and the scales amp_scales[f] * robust amp_scales[e].  Weights and risk are the ensemble's."""
    if robust is None:
        raise ValueError('fleet.around: robust (the ensemble every device gets) is required')
    if k is None:
        k = np.shape(robust['amp_scales'])[1] if robust.get('amp_scales') is not None else None
    centre = devices(operators, offsets, amp_scales, k=k)
    q = len(centre.operators)
    ens = _robust.validate(robust, centre.operators[0].shape[0] if q else None, int(k))
    if len(ens['operators']) != q or any(not np.array_equal(a, b) for a, b in zip(ens['operators'], centre.operators)):
        raise ValueError('fleet.around: the ensemble must perturb the fleet\'s own operators (%d given, the ensemble has %d)'
                         % (q, len(ens['operators'])))
    off = centre.offsets[:, 0][:, None, :] + ens['offsets'][None, :, :]
    amp = centre.amp_scales[:, 0][:, None, :] * ens['amp_scales'][None, :, :]
    return validate(Fleet(centre.operators, off, amp, weights=ens['weights'], risk=ens['risk']), None, int(k))


def validate(fleet, n, k):
    """Checks a Fleet against a problem of n levels (None: from the operators) and k pulses and returns a normalised copy: operators complex
    Hermitian n x n, offsets (F, E, q), amp_scales (F, E, k), weights (E,) summing to 1 (default uniform), risk a finite float >= 0.
    Raises ValueError with the cause."""
    if not isinstance(fleet, Fleet):
        raise ValueError('fleet: a helper_functions.fleet.Fleet (fleet.devices, fleet.around)')
    amp = np.array(fleet.amp_scales, dtype=np.float64)            # (copies: the normalised fleet owns its arrays)
    if amp.ndim != 3 or amp.shape[2] != k or amp.shape[0] < 1 or amp.shape[1] < 1:
        raise ValueError('fleet: amp_scales have shape %s, expected (F, E, %d)' % (amp.shape, k))
    F, E = amp.shape[:2]
    q = len(fleet.operators)
    off = np.array(fleet.offsets, dtype=np.float64)
    if off.size == 0 and q == 0:
        off = np.zeros((F, E, 0))
    if off.shape != (F, E, q):
        raise ValueError('fleet: offsets have shape %s, expected (%d, %d, %d)' % (off.shape, F, E, q))
    if not (np.all(np.isfinite(amp)) and np.all(np.isfinite(off))):
        raise ValueError('fleet: offsets and amp_scales must be finite')
    # operators, weights and risk: the ensemble's rules (helper_functions/robust.py), on device 0's rows
    try:
        ens = _robust.validate(dict(operators=fleet.operators, offsets=off[0], amp_scales=amp[0], weights=fleet.weights, risk=fleet.risk), n, k)
    except ValueError as err:
        raise ValueError(str(err).replace('robust:', 'fleet:', 1))
    return Fleet(ens['operators'], off, amp, weights=ens['weights'], risk=ens['risk'])


def tile_bases(base, F):
    """The start points of a fleet's F R control sets, device-major, from the R start points of Grape(restarts=R) (R, k, P) -- every device starts
    from the same R points -- or from per-device first points (F, R, k, P)."""
    base = np.asarray(base, dtype=np.float64)
    if base.ndim == 3:
        base = np.broadcast_to(base[None], (F,) + base.shape)
    return np.ascontiguousarray(base.reshape((F * base.shape[1],) + base.shape[2:]))


def select_best(loss, F):
    """The winning restart of every device: the argmin of `loss` (F R,) over each device's R control sets, first smallest wins; a NaN never wins
    unless all of a device's losses are NaN (then restart 0).  Returns (best (F,) restart indices, sets (F,) control-set indices)."""
    loss = np.asarray(loss, dtype=np.float64).reshape(F, -1)
    R = loss.shape[1]
    best = np.argmin(np.where(np.isnan(loss), np.inf, loss), axis=1)
    best = np.where(np.all(np.isnan(loss), axis=1), 0, best).astype(int)
    return best, np.arange(F) * R + best


def choose_taylor(fleet, H0, Hops, control_map, maxA, U0, total_time, steps, unitary_error, state_transfer, no_scaling):
    """(Taylor terms, squarings): the maximum over every member of every device of robust.choose_taylor / control_map.choose_taylor."""
    best_t, best_s = 0, 0
    for f in range(fleet.n_devices):
        dev = fleet.device(f)
        if control_map is not None:
            from quantum_optimal_control.helper_functions import control_map as _cmap
            t, s = _cmap.choose_taylor(control_map, H0, Hops, dev, maxA, U0, total_time, steps, unitary_error, state_transfer, no_scaling)
        else:
            t, s = _robust.choose_taylor(H0, Hops, dev, maxA, U0, total_time, steps, unitary_error, state_transfer, no_scaling)
        best_t, best_s = max(best_t, int(t)), max(best_s, int(s))
    return best_t, best_s
