"""Device fleets: one pulse per device, for many devices that differ slightly, for ``Grape(..., fleet=...)``.

A fleet has F devices.  Device f is an ensemble of E members (E = 1: the plain case): member e has the drift
H0 + sum_q offsets[f, e, q] P_q and the control Hamiltonians amp_scales[f, e, j] H_j.  The devices share the operators P_q, the member
weights and the risk, the targets, the states of interest, maxA, the regularisers, the line and the control map; nothing else couples them.
One engine holds R control sets per device (``restarts=R``), device-major, and optimises every device's own pulse in the same launches
(include/qoc.h, qoc_create_fleet).

Decay per device: a fleet may carry collapse_ops (c operators as Grape(collapse_ops=...) takes them, shared by the devices) and rate_scales
(F, E, c): member e of device f decays through sqrt(rate_scales[f, e, j]) C_j, and every member is an open problem (qoc_create_open_fleet).

Noise traces: a fleet may carry traces (F, E, q, steps): member e of device f then runs offsets[f, e, q] + traces[f, e, q, t] at slice t
(helper_functions/robust.py, include/qoc.h qoc_set_traces).
"""
import numpy as np

from quantum_optimal_control.helper_functions import robust as _robust


class Fleet(object):
    """offsets (F, E, q), amp_scales (F, E, k), operators (q Hermitian n x n matrices), weights (E,) and risk (beta >= 0).  After a
    Grape(fleet=...) run: losses (F,) of every device's best control set, best (F,) the restart that won, member_losses (F, E) of that
    control set and iterations (F,) it took.  collapse_ops (c operators, or None: closed devices) and rate_scales (F, E, c), default ones.
    traces (F, E, q, steps), or None: noise traces added per slice to the offsets."""

    def __init__(self, operators, offsets, amp_scales, weights=None, risk=0.0, collapse_ops=None, rate_scales=None, traces=None):
        self.traces = None if traces is None else np.asarray(traces, dtype=np.float64)
        self.operators = [_robust.as_operator(p) for p in operators]
        self.offsets = np.asarray(offsets, dtype=np.float64)
        self.amp_scales = np.asarray(amp_scales, dtype=np.float64)
        self.weights = None if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        self.risk = risk
        if rate_scales is not None and collapse_ops is None:
            raise ValueError('fleet: rate_scales given without collapse_ops')
        self.collapse_ops = None if collapse_ops is None else list(collapse_ops)
        self.rate_scales = None if rate_scales is None else np.asarray(rate_scales, dtype=np.float64)
        self.losses = self.best = self.member_losses = self.iterations = None

    @property
    def n_devices(self):
        return int(self.amp_scales.shape[0])

    @property
    def n_members(self):
        return int(self.amp_scales.shape[1])

    def device(self, f):
        """Device f as the dict Grape(robust=...) takes: its member rows, the shared operators, weights and risk, and its decay."""
        w = np.ones(self.n_members) if self.weights is None else self.weights
        dev = dict(operators=list(self.operators), offsets=np.array(self.offsets[f]), amp_scales=np.array(self.amp_scales[f]),
                   weights=np.array(w), risk=self.risk)
        if self.collapse_ops is not None:
            dev['collapse_ops'] = list(self.collapse_ops)
            dev['rate_scales'] = (np.ones((self.n_members, len(self.collapse_ops))) if self.rate_scales is None
                                  else np.array(self.rate_scales[f]))
        if getattr(self, 'traces', None) is not None:
            dev['traces'] = np.array(self.traces[f])
        return dev

    @property
    def has_decay(self):
        return self.collapse_ops is not None


def _device_rows(values, F, width, name):
    a = np.asarray(values, dtype=np.float64)
    if a.ndim == 1 and width == 1:
        a = a.reshape(-1, 1)
    if a.ndim != 2 or a.shape[1] != width or (F is not None and a.shape[0] != F):
        raise ValueError('fleet: %s have shape %s, expected (%s, %d)' % (name, a.shape, 'F' if F is None else F, width))
    return a


def devices(operators=(), offsets=None, amp_scales=None, k=None, collapse_ops=None, rate_scales=None, traces=None):
    """A fleet of one member per device: offsets (F, q), one row of perturbation values per device, and amp_scales (F, k) or None (ones).
    collapse_ops with rate_scales (F, c) or None (ones): every device decays through its own sqrt(rate_scales[f, j]) C_j.
    traces (F, q, steps) or None: every device's own noise traces."""
    if k is None:
        raise ValueError('fleet.devices: k (the number of pulses) is required')
    k = int(k)
    operators = [_robust.as_operator(p) for p in operators]
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
    if rate_scales is not None:
        if collapse_ops is None:
            raise ValueError('fleet: rate_scales given without collapse_ops')
        rate_scales = _device_rows(rate_scales, F, len(collapse_ops), 'rate_scales')
        F = rate_scales.shape[0]
    if F is None:
        raise ValueError('fleet: the fleet has no devices (give offsets, amp_scales or rate_scales)')
    off = np.zeros((F, 1, q)) if not q else offsets.reshape(F, 1, q)
    amp = np.ones((F, 1, k)) if amp_scales is None else amp_scales.reshape(F, 1, k)
    rates = None if rate_scales is None else rate_scales.reshape(F, 1, -1)
    if traces is not None:
        traces = np.asarray(traces, dtype=np.float64)
        if traces.ndim != 3 or traces.shape[:2] != (F, q):
            raise ValueError('fleet: traces have shape %s, expected (%d, %d, steps)' % (traces.shape, F, q))
        traces = traces[:, None]
    return validate(Fleet(operators, off, amp, collapse_ops=collapse_ops, rate_scales=rates, traces=traces), None, k, sparse=None)


def around(operators=(), offsets=None, amp_scales=None, robust=None, k=None, collapse_ops=None, rate_scales=None, traces=None):
    """Every device gets the ensemble `robust` (a Grape(robust=...) dict over the same operators) centred on it: member e of device f has the
    offsets offsets[f] + robust offsets[e] and the scales amp_scales[f] * robust amp_scales[e].  Weights and risk are the ensemble's.
    Decay: the collapse operators are the fleet's (collapse_ops) or the ensemble's -- the same list when both carry one --, and member e of
    device f has the rate scales rate_scales[f] * robust rate_scales[e] (either defaults to ones).
    traces (F, E, q, steps) or None: the members' noise traces, device by device; the ensemble's own traces (E, q, steps), when it carries some, are
    added to every device's."""
    if robust is None:
        raise ValueError('fleet.around: robust (the ensemble every device gets) is required')
    if k is None:
        k = np.shape(robust['amp_scales'])[1] if robust.get('amp_scales') is not None else None
    centre = devices(operators, offsets, amp_scales, k=k, collapse_ops=collapse_ops, rate_scales=rate_scales)
    q = len(centre.operators)
    ens = _robust.validate(robust, centre.operators[0].shape[0] if q else None, int(k), sparse=None)
    if len(ens['operators']) != q or any(not _robust.same_operator(a, b) for a, b in zip(ens['operators'], centre.operators)):
        raise ValueError('fleet.around: the ensemble must perturb the fleet\'s own operators (%d given, the ensemble has %d)'
                         % (q, len(ens['operators'])))
    off = centre.offsets[:, 0][:, None, :] + ens['offsets'][None, :, :]
    amp = centre.amp_scales[:, 0][:, None, :] * ens['amp_scales'][None, :, :]
    cops, rates = centre.collapse_ops, None
    if 'collapse_ops' in ens:
        if cops is not None and (len(cops) != len(ens['collapse_ops']) or any(not np.array_equal(a, b) for a, b in zip(cops, ens['collapse_ops']))):
            raise ValueError('fleet.around: the ensemble and the fleet must carry the same collapse operators')
        cops = ens['collapse_ops']
    if cops is not None:
        F, E, c = off.shape[0], off.shape[1], len(cops)
        dev_r = np.ones((F, 1, c)) if centre.rate_scales is None else centre.rate_scales
        rates = dev_r[:, 0][:, None, :] * (ens['rate_scales'] if 'rate_scales' in ens else np.ones((E, c)))[None, :, :]
    if traces is not None:
        traces = np.asarray(traces, dtype=np.float64)
        if traces.ndim != 4 or traces.shape[:3] != off.shape:
            raise ValueError('fleet: traces have shape %s, expected %s + (steps,)' % (traces.shape, off.shape))
    if 'traces' in ens:
        traces = np.broadcast_to(ens['traces'][None], off.shape + ens['traces'].shape[2:]) + (0.0 if traces is None else traces)
    return validate(Fleet(centre.operators, off, amp, weights=ens['weights'], risk=ens['risk'], collapse_ops=cops, rate_scales=rates, traces=traces),
                    None, int(k), sparse=None)


def validate(fleet, n, k, sparse=False, steps=None):
    """Checks a Fleet against a problem of n levels (None: from the operators) and k pulses and returns a normalised copy: operators complex
    Hermitian n x n, offsets (F, E, q), amp_scales (F, E, k), weights (E,) summing to 1 (default uniform), risk a finite float >= 0.
    collapse_ops (None, or c complex n x n matrices) and rate_scales (F, E, c), finite and >= 0 (default ones; None without collapse_ops).
    Raises ValueError with the cause.  sparse=True (the sparse state-transfer route): the operators come back as complex CSR and are never
    densified, and decay is refused; sparse=None (the builders): the operators stay as given (robust.validate's rules).
    traces (None, or (F, E, q, steps), finite, q >= 1; steps given: checked against it)."""
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
    dev0 = dict(operators=fleet.operators, offsets=off[0], amp_scales=amp[0], weights=fleet.weights, risk=fleet.risk)
    cops, rates = getattr(fleet, 'collapse_ops', None), getattr(fleet, 'rate_scales', None)
    if rates is not None and cops is None:
        raise ValueError('fleet: rate_scales given without collapse_ops')
    if cops is not None:
        c = len(cops)
        rates = np.ones((F, E, c)) if rates is None else np.array(rates, dtype=np.float64)
        if rates.shape != (F, E, c):
            raise ValueError('fleet: rate_scales have shape %s, expected (%d, %d, %d)' % (rates.shape, F, E, c))
        if not np.all(np.isfinite(rates)) or np.any(rates < 0):
            raise ValueError('fleet: rate_scales must be finite and >= 0')
        dev0.update(collapse_ops=cops, rate_scales=rates[0])
    traces = getattr(fleet, 'traces', None)
    if traces is not None:
        traces = np.array(traces, dtype=np.float64)
        if q < 1:
            raise ValueError('fleet: traces given without operators (a trace is added to a perturbation row: q >= 1)')
        if traces.ndim != 4 or traces.shape[:3] != (F, E, q) or traces.shape[3] < 1:
            raise ValueError('fleet: traces have shape %s, expected (%d, %d, %d, steps)' % (traces.shape, F, E, q))
        if steps is not None and traces.shape[3] != int(steps):
            raise ValueError('fleet: traces have %d slices, the pulse has %d' % (traces.shape[3], int(steps)))
        if not np.all(np.isfinite(traces)):
            raise ValueError('fleet: traces must be finite')
    try:
        ens = _robust.validate(dev0, n, k, sparse=sparse)
    except ValueError as err:
        raise ValueError(str(err).replace('robust:', 'fleet:', 1))
    return Fleet(ens['operators'], off, amp, weights=ens['weights'], risk=ens['risk'], collapse_ops=ens.get('collapse_ops'), rate_scales=rates,
                 traces=traces)


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
    """(Taylor terms, squarings): the maximum over every member of every device of robust.choose_taylor / control_map.choose_taylor.  With traces a
    member's problem uses, per operator, the value of offsets + traces[t] of largest magnitude over t (robust.taylor_view)."""
    best_t, best_s = 0, 0
    for f in range(fleet.n_devices):
        dev = _robust.taylor_view(fleet.device(f))
        if control_map is not None:
            from quantum_optimal_control.helper_functions import control_map as _cmap
            t, s = _cmap.choose_taylor(control_map, H0, Hops, dev, maxA, U0, total_time, steps, unitary_error, state_transfer, no_scaling)
        else:
            t, s = _robust.choose_taylor(H0, Hops, dev, maxA, U0, total_time, steps, unitary_error, state_transfer, no_scaling)
        best_t, best_s = max(best_t, int(t)), max(best_s, int(s))
    return best_t, best_s
