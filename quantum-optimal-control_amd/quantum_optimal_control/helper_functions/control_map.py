"""Control maps for ``Grape(..., control_map=...)``: the coefficients of the Hamiltonian as functions of the pulses.

Without a map every pulse multiplies exactly one operator, linearly: H(t) = H0 + sum_k u_k(t) H_k.  A map stands between the pulse a line
delivers and the coefficient the Hamiltonian sees.  For the k pulses v_j[t] (what a member of an ensemble runs on: its amplitude scale times
maxA_j sin(base_j[t]), or the filtered pulse of a transfer function) and the r operators G_i the map feeds,

    c_i[t] = F[i, t] + sum_j M[i, j, t] * p_ij(v_j[t]),      p_ij(x) = sum_{d = 1 .. D} alpha[i, j, d - 1] x^d

and H(t) = H0 + sum_i c_i(t) G_i (include/qoc.h, qoc_create_mapped).  alpha is (r, k, D); M is (r, k, steps) or None (ones); F is
(r, steps) or None (zeros); r need not equal k.  That covers crosstalk (``linear``), carriers and rotating frames (``carriers``), a nonlinear
response of each line (``polynomial``) and fixed drives or time-dependent drifts (``fixed``); ``compose``, ``combine`` and ``stack`` build one map
out of several.  Cross terms between two pulses are outside the model.  ``apply`` is the NumPy statement of the formula, ``pullback`` of its chain
rule.  After a Grape call ``cm.coefficients`` holds the r x steps coefficients of the nominal member, as ``line.samples`` does for a transfer.
"""
import numpy as np

MAX_DEGREE = 8          # QOC_MAP_MAX_DEGREE (csrc/qoc_control_map.h)
MAX_TERMS = 64          # QOC_MAP_MAX_TERMS


class ControlMap(object):
    """alpha (r, k, D), mix (r, k, steps) or None, fixed (r, steps) or None; ``coefficients`` is filled by Grape (r x steps, nominal member)."""

    def __init__(self, alpha, mix=None, fixed=None):
        self.alpha = np.asarray(alpha, dtype=np.float64)
        self.mix = None if mix is None else np.asarray(mix, dtype=np.float64)
        self.fixed = None if fixed is None else np.asarray(fixed, dtype=np.float64)
        self.coefficients = None

    n_terms = property(lambda self: self.alpha.shape[0])
    n_pulses = property(lambda self: self.alpha.shape[1])
    degree = property(lambda self: self.alpha.shape[2])

    @property
    def steps(self):
        """The number of time slices the map is tied to, or None when it has neither mix nor fixed."""
        if self.mix is not None:
            return self.mix.shape[2]
        return None if self.fixed is None else self.fixed.shape[1]

    def __repr__(self):
        return 'ControlMap(terms=%d, pulses=%d, degree=%d, mix=%s, fixed=%s)' % (self.n_terms, self.n_pulses, self.degree,
                                                                              self.mix is not None, self.fixed is not None)


# ---- builders ---------------------------------------------------------------------------------------------------------------------------------

def linear(X):
    """Crosstalk / mixing: c = X v with X an r x k matrix (X[i, j]: how much of line j reaches operator i)."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError('control_map.linear: X has shape %s, expected (r, k)' % (X.shape,))
    return ControlMap(X[:, :, None].copy())


def identity(k):
    """Every pulse feeds its own operator, linearly: the model without a map."""
    return linear(np.eye(int(k)))


def carriers(freqs, phases, total_time, steps):
    """Pulse j is the envelope of a carrier: operators 2 j and 2 j + 1 (its in-phase and quadrature operator, e.g. X_j and Y_j) get
    v_j[t] cos(2 pi f_j t' + phi_j) and v_j[t] sin(2 pi f_j t' + phi_j) at the slice mid-points t' = (t + 1/2) dt.  r = 2 k."""
    f = np.asarray(freqs, dtype=np.float64).reshape(-1)
    ph = np.broadcast_to(np.asarray(phases, dtype=np.float64), f.shape)
    k, steps = f.shape[0], int(steps)
    if k < 1 or steps < 1:
        raise ValueError('control_map.carriers: at least one carrier and one time slice')
    t = (np.arange(steps) + 0.5) * (float(total_time) / steps)
    alpha = np.zeros((2 * k, k, 1))
    mix = np.zeros((2 * k, k, steps))
    for j in range(k):
        arg = 2.0 * np.pi * f[j] * t + ph[j]
        alpha[2 * j, j, 0] = alpha[2 * j + 1, j, 0] = 1.0
        mix[2 * j, j], mix[2 * j + 1, j] = np.cos(arg), np.sin(arg)
    return ControlMap(alpha, mix=mix)


def polynomial(alpha):
    """A nonlinear response.  alpha (k, D): line j delivers p_j(v) = sum_d alpha[j, d - 1] v^d to its own operator j (r = k; compose it under
    ``linear`` or ``carriers``).  alpha (r, k, D): the general form, one polynomial per (operator, pulse) pair."""
    a = np.asarray(alpha, dtype=np.float64)
    if a.ndim == 2:
        k, D = a.shape
        full = np.zeros((k, k, D))
        full[np.arange(k), np.arange(k)] = a
        return ControlMap(full)
    if a.ndim != 3:
        raise ValueError('control_map.polynomial: alpha has shape %s, expected (k, D) or (r, k, D)' % (a.shape,))
    return ControlMap(a.copy())


def fixed(waveforms):
    """Fixed drives and time-dependent drifts: operator i gets the known waveform F[i, t] whatever the pulses do (an always-on pump, a
    neighbour's pulse).  It takes no pulse at all and is no map on its own: ``combine`` it with one that feeds the same operators, or ``stack``
    it below one (it then adopts that map's pulses)."""
    F = np.asarray(waveforms, dtype=np.float64)
    if F.ndim != 2:
        raise ValueError('control_map.fixed: the waveforms have shape %s, expected (r, steps)' % (F.shape,))
    return ControlMap(np.zeros((F.shape[0], 0, 1)), fixed=F.copy())


# ---- combining --------------------------------------------------------------------------------------------------------------------------------

def _padded(alpha, k, D):
    """alpha with D powers (zeros above its own degree); a map of no pulses (``fixed``) widened to k columns of zeros."""
    out = np.zeros((alpha.shape[0], k, D))
    out[:, :alpha.shape[1], :alpha.shape[2]] = alpha
    return out


def _full_mix(cm, k, steps):
    return np.ones((cm.n_terms, k, steps)) if cm.mix is None else cm.mix


def _common_pulses(maps, who):
    ks = {m.n_pulses for m in maps if m.n_pulses > 0}
    if len(ks) != 1:
        raise ValueError('control_map.%s: the maps take different numbers of pulses %s' % (who, [m.n_pulses for m in maps]))
    return ks.pop()


def _common_steps(maps, who):
    steps = {m.steps for m in maps if m.steps is not None}
    if len(steps) > 1:
        raise ValueError('control_map.%s: the maps are tied to different numbers of time slices %s' % (who, sorted(steps)))
    return steps.pop() if steps else None


def compose(outer, inner):
    """outer after inner: line j first responds with its own polynomial p_j (inner = ``polynomial`` of a (k, D) array: r = k, diagonal, no mix,
    no fixed), then outer -- of degree 1, e.g. ``linear`` or ``carriers`` -- distributes p_j(v_j) over the operators:
    c_i = F_i + sum_j M_ij X_ij p_j(v_j)."""
    k = inner.n_pulses
    diagonal = inner.n_terms == k and inner.mix is None and inner.fixed is None and \
        not np.any(inner.alpha[~np.eye(k, dtype=bool)] != 0.0)
    if not diagonal:
        raise ValueError('control_map.compose: the inner map must give every line its own polynomial and nothing else (polynomial of a (k, D) array)')
    if outer.degree != 1:
        raise ValueError('control_map.compose: the outer map must be of degree 1 (linear, carriers), got degree %d' % outer.degree)
    if outer.n_pulses != k:
        raise ValueError('control_map.compose: the outer map takes %d pulses, the inner one delivers %d' % (outer.n_pulses, k))
    alpha = outer.alpha[:, :, 0][:, :, None] * inner.alpha[np.arange(k), np.arange(k)][None, :, :]
    return ControlMap(alpha, mix=outer.mix, fixed=outer.fixed)


def combine(*maps):
    """The sum of maps over the same r operators and k pulses: c = c_1 + c_2 + ...  A pair (i, j) that two maps both feed must carry the same mix
    in both (their polynomials add); otherwise the sum is not of the model's form (ValueError)."""
    if not maps:
        raise ValueError('control_map.combine: nothing to combine')
    r, k = maps[0].n_terms, _common_pulses(maps, 'combine')
    for m in maps:
        if m.n_terms != r:
            raise ValueError('control_map.combine: maps of %d and %d operators (stack maps that feed different operators)' % (r, m.n_terms))
    steps = _common_steps(maps, 'combine')
    D = max(m.degree for m in maps)
    alpha = np.zeros((r, k, D))
    mix = None if steps is None or all(m.mix is None for m in maps) else np.ones((r, k, steps))
    fed = np.zeros((r, k), dtype=bool)
    Fsum = None
    for m in maps:
        a = _padded(m.alpha, k, D)
        feeds = np.any(a != 0.0, axis=2)
        if mix is not None:
            mm = _full_mix(m, k, steps)
            clash = fed & feeds & np.any(mm != mix, axis=2)
            if np.any(clash):
                i, j = np.argwhere(clash)[0]
                raise ValueError('control_map.combine: pulse %d reaches operator %d through two different mixes; the sum is not of the form '
                                 'M p(v)' % (j, i))
            new = feeds & ~fed
            mix[new] = mm[new]
        alpha += a
        fed |= feeds
        if m.fixed is not None:
            Fsum = m.fixed.copy() if Fsum is None else Fsum + m.fixed
    return ControlMap(alpha, mix=mix, fixed=Fsum)


def stack(*maps):
    """Maps of the same k pulses that feed different operators, one below the other: r = sum of their r (the operators in the same order)."""
    if not maps:
        raise ValueError('control_map.stack: nothing to stack')
    k = _common_pulses(maps, 'stack')
    steps = _common_steps(maps, 'stack')
    D = max(m.degree for m in maps)
    alpha = np.concatenate([_padded(m.alpha, k, D) for m in maps], axis=0)
    mix = None if steps is None or all(m.mix is None for m in maps) else np.concatenate([_full_mix(m, k, steps) for m in maps], axis=0)
    Fs = None
    if any(m.fixed is not None for m in maps):
        Fs = np.concatenate([np.zeros((m.n_terms, steps)) if m.fixed is None else m.fixed for m in maps], axis=0)
    return ControlMap(alpha, mix=mix, fixed=Fs)


# ---- checks -----------------------------------------------------------------------------------------------------------------------------------

def validate(cm, k=None, r=None, steps=None):
    """Checks a map (a ControlMap, or a dict with keys alpha, mix, fixed) against k pulses, r operators and `steps` time slices (None: not
    checked) and returns it with C-contiguous float64 arrays.  Raises ValueError."""
    if isinstance(cm, dict):
        unknown = set(cm) - {'alpha', 'mix', 'fixed'}
        if unknown:
            raise ValueError('control_map: unknown keys %s' % sorted(unknown))
        if 'alpha' not in cm:
            raise ValueError('control_map: alpha (r x k x D) is required')
        cm = ControlMap(cm['alpha'], cm.get('mix'), cm.get('fixed'))
    if not isinstance(cm, ControlMap):
        raise ValueError('control_map: a helper_functions.control_map.ControlMap (or a dict with keys alpha, mix, fixed), got %s' % type(cm).__name__)
    a = cm.alpha
    if a.ndim != 3 or 0 in a.shape:
        raise ValueError('control_map: alpha has shape %s, expected (r, k, D)' % (a.shape,))
    rr, kk, D = a.shape
    if rr > MAX_TERMS:
        raise ValueError('control_map: %d operators, at most %d' % (rr, MAX_TERMS))
    if D > MAX_DEGREE:
        raise ValueError('control_map: degree %d, at most %d' % (D, MAX_DEGREE))
    if k is not None and kk != int(k):
        raise ValueError('control_map: the map takes %d pulses, the problem has %d (Hnames, maxA)' % (kk, int(k)))
    if r is not None and rr != int(r):
        raise ValueError('control_map: the map feeds %d operators, the problem has %d (Hops)' % (rr, int(r)))
    if cm.mix is not None and (cm.mix.ndim != 3 or cm.mix.shape[:2] != (rr, kk) or (steps is not None and cm.mix.shape[2] != int(steps))):
        raise ValueError('control_map: mix has shape %s, expected (%d, %d, %s)' % (cm.mix.shape, rr, kk, 'steps' if steps is None else int(steps)))
    if cm.fixed is not None and (cm.fixed.ndim != 2 or cm.fixed.shape[0] != rr or (steps is not None and cm.fixed.shape[1] != int(steps))):
        raise ValueError('control_map: fixed has shape %s, expected (%d, %s)' % (cm.fixed.shape, rr, 'steps' if steps is None else int(steps)))
    if cm.mix is not None and cm.fixed is not None and cm.mix.shape[2] != cm.fixed.shape[1]:
        raise ValueError('control_map: mix has %d time slices, fixed %d' % (cm.mix.shape[2], cm.fixed.shape[1]))
    for name, arr in (('alpha', a), ('mix', cm.mix), ('fixed', cm.fixed)):
        if arr is not None and not np.all(np.isfinite(arr)):
            raise ValueError('control_map: %s has a non-finite entry' % name)
    reach = np.any(a != 0.0, axis=2)
    if cm.mix is not None:
        reach = reach & np.any(cm.mix != 0.0, axis=2)
    for j in range(kk):
        if not np.any(reach[:, j]):
            raise ValueError('control_map: pulse %d reaches no operator (alpha[i, %d] or mix[i, %d] is zero for every i)' % (j, j, j))
    out = ControlMap(np.ascontiguousarray(a), None if cm.mix is None else np.ascontiguousarray(cm.mix),
                     None if cm.fixed is None else np.ascontiguousarray(cm.fixed))
    out.coefficients = cm.coefficients
    return out


# ---- the formula ------------------------------------------------------------------------------------------------------------------------------

def _powers(v, D):
    """v^1 .. v^D, (D, k, steps)."""
    return np.stack([v ** d for d in range(1, D + 1)])


def apply(cm, v):
    """c (r x steps) of the pulses v (k x steps)."""
    v = np.asarray(v, dtype=np.float64)
    p = np.einsum('ijd,djt->ijt', cm.alpha, _powers(v, cm.degree))
    if cm.mix is not None:
        p = cm.mix * p
    c = np.sum(p, axis=1)
    return c if cm.fixed is None else cm.fixed + c


def jacobian(cm, v):
    """dc_i[t] / dv_j[t], (r, k, steps): M[i, j, t] p_ij'(v_j[t])."""
    v = np.asarray(v, dtype=np.float64)
    D = cm.degree
    dp = np.stack([d * v ** (d - 1) for d in range(1, D + 1)])
    J = np.einsum('ijd,djt->ijt', cm.alpha, dp)
    return J if cm.mix is None else cm.mix * J


def pullback(cm, v, dJ_dc):
    """dJ/dv (k x steps) from dJ/dc (r x steps): sum_i dJ/dc_i[t] M[i, j, t] p_ij'(v_j[t])."""
    return np.einsum('it,ijt->jt', np.asarray(dJ_dc, dtype=np.float64), jacobian(cm, v))


def coefficient_bounds(cm, pulse_bound):
    """cmax_i = max_t |F_i| + sum_j max_t |M_ij| sum_d |alpha_ijd| bound_j^d: what |c_i| cannot exceed while |v_j| <= bound_j."""
    b = np.asarray(pulse_bound, dtype=np.float64).reshape(-1)
    pw = np.stack([b ** d for d in range(1, cm.degree + 1)], axis=1)             # (k, D)
    per = np.einsum('ijd,jd->ij', np.abs(cm.alpha), pw)
    if cm.mix is not None:
        per = per * np.max(np.abs(cm.mix), axis=2)
    out = np.sum(per, axis=1)
    return out if cm.fixed is None else out + np.max(np.abs(cm.fixed), axis=1)


def choose_taylor(cm, H0, Hops, robust, maxA, U0, total_time, steps, unitary_error, state_transfer, no_scaling):
    """(Taylor terms, squarings) of a mapped problem: SystemParameters' chooser on (H0, Hops, cmax) with the coefficient bounds in the place of
    maxA -- the pulse bound of line j is maxA_j times the member's amplitude scale -- and, for an ensemble, the maximum over its members as
    robust.choose_taylor takes it (each with its own drift)."""
    from quantum_optimal_control.core.system_parameters import N_CANDIDATES, SystemParameters
    maxA = np.asarray(maxA, dtype=np.float64)
    members = 1 if robust is None else robust['weights'].shape[0]
    best_t, best_s = 0, 0
    for e in range(members):
        H0e = np.asarray(H0, dtype=np.complex128)
        scale = np.ones_like(maxA)
        if robust is not None:
            for qq, p in enumerate(robust['operators']):
                H0e = H0e + robust['offsets'][e, qq] * p
            scale = np.abs(robust['amp_scales'][e])
        ch = SystemParameters.__new__(SystemParameters)      # the chooser alone: no initial guess is drawn
        ch.H0_c, ch.ops_c, ch.ops_max_amp, ch.U0_c = H0e, Hops, coefficient_bounds(cm, scale * maxA), U0
        ch.dt, ch.steps, ch.state_num = float(total_time) / steps, steps, len(H0e)
        ch.Unitary_error, ch.state_transfer, ch.no_scaling = unitary_error, state_transfer, no_scaling
        exps, scalings = [], []
        for d in range(1 if (state_transfer or no_scaling) else N_CANDIDATES):
            exps.append(ch.Choose_exp_terms(d))
            scalings.append(ch.scaling)
        i = int(np.argmin(np.add(exps, scalings)))
        best_t, best_s = max(best_t, int(exps[i])), max(best_s, int(scalings[i]))
    return best_t, best_s
