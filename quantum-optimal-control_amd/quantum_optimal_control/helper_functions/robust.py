"""Robust GRAPE: ensembles of perturbed Hamiltonians for ``Grape(..., robust=...)``.

Member e of an ensemble is an ordinary GRAPE problem with the drift H0 + sum_q offsets[e, q] P_q and the control Hamiltonians
amp_scales[e, j] H_j; all members share U0, the targets, the states of interest, maxA, the regularisers and the one trainable pulse.
Grape optimises the weighted mean objective over the members (include/qoc.h, qoc_create_ensemble), or, with a `risk` beta > 0, their soft
worst case  max_e c_e + log1p(sum_e w_e expm1(beta (c_e - max_e c_e))) / beta  (qoc_set_risk): the mean at beta = 0, the worst member as beta grows.

Decay per member: with the optional keys `collapse_ops` (c operators as Grape(collapse_ops=...) takes them) and `rate_scales` (E, c) a member is
an OPEN problem: member e decays through sqrt(rate_scales[e, j]) C_j (a scale of 0 switches the channel off; default ones), and Grape scores and
optimises the pulse under every member's master equation (include/qoc.h, qoc_create_open_fleet).

Noise traces: with the optional key `traces` (E, q, steps) the perturbation of a member is no longer constant over the pulse: at slice t member e
has the drift H0 + sum_q (offsets[e, q] + traces[e, q, t]) P_q -- sampled noise trajectories, e.g. from helper_functions.noise -- and the pulse is
optimised for the sample average (or soft worst case) over them (include/qoc.h, qoc_set_traces).
"""
import itertools

import numpy as np


def _rows(values, width, name):
    """values as a 2-D float array of `width` columns; a scalar row applies to all columns."""
    out = []
    for row in values:
        r = np.asarray(row, dtype=np.float64)
        if r.ndim == 0:
            r = np.full(width, float(r))
        r = r.reshape(-1)
        if r.shape != (width,):
            raise ValueError('%s: a row has %d entries, expected %d' % (name, r.shape[0], width))
        out.append(r)
    return np.array(out, dtype=np.float64).reshape(len(out), width)


def _is_sparse(op):
    """A scipy.sparse matrix (duck-typed, so that dense-only callers never import scipy)."""
    return hasattr(op, 'tocsr') and hasattr(op, 'nnz')


def as_operator(op):
    """A perturbation operator as it was given: a scipy.sparse matrix stays one (np.asarray would wrap it in a 0-d object array), anything else
    becomes an array."""
    return op if _is_sparse(op) else np.asarray(op)


def same_operator(a, b):
    """Entry-for-entry equality of two operators, either of which may be scipy.sparse; a sparse one is never densified."""
    if _is_sparse(a) or _is_sparse(b):
        import scipy.sparse as sps
        a, b = sps.csr_matrix(a), sps.csr_matrix(b)
        return a.shape == b.shape and (a != b).nnz == 0
    return np.array_equal(a, b)


def _validated_operators(operators, n, sparse):
    """The perturbation operators for the route at hand, checked square, n x n and Hermitian: complex CSR on the sparse route (sparse=True: a dense
    one is converted, a sparse one is never densified), complex arrays on a dense route (sparse=False: a sparse one is densified); sparse=None (the
    builders, which know no route yet): every operator in the kind it was given as.  Returns (operators, n)."""
    ops = []
    kind = sparse
    for i, p in enumerate(operators):
        sparse = _is_sparse(p) if kind is None else kind
        if sparse:
            import scipy.sparse as sps
            p = sps.csr_matrix(p, dtype=np.complex128)
        else:
            p = np.asarray(p.toarray() if _is_sparse(p) else p, dtype=np.complex128)
        if p.ndim != 2 or p.shape[0] != p.shape[1] or (n is not None and p.shape[0] != n):
            raise ValueError('robust: operator %d has shape %s, expected %s' % (i, p.shape, (n, n) if n is not None else 'square'))
        if n is None:
            n = p.shape[0]
        if sparse:
            top = float(np.max(np.abs(p.data))) if p.nnz else 0.0
            diff = (p - p.conj().T).tocsr()
            if diff.nnz and float(np.max(np.abs(diff.data))) > 1e-12 * max(1.0, top):
                raise ValueError('robust: operator %d is not Hermitian' % i)
        elif not np.allclose(p, p.conj().T, rtol=0.0, atol=1e-12 * max(1.0, float(np.max(np.abs(p))))):
            raise ValueError('robust: operator %d is not Hermitian' % i)
        ops.append(p)
    return ops, n


def has_decay(robust):
    """True when the ensemble dict makes its members open problems (the key collapse_ops is given, an empty list included)."""
    return isinstance(robust, dict) and robust.get('collapse_ops') is not None


def ensemble_grid(operators=(), offsets=None, amp_scales=None, k=None, weights=None, risk=0.0, collapse_ops=None, rate_scales=None):
    """Cartesian product of offset rows (each q values, one per operator) and amplitude-scale rows (each k values, or a scalar for
    all k controls).  The nominal point (all offsets 0, all scales 1) comes first when the grid contains it; otherwise the
    product order is kept (offset rows outer).  weights: one per grid point (default uniform), normalised to sum 1.  risk: beta >= 0 of the
    soft worst-case objective (0: the weighted mean).
    collapse_ops, rate_scales: the members are open problems; the rate-scale rows (each c values, or a scalar for all c operators) are a third
    axis of the product (innermost), and the nominal point has all rate scales 1 as well.
    Returns the dict Grape(robust=...) takes."""
    operators = [as_operator(p) for p in operators]
    q = len(operators)
    if k is None:
        raise ValueError('ensemble_grid: k (the number of control Hamiltonians) is required')
    k = int(k)
    off_rows = _rows(offsets if offsets is not None else [np.zeros(q)], q, 'offsets') if q else np.zeros((1, 0))
    if q == 0 and offsets is not None and np.size(offsets) != 0:
        raise ValueError('ensemble_grid: offsets given without operators')
    amp_rows = _rows(amp_scales if amp_scales is not None else [1.0], k, 'amp_scales')
    if rate_scales is not None and collapse_ops is None:
        raise ValueError('ensemble_grid: rate_scales given without collapse_ops')
    c = 0 if collapse_ops is None else len(collapse_ops)
    rate_rows = _rows(rate_scales if rate_scales is not None else [1.0], c, 'rate_scales') if c else np.ones((1, 0))
    if c == 0 and rate_scales is not None and np.size(rate_scales) != 0:
        raise ValueError('ensemble_grid: rate_scales given without a collapse operator')
    pts = [(o, a, r) for o, a, r in itertools.product(off_rows, amp_rows, rate_rows)]
    if weights is None:
        w = np.ones(len(pts))
    else:
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
        if w.shape[0] != len(pts):
            raise ValueError('ensemble_grid: %d weights for %d grid points' % (w.shape[0], len(pts)))
    nominal = [i for i, (o, a, r) in enumerate(pts) if np.all(o == 0.0) and np.all(a == 1.0) and np.all(r == 1.0)]
    order = list(range(len(pts)))
    if nominal:
        order = [nominal[0]] + [i for i in order if i != nominal[0]]
    ens = dict(operators=operators, offsets=np.array([pts[i][0] for i in order]).reshape(len(pts), q),
               amp_scales=np.array([pts[i][1] for i in order]).reshape(len(pts), k), weights=w[order], risk=risk)
    if collapse_ops is not None:
        ens['collapse_ops'] = list(collapse_ops)
        ens['rate_scales'] = np.array([pts[i][2] for i in order]).reshape(len(pts), c)
    return validate(ens, None, k, sparse=None)          # (the operators stay as given: the route's own validate call makes them sparse or dense)


def validate(robust, n, k, sparse=False, steps=None):
    """Checks a robust dict (keys operators, offsets, amp_scales, weights, risk) against a problem of n levels (None: from the operators) and
    k controls and returns it normalised: operators a list of q complex n x n Hermitian matrices, offsets (E, q), amp_scales (E, k)
    (default ones), weights (E,) summing to 1 (default uniform), risk a finite float >= 0 (default 0.0: the weighted mean).  With the key
    collapse_ops the result also holds collapse_ops (c complex n x n matrices, open_system.validate's rules) and rate_scales (E, c), finite and
    >= 0 (default ones); without it the result has exactly the five keys above.  Raises ValueError.
    sparse=True (the sparse state-transfer route): the operators come back as complex CSR matrices -- a scipy.sparse operator is never densified,
    a dense one is converted once -- and the decay keys are refused; sparse=False densifies scipy.sparse operators; sparse=None (ensemble_grid and
    the fleet builders, before any route is known) leaves every operator in the kind it was given as and refuses nothing.
    With the key traces the result also holds traces (E, q, steps), finite, q >= 1, checked against the other rows and -- steps given -- against the
    number of slices; the key is allowed with sparse=True and with decay.  Without it the result has no such key."""
    if not isinstance(robust, dict):
        raise ValueError('robust: a dict with keys operators, offsets, amp_scales, weights, risk')
    unknown = set(robust) - {'operators', 'offsets', 'amp_scales', 'weights', 'risk', 'collapse_ops', 'rate_scales', 'traces'}
    if unknown:
        raise ValueError('robust: unknown keys %s' % sorted(unknown))
    try:
        risk = float(robust.get('risk', 0.0))
    except (TypeError, ValueError):
        raise ValueError('robust: risk must be a number >= 0, got %r' % (robust.get('risk'),))
    if not (np.isfinite(risk) and risk >= 0):
        raise ValueError('robust: risk must be finite and >= 0, got %r' % risk)
    ops, n = _validated_operators(robust.get('operators', []), n, sparse)
    q = len(ops)
    cops, rates = robust.get('collapse_ops'), robust.get('rate_scales')
    if sparse is True and (cops is not None or rates is not None):
        raise ValueError('robust: decay per member (%s) is not available on scipy.sparse Hamiltonians (sparse state transfer)'
                         % ('collapse_ops' if cops is not None else 'rate_scales'))
    if rates is not None and cops is None:
        raise ValueError('robust: rate_scales given without collapse_ops')
    if cops is not None:
        from quantum_optimal_control.helper_functions import open_system
        if n is None:
            if not isinstance(cops, (list, tuple)) or (len(cops) and np.ndim(cops[0]) != 2):
                raise ValueError('robust: collapse_ops is a list of n x n collapse operators')
            n_c = np.shape(cops[0])[0] if len(cops) else None
        else:
            n_c = n
        try:
            cops = open_system.validate(cops, n_c) if n_c is not None else []
        except ValueError as err:
            raise ValueError('robust: %s' % err)
    E = None if rates is None else np.shape(rates)[0] if np.ndim(rates) == 2 else None
    offsets = robust.get('offsets')
    if q:
        if offsets is None:
            raise ValueError('robust: offsets (E x q) are required with operators')
        offsets = np.asarray(offsets, dtype=np.float64)
        if offsets.ndim != 2 or offsets.shape[1] != q:
            raise ValueError('robust: offsets have shape %s, expected (E, %d)' % (offsets.shape, q))
        E = offsets.shape[0]
    elif offsets is not None and np.size(offsets) != 0:
        offsets = np.asarray(offsets, dtype=np.float64)
        if offsets.ndim != 2 or offsets.shape[1] != 0:
            raise ValueError('robust: offsets given without operators')
        E = offsets.shape[0]
    traces = robust.get('traces')
    if traces is not None:
        traces = np.asarray(traces, dtype=np.float64)
        if q < 1:
            raise ValueError('robust: traces given without operators (a trace is added to a perturbation row: q >= 1)')
        if traces.ndim != 3 or traces.shape[0] != E or traces.shape[1] != q or traces.shape[2] < 1:
            raise ValueError('robust: traces have shape %s, expected (%d, %d, steps)' % (traces.shape, E, q))
        if steps is not None and traces.shape[2] != int(steps):
            raise ValueError('robust: traces have %d slices, the pulse has %d' % (traces.shape[2], int(steps)))
        if not np.all(np.isfinite(traces)):
            raise ValueError('robust: traces must be finite')
    amp = robust.get('amp_scales')
    if amp is not None:
        amp = np.asarray(amp, dtype=np.float64)
        if amp.ndim != 2 or amp.shape[1] != k or (E is not None and amp.shape[0] != E):
            raise ValueError('robust: amp_scales have shape %s, expected (%s, %d)' % (amp.shape, 'E' if E is None else E, k))
        E = amp.shape[0]
    w = robust.get('weights')
    if w is not None:
        w = np.asarray(w, dtype=np.float64).reshape(-1)
        if E is not None and w.shape[0] != E:
            raise ValueError('robust: %d weights for %d members' % (w.shape[0], E))
        E = w.shape[0]
    if E is None or E < 1:
        raise ValueError('robust: the ensemble has no members')
    if amp is None:
        amp = np.ones((E, k))
    if w is None:
        w = np.ones(E)
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError('robust: weights must be finite and >= 0')
    if not w.sum() > 0:
        raise ValueError('robust: the weights sum to zero')
    if not (np.all(np.isfinite(amp)) and (offsets is None or np.all(np.isfinite(offsets)))):
        raise ValueError('robust: offsets and amp_scales must be finite')
    out = dict(operators=ops, offsets=np.zeros((E, 0)) if offsets is None else offsets.reshape(E, q), amp_scales=amp,
               weights=w / w.sum(), risk=risk)
    if cops is not None:
        c = len(cops)
        rates = np.ones((E, c)) if rates is None else np.asarray(rates, dtype=np.float64)
        if rates.shape != (E, c):
            raise ValueError('robust: rate_scales have shape %s, expected (%d, %d)' % (rates.shape, E, c))
        if not np.all(np.isfinite(rates)) or np.any(rates < 0):
            raise ValueError('robust: rate_scales must be finite and >= 0')
        out['collapse_ops'], out['rate_scales'] = cops, rates
    if traces is not None:
        out['traces'] = traces
    return out


def taylor_view(robust):
    """The ensemble as the Taylor choosers see it.  Without traces: the dict itself.  With traces: a copy without them whose offsets are, per member
    and operator, the value of offsets[e, q] + traces[e, q, t] of largest magnitude over t -- the largest perturbation any slice of that member
    runs."""
    if not isinstance(robust, dict) or robust.get('traces') is None:
        return robust
    v = np.asarray(robust['offsets'], dtype=np.float64)[:, :, None] + np.asarray(robust['traces'], dtype=np.float64)
    t = np.argmax(np.abs(v), axis=2)
    out = {key: val for key, val in robust.items() if key != 'traces'}
    out['offsets'] = np.take_along_axis(v, t[:, :, None], axis=2)[:, :, 0]
    return out


def member_hamiltonians(H0, Hops, robust, e):
    """(H0_e, [H_j,e]) of member e: the drift with its perturbations, the controls with their amplitude scales."""
    H0e = np.asarray(H0, dtype=np.complex128).copy()
    for qq, p in enumerate(robust['operators']):
        H0e = H0e + robust['offsets'][e, qq] * p
    return H0e, [robust['amp_scales'][e, j] * np.asarray(h) for j, h in enumerate(Hops)]


def member_collapse_ops(robust, e):
    """The collapse operators of member e: sqrt(rate_scales[e, j]) C_j, switched-off channels (scale 0) left out.  [] without decay."""
    if not has_decay(robust):
        return []
    return [np.sqrt(s) * np.asarray(cj, dtype=np.complex128) for s, cj in zip(robust['rate_scales'][e], robust['collapse_ops']) if s > 0]


def choose_taylor(H0, Hops, robust, maxA, U0, total_time, steps, unitary_error, state_transfer, no_scaling):
    """(Taylor terms, squarings): the maximum over members of what SystemParameters' chooser picks for each member's problem.  With traces a
    member's problem uses, per operator, the value of offsets + traces[t] of largest magnitude over t (taylor_view)."""
    from quantum_optimal_control.core.system_parameters import N_CANDIDATES, SystemParameters
    robust = taylor_view(robust)
    best_t, best_s = 0, 0
    for e in range(robust['weights'].shape[0]):
        H0e, Hopse = member_hamiltonians(H0, Hops, robust, e)
        ch = SystemParameters.__new__(SystemParameters)      # the chooser alone: no initial guess is drawn
        ch.H0_c, ch.ops_c, ch.ops_max_amp, ch.U0_c = H0e, Hopse, maxA, U0
        ch.dt, ch.steps, ch.state_num = float(total_time) / steps, steps, len(H0e)
        ch.Unitary_error, ch.state_transfer, ch.no_scaling = unitary_error, state_transfer, no_scaling
        exps, scalings = [], []
        for d in range(1 if (state_transfer or no_scaling) else N_CANDIDATES):
            exps.append(ch.Choose_exp_terms(d))
            scalings.append(ch.scaling)
        i = int(np.argmin(np.add(exps, scalings)))
        best_t, best_s = max(best_t, int(exps[i])), max(best_s, int(scalings[i]))
    return best_t, best_s
