"""Open-system GRAPE: collapse operators for Grape(collapse_ops=...) / HipEngine(collapse_ops=...) and the Taylor rule of the Lindblad slice map.

A collapse operator C_j is n x n and carries the square root of its rate, so that the master equation reads
    d rho / dt = -i [H, rho] + sum_j (C_j rho C_j^dagger - 1/2 {C_j^dagger C_j, rho}).
The reference has no counterpart (it propagates state vectors only).
"""
import math

import numpy as np


def validate(collapse_ops, n):
    """The list as the engine takes it: complex n x n arrays.  ValueError on anything else (an empty list is the closed limit)."""
    if not isinstance(collapse_ops, (list, tuple)):
        raise ValueError('collapse_ops: a list of %d x %d collapse operators is expected, got %s' % (n, n, type(collapse_ops).__name__))
    out = []
    for j, op in enumerate(collapse_ops):
        a = np.asarray(op)
        if a.shape != (n, n):
            raise ValueError('collapse_ops[%d] has shape %s, expected (%d, %d)' % (j, a.shape, n, n))
        try:
            a = a.astype(np.complex128)
        except (TypeError, ValueError):
            raise ValueError('collapse_ops[%d] is not numeric' % j)
        if not np.all(np.isfinite(a)):
            raise ValueError('collapse_ops[%d] is not finite' % j)
        if not np.any(a):
            raise ValueError('collapse_ops[%d] is all zero (leave it out)' % j)
        out.append(np.ascontiguousarray(a))
    return out


# ---- where an open engine runs ------------------------------------------------------------------------------------------------------------------
PATH_LINDBLAD, PATH_LINDBLAD_TILED = 6, 8          # include/qoc.h QOC_PATH_LINDBLAD, QOC_PATH_LINDBLAD_TILED (hip_engine has the same numbers)
LDS_MAX_N, LDS_LIMIT, TILED_MAX_N = 32, 159 * 1024, 128


def choose_path(n, c):
    """The path of an open engine of n levels with c collapse operators: PATH_LINDBLAD (the operators of a pair in the LDS of one compute unit)
    wherever its size rule holds -- n <= 32 and (c + 4) n (n | 1) 16 bytes <= 159 KiB --, else PATH_LINDBLAD_TILED (global scratch, 16 x 16 tiles
    on the matrix pipe) up to n = 128.  ValueError above."""
    n, c = int(n), int(c)
    if n <= LDS_MAX_N and (c + 4) * n * (n | 1) * 16 <= LDS_LIMIT:
        return PATH_LINDBLAD
    if n <= TILED_MAX_N:
        return PATH_LINDBLAD_TILED
    raise ValueError('open-system GRAPE: n = %d levels; PATH_LINDBLAD holds up to %d levels within %d bytes of LDS, PATH_LINDBLAD_TILED up to %d levels'
                     % (n, LDS_MAX_N, LDS_LIMIT, TILED_MAX_N))


def _lowering(n):
    return np.diag(np.sqrt(np.arange(1, n)), 1).astype(np.complex128)


def relaxation(n, t1):
    """Energy relaxation of an n-level oscillator with lifetime t1: sqrt(1 / t1) a."""
    if not (t1 > 0 and np.isfinite(t1)):
        raise ValueError('relaxation: t1 = %r (a positive time)' % (t1,))
    return math.sqrt(1.0 / float(t1)) * _lowering(n)


def dephasing(n, tphi):
    """Pure dephasing of an n-level oscillator with dephasing time tphi: sqrt(2 / tphi) a^dagger a."""
    if not (tphi > 0 and np.isfinite(tphi)):
        raise ValueError('dephasing: tphi = %r (a positive time)' % (tphi,))
    a = _lowering(n)
    return math.sqrt(2.0 / float(tphi)) * (a.conj().T @ a)


# ---- running costs: penalties on expectation values along the pulse (Grape(running_costs=...) / HipEngine(running_costs=...)) ------------------
# A cost is one record (O, coeff, power): with x_i(tau) = Re Tr(O rho_ii(tau)) of every state of interest i at every slice boundary tau = 0 .. steps
# it adds (coeff / steps) sum_tau sum_i x_i(tau)^power / power to the objective.

MAX_COSTS = 16


def observable_cost(O, coeff, power=2):
    """A penalty on the expectation value of the Hermitian observable O (n x n)."""
    return (np.array(O, dtype=np.complex128), float(coeff), int(power))


def level_cost(n, level, coeff, power=2):
    """A penalty on the population of one bare level: O = |level><level| (power 2: the closed engines' forbidden level)."""
    return subspace_cost(n, [level], coeff, power)


def subspace_cost(n, levels, coeff, power=2):
    """A penalty on the population of a set of bare levels, e.g. everything outside the computational subspace: O = the projector on them."""
    O = np.zeros((n, n), dtype=np.complex128)
    for l in levels:
        if not 0 <= int(l) < n:
            raise ValueError('subspace_cost: level %r is outside 0 .. %d' % (l, n - 1))
        O[int(l), int(l)] = 1.0
    return observable_cost(O, coeff, power)


def dressed_level_cost(v, coeff, power=2):
    """A penalty on the population of the (dressed) state v: O = v v^dagger."""
    v = np.asarray(v, dtype=np.complex128).reshape(-1)
    return observable_cost(np.outer(v, np.conj(v)), coeff, power)


def validate_costs(costs, n):
    """The list as the engine takes it: records (O complex n x n, coeff, power).  ValueError on a wrong shape, an observable that is not Hermitian within
    1e-12 max|O|, a coefficient that is not finite, a power other than 1 or 2, or more than 16 costs (an empty list is no cost)."""
    if not isinstance(costs, (list, tuple)):
        raise ValueError('running_costs: a list of (O, coeff, power) records is expected, got %s' % type(costs).__name__)
    if len(costs) > MAX_COSTS:
        raise ValueError('running_costs: %d costs, at most %d' % (len(costs), MAX_COSTS))
    out = []
    for j, rec in enumerate(costs):
        if not isinstance(rec, (list, tuple)) or len(rec) != 3:
            raise ValueError('running_costs[%d]: a record (O, coeff, power) is expected (open_system.level_cost and its kin build them)' % j)
        O, coeff, power = rec
        a = np.asarray(O)
        if a.shape != (n, n):
            raise ValueError('running_costs[%d]: the observable has shape %s, expected (%d, %d)' % (j, a.shape, n, n))
        try:
            a = np.ascontiguousarray(a.astype(np.complex128))
            coeff = float(coeff)
        except (TypeError, ValueError):
            raise ValueError('running_costs[%d] is not numeric' % j)
        if not np.all(np.isfinite(a)):
            raise ValueError('running_costs[%d]: the observable is not finite' % j)
        if np.max(np.abs(a - a.conj().T)) > 1e-12 * np.max(np.abs(a)):
            raise ValueError('running_costs[%d]: the observable is not Hermitian' % j)
        if not np.isfinite(coeff):
            raise ValueError('running_costs[%d]: the coefficient is not finite' % j)
        if isinstance(power, bool) or power not in (1, 2):
            raise ValueError('running_costs[%d]: power = %r (1 or 2)' % (j, power))
        out.append((a, coeff, int(power)))
    return out


def lindblad_bound(H0, Hops, maxA, collapse_ops, dt):
    """x = 2 dt (|H0|_2 + sum_k maxA_k |H_k|_2 + sum_j |C_j|_2^2) >= |dt L| for every admissible pulse."""
    x = np.linalg.norm(np.asarray(H0, dtype=np.complex128), 2)
    for a, h in zip(np.asarray(maxA, dtype=np.float64), Hops):
        x += abs(float(a)) * np.linalg.norm(np.asarray(h, dtype=np.complex128), 2)
    for c in collapse_ops:
        x += np.linalg.norm(np.asarray(c, dtype=np.complex128), 2) ** 2
    return 2.0 * float(dt) * float(x)


def taylor_remainder(y, T, steps, s):
    """steps 2^s 2 y^(T+1) / (T+1)!: the Taylor remainder with e^y <= 2, summed over all sub-steps of a contractive map."""
    return steps * (2.0 ** s) * 2.0 * y ** (T + 1) / math.factorial(T + 1)


def choose_taylor(H0, Hops, maxA, collapse_ops, dt, steps, unitary_error):
    """(T, s) of the Lindblad slice map (degree T, 2^s sub-steps): s the smallest value with y = x / 2^s <= 0.5, T the smallest value >= 2 with
    taylor_remainder(y, T, steps, s) <= unitary_error.  ValueError past T = 60 or s = 12 (the engine's limits)."""
    x = lindblad_bound(H0, Hops, maxA, collapse_ops, dt)
    s = 0
    while x / 2.0 ** s > 0.5:
        s += 1
        if s > 12:
            raise ValueError('choose_taylor: |dt L| <= %.3g needs more than 2^12 sub-steps per slice; use more time slices' % x)
    y = x / 2.0 ** s
    T = 2
    while taylor_remainder(y, T, steps, s) > unitary_error:
        T += 1
        if T > 60:
            raise ValueError('choose_taylor: unitary_error = %g is not reached with 60 Taylor terms' % unitary_error)
    return T, s


def choose_taylor_members(H0, Hops, maxA, devices, dt, steps, unitary_error, control_map=None):
    """(T, s) for an ensemble or fleet with decay: the maximum over the members of choose_taylor on each member's Hamiltonians and scaled collapse
    operators.  devices: the validated robust dicts (helper_functions/robust.py), one per device -- one dict for a plain ensemble.  control_map: Hops
    are then the operators the map feeds, bounded by the largest coefficients it can deliver from the member's scaled pulses."""
    from quantum_optimal_control.helper_functions import robust as _robust
    best_t, best_s = 0, 0
    for dev in devices:
        for e in range(dev['weights'].shape[0]):
            if control_map is None:
                H0e, Hopse = _robust.member_hamiltonians(H0, Hops, dev, e)
                bound = maxA
            else:
                from quantum_optimal_control.helper_functions.control_map import coefficient_bounds
                H0e, _ = _robust.member_hamiltonians(H0, [], dev, e)
                Hopse, bound = Hops, coefficient_bounds(control_map, np.abs(dev['amp_scales'][e]) * np.asarray(maxA, dtype=np.float64))
            t, s = choose_taylor(H0e, Hopse, bound, _robust.member_collapse_ops(dev, e), dt, steps, unitary_error)
            best_t, best_s = max(best_t, t), max(best_s, s)
    return best_t, best_s
