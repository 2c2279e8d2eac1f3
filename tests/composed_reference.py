"""What every composed reference shares (TEST INFRASTRUCTURE ONLY): the combination of member trajectories into a control set's expected values
at the level of the Hamiltonian's COEFFICIENTS, once.

    x --sin--> w --(the line T)--> wf --maxA--> u --(amp_scales[e])--> v_e --(the map)--> c_e --run(e, c_e)--> one trajectory per member
    the weighted mean of the members, or its tilt (soft_worst_case)  -->  the map's pullback, a[e, j], T^T  -->  the pulse regularisers once on
    the group view (pulse_view)  -->  the chain rule cos(x)

`run` is the feature module's: the closed oracle or the exact gradient (tests/control_map_reference.py), the Lindblad reference
(tests/open_fleet_reference.py), the same with running costs (tests/running_cost_reference.py), the sparse reference
(tests/sparse_ensemble_reference.py), each at arcsin(c / S) (at_coefficients); tests/noise_reference.py appends a member's frozen rows inside its
run.  The ensemble composed from the members' OWN gradients (tests/robust_reference.py) is a separate statement, and the tests that compare the
two are the check of both.  Also here: the Adam loop with the device loop's semantics over any evaluation, and central differences."""
from types import SimpleNamespace

import numpy as np

from oracle import grape_oracle as go
from quantum_optimal_control.helper_functions import control_map as cmap

PULSE_KEYS = ('amplitude', 'envelope', 'dwdt', 'd2wdt2', 'bandpass', 'band')


def split_regs(rc):
    """(state regularisers, pulse regularisers) of a reg_coeffs dict."""
    return {key: v for key, v in rc.items() if key not in PULSE_KEYS}, {key: v for key, v in rc.items() if key in PULSE_KEYS}


def at_coefficients(coeff):
    """(S, base): the amplitude bounds S_i = 2 max_t |c_i| (1 for a zero row; arcsin stays far from its end points) and base = arcsin(c / S), at
    which a system with maxA = S runs the coefficients coeff (rows x steps) in place of a pulse."""
    S = 2.0 * np.max(np.abs(coeff), axis=1)
    S[S == 0.0] = 1.0
    return S, np.arcsin(coeff / S[:, None])


def pulse_view(k, Pn, total_time, pulse_rc):
    """What go.pulse_regularisers reads of a system, for k pulses of Pn samples over total_time; the envelope constant where it is asked for."""
    omg = None
    if 'envelope' in pulse_rc:
        grid = np.linspace(-2, 2, Pn)
        shape = np.ones(Pn) - np.exp(-np.power(grid, 2.) / 2.)
        omg = np.tile(shape * (shape > 0) + 0.01 * np.ones(Pn), (k, 1))
    return SimpleNamespace(reg_coeffs=pulse_rc, steps=Pn, dt=total_time / Pn, k=k, total_time=total_time, use_gpu=True, one_minus_gauss=omg)


def soft_worst_case(costs, w, beta):
    """(J, pi) of member costs and weights (include/qoc.h qoc_set_risk, DESIGN.md 6b'); beta = 0: the weighted sum and the weights themselves.

        x_e = beta (c_e - c_max)             c_max = max c_e over the members with w_e > 0
        S   = sum_e w_e expm1(x_e)           members in the order 0 .. E-1, as k_ens_tilt sums them
        J   = c_max + log1p(S) / beta        the soft worst case: mean <= J <= max when sum w = 1
        pi_e = w_e exp(x_e) / (1 + S)        dJ / dc_e"""
    c = np.asarray(costs, dtype=np.float64).reshape(-1)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if beta == 0:
        return float(np.dot(w, c)), w.copy()
    cmax = float(np.max(c[w > 0]))
    x = np.where(w > 0, beta * (c - cmax), 0.0)
    S = 0.0
    for e in range(len(c)):
        S = S + (w[e] * np.expm1(x[e]) if w[e] > 0 else 0.0)
    J = cmax + np.log1p(S) / beta
    pi = np.where(w > 0, w * np.exp(x) / (1.0 + S), 0.0)
    return float(J), pi


def combine(x, maxA, ens, total_time, pulse_rc, run, cm=None, T=None, beta=None, want_grad=True):
    """The control set's expected values at the variable x (k x steps, or k x P behind the line T (steps x P)) over the members of `ens` (a validated
    robust dict), from run(e, c): member e's trajectory at its coefficients c = apply(cm, v_e) (cm None: its pulses v_e themselves), a dict with loss,
    unitary_scale, reg_state (or reg_loss, of a system that carries the state regularisers only) and, with the gradient, dL_du = dJ/dc.  beta None:
    the ensemble's own risk.  Returns loss, reg_loss, reg_state, unitary_scale, member_loss, member_reg_state, weights (pi), pulse, uks,
    coefficients (member 0), members (what run returned) and, with the gradient, grad and grad_squared.  Under a risk beta > 0 the members' costs
    are c_e = loss_e + reg_state_e, reg_state = sum_e pi_e reg_state_e, loss = J - reg_state and reg_loss = J + the pulse regularisers."""
    maxA = np.asarray(maxA, dtype=np.float64)
    k = len(maxA)
    x = np.asarray(x, dtype=np.float64).reshape(k, -1)
    beta = float(ens.get('risk', 0.0)) if beta is None else float(beta)
    ws = np.sin(x)
    u = maxA[:, None] * (ws if T is None else ws @ T.T)
    w = np.asarray(ens['weights'], dtype=np.float64)
    E = len(w)
    vs = [ens['amp_scales'][e][:, None] * u for e in range(E)]
    cs = [v if cm is None else cmap.apply(cm, v) for v in vs]
    rs = [run(e, cs[e]) for e in range(E)]
    loss_e = np.array([r['loss'] for r in rs])
    state_e = np.array([r['reg_state'] if 'reg_state' in r else r['reg_loss'] - r['loss'] for r in rs])
    val, dR = go.pulse_regularisers(pulse_view(k, x.shape[1], total_time, pulse_rc), ws)
    if beta > 0 and E > 1:
        J, pi = soft_worst_case(loss_e + state_e, w, beta)
        reg_state = float(np.sum(pi * state_e))
        loss, reg_loss = J - reg_state, J + val
    else:
        pi, reg_state = w, float(np.sum(w * state_e))
        loss, reg_loss = float(np.sum(w * loss_e)), float(np.sum(w * (loss_e + state_e))) + val
    out = dict(loss=float(loss), reg_loss=float(reg_loss), reg_state=reg_state, unitary_scale=float(np.sum(w * np.array([r['unitary_scale'] for r in rs]))),
               member_loss=loss_e, member_reg_state=state_e, weights=pi, pulse=u, uks=maxA[:, None] * ws, coefficients=cs[0], members=rs)
    if not want_grad:
        return out
    back = (lambda v, g: g) if cm is None else (lambda v, g: cmap.pullback(cm, v, g))
    dJdu = sum(pi[e] * ens['amp_scales'][e][:, None] * back(vs[e], rs[e]['dL_du']) for e in range(E))
    grad = np.cos(x) * (maxA[:, None] * (dJdu if T is None else dJdu @ T) + dR)
    out.update(grad=grad, grad_squared=0.5 * float(np.sum(grad * grad)))
    return out


def run_adam(evaluate_at, x0, conv):
    """The device loop's semantics (oracle.grape_oracle.run_adam) over any evaluation x -> dict(loss, reg_loss, grad_squared, unitary_scale, grad):
    the stop rule reads the loss, the step follows `grad`.  dict(base, iterations, loss, reg_loss, last (the evaluation that ended the loop),
    history (one row (loss, reg_loss, grad_squared, unitary_scale) per evaluation))."""
    x = np.array(x0, dtype=np.float64)
    opt = go.Adam(x.shape)
    iterations, hist = 0, []
    while True:
        r = evaluate_at(x)
        hist.append((r['loss'], r['reg_loss'], r['grad_squared'], r['unitary_scale']))
        if r['loss'] < conv['conv_target'] or r['grad_squared'] < conv['min_grad'] or iterations >= conv['max_iterations']:
            return dict(base=x, iterations=iterations, loss=r['loss'], reg_loss=r['reg_loss'], last=r, history=np.array(hist))
        iterations += 1
        x = opt.step(x, r['grad'], float(conv['rate']) * np.exp(-float(iterations) / conv['learning_rate_decay']))


def central_differences(f, x, h=1e-6):
    g = np.zeros_like(x)
    for idx in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[idx] += h
        xm[idx] -= h
        g[idx] = (f(xp) - f(xm)) / (2 * h)
    return g
