"""NumPy reference of the open-system running costs (TEST INFRASTRUCTURE ONLY), written from the definition of DESIGN.md section 6l on top of
tests/lindblad_reference.py (generator, slice_map, propagate, loss_of), over all m^2 pairs:

    x_l,i(tau) = Re sum_ac conj(O_l[a][c]) rho_ii(tau)[a][c]
    R          = sum_l (a_l / steps) sum_{tau = 0 .. steps} sum_{i < m} x_l,i(tau)^p_l / p_l
    Lambda_ii(t+1) += sum_l (a_l / steps) x_l,i(t+1)^(p_l - 1) O_l      after rho_ii(t+1) is at hand, before the contraction of slice t

A cost is a record (O, a, p), as helper_functions/open_system.py builds them.  Also here: the Adam loop over this evaluation, and the composition of
members into a control set (the weighted mean, the soft worst case of include/qoc.h with the members' costs c_e = loss_e + R_e, the line, the map) as
tests/open_fleet_reference.py composes members without costs."""
from types import SimpleNamespace

import numpy as np

from oracle import grape_oracle as go
from quantum_optimal_control.helper_functions import control_map as cmap
from quantum_optimal_control.helper_functions import robust as rb
from tests import control_map_reference as ref
from tests import lindblad_reference as lr
from tests import open_fleet_reference as ofr


def expectations(costs, hist):
    """x[tau, l, i] of a history hist[tau, i, j] (steps + 1, m, m, n, n)."""
    m = hist.shape[1]
    x = np.empty((hist.shape[0], len(costs), m))
    for l, (O, _, _) in enumerate(costs):
        for i in range(m):
            x[:, l, i] = np.real(np.sum(np.conj(O)[None] * hist[:, i, i], axis=(1, 2)))
    return x


def cost_value(costs, x, steps):
    """R from the expectation values x[tau, l, i]."""
    return float(sum((a / steps) * np.sum(x[:, l, :] ** p) / p for l, (_, a, p) in enumerate(costs)))


def source(costs, x_tau, i, steps):
    """sum_l (a_l / steps) x_l,i^(p_l - 1) O_l for the expectation values x_tau[l, i] of one tau."""
    return sum((a / steps) * x_tau[l, i] ** (p - 1) * np.asarray(O, dtype=np.complex128) for l, (O, a, p) in enumerate(costs))


def evaluate(sp, collapse_ops, costs, base, want_grad=True):
    """lindblad_reference.evaluate with the running costs: its dict, reg_loss = loss + R + the pulse regularisers, plus reg_state (R), expectations
    (steps + 1, L, m) and, with the gradient, costates (steps + 1, m, m, n, n): Lambda_ij(tau) with its source, tau = 1 .. steps (row 0 unused)."""
    k, steps, m = sp.k, sp.steps, sp.m
    base = np.asarray(base, dtype=np.float64).reshape(k, steps)
    w = np.sin(base)
    u = sp.maxA[:, None] * w
    Ds = lr.scaled_ops(sp, collapse_ops)
    hist = lr.propagate(sp, collapse_ops, u)
    rho_final = hist[steps]
    loss = lr.loss_of(sp, rho_final)
    x = expectations(costs, hist)
    R = cost_value(costs, x, steps)
    reg_pulse, dR_dw = go.pulse_regularisers(sp, w)
    out = dict(loss=float(loss), reg_state=R, reg_loss=float(loss + R + reg_pulse), rho_final=rho_final, hist=hist, uks=u, expectations=x,
               unitary_scale=float(sum(np.real(np.trace(rho_final[i, i])) for i in range(m)) / m),
               populations=np.stack([np.real(np.einsum('tll->tl', hist[:, i, i])) for i in range(m)], axis=2))
    if not want_grad:
        return out
    dL_du = np.zeros((k, steps))
    lam = np.empty((m, m) + rho_final.shape[2:], dtype=np.complex128)
    costates = np.zeros_like(hist)
    for i in range(m):
        for j in range(m):
            lam[i, j] = -np.outer(sp.W[:, i], np.conj(sp.W[:, j])) / m ** 2
    for t in range(steps - 1, -1, -1):
        A = lr.generator(sp, Ds, u[:, t])
        for i in range(m):
            if costs:
                lam[i, i] = lam[i, i] + source(costs, x[t + 1], i, steps)
            for j in range(m):
                rho = hist[t + 1, i, j]
                costates[t + 1, i, j] = lam[i, j]
                for kk in range(k):
                    H = sp.Hs[kk + 1]
                    dL_du[kk, t] += np.real(np.sum(np.conj(lam[i, j]) * (H @ rho + rho @ H.conj().T)))
                lam[i, j] = lr.slice_map(A, Ds, lam[i, j], sp.exp_terms, sp.scaling, adjoint=True)
    grad = np.cos(base) * (sp.maxA[:, None] * dL_du + dR_dw)
    out.update(grad=grad, dL_du=dL_du, grad_squared=float(0.5 * np.sum(grad ** 2)), costates=costates)
    return out


def continue_from(sp, collapse_ops, costs, u, hist, tau):
    """loss + R of the history that agrees with hist up to tau and is propagated on from hist[tau] (which the caller may have changed)."""
    Ds = lr.scaled_ops(sp, collapse_ops)
    h = np.array(hist)
    for t in range(tau, sp.steps):
        A = lr.generator(sp, Ds, u[:, t])
        for i in range(sp.m):
            for j in range(sp.m):
                h[t + 1, i, j] = lr.slice_map(A, Ds, h[t, i, j], sp.exp_terms, sp.scaling)
    return lr.loss_of(sp, h[sp.steps]) + cost_value(costs, expectations(costs, h), sp.steps)


def run_adam(sp, collapse_ops, costs, convergence, base):
    """lindblad_reference.run_adam over this evaluation (the stop rule reads the loss, the step follows the gradient of reg_loss)."""
    conv = dict(go.CONVERGENCE_DEFAULTS)
    conv.update(convergence)
    base = np.array(base, dtype=np.float64)
    opt = go.Adam(base.shape)
    iterations = 0
    hist = []
    while True:
        r = evaluate(sp, collapse_ops, costs, base)
        hist.append((r['loss'], r['reg_loss'], r['grad_squared'], r['unitary_scale']))
        if (r['loss'] < conv['conv_target']) or (r['grad_squared'] < conv['min_grad']) or (iterations >= conv['max_iterations']):
            break
        iterations += 1
        base = opt.step(base, r['grad'], float(conv['rate']) * np.exp(-float(iterations) / conv['learning_rate_decay']))
    return dict(base=base, iterations=iterations, last=r, uks=sp.maxA[:, None] * np.sin(base), history=np.array(hist))


def trajectory(p, H0e, coeff, ops, costs, want_grad=True):
    """tests/open_fleet_reference.py: trajectory with the running costs: evaluate at the coefficients coeff (r x steps), dL_du = d(loss + R)/dc."""
    S = 2.0 * np.max(np.abs(coeff), axis=1)
    S[S == 0.0] = 1.0
    return evaluate(ofr.member_system(p, H0e, S), ops, costs, np.arcsin(coeff / S[:, None]), want_grad=want_grad)


def evaluate_members(p, cm, ens, costs, x, T=None, beta=None, want_grad=True):
    """tests/open_fleet_reference.py: evaluate with the running costs.  The members' R_e are their state regularisers: with the weights w (sum 1) the
    control set has reg_state = sum_e w_e R_e and reg_loss = sum_e w_e (loss_e + R_e) + the pulse regularisers; under a risk beta > 0 the members'
    costs are c_e = loss_e + R_e, J and the tilted weights pi_e those of include/qoc.h, reg_state = sum_e pi_e R_e, loss = J - reg_state and
    reg_loss = J + the pulse regularisers.  Adds member_reg_state (E,), reg_state and expectations (member 0) to that function's dict."""
    maxA = np.asarray(p['maxA'], dtype=np.float64)
    k = len(maxA)
    x = np.asarray(x, dtype=np.float64).reshape(k, -1)
    beta = float(ens.get('risk', 0.0)) if beta is None else float(beta)
    _, pulse_rc = ref.split_regs(p['reg_coeffs'])
    ws = np.sin(x)
    wf = ws if T is None else ws @ T.T
    u = maxA[:, None] * wf
    w = np.asarray(ens['weights'], dtype=np.float64)
    E = len(w)
    rs, vs = [], []
    for e in range(E):
        H0e, _ = rb.member_hamiltonians(p['H0'], [], ens, e)
        v = ens['amp_scales'][e][:, None] * u
        vs.append(v)
        rs.append(trajectory(p, H0e, v if cm is None else cmap.apply(cm, v), rb.member_collapse_ops(ens, e), costs, want_grad))
    loss_e = np.array([r['loss'] for r in rs])
    state_e = np.array([r['reg_state'] for r in rs])
    Pn = x.shape[1]
    view = SimpleNamespace(reg_coeffs=pulse_rc, steps=Pn, dt=p['total_time'] / Pn, k=k, total_time=p['total_time'], use_gpu=True, one_minus_gauss=None)
    val, dR = go.pulse_regularisers(view, ws)
    if beta > 0 and E > 1:
        J, pi = ref.tilt(loss_e + state_e, w, beta)
        reg_state = float(np.sum(pi * state_e))
        loss, reg_loss = J - reg_state, J + val
    else:
        pi = w
        reg_state = float(np.sum(w * state_e))
        loss, reg_loss = float(np.sum(w * loss_e)), float(np.sum(w * (loss_e + state_e))) + val
    out = dict(loss=float(loss), reg_loss=float(reg_loss), reg_state=reg_state, unitary_scale=float(np.sum(w * np.array([r['unitary_scale'] for r in rs]))),
               member_loss=loss_e, member_reg_state=state_e, weights=pi, pulse=u, uks=maxA[:, None] * ws, rho_final=rs[0]['rho_final'],
               populations=rs[0]['populations'], expectations=rs[0]['expectations'], member_rho=np.stack([r['rho_final'] for r in rs]))
    if not want_grad:
        return out
    back = (lambda v, g: g) if cm is None else (lambda v, g: cmap.pullback(cm, v, g))
    dJdu = sum(pi[e] * ens['amp_scales'][e][:, None] * back(vs[e], rs[e]['dL_du']) for e in range(E))
    grad = np.cos(x) * (maxA[:, None] * (dJdu if T is None else dJdu @ T) + dR)
    out.update(grad=grad, grad_squared=0.5 * float(np.sum(grad * grad)))
    return out
