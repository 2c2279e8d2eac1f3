"""NumPy reference of the open-system running costs (TEST INFRASTRUCTURE ONLY), written from the definition of DESIGN.md section 6l on top of
tests/lindblad_reference.py (generator, slice_map, propagate, loss_of), over all m^2 pairs:

    x_l,i(tau) = Re sum_ac conj(O_l[a][c]) rho_ii(tau)[a][c]
    R          = sum_l (a_l / steps) sum_{tau = 0 .. steps} sum_{i < m} x_l,i(tau)^p_l / p_l
    Lambda_ii(t+1) += sum_l (a_l / steps) x_l,i(t+1)^(p_l - 1) O_l      after rho_ii(t+1) is at hand, before the contraction of slice t

A cost is a record (O, a, p), as helper_functions/open_system.py builds them.  Also here: the Adam loop over this evaluation, and the composition of
members into a control set (the weighted mean, the soft worst case of include/qoc.h with the members' costs c_e = loss_e + R_e, the line, the map) as
tests/open_fleet_reference.py composes members without costs."""
import numpy as np

from oracle import grape_oracle as go
from quantum_optimal_control.helper_functions import robust as rb
from tests import lindblad_reference as lr
from tests import open_fleet_reference as ofr
from tests.composed_reference import at_coefficients, combine, split_regs
from tests.composed_reference import run_adam as loop


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
    out = loop(lambda b: evaluate(sp, collapse_ops, costs, b), base, dict(go.CONVERGENCE_DEFAULTS, **convergence))
    return dict(out, uks=sp.maxA[:, None] * np.sin(out['base']))


def trajectory(p, H0e, coeff, ops, costs, want_grad=True):
    """tests/open_fleet_reference.py: trajectory with the running costs: evaluate at the coefficients coeff (r x steps), dL_du = d(loss + R)/dc."""
    S, base = at_coefficients(coeff)
    return evaluate(ofr.member_system(p, H0e, S), ops, costs, base, want_grad=want_grad)


def evaluate_members(p, cm, ens, costs, x, T=None, beta=None, want_grad=True):
    """tests/open_fleet_reference.py: evaluate with the running costs.  The members' R_e are their state regularisers: with the weights w (sum 1) the
    control set has reg_state = sum_e w_e R_e and reg_loss = sum_e w_e (loss_e + R_e) + the pulse regularisers; under a risk beta > 0 the members'
    costs are c_e = loss_e + R_e, J and the tilted weights pi_e those of include/qoc.h, reg_state = sum_e pi_e R_e, loss = J - reg_state and
    reg_loss = J + the pulse regularisers (tests/composed_reference.py: combine).  Adds expectations (member 0) to that function's read-backs."""
    run = lambda e, coeff: trajectory(p, rb.member_hamiltonians(p['H0'], [], ens, e)[0], coeff, rb.member_collapse_ops(ens, e), costs, want_grad)
    out = ofr.read_backs(combine(x, p['maxA'], ens, p['total_time'], split_regs(p['reg_coeffs'])[1], run, cm=cm, T=T, beta=beta, want_grad=want_grad))
    out['expectations'] = out['members'][0]['expectations']
    return out
