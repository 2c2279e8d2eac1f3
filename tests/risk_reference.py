"""NumPy statement of the risk-sensitive ensemble objective (include/qoc.h qoc_set_risk, DESIGN.md 6b'): test infrastructure.

    x_e = beta (c_e - c_max)             c_max = max c_e over the members with w_e > 0
    S   = sum_e w_e expm1(x_e)           members in the order 0 .. E-1
    J   = c_max + log1p(S) / beta        the soft worst case: mean <= J <= max when sum w = 1
    pi_e = w_e exp(x_e) / (1 + S)        dJ / dc_e

composed_risk builds the ensemble's expected values on the unchanged go.evaluate of every member, as tests/test_robust_gpu.py's `composed` does for
the mean; composed_risk_shaped does the same behind a response matrix, as tests/test_transfer_gpu.py's `composed`."""
from types import SimpleNamespace

import numpy as np

from oracle import grape_oracle as go


def soft_worst_case(costs, w, beta):
    """(J, pi) of member costs and weights; beta = 0: the weighted sum and the weights themselves."""
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


def composed_risk(sps, w, beta, base, evaluate=go.evaluate):
    """The risk ensemble's expected values at `base` (k x steps) from the members' oracle evaluations.  pi comes from the members' reg_loss (the
    common pulse term shifts every member alike and cancels in it), reg_loss is the soft worst case of those, grad = sum_e pi_e grad_e (the members'
    own gradients carry a[e][j], the chain rule and the shared pulse term; sum pi = 1), reg_state = sum_e pi_e reg_state_e, loss = J_c - reg_state with
    J_c the soft worst case of the costs c_e = loss_e + reg_state_e, unitary_scale the w-mean.  evaluate: go.evaluate, or a stand-in with its dict
    (tests/exact_gradient_reference.py: evaluate)."""
    rs = [evaluate(sp, base) for sp in sps]
    reg_pulse = float(go.pulse_regularisers(sps[0], np.sin(np.asarray(base, dtype=np.float64).reshape(sps[0].k, sps[0].steps)))[0])
    reg_state_e = np.array([r['reg_loss'] - r['loss'] - reg_pulse for r in rs])
    reg_loss_e = np.array([r['reg_loss'] for r in rs])
    J, pi = soft_worst_case(reg_loss_e, w, beta)
    Jc, _ = soft_worst_case(reg_loss_e - reg_pulse, w, beta)
    reg_state = float(np.dot(pi, reg_state_e))
    grad = sum(p * r['grad'] for p, r in zip(pi, rs))
    return dict(loss=Jc - reg_state, reg_loss=J, reg_state=reg_state, grad=grad, grad_squared=0.5 * float(np.sum(grad * grad)),
                unitary_scale=sum(wi * r['unitary_scale'] for wi, r in zip(w, rs)), pi=pi, member_loss=np.array([r['loss'] for r in rs]),
                member_cost=reg_loss_e - reg_pulse, members=rs)


def composed_risk_shaped(sps, w, beta, T, theta, pulse_rc, total_time):
    """The same behind a response matrix T (steps x P) at the samples' variable theta (k x P): sps are the members' systems with the state regularisers
    only, the pulse regularisers act on the samples (tests/test_transfer_gpu.py)."""
    k, Pn = theta.shape
    ws = np.sin(theta)
    wf = ws @ T.T
    rs = [go.evaluate(sp, np.arcsin(wf)) for sp in sps]
    view = SimpleNamespace(reg_coeffs=pulse_rc, steps=Pn, dt=total_time / Pn, k=k, total_time=total_time, use_gpu=True, one_minus_gauss=None)
    val, dR = go.pulse_regularisers(view, ws)
    cost = np.array([r['reg_loss'] for r in rs])                 # (no pulse term inside: loss_e + reg_state_e)
    Jc, pi = soft_worst_case(cost, w, beta)
    reg_state = float(np.dot(pi, [r['reg_loss'] - r['loss'] for r in rs]))
    maxA = sps[0].maxA
    dLdu = sum(p * r['dL_du'] for p, r in zip(pi, rs))
    grad = np.cos(theta) * (maxA[:, None] * (dLdu @ T) + dR)
    return dict(loss=Jc - reg_state, reg_loss=Jc + float(val), reg_state=reg_state, grad=grad, grad_squared=0.5 * float(np.sum(grad * grad)),
                unitary_scale=sum(wi * r['unitary_scale'] for wi, r in zip(w, rs)), pi=pi, member_loss=np.array([r['loss'] for r in rs]),
                member_cost=cost, members=rs)
