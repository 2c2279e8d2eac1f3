"""The expected values of an ensemble engine composed from the members' OWN oracle evaluations (TEST INFRASTRUCTURE ONLY): one go.OracleSystem per
member, with its perturbations in its drift and its amplitude scales on its controls (rb.member_hamiltonians), its own maxA and the full
regularisers, evaluated by the unchanged go.evaluate (or a stand-in with its dict: tests/exact_gradient_reference.py: evaluate) -- and the members'
gradients weighted, or tilted by the soft worst case (include/qoc.h qoc_set_risk, DESIGN.md 6b').  composed_shaped is the same behind a response
matrix.  tests/composed_reference.py: combine states the same quantities at the level of the Hamiltonian's coefficients; the two
share soft_worst_case and pulse_view and nothing else, and the tests that compare them are the check of both."""
import numpy as np

from oracle import grape_oracle as go
from quantum_optimal_control.helper_functions import robust as rb
from tests.composed_reference import pulse_view, soft_worst_case
from tests.helpers import resolve_dressed


def member_systems(c, ens, taylor):
    """go.OracleSystem of every member (the unchanged oracle) of a case dict (tests/golden/cases.py style), with the engine's (T, s)."""
    out = []
    for e in range(len(ens['weights'])):
        H0e, Hopse = rb.member_hamiltonians(c['H0'], c['Hops'], ens, e)
        np.random.seed(c['np_seed'])
        out.append(go.OracleSystem(H0e, Hopse, c['U'], c['total_time'], c['steps'], c['states_concerned_list'], U0=c['U0'],
                                   reg_coeffs=c['reg_coeffs'], dressed_info=resolve_dressed(c), maxA=c['maxA'],
                                   state_transfer=c['state_transfer'], Taylor_terms=taylor))
    return out


def nominal_system(c):
    """The problem without perturbations: what the engine is given beside the ensemble."""
    return member_systems(c, dict(operators=[], offsets=np.zeros((1, 0)), amp_scales=np.ones((1, len(c['Hops']))), weights=np.ones(1)),
                          c['Taylor_terms'])[0]


def _wsum(w, rs, key):
    return sum(wi * r[key] for wi, r in zip(w, rs))


def composed(sps, w, base, beta=0.0, evaluate=go.evaluate, want_inter=False):
    """The ensemble's expected values at `base` (k x steps) from the members' evaluations (`members`: the evaluations themselves).  beta = 0: the
    weighted sums.  beta > 0: pi comes from the members' reg_loss (the common pulse term shifts every member alike and cancels in it), reg_loss is
    the soft worst case of those, grad = sum_e pi_e grad_e (the members' own gradients carry a[e][j], the chain rule and the shared pulse term;
    sum pi = 1), reg_state = sum_e pi_e reg_state_e, loss = J_c - reg_state with J_c the soft worst case of the costs c_e = loss_e + reg_state_e
    (member_cost); unitary_scale stays the w-mean."""
    rs = [evaluate(sp, base, **(dict(want_inter=True) if want_inter else {})) for sp in sps]
    reg_pulse = float(go.pulse_regularisers(sps[0], np.sin(np.asarray(base, dtype=np.float64).reshape(sps[0].k, sps[0].steps)))[0])
    reg_loss_e = np.array([r['reg_loss'] for r in rs])
    out = dict(unitary_scale=_wsum(w, rs, 'unitary_scale'), member_loss=np.array([r['loss'] for r in rs]), member_cost=reg_loss_e - reg_pulse,
               U0=rs[0]['U_final'] if not sps[0].state_transfer else None, members=rs)
    if beta == 0:
        grad = _wsum(w, rs, 'grad')
        out.update(loss=_wsum(w, rs, 'loss'), reg_loss=_wsum(w, rs, 'reg_loss'))
    else:
        reg_state_e = np.array([r['reg_loss'] - r['loss'] - reg_pulse for r in rs])
        J, pi = soft_worst_case(reg_loss_e, w, beta)
        Jc, _ = soft_worst_case(reg_loss_e - reg_pulse, w, beta)
        reg_state = float(np.dot(pi, reg_state_e))
        grad = sum(p * r['grad'] for p, r in zip(pi, rs))
        out.update(loss=Jc - reg_state, reg_loss=J, reg_state=reg_state, pi=pi)
    out.update(grad=grad, grad_squared=0.5 * float(np.sum(grad * grad)))
    return out


def composed_shaped(sps, w, T, theta, pulse_rc, total_time, beta=0.0, evaluate=go.evaluate):
    """The same behind a response matrix T (steps x P) at the samples' variable theta (k x P): the quantum part is the members' evaluation at
    arcsin(sin(theta) @ T.T) on systems that carry the state regularisers only (the sin o arcsin round trip is exact to 4e-16), the pulse part
    go.pulse_regularisers on a view of P samples of total_time / P each, the gradient cos(theta) (maxA (dL_du @ T) + dR) with the members' dL_du
    weighted (beta = 0) or tilted by their costs reg_loss_e = loss_e + reg_state_e (no pulse term inside)."""
    k, Pn = theta.shape
    ws = np.sin(theta)
    wf = ws @ T.T
    rs = [evaluate(sp, np.arcsin(wf)) for sp in sps]
    val, dR = go.pulse_regularisers(pulse_view(k, Pn, total_time, pulse_rc), ws)
    maxA = sps[0].maxA
    out = dict(unitary_scale=_wsum(w, rs, 'unitary_scale'), pulse=maxA[:, None] * wf, U0=rs[0]['U_final'] if not sps[0].state_transfer else None)
    if beta == 0:
        pi = w
        out.update(loss=_wsum(w, rs, 'loss'), reg_loss=_wsum(w, rs, 'reg_loss') + val)
    else:
        cost = np.array([r['reg_loss'] for r in rs])
        Jc, pi = soft_worst_case(cost, w, beta)
        reg_state = float(np.dot(pi, [r['reg_loss'] - r['loss'] for r in rs]))
        out.update(loss=Jc - reg_state, reg_loss=Jc + float(val), reg_state=reg_state, pi=pi, member_loss=np.array([r['loss'] for r in rs]),
                   member_cost=cost, members=rs)
    dLdu = sum(p * r['dL_du'] for p, r in zip(pi, rs))
    grad = np.cos(theta) * (maxA[:, None] * (dLdu @ T) + dR)
    out.update(grad=grad, grad_squared=0.5 * float(np.sum(grad * grad)))
    return out
