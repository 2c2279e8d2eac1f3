"""The expected values of a sparse ensemble engine, composed from tests/sparse_reference.py without ever forming a dense array.

Member e of an ensemble is the sparse problem with the drift H0 + sum_q offsets[e, q] P_q (a sparse sum) run at the coefficients c = apply(map, v_e),
v_e = amp_scales[e] u the member's pulses -- without a map c = v_e.  As tests/control_map_reference.py does for dense members, the trajectory is a
sparse_reference.SparseProblem on the r operators with the amplitude bound S_i = 2 max_t |c_i|, the state regularisers only, evaluated at
arcsin(c / S): from it come loss, the state regularisers, inter_vecs and dL_du = dJ/dc.  The members are weighted, or tilted by
tests/risk_reference.py: soft_worst_case; the gradient is sum_e pi_e a[e, j] (pullback of dJ/dc), a line T applied as a matrix product, and the pulse
regularisers are go.pulse_regularisers on the k pulses (on the P samples behind a line).  A fleet is evaluated device by device."""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sps

from oracle import grape_oracle as go
from quantum_optimal_control.helper_functions import control_map as cmap
from tests import sparse_reference as sr
from tests.risk_reference import soft_worst_case

PULSE_KEYS = ('amplitude', 'envelope', 'dwdt', 'd2wdt2', 'bandpass', 'band')


class Problem(object):
    """H0 and the r operators (scipy.sparse), V and W (n x m), the k pulse bounds maxA, the Taylor order and the regularisers."""

    def __init__(self, H0, Hops, V, W, total_time, steps, T, maxA, reg_coeffs=None):
        self.H0, self.Hops = sps.csr_matrix(H0, dtype=np.complex128), [sps.csr_matrix(h, dtype=np.complex128) for h in Hops]
        self.n = self.H0.shape[0]
        self.V, self.W = np.asarray(V, dtype=np.complex128).reshape(self.n, -1), np.asarray(W, dtype=np.complex128).reshape(self.n, -1)
        self.m = self.V.shape[1]
        self.total_time, self.steps, self.dt, self.T = float(total_time), int(steps), float(total_time) / steps, int(T)
        self.maxA = np.asarray(maxA, dtype=np.float64)
        self.k = len(self.maxA)
        self.reg_coeffs = dict(reg_coeffs or {})

    def engine_ops(self):
        """[-i dt H0, -i dt G_1 ..]: what HipEngine's sparse_ops takes (the perturbations go in through the ensemble dict)."""
        return [sps.csr_matrix(-1j * self.dt * h) for h in [self.H0] + self.Hops]


def from_sparse_case(sp):
    """tests/sparse_reference.py: SparseProblem -> Problem (the same operators, vectors, bounds and regularisers)."""
    return Problem(sp.H0_in, sp.Hops_in, sp.V, sp.W, sp.total_time, sp.steps, sp.exp_terms, sp.maxA, sp.reg_coeffs)


def nominal(k):
    return dict(operators=[], offsets=np.zeros((1, 0)), amp_scales=np.ones((1, k)), weights=np.ones(1), risk=0.0)


def member_drift(p, ens, e):
    """H0 + sum_q offsets[e, q] P_q, sparse."""
    H = p.H0
    for qq, op in enumerate(ens['operators']):
        H = H + float(ens['offsets'][e, qq]) * sps.csr_matrix(op, dtype=np.complex128)
    return sps.csr_matrix(H)


def trajectory(p, state_rc, H0e, coeff):
    """sparse_reference.evaluate at the coefficients coeff (r x steps): its dict, with dL_du = dJ/dc."""
    S = 2.0 * np.max(np.abs(coeff), axis=1)
    S[S == 0.0] = 1.0
    sp = sr.SparseProblem(H0e, p.Hops, p.V, p.W, p.total_time, p.steps, p.T, S, state_rc)
    return sr.evaluate(sp, np.arcsin(coeff / S[:, None]))


def evaluate(p, ens, x, cm=None, T=None, beta=0.0):
    """Expected values at the variable x (k x steps, or k x P behind the line T (steps x P)) over the members of `ens` (a validated robust dict whose
    operators may be scipy.sparse): loss, reg_loss, grad, grad_squared, unitary_scale, member_loss, member_reg_state, weights (pi), pulse, uks,
    coefficients and inter_vecs of member 0."""
    k = p.k
    x = np.asarray(x, dtype=np.float64).reshape(k, -1)
    state_rc = {key: v for key, v in p.reg_coeffs.items() if key not in PULSE_KEYS}
    pulse_rc = {key: v for key, v in p.reg_coeffs.items() if key in PULSE_KEYS}
    ws = np.sin(x)
    wf = ws if T is None else ws @ T.T
    u = p.maxA[:, None] * wf
    w = np.asarray(ens['weights'], dtype=np.float64)
    E = len(w)
    rs, vs = [], []
    for e in range(E):
        v = ens['amp_scales'][e][:, None] * u
        vs.append(v)
        rs.append(trajectory(p, state_rc, member_drift(p, ens, e), v if cm is None else cmap.apply(cm, v)))
    loss_e = np.array([r['loss'] for r in rs])
    state_e = np.array([r['reg_loss'] - r['loss'] for r in rs])
    Pn = x.shape[1]
    omg = None
    if 'envelope' in pulse_rc:
        grid = np.linspace(-2, 2, Pn)
        shape = np.ones(Pn) - np.exp(-np.power(grid, 2.) / 2.)
        omg = np.tile(shape * (shape > 0) + 0.01 * np.ones(Pn), (k, 1))
    view = SimpleNamespace(reg_coeffs=pulse_rc, steps=Pn, dt=p.total_time / Pn, k=k, total_time=p.total_time, use_gpu=True, one_minus_gauss=omg)
    val, dR = go.pulse_regularisers(view, ws)
    if beta > 0 and E > 1:
        J, pi = soft_worst_case(loss_e + state_e, w, beta)
        reg_state = float(np.sum(pi * state_e))
        loss, reg_loss = J - reg_state, J + val
    else:
        pi = w
        loss, reg_loss = float(np.sum(w * loss_e)), float(np.sum(w * (loss_e + state_e))) + val
    pull = (lambda v, g: g) if cm is None else (lambda v, g: cmap.pullback(cm, v, g))
    dJdu = sum(pi[e] * ens['amp_scales'][e][:, None] * pull(vs[e], rs[e]['dL_du']) for e in range(E))
    grad = np.cos(x) * (p.maxA[:, None] * (dJdu if T is None else dJdu @ T) + dR)
    return dict(loss=loss, reg_loss=float(reg_loss), grad=grad, grad_squared=0.5 * float(np.sum(grad * grad)),
                unitary_scale=float(np.sum(w * np.array([r['unitary_scale'] for r in rs]))), member_loss=loss_e, member_reg_state=state_e, weights=pi,
                pulse=u, uks=p.maxA[:, None] * ws, coefficients=vs[0] if cm is None else cmap.apply(cm, vs[0]), inter_vecs=rs[0]['inter_vecs'])


def evaluate_fleet(p, fl, f, x, cm=None, T=None):
    """Device f of a helper_functions.fleet.Fleet: the ensemble with that device's rows, the fleet's weights and risk."""
    return evaluate(p, fl.device(f), x, cm=cm, T=T, beta=float(fl.risk))


def run_adam(evaluate_at, x0, conv):
    """tests/control_map_reference.py: run_adam (the device loop's semantics over any evaluation)."""
    from tests.control_map_reference import run_adam as loop
    return loop(evaluate_at, x0, conv)
