"""The expected values of a sparse ensemble engine, composed from tests/sparse_reference.py without ever forming a dense array.

Member e of an ensemble is the sparse problem with the drift H0 + sum_q offsets[e, q] P_q (a sparse sum) run at the coefficients c = apply(map, v_e),
v_e = amp_scales[e] u the member's pulses -- without a map c = v_e.  As tests/control_map_reference.py does for dense members, the trajectory is a
sparse_reference.SparseProblem on the r operators with the amplitude bound S_i = 2 max_t |c_i|, the state regularisers only, evaluated at
arcsin(c / S): from it come loss, the state regularisers, inter_vecs and dL_du = dJ/dc.  The members are combined by
tests/composed_reference.py: combine.  A fleet is evaluated device by device."""
import numpy as np
import scipy.sparse as sps

from tests import sparse_reference as sr
from tests.composed_reference import at_coefficients, combine, split_regs


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
    S, base = at_coefficients(coeff)
    return sr.evaluate(sr.SparseProblem(H0e, p.Hops, p.V, p.W, p.total_time, p.steps, p.T, S, state_rc), base)


def evaluate(p, ens, x, cm=None, T=None, beta=0.0):
    """Expected values at the variable x (k x steps, or k x P behind the line T (steps x P)) over the members of `ens` (a validated robust dict whose
    operators may be scipy.sparse): tests/composed_reference.py: combine over the sparse trajectories, with inter_vecs of member 0."""
    state_rc, pulse_rc = split_regs(p.reg_coeffs)
    out = combine(x, p.maxA, ens, p.total_time, pulse_rc, lambda e, coeff: trajectory(p, state_rc, member_drift(p, ens, e), coeff), cm=cm, T=T, beta=beta)
    out['inter_vecs'] = out['members'][0]['inter_vecs']
    return out


def evaluate_fleet(p, fl, f, x, cm=None, T=None):
    """Device f of a helper_functions.fleet.Fleet: the ensemble with that device's rows, the fleet's weights and risk."""
    return evaluate(p, fl.device(f), x, cm=cm, T=T, beta=float(fl.risk))
