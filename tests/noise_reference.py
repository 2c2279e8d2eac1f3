"""The expected values of an engine with a table of noise traces, composed from the unchanged oracle (TEST INFRASTRUCTURE ONLY).

With a table, frozen row q' of member e has at slice t the value offsets[e, q'] + traces[e, q', t].  A perturbation no longer folds into the
member's drift, so a member's trajectory is what tests/control_map_reference.py: trajectory already runs -- the oracle at given COEFFICIENTS --
on the problem c' whose operators are Hops + the perturbation operators, at the coefficients
    coeff = [ the member's control rows (its pulses a[e, j] u_j, or apply(map, them)) ; offsets[e][:, None] + traces[e] ]
through that function's arcsin(coeff / S) device, with the nominal drift H0 and the state regularisers only.  Of its dL_du = dJ/dcoeff the first r
rows are the member's dJ/dc; the frozen rows have no reader.  The members are then combined by tests/composed_reference.py: combine, as
tests/control_map_reference.py: evaluate combines them; the frozen rows are appended inside the member's run (with_rows), so the pulse
regularisers never see them.  Open members run through tests/running_cost_reference.py: trajectory (which is
tests/open_fleet_reference.py: trajectory when there is no cost), sparse ones through tests/sparse_ensemble_reference.py: trajectory."""
import numpy as np

from quantum_optimal_control.helper_functions import robust as rb
from tests import control_map_reference as ref
from tests.composed_reference import combine, split_regs


def member_rows(ens, e, steps):
    """offsets[e][:, None] + traces[e]: the q frozen rows of member e, (q, steps).  No table: the constant rows."""
    off = np.asarray(ens['offsets'], dtype=np.float64)[e][:, None]
    tr = ens.get('traces')
    return off + (np.zeros((off.shape[0], steps)) if tr is None else np.asarray(tr, dtype=np.float64)[e])


def with_rows(ens, steps, trajectory):
    """combine's run(e, c) for members with frozen rows: trajectory(e, coeff) at coeff = [c ; member_rows] ((r + q) x steps), its dL_du cut back to
    the r rows of c."""
    def run(e, c):
        r = trajectory(e, np.vstack([c, member_rows(ens, e, steps)]))
        return dict(r, dL_du=r['dL_du'][:len(c)]) if 'dL_du' in r else r
    return run


def evaluate(c, ens, x, cm=None, T=None, exact=False, beta=None, want_grad=True):
    """A dense closed engine (c: a case dict of tests/control_map_reference.py: problem style, `maxA` of k entries; ens: a validated robust dict with
    or without traces) at the variable x (k x steps, or k x P behind the line T): loss, reg_loss, grad, grad_squared, unitary_scale, member_loss,
    weights, pulse, uks, coefficients (member 0's r rows), U_final / member_U / inter_vecs as tests/control_map_reference.py: evaluate gives them."""
    state_rc, pulse_rc = split_regs(c['reg_coeffs'])
    cp = dict(c, Hops=list(c['Hops']) + [np.asarray(p, dtype=np.complex128) for p in ens['operators']])
    run = with_rows(ens, c['steps'], lambda e, coeff: ref.trajectory(cp, state_rc, c['H0'], coeff, exact, want_grad))
    out = combine(x, c['maxA'], ens, c['total_time'], pulse_rc, run, cm=cm, T=T, beta=beta, want_grad=want_grad)
    return ref.read_backs(out, c['state_transfer'], want_grad)


def evaluate_open(p, ens, x, cm=None, T=None, beta=None, costs=(), want_grad=True):
    """An open engine (p: tests/open_fleet_reference.py: problem; ens with collapse_ops and rate_scales; costs: running-cost records): the dict of
    evaluate with rho_final and populations of member 0, member_rho, and expectations of member 0."""
    from tests import open_fleet_reference as ofr
    from tests import running_cost_reference as rcr
    pp = dict(p, Hops=list(p['Hops']) + [np.asarray(op, dtype=np.complex128) for op in ens['operators']])
    run = with_rows(ens, p['steps'], lambda e, coeff: rcr.trajectory(pp, p['H0'], coeff, rb.member_collapse_ops(ens, e), list(costs), want_grad))
    out = ofr.read_backs(combine(x, p['maxA'], ens, p['total_time'], split_regs(p['reg_coeffs'])[1], run, cm=cm, T=T, beta=beta, want_grad=want_grad))
    out['expectations'] = out['members'][0]['expectations']
    return out


def evaluate_sparse(p, ens, x, cm=None, T=None, beta=None):
    """A sparse engine (p: tests/sparse_ensemble_reference.py: Problem; the operators of ens may be scipy.sparse): the dict of evaluate with member
    0's inter_vecs."""
    from tests import sparse_ensemble_reference as ser
    state_rc, pulse_rc = split_regs(p.reg_coeffs)
    pp = ser.Problem(p.H0, list(p.Hops) + list(ens['operators']), p.V, p.W, p.total_time, p.steps, p.T, p.maxA, p.reg_coeffs)
    out = combine(x, p.maxA, ens, p.total_time, pulse_rc, with_rows(ens, p.steps, lambda e, coeff: ser.trajectory(pp, state_rc, p.H0, coeff)), cm=cm, T=T,
                  beta=beta)
    out['inter_vecs'] = out['members'][0]['inter_vecs']
    return out


def with_traces(ens, traces):
    """The validated robust dict `ens` with the table `traces` (E, q, steps), or without one (None)."""
    out = {key: v for key, v in ens.items() if key != 'traces'}
    if traces is not None:
        out['traces'] = np.array(traces, dtype=np.float64)
    return out


def make_traces(E, q, steps, seed=0, F=None, scale=0.3):
    """Random traces in which one (member, operator) row is zero except at a single slice, so that a transposed index cannot pass; F given: a leading
    device axis, every device with a draw (and a lone slice) of its own."""
    rng = np.random.default_rng(9000 + seed)
    tr = rng.uniform(-scale, scale, size=((F or 1), E, q, steps))
    for f in range(tr.shape[0]):
        e, qq, t = (f + 1) % E, (f + q - 1) % q, (2 + 3 * f) % steps
        tr[f, e, qq, :] = 0.0
        tr[f, e, qq, t] = scale * (1.0 + 0.1 * f)
    return tr if F else tr[0]
