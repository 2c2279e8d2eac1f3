"""The expected values of a mapped engine, composed from the unchanged oracle.

A trajectory of a mapped engine is the oracle's problem on the r operators the map feeds, run at the coefficients c = apply(map, v) in place of a
pulse: a go.OracleSystem with those operators (a member's perturbations folded into its drift, as tests/test_robust_gpu.py does), the amplitude
bound S_i = 2 max_t |c_i| (so that arcsin is far from its end points) and only the state regularisers, evaluated at arcsin(c / S).  From it come
loss, inter_vecs and dL_du = dJ/dc -- the oracle's first-order gradient, or the exact one of tests/exact_gradient_reference.py.  The chain rule
    dJ/dv_j[t] = sum_i dJ/dc_i[t] M[i, j, t] p_ij'(v_j[t])
the weighting or tilt of the members, the line and the pulse regularisers on the k pulses (on the P samples behind a line) are
tests/composed_reference.py: combine."""
import numpy as np

from oracle import grape_oracle as go
from quantum_optimal_control.helper_functions import control_map as cmap
from quantum_optimal_control.helper_functions import robust as rb
from quantum_optimal_control.helper_functions.synthetic_systems import herm, random_unitary
from tests import exact_gradient_reference as xr
from tests.composed_reference import at_coefficients, combine, split_regs
from tests.composed_reference import central_differences, run_adam          # noqa: F401  (re-exported for the tests)


def problem(n, r, k, steps, m, state_transfer=False, taylor=(6, 1), seed=0, total_time=None, regs=None):
    """A synthetic problem with r operators and k pulses (tests/golden/cases.py style, with `maxA` of k entries)."""
    rng = np.random.default_rng(1000 + seed)
    H0 = 2 * np.pi * 0.3 * herm(rng, n)
    Hops = [2 * np.pi * 0.15 * herm(rng, n) for _ in range(r)]
    if state_transfer:
        vec = lambda: (lambda v: v / np.linalg.norm(v))(rng.normal(size=n) + 1j * rng.normal(size=n))
        states = [vec() for _ in range(m)]
        U = [vec() for _ in range(m)]
        taylor = (taylor[0], 0)
    else:
        states = list(range(m))
        U = random_unitary(rng, n)
    return dict(H0=H0, Hops=Hops, U=U, total_time=0.25 * steps if total_time is None else total_time, steps=steps, states_concerned_list=states,
                U0=None if state_transfer else random_unitary(rng, n), maxA=rng.uniform(0.8, 1.6, size=k), state_transfer=state_transfer,
                Taylor_terms=list(taylor), reg_coeffs=dict(regs or {}), np_seed=seed)


def make_map(k, r, D, steps, mix=False, fixed=False, seed=0):
    """A dense random map: every polynomial coefficient nonzero, a signed slice-dependent M and an F where asked for."""
    rng = np.random.default_rng(2000 + 17 * seed + 100 * k + 10 * r + D)
    alpha = rng.uniform(0.3, 1.0, size=(r, k, D)) * rng.choice([-1.0, 1.0], size=(r, k, D)) / np.arange(1, D + 1)
    M = rng.uniform(-1.0, 1.0, size=(r, k, steps)) if mix else None
    F = rng.uniform(-0.5, 0.5, size=(r, steps)) if fixed else None
    return cmap.validate(cmap.ControlMap(alpha, M, F), k=k, r=r, steps=steps)


def nominal_ensemble(k):
    return dict(operators=[], offsets=np.zeros((1, 0)), amp_scales=np.ones((1, k)), weights=np.ones(1), risk=0.0)


def ensemble(c, E, q, seed=5):
    """tests/test_robust_gpu.py: ensemble, on the k pulses of a mapped problem."""
    rng = np.random.default_rng(seed)
    n, k = len(c['H0']), len(c['maxA'])
    if E == 1 and q == 0:
        return rb.validate(nominal_ensemble(k), n, k)
    ops = [0.3 * 2 * np.pi * herm(rng, n) for _ in range(q)]
    return rb.validate(dict(operators=ops, offsets=rng.uniform(-0.2, 0.2, size=(E, q)), amp_scales=rng.uniform(0.9, 1.1, size=(E, k)),
                            weights=rng.uniform(0.5, 1.5, size=E)), n, k)


def engine_system(c):
    """What the engine is given beside the map, the ensemble and the line: the oracle's arrays for the r operators (Hs, U0, V, W, T, s); its maxA and
    base0 belong to no pulse and are not used."""
    np.random.seed(c['np_seed'])
    return go.OracleSystem(c['H0'], c['Hops'], c['U'], c['total_time'], c['steps'], c['states_concerned_list'], U0=c['U0'], reg_coeffs=c['reg_coeffs'],
                           maxA=np.ones(len(c['Hops'])), state_transfer=c['state_transfer'], Taylor_terms=c['Taylor_terms'])


def trajectory(c, state_rc, H0e, coeff, exact=False, want_grad=True):
    """The oracle at the coefficients coeff (r x steps): its evaluation dict, with dL_du = dJ/dc."""
    S, base = at_coefficients(coeff)
    np.random.seed(c['np_seed'])
    sp = go.OracleSystem(H0e, c['Hops'], c['U'], c['total_time'], c['steps'], c['states_concerned_list'], U0=c['U0'], reg_coeffs=state_rc, maxA=S,
                         state_transfer=c['state_transfer'], Taylor_terms=c['Taylor_terms'])
    if not want_grad:
        return go.evaluate(sp, base, want_grad=False)
    return xr.evaluate(sp, base) if exact else go.evaluate(sp, base, want_inter=True)


def read_backs(out, state_transfer, want_grad):
    """combine's dict with the read-backs of a dense closed engine: U_final and (with the gradient) inter_vecs of member 0, member_U (every member's
    final unitary; None in state-transfer mode)."""
    rs = out['members']
    out.update(U_final=rs[0]['U_final'], member_U=None if state_transfer else np.stack([r['U_final'] for r in rs]))
    if want_grad:
        out['inter_vecs'] = rs[0]['inter_vecs']
    return out


def evaluate(c, cm, ens, x, T=None, exact=False, beta=0.0, want_grad=True):
    """The mapped engine's expected values at the variable x (k x steps, or k x P behind the line T (steps x P)) for the members of `ens` (a validated
    robust dict): tests/composed_reference.py: combine over the oracle's trajectories, a member's perturbations folded into its drift, with the
    read-backs above."""
    state_rc, pulse_rc = split_regs(c['reg_coeffs'])
    out = combine(x, c['maxA'], ens, c['total_time'], pulse_rc, cm=cm, T=T, beta=beta, want_grad=want_grad,
                  run=lambda e, coeff: trajectory(c, state_rc, rb.member_hamiltonians(c['H0'], [], ens, e)[0], coeff, exact, want_grad))
    return read_backs(out, c['state_transfer'], want_grad)


def variables(k, Pn, G, seed=0):
    return np.random.default_rng(3000 + Pn + seed).normal(0.0, 0.7, size=(3, k, Pn))[:G]
