"""Reference of the sparse state-transfer path (csrc/qoc_sparse.h, qoc_create_sparse): the state-transfer branch of oracle/grape_oracle.py (evaluate,
matvecexp) restated on scipy.sparse operators.  No dense n x n array is formed anywhere in this file, so it also serves at n = 16384, where the dense
oracle cannot go; tests/test_sparse.py holds it to the dense oracle at n = 16 and n = 64.

    B_t = H0' + sum_k u_k[t] H_k'  (H' = -i dt H);  psi_{t+1} = sum_{j < T} B_t^j psi_t / j!  (a chain, summed in ascending j)
    lam_N = (-2 / m^2) z W + S_N;  lam_t = sum_{j < T} (-B_t)^j lam_{t+1} / j! + S_t;  dL/du[k, t] = Re <lam_{t+1}, H_k' psi_{t+1}>
The pulse and state regularisers are the oracle's own functions: they read the controls and the propagated vectors, never an operator.
"""
import numpy as np
import scipy.sparse as sps

from oracle import grape_oracle as go


class SparseProblem(object):
    """What OracleSystem holds, with `ops` = [-i dt H0, -i dt H_1, ...] as CSR in place of the dense stack Hs."""

    def __init__(self, H0, Hops, V, W, total_time, steps, taylor_terms, maxA, reg_coeffs=None, base0=None):
        self.H0_in, self.Hops_in = H0, list(Hops)
        self.n, self.k, self.steps = H0.shape[0], len(Hops), int(steps)
        self.total_time, self.dt = total_time, float(total_time) / steps
        self.V = np.asarray(V, dtype=np.complex128).reshape(self.n, -1)
        self.W = np.asarray(W, dtype=np.complex128).reshape(self.n, -1)
        self.m = self.V.shape[1]
        self.maxA = np.asarray(maxA, dtype=np.float64)
        self.exp_terms, self.scaling = int(taylor_terms), 0
        self.state_transfer, self.use_gpu, self.Vs = True, True, None
        self.reg_coeffs = {} if reg_coeffs is None else reg_coeffs
        self.ops = [sps.csr_matrix(-1j * self.dt * sps.csr_matrix(h, dtype=np.complex128)) for h in [H0] + list(Hops)]
        x = np.linspace(-2, 2, self.steps)
        shape = np.ones(self.steps) - np.exp(-np.power(x, 2.) / 2.)
        self.one_minus_gauss = np.tile(shape * (shape > 0) + 0.01 * np.ones(self.steps), (self.k, 1))
        self.base0 = base0


def _generator(sp, u_t):
    B = sp.ops[0]
    for kk in range(sp.k):
        B = B + float(u_t[kk]) * sp.ops[kk + 1]
    return sps.csr_matrix(B)


def _chain(B, psi, T, sign=1.0):
    out, pn, fact = psi, psi, 1.0
    for ii in range(1, T):
        fact *= ii
        pn = sign * (B @ pn)
        out = out + pn / fact
    return out


def evaluate(sp, base):
    """dict(loss, reg_loss, grad, dL_du, grad_squared, unitary_scale, inter_vecs) at the variable `base` (k x steps)."""
    n, k, steps, m, T = sp.n, sp.k, sp.steps, sp.m, sp.exp_terms
    base = np.asarray(base, dtype=np.float64).reshape(k, steps)
    w = np.sin(base)
    u = sp.maxA[:, None] * w
    inter = np.empty((steps + 1, n, m), dtype=np.complex128)
    inter[0] = sp.V
    for t in range(steps):
        inter[t + 1] = _chain(_generator(sp, u[:, t]), inter[t], T)
    fin = inter[steps]
    z = np.sum(fin * np.conj(sp.W))
    loss = 1.0 - np.abs(z) ** 2 / m ** 2
    reg_pulse, dR_dw = go.pulse_regularisers(sp, w)
    rc = sp.reg_coeffs
    if 'forbidden_coeff_list' in rc or 'speed_up' in rc:
        reg_state, S = go.state_regularisers(sp, inter)
    else:
        reg_state, S = 0.0, None
    dL_du = np.zeros((k, steps))
    lam = (-2.0 / m ** 2) * z * sp.W
    if S is not None:
        lam = lam + S[steps]
    for t in range(steps - 1, -1, -1):
        for kk in range(k):
            dL_du[kk, t] = np.real(np.sum(np.conj(lam) * (sp.ops[kk + 1] @ inter[t + 1])))
        lam = _chain(_generator(sp, u[:, t]), lam, T, sign=-1.0)
        if S is not None and t > 0:
            lam = lam + S[t]
    grad = np.cos(base) * (sp.maxA[:, None] * dL_du + dR_dw)
    return dict(loss=float(loss), reg_loss=float(loss + reg_pulse + reg_state), grad=grad, dL_du=dL_du, grad_squared=float(0.5 * np.sum(grad ** 2)),
                unitary_scale=float(np.sum(np.abs(fin) ** 2) ** 2 / m ** 2), inter_vecs=inter, uks=u)


# ---- problems -----------------------------------------------------------------------------------------------------------------------------------

def random_sparse(rng, n, per_row=(1, 6), hermitian=True):
    """n x n complex CSR with per_row[0] .. per_row[1] entries in every row at random columns; hermitian: (A + A^dagger) / 2 of it."""
    lo, hi = min(per_row[0], n), min(per_row[1], n)
    rows, cols = [], []
    for r in range(n):
        c = rng.choice(n, size=int(rng.integers(lo, hi + 1)), replace=False)
        rows += [r] * len(c)
        cols += list(c)
    vals = rng.normal(size=len(rows)) + 1j * rng.normal(size=len(rows))
    A = sps.csr_matrix((vals, (rows, cols)), shape=(n, n))
    if hermitian:
        A = sps.csr_matrix((A + A.conj().T) / 2)
    return A


def unit_columns(rng, n, m):
    X = rng.normal(size=(n, m)) + 1j * rng.normal(size=(n, m))
    return X / np.linalg.norm(X, axis=0)[None, :]


ALL_REGS = {'amplitude': 0.3, 'envelope': 0.2, 'dwdt': 0.02, 'd2wdt2': 0.001, 'speed_up': 0.4, 'bandpass': 0.1, 'band': [0.4, 1.0]}


def sparse_case(n, steps, k=2, m=1, T=8, seed=0, kind='random', reg_coeffs=None, forbidden=False):
    """A seeded sparse problem.  kind: random (1 to 6 entries per row, Hermitian), dense (every entry stored), diagonal, zero_control (control 0 has
    no entry), disjoint (the operators' patterns share no position), nonhermitian.  forbidden: two bare forbidden levels join reg_coeffs."""
    rng = np.random.default_rng(1000 + seed)
    if kind == 'dense':
        mk = lambda: random_sparse(rng, n, (n, n), True)
    elif kind == 'diagonal':
        mk = lambda: sps.diags(rng.normal(size=n).astype(np.complex128), format='csr')
    elif kind == 'disjoint':
        offs = iter(range(0, k + 1))
        mk = lambda: sps.csr_matrix((rng.normal(size=n) + 1j * rng.normal(size=n), (np.arange(n), (np.arange(n) + next(offs)) % n)), shape=(n, n))
    elif kind == 'nonhermitian':
        mk = lambda: 0.4 * random_sparse(rng, n, (1, 6), False)        # (scaled down: nothing keeps the norm of the vectors at 1 here)
    else:
        mk = lambda: random_sparse(rng, n, (1, 6), True)
    H0 = mk()
    Hops = [mk() for _ in range(k)]
    if kind == 'zero_control':
        Hops[0] = sps.csr_matrix((n, n), dtype=np.complex128)
    rc = dict(reg_coeffs or {})
    if forbidden:
        rc.update(forbidden_coeff_list=[3.0, 1.5], states_forbidden_list=[n - 1, n // 2])
    total_time = 0.12 * steps
    base0 = rng.normal(0, 0.6, size=(k, steps))
    return SparseProblem(H0, Hops, unit_columns(rng, n, m), unit_columns(rng, n, m), total_time, steps, T, [1.0 + 0.25 * i for i in range(k)], rc, base0)


def bases_of(sp, count=3):
    """`count` variables of a problem: its own base0 and seeded perturbations of it."""
    rng = np.random.default_rng(77)
    return [sp.base0] + [sp.base0 + rng.normal(0, 0.3, size=sp.base0.shape) for _ in range(count - 1)]


def dense_oracle(sp):
    """The dense OracleSystem of a (small) sparse problem: what oracle.grape_oracle.evaluate runs on."""
    return go.OracleSystem(sp.H0_in.toarray(), [h.toarray() for h in sp.Hops_in], [sp.W[:, j] for j in range(sp.m)], sp.total_time, sp.steps,
                           [sp.V[:, j] for j in range(sp.m)], reg_coeffs=sp.reg_coeffs, maxA=sp.maxA, state_transfer=True, Taylor_terms=(sp.exp_terms, 0))


def chain_problem(spins, steps, T, k=2, seed=5, target_site=None):
    """The XX chain of helper_functions/synthetic_systems.xx_chain: an excitation sent from the first spin to `target_site` (default: the last), z controls
    on the first k sites counted from both ends alternately."""
    from quantum_optimal_control.helper_functions.synthetic_systems import xx_chain
    ends = [0, spins - 1, 1, spins - 2, 2, spins - 3][:k]
    H0, Hops, _, exc = xx_chain(spins, coupling=1.0, control_sites=ends)
    rng = np.random.default_rng(seed)
    return SparseProblem(H0, Hops, exc(0), exc(spins - 1 if target_site is None else target_site), 0.25 * steps, steps, T, [2.0] * k, {}, rng.normal(0, 0.6, size=(k, steps)))
