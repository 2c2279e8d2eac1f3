"""NumPy reference of open-system GRAPE (TEST INFRASTRUCTURE ONLY), written from the formulas of DESIGN.md section 6e on top of the unchanged
OracleSystem: all m^2 pairs (no symmetry shortcut), history kept, adjoint sweep, first-order gradient, then the oracle's pulse regularisers and
chain rule.

With H' = -i dt H (sp.Hs) and D_j = sqrt(dt) C_j:
    A_t = H0' + sum_k u_k[t] H_k' - 1/2 sum_j D_j^dagger D_j
    L_t(X) = A_t X + X A_t^dagger + sum_j D_j X D_j^dagger,    L_t^dagger(Y) = A_t^dagger Y + Y A_t + sum_j D_j^dagger Y D_j
Slice map: N = 2^s sub-steps of X <- sum_{j = 0 .. T} (L_t / N)^j X / j! (chain X_j = (L_t / N) X_{j-1}, ascending sums), T = sp.exp_terms and
s = sp.scaling in BOTH modes."""
import math

import numpy as np

from oracle import grape_oracle as go
from tests.composed_reference import run_adam as loop


def scaled_ops(sp, collapse_ops):
    return [np.sqrt(sp.dt) * np.asarray(c, dtype=np.complex128) for c in collapse_ops]


def generator(sp, Ds, u_t):
    A = sp.Hs[0] + np.tensordot(u_t, sp.Hs[1:], axes=1)
    for D in Ds:
        A = A - 0.5 * (D.conj().T @ D)
    return A


def lindbladian(A, Ds, X, adjoint=False):
    if adjoint:
        out = A.conj().T @ X + X @ A
        for D in Ds:
            out = out + D.conj().T @ X @ D
        return out
    out = A @ X + X @ A.conj().T
    for D in Ds:
        out = out + D @ X @ D.conj().T
    return out


def slice_map(A, Ds, X, T, s, adjoint=False):
    N = 2 ** s
    for _ in range(N):
        term = X
        acc = X
        fact = 1.0
        for j in range(1, T + 1):
            term = lindbladian(A, Ds, term, adjoint) / N
            fact *= j
            acc = acc + term / fact
        X = acc
    return X


def start_vectors(sp):
    return sp.V if sp.state_transfer else sp.U0 @ sp.V


def propagate(sp, collapse_ops, u):
    """hist[tau, i, j] = rho_ij(tau), tau = 0 .. steps, shape (steps + 1, m, m, n, n)."""
    Ds = scaled_ops(sp, collapse_ops)
    psi = start_vectors(sp)
    m, n, steps = sp.m, sp.n, sp.steps
    hist = np.empty((steps + 1, m, m, n, n), dtype=np.complex128)
    for i in range(m):
        for j in range(m):
            hist[0, i, j] = np.outer(psi[:, i], np.conj(psi[:, j]))
    for t in range(steps):
        A = generator(sp, Ds, u[:, t])
        for i in range(m):
            for j in range(m):
                hist[t + 1, i, j] = slice_map(A, Ds, hist[t, i, j], sp.exp_terms, sp.scaling)
    return hist


def loss_of(sp, rho_final):
    m = sp.m
    tot = 0.0
    for i in range(m):
        for j in range(m):
            sigma = np.outer(sp.W[:, i], np.conj(sp.W[:, j]))
            tot += np.real(np.sum(np.conj(sigma) * rho_final[i, j]))               # Re Tr(sigma^dagger rho)
    return 1.0 - tot / m ** 2


def evaluate(sp, collapse_ops, base, want_grad=True):
    """dict(loss, reg_loss, grad, dL_du, grad_squared, unitary_scale, rho_final (m, m, n, n), populations (steps + 1, n, m), hist)."""
    k, steps, m = sp.k, sp.steps, sp.m
    base = np.asarray(base, dtype=np.float64).reshape(k, steps)
    w = np.sin(base)
    u = sp.maxA[:, None] * w
    Ds = scaled_ops(sp, collapse_ops)
    hist = propagate(sp, collapse_ops, u)
    rho_final = hist[steps]
    loss = loss_of(sp, rho_final)
    reg_pulse, dR_dw = go.pulse_regularisers(sp, w)
    out = dict(loss=float(loss), reg_loss=float(loss + reg_pulse), rho_final=rho_final, hist=hist, uks=u,
               unitary_scale=float(sum(np.real(np.trace(rho_final[i, i])) for i in range(m)) / m),
               populations=np.stack([np.real(np.einsum('tll->tl', hist[:, i, i])) for i in range(m)], axis=2))
    if not want_grad:
        return out
    dL_du = np.zeros((k, steps))
    lam = np.empty((m, m) + rho_final.shape[2:], dtype=np.complex128)
    for i in range(m):
        for j in range(m):
            lam[i, j] = -np.outer(sp.W[:, i], np.conj(sp.W[:, j])) / m ** 2
    for t in range(steps - 1, -1, -1):
        A = generator(sp, Ds, u[:, t])
        for i in range(m):
            for j in range(m):
                rho = hist[t + 1, i, j]
                for kk in range(k):
                    H = sp.Hs[kk + 1]
                    dL_du[kk, t] += np.real(np.sum(np.conj(lam[i, j]) * (H @ rho + rho @ H.conj().T)))
                lam[i, j] = slice_map(A, Ds, lam[i, j], sp.exp_terms, sp.scaling, adjoint=True)
    grad = np.cos(base) * (sp.maxA[:, None] * dL_du + dR_dw)
    out.update(grad=grad, dL_du=dL_du, grad_squared=float(0.5 * np.sum(grad ** 2)))
    return out


def liouvillian(A, Ds):
    """The n^2 x n^2 matrix of L on row-major vec(X): vec(A X B) = (A kron B^T) vec(X)."""
    n = A.shape[0]
    I = np.eye(n)
    Lm = np.kron(A, I) + np.kron(I, np.conj(A))
    for D in Ds:
        Lm = Lm + np.kron(D, np.conj(D))
    return Lm


def run_adam(sp, collapse_ops, convergence, base):
    """The run_session loop (oracle.grape_oracle.run_adam) over this reference: dict(base, iterations, last (the evaluation that ended the loop),
    uks, history (one row (loss, reg_loss, grad_squared, unitary_scale) per evaluation))."""
    out = loop(lambda b: evaluate(sp, collapse_ops, b), base, dict(go.CONVERGENCE_DEFAULTS, **convergence))
    return dict(out, uks=sp.maxA[:, None] * np.sin(out['base']))


def collapse_list(n, c, seed):
    """c collapse operators of spectral norm sqrt(rate): a lowering operator, a number operator, then random complex matrices."""
    rng = np.random.default_rng(1000 + seed)
    a = np.diag(np.sqrt(np.arange(1, n)), 1).astype(complex)
    pool = [a, a.conj().T @ a]
    while len(pool) < c:
        pool.append(rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n)))
    rates = [0.30, 0.20, 0.15, 0.10, 0.12, 0.08, 0.05, 0.04]
    return [math.sqrt(rates[j]) * pool[j] / np.linalg.norm(pool[j], 2) for j in range(c)]
