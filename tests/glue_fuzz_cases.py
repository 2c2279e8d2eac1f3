"""Seeded random draws for the glue between the views of an ensemble engine (tests/test_glue_fuzz.py): k_ens_expand / k_ens_reduce(_risk), k_ens_tilt,
k_shape_expand / k_shape_reduce(_risk)<1|64>, k_map_expand / k_map_reduce, as robust ensembles, risk, transfer lines, control maps, device fleets,
open-system members and sparse operators reach them through create_composed.

Three families, each a pure function of its seed: closed(seed), opened(seed), sparse(seed).  A draw holds the problem, the glue objects (the
ensemble or the Fleet, the map, the line's matrix, beta, the exact flag), the start points `xs` of its G control sets, `info` (what was drawn: it
goes into every assertion message), and `expected()`: the reference of every control set, composed by tests/control_map_reference.py,
tests/open_fleet_reference.py or tests/sparse_ensemble_reference.py from the unchanged oracle, each with the members' own unitary_scale beside it.

There is no re-draw rule: a seed is its draw.  The operator scales are those of control_map_reference.problem and dt lies in 0.1 .. 0.3.  Nothing
here imports the engine; the draws are checked on the CPU by the unmarked tests of tests/test_glue_fuzz.py.

Where the draws leave the ranges the families are described by:
  * r + q = 9 cannot come out of r <= 4 and q <= 3, so about one closed draw in sixteen is a `nine` draw: a map onto r = 6 .. 8 operators and q = 9 - r.
  * A response matrix with an all-zero column is refused by helper_functions/transfer.py: validate and by create_shaped ("column p of T is zero (the
    sample never reaches the pulse)"), so the dense line has its all-zero row and, in place of the all-zero column, a column with ONE nonzero entry
    (a window of one slice, against the full windows of its neighbours).
"""
import functools
from types import SimpleNamespace

import numpy as np

from quantum_optimal_control.helper_functions import control_map as cmap
from quantum_optimal_control.helper_functions import fleet as fl_mod
from quantum_optimal_control.helper_functions import robust as rb
from quantum_optimal_control.helper_functions import transfer as tf
from quantum_optimal_control.helper_functions.synthetic_systems import herm
from tests import control_map_reference as ref
from tests.composed_reference import pulse_view, run_adam

CLOSED_SEEDS, OPEN_SEEDS, SPARSE_SEEDS = 96, 32, 32
CLOSED_N = (2, 5, 12, 13, 16, 17, 24, 31, 32, 33, 40, 47, 48, 49, 63, 64, 65, 70)
CLOSED_STEPS = (1, 2, 3, 7, 8, 9, 16, 17, 31, 33, 40, 64, 65, 70)
OPEN_N = (2, 3, 5, 8, 9, 16, 17, 24, 32)
SPARSE_N = (16, 24, 64, 100, 257)
LINES = ('none', 'hold', 'linear_interp', 'gaussian_filter', 'dense')
MFMA_CHUNKS, GEMM_CHUNKS = (0, 3, 2, 5, 4), (0, 1, 2)            # tests/test_hip_fuzz.py: the chunk counts it asks the two paths for
ADAM = dict(rate=0.02, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=4)
# The member tables (operators, offsets, scales, weights) come from a stream of their own, so that the shapes a seed draws do not depend on them.
# Whether two members' losses fall within 1e-6 of each other is chance (a random target at n = 48 leaves every member's loss within 1e-3 of 1), and
# tests/test_glue_fuzz.py: test_devices_and_members_are_apart holds the committed streams to it; the closed stream was chosen as the first of
# 51_000, 52_000, .. that passes.
MEMBER_STREAM = dict(closed=58_000, open=61_000, sparse=71_000)


# ---- what the three families share ------------------------------------------------------------------------------------------------------------------

def draw_line(rng, kind, steps, total_time):
    """(T or None, widest column window): the response matrix of a line kind with P = 1 .. steps samples."""
    if kind == 'none':
        return None, 0
    P = int(rng.integers(1, steps + 1))
    if kind == 'hold':
        T = tf.hold(steps, P).matrix
    elif kind == 'linear_interp':
        T = tf.linear_interp(steps, P).matrix
    elif kind == 'gaussian_filter':
        T = tf.gaussian_filter(steps, P, total_time, float(rng.uniform(0.5, 2.0)) * total_time / steps).matrix
    else:
        # dense and signed, rows of l1 norm <= 1; one all-zero row inside (not at an end, where it would only shorten the windows) and one column
        # with a single entry
        T = rng.uniform(0.2, 1.0, size=(steps, P)) * rng.choice([-1.0, 1.0], size=(steps, P)) / P
        if steps >= 3:
            T[int(rng.integers(1, steps - 1))] = 0.0
        if P >= 2 and steps >= 3:
            p, t = int(rng.integers(0, P)), int(rng.integers(0, steps))
            while not np.any(T[t]):
                t = (t + 1) % steps
            keep = T[t, p]
            T[:, p] = 0.0
            T[t, p] = keep
    T = np.ascontiguousarray(T, dtype=np.float64)
    return T, max(column_windows(T))


def column_windows(T):
    """The length of the nonzero window [first, last] of every column of T: what create_shaped finds (col_win)."""
    out = []
    for p in range(T.shape[1]):
        nz = np.flatnonzero(T[:, p])
        out.append(int(nz[-1] - nz[0] + 1) if nz.size else 0)
    return out


def draw_beta(rng):
    return 0.0 if rng.random() < 0.5 else float(np.exp(rng.uniform(np.log(0.1), np.log(50.0))))


def draw_weights(rng, E, zero):
    """E weights in 0.5 .. 1.5 and, `zero`, one of them exactly 0 (robust.validate and fleet.validate take it while the sum stays positive)."""
    w = rng.uniform(0.5, 1.5, size=E)
    z = -1
    if zero and E >= 2:
        z = int(rng.integers(0, E))
        w[z] = 0.0
    return w, z


def draw_pulse_regs(rng, with_line):
    reg = {}
    if rng.random() < 0.4:
        reg['amplitude'] = float(rng.uniform(0.05, 0.5))
    if rng.random() < 0.4:
        reg['dwdt'] = float(rng.uniform(0.01, 0.2))
        if rng.random() < 0.5:
            reg['d2wdt2'] = float(rng.uniform(0.01, 0.1))
    if rng.random() < 0.3 and not with_line:                      # (the envelope is defined per time slice: create_shaped refuses it on samples)
        reg['envelope'] = float(rng.uniform(0.05, 0.3))
    return reg


def draw_map(rng, k, r, steps, seed):
    D = int(rng.integers(1, 5))
    mix, fixed = bool(rng.random() < 0.5), bool(rng.random() < 0.5)
    return ref.make_map(k, r, D, steps, mix=mix, fixed=fixed, seed=seed), dict(D=D, M=mix, F=fixed)


def envelope_constant(k, width):
    """one_minus_gauss as the references form it for `width` slices (tests/composed_reference.py: pulse_view)."""
    return pulse_view(k, width, 1.0, {'envelope': 1.0}).one_minus_gauss


class Draw(SimpleNamespace):
    """family, seed, c (the problem), ens (the ensemble: device 0's of a fleet), fleet (or None), cm (or None), ref_map (the map the reference runs:
    cm, or the identity), T (or None), beta, exact, F (0 without a fleet), R, G, xs (G, k, width), info, and expected(): a list of G dicts."""

    def device_of(self, g):
        return g // self.R if self.fleet is not None else 0

    def members_of(self, g):
        """The validated robust dict whose rows control set g runs on."""
        return self.fleet.device(self.device_of(g)) if self.fleet is not None else self.ens

    def evaluate_at(self, g, x, want_grad=True):
        return _EVALUATE[self.family](self, g, x, want_grad)

    def expected(self):
        return _expected(self.family, self.seed)

    def adam_reference(self, g):
        return _adam_reference(self.family, self.seed, g)

    def tag(self):
        return '%s seed %d %s' % (self.family, self.seed, self.info)


def _tables(rng, F, E, k, q, c):
    """(offsets (F, E, q), amp_scales (F, E, k), rate_scales (F, E, c)) in +-0.2, 0.88 .. 1.12 and 0.4 .. 2.5.  The F E rows are STRATIFIED: row (f, e)
    sits at its own position s in (0, 1) -- the members in a random order, the devices interleaved inside every member's stratum -- and every column
    runs along s in a direction of its own, with a small jitter.  Where a pulse is short the members' losses are close to linear in their
    parameters, so that rows drawn independently would often land within 1e-6 of each other; rows in a line do not."""
    perm = rng.permutation(E)
    s = (perm[None, :] + (np.arange(F)[:, None] + rng.uniform(0.25, 0.75, size=(F, E))) / F) / E

    def column(width, half, jitter, centre):
        sign = rng.choice([-1.0, 1.0], size=width)
        return centre + 2.0 * half * sign[None, None, :] * (s[:, :, None] - 0.5) + rng.uniform(-jitter, jitter, size=(F, E, width))
    return column(q, 0.2, 0.005, 0.0), column(k, 0.12, 0.003, 1.0), column(c, 1.05, 0.02, 1.45)


def _members(rng, n, k, E, q, F, zero, risk, sparse_ops=None, decay=None):
    """(ensemble dict, Fleet or None, index of the zero weight): no two devices and no two members share a row (_tables)."""
    ops = sparse_ops if sparse_ops is not None else [0.3 * 2 * np.pi * herm(rng, n) for _ in range(q)]
    w, z = draw_weights(rng, E, zero)
    sparse = sparse_ops is not None
    off, amp, rates = _tables(rng, max(F, 1), E, k, q, 0 if decay is None else len(decay))
    if F == 0:
        if E == 1 and q == 0 and decay is None:
            ens = ref.nominal_ensemble(k)
        else:
            ens = dict(operators=ops, offsets=off[0], amp_scales=amp[0], weights=w, risk=risk)
        if decay is not None:
            ens.update(collapse_ops=decay, rate_scales=rates[0])
        return rb.validate(ens, n, k, sparse=sparse), None, z
    kw = dict(collapse_ops=decay, rate_scales=rates) if decay is not None else {}
    fl = fl_mod.validate(fl_mod.Fleet(ops, off, amp, weights=w, risk=risk, **kw), n, k, sparse=sparse)
    return fl.device(0), fl, z


def _fleet_shape(rng, p_fleet, Fs, Fp, Rs, Rp):
    """(F, R, G): F = 0 and R = G = 1 .. 3 control sets without a fleet."""
    if rng.random() >= p_fleet:
        G = int(rng.integers(1, 4))
        return 0, G, G
    F, R = int(rng.choice(Fs, p=Fp)), int(rng.choice(Rs, p=Rp))
    return F, R, F * R


# ---- the closed dense family ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def closed(seed):
    rng = np.random.default_rng(50_000 + seed)
    unitary = bool(rng.random() < 0.5)
    lossy = (not unitary) and bool(rng.random() < 0.2)
    n = int(rng.choice(CLOSED_N))
    m = int(rng.integers(1, min(n, 8) + 1))
    k = int(rng.integers(1, 4))
    nine = bool(rng.random() < 1.0 / 16)
    with_map = nine or bool(rng.random() < 0.5)
    if nine:
        r = int(rng.integers(6, 9))
        q = 9 - r
    else:
        r = int(rng.integers(1, 5)) if with_map else k
        q = int(rng.integers(0, 4))
    E = int(rng.integers(1, 7))
    if rng.random() < 0.08 and not nine:                          # the nominal ensemble
        E, q = 1, 0
    zero = E >= 2 and bool(rng.random() < 0.15)
    F, R, G = _fleet_shape(rng, 2.0 / 3, (1, 2, 3, 4), (0.1, 0.3, 0.3, 0.3), (1, 2, 3), (0.2, 0.4, 0.4))
    # (long pulses a little more often than short ones: only they give a dense line column windows past 32 and 64 slices)
    allowed = [s for s in CLOSED_STEPS if n <= 40 or s <= 17]
    weight = np.array([3.0 if s >= 65 else 2.0 if s >= 33 else 1.0 for s in allowed])
    steps = int(rng.choice(allowed, p=weight / weight.sum()))
    # a dense line is the only one whose column windows pass 32 and 64 slices: long pulses get one more often
    kind = str(rng.choice(LINES, p=(0.28, 0.18, 0.18, 0.18, 0.18) if steps < 33 else (0.1, 0.1, 0.1, 0.1, 0.6)))
    dt = float(rng.uniform(0.1, 0.3))
    T, window = draw_line(rng, kind, steps, dt * steps)
    beta = draw_beta(rng)
    exact = bool(rng.random() < 0.25)
    regs = draw_pulse_regs(rng, T is not None)
    if rng.random() < 0.4 and n >= 3:
        f = rng.choice(n, size=min(2, n - 1), replace=False)
        regs['forbidden_coeff_list'] = [float(x) for x in rng.uniform(1, 5, size=len(f))]
        regs['states_forbidden_list'] = [int(x) for x in f]
    if rng.random() < 0.3:
        regs['speed_up'] = float(rng.uniform(0.1, 0.8))
    taylor = (int(rng.integers(3, 10)), int(rng.integers(0, 3))) if unitary else (int(rng.integers(4, 11)), 0)
    c = ref.problem(n, r, k, steps, m, state_transfer=not unitary, taylor=taylor, seed=seed, total_time=dt * steps, regs=regs)
    if lossy:
        c['H0'] = c['H0'] - 0.05j * np.diag(np.arange(n) / n)     # (generators no longer anti-Hermitian: the route changes)
    cm, minfo = draw_map(rng, k, r, steps, seed) if with_map else (None, {})
    ens, fleet, z = _members(np.random.default_rng(MEMBER_STREAM['closed'] + seed), n, k, E, q, F, zero, beta)
    width = steps if T is None else T.shape[1]
    xs = rng.normal(0.0, 0.7, size=(G, k, width))
    info = dict(mode='unitary' if unitary else 'state', lossy=lossy, n=n, m=m, k=k, r=r, q=q, E=E, F=F, R=R, G=G, steps=steps, line=kind, P=width,
                window=window, beta=round(beta, 4), exact=exact, map=minfo, zero_weight=z, taylor=taylor, dt=round(dt, 4), regs=sorted(regs),
                mfma_chunks=int(rng.choice(MFMA_CHUNKS)), gemm_chunks=int(rng.choice(GEMM_CHUNKS)), member=int(rng.integers(1, E)) if E > 1 else 0)
    return Draw(family='closed', seed=seed, c=c, ens=ens, fleet=fleet, cm=cm, ref_map=cm if cm is not None else cmap.validate(cmap.identity(k), k=k, r=k, steps=steps),
                T=T, beta=beta, exact=exact, F=F, R=R, G=G, xs=xs, info=info)


def _closed_at(d, g, x, want_grad=True):
    return ref.evaluate(d.c, d.ref_map, d.members_of(g), x, T=d.T, exact=d.exact, beta=d.beta, want_grad=want_grad)


# ---- the open family --------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def opened(seed):
    """Members that decay (include/qoc.h, qoc_create_open_fleet: n <= 32, at most 8 collapse operators, m <= n, pulse regularisers only, the
    first-order gradient, taylor_terms <= 60, scaling <= 12)."""
    from tests import open_fleet_reference as ofr
    rng = np.random.default_rng(60_000 + seed)
    unitary = bool(rng.random() < 0.5)
    n = int(rng.choice(OPEN_N))
    m = int(rng.integers(1, min(n, 3) + 1))
    k = int(rng.integers(1, 4))
    ncol = int(rng.integers(0, 4))
    with_map = bool(rng.random() < 0.5)
    r = int(rng.integers(1, 5)) if with_map else k
    q = int(rng.integers(0, 3))
    E = int(rng.integers(1, 5))
    zero = E >= 2 and bool(rng.random() < 0.15)
    F, R, G = _fleet_shape(rng, 2.0 / 3, (1, 2, 3), (0.2, 0.4, 0.4), (1, 2), (0.4, 0.6))
    steps = int(rng.integers(1, 9))
    kind = str(rng.choice(LINES))
    dt = float(rng.uniform(0.1, 0.3))
    T, window = draw_line(rng, kind, steps, dt * steps)
    beta = draw_beta(rng)
    regs = draw_pulse_regs(rng, T is not None)
    taylor = (int(rng.integers(4, 9)), int(rng.integers(0, 2)))
    p = ofr.problem(n, k, steps, m, ncol, r=r, state_transfer=not unitary, taylor=taylor, seed=seed, regs=regs)
    p['total_time'] = dt * steps
    cm, minfo = draw_map(rng, k, r, steps, seed) if with_map else (None, {})
    ens, fleet, z = _members(np.random.default_rng(MEMBER_STREAM['open'] + seed), n, k, E, q, F, zero, beta, decay=p['collapse_ops'])
    width = steps if T is None else T.shape[1]
    xs = rng.normal(0.0, 0.7, size=(G, k, width))
    info = dict(mode='unitary' if unitary else 'state', n=n, m=m, k=k, r=r, q=q, c=ncol, E=E, F=F, R=R, G=G, steps=steps, line=kind, P=width, window=window,
                beta=round(beta, 4), map=minfo, zero_weight=z, taylor=taylor, dt=round(dt, 4), regs=sorted(regs), member=int(rng.integers(1, E)) if E > 1 else 0)
    return Draw(family='open', seed=seed, c=p, ens=ens, fleet=fleet, cm=cm, ref_map=cm, T=T, beta=beta, exact=False, F=F, R=R, G=G, xs=xs, info=info)


def _open_at(d, g, x, want_grad=True):
    from tests import open_fleet_reference as ofr
    return ofr.evaluate(d.c, d.cm, d.members_of(g), x, T=d.T, beta=d.beta, want_grad=want_grad)


# ---- the sparse family ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sparse(seed):
    """Sparse state transfer through the ensemble funnel (qoc_create_sparse_fleet).  A line reaches sparse operators through the C entry point alone
    (tests/test_sparse_ensemble_gpu.py: line_engine, which takes no fleet and no regulariser), so a draw with a line has neither."""
    from tests import sparse_ensemble_reference as ser
    from tests import sparse_reference as sr
    rng = np.random.default_rng(70_000 + seed)
    n = int(rng.choice(SPARSE_N))
    m = int(rng.integers(1, 4))
    k = int(rng.integers(1, 4))
    with_map = bool(rng.random() < 0.5)
    r = int(rng.integers(1, 5)) if with_map else k
    q = int(rng.integers(0, 3))
    E = int(rng.integers(1, 5))
    zero = E >= 2 and bool(rng.random() < 0.15)
    kind = str(rng.choice(LINES, p=(0.6, 0.1, 0.1, 0.1, 0.1)))
    F, R, G = _fleet_shape(rng, 0.0 if kind != 'none' else 0.75, (1, 2, 3), (0.2, 0.4, 0.4), (1, 2), (0.4, 0.6))
    steps = int(rng.integers(1, 13))
    dt = float(rng.uniform(0.1, 0.3))
    T, window = draw_line(rng, kind, steps, dt * steps)
    beta = draw_beta(rng)
    regs = {}
    if T is None:
        regs = draw_pulse_regs(rng, False)
        if rng.random() < 0.3:
            regs['speed_up'] = float(rng.uniform(0.1, 0.8))
    forbidden = T is None and bool(rng.random() < 0.4)
    taylor = int(rng.integers(4, 11))
    sp = sr.sparse_case(n, steps, k=r, m=m, T=taylor, seed=seed, reg_coeffs=regs, forbidden=forbidden)
    p = ser.Problem(sp.H0_in, sp.Hops_in, sp.V, sp.W, dt * steps, steps, taylor, rng.uniform(0.8, 1.6, size=k), sp.reg_coeffs)
    cm, minfo = draw_map(rng, k, r, steps, seed) if with_map else (None, {})
    mrng = np.random.default_rng(MEMBER_STREAM['sparse'] + seed)
    ops = [0.5 * sr.random_sparse(mrng, n, (1, 3)) for _ in range(q)]
    ens, fleet, z = _members(mrng, n, k, E, q, F, zero, beta, sparse_ops=ops)
    width = steps if T is None else T.shape[1]
    xs = rng.normal(0.0, 0.6, size=(G, k, width))
    info = dict(n=n, m=m, k=k, r=r, q=q, E=E, F=F, R=R, G=G, steps=steps, line=kind, P=width, window=window, beta=round(beta, 4), map=minfo, zero_weight=z,
                taylor=taylor, dt=round(dt, 4), regs=sorted(p.reg_coeffs), vector_home=str(rng.choice(['lds', 'global'])), row_layout=int(rng.choice([1, 2])))
    return Draw(family='sparse', seed=seed, c=p, ens=ens, fleet=fleet, cm=cm, ref_map=cm, T=T, beta=beta, exact=False, F=F, R=R, G=G, xs=xs, info=info)


def _sparse_at(d, g, x, want_grad=True):
    from tests import sparse_ensemble_reference as ser
    return ser.evaluate(d.c, d.members_of(g), x, cm=d.cm, T=d.T, beta=d.beta)


# ---- expected values --------------------------------------------------------------------------------------------------------------------------------

FAMILIES = {'closed': (closed, CLOSED_SEEDS), 'open': (opened, OPEN_SEEDS), 'sparse': (sparse, SPARSE_SEEDS)}
_EVALUATE = {'closed': _closed_at, 'open': _open_at, 'sparse': _sparse_at}


@functools.lru_cache(maxsize=None)
def _expected(family, seed):
    """The reference of every control set at its start point, with member_unitary_scale (the members' own figures, which the composed references
    return only as their weighted sum) in place of the members' trajectories: computed once, shared by every test and engine."""
    d = FAMILIES[family][0](seed)
    out = []
    for g in range(d.G):
        o = d.evaluate_at(g, d.xs[g])
        o['member_unitary_scale'] = np.array([float(r['unitary_scale']) for r in o.pop('members')])
        out.append(o)
    return out


@functools.lru_cache(maxsize=None)
def _adam_reference(family, seed, g):
    """Four iterations of the device loop's semantics from control set g's start point (composed_reference.run_adam): dict(base, loss, reg_loss, ..)."""
    d = FAMILIES[family][0](seed)
    return run_adam(lambda x: d.evaluate_at(g, x), d.xs[g], ADAM)


# ---- which kernel family takes a closed draw --------------------------------------------------------------------------------------------------------

def antihermitian(d):
    """Exactly anti-Hermitian generators -i dt H: a Hermitian drift (the controls and the perturbations always are)."""
    return not d.info['lossy']


def eligible(d, path):
    """Whether `path` ('auto', 'generic', 'mfma', 'gemm', 'st_fused') takes the closed draw d, from the limits include/qoc.h documents:
      * the exact gradient runs on the generic path (AUTO resolves to it), on no other;
      * MFMA: n <= 64, m <= 16, at most 8 trajectory controls (r + q: qoc_create_ensemble), and in state transfer exactly anti-Hermitian generators;
      * ST_FUSED: state transfer, n <= 64, m <= 4, at most 8 trajectory controls;
      * GEMM: any n, m <= 32, both modes; state transfer by propagators (chunks > 1: anti-Hermitian generators only) or directly (n <= 64, m <= 8: what
        a lossy drift needs, whatever the chunk count asked for is otherwise)."""
    i = d.info
    if path in ('auto', 'generic'):
        return True
    if d.exact:
        return False
    st, controls = i['mode'] == 'state', i['r'] + i['q']
    if path == 'mfma':
        return i['n'] <= 64 and i['m'] <= 16 and controls <= 8 and (not st or antihermitian(d))
    if path == 'st_fused':
        return st and i['n'] <= 64 and i['m'] <= 4 and controls <= 8
    if path == 'gemm':
        if not st or antihermitian(d):
            return i['m'] <= 32
        return i['n'] <= 64 and i['m'] <= 8 and i['gemm_chunks'] <= 1
    raise ValueError(path)
