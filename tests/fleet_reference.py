"""The expected values of a fleet engine, by picking rows.

Control set g of a fleet with R control sets per device belongs to device g // R, and every quantity of it is what the ensemble engine defines for an
ensemble with that device's rows.  So device f's expectation is the expectation of ONE ensemble -- Fleet.device(f) -- from the modules that already
compose it from the unchanged oracle: tests/robust_reference.py (composed: the weighted mean of the members' oracle evaluations) and
tests/control_map_reference.py (evaluate: the same with a line, a control map, a risk and the exact gradient).  Nothing is computed here."""
import numpy as np

from quantum_optimal_control.helper_functions import fleet as fl_mod
from quantum_optimal_control.helper_functions.synthetic_systems import herm
from tests import control_map_reference as ref
from tests import robust_reference as rr

REGS_UNITARY = {'dwdt': 0.1, 'amplitude': 0.2}
REGS_STATE = {'dwdt': 0.1, 'forbidden_coeff_list': [5.0], 'states_forbidden_list': [4], 'speed_up': 0.3}


def problem(kind, n=None, k=2, r=None, steps=None, m=None, regs=None, seed=0):
    """tests/control_map_reference.py: problem, with the keys tests/robust_reference.py: member_systems reads.  unitary: n = 4, steps = 8, m = 3;
    state: n = 5, m = 2, steps = 7, a forbidden level and speed_up."""
    st = kind == 'state'
    n, steps, m = n or (5 if st else 4), steps or (7 if st else 8), m or (2 if st else 3)
    c = ref.problem(n, k if r is None else r, k, steps, m, state_transfer=st, taylor=(8, 0) if st else (6, 1), seed=70 + seed,
                    regs=(REGS_STATE if st else REGS_UNITARY) if regs is None else regs)
    return dict(c, dressed_info=None, initial_guess=None, Hnames=['p%d' % j for j in range(k)])


def make_fleet(c, F, E, q, seed=5, risk=0.0):
    """F devices of E members and q perturbations: every row distinct (devices differ in their offsets AND in their scales), random weights."""
    rng = np.random.default_rng(seed + 100 * F + 10 * E + q)
    n, k = len(c['H0']), len(c['maxA'])
    ops = [0.3 * 2 * np.pi * herm(rng, n) for _ in range(q)]
    off = rng.uniform(-0.2, 0.2, size=(F, E, q))
    amp = rng.uniform(0.9, 1.1, size=(F, E, k)) + 0.05 * np.arange(F)[:, None, None]
    w = rng.uniform(0.5, 1.5, size=E) if E > 1 else None
    return fl_mod.validate(fl_mod.Fleet(ops, off, amp, weights=w, risk=risk), n, k)


def device(fl, f):
    """Device f as the validated robust dict an ensemble engine takes (the fleet's weights are normalised already)."""
    return fl.device(f)


def member_systems(c, fl, f):
    """tests/robust_reference.py: member_systems of device f, with the problem's (T, s)."""
    return rr.member_systems(c, device(fl, f), c['Taylor_terms'])


def composed(c, fl, f, base):
    """tests/robust_reference.py: composed, with device f's rows."""
    return rr.composed(member_systems(c, fl, f), fl.weights, base)


def evaluate(c, cm, fl, f, x, T=None, exact=False):
    """tests/control_map_reference.py: evaluate, with device f's rows and the fleet's risk."""
    return ref.evaluate(c, cm, device(fl, f), x, T=T, exact=exact, beta=float(fl.risk))


def control_sets(F, R):
    """(device, restart) of every control set, device-major."""
    return [(g // R, g % R) for g in range(F * R)]


def swapped_apart(values, floor=1e-6):
    """True when the expectations `values[f]` (scalars or arrays, one per device) of any two devices differ by more than `floor`: a kernel that
    reads another device's rows cannot pass."""
    vals = [np.asarray(v, dtype=np.float64) for v in values]
    return all(np.max(np.abs(vals[a] - vals[b])) > floor for a in range(len(vals)) for b in range(a + 1, len(vals)))
