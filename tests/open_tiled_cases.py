"""The problems of tests/test_open_tiled.py and tests/test_open_tiled_gpu.py (TEST INFRASTRUCTURE ONLY): the rows of the tiled open-system path
(QOC_PATH_LINDBLAD_TILED, csrc/qoc_lindblad_tiled.h), the smallest shapes at which each of its pieces can go wrong, with their references computed
once and shared.

open_case's targets are random: above 32 levels they give a loss near 1 and gradients of a few 1e-4, under the floor of assert_gradient.  near_case
keeps open_case's Hamiltonians, start vectors and collapse operators (state-transfer mode) and takes as targets the CLOSED propagation of the start
vectors under the pulse of bases_of(sp)[2]: at bases 0 and 1 the pulse is another one and the decay is on, so the loss is neither 0 nor 1 and the
gradient is of order 1e-2 and above (tests/test_open_tiled.py asserts both on every near row)."""
import functools

import numpy as np
from scipy.linalg import expm

from tests import lindblad_reference as lr
from tests.test_open_system import bases_of, open_case


def near_case(n, k, m, steps, taylor, c, seed):
    """(OracleSystem, collapse operators) in state-transfer mode with W = the exact closed propagation of V under the pulse of bases_of(sp)[2]."""
    sp, ops = open_case(n, k, m, steps, taylor, c, seed, state_transfer=True)
    u = sp.maxA[:, None] * np.sin(bases_of(sp)[2])
    psi = np.array(sp.V)
    for t in range(steps):
        psi = expm(sp.Hs[0] + np.tensordot(u[:, t], sp.Hs[1:], axes=1)) @ psi
    sp.W = np.ascontiguousarray(psi)
    return sp, ops


# name: (near, n, k, m, steps, (T, s), c) -- and what the row exercises
ROWS = {
    'n3': (False, 3, 1, 2, 5, (4, 0), 1),              # far inside one tile
    'n16': (False, 16, 2, 2, 3, (5, 1), 2),            # exactly one tile
    'n17': (False, 17, 2, 3, 3, (5, 1), 2),            # ragged second tile, six pairs
    'n32_c6': (False, 32, 2, 2, 3, (5, 1), 6),         # what the LDS rule refuses
    'near33': (True, 33, 2, 2, 3, (5, 1), 2),          # first size past the limit
    'n33_s2': (False, 33, 1, 2, 2, (6, 2), 1),         # four sub-steps
    'near48': (True, 48, 4, 3, 3, (5, 1), 5),          # three exact tiles
    'near65': (True, 65, 2, 2, 3, (5, 1), 2),          # 25 tiles on 4 waves
    'n128': (False, 128, 2, 1, 2, (4, 0), 1),          # the limit, a single pair
}
NEAR = [name for name in ROWS if ROWS[name][0]]
BOTH_PATHS = [name for name in ROWS if ROWS[name][1] <= 17]      # the rows the LDS path runs too


@functools.lru_cache(maxsize=None)
def system(name):
    near, n, k, m, steps, taylor, c = ROWS[name]
    # (near rows: one seed at which the condition on the inputs holds with a margin at all three sizes -- largest gradient entry 2.7e-2 and above,
    # the dissipator worth 0.17 of loss and above; about one seed in six gives an entry under 1e-2 at base 0 and is no use here)
    if near:
        return near_case(n, k, m, steps, taylor, c, 202)
    return open_case(n, k, m, steps, taylor, c, 200 + list(ROWS).index(name))


@functools.lru_cache(maxsize=None)
def reference(name):
    """lindblad_reference.evaluate at the row's three bases: computed once, shared by every test that needs it, never changed."""
    sp, ops = system(name)
    return [lr.evaluate(sp, ops, b) for b in bases_of(sp)]


@functools.lru_cache(maxsize=None)
def closed_reference(name):
    """The same without collapse operators, bases 0 and 1 (the loss only)."""
    sp, _ = system(name)
    return [lr.evaluate(sp, [], b, want_grad=False) for b in bases_of(sp)[:2]]
