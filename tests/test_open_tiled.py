"""The tiled open-system path without a GPU: the path number, open_system.choose_path either side of every threshold, and the condition on the inputs
of tests/test_open_tiled_gpu.py -- the near-target rows have a gradient well above assert_gradient's floor and a loss that the dissipator moves, so
they cannot pass with the dissipator dropped or the gradient zeroed."""
import numpy as np
import pytest

from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import open_system
from tests import open_tiled_cases as tc


def test_the_path_number():
    assert hip_engine.PATH_LINDBLAD_TILED == 8 and hip_engine.PATH_LINDBLAD == 6
    assert (open_system.PATH_LINDBLAD, open_system.PATH_LINDBLAD_TILED) == (hip_engine.PATH_LINDBLAD, hip_engine.PATH_LINDBLAD_TILED)


@pytest.mark.parametrize('n, c, path', [(32, 5, 6), (32, 6, 8), (24, 8, 6), (31, 8, 8), (33, 0, 8), (128, 8, 8), (1, 0, 6), (4, 2, 6)])
def test_choose_path_either_side_of_every_threshold(n, c, path):
    assert open_system.choose_path(n, c) == path


def test_choose_path_names_both_limits_past_128_levels():
    with pytest.raises(ValueError) as err:
        open_system.choose_path(129, 0)
    text = str(err.value)
    assert 'n = 129' in text and '32 levels' in text and '128 levels' in text, text


def test_choose_path_restates_the_lds_rule():
    """The rule of csrc/qoc_lindblad.h, (c + 4) n (n | 1) 16 bytes <= 159 KiB with n <= 32: the largest c per n, by the rule written out again."""
    for n in range(1, 33):
        for c in range(0, 9):
            fits = (c + 4) * n * (n + 1 - n % 2) * 16 <= 162816
            assert open_system.choose_path(n, c) == (6 if fits else 8), (n, c)


@pytest.mark.parametrize('name', tc.NEAR)
def test_near_rows_see_the_dissipator_and_have_a_gradient(name):
    refs, closed = tc.reference(name), tc.closed_reference(name)
    for b in (0, 1):
        gmax = float(np.max(np.abs(refs[b]['grad'])))
        gap = abs(refs[b]['loss'] - closed[b]['loss'])
        print('%s base %d: loss %.4f, closed loss %.4f, largest gradient entry %.3e' % (name, b, refs[b]['loss'], closed[b]['loss'], gmax))
        assert gmax >= 1e-2, (name, b, gmax)
        assert gap >= 0.05, (name, b, gap)
