"""examples/qubit_pi_pulse_under_noise.py at a small budget: it runs, every figure is finite, and on the TRAINING traces the trace pulse's mean
infidelity lies below the nominal pulse's -- the optimiser minimises exactly that number, starting from the nominal pulse.  Whether the trace pulse
wins on held-out noise is a measurement (profiles/noise_traces.txt), not an assertion: the held-out figures are printed."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs_and_the_trace_pulse_wins_on_its_training_traces():
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import qubit_pi_pulse_under_noise as ex
    with contextlib.redirect_stdout(io.StringIO()) as out:
        figures = ex.main(iterations=60, members=8, heldout=16, quiet=True)
    held_nominal, held_static, held_traces, train_nominal, train_traces = figures
    print('held-out: nominal %.3e quasi-static %.3e traces %.3e; training: nominal %.3e traces %.3e' % figures)
    assert len(figures) == 5 and all(np.isfinite(f) for f in figures)
    assert train_traces < train_nominal, (train_traces, train_nominal)
    assert 'held-out mean infidelity over 16 fresh traces' in out.getvalue() and 'Robust ensemble: 8 members' in out.getvalue()
