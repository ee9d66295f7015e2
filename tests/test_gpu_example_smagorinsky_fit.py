"""GPU: examples/SmagorinskyFit3D.py as it stands (16^3 periodic, RK44, 10 steps, 6 Adam steps on θ): the loss falls and θ moves towards the
target's constant."""
import importlib.util
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

EXAMPLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")


def test_smagorinsky_fit_example():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, EXAMPLES)
    try:
        spec = importlib.util.spec_from_file_location("SmagorinskyFit3D", os.path.join(EXAMPLES, "SmagorinskyFit3D.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        r = mod.main(verbose=True)
    finally:
        sys.path.remove(EXAMPLES)
    losses, thetas = r["losses"], r["thetas"]
    assert len(losses) == 7 and all(np_isfinite(x) for x in losses)
    assert losses[0] > 0 and losses[-1] < losses[0], losses
    assert abs(thetas[-1] - r["theta_target"]) < abs(thetas[0] - r["theta_target"]), thetas


def np_isfinite(x):
    return x == x and abs(x) != float("inf")
