"""GPU: examples/TaylorGreenGradient3D.py at 32^3 with 8 steps — the gradient of the final kinetic energy through `ad.timesteps` passes the example's own
finite-difference check."""
import importlib.util
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

EXAMPLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")


def test_taylor_green_gradient_example():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, EXAMPLES)
    try:
        spec = importlib.util.spec_from_file_location("TaylorGreenGradient3D", os.path.join(EXAMPLES, "TaylorGreenGradient3D.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        r = mod.main(n=32, nsteps=8, verbose=True)
    finally:
        sys.path.remove(EXAMPLES)
    assert r["gnorm"] > 0 and r["dJ"] != 0
    assert abs(r["E"] - r["E_native"]) <= 1e-12 * abs(r["E_native"]), (r["E"], r["E_native"])
    assert r["rel"] <= r["tol"] == 1e-6, (r["dJ"], r["fd"], r["rel"])
    assert r["grad"].shape == (34, 34, 34, 3)
