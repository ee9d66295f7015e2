"""examples/DecayingTurbulenceEnsemble2D.py end to end on the GPU at 32², B = 4: one native ensemble call between observations, the ensemble-mean
spectrum through `observespectrum` on the members."""
import importlib.util
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EX = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")


def load(name):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, EX)
    spec = importlib.util.spec_from_file_location(name, os.path.join(EX, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_decaying_turbulence_ensemble_2d():
    import torch

    r = load("DecayingTurbulenceEnsemble2D").main(n=32, B=4, tend=0.04, dt=1e-3, nobs=2, kp=4, verbose=False)
    E = [e for _, e in r["energy"]]
    assert len(r["E"]) == 4 and r["t"] == pytest.approx(0.04) and r["maxdiv"] < 1e-10
    assert all(b < a for a, b in zip(E, E[1:]))  # every member decays, so does the mean
    assert all(e1 < e0 for e0, e1 in zip(r["E0"], r["E"]))
    assert not torch.equal(r["U"][0], r["U"][1])  # different initial conditions stay different flows
    assert r["ehat"].shape == r["ehat0"].shape and np.isfinite(r["ehat"]).all() and abs(int(r["κ"][np.argmax(r["ehat0"])]) - 4) <= 2
