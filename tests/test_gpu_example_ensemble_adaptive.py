"""examples/DecayingTurbulenceEnsembleAdaptive2D.py end to end on the GPU at 64², B = 4: `solve_unsteady_ensemble(Δt=None)`, the ensemble-mean energy, max
divergence and mean spectrum through `ensemble_stats` / `observespectrum_ensemble`."""
import numpy as np
import pytest

from tests.test_gpu_example_ensemble import load

pytestmark = pytest.mark.gpu


def test_decaying_turbulence_ensemble_adaptive_2d():
    import torch

    r = load("DecayingTurbulenceEnsembleAdaptive2D").main(n=64, B=4, tend=0.06, n_adapt=2, nupdate=3, kp=4, verbose=False)  # about ten steps
    E = [e for _, e in r["energy"]]
    assert len(r["E"]) == 4 and r["t"] == pytest.approx(0.06) and len(r["Δts"]) >= 5 and len(E) >= 3
    assert np.isfinite(E).all() and np.isfinite(r["E"]).all() and np.isfinite(r["ehat"]).all() and bool(torch.isfinite(r["U"]).all())
    assert all(b < a for a, b in zip(E, E[1:]))  # the ensemble-mean energy decays
    assert r["maxdiv"] < 1e-10  # the bound of tests/test_gpu_example_ensemble.py
    assert all(dt > 0 for dt in r["Δts"]) and sum(r["Δts"]) == pytest.approx(0.06)
    assert not torch.equal(r["U"][0], r["U"][1])
    assert r["ehat"].shape == r["ehat0"].shape and abs(int(r["κ"][np.argmax(r["ehat0"])]) - 4) <= 2
