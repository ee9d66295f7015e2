"""examples/NeuralClosurePost2D.py end to end on the GPU at ndns 64, nles 32, B = 4, nunroll 3: ensemble data generation, a few Adam iterations through
`create_loss_post_ensemble`; the a-posteriori loss on a fixed batch is finite and goes down."""
import numpy as np
import pytest

from tests.test_gpu_example_ensemble import load

pytestmark = pytest.mark.gpu


def test_neural_closure_post_2d():
    r = load("NeuralClosurePost2D").main(ndns=64, nles=32, B=4, tburn=0.01, tsim=0.012, dt=1e-3, savefreq=2, nunroll=3, niter=6, lr=1e-3, seed=0)
    print(f"a-posteriori loss {r['loss_before']:.6e} -> {r['loss_after']:.6e}; history {r['history']}")
    assert r["ntrajectory"] == 4 and r["nstate"] == 7 and len(r["history"]) == 6
    assert np.isfinite(r["loss_before"]) and np.isfinite(r["history"]).all()
    assert r["loss_after"] < r["loss_before"]
