"""GPU: the opt-in keywords of the gradient examples: `rollout=True` of examples/RayleighBenardGradient2D.py (one `ad.timesteps` / `ad32.timesteps`
call instead of a loop of `timestep` calls) and `dtype=torch.float32` of examples/TaylorGreenGradient3D.py.

Bounds.  fp64 rollout against the step-by-step run of the same example: TOL = 1e-12 of tests/test_gpu_adjoint.py, what `ad.timesteps` meets against
chained `ad.timestep` calls (the same kernels, another summation order).  Float32 Rayleigh-Benard rollout: the rule of
tests/test_gpu_ad32_timesteps.py item 2, its error against the fp64 gradient is at most MARGIN (4, tests/test_gpu_adjoint32.py) times that of the
example's step-by-step Float32 run.  Float32 Taylor-Green (it has no step-by-step form): MARGIN x 2^-24 per stage and step against fp64, i.e.
4 x 6e-8 x 4 x 8 = 8e-6.  The examples' central differences are printed, not asserted, in Float32.
"""
import importlib.util
import os
import sys

import pytest

from tests.test_gpu_adjoint import TOL
from tests.test_gpu_adjoint32 import MARGIN

pytestmark = pytest.mark.gpu
EXAMPLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def example(name):
    sys.path.insert(0, EXAMPLES)
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(EXAMPLES, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(EXAMPLES)
    return mod


def rel(a, b):
    return float((a.double() - b.double()).norm()) / float(b.double().norm())


def test_rayleigh_benard_gradient_through_one_rollout(ins):
    import torch

    ex = example("RayleighBenardGradient2D")
    kw = dict(n=16, nstep=5, dt=5e-3, verbose=False)
    steps = ex.main(**kw)
    roll = ex.main(rollout=True, checkpoint_every=2, **kw)
    r = rel(roll["grad"], steps["grad"])
    print(f"RayleighBenardGradient2D rollout against step by step: rel = {r:.3e}; Nu {roll['Nu']!r} / {steps['Nu']!r}")
    assert float(steps["grad"].norm()) > 0 and r <= TOL and abs(roll["Nu"] - steps["Nu"]) <= TOL * abs(steps["Nu"])
    steps32 = ex.main(dtype=torch.float32, **kw)
    roll32 = ex.main(rollout=True, checkpoint_every=2, dtype=torch.float32, **kw)
    e_native, e_unrolled = rel(roll32["grad"], steps["grad"]), rel(steps32["grad"], steps["grad"])
    print(f"RayleighBenardGradient2D Float32 against fp64: e_native = {e_native:.3e}, e_unrolled = {e_unrolled:.3e}; dJ {roll32['dJ']:.6e}, "
          f"fd {roll32['fd']:.6e}")
    assert roll32["grad"].dtype == torch.float32 and e_native <= MARGIN * e_unrolled


def test_taylor_green_gradient_float32(ins):
    import torch

    ex = example("TaylorGreenGradient3D")
    kw = dict(n=32, nsteps=8, dt=1e-3, verbose=False)
    r64 = ex.main(**kw)
    r32 = ex.main(dtype=torch.float32, **kw)
    r = rel(r32["grad"], r64["grad"])
    bound = MARGIN * 2.0**-24 * 4 * kw["nsteps"]
    print(f"TaylorGreenGradient3D Float32 against fp64: rel = {r:.3e} (bound {bound:.1e}); dJ {r32['dJ']:.6e}, fd {r32['fd']:.6e}, "
          f"rel fd {r32['rel']:.2e} (example's tolerance {r32['tol']:.0e})")
    assert r32["grad"].dtype == torch.float32 and r64["rel"] <= r64["tol"]
    assert r <= bound
