"""bench.py on one GPU as its callers run it, on small boxes (the numbers mean nothing here): a plain run prints the headline and nothing else,
`--dump-outputs` writes what the timed path returned after its last step — checked against the same warm-up and timed steps run here through the
API —, and `--full` adds the extra measurements without changing what the timed path computes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, STEPS, DT = 2, 3, 1e-3


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def run_bench(n, out_dir, *extra):
    env = dict(os.environ, INS_BENCH_SKIP_K1_512="1", INS_BENCH_SKIP_STRONG_512="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--n", str(n),
           "--dump-outputs", str(out_dir), *extra]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def timed_path_here(ins, n):
    """The bench's set-up, warm-up and timed steps, in this process."""
    from bench import tgv3d

    setup = ins.Setup(x=(np.linspace(0.0, 1.0, n + 1),) * 3, Re=1000.0, device="cuda:0")
    ps = ins.psolver_spectral(setup)
    method = ins.RKMethods.RK44()
    cache = ins.ode_method_cache(method, setup, ps)
    st = ins.create_stepper(method, setup=setup, psolver=ps, u=ins.velocityfield(setup, tgv3d, 0.0, psolver=ps), t=0.0)
    st = ins.timesteps_(method, st, DT, WARMUP, cache=cache)
    return ins.timesteps_(method, st, DT, STEPS, cache=cache)


@pytest.mark.parametrize("n", [32, 128])  # 32^3: the whole field is written; 128^3: more than DUMP_VALUES values, a fixed sample
def test_plain_run_dump_and_full(ins, n, tmp_path):
    from bench import DUMP_VALUES

    plain = run_bench(n, tmp_path / "plain")
    assert plain["steps"] == STEPS and plain["warmup"] == WARMUP and plain["n_gpus"] == 1 and plain["config"]["grid"] == [n, n, n]
    assert plain["ms_per_step"] > 0 and plain["value"] > 0 and plain["higher_is_better"] is True and plain["dtype"] == "f64"
    assert not {"roofline", "roofline_k1", "ms_per_step_single_calls", "check", "strong_512", "cpu_baseline"} & set(plain)

    full = run_bench(n, tmp_path / "full", "--full", "--no-cpu-baseline")
    assert full["steps"] == STEPS and full["ms_per_step"] > 0 and full["roofline"]["launches"] > 0 and full["roofline_k1"]["avg_launch_ms"] > 0
    assert full["ms_per_step_single_calls"] > 0 and full["check"]["max_abs_div_times_dx"] < 1e-10

    st = timed_path_here(ins, n)
    u = st.u
    if u.numel() <= DUMP_VALUES:
        want = ins.to_numpy(u).ravel(order="F")
    else:
        flat = np.unique(np.random.default_rng(0).integers(0, u.numel(), DUMP_VALUES))
        want = ins.to_numpy(u).ravel(order="F")[flat]
    scale = float(np.max(np.abs(want)))
    for run in ("plain", "full"):
        got = np.load(tmp_path / run / "u.npy")
        t = np.load(tmp_path / run / "t.npy")
        assert got.dtype == np.float64 and got.shape == want.shape and got.nbytes <= 64 << 20
        assert float(np.max(np.abs(got - want))) <= 1e-13 * scale, run
        assert t.dtype == np.float64 and t.shape == (1,) and abs(t[0] - st.t) < 1e-15
