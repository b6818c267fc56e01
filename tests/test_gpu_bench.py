"""A plain ``bench.py`` run on the GPU: exactly ``--steps`` timed steps, none of the ``--full`` legs, and ``--dump-outputs``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT, capture_output=True,
                          text=True, timeout=600)


def test_plain_run_times_the_given_steps_and_dumps_the_same_outputs_twice(tmp_path):
    """``bench.py --steps K --dump-outputs DIR`` without ``--full``: the line reports exactly K timed steps and none of the
    ``--full`` legs, and two runs with the same arguments write the same arrays (seeded corpus, model and batch order)."""
    got = []
    for k in range(2):
        out_dir = tmp_path / f"run{k}"
        out = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "32", "--dump-outputs", str(out_dir)])
        assert out.returncode == 0, out.stderr[-2000:]
        rec = json.loads(out.stdout.strip().splitlines()[-1])
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["unit"] == "circuits/s"
        assert not set(rec) & {"roofline", "cpu_baseline", "parity", "host_enqueue_ms_per_step", "full_record"}
        arrays = {name: np.load(out_dir / f"{name}.npy") for name in ("loss", "params", "grad")}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
        assert arrays["params"].shape == arrays["grad"].shape == (rec["config"]["gradient_floats_all_reduced"],)
        assert abs(float(arrays["loss"].reshape(-1)[0]) - rec["final_loss"]) < 1e-5
        got.append(arrays)
    for name in ("loss", "params", "grad"):
        np.testing.assert_allclose(got[0][name], got[1][name], rtol=1e-5, atol=1e-7, err_msg=name)
