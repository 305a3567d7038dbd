"""bench.py --dump-outputs on the HIP path: config 1 (the image tower's no-grad forward) writes its embeddings, the same bits from run to
run.  (The training configs: tests/test_bench_cpu.py.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_forward_config_dumps_the_same_embeddings_every_run(tmp_path):
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "1", "--layers", "2", "--batch", "4",
                            "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-profile", "--no-power-probe", "--dump-outputs", str(d)],
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    assert sorted(os.listdir(dirs[0])) == ["image_embeddings.npy"]
    a, b = np.load(dirs[0] / "image_embeddings.npy"), np.load(dirs[1] / "image_embeddings.npy")
    assert a.dtype == np.float32 and a.shape == (4 * 1536,) and np.isfinite(a).all()
    assert np.allclose(np.linalg.norm(a.reshape(4, 1536), axis=1), 1.0, atol=1e-2)  # L2-normalised embeddings
    assert np.array_equal(a, b)
