"""bench.py's command line on CPU (`--debug-cpu-micro`: 2-layer H=128 model, torch path): `--steps` is the number of timed steps, and
`--dump-outputs DIR` writes what the last timed step computed, the same arrays from run to run."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    env = dict(os.environ, OMP_NUM_THREADS="2", HIP_VISIBLE_DEVICES="-1")  # CPU run on a GPU host too (ordinal -1 hides every device)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--debug-cpu-micro", "--gpus", "1", *args], cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)


def test_steps_sets_the_number_of_timed_steps():
    r = _bench("--steps", "3", "--warmup", "1", "--loss-curve")
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["steps"] == 3 and len(out["config"]["loss_curve"]) == 3
    r = _bench("--steps", "0")
    assert r.returncode != 0 and "--steps" in r.stderr


def test_dump_outputs_are_the_last_step_and_repeat_exactly(tmp_path):
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        r = _bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(d))
        assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    names = sorted(os.listdir(dirs[0]))
    assert names == ["grads.npy", "loss.npy", "params.npy"] and sorted(os.listdir(dirs[1])) == names
    assert sum(os.path.getsize(dirs[0] / n) for n in names) <= 64 << 20
    for n in names:
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        assert np.array_equal(a, b), "%s differs between two runs with the same arguments" % n
    loss = np.load(dirs[0] / "loss.npy")
    assert loss.shape == (1,) and abs(float(loss[0]) - out["config"]["final_loss"]) <= 1e-6 * abs(out["config"]["final_loss"])
    grads = np.load(dirs[0] / "grads.npy")
    assert grads.shape == np.load(dirs[0] / "params.npy").shape and np.abs(grads).sum() > 0


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("onepeace_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_sample_takes_distinct_fixed_positions():
    import torch
    B = _bench_module()
    k = B.DUMP_SAMPLE
    big = torch.arange(3 * k + 5, dtype=torch.float64)  # value = position
    cache = {}
    a = B.dump_sample(big, cache)
    assert a.dtype == np.float32 and a.shape == (k,)
    pos = a.astype(np.int64)
    assert (np.diff(pos) == 3).all() and 0 <= pos[0] < 3  # distinct, every third from an offset in the first stride
    assert np.array_equal(B.dump_sample(-big, cache), -a) and np.array_equal(B.dump_sample(big, {}), a)  # same positions every time
    small = torch.randn(6, 5, dtype=torch.bfloat16)
    assert np.array_equal(B.dump_sample(small, cache), small.float().reshape(-1).numpy())  # whole when small


def test_forward_config_dumps_the_image_embeddings():
    import torch
    B = _bench_module()
    emb = torch.nn.functional.normalize(torch.randn(4, 1536), dim=-1).to(torch.bfloat16)
    out = B.step_outputs(False, emb, None)
    assert list(out) == ["image_embeddings"] and np.array_equal(out["image_embeddings"], emb.float().reshape(-1).numpy())
