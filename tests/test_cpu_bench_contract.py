"""-m 'not gpu': bench.py's launch contract that can be checked without a device: `--gpus N` from a plain invocation must
refuse to run when fewer than N devices answer (it never silently falls back to one rank), a WORLD_SIZE that disagrees with
--gpus is an error, and the N>1 clip sharding + weight-broadcast helpers work over gloo with two ranks."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=e, timeout=300)


def test_gpus_n_refuses_when_fewer_devices_answer():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert "--gpus 2 but only 0 device(s) answer" in (r.stderr + r.stdout)


def test_world_size_must_match_gpus():
    r = _run(["--gpus", "1", "--steps", "1", "--warmup", "0"], env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1",
                                                                     "MASTER_PORT": "29999", "EW_BENCH_SKIP_INIT": "1"})
    assert r.returncode != 0
    assert "--gpus 1 but WORLD_SIZE=2" in (r.stderr + r.stdout)


def test_full_and_dump_outputs_options():
    r = _run(["--help"])
    assert r.returncode == 0
    assert "--full" in r.stdout and "--dump-outputs DIR" in r.stdout


def test_dump_outputs_writes_float32_within_the_cap(tmp_path):
    """bench.dump_outputs: small arrays land whole; past the byte cap every array becomes the same seeded sample from call to
    call, its share of the cap proportional to its size."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    a, b = torch.randn(3, 5, dtype=torch.float16), torch.arange(7, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "whole"), {"a": a, "b": b})
    x = np.load(tmp_path / "whole" / "a.npy")
    assert x.dtype == np.float32 and x.shape == (3, 5) and np.array_equal(x, a.float().numpy())
    assert np.array_equal(np.load(tmp_path / "whole" / "b.npy"), np.arange(7, dtype=np.float32))
    big, small = torch.randn(3000), torch.randn(1000)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small}, max_bytes=4 * 400)
    s1 = {n: np.load(tmp_path / "s1" / f"{n}.npy") for n in ("big", "small")}
    assert s1["big"].shape == (300,) and s1["small"].shape == (100,)
    assert sum(v.nbytes for v in s1.values()) <= 4 * 400
    assert np.isin(s1["big"], big.numpy()).all()
    for n in ("big", "small"):
        assert np.array_equal(s1[n], np.load(tmp_path / "s2" / f"{n}.npy"))
