"""bench.py's plain run and its --dump-outputs / --full options.

A plain run carries the headline fields only (everything measured beside it is null) and,
with --dump-outputs DIR, writes what its last timed step returned as DIR/<name>.npy.  The CPU
test drives the dry-run stand-in; the GPU test runs the smallest configuration once and checks
the dumped arrays against the oracle at the suite's parity bar (1e-4 relative, test_gpu_parity).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    e = dict(os.environ)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(v, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=e,
                       capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return r.returncode, (json.loads(lines[-1]) if lines else None), r.stderr


def test_dry_run_dumps_the_last_step(tmp_path):
    d = tmp_path / "out"
    rc, out, err = _bench("--gpus", "1", "--dry-run", "--steps", "7", "--warmup", "2",
                          "--dump-outputs", str(d))
    assert rc == 0, err[-2000:]
    assert out["steps"] == 7 and out["ms_per_step"] >= 0
    U = np.load(d / "U.npy")
    m = U.shape[0]
    assert U.dtype == np.float64 and U.shape == (m, 10)
    # the stand-in step s returns base_u + rank + 1000 s; the last timed step is warmup + steps - 1
    base_u = np.arange(m * 10, dtype=np.float64).reshape(m, 10) / (m * 10)
    assert np.array_equal(U, base_u + 1000.0 * 8)


def test_dump_cap_samples_large_arrays(tmp_path, monkeypatch):
    import torch

    import bench
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 4096)
    big = torch.arange(4096, dtype=torch.float32).reshape(64, 64)     # 16 KiB: sampled
    small = torch.arange(30, dtype=torch.float64).reshape(3, 10)      # kept whole
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), {"grad_X": big, "U": small})
    a, b = np.load(tmp_path / "a" / "grad_X.npy"), np.load(tmp_path / "b" / "grad_X.npy")
    assert a.dtype == np.float32 and a.shape == (512,) and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0)                                     # distinct entries, in order
    assert np.array_equal(np.load(tmp_path / "a" / "U.npy"), small.numpy())
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 4096 + 2 * 128                                    # data + two .npy headers


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from graphlearninglayer_amd import GLL
    from graphlearninglayer_amd.synth import CONFIGS, one_hot, seeded_gbar, synth
    from oracle import gll_oracle as O

    d = tmp_path / "out"
    rc, out, err = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "plumbing",
                          "--dump-outputs", str(d))
    assert rc == 0, err[-2000:]
    assert out["steps"] == 3 and out["full"] is False
    assert out["unit"] == "calls/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    # one GPU: value = 1 / step time (ms_per_step is rounded to 1e-4 ms, a step takes > 0.01 ms)
    assert out["value"] == pytest.approx(1e3 / out["ms_per_step"], rel=1e-2)
    for moved in ("roofline", "events_pass", "cpu_baseline", "c_abi", "autograd_other_thread",
                  "batched", "auto_eps_extra"):
        assert out[moved] is None, moved
    assert out["kernels"] == {} and "call_roofline" not in out

    c = CONFIGS["plumbing"]
    n, m = c["base"] + c["batch"], c["batch"]
    U, gx = np.load(d / "U.npy"), np.load(d / "grad_X.npy")
    assert U.dtype == np.float64 and U.shape == (m, 10)
    assert gx.dtype == np.float32 and gx.shape == (n, c["d"])
    # the bench's seeded inputs (rank 0), through the oracle on the GPU's own kNN lists
    X, lab = synth(c["base"], c["batch"], c["d"], r=c["r"], seed=0)
    Y, g = one_hot(lab[: c["base"]]), seeded_gbar(m, 10, 1234)
    ind = GLL.device_graph(torch.from_numpy(X).cuda(), c["k"])["knn_idx"].cpu().numpy()
    Uo, st = O.forward(X, Y, 0.07, 1.0, c["k"], knn=(ind, None))
    eU, eg = O.rel_err(U, Uo), O.rel_err(gx, O.backward(st, g))
    print(f"dumped U vs oracle {eU:.2e}, dumped grad_X vs oracle {eg:.2e}")
    assert eU < 1e-4 and eg < 1e-4, (eU, eg)
