"""bench.py's plain run and --dump-outputs: the plain line carries the headline figures only (the instrumented step, the
CPU baseline and the other configurations are --full), and the dump holds what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + [str(a) for a in argv],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {fn[:-4]: np.load(os.path.join(d, fn)) for fn in sorted(os.listdir(d))}


def test_dump_outputs_writes_float32_and_keeps_the_size_limit(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    bench.dump_outputs(str(tmp_path / "a"), {"x": torch.arange(6, dtype=torch.float64).reshape(2, 3)})
    x = np.load(tmp_path / "a" / "x.npy")
    assert x.dtype == np.float32 and x.shape == (2, 3) and x[1, 2] == 5
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 16)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "b"), {"x": torch.zeros(5)})
    assert not (tmp_path / "b").exists()


@pytest.mark.gpu
def test_plain_train_bench_line_and_dump_are_reproducible(tmp_path):
    args = ["--gpus", 1, "--steps", 3, "--warmup", 1, "--batch", 4, "--seconds", 1]
    res = [_bench(*(args + ["--dump-outputs", tmp_path / str(i)])) for i in range(2)]
    for r in res:
        assert r["metric"] == "16 kHz frames/sec (train step)" and r["unit"] == "frames/s" and r["dtype"] == "f32"
        assert r["higher_is_better"] is True and r["steps"] == 3 and r["warmup"] == 1
        assert r["ms_per_step"] > 0 and r["value"] > 0
        assert r["roofline"] is None and r["cpu_baseline"] is None and "other_configs" not in r
    a, b = _load(tmp_path / "0"), _load(tmp_path / "1")
    assert sorted(a) == sorted(["loss", "loss_l1", "loss_stft_sc", "loss_stft_mag", "grad_norm_sq", "gradients", "parameters",
                                "bn_statistics"])
    assert a["gradients"].shape == (298592,) and a["parameters"].shape == (381472,)
    assert abs(float(a["loss"][0]) - res[0]["config"]["loss"]) <= 1e-6 * abs(res[0]["config"]["loss"])
    np.testing.assert_allclose(a["grad_norm_sq"][0], float((a["gradients"].astype(np.float64) ** 2).sum()), rtol=1e-4)
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all(), k
        # same arguments, same seeded inputs: the same outputs (the kernels reduce in a fixed order)
        np.testing.assert_allclose(a[k], b[k], rtol=1e-5, atol=1e-7, err_msg=k)


@pytest.mark.gpu
def test_plain_streaming_bench_dumps_the_forward_output(tmp_path):
    r = _bench("--gpus", 1, "--streaming", "--steps", 5, "--warmup", 2, "--dump-outputs", tmp_path)
    assert r["steps"] == 5 and r["ms_per_step"] > 0 and r["roofline"] is None and r["cpu_baseline"] is None
    y = np.load(tmp_path / "output.npy")
    assert y.dtype == np.float32 and y.shape[0] == 1024 and np.isfinite(y).all()
