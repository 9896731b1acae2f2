"""bench.py --dump-outputs: what the timed path computed in its last step, as DIR/<name>.npy (float32 / float64, at most 64 MB in all,
large buffers as a fixed seeded sample), identical from run to run with the same arguments; and --steps is the number of timed steps."""
import os

import numpy as np
import pytest


class _Frame:
    """stands in for a DeviceFrame: outputs() as DeviceFrame.outputs() gives them (uint16 / uint32 values held as int16 / int32 bits)"""

    def __init__(self, torch):
        g = torch.Generator().manual_seed(3)
        self.bufs = {"pred": (torch.randint(0, 256, (5_000_000,), dtype=torch.uint8, generator=g), np.uint8),
                     "pred16": (torch.randint(-2 ** 15, 2 ** 15, (3_000_000,), dtype=torch.int16, generator=g), np.uint16),
                     "coef": (torch.randint(-2 ** 15, 2 ** 15, (1000,), dtype=torch.int16, generator=g), np.int16),
                     "cost": (torch.tensor([-1, 0, 7, 2 ** 31 - 1], dtype=torch.int32), np.int32),
                     "ssd": (torch.tensor([-1, 0, 7], dtype=torch.int32), np.uint32)}

    def outputs(self):
        return self.bufs


def test_dump_outputs_types_budget_and_sample(tmp_path):
    import torch
    import bench
    dev = _Frame(torch)
    a, b = tmp_path / "a", tmp_path / "b"
    ra, rb = bench.dump_outputs(torch, dev, str(a)), bench.dump_outputs(torch, dev, str(b))
    assert ra == rb and sorted(os.listdir(a)) == sorted(n + ".npy" for n in dev.bufs)
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= bench.DUMP_BYTES
    for name, (t, dtype) in dev.bufs.items():
        got = np.load(a / (name + ".npy"))
        assert got.dtype == (np.float32 if np.dtype(dtype).itemsize <= 2 else np.float64)
        assert np.array_equal(got, np.load(b / (name + ".npy")))
        full = t.numpy().view(dtype)
        if ra[name][0] == ra[name][1]:
            assert np.array_equal(got, full)
        else:   # a sample: fewer elements, every one of them a value of the buffer, the same elements from run to run (above)
            assert 0 < ra[name][0] < ra[name][1] == full.size
            assert np.isin(got, full).all()
    assert list(np.load(a / "ssd.npy")) == [2.0 ** 32 - 1, 0.0, 7.0]
    assert list(np.load(a / "cost.npy")) == [-1.0, 0.0, 7.0, 2.0 ** 31 - 1]


@pytest.mark.gpu
def test_bench_dump_is_the_timed_step_and_repeatable(tmp_path):
    """two runs with the same arguments dump the same arrays, and they are what the same picture's step computes in this process;
    the line's `steps` are the timed steps (one block of exactly --steps steps)"""
    import json
    import subprocess
    import sys
    import torch
    import bench
    from turingcodec_amd import Havoc, step
    from turingcodec_amd.workload import FrameWorkload
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = ["--res", "416x240", "--seed", "5", "--inflight", "1", "--steps", "3", "--warmup", "1", "--tune", "0", "--kernel-reps", "1", "--decisions", "0",
            "--no-cpu-baseline", "--extra-4k", "0", "--traffic", "0"]
    lines = []
    for d in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args + ["--dump-outputs", str(tmp_path / d), "--detail-out", str(tmp_path / (d + ".json"))],
                             capture_output=True, text=True, timeout=600, cwd=root)
        assert out.returncode == 0, out.stderr[-2000:]
        lines.append(json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1]))
    detail = json.load(open(tmp_path / "a.json"))
    assert lines[0]["steps"] == 3 and detail["timing"]["timed_blocks"] == 1 and detail["outputs_dumped"]["dir"] == str(tmp_path / "a")
    hv = Havoc(0, stream="new")
    dev = step.DeviceFrame(hv, FrameWorkload(416, 240, 8, 5, qp=32, mix="ra"))
    dev.step()
    hv.sync()
    bench.dump_outputs(torch, dev, str(tmp_path / "here"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(n + ".npy" for n in dev.outputs()) and sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= bench.DUMP_BYTES
    for f in names:
        a = np.load(tmp_path / "a" / f)
        assert a.dtype in (np.float32, np.float64)
        assert np.array_equal(a, np.load(tmp_path / "b" / f)), f
        assert np.array_equal(a, np.load(tmp_path / "here" / f)), f
