"""CPU: bench.py's --dump-outputs writer (the arrays one step() call returned, as .npy files in
float32 / float64)."""
import os

import numpy as np
import torch


def _returned(n=5):
    g = torch.Generator().manual_seed(3)
    obs = torch.rand(n, 7, generator=g, dtype=torch.float32)
    rew = torch.rand(n, generator=g, dtype=torch.float64)
    term = torch.tensor([0, 1, 0, 0, 1], dtype=torch.uint8)
    trunc = torch.tensor([0, 0, 1, 0, 0], dtype=torch.uint8)
    return obs, rew, term, trunc, {"info": None}


def test_dump_outputs_writes_float_arrays(tmp_path):
    import bench
    ret = _returned()
    d = str(tmp_path / "out")
    bench.dump_outputs(d, ret)
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in bench.DUMP_NAMES)
    want = {"obs": np.float32, "reward": np.float64, "terminated": np.float32, "truncated": np.float32}
    for name, t in zip(bench.DUMP_NAMES, ret):
        a = np.load(os.path.join(d, name + ".npy"))
        assert a.dtype == want[name] and a.shape == tuple(t.shape)
        np.testing.assert_array_equal(a, t.numpy().astype(want[name]))


def test_dump_outputs_rank_and_task_names(tmp_path):
    import bench
    d = str(tmp_path)
    bench.dump_outputs(d, _returned(), world=2, rank=1, prefix="humanoid_soccer_")
    assert sorted(os.listdir(d)) == sorted(f"humanoid_soccer_{n}.rank1.npy" for n in bench.DUMP_NAMES)
