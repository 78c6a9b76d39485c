"""bench.py --dump-outputs: the writer of the timed path's last outputs (one float32 .npy per array, a fixed seeded
sample of the elements when the arrays together would pass the size cap).  CPU only."""
import os

import numpy as np
import torch

import bench


def _outputs(n):
    rng = np.random.default_rng(5)
    return {"tile": torch.from_numpy(rng.integers(0, 1 << 20, n).astype(np.int32)),
            "hmirror": torch.from_numpy(rng.integers(0, 2, n).astype(np.uint8)),
            "err": torch.from_numpy(rng.random(n).astype(np.float32))}


def test_dump_outputs_whole_arrays(tmp_path):
    outs = _outputs(1000)
    d = str(tmp_path / "dump" / "nested")
    bench.dump_outputs(d, outs)
    assert sorted(os.listdir(d)) == ["err.npy", "hmirror.npy", "tile.npy"]
    for k, v in outs.items():
        a = np.load(os.path.join(d, k + ".npy"))
        assert a.dtype == np.float32 and a.shape == (1000,)
        assert np.array_equal(a.astype(np.float64), v.numpy().astype(np.float64))  # indices below 2^24: exact


def test_dump_outputs_sample_is_capped_and_repeatable(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 3 * (4 * 100 + 1024))
    outs = _outputs(1000)
    bench.dump_outputs(str(tmp_path / "a"), outs)
    bench.dump_outputs(str(tmp_path / "b"), outs)
    sel = None
    for k, v in outs.items():
        a, b = np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))
        assert a.shape == (100,) and np.array_equal(a, b)
        if k == "tile":  # the sampled positions: found from the (distinct enough) tile values, in order
            full = v.numpy().astype(np.float32)
            sel = np.sort(np.random.default_rng(0).choice(1000, 100, replace=False))
            assert np.array_equal(a, full[sel])
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_MAX_BYTES  # data + the .npy headers
    assert np.array_equal(np.load(tmp_path / "a" / "err.npy"), outs["err"].numpy()[sel])
