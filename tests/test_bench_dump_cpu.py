"""bench.py `--dump-outputs` without a GPU: names, dtype and the size limit of the dump; a grid gradient too large for the
limit is written as a sample of its rows, with the row indices, that depends on the buffer's shape and the seed only (two
builds dump the same rows), the rest is written whole."""
import os
from types import SimpleNamespace

import numpy as np
import torch

import bench


def _step(scale):
    g = torch.Generator().manual_seed(7)
    rows = torch.arange(64 ** 3, dtype=torch.float32)                       # row r of the large grid holds r * scale
    return SimpleNamespace(
        mlp_names=["net/affine-0/W", "net/affine-0/b"], grad_views=[torch.randn(3, 5, generator=g), torch.randn(7, generator=g)],
        grid_bufs={"net/voxel_feature/F": (rows * scale)[:, None].repeat(1, 4).view(64, 64, 64, 4),
                   "net/triline_feature/F": torch.randn(3, 16, 2, generator=g)})


def _dump(tmp_path, tag, step):
    out = str(tmp_path / tag)
    bench.dump_outputs(step, torch.tensor(0.5), out)
    return {f[:-len(".npy")]: np.load(os.path.join(out, f)) for f in os.listdir(out)}, \
        sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)                # the 4 MiB voxel gradient does not fit
    s1, s2 = _step(1.0), _step(2.0)
    got, size = _dump(tmp_path, "a", s1)
    assert size <= 1 << 20
    assert set(got) == {"loss", "grad.net.affine-0.W", "grad.net.affine-0.b", "grad.net.voxel_feature.F.sample",
                        "grad.net.voxel_feature.F.sample_rows", "grad.net.triline_feature.F"}
    assert all(v.dtype == (np.float64 if k.endswith(".sample_rows") else np.float32) for k, v in got.items())
    assert got["loss"].tolist() == [0.5]
    np.testing.assert_array_equal(got["grad.net.affine-0.W"], s1.grad_views[0].numpy())
    np.testing.assert_array_equal(got["grad.net.triline_feature.F"], s1.grid_bufs["net/triline_feature/F"].numpy())
    sample = got["grad.net.voxel_feature.F.sample"]
    assert sample.ndim == 2 and sample.shape[1] == 4 and 10000 < sample.shape[0] <= (1 << 19) // 24
    idx = sample[:, 0]
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < 64 ** 3        # distinct rows, in order
    assert (sample == idx[:, None]).all()                                       # whole rows ...
    np.testing.assert_array_equal(got["grad.net.voxel_feature.F.sample_rows"], idx)      # ... the rows the indices name
    got2, _ = _dump(tmp_path, "b", s2)
    np.testing.assert_array_equal(got2["grad.net.voxel_feature.F.sample"], 2 * sample)     # the same rows
