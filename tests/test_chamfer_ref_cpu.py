"""The numpy restatement of the Chamfer evaluation (tests/chamfer_ref.py) against what pins it without a GPU: the reference's
own `sample_single_tri` (recorded in tests/golden/chamfer_sample_tri.npz by make_chamfer_golden.py), numpy's own reductions,
and sklearn's kd-tree where it is installed; the PLY reader; and the conditions the shared fixtures must meet for the GPU
tests to demand exact equality."""
import os

import numpy as np
import pytest

from ndjir_amd import meshio
from ndjir_amd import config as cfg
from tests import chamfer_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chamfer_sample_tri.npz")


def test_sampler_equals_the_recorded_reference():
    g = np.load(GOLDEN)
    ns = {tuple(n) for n in g["n"].tolist()}
    assert ns == {(a, b) for a in (0, 1, 2, 3, 7, 16) for b in (0, 1, 2, 3, 7, 16)}
    start = 0
    for k, (n1, n2) in enumerate(g["n"]):
        q = R.sample_tri(n1, n2, g["v1"][k], g["v2"][k], g["p0"][k])
        want = g["points"][start:start + g["counts"][k]]
        start += g["counts"][k]
        assert q.shape == want.shape, (n1, n2)
        assert q.tobytes() == want.tobytes(), (n1, n2)
    assert start == g["points"].shape[0]
    by_n = dict(zip(map(tuple, g["n"].tolist()), g["counts"].tolist()))
    assert by_n[(2, 2)] == 1 and by_n[(3, 3)] == 3 and by_n[(0, 7)] == 0 and by_n[(7, 0)] == 0      # the ties at k0 + k1 = 1


def test_written_out_sums_are_numpys():
    rng = np.random.default_rng(0)
    v = rng.standard_normal((100000, 3)) * 10.0 ** rng.uniform(-3, 3, (100000, 3))
    assert R.norm3(v).tobytes() == np.linalg.norm(v, axis=-1).tobytes()
    P = rng.standard_normal(4)
    hom = np.concatenate([v, np.ones_like(v[:, :1])], -1)
    s = (P.reshape((1, 4)) * hom).sum(-1)
    mine = ((P[0] * v[:, 0] + P[1] * v[:, 1]) + P[2] * v[:, 2]) + P[3] * 1.0
    assert mine.tobytes() == s.tobytes()
    assert (R.above_plane(v, P) == (s > 0)).all()
    w = rng.standard_normal((1000, 3))
    c = np.cross(v[:1000], w)
    valid, n1, n2, v1, v2, p0 = R.triangle_grid(np.concatenate([np.zeros((1, 3)), v[:1000], w]),
                                                np.stack([np.zeros(1000, int), np.arange(1, 1001), np.arange(1001, 2001)], 1), 0.2)
    assert valid.all() and (v1 == v[:1000]).all() and (v2 == w).all()
    l1, l2, area2 = np.linalg.norm(v1, axis=-1), np.linalg.norm(v2, axis=-1), np.linalg.norm(c, axis=-1)
    thr = 0.2 * np.sqrt(l1 * l2 / area2)
    assert (n1 == np.floor(l1 / thr)).all() and (n2 == np.floor(l2 / thr)).all()


def test_fixture_conditions():
    """Exact equality on the GPU is demanded only where no decision hangs on the last bits: every pair of the thinning
    fixtures is at least 1e-9 from thresh, every nearest distance at least 1e-9 from max_dist."""
    pts, nbrs, gap = R.sheet_fixture()
    assert pts.shape == (20000, 3) and gap >= 1e-9, gap
    assert R.nearest_fixture()[4] >= 1e-9
    f, C = R.composed_fixture(), R.COMPOSED
    ref = R.evaluate(f["verts"], f["faces"], f["stl"], f["obs"], f["BB"], f["Res"], f["plane"], C["thresh"], C["patch"],
                     C["max_dist"], C["scale"], C["trans"], f["order"])
    assert ref["max_dist_gap"] >= 1e-9
    assert R.radius_neighbors(ref["cloud"], C["thresh"], with_gap=True)[1] >= 1e-9
    # the fixture exercises every stage
    assert 0 < ref["sampled"] and ref["in_obs"] < ref["in_bb"] < ref["thinned"] < ref["cloud"].shape[0]
    assert ref["used_s2d"] < ref["above"] < f["stl"].shape[0] and ref["used_d2s"] == ref["in_obs"]
    assert abs(ref["mean_d2s"] - 0.5) < 0.1


def test_thinning_is_the_greedy_independent_set():
    pts, nbrs, _ = R.sheet_fixture()
    for order in (None, R.sheet_order(pts.shape[0])):
        keep = R.thin(pts, R.SHEET_THRESH, order, nbrs)
        assert R.thin_invariants(pts, keep, R.SHEET_THRESH) == (True, True)
        first = 0 if order is None else order[0]
        assert keep[first]


def test_against_sklearn_kd_tree():
    skln = pytest.importorskip("sklearn.neighbors")
    pts, nbrs, _ = R.sheet_fixture()
    engine = skln.NearestNeighbors(n_neighbors=1, radius=R.SHEET_THRESH, algorithm="kd_tree")
    for order in (np.arange(pts.shape[0]), R.sheet_order(pts.shape[0])):
        shuffled = pts[order]
        engine.fit(shuffled)
        rnn = engine.radius_neighbors(shuffled, radius=R.SHEET_THRESH, return_distance=False)
        mask = np.ones(shuffled.shape[0], dtype=np.bool_)
        for curr, idxs in enumerate(rnn):                     # python/evaluate_chamfer_dtumvs.py:128-132
            if mask[curr]:
                mask[idxs] = 0
                mask[curr] = 1
        keep = np.zeros_like(mask)
        keep[order] = mask
        assert (keep == R.thin(pts, R.SHEET_THRESH, order, nbrs)).all()
    targets, queries, dist, idx, _ = R.nearest_fixture()
    engine.fit(targets)
    d, _ = engine.kneighbors(queries, n_neighbors=1, return_distance=True)
    found = d[:, 0] < R.NEAREST_MAX_DIST
    assert (found == np.isfinite(dist)).all()
    np.testing.assert_allclose(dist[found], d[found, 0], rtol=1e-12)


def _write_ply(path, binary, rng):
    n = 37
    xyz = rng.standard_normal((n, 3)) * 100.0
    normals = rng.standard_normal((n, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, size=(n, 3)).astype(np.uint8)
    header = ["ply", "format " + ("binary_little_endian" if binary else "ascii") + " 1.0", "comment made for the test",
              f"element vertex {n}", "property float nx", "property double x", "property double y", "property float ny",
              "property double z", "property float nz", "property uchar red", "property uchar green", "property uchar blue",
              "element face 1", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fp:
        fp.write(("\n".join(header) + "\n").encode("ascii"))
        if binary:
            rec = np.zeros(n, dtype=[("nx", "<f4"), ("x", "<f8"), ("y", "<f8"), ("ny", "<f4"), ("z", "<f8"), ("nz", "<f4"),
                                     ("r", "u1"), ("g", "u1"), ("b", "u1")])
            rec["nx"], rec["ny"], rec["nz"] = normals.T
            rec["x"], rec["y"], rec["z"] = xyz.T
            rec["r"], rec["g"], rec["b"] = rgb.T
            fp.write(rec.tobytes())
            fp.write(np.uint8(3).tobytes() + np.asarray([0, 1, 2], dtype="<i4").tobytes())
        else:
            for k in range(n):
                nx, ny, nz = (float(c) for c in normals[k])
                x, y, z = (float(c) for c in xyz[k])             # repr of a Python float round-trips
                fp.write(f"{nx!r} {x!r} {y!r} {ny!r} {z!r} {nz!r} {rgb[k, 0]} {rgb[k, 1]} {rgb[k, 2]}\n".encode("ascii"))
            fp.write(b"3 0 1 2\n")
    return xyz


@pytest.mark.parametrize("binary", [False, True])
def test_read_ply_points(tmp_path, binary):
    path = str(tmp_path / "cloud.ply")
    xyz = _write_ply(path, binary, np.random.default_rng(1))
    got = meshio.read_ply_points(path)
    assert got.dtype == np.float64 and got.shape == xyz.shape
    assert got.tobytes() == xyz.tobytes()


def test_read_ply_points_rejects_what_it_cannot_read(tmp_path):
    path = str(tmp_path / "bad.ply")
    with open(path, "wb") as fp:
        fp.write(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
    with pytest.raises(ValueError):
        meshio.read_ply_points(path)
    with open(path, "wb") as fp:
        fp.write(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nend_header\n0 0\n")
    with pytest.raises(ValueError):
        meshio.read_ply_points(path)


def test_config_keys_of_the_evaluation():
    d = cfg.load("default").valid.dtumvs
    assert (d.downsample_density, d.patch_size, d.max_dist) == (0.2, 60, 20)


def test_load_dtu_reference_needs_scipy(monkeypatch, tmp_path):
    import builtins
    from ndjir_amd import chamfer
    real = builtins.__import__

    def no_scipy(name, *a, **k):
        if name.startswith("scipy"):
            raise ImportError(name)
        return real(name, *a, **k)

    monkeypatch.setattr(builtins, "__import__", no_scipy)
    with pytest.raises(ImportError, match="scipy"):
        chamfer.load_dtu_reference(str(tmp_path), 69)
