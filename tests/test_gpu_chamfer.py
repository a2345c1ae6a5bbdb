"""The Chamfer evaluation on the device (ndjir_amd/chamfer.py, csrc/chamfer.hip; python/evaluate_chamfer_dtumvs.py:84-197)
against the numpy restatement tests/chamfer_ref.py, stage by stage and composed.  Every stage but the nearest distances is
compared exactly; tests/test_chamfer_ref_cpu.py holds the restatement against the reference, numpy and sklearn, and asserts
that no decision of the shared fixtures hangs on the last bits."""
import numpy as np
import pytest
import torch

from ndjir_amd import chamfer as C
from ndjir_amd import config as cfg
from tests import chamfer_ref as R

pytestmark = pytest.mark.gpu

THRESH = 0.2


def _np(t):
    return t.detach().cpu().numpy()


# ---- sampling --------------------------------------------------------------------------------------------------------------
def _random_triangles(F, rng, shortest=1e-3, longest=3.0):
    """F triangles (3F vertices) whose first two edges have lengths log-uniform in [shortest, longest]."""
    def edges():
        d = rng.standard_normal((F, 3))
        return d / R.norm3(d)[:, None] * np.exp(rng.uniform(np.log(shortest), np.log(longest), size=(F, 1)))
    p0 = rng.uniform(-5.0, 5.0, size=(F, 3))
    verts = np.stack([p0, p0 + edges(), p0 + edges()], axis=1).reshape(-1, 3)
    return verts, np.arange(3 * F, dtype=np.int64).reshape(F, 3)


def _check_sampling(gpu, verts, faces, thresh=THRESH):
    want, want_counts = R.sample_mesh(verts, faces, thresh)
    got, counts = C.sample_mesh_points(torch.from_numpy(verts).to(gpu), torch.from_numpy(faces).to(gpu), thresh, return_counts=True)
    assert got.dtype == torch.float64 and got.is_cuda
    np.testing.assert_array_equal(_np(counts), want_counts)
    assert got.shape == want.shape
    assert _np(got).tobytes() == want.tobytes()              # values and order, bit for bit
    return want_counts


@pytest.mark.parametrize("F", [1, 257, 5000])
def test_sampling_random_triangles(gpu, F):
    verts, faces = _random_triangles(F, np.random.default_rng(100 + F))
    counts = _check_sampling(gpu, verts, faces)
    if F >= 257:
        assert counts.max() > 20 and (counts == 0).sum() > F // 10       # large and empty triangles both occur


def test_sampling_more_than_a_million_triangles(gpu):
    """More than 1024 blocks of 1024 triangles: the scan of the block totals takes a second pass with a carry.  All but a few
    triangles are degenerate (one repeated vertex), so the restatement's loop stays short."""
    F = 1024 * 1024 + 300
    verts, some = _random_triangles(64, np.random.default_rng(77), 0.3, 1.0)
    faces = np.zeros((F, 3), dtype=np.int64)
    faces[:, 2] = 1
    faces[::16389] = some[:len(faces[::16389])]
    faces[-1] = some[-1]
    counts = _check_sampling(gpu, verts, faces, 0.05)
    assert counts[-1] > 0 and (counts > 0).sum() > 50


def test_sampling_special_triangles(gpu):
    a = np.array([0.3, -0.2, 0.1])
    e1, e2 = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    s = 70.0 * np.array([0.5, np.sqrt(0.75), 0.0])
    tris = [(a, a, a + e1),                                   # a repeated vertex
            (a, a + 0.5 * e1, a + 2.0 * e1),                   # collinear
            (a, a + 0.05 * e1, a + 2.0 * e2),                  # n1 = 0 < n2 = 10: nothing passes
            (a, a + 70.0 * e1, a + s),                         # about 10^5 candidates in one triangle
            (a, a + 0.7 * e1, a + 0.7 * e2),                   # n1 = n2 = 3: k0 + k1 reaches 1 up to rounding
            (a, a + 0.5 * e1, a + 0.5 * e2)]                   # n1 = n2 = 2: exactly 1
    verts = np.stack([p for t in tris for p in t])
    faces = np.arange(18, dtype=np.int64).reshape(6, 3)
    valid, n1, n2, *_ = R.triangle_grid(verts, faces, THRESH)
    assert valid.tolist() == [False, False, True, True, True, True]
    assert (n1[2], n2[2]) == (0, 10) and (n1[3] + 1) * (n2[3] + 1) > 1e5 and (n1[4], n2[4], n1[5], n2[5]) == (3, 3, 2, 2)
    counts = _check_sampling(gpu, verts, faces)
    assert counts[:3].tolist() == [0, 0, 0] and counts[3] > 5e4


def test_sampling_empty_and_float32(gpu):
    verts, faces = _random_triangles(40, np.random.default_rng(9))
    got = C.sample_mesh_points(verts, np.zeros((0, 3), dtype=np.int64), THRESH)
    assert got.shape == (0, 3) and got.dtype == torch.float64
    v32 = verts.astype(np.float32)                            # widened exactly, never rounded again
    want, _ = R.sample_mesh(v32.astype(np.float64), faces, THRESH)
    got = C.sample_mesh_points(torch.from_numpy(v32).to(gpu), faces, THRESH)
    assert _np(got).tobytes() == want.tobytes()


def test_sampling_reports_overflow_and_bad_faces(gpu):
    big = np.array([[0.0, 0.0, 0.0], [1e6, 0.0, 0.0], [0.0, 1e6, 0.0]])
    with pytest.raises(OverflowError):
        C.sample_mesh_points(torch.from_numpy(big).to(gpu), np.array([[0, 1, 2]]), THRESH)
    with pytest.raises(ValueError):
        C.sample_mesh_points(torch.from_numpy(big).to(gpu), np.array([[0, 1, 3]]), THRESH)


# ---- thinning --------------------------------------------------------------------------------------------------------------
def _check_thinning(gpu, pts, thresh, order=None, neighbors=None):
    want = R.thin(pts, thresh, order, neighbors)
    got, rounds = C.thin_points(torch.from_numpy(pts).to(gpu), thresh, order=np.arange(pts.shape[0]) if order is None else order,
                                return_rounds=True)
    assert got.dtype == torch.bool and got.shape == (pts.shape[0],)
    np.testing.assert_array_equal(_np(got), want)
    return _np(got), rounds


def test_thinning_small_clouds(gpu):
    keep = C.thin_points(torch.zeros((0, 3), device=gpu, dtype=torch.float64), THRESH)
    assert keep.shape == (0,) and keep.dtype == torch.bool
    assert _np(C.thin_points(np.array([[1.0, 2.0, 3.0]]), THRESH)).tolist() == [True]
    four = np.array([[0.0, 0.0, 0.0], [0.15, 0.0, 0.0], [0.0, 0.21, 0.0], [5.0, 5.0, 5.0]])      # 0-1 inside, the rest outside
    assert _check_thinning(gpu, four, THRESH)[0].tolist() == [True, False, True, True]
    assert _check_thinning(gpu, four, THRESH, np.array([1, 0, 3, 2]))[0].tolist() == [False, True, True, True]
    rng = np.random.default_rng(4)
    dup = np.repeat(rng.uniform(0.0, 3.0, size=(60, 3)), 3, axis=0)                                # every point three times
    keep, _ = _check_thinning(gpu, dup, THRESH, rng.permutation(180))
    assert keep.reshape(60, 3).sum(axis=1).max() == 1


def test_thinning_long_chain(gpu):
    """1 025 points on a line 0.6 thresh apart in index order: each point waits for its predecessor, so about one round per
    point; every second point is kept."""
    line = np.zeros((1025, 3))
    line[:, 0] = 0.6 * THRESH * np.arange(1025)
    keep, rounds = _check_thinning(gpu, line, THRESH)
    assert keep.tolist() == [k % 2 == 0 for k in range(1025)] and 1000 <= rounds <= 1025


@pytest.mark.parametrize("shuffled", [False, True])
def test_thinning_sheet(gpu, shuffled):
    pts, nbrs, _ = R.sheet_fixture()
    order = R.sheet_order(pts.shape[0]) if shuffled else None
    keep, rounds = _check_thinning(gpu, pts, R.SHEET_THRESH, order, nbrs)
    assert R.thin_invariants(pts, keep, R.SHEET_THRESH) == (True, True)
    assert rounds < 100


def test_thinning_default_order_is_seeded(gpu):
    pts = R.bumpy_sheet(3000, seed=2)
    a = _np(C.thin_points(torch.from_numpy(pts).to(gpu), THRESH, seed=5))
    order = torch.randperm(3000, generator=torch.Generator().manual_seed(5)).numpy()
    np.testing.assert_array_equal(a, R.thin(pts, THRESH, order))
    assert (a != _np(C.thin_points(pts, THRESH, seed=6))).any()
    with pytest.raises(ValueError):
        C.thin_points(pts, THRESH, order=np.zeros(3000, dtype=np.int64))


# ---- mask and plane --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,patch", [(0.5, 1.25), (0.37, 1.3)])
def test_mask_and_plane_filters(gpu, res, patch):
    rng = np.random.default_rng(31)
    dims = np.array([23, 17, 31])
    obs = (rng.uniform(size=tuple(dims)) < 0.6).astype(np.uint8)
    bb0 = np.array([-3.125, 2.25, -7.5])
    BB = np.stack([bb0, bb0 + dims * res + np.array([0.3, -0.2, 0.1])])
    B32 = BB.astype(np.float32)
    lo, hi = (B32[0] - patch).astype(np.float64), (B32[1] + patch * 2).astype(np.float64)
    pts = [rng.uniform(lo - patch, hi + patch, size=(10000, 3))]
    inside = rng.uniform(B32[0], B32[0] + dims * res, size=(400, 3))
    for a in range(3):
        for edge in (lo[a], np.nextafter(lo[a], -np.inf), hi[a], np.nextafter(hi[a], -np.inf)):     # exactly on the box's faces
            p = inside[:20].copy()
            p[:, a] = edge
            pts.append(p)
        for g in (-1.0, -0.5, 0.5, 1.5, 2.5, dims[a] - 1.5, dims[a] - 0.5, float(dims[a])):          # ties, one cell outside
            p = inside[:20].copy()
            p[:, a] = B32[0, a].astype(np.float64) + g * res
            pts.append(p)
    pts = np.concatenate(pts)
    want_bb, want_obs = R.mask_filter(pts, obs, BB, np.array([[res]]), patch)
    got_bb, got_obs = C.mask_points(torch.from_numpy(pts).to(gpu), obs, BB, np.array([[res]]), patch)
    np.testing.assert_array_equal(_np(got_bb), want_bb)
    np.testing.assert_array_equal(_np(got_obs), want_obs)
    assert 0 < want_obs.sum() < want_bb.sum() < pts.shape[0] and not (want_obs & ~want_bb).any()
    plane = np.array([0.3, -0.5, 1.0, -2.0])
    on = inside.copy()
    on[:, 2] = 2.0
    on[:, :2] = 0.0                                             # exactly on the plane: not above
    pts = np.concatenate([pts, on, on + 1e-12, on - 1e-12])
    want = R.above_plane(pts, plane)
    np.testing.assert_array_equal(_np(C.above_plane(torch.from_numpy(pts).to(gpu), plane.reshape(4, 1))), want)
    assert not want[-1200:-800].any() and want[-800:-400].all() and not want[-400:].any()


# ---- nearest ---------------------------------------------------------------------------------------------------------------
def _check_nearest(gpu, queries, targets, max_dist, want):
    dist, idx = C.nearest_distances(torch.from_numpy(queries).to(gpu), torch.from_numpy(targets).to(gpu), max_dist)
    dist, idx = _np(dist), _np(idx)
    assert dist.dtype == np.float64 and idx.dtype == np.int32
    found = np.isfinite(want)
    np.testing.assert_array_equal(np.isfinite(dist), found)                  # the +inf / -1 pattern
    np.testing.assert_array_equal(idx >= 0, found)
    assert (dist[~found] == np.inf).all() and (idx[~found] == -1).all()
    assert (np.abs(dist[found] - want[found]) <= 2 * np.spacing(want[found])).all()
    d = queries[found] - targets[idx[found]]
    assert (np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) == dist[found]).all()
    return dist, idx


def test_nearest_bumpy_sphere(gpu):
    targets, queries, want, _, _ = R.nearest_fixture()
    found = np.isfinite(want).reshape(4, -1).sum(axis=1)
    assert found[0] == found[1] == 1250 and 0 < found[2] < 1250 and found[3] == 0
    _check_nearest(gpu, queries, targets, R.NEAREST_MAX_DIST, want)


def test_nearest_small_inputs(gpu):
    rng = np.random.default_rng(8)
    targets = rng.uniform(-1.0, 1.0, size=(100, 3))
    dist, idx = C.nearest_distances(np.zeros((0, 3)), targets, 2.0)
    assert dist.shape == (0,) and idx.shape == (0,)
    dist, idx = C.nearest_distances(targets, np.zeros((0, 3)), 2.0)           # no targets: nothing is near
    assert (_np(dist) == np.inf).all() and (_np(idx) == -1).all()
    queries = rng.uniform(-4.0, 4.0, size=(500, 3))
    one = np.array([[0.25, -0.5, 1.0]])
    _check_nearest(gpu, queries, one, 2.0, R.nearest(queries, one, 2.0)[0])
    ball = one + 1e-3 * rng.standard_normal((300, 3))                         # all targets in one cell (h = 0.25)
    _check_nearest(gpu, queries, ball, 2.0, R.nearest(queries, ball, 2.0)[0])


# ---- composed --------------------------------------------------------------------------------------------------------------
COUNTS = ("sampled", "thinned", "in_bb", "in_obs", "above", "used_d2s", "used_s2d")


def _conf():
    c = R.COMPOSED
    return cfg.load("default", [f"valid.dtumvs.downsample_density={c['thresh']}", f"valid.dtumvs.patch_size={c['patch']}",
                                f"valid.dtumvs.max_dist={c['max_dist']}"])


def _evaluate_both(gpu, faces=True, order=True, **kw):
    f, c = R.composed_fixture(), R.COMPOSED
    faces = f["faces"] if faces else None
    order = f["order"] if order else np.arange(f["verts"].shape[0])
    ref = R.evaluate(f["verts"], faces, f["stl"], f["obs"], f["BB"], f["Res"], f["plane"], c["thresh"], c["patch"], c["max_dist"],
                     c["scale"], c["trans"], order, **kw)
    got = C.evaluate_chamfer(torch.from_numpy(f["verts"]).to(gpu), faces, f["stl"], f["obs"], f["BB"], f["Res"], f["plane"], _conf(),
                             scale=c["scale"], trans=c["trans"], order=order, **kw)
    for k in COUNTS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    np.testing.assert_array_equal(_np(got["data_down"]), ref["cloud"][ref["keep"]])
    np.testing.assert_array_equal(_np(got["in_bb_mask"]), ref["in_bb_mask"])
    np.testing.assert_array_equal(_np(got["in_obs_mask"]), ref["in_obs_mask"])
    for k in ("dist_d2s", "dist_s2d"):
        np.testing.assert_array_equal(np.isfinite(_np(got[k])), np.isfinite(ref[k]))
    for k in ("mean_d2s", "mean_s2d", "overall"):
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-12)
    return got, ref


def test_evaluate_chamfer(gpu):
    got, ref = _evaluate_both(gpu)
    assert got["sampled"] > 0 and abs(got["mean_d2s"] - 0.5) < 0.1          # the mesh lies 0.5 mm outside the scan
    assert got["overall"] == (got["mean_d2s"] + got["mean_s2d"]) / 2


def test_evaluate_chamfer_reference_sampling_order(gpu):
    """`sample_before_transform=True`: the reference samples the normalised mesh with thresh in millimetres -- edges of
    about 0.09 against thresh 1.5 give n1 = n2 = 0, no samples; the cloud is the transformed vertices alone."""
    got, _ = _evaluate_both(gpu, order=False, sample_before_transform=True)
    assert got["sampled"] == 0 and got["thinned"] <= R.composed_fixture()["verts"].shape[0]


def test_evaluate_chamfer_point_cloud_mode_and_empty_stage(gpu):
    got, _ = _evaluate_both(gpu, faces=False, order=False)
    assert got["sampled"] == 0
    f, c = R.composed_fixture(), R.COMPOSED
    with pytest.raises(ValueError, match="d2s"):                          # the mesh far from the mask: nothing to average
        C.evaluate_chamfer(torch.from_numpy(f["verts"]).to(gpu), None, f["stl"], f["obs"], f["BB"], f["Res"], f["plane"], _conf(),
                           scale=c["scale"], trans=c["trans"] + 1000.0)
