"""numpy restatement of python/evaluate_chamfer_dtumvs.py:84-197 in float64 for the Chamfer tests: the triangle sampler
(`sample_single_tri` and the expressions around it), the greedy thinning as the sequential loop over brute-force radius
neighbours, the observation-mask and ground-plane filters, brute-force nearest neighbours bounded by max_dist, and the stages
composed.  Sums whose order decides the last bit are written out (numpy sums three or four terms along the last axis left
to right; tests/test_chamfer_ref_cpu.py holds that against `np.linalg.norm` and `.sum(-1)`).  Also the fixtures several test
files share.  A helper, not a test; nothing here touches the product."""
import functools

import numpy as np

PAIR_BLOCK = 1 << 22        # pairs per block of the brute-force passes


def norm3(v):
    """np.linalg.norm(v, axis=-1) for (..., 3): the squares summed left to right."""
    return np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])


def sample_tri(n1, n2, v1, v2, p0):
    """`sample_single_tri` (:32-41): candidates (i, j), i in [0, n1], j in [0, n2], i major, at k = ((i + .5) / max(n1, 1e-7),
    (j + .5) / max(n2, 1e-7)); those with k0 + k1 < 1 give (v1 k0 + v2 k1) + p0.  v1, v2, p0: (3,)."""
    k0 = (np.arange(int(n1) + 1, dtype=np.float64) + 0.5) / max(float(n1), 1e-7)
    k1 = (np.arange(int(n2) + 1, dtype=np.float64) + 0.5) / max(float(n2), 1e-7)
    K0, K1 = np.meshgrid(k0, k1, indexing="ij")
    sel = (K0 + K1) < 1
    a, b = K0[sel][:, None], K1[sel][:, None]          # boolean selection walks row-major: i major
    return (v1[None, :] * a + v2[None, :] * b) + p0[None, :]


def triangle_grid(verts, faces, thresh):
    """:86, :92-103 for every triangle: (valid (F,), n1, n2 (F,) float64 -- meaningless where not valid --, v1, v2, p0)."""
    tri = np.asarray(verts, dtype=np.float64)[np.asarray(faces, dtype=np.int64).reshape(-1, 3)]
    p0 = tri[:, 0]
    v1, v2 = tri[:, 1] - p0, tri[:, 2] - p0
    l1, l2 = norm3(v1), norm3(v2)
    c = np.stack([v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1], v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2],
                  v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]], axis=1)
    area2 = norm3(c)
    valid = area2 > 0
    with np.errstate(all="ignore"):
        thr = thresh * np.sqrt(l1 * l2 / area2)
        n1, n2 = np.floor(l1 / thr), np.floor(l2 / thr)
    return valid, n1, n2, v1, v2, p0


def sample_mesh(verts, faces, thresh):
    """:92-108 -> (points (S, 3), points per triangle (F,))."""
    valid, n1, n2, v1, v2, p0 = triangle_grid(verts, faces, thresh)
    out, counts = [np.zeros((0, 3))], np.zeros(valid.shape[0], dtype=np.int64)
    for t in np.nonzero(valid)[0]:
        q = sample_tri(n1[t], n2[t], v1[t], v2[t], p0[t])
        counts[t] = q.shape[0]
        out.append(q)
    return np.concatenate(out, axis=0), counts


def _pair_d2(a, b):
    dx, dy, dz = b[None, :, 0] - a[:, None, 0], b[None, :, 1] - a[:, None, 1], b[None, :, 2] - a[:, None, 2]
    return dx * dx + dy * dy + dz * dz


def pair_blocks(a, b):
    """(first row, squared distances of a[first row : ...] to all of b) in blocks of at most PAIR_BLOCK pairs."""
    step = max(1, PAIR_BLOCK // max(1, b.shape[0]))
    for s in range(0, a.shape[0], step):
        yield s, _pair_d2(a[s:s + step], b)


def radius_neighbors(points, thresh, with_gap=False):
    """For every point the indices within thresh (d2 <= thresh^2, the point itself included), ascending, by brute force
    over the points whose x lies within 1.5 thresh of the block's (every other pair is farther than 1.5 thresh).  With
    `with_gap`, also the smallest |d - thresh| over all pairs (`thresh_gap`)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    by_x = np.argsort(points[:, 0], kind="stable")
    xs = points[by_x, 0]
    out, gap = [None] * points.shape[0], 0.29 * thresh
    for s in range(0, points.shape[0], 256):
        rows = by_x[s:s + 256]
        lo = np.searchsorted(xs, xs[s] - 1.5 * thresh, side="left")
        hi = np.searchsorted(xs, xs[min(s + 256, xs.shape[0]) - 1] + 1.5 * thresh, side="right")
        cand = np.sort(by_x[lo:hi])
        d2 = _pair_d2(points[rows], points[cand])
        gap = min(gap, thresh_gap(d2, thresh))
        for r, row in zip(rows, d2 <= thresh * thresh):
            out[r] = cand[row]
    return (out, gap) if with_gap else out


def thresh_gap(d2, thresh):
    """The smallest |d - thresh| among squared distances d2; only those within a factor two of thresh^2 can hold it (else
    the answer is at least 0.29 thresh, returned as that)."""
    near = d2[(d2 > 0.5 * thresh * thresh) & (d2 < 2.0 * thresh * thresh)]
    return min(edge_gap(np.sqrt(near), thresh), 0.29 * thresh)


def thin(points, thresh, order=None, neighbors=None):
    """:119-133 with the shuffle as the permutation `order` (point order[k] is visited k-th; the reference moves the rows
    instead, which changes no distance): keep (N,) bool in the input order.  `neighbors`: `radius_neighbors(points, thresh)`
    if already known."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    N = points.shape[0]
    order = np.arange(N) if order is None else np.asarray(order, dtype=np.int64)
    nbrs = radius_neighbors(points, thresh) if neighbors is None else neighbors
    mask = np.ones(N, dtype=bool)
    for curr in order:
        if mask[curr]:
            mask[nbrs[curr]] = False
            mask[curr] = True
    return mask


def thin_invariants(points, keep, thresh):
    """(no two kept points within thresh, every dropped point has a kept point within thresh), by brute force."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    kept = points[keep]
    independent, covered = True, True
    for s, d2 in pair_blocks(points, kept):
        near = (d2 <= thresh * thresh).sum(axis=1)
        k = keep[s:s + d2.shape[0]]
        independent = independent and bool((near[k] == 1).all())       # a kept point sees itself only
        covered = covered and bool((near[~k] >= 1).all())
    return independent, covered


def mask_filter(points, obs_mask, BB, Res, patch):
    """:139-149 -> (in_bb (N,), in_obs (N,)): in_obs marks the points of `data_in_obs` among all points."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    BB = np.asarray(BB).astype(np.float32)
    inbound = ((points >= BB[:1] - patch) & (points < BB[1:] + patch * 2)).sum(axis=-1) == 3
    data_in = points[inbound]
    grid = np.around((data_in - BB[:1]) / Res)
    shape = np.asarray(obs_mask.shape, dtype=np.float64)[None]
    grid_inbound = ((grid >= 0) & (grid < shape)).sum(axis=-1) == 3
    g = grid[grid_inbound].astype(np.int32)
    hit = obs_mask[g[:, 0], g[:, 1], g[:, 2]].astype(bool)
    in_obs = np.zeros(points.shape[0], dtype=bool)
    in_obs[np.nonzero(inbound)[0][grid_inbound][hit]] = True
    return inbound, in_obs


def above_plane(points, plane):
    """:168-169, the four products summed left to right."""
    p, P = np.asarray(points, dtype=np.float64).reshape(-1, 3), np.asarray(plane, dtype=np.float64).reshape(4)
    return ((P[0] * p[:, 0] + P[1] * p[:, 1]) + P[2] * p[:, 2]) + P[3] * 1.0 > 0


def nearest_raw(queries, targets):
    """Brute force: (distance (Q,), index (Q,)) of the nearest target, whatever its distance."""
    queries = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    targets = np.asarray(targets, dtype=np.float64).reshape(-1, 3)
    dist = np.full(queries.shape[0], np.inf)
    idx = np.full(queries.shape[0], -1, dtype=np.int64)
    if targets.shape[0] == 0:
        return dist, idx
    for s, d2 in pair_blocks(queries, targets):
        j = d2.argmin(axis=1)
        dist[s:s + d2.shape[0]] = np.sqrt(d2[np.arange(d2.shape[0]), j])
        idx[s:s + d2.shape[0]] = j
    return dist, idx


def nearest(queries, targets, max_dist, raw=None):
    """(dist (Q,), idx (Q,)) of the nearest target closer than max_dist; +inf and -1 where there is none (:162, :174 use
    nothing else).  `raw`: `nearest_raw(queries, targets)` if already known."""
    d, j = nearest_raw(queries, targets) if raw is None else raw
    ok = d < max_dist
    return np.where(ok, d, np.inf), np.where(ok, j, -1)


def edge_gap(values, edge):
    """The smallest |value - edge| (inf for no values): how far a fixture stays from a decision boundary."""
    values = np.asarray(values, dtype=np.float64)
    return float(np.abs(values - edge).min()) if values.size else np.inf


def evaluate(verts, faces, stl, obs_mask, BB, Res, plane, thresh, patch, max_dist, scale=1.0, trans=0.0, order=None,
             sample_before_transform=False):
    """:84-197 (without the smoothing and the visualisation): dict of the three means, the stage counts and the flags."""
    verts = np.asarray(verts, dtype=np.float64)
    world = verts * scale + trans
    if faces is None:
        cloud, sampled = world, 0
    else:
        new_pts, _ = sample_mesh(verts if sample_before_transform else world, faces, thresh)
        cloud, sampled = np.concatenate([world, new_pts], axis=0), new_pts.shape[0]
    keep = thin(cloud, thresh, order)
    data_down = cloud[keep]
    in_bb, in_obs = mask_filter(data_down, obs_mask, BB, Res, patch)
    data_in, data_in_obs = data_down[in_bb], data_down[in_obs]
    raw_d2s = nearest_raw(data_in_obs, stl)
    dist_d2s, _ = nearest(data_in_obs, stl, max_dist, raw_d2s)
    used_d2s = dist_d2s[dist_d2s < max_dist]
    above = above_plane(stl, plane)
    raw_s2d = nearest_raw(stl[above], data_in)
    dist_s2d, _ = nearest(stl[above], data_in, max_dist, raw_s2d)
    used_s2d = dist_s2d[dist_s2d < max_dist]
    mean_d2s, mean_s2d = used_d2s.mean(), used_s2d.mean()
    return dict(mean_d2s=mean_d2s, mean_s2d=mean_s2d, overall=(mean_d2s + mean_s2d) / 2, sampled=sampled,
                thinned=data_down.shape[0], in_bb=data_in.shape[0], in_obs=data_in_obs.shape[0], above=int(above.sum()),
                used_d2s=used_d2s.shape[0], used_s2d=used_s2d.shape[0], keep=keep, in_bb_mask=in_bb, in_obs_mask=in_obs,
                dist_d2s=dist_d2s, dist_s2d=dist_s2d, cloud=cloud,
                max_dist_gap=min(edge_gap(raw_d2s[0], max_dist), edge_gap(raw_s2d[0], max_dist)))


# ---- fixtures --------------------------------------------------------------------------------------------------------------
SHEET_THRESH = 0.2


def bumpy_sheet(n=20000, seed=7):
    """n random points of a bumpy sheet with mean spacing about 0.14 (the thinning fixture, thresh 0.2)."""
    rng = np.random.default_rng(seed)
    side = 0.14 * np.sqrt(n)
    xy = rng.uniform(0.0, side, size=(n, 2))
    z = 0.3 * np.sin(xy[:, 0] * 0.9) * np.cos(xy[:, 1] * 0.7) + 0.02 * rng.standard_normal(n)
    return np.concatenate([xy, z[:, None]], axis=1)


def bumpy_sphere(n=50000, radius=30.0, seed=11):
    """n random points of a sphere whose radius varies by a few percent (the nearest-neighbour targets)."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= norm3(d)[:, None]
    r = radius * (1.0 + 0.03 * np.sin(5.0 * d[:, 0]) * np.cos(4.0 * d[:, 1]) + 0.02 * np.sin(7.0 * d[:, 2]))
    return d * r[:, None]


def icosphere(level, radius):
    """(verts (V, 3) float64, faces (F, 3) int64): an icosahedron subdivided `level` times, pushed to `radius`."""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.sqrt(1.0 + t * t) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.sqrt((m * m).sum()))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v) * radius, np.asarray(f, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def sheet_fixture():
    """(points, neighbour lists at SHEET_THRESH, the smallest |d - thresh| over all pairs): computed once per process."""
    pts = bumpy_sheet()
    nbrs, gap = radius_neighbors(pts, SHEET_THRESH, with_gap=True)
    return pts, nbrs, gap


def sheet_order(n, seed=3):
    return np.random.default_rng(seed).permutation(n)


NEAREST_MAX_DIST = 20.0


@functools.lru_cache(maxsize=None)
def nearest_fixture():
    """(targets (50000, 3), queries (5000, 3), brute-force dist, idx, the smallest |d - max_dist|): queries on the surface, 1 - 15 away, just inside
    max_dist, and well beyond it."""
    targets = bumpy_sphere()
    rng = np.random.default_rng(5)
    base = targets[rng.integers(0, targets.shape[0], size=5000)]
    out = base / norm3(base)[:, None]
    off = np.concatenate([0.05 * rng.standard_normal(1250), rng.uniform(1.0, 15.0, 1250), rng.uniform(19.6, 20.4, 1250),
                          rng.uniform(25.0, 90.0, 1250)])
    tangent = 0.2 * rng.standard_normal((5000, 3))
    queries = base + out * off[:, None] + tangent
    raw = nearest_raw(queries, targets)
    dist, idx = nearest(queries, targets, NEAREST_MAX_DIST, raw)
    return targets, queries, dist, idx, edge_gap(raw[0], NEAREST_MAX_DIST)


COMPOSED = dict(thresh=1.5, patch=1.0, max_dist=3.0, scale=50.0, trans=np.array([1.0, -2.0, 0.5]))


@functools.lru_cache(maxsize=None)
def composed_fixture():
    """A synthetic scan and mesh: 40 000 scan points on the sphere of radius 30 about `trans`, the ground plane z = trans_z - 20
    cutting it, an observation mask of 2 mm cells over [-28, 28) x [-28, 28) x [-28, 20) about the centre with a block of
    unobserved cells, and an icosphere of radius 30.5 in normalised coordinates (world = verts * 50 + trans)."""
    c = COMPOSED["trans"]
    rng = np.random.default_rng(17)
    d = rng.standard_normal((40000, 3))
    stl = d / norm3(d)[:, None] * 30.0 + c
    plane = np.array([0.0, 0.0, 1.0, 20.0 - c[2]])
    BB = np.stack([c - 28.0, c + np.array([28.0, 28.0, 20.0])]).astype(np.float32)
    obs = np.ones((29, 29, 25), dtype=np.uint8)
    obs[20:, :6, 10:18] = 0
    verts, faces = icosphere(3, 30.5)
    verts = verts / COMPOSED["scale"]
    n_cloud = verts.shape[0] + sample_mesh(verts * COMPOSED["scale"] + c, faces, COMPOSED["thresh"])[0].shape[0]
    order = np.random.default_rng(23).permutation(n_cloud)
    return dict(stl=stl, plane=plane, BB=BB, Res=np.array([[2.0]]), obs=obs, verts=verts, faces=faces, order=order)
