"""DTU Chamfer distance of an extracted mesh on the device (csrc/chamfer.hip).

Reference: `evaluate_by_chamfer` (python/evaluate_chamfer_dtumvs.py:54-207, borrowed from DTUeval-python), the last step of
the reference's `validate()` (python/train.py:99-118).  It samples points from the triangles in a process pool, thins the
cloud to one point per `downsample_density` with a kd-tree and a sequential loop, filters it by the scan's observation
mask, and averages the nearest-neighbour distances below `max_dist` in both directions.  Here every stage is a kernel and
the clouds stay on the device, in float64 like the reference's arrays:

    sample_mesh_points   :92-108   ndjir_chamfer_tri_rows / _row_counts / _emit_points (+ _scan)
    thin_points          :119-133  ndjir_chamfer_cell_keys, ndjir_chamfer_thin_round until nothing is undecided
    mask_points          :141-149  ndjir_chamfer_mask_points
    above_plane          :166-170  ndjir_chamfer_above_plane
    nearest_distances    :158-159, :172-173  ndjir_chamfer_nearest over a sparse uniform grid
    evaluate_chamfer     :84-197   the stages composed; mode 'pcd' is the same call with faces=None

Each stage equals a numpy restatement of the reference's expressions exactly (tests/chamfer_ref.py, tests/test_gpu_chamfer.py;
nearest distances to the last bit or two).  What differs from the reference, on purpose:

* The shuffle.  The reference shuffles the cloud with an unseeded generator (:119-120), so its result changes from run to
  run.  Here the processing order is an explicit permutation `order` (point order[k] is visited k-th), by default
  `torch.randperm` from a CPU generator seeded with `seed`: reproducible on every device.  For a given order the kept set is
  the reference's: the greedy loop has one answer, which the rounds of ndjir_chamfer_thin_round reach in parallel.
* Sampling order.  The reference takes `tri_vert = vertices[triangles]` BEFORE `vertices * ds.scale + ds.trans` (:84-88): its
  samples are generated in normalised coordinates with `thresh` in millimetres -- marching-cubes edges of about 0.005 give
  n1 = n2 = 0, no samples at all -- and are never moved to world space, while the vertices are.  Upstream DTUeval samples
  in world space.  `evaluate_chamfer` samples AFTER the transform by default; `sample_before_transform=True` reproduces the
  reference's order (samples from the untransformed vertices, left untransformed).
* Neighbours beyond `max_dist` are not searched: only distances < max_dist enter the means (:162, :174), so the bounded
  search is the complete semantics; such a query reports +inf / -1 where the reference holds a distance it then ignores.

Out of scope: `filter_smooth_simple` (:81; open3d is not available to pin it against -- the caller passes the mesh to
evaluate, so the number of the default `valid.filter_iters: 2` is not reproducible yet); the two visualisation PLYs
(:177-192; the returned distances and flags are everything they are made from); the nnabla monitors; sharding over ranks.
UNPINNED: sklearn's kd-tree where it is not installed (the CPU tests compare against it where it is), scipy's `loadmat`
layout of the DTU `.mat` files (`load_dtu_reference`; no DTU file is available here).

The host waits for the device to learn sizes: twice per sampling (rows, points), once per thinning round (the count of
undecided points), once per grid (its bounding box).
"""
import os

import numpy as np
import torch

from . import lib

SCAN_BLOCK = 1024           # elements per block of the scan kernels (csrc/chamfer.hip CH_SCAN)
MAX_CELLS = 1 << 20         # cells per axis of a grid (CH_MAX_DIM)
NEAREST_CELLS = 8           # nearest_distances: cells per max_dist (h = max_dist / 8)


def _device(*xs):
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    from . import parameter as P
    return P.get_device()


def _points(points, device):
    """(n, 3) float64 on the device; float32 input is widened exactly."""
    if not torch.is_tensor(points):
        points = torch.from_numpy(np.ascontiguousarray(np.asarray(points, dtype=np.float64)))
    return points.detach().to(device=device, dtype=torch.float64).reshape(-1, 3).contiguous()


def _faces(faces, device):
    if not torch.is_tensor(faces):
        faces = torch.from_numpy(np.ascontiguousarray(np.asarray(faces, dtype=np.int64)))
    return faces.detach().to(device=device, dtype=torch.int32).reshape(-1, 3).contiguous()


def _host(x):
    return np.asarray(x.detach().cpu() if torch.is_tensor(x) else x)


def _scan(vals):
    """(exclusive prefix sums, counts (2,) int32 on the device: total, overflow)."""
    n = vals.shape[0]
    offsets = torch.empty_like(vals)
    counts = torch.empty(2, device=vals.device, dtype=torch.int32)
    workspace = torch.empty(max(1, -(-n // SCAN_BLOCK)), device=vals.device, dtype=torch.int32)
    lib.call("chamfer_scan", n, vals, offsets, workspace, counts)
    return offsets, counts


def sample_mesh_points(verts, faces, thresh, return_counts=False):
    """:92-108: the points `sample_single_tri` yields for every triangle, concatenated in triangle order -> (S, 3) float64 on
    the device (with `return_counts`, also the number of points per triangle, (F,) int64).  Raises OverflowError if a
    triangle's n1 or n2 exceeds 32767 or the cloud would exceed 2^31 - 1 points."""
    device = _device(verts, faces)
    verts, faces = _points(verts, device), _faces(faces, device)
    N, F = verts.shape[0], faces.shape[0]
    i32 = dict(device=device, dtype=torch.int32)
    rows, n2, flags = torch.empty(F, **i32), torch.empty(F, **i32), torch.empty(2, **i32)
    lib.call("chamfer_tri_rows", N, verts, F, faces, float(thresh), rows, n2, flags)
    tri_row_off, row_total = _scan(rows)
    too_big, bad_index, R, rows_overflow = torch.cat([flags, row_total]).cpu().tolist()
    if bad_index:
        raise ValueError("a face names a vertex outside [0, N)")
    if too_big or rows_overflow:
        raise OverflowError("sample_mesh_points: a triangle is too large for thresh (n1 or n2 > 32767), or too many rows")
    row_tri, row_cnt = torch.empty(R, **i32), torch.empty(R, **i32)
    lib.call("chamfer_row_counts", F, rows, n2, tri_row_off, R, row_tri, row_cnt)
    row_pt_off, pt_total = _scan(row_cnt)
    S, overflow = pt_total.cpu().tolist()
    if overflow:
        raise OverflowError("sample_mesh_points: more than 2^31 - 1 points")
    points = torch.empty((S, 3), device=device, dtype=torch.float64)
    lib.call("chamfer_emit_points", N, verts, faces, rows, n2, tri_row_off, R, row_tri, row_cnt, row_pt_off, S, points)
    if return_counts:
        counts = torch.zeros(F, device=device, dtype=torch.int64)
        counts.index_add_(0, row_tri.to(torch.int64), row_cnt.to(torch.int64))
        return points, counts
    return points


class _Grid:
    """A cloud sorted into a sparse uniform grid of cell size h: `points` and `keys` in key order, `perm[k]` = the input
    index of sorted point k."""

    def __init__(self, points, h):
        h = float(h)
        if not h > 0:
            raise ValueError("cell size must be positive")
        box = torch.stack([points.min(dim=0).values, points.max(dim=0).values]).cpu().tolist()      # one wait
        if not np.isfinite(box).all():
            raise ValueError("points must be finite")
        self.origin, self.h = box[0], h
        # the kernel's own expression for the farthest point; cells do not decrease with the coordinate
        self.dims = [int(np.floor((hi - lo) / h)) + 1 for lo, hi in zip(*box)]
        if max(self.dims) > MAX_CELLS:
            raise ValueError(f"the cloud spans {max(self.dims)} cells of size {h} along an axis (at most {MAX_CELLS})")
        keys = torch.empty(points.shape[0], device=points.device, dtype=torch.int64)
        lib.call("chamfer_cell_keys", points.shape[0], points, self.origin, h, self.dims, keys)
        self.keys, self.perm = torch.sort(keys)
        self.points = points[self.perm].contiguous()


def thin_points(points, thresh, order=None, seed=0, return_rounds=False):
    """:119-133: keep (N,) bool in the input order: point order[k] is visited k-th and kept iff no point kept before it lies
    within `thresh` (d <= thresh, as `radius_neighbors`).  `order`: a permutation of range(N); default `torch.randperm(N)`
    from a CPU generator seeded with `seed` (the reference's unseeded shuffle, made reproducible)."""
    device = _device(points)
    points = _points(points, device)
    N = points.shape[0]
    keep = torch.zeros(N, device=device, dtype=torch.bool)
    if N == 0:
        return (keep, 0) if return_rounds else keep
    if order is None:
        order = torch.randperm(N, generator=torch.Generator().manual_seed(int(seed)))
    elif not torch.is_tensor(order):
        order = torch.from_numpy(np.ascontiguousarray(np.asarray(order, dtype=np.int64)))
    order = order.to(device=device, dtype=torch.int64).reshape(-1)
    rank = torch.full((N,), -1, device=device, dtype=torch.int32)
    if order.shape[0] != N or int(order.min()) < 0 or int(order.max()) >= N:
        raise ValueError("order must be a permutation of range(N)")
    rank[order] = torch.arange(N, device=device, dtype=torch.int32)
    if int(rank.min()) < 0:
        raise ValueError("order must be a permutation of range(N)")
    grid = _Grid(points, thresh)
    srank = rank[grid.perm].contiguous()
    state = [torch.zeros(N, device=device, dtype=torch.uint8), torch.empty(N, device=device, dtype=torch.uint8)]
    undecided = torch.empty(1, device=device, dtype=torch.int32)
    left, rounds = N, 0
    while left:
        lib.call("chamfer_thin_round", N, grid.points, grid.keys, srank, grid.origin, float(thresh), grid.dims, state[0], state[1],
                 undecided)
        state.reverse()
        rounds += 1
        now = int(undecided.item())
        if now >= left:
            raise RuntimeError(f"thinning stalled: {now} points undecided after round {rounds}, {left} before")
        left = now
    keep[grid.perm] = state[0] == 1
    return (keep, rounds) if return_rounds else keep


def mask_points(points, obs_mask, BB, Res, patch):
    """:141-149 -> (in_bb, in_obs), (N,) bool each: inside the padded bounding box, and additionally inside the observation
    mask.  obs_mask (X, Y, Z), BB (2, 3), Res a number or a one-element array (as `loadmat` returns it).  BB is rounded to
    float32 and BB[0] - patch, BB[1] + 2 patch are formed in numpy's float32 arithmetic as at :139, :142."""
    device = _device(points, obs_mask)
    points = _points(points, device)
    if not torch.is_tensor(obs_mask):
        obs_mask = torch.from_numpy(np.ascontiguousarray(np.asarray(obs_mask) != 0).view(np.uint8))
    obs_mask = (obs_mask != 0).to(device=device, dtype=torch.uint8).contiguous()
    if obs_mask.dim() != 3:
        raise ValueError("obs_mask must be (X, Y, Z)")
    BB = _host(BB).astype(np.float32).reshape(2, 3)
    lo = (BB[0] - patch).astype(np.float64)
    hi = (BB[1] + patch * 2).astype(np.float64)
    res = float(np.asarray(_host(Res), dtype=np.float64).reshape(-1)[0])
    N = points.shape[0]
    in_bb = torch.empty(N, device=device, dtype=torch.uint8)
    in_obs = torch.empty(N, device=device, dtype=torch.uint8)
    lib.call("chamfer_mask_points", N, points, lo.tolist(), hi.tolist(), BB[0].astype(np.float64).tolist(), res,
             list(obs_mask.shape), obs_mask, in_bb, in_obs)
    return in_bb.bool(), in_obs.bool()


def above_plane(points, plane):
    """:166-170: (N,) bool, `(P * [x, y, z, 1]).sum(-1) > 0` for the ground plane P (4 numbers, any shape)."""
    device = _device(points)
    points = _points(points, device)
    plane = np.asarray(_host(plane), dtype=np.float64).reshape(-1)
    if plane.shape[0] != 4:
        raise ValueError("plane must hold 4 numbers")
    above = torch.empty(points.shape[0], device=device, dtype=torch.uint8)
    lib.call("chamfer_above_plane", points.shape[0], points, plane.tolist(), above)
    return above.bool()


def nearest_distances(queries, targets, max_dist):
    """For every query the nearest target closer than max_dist -> (dist (Q,) float64, idx (Q,) int32 into `targets`); +inf and
    -1 where no target lies within max_dist.  `dist` is the exact minimum of the float64 distances."""
    device = _device(queries, targets)
    queries, targets = _points(queries, device), _points(targets, device)
    Q, T = queries.shape[0], targets.shape[0]
    max_dist = float(max_dist)
    if not max_dist > 0:
        raise ValueError("max_dist must be positive")
    dist = torch.full((Q,), float("inf"), device=device, dtype=torch.float64)
    idx = torch.full((Q,), -1, device=device, dtype=torch.int32)
    if Q == 0 or T == 0:
        return dist, idx
    grid = _Grid(targets, max_dist / NEAREST_CELLS)
    lib.call("chamfer_nearest", Q, queries, T, grid.points, grid.keys, grid.origin, grid.h, grid.dims, max_dist, dist, idx)
    found = idx >= 0
    idx = torch.where(found, grid.perm[idx.clamp(min=0).to(torch.int64)].to(torch.int32), idx)
    return dist, idx


def _mean(dist, max_dist, stage):
    used = dist[dist < max_dist]
    if used.numel() == 0:
        raise ValueError(f"{stage}: no distance below max_dist = {max_dist} to average")
    return float(used.sum(dtype=torch.float64).item() / used.numel()), int(used.numel())


def evaluate_chamfer(verts, faces, stl_points, obs_mask, BB, Res, plane, conf, scale=1.0, trans=0, order=None, seed=0,
                     sample_before_transform=False):
    """:84-197.  verts (N, 3) in the model's normalised coordinates, faces (F, 3) or None (mode 'pcd': `verts` is the cloud);
    scale, trans: the data source's `vertices * scale + trans` to world millimetres (:88); stl_points, obs_mask, BB, Res,
    plane: the scan's reference data (`load_dtu_reference`); conf.valid.dtumvs.{downsample_density, patch_size, max_dist}.
    `order` / `seed`: the thinning order over the cloud [vertices, samples] (`thin_points`).  Returns a dict: mean_d2s, mean_s2d,
    overall; counts (sampled, thinned, in_bb, in_obs, above, used_d2s, used_s2d); per-point tensors on the device (data_down,
    in_bb, in_obs, dist_d2s for the points in_obs, above, dist_s2d for the scan points above the plane); thin_rounds."""
    dt = conf.valid.dtumvs
    thresh, patch, max_dist = dt.downsample_density, dt.patch_size, float(dt.max_dist)
    device = _device(verts, stl_points)
    verts = _points(verts, device)
    trans_t = torch.as_tensor(_host(trans), dtype=torch.float64).to(device)
    world = verts * float(scale) + trans_t                                                       # :88
    if faces is None:
        cloud, sampled = world, 0
    else:
        new_pts = sample_mesh_points(verts if sample_before_transform else world, faces, thresh)
        cloud, sampled = torch.cat([world, new_pts], dim=0), int(new_pts.shape[0])                 # :109
    keep, rounds = thin_points(cloud, thresh, order=order, seed=seed, return_rounds=True)
    data_down = cloud[keep]
    in_bb, in_obs = mask_points(data_down, obs_mask, BB, Res, patch)
    data_in, data_in_obs = data_down[in_bb], data_down[in_obs]
    stl = _points(stl_points, device)
    dist_d2s, _ = nearest_distances(data_in_obs, stl, max_dist)                                  # :158-159
    mean_d2s, used_d2s = _mean(dist_d2s, max_dist, "data to scan (d2s)")
    above = above_plane(stl, plane)
    dist_s2d, _ = nearest_distances(stl[above], data_in, max_dist)                               # :172-173: data_in, not data_in_obs
    mean_s2d, used_s2d = _mean(dist_s2d, max_dist, "scan to data (s2d)")
    return dict(mean_d2s=mean_d2s, mean_s2d=mean_s2d, overall=(mean_d2s + mean_s2d) / 2,
                sampled=sampled, thinned=int(data_down.shape[0]), in_bb=int(data_in.shape[0]), in_obs=int(data_in_obs.shape[0]),
                above=int(above.sum().item()), used_d2s=used_d2s, used_s2d=used_s2d, thin_rounds=rounds,
                data_down=data_down, in_bb_mask=in_bb, in_obs_mask=in_obs, dist_d2s=dist_d2s, above_mask=above, dist_s2d=dist_s2d)


def load_dtu_reference(ref_dir, scan):
    """The scan's reference data as the reference reads it (:137-139, :153, :166): (stl_points (T, 3) float64, ObsMask (X, Y, Z),
    BB (2, 3) float32, Res, plane (4,)) from `ObsMask/ObsMask{scan}_10.mat`, `ObsMask/Plane{scan}.mat` and
    `Points/stl/stl{scan:03}_total.ply`."""
    try:
        from scipy.io import loadmat
    except ImportError as e:
        raise ImportError("load_dtu_reference reads DTU's .mat files with scipy.io.loadmat; scipy is not installed") from e
    from . import meshio
    scan = int(str(scan).split("scan")[-1])
    obs = loadmat(os.path.join(ref_dir, "ObsMask", f"ObsMask{scan}_10.mat"))
    plane = loadmat(os.path.join(ref_dir, "ObsMask", f"Plane{scan}.mat"))["P"]
    stl = meshio.read_ply_points(os.path.join(ref_dir, "Points", "stl", f"stl{scan:03}_total.ply"))
    return (stl, np.ascontiguousarray(obs["ObsMask"]), obs["BB"].astype(np.float32), obs["Res"],
            np.asarray(plane, dtype=np.float64).reshape(4))
