"""Times the stages of the DTU Chamfer evaluation (ndjir_amd/chamfer.py; python/evaluate_chamfer_dtumvs.py:84-197) at the size
of a DTU scan, on a synthetic workload in millimetres: a wavy sheet of lattice quads with 2^21 vertices 0.6 mm apart (two
triangles per quad, what marching cubes at 512^3 leaves), a scan of 3 M points on the same sheet 0.5 mm above it and shifted
sideways so that part of it has no mesh within max_dist, an observation mask of 2 mm cells with unobserved blocks, a ground
plane under the sheet; thresh = 0.2, max_dist = 20, patch = 60.  Each stage runs once to warm up, then `--repeats` times
between two device events (the stage's waits for sizes included).  `--cpu` also runs the reference's own pipeline (sklearn's
kd-tree, the sequential loop) on the same input on the host, where sklearn is installed, for scale.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ndjir_amd import chamfer
from ndjir_amd import config as cfg

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--log2-vertices", type=int, default=21)
ap.add_argument("--scan-points", type=int, default=3_000_000)
ap.add_argument("--cpu", action="store_true")
args = ap.parse_args()

dev = torch.device("cuda:0")
conf = cfg.load("default")
dt = conf.valid.dtumvs
thresh, patch, max_dist = dt.downsample_density, dt.patch_size, float(dt.max_dist)
f64 = dict(device=dev, dtype=torch.float64)


def sheet(u, v):
    return 12.0 * torch.sin(u / 40.0) * torch.cos(v / 55.0)


nu, nv = 1 << ((args.log2_vertices + 1) // 2), 1 << (args.log2_vertices // 2)
u = (torch.arange(nu, **f64) * 0.6)[:, None].expand(nu, nv)
v = (torch.arange(nv, **f64) * 0.6)[None, :].expand(nu, nv)
verts = torch.stack([u, v, sheet(u, v)], dim=-1).reshape(-1, 3).contiguous()
idx = (torch.arange(nu - 1, device=dev)[:, None] * nv + torch.arange(nv - 1, device=dev)[None, :]).reshape(-1)
faces = torch.cat([torch.stack([idx, idx + nv, idx + nv + 1], dim=1), torch.stack([idx, idx + nv + 1, idx + 1], dim=1)]).to(torch.int32)
extent = np.array([(nu - 1) * 0.6, (nv - 1) * 0.6])

gen = torch.Generator(device=dev)
gen.manual_seed(7)
su = torch.rand(args.scan_points, generator=gen, **f64) * extent[0] + 0.08 * extent[0]      # 8 % of the scan lies beyond the mesh
sv = torch.rand(args.scan_points, generator=gen, **f64) * extent[1]
stl = torch.stack([su, sv, sheet(su, sv) + 0.5 + 0.05 * torch.randn(args.scan_points, generator=gen, **f64)], dim=-1).contiguous()
Res = 2.0
BB = np.array([[0.0, 0.0, -20.0], [extent[0], extent[1], 20.0]], dtype=np.float32)
dims = np.ceil((BB[1] - BB[0]) / Res).astype(int) + 1
obs = torch.ones(tuple(int(d) for d in dims), device=dev, dtype=torch.uint8)
obs[:: 7, :: 5] = 0
plane = np.array([0.0, 0.0, 1.0, 11.0])                        # z > -11: the sheet's troughs lie below


def timed(fn):
    out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) * 1e-3)
    return out, times


res = {"vertices": int(verts.shape[0]), "faces": int(faces.shape[0]), "scan_points": int(stl.shape[0]), "thresh": thresh,
       "max_dist": max_dist, "nearest_cell": max_dist / chamfer.NEAREST_CELLS}
new_pts, res["sample_s"] = timed(lambda: chamfer.sample_mesh_points(verts, faces, thresh))
cloud = torch.cat([verts, new_pts], dim=0)
order = torch.randperm(cloud.shape[0], generator=torch.Generator().manual_seed(0))
(keep, rounds), res["thin_s"] = timed(lambda: chamfer.thin_points(cloud, thresh, order=order, return_rounds=True))
data_down = cloud[keep]
(in_bb, in_obs), res["mask_s"] = timed(lambda: chamfer.mask_points(data_down, obs, BB, Res, patch))
data_in, data_in_obs = data_down[in_bb], data_down[in_obs]
(d2s, _), res["nearest_d2s_s"] = timed(lambda: chamfer.nearest_distances(data_in_obs, stl, max_dist))
above, res["plane_s"] = timed(lambda: chamfer.above_plane(stl, plane))
stl_above = stl[above]
(s2d, _), res["nearest_s2d_s"] = timed(lambda: chamfer.nearest_distances(stl_above, data_in, max_dist))
out, res["evaluate_chamfer_s"] = timed(lambda: chamfer.evaluate_chamfer(verts, faces, stl, obs, BB, Res, plane, conf, order=order))
res.update(sampled=int(new_pts.shape[0]), cloud=int(cloud.shape[0]), thin_rounds=rounds, thinned=int(data_down.shape[0]),
           in_bb=int(data_in.shape[0]), in_obs=int(data_in_obs.shape[0]), above=int(stl_above.shape[0]),
           used_d2s=int((d2s < max_dist).sum()), used_s2d=int((s2d < max_dist).sum()),
           mean_d2s=out["mean_d2s"], mean_s2d=out["mean_s2d"], overall=out["overall"])

if args.cpu:
    try:
        import sklearn.neighbors as skln
    except ImportError:
        res["cpu_s"] = None
    else:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import chamfer_ref as R
        t0 = time.perf_counter()
        pts, _ = R.sample_mesh(verts.cpu().numpy(), faces.cpu().numpy(), thresh)
        t1 = time.perf_counter()
        shuffled = np.concatenate([verts.cpu().numpy(), pts])[order.numpy()]
        engine = skln.NearestNeighbors(n_neighbors=1, radius=thresh, algorithm="kd_tree", n_jobs=-1)
        engine.fit(shuffled)
        rnn = engine.radius_neighbors(shuffled, radius=thresh, return_distance=False)
        mask = np.ones(shuffled.shape[0], dtype=np.bool_)
        for curr, idxs in enumerate(rnn):
            if mask[curr]:
                mask[idxs] = 0
                mask[curr] = 1
        down = shuffled[mask]
        t2 = time.perf_counter()
        bb, ob = R.mask_filter(down, obs.cpu().numpy(), BB, Res, patch)
        scan = stl.cpu().numpy()
        engine.fit(scan)
        d1, _ = engine.kneighbors(down[ob], n_neighbors=1, return_distance=True)
        engine.fit(down[bb])
        d2, _ = engine.kneighbors(scan[R.above_plane(scan, plane)], n_neighbors=1, return_distance=True)
        t3 = time.perf_counter()
        res.update(cpu_sample_s=t1 - t0, cpu_thin_s=t2 - t1, cpu_mask_nearest_s=t3 - t2, cpu_s=t3 - t0, cpu_thinned=int(mask.sum()),
                   cpu_mean_d2s=float(d1[d1 < max_dist].mean()), cpu_mean_s2d=float(d2[d2 < max_dist].mean()))
print(json.dumps(res))
