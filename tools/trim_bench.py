"""Times the stages of the mesh trimming (ndjir_amd/trim.py; python/extract_by_mc.py:77-128) at the size of a DTU scan: 49 synthetic
1200 x 1600 masks (a disc plus speckle per view) dilated by 50 pixels, a 2^21-vertex mesh of lattice quads (a wavy sheet
through the bounding box, two triangles per quad), 49 cameras three units out.  Each stage runs once to warm up, then
`repeats` times between a host clock and a synchronise.  Usage: trim_bench.py [repeats = 3] [views = 49] [log2 vertices = 21]."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ndjir_amd import trim

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
M = int(sys.argv[2]) if len(sys.argv) > 2 else 49
log2n = int(sys.argv[3]) if len(sys.argv) > 3 else 21
H, W, r = 1200, 1600, 50
dev = torch.device("cuda:0")
rng = np.random.RandomState(7)
gen = torch.Generator(device=dev)
gen.manual_seed(7)

yy = torch.arange(H, device=dev, dtype=torch.float32)[:, None]
xx = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
masks = torch.empty((M, H, W), device=dev, dtype=torch.float32)
for i in range(M):
    cy, cx, rad = 600 + rng.randint(-80, 80), 800 + rng.randint(-80, 80), 300 + rng.randint(0, 150)
    masks[i] = (((yy - cy) ** 2 + (xx - cx) ** 2 < rad ** 2) | (torch.rand((H, W), device=dev, generator=gen) < 1e-4)).float()

K = np.array([[2900.0, 0.3, 800.0], [0.0, 2890.0, 600.0], [0.0, 0.0, 1.0]])
poses = []
for i in range(M):
    c = rng.normal(size=3)
    c = 3.0 * c / np.linalg.norm(c)
    z = -c / np.linalg.norm(c)
    a = rng.normal(size=3)
    x = a - z * (a @ z)
    x /= np.linalg.norm(x)
    pose = np.eye(4)
    pose[:3, :3] = np.stack([x, np.cross(z, x), z], axis=1)
    pose[:3, 3] = c
    poses.append(pose.astype(np.float32))
cams = torch.from_numpy(trim.camera_table(np.stack([K] * M), np.stack(poses))).to(dev)

nu, nv = 1 << ((log2n + 1) // 2), 1 << (log2n // 2)
u = torch.linspace(-1, 1, nu, device=dev)[:, None].expand(nu, nv)
v = torch.linspace(-1, 1, nv, device=dev)[None, :].expand(nu, nv)
verts = torch.stack([u, v, 0.3 * torch.sin(5 * u) * torch.cos(4 * v)], dim=-1).reshape(-1, 3).contiguous()
idx = (torch.arange(nu - 1, device=dev)[:, None] * nv + torch.arange(nv - 1, device=dev)[None, :]).reshape(-1)
faces = torch.cat([torch.stack([idx, idx + nv, idx + nv + 1], dim=1), torch.stack([idx, idx + nv + 1, idx + 1], dim=1)]).to(torch.int32)


def timed(fn):
    out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, times


res = {"views": M, "vertices": int(verts.shape[0]), "faces": int(faces.shape[0]), "radius": r}
padded, res["dilate_s"] = timed(lambda: trim.dilate_masks(masks, r))
keep, res["vertex_test_s"] = timed(lambda: trim.points_inside_masks(verts, padded, cams))
(tv, tf), res["trim_mesh_s"] = timed(lambda: trim.trim_mesh(verts, faces, keep))
labels, res["face_components_s"] = timed(lambda: trim.face_components(tf, tv.shape[0]))
(meshes, n), res["split_components_s"] = timed(lambda: trim.split_components(tv, tf, 5))
res.update(kept_vertices=int(tv.shape[0]), kept_faces=int(tf.shape[0]), components=n,
           mesh_faces=[int(f.shape[0]) for _, f in meshes], dilated_fraction=float(padded[:, 1:-1, 1:-1].float().mean()))
print(json.dumps(res))
