"""SDF volume evaluation for mesh extraction.

Reference: `compute_pts_vol` (python/extract_by_mc.py:46-74): G^3 points of a regular lattice through
`geometric_network(...)[0]` in batches of `extraction.batch_size` (50 000), each batch built on the host,
copied to the device, evaluated layer by layer, and its 257-column output copied back.  Here the lattice
points are formed on the device chunk by chunk, the geometric net runs as the fused sdf-only MFMA chain
(grid gather + 8 layers in one launch sequence, only column 0 of the last layer is computed) and the volume
stays on the device until the caller asks for it.

Marching cubes (`create_mesh_from_volume`, :36-43; skimage on the CPU in the reference) runs on the device too
(ndjir_amd/mc.py, csrc/mc.hip): a rule-defined isosurface with a generated case table, fp32 vertices, output order fixed by
prefix sums.  Its vertices are those of any marching cubes; its connectivity can differ from skimage's Lewiner variant in
ambiguous cells, and which winding skimage calls "descent" is UNPINNED (see mc.py).  `extract_scene` is the reference's
whole `extract` (:263-288): volume, mesh, textures, files.

The lattice shards over x-slabs: `slab_range(G, rank, world)`; each rank evaluates its slabs independently
(no collective on the data path), `gather_volume` concatenates them.

Export half (`compute_vertex_colors`, `create_rgb_color`, `save_attributed_mesh`, `extract_environment_map`, `extract`;
extract_by_mc.py:144-261): these take a mesh (vertices and faces), from `create_mesh_from_volume` or the caller's own.
`bake_vertex_attributes` evaluates the geometric net with its gradient once per vertex and the four material nets once on
the packed input, and one head launch (csrc/bake.hip) turns their raw outputs into the six textures -- the reference runs
the geometric net and `nn.grad` six times per vertex, once per texture.  `extract_environment_map` builds the direction
lattice, evaluates the environment light net and quantises on the device.

Trimming (`clean_points_by_mask`, `create_trimmed_meshes`, :77-128): `create_trimmed_meshes` dilates the scene's masks,
tests every vertex against every view, drops what falls outside and splits the rest into components, all on the device
(ndjir_amd/trim.py, csrc/trim.hip) and equal to the reference's integers; `extract(..., source=...)` writes the `trimmed`
meshes.  Out of scope: `create_largest_meshes` (:131-141, never called by `extract`); trimesh's merging of
bit-identical vertices and its exclusion of edges shared by more than two faces; fp64 vertices; sharding the vertices over
ranks.
"""
import os

import numpy as np
import torch

from . import lib
from . import meshio
from .network import geometric_network

# the six textures in the reference's order (extract_by_mc.py:198-208)
TEXTURES = ("base_color", "implicit_illumination", "roughness", "specular_reflectance", "roughness_std",
            "specular_reflectance_std")
_LAST_ACTS = {"softplus": 1, "sigmoid": 2, "relu": 3}


def lattice_axes(mins, maxs, grid_size):
    """The reference's coordinates: float64 `np.linspace`, rounded to fp32 (extract_by_mc.py:48-50)."""
    return [np.linspace(mins[a], maxs[a], grid_size).astype(np.float32) for a in range(3)]


def slab_range(grid_size, rank=0, world=1):
    """x-index range [i0, i1) of `rank`: contiguous slabs, sizes differing by at most one."""
    base, rem = divmod(grid_size, world)
    i0 = rank * base + min(rank, rem)
    return i0, i0 + base + (1 if rank < rem else 0)


def compute_vol(mins, maxs, grid_size, conf, device=None, chunk=1 << 20, rank=0, world=1):
    """vol[i - i0, j, k] = sdf(x_i, y_j, z_k) for this rank's x-slabs, a float32 GPU tensor of shape
    (i1 - i0, G, G) -- the layout `compute_pts_vol` returns after its reshape / transpose (:71)."""
    from . import parameter as P
    device = device or P.get_device()
    G = int(grid_size)
    xs, ys, zs = (torch.from_numpy(a).to(device) for a in lattice_axes(mins, maxs, G))
    i0, i1 = slab_range(G, rank, world)
    n = (i1 - i0) * G * G
    vol = torch.empty(n, device=device, dtype=torch.float32)
    with torch.no_grad():
        for p0 in range(0, n, chunk):
            p1 = min(n, p0 + chunk)
            idx = torch.arange(p0, p1, device=device, dtype=torch.int64) + i0 * G * G
            i = torch.div(idx, G * G, rounding_mode="floor")
            jk = idx - i * (G * G)
            j = torch.div(jk, G, rounding_mode="floor")
            pts = torch.stack([xs[i], ys[j], zs[jk - j * G]], dim=1)
            sdf = geometric_network(pts, conf, first_order_only=True, sdf_only=True)[0]
            vol[p0:p1] = sdf.reshape(-1)
    return vol.view(i1 - i0, G, G)


def gather_volume(local, grid_size, world=1):
    """All ranks' slabs -> the full (G, G, G) volume on every rank (slab sizes may differ by one)."""
    if world == 1:
        return local
    import torch.distributed as dist
    G = int(grid_size)
    parts = [torch.empty((slab_range(G, r, world)[1] - slab_range(G, r, world)[0], G, G), device=local.device,
                         dtype=local.dtype) for r in range(world)]
    dist.all_gather(parts, local.contiguous())
    return torch.cat(parts, dim=0)


def compute_pts_vol(mins, maxs, grid_size, conf, **kw):
    """Reference signature (extract_by_mc.py:46): returns (pts (G^3, 3), vol (G, G, G)) as numpy arrays, pts in the
    reference's meshgrid order."""
    x, y, z = lattice_axes(mins, maxs, grid_size)
    X, Y, Z = np.meshgrid(x, y, z)
    pts = np.stack((X.reshape(-1), Y.reshape(-1), Z.reshape(-1)), axis=1)
    vol = compute_vol(mins, maxs, grid_size, conf, **kw)
    return pts, vol.cpu().numpy()


def create_mesh_from_volume(volume, level, mins, maxs, G, gradient_direction="ascent"):
    """`create_mesh_from_volume` (extract_by_mc.py:36-43, its signature and default): marching cubes over `volume` (G, G, G),
    a numpy array or a tensor, at `level`, the vertices scaled into the box `mins` ... `maxs` (:41).  Returns
    (verts (V, 3) float32, faces (F, 3) int32) on the device -- no trimesh object, no normals (`save_attributed_mesh` takes
    them from the net).  See `mc.marching_cubes` for the rule and what is UNPINNED."""
    from . import mc
    if tuple(volume.shape) != (int(G),) * 3:
        raise ValueError(f"volume of shape {tuple(volume.shape)} is not the ({G}, {G}, {G}) lattice the scale is formed for")
    return mc.marching_cubes(volume, level, gradient_direction, mins, maxs)


def _place(v, dim):
    """`create_rgb_color` (extract_by_mc.py:187-194): clip to [0, 1]; a one-channel output goes to channel `dim` of zeros."""
    v = v.clamp(0.0, 1.0)
    if v.shape[-1] == 3:
        return v
    out = torch.zeros((v.shape[0], 3), device=v.device, dtype=v.dtype)
    out[:, dim:dim + 1] = v
    return out


def bake_vertex_attributes(points, conf, chunk=1 << 18, device=None):
    """The six vertex textures of `save_attributed_mesh` (extract_by_mc.py:197-216) for `points` (N, 3), numpy or torch,
    cast to fp32.  Returns a dict of GPU tensors: the textures of `TEXTURES`, each (N, 3) float32 in [0, 1] with the net's
    output placed as the reference places it (one-channel implicit illumination -> blue, roughness -> green, one-channel
    specular reflectance -> red, other channels 0) and the two `_std` textures divided by their maximum over ALL vertices
    (:215-216), plus `normal` (N, 3), the raw SDF gradient the nets are fed (:156, not normalised), and `sdf` (N, 1).

    Points go through in chunks of `chunk`.  Where `material_nets_raw` evaluates the four nets as one operator, their raw
    outputs go to `ndjir_bake_head`; otherwise (relu nets, weight normalisation, ...) the per-net functions and stock ops do
    the same.  `specular_reflectance_network.fixme=true` raises: the reference's net then returns one constant and no std
    (python/network.py:475-476), which its own `vc[out_index]` (:158-159) indexes into.  Vertices are not sharded over ranks."""
    from . import parameter as P
    from .network import (base_color_network, geometric_network_with_grad, implicit_illumination_network, material_nets_raw,
                          roughness_network, specular_reflectance_network, uses_fused_geometric)
    if conf.specular_reflectance_network.fixme:
        raise ValueError("specular_reflectance_network.fixme=true: the net has no std output to bake "
                         "(python/network.py:475-476 returns a constant, extract_by_mc.py:158-159 indexes it)")
    device = device or P.get_device()
    if not torch.is_tensor(points):
        points = torch.from_numpy(np.ascontiguousarray(np.asarray(points, dtype=np.float32)))
    pts = points.detach().to(device=device, dtype=torch.float32).reshape(-1, 3).contiguous()
    N = pts.shape[0]
    out = {name: torch.empty((N, 3), device=device, dtype=torch.float32) for name in TEXTURES}
    out["normal"] = torch.empty((N, 3), device=device, dtype=torch.float32)
    out["sdf"] = torch.empty((N, 1), device=device, dtype=torch.float32)
    if N == 0:
        return out
    ci, cs = conf.implicit_illumination_network, conf.specular_reflectance_network
    remap = int(conf.specular_brdf.model == "filament" and bool(conf.specular_brdf.remap))
    fused_geo = uses_fused_geometric(conf)
    std_max = torch.zeros(2, device=device, dtype=torch.int32)
    head = None
    for p0 in range(0, N, int(chunk)):
        p1 = min(N, p0 + int(chunk))
        x = pts[p0:p1]
        # the fused geometric pass produces d(sdf)/dx itself; otherwise the normal comes from autograd (as in render_image)
        with (torch.no_grad() if fused_geo else torch.enable_grad()):
            if not fused_geo:
                x = x.clone().requires_grad_(True)
            sdf, feat, _, normal, Z = geometric_network_with_grad(x, conf, packed=True)
        with torch.no_grad():
            x, sdf, feat, normal = x.detach(), sdf.detach(), feat.detach(), normal.detach()
            out["sdf"][p0:p1] = sdf
            out["normal"][p0:p1] = normal
            raws = material_nets_raw(x, feat, normal, conf, packed=Z.detach() if Z is not None else None)
            if head is None:
                head = raws is not None
            if head:
                raw_imp, raw_bc, raw_r, raw_s = (t.contiguous() for t in raws)
                lib.call("bake_head", p1 - p0, raw_imp, raw_bc, raw_r, raw_s, raw_imp.shape[-1], raw_s.shape[-1] // 2,
                         _LAST_ACTS[ci.act_last], float(ci.inverse_black_degree), remap, float(conf.roughness_network.lower_bound),
                         float(cs.upper_bound_scale), [out[name][p0:p1] for name in TEXTURES], std_max)
            else:
                r, r_std = roughness_network(x, feat, normal, conf)
                s, s_std = specular_reflectance_network(x, feat, normal, conf)
                for name, v, dim in (("base_color", base_color_network(x, feat, normal, conf), 0),
                                     ("implicit_illumination", implicit_illumination_network(x, feat, normal, conf), 2),
                                     ("roughness", r, 1), ("specular_reflectance", s, 0), ("roughness_std", r_std, 1),
                                     ("specular_reflectance_std", s_std, 0)):
                    out[name][p0:p1] = _place(v, dim)
    if head:
        lib.call("bake_scale", N, out["roughness_std"], out["specular_reflectance_std"], std_max)
    else:
        for name in ("roughness_std", "specular_reflectance_std"):
            out[name].div_(out[name].max())
    return out


def environment_map_directions(H, device=None):
    """The (H * 2H, 3) lattice of light directions of extract_by_mc.py:227-237 (ndjir_envmap_directions)."""
    from . import parameter as P
    device = device or P.get_device()
    dirs = torch.empty((H * 2 * H, 3), device=device, dtype=torch.float32)
    lib.call("envmap_directions", H, dirs)
    return dirs


def quantize_environment_map(intensity, H, W, sigmoid_mode):
    """extract_by_mc.py:242-255 on the device: intensity (H * W, C) float32 -> uint8 (H, W, 3) or (H, W), the pixels a reader
    decodes from the reference's file (ndjir_envmap_quantize).  Returns (image, min_max), min_max a (2,) device tensor."""
    C = intensity.shape[-1]
    x = intensity.detach().reshape(H * W, C).contiguous()
    m, M = torch.aminmax(x)
    min_max = torch.stack([m, M])
    image = torch.empty((H, W, 3) if C == 3 else (H, W), device=x.device, dtype=torch.uint8)
    lib.call("envmap_quantize", H, W, C, x, min_max, int(bool(sigmoid_mode)), image)
    return image, min_max


def extract_environment_map(dirname, conf, H=256):
    """`extract_environment_map` (extract_by_mc.py:226-261): writes `environment_map.png` and
    `environment_map_min_max.txt` into `dirname`; returns dict(image uint8 ndarray, min, max, intensity (H * 2H, C) GPU
    tensor).  For three channels the file's RGB is the net's RGB; for one channel the image is mirrored left-right, as
    the reference's is (:255, sic)."""
    from .network import environment_light_network
    W = 2 * H
    with torch.no_grad():
        dirs = environment_map_directions(H)
        intensity = environment_light_network(dirs.view(1, 1, H * W, 3), conf).reshape(H * W, -1)
        if not bool(torch.isfinite(intensity).all()):
            raise ValueError("environment light network returned non-finite intensities")
        image, min_max = quantize_environment_map(intensity, H, W, conf.environment_light_network.act_last == "sigmoid")
    m, M = (np.float32(v) for v in min_max.cpu().numpy())
    image = image.cpu().numpy()
    meshio.write_png(os.path.join(dirname, "environment_map.png"), image)
    meshio.write_min_max(os.path.join(dirname, "environment_map_min_max.txt"), m, M)
    return dict(image=image, min=m, max=M, intensity=intensity)


def save_attributed_mesh(dirname, fname, verts, faces, conf, train=False, type="raw", idx=0):
    """`save_attributed_mesh` (extract_by_mc.py:197-223) for a mesh the caller brings: bakes once and writes the six files
    `{fname}_{G}grid_{type}_{texture}_mesh{idx:02d}.obj` (vertex colours = the texture, vertex normals = the normalised SDF
    gradient); returns the last path, like the reference."""
    G = conf.extraction.rough_grid_size if train else conf.extraction.grid_size
    verts = np.ascontiguousarray(np.asarray(verts.detach().cpu() if torch.is_tensor(verts) else verts, dtype=np.float32)).reshape(-1, 3)
    faces = np.asarray(faces.detach().cpu() if torch.is_tensor(faces) else faces).reshape(-1, 3)
    baked = bake_vertex_attributes(verts, conf)
    normals = meshio.normalize_rows(baked["normal"].cpu().numpy())
    fpath = None
    for name in TEXTURES:
        fpath = f"{dirname}/{fname}_{G}grid_{type}_{name}_mesh{idx:02d}.obj"
        meshio.write_obj(fpath, verts, faces, colors=baked[name].cpu().numpy(), normals=normals)
    return fpath


def create_trimmed_meshes(verts, faces, source, conf, pixel_margin=50, max_meshes=5):
    """`create_trimmed_meshes` (extract_by_mc.py:105-128) for the scene of `source` (an `IDRRaySource`: masks, intrinsics and
    poses on the device): the vertices that project into every view's mask, dilated by `pixel_margin` pixels, the faces they
    keep, split into components.  Returns [(verts_k, faces_k), ...] on the device, largest first (`trim.split_components`),
    at most `max_meshes`; [] when nothing survives.  The image size is the masks' (the reference hard-codes 1600 x 1200)."""
    from . import trim
    masks = source.masks.view(source._size, source._H, source._W)
    padded = trim.dilate_masks(masks, pixel_margin)
    cams = trim.camera_table(source.intrinsics, source.poses)
    keep = trim.points_inside_masks(verts, padded, cams)
    new_verts, new_faces = trim.trim_mesh(verts, faces, keep)
    if new_faces.shape[0] == 0:
        return []
    return trim.split_components(new_verts, new_faces, max_meshes)[0]


def extract(dirname, fname, conf, verts, faces, train=False, source=None):
    """`extract` (extract_by_mc.py:263-288) without its marching-cubes step: the environment map, then the raw mesh `verts`,
    `faces` with its six textures; with a `source` (an `IDRRaySource`) and not `train`, also the trimmed meshes
    `..._trimmed_..._mesh{k:02d}.obj` for k = min(n, 5) - 1 ... 0 (:281-286; whether the scene is a DTU scan, the reference's
    `check_dtu_data`, is the caller's decision).  Returns the last mesh path."""
    extract_environment_map(dirname, conf)
    fpath = save_attributed_mesh(dirname, fname, verts, faces, conf, train, "raw", 0)
    if source is not None and not train:
        meshes = create_trimmed_meshes(verts, faces, source, conf)
        for k in range(min(len(meshes), 5) - 1, -1, -1):
            fpath = save_attributed_mesh(dirname, fname, meshes[k][0], meshes[k][1], conf, train, "trimmed", k)
    return fpath


def extract_scene(dirname, fname, conf, train=False, source=None):
    """The reference's whole `extract` (extract_by_mc.py:263-288), from the loaded parameters to the files: the SDF volume
    over [-r, r]^3, r = `renderer.bounding_sphere_radius`, at `extraction.rough_grid_size` (train) or `extraction.grid_size`
    points per axis, marching cubes at `extraction.level` with `extraction.gradient_direction`, then `extract` with that
    mesh.  ValueError when the level set does not cross the volume.  Returns the last mesh path."""
    radius = float(conf.renderer.bounding_sphere_radius)
    mins, maxs = np.asarray([-radius] * 3), np.asarray([+radius] * 3)
    G = int(conf.extraction.rough_grid_size if train else conf.extraction.grid_size)
    vol = compute_vol(mins, maxs, G, conf)
    verts, faces = create_mesh_from_volume(vol, conf.extraction.level, mins, maxs, G, conf.extraction.gradient_direction)
    if faces.shape[0] == 0:
        lo, hi = (float(v) for v in torch.aminmax(vol))
        raise ValueError(f"no surface at level {conf.extraction.level}: the volume's values span [{lo}, {hi}]")
    return extract(dirname, fname, conf, verts, faces, train, source)
