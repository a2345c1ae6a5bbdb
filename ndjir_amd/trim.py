"""Trimming an extracted mesh by the camera masks and splitting it into components (csrc/trim.hip).

Reference: `clean_points_by_mask` and `create_trimmed_meshes` (python/extract_by_mc.py:77-128): every mask is dilated with
cv2's 101 x 101 ellipse on the CPU, every vertex is projected into every view in numpy, vertices outside any dilated mask
and the faces that lose a vertex are dropped, and trimesh splits the rest into components ordered by face count.  Here the
masks, cameras and the mesh stay on the device: `dilate_masks` (ndjir_mask_dilate), `points_inside_masks`
(ndjir_points_in_masks), `trim_mesh` (ndjir_compact_flags, ndjir_trim_faces) and `split_components`
(ndjir_face_components, then the compaction again per mesh).  Every result is an integer array or a selection of the input
rows, and equals the reference's exactly (tests/test_gpu_trim.py) -- with two things UNPINNED, because neither cv2 nor
trimesh exists where this was written: the ellipse's row table (`ellipse_half_widths`, OpenCV's expression from memory) and
trimesh's ordering of equal-sized components and merging of vertices.

The host waits for the device only to learn sizes: `trim_mesh` reads its two counts, `split_components` the component
ranking (`torch.unique`) and each mesh's vertex count, `ndjir_face_components` its error code.

Out of scope: `trimesh.Trimesh(process=True)`'s merging of bit-identical vertices (:122; marching-cubes output has none);
`face_adjacency`'s exclusion of edges shared by more than two faces (here such an edge connects all its faces);
`create_largest_meshes` (:131-140, never called by `extract`); sharding over ranks; fp64 vertices (ours are fp32, widened
exactly for the projection).
"""
import numpy as np
import torch

from . import lib

SCAN_BLOCK = 1024           # elements per block of the compaction kernels (csrc/trim.hip TR_SCAN)
MAX_RADIUS = 127


def ellipse_half_widths(r):
    """Row half-widths of `cv.getStructuringElement(cv.MORPH_ELLIPSE, (2r + 1, 2r + 1))`: row dy + r holds the cells
    |dx| <= half[dy + r].  OpenCV's expression as recalled, in float64: rint(r * sqrt((r^2 - dy^2) / r^2)); UNPINNED -- cv2 is
    not available to compare with.  r = 5 gives [0 3 4 5 5 5 5 5 4 3 0]."""
    r = int(r)
    if not 0 <= r <= MAX_RADIUS:
        raise ValueError(f"dilation radius {r} outside [0, {MAX_RADIUS}]")
    if r == 0:
        return np.zeros(1, dtype=np.int32)
    dy = np.arange(-r, r + 1, dtype=np.float64)
    inv_r2 = 1.0 / (float(r) * float(r))
    return np.rint(r * np.sqrt((float(r) * float(r) - dy * dy) * inv_r2)).astype(np.int32)


def dilate_masks(masks, pixel_margin=50):
    """masks (M, H, W) or (M, H, W, 1) float32 on the device, set where >= 0.5 -> (M, H + 2, W + 2) uint8: the masks dilated
    by the ellipse of radius `pixel_margin` inside a one-pixel frame of ones (extract_by_mc.py:89-96)."""
    if masks.dim() == 4:
        masks = masks[..., 0]
    masks = masks.detach().to(torch.float32).contiguous()
    M, H, W = masks.shape
    half = ellipse_half_widths(pixel_margin)
    out = torch.empty((M, H + 2, W + 2), device=masks.device, dtype=torch.uint8)
    row_dist = torch.empty((M, H, W), device=masks.device, dtype=torch.uint8)
    lib.call("mask_dilate", M, H, W, masks, int(pixel_margin), half.tolist(), row_dist, out)
    return out


def camera_table(intrinsics, poses):
    """(M, 21) float64 rows [K | R | t] as the reference forms them on the host (extract_by_mc.py:81-84): R = inv(pose[:3, :3])
    and t = -R @ pose[:3, 3:] in float32 (the reference's poses are float32; ours are kept widened, so they are cast back
    first), K in float64."""
    K = np.asarray(intrinsics.detach().cpu() if torch.is_tensor(intrinsics) else intrinsics, dtype=np.float64)[:, :3, :3]
    pose = np.asarray(poses.detach().cpu() if torch.is_tensor(poses) else poses).astype(np.float32)
    R = np.linalg.inv(pose[:, :3, :3])
    t = -R @ pose[:, :3, 3:]
    M = K.shape[0]
    return np.ascontiguousarray(np.concatenate([K.reshape(M, 9), R.reshape(M, 9).astype(np.float64),
                                                t.reshape(M, 3).astype(np.float64)], axis=1))


def _points(points, device):
    if not torch.is_tensor(points):
        points = torch.from_numpy(np.ascontiguousarray(np.asarray(points, dtype=np.float32)))
    return points.detach().to(device=device, dtype=torch.float32).reshape(-1, 3).contiguous()


def _faces(faces, device):
    if not torch.is_tensor(faces):
        faces = torch.from_numpy(np.ascontiguousarray(np.asarray(faces, dtype=np.int64)))
    return faces.detach().to(device=device, dtype=torch.int32).reshape(-1, 3).contiguous()


def points_inside_masks(points, padded_masks, cams):
    """keep (N,) bool: the vertex projects into the padded, dilated mask of every view (`clean_points_by_mask`).  points
    (N, 3) float32 (numpy or torch); padded_masks from `dilate_masks`; cams from `camera_table` (numpy or a device tensor)."""
    device = padded_masks.device
    pts = _points(points, device)
    M, Hp, Wp = padded_masks.shape
    if not torch.is_tensor(cams):
        cams = torch.from_numpy(np.ascontiguousarray(cams, dtype=np.float64))
    cams = cams.to(device=device, dtype=torch.float64).contiguous()
    if cams.shape != (M, 21):
        raise ValueError(f"camera table {tuple(cams.shape)} does not match {M} masks")
    keep = torch.empty(pts.shape[0], device=device, dtype=torch.uint8)
    lib.call("points_in_masks", pts.shape[0], pts, M, Hp - 2, Wp - 2, padded_masks.contiguous(), cams, keep)
    return keep.bool()


def _workspace(n, device):
    return torch.empty(max(1, -(-n // SCAN_BLOCK)), device=device, dtype=torch.int32)


def _compact_vertices(verts, keep):
    """(new_index (N,) int32, moved rows (N, 3) of which the first count are valid, count (2,) int32 on the device)."""
    N = verts.shape[0]
    new_index = torch.empty(N, device=verts.device, dtype=torch.int32)
    out = torch.empty_like(verts)
    count = torch.empty(2, device=verts.device, dtype=torch.int32)
    lib.call("compact_flags", N, keep.to(torch.uint8).contiguous(), new_index, count, _workspace(N, verts.device), verts, 3, out)
    return new_index, out, count


def _trim_faces(faces, face_keep, n_verts, new_index):
    out = torch.empty_like(faces)
    count = torch.empty(2, device=faces.device, dtype=torch.int32)
    lib.call("trim_faces", faces.shape[0], faces, face_keep, n_verts, new_index, out, count, _workspace(faces.shape[0], faces.device))
    return out, count


def _counts(*counts):
    """The device counts on the host, one wait; a face that names a vertex outside the mesh is an error."""
    host = torch.stack(counts).cpu().tolist()
    if any(bad for _, bad in host):
        raise ValueError("a face names a vertex outside [0, N)")
    return [n for n, _ in host]


def trim_mesh(verts, faces, keep):
    """extract_by_mc.py:111-120: the kept vertices in order, and the faces whose three vertices are kept, in order, with their
    indices remapped.  verts (N, 3), faces (F, 3), keep (N,) bool on the device -> (new_verts float32, new_faces int32)."""
    device = keep.device
    verts, faces = _points(verts, device), _faces(faces, device)
    new_index, moved, cv = _compact_vertices(verts, keep)
    out_faces, cf = _trim_faces(faces, None, verts.shape[0], new_index)
    nv, nf = _counts(cv, cf)
    return moved[:nv], out_faces[:nf]


def face_components(faces, n_verts, slots=None):
    """labels (F,) int32: the smallest face index of each face's component; faces are connected through shared undirected
    edges (ndjir_face_components).  `slots`: size of the edge table, a power of two, by default the first one >= 2 * 3F."""
    F = faces.shape[0]
    labels = torch.empty(F, device=faces.device, dtype=torch.int32)
    if F == 0:
        return labels
    if slots is None:
        slots = 1 << max(1, (6 * F - 1).bit_length())
    keys = torch.empty(slots, device=faces.device, dtype=torch.int64)
    owner = torch.empty(slots, device=faces.device, dtype=torch.int32)
    status = torch.empty(1, device=faces.device, dtype=torch.int32)
    lib.call("face_components", F, faces, n_verts, slots, keys, owner, labels, status)
    return labels


def split_components(verts, faces, max_meshes=None):
    """`new_mesh.split(only_watertight=False)` ordered by face count (extract_by_mc.py:124-126) -> (meshes, n_components):
    meshes = [(verts_k, faces_k), ...] by face count descending, ties by smallest original face index ascending (the
    reference's tie order is whatever `np.argsort(...)[::-1]` yields), at most `max_meshes` of them.  Each mesh keeps its
    faces in the original order and exactly the vertices its faces use, in ascending original index (trimesh's `submesh`);
    vertices no face uses disappear."""
    device = verts.device if torch.is_tensor(verts) else (faces.device if torch.is_tensor(faces) else None)
    if device is None or device.type != "cuda":
        from . import parameter as P
        device = P.get_device()
    verts, faces = _points(verts, device), _faces(faces, device)
    N, F = verts.shape[0], faces.shape[0]
    if F == 0:
        return [], 0
    labels = face_components(faces, N)
    roots, sizes = torch.unique(labels, return_counts=True)              # roots ascending
    order = torch.sort(sizes, descending=True, stable=True)[1]           # stable: equal sizes stay in root order
    n_components = int(roots.shape[0])
    top = roots[order[:n_components if max_meshes is None else int(max_meshes)]]
    meshes = []
    faces64 = faces.to(torch.int64)
    for k in range(top.shape[0]):
        member = labels == top[k]
        used = torch.zeros(N + 1, device=device, dtype=torch.uint8)       # slot N takes the other components' faces
        used.index_fill_(0, torch.where(member[:, None], faces64, N).reshape(-1), 1)
        new_index, moved, cv = _compact_vertices(verts, used[:N])
        out_faces, cf = _trim_faces(faces, member.to(torch.uint8), N, new_index)
        nv, nf = _counts(cv, cf)
        meshes.append((moved[:nv], out_faces[:nf]))
    return meshes, n_components
