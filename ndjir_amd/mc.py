"""Marching cubes on the device: an SDF volume to a closed, indexed triangle mesh (csrc/mc.hip).

Reference: `create_mesh_from_volume` (python/extract_by_mc.py:36-43) calls `skimage.measure.marching_cubes` on the CPU.
Here the volume stays on the device and the surface is defined by a rule, from which the 256-case table is generated
(`ndjir_mc_case_table`), not typed:

  * a lattice point is inside iff vol < level (equality, and -0.0 at level 0, are outside);
  * one vertex per lattice edge whose endpoints differ, at index + t, t = (level - v0) / (v1 - v0) in fp32, ordered by
    (point linear index (i * Gy + j) * Gz + k, axis x < y < z); world position pos * scale + mins, an fp32 multiply and then
    an fp32 add, scale = float32((maxs - mins) / (G - 1)) formed in float64;
  * in a cell, each face is walked counter-clockwise as seen from outside; every maximal run of inside corners gives one
    directed segment from the crossing where the run ends to the one where it begins; the segments link into closed loops,
    each cut into a fan.  The neighbouring cell finds the same runs the other way round, so the mesh is closed wherever the
    surface stays inside the volume;
  * faces are ordered by cell, then by the table's order.  Nothing is placed by an atomic: two runs give equal tensors.

Orientation: the loops' right-hand normals point toward decreasing values.  `gradient_direction="descent"` (the
reference's configured default, config/default.yaml:182) delivers the reverse winding -- counter-clockwise seen from the
higher-value side, so the normals of an SDF's surface point outward, as the OBJ normals `save_attributed_mesh` writes do;
"ascent" is the other winding.  UNPINNED: which of the two skimage calls "descent" could not be compared, skimage is not
available where this was written.

Different from the reference on purpose: skimage's Lewiner variant resolves ambiguous faces and cell interiors by extra
tests, this rule is fixed (the vertices are those of any marching cubes; the connectivity can differ in ambiguous cells
only); vertices are fp32 (the reference's are float64 after scaling); there are no `normals` / `values` outputs; one device
holds the whole volume (`extract.gather_volume` first).

The host waits for the device once, to read the two counts before allocating the exact-size outputs.
"""
import ctypes

import numpy as np
import torch

from . import lib

SCAN_BLOCK = 1024            # lattice points per block (csrc/mc.hip MC_BLOCK)
MAX_DIM = 1 << 15
DIRECTIONS = ("descent", "ascent")
_TABLES = {}


def case_table():
    """The 256 x 16 uint8 table the C library generates from the rule: row[0] = number of triangles (<= 5), then three cube
    edges per triangle in the "descent" winding.  Corner bit = dx + 2 dy + 4 dz; cube edge = 4 * axis + rank of its lower
    corner among the four edges of that axis.  Needs no GPU."""
    fn = lib.load().ndjir_mc_case_table
    fn.argtypes, fn.restype = [ctypes.c_void_p], ctypes.c_int
    buf = (ctypes.c_ubyte * 4096)()
    rc = fn(ctypes.cast(buf, ctypes.c_void_p))
    if rc != 0:
        raise lib.NdjirHipError(f"ndjir_mc_case_table failed with status {rc}")
    return np.frombuffer(buf, dtype=np.uint8).reshape(256, 16).copy()


def _device_table(device):
    key = (device.type, device.index)
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(case_table()).to(device)
    return _TABLES[key]


def _empty(device):
    return (torch.empty((0, 3), device=device, dtype=torch.float32), torch.empty((0, 3), device=device, dtype=torch.int32))


def marching_cubes(vol, level=0.0, gradient_direction="descent", mins=None, maxs=None):
    """vol (Gx, Gy, Gz), numpy or torch, cast to fp32 -> (verts (V, 3) float32, faces (F, 3) int32) on the device, by the
    rule in the module docstring.  Lattice coordinates when `mins` / `maxs` are None, else the box they span.  ValueError for
    an input that is not 3-D or not real-valued, an unknown direction, a non-finite volume, a dimension above 2^15 or 2^31
    points or more, and more than 2^31 - 1 vertices or faces.  A dimension below 2 or a volume without a crossing gives
    (0, 3) tensors."""
    if gradient_direction not in DIRECTIONS:
        raise ValueError(f"gradient_direction {gradient_direction!r} is not one of {DIRECTIONS}")
    if (mins is None) != (maxs is None):
        raise ValueError("mins and maxs go together")
    try:
        if not torch.is_tensor(vol):
            vol = torch.from_numpy(np.ascontiguousarray(np.asarray(vol, dtype=np.float32)))
        if vol.is_complex():
            raise TypeError("complex volume")
        device = vol.device
        if device.type != "cuda":
            from . import parameter as P
            device = P.get_device()
        vol = vol.detach().to(device=device, dtype=torch.float32).contiguous()
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"the volume cannot be read as float32: {e}") from e
    if vol.dim() != 3:
        raise ValueError(f"the volume must be 3-D, got shape {tuple(vol.shape)}")
    G = tuple(int(g) for g in vol.shape)
    if min(G) < 2:
        return _empty(device)
    N = G[0] * G[1] * G[2]
    if max(G) > MAX_DIM or N >= 1 << 31:
        raise ValueError(f"volume {G} too large: each dimension <= {MAX_DIM} and fewer than 2^31 points")
    if not bool(torch.isfinite(vol).all()):
        raise ValueError("the volume holds non-finite values")
    if mins is None:
        scale, lo = [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]
    else:
        lo = [float(np.float32(float(mins[a]))) for a in range(3)]
        scale = [float(np.float32((float(maxs[a]) - float(mins[a])) / (G[a] - 1))) for a in range(3)]
    table = _device_table(device)
    nb = -(-N // SCAN_BLOCK)
    code = torch.empty(N, device=device, dtype=torch.int16)
    sums = torch.empty(2 * nb, device=device, dtype=torch.int32)
    counts = torch.empty(4, device=device, dtype=torch.int32)
    lib.call("mc_count", G[0], G[1], G[2], vol, float(level), table, code, sums, counts)
    V, F, over_v, over_f = counts.cpu().tolist()                           # the one wait
    if over_v or over_f:
        raise ValueError("the surface has more than 2^31 - 1 vertices or faces")
    if V == 0:
        return _empty(device)
    verts = torch.empty((V, 3), device=device, dtype=torch.float32)
    faces = torch.empty((F, 3), device=device, dtype=torch.int32)
    vertex_base = torch.empty(N, device=device, dtype=torch.int32)
    lib.call("mc_emit", G[0], G[1], G[2], vol, float(level), table, code, sums, scale, lo, int(gradient_direction == "ascent"),
             vertex_base, verts, V, faces, F)
    return verts, faces
