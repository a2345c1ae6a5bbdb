"""Writers of the mesh export: Wavefront OBJ with per-vertex colours, 8-bit PNG, the environment map's min/max note; and the
reader of a PLY point cloud's positions (`read_ply_points`, the scan of the Chamfer evaluation).

Reference: `mesh.export(fpath, "obj")` through trimesh (python/extract_by_mc.py:217-219) and `cv.imwrite`
(:257-258).  BOTH FORMATS ARE UNPINNED: neither trimesh nor cv2 is available here, so the bytes of the reference's files
cannot be compared; what is kept is the content a reader gets back.  One difference is deliberate: trimesh quantises
vertex colours to 8 bits when they are assigned (`mesh.visual.vertex_colors = ...`, :217), this writer keeps the fp32
values (`%.9g` round-trips fp32 exactly).  Standard library and numpy only.

OBJ layout: `v x y z r g b` per vertex, `vn nx ny nz` per vertex (optional), `f a//a b//b c//c` (or `f a b c` without
normals), indices 1-based.  PNG: 8-bit grey (H, W) or RGB (H, W, 3), one IDAT chunk, filter type 0 on every row.
"""
import struct
import zlib

import numpy as np


def normalize_rows(v, eps=1e-30):
    """Rows of v scaled to unit length (a zero row stays zero)."""
    v = np.asarray(v, dtype=np.float32)
    n = np.sqrt((v.astype(np.float64) ** 2).sum(axis=1, keepdims=True))
    return (v / np.maximum(n, eps)).astype(np.float32)


def write_obj(path, verts, faces, colors=None, normals=None):
    """verts (N, 3), colors (N, 3) or None, normals (N, 3) or None (written as given), faces (F, 3) 0-based integers."""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    N = verts.shape[0]
    if faces.size and (faces.min() < 0 or faces.max() >= N):
        raise ValueError("face index out of range")
    rows = verts
    if colors is not None:
        colors = np.asarray(colors, dtype=np.float32).reshape(-1, 3)
        if colors.shape[0] != N:
            raise ValueError("one colour per vertex")
        rows = np.concatenate([verts, colors], axis=1)
    with open(path, "w") as fp:
        np.savetxt(fp, rows, fmt="v" + " %.9g" * rows.shape[1])
        if normals is not None:
            normals = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
            if normals.shape[0] != N:
                raise ValueError("one normal per vertex")
            np.savetxt(fp, normals, fmt="vn %.9g %.9g %.9g")
            f1 = np.repeat(faces + 1, 2, axis=1)
            np.savetxt(fp, f1, fmt="f %d//%d %d//%d %d//%d")
        else:
            np.savetxt(fp, faces + 1, fmt="f %d %d %d")
    return path


def read_obj(path):
    """The arrays `write_obj` wrote: dict(verts, colors | None, normals | None, faces 0-based)."""
    v, vn, f = [], [], []
    with open(path) as fp:
        for line in fp:
            t = line.split()
            if not t:
                continue
            if t[0] == "v":
                v.append([np.float32(s) for s in t[1:]])
            elif t[0] == "vn":
                vn.append([np.float32(s) for s in t[1:4]])
            elif t[0] == "f":
                f.append([int(s.split("/")[0]) - 1 for s in t[1:4]])
    v = np.asarray(v, dtype=np.float32).reshape(len(v), -1)
    return dict(verts=v[:, :3], colors=v[:, 3:6] if v.shape[1] >= 6 else None,
                normals=np.asarray(vn, dtype=np.float32).reshape(-1, 3) if vn else None,
                faces=np.asarray(f, dtype=np.int64).reshape(-1, 3))


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_ply_points(path):
    """The vertex positions of a PLY file, (N, 3) float64 (`o3d.io.read_point_cloud(...).points`,
    python/evaluate_chamfer_dtumvs.py:153-154): `format ascii 1.0` or `binary_little_endian 1.0`, the `vertex` element
    first, scalar properties only in it; `x`, `y`, `z` are read, every other property (DTU's `stl###_total.ply` carries
    normals and colours) and every later element is skipped."""
    with open(path, "rb") as fp:
        if fp.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, n_vertex, props, element, elements = None, None, [], None, []
        while True:
            line = fp.readline()
            if not line:
                raise ValueError(f"{path}: the header does not end")
            t = line.decode("ascii", errors="replace").split()
            if not t or t[0] in ("comment", "obj_info"):
                continue
            if t[0] == "end_header":
                break
            if t[0] == "format":
                fmt = t[1]
            elif t[0] == "element":
                element = t[1]
                elements.append(element)
                if element == "vertex":
                    n_vertex = int(t[2])
            elif t[0] == "property" and element == "vertex":
                if t[1] == "list" or t[1] not in _PLY_TYPES:
                    raise ValueError(f"{path}: vertex property {' '.join(t[1:])} is not a scalar")
                props.append((t[2], _PLY_TYPES[t[1]]))
        names = [n for n, _ in props]
        if n_vertex is None or elements[0] != "vertex" or any(a not in names for a in "xyz"):
            raise ValueError(f"{path}: the first element must be `vertex` with properties x, y, z")
        if fmt == "ascii":
            rows = np.loadtxt(fp, dtype=np.float64, max_rows=n_vertex, ndmin=2) if n_vertex else np.zeros((0, len(props)))
            if rows.shape != (n_vertex, len(props)):
                raise ValueError(f"{path}: expected {n_vertex} vertex rows of {len(props)} numbers")
            return np.ascontiguousarray(rows[:, [names.index(a) for a in "xyz"]])
        if fmt != "binary_little_endian":
            raise ValueError(f"{path}: format {fmt} is not supported (ascii, binary_little_endian)")
        dtype = np.dtype([(n, "<" + c) for n, c in props])
        rows = np.frombuffer(fp.read(n_vertex * dtype.itemsize), dtype=dtype)
        if rows.shape[0] != n_vertex:
            raise ValueError(f"{path}: expected {n_vertex} vertices, found {rows.shape[0]}")
        return np.stack([rows[a].astype(np.float64) for a in "xyz"], axis=1)


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, image):
    """image: uint8 (H, W) grey or (H, W, 3) RGB."""
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim not in (2, 3) or (image.ndim == 3 and image.shape[2] != 3) or image.size == 0:
        raise ValueError("write_png: uint8 (H, W) or (H, W, 3)")
    H, W = image.shape[:2]
    rows = np.ascontiguousarray(image).reshape(H, -1)
    raw = np.concatenate([np.zeros((H, 1), np.uint8), rows], axis=1).tobytes()      # filter type 0 in front of every row
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 0 if image.ndim == 2 else 2, 0, 0, 0)
    with open(path, "wb") as fp:
        fp.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw, 6)) + _chunk(b"IEND", b""))
    return path


def write_min_max(path, m, M):
    """python/extract_by_mc.py:259-261; the numbers as `str` prints them (for fp32 scalars: the shortest digits that
    round-trip, whatever the numpy version's `format` does)."""
    with open(path, "w") as fp:
        fp.write(f"min, max = {str(m)}, {str(M)}")
    return path
