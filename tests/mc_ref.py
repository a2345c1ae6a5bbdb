"""A slow, table-free restatement of the marching-cubes rule of ndjir_amd/mc.py (csrc/mc.hip), written from the rule's
definition and not from the kernels.

The rule.  A lattice point is inside iff vol < level.  One vertex per lattice edge whose endpoints differ, at
index + t, t = (level - v0) / (v1 - v0) in fp32, ordered by (point linear index, axis).  In a cell, each of the six faces
is walked counter-clockwise as seen from outside the cell; every maximal run of consecutive inside corners gives one
directed segment from the crossing where the run ends to the crossing where it begins.  The segments of a cell link into
closed loops whose right-hand normals point toward decreasing values; "descent" delivers the reverse winding (normals
toward increasing values), "ascent" the loops as they are.  How a loop is cut into triangles is the implementer's choice,
so triangle lists are compared through two reductions that do not depend on it: the directed boundary segments per cell
and the global directed-edge counts.

Numbering: corner c = dx + 2 dy + 4 dz; cube edge = 4 * axis + rank of its lower corner among the four corners with
d_axis == 0 (ascending corner number)."""
import collections

import numpy as np


def corner_id(d):
    return int(d[0]) + 2 * int(d[1]) + 4 * int(d[2])


def edge_id(c0, c1):
    """The cube edge between two adjacent corners."""
    axis = {1: 0, 2: 1, 4: 2}[c0 ^ c1]
    lows = [c for c in range(8) if not (c >> axis) & 1]
    return 4 * axis + lows.index(min(c0, c1))


def _face_walks():
    walks = []
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3                   # e_u x e_v = e_a
        for side in (0, 1):
            # counter-clockwise about the outward normal: +e_a on the far side, -e_a on the near side
            uv = [(0, 0), (1, 0), (1, 1), (0, 1)] if side else [(0, 0), (0, 1), (1, 1), (1, 0)]
            walk = []
            for pu, pv in uv:
                d = [0, 0, 0]
                d[a], d[u], d[v] = side, pu, pv
                walk.append(corner_id(d))
            walks.append(walk)
    return walks


FACE_WALKS = _face_walks()


def cell_segments(inside8):
    """inside8[c] for the eight corners -> (segments, loops): the directed segments (from_edge, to_edge) of the six faces
    and the closed loops they link into (lists of cube edges, each starting at its smallest edge)."""
    segs = []
    for w in FACE_WALKS:
        ins = [bool(inside8[c]) for c in w]
        if all(ins) or not any(ins):
            continue
        for s in range(4):
            if ins[s] and not ins[s - 1]:                 # a run begins at s
                e = s
                while ins[(e + 1) % 4]:
                    e = (e + 1) % 4
                begin = edge_id(w[s - 1], w[s])           # outside -> inside
                end = edge_id(w[e], w[(e + 1) % 4])       # inside -> outside
                segs.append((end, begin))
    nxt = dict(segs)
    assert len(nxt) == len(segs) and sorted(nxt) == sorted(nxt.values())
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        loops.append(loop)
    return segs, loops


def inside_of(vol, level):
    return np.asarray(vol, np.float32) < np.float32(level)


def crossing_edges(vol, level):
    """(lin, axis): the lattice edges whose endpoints differ in insideness, as the linear index of the lower point and the
    axis, in vertex order (lin ascending, then axis)."""
    ins = inside_of(vol, level)
    G = ins.shape
    lin = np.arange(ins.size, dtype=np.int64).reshape(G)
    keys = []
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        cross = ins[tuple(lo)] != ins[tuple(hi)]
        keys.append(lin[tuple(lo)][cross] * 3 + a)
    keys = np.sort(np.concatenate(keys))
    return keys // 3, (keys % 3).astype(np.int64)


def vertex_positions(vol, level, lin, axis, mins=None, maxs=None):
    """fp32 positions of the vertices on the edges (lin, axis): lattice coordinates, or world coordinates
    pos * scale + mins with scale = float32((maxs - mins) / (G - 1)) formed in float64, a multiply and then an add."""
    vol = np.asarray(vol, np.float32)
    G = vol.shape
    level = np.float32(level)
    n = len(lin)
    ijk = np.stack(np.unravel_index(np.asarray(lin, np.int64), G), axis=1).reshape(n, 3)
    nb = ijk.copy()
    nb[np.arange(n), axis] += 1
    v0, v1 = vol[tuple(ijk.T)], vol[tuple(nb.T)]
    with np.errstate(all="ignore"):
        t = (level - v0) / (v1 - v0)
        assert t.dtype == np.float32
        pos = ijk.astype(np.float32)
        pos[np.arange(n), axis] = pos[np.arange(n), axis] + t
        if mins is None:
            return pos
        scale = np.array([(float(maxs[a]) - float(mins[a])) / (G[a] - 1) for a in range(3)], np.float64).astype(np.float32)
        out = pos * scale[None, :]
        out = out + np.asarray(mins, np.float64).astype(np.float32)[None, :]
    assert out.dtype == np.float32
    return out


def active_cells(vol, level):
    """(origins (n, 3), inside (n, 8)): the cells whose corners are not all alike, ascending by the origin's linear index."""
    ins = inside_of(vol, level)
    Gx, Gy, Gz = ins.shape
    if min(ins.shape) < 2:
        return np.zeros((0, 3), np.int64), np.zeros((0, 8), bool)
    corners = np.stack([ins[dx:Gx - 1 + dx, dy:Gy - 1 + dy, dz:Gz - 1 + dz]
                        for dx, dy, dz in [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]], axis=-1)
    n_in = corners.sum(axis=-1)
    origins = np.argwhere((n_in > 0) & (n_in < 8))         # row-major: ascending linear index
    return origins, corners[tuple(origins.T)]


def local_edge(origin, G, lin, axis):
    """The cube edge, in the cell at `origin`, of the lattice edge (lin, axis); asserts that it belongs to the cell."""
    p = np.array(np.unravel_index(int(lin), G)) - np.asarray(origin)
    assert p.min() >= 0 and p.max() <= 1 and p[axis] == 0, (origin, lin, axis)
    q = p.copy()
    q[axis] = 1
    return edge_id(corner_id(p), corner_id(q))


def global_edge(origin, G, e):
    """(lin, axis) of cube edge e of the cell at `origin`."""
    axis = e >> 2
    low = [c for c in range(8) if not (c >> axis) & 1][e & 3]
    p = np.asarray(origin) + np.array([low & 1, (low >> 1) & 1, (low >> 2) & 1])
    return int(np.ravel_multi_index(tuple(p), G)), axis


def boundary_segments(tris):
    """Directed edges of the triangles that are not cancelled by their reverse: the boundary of what the triangles
    cover, whatever the triangulation.  tris: iterable of 3-tuples of hashable vertices.  Returns a sorted list (with
    multiplicity)."""
    count = collections.Counter()
    for a, b, c in tris:
        for u, v in ((a, b), (b, c), (c, a)):
            if count[(v, u)] > 0:
                count[(v, u)] -= 1
            else:
                count[(u, v)] += 1
    return sorted(count.elements())


def reference_mesh(vol, level, direction="descent"):
    """(lin, axis, faces (F, 3) int64, cells): the rule's mesh with every loop cut as a fan from its first vertex; `cells`
    lists per active cell (origin, number of triangles, directed segments in cube-edge numbers, in `direction`)."""
    assert direction in ("descent", "ascent")
    vol = np.asarray(vol, np.float32)
    G = vol.shape
    lin, axis = crossing_edges(vol, level)
    index = {(int(p), int(a)): n for n, (p, a) in enumerate(zip(lin, axis))}
    origins, inside = active_cells(vol, level)
    faces, cells = [], []
    for origin, ins8 in zip(origins, inside):
        segs, loops = cell_segments(ins8)
        if direction == "descent":
            segs = [(b, a) for a, b in segs]
            loops = [loop[::-1] for loop in loops]
        ntri = 0
        for loop in loops:
            ids = [index[global_edge(origin, G, e)] for e in loop]
            for m in range(1, len(ids) - 1):
                faces.append((ids[0], ids[m], ids[m + 1]))
                ntri += 1
        cells.append((tuple(int(x) for x in origin), ntri, sorted(segs)))
    return lin, axis, np.asarray(faces, np.int64).reshape(-1, 3), cells


def faces_per_cell(vol, faces, lin, axis, cells):
    """Splits `faces` (in face order: ascending cell, cells[n][1] triangles each) and renames every vertex to its cube edge in
    that cell.  Returns a list of triangle lists, one per cell of `cells`."""
    G = np.asarray(vol).shape
    faces = np.asarray(faces).reshape(-1, 3)
    assert faces.shape[0] == sum(c[1] for c in cells), (faces.shape[0], sum(c[1] for c in cells))
    out, f = [], 0
    for origin, ntri, _ in cells:
        out.append([tuple(local_edge(origin, G, lin[v], axis[v]) for v in faces[f + m]) for m in range(ntri)])
        f += ntri
    return out


def directed_edge_counts(faces):
    """Counter of the directed edges (u, v) of a face list."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    pairs, counts = np.unique(e, axis=0, return_counts=True) if len(e) else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    return collections.Counter({(int(u), int(v)): int(n) for (u, v), n in zip(pairs, counts)})


def is_balanced(faces):
    """Every directed edge occurs as often as its reverse (closed, consistently oriented)."""
    c = directed_edge_counts(faces)
    return all(c.get((v, u), 0) == n for (u, v), n in c.items())


def is_strictly_manifold(faces):
    """Every directed edge occurs exactly once and its reverse exactly once."""
    c = directed_edge_counts(faces)
    return all(n == 1 and c.get((v, u), 0) == 1 for (u, v), n in c.items())


def euler_characteristic(n_verts, faces):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    return int(n_verts) - len(np.unique(e, axis=0)) + len(faces)


# ---- analytic volumes on [-1, 1]^3 (or any box), indexing='ij' ----------------------------------------------------------------

def lattice(G, mins=(-1.0, -1.0, -1.0), maxs=(1.0, 1.0, 1.0)):
    G = (G, G, G) if np.isscalar(G) else tuple(G)
    return np.meshgrid(*[np.linspace(mins[a], maxs[a], G[a]) for a in range(3)], indexing="ij")


def sphere(G, radius=0.6, centre=(0.0, 0.0, 0.0)):
    X, Y, Z = lattice(G)
    return (np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - radius).astype(np.float32)


def torus(G, R=0.55, r=0.25):
    X, Y, Z = lattice(G)
    return (np.sqrt((np.sqrt(X ** 2 + Y ** 2) - R) ** 2 + Z ** 2) - r).astype(np.float32)


def two_spheres(G, radius=0.3, offset=0.45):
    X, Y, Z = lattice(G)
    d = lambda cx: np.sqrt((X - cx) ** 2 + Y ** 2 + Z ** 2) - radius
    return np.minimum(d(-offset), d(offset)).astype(np.float32)


def all_cases_volume():
    """(4, 4, 1024): case c occupies the points (1..2, 1..2, 4c + 1 .. 4c + 2), inside = -1, everything else +1."""
    vol = np.ones((4, 4, 1024), np.float32)
    for c in range(256):
        for b in range(8):
            if (c >> b) & 1:
                vol[1 + (b & 1), 1 + ((b >> 1) & 1), 4 * c + 1 + ((b >> 2) & 1)] = -1.0
    return vol
