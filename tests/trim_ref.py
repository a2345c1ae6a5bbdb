"""numpy restatement of python/extract_by_mc.py:77-128 (`clean_points_by_mask`, `create_trimmed_meshes`) for the trimming tests:
the dilation by stamping the structuring element's rows, the projection operation by operation in float64, the index remap,
and the split into components (sorted edge keys + scipy's connected_components, labels made canonical: the smallest face
index of the component).  A helper, not a test; nothing here touches the product."""
import numpy as np

INT_MIN = np.iinfo(np.int32).min


def ellipse_half_widths(r):
    """cv.getStructuringElement(cv.MORPH_ELLIPSE, (2r + 1, 2r + 1)), row by row (OpenCV's expression, unpinned: no cv2 here)."""
    if r == 0:
        return np.zeros(1, dtype=np.int64)
    out = []
    for dy in range(-r, r + 1):
        out.append(int(np.rint(r * np.sqrt((r * r - dy * dy) * (1.0 / (r * r))))))
    return np.asarray(out, dtype=np.int64)


def ellipse(r):
    """The structuring element as a (2r + 1, 2r + 1) bool array."""
    half = ellipse_half_widths(r)
    dx = np.abs(np.arange(-r, r + 1))
    return dx[None, :] <= half[:, None]


def dilate(mask, r):
    """Binary dilation of a bool (H, W) image, zero border: every set pixel stamps the element's rows."""
    H, W = mask.shape
    half = ellipse_half_widths(r)
    out = np.zeros((H, W), dtype=bool)
    for y, x in zip(*np.nonzero(mask)):
        for dy in range(max(-r, -y), min(r, H - 1 - y) + 1):
            h = half[dy + r]
            out[y + dy, max(0, x - h):x + h + 1] = True
    return out


def padded_mask(mask, r):
    """extract_by_mc.py:89-96 for one view: float mask -> (H + 2, W + 2) uint8, dilated, framed with ones."""
    m = dilate(np.asarray(mask) >= 0.5, r).astype(np.uint8)
    H, W = m.shape
    m = np.concatenate([np.ones([1, W], np.uint8), m, np.ones([1, W], np.uint8)], axis=0)
    return np.concatenate([np.ones([H + 2, 1], np.uint8), m, np.ones([H + 2, 1], np.uint8)], axis=1)


def camera(K, pose):
    """:81-84 for one view: pose (4, 4) float32 camera-to-world -> (K float64, R, t in the pose's dtype)."""
    pose = pose[None]
    R = np.linalg.inv(pose[:, :3, :3])
    t = -R @ pose[:, :3, 3:]
    return np.asarray(K, np.float64)[None], R, t


def camera_table(Ks, poses):
    rows = []
    for K, pose in zip(Ks, poses):
        K, R, t = camera(K, np.asarray(pose, np.float32))
        rows.append(np.concatenate([K.reshape(-1), R.reshape(-1).astype(np.float64), t.reshape(-1).astype(np.float64)]))
    return np.asarray(rows, np.float64).reshape(-1, 21)


def _to_int32(a):
    """`astype(np.int32)` as x86 does it: what int32 cannot hold (NaN, inf, out of range) becomes INT_MIN."""
    ok = np.isfinite(a) & (np.abs(a) < 2.0 ** 31)
    return np.where(ok, np.where(ok, a, 0).astype(np.int64), INT_MIN)


def inside_masks(points, padded, Ks, poses, eps=1e-6):
    """`clean_points_by_mask` (:77-102) -> (keep (N,) bool, ambiguous (N,) bool).  points (N, 3) float32, widened to float64;
    padded (M, H + 2, W + 2).  ambiguous: some view's projected x or y lies within `eps` of a half-integer, or |u_z| < 1e-9 --
    there the last bit of the arithmetic decides and the comparison is not made."""
    points = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    N = len(points)
    inside = np.ones(N) > 0.5
    ambiguous = np.zeros(N, dtype=bool)
    Hp, Wp = padded.shape[1:]
    with np.errstate(all="ignore"):
        for i in range(len(padded)):
            K, R, t = camera(Ks[i], np.asarray(poses[i], np.float32))
            pts_image = np.matmul(K, np.matmul(R, points[:, :, None]) + t).reshape(N, 3)
            uz = pts_image[:, 2:].copy()
            pts_image = pts_image / pts_image[:, 2:]
            frac = np.abs(pts_image[:, :2] - np.floor(pts_image[:, :2]) - 0.5)
            ambiguous |= (frac < eps).any(axis=1) | (np.abs(uz[:, 0]) < 1e-9)
            pix = _to_int32(np.round(pts_image)) + 1
            curr = padded[i][(pix[:, 1].clip(0, Hp - 1), pix[:, 0].clip(0, Wp - 1))]
            inside &= curr.astype(bool)
    return inside, ambiguous


def trim(verts, faces, mask):
    """:111-120: (new_vertices, new_faces)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    indexes = np.ones(len(verts)) * -1
    indexes = indexes.astype(np.int64)
    indexes[np.where(mask)] = np.arange(len(np.where(mask)[0]))
    faces_mask = mask[faces[:, 0]] & mask[faces[:, 1]] & mask[faces[:, 2]]
    new_faces = faces[np.where(faces_mask)].copy()
    for k in range(3):
        new_faces[:, k] = indexes[new_faces[:, k]]
    return verts[np.where(mask)], new_faces, indexes


def component_labels(faces):
    """labels (F,): the smallest face index of the face's component; faces sharing an undirected edge (u != v) are connected."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(faces)
    if F == 0:
        return np.zeros(0, np.int64)
    e = np.stack([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], axis=1).reshape(-1, 2)
    owner = np.repeat(np.arange(F), 3)
    real = e[:, 0] != e[:, 1]
    e, owner = e[real], owner[real]
    key = (e.min(axis=1) << 32) | e.max(axis=1)
    order = np.argsort(key, kind="stable")
    key, owner = key[order], owner[order]
    same = key[1:] == key[:-1]
    a, b = owner[:-1][same], owner[1:][same]
    g = coo_matrix((np.ones(len(a)), (a, b)), shape=(F, F))
    n, lab = connected_components(g, directed=False)
    smallest = np.full(n, F, np.int64)
    np.minimum.at(smallest, lab, np.arange(F))
    return smallest[lab]


def split(verts, faces, max_meshes=None):
    """`split(only_watertight=False)` + the ordering by face count (:124-126) -> ([(verts_k, faces_k)], n_components):
    face count descending, ties by smallest face index; faces in order; vertices = those used, ascending."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    lab = component_labels(faces)
    roots, sizes = np.unique(lab, return_counts=True)
    order = sorted(range(len(roots)), key=lambda i: (-sizes[i], roots[i]))
    meshes = []
    for i in order[:max_meshes]:
        f = faces[lab == roots[i]]
        used = np.unique(f)
        index = np.full(len(verts), -1, np.int64)
        index[used] = np.arange(len(used))
        meshes.append((verts[used], index[f]))
    return meshes, len(roots)


def trimmed_meshes(verts, faces, masks, Ks, poses, r, max_meshes=5):
    """`create_trimmed_meshes` end to end; masks (M, H, W) float."""
    padded = np.stack([padded_mask(m, r) for m in masks])
    keep, ambiguous = inside_masks(verts, padded, Ks, poses)
    nv, nf, _ = trim(np.asarray(verts, np.float32), faces, keep)
    if len(nf) == 0:
        return [], keep, ambiguous
    return split(nv, nf, max_meshes)[0], keep, ambiguous


# ---- hand-made component cases (shared by the CPU and GPU tests) ---------------------------------------------------------

def tetrahedron(a, b, c, d):
    return [[a, b, c], [a, d, b], [b, d, c], [c, d, a]]


def lattice_sphere(rings, segments, base=0):
    """A closed latitude/longitude sphere: (vertices used, faces); two poles, `rings` rings of `segments` vertices."""
    top, bottom = base, base + 1
    ring = lambda i, j: base + 2 + i * segments + (j % segments)
    faces = []
    for j in range(segments):
        faces.append([top, ring(0, j), ring(0, j + 1)])
        for i in range(rings - 1):
            faces.append([ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)])
            faces.append([ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)])
        faces.append([bottom, ring(rings - 1, j + 1), ring(rings - 1, j)])
    return 2 + rings * segments, faces


def component_cases():
    """name -> (faces (F, 3) int64, n_verts, number of components or None)."""
    rng = np.random.RandomState(5)
    strip = np.stack([np.arange(20000), np.arange(20000) + 1, np.arange(20000) + 2], axis=1)
    n_sphere, sphere = lattice_sphere(12, 16)
    floaters = (tetrahedron(*range(n_sphere, n_sphere + 4)) + [[n_sphere + 4, n_sphere + 5, n_sphere + 6]]
                + tetrahedron(*range(n_sphere + 7, n_sphere + 11)) + [[n_sphere + 11, n_sphere + 12, n_sphere + 13]])
    cases = {
        "tets_disjoint": (tetrahedron(0, 1, 2, 3) + tetrahedron(4, 5, 6, 7), 8, 2),
        "tets_share_vertex": (tetrahedron(0, 1, 2, 3) + tetrahedron(3, 4, 5, 6), 7, 2),
        "tets_share_edge": (tetrahedron(0, 1, 2, 3) + tetrahedron(2, 3, 4, 5), 6, 1),
        "strip": (strip, 20002, 1),
        "strip_shuffled": (strip[rng.permutation(20000)], 20002, 1),
        "isolated": (np.arange(30000).reshape(10000, 3), 30000, 10000),
        "three_on_an_edge": ([[0, 1, 2], [0, 1, 3], [1, 0, 4], [5, 6, 7]], 8, 2),
        "repeated_vertex": ([[0, 0, 1], [0, 1, 2], [5, 5, 5], [6, 6, 7], [6, 7, 7]], 8, 3),
        "one_face": ([[2, 0, 1]], 3, 1),
        "soup": (rng.randint(0, 12000, size=(20000, 3)), 12000, None),
        "sphere_and_floaters": (floaters[:5] + sphere + floaters[5:], n_sphere + 14, 5),
    }
    return {k: (np.asarray(f, np.int64).reshape(-1, 3), n, c) for k, (f, n, c) in cases.items()}
