"""Mesh trimming on the device (ndjir_amd/trim.py, csrc/trim.hip; python/extract_by_mc.py:77-128) against the numpy
restatement tests/trim_ref.py: mask dilation, the vertex test, the stable compactions, face components, and the composed
`create_trimmed_meshes` / `extract`.  Every result is an integer array or a selection of input rows: every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from tests import trim_ref as R
from tests.parity_utils import small_conf

pytestmark = pytest.mark.gpu

K_DTU = np.array([[2900.0, 0.3, 800.0], [0.0, 2890.0, 600.0], [0.0, 0.0, 1.0]])
_CACHE = {}


def _pow2_at_least(n):
    return 1 << max(0, int(n - 1).bit_length())


# ---- dilation ---------------------------------------------------------------------------------------------------------------

def _pattern(name, H, W, rng):
    m = np.zeros((H, W), np.float32)
    if name == "full":
        m[:] = 1.0
    elif name == "points":           # the four corners, the mid-edges and the centre
        for y in (0, H // 2, H - 1):
            for x in (0, W // 2, W - 1):
                m[y, x] = 1.0
    elif name == "sparse":
        m[rng.uniform(size=(H, W)) < 0.005] = 1.0
    elif name == "dense":
        m[rng.uniform(size=(H, W)) < 0.5] = 1.0
    elif name == "threshold":        # 0.5 counts as set, 0.49 does not
        m[:] = rng.choice(np.array([0.0, 0.49], np.float32), size=(H, W))
        sel = rng.uniform(size=(H, W)) < 0.01
        m[sel] = rng.choice(np.array([0.5, 0.51], np.float32), size=int(sel.sum()))
        m[H // 3, W // 3], m[H // 2, W // 2] = 0.5, 0.51
    else:
        assert name == "empty"
    return m


def _dilate(masks, r, gpu):
    from ndjir_amd.trim import dilate_masks
    out = dilate_masks(torch.from_numpy(masks).to(gpu), r)
    assert out.dtype == torch.uint8 and out.shape == (masks.shape[0], masks.shape[1] + 2, masks.shape[2] + 2)
    return out.cpu().numpy()


def _check_dilation(got, masks, r):
    for g, m in zip(got, masks):
        assert g[0].all() and g[-1].all() and g[:, 0].all() and g[:, -1].all()          # the frame
        np.testing.assert_array_equal(g, R.padded_mask(m, r))
    assert set(np.unique(got)) <= {0, 1}


SIZES = [(67, 131, 0), (67, 131, 1), (67, 131, 5), (67, 131, 50), (1, 1, 0), (1, 1, 5), (1, 200, 5), (200, 1, 5)]


@pytest.mark.parametrize("pattern", ["empty", "full", "points", "sparse", "dense", "threshold"])
@pytest.mark.parametrize("H,W,r", SIZES)
def test_dilation(gpu, H, W, r, pattern):
    rng = np.random.RandomState(H * 1000 + W + r)
    masks = _pattern(pattern, H, W, rng)[None]
    got = _dilate(masks, r, gpu)
    _check_dilation(got, masks, r)
    if pattern == "threshold":
        assert got[0, 1:-1, 1:-1].any()


def test_dilation_three_views(gpu):
    rng = np.random.RandomState(3)
    masks = np.stack([_pattern(p, 67, 131, rng) for p in ("sparse", "points", "empty")])
    got = _dilate(masks, 5, gpu)
    _check_dilation(got, masks, 5)
    assert got[0].sum() != got[1].sum() and got[2, 1:-1, 1:-1].sum() == 0


def test_dilation_full_size(gpu):
    H, W, r = 1200, 1600, 50
    rng = np.random.RandomState(9)
    m = np.zeros((H, W), np.float32)
    m[rng.randint(0, H, 190), rng.randint(0, W, 190)] = 1.0
    for y in (0, H // 2, H - 1):
        for x in (0, W // 2, W - 1):
            m[y, x] = 1.0
    m[0, 255:258] = 1.0               # around a row-segment boundary of the row pass
    m[H - 1, 1023] = m[63, 64] = 1.0
    got = _dilate(m[None], r, gpu)
    _check_dilation(got, m[None], r)


# ---- vertex test ------------------------------------------------------------------------------------------------------------

def _look_at(centre, rng):
    """camera-to-world pose (4, 4) float32 of a camera at `centre` looking at the origin, rolled at random."""
    z = -centre / np.linalg.norm(centre)
    a = rng.normal(size=3)
    x = a - z * (a @ z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    pose = np.eye(4)
    pose[:3, :3] = np.stack([x, y, z], axis=1)
    pose[:3, 3] = centre
    return pose.astype(np.float32)


def _scene(gpu):
    """4099 points, 7 cameras 3 units out, 1200 x 1600 masks dilated with r = 5 -- built once, never modified."""
    if "scene" in _CACHE:
        return _CACHE["scene"]
    from scipy.ndimage import binary_dilation
    from ndjir_amd.trim import camera_table, dilate_masks
    rng = np.random.RandomState(41)
    M, H, W, r = 7, 1200, 1600, 5
    pts = rng.uniform(-1, 1, size=(4099, 3)).astype(np.float32)
    poses = []
    for _ in range(M):
        d = rng.normal(size=3)
        poses.append(_look_at(3.0 * d / np.linalg.norm(d) + rng.uniform(-0.1, 0.1, size=3), rng))
    poses = np.stack(poses)
    Ks = np.stack([K_DTU] * M)
    yy, xx = np.mgrid[:H, :W]
    masks = np.zeros((M, H, W), np.float32)
    for i in range(M):
        cy, cx, rad = 600 + rng.randint(-80, 80), 800 + rng.randint(-80, 80), 420 + rng.randint(0, 120)
        masks[i] = ((yy - cy) ** 2 + (xx - cx) ** 2 < rad ** 2) | (rng.uniform(size=(H, W)) < 0.002)
    padded_ref = np.ones((M, H + 2, W + 2), np.uint8)
    for i in range(M):              # scipy's dilation (tests/test_trim_ref_cpu.py ties it to the stamping) -- stamping a disc is slow
        padded_ref[i, 1:-1, 1:-1] = binary_dilation(masks[i] >= 0.5, structure=R.ellipse(r), border_value=0)
    padded = dilate_masks(torch.from_numpy(masks).to(gpu), r)
    keep_ref, ambiguous = R.inside_masks(pts, padded_ref, Ks, poses)
    cams = camera_table(Ks, poses.astype(np.float64))          # widened, as IDRRaySource keeps them
    _CACHE["scene"] = dict(pts=pts, poses=poses, Ks=Ks, padded_ref=padded_ref, padded=padded, keep_ref=keep_ref,
                           ambiguous=ambiguous, cams=cams)
    return _CACHE["scene"]


def test_camera_table(gpu):
    s = _scene(gpu)
    assert s["cams"].dtype == np.float64 and s["cams"].shape == (7, 21)
    np.testing.assert_array_equal(s["cams"], R.camera_table(s["Ks"], s["poses"]))


def test_vertex_test_random_cameras(gpu):
    from ndjir_amd.trim import points_inside_masks
    s = _scene(gpu)
    np.testing.assert_array_equal(s["padded"].cpu().numpy(), s["padded_ref"])
    amb = s["ambiguous"]
    print(f"ambiguous vertices: {int(amb.sum())} of {len(amb)}")
    assert amb.sum() <= 0.005 * len(amb)
    keep = points_inside_masks(s["pts"], s["padded"], s["cams"])
    assert keep.dtype == torch.bool and keep.shape == (4099,)
    keep = keep.cpu().numpy()
    ref = s["keep_ref"]
    assert ref[~amb].any() and not ref[~amb].all()
    print(f"kept {int(ref.sum())} of {len(ref)}")
    np.testing.assert_array_equal(keep[~amb], ref[~amb])


@pytest.mark.parametrize("N", [0, 1, 255, 256, 257])
def test_vertex_test_sizes_one_view(gpu, N):
    from ndjir_amd.trim import points_inside_masks
    s = _scene(gpu)
    pts = s["pts"][100:100 + N]
    keep = points_inside_masks(torch.from_numpy(pts).to(gpu), s["padded"][2:3].contiguous(), s["cams"][2:3]).cpu().numpy()
    ref, amb = R.inside_masks(pts, s["padded_ref"][2:3], s["Ks"][2:3], s["poses"][2:3])
    assert keep.shape == (N,)
    np.testing.assert_array_equal(keep[~amb], ref[~amb])
    if N >= 255:
        assert ref.any() and not ref.all() and amb.sum() <= 2


def test_vertex_test_hand_made_points(gpu):
    """One camera at c = (0.5, 0.25, -2) looking along +z, f = 100, principal point (50, 40), image 80 x 100: the pixel of
    p is (100 (p_x - c_x) / (p_z - c_z) + 50, 100 (p_y - c_y) / (p_z - c_z) + 40).  Only pixel (x 40, y 40) is set."""
    from ndjir_amd.trim import camera_table, dilate_masks, points_inside_masks
    H, W = 80, 100
    c = np.array([0.5, 0.25, -2.0])
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = c
    K = np.array([[100.0, 0.0, 50.0], [0.0, 100.0, 40.0], [0.0, 0.0, 1.0]])
    mask = np.zeros((1, H, W), np.float32)
    mask[0, 40, 40] = 1.0
    at = lambda px, py, depth=1.0: c + np.array([(px - 50) / 100.0 * depth, (py - 40) / 100.0 * depth, depth])
    cases = [
        (c, True),                          # at the camera centre: 0 / 0, non-finite -> the frame
        (at(40, 40, -1.0), True),           # behind the camera, mirrored onto the set pixel
        (at(41, 40, -1.0), False),          # behind the camera, next to it
        (at(40, 40), True), (at(41, 40), False), (at(40, 41), False),
        (c + np.array([16.0, 0.0, 2.0 ** -20]), True),      # 1.7 10^9 pixels to the right -> column W + 1
        (c + np.array([-16.0, 0.0, 2.0 ** -20]), True),     # ... to the left -> column 0
        (c + np.array([0.0, 64.0, 2.0 ** -20]), True),      # beyond int32: INT_MIN in numpy, clipped to row 0
        (at(-1, 40), True), (at(0, 40), False),       # frame column 0 / first image column
        (at(100, 40), True), (at(99, 40), False),     # frame column W + 1 / last image column
        (at(40, -1), True), (at(40, 0), False),       # frame row 0 / first image row
        (at(40, 80), True), (at(40, 79), False),      # frame row H + 1 / last image row
        (at(-7, -9), True), (at(300, 40), True),      # well outside the image
    ]
    pts = np.array([p for p, _ in cases], np.float32)
    expected = np.array([e for _, e in cases])
    padded = dilate_masks(torch.from_numpy(mask).to(gpu), 0)
    keep = points_inside_masks(pts, padded, camera_table(K[None], pose[None])).cpu().numpy()
    np.testing.assert_array_equal(keep, expected)
    ref, amb = R.inside_masks(pts, R.padded_mask(mask[0], 0)[None], K[None], pose[None])
    np.testing.assert_array_equal(ref[~amb], expected[~amb])
    assert amb[0] and amb.sum() == 1        # the camera centre only


# ---- compaction and trim_mesh -----------------------------------------------------------------------------------------------

def _keep_patterns(N, rng):
    alt = np.arange(N) % 2 == 0
    last = np.zeros(N, bool)
    last[N - 1:] = True
    return {"all": np.ones(N, bool), "none": np.zeros(N, bool), "alternating": alt, "random": rng.uniform(size=N) < 0.37, "last": last}


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 5, (1 << 20) + 1029])
def test_compaction_and_trim_mesh(gpu, N):
    """(1 << 20) + 1029: more than 1024 blocks of 1024, so the scan of the block totals takes a second pass with a carry."""
    from ndjir_amd import lib
    from ndjir_amd.trim import trim_mesh
    rng = np.random.RandomState(N % 9973)
    verts = rng.uniform(-1, 1, size=(N, 3)).astype(np.float32)
    F = 0 if N == 0 else min(2 * N + 3, 300000)
    faces = rng.randint(0, max(N, 1), size=(F, 3))
    verts_t, faces_t = torch.from_numpy(verts).to(gpu), torch.from_numpy(faces).to(gpu)
    for name, keep in _keep_patterns(N, rng).items():
        if N >= 63 and name in ("random", "alternating"):       # faces that lose exactly one vertex, and one that keeps all
            k, d = np.nonzero(keep)[0], np.nonzero(~keep)[0]
            faces[0], faces[1], faces[2] = [k[0], k[-1], d[0]], [d[-1], k[0], k[-1]], [k[0], k[-1], k[len(k) // 2]]
            faces_t = torch.from_numpy(faces).to(gpu)
        ref_v, ref_f, ref_index = R.trim(verts, faces, keep)
        keep_t = torch.from_numpy(keep).to(gpu)
        new_index = torch.full((N,), 7, device=gpu, dtype=torch.int32)
        count = torch.full((2,), 7, device=gpu, dtype=torch.int32)
        lib.call("compact_flags", N, keep_t.to(torch.uint8), new_index, count,
                 torch.empty(max(1, -(-N // 1024)), device=gpu, dtype=torch.int32), None, 0, None)
        assert count.cpu().tolist() == [int(keep.sum()), 0], name
        np.testing.assert_array_equal(new_index.cpu().numpy(), ref_index, err_msg=name)
        v, f = trim_mesh(verts_t, faces_t, keep_t)
        assert v.dtype == torch.float32 and f.dtype == torch.int32
        np.testing.assert_array_equal(v.cpu().numpy(), ref_v, err_msg=name)
        np.testing.assert_array_equal(f.cpu().numpy(), ref_f, err_msg=name)
        if N >= 63 and name == "random":
            assert 0 < len(ref_f) < F


def test_trim_mesh_rejects_a_face_outside_the_mesh(gpu):
    from ndjir_amd.trim import trim_mesh
    verts = torch.zeros((4, 3), device=gpu)
    keep = torch.ones(4, device=gpu, dtype=torch.bool)
    with pytest.raises(ValueError, match="outside"):
        trim_mesh(verts, torch.tensor([[0, 1, 2], [1, 2, 4]], device=gpu), keep)


# ---- components -------------------------------------------------------------------------------------------------------------

CASES = R.component_cases()


def _ref_labels(name):
    if ("labels", name) not in _CACHE:
        _CACHE["labels", name] = R.component_labels(CASES[name][0])
    return _CACHE["labels", name]


@pytest.mark.parametrize("name", list(CASES))
def test_face_components(gpu, name):
    from ndjir_amd.trim import face_components
    faces, n_verts, n_components = CASES[name]
    faces_t = torch.from_numpy(faces).to(device=gpu, dtype=torch.int32)
    a = face_components(faces_t, n_verts)
    b = face_components(faces_t, n_verts)
    assert a.dtype == torch.int32 and torch.equal(a, b)
    ref = _ref_labels(name)
    np.testing.assert_array_equal(a.cpu().numpy(), ref)
    print(f"{name}: {len(np.unique(ref))} components of {len(faces)} faces")
    if n_components is not None:
        assert len(np.unique(ref)) == n_components


def test_face_components_empty(gpu):
    from ndjir_amd.trim import face_components, split_components
    lab = face_components(torch.zeros((0, 3), device=gpu, dtype=torch.int32), 5)
    assert lab.shape == (0,)
    assert split_components(torch.zeros((5, 3), device=gpu), torch.zeros((0, 3), device=gpu, dtype=torch.int32)) == ([], 0)


def _distinct_edges(faces):
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    e = e[e[:, 0] != e[:, 1]]
    return len(np.unique((e.min(axis=1) << 32) | e.max(axis=1)))


def test_face_components_tight_table(gpu):
    """The smallest power of two that holds every distinct edge: long probe chains, same labels."""
    from ndjir_amd.trim import face_components
    faces, n_verts, _ = CASES["soup"]
    E = _distinct_edges(faces)
    slots = _pow2_at_least(E)
    print(f"{E} distinct edges in {slots} slots")
    assert slots // 2 < E <= slots
    lab = face_components(torch.from_numpy(faces).to(device=gpu, dtype=torch.int32), n_verts, slots=slots)
    np.testing.assert_array_equal(lab.cpu().numpy(), _ref_labels("soup"))


def test_face_components_table_too_small(gpu):
    """Half the slots the edges need: the bounded probe gives up, the call returns NDJIR_ERR_CAPACITY, the binding raises."""
    from ndjir_amd import lib
    from ndjir_amd.trim import face_components
    faces, n_verts, _ = CASES["sphere_and_floaters"]
    slots = _pow2_at_least(_distinct_edges(faces)) // 2
    faces_t = torch.from_numpy(faces).to(device=gpu, dtype=torch.int32)
    with pytest.raises(lib.NdjirHipError, match="status 4"):
        face_components(faces_t, n_verts, slots=slots)
    with pytest.raises(lib.NdjirHipError, match="status 3"):           # not a power of two
        face_components(faces_t, n_verts, slots=3000)
    with pytest.raises(lib.NdjirHipError, match="status 3"):           # a vertex index outside the mesh
        face_components(faces_t, n_verts - 1)
    np.testing.assert_array_equal(face_components(faces_t, n_verts).cpu().numpy(), _ref_labels("sphere_and_floaters"))


def _check_meshes(got, ref):
    assert len(got) == len(ref)
    for (v, f), (rv, rf) in zip(got, ref):
        assert v.dtype == torch.float32 and f.dtype == torch.int32
        np.testing.assert_array_equal(v.cpu().numpy(), rv)
        np.testing.assert_array_equal(f.cpu().numpy(), rf)


@pytest.mark.parametrize("max_meshes", [None, 3])
def test_split_components_ranking(gpu, max_meshes):
    """A closed sphere and four floaters: largest first, the two tetrahedra and the two triangles each in face order."""
    from ndjir_amd.trim import split_components
    faces, n_verts, _ = CASES["sphere_and_floaters"]
    rng = np.random.RandomState(2)
    verts = rng.uniform(-1, 1, size=(n_verts + 3, 3)).astype(np.float32)          # three vertices no face uses
    got, n = split_components(torch.from_numpy(verts).to(gpu), torch.from_numpy(faces).to(gpu), max_meshes)
    ref, rn = R.split(verts, faces, max_meshes)
    assert n == rn == 5 and len(got) == (5 if max_meshes is None else 3)
    _check_meshes(got, ref)
    assert [int(f.shape[0]) for _, f in got][:3] == [len(faces) - 10, 4, 4]
    np.testing.assert_array_equal(got[1][0].cpu().numpy(), verts[n_verts - 14:n_verts - 10])      # the tetrahedron listed first


def test_split_components_shared_vertices(gpu):
    """A fan, and a lone face whose three vertices the fan uses without sharing an edge with it: extracting the fan must not
    take that face along, and the lone face's mesh has three vertices."""
    from ndjir_amd.trim import split_components
    faces = np.array([[0, 1, 2], [0, 2, 3], [1, 3, 5], [0, 3, 4], [0, 4, 5], [0, 5, 6], [7, 8, 9]])
    verts = np.arange(30, dtype=np.float32).reshape(10, 3)
    got, n = split_components(torch.from_numpy(verts).to(gpu), torch.from_numpy(faces).to(gpu))
    ref, rn = R.split(verts, faces)
    assert n == rn == 3 and [len(f) for _, f in ref] == [5, 1, 1]
    _check_meshes(got, ref)
    np.testing.assert_array_equal(got[1][0].cpu().numpy(), verts[[1, 3, 5]])


# ---- end to end -------------------------------------------------------------------------------------------------------------

def _blob(centre, radius, rings, segments, base):
    n, faces = R.lattice_sphere(rings, segments, base)
    lat = np.pi * (np.arange(rings) + 1) / (rings + 1)
    lon = 2 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.sin(lat)[:, None] * np.cos(lon), np.sin(lat)[:, None] * np.sin(lon), np.cos(lat)[:, None] * np.ones(segments)],
                    axis=-1).reshape(-1, 3)
    v = np.concatenate([[[0, 0, 1.0]], [[0, 0, -1.0]], ring]) * radius + np.asarray(centre)
    return v.astype(np.float32), faces


def _synthetic_scene(gpu):
    """Three views of three blobs; the second blob lies outside the third view's mask.  Returns the source and the numpy scene."""
    from ndjir_amd.dataset import IDRRaySource
    H, W, M = 64, 96, 3
    rng = np.random.RandomState(11)
    verts, faces, owner = [], [], []
    for b, (centre, radius, rings) in enumerate([((0, 0, 0), 0.2, 6), ((0.6, 0, 0), 0.15, 5), ((-0.5, 0.1, 0), 0.1, 4)]):
        v, f = _blob(centre, radius, rings, 8, sum(len(x) for x in verts))
        verts.append(v)
        faces += f
        owner += [b] * len(v)
    verts, faces, owner = np.concatenate(verts), np.asarray(faces, np.int64), np.asarray(owner)
    K = np.array([[90.0, 0.0, 48.0], [0.0, 90.0, 32.0], [0.0, 0.0, 1.0]])
    poses = np.stack([_look_at(np.array(c), rng) for c in ([0.0, 0.0, -3.0], [0.0, -3.0, 0.3], [0.3, 0.2, -3.0])])
    masks = np.zeros((M, H, W, 1), np.float32)
    for i in range(M):
        Kc, Rc, tc = R.camera(K, poses[i])
        u = np.matmul(Kc, np.matmul(Rc, verts.astype(np.float64)[:, :, None]) + tc).reshape(-1, 3)
        px = np.round(u[:, :2] / u[:, 2:]).astype(int)
        assert (px >= 8).all() and (px[:, 0] < W - 8).all() and (px[:, 1] < H - 8).all()        # nothing near the frame
        seen = owner != 1 if i == 2 else np.ones(len(owner), bool)
        masks[i, px[seen, 1], px[seen, 0], 0] = 1.0
    conf = small_conf(grid_size=16)
    src = IDRRaySource(np.zeros((M, H, W, 3), np.float32), masks, np.stack([K] * M), poses, conf, device=gpu)
    return src, conf, dict(verts=verts, faces=faces, owner=owner, masks=masks[..., 0], Ks=np.stack([K] * M), poses=poses)


def test_create_trimmed_meshes(gpu):
    from ndjir_amd.extract import create_trimmed_meshes
    src, conf, s = _synthetic_scene(gpu)
    ref, keep, amb = R.trimmed_meshes(s["verts"], s["faces"], s["masks"], s["Ks"], s["poses"], 3)
    assert not amb.any()
    assert keep[s["owner"] != 1].all() and not keep[s["owner"] == 1].all()
    assert len(ref) == 2 and ref[0][1].shape[0] > ref[1][1].shape[0]
    got = create_trimmed_meshes(torch.from_numpy(s["verts"]).to(gpu), torch.from_numpy(s["faces"]).to(gpu), src, conf, pixel_margin=3)
    _check_meshes(got, ref)
    got = create_trimmed_meshes(s["verts"], s["faces"], src, conf, pixel_margin=3, max_meshes=1)       # numpy in
    _check_meshes(got, ref[:1])
    # nothing survives: a mesh wholly outside the first view's mask
    far = (s["verts"][s["owner"] == 2] + np.float32([0.0, 0.45, 0.0])).astype(np.float32)
    f2 = s["faces"][(s["owner"][s["faces"]] == 2).all(axis=1)] - int(np.nonzero(s["owner"] == 2)[0][0])
    assert R.trimmed_meshes(far, f2, s["masks"], s["Ks"], s["poses"], 3)[0] == []
    assert create_trimmed_meshes(far, f2, src, conf, pixel_margin=3) == []


def test_extract_writes_trimmed_meshes(gpu, tmp_path):
    from ndjir_amd import network, parameter as P
    from ndjir_amd.extract import TEXTURES, extract
    from tests.bake_ref import parse_obj
    src, conf, s = _synthetic_scene(gpu)
    P.clear_parameters()
    P.set_device(gpu)
    network.seed(313)
    ref, _, _ = R.trimmed_meshes(s["verts"], s["faces"], s["masks"], s["Ks"], s["poses"], 50)
    assert 1 <= len(ref) <= 5
    plain, trimmed = tmp_path / "plain", tmp_path / "trimmed"
    os.makedirs(plain)
    os.makedirs(trimmed)
    G = conf.extraction.grid_size
    raw = [f"net_{G}grid_raw_{t}_mesh00.obj" for t in TEXTURES]
    env = ["environment_map.png", "environment_map_min_max.txt"]
    # without a source: exactly the files written before
    last = extract(str(plain), "net", conf, s["verts"], s["faces"])
    assert sorted(os.listdir(plain)) == sorted(raw + env) and last == f"{plain}/{raw[-1]}"
    last = extract(str(trimmed), "net", conf, s["verts"], s["faces"], source=src)
    names = [f"net_{G}grid_trimmed_{t}_mesh{k:02d}.obj" for k in range(len(ref)) for t in TEXTURES]
    assert sorted(os.listdir(trimmed)) == sorted(raw + env + names)
    assert last == f"{trimmed}/net_{G}grid_trimmed_{TEXTURES[-1]}_mesh00.obj"
    for k, (rv, rf) in enumerate(ref):
        for t in TEXTURES:
            v, col, vn, f, fn = parse_obj(str(trimmed / f"net_{G}grid_trimmed_{t}_mesh{k:02d}.obj"))
            np.testing.assert_array_equal(v, rv)
            np.testing.assert_array_equal(f, rf + 1)
            assert col.shape == (len(rv), 3) and vn.shape == (len(rv), 3)
    # a training-time extraction writes the rough raw mesh only
    rough = tmp_path / "rough"
    os.makedirs(rough)
    extract(str(rough), "net", conf, s["verts"], s["faces"], train=True, source=src)
    assert not [n for n in os.listdir(rough) if "trimmed" in n]
