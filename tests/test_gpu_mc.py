"""Marching cubes on the device (ndjir_amd/mc.py, csrc/mc.hip) against the table-free restatement of the rule in
tests/mc_ref.py.  Every comparison is exact (vertex keys, order, fp32 bits of the positions, counts) or independent of how a
loop is cut into triangles (directed boundary segments per cell, global directed-edge counts, Euler characteristic,
orientation against the analytic gradient).  The Python reference visits active cells only."""
import os

import numpy as np
import pytest
import torch

from tests import mc_ref as R
from tests.parity_utils import small_conf

pytestmark = pytest.mark.gpu

BOX = ((-1.0, -2.0, -3.0), (1.0, 0.5, 2.0))


def _run(vol, level=0.0, direction="descent", mins=None, maxs=None, device=None):
    from ndjir_amd.mc import marching_cubes
    v, f = marching_cubes(torch.from_numpy(np.ascontiguousarray(vol)).to(device), level, direction, mins, maxs)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.dim() == 2 and f.dim() == 2
    assert v.shape[1] == 3 and f.shape[1] == 3 and v.device.type == f.device.type == torch.device(device).type
    return v.cpu().numpy(), f.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _keys_from_positions(pos, G):
    """(lin, axis) read back from lattice positions with exactly one fractional coordinate (no vertex on a lattice point)."""
    frac = pos != np.floor(pos)
    assert (frac.sum(axis=1) == 1).all()
    axis = frac.argmax(axis=1)
    ijk = np.floor(pos).astype(np.int64)
    return np.ravel_multi_index(tuple(ijk.T), G), axis


def _check(vol, level, device, direction="descent", closed=None, fractional=True):
    """The checks shared by the tests: vertex keys, order and bits; faces per cell against the rule's segments; `closed`:
    None (open surface), "balanced" (every directed edge as often as its reverse) or "manifold" (each exactly once)."""
    vol = np.asarray(vol, np.float32)
    verts, faces = _run(vol, level, direction, device=device)
    lin, axis = R.crossing_edges(vol, level)
    assert verts.shape[0] == len(lin)
    ref_pos = R.vertex_positions(vol, level, lin, axis)
    if fractional:                                        # the key set and the order, read from the device's own output
        got_lin, got_axis = _keys_from_positions(verts, vol.shape)
        np.testing.assert_array_equal(got_lin, lin)
        np.testing.assert_array_equal(got_axis, axis)
    np.testing.assert_array_equal(_bits(verts), _bits(ref_pos))
    cells = R.reference_mesh(vol, level, direction)[3]
    assert faces.shape[0] == sum(c[1] for c in cells)
    assert faces.min(initial=0) >= 0 and faces.max(initial=-1) < len(lin)
    per_cell = R.faces_per_cell(vol, faces, lin, axis, cells)          # also: every face lies in its cell, counts per cell
    for (origin, ntri, segs), tris in zip(cells, per_cell):
        assert R.boundary_segments(tris) == segs, (origin, tris, segs)
    if closed == "manifold":
        assert R.is_strictly_manifold(faces)
    elif closed == "balanced":
        assert R.is_balanced(faces)
    return verts, faces, lin, axis


# ---- 1. all 256 cases ---------------------------------------------------------------------------------------------------------

def test_all_cases(gpu):
    vol = R.all_cases_volume()
    _, f_desc, lin, _ = _check(vol, 0.0, gpu, "descent", closed="manifold")
    _, f_asc, _, _ = _check(vol, 0.0, gpu, "ascent", closed="manifold")
    # "ascent" is "descent" with the winding reversed, face by face
    np.testing.assert_array_equal(f_asc, f_desc[:, [0, 2, 1]])
    assert len(lin) == 4608


# ---- 2. shapes ----------------------------------------------------------------------------------------------------------------

def _grad_sphere(p, centre=(0.0, 0.0, 0.0)):
    return p - np.asarray(centre)


def _grad_torus(p, Rm=0.55):
    rho = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2)
    g = np.stack([(rho - Rm) * p[:, 0] / rho, (rho - Rm) * p[:, 1] / rho, p[:, 2]], axis=1)
    return g


def _grad_two(p, offset=0.45):
    c = np.where(p[:, :1] < 0, -offset, offset) * np.array([[1.0, 0.0, 0.0]])
    return p - c


ELL = (0.7, 0.5, 0.8)


def _ellipsoid(G):
    X, Y, Z = R.lattice(G)
    return (np.sqrt((X / ELL[0]) ** 2 + (Y / ELL[1]) ** 2 + (Z / ELL[2]) ** 2) - 1.0).astype(np.float32)


def _grad_ellipsoid(p):
    return p / (np.asarray(ELL) ** 2)[None, :]


SHAPES = {"sphere": (R.sphere, _grad_sphere, 2), "torus": (R.torus, _grad_torus, 0), "two_spheres": (R.two_spheres, _grad_two, 4),
          "ellipsoid": (_ellipsoid, _grad_ellipsoid, 2)}


@pytest.mark.parametrize("name,G", [("sphere", 12), ("torus", 12), ("two_spheres", 12), ("sphere", 33), ("torus", 33),
                                    ("two_spheres", 33), ("ellipsoid", (9, 13, 17))])
def test_shapes(gpu, name, G):
    make, grad, chi = SHAPES[name]
    vol = make(G)
    # two of these volumes hold an exact zero (a vertex on a lattice point), so the keys are not read back from positions
    verts, faces, lin, axis = _check(vol, 0.0, gpu, "descent", closed="manifold", fractional=False)
    assert R.euler_characteristic(len(verts), faces) == chi
    if G == 12:
        assert (len(verts), len(faces)) == {"sphere": (192, 380), "torus": (192, 384), "two_spheres": (112, 216)}[name]
    # orientation: in the coordinates the volume was sampled in, normals along the analytic gradient
    dims = np.asarray(vol.shape, np.float64)
    pos = -1.0 + 2.0 * verts.astype(np.float64) / (dims - 1.0)[None, :]
    f_asc = _run(vol, 0.0, "ascent", device=gpu)[1]
    np.testing.assert_array_equal(f_asc, faces[:, [0, 2, 1]])
    for f, sign in ((faces, 1.0), (f_asc, -1.0)):
        n = np.cross(pos[f[:, 1]] - pos[f[:, 0]], pos[f[:, 2]] - pos[f[:, 0]])
        dot = (n * grad(pos[f].mean(axis=1))).sum(axis=1)
        assert (sign * dot > 0).all(), (name, G, int((sign * dot <= 0).sum()))
    # world positions: the bits of numpy's fp32 multiply and add
    world, faces_w = _run(vol, 0.0, "descent", BOX[0], BOX[1], device=gpu)
    np.testing.assert_array_equal(_bits(world), _bits(R.vertex_positions(vol, 0.0, lin, axis, BOX[0], BOX[1])))
    np.testing.assert_array_equal(faces_w, faces)


# ---- 3. noise -----------------------------------------------------------------------------------------------------------------

def test_noise_open(gpu):
    vol = np.random.RandomState(0).randn(9, 7, 8).astype(np.float32)
    _check(vol, 0.0, gpu, "descent")
    _check(vol, 0.0, gpu, "ascent")


def test_noise_padded_and_repeatable(gpu):
    from ndjir_amd.mc import marching_cubes
    vol = np.pad(np.random.RandomState(0).randn(10, 11, 9).astype(np.float32), 1, constant_values=1.0)
    _check(vol, 0.0, gpu, "descent", closed="balanced")       # the rule itself doubles a few coincident fan diagonals here
    t = torch.from_numpy(vol).to(gpu)
    a, b = marching_cubes(t, 0.0, "descent", *BOX), marching_cubes(t, 0.0, "descent", *BOX)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 4. scan boundaries -------------------------------------------------------------------------------------------------------

def test_scan_odd_row_length(gpu):
    vol = np.random.RandomState(4).randn(3, 5, 1031).astype(np.float32)
    # index + t may round up to the next lattice point at indices near 1000, so the keys are not read back here: the bits of
    # the positions, in order, are compared all the same
    _check(vol, 0.0, gpu, "descent", fractional=False)


def _six_spheres():
    """(128, 96, 97) of +1 with six spheres of radius 2.5 (lattice units) centred on points whose linear index is a multiple
    of 1024 -- one of them 1024^2 -- so each straddles a block boundary of the scans and one the 1024th block total."""
    G = (128, 96, 97)
    centres, m = [np.unravel_index(1024 * 1024, G)], 97
    while len(centres) < 6:
        c = np.unravel_index(1024 * m, G)
        if all(3 <= c[a] < G[a] - 3 for a in range(3)) and all(np.abs(np.subtract(c, o)).max() > 6 for o in centres):
            centres.append(c)
            m += 211
        else:
            m += 1
    assert all(3 <= c[a] < G[a] - 3 for c in centres for a in range(3))
    I, J, K = np.meshgrid(*[np.arange(g, dtype=np.float64) for g in G], indexing="ij")
    vol = np.ones(G, np.float64)
    for c in centres:
        vol = np.minimum(vol, np.sqrt((I - c[0]) ** 2 + (J - c[1]) ** 2 + (K - c[2]) ** 2) - 2.5)
    return vol.astype(np.float32), centres


def test_scan_block_boundaries(gpu):
    vol, centres = _six_spheres()
    assert vol.size > 1024 * 1024 and any(np.ravel_multi_index(c, vol.shape) == 1024 * 1024 for c in centres)
    verts, faces, lin, _ = _check(vol, 0.0, gpu, "descent", closed="manifold")
    assert R.euler_characteristic(len(verts), faces) == 12
    for c in centres:                                     # each sphere owns vertices on both sides of its block boundary
        b = np.ravel_multi_index(c, vol.shape)
        assert ((lin >= b - 3 * 97 * 96) & (lin < b)).any() and ((lin >= b) & (lin < b + 3 * 97 * 96)).any()


# ---- 5. level and ties --------------------------------------------------------------------------------------------------------

def test_level_on_sphere(gpu):
    vol = R.sphere(12)
    verts, faces, lin, axis = _check(vol, 0.25, gpu, "descent", closed="manifold")
    assert R.euler_characteristic(len(verts), faces) == 2
    world = _run(vol, 0.25, "descent", BOX[0], BOX[1], device=gpu)[0]
    np.testing.assert_array_equal(_bits(world), _bits(R.vertex_positions(vol, 0.25, lin, axis, BOX[0], BOX[1])))


@pytest.mark.parametrize("level", [0.0, 0.25])
def test_ties(gpu, level):
    """Values exactly equal to the level, and -0.0 at level 0, are outside: vertices with t = 0 or 1 land on lattice points,
    still one per crossing edge; zero-area triangles are allowed."""
    rng = np.random.RandomState(5)
    vol = (np.round(rng.randn(6, 7, 8) * 2.0) / 4.0).astype(np.float32)
    zero = vol == 0
    vol[zero & (rng.uniform(size=vol.shape) < 0.5)] = -0.0
    assert (vol == np.float32(level)).sum() > 20 and np.signbit(vol[vol == 0]).any()
    verts, faces, lin, axis = _check(vol, level, gpu, "descent", fractional=False)
    assert (verts == np.floor(verts)).all(axis=1).any()          # some vertex sits on a lattice point
    _check(vol, level, gpu, "ascent", fractional=False)
    # the hand-made line of tests/test_mc_ref_cpu.py: counts and positions exact
    line = np.ones((2, 2, 3), np.float32)
    line[0, 0, 1], line[0, 0, 0], line[0, 0, 2] = -1.0, 0.0, -0.0
    v, f = _run(line, 0.0, device=gpu)
    np.testing.assert_array_equal(_bits(v), _bits(np.float32([[0, 0, 0], [0.5, 0, 1], [0, 0.5, 1], [0, 0, 2]])))
    assert f.shape == (2, 3)


# ---- 6. degenerate inputs -----------------------------------------------------------------------------------------------------

def test_degenerate_inputs(gpu):
    from ndjir_amd.mc import marching_cubes
    for vol in (np.ones((5, 6, 7), np.float32), -np.ones((5, 6, 7), np.float32), np.random.RandomState(1).randn(1, 5, 5),
                np.random.RandomState(1).randn(5, 1, 5), np.random.RandomState(1).randn(5, 5, 1)):
        v, f = _run(vol.astype(np.float32), 0.0, device=gpu)
        assert v.shape == (0, 3) and f.shape == (0, 3)
    one = np.ones((2, 2, 2), np.float32)
    assert _run(one, 0.0, device=gpu)[0].shape == (0, 3)
    one[1, 0, 1] = -1.0
    v, f, _, _ = _check(one, 0.0, gpu, "descent")
    assert v.shape == (3, 3) and f.shape == (1, 3)
    noise = np.random.RandomState(2).randn(2, 2, 2).astype(np.float32)
    _check(noise, 0.0, gpu, "descent")
    bad = np.ones((4, 4, 4), np.float32)
    t = torch.from_numpy(bad).to(gpu)
    with pytest.raises(ValueError):
        marching_cubes(t, 0.0, "sideways")
    with pytest.raises(ValueError):
        marching_cubes(t[0], 0.0)
    with pytest.raises(ValueError):
        marching_cubes(torch.zeros((4, 4, 4), dtype=torch.complex64, device=gpu), 0.0)
    for poison in (np.nan, np.inf, -np.inf):
        bad[1, 2, 3] = poison
        with pytest.raises(ValueError):
            marching_cubes(torch.from_numpy(bad).to(gpu), 0.0)


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------

def _look_at(centre):
    centre = np.asarray(centre, np.float64)
    z = -centre / np.linalg.norm(centre)
    x = np.cross([0.0, 1.0, 0.3], z)
    x /= np.linalg.norm(x)
    pose = np.eye(4)
    pose[:3, :3] = np.stack([x, np.cross(z, x), z], axis=1)
    pose[:3, 3] = centre
    return pose.astype(np.float32)


def test_extract_scene(gpu, tmp_path):
    from ndjir_amd import network, parameter as P
    from ndjir_amd.dataset import IDRRaySource
    from ndjir_amd.extract import (TEXTURES, bake_vertex_attributes, compute_vol, create_mesh_from_volume, extract,
                                   extract_scene)
    from tests.bake_ref import parse_obj
    G = 24
    conf = small_conf(grid_size=16, overrides=[f"extraction.rough_grid_size={G}", f"extraction.grid_size={G}"])
    P.clear_parameters()
    P.set_device(gpu)
    network.seed(313)
    scene, hand = tmp_path / "scene", tmp_path / "hand"
    os.makedirs(scene)
    os.makedirs(hand)
    last = extract_scene(str(scene), "net", conf, train=True)
    names = sorted([f"net_{G}grid_raw_{t}_mesh00.obj" for t in TEXTURES] + ["environment_map.png", "environment_map_min_max.txt"])
    assert sorted(os.listdir(scene)) == names and last == f"{scene}/net_{G}grid_raw_{TEXTURES[-1]}_mesh00.obj"
    # the same by hand
    r = float(conf.renderer.bounding_sphere_radius)
    mins, maxs = np.asarray([-r] * 3), np.asarray([r] * 3)
    vol = compute_vol(mins, maxs, G, conf)
    verts, faces = create_mesh_from_volume(vol, conf.extraction.level, mins, maxs, G, conf.extraction.gradient_direction)
    extract(str(hand), "net", conf, verts, faces, train=True)
    for n in names:
        assert open(scene / n, "rb").read() == open(hand / n, "rb").read(), n
    v, _, _, f, _ = parse_obj(str(scene / names[-1]))
    np.testing.assert_array_equal(v, verts.cpu().numpy())
    np.testing.assert_array_equal(f, faces.cpu().numpy() + 1)
    # geometric init: one sphere; the vertices lie on the net's zero set to within one lattice step of the volume
    fn = faces.cpu().numpy()
    assert R.euler_characteristic(verts.shape[0], fn) == 2 and R.is_strictly_manifold(fn)
    step = max(float((vol[1:] - vol[:-1]).abs().max()), float((vol[:, 1:] - vol[:, :-1]).abs().max()),
               float((vol[:, :, 1:] - vol[:, :, :-1]).abs().max()))
    sdf = bake_vertex_attributes(verts, conf)["sdf"]
    assert float(sdf.abs().max()) < step, (float(sdf.abs().max()), step)
    # numpy volume in, and the reference's default direction ("ascent") is the other winding
    v2, f2 = create_mesh_from_volume(vol.cpu().numpy(), conf.extraction.level, mins, maxs, G)
    assert torch.equal(v2, verts) and torch.equal(f2, faces[:, [0, 2, 1]])
    # with a source and not train: the trimmed meshes too, with valid indices
    # the sphere (radius 0.35, three units away) covers about 18 pixels around the image centre; the second view's mask
    # starts 55 pixels right of it, so its 50-pixel dilation cuts the sphere about 5 pixels right of its centre
    H, W, M = 160, 240, 2
    K = np.array([[150.0, 0.0, 120.0], [0.0, 150.0, 80.0], [0.0, 0.0, 1.0]])
    poses = np.stack([_look_at([0.0, 0.0, -3.0]), _look_at([0.0, -3.0, 0.3])])
    masks = np.ones((M, H, W, 1), np.float32)
    masks[1, :, :W // 2 + 55] = 0.0
    src = IDRRaySource(np.zeros((M, H, W, 3), np.float32), masks, np.stack([K] * M), poses, conf, device=gpu)
    trimmed = tmp_path / "trimmed"
    os.makedirs(trimmed)
    last = extract_scene(str(trimmed), "net", conf, train=False, source=src)
    tnames = [n for n in os.listdir(trimmed) if "_trimmed_" in n]
    assert sorted(set(os.listdir(trimmed)) - set(tnames)) == names
    assert tnames and len(tnames) % len(TEXTURES) == 0 and "_trimmed_" in last
    for n in tnames:
        tv, col, vn, tf, _ = parse_obj(str(trimmed / n))
        assert 0 < len(tv) < verts.shape[0] and len(tf) > 0 and tf.min() >= 1 and tf.max() <= len(tv)
        assert col.shape == tv.shape and vn.shape == tv.shape
    # an empty level set names the level and the range
    conf_hi = small_conf(grid_size=16, overrides=[f"extraction.rough_grid_size={G}", "extraction.level=50.0"])
    with pytest.raises(ValueError, match="level 50"):
        extract_scene(str(tmp_path), "none", conf_hi, train=True)
