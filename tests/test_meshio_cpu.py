"""Writers of the mesh export (ndjir_amd/meshio.py), the export's file names and the texture placement table of
python/extract_by_mc.py:187-216 -- no GPU."""
import os

import numpy as np
import pytest
import torch

from ndjir_amd import config as cfg
from ndjir_amd import extract as E
from ndjir_amd import meshio
from tests import bake_ref as R


def _mesh():
    rng = np.random.RandomState(3)
    verts = rng.randn(5, 3).astype(np.float32)
    verts[0] = [1.0 / 3.0, -2.5e-7, 123456.789]                 # values that need all nine digits
    colors = rng.rand(5, 3).astype(np.float32)
    colors[1] = [0.0, 1.0, np.float32(0.1)]
    normals = meshio.normalize_rows(rng.randn(5, 3))
    faces = np.array([[0, 1, 2], [2, 3, 4], [4, 0, 3]])
    return verts, colors, normals, faces


def test_obj_round_trips_fp32_exactly(tmp_path):
    verts, colors, normals, faces = _mesh()
    path = meshio.write_obj(str(tmp_path / "m.obj"), verts, faces, colors=colors, normals=normals)
    v, c, n, f, fn = R.parse_obj(path)
    np.testing.assert_array_equal(v, verts)
    np.testing.assert_array_equal(c, colors)
    np.testing.assert_array_equal(n, normals)
    np.testing.assert_array_equal(f, faces + 1)                  # 1-based
    np.testing.assert_array_equal(fn, faces + 1)                 # a//a: the vertex's own normal
    assert f.min() == 1 and f.max() == 5
    np.testing.assert_allclose(np.linalg.norm(n.astype(np.float64), axis=1), 1.0, atol=1e-6)
    back = meshio.read_obj(path)
    np.testing.assert_array_equal(back["verts"], verts)
    np.testing.assert_array_equal(back["colors"], colors)
    np.testing.assert_array_equal(back["faces"], faces)
    lines = open(path).read().splitlines()
    assert [l.split()[0] for l in lines] == ["v"] * 5 + ["vn"] * 5 + ["f"] * 3
    assert all(len(l.split()) == 7 for l in lines[:5])
    with pytest.raises(ValueError):
        meshio.write_obj(str(tmp_path / "bad.obj"), verts, faces + 3)


@pytest.mark.parametrize("shape", [(3, 5), (3, 5, 3)])
def test_png_decodes_to_the_image(tmp_path, shape):
    img = np.random.RandomState(5).randint(0, 256, size=shape).astype(np.uint8)
    img.reshape(-1)[:2] = [0, 255]
    path = meshio.write_png(str(tmp_path / "i.png"), img)
    out = R.decode_png(path)
    assert out.shape == shape
    np.testing.assert_array_equal(out, img)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(path) as im:
            assert im.mode == ("L" if len(shape) == 2 else "RGB")
            np.testing.assert_array_equal(np.asarray(im), img)
    with pytest.raises(ValueError):
        meshio.write_png(str(tmp_path / "f.png"), img.astype(np.float32))


def test_min_max_text(tmp_path):
    path = meshio.write_min_max(str(tmp_path / "environment_map_min_max.txt"), np.float32(0.25), np.float32(1.5))
    assert open(path).read() == "min, max = 0.25, 1.5"


def test_extraction_defaults():
    e = cfg.load("default").extraction
    assert (e.level, e.rough_grid_size, e.grid_size, e.batch_size, e.gradient_direction) == (0.0, 128, 512, 50000, "descent")


@pytest.mark.parametrize("train,G", [(False, 512), (True, 128)])
def test_mesh_file_names(tmp_path, monkeypatch, train, G):
    """`{fname}_{G}grid_{type}_{texture}_mesh{idx:02d}.obj` (extract_by_mc.py:218), the last path returned (:223)."""
    verts, colors, normals, faces = _mesh()
    baked = {name: torch.from_numpy(colors * (i + 1) / 6) for i, name in enumerate(E.TEXTURES)}
    baked["normal"] = torch.from_numpy(normals * 3)
    monkeypatch.setattr(E, "bake_vertex_attributes", lambda points, conf, **kw: baked)
    conf = cfg.load("default")
    last = E.save_attributed_mesh(str(tmp_path), "model", verts, faces, conf, train=train, type="trimmed", idx=3)
    names = [f"model_{G}grid_trimmed_{t}_mesh03.obj" for t in R.TEXTURES]
    assert sorted(os.listdir(tmp_path)) == sorted(names)
    assert last == f"{tmp_path}/{names[-1]}" and names[-1].endswith("specular_reflectance_std_mesh03.obj")
    for i, n in enumerate(names):
        v, c, vn, f, _ = R.parse_obj(str(tmp_path / n))
        np.testing.assert_array_equal(v, verts)
        np.testing.assert_array_equal(c, colors * (i + 1) / 6)
        np.testing.assert_allclose(vn, normals, atol=2e-7)       # normalised SDF gradient
        np.testing.assert_array_equal(f, faces + 1)


@pytest.mark.parametrize("ci", [1, 3])
@pytest.mark.parametrize("cs", [1, 3])
def test_texture_placement_table(ci, cs):
    """Shapes and channel rules of the six textures, and the product's stock-op placement (`extract._place`) against the
    restatement of `create_rgb_color`."""
    rng = np.random.RandomState(ci * 10 + cs)
    N = 9
    bc, imp, r, s = rng.rand(N, 3), rng.rand(N, ci) * 1.5 - 0.2, rng.rand(N, 1), rng.rand(N, cs)
    r_std, s_std = rng.rand(N, 1) * 1.4, rng.rand(N, cs) * 0.7
    tex = R.place_textures(bc, imp, r, s, r_std, s_std)
    assert tuple(tex) == R.TEXTURES == E.TEXTURES
    for k, t in tex.items():
        assert t.shape == (N, 3) and t.min() >= 0.0 and t.max() <= 1.0, k
    np.testing.assert_array_equal(tex["base_color"], bc)
    filled = {"implicit_illumination": [2] if ci == 1 else [0, 1, 2], "roughness": [1], "roughness_std": [1],
              "specular_reflectance": [0] if cs == 1 else [0, 1, 2], "specular_reflectance_std": [0] if cs == 1 else [0, 1, 2]}
    for k, ch in filled.items():
        empty = [c for c in range(3) if c not in ch]
        assert (tex[k][:, empty] == 0).all() and (tex[k][:, ch] > 0).any(), k
    np.testing.assert_array_equal(tex["implicit_illumination"][:, filled["implicit_illumination"]], np.clip(imp, 0, 1))
    # std textures: clipped first, then divided by their own maximum -> the maximum is exactly 1
    np.testing.assert_array_equal(tex["roughness_std"][:, 1:2], np.clip(r_std, 0, 1) / np.clip(r_std, 0, 1).max())
    assert tex["roughness_std"].max() == 1.0 and tex["specular_reflectance_std"].max() == 1.0
    assert np.clip(s_std, 0, 1).max() < 1.0                       # ... also where nothing was clipped
    for v, dim in ((bc, 0), (imp, 2), (r, 1), (s, 0)):
        np.testing.assert_array_equal(E._place(torch.from_numpy(v), dim).numpy(),
                                      R.create_rgb_color(v, dim if v.shape[1] == 1 else -1))
