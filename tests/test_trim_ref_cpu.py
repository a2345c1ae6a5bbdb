"""The numpy restatement the trimming tests compare against (tests/trim_ref.py), checked on the CPU against scipy: its
dilation against `scipy.ndimage.binary_dilation`, the ellipse's row table against the two facts known about it, and its
component labels on hand-made meshes."""
import numpy as np
import pytest

from tests import trim_ref as R


@pytest.mark.parametrize("r", [0, 1, 5, 50])
@pytest.mark.parametrize("density", [0.005, 0.5])
def test_dilation_matches_scipy(r, density):
    from scipy.ndimage import binary_dilation
    rng = np.random.RandomState(100 + r)
    mask = rng.uniform(size=(67, 131)) < density
    mask[0, 0] = mask[66, 130] = True
    ref = binary_dilation(mask, structure=R.ellipse(r), border_value=0)
    np.testing.assert_array_equal(R.dilate(mask, r), ref)


def test_ellipse_table_facts():
    np.testing.assert_array_equal(R.ellipse_half_widths(5), [0, 3, 4, 5, 5, 5, 5, 5, 4, 3, 0])
    assert R.ellipse(50).sum() == 7957
    np.testing.assert_array_equal(R.ellipse_half_widths(0), [0])
    from ndjir_amd.trim import ellipse_half_widths
    for r in (0, 1, 2, 5, 50, 127):
        np.testing.assert_array_equal(ellipse_half_widths(r), R.ellipse_half_widths(r))


def test_padded_mask_frame_and_threshold():
    m = np.zeros((5, 7), np.float32)
    m[2, 3], m[0, 0], m[4, 6] = 0.5, 0.49, 0.51
    p = R.padded_mask(m, 0)
    assert p.shape == (7, 9) and p.dtype == np.uint8
    assert p[0].all() and p[-1].all() and p[:, 0].all() and p[:, -1].all()
    inner = p[1:-1, 1:-1]
    assert inner[2, 3] == 1 and inner[0, 0] == 0 and inner[4, 6] == 1 and inner.sum() == 2


@pytest.mark.parametrize("name", list(R.component_cases()))
def test_component_labels(name):
    faces, n_verts, n_components = R.component_cases()[name]
    lab = R.component_labels(faces)
    assert lab.shape == (len(faces),) and faces.max() < n_verts
    assert (lab <= np.arange(len(faces))).all() and (lab[lab] == lab).all()       # canonical: a root labels itself
    if n_components is not None:
        assert len(np.unique(lab)) == n_components
    else:
        print(f"{name}: {len(np.unique(lab))} components")
        assert 1 < len(np.unique(lab)) < len(faces)


def test_split_order_and_submeshes():
    faces, n_verts, _ = R.component_cases()["sphere_and_floaters"]
    verts = np.arange(n_verts * 3, dtype=np.float32).reshape(n_verts, 3)
    meshes, n = R.split(verts, faces)
    assert n == 5 and [len(f) for _, f in meshes] == [len(faces) - 10, 4, 4, 1, 1]
    # equal sizes: the component with the smaller first face comes first (the tetrahedron listed before the sphere)
    assert meshes[1][0][0, 0] < meshes[2][0][0, 0] and meshes[3][0][0, 0] < meshes[4][0][0, 0]
    for v, f in meshes:
        assert f.min() == 0 and f.max() == len(v) - 1 and len(np.unique(f)) == len(v)
        assert (np.diff(v[:, 0]) > 0).all()                      # ascending original index
    assert len(R.split(verts, faces, max_meshes=2)[0]) == 2
