"""Marching cubes without a GPU: the case table the C library generates (`ndjir_mc_case_table`, host code) against the
table-free restatement of the rule in tests/mc_ref.py, for all 256 cases, and the restatement's own results on three
analytic volumes (vertex / face counts and Euler characteristic worked out when the rule was prototyped)."""
import os

import numpy as np
import pytest

from tests import mc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(os.path.join(ROOT, "ndjir_amd", "_lib", "libndjir_hip.so")):
        import __graft_entry__ as g
        g.build()
    from ndjir_amd.mc import case_table
    t = case_table()
    assert t.shape == (256, 16) and t.dtype == np.uint8
    return t


def _inside8(c):
    return [(c >> b) & 1 for b in range(8)]


def _crossing(c):
    """The cube edges whose two corners differ in case c."""
    out = set()
    for a in range(8):
        for ax in range(3):
            b = a ^ (1 << ax)
            if a < b and ((c >> a) & 1) != ((c >> b) & 1):
                out.add(R.edge_id(a, b))
    return out


def test_numbering():
    # x edges leave corners 0, 2, 4, 6; y edges 0, 1, 4, 5; z edges 0, 1, 2, 3
    assert [R.edge_id(c, c + 1) for c in (0, 2, 4, 6)] == [0, 1, 2, 3]
    assert [R.edge_id(c, c + 2) for c in (0, 1, 4, 5)] == [4, 5, 6, 7]
    assert [R.edge_id(c, c + 4) for c in (0, 1, 2, 3)] == [8, 9, 10, 11]
    # every face walk turns about its outward normal
    pos = lambda c: np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], float)
    for w in R.FACE_WALKS:
        n = np.cross(pos(w[1]) - pos(w[0]), pos(w[2]) - pos(w[1]))
        centre = sum(pos(c) for c in w) / 4 - 0.5
        assert n @ centre > 0


def test_rule_facts():
    """Over all cases: at most 5 triangles, loops of 3 to 7 vertices, at most 4 loops; every crossing edge starts one segment
    and ends one."""
    most_tri = longest = most_loops = 0
    for c in range(256):
        segs, loops = R.cell_segments(_inside8(c))
        assert sorted(a for a, _ in segs) == sorted(b for _, b in segs) == sorted(_crossing(c))
        assert sorted(e for loop in loops for e in loop) == sorted(_crossing(c))
        assert all(len(loop) >= 3 for loop in loops)
        most_tri = max(most_tri, sum(len(loop) - 2 for loop in loops))
        longest = max([longest] + [len(loop) for loop in loops])
        most_loops = max(most_loops, len(loops))
    assert (most_tri, longest, most_loops) == (5, 7, 4)
    # one inside corner at the origin: the loop's right-hand normal points at the corner (toward decreasing values)
    segs, loops = R.cell_segments(_inside8(1))
    assert sorted(segs) == [(0, 8), (4, 0), (8, 4)] and loops == [[0, 8, 4]]


@pytest.mark.parametrize("block", range(8))
def test_case_table_matches_the_rule(table, block):
    for c in range(32 * block, 32 * block + 32):
        row = table[c]
        segs, loops = R.cell_segments(_inside8(c))
        ntri = int(row[0])
        assert ntri == sum(len(loop) - 2 for loop in loops) and ntri <= 5
        tris = [tuple(int(e) for e in row[1 + 3 * t:4 + 3 * t]) for t in range(ntri)]
        assert not row[1 + 3 * ntri:].any()
        assert {e for t in tris for e in t} <= _crossing(c)
        assert all(e < 12 for t in tris for e in t)
        # "descent": the boundary of the row's triangles is the rule's segments reversed
        assert R.boundary_segments(tris) == sorted((b, a) for a, b in segs)
        if ntri:
            assert {e for t in tris for e in t} == _crossing(c)


@pytest.mark.parametrize("name,expect", [("sphere", (192, 380, 2)), ("torus", (192, 384, 0)), ("two_spheres", (112, 216, 4))])
def test_reference_on_analytic_volumes(name, expect):
    vol = getattr(R, name)(12)
    lin, axis, faces, cells = R.reference_mesh(vol, 0.0)
    assert (len(lin), len(faces), R.euler_characteristic(len(lin), faces)) == expect
    assert R.is_strictly_manifold(faces)
    # "descent": normals along the gradient (outward for a signed distance)
    pos = R.vertex_positions(vol, 0.0, lin, axis, (-1, -1, -1), (1, 1, 1)).astype(np.float64)
    faces2 = R.reference_mesh(vol, 0.0, "ascent")[2]
    assert len(faces2) == len(faces) and R.is_strictly_manifold(faces2)
    if name == "sphere":
        for f, sign in ((faces, 1.0), (faces2, -1.0)):
            n = np.cross(pos[f[:, 1]] - pos[f[:, 0]], pos[f[:, 2]] - pos[f[:, 0]])
            assert (sign * (n * pos[f].mean(axis=1)).sum(axis=1) > 0).all()


def test_reference_all_cases_and_noise():
    vol = R.all_cases_volume()
    lin, axis, faces, cells = R.reference_mesh(vol, 0.0)
    assert R.is_strictly_manifold(faces)
    per_cell = R.faces_per_cell(vol, faces, lin, axis, cells)
    for (origin, ntri, segs), tris in zip(cells, per_cell):
        assert R.boundary_segments(tris) == segs
    noise = np.pad(np.random.RandomState(0).randn(10, 11, 9).astype(np.float32), 1, constant_values=1.0)
    faces = R.reference_mesh(noise, 0.0)[2]
    assert R.is_balanced(faces)


def test_vertex_positions_ties():
    vol = np.ones((2, 2, 3), np.float32)
    vol[0, 0, 1] = -1.0
    vol[0, 0, 0] = 0.0            # equal to the level: outside, t = 0 on the edge toward the inside point
    vol[0, 0, 2] = -0.0           # -0.0 is outside at level 0 too, t = 1 seen from the inside point
    lin, axis = R.crossing_edges(vol, 0.0)
    assert list(zip(lin.tolist(), axis.tolist())) == [(0, 2), (1, 0), (1, 1), (1, 2)]
    pos = R.vertex_positions(vol, 0.0, lin, axis)
    np.testing.assert_array_equal(pos, np.float32([[0, 0, 0], [0.5, 0, 1], [0, 0.5, 1], [0, 0, 2]]))
