"""Host side of the grouped weight-gradient call (ndjir_amd/mlp.py): the `WgradGroupCall` record against the C declaration it is
turned into, the per-element rules of its builder, `_merge_same_destination` and `wgrad_jobs`.  No launch: CPU tensors, `_Strided`
replaced by the identity, the library's size queries by a recorder."""
import dataclasses
import os
import re

import pytest
import torch

from ndjir_amd import lib, mlp

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ndjir_hip.h")


def _declared(name):
    """Parameter names of `int ndjir_<name>(...)` in the header, without the trailing stream."""
    with open(HEADER) as f:
        m = re.search(r"\bint ndjir_%s\(([^;]*?)\);" % name, f.read(), re.S)
    names = [re.search(r"(\w+)\s*$", p).group(1) for p in m.group(1).split(",")]
    assert names[-1] == "stream"
    return names[:-1]


@pytest.fixture(autouse=True)
def _cpu_operands(monkeypatch):
    monkeypatch.setattr(mlp, "_Strided", lambda t: t)
    monkeypatch.setattr(mlp, "WGRAD_GROUP_ITEMS", 0)


def _blocked(t):
    """`t` as a point-blocked operand (`PB` itself only wraps GPU tensors)."""
    b = object.__new__(mlp.PB)
    b.t, b.c0, b.c1 = t, 0, t.shape[1]
    return b


def _got(jobs, extras=()):
    call = mlp.WgradGroupCall.build(jobs, extras)
    args = call.args()
    assert len(args) == len(lib.SIGS["mlp_wgrad_group"]) == 25
    return call, dict(zip(_declared("mlp_wgrad_group"), args))


def _same(got, want):
    """Lists of tensors compare by identity, everything else by value."""
    assert len(got) == len(want)
    return all((g is w) if (torch.is_tensor(w) or isinstance(w, mlp.PB)) else (g == w and type(g) is type(w)) for g, w in zip(got, want))


def test_fields_are_the_header_parameters_in_order():
    fields = [f.name for f in dataclasses.fields(mlp.WgradGroupCall)]
    assert fields[-3:] == ["kind", "flops", "shape"]
    assert fields[:-3] == _declared("mlp_wgrad_group") and len(fields) == 28
    assert len(mlp.WgradGroupCall().args()) == len(lib.SIGS["mlp_wgrad_group"])
    assert mlp.WgradSource._fields == ("A", "B", "amax_a", "amax_b") and mlp.WgradJob._fields == ("out", "accum", "sources")
    assert mlp.BiasPartial._fields == ("grad", "partial", "floats", "rows", "row_stride")


def test_one_job_one_source():
    A, B, out, ma, mb = torch.zeros(32, 3), torch.zeros(32, 8), torch.zeros(3, 8), torch.zeros(1), torch.zeros(1)
    call, got = _got([(out, False, [(A, B, ma, mb)])])
    assert (got["n_src"], got["n_out"], got["n_extra"], got["target_items"], got["workspace"]) == (1, 1, 0, 0, None)
    assert _same(got["A"], [A]) and _same(got["B"], [B]) and _same(got["out"], [out])
    assert _same(got["amax_a"], [ma]) and _same(got["amax_b"], [mb])
    assert (got["lda"], got["ldb"], got["P"], got["out_id"], got["layout"]) == ([3], [8], [32], [0], [0])
    assert (got["ldo"], got["K"], got["N"], got["accum"]) == ([8], [3], [8], [0])
    assert [got[k] for k in ("ex_out", "ex_partial", "ex_n", "ex_S", "ex_stride", "ex_accum")] == [[]] * 6
    assert call.kind == "wgrad" and call.flops == 1536.0 and call.nbytes == 1504.0         # 2 * 32 * 3 * 8; 4 * (32 * 11 + 24)
    assert call.shape == "group 1 out / 1 src 0.0 GMAC 32:3x8"


def test_one_job_two_sources_accumulated():
    A0, B0, A1, B1, out = torch.zeros(32, 8), torch.zeros(32, 3), torch.zeros(1, 8), torch.zeros(1, 3), torch.zeros(8, 3)
    call, got = _got([(out, True, [(A0, B0, None, None), (A1, B1, None, None)])])
    assert (got["n_src"], got["n_out"]) == (2, 1) and _same(got["A"], [A0, A1]) and _same(got["B"], [B0, B1])
    assert got["amax_a"] == [None, None] and got["amax_b"] == [None, None]
    assert (got["lda"], got["ldb"], got["P"], got["out_id"], got["layout"]) == ([8, 8], [3, 3], [32, 1], [0, 0], [0, 0])
    assert (got["ldo"], got["K"], got["N"], got["accum"]) == ([3], [8], [3], [1])
    assert call.flops == 1584.0 and call.nbytes == 1644.0            # 2 * 33 * 24; 4 * (33 * 11 + 2 * 24)


def test_two_jobs():
    A0, B0, A1, B1 = torch.zeros(32, 3), torch.zeros(32, 8), torch.zeros(32, 8), torch.zeros(32, 1)
    o0, o1 = torch.zeros(3, 8), torch.zeros(8, 1)
    call, got = _got([(o0, True, [(A0, B0, None, None)]), (o1, False, [(A1, B1, None, None)])])
    assert (got["n_src"], got["n_out"]) == (2, 2) and _same(got["out"], [o0, o1]) and _same(got["A"], [A0, A1])
    assert (got["lda"], got["ldb"], got["P"], got["out_id"]) == ([3, 8], [8, 1], [32, 32], [0, 1])
    assert (got["ldo"], got["K"], got["N"], got["accum"]) == ([8, 1], [3, 8], [8, 1], [1, 0])
    assert call.flops == 2048.0 and call.nbytes == 2784.0            # 2 * 32 * (24 + 8); 4 * (32 * 11 + 32 * 9 + 2 * 24 + 8)
    assert call.shape == "group 2 out / 2 src 0.0 GMAC 32:3x8,32:8x1"


def test_one_row_sources_take_their_width_as_row_stride():
    wide_a, wide_b = torch.zeros(1, 16), torch.zeros(1, 16)
    A, B = wide_a[:, :3], wide_b[:, :8]                    # (a one-row view's stride(0) is arbitrary: the width is passed)
    call, got = _got([(torch.zeros(3, 8), False, [(A, B, None, None)])])
    assert (got["lda"], got["ldb"], got["P"]) == ([3], [8], [1])
    assert call.flops == 48.0 and call.nbytes == 140.0               # 2 * 1 * 24; 4 * (11 + 24)
    # ... and rows of a wider buffer keep the buffer's row stride
    A, B = torch.zeros(32, 16)[:, :3], torch.zeros(32, 16)[:, :8]
    got = _got([(torch.zeros(3, 8), False, [(A, B, None, None)])])[1]
    assert (got["lda"], got["ldb"], got["P"]) == ([16], [16], [32])


def test_one_row_output_and_column_slice_output():
    out = torch.zeros(1, 16)[:, :8]                        # K = 1: ldo = N
    call, got = _got([(out, False, [(torch.zeros(32, 1), torch.zeros(32, 8), None, None)])])
    assert (got["ldo"], got["K"], got["N"], got["lda"], got["ldb"]) == ([8], [1], [8], [1], [8])
    assert call.flops == 512.0 and call.nbytes == 1184.0             # 2 * 32 * 8; 4 * (32 * 9 + 8)
    buf = torch.zeros(3, 9)
    out = buf[:, 1:]                                       # columns 1.. of a wider gradient buffer: row stride 9, N = 8
    got = _got([(out, True, [(torch.zeros(32, 3), torch.zeros(32, 8), None, None)])])[1]
    assert (got["ldo"], got["K"], got["N"], got["accum"]) == ([9], [3], [8], [1]) and got["out"][0] is out
    out = torch.zeros(8, 4)[:, :1]                         # N = 1: a column (stride(1) is free), row stride of the buffer
    got = _got([(out, False, [(torch.zeros(32, 8), torch.zeros(32, 1), None, None)])])[1]
    assert (got["ldo"], got["K"], got["N"]) == ([4], [8], [1])


@pytest.mark.parametrize("blocked_a,blocked_b,layout", [(True, False, 1), (False, True, 2), (True, True, 3)])
def test_point_blocked_operands_set_layout_bits(blocked_a, blocked_b, layout):
    A, B = torch.zeros(32, 8), torch.zeros(32, 3)
    a, b = (_blocked(A) if blocked_a else A), (_blocked(B) if blocked_b else B)
    row = torch.zeros(32, 8), torch.zeros(32, 3)
    call, got = _got([(torch.zeros(8, 3), True, [(a, b, None, None), (*row, None, None)])])
    assert got["layout"] == [layout, 0] and _same(got["A"], [a, row[0]]) and _same(got["B"], [b, row[1]])
    assert (got["lda"], got["ldb"], got["P"]) == ([8, 8], [3, 3], [32, 32])
    assert call.flops == 3072.0 and call.nbytes == 3008.0            # 2 * 64 * 24; 4 * (64 * 11 + 2 * 24)


def test_no_jobs_two_bias_partials():
    g0, g1, region = torch.zeros(8), torch.zeros(3), torch.zeros(3 * 12)
    extras = [mlp.BiasPartial(g0, region, 8, 3, 12), (g1, region[8:], 3, 3, 12)]
    call, got = _got([], extras)
    assert (got["n_src"], got["n_out"], got["n_extra"]) == (0, 0, 2)
    for k in ("A", "lda", "B", "ldb", "P", "amax_a", "amax_b", "out_id", "out", "ldo", "K", "N", "accum", "layout"):
        assert got[k] == [], k
    assert got["ex_out"][0] is g0 and got["ex_out"][1] is g1
    assert got["ex_partial"][0] is region and got["ex_partial"][1].data_ptr() == region.data_ptr() + 32
    assert (got["ex_n"], got["ex_S"], got["ex_stride"], got["ex_accum"]) == ([8, 3], [3, 3], [12, 12], [1, 1])
    assert call.flops == 0.0 and call.nbytes == 0.0 and call.shape == "group 0 out / 0 src 0.0 GMAC "
    # the extras ride along with jobs unchanged
    with_job = _got([(torch.zeros(3, 8), True, [(torch.zeros(32, 3), torch.zeros(32, 8), None, None)])], extras)[1]
    assert with_job["n_extra"] == 2 and with_job["ex_n"] == [8, 3] and with_job["n_src"] == 1


def test_shape_and_stride_asserts():
    ok = (torch.zeros(32, 3), torch.zeros(32, 8), None, None)
    for bad in [(torch.zeros(32, 8), ok[1], None, None),                 # A's width is not K
                (ok[0], torch.zeros(32, 3), None, None),                 # B's width is not N
                (ok[0], torch.zeros(8, 8), None, None),                  # different numbers of rows
                (torch.zeros(32, 6)[:, ::2], ok[1], None, None),         # A's column stride
                (ok[0], torch.zeros(32, 16)[:, ::2], None, None)]:       # B's column stride
        with pytest.raises(AssertionError):
            mlp.WgradGroupCall.build([(torch.zeros(3, 8), False, [bad])])
    with pytest.raises(AssertionError):
        mlp.WgradGroupCall.build([(torch.zeros(3, 16)[:, ::2], False, [ok])])


def test_tuples_and_records_give_the_same_arguments():
    A, B, A1, B1, out, o1, ma = torch.zeros(32, 3), torch.zeros(32, 8), torch.zeros(1, 8), torch.zeros(1, 1), torch.zeros(3, 8), torch.zeros(8, 1), torch.zeros(1)
    g, region = torch.zeros(3), torch.zeros(36)
    plain = mlp.WgradGroupCall.build([(out, True, [(A, B, ma, None), (A, B, None, ma)]), (o1, False, ((A1, B1, None, None),))],
                                     [(g, region, 3, 3, 12)])
    named = mlp.WgradGroupCall.build([mlp.WgradJob(out, True, [mlp.WgradSource(A, B, ma, None), mlp.WgradSource(A, B, None, ma)]),
                                      mlp.WgradJob(o1, False, [mlp.WgradSource(A1, B1, None, None)])],
                                     [mlp.BiasPartial(g, region, 3, 3, 12)])
    for name, p, n in zip(_declared("mlp_wgrad_group"), plain.args(), named.args()):
        assert _same(p, n) if isinstance(p, list) else p == n, name
    assert (plain.kind, plain.flops, plain.shape, plain.nbytes) == (named.kind, named.flops, named.shape, named.nbytes)


def test_size_queries_take_the_records_own_lists(monkeypatch):
    asked = []
    monkeypatch.setattr(lib, "query", lambda name, *args: asked.append((name, args)) or {"mlp_wgrad_group_workspace": 77}.get(name, 0))
    call = mlp.WgradGroupCall.build([(torch.zeros(3, 8), False, [(torch.zeros(32, 3), torch.zeros(32, 8), None, None)])])
    assert call.workspace_floats() == 77 and call.n_launches() == 1          # (at least the one launch)
    (n0, a0), (n1, a1) = asked
    assert n0 == "mlp_wgrad_group_workspace" and len(a0) == len(lib.PROTOTYPES[n0][0])
    want = [call.n_src, call.A, call.lda, call.P, call.out_id, call.n_out, call.K, call.N, call.target_items, call.layout]
    assert all(x is y for x, y in zip(a0, want))
    assert n1 == "mlp_wgrad_group_launches" and len(a1) == len(lib.PROTOTYPES[n1][0])
    assert all(x is y for x, y in zip(a1, [call.n_src, call.P, call.out_id, call.n_out]))
    # the header's parameter lists of the two queries, in the order the record passes them
    with open(HEADER) as f:
        text = f.read()
    for name, fields in (("mlp_wgrad_group_workspace", ["n_src", "A", "lda", "P", "out_id", "n_out", "K", "N", "target_items", "layout"]),
                         ("mlp_wgrad_group_launches", ["n_src", "P", "out_id", "n_out"])):
        m = re.search(r"\b(?:int|long long) ndjir_%s\(([^;]*?)\);" % name, text, re.S)
        assert [re.search(r"(\w+)\s*$", p).group(1) for p in m.group(1).split(",")] == fields


def _is(got, want):
    return len(got) == len(want) and all(g is w for g, w in zip(got, want))


def test_merge_same_destination():
    buf = torch.zeros(8, 8)
    view = buf[:, :3]
    s0, s1, s2 = [(torch.zeros(32, 8), torch.zeros(32, 3), None, None) for _ in range(3)]
    merged = mlp._merge_same_destination([(view, True, [s0]), (buf[:, :3], True, [s1])])       # the same view twice, accumulating
    assert len(merged) == 1 and merged[0].out is view and merged[0].accum is True
    assert _is([s.A for s in merged[0].sources], [s0[0], s1[0]]) and all(isinstance(s, mlp.WgradSource) for s in merged[0].sources)
    jobs = [(view, True, [s0]), (view, False, [s1]), (view, True, [s2])]                       # overwritten in between: a job of its own
    merged = mlp._merge_same_destination(jobs)
    assert [j.accum for j in merged] == [True, False]
    assert _is([s.A for s in merged[0].sources], [s0[0], s2[0]]) and _is([s.A for s in merged[1].sources], [s1[0]])
    assert [len(j[2]) for j in jobs] == [1, 1, 1]                                              # (the callers' lists are left alone)
    rows, column = buf[:3], buf[:, :1]                                                         # overlapping, different views
    merged = mlp._merge_same_destination([(view, True, [s0]), (rows, True, [(torch.zeros(32, 3), torch.zeros(32, 8), None, None)]),
                                          (column, True, [(torch.zeros(32, 8), torch.zeros(32, 1), None, None)])])
    assert _is([j.out for j in merged], [view, rows, column]) and [len(j.sources) for j in merged] == [1, 1, 1]


def test_wgrad_jobs_of_a_split_target():
    A, B, ma, mb = torch.zeros(32, 4), torch.zeros(32, 3), torch.zeros(1), torch.zeros(1)
    top, bottom = torch.zeros(1, 3), torch.zeros(3, 3)
    jobs = mlp.wgrad_jobs(mlp.SplitTarget(top, bottom, 1), A, B, ma, mb)
    assert len(jobs) == 2 and all(isinstance(j, mlp.WgradJob) and j.accum is True and len(j.sources) == 1 for j in jobs)
    (s0,), (s1,) = jobs[0].sources, jobs[1].sources
    assert jobs[0].out is top and jobs[1].out is bottom and isinstance(s0, mlp.WgradSource) and isinstance(s1, mlp.WgradSource)
    assert tuple(s0.A.shape) == (32, 1) and s0.A.data_ptr() == A.data_ptr() and s0.A.stride(0) == 4
    assert tuple(s1.A.shape) == (32, 3) and s1.A.data_ptr() == A.data_ptr() + 4 and s1.A.stride() == (4, 1)
    assert s0.B is B and s1.B is B and s0.amax_a is ma and s1.amax_a is ma and s0.amax_b is mb and s1.amax_b is mb
    got = _got(jobs)[1]
    assert (got["lda"], got["ldb"], got["K"], got["N"], got["ldo"], got["out_id"]) == ([4, 4], [3, 3], [1, 3], [3, 3], [3, 3], [0, 1])
    (job,) = mlp.wgrad_jobs(bottom, A[:, 1:], B, None, mb)                  # a plain target: one job
    assert job.out is bottom and job.accum is True and len(job.sources) == 1
    assert job.sources[0].B is B and job.sources[0].amax_a is None and job.sources[0].amax_b is mb
