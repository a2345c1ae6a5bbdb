"""Weight-gradient kernels (ndjir_amd/csrc/wgrad.hip) against fp64, ELEMENT-WISE: every kind of work item of the grouped launch
x operand layout x point-count edge, columns spread over six decades, memory outside the destination, non-finite and all-zero
operands, run-to-run identity, more operand pairs than one device table holds, the per-layer kernel under every engine.

The statistic (one helper, `_stats` / `_judge`, used by every accuracy test).  ref = A64^T B64 (+ the destination's previous
value when the call accumulates), M_A / M_B = the maxima handed to the kernel (the largest finite magnitudes when none is
recorded),

    D_kn = (|A|^T |B|)_kn + 2^-17 (M_A sum_p |b_pn| + M_B sum_p |a_pk|) [+ |previous value|_kn],   rho(got) = max_kn |got - ref| / D_kn.

The second term is the per-tensor floor of the f16 split: x s is held to 2^-22 relative or 2^-39 of the scale's range
(csrc/wgrad.hip "the same tiles on the f16 matrix cores"; test_gpu_mlp.py::test_wgrad_one_outlier_row_elementwise), and with a
power-of-two scale 2^-21 D covers it.  The third term is this file's: an accumulating call ends in ONE more fp32 addition,
dst + sum, whose rounding is 2^-24 |dst + sum| <= 2^-24 (|dst| + D) -- the previous value is one more term of the sum.  The
previous values are drawn no larger than (|A|^T |B|)_kn, so D at most doubles and a defect of the product stays as visible.

    f16x3 (and bf16x6: loose for it, the exact three-way split delivers the strict figure)   rho <= 2^-21 + 4 rho32
    strict fp32, and the fp32 streaming items (kind 3) of the grouped launch                  rho <= 2^-23 + 4 rho32,  M_A = M_B = 0 in D

rho32 = the same statistic of the CPU float32 product `A.t() @ B` of the same inputs: measured on the reference, never on the
kernel.  2^-21 = two operands at 22 bits; the factor 4 = summation order (32-point MFMA chunks, split slabs, eight reduction
phases against BLAS's blocking; both are fp32 sums of the same P terms).

Every input is built on the CPU from a seeded RandomState; every test prints rho, rho32 and the bound per case."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ITEMS = 4096                 # explicit item target: the nominal split is the 512-point minimum, the wide-item rounding search is off
E_F16, E_STRICT = 2.0 ** -21, 2.0 ** -23
# (K, N) -> the kinds of work item that tile it (wgg_regions): 5 = 128 x 256, 0 = 128 x 128, 1 = 32 x 128, 4 = 64 x 128, 2 = 128 x 32
MFMA_SHAPES = [(128, 256), (100, 200),        # kind 5: full; ragged in both
               (128, 128), (100, 100),        # kind 0
               (5, 7), (133, 128),            # kind 1 (alone -- with a blocked A and a row-major B it streams, kind 3; under a 128 x 128 tile)
               (43, 128), (171, 40),          # kind 4 (alone; beside 128 x 32 strips)
               (128, 9), (128, 168)]          # kind 2 (alone; beside a tile)
NARROW_SHAPES = [(64, 3), (128, 8), (12, 1)]  # kind 3, row-major A: K % 4 == 0, 16-byte-aligned rows
NARROW_BLOCKED_A = [(43, 3)]                  # kind 3 with a point-blocked A: any K
P_ROW = [1, 31, 33, 64, 70, 1100, 1650]       # row-major pairs
P_BLK = [32, 64, 96, 1120, 1664]              # pairs with a point-blocked operand (whole 32-point blocks)


def _to_blocked(x):
    """(P, W) row-major -> the same P * W floats point-blocked: element (p, f) at ((p >> 5) * W + f) * 32 + (p & 31)."""
    P, W = x.shape
    return x.reshape(P // 32, 32, W).permute(0, 2, 1).contiguous().reshape(P, W)


def _finite(x):
    return np.where(np.isfinite(x), x, np.float32(0.0))


def _finite_max(x):
    return np.float32(np.abs(_finite(x)).max()) if x.size else np.float32(0.0)


def _pair(rng, P, K, N, lay, maxima, sa=1.0, sb=1.0):
    """One operand pair, on the CPU.  A is the feature range [4, 4 + K) of a (P, K + 8) buffer (row-major or point-blocked alike),
    B is (P, N).  maxima: "exact", "loose" (3 x) or "none"."""
    Aw = (rng.randn(P, K + 8) * sa).astype(np.float32)
    B = (rng.randn(P, N) * sb).astype(np.float32)
    return _finish_pair(dict(Aw=Aw, A=Aw[:, 4:4 + K], B=B, P=P, K=K, N=N, lay=lay, maxima=maxima))


def _finish_pair(p):
    f = np.float32(3.0) if p["maxima"] == "loose" else np.float32(1.0)
    p["MA"], p["MB"] = float(_finite_max(p["A"]) * f), float(_finite_max(p["B"]) * f)
    return p


def _streams(p):
    """Whether the pair takes the fp32 streaming path (wgg_narrow / the per-layer launcher's test): no operand scale, strict bound."""
    K, N, lay = p["K"], p["N"], p["lay"]
    if lay & 2:
        return False
    if lay & 1:
        return N <= 8
    return N <= 8 and K % 4 == 0 and p["Aw"].shape[1] % 4 == 0      # (the range starts 16 bytes into a fresh allocation)


def _upload(p, gpu):
    from ndjir_amd import mlp
    K = p["K"]
    Ad, Bd = torch.from_numpy(p["Aw"]).to(gpu), torch.from_numpy(p["B"]).to(gpu)
    a = mlp.PB(_to_blocked(Ad))[:, 4:4 + K] if p["lay"] & 1 else Ad[:, 4:4 + K]
    b = mlp.PB(_to_blocked(Bd)) if p["lay"] & 2 else Bd
    if p["maxima"] == "none":
        return (a, b, None, None)
    return (a, b, torch.tensor([p["MA"]], dtype=torch.float32, device=gpu), torch.tensor([p["MB"]], dtype=torch.float32, device=gpu))


def _abs_product(pairs):
    return sum(np.abs(_finite(p["A"]).astype(np.float64)).T @ np.abs(_finite(p["B"]).astype(np.float64)) for p in pairs)


def _stats(pairs, base=None, strict=False):
    """fp64 reference, D and rho32 of one output = sum over its operand pairs (+ base).  Non-finite entries count as 0: the
    callers only look at the entries they do not reach."""
    K, N = pairs[0]["K"], pairs[0]["N"]
    ref, D, f32 = np.zeros((K, N)), np.zeros((K, N)), torch.zeros(K, N)
    for p in pairs:
        A, B = np.ascontiguousarray(_finite(p["A"])), np.ascontiguousarray(_finite(p["B"]))
        aA, aB = np.abs(A.astype(np.float64)), np.abs(B.astype(np.float64))
        ref += A.astype(np.float64).T @ B.astype(np.float64)
        D += aA.T @ aB
        if not strict:
            D += 2.0 ** -17 * (p["MA"] * aB.sum(0)[None, :] + p["MB"] * aA.sum(0)[:, None])
        f32 = f32 + torch.from_numpy(A).t() @ torch.from_numpy(B)
    if base is not None:
        ref, D, f32 = ref + base.astype(np.float64), D + np.abs(base.astype(np.float64)), torch.from_numpy(base) + f32
    return ref, D, _ratio(f32.numpy().astype(np.float64) - ref, D)


def _ratio(err, D, keep=None):
    err = np.abs(err)
    r = np.divide(err, D, out=np.where(err > 0, np.inf, 0.0), where=D > 0)
    r = np.where(np.isnan(err), np.inf, r)
    return float(r.max() if keep is None else r[keep].max())


def _judge(got, ref, D, rho32, strict, keep=None):
    """(rho(got), bound) of one output; got: the destination back on the CPU"""
    return _ratio(got.astype(np.float64) - ref, D, keep), (E_STRICT if strict else E_F16) + 4.0 * rho32


def _report(title, rows):
    """rows: (case, rho, rho32, bound).  Prints every case, asserts every bound, returns the largest rho / bound."""
    print(f"\n{title}")
    for case, rho, rho32, bound in rows:
        print(f"  {case}: rho {rho:.2e}  rho32 {rho32:.2e}  bound {bound:.2e}  ratio {rho / bound:.3f}")
    worst = max(rho / bound for _, rho, _, bound in rows)
    print(f"  largest rho / bound: {worst:.3f}")
    bad = [(c, rho, bound) for c, rho, _, bound in rows if not rho <= bound]
    assert not bad, bad
    return worst


def _spec(rng, pairs, accum):
    """One output of a grouped call, on the CPU: operand pairs, accumulate or overwrite, the previous value of the destination
    (accumulate: random, no larger than the sum's own terms; overwrite: NaN)."""
    K, N = pairs[0]["K"], pairs[0]["N"]
    base = (rng.uniform(-1.0, 1.0, (K, N)) * _abs_product(pairs)).astype(np.float32) if accum else None
    strict = all(_streams(p) for p in pairs)
    ref, D, rho32 = _stats(pairs, base, strict)
    return dict(pairs=pairs, accum=accum, base=base, strict=strict, ref=ref, D=D, rho32=rho32,
                name=f"{K}x{N} " + "+".join(f"P{p['P']} lay{p['lay']} {p['maxima']}" for p in pairs) + (" accum" if accum else " write"))


def _run_specs(specs, gpu):
    """One grouped call over fresh destinations; returns them (device tensors)."""
    from ndjir_amd import mlp
    jobs = []
    for s in specs:
        K, N = s["pairs"][0]["K"], s["pairs"][0]["N"]
        out = torch.from_numpy(s["base"]).to(gpu) if s["accum"] else torch.full((K, N), float("nan"), device=gpu)
        jobs.append((out, s["accum"], [_upload(p, gpu) for p in s["pairs"]]))
    mlp.wgrad_group(jobs)
    return [j[0] for j in jobs]


def _judge_specs(title, specs, outs):
    rows = []
    for s, out in zip(specs, outs):
        rho, bound = _judge(out.cpu().numpy(), s["ref"], s["D"], s["rho32"], s["strict"])
        rows.append((s["name"], rho, s["rho32"], bound))
    return _report(title, rows)


_MIXED = {}


def _mixed_specs(lay, big_only):
    """The job list of one grouped call: every item kind at every point count, all pairs in layout `lay` (the streaming shapes:
    row-major A in the call of layout 0, point-blocked A in the call of layout 1 -- wgg_narrow allows no blocked B).  Accumulate
    and overwrite alternate; recorded maxima cycle through exact, 3 x loose and absent."""
    key = (lay, big_only)
    if key not in _MIXED:
        rng = np.random.RandomState(100 + lay)
        shapes = MFMA_SHAPES + (NARROW_SHAPES if lay == 0 else NARROW_SHAPES + NARROW_BLOCKED_A if lay == 1 else [])
        Ps = (P_ROW if lay == 0 else P_BLK)[-2 if big_only else 0:]
        specs = []
        for K, N in shapes:
            for P in Ps:
                i = len(specs)
                pair = _pair(rng, P, K, N, lay, ("exact", "loose", "none")[i % 3], sa=10.0 ** (i % 5 - 2), sb=2.0 + i % 4)
                specs.append(_spec(rng, [pair], accum=(i % 2 == 0)))
        _MIXED[key] = specs
    return _MIXED[key]


def _splits(P, K, N, lay, items):
    """Splits of the point axis of a single-pair grouped call, read from the library: its workspace is two tables + S slabs of
    K * N floats (rounded up to 4 floats); a call without operands is the two tables."""
    from ndjir_amd import lib
    L = lib.load()
    addr = (ctypes.c_void_p * 1)(1 << 20)           # (the planner looks at A's address only: 16-byte alignment, for the streaming path)
    need = int(L.ndjir_mlp_wgrad_group_workspace(1, addr, (ctypes.c_int * 1)(K + 8), (ctypes.c_longlong * 1)(P), (ctypes.c_int * 1)(0), 1,
                                                 (ctypes.c_int * 1)(K), (ctypes.c_int * 1)(N), items, (ctypes.c_int * 1)(lay)))
    empty = int(L.ndjir_mlp_wgrad_group_workspace(0, None, None, None, None, 0, None, None, items, None))
    assert need > empty
    return (need - empty) // (K * N)


def test_split_patterns_of_the_parametrisation(gpu):
    """The point counts of `test_every_item_kind_layout_and_chunk_pattern` reach every chunk pattern of the chunk loops: a split of
    ONE ragged chunk, splits of an even and of an odd number of 32-point chunks (wgrad3_pipe runs its chunks in pairs and
    multiplies a zero chunk past an odd end), three or more splits whose last is shorter and ragged.  The split COUNT is the
    library's (workspace sizes); the split length follows from it by the last line of wgg_split_plan, rows = P / S rounded up to
    whole chunks, and is checked for consistency (S splits of that length cover P, S - 1 do not)."""
    seen = set()
    for lay, Ps in ((0, P_ROW), (1, P_BLK), (2, P_BLK), (3, P_BLK)):
        for K, N in MFMA_SHAPES:
            for P in Ps:
                S = _splits(P, K, N, lay, ITEMS)
                if lay == 1 and N <= 8:          # (5 x 7 with a point-blocked A is a streaming output: 128 points per item)
                    assert S == -(-P // 128)
                    continue
                rows = -(-(-(-P // S)) // 32) * 32
                assert (S - 1) * rows < P <= S * rows, (P, K, N, S, rows)
                last = P - (S - 1) * rows
                if P in (1100, 1120):
                    assert (S, rows) == (3, 384), (P, K, N, lay, S, rows)
                if P in (1650, 1664):
                    assert (S, rows) == (4, 416), (P, K, N, lay, S, rows)
                for n in [rows] * (S - 1) + [last]:           # points of every split
                    chunks = -(-n // 32)
                    if chunks == 1 and n % 32 != 0:
                        seen.add("one ragged chunk")
                    seen.add("even" if chunks % 2 == 0 else "odd")
                if S >= 3 and last < rows and last % 32 != 0:
                    seen.add("short ragged last split")
    for P in P_ROW:           # streaming items: 128 points each
        assert _splits(P, 64, 3, 0, ITEMS) == -(-P // 128)
    for P in P_BLK:
        assert _splits(P, 43, 3, 1, ITEMS) == -(-P // 128)
    assert seen == {"one ragged chunk", "even", "odd", "short ragged last split"}, seen


@pytest.mark.parametrize("items", [ITEMS, 0])
@pytest.mark.parametrize("lay", [0, 1, 2, 3])
def test_every_item_kind_layout_and_chunk_pattern(gpu, lay, items, monkeypatch):
    """One grouped call per operand layout with every kind of work item (5 full and ragged in both, 0, 1, 4, 2, 3 -- the shapes
    at the top of the file) at every point count (row-major 1 ... 1650, point-blocked 32 ... 1664: see
    test_split_patterns_of_the_parametrisation), accumulate and overwrite (into NaN), recorded maxima exact / 3 x loose / absent
    (k_wgg_absmax), each output judged element-wise.  items = 0: the default target with the wide-item rounding search, at the
    two largest point counts.  Largest rho / bound measured on an MI355X: 0.651 (100 x 100 at P = 1: a single product, where 2^-21 is the split's own worst case; 0.21 from P = 31 on, 0.10 at items = 0)."""
    from ndjir_amd import mlp
    assert mlp.get_math() == mlp.MATH_F16X3
    monkeypatch.setattr(mlp, "WGRAD_GROUP_ITEMS", items)
    specs = _mixed_specs(lay, big_only=(items == 0))
    _judge_specs(f"item kinds x point counts, layout {lay}, items {items}", specs, _run_specs(specs, gpu))


@pytest.mark.parametrize("lay", [0, 3])
@pytest.mark.parametrize("P,K,N", [(1650, 171, 213), (2048, 256, 256)])
def test_columns_over_six_decades(gpu, P, K, N, lay, monkeypatch):
    """The column twin of test_wgrad_one_outlier_row_elementwise at a sixteenth of its size: the columns of A and of B are scaled
    by 10^(-6 u), so most of dW is made of columns 20 bits down their operand's range -- the per-element bound holds every entry
    to the documented floor, where a matrix norm sees the largest columns only.  (Point-blocked operands are whole 32-point
    blocks: layout 3 runs the first shape at P = 1664.)  Largest rho / bound measured on an MI355X: 0.076."""
    from ndjir_amd import mlp
    monkeypatch.setattr(mlp, "WGRAD_GROUP_ITEMS", ITEMS)
    if lay and P % 32:
        P = (P + 31) // 32 * 32
    rng = np.random.RandomState(P + lay)
    specs = []
    for maxima, accum in (("exact", False), ("none", True)):
        p = _pair(rng, P, K, N, lay, maxima)
        p["Aw"][:, 4:4 + K] *= (10.0 ** (-6.0 * rng.uniform(size=K))).astype(np.float32)[None, :]
        p["B"] *= (10.0 ** (-6.0 * rng.uniform(size=N))).astype(np.float32)[None, :]
        specs.append(_spec(rng, [_finish_pair(p)], accum))
    _judge_specs(f"columns over six decades {P}:{K}x{N} layout {lay}", specs, _run_specs(specs, gpu))


WINDOW_SHAPES = [(128, 256), (133, 128), (128, 9), (43, 128), (64, 3), (5, 7)]


def _window_cases(rng, P):
    """Destinations inside larger buffers, on the CPU: (buffer, mask of the window, view function, pair, accum)."""
    cases = []
    for K, N in WINDOW_SHAPES:
        for kind, off in [("window", c) for c in (0, 1, 3, 4)] + [("flat", o) for o in (0, 1, 2, 3)]:
            for accum in (False, True):
                pair = _pair(rng, P, K, N, 0, "exact")
                if kind == "window":        # rows [1, 1 + K), columns [off, off + N) of a (K + 2, N + 8) buffer: the 4-byte reduction
                    buf = rng.randn(K + 2, N + 8).astype(np.float32)
                    view = (lambda t, K=K, N=N, off=off: t[1:1 + K, off:off + N])
                else:                        # a contiguous (K, N) view `off` floats into a flat buffer, 8 sentinels on either side: the 16-byte one when K N % 4 == 0
                    buf = rng.randn(8 + 3 + K * N + 8).astype(np.float32)
                    view = (lambda t, K=K, N=N, off=off: t[8 + off:8 + off + K * N].reshape(K, N))
                mask = np.zeros(buf.shape, dtype=bool)
                view(mask)[...] = True
                view(buf)[...] = (rng.uniform(-1.0, 1.0, (K, N)) * _abs_product([pair])).astype(np.float32) if accum else np.float32("nan")
                cases.append(dict(buf=buf, mask=mask, view=view, pair=pair, accum=accum, name=f"{K}x{N} {kind} +{off} {'accum' if accum else 'write'}"))
    return cases


def _check_windows(title, cases, after):
    rows = []
    for c, got in zip(cases, after):
        got = got.cpu().numpy()
        outside = ~c["mask"]
        assert np.array_equal(got.view(np.int32)[outside], c["buf"].view(np.int32)[outside]), (c["name"], "memory outside the destination changed")
        strict = _streams(c["pair"])
        ref, D, rho32 = _stats([c["pair"]], np.ascontiguousarray(c["view"](c["buf"])) if c["accum"] else None, strict)
        rho, bound = _judge(np.ascontiguousarray(c["view"](got)), ref, D, rho32, strict)
        rows.append((c["name"], rho, rho32, bound))
    return _report(title, rows)


def test_nothing_outside_the_destination_is_written(gpu, monkeypatch):
    """Destinations in the product are windows of one flat gradient bucket.  Here: windows [1 : 1 + K, c0 : c0 + N] of a
    (K + 2, N + 8) buffer, c0 in {0, 1, 3, 4}, and contiguous (K, N) views at float offsets 0 .. 3 of a flat buffer with 8 sentinel
    floats on either side (both branches of wgg_out_vec: the 16-byte reduction store at every 4-byte alignment), per item kind,
    accumulate and overwrite, all in one grouped call.  Every float outside a window must keep its BITS; the window is judged
    like any other result.  Largest rho / bound measured on an MI355X: 0.149."""
    from ndjir_amd import mlp
    monkeypatch.setattr(mlp, "WGRAD_GROUP_ITEMS", ITEMS)
    cases = _window_cases(np.random.RandomState(31), 70)
    bufs = [torch.from_numpy(c["buf"]).to(gpu) for c in cases]
    mlp.wgrad_group([(c["view"](b), c["accum"], [_upload(c["pair"], gpu)]) for c, b in zip(cases, bufs)])
    _check_windows("windows of larger buffers, grouped call", cases, bufs)


def test_per_layer_kernel_writes_nothing_outside_its_destination(gpu):
    """The same for the per-layer kernel, `wgrad(out=...)`, on the contiguous windows of flat buffers (its reductions store 16 bytes
    at a time, too).  Largest rho / bound measured on an MI355X: 0.125."""
    from ndjir_amd import mlp
    cases = [c for c in _window_cases(np.random.RandomState(32), 70) if " flat " in c["name"]]
    bufs = []
    for c in cases:
        b = torch.from_numpy(c["buf"]).to(gpu)
        a, bb, ma, mb = _upload(c["pair"], gpu)
        mlp.wgrad(a, bb, out=c["view"](b), accum=c["accum"], amax_a=ma, amax_b=mb)
        bufs.append(b)
    _check_windows("windows of flat buffers, per-layer kernel", cases, bufs)


@pytest.mark.parametrize("recorded", [True, False])
def test_nonfinite_operands_reach_dw_and_only_where_they_should(gpu, recorded, monkeypatch):
    """The step's device-side veto (solver.check_inf_or_nan on the gradients) relies on a NaN / Inf in an activation or delta
    reaching dW -- through maxima that record the largest FINITE magnitude, the inline v_fma_mix* split and the fp32 streaming items
    alike.  A[5, 3] = NaN, A[70, 130 | 60] = +Inf, B[33, 35 | 1] = -Inf: rows 3 and 130 | 60 and column 35 | 1 of dW must be
    non-finite in EVERY entry, every other entry finite and within the bound (reference over the finite entries).  Row-major
    P = 100 and point-blocked P = 96; maxima recorded (finite) or found by k_wgg_absmax.  Largest rho / bound measured on an
    MI355X: 0.117."""
    from ndjir_amd import mlp
    monkeypatch.setattr(mlp, "WGRAD_GROUP_ITEMS", ITEMS)
    rng = np.random.RandomState(41)
    specs, marks = [], []
    for K, N in ((171, 40), (64, 3), (128, 128), (100, 200)):      # (the last two: the pipelined tiles, which multiply masked features and a chunk past the end by a scale of 0)
        for P, lay in ((100, 0), (96, 3 if N > 8 else 1)):
            p = _pair(rng, P, K, N, lay, "exact" if recorded else "none")
            ka, nb = (130 if K == 171 else 60), (35 if N >= 40 else 1)
            p["Aw"][5, 4 + 3], p["Aw"][70, 4 + ka], p["B"][33, nb] = np.float32("nan"), np.float32("inf"), np.float32("-inf")
            specs.append(_spec(rng, [_finish_pair(p)], accum=False))
            bad = np.zeros((K, N), dtype=bool)
            bad[3], bad[ka], bad[:, nb] = True, True, True
            marks.append(bad)
    outs = _run_specs(specs, gpu)
    rows = []
    for s, bad, out in zip(specs, marks, outs):
        got = out.cpu().numpy()
        assert not np.isfinite(got[bad]).any(), (s["name"], "finite entries where a NaN / Inf operand entry reaches", int(np.isfinite(got[bad]).sum()))
        assert np.isfinite(got[~bad]).all(), (s["name"], "non-finite entries a NaN / Inf operand entry does not reach", int((~np.isfinite(got[~bad])).sum()))
        rho, bound = _judge(got, s["ref"], s["D"], s["rho32"], s["strict"], keep=~bad)
        rows.append((s["name"], rho, s["rho32"], bound))
    _report(f"non-finite operand entries, maxima {'recorded' if recorded else 'found by the call'}", rows)


@pytest.mark.parametrize("recorded", [True, False])
def test_all_zero_operands(gpu, recorded, monkeypatch):
    """A == 0, B == 0, both: a zero maximum (recorded as 0.0, or left at 0 by k_wgg_absmax) takes the clamp of wg_scale_from_max
    (scale 2^126).  Overwriting gives exactly 0 everywhere, from NaN-filled memory; accumulating leaves the destination's bits as
    they are.  Item kinds 0, 1, 3 and 5; row-major P = 70 and point-blocked P = 1120."""
    from ndjir_amd import mlp
    monkeypatch.setattr(mlp, "WGRAD_GROUP_ITEMS", ITEMS)
    rng = np.random.RandomState(51)
    jobs, before = [], []
    for K, N in ((128, 128), (5, 7), (64, 3), (128, 256)):
        for P, lay in ((70, 0), (1120, 3 if N > 8 else 1)):
            for zero_a, zero_b in ((True, False), (False, True), (True, True)):
                for accum in (False, True):
                    p = _pair(rng, P, K, N, lay, "exact" if recorded else "none")
                    if zero_a:
                        p["Aw"][:, 4:4 + K] = 0.0          # (the rest of the wider buffer stays random: not the operand's)
                    if zero_b:
                        p["B"][...] = 0.0
                    _finish_pair(p)
                    assert (p["MA"] == 0.0) == zero_a and (p["MB"] == 0.0) == zero_b
                    out = torch.from_numpy(rng.randn(K, N).astype(np.float32)).to(gpu) if accum else torch.full((K, N), float("nan"), device=gpu)
                    jobs.append((out, accum, [_upload(p, gpu)]))
                    before.append(out.clone() if accum else torch.zeros_like(out))
    mlp.wgrad_group(jobs)
    for (out, accum, _), want in zip(jobs, before):
        if accum:
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (tuple(out.shape), "accumulating a zero product changed the destination")
        else:
            assert torch.equal(out, want), (tuple(out.shape), "a zero product is not exactly zero")


@pytest.mark.parametrize("lay", [0, 1, 2, 3])
def test_same_call_twice_is_bit_identical(gpu, lay, monkeypatch):
    """Slabs and reductions use no float atomics: the mixed job list of test_every_item_kind_layout_and_chunk_pattern, run twice
    into fresh destinations, gives the same bits."""
    from ndjir_amd import mlp
    monkeypatch.setattr(mlp, "WGRAD_GROUP_ITEMS", ITEMS)
    specs = _mixed_specs(lay, big_only=False)
    first, second = _run_specs(specs, gpu), _run_specs(specs, gpu)
    for s, a, b in zip(specs, first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), s["name"]


@pytest.mark.parametrize("n_out,per_out", [(200, 1), (100, 2)])
def test_more_sources_than_one_table_holds(gpu, n_out, per_out, monkeypatch):
    """200 operand pairs in one grouped call (the step has 66, the suite's largest call so far 46): wgg_chunk_end cuts at 192 sources
    (4 segments per source against WGT_MAX_SEG) and the call runs a SECOND table -- writer pieces, maxima pre-pass, item and
    reduction launches again, further into the workspace.  Every output is judged.  Largest rho / bound measured on an MI355X:
    0.156."""
    from ndjir_amd import lib, mlp
    monkeypatch.setattr(mlp, "WGRAD_GROUP_ITEMS", ITEMS)
    rng = np.random.RandomState(70 + per_out)
    shapes = [(32, 16), (43, 9), (64, 3), (128, 9), (5, 7)]
    specs = []
    for o in range(n_out):
        K, N = shapes[o % len(shapes)]
        pairs = [_pair(rng, (64, 70)[(o + j) % 2], K, N, 0, ("exact", "none", "loose")[(o + j) % 3], sb=1.0 + j) for j in range(per_out)]
        specs.append(_spec(rng, pairs, accum=(o % 2 == 1)))
    n = n_out * per_out
    Ps = (ctypes.c_longlong * n)(*[p["P"] for s in specs for p in s["pairs"]])
    oid = (ctypes.c_int * n)(*[o for o, s in enumerate(specs) for _ in s["pairs"]])
    assert int(lib.load().ndjir_mlp_wgrad_group_launches(n, Ps, oid, n_out)) == 2
    _judge_specs(f"{n_out} outputs x {per_out} operand pairs: two tables", specs, _run_specs(specs, gpu))


def test_reduce_only_call_sums_deferred_bias_partials(gpu, monkeypatch):
    """A grouped call without jobs (what `deferred_wgrads` ends in when only bias gradients were deferred): two bias destinations
    of 8 and 3 floats, three partial rows each in one region of row stride 12, ADDED to non-zero destinations -- against the fp64
    sum, to the tolerance of test_gpu_mlp.py::test_colsum_kernel.  Eagerly, then under a graph capture."""
    from ndjir_amd import mlp
    rng = np.random.RandomState(81)
    region = rng.randn(3, 12).astype(np.float32)
    prev = [rng.randn(8).astype(np.float32), rng.randn(3).astype(np.float32)]
    ref = [prev[0].astype(np.float64) + region[:, :8].astype(np.float64).sum(0), prev[1].astype(np.float64) + region[:, 8:11].astype(np.float64).sum(0)]
    part, dst = torch.from_numpy(region).to(gpu).view(-1), [torch.from_numpy(p.copy()).to(gpu) for p in prev]
    mlp._wgrad_group_now([], [mlp.BiasPartial(dst[0], part, 8, 3, 12), mlp.BiasPartial(dst[1], part[8:], 3, 3, 12)])
    torch.cuda.synchronize()
    for got, want in zip(dst, ref):
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max()) / max(float(np.abs(want).max()), 1.0)
        print(f"\nreduce-only call, {want.size} floats: error / scale {err:.2e}")
        assert err < 2e-5
    assert torch.equal(part.cpu(), torch.from_numpy(region).view(-1))          # (the partial rows are only read)
    # ... and captured into a graph on a stream that has no workspace yet: the capture gets a one-off of its own and nothing is cached
    # for later launches to share (`hold_buffers`); every replay adds the three rows once more
    monkeypatch.setattr(mlp, "_WORKSPACE_G", {})
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mlp._wgrad_group_now([], [mlp.BiasPartial(dst[0], part, 8, 3, 12), mlp.BiasPartial(dst[1], part[8:], 3, 3, 12)])
    assert mlp._WORKSPACE_G == {}
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for got, want, p in zip(dst, ref, prev):
        want = 3.0 * want - 2.0 * p.astype(np.float64)
        assert float(np.abs(got.cpu().numpy().astype(np.float64) - want).max()) / max(float(np.abs(want).max()), 1.0) < 2e-5


def test_one_output_with_more_pairs_than_a_table_is_refused(gpu):
    """193 operand pairs of ONE output fit no table (4 x 193 segments > 768): the library's error, before any launch -- the
    destination keeps its bits."""
    from ndjir_amd import lib, mlp
    rng = np.random.RandomState(77)
    src = _upload(_pair(rng, 64, 5, 7, 0, "exact"), gpu)
    out = torch.from_numpy(rng.randn(5, 7).astype(np.float32)).to(gpu)
    before = out.clone()
    with pytest.raises(lib.NdjirHipError):
        mlp.wgrad_group([(out, True, [src] * 193)])
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), before.view(torch.int32))
    mlp.wgrad_group([(out, True, [src] * 192)])          # (the limit itself runs)
    torch.cuda.synchronize()
    assert not torch.equal(out, before)


def test_blocked_layout_needs_whole_blocks_at_the_c_abi(gpu):
    """include/ndjir_hip.h is a drop-in boundary: a layout bit on an operand whose point count is no multiple of 32 (k_wgg_absmax
    and the blocked loaders read every 32-point block to its end) is NDJIR_ERR_ARG from ndjir_mlp_wgrad_group itself (the check
    sits in the entry point, csrc/capi_mlp.hip, in front of the launcher), not only an assertion of the Python wrapper -- before
    any launch, destination untouched."""
    from ndjir_amd import lib
    f, sig = lib._fn("mlp_wgrad_group")
    rng = np.random.RandomState(78)
    P, K, N = 70, 64, 16
    A = torch.from_numpy(rng.randn(96, K).astype(np.float32)).to(gpu)         # (allocated to the end of the last block)
    B = torch.from_numpy(rng.randn(96, N).astype(np.float32)).to(gpu)
    out = torch.from_numpy(rng.randn(K, N).astype(np.float32)).to(gpu)
    ws = torch.empty(1 << 22, device=gpu)
    before = out.clone()
    vp, ci = ctypes.c_void_p, ctypes.c_int

    def call(P, lay):
        return f(1, (vp * 1)(A.data_ptr()), (ci * 1)(K), (vp * 1)(B.data_ptr()), (ci * 1)(N), (ctypes.c_longlong * 1)(P), None, None,
                 (ci * 1)(0), 1, (vp * 1)(out.data_ptr()), (ci * 1)(N), (ci * 1)(K), (ci * 1)(N), (ci * 1)(1), ws.data_ptr(), 0,
                 0, None, None, None, None, None, None, (ci * 1)(lay), torch.cuda.current_stream().cuda_stream)
    for lay in (1, 2, 3):
        assert call(P, lay) == 3          # NDJIR_ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), before.view(torch.int32))
    assert call(96, 3) == 0 and call(P, 0) == 0          # whole blocks, and row-major operands of any length, run
    torch.cuda.synchronize()
    assert not torch.equal(out, before)


ENGINE_SHAPES = [(1, 5, 7), (33, 5, 7), (100, 128, 9), (777, 52, 40), (1000, 301, 128), (2000, 128, 192), (1000, 64, 3)]


@pytest.mark.parametrize("engine", ["FP32", "F16X3", "BF16X6"])
def test_per_layer_kernel_under_every_engine(gpu, engine):
    """`wgrad` on strided operand views (as test_gpu_mlp.py::test_wgrad_kernel) under the strict-fp32 k_wgrad -- the leg bench.py
    reports as fp32_engine --, the f16x3 k_wgrad3 with its own maxima pass (k_absmax2) and the bf16x6 k_wgrad6, element-wise with
    the engine's bound (bf16x6 is held to the f16x3 bound: loose for it).  Largest rho / bound measured on an MI355X:
    0.151 (fp32), 0.499 (f16x3, 5 x 7 at P = 1), 0.098 (bf16x6)."""
    from ndjir_amd import mlp
    math = getattr(mlp, "MATH_" + engine)
    rng = np.random.RandomState(81)
    pairs = []
    for P, K, N in ENGINE_SHAPES:
        Aw = rng.randn(P, K + 3).astype(np.float32)
        Bw = rng.randn(P, N + 5).astype(np.float32)
        pairs.append(_finish_pair(dict(Aw=Aw, Bw=Bw, A=Aw[:, :K], B=Bw[:, 2:2 + N], P=P, K=K, N=N, lay=0, maxima="none")))
    old = mlp.get_math()
    mlp.set_math(math)
    try:
        outs = [mlp.wgrad(torch.from_numpy(p["Aw"]).to(gpu)[:, :p["K"]], torch.from_numpy(p["Bw"]).to(gpu)[:, 2:2 + p["N"]]).cpu().numpy()
                for p in pairs]
    finally:
        mlp.set_math(old)
    rows = []
    for p, got in zip(pairs, outs):
        strict = engine == "FP32"
        ref, D, rho32 = _stats([p], None, strict)
        rho, bound = _judge(got, ref, D, rho32, strict)
        rows.append((f"{p['P']}:{p['K']}x{p['N']}", rho, rho32, bound))
    _report(f"per-layer kernel, engine {engine}", rows)


_ORDER_CHILD = r'''
import os, sys
sys.path.insert(0, os.getcwd())
import numpy as np, torch
from ndjir_amd import mlp
rng, dev = np.random.RandomState(91), torch.device("cuda:0")
jobs, refs = [], []
for K, N in ((64, 3), (5, 7), (128, 128), (128, 256)):          # kinds 3, 1, 0, 5
    A, B = rng.randn(70, K).astype(np.float32), rng.randn(70, N).astype(np.float32)
    refs.append(A.astype(np.float64).T @ B.astype(np.float64))
    jobs.append((torch.full((K, N), float("nan"), device=dev), False, [(torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev), None, None)]))
mlp.wgrad_group(jobs)
print("ORDER_CHILD", max(float(np.abs(j[0].cpu().numpy() - r).max() / np.abs(r).max()) for j, r in zip(jobs, refs)))
'''


def test_item_order_switch_is_ignored_unless_a_permutation(gpu):
    """NDJIR_WGG_ORDER (the A/B switch for the order in which a grouped call issues its item kinds) is read once per process: a
    value that is no permutation of 0..5 -- here 550412, kind 3 missing -- used to leave the missing kind's items unissued and
    their slabs unwritten.  It is ignored now: a fresh process with that value computes every output."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _ORDER_CHILD], cwd=root, env=dict(os.environ, NDJIR_WGG_ORDER="550412"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    err = float([line for line in r.stdout.splitlines() if line.startswith("ORDER_CHILD")][-1].split()[1])
    assert err < 1e-5, err          # (every kind issued -- accuracy is the other tests' business; NaN = an output nobody wrote)
