"""The small kernels that every step runs around the fused chains -- csrc/geo.hip, the positional encoding and the background
head of csrc/render.hip, csrc/loss.hip -- against the fp64 references of tests/tail_ref.py, element by element:

* at "wrapping" shapes (tail_ref.WRAP_SHAPES): more than 2.5 x 2^21 elements, so that every thread of the capped launch takes
  three passes and `RowCol::next()` its carry, with the row width no divisor of 2^21 and the output rows wider than the row;
* at small sizes over every switch: segment counts, band counts, absent tensors, strides, argument errors;
* the per-ray kernels past one block and one loop pass, with signed inputs, real-valued masks, zero weights, non-finite inputs
  of switched-off terms.

Bounds (u = 2^-24), each per element: copies exact; cos / sin 2e-6 absolute at |x 2^k| <= 2^10; g-bar_0 one rounded product,
2 u |ref| + 2^-126; sums of T terms (T + 2) u sum|terms| -- T counts every added term, each a product rounded once (a power of
two is exact) and added with at most T - 1 roundings, so T u to first order and 2 u for the higher orders; backward-begin
bit-equal to the fp32 addition; the remaining kernels keep the tolerance of their earlier test (2e-6, 2e-5, 1e-6, 1e-5, 2e-5),
now relative to the element's own magnitude -- where the element is a sum that cancels, to its sum|terms| -- with the earlier
test's absolute floor.  Every check prints `RATIO <kernel> <largest error / bound>`; the docstrings quote the MI355X figures."""
import numpy as np
import pytest
import torch

from tests import tail_ref as TR

pytestmark = pytest.mark.gpu
NAN = float("nan")
INF = float("inf")


def _ratio(name, got, ref, bound):
    """max over the elements of |got - ref| / bound (0 / 0 = 0; a NaN or an error at bound 0 = inf), printed and returned."""
    got = TR.d(got).reshape(ref.shape)
    bound = bound if torch.is_tensor(bound) else torch.full_like(ref, float(bound))
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = float(torch.nan_to_num(r, nan=INF).max()) if r.numel() else 0.0
    print(f"RATIO {name} {r:.3g}")
    return r


def _within(name, got, ref, bound):
    r = _ratio(name, got, ref, bound)
    assert r <= 1.0, (name, r)


def _gen(gpu, seed):
    return torch.Generator(device=gpu).manual_seed(seed)


def _nan_rows(P, ld, gpu):
    return torch.full((P, ld), NAN, device=gpu)


def _guarded(n, gpu, guard=64):
    """A flat NaN buffer of n floats between two guards of NaN: (whole buffer, the n floats)."""
    buf = torch.full((n + 2 * guard,), NAN, device=gpu)
    return buf, buf[guard:guard + n]


def _guards_untouched(buf, n, guard=64):
    return bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all())


# ---- wrapping shapes -------------------------------------------------------------------------------------------------------------
def _check_encode(gpu, P, M, seg_widths, lde, seed, tag):
    from ndjir_amd import lib
    gen = _gen(gpu, seed)
    x = (torch.randn(P, 3, device=gpu, generator=gen) * 0.5).clamp(-2.0, 2.0)               # |x 2^k| <= 2^10 up to M = 10
    segs = [torch.randn(P, C, device=gpu, generator=gen) for C in seg_widths]
    W = 3 + 6 * M + sum(seg_widths)
    e = _nan_rows(P, lde, gpu)
    lib.call("geo_encode", P, M, x, len(segs), segs, list(seg_widths), e, lde)
    npe = 3 + 6 * M
    assert torch.equal(e[:, :3], x)
    assert torch.equal(e[:, npe:W], torch.cat(segs, dim=-1) if segs else e[:, npe:W])
    assert bool(torch.isnan(e[:, W:]).all())
    ref = TR.encode(x, M, segs)
    _within(f"geo_encode[{tag}]", e[:, 3:npe], ref[:, 3:npe], 2e-6)
    return x, segs, e


def _check_gbar0(gpu, P, M, seg_widths, lde, seed, tag):
    from ndjir_amd import lib
    gen = _gen(gpu, seed)
    e = torch.randn(P, lde, device=gpu, generator=gen)
    nbar = torch.randn(P, 3, device=gpu, generator=gen)
    nbar[0] = 0.0
    segs = [torch.randn(P, C, device=gpu, generator=gen) for C in seg_widths]
    W = 3 + 6 * M + sum(seg_widths)
    buf, flat = _guarded(P * W, gpu)
    lib.call("geo_gbar0", P, M, e, lde, nbar, len(segs), segs, list(seg_widths), flat)
    gb = flat.view(P, W)
    npe = 3 + 6 * M
    assert _guards_untouched(buf, P * W)
    assert torch.equal(gb[:, :3], nbar)
    assert torch.equal(gb[:, npe:], torch.cat(segs, dim=-1) if segs else gb[:, npe:])
    ref = TR.gbar0(e, nbar, M, segs)
    _within(f"geo_gbar0[{tag}]", gb[:, 3:npe], ref[:, 3:npe], 2 * TR.U * ref[:, 3:npe].abs() + TR.FLT_MIN)


def test_wrap_geo_encode(gpu):
    """120 001 x 49 (W odd, lde = 52): 3 passes, dr = 2^21 mod 49 = 1.  MI355X: cos / sin 0.035 of 2e-6."""
    s = TR.WRAP_SHAPES["geo_encode"]
    _check_encode(gpu, s["P"], s["M"], s["segs"], s["lde"], 1, "wrap")


def test_wrap_geo_gbar0(gpu):
    """120 001 x 49 read from rows of 52.  MI355X: 0.5 of 2 u |ref| (one rounded product: half an ulp)."""
    s = TR.WRAP_SHAPES["geo_gbar0"]
    _check_gbar0(gpu, s["P"], s["M"], s["segs"], s["lde"], 2, "wrap")


def _check_backward_begin(gpu, P, D, ldf, ldz, seed, g_sdf=True, g_feat=True, g_n=True, gZ=True, nbar=True):
    from ndjir_amd import lib
    from ndjir_amd.mlp import _Strided
    gen = _gen(gpu, seed)
    r = lambda *s: torch.randn(*s, device=gpu, generator=gen)
    a_sdf = r(P) if g_sdf else None
    a_feat = r(P, ldf) if g_feat else None
    a_n = r(P, 3) if g_n else None
    a_Z = r(P, ldz) if gZ else None
    bgy, gy = _guarded(P * (1 + D), gpu)
    bnb, nb = _guarded(P * 3, gpu)
    lib.call("geo_backward_begin", P, D, a_sdf, None if a_feat is None else _Strided(a_feat[:, :D]), ldf, a_n, a_Z, ldz, gy,
             nb if nbar else None)
    assert _guards_untouched(bgy, P * (1 + D)) and _guards_untouched(bnb, P * 3)
    gy, nb = gy.view(P, 1 + D), nb.view(P, 3)
    z = lambda *s: torch.zeros(*s, device=gpu)
    # bit-equal to the fp32 addition (one rounding: within u |ref| of the fp64 sum, checked below as well)
    assert torch.equal(gy[:, 0], a_sdf if g_sdf else z(P))
    assert torch.equal(gy[:, 1:], (a_feat[:, :D] if g_feat else z(P, D)) + (a_Z[:, 3:3 + D] if gZ else z(P, D)))
    ref_gy, ref_nb = TR.backward_begin(P, D, a_sdf, a_feat, a_n, a_Z)
    _within(f"geo_backward_begin[D={D}]", gy, ref_gy, TR.U * ref_gy.abs())
    if nbar:
        assert torch.equal(nb, (a_n if g_n else z(P, 3)) + (a_Z[:, 3 + D:6 + D] if gZ else z(P, 3)))
        _within(f"geo_backward_begin[D={D}] nbar", nb, ref_nb, TR.U * ref_nb.abs())
    else:
        assert bool(torch.isnan(nb).all())


def test_wrap_geo_backward_begin_scalar(gpu):
    """D = 7: 500 003 x 11 items, strided g_feat (9) and gZ (16).  MI355X: bit-equal to the fp32 addition; 1.0 of u |ref| (half an ulp just above a power of two)."""
    s = TR.WRAP_SHAPES["geo_backward_begin"]
    _check_backward_begin(gpu, s["P"], s["D"], s["ldf"], s["ldz"], 3)


def test_wrap_geo_backward_begin_v4(gpu):
    """D = 20: 600 001 x 9 items (5 vectors of 16 bytes at 4-byte alignment, the sdf column, three of n-bar), g_feat in rows of 21, gZ in rows of 26.
    MI355X: bit-equal to the fp32 addition; 1.0 of u |ref|."""
    s = TR.WRAP_SHAPES["geo_backward_begin_v4"]
    _check_backward_begin(gpu, s["P"], s["D"], s["ldf"], s["ldz"], 4)


def test_wrap_copy_columns(gpu):
    """1 100 003 x 5 out of rows of 7 into rows of 6: exact, the sixth column stays NaN."""
    from ndjir_amd import lib
    s = TR.WRAP_SHAPES["copy_columns"]
    P, C = s["P"], s["W"]
    src = torch.randn(P, s["lds"], device=gpu, generator=_gen(gpu, 5))
    dst = _nan_rows(P, s["ldd"], gpu)
    lib.call("copy_columns", P, C, src, s["lds"], dst, s["ldd"])
    assert torch.equal(dst[:, :C], src[:, :C]) and bool(torch.isnan(dst[:, C:]).all())


def test_wrap_positional_encoding(gpu):
    """140 001 x 39 through `_PosEnc`.  MI355X: cos / sin 0.035 of 2e-6."""
    from ndjir_amd.network import _PosEnc
    s = TR.WRAP_SHAPES["posenc"]
    P, C, M = s["P"], s["C"], s["M"]
    x = (torch.randn(P, C, device=gpu, generator=_gen(gpu, 6)) * 0.7).clamp(-30.0, 30.0)
    out = _PosEnc.apply(x, M, True)
    assert out.shape == (P, s["W"]) and torch.equal(out[:, :C], x)
    _within("posenc[wrap]", out[:, C:], TR.posenc(x, M, True)[:, C:], 2e-6)


def test_wrap_positional_encoding_backward(gpu):
    """1 750 001 x 3 elements, each a sum of T = 3 terms (M = 1, the input's own column) read from rows of 9.
    MI355X: 0.64 of 5 u sum|terms| (the bound leaves no room for sinf / cosf's own error; it is not needed)."""
    from ndjir_amd.network import _PosEnc
    s = TR.WRAP_SHAPES["posenc_backward"]
    P, C, M = s["P"], s["C"], s["M"]
    gen = _gen(gpu, 7)
    x = (torch.randn(P, C, device=gpu, generator=gen) * 0.7).requires_grad_(True)
    g = torch.randn(P, C + 2 * C * M, device=gpu, generator=gen)
    (gx,) = torch.autograd.grad(_PosEnc.apply(x, M, True), x, g)
    ref, mag, T = TR.posenc_backward(x, g, M, True)
    assert T == 3
    _within("posenc_backward[wrap]", gx, ref, (T + 2) * TR.U * mag)


def _bg_inputs(gpu, P, nx, F, seed):
    gen = _gen(gpu, seed)
    h = torch.randn(P, 1 + F, device=gpu, generator=gen) * 0.05
    h[::7, 0] = 0.5                                              # softplus' linear branch among the others
    x = torch.randn(P, nx, device=gpu, generator=gen)
    delta = torch.rand(P, 1, device=gpu, generator=gen) * 3
    return h, x, delta, gen


def test_wrap_background_head(gpu):
    """21 001 x 259.  The lighting net's input is a copy; alpha within 2e-6 max(|ref|, 1).  MI355X: 0.034."""
    from ndjir_amd.volume import background_head
    s = TR.WRAP_SHAPES["background_head"]
    h, x, delta, _ = _bg_inputs(gpu, s["P"], s["nx"], s["F"], 8)
    alpha, inp = background_head(h, x, delta)
    ra, ri = TR.background_head(h, x, delta)
    assert torch.equal(inp, torch.cat([x, h[:, 1:]], dim=-1)) and torch.equal(TR.d(inp), ri)
    _within("background_head[wrap] alpha", alpha, ra, 2e-6 * ra.abs().clamp(min=1.0))


def test_wrap_background_head_backward(gpu):
    """21 001 x 257: the feature columns are a copy of g_inp's, column 0 within 2e-5 |ref| + 2^-126.  MI355X: 0.044."""
    from ndjir_amd.volume import background_head
    s = TR.WRAP_SHAPES["background_head_backward"]
    h, x, delta, gen = _bg_inputs(gpu, s["P"], s["nx"], s["F"], 9)
    h.requires_grad_(True)
    alpha, inp = background_head(h, x, delta)
    ga, gi = torch.randn(alpha.shape, device=gpu, generator=gen), torch.randn(inp.shape, device=gpu, generator=gen)
    (gh,) = torch.autograd.grad([alpha, inp], h, [ga, gi])
    ref = TR.background_head_backward(h, delta, ga, gi, s["nx"])
    assert torch.equal(gh[:, 1:], gi[:, s["nx"]:])
    _within("background_head_backward[wrap]", gh[:, 0], ref[:, 0], 2e-5 * ref[:, 0].abs() + TR.FLT_MIN)


def _check_normal(gpu, P, M, nseg, lde, D, ldz, seed, use_n=True, use_Z=True, tag="", ldg=None):
    from ndjir_amd import lib
    gen = _gen(gpu, seed)
    r = lambda *s: torch.randn(*s, device=gpu, generator=gen)
    ldg = lde + 1 if ldg is None else ldg
    e, g0 = r(P, lde), r(P, ldg)
    gqs = [r(P, 3) for _ in range(nseg)]
    bn, n = _guarded(P * 3, gpu)
    Z0 = r(P, ldz) if use_Z else None
    Z = Z0.clone() if use_Z else None
    bs, sdf = _guarded(P, gpu)
    lib.call("geo_normal", P, M, e, lde, g0, ldg, nseg, gqs, n if use_n else None, Z, ldz, D, sdf if use_Z else None)
    ref, mag, T = TR.normal_from_g0(e, g0, M, gqs)
    assert T == 1 + 2 * M + nseg
    bound = (T + 2) * TR.U * mag
    assert _guards_untouched(bn, P * 3) and _guards_untouched(bs, P)
    if use_n:
        _within(f"geo_normal[{tag}] n_out", n.view(P, 3), ref, bound)
    else:
        assert bool(torch.isnan(n).all())
    if use_Z:
        assert torch.equal(sdf, Z0[:, 2]), "sdf_out is what the forward chain left in column 2"
        assert torch.equal(Z[:, :3], e[:, :3]) and torch.equal(Z[:, 3:3 + D], Z0[:, 3:3 + D])
        assert float(Z[:, 6 + D:].abs().max()) == 0.0 if ldz > 6 + D else True
        _within(f"geo_normal[{tag}] Z", Z[:, 3 + D:6 + D], ref, bound)
        if use_n:
            assert torch.equal(Z[:, 3 + D:6 + D], n.view(P, 3))
    else:
        assert bool(torch.isnan(sdf).all())


def test_wrap_geo_normal(gpu):
    """1 750 001 x 3 elements (t / 3, no RowCol), M = 1 and one extra term: T = 4; n_out and Z = [x | n | 0] in rows of 7.
    MI355X: 0.48 of 6 u sum|terms|."""
    s = TR.WRAP_SHAPES["geo_normal"]
    _check_normal(gpu, s["P"], s["M"], 1, s["lde"], s["D"], s["ldz"], 10, tag="wrap", ldg=s["lde"])


def test_wrap_inverse_squared_distance(gpu):
    """5 300 001 rows in batches of 1 000 003 (the last one short), into column 0 of rows of 2.  1e-5 relative.  MI355X: 0.041."""
    from ndjir_amd import lib
    s = TR.WRAP_SHAPES["inverse_squared_distance"]
    P, rows = s["P"], s["rows_per_batch"]
    gen = _gen(gpu, 11)
    x = torch.randn(P, s["ldx"], device=gpu, generator=gen)
    cam = torch.randn((P + rows - 1) // rows, 3, device=gpu, generator=gen)
    out = _nan_rows(P, s["ldo"], gpu)
    lib.call("inverse_squared_distance", P, rows, x, s["ldx"], cam, out, s["ldo"])
    ref = TR.inverse_squared_distance(x, cam, rows)
    assert bool(torch.isnan(out[:, 1:]).all())
    _within("inverse_squared_distance[wrap]", out[:, 0], ref, 1e-5 * ref.abs())


# ---- geo.hip at small P -----------------------------------------------------------------------------------------------------------
SEGS = {0: (), 1: (5,), 4: (4, 1, 7, 3)}


@pytest.mark.parametrize("M", [0, 1, 6, 10])
@pytest.mark.parametrize("nseg", [0, 1, 4])
def test_geo_encode_and_gbar0_small(gpu, nseg, M):
    """P = 301 over the segment and band counts, rows of W and of W + 3.  MI355X: cos / sin <= 0.031 of 2e-6, g-bar_0 <= 0.499 of 2 u |ref|."""
    W = 3 + 6 * M + sum(SEGS[nseg])
    for lde in (W, W + 3):
        _check_encode(gpu, 301, M, SEGS[nseg], lde, 20 + M, f"nseg={nseg},M={M}")
        _check_gbar0(gpu, 301, M, SEGS[nseg], lde, 30 + M, f"nseg={nseg},M={M}")


@pytest.mark.parametrize("M", [0, 1, 6, 10])
@pytest.mark.parametrize("nseg", [0, 4])
def test_geo_normal_small(gpu, nseg, M):
    """P = 301: Z only, n_out only, both; ldz = 6 + D and 6 + D + 5; spare columns zero, feature columns untouched, sdf_out
    bit-equal to column 2.  MI355X: <= 0.36 of (T + 2) u sum|terms|."""
    D, lde = 16, 3 + 6 * M + 2
    for ldz in (6 + D, 6 + D + 5):
        _check_normal(gpu, 301, M, nseg, lde, D, ldz, 40 + M, True, True, f"nseg={nseg},M={M}")
        _check_normal(gpu, 301, M, nseg, lde, D, ldz, 41 + M, False, True, f"nseg={nseg},M={M}")
    _check_normal(gpu, 301, M, nseg, lde, D, 6 + D, 42 + M, True, False, f"nseg={nseg},M={M}")


@pytest.mark.parametrize("D", [0, 7, 16])
def test_geo_backward_begin_small(gpu, D):
    """P = 301, both kernels and D = 0: everything given, then each tensor absent on its own.  MI355X: bit-equal to the fp32
    addition; 1.0 of u |ref|."""
    ldf, ldz = D + 2, 6 + D + 3
    _check_backward_begin(gpu, 301, D, ldf, ldz, 50)
    for k, absent in enumerate(("g_sdf", "g_feat", "g_n", "gZ", "nbar")):
        _check_backward_begin(gpu, 301, D, ldf, ldz, 51 + k, **{absent: False})


def test_geo_argument_errors_are_returned(gpu):
    """A bad argument is a status, not a launch: nothing is written."""
    from ndjir_amd import lib
    P, M = 16, 2
    x = torch.randn(P, 3, device=gpu)
    segs = [torch.randn(P, 2, device=gpu) for _ in range(5)]
    W = 3 + 6 * M + 2
    e = _nan_rows(P, 64, gpu)
    with pytest.raises(lib.NdjirHipError):
        lib.call("geo_encode", P, M, x, 5, segs, [2] * 5, e, 64)
    with pytest.raises(lib.NdjirHipError):
        lib.call("geo_encode", P, 31, x, 0, [], [], _nan_rows(P, 3 + 6 * 31, gpu), 3 + 6 * 31)
    with pytest.raises(lib.NdjirHipError):
        lib.call("geo_encode", P, M, x, 1, segs[:1], [2], e, W - 1)
    assert bool(torch.isnan(e).all())
    D = 4
    ev, g0, Z, n, sdf = torch.randn(P, 15, device=gpu), torch.randn(P, 15, device=gpu), _nan_rows(P, 6 + D, gpu), _nan_rows(P, 3, gpu), _nan_rows(P, 1, gpu)
    with pytest.raises(lib.NdjirHipError):
        lib.call("geo_normal", P, M, ev, 15, g0, 15, 0, [], n, Z, 6 + D - 1, D, sdf)
    assert bool(torch.isnan(Z).all()) and bool(torch.isnan(n).all()) and bool(torch.isnan(sdf).all())
    gy = _nan_rows(P, 1 + D, gpu)
    with pytest.raises(lib.NdjirHipError):
        lib.call("geo_backward_begin", P, D, None, torch.randn(P, D, device=gpu), D - 1, None, None, 0, gy, None)
    assert bool(torch.isnan(gy).all())
    dst = _nan_rows(P, 8, gpu)
    with pytest.raises(lib.NdjirHipError):
        lib.call("copy_columns", P, 5, torch.randn(P, 8, device=gpu), 4, dst, 8)
    assert bool(torch.isnan(dst).all())


# ---- background head edges -------------------------------------------------------------------------------------------------------
def test_background_head_edges(gpu):
    """100 h_0 on either side of softplus' threshold 20 (by one fp32 step and by 1e-3), h_0 = -1 (exp underflows), h_0 = 0,
    delta = 0; backward with g_alpha alone, g_inp alone, both.  MI355X: alpha 0.013 of 2e-6, gradient 0.004 of 2e-5."""
    from ndjir_amd import lib
    from ndjir_amd.volume import background_head
    nx, F = 3, 5
    lo, hi = np.nextafter(np.float32(0.2), np.float32(0)), np.nextafter(np.float32(0.2), np.float32(1))
    h0 = [0.199, float(lo), 0.2, float(hi), 0.201, -1.0, 0.0, 0.05, 0.5]
    P = len(h0)
    gen = _gen(gpu, 60)
    h = torch.randn(P, 1 + F, device=gpu, generator=gen)
    h[:, 0] = torch.tensor(h0, device=gpu)
    x = torch.randn(P, nx, device=gpu, generator=gen)
    delta = torch.rand(P, 1, device=gpu, generator=gen) * 3 + 0.5
    delta[7] = 0.0
    alpha, inp = background_head(h, x, delta)
    ra, ri = TR.background_head(h, x, delta)
    assert torch.equal(TR.d(inp), ri)
    assert float(alpha[7]) == 0.0 and float(alpha[5]) == 0.0
    _within("background_head[edges] alpha", alpha, ra, 2e-6 * ra.abs().clamp(min=1.0))
    ga, gi = torch.randn(P, 1, device=gpu, generator=gen), torch.randn(P, nx + F, device=gpu, generator=gen)
    for a, i in ((ga, None), (None, gi), (ga, gi)):
        gh = _nan_rows(P, 1 + F, gpu)
        lib.call("render_background_head_backward", P, nx, F, h, delta, a, i, gh)
        ref = TR.background_head_backward(h, delta, a, i, nx)
        assert torch.equal(TR.d(gh[:, 1:]), ref[:, 1:])
        _within("background_head_backward[edges]", gh[:, 0], ref[:, 0], 2e-5 * ref[:, 0].abs() + TR.FLT_MIN)
        if a is None:
            assert float(gh[:, 0].abs().max()) == 0.0


# ---- pixel normal, pixel compose ---------------------------------------------------------------------------------------------------
R3 = 2 * 256 + 3                     # three blocks of rays, the last one partial


def test_pixel_normal_three_blocks_and_degenerate_rows(gpu):
    """515 signed rows; one row exactly -eps in every component: 0 / 0, NaN where the fp32 stock spelling has NaN and nowhere
    else, forward and backward.  Value within 1e-6 max(|ref|, 1), gradient within 1e-5 sum|terms|.
    MI355X: value 0.08, gradient 0.025."""
    from ndjir_amd.volume import pixel_normal
    eps = 1e-6
    gen = _gen(gpu, 70)
    g = torch.randn(1, R3, 3, device=gpu, generator=gen)
    g[0, 300] = -torch.tensor(eps, device=gpu)
    g.requires_grad_(True)
    out = pixel_normal(g, eps)
    v = g.detach() + eps
    stock = v / torch.sqrt((v * v).sum(-1, keepdim=True))
    assert torch.equal(torch.isnan(out), torch.isnan(stock)) and bool(torch.isnan(out[0, 300]).all())
    ok = torch.ones(R3, dtype=torch.bool)
    ok[300] = False
    ref = TR.pixel_normal(g, eps)
    _within("pixel_normal", TR.d(out)[0][ok], ref[0][ok], 1e-6 * ref[0][ok].abs().clamp(min=1.0))
    w = torch.randn(1, R3, 3, device=gpu, generator=gen)
    (gg,) = torch.autograd.grad(out, g, w)
    rg, mag = TR.pixel_normal_backward(g, eps, w)
    assert bool(torch.isnan(gg[0, 300]).all()) and bool(torch.isfinite(TR.d(gg)[0][ok]).all())
    _within("pixel_normal_backward", TR.d(gg)[0][ok], rg[0][ok], 1e-5 * mag[0][ok])


def test_pixel_normal_tiny_row(gpu):
    """A row whose grad + eps is of the order 1e-20 (its squares are subnormal: the kernel's length then carries a relative
    error of up to 2^-149 / |v|^2 = 4e-7 here, inside the 1e-6) next to ordinary rows.  MI355X: value 0.05, gradient 0.013."""
    from ndjir_amd.volume import pixel_normal
    eps = 2.0 ** -67
    g = torch.randn(1, 9, 3, device=gpu, generator=_gen(gpu, 71))
    g[0, 4] = torch.tensor([4e-20, -3e-20, 2e-20], device=gpu) - eps
    g.requires_grad_(True)
    out = pixel_normal(g, eps)
    ref = TR.pixel_normal(g, eps)
    assert bool(torch.isfinite(out).all())
    _within("pixel_normal[tiny]", out, ref, 1e-6 * ref.abs().clamp(min=1.0))
    w = torch.randn(1, 9, 3, device=gpu, generator=_gen(gpu, 72))
    (gg,) = torch.autograd.grad(out, g, w)
    rg, mag = TR.pixel_normal_backward(g, eps, w)
    _within("pixel_normal_backward[tiny]", gg, rg, 1e-5 * mag)


@pytest.mark.parametrize("entangle", [True, False])
@pytest.mark.parametrize("Ce", [1, 3])
def test_pixel_compose_three_blocks_signed(gpu, entangle, Ce):
    """515 rays, inputs in [-1, 1], with a background and without (then no gradient for it exists).  Value within
    1e-6 max(|ref|, 1), gradients within 1e-6 max(sum|terms|, 1).  MI355X: value 0.13, gradients 0.11."""
    from ndjir_amd import lib
    from ndjir_amd.volume import pixel_compose
    gen = _gen(gpu, 80 + Ce)
    mk = lambda *s: (torch.rand(*s, device=gpu, generator=gen) * 2 - 1)
    pix, env, spec, bg, go = mk(1, R3, 9), mk(1, R3, Ce), mk(1, R3, 3), mk(1, R3, 3), mk(1, R3, 3)
    for with_bg in (True, False):
        ins = [t.clone().requires_grad_(True) for t in (pix, env, spec)] + ([bg.clone().requires_grad_(True)] if with_bg else [])
        out = pixel_compose(ins[0], ins[1], ins[2], ins[3] if with_bg else None, entangle)
        gout = torch.autograd.grad(out, ins, go)
        assert len(gout) == (4 if with_bg else 3)
        ref, gref, gmag = TR.pixel_compose(pix, env, spec, bg if with_bg else None, entangle, go)
        _within("pixel_compose", out, ref, 1e-6 * ref.abs().clamp(min=1.0))
        for a, b, m in zip(gout, gref, gmag):
            _within("pixel_compose_backward", a, b, 1e-6 * m.clamp(min=1.0))
        assert float(gout[0][..., 1:5].abs().max()) == 0.0                     # roughness / specular: not in the colour
        if with_bg:
            assert torch.equal(gout[3], go)
    # the entry point with no background gradient asked for writes the other three and nothing else
    g_pix, g_env, g_spec = _nan_rows(R3, 9, gpu), _nan_rows(R3, Ce, gpu), _nan_rows(R3, 3, gpu)
    lib.call("render_pixel_compose_backward", R3, Ce, int(entangle), pix, env, spec, go, g_pix, g_env, g_spec, None)
    assert torch.equal(g_pix, gout[0][0]) and torch.equal(g_env, gout[1][0]) and torch.equal(g_spec, gout[2][0])


# ---- loss terms ------------------------------------------------------------------------------------------------------------------
W_ALL = (0.1, 0.2, 0.3, 1e-2, 1e-3)
BIG = (1, R3, 130)                   # 3 passes of the final reduction, a partial last block of rays, 3 lane passes with a ragged tail


def _loss_case(B, R, N, seed, tv_widths=(4, 24), zero_mask=False):
    """CPU fp32 inputs.  Rays 0 and 1 differ in the mask alone (1 and 0.5)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    c = dict(color=rnd(B, R, 3), color_gt=rnd(B, R, 3), grad_x=rnd(B, R, N, 3), prior=torch.rand(B, R, 5, generator=g) * N,
             tvs=[torch.rand(B, R, N, D, generator=g) for D in tv_widths])
    mask = torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (B, R, 1, 1), generator=g)]
    if R > 1:
        for k in ("color", "color_gt", "grad_x", "prior"):
            c[k][0, 1] = c[k][0, 0]
        for t in c["tvs"]:
            t[0, 1] = t[0, 0]
        mask[0, 0], mask[0, 1] = 1.0, 0.5
    if R > 4:
        c["color"][0, 2] = c["color_gt"][0, 2]                      # L1 at d == 0
        c["color"][0, 4, 1] = c["color_gt"][0, 4, 1]
    c["mask"] = torch.zeros_like(mask) if zero_mask else mask
    return c


def _run_loss(gpu, c, N, weights=W_ALL, l2=False, N_prior=None, msum=None, upstream=1.0, gx=True, prior=True, tv=True, shards=1):
    """The wrapper against the reference: every term, every gradient.  -> (terms, gradients by name, reference)."""
    from ndjir_amd.volume import LOSS_TERM_NAMES, loss_terms
    B, R = c["color"].shape[:2]
    inv_rays = 1.0 / (B * R * shards)
    dev = lambda t: t.to(gpu).requires_grad_(True)
    c_d = dev(c["color"])
    gx_d = dev(c["grad_x"]) if gx else None
    pr_d = dev(c["prior"]) if prior else None
    tv_d = [dev(t) for t in c["tvs"]] if tv else []
    msum_d = None if msum is None else torch.tensor(msum, device=gpu)
    terms = loss_terms(c_d, c["color_gt"].to(gpu), c["mask"].to(gpu), gx_d, pr_d, msum_d, N, inv_rays, weights, l2, tv_d, N_prior=N_prior)
    ref = TR.loss_terms(c["color"], c["color_gt"], c["mask"], c["grad_x"] if gx else None, c["prior"] if prior else None,
                        c["tvs"] if tv else [], N, inv_rays, weights, l2, N_prior=N_prior,
                        mask_sum_global=None if msum is None else torch.tensor(msum), upstream=upstream)
    assert LOSS_TERM_NAMES == TR.LOSS_TERM_NAMES
    worst, val = 0.0, terms.detach().cpu()
    for i, k in enumerate(LOSS_TERM_NAMES):
        want = ref["terms"][k]
        worst = max(worst, abs(float(val[i]) - want) / max(2e-5 * abs(want), 1e-9))
    print(f"RATIO loss_terms {worst:.3g}")
    for i, k in enumerate(LOSS_TERM_NAMES):
        assert float(val[i]) == pytest.approx(ref["terms"][k], rel=2e-5, abs=1e-9), k
    assert float(val[9]) == pytest.approx(ref["inv_denorm"], rel=2e-6) and float(val[11]) == pytest.approx(ref["inv_denorm_prior"], rel=2e-6)
    assert float(val[10]) == pytest.approx(float(c["mask"].sum()), rel=1e-6)
    leaves = [c_d] + ([gx_d] if gx else []) + ([pr_d] if prior else []) + tv_d
    gout = list(torch.autograd.grad(terms[0], leaves, grad_outputs=torch.tensor(upstream, device=gpu)))
    got = dict(color=gout.pop(0), grad_x=gout.pop(0) if gx else None, prior=gout.pop(0) if prior else None, tvs=gout)
    rel = lambda r: 2e-5 * r.abs().clamp(min=1e-12)
    _within("loss_terms_backward color", got["color"], ref["grads"]["color"], rel(ref["grads"]["color"]))
    if gx:
        # |grad| - 1 cancels: relative to the magnitude with |grad| + 1 in its place
        _within("loss_terms_backward grad_x", got["grad_x"], ref["grads"]["grad_x"], 2e-5 * ref["gx_mag"].clamp(min=1e-12))
    if prior:
        _within("loss_terms_backward prior", got["prior"], ref["grads"]["prior"], rel(ref["grads"]["prior"]))
    for a, b in zip(got["tvs"], ref["grads"]["tvs"]):
        _within("loss_terms_backward tv", a, b, rel(b))
    return terms.detach(), got, ref


@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("size", [(1, 1, 1), BIG])
def test_loss_terms_real_mask(gpu, size, l2):
    """Mask values 0, 0.25, 0.5, 1: every term and gradient; between two rays that differ in the mask alone (1 and 0.5) the
    gradient of grad_x scales with m^2 and those of the TV tensors and the prior sums with m, bit for bit (powers of two);
    the L1 gradient at color == gt is exactly 0; the same call twice gives the same bits.
    MI355X (all loss tests): terms <= 0.01 of 2e-5, gradients <= 0.009."""
    from ndjir_amd.volume import loss_terms
    B, R, N = size
    c = _loss_case(B, R, N, 90)
    terms, got, _ = _run_loss(gpu, c, N, l2=l2)
    if R > 4:
        assert torch.equal(got["grad_x"][0, 0], 4 * got["grad_x"][0, 1]) and float(got["grad_x"][0, 0].abs().max()) > 0
        assert torch.equal(got["prior"][0, 0], 2 * got["prior"][0, 1]) and float(got["prior"][0, 0].abs().min()) > 0
        for t in got["tvs"]:
            assert torch.equal(t[0, 0], 2 * t[0, 1]) and float(t[0, 0].abs().min()) > 0
        assert float(got["color"][0, 2].abs().max()) == 0.0 and float(got["color"][0, 4, 1]) == 0.0
        assert float(got["color"][0, 4, 0]) != 0.0
        dev = lambda t: t.to(gpu)
        again = loss_terms(dev(c["color"]), dev(c["color_gt"]), dev(c["mask"]), dev(c["grad_x"]), dev(c["prior"]), None, N, 1.0 / (B * R),
                           W_ALL, l2, [dev(t) for t in c["tvs"]])
        assert torch.equal(again[:9], terms[:9])


@pytest.mark.parametrize("upstream", [1.0, -2.5])
def test_loss_terms_upstream_prior_count_and_global_mask_sum(gpu, upstream):
    """An upstream gradient of the total; the priors divided by their own N (64 against 130) with the eikonal term on; the mask
    sum of all ray shards handed in."""
    B, R, N = BIG
    c = _loss_case(B, R, N, 91)
    _run_loss(gpu, c, N, upstream=upstream, N_prior=64)
    _run_loss(gpu, c, N, upstream=upstream, l2=True, msum=float(c["mask"].sum()) * 2.5, shards=4)


OFF = {0: ("loss_eikonal",), 1: ("loss_tv",), 2: ("prior_base_color",), 3: ("prior_roughness", "reg_std_roughness"),
       4: ("prior_specular_reflectance", "reg_std_specular_reflectance")}
PRIOR_COLS = {2: [0], 3: [1, 2], 4: [3, 4]}


@pytest.mark.parametrize("off", [(0,), (1,), (2,), (3,), (4,), (0, 1, 2, 3, 4)])
def test_loss_terms_zero_weights(gpu, off):
    """A weight of zero: the term is reported as exactly 0.0, the total is the reference's (which does not evaluate the term),
    and the gradients of the term's inputs are exactly zero."""
    from ndjir_amd.volume import LOSS_TERM_NAMES
    B, R, N = BIG
    c = _loss_case(B, R, N, 92)
    w = [0.0 if k in off else v for k, v in enumerate(W_ALL)]
    terms, got, _ = _run_loss(gpu, c, N, weights=w)
    for k in range(5):
        for name in OFF[k]:
            assert (float(terms[LOSS_TERM_NAMES.index(name)]) == 0.0) == (k in off), name
    if 0 in off:
        assert float(got["grad_x"].abs().max()) == 0.0
    if 1 in off:
        assert all(float(t.abs().max()) == 0.0 for t in got["tvs"])
    for k in (2, 3, 4):
        assert (float(got["prior"][..., PRIOR_COLS[k]].abs().max()) == 0.0) == (k in off)


def test_loss_terms_nonfinite_prior_of_switched_off_terms(gpu):
    """Prior weights zero and Inf / NaN in the matching columns of `prior` (total_loss always passes the tensor): the total and
    g_color are finite and equal to those of the finite input."""
    from ndjir_amd.volume import loss_terms
    B, R, N = BIG
    c = _loss_case(B, R, N, 93)
    w = (0.1, 0.2, 0.3, 0.0, 0.0)
    terms, got, ref = _run_loss(gpu, c, N, weights=w)
    bad = c["prior"].clone()
    bad[0, 5, 1], bad[0, 6, 2], bad[0, 7, 3], bad[0, 8, 4] = INF, NAN, -INF, NAN
    bad[0, 9, 3] = INF                                              # a ray whose mask may be zero as well: 0 * Inf
    c_d, pr_d = c["color"].to(gpu).requires_grad_(True), bad.to(gpu).requires_grad_(True)
    dev = lambda t: t.to(gpu)
    t2 = loss_terms(c_d, dev(c["color_gt"]), dev(c["mask"]), dev(c["grad_x"]), pr_d, None, N, 1.0 / (B * R), w, False, [dev(t) for t in c["tvs"]])
    assert torch.equal(t2[:5], terms[:5]) and float(t2.detach()[5:9].abs().max()) == 0.0 and bool(torch.isfinite(t2).all())
    g_c, g_p = torch.autograd.grad(t2[0], [c_d, pr_d])
    assert torch.equal(g_c, got["color"]) and bool(torch.isfinite(g_p).all()) and float(g_p[..., 1:].abs().max()) == 0.0
    assert torch.equal(g_p[..., 0], got["prior"][..., 0])


@pytest.mark.parametrize("absent", [("gx",), ("prior",), ("tv",), ("gx", "prior", "tv")])
def test_loss_terms_absent_tensors(gpu, absent):
    """grad_x = None, prior = None, no TV tensors: each alone and all together; their terms are 0."""
    from ndjir_amd.volume import LOSS_TERM_NAMES
    B, R, N = BIG
    c = _loss_case(B, R, N, 94)
    terms, _, _ = _run_loss(gpu, c, N, **{k: False for k in absent})
    gone = dict(gx=[2], prior=[4, 5, 6, 7, 8], tv=[3])
    for k in absent:
        assert all(float(terms[i]) == 0.0 for i in gone[k]), k
    if len(absent) == 3:
        assert float(terms[0]) == float(terms[1])


def test_loss_terms_all_zero_mask(gpu):
    """No ray hits: the normalisers are 1 / 1e-5, every masked term is 0, the gradients are finite and the reference's."""
    B, R, N = BIG
    c = _loss_case(B, R, N, 95, zero_mask=True)
    terms, got, _ = _run_loss(gpu, c, N)
    assert float(terms[9]) == pytest.approx(1e5, rel=1e-6) and float(terms[11]) == pytest.approx(1e5, rel=1e-6) and float(terms[10]) == 0.0
    assert float(terms[2:9].abs().max()) == 0.0 and float(terms[0]) == float(terms[1])
    for t in [got["color"], got["grad_x"], got["prior"]] + got["tvs"]:
        assert bool(torch.isfinite(t).all())
    assert float(got["grad_x"].abs().max()) == 0.0 and float(got["prior"].abs().max()) == 0.0
