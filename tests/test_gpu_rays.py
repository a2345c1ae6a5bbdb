"""The per-ray kernels of csrc/render.hip -- alpha / transmittance / weights, the VR integrals, the light integrals, the
material head, the gain, each with its hand-derived backward -- against the fp64 references of tests/render_ref.py, element by
element, through `lib.call` (a few cases per kernel through the ndjir_amd.volume wrapper as well): past one loop pass and one
wave, at every switch between two code paths, at the limits the host code accepts and just past them.

Every output is cut from a NaN-filled buffer between NaN guards: the guards and any padding stay NaN, every element the
reference has is written.  Every comparison is per element, against a bound tied to that element's own magnitude or to the sum
of the absolute values of the terms it adds (u = 2^-24):

* alpha (2 |x1| + 2 |x0| sigmoid(-x0) + (2 G + 1) (1 + rho) + 19) u |ref| (render_ref.alpha_roundings: the 2 |x1| + 15 of the
  earlier far-outside test plus what iter_cos and the sample's length add); trans_i given the kernel's own alpha (3 i + 2) u |ref|, weights one rounding more;
* sums of T products (T + c) u sum|terms|, c the rounded operations of one term, counted from the kernel in the docstring of the
  test; a single product 2 u |ref| + 2^-126;
* the GGX / UE4 algebra (specular kernels, direct_light): max(c, 4 rho32) u sum|terms|, rho32 = the largest error of the fp32
  stock-op composite (render_ref in float32, on the CPU, same inputs) over u sum|terms| of its element.

No element is left out of any comparison: the input builders keep the kinks away from the data, the exact-kink cases are built
from exactly representable numbers.  Every check prints `RATIO <kernel> <largest error / bound>`; the docstrings quote the
MI355X figures."""
import pytest
import torch

from tests import render_ref as RR
from tests.test_gpu_tail import _guarded, _guards_untouched, _ratio, _within  # noqa: F401

pytestmark = pytest.mark.gpu
NAN = float("nan")
U, FLT_MIN, F32 = RR.U, RR.FLT_MIN, torch.float32


class Out:
    """An output of `shape` cut from a NaN buffer between two NaN guards."""

    def __init__(self, gpu, *shape):
        self.n = 1
        for s in shape:
            self.n *= s
        self.buf, flat = _guarded(self.n, gpu)
        self.t = flat.view(*shape)

    def guards_ok(self):
        return _guards_untouched(self.buf, self.n)

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


def _dev(gpu, *ts):
    return [None if t is None else t.to(gpu).contiguous() for t in ts]


def _rel(ref, c):
    return c * U * ref.abs() + FLT_MIN


# ---- (a) alpha, transmittance, weights ---------------------------------------------------------------------------------------------
def _alpha_args(gpu, b, Nb):
    sdf, n, rd, t, gain, car, mask = _dev(gpu, b["sdf"], b["n"], b["raydir"], b["t"], b["gain"], b["car"], b["mask"])
    abg = b["alpha_bg"].to(gpu).contiguous() if Nb else None
    return [sdf, n, rd, t, gain, car, mask, abg]


def _alpha_forward(gpu, b, R, N, Nb, tag):
    from ndjir_amd import lib
    args = _alpha_args(gpu, b, Nb)
    a, tr, w = Out(gpu, R, N), Out(gpu, R, N + Nb), Out(gpu, R, N + Nb)
    lib.call("render_alpha_weights", R, N, Nb, *args, a.t, tr.t, w.t)
    assert a.guards_ok() and tr.guards_ok() and w.guards_ok()
    ref, count = RR.alpha_fg(b["sdf"], b["n"], b["raydir"], b["t"], b["gain"], b["car"])
    _within(f"alpha_weights[{tag}] alpha_fg", a.t, ref, count * U * ref.abs())
    a_all = a.t * args[6][:, None]
    if Nb:
        a_all = torch.cat([a_all, args[7]], dim=1)
    rt, rw = RR.scan(a_all)
    i = torch.arange(N + Nb, dtype=torch.float64)
    _within(f"alpha_weights[{tag}] trans", tr.t, rt, (3 * i + 2) * U * rt.abs())
    _within(f"alpha_weights[{tag}] weights", w.t, rw, (3 * i + 3) * U * rw.abs())
    return args, a.t, tr.t, w.t


@pytest.mark.parametrize("N,Nb", RR.ALPHA_SHAPES)
def test_alpha_weights_forward(gpu, N, Nb):
    """R = 1, 3, 130; mask in {0, 0.25, 1}; ray 0 opaque at sample 3 (trans exactly 0 behind it), a background alpha of 1,
    samples with t unsorted (alpha exactly 0).  MI355X: alpha <= 0.46, trans <= 0.27, weights <= 0.24."""
    for R in RR.RAYS:
        b = RR.build_alpha(R, N, Nb, 100 + N)
        _, a, tr, w = _alpha_forward(gpu, b, R, N, Nb, f"{R}x{N}+{Nb}")
        if N >= 8:
            assert float(a[0, 3]) == 1.0 and float(tr[0, 4:].abs().max()) == 0.0 and float(w[0, 4:].abs().max()) == 0.0
            assert bool((a[R - 1] == 0.0).any())


GRADS = {"alpha": (1, 0, 0), "trans": (0, 1, 0), "weights": (0, 0, 1), "all": (1, 1, 1)}


@pytest.mark.parametrize("N,Nb", RR.ALPHA_SHAPES)
def test_alpha_weights_backward(gpu, N, Nb):
    """Each upstream gradient alone (R = 1, 3) and all three (R = 1, 3, 130); g_alpha_bg asked for and not.  Reference: autograd of
    the fp64 formulas with the scan evaluated at the kernel's alpha.  Bounds, from k_alpha_weights_bwd: dL/dA_i = trans_i (gw_i - S_i)
    reads trans_i (3 i + 2 roundings) and S_i, a Horner recurrence of two rounded operations per sample behind i --
    K_i = 3 i + 2 + 2 (S - 1 - i), on the share of the terms that came through the scan (g_alpha_fg does not); the chain from A to sdf has 32 rounded operations (g_n: 40) and the arguments x = gain s of the
    sigmoids carry u (|x0| + |x1| + |gain ic delta|) absolute, which is the relative error of sigmoid' and of c1:
    K_i u sum|scan terms| + (2 xs + 40) u sum|terms|; sigmoid' = c (1 - c) is formed from a c that is rounded to u near 1, an error of u c beside
    c (1 - c): + 4 u of the terms with c in place of c (1 - c).  g_alpha_bg: (K_i + 4) u sum|terms|.  g_gain_ray: its N terms, the
    same per term, + N u.  MI355X: g_sdf <= 0.33, g_n <= 0.34, g_gain_ray <= 0.23, g_alpha_bg <= 0.043."""
    from ndjir_amd import lib
    for R in RR.RAYS:
        b = RR.build_alpha(R, N, Nb, 100 + N)
        args, a, tr, w = _alpha_forward(gpu, b, R, N, Nb, f"{R}x{N}+{Nb}")
        gen = torch.Generator().manual_seed(7 + N)
        gs = [torch.randn(R, N, generator=gen), torch.randn(R, N + Nb, generator=gen), torch.randn(R, N + Nb, generator=gen)]
        for which in (("all",) if R == 130 else sorted(GRADS)):
            use = GRADS[which]
            gd = [g.to(gpu) if u_ else None for g, u_ in zip(gs, use)]
            bg = Out(gpu, R, max(Nb, 1))
            g_sdf, g_n, g_gain = Out(gpu, R, N), Out(gpu, R, N, 3), Out(gpu, R)
            lib.call("render_alpha_weights_backward", R, N, Nb, *args, tr, *gd, g_sdf.t, g_n.t, g_gain.t, bg.t if Nb else None)
            assert g_sdf.guards_ok() and g_n.guards_ok() and g_gain.guards_ok() and (bg.guards_ok() if Nb else bg.untouched())
            o_sdf, o_n, o_gain = Out(gpu, R, N), Out(gpu, R, N, 3), Out(gpu, R)              # the same without g_alpha_bg: the same bits
            lib.call("render_alpha_weights_backward", R, N, Nb, *args, tr, *gd, o_sdf.t, o_n.t, o_gain.t, None)
            assert torch.equal(o_sdf.t, g_sdf.t) and torch.equal(o_n.t, g_n.t) and torch.equal(o_gain.t, g_gain.t)
            r = RR.alpha_weights_backward(b["sdf"], b["n"], b["raydir"], b["t"], b["gain"], b["car"], b["mask"], b["alpha_bg"], a,
                                          *[g if u_ else None for g, u_ in zip(gs, use)])
            K = 2 * r["xs"] + 40                       # (the scan's K_i multiplies only what came through the scan: hmag_*)
            tag = f"{R}x{N}+{Nb},{which}"
            _within(f"alpha_weights_backward[{tag}] g_sdf", g_sdf.t, r["g_sdf"], U * (r["hmag_sdf"] + K * r["mag_sdf"] + 4 * r["sig_sdf"]) + FLT_MIN * (r["mag_sdf"] > 0))
            _within(f"alpha_weights_backward[{tag}] g_n", g_n.t, r["g_n"], U * (r["hmag_n"] + K[..., None] * r["mag_n"] + 4 * r["sig_n"]) + FLT_MIN * (r["mag_n"] > 0))
            _within(f"alpha_weights_backward[{tag}] g_gain_ray", g_gain.t, r["g_gain_ray"],
                    U * ((r["hmag_gain"] + (K + N) * r["mag_gain"]).sum(1) + 4 * r["sig_gain"].sum(1)) + FLT_MIN * (r["mag_gain"].sum(1) > 0))
            if Nb:
                _within(f"alpha_weights_backward[{tag}] g_alpha_bg", bg.t, r["g_alpha_bg"],
                        (r["horner"][None, N:] + 4) * U * r["mag_bg"] + FLT_MIN * (r["mag_bg"] > 0))


def test_alpha_weights_refuses_more_than_512_slots(gpu):
    """(481, 32) is one sample past RD_SLOTS: both entry points raise before any launch, the outputs stay NaN."""
    from ndjir_amd import lib
    R, N, Nb = 3, 481, 32
    b = RR.build_alpha(R, N, Nb, 9, opaque=False, unsorted=False)
    args = _alpha_args(gpu, b, Nb)
    outs = [Out(gpu, R, N), Out(gpu, R, N + Nb), Out(gpu, R, N + Nb)]
    with pytest.raises(RuntimeError):
        lib.call("render_alpha_weights", R, N, Nb, *args, *[o.t for o in outs])
    gouts = [Out(gpu, R, N), Out(gpu, R, N, 3), Out(gpu, R), Out(gpu, R, Nb)]
    z = torch.zeros(R, N + Nb, device=gpu)
    with pytest.raises(RuntimeError):
        lib.call("render_alpha_weights_backward", R, N, Nb, *args, z, None, z, z, *[o.t for o in gouts])
    assert all(o.untouched() for o in outs + gouts)


def test_alpha_weights_through_the_wrapper(gpu):
    """volume.alpha_weights at (B, R, N, Nb) = (2, 3, 65, 0) and (1, 3, 63, 1): the same numbers as the direct call, bit for bit,
    and the gain gradient the sum of the per-ray ones."""
    from ndjir_amd import lib
    from ndjir_amd.volume import alpha_weights
    for B, R, N, Nb in ((2, 3, 65, 0), (1, 3, 63, 1)):
        b = RR.build_alpha(B * R, N, Nb, 100 + N)
        args = _alpha_args(gpu, b, Nb)
        sdf, n, gain = args[0].view(B, R, N, 1).requires_grad_(True), args[1].view(B, R, N, 3).requires_grad_(True), args[4].clone().requires_grad_(True)
        abg = b["alpha_bg"].to(gpu).view(B, R, Nb, 1).requires_grad_(True)
        a, tr, w = alpha_weights(sdf, n, args[2].view(B, R, 3), args[3].view(B, R, N + 1, 1), gain, args[5], args[6].view(B, R, 1, 1), abg)
        _, a0, tr0, w0 = _alpha_forward(gpu, b, B * R, N, Nb, "wrapper")
        assert torch.equal(a.reshape(-1), a0.reshape(-1)) and torch.equal(tr.reshape(-1), tr0.reshape(-1)) and torch.equal(w.reshape(-1), w0.reshape(-1))
        gw = torch.randn(w.shape, device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))
        g_sdf, g_n, g_gain, g_bg = torch.autograd.grad(w, [sdf, n, gain, abg], gw)
        d_sdf, d_n, d_gain, d_bg = Out(gpu, B * R, N), Out(gpu, B * R, N, 3), Out(gpu, B * R), Out(gpu, B * R, max(Nb, 1))
        lib.call("render_alpha_weights_backward", B * R, N, Nb, *args, tr0, None, None, gw.view(B * R, N + Nb).contiguous(), d_sdf.t, d_n.t, d_gain.t,
                 d_bg.t if Nb else None)
        assert torch.equal(g_sdf.reshape(-1), d_sdf.t.reshape(-1)) and torch.equal(g_n.reshape(-1), d_n.t.reshape(-1))
        assert torch.equal(g_gain.reshape(()), d_gain.t.sum()) and g_bg.shape == (B, R, Nb, 1)
        if Nb:
            assert torch.equal(g_bg.reshape(-1), d_bg.t.reshape(-1))


# ---- (b) integrate -----------------------------------------------------------------------------------------------------------------
def _integrate_case(gpu, R, S, C, ldx, off, S_all, seed, tag):
    from ndjir_amd import lib
    from ndjir_amd.mlp import _Strided
    gen = torch.Generator().manual_seed(seed)
    w_all, x_all, g = torch.randn(R, S_all, generator=gen), torch.randn(R, S, ldx, generator=gen), torch.randn(R, C, generator=gen)
    wd, xd, gd = _dev(gpu, w_all, x_all, g)
    w, x = w_all[:, off:off + S], x_all[..., :C]
    out = Out(gpu, R, C)
    lib.call("render_integrate", R, S, C, _Strided(wd[:, off:]), S_all, _Strided(xd), ldx, out.t)
    assert out.guards_ok()
    ref, mag, T = RR.integrate(w, x)
    _within(f"integrate[{tag}]", out.t, ref, (T + 2) * U * mag)
    gxr, gwr, gwmag, Tc = RR.integrate_backward(w, x, g)
    for need_x, need_w in ((True, True), (False, True), (True, False)):
        gx, gw = Out(gpu, R, S, C), Out(gpu, R, S_all)
        lib.call("render_integrate_backward", R, S, C, _Strided(wd[:, off:]), S_all, _Strided(xd), ldx, gd, gx.t if need_x else None,
                 _Strided(gw.t[:, off:]) if need_w else None, S_all)
        assert gx.guards_ok() and gw.guards_ok()
        if need_x:
            _within(f"integrate_backward[{tag}] gx", gx.t, gxr, _rel(gxr, 2))
        else:
            assert gx.untouched()
        if need_w:
            _within(f"integrate_backward[{tag}] gw", gw.t[:, off:off + S], gwr, (Tc + 2) * U * gwmag)
            assert bool(torch.isnan(gw.t[:, :off]).all()) and bool(torch.isnan(gw.t[:, off + S:]).all()), "the other weight positions"
        else:
            assert gw.untouched()


@pytest.mark.parametrize("S,C", RR.INTEGRATE_SHAPES)
def test_integrate(gpu, S, C):
    """R = 1, 3, 130 at every (S, C) of the table -- TY == 1 (C = 256 / 257 / 300), TY = 256 with S > TY, the thread- / wave-per-sample
    switch of the backward (C = 4 / 5), its second lane trip (C = 64 / 65) -- packed, then as a column slice (ldx = C + 3) of a
    foreground part (off = 2, ldw = S + 5); gx null, gw null, neither.  Signed weights.  (T + 2) u sum|terms| with T = S forward,
    T = C for gw; gx 2 u |ref| + 2^-126.  MI355X: forward <= 0.32, gw <= 0.37, gx 0.5."""
    for R in RR.RAYS:
        _integrate_case(gpu, R, S, C, C, 0, S, 10 + C, f"{R}x{S}x{C}")
    _integrate_case(gpu, 3, S, C, C + 3, 2, S + 5, 11 + C, f"3x{S}x{C},slice")


# ---- (c) integrate_many --------------------------------------------------------------------------------------------------------------
def _many_inputs(gpu, R, S_all, widths, lds, Ss, seed):
    """x_k: a column slice of C_k out of rows of ld_k, its first element k floats into its allocation."""
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(R, S_all, generator=gen)
    xs, xds, gs = [], [], []
    for k, (C, ld, S) in enumerate(zip(widths, lds, Ss)):
        full = torch.randn(R, S, ld, generator=gen)
        flat = torch.zeros(R * S * ld + 8, device=gpu)
        flat[k % 4:k % 4 + R * S * ld] = full.reshape(-1).to(gpu)
        xs.append(full[..., :C])
        xds.append(flat[k % 4:k % 4 + R * S * ld].view(R, S, ld))
        gs.append(torch.randn(R, C, generator=gen))
    return w, xs, xds, gs


def _many_forward(gpu, case, offs=None, Ss=None, tag=""):
    from ndjir_amd import lib
    from ndjir_amd.mlp import _Strided
    R, S_all, widths, lds = case["R"], case["S_all"], case["widths"], case["lds"]
    Ss = Ss or [S_all] * len(widths)
    offs = offs or [0] * len(widths)
    w, xs, xds, gs = _many_inputs(gpu, R, S_all, widths, lds, Ss, 20 + len(widths))
    outs = [Out(gpu, R, C) for C in widths]
    lib.call("render_integrate_many", R, S_all, w.to(gpu), len(widths), [_Strided(x) for x in xds], list(lds), list(widths), list(Ss), list(offs),
             [o.t for o in outs])
    for k, (o, x, off, S) in enumerate(zip(outs, xs, offs, Ss)):
        assert o.guards_ok()
        ref, mag, T = RR.integrate(w[:, off:off + S], x)
        _within(f"integrate_many[{tag}] segment {k} (C = {widths[k]})", o.t, ref, (T + 2) * U * mag)


def _many_backward(gpu, case, offs=None, Ss=None, no_g=(), need_w=True, tag=""):
    from ndjir_amd import lib
    from ndjir_amd.mlp import _Strided
    R, S_all, widths, lds = case["R"], case["S_all"], case["widths"], case["lds"]
    Ss = Ss or [S_all] * len(widths)
    offs = offs or [0] * len(widths)
    w, xs, xds, gs = _many_inputs(gpu, R, S_all, widths, lds, Ss, 30 + len(widths))
    gs = [None if k in no_g else g for k, g in enumerate(gs)]
    gxs = [Out(gpu, R, S, C) for S, C in zip(Ss, widths)]
    gw = Out(gpu, R, S_all)
    lib.call("render_integrate_many_backward", R, S_all, w.to(gpu), len(widths), [_Strided(x) for x in xds], list(lds), list(widths), list(Ss),
             list(offs), [None if g is None else g.to(gpu) for g in gs], [o.t for o in gxs], gw.t if need_w else None)
    rgx, rgw, mag, T = RR.integrate_many_backward(w, xs, offs, gs)
    for k, (o, r) in enumerate(zip(gxs, rgx)):
        assert o.guards_ok()
        if r is None:
            assert o.untouched(), "a segment without a gradient gets no gx"
        else:
            _within(f"integrate_many_backward[{tag}] gx {k} (C = {widths[k]})", o.t, r, _rel(r, 2))
    assert gw.guards_ok()
    if need_w:
        _within(f"integrate_many_backward[{tag}] gw", gw.t, rgw, (T[None, :] + 2) * U * mag)
        uncovered = T == 0
        assert float(gw.t[:, uncovered.to(gw.t.device)].abs().max() if bool(uncovered.any()) else 0.0) == 0.0
    else:
        assert gw.untouched()
    return T


def test_integrate_many_forward_wide(gpu):
    """R = 2, S_all = 9, widths 3, 64, 65, 256 and 520 (a slice of 530): ny = 8, blockIdx.y > 0, the second c0 trip, the TX cap;
    then R = 1 x 40 and R = 5000 x 9.  (S + 2) u sum|terms|.  MI355X: <= 0.31."""
    _many_forward(gpu, RR.MANY_FWD, tag="wide")
    _many_forward(gpu, RR.MANY_ONE_RAY, tag="1x40")
    _many_forward(gpu, RR.MANY_STRIDE, tag="5000x9")
    _many_forward(gpu, RR.MANY_FWD, offs=[0, 2, 0, 5, 1], Ss=[9, 7, 4, 4, 8], tag="wide,parts")


def test_integrate_many_backward_wide(gpu):
    """The forward's widths plus 260 (six segments: IM_SEGS), then 258 / 260 / 9: the 16-byte branch past 256 channels (its second
    and third lane trips) and the scalar one (five trips), x rows at every float offset 0..3.  gw: (T_j + 2) u sum|terms|, T_j the
    channels of the segments covering j; gx: 2 u |ref| + 2^-126.  MI355X: gw <= 0.16, gx 0.5."""
    for k, case in enumerate(RR.MANY_BWD):
        _many_backward(gpu, case, tag=f"wide{k}")
    _many_backward(gpu, RR.MANY_BWD[0], need_w=False, tag="wide0,gw null")


def test_integrate_many_backward_walks(gpu):
    """R = 1, S_all = 40: ten workgroup rows, one position per wave.  R = 5000, S_all = 9: ny = 1, each wave walks j, j + 4, j + 8.
    MI355X: gw <= 0.16."""
    _many_backward(gpu, RR.MANY_ONE_RAY, tag="1x40")
    _many_backward(gpu, RR.MANY_STRIDE, tag="5000x9")


def test_integrate_many_backward_uncovered_positions_and_absent_gradients(gpu):
    """Segments over [0, 4), [2, 4) and [6, 9) of nine positions, the middle one without a gradient: positions 4 and 5 are covered
    by no segment, 2 and 3 only by segments 0: gw is exactly 0 at 4 and 5, NaN nowhere; the middle segment's gx is not written."""
    case = dict(R=3, S_all=9, widths=(5, 64, 260), lds=(5, 64, 261))
    T = _many_backward(gpu, case, offs=[0, 2, 6], Ss=[4, 2, 3], no_g=(1,), tag="uncovered")
    assert T.tolist() == [5, 5, 5, 5, 0, 0, 260, 260, 260]


def test_integrate_many_refusals(gpu):
    """Seven segments, and a segment that ends past S_all: refused by the host code before any launch, nothing written."""
    from ndjir_amd import lib
    R, S_all = 2, 9
    x = [torch.randn(R, S_all, 3, device=gpu) for _ in range(7)]
    g = [torch.randn(R, 3, device=gpu) for _ in range(7)]
    w = torch.randn(R, S_all, device=gpu)
    outs, gxs, gw = [Out(gpu, R, 3) for _ in range(7)], [Out(gpu, R, S_all, 3) for _ in range(7)], Out(gpu, R, S_all)
    for n, S, off in ((7, S_all, 0), (2, 5, 5)):
        cfg = ([3] * n, [3] * n, [S] * n, [off] * n)
        with pytest.raises(RuntimeError):
            lib.call("render_integrate_many", R, S_all, w, n, x[:n], *cfg, [o.t for o in outs[:n]])
        with pytest.raises(RuntimeError):
            lib.call("render_integrate_many_backward", R, S_all, w, n, x[:n], *cfg, g[:n], [o.t for o in gxs[:n]], gw.t)
    lib.call("render_integrate_many", R, S_all, w, 6, x[:6], [3] * 6, [3] * 6, [S_all] * 6, [0] * 6, [o.t for o in outs[:6]])      # six: accepted
    assert not any(o.untouched() for o in outs[:6]) and outs[6].untouched()
    assert all(o.untouched() for o in gxs) and gw.untouched()


def test_integrate_through_the_wrappers(gpu):
    """volume.integrate on a column slice with off > 0, volume.integrate_many with the 520-of-530 slice and an unused output:
    values and gradients against the references."""
    from ndjir_amd.volume import integrate, integrate_many
    gen = torch.Generator().manual_seed(40)
    B, R, S_all, S, off, C = 1, 3, 12, 9, 3, 65
    w = torch.randn(B, R, S_all, 1, generator=gen)
    wide = torch.randn(B, R, S, C + 3, generator=gen)
    g = torch.randn(B, R, C, generator=gen)
    wd, xd = w.to(gpu).requires_grad_(True), wide.to(gpu).requires_grad_(True)
    out = integrate(wd, xd[..., 1:1 + C], off)
    gw, gx = torch.autograd.grad(out, [wd, xd], g.to(gpu))
    ws, xs = w[0, :, off:, 0], wide[0, :, :, 1:1 + C]
    ref, mag, T = RR.integrate(ws, xs)
    _within("integrate[wrapper]", out[0], ref, (T + 2) * U * mag)
    rgx, rgw, gmag, Tc = RR.integrate_backward(ws, xs, g[0])
    _within("integrate_backward[wrapper] gx", gx[0, :, :, 1:1 + C], rgx, _rel(rgx, 2))
    assert float(gx[..., 0].abs().max()) == 0.0 and float(gx[..., 1 + C:].abs().max()) == 0.0 and float(gw[0, :, :off].abs().max()) == 0.0
    _within("integrate_backward[wrapper] gw", gw[0, :, off:, 0], rgw, (Tc + 2) * U * gmag)
    S_all = 9
    w = torch.randn(B, R, S_all, 1, generator=gen)
    wide = torch.randn(B, R, S_all, 530, generator=gen)
    x3, xb = torch.randn(B, R, S_all, 3, generator=gen), torch.randn(B, R, 4, 3, generator=gen)
    gs = [torch.randn(B, R, c, generator=gen) for c in (520, 3, 3)]
    wd, wided, x3d, xbd = (t.to(gpu).requires_grad_(True) for t in (w, wide, x3, xb))
    outs = integrate_many(wd, [wided[..., 5:525], x3d, xbd], [0, 0, 5])
    for o, x, o_, s_ in zip(outs, (wide[0, :, :, 5:525], x3[0], xb[0]), (0, 0, 5), (9, 9, 4)):
        ref, mag, T = RR.integrate(w[0, :, o_:o_ + s_, 0], x)
        _within("integrate_many[wrapper]", o[0], ref, (T + 2) * U * mag)
    got = torch.autograd.grad([outs[0], outs[2]], [wd, wided, x3d, xbd], [gs[0].to(gpu), gs[2].to(gpu)], allow_unused=True)
    assert got[2] is None
    rgx, rgw, mag, T = RR.integrate_many_backward(w[0, :, :, 0], [wide[0, :, :, 5:525], x3[0], xb[0]], [0, 0, 5], [gs[0][0], None, gs[2][0]])
    _within("integrate_many_backward[wrapper] gw", got[0][0, :, :, 0], rgw, (T[None, :] + 2) * U * mag)
    _within("integrate_many_backward[wrapper] gx wide", got[1][0, :, :, 5:525], rgx[0], _rel(rgx[0], 2))
    _within("integrate_many_backward[wrapper] gx bg", got[3][0], rgx[2], _rel(rgx[2], 2))


# ---- (d) light integrals -------------------------------------------------------------------------------------------------------------
def _light_rays(M):
    """R = 1, 3, 130 at every M but 300, where 130 rays are left out (R only moves blockIdx.x)."""
    return (1, 3) if M == 300 else RR.RAYS


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("M", RR.LIGHT_M)
def test_diffuse_light(gpu, M, C):
    """k_diffuse_light: a term is sv env max(n.l, eps) -- 5 roundings of the dot, 2 products, the division by M: (M + 8) u sum|terms|
    with sum_i |n_i l_i| in place of n.l.  Backward: g_env one chain of 9 roundings, 10 u; g_soft_vis C terms, (C + 10) u;
    g_normal M terms of C + 5 roundings each, (M + C + 8) u.  Lights under the surface.  MI355X: value 0.26, g_env 0.47, g_soft_vis 0.36, g_normal 0.22."""
    from ndjir_amd import lib
    for R in _light_rays(M):
        L = RR.build_lights(R, M, C, 200 + M)
        n, l, sv, e, g = _dev(gpu, L["normal"], L["light"], L["soft_vis"], L["env"], L["gC"])
        out = Out(gpu, R, C)
        lib.call("render_diffuse_light", R, M, C, n, l, sv, e, L["eps"], out.t)
        r = RR.diffuse_light(L["normal"], L["light"], L["soft_vis"], L["env"], L["eps"], L["gC"])
        tag = f"{R}x{M}x{C}"
        assert out.guards_ok()
        _within(f"diffuse_light[{tag}]", out.t, r["out"], (M + 8) * U * r["mag"])
        gn, gsv, ge = Out(gpu, R, 3), Out(gpu, R, M), Out(gpu, R, M, C)
        lib.call("render_diffuse_light_backward", R, M, C, n, l, sv, e, L["eps"], g, gn.t, gsv.t, ge.t)
        assert gn.guards_ok() and gsv.guards_ok() and ge.guards_ok()
        _within(f"diffuse_light_backward[{tag}] g_normal", gn.t, r["g_normal"], (M + C + 8) * U * r["mag_normal"])
        _within(f"diffuse_light_backward[{tag}] g_soft_vis", gsv.t, r["g_soft_vis"], (C + 10) * U * r["mag_soft_vis"] + FLT_MIN)
        _within(f"diffuse_light_backward[{tag}] g_env", ge.t, r["g_env"], 10 * U * r["mag_env"] + FLT_MIN)


SPEC_OUT = (("out", "mag", "T"), ("g_normal", "mag_normal", "T_ray"), ("g_rough", "mag_rough", "T_ray"), ("g_spec", "mag_spec", "T_ray"),
            ("g_soft_vis", "mag_soft_vis", None), ("g_env", "mag_env", None))
SPEC_C = 48            # rounded operations of one term of the GGX / UE4 algebra (spec_terms 34, spec_general and the colour loop the rest)


def _rho_check(name, got, r64, r32, keys):
    """Per element: |got - ref| <= max(T + SPEC_C, 4 rho32) u sum|terms|, rho32 = max |composite32 - ref| / (u sum|terms|)."""
    worst = 0.0
    for out, (key, mkey, tkey) in zip(got, keys):
        if out is None:
            continue
        ref, scale = r64[key], U * r64[mkey]
        err32 = (r32[key].double() - ref).abs()
        rho32 = float(torch.where(err32 == 0, torch.zeros_like(err32), err32 / scale).max())
        c = max((r64[tkey] if tkey else 0) + SPEC_C, 4.0 * rho32)
        print(f"RHO32 {name} {key} {rho32:.3g} (allowed {c:.3g} u)")
        worst = max(worst, _ratio(f"{name} {key}", out, ref, c * scale + FLT_MIN * (scale > 0)))
    assert worst <= 1.0, (name, worst)


def _spec_case(gpu, R, M, C, variant, seed):
    from ndjir_amd import lib
    L = RR.build_lights(R, M, C, seed)
    names = ("normal", "view", "light", "rough", "spec", "soft_vis", "env")
    dv = _dev(gpu, *[L[k] for k in names])
    eps, weight = L["eps"], 1.3
    if variant is None:
        fwd, bwd, cfg, kw = "render_specular_light_filament", "render_specular_light_filament_backward", (), dict(model=0, sampling=0, split=False)
    else:
        fwd, bwd, cfg, kw = "render_specular_light", "render_specular_light_backward", variant, dict(model=variant[0], sampling=variant[1], split=bool(variant[2]))
    out = Out(gpu, R, 3)
    lib.call(fwd, R, M, C, *cfg, *dv, eps, weight, out.t)
    outs = [Out(gpu, R, 3), Out(gpu, R), Out(gpu, R, 3), Out(gpu, R, M), Out(gpu, R, M, C)]
    lib.call(bwd, R, M, C, *cfg, *dv, eps, weight, L["g"].to(gpu), *[o.t for o in outs])
    assert out.guards_ok() and all(o.guards_ok() for o in outs)
    r64 = RR.specular_light(*[L[k] for k in names], eps, weight, g=L["g"], **kw)
    r32 = RR.specular_light(*[L[k] for k in names], eps, weight, g=L["g"], dtype=F32, **kw)
    _rho_check(f"specular_light[{variant},{R}x{M}x{C}]", [out.t] + [o.t for o in outs], r64, r32, SPEC_OUT)
    below = (RR.up(L["normal"])[:, None, :] * RR.up(L["light"])).sum(-1) < 0
    if not kw["split"] and bool(below.any()):            # (the split sum's mean of soft_vis env carries no mask)
        assert float(outs[3].t[below.to(gpu)].abs().max()) == 0.0, "a light under the surface: masked, exactly"


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("M", RR.LIGHT_M)
def test_specular_light_filament(gpu, M, C):
    """k_specular_light and its backward.  MI355X: rho32 <= 2.3e3 u per ray, 1.6e3 u per light (grazing lights and views among 130 rays); largest error / bound 0.76."""
    for R in _light_rays(M):
        _spec_case(gpu, R, M, C, None, 210 + M)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("sampling", [0, 1])
@pytest.mark.parametrize("model", [0, 1])
def test_specular_light_general(gpu, model, sampling, split):
    """k_specular_light_g<MODEL, SAMPLING, SPLIT> and its backward at M = 64, 65, 129, 300 (second wave empty / one light / both
    waves, second and third pass), C = 1 and 3, R = 1, 3, 130 (M = 300: 1, 3).  MI355X: rho32 per ray <= 80 u (importance), 371 u (filament, uniform), 6.2e3 u (ue4, uniform: a2 = r^4), per light <= 8.7e3 u; largest error / bound 0.76."""
    for M in (64, 65, 129, 300):
        for C in (1, 3):
            for R in _light_rays(M):
                _spec_case(gpu, R, M, C, (model, sampling, split), 220 + M)


DIRECT_OUT = (("color", "mag_color", "T"), ("env_pix", "mag_env_pix", "T"), ("spec_pix", "mag_spec_pix", "T"))
DIRECT_GRAD = (("g_normal", "mag_normal", "T_ray"), ("g_raw_sv", "mag_raw_sv", None), ("g_raw_env", "mag_raw_env", None), ("g_pix", "mag_pix", "T_ray"))
BETAS = (1.7, 0.6)


def _direct_case(gpu, R, M, C, acts, ub, entangle, with_bg, seed):
    from ndjir_amd import lib
    D = RR.build_direct(R, M, C, seed, acts, BETAS, ub, with_bg=with_bg)
    params = (BETAS[0], BETAS[1], ub, 1e-8, 0.7)
    names = ("normal", "view", "dirs", "raw_sv", "raw_env", "pix")
    dv = _dev(gpu, *[D[k] for k in names])
    bg = D["bg"].to(gpu) if with_bg else None
    color, envp, specp = Out(gpu, R, 3), Out(gpu, R, C), Out(gpu, R, 3)
    lib.call("render_direct_light", R, M, C, list(acts), list(params), int(entangle), *dv, bg, color.t, envp.t, specp.t)
    gouts = [Out(gpu, R, 3), Out(gpu, R, 2 * M), Out(gpu, R, 2 * M, C), Out(gpu, R, 9)]
    gbg = Out(gpu, R, 3)
    lib.call("render_direct_light_backward", R, M, C, list(acts), list(params), int(entangle), *dv, envp.t, specp.t, D["g"].to(gpu),
             *[o.t for o in gouts], gbg.t if with_bg else None)
    assert all(o.guards_ok() for o in [color, envp, specp, gbg] + gouts)
    r64 = RR.direct_light(*[D[k] for k in names], D["bg"], acts, params, entangle, D["g"])
    r32 = RR.direct_light(*[D[k] for k in names], D["bg"], acts, params, entangle, D["g"], dtype=F32)
    tag = f"direct_light[acts {acts},ub {ub},{'entangled' if entangle else 'plain'},{'bg' if with_bg else 'no bg'},{R}x{M}x{C}]"
    _rho_check(tag, [color.t, envp.t, specp.t], r64, r32, DIRECT_OUT)
    _rho_check(tag, [o.t for o in gouts], r64, r32, DIRECT_GRAD)
    if with_bg:
        assert torch.equal(gbg.t.cpu(), D["g"]), "g_bg is the upstream gradient"
    else:
        assert gbg.untouched()
    assert float(gouts[3].t[:, 0].abs().max()) > 0 and float(gouts[3].t[:, 1:5].abs().max()) > 0


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("M", [1, 129, 300])
def test_direct_light_default_pair(gpu, M, C):
    """k_direct_light and its backward, sigmoid / softplus (the default): both `entangle`, with and without a background, ub_env
    off and on.  MI355X: rho32 <= 209 u per ray, 2.2e3 u per light; largest error / bound 0.53."""
    for R in _light_rays(M):
        for entangle in (True, False):
            for with_bg in (True, False):
                for ub in (-1.0, 0.8):
                    _direct_case(gpu, R, M, C, (2, 1), ub, entangle, with_bg, 230 + M)


@pytest.mark.parametrize("act_env", [0, 1, 2, 3])
@pytest.mark.parametrize("act_sv", [0, 1, 2, 3])
def test_direct_light_every_activation_pair(gpu, act_sv, act_env):
    """Every pair of LIGHT_ACTS at M = 129, C = 3, with ub_env = 0.8 and without; softplus inputs at beta v = 19.5, 20, 20.5 (the
    threshold and either side of it).  MI355X: largest error / bound 0.29."""
    from ndjir_amd.volume import LIGHT_ACTS
    assert sorted(LIGHT_ACTS.values()) == [0, 1, 2, 3]
    for ub in (-1.0, 0.8):
        _direct_case(gpu, 3, 129, 3, (act_sv, act_env), ub, True, True, 240 + 4 * act_sv + act_env)


def test_light_wrappers_give_the_direct_bits(gpu):
    """volume.diffuse_light, specular_light_filament, specular_light (ue4, uniform, split sum) and direct_light at
    (B, R, M, C) = (2, 3, 129, 3) with env and the upstream gradient as column slices of wider arrays (the wrappers make them
    contiguous): values and every gradient are the direct calls' bits."""
    from ndjir_amd import lib
    from ndjir_amd import volume as V
    B, R, M, C = 2, 3, 129, 3
    L = RR.build_lights(B * R, M, C, 600)
    gen = torch.Generator().manual_seed(601)
    eps, weight = L["eps"], 1.3
    wide = lambda t: torch.cat([t, torch.randn(t.shape, generator=gen)], dim=-1).to(gpu)[..., :t.shape[-1]]      # a column slice
    leaf = lambda t, *s: wide(t.view(*s)).requires_grad_(True)
    n, rough, spec = leaf(L["normal"], B, R, 3), leaf(L["rough"], B, R, 1), leaf(L["spec"], B, R, 3)
    sv, env = leaf(L["soft_vis"], B, R, M, 1), leaf(L["env"], B, R, M, C)
    view, light = wide(L["view"].view(B, R, 3)), wide(L["light"].view(B, R, M, 3))
    assert not env.is_contiguous() and not light.is_contiguous()
    g3, gC = wide(L["g"].view(B, R, 3)), wide(L["gC"].view(B, R, C))
    dn, dv, dl, dr, ds, dsv, de, dg3, dgC = _dev(gpu, L["normal"], L["view"], L["light"], L["rough"], L["spec"], L["soft_vis"], L["env"], L["g"], L["gC"])
    P = B * R
    same = lambda a, o: torch.equal(a.reshape(-1), o.t.reshape(-1))
    # diffuse
    out = V.diffuse_light(n, light, sv, env, eps)
    got = torch.autograd.grad(out, [n, sv, env], gC)
    o, gouts = Out(gpu, P, C), [Out(gpu, P, 3), Out(gpu, P, M), Out(gpu, P, M, C)]
    lib.call("render_diffuse_light", P, M, C, dn, dl, dsv, de, eps, o.t)
    lib.call("render_diffuse_light_backward", P, M, C, dn, dl, dsv, de, eps, dgC, *[x.t for x in gouts])
    assert out.shape == (B, R, C) and same(out, o) and all(same(a, x) for a, x in zip(got, gouts)), "diffuse_light"
    # filament and one general instantiation
    for fn, extra, name, cfg in ((V.specular_light_filament, (), "render_specular_light_filament", ()),
                                 (V.specular_light, ("ue4", "uniform", True), "render_specular_light", (1, 1, 1))):
        out = fn(n, view, light, rough, spec, sv, env, eps, weight, *extra)
        got = torch.autograd.grad(out, [n, rough, spec, sv, env], g3)
        o, gouts = Out(gpu, P, 3), [Out(gpu, P, 3), Out(gpu, P), Out(gpu, P, 3), Out(gpu, P, M), Out(gpu, P, M, C)]
        lib.call(name, P, M, C, *cfg, dn, dv, dl, dr, ds, dsv, de, eps, weight, o.t)
        lib.call(name + "_backward", P, M, C, *cfg, dn, dv, dl, dr, ds, dsv, de, eps, weight, dg3, *[x.t for x in gouts])
        assert out.shape == (B, R, 3) and same(out, o) and all(same(a, x) for a, x in zip(got, gouts)), name
    # direct light
    acts, params = (2, 1), (BETAS[0], BETAS[1], 0.8, 1e-8, 0.7)
    D = RR.build_direct(P, M, C, 602, acts, BETAS, 0.8)
    names = ("normal", "view", "dirs", "raw_sv", "raw_env", "pix")
    dd = _dev(gpu, *[D[k] for k in names])
    dbg, dgo = _dev(gpu, D["bg"], D["g"])
    shapes = dict(normal=(B, R, 3), view=(B, R, 3), dirs=(B, R, 2 * M, 3), raw_sv=(B, R, 2 * M, 1), raw_env=(B, R, 2 * M, C), pix=(B, R, 9))
    w_ = {k: wide(D[k].view(*shapes[k])) for k in names}
    leaves = [w_[k].requires_grad_(True) for k in ("normal", "raw_sv", "raw_env", "pix")] + [wide(D["bg"].view(B, R, 3)).requires_grad_(True)]
    color = V.direct_light(leaves[0], w_["view"], w_["dirs"], leaves[1], leaves[2], leaves[3], leaves[4], acts, params, True)
    got = torch.autograd.grad(color, leaves, wide(D["g"].view(B, R, 3)))
    oc, oe, os_ = Out(gpu, P, 3), Out(gpu, P, C), Out(gpu, P, 3)
    lib.call("render_direct_light", P, M, C, list(acts), list(params), 1, *dd, dbg, oc.t, oe.t, os_.t)
    gouts = [Out(gpu, P, 3), Out(gpu, P, 2 * M), Out(gpu, P, 2 * M, C), Out(gpu, P, 9), Out(gpu, P, 3)]
    lib.call("render_direct_light_backward", P, M, C, list(acts), list(params), 1, *dd, oe.t, os_.t, dgo, *[x.t for x in gouts])
    assert color.shape == (B, R, 3) and same(color, oc) and all(same(a, x) for a, x in zip(got, gouts)), "direct_light"


def test_gain_through_the_wrapper(gpu):
    """volume.sdf_gain on a (2, 3) column slice with the reference's constants (scale 10, lo 1e-6, hi 5e4): the direct call's bits,
    value and gradient."""
    from ndjir_amd import lib
    from ndjir_amd.volume import sdf_gain
    gen = torch.Generator().manual_seed(603)
    p = (torch.rand(2, 6, generator=gen) * 2.2 - 1.3).to(gpu)[:, :3].requires_grad_(True)
    g = torch.randn(2, 6, generator=gen).to(gpu)[:, :3]
    assert not p.is_contiguous()
    out = sdf_gain(p)
    (gp,) = torch.autograd.grad(out, p, g)
    o, og = Out(gpu, 6), Out(gpu, 6)
    lib.call("render_gain", 6, p.detach().contiguous(), 10.0, 1e-6, 5e4, o.t)
    lib.call("render_gain_backward", 6, p.detach().contiguous(), 10.0, 1e-6, 5e4, g.contiguous(), og.t)
    assert out.shape == (2, 3) and torch.equal(out.reshape(-1), o.t) and torch.equal(gp.reshape(-1), og.t)


# ---- (e) material head, gain ----------------------------------------------------------------------------------------------------------
MAT_CFGS = [(r, e, s, 0.089, 0.16, 0.5, 0.04) for r in (0, 1) for e in (0, 1) for s in (0, 1)]


def _material_case(gpu, R, N, cfg, seed, with_prior=True):
    """V: a sigmoid is 4 roundings, its argument's own rounding u |x| relative, a square doubles both, the products add 2:
    (12 + 2 |x|) u |ref|, |x| the arguments of the element's sigmoids.  aux: sigmoids (6 + 2 |x|) u, std = softplus 8 u.  Prior
    sums of T terms: (T + 16 + 2 max|x|) u sum of the terms' scales (a difference: the sum of its operands; a logarithm: 1 + |log|).
    Raw gradients: chains of at most 40 roundings over 6 sigmoid-type factors, (40 + 6 |x|) u sum|terms|; where the chain ends in
    sigmoid' = s (1 - s), s is rounded to u near 1: + 2 u / (1 - s) = 2 (1 + e^x) u; the std columns hold |ro - prior| / std^2: +
    8 u of that term with ro + prior for the difference."""
    from ndjir_amd import lib
    raws, pg, gV, gp = RR.build_material(R, N, seed, cfg)
    dv = _dev(gpu, raws[0], raws[1], raws[2], raws[3], pg, raws[4], raws[5])
    V, aux, prior = Out(gpu, R, N, 9), Out(gpu, R, N, 10), Out(gpu, R, 5)
    lib.call("render_material_head", R, N, *dv, *cfg, V.t, aux.t, prior.t)
    assert V.guards_ok() and aux.guards_ok() and prior.guards_ok()
    r = RR.material_head(raws, pg, cfg, gV, gp if with_prior else None)
    x = [t.double().abs() for t in raws]
    xph = (x[3] * float(pg)).expand(R, N, 1)
    xV = torch.cat([x[2], x[4][..., 0:1], x[5][..., :3], xph, x[0] + (xph if cfg[1] else 0.0)], dim=-1)
    tag = f"{R}x{N},{cfg[:3]}"
    _within(f"material_head[{tag}] V", V.t, r["V"], (12 + 2 * xV) * U * r["V"].abs())
    xa = torch.cat([x[0], x[1], torch.zeros(R, N, 4, dtype=torch.float64)], dim=-1)
    _within(f"material_head[{tag}] aux", aux.t, r["aux"], (8 + 2 * xa) * U * r["aux"].abs())
    xmax = torch.stack([t.reshape(R, -1).amax(1) for t in (x[0], x[1], x[4][..., 0], x[5][..., :3])], dim=-1).amax(-1, keepdim=True)
    _within(f"material_head[{tag}] prior", prior.t, r["prior"], (r["T_prior"][None, :] + 16 + 2 * xmax) * U * r["mag_prior"])
    gouts = [Out(gpu, *t.shape) for t in raws]
    lib.call("render_material_head_backward", R, N, *dv, *cfg, gV.to(gpu), gp.to(gpu) if with_prior else None, *[o.t for o in gouts])
    own = [x[0], x[1], x[2], xph, torch.cat([x[4][..., 0:1], torch.zeros(R, N, 1, dtype=torch.float64)], -1),
           torch.cat([x[5][..., :3], torch.zeros(R, N, 3, dtype=torch.float64)], -1)]
    signed = [raws[0], raws[1], raws[2], raws[3] * float(pg), raws[4], raws[5]]
    for k, (o, ref, mag, extra, xo, sx, name) in enumerate(zip(gouts, r["grads"], r["mags"], r["extra"], own, signed,
                                                               ("base", "ptb", "implicit", "photo", "roughness", "specular"))):
        assert o.guards_ok()
        cancel = 2.0 * (1.0 + torch.exp(sx.double()))
        if k >= 4:
            cancel[..., (1 if k == 4 else 3):] = 0.0           # softplus' = sigmoid(h): no 1 - s
        _within(f"material_head_backward[{tag}] {name}", o.t, ref, (40 + 6 * xo + cancel) * U * mag + 8 * U * extra + FLT_MIN * (mag > 0))
    return gouts


@pytest.mark.parametrize("cfg", MAT_CFGS)
def test_material_head(gpu, cfg):
    """k_material_head and its backward over remap x entangle x sym at N = 1, 127, 128, 129, 300, 1030 (R = 1, 3, 130; at N = 300 and 1030
    R = 1, 3: the reference's 14 backward passes per case); raw std inputs at 19.5, 20, 20.5 and at -30, -40.  MI355X: V <= 0.43, aux <= 0.25, prior <= 0.09, gradients <= 0.64."""
    for N in RR.MATERIAL_N:
        for R in ((1, 3) if N >= 300 else RR.RAYS):
            _material_case(gpu, R, N, cfg, 500 + N)


def test_material_head_without_the_prior_gradient(gpu):
    """g_prior null: the gradient of V alone; the perturbed base colour gets exactly 0."""
    for cfg in (MAT_CFGS[0], MAT_CFGS[7]):
        gouts = _material_case(gpu, 3, 129, cfg, 77, with_prior=False)
        assert float(gouts[1].t.abs().max()) == 0.0


def test_material_head_through_the_wrapper(gpu):
    """volume.material_head at (B, R, N) = (2, 3, 129): the direct call's bits; with only V used, the null g_prior."""
    from ndjir_amd import lib
    from ndjir_amd.volume import material_head
    cfg = MAT_CFGS[7]
    B, R, N = 2, 3, 129
    raws, pg, gV, gp = RR.build_material(B * R, N, 78, cfg)
    leaves = [t.to(gpu).view(B, R, N, -1).requires_grad_(True) for t in raws]
    V, aux, prior = material_head(leaves[0], leaves[1], leaves[2], leaves[3], pg.to(gpu), leaves[4], leaves[5], *cfg)
    dv = _dev(gpu, raws[0], raws[1], raws[2], raws[3], pg, raws[4], raws[5])
    V0, aux0, prior0 = Out(gpu, B * R, N, 9), Out(gpu, B * R, N, 10), Out(gpu, B * R, 5)
    lib.call("render_material_head", B * R, N, *dv, *cfg, V0.t, aux0.t, prior0.t)
    assert torch.equal(V.reshape(-1), V0.t.reshape(-1)) and torch.equal(aux.reshape(-1), aux0.t.reshape(-1)) and torch.equal(prior.reshape(-1), prior0.t.reshape(-1))
    for with_prior in (True, False):
        got = torch.autograd.grad([V, prior] if with_prior else [V], leaves, [gV.to(gpu).view(B, R, N, 9)] + ([gp.to(gpu).view(B, R, 5)] if with_prior else []),
                                  retain_graph=True)
        gouts = [Out(gpu, *t.shape) for t in raws]
        lib.call("render_material_head_backward", B * R, N, *dv, *cfg, gV.to(gpu), gp.to(gpu) if with_prior else None, *[o.t for o in gouts])
        assert all(torch.equal(a.reshape(-1), o.t.reshape(-1)) for a, o in zip(got, gouts))


@pytest.mark.parametrize("n", [1, 130])
def test_gain(gpu, n):
    """k_gain: clamp(exp(10 p), 1e-6, 5e4) at values below lo, inside, above hi: inside 4 u |ref| + the argument's u |10 p| (expf
    2 u, the product 10 p one rounding), outside exactly the bound; gradient exactly 0 outside, g e scale inside (3 roundings more).
    MI355X: 0.65 / 0.56."""
    from ndjir_amd import lib
    gen = torch.Generator().manual_seed(n)
    p = torch.rand(n, generator=gen) * 2.2 - 1.3                      # 10 p in [-13, 9]: lo = e^-13.8, hi = e^10.8
    p[0] = 0.3
    if n > 3:
        p[1], p[2], p[3] = -2.0, 1.2, -1.45
    g = torch.randn(n, generator=gen)
    lo, hi = 1e-6, 5e4
    out, gp = Out(gpu, n), Out(gpu, n)
    lib.call("render_gain", n, p.to(gpu), 10.0, lo, hi, out.t)
    lib.call("render_gain_backward", n, p.to(gpu), 10.0, lo, hi, g.to(gpu), gp.t)
    assert out.guards_ok() and gp.guards_ok()
    ref, e, gref = RR.gain(p, 10.0, lo, hi, g)
    assert float(((e - RR.f32(lo)).abs() / RR.f32(lo)).min()) > 64 * U * 14 and float(((e - RR.f32(hi)).abs() / RR.f32(hi)).min()) > 64 * U * 14, "no value at the clamp"
    c = 4 + (10.0 * p.double()).abs()
    inside = (e > RR.f32(lo)) & (e < RR.f32(hi))
    _within(f"gain[{n}]", out.t, ref, torch.where(inside, c * U * ref.abs(), torch.zeros_like(ref)))
    _within(f"gain_backward[{n}]", gp.t, gref, (c + 3) * U * gref.abs())
    if n > 3:
        assert float(gp.t[1]) == 0.0 and float(gp.t[2]) == 0.0 and float(out.t[1]) == RR.f32(lo) and float(out.t[2]) == RR.f32(hi)
        assert float(gp.t[3]) == 0.0 and float(gp.t[0]) != 0.0


# ---- (f) exact kinks -------------------------------------------------------------------------------------------------------------------
def _exact_lights(gpu):
    """eps_dot = 0.25, n = (0, 0, 1); light 0 = (0.5, 0, 0.25): n.l == eps exactly; light 1 = (0, 0.5, 0.5).  Not unit vectors: every
    number is exactly representable.  view = (0.25, 0, 0.75)."""
    n = torch.tensor([[0.0, 0.0, 1.0]])
    l = torch.tensor([[[0.5, 0.0, 0.25], [0.0, 0.5, 0.5]]])
    v = torch.tensor([[0.25, 0.0, 0.75]])
    return n, v, l


def test_a_dot_equal_to_eps_diffuse(gpu):
    """raw == eps: the value is eps, the clamp passes the gradient (`>=`, as torch's clamp(min) does): with sv = env = g = 1 and
    M = 2 every number is exact -- g_normal = (l0 + l1) / 2 bit for bit."""
    from ndjir_amd import lib
    n, v, l = _exact_lights(gpu)
    one = torch.ones(1, 2)
    out, gn, gsv, ge = Out(gpu, 1, 1), Out(gpu, 1, 3), Out(gpu, 1, 2), Out(gpu, 1, 2, 1)
    nd, ld, sv, e, g = _dev(gpu, n, l, one, one.view(1, 2, 1), torch.ones(1, 1))
    lib.call("render_diffuse_light", 1, 2, 1, nd, ld, sv, e, 0.25, out.t)
    lib.call("render_diffuse_light_backward", 1, 2, 1, nd, ld, sv, e, 0.25, g, gn.t, gsv.t, ge.t)
    r = RR.diffuse_light(n, l, one, one.view(1, 2, 1), 0.25, torch.ones(1, 1))
    assert float(out.t) == 0.375 == float(r["out"])
    assert gn.t.cpu().tolist() == [[0.25, 0.25, 0.375]] == r["g_normal"].tolist(), "(l0 + l1) / 2: the light at the clamp passes its gradient"
    assert gsv.t.cpu().tolist() == [[0.125, 0.25]] == r["g_soft_vis"].tolist()


def test_a_dot_equal_to_eps_specular_and_direct(gpu):
    """raw n.l == eps (then n.v == eps, which masks every light of the ray: all outputs exactly 0): the mask is 0 (`>`, specular_brdf.dot), so the light at the clamp adds exactly nothing to the filament
    kernel, to one general instantiation (ue4, uniform, split) and to direct_light's specular integral, forward and backward
    (the gradient `>=` of these three kernels cannot be told from `>` at equality: the mask multiplies it); direct_light's diffuse
    integral passes the gradient as the diffuse kernel does.  All against the references, which use clamp(min) and `>`."""
    from ndjir_amd import lib
    n, v, l = _exact_lights(gpu)
    L = dict(normal=n, view=v, light=l, rough=torch.tensor([0.5]), spec=torch.tensor([[0.25, 0.5, 0.75]]), soft_vis=torch.ones(1, 2),
             env=torch.ones(1, 2, 1), g=torch.ones(1, 3))
    names = ("normal", "view", "light", "rough", "spec", "soft_vis", "env")
    dv = _dev(gpu, *[L[k] for k in names])
    for fwd, cfg, kw in (("render_specular_light_filament", (), dict(model=0, sampling=0, split=False)),
                         ("render_specular_light", (1, 1, 1), dict(model=1, sampling=1, split=True))):
        out = Out(gpu, 1, 3)
        lib.call(fwd, 1, 2, 1, *cfg, *dv, 0.25, 1.0, out.t)
        outs = [Out(gpu, 1, 3), Out(gpu, 1), Out(gpu, 1, 3), Out(gpu, 1, 2), Out(gpu, 1, 2, 1)]
        lib.call(fwd + "_backward", 1, 2, 1, *cfg, *dv, 0.25, 1.0, dv[0].new_ones(1, 3), *[o.t for o in outs])
        r64 = RR.specular_light(*[L[k] for k in names], 0.25, 1.0, g=L["g"], **kw)
        r32 = RR.specular_light(*[L[k] for k in names], 0.25, 1.0, g=L["g"], dtype=F32, **kw)
        _rho_check(f"specular_light[exact,{fwd}]", [out.t] + [o.t for o in outs], r64, r32, SPEC_OUT)
        one = RR.specular_light(n, v, l[:, 1:], L["rough"], L["spec"], torch.ones(1, 1), torch.ones(1, 1, 1), 0.25, 1.0, g=L["g"], **kw)
        if not kw["split"]:
            assert float(outs[3].t[0, 0]) == 0.0 and float(outs[4].t[0, 0, 0]) == 0.0, "the light at the clamp: masked"
            _within(f"specular_light[exact,{fwd}] without the masked light", out.t, one["out"] / 2, (2 + SPEC_C) * U * one["mag"] / 2)
    # the view at the clamp, n.v == eps: every light of the ray is masked
    Lv = dict(L, view=torch.tensor([[0.5, 0.0, 0.25]]))
    dvv = _dev(gpu, *[Lv[k] for k in names])
    out = Out(gpu, 1, 3)
    lib.call("render_specular_light_filament", 1, 2, 1, *dvv, 0.25, 1.0, out.t)
    outs = [Out(gpu, 1, 3), Out(gpu, 1), Out(gpu, 1, 3), Out(gpu, 1, 2), Out(gpu, 1, 2, 1)]
    lib.call("render_specular_light_filament_backward", 1, 2, 1, *dvv, 0.25, 1.0, dvv[0].new_ones(1, 3), *[o.t for o in outs])
    rv = RR.specular_light(*[Lv[k] for k in names], 0.25, 1.0, g=L["g"])
    assert float(rv["out"].abs().max()) == 0.0 and float(out.t.abs().max()) == 0.0 and all(float(o.t.abs().max()) == 0.0 for o in outs)
    dirs = torch.cat([l, l], dim=1)
    D = dict(normal=n, view=v, dirs=dirs, raw_sv=torch.ones(1, 4), raw_env=torch.ones(1, 4, 1),
             pix=torch.tensor([[0.5, 0.5, 0.25, 0.5, 0.75, 0.5, 0.25, 0.5, 0.75]]), g=torch.ones(1, 3))
    params = (1.0, 1.0, -1.0, 0.25, 1.0)
    dn = ("normal", "view", "dirs", "raw_sv", "raw_env", "pix")
    dd = _dev(gpu, *[D[k] for k in dn])
    color, envp, specp = Out(gpu, 1, 3), Out(gpu, 1, 1), Out(gpu, 1, 3)
    lib.call("render_direct_light", 1, 2, 1, [0, 0], list(params), 1, *dd, None, color.t, envp.t, specp.t)
    gouts = [Out(gpu, 1, 3), Out(gpu, 1, 4), Out(gpu, 1, 4, 1), Out(gpu, 1, 9)]
    lib.call("render_direct_light_backward", 1, 2, 1, [0, 0], list(params), 1, *dd, envp.t, specp.t, dd[0].new_ones(1, 3), *[o.t for o in gouts], None)
    r64 = RR.direct_light(*[D[k] for k in dn], None, (0, 0), params, True, D["g"])
    r32 = RR.direct_light(*[D[k] for k in dn], None, (0, 0), params, True, D["g"], dtype=F32)
    _rho_check("direct_light[exact]", [color.t, envp.t, specp.t], r64, r32, DIRECT_OUT)
    _rho_check("direct_light[exact]", [o.t for o in gouts], r64, r32, DIRECT_GRAD)
    assert float(envp.t) == 0.375, "identity activations: the diffuse integral is exact"
    assert float(gouts[1].t[0, 2]) == 0.0 and float(gouts[2].t[0, 2, 0]) == 0.0, "specular light at the clamp: masked"
    assert float(gouts[1].t[0, 0]) != 0.0, "diffuse light at the clamp: its value is eps"


def test_gain_exactly_at_a_bound(gpu):
    """exp(10 * 0) = 1 exactly: with lo = 1 and with hi = 1 the value sits on the bound and the clamp passes the gradient (bounds
    included): g e scale = 7 exactly.  (q exactly 0 in k_alpha_weights is left out: no representable input makes
    c0 sigmoid(-x1) expm1(...) equal -1e-5f; q exactly 1 is the planted opaque sample of the alpha tests.)"""
    from ndjir_amd import lib
    p, g = torch.zeros(1, device=gpu), torch.full((1,), 0.7, device=gpu)
    for lo, hi in ((1.0, 5e4), (1e-6, 1.0)):
        out, gp = Out(gpu, 1), Out(gpu, 1)
        lib.call("render_gain", 1, p, 10.0, lo, hi, out.t)
        lib.call("render_gain_backward", 1, p, 10.0, lo, hi, g, gp.t)
        assert float(out.t) == 1.0 and float(gp.t) == float(g * 10.0)
        _, _, gref = RR.gain(p, 10.0, lo, hi, g)
        assert float(gref) == pytest.approx(float(gp.t), rel=1e-7)


# ---- (g) degenerate calls ----------------------------------------------------------------------------------------------------------------
def test_zero_rays_touch_nothing(gpu):
    """R = 0 (N = 0 for the material head, n = 0 for the gain) returns before anything is looked at: every output stays NaN."""
    from ndjir_amd import lib
    o = [Out(gpu, 4) for _ in range(6)]
    t = torch.zeros(8, device=gpu)
    lib.call("render_alpha_weights", 0, 4, 0, t, t, t, t, t, t, t, None, o[0].t, o[1].t, o[2].t)
    lib.call("render_alpha_weights_backward", 0, 4, 0, t, t, t, t, t, t, t, None, t, None, None, t, o[0].t, o[1].t, o[2].t, None)
    lib.call("render_integrate", 0, 2, 2, t, 2, t, 2, o[0].t)
    lib.call("render_integrate_backward", 0, 2, 2, t, 2, t, 2, t, o[0].t, o[1].t, 2)
    lib.call("render_integrate_many", 0, 2, t, 1, [t], [2], [2], [2], [0], [o[0].t])
    lib.call("render_integrate_many_backward", 0, 2, t, 1, [t], [2], [2], [2], [0], [t], [o[0].t], o[1].t)
    lib.call("render_diffuse_light", 0, 2, 1, t, t, t, t, 0.25, o[0].t)
    lib.call("render_diffuse_light_backward", 0, 2, 1, t, t, t, t, 0.25, t, o[0].t, o[1].t, o[2].t)
    lib.call("render_specular_light_filament", 0, 2, 1, t, t, t, t, t, t, t, 0.25, 1.0, o[0].t)
    lib.call("render_specular_light_filament_backward", 0, 2, 1, t, t, t, t, t, t, t, 0.25, 1.0, t, *[x.t for x in o[:5]])
    lib.call("render_specular_light", 0, 2, 1, 1, 1, 1, t, t, t, t, t, t, t, 0.25, 1.0, o[0].t)
    lib.call("render_specular_light_backward", 0, 2, 1, 1, 1, 1, t, t, t, t, t, t, t, 0.25, 1.0, t, *[x.t for x in o[:5]])
    lib.call("render_direct_light", 0, 1, 1, [0, 0], [1.0, 1.0, -1.0, 0.25, 1.0], 1, t, t, t, t, t, t, None, o[0].t, o[1].t, o[2].t)
    lib.call("render_direct_light_backward", 0, 1, 1, [0, 0], [1.0, 1.0, -1.0, 0.25, 1.0], 1, t, t, t, t, t, t, t, t, t, *[x.t for x in o[:4]], None)
    lib.call("render_material_head", 0, 1, t, t, t, t, t, t, t, 1, 1, 1, 0.1, 0.16, 0.5, 0.04, o[0].t, o[1].t, o[2].t)
    lib.call("render_material_head", 1, 0, t, t, t, t, t, t, t, 1, 1, 1, 0.1, 0.16, 0.5, 0.04, o[0].t, o[1].t, o[2].t)
    lib.call("render_material_head_backward", 0, 1, t, t, t, t, t, t, t, 1, 1, 1, 0.1, 0.16, 0.5, 0.04, t, t, *[x.t for x in o])
    lib.call("render_gain", 0, t, 10.0, 1e-6, 5e4, o[0].t)
    lib.call("render_gain_backward", 0, t, 10.0, 1e-6, 5e4, t, o[0].t)
    torch.cuda.synchronize()
    assert all(x.untouched() for x in o)


def test_integrate_without_samples_writes_zeros(gpu):
    """S = 0: the integral of nothing is 0 in every channel; the backward has nothing to write."""
    from ndjir_amd import lib
    R, C = 3, 5
    t = torch.zeros(8, device=gpu)
    out, gx, gw = Out(gpu, R, C), Out(gpu, 4), Out(gpu, 4)
    lib.call("render_integrate", R, 0, C, t, 0, t, C, out.t)
    lib.call("render_integrate_backward", R, 0, C, t, 0, t, C, t, gx.t, gw.t, 0)
    assert out.guards_ok() and float(out.t.abs().max()) == 0.0 and not bool(torch.isnan(out.t).any())
    assert gx.untouched() and gw.untouched()


def test_null_required_pointers_raise(gpu):
    """A missing required tensor is a status before any launch: nothing is written."""
    from ndjir_amd import lib
    t = torch.zeros(64, device=gpu)
    o = [Out(gpu, 8) for _ in range(6)]
    calls = [
        ("render_alpha_weights", (1, 4, 0, t, t, t, t, t, t, None, None, o[0].t, o[1].t, o[2].t)),
        ("render_alpha_weights", (1, 4, 1, t, t, t, t, t, t, t, None, o[0].t, o[1].t, o[2].t)),              # Nb > 0 without alpha_bg
        ("render_alpha_weights_backward", (1, 4, 0, t, t, t, t, t, t, t, None, None, None, None, t, o[0].t, o[1].t, o[2].t, None)),   # no trans
        ("render_integrate", (1, 2, 2, None, 2, t, 2, o[0].t)),
        ("render_integrate", (1, 2, 2, t, 2, t, 1, o[0].t)),                                                # ldx < C
        ("render_integrate_backward", (1, 2, 2, t, 2, t, 2, None, o[0].t, o[1].t, 2)),
        ("render_integrate_backward", (1, 2, 2, t, 2, t, 2, t, o[0].t, o[1].t, 1)),                         # ldgw < S
        ("render_integrate_many", (1, 2, None, 1, [t], [2], [2], [2], [0], [o[0].t])),
        ("render_integrate_many", (1, 2, t, 1, [t], [2], [2], [2], [0], [None])),
        ("render_integrate_many", (1, 2, t, 1, [t], [1], [2], [2], [0], [o[0].t])),                          # ld < C
        ("render_diffuse_light", (1, 2, 4, t, t, t, t, 0.25, o[0].t)),                                       # C > 3
        ("render_diffuse_light", (1, 2, 1, t, None, t, t, 0.25, o[0].t)),
        ("render_diffuse_light_backward", (1, 2, 1, t, t, t, t, 0.25, None, o[0].t, o[1].t, o[2].t)),
        ("render_specular_light_filament", (1, 2, 2, t, t, t, t, t, t, t, 0.25, 1.0, o[0].t)),               # C = 2
        ("render_specular_light", (1, 2, 1, 2, 0, 0, t, t, t, t, t, t, t, 0.25, 1.0, o[0].t)),               # model 2
        ("render_specular_light_backward", (1, 2, 1, 0, 0, 0, t, t, t, t, t, t, t, 0.25, 1.0, None, *[x.t for x in o[:5]])),
        ("render_direct_light", (1, 1, 1, [0, 4], [1.0, 1.0, -1.0, 0.25, 1.0], 1, t, t, t, t, t, t, None, o[0].t, o[1].t, o[2].t)),     # activation 4
        ("render_direct_light", (1, 0, 1, [0, 0], [1.0, 1.0, -1.0, 0.25, 1.0], 1, t, t, t, t, t, t, None, o[0].t, o[1].t, o[2].t)),     # M = 0
        ("render_direct_light_backward", (1, 1, 1, [0, 0], [1.0, 1.0, -1.0, 0.25, 1.0], 1, t, t, t, t, t, t, t, t, None, *[x.t for x in o[:4]], None)),
        ("render_material_head", (1, 1, t, t, t, t, None, t, t, 1, 1, 1, 0.1, 0.16, 0.5, 0.04, o[0].t, o[1].t, o[2].t)),
        ("render_material_head_backward", (1, 1, t, t, t, t, t, t, t, 1, 1, 1, 0.1, 0.16, 0.5, 0.04, None, t, *[x.t for x in o])),
        ("render_gain", (1, None, 10.0, 1e-6, 5e4, o[0].t)),
        ("render_gain_backward", (1, t, 10.0, 1e-6, 5e4, None, o[0].t)),
    ]
    for name, args in calls:
        with pytest.raises(RuntimeError):
            lib.call(name, *args)
    torch.cuda.synchronize()
    assert all(x.untouched() for x in o)
