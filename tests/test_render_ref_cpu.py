"""CPU checks of tests/render_ref.py, the references of tests/test_gpu_rays.py: each reference against an independent fp64
spelling of the same operation (the stock-op composites of tests/test_gpu_render.py, ndjir_amd.specular_brdf in fp64) to 1e-9,
values and gradients; each input builder at the shapes of the GPU tests -- no kink argument inside the margin; and, from the host
code's launch geometry as integer arithmetic, that each shape enters the path it is meant for and that the walks cover every
output once (a guard of the test inputs, not a test of the kernels)."""
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn.functional as TF

from tests import render_ref as RR

F64 = torch.float64
EPS = 2.0 ** -20                     # an eps_dot that is the same number in fp32 and fp64


def _close(a, b, tol=1e-9):
    a, b = a.detach().to(F64), b.detach().to(F64).reshape(a.shape)
    scale = float(b.abs().max()) if b.numel() else 0.0
    assert float((a - b).abs().max()) <= tol * max(scale, 1e-300), (float((a - b).abs().max()), scale)


# ---- the references against independent spellings ---------------------------------------------------------------------------------
def test_alpha_weights_reference_matches_the_composite(monkeypatch):
    from tests.test_gpu_render import composite_alpha_weights
    monkeypatch.setattr(RR, "E5", 1e-5)                      # the composite's constant (the kernels' is the fp32 1e-5)
    R, N, Nb = 5, 40, 7
    b = RR.build_alpha(R, N, Nb, 3)
    ins = [b["sdf"].double()[None, :, :, None], b["n"].double()[None], b["raydir"].double()[None], b["t"].double()[None, :, :, None],
           b["gain"].double(), b["car"].double(), b["mask"].double()[None, :, None, None], b["alpha_bg"].double()[None, :, :, None]]
    req = (0, 1, 4, 7)
    leaves = [t.clone().requires_grad_(i in req) for i, t in enumerate(ins)]
    a, tr, w = composite_alpha_weights(*leaves)
    alpha, _ = RR.alpha_fg(b["sdf"], b["n"], b["raydir"], b["t"], b["gain"], b["car"])
    _close(alpha, a)
    trans, weights = RR.scan(torch.cat([alpha * b["mask"].double()[:, None], b["alpha_bg"].double()], dim=1))
    _close(trans, tr)
    _close(weights, w)
    g = torch.Generator().manual_seed(1)
    gs = [torch.randn(o.shape, generator=g, dtype=F64) for o in (a, tr, w)]
    for use in ((0,), (1,), (2,), (0, 1, 2)):
        gref = torch.autograd.grad([(a, tr, w)[k] for k in use], [leaves[i] for i in req], [gs[k] for k in use], retain_graph=True,
                                   allow_unused=True)
        opt = lambda k: gs[k][0, :, :, 0] if k in use else None
        r = RR.alpha_weights_backward(b["sdf"], b["n"], b["raydir"], b["t"], b["gain"], b["car"], b["mask"], b["alpha_bg"], alpha,
                                      opt(0), opt(1), opt(2))
        _close(r["g_sdf"], gref[0])
        _close(r["g_n"], gref[1])
        _close(r["g_gain_ray"].sum().reshape(1), gref[2])
        if gref[3] is not None:
            _close(r["g_alpha_bg"], gref[3])
        else:
            assert float(r["g_alpha_bg"].abs().max()) == 0.0
        # the magnitudes bound the values they belong to
        assert bool((r["g_sdf"].abs() <= r["mag_sdf"] * (1 + 1e-9) + 1e-300).all())
        assert bool((r["g_alpha_bg"].abs() <= r["mag_bg"] * (1 + 1e-9) + 1e-300).all())
        assert bool((r["g_gain_ray"].abs() <= r["mag_gain"].sum(1) * (1 + 1e-9) + 1e-300).all())


def test_integrate_references_match_einsum():
    g = torch.Generator().manual_seed(2)
    w, x, go = torch.rand(4, 9, generator=g), torch.randn(4, 9, 13, generator=g), torch.randn(4, 13, generator=g)
    out, mag, T = RR.integrate(w, x)
    _close(out, torch.einsum("rs,rsc->rc", w.double(), x.double()))
    assert T == 9 and bool((out.abs() <= mag).all())
    gx, gw, gmag, Tc = RR.integrate_backward(w, x, go)
    wl, xl = w.double().requires_grad_(True), x.double().requires_grad_(True)
    rw, rx = torch.autograd.grad(torch.einsum("rs,rsc->rc", wl, xl), [wl, xl], go.double())
    _close(gx, rx)
    _close(gw, rw)
    assert Tc == 13
    x2 = torch.randn(4, 4, 5, generator=g)
    g2 = torch.randn(4, 5, generator=g)
    gxs, gwm, magm, Tm = RR.integrate_many_backward(w, [x, x2, x2], [0, 2, 5], [go, None, g2])
    want = rw.clone()
    want[:, 5:9] += torch.einsum("rsc,rc->rs", x2.double(), g2.double())
    _close(gwm, want)
    assert gxs[1] is None and Tm.tolist() == [13] * 5 + [18] * 4


def _conf(model, sampling):
    return NS(renderer=NS(eps_dot=EPS), specular_brdf=NS(sampling=("importance", "uniform")[sampling], model=("filament", "ue4")[model]))


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("sampling", [0, 1])
@pytest.mark.parametrize("model", [0, 1])
def test_specular_reference_matches_specular_brdf(model, sampling, split):
    from ndjir_amd.specular_brdf import specular_brdf_model
    R, M, C, weight = 4, 21, 3, 1.25
    L = RR.build_lights(R, M, C, 5, EPS)
    names = ("normal", "view", "light", "rough", "spec", "soft_vis", "env")
    a = [L[k].double().requires_grad_(k not in ("view", "light")) for k in names]

    def composite(n, v, l, r, s, sv, e):
        sB, cos = specular_brdf_model(n[None], v[None, :, None, :], l[None], r[None, :, None], s[None], _conf(model, sampling))
        if split:
            return (weight * (sv[None, ..., None] * e[None]).mean(dim=2) * (sB * cos).mean(dim=2))[0]
        return (weight * (sB * sv[None, ..., None] * e[None] * cos).mean(dim=2))[0]

    ref = composite(*a)
    gref = torch.autograd.grad(ref, [a[i] for i in (0, 3, 4, 5, 6)], L["g"].double())
    r = RR.specular_light(*[L[k] for k in names], EPS, weight, model, sampling, split, L["g"])
    _close(r["out"], ref)
    for k, gr in zip(("g_normal", "g_rough", "g_spec", "g_soft_vis", "g_env"), gref):
        _close(r[k], gr)
    assert bool((r["out"].abs() <= r["mag"] * (1 + 1e-12)).all()) and bool((r["g_normal"].abs() <= r["mag_normal"] * (1 + 1e-12)).all())


def test_diffuse_reference_matches_dot():
    from ndjir_amd.specular_brdf import dot
    R, M, C = 4, 21, 3
    L = RR.build_lights(R, M, C, 6, EPS)
    n, sv, e = (L[k].double().requires_grad_(True) for k in ("normal", "soft_vis", "env"))
    ref = (sv[..., None] * e * dot(n[:, None, :].expand(R, M, 3), L["light"].double(), False, EPS)).mean(dim=1)
    gref = torch.autograd.grad(ref, [n, sv, e], L["g"].double())
    r = RR.diffuse_light(L["normal"], L["light"], L["soft_vis"], L["env"], EPS, L["g"])
    _close(r["out"], ref)
    for k, gr in zip(("g_normal", "g_soft_vis", "g_env"), gref):
        _close(r[k], gr)
        assert bool((r[k].abs() <= r["mag" + k[1:]] * (1 + 1e-12)).all())


@pytest.mark.parametrize("acts,ub,entangle,with_bg,C", [((2, 1), -1.0, True, True, 1), ((2, 1), 0.8, False, True, 3),
                                                        ((1, 3), -1.0, True, False, 1), ((3, 2), 0.6, True, True, 3), ((0, 0), 0.7, False, False, 3)])
def test_direct_light_reference_matches_the_separate_spellings(acts, ub, entangle, with_bg, C):
    from ndjir_amd.specular_brdf import dot, filament_specular_brdf
    R, M, betas, weight = 3, 17, (1.7, 0.6), 0.7
    D = RR.build_direct(R, M, C, 7, acts, betas, ub, EPS, with_bg)
    act = {0: lambda v, b: v, 1: lambda v, b: TF.softplus(v, beta=b), 2: lambda v, b: torch.sigmoid(v), 3: lambda v, b: torch.relu(v)}
    view, dirs = D["view"].double(), D["dirs"].double()
    ins = [D[k].double().requires_grad_(True) for k in ("normal", "raw_sv", "raw_env", "pix")] + ([D["bg"].double().requires_grad_(True)] if with_bg else [])

    def composite(n, rsv, renv, px, bgv=None):
        sv, env = act[acts[0]](rsv, RR.f32(betas[0]))[None, ..., None], act[acts[1]](renv, RR.f32(betas[1]))[None]
        if ub > 0:
            env = env.clamp(0.0, RR.f32(ub))
        l_d, l_s = dirs[None, :, :M], dirs[None, :, M:]
        env_pixel = (sv[:, :, :M] * env[:, :, :M] * dot(n[None, :, None, :].expand(1, R, M, 3), l_d, False, EPS)).mean(dim=2)
        sB, cos = filament_specular_brdf(n[None], view[None, :, None, :], l_s, px[None, :, 1:2], px[None, :, 2:5], _conf(0, 0))
        spec = RR.f32(weight) * (sB * sv[:, :, M:] * env[:, :, M:] * cos).mean(dim=2)
        imp, photo, base = px[None, :, 0:1], px[None, :, 5:6], px[None, :, 6:9]
        diff = env_pixel + imp
        fg = base * diff + photo * spec if entangle else photo * (base * diff + spec)
        return (fg + bgv[None] if bgv is not None else fg)[0], env_pixel[0], spec[0]

    color, env_pixel, spec = composite(*ins)
    gref = torch.autograd.grad(color, ins, D["g"].double())
    r = RR.direct_light(D["normal"], D["view"], D["dirs"], D["raw_sv"], D["raw_env"], D["pix"], D["bg"], acts,
                        (betas[0], betas[1], ub, EPS, weight), entangle, D["g"])
    _close(r["color"], color)
    _close(r["env_pix"], env_pixel)
    _close(r["spec_pix"], spec)
    for k, gr in zip(("g_normal", "g_raw_sv", "g_raw_env", "g_pix", "g_bg"), gref):
        _close(r[k], gr)
    assert float(r["g_pix"][:, 1:5].abs().max()) > 0


def _composite_material(raws, gain, cfg):
    """The stock-op formulas of python/network.py / python/loss.py as tests/test_gpu_render.py spells them, per ray."""
    remap, entangle, sym, lb, scale, pr, ps = cfg
    bc_r, pt_r, imp_r, ph_r, ro_r, sp_r = raws
    bc, pt = torch.sigmoid(bc_r), torch.sigmoid(pt_r)
    imp, photo = torch.sigmoid(imp_r), torch.sigmoid(gain * ph_r)
    r = torch.sigmoid(ro_r[..., 0:1])
    r = (r ** 2 if remap else r).clamp(lb, 1.0)
    std_r = TF.softplus(ro_r[..., 1:2])
    s = torch.sigmoid(sp_r[..., :3])
    s = 0.16 * s ** 2 if remap else scale * s
    std_s = TF.softplus(sp_r[..., 3:])
    V = torch.cat([imp, r, s, photo, bc * photo if entangle else bc], dim=-1)
    bcp = bc if sym else bc.detach()
    prior = torch.stack([(bcp - pt).abs().sum(-1).sum(-1), ((r - pr).abs() / std_r).sum(-1).sum(-1),
                         torch.log(std_r).clamp(1e-5, 1e5).sum(-1).sum(-1), ((s - ps).abs() / std_s).sum(-1).sum(-1),
                         torch.log(std_s).clamp(1e-5, 1e5).sum(-1).sum(-1)], dim=-1)
    return V, torch.cat([bc, pt, std_r, std_s], dim=-1), prior


MAT_CFGS = [(r, e, s, 0.089, 0.16, 0.5, 0.04) for r in (0, 1) for e in (0, 1) for s in (0, 1)]


@pytest.mark.parametrize("cfg", MAT_CFGS)
def test_material_reference_matches_the_composite(cfg):
    raws, pg, gV, gp = RR.build_material(3, 11, 8, cfg)
    c64 = tuple(cfg[:3]) + tuple(RR.f32(c) for c in cfg[3:])
    leaves = [t.double().requires_grad_(True) for t in raws]
    V, aux, prior = _composite_material(leaves, pg.double(), c64)
    r = RR.material_head(raws, pg, cfg, gV, gp)
    _close(r["V"], V)
    _close(r["aux"], aux)
    for k in range(5):
        _close(r["prior"][:, k], prior[:, k])
    assert r["T_prior"].tolist() == [33, 11, 11, 33, 33]
    gref = torch.autograd.grad([V, prior], leaves, [gV.double(), gp.double()], retain_graph=True)
    for a, b, m in zip(r["grads"], gref, r["mags"]):
        _close(a, b)
        assert bool((a.abs() <= m * (1 + 1e-12)).all())
    r2 = RR.material_head(raws, pg, cfg, gV, None)
    for a, b in zip(r2["grads"], torch.autograd.grad(V, leaves, gV.double(), allow_unused=True)):
        _close(a, b if b is not None else torch.zeros_like(a))


def test_gain_reference():
    p = torch.tensor([0.3, -2.0, 1.2])
    out, e, gp = RR.gain(p, 10.0, 1e-6, 5e4, torch.tensor([0.7, 0.7, 0.7]))
    pl = p.double().requires_grad_(True)
    ref = torch.exp(pl * 10.0).clamp(RR.f32(1e-6), RR.f32(5e4))
    _close(out, ref)
    _close(gp, torch.autograd.grad(ref, pl, torch.full((3,), RR.f32(0.7), dtype=F64))[0])
    assert float(gp[1]) == 0.0 and float(gp[2]) == 0.0


# ---- the strictness of the clamped dots ----------------------------------------------------------------------------------------------
def test_a_dot_equal_to_eps_passes_the_gradient_and_fails_the_mask():
    """raw == eps exactly (eps_dot = 0.25, n = (0, 0, 1), z = 0.25): `specular_brdf.dot` has the mask 0 (`>`), torch's
    clamp(min) passes the gradient (`>=`); the reference here does the same."""
    from ndjir_amd.specular_brdf import dot
    n = torch.tensor([[0.0, 0.0, 1.0]], dtype=F64, requires_grad=True)
    l = torch.tensor([[0.5, 0.0, 0.25]], dtype=F64)                # not unit length: every number exact
    uv, mask = dot(n, l, True, 0.25)
    assert float(uv.detach()) == 0.25 and float(mask) == 0.0
    (g,) = torch.autograd.grad(uv.sum(), n)
    assert g.tolist() == [[0.5, 0.0, 0.25]]
    r = RR.diffuse_light(n.detach().float(), l.float()[:, None, :], torch.ones(1, 1), torch.ones(1, 1, 1), 0.25, torch.ones(1, 1))
    assert r["g_normal"].tolist() == [[0.5, 0.0, 0.25]] and float(r["out"]) == 0.25
    q = torch.tensor([0.0, 1.0], dtype=F64, requires_grad=True)                         # clamp(q, 0, 1) at either bound: passes
    assert torch.autograd.grad(q.clamp(0.0, 1.0).sum(), q)[0].tolist() == [1.0, 1.0]


# ---- the builders keep every kink outside the margin ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Nb", RR.ALPHA_SHAPES)
def test_alpha_builder_margin(N, Nb):
    for R in RR.RAYS:
        b = RR.build_alpha(R, N, Nb, 100 + N)
        dist = RR.alpha_kink_distance(b["sdf"], b["n"], b["raydir"], b["t"], b["gain"], b["car"])
        assert bool((dist[~b["exact"]] >= 1.0).all())
        alpha, count = RR.alpha_fg(b["sdf"], b["n"], b["raydir"], b["t"], b["gain"], b["car"])
        assert bool(torch.isfinite(count).all())
        assert float((b["gain"] * b["sdf"]).abs()[~b["exact"]].max()) <= 16.0
        if N >= 8:
            assert float(alpha[0, 3]) == 1.0 and bool(b["exact"][0, 3]), "the planted opaque sample is exactly 1 in fp64 too"
            assert bool((alpha[R - 1] == 0.0).any()), "an unsorted t clamps q < 0"
        if Nb:
            assert float(b["alpha_bg"][R - 1, 0]) == 1.0
        assert set(b["mask"].tolist()) <= {0.0, 0.25, 1.0}


@pytest.mark.parametrize("M", RR.LIGHT_M)
def test_light_builders_margin(M):
    for C in (1, 3):
        for R in RR.RAYS:
            L = RR.build_lights(R, M, C, 200 + M)
            assert bool((RR.light_kink_distance(L["normal"], L["view"], L["light"], L["eps"]) >= 1.0).all())
            if M > 3:
                below = ((L["normal"][:, None, :] * L["light"]).sum(-1) < 0).sum(1)
                assert bool((below >= 1).all()), "lights under the surface: the masks are used"
    for acts, ub in (((2, 1), -1.0), ((1, 3), 0.8), ((3, 2), 0.6), ((0, 0), 0.7)):
        D = RR.build_direct(3, M, 3, 300 + M, acts, (1.7, 0.5), ub)
        assert bool((RR.light_kink_distance(D["normal"], D["view"], D["dirs"], 1e-8) >= 1.0).all())
        assert bool((RR.act_kink_distance(acts[1], 0.5, ub, D["raw_env"]) >= 1.0).all())
        assert bool((RR.act_kink_distance(acts[0], 1.7, -1.0, D["raw_sv"]) >= 1.0).all())
    D = RR.build_direct(3, M, 1, 400 + M, (1, 1), (0.5, 0.5), -1.0)
    if M >= 2:
        assert (D["raw_sv"].view(-1)[:3] * 0.5).tolist() == [19.5, 20.0, 20.5], "beta v = 19.5, 20, 20.5 exactly"


@pytest.mark.parametrize("N", RR.MATERIAL_N)
def test_material_builder_margin(N):
    for cfg in MAT_CFGS[::3]:
        for R in RR.RAYS:
            raws, pg, _, _ = RR.build_material(R, N, 500 + N, cfg)
            assert bool((RR.material_kink_distance(raws, pg, cfg) >= 1.0).all())
            assert float(raws[4].view(-1, 2)[0, 1]) == 19.5


# ---- the shapes enter the paths they are meant for -----------------------------------------------------------------------------------
def test_alpha_shapes_against_the_slots():
    S = [n + nb for n, nb in RR.ALPHA_SHAPES]
    assert max(S) == RR.RD_SLOTS and {(s + 63) // 64 for s in S} >= {1, 2, 4, 8}
    assert any(nb == 0 for _, nb in RR.ALPHA_SHAPES) and 481 + 32 > RR.RD_SLOTS


def test_integrate_shapes_take_their_paths():
    g = {sc: RR.integrate_geometry(sc[1]) for sc in RR.INTEGRATE_SHAPES}
    assert g[(9, 256)][:2] == (256, 1) and g[(9, 257)] == (256, 1, 2) and g[(9, 300)] == (256, 1, 2), "TY == 1: no tree reduction"
    assert g[(300, 1)][:2] == (1, 256) and 300 > 256, "TY = 256 and a second sample trip"
    assert g[(33, 6)][:2] == (8, 32) and g[(130, 65)][:2] == (128, 2)
    b = {sc: RR.integrate_bwd_geometry(*sc) for sc in RR.INTEGRATE_SHAPES}
    assert b[(7, 4)][0] == "thread" and b[(7, 5)][0] == "wave", "C = 4 / 5: thread per sample / wave per sample"
    assert b[(130, 64)][1] == 1 and b[(130, 65)][1] == 2, "C = 64 / 65: the second lane trip"
    assert b[(300, 1)] == ("thread", 1, 2) and b[(130, 64)][2] == 33


def test_integrate_many_forward_geometry():
    ny, segs = RR.integrate_many_geometry(RR.MANY_FWD["widths"])
    assert ny == 8, "the cap of 8"
    for C, (TX, TY, chunks) in zip(RR.MANY_FWD["widths"], segs):
        assert TX <= 64 and TX * TY == 256
        covered = sorted(c for _, _, c0 in chunks for c in range(c0, min(c0 + TX, C)))
        assert covered == list(range(C)), "every channel once"
    TX, _, chunks = segs[4]
    assert RR.rd_pow2(520) == 256 and TX == 64, "the TX cap"
    assert any(y > 0 for y, _, _ in chunks) and any(trip == 1 for _, trip, _ in chunks), "blockIdx.y > 0 and a second c0 trip"
    assert (0, 1, 512) in chunks
    assert RR.integrate_many_geometry((3, 3, 20, 9, 3))[0] == 1, "the earlier test's widths: one workgroup row, one chunk"


def test_integrate_many_backward_geometry():
    for case in RR.MANY_BWD + (RR.MANY_ONE_RAY, RR.MANY_STRIDE):
        ny, owners = RR.integrate_many_bwd_geometry(case["R"], case["S_all"])
        assert sorted(owners) == list(range(case["S_all"])) and all(len(o) == 1 for o in owners.values()), "every position once"
    assert len(RR.MANY_BWD[0]["widths"]) == RR.IM_SEGS
    assert RR.integrate_many_bwd_geometry(2, 9)[0] == 3
    ny, owners = RR.integrate_many_bwd_geometry(1, 40)
    assert ny == 10 and all(o[0][2] == 0 for o in owners.values()), "many y, one position each"
    ny, owners = RR.integrate_many_bwd_geometry(5000, 9)
    assert ny == 1 and max(o[0][2] for o in owners.values()) == 2, "ny = 1: the stride walk, three trips"
    c = RR.MANY_STRIDE
    assert c["R"] * c["S_all"] * max(c["lds"]) * 4 <= 2e6, "the largest array: under 2 MB"
    assert RR.vec_trips(520) == ("v4", 3) and RR.vec_trips(260) == ("v4", 2) and RR.vec_trips(256) == ("v4", 1)
    assert RR.vec_trips(258) == ("scalar", 5) and RR.vec_trips(65) == ("scalar", 2) and RR.vec_trips(20) == ("v4", 1)
    for case in RR.MANY_BWD:                                # x rows at every float offset 0..3 (base offsets k = segment index)
        offs = {(k + i * ld) % 4 for k, (C, ld) in enumerate(zip(case["widths"], case["lds"])) if C % 4 == 0 for i in range(case["S_all"])}
        assert offs == {0, 1, 2, 3}


def test_light_and_material_shapes_fill_both_waves_and_take_a_second_pass():
    for sizes, threads in ((RR.LIGHT_M, RR.SH_THREADS), (RR.MATERIAL_N, RR.MH_THREADS)):
        fill = {m: RR.wave_fill(m, threads) for m in sizes}
        assert any(second == 0 and passes == 1 for _, second, passes in fill.values()), "second wave empty"
        if sizes is RR.LIGHT_M:
            assert any(second == 1 for _, second, _ in fill.values()), "second wave holds one light"
        assert any(second == 64 and passes == 1 for _, second, passes in fill.values()), "both waves full, one pass"
        assert any(passes == 2 and first == 65 and second == 64 for first, second, passes in fill.values()), "second pass: one item, first wave"
        assert any(passes >= 3 and second > 64 for _, second, passes in fill.values()), "a third, ragged pass with both waves"
    assert RR.wave_fill(37) == (37, 0, 1), "the earlier tests' M: the second wave adds zeros"


@pytest.mark.parametrize("N,Nb", [(65, 0), (480, 32)])
def test_alpha_bound_against_the_fp32_spelling(N, Nb):
    """Plain fp32 arithmetic on `alpha_terms`' formula (no GPU) breaks (2 |x1| + 15) u |alpha| -- it leaves out what iter_cos and the
    sample's length add to x1 -- and keeps the bound of `alpha_roundings`: the bound follows the formula, not a kernel."""
    b = RR.build_alpha(130, N, Nb, 100 + N)
    args = [b[k] for k in ("sdf", "n", "raydir", "t", "gain", "car")]
    a32 = RR.alpha_fp32_spelling(*args).double()
    ref, count = RR.alpha_fg(*args)
    p = RR.alpha_parts(*[RR.up(x) for x in args[:4]], RR.up(args[4]).reshape(()), RR.up(args[5]).reshape(()))
    err = (a32 - ref).abs()
    ratio = lambda bound: float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
    old, new = ratio((2 * p["x1"].abs() + 15) * RR.U * ref.abs()), ratio(count * RR.U * ref.abs())
    print(f"fp32 spelling of alpha at 130 x ({N}, {Nb}): {old:.3g} of (2 |x1| + 15) u, {new:.3g} of alpha_roundings")
    assert old > 1.0 and new <= 1.0, (old, new)
